"""Plain NumPy restatement of the pipe-geometry fit (include/rtus.h: rtus_echo_pick, rtus_geom_misfit; api.pipe_misfit, api.fit_pipe):
the echo pick, the misfit sums and the Levenberg-Marquardt loop.  Model times come from the CPU oracle (oracle/cport.solve, the C
port of the reference's trace with a root-finding matcher); nothing here touches the GPU.  The oracle of tests/test_geomfit_cpu.py
and tests/test_gpu_geomfit.py."""
import numpy as np

import pipe_numpy as P

FIT_STEP = (2e-5, 2e-5)          # central-difference half steps in (r_outer, pipe_offset) [m]
FIT_TOL = 1e-10                  # stop when both components of the step are below this [m]


# ------------------------------------------------------------------------------------------------ pick
def magnitude(a):
    """|a| the way the header forms it: fp32, every operation rounded on its own"""
    a = np.asarray(a)
    re, im = a.real.astype(np.float32), a.imag.astype(np.float32)
    with np.errstate(all="ignore"):
        return np.sqrt(re * re + im * im)                  # float32 throughout


def gate(t_lo, t_hi, t0, fs, n_t):
    """-> (i_lo, i_hi) or None when the gate holds no sample of the record"""
    with np.errstate(all="ignore"):
        lo = np.ceil((np.float64(t_lo) - np.float64(t0)) * np.float64(fs))
        hi = np.floor((np.float64(t_hi) - np.float64(t0)) * np.float64(fs))
    if np.isnan(lo) or np.isnan(hi):
        return None
    lo, hi = max(lo, 0.0), min(hi, float(n_t - 1))
    return (int(lo), int(hi)) if lo <= hi else None


def pick(a, fs, t_lo, t_hi, t0=0.0):
    """a complex [n_tx, n_rx, n_t]; t_lo / t_hi scalars or [n_tx, n_rx] -> (t_pick float64, amp float32) [n_tx, n_rx]"""
    a = np.asarray(a)
    n_tx, n_rx, n_t = a.shape
    lo_all, hi_all = np.broadcast_to(np.asarray(t_lo, dtype=np.float64), (n_tx, n_rx)), np.broadcast_to(
        np.asarray(t_hi, dtype=np.float64), (n_tx, n_rx))
    t = np.full((n_tx, n_rx), np.nan)
    amp = np.full((n_tx, n_rx), np.nan, dtype=np.float32)
    fs, t0 = np.float64(fs), np.float64(t0)
    for i in range(n_tx):
        m_all = magnitude(a[i])
        for j in range(n_rx):
            g = gate(lo_all[i, j], hi_all[i, j], t0, fs, n_t)
            if g is None:
                continue
            i_lo, i_hi = g
            m = m_all[j, i_lo:i_hi + 1]
            if not np.isfinite(m).all():
                continue                                    # amp NaN, no pick
            k = int(np.argmax(m))                           # the first index of the maximum
            amp[i, j] = m[k]
            if k == 0 or k == m.size - 1 or not m[k] > 0:
                continue
            am, a0, ap = np.float64(m[k - 1]), np.float64(m[k]), np.float64(m[k + 1])
            d = (am - ap) / (2.0 * (am - 2.0 * a0 + ap))
            d = min(max(d, -0.5), 0.5)
            t[i, j] = t0 + (np.float64(i_lo + k) + d) / fs
    return t, amp


def valid(t, amp, threshold=0.1):
    fin = np.isfinite(amp)
    top = amp[fin].max() if fin.any() else np.nan
    with np.errstate(invalid="ignore"):
        return np.isfinite(t) & fin & (amp >= threshold * top)


# ------------------------------------------------------------------------------------------------ misfit
def misfit(tt, t_meas, w=None):
    """-> (n, sse, sum_r, sum_w) [G] in the header's order: receive elements ascending within a row, then the rows ascending
    (np.cumsum adds in sequence; a pair that does not count adds an exact zero).  sse without the kernel's fused multiply-add."""
    tt, tm = np.asarray(tt, dtype=np.float64), np.asarray(t_meas, dtype=np.float64)
    wt = np.ones_like(tm) if w is None else np.asarray(w, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        d = tt - tm[None]
        use = np.isfinite(d) & (wt > 0)[None]
    d = np.where(use, d, 0.0)
    wu = np.where(use, wt[None], 0.0)
    wd = wu * d
    rows = lambda v: np.cumsum(np.cumsum(v, axis=2)[:, :, -1], axis=1)[:, -1]      # noqa: E731
    return use.sum(axis=(1, 2)).astype(np.int32), rows(wd * d), rows(wd), rows(wu)


def stats(n, sse, sr, sw, fit_delay=False):
    """(mse, delay) per geometry"""
    with np.errstate(all="ignore"):
        if fit_delay:
            return np.where(n > 0, np.maximum(sse - sr * sr / sw, 0.0) / n, np.nan), np.where(n > 0, -sr / sw, np.nan)
        return np.where(n > 0, sse / n, np.nan), np.where(n > 0, 0.0, np.nan)


# ------------------------------------------------------------------------------------------------ model times
def model_times(x_a, z_a, x_rx, alpha, geoms, z_land=P.D):
    """tt [G, T, E] from the CPU oracle: least pulse-echo time tx -> lens -> pipe -> lens -> rx, NaN without a path"""
    from oracle import cport
    geoms = np.atleast_2d(np.asarray(geoms, dtype=np.float64))
    x_a, z_a = np.atleast_1d(x_a), np.atleast_1d(z_a)
    tt = np.empty((geoms.shape[0], x_a.size, np.size(x_rx)))
    for g, (r, off) in enumerate(geoms):
        for t in range(x_a.size):
            tt[g, t] = cport.solve(x_a[t], z_a[t], z_land, alpha, x_rx, float(r), float(off))[0]
    return tt


def clearance(x_off):
    return P.clearance(P.Lens(), x_off, n=20001)


# ------------------------------------------------------------------------------------------------ the fit
def _step(JtJ, Jtr, lam):
    return -np.linalg.solve(JtJ + lam * np.diag(np.diag(JtJ)), Jtr)


def fit(model, t_meas, radii, offsets, *, min_pairs=8, fit_delay=False, w=None, max_iter=40):
    """model(geoms [G, 2]) -> tt [G, T, E].  The coarse map, then Levenberg-Marquardt from the best node: five geometries an
    iteration, central differences over the pairs finite at all five; a centre that costs more, has too few pairs or touches the lens
    is taken back with ten times the damping; stop when the step is below FIT_TOL.  -> dict as api.fit_pipe's."""
    tm = np.asarray(t_meas, dtype=np.float64)
    wt_all = np.ones_like(tm) if w is None else np.asarray(w, dtype=np.float64)
    dr, dx = FIT_STEP
    n_par = 3 if fit_delay else 2
    fits = lambda r, x: r - dr > 0 and all(r + dr < clearance(x + s) for s in (-dx, 0.0, dx))      # noqa: E731
    geoms = np.asarray([[r, x] for r in radii for x in offsets], dtype=np.float64)
    n, sse, sr, sw = misfit(model(geoms), tm, w)
    mse, _ = stats(n, sse, sr, sw, fit_delay)
    ok = (n >= min_pairs) & np.isfinite(mse) & np.asarray([fits(r, x) for r, x in geoms])
    if not ok.any():
        raise ValueError("no grid node reaches min_pairs")
    grid_mse = np.where(ok, mse, np.nan).reshape(len(radii), len(offsets))
    x = geoms[np.nanargmin(np.where(ok, mse, np.nan))].copy()
    lam, last, it, converged, step = 1e-3, None, 0, False, None
    while it < max_iter:
        if last is not None:
            x = last["x"] + step
            if not fits(x[0], x[1]):
                lam *= 10.0
                step = _step(last["JtJ"], last["Jtr"], lam)
                if lam > 1e12:
                    break
                continue
        it += 1
        tt = model(np.asarray([x, x + [dr, 0], x - [dr, 0], x + [0, dx], x - [0, dx]]))
        n, sse, sr, sw = misfit(tt, tm, w)
        mse, delay = stats(n, sse, sr, sw, fit_delay)
        if n[0] < min_pairs or not np.isfinite(mse[0]) or (last is not None and mse[0] > last["mse"]):
            lam *= 10.0
            step = _step(last["JtJ"], last["Jtr"], lam)
            if abs(step[0]) <= FIT_TOL and abs(step[1]) <= FIT_TOL:
                converged = True
                break
            if lam > 1e12:
                break
            continue
        use = np.isfinite(tt).all(axis=0) & np.isfinite(tm) & (wt_all > 0)
        res = (tt[0] - tm)[use]
        J = np.stack([(tt[1] - tt[2])[use] / (2 * dr), (tt[3] - tt[4])[use] / (2 * dx)], axis=1)
        wt = wt_all[use]
        if fit_delay:
            res = res - np.sum(wt * res) / np.sum(wt)
            J = J - (wt @ J) / np.sum(wt)
        JtJ, Jtr = J.T @ (J * wt[:, None]), J.T @ (wt * res)
        if last is not None:
            lam = max(lam / 10.0, 1e-12)
        last = dict(x=x.copy(), mse=float(mse[0]), delay=float(delay[0]), n=int(n[0]), JtJ=JtJ, Jtr=Jtr,
                    s2=float(np.sum(wt * res * res)) / max(int(use.sum()) - n_par, 1))
        if use.sum() < n_par or np.linalg.cond(JtJ) > 1e15:
            break
        step = _step(JtJ, Jtr, lam)
        if abs(step[0]) <= FIT_TOL and abs(step[1]) <= FIT_TOL:
            converged = True
            break
    return dict(r_outer=float(last["x"][0]), pipe_offset=float(last["x"][1]), delay=last["delay"], mse=last["mse"], n_pairs=last["n"],
                cov=last["s2"] * np.linalg.inv(last["JtJ"]), grid_mse=grid_mse, iterations=it, converged=converged)

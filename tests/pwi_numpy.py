"""Independent NumPy oracle of the plane-wave imaging entries (include/rtus.h: rtus_pw_layers, rtus_pw_surface, rtus_fmc_synth_tx).
NumPy only (scipy may be missing on the GPU machine); fp64 unless stated.

  * layers(): the planar closed form, with each layer's vertical extent clipped per entry (not the kernel's cumulative sums).
  * surface(): T'(x) sampled at SUB = 64 points per profile segment; every sign change is a stationary point, refined by bisection
    and safeguarded Newton in fp64 (surface_numpy's spline).  The entry is the least T over the minima whose refined x is
    insonified.  For each entry it also reports the winner's basin: twice the distance from the winning minimum to the nearer of its
    neighbouring stationary points and band edges (infinite without one) — the kernel's guarantee holds where basin >= dx.
  * synth(): the synthesis in fp32 arithmetic, term by term in tx order.
"""
import numpy as np

import surface_numpy as S

SUB = 64


def aperture_ref(angles, x_lo, x_hi):
    """sin, cos, x_ref and validity of each angle"""
    a = np.atleast_1d(np.asarray(angles, dtype=np.float64))
    ok = np.abs(a) < np.pi / 2
    t = np.where(ok, a, 0.0)
    sn, cs = np.sin(t), np.cos(t)
    return sn, cs, np.where(sn >= 0.0, x_lo, x_hi), ok


def delays(xe, angles, c1):
    """the plane waves' firing delays [n_a, n_e] of a horizontal array"""
    xe = np.asarray(xe, dtype=np.float64)
    sn, _, xref, ok = aperture_ref(angles, xe.min(), xe.max())
    d = (xe[None, :] - xref[:, None]) * sn[:, None] / c1
    d[~ok] = np.nan
    return d


def layers(z_if, c, angles, x_lo, x_hi, z_a, xf, zf):
    """t(F) = (xf - x_ref) p + sum_i h_i sqrt(1/c_i^2 - p^2), NaN under the header's rules -> [n_a, n_f]"""
    z_if = np.atleast_1d(np.asarray(z_if, dtype=np.float64)) if np.size(z_if) else np.zeros(0)
    c = np.asarray(c, dtype=np.float64)
    xf, zf = np.atleast_1d(np.asarray(xf, dtype=np.float64)), np.atleast_1d(np.asarray(zf, dtype=np.float64))
    sn, _, xref, ok = aperture_ref(angles, x_lo, x_hi)
    p = sn / c[0]
    tops = np.r_[z_a, z_if]
    bots = np.r_[z_if, np.inf]
    t = (xf[None, :] - xref[:, None]) * p[:, None]
    xb = np.broadcast_to(xf[None, :], t.shape).copy()
    bad = np.zeros(t.shape, dtype=bool)
    for i in range(c.size):
        h = np.clip(np.minimum(zf, bots[i]) - tops[i], 0.0, None)[None, :]            # vertical extent of layer i above zf
        pc = p * c[i]
        prop = np.abs(pc) < 1.0
        with np.errstate(invalid="ignore"):
            w = np.where(prop, np.sqrt((1.0 - pc) * (1.0 + pc)) / c[i], np.nan)[:, None]
            g = np.where(prop, pc / np.sqrt((1.0 - pc) * (1.0 + pc)), np.nan)[:, None]
        crossed = h > 0
        bad |= crossed & ~prop[:, None]
        t = t + np.where(crossed, h * np.where(prop[:, None], w, 0.0), 0.0)
        xb = xb - np.where(crossed, h * np.where(prop[:, None], g, 0.0), 0.0)
    good = ~bad & ok[:, None] & (zf[None, :] > z_a) & (xb >= x_lo) & (xb <= x_hi)
    return np.where(good, t, np.nan)


def _pw_T(coef, x0, dx, c1, c2, sn, cs, xref, za, xf, zf, x):
    """T, T', T'' of the plane-wave path at x (broadcasting)"""
    s, s1, s2 = S.spline_eval(coef, x0, dx, x)
    t1 = ((x - xref) * sn + (s - za) * cs) / c1
    d1 = (sn + s1 * cs) / c1
    L, L1, L2 = S._legs(coef, x0, dx, x, xf, zf, c2)
    return t1 + L, d1 + L1, s2 * cs / c1 + L2


def _refine(f, lo, hi, kind):
    lo, hi = lo.copy(), hi.copy()
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        right = (f(mid)[1] * kind) < 0
        lo = np.where(right, mid, lo)
        hi = np.where(right, hi, mid)
    x = 0.5 * (lo + hi)
    for _ in range(3):
        _, d1, d2 = f(x)
        with np.errstate(invalid="ignore", divide="ignore"):
            xn = x - d1 / d2
        x = np.where(np.isfinite(xn) & (xn >= lo) & (xn <= hi), xn, x)
    return x


def surface(x0, dx, zs, c1, c2, angles, x_lo, x_hi, z_a, xf, zf, chunk=256):
    """-> dict(t, x, basin), each [n_a, n_f]"""
    zs = np.asarray(zs, dtype=np.float64)
    coef = S.spline(x0, dx, zs)
    xf, zf = np.atleast_1d(np.asarray(xf, dtype=np.float64)), np.atleast_1d(np.asarray(zf, dtype=np.float64))
    sn, cs, xref, aok = aperture_ref(angles, x_lo, x_hi)
    n_a, n_f = sn.size, xf.size
    X = x0 + dx * np.arange(SUB * (zs.size - 1) + 1) / SUB
    sX = S.spline_eval(coef, x0, dx, X)[0]
    out_t, out_x, out_b = np.full((n_a, n_f), np.nan), np.full((n_a, n_f), np.nan), np.full((n_a, n_f), np.inf)
    xend = x0 + (zs.size - 1) * dx
    fok = (xf >= x0) & (xf <= xend) & (zf > S.spline_eval(coef, x0, dx, xf)[0])
    if not (z_a < S.spline_min(coef, dx)):
        return dict(t=out_t, x=out_x, basin=out_b)
    for a in range(n_a):
        if not aok[a]:
            continue
        tn = sn[a] / cs[a]
        inb = X - (sX - z_a) * tn
        inb = (inb >= x_lo) & (inb <= x_hi)
        edges = X[np.nonzero(inb[1:] != inb[:-1])[0]] + 0.5 * dx / SUB                # band edges on the dense grid

        def band(x):
            s = S.spline_eval(coef, x0, dx, x)[0]
            xb = x - (s - z_a) * tn
            return (xb >= x_lo) & (xb <= x_hi)

        for c0 in range(0, n_f, chunk):
            F = np.arange(c0, min(n_f, c0 + chunk))
            D = _pw_T(coef, x0, dx, c1, c2, sn[a], cs[a], xref[a], z_a, xf[F, None], zf[F, None], X[None, :])[1]
            ent, lo, hi, kind = [], [], [], []
            for k, m in ((1, (D[:, :-1] < 0) & (D[:, 1:] >= 0)), (-1, (D[:, :-1] > 0) & (D[:, 1:] <= 0))):
                fi, i = np.nonzero(m)
                ent.append(fi); lo.append(X[i]); hi.append(X[i + 1]); kind.append(np.full(fi.size, k))
            ent, lo, hi, kind = (np.concatenate(v) for v in (ent, lo, hi, kind))
            if ent.size == 0:
                continue
            fx, fz = xf[F][ent], zf[F][ent]
            f = lambda x: _pw_T(coef, x0, dx, c1, c2, sn[a], cs[a], xref[a], z_a, fx, fz, x)   # noqa: E731
            x = _refine(f, lo, hi, kind)
            t = f(x)[0]
            ok = band(x)
            for j in np.unique(ent):
                sel = np.nonzero(ent == j)[0]
                mins = sel[(kind[sel] == 1) & ok[sel]]
                if mins.size == 0 or not fok[F[j]]:
                    continue
                w = mins[np.argmin(t[mins])]
                others = np.r_[x[sel[sel != w]], edges]
                dist = np.abs(others - x[w])
                out_t[a, F[j]] = t[w]
                out_x[a, F[j]] = x[w]
                out_b[a, F[j]] = 2.0 * dist.min() if dist.size else np.inf
    return dict(t=out_t, x=out_x, basin=out_b)


def synth(fmc, fs, d):
    """out[v][rx][n] = sum over tx of x_{tx,rx}(n - d[v][tx] fs) in the header's fp32 arithmetic"""
    fmc = np.asarray(fmc, dtype=np.float32)
    d = np.atleast_2d(np.asarray(d, dtype=np.float64))
    n_tx, n_rx, n_t = fmc.shape
    out = np.zeros((d.shape[0], n_rx, n_t), dtype=np.float32)
    n = np.arange(n_t)
    for v in range(d.shape[0]):
        for tx in range(n_tx):
            with np.errstate(invalid="ignore"):
                sh = d[v, tx] * fs
            if not (abs(sh) < 1e8):
                continue
            m = np.ceil(sh)
            w = np.float32(m - sh)
            i = n - int(m)
            x0 = np.where((i >= 0) & (i < n_t), fmc[tx][:, np.clip(i, 0, n_t - 1)], np.float32(0))
            x1 = np.where((i + 1 >= 0) & (i + 1 < n_t), fmc[tx][:, np.clip(i + 1, 0, n_t - 1)], np.float32(0))
            dd = (x1 - x0).astype(np.float32)
            term = (np.float64(w) * dd.astype(np.float64) + x0.astype(np.float64)).astype(np.float32)   # fmaf: w*dd exact in fp64
            out[v] = (out[v] + term).astype(np.float32)
    return out

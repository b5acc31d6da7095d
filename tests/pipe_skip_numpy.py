"""fp64 NumPy restatement of rtus_tt_pipe_skip's definition (include/rtus.h): element behind the curved lens (c1) -> water (c2) ->
the pipe's outer circle at Q(beta) -> the wall at c_down -> a bounce off the bore at R(gamma) -> the wall at c_up -> the point F.
Built on tests/pipe_numpy.py (the lens leg, the outer circle, rule 1); the oracle of tests/test_pipe_skip_cpu.py and
tests/test_gpu_pipe_skip.py, itself checked against a 40-digit joint solve in (alpha, beta, gamma).

    T(beta) = T_lens(E, Q(beta)) + W(Q(beta), F),   W(Q, F) = min over gamma of |Q - R(gamma)| / c_down + |R(gamma) - F| / c_up

gamma runs over the arc of the bore that Q and F both see; W is the time at the interior minimum on that arc and does not exist
where the arc is empty or the least time sits at an end of it (a grazing bounce).  On that arc both lengths are convex in gamma
(d2|Q - R| / dgamma2 = ro ri (ro cos u - ri)(ro - ri cos u) / |Q - R|^3 with u = gamma - beta, positive exactly where Q sees R), so
W exists when dW_path/dgamma is negative at the arc's lower end and positive at its upper end, and the minimum is the only one.
The oracle works in Cartesian coordinates and counts the minima on a dense gamma grid all the same (``detail``: n_gamma).
T'(beta) = u . Q' / c2 + w . Q' / c_down (u the water segment's unit direction at Q, w the unit vector from R to Q)."""
import numpy as np

import pipe_numpy as O

ALPHA_MAX = O.ALPHA_MAX


def _bore(pipe, g):
    s, c = np.sin(g), np.cos(g)
    return pipe.x0 + pipe.ri * s, pipe.ri * c, pipe.ri * c, -pipe.ri * s


def _h(pipe, c_up, qx, qz, fx, fz, g):
    """the bounce path's time at gamma and its derivative in gamma"""
    rx, rz, r1x, r1z = _bore(pipe, g)
    ax, az, bx, bz = rx - qx, rz - qz, rx - fx, rz - fz
    la, lb = np.hypot(ax, az), np.hypot(bx, bz)
    return la / pipe.c3 + lb / c_up, (ax * r1x + az * r1z) / la / pipe.c3 + (bx * r1x + bz * r1z) / lb / c_up


def arc(pipe, qx, qz, fx, fz):
    """the bore's arc that Q and F both see -> (lo, hi) in gamma, hi <= lo where it is empty.  Q sees R(gamma) when
    (Q - R) . (R - Cp) > 0: |gamma - angle of Q| < arccos(ri / |Q - Cp|); both arcs are shorter than pi, so their common part is
    one interval (the angle of F is unwrapped to within pi of Q's)"""
    tq, tf = np.arctan2(qx - pipe.x0, qz), np.arctan2(fx - pipe.x0, fz)
    with np.errstate(invalid="ignore"):
        aq = np.arccos(pipe.ri / np.hypot(qx - pipe.x0, qz))
        af = np.arccos(pipe.ri / np.hypot(fx - pipe.x0, fz))
    d = tf - tq
    d = d - 2 * np.pi * np.round(d / (2 * np.pi))
    tf = tq + d
    return np.maximum(tq - aq, tf - af), np.minimum(tq + aq, tf + af)


def bore_min(pipe, c_up, qx, qz, fx, fz, iters=100):
    """W(Q, F) and its gamma (broadcast arrays); NaN where W does not exist.  Bisection-safeguarded secant steps (Illinois) on
    dW_path/dgamma between the arc's ends"""
    qx, qz, fx, fz = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (qx, qz, fx, fz)))
    shp = qx.shape
    qx, qz, fx, fz = (v.ravel() for v in (qx, qz, fx, fz))
    lo, hi = arc(pipe, qx, qz, fx, fz)
    with np.errstate(invalid="ignore", divide="ignore"):
        glo, ghi = _h(pipe, c_up, qx, qz, fx, fz, lo)[1], _h(pipe, c_up, qx, qz, fx, fz, hi)[1]
        ok = (hi > lo) & (glo < 0) & (ghi > 0)
    W, G = np.full(qx.size, np.nan), np.full(qx.size, np.nan)
    k = np.nonzero(ok)[0]
    if k.size:
        lo, hi, glo, ghi, qx, qz, fx, fz = (v[k] for v in (lo, hi, glo, ghi, qx, qz, fx, fz))
        side = np.zeros(k.size)
        x = lo
        for _ in range(iters):
            x = lo - glo * (hi - lo) / (ghi - glo)
            x = np.where((x > lo) & (x < hi), x, 0.5 * (lo + hi))
            gx = _h(pipe, c_up, qx, qz, fx, fz, x)[1]
            neg = gx < 0
            ghi = np.where(neg & (side < 0), 0.5 * ghi, ghi)
            glo = np.where(~neg & (side > 0), 0.5 * glo, glo)
            lo, glo = np.where(neg, x, lo), np.where(neg, gx, glo)
            hi, ghi = np.where(neg, hi, x), np.where(neg, ghi, gx)
            side = np.where(neg, -1.0, 1.0)
            if np.all((hi - lo <= 4e-16) | (gx == 0)):
                break
        W[k], G[k] = _h(pipe, c_up, qx, qz, fx, fz, x)[0], x
    return W.reshape(shp), G.reshape(shp)


def gamma_minima(pipe, c_up, qx, qz, fx, fz, n=513):
    """how many local minima the bounce path's time has on ``n`` even samples of the common arc (0 where there is no arc)"""
    qx, qz, fx, fz = (np.asarray(v, dtype=np.float64).ravel() for v in np.broadcast_arrays(qx, qz, fx, fz))
    lo, hi = arc(pipe, qx, qz, fx, fz)
    has = hi > lo
    g = lo[:, None] + (hi - lo)[:, None] * np.linspace(0.0, 1.0, n)[None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        d = _h(pipe, c_up, qx[:, None], qz[:, None], fx[:, None], fz[:, None], g)[1]
    return np.where(has, np.sum((d[:, :-1] < 0) & (d[:, 1:] >= 0), axis=1), 0)


def _dT(lens, pipe, c_up, xa, za, xf, zf, beta, a_lo, a_hi):
    """T'(beta) and the path (T, alpha, gamma, lens point, Q) for arrays of pairs and angles"""
    qx, qz, q1x, q1z = pipe.q(beta)
    Tl, al = O.lens_min(lens, xa, za, qx, qz, a_lo, a_hi)
    px, pz, _, _ = lens.point(al)
    ux, uz = qx - px, qz - pz
    W, g = bore_min(pipe, c_up, qx, qz, xf, zf)
    rx, rz, _, _ = _bore(pipe, g)
    wx, wz = qx - rx, qz - rz
    d1 = (ux * q1x + uz * q1z) / np.hypot(ux, uz) / lens.c2 + (wx * q1x + wz * q1z) / np.hypot(wx, wz) / pipe.c3
    return d1, Tl + W, al, g, px, pz, qx, qz


def table(lens, pipe, c_up, xe, ze, xf, zf, *, a_lo=-ALPHA_MAX, a_hi=ALPHA_MAX, b_lo=-np.pi / 2, b_hi=np.pi / 2, n_scan=None,
          pairs=None, dense=4, iters=60, detail=False):
    """-> dict t, alpha, beta, gamma [n_e, n_f] (or [n_pairs] for pairs = (ie, jf) index arrays) and flag: an interior minimum of
    T has a neighbouring stationary point closer than one scan step of the kernel, or lies in a scan cell of the kernel with an end
    (or the dense point beyond it) without W (such entries may be found late by the kernel).  ``pipe.c3`` is c_down.
    detail: also n_min, the interior minima of T found on the dense grid; rank, how many of them are earlier than the winner (-1
    without a winner: a winner of rank > 0 is not the earliest minimum); rej1, how many of those earlier ones (of all of them
    without a winner) fail rule 1; no_arc, entries of points in the wall for which no beta of the grid shares an arc of the bore
    with the point; graze, entries with an arc somewhere and yet no interior minimum of T (the least time over the betas that have
    a W sits where the bounce grazes); n_gamma, the most local minima of the inner problem seen on a dense gamma grid, at every
    eighth beta of the dense grid and at the winner's; minima, every refined interior minimum of T as flat arrays: entry (the flat index
    into the table), t (inf without W), alpha, beta, gamma, rule1."""
    xe, ze, xf, zf = (np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in (xe, ze, xf, zf))
    if pairs is None:
        ie, jf = (a.ravel() for a in np.meshgrid(np.arange(xe.size), np.arange(xf.size), indexing="ij"))
        shape = (xe.size, xf.size)
    else:
        ie, jf = (np.asarray(a) for a in pairs)
        shape = ie.shape
    n_scan = O.default_n_scan(pipe.r, b_lo, b_hi) if n_scan is None else int(n_scan)
    hb = (b_hi - b_lo) / (n_scan - 1)
    nb = dense * (n_scan - 1) + 1
    beta = np.linspace(b_lo, b_hi, nb)
    ue, inv = np.unique(ie, return_inverse=True)
    qx, qz, q1x, q1z = pipe.q(beta)
    Tl, al = O.lens_min(lens, xe[ue][:, None], ze[ue][:, None], qx[None, :], qz[None, :], a_lo, a_hi)
    px, pz, _, _ = lens.point(al)
    ux, uz = qx - px, qz - pz
    dl = (ux * q1x + uz * q1z) / np.hypot(ux, uz) / lens.c2               # [n_ue, nb]
    # the bounce term depends on (point, beta) only
    uf, finv = np.unique(jf, return_inverse=True)
    P = ie.size
    out = {k: np.full(P, np.nan) for k in ("t", "alpha", "beta", "gamma")}
    flag = np.zeros(P, dtype=bool)
    no_arc, has_w = np.zeros(P, dtype=bool), np.zeros(P, dtype=bool)
    n_gamma = np.zeros(P, dtype=np.int64)
    m_p, m_T, m_1, m_a, m_b, m_g = [], [], [], [], [], []
    fx, fz = xf[jf], zf[jf]
    rf = np.hypot(fx - pipe.x0, fz)
    inwall = (rf > pipe.ri) & (rf < pipe.r) & np.isfinite(xe[ie]) & np.isfinite(ze[ie])
    CH = 256
    for c0 in range(0, uf.size, CH):
        fsel = uf[c0:c0 + CH]
        W, g = bore_min(pipe, c_up, qx[None, :], qz[None, :], xf[fsel][:, None], zf[fsel][:, None])
        rx, rz, _, _ = _bore(pipe, g)
        wx, wz = qx - rx, qz - rz
        dw = (wx * q1x + wz * q1z) / np.hypot(wx, wz) / pipe.c3          # [n_sel, nb], NaN without W
        alo, ahi = arc(pipe, qx[None, :], qz[None, :], xf[fsel][:, None], zf[fsel][:, None])
        anyarc = np.any(ahi > alo, axis=1)
        ng = np.zeros(fsel.size, dtype=np.int64)
        if detail:
            sub = slice(0, nb, 8)
            ng = gamma_minima(pipe, c_up, qx[None, sub], qz[None, sub], xf[fsel][:, None],
                              zf[fsel][:, None]).reshape(fsel.size, -1).max(axis=1)
        ps = np.nonzero((finv >= c0) & (finv < c0 + fsel.size))[0]         # the entries of these points
        if not ps.size:
            continue
        row = finv[ps] - c0
        no_arc[ps] = ~anyarc[row] & inwall[ps]
        has_w[ps] = np.any(np.isfinite(dw[row]), axis=1)
        n_gamma[ps] = ng[row]
        d1 = dl[inv[ps]] + dw[row]
        nan = np.isnan(d1)
        s = np.where(nan, 0, np.sign(d1))
        mins = (d1[:, :-1] < 0) & (d1[:, 1:] >= 0) & inwall[ps, None]
        stat = (s[:, :-1] * s[:, 1:]) < 0
        ri_, ci = np.nonzero(mins)
        for r, i in zip(ri_, ci):
            sp = np.nonzero(stat[r])[0]
            k = np.searchsorted(sp, i)
            left = beta[i] - beta[sp[k - 1]] if k > 0 else np.inf
            right = beta[sp[k + 1]] - beta[i] if k + 1 < sp.size else np.inf
            jc = (i // dense) * dense                          # the kernel's scan cell around the minimum: both ends need a W
            if min(left, right) < hb or nan[r, max(jc - 1, 0):jc + 1].any() or nan[r, jc + dense:jc + dense + 2].any():
                flag[ps[r]] = True
        if not ri_.size:
            continue
        p = ps[ri_]
        ia, ja = ie[p], jf[p]
        lo, hi = beta[ci], beta[ci + 1]
        glo, ghi = d1[ri_, ci], d1[ri_, ci + 1]
        side = np.zeros(p.size)
        x = lo
        for _ in range(iters):
            x = lo - glo * (hi - lo) / (ghi - glo)
            x = np.where((x > lo) & (x < hi), x, 0.5 * (lo + hi))
            gx = _dT(lens, pipe, c_up, xe[ia], ze[ia], xf[ja], zf[ja], x, a_lo, a_hi)[0]
            neg = gx < 0
            ghi = np.where(neg & (side < 0), 0.5 * ghi, ghi)
            glo = np.where(~neg & (side > 0), 0.5 * glo, glo)
            lo, glo = np.where(neg, x, lo), np.where(neg, gx, glo)
            hi, ghi = np.where(neg, hi, x), np.where(neg, ghi, gx)
            side = np.where(neg, -1.0, 1.0)
            if np.all(hi - lo <= 4e-16):
                break
        _, T, a_, g_, px_, pz_, qx_, qz_ = _dT(lens, pipe, c_up, xe[ia], ze[ia], xf[ja], zf[ja], x, a_lo, a_hi)
        r1, _ = O.rules(px_, pz_, qx_, qz_, xf[ja], zf[ja], pipe)
        ok = r1 & np.isfinite(T)
        m_p.append(p); m_T.append(np.where(np.isfinite(T), T, np.inf)); m_1.append(r1)
        m_a.append(a_); m_b.append(x); m_g.append(g_)
        for n in np.nonzero(ok)[0]:
            if not (T[n] >= out["t"][p[n]]):
                out["t"][p[n]], out["alpha"][p[n]], out["beta"][p[n]], out["gamma"][p[n]] = T[n], a_[n], x[n], g_[n]
    o = {k: v.reshape(shape) for k, v in out.items()}
    o["flag"] = flag.reshape(shape)
    if detail:
        m_p, m_T = (np.concatenate(v) if v else np.zeros(0, dtype=t) for v, t in ((m_p, np.intp), (m_T, np.float64)))
        m_1 = np.concatenate(m_1) if m_1 else np.zeros(0, dtype=bool)
        earlier = ~(m_T >= out["t"][m_p])
        count = lambda w: np.bincount(m_p, weights=w, minlength=P).astype(np.int64)      # noqa: E731
        n_min = count(np.ones(m_p.size))
        o["n_min"] = n_min.reshape(shape)
        o["rank"] = np.where(np.isfinite(out["t"]), count(earlier), -1).reshape(shape)
        o["rej1"] = count(earlier & ~m_1).reshape(shape)
        m_a, m_b, m_g = (np.concatenate(v) if v else np.zeros(0) for v in (m_a, m_b, m_g))
        o["minima"] = {"entry": m_p, "t": m_T, "alpha": m_a, "beta": m_b, "gamma": m_g, "rule1": m_1}
        o["no_arc"] = no_arc.reshape(shape)
        o["graze"] = (inwall & ~no_arc & has_w & (n_min == 0)).reshape(shape)
        won = np.isfinite(out["t"])
        if won.any():
            wq = pipe.q(out["beta"][won])
            n_gamma[won] = np.maximum(n_gamma[won], gamma_minima(pipe, c_up, wq[0], wq[1], fx[won], fz[won]))
        o["n_gamma"] = n_gamma.reshape(shape)
    return o


def snell_residuals(lens, pipe, c_up, xe, ze, xf, zf, alpha, beta, gamma):
    """(sin of the incidence angle / c_in - sin of the outgoing angle / c_out) / (1 / c_out) at the lens, at the outer circle and
    at the bore (there: the reflection law with conversion, sin i / c_down = sin r / c_up)"""
    px, pz, p1x, p1z = lens.point(alpha)
    qx, qz, q1x, q1z = pipe.q(beta)
    rx, rz, r1x, r1z = _bore(pipe, gamma)

    def unit(x, z):
        n = np.hypot(x, z)
        return x / n, z / n
    a1, a2, a3, a4 = unit(px - xe, pz - ze), unit(qx - px, qz - pz), unit(rx - qx, rz - qz), unit(xf - rx, zf - rz)
    t1, t2, t3 = unit(p1x, p1z), unit(q1x, q1z), unit(r1x, r1z)
    dot = lambda a, t: a[0] * t[0] + a[1] * t[1]      # noqa: E731
    return ((dot(a1, t1) / lens.c1 - dot(a2, t1) / lens.c2) * lens.c2, (dot(a2, t2) / lens.c2 - dot(a3, t2) / pipe.c3) * pipe.c3,
            (dot(a3, t3) / pipe.c3 - dot(a4, t3) / c_up) * c_up)

"""fp64 NumPy restatement of rtus_tt_pipe's definition (include/rtus.h): element behind the curved lens (c1) -> water (c2) -> the
pipe's outer circle -> a point in the wall (c3).  Slow and plain; the oracle of tests/test_pipe_cpu.py and tests/test_gpu_pipe.py,
itself checked against a 40-digit joint solve in (alpha, beta).

Lens leg to a point Q: T_lens(E, Q) = the least time over alpha in [a_lo, a_hi] of |P(alpha) - E| / c1 + |Q - P(alpha)| / c2, the
ends included — dense samples of alpha, and the zero of g = dT/dalpha by Illinois regula falsi in every cell where g goes - -> +.
Outer problem: T(beta) = T_lens(E, Q(beta)) + |Q(beta) - F| / c3 on a dense grid of beta, T'(beta) = u . Q' / c2 + v . Q' / c3
(u, v the unit directions of the water and wall segments at Q: envelope theorem), each - -> + sign change refined by Illinois
regula falsi on T'.  Rules: the water segment arrives from outside the circle, the wall segment keeps r_inner off the centre."""
import numpy as np

ALPHA_MAX = float(np.float64(50.62033040986099 * (np.pi / 180)))
C1, C2, C3 = 6400.0, 1483.0, 5600.0
L0, H0 = 0.12156646438729327, 0.08843353561270673
D = float(np.float64(L0) + np.float64(H0))


class Lens:
    def __init__(self, c1=C1, c2=C2, l0=L0, h0=H0, d=D):
        self.c1, self.c2, self.d = float(c1), float(c2), float(d)
        T = l0 / c1 + h0 / c2
        self.A = c1 * c1 / (c2 * c2) - 1.0                              # main_rt.py:183
        self.C = c1 * c1 * T * T - d * d                                # :185
        self.phi_2 = -2.0 * T * c1 * c1 / c2                            # :200
        self.phi_3 = 2.0 * d                                            # :201

    def point(self, alpha):
        """P(alpha) and P'(alpha) (main_rt.py:180-234)"""
        s, c = np.sin(alpha), np.cos(alpha)
        B = self.phi_2 + self.phi_3 * c
        sq = np.sqrt(B * B - 4.0 * self.A * self.C)
        h = (-B - sq) / (2.0 * self.A)                                  # roots_bhaskara(...)[1]
        dB = -self.phi_3 * s
        dh = -1.0 / (2.0 * self.A) * (dB + B * dB / sq)
        return h * s, h * c, dh * s + h * c, dh * c - h * s


def clearance(lens, x_off, a_lo=-ALPHA_MAX, a_hi=ALPHA_MAX, n=200001):
    """the least distance from (x_off, 0) to the lens surface over [a_lo, a_hi]"""
    al = np.linspace(a_lo, a_hi, n)
    px, pz, _, _ = lens.point(al)
    d = np.hypot(px - x_off, pz)
    return float(np.nanmin(d))


def _lens_tg(lens, al, xa, za, qx, qz):
    px, pz, p1x, p1z = lens.point(al)
    ax, az, fx, fz = px - xa, pz - za, px - qx, pz - qz
    la, lf = np.hypot(ax, az), np.hypot(fx, fz)
    T = la / lens.c1 + lf / lens.c2
    g = (ax * p1x + az * p1z) / la / lens.c1 + (fx * p1x + fz * p1z) / lf / lens.c2
    return T, g


def lens_min(lens, xa, za, qx, qz, a_lo=-ALPHA_MAX, a_hi=ALPHA_MAX, ns=96, iters=80):
    """least lens-leg time from E = (xa, za) to Q = (qx, qz) (broadcast arrays) -> (T, alpha)"""
    xa, za, qx, qz = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (xa, za, qx, qz)))
    shp = xa.shape
    xa, za, qx, qz = (v.ravel() for v in (xa, za, qx, qz))
    al = np.linspace(a_lo, a_hi, ns + 1)[:, None] * np.ones((1, xa.size))
    T, g = _lens_tg(lens, al, xa, za, qx, qz)
    Tn = np.where(np.isnan(T), np.inf, T)
    k = np.argmin(Tn, axis=0)
    cols = np.arange(xa.size)
    bT, bA = Tn[k, cols], al[k, cols]
    ci, cj = np.nonzero((g[:-1] < 0) & (g[1:] >= 0))                   # cells with a minimum inside
    if ci.size:
        lo, hi, glo, ghi = al[ci, cj], al[ci + 1, cj], g[ci, cj], g[ci + 1, cj]
        ex, ez, fx_, fz_ = xa[cj], za[cj], qx[cj], qz[cj]
        side = np.zeros(ci.size)
        x = lo
        for _ in range(iters):
            x = lo - glo * (hi - lo) / (ghi - glo)
            x = np.where((x > lo) & (x < hi), x, 0.5 * (lo + hi))
            _, gx = _lens_tg(lens, x, ex, ez, fx_, fz_)
            neg = gx < 0
            ghi = np.where(neg & (side < 0), 0.5 * ghi, ghi)
            glo = np.where(~neg & (side > 0), 0.5 * glo, glo)
            lo, glo = np.where(neg, x, lo), np.where(neg, gx, glo)
            hi, ghi = np.where(neg, hi, x), np.where(neg, ghi, gx)
            side = np.where(neg, -1.0, 1.0)
            if np.all(hi - lo <= 1e-15 * np.maximum(1.0, np.abs(x))):
                break
        Tx, _ = _lens_tg(lens, x, ex, ez, fx_, fz_)
        Tx = np.where(np.isnan(Tx), np.inf, Tx)                         # the least over the cells of each entry
        o = np.lexsort((Tx, cj))
        first = o[np.r_[True, cj[o][1:] != cj[o][:-1]]]
        c = cj[first]
        take = Tx[first] < bT[c]
        bT[c[take]], bA[c[take]] = Tx[first][take], x[first][take]
    bT = np.where(np.isfinite(bT), bT, np.nan)
    return bT.reshape(shp), bA.reshape(shp)


class Pipe:
    def __init__(self, r_outer, x_off, r_inner=0.0, c3=C3):
        self.r, self.x0, self.ri, self.c3 = float(r_outer), float(x_off), float(r_inner), float(c3)

    def q(self, beta):
        s, c = np.sin(beta), np.cos(beta)
        return self.x0 + self.r * s, self.r * c, self.r * c, -self.r * s


def _dT(lens, pipe, xa, za, xf, zf, beta, a_lo, a_hi):
    """T'(beta) and the path (T, alpha, lens point) for arrays of pairs and angles"""
    qx, qz, q1x, q1z = pipe.q(beta)
    Tl, al = lens_min(lens, xa, za, qx, qz, a_lo, a_hi)
    px, pz, _, _ = lens.point(al)
    ux, uz = qx - px, qz - pz
    lu = np.hypot(ux, uz)
    vx, vz = qx - xf, qz - zf
    lv = np.hypot(vx, vz)
    d1 = (ux * q1x + uz * q1z) / lu / lens.c2 + (vx * q1x + vz * q1z) / lv / pipe.c3
    return d1, Tl + lv / pipe.c3, al, px, pz, qx, qz


def rules(px, pz, qx, qz, xf, zf, pipe):
    """-> (rule 1: the water segment L -> Q arrives from outside the circle, rule 2: the wall segment Q -> F keeps r_inner off Cp)"""
    cx, cz = qx - pipe.x0, qz
    outside = (qx - px) * cx + (qz - pz) * cz < 0
    sx, sz = xf - qx, zf - qz
    t = np.clip(-(cx * sx + cz * sz) / (sx * sx + sz * sz), 0.0, 1.0)
    clear = np.hypot(cx + t * sx, cz + t * sz) >= pipe.ri
    return outside, clear


def qualifies(px, pz, qx, qz, xf, zf, pipe):
    outside, clear = rules(px, pz, qx, qz, xf, zf, pipe)
    return outside & clear


def default_n_scan(r_outer, b_lo=-np.pi / 2, b_hi=np.pi / 2, arc=0.25e-3):
    return max(int(np.ceil(r_outer * (b_hi - b_lo) / arc)) + 1, 4)


def table(lens, pipe, xe, ze, xf, zf, *, a_lo=-ALPHA_MAX, a_hi=ALPHA_MAX, b_lo=-np.pi / 2, b_hi=np.pi / 2, n_scan=None, pairs=None,
          dense=4, iters=60, detail=False):
    """-> dict t, alpha, beta [n_e, n_f] (or [n_pairs] for pairs = (ie, jf) index arrays) and flag: an interior minimum of T has a
    neighbouring stationary point closer than one scan step of the kernel (such entries may be found late by the kernel).
    detail: also n_min, the interior minima of T found on the dense grid; rank, how many of them are earlier than the winner (-1
    without a winner); rej1 / rej2, how many of those earlier ones (of all of them without a winner) fail rule 1 / rule 2"""
    xe, ze, xf, zf = (np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in (xe, ze, xf, zf))
    if pairs is None:
        ie, jf = (a.ravel() for a in np.meshgrid(np.arange(xe.size), np.arange(xf.size), indexing="ij"))
        shape = (xe.size, xf.size)
    else:
        ie, jf = (np.asarray(a) for a in pairs)
        shape = ie.shape
    n_scan = default_n_scan(pipe.r, b_lo, b_hi) if n_scan is None else int(n_scan)
    hb = (b_hi - b_lo) / (n_scan - 1)
    nb = dense * (n_scan - 1) + 1
    beta = np.linspace(b_lo, b_hi, nb)
    # the lens leg on the grid depends on (element, beta) only
    ue, inv = np.unique(ie, return_inverse=True)
    qx, qz, q1x, q1z = pipe.q(beta)
    Tl, al = lens_min(lens, xe[ue][:, None], ze[ue][:, None], qx[None, :], qz[None, :], a_lo, a_hi)
    px, pz, _, _ = lens.point(al)
    ux, uz = qx - px, qz - pz
    dl = (ux * q1x + uz * q1z) / np.hypot(ux, uz) / lens.c2               # [n_ue, nb]
    P = ie.size
    out_t, out_a, out_b = np.full(P, np.nan), np.full(P, np.nan), np.full(P, np.nan)
    flag = np.zeros(P, dtype=bool)
    m_p, m_T, m_1, m_2 = [], [], [], []                                 # every refined minimum: entry, time, rule 1, rule 2
    fx, fz = xf[jf], zf[jf]
    rf = np.hypot(fx - pipe.x0, fz)
    inwall = (rf > pipe.ri) & (rf < pipe.r) & np.isfinite(xe[ie]) & np.isfinite(ze[ie])
    CH = 512
    for c0 in range(0, P, CH):
        sl = slice(c0, min(P, c0 + CH))
        vx, vz = qx[None, :] - fx[sl, None], qz[None, :] - fz[sl, None]
        d1 = dl[inv[sl]] + (vx * q1x + vz * q1z) / np.hypot(vx, vz) / pipe.c3
        s = np.where(np.isnan(d1), 0, np.sign(d1))
        mins = (d1[:, :-1] < 0) & (d1[:, 1:] >= 0)
        stat = (s[:, :-1] * s[:, 1:]) < 0                              # every sign change: a stationary point
        for r, i in zip(*np.nonzero(mins & inwall[sl, None])):
            sp = np.nonzero(stat[r])[0]
            k = np.searchsorted(sp, i)
            left = beta[i] - beta[sp[k - 1]] if k > 0 else np.inf
            right = beta[sp[k + 1]] - beta[i] if k + 1 < sp.size else np.inf
            if min(left, right) < hb:
                flag[c0 + r] = True
        ri, ci = np.nonzero(mins & inwall[sl, None])
        if not ri.size:
            continue
        p = c0 + ri
        ia = ie[p]
        lo, hi = beta[ci], beta[ci + 1]
        glo, ghi = d1[ri, ci], d1[ri, ci + 1]
        side = np.zeros(ri.size)
        x = lo
        for _ in range(iters):
            x = lo - glo * (hi - lo) / (ghi - glo)
            x = np.where((x > lo) & (x < hi), x, 0.5 * (lo + hi))
            gx = _dT(lens, pipe, xe[ia], ze[ia], xf[jf[p]], zf[jf[p]], x, a_lo, a_hi)[0]
            neg = gx < 0
            ghi = np.where(neg & (side < 0), 0.5 * ghi, ghi)
            glo = np.where(~neg & (side > 0), 0.5 * glo, glo)
            lo, glo = np.where(neg, x, lo), np.where(neg, gx, glo)
            hi, ghi = np.where(neg, hi, x), np.where(neg, ghi, gx)
            side = np.where(neg, -1.0, 1.0)
            if np.all(hi - lo <= 4e-16):
                break
        _, T, a_, px_, pz_, qx_, qz_ = _dT(lens, pipe, xe[ia], ze[ia], xf[jf[p]], zf[jf[p]], x, a_lo, a_hi)
        r1, r2 = rules(px_, pz_, qx_, qz_, xf[jf[p]], zf[jf[p]], pipe)
        ok = r1 & r2 & np.isfinite(T)
        m_p.append(p); m_T.append(np.where(np.isfinite(T), T, np.inf)); m_1.append(r1); m_2.append(r2)
        for n in np.nonzero(ok)[0]:
            if not (T[n] >= out_t[p[n]]):
                out_t[p[n]], out_a[p[n]], out_b[p[n]] = T[n], a_[n], x[n]
    o = {"t": out_t.reshape(shape), "alpha": out_a.reshape(shape), "beta": out_b.reshape(shape), "flag": flag.reshape(shape)}
    if detail:
        m_p, m_T = (np.concatenate(v) if v else np.zeros(0, dtype=t) for v, t in ((m_p, np.intp), (m_T, np.float64)))
        m_1, m_2 = (np.concatenate(v) if v else np.zeros(0, dtype=bool) for v in (m_1, m_2))
        earlier = ~(m_T >= out_t[m_p])                                  # (no winner: every minimum)
        count = lambda w: np.bincount(m_p, weights=w, minlength=P).astype(np.int64)      # noqa: E731
        o["n_min"] = count(np.ones(m_p.size)).reshape(shape)
        o["rank"] = np.where(np.isfinite(out_t), count(earlier), -1).reshape(shape)
        o["rej1"], o["rej2"] = count(earlier & ~m_1).reshape(shape), count(earlier & ~m_2).reshape(shape)
    return o


def snell_residuals(lens, pipe, xe, ze, xf, zf, alpha, beta):
    """(sin of the incidence angle / c_in - sin of the refraction angle / c_out) / (1 / c_out) at the lens and at the pipe"""
    px, pz, p1x, p1z = lens.point(alpha)
    qx, qz, q1x, q1z = pipe.q(beta)

    def unit(x, z):
        n = np.hypot(x, z)
        return x / n, z / n
    a1, a2, a3 = unit(px - xe, pz - ze), unit(qx - px, qz - pz), unit(xf - qx, zf - qz)
    t1, t2 = unit(p1x, p1z), unit(q1x, q1z)
    r1 = ((a1[0] * t1[0] + a1[1] * t1[1]) / lens.c1 - (a2[0] * t1[0] + a2[1] * t1[1]) / lens.c2) * lens.c2
    r2 = ((a2[0] * t2[0] + a2[1] * t2[1]) / lens.c2 - (a3[0] * t2[0] + a3[1] * t2[1]) / pipe.c3) * pipe.c3
    return r1, r2

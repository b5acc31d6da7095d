"""NumPy oracle of the ray amplitude tables (include/rtus.h, rtus_leg_amp_surface): plane-wave displacement coefficients at a
fluid-solid interface and at a free surface (closed forms by Cramer's rule), 2-D geometric spreading by the ray tube carried through
each segment and interface, element directivity — and the fp64 restatement of the weighted delay-and-sum (rtus_tfm_weighted).

Frame of an interface: unit normal n, tangent t = (n_z, -n_x) (a proper rotation of (x, z)).  A wave with horizontal slowness p
(along t) travels along d = c (p, +-q) in (t, n) components, q = sqrt(1/c^2 - p^2), or i sqrt(p^2 - 1/c^2) past its critical angle
(evanescent: it decays away from the interface in the e^{i(k.x - wt)} convention used here).  Polarisation: L along d, T along
(-d_n, d_t).  Per unit amplitude a wave contributes u_n, sigma_nn / (i w), sigma_tn / (i w):
    L:  c s q,            rho c (1 - 2 c_T^2 p^2),       2 rho c_T^2 c s p q          (s = +1 along n, -1 against it)
    T:  c p,              2 rho c_T^2 c s p q,           -rho c (1 - 2 c_T^2 p^2)
    fluid (L, c_T = 0):   c s q,  rho c,  0
These coefficients are those of e^{-iwt}; the tabulated amplitude is their CONJUGATE (it multiplies the analytic signal, e^{+iwt})."""
import numpy as np

import surface_numpy as S

LEG_CODES = {"L": 0, "T": 1, "LL": 2, "LT": 3, "TL": 4, "TT": 5}


def qv(p, c):
    """vertical slowness: real and >= 0 while the wave propagates, +i |.| past its critical angle"""
    a = 1.0 / (c * c) - p * p
    return np.where(a >= 0, np.sqrt(np.abs(a)) + 0j, 1j * np.sqrt(np.abs(a)))


def _wave(mode, p, c, ct, rho, s):
    """(u_n, sigma_nn / (i w), sigma_tn / (i w)) of one wave; ct = 0 for the fluid"""
    q = qv(p, c)
    b = 1.0 - 2.0 * ct * ct * p * p
    if mode == "L":
        return c * s * q, rho * c * b + 0j, 2.0 * rho * ct * ct * c * s * p * q
    return c * p + 0j, 2.0 * rho * ct * ct * c * s * p * q, -rho * c * b + 0j


def _det3(m):
    return (m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0])
            + m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]))


def _cramer3(cols, rhs):
    """solution of sum_j x_j cols[j] = rhs (three 3-vectors of arrays) by Cramer's rule"""
    m = [[cols[j][i] for j in range(3)] for i in range(3)]
    d = _det3(m)
    out = []
    for k in range(3):
        mk = [[rhs[i] if j == k else m[i][j] for j in range(3)] for i in range(3)]
        out.append(_det3(mk) / d)
    return out


def fluid_solid(p, r1, c1, r2, cl, ct):
    """fluid -> solid (incident in the fluid along +n): (R, T_L, T_T)"""
    inc = _wave("L", p, c1, 0.0, r1, +1)
    ref = _wave("L", p, c1, 0.0, r1, -1)
    wl, wt = _wave("L", p, cl, ct, r2, +1), _wave("T", p, ct, ct, r2, +1)
    # fluid side = solid side for u_n and sigma_nn, sigma_tn = 0:  -R ref + TL wl + TT wt = inc  (rows 1, 2);  row 3 solid only
    cols = [(-ref[0], -ref[1], 0j * p), (wl[0], wl[1], wl[2]), (wt[0], wt[1], wt[2])]
    return _cramer3(cols, (inc[0], inc[1], 0j * p))


def solid_fluid(mode, p, r1, c1, r2, cl, ct):
    """solid -> fluid (incident mode ``mode`` in the solid along -n): (R_L, R_T, T_fluid)"""
    inc = _wave(mode, p, cl if mode == "L" else ct, ct, r2, -1)
    wl, wt = _wave("L", p, cl, ct, r2, +1), _wave("T", p, ct, ct, r2, +1)
    tf = _wave("L", p, c1, 0.0, r1, -1)
    # RL wl + RT wt - Tf tf = -inc   (sigma_tn of the fluid is 0)
    cols = [(wl[0], wl[1], wl[2]), (wt[0], wt[1], wt[2]), (-tf[0], -tf[1], 0j * p)]
    return _cramer3(cols, (-inc[0], -inc[1], -inc[2]))


def free(mode, p, r2, cl, ct):
    """free surface (incident mode ``mode`` along +n, n out of the solid): (R_L, R_T)"""
    inc = _wave(mode, p, cl if mode == "L" else ct, ct, r2, +1)
    wl, wt = _wave("L", p, cl, ct, r2, -1), _wave("T", p, ct, ct, r2, -1)
    d = wl[1] * wt[2] - wt[1] * wl[2]
    return (-inc[1] * wt[2] + wt[1] * inc[2]) / d, (-wl[1] * inc[2] + inc[1] * wl[2]) / d


def sinc(u):
    return np.sinc(u)


def _unit(x, z):
    n = np.hypot(x, z)
    return x / n, z / n, n


def _tube(segs, ifs):
    """J and the product of cos(out) / cos(in) of a ray tube: segs = [(dx, dz, length, c)], ifs = [(nx, nz, curv, reflect)] between
    them; (nx, nz) is the interface normal with its fixed orientation, curv = d(angle of that normal) / d(arc along (nz, -nx))"""
    W, Th, prod = 0.0, 1.0, 1.0
    for k, (dx, dz, L, c) in enumerate(segs):
        W = W + L * Th
        if k == len(ifs):
            break
        nx, nz, curv, refl = ifs[k]
        odx, odz, _, oc = segs[k + 1]
        cin = dx * nx + dz * nz
        flip = cin < 0                                     # orient the normal along the incoming ray
        sg = np.where(flip, -1.0, 1.0)
        cin = cin * sg
        cout = (odx * nx + odz * nz) * sg * (-1.0 if refl else 1.0)
        K = curv * sg                                      # flipped normal and tangent: d(angle) / d(arc) changes sign
        ds = W / cin
        dtin = Th - K * ds
        dtout = (oc * cin) / (c * cout) * dtin
        if refl:
            W, Th = -ds * cout, K * ds - dtout
        else:
            W, Th = ds * cout, K * ds + dtout
        prod = prod * cout / cin
    return W, prod


def amplitude(x0, dx, zs, media, leg, up, xe, ze, xf, zf, xent, xback=None, width=0.0, fc=1.0, parts=False):
    """the tabulated amplitude (complex128, broadcast over the inputs) of ``leg`` in direction ``up``; media = (c1, rho1, c_l, c_t,
    rho2, z_back)"""
    c1, r1, cl, ct, r2, zb = media
    sp = {"L": cl, "T": ct}
    coef = S.spline(x0, dx, np.asarray(zs, dtype=np.float64))
    xe, ze, xf, zf, xent = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (xe, ze, xf, zf, xent)))
    s, s1, s2 = S.spline_eval(coef, x0, dx, xent)
    nn = np.sqrt(1.0 + s1 * s1)
    nx, nz = -s1 / nn, 1.0 / nn
    tx, tz = nz, -nx
    kap = s2 / nn ** 3
    skip = len(leg) == 2
    X, Y = leg[0], leg[-1]
    # down: E -> S -> (B) -> F
    ex, ez, l1 = _unit(xent - xe, s - ze)
    if skip:
        xb = np.broadcast_to(np.asarray(xback, dtype=np.float64), xent.shape)
        bx, bz, l2 = _unit(xb - xent, zb - s)
        fx, fz, l3 = _unit(xf - xb, zf - zb)
        down = [(ex, ez, l1, c1), (bx, bz, l2, sp[X]), (fx, fz, l3, sp[Y])]
    else:
        fx, fz, l2 = _unit(xf - xent, zf - s)
        down = [(ex, ez, l1, c1), (fx, fz, l2, sp[X])]
    surf = (nx, nz, -kap, False)
    back = (0.0, 1.0, 0.0, True)
    if not up:
        segs, ifs = down, [surf] + ([back] if skip else [])
    else:
        segs = [(-a, -b, L, c) for a, b, L, c in down[::-1]]
        ifs = ([back] if skip else []) + [surf]
    J, prod = _tube(segs, ifs)
    with np.errstate(invalid="ignore", divide="ignore"):             # (paths that do not cross: zeroed below)
        G = np.sqrt(prod / np.abs(J))
    D = sinc(width * ex * fc / c1) if width > 0 else np.ones_like(ex)
    # coefficients: p from the incoming segment at each interface
    if not up:
        p = (ex * tx + ez * tz) / c1
        cs = fluid_solid(p, r1, c1, r2, cl, ct)[1 if X == "L" else 2]
        cb = 1.0
        if skip:
            pb = bx / sp[X]
            cb = free(X, pb, r2, cl, ct)[0 if Y == "L" else 1]
    else:
        cb = 1.0
        if skip:
            pb = -fx / sp[Y]                                # the wave leaves F along -(fx, fz)
            cb = free(Y, pb, r2, cl, ct)[0 if X == "L" else 1]
            ux, uz = -bx, -bz
        else:
            ux, uz = -fx, -fz
        p = (ux * tx + uz * tz) / sp[X]
        cs = solid_fluid(X, p, r1, c1, r2, cl, ct)[2]
    with np.errstate(invalid="ignore"):
        amp = np.conj(D * G * cs * cb)
        amp = np.where(J == 0, complex(np.inf, np.inf), amp)              # a caustic: +inf + inf i (include/rtus.h)
    ox, oz = (bx, bz) if skip else (fx, fz)
    # else not a refraction into the part: no ray, amplitude 0 (an infinite x_entry / x_back: the cosines are NaN, the test fails)
    with np.errstate(invalid="ignore"):
        crosses = (ex * nx + ez * nz > 0) & (ox * nx + oz * nz > 0)
    amp = np.where(crosses, amp, 0j)
    bad = np.isnan(xent) | (np.isnan(xb) if skip else False)
    amp = np.where(bad, np.nan + 1j * np.nan, amp)
    if parts:
        return amp, dict(D=D, G=G, J=J, prod=prod, cs=cs, cb=cb)
    return amp


# ---------------------------------------------------------------------------------------------- weighted delay-and-sum, fp64
def _tau(t, fs, half_t0s):
    v = (t * fs - half_t0s).astype(np.float32)
    with np.errstate(invalid="ignore"):
        ok = np.abs(v) < np.float32(1e8)
    return np.where(ok, v, np.float32(-1e8))


def tfm_weighted(a, fs, tt_tx, w_tx, tt_rx, w_rx, t0=0.0):
    """(S complex128 [n_f], P float64 [n_f]) with rtus_tfm_analytic's sample positions (fp32 taus, fp32 position) and edge rules,
    interpolation and sums in fp64; a leg with a non-finite weight has no path"""
    a = np.asarray(a)
    n_tx, n_rx, n_t = a.shape
    h = 0.5 * t0 * fs
    ttx, trx = _tau(np.asarray(tt_tx), fs, h), _tau(np.asarray(tt_rx), fs, h)
    w_tx, w_rx = np.asarray(w_tx, dtype=np.complex128), np.asarray(w_rx, dtype=np.complex128)
    okt = (ttx > np.float32(-1e8)) & np.isfinite(w_tx)
    okr = (trx > np.float32(-1e8)) & np.isfinite(w_rx)
    n_f = ttx.shape[1]
    Sm = np.zeros(n_f, dtype=np.complex128)
    ap = np.concatenate([a.astype(np.complex128), np.zeros((n_tx, n_rx, 1))], axis=2)
    for i in range(n_tx):
        for j in range(n_rx):
            ok = okt[i] & okr[j]
            s = np.where(ok, ttx[i] + trx[j], np.float32(-1.0)).astype(np.float32)
            fl = np.floor(s)
            w = (s - fl).astype(np.float64)
            k = fl.astype(np.int64)
            inr = (k >= 0) & (k < n_t)
            kk = np.clip(k, 0, n_t - 1)
            v = (1 - w) * ap[i, j, kk] + w * ap[i, j, kk + 1]
            Sm += np.where(inr & ok, np.where(ok, w_tx[i], 0) * np.where(ok, w_rx[j], 0) * v, 0)
    P = np.sum(np.where(okt, np.abs(np.where(okt, w_tx, 0)) ** 2, 0), axis=0) * \
        np.sum(np.where(okr, np.abs(np.where(okr, w_rx, 0)) ** 2, 0), axis=0)
    return Sm, P

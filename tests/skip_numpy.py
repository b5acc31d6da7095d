"""Independent NumPy oracle of rtus_tt_surface_skip (include/rtus.h): the skip leg of multi-view TFM through one curved front
surface — element -> couplant (c1) -> surface -> down at c_down to the planar backwall at z_back -> up at c_up to the point.
NumPy only; the spline is surface_numpy's.

Definition (the header's): with S(x) = (x, s(x)) and B = (xb, z_back),
    T(x) = |E - S(x)| / c1 + T_in(S(x)),   T_in(S) = min over xb of |S - B| / c_down + |B - F| / c_up;
the entry is the least T over the interior local minima of T; NaN without one, for an element with ze >= min s, for a focal point
outside the extent or not strictly between s(xf) and z_back, and everywhere when z_back <= max s.

Method (not the kernel's): the inner ray is solved in the scaled slowness u = c_down p by bisection of
f(u) = h1 u / a_d + h2 u / a_u - X (a_d = sqrt(1 - u^2), a_u = sqrt(kap^2 - u^2), kap = c_down / c_up) on (-umax, umax) and
polished by Newton steps, in fp64.  T' is sampled at SUB = 64 points per profile segment; every sign change is a stationary point,
refined by bisection and safeguarded Newton on T'.  Like surface_numpy, each entry also reports the winner's basin and the gap
to the runner-up.
"""
import numpy as np

import surface_numpy as S

SUB = 64


def spline_max(coef, dx):
    """greatest depth of the spline over the extent"""
    return -S.spline_min(-coef, dx)


def inner(h1, h2, X, c_down, c_up):
    """the inner ray: -> (u, a_d, a_u, f_u) with u = c_down p (fp64; bisection, then Newton steps kept inside the bracket)"""
    kap = c_down / c_up
    kap2, umax = kap * kap, min(1.0, kap)
    h1, h2, X = np.broadcast_arrays(np.asarray(h1, dtype=np.float64), np.asarray(h2, dtype=np.float64),
                                    np.asarray(X, dtype=np.float64))
    lo = np.full(h1.shape, -umax)
    hi = np.full(h1.shape, umax)

    def f_and_fu(u):
        with np.errstate(invalid="ignore", divide="ignore"):
            ad, au = np.sqrt(1.0 - u * u), np.sqrt(kap2 - u * u)
            return h1 * u / ad + h2 * u / au - X, h1 / ad ** 3 + h2 * kap2 / au ** 3
    for _ in range(45):
        mid = 0.5 * (lo + hi)
        neg = f_and_fu(mid)[0] < 0
        lo = np.where(neg, mid, lo)
        hi = np.where(neg, hi, mid)
    u = 0.5 * (lo + hi)
    for _ in range(3):
        f, fu = f_and_fu(u)
        with np.errstate(invalid="ignore", divide="ignore"):
            un = u - f / fu
        u = np.where(np.isfinite(un) & (un >= lo) & (un <= hi), un, u)
    with np.errstate(invalid="ignore"):
        ad, au = np.sqrt(1.0 - u * u), np.sqrt(kap2 - u * u)
    return u, ad, au, f_and_fu(u)[1]


def inner_leg(coef, x0, dx, x, xf, zf, zb, c_down, c_up):
    """T_in and its first two derivatives in x, and the reflection point's x"""
    s, s1, s2 = S.spline_eval(coef, x0, dx, x)
    h1, h2, X = zb - s, zb - zf, xf - x
    u, ad, au, fu = inner(h1, h2, X, c_down, c_up)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = (u * X + h1 * ad + h2 * au) / c_down
        d1 = -(u + ad * s1) / c_down
        w = 1.0 - s1 * u / ad
        d2 = (w * w / fu - ad * s2) / c_down
        xb = x + h1 * u / ad
    return t, d1, d2, xb


def travel(coef, x0, dx, c1, c_down, c_up, zb, xe, ze, xf, zf, x):
    """T, T', T'' at x"""
    a = S._legs(coef, x0, dx, x, xe, ze, c1)
    b = inner_leg(coef, x0, dx, x, xf, zf, zb, c_down, c_up)
    return a[0] + b[0], a[1] + b[1], a[2] + b[2]


def _refine(coef, x0, dx, c1, c_down, c_up, zb, xe, ze, xf, zf, lo, hi, kind):
    lo, hi = lo.copy(), hi.copy()
    for _ in range(36):
        mid = 0.5 * (lo + hi)
        d1 = travel(coef, x0, dx, c1, c_down, c_up, zb, xe, ze, xf, zf, mid)[1]
        right = (d1 * kind) < 0
        lo = np.where(right, mid, lo)
        hi = np.where(right, hi, mid)
    x = 0.5 * (lo + hi)
    for _ in range(3):
        _, d1, d2 = travel(coef, x0, dx, c1, c_down, c_up, zb, xe, ze, xf, zf, x)
        with np.errstate(invalid="ignore", divide="ignore"):
            xn = x - d1 / d2
        x = np.where(np.isfinite(xn) & (xn >= lo) & (xn <= hi), xn, x)
    return x


def stationary(x0, dx, zs, c1, c_down, c_up, zb, xe, ze, xf, zf, coef=None):
    """every stationary point of T per entry -> (entry e * n_f + f, x, kind (+1 min, -1 max), T), sorted by (entry, x)"""
    zs = np.asarray(zs, dtype=np.float64)
    coef = S.spline(x0, dx, zs) if coef is None else coef
    xe, ze, xf, zf = (np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in (xe, ze, xf, zf))
    n_f = xf.size
    X = x0 + dx * np.arange(SUB * (zs.size - 1) + 1) / SUB
    G = inner_leg(coef, x0, dx, X[None, :], xf[:, None], zf[:, None], zb, c_down, c_up)[1]       # [n_f, N]
    ent, lo, hi, kind = [], [], [], []
    for e in range(xe.size):
        D = S._legs(coef, x0, dx, X, xe[e], ze[e], c1)[1][None, :] + G
        for k, m in ((1, (D[:, :-1] < 0) & (D[:, 1:] >= 0)), (-1, (D[:, :-1] > 0) & (D[:, 1:] <= 0))):
            f, i = np.nonzero(m)
            ent.append(e * n_f + f)
            lo.append(X[i])
            hi.append(X[i + 1])
            kind.append(np.full(f.size, k))
    ent, lo, hi, kind = (np.concatenate(v) for v in (ent, lo, hi, kind))
    E, F = ent // n_f, ent % n_f
    x = _refine(coef, x0, dx, c1, c_down, c_up, zb, xe[E], ze[E], xf[F], zf[F], lo, hi, kind)
    t = travel(coef, x0, dx, c1, c_down, c_up, zb, xe[E], ze[E], xf[F], zf[F], x)[0]
    o = np.lexsort((x, ent))
    return ent[o], x[o], kind[o], t[o]


def table(x0, dx, zs, c1, c_down, c_up, zb, xe, ze, xf, zf, coef=None):
    """-> dict(t, x, xb, basin, gap), each [n_e, n_f]: time, winning entry point, its reflection point, basin, runner-up gap"""
    zs = np.asarray(zs, dtype=np.float64)
    coef = S.spline(x0, dx, zs) if coef is None else coef
    xe, ze, xf, zf = (np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in (xe, ze, xf, zf))
    n_e, n_f = xe.size, xf.size
    ent, x, kind, t = stationary(x0, dx, zs, c1, c_down, c_up, zb, xe, ze, xf, zf, coef)
    same_l = np.r_[False, ent[1:] == ent[:-1]]
    same_r = np.r_[ent[:-1] == ent[1:], False]
    dl = np.where(same_l, x - np.r_[np.nan, x[:-1]], np.inf)
    dr = np.where(same_r, np.r_[x[1:], np.nan] - x, np.inf)
    basin = 2.0 * np.minimum(dl, dr)
    out_t = np.full(n_e * n_f, np.nan)
    out_x = np.full(n_e * n_f, np.nan)
    out_b = np.full(n_e * n_f, np.inf)
    out_g = np.full(n_e * n_f, np.inf)
    mins = np.nonzero(kind == 1)[0]
    if mins.size:
        o = mins[np.lexsort((t[mins], ent[mins]))]
        first = np.r_[True, ent[o][1:] != ent[o][:-1]]
        w = o[first]
        out_t[ent[w]] = t[w]
        out_x[ent[w]] = x[w]
        out_b[ent[w]] = basin[w]
        second = ~first & np.r_[False, first[:-1]]
        r = o[second]
        out_g[ent[r]] = t[r] - out_t[ent[r]]
    xend = x0 + (zs.size - 1) * dx
    fs = S.spline_eval(coef, x0, dx, xf)[0]
    fok = (xf >= x0) & (xf <= xend) & (zf > fs) & (zf < zb)
    eok = ze < S.spline_min(coef, dx)
    ok = (eok[:, None] & fok[None, :]).reshape(-1) & (zb > spline_max(coef, dx))
    out_t[~ok] = np.nan
    out_x[~ok] = np.nan
    F = np.arange(n_e * n_f) % n_f
    win = np.isfinite(out_x)
    xb = np.where(win, inner_leg(coef, x0, dx, np.where(win, out_x, x0), xf[F], zf[F], zb, c_down, c_up)[3], np.nan)
    shp = (n_e, n_f)
    return dict(t=out_t.reshape(shp), x=out_x.reshape(shp), xb=xb.reshape(shp), basin=out_b.reshape(shp), gap=out_g.reshape(shp))


def table_chunked(x0, dx, zs, c1, c_down, c_up, zb, xe, ze, xf, zf, chunk=128):
    """table() over the focal points in chunks of ``chunk`` (the scan's arrays are [chunk, 64 (n_s - 1)] doubles), the spline
    solved once"""
    coef = S.spline(x0, dx, zs)
    xf, zf = np.atleast_1d(np.asarray(xf, dtype=np.float64)), np.atleast_1d(np.asarray(zf, dtype=np.float64))
    parts = [table(x0, dx, zs, c1, c_down, c_up, zb, xe, ze, xf[i:i + chunk], zf[i:i + chunk], coef) for i in range(0, xf.size, chunk)]
    return {k: np.concatenate([p[k] for p in parts], axis=1) for k in parts[0]}


def planar(xe, ze, z_s, zb, xf, zf, c1, c_down, c_up):
    """flat front at z_s: the closed tau-p form of the three-segment ray (couplant, down, up), solved by bisection on the
    horizontal slowness -> T (no validity rules)"""
    xe, ze, xf, zf = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in (xe, ze, xf, zf)))
    hs = np.stack([z_s - ze, np.full(ze.shape, zb - z_s), zb - zf])
    cs = np.array([c1, c_down, c_up])[:, None]
    hs = hs.reshape(3, -1)
    X = (xf - xe).reshape(-1)
    pmax = 1.0 / cs.max()
    lo, hi = np.full(X.shape, -pmax), np.full(X.shape, pmax)

    def xsum(p):
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.sum(hs * p * cs / np.sqrt(1.0 - (p * cs) ** 2), axis=0)
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lt = xsum(mid) < X
        lo = np.where(lt, mid, lo)
        hi = np.where(lt, hi, mid)
    p = 0.5 * (lo + hi)
    t = p * X + np.sum(hs * np.sqrt(1.0 / cs ** 2 - p * p), axis=0)
    return t.reshape(xe.shape)

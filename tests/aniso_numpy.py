"""Independent NumPy oracle of rtus_tt_aniso_surface and rtus_tt_aniso_direct (include/rtus.h): Fermat travel times through one
curved interface into an anisotropic part whose group slowness is a Fourier series of period pi in the ray angle.  NumPy only
(scipy may be missing on the GPU machine); the spline is tests/surface_numpy.py's.

Definition (the header's): T(x) = |E - S(x)| / c1 + |F - S(x)| S(psi(x)), S(x) = (x, s(x)), psi = atan2(F_x - x, F_z - s(x)),
S(psi) = a[0] + sum_k (a[k] cos 2k psi + b[k] sin 2k psi); the entry is the least T over the interior local minima of T, NaN
without one, for an element with ze >= min s, or for a focal point outside the extent or with zf <= s(xf).

Method (not the kernel's): the series is evaluated with np.cos / np.sin of 2 k psi and psi from np.arctan2 (no recurrence, no unit
vector); T' = T1' + L' S + L S_psi psi' is sampled at SUB = 64 points per profile segment; EVERY sign change is a stationary point
(- -> + a minimum, + -> - a maximum), refined by 60 bisections on T' alone — no second derivative anywhere.  For each entry it
also reports the winner's basin (twice the distance from the winning minimum to the nearer neighbouring stationary point, infinite
where the ends of the extent are the neighbours), the time gap to the runner-up minimum, the number of minima and the gap to the
third-least minimum (infinite without one).
"""
import numpy as np

import surface_numpy as S

SUB = 64


def series(a, b, psi):
    """S and dS/dpsi at psi"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    psi = np.asarray(psi, dtype=np.float64)
    s, s1 = np.full(psi.shape, a[0]), np.zeros(psi.shape)
    for k in range(1, a.size):
        c, sn = np.cos(2 * k * psi), np.sin(2 * k * psi)
        s = s + a[k] * c + b[k] * sn
        s1 = s1 + 2 * k * (b[k] * c - a[k] * sn)
    return s, s1


def leg1(coef, x0, dx, x, px, pz, c1):
    """|S(x) - E| / c1 and its derivative in x"""
    s, s1, _ = S.spline_eval(coef, x0, dx, x)
    ux, uz = x - px, s - pz
    L = np.sqrt(ux * ux + uz * uz)
    return L / c1, (ux + uz * s1) / (L * c1)


def leg2(coef, x0, dx, x, a, b, xf, zf):
    """|F - S(x)| S(psi) and its derivative in x"""
    s, s1, _ = S.spline_eval(coef, x0, dx, x)
    vx, vz = xf - x, zf - s
    L2 = vx * vx + vz * vz
    L = np.sqrt(L2)
    Sv, Sp = series(a, b, np.arctan2(vx, vz))
    with np.errstate(invalid="ignore", divide="ignore"):
        return L * Sv, -(vx + vz * s1) / L * Sv + L * Sp * (vx * s1 - vz) / L2


def travel(coef, x0, dx, c1, a, b, xe, ze, xf, zf, x):
    """T, T' at x"""
    p, q = leg1(coef, x0, dx, x, xe, ze, c1), leg2(coef, x0, dx, x, a, b, xf, zf)
    return p[0] + q[0], p[1] + q[1]


def _bisect(coef, x0, dx, c1, a, b, xe, ze, xf, zf, lo, hi, kind):
    """root of T' in [lo, hi] (kind +1 for - -> +, -1 for + -> -), vectorised over roots: 60 bisections"""
    lo, hi = lo.copy(), hi.copy()
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        d1 = travel(coef, x0, dx, c1, a, b, xe, ze, xf, zf, mid)[1]
        right = (d1 * kind) < 0
        lo = np.where(right, mid, lo)
        hi = np.where(right, hi, mid)
    return 0.5 * (lo + hi)


def stationary(x0, dx, zs, c1, a, b, xe, ze, xf, zf, coef=None):
    """every stationary point of T for every (element, focal point) entry -> (entry index e * n_f + f, x, kind (+1 min, -1 max), T)
    sorted by (entry, x); validity is NOT applied here"""
    zs = np.asarray(zs, dtype=np.float64)
    coef = S.spline(x0, dx, zs) if coef is None else coef
    xe, ze, xf, zf = (np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in (xe, ze, xf, zf))
    n_f = xf.size
    X = x0 + dx * np.arange(SUB * (zs.size - 1) + 1) / SUB
    G2 = leg2(coef, x0, dx, X[None, :], a, b, xf[:, None], zf[:, None])[1]          # [n_f, N]
    ent, lo, hi, kind = [], [], [], []
    for e in range(xe.size):
        D = leg1(coef, x0, dx, X, xe[e], ze[e], c1)[1][None, :] + G2
        for k, m in ((1, (D[:, :-1] < 0) & (D[:, 1:] >= 0)), (-1, (D[:, :-1] > 0) & (D[:, 1:] <= 0))):
            f, i = np.nonzero(m)
            ent.append(e * n_f + f)
            lo.append(X[i])
            hi.append(X[i + 1])
            kind.append(np.full(f.size, k))
    ent, lo, hi, kind = (np.concatenate(v) for v in (ent, lo, hi, kind))
    E, F = ent // n_f, ent % n_f
    x = _bisect(coef, x0, dx, c1, a, b, xe[E], ze[E], xf[F], zf[F], lo, hi, kind)
    t = travel(coef, x0, dx, c1, a, b, xe[E], ze[E], xf[F], zf[F], x)[0]
    o = np.lexsort((x, ent))
    return ent[o], x[o], kind[o], t[o]


def table(x0, dx, zs, c1, a, b, xe, ze, xf, zf):
    """-> dict(t, x, basin, gap, gap3, n_min), each [n_e, n_f]: travel time, winning entry point, winner's basin width, the
    runner-up's and the third-least minimum's time above the winner's, the number of interior minima (validity not applied to it)"""
    zs = np.asarray(zs, dtype=np.float64)
    coef = S.spline(x0, dx, zs)
    xe, ze, xf, zf = (np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in (xe, ze, xf, zf))
    n_e, n_f = xe.size, xf.size
    ent, x, kind, t = stationary(x0, dx, zs, c1, a, b, xe, ze, xf, zf, coef)
    same_l = np.r_[False, ent[1:] == ent[:-1]]
    same_r = np.r_[ent[:-1] == ent[1:], False]
    dl = np.where(same_l, x - np.r_[np.nan, x[:-1]], np.inf)
    dr = np.where(same_r, np.r_[x[1:], np.nan] - x, np.inf)
    basin = 2.0 * np.minimum(dl, dr)
    tot = n_e * n_f
    out_t, out_x = np.full(tot, np.nan), np.full(tot, np.nan)
    out_b, out_g, out_g3 = np.full(tot, np.inf), np.full(tot, np.inf), np.full(tot, np.inf)
    mins = np.nonzero(kind == 1)[0]
    n_min = np.bincount(ent[mins], minlength=tot)
    if mins.size:
        o = mins[np.lexsort((t[mins], ent[mins]))]               # minima by (entry, time)
        eo = ent[o]
        first = np.r_[True, eo[1:] != eo[:-1]]
        rank = np.arange(o.size) - np.maximum.accumulate(np.where(first, np.arange(o.size), 0))
        w = o[first]
        out_t[ent[w]] = t[w]
        out_x[ent[w]] = x[w]
        out_b[ent[w]] = basin[w]
        r = o[rank == 1]
        out_g[ent[r]] = t[r] - out_t[ent[r]]
        r = o[rank == 2]
        out_g3[ent[r]] = t[r] - out_t[ent[r]]
    xend = x0 + (zs.size - 1) * dx
    fs = S.spline_eval(coef, x0, dx, xf)[0]
    fok = (xf >= x0) & (xf <= xend) & (zf > fs)
    eok = ze < S.spline_min(coef, dx)
    ok = (eok[:, None] & fok[None, :]).reshape(-1)
    out_t[~ok] = np.nan
    out_x[~ok] = np.nan
    shp = (n_e, n_f)
    return dict(t=out_t.reshape(shp), x=out_x.reshape(shp), basin=out_b.reshape(shp), gap=out_g.reshape(shp),
                gap3=out_g3.reshape(shp), n_min=n_min.reshape(shp))


def direct(a, b, xe, ze, xf, zf):
    """contact: |F - E| S(atan2(dx, dz)) [n_e, n_f]; NaN for a non-finite coordinate, 0 at zero distance"""
    xe, ze, xf, zf = (np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in (xe, ze, xf, zf))
    with np.errstate(invalid="ignore"):
        vx, vz = xf[None, :] - xe[:, None], zf[None, :] - ze[:, None]
        t = np.hypot(vx, vz) * series(a, b, np.arctan2(vx, vz))[0]
    fin = np.isfinite(xe)[:, None] & np.isfinite(ze)[:, None] & np.isfinite(xf)[None, :] & np.isfinite(zf)[None, :]
    return np.where(fin, t, np.nan)

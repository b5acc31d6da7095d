"""Independent NumPy oracle of rtus_tt_surface (include/rtus.h): Fermat travel times through one curved interface, the natural
cubic spline through a sampled depth profile.  NumPy only (scipy may be missing on the GPU machine).

Definition (the header's): s(x) is the natural cubic spline through zs[k] at x0 + k dx on [x0, x0 + (n_s - 1) dx], z down;
T(x) = |E - S(x)| / c1 + |S(x) - F| / c2 with S(x) = (x, s(x)); the entry is the least T over the interior local minima of T,
NaN without one, for an element with ze >= min s, or for a focal point outside the extent or with zf <= s(xf).

Method (not the kernel's): T' is sampled at SUB = 64 points per profile segment; EVERY sign change is a stationary point
(- -> + a minimum, + -> - a maximum), refined by bisection to the bracket's resolution and then by safeguarded Newton steps in
fp64.  For each entry it also reports the winner's basin — twice the distance from the winning minimum to the nearer of its
neighbouring stationary points (infinite where an end of the extent is the neighbour on both sides) — and the time gap to
the runner-up minimum (infinite without one).
"""
import numpy as np

SUB = 64


def spline(x0, dx, zs):
    """coefficients [n_s - 1, 4] (a, b, c, d) of s(x_k + t) = a + b t + c t^2 + d t^3: natural spline, dense solve"""
    z = np.asarray(zs, dtype=np.float64)
    n = z.size
    A = np.zeros((n - 2, n - 2))
    i = np.arange(n - 2)
    A[i, i] = 4.0
    A[i[1:], i[1:] - 1] = 1.0
    A[i[:-1], i[:-1] + 1] = 1.0
    rhs = 6.0 * (z[2:] - 2.0 * z[1:-1] + z[:-2]) / (dx * dx)
    M = np.zeros(n)
    M[1:-1] = np.linalg.solve(A, rhs)
    a = z[:-1]
    b = (z[1:] - z[:-1]) / dx - dx * (2.0 * M[:-1] + M[1:]) / 6.0
    c = M[:-1] / 2.0
    d = (M[1:] - M[:-1]) / (6.0 * dx)
    return np.stack([a, b, c, d], axis=1)


def spline_eval(coef, x0, dx, x):
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        kf = np.floor((x - x0) / dx)
    k = np.clip(np.where(np.isnan(kf), 0.0, kf), 0, coef.shape[0] - 1).astype(np.int64)    # (NaN -> segment 0; the result is NaN)
    t = x - (x0 + k * dx)
    a, b, c, d = (coef[k, i] for i in range(4))
    return a + t * (b + t * (c + t * d)), b + t * (2 * c + 3 * t * d), 2 * c + 6 * t * d


def spline_min(coef, dx):
    """least depth of the spline over the extent: segment ends and the roots of s' inside each segment"""
    a, b, c, d = coef.T
    cand = [a, a + dx * (b + dx * (c + dx * d))]
    A, B = 3 * d, 2 * c
    with np.errstate(invalid="ignore", divide="ignore"):
        disc = B * B - 4 * A * b
        q = np.sqrt(np.where(disc >= 0, disc, np.nan))
        roots = [np.where(A != 0, (-B - q) / (2 * A), np.where(B != 0, -b / B, np.nan)),
                 np.where(A != 0, (-B + q) / (2 * A), np.nan)]
    for r in roots:
        ok = (r > 0) & (r < dx)
        rr = np.where(ok, r, 0.0)
        cand.append(np.where(ok, a + rr * (b + rr * (c + rr * d)), np.inf))
    return float(np.min(np.stack(cand)))


def _legs(coef, x0, dx, x, px, pz, c):
    """|S(x) - P| / c and its first two derivatives in x"""
    s, s1, s2 = spline_eval(coef, x0, dx, x)
    ux, uz = x - px, s - pz
    L = np.sqrt(ux * ux + uz * uz)
    A = ux + uz * s1
    return L / c, A / (L * c), ((1 + s1 * s1 + uz * s2) / L - A * A / L ** 3) / c


def travel(coef, x0, dx, c1, c2, xe, ze, xf, zf, x):
    """T, T', T'' at x"""
    a = _legs(coef, x0, dx, x, xe, ze, c1)
    b = _legs(coef, x0, dx, x, xf, zf, c2)
    return a[0] + b[0], a[1] + b[1], a[2] + b[2]


def _refine(coef, x0, dx, c1, c2, xe, ze, xf, zf, lo, hi, kind):
    """root of T' in [lo, hi] (T' changes sign there: kind +1 for - -> +, -1 for + -> -), vectorised over roots"""
    lo, hi = lo.copy(), hi.copy()
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        d1 = travel(coef, x0, dx, c1, c2, xe, ze, xf, zf, mid)[1]
        right = (d1 * kind) < 0                     # mid is still on the bracket's left side
        lo = np.where(right, mid, lo)
        hi = np.where(right, hi, mid)
    x = 0.5 * (lo + hi)
    for _ in range(3):                              # Newton, kept inside the bracket
        _, d1, d2 = travel(coef, x0, dx, c1, c2, xe, ze, xf, zf, x)
        with np.errstate(invalid="ignore", divide="ignore"):
            xn = x - d1 / d2
        x = np.where(np.isfinite(xn) & (xn >= lo) & (xn <= hi), xn, x)
    return x


def stationary(x0, dx, zs, c1, c2, xe, ze, xf, zf, coef=None):
    """every stationary point of T for every (element, focal point) entry -> (entry index e * n_f + f, x, kind (+1 min, -1 max), T)
    sorted by (entry, x); validity is NOT applied here"""
    zs = np.asarray(zs, dtype=np.float64)
    coef = spline(x0, dx, zs) if coef is None else coef
    n_s = zs.size
    xe, ze, xf, zf = (np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in (xe, ze, xf, zf))
    n_f = xf.size
    X = x0 + dx * np.arange(SUB * (n_s - 1) + 1) / SUB
    G2 = _legs(coef, x0, dx, X[None, :], xf[:, None], zf[:, None], c2)[1]          # [n_f, N]
    ent, lo, hi, kind = [], [], [], []
    for e in range(xe.size):
        D = _legs(coef, x0, dx, X, xe[e], ze[e], c1)[1][None, :] + G2
        for k, m in ((1, (D[:, :-1] < 0) & (D[:, 1:] >= 0)), (-1, (D[:, :-1] > 0) & (D[:, 1:] <= 0))):
            f, i = np.nonzero(m)
            ent.append(e * n_f + f)
            lo.append(X[i])
            hi.append(X[i + 1])
            kind.append(np.full(f.size, k))
    ent, lo, hi, kind = (np.concatenate(v) for v in (ent, lo, hi, kind))
    E, F = ent // n_f, ent % n_f
    x = _refine(coef, x0, dx, c1, c2, xe[E], ze[E], xf[F], zf[F], lo, hi, kind)
    t = travel(coef, x0, dx, c1, c2, xe[E], ze[E], xf[F], zf[F], x)[0]
    o = np.lexsort((x, ent))
    return ent[o], x[o], kind[o], t[o]


def table(x0, dx, zs, c1, c2, xe, ze, xf, zf, coef=None):
    """-> dict(t, x, basin, gap), each [n_e, n_f]: travel time, winning entry point, winner's basin width, runner-up gap"""
    zs = np.asarray(zs, dtype=np.float64)
    coef = spline(x0, dx, zs) if coef is None else coef
    xe, ze, xf, zf = (np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in (xe, ze, xf, zf))
    n_e, n_f = xe.size, xf.size
    ent, x, kind, t = stationary(x0, dx, zs, c1, c2, xe, ze, xf, zf, coef)
    n = ent.size
    same_l = np.r_[False, ent[1:] == ent[:-1]]
    same_r = np.r_[ent[:-1] == ent[1:], False]
    dl = np.where(same_l, x - np.r_[np.nan, x[:-1]], np.inf)
    dr = np.where(same_r, np.r_[x[1:], np.nan] - x, np.inf)
    basin = 2.0 * np.minimum(dl, dr)
    out_t = np.full(n_e * n_f, np.nan)
    out_x = np.full(n_e * n_f, np.nan)
    out_b = np.full(n_e * n_f, np.inf)
    out_g = np.full(n_e * n_f, np.inf)
    mins = np.nonzero(kind == 1)[0] if n else np.zeros(0, dtype=np.int64)
    if mins.size:
        o = mins[np.lexsort((t[mins], ent[mins]))]               # minima by (entry, time)
        first = np.r_[True, ent[o][1:] != ent[o][:-1]]
        w = o[first]
        out_t[ent[w]] = t[w]
        out_x[ent[w]] = x[w]
        out_b[ent[w]] = basin[w]
        second = ~first & np.r_[False, first[:-1]]              # the runner-up: directly after a winner, same entry
        r = o[second]
        out_g[ent[r]] = t[r] - out_t[ent[r]]
    xend = x0 + (zs.size - 1) * dx
    fs = spline_eval(coef, x0, dx, xf)[0]
    fok = (xf >= x0) & (xf <= xend) & (zf > fs)
    eok = ze < spline_min(coef, dx)
    ok = (eok[:, None] & fok[None, :]).reshape(-1)
    out_t[~ok] = np.nan
    out_x[~ok] = np.nan
    shp = (n_e, n_f)
    return dict(t=out_t.reshape(shp), x=out_x.reshape(shp), basin=out_b.reshape(shp), gap=out_g.reshape(shp))


def table_chunked(x0, dx, zs, c1, c2, xe, ze, xf, zf, chunk=256):
    """table() over the focal points in chunks of ``chunk`` (stationary()'s arrays are [chunk, 64 (n_s - 1)] doubles), the spline
    solved once"""
    coef = spline(x0, dx, zs)
    xf, zf = np.atleast_1d(np.asarray(xf, dtype=np.float64)), np.atleast_1d(np.asarray(zf, dtype=np.float64))
    parts = [table(x0, dx, zs, c1, c2, xe, ze, xf[i:i + chunk], zf[i:i + chunk], coef) for i in range(0, xf.size, chunk)]
    return {k: np.concatenate([p[k] for p in parts], axis=1) for k in parts[0]}


def count_minima(x0, dx, zs, c1, c2, xe, ze, xf, zf, chunk=256):
    """[n_e, n_f] number of interior local minima of T per entry (validity not applied), over the focal points in chunks"""
    coef = spline(x0, dx, zs)
    xe = np.atleast_1d(np.asarray(xe, dtype=np.float64))
    xf, zf = np.atleast_1d(np.asarray(xf, dtype=np.float64)), np.atleast_1d(np.asarray(zf, dtype=np.float64))
    out = np.zeros((xe.size, xf.size), dtype=np.int64)
    for i in range(0, xf.size, chunk):
        n = min(chunk, xf.size - i)
        ent, _, kind, _ = stationary(x0, dx, zs, c1, c2, xe, ze, xf[i:i + n], zf[i:i + n], coef)
        out[:, i:i + n] = np.bincount(ent[kind == 1], minlength=xe.size * n).reshape(xe.size, n)
    return out


def minima(x0, dx, zs, c1, c2, xe, ze, xf, zf):
    """all interior local minima of one entry -> [(x, T)], by x"""
    ent, x, kind, t = stationary(x0, dx, zs, c1, c2, [xe], [ze], [xf], [zf])
    return [(float(a), float(b)) for a, b, k in zip(x, t, kind) if k == 1]

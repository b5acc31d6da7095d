"""fp64 NumPy model of rtus_surface.hip's SELECTION rule — which - -> + brackets of T' the scan sees, how it ranks them and which
of the kept ones it refines — generic over the mode's T(x), and the constructors of the inputs that tests/test_surface_select_cpu.py
and tests/test_gpu_surface_branches.py share.  NumPy only.

The model exists to CONSTRUCT inputs and to ASSERT that they sit on a branch of the kernel.  Kernel results are compared with the
oracles (surface_numpy.table, skip_numpy.table, pwi_numpy.surface), never with the model.

A mode is a callable f(i, x) -> (T, T', T'') over entry indices i and positions x (broadcasting): elem_T, skip_T, pw_T below wrap
surface_numpy.travel, skip_numpy.travel and pwi_numpy._pw_T.

select(f, n, x0, dx, n_s, rule=...):  per entry
  * the signs of T' at the scan points P_j = x0 + j dx / 4 (T' = 0 counts as -, a NaN as neither; plane waves: a scan point
    outside the insonified band is neither side of a bracket),
  * the brackets (T'(P_j-1) <= 0, T'(P_j) > 0), each with the scan's figure; the three least figures are kept (ties: the one
    further left, as the kernel's strict compare),
  * ranks 0 and 1 are refined always, rank 2 under the rule:
      "bound" (the kernel): the figure is T(P_j) - (dx / 4) T'(P_j), a lower bound of the minimum's time; rank 2 is refined
               unless its bound is later than the best REFINED time of ranks 0 and 1 by more than 4e-6 relative,
      "estimate" (the kernel before tests/test_gpu_surface_branches.py): the figure is T(P_j); rank 2 is refined only if it
               is within 4e-6 relative of rank 0's figure,
      "all": the figure is T(P_j), rank 2 is refined always,
  * the entry is the least refined time (plane waves: over refined roots inside the band).
It returns the pick and, for EVERY bracket, the refined (x, T), the figure and its fate.

stationary(f, n, x0, dx, n_s): every stationary point of T on a dense grid (64 points per segment, the oracles' method), for the
conditions the oracles' tables do not report (all minima of an entry and their neighbours).
"""
from functools import lru_cache

import numpy as np

import pwi_numpy as P
import skip_numpy as K
import surface_numpy as S

SUB_SCAN = 4                 # SURF_SUB
KEEP = 3                     # SURF_K
GATE = 4e-6                  # the parent kernel's fp32 ranking margin, relative to the best estimate
TILE = 64                    # SURF_TILE
REFINED, GATED, DROPPED, OFFBAND = 0, 1, 2, 3

C1, CL, CT = 1480.0, 5900.0, 3230.0          # water over steel


# ------------------------------------------------------------------------------------------------------------ the modes' T(x)
def _per_entry(v):
    """a per-entry parameter: a scalar for all entries, or an array indexed by the entry"""
    v = np.asarray(v, dtype=np.float64)
    return (lambda i: v) if v.ndim == 0 else (lambda i: v[i])


def elem_T(coef, x0, dx, c1, c2, xe, ze, xf, zf):
    xe, ze, xf, zf = (_per_entry(v) for v in (xe, ze, xf, zf))
    return lambda i, x: S.travel(coef, x0, dx, c1, c2, xe(i), ze(i), xf(i), zf(i), x)


def skip_T(coef, x0, dx, c1, c_down, c_up, zb, xe, ze, xf, zf):
    xe, ze, xf, zf = (_per_entry(v) for v in (xe, ze, xf, zf))
    return lambda i, x: K.travel(coef, x0, dx, c1, c_down, c_up, zb, xe(i), ze(i), xf(i), zf(i), x)


def pw_T(coef, x0, dx, c1, c2, angle, x_lo, x_hi, z_a, xf, zf):
    sn, cs, xref, _ = P.aperture_ref(angle, x_lo, x_hi)
    if np.ndim(angle) == 0:
        sn, cs, xref = sn[0], cs[0], xref[0]
    sn, cs, xref, xf, zf = (_per_entry(v) for v in (sn, cs, xref, xf, zf))
    return lambda i, x: P._pw_T(coef, x0, dx, c1, c2, sn(i), cs(i), xref(i), z_a, xf(i), zf(i), x)


def pw_band(coef, x0, dx, angle, x_lo, x_hi, z_a):
    """x -> whether the entry point x is insonified (the ray traced back along the incident direction meets the aperture)"""
    tn = np.tan(angle)

    def band(x):
        xb = x - (S.spline_eval(coef, x0, dx, x)[0] - z_a) * tn
        return (xb >= x_lo) & (xb <= x_hi)
    return band


# ------------------------------------------------------------------------------------------------------------ root refinement
def _refine(f, i, lo, hi, kind):
    """roots of T' in [lo, hi] (kind +1: - -> +, -1: + -> -), flat over brackets: bisection to ~1e-8 of the bracket, then Newton"""
    lo, hi = lo.copy(), hi.copy()
    for _ in range(16):
        mid = 0.5 * (lo + hi)
        right = (f(i, mid)[1] * kind) < 0
        lo = np.where(right, mid, lo)
        hi = np.where(right, hi, mid)
    x = 0.5 * (lo + hi)
    for _ in range(5):
        _, d1, d2 = f(i, x)
        with np.errstate(invalid="ignore", divide="ignore"):
            xn = x - d1 / d2
        x = np.where(np.isfinite(xn) & (xn >= lo) & (xn <= hi), xn, x)
    return x


def scan_points(x0, dx, n_s):
    return x0 + (dx / SUB_SCAN) * np.arange(SUB_SCAN * (n_s - 1) + 1)


def select(f, n, x0, dx, n_s, band=None, rule="bound"):
    """the kernel's selection over n entries -> dict of
         t, x [n]: the pick (NaN without a refined in-band bracket);  best [n]: the least T over ALL brackets' in-band roots;
         late [n]: t - best (0 where both NaN; inf where only the pick is NaN);  n_br [n]: brackets seen;
         ent, j, est, xr, tr, fate, rank: flat over every bracket, sorted by (entry, figure): its entry, the scan index of its right
         end, the scan's figure, its refined root and time, and REFINED / GATED (kept third, not refined) / DROPPED (4th or
         later) / OFFBAND (refined, root outside the band)"""
    Pj = scan_points(x0, dx, n_s)
    ii = np.arange(n)[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        T, D, _ = f(ii, Pj[None, :])
    T, D = np.broadcast_to(T, (n, Pj.size)), np.broadcast_to(D, (n, Pj.size))
    inb = np.broadcast_to(band(Pj)[None, :] if band is not None else True, D.shape)
    pos = (D > 0) & inb
    neg = ~(D > 0) & ~np.isnan(D) & inb                     # (the kernel's neg is "not +", a NaN sign included: NaN only for a
    br = pos[:, 1:] & neg[:, :-1]                           # point the kernel rejects before the scan; the model takes valid input)
    ent, jj = np.nonzero(br)
    jj = jj + 1
    est = T[ent, jj] - (dx / SUB_SCAN) * D[ent, jj] if rule == "bound" else T[ent, jj]
    o = np.lexsort((jj, est, ent))                          # by entry, then figure, then position
    ent, jj, est = ent[o], jj[o], est[o]
    first = np.r_[True, ent[1:] != ent[:-1]]
    start = np.maximum.accumulate(np.where(first, np.arange(ent.size), 0)) if ent.size else np.zeros(0, dtype=np.int64)
    rank = np.arange(ent.size) - start
    fate = np.where(rank >= KEEP, DROPPED, REFINED)
    xr = _refine(f, ent, Pj[jj - 1], Pj[jj], np.ones(ent.size)) if ent.size else np.zeros(0)
    tr = f(ent, xr)[0] if ent.size else np.zeros(0)
    counts = band(xr) if band is not None and ent.size else np.ones(ent.size, dtype=bool)
    if rule == "estimate" and ent.size:
        fate = np.where((rank == KEEP - 1) & ~(est <= est[start] * (1.0 + GATE)), GATED, fate)
    elif rule == "bound" and ent.size:
        best01 = np.full(n, np.inf)                         # the best refined in-band time of ranks 0 and 1 (inf: none)
        np.minimum.at(best01, ent[(rank < KEEP - 1) & counts], tr[(rank < KEEP - 1) & counts])
        fate = np.where((rank == KEEP - 1) & (est > best01[ent] * (1.0 + GATE)), GATED, fate)
    fate = np.where(~counts & (fate == REFINED), OFFBAND, fate)
    t, x, best = np.full(n, np.inf), np.full(n, np.nan), np.full(n, np.inf)
    for k in np.argsort(-tr, kind="stable"):                # (later times first: the least one is written last)
        if counts[k]:
            best[ent[k]] = tr[k]
            if fate[k] == REFINED:
                t[ent[k]], x[ent[k]] = tr[k], xr[k]
    with np.errstate(invalid="ignore"):
        late = np.where(np.isinf(best), 0.0, t - best)
    t, best = np.where(np.isinf(t), np.nan, t), np.where(np.isinf(best), np.nan, best)
    return dict(t=t, x=x, best=best, late=late, n_br=np.bincount(ent, minlength=n), ent=ent, j=jj, est=est, xr=xr, tr=tr, fate=fate,
                rank=rank)


def stationary(f, n, x0, dx, n_s, sub=64):
    """every stationary point of T over n entries on a grid of ``sub`` points per segment -> (entry, x, kind (+1 min, -1 max), T),
    sorted by (entry, x)"""
    X = x0 + dx * np.arange(sub * (n_s - 1) + 1) / sub
    with np.errstate(invalid="ignore", divide="ignore"):
        D = np.broadcast_to(f(np.arange(n)[:, None], X[None, :])[1], (n, X.size))
    ent, lo, hi, kind = [], [], [], []
    for k, m in ((1, (D[:, :-1] < 0) & (D[:, 1:] >= 0)), (-1, (D[:, :-1] > 0) & (D[:, 1:] <= 0))):
        e, i = np.nonzero(m)
        ent.append(e); lo.append(X[i]); hi.append(X[i + 1]); kind.append(np.full(e.size, k))
    ent, lo, hi, kind = (np.concatenate(v) for v in (ent, lo, hi, kind))
    x = _refine(f, ent, lo, hi, kind)
    t = f(ent, x)[0]
    o = np.lexsort((x, ent))
    return ent[o], x[o], kind[o], t[o]


# ------------------------------------------------------------------------------------------------------------ C1: three near-tied minima
X0, DX, NS = -0.02, 1e-3, 41
Z0 = 0.02


def bumps(centres, amps, width, x0=X0, dx=DX, n_s=NS, z0=Z0):
    """a flat profile at z0 with raised-cosine bumps TOWARDS the array (less couplant: each hosts a minimum of T): depth samples"""
    x = x0 + dx * np.arange(n_s)
    z = np.full(n_s, z0)
    for c, a in zip(centres, amps):
        u = (x - c) / width
        z = z - a * np.where(np.abs(u) < 0.5, 0.5 * (1.0 + np.cos(2.0 * np.pi * u)), 0.0)
    return z


# per mode: the bumps' centres, starting heights and width, the element (or the angle and the aperture), the tie point F*
TIE = {
    "elem": dict(centres=(-0.0062, 0.0004, 0.0069), amps=(0.0014, 0.0006, 0.0014), width=0.006, xe=0.0007, ze=-0.03, F=(0.0005, 0.035)),
    "skip": dict(centres=(-0.0062, 0.0004, 0.0069), amps=(0.0014, 0.0006, 0.0014), width=0.006, xe=0.0007, ze=-0.03, F=(0.0005, 0.027),
                 zb=Z0 + 0.010),
    "pw": dict(centres=(-0.0062, 0.0004, 0.0069), amps=(0.0010, 0.0006, 0.0010), width=0.006, angle=0.02, x_lo=-0.015, x_hi=0.015,
               z_a=0.0, F=(0.0005, 0.035)),
}
PATCH_N = 25


def tie_mode(mode, zs, xf, zf):
    """(f, band, n) of ``mode``'s one row over the focal points"""
    c = TIE[mode]
    coef = S.spline(X0, DX, zs)
    if mode == "elem":
        return elem_T(coef, X0, DX, C1, CL, c["xe"], c["ze"], xf, zf), None
    if mode == "skip":
        return skip_T(coef, X0, DX, C1, CL, CT, c["zb"], c["xe"], c["ze"], xf, zf), None
    return (pw_T(coef, X0, DX, C1, CL, c["angle"], c["x_lo"], c["x_hi"], c["z_a"], xf, zf),
            pw_band(coef, X0, DX, c["angle"], c["x_lo"], c["x_hi"], c["z_a"]))


def _dip_times(mode, amps):
    """the time of the minimum hosted by each of the three bumps at F* (NaN where a bump hosts none)"""
    c = TIE[mode]
    zs = bumps(c["centres"], amps, c["width"])
    f, _ = tie_mode(mode, zs, [c["F"][0]], [c["F"][1]])
    _, x, kind, t = stationary(f, 1, X0, DX, NS)
    out = []
    for cen in c["centres"]:
        m = (kind == 1) & (np.abs(x - cen) < 0.4 * c["width"])
        out.append(t[m].min() if m.any() else np.nan)
    return np.array(out)


@lru_cache(maxsize=None)
def tie_profile(mode):
    """the two outer bumps' heights tuned by a two-unknown Newton (finite-difference Jacobian) until the three minima's times agree
    at F* -> (zs, amps, steps, residual [s])"""
    c = TIE[mode]
    a = np.array(c["amps"], dtype=np.float64)
    h = 1e-7
    for step in range(25):
        t = _dip_times(mode, a)
        r = np.array([t[0] - t[1], t[2] - t[1]])
        if np.max(np.abs(r)) < 1e-15:
            break
        J = np.zeros((2, 2))
        for k, i in enumerate((0, 2)):
            b = a.copy()
            b[i] += h
            tb = _dip_times(mode, b)
            J[:, k] = (np.array([tb[0] - tb[1], tb[2] - tb[1]]) - r) / h
        d = np.linalg.solve(J, -r)
        a[0] += d[0]
        a[2] += d[1]
    t = _dip_times(mode, a)
    res = float(max(abs(t[0] - t[1]), abs(t[2] - t[1])))
    return bumps(c["centres"], a, c["width"]), a, step, res


def tie_patch(mode, half=60e-6, n=PATCH_N):
    """the n x n focal points around F*"""
    fx, fz = TIE[mode]["F"]
    gx, gz = np.meshgrid(fx + np.linspace(-half, half, n), fz + np.linspace(-half, half, n))
    return gx.ravel(), gz.ravel()


def _nth_least(ent, t, n, k):
    """[n] the k-th least (0-based) of t per entry, inf where an entry has fewer"""
    out = np.full(n, np.inf)
    o = np.lexsort((t, ent))
    e, tt = ent[o], t[o]
    first = np.r_[True, e[1:] != e[:-1]]
    start = np.maximum.accumulate(np.where(first, np.arange(e.size), 0))
    sel = (np.arange(e.size) - start) == k
    out[e[sel]] = tt[sel]
    return out


@lru_cache(maxsize=None)
def tie_case(mode):
    """everything the CPU and GPU tests of C1 share: the tuned profile, the patch, the oracle's table, the model's picks under
    the three rules, and the conditions on the input (computed from the dense stationary points):
      sep      [n] the entry's three least minima sit on three different bumps
      clear    [n] the least distance from one of those three minima to a neighbouring stationary point (plane waves: or to a
                   scan-grid band edge)
      fourth   [n] time of the fourth minimum less that of the third (inf without a fourth)
      gap      [n] runner-up's time less the winner's
      slope    max |s'| over the extent"""
    c = TIE[mode]
    zs, amps, steps, res = tie_profile(mode)
    xf, zf = tie_patch(mode)
    n = xf.size
    coef = S.spline(X0, DX, zs)
    f, band = tie_mode(mode, zs, xf, zf)
    if mode == "elem":
        o = S.table(X0, DX, zs, C1, CL, [c["xe"]], [c["ze"]], xf, zf)
    elif mode == "skip":
        o = K.table(X0, DX, zs, C1, CL, CT, c["zb"], [c["xe"]], [c["ze"]], xf, zf)
    else:
        o = P.surface(X0, DX, zs, C1, CL, [c["angle"]], c["x_lo"], c["x_hi"], c["z_a"], xf, zf)
    # (the bumps' stationary points are millimetres apart: 16 points per segment find them; the oracle's own 64 are in o)
    ent, x, kind, t = stationary(f, n, X0, DX, NS, sub=16)
    same_l = np.r_[False, ent[1:] == ent[:-1]]
    same_r = np.r_[ent[:-1] == ent[1:], False]
    near = np.minimum(np.where(same_l, x - np.r_[np.nan, x[:-1]], np.inf), np.where(same_r, np.r_[x[1:], np.nan] - x, np.inf))
    mn = kind == 1
    if band is not None:
        mn &= band(x)
        Pd = X0 + DX * np.arange(64 * (NS - 1) + 1) / 64
        inb = band(Pd)
        edges = Pd[np.nonzero(inb[1:] != inb[:-1])[0]]
        if edges.size:
            near = np.minimum(near, np.min(np.abs(x[:, None] - edges[None, :]), axis=1))
    e3, t3, x3, near3 = ent[mn], t[mn], x[mn], near[mn]
    third = _nth_least(e3, t3, n, 2)
    top = t3 <= third[e3]                                      # the entry's three least minima
    bump = np.argmin(np.abs(x3[:, None] - np.array(c["centres"])[None, :]), axis=1)
    on = np.abs(x3 - np.array(c["centres"])[bump]) < 0.4 * c["width"]
    sep = np.zeros(n, dtype=bool)
    clear = np.full(n, np.inf)
    for i in range(n):
        s = top & (e3 == i)
        sep[i] = s.sum() == 3 and on[s].all() and set(bump[s]) == {0, 1, 2}
        clear[i] = near3[s].min() if s.any() else np.inf
    xx = np.linspace(X0, X0 + (NS - 1) * DX, 64 * (NS - 1) + 1)
    return dict(mode=mode, zs=zs, amps=amps, steps=steps, res=res, xf=xf, zf=zf, o=o, sep=sep, clear=clear,
                fourth=_nth_least(e3, t3, n, 3) - third, gap=_nth_least(e3, t3, n, 1) - _nth_least(e3, t3, n, 0),
                least=_nth_least(e3, t3, n, 0), slope=float(np.abs(S.spline_eval(coef, X0, DX, xx)[1]).max()),
                gated=select(f, n, X0, DX, NS, band=band, rule="estimate"), ungated=select(f, n, X0, DX, NS, band=band, rule="all"),
                kernel=select(f, n, X0, DX, NS, band=band, rule="bound"))


def winners(f, n, x0, dx, n_s, band=None):
    """the oracles' definition per entry, from the dense stationary points -> dict(t, x, basin, gap) [n]: the least (in-band)
    minimum, its basin (twice the distance to the nearer neighbouring stationary point or band edge) and the runner-up's gap"""
    ent, x, kind, t = stationary(f, n, x0, dx, n_s)
    same_l = np.r_[False, ent[1:] == ent[:-1]]
    same_r = np.r_[ent[:-1] == ent[1:], False]
    near = np.minimum(np.where(same_l, x - np.r_[np.nan, x[:-1]], np.inf), np.where(same_r, np.r_[x[1:], np.nan] - x, np.inf))
    mn = kind == 1
    if band is not None:
        mn &= band(x)
        Pd = x0 + dx * np.arange(64 * (n_s - 1) + 1) / 64
        inb = band(Pd)
        edges = Pd[np.nonzero(inb[1:] != inb[:-1])[0]] + 0.5 * dx / 64
        if edges.size:
            near = np.minimum(near, np.min(np.abs(x[:, None] - edges[None, :]), axis=1))
    out = dict(t=np.full(n, np.nan), x=np.full(n, np.nan), basin=np.full(n, np.inf), gap=np.full(n, np.inf))
    e, tm, xm, nm = ent[mn], t[mn], x[mn], near[mn]
    if e.size == 0:
        return out
    o = np.lexsort((tm, e))
    e, tm, xm, nm = e[o], tm[o], xm[o], nm[o]
    first = np.r_[True, e[1:] != e[:-1]]
    out["t"][e[first]], out["x"][e[first]], out["basin"][e[first]] = tm[first], xm[first], 2.0 * nm[first]
    second = ~first & np.r_[False, first[:-1]]
    out["gap"][e[second]] = tm[second] - out["t"][e[second]]
    return out


# ------------------------------------------------------------------------------------------------------------ C2: roots on scan points
ZB_OFF = 0.010                                                 # skip legs: the backwall this far below the profile's mean depth
C2_NS = (4, 17, 33, 41)
C2_OFFS = (0.0, -1e-8, 1e-8)                                   # the root on the scan point and its two neighbours
C2_L = (0.005, 0.015, 0.025)                                   # lengths of the refracted ray to F
PW_APERTURE = (-0.03, 0.03, 0.0)                               # x_lo, x_hi, z_a


def c2_profile(n_s):
    """-> x0, dx, zs: n_s = 4 a gentle cubic on a 4 mm grid (13 scan points), else a gentle wave on a 1 mm grid"""
    if n_s == 4:
        dx, x0 = 4e-3, -6e-3
        u = (x0 + dx * np.arange(4)) / 6e-3
        return x0, dx, Z0 + 3e-4 * u + 4e-4 * u ** 3
    dx = 1e-3
    x0 = -0.5 * (n_s - 1) * dx
    x = x0 + dx * np.arange(n_s)
    return x0, dx, Z0 + 5e-4 * np.sin(2 * np.pi * x / 0.016 + 0.3)


def c2_scan_indices(n_s, n_random=12):
    """the scan points that get a root: the first and last interior ones, the tile seams this profile has, n_random random ones"""
    m = SUB_SCAN * (n_s - 1) + 1
    js = [1, m - 2] + [j for j in (TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE) if 1 < j < m - 2]
    rng = np.random.default_rng(100 + n_s)
    rest = np.setdiff1d(np.arange(2, m - 2), js)
    return np.array(js + sorted(rng.choice(rest, min(n_random, rest.size), replace=False).tolist()))


C2_ROWS = 16                                                   # two row blocks of 8


def c2_elements(n_s):
    """16 elements from 3 mm left of the extent to 3 mm right of it: a root in the first or the last scan cell needs an element
    outside the extent for its refracted ray to head inwards"""
    x0, dx, _ = c2_profile(n_s)
    h = 0.5 * (n_s - 1) * dx
    return np.linspace(-h - 0.003, h + 0.003, C2_ROWS), np.zeros(C2_ROWS)


C2_ANGLES = np.linspace(-0.24, 0.24, C2_ROWS)


def _refract(mode, coef, x0, dx, xs, src, L):
    """Snell's law in the spline's tangent frame at the surface points xs: the ray from the element src = (xe, ze) — plane waves:
    the angle src — refracted into the part (CL), followed for the length L -> (xf, zf, ok); skip legs: down to the backwall,
    reflected with conversion to CT, and up by a share of the way set by L"""
    s, s1, _ = S.spline_eval(coef, x0, dx, xs)
    nrm = np.sqrt(1.0 + s1 * s1)
    tx, tz, nx, nz = 1.0 / nrm, s1 / nrm, -s1 / nrm, 1.0 / nrm            # unit tangent, unit normal into the part (z down)
    if mode == "pw":
        d1x, d1z = np.sin(src) * np.ones_like(xs), np.cos(src) * np.ones_like(xs)
    else:
        d1x, d1z = xs - src[0], s - src[1]
        r = np.hypot(d1x, d1z)
        d1x, d1z = d1x / r, d1z / r
    sin1 = d1x * tx + d1z * tz
    sin2 = sin1 * CL / C1
    ok = (np.abs(sin2) < 0.9) & (d1x * nx + d1z * nz > 0.2)               # sin(theta_1) < 0.9 c1 / c2
    cos2 = np.sqrt(np.where(ok, 1.0 - sin2 * sin2, 1.0))
    d2x, d2z = sin2 * tx + cos2 * nx, sin2 * tz + cos2 * nz
    if mode != "skip":
        return xs + L * d2x, s + L * d2z, ok & (d2z > 0)
    zb = Z0 + ZB_OFF
    ok &= d2z > 0.2
    d2z = np.where(ok, d2z, 1.0)
    xb = xs + (zb - s) * d2x / d2z
    pu = np.clip(d2x * CT / CL, -0.99, 0.99)                              # sin of the up-going ray (horizontal slowness conserved)
    rise = ZB_OFF * (0.2 + 20.0 * L)                                      # (L = 5 .. 25 mm -> 30 % .. 70 % of the way up)
    return xb + rise * pu / np.sqrt(1.0 - pu * pu), zb - rise, ok


def _c2_winners(mode, c, R, xf, zf):
    """the dense oracle's winner of each (row R, focal point) pair"""
    x0, dx, n_s, coef = c["x0"], c["dx"], c["zs"].size, c["coef"]
    if mode == "skip":
        return winners(skip_T(coef, x0, dx, C1, CL, CT, c["zb"], c["xe"][R], c["ze"][R], xf, zf), R.size, x0, dx, n_s)
    if mode == "elem":
        return winners(elem_T(coef, x0, dx, C1, CL, c["xe"][R], c["ze"][R], xf, zf), R.size, x0, dx, n_s)
    w = dict(t=np.full(R.size, np.nan), x=np.full(R.size, np.nan), basin=np.zeros(R.size), gap=np.zeros(R.size))
    for a in np.unique(R):
        sel = np.nonzero(R == a)[0]
        band = pw_band(coef, x0, dx, c["ang"][a], *PW_APERTURE)
        wa = winners(pw_T(coef, x0, dx, C1, CL, c["ang"][a], *PW_APERTURE, xf[sel], zf[sel]), sel.size, x0, dx, n_s, band)
        for k in w:
            w[k][sel] = wa[k]
    return w


@lru_cache(maxsize=None)
def c2_case(mode, n_s):
    """roots of T' on scan points -> dict(x0, dx, zs, xe, ze, ang, zb, xf, zf, row, j, off, w, accepted, m): per kept construction its
    row (element or angle), focal point, scan index, offset of the root from the scan point and the dense oracle's winner; per scan
    index how many of its (row, ray length) candidates the oracle accepted (its winner within 1e-9 m of the scan point, basin >=
    dx, runner-up more than 1e-12 s behind).  At most three candidates per scan index are kept (the first, the middle and the last
    row accepted), each with its two neighbours 1e-8 m left and right of the scan point, built the same way and accepted alike."""
    x0, dx, zs = c2_profile(n_s)
    xe, ze = c2_elements(n_s)
    c = dict(x0=x0, dx=dx, zs=zs, coef=S.spline(x0, dx, zs), xe=xe, ze=ze, ang=C2_ANGLES, zb=Z0 + ZB_OFF)
    Pj = scan_points(x0, dx, n_s)
    js = c2_scan_indices(n_s, 12 if mode == "elem" else 3)
    R, J, Lg = (v.ravel() for v in np.meshgrid(np.arange(C2_ROWS), js, np.array(C2_L if mode == "elem" else C2_L[:2]), indexing="ij"))
    xend = x0 + (n_s - 1) * dx

    def build(R, J, Lg, off):
        xs = Pj[J] + off
        xf, zf, ok = _refract(mode, c["coef"], x0, dx, xs, c["ang"][R] if mode == "pw" else (xe[R], ze[R]), Lg)
        ok &= (xf > x0) & (xf < xend)
        xfc, zfc = np.where(ok, xf, 0.5 * (x0 + xend)), np.where(ok, zf, Z0 + 0.005)
        ok &= zfc > S.spline_eval(c["coef"], x0, dx, xfc)[0] + 1e-4
        if mode == "skip":
            ok &= zfc < c["zb"] - 1e-4
        w = _c2_winners(mode, c, R, xfc, zfc)
        with np.errstate(invalid="ignore"):
            ok &= (np.abs(w["x"] - xs) < 1e-9) & (w["basin"] >= dx) & (w["gap"] > 1e-12)
        return xf, zf, w, ok

    _, _, _, ok0 = build(R, J, Lg, 0.0)
    pick = []
    for j in js:
        k = np.nonzero(ok0 & (J == j))[0]
        pick += sorted(set(k[[0, k.size // 2, -1]].tolist())) if k.size else []
    pick = np.array(pick, dtype=np.int64)
    parts = [build(R[pick], J[pick], Lg[pick], off) for off in C2_OFFS]
    good = parts[0][3] & parts[1][3] & parts[2][3]
    cat = lambda k: np.concatenate([p[k][good] for p in parts])                  # noqa: E731
    w = {k: np.concatenate([p[2][k][good] for p in parts]) for k in ("t", "x", "basin", "gap")}
    c.update(xf=cat(0), zf=cat(1), row=np.tile(R[pick][good], 3), j=np.tile(J[pick][good], 3), w=w, m=Pj.size,
             off=np.repeat(np.array(C2_OFFS), int(good.sum())), accepted={int(j): int((ok0 & (J == j)).sum()) for j in js},
             kept={int(j): int((J[pick][good] == j).sum()) for j in js})
    return c


# ------------------------------------------------------------------------------------------------------------ C3: the validity edges
E_X0, E_DX, E_NS = -2.0 ** -6, 2.0 ** -10, 33                 # the knots x0 + k dx and xend = +2^-6 are exact in fp64
E_XEND = 2.0 ** -6


def edge_profile():
    """a flat profile 20 mm deep with one sharp bump towards the array centred BETWEEN the knots 20 and 21 and one sharp pit away
    from it between the knots 8 and 9: the spline's least and greatest depth lie between samples"""
    x = E_X0 + E_DX * np.arange(E_NS)
    g = lambda k: np.exp(-(((x - (E_X0 + (k + 0.5) * E_DX)) / (0.8 * E_DX)) ** 2))          # noqa: E731
    return Z0 - 1.0e-3 * g(20) + 0.6e-3 * g(8)


def edge_extremes():
    """-> (zs, smin, smax): the spline's true least and greatest depth (surface_numpy.spline_min, skip_numpy.spline_max)"""
    zs = edge_profile()
    coef = S.spline(E_X0, E_DX, zs)
    return zs, S.spline_min(coef, E_DX), K.spline_max(coef, E_DX)


def ulps(v, k):
    """v moved by k units in the last place (k < 0: down)"""
    for _ in range(abs(k)):
        v = np.nextafter(v, np.inf if k > 0 else -np.inf)
    return float(v)


def ramp_profile():
    """a linear ramp of dyadic depths, 2^-6 + k 2^-14: the natural spline is the ramp itself (second derivatives 0, slope 2^-4), and
    its least and greatest depth are the end samples EXACTLY, in the oracle's arithmetic and in the kernel's"""
    return 2.0 ** -6 + 2.0 ** -14 * np.arange(E_NS)

"""Inputs that hold the element matchers at the edge of their tolerance, and np.isclose's decisions on them (NumPy only).

The reference's matcher (main_rt.py:487-501, main_compare.py:518-521) takes, per receive element, the FIRST ray whose landing point
passes ``np.isclose(land_x, x_rx, rtol, atol)``.  The one reference here is that call itself, on the whole rays x elements grid:

    first_ray  first true index per column, -1 when there is none       hit       its mask
    tof_hit    tof[first_ray], 0.0 when there is none                   ray_hits  any over the elements

What the cases are made of:

* apertures of 1, 63, 64, 65 and 129 elements in four orders (ascending, reversed, a fixed permutation, ascending inside every
  64-element chunk but not across the seam); the 65-element one carries a centre element with bits below ulp(atol)
  (257.7 * spacing(1e-4)), and comes with an equal pair of neighbours, with -0.0 next to +0.0 and with +-inf at its ends;
* landing points within 4 ulp of every element's ``x_e +- tol_e``, ``tol_e = fl(atol + fl(rtol * |x_e|))``: 18 per element;
* a fixed permutation of them with NaN at every seventh index and +-inf at two, so that an element's earliest hitting rays lie in
  different waves, workgroups and chunks;
* 820 cyclic rotations of the 65-element aperture's landing points: 4100 workgroups of 256 rays, the size at which the stand-alone
  kernel gives every workgroup two chunks;
* for the fused kernel, whose landing points the trace chooses: elements solved FROM a row of landing points, each moved by
  -4..4 ulp off the edge of its own tolerance.
"""
import numpy as np

PITCH = 0.6e-3
#: (atol, rtol).  rtol = 0: the window of an ascending aperture is every element's own tolerance; rtol >= 1: x - tol(x) no longer ascends
PAIRS = ((1e-6, 1e-5), (1e-4, 1e-5), (2e-3, 0.0), (2e-3, 1e-5), (1e-6, 0.0), (0.0, 0.0), (0.0, 1e-5), (1e-4, 1.0), (1e-4, 3.0))
#: the families on which a window of fl(x +- win) drops hits (test_match_edge_cases_cpu.py)
SHARP = ((2e-3, 0.0), (1e-6, 0.0), (1e-4, 3.0))
SIZES = (1, 63, 64, 65, 129)
ORDERS = ("ascending", "reversed", "permuted", "seam")
RESIDUE = 257.7 * np.spacing(1e-4)          # the centre element: bits far below ulp(atol)
ROWS, STEP = 820, 37                        # the chunked case: row k is the probe vector rotated by k * 37 mod n


# ---------------------------------------------------------------------------------------------------------------- reference
def isclose_matrix(land, x_rx, atol, rtol):
    with np.errstate(invalid="ignore", over="ignore"):
        return np.isclose(np.asarray(land)[:, None], np.asarray(x_rx)[None, :], rtol=rtol, atol=atol)


def decisions(land, tof, x_rx, atol, rtol, H=None):
    """-> dict(hit bool[E], first_ray i32[E], tof_hit f64[E], ray_hits bool[N]) of one row of landing points"""
    H = isclose_matrix(land, x_rx, atol, rtol) if H is None else H
    hit = H.any(axis=0)
    first = np.where(hit, H.argmax(axis=0), -1).astype(np.int32)
    tof_hit = np.where(hit, np.asarray(tof, dtype=np.float64)[np.maximum(first, 0)], 0.0)
    return dict(hit=hit, first_ray=first, tof_hit=tof_hit, ray_hits=H.any(axis=1))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---------------------------------------------------------------------------------------------------------------- apertures
def base_aperture(n_rx, variant="plain"):
    """ascending.  65 elements: the reference's pitch, centred, the centre element RESIDUE; the other sizes sit off the pitch's
    grid by 0.17 mm so that no element is a short binary fraction of another"""
    x = (np.arange(n_rx, dtype=np.float64) - n_rx // 2) * PITCH
    if n_rx == 65:
        x[32] = RESIDUE
    else:
        x = x + 1.7e-4
    if variant == "equal_pair":
        x[11] = x[10]
    elif variant == "signed_zeros":
        x[32], x[33] = -0.0, 0.0
    elif variant == "inf_ends":
        x[0], x[-1] = -np.inf, np.inf
    elif variant != "plain":
        raise ValueError(variant)
    assert n_rx == 1 or np.all(x[:-1] <= x[1:])
    return x


def order_index(n_rx, order):
    """positions -> indices into the ascending aperture.  "seam": rotated by n_rx - 64, so that positions 0..63 and 64.. ascend
    each and the one descent lies between positions 63 and 64 (None when the aperture has one chunk only)"""
    i = np.arange(n_rx)
    if order == "ascending":
        return i
    if order == "reversed":
        return i[::-1].copy()
    if order == "permuted":
        return np.random.default_rng(1000 + n_rx).permutation(n_rx)
    if order == "seam":
        return None if n_rx <= 64 else np.roll(i, -(n_rx - 64))
    raise ValueError(order)


def apertures():
    """every (name, ascending aperture): the five sizes and the three variants of the 65-element one"""
    out = [(f"n{n}", base_aperture(n)) for n in SIZES]
    out += [(f"n65_{v}", base_aperture(65, v)) for v in ("equal_pair", "signed_zeros", "inf_ends")]
    return out


# ---------------------------------------------------------------------------------------------------------------- edge probes
def tolerance(x_rx, atol, rtol):
    with np.errstate(invalid="ignore"):
        return np.float64(atol) + np.float64(rtol) * np.abs(x_rx)        # two roundings, as np.isclose


def edge_probes(x_rx, atol, rtol):
    """-> (probes, owner): per finite element and side the double x_e +- tol_e and its four neighbours either way, 18 per element"""
    x_rx = np.asarray(x_rx, dtype=np.float64)
    own = np.flatnonzero(np.isfinite(x_rx))
    xe, tol = x_rx[own], tolerance(x_rx[own], atol, rtol)
    cols = []
    for side in (-1.0, 1.0):
        c = xe + side * tol
        lo, hi = [c], [c]
        for _ in range(4):
            lo.append(np.nextafter(lo[-1], -np.inf)); hi.append(np.nextafter(hi[-1], np.inf))
        cols += lo[:0:-1] + hi
    return np.stack(cols, axis=1).reshape(-1), np.repeat(own, 18)


def layout(probes, owner):
    """the probe vector as a row of rays: a fixed permutation, then NaN at every seventh index and +inf / -inf at two
    -> (land, owner of each ray or -1, tof)"""
    n = probes.size
    perm = np.random.default_rng(2024).permutation(n)
    land, own = probes[perm].copy(), owner[perm].copy()
    land[::7] = np.nan; own[::7] = -1
    for i, v in ((min(5, n - 1), np.inf), (n // 2 + 1 if (n // 2 + 1) % 7 else n // 2 + 2, -np.inf)):
        if 0 < i < n:
            land[i] = v; own[i] = -1
    tof = 2.5e-5 + np.arange(n) * 1.0000001e-9                           # distinct, so tof_hit tells which ray was taken
    return land, own, tof


def case(x_rx, atol, rtol):
    """one row of rays at the edges of ``x_rx`` (any order) and np.isclose's decisions on it"""
    probes, owner = edge_probes(x_rx, atol, rtol)
    land, own, tof = layout(probes, owner)
    H = isclose_matrix(land, x_rx, atol, rtol)
    d = decisions(land, tof, x_rx, atol, rtol, H)
    d.update(land=land, tof=tof, owner=own, H=H, x_rx=np.asarray(x_rx, dtype=np.float64), atol=atol, rtol=rtol)
    return d


def two_earliest(H):
    """per element the indices of its two earliest hitting rays, [2, E]; -1 where there are fewer"""
    n = H.shape[0]
    idx = np.where(H, np.arange(n)[:, None], n)
    two = np.sort(idx, axis=0)[:2]
    return np.where(two < n, two, -1)


def layout_counts(H, chunks=2):
    """how many elements have their two earliest hitting rays in different 64-ray waves / different 256-ray workgroups / the two
    256-ray chunks of one workgroup of ``chunks`` chunks"""
    a, b = two_earliest(H)
    ok = b >= 0
    waves = ok & (a >> 6 != b >> 6)
    groups = ok & (a >> 8 != b >> 8)
    inside = groups & ((a >> 8) // chunks == (b >> 8) // chunks)
    return int(waves.sum()), int(groups.sum()), int(inside.sum())


# ---------------------------------------------------------------------------------------------------------------- window model
def window_model(land, x_sorted, atol, rtol, widen=False):
    """The stand-alone kernel's search on an ascending aperture, as the parent commit has it: ``win = atol + rtol * max|x_rx|``, the
    scan starts at the first element not below fl(x - win) and stops at the first above fl(x + win); inside, np.isclose decides.
    ``widen``: win plus 8 eps (max|x_rx| + win), the fused kernel's margin.  -> H as the kernel sees it"""
    x_sorted = np.asarray(x_sorted, dtype=np.float64)
    amax = np.max(np.abs(x_sorted))
    win = np.float64(atol) + np.float64(rtol) * amax
    if widen:
        win = win + (8.0 * np.finfo(np.float64).eps) * (amax + win)
    H = isclose_matrix(land, x_sorted, atol, rtol)
    with np.errstate(invalid="ignore"):
        lo, hi = (land - win)[:, None], (land + win)[:, None]
        seen = ~(x_sorted[None, :] < lo) & ~(x_sorted[None, :] > hi)
    # (the scan stops at the FIRST element above the window: on an ascending aperture all that follow are above it too)
    return H & seen


# ---------------------------------------------------------------------------------------------------------------- chunked rows
def chunked_rows(atol, rtol):
    """820 rotations of the 65-element aperture's row of rays: 820 x 5 = 4100 workgroups of 256 rays.  The hit matrix is computed
    once; row k is the row rotated by s = k * 37 mod n (land_k[j] = land[(j + s) mod n]), so its first hitting ray of an element
    is the element's first hit index >= s, minus s, or else its first hit index at all, plus n - s."""
    c = case(base_aperture(65), atol, rtol)
    land, tof, H = c["land"], c["tof"], c["H"]
    n, E = H.shape
    shift = (np.arange(ROWS) * STEP) % n
    idx = (np.arange(n)[None, :] + shift[:, None]) % n
    first = np.full((ROWS, E), -1, dtype=np.int32)
    for e in range(E):
        h = np.flatnonzero(H[:, e])
        if h.size:
            k = np.searchsorted(h, shift)                                 # first hit index >= shift
            first[:, e] = np.where(k < h.size, h[np.minimum(k, h.size - 1)] - shift, h[0] + n - shift)
    hit = first >= 0
    src = (np.maximum(first, 0) + shift[:, None]) % n
    c.update(land_rows=land[idx], tof_rows=tof[idx], shift=shift, first_rows=first, hit_rows=hit,
             tof_hit_rows=np.where(hit, tof[src], 0.0), ray_hits_rows=c["ray_hits"][idx])
    return c


# ---------------------------------------------------------------------------------------------------------------- fused cases
def grid_unit(land, xe, tol):
    """The spacing of the doubles a case lives on.  |land - x_e| is formed from land and x_e: it is a multiple of the finer of
    their two spacings, so it comes no closer to tol_e than the coarsest of spacing(land), spacing(x_e), spacing(tol_e) allows.
    Where tol_e is the coarsest — small elements, rtol >= 1 — this is ulp(tol_e) itself."""
    return np.maximum(np.spacing(np.abs(tol)), np.maximum(np.spacing(np.abs(land)), np.spacing(np.abs(xe))))


def fused_elements(land_row, n_rx, atol, rtol):
    """Elements at the edge of the landing points of one traced row.

    ``n_rx`` rays with finite, distinct landing points, one of every wave that has any and the rest spread evenly over the row;
    per ray the x_e with |land - x_e| = tol(x_e), on alternating sides: x_e = (land -+ atol) / (1 +- rtol * sign(x_e)) — closed,
    and exact for rtol = 0 — then two fixed-point steps x_e = land -+ (atol + rtol |x_e|), which contract for rtol < 1.  For
    rtol >= 1 they do not, and the closed form stands; there an edge exists only on the side of the origin and only for
    |land| > atol (elsewhere |land - x_e| < atol + |x_e| whatever x_e), so rays with |land| > 2 atol are taken and the element
    lies between the origin and its ray.  Each x_e is then moved by k in -4..4 of its own ulp, k cycling over the elements; sorted.
    -> (x_rx ascending, picked ray per element, distance |fl(|land - x_e|) - tol_e| in grid units per element)"""
    land_row = np.asarray(land_row, dtype=np.float64)
    ok = np.flatnonzero(np.isfinite(land_row))
    _, uniq = np.unique(land_row[ok], return_index=True)
    ok = np.sort(ok[uniq])
    if rtol >= 1.0:
        ok = ok[np.abs(land_row[ok]) > 2.0 * atol]
    _, per_wave = np.unique(ok >> 6, return_index=True)                   # one ray of every wave that has any, then evenly the rest
    rest = np.setdiff1d(ok, ok[per_wave])
    if ok.size < n_rx or per_wave.size > n_rx:
        raise ValueError("too few distinct finite landing points, or more waves than elements")
    fill = rest[np.round(np.linspace(0, rest.size - 1, n_rx - per_wave.size)).astype(int)] if n_rx > per_wave.size else rest[:0]
    rays = np.sort(np.concatenate([ok[per_wave], fill]))
    assert np.unique(rays).size == n_rx
    x = land_row[rays]
    side = np.where(np.arange(n_rx) % 2 == 0, 1.0, -1.0)                 # +1: the element lies below its ray
    if rtol >= 1.0:
        side = np.sign(x)                                                # |x - x_e| < |x_e| <= tol(x_e) on the far side: no edge there
    xe = x - side * atol
    if rtol > 0.0:
        den = 1.0 + side * rtol * np.sign(xe)
        good = den > 0.25
        xe = np.where(good, xe / np.where(good, den, 1.0), xe)
        if rtol < 1.0:
            for _ in range(2):
                xe = x - side * (atol + rtol * np.abs(xe))
    k = (np.arange(n_rx) % 9) - 4
    for step in range(1, 5):
        xe = np.where(k >= step, np.nextafter(xe, np.inf), np.where(k <= -step, np.nextafter(xe, -np.inf), xe))
    tol = tolerance(xe, atol, rtol)
    dist = np.abs(np.abs(x - xe) - tol) / grid_unit(x, xe, tol)
    o = np.argsort(xe, kind="stable")
    return xe[o], rays[o], dist[o]


def residue_case(land_row):
    """The sub-ulp(atol) element reached through a chosen atol: for the smallest landing point x above 1e-6 m,
    atol = x - 258 spacing(x), rtol = 0 and the centre element of the 65-element aperture at 257.7 spacing(atol).  Then
    fl(x - x_e) == atol — a hit — while fl(x - atol) = 258 spacing(atol) > x_e.  -> (x_rx ascending, atol, ray)"""
    land_row = np.asarray(land_row, dtype=np.float64)
    cand = np.flatnonzero(np.isfinite(land_row) & (land_row > 1e-6))
    ray = cand[np.argmin(land_row[cand])]
    x = land_row[ray]
    atol = float(x - 258 * np.spacing(x))
    x_rx = (np.arange(65, dtype=np.float64) - 32) * PITCH
    x_rx[32] = 257.7 * np.spacing(atol)
    return x_rx, atol, int(ray)

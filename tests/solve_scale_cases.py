"""The cases of the large-call solve tests (tests/test_solve_scale_cases_cpu.py, tests/test_gpu_solve_scale.py) and the REFERENCE'S OWN
census of them: the shapes on either side of the launcher's thresholds (32,768 and 131,072 element tasks, 512 elements), what
oracle.cport says about every (row, element) of them, and where the reference itself is ambiguous.

Plain data and helpers: no GPU, no random numbers, nothing of the library under test.  A case is (G pipe geometries) x (the first T
transmit points) x (an aperture) over n grid rays; row = g * T + t.  Rows are solved by cport.solve / cport.shoot once per process
and geometry / transmit point / aperture / grid (cached; A- and A+ share their rows, and so on) and must not be written to.

An element is NOT ``clean`` only where the reference is ambiguous:
  - its grid trace brackets it more than RTUS_MAX_ROOTS = 4 times (the kernel keeps the first four BRACKETS, the oracle the first
    four ROOTS), under the kernel's rule (f_prev < 0 && f_cur >= 0) || (f_prev > 0 && f_cur <= 0) with both rays finite;
  - the oracle's bracket count differs from its root count: a jump of x_land, or a branch that ends inside a bracket;
  - a grid ray lands within 1e-9 m of the element: the two traces differ in the last bits of a landing point, so which of the two
    neighbouring pairs owns such a root is not defined;
  - the oracle's own x_land SCATTERS by more than 5e-12 m over five launch angles 1e-13 rad apart around one of its roots.  The
    tolerance for a root's angle, 5e-12 m / slope, is the landing noise of a trace; the chain works with the water legs as lines
    z = m x + b (the reference's np.polyfit), and where a leg is within ~1e-5 of vertical m is ~1e5 and the landing point of the
    reference's own arithmetic is noise of 1e-10 .. 1e-9 m from one angle to the next (x_land itself moves by < 4e-14 m over those
    five angles).  A bisection of such a function ends at ONE of many sign changes: the root is defined to noise / slope ~ 1e-8 rad
    and its time to ~1e-12 s, whoever solves it.  At most three elements of a case.
On clean elements a root count is a fact, and the k-th root lies in the k-th bracket."""
from collections import namedtuple
from concurrent.futures import ThreadPoolExecutor
from functools import lru_cache
import os

import numpy as np

from conftest import D_PLANE
from oracle import cport

MAX_ROOTS = 4
NEAR = 1e-9                                                   # m: a grid ray this close to an element makes its brackets ambiguous
NOISE_CAP = 5e-12                                             # m: the landing noise the angle tolerance allows for (scripts/fuzz_solve.py)
NOISE_STEP = 1e-13                                            # rad: x_land moves by < 1e-13 m per step (|slope| < 1 m/rad)
NOT_CLEAN_CAP = 0.01                                          # a condition on the inputs (scripts/fuzz_solve.py's figure), no tolerance
ALPHA_MAX = float(np.float64(50.62033040986099 * (np.pi / 180)))      # main_rt.py:479 (the CPU test holds it to rtus.ALPHA_MAX)

# about half the elements get two roots, some one or three; a near-tangent pipe (offset = 0.999 r) and a centred one
PIPES = np.array([(0.037, 0.0038), (0.04, -0.006), (0.06, 0.009), (0.02, 0.999 * 0.02), (0.037, 0.0), (0.012, -0.004), (0.08, 0.001),
                  (0.1, -0.01)])
TX_ALL = (np.arange(253) - 126) * 0.15e-3


def _reference_elements():                                    # main_rt.py:469-474: 64 elements, pitch 0.6 mm, + the virtual centre element
    x = np.arange(64, dtype=np.float64) * np.float64(0.0006)
    return np.insert(x - np.mean(x), 32, np.float64(0.0))


def _ragged(x, seed):
    """an unsorted order, a duplicate and one NaN element (as tests/test_gpu_solve_modes.py's ragged sizes)"""
    x = x[np.random.default_rng(seed).permutation(x.size)].copy()
    x[3] = x[1]
    x[2] = np.nan
    return x


APERTURES = {"ref65": _reference_elements(), "lin513": np.linspace(-0.03, 0.03, 513)}
APERTURES["ref65_ragged"] = _ragged(APERTURES["ref65"], 65)
APERTURES["lin513_ragged"] = _ragged(APERTURES["lin513"], 513)
for _x in APERTURES.values():
    _x.setflags(write=False)

# lanes: element lanes per workgroup of the one-lane kernel (0: three lanes per bracket, no list census); rows: "all" or "sample"
Case = namedtuple("Case", "name T aperture n path lanes rows")
CASES = {c.name: c for c in (
    Case("A-", 63, "ref65", 257, "ROW", 0, "all"),            # 32,760 tasks
    Case("A+", 64, "ref65", 257, "HALF", 128, "all"),         # 33,280 = 260 x 128: every workgroup full
    Case("A+T65", 65, "ref65", 257, "HALF", 128, "all"),      # 33,800: eight element lanes in the last workgroup
    Case("A+n256", 64, "ref65", 256, "HALF", 128, "all"),     # four full 64-ray blocks: no straddling pair after the last
    Case("A+n258", 64, "ref65", 258, "HALF", 128, "all"),     # the last block holds two rays
    Case("A+ragged", 64, "ref65_ragged", 257, "HALF", 128, "all"),
    Case("B-", 252, "ref65", 257, "HALF", 128, "sample"),     # 131,040
    Case("B+", 253, "ref65", 257, "FULL", 256, "sample"),     # 131,560
    Case("C-", 7, "lin513", 257, "TRIO_SCAN", 0, "all"),      # 28,728
    Case("C+", 8, "lin513", 257, "SCAN", 256, "all"),         # 32,832: 9 chunks a row, the last with one live lane
    Case("C+ragged", 8, "lin513_ragged", 257, "SCAN", 256, "all"),
)}
G = PIPES.shape[0]


def alpha_grid(n):
    return np.linspace(-ALPHA_MAX, ALPHA_MAX, n)


def x_rx(c):
    return APERTURES[c.aperture]


def n_rows(c):
    return G * c.T


def n_tasks(c):
    return n_rows(c) * x_rx(c).size


def sample_rows(c):
    """The rows compared with the oracle: all of them, or (B) the first four, the last four, every eighth and every row that shares
    the ragged last workgroup — ascending."""
    R, E = n_rows(c), x_rx(c).size
    if c.rows == "all":
        return np.arange(R)
    last = ((R * E - 1) // c.lanes) * c.lanes // E            # the first row of the last workgroup's element lanes
    return np.unique(np.concatenate([np.arange(4), np.arange(R - 4, R), np.arange(0, R, 8), np.arange(last, R)]))


# ---- the oracle, row by row ----------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def _row(g, t, aperture, n):
    """cport.solve and cport.shoot of one (geometry, transmit point): (tt_min [E], tt_all [E, 4], alpha_all [E, 4], land [n], scatter
    [E, 4]: max - min of the oracle's x_land over the five angles root + (-2 .. 2) NOISE_STEP)"""
    alpha, x = alpha_grid(n), APERTURES[aperture]
    tmin, ta, aa = cport.solve(TX_ALL[t], D_PLANE, D_PLANE, alpha, x, PIPES[g, 0], PIPES[g, 1])
    land = cport.shoot(TX_ALL[t], D_PLANE, np.full(n, D_PLANE), alpha, PIPES[g, 0], PIPES[g, 1])[0][6].copy()
    fin = np.isfinite(aa)
    xl = cport.land_alphas(TX_ALL[t], D_PLANE, D_PLANE, aa[fin][:, None] + NOISE_STEP * np.arange(-2, 3), alpha, PIPES[g, 0], PIPES[g, 1])
    scatter = np.full(aa.shape, np.nan)
    scatter[fin] = xl.max(1) - xl.min(1)                       # (a NaN among the five: NaN, which counts as noisy)
    for a in (tmin, ta, aa, land, scatter):
        a.setflags(write=False)
    return tmin, ta, aa, land, scatter


@lru_cache(maxsize=None)
def land_all(n):
    """landing x of every grid ray of every (geometry, transmit point): [G, 253, n] (cport.shoot_batch)"""
    a = cport.shoot_batch(TX_ALL, np.full(TX_ALL.size, D_PLANE), np.full(n, D_PLANE), alpha_grid(n), PIPES)[:, :, 6, :].copy()
    a.setflags(write=False)
    return a


def brackets(land, x):
    """land [R, n], x [E] -> (count [R, E] of the kernel's brackets, first four lower-ray indices [R, E, 4] (-1 padded), near [R, E]:
    some finite grid ray within NEAR of the element)"""
    R, n = land.shape
    cnt = np.empty((R, x.size), dtype=np.int64)
    idx = np.empty((R, x.size, MAX_ROOTS), dtype=np.int64)
    near = np.empty((R, x.size), dtype=bool)
    with np.errstate(invalid="ignore"):
        for r0 in range(0, R, 64):
            f = land[r0:r0 + 64, None, :] - x[None, :, None]
            fp, fc = f[..., :-1], f[..., 1:]
            st = np.isfinite(fp) & np.isfinite(fc) & (((fp < 0) & (fc >= 0)) | ((fp > 0) & (fc <= 0)))
            cnt[r0:r0 + 64] = st.sum(-1)
            first = np.sort(np.where(st, np.arange(n - 1), n), axis=-1)[..., :MAX_ROOTS]
            idx[r0:r0 + 64] = np.where(first == n, -1, first)
            near[r0:r0 + 64] = (np.abs(f) <= NEAR).any(-1)
    return cnt, idx, near


Census = namedtuple("Census", "rows tmin ta aa nroots land cnt bidx near noisy clean")


def oracle_rows(name, rows):
    """The oracle on the given rows of the case: everything [len(rows), ...] in the order of ``rows``."""
    c = CASES[name]
    rows = np.asarray(rows, dtype=np.int64)
    with ThreadPoolExecutor(max(1, min(8, os.cpu_count() or 1))) as ex:          # (the C functions run without the GIL)
        got = list(ex.map(lambda r: _row(int(r) // c.T, int(r) % c.T, c.aperture, c.n), rows))
    tmin, ta, aa, land, scatter = (np.stack([g[k] for g in got]) for k in range(5))
    nroots = np.isfinite(ta).sum(-1)
    cnt, bidx, near = brackets(land, x_rx(c))
    noisy = (np.isfinite(aa) & ~(scatter <= NOISE_CAP)).any(-1)
    clean = (cnt <= MAX_ROOTS) & (cnt == nroots) & ~near & ~noisy
    out = Census(rows, tmin, ta, aa, nroots, land, cnt, bidx, near, noisy, clean)
    for a in out:
        a.setflags(write=False)
    return out


@lru_cache(maxsize=None)
def census(name):
    """The oracle on the case's sample_rows."""
    return oracle_rows(name, sample_rows(CASES[name]))


GridCensus = namedtuple("GridCensus", "cnt bidx near")


@lru_cache(maxsize=None)
def grid_census(name):
    """What the grid trace alone says about EVERY row of the case (no root-finding): bracket counts, indices and the near mask."""
    c = CASES[name]
    land = land_all(c.n)[:, :c.T, :].reshape(G * c.T, c.n)
    out = GridCensus(*brackets(land, x_rx(c)))
    for a in out:
        a.setflags(write=False)
    return out


def workgroup_lists(name):
    """The one-lane kernel's bracket list per workgroup, from the oracle's bracket counts capped at four: (length [n_workgroups],
    workgroup of every (row, element) [R, E]).  Mask mode: ``lanes`` consecutive flat (row, element) lanes; scan mode (more than 512
    elements): four consecutive (row, 64-element chunk) wave-tasks."""
    c = CASES[name]
    assert c.lanes, "three lanes per bracket: no list"
    cnt = np.minimum(grid_census(name).cnt, MAX_ROOTS)
    R, E = cnt.shape
    if E <= 512:
        wg = (np.arange(R * E) // c.lanes).reshape(R, E)
    else:
        chunks = (E + 63) // 64
        wg = ((np.arange(R)[:, None] * chunks + np.arange(E)[None, :] // 64) // 4)
    return np.bincount(wg.ravel(), weights=cnt.ravel()).astype(np.int64), wg


def slopes(c, land, aa):
    """|dx_land / dalpha| between the oracle's grid rays about each root: land [R, n], aa [R, E, 4] -> [R, E, 4] (NaN roots: NaN)"""
    alpha = alpha_grid(c.n)
    j = np.clip(np.searchsorted(alpha, np.nan_to_num(aa, nan=0.0)) - 1, 0, c.n - 2)
    r = np.arange(land.shape[0])[:, None, None]
    s = np.abs(land[r, j + 1] - land[r, j]) / (alpha[1] - alpha[0])
    return np.where(np.isfinite(aa), s, np.nan)

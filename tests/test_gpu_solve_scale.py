"""GPU: the solve's LARGE-call paths (one lane per bracket: HALF, FULL, SCAN) against the oracle's bisection, at the smallest shapes
on either side of the launcher's thresholds (tests/solve_scale_cases.py; its premises: tests/test_solve_scale_cases_cpu.py).

Every other comparison of rtus_solve with oracle.cport stays at or below 32,768 element tasks and so runs the three-lane paths;
bench.py's solve_scale times FULL and only counts finite results.  The one-lane kernel holds decision points of its own: a
workgroup's bracket list longer than 256 takes a second trip; EPB sits on both sides of the owner -> (row, element) map; the straggler
rescue borrows finished lanes; the scan mode skips 64-ray blocks through land_box and the previous block's last ray; element lanes
span rows; chunks and workgroups are ragged.

The rule for root COUNTS is equality on every clean element (no share): an element is left out only where the reference itself is
ambiguous, and that is at most 1 % of a case by the CPU test (measured <= 0.024 %).  Tolerances are scripts/fuzz_solve.py's:
|dt| <= 1e-13 s with the same NaN slots; |dalpha| <= 1e-11 rad (three lanes) or 5e-11 rad (one lane) + 5e-12 m / max(slope, 1e-3),
roots on stretches of x_land flatter than 1e-3 m/rad in time only; fast=True: 1e-11 s, 1e-9 rad, counts may differ on 2 % + 2 / n_rx
of a row's clean elements.

Measured on the MI355X (clean roots of the rows compared; DESIGN.md's solve section has the table): worst |dt| 8.7e-15 s, worst
|dalpha| / allowed 0.51 on every one-lane path (1.3e-10 rad on a slope of 0.025 m/rad: the noise term), 0.50 on ROW, 0.23 on TRIO_SCAN,
0.10 in the vector form; root counts equal on every clean element of every case.  The tolerances hold as they are.

What the cases found in the REFERENCE, not in the kernels: where a water leg is within ~1e-5 of vertical the chain's own landing point
is noise of 1e-10 .. 1e-9 m from one launch angle to the next, a root is then defined to ~1e-8 rad / ~1e-12 s whoever solves it, and
ROW, HALF and the oracle give three different answers (up to 87 x the allowance before the rule).  tests/solve_scale_cases.py
measures that scatter on the oracle alone and counts such an element as not clean (2 - 8 elements of a case).

What this file catches: each change below was made once in a scratch build of rtus_solve.hip and the cases were run through it.
  M1  the list loop's bound total -> min(total, RTUS_SOLVE_TPB): test_case_against_the_oracle[B+, C+, C+ragged] (2,031 - 4,422 clean
      elements without their roots), test_fast_against_the_oracle[B+, C+], test_either_side_of_a_threshold[B-|B+, C-|C+],
      test_every_row_of_b_plus_against_small_calls.  The 128-lane cases pass: their lists peak at exactly 256.
  M2  edge forced false in the mask path: test_case_against_the_oracle[every A+ case, B-, B+] (226 - 662 clean elements one root
      short), test_fast_against_the_oracle[A+, B+], test_either_side_of_a_threshold[A-|A+], the small calls.
  M3  lprev left out of the scan path's block interval: test_case_against_the_oracle[C-, C+] (36 / 46 clean elements one root short;
      an unsorted wave spans the whole aperture and skips no block, so C+ragged passes).
  M4  the rescue's continuity test removed: NOTHING fails, and every output of every case keeps its bits.  The test acts only where a
      rescue triple straddles a jump of x_land; this family has no jump inside a bracket that needs a third evaluation, and a bracket
      over a jump has no root by the oracle, so its element is not clean by construction.  Catching it needs a rule for jump
      brackets and a geometry with jumps (scripts/fuzz_solve.py draws them for the three-lane twin of the test)."""
from importlib import import_module

import numpy as np
import pytest

import solve_scale_cases as S
from conftest import D_PLANE

pytestmark = pytest.mark.gpu

TOL_T, TOL_A3, TOL_A1 = 1e-13, 1e-11, 5e-11                   # s, rad (three lanes per bracket), rad (one lane per bracket)
FAST_T, FAST_A, FAST_CNT = 1e-11, 1e-9, 0.02                  # the vector-form trace: another arithmetic than the oracle's
NOISE, FLAT = 5e-12, 1e-3                                     # m: the traces' own landing noise; m/rad: below it alpha is not compared
ONE_LANE = ("HALF", "FULL", "SCAN")
NAMES = ("tt", "alpha_root", "tt_all", "alpha_all", "n_roots")

_GPU = {}


def _call(rtus, c, tx=None, fast=False):
    tx = S.TX_ALL[:c.T] if tx is None else tx
    x = S.x_rx(c)
    out = rtus.solve_travel_times(tx, np.full(tx.size, D_PLANE), x, S.alpha_grid(c.n), S.PIPES, params=rtus.Params(), all_roots=True, fast=fast)
    return out                                                # tt, alpha_root [G, T, E], tt_all, alpha_all [G, T, E, 4], n_roots [G, T, E]


def gpu(rtus, name, fast=False):
    """the case through the host API, once per process: (tt, alpha_root, tt_all, alpha_all, n_roots) with rows flat, read-only"""
    if (name, fast) not in _GPU:
        c = S.CASES[name]
        E = S.x_rx(c).size
        assert rtus.solve_path(S.G, c.T, c.n, E) == c.path
        out = tuple(a.reshape((S.G * c.T, E) + a.shape[3:]) for a in _call(rtus, c, fast=fast))
        for a in out:
            a.setflags(write=False)
        _GPU[(name, fast)] = out
    return _GPU[(name, fast)]


def well_formed(c, out):
    """what holds for EVERY element, clean or not: n_roots <= 4 and = the finite slots, NaN padding behind the roots, roots ascending
    in alpha, (tt, alpha_root) = the least-time root bit for bit, nothing for a NaN element.  Ascending: to what an angle can be known
    to at all, FAST_A + NOISE / FLAT = 6e-9 rad — where a grid ray lands ON the element (the centre element under a centred pipe,
    transmit point 0: x_land(0) = -6e-18 m) both neighbouring brackets hold that root and report it, 3e-13 rad apart in either order;
    on clean elements against_oracle asks for strictly ascending."""
    tt, ar, ta, aa, nr = out
    fin = np.isfinite(ta)
    assert nr.max() <= S.MAX_ROOTS and np.array_equal(fin.sum(-1), nr) and np.array_equal(fin, np.isfinite(aa))
    assert np.array_equal(fin, np.arange(S.MAX_ROOTS) < nr[..., None])
    with np.errstate(invalid="ignore"):
        assert not (np.diff(aa, axis=-1) < -(FAST_A + NOISE / FLAT)).any()
    has = nr > 0
    assert np.array_equal(np.isfinite(tt), has) and np.array_equal(np.isfinite(ar), has)
    k = np.argmin(np.where(fin, ta, np.inf), axis=-1)
    assert np.array_equal(tt[has], np.take_along_axis(ta, k[..., None], -1)[..., 0][has])
    at = (ta == tt[..., None]) & (aa == ar[..., None])
    assert at.any(-1)[has].all()
    bad = ~np.isfinite(S.x_rx(c))
    assert nr[:, bad].max(initial=0) == 0 and np.isnan(tt[:, bad]).all() and np.isnan(ta[:, bad]).all()


def compare_roots(c, land, ref, got, m, tol_a, times=1.0):
    """roots ref / got = (tt_all, alpha_all) [R, E, 4] on the mask m [R, E, 4] -> (number compared, worst |dt|, worst |dalpha| / allowed);
    allowed = times x (tol_a + NOISE / slope)"""
    if not m.any():
        return 0, 0.0, 0.0
    dt = np.abs(got[0] - ref[0])[m]
    da = np.abs(got[1] - ref[1])[m]
    slope = S.slopes(c, land, ref[1])[m]
    with np.errstate(invalid="ignore"):
        steep = slope > FLAT
    allow = times * (tol_a + NOISE / np.maximum(np.where(steep, slope, FLAT), FLAT))
    ratio = np.where(steep, da / allow, 0.0)
    return int(m.sum()), float(dt.max()), float(ratio.max())


def against_oracle(rtus, name, fast=False):
    c = S.CASES[name]
    z = S.census(name)
    out = gpu(rtus, name, fast)
    well_formed(c, out)
    tt, ar, ta, aa, nr = (a[z.rows] for a in out)
    E = S.x_rx(c).size
    one_lane = c.path in ONE_LANE
    tol_t, tol_a = (FAST_T, FAST_A) if fast else (TOL_T, TOL_A1 if one_lane else TOL_A3)
    differ = z.clean & (nr != z.nroots)
    if fast:
        assert np.all(differ.sum(1) <= (FAST_CNT + 2.0 / E) * z.clean.sum(1)), f"{name}: root counts differ on {differ.sum(1).max()} clean elements of a row"
    else:
        r, e = (np.argwhere(differ)[0] if differ.any() else (0, 0))
        assert not differ.any(), (f"{name} ({c.path}): root counts differ on {int(differ.sum())} clean elements, first row {int(z.rows[r])} "
                                  f"element {e}: gpu {int(nr[r, e])}, oracle {int(z.nroots[r, e])}")
    same = z.clean & (nr == z.nroots)
    assert np.array_equal(np.isnan(ta[same]), np.isnan(z.ta[same]))
    with np.errstate(invalid="ignore"):
        assert not (np.diff(aa, axis=-1) <= 0)[z.clean].any()
    m = same[..., None] & np.isfinite(z.ta)
    n, wt, wa = compare_roots(c, z.land, (z.ta, z.aa), (ta, aa), m, tol_a)
    # the least-time outputs: the time always; the angle where the oracle's least time stands clear of its other roots (the centre
    # element over the centred pipe has two mirror paths of one time: which of them is "the" least is rounding)
    has = same & (z.nroots > 0)
    wl = float(np.abs(tt - z.tmin)[has].max())
    by_time = np.where(np.isfinite(z.ta), z.ta, np.inf)
    clear = has & (np.sort(by_time, axis=-1)[..., 1] - z.tmin > 2.0 * tol_t)
    a_least = np.take_along_axis(z.aa, np.argmin(by_time, axis=-1)[..., None], -1)
    _, _, wla = compare_roots(c, z.land, (z.tmin[..., None], a_least), (tt[..., None], ar[..., None]), clear[..., None], tol_a)
    print(f"{name}{' fast' if fast else ''}: {c.path}, {len(z.rows)} rows, {int(z.clean.sum())} clean elements of {z.clean.size}, {n} roots compared, "
          f"worst |dt| {wt:.2e} s (least time {wl:.2e} s), worst |dalpha| / allowed {wa:.3f} (least-time root {wla:.3f}; allowed = {tol_a:.0e} rad + "
          f"{NOISE:.0e} m / slope)")
    assert n > 2000
    assert wt <= tol_t and wl <= tol_t and wa <= 1.0 and wla <= 1.0
    return c, z, m


ORACLE_CASES = list(S.CASES)


@pytest.mark.parametrize("name", ORACLE_CASES)
def test_case_against_the_oracle(rtus, name):
    """Equal root counts on every clean element, every root, the least-time outputs, the outputs' form on every element — and WHAT IS
    SEEN: some compared root comes from the pair of grid rays that straddles two 64-ray blocks; in the 256-lane cases some compared
    root belongs to an element whose workgroup's bracket list is longer than 256 (a second trip of the list loop); a duplicated
    element gets the same roots (one-lane bits may depend on a bracket's wave-mates: tolerance, not bits)."""
    c, z, m = against_oracle(rtus, name)
    assert (z.bidx[m] % 64 == 63).any()
    if c.lanes == 256:
        lists, wg = S.workgroup_lists(name)
        long_list = (lists[wg[z.rows]] > 256)[..., None] & m
        print(f"{name}: {int(long_list.sum())} compared roots in workgroups with a list longer than 256")
        assert long_list.any()
    if "ragged" in name:
        tt, ar, ta, aa, nr = (a[z.rows] for a in gpu(rtus, name))
        both = z.clean[:, 1] & z.clean[:, 3]
        assert np.array_equal(nr[:, 1][both], nr[:, 3][both]) and (nr[:, 1][both] > 0).any()
        d = np.abs(ta[:, 1] - ta[:, 3])[both]
        assert np.array_equal(np.isnan(ta[:, 1])[both], np.isnan(ta[:, 3])[both]) and np.nanmax(d) <= 2.0 * TOL_T


@pytest.mark.parametrize("name", ["A+", "B+", "C+"])
def test_fast_against_the_oracle(rtus, name):
    against_oracle(rtus, name, fast=True)


def _grid_clean(name, rows):
    """what can be said about rows the oracle did not solve: at most four brackets and no grid ray on the element (both sides of such a
    comparison share ONE grid trace, so a bracket is a bracket for both)"""
    g = S.grid_census(name)
    return (g.cnt[rows] <= S.MAX_ROOTS) & ~g.near[rows]


def _agree(c, name, rows, a, b, what):
    """Two solves of the same rows (a, b: outputs restricted to them; ``rows`` index the case ``name``) agree within TWICE the tolerances,
    each being within once of the truth, and in their root counts.  Rows the oracle has not solved are compared wherever the grid
    trace is unambiguous; where such a row disagrees, the oracle is asked whether IT is ambiguous there (its clean mask) — only then
    is the element left out."""
    well_formed(c, a), well_formed(c, b)
    ok = _grid_clean(name, rows).copy()
    z = S.census(name)
    solved = np.isin(rows, z.rows)
    ok[solved] &= z.clean[np.searchsorted(z.rows, rows[solved])]
    land = S.land_all(c.n)[:, :c.T, :].reshape(S.G * c.T, c.n)[rows]
    slope = S.slopes(c, land, a[3])
    steep = slope > FLAT
    allow = 2.0 * (TOL_A1 + NOISE / np.maximum(np.where(steep, slope, FLAT), FLAT))
    with np.errstate(invalid="ignore"):
        both = np.isfinite(a[2]) & np.isfinite(b[2])
        off = both & ((np.abs(a[2] - b[2]) > 2.0 * TOL_T) | (steep & (np.abs(a[3] - b[3]) > allow)))
        bad = (a[4] != b[4]) | off.any(-1) | (np.abs(a[0] - b[0]) > 2.0 * TOL_T)
    ask = np.flatnonzero((bad & ok).any(1) & ~solved)
    assert ask.size <= 32, f"{what}: {ask.size} rows disagree"
    if ask.size:
        ok[ask] &= S.oracle_rows(name, rows[ask]).clean
    differ = ok & (a[4] != b[4])
    assert not differ.any(), f"{what}: root counts differ on {int(differ.sum())} elements, first (row, element) {np.argwhere(differ)[:1].tolist()}"
    m = ok[..., None] & np.isfinite(a[2])
    n, wt, wa = compare_roots(c, land, (a[2], a[3]), (b[2], b[3]), m, TOL_A1, times=2.0)
    has = ok & (a[4] > 0)
    wl = float(np.abs(a[0] - b[0])[has].max())
    print(f"{what}: {len(rows)} rows ({int(solved.sum())} solved by the oracle, {ask.size} more asked), {int(ok.sum())} elements of {ok.size}, "
          f"{n} roots compared, worst |dt| {wt:.2e} s (least time {wl:.2e} s), |dalpha| / (2 x allowed) {wa:.3f}")
    assert n > 2000 and wt <= 2.0 * TOL_T and wl <= 2.0 * TOL_T and wa <= 1.0


@pytest.mark.parametrize("lo,hi", [("A-", "A+"), ("B-", "B+"), ("C-", "C+")])
def test_either_side_of_a_threshold(rtus, lo, hi):
    """The rows the two shapes share ((g, t) for the smaller shape's t) through the path below and the path above the threshold."""
    cl, ch = S.CASES[lo], S.CASES[hi]
    a, b = gpu(rtus, lo), gpu(rtus, hi)
    rows_lo = np.arange(S.G * cl.T)
    rows_hi = (rows_lo // cl.T) * ch.T + rows_lo % cl.T
    _agree(ch, hi, rows_hi, tuple(x[rows_lo] for x in a), tuple(x[rows_hi] for x in b), f"{lo} ({cl.path}) | {hi} ({ch.path})")


def test_every_row_of_b_plus_against_small_calls(rtus):
    """A consistency check over the rows the oracle's sample skips (not the reference): all 2,024 rows of B+ (FULL) against the same
    rows solved in calls of 8 x 63 = 504 rows, the three-lane one-launch path every other test compares with the oracle."""
    c = S.CASES["B+"]
    E = S.x_rx(c).size
    parts = []
    for t0 in range(0, c.T, 63):
        tx = S.TX_ALL[t0:min(t0 + 63, c.T)]
        assert rtus.solve_path(S.G, tx.size, c.n, E) == "ROW"
        parts.append(_call(rtus, c, tx=tx))
    small = tuple(np.concatenate([p[k] for p in parts], axis=1).reshape((S.G * c.T, E) + parts[0][k].shape[3:]) for k in range(5))
    _agree(c, "B+", np.arange(S.G * c.T), small, gpu(rtus, "B+"), "B+ in calls of 504 rows (ROW) | B+ (FULL)")


@pytest.mark.parametrize("name", ["A+", "B+"])
def test_the_same_call_twice_gives_the_same_bits(rtus, name):
    c = S.CASES[name]
    first = gpu(rtus, name)
    again = _call(rtus, c)
    for k, (a, b) in enumerate(zip(first, again)):
        assert np.array_equal(a, b.reshape(a.shape), equal_nan=True), NAMES[k]


@pytest.mark.parametrize("fast", [False, True])
@pytest.mark.parametrize("name", ["A+", "B+"])
def test_every_entry_gives_the_same_bits(rtus, name, fast):
    """The host API, SolvePlan.run, SolvePlan.run(polyline_ready=True) and a replayed graph of the plan (bench.py's path): one launcher,
    one workspace layout, the same grid — the same bits, in both arithmetics."""
    import torch
    dev = import_module("ray-tracing-ultrasound_amd.device")
    c = S.CASES[name]
    x = S.x_rx(c)
    host = gpu(rtus, name, fast)
    t64 = lambda a: torch.tensor(np.array(a, dtype=np.float64), device="cuda")     # (a copy: the cases' arrays are read-only)
    args = [t64(S.PIPES), t64(S.TX_ALL[:c.T]), t64(np.full(c.T, D_PLANE)), t64(S.alpha_grid(c.n)), t64(x)]
    plan = dev.SolvePlan(S.G, c.T, c.n, x.size, params=rtus.Params(), fast=fast, all_roots=True)

    def same(o, what):
        torch.cuda.synchronize()
        for k, h in zip(NAMES, host):
            assert np.array_equal(o[k].cpu().numpy().reshape(h.shape), h, equal_nan=True), f"{what}: {k}"

    def clear(o):
        for v in o.values():
            v.zero_()

    same(plan.run(*args), "SolvePlan.run")
    clear(plan.out)
    same(plan.run(*args, polyline_ready=True), "SolvePlan.run(polyline_ready=True)")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        plan.run(*args)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        plan.run(*args)
    clear(plan.out)
    g.replay()
    same(plan.out, "graph replay")

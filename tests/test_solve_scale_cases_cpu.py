"""CPU: the premises of tests/test_gpu_solve_scale.py, proved on the oracle alone, and rtus_solve_path on both sides of every
threshold of the solve's launcher.

The GPU test compares root COUNTS for equality on clean elements and looks at specific places of the one-lane kernel (a bracket list
longer than one trip of the workgroup, the pair of grid rays that straddles two 64-ray blocks, a ragged last workgroup).  Whether the
cases hold such places is a property of the inputs, so it is asserted here, where no GPU is needed.  Per case (oracle.cport only):
  - at most 1 % of the elements are not clean (tests/solve_scale_cases.py says what that means; measured 0.012 - 0.024 %:
    2 - 8 elements);
  - at least 1,000 clean elements have two roots or more, some have one, some three;
  - some clean root's bracket has its lower ray at index % 64 == 63;
  - the 256-lane cases (B+, C+) have workgroups whose bracket list is longer than 256 (259 of 514, 50 of 144);
  - the 128-lane cases CANNOT have one with this family: a list needs more than two brackets per element lane on average, and the
    family has two for most elements and three for a few tens in 33,000 — its lists peak at exactly 256 (asserted: <= 256, and some
    list is full).  The second trip of the list loop is therefore checked through the 256-lane cases only;
  - the last workgroup of B- (96 element lanes of 128), A+T65 (8 of 128) and B+ (232 of 256) is ragged.  A+ itself is 33,280 =
    260 x 128 element lanes, every workgroup full — which is why A+T65 exists;
  - solve_path names the expected path."""
import os
import re
from importlib import import_module

import numpy as np
import pytest

import solve_scale_cases as S
from conftest import ROOT


def test_the_cases_use_the_librarys_constants(rtus):
    assert S.ALPHA_MAX == rtus.ALPHA_MAX and S.MAX_ROOTS == 4
    assert np.array_equal(S.APERTURES["ref65"], rtus.reference_elements())
    hdr = open(os.path.join(ROOT, "include", "rtus.h")).read()
    assert int(re.search(r"#define\s+RTUS_MAX_ROOTS\s+(\d+)", hdr).group(1)) == S.MAX_ROOTS
    for x in (S.APERTURES["ref65_ragged"], S.APERTURES["lin513_ragged"]):
        assert np.isnan(x).sum() == 1 and x[3] == x[1] and not np.all(np.diff(x[np.isfinite(x)]) > 0)


@pytest.mark.parametrize("name", list(S.CASES))
def test_case_premises(rtus, name):
    c = S.CASES[name]
    z = S.census(name)
    E = S.x_rx(c).size
    assert rtus.solve_path(S.G, c.T, c.n, E) == c.path
    share = float((~z.clean).mean())
    hist = np.bincount(z.nroots[z.clean], minlength=5)
    b = z.bidx[z.clean]
    straddle = int(((b >= 0) & (b % 64 == 63)).sum())
    print(f"{name}: {S.n_tasks(c)} tasks, {c.path}; {len(z.rows)} rows by the oracle, not clean {100 * share:.3f} % "
          f"({int((~z.clean).sum())} elements: {int((z.cnt > S.MAX_ROOTS).sum())} with more than four brackets, "
          f"{int((z.cnt != z.nroots).sum())} brackets != roots, {int(z.near.sum())} with a grid ray within 1e-9 m, {int(z.noisy.sum())} with a "
          f"root where the oracle's own x_land scatters by more than {S.NOISE_CAP:.0e} m); "
          f"clean elements with 0..4 roots {hist.tolist()}; {straddle} clean roots in a straddling pair")
    assert share <= S.NOT_CLEAN_CAP
    assert hist[2:].sum() >= 1000 and hist[1] > 0 and hist[3] > 0
    assert straddle >= 1
    # on a clean element the oracle's k-th root lies in the k-th bracket of its own grid trace
    alpha = S.alpha_grid(c.n)
    m = z.clean[..., None] & np.isfinite(z.aa)
    j = np.searchsorted(alpha, z.aa[m], side="right") - 1
    assert np.array_equal(np.isfinite(z.aa)[z.clean], (z.bidx >= 0)[z.clean])
    assert np.all((j == z.bidx[m]) | (j == z.bidx[m] + 1))              # (+ 1: a root AT the bracket's upper ray, to rounding)
    if not c.lanes:
        return
    lists, wg = S.workgroup_lists(name)
    print(f"{name}: {lists.size} workgroups, longest bracket list {int(lists.max())}, {int((lists > 256).sum())} longer than 256")
    if c.lanes == 256:
        assert (lists > 256).sum() >= 10
        assert (lists[wg[z.rows]] > 256)[z.clean & (z.nroots > 0)].any()   # ... and the oracle's rows reach into one
    else:
        assert lists.max() <= 256 and ((lists == 256).any() or "ragged" in name)     # (the NaN element takes two brackets away)
    if name in ("A+T65", "B-", "B+"):
        assert S.n_tasks(c) % c.lanes != 0
        assert np.isin(np.unique(np.flatnonzero((wg == wg.max()).any(1))), z.rows).all()    # every row of the ragged workgroup is compared
    if name == "A+":
        assert S.n_tasks(c) % c.lanes == 0
    if E > 512:
        assert E % 64 == 1                                    # the last chunk of a row has one live lane


def test_cases_sit_on_either_side_of_the_thresholds():
    t = {n: S.n_tasks(c) for n, c in S.CASES.items()}
    assert t["A-"] <= 32768 < t["A+"] and t["A+"] - t["A-"] == 8 * 65
    assert t["B-"] <= 131072 < t["B+"] and t["B+"] - t["B-"] == 8 * 65
    assert t["C-"] <= 32768 < t["C+"] and t["C+"] - t["C-"] == 8 * 513
    for n in (256, 257, 258):
        assert (n + 63) // 64 % 8 != 0                        # the mask loop's eight blocks a trip: a partial trip
    assert 257 % 64 == 1                                      # the last block holds one ray: (255, 256) is a straddling pair
    r = S.sample_rows(S.CASES["B+"])
    assert 250 <= r.size <= 290 and np.all(np.diff(r) > 0)


def _path_values():
    hdr = open(os.path.join(ROOT, "include", "rtus.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+RTUS_SOLVE_PATH_(\w+)\s+(\d+)\b", hdr)}


def test_solve_path_on_both_sides_of_every_threshold(rtus):
    """rows = n_geom * n_tx, tasks = rows * n_rx.  ROW: tasks <= 32,768, n <= 1,024, n_rx <= 128; three lanes per bracket up to
    32,768 tasks; masks up to 512 elements; 128 element lanes per workgroup up to 131,072 tasks.  RTUS_SOLVE_ONE_LANE and
    RTUS_SOLVE_THREE_LAUNCHES leave ROW, RTUS_SOLVE_ONE_LANE leaves the three-lane paths too."""
    vals = _path_values()
    assert [k for k, _ in sorted(vals.items(), key=lambda kv: kv[1])] == list(rtus.SOLVE_PATHS) and sorted(vals.values()) == list(range(6))
    P = rtus.solve_path
    L = rtus.lib()
    api = import_module("ray-tracing-ultrasound_amd.api")
    # 32,768 | 32,769 tasks
    for lo, hi, below, above in (((1, 32768, 1), (1, 32769, 1), "ROW", "HALF"),
                                 ((8, 64, 64), (331, 1, 99), "ROW", "HALF"),
                                 ((1, 64, 512), (3, 3641, 3), "TRIO_MASKS", "HALF"),       # n_rx > 128: not ROW below it
                                 ((1, 32, 1024), (1, 11, 2979), "TRIO_SCAN", "SCAN")):
        for (g, t, e), want in ((lo, below), (hi, above)):
            assert g * t * e == (32768 if want == below else 32769)
            assert P(g, t, 257, e) == want, (g, t, e)
    # 131,072 | 131,073 tasks
    for (g, t, e), want in (((1, 131072, 1), "HALF"), ((1, 131073, 1), "FULL"), ((16, 128, 64), "HALF"), ((1, 43691, 3), "FULL"),
                            ((2, 128, 512), "HALF"), ((1, 128, 1024), "SCAN"), ((1, 129, 1024), "SCAN")):
        assert P(g, t, 905, e) == want, (g, t, e)
    # n 1,024 | 1,025 rays (ROW keeps the grid in one workgroup)
    assert P(4, 2, 1024, 65) == "ROW" and P(4, 2, 1025, 65) == "TRIO_MASKS"
    assert P(8, 253, 1024, 65) == P(8, 253, 1025, 65) == "FULL"
    # n_rx 128 | 129
    assert P(1, 10, 905, 128) == "ROW" and P(1, 10, 905, 129) == "TRIO_MASKS"
    assert P(1, 256, 905, 128) == "ROW" and P(1, 256, 905, 129) == "HALF"            # 32,768 | 33,024 tasks
    # n_rx 512 | 513
    assert P(1, 10, 905, 512) == "TRIO_MASKS" and P(1, 10, 905, 513) == "TRIO_SCAN"
    assert P(1, 100, 905, 512) == "HALF" and P(1, 100, 905, 513) == "SCAN"
    assert P(1, 300, 905, 512) == "FULL" and P(1, 300, 905, 513) == "SCAN"
    # the flags
    assert P(4, 2, 905, 65, one_lane=True) == "HALF" and P(4, 2, 905, 65, three_launches=True) == "TRIO_MASKS"
    assert P(4, 2, 905, 65, one_lane=True, three_launches=True) == "HALF"
    assert P(1, 10, 905, 513, one_lane=True) == "SCAN" and P(1, 10, 905, 513, three_launches=True) == "TRIO_SCAN"
    assert P(1, 10, 905, 300, one_lane=True) == "HALF" and P(1, 10, 905, 300, three_launches=True) == "TRIO_MASKS"
    for kw in (dict(one_lane=True), dict(three_launches=True)):
        assert P(8, 64, 257, 65, **kw) == "HALF" and P(8, 253, 257, 65, **kw) == "FULL" and P(8, 8, 257, 513, **kw) == "SCAN"
    # flags that do not choose a scheme (the vector form, the kept polyline) change nothing
    for g, t, n, e in ((4, 2, 905, 65), (8, 64, 257, 65), (8, 253, 257, 65), (8, 8, 257, 513), (8, 7, 257, 513), (1, 10, 905, 300)):
        base = L.rtus_solve_path(g, t, n, e, 0)
        assert base == vals[P(g, t, n, e)]
        assert L.rtus_solve_path(g, t, n, e, api.SHOOT_FAST_MATH | api.POLYLINE_READY) == base
    # the benchmark's shapes
    assert P(210, 1, 905, 65) == "ROW" and P(16, 1024, 905, 65) == "FULL"
    # sizes rtus_solve refuses
    for bad in ((0, 1, 905, 65), (1, 0, 905, 65), (1, 1, 1, 65), (1, 1, 905, 0), (-1, 1, 905, 65), (1 << 20, 1 << 12, 905, 65)):
        assert L.rtus_solve_path(*bad, 0) == -1
        with pytest.raises(ValueError):
            P(*bad)

"""CPU: the input sets of tests/test_gpu_pipe_skip_branches.py (tests/pipe_skip_cases.py) on the oracle alone.  Every set's condition
is computed from the oracle's ``detail`` output and asserted, so that the GPU comparison cannot pass on a set that no longer reaches
its branch; the flag caps (1 % for the two-minima sets, 0.2 % for every other) are conditions too.  On every set: at most two
interior minima of T(beta) and no minimum rejected by rule 1 - the third bracket of the kernel's refine loop and a winner that is not
the earliest minimum are NOT reachable with these geometries (10 and 37 mm pipes, bores from 0.4 to 0.95 of the radius); the day an
input reaches them these assertions say so.

The oracle itself against tests/test_pipe_skip_cpu.py's 40-digit joint solve in (alpha, beta, gamma) on the new kinds of entry: both
minima of two-minima entries (ranked as mpmath ranks them), winners past ALPHA_MAX, points 1 um above the bore.  Bar: that file's,
1e-14 t."""
import numpy as np
import pytest

import pipe_numpy as O
import pipe_skip_cases as K
from test_pipe_skip_cpu import CL, LEGS, _mp_solve


@pytest.mark.parametrize("name", list(K.TWO_MINIMA))
def test_two_minima_sets(name):
    c, o = K.CASES[name], K.oracle(name)
    K.conditions(c, o)
    tw = K.two_minima(o)
    print(f"\n{name}: {tw['idx'].size} unflagged two-minima entries, the later beta wins in {int(tw['later'].sum())}, flagged "
          f"{o['flag'].mean():.4f}; the scan ranks {K.second_bracket(c, tw)} winners second (fp64 model)")
    assert tw["idx"].size >= K.TWO_MINIMA[name]
    if name == K.RANKED_SECOND.name:
        assert K.second_bracket(c, tw) >= K.RANKED_SECOND_MIN
    if name == "mid10 TT":
        assert tw["later"].sum() >= 10 and (~tw["later"]).sum() >= 10
    # the unchosen minimum is another path: its beta and gamma are far from the winner's
    assert np.min(np.abs(tw["w_beta"] - tw["u_beta"])) >= 1e-3 and np.min(np.abs(tw["w_gamma"] - tw["u_gamma"])) >= 1e-3


@pytest.mark.parametrize("leg", ["LL", "LT"])
def test_wide_alpha_sets(leg):
    for name in ("wide " + leg, "wide-default " + leg):
        K.conditions(K.CASES[name], K.oracle(name))
    o = K.oracle("wide " + leg)
    past = np.isfinite(o["t"]) & (np.abs(o["alpha"]) > O.ALPHA_MAX)
    print(leg, "winners past ALPHA_MAX", int(past.sum()), "finite", int(np.isfinite(o["t"]).sum()))
    assert past.sum() >= 200 and np.isfinite(o["t"]).all()


@pytest.mark.parametrize("leg", ["LL", "LT", "TL"])
def test_thin_shell_sets(leg):
    c, o = K.CASES["thin " + leg], K.oracle("thin " + leg)
    K.conditions(c, o)
    assert np.isfinite(o["t"]).all() and not o["flag"].any() and not o["graze"].any()


def test_thin_shell_detour_bound_on_the_oracles():
    """1 um above the bore the LL skip path is the direct path with a detour of at most 2 um: |t_skip - t_direct| <= 2e-6 / c_t (the
    slower wall speed: a bound, not an estimate).  The direct oracle finds a path to most of these points (its wall segment must
    keep off the bore)"""
    c = K.CASES["thin LL"]
    d = O.table(K.LENS, O.Pipe(c.ro, c.off, c.ri, CL), c.xe, c.ze, c.xf[:61], c.zf[:61])["t"]
    s = K.oracle("thin LL")["t"][:, :61]
    both = np.isfinite(d) & np.isfinite(s)
    print("direct paths", int(both.sum()), "of", d.size, "max |dt|", float(np.max(np.abs(s - d)[both])), "bound", 2e-6 / K.CT)
    assert both.sum() >= d.size // 2
    assert np.max(np.abs(s - d)[both]) <= 2e-6 / K.CT


def test_arc_windows():
    n_fin = []
    for b in K.ARC_WINDOWS:
        c, o = K.CASES[f"arc {b}"], K.oracle(f"arc {b}")
        K.conditions(c, o)
        n_fin.append(int(np.isfinite(o["t"]).sum()))
    o = K.oracle(f"arc {K.ARC_WINDOWS[0]}")
    assert o["no_arc"].all() and np.isnan(o["t"]).all()
    print("winners per window", n_fin)
    # the steps in between hold points with an arc and no winner and points with one; the last step holds a winner everywhere
    assert n_fin[-1] == o["t"].size and all(0 < n < o["t"].size for n in n_fin[1:-1]) and n_fin == sorted(n_fin)
    for b in K.ARC_WINDOWS[1:-1]:                             # W on part of the scan: an arc, a W somewhere, and yet no minimum
        mid = K.oracle(f"arc {b}")
        assert mid["graze"].any() and not mid["no_arc"].any()
    # the mirrored points, the window widened upwards: the betas without W are the first ones of the scan
    up = [K.oracle(f"arc up {b}") for b in K.ARC_WINDOWS_UP]
    for b, o in zip(K.ARC_WINDOWS_UP, up):
        K.conditions(K.CASES[f"arc up {b}"], o)
    n_up = [int(np.isfinite(o["t"]).sum()) for o in up]
    print("winners per window, upwards", n_up)
    assert up[0]["no_arc"].all() and n_up[0] == 0 and 0 < n_up[2] < n_up[3] == 128 and n_up == sorted(n_up)


@pytest.mark.parametrize("leg", ["LL", "LT", "TL"])
def test_scan_edge_sets(leg):
    seen = set()
    for case, ed, m, c, fr, b0 in K.scan_cases(leg):
        if (m, c, fr) not in K.SCAN_CPU:
            continue
        o = K.oracle(case.name)
        K.conditions(case, o)
        assert not o["flag"].any()
        n, inside = K.scan_condition(case, o, ed, m, c, fr, b0)
        seen.add((ed, m, c))
    assert len(seen) == 2 * len(K.SCAN_CPU)


def test_edge_and_shape_sets():
    for c in (K.EDGE, *K.SHAPES.values()):
        o = K.oracle(c.name)
        K.conditions(c, o)
        assert np.isfinite(o["t"]).mean() > 0.9


def _against_mp(c, o_t, o_a, o_b, o_g, i, j):
    t, a, b, g = _mp_solve(c.xe[i], c.ze[i], c.xf[j], c.zf[j], K.pipe(c), LEGS[c.leg][1], o_a, o_b, o_g)
    print(c.name, i, j, "dt / t", abs(float(t) - o_t) / o_t)
    assert abs(float(t) - o_t) <= 1e-14 * o_t, (c.name, i, j)
    assert abs(float(a) - o_a) <= 1e-9 and abs(float(b) - o_b) <= 1e-9 and abs(float(g) - o_g) <= 1e-9, (c.name, i, j)
    return t


def test_oracle_against_mpmath_on_the_new_kinds():
    # both minima of three two-minima entries: the closest race, the widest one, and one of another set
    c, o = K.CASES["mid10 TT"], K.oracle("mid10 TT")
    tw = K.two_minima(o)
    race = (tw["u_t"] - tw["w_t"]) / tw["w_t"]
    picks = [(c, o, tw, int(np.argmin(race))), (c, o, tw, int(np.argmax(race)))]
    c2, o2 = K.CASES["thick37 TT"], K.oracle("thick37 TT")
    tw2 = K.two_minima(o2)
    picks.append((c2, o2, tw2, int(np.argmin((tw2["u_t"] - tw2["w_t"]) / tw2["w_t"]))))
    for cc, oo, t2, n in picks:
        p = t2["idx"][n]
        i, j = np.unravel_index(p, oo["t"].shape)
        m = oo["minima"]
        k = np.nonzero(m["entry"] == p)[0]
        tm = {}
        for q in k:
            tm[m["beta"][q]] = _against_mp(cc, m["t"][q], m["alpha"][q], m["beta"][q], m["gamma"][q], i, j)
        assert tm[t2["w_beta"][n]] < tm[t2["u_beta"][n]], (cc.name, i, j)          # mpmath ranks the two as the oracle does
    # two winners past ALPHA_MAX (off the wide interval's ends)
    c, o = K.CASES["wide LT"], K.oracle("wide LT")
    past = np.argwhere(np.isfinite(o["t"]) & (np.abs(o["alpha"]) > O.ALPHA_MAX + 0.01) & (np.abs(o["alpha"]) < K.WIDE - 0.01))
    assert len(past) >= 2
    for i, j in (past[0], past[-1]):
        _against_mp(c, o["t"][i, j], o["alpha"][i, j], o["beta"][i, j], o["gamma"][i, j], i, j)
    # two points 1 um above the bore
    c, o = K.CASES["thin LL"], K.oracle("thin LL")
    for i, j in ((0, 5), (7, 40)):
        assert abs(np.hypot(c.xf[j] - c.off, c.zf[j]) - c.ri - 1e-6) <= 1e-12
        _against_mp(c, o["t"][i, j], o["alpha"][i, j], o["beta"][i, j], o["gamma"][i, j], i, j)

"""GPU: rtus_tt_pipe_skip's decision points against the NumPy oracle (tests/pipe_skip_numpy.py), on the input sets of
tests/pipe_skip_cases.py - entries with two qualifying minima of T(beta) (the winner's beta AND gamma come back), the general
trigonometry instantiation (rtus_pipe_skip_kernel<false>), brackets in the first and the last scan cell and on the seam of the
scan's 64-point LDS tiles, windows that share no arc of the bore with the points or only part of one, points micrometres off the two
circles, non-finite and on-the-boundary inputs, launch shapes at small windows.  Every set's condition is computed by the oracle and
asserted before anything is compared (tests/test_pipe_skip_branches_cpu.py asserts the same conditions without a GPU).

Rules: tests/test_gpu_pipe_skip.py's (_compare: 1e-17 + 1e-13 t, NaN masks equal outside flagged entries, which may only be later;
beta, gamma and free alpha within 1e-9 rad where T'' is firm, pinned alpha bit-equal).  Each docstring names the one-line changes of
the kernel ("Pipe wall: bore-reflected skip legs") that the test caught when they were tried."""
import numpy as np
import pytest

import pipe_numpy as O
import pipe_skip_cases as K
import pipe_skip_numpy as S
from test_gpu_pipe_skip import _compare
from test_pipe_skip_cpu import CL, CT, LEGS

pytestmark = pytest.mark.gpu


def _call(rtus, c, **over):
    kw = K.kernel_kw(rtus, c)
    kw.update(over)
    xe, ze, xf, zf = (kw.pop(k, getattr(c, k)) for k in ("xe", "ze", "xf", "zf"))
    return rtus.skip_travel_time_pipe(xe, ze, xf, zf, return_path=True, **kw)


def _t2(c, ie, jf, beta):
    """T''(beta) of the oracle's problem by a central difference of T'"""
    h = 1e-6
    a = (K.LENS, K.pipe(c), LEGS[c.leg][1], c.xe[ie], c.ze[ie], c.xf[jf], c.zf[jf])
    return (S._dT(*a, beta + h, c.a_lo, c.a_hi)[0] - S._dT(*a, beta - h, c.a_lo, c.a_hi)[0]) / (2 * h)


def _check_path(got, o, sel, c):
    """on the entries sel: beta and gamma, and alpha off the interval's ends, within 1e-9 rad where T'' is firm; alpha pinned at an
    end bit-equal"""
    if not sel.any():
        return
    _, al, be, ga = got
    ie, jf = np.nonzero(sel)
    t2 = _t2(c, ie, jf, o["beta"][sel])
    firm = t2 > 1e-3 * np.median(np.abs(t2))
    da, db, dg = (np.abs(u[sel] - o[k][sel]) for u, k in ((al, "alpha"), (be, "beta"), (ga, "gamma")))
    free = firm & (o["alpha"][sel] > c.a_lo) & (o["alpha"][sel] < c.a_hi)
    print(f"  {c.name}: path, {int(firm.sum())} firm of {int(sel.sum())}: max |dbeta| {np.max(db[firm], initial=0.0):.2e}, |dgamma| "
          f"{np.max(dg[firm], initial=0.0):.2e}, |dalpha| (free) {np.max(da[free], initial=0.0):.2e}")
    assert np.max(db[firm], initial=0.0) <= 1e-9 and np.max(dg[firm], initial=0.0) <= 1e-9
    assert np.max(da[free], initial=0.0) <= 1e-9
    pinned = (o["alpha"][sel] == c.a_lo) | (o["alpha"][sel] == c.a_hi)
    assert np.array_equal(al[sel][pinned], o["alpha"][sel][pinned])


def _against_oracle(rtus, name):
    c, o = K.CASES[name], K.oracle(name)
    K.conditions(c, o)
    got = _call(rtus, c)
    both = _compare(got[0], o, name)
    for g in got[1:]:
        assert np.array_equal(np.isnan(g), np.isnan(got[0])), name
    _check_path(got, o, both & ~o["flag"], c)
    return c, o, got


@pytest.mark.parametrize("name", list(K.TWO_MINIMA))
def test_two_minima(rtus, name):
    """Entries with two interior minima of T(beta), both qualifying: the kernel keeps both brackets, refines both and returns the
    earlier one's time, beta and gamma.  The other minimum is another path (its beta and gamma are at least 1e-3 rad away, asserted
    on the oracle), so a kernel that returned the wrong bracket's gamma with the right time would show.  In the three sets the
    issue names the scan ranks the winner FIRST in every two-minima entry (printed: an fp64 model of its fp32 estimate), so there
    the second bracket is refined and always loses; the set "ranked second" (tests/pipe_skip_cases.py) holds two entries whose
    winner is the second kept bracket.  Measured on MI355X: |dt| <= 1.1e-15 t, |dbeta| <= 2.9e-14, |dgamma| <= 2.4e-14 rad.
    Fails (the ranked-second set only) with only bracket 0 refined: two times 3.3e-6 t late; and with the winner's gamma kept from the
    first qualifying bracket: gamma 0.31 rad off beside a beta within 2e-14.  The three large sets pass under both changes."""
    c, o, got = _against_oracle(rtus, name)
    tw = K.two_minima(o)
    assert tw["idx"].size >= K.TWO_MINIMA[name]
    if name == K.RANKED_SECOND.name:
        assert K.second_bracket(c, tw) >= K.RANKED_SECOND_MIN
    assert np.min(np.abs(tw["w_beta"] - tw["u_beta"])) >= 1e-3 and np.min(np.abs(tw["w_gamma"] - tw["u_gamma"])) >= 1e-3
    tt, _, be, ga = (g.ravel()[tw["idx"]] for g in got)
    print(f"  {name}: {tw['idx'].size} two-minima entries, the later beta wins in {int(tw['later'].sum())}; winners the scan ranks second "
          f"(fp64 model of its fp32 estimate): {K.second_bracket(c, tw)}; max |dt| / t {np.max(np.abs(tt - tw['w_t']) / tw['w_t']):.2e}, |dbeta| "
          f"{np.max(np.abs(be - tw['w_beta'])):.2e}, |dgamma| {np.max(np.abs(ga - tw['w_gamma'])):.2e}")
    assert np.isfinite(tt).all()
    assert np.all(np.abs(tt - tw["w_t"]) <= 1e-17 + 1e-13 * tw["w_t"])
    assert np.max(np.abs(be - tw["w_beta"])) <= 1e-9 and np.max(np.abs(ga - tw["w_gamma"])) <= 1e-9


@pytest.mark.parametrize("leg", ["LL", "LT"])
def test_general_trigonometry(rtus, leg):
    """alpha_lo, alpha_hi = -+1.05 rad: rtus_pipe_skip_kernel<false> and the set-up kernel's sincos instantiation.  As for the direct
    kernel, no change was found that this test alone catches; it shows that the instantiation runs and agrees with the oracle
    (measured: |dt| <= 1.2e-15 t, |dbeta| <= 1.3e-14, |dgamma| <= 5.8e-15 rad).  Fails with neg[e] cleared at every tile."""
    c, ow, gw = _against_oracle(rtus, "wide " + leg)
    past = np.isfinite(ow["t"]) & (np.abs(ow["alpha"]) > O.ALPHA_MAX)
    assert past.sum() >= 200 and np.isfinite(gw[0]).all()
    # a winner whose alpha is inside +-ALPHA_MAX in both the wide and the default call is the same path
    _, od, gd = _against_oracle(rtus, "wide-default " + leg)
    inside = lambda a, b: np.isfinite(a) & np.isfinite(b) & (np.abs(a) < O.ALPHA_MAX) & (np.abs(b) < O.ALPHA_MAX)      # noqa: E731
    same, want = inside(gw[1], gd[1]), inside(ow["alpha"], od["alpha"])
    print(f"  {leg}: winners past ALPHA_MAX {int(past.sum())}, inside it in both calls {int(same.sum())} (oracle {int(want.sum())})")
    assert want.sum() >= 1000 and np.array_equal(same, want)
    assert np.all(np.abs(gw[0][same] - gd[0][same]) <= 1e-17 + 1e-13 * gd[0][same])


@pytest.mark.parametrize("leg", ["LL", "LT", "TL"])
def test_scan_edges(rtus, leg):
    """The winner of one entry in the first and the last scan cell, in the cells either side of the 64-point tile seams (a root
    2e-6 of a cell from the scan point on the seam), and one cell outside either end of the window (NaN).  Measured: |dt| <=
    8.5e-16 t over the 136 windows of each leg.  Fails with neg[e] cleared at the start of every tile (first at n_scan 65, cell 63).
    Whether the refine's bracket shift (rtus_bracket_fix) is pinned here was not tried; the direct file's cases do not pin it."""
    seen = set()
    worst = 0.0
    for case, ed, m, c, fr, b0 in K.scan_cases(leg):
        o = K.oracle(case.name)
        K.conditions(case, o)
        n, inside = K.scan_condition(case, o, ed, m, c, fr, b0)
        tt, al, be, ga = _call(rtus, case)
        both = _compare(tt, o, case.name)
        worst = max(worst, float(np.max(np.abs(tt - o["t"])[both] / o["t"][both], initial=0.0)))
        if inside:
            assert abs(tt[ed, 1] - o["t"][ed, 1]) <= 1e-17 + 1e-13 * o["t"][ed, 1], case.name
            assert abs(be[ed, 1] - b0) <= 1e-9 and abs(al[ed, 1] - o["alpha"][ed, 1]) <= 1e-9, case.name
            assert abs(ga[ed, 1] - o["gamma"][ed, 1]) <= 1e-9, case.name
        else:
            assert np.isnan(tt[ed, 1]) and np.isnan(be[ed, 1]) and np.isnan(ga[ed, 1]), case.name
        seen.add((n, c if inside else None))
    print(f"  {leg}: {len(K.scan_cases(leg))} windows, max |dt| / t {worst:.2e}")
    assert K.SCAN_SEEN <= seen


def test_window_without_an_arc_and_with_a_partial_arc(rtus):
    """16 points whose arcs of the bore no beta of the window 0.6 .. 1.4 shares: an all-NaN table.  The window widened downwards in
    three steps: W exists on part of the scan only (a beta without W is neither side of a bracket), until every point has a winner.
    Then the mirrored points under windows widened upwards, where the betas without W come first in the scan.  Measured: |dt| <=
    8.2e-16 t, |dbeta| <= 4.1e-15, |dgamma| <= 1.4e-15 rad.  NOT caught: "&& g == g" dropped from neg[e].  A beta without W then
    counts as the negative side, and the bracket it makes with the first beta whose T' > 0 is thrown out by rtus_bracket_fix (T' is
    NaN in fp64 at that end); it costs one of the three kept slots and no tested entry has more than two minima.  Fails with
    neg[e] cleared at every tile."""
    n_fin = []
    for b in K.ARC_WINDOWS:
        c, o, got = _against_oracle(rtus, f"arc {b}")
        n_fin.append(int(np.isfinite(got[0]).sum()))
        if b == K.ARC_WINDOWS[0]:
            assert o["no_arc"].all() and all(np.isnan(g).all() for g in got)
    print("  winners per window", n_fin)
    assert n_fin[0] == 0 and 0 < n_fin[1] <= n_fin[2] < n_fin[3] == 128
    # the mirrored points, the window -1.4 .. widened upwards: the betas without W are the first ones of the scan
    n_up = []
    for b in K.ARC_WINDOWS_UP:
        c, o, got = _against_oracle(rtus, f"arc up {b}")
        n_up.append(int(np.isfinite(got[0]).sum()))
    print("  winners per window, upwards", n_up)
    assert n_up[0] == 0 and 0 < n_up[2] < n_up[3] == 128


@pytest.mark.parametrize("leg", ["LL", "LT", "TL"])
def test_thin_shells(rtus, leg):
    """61 points each on the shells 1 um and 30 um above the bore and 30 um under the outer surface: the fp32 scan's r_F - r_inner
    and arccos(r_inner / r_F) are small there and the lengths must not cancel.  LL: 1 um above the bore the bounce is a detour of
    at most 2 um on the direct path to the same point, so |t_skip - t_direct| <= 2e-6 / c_t (the slower wall speed).  Measured:
    |dt| <= 1.4e-15 t, |dbeta| <= 3.2e-15, |dgamma| <= 1.4e-15 rad on all three shells; the detour 3.56e-10 s against the bound
    6.19e-10 s.  NOT caught by this or any other test of the file: the scan's bounce solve started cold at every scan point (vwf
    always NaN) - the warm start saves Newton steps and decides no sign.  Fails with neg[e] cleared at every tile."""
    c, o, got = _against_oracle(rtus, "thin " + leg)
    assert np.isfinite(o["t"]).all() and np.isfinite(got[0]).all()
    if leg == "LL":
        d = rtus.travel_time_pipe(c.xe, c.ze, c.xf[:61], c.zf[:61], c3=CL, r_inner=c.ri, params=rtus.Params(r_outer=c.ro, pipe_offset=c.off))
        both = np.isfinite(d)
        print(f"  direct paths to the shell 1 um above the bore: {int(both.sum())} of {d.size}, max |t_skip - t_direct| "
              f"{np.max(np.abs(got[0][:, :61] - d)[both]):.3e} s, bound {2e-6 / CT:.3e} s")
        assert both.sum() >= d.size // 2
        assert np.max(np.abs(got[0][:, :61] - d)[both]) <= 2e-6 / CT


def test_edge_inputs(rtus):
    """non-finite elements and focal points, focal points exactly on the wall's two circles and at the centre: NaN in all four
    outputs, and nothing else in the call changes a bit.  (Fails with neg[e] cleared at every tile, through its comparison with
    the oracle; none of the five changes tried touches the tests on the wall.)"""
    c, o, base = _against_oracle(rtus, K.EDGE.name)
    assert np.isfinite(base[0]).mean() > 0.9
    # elements: NaN x in slot 2, inf z in slot 7 (the last row of the first block of 8), the others keep their order
    xe, ze = np.insert(c.xe, [2, 6], [np.nan, 0.001]), np.insert(c.ze, [2, 6], [O.D, np.inf])
    assert xe.size == 10 and np.isnan(xe[2]) and np.isinf(ze[7])
    keep = np.array([0, 1, 3, 4, 5, 6, 8, 9])
    got = _call(rtus, c, xe=xe, ze=ze)
    for g, b in zip(got, base):
        assert np.isnan(g[[2, 7]]).all() and np.array_equal(g[keep], b, equal_nan=True)
    ob = K.run_oracle(c._replace(xe=xe, ze=ze))
    assert ob["flag"].mean() <= K.CAP
    _compare(got[0], ob, "bad elements")
    # focal points
    xg, zg = np.insert(c.xf, K.BAD_AT, K.BAD_X), np.insert(c.zf, K.BAD_AT, K.BAD_Z)
    bad = np.zeros(xg.size, dtype=bool)
    bad[K.BAD_AT + np.arange(K.BAD_AT.size)] = True
    assert np.array_equal(xg[~bad], c.xf) and np.isnan(xg[0]) and zg[-1] == -c.ro
    got = _call(rtus, c, xf=xg, zf=zg)
    for g, b in zip(got, base):
        assert np.isnan(g[:, bad]).all() and np.array_equal(g[:, ~bad], b, equal_nan=True)
    ob = K.run_oracle(c._replace(xf=xg, zf=zg))
    assert ob["flag"].mean() <= K.CAP
    _compare(got[0], ob, "bad points")


def test_launch_shapes_at_small_windows(rtus):
    """n_scan in {4, 64, 65} (less than a tile, one tile, one tile and a point) x n_e in {1, 9} x n_f in {1, 257}: every entry is
    the entry of one big call, bit for bit.  Passes under all five changes tried (they are functions of the entry alone)."""
    for n, c in K.SHAPES.items():
        _, _, full = _against_oracle(rtus, c.name)
        assert np.isfinite(full[0]).mean() > 0.9
        n_e0, n_f0 = c.xe.size, c.xf.size
        for n_e in (1, 9):
            for n_f in (1, 257):
                # the last elements and points of the big call
                es, fs = slice(n_e0 - n_e, n_e0), slice(n_f0 - n_f, n_f0)
                part = _call(rtus, c, xe=c.xe[es], ze=c.ze[es], xf=c.xf[fs], zf=c.zf[fs])
                for u, v in zip(part, full):
                    assert np.array_equal(u, v[es, fs], equal_nan=True), (n, n_e, n_f)

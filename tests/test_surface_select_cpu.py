"""CPU: the inputs of tests/test_gpu_surface_branches.py sit on the branches they are built for — asserted with the oracles
(surface_numpy, skip_numpy, pwi_numpy) and the fp64 model of the kernel's selection rule (surface_select_numpy) alone, so an input
set that drifts off its branch fails here, without a GPU.  Each test prints the counts it asserts."""
from fractions import Fraction

import numpy as np
import pytest

import surface_select_numpy as M


@pytest.mark.parametrize("mode", ["elem", "skip", "pw"])
def test_three_near_tied_minima(mode):
    """C1's input: three minima on three bumps tied at F*, and a 25 x 25 patch around it on which a kernel that gates the third
    kept bracket on T(P_j) alone picks late"""
    c = M.tie_case(mode)
    start = np.array(M.TIE[mode]["amps"])
    g, u, o = c["gated"], c["ungated"], c["o"]
    est_err = float(np.max(g["est"] - g["tr"]))
    share = float(np.mean(g["late"] > 1e-13))
    fl = float(np.mean(o["basin"] < M.DX))
    print(f"\n{mode}: Newton steps {c['steps']}, residual {c['res']:.1e} s, bump heights {np.round(c['amps'] * 1e3, 4)} mm "
          f"(start {start * 1e3}), max |s'| {c['slope']:.3f}")
    print(f"  brackets per entry {np.bincount(g['n_br'])}, least clearance {c['clear'].min() * 1e3:.3f} mm, fourth minimum "
          f"{c['fourth'].min():.2e} s after the third, oracle flags {fl:.4f}")
    print(f"  model with the gate: late on {share:.4f} of {g['late'].size} (most {g['late'].max():.2e} s), largest estimate error "
          f"{est_err:.2e} s, gate margin {M.GATE * np.nanmin(g['t']):.2e} s; without the gate: late on "
          f"{float(np.mean(u['late'] > 1e-13)):.4f}")
    assert c["res"] < 1e-15 and c["steps"] < 25
    assert np.all(c["amps"] <= 2 * start) and np.all(c["amps"] >= 0.5 * start)
    assert c["slope"] < 1.0
    assert c["sep"].all()
    assert c["clear"].min() >= 0.5 * M.DX                       # the header's guarantee covers all three minima
    assert c["fourth"].min() >= 100 * est_err                   # RTUS_KEEP3's drop of a 4th bracket is out of play
    assert fl == 0.0
    assert np.array_equal(np.isfinite(o["t"][0]), np.isfinite(c["least"])) and np.max(np.abs(o["t"][0] - c["least"])) <= 1e-16
    assert np.all(g["n_br"] == 3)                               # the scan sees exactly the three minima
    assert share >= 0.05
    assert np.all(u["late"] == 0.0)
    # the kernel's rule: the scan's figure is a lower bound of every bracket's refined time, so no pick is late; how often it
    # still refines the third bracket
    k = c["kernel"]
    slack = k["tr"] - k["est"]
    print(f"  the kernel's rule: late on {float(np.mean(k['late'] > 1e-13)):.4f}, third bracket refined on "
          f"{float(np.mean(k['fate'][k['rank'] == 2] == M.REFINED)):.4f}, refined time less lower bound {slack.min():.2e} .. {slack.max():.2e} s")
    assert np.all(slack >= 0.0) and np.all(k["late"] == 0.0)


@pytest.mark.parametrize("mode", ["elem", "skip", "pw"])
def test_roots_on_scan_points(mode):
    """C2's input: focal points on the refracted ray of a scan point's surface point (and of the points 1e-8 m left and right of
    it), kept where the dense oracle's winner is that root with a basin >= dx: the first and the last interior scan point, every
    tile seam the profile has, random ones.  Plane waves reach no accepted root at the last interior scan point of the 41-sample
    profile (another insonified minimum is earlier there) nor at three of the random ones."""
    tot = 0
    for n_s in M.C2_NS:
        c = M.c2_case(mode, n_s)
        m = c["m"]
        print(f"\n{mode} n_s {n_s} (m {m}): accepted per j {c['accepted']}, kept {c['kept']}, entries {c['xf'].size}")
        must = [1, m - 2] + [j for j in (63, 64, 65, 127, 128) if 1 < j < m - 2]
        if mode == "pw" and n_s == 41:
            must.remove(m - 2)
        assert all(c["kept"][j] >= 1 for j in must), (n_s, c["kept"])
        root = M.scan_points(c["x0"], c["dx"], n_s)[c["j"]] + c["off"]
        assert np.max(np.abs(c["w"]["x"] - root)) < 1e-9 and np.all(c["w"]["basin"] >= c["dx"])
        assert set(np.unique(c["off"])) == {-1e-8, 0.0, 1e-8}
        tot += c["xf"].size
    assert tot >= (400 if mode == "elem" else 150)


def test_validity_edge_profile():
    """C3's input: exact knots, and a spline whose least and greatest depth lie between samples by more than 1e-6 m"""
    zs, smin, smax = M.edge_extremes()
    k = np.arange(M.E_NS)
    assert all(Fraction(M.E_X0) + int(i) * Fraction(M.E_DX) == Fraction(float(M.E_X0 + i * M.E_DX)) for i in k)   # no rounding
    assert M.E_X0 + (M.E_NS - 1) * M.E_DX == M.E_XEND == 2.0 ** -6
    print(f"\nmin zs - smin {zs.min() - smin:.3e} m, smax - max zs {smax - zs.max():.3e} m")
    assert zs.min() - smin > 1e-6 and smax - zs.max() > 1e-6
    coef = M.S.spline(M.E_X0, M.E_DX, zs)
    xx = np.linspace(M.E_X0, M.E_XEND, 8193)
    s, s1, _ = M.S.spline_eval(coef, M.E_X0, M.E_DX, xx)
    assert np.abs(s1).max() < 1.5 and abs(s.min() - smin) < 1e-9 and abs(s.max() - smax) < 1e-9
    assert np.all(M.S.spline_eval(coef, M.E_X0, M.E_DX, M.E_X0 + k[:-1] * M.E_DX)[0] == zs[:-1])      # s = a exactly at a knot


def test_the_scans_figure_is_a_lower_bound_inside_the_guarantee():
    """T(P_j) - (dx / 4) T'(P_j), the figure the kernel ranks a bracket by and gates the third one on, is at or below the
    bracket's refined time wherever the minimum is under the header's guarantee (neighbouring stationary points >= dx / 2 away),
    on the suite's rougher wavy profile (0.8 mm, 6.5 mm period, 1 mm samples); the brackets that exceed it are counted and all
    sit at narrower minima."""
    x0, dx, n_s = M.X0, M.DX, M.NS
    zs = M.Z0 + 0.0008 * np.sin(2 * np.pi * (x0 + dx * np.arange(n_s)) / 0.0065)
    coef = M.S.spline(x0, dx, zs)
    rng = np.random.default_rng(11)
    xf, zf = rng.uniform(-0.019, 0.019, 400), rng.uniform(0.023, 0.045, 400)
    n_in = n_out = over = 0
    for xe in np.linspace(-0.012, 0.012, 8):
        f = M.elem_T(coef, x0, dx, M.C1, M.CL, xe, 0.0, xf, zf)
        r = M.select(f, xf.size, x0, dx, n_s)
        ent, x, kind, _ = M.stationary(f, xf.size, x0, dx, n_s)
        for k in range(r["ent"].size):
            d = np.sort(np.abs(x[ent == r["ent"][k]] - r["xr"][k]))
            inside = d.size < 2 or d[1] >= 0.5 * dx          # (d[0] is the root itself)
            slack = r["tr"][k] - r["est"][k]
            n_in, n_out, over = n_in + inside, n_out + (not inside), over + (slack < 0)
            assert slack >= 0 or not inside, (xe, r["xr"][k], slack, d[:3])
    print(f"\nbrackets under the guarantee {n_in}, narrower {n_out}; figure above the refined time at {over}, all of them narrower")
    assert n_in >= 5000

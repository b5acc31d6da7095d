"""CPU: the skip-leg oracle (tests/pipe_skip_numpy.py) against a 40-digit joint solve in (alpha, beta, gamma) at the corners of the
reference's sweep for LL, LT, TL and TT; Snell's law and the reflection law at the three interfaces; the limit of a point
approaching the bore; mirror symmetry; the oracle's flag cap and counted conditions on the GPU suite's corner sets; argument
validation of rtus_tt_pipe_skip* through ctypes (status codes, no GPU touched) and of the Python layer.

Bar against mpmath: the direct oracle's, 1e-14 t (measured here: at most 9e-16 t over the solves below)."""
import ctypes as C

import mpmath as mp
import numpy as np
import pytest

import pipe_numpy as O
import pipe_skip_numpy as S

mp.mp.dps = 40
LENS = O.Lens()
XE = np.array([-0.0189, 0.0, 0.0189])
ZE = np.full(3, O.D)
XE64 = (np.arange(64) - 31.5) * 0.6e-3
ZE64 = np.full(64, O.D)
CL, CT = 5600.0, 3230.0                                     # the reference's wall speed; the shear speed of tests/test_gpu_skip.py
LEGS = {"LL": (CL, CL), "LT": (CL, CT), "TL": (CT, CL), "TT": (CT, CT)}
CORNERS = [(r, off) for r in (0.01, 0.037, 0.06) for off in (-0.01, 0.0038, 0.01)]
FLAG_CAP = 2e-3
# the 10 mm pipe's default scan (127 points) leaves minima within a scan step of the betas where the bounce starts to graze: the
# oracle flags 1-3 % of those sets.  At these finer scans it flags nothing (checked below for every leg)
N_SCAN = {(0.01, -0.01): 1017, (0.01, 0.0038): 4065, (0.01, 0.01): 1017}


def corner_case(r_outer, off):
    """a sweep corner's input set for the kernel comparison: 8 elements x (5 radii x 21 angles over +-0.45 rad, and a point in the
    bore, in the water, far outside) -> (r_inner, xe, ze, xf, zf, n_scan)"""
    ri = 0.6 * r_outer
    rr, th = np.meshgrid(np.linspace(ri + 1e-4, r_outer - 1e-4, 5), np.linspace(-0.45, 0.45, 21), indexing="ij")
    xf, zf = (off + rr * np.sin(th)).ravel(), (rr * np.cos(th)).ravel()
    xf, zf = np.r_[xf, off, off, off + 2 * r_outer], np.r_[zf, 0.5 * ri, r_outer + 1e-3, 0.0]
    return ri, XE64[::9], ZE64[::9], xf, zf, N_SCAN.get((r_outer, off))


def _wall_points(pipe, depth_frac=0.4, deg=(-14.0, 3.0, 16.0)):
    r = pipe.r - depth_frac * (pipe.r - pipe.ri)
    th = np.radians(np.asarray(deg))
    return pipe.x0 + r * np.sin(th), r * np.cos(th)


def _mp_solve(xe, ze, xf, zf, pipe, c_up, a0, b0, g0):
    """T at the stationary point of the four-segment path near (a0, b0, g0), in mpmath; with the lens leg pinned at an end of the
    interval, in (beta, gamma) only"""
    c1, c2, cd, cu, d = mp.mpf(O.C1), mp.mpf(O.C2), mp.mpf(pipe.c3), mp.mpf(c_up), mp.mpf(O.L0) + mp.mpf(O.H0)
    Tl = mp.mpf(O.L0) / c1 + mp.mpf(O.H0) / c2
    A = c1 ** 2 / c2 ** 2 - 1
    Cc = c1 ** 2 * Tl ** 2 - d ** 2
    E, F = (mp.mpf(float(xe)), mp.mpf(float(ze))), (mp.mpf(float(xf)), mp.mpf(float(zf)))
    R, Ri, X0 = mp.mpf(pipe.r), mp.mpf(pipe.ri), mp.mpf(pipe.x0)

    def T(a, b, g):
        B = 2 * d * mp.cos(a) - 2 * Tl * c1 ** 2 / c2
        h = (-B - mp.sqrt(B ** 2 - 4 * A * Cc)) / (2 * A)
        px, pz = h * mp.sin(a), h * mp.cos(a)
        qx, qz = X0 + R * mp.sin(b), R * mp.cos(b)
        rx, rz = X0 + Ri * mp.sin(g), Ri * mp.cos(g)
        return (mp.sqrt((px - E[0]) ** 2 + (pz - E[1]) ** 2) / c1 + mp.sqrt((qx - px) ** 2 + (qz - pz) ** 2) / c2
                + mp.sqrt((rx - qx) ** 2 + (rz - qz) ** 2) / cd + mp.sqrt((F[0] - rx) ** 2 + (F[1] - rz) ** 2) / cu)
    if abs(a0) == O.ALPHA_MAX:
        a = mp.mpf(float(a0))
        grad = lambda b, g: (mp.diff(lambda v: T(a, v, g), b), mp.diff(lambda v: T(a, b, v), g))      # noqa: E731
        b, g = mp.findroot(grad, (mp.mpf(float(b0)), mp.mpf(float(g0))))
        return T(a, b, g), a, b, g
    grad = lambda a, b, g: (mp.diff(lambda v: T(v, b, g), a), mp.diff(lambda v: T(a, v, g), b),      # noqa: E731
                            mp.diff(lambda v: T(a, b, v), g))
    a, b, g = mp.findroot(grad, (mp.mpf(float(a0)), mp.mpf(float(b0)), mp.mpf(float(g0))))
    return T(a, b, g), a, b, g


@pytest.mark.parametrize("leg", list(LEGS))
@pytest.mark.parametrize("r_outer,off", CORNERS)
def test_oracle_against_mpmath(r_outer, off, leg):
    cd, cu = LEGS[leg]
    pipe = O.Pipe(r_outer, off, 0.6 * r_outer if r_outer != 0.037 else 0.029, cd)
    xf, zf = _wall_points(pipe)
    pairs = (np.array([0, 2]), np.array([0, 2])) if r_outer != 0.037 else (np.array([0, 1, 2]), np.array([2, 1, 0]))
    o = S.table(LENS, pipe, cu, XE, ZE, xf, zf, pairs=pairs, detail=True)
    assert o["n_gamma"].max() <= 1
    n_ok = 0
    for n, (i, j) in enumerate(zip(*pairs)):
        if np.isnan(o["t"][n]):                              # (TL past the critical angle of the conversion: no bounce)
            assert leg != "LL" and leg != "TT"
            continue
        t, a, b, g = _mp_solve(XE[i], ZE[i], xf[j], zf[j], pipe, cu, o["alpha"][n], o["beta"][n], o["gamma"][n])
        print(r_outer, off, leg, i, j, "dt / t", abs(float(t) - o["t"][n]) / o["t"][n])
        assert abs(float(t) - o["t"][n]) <= 1e-14 * o["t"][n], (r_outer, off, i, j)
        assert abs(float(a) - o["alpha"][n]) <= 1e-9 and abs(float(b) - o["beta"][n]) <= 1e-9 and abs(float(g) - o["gamma"][n]) <= 1e-9
        n_ok += 1
    assert n_ok >= 1


@pytest.mark.parametrize("leg", list(LEGS))
def test_oracle_paths_obey_snell_and_the_reflection_law(leg):
    cd, cu = LEGS[leg]
    pipe = O.Pipe(0.037, 0.0038, 0.029, cd)
    xf, zf = _wall_points(pipe, deg=np.linspace(-20, 20, 9))
    o = S.table(LENS, pipe, cu, XE, ZE, xf, zf)
    g = np.isfinite(o["t"])
    assert g.mean() > 0.5
    ie, jf = np.nonzero(g)
    r1, r2, r3 = S.snell_residuals(LENS, pipe, cu, XE[ie], ZE[ie], xf[jf], zf[jf], o["alpha"][g], o["beta"][g], o["gamma"][g])
    free = np.abs(o["alpha"][g]) < O.ALPHA_MAX
    assert np.max(np.abs(r1[free]), initial=0.0) <= 1e-9 and np.max(np.abs(r2)) <= 1e-9 and np.max(np.abs(r3)) <= 1e-9


def test_point_approaching_the_bore():
    """F = R0 + eps n (n the bore's outward normal at R0): the skip LL path to F is the direct path to F's mirror image in the
    bore's tangent at the bounce, eps below the surface to first order, so (T_LL(F) - T_L(R0)) / eps -> cos(i) / c_l, i the angle
    of incidence at R0: positive, at most 1 / c_l, and settled between eps = 1e-5 and 1e-6 m.  (T_L(R0): the direct table of a pipe
    with a bore 1 mm narrower, so that R0 lies inside its wall)"""
    ri, g0 = 0.029, np.radians([-10.0, 2.0, 14.0])
    x0, z0 = 0.0038 + ri * np.sin(g0), ri * np.cos(g0)
    direct = O.table(LENS, O.Pipe(0.037, 0.0038, ri - 1e-3, CL), XE, ZE, x0, z0)["t"]
    assert np.isfinite(direct).all()
    slope = []
    for eps in (1e-5, 1e-6):
        xf, zf = 0.0038 + (ri + eps) * np.sin(g0), (ri + eps) * np.cos(g0)
        t = S.table(LENS, O.Pipe(0.037, 0.0038, ri, CL), CL, XE, ZE, xf, zf)["t"]
        assert np.isfinite(t).all()
        slope.append((t - direct) / eps)
    assert np.all(slope[1] > 0) and np.all(slope[1] <= (1 + 1e-3) / CL)
    assert np.max(np.abs(slope[0] - slope[1]) * CL) <= 1e-2


def test_mirror_symmetry():
    pipe = O.Pipe(0.037, 0.0, 0.029, CT)
    xf, zf = _wall_points(pipe, deg=(-17.0, -4.0, 9.0, 21.0))
    a = S.table(LENS, pipe, CT, XE64[::7], ZE64[::7], xf, zf)
    b = S.table(LENS, pipe, CT, -XE64[::7], ZE64[::7], -xf, zf)
    assert np.isfinite(a["t"]).all()
    assert np.max(np.abs(a["t"] - b["t"]) / a["t"]) <= 1e-14
    assert np.max(np.abs(a["beta"] + b["beta"])) <= 1e-9 and np.max(np.abs(a["gamma"] + b["gamma"])) <= 1e-9


@pytest.mark.parametrize("r_outer,off", CORNERS)
def test_corner_sets_stay_under_the_flag_cap(r_outer, off):
    """the GPU comparison's corner sets, on the oracle alone: flags, the inner problem's minima, and what the sets hold"""
    ri, xe, ze, xf, zf, n_scan = corner_case(r_outer, off)
    graze = 0
    for leg, (cd, cu) in LEGS.items():
        o = S.table(LENS, O.Pipe(r_outer, off, ri, cd), cu, xe, ze, xf, zf, n_scan=n_scan, detail=True)
        assert o["flag"].mean() <= FLAG_CAP, (leg, float(o["flag"].mean()))
        assert o["n_gamma"].max() <= 1 and not o["no_arc"].any() and not (o["rank"] > 0).any(), leg
        assert np.isnan(o["t"][:, -3:]).all()
        graze += int(o["graze"].sum())
    if (r_outer, off) != (0.06, 0.0038):
        assert graze >= 10, graze                            # (TL past the critical angle: entries whose only minima graze)


def _d(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def test_status_codes(rtus):
    L = rtus.lib()
    assert L.rtus_version() >= 111
    p = lambda a: a.ctypes.data                                                       # noqa: E731
    fake = C.c_void_p(256)
    lens = rtus.Params().lens()
    xe, ze, xf, zf, tt = _d([0.0]), _d([O.D]), _d([0.0038]), _d([0.033]), np.zeros(1)
    a_max = rtus.ALPHA_MAX
    for dev in (True, False):
        def call(r_outer=0.037, r_inner=0.029, x_off=0.0038, c3=5600.0, c_up=3230.0, ln=lens, a_lo=-a_max, a_hi=a_max, b_lo=-np.pi / 2,
                 b_hi=np.pi / 2, n_scan=64, e=xe, n_e=1, n_f=1, out=tt, ws=fake, wsb=1 << 30, pipe=True):
            pp = C.byref(rtus.Pipe(r_outer, r_inner, x_off, c3)) if pipe else None
            lp = None if ln is None else C.byref(ln)
            args = (lp, a_lo, a_hi, pp, c_up, b_lo, b_hi, n_scan, None if e is None else p(e), p(ze), n_e, p(xf), p(zf), n_f,
                    None if out is None else p(out), None, None, None)
            return L.rtus_tt_pipe_skip_dev(*args, ws, wsb, None) if dev else L.rtus_tt_pipe_skip(*args, 0)
        # everything rtus_tt_pipe rejects
        assert call(ln=None) == -1 and call(pipe=False) == -1 and call(e=None) == -1 and call(out=None) == -1
        assert call(n_e=0) == -1 and call(n_f=0) == -1 and call(n_scan=3) == -1
        assert call(a_lo=0.5, a_hi=0.5) == -1 and call(a_hi=np.nan) == -1
        assert call(b_lo=0.2, b_hi=0.1) == -1 and call(b_hi=np.inf) == -1
        assert call(c3=0.0) == -1 and call(c3=-5600.0) == -1 and call(c3=np.inf) == -1 and call(c3=np.nan) == -1
        assert call(r_outer=0.0) == -1 and call(r_outer=np.nan) == -1 and call(x_off=np.nan) == -1
        assert call(r_inner=-1e-3) == -1 and call(r_inner=0.037) == -1 and call(r_inner=0.05) == -1 and call(r_inner=np.nan) == -1
        assert call(ln=rtus.Params(c2=np.inf).lens()) == -1
        assert call(r_outer=0.07, x_off=0.01, r_inner=0.05) == -1 and call(r_outer=0.08, x_off=0.0, r_inner=0.05) == -1
        assert call(n_scan=65537) == -5 and call(n_e=65535 * 8 + 1) == -5 and call(n_e=2048, n_scan=1 << 16) == -5
        # its own: no bore, a bad c_up
        assert call(r_inner=0.0) == -1
        assert call(c_up=0.0) == -1 and call(c_up=-3230.0) == -1 and call(c_up=np.inf) == -1 and call(c_up=np.nan) == -1
        if dev:
            assert call(ws=None) == -4 and call(wsb=16) == -4 and call(ws=C.c_void_p(257)) == -4
    assert L.rtus_tt_pipe_skip_workspace_bytes(64, 466) == L.rtus_tt_pipe_workspace_bytes(64, 466) > 0
    assert L.rtus_tt_pipe_skip_workspace_bytes(0, 466) == 0 and L.rtus_tt_pipe_skip_workspace_bytes(64, 65537) == 0


def test_python_layer_before_any_gpu_call(rtus):
    p = rtus.Params(r_outer=0.037, pipe_offset=0.0038)
    with pytest.raises(ValueError):
        rtus.skip_travel_time_pipe([0.0, 1.0], [O.D], [0.0], [0.03], c_down=CL, r_inner=0.029, params=p)
    with pytest.raises(rtus.RtusError) as ei:
        rtus.skip_travel_time_pipe([0.0], [O.D], [0.0], [0.03], c_down=CL, r_inner=0.0, params=p)
    assert ei.value.status == -1
    with pytest.raises(rtus.RtusError):
        rtus.skip_travel_time_pipe([0.0], [O.D], [0.0], [0.03], c_down=CL, c_up=-1.0, r_inner=0.029, params=p)
    with pytest.raises(ValueError):
        rtus.view_legs_pipe(CL, CT, 0.029, [0.0], [O.D], [0.0], [0.03], legs=("LX",), params=p)
    assert "skip_travel_time_pipe" in rtus.__all__ and "view_legs_pipe" in rtus.__all__

"""CPU: the pipe-wall amplitude oracle (tests/pipe_amplitude_numpy.py) against first principles — the ray tube's width against a
finite-difference tube traced with Snell's law through the lens surface, the outer circle and the bore of an offset pipe; a
closed-form point on the axis of a centred pipe (textbook normal-incidence coefficients, a paraxial chain written out by hand);
reciprocity chained over the interfaces; mirror symmetry — and argument validation of rtus_leg_amp_pipe* through ctypes (status
codes, no GPU touched) and of the Python layer."""
import ctypes as C

import numpy as np
import pytest

import pipe_amplitude_numpy as PA
import pipe_numpy as O

LENS = O.Lens()
RO, XOFF, RI = 0.037, 0.0038, 0.029
CL, CT = 5600.0, 3230.0
MEDIA = (2700.0, 3100.0, 1000.0, 7850.0, CL, CT)              # rho_lens, ct_lens, rho_water, rho_wall, c_l, c_t
SP = {"L": CL, "T": CT}
LEGS = ("L", "T", "LL", "LT", "TL", "TT")


# ---------------------------------------------------------------------------------------------- a ray tracer of its own
def _rot(d, a):
    c, s = np.cos(a), np.sin(a)
    return np.array([c * d[0] + s * d[1], -s * d[0] + c * d[1]])      # angle from +z towards +x grows by a


def _snell(d, n, c_in, c_out, reflect):
    sg = 1.0 if d @ n > 0 else -1.0
    n = n * sg
    t = np.array([n[1], -n[0]])
    p = (d @ t) / c_in
    q = np.sqrt(1 / c_out ** 2 - p ** 2)                                # NaN past the critical angle
    return c_out * (p * t + (-q if reflect else q) * n)


def _hit_lens(P, d, a0):
    """the lens point on the line P + l d, by Newton's method in alpha from a0 -> (alpha, point, normal)"""
    a = a0
    for _ in range(60):
        px, pz, p1x, p1z = LENS.point(a)
        f = (px - P[0]) * d[1] - (pz - P[1]) * d[0]
        a -= f / (p1x * d[1] - p1z * d[0])
        if abs(f) < 1e-19:
            break
    px, pz, p1x, p1z = LENS.point(a)
    return a, np.array([px, pz]), np.array([p1z, -p1x]) / np.hypot(p1x, p1z)


def _hit_circle(P, d, cx, r, far):
    v = P - np.array([cx, 0.0])
    b, c = v @ d, v @ v - r * r
    l = -b + (1.0 if far else -1.0) * np.sqrt(b * b - c)                # NaN: the line misses the circle
    Q = P + l * d
    return Q, (Q - np.array([cx, 0.0])) / r


def _trace(start, d, steps, x_off, a0):
    """steps: [(kind, c_before, c_after)], kind 'lens' / 'outer_in' / 'outer_out' / 'bore' -> (last point, direction, angles)"""
    P = np.array(start, dtype=float)
    ang = {}
    for kind, ci, co in steps:
        if kind == "lens":
            ang["alpha"], Q, n = _hit_lens(P, d, a0)
        elif kind == "bore":
            Q, n = _hit_circle(P, d, x_off, RI, False)
            ang["gamma"] = np.arctan2(Q[0] - x_off, Q[1])
        else:
            Q, n = _hit_circle(P, d, x_off, RO, kind == "outer_out")
            ang["beta"] = np.arctan2(Q[0] - x_off, Q[1])
        d = _snell(d, n, ci, co, kind == "bore")
        P = Q
    return P, d, ang


def _steps(leg, up):
    down = [("lens", LENS.c1, LENS.c2), ("outer_in", LENS.c2, SP[leg[0]])]
    if len(leg) == 2:
        down.append(("bore", SP[leg[0]], SP[leg[1]]))
    if not up:
        return down
    return [({"outer_in": "outer_out"}.get(k, k), co, ci) for k, ci, co in down[::-1]]


def _shoot(leg, xe, phi, x_off=XOFF, l_last=0.003):
    """the leg from the element (xe, D) launched at phi from straight down -> (alpha, beta, gamma, F), Snell's law exact; NaNs
    where the ray misses an interface or passes a critical angle"""
    with np.errstate(invalid="ignore"):
        P, d, ang = _trace((xe, O.D), np.array([np.sin(phi), -np.cos(phi)]), _steps(leg, False), x_off, np.arctan2(xe, O.D) * 0.4)
    return ang["alpha"], ang["beta"], ang.get("gamma", np.nan), P + l_last * d


def _offset(P, d, F, dm):
    """where the line P + l d crosses the line through F perpendicular to dm, along (dm_z, -dm_x)"""
    e = np.array([dm[1], -dm[0]])
    M = np.array([[d[0], -e[0]], [d[1], -e[1]]])
    return np.linalg.solve(M, F - P)[1]


def _fd_J(leg, up, xe, al, be, ga, F, delta):
    pipe = O.Pipe(RO, XOFF, RI)
    px, pz, _, _ = LENS.point(al)
    pts = [np.array([xe, O.D]), np.array([px, pz]), np.array(pipe.q(be)[:2])]
    if len(leg) == 2:
        pts.append(np.array([XOFF + RI * np.sin(ga), RI * np.cos(ga)]))
    pts.append(F)
    if up:
        pts = pts[::-1]
    d0 = (pts[1] - pts[0]) / np.hypot(*(pts[1] - pts[0]))
    dm = (pts[-1] - pts[-2]) / np.hypot(*(pts[-1] - pts[-2]))
    w = []
    for sgn in (1, -1):
        P, d, _ = _trace(pts[0], _rot(d0, sgn * delta), _steps(leg, up), XOFF, al)
        w.append(_offset(P, d, pts[-1], dm))
    return (w[0] - w[1]) / (2 * delta)


def _cases(leg, x_off=XOFF):
    for xe in (-0.0189, -0.011, -0.003, 0.0045, 0.012, 0.0189):
        for phi in np.radians([-7.0, -3.0, -1.0, 0.5, 2.0, 5.0]):
            al, be, ga, F = _shoot(leg, xe, phi, x_off)
            rf = np.hypot(F[0] - x_off, F[1])
            if np.isfinite(F).all() and RI < rf < RO:
                yield xe, al, be, ga, F


# ---------------------------------------------------------------------------------------------- 1. spreading
@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("up", [False, True], ids=["down", "up"])
def test_spreading_against_a_finite_difference_ray_tube(leg, up):
    """|J| of the oracle against the width per launch radian of a tube traced with Snell's law, offset pipe; 1e-6 relative (the bar
    of tests/test_amplitude_cpu.py for the same check); both signs of alpha and of beta occur (the lens
    focuses near the origin, left of the pipe's centre: every ray meets the outer circle on the same side of its normal)"""
    pipe = O.Pipe(RO, XOFF, RI)
    checked, signs, worst = 0, set(), 0.0
    for xe, al, be, ga, F in _cases(leg):
        amp, parts = PA.amplitude(LENS, pipe, MEDIA, leg, up, xe, O.D, F[0], F[1], al, be, ga, parts=True)
        assert np.isfinite(amp) and abs(amp) > 0
        J_fd = _fd_J(leg, up, xe, al, be, ga, F, 1e-6)
        rel = abs(abs(parts["J"]) - abs(J_fd)) / abs(J_fd)
        worst = max(worst, rel)
        assert rel <= 1e-6, (leg, up, xe, al, parts["J"], J_fd)
        G_fd = np.sqrt(parts["prod"] / abs(J_fd))
        assert abs(parts["G"] - G_fd) <= 1e-6 * G_fd
        signs.add((np.sign(al), np.sign(be)))
        checked += 1
    print(leg, "up" if up else "down", "checked", checked, "worst relative difference", worst)
    assert checked >= 12 and {a for a, _ in signs} == {-1.0, 1.0} and {b for _, b in signs} == {-1.0, 1.0}


# ---------------------------------------------------------------------------------------------- 2. a closed-form point
def _h_axis():
    """h(0), h''(0) by hand: B = phi_2 + phi_3, S = sqrt(B^2 - 4 A C), h = -(B + S) / (2 A); B'(0) = 0, B''(0) = -phi_3, so
    h''(0) = phi_3 (1 + B / S) / (2 A)"""
    B = LENS.phi_2 + LENS.phi_3
    S = np.sqrt(B * B - 4 * LENS.A * LENS.C)
    return -(B + S) / (2 * LENS.A), LENS.phi_3 * (1 + B / S) / (2 * LENS.A)


def _paraxial(chain):
    """(y, theta) from (0, 1) through ('move', l) / ('refract', R, c_in, c_out) / ('mirror', R): R > 0 with the centre of curvature
    ahead of the ray; refraction n2 th2 = n1 th1 - (n2 - n1) y / R with n = 1 / c; convex mirror (centre ahead) th2 = th1 + 2 y / R
    in the unfolded coordinates"""
    y, th = 0.0, 1.0
    for step in chain:
        if step[0] == "move":
            y += step[1] * th
        elif step[0] == "refract":
            _, R, ci, co = step
            th = (co / ci) * th - (1 - co / ci) * y / R
        else:
            th = th + 2 * y / step[1]
    return y


@pytest.mark.parametrize("leg", ["L", "LL"])
def test_closed_form_point_on_the_axis(leg):
    rl, ctl, rw, r2, cl, ct = MEDIA
    c1, c2 = LENS.c1, LENS.c2
    h0, h2 = _h_axis()
    assert abs(h0 - O.H0) <= 1e-12
    R1 = h0 * h0 / (h0 - h2)                                           # radius of curvature of P at alpha = 0, centre below
    assert R1 > 0
    pipe = O.Pipe(RO, 0.0, RI)
    zf = RI + 0.003 if leg == "LL" else RO - 0.004
    l1, l2 = O.D - h0, h0 - RO
    zl, zw, zs = rl * c1, rw * c2, r2 * cl
    if leg == "L":
        down = [("move", l1), ("refract", R1, c1, c2), ("move", l2), ("refract", RO, c2, cl), ("move", RO - zf)]
        up = [("move", RO - zf), ("refract", -RO, cl, c2), ("move", l2), ("refract", -R1, c2, c1), ("move", l1)]
    else:
        down = [("move", l1), ("refract", R1, c1, c2), ("move", l2), ("refract", RO, c2, cl), ("move", RO - RI), ("mirror", RI),
                ("move", zf - RI)]
        up = [("move", zf - RI), ("mirror", RI), ("move", RO - RI), ("refract", -RO, cl, c2), ("move", l2), ("refract", -R1, c2, c1),
              ("move", l1)]
    ref_down = (2 * zl / (zl + zw)) * (2 * zw / (zw + zs)) / np.sqrt(abs(_paraxial(down)))
    ref_up = (2 * zs / (zs + zw)) * (2 * zw / (zw + zl)) / np.sqrt(abs(_paraxial(up)))
    g = 0.0 if leg == "LL" else None
    for u, ref in ((False, ref_down), (True, ref_up)):
        amp = PA.amplitude(LENS, pipe, MEDIA, leg, u, 0.0, O.D, 0.0, zf, 0.0, 0.0, g)
        assert abs(abs(amp) - ref) <= 1e-12 * ref, (leg, u, abs(amp), ref)
        assert abs(amp.imag) <= 1e-12 * ref and (amp.real > 0) == (leg == "L")      # the bore's -1


# ---------------------------------------------------------------------------------------------- 3. reciprocity
@pytest.mark.parametrize("leg", LEGS)
def test_reciprocity(leg):
    """per interface C_down sqrt(Z_out cos_out / (Z_in cos_in)) = +- C_up sqrt(Z_in cos_in / (Z_out cos_out)) (tests/
    test_amplitude_cpu.py::test_reciprocity); chained, the impedances telescope to Z_F / Z_E and the cosines to the tube's product:
    C_down prod Z_F / Z_E = +- C_up, one sign per leg"""
    pipe = O.Pipe(RO, XOFF, RI)
    rl, ctl, rw, r2, cl, ct = MEDIA
    zr = r2 * SP[leg[-1]] / (rl * LENS.c1)
    signs, n = set(), 0
    for xe, al, be, ga, F in _cases(leg):
        pd = PA.amplitude(LENS, pipe, MEDIA, leg, False, xe, O.D, F[0], F[1], al, be, ga, parts=True)[1]
        pu = PA.amplitude(LENS, pipe, MEDIA, leg, True, xe, O.D, F[0], F[1], al, be, ga, parts=True)[1]
        assert abs(pd["prod"] * pu["prod"] - 1) <= 1e-12
        r = complex(pd["c_lens"] * pd["c_outer"] * pd["c_bore"] * pd["prod"] * zr / (pu["c_lens"] * pu["c_outer"] * pu["c_bore"]))
        assert abs(abs(r) - 1) <= 1e-12 and abs(r.imag) <= 1e-12, (leg, xe, al, r)
        signs.add(np.sign(r.real))
        n += 1
    assert n >= 12 and len(signs) == 1


# ---------------------------------------------------------------------------------------------- 4. mirror symmetry
@pytest.mark.parametrize("leg", LEGS)
@pytest.mark.parametrize("up", [False, True], ids=["down", "up"])
def test_mirror_symmetry(leg, up):
    """x -> -x of the pipe, the elements and the points: |A| is kept; A changes sign exactly when the mode at the point is T (its
    polarisation (-d_z, d_x) is a pseudovector; include/rtus.h)"""
    a, b = O.Pipe(RO, XOFF, RI), O.Pipe(RO, -XOFF, RI)
    sgn = -1.0 if leg[-1] == "T" else 1.0
    n = 0
    for xe, al, be, ga, F in _cases(leg):
        kw = dict(width=0.5e-3, fc=5e6)
        v = PA.amplitude(LENS, a, MEDIA, leg, up, xe, O.D, F[0], F[1], al, be, ga, **kw)
        w = PA.amplitude(LENS, b, MEDIA, leg, up, -xe, O.D, -F[0], F[1], -al, -be, -ga, **kw)
        assert abs(w - sgn * v) <= 1e-12 * abs(v) and abs(v) > 0, (leg, up, xe, v, w)
        n += 1
    assert n >= 12


def test_invalid_entries():
    pipe = O.Pipe(RO, XOFF, RI)
    xe, al, be, ga, F = next(_cases("LT"))
    f = lambda **k: PA.amplitude(LENS, pipe, MEDIA, "LT", False, xe, O.D, F[0], F[1], k.get("al", al), k.get("be", be),   # noqa: E731
                                 k.get("ga", ga))
    assert np.isfinite(f()) and abs(f()) > 0
    for k in ("al", "be", "ga"):
        v = f(**{k: np.nan})
        assert np.isnan(v.real) and np.isnan(v.imag)
    assert f(al=O.ALPHA_MAX) == 0 and f(al=-O.ALPHA_MAX) == 0            # a pinned lens leg
    assert f(be=be + np.pi) == 0                                          # the water segment would arrive from inside the circle
    assert f(ga=ga + np.pi) == 0                                          # the far side of the bore


# ---------------------------------------------------------------------------------------------- 5. status codes, Python layer
def _d(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def test_status_codes(rtus):
    L = rtus.lib()
    assert L.rtus_version() >= 112
    p = lambda a: None if a is None else a.ctypes.data                                # noqa: E731
    lens = rtus.Params().lens()
    xe, ze, xf, zf, ang = _d([0.0]), _d([O.D]), _d([0.0038]), _d([0.033]), _d([0.0])
    amp = np.zeros(2, dtype=np.float32)
    a_max = rtus.ALPHA_MAX
    for dev in (True, False):
        def call(ln=lens, a_lo=-a_max, a_hi=a_max, r_outer=0.037, r_inner=0.029, x_off=0.0038, pipe=True, media=True, rho_lens=2700.0,
                 ct_lens=3100.0, rho_w=1000.0, rho_wall=7850.0, c_l=5600.0, c_t=3230.0, leg=2, direction=0, width=0.0, f_c=0.0, e=xe,
                 n_e=1, f=xf, n_f=1, al=ang, be=ang, ga=ang, out=amp):
            pp = C.byref(rtus.Pipe(r_outer, r_inner, x_off, 0.0)) if pipe else None      # c3 is not read
            mm = C.byref(rtus.PipeMedia(rho_lens, ct_lens, rho_w, rho_wall, c_l, c_t)) if media else None
            args = (None if ln is None else C.byref(ln), a_lo, a_hi, pp, mm, leg, direction, width, f_c, p(e), p(ze), n_e, p(f), p(zf),
                    n_f, p(al), p(be), p(ga), p(out))
            return L.rtus_leg_amp_pipe_dev(*args, None) if dev else L.rtus_leg_amp_pipe(*args, 0)
        assert call(ln=None) == -1 and call(pipe=False) == -1 and call(media=False) == -1
        assert call(e=None) == -1 and call(f=None) == -1 and call(al=None) == -1 and call(be=None) == -1 and call(out=None) == -1
        assert call(n_e=0) == -1 and call(n_f=0) == -1 and call(n_e=-3) == -1
        assert call(leg=-1) == -1 and call(leg=6) == -1 and call(direction=2) == -1 and call(direction=-1) == -1
        for k in ("rho_lens", "ct_lens", "rho_w", "rho_wall", "c_l", "c_t"):
            for v in (0.0, -1.0, np.inf, np.nan):
                assert call(**{k: v}) == -1, (k, v)
        assert call(ln=rtus.Params(c2=np.inf).lens()) == -1 and call(ln=rtus.Params(c1=-6400.0).lens()) == -1
        assert call(c_t=5600.0) == -1 and call(c_t=6000.0) == -1                       # c_t >= c_l
        assert call(ct_lens=6400.0) == -1 and call(ct_lens=7000.0) == -1               # ct_lens >= c1
        assert call(r_outer=0.0) == -1 and call(r_outer=np.nan) == -1 and call(x_off=np.inf) == -1
        assert call(r_inner=-1e-3) == -1 and call(r_inner=0.037) == -1 and call(r_inner=np.nan) == -1
        assert call(r_inner=0.0) == -1                                                 # a skip leg without a bore
        assert call(a_lo=0.5, a_hi=0.5) == -1 and call(a_lo=0.6, a_hi=0.5) == -1 and call(a_hi=np.nan) == -1
        assert call(width=-1e-4) == -1 and call(width=np.nan) == -1
        assert call(width=5e-4, f_c=0.0) == -1 and call(width=5e-4, f_c=-1.0) == -1 and call(width=5e-4, f_c=np.nan) == -1
        assert call(ga=None) == -1                                                     # a skip leg without gamma
        assert call(n_e=65536) == -5
        if dev:
            # accepted by every check (nothing is launched for these: the next check is the only difference to the calls above)
            assert call(leg=0, ga=None, r_inner=0.0, n_e=65536) == -5 and call(width=5e-4, f_c=5e6, n_e=65536) == -5


def test_python_layer_before_any_gpu_call(rtus):
    p = rtus.Params(r_outer=0.037, pipe_offset=0.0038)
    kw = dict(c_l=CL, c_t=CT, rho_wall=7850.0, rho_water=1000.0, rho_lens=2700.0, ct_lens=3100.0, r_inner=0.029, params=p)
    xe, ze, xf, zf = [0.0, 1e-3], [O.D, O.D], [0.0038, 0.004, 0.005], [0.033, 0.033, 0.033]
    ang = np.zeros((2, 3))
    assert "leg_amplitudes_pipe" in rtus.__all__ and "view_amplitudes_pipe" in rtus.__all__
    with pytest.raises(ValueError):
        rtus.leg_amplitudes_pipe("LL", xe, ze, xf, zf, ang, ang, **kw)                  # a skip leg without gamma
    with pytest.raises(ValueError):
        rtus.leg_amplitudes_pipe("LX", xe, ze, xf, zf, ang, ang, ang, **kw)             # a bad leg
    with pytest.raises(ValueError):
        rtus.leg_amplitudes_pipe("L", xe, ze[:1], xf, zf, ang, ang, **kw)               # xe / ze do not pair up
    with pytest.raises(ValueError):
        rtus.leg_amplitudes_pipe("L", xe, ze, xf, zf, ang[:, :2], ang, **kw)            # alpha is not [n_e, n_f]
    with pytest.raises(ValueError):
        rtus.leg_amplitudes_pipe("LT", xe, ze, xf, zf, ang, ang, ang[:1], **kw)         # gamma is not [n_e, n_f]
    with pytest.raises(ValueError):
        rtus.leg_amplitudes_pipe("L", xe, ze, xf, zf, ang, ang, element_width=5e-4, **kw)   # a width without f_c
    with pytest.raises(rtus.RtusError) as ei:
        rtus.leg_amplitudes_pipe("L", xe, ze, xf, zf, ang, ang, **dict(kw, c_t=6000.0))
    assert ei.value.status == -1
    with pytest.raises(ValueError):
        rtus.view_amplitudes_pipe(xe, ze, xf, zf, legs=("LX",), **kw)

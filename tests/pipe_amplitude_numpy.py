"""NumPy oracle of the pipe-wall ray amplitude tables (include/rtus.h, rtus_leg_amp_pipe): the amplitude of one leg E -> P(alpha) ->
Q(beta) -> [R(gamma)] -> F in one direction.  The plane-wave coefficient closed forms and the ray tube are tests/amplitude_numpy.py's
(fluid_solid, solid_fluid, free, _tube), the lens and the circles tests/pipe_numpy.py's; new here are h'', P'' and the turning rates
of the three normals.

Frames (component algebra in (x, z), z up, exactly as the surface section writes it with z down): an interface frame is a unit normal
n and the tangent t = (n_z, -n_x); angles grow from +z towards +x.  Tube normals (fixed orientation) and their turning rates
d(angle of n) / d(arc along t):
    lens   n = (P'_z, -P'_x) / |P'| (towards the water)    K = (P'_x P''_z - P'_z P''_x) / |P'|^3
    outer  n = (Q - Cp) / r_outer                           K = 1 / r_outer
    bore   n = (R - Cp) / r_inner                           K = 1 / r_inner
(_tube re-orients each along the incoming ray and flips K with it).  Coefficient frames: n into the solid at a fluid-solid interface
(into the lens: t = P' / |P'|; into the wall: n = -(Q - Cp) / r_outer), n out of the solid at the bore (n = -(R - Cp) / r_inner)."""
import numpy as np

import amplitude_numpy as A
import pipe_numpy as O


def lens_point2(lens, alpha):
    """P, P' (pipe_numpy's) and P'' of the lens surface: h'' from B = phi_2 + phi_3 cos(alpha), S = sqrt(B^2 - 4 A C),
    h' = -B'(1 + B / S) / (2 A), h'' = -(B''(1 + B / S) + B'^2 / S (1 - B^2 / S^2)) / (2 A)"""
    px, pz, p1x, p1z = lens.point(alpha)
    s, c = np.sin(alpha), np.cos(alpha)
    B = lens.phi_2 + lens.phi_3 * c
    B1, B2 = -lens.phi_3 * s, -lens.phi_3 * c
    S = np.sqrt(B * B - 4.0 * lens.A * lens.C)
    h1 = p1x * s + p1z * c
    h2 = -(B2 * (1.0 + B / S) + B1 * B1 / S * (1.0 - B * B / (S * S))) / (2.0 * lens.A)
    return px, pz, p1x, p1z, h2 * s + 2.0 * h1 * c - px, h2 * c - 2.0 * h1 * s - pz


def lens_curvature(lens, alpha):
    """the signed curvature of P(alpha), (P'_x P''_z - P'_z P''_x) / |P'|^3"""
    _, _, p1x, p1z, p2x, p2z = lens_point2(lens, alpha)
    return (p1x * p2z - p1z * p2x) / np.hypot(p1x, p1z) ** 3


def path(lens, pipe, leg, xe, ze, xf, zf, alpha, beta, gamma=None):
    """the path's unit segments (element towards point), lengths, tube normals and turning rates"""
    px, pz, p1x, p1z, p2x, p2z = lens_point2(lens, alpha)
    n1 = np.hypot(p1x, p1z)
    g = dict(taux=p1x / n1, tauz=p1z / n1, nlx=p1z / n1, nlz=-p1x / n1, Kl=(p1x * p2z - p1z * p2x) / n1 ** 3)
    qx, qz, _, _ = pipe.q(beta)
    g["nqx"], g["nqz"] = (qx - pipe.x0) / pipe.r, qz / pipe.r
    pts = [(xe, ze), (px, pz), (qx, qz)]
    if len(leg) == 2:
        rx, rz = pipe.x0 + pipe.ri * np.sin(gamma), pipe.ri * np.cos(gamma)
        g["nrx"], g["nrz"] = (rx - pipe.x0) / pipe.ri, rz / pipe.ri
        pts.append((rx, rz))
    pts.append((xf, zf))
    g["seg"] = [A._unit(b[0] - a[0], b[1] - a[1]) for a, b in zip(pts[:-1], pts[1:])]
    return g


def amplitude(lens, pipe, media, leg, up, xe, ze, xf, zf, alpha, beta, gamma=None, width=0.0, fc=1.0, a_lo=-O.ALPHA_MAX,
              a_hi=O.ALPHA_MAX, parts=False):
    """the tabulated amplitude (complex128, broadcast over the inputs) of ``leg`` in direction ``up``; media = (rho_lens, ct_lens,
    rho_water, rho_wall, c_l, c_t); the lens's L speed and the water's speed are lens.c1, lens.c2; pipe.c3 is not read"""
    rl, ctl, rw, r2, cl, ct = media
    c1, c2 = lens.c1, lens.c2
    sp = {"L": cl, "T": ct}
    skip = len(leg) == 2
    X, Y = leg[0], leg[-1]
    arrs = [xe, ze, xf, zf, alpha, beta] + ([gamma] if skip else [])
    arrs = np.broadcast_arrays(*(np.asarray(v, dtype=np.float64) for v in arrs))
    xe, ze, xf, zf, alpha, beta = arrs[:6]
    gamma = arrs[6] if skip else None
    with np.errstate(invalid="ignore", divide="ignore"):
        g = path(lens, pipe, leg, xe, ze, xf, zf, alpha, beta, gamma)
        seg = g["seg"]
        cs = [c1, c2, sp[X]] + ([sp[Y]] if skip else [])
        down = [(s[0], s[1], s[2], c) for s, c in zip(seg, cs)]
        ifs = [(g["nlx"], g["nlz"], g["Kl"], False), (g["nqx"], g["nqz"], 1.0 / pipe.r, False)]
        if skip:
            ifs.append((g["nrx"], g["nrz"], 1.0 / pipe.ri, True))
        if up:
            segs, ifs_ = [(-a, -b, L, c) for a, b, L, c in down[::-1]], ifs[::-1]
        else:
            segs, ifs_ = down, ifs
        J, prod = A._tube(segs, ifs_)
        G = np.sqrt(prod / np.abs(J))
        e1, e2, e3 = seg[0], seg[1], seg[2]
        D = A.sinc(width * e1[0] * fc / c1) if width > 0 else np.ones_like(e1[0])
        tqx, tqz = -g["nqz"], g["nqx"]                                 # t of n = -(Q - Cp) / r_outer
        cb = 1.0
        if skip:
            e4 = seg[3]
            tbx, tbz = -g["nrz"], g["nrx"]                             # t of n = -(R - Cp) / r_inner
        if not up:
            cl_ = A.solid_fluid("L", (e1[0] * g["taux"] + e1[1] * g["tauz"]) / c1, rw, c2, rl, c1, ctl)[2]
            co = A.fluid_solid((e2[0] * tqx + e2[1] * tqz) / c2, rw, c2, r2, cl, ct)[1 if X == "L" else 2]
            if skip:
                cb = A.free(X, (e3[0] * tbx + e3[1] * tbz) / sp[X], r2, cl, ct)[0 if Y == "L" else 1]
        else:
            if skip:
                cb = A.free(Y, -(e4[0] * tbx + e4[1] * tbz) / sp[Y], r2, cl, ct)[0 if X == "L" else 1]
            co = A.solid_fluid(X, -(e3[0] * tqx + e3[1] * tqz) / sp[X], rw, c2, r2, cl, ct)[2]
            cl_ = A.fluid_solid(-(e2[0] * g["taux"] + e2[1] * g["tauz"]) / c2, rw, c2, rl, c1, ctl)[1]
        amp = np.conj(D * G * cl_ * co * cb)
        amp = np.where(J == 0, complex(np.inf, np.inf), amp)
        dot = lambda e, nx, nz: e[0] * nx + e[1] * nz                  # noqa: E731
        ray = (dot(e1, g["nlx"], g["nlz"]) > 0) & (dot(e2, g["nlx"], g["nlz"]) > 0)
        ray &= (dot(e2, g["nqx"], g["nqz"]) < 0) & (dot(e3, g["nqx"], g["nqz"]) < 0)
        if skip:
            ray &= (dot(e3, g["nrx"], g["nrz"]) < 0) & (dot(e4, g["nrx"], g["nrz"]) > 0)
        ray &= (alpha != a_lo) & (alpha != a_hi)                        # a pinned lens leg refracts by no law
    amp = np.where(ray, amp, 0j)
    bad = np.isnan(alpha) | np.isnan(beta) | (np.isnan(gamma) if skip else False)
    amp = np.where(bad, np.nan + 1j * np.nan, amp)
    if parts:
        return amp, dict(D=D, G=G, J=J, prod=prod, c_lens=cl_, c_outer=co, c_bore=cb)
    return amp


def outer_slowness(lens, pipe, xe, ze, alpha, beta):
    """|horizontal slowness| of the water segment at the outer circle (a leg's first mode is evanescent-free only below 1 / c)"""
    px, pz, _, _ = lens.point(alpha)
    qx, qz, _, _ = pipe.q(beta)
    ex, ez, _ = A._unit(qx - px, qz - pz)
    nx, nz = (qx - pipe.x0) / pipe.r, qz / pipe.r
    return np.abs(ex * nz - ez * nx) / lens.c2

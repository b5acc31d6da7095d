"""The case lists of the ray-amplitude branch tests (tests/golden/make_amp_branches.py -> tests/golden/amp_branches.npz;
tests/test_amp_branches_cpu.py, tests/test_gpu_amp_branches.py, tests/test_gpu_pipe_amp_branches.py): paths SHOT FORWARD with
Snell's law from chosen slownesses, so that every decision point of rtus_leg_amp_surface / rtus_leg_amp_pipe (include/rtus.h) is
reached on purpose.  No solver is in the loop: both kernels take the path as input.

Surface.  A path is (E, x_entry, [x_back], F).  shoot_surface() refracts E -> S(x_entry) into the leg's first mode, follows it to F
or to the backwall, reflects into the second mode and places F at a chosen length; seek() moves x_entry (or any other scalar) by
bisection in fp64 until a slowness, a cosine, a directivity argument or a tube width takes a chosen value.  The values the classes
are COUNTED by (slownesses, J, D) are not these fp64 numbers but the 40-digit ones the generator stores next to each case.

Pipe.  The tracer is tests/test_pipe_amplitude_cpu.py's (_hit_lens, _hit_circle, _snell), with the radii as arguments.

Everything here is plain fp64 NumPy and deterministic (no random numbers): the generator must reproduce the inputs bit for bit."""
import os

import numpy as np

import surface_numpy as S

LEGS = ("L", "T", "LL", "LT", "TL", "TT")
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "amp_branches.npz")

# ---------------------------------------------------------------------------------------------- surface: media, profiles
STEEL = (1480.0, 1000.0, 5900.0, 3230.0, 7850.0)          # c1, rho1, c_l, c_t, rho2: c1 < c_t < c_l
PERSPEX = (1480.0, 1000.0, 2730.0, 1430.0, 1180.0)        # c_t < c1 < c_l: another order of the slownesses
MEDIA = (STEEL, PERSPEX)
X0, DX, NS, ZB = -0.02, 1e-3, 41, 0.045
PROFILES = ("flat", "wavy", "ripple")
DELTAS = (1e-3, 1e-6, 1e-8)                                # |p c - 1| (at 1e-9 the oracle's own error is 2.8e-7)
DIR_EPS = (1e-3, 1e-6, 1e-8)                               # |u - k| (1e-9 is past the oracle's own conditioning)
W_NULL, FC_NULL = 1e-3, 10e6                               # w / lambda_1 = 6.76: the first two nulls at 8.5 and 17.2 degrees
W_EL, F_C = 0.5e-3, 5e6


def profile(kind):
    x = X0 + DX * np.arange(NS)
    if kind == "flat":
        return np.full(NS, 0.02)
    return 0.02 + (0.0012 if kind == "wavy" else 50e-6) * np.sin(2 * np.pi * x / 0.012)


class Surf:
    def __init__(self, kind):
        self.kind, self.zs = kind, profile(kind)
        self.coef = S.spline(X0, DX, self.zs)

    def at(self, x):
        s, s1, s2 = S.spline_eval(self.coef, X0, DX, np.float64(x))
        return float(s), float(s1), float(s2)

    def frame(self, x):
        s, s1, _ = self.at(x)
        n = np.hypot(1.0, s1)
        return s, -s1 / n, 1.0 / n                          # s, n = (nx, nz); t = (nz, -nx)


def shoot_surface(surf, med, leg, xe, ze, xs, l_last):
    """E -> S(xs) -> [B] -> F by Snell's law -> dict(xent, xback, xf, zf, ps, pb) (pb NaN for a direct leg), or None where the path
    does not exist (E below the tangent, a mode past its critical angle)"""
    c1, _, cl, ct, _ = med
    sp = {"L": cl, "T": ct}
    s, nx, nz = surf.frame(xs)
    tx, tz = nz, -nx
    l = np.hypot(xs - xe, s - ze)
    ux, uz = (xs - xe) / l, (s - ze) / l
    if not ux * nx + uz * nz > 0:
        return None
    p = (ux * tx + uz * tz) / c1
    cx = sp[leg[0]]
    a = 1.0 / cx ** 2 - p * p
    if not a > 0:
        return None
    q = np.sqrt(a)
    dx, dz = cx * (p * tx + q * nx), cx * (p * tz + q * nz)
    if len(leg) == 1:
        return dict(xent=xs, xback=np.nan, xf=xs + l_last * dx, zf=s + l_last * dz, ps=p, pb=np.nan)
    if not dz > 0:
        return None
    xb = xs + (ZB - s) / dz * dx
    pb = dx / cx
    cy = sp[leg[1]]
    a = 1.0 / cy ** 2 - pb * pb
    if not a > 0:
        return None
    return dict(xent=xs, xback=xb, xf=xb + l_last * cy * pb, zf=ZB - l_last * cy * np.sqrt(a), ps=p, pb=pb)


def seek(fn, lo, hi, n=401):
    """an x in [lo, hi] next to a sign change of fn (NaN: undefined there), by a scan and then bisection to neighbouring doubles;
    None without a sign change"""
    xs = np.linspace(lo, hi, n)
    with np.errstate(all="ignore"):
        v = np.array([fn(x) for x in xs], dtype=np.float64)
    k = np.nonzero(np.isfinite(v[:-1]) & np.isfinite(v[1:]) & (np.sign(v[:-1]) * np.sign(v[1:]) <= 0))[0]
    if k.size == 0:
        return None
    a, b, fa = xs[k[0]], xs[k[0] + 1], v[k[0]]
    if fa == 0:
        return float(a)
    for _ in range(200):
        m = 0.5 * (a + b)
        if m == a or m == b:
            break
        with np.errstate(all="ignore"):
            fm = fn(m)
        if not np.isfinite(fm):
            return None
        if (fm > 0) == (fa > 0):
            a = m
        else:
            b = m
    return float(a)


class _List:
    """the growing table of one kernel's cases: one row per (call parameters, element, point, path)"""

    def __init__(self, cols):
        self.cols, self.rows, self.classes = cols, [], []

    def add(self, cls, **kw):
        if cls not in self.classes:
            self.classes.append(cls)
        self.rows.append(dict(kw, cls=self.classes.index(cls)))

    def arrays(self, prefix):
        out = {prefix + "classes": np.array(self.classes)}
        for c, dt in self.cols:
            out[prefix + c] = np.array([r[c] for r in self.rows], dtype=dt)
        return out


S_COLS = (("prof", np.int8), ("med", np.int8), ("leg", np.int8), ("up", np.int8), ("width", np.float64), ("fc", np.float64),
          ("xe", np.float64), ("ze", np.float64), ("xf", np.float64), ("zf", np.float64), ("xent", np.float64),
          ("xback", np.float64), ("cls", np.int16))


def _oracle_J(surf, med, leg, up, c):
    import amplitude_numpy as A                            # (only to PLACE points: the labels come from the 40-digit values)
    with np.errstate(all="ignore"):
        _, parts = A.amplitude(X0, DX, surf.zs, med + (ZB,), leg, up, c["xe"], c["ze"], c["xf"], c["zf"], c["xent"],
                               c["xback"] if len(leg) == 2 else None, parts=True)
    return float(parts["J"])


def _with_length(surf, med, leg, c, l):
    """the path c with its last segment made l long (same direction)"""
    if len(leg) == 1:
        ax, az = c["xent"], surf.at(c["xent"])[0]
    else:
        ax, az = c["xback"], ZB
    l0 = np.hypot(c["xf"] - ax, c["zf"] - az)
    ux, uz = (c["xf"] - ax) / l0, (c["zf"] - az) / l0
    return dict(c, xf=ax + l * ux, zf=az + l * uz)


def caustic_search(span=100000):
    """the search for an exact caustic: wavy profile, leg T, normal incidence at x = +3 mm; around the root of J in zf, +-span ulp of zf, is there
    an input whose J is exactly zero in the fp64 oracle?  -> (zf of the root, number of exact zeros, least |J| seen)"""
    import amplitude_numpy as A
    surf = Surf("wavy")
    xe = 0.003
    f = lambda z: float(A.amplitude(X0, DX, surf.zs, STEEL + (ZB,), "T", False, xe, 0.0, xe, z, xe, parts=True)[1]["J"])   # noqa: E731
    z0 = seek(f, 0.022, 0.03)
    zs = z0 + np.spacing(z0) * np.arange(-span, span + 1)
    J = A.amplitude(X0, DX, surf.zs, STEEL + (ZB,), "T", False, xe, 0.0, xe, zs, xe, parts=True)[1]["J"]
    return z0, zs[J == 0.0], float(np.min(np.abs(J)))


def surface_cases():
    """-> (_List, {profile index: zs})"""
    L = _List(S_COLS)
    surfs = [Surf(k) for k in PROFILES]

    def add(cls, pi, mi, leg, up, c, width=0.0, fc=1.0):
        L.add(cls, prof=pi, med=mi, leg=LEGS.index(leg), up=int(up), width=width, fc=fc,
              **{k: c[k] for k in ("xe", "ze", "xf", "zf", "xent", "xback")})

    def both(cls, pi, mi, leg, c, **kw):
        for up in (False, True):
            add(f"{cls}_{'up' if up else 'down'}", pi, mi, leg, up, c, **kw)

    def shot(pi, mi, leg, xe, ze, xs, l_last):
        c = shoot_surface(surfs[pi], MEDIA[mi], leg, xe, ze, xs, l_last)
        return None if c is None else dict(c, xe=xe, ze=ze)

    def seek_xs(pi, mi, leg, xe, key, target, lo, hi):
        def f(x):
            c = shoot_surface(surfs[pi], MEDIA[mi], leg, xe, 0.0, x, 0.004)
            return 1.0 if c is None else c[key] - target     # (no such path: the slowness is past the wave's own 1 / c)
        x = seek(f, lo, hi)
        if x is None or abs(f(x)) > 1e-12 * abs(target):      # (the sign change was the end of the leg's existence, not the target)
            return None
        return x

    # -- 0. plain paths: every leg and direction on every profile and pair, with the element's directivity
    for pi in range(3):
        for mi in range(2):
            for leg in LEGS:
                for xe, xs in ((-0.0105, -0.009), (-0.0045, -0.0062), (0.0015, 0.0031), (0.0075, 0.0068)):
                    c = shot(pi, mi, leg, xe, 0.0, xs, 0.006)
                    if c is not None:
                        both("plain", pi, mi, leg, c, width=W_EL, fc=F_C)

    # -- 1. critical slownesses at the surface: p c_l = 1 +- delta for legs whose first mode is T (down: the transmitted L goes
    #       evanescent; up: the reflected L does), on the flat and the wavy profile, both pairs
    for mi in range(2):
        cl, ct = MEDIA[mi][2], MEDIA[mi][3]
        for pi in (0, 1):
            for leg in ("T", "TL", "TT"):
                for d in DELTAS:
                    for side, sg in (("minus", -1), ("plus", 1)):
                        xs = seek_xs(pi, mi, leg, -0.0105, "ps", (1 + sg * d) / cl, -0.0105, 0.0195)
                        c = None if xs is None else shot(pi, mi, leg, -0.0105, 0.0, xs, 0.004)
                        if c is not None:
                            both(f"crit_surf_cl_{side}", pi, mi, leg, c)
        # the wave's own grazing angle (1 - delta only): the refracted L of leg L, the refracted T of leg T (steel; in perspex
        # c_t < c1 and p c_t < 1 always)
        for leg, c_own in (("L", cl),) + ((("T", ct),) if ct > MEDIA[mi][0] else ()):
            for d in DELTAS:
                xs = seek_xs(0, mi, leg, -0.0105, "ps", (1 - d) / c_own, -0.0105, 0.0195)
                c = None if xs is None else shot(0, mi, leg, -0.0105, 0.0, xs, 0.004)
                if c is not None:
                    both(f"crit_surf_{'cl' if leg == 'L' else 'ct'}_graze", 0, mi, leg, c)
        # -- the backwall: p c_l = 1 +- delta for T -> T, 1 - delta for the conversions (the L side at grazing)
        for pi in (0, 1):
            for leg, sides in (("TT", (("minus", -1), ("plus", 1))), ("TL", (("minus", -1),)), ("LT", (("minus", -1),))):
                for d in DELTAS:
                    for side, sg in sides:
                        xs = seek_xs(pi, mi, leg, -0.0105, "pb", (1 + sg * d) / cl, -0.0105, 0.0195)
                        c = None if xs is None else shot(pi, mi, leg, -0.0105, 0.0, xs, 0.004)
                        if c is not None:
                            both(f"crit_back_cl_{side}", pi, mi, leg, c)
    # -- the couplant's own slowness on the up legs of the second pair: T arrives at the surface with p c1 = 1 -+ delta.  Below 1 the
    #    water segment leaves at grazing (E just above the surface); past 1 no transmitted ray exists: the path is an input, the
    #    coefficient is that of the evanescent wave in the couplant (include/rtus.h: the path is not checked against Snell's law)
    c1, _, cl, ct, _ = PERSPEX
    for leg in ("T", "TT", "TL"):
        for d in DELTAS:
            for side, sg in (("minus", -1), ("plus", 1)):
                xs, p = 0.004, (1 + sg * d) / c1
                cosw = np.sqrt(2 * d)                       # the water segment's cosine at 1 - delta (kept for 1 + delta)
                ze = 0.02 - 0.012 * cosw
                xe = xs - 0.012 * np.sqrt(1 - cosw * cosw)
                if sg < 0:                                  # put E exactly where Snell wants it: p from the water side
                    f = lambda z: (xs - xe) / np.hypot(xs - xe, 0.02 - z) / c1 - p      # noqa: E731
                    ze = seek(f, 0.02 - 0.024 * cosw, 0.02 - 0.006 * cosw)
                # the solid side, by hand (shoot_surface would refuse p c1 > 1): T leaves S along (p c_t, q c_t)
                q = np.sqrt(1 / ct ** 2 - p * p)
                if leg == "T":
                    c = dict(xent=xs, xback=np.nan, xf=xs + 0.004 * ct * p, zf=0.02 + 0.004 * ct * q)
                else:
                    xb = xs + (ZB - 0.02) / q * p
                    cy = cl if leg == "TL" else ct
                    a = 1 / cy ** 2 - p * p
                    if not a > 0:
                        continue                            # (T -> L at the backwall: p c_l > 1, no reflected L)
                    c = dict(xent=xs, xback=xb, xf=xb + 0.004 * cy * p, zf=ZB - 0.004 * cy * np.sqrt(a))
                add(f"crit_surf_c1_{side}_up", 0, 1, leg, True, dict(c, xe=xe, ze=ze))

    # -- 2. normal incidence, exactly: x_entry == xe == xf (== x_back) on the flat profile
    for xe in (-0.0045, 0.003):
        for leg in LEGS:
            skip = len(leg) == 2
            c = dict(xe=xe, ze=0.0, xent=xe, xback=xe if skip else np.nan, xf=xe, zf=0.031)
            both("normal", 0, 0, leg, c, width=W_EL, fc=F_C)

    # -- 3. directivity: width 0 (f_c not read), u either side of the first two nulls, u < 0
    for leg in ("L", "TT"):
        c = shot(1, 0, leg, -0.0045, 0.0, -0.0031, 0.006)
        for fc in (1.0, 5e6):
            both("dir_width0", 1, 0, leg, c, width=0.0, fc=fc)
    for leg, ks in (("L", (1,)), ("T", (1, 2)), ("TL", (1, 2))):
        for k in ks:
            for eps in DIR_EPS:
                for sg in (-1, 1):
                    for xe, sign in ((-0.0105, 1), (0.0105, -1)):          # the entry right / left of the element: u > 0 / u < 0
                        def f(x):
                            s = surfs[0].at(x)[0]
                            return W_NULL * ((x - xe) / np.hypot(x - xe, s)) * FC_NULL / 1480.0 - sign * (k + sg * eps)
                        xs = seek(f, min(xe, xe + sign * 0.0095), max(xe, xe + sign * 0.0095))
                        c = None if xs is None else shot(0, 0, leg, xe, 0.0, xs, 0.006)
                        if c is not None:
                            both(f"dir_null{'_neg' if sign < 0 else ''}", 0, 0, leg, c, width=W_NULL, fc=FC_NULL)

    # -- 4. the ray tube: under the focusing (x = +3 mm) and the defocusing (x = -3 mm) half-wave of the wavy profile a line of F's
    #       along the last segment, through the leg's own focus where it has one inside the part: J is linear in the last length
    for pi, tag in ((1, "tube"), (2, "ripple")):
        for leg in LEGS:
            # (the ripple also where it slopes: at the crests s' = 0 and the (1 + s'^2)^{3/2} of the curvature is 1)
            for xs in (0.003, -0.003) if pi == 1 else (0.003, -0.003, 0.0015, -0.0045):
                for xe in (xs - 0.001, xs - 0.004):           # (not xs itself: there the T legs are 0 but for the spline's rounding)
                    c0 = shot(pi, 0, leg, xe, 0.0, xs, 0.004)
                    if c0 is None:
                        continue
                    lmax = 0.018 if len(leg) == 1 else 0.02
                    for up in (False, True):
                        ud = "up" if up else "down"
                        for l in ((0.003, 0.006, 0.01, 0.016) if pi == 1 else (0.005, 0.015)):
                            add(f"{tag}_{ud}", pi, 0, leg, up, _with_length(surfs[pi], STEEL, leg, c0, l), width=W_EL, fc=F_C)
                        if pi != 1:
                            continue
                        Jl = lambda l: _oracle_J(surfs[pi], STEEL, leg, up, _with_length(surfs[pi], STEEL, leg, c0, l))   # noqa: E731
                        J1, J2 = Jl(0.004), Jl(0.008)
                        th = (J2 - J1) / 0.004
                        lf = 0.004 - J1 / th if th != 0 else np.inf
                        if not 0.001 < lf < lmax:
                            continue
                        lf -= Jl(lf) / th                   # (J is affine in the last length: one more step lands on the root)
                        for Jt in (1e-9, 1e-7, 1e-5):
                            for sg in (-1, 1):
                                c = _with_length(surfs[pi], STEEL, leg, c0, lf + sg * Jt / th)
                                add(f"{tag}_{ud}", pi, 0, leg, up, c, width=W_EL, fc=F_C)

    # -- 5. the no-ray rule on the steep facet of the wavy profile at x = 0 (slope 0.63): the water segment (condition 1) and the
    #       segment below S (condition 2) either side of the tangent, |cos| = 1e-3 and 1e-9; each alone and both together
    s, nx, nz = surfs[1].frame(0.0)
    tx, tz = nz, -nx
    ze = 0.015
    for leg in ("L", "TT"):
        skip = len(leg) == 2

        def path(c1s, c2s):
            """cosines c1s / c2s of the two segments on n (E to the left, below the facet's tangent when c1s < 0)"""
            f = lambda x: ((0.0 - x) * nx + (s - ze) * nz) / np.hypot(0.0 - x, s - ze) - c1s     # noqa: E731
            xe = seek(f, -0.019, -0.001)
            dx, dz = c2s * nx + np.sqrt(1 - c2s * c2s) * tx, c2s * nz + np.sqrt(1 - c2s * c2s) * tz
            if not skip:
                return dict(xe=xe, ze=ze, xent=0.0, xback=np.nan, xf=0.003 * dx, zf=s + 0.003 * dz)
            xb = (ZB - s) / dz * dx
            return dict(xe=xe, ze=ze, xent=0.0, xback=xb, xf=xb + 0.002, zf=ZB - 0.004)
        for cs in (1e-3, 1e-9):
            both("noray_1_neg", 1, 0, leg, path(-cs, 0.6))
            both("noray_2_neg", 1, 0, leg, path(0.3, -cs))
            both("noray_both", 1, 0, leg, path(-cs, -cs))
        for cs in (1e-3, 1e-4):                             # the ray side: a finite value, compared (why not 1e-9)
            both("noray_1_pos", 1, 0, leg, path(cs, 0.6))
            both("noray_2_pos", 1, 0, leg, path(0.3, cs))

    # -- 6. NaN and infinity in the path
    for leg in LEGS:
        c = shot(1, 0, leg, -0.0045, 0.0, -0.0031, 0.006)
        both("nan_entry", 1, 0, leg, dict(c, xent=np.nan))
        both("inf_entry", 1, 0, leg, dict(c, xent=np.inf))
        both("inf_entry", 1, 0, leg, dict(c, xent=-np.inf))
        if len(leg) == 2:
            both("nan_back", 1, 0, leg, dict(c, xback=np.nan))
            both("inf_back", 1, 0, leg, dict(c, xback=np.inf))
            both("inf_back", 1, 0, leg, dict(c, xback=-np.inf))

    # -- 7. spline addressing: x_entry on the first, the last and interior knots, one ulp either side of an interior knot
    knots = [X0, X0 + 40 * DX, X0 + 7 * DX, X0 + 12 * DX, X0 + 20 * DX, X0 + 26 * DX, X0 + 33 * DX]
    k17 = X0 + 17 * DX
    knots += [np.nextafter(k17, -1.0), k17, np.nextafter(k17, 1.0)]
    for xs in knots:
        for leg in ("L", "TT"):
            for off in (-0.0021, 0.0021, -0.004, 0.004, -0.006, 0.006, -0.012, 0.012):      # the first element from which the leg exists
                c = shot(1, 0, leg, float(xs) + off, 0.0, float(xs), 0.006)
                if c is not None:
                    both("knots", 1, 0, leg, c, width=W_EL, fc=F_C)
                    break
    return L, {i: surfs[i].zs for i in range(3)}


# the least number of cases per class (asserted on the fixture's labels, tests/test_amp_branches_cpu.py)
S_MINIMA = {
    "crit_surf_cl_minus_down": 6, "crit_surf_cl_plus_down": 6, "crit_surf_cl_minus_up": 6, "crit_surf_cl_plus_up": 6,
    "crit_surf_cl_graze_down": 6, "crit_surf_cl_graze_up": 6, "crit_surf_ct_graze_down": 3, "crit_surf_ct_graze_up": 3,
    "crit_back_cl_minus_down": 6, "crit_back_cl_plus_down": 6, "crit_back_cl_minus_up": 6, "crit_back_cl_plus_up": 6,
    "crit_surf_c1_minus_up": 6, "crit_surf_c1_plus_up": 6,
    "normal_down": 4, "normal_up": 4, "dir_width0_down": 2, "dir_width0_up": 2, "dir_null_down": 12, "dir_null_up": 12,
    "dir_null_neg_down": 12, "dir_null_neg_up": 12, "ripple_down": 40, "ripple_up": 40,
    "noray_1_neg_down": 4, "noray_1_pos_down": 4, "noray_2_neg_down": 4, "noray_2_pos_down": 4, "noray_both_down": 4,
    "noray_1_neg_up": 4, "noray_1_pos_up": 4, "noray_2_neg_up": 4, "noray_2_pos_up": 4, "noray_both_up": 4,
    "nan_entry_down": 6, "nan_entry_up": 6, "nan_back_down": 4, "nan_back_up": 4, "inf_entry_down": 12, "inf_entry_up": 12,
    "inf_back_down": 8, "inf_back_up": 8, "knots_down": 10, "knots_up": 10, "plain_down": 60, "plain_up": 60,
}
TUBE_MIN_PER_SIGN = 8                                      # tube_down / tube_up: by the sign of the reference's J


# ---------------------------------------------------------------------------------------------- pipe: geometry, tracer
P_MEDIA = (2700.0, 3100.0, 1000.0, 7850.0, 5600.0, 3230.0)            # rho_lens, ct_lens, rho_water, rho_wall, c_l, c_t
G37 = (0.037, 0.029, 0.0038)                                          # r_outer, r_inner, x_off: tests/test_pipe_amplitude_cpu.py's
G10 = (0.01, 0.006, 0.0038)                                           # the corner where the lens focus lies near the pipe
GFAR = (0.037, 0.029, 0.09)                                           # a pipe beside the lens: the water segment can leave backwards
P_COLS = (("ro", np.float64), ("ri", np.float64), ("xoff", np.float64), ("alo", np.float64), ("ahi", np.float64), ("leg", np.int8),
          ("up", np.int8), ("width", np.float64), ("fc", np.float64), ("xe", np.float64), ("ze", np.float64), ("xf", np.float64),
          ("zf", np.float64), ("alpha", np.float64), ("beta", np.float64), ("gamma", np.float64), ("mir", np.int8), ("cls", np.int16))


def shoot_pipe(geom, leg, xe, phi, l_last):
    """the leg from the element (xe, d) launched at phi from straight down, by Snell's law through the lens surface, the outer circle
    and (skip legs) the bore -> dict(alpha, beta, gamma, xf, zf, pq, pr) (|tangential slowness| at the outer circle and the bore),
    or None where the ray misses an interface or passes a critical angle"""
    import pipe_numpy as O
    from test_pipe_amplitude_cpu import _hit_circle, _hit_lens, _snell, LENS
    ro, ri, xoff = geom
    sp = {"L": P_MEDIA[4], "T": P_MEDIA[5]}
    with np.errstate(invalid="ignore"):
        d = np.array([np.sin(phi), -np.cos(phi)])
        al, P, n = _hit_lens(np.array([xe, O.D]), d, np.arctan2(xe, O.D) * 0.4)
        d = _snell(d, n, LENS.c1, LENS.c2, False)
        Q, nq = _hit_circle(P, d, xoff, ro, False)
        pq = abs(d @ np.array([nq[1], -nq[0]])) / LENS.c2
        be, ga, pr, last = np.arctan2(Q[0] - xoff, Q[1]), np.nan, np.nan, Q
        d = _snell(d, nq, LENS.c2, sp[leg[0]], False)
        if len(leg) == 2:
            R, nr = _hit_circle(Q, d, xoff, ri, False)
            ga, pr, last = np.arctan2(R[0] - xoff, R[1]), abs(d @ np.array([nr[1], -nr[0]])) / sp[leg[0]], R
            d = _snell(d, nr, sp[leg[0]], sp[leg[1]], True)
        F = last + l_last * d
    if not (np.isfinite(F).all() and np.isfinite([al, be]).all()):
        return None
    return dict(alpha=float(al), beta=float(be), gamma=float(ga), xf=float(F[0]), zf=float(F[1]), pq=float(pq), pr=float(pr))


def _pipe_oracle(geom, leg, up, c, key=None, **kw):
    """(only to PLACE points) the fp64 oracle's parts, or one dot product of its path"""
    import pipe_amplitude_numpy as PA
    import pipe_numpy as O
    from test_pipe_amplitude_cpu import LENS
    pipe = O.Pipe(geom[0], geom[2], geom[1])
    with np.errstate(all="ignore"):
        if key is None:
            return PA.amplitude(LENS, pipe, P_MEDIA, leg, up, c["xe"], c["ze"], c["xf"], c["zf"], c["alpha"], c["beta"],
                                c["gamma"] if len(leg) == 2 else None, parts=True, **kw)[1]
        g = PA.path(LENS, pipe, leg, c["xe"], c["ze"], c["xf"], c["zf"], c["alpha"], c["beta"], c["gamma"] if len(leg) == 2 else None)
    seg = g["seg"]
    k, n = {"a": (0, "l"), "b": (1, "l"), "c": (1, "q"), "d": (2, "q"), "e": (2, "r"), "f": (3, "r")}[key]
    return float(seg[k][0] * g[f"n{n}x"] + seg[k][1] * g[f"n{n}z"])


def _radial(geom, leg, xe, alpha, beta, l=0.003):
    """a path by hand: E, P(alpha), Q(beta), then inwards at a slant (R 0.04 rad on from Q, F 3 mm off the circle it left, another
    0.02 rad on) — every wall-side condition holds with a cosine near 1, and no segment meets an interface at normal incidence,
    where the T coefficients are 0 but for rounding"""
    import pipe_numpy as O
    ro, ri, xoff = geom
    if len(leg) == 1:
        a = beta + 0.02
        return dict(xe=xe, ze=O.D, alpha=alpha, beta=beta, gamma=np.nan, xf=xoff + (ro - l) * np.sin(a), zf=(ro - l) * np.cos(a))
    a = beta + 0.06
    return dict(xe=xe, ze=O.D, alpha=alpha, beta=beta, gamma=beta + 0.04, xf=xoff + (ri + l) * np.sin(a), zf=(ri + l) * np.cos(a))


def pipe_cases():
    import pipe_numpy as O
    L = _List(P_COLS)
    AM = O.ALPHA_MAX

    def add(cls, geom, leg, up, c, width=0.0, fc=1.0, alo=-AM, ahi=AM):
        for mir in (0, 1):
            sg = -1.0 if mir else 1.0
            L.add(cls, ro=geom[0], ri=geom[1], xoff=sg * geom[2], alo=-ahi if mir else alo, ahi=-alo if mir else ahi,
                  leg=LEGS.index(leg), up=int(up), width=width, fc=fc, xe=sg * c["xe"], ze=c["ze"], xf=sg * c["xf"], zf=c["zf"],
                  alpha=sg * c["alpha"], beta=sg * c["beta"], gamma=sg * c["gamma"], mir=mir)

    def both(cls, geom, leg, c, **kw):
        for up in (False, True):
            add(f"{cls}_{'up' if up else 'down'}", geom, leg, up, c, **kw)

    def shot(geom, leg, xe, phi, l_last=0.003):
        c = shoot_pipe(geom, leg, xe, phi, l_last)
        if c is None:
            return None
        r = np.hypot(c["xf"] - geom[2], c["zf"])
        return dict(c, xe=xe, ze=O.D) if geom[1] < r < geom[0] else None

    # -- 0. plain paths, with the directivity; and the same with a lens interval past +-1 rad (the kernel's other sincos)
    for leg in LEGS:
        for xe, phi in ((-0.0189, -3.0), (-0.003, 2.0), (0.0045, -1.0), (0.012, 5.0)):
            c = shot(G37, leg, xe, np.radians(phi))
            if c is not None:
                both("plain", G37, leg, c, width=W_EL, fc=F_C)
                both("wide_interval", G37, leg, c, width=W_EL, fc=F_C, alo=-1.05, ahi=1.02)

    # -- 1. critical slownesses (the 10 mm corner): p c_l = 1 +- delta at the outer circle for legs whose first mode is T; at the bore
    #       for T -> T both sides, for the conversions 1 - delta (TL: the reflected L at grazing; LT: the L segment tangent to the bore)
    cl = P_MEDIA[4]

    def crit(cls, leg, key, target, want=2):
        """the first ``want`` elements of a scan of the aperture from which a launch angle with c[key] == target exists"""
        found = 0
        for xe in np.linspace(-0.0189, 0.0189, 22):
            def f(phi):
                c = shoot_pipe(G10, leg, xe, phi, 0.001)
                return 1.0 if c is None else c[key] - target
            phi = seek(f, np.radians(-14.0), np.radians(14.0), n=141)
            if phi is None or abs(f(phi)) > 1e-12 * abs(target):
                continue
            c = shot(G10, leg, xe, phi, 0.001)
            if c is not None:
                both(cls, G10, leg, c)
                found += 1
                if found == want:
                    return
    for d in DELTAS:
        for side, sg in (("minus", -1), ("plus", 1)):
            for leg in ("T", "TT"):
                crit(f"crit_outer_cl_{side}", leg, "pq", (1 + sg * d) / cl)
            for leg in ("TT",) + (("TL", "LT") if sg < 0 else ()):
                crit(f"crit_bore_cl_{side}", leg, "pr", (1 + sg * d) / cl)

    # -- 2. the six no-ray conditions, each failing alone, either side of tangency: a (P - E) . n_lens, b (Q - P) . n_lens,
    #       c (Q - P) . n_outer, d (wall segment) . n_outer, e (segment to R) . n_bore, f (segment from R) . n_bore.  The zero side
    #       goes to |cos| = 1e-9; the ray side stops at 1e-4 (a grazing segment's vertical slowness is lost in fp64)
    def vary(geom, leg, c0, key, name, lo, hi, target, sense):
        """move c0[name] in [lo, hi] until dot product ``key`` is sense * target"""
        f = lambda v: _pipe_oracle(geom, leg, False, dict(c0, **{name: v}), key) - sense * target     # noqa: E731
        v = seek(f, lo, hi, n=2001)
        return None if v is None else dict(c0, **{name: v})

    def place(geom, c0, key, cosv, l=0.003):
        """the last segment (d: from Q; f: from R) at the cosine cosv on the local normal"""
        ro, ri, xoff = geom
        a, r, sg = (c0["beta"], ro, -1.0) if key == "d" else (c0["gamma"], ri, 1.0)
        nx, nz = np.sin(a), np.cos(a)
        s = np.sqrt(1 - cosv * cosv)
        return dict(c0, xf=xoff + r * nx + l * (sg * cosv * nx + s * nz), zf=r * nz + l * (sg * cosv * nz - s * nx))
    sides = [("neg", -1.0, cs) for cs in (1e-3, 1e-9)] + [("pos", 1.0, cs) for cs in (1e-3, 1e-4)]
    for tag, sg, cs in sides:
        for leg in ("L", "TT"):
            c0 = _radial(G37, leg, 0.0189, 0.6, 0.25)
            c = vary(G37, leg, c0, "a", "xe", -3.0, 0.0189, cs, sg)
            if c is not None:
                both(f"noray_a_{tag}", G37, leg, c)
            c0 = _radial(GFAR, leg, 0.0045, 0.4, 0.1)
            c = vary(GFAR, leg, c0, "b", "beta", 0.1, 0.6, cs, sg)
            if c is not None:
                both(f"noray_b_{tag}", GFAR, leg, _radial(GFAR, leg, 0.0045, 0.4, c["beta"]))
            c0 = _radial(G37, leg, 0.0045, 0.1, 0.05)
            c = vary(G37, leg, c0, "c", "beta", 0.05, 3.0, cs, -sg)
            if c is not None:
                both(f"noray_c_{tag}", G37, leg, _radial(G37, leg, 0.0045, 0.1, c["beta"]))
        for leg in ("L", "T"):
            both(f"noray_d_{tag}", G37, leg, place(G37, _radial(G37, leg, 0.0045, 0.1, 0.05), "d", sg * cs))
        for leg in ("LT", "TT"):
            c0 = _radial(G37, leg, 0.0045, 0.1, 0.05)
            c = vary(G37, leg, c0, "e", "gamma", 0.05, 3.0, cs, -sg)
            if c is not None:
                ga = c["gamma"] + 0.02
                both(f"noray_e_{tag}", G37, leg, dict(c, xf=G37[2] + (G37[1] + 0.003) * np.sin(ga), zf=(G37[1] + 0.003) * np.cos(ga)))
            both(f"noray_f_{tag}", G37, leg, place(G37, c0, "f", sg * cs))

    # -- 3. the pinned lens leg: alpha equal to an end of the interval is no ray, one ulp inside is one; a call with its own interval
    for leg in ("L", "LT"):
        for end in (-AM, AM):
            beta = 0.35 * np.sign(end)
            both("pinned", G37, leg, _radial(G37, leg, 0.0189 * np.sign(end), end, beta))
            both("pinned_inside", G37, leg, _radial(G37, leg, 0.0189 * np.sign(end), float(np.nextafter(end, 0.0)), beta))
        c = shot(G37, leg, 0.0045, np.radians(3.0))
        a = c["alpha"]
        both("pinned", G37, leg, c, alo=-0.3, ahi=a)
        both("pinned", G37, leg, c, alo=a, ahi=0.7)
        both("pinned_inside", G37, leg, c, alo=-0.3, ahi=float(np.nextafter(a, 1.0)))
        both("pinned_inside", G37, leg, c, alo=float(np.nextafter(a, -1.0)), ahi=0.7)
        both("pinned_inside", G37, leg, _radial(G37, leg, 0.0189, AM, 0.35), alo=-0.3, ahi=0.7)    # +-ALPHA_MAX is no end of this one

    # -- 4. NaN in the path
    for leg in LEGS:
        c = shot(G37, leg, 0.0045, np.radians(-1.0))
        both("nan_alpha", G37, leg, dict(c, alpha=np.nan))
        both("nan_beta", G37, leg, dict(c, beta=np.nan))
        if len(leg) == 2:
            both("nan_gamma", G37, leg, dict(c, gamma=np.nan))

    # -- 5. the tube at the 10 mm corner: the lens focus lies near the pipe, the width changes sign along the water segment or in the
    #       wall; a line of F's along the last segment and, where it has one inside the wall, through the leg's focus
    for leg in LEGS:
        for xe, phi in ((-0.011, 1.0), (-0.003, -0.5), (0.0045, -1.5), (-0.0189, 2.0)):
            c0 = shot(G10, leg, xe, np.radians(phi), 0.001)
            if c0 is None:
                continue
            ax, az = c0["xf"], c0["zf"]

            def at(l):
                s = shoot_pipe(G10, leg, xe, np.radians(phi), l)
                return dict(c0, xf=s["xf"], zf=s["zf"])
            for up in (False, True):
                ud = "up" if up else "down"
                for l in (0.0007, 0.0015, 0.0025):
                    add(f"tube_{ud}", G10, leg, up, at(l), width=W_EL, fc=F_C)
                Jl = lambda l: float(_pipe_oracle(G10, leg, up, at(l))["J"])     # noqa: E731
                J1, J2 = Jl(0.001), Jl(0.002)
                th = (J2 - J1) / 0.001
                lf = 0.001 - J1 / th if th != 0 else np.inf
                if not 0.0003 < lf < 0.0035:
                    continue
                lf -= Jl(lf) / th
                for Jt in (3e-9, 1e-7, 1e-5):               # (at 1e-9 the oracle's own error is 7.5e-8 here)
                    for sg in (-1, 1):
                        add(f"tube_{ud}", G10, leg, up, at(lf + sg * Jt / th), width=W_EL, fc=F_C)
    # -- 6. the lens focus BEFORE the outer circle, going down (W < 0 on arrival at Q).  No Snell path has it: the focus lies at
    #       the origin, level with the pipe's centre, and a pipe beside it is met past every critical angle.  So by hand: the water
    #       segment from P(alpha) through the origin to the flank of a 10 mm pipe just right of it, then inwards at a slant
    from test_pipe_amplitude_cpu import _hit_circle, LENS
    GB = (0.01, 0.006, 0.0105)
    for al in (-0.36, -0.40, -0.45, -0.50):                # (from the element at x = 0: the one the lens focuses exactly)
        px, pz, _, _ = LENS.point(al)
        P = np.array([px, pz])
        Q, _ = _hit_circle(P, -P / np.hypot(px, pz), GB[2], GB[0], False)
        be = float(np.arctan2(Q[0] - GB[2], Q[1]))
        for leg in ("L", "TT"):
            c = _radial(GB, leg, 0.0, al, be, l=0.002)
            both("focus_before_outer", GB, leg, c, width=W_EL, fc=F_C)
    return L


P_MINIMA = {
    "plain_down": 20, "plain_up": 20, "wide_interval_down": 20, "wide_interval_up": 20,
    "crit_outer_cl_minus_down": 6, "crit_outer_cl_plus_down": 6, "crit_outer_cl_minus_up": 6, "crit_outer_cl_plus_up": 6,
    "crit_bore_cl_minus_down": 6, "crit_bore_cl_plus_down": 6, "crit_bore_cl_minus_up": 6, "crit_bore_cl_plus_up": 6,
    "pinned_down": 8, "pinned_up": 8, "pinned_inside_down": 8, "pinned_inside_up": 8,
    "focus_before_outer_down": 8, "focus_before_outer_up": 8, "nan_alpha_down": 6, "nan_alpha_up": 6, "nan_beta_down": 6, "nan_beta_up": 6, "nan_gamma_down": 4, "nan_gamma_up": 4,
}
for _k in "abcdef":
    for _s in ("neg", "pos"):
        for _d in ("down", "up"):
            P_MINIMA[f"noray_{_k}_{_s}_{_d}"] = 4


# ---------------------------------------------------------------------------------------------- the fixture: loading, oracles, calls
def load():
    with np.load(FIXTURE, allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def oracle_surface(fx):
    """tests/amplitude_numpy.py on every surface case -> complex128 [n]"""
    import amplitude_numpy as A
    zs = [profile(k) for k in PROFILES]
    out = np.zeros(fx["s_ref"].size, dtype=np.complex128)
    with np.errstate(all="ignore"):
        for i in range(out.size):
            leg = LEGS[fx["s_leg"][i]]
            out[i] = A.amplitude(X0, DX, zs[fx["s_prof"][i]], MEDIA[fx["s_med"][i]] + (ZB,), leg, bool(fx["s_up"][i]), fx["s_xe"][i],
                                 fx["s_ze"][i], fx["s_xf"][i], fx["s_zf"][i], fx["s_xent"][i],
                                 fx["s_xback"][i] if len(leg) == 2 else None, fx["s_width"][i], fx["s_fc"][i])
    return out


def oracle_pipe(fx):
    """tests/pipe_amplitude_numpy.py on every pipe case -> complex128 [n]"""
    import pipe_amplitude_numpy as PA
    import pipe_numpy as O
    lens = O.Lens()
    out = np.zeros(fx["p_ref"].size, dtype=np.complex128)
    with np.errstate(all="ignore"):
        for i in range(out.size):
            leg = LEGS[fx["p_leg"][i]]
            pipe = O.Pipe(fx["p_ro"][i], fx["p_xoff"][i], fx["p_ri"][i])
            out[i] = PA.amplitude(lens, pipe, P_MEDIA, leg, bool(fx["p_up"][i]), fx["p_xe"][i], fx["p_ze"][i], fx["p_xf"][i],
                                  fx["p_zf"][i], fx["p_alpha"][i], fx["p_beta"][i], fx["p_gamma"][i] if len(leg) == 2 else None,
                                  fx["p_width"][i], fx["p_fc"][i], a_lo=fx["p_alo"][i], a_hi=fx["p_ahi"][i])
    return out


def masks_equal(got, ref):
    """the three masks of the bar, over every entry: NaN, inf, == 0"""
    return (np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(np.isinf(got), np.isinf(ref))
            and np.array_equal(got == 0, ref == 0))


def rel_err(got, ref):
    """|got - ref| / |ref| over the finite, non-zero entries of ref (0 elsewhere)"""
    m = np.isfinite(ref) & (ref != 0)
    out = np.zeros(ref.size)
    out[m] = np.abs(got[m] - ref[m]) / np.abs(ref[m])
    return out


def class_max(cls, v, n):
    return np.array([np.max(v[cls == k], initial=0.0) for k in range(n)])


S_KEY = ("prof", "med", "leg", "up", "width", "fc")
P_KEY = ("ro", "ri", "xoff", "alo", "ahi", "leg", "up", "width", "fc")


def calls(fx, prefix, max_e=8):
    """the cases grouped into kernel calls: one call per set of call parameters and per (at most) max_e distinct elements.  A call's
    points are its cases, column j being case idx[j]; the path matrices [n_e][n_f] hold case j's path in the row of its element
    and NaN elsewhere -> [dict(key: the parameters, idx, row, xe, ze)]"""
    key = S_KEY if prefix == "s_" else P_KEY
    K = np.stack([fx[prefix + k].astype(np.float64) for k in key], axis=1)
    _, ginv = np.unique(K, axis=0, return_inverse=True)
    ginv = ginv.reshape(-1)
    out = []
    for g in range(ginv.max() + 1):
        idx = np.nonzero(ginv == g)[0]
        E = np.stack([fx[prefix + "xe"][idx], fx[prefix + "ze"][idx]], axis=1)
        U, einv = np.unique(E, axis=0, return_inverse=True)
        einv = einv.reshape(-1)
        for e0 in range(0, U.shape[0], max_e):
            m = (einv >= e0) & (einv < e0 + max_e)
            out.append(dict(key={k: fx[prefix + k][idx[0]] for k in key}, idx=idx[m], row=einv[m] - e0,
                            xe=np.ascontiguousarray(U[e0:e0 + max_e, 0]), ze=np.ascontiguousarray(U[e0:e0 + max_e, 1])))
    return out


def matrix(call, v):
    """the per-case values v[idx] spread into the call's [n_e][n_f] matrix, NaN elsewhere"""
    m = np.full((call["xe"].size, call["idx"].size), np.nan)
    m[call["row"], np.arange(call["idx"].size)] = v[call["idx"]]
    return m

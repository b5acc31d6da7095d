"""Generates tests/golden/amp_branches.npz — the ray amplitudes of include/rtus.h (rtus_leg_amp_surface, rtus_leg_amp_pipe) at 40
significant digits on the case lists of tests/amp_branch_cases.py, for tests/test_amp_branches_cpu.py (the NumPy oracles against
these values), tests/test_gpu_amp_branches.py and tests/test_gpu_pipe_amp_branches.py (the kernels against them).

Every case stores the kernel's inputs exactly as float64 and the amplitude evaluated in mpmath ON THOSE float64 INPUTS, rounded once
to complex128, with what the classes are counted by: J, D and the tangential slowness at each interface (NaN where the leg has no
such interface), also from the 40-digit evaluation; and per class E64, the fp64 NumPy oracle's largest relative error against them.

The evaluation is a restatement of the header, not of tests/amplitude_numpy.py or tests/pipe_amplitude_numpy.py:
  * the natural spline from its own tridiagonal (Thomas) solve for the knots' second derivatives, evaluated in the Hermite form
    z_k (1 - u) + z_{k+1} u + ((u^3 - u) M_{k+1} + ((1 - u)^3 - (1 - u)) M_k) dx^2 / 6; the lens curve from its quadratic
    A h^2 + B(alpha) h + C = 0 with h', h'' by implicit differentiation; the circles as written;
  * every wave's (u_n, sigma_nn, sigma_tn) from Hooke's law sigma = lambda div(u) I + mu (grad u + grad u^T) with the Lame constants
    (not the oracle's table in rho, c_T, p), and the boundary conditions as a 3 x 3 / 2 x 2 linear system solved by mpmath's LU;
  * the tube by the header's closed form with POSITIVE cosines |d . n| and the header's sign of K for the direction of travel (the
    oracles carry an oriented normal and a flipped curvature instead);
  * sinc(u) = sin(pi u) / (pi u) by mpmath's sinpi.
Rules for entries that are no ray (NaN, 0, the caustic) are the header's, decided on the 40-digit numbers.

    python tests/golden/make_amp_branches.py        (needs mpmath; about a minute)
"""
import os
import sys

import mpmath as mp
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import amp_branch_cases as B  # noqa: E402

mp.mp.dps = 40
NAN = complex(np.nan, np.nan)
CAUSTIC = complex(np.inf, np.inf)
F = lambda v: mp.mpf(float(v))                              # noqa: E731  (a float64 input, exactly)


# ---------------------------------------------------------------------------------------------- plane waves, boundary conditions
def vertical(p, c):
    """vertical slowness: real >= 0 while the wave propagates, +i |.| past its critical angle"""
    a = 1 / (c * c) - p * p
    return mp.sqrt(a) if a >= 0 else mp.mpc(0, mp.sqrt(-a))


def wave(mode, p, c, lam, mu, s):
    """(u_n, sigma_nn / (i w), sigma_tn / (i w)) of a unit wave with slowness (p, s q) in the frame (t, n), from Hooke's law"""
    st, sn = p, s * vertical(p, c)
    dt, dn = c * st, c * sn                                  # the propagation direction
    pt, pn = (dt, dn) if mode == "L" else (-dn, dt)          # polarisation: L along d, T along (-d_n, d_t)
    div = st * pt + sn * pn
    return pn, lam * div + 2 * mu * sn * pn, mu * (st * pn + sn * pt)


def _solve(cols, rhs):
    n = len(rhs)
    return mp.lu_solve(mp.matrix([[cols[j][i] for j in range(n)] for i in range(n)]), mp.matrix(rhs))


class Pair:
    """a fluid (rho1, c1) against a solid (rho2, c_l, c_t): the three displacement coefficients of the header"""

    def __init__(self, c1, rho1, cl, ct, rho2):
        self.c1, self.cl, self.ct = F(c1), F(cl), F(ct)
        self.lf = F(rho1) * self.c1 ** 2
        self.mu = F(rho2) * self.ct ** 2
        self.lam = F(rho2) * self.cl ** 2 - 2 * self.mu

    def c(self, mode):
        return self.cl if mode == "L" else self.ct

    def into_solid(self, mode, p):
        """fluid -> solid into ``mode``, the incident wave along +n (n into the solid)"""
        inc, ref = wave("L", p, self.c1, self.lf, 0, 1), wave("L", p, self.c1, self.lf, 0, -1)
        wl, wt = wave("L", p, self.cl, self.lam, self.mu, 1), wave("T", p, self.ct, self.lam, self.mu, 1)
        x = _solve([(-ref[0], -ref[1], 0), wl, wt], [inc[0], inc[1], 0])
        return x[1] if mode == "L" else x[2]

    def into_fluid(self, mode, p):
        """solid -> fluid from ``mode``, the incident wave along -n"""
        inc = wave(mode, p, self.c(mode), self.lam, self.mu, -1)
        wl, wt = wave("L", p, self.cl, self.lam, self.mu, 1), wave("T", p, self.ct, self.lam, self.mu, 1)
        tf = wave("L", p, self.c1, self.lf, 0, -1)
        return _solve([wl, wt, (-tf[0], -tf[1], 0)], [-inc[0], -inc[1], -inc[2]])[2]

    def free(self, mode_in, mode_out, p):
        """traction-free surface, the incident wave along +n (n out of the solid)"""
        inc = wave(mode_in, p, self.c(mode_in), self.lam, self.mu, 1)
        wl, wt = wave("L", p, self.cl, self.lam, self.mu, -1), wave("T", p, self.ct, self.lam, self.mu, -1)
        x = _solve([wl[1:], wt[1:]], [-inc[1], -inc[2]])
        return x[0] if mode_out == "L" else x[1]


def sinc(u):
    return mp.mpf(1) if u == 0 else mp.sinpi(u) / (mp.pi * u)


# ---------------------------------------------------------------------------------------------- the ray tube (header's closed form)
def tube(segs, ifs, trace=False):
    """segs: [(length, speed)] in the order of travel; ifs: [(ci, co, K, reflect)] between them, ci, co > 0 the incidence and exit
    cosines on the local normal, K the normal's turning rate per arc length as the travelling ray sees it -> (J, prod co / ci)
    (trace: and the widths on arrival at each segment's end)"""
    W, Th, prod, Ws = mp.mpf(0), mp.mpf(1), mp.mpf(1), []
    for k, (l, c) in enumerate(segs):
        W += l * Th
        Ws.append(W)                                         # the width on arrival at the end of segment k
        if k == len(ifs):
            break
        ci, co, K, refl = ifs[k]
        ds = W / ci
        dtin = Th - K * ds
        dtout = segs[k + 1][1] * ci / (c * co) * dtin
        W, Th = (-ds * co, K * ds - dtout) if refl else (ds * co, K * ds + dtout)
        prod *= co / ci
    return (W, prod, Ws) if trace else (W, prod)


def _unit(ax, az, bx, bz):
    dx, dz = bx - ax, bz - az
    l = mp.sqrt(dx * dx + dz * dz)
    return dx / l, dz / l, l


# ---------------------------------------------------------------------------------------------- the surface leg
class Spline:
    def __init__(self, zs):
        z = [F(v) for v in zs]
        n, h = len(z), F(B.DX)
        # natural spline: M_0 = M_{n-1} = 0, M_{k-1} + 4 M_k + M_{k+1} = 6 (z_{k-1} - 2 z_k + z_{k+1}) / h^2; Thomas
        r = [6 * (z[k - 1] - 2 * z[k] + z[k + 1]) / (h * h) for k in range(1, n - 1)]
        cp, dp = [], []
        for k, rk in enumerate(r):
            den = 4 - (cp[-1] if k else 0)
            cp.append(1 / den)
            dp.append((rk - (dp[-1] if k else 0)) / den)
        M = [mp.mpf(0)] * n
        for k in range(n - 3, -1, -1):
            M[k + 1] = dp[k] - cp[k] * M[k + 2]
        self.z, self.M, self.h, self.x0, self.n = z, M, h, F(B.X0), n

    def at(self, x):
        k = int(mp.floor((x - self.x0) / self.h))
        k = min(max(k, 0), self.n - 2)                       # (outside the extent the end segments' cubics continue)
        u = (x - (self.x0 + k * self.h)) / self.h
        v = 1 - u
        z0, z1, m0, m1, h = self.z[k], self.z[k + 1], self.M[k], self.M[k + 1], self.h
        s = z0 * v + z1 * u + ((u ** 3 - u) * m1 + (v ** 3 - v) * m0) * h * h / 6
        s1 = (z1 - z0) / h + ((3 * u * u - 1) * m1 - (3 * v * v - 1) * m0) * h / 6
        s2 = u * m1 + v * m0
        return s, s1, s2


_splines = {}


def surface_amplitude(zs_key, zs, med, leg, up, width, fc, xe, ze, xf, zf, xent, xback):
    """-> (A complex128, J, D, p_surface, p_backwall) of one entry (floats; NaN where undefined)"""
    skip = len(leg) == 2
    if np.isnan(xent) or (skip and np.isnan(xback)):
        return NAN, np.nan, np.nan, np.nan, np.nan
    if np.isinf(xent) or (skip and np.isinf(xback)):         # no such point on the surface / the backwall: no ray
        return 0j, np.nan, np.nan, np.nan, np.nan
    if zs_key not in _splines:
        _splines[zs_key] = Spline(zs)
    pair = Pair(*med)
    zb = F(B.ZB)
    X, Y = leg[0], leg[-1]
    x = F(xent)
    s, s1, s2 = _splines[zs_key].at(x)
    N = mp.sqrt(1 + s1 * s1)
    nx, nz = -s1 / N, 1 / N
    tx, tz = nz, -nx
    kap = s2 / N ** 3
    e = _unit(F(xe), F(ze), x, s)                            # E -> S
    if skip:
        b = _unit(x, s, F(xback), zb)                        # S -> B
        f = _unit(F(xback), zb, F(xf), F(zf))                # B -> F
    else:
        b = _unit(x, s, F(xf), F(zf))                        # S -> F
    ce, cb = e[0] * nx + e[1] * nz, b[0] * nx + b[1] * nz
    if not (ce > 0 and cb > 0):
        return 0j, np.nan, np.nan, float((e[0] * tx + e[1] * tz) / pair.c1), np.nan
    D = sinc(F(width) * e[0] * F(fc) / pair.c1) if width > 0 else mp.mpf(1)
    pb = mp.nan
    if not up:
        ps = (e[0] * tx + e[1] * tz) / pair.c1
        C = pair.into_solid(X, ps)
        segs, ifs = [(e[2], pair.c1), (b[2], pair.c(X))], [(ce, cb, -kap, False)]
        if skip:
            pb = b[0] / pair.c(X)
            C *= pair.free(X, Y, pb)
            segs.append((f[2], pair.c(Y)))
            ifs.append((abs(b[1]), abs(f[1]), 0, True))
    else:
        segs, ifs, C = [], [], mp.mpf(1)
        if skip:
            pb = -f[0] / pair.c(Y)
            C *= pair.free(Y, X, pb)
            segs.append((f[2], pair.c(Y)))
            ifs.append((abs(f[1]), abs(b[1]), 0, True))
        ps = -(b[0] * tx + b[1] * tz) / pair.c(X)
        C *= pair.into_fluid(X, ps)
        segs += [(b[2], pair.c(X)), (e[2], pair.c1)]
        ifs.append((cb, ce, kap, False))
    J, prod = tube(segs, ifs)
    if J == 0:
        return CAUSTIC, 0.0, float(D), float(ps), float(pb)
    A = mp.conj(D * C * mp.sqrt(prod / abs(J)))
    return complex(A), float(J), float(D), float(ps), float(pb)


def surface_table():
    L, zs = B.surface_cases()
    out = L.arrays("s_")
    n = len(L.rows)
    ref, J, D, ps, pb = np.zeros(n, np.complex128), np.zeros(n), np.zeros(n), np.zeros(n), np.zeros(n)
    for i, r in enumerate(L.rows):
        ref[i], J[i], D[i], ps[i], pb[i] = surface_amplitude(r["prof"], zs[r["prof"]], B.MEDIA[r["med"]], B.LEGS[r["leg"]], bool(r["up"]),
                                                             r["width"], r["fc"], r["xe"], r["ze"], r["xf"], r["zf"], r["xent"], r["xback"])
    out.update(s_ref=ref, s_J=J, s_D=D, s_ps=ps, s_pb=pb)
    return out


# ---------------------------------------------------------------------------------------------- the pipe leg
class LensCurve:
    """P(alpha) = h(alpha) (sin alpha, cos alpha), h the root -(B + sqrt(B^2 - 4 A C)) / (2 A) of A h^2 + B(alpha) h + C = 0 with
    A = c1^2 / c2^2 - 1, B = phi_2 + phi_3 cos(alpha), C = c1^2 T^2 - d^2, T = l0 / c1 + h0 / c2, phi_2 = -2 T c1^2 / c2, phi_3 = 2 d"""

    def __init__(self, c1, c2, l0, h0, d):
        c1, c2, l0, h0, d = F(c1), F(c2), F(l0), F(h0), F(d)
        T = l0 / c1 + h0 / c2
        self.A, self.C = c1 * c1 / (c2 * c2) - 1, c1 * c1 * T * T - d * d
        self.phi_2, self.phi_3 = -2 * T * c1 * c1 / c2, 2 * d

    def at(self, a):
        """P, P', P'': h' and h'' by differentiating the quadratic, not its root"""
        s, c = mp.sin(a), mp.cos(a)
        Bq, B1, B2 = self.phi_2 + self.phi_3 * c, -self.phi_3 * s, -self.phi_3 * c
        h = -(Bq + mp.sqrt(Bq * Bq - 4 * self.A * self.C)) / (2 * self.A)
        den = 2 * self.A * h + Bq
        h1 = -B1 * h / den
        h2 = -(B2 * h + 2 * B1 * h1 + 2 * self.A * h1 * h1) / den
        return ((h * s, h * c), (h1 * s + h * c, h1 * c - h * s), (h2 * s + 2 * h1 * c - h * s, h2 * c - 2 * h1 * s - h * c))


def pipe_amplitude(lens, ro, ri, xoff, alo, ahi, media, leg, up, width, fc, xe, ze, xf, zf, alpha, beta, gamma):
    """-> (A complex128, J, D, p_lens, p_outer, p_bore, W on arrival at the outer circle) of one entry"""
    none = (np.nan,) * 6
    skip = len(leg) == 2
    if np.isnan(alpha) or np.isnan(beta) or (skip and np.isnan(gamma)):
        return (NAN,) + none
    if alpha == alo or alpha == ahi:                         # a pinned lens leg refracts by no law
        return (0j,) + none
    rl, ctl, rw, r2, cl, ct = media
    lp, wp = Pair(lens[1], rw, lens[0], ctl, rl), Pair(lens[1], rw, cl, ct, r2)     # water | lens, water | wall
    X, Y = leg[0], leg[-1]
    P, P1, P2 = LensCurve(*lens).at(F(alpha))
    n1 = mp.sqrt(P1[0] ** 2 + P1[1] ** 2)
    tau = (P1[0] / n1, P1[1] / n1)
    nl = (tau[1], -tau[0])                                   # towards the water
    Kl = (P1[0] * P2[1] - P1[1] * P2[0]) / n1 ** 3
    ro_, ri_, x0 = F(ro), F(ri), F(xoff)
    nq = (mp.sin(F(beta)), mp.cos(F(beta)))
    Q = (x0 + ro_ * nq[0], ro_ * nq[1])
    pts = [(F(xe), F(ze)), P, Q]
    if skip:
        nr = (mp.sin(F(gamma)), mp.cos(F(gamma)))
        pts.append((x0 + ri_ * nr[0], ri_ * nr[1]))
    pts.append((F(xf), F(zf)))
    e = [_unit(a[0], a[1], b[0], b[1]) for a, b in zip(pts[:-1], pts[1:])]
    dot = lambda u, n: u[0] * n[0] + u[1] * n[1]             # noqa: E731
    ray = dot(e[0], nl) > 0 and dot(e[1], nl) > 0 and dot(e[1], nq) < 0 and dot(e[2], nq) < 0
    if skip:
        ray = ray and dot(e[2], nr) < 0 and dot(e[3], nr) > 0
    if not ray:
        return (0j,) + none
    D = sinc(F(width) * e[0][0] * F(fc) / lp.cl) if width > 0 else mp.mpf(1)
    tq = (-nq[1], nq[0])                                     # the tangent of the frame n = -(Q - Cp) / r_outer
    cs = [lp.cl, lp.c1, wp.c(X)] + ([wp.c(Y)] if skip else [])
    segs = [(u[2], c) for u, c in zip(e, cs)]
    # the tube's interfaces in the down order: cosines on the local normal, K as a ray going DOWN sees it (the lens normal already
    # points along it; the circles' outward normals point against it: K flips)
    ifs = [(dot(e[0], nl), dot(e[1], nl), Kl, False), (-dot(e[1], nq), -dot(e[2], nq), -1 / ro_, False)]
    if skip:
        tb = (-nr[1], nr[0])
        ifs.append((-dot(e[2], nr), dot(e[3], nr), -1 / ri_, True))
    pb = mp.nan
    if not up:
        pl, pq = dot(e[0], tau) / lp.cl, dot(e[1], tq) / lp.c1
        C = lp.into_fluid("L", pl) * wp.into_solid(X, pq)
        if skip:
            pb = dot(e[2], tb) / wp.c(X)
            C *= wp.free(X, Y, pb)
    else:
        # the same path walked from F: cosines swap, every normal is met from its other side (K changes sign, except at the
        # reflection, where the ray is on the same side of the bore both ways)
        segs = segs[::-1]
        ifs = [(co, ci, K if refl else -K, refl) for ci, co, K, refl in ifs[::-1]]
        C = mp.mpf(1)
        if skip:
            pb = -dot(e[3], tb) / wp.c(Y)
            C *= wp.free(Y, X, pb)
        pq, pl = -dot(e[2], tq) / wp.c(X), -dot(e[1], tau) / lp.c1
        C *= wp.into_fluid(X, pq) * lp.into_solid("L", pl)
    J, prod, Ws = tube(segs, ifs, trace=True)
    Wq = Ws[1] if not up else Ws[-3]                          # on arrival at the outer circle
    if J == 0:
        return CAUSTIC, 0.0, float(D), float(pl), float(pq), float(pb), float(Wq)
    A = mp.conj(D * C * mp.sqrt(prod / abs(J)))
    return complex(A), float(J), float(D), float(pl), float(pq), float(pb), float(Wq)


def pipe_table():
    import pipe_numpy as O
    L = B.pipe_cases()
    out = L.arrays("p_")
    lens = (O.C1, O.C2, O.L0, O.H0, O.D)
    n = len(L.rows)
    ref = np.zeros(n, np.complex128)
    cols = np.zeros((6, n))
    for i, r in enumerate(L.rows):
        v = pipe_amplitude(lens, r["ro"], r["ri"], r["xoff"], r["alo"], r["ahi"], B.P_MEDIA, B.LEGS[r["leg"]], bool(r["up"]), r["width"],
                           r["fc"], r["xe"], r["ze"], r["xf"], r["zf"], r["alpha"], r["beta"], r["gamma"])
        ref[i], cols[:, i] = v[0], v[1:]
    out.update(p_ref=ref, p_J=cols[0], p_D=cols[1], p_pl=cols[2], p_pq=cols[3], p_pb=cols[4], p_Wq=cols[5],
               p_lens=np.array(lens), p_media=np.array(B.P_MEDIA))
    return out


def main():
    out = surface_table()
    out.update(pipe_table())
    # E64: the largest relative error of the fp64 NumPy oracle against the 40-digit value, per class (the GPU tests' bar is built on it)
    for pre, oracle in (("s_", B.oracle_surface), ("p_", B.oracle_pipe)):
        out[pre + "E64"] = B.class_max(out[pre + "cls"], B.rel_err(oracle(out), out[pre + "ref"]), out[pre + "classes"].size)
    np.savez_compressed(B.FIXTURE, **out)
    print(B.FIXTURE, os.path.getsize(B.FIXTURE), "bytes;", out["s_ref"].size, "surface cases,", out["p_ref"].size, "pipe cases")


if __name__ == "__main__":
    main()

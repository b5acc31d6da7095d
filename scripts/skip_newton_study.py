"""How many fp32 Newton steps the skip-leg scan of rtus_surface_kernel (SURF_SKIP) needs.

A NumPy restatement of the kernel's fp32 scan: per focal point, u = c_down p is warm-started from the previous scan point (the
straight line to the mirrored point at the first one) and takes N safeguarded Newton steps per scan point; the sign of T' at
every (element, scan point) is then compared with the fp64 sign (tests/skip_numpy.py's inner solve).  A wrong sign only matters
where it is not within one scan point of a root of T': surf_refine re-checks the bracket's ends in fp64 and moves one interval
left or right, so errors next to a root are recovered and others can lose or fake a bracket.

    python scripts/skip_newton_study.py [--steps 1 2 3] [--n-f 400]

Prints, per step count and mode pair, the sign errors and how many lie farther than one scan point from every root.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import skip_numpy as K          # noqa: E402
import surface_numpy as S       # noqa: E402

f32 = np.float32


def scan_fp32(P, xf, zf, zb, c_down, c_up, steps):
    """the kernel's lane term in fp32 -> g2 [n_f, m] (T' c_down = g2 - ng)"""
    kap = c_down / c_up
    kap2 = f32(kap * kap)
    umax = f32(f32(min(1.0, kap)) * f32(1.0 - 1e-6))
    xfr, h2 = f32(xf), f32(zb) - f32(zf)
    u = None
    g2 = np.empty((xf.size, P.shape[0]), dtype=np.float32)
    with np.errstate(all="ignore"):
        for j in range(P.shape[0]):
            px, py, ps = P[j]
            h1, X = f32(zb) - py, xfr - px
            if u is None:
                h = h1 + h2
                u = umax * X / np.sqrt(X * X + h * h)
            for _ in range(steps):
                rd, ru = f32(1) / np.sqrt(f32(1) - u * u), f32(1) / np.sqrt(kap2 - u * u)
                fv = u * (h1 * rd + h2 * ru) - X
                fu = h1 * rd * rd * rd + h2 * kap2 * ru * ru * ru
                un = u - fv / fu
                u = np.where(np.abs(un) < umax, un, f32(0.5) * (u + np.where(fv < 0, umax, -umax))).astype(np.float32)
            ad = np.sqrt(f32(1) - u * u)
            g2[:, j] = -(ad * ps + u)
    return g2


def study(steps, n_f, seed=3):
    X0, DX, NS = -0.02, 1e-3, 41
    x = X0 + DX * np.arange(NS)
    zs = 0.02 + 0.0015 * np.sin(2 * np.pi * x / 0.010)
    zb = 0.045
    coef = S.spline(X0, DX, zs)
    m = 4 * (NS - 1) + 1
    xp = X0 + DX * np.arange(m) / 4
    s, s1, _ = S.spline_eval(coef, X0, DX, xp)
    P = np.stack([xp, s, s1], axis=1).astype(np.float32)
    rng = np.random.default_rng(seed)
    xf, zf = rng.uniform(-0.019, 0.019, n_f), rng.uniform(0.024, 0.044, n_f)
    xe, ze = np.linspace(-0.012, 0.012, 8), np.zeros(8)
    c1, cl, ct = 1480.0, 5900.0, 3230.0
    for name, cd, cu in (("LL", cl, cl), ("LT", cl, ct), ("TL", ct, cl), ("TT", ct, ct)):
        g2 = scan_fp32(P, xf, zf, zb, cd, cu, steps)
        d64 = K.inner_leg(coef, X0, DX, xp[None, :], xf[:, None], zf[:, None], zb, cd, cu)[1] * cd        # fp64 T_in' c_down
        n_err = n_far = 0
        for e in range(xe.size):
            ux, uz = P[:, 0] - f32(xe[e]), P[:, 1] - f32(ze[e])
            ng = -((ux + uz * P[:, 2]) / np.sqrt(ux * ux + uz * uz)) * f32(cd / c1)       # the LDS term, fp32
            pos32 = g2 > ng[None, :]
            d = S._legs(coef, X0, DX, xp, xe[e], ze[e], c1)[1][None, :] * cd + d64          # T' c_down in fp64
            pos64 = d > 0
            err = pos32 != pos64
            # a root of T' between scan points j and j+1: sign change of the fp64 values
            ch = np.zeros_like(pos64)
            ch[:, :-1] |= pos64[:, :-1] != pos64[:, 1:]
            ch[:, 1:] |= pos64[:, :-1] != pos64[:, 1:]
            near = ch.copy()                                   # within one scan point of a root
            near[:, 1:] |= ch[:, :-1]
            near[:, :-1] |= ch[:, 1:]
            n_err += int(err.sum())
            n_far += int((err & ~near).sum())
        print(f"steps={steps} {name}: {n_f * xe.size * m} signs, {n_err} wrong, {n_far} farther than one scan point from a root")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, nargs="+", default=[1, 2, 3])
    ap.add_argument("--n-f", type=int, default=400)
    a = ap.parse_args()
    for k in a.steps:
        study(k, a.n_f)

"""CPU emulation of the planar kernel's row table (DESIGN.md section 4 "Row table"): image-grid rows served from a verified
quintic Hermite table of T(X), X = |xf - xe|, instead of one root-find per (element, target).

Emulated as the kernel does it, in fp64: the lattice X_j = j h anchored at 0 with h a power of two chosen from zf - ze alone,
nodes (T, p, p') from fp64 Newton on X(q) = X_j down to a residual of 1e-13 X, the six coefficients of each interval, the
off-centre check of every interval at s = 0.3 against a solved point, and the Horner evaluation.  Compared with the long-double
oracle (oracle/cport.tt_layers) on the media of BASELINE configs[1], [2], [4] and of tests/test_gpu_irregular_apertures.py.

    python scripts/study_planar_rowtable.py [divisor ...]      (default divisors: 64 128 192)

Prints per medium, depth and divisor: h, intervals needed for a 40 mm span, worst relative error of served solves against the
oracle, worst relative check value at s = 0.3, and how many intervals the 1e-11 check rejects.  Settles the divisor, the
capacity and the check bound used in csrc/rtus_fermat.hip."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import cport  # noqa: E402

SQRT2 = 1.4142135623730951
CHECK_S, CHECK_BOUND, RESID = 0.3, 1e-11, 1e-13


def lattice_h(D, div):
    """the power of two nearest (in ratio) to D / div: the exponent of D sqrt(2) / div, mantissa cleared"""
    m, e = np.frexp(D * (SQRT2 / div))          # value = m 2^e, m in [0.5, 1)
    return float(np.ldexp(1.0, e - 1))


def layer_tables(z_if, c, ze, zf):
    z_if, c = np.asarray(z_if, float), np.asarray(c, float)
    top = np.maximum(np.concatenate([[ze], z_if]), ze)
    bot = np.minimum(np.concatenate([z_if, [np.inf]]), zf)
    h = np.maximum(bot - top, 0.0)
    cm = c[h > 0].max()
    r = c / cm
    k = np.where(c == cm, 0.0, np.maximum(1.0 - r * r, 0.0))
    r = np.where(c == cm, 1.0, r)
    return h * r, k, h / c, cm


def solve_nodes(X, hr, k, hc, cm):
    """(T, p, p') at reach X: Newton on X(q) = X from a lower bound of the root (monotone: X(q) is concave), fp64"""
    X = np.asarray(X, float)
    lin = k == 0.0
    lb = np.maximum(X / hr.sum(), (X - (hr[~lin] / np.sqrt(k[~lin])).sum()) / hr[lin].sum())
    q = np.maximum(lb, 0.0)
    ok = np.zeros(X.shape, bool)
    for _ in range(60):
        w = 1.0 / np.sqrt(1.0 + k[:, None] * q * q)
        S1 = (hr[:, None] * w).sum(0)
        S3 = (hr[:, None] * w ** 3).sum(0)
        dX = X - q * S1
        ok = np.abs(dX) <= RESID * X
        if ok.all():
            break
        q = np.where(ok, q, q + dX / S3)
    w = 1.0 / np.sqrt(1.0 + k[:, None] * q * q)
    S1 = (hr[:, None] * w).sum(0)
    S3 = (hr[:, None] * w ** 3).sum(0)
    u = 1.0 / np.sqrt(1.0 + q * q)
    p = q * u / cm
    T = (1.0 + q * q) * u * (hc[:, None] * w).sum(0) + p * (X - q * S1)
    return T, p, u ** 3 / (cm * S3), ok


def coefficients(T, p, pp, h):
    c0, c1, c2 = T[:-1], h * p[:-1], 0.5 * h * h * pp[:-1]
    d = ((T[1:] - c0) - c1) - c2
    e = (h * p[1:] - c1) - 2.0 * c2
    f = h * h * pp[1:] - 2.0 * c2
    return np.stack([c0, c1, c2, 10.0 * d - 4.0 * e + 0.5 * f, -15.0 * d + 7.0 * e - f, 6.0 * d - 3.0 * e + 0.5 * f])


def horner(C, s):
    return C[0] + s * (C[1] + s * (C[2] + s * (C[3] + s * (C[4] + s * C[5]))))


def study(name, z_if, c, depths, div, xmax=0.06, n_probe=6000):
    rng = np.random.default_rng(3)
    worst = 0.0
    for zf in depths:
        h = lattice_h(zf, div)
        hr, k, hc, cm = layer_tables(z_if, c, 0.0, zf)
        n_int = int(np.floor(xmax / h)) + 1
        T, p, pp, ok = solve_nodes(np.arange(n_int + 1) * h, hr, k, hc, cm)
        C = coefficients(T, p, pp, h)
        Tc, _, _, okc = solve_nodes((np.arange(n_int) + CHECK_S) * h, hr, k, hc, cm)
        chk = np.abs(horner(C, CHECK_S) - Tc) / Tc
        bad = (chk > CHECK_BOUND) | ~ok[:-1] | ~ok[1:] | ~okc
        X = np.sort(rng.uniform(0.0, xmax, n_probe))
        X[:8] = [0.0, h * 1e-9, h * 0.5, h, h * (1 - 2 ** -52), xmax * 0.999, h * 7.3, h * 2]
        t = X / h
        j = np.floor(t).astype(int)
        got = horner(C[:, j], t - j)
        ref = cport.tt_layers(z_if, c, np.zeros(1), np.zeros(1), X, np.full(X.size, zf))[0]
        err = np.abs(got - ref) / ref
        served = ~bad[j]
        e = float(err[served].max()) if served.any() else 0.0
        worst = max(worst, e)
        print(f"{name:10s} div {div:4d} zf {zf*1e3:7.3f} mm  h 2^{int(np.log2(h)):d} = {h*1e3:.4f} mm  40 mm span = {int(0.04/h)+2:4d} intervals  "
              f"served err {e:.2e}  check max {chk.max():.2e}  rejected {int(bad.sum())}/{n_int}", flush=True)
    return worst


def main():
    divs = [int(a) for a in sys.argv[1:]] or [64, 128, 192]
    media = [
        ("configs[1]", [0.020], [2330.0, 1483.0], [0.0201, 0.021, 0.025, 0.035, 0.065], 0.06),
        ("configs[2]", [0.010, 0.025], [2330.0, 1483.0, 5900.0], [0.026, 0.0268, 0.030, 0.045, 0.066], 0.06),
        ("configs[4]", [0.008, 0.020, 0.050, 0.062], [2330.0, 1483.0, 5900.0, 1483.0, 2330.0], [0.070], 0.62),
        ("irregular", [0.010, 0.025], [1483.0, 5900.0, 2330.0], [0.0251, 0.026, 0.030, 0.045, 0.065], 0.06),
        ("one layer", [], [1483.0], [0.001, 0.03], 0.06),
    ]
    # harder than any configuration: 0.1 mm of the fast layer under the interface.  The check sits at s = 0.3, where the quintic's
    # error s^3 (1 - s)^3 is 0.59 of its maximum at the centre: an interval that passes at 1e-11 is within 1.7e-11 everywhere
    stress = [("thin steel", [0.010, 0.025], [2330.0, 1483.0, 5900.0], [0.02501, 0.0251, 0.0253], 0.06)]
    for div in divs:
        worst = 0.0
        for name, z_if, c, depths, xmax in media:
            worst = max(worst, study(name, z_if, c, depths, div, xmax))
        print(f"== divisor {div}: worst served error against the oracle {worst:.2e} (must stay below {CHECK_BOUND:g})", flush=True)
        assert worst < CHECK_BOUND
        ws = max(study(name, z_if, c, depths, div, xmax) for name, z_if, c, depths, xmax in stress)
        print(f"== divisor {div}: stress rows, worst served error {ws:.2e} (bound of a checked interval: 1.7e-11 + node error)", flush=True)
        assert ws < 2e-11


if __name__ == "__main__":
    main()

"""CPU: the oracle of the curved-interface solver (tests/surface_numpy.py) against mpmath at 40 digits and against the flat
closed form; argument validation of rtus_tt_surface* through ctypes (status codes, no GPU touched)."""
import ctypes as C

import mpmath as mp
import numpy as np
import pytest

import surface_numpy as S

C1, C2 = 1480.0, 5900.0
X0, DX, NS = -0.02, 1e-3, 41


def _wavy():
    x = X0 + DX * np.arange(NS)
    return 0.02 + 0.0015 * np.sin(2 * np.pi * x / 0.010)


def _mp_spline(x0, dx, zs):
    """natural spline in mpmath (own tridiagonal solve) -> s(x), s'(x)"""
    z = [mp.mpf(float(v)) for v in zs]
    x0, dx = mp.mpf(x0), mp.mpf(dx)
    n = len(z)
    rhs = [6 * (z[i + 1] - 2 * z[i] + z[i - 1]) / dx ** 2 for i in range(1, n - 1)]
    cp, dp = [mp.mpf(0)] * (n - 2), [mp.mpf(0)] * (n - 2)
    for i in range(n - 2):
        w = 4 - (cp[i - 1] if i else 0)
        cp[i] = 1 / w
        dp[i] = (rhs[i] - (dp[i - 1] if i else 0)) / w
    M = [mp.mpf(0)] * n
    for i in range(n - 3, -1, -1):
        M[i + 1] = dp[i] - cp[i] * (M[i + 2] if i + 2 < n - 1 else 0)

    def seg(x):
        k = int(mp.floor((x - x0) / dx))
        k = min(max(k, 0), n - 2)
        t = x - (x0 + k * dx)
        b = (z[k + 1] - z[k]) / dx - dx * (2 * M[k] + M[k + 1]) / 6
        c, d = M[k] / 2, (M[k + 1] - M[k]) / (6 * dx)
        return z[k] + t * (b + t * (c + t * d)), b + t * (2 * c + 3 * t * d)
    return seg


def _mp_least_minimum(zs, xe, ze, xf, zf, seeds):
    seg = _mp_spline(X0, DX, zs)
    xe, ze, xf, zf = (mp.mpf(float(v)) for v in (xe, ze, xf, zf))

    def T(x):
        s, _ = seg(x)
        return mp.sqrt((x - xe) ** 2 + (s - ze) ** 2) / C1 + mp.sqrt((x - xf) ** 2 + (s - zf) ** 2) / C2

    def dT(x):
        s, s1 = seg(x)
        return (((x - xe) + (s - ze) * s1) / mp.sqrt((x - xe) ** 2 + (s - ze) ** 2) / C1
                + ((x - xf) + (s - zf) * s1) / mp.sqrt((x - xf) ** 2 + (s - zf) ** 2) / C2)
    best = None
    for x in seeds:
        h = mp.mpf(DX) / 64
        r = mp.findroot(dT, (mp.mpf(x) - h, mp.mpf(x) + h), solver="anderson")
        t = T(r)
        best = t if best is None or t < best else best
    return best


def test_oracle_against_mpmath_including_two_minima():
    mp.mp.dps = 40
    zs = _wavy()
    cases = [(0.0, 0.0, 0.001, 0.03), (-0.008, 0.0, 0.004, 0.028), (0.01, 0.0, -0.006, 0.035), (0.003, 0.002, 0.0125, 0.024)]
    multi = 0
    for xe, ze, xf, zf in cases:
        m = S.minima(X0, DX, zs, C1, C2, xe, ze, xf, zf)
        assert m, "each case has a path"
        multi += len(m) >= 2
        t_or = S.table(X0, DX, zs, C1, C2, [xe], [ze], [xf], [zf])["t"][0, 0]
        t_mp = _mp_least_minimum(zs, xe, ze, xf, zf, [x for x, _ in m])
        assert abs(float(t_mp - mp.mpf(float(t_or)))) <= 1e-18, (xe, ze, xf, zf, t_or, t_mp)
    assert multi >= 1, "at least one case with two or more competing minima"


def test_flat_profile_equals_the_closed_form():
    """one flat interface: Snell in the ray parameter p, X(p) = h1 tan(th1) + h2 tan(th2) = |xf - xe|, solved at 40 digits"""
    mp.mp.dps = 40
    z0 = 0.02
    zs = np.full(NS, z0)
    rng = np.random.default_rng(3)
    xe, ze = rng.uniform(-0.01, 0.01, 4), rng.uniform(-0.005, 0.01, 4)
    xf, zf = rng.uniform(-0.01, 0.01, 5), rng.uniform(0.025, 0.06, 5)
    got = S.table(X0, DX, zs, C1, C2, xe, ze, xf, zf)["t"]
    for i in range(xe.size):
        for j in range(xf.size):
            h1, h2, X = mp.mpf(z0) - mp.mpf(float(ze[i])), mp.mpf(float(zf[j])) - mp.mpf(z0), abs(mp.mpf(float(xf[j])) - mp.mpf(float(xe[i])))
            pmax = 1 / mp.mpf(C2)

            def reach(p):
                return h1 * p * C1 / mp.sqrt(1 - (p * C1) ** 2) + h2 * p * C2 / mp.sqrt(1 - (p * C2) ** 2) - X
            p = mp.findroot(reach, (mp.mpf(0), pmax * (1 - mp.mpf(10) ** -30)), solver="bisect") if X > 0 else mp.mpf(0)
            t = h1 / (C1 * mp.sqrt(1 - (p * C1) ** 2)) + h2 / (C2 * mp.sqrt(1 - (p * C2) ** 2))
            assert abs(float(t - mp.mpf(float(got[i, j])))) <= 1e-18


def test_oracle_validity_rules():
    zs = _wavy()
    r = S.table(X0, DX, zs, C1, C2, [0.0, 0.0], [0.0, 0.019], [0.0, 0.03, 0.0], [0.03, 0.03, 0.01])
    assert np.isnan(r["t"][1]).all(), "an element not above the whole profile has a NaN row"
    assert np.isnan(r["t"][0, 1]), "a focal point outside the extent is NaN"
    assert np.isnan(r["t"][0, 2]), "a focal point above the surface is NaN"
    assert np.isfinite(r["t"][0, 0])


def test_chunked_oracle_equals_the_whole_table():
    """table_chunked / count_minima (the GPU suite's memory-bounded forms) are table / stationary over slices of the focal points"""
    zs = _wavy()
    xe, ze = np.linspace(-0.01, 0.01, 3), np.zeros(3)
    rng = np.random.default_rng(3)
    xf, zf = rng.uniform(-0.018, 0.018, 70), rng.uniform(0.015, 0.04, 70)
    whole = S.table(X0, DX, zs, C1, C2, xe, ze, xf, zf)
    parts = S.table_chunked(X0, DX, zs, C1, C2, xe, ze, xf, zf, chunk=16)
    for k in whole:
        assert np.array_equal(whole[k], parts[k], equal_nan=True), k
    ent, _, kind, _ = S.stationary(X0, DX, zs, C1, C2, xe, ze, xf, zf)
    n = np.bincount(ent[kind == 1], minlength=xe.size * xf.size).reshape(xe.size, xf.size)
    assert np.array_equal(S.count_minima(X0, DX, zs, C1, C2, xe, ze, xf, zf, chunk=16), n)
    assert n.max() >= 2


def test_invalid_arguments_are_status_codes(rtus):
    """argument checks return -1 / -4 before any HIP call (no GPU here)"""
    L = rtus.lib()
    zs = np.full(8, 0.02)
    a = np.zeros(4)
    p, z = a.ctypes.data, zs.ctypes.data
    ws = np.zeros(L.rtus_tt_surface_workspace_bytes(8) + 512, dtype=np.uint8)
    wp = (ws.ctypes.data + 255) // 256 * 256
    nb = L.rtus_tt_surface_workspace_bytes(8)
    assert nb > 0 and L.rtus_tt_surface_workspace_bytes(3) == 0

    def dev(x0=0.0, dx=1e-3, zsp=z, n_s=8, c1=C1, c2=C2, xe=p, n_e=1, n_f=1, tt=p, w=wp, nbytes=nb):
        return L.rtus_tt_surface_dev(x0, dx, zsp, n_s, c1, c2, xe, p, n_e, p, p, n_f, tt, None, w, nbytes, None)

    assert dev(n_s=3) == -1
    assert dev(dx=0.0) == -1 and dev(dx=-1e-3) == -1 and dev(dx=float("nan")) == -1 and dev(dx=float("inf")) == -1
    assert dev(x0=float("nan")) == -1
    assert dev(c1=0.0) == -1 and dev(c2=-1.0) == -1 and dev(c2=float("nan")) == -1
    assert dev(zsp=None) == -1 and dev(xe=None) == -1 and dev(tt=None) == -1
    assert dev(n_e=0) == -1 and dev(n_f=-1) == -1
    assert dev(w=None) == -4
    assert dev(w=wp + 8) == -4                                   # misaligned
    assert dev(nbytes=nb - 1) == -4                              # short
    host = L.rtus_tt_surface
    assert host(0.0, 1e-3, z, 3, C1, C2, p, p, 1, p, p, 1, p, None, 0) == -1
    assert host(0.0, 0.0, z, 8, C1, C2, p, p, 1, p, p, 1, p, None, 0) == -1
    assert host(0.0, 1e-3, z, 8, C1, 0.0, p, p, 1, p, p, 1, p, None, 0) == -1
    assert host(0.0, 1e-3, z, 8, C1, C2, p, p, 1, p, p, 1, None, None, 0) == -1


def test_python_wrapper_validation(rtus):
    with pytest.raises(ValueError):
        rtus.travel_time_surface(0.0, 1e-3, np.zeros(8), C1, C2, [0.0, 1.0], [0.0], [0.0], [0.03])
    with pytest.raises(ValueError):
        rtus.travel_time_surface(0.0, 1e-3, np.zeros(8), C1, C2, [0.0], [0.0], [0.0], [0.03], out=np.zeros((2, 1)))
    with pytest.raises(rtus.RtusError):
        rtus.travel_time_surface(0.0, 1e-3, np.zeros(3), C1, C2, [0.0], [0.0], [0.0], [0.03])

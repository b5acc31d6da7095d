"""CPU: the host side of the anisotropic travel times (Christoffel group slowness, the series fit, the elliptical model), the
NumPy oracle (tests/aniso_numpy.py) against finite differences and against the isotropic oracle, and the argument checks of
rtus_tt_aniso_* through ctypes and the wrappers (status codes before any HIP call: no GPU touched)."""
import numpy as np
import pytest

import aniso_numpy as A
import surface_numpy as S

C1 = 1480.0
X0, DX, NS = -0.02, 1e-3, 41
WELD = dict(C11=263e9, C13=145e9, C33=216e9, C55=129e9, rho=7900.0)       # representative austenitic weld metal


def _wavy(amp=0.0015, lam=0.010, z0=0.02):
    x = X0 + DX * np.arange(NS)
    return z0 + amp * np.sin(2 * np.pi * x / lam)


def test_isotropic_constants_give_a_constant_slowness(rtus):
    lam, mu, rho = 110e9, 80e9, 7800.0
    for mode, c in (("qP", np.sqrt((lam + 2 * mu) / rho)), ("qSV", np.sqrt(mu / rho)), ("SH", np.sqrt(mu / rho))):
        psi, s = rtus.group_slowness_ti(lam + 2 * mu, lam, lam + 2 * mu, mu, rho, mode, C66=mu, n=512)
        assert np.max(np.abs(s * c - 1)) <= 1e-14, mode
        assert np.max(np.abs(psi - np.pi * np.arange(512) / 512)) <= 1e-14, mode
        a, b, res = rtus.fit_group_slowness(psi, s, 4)
        assert abs(a[0] * c - 1) <= 1e-14 and np.max(np.abs(a[1:])) <= 1e-14 / c and np.max(np.abs(b)) <= 1e-14 / c and res <= 1e-14


def test_weld_metal_qp_fit_residual_falls_with_k(rtus):
    psi, s = rtus.group_slowness_ti(**WELD, mode="qP")
    assert 5200 < 1 / s.max() < 5260 and 6360 < 1 / s.min() < 6420          # the group velocity's range: ~20 %
    res = [rtus.fit_group_slowness(psi, s, K)[2] for K in (2, 4, 8, 12, 16)]
    print("relative misfit at K = 2, 4, 8, 12, 16:", res)
    assert all(hi > 2 * lo for hi, lo in zip(res, res[1:]))
    assert res[0] < 3e-2 and res[-1] < 2e-5
    a, b, _ = rtus.fit_group_slowness(psi, s, 16)
    assert a.shape == b.shape == (17,) and b[0] == 0.0
    assert np.max(np.abs(b)) <= 1e-9 * a[0], "the untilted medium is symmetric about its axis"
    u = np.linspace(0, np.pi, 999)
    assert np.max(np.abs(rtus.eval_group_slowness(a, b, u) / np.interp(u, psi, s, period=np.pi) - 1)) < 2e-5


def test_tilt_is_a_rotation(rtus):
    psi, s = rtus.group_slowness_ti(**WELD, mode="qP")
    a0, b0, r0 = rtus.fit_group_slowness(psi, s, 12)
    u = np.linspace(-2.0, 2.0, 777)
    for tilt in (np.deg2rad(25), np.deg2rad(-40), 1.3):
        a, b, r = rtus.fit_group_slowness(psi, s, 12, tilt=tilt)
        assert r == r0
        assert np.max(np.abs(rtus.eval_group_slowness(a, b, u) - rtus.eval_group_slowness(a0, b0, u - tilt))) <= 1e-15 * a0[0] * 20
        assert np.allclose(a ** 2 + b ** 2, a0 ** 2 + b0 ** 2, rtol=1e-12, atol=0)       # each harmonic keeps its amplitude
    a, b = rtus.elliptical_slowness(6100.0, 5300.0, 8, tilt=np.pi / 2)                    # a quarter turn swaps the axes
    a2, b2 = rtus.elliptical_slowness(5300.0, 6100.0, 8)
    assert np.max(np.abs(a - a2)) <= 1e-18 and np.max(np.abs(b - b2)) <= 1e-18


def test_cusps_raise_for_qsv_and_not_for_qp_and_sh(rtus):
    with pytest.raises(ValueError, match="cusps"):
        rtus.group_slowness_ti(**WELD, mode="qSV")
    rtus.group_slowness_ti(**WELD, mode="qP")
    psi, s = rtus.group_slowness_ti(**WELD, mode="SH", C66=82e9)
    # SH is elliptical in a TI medium: group velocities sqrt(C66 / rho) across and sqrt(C55 / rho) along the axis
    vx, vz = np.sqrt(82e9 / 7900.0), np.sqrt(129e9 / 7900.0)
    assert np.max(np.abs(s / np.sqrt((np.sin(psi) / vx) ** 2 + (np.cos(psi) / vz) ** 2) - 1)) <= 1e-13
    with pytest.raises(ValueError):
        rtus.group_slowness_ti(**WELD, mode="SH")
    with pytest.raises(ValueError):
        rtus.group_slowness_ti(**WELD, mode="P")


def test_elliptical_slowness_matches_its_closed_form(rtus):
    vx, vz = 6100.0, 5300.0
    u = np.linspace(-np.pi, np.pi, 2001)
    exact = np.sqrt((np.sin(u) / vx) ** 2 + (np.cos(u) / vz) ** 2)
    err = {K: float(np.max(np.abs(rtus.eval_group_slowness(*rtus.elliptical_slowness(vx, vz, K), u) / exact - 1))) for K in (4, 8, 12)}
    print("elliptical series, relative misfit:", err)
    assert err[4] < 1e-6 and err[8] < 1e-11 and err[12] <= 2e-15
    t = 0.3
    a, b = rtus.elliptical_slowness(vx, vz, 12, tilt=t)
    assert np.max(np.abs(rtus.eval_group_slowness(a, b, u) / np.sqrt((np.sin(u - t) / vx) ** 2 + (np.cos(u - t) / vz) ** 2) - 1)) <= 2e-15


def test_oracle_derivative_matches_central_differences(rtus):
    psi, s = rtus.group_slowness_ti(**WELD, mode="qP")
    a, b, _ = rtus.fit_group_slowness(psi, s, 16, tilt=np.deg2rad(25))
    coef = S.spline(X0, DX, _wavy())
    rng = np.random.default_rng(2)
    n = 400
    x = rng.uniform(X0 + 1e-4, X0 + (NS - 1) * DX - 1e-4, n)
    xe, ze = rng.uniform(-0.02, 0.02, n), rng.uniform(-0.005, 0.01, n)
    xf, zf = rng.uniform(-0.02, 0.02, n), rng.uniform(0.023, 0.05, n)
    h = 3e-8
    k = np.floor((x - X0) / DX)
    keep = (np.floor((x - h - X0) / DX) == k) & (np.floor((x + h - X0) / DX) == k)        # (T''' jumps at the knots)
    d1 = A.travel(coef, X0, DX, C1, a, b, xe, ze, xf, zf, x)[1]
    fd = (A.travel(coef, X0, DX, C1, a, b, xe, ze, xf, zf, x + h)[0] - A.travel(coef, X0, DX, C1, a, b, xe, ze, xf, zf, x - h)[0]) / (2 * h)
    # T ~ 2e-5 s at 1e-16 relative over 2 h: 7e-14 s/m of rounding; truncation h^2 T''' / 6 ~ 4e-14 (s''' ~ 4e5 / m^2); the bound
    # is 7e-13
    assert keep.sum() > 300 and np.max(np.abs(d1 - fd)[keep]) <= 1e-9 * np.max(np.abs(d1))


def test_oracle_with_an_isotropic_series_equals_the_isotropic_oracle():
    zs = _wavy()
    xe, ze = np.r_[np.linspace(-0.012, 0.012, 4), 0.025], np.zeros(5)
    rng = np.random.default_rng(11)
    xf, zf = rng.uniform(-0.024, 0.024, 150), rng.uniform(0.012, 0.045, 150)
    o = A.table(X0, DX, zs, C1, [1 / 5900.0], [0.0], xe, ze, xf, zf)
    r = S.table(X0, DX, zs, C1, 5900.0, xe, ze, xf, zf)
    assert np.array_equal(np.isnan(o["t"]), np.isnan(r["t"]))
    fin = np.isfinite(r["t"])
    assert 0.3 < fin.mean() < 0.9
    assert np.max(np.abs(o["t"][fin] - r["t"][fin])) <= 1e-18
    clear = fin & (r["gap"] > 1e-12)
    assert np.max(np.abs(o["x"][clear] - r["x"][clear])) <= 1e-9
    assert np.array_equal(o["n_min"], S.count_minima(X0, DX, zs, C1, 5900.0, xe, ze, xf, zf))
    assert o["n_min"].max() >= 3 and np.all((o["gap3"] >= o["gap"]) | (o["n_min"] < 3))
    d = A.direct([1 / 5900.0], [0.0], [0.0, np.nan], [0.0, 0.0], [0.003, 0.0, np.inf], [0.004, 0.0, 1.0])
    assert d[0, 0] == pytest.approx(0.005 / 5900.0, rel=1e-15) and d[0, 1] == 0.0 and np.isnan(d[0, 2]) and np.isnan(d[1]).all()


def test_invalid_arguments_are_status_codes(rtus):
    """the series' checks (K, finite, positive) and rtus_tt_surface's return -1 / -4 before any HIP call (no GPU here)"""
    L = rtus.lib()
    assert L.rtus_version() >= 127
    zs = np.full(8, 0.02)
    v = np.zeros(4)
    p, z = v.ctypes.data, zs.ctypes.data
    nb = L.rtus_tt_surface_workspace_bytes(8)
    ws = np.zeros(nb + 512, dtype=np.uint8)
    wp = (ws.ctypes.data + 255) // 256 * 256
    good = np.r_[1 / 5900.0, np.zeros(17)]
    zero = np.zeros(18)

    def dev(a=good, b=zero, K=0, dx=1e-3, n_s=8, c1=C1, xe=p, n_e=1, n_f=1, tt=p, w=wp, nbytes=nb):
        return L.rtus_tt_aniso_surface_dev(0.0, dx, z, n_s, c1, None if a is None else a.ctypes.data, None if b is None else b.ctypes.data,
                                           K, xe, p, n_e, p, p, n_f, tt, None, w, nbytes, None)

    def host(a=good, b=zero, K=0, n_s=8, tt=p):
        return L.rtus_tt_aniso_surface(0.0, 1e-3, z, n_s, C1, a.ctypes.data, b.ctypes.data, K, p, p, 1, p, p, 1, tt, None, 0)

    def direct(a=good, b=zero, K=0, n_e=1, tt=p, fn=L.rtus_tt_aniso_direct, last=0):
        return fn(a.ctypes.data, b.ctypes.data, K, p, p, n_e, p, p, 1, tt, last)

    bad_series = [dict(K=17), dict(K=-1), dict(a=None), dict(b=None),
                  dict(a=np.r_[np.nan, zero[1:]]), dict(a=np.r_[good[0], np.inf, zero[2:]], K=1), dict(b=np.r_[0.0, np.nan, zero[2:]], K=1),
                  dict(a=zero), dict(a=-good), dict(a=np.r_[1e-4, 2e-4, zero[2:]], K=1), dict(b=np.r_[0.0, 1.5 * good[0], zero[2:]], K=1)]
    for kw in bad_series:
        assert dev(**kw) == -1, kw
        if kw.get("a", 0) is not None and kw.get("b", 0) is not None:
            assert host(**kw) == -1 and direct(**kw) == -1 and direct(fn=L.rtus_tt_aniso_direct_dev, last=None, **kw) == -1, kw
    assert dev(b=np.r_[np.nan, zero[1:]], w=None) == -4, "b[0] is ignored"
    assert dev(a=np.r_[1e-4, 0.9e-4, zero[2:]], K=1, w=None) == -4 and dev(K=16, w=None) == -4       # good series: the next check answers
    assert dev(n_s=3) == -1 and dev(dx=0.0) == -1 and dev(c1=0.0) == -1 and dev(c1=float("nan")) == -1
    assert dev(xe=None) == -1 and dev(tt=None) == -1 and dev(n_e=0) == -1 and dev(n_f=-1) == -1
    assert dev(w=None) == -4 and dev(w=wp + 8) == -4 and dev(nbytes=nb - 1) == -4
    assert host(n_s=3) == -1 and host(tt=None) == -1
    assert direct(n_e=0) == -1 and direct(tt=None) == -1 and direct(n_e=65536) == -5


def test_python_wrapper_validation(rtus):
    iso = ([1 / 5900.0], [0.0])
    zs = np.full(8, 0.02)
    with pytest.raises(ValueError):
        rtus.travel_time_surface_aniso(0.0, 1e-3, zs, C1, iso, [0.0, 1.0], [0.0], [0.0], [0.03])
    with pytest.raises(ValueError):
        rtus.travel_time_surface_aniso(0.0, 1e-3, zs, C1, iso, [0.0], [0.0], [0.0], [0.03], out=np.zeros((2, 1)))
    for bad in (([1e-4, 0.0], [0.0]), ([], []), 1e-4, ([[1e-4]], [[0.0]])):
        with pytest.raises(ValueError):
            rtus.travel_time_surface_aniso(0.0, 1e-3, zs, C1, bad, [0.0], [0.0], [0.0], [0.03])
        with pytest.raises(ValueError):
            rtus.travel_time_aniso(bad, [0.0], [0.0], [0.0], [0.03])
    for bad in ((np.full(18, 1e-4), np.zeros(18)), ([np.nan], [0.0]), ([1e-4, 2e-4], [0.0, 0.0])):     # K = 17, NaN, negative
        with pytest.raises(rtus.RtusError) as e:
            rtus.travel_time_surface_aniso(0.0, 1e-3, zs, C1, bad, [0.0], [0.0], [0.0], [0.03])
        assert e.value.status == -1
        with pytest.raises(rtus.RtusError) as e:
            rtus.travel_time_aniso(bad, [0.0], [0.0], [0.0], [0.03])
        assert e.value.status == -1
    with pytest.raises(rtus.RtusError):
        rtus.travel_time_surface_aniso(0.0, 1e-3, np.zeros(3), C1, iso, [0.0], [0.0], [0.0], [0.03])
    with pytest.raises(ValueError):
        rtus.fit_group_slowness([0.0, 1.0], [1.0, 1.0], 2)
    psi = np.pi * np.arange(64) / 64
    with pytest.raises(ValueError):
        rtus.fit_group_slowness(psi, np.ones(64), 17)
    with pytest.raises(ValueError):
        rtus.fit_group_slowness(psi[::-1], np.ones(64), 2)
    with pytest.raises(ValueError):
        rtus.elliptical_slowness(0.0, 5300.0)
    for name in ("travel_time_surface_aniso", "travel_time_aniso", "group_slowness_ti", "fit_group_slowness", "elliptical_slowness",
                 "eval_group_slowness"):
        assert name in rtus.__all__ and callable(getattr(rtus, name))
    assert {"rtus_tt_aniso_surface", "rtus_tt_aniso_surface_dev", "rtus_tt_aniso_direct", "rtus_tt_aniso_direct_dev"} <= set(rtus.EXPORTS)

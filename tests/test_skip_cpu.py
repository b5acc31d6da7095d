"""CPU: the skip-leg oracle (tests/skip_numpy.py) against mpmath at 40 digits (a nested minimisation over the entry and reflection
points), against surface_numpy at the mirrored depth and against a planar restatement; the view and leg naming; ValueErrors of
the Python layer; argument validation of rtus_tt_surface_skip* through ctypes (status codes, no GPU touched)."""
import ctypes as C

import mpmath as mp
import numpy as np
import pytest

import skip_numpy as K
import surface_numpy as S

mp.mp.dps = 40
X0, DX, NS = -0.02, 1e-3, 41
C1, CL, CT = 1480.0, 5900.0, 3230.0
ZB = 0.045
MODES = {"LL": (CL, CL), "LT": (CL, CT), "TL": (CT, CL), "TT": (CT, CT)}


def _wavy(amp=0.0015, lam=0.010, z0=0.02):
    x = X0 + DX * np.arange(NS)
    return z0 + amp * np.sin(2 * np.pi * x / lam)


def _mp_entry(coef, xe, ze, xf, zf, cd, cu, x_start, xb_start):
    """T at the stationary point of |E - S(x)|/c1 + |S(x) - B|/c_down + |B - F|/c_up over (x, xb) near the start, in mpmath"""
    k = int(np.clip(np.floor((x_start - X0) / DX), 0, NS - 2))
    a, b, c, d = (mp.mpf(float(v)) for v in coef[k])
    xk = mp.mpf(X0) + k * mp.mpf(DX)
    E, F = (mp.mpf(float(xe)), mp.mpf(float(ze))), (mp.mpf(float(xf)), mp.mpf(float(zf)))
    c1, cd, cu, zb = mp.mpf(C1), mp.mpf(cd), mp.mpf(cu), mp.mpf(ZB)

    def T(x, xb):
        t = x - xk
        s = a + t * (b + t * (c + t * d))
        return (mp.sqrt((x - E[0]) ** 2 + (s - E[1]) ** 2) / c1 + mp.sqrt((xb - x) ** 2 + (zb - s) ** 2) / cd
                + mp.sqrt((F[0] - xb) ** 2 + (zb - F[1]) ** 2) / cu)
    g = lambda x, xb: (mp.diff(lambda v: T(v, xb), x), mp.diff(lambda v: T(x, v), xb))      # noqa: E731
    x, xb = mp.findroot(g, (mp.mpf(float(x_start)), mp.mpf(float(xb_start))))
    assert xk <= x <= xk + mp.mpf(DX)                   # the root stayed on the start's segment (one cubic)
    return T(x, xb), x, xb


@pytest.mark.parametrize("mode", ["LL", "LT", "TL", "TT"])
def test_oracle_against_mpmath(mode):
    cd, cu = MODES[mode]
    zs = _wavy()
    coef = S.spline(X0, DX, zs)
    xe, ze = np.array([-0.011, 0.0, 0.007]), np.array([0.0, -0.002, 0.001])
    xf, zf = np.array([-0.006, 0.004, 0.013]), np.array([0.031, 0.042, 0.026])
    o = K.table(X0, DX, zs, C1, cd, cu, ZB, xe, ze, xf, zf)
    assert np.isfinite(o["t"]).all()
    for i in range(3):
        for j in range(3):
            t, x, xb = _mp_entry(coef, xe[i], ze[i], xf[j], zf[j], cd, cu, o["x"][i, j], o["xb"][i, j])
            assert abs(float(t) - o["t"][i, j]) <= 1e-17 + 2e-15 * o["t"][i, j], (mode, i, j)
            assert abs(float(x) - o["x"][i, j]) <= 1e-9 and abs(float(xb) - o["xb"][i, j]) <= 1e-9


def test_oracle_equal_speeds_is_the_surface_oracle_at_the_mirrored_depth():
    zs = _wavy()
    xe, ze = np.linspace(-0.012, 0.012, 6), np.zeros(6)
    rng = np.random.default_rng(4)
    xf, zf = rng.uniform(-0.019, 0.019, 120), rng.uniform(0.018, 0.05, 120)     # some above the surface, some below the backwall
    for c in (CL, CT):
        o = K.table(X0, DX, zs, C1, c, c, ZB, xe, ze, xf, zf)
        r = S.table(X0, DX, zs, C1, c, xe, ze, xf, 2 * ZB - zf)
        r_t = np.where(zf[None, :] < ZB, r["t"], np.nan)
        s_f = S.spline_eval(S.spline(X0, DX, zs), X0, DX, xf)[0]
        r_t = np.where(zf[None, :] > s_f[None, :], r_t, np.nan)
        assert np.array_equal(np.isnan(o["t"]), np.isnan(r_t))
        g = np.isfinite(r_t)
        assert g.mean() > 0.5
        assert np.max(np.abs(o["t"][g] - r_t[g]) / r_t[g]) <= 2e-15


@pytest.mark.parametrize("mode", ["LL", "LT", "TL", "TT"])
def test_oracle_flat_profile_against_the_planar_form(mode):
    cd, cu = MODES[mode]
    xe, ze = np.linspace(-0.01, 0.01, 5), np.linspace(-0.003, 0.0, 5)
    rng = np.random.default_rng(5)
    xf, zf = rng.uniform(-0.015, 0.015, 80), rng.uniform(0.021, 0.0449, 80)
    o = K.table(X0, DX, np.full(NS, 0.02), C1, cd, cu, ZB, xe, ze, xf, zf)
    p = K.planar(xe[:, None], ze[:, None], 0.02, ZB, xf[None, :], zf[None, :], C1, cd, cu)
    assert np.isfinite(o["t"]).all()
    assert np.max(np.abs(o["t"] - p) / p) <= 2e-15


def test_oracle_validity_rules():
    zs = _wavy()
    xe, ze = np.array([0.0, 0.0]), np.array([0.0, 0.019])            # the second element is not above the whole profile
    xf, zf = np.array([0.0, 0.0, 0.0, 0.03]), np.array([0.03, ZB, 0.05, 0.03])
    o = K.table(X0, DX, zs, C1, CL, CT, ZB, xe, ze, xf, zf)
    assert np.isfinite(o["t"][0, 0]) and np.isnan(o["t"][0, 1:]).all() and np.isnan(o["t"][1]).all()
    assert np.isnan(K.table(X0, DX, zs, C1, CL, CT, float(zs.max()), xe[:1], ze[:1], [0.0], [0.02])["t"]).all()


# ---------------------------------------------------------------------------------------------- views and legs
def test_view_and_leg_naming(rtus):
    assert rtus.LEGS == ("L", "T", "LL", "LT", "TL", "TT")
    assert len(rtus.VIEWS) == 21 and len(set(rtus.VIEWS)) == 21
    assert [rtus.reverse_leg(g) for g in rtus.LEGS] == ["L", "T", "LL", "TL", "LT", "TT"]
    recip = lambda v: "-".join(rtus.reverse_leg(g) for g in v.split("-")[::-1])          # noqa: E731
    assert recip("LT-T") == "T-TL" and recip("LT-LT") == "TL-TL"
    # the 21 views are one per reciprocity class of the 36 (transmit leg, receive leg) pairs
    classes = {frozenset((f"{a}-{b}", recip(f"{a}-{b}"))) for a in rtus.LEGS for b in rtus.LEGS}
    assert len(classes) == 21
    assert all(sum(v in c for v in rtus.VIEWS) == 1 for c in classes)
    # a view's tables: transmit leg A, receive table reverse(B); a view and its reciprocal swap the tables
    assert rtus.view_tables("LT-LT") == ("LT", "TL") and rtus.view_tables("TL-TL") == ("TL", "LT")
    assert rtus.view_tables("L-T") == ("L", "T") and rtus.view_tables("LL-TL") == ("LL", "LT")
    for v in rtus.VIEWS:
        a, b = rtus.view_tables(v)
        assert rtus.view_tables(recip(v)) == (b, a)
    for bad in ("L", "L-", "LX-L", "L-T-L", "LLL-L", "l-l", 3):
        with pytest.raises(ValueError):
            rtus.view_tables(bad)
    with pytest.raises(ValueError):
        rtus.reverse_leg("LTT")


def test_value_errors_before_any_gpu_call(rtus):
    xe, ze, xf, zf = [0.0], [0.0], [0.0], [0.03]
    with pytest.raises(ValueError):                     # backwall at or above the last interface
        rtus.skip_travel_time_layers([0.02], [1480.0, 5900.0], 0.02, xe, ze, xf, zf)
    with pytest.raises(ValueError):
        rtus.skip_travel_time_layers([0.02], [1480.0, 5900.0], 0.01, xe, ze, xf, zf)
    with pytest.raises(ValueError):                     # n_if + 1 > RTUS_MAX_LAYERS
        z = list(0.001 * np.arange(1, 9))
        rtus.skip_travel_time_layers(z, [1480.0] * 9, 0.05, xe, ze, xf, zf)
    with pytest.raises(ValueError):
        rtus.skip_travel_time_layers([0.02], [1480.0], 0.05, xe, ze, xf, zf)
    with pytest.raises(ValueError):
        rtus.view_legs_layers([0.02], [1480.0], CL, CT, ZB, xe, ze, xf, zf, legs=("L", "LX"))
    with pytest.raises(ValueError):
        rtus.view_legs_layers([0.02], [1480.0, 2330.0], CL, CT, ZB, xe, ze, xf, zf)
    with pytest.raises(ValueError):
        rtus.view_legs_surface(X0, DX, np.full(NS, 0.02), C1, CL, CT, ZB, xe, ze, xf, zf, legs=("Q",))
    fmc = np.zeros((1, 1, 8), dtype=np.float32)
    legs = {"L": np.zeros((1, 1)), "LT": np.zeros((1, 1))}
    with pytest.raises(ValueError):                     # unknown view
        rtus.tfm_views(fmc, 1e8, legs, ["L-L", "L-X"])
    with pytest.raises(ValueError):                     # LT-LT needs TL
        rtus.tfm_views(fmc, 1e8, legs, ["LT-LT"])
    with pytest.raises(ValueError):
        rtus.tfm_views(fmc, 1e8, legs, ["L-L"], coherence=True)


# ---------------------------------------------------------------------------------------------- status codes through ctypes
def _d(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def test_status_codes(rtus):
    L = rtus.lib()
    p = lambda a: a.ctypes.data                                                       # noqa: E731
    fake = C.c_void_p(256)                                                           # device pointers are never dereferenced by the checks
    zs, xe, ze, xf, zf, tt = _d(np.full(16, 0.02)), _d([0.0]), _d([0.0]), _d([0.0]), _d([0.03]), np.zeros(1)
    for dev in (True, False):
        def skip(zsv=zs, n_s=16, dx=1e-3, x0=0.0, c1=1480.0, cd=5900.0, cu=3230.0, zb=0.05, e=xe, n_e=1, n_f=1, out=tt, ws=fake,
                 wsb=1 << 20):
            args = (x0, dx, None if zsv is None else p(zsv), n_s, c1, cd, cu, zb, None if e is None else p(e), p(ze), n_e, p(xf), p(zf),
                    n_f, None if out is None else p(out), None, None)
            return L.rtus_tt_surface_skip_dev(*args, ws, wsb, None) if dev else L.rtus_tt_surface_skip(*args, 0)
        assert skip(zsv=None) == -1 and skip(e=None) == -1 and skip(out=None) == -1
        assert skip(n_s=3) == -1 and skip(n_e=0) == -1 and skip(n_f=0) == -1 and skip(dx=0.0) == -1 and skip(x0=np.nan) == -1
        assert skip(c1=-1.0) == -1 and skip(cd=0.0) == -1 and skip(cd=np.inf) == -1 and skip(cu=-3230.0) == -1 and skip(cu=np.nan) == -1
        assert skip(zb=np.nan) == -1 and skip(zb=np.inf) == -1
        assert skip(n_s=(1 << 22) + 1) == -5 and skip(n_e=65535 * 8 + 1) == -5
        if dev:
            assert skip(ws=None) == -4 and skip(wsb=16) == -4 and skip(ws=C.c_void_p(257)) == -4

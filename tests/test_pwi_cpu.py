"""CPU: the plane-wave oracle (tests/pwi_numpy.py) against mpmath at 40 digits and a brute-force Huygens minimum, the synthesis
oracle on exact cases, and argument validation of the six plane-wave entries through ctypes (status codes, no GPU touched)."""
import ctypes as C

import mpmath as mp
import numpy as np
import pytest

import pwi_numpy as P
import surface_numpy as S

mp.mp.dps = 40
X_LO, X_HI, Z_A = -0.0096, 0.0096, 0.0


def _mp_layers(z_if, c, th, x_lo, x_hi, z_a, xf, zf):
    """the header's closed form in mpmath: None where the entry is NaN"""
    th = mp.mpf(float(th))
    sn = mp.sin(th)
    xref = mp.mpf(x_lo) if sn >= 0 else mp.mpf(x_hi)
    p = sn / mp.mpf(c[0])
    tops = [mp.mpf(z_a)] + [mp.mpf(float(z)) for z in z_if]
    bots = [mp.mpf(float(z)) for z in z_if] + [mp.inf]
    zf, xf = mp.mpf(float(zf)), mp.mpf(float(xf))
    if not zf > tops[0]:
        return None
    t, xb = (xf - xref) * p, xf
    for i, ci in enumerate(c):
        h = max(min(zf, bots[i]) - tops[i], mp.mpf(0))
        if h == 0:
            continue
        pc = p * mp.mpf(ci)
        if abs(pc) >= 1:
            return None
        t += h * mp.sqrt(1 / mp.mpf(ci) ** 2 - p * p)
        xb -= h * pc / mp.sqrt(1 - pc * pc)
    return t if mp.mpf(x_lo) <= xb <= mp.mpf(x_hi) else None


@pytest.mark.parametrize("z_if,c", [([0.02], [1480.0, 5900.0]), ([0.01, 0.025], [1480.0, 2330.0, 5900.0]),
                                    ([0.008, 0.015, 0.03], [2330.0, 1480.0, 3200.0, 5900.0])])
def test_planar_oracle_against_mpmath(z_if, c):
    crit = np.arcsin(c[0] / max(c))
    ang = np.r_[-0.25, -0.05, 0.0, 0.1, crit - 1e-4, crit + 1e-4, 0.9 * np.pi / 2, -(np.pi / 2) + 1e-3]
    rng = np.random.default_rng(3)
    xf = np.r_[rng.uniform(-0.03, 0.03, 40), 0.0, 0.0]
    zf = np.r_[rng.uniform(0.002, 0.05, 40), z_if[0], Z_A]
    got = P.layers(z_if, c, ang, X_LO, X_HI, Z_A, xf, zf)
    n_fin = 0
    for a in range(ang.size):
        for f in range(xf.size):
            r = _mp_layers(z_if, c, ang[a], X_LO, X_HI, Z_A, xf[f], zf[f])
            if r is None:
                assert np.isnan(got[a, f]), (a, f)
            else:
                n_fin += 1
                assert abs(got[a, f] - float(r)) <= 1e-15 * float(r), (a, f)
    assert n_fin > 40


def test_planar_band_edges_against_mpmath():
    """focal points a hair inside and outside the insonified band: the oracle's mask is the closed form's"""
    z_if, c = [0.02], [1480.0, 5900.0]
    th = 0.12
    p = np.sin(th) / c[0]
    drift = 0.02 * np.tan(th) + 0.01 * p * c[1] / np.sqrt(1 - (p * c[1]) ** 2)       # lateral drift down to zf = 0.03
    xf = np.array([X_LO + drift + 1e-9, X_LO + drift - 1e-9, X_HI + drift - 1e-9, X_HI + drift + 1e-9])
    zf = np.full(4, 0.03)
    got = P.layers(z_if, c, [th], X_LO, X_HI, Z_A, xf, zf)[0]
    assert np.isfinite(got[[0, 2]]).all() and np.isnan(got[[1, 3]]).all()
    for f in range(4):
        r = _mp_layers(z_if, c, th, X_LO, X_HI, Z_A, xf[f], zf[f])
        assert (r is None) == bool(np.isnan(got[f]))


def _layers_point(z_if, c, z_a, xf, zf, q):
    """point-to-point times from (x(q), z_a) to F along the ray of horizontal slowness q, and x(q)"""
    tops = np.r_[z_a, z_if]
    bots = np.r_[z_if, np.inf]
    t, x = np.zeros_like(q), np.full_like(q, xf)
    for i, ci in enumerate(c):
        h = max(min(zf, bots[i]) - tops[i], 0.0)
        ct = np.sqrt(1 - (q * ci) ** 2)
        t += h / (ci * ct)
        x -= h * q * ci / ct
    return t, x


def test_planar_oracle_against_a_huygens_minimum():
    """min over secondary sources on the array line of (firing delay + point-to-point time): sources are sampled densely through the
    ray parameter q of the path to F, so each sample is an exact Fermat path; a parabolic step over the discrete minimum"""
    z_if, c = [0.012, 0.02], [1480.0, 2330.0, 5900.0]
    rng = np.random.default_rng(5)
    ang = np.array([-0.2, -0.06, 0.0, 0.08, 0.18])
    xf, zf = rng.uniform(-0.015, 0.015, 30), rng.uniform(0.022, 0.05, 30)
    tab = P.layers(z_if, c, ang, X_LO, X_HI, Z_A, xf, zf)
    qmax = 1 / max(c) * (1 - 1e-9)
    q = np.linspace(-qmax, qmax, 400001)
    checked = 0
    for a, th in enumerate(ang):
        sn = np.sin(th)
        xref = X_LO if sn >= 0 else X_HI
        for f in range(xf.size):
            t, x = _layers_point(z_if, c, Z_A, xf[f], zf[f], q)
            tot = np.where((x >= X_LO) & (x <= X_HI), (x - xref) * sn / c[0] + t, np.inf)
            k = int(np.argmin(tot))
            if not np.isfinite(tab[a, f]):
                assert k == 0 or k == q.size - 1 or not np.isfinite(tot[k - 1]) or not np.isfinite(tot[k + 1]), (a, f)
                continue
            y0, y1, y2 = tot[k - 1], tot[k], tot[k + 1]
            den = y0 - 2 * y1 + y2
            best = y1 - (y0 - y2) ** 2 / (8 * den) if den > 0 else y1
            assert abs(best - tab[a, f]) <= 1e-12 * tab[a, f], (a, f, best, tab[a, f])
            checked += 1
    assert checked > 40


def _wavy(x0=-0.02, dx=1e-3, ns=41):
    x = x0 + dx * np.arange(ns)
    return x0, dx, 0.02 + 0.0015 * np.sin(2 * np.pi * x / 0.010)


def test_surface_oracle_against_mpmath():
    """the winning minimum of a few entries on a wavy profile with competing minima, re-solved in mpmath at 40 digits"""
    from test_surface_cpu import _mp_spline
    x0, dx, zs = _wavy()
    c1, c2 = 1480.0, 5900.0
    ang = np.array([-0.12, 0.0, 0.15])
    rng = np.random.default_rng(9)
    xf, zf = rng.uniform(-0.012, 0.012, 40), rng.uniform(0.024, 0.045, 40)
    o = P.surface(x0, dx, zs, c1, c2, ang, X_LO, X_HI, Z_A, xf, zf)
    s = _mp_spline(x0, dx, zs)
    n = 0
    for a in range(ang.size):
        th = mp.mpf(float(ang[a]))
        sn, cs = mp.sin(th), mp.cos(th)
        xref = mp.mpf(X_LO) if sn >= 0 else mp.mpf(X_HI)
        for f in range(0, xf.size, 3):
            if not np.isfinite(o["t"][a, f]):
                continue
            F = (mp.mpf(float(xf[f])), mp.mpf(float(zf[f])))

            def T(x):
                sx = s(x)[0]
                return ((x - xref) * sn + (sx - Z_A) * cs) / c1 + mp.sqrt((x - F[0]) ** 2 + (sx - F[1]) ** 2) / c2

            xs = mp.findroot(lambda x: mp.diff(T, x), mp.mpf(float(o["x"][a, f])))
            assert abs(float(T(xs)) - o["t"][a, f]) <= 1e-15 * o["t"][a, f]
            assert abs(float(xs) - o["x"][a, f]) <= 1e-9
            sx = s(xs)[0]
            xb = xs - (sx - Z_A) * sn / cs
            assert mp.mpf(X_LO) <= xb <= mp.mpf(X_HI)
            n += 1
    assert n >= 10
    # the profile has competing minima: some entry keeps more than one
    _, xall, kind, _ = S.stationary(x0, dx, zs, c1, c2, [0.0], [Z_A], xf, zf)
    assert (kind == 1).sum() > xf.size


def test_surface_oracle_flat_profile_is_the_planar_closed_form():
    x0, dx = -0.02, 1e-3
    zs = np.full(41, 0.02)
    ang = np.array([-0.2, 0.0, 0.1, 0.22])
    rng = np.random.default_rng(2)
    xf, zf = rng.uniform(-0.015, 0.015, 60), rng.uniform(0.021, 0.05, 60)
    o = P.surface(x0, dx, zs, 1480.0, 5900.0, ang, X_LO, X_HI, Z_A, xf, zf)
    r = P.layers([0.02], [1480.0, 5900.0], ang, X_LO, X_HI, Z_A, xf, zf)
    ok = o["basin"] >= dx                            # away from the band edges
    assert np.array_equal(np.isnan(o["t"][ok]), np.isnan(r[ok]))
    fin = ok & np.isfinite(r)
    assert fin.sum() > 60 and np.max(np.abs(o["t"][fin] - r[fin]) / r[fin]) < 1e-14


def test_synth_oracle_exact_cases():
    rng = np.random.default_rng(1)
    fs = 50e6
    fmc = rng.standard_normal((4, 3, 64)).astype(np.float32)
    d = np.array([[0.0, 0.0, 0.0, 0.0],
                  [3 / fs, -2 / fs, 0.0, 10 / fs],
                  [np.nan, 0.0, np.inf, 1e9 / fs]])
    out = P.synth(fmc, fs, d)
    # zero delays: the sum over tx
    acc = np.zeros((3, 64), dtype=np.float32)
    for tx in range(4):
        acc = (acc + fmc[tx]).astype(np.float32)
    assert np.array_equal(out[0], acc)
    # whole-sample delays shift exactly
    acc = np.zeros((3, 64), dtype=np.float32)
    for tx, k in enumerate((3, -2, 0, 10)):
        sh = np.zeros((3, 64), dtype=np.float32)
        if k >= 0:
            sh[:, k:] = fmc[tx][:, :64 - k]
        else:
            sh[:, :k] = fmc[tx][:, -k:]
        acc = (acc + sh).astype(np.float32)
    assert np.array_equal(out[1], acc)
    # NaN, infinite and absurd delays are skipped: only tx 1 fires
    assert np.array_equal(out[2], fmc[1])
    # a half-sample delay interpolates, and the record's first sample leaks into n = 0 from index -1
    h = P.synth(fmc[:1], fs, [[0.5 / fs]])[0]
    assert np.allclose(h[:, 1:], 0.5 * (fmc[0][:, 1:] + fmc[0][:, :-1]), atol=1e-6)
    assert np.allclose(h[:, 0], 0.5 * fmc[0][:, 0], atol=1e-6)


# ---------------------------------------------------------------------------------------------- status codes through ctypes
def _d(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def test_status_codes(rtus):
    L = rtus.lib()
    ang, xf, zf, tt = _d([0.0, 0.1]), _d([0.0]), _d([0.03]), np.zeros(2)
    z1, c2 = _d([0.02]), _d([1480.0, 5900.0])
    p = lambda a: a.ctypes.data                                                       # noqa: E731
    fake = C.c_void_p(256)                                                           # device pointers are never dereferenced by the checks
    for dev in (True, False):
        f = L.rtus_pw_layers_dev if dev else L.rtus_pw_layers
        tail = (None,) if dev else (0,)

        def lay(zif=z1, c=c2, n_if=1, a=ang, n_a=2, lo=-0.01, hi=0.01, za=0.0, x=xf, z=zf, n_f=1, out=tt):
            return f(None if zif is None else p(zif), None if c is None else p(c), n_if, None if a is None else p(a), n_a, lo, hi, za,
                     None if x is None else p(x), p(z), n_f, None if out is None else p(out), *tail)
        assert lay(a=None) == -1 and lay(x=None) == -1 and lay(out=None) == -1 and lay(c=None) == -1
        assert lay(n_a=0) == -1 and lay(n_f=0) == -1 and lay(n_if=-1) == -1
        assert lay(lo=0.02, hi=0.01) == -1 and lay(lo=np.nan) == -1 and lay(za=np.inf) == -1
        assert lay(za=0.02) == -1 and lay(za=0.03) == -1                              # z_a >= z_if[0]
        assert lay(c=_d([0.0, 5900.0])) == -1 and lay(c=_d([1480.0, np.nan])) == -1
        assert lay(zif=_d([0.02, 0.02]), c=_d([1480.0, 2330.0, 5900.0]), n_if=2) == -1
        assert lay(n_a=65536) == -5
        assert lay(zif=_d(np.arange(1, 10) * 0.01), c=_d(np.full(10, 1480.0)), n_if=9) == -5

    zs = _d(np.full(16, 0.02))
    for dev in (True, False):
        def surf(zsv=zs, n_s=16, dx=1e-3, c1=1480.0, cc2=5900.0, a=ang, n_a=2, lo=-0.01, hi=0.01, za=0.0, out=tt, ws=fake, wsb=1 << 20):
            args = (0.0, dx, None if zsv is None else p(zsv), n_s, c1, cc2, None if a is None else p(a), n_a, lo, hi, za, p(xf), p(zf), 1,
                    None if out is None else p(out), None)
            return L.rtus_pw_surface_dev(*args, ws, wsb, None) if dev else L.rtus_pw_surface(*args, 0)
        assert surf(zsv=None) == -1 and surf(a=None) == -1 and surf(out=None) == -1
        assert surf(n_s=3) == -1 and surf(n_a=0) == -1 and surf(dx=0.0) == -1 and surf(dx=np.nan) == -1
        assert surf(c1=-1.0) == -1 and surf(cc2=np.inf) == -1 and surf(lo=0.02, hi=0.01) == -1 and surf(za=np.nan) == -1
        assert surf(n_a=65536) == -5
        if dev:
            assert surf(ws=None) == -4 and surf(wsb=16) == -4 and surf(ws=C.c_void_p(257)) == -4

    fmc = np.zeros((2, 3, 8), dtype=np.float32)
    dl = _d(np.zeros((2, 2)))
    out = np.zeros((2, 3, 8), dtype=np.float32)
    for dev in (True, False):
        g = L.rtus_fmc_synth_tx_dev if dev else L.rtus_fmc_synth_tx
        tail = (None,) if dev else (0,)

        def syn(x=fmc, n_tx=2, n_rx=3, n_t=8, fs=50e6, d=dl, n_v=2, o=out):
            return g(None if x is None else p(x), n_tx, n_rx, n_t, fs, None if d is None else p(d), n_v, None if o is None else p(o), *tail)
        assert syn(x=None) == -1 and syn(d=None) == -1 and syn(o=None) == -1
        assert syn(n_tx=0) == -1 and syn(n_rx=0) == -1 and syn(n_t=0) == -1 and syn(n_v=0) == -1
        assert syn(fs=0.0) == -1 and syn(fs=np.nan) == -1
        assert syn(o=fmc) == -1 and syn(o=dl) == -1                                    # the output overlaps an input
        assert syn(n_v=65536) == -5 and syn(n_t=(1 << 28) + 1) == -5 and syn(n_rx=65536) == -5


def test_python_errors_before_the_library(rtus):
    xe, ze = np.linspace(-0.01, 0.01, 8), np.zeros(8)
    with pytest.raises(ValueError):
        rtus.pw_delays(xe, np.r_[ze[:-1], 1e-3], [0.0], 1480.0)
    with pytest.raises(ValueError):
        rtus.pw_delays(xe, ze, [0.0], -1.0)
    with pytest.raises(ValueError):
        rtus.pw_travel_time_layers([0.02], [1480.0], [0.0], xe, ze, [0.0], [0.03])
    with pytest.raises(ValueError):
        rtus.pw_travel_time_surface(-0.02, 1e-3, np.full(41, 0.02), 1480.0, 5900.0, [0.0], xe, ze[:-1], [0.0], [0.03])
    with pytest.raises(ValueError):
        rtus.fmc_synth_tx(np.zeros((8, 8, 16), np.float32), 50e6, np.zeros((3, 7)))
    with pytest.raises(ValueError):
        rtus.pwi_image(np.zeros((3, 8, 16), np.float32), 50e6, np.zeros((3, 4)), np.zeros((8, 4)), coherence=True)


def test_pw_delays_definition(rtus):
    xe, ze = np.linspace(-0.01, 0.01, 8), np.zeros(8)
    ang = np.array([-0.2, -0.0, 0.0, 0.3, np.nan, np.pi / 2])
    d = rtus.pw_delays(xe, ze, ang, 1480.0)
    r = P.delays(xe, ang, 1480.0)
    assert np.array_equal(np.isnan(d), np.isnan(r)) and np.array_equal(d[:4], r[:4])
    assert np.all(d[:4] >= 0) and np.all(np.min(d[:4], axis=1) == 0)
    assert np.isnan(d[4:]).all()

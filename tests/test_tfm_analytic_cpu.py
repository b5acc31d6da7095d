"""CPU: the envelope-TFM oracle (tests/tfm_analytic_numpy.py) against oracle/tfm_numpy.py plane by plane, the coherence factor's
properties and NaN / zero rules, and argument validation of rtus_tfm_analytic* (status codes through ctypes, Python errors raised
before any library call; no GPU touched)."""
import numpy as np
import pytest

import tfm_analytic_numpy as TA
from oracle import tfm_numpy as T

FS = 50e6


def _case(rng, n_tx=5, n_rx=7, n_t=300, n_f=400, t0=1.0e-6):
    a = (rng.standard_normal((n_tx, n_rx, n_t)) + 1j * rng.standard_normal((n_tx, n_rx, n_t))).astype(np.complex64)
    tt_tx = rng.uniform(0.0, 3.5e-6, (n_tx, n_f))
    tt_rx = rng.uniform(0.0, 3.5e-6, (n_rx, n_f))             # positions from before the record to past its end
    tt_tx[rng.random(tt_tx.shape) < 0.05] = np.nan
    tt_rx[rng.random(tt_rx.shape) < 0.05] = np.nan
    return a, tt_tx, tt_rx, t0


def test_oracle_planes_are_tfm_numpy():
    rng = np.random.default_rng(0)
    a, tt_tx, tt_rx, t0 = _case(rng)
    o = TA.tfm_analytic(a, FS, t0, tt_tx, tt_rx)
    re = T.tfm(a.real, FS, t0, tt_tx, tt_rx)
    im = T.tfm(a.imag, FS, t0, tt_tx, tt_rx)
    assert np.allclose(o["image"].real, re, rtol=0, atol=1e-12) and np.allclose(o["image"].imag, im, rtol=0, atol=1e-12)
    # the float32 [..., 2] layout is the same FMC
    f2 = np.stack([a.real, a.imag], axis=-1).astype(np.float32)
    assert np.array_equal(TA.tfm_analytic(f2, FS, t0, tt_tx, tt_rx)["image"], o["image"])
    # N counts legs, not positions inside the record
    ok_tx, ok_rx = ~np.isnan(tt_tx), ~np.isnan(tt_rx)
    assert np.array_equal(o["N"], ok_tx.sum(0) * ok_rx.sum(0))
    assert np.all((o["cf"] >= 0) & (o["cf"] <= 1))


def _constant_records(value, n_tx, n_rx, n_t=64):
    return np.full((n_tx, n_rx, n_t), value, dtype=np.complex64)


def test_cf_is_one_for_one_pair_and_for_identical_pairs():
    rng = np.random.default_rng(1)
    tt = rng.uniform(0.1e-6, 0.5e-6, (1, 50))
    a = (rng.standard_normal((1, 1, 64)) + 1j * rng.standard_normal((1, 1, 64))).astype(np.complex64)
    o = TA.tfm_analytic(a, FS, 0.0, tt)
    assert np.allclose(o["cf"], 1.0, rtol=0, atol=1e-12) and np.all(o["N"] == 1)
    a = _constant_records(0.3 - 0.7j, 6, 6)                    # every pair reads the same value
    tt = rng.uniform(0.1e-6, 0.5e-6, (6, 50))
    o = TA.tfm_analytic(a, FS, 0.0, tt)
    assert np.allclose(o["cf"], 1.0, rtol=0, atol=1e-12) and np.all(o["N"] == 36)


def test_cf_of_random_phases_is_about_one_over_n():
    rng = np.random.default_rng(2)
    n_e, n_t, n_f = 16, 4096, 3000
    a = np.exp(2j * np.pi * rng.random((n_e, n_e, n_t))).astype(np.complex64)
    tt = rng.integers(0, n_t // 2 - 1, (n_e, n_f)).astype(np.float64)   # fs = 1: integer positions, w = 0, |a| = 1
    o = TA.tfm_analytic(a, 1.0, 0.0, tt)
    n = n_e * n_e
    assert np.allclose(o["E"], n, rtol=1e-6)
    m = np.mean(o["cf"]) * n                                   # |S|^2 / N is exponential with mean 1: std of the mean 0.02
    assert 0.9 <= m <= 1.1, m


def test_cf_counts_legs_with_a_path_and_positions_outside_the_record():
    n_tx, n_rx, n_t = 4, 5, 64
    a = _constant_records(1.0 + 1.0j, n_tx, n_rx, n_t)
    tt_tx = np.full((n_tx, 6), 0.2e-6)
    tt_rx = np.full((n_rx, 6), 0.2e-6)
    tt_tx[0, 1] = np.nan                                       # f = 1: one tx without a path -> N = 3 * 5, cf 1
    tt_rx[[1, 3], 2] = np.nan                                  # f = 2: two rx without a path -> N = 4 * 3, cf 1
    tt_rx[2, 3] = np.inf                                       # f = 3: not finite
    tt_tx[1, 4] = 1e3                                          # f = 4: absurd (5e10 samples)
    tt_rx[4, 5] = 10e-6                                        # f = 5: a path, but past the record: counts in N with value 0
    o = TA.tfm_analytic(a, FS, 0.0, tt_tx, tt_rx)
    assert list(o["N"]) == [20, 15, 12, 16, 15, 20]
    assert np.allclose(o["cf"][:5], 1.0, rtol=0, atol=1e-12)
    assert np.isclose(o["cf"][5], 16 / 20, rtol=1e-12)        # |16 c|^2 / (20 * 16 |c|^2)
    assert abs(o["image"][5] - 16 * (1 + 1j)) < 1e-9


def test_cf_nan_and_zero_rules():
    a = _constant_records(1.0 + 0.0j, 3, 3)
    tt = np.full((3, 4), 0.2e-6)
    tt[:, 0] = np.nan                                          # N = 0: NaN
    tt[:, 1] = 10e-6                                           # every position past the record: E = 0 < N -> 0
    o = TA.tfm_analytic(a, FS, 0.0, tt)
    assert np.isnan(o["cf"][0]) and o["N"][0] == 0 and o["image"][0] == 0
    assert o["cf"][1] == 0.0 and o["N"][1] == 9 and o["E"][1] == 0
    o = TA.tfm_analytic(np.zeros_like(a), FS, 0.0, tt)         # zero records: E = 0 everywhere a path exists
    assert np.isnan(o["cf"][0]) and np.all(o["cf"][1:] == 0.0)
    assert np.isnan(TA.coherence([0j], [0], [0.0])[0]) and TA.coherence([1 + 0j], [1], [0.5])[0] == 1.0   # (clamped)


def test_invalid_arguments_are_status_codes(rtus):
    """argument checks return -1 / -5 before any HIP call (no GPU here)"""
    L = rtus.lib()
    a = np.zeros(2 * 2 * 3 * 64 * 2, dtype=np.float32)
    tt = np.zeros((3, 8))
    img, cf = np.zeros(16, dtype=np.float32), np.zeros(8, dtype=np.float32)
    pa, pt, pi, pc = a.ctypes.data, tt.ctypes.data, img.ctypes.data, cf.ctypes.data

    def call(dev, a=pa, n_tx=2, n_rx=3, n_t=64, fs=FS, t0=0.0, tx=pt, rx=pt, n_f=8, image=pi, cf=pc):
        if dev:
            return L.rtus_tfm_analytic_dev(a, n_tx, n_rx, n_t, fs, t0, tx, rx, n_f, image, cf, None)
        return L.rtus_tfm_analytic(a, n_tx, n_rx, n_t, fs, t0, tx, rx, n_f, image, cf, 0)
    for dev in (False, True):
        assert call(dev, a=None) == -1 and call(dev, tx=None) == -1 and call(dev, rx=None) == -1 and call(dev, image=None) == -1
        assert call(dev, image=None, cf=None) == -1
        assert call(dev, n_t=1) == -1 and call(dev, n_t=0) == -1 and call(dev, n_tx=0) == -1 and call(dev, n_rx=-1) == -1
        assert call(dev, n_f=0) == -1
        assert call(dev, fs=0.0) == -1 and call(dev, fs=-FS) == -1 and call(dev, fs=float("nan")) == -1 and call(dev, fs=float("inf")) == -1
        assert call(dev, t0=float("nan")) == -1 and call(dev, t0=float("inf")) == -1
        assert call(dev, n_t=(1 << 26) + 1) == -5 and call(dev, n_t=1 << 28) == -5
        assert call(dev, n_t=(1 << 26) + 1, a=None) == -1       # invalid before unsupported


def test_python_wrapper_validation(rtus, monkeypatch):
    from importlib import import_module
    api = import_module("ray-tracing-ultrasound_amd.api")

    def no_library():
        raise AssertionError("the library was called")
    monkeypatch.setattr(api._lib, "lib", no_library)
    a = np.zeros((2, 3, 64), dtype=np.complex64)
    tt2, tt3 = np.zeros((2, 5)), np.zeros((3, 5))
    bad = [
        dict(analytic=np.zeros((2, 64), dtype=np.complex64), tt_tx=tt2, tt_rx=tt3),          # not 3-D
        dict(analytic=np.zeros((2, 3, 64), dtype=np.float32), tt_tx=tt2, tt_rx=tt3),         # real, not [..., 2]
        dict(analytic=np.zeros((2, 3, 64, 3), dtype=np.float32), tt_tx=tt2, tt_rx=tt3),
        dict(analytic=np.zeros((2, 3, 64), dtype=np.complex128), tt_tx=tt2, tt_rx=tt3),      # not complex64
        dict(analytic=a, tt_tx=tt2),                                                          # tt_rx defaults to tt_tx: 2 != 3 rows
        dict(analytic=a, tt_tx=tt3, tt_rx=tt3),                                               # tx rows
        dict(analytic=a, tt_tx=tt2, tt_rx=np.zeros((3, 4))),                                  # focal counts differ
        dict(analytic=a, tt_tx=tt2[0], tt_rx=tt3),                                            # 1-D table
        dict(analytic=a, tt_tx=tt2, tt_rx=tt3, out=np.zeros(5, dtype=np.float32)),           # out not complex64
        dict(analytic=a, tt_tx=tt2, tt_rx=tt3, out=np.zeros(4, dtype=np.complex64)),         # out too small
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            rtus.tfm_analytic(fs=FS, **kw)

"""CPU: carrier-aware (IQ) interpolation — the oracle (tests/tfm_iq_numpy.py) at f_demod = 0 against the envelope-TFM oracle, a
pure tone at any fraction, what the step buys on a closed-form point scatterer at 4 samples per cycle (and what linear
interpolation loses there), centre_frequency, every argument error of the Python layer (raised before the library is called) and
the f_demod=None paths.  No GPU call.

The point scatterer: a Gaussian burst of 3 cycles at f0 = 5 MHz (gaussian_pulse's envelope), 16 elements at 0.6 mm pitch,
c = 5900 m/s, fs = 20 MHz, one scatterer at (1.3 mm, 20 mm); the focal point is the scatterer, so every pair's ideal term is 1
and the ideal sum is N = 256.  Figures of this file's own run: |S| / N = 0.9968 carrier-aware against 0.810 linear; the worst
single term is off by 0.0048 against 0.296; with f_demod 10 % off |S| / N = 0.9948."""
import numpy as np
import pytest

import tfm_analytic_numpy as TA
import tfm_iq_numpy as TQ

F0, FS, C, CYCLES = 5e6, 20e6, 5900.0, 3.0
N_EL, PITCH, SCATTERER, N_T = 16, 0.6e-3, (1.3e-3, 20e-3), 256


def burst_fmc(fs=FS, scatterer=SCATTERER, n_t=N_T):
    """-> (a complex128 [16, 16, n_t], tt [16, 1]): the closed-form analytic FMC of one unit scatterer and the travel times to it"""
    x = (np.arange(N_EL) - (N_EL - 1) / 2) * PITCH
    tau = np.hypot(x - scatterer[0], scatterer[1]) / C
    sig = CYCLES / F0 / 2.355
    u = np.arange(n_t)[None, None, :] / fs - (tau[:, None, None] + tau[None, :, None])
    return np.exp(-0.5 * (u / sig) ** 2) * np.exp(2j * np.pi * F0 * u), tau[:, None]


def _terms(a, tt, fs, f_demod):
    """every pair's term at the focal point (the step on the kernels' positions) -> complex [n_tx, n_rx]"""
    h = TQ.half_positions(tt, fs, 0.0)[:, 0]
    s = h[:, None] + h[None, :]
    fl = np.floor(s)
    i = fl.astype(np.int64)
    tx, rx = np.meshgrid(np.arange(a.shape[0]), np.arange(a.shape[1]), indexing="ij")
    return TQ.step(a[tx, rx, i], a[tx, rx, i + 1], (s - fl).astype(np.float64), f_demod, fs)


def test_f_demod_zero_is_the_envelope_oracle_on_the_same_positions():
    """fs a power of two and the times multiples of 2^-31 s: the half positions are fp32 numbers already, so the two oracles see
    the same positions and differ by the rounding of two fp64 sums"""
    rng = np.random.default_rng(11)
    fs, t0, n_t, n_f = 2.0 ** 25, 2.0 ** -20, 120, 300
    a = (rng.standard_normal((5, 4, n_t)) + 1j * rng.standard_normal((5, 4, n_t))).astype(np.complex64)
    tt_tx = rng.integers(-8 * 64, (n_t // 2 + 8) * 64, (5, n_f)) / 64.0 / fs + 0.5 * t0
    tt_rx = rng.integers(-8 * 64, (n_t // 2 + 8) * 64, (4, n_f)) / 64.0 / fs + 0.5 * t0
    tt_tx[rng.random(tt_tx.shape) < 0.05] = np.nan
    tt_rx[rng.random(tt_rx.shape) < 0.05] = np.inf
    tt_tx[:, -2:] = np.nan
    o, ref = TQ.tfm_iq(a, fs, t0, 0.0, tt_tx, tt_rx), TA.tfm_analytic(a, fs, t0, tt_tx, tt_rx)
    assert np.max(np.abs(o["image"] - ref["image"])) <= 1e-12 * np.max(np.abs(ref["image"]))
    assert np.array_equal(o["N"], ref["N"]) and np.allclose(o["E"], ref["E"], rtol=1e-12, atol=0)
    assert np.array_equal(np.isnan(o["cf"]), np.isnan(ref["cf"])) and np.isnan(o["cf"][-2:]).all()
    assert np.allclose(o["cf"], ref["cf"], rtol=0, atol=1e-12, equal_nan=True)
    # one table, and the packed block against the unpacked one
    sq = (rng.standard_normal((6, 6, n_t)) + 1j * rng.standard_normal((6, 6, n_t))).astype(np.complex64)
    sq = sq + sq.transpose(1, 0, 2)
    i, j = np.triu_indices(6)
    tt = np.vstack([tt_tx, tt_rx[:1]])
    for f_demod in (0.0, 0.2 * fs):
        full, packed = TQ.tfm_iq(sq, fs, t0, f_demod, tt), TQ.tfm_iq(sq[i, j], fs, t0, f_demod, tt)
        for k in ("image", "N", "E", "A", "cf"):
            assert np.array_equal(full[k], packed[k], equal_nan=True)
    ref = TA.tfm_analytic(sq, fs, t0, tt)
    assert np.max(np.abs(TQ.tfm_iq(sq, fs, t0, 0.0, tt)["image"] - ref["image"])) <= 1e-12 * np.max(np.abs(ref["image"]))


@pytest.mark.parametrize("nu", [0.11, 0.25, 0.49])
def test_a_pure_tone_is_reproduced_at_any_fraction(nu):
    """a[n] = exp(2 pi i nu n) has a constant envelope: the step returns exp(2 pi i nu s) at every fraction.  (With R as the
    fp64 pair: the header rounds R to fp32 for the kernel, 6e-8 — a figure of the format, not of the step's algebra.)"""
    rng = np.random.default_rng(3)
    n = rng.integers(0, 1000, 4000)
    w = np.r_[0.0, 1.0 - 2.0 ** -24, rng.random(3998)]
    a0, a1 = np.exp(2j * np.pi * nu * n), np.exp(2j * np.pi * nu * (n + 1))
    p = TQ.step(a0, a1, w, nu * FS, FS, exact_r=True)
    assert np.max(np.abs(p - np.exp(2j * np.pi * nu * (n + w)))) <= 1e-12
    rounded = TQ.step(a0, a1, w, nu * FS, FS)
    assert np.max(np.abs(rounded - p)) <= 2.0 ** -24
    if nu != 0.25:                                                          # linear interpolation cuts the corner
        lin = TQ.step(a0, a1, w, 0.0, FS)
        assert np.max(np.abs(lin - np.exp(2j * np.pi * nu * (n + w)))) >= 1.0 - np.cos(np.pi * nu) - 1e-3


@pytest.mark.parametrize("nu", [0.11, 0.25, 0.49])
def test_the_fp32_emulation_stays_inside_the_gpu_tests_bound(nu):
    """what test_gpu_tfm_iq.py allows the kernels: (2 n_tx n_rx 2^-24 + 1e-5) A[f].  The step and the sums in fp32 with correctly
    rounded sines and cosines use a fraction of it (here 1e-7 of A; 2.3e-6 on that file's 1 x 1 case)"""
    rng = np.random.default_rng(17)
    fs, t0, n_t, n_f = 40e6, 1.5e-6, 120, 200
    a = (rng.standard_normal((5, 4, n_t)) + 1j * rng.standard_normal((5, 4, n_t))).astype(np.complex64)
    lo, hi = (-12 + 0.5 * t0 * fs) / fs, (n_t / 2 + 12 + 0.5 * t0 * fs) / fs
    tt_tx, tt_rx = rng.uniform(lo, hi, (5, n_f)), rng.uniform(lo, hi, (4, n_f))
    o, e = TQ.tfm_iq(a, fs, t0, nu * fs, tt_tx, tt_rx), TQ.tfm_iq(a, fs, t0, nu * fs, tt_tx, tt_rx, emulate=True)
    assert o["A"].min() > 0
    d = np.abs(e["image"] - o["image"])
    print(f"nu = {nu}: largest |emulation - oracle| / A = {np.max(d / o['A']):.2e}")
    assert np.all(d <= (2.0 * 5 * 4 * 2.0 ** -24 + 1e-5) * o["A"])
    assert np.max(d / o["A"]) >= 1e-9                                       # (it is an fp32 computation)


def test_point_scatterer_at_four_samples_per_cycle():
    a, tt = burst_fmc()
    n = N_EL * N_EL
    iq, lin = TQ.tfm_iq(a, FS, 0.0, F0, tt), TQ.tfm_iq(a, FS, 0.0, 0.0, tt)
    assert iq["N"][0] == n and lin["N"][0] == n
    t_iq, t_lin = _terms(a, tt, FS, F0), _terms(a, tt, FS, 0.0)
    assert abs(t_iq.sum() - iq["image"][0]) <= 1e-9 and abs(t_lin.sum() - lin["image"][0]) <= 1e-9
    got, got_lin = abs(iq["image"][0]) / n, abs(lin["image"][0]) / n
    off = abs(TQ.tfm_iq(a, FS, 0.0, 1.1 * F0, tt)["image"][0]) / n
    e_iq, e_lin = np.max(np.abs(t_iq - 1.0)), np.max(np.abs(t_lin - 1.0))
    print(f"|S|/N: carrier-aware {got:.4f}, linear {got_lin:.4f}, f_demod 10 % off {off:.4f}; worst term {e_iq:.4f} / {e_lin:.4f}")
    assert got >= 0.99
    assert got_lin <= 0.85
    assert e_iq <= 0.005
    assert e_lin <= 0.30
    assert e_lin >= 0.25 and off >= 0.99                                    # (the loss is there, and f_demod is forgiving)
    ref = TA.tfm_analytic(a, FS, 0.0, tt)                                   # the linear figure is the envelope oracle's
    assert abs(abs(ref["image"][0]) / n - got_lin) <= 1e-3


def test_centre_frequency(rtus):
    a, _ = burst_fmc()
    f = rtus.centre_frequency(a.astype(np.complex64), FS)
    assert isinstance(f, float) and abs(f - F0) <= 0.01 * F0
    assert abs(rtus.centre_frequency(a.real.astype(np.float32), FS) - F0) <= 0.01 * F0      # RF data: the same
    i, j = np.triu_indices(N_EL)
    assert abs(rtus.centre_frequency(a[i, j], FS) - F0) <= 0.01 * F0                        # a packed block
    tone = np.exp(2j * np.pi * 0.125 * np.arange(64))                                        # one positive bin
    assert abs(rtus.centre_frequency(tone, 8.0) - 1.0) <= 1e-9
    for bad in (np.zeros((3, 64)), np.ones(3), np.zeros((0, 64))):
        with pytest.raises(ValueError):
            rtus.centre_frequency(bad, FS)
    with pytest.raises(ValueError):
        rtus.centre_frequency(a, 0.0)


@pytest.fixture
def no_library(rtus, monkeypatch):
    """every use of the library raises: the checks below come before it"""
    import importlib
    lib = importlib.import_module("ray-tracing-ultrasound_amd._lib")

    def boom():
        raise AssertionError("the library was touched before the arguments were checked")
    monkeypatch.setattr(lib, "lib", boom)
    return rtus


def test_value_errors_of_the_wrappers(no_library):
    rtus = no_library
    fs = 40e6
    a = np.zeros((3, 2, 50), dtype=np.complex64)
    tt_tx, tt_rx = np.zeros((3, 7)), np.zeros((2, 7))
    h = np.zeros((6, 50), dtype=np.complex64)
    tt = np.zeros((3, 7))
    for bad in (-1.0, 0.5 * fs, fs, np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError):
            rtus.tfm_iq(a, fs, bad, tt_tx, tt_rx)
        with pytest.raises(ValueError):
            rtus.tfm_iq_hmc(h, fs, bad, tt)
        with pytest.raises(ValueError):
            rtus.tfm_views(np.zeros((3, 3, 50), dtype=np.float32), fs, {"L": tt}, "L-L", envelope=True, f_demod=bad)
        with pytest.raises(ValueError):
            rtus.pwi_image(np.zeros((3, 2, 50), dtype=np.float32), fs, tt_tx, tt_rx, envelope=True, f_demod=bad)
    for mode in ("vcf", "scf", "xcf", 3):
        with pytest.raises(ValueError):
            rtus.tfm_iq(a, fs, 5e6, tt_tx, tt_rx, coherence=mode)
        with pytest.raises(ValueError):
            rtus.tfm_iq_hmc(h, fs, 5e6, tt, coherence=mode)
    with pytest.raises(ValueError):
        rtus.tfm_iq(a.real.copy(), fs, 5e6, tt_tx, tt_rx)                   # not complex
    with pytest.raises(ValueError):
        rtus.tfm_iq(a, fs, 5e6, tt_rx, tt_tx)                               # rows against the FMC
    with pytest.raises(ValueError):
        rtus.tfm_iq(a, fs, 5e6, tt_tx, tt_rx[:, :5])                        # columns differ
    with pytest.raises(ValueError):
        rtus.tfm_iq(a, fs, 5e6, tt_tx, tt_rx, out=np.empty(6, dtype=np.complex64))
    with pytest.raises(ValueError):
        rtus.tfm_iq(a, 0.0, 0.0, tt_tx, tt_rx)
    with pytest.raises(ValueError):
        rtus.tfm_iq_hmc(h[:5], fs, 5e6, tt)                                 # 5 is not a triangular number
    with pytest.raises(ValueError):
        rtus.tfm_iq_hmc(h, fs, 5e6, tt[:2])
    with pytest.raises(ValueError):
        rtus.tfm_iq_hmc(h.real.copy(), fs, 5e6, tt)
    # the f_demod keyword: needs envelope=True, excludes amplitudes and the phase-coherence factors
    rf = np.zeros((3, 3, 50), dtype=np.float32)
    legs = {"L": tt}
    amps = {"L": (np.ones((3, 7), dtype=np.complex64),) * 2}
    with pytest.raises(ValueError, match="envelope"):
        rtus.tfm_views(rf, fs, legs, "L-L", f_demod=5e6)
    with pytest.raises(ValueError, match="envelope"):
        rtus.tfm_views(np.zeros((6, 50), dtype=np.float32), fs, legs, "L-L", hmc=True, f_demod=5e6)
    with pytest.raises(ValueError, match="amplitude"):
        rtus.tfm_views(rf, fs, legs, "L-L", envelope=True, amplitudes=amps, f_demod=5e6)
    for mode in ("vcf", "scf"):
        with pytest.raises(ValueError, match="carrier-aware"):
            rtus.tfm_views(rf, fs, legs, "L-L", envelope=True, coherence=mode, f_demod=5e6)
        with pytest.raises(ValueError, match="carrier-aware"):
            rtus.pwi_image(rf, fs, tt, tt, envelope=True, coherence=mode, f_demod=5e6)
    with pytest.raises(ValueError, match="envelope"):
        rtus.pwi_image(rf, fs, tt, tt, f_demod=5e6)
    xe = np.arange(3) * 1e-3
    with pytest.raises(ValueError, match="envelope"):
        rtus.adaptive_tfm(rf, fs, xe, np.zeros(3), 1480.0, 5900.0, 0.0, 1e-3, 4, 0.01, 0.02, 1e-4, [0.0], [0.03], f_demod=5e6)
    with pytest.raises(ValueError):
        rtus.adaptive_tfm(rf, fs, xe, np.zeros(3), 1480.0, 5900.0, 0.0, 1e-3, 4, 0.01, 0.02, 1e-4, [0.0], [0.03], envelope=True,
                          f_demod=0.5 * fs)


def test_f_demod_none_takes_the_old_paths_and_a_value_the_new_ones(rtus, monkeypatch):
    import importlib
    api = importlib.import_module("ray-tracing-ultrasound_amd.api")
    calls = []

    def new(name):
        def f(analytic, fs, f_demod, tt_tx, tt_rx=None, *, t0=0.0, coherence=False, out=None, device=0):
            calls.append((name, f_demod, coherence))
            img = np.full(np.shape(tt_tx)[1], 2.0 + 0j, dtype=np.complex64)
            return (img, np.ones(img.size, dtype=np.float32)) if coherence else img
        return f

    def old(name):
        def f(analytic, fs, tt_tx, tt_rx=None, *, t0=0.0, coherence=False, out=None, device=0):
            calls.append((name, None, coherence))
            img = np.full(np.shape(tt_tx)[1], 1.0 + 0j, dtype=np.complex64)
            return (img, np.ones(img.size, dtype=np.float32)) if coherence else img
        return f
    for name in ("tfm_iq", "tfm_iq_hmc"):
        monkeypatch.setattr(api, name, new(name))
    for name in ("tfm_analytic", "tfm_analytic_hmc"):
        monkeypatch.setattr(api, name, old(name))
    monkeypatch.setattr(api, "fmc_analytic", lambda fmc, n_taps=63, **k: np.asarray(fmc).astype(np.complex64))
    monkeypatch.setattr(api, "hmc_analytic", lambda h, n_taps=63, **k: np.asarray(h).astype(np.complex64))
    fs, tt = 40e6, np.zeros((3, 7))
    legs = {"L": tt, "T": tt + 1e-6}
    rf, packed = np.zeros((3, 3, 50), dtype=np.float32), np.zeros((6, 50), dtype=np.float32)
    # None: the entry points of before, and only those
    r = api.tfm_views(rf, fs, legs, ("L-L", "L-T"), envelope=True)
    r2 = api.tfm_views(packed, fs, legs, ("L-L", "L-T"), envelope=True, coherence=True, hmc=True, f_demod=None)
    assert np.all(r["L-T"] == 1.0) and np.all(r2["L-L"][0] == 1.0)
    assert np.all(api.pwi_image(rf, fs, tt, tt, envelope=True) == 1.0)
    assert [c[0] for c in calls] == ["tfm_analytic"] * 2 + ["tfm_analytic_hmc"] * 2 + ["tfm_analytic"]
    # a value: the new ones, with the value and the factor handed on
    del calls[:]
    r = api.tfm_views(rf, fs, legs, ("L-L", "L-T"), envelope=True, f_demod=5e6)
    r2 = api.tfm_views(packed, fs, legs, "L-T", envelope=True, coherence=True, hmc=True, f_demod=0.0)
    env, cf = api.pwi_image(rf, fs, tt, tt, envelope=True, coherence="cf", f_demod=4e6)
    assert np.all(r["L-L"] == 2.0) and np.all(r2["L-T"][0] == 2.0) and np.all(env == 2.0) and np.all(cf == 1.0)
    assert calls == [("tfm_iq", 5e6, None)] * 2 + [("tfm_iq_hmc", 0.0, "cf"), ("tfm_iq", 4e6, "cf")]


def test_the_abi_has_the_new_names(rtus):
    L = rtus.lib()
    assert L.rtus_version() >= 119
    for name in ("rtus_tfm_iq_dev", "rtus_tfm_iq", "rtus_tfm_iq_hmc_dev", "rtus_tfm_iq_hmc"):
        assert name in rtus.EXPORTS and hasattr(L, name)
    # a bad f_demod is a status code before any HIP call (no device is needed to be told so), host and _dev twins alike
    a = np.zeros((2, 2, 50), dtype=np.complex64)
    tt = np.zeros((2, 4))
    img = np.zeros(4, dtype=np.complex64)
    p = lambda x: x.ctypes.data
    for bad in (-1.0, 20e6, float("nan"), float("inf")):
        assert L.rtus_tfm_iq(p(a), 2, 2, 50, 40e6, 0.0, bad, p(tt), p(tt), 4, p(img), None, 0) == -1
        assert L.rtus_tfm_iq_dev(p(a), 2, 2, 50, 40e6, 0.0, bad, p(tt), p(tt), 4, p(img), None, None) == -1
        assert L.rtus_tfm_iq_hmc(p(a), 2, 50, 40e6, 0.0, bad, p(tt), p(tt), 4, p(img), None, 0) == -1
        assert L.rtus_tfm_iq_hmc_dev(p(a), 2, 50, 40e6, 0.0, bad, p(tt), p(tt), 4, p(img), None, None) == -1
    assert L.rtus_tfm_iq_dev(None, 2, 2, 50, 40e6, 0.0, 5e6, p(tt), p(tt), 4, p(img), None, None) == -1
    assert L.rtus_tfm_iq_hmc_dev(p(a), 0, 50, 40e6, 0.0, 5e6, p(tt), p(tt), 4, p(img), None, None) == -1


def test_the_new_kernels_use_no_scratch():
    """rtus_tfm.hip and rtus_tfm_hmc.hip compiled device-only to assembly with the Makefile's flags: the two full-matrix and the
    four half-matrix carrier-aware kernels keep everything in registers (no scratch, no spilled VGPR), 64 KiB of LDS each, and few
    enough VGPRs for two waves per SIMD (two workgroups per CU)"""
    import os
    import re
    import subprocess
    import tempfile
    from conftest import ROOT
    csrc = os.path.join(ROOT, "ray-tracing-ultrasound_amd", "csrc")
    flags = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-fno-fast-math", "-fno-slp-vectorize", "--cuda-device-only", "-S"]
    res = {}
    with tempfile.TemporaryDirectory() as td:
        jobs = [(os.path.join(td, f + ".s"), subprocess.Popen(["/opt/rocm/bin/hipcc"] + flags + [os.path.join(csrc, f + ".hip"), "-o",
                                                                os.path.join(td, f + ".s")], stdout=subprocess.DEVNULL,
                                                               stderr=subprocess.DEVNULL)) for f in ("rtus_tfm", "rtus_tfm_hmc")]
        for out, job in jobs:
            assert job.wait(timeout=600) == 0
            meta = open(out).read().split("amdhsa.kernels:")[1]
            for entry in re.split(r"^  - ", meta, flags=re.M)[1:]:          # one list item per kernel; its keys are indented by 4
                kv = dict(re.findall(r"^ {0,4}(\.\w+):\s+(\S+)\s*$", entry, flags=re.M))
                if ".vgpr_count" in kv and "_iq_kernel" in kv[".name"]:
                    res[kv[".name"]] = {k: int(kv[k]) for k in (".vgpr_count", ".vgpr_spill_count", ".private_segment_fixed_size",
                                                                ".group_segment_fixed_size")}
    assert len(res) == 6 and sum("hmc" in k for k in res) == 4, sorted(res)
    for k, v in res.items():
        assert v[".private_segment_fixed_size"] == 0 and v[".vgpr_spill_count"] == 0, (k, v)
        assert v[".vgpr_count"] <= 256 and v[".group_segment_fixed_size"] == 65536, (k, v)

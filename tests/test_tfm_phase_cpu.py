"""CPU: the phase-coherence oracle (tests/tfm_phase_numpy.py) — properties of vcf, scf and the counts, its fp32 mode against its
fp64 mode — and rtus_tfm_phase*'s argument validation (status codes through ctypes, Python errors raised before any library call),
the version, and the new kernel's resources read from the code object's metadata.  No GPU touched."""
import os

import numpy as np
import pytest

import tfm_phase_numpy as TP
import tfm_analytic_numpy as TA
from conftest import ROOT

FS = 50e6


def _constant_records(value, n_tx, n_rx, n_t=64):
    return np.full((n_tx, n_rx, n_t), value, dtype=np.complex64)


def test_identical_constant_records_are_fully_coherent():
    rng = np.random.default_rng(1)
    a = _constant_records(0.3 - 0.7j, 6, 6)
    tt = rng.uniform(0.1e-6, 0.5e-6, (6, 50))
    for fp32 in (False, True):
        o = TP.tfm_phase(a, FS, 0.0, tt, fp32=fp32, kernel_sum=True)
        assert np.all(o["N"] == 36) and np.all(o["B"] == 36)
        assert np.allclose(o["vcf"], 1.0, rtol=0, atol=1e-12) and np.array_equal(o["scf"], np.ones(50))
        assert np.allclose(o["vcf32"], 1.0, rtol=0, atol=36 * 2.0 ** -23)
    o = TP.tfm_phase(_constant_records(-2.0 + 0.0j, 6, 6), FS, 0.0, tt)
    assert np.all(o["B"] == -36) and np.array_equal(o["scf"], np.ones(50))


def test_vcf_of_random_phases_is_about_one_over_n():
    rng = np.random.default_rng(2)
    n_e, n_t, n_f = 16, 4096, 3000
    a = np.exp(2j * np.pi * rng.random((n_e, n_e, n_t))).astype(np.complex64)
    tt = rng.integers(0, n_t // 2 - 1, (n_e, n_f)).astype(np.float64)   # fs = 1: integer positions, w = 0, |a| = 1
    o = TP.tfm_phase(a, 1.0, 0.0, tt)
    n = n_e * n_e
    assert np.all(o["N"] == n)
    m = np.mean(o["vcf"] ** 2) * n                             # |U|^2 / N is exponential with mean 1: std of the mean 0.02
    assert 0.9 <= m <= 1.1, m
    # unit samples: U is S, so vcf^2 is the amplitude coherence factor
    assert np.allclose(o["vcf"] ** 2, TA.tfm_analytic(a, 1.0, 0.0, tt)["cf"], rtol=0, atol=1e-6)
    assert np.mean(o["scf"]) < 0.01                            # signs of random phases: B / N ~ 1 / sqrt N, scf ~ 1 / (2 N)


def test_counts_are_legs_and_positions_outside_the_record_lower_vcf():
    n_tx, n_rx, n_t = 4, 5, 64
    a = _constant_records(1.0 + 1.0j, n_tx, n_rx, n_t)
    tt_tx = np.full((n_tx, 6), 0.2e-6)
    tt_rx = np.full((n_rx, 6), 0.2e-6)
    tt_tx[0, 1] = np.nan                                       # f = 1: one tx without a path -> N = 3 * 5
    tt_rx[[1, 3], 2] = np.nan                                  # f = 2: two rx without a path -> N = 4 * 3
    tt_rx[2, 3] = np.inf                                       # f = 3: not finite
    tt_tx[1, 4] = 1e3                                          # f = 4: absurd (5e10 samples)
    tt_rx[4, 5] = 10e-6                                        # f = 5: a path, but past the record: counts in N with a zero phasor
    for fp32 in (False, True):
        o = TP.tfm_phase(a, FS, 0.0, tt_tx, tt_rx, fp32=fp32)
        assert list(o["N"]) == [20, 15, 12, 16, 15, 20]
        assert list(o["B"]) == [20, 15, 12, 16, 15, 16]
        assert np.allclose(o["vcf"][:5], 1.0, rtol=0, atol=1e-12) and np.all(o["scf"][:5] == 1.0)
        assert np.isclose(o["vcf"][5], 16 / 20, rtol=1e-12)   # K / N, K the pairs still inside the record
        assert np.isclose(o["scf"][5], 1 - np.sqrt(1 - 0.8 ** 2), rtol=1e-12)


def test_nan_and_zero_rules():
    a = _constant_records(1.0 + 0.0j, 3, 3)
    tt = np.full((3, 4), 0.2e-6)
    tt[:, 0] = np.nan                                          # N = 0: NaN
    tt[:, 1] = 10e-6                                           # every position past the record: 0 < N, all phasors zero
    for fp32 in (False, True):
        o = TP.tfm_phase(a, FS, 0.0, tt, fp32=fp32, kernel_sum=True)
        assert np.isnan(o["vcf"][0]) and np.isnan(o["scf"][0]) and np.isnan(o["vcf32"][0]) and o["N"][0] == 0 and o["B"][0] == 0
        assert o["vcf"][1] == 0.0 and o["scf"][1] == 0.0 and o["N"][1] == 9
        assert np.all(o["vcf"][2:] == 1.0) and np.all(o["scf"][2:] == 1.0)
        o = TP.tfm_phase(np.zeros_like(a), FS, 0.0, tt, fp32=fp32)   # an all-zero FMC: 0 wherever a pair has a path
        assert np.isnan(o["vcf"][0]) and np.all(o["vcf"][1:] == 0.0) and np.all(o["scf"][1:] == 0.0) and np.all(o["B"] == 0)
    o = TP.tfm_phase(_constant_records(0.0 + 1.0j, 3, 3), FS, 0.0, tt)   # purely imaginary: every sign is 0, every phasor i
    assert np.all(o["B"] == 0) and np.all(o["scf"][1:] == 0.0) and np.all(o["vcf"][2:] == 1.0)


def test_unit_phasors_of_tiny_and_huge_samples_and_the_fp32_mode():
    """the oracle's phasors do not under- or overflow, and its fp32 mode (the kernel's positions) stays close to the definition"""
    rng = np.random.default_rng(3)
    n_tx, n_rx, n_t, n_f = 5, 7, 300, 400
    a = (rng.standard_normal((n_tx, n_rx, n_t)) + 1j * rng.standard_normal((n_tx, n_rx, n_t))).astype(np.complex64)
    a[2] *= np.float32(1e-30)
    a[3] *= np.float32(1e30)
    a[:, :, 100:120] = 0
    tt_tx = rng.uniform(0.0, 3.5e-6, (n_tx, n_f))
    tt_rx = rng.uniform(0.0, 3.5e-6, (n_rx, n_f))
    tt_tx[rng.random(tt_tx.shape) < 0.05] = np.nan
    P, ok_tx, ok_rx = TP.samples(a, FS, 1e-6, tt_tx, tt_rx, fp32=True)
    u = TP.unit(P)
    m = np.abs(u)
    assert np.all((m == 0) == (P == 0)) and np.allclose(m[m > 0], 1.0, rtol=0, atol=1e-15)
    assert (P[2] != 0).any() and (P[3] != 0).any() and np.array_equal(ok_tx, ~np.isnan(tt_tx))
    o64 = TP.tfm_phase(a, FS, 1e-6, tt_tx, tt_rx)
    o32 = TP.tfm_phase(a, FS, 1e-6, tt_tx, tt_rx, fp32=True, kernel_sum=True)
    assert np.array_equal(o64["N"], o32["N"]) and np.abs(o64["B"] - o32["B"]).max() <= 1
    assert np.nanmax(np.abs(o64["vcf"] - o32["vcf"])) <= 1e-3
    assert np.nanmax(np.abs(o32["vcf32"] - o32["vcf"])) <= (35 + 8) * 2.0 ** -23
    # the legs of the fp32 mode, once more with the multiplication and the subtraction fused
    assert np.array_equal(TP.legs_f32(tt_tx, FS, 1e-6), TP.legs_f32(tt_tx, FS, 1e-6, fused=True))


def test_invalid_arguments_are_status_codes(rtus):
    """argument checks return -1 / -5 before any HIP call (no GPU here): rtus_tfm_analytic's list, and the pair limit"""
    L = rtus.lib()
    a = np.zeros(2 * 2 * 3 * 64 * 2, dtype=np.float32)
    tt = np.zeros((3, 8))
    img, f1, f2, cn = (np.zeros(16, dtype=np.float32), np.zeros(8, dtype=np.float32), np.zeros(8, dtype=np.float32),
                       np.zeros(16, dtype=np.int32))
    pa, pt, pi = a.ctypes.data, tt.ctypes.data, img.ctypes.data
    opt = (f1.ctypes.data, f2.ctypes.data, cn.ctypes.data)

    def call(dev, a=pa, n_tx=2, n_rx=3, n_t=64, fs=FS, t0=0.0, tx=pt, rx=pt, n_f=8, image=pi, opt=opt):
        if dev:
            return L.rtus_tfm_phase_dev(a, n_tx, n_rx, n_t, fs, t0, tx, rx, n_f, image, *opt, None)
        return L.rtus_tfm_phase(a, n_tx, n_rx, n_t, fs, t0, tx, rx, n_f, image, *opt, 0)
    none = (None, None, None)
    for dev in (False, True):
        assert call(dev, a=None) == -1 and call(dev, tx=None) == -1 and call(dev, rx=None) == -1 and call(dev, image=None) == -1
        assert call(dev, image=None, opt=none) == -1
        assert call(dev, n_t=1) == -1 and call(dev, n_t=0) == -1 and call(dev, n_tx=0) == -1 and call(dev, n_rx=-1) == -1
        assert call(dev, n_f=0) == -1
        assert call(dev, fs=0.0) == -1 and call(dev, fs=-FS) == -1 and call(dev, fs=float("nan")) == -1 and call(dev, fs=float("inf")) == -1
        assert call(dev, t0=float("nan")) == -1 and call(dev, t0=float("inf")) == -1
        assert call(dev, n_t=(1 << 26) + 1) == -5 and call(dev, n_t=1 << 28) == -5
        assert call(dev, n_t=(1 << 26) + 1, a=None) == -1       # invalid before unsupported
        # the sign sum is an int32: n_tx n_rx <= 2^30; with every optional output null too (accepted at the argument check: the limit
        # is what refuses the call)
        assert call(dev, n_tx=1 << 15, n_rx=(1 << 15) + 1) == -5 and call(dev, n_tx=1 << 16, n_rx=1 << 16, opt=none) == -5
        assert call(dev, n_tx=(1 << 15) + 1, n_rx=1 << 15, opt=none) == -5
        assert call(dev, n_tx=1 << 16, n_rx=1 << 16, opt=none, image=None) == -1
    assert L.rtus_version() >= 115
    for name in ("rtus_tfm_phase", "rtus_tfm_phase_dev"):
        assert name in rtus.EXPORTS and hasattr(L, name)


def test_python_wrapper_validation(rtus, monkeypatch):
    from importlib import import_module
    api = import_module("ray-tracing-ultrasound_amd.api")
    assert rtus.tfm_phase is api.tfm_phase and "tfm_phase" in rtus.__all__

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
            rtus.tfm_phase(fs=FS, **kw)
        with pytest.raises(ValueError):
            rtus.tfm_analytic(fs=FS, coherence="vcf", **kw)
    # the coherence keyword: anything but False, True, "cf", "vcf", "scf" is refused
    fmc = np.zeros((2, 3, 64), dtype=np.float32)
    for what in ("nonsense", "VCF", "", 2, 1.0, ("vcf",)):
        with pytest.raises(ValueError):
            rtus.tfm_analytic(a, FS, tt2, tt3, coherence=what)
        with pytest.raises(ValueError):
            rtus.pwi_image(fmc, FS, tt2, tt3, envelope=True, coherence=what)
        with pytest.raises(ValueError):
            rtus.tfm_views(np.zeros((3, 3, 64), dtype=np.float32), FS, {"L": tt3}, ("L-L",), envelope=True, coherence=what)
    # a factor's name needs envelope=True, and excludes amplitudes, as True does
    for what in (True, "cf", "vcf", "scf"):
        with pytest.raises(ValueError, match="envelope"):
            rtus.pwi_image(fmc, FS, tt2, tt3, coherence=what)
        with pytest.raises(ValueError, match="envelope"):
            rtus.tfm_views(fmc, FS, {"L": tt3}, ("L-L",), coherence=what)
        with pytest.raises(ValueError, match="exclusive"):
            rtus.tfm_views(fmc, FS, {"L": tt3}, ("L-L",), envelope=True, coherence=what, amplitudes={"L": (None, None)})


def test_kernel_resources_of_the_phase_kernel():
    """rtus_tfm.hip compiled device-only to assembly with the Makefile's flags; every rtus_tfm_phase_kernel instantiation: no
    scratch, no spilled VGPR (64 KB of LDS allow two workgroups per CU: up to 128 VGPRs cost no occupancy).  Metadata only."""
    import re
    import subprocess
    import tempfile
    csrc = os.path.join(ROOT, "ray-tracing-ultrasound_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS\s*:=\s*(.*)$", mk, flags=re.M).group(1).replace("$(ARCH)", "gfx950").split()
    res, name = {}, None
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "rtus_tfm.s")
        subprocess.run(["/opt/rocm/bin/hipcc"] + flags + ["--cuda-device-only", "-S", os.path.join(csrc, "rtus_tfm.hip"), "-o", out],
                       check=True, capture_output=True, timeout=600)
        for ln in open(out):
            ln = ln.strip()
            if ln.startswith(".name:"):
                name = ln.split()[1]
            for key in (".vgpr_count:", ".vgpr_spill_count:", ".private_segment_fixed_size:"):
                if ln.startswith(key) and name:
                    res.setdefault(name, {})[key] = int(ln.split()[1])
    phase = {k: v for k, v in res.items() if "rtus_tfm_phase_kernel" in k}
    assert len(phase) == 4, sorted(res)                              # {phasors or not} x {signs or not}
    for k, v in phase.items():
        assert v[".private_segment_fixed_size:"] == 0 and v[".vgpr_spill_count:"] == 0 and v[".vgpr_count:"] <= 128, (k, v)

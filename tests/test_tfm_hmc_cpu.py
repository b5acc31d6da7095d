"""CPU: half-matrix capture — the packed index, pack / unpack, the triangular oracle (tests/tfm_hmc_numpy.py) against the
full-matrix oracle on the unpacked block, every argument error of the Python layer (raised before the library is called), and the
C ABI's new names.  No GPU call."""
import numpy as np
import pytest

import tfm_analytic_numpy as TA
import tfm_hmc_numpy as TH


def test_hmc_index_is_triu_indices_and_the_closed_formula(rtus):
    for n_e in (1, 2, 5, 17, 64, 70):
        i, j = rtus.hmc_index(n_e)
        ti, tj = np.triu_indices(n_e)
        assert np.array_equal(i, ti) and np.array_equal(j, tj)
        assert i.size == n_e * (n_e + 1) // 2 and np.all(i <= j)
        assert np.array_equal(TH.packed_index(i, j, n_e), np.arange(i.size))
        p = i * n_e - i * (i - 1) // 2 + (j - i)                            # the header's formula
        assert np.array_equal(p, np.arange(i.size))
        for k in range(n_e):                                                # a row's records are contiguous
            assert np.array_equal(np.nonzero(i == k)[0], p[i == k]) and np.all(np.diff(p[i == k]) == 1)
    with pytest.raises(ValueError):
        rtus.hmc_index(0)


@pytest.mark.parametrize("kind", ["real", "complex"])
def test_pack_and_unpack_round_trip(rtus, kind):
    rng = np.random.default_rng(5)
    n_e, n_t = 7, 11
    fmc = rng.standard_normal((n_e, n_e, n_t)).astype(np.float32)
    if kind == "complex":
        fmc = (fmc + 1j * rng.standard_normal(fmc.shape)).astype(np.complex64)
    i, j = np.triu_indices(n_e)
    up = rtus.hmc_pack(fmc)                                                  # mode="upper": the records i <= j as they are
    assert up.shape == (28, n_t) and up.dtype == fmc.dtype and up.flags.c_contiguous
    assert np.array_equal(up, fmc[i, j]) and np.array_equal(rtus.hmc_pack(fmc, mode="upper"), up)
    mean = rtus.hmc_pack(fmc, mode="mean")
    assert mean.dtype == fmc.dtype and np.array_equal(mean, (fmc[i, j] + fmc[j, i]) * np.float32(0.5))
    full = rtus.hmc_unpack(up)
    assert full.shape == fmc.shape and full.dtype == fmc.dtype
    assert np.array_equal(full, full.transpose(1, 0, 2)) and np.array_equal(full[i, j], up)
    for mode in ("upper", "mean"):                                           # a symmetric matrix survives both ways
        assert np.array_equal(rtus.hmc_pack(full, mode=mode), up)
        assert np.array_equal(rtus.hmc_unpack(rtus.hmc_pack(full, mode=mode)), full)
    assert rtus.hmc_pack(fmc.astype(np.float64 if kind == "real" else np.complex128)).dtype == fmc.dtype
    with pytest.raises(ValueError):
        rtus.hmc_pack(fmc, mode="lower")
    with pytest.raises(ValueError):
        rtus.hmc_pack(fmc[:, :5])
    with pytest.raises(ValueError):
        rtus.hmc_unpack(up[:27])                                             # 27 is not a triangular number
    with pytest.raises(ValueError):
        rtus.hmc_unpack(up[0])


def _tables(rng, n_e, n_f, n_t, fs, t0):
    lo, hi = (-12 + 0.5 * t0 * fs) / fs, (n_t / 2 + 12 + 0.5 * t0 * fs) / fs
    t = rng.uniform(lo, hi, (n_e, n_f))
    m = rng.random(t.shape)
    t[m < 0.03] = np.nan
    t[(m >= 0.03) & (m < 0.035)] = 1e3
    t[(m >= 0.035) & (m < 0.037)] = -np.inf
    t[(m >= 0.037) & (m < 0.039)] = np.inf
    t[:, -3:] = np.nan
    return t


@pytest.mark.parametrize("n_e, same", [(1, True), (6, True), (6, False), (19, False)])
def test_triangular_oracle_is_the_full_matrix_oracle_on_the_unpacked_block(rtus, n_e, same):
    """the same sum in another order: 1e-12 of the image maximum, with NaN / +-inf / absurd legs and focal points without a path"""
    rng = np.random.default_rng(40 + n_e)
    n_t, n_f, fs, t0 = 120, 300, 40e6, 1.5e-6
    h = (rng.standard_normal((n_e * (n_e + 1) // 2, n_t)) + 1j * rng.standard_normal((n_e * (n_e + 1) // 2, n_t))).astype(np.complex64)
    tt_tx = _tables(rng, n_e, n_f, n_t, fs, t0)
    tt_rx = None if same else _tables(rng, n_e, n_f, n_t, fs, t0)
    o = TH.tfm_hmc(h, fs, t0, tt_tx, tt_rx)
    ref = TA.tfm_analytic(rtus.hmc_unpack(h), fs, t0, tt_tx, tt_rx)
    top = np.max(np.abs(ref["image"]))
    assert top > 0 and np.max(np.abs(o["image"] - ref["image"])) <= 1e-12 * top
    assert np.array_equal(o["N"], ref["N"]) and np.max(np.abs(o["E"] - ref["E"])) <= 1e-12 * ref["E"].max()
    assert np.array_equal(np.isnan(o["cf"]), np.isnan(ref["cf"])) and np.isnan(o["cf"][-3:]).all() and np.all(o["image"][-3:] == 0)
    fin = ~np.isnan(ref["cf"]) & (ref["E"] >= 1e-12 * ref["E"].max())
    assert np.max(np.abs(o["cf"][fin] - ref["cf"][fin])) <= 1e-9
    assert np.all(o["A"] >= np.abs(o["image"]) * (1 - 1e-12))               # the triangle inequality
    # the real plane alone, and the float32 [..., 2] layout
    re = TH.tfm_hmc(h.real, fs, t0, tt_tx, tt_rx)["image"]
    assert np.max(np.abs(re.imag)) == 0 and np.max(np.abs(re.real - o["image"].real)) <= 1e-12 * top
    f2 = np.ascontiguousarray(h.view(np.float32).reshape(*h.shape, 2))
    assert np.array_equal(TH.tfm_hmc(f2, fs, t0, tt_tx, tt_rx)["image"], o["image"])


def test_value_errors_are_raised_before_the_library_is_called(rtus, monkeypatch):
    from importlib import import_module
    lib_mod = import_module("ray-tracing-ultrasound_amd._lib")

    def no_library():
        raise AssertionError("the library was called")
    monkeypatch.setattr(lib_mod, "lib", no_library)
    n_e, n_t, n_f, fs = 4, 16, 5, 40e6
    h = np.zeros((10, n_t), dtype=np.float32)
    a = np.zeros((10, n_t), dtype=np.complex64)
    tt = np.zeros((n_e, n_f))
    for fn, x in ((rtus.tfm_hmc, h), (rtus.tfm_analytic_hmc, a)):
        with pytest.raises(ValueError):
            fn(x[:9], fs, tt)                                                # 9 records: not a triangular number
        with pytest.raises(ValueError):
            fn(x, fs, tt[:3])                                                # the table's rows are not n_e
        with pytest.raises(ValueError):
            fn(x, fs, tt, np.zeros((n_e + 1, n_f)))                          # nor tt_rx's
        with pytest.raises(ValueError):
            fn(x, fs, tt, np.zeros((n_e, n_f + 1)))                          # the tables' columns differ
        with pytest.raises(ValueError):
            fn(x, fs, tt[0])                                                 # not a table
        with pytest.raises(ValueError):
            fn(x[0], fs, tt)                                                 # not a block
    with pytest.raises(ValueError):
        rtus.tfm_analytic_hmc(h, fs, tt)                                     # a real block is not an analytic one
    with pytest.raises(ValueError):
        rtus.tfm_analytic_hmc(np.zeros((10, n_t, 3), dtype=np.float32), fs, tt)
    for c in ("vcf", "scf"):
        with pytest.raises(ValueError):
            rtus.tfm_analytic_hmc(a, fs, tt, coherence=c)                    # the phase kernel has no HMC form
    with pytest.raises(ValueError):
        rtus.tfm_analytic_hmc(a, fs, tt, coherence="nope")
    with pytest.raises(ValueError):
        rtus.hmc_analytic(h[:9])
    with pytest.raises(ValueError):
        rtus.hmc_analytic(h[0])
    # tfm_views(hmc=True)
    legs = {"L": tt, "T": tt + 1e-6}
    amps = {g: (np.ones((n_e, n_f), np.complex64), np.ones((n_e, n_f), np.complex64)) for g in legs}
    with pytest.raises(ValueError):
        rtus.tfm_views(h, fs, legs, ("L-L",), envelope=True, amplitudes=amps, hmc=True)
    for c in ("vcf", "scf"):
        with pytest.raises(ValueError):
            rtus.tfm_views(h, fs, legs, ("L-L",), envelope=True, coherence=c, hmc=True)
    with pytest.raises(ValueError):
        rtus.tfm_views(h, fs, legs, ("L-LL",), hmc=True)                     # a leg missing from ``legs``
    with pytest.raises(ValueError):
        rtus.tfm_views(h, fs, legs, ("L-L",), coherence=True, hmc=True)      # the coherence factor needs envelope=True
    with pytest.raises(ValueError):
        rtus.tfm_views(h[:9], fs, legs, ("L-T",), hmc=True)                  # the block's own checks, still before any GPU call


def test_abi_version_and_names(rtus):
    import ctypes as C
    L = rtus.lib()
    assert L.rtus_version() >= 118
    proto = {p[0]: p for p in import_module_lib().PROTOTYPES}
    for name in ("rtus_tfm_hmc_dev", "rtus_tfm_hmc", "rtus_tfm_analytic_hmc_dev", "rtus_tfm_analytic_hmc"):
        assert name in proto and proto[name][3] == 118 and hasattr(L, name)
    # bad arguments are status codes, before any HIP call: n_e out of [1, 32768], and the full-matrix entries' own rules
    x = np.zeros(64, dtype=np.float32)
    t = np.zeros(64)
    p, q = x.ctypes.data, t.ctypes.data
    for n_e in (0, -3, 32769):
        assert L.rtus_tfm_hmc(p, n_e, 8, 1.0, 0.0, q, q, 4, p, 0) == -1
        assert L.rtus_tfm_analytic_hmc(p, n_e, 8, 1.0, 0.0, q, q, 4, p, None, 0) == -1
        assert L.rtus_tfm_hmc_dev(p, n_e, 8, 1.0, 0.0, q, q, 4, p, None) == -1
        assert L.rtus_tfm_analytic_hmc_dev(p, n_e, 8, 1.0, 0.0, q, q, 4, p, None, None) == -1
    assert L.rtus_tfm_hmc(None, 2, 8, 1.0, 0.0, q, q, 4, p, 0) == -1
    assert L.rtus_tfm_hmc(p, 2, 1, 1.0, 0.0, q, q, 4, p, 0) == -1            # n_t < 2
    assert L.rtus_tfm_hmc(p, 2, 8, 0.0, 0.0, q, q, 4, p, 0) == -1            # fs
    assert L.rtus_tfm_analytic_hmc(p, 2, (1 << 26) + 1, 1.0, 0.0, q, q, 4, p, None, 0) == -5
    assert C.sizeof(C.c_int) == 4


def import_module_lib():
    from importlib import import_module
    return import_module("ray-tracing-ultrasound_amd._lib")


def test_kernels_use_no_scratch():
    """rtus_tfm_hmc.hip compiled device-only to assembly with the Makefile's flags: the two real and the four analytic kernels keep
    everything in registers (no scratch, no spilled VGPR); 64 KiB of LDS each (two workgroups per CU)"""
    import os
    import re
    import subprocess
    import tempfile
    from conftest import ROOT
    csrc = os.path.join(ROOT, "ray-tracing-ultrasound_amd", "csrc")
    flags = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-fno-fast-math", "-fno-slp-vectorize", "--cuda-device-only", "-S"]
    res = {}
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "rtus_tfm_hmc.s")
        subprocess.run(["/opt/rocm/bin/hipcc"] + flags + [os.path.join(csrc, "rtus_tfm_hmc.hip"), "-o", out], check=True,
                       capture_output=True, timeout=600)
        meta = open(out).read().split("amdhsa.kernels:")[1]
    for entry in re.split(r"^  - ", meta, flags=re.M)[1:]:                  # one list item per kernel; its keys are indented by 4
        kv = dict(re.findall(r"^ {0,4}(\.\w+):\s+(\S+)\s*$", entry, flags=re.M))
        if ".vgpr_count" in kv:
            res[kv[".name"]] = {k: int(kv[k]) for k in (".vgpr_count", ".vgpr_spill_count", ".private_segment_fixed_size",
                                                        ".group_segment_fixed_size")}
    res = {k: v for k, v in res.items() if "hmc_kernel" in k}
    assert len(res) == 6, sorted(res)
    for k, v in res.items():
        assert v[".private_segment_fixed_size"] == 0 and v[".vgpr_spill_count"] == 0, (k, v)
        assert v[".vgpr_count"] <= 256, (k, v)                               # two workgroups per CU: two waves per SIMD
    assert sorted(v[".group_segment_fixed_size"] for v in res.values()) == [65536] * 6

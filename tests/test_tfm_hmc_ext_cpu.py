"""CPU: the NumPy definitions of rtus_tfm_phase_hmc and rtus_tfm_weighted_hmc (tests/tfm_hmc_ext_numpy.py) against the full-matrix
definitions of tests/das_exact_numpy.py on the unpacked capture — exact data, no tolerance — the width of the widest partial sum, the
bar of vcf for the GPU test, the argument checks of the two Python wrappers, and the C entries' table.  No GPU."""
import numpy as np
import pytest

import das_exact_numpy as D
import tfm_hmc_ext_numpy as X

CASES = [(n_e, two) for n_e in D.HMC_SIZES for two in (False, True)]


def _unpack(h, n_e):
    i, j = np.triu_indices(n_e)
    full = np.empty((n_e, n_e, h.shape[1]), dtype=h.dtype)
    full[i, j] = h
    full[j, i] = h
    return full


@pytest.mark.parametrize("n_e,two", CASES)
@pytest.mark.parametrize("two_w", [False, True])
def test_the_packed_walk_is_the_full_matrix_on_exact_data(n_e, two, two_w):
    """S, S_w (both rules), P, B, N and scf of the packed model equal the full-matrix model on the unpacked capture with no tolerance;
    the model asserts on the way that nothing rounds (every product, W_ij + W_ji, every partial sum in the kernel's order)"""
    c, m = X.exact_case(n_e, two, two_w), X.exact_model(n_e, two, two_w)
    for w in (c["w_tx"], c["w_rx"]):
        if w is not None and n_e > 1:
            assert np.isnan(w.real).any() and np.isinf(w.real).any()     # some legs carry NaN / infinite weights
    full = D.tfm(_unpack(c["h"], n_e), c["fs"], c["t0"], c["tt_tx"], c["tt_rx"], c["w_tx"], c["w_rx"])
    assert np.array_equal(m["S"], full["S"]) and np.array_equal(m["S"], D.hmc_model(n_e, two)["S"])
    assert np.array_equal(m["S_w"], full["S_w"]) and np.array_equal(m["P"], full["P"])
    if not two:
        assert np.array_equal(m["S_w1"], full["S_w"])                    # one gather, the weights' sum first: the same number
    else:
        assert "S_w1" not in m
    assert np.array_equal(m["B"], full["B"]) and np.array_equal(m["N"], full["N"])
    assert np.array_equal(m["T"], full["T"]) and np.array_equal(m["R"], full["R"])
    assert np.array_equal(m["scf"], D.scf_header(full["B"], full["N"]), equal_nan=True)
    assert np.max(np.abs(m["U"] - full["U"])) <= 1e-9                    # (fp64 sums of irrational phasors in two orders)
    col = c["cols"]["no_path"]
    assert m["N"][col] == 0 and m["S_w"][col] == 0 and m["P"][col] == 0 and np.isnan(m["scf"][col])
    print(f"n_e = {n_e}, {'two' if two else 'one'} delay table(s), {'two' if two_w else 'one'} weight table(s): "
          f"the widest partial sum needs {m['widest']} bits")
    assert m["widest"] <= 24


def test_the_kernel_order_visits_every_record_once():
    for n_e in D.HMC_SIZES:
        o = X.order(n_e)
        i, j = np.triu_indices(n_e)
        blocks = j[o] // X.GROUP
        assert np.all(np.diff(blocks) >= 0)                              # column blocks ascending
    assert list(X.order(3)) == [0, 1, 2, 3, 4, 5] and X.order(17)[-1] == 17 * 18 // 2 - 1
    o = X.order(17)
    assert list(o[136:152]) == [D.packed_index(i, 16, 17) for i in range(16)]   # the rows above the second block


def test_the_bar_of_vcf():
    """the float32 sum of the phasors in the kernel's order against their fp64 sum, every exact case with n_e^2 <= 4900: the largest
    |vcf32 - vcf|; X.VCF_BAR is 4 x that (to the two digits it is written with) and far below the hard cap"""
    worst, where = 0.0, None
    for n_e in X.VCF_SIZES:
        for two in (False, True):
            m = X.exact_model(n_e, two, False)
            assert m["N"].max() <= 4900
            fin = m["N"] > 0
            assert np.array_equal(np.isnan(m["vcf32"]), ~fin)
            err = float(np.max(np.abs(m["vcf32"][fin] - m["vcf"][fin]))) if fin.any() else 0.0
            print(f"n_e = {n_e}, {'two tables' if two else 'one table'}: largest |vcf32 - vcf| = {err:.3e}")
            if err > worst:
                worst, where = err, (n_e, two)
    print(f"largest {worst:.3e} at {where}; 4 x = {4 * worst:.3e}; VCF_BAR = {X.VCF_BAR:.1e}; cap {X.VCF_CAP:.2e}")
    assert 81 not in X.VCF_SIZES and set(X.VCF_SIZES) == set(D.HMC_SIZES) - {81}
    assert abs(X.VCF_BAR - 4 * worst) <= 0.02 * X.VCF_BAR
    assert X.VCF_BAR < X.VCF_CAP


def test_random_data_model_agrees_with_the_phase_oracle():
    """exact=False: the samples are tests/tfm_phase_numpy.py's fp32 samples of the unpacked capture, pair by pair, so B and N are its
    B and N — the consequence the header states for the kernels"""
    import tfm_phase_numpy as TP
    rng = np.random.default_rng(3)
    n_e, n_t, n_f, fs, t0 = 9, 40, 61, 40e6, 1.5e-6
    h = (rng.standard_normal((n_e * (n_e + 1) // 2, n_t)) + 1j * rng.standard_normal((n_e * (n_e + 1) // 2, n_t))).astype(np.complex64)
    lo, hi = (-6 + 0.5 * t0 * fs) / fs, (n_t / 2 + 6 + 0.5 * t0 * fs) / fs
    tt_a, tt_b = rng.uniform(lo, hi, (n_e, n_f)), rng.uniform(lo, hi, (n_e, n_f))
    tt_a[rng.random(tt_a.shape) < 0.05] = np.nan
    for tt_rx in (None, tt_b):
        m = X.walk(h, fs, t0, tt_a, tt_rx, exact=False)
        o = TP.tfm_phase(_unpack(h, n_e), fs, t0, tt_a, tt_rx, fp32=True)
        assert np.array_equal(m["B"], o["B"]) and np.array_equal(m["N"], o["N"])
        assert np.allclose(m["vcf"], o["vcf"], rtol=0, atol=1e-12, equal_nan=True)


def test_value_errors_are_raised_before_the_library_is_called(rtus, monkeypatch):
    from importlib import import_module
    lib_mod = import_module("ray-tracing-ultrasound_amd._lib")

    def no_library():
        raise AssertionError("the library was called")
    monkeypatch.setattr(lib_mod, "lib", no_library)
    n_e, n_t, n_f, fs = 4, 16, 5, 40e6
    a = np.zeros((10, n_t), dtype=np.complex64)
    tt = np.zeros((n_e, n_f))
    w = np.ones((n_e, n_f), dtype=np.complex64)
    phase = lambda x, *t, **k: rtus.tfm_phase_hmc(x, fs, *t, **k)
    weighted = lambda x, *t, **k: rtus.tfm_weighted_hmc(x, fs, t[0], w, *t[1:], **k)
    for fn in (phase, weighted):
        bad = [
            lambda: fn(a.real.astype(np.float32), tt),                   # a real block is not an analytic one
            lambda: fn(np.zeros((10, n_t, 3), dtype=np.float32), tt),
            lambda: fn(a[:9], tt),                                       # 9 records: not a triangular number
            lambda: fn(a[0], tt),
            lambda: fn(a, tt[:3]),                                       # the table's rows are not n_e
            lambda: fn(a, tt[0]),
            lambda: fn(a, tt, np.zeros((n_e, n_f + 1))),                 # the tables' columns differ
            lambda: fn(a, tt, np.zeros((n_e + 1, n_f))),
            lambda: fn(a, tt, out=np.zeros(n_f + 1, dtype=np.complex64)),
            lambda: fn(a, tt, out=np.zeros(n_f, dtype=np.complex128)),
        ]
        for k, call in enumerate(bad):
            with pytest.raises(ValueError):
                call()
                pytest.fail(f"case {k} did not raise")
    for bad_w in (np.ones((n_e, n_f), dtype=np.float32),                 # weights are complex
                  np.ones((n_e, n_f), dtype=np.float64),
                  np.ones((n_e, n_f), dtype=np.int32),
                  np.ones((n_e + 1, n_f), dtype=np.complex64),
                  np.ones((n_e, n_f - 1), dtype=np.complex64),
                  np.ones((n_e, n_f, 2), dtype=np.float32),
                  np.ones(n_e * n_f, dtype=np.complex64)):
        with pytest.raises(ValueError):
            rtus.tfm_weighted_hmc(a, fs, tt, bad_w)
        with pytest.raises(ValueError):
            rtus.tfm_weighted_hmc(a, fs, tt, w, tt.copy(), bad_w)
        with pytest.raises(ValueError):
            rtus.tfm_weighted_hmc(a, fs, tt, w, None, bad_w)
    # a well-formed call reaches the library
    for call in (lambda: rtus.tfm_phase_hmc(a, fs, tt), lambda: rtus.tfm_weighted_hmc(a, fs, tt, w),
                 lambda: rtus.tfm_weighted_hmc(np.zeros((10, n_t, 2), dtype=np.float32), fs, tt, w.astype(np.complex128), tt, w)):
        with pytest.raises(AssertionError, match="the library was called"):
            call()


def test_one_table_means_one_pointer(rtus, monkeypatch):
    """tt_rx=None or the same object reach the C entry as ONE pointer (the one-table kernel); an equal copy as two; w_rx=None as
    w_tx's pointer"""
    from importlib import import_module
    lib_mod = import_module("ray-tracing-ultrasound_amd._lib")
    seen = []

    class Fake:
        def rtus_tfm_phase_hmc(self, a, n_e, n_t, fs, t0, tx, rx, n_f, *rest):
            seen.append(("phase", n_e, n_t, n_f, tx == rx))
            return 0

        def rtus_tfm_weighted_hmc(self, a, n_e, n_t, fs, t0, tx, rx, wt, wr, n_f, *rest):
            seen.append(("weighted", n_e, n_t, n_f, tx == rx, wt == wr))
            return 0
    monkeypatch.setattr(lib_mod, "lib", lambda: Fake())
    a = np.zeros((10, 16), dtype=np.complex64)
    tt, w = np.zeros((4, 5)), np.ones((4, 5), dtype=np.complex64)
    r = rtus.tfm_phase_hmc(a, 40e6, tt)
    assert set(r) == {"image", "vcf", "scf"} and r["image"].dtype == np.complex64 and r["image"].shape == (5,)
    assert r["vcf"].dtype == r["scf"].dtype == np.float32 and r["vcf"].shape == r["scf"].shape == (5,)
    r = rtus.tfm_phase_hmc(a, 40e6, tt, tt, counts=True)
    assert set(r) == {"image", "vcf", "scf", "sign_sum", "n_pairs"} and r["sign_sum"].dtype == r["n_pairs"].dtype == np.int32
    rtus.tfm_phase_hmc(a, 40e6, tt, tt.copy())
    assert seen == [("phase", 4, 16, 5, True), ("phase", 4, 16, 5, True), ("phase", 4, 16, 5, False)]
    del seen[:]
    img = rtus.tfm_weighted_hmc(a, 40e6, tt, w)
    assert img.dtype == np.complex64 and img.shape == (5,)
    img, sens = rtus.tfm_weighted_hmc(a, 40e6, tt, w, tt, w.copy(), sensitivity=True)
    assert sens.dtype == np.float32 and sens.shape == (5,)
    out = np.zeros(5, dtype=np.complex64)
    assert rtus.tfm_weighted_hmc(a, 40e6, tt, w, tt.copy(), out=out) is out
    assert seen == [("weighted", 4, 16, 5, True, True), ("weighted", 4, 16, 5, True, False), ("weighted", 4, 16, 5, False, True)]


def test_the_c_entries_are_declared_and_exported(rtus):
    from importlib import import_module
    lib_mod = import_module("ray-tracing-ultrasound_amd._lib")
    names = ("rtus_tfm_phase_hmc_dev", "rtus_tfm_phase_hmc", "rtus_tfm_weighted_hmc_dev", "rtus_tfm_weighted_hmc")
    L = rtus.lib()
    assert L.rtus_version() >= 124
    assert [n for n, _, _, since in lib_mod.PROTOTYPES if since == 124] == list(names)
    for n in names:
        assert hasattr(L, n) and n in rtus.EXPORTS
    for n in ("tfm_phase_hmc", "tfm_weighted_hmc"):
        assert n in rtus.__all__ and callable(getattr(rtus, n))
    # invalid arguments and limits come back before any HIP call (no GPU here)
    a = np.zeros((3, 8, 2), dtype=np.float32)
    tt = np.zeros((2, 4))
    w = np.zeros((2, 4, 2), dtype=np.float32)
    img = np.zeros((4, 2), dtype=np.float32)
    p = lambda x: None if x is None else x.ctypes.data
    assert L.rtus_tfm_phase_hmc(p(a), 0, 8, 40e6, 0.0, p(tt), p(tt), 4, p(img), None, None, None, 0) == -1
    assert L.rtus_tfm_phase_hmc(p(a), 32769, 8, 40e6, 0.0, p(tt), p(tt), 4, p(img), None, None, None, 0) == -1
    assert L.rtus_tfm_phase_hmc(p(a), 2, 8, 40e6, 0.0, p(tt), p(tt), 4, None, None, None, None, 0) == -1
    assert L.rtus_tfm_phase_hmc(p(a), 2, 2 ** 26 + 1, 40e6, 0.0, p(tt), p(tt), 4, p(img), None, None, None, 0) == -5
    assert L.rtus_tfm_phase_hmc_dev(p(a), 2, 1, 40e6, 0.0, p(tt), p(tt), 4, p(img), None, None, None, None) == -1
    assert L.rtus_tfm_weighted_hmc(p(a), 2, 8, 40e6, 0.0, p(tt), p(tt), None, p(w), 4, p(img), None, 0) == -1
    assert L.rtus_tfm_weighted_hmc(p(a), 2, 8, 40e6, 0.0, p(tt), p(tt), p(w), None, 4, p(img), None, 0) == -1
    assert L.rtus_tfm_weighted_hmc(p(a), 0, 8, 40e6, 0.0, p(tt), p(tt), p(w), p(w), 4, p(img), None, 0) == -1
    assert L.rtus_tfm_weighted_hmc(p(a), 2, 2 ** 26 + 1, 40e6, 0.0, p(tt), p(tt), p(w), p(w), 4, p(img), None, 0) == -5
    assert L.rtus_tfm_weighted_hmc_dev(p(a), 2, 8, 40e6, 0.0, None, p(tt), p(w), p(w), 4, p(img), None, None) == -1


def test_the_new_kernels_use_no_scratch():
    """rtus_tfm_hmc.hip compiled device-only to assembly with the Makefile's flags: the eight phase and the four weighted kernels have
    no private segment; the phase kernels keep the family's 64 KiB of LDS and at most 256 VGPRs (two workgroups per CU), the weighted
    ones hold one column block of delays and weights: 80 KiB with one delay table, 96 KiB with two (one workgroup per CU)"""
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
            res[kv[".name"]] = {k: int(kv[k]) for k in (".vgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")}
    phase = {k: v for k, v in res.items() if "hmc_phase_kernel" in k}
    weighted = {k: v for k, v in res.items() if "hmc_weighted_kernel" in k}
    assert len(phase) == 8 and len(weighted) == 4, sorted(res)
    for k, v in {**phase, **weighted}.items():
        assert v[".private_segment_fixed_size"] == 0, (k, v)
        print(k, v)
    for k, v in phase.items():
        assert v[".group_segment_fixed_size"] == 65536 and v[".vgpr_count"] <= 256, (k, v)
    assert sorted(v[".group_segment_fixed_size"] for v in weighted.values()) == [81920, 81920, 98304, 98304]

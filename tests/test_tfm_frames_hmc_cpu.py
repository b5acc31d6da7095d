"""CPU: the plumbing of TFM over a stack of half-matrix frames (include/rtus.h: rtus_tfm_frames_hmc_i16, rtus_tfm_frames_hmc): the
exports, the header and the version, the status code of every bad argument through ctypes (the checks run before any HIP call), the
Python errors of tfm_frames(hmc=True) raised before any library call, the documented identity of the packed layouts, and the exact
model's own consistency on the record sets that tests/test_gpu_tfm_frames_hmc.py images.  No GPU touched."""
import os
import re

import numpy as np
import pytest

import das_exact_numpy as D
from conftest import ROOT

NAMES = ("rtus_tfm_frames_hmc_i16_dev", "rtus_tfm_frames_hmc_i16", "rtus_tfm_frames_hmc_dev", "rtus_tfm_frames_hmc")
N_SETS = 5                                                               # complex record sets: ten frames
_sets = {}


def record_sets(n_e):
    """five complex record sets [5, n_pairs, N_T] of integers in [-4, 4] for a capture of n_e elements: the real and the imaginary
    plane of set k are frames 2 k and 2 k + 1 of the stacks of the GPU test"""
    if n_e not in _sets:
        a = D.records(np.random.default_rng(500 + n_e), (N_SETS, n_e * (n_e + 1) // 2, D.N_T))
        a.flags.writeable = False
        _sets[n_e] = a
    return _sets[n_e]


def test_exports_header_version_and_status_codes(rtus):
    from importlib import import_module
    L = rtus.lib()
    assert L.rtus_version() >= 123
    header = open(os.path.join(ROOT, "include", "rtus.h")).read()
    for name in NAMES:
        assert name in rtus.EXPORTS and hasattr(L, name)
        assert len(re.findall(r"^int %s\(" % name, header, flags=re.M)) == 1, name     # declared once
    lib_mod = import_module("ray-tracing-ultrasound_amd._lib")
    assert [n for n, _, _, since in lib_mod.PROTOTYPES if since == 123] == list(NAMES)
    assert "tfm_frames" in rtus.__all__
    dev = import_module("ray-tracing-ultrasound_amd.device")
    assert all(callable(getattr(dev, n)) for n in ("tfm_frames_hmc_i16_dev", "tfm_frames_hmc_dev"))

    buf = np.zeros(4096)
    p = buf.ctypes.data
    big = 0x7fffffff
    # (data, n_frames, n_e, n_t, fs, t0, tt_tx, tt_rx, n_f, images, stream | device): test_tfm_frames_i16_cpu.py's calls, n_e for
    # (n_tx, n_rx); per: frames per block of the packed stack
    base = dict(d=p, f=3, e=2, t=8, fs=1.0e6, t0=0.0, ttx=p, trx=p, nf=4, img=p)
    for i16, per in ((True, 4), (False, 2)):
        fn_dev, fn_host = (L.rtus_tfm_frames_hmc_i16_dev, L.rtus_tfm_frames_hmc_i16) if i16 else (L.rtus_tfm_frames_hmc_dev, L.rtus_tfm_frames_hmc)

        def call(dev, **kw):
            a = {**base, **kw}
            args = (a["d"], a["f"], a["e"], a["t"], a["fs"], a["t0"], a["ttx"], a["trx"], a["nf"], a["img"])
            return fn_dev(*args, None) if dev else fn_host(*args, 0)
        for dev in (False, True):
            for name in ("d", "ttx", "trx", "img"):
                assert call(dev, **{name: None}) == -1, name
            for name in ("f", "e", "t", "nf"):
                assert call(dev, **{name: 0}) == -1 and call(dev, **{name: -4}) == -1, name
            assert call(dev, e=32769) == -1                                      # n_e (n_e + 1) / 2 must fit an int
            assert call(dev, t=1) == -1                                          # rtus_tfm's: two samples at least
            for fs in (0.0, -1.0, np.inf, np.nan):
                assert call(dev, fs=fs) == -1, fs
            for t0 in (np.inf, np.nan):
                assert call(dev, t0=t0) == -1, t0
            assert call(dev, t=(1 << 26) + 1) == -5                              # 8-byte positions, 32-bit byte offsets
            assert call(dev, t=(1 << 26) + 1, img=None) == -1                    # invalid before unsupported
            # the workgroup count: ceil(n_f / 256) per block of `per` frames, 2^31 - 1 at the most
            assert call(dev, f=256 * per, nf=big) == -5 and call(dev, f=256 * per - per + 1, nf=big) == -5   # 256 blocks x 2^23 = 2^31
            assert call(dev, f=1 << 22, nf=1 << 20) == -5
            assert call(dev, f=1 << 22, nf=1 << 20, d=None) == -1


def test_python_errors_of_hmc_stacks_before_any_library_call(rtus, monkeypatch):
    from importlib import import_module
    api = import_module("ray-tracing-ultrasound_amd.api")

    def no_library():
        raise AssertionError("the library was called")
    monkeypatch.setattr(api._lib, "lib", no_library)
    tt = np.zeros((3, 5))
    for dtype in (np.int16, np.float32, np.float64):
        stack = np.zeros((5, 6, 16), dtype=dtype)                                # five frames of a 3-element capture
        good = dict(stack=stack, fs=1.0e6, tt_tx=tt, hmc=True)
        for kw in (dict(stack=np.zeros((5, 7, 16), dtype=dtype)),                # 7 is not a triangular number
                   dict(tt_tx=np.zeros((4, 5))), dict(tt_tx=np.zeros((2, 5))), dict(tt_rx=np.zeros((4, 5))), dict(tt_rx=np.zeros((3, 6))),
                   dict(tt_tx=tt[0]),
                   dict(envelope=True), dict(coherence=True), dict(coherence="cf"), dict(f_demod=1.0e5),
                   dict(envelope=True, coherence=True), dict(envelope=True, f_demod=1.0e5),
                   dict(stack=np.zeros((5, 1, 6, 16), dtype=dtype)),              # a 4-D stack is a full-matrix stack
                   dict(stack=stack[0]), dict(stack=stack[:0]),
                   dict(max_frames=0), dict(max_frames=1.5), dict(max_frames=True),
                   dict(out=np.zeros((5, 5))), dict(out=np.zeros((4, 5), dtype=np.float32))):
            with pytest.raises(ValueError):
                rtus.tfm_frames(**{**good, **kw})
            # (kw is reported by pytest's traceback when the call does not raise)
        with pytest.raises(ValueError, match="tfm_analytic_hmc"):
            rtus.tfm_frames(**{**good, "envelope": True})
        for kw in (dict(), dict(tt_rx=tt), dict(tt_rx=tt.copy()), dict(max_frames=2)):
            with pytest.raises(AssertionError, match="the library was called"):  # a good call gets as far as the library
                rtus.tfm_frames(**{**good, **kw})
    # hmc=False is the call as it was: a 3-D stack is refused, a 4-D one goes through
    with pytest.raises(ValueError):
        rtus.tfm_frames(np.zeros((5, 6, 16), dtype=np.int16), 1.0e6, tt)
    with pytest.raises(AssertionError, match="the library was called"):
        rtus.tfm_frames(np.zeros((5, 3, 3, 16), dtype=np.int16), 1.0e6, tt, hmc=False)


@pytest.mark.parametrize("n_frames", [1, 2, 3, 4, 5, 9])
def test_the_packed_layouts_are_the_full_matrix_packs_of_one_transmit_row(rtus, n_frames):
    """frames_pack_i16(stack[:, None])[:, 0] is [n_quads, n_pairs, n_t, 4] with frame 4 q + c in plane c of quad q and zero planes for
    the absent frames; frames_pack(stack[:, None])[:, 0] the same in pairs"""
    rng = np.random.default_rng(n_frames)
    n_pairs, n_t = 6, 7
    stack = rng.integers(-32768, 32768, (n_frames, n_pairs, n_t)).astype(np.int16)
    stack[stack == 0] = 1                                                        # a zero plane is then an absent frame's
    for pack, per, s in ((rtus.frames_pack_i16, 4, stack), (rtus.frames_pack, 2, stack.astype(np.float32))):
        packed = pack(s[:, None])[:, 0]
        n_blocks = (n_frames + per - 1) // per
        assert packed.dtype == s.dtype and packed.shape == (n_blocks, n_pairs, n_t, per)
        assert np.ascontiguousarray(packed).tobytes() == pack(s[:, None]).tobytes()     # the same bytes: one transmit row
        for k in range(n_frames):
            assert np.array_equal(packed[k // per, ..., k % per], s[k])
        for k in range(n_frames, per * n_blocks):
            assert np.all(packed[k // per, ..., k % per] == 0) and not np.signbit(packed[k // per, ..., k % per].astype(np.float32)).any()


@pytest.mark.parametrize("two", [False, True], ids=["one_table", "two_tables"])
@pytest.mark.parametrize("n_e", D.HMC_SIZES)
def test_exact_model_of_a_plane_is_the_full_matrix_model_of_its_unpacked_plane(rtus, n_e, two):
    """das_exact_numpy.tfm_hmc on a plane of the generated record sets == das_exact_numpy.tfm on hmc_unpack of it: every term is
    exact (_exact32 asserts it), so the order of the sums does not matter.  Both planes of every set through the models' complex
    form (the planes never meet in S)."""
    c = D.hmc_case(n_e, two)
    a = record_sets(n_e)
    for k in range(N_SETS):
        half = D.tfm_hmc(a[k], c["fs"], c["t0"], c["tt_tx"], c["tt_rx"])["S"]
        full = D.tfm(rtus.hmc_unpack(a[k]), c["fs"], c["t0"], c["tt_tx"], c["tt_rx"])["S"]
        assert np.array_equal(half, full), (n_e, two, k)
        assert np.count_nonzero(half.real) > 0.5 * half.size or n_e == 1
    plane = np.ascontiguousarray(a[0].real)                                      # and a plane by itself, as a real block
    alone = D.tfm_hmc(plane, c["fs"], c["t0"], c["tt_tx"], c["tt_rx"])["S"]
    assert np.array_equal(alone.real, D.tfm_hmc(a[0], c["fs"], c["t0"], c["tt_tx"], c["tt_rx"])["S"].real) and not alone.imag.any()

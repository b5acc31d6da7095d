"""No GPU: envelope TFM over half-matrix frame stacks (include/rtus.h: rtus_tfm_envelope_frames_hmc[_i16][_dev],
rtus_fmc_analytic_i16[_dev], rtus_fmc_hilbert_pairs_i16_dev; api.tfm_envelope_frames) — the exports, every limit and workspace
error of the C entries (all returned before any HIP call, so they are the same without a device), the Python errors, and the two
definitions that are NumPy: the pair-packed Hilbert layout and the magnitude."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT

NEW = ("rtus_fmc_analytic_i16_dev", "rtus_fmc_analytic_i16", "rtus_fmc_hilbert_pairs_i16_dev",
       "rtus_tfm_envelope_frames_hmc_workspace_bytes", "rtus_tfm_envelope_frames_hmc_i16_dev", "rtus_tfm_envelope_frames_hmc_i16",
       "rtus_tfm_envelope_frames_hmc_dev", "rtus_tfm_envelope_frames_hmc")
FS = 40.0e6


def test_exports_header_and_version(rtus):
    from importlib import import_module
    lib_mod = import_module("ray-tracing-ultrasound_amd._lib")
    L = rtus.lib()
    assert L.rtus_version() >= 125
    assert [n for n, _, _, since in lib_mod.PROTOTYPES if since == 125] == list(NEW)
    hdr = open(os.path.join(ROOT, "include", "rtus.h")).read()
    code = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    for name in NEW:
        assert hasattr(L, name), name
        assert len(re.findall(r"\b%s\s*\(" % name, code)) == 1, f"{name} is declared once"
    assert re.search(r"#define\s+RTUS_ENV_MAGNITUDE\s+1\b", hdr)
    for name in ("tfm_envelope_frames", "fmc_analytic_i16"):
        assert name in rtus.__all__ and callable(getattr(rtus, name))


def hilbert_pairs(analytic_stack):
    """The pair-packed Hilbert planes, restated in NumPy: complex64 [n_frames, n_scans, n_t] (fmc_analytic's of each frame) -> float32
    [n_fpairs, n_scans, n_t, 2]; plane c of pair p is the imaginary part of frame 2 p + c, the absent frame of an odd stack +0.0.  The
    layout rtus_fmc_hilbert_pairs_i16_dev writes and rtus_tfm_frames_hmc_dev reads (include/rtus.h)."""
    a = np.asarray(analytic_stack, dtype=np.complex64)
    assert a.ndim == 3 and a.shape[0] >= 1
    n_frames = a.shape[0]
    packed = np.zeros(((n_frames + 1) // 2,) + a.shape[1:] + (2,), dtype=np.float32)
    for k in range(n_frames):
        packed[k // 2, :, :, k % 2] = a[k].imag
    return packed


def envelope_magnitude(images):
    """RTUS_ENV_MAGNITUDE's definition (include/rtus.h) on complex64 images -> float32: the squares exact in float64, their sum
    rounded once, a correctly rounded float64 sqrt, one rounding to float32."""
    images = np.asarray(images, dtype=np.complex64)
    with np.errstate(over="ignore", invalid="ignore"):
        return np.sqrt(images.real.astype(np.float64) ** 2 + images.imag.astype(np.float64) ** 2).astype(np.float32)


class _Bufs:
    """addresses that pass every pointer check; no entry dereferences them before its checks are through"""
    def __init__(self):
        self.keep = np.zeros(4096, dtype=np.uint8)
        base = self.keep.ctypes.data
        self.p = (base + 63) & ~63                                       # 64-byte aligned, 4032 bytes behind it


def _env_args(b, **kw):
    """a call of the envelope _dev entries that passes every check: 5 frames of a 3-element capture"""
    a = dict(hmc=b.p, n_frames=5, n_e=3, n_t=300, n_taps=63, fs=FS, t0=0.0, f_demod=0.0, tx=b.p, rx=b.p, n_f=600, flags=0, images=b.p,
             cf=None, work=b.p, work_bytes=1 << 40, stream=None)
    a.update(kw)
    return a


def _dev_call(fn, a):
    return fn(a["hmc"], a["n_frames"], a["n_e"], a["n_t"], a["n_taps"], a["fs"], a["t0"], a["f_demod"], a["tx"], a["rx"], a["n_f"],
              a["flags"], a["images"], a["cf"], a["work"], a["work_bytes"], a["stream"])


def _host_call(fn, a):
    return fn(a["hmc"], a["n_frames"], a["n_e"], a["n_t"], a["n_taps"], a["fs"], a["t0"], a["f_demod"], a["tx"], a["rx"], a["n_f"],
              a["flags"], a["images"], a["cf"], 0)


BAD = [
    (dict(hmc=None), -1), (dict(tx=None), -1), (dict(rx=None), -1), (dict(images=None), -1),
    (dict(n_frames=0), -1), (dict(n_e=0), -1), (dict(n_e=32769), -1), (dict(n_t=1), -1), (dict(n_f=0), -1),
    (dict(n_taps=62), -1), (dict(n_taps=1), -1), (dict(n_taps=257), -1), (dict(n_taps=-3), -1),
    (dict(f_demod=-1.0), -1), (dict(f_demod=0.5 * FS), -1), (dict(f_demod=float("nan")), -1), (dict(f_demod=float("inf")), -1),
    (dict(fs=0.0), -1), (dict(fs=float("inf")), -1), (dict(t0=float("nan")), -1), (dict(flags=2), -1), (dict(flags=-1), -1),
    (dict(n_t=(1 << 26) + 1), -5),                                       # a record past the 32-bit byte offsets
    (dict(n_frames=1 << 22, n_f=1 << 30), -5),                           # 2^22 frames of 2^22 workgroups: no grid holds them
    (dict(n_frames=1 << 30, n_e=64), -5),                                # 2^30 x 2080 A-scans: the transformer's grid
]


@pytest.mark.parametrize("i16", [True, False], ids=["int16", "float32"])
def test_every_limit_is_a_status_before_any_hip_call(rtus, i16):
    L, b = rtus.lib(), _Bufs()
    dev = L.rtus_tfm_envelope_frames_hmc_i16_dev if i16 else L.rtus_tfm_envelope_frames_hmc_dev
    host = L.rtus_tfm_envelope_frames_hmc_i16 if i16 else L.rtus_tfm_envelope_frames_hmc
    for change, status in BAD:
        for extra in (dict(), dict(cf=b.p), dict(flags=1) if "flags" not in change else dict()):
            a = _env_args(b, **{**extra, **change})
            assert _dev_call(dev, a) == status, (change, extra)
            assert _host_call(host, a) == status, (change, extra)
    # misaligned pointers: the complex images are stored 8 bytes at a time, the float32 stack read 4 at a time, int16 2 at a time
    assert _dev_call(dev, _env_args(b, images=b.p + 4)) == -1
    assert _dev_call(dev, _env_args(b, images=b.p + 4, flags=1, work=None)) == -4          # (magnitude rows: 4-byte stores)
    assert _dev_call(dev, _env_args(b, hmc=b.p + 1)) == -1
    # the workspace: null, misaligned, one byte short — after every other check, before any HIP call
    for kw in (dict(), dict(cf=b.p), dict(flags=1), dict(f_demod=5.0e6)):
        a = _env_args(b, **kw)
        need = L.rtus_tfm_envelope_frames_hmc_workspace_bytes(a["n_frames"], a["n_e"], a["n_t"], a["n_f"], int(i16), a["f_demod"],
                                                              int(a["cf"] is not None), a["flags"])
        assert need > 0
        assert _dev_call(dev, {**a, "work": None}) == -4
        assert _dev_call(dev, {**a, "work": b.p + 32}) == -4
        assert _dev_call(dev, {**a, "work_bytes": need - 1}) == -4
        assert _dev_call(dev, {**a, "work_bytes": 0}) == -4


def test_workspace_bytes(rtus):
    size = rtus.lib().rtus_tfm_envelope_frames_hmc_workspace_bytes
    al = lambda n: (n + 255) & ~255                                      # noqa: E731
    n_pairs, n_t, n_f = 6, 300, 600
    for n in (1, 2, 3, 4, 5, 9):
        split = al(((n + 3) // 4) * 8 * n_pairs * n_t) + al(((n + 1) // 2) * 8 * n_pairs * n_t) + 2 * al(4 * n * n_f)
        cplx = al(8 * n_pairs * n_t)                                     # one frame's analytic block, reused
        assert size(n, 3, n_t, n_f, 1, 0.0, 0, 0) == split == size(n, 3, n_t, n_f, 1, 0.0, 0, 1)
        assert size(n, 3, n_t, n_f, 1, 0.0, 1, 0) == cplx == size(n, 3, n_t, n_f, 1, 5.0e6, 0, 0) == size(n, 3, n_t, n_f, 0, 0.0, 0, 0)
        assert size(n, 3, n_t, n_f, 0, 0.0, 0, 1) == cplx + al(8 * n * n_f) == size(n, 3, n_t, n_f, 1, 0.0, 1, 1)
    for bad in ((0, 3, n_t, n_f), (-1, 3, n_t, n_f), (5, 0, n_t, n_f), (5, 32769, n_t, n_f), (5, 3, 0, n_f), (5, 3, n_t, 0)):
        for i16 in (0, 1):
            assert size(*bad, i16, 0.0, 0, 0) == 0, bad
    assert size(5, 3, n_t, n_f, 1, 0.0, 0, 2) == 0 and size(5, 3, n_t, n_f, 1, -1.0, 0, 0) == 0
    assert size(5, 3, n_t, n_f, 1, float("nan"), 0, 0) == 0 and size(5, 3, n_t, n_f, 1, float("inf"), 0, 0) == 0
    big = 2 ** 31 - 1
    assert size(big, 32768, big, big, 0, 0.0, 0, 0) == 0 and size(big, 32768, big, big, 1, 0.0, 0, 1) == 0   # 2^98 bytes


def test_hilbert_entries_refuse_before_any_hip_call(rtus):
    L, b = rtus.lib(), _Bufs()
    out = b.p + 2048
    for fn, tail in ((L.rtus_fmc_analytic_i16_dev, (None,)), (L.rtus_fmc_analytic_i16, (0,))):
        for args in ((None, 1, 3, 100, 63, out), (b.p, 1, 3, 100, 63, None), (b.p, 0, 3, 100, 63, out), (b.p, 1, 0, 100, 63, out),
                     (b.p, 1, 3, 0, 63, out), (b.p, 1, 3, 100, 62, out), (b.p, 1, 3, 100, 1, out), (b.p, 1, 3, 100, 257, out),
                     (b.p, 1, 3, 100, 63, b.p + 64)):                   # (600 bytes in, the output starts inside them)
            assert fn(*args, *tail) == -1, args
        assert fn(b.p, 1, 3, (1 << 26) + 1, 63, b.p + (1 << 40), *tail) == -5
        assert fn(b.p, 1 << 15, 1 << 15, 4096, 63, b.p + (1 << 50), *tail) == -5       # 2^32 workgroups
    assert L.rtus_fmc_analytic_i16_dev(b.p + 1, 1, 3, 100, 63, out, None) == -1
    assert L.rtus_fmc_analytic_i16_dev(b.p, 1, 3, 100, 63, out + 4, None) == -1
    pairs = L.rtus_fmc_hilbert_pairs_i16_dev
    far = b.p + (1 << 50)
    for args in ((None, 5, 3, 100, 63, far), (b.p, 5, 3, 100, 63, None), (b.p, 0, 3, 100, 63, far), (b.p, 5, 0, 100, 63, far),
                 (b.p, 5, 3, 0, 63, far), (b.p, 5, 3, 100, 64, far), (b.p, 5, 3, 100, 1, far), (b.p, 5, 3, 100, 257, far),
                 (b.p + 1, 5, 3, 100, 63, far), (b.p, 5, 3, 100, 63, far + 4), (b.p, 5, 3, 100, 63, b.p + 2992)):   # 3000 bytes in
        assert pairs(*args, None) == -1, args
    assert pairs(b.p, 5, 3, (1 << 26) + 1, 63, far, None) == -5
    assert pairs(b.p, 1 << 30, 1 << 20, 100, 63, far, None) == -5


def test_python_errors_come_before_any_library_call(rtus, monkeypatch):
    from importlib import import_module
    lib_mod = import_module("ray-tracing-ultrasound_amd._lib")

    class NoCalls:
        def __getattr__(self, name):
            raise AssertionError(f"the library was called: {name}")
    monkeypatch.setattr(lib_mod, "lib", lambda: NoCalls())
    stack = np.zeros((5, 6, 300), dtype=np.int16)                        # a 3-element capture
    tt = np.zeros((3, 600))
    f = rtus.tfm_envelope_frames
    for bad in (dict(coherence="vcf"), dict(coherence="scf"), dict(coherence="nope"), dict(coherence=1.5), dict(f_demod=-1.0),
                dict(f_demod=0.5 * FS), dict(f_demod=float("nan")), dict(n_taps=62), dict(n_taps=1), dict(n_taps=257), dict(n_taps=63.5),
                dict(n_taps=True), dict(max_frames=0), dict(max_frames=2.5), dict(max_frames=True), dict(out=np.zeros((5, 600), dtype=np.float32)),
                dict(magnitude=True, out=np.zeros((5, 600), dtype=np.complex64)), dict(out=np.zeros((4, 600), dtype=np.complex64))):
        with pytest.raises(ValueError):
            f(stack, FS, tt, **bad)
    with pytest.raises(ValueError):
        f(stack[0], FS, tt)
    with pytest.raises(ValueError):
        f(stack[:0], FS, tt)
    with pytest.raises(ValueError):
        f(stack[:, :5], FS, tt)                                          # five records are no triangle
    with pytest.raises(ValueError):
        f(stack, FS, tt[:2])
    with pytest.raises(ValueError):
        f(stack, FS, tt, tt[:, :599])
    with pytest.raises(ValueError):
        f(stack, 0.0, tt, f_demod=1.0)
    with pytest.raises(ValueError):
        rtus.fmc_analytic_i16(np.zeros((1, 3, 100), dtype=np.float32))
    with pytest.raises(ValueError):
        rtus.fmc_analytic_i16(np.zeros((3, 100), dtype=np.int16))
    # tfm_frames(hmc=True, envelope=True) still raises, and now names the call that does it
    with pytest.raises(ValueError):
        rtus.tfm_frames(stack, FS, tt, hmc=True, envelope=True)
    assert "tfm_envelope_frames" in rtus.tfm_frames.__doc__


@pytest.mark.parametrize("n_frames", [1, 2, 3, 5])
def test_pair_packed_hilbert_layout(rtus, n_frames):
    """plane c of pair p is the imaginary part of frame 2 p + c; the absent frame of an odd stack is +0.0; the real parts are nowhere"""
    rng = np.random.default_rng(n_frames)
    a = (rng.normal(size=(n_frames, 3, 7)) + 1j * rng.normal(size=(n_frames, 3, 7))).astype(np.complex64)
    p = hilbert_pairs(a)
    assert p.dtype == np.float32 and p.shape == ((n_frames + 1) // 2, 3, 7, 2) and p.flags.c_contiguous
    for k in range(n_frames):
        assert np.array_equal(p[k // 2, :, :, k % 2], a[k].imag)
    if n_frames & 1:
        last = p[-1, :, :, 1]
        assert np.all(last == 0) and not np.any(np.signbit(last))
    assert np.array_equal(p, rtus.frames_pack(a.imag[:, None])[:, 0])           # the pack entries' layout with one transmit row


def test_magnitude_definition_on_hand_cases():
    f4, mag = np.float32, envelope_magnitude
    def z(re, im):
        v = np.empty(1, dtype=np.complex64)
        v.real, v.imag = f4(re), f4(im)
        return mag(v)[0]
    assert z(3, 4) == f4(5) and z(-3, 4) == f4(5) and z(0, 0) == 0 and z(-0.0, 0.0) == 0 and mag(np.zeros(3, np.complex64)).dtype == f4
    tiny = np.ldexp(1.0, -149)                                           # the smallest subnormal: its square underflows in float32
    assert z(tiny, 0) == f4(tiny) and z(0, -tiny) == f4(tiny)
    assert z(3 * tiny, 4 * tiny) == f4(5 * tiny)
    assert z(tiny, tiny) == f4(tiny)                                     # sqrt(2) tiny = 1.41 tiny rounds to tiny
    assert z(2 * tiny, 2 * tiny) == f4(3 * tiny)                         # 2.83 tiny rounds to 3 tiny
    big = float(np.finfo(f4).max)
    assert z(big, 0) == f4(big) and z(0, -big) == f4(big)               # no overflow on the way: the square is 1.2e77 in float64
    assert z(big, tiny) == f4(big)
    assert z(0.6 * big, 0.8 * big) == np.sqrt(np.float64(f4(0.6 * big)) ** 2 + np.float64(f4(0.8 * big)) ** 2).astype(f4) and np.isfinite(z(0.6 * big, 0.8 * big))
    assert np.isinf(z(big, big))                                         # sqrt(2) max is not a float: the one rounding to float gives inf
    assert np.isnan(z(float("nan"), 1)) and np.isinf(z(float("inf"), 1))
    # one rounding: a value whose float64 magnitude is not a float32 rounds once, to nearest
    v = np.empty(1000, dtype=np.complex64)
    rng = np.random.default_rng(5)
    v.real, v.imag = rng.normal(size=1000).astype(f4), rng.normal(size=1000).astype(f4)
    from math import sqrt
    want = np.array([f4(sqrt(float(c.real) * float(c.real) + float(c.imag) * float(c.imag))) for c in v])
    assert np.array_equal(mag(v), want)


def _kernel_metadata(source):
    """a file of csrc compiled device-only to assembly with the Makefile's flags -> {kernel name: its code-object metadata}"""
    import subprocess
    import tempfile
    csrc = os.path.join(ROOT, "ray-tracing-ultrasound_amd", "csrc")
    flags = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-fno-fast-math", "-fno-slp-vectorize", "--cuda-device-only", "-S"]
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "k.s")
        subprocess.run(["/opt/rocm/bin/hipcc"] + flags + [os.path.join(csrc, source), "-o", out], check=True, capture_output=True, timeout=600)
        meta = open(out).read().split("amdhsa.kernels:")[1]
    res = {}
    for entry in re.split(r"^  - ", meta, flags=re.M)[1:]:
        kv = dict(re.findall(r"^ {0,4}(\.\w+):\s+(\S+)\s*$", entry, flags=re.M))
        if ".vgpr_count" in kv:
            res[kv[".name"]] = {k: int(kv[k]) for k in (".vgpr_count", ".vgpr_spill_count", ".private_segment_fixed_size", ".group_segment_fixed_size")}
    return res


@pytest.mark.parametrize("source,pattern,count,lds", [
    ("rtus_autofocus.hip", "rtus_analytic_i16_kernel", 2, [5112, 10224]),           # one tile + halo; the pair form holds two
    ("rtus_tfm_envelope_frames.hip", "rtus_envelope_combine_kernel", 6, [0] * 6)])
def test_new_kernels_use_no_scratch(source, pattern, count, lds):
    """every new kernel keeps everything in registers (no scratch, no spilled VGPR) and at most 64 VGPRs (eight waves per SIMD)"""
    res = {k: v for k, v in _kernel_metadata(source).items() if pattern in k}
    assert len(res) == count, sorted(res)
    for k, v in res.items():
        assert v[".private_segment_fixed_size"] == 0 and v[".vgpr_spill_count"] == 0, (k, v)
        assert v[".vgpr_count"] <= 64, (k, v)
    assert sorted(v[".group_segment_fixed_size"] for v in res.values()) == lds

"""CPU: the plumbing of TFM over a stack of frames (include/rtus.h: rtus_tfm_frames, rtus_tfm_analytic_frames): the packed layout's
NumPy restatement on every small shape, the exports and the version, the status code of every bad argument through ctypes (the checks
run before any HIP call), the Python errors raised before any library call, and the kernels' resources from the code object's
metadata.  No GPU touched."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import ROOT


@pytest.mark.parametrize("shape", [(1, 1), (2, 3)], ids=["1x1", "2x3"])
@pytest.mark.parametrize("n_t", [1, 23, 24])
@pytest.mark.parametrize("n_frames", [1, 2, 3, 5])
def test_pack_and_unpack_round_trip(rtus, n_frames, n_t, shape):
    rng = np.random.default_rng(100 * n_frames + n_t)
    stack = rng.standard_normal((n_frames, *shape, n_t)).astype(np.float32)
    stack[stack == 0] = 1.0
    packed = rtus.frames_pack(stack)
    n_pairs = (n_frames + 1) // 2
    assert packed.dtype == np.float32 and packed.shape == (n_pairs, *shape, n_t, 2) and packed.flags.c_contiguous
    for k in range(n_frames):                                            # the layout, element by element
        assert np.array_equal(packed[k // 2, ..., k % 2], stack[k])
    if n_frames % 2:                                                     # the absent partner: +0.0 everywhere
        tail = packed[-1, ..., 1]
        assert np.all(tail == 0) and not np.signbit(tail).any()
    back = rtus.frames_unpack(packed, n_frames)
    assert back.dtype == np.float32 and np.array_equal(back, stack)
    if n_frames % 2 == 0:                                                # an even count may be read as one frame fewer
        assert np.array_equal(rtus.frames_unpack(packed, n_frames - 1), stack[:-1])
    for bad in (0, n_frames + 2, 2 * n_pairs + 1, -1):
        with pytest.raises(ValueError):
            rtus.frames_unpack(packed, bad)
    with pytest.raises(ValueError):
        rtus.frames_pack(stack[0])
    with pytest.raises(ValueError):
        rtus.frames_unpack(packed[..., 0], n_frames)


def test_exports_version_and_status_codes(rtus):
    from importlib import import_module
    L = rtus.lib()
    assert L.rtus_version() >= 121
    names = ("rtus_fmc_pack_frames_floats", "rtus_fmc_pack_frames_dev", "rtus_tfm_frames_dev", "rtus_tfm_frames",
             "rtus_tfm_analytic_frames_dev", "rtus_tfm_analytic_frames")
    for name in names:
        assert name in rtus.EXPORTS and hasattr(L, name)
    lib_mod = import_module("ray-tracing-ultrasound_amd._lib")
    assert all(since == 121 for n, _, _, since in lib_mod.PROTOTYPES if n in names)
    for name in ("frames_pack", "frames_unpack", "tfm_frames"):
        assert name in rtus.__all__ and callable(getattr(rtus, name))
    dev = import_module("ray-tracing-ultrasound_amd.device")
    assert all(callable(getattr(dev, n)) for n in ("fmc_pack_frames_dev", "tfm_frames_dev", "tfm_analytic_frames_dev"))

    # the packed size
    size = L.rtus_fmc_pack_frames_floats
    assert size(1, 1, 1, 1) == 2 and size(2, 1, 1, 1) == 2 and size(3, 2, 3, 5) == 2 * 2 * 30 and size(9, 64, 64, 2048) == 10 * 64 * 64 * 2048
    for bad in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 1, 0), (-2, 1, 1, 1), (1, 1, 1, -7)):
        assert size(*bad) == 0, bad
    big = 0x7fffffff
    assert size(big, big, big, big) == 0 and size(big, big, big, 1) == 0          # 2^93 floats; 2^62 floats: out of range
    assert size(big, 1 << 15, 1 << 13, 1) == (big + 1) << 28                     # 2^59 floats: in range

    buf = np.zeros(4096)
    p = buf.ctypes.data
    assert p % 16 == 0

    # pack
    pack = lambda **kw: L.rtus_fmc_pack_frames_dev(*[{**dict(i=p, f=3, tx=2, rx=2, t=5, o=p + 2048), **kw}[k] for k in ("i", "f", "tx", "rx", "t", "o")], None)   # noqa: E731
    for name in ("i", "o"):
        assert pack(**{name: None}) == -1, name
    for name in ("f", "tx", "rx", "t"):
        assert pack(**{name: 0}) == -1 and pack(**{name: -1}) == -1, name
    assert pack(o=p) == -1 and pack(o=p + 4 * 58) == -1 and pack(i=p + 4 * 79, o=p) == -1      # overlap: 60 floats in, 80 out
    assert pack(o=p + 2052) == -1                                                # not 8-byte aligned
    assert pack(f=big, tx=big, rx=big, t=big) == -5                              # the size does not fit

    # the imaging entries: (data, n_frames, n_tx, n_rx, n_t, fs, t0[, f_demod], tt_tx, tt_rx, n_f, images[, cf], stream | device)
    base = dict(d=p, f=3, tx=2, rx=2, t=8, fs=1.0e6, t0=0.0, fd=0.0, ttx=p, trx=p, nf=4, img=p)

    def rf(dev, **kw):
        a = {**base, **kw}
        args = (a["d"], a["f"], a["tx"], a["rx"], a["t"], a["fs"], a["t0"], a["ttx"], a["trx"], a["nf"], a["img"])
        return L.rtus_tfm_frames_dev(*args, None) if dev else L.rtus_tfm_frames(*args, 0)

    def an(dev, **kw):
        a = {**base, **kw}
        args = (a["d"], a["f"], a["tx"], a["rx"], a["t"], a["fs"], a["t0"], a["fd"], a["ttx"], a["trx"], a["nf"], a["img"], None)
        return L.rtus_tfm_analytic_frames_dev(*args, None) if dev else L.rtus_tfm_analytic_frames(*args, 0)
    for call in (rf, an):
        for dev in (False, True):
            for name in ("d", "ttx", "trx", "img"):
                assert call(dev, **{name: None}) == -1, name
            for name in ("f", "tx", "rx", "t", "nf"):
                assert call(dev, **{name: 0}) == -1 and call(dev, **{name: -4}) == -1, name
            assert call(dev, t=1) == -1                                          # rtus_tfm's: two samples at least
            for fs in (0.0, -1.0, np.inf, np.nan):
                assert call(dev, fs=fs) == -1, fs
            for t0 in (np.inf, np.nan):
                assert call(dev, t0=t0) == -1, t0
            assert call(dev, t=(1 << 26) + 1) == -5                              # rtus_tfm_analytic's n_t limit
            assert call(dev, t=(1 << 26) + 1, img=None) == -1                    # invalid before unsupported
    for dev in (False, True):
        for fd in (-1.0, 0.5e6, 1.0e6, np.inf, np.nan):
            assert an(dev, fd=fd) == -1, fd
        # the workgroup count: ceil(n_f / 256) per image, 2^31 - 1 at the most
        assert an(dev, f=256, nf=big) == -5                                      # 256 frames x 2^23 workgroups = 2^31
        assert rf(dev, f=512, nf=big) == -5                                      # 256 pairs x 2^23 workgroups = 2^31
        assert an(dev, f=1 << 20, nf=1 << 20) == -5 and rf(dev, f=1 << 21, nf=1 << 20) == -5


def test_python_errors_before_any_library_call(rtus, monkeypatch):
    from importlib import import_module
    api = import_module("ray-tracing-ultrasound_amd.api")

    def no_library():
        raise AssertionError("the library was called")
    monkeypatch.setattr(api._lib, "lib", no_library)
    stack = np.zeros((3, 2, 4, 16), dtype=np.float32)
    tt_tx, tt_rx = np.zeros((2, 5)), np.zeros((4, 5))
    good = dict(stack=stack, fs=1.0e6, tt_tx=tt_tx, tt_rx=tt_rx)
    for kw in (dict(stack=stack[0]), dict(stack=stack[:0]), dict(stack=np.zeros((3, 2, 4, 16, 2), dtype=np.float32)),
               dict(tt_tx=tt_tx[0]), dict(tt_tx=np.zeros((3, 5))), dict(tt_rx=np.zeros((4, 6))), dict(tt_rx=np.zeros((2, 5))),
               dict(tt_rx=None),                                                 # one table against 2 x 4 elements
               dict(coherence=True), dict(coherence="cf"), dict(f_demod=1.0e5),  # both need envelope=True
               dict(envelope=True, coherence="vcf"), dict(envelope=True, coherence="scf"), dict(envelope=True, coherence="xx"),
               dict(envelope=True, f_demod=-1.0), dict(envelope=True, f_demod=0.5e6), dict(envelope=True, f_demod=np.nan),
               dict(envelope=True, n_taps=4), dict(envelope=True, n_taps=1), dict(envelope=True, n_taps=257),
               dict(max_frames=0), dict(max_frames=-1), dict(max_frames=1.5), dict(max_frames=True),
               dict(out=np.zeros((3, 5))), dict(out=np.zeros((2, 5), dtype=np.float32)), dict(out=np.zeros((3, 5), dtype=np.complex64)),
               dict(envelope=True, out=np.zeros((3, 5), dtype=np.float32)),
               dict(out=np.zeros((5, 3), dtype=np.float32).T)):
        with pytest.raises(ValueError):
            rtus.tfm_frames(**{**good, **kw})
        # (kw is reported by pytest's traceback when the call does not raise)


def test_kernel_resources_of_the_frames_kernels():
    """rtus_tfm_frames.hip compiled device-only to assembly with the Makefile's flags.  Every kernel: no scratch, no spilled register.
    The imaging kernels: the 64 x 256 delay tile in LDS (65,536 bytes) and no more VGPRs than the existing sibling of each needs,
    read from rtus_tfm.hip's metadata in the same way: rtus_tfm_analytic_kernel<false> (95) for the RF pair kernel (94),
    rtus_tfm_analytic_kernel<CF> (98 / 95) and rtus_tfm_iq_kernel<CF> (132 / 129) for the frames kernels of the same arguments (the
    same counts), and 98 at the most for the linear ones.  The pack kernels: no LDS.  Metadata only."""
    import re
    import subprocess
    import tempfile
    csrc = os.path.join(ROOT, "ray-tracing-ultrasound_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "rtus_tfm_frames.hip" in re.search(r"^SRCS\s*:=\s*(.*)$", mk, flags=re.M).group(1).split()
    flags = re.search(r"^CXXFLAGS\s*:=\s*(.*)$", mk, flags=re.M).group(1).replace("$(ARCH)", "gfx950").split()
    keys = (".vgpr_count:", ".vgpr_spill_count:", ".sgpr_spill_count:", ".private_segment_fixed_size:", ".group_segment_fixed_size:")

    def kernels_of(src):
        found = {}
        with tempfile.TemporaryDirectory() as td:
            out = os.path.join(td, src + ".s")
            subprocess.run(["/opt/rocm/bin/hipcc"] + flags + ["--cuda-device-only", "-S", os.path.join(csrc, src), "-o", out],
                           check=True, capture_output=True, timeout=600)
            meta = open(out).read().split("amdhsa.kernels:")[1]
            for entry in re.split(r"\n  - \.", meta)[1:]:                 # one entry per kernel; its keys in any order
                v = {}
                for ln in ("." + entry).splitlines():
                    ln = ln.strip().lstrip("- ")
                    for key in keys + (".name:",):
                        if ln.startswith(key):
                            v[key] = ln.split()[1]
                assert all(key in v for key in keys), v
                found[v[".name:"]] = {k: int(v[k]) for k in keys}
        return found
    new, old = kernels_of("rtus_tfm_frames.hip"), kernels_of("rtus_tfm.hip")
    print(new)
    pick = lambda d, part: [v for k, v in d.items() if part in k]         # noqa: E731
    one = lambda d, part: (lambda m: m[0] if len(m) == 1 else pytest.fail(f"{part}: {len(m)} kernels"))(pick(d, part))   # noqa: E731
    assert len(new) == 7, sorted(new)
    for v in new.values():
        assert v[".private_segment_fixed_size:"] == 0 and v[".vgpr_spill_count:"] == 0 and v[".sgpr_spill_count:"] == 0, v
    assert len(pick(new, "rtus_fmc_pack_frames_kernel")) == 2
    for v in pick(new, "rtus_fmc_pack_frames_kernel"):
        assert v[".group_segment_fixed_size:"] == 0 and v[".vgpr_count:"] <= 32, v
    # (mangled names: ILb1E / ILb0E are the template argument CF = true / false)
    pairs = [("22rtus_tfm_frames_kernel", "24rtus_tfm_analytic_kernelILb0E")]
    for cf in ("ILb1E", "ILb0E"):
        pairs.append(("31rtus_tfm_analytic_frames_kernel" + cf, "24rtus_tfm_analytic_kernel" + cf))
        pairs.append(("25rtus_tfm_iq_frames_kernel" + cf, "18rtus_tfm_iq_kernel" + cf))
    for mine, sibling in pairs:
        v, s = one(new, mine), one(old, sibling)
        assert v[".group_segment_fixed_size:"] == 64 * 256 * 4 == s[".group_segment_fixed_size:"], (mine, v)
        assert v[".vgpr_count:"] <= s[".vgpr_count:"], (mine, v[".vgpr_count:"], sibling, s[".vgpr_count:"])
        if "iq" not in mine:
            assert v[".vgpr_count:"] <= 98, (mine, v)

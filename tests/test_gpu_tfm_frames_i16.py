"""GPU: TFM over a stack of int16 frames (include/rtus.h: rtus_tfm_frames_i16, rtus_tfm_frames_i16_dev, rtus_fmc_pack_frames_i16_dev),
held BIT FOR BIT — every comparison is np.array_equal up to the sign of a zero — to

  * the exact model tests/das_exact_numpy.py on its cases: the records are integers in [-4, 4], so the real and the imaginary plane of
    record set k are int16 frames 2 k and 2 k + 1, each with records of its own (the models are test_gpu_tfm_frames.py's, formed once
    for both files);
  * rtus_tfm (tfm_image) on each frame converted to float32, on samples over the whole int16 range and random times off the lattice;
  * api.frames_pack_i16 for the pack kernel, the host twin for the _dev entries, a graph replay for the capture;
  * sparse long records (n_t = 2^22: a quad's record is 2^25 bytes) for the 32-bit offsets inside the packed layout, and a packed
    stack whose second quad starts 4 GiB in for the 64-bit offsets between quads;
  * the sizes at which a call cuts its stack into several launches (about 2304 workgroups each, counted in quads).

That the tests can fail — each change made once on a scratch build and this file run once against it (DESIGN.md §4 lists the same):
  M1  the low half decoded without sign extension   -> 16 of the 18 tests: every one that reads an image through the host twin or
                                                       against a model (a negative even plane reads 65536 too high)
  M2  planes 0 and 1 swapped in the epilogue        -> the same 16
  M3  the quad offset dropped from the record base  -> 14: every one of those with two quads in one launch (not: one quad per launch at
                                                       1153 workgroups per image, the single long quad)
  M4  the pack's zero planes left as they were      -> test_device_pack_is_frames_pack_i16 (ragged stacks, into a sentinel-filled output)
  M5  the absent-frame stores not skipped           -> NOT RUN: the mutant stores rows past the end of the images wherever a test gives
                                                       exactly n_frames rows, and an out-of-bounds store is not a wrong-answer mutation.
                                                       By reading: test_dev_entries_are_the_host_twin_and_leave_the_rows_after_a_ragged_stack
                                                       checks the sentinel row after 5, 6, 7 and 1 frames, which such a store overwrites.
(test_device_pack_is_frames_pack_i16 does not image; test_dev_entries_... compares the _dev entries with the host twin of the same
build, so it cannot see M1 to M3)
"""
import numpy as np
import pytest

import das_exact_numpy as D
from test_gpu_tfm_frames import LONG_TARGETS, _case_frames, _dev, _f32, _long_case, _long_sum, _same, _t, _tables

pytestmark = pytest.mark.gpu

CASES = ("1x1_one", "2x17", "5x63", "64x64_one", "65x65_one", "4x129")
N_FRAMES = (1, 2, 3, 4, 5, 9)                                            # every raggedness of the last quad
_made = {}


def _case_i16(name):
    """the case's tables with nine int16 frames -> (case, stack int16 [9, n_tx, n_rx, N_T], [model image of frame k]): frame 2 k is
    the real, frame 2 k + 1 the imaginary plane of record set k"""
    if name not in _made:
        c, a, m = _case_frames(name)
        planes = [p for k in range(a.shape[0]) for p in (a[k].real, a[k].imag)][:max(N_FRAMES)]
        stack = np.stack(planes).astype(np.int16)
        assert np.array_equal(stack.astype(np.float32), np.stack(planes))
        want = [_f32(m[j // 2]["S"].real if j % 2 == 0 else m[j // 2]["S"].imag) for j in range(stack.shape[0])]
        stack.flags.writeable = False
        _made[name] = (c, stack, want)
    return _made[name]


# ------------------------------------------------------------------------------------------------------------ the exact model
@pytest.mark.parametrize("name", CASES)
def test_int16_stacks_against_the_exact_model(rtus, name):
    """stacks of 1, 2, 3, 4, 5 and 9 frames: frame k against the model of frame k; the no-path column is zero."""
    c, stack, want = _case_i16(name)
    tt_tx, tt_rx = _tables(c)
    for n in N_FRAMES:
        got = rtus.tfm_frames(stack[:n], c["fs"], tt_tx, tt_rx, t0=c["t0"])
        _same(got, np.stack(want[:n]), f"{name} {n} frames")
        assert np.all(got[:, c["cols"]["no_path"]] == 0)
    # other partners in the quads: the planes shifted by three
    _same(rtus.tfm_frames(stack[3:8], c["fs"], tt_tx, tt_rx, t0=c["t0"]), np.stack(want[3:8]), f"{name} frames 3 .. 7")


@pytest.mark.parametrize("name", ["5x63", "64x64_one"])
def test_eight_workgroups_per_image_in_xcd_order(rtus, name):
    """the tables tiled to 2048 focal points: eight workgroups per image, the XCD-contiguous branch of the workgroup order; nine
    frames, so three quads of eight.  A wrong block index moves whole blocks of 256 columns or whole images."""
    c, stack, want = _case_i16(name)
    sel = np.arange(2048) % D.N_F
    tt_tx, tt_rx = _tables(c, sel)
    _same(rtus.tfm_frames(stack, c["fs"], tt_tx, tt_rx, t0=c["t0"]), np.stack([w[sel] for w in want]), name)


# A call cuts its stack into launches of about 2304 workgroups (rtus_tfm_frames_i16.hip): 2304 // n_blk quads per launch, one at least
PER_LAUNCH_2, PER_LAUNCH_1 = 1152 * 256, 1153 * 256                      # the last size with two quads per launch, the first with one


@pytest.mark.parametrize("name,n_f", [("2x17", PER_LAUNCH_2), ("2x17", PER_LAUNCH_1), ("64x64_one", PER_LAUNCH_2)],
                         ids=["2x17_two_per_launch", "2x17_one_per_launch", "64x64_one_two_per_launch"])
def test_large_images_take_several_launches(rtus, name, n_f):
    """the tables tiled to 1152 and to 1153 workgroups per image, nine frames: three quads in launches of 2 + 1 and of 1 + 1 + 1 (the
    last quad holds one frame); the offsets of the data and the images between the launches."""
    c, stack, want = _case_i16(name)
    sel = np.arange(n_f) % D.N_F
    tt_tx, tt_rx = _tables(c, sel)
    _same(rtus.tfm_frames(stack, c["fs"], tt_tx, tt_rx, t0=c["t0"]), np.stack([w[sel] for w in want]), name)


# ------------------------------------------------------------------------------------------------------------ full-range data
FS_R, N_T_R, N_F_R, T0_R = 40.0e6, 200, 300, 0.25e-6


def _full_range_case(rtus):
    """nine frames of 5 x 7 records of 200 samples uniform over the whole int16 range; record (0, 0) of every frame alternates
    -32768 and 32767 and record (1, 1) alternates -1 and 1, each frame the other way round than its neighbour: in the packed layout
    every dword of these records has a negative half beside a positive one, in both orders.  Two tables of random times: positions
    over [-8, n_t + 8] samples, off every lattice, 2 % of the legs NaN; 300 focal points: two workgroups, the second ragged.
    -> (stack, tt_tx, tt_rx, [tfm_image of frame k as float32])"""
    if "full" not in _made:
        rng = np.random.default_rng(2025)
        stack = rng.integers(-32768, 32768, (9, 5, 7, N_T_R)).astype(np.int16)
        t = np.arange(N_T_R)
        for k in range(9):
            stack[k, 0, 0] = np.where((t + k) % 2, -32768, 32767)
            stack[k, 1, 1] = np.where((t + k) % 2, 1, -1)
        assert stack.min() == -32768 and stack.max() == 32767
        words = np.ascontiguousarray(rtus.frames_pack_i16(stack)).view(np.uint32)
        lo, hi = (words & 0xffff).astype(np.int64), (words >> 16).astype(np.int64)
        assert np.any((lo >= 0x8000) & (hi < 0x8000) & (hi > 0)) and np.any((lo < 0x8000) & (lo > 0) & (hi >= 0x8000))
        tt = [(rng.uniform(-4.0, N_T_R / 2 + 4.0, (n, N_F_R)) / FS_R + 0.5 * T0_R) for n in (5, 7)]
        for v in tt:
            v[rng.random(v.shape) < 0.02] = np.nan
        want = np.stack([rtus.tfm_image(stack[k].astype(np.float32), FS_R, tt[0], tt[1], t0=T0_R) for k in range(9)])
        for v in (stack, want, *tt):
            v.flags.writeable = False
        _made["full"] = (stack, tt[0], tt[1], want)
    return _made["full"]


def test_int16_frames_are_tfm_image_of_each_frame_as_float32(rtus):
    stack, tt_tx, tt_rx, want = _full_range_case(rtus)
    assert np.count_nonzero(want) > 0.9 * want.size
    got = rtus.tfm_frames(stack, FS_R, tt_tx, tt_rx, t0=T0_R)
    _same(got, want, "int16")
    for n in range(1, 9):                                                # no bit depends on n_frames or on the partners
        _same(rtus.tfm_frames(stack[1:1 + n], FS_R, tt_tx, tt_rx, t0=T0_R), want[1:1 + n], f"frames 1 .. {n}")
    for per in (1, 2, 3, 4, 5):
        _same(rtus.tfm_frames(stack, FS_R, tt_tx, tt_rx, t0=T0_R, max_frames=per), want, f"in chunks of {per}")
    out = np.zeros_like(want)
    assert rtus.tfm_frames(stack, FS_R, tt_tx, tt_rx, t0=T0_R, out=out) is out and np.array_equal(out, want)
    _same(got, rtus.tfm_frames(stack.astype(np.float32), FS_R, tt_tx, tt_rx, t0=T0_R), "against the float32 stack call")


def test_a_long_stack_is_cut_into_launches(rtus):
    """37 frames (the nine of the case, cycled) at 256 workgroups per image, nine quads per launch: ten quads in launches of 9 + 1,
    the last quad holding one frame; each frame against tfm_image.  (4 and 9 have no common factor: a quad taken from the wrong
    place holds other frames.)"""
    stack, tt_tx, tt_rx, _ = _full_range_case(rtus)
    sel = np.arange(256 * 256) % N_F_R
    tx, rx = np.ascontiguousarray(tt_tx[:, sel]), np.ascontiguousarray(tt_rx[:, sel])
    pick = np.arange(37) % 9
    one = [rtus.tfm_image(stack[k].astype(np.float32), FS_R, tx, rx, t0=T0_R) for k in range(9)]   # each formed once
    _same(rtus.tfm_frames(stack[pick], FS_R, tx, rx, t0=T0_R), np.stack([one[k] for k in pick]), "37 frames")


# ------------------------------------------------------------------------------------------------------------ pack, the _dev entries
SENTINEL_I16 = -21846                                                    # 0xAAAA


def test_device_pack_is_frames_pack_i16(rtus):
    """every small shape of the CPU test and n_t = 1025 (more than one workgroup per frame), with a 4 x 1 aperture besides: frames of
    n_tx n_rx n_t samples that are a multiple of eight (the 16-byte form) and that are not; into an output filled with a sentinel, so
    that an unwritten zero plane shows."""
    torch, dev = _dev()
    for n_frames in range(1, 10):
        for n_t in (1, 23, 24, 1025):
            for shape in ((1, 1), (2, 3), (4, 1)):
                rng = np.random.default_rng(7 * n_frames + n_t)
                stack = rng.integers(-32768, 32768, (n_frames, *shape, n_t)).astype(np.int16)
                out = torch.full(((n_frames + 3) // 4, *shape, n_t, 4), SENTINEL_I16, dtype=torch.int16, device="cuda")
                got = dev.fmc_pack_frames_i16_dev(torch.as_tensor(stack, device="cuda"), out=out)
                assert got is out
                _same(got.cpu().numpy(), rtus.frames_pack_i16(stack), f"{n_frames} frames of {shape} x {n_t}")
    # a stack that starts 2 bytes off a 16-byte boundary: the 2-byte form on a size that is a multiple of eight
    stack = np.random.default_rng(5).integers(-32768, 32768, (5, 2, 2, 64)).astype(np.int16)
    buf = torch.zeros(stack.size + 8, dtype=torch.int16, device="cuda")
    buf[1:1 + stack.size] = torch.as_tensor(stack.reshape(-1), device="cuda")
    view = buf[1:1 + stack.size].view(stack.shape)
    assert view.data_ptr() % 16 == 2 and view.is_contiguous()
    _same(dev.fmc_pack_frames_i16_dev(view).cpu().numpy(), rtus.frames_pack_i16(stack), "off the boundary")
    with pytest.raises(ValueError):
        dev.fmc_pack_frames_i16_dev(view[0])
    with pytest.raises(ValueError):
        dev.fmc_pack_frames_i16_dev(view, out=torch.empty(7, dtype=torch.int16, device="cuda"))
    with pytest.raises(ValueError):
        dev.fmc_pack_frames_i16_dev(view.to(torch.float32))
    with pytest.raises(ValueError):
        dev.fmc_pack_frames_i16_dev(view, out=torch.empty((2, 2, 2, 64, 4), dtype=torch.float32, device="cuda"))


def test_dev_entries_are_the_host_twin_and_leave_the_rows_after_a_ragged_stack(rtus):
    """pack + tfm_frames_i16_dev against tfm_frames (the host twin of the same build).  The outputs are views big[:n_frames] of
    tensors one frame longer filled with a sentinel: the row after the last frame keeps it — the absent frames' stores are skipped."""
    torch, dev = _dev()
    stack, tt_tx, tt_rx, _ = _full_range_case(rtus)
    tx, rx = _t(torch, tt_tx), _t(torch, tt_rx)
    sentinel = -12345.0
    for n in (5, 6, 7, 8, 1):
        want = rtus.tfm_frames(stack[:n], FS_R, tt_tx, tt_rx, t0=T0_R)
        packed = dev.fmc_pack_frames_i16_dev(_t(torch, stack[:n]))
        big = torch.full((n + 1, N_F_R), sentinel, dtype=torch.float32, device="cuda")
        got = dev.tfm_frames_i16_dev(packed, n, FS_R, tx, rx, t0=T0_R, out=big[:n])
        assert got.data_ptr() == big.data_ptr()
        host = big.cpu().numpy()
        _same(host[:n], want, f"{n} frames")
        assert np.all(host[n] == sentinel), f"{n} frames: the row after the last frame was written"
        _same(dev.tfm_frames_i16_dev(packed, n, FS_R, tx, rx, t0=T0_R).cpu().numpy(), want, f"{n} frames, fresh output")
    full = dev.fmc_pack_frames_i16_dev(_t(torch, stack))                # three quads: nine to twelve frames
    for bad in (13, 8, 0):
        with pytest.raises(ValueError):
            dev.tfm_frames_i16_dev(full, bad, FS_R, tx, rx)
    with pytest.raises(ValueError):
        dev.tfm_frames_i16_dev(full.to(torch.float32), 9, FS_R, tx, rx)
    with pytest.raises(ValueError):
        dev.tfm_frames_i16_dev(full, 9, FS_R, rx, tx)
    with pytest.raises(ValueError):
        dev.tfm_frames_i16_dev(full, 9, FS_R, tx, rx, out=torch.empty(N_F_R, dtype=torch.float32, device="cuda"))


def test_capture_and_replay_of_the_int16_stack_call(rtus):
    """pack + rtus_tfm_frames_i16_dev captured once in a torch.cuda.graph and replayed: the same bits (the _dev entries allocate
    nothing and do not synchronise)"""
    torch, dev = _dev()
    stack, tt_tx, tt_rx, want = _full_range_case(rtus)
    d_stack = _t(torch, stack)
    tx, rx = _t(torch, tt_tx), _t(torch, tt_rx)
    packed = torch.empty((3, *stack.shape[1:], 4), dtype=torch.int16, device="cuda")
    out = torch.empty((9, N_F_R), dtype=torch.float32, device="cuda")

    def run():
        dev.fmc_pack_frames_i16_dev(d_stack, out=packed)
        dev.tfm_frames_i16_dev(packed, 9, FS_R, tx, rx, t0=T0_R, out=out)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                       # warm-up off the default stream, as torch.cuda.graph wants
        run()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    _same(out.cpu().numpy(), want, "before the capture")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                        # one capture stream: the two kernels in sequence
        run()
    packed.fill_(SENTINEL_I16); out.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    _same(out.cpu().numpy(), want, "replayed")


# ------------------------------------------------------------------------------------------------------------ long records
def _fill_quad(torch, quad, parts, n_t):
    """the sparse records into one quad [n_tx, n_rx, n_t, 4] of a packed stack on the device: parts = [(head, tail)] of one or two
    long cases; planes 0, 1 the real and imaginary parts of the first, planes 2, 3 of the second"""
    for k, (head, tail) in enumerate(parts):
        for block, where in ((head, slice(0, 8)), (tail, slice(n_t - 8, n_t))):
            v = np.stack([block.real, block.imag], axis=-1).astype(np.int16)
            quad[:, :, where, 2 * k:2 * k + 2] = torch.as_tensor(v, device="cuda")


def test_long_records_and_32_bit_offsets_inside_a_quad(rtus):
    """n_t = 2^22, one quad of four frames made on the device, 2 x 3 records of 2^25 bytes each: zero but for the first and last eight
    samples of each plane, so a byte offset that wrapped, lost its high bits or was scaled for another record size reads zeros or
    the wrong end.  Then the quad read as one, two and three frames, and the same four frames frame-major through the pack kernel
    (its offsets: 2^23 bytes per record side by side), which must give the quad back."""
    torch, dev = _dev()
    n_t, fs = 2 ** 22, D.FS
    parts, S = [], []
    for seed in (31, 32):
        head, tail, tau_tx, tau_rx = _long_case(n_t, 2, 3, LONG_TARGETS, seed)      # (the legs depend on the targets only)
        parts.append((head, tail))
        s = _long_sum(head, tail, n_t, tau_tx, tau_rx)
        S += [_f32(s.real), _f32(s.imag)]
    assert all(np.count_nonzero(s) >= 5 for s in S) and len({s.tobytes() for s in S}) == 4
    packed = torch.zeros((1, 2, 3, n_t, 4), dtype=torch.int16, device="cuda")
    _fill_quad(torch, packed[0], parts, n_t)
    tt, tr = torch.as_tensor(tau_tx / fs, device="cuda"), torch.as_tensor(tau_rx / fs, device="cuda")
    for n in (4, 3, 2, 1):
        _same(dev.tfm_frames_i16_dev(packed, n, fs, tt, tr).cpu().numpy(), np.stack(S[:n]), f"{n} frames of long records")
    stack = packed[0].permute(3, 0, 1, 2).contiguous()
    again = dev.fmc_pack_frames_i16_dev(stack)
    assert bool(torch.equal(again, packed))
    del stack, again, packed
    torch.cuda.empty_cache()


def test_second_quad_four_gib_into_the_packed_stack(rtus):
    """five frames of 8 x 16 records of 2^22 samples: a quad is 2^32 bytes, so quad 1 starts exactly 4 GiB in (8 GiB on the device,
    zero-filled there; no host copy) — an offset between quads kept in 32 bits reads quad 0.  The quads hold different records."""
    torch, dev = _dev()
    n_t, fs, n_tx, n_rx = 2 ** 22, D.FS, 8, 16
    packed = torch.zeros((2, n_tx, n_rx, n_t, 4), dtype=torch.int16, device="cuda")
    assert packed[1].data_ptr() - packed[0].data_ptr() == 2 ** 32
    targets = [0.0, 3.5, 9.0, 2.0 ** 22 - 8.5, 2.0 ** 22 - 1.0, 2.0 ** 22 + 4.0]
    want, quads = [], [[], []]
    for k, q in ((0, 0), (1, 0), (2, 1)):
        head, tail, tau_tx, tau_rx = _long_case(n_t, n_tx, n_rx, targets, 40 + k)
        quads[q].append((head, tail))
        s = _long_sum(head, tail, n_t, tau_tx, tau_rx)
        want += [_f32(s.real), _f32(s.imag)]
    for q in range(2):
        _fill_quad(torch, packed[q], quads[q], n_t)
    assert not np.array_equal(want[0], want[4]) and np.count_nonzero(want[4]) >= 3
    tt, tr = torch.as_tensor(tau_tx / fs, device="cuda"), torch.as_tensor(tau_rx / fs, device="cuda")
    got = dev.tfm_frames_i16_dev(packed, 5, fs, tt, tr).cpu().numpy()
    _same(got, np.stack(want[:5]), "five frames, the fifth 4 GiB in")
    del packed
    torch.cuda.empty_cache()

"""GPU: TFM over a stack of half-matrix frames (include/rtus.h: rtus_tfm_frames_hmc_i16[_dev], rtus_tfm_frames_hmc[_dev];
api.tfm_frames(hmc=True)), held BIT FOR BIT — every comparison is np.array_equal up to the sign of a zero — to

  * the exact model tests/das_exact_numpy.py (tfm_hmc) at every size of D.HMC_SIZES, one table and two: the records are integers in
    [-4, 4], so the real and the imaginary plane of record set k are int16 frames 2 k and 2 k + 1, each with records of its own;
  * rtus_tfm_hmc (api.tfm_hmc) on each frame converted to float32, on samples over the whole int16 range and random times off the
    lattice;
  * the host twins for the _dev entries, a graph replay for the capture;
  * sparse long records (n_t = 2^22: a quad's record is 2^25 bytes) for the 32-bit offsets inside a record, and a 16-element stack
    whose quad is 4.6 GB for the 64-bit offsets between the records of a quad and between quads;
  * the sizes at which a call cuts its stack into several launches (about 2304 workgroups each, counted in quads or pairs).
Both routes everywhere: int16 quads and float32 pairs.

That the tests can fail — each change made once on a scratch build and this file (41 tests) run once against it (DESIGN.md §4 lists
the same):
  M1  the low half decoded without sign extension        -> all 41: every test reads an int16 image against a model, tfm_hmc or the
                                                            long records' sums (a negative even plane reads 65536 too high)
  M2  planes 0 and 1 swapped in the quad epilogue        -> all 41
  M3  the quad offset dropped from the record base       -> 37: every test with two quads in one launch, test_records_and_second_quad_
                                                            beyond_four_gib included (not: the two 1153-workgroup cases of
                                                            test_large_images_take_several_launches — one quad per launch — and the
                                                            single long quad of test_long_records_and_32_bit_offsets_inside_a_record)
  M4  the diagonal weighted 2, one-table quad kernel     -> 20: every one-table case, first of all test_stacks_against_the_exact_model
                                                            [*-one_table] at all eleven sizes; no two-table case
  M5  s_ji gathered at s_ij, two-table quad kernel       -> 20: every two-table case but n_e = 1 (a lone diagonal has no pair), first of
                                                            all test_stacks_against_the_exact_model[*-two_tables]
  M6  the absent-frame stores not skipped                -> NOT RUN: the mutant stores rows past the end of the images wherever a test
                                                            gives exactly n_frames rows, and an out-of-bounds store is not a wrong-answer
                                                            mutation.  By reading: test_dev_entries_are_the_host_twin_and_leave_the_row_
                                                            after_a_ragged_stack checks the sentinel row after 5, 6, 7 and 1 frames, on
                                                            both routes, which such a store overwrites.
"""
import numpy as np
import pytest

import das_exact_numpy as D
from test_gpu_tfm_frames import _dev, _f32, _same, _t
from test_tfm_frames_hmc_cpu import N_SETS, record_sets

pytestmark = pytest.mark.gpu

N_FRAMES = (1, 2, 3, 4, 5, 9)                                            # every raggedness of the last quad and pair
_made = {}


def _case(n_e, two):
    """D.hmc_case's tables with ten int16 frames -> (case, stack int16 [10, n_pairs, N_T], [model image of frame k]): frame 2 k is the
    real, frame 2 k + 1 the imaginary plane of record set k; the model D.tfm_hmc on the set (its S.re reads the real plane alone, its
    S.im the imaginary one: test_tfm_frames_hmc_cpu.py)"""
    if (n_e, two) not in _made:
        c = D.hmc_case(n_e, two)
        a = record_sets(n_e)
        planes = [p for k in range(N_SETS) for p in (a[k].real, a[k].imag)]
        stack = np.stack(planes).astype(np.int16)
        assert np.array_equal(stack.astype(np.float32), np.stack(planes))          # the conversion is exact
        want = []
        for k in range(N_SETS):
            S = D.tfm_hmc(a[k], c["fs"], c["t0"], c["tt_tx"], c["tt_rx"])["S"]
            want += [_f32(S.real), _f32(S.imag)]
        stack.flags.writeable = False
        _made[(n_e, two)] = (c, stack, want)
    return _made[(n_e, two)]


def _tables(c, sel=None):
    """the tables as the call gets them: one table -> tt_rx None (the same pointer)"""
    pick = (lambda t: t) if sel is None else (lambda t: np.ascontiguousarray(t[:, sel]))
    return pick(c["tt_tx"]), (None if c["tt_rx"] is None else pick(c["tt_rx"]))


def _both(rtus, stack, what, want, *args, **kw):
    """tfm_frames(hmc=True) on the int16 stack and on the same stack as float32 against ``want``"""
    _same(rtus.tfm_frames(stack, *args, hmc=True, **kw), want, f"{what}, int16")
    _same(rtus.tfm_frames(stack.astype(np.float32), *args, hmc=True, **kw), want, f"{what}, float32")


# ------------------------------------------------------------------------------------------------------------ 1: the exact model
@pytest.mark.parametrize("two", [False, True], ids=["one_table", "two_tables"])
@pytest.mark.parametrize("n_e", D.HMC_SIZES)
def test_stacks_against_the_exact_model(rtus, n_e, two):
    """a lone diagonal (1), partial column blocks (15, 17, 31, 33), a full block (16), the two-table tile edge (32), the one-table
    tile edge (64), one element past it (65), several tiles and a partial block (48, 81); stacks of 1 .. 9 frames: frame k against
    the model of frame k; the no-path column is zero; frames 3 .. 7: other partners in a quad and a pair."""
    c, stack, want = _case(n_e, two)
    tt_tx, tt_rx = _tables(c)
    for n in N_FRAMES:
        for s in (stack[:n], stack[:n].astype(np.float32)):
            got = rtus.tfm_frames(s, c["fs"], tt_tx, tt_rx, t0=c["t0"], hmc=True)
            _same(got, np.stack(want[:n]), f"n_e = {n_e}, {n} frames, {s.dtype}")
            assert np.all(got[:, c["cols"]["no_path"]] == 0)
    _both(rtus, stack[3:8], f"n_e = {n_e}, frames 3 .. 7", np.stack(want[3:8]), c["fs"], tt_tx, tt_rx, t0=c["t0"])
    if not two:                                                          # equal tables through two pointers: the two-table kernels' bits
        _both(rtus, stack[:9], f"n_e = {n_e}, a copy of the table", np.stack(want[:9]), c["fs"], tt_tx, tt_tx.copy(), t0=c["t0"])


# ------------------------------------------------------------------------------------------------------------ 2: full-range data
FS_R, N_T_R, N_F_R, T0_R = 40.0e6, 300, 700, 0.25e-6


def _full_range_case(rtus, n_e, two):
    """six frames of a capture of n_e elements, 300 samples uniform over the whole int16 range; record (0, 0) of every frame
    alternates -32768 and 32767 and record (0, 1) alternates -1 and 1, each frame the other way round than its neighbour: in the
    packed layout every dword of these records has a negative half beside a positive one, in both orders.  Random times: positions
    over [-8, n_t + 8] samples, off every lattice, 2 % of the legs NaN; 700 focal points: three workgroups, the third ragged.
    -> (stack, tt_tx, tt_rx | None, [api.tfm_hmc of frame k as float32])"""
    key = ("full", n_e, two)
    if key not in _made:
        rng = np.random.default_rng(2026 + n_e)
        n_pairs = n_e * (n_e + 1) // 2
        stack = rng.integers(-32768, 32768, (6, n_pairs, N_T_R)).astype(np.int16)
        t = np.arange(N_T_R)
        for k in range(6):
            stack[k, 0] = np.where((t + k) % 2, -32768, 32767)
            stack[k, 1] = np.where((t + k) % 2, 1, -1)
        assert stack.min() == -32768 and stack.max() == 32767
        tt = [(rng.uniform(-4.0, N_T_R / 2 + 4.0, (n_e, N_F_R)) / FS_R + 0.5 * T0_R) for _ in range(2)]
        for v in tt:
            v[rng.random(v.shape) < 0.02] = np.nan
        tt_rx = tt[1] if two else None
        want = np.stack([rtus.tfm_hmc(stack[k].astype(np.float32), FS_R, tt[0], tt_rx, t0=T0_R) for k in range(6)])
        for v in (stack, want, *tt):
            v.flags.writeable = False
        _made[key] = (stack, tt[0], tt_rx, want)
    return _made[key]


@pytest.mark.parametrize("two", [False, True], ids=["one_table", "two_tables"])
@pytest.mark.parametrize("n_e", [33, 64])
def test_each_frame_is_tfm_hmc_of_it(rtus, n_e, two):
    stack, tt_tx, tt_rx, want = _full_range_case(rtus, n_e, two)
    assert np.count_nonzero(want) > 0.9 * want.size
    _both(rtus, stack, "six frames", want, FS_R, tt_tx, tt_rx, t0=T0_R)
    for n in (1, 2, 3, 5):                                               # no bit depends on n_frames or on the partners
        _both(rtus, stack[1:1 + n], f"frames 1 .. {n}", want[1:1 + n], FS_R, tt_tx, tt_rx, t0=T0_R)


# ------------------------------------------------------------------------------------------------------------ 3: workgroup order
@pytest.mark.parametrize("two", [False, True], ids=["one_table", "two_tables"])
@pytest.mark.parametrize("n_e", [17, 64])
def test_eight_workgroups_per_image_in_xcd_order(rtus, n_e, two):
    """the tables tiled to 2048 focal points: eight workgroups per image, the XCD-contiguous branch of the workgroup order; nine
    frames: three quads, five pairs.  A wrong block index moves whole blocks of 256 columns or whole images."""
    c, stack, want = _case(n_e, two)
    sel = np.arange(2048) % D.N_F
    tt_tx, tt_rx = _tables(c, sel)
    _both(rtus, stack[:9], f"n_e = {n_e}", np.stack([w[sel] for w in want[:9]]), c["fs"], tt_tx, tt_rx, t0=c["t0"])


# ------------------------------------------------------------------------------------------------------------ 4: several launches
# A call cuts its stack into launches of about 2304 workgroups (rtus_tfm_hmc.hip): 2304 // n_blk quads (pairs) per launch, one at least
PER_LAUNCH_2, PER_LAUNCH_1 = 1152 * 256, 1153 * 256                      # the last size with two blocks per launch, the first with one


@pytest.mark.parametrize("n_e,two,n_f", [(2, True, PER_LAUNCH_2), (2, True, PER_LAUNCH_1), (2, False, PER_LAUNCH_1), (16, False, PER_LAUNCH_2)],
                         ids=["2_two_per_launch", "2_one_per_launch", "2_one_table_one_per_launch", "16_two_per_launch"])
def test_large_images_take_several_launches(rtus, n_e, two, n_f):
    """the tables tiled to 1152 and to 1153 workgroups per image, five frames: two quads in launches of 2 and of 1 + 1, three pairs
    in launches of 2 + 1 and of 1 + 1 + 1; the offsets of the data and the images between the launches."""
    if n_e == 2:
        c = D.hmc_case(17, two)                                          # (2 is not one of the model's sizes: the first two rows of 17's tables)
        a = D.records(np.random.default_rng(77), (3, 3, D.N_T))
        tx, rx = c["tt_tx"][:2], (None if c["tt_rx"] is None else c["tt_rx"][:2])
        planes = [p for k in range(3) for p in (a[k].real, a[k].imag)][:5]
        stack = np.stack(planes).astype(np.int16)
        S = [D.tfm_hmc(a[k], c["fs"], c["t0"], tx, rx)["S"] for k in range(3)]
        want = [_f32(v) for k in range(3) for v in (S[k].real, S[k].imag)][:5]
    else:
        c, stack, want = _case(n_e, two)
        tx, rx = c["tt_tx"], c["tt_rx"]
        stack, want = stack[:5], want[:5]
    sel = np.arange(n_f) % D.N_F
    tx, rx = np.ascontiguousarray(tx[:, sel]), (None if rx is None else np.ascontiguousarray(rx[:, sel]))
    _both(rtus, stack, f"n_e = {n_e}", np.stack([w[sel] for w in want]), c["fs"], tx, rx, t0=c["t0"])


# ------------------------------------------------------------------------------------------------------------ 5: chunking
def test_max_frames_changes_no_bit(rtus):
    stack, tt_tx, tt_rx, want = _full_range_case(rtus, 33, True)
    for per in (1, 3, 4):
        _both(rtus, stack, f"in chunks of {per}", want, FS_R, tt_tx, tt_rx, t0=T0_R, max_frames=per)
    out = np.zeros_like(want)
    assert rtus.tfm_frames(stack, FS_R, tt_tx, tt_rx, t0=T0_R, out=out, hmc=True) is out and np.array_equal(out, want)


# ------------------------------------------------------------------------------------------------------------ 6, 7: the _dev entries
def _routes(torch, dev):
    """(name, dtype of the stack, frames per block, pack wrapper, imaging wrapper)"""
    return (("int16", torch.int16, 4, dev.fmc_pack_frames_i16_dev, dev.tfm_frames_hmc_i16_dev),
            ("float32", torch.float32, 2, dev.fmc_pack_frames_dev, dev.tfm_frames_hmc_dev))


@pytest.mark.parametrize("two", [False, True], ids=["one_table", "two_tables"])
def test_dev_entries_are_the_host_twin_and_leave_the_row_after_a_ragged_stack(rtus, two):
    """the existing pack wrappers on a [n_frames, 1, n_pairs, n_t] view + the _dev entries against tfm_frames(hmc=True) (the host
    twin of the same build) and against api.tfm_hmc.  The outputs are views big[:n_frames] of tensors one frame longer filled with a
    sentinel: the row after the last frame keeps it — the absent frames' stores are skipped."""
    torch, dev = _dev()
    stack, tt_tx, tt_rx, want = _full_range_case(rtus, 33, two)
    tx = _t(torch, tt_tx)
    rx = None if tt_rx is None else _t(torch, tt_rx)
    sentinel = -12345.0
    for name, dtype, per, pack, image in _routes(torch, dev):
        for n in (5, 6, 7, 1):
            s = stack[np.arange(n) % 6]                                  # (seven frames: the six and the first again)
            w = want[np.arange(n) % 6]
            _same(rtus.tfm_frames(s if per == 4 else s.astype(np.float32), FS_R, tt_tx, tt_rx, t0=T0_R, hmc=True), w, f"{name} host twin, {n}")
            packed = pack(_t(torch, s).to(dtype)[:, None])[:, 0]
            assert tuple(packed.shape) == ((n + per - 1) // per, s.shape[1], N_T_R, per)
            big = torch.full((n + 1, N_F_R), sentinel, dtype=torch.float32, device="cuda")
            got = image(packed, n, FS_R, tx, rx, t0=T0_R, out=big[:n])
            assert got.data_ptr() == big.data_ptr()
            host = big.cpu().numpy()
            _same(host[:n], w, f"{name}, {n} frames")
            assert np.all(host[n] == sentinel), f"{name}, {n} frames: the row after the last frame was written"
        full = pack(_t(torch, stack).to(dtype)[:, None])[:, 0]           # six frames: two quads (5 .. 8), three pairs (5, 6)
        for bad in (9 if per == 4 else 7, 4, 0):
            with pytest.raises(ValueError):
                image(full, bad, FS_R, tx, rx)
        with pytest.raises(ValueError):
            image(full.to(torch.float64), 6, FS_R, tx, rx)
        with pytest.raises(ValueError):
            image(full, 6, FS_R, tx[:32], rx)
        with pytest.raises(ValueError):
            image(full[:, None], 6, FS_R, tx, rx)
        with pytest.raises(ValueError):
            image(full, 6, FS_R, tx, rx, out=torch.empty(N_F_R, dtype=torch.float32, device="cuda"))


def test_capture_and_replay_of_the_two_dev_calls(rtus):
    """pack + rtus_tfm_frames_hmc_i16_dev and pack + rtus_tfm_frames_hmc_dev captured once in a torch.cuda.graph and replayed: the
    same bits (the _dev entries allocate nothing and do not synchronise)"""
    torch, dev = _dev()
    stack, tt_tx, tt_rx, want = _full_range_case(rtus, 33, True)
    tx, rx = _t(torch, tt_tx), _t(torch, tt_rx)
    n_pairs = stack.shape[1]
    d16 = _t(torch, stack)[:, None]
    d32 = d16.to(torch.float32)
    p16 = torch.empty((2, 1, n_pairs, N_T_R, 4), dtype=torch.int16, device="cuda")
    p32 = torch.empty((3, 1, n_pairs, N_T_R, 2), dtype=torch.float32, device="cuda")
    o16, o32 = (torch.empty((6, N_F_R), dtype=torch.float32, device="cuda") for _ in range(2))

    def run():
        dev.fmc_pack_frames_i16_dev(d16, out=p16)
        dev.tfm_frames_hmc_i16_dev(p16[:, 0], 6, FS_R, tx, rx, t0=T0_R, out=o16)
        dev.fmc_pack_frames_dev(d32, out=p32)
        dev.tfm_frames_hmc_dev(p32[:, 0], 6, FS_R, tx, rx, t0=T0_R, out=o32)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                       # warm-up off the default stream, as torch.cuda.graph wants
        run()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    _same(o16.cpu().numpy(), want, "int16 before the capture")
    _same(o32.cpu().numpy(), want, "float32 before the capture")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                        # one capture stream: the four kernels in sequence
        run()
    p16.fill_(-21846); p32.fill_(float("nan")); o16.fill_(float("nan")); o32.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    _same(o16.cpu().numpy(), want, "int16 replayed")
    _same(o32.cpu().numpy(), want, "float32 replayed")


# ------------------------------------------------------------------------------------------------------------ 8: offsets
LONG_TARGETS = [-4.0, -0.5, 0.0, 0.5, 3.0, 6.5, 7.5, 9.0, 2.0 ** 21, 2.0 ** 22 - 10.5, 2.0 ** 22 - 8.5, 2.0 ** 22 - 4.5, 2.0 ** 22 - 2.5,
                2.0 ** 22 - 2.0, 2.0 ** 22 - 1.0, 2.0 ** 22 - 0.5, 2.0 ** 22, 2.0 ** 22 + 4.0]


def _long_case(n_t, n_e, targets, seed, two):
    """records of a capture of n_e elements that are zero but for integers on their first and last eight samples, and legs in samples
    (fp32 numbers, exact sums).  Two tables: s_ij = targets[f] + j - i, s_ji = targets[f] + i - j; one table: s_ij = targets[f] + i + j.
    -> (head, tail complex [n_pairs, 8], tau_tx [n_e, n_f], tau_rx | None, S complex128 [n_f]: D.tfm_hmc's sum, through D.sparse_value)"""
    rng = np.random.default_rng(seed)
    n_pairs = n_e * (n_e + 1) // 2
    part = lambda: rng.integers(1, 5, (n_pairs, 8)) * rng.choice([-1.0, 1.0], (n_pairs, 8))     # noqa: E731  (no zero among them)
    head, tail = (part() + 1j * part() for _ in range(2))
    p = np.asarray(targets, dtype=np.float64)
    e = np.arange(n_e)[:, None]
    if two:
        half = np.floor(p / 2)
        tau_tx, tau_rx = half[None, :] - e, (p - half)[None, :] + e
    else:
        tau_tx, tau_rx = (p / 2)[None, :] + e, None
    for t in (tau_tx, tau_tx if tau_rx is None else tau_rx):
        assert np.array_equal(t.astype(np.float32).astype(np.float64), t)
    t32 = tau_tx.astype(np.float32)
    r32 = t32 if tau_rx is None else tau_rx.astype(np.float32)
    S = np.zeros(p.size, dtype=np.complex128)
    for i in range(n_e):
        for j in range(i, n_e):
            r = D.packed_index(i, j, n_e)
            S += D.sparse_value(head[r], tail[r], n_t, (t32[i] + r32[j]).astype(np.float32))
            if j > i:
                S += D.sparse_value(head[r], tail[r], n_t, (t32[j] + r32[i]).astype(np.float32))
    return head, tail, tau_tx, tau_rx, S


def _fill(torch, block, parts, n_t, dtype):
    """the sparse records into one block [n_pairs, n_t, P] of a packed stack on the device: parts = [(head, tail)] of one or two long
    cases; planes 0, 1 the real and imaginary parts of the first, planes 2, 3 of the second.  Only the sixteen samples that the
    targets can touch are written."""
    for k, (head, tail) in enumerate(parts):
        for part, where in ((head, slice(0, 8)), (tail, slice(n_t - 8, n_t))):
            v = np.stack([part.real, part.imag], axis=-1).astype(dtype)
            block[:, where, 2 * k:2 * k + 2] = torch.as_tensor(v, device="cuda")


@pytest.mark.parametrize("two", [False, True], ids=["one_table", "two_tables"])
def test_long_records_and_32_bit_offsets_inside_a_record(rtus, two):
    """n_t = 2^22 at n_e = 3, one quad of four frames made on the device: six records of 2^25 bytes each, zero but for the first and
    last eight samples of each plane, so a byte offset that wrapped, lost its high bits or was scaled for another record size reads
    zeros or the wrong end.  The quad read as four, three, two and one frames; the first two frames as a float32 pair besides."""
    torch, dev = _dev()
    n_t, fs, n_e = 2 ** 22, D.FS, 3
    parts, S = [], []
    for seed in (31, 32):
        head, tail, tau_tx, tau_rx, s = _long_case(n_t, n_e, LONG_TARGETS, seed, two)   # (the legs depend on the targets only)
        parts.append((head, tail))
        S += [_f32(s.real), _f32(s.imag)]
    assert all(np.count_nonzero(s) >= 5 for s in S) and len({s.tobytes() for s in S}) == 4
    tt = torch.as_tensor(tau_tx / fs, device="cuda")
    tr = None if tau_rx is None else torch.as_tensor(tau_rx / fs, device="cuda")
    packed = torch.zeros((1, 6, n_t, 4), dtype=torch.int16, device="cuda")
    _fill(torch, packed[0], parts, n_t, np.int16)
    for n in (4, 3, 2, 1):
        _same(dev.tfm_frames_hmc_i16_dev(packed, n, fs, tt, tr).cpu().numpy(), np.stack(S[:n]), f"{n} frames of long records")
    del packed
    pair = torch.zeros((1, 6, n_t, 2), dtype=torch.float32, device="cuda")
    _fill(torch, pair[0], parts[:1], n_t, np.float32)
    for n in (2, 1):
        _same(dev.tfm_frames_hmc_dev(pair, n, fs, tt, tr).cpu().numpy(), np.stack(S[:n]), f"{n} float32 frames of long records")
    del pair
    torch.cuda.empty_cache()


def test_records_and_second_quad_beyond_four_gib(rtus):
    """five frames of a 16-element capture of 2^22 samples: a quad's block is 136 records of 2^25 bytes, 4.6 GB — records 128 .. 135
    of quad 0 lie beyond 4 GiB (the 64-bit row / down / past steps of the walk), and quad 1 starts beyond 4 GiB (the quad offset):
    9.1 GB on the device, zero-filled there, no host copy.  The quads hold different records; one table, so every record counts."""
    torch, dev = _dev()
    n_t, fs, n_e = 2 ** 22, D.FS, 16
    packed = torch.zeros((2, 136, n_t, 4), dtype=torch.int16, device="cuda")
    assert packed[1].data_ptr() - packed[0].data_ptr() == 136 * 2 ** 25 > 2 ** 32
    assert packed[0, 128].data_ptr() - packed.data_ptr() == 2 ** 32
    targets = [0.0, 3.5, 9.0, 2.0 ** 22 - 38.5, 2.0 ** 22 - 31.0, 2.0 ** 22 - 8.5, 2.0 ** 22 - 1.0, 2.0 ** 22 + 4.0]
    want, quads = [], [[], []]
    for k, q in ((0, 0), (1, 0), (2, 1)):
        head, tail, tau_tx, _, s = _long_case(n_t, n_e, targets, 40 + k, False)
        quads[q].append((head, tail))
        want += [_f32(s.real), _f32(s.imag)]
    for q in range(2):
        _fill(torch, packed[q], quads[q], n_t, np.int16)
    assert not np.array_equal(want[0], want[4]) and np.count_nonzero(want[4]) >= 3
    tt =torch.as_tensor(tau_tx / fs, device="cuda")
    got = dev.tfm_frames_hmc_i16_dev(packed, 5, fs, tt).cpu().numpy()
    _same(got, np.stack(want[:5]), "five frames, the fifth beyond 4 GiB")
    del packed
    torch.cuda.empty_cache()

"""GPU: the delay-and-sum family BIT FOR BIT against tests/das_exact_numpy.py — rtus_tfm, rtus_tfm_analytic (+ cf), rtus_tfm_weighted
(+ sensitivity), rtus_tfm_phase (image, counts, scf; vcf within its bound), rtus_tfm_iq, the half-matrix forms of the first, second
and last, and rtus_fmc_synth_tx — at record edges, at the 1e8 leg limit and at every tile seam.

Why no tolerance: the inputs follow the generator rules of tests/das_exact_numpy.py (fs = 2^25, times on the 1/4-sample lattice,
integer records, Gaussian-integer weights, n_tx n_rx <= 2^13), under which no operation that include/rtus.h prescribes rounds — not
a leg, not a position (but in the columns built so that it does), not an interpolation, not a partial sum in ANY order.
tests/test_das_exact_cpu.py proves each of these premises without a GPU.  So a plain loop over the pairs is the kernels' result,
whatever their order of summation, and every comparison here is np.array_equal (cf and scf: with equal NaNs).  The one exception is
vcf: its unit phasors go through the hardware's reciprocal square root, so it is held to test_gpu_tfm_phase.py's bar VCF_BAR (the
derivation is there; every N here is below that file's 4900).

What the shapes reach: (1, 1); a tail of fifteen gathers, one full group of sixteen, a group and a tail of one, three groups and a
tail (the weighted kernel: one, one, two and four receive tiles); 64 x 64 with ONE table (the transmit delay read from the tile)
and with an equal copy as tt_rx (formed again); 65 x 65 with one table (two tiles: not in the tile); 4 x 129 (three tiles).  Half
matrix: 1, 15, 16, 17, 31, 32, 33, 48, 64, 65, 81 elements — either side of every block of sixteen columns, of the 32-element tile
of the two-table form and of the 64-element tile of the one-table form — each with one table and with two different ones.  257
focal points (two workgroups, the second ragged), once tiled to 2048 (eight workgroups: the XCD-contiguous order).  Synthesis:
127, 128, 129, 257 transmit elements (either side of the 128-element tile of shifts, and three tiles), 1, 8, 9 laws (either side of
a group of eight), 255, 256, 257 samples (either side of a workgroup).  Long records on the device: 2^22 samples, and 2^26 (the
limit: 16-byte samples at 32-bit byte offsets) with one pair.

Each test names the kernel changes that it was seen to catch.  The six changes were each made once on a scratch build, which this
file was then run against on MI355X (none can fault: every load stays range-checked and every offset only shrinks).  The counts are
of the 78 delay-and-sum and 36 synthesis tests of that run; the whole-sample half-matrix test ran at 33 elements only then:
  M1  das_load2 without the clamp of negative indices (min((unsigned) i, ...) removed; the load stays range-checked).
      NOT CAUGHT: 78 of 78 delay-and-sum comparisons pass.  The clamp-less kernel issues the same buffer_load_dwordx2 / x4 at
      byte offset 0xFFFFFFFC / 0xFFFFFFF8 for index -1, and gfx950 returns zeros for both samples: the change is no change on
      this hardware.  Every case holds >= 257 pairs at index -1 with w in {1/4, 1/2, 3/4, 1 - 2^-23} over non-zero first samples
      (tests/test_das_exact_cpu.py's census), so a wrap to sample 0 would show in every image test below.
  M2  das_clamp with <= for <: a leg on the float32 1e8 has a path.  76 of 78 fail.
  M3  weight 2 on the diagonal of the half matrix (one table) / the diagonal's term doubled (two tables).  All 26 tests that
      run a half-matrix kernel fail, nothing else.
  M4  r0 dropped from the record offset in rtus_tfm.hip (RF, analytic / IQ, phase, weighted): a later receive tile reads the
      first tile's records.  15 fail: every shape with more than one tile.
  M5  synth_term without `lead`: index -1 is clamped away like every other negative index.  36 of 36 synthesis cases fail.
  M6  the synthesis kernel's delay index without `t0 +`: a later tile of transmit elements gets the first tile's shifts.  The 18
      cases with n_tx > 128 fail.
The same table is in DESIGN.md §2 ("Delay-and-sum family: pinned bit for bit on exact inputs").
"""
import numpy as np
import pytest

import das_exact_numpy as D
import pwi_numpy as PW
import tfm_phase_numpy as TP

pytestmark = pytest.mark.gpu

VCF_BAR = 3.0e-7                     # test_gpu_tfm_phase.py's (its module docstring derives it; it needs N <= 4900)
FULL = list(D.FULL_CASES)
WHOLE_FULL = ("5x63", "64x64_one")
NUS = (0.125, 0.25, 0.49)            # carrier frequencies in cycles per sample, exact in fp32 or not


def _c64(z):
    """the model's exact complex sum as the kernels store it"""
    got = np.asarray(z).astype(np.complex64)
    assert np.array_equal(got.astype(np.complex128), z)
    return got


def _f32(x):
    got = np.asarray(x).astype(np.float32)
    assert np.array_equal(got.astype(np.float64), np.asarray(x, dtype=np.float64), equal_nan=True)
    return got


def _same(got, want, what, equal_nan=False):
    """bit equality up to the sign of a zero (a sum that starts at +0 never shows one), with the first differences in the message"""
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape)
    if not np.array_equal(got, want, equal_nan=equal_nan):
        bad = np.nonzero(~((got == want) | (equal_nan & np.isnan(got) & np.isnan(want))))[0]
        raise AssertionError(f"{what}: {bad.size} of {got.size} focal points differ; first at {bad[:8]}: got {got[bad[:8]]}, "
                             f"expected {want[bad[:8]]}")


def _tables(c, sel=None):
    """the tables as the call gets them: one table -> tt_rx None (the same pointer)"""
    pick = (lambda t: t) if sel is None else (lambda t: np.ascontiguousarray(t[:, sel]))
    return pick(c["tt_tx"]), (None if c["tt_rx"] is None else pick(c["tt_rx"]))


@pytest.mark.parametrize("name", FULL)
def test_rf_image_of_each_plane(rtus, name):
    """rtus_tfm on the real and on the imaginary plane.  Fails under M2 (all but 1x1_one: 1e8 + (8 - 99999992) lands on sample 16,
    1e8 + (-1e8) on sample 0) and M4 (65x65_one, 4x129)."""
    c, m = D.full_case(name), D.full_model(name)
    tt_tx, tt_rx = _tables(c)
    for part, want in (("re", m["S"].real), ("im", m["S"].imag)):
        plane = np.ascontiguousarray(getattr(c["a"], "real" if part == "re" else "imag"))
        _same(rtus.tfm_image(plane, c["fs"], tt_tx, tt_rx, t0=c["t0"]), _f32(want), f"{name} {part}")


@pytest.mark.parametrize("name", FULL)
def test_analytic_image_and_cf(rtus, name):
    """rtus_tfm_analytic without and with cf; cf from the model's exact S, E and N = T R by the header's fp64 formula.  Fails
    under M2 (every case; 1x1_one by cf alone: N = 1 where the one leg is 1e8) and M4 (65x65_one, 4x129)."""
    c, m = D.full_case(name), D.full_model(name)
    tt_tx, tt_rx = _tables(c)
    want = _c64(m["S"])
    _same(rtus.tfm_analytic(c["a"], c["fs"], tt_tx, tt_rx, t0=c["t0"]), want, f"{name} image")
    img, cf = rtus.tfm_analytic(c["a"], c["fs"], tt_tx, tt_rx, t0=c["t0"], coherence=True)
    _same(img, want, f"{name} image with cf")
    _same(cf, D.cf_header(m["S"], m["E"], m["N"]), f"{name} cf", equal_nan=True)
    assert np.isnan(cf[c["cols"]["no_path"]]) and img[c["cols"]["no_path"]] == 0


@pytest.mark.parametrize("name", FULL)
def test_weighted_image_and_sensitivity(rtus, name):
    """rtus_tfm_weighted with sens: receive tiles of sixteen, NaN and infinite weights.  Fails under M2 (every case) and M4 (2x17, 5x63,
    both 64x64, 65x65_one, 4x129: its tile is sixteen)."""
    c, m = D.full_case(name), D.full_model(name)
    tt_tx, tt_rx = _tables(c)
    img, sens = rtus.tfm_weighted(c["a"], c["fs"], tt_tx, c["w_tx"], tt_rx, c["w_rx"], t0=c["t0"], sensitivity=True)
    _same(img, _c64(m["S_w"]), f"{name} weighted image")
    _same(sens, _f32(m["P"]), f"{name} sensitivity")


@pytest.mark.parametrize("name", FULL)
def test_phase_image_counts_scf_and_vcf(rtus, name):
    """rtus_tfm_phase: the image; (B, N) as integers; scf from them by the header's formula, bit for bit; vcf within VCF_BAR of the
    fp64 phasor sum.  Fails under M2 (every case: N, scf, image) and M4 (65x65_one, 4x129)."""
    c, m = D.full_case(name), D.full_model(name)
    tt_tx, tt_rx = _tables(c)
    r = rtus.tfm_phase(c["a"], c["fs"], tt_tx, tt_rx, t0=c["t0"], counts=True)
    _same(r["image"], _c64(m["S"]), f"{name} image")
    _same(r["n_pairs"], m["N"].astype(np.int32), f"{name} N")
    _same(r["sign_sum"], m["B"].astype(np.int32), f"{name} B")
    _same(r["scf"], D.scf_header(m["B"], m["N"]), f"{name} scf", equal_nan=True)
    assert m["N"].max() <= 4900
    want = TP.vcf_of(m["U"], m["N"])
    assert np.array_equal(np.isnan(r["vcf"]), np.isnan(want))
    fin = ~np.isnan(want)
    err = float(np.max(np.abs(r["vcf"][fin].astype(np.float64) - want[fin])))
    print(f"{name}: vcf {err:.2e} (bar {VCF_BAR:.1e})")
    assert err <= VCF_BAR and np.all((r["vcf"][fin] >= 0) & (r["vcf"][fin] <= 1))


@pytest.mark.parametrize("name", FULL)
def test_iq_at_zero_carrier(rtus, name):
    """rtus_tfm_iq at f_demod = 0, every position: R = (1, +0) and the phasor (1, 0) multiply exactly.  Fails under M2 (every case) and M4 (65x65_one, 4x129)."""
    c, m = D.full_case(name), D.full_model(name)
    tt_tx, tt_rx = _tables(c)
    img, cf = rtus.tfm_iq(c["a"], c["fs"], 0.0, tt_tx, tt_rx, t0=c["t0"], coherence=True)
    _same(img, _c64(m["S"]), f"{name} image")
    _same(cf, D.cf_header(m["S"], m["E"], m["N"]), f"{name} cf", equal_nan=True)
    _same(rtus.tfm_iq(c["a"], c["fs"], 0.0, tt_tx, tt_rx, t0=c["t0"]), _c64(m["S"]), f"{name} image without cf")


@pytest.mark.parametrize("name", WHOLE_FULL)
def test_iq_on_whole_samples_at_any_carrier(rtus, name):
    """every position a whole sample: w = 0, b = fmaf(0, q - a0, a0) = a0 and the phasor at x = nu 0 is (1, 0), so the step returns
    a0 exactly whatever R is — the linear model, at three carriers.  This pins the IQ step itself at f_demod != 0: a step that
    took R, w or nu wrongly shows here and nowhere above.  Fails under M2 (both cases; both are one tile: M4 is silent)."""
    c, m = D.full_case(name, whole=True), D.full_model(name, whole=True)
    tt_tx, tt_rx = _tables(c)
    for nu in NUS:
        img, cf = rtus.tfm_iq(c["a"], c["fs"], nu * c["fs"], tt_tx, tt_rx, t0=c["t0"], coherence=True)
        _same(img, _c64(m["S"]), f"{name} nu = {nu} image")
        _same(cf, D.cf_header(m["S"], m["E"], m["N"]), f"{name} nu = {nu} cf", equal_nan=True)


def test_eight_workgroups_in_xcd_order(rtus):
    """5x63 and the 33-element half matrix (one table) tiled to 2048 focal points: eight workgroups, das_workgroup()'s
    XCD-contiguous order; every kernel family once.  A wrong block index moves whole blocks of 256 columns.  Fails under M2, M3
    and M4 (the weighted kernel's four tiles)."""
    sel = np.arange(2048) % D.N_F
    c, m = D.full_case("5x63"), D.full_model("5x63")
    tt_tx, tt_rx = _tables(c, sel)
    w_tx, w_rx = np.ascontiguousarray(c["w_tx"][:, sel]), np.ascontiguousarray(c["w_rx"][:, sel])
    S, cf = _c64(m["S"])[sel], D.cf_header(m["S"], m["E"], m["N"])[sel]
    _same(rtus.tfm_image(np.ascontiguousarray(c["a"].real), c["fs"], tt_tx, tt_rx, t0=c["t0"]), S.real, "rf")
    img, got_cf = rtus.tfm_analytic(c["a"], c["fs"], tt_tx, tt_rx, t0=c["t0"], coherence=True)
    _same(img, S, "analytic"); _same(got_cf, cf, "cf", equal_nan=True)
    img, sens = rtus.tfm_weighted(c["a"], c["fs"], tt_tx, w_tx, tt_rx, w_rx, t0=c["t0"], sensitivity=True)
    _same(img, _c64(m["S_w"])[sel], "weighted"); _same(sens, _f32(m["P"])[sel], "sens")
    r = rtus.tfm_phase(c["a"], c["fs"], tt_tx, tt_rx, t0=c["t0"], counts=True)
    _same(r["image"], S, "phase"); _same(r["sign_sum"], m["B"].astype(np.int32)[sel], "B")
    _same(r["n_pairs"], m["N"].astype(np.int32)[sel], "N")
    img, got_cf = rtus.tfm_iq(c["a"], c["fs"], 0.0, tt_tx, tt_rx, t0=c["t0"], coherence=True)
    _same(img, S, "iq"); _same(got_cf, cf, "iq cf", equal_nan=True)
    c, m = D.hmc_case(33, False), D.hmc_model(33, False)
    tt_tx, _ = _tables(c, sel)
    S, cf = _c64(m["S"])[sel], D.cf_header(m["S"], m["E"], m["N"])[sel]
    _same(rtus.tfm_hmc(np.ascontiguousarray(c["h"].imag), c["fs"], tt_tx, t0=c["t0"]), S.imag, "hmc rf")
    img, got_cf = rtus.tfm_analytic_hmc(c["h"], c["fs"], tt_tx, t0=c["t0"], coherence=True)
    _same(img, S, "hmc analytic"); _same(got_cf, cf, "hmc cf", equal_nan=True)


@pytest.mark.parametrize("two", [False, True], ids=["one_table", "two_tables"])
@pytest.mark.parametrize("n_e", D.HMC_SIZES)
def test_half_matrix_family(rtus, n_e, two):
    """rtus_tfm_hmc on both planes, rtus_tfm_analytic_hmc without and with cf, rtus_tfm_iq_hmc at f_demod = 0 — the packed triangle,
    the pair first, the diagonal once.  Fails under M2 and under M3 (every size, both forms: the diagonal's terms double)."""
    c, m = D.hmc_case(n_e, two), D.hmc_model(n_e, two)
    tt_tx, tt_rx = _tables(c)
    what = f"n_e = {n_e}, {'two tables' if two else 'one table'}"
    S, cf = _c64(m["S"]), D.cf_header(m["S"], m["E"], m["N"])
    for part in ("real", "imag"):
        plane = np.ascontiguousarray(getattr(c["h"], part))
        _same(rtus.tfm_hmc(plane, c["fs"], tt_tx, tt_rx, t0=c["t0"]), getattr(S, part), f"{what} rf {part}")
    _same(rtus.tfm_analytic_hmc(c["h"], c["fs"], tt_tx, tt_rx, t0=c["t0"]), S, f"{what} analytic")
    img, got = rtus.tfm_analytic_hmc(c["h"], c["fs"], tt_tx, tt_rx, t0=c["t0"], coherence=True)
    _same(img, S, f"{what} analytic with cf"); _same(got, cf, f"{what} cf", equal_nan=True)
    img, got = rtus.tfm_iq_hmc(c["h"], c["fs"], 0.0, tt_tx, tt_rx, t0=c["t0"], coherence=True)
    _same(img, S, f"{what} iq"); _same(got, cf, f"{what} iq cf", equal_nan=True)
    _same(rtus.tfm_iq_hmc(c["h"], c["fs"], 0.0, tt_tx, tt_rx, t0=c["t0"]), S, f"{what} iq without cf")


@pytest.mark.parametrize("two", [False, True], ids=["one_table", "two_tables"])
@pytest.mark.parametrize("n_e", D.HMC_SIZES)
def test_half_matrix_iq_on_whole_samples_at_any_carrier(rtus, n_e, two):
    """as test_iq_on_whole_samples_at_any_carrier, every size and both forms of the half matrix.  Fails under M2 and M3."""
    c, m = D.hmc_case(n_e, two, whole=True), D.hmc_model(n_e, two, whole=True)
    tt_tx, tt_rx = _tables(c)
    for nu in NUS:
        img, cf = rtus.tfm_iq_hmc(c["h"], c["fs"], nu * c["fs"], tt_tx, tt_rx, t0=c["t0"], coherence=True)
        _same(img, _c64(m["S"]), f"nu = {nu} image")
        _same(cf, D.cf_header(m["S"], m["E"], m["N"]), f"nu = {nu} cf", equal_nan=True)


# ------------------------------------------------------------------------------------------------------------ long records
def _long_case(n_t, n_tx, n_rx, targets):
    """records that are zero but for integers on their first and last eight samples; legs whose fp32 sum is targets[f] + rx - tx
    -> (head, tail complex [n_tx, n_rx, 8], tau_tx [n_tx, n_f], tau_rx [n_rx, n_f] float64: fp32 numbers, in samples)"""
    rng = np.random.default_rng(n_t % 1000 + n_tx)
    part = lambda: rng.integers(1, 5, (n_tx, n_rx, 8)) * rng.choice([-1.0, 1.0], (n_tx, n_rx, 8))     # no zero among them
    head, tail = (part() + 1j * part() for _ in range(2))
    p = np.asarray(targets, dtype=np.float64)
    half = np.floor(p / 2)
    if n_t > 2 ** 24:                                                    # halves that fp32 holds up there: 2^25 + (p - 2^25), or 0 + p
        assert n_tx == n_rx == 1
        half = np.where(p >= 2.0 ** 25, 2.0 ** 25, 0.0)
    tau_tx = half[None, :] - np.arange(n_tx)[:, None]
    tau_rx = (p - half)[None, :] + np.arange(n_rx)[:, None]
    for t in (tau_tx, tau_rx):
        assert np.array_equal(t.astype(np.float32).astype(np.float64), t)
    return head, tail, tau_tx, tau_rx


def _long_model(head, tail, n_t, tau_tx, tau_rx):
    """S and E [n_f] of the full matrix: every leg has a path"""
    t32, r32 = tau_tx.astype(np.float32), tau_rx.astype(np.float32)
    S = np.zeros(tau_tx.shape[1], dtype=np.complex128)
    E = np.zeros(tau_tx.shape[1])
    for tx in range(t32.shape[0]):
        for rx in range(r32.shape[0]):
            p = D.sparse_value(head[tx, rx], tail[tx, rx], n_t, (t32[tx] + r32[rx]).astype(np.float32))
            S += p
            E += p.real ** 2 + p.imag ** 2
    return S, E


def _device_block(torch, head, tail, n_t):
    """float32 [n_tx, n_rx, n_t, 2] made on the device: no host copy of the block"""
    a = torch.zeros((*head.shape[:2], n_t, 2), dtype=torch.float32, device="cuda")
    for block, where in ((head, slice(0, 8)), (tail, slice(n_t - 8, n_t))):
        v = np.stack([block.real, block.imag], axis=-1).astype(np.float32)
        a[:, :, where, :] = torch.as_tensor(v, device="cuda")
    return a


def test_long_records_and_32_bit_byte_offsets(rtus):
    """n_t = 2^22 (2 x 3 pairs; positions on the half-sample lattice that fp32 still has there) and n_t = 2^26, the limit (one
    pair, 0.5 GB on the device, no host staging; fp32 positions are multiples of 4 there, two of the sums round: 2^26 - 6 onto
    2^26 - 8 and 2^26 - 2 onto n_t itself).  The records are zero except for their first and last eight samples, so a byte offset
    that wrapped, lost its high bits or was scaled wrongly reads zeros (or the wrong end).  Through the _dev entries: RF (2^22),
    analytic + cf, IQ at f_demod = 0, and the half matrix on the first three records (2^22).  Fails under M3 (the half matrix of
    two elements); every leg is far from 1e8 and every shape is one tile, so M2 and M4 are silent here."""
    import torch
    from importlib import import_module
    dev = import_module("ray-tracing-ultrasound_amd.device")
    fs = D.FS
    as_c = lambda t: t.cpu().numpy().view(np.complex64)[:, 0]
    for n_t, n_tx, n_rx, targets in (
            (2 ** 22, 2, 3, [-4.0, -0.5, 0.0, 0.5, 3.0, 6.5, 7.5, 9.0, 2.0 ** 21, 2.0 ** 22 - 10.5, 2.0 ** 22 - 8.5, 2.0 ** 22 - 4.5,
                             2.0 ** 22 - 2.5, 2.0 ** 22 - 2.0, 2.0 ** 22 - 1.0, 2.0 ** 22 - 0.5, 2.0 ** 22, 2.0 ** 22 + 4.0]),
            (2 ** 26, 1, 1, [-4.0, 0.0, 4.0, 8.0, 2.0 ** 25, 2.0 ** 26 - 12.0, 2.0 ** 26 - 8.0, 2.0 ** 26 - 6.0, 2.0 ** 26 - 4.0,
                             2.0 ** 26 - 2.0, 2.0 ** 26, 2.0 ** 26 + 8.0])):
        head, tail, tau_tx, tau_rx = _long_case(n_t, n_tx, n_rx, targets)
        S, E = _long_model(head, tail, n_t, tau_tx, tau_rx)
        n_f = tau_tx.shape[1]
        N = np.full(n_f, n_tx * n_rx)
        assert np.count_nonzero(S) >= 5
        a = _device_block(torch, head, tail, n_t)
        tt, tr = torch.as_tensor(tau_tx / fs, device="cuda"), torch.as_tensor(tau_rx / fs, device="cuda")
        cf = torch.empty(n_f, dtype=torch.float32, device="cuda")
        out, _ = dev.tfm_analytic_dev(a, fs, tt, tr, cf=cf)
        torch.cuda.synchronize()
        _same(as_c(out), _c64(S), f"n_t = {n_t} analytic")
        _same(cf.cpu().numpy(), D.cf_header(S, E, N), f"n_t = {n_t} cf", equal_nan=True)
        _same(as_c(dev.tfm_iq_dev(a, fs, 0.0, tt, tr)), _c64(S), f"n_t = {n_t} iq")
        if n_t == 2 ** 26:
            continue
        re = a[..., 0].contiguous()
        _same(dev.tfm_dev(re, fs, tt, tr).cpu().numpy(), _f32(S.real), f"n_t = {n_t} rf")
        del re
        # the half matrix of two elements on the block's first three records, one table (the transmit legs): (0, 0), (0, 1), (1, 1)
        h = a.reshape(n_tx * n_rx, n_t, 2)[:3]
        hh, ht = head.reshape(-1, 8)[:3], tail.reshape(-1, 8)[:3]
        t32 = tau_tx.astype(np.float32)
        terms = [D.sparse_value(hh[k], ht[k], n_t, (t32[i] + t32[j]).astype(np.float32)) for k, (i, j) in enumerate(((0, 0), (0, 1), (1, 1)))]
        S_h = terms[0] + 2.0 * terms[1] + terms[2]
        _same(as_c(dev.tfm_analytic_hmc_dev(h, fs, tt)), _c64(S_h), f"n_t = {n_t} half matrix")
        assert np.count_nonzero(S_h) >= 3
        del a, h
        torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------ synthesis
@pytest.mark.parametrize("n_t", [255, 256, 257])
@pytest.mark.parametrize("n_v", [1, 8, 9])
@pytest.mark.parametrize("n_tx", [127, 128, 129, 257])
def test_synthesis_of_transmit_laws(rtus, n_tx, n_v, n_t):
    """rtus_fmc_synth_tx against the plain exact loop and against tests/pwi_numpy.py's float32 emulation: integer records, shifts
    on the 1/4-sample lattice that put i = n - m on -1 (the kernel's own rule: sample 0 is the upper neighbour), 0, n_t - 1 and
    past either end; NaN, infinite and +-1e8 delays (not fired), +-(1e8 - 1/4) (fired, nothing in the record).  n_tx > 128: the
    second LDS tile of shifts.  Fails under M5 (every case: the terms with i = -1 and w > 0 lose w x[0]) and M6 (n_tx = 129, 257)."""
    fmc, d = D.synth_case(n_tx, n_v, n_t)
    want = D.synth(fmc, D.FS, d)
    assert np.array_equal(want, PW.synth(fmc, D.FS, d))
    got = rtus.fmc_synth_tx(fmc, D.FS, d)
    assert got.dtype == np.float32 and got.shape == want.shape
    if not np.array_equal(got, want):
        v, rx, n = (k[:8] for k in np.nonzero(got != want))
        raise AssertionError(f"{np.count_nonzero(got != want)} samples differ; first at (v, rx, n) = {list(zip(v, rx, n))}: got {got[v, rx, n]}, "
                             f"expected {want[v, rx, n]}")

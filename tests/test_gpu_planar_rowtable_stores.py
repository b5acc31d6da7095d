"""GPU: where the planar kernel's ROW TABLE path stores its rows (csrc/rtus_fermat.hip, DESIGN.md section 4 "Store stream"): the
layout-facing side of the served path, which tests/test_gpu_planar_rowtable.py leaves open.  Checked here: rows whose length is
odd (every second row starts 8 bytes off a 16-byte boundary), a last workgroup of 255 live targets and of one, values that
landed in the right element at the pair, half-wave, wave and workgroup seams, that nothing outside the launch's rows is written
(whole table and row shards, cut at block boundaries and inside blocks: a launch then holds 5, 27, 15 or 17 rows of a served block), the per-row
descriptors of the sorted entry, the batched entry, and a table of 131 rows.  They hold for any width of the store and any
order of the work items.

Shapes as tests/test_gpu_planar_rowtable.py: 150 elements at 0.3 mm, the configs[2] medium, a 256-column grid of 65,536 targets,
truncated where a test says so.  rows_per_block is 32 for them (37.5 by the waves, capped at 32 below the 64-row regime): four
blocks of 32 rows, which take the table, and a ragged one of 22, which takes the solver."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_E = 150
CFG3 = ([0.010, 0.025], [2330.0, 1483.0, 5900.0], (0.026, 0.066))
N_ODD = 65535                       # last workgroup: 255 live targets, a lone first-of-pair at the end of every row
N_ONE = 65281                       # last workgroup: one live target
SENTINEL = 0x7FF8DEADBEEF0001       # a NaN no solve produces


def _dev():
    import torch
    from importlib import import_module
    return torch, import_module("ray-tracing-ultrasound_amd.device")


def _t(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")


def _grid(width, zr):
    """an image grid of `width` columns with at least 65,536 targets"""
    n_rows = -(-65536 // width)
    x = (np.arange(width) - (width - 1) / 2.0) * (0.04 / (width - 1))
    xs, zs = np.meshgrid(x, np.linspace(zr[0], zr[1], n_rows))
    return xs.ravel(), zs.ravel()


def _aperture(n_e=N_E, pitch=0.3e-3):
    return (np.arange(n_e) - (n_e - 1) / 2.0) * pitch, np.zeros(n_e)


def _seams(n_f):
    """the pair, half-wave, wave and workgroup seams of the first and of the last workgroup, and both ends of a row"""
    last = (n_f - 1) // 256 * 256
    c = np.concatenate([[0, 1, 2], np.arange(126, 131), np.arange(253, 259), last + np.array([0, 1, 2]), last + np.arange(126, 131),
                        last + np.arange(253, 256), np.arange(n_f - 3, n_f)])
    return np.unique(c[(c >= 0) & (c < n_f)])


def _check(got, z_if, c, xe, ze, xf, zf, rows, cols):
    """the tier's bar (tests/test_gpu_planar_tiers.py): 1e-10 relative against the long-double oracle, identical NaN masks"""
    from oracle import cport
    want_nan = ~np.isfinite(xe[rows])[:, None] | (zf[cols][None, :] <= ze[rows][:, None])
    sub = got[np.ix_(rows, cols)]
    assert np.array_equal(np.isnan(sub), want_nan)
    fin = np.isfinite(xe[rows])
    ref = cport.tt_layers(z_if, c, xe[rows][fin], ze[rows][fin], xf[cols], zf[cols])
    m = ~want_nan[fin]
    assert np.array_equal(np.isnan(ref), ~m)
    err = np.abs(sub[fin] - ref)[m]
    rel = float((err / ref[m]).max())
    print(f"max relative error against the oracle {rel:.2e} over {int(m.sum())} solves")
    assert np.all(err <= 1e-16 + 1e-10 * ref[m]), rel


def _bits(t):
    import torch
    return t.view(torch.int64)


@pytest.fixture(scope="module")
def tables(rtus):
    """the 65,536-target table and its two truncations, one launch each, tau-p tier; shared, never modified"""
    torch, dev = _dev()
    z_if, c, zr = CFG3
    xe, ze = _aperture()
    xf, zf = _grid(256, zr)
    ebs = {n: dev.rows_per_block(N_E, n) for n in (xf.size, N_ODD, N_ONE)}
    assert set(ebs.values()) == {32}, ebs
    tt = {n: dev.tt_layers_dev(z_if, c, _t(xe), _t(ze), _t(xf[:n]), _t(zf[:n]), taup=True) for n in ebs}
    return dict(z_if=z_if, c=c, xe=xe, ze=ze, xf=xf, zf=zf, eb=32, tt=tt)


@pytest.mark.parametrize("n_f", [N_ODD, N_ONE])
def test_odd_row_length_against_the_oracle(rtus, tables, n_f):
    E = tables
    got = E["tt"][n_f].cpu().numpy()
    assert got.shape == (N_E, n_f) and np.isfinite(got).all()
    _check(got, E["z_if"], E["c"], E["xe"], E["ze"], E["xf"][:n_f], E["zf"][:n_f], np.arange(N_E), _seams(n_f))


@pytest.mark.parametrize("n_f", [N_ODD, N_ONE])
def test_truncated_tables_have_the_bits_of_the_whole_one(rtus, tables, n_f):
    """a served solve is a function of X, the depths and the medium: not of where its row starts, nor of its workgroup's other lanes"""
    torch, dev = _dev()
    E = tables
    assert dev.rows_per_block(N_E, n_f) == dev.rows_per_block(N_E, E["xf"].size) == E["eb"]
    whole = E["tt"][E["xf"].size][:, :n_f].contiguous()
    diff = int((_bits(whole) != _bits(E["tt"][n_f])).sum())
    print(f"n_f = {n_f}: {diff} of {whole.numel()} elements differ in bits from the 65,536-target table")
    assert diff == 0


def test_nothing_outside_the_rows_is_written(rtus, tables):
    """out= is rows 1 .. 150 of a 152-row tensor of sentinels, rows of odd length; then the same through the row-shard entry with
    shards of a block's 32 rows, and with shards of 37 rows: every one of those is cut inside a block"""
    torch, dev = _dev()
    E = tables
    n_f = N_ODD
    assert dev.rows_per_block(N_E, n_f) == E["eb"] == 32
    xe, ze, xf, zf = _t(E["xe"]), _t(E["ze"]), _t(E["xf"][:n_f]), _t(E["zf"][:n_f])
    big = torch.empty((N_E + 2, n_f), dtype=torch.float64, device="cuda")
    _bits(big).fill_(SENTINEL)
    dev.tt_layers_dev(E["z_if"], E["c"], xe, ze, xf, zf, out=big[1:N_E + 1], taup=True)
    hit = _bits(big) == SENTINEL
    assert bool(hit[0].all()) and bool(hit[N_E + 1].all()) and not bool(hit[1:N_E + 1].any())
    assert torch.equal(_bits(big[1:N_E + 1]), _bits(E["tt"][n_f]))
    for lo, hi in ((0, 32), (32, 64), (64, 96), (96, 128), (128, N_E), (0, 37), (37, 74), (74, 111), (111, 148), (148, N_E)):
        _bits(big).fill_(SENTINEL)
        dev.tt_layers_dev(E["z_if"], E["c"], xe[lo:hi], ze[lo:hi], xf, zf, out=big[1 + lo:1 + hi], row0=lo, n_rows_total=N_E, taup=True)
        hit = _bits(big) == SENTINEL
        assert bool(hit[:1 + lo].all()) and bool(hit[1 + hi:].all()) and not bool(hit[1 + lo:1 + hi].any()), (lo, hi)
        # (served rows have the whole table's bits wherever the shard is cut; the ragged block's solver rows only in a shard that
        # holds that block whole)
        top = hi if (lo, hi) == (128, N_E) else min(hi, 128)
        assert torch.equal(_bits(big[1 + lo:1 + top]), _bits(E["tt"][n_f][lo:top])), (lo, hi)


def test_sorted_entry_with_a_shuffled_aperture_and_odd_rows(rtus, tables):
    """one descriptor per row, each row where it belongs: bit-equal to the plain entry"""
    torch, dev = _dev()
    E = tables
    n_f = N_ODD
    perm = np.random.default_rng(5).permutation(N_E)
    got = dev.tt_layers_sorted_dev(E["z_if"], E["c"], _t(E["xe"][perm]), _t(E["ze"][perm]), _t(E["xf"][:n_f]), _t(E["zf"][:n_f]), taup=True)
    assert torch.equal(_bits(got), _bits(E["tt"][n_f][torch.as_tensor(perm, device="cuda")]))


def test_batched_entry_with_odd_rows(rtus, tables):
    torch, dev = _dev()
    E = tables
    n_f = N_ODD
    xf, zf = _t(E["xf"][:n_f]), _t(E["zf"][:n_f])
    xe2 = np.stack([E["xe"], E["xe"] + 0.0021])
    got = dev.tt_layers_batch_dev(E["z_if"], E["c"], _t(xe2), _t(np.zeros_like(xe2)), xf, zf, taup=True)
    assert torch.equal(_bits(got[0]), _bits(E["tt"][n_f]))
    one = dev.tt_layers_dev(E["z_if"], E["c"], _t(xe2[1]), _t(E["ze"]), xf, zf, taup=True)
    assert torch.equal(_bits(got[1]), _bits(one))


def test_a_block_of_exactly_32_rows(rtus):
    """131 rows of 65,536 targets: four blocks of 32 rows, the shortest that takes the table, and a ragged one of three"""
    torch, dev = _dev()
    z_if, c, zr = CFG3
    n_e = 131
    xe, ze = _aperture(n_e)
    xf, zf = _grid(256, zr)
    assert dev.rows_per_block(n_e, xf.size) == 32
    got = dev.tt_layers_dev(z_if, c, _t(xe), _t(ze), _t(xf), _t(zf), taup=True).cpu().numpy()
    assert np.isfinite(got).all()
    rows = np.array([0, 1, 15, 16, 30, 31, 32, 47, 63, 64, 95, 96, 112, 126, 127, 128, 130])
    _check(got, z_if, c, xe, ze, xf, zf, rows, _seams(xf.size))

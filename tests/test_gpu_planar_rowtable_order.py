"""GPU: the ORDER in which the planar kernel's row-table launches hand out their work items and write their rows
(csrc/rtus_fermat.hip work_item, DESIGN.md section 4 "Order across rows and XCDs").  An order is index arithmetic:
it may change no bit and must leave no element unwritten or written twice into another's place.  Checked here, for launches of every
block length and column count at which that arithmetic takes another branch: the tier's bar against the long-double oracle, the bits
of the same rows taken from launches that hold one block each, the mirror property of the served rows (row of +x = row of -x read
backwards along each image line: tests/test_gpu_planar_rowtable.py; the solver's rows do not have it, so it also shows that the rows
WERE served), and NaN guard rows above and below the launch's rows that must stay NaN.

Shapes.  Image lines of 256 columns, one depth per line, so every workgroup's 256 targets share a depth; a linear array at 0.3 mm;
the configs[2] medium (three layers); the tau-p tier.  The small cases are launches of a few rows x gx lines through the row-shard
entry, rows of a table of 2^20 rows: the whole table's size puts it in the 64-row regime (rtus_table_rows_per_block), the launch
itself is a few thousand to 230,000 solves.  The sorted and the batched entry have no shard form, and a ragged last block needs the
table's true length: those use the 150 x 65,536 table of the other row-table tests (blocks of 32 rows and one of 22, which takes the solver)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CFG3 = ([0.010, 0.025], [2330.0, 1483.0, 5900.0], (0.026, 0.066))
NT = 1 << 20                        # rows of the (never formed) whole table of the small cases: blocks of 64 rows for any n_f >= 64
N_A = 128                           # their aperture: two blocks
N_E = 150                           # the 65,536-target table's


def _dev():
    import torch
    from importlib import import_module
    return torch, import_module("ray-tracing-ultrasound_amd.device")


def _t(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")


def _lines(n_lines, zr=CFG3[2]):
    """n_lines image lines of 256 columns, symmetric in x bit for bit, one depth each"""
    x = (np.arange(256) - 127.5) * (0.04 / 255)
    xs, zs = np.meshgrid(x, np.linspace(zr[0], zr[1], n_lines))
    return xs.ravel(), zs.ravel()


def _aperture(n_e, pitch=0.3e-3):
    return (np.arange(n_e) - (n_e - 1) / 2.0) * pitch, np.zeros(n_e)


def _cols(n_f):
    """every seventh column, and three at both ends of every workgroup"""
    c = np.concatenate([np.arange(0, n_f, 7)] + [np.arange(0, n_f, 256) + k for k in (0, 1, 2, 253, 254, 255)] + [np.arange(n_f - 3, n_f)])
    return np.unique(c[(c >= 0) & (c < n_f)])


def _rows(n):
    r = np.concatenate([np.arange(0, n, max(n // 8, 1)), [0, 1, 15, 16, 31, 32, 47, 48, 63, 64, 65, n - 2, n - 1]])
    return np.unique(r[(r >= 0) & (r < n)])


def _check(sub, z_if, c, xe, ze, xf, zf):
    """the tier's bar (tests/test_gpu_planar_tiers.py, tests/test_gpu_planar_rowtable.py): 1e-10 relative against the long-double oracle"""
    from oracle import cport
    assert np.isfinite(sub).all()
    ref = cport.tt_layers(z_if, c, xe, ze, xf, zf)
    err = np.abs(sub - ref)
    rel = float((err / ref).max())
    print(f"max relative error against the oracle {rel:.2e} over {sub.size} solves")
    assert np.all(err <= 1e-16 + 1e-10 * ref), rel


def _launch(dev, torch, z_if, c, xe, ze, xf, zf, row0, n_rows_total):
    """the rows into the middle of a NaN-filled tensor with a guard row above and below; the guards must still be NaN"""
    n = len(xe)
    big = torch.full((n + 2, len(xf)), float("nan"), dtype=torch.float64, device="cuda")
    dev.tt_layers_dev(z_if, c, _t(xe), _t(ze), _t(xf), _t(zf), out=big[1:n + 1], row0=row0, n_rows_total=n_rows_total, taup=True)
    assert bool(torch.isnan(big[0]).all()) and bool(torch.isnan(big[n + 1]).all()), "a guard row was written"
    assert not bool(torch.isnan(big[1:n + 1]).any()), "an element of the launch's rows was not written"
    return big[1:n + 1]


def _mirrored(t):
    """rows x (whole image lines x 256), every line read backwards"""
    n_f = t.shape[1] // 256 * 256
    return t[:, :n_f].reshape(t.shape[0], -1, 256).flip(2).reshape(t.shape[0], n_f)


@pytest.fixture(scope="module")
def small(rtus):
    """per n_f: the 128 rows of the small cases' aperture from two launches of one 64-row block each; computed once, never modified"""
    torch, dev = _dev()
    z_if, c, _ = CFG3
    xe, ze = _aperture(N_A)
    cache = {}

    def get(n_f):
        if n_f not in cache:
            assert dev.rows_per_block(NT, n_f) == 64
            xf, zf = _lines(-(-n_f // 256))
            xf, zf = xf[:n_f], zf[:n_f]
            ref = torch.cat([_launch(dev, torch, z_if, c, xe[lo:lo + 64], ze[lo:lo + 64], xf, zf, lo, NT) for lo in (0, 64)])
            # (the aperture and the lines are symmetric: the reference itself has the mirror property, every row of it being served)
            assert torch.equal(ref[:, :n_f // 256 * 256].contiguous().view(torch.int64), _mirrored(ref.flip(0)).contiguous().view(torch.int64))
            cache[n_f] = dict(xf=xf, zf=zf, ref=ref)
        return cache[n_f]
    return dict(z_if=z_if, c=c, xe=xe, ze=ze, get=get)


def _small_case(S, n_f, row0, n):
    """rows [row0, row0 + n) of the small aperture in one launch: oracle, bits of the one-block launches, mirror"""
    torch, dev = _dev()
    R = S["get"](n_f)
    xe, ze = S["xe"][row0:row0 + n], S["ze"][row0:row0 + n]
    got = _launch(dev, torch, S["z_if"], S["c"], xe, ze, R["xf"], R["zf"], row0, NT)
    rows, cols = _rows(n), _cols(n_f)
    _check(got.cpu().numpy()[np.ix_(rows, cols)], S["z_if"], S["c"], xe[rows], ze[rows], R["xf"][cols], R["zf"][cols])
    diff = int((got.view(torch.int64) != R["ref"][row0:row0 + n].view(torch.int64)).sum())
    print(f"n_f = {n_f}, rows {row0} .. {row0 + n - 1}: {diff} of {got.numel()} elements differ in bits from the one-block launches")
    assert diff == 0
    # row r of +x against row N_A - 1 - r of -x (from the reference: a launch need not hold both), whole lines only
    assert np.array_equal(S["xe"], -S["xe"][::-1]) and np.array_equal(R["xf"][:256], -R["xf"][:256][::-1])
    mirror = _mirrored(R["ref"].flip(0)[row0:row0 + n])
    assert torch.equal(got[:, :mirror.shape[1]].contiguous().view(torch.int64), mirror.contiguous().view(torch.int64))


@pytest.mark.parametrize("n", [32, 33, 63, 64, 96, 100])
def test_block_lengths(rtus, small, n):
    """launches of n rows from the table's first row, nine lines: one block of n rows, or one of 64 and one of n - 64"""
    _small_case(small, 9 * 256, 0, n)


@pytest.mark.parametrize("n", [1, 2, 3, 5, 59])
def test_shards_of_an_eligible_block(rtus, small, n):
    """the launch starts at row 5 of a block that qualifies in the whole table and holds n rows of it (59: to the block's end)"""
    _small_case(small, 9 * 256, 5, n)


@pytest.mark.parametrize("gx", [1, 2, 7, 8, 9, 17])
def test_column_counts(rtus, small, gx):
    """fewer columns than XCDs, groups of four and of eight columns with and without a remainder; two row blocks (64 + 36 rows)"""
    _small_case(small, gx * 256, 0, 100)


@pytest.mark.parametrize("n_f", [4 * 256 + 1, 4 * 256 + 255, 7 * 256 + 1, 7 * 256 + 255])
def test_ragged_last_workgroup(rtus, small, n_f):
    _small_case(small, n_f, 0, 100)


@pytest.fixture(scope="module")
def table150(rtus):
    """the 150 x 65,536 table, tau-p tier: one launch, and one launch per block of it (four of 32 rows, one of 22); never modified"""
    torch, dev = _dev()
    z_if, c, _ = CFG3
    xe, ze = _aperture(N_E)
    xf, zf = _lines(256)
    assert dev.rows_per_block(N_E, xf.size) == 32
    whole = _launch(dev, torch, z_if, c, xe, ze, xf, zf, 0, N_E)
    blocks = torch.cat([_launch(dev, torch, z_if, c, xe[lo:lo + 32], ze[lo:lo + 32], xf, zf, lo, N_E) for lo in range(0, N_E, 32)])
    return dict(z_if=z_if, c=c, xe=xe, ze=ze, xf=xf, zf=zf, whole=whole, blocks=blocks)


def test_a_last_block_that_does_not_qualify(rtus, table150):
    """150 rows: the last block, 22 rows, takes the solver in its own order; every row has the bits of its block's own launch"""
    torch, _ = _dev()
    E = table150
    rows, cols = np.unique(np.concatenate([_rows(N_E), [127, 128, 129, 140]])), _cols(E["xf"].size)[::5]
    _check(E["whole"].cpu().numpy()[np.ix_(rows, cols)], E["z_if"], E["c"], E["xe"][rows], E["ze"][rows], E["xf"][cols], E["zf"][cols])
    assert torch.equal(E["whole"].view(torch.int64), E["blocks"].view(torch.int64))
    # mirror: rows 22 .. 127 have their partner among the served rows
    m = _mirrored(E["whole"].flip(0))
    assert torch.equal(E["whole"][22:128].view(torch.int64), m[22:128].contiguous().view(torch.int64))


def test_sorted_entry_with_a_shuffled_aperture(rtus, table150):
    """PERM: every served row goes through its own descriptor to the row it belongs to"""
    torch, dev = _dev()
    E = table150
    perm = np.random.default_rng(11).permutation(N_E)
    big = torch.full((N_E + 2, E["xf"].size), float("nan"), dtype=torch.float64, device="cuda")
    dev.tt_layers_sorted_dev(E["z_if"], E["c"], _t(E["xe"][perm]), _t(E["ze"][perm]), _t(E["xf"]), _t(E["zf"]), out=big[1:N_E + 1], taup=True)
    assert bool(torch.isnan(big[0]).all()) and bool(torch.isnan(big[N_E + 1]).all())
    got = big[1:N_E + 1]
    assert torch.equal(got.view(torch.int64), E["blocks"][torch.as_tensor(perm, device="cuda")].view(torch.int64))
    rows, cols = _rows(N_E), _cols(E["xf"].size)[::5]
    _check(got.cpu().numpy()[np.ix_(rows, cols)], E["z_if"], E["c"], E["xe"][perm][rows], E["ze"][perm][rows], E["xf"][cols], E["zf"][cols])
    inv = torch.as_tensor(np.argsort(perm), device="cuda")           # back in the aperture's order: the mirror property of the served rows
    assert torch.equal(got[inv][22:128].view(torch.int64), _mirrored(got[inv].flip(0))[22:128].contiguous().view(torch.int64))


def test_batched_entry_with_two_problems(rtus, table150):
    torch, dev = _dev()
    E = table150
    xe2 = np.stack([E["xe"], E["xe"] + 0.0021])
    big = torch.full((2 * N_E + 2, E["xf"].size), float("nan"), dtype=torch.float64, device="cuda")
    got = big[1:2 * N_E + 1].view(2, N_E, -1)
    dev.tt_layers_batch_dev(E["z_if"], E["c"], _t(xe2), _t(np.zeros_like(xe2)), _t(E["xf"]), _t(E["zf"]), out=got, taup=True)
    assert bool(torch.isnan(big[0]).all()) and bool(torch.isnan(big[2 * N_E + 1]).all()) and not bool(torch.isnan(got).any())
    assert torch.equal(got[0].view(torch.int64), E["blocks"].view(torch.int64))
    one = torch.cat([_launch(dev, torch, E["z_if"], E["c"], xe2[1][lo:lo + 32], E["ze"][lo:lo + 32], E["xf"], E["zf"], lo, N_E)
                     for lo in range(0, N_E, 32)])
    assert torch.equal(got[1].view(torch.int64), one.view(torch.int64))
    rows, cols = _rows(N_E), _cols(E["xf"].size)[::5]
    _check(got[1].cpu().numpy()[np.ix_(rows, cols)], E["z_if"], E["c"], xe2[1][rows], E["ze"][rows], E["xf"][cols], E["zf"][cols])
    m = _mirrored(got[0].flip(0))
    assert torch.equal(got[0][22:128].view(torch.int64), m[22:128].contiguous().view(torch.int64))

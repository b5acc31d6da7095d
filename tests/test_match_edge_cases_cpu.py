"""CPU: the premises of tests/test_gpu_match_edges.py, asserted where they can be checked without a GPU — the probes sit where
they should (about half of them hit), the C oracle (until now the matcher's only judge) gives np.isclose's decisions on every
one of them, a search window of fl(x +- win) really does drop hits on three of the families, the earliest hitting rays of
enough elements lie in different waves, workgroups and chunks, and the elements built for the fused kernel lie within a few
grid steps of the edge of their tolerance."""
import numpy as np
import pytest

import match_edge_cases as M

X65 = M.base_aperture(65)


def test_sizes_orders_and_variants():
    assert M.RESIDUE < 1e-17 and X65[32] == M.RESIDUE and X65.size == 65
    names = [n for n, _ in M.apertures()]
    assert names == ["n1", "n63", "n64", "n65", "n129", "n65_equal_pair", "n65_signed_zeros", "n65_inf_ends"]
    for name, x in M.apertures():
        n = x.size
        for order in M.ORDERS:
            idx = M.order_index(n, order)
            if idx is None:
                assert order == "seam" and n <= 64
                continue
            assert np.array_equal(np.sort(idx), np.arange(n))
            y = x[idx]
            if order == "seam":          # ascending inside every 64-element chunk, one descent, and that at a seam
                down = np.flatnonzero(~(y[:-1] <= y[1:]))
                assert list(down) == [63]
                assert all(np.all(np.diff(y[c:c + 64]) >= 0) for c in range(0, n, 64))
    e = M.base_aperture(65, "equal_pair"); assert e[10] == e[11]
    z = M.base_aperture(65, "signed_zeros"); assert np.signbit(z[32]) and not np.signbit(z[33]) and z[32] == z[33] == 0.0
    f = M.base_aperture(65, "inf_ends"); assert f[0] == -np.inf and f[-1] == np.inf


@pytest.mark.parametrize("atol,rtol", M.PAIRS)
def test_about_half_of_the_probes_hit_their_own_element(atol, rtol):
    probes, owner = M.edge_probes(X65, atol, rtol)
    assert probes.size == 1170 == 18 * 65
    H = M.isclose_matrix(probes, X65, atol, rtol)
    share = H[np.arange(probes.size), owner].mean()
    print(f"atol {atol:g} rtol {rtol:g}: {probes.size} probes, share hitting their own element {share:.3f}")
    assert 0.1 <= share <= 0.8               # (0.111 for atol = rtol = 0: of nine neighbours only x == x_e hits)
    assert H.any(axis=0).all()               # every element is hit by some probe
    # the middle probe of each side is fl(x_e +- tol_e) itself
    tol = M.tolerance(X65, atol, rtol)
    assert np.array_equal(probes.reshape(65, 2, 9)[:, 0, 4], X65 - tol) and np.array_equal(probes.reshape(65, 2, 9)[:, 1, 4], X65 + tol)


def test_layout_has_nan_every_seventh_and_both_infinities():
    c = M.case(X65, 1e-6, 0.0)
    land = c["land"]
    assert land.size == 1170 and np.isnan(land[::7]).all() and np.isnan(land).sum() == len(land[::7])
    assert (land == np.inf).sum() == 1 and (land == -np.inf).sum() == 1
    assert np.unique(c["tof"]).size == land.size
    p, o = M.edge_probes(X65, 1e-6, 0.0)
    keep = c["owner"] >= 0                    # what is left of the probes is a permutation of them
    assert np.isin(land[keep], p).all() and keep.sum() == 1170 - len(land[::7]) - 2


@pytest.mark.parametrize("name,x", M.apertures())
def test_c_oracle_gives_np_isclose_decisions(name, x):
    from oracle import cport
    differ = 0
    for order in M.ORDERS:
        idx = M.order_index(x.size, order)
        if idx is None:
            continue
        for atol, rtol in M.PAIRS:
            c = M.case(x[idx], atol, rtol)
            t4 = np.zeros((4, c["land"].size)); t4[0] = c["tof"]
            oh, ot, of = cport.match(c["land"], t4, c["x_rx"], atol, rtol)
            orh = cport.ray_hits(c["land"], c["x_rx"], atol, rtol)
            differ += int((oh != c["hit"]).sum() + (of != c["first_ray"]).sum() + (orh != c["ray_hits"]).sum())
            assert np.array_equal(oh, c["hit"]) and np.array_equal(of, c["first_ray"]) and M.same_bits(ot, c["tof_hit"])
            assert np.array_equal(orh, c["ray_hits"])
    print(f"{name}: decisions that differ from np.isclose's: {differ}")


@pytest.mark.parametrize("atol,rtol", M.PAIRS)
def test_a_window_of_rounded_sums_drops_hits_on_the_sharp_families_only(atol, rtol):
    """fl(x - win) can lie one grid step above an element whose rounded |x - x_e| is exactly its tolerance.  With rtol > 0 the
    window is wider than every tolerance but the outermost element's, which is why the default never showed it."""
    c = M.case(X65, atol, rtol)               # (on the row of rays as the kernels get it: NaN and infinities in place)
    plain = M.window_model(c["land"], X65, atol, rtol)
    wide = M.window_model(c["land"], X65, atol, rtol, widen=True)
    dropped = int((plain != c["H"]).sum())
    print(f"atol {atol:g} rtol {rtol:g}: fl(x +- win) drops {dropped} of {int(c['H'].sum())} hits; widened: {int((wide != c['H']).sum())}")
    assert not (plain & ~c["H"]).any()
    assert (dropped >= 1) == ((atol, rtol) in M.SHARP)
    assert np.array_equal(wide, c["H"])


def test_matcher_kernel_has_no_fused_multiply_add():
    """np.isclose's tolerance is a rounded product plus atol.  The stand-alone kernel formed it with one v_fma_f64 until the
    (1e-4, 3.0) family showed it (spelling it __dadd_rn(atol, __dmul_rn(rtol, |x|)) does not keep the compiler from contracting):
    the file now switches contraction off, and nothing in it has a use for an FMA.  Built as the Makefile builds it."""
    import os
    import subprocess
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "ray-tracing-ultrasound_amd", "csrc", "rtus_match.hip")
    flags = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-fPIC", "-fno-fast-math", "-fno-slp-vectorize", "--cuda-device-only", "-S"]
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "rtus_match.s")
        subprocess.run(["/opt/rocm/bin/hipcc"] + flags + [src, "-o", out], check=True, capture_output=True, timeout=600)
        asm = open(out).read()
    assert "rtus_match_kernel" in asm and "v_mul_f64" in asm and "v_fma_f64" not in asm


def test_smallest_dropped_hit():
    u = np.spacing(1e-4)
    xe, x = 257.7 * u, 1e-4 + 258 * u
    assert x - xe == 1e-4 and np.isclose(x, xe, rtol=0.0, atol=1e-4) and x - 1e-4 == 258 * u > xe


@pytest.mark.parametrize("atol,rtol", [p for p in M.PAIRS if p[0] + p[1] * 0.02 < M.PITCH / 2])
def test_earliest_hitting_rays_lie_in_different_waves_workgroups_and_chunks(atol, rtol):
    """(the families whose tolerance is below half the pitch: on the others an element is hit by the probes of several
    neighbours, dozens of rays, and its two earliest are among the first few of the row whatever the order)"""
    c = M.case(X65, atol, rtol)
    waves, groups, inside = M.layout_counts(c["H"])
    print(f"atol {atol:g} rtol {rtol:g}: elements whose two earliest rays differ in wave {waves}, workgroup {groups}, chunk of one workgroup {inside}")
    assert waves >= 8 and groups >= 8 and inside >= 8


def test_chunked_rows_follow_from_the_rotation():
    for atol, rtol in M.SHARP:
        c = M.chunked_rows(atol, rtol)
        assert c["land_rows"].shape == (M.ROWS, 1170) and M.ROWS * ((1170 + 255) // 256) == 4100 and 4100 // 2048 == 2
        assert np.unique(c["shift"]).size == M.ROWS
        for k in (0, 1, 37, 409, 819):
            assert M.same_bits(c["land_rows"][k], np.roll(c["land"], -int(c["shift"][k])))
            d = M.decisions(c["land_rows"][k], c["tof_rows"][k], c["x_rx"], atol, rtol)
            assert np.array_equal(d["first_ray"], c["first_rows"][k]) and np.array_equal(d["hit"], c["hit_rows"][k])
            assert M.same_bits(d["tof_hit"], c["tof_hit_rows"][k]) and np.array_equal(d["ray_hits"], c["ray_hits_rows"][k])
    c = M.chunked_rows(1e-6, 0.0)             # rows in which an element's two earliest rays lie in the two chunks of one workgroup
    rows = [k for k in range(0, M.ROWS, 41) if M.layout_counts(c["H"][(np.arange(1170) + c["shift"][k]) % 1170])[2] >= 8]
    assert len(rows) >= 8


@pytest.mark.parametrize("rtol", [0.0, 1e-5, 1.0, 3.0])
def test_fused_elements_sit_at_the_edge_of_a_stand_in_row(rtol):
    """|fl(|land - x_e|) - tol_e| <= 8 grid steps, a grid step being the coarsest of spacing(land), spacing(x_e) and ulp(tol_e):
    |land - x_e| is formed from the first two and comes no closer to tol_e than they allow, and the elements are moved by up
    to 4 of their own ulp on purpose.  Where tol_e is the coarsest of the three the bound is 8 ulp(tol_e)."""
    rng = np.random.default_rng(5)
    land = np.sort(rng.uniform(-0.03, 0.03, 1025))
    land[::50] = np.nan
    for atol in (1e-6, 1e-4, 2e-3):
        for n_rx in (63, 64, 65, 129):
            xe, rays, dist = M.fused_elements(land, n_rx, atol, rtol)
            assert xe.size == n_rx and np.all(np.diff(xe) >= 0) and np.isfinite(xe).all()
            tol = M.tolerance(xe, atol, rtol)
            d = np.abs(land[rays] - xe)
            assert np.all(np.abs(d - tol) <= 8 * M.grid_unit(land[rays], xe, tol)) and dist.max() <= 8
            fine = (np.spacing(tol) >= np.spacing(np.abs(xe))) & (np.spacing(tol) >= np.spacing(np.abs(land[rays])))
            assert np.all(np.abs(d - tol)[fine] <= 8 * np.spacing(tol[fine]))
            own = M.isclose_matrix(land, xe, atol, rtol)[rays, np.arange(n_rx)]
            assert 0.25 <= own.mean() <= 0.75                           # both decisions occur, on about half the elements each
            assert np.unique(rays >> 6).size == np.unique(np.flatnonzero(np.isfinite(land) & ((rtol < 1) | (np.abs(land) > 2 * atol))) >> 6).size
    x_rx, atol, ray = M.residue_case(land)
    x = land[ray]
    assert np.all(np.diff(x_rx) > 0) and x - x_rx[32] == atol and np.isclose(x, x_rx[32], rtol=0.0, atol=atol) and x - atol > x_rx[32]

"""GPU: phase-coherence and weighted TFM over a half-matrix capture (rtus_tfm_phase_hmc*, rtus_tfm_weighted_hmc*) against
tests/tfm_hmc_ext_numpy.py and against the full-matrix kernels on the unpacked capture.

1. exact data (das_exact_numpy's generator rules: no operation rounds, so every order of summation gives the same float32 sums) at
   every size of D.HMC_SIZES — 1, 15, 16, 17 (a block, its unrolled triangle, a block of one column under sixteen rows), 31, 32, 33,
   48, 64, 65 (the one-table phase kernel's second tile), 81 — one and two delay tables, one and two weight tables, NaN / infinite
   weights on some legs, the hand-made columns (record edges, the 1e8 leg limit, NaN / infinite legs, the column without a path):
   np.array_equal against the model and against tfm_weighted / tfm_phase of hmc_unpack;
2. random float data (n_e = 17, 33): counts and scf bit for bit tfm_phase's on the unpacked capture; the weighted image within the
   recursive-sum bound (n_e^2 + 16) 2^-24 sum |W| |p| of the fp64 model;
3. the one-table paths against equal copies; 4. independence of the outputs asked for, of the focal points sharing the call and of
   the grid's shape; 5. host, device and captured-graph paths; 6. a point scatterer end to end.

The bar of vcf (X.VCF_BAR = 5.2e-7).  The comparison is against the model's fp64 sum of fp64 phasors of the kernel's own samples
(exact data: the samples are exact), so what is left is the kernel's fp32 phasors and its recursive fp32 sum.
  hard cap: (N_max + 8) 2^-23 = 5.85e-4 at N_max = 4900, as tests/test_gpu_tfm_phase.py derives it; sizes with n_e^2 > 4900 (81) are
            left out of the vcf comparison (their counts, scf and image are compared like the others);
  asserted: 4 x the largest |vcf32 - vcf| of the model's float32 sum of float32 phasors in the kernel's half-matrix order (the pair
            first) against its fp64 sum, over the exact cases of every other size with one and two tables, measured on the CPU by
            tests/test_tfm_hmc_ext_cpu.py::test_the_bar_of_vcf: 1.294e-7 (n_e = 64, both forms; 7.8e-8 at 33, 7.1e-8 at 48 and 65),
            4 x 1.294e-7 = 5.2e-7.  The factor 4 is test_gpu_tfm_phase.py's margin for the hardware's reciprocal square root and the
            phasor products, which the emulation does not reproduce.
"""
import functools

import numpy as np
import pytest

import das_exact_numpy as D
import tfm_hmc_ext_numpy as X

pytestmark = pytest.mark.gpu

CASES = [(n_e, two) for n_e in D.HMC_SIZES for two in (False, True)]


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32 if x.dtype.itemsize % 8 else np.uint64)


def _same(x, y):
    return x.dtype == y.dtype and x.shape == y.shape and np.array_equal(_bits(x), _bits(y))


def _c64(x):
    """an exact model sum (complex128 holding float32 numbers) as complex64"""
    y = x.astype(np.complex64)
    assert np.array_equal(y.astype(np.complex128), x)
    return y


@functools.lru_cache(maxsize=None)
def _weighted(rtus, n_e, two, two_w):
    c = X.exact_case(n_e, two, two_w)
    return rtus.tfm_weighted_hmc(c["h"], c["fs"], c["tt_tx"], c["w_tx"], c["tt_rx"], c["w_rx"], t0=c["t0"], sensitivity=True)


@functools.lru_cache(maxsize=None)
def _phase(rtus, n_e, two):
    c = D.hmc_case(n_e, two)
    r = rtus.tfm_phase_hmc(c["h"], c["fs"], c["tt_tx"], c["tt_rx"], t0=c["t0"], counts=True)
    for v in r.values():
        v.flags.writeable = False
    return r


# ------------------------------------------------------------------------------------------------ 1. exact, every tile seam
@pytest.mark.parametrize("n_e,two", CASES)
@pytest.mark.parametrize("two_w", [False, True])
def test_weighted_is_the_model_and_the_full_matrix_kernel_on_exact_data(rtus, n_e, two, two_w):
    c, m = X.exact_case(n_e, two, two_w), X.exact_model(n_e, two, two_w)
    img, sens = _weighted(rtus, n_e, two, two_w)
    assert img.dtype == np.complex64 and img.shape == (D.N_F,) and sens.dtype == np.float32 and sens.shape == (D.N_F,)
    want, want_p = _c64(m["S_w"]), m["P"].astype(np.float32)
    bad = np.nonzero(img != want)[0]
    assert bad.size == 0, (bad[:8], img[bad[:8]], want[bad[:8]], {k: v for k, v in c["cols"].items() if v in bad})
    assert np.array_equal(sens, want_p)
    if not two:
        assert np.array_equal(img, _c64(m["S_w1"]))
    w_rx = c["w_tx"] if c["w_rx"] is None else c["w_rx"]
    f_img, f_sens = rtus.tfm_weighted(rtus.hmc_unpack(c["h"]), c["fs"], c["tt_tx"], c["w_tx"], c["tt_rx"],
                                      w_rx if (two or two_w) else None, t0=c["t0"], sensitivity=True)
    assert np.array_equal(img, f_img) and _same(sens, f_sens)
    col = c["cols"]["no_path"]
    assert img[col] == 0 and sens[col] == 0
    assert np.abs(img).max() > 0 and sens.max() > 0
    plain = rtus.tfm_weighted_hmc(c["h"], c["fs"], c["tt_tx"], c["w_tx"], c["tt_rx"], c["w_rx"], t0=c["t0"])
    assert _same(plain, img)                                           # passing sens does not change the image


@pytest.mark.parametrize("n_e,two", CASES)
def test_phase_is_the_model_and_the_full_matrix_kernel_on_exact_data(rtus, n_e, two):
    c, m = D.hmc_case(n_e, two), X.exact_model(n_e, two, False)
    r = _phase(rtus, n_e, two)
    assert r["image"].dtype == np.complex64 and r["vcf"].dtype == r["scf"].dtype == np.float32
    assert r["sign_sum"].dtype == r["n_pairs"].dtype == np.int32
    assert _same(r["image"], rtus.tfm_analytic_hmc(c["h"], c["fs"], c["tt_tx"], c["tt_rx"], t0=c["t0"]))
    assert np.array_equal(r["image"], _c64(m["S"]))
    assert np.array_equal(r["n_pairs"], m["N"])
    bad = np.nonzero(r["sign_sum"] != m["B"])[0]
    assert bad.size == 0, (bad[:8], r["sign_sum"][bad[:8]], m["B"][bad[:8]])
    assert r["scf"].dtype == m["scf"].dtype and np.array_equal(r["scf"], m["scf"], equal_nan=True)
    full = rtus.tfm_phase(rtus.hmc_unpack(c["h"]), c["fs"], c["tt_tx"], c["tt_rx"], t0=c["t0"], counts=True)
    assert np.array_equal(r["sign_sum"], full["sign_sum"]) and np.array_equal(r["n_pairs"], full["n_pairs"])
    assert _same(r["scf"], full["scf"])
    col = c["cols"]["no_path"]
    assert r["n_pairs"][col] == 0 and np.isnan(r["scf"][col]) and np.isnan(r["vcf"][col])
    assert np.array_equal(np.isnan(r["vcf"]), np.isnan(m["vcf"]))
    fin = ~np.isnan(m["vcf"])
    assert np.all((r["vcf"][fin] >= 0) & (r["vcf"][fin] <= 1))
    if n_e in X.VCF_SIZES:
        assert X.VCF_BAR < X.VCF_CAP and m["N"].max() <= 4900
        err = float(np.max(np.abs(r["vcf"][fin].astype(np.float64) - m["vcf"][fin]))) if fin.any() else 0.0
        print(f"n_e = {n_e}, {'two tables' if two else 'one table'}: vcf {err:.2e} (bar {X.VCF_BAR:.1e})")
        assert err <= X.VCF_BAR, err


# ------------------------------------------------------------------------------------------------ 2. random float data
N_F = 1000


@functools.lru_cache(maxsize=None)
def _random(n_e):
    """random complex records, two different random tables (half positions from 12 samples before the record to 12 past the half of
    it; NaN, absurd and infinite legs; the last three focal points without a path), two weight tables with NaN / infinite entries; a
    band of zero samples and a silent record"""
    rng = np.random.default_rng(40 + n_e)
    fs, t0, n_t = 40e6, 1.5e-6, 300
    n_p = n_e * (n_e + 1) // 2
    h = (rng.standard_normal((n_p, n_t)) + 1j * rng.standard_normal((n_p, n_t))).astype(np.complex64)
    h[:, 100:140] = 0
    h[3] = 0

    def table():
        lo, hi = (-12 + 0.5 * t0 * fs) / fs, (n_t / 2 + 12 + 0.5 * t0 * fs) / fs
        t = rng.uniform(lo, hi, (n_e, N_F))
        m = rng.random(t.shape)
        t[m < 0.03] = np.nan
        t[(m >= 0.03) & (m < 0.035)] = 1e3
        t[(m >= 0.035) & (m < 0.037)] = -np.inf
        t[(m >= 0.037) & (m < 0.039)] = np.inf
        t[:, -3:] = np.nan
        return t

    def weights():
        w = (rng.standard_normal((n_e, N_F)) + 1j * rng.standard_normal((n_e, N_F))).astype(np.complex64)
        m = rng.random(w.shape)
        w[m < 0.01] = np.nan
        w[(m >= 0.01) & (m < 0.02)] = np.complex64(complex(1.0, -np.inf))
        return w
    out = (h, fs, t0, table(), table(), weights(), weights())
    for v in out:
        if isinstance(v, np.ndarray):
            v.flags.writeable = False
    return out


@pytest.mark.parametrize("n_e", [17, 33])
@pytest.mark.parametrize("two", [False, True])
def test_random_data(rtus, n_e, two):
    h, fs, t0, tt_a, tt_b, w_a, w_b = _random(n_e)
    tt_rx = tt_b if two else None
    r = rtus.tfm_phase_hmc(h, fs, tt_a, tt_rx, t0=t0, counts=True)
    full = rtus.tfm_phase(rtus.hmc_unpack(h), fs, tt_a, tt_rx, t0=t0, counts=True)
    assert np.array_equal(r["sign_sum"], full["sign_sum"]) and np.array_equal(r["n_pairs"], full["n_pairs"])
    assert _same(r["scf"], full["scf"])
    assert np.abs(r["sign_sum"]).max() > 0 and r["n_pairs"].max() > 0.8 * n_e * n_e and np.all(r["n_pairs"][-3:] == 0)
    assert _same(r["image"], rtus.tfm_analytic_hmc(h, fs, tt_a, tt_rx, t0=t0))
    fin = r["n_pairs"] > 0
    assert np.array_equal(np.isnan(r["vcf"]), ~fin) and np.all((r["vcf"][fin] >= 0) & (r["vcf"][fin] <= 1))
    # (each form within its bar of the exact value: 3.0e-7 is tests/test_gpu_tfm_phase.py's VCF_BAR for the full-matrix kernel)
    assert np.max(np.abs(r["vcf"][fin].astype(np.float64) - full["vcf"][fin])) <= X.VCF_BAR + 3.0e-7
    m = X.walk(h, fs, t0, tt_a, tt_rx, w_a, w_b, exact=False)
    img, sens = rtus.tfm_weighted_hmc(h, fs, tt_a, w_a, tt_rx, w_b, t0=t0, sensitivity=True)
    bound = (n_e * n_e + 16) * 2.0 ** -24 * m["Aw"]
    err = np.abs(img.astype(np.complex128) - m["S_w"])
    with np.errstate(divide="ignore", invalid="ignore"):
        worst = float(np.max(np.where(bound > 0, err / bound, 0.0)))
    print(f"n_e = {n_e}, {'two' if two else 'one'} delay table(s): largest |image - fp64 model| / bound = {worst:.3e}")
    assert np.isfinite(img.view(np.float32)).all() and np.all(err <= bound), float(np.max(err - bound))
    assert np.all(img[-3:] == 0) and np.all(sens[-3:] == 0) and np.abs(img).max() > 0
    f_img, f_sens = rtus.tfm_weighted(rtus.hmc_unpack(h), fs, tt_a, w_a, tt_rx, w_b, t0=t0, sensitivity=True)
    assert _same(sens, f_sens)                                         # the same fmaf chain and fp64 product
    assert np.all(np.abs(f_img.astype(np.complex128) - m["S_w"]) <= bound)


# ------------------------------------------------------------------------------------------------ 3. one-table paths
def test_one_table_paths_give_the_bits_of_two_equal_tables(rtus):
    for n_e in (17, 65):
        c = X.exact_case(n_e, False, False)
        r = _phase(rtus, n_e, False)
        for tt_rx in (c["tt_tx"], c["tt_tx"].copy()):                  # the same object: one table; an equal copy: two gathers
            r2 = rtus.tfm_phase_hmc(c["h"], c["fs"], c["tt_tx"], tt_rx, t0=c["t0"], counts=True)
            for k in r:
                assert _same(r2[k], r[k]), (n_e, k)
        img, sens = _weighted(rtus, n_e, False, False)
        for tt_rx in (c["tt_tx"], c["tt_tx"].copy()):
            i2, s2 = rtus.tfm_weighted_hmc(c["h"], c["fs"], c["tt_tx"], c["w_tx"], tt_rx, t0=c["t0"], sensitivity=True)
            assert _same(i2, img) and _same(s2, sens), n_e
    h, fs, t0, tt_a, _, _, _ = _random(17)                             # float data: the phase sums' fmaf(2, u, U) is U + (u + u)
    r = rtus.tfm_phase_hmc(h, fs, tt_a, t0=t0, counts=True)
    r2 = rtus.tfm_phase_hmc(h, fs, tt_a, tt_a.copy(), t0=t0, counts=True)
    for k in r:
        assert _same(r2[k], r[k]), k


# ------------------------------------------------------------------------------------------------ 4. independence
@pytest.mark.parametrize("two", [False, True])
def test_no_output_depends_on_which_others_are_asked_for(rtus, two):
    h, fs, t0, tt_a, tt_b, w_a, w_b = _random(33)
    tt_rx = tt_b if two else tt_a
    n_e, n_t = 33, h.shape[1]
    L = rtus.lib()
    r = rtus.tfm_phase_hmc(h, fs, tt_a, tt_rx, t0=t0, counts=True)
    full = dict(vcf=r["vcf"], scf=r["scf"], counts=np.stack([r["sign_sum"], r["n_pairs"]], axis=1))
    ref = rtus.tfm_analytic_hmc(h, fs, tt_a, tt_rx, t0=t0)
    for mask in range(8):
        img = np.full(N_F, np.nan, dtype=np.complex64)
        got = dict(vcf=np.full(N_F, np.nan, dtype=np.float32) if mask & 1 else None,
                   scf=np.full(N_F, np.nan, dtype=np.float32) if mask & 2 else None,
                   counts=np.full((N_F, 2), -7, dtype=np.int32) if mask & 4 else None)
        ptr = {k: (None if v is None else v.ctypes.data) for k, v in got.items()}
        st = L.rtus_tfm_phase_hmc(h.ctypes.data, n_e, n_t, fs, t0, tt_a.ctypes.data, tt_rx.ctypes.data, N_F, img.ctypes.data,
                                  ptr["vcf"], ptr["scf"], ptr["counts"], 0)
        assert st == 0, (mask, st)
        assert _same(img, ref), mask
        for k, v in got.items():
            assert v is None or _same(v, full[k]), (mask, k)
    img, sens = rtus.tfm_weighted_hmc(h, fs, tt_a, w_a, tt_rx, w_b, t0=t0, sensitivity=True)
    assert _same(rtus.tfm_weighted_hmc(h, fs, tt_a, w_a, tt_rx, w_b, t0=t0), img)


@pytest.mark.parametrize("two", [False, True])
def test_subsets_and_grid_shapes_do_not_change_the_bits(rtus, two):
    """a reversed strided subset of the focal points; n_f = 8 x 256 + 1 (nine workgroups: the ragged grid keeps the plain order) and
    16 x 256 (the XCD-contiguous order), the exact case's 257 columns repeated"""
    n_e = 33
    c = X.exact_case(n_e, two, True)
    r = _phase(rtus, n_e, two)
    img, sens = _weighted(rtus, n_e, two, True)
    keys = ("image", "vcf", "scf", "sign_sum", "n_pairs")
    pick = lambda t, sel: None if t is None else np.ascontiguousarray(t[:, sel])
    for sel in (np.r_[np.arange(255, 3, -7), 5, 0], np.arange(8 * 256 + 1) % D.N_F, np.arange(16 * 256) % D.N_F):
        tt_tx, tt_rx = pick(c["tt_tx"], sel), pick(c["tt_rx"], sel)
        s = rtus.tfm_phase_hmc(c["h"], c["fs"], tt_tx, tt_rx, t0=c["t0"], counts=True)
        for k in keys:
            assert _same(s[k], r[k][sel]), (sel.size, k)
        i2, s2 = rtus.tfm_weighted_hmc(c["h"], c["fs"], tt_tx, pick(c["w_tx"], sel), tt_rx, pick(c["w_rx"], sel), t0=c["t0"],
                                       sensitivity=True)
        assert _same(i2, img[sel]) and _same(s2, sens[sel]), sel.size


# ------------------------------------------------------------------------------------------------ 5. paths
def test_host_device_and_graph_paths_agree(rtus):
    import torch
    from importlib import import_module
    dev = import_module("ray-tracing-ultrasound_amd.device")
    h, fs, t0, tt_a, tt_b, w_a, w_b = _random(33)
    want = {two: rtus.tfm_phase_hmc(h, fs, tt_a, tt_b if two else None, t0=t0, counts=True) for two in (False, True)}
    want_w = {two: rtus.tfm_weighted_hmc(h, fs, tt_a, w_a, tt_b if two else None, w_b, t0=t0, sensitivity=True) for two in (False, True)}
    cuda = lambda x: torch.as_tensor(np.array(x), device="cuda")
    da = cuda(h.view(np.float32).reshape(*h.shape, 2))
    ta, tb = cuda(tt_a), cuda(tt_b)
    wa, wb = cuda(w_a.view(np.float32).reshape(*w_a.shape, 2)), cuda(w_b.view(np.float32).reshape(*w_b.shape, 2))
    f32 = lambda *n: torch.empty(n, dtype=torch.float32, device="cuda")
    out, vcf, scf, cnt = f32(N_F, 2), f32(N_F), f32(N_F), torch.empty((N_F, 2), dtype=torch.int32, device="cuda")
    wout, sens = f32(N_F, 2), f32(N_F)
    as_c = lambda t: t.cpu().numpy().view(np.complex64)[:, 0]

    def check(two):
        torch.cuda.synchronize()
        r, (w_img, w_sens) = want[two], want_w[two]
        assert _same(as_c(out), r["image"]) and _same(vcf.cpu().numpy(), r["vcf"]) and _same(scf.cpu().numpy(), r["scf"])
        c = cnt.cpu().numpy()
        assert np.array_equal(c[:, 0], r["sign_sum"]) and np.array_equal(c[:, 1], r["n_pairs"])
        assert _same(as_c(wout), w_img) and _same(sens.cpu().numpy(), w_sens)

    def run(two):
        dev.tfm_phase_hmc_dev(da, fs, ta, tb if two else None, t0=t0, out=out, vcf=vcf, scf=scf, counts=cnt)
        dev.tfm_weighted_hmc_dev(da, fs, ta, wa, tb if two else None, wb, t0=t0, out=wout, sens=sens)

    got = dev.tfm_phase_hmc_dev(da, fs, ta, t0=t0, out=out, vcf=vcf, scf=scf, counts=cnt)
    assert len(got) == 4 and got[0] is out and got[1] is vcf and got[2] is scf and got[3] is cnt
    got = dev.tfm_weighted_hmc_dev(da, fs, ta, wa, None, wb, t0=t0, out=wout, sens=sens)
    assert got[0] is wout and got[1] is sens
    check(False)
    plain = dev.tfm_phase_hmc_dev(da, fs, ta, ta, t0=t0)                # allocated output, nothing else, the same table twice
    o2, s2 = dev.tfm_phase_hmc_dev(da, fs, ta, tb, t0=t0, scf=torch.empty_like(scf))
    w_plain = dev.tfm_weighted_hmc_dev(da, fs, ta, wa, tb, wb, t0=t0)   # allocated output, no sens, two delay tables
    torch.cuda.synchronize()
    assert _same(as_c(plain), want[False]["image"])
    assert _same(as_c(o2), want[True]["image"]) and _same(s2.cpu().numpy(), want[True]["scf"])
    assert _same(as_c(w_plain), want_w[True][0])
    f64 = lambda n: torch.empty(n, dtype=torch.float64, device="cuda")
    i32 = lambda n: torch.empty(n, dtype=torch.int32, device="cuda")
    for kw in (dict(vcf=f64(N_F)), dict(vcf=f32(N_F + 1)), dict(scf=f64(N_F)), dict(scf=f32(N_F - 1)), dict(counts=f32(2 * N_F)),
               dict(counts=i32(N_F)), dict(out=f32(N_F))):
        with pytest.raises(ValueError):
            dev.tfm_phase_hmc_dev(da, fs, ta, t0=t0, **kw)
    for args in ((da[..., 0].contiguous(), fs, ta), (da[:-1].contiguous(), fs, ta), (da, fs, ta[:5].contiguous()),
                 (da, fs, ta, tb[:, :5].contiguous()), (da.cpu(), fs, ta)):
        with pytest.raises(ValueError):
            dev.tfm_phase_hmc_dev(*args)
    for args, kw in (((da, fs, ta, wa[:5].contiguous()), {}), ((da, fs, ta, wa[..., 0].contiguous()), {}),
                     ((da, fs, ta, wa.double()), {}), ((da, fs, ta, wa, None, wb[:, :7].contiguous()), {}),
                     ((da[:-1].contiguous(), fs, ta, wa), {}), ((da, fs, ta, wa), dict(sens=f64(N_F))),
                     ((da, fs, ta, wa), dict(out=f32(N_F))), ((da, fs, ta, wa.cpu()), {})):
        with pytest.raises(ValueError):
            dev.tfm_weighted_hmc_dev(*args, **kw)

    for two in (True, False):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):                                     # warm-up off the default stream, as torch.cuda.graph wants
            run(two)
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):                                      # one capture stream
            run(two)
        for t in (out, vcf, scf, wout, sens):
            t.fill_(float("nan"))
        cnt.fill_(-7)
        g.replay()
        check(two)


# ------------------------------------------------------------------------------------------------ 6. end to end
def test_point_scatterer_weighted_and_phase_end_to_end(rtus):
    """one point scatterer through simulate_fmc with synthetic complex leg amplitudes A[e, f] — phases that vary with the element and
    the point, parts on a grid of 1/16 so that A[i] A[j] is exact and the simulated FMC symmetric bit for bit.  hmc_pack ->
    hmc_analytic -> tfm_weighted_hmc with the conjugate amplitudes: |S| / P peaks at the scatterer and agrees there with tfm_views on
    the full matrix to 1e-4 (the summation order is the only difference); tfm_phase_hmc's scf is the full matrix's exactly"""
    n_el, c, fs, n_t = 16, 1500.0, 50e6, 1500
    x = (np.arange(n_el) - (n_el - 1) / 2) * 0.6e-3
    z = np.zeros(n_el)
    xs, zs = np.meshgrid(np.linspace(-0.003, 0.005, 33), np.linspace(0.011, 0.019, 33))
    at = (16, 16)                                                       # the scatterer: the grid's centre point (1 mm, 15 mm)
    f_s = int(np.ravel_multi_index(at, xs.shape))
    tt = rtus.travel_time_layers([], [c], x, z, xs.ravel(), zs.ravel())
    theta = np.arctan2(xs.ravel()[None, :] - x[:, None], zs.ravel()[None, :])          # [n_el, n_f]
    amp = np.exp(1j * (2.5 * theta + 0.3 * np.arange(n_el)[:, None]))
    amp = ((np.rint(amp.real * 16) + 1j * np.rint(amp.imag * 16)) / 16).astype(np.complex64)
    pulse, centre = rtus.gaussian_pulse(5e6, 3.0, fs, 8)
    a_s = np.ascontiguousarray(amp[:, [f_s]])
    fmc = rtus.simulate_fmc(np.ascontiguousarray(tt[:, [f_s]]), fs=fs, n_t=n_t, pulse=pulse, centre=centre, oversample=8, w_tx=a_s)
    assert fmc.dtype == np.float32 and np.abs(fmc).max() > 0.5
    assert np.array_equal(fmc, fmc.transpose(1, 0, 2))
    analytic = rtus.hmc_analytic(rtus.hmc_pack(fmc))
    w = np.conj(amp)
    S, P = rtus.tfm_weighted_hmc(analytic, fs, tt, w, None, w.copy(), sensitivity=True)
    assert np.all(P > 0)
    val = np.abs(S) / P
    assert int(np.argmax(val)) == f_s, (np.unravel_index(np.argmax(val), xs.shape), at)
    views = rtus.tfm_views(fmc, fs, {"L": tt}, "L-L", envelope=True, amplitudes={"L": (amp, amp)})
    ref = views["L-L"]
    print(f"|S| / P at the scatterer: half matrix {val[f_s]:.6f}, full matrix {ref[f_s]:.6f}")
    assert 0.8 <= ref[f_s] <= 1.2                                      # a unit scatterer reads 1 (less the Hilbert filter's and the lerp's loss)
    assert abs(val[f_s] - ref[f_s]) <= 1e-4 * ref[f_s]
    assert int(np.argmax(ref)) == f_s
    full = rtus.tfm_phase(rtus.fmc_analytic(fmc), fs, tt)
    r = rtus.tfm_phase_hmc(analytic, fs, tt)
    assert _same(r["scf"], full["scf"]) and np.isfinite(r["scf"]).all() and r["scf"].max() > 0

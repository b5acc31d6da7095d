"""GPU: envelope TFM with carrier-aware (IQ) interpolation (rtus_tfm_iq*, rtus_tfm_iq_hmc*) — f_demod = 0 against rtus_tfm_analytic /
rtus_tfm_analytic_hmc bit for bit, the NumPy oracle (tests/tfm_iq_numpy.py) at three carrier frequencies, the half-matrix kernels
against the full-matrix kernel on the unpacked block, determinism under any sharing of the call, host / device / captured-graph
paths, status codes, and a point scatterer at 4 samples per cycle through tfm_iq, tfm_views, pwi_image and adaptive_tfm.

Shapes: the ones test_gpu_tfm_analytic.py and test_gpu_tfm_hmc.py justify.  Full matrix: 70 x 70 x 500 (one table, two receive
tiles, 70 = 4 x 16 + 6), 24 x 11 x 400 (separate tables), 40 x 40 x 300 (one table, the transmit delays read from the tile),
1 x 1 x 300.  Half matrix: 1 element (the diagonal alone), 17 (a full block of sixteen columns, its unrolled triangle, a block of
one column), 40 (the walk with its state in registers and a padded last batch), 70 (rows of earlier tiles), each with one table
and with two.  1000 focal points (a ragged last workgroup), once tiled to 2000 (eight workgroups: the XCD-contiguous order); t0
zero and not; legs that are NaN, infinite or absurd; the last three focal points without any path.

Bounds.  Oracle: |image - oracle| <= (2 n_tx n_rx 2^-24 + 1e-5) A[f], A = the sum of the terms' moduli.  The first term is the
first-order worst case of two recursive fp32 sums (test_gpu_tfm_hmc.py); 1e-5 is the allowance for the two fp32 phasors and the
products of the step, a thousand times below the effect delivered.  The oracle forms the positions as the kernels do, so the
comparison measures the step.  An fp32 NumPy emulation of the step and the sums (tfm_iq_numpy.tfm_iq(emulate=True), correctly
rounded sine and cosine) stays inside it on the CPU: the largest |difference| / A over the full-matrix cases and nu = 0.11, 0.25,
0.49 is 2.3e-6, at 1 x 1 (bound 1.0e-5), where a single term stands alone and b = a0 + w (q - a0) can cancel; 1.2e-7 at the other
shapes (bounds 4.1e-5 to 5.9e-4).  test_tfm_iq_cpu.py holds the emulation to the bound on a small case.  cf: <= 1e-4 absolute where E >= 1e-12 of its maximum
(test_gpu_tfm_analytic.py's bar, for its reason).  Half matrix against full matrix: 2 n_e^2 2^-24 A[f] (test_gpu_tfm_hmc.py's: the
same fp32 terms in another order, and the pair's own sum).
"""
import functools

import numpy as np
import pytest

import autofocus_numpy as AF
import tfm_iq_numpy as TQ

pytestmark = pytest.mark.gpu

N_F = 1000
FS = 40e6
NUS = (0.11, 0.25, 0.49)
#            seed n_tx n_rx n_t  t0      one table
FULL = {
    "tiles70": (1, 70, 70, 500, 1.5e-6, True),
    "separate24x11": (2, 24, 11, 400, 2.0e-6, False),
    "intile40": (3, 40, 40, 300, 0.0, True),
    "one1": (5, 1, 1, 300, 0.0, True),
}
#           seed n_e n_t  t0
HMC = {
    "diag1": (1, 1, 300, 0.0),
    "batch17": (2, 17, 300, 1.5e-6),
    "tile40": (3, 40, 300, 0.0),
    "tiles70": (4, 70, 500, 2.0e-6),
}


def _table(rng, n_e, n_t, t0):
    """half positions from 12 samples before the record to 12 past the half of it (pair positions cross both ends); NaN, absurd
    (1e3 s) and infinite legs; the last three focal points without any path"""
    lo, hi = (-12 + 0.5 * t0 * FS) / FS, (n_t / 2 + 12 + 0.5 * t0 * FS) / FS
    t = rng.uniform(lo, hi, (n_e, N_F))
    m = rng.random(t.shape)
    t[m < 0.03] = np.nan
    t[(m >= 0.03) & (m < 0.035)] = 1e3
    t[(m >= 0.035) & (m < 0.037)] = -np.inf
    t[(m >= 0.037) & (m < 0.039)] = np.inf
    t[:, -3:] = np.nan
    return t


def _records(rng, shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


@functools.lru_cache(maxsize=None)
def _full(name):
    """-> (a complex64 [n_tx, n_rx, n_t], t0, tt_tx, tt_rx or None)"""
    seed, n_tx, n_rx, n_t, t0, same = FULL[name]
    rng = np.random.default_rng(seed)
    a = _records(rng, (n_tx, n_rx, n_t))
    tt_tx = _table(rng, n_tx, n_t, t0)
    return a, t0, tt_tx, (None if same else _table(rng, n_rx, n_t, t0))


@functools.lru_cache(maxsize=None)
def _hmc(name):
    """-> (h complex64 [n_pairs, n_t], t0, tt_a, tt_b): two different random tables"""
    seed, n_e, n_t, t0 = HMC[name]
    rng = np.random.default_rng(seed)
    return _records(rng, (n_e * (n_e + 1) // 2, n_t)), t0, _table(rng, n_e, n_t, t0), _table(rng, n_e, n_t, t0)


@functools.lru_cache(maxsize=None)
def _gpu_full(rtus, name, nu):
    a, t0, tt_tx, tt_rx = _full(name)
    return rtus.tfm_iq(a, FS, nu * FS, tt_tx, tt_rx, t0=t0, coherence=True)


@functools.lru_cache(maxsize=None)
def _gpu_hmc(rtus, name, two, nu):
    h, t0, tt_a, tt_b = _hmc(name)
    return rtus.tfm_iq_hmc(h, FS, nu * FS, tt_a, tt_b if two else None, t0=t0, coherence=True)


@functools.lru_cache(maxsize=None)
def _oracle_hmc(name, two, nu):
    h, t0, tt_a, tt_b = _hmc(name)
    return TQ.tfm_iq(h, FS, t0, nu * FS, tt_a, tt_b if two else tt_a)


def _f2(a):
    """complex64 [...] -> the float32 [..., 2] layout"""
    return np.ascontiguousarray(a.view(np.float32).reshape(*a.shape, 2))


def _as_c(t):
    return t.cpu().numpy().view(np.complex64)[:, 0]


# ---------------------------------------------------------------- 1. f_demod = 0 is the linear kernel, bit for bit
@pytest.mark.parametrize("name", list(FULL))
def test_f_demod_zero_is_tfm_analytic_bit_for_bit(rtus, name):
    a, t0, tt_tx, tt_rx = _full(name)
    img, cf = _gpu_full(rtus, name, 0.0)
    assert img.dtype == np.complex64 and img.shape == (N_F,) and cf.dtype == np.float32 and cf.shape == (N_F,)
    ref, ref_cf = rtus.tfm_analytic(a, FS, tt_tx, tt_rx, t0=t0, coherence=True)
    assert np.array_equal(img, ref) and np.array_equal(cf, ref_cf, equal_nan=True)
    assert np.isnan(cf[-3:]).all() and np.all(img[-3:] == 0)
    assert np.array_equal(rtus.tfm_iq(_f2(a), FS, 0.0, tt_tx, tt_rx, t0=t0), ref)     # the float32 [..., 2] layout, no cf


@pytest.mark.parametrize("name", list(HMC))
@pytest.mark.parametrize("two", [False, True])
def test_f_demod_zero_is_tfm_analytic_hmc_bit_for_bit(rtus, name, two):
    h, t0, tt_a, tt_b = _hmc(name)
    img, cf = _gpu_hmc(rtus, name, two, 0.0)
    ref, ref_cf = rtus.tfm_analytic_hmc(h, FS, tt_a, tt_b if two else None, t0=t0, coherence=True)
    assert img.dtype == np.complex64 and cf.dtype == np.float32
    assert np.array_equal(img, ref) and np.array_equal(cf, ref_cf, equal_nan=True)


def test_f_demod_zero_through_the_device_entries(rtus):
    import torch
    from importlib import import_module
    dev = import_module("ray-tracing-ultrasound_amd.device")
    a, t0, tt_tx, tt_rx = _full("separate24x11")
    da, tx, rx = (torch.as_tensor(x, device="cuda") for x in (_f2(a), tt_tx, tt_rx))
    cf, cf0 = (torch.empty(N_F, dtype=torch.float32, device="cuda") for _ in range(2))
    img, _ = dev.tfm_iq_dev(da, FS, 0.0, tx, rx, t0=t0, cf=cf)
    ref, _ = dev.tfm_analytic_dev(da, FS, tx, rx, t0=t0, cf=cf0)
    assert torch.equal(img, ref) and np.array_equal(cf.cpu().numpy(), cf0.cpu().numpy(), equal_nan=True)
    assert np.array_equal(_as_c(img), _gpu_full(rtus, "separate24x11", 0.0)[0])
    h, t0, tt_a, tt_b = _hmc("tiles70")
    dh, ta, tb = (torch.as_tensor(x, device="cuda") for x in (_f2(h), tt_a, tt_b))
    for second in (None, tb):
        img, _ = dev.tfm_iq_hmc_dev(dh, FS, 0.0, ta, second, t0=t0, cf=cf)
        ref, _ = dev.tfm_analytic_hmc_dev(dh, FS, ta, second, t0=t0, cf=cf0)
        assert torch.equal(img, ref) and np.array_equal(cf.cpu().numpy(), cf0.cpu().numpy(), equal_nan=True)


# ---------------------------------------------------------------- 2. the oracle
def _check_against(img, cf, o, n_tx, n_rx, what):
    bound = (2.0 * n_tx * n_rx * 2.0 ** -24 + 1e-5) * o["A"]
    d = np.abs(img - o["image"])
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = float(np.max(np.where(o["A"] > 0, d / o["A"], 0.0)))
    assert np.array_equal(np.isnan(cf), np.isnan(o["cf"])) and np.isnan(cf[-3:]).all() and np.all(img[-3:] == 0)
    m = o["E"] >= 1e-12 * o["E"].max()
    dcf = float(np.max(np.abs(cf[m] - o["cf"][m])))
    print(f"{what}: largest |image - oracle| / A = {rel:.2e}, cf {dcf:.1e}")
    assert np.all(d <= bound), float(np.max(d - bound))
    assert dcf <= 1e-4
    fin = ~np.isnan(cf)
    assert np.all((cf[fin] >= 0) & (cf[fin] <= 1))


@pytest.mark.parametrize("nu", NUS)
@pytest.mark.parametrize("name", list(FULL))
def test_full_matrix_against_the_oracle(rtus, name, nu):
    a, t0, tt_tx, tt_rx = _full(name)
    img, cf = _gpu_full(rtus, name, nu)
    o = TQ.tfm_iq(a, FS, t0, nu * FS, tt_tx, tt_rx)
    _check_against(img, cf, o, a.shape[0], a.shape[1], f"{name} nu = {nu}")
    if name != "one1":                                                      # the carrier matters: this is not the linear image
        lin = _gpu_full(rtus, name, 0.0)[0]
        assert np.max(np.abs(img - lin)) >= 1e-2 * np.max(np.abs(lin))


@pytest.mark.parametrize("nu", NUS)
@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("name", list(HMC))
def test_half_matrix_against_the_oracle(rtus, name, two, nu):
    """two different tables: s_ij != s_ji, a swapped leg or a wrong record index shows here"""
    n_e = HMC[name][1]
    img, cf = _gpu_hmc(rtus, name, two, nu)
    _check_against(img, cf, _oracle_hmc(name, two, nu), n_e, n_e, f"{name} {'two tables' if two else 'one table'} nu = {nu}")


# ---------------------------------------------------------------- 3. half matrix against full matrix
@pytest.mark.parametrize("two", [False, True])
@pytest.mark.parametrize("name", list(HMC))
def test_half_matrix_against_the_full_matrix_kernel_on_the_unpacked_block(rtus, name, two):
    h, t0, tt_a, tt_b = _hmc(name)
    n_e, nu = HMC[name][1], 0.25
    tt_rx = tt_b if two else None
    img, cf = _gpu_hmc(rtus, name, two, nu)
    ref = rtus.tfm_iq(rtus.hmc_unpack(h), FS, nu * FS, tt_a, tt_rx, t0=t0)
    bound = 2.0 * n_e * n_e * 2.0 ** -24 * _oracle_hmc(name, two, nu)["A"]
    d = img.astype(np.complex128) - ref
    for part in (np.abs(d.real), np.abs(d.imag)):
        assert np.all(part <= bound), float(np.max(part - bound))
    if not two:                                                             # one table: the bits of the two-table form on equal tables
        i2, c2 = rtus.tfm_iq_hmc(h, FS, nu * FS, tt_a, tt_a.copy(), t0=t0, coherence=True)
        assert np.array_equal(i2, img) and np.array_equal(c2, cf, equal_nan=True)
        i3 = rtus.tfm_iq_hmc(h, FS, nu * FS, tt_a, tt_a, t0=t0)            # the same object: the one-table path
        assert np.array_equal(i3, img)


# ---------------------------------------------------------------- 4. determinism
def test_subsets_tiling_and_cf_do_not_change_the_bits(rtus):
    nu = 0.11
    sel = np.r_[np.arange(997, 3, -7), 5, 0]                   # a reversed, strided subset: other blocks, other lanes
    cols = lambda t, f: None if t is None else np.ascontiguousarray(f(t))
    twice = lambda t: np.tile(t, (1, 2))                       # n_f = 2000: 8 workgroups, the XCD-contiguous order
    runs = [(rtus.tfm_iq, _full(name), _gpu_full(rtus, name, nu)) for name in ("tiles70", "separate24x11")]
    for name, two in (("tiles70", False), ("batch17", True), ("tile40", True)):
        h, t0, tt_a, tt_b = _hmc(name)
        runs.append((rtus.tfm_iq_hmc, (h, t0, tt_a, tt_b if two else None), _gpu_hmc(rtus, name, two, nu)))
    for fn, (a, t0, tt_tx, tt_rx), (img, cf) in runs:
        assert np.array_equal(fn(a, FS, nu * FS, tt_tx, tt_rx, t0=t0), img)                # no cf: the same image bits
        s_img, s_cf = fn(a, FS, nu * FS, cols(tt_tx, lambda t: t[:, sel]), cols(tt_rx, lambda t: t[:, sel]), t0=t0, coherence="cf")
        assert np.array_equal(s_img, img[sel]) and np.array_equal(s_cf, cf[sel], equal_nan=True)
        b_img, b_cf = fn(a, FS, nu * FS, cols(tt_tx, twice), cols(tt_rx, twice), t0=t0, coherence=True)
        for k in range(2):
            part = slice(k * N_F, (k + 1) * N_F)
            assert np.array_equal(b_img[part], img) and np.array_equal(b_cf[part], cf, equal_nan=True)


# ---------------------------------------------------------------- 5. host, device and captured-graph paths
def test_host_device_and_graph_paths_agree(rtus):
    import torch
    from importlib import import_module
    dev = import_module("ray-tracing-ultrasound_amd.device")
    nu = 0.25
    a, t0, tt_tx, _ = _full("intile40")
    h, t0h, tt_a, tt_b = _hmc("tiles70")
    f_img, f_cf = _gpu_full(rtus, "intile40", nu)
    h_img, h_cf = _gpu_hmc(rtus, "tiles70", False, nu)
    t_img, t_cf = _gpu_hmc(rtus, "tiles70", True, nu)
    da, tt = torch.as_tensor(_f2(a), device="cuda"), torch.as_tensor(tt_tx, device="cuda")
    dh, ta, tb = (torch.as_tensor(x, device="cuda") for x in (_f2(h), tt_a, tt_b))
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device="cuda")
    out, cf, hout, hcf, tout = new(N_F, 2), new(N_F), new(N_F, 2), new(N_F), new(N_F, 2)
    r = dev.tfm_iq_dev(da, FS, nu * FS, tt, t0=t0, out=out, cf=cf)
    assert r[0] is out and r[1] is cf
    plain = dev.tfm_iq_dev(da, FS, nu * FS, tt, tt, t0=t0)      # allocated output, no cf, the same table twice
    r = dev.tfm_iq_hmc_dev(dh, FS, nu * FS, ta, t0=t0h, out=hout, cf=hcf)
    assert r[0] is hout and r[1] is hcf
    two, two_cf = dev.tfm_iq_hmc_dev(dh, FS, nu * FS, ta, tb, t0=t0h, cf=new(N_F))
    torch.cuda.synchronize()
    assert np.array_equal(_as_c(out), f_img) and np.array_equal(_as_c(plain), f_img)
    assert np.array_equal(cf.cpu().numpy(), f_cf, equal_nan=True)
    assert np.array_equal(_as_c(hout), h_img) and np.array_equal(hcf.cpu().numpy(), h_cf, equal_nan=True)
    assert np.array_equal(_as_c(two), t_img) and np.array_equal(two_cf.cpu().numpy(), t_cf, equal_nan=True)
    for bad in (-1.0, 0.5 * FS, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            dev.tfm_iq_dev(da, FS, bad, tt)
        with pytest.raises(ValueError):
            dev.tfm_iq_hmc_dev(dh, FS, bad, ta)
    with pytest.raises(ValueError):
        dev.tfm_iq_dev(da[..., 0].contiguous(), FS, nu * FS, tt)                         # not [..., 2]
    with pytest.raises(ValueError):
        dev.tfm_iq_dev(da, FS, nu * FS, tt, out=new(N_F))
    with pytest.raises(ValueError):
        dev.tfm_iq_dev(da, FS, nu * FS, tt[:5].contiguous())
    with pytest.raises(ValueError):
        dev.tfm_iq_hmc_dev(dh[:-1].contiguous(), FS, nu * FS, ta)                        # not n_e (n_e + 1) / 2 records
    with pytest.raises(ValueError):
        dev.tfm_iq_hmc_dev(dh, FS, nu * FS, ta, cf=torch.empty(N_F, dtype=torch.float64, device="cuda"))

    def run():
        dev.tfm_iq_dev(da, FS, nu * FS, tt, t0=t0, out=out, cf=cf)
        dev.tfm_iq_hmc_dev(dh, FS, nu * FS, ta, t0=t0h, out=hout, cf=hcf)
        dev.tfm_iq_hmc_dev(dh, FS, nu * FS, ta, tb, t0=t0h, out=tout)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                 # warm-up off the default stream, as torch.cuda.graph wants
        run()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                  # one capture stream
        run()
    for t in (out, cf, hout, hcf, tout):
        t.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(_as_c(out), f_img) and np.array_equal(cf.cpu().numpy(), f_cf, equal_nan=True)
    assert np.array_equal(_as_c(hout), h_img) and np.array_equal(hcf.cpu().numpy(), h_cf, equal_nan=True)
    assert np.array_equal(_as_c(tout), t_img)


# ---------------------------------------------------------------- 6. status codes
def test_bad_f_demod_is_a_status_code(rtus):
    import torch
    L = rtus.lib()
    a, t0, tt_tx, _ = _full("one1")
    h, _, tt_a, _ = _hmc("diag1")
    img = np.zeros(N_F, dtype=np.complex64)
    p = lambda x: x.ctypes.data
    da, dt, dimg = torch.as_tensor(_f2(a), device="cuda"), torch.as_tensor(tt_tx, device="cuda"), torch.zeros((N_F, 2), device="cuda")
    for bad in (-1.0, 0.5 * FS, float("nan"), float("inf")):
        assert L.rtus_tfm_iq(p(a), 1, 1, 300, FS, 0.0, bad, p(tt_tx), p(tt_tx), N_F, p(img), None, 0) == -1
        assert L.rtus_tfm_iq_hmc(p(h), 1, 300, FS, 0.0, bad, p(tt_a), p(tt_a), N_F, p(img), None, 0) == -1
        assert L.rtus_tfm_iq_dev(da.data_ptr(), 1, 1, 300, FS, 0.0, bad, dt.data_ptr(), dt.data_ptr(), N_F, dimg.data_ptr(), None, None) == -1
        assert L.rtus_tfm_iq_hmc_dev(da.data_ptr(), 1, 300, FS, 0.0, bad, dt.data_ptr(), dt.data_ptr(), N_F, dimg.data_ptr(), None, None) == -1
    assert not img.any() and not dimg.any()
    assert L.rtus_tfm_iq(p(a), 1, 1, 300, FS, 0.0, np.nextafter(0.5 * FS, 0.0), p(tt_tx), p(tt_tx), N_F, p(img), None, 0) == 0
    assert L.rtus_tfm_iq(p(a), 1, 1, 1, FS, 0.0, 5e6, p(tt_tx), p(tt_tx), N_F, p(img), None, 0) == \
        L.rtus_tfm_analytic(p(a), 1, 1, 1, FS, 0.0, p(tt_tx), p(tt_tx), N_F, p(img), None, 0) != 0   # the twin's codes for the rest


# ---------------------------------------------------------------- 7. end to end: a point scatterer at 4 samples per cycle
F0, FS_E, C_E, N_EL, N_T_E = 5e6, 20e6, 5900.0, 16, 256
XE, ZE = (np.arange(N_EL) - (N_EL - 1) / 2) * 0.6e-3, np.zeros(N_EL)
SCAT = (1.3e-3, 20e-3)


@functools.lru_cache(maxsize=None)
def _scatterer(rtus):
    """the analytic FMC of one unit scatterer from the simulator (the wavelet table oversampled 16 times: its own linear
    interpolation costs 0.12 %) and the table over a 5 x 5 grid of 0.1 mm pitch whose centre (index 12) is the scatterer"""
    pulse, centre = rtus.gaussian_pulse(F0, 3, FS_E, oversample=16)
    tts = rtus.travel_time_layers([], [C_E], XE, ZE, [SCAT[0]], [SCAT[1]])
    a = rtus.simulate_fmc(tts, fs=FS_E, n_t=N_T_E, pulse=pulse, centre=centre, oversample=16, analytic=True)
    gx, gz = np.meshgrid(SCAT[0] + 1e-4 * np.arange(-2, 3), SCAT[1] + 1e-4 * np.arange(-2, 3))
    return a, rtus.travel_time_layers([], [C_E], XE, ZE, gx.ravel(), gz.ravel())


def test_point_scatterer_reads_one_with_the_carrier_and_low_without(rtus):
    a, tt = _scatterer(rtus)
    n = N_EL * N_EL
    iq, cf = rtus.tfm_iq(a, FS_E, F0, tt, coherence=True)
    lin = rtus.tfm_analytic(a, FS_E, tt)
    got, got_lin = abs(iq[12]) / n, abs(lin[12]) / n
    est = rtus.centre_frequency(a, FS_E)
    from_data = abs(rtus.tfm_iq(a, FS_E, est, tt)[12]) / n
    packed = abs(rtus.tfm_iq_hmc(rtus.hmc_pack(a), FS_E, F0, tt)[12]) / n
    print(f"|S|/N at the scatterer: carrier-aware {got:.4f} (f_demod from the data, {est / 1e6:.3f} MHz: {from_data:.4f}; "
          f"half matrix {packed:.4f}), linear {got_lin:.4f}; cf {cf[12]:.4f}")
    assert got >= 0.99
    assert got_lin <= 0.85
    assert abs(est - F0) <= 0.01 * F0 and from_data >= 0.99 and packed >= 0.99
    assert cf[12] >= 0.99                                                   # (terms within 0.005 of 1: cf = 1 - their variance)


def test_tfm_views_with_f_demod_is_tfm_iq_per_view(rtus):
    a, tt = _scatterer(rtus)
    rf = np.ascontiguousarray(a.real)
    legs = {"L": tt, "T": tt * (5900.0 / 3200.0)}
    views = ("L-L", "L-T")
    tables = {"L-L": (legs["L"], legs["L"]), "L-T": (legs["L"], legs["T"])}
    an = rtus.fmc_analytic(rf)
    got = rtus.tfm_views(rf, FS_E, legs, views, envelope=True, f_demod=F0)
    got_cf = rtus.tfm_views(rf, FS_E, legs, views, envelope=True, coherence=True, f_demod=F0)
    for v in views:
        img, cf = rtus.tfm_iq(an, FS_E, F0, *tables[v], coherence=True)
        assert got[v].dtype == np.float32 and np.array_equal(got[v], np.abs(img))
        assert np.array_equal(got_cf[v][0], np.abs(img)) and np.array_equal(got_cf[v][1], cf, equal_nan=True)
    h = rtus.hmc_pack(rf)
    han = rtus.hmc_analytic(h)
    got = rtus.tfm_views(h, FS_E, legs, views, envelope=True, coherence="cf", hmc=True, f_demod=F0)
    for v in views:
        img, cf = rtus.tfm_iq_hmc(han, FS_E, F0, *tables[v], coherence=True)
        assert np.array_equal(got[v][0], np.abs(img)) and np.array_equal(got[v][1], cf, equal_nan=True)
    # None: the linear kernels, as before
    old = rtus.tfm_views(rf, FS_E, legs, "L-T", envelope=True, f_demod=None)
    assert np.array_equal(old["L-T"], np.abs(rtus.tfm_analytic(an, FS_E, *tables["L-T"])))
    assert not np.array_equal(old["L-T"], rtus.tfm_views(rf, FS_E, legs, "L-T", envelope=True, f_demod=F0)["L-T"])


def test_pwi_image_with_f_demod_is_its_hand_composed_form(rtus):
    a, t0, tt_tx, tt_rx = _full("separate24x11")
    pw = np.ascontiguousarray(a.real)
    env, cf = rtus.pwi_image(pw, FS, tt_tx, tt_rx, t0=t0, envelope=True, coherence=True, f_demod=0.11 * FS)
    img, cf0 = rtus.tfm_iq(rtus.fmc_analytic(pw), FS, 0.11 * FS, tt_tx, tt_rx, t0=t0, coherence=True)
    assert env.dtype == np.float32 and np.array_equal(env, np.abs(img)) and np.array_equal(cf, cf0, equal_nan=True)
    assert np.array_equal(rtus.pwi_image(pw, FS, tt_tx, tt_rx, t0=t0, envelope=True, f_demod=0.11 * FS), env)
    assert np.array_equal(rtus.pwi_image(pw, FS, tt_tx, tt_rx, t0=t0, envelope=True),
                          np.abs(rtus.tfm_analytic(rtus.fmc_analytic(pw), FS, tt_tx, tt_rx, t0=t0)))


# adaptive_tfm: test_gpu_tfm_analytic.py's wavy surface
AC1, AC2, AFS, ANT = 1480.0, 5900.0, 50e6, 2400
AXE, AZE = (np.arange(64) - 31.5) * 0.25e-3, np.zeros(64)
SX0, SDX = -0.016, 0.0005
SZS = 0.020 + 0.0005 * np.sin(2 * np.pi * (SX0 + SDX * np.arange(65)) / 0.020)
DX, X0, NS = 2.0 ** -11, -16 * 2.0 ** -11, 33
DZ, ZLO, ZHI = AC1 / 5e6 / 8, 0.017, 0.023
HOLE = (0.001, 0.038)


def test_adaptive_tfm_with_f_demod_is_its_hand_composed_form(rtus):
    fmc = AF.synth_fmc(AXE, AZE, AC1, AFS, ANT, SX0, SDX, SZS, -0.012, 0.012, scatterer=(HOLE[0], HOLE[1], 1.0), c2=AC2)
    pix = 1e-4
    gx, gz = np.meshgrid(HOLE[0] + pix * np.arange(-5, 6), HOLE[1] + pix * np.arange(-5, 6))
    args = (fmc, AFS, AXE, AZE, AC1, AC2, X0, DX, NS, ZLO, ZHI, DZ, gx.ravel(), gz.ravel())
    f_demod = rtus.centre_frequency(fmc, AFS)
    env, surf = rtus.adaptive_tfm(*args, envelope=True, f_demod=f_demod)
    old, surf_old = rtus.adaptive_tfm(*args, envelope=True)
    assert np.array_equal(surf["zs"], surf_old["zs"]) and surf["x0"] == surf_old["x0"]      # the surface measurement stays
    tt = rtus.travel_time_surface(surf["x0"], surf["dx"], surf["zs"], AC1, AC2, AXE, AZE, gx.ravel(), gz.ravel())
    an = rtus.fmc_analytic(fmc)
    assert env.dtype == np.float32 and np.array_equal(env, np.abs(rtus.tfm_iq(an, AFS, f_demod, tt)))
    assert np.array_equal(old, np.abs(rtus.tfm_analytic(an, AFS, tt)))
    iz, ix = np.unravel_index(np.argmax(env.reshape(gx.shape)), gx.shape)
    assert abs(iz - 5) <= 1 and abs(ix - 5) <= 1, (iz, ix)

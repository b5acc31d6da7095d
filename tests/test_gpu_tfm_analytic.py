"""GPU: the envelope TFM with coherence factor (rtus_tfm_analytic*) — bit identity with rtus_tfm on each plane of the analytic
FMC, the NumPy oracle (tests/tfm_analytic_numpy.py), determinism under any sharing of the call, host / device / captured-graph
paths, point-scatterer physics with and without noise, and adaptive_tfm(envelope=True) on the wavy-surface case.

Tolerances, calibrated on the CPU with an fp32 emulation of the kernel (fp32 legs and positions, fp32 sums in rtus_tfm's order)
against the fp64 oracle:
  image: <= 2e-4 of the image maximum (test_gpu_tfm.py's; the emulation is within 1.7e-5);
  cf:    <= 1e-4 absolute where E >= 1e-12 of its maximum (the emulation: 7e-6 on point scatterers, 3.5e-7 on random data).  Where
         E is smaller still (deep in the tails of every echo, E ~ 1e-50 of its maximum) the fp32 sample position decides the ratio
         of two underflowing sums, and cf carries no information.
"""
import functools

import numpy as np
import pytest

import autofocus_numpy as AF
import tfm_analytic_numpy as TA
from oracle import tfm_numpy as T

pytestmark = pytest.mark.gpu


def _case(seed, n_tx, n_rx, n_t, n_f, t0, same):
    """random complex FMC; half positions from 12 samples before the record to 12 past the half of it (pair positions cross both
    ends); NaN, absurd (5e10 samples) and infinite legs; the last three focal points without any path"""
    rng = np.random.default_rng(seed)
    fs = 40e6
    a = (rng.standard_normal((n_tx, n_rx, n_t)) + 1j * rng.standard_normal((n_tx, n_rx, n_t))).astype(np.complex64)
    lo, hi = (-12 + 0.5 * t0 * fs) / fs, (n_t / 2 + 12 + 0.5 * t0 * fs) / fs
    tt_tx = rng.uniform(lo, hi, (n_tx, n_f))
    tt_rx = tt_tx if same else rng.uniform(lo, hi, (n_rx, n_f))
    for t in ((tt_tx,) if same else (tt_tx, tt_rx)):
        m = rng.random(t.shape)
        t[m < 0.03] = np.nan
        t[(m >= 0.03) & (m < 0.035)] = 1e3
        t[(m >= 0.035) & (m < 0.037)] = -np.inf
        t[(m >= 0.037) & (m < 0.039)] = np.inf
    tt_tx[:, -3:] = np.nan
    return a, fs, t0, tt_tx, (None if same else tt_rx)


CASES = {
    "tiles70": (1, 70, 70, 500, 1000, 1.5e-6, True),        # one table, two receive tiles (70 = 4 x 16 + 6)
    "separate24x11": (2, 24, 11, 400, 1000, 2.0e-6, False),  # separate tables
    "intile40": (3, 40, 40, 300, 1000, 0.0, True),           # one table, the transmit delays read from the tile, t0 = 0
}


@pytest.mark.parametrize("name", list(CASES))
def test_planes_are_rtus_tfm_bit_for_bit(rtus, name):
    a, fs, t0, tt_tx, tt_rx = _case(*CASES[name])
    img, cf = rtus.tfm_analytic(a, fs, tt_tx, tt_rx, t0=t0, coherence=True)
    assert img.dtype == np.complex64 and img.shape == (tt_tx.shape[1],) and cf.dtype == np.float32
    re = rtus.tfm_image(np.ascontiguousarray(a.real), fs, tt_tx, tt_rx, t0=t0)
    im = rtus.tfm_image(np.ascontiguousarray(a.imag), fs, tt_tx, tt_rx, t0=t0)
    assert np.array_equal(img.real, re) and np.array_equal(img.imag, im)
    # the float32 [..., 2] layout, and no cf: the same bits
    f2 = np.ascontiguousarray(a.view(np.float32).reshape(*a.shape, 2))
    assert np.array_equal(rtus.tfm_analytic(f2, fs, tt_tx, tt_rx, t0=t0), img)


@pytest.mark.parametrize("name", list(CASES))
def test_against_the_oracle(rtus, name):
    a, fs, t0, tt_tx, tt_rx = _case(*CASES[name])
    img, cf = rtus.tfm_analytic(a, fs, tt_tx, tt_rx, t0=t0, coherence=True)
    o = TA.tfm_analytic(a, fs, t0, tt_tx, tt_rx)
    err = np.max(np.abs(img - o["image"])) / np.max(np.abs(o["image"]))
    assert err <= 2e-4, err
    assert np.array_equal(np.isnan(cf), np.isnan(o["cf"])) and np.isnan(cf[-3:]).all() and np.all(img[-3:] == 0)
    m = o["E"] >= 1e-12 * o["E"].max()
    dcf = np.max(np.abs(cf[m] - o["cf"][m]))
    print(f"{name}: image {err:.1e} of max, cf {dcf:.1e}")
    assert dcf <= 1e-4
    fin = ~np.isnan(cf)
    assert np.all((cf[fin] >= 0) & (cf[fin] <= 1))


def test_subsets_and_cf_do_not_change_the_bits(rtus):
    a, fs, t0, tt_tx, tt_rx = _case(*CASES["separate24x11"])
    img, cf = rtus.tfm_analytic(a, fs, tt_tx, tt_rx, t0=t0, coherence=True)
    assert np.array_equal(rtus.tfm_analytic(a, fs, tt_tx, tt_rx, t0=t0), img)              # no cf: same image bits
    sel = np.r_[np.arange(997, 3, -7), 5, 0]                   # a reversed, strided subset: other blocks, other lanes
    s_img, s_cf = rtus.tfm_analytic(a, fs, np.ascontiguousarray(tt_tx[:, sel]), np.ascontiguousarray(tt_rx[:, sel]), t0=t0,
                                    coherence=True)
    assert np.array_equal(s_img, img[sel]) and np.array_equal(s_cf, cf[sel], equal_nan=True)
    big = np.tile(tt_tx, (1, 2))                               # n_f = 2000: 8 workgroups, the XCD-contiguous order
    b_img, b_cf = rtus.tfm_analytic(a, fs, big, np.tile(tt_rx, (1, 2)), t0=t0, coherence=True)
    for k in range(2):
        assert np.array_equal(b_img[k * 1000:(k + 1) * 1000], img) and np.array_equal(b_cf[k * 1000:(k + 1) * 1000], cf, equal_nan=True)


def test_host_device_and_graph_paths_agree(rtus):
    import torch
    from importlib import import_module
    dev = import_module("ray-tracing-ultrasound_amd.device")
    a, fs, t0, tt_tx, _ = _case(*CASES["intile40"])
    h_img, h_cf = rtus.tfm_analytic(a, fs, tt_tx, t0=t0, coherence=True)
    da = torch.as_tensor(np.ascontiguousarray(a.view(np.float32).reshape(*a.shape, 2)), device="cuda")
    tt = torch.as_tensor(tt_tx, device="cuda")
    n_f = tt_tx.shape[1]
    out = torch.empty((n_f, 2), dtype=torch.float32, device="cuda")
    cf = torch.empty(n_f, dtype=torch.float32, device="cuda")
    r = dev.tfm_analytic_dev(da, fs, tt, t0=t0, out=out, cf=cf)
    assert r[0] is out and r[1] is cf
    plain = dev.tfm_analytic_dev(da, fs, tt, tt, t0=t0)         # allocated output, no cf, the same table twice
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.complex64)[:, 0], h_img)
    assert np.array_equal(plain.cpu().numpy().view(np.complex64)[:, 0], h_img)
    assert np.array_equal(cf.cpu().numpy(), h_cf, equal_nan=True)
    with pytest.raises(ValueError):
        dev.tfm_analytic_dev(da[..., 0].contiguous(), fs, tt)                          # not [..., 2]
    with pytest.raises(ValueError):
        dev.tfm_analytic_dev(da, fs, tt, out=torch.empty(n_f, dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError):
        dev.tfm_analytic_dev(da, fs, tt, cf=torch.empty(n_f, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        dev.tfm_analytic_dev(da, fs, tt[:5].contiguous())

    def run():
        dev.tfm_analytic_dev(da, fs, tt, t0=t0, out=out, cf=cf)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                 # warm-up off the default stream, as torch.cuda.graph wants
        run()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                  # one capture stream
        run()
    out.fill_(float("nan")); cf.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.complex64)[:, 0], h_img)
    assert np.array_equal(cf.cpu().numpy(), h_cf, equal_nan=True)


# ---------------------------------------------------------------- physics: two point scatterers (test_gpu_tfm.py's set-up)
N_EL, C, FS, NT = 32, 1500.0, 50e6, 2200
SCAT = [(0.003, 0.020, 1.0), (-0.004, 0.026, 0.7)]
XS, ZS = np.meshgrid(np.linspace(-0.008, 0.008, 81), np.linspace(0.015, 0.031, 81))


@functools.lru_cache(maxsize=None)
def _scatterers(rtus, noise):
    x = (np.arange(N_EL) - (N_EL - 1) / 2) * 0.6e-3
    z = np.zeros(N_EL)
    fmc = T.synth_fmc(x, z, SCAT, C, FS, NT)
    if noise:
        fmc = (fmc + np.random.default_rng(11).normal(0.0, noise, fmc.shape)).astype(np.float32)
    tt = rtus.travel_time_layers([], [C], x, z, XS.ravel(), ZS.ravel())             # the library's own table
    a = rtus.fmc_analytic(fmc)
    img, cf = rtus.tfm_analytic(a, FS, tt, coherence=True)
    return a, tt, img, cf


def _far():
    far = np.ones(XS.shape, bool)
    for sx, sz, _ in SCAT:
        far &= np.hypot(XS - sx, ZS - sz) > 2e-3
    return far


def _at(sx, sz):
    return int(np.argmin(np.abs(ZS[:, 0] - sz))), int(np.argmin(np.abs(XS[0] - sx)))


def test_point_scatterers_envelope_and_cf(rtus):
    """thresholds from the oracle on the CPU: the envelope peaks AT both scatterers (offset 0), cf there 0.9997 against a background
    median of 1.6e-4"""
    a, tt, img, cf = _scatterers(rtus, 0.0)
    o = TA.tfm_analytic(a, FS, 0.0, tt)
    assert np.max(np.abs(img - o["image"])) <= 2e-4 * np.max(np.abs(o["image"]))
    m = o["E"] >= 1e-12 * o["E"].max()
    assert np.max(np.abs(cf[m] - o["cf"][m])) <= 1e-4
    env, cf = np.abs(img).reshape(XS.shape), cf.reshape(XS.shape)
    bg = np.median(cf[_far()])
    for sx, sz, _ in SCAT:
        i0, j0 = _at(sx, sz)
        win = env[i0 - 6:i0 + 7, j0 - 6:j0 + 7]
        k = np.unravel_index(np.argmax(win), win.shape)
        assert abs(k[0] - 6) <= 1 and abs(k[1] - 6) <= 1, k
        c = cf[i0 - 1:i0 + 2, j0 - 1:j0 + 2].max()
        print(f"scatterer ({sx}, {sz}): cf {c:.4f}, background median {bg:.2e}")
        assert c >= 0.9 and c >= 100 * bg


def test_cf_weighting_raises_the_contrast_in_noise(rtus):
    """white noise of twice the echo amplitude on every A-scan.  Oracle on the CPU: peak / background median 15.7 and 11.3 for the
    envelope, 3390 and 1358 for envelope x cf: the CF-weighted image must win by a factor of 10 at least"""
    a, tt, img, cf = _scatterers(rtus, 2.0)
    env = np.abs(img).reshape(XS.shape)
    weighted = env * cf.reshape(XS.shape)
    far = _far()
    for sx, sz, _ in SCAT:
        i0, j0 = _at(sx, sz)
        r_env = env[i0 - 2:i0 + 3, j0 - 2:j0 + 3].max() / np.median(env[far])
        r_cf = weighted[i0 - 2:i0 + 3, j0 - 2:j0 + 3].max() / np.median(weighted[far])
        print(f"scatterer ({sx}, {sz}): peak / background median, envelope {r_env:.1f}, envelope x cf {r_cf:.1f}")
        assert r_env >= 5 and r_cf >= 10 * r_env


# ---------------------------------------------------------------- adaptive_tfm(envelope=True): test_gpu_autofocus.py's wavy surface
AC1, AC2, AFS, ANT = 1480.0, 5900.0, 50e6, 2400
AXE, AZE = (np.arange(64) - 31.5) * 0.25e-3, np.zeros(64)
SX0, SDX = -0.016, 0.0005
SZS = 0.020 + 0.0005 * np.sin(2 * np.pi * (SX0 + SDX * np.arange(65)) / 0.020)
DX, X0, NS = 2.0 ** -11, -16 * 2.0 ** -11, 33
DZ, ZLO, ZHI = AC1 / 5e6 / 8, 0.017, 0.023
HOLE = (0.001, 0.038)


def test_adaptive_tfm_envelope_images_the_hole(rtus):
    fmc = AF.synth_fmc(AXE, AZE, AC1, AFS, ANT, SX0, SDX, SZS, -0.012, 0.012, scatterer=(HOLE[0], HOLE[1], 1.0), c2=AC2)
    pix = 1e-4
    gx, gz = np.meshgrid(HOLE[0] + pix * np.arange(-10, 11), HOLE[1] + pix * np.arange(-10, 11))
    args = (fmc, AFS, AXE, AZE, AC1, AC2, X0, DX, NS, ZLO, ZHI, DZ, gx.ravel(), gz.ravel())
    env, surf = rtus.adaptive_tfm(*args, envelope=True)
    assert env.dtype == np.float32 and env.shape == (gx.size,)
    iz, ix = np.unravel_index(np.argmax(env.reshape(gx.shape)), gx.shape)
    assert abs(iz - 10) <= 1 and abs(ix - 10) <= 1, (iz, ix)
    # the same as building it by hand from the returned profile
    tt = rtus.travel_time_surface(surf["x0"], surf["dx"], surf["zs"], AC1, AC2, AXE, AZE, gx.ravel(), gz.ravel())
    assert np.array_equal(env, np.abs(rtus.tfm_analytic(rtus.fmc_analytic(fmc), AFS, tt)))
    # the default is the RF image, exactly as before
    rf, surf_rf = rtus.adaptive_tfm(*args)
    assert np.array_equal(surf_rf["zs"], surf["zs"]) and surf_rf["x0"] == surf["x0"]
    assert np.array_equal(rf, rtus.tfm_image(fmc, AFS, tt))
    assert np.array_equal(rf, rtus.tfm_analytic(rtus.fmc_analytic(fmc), AFS, tt).real)

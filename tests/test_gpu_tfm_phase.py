"""GPU: phase-coherence imaging (rtus_tfm_phase*) — the image is rtus_tfm_analytic's bit for bit, the integer sums are the fp32
oracle's exactly, scf and vcf against tests/tfm_phase_numpy.py, determinism under any sharing of the call, host / device /
captured-graph paths, point-scatterer physics with and without noise, and the ``coherence=`` keyword of tfm_analytic, tfm_views and
pwi_image.

The bar of vcf (test_vcf_against_the_oracle): the comparison is against the fp32=True oracle — the kernel's p_k, phasors and sums
in fp64 — so what is left is the kernel's fp32 phasors and its recursive fp32 sum.
  hard cap: (N_max + 8) 2^-23 absolute = 5.85e-4 at N_max = 4900 (N terms of modulus <= 1 summed recursively in fp32, a factor
            sqrt 2 for the two components, 8 ulp for forming a phasor; divided by N the bound on vcf is far smaller still, the
            cap is not taken that far);
  asserted: VCF_BAR = 4 x the largest |vcf32 - vcf| of the oracle's float32 kernel-order sum against its fp64 sum on the three
            cases, measured on the CPU (tiles70 7.53e-8, separate24x11 5.71e-8, intile40 5.67e-8): 4 x 7.53e-8 = 3.0e-7.  The factor 4
            leaves room for the hardware's reciprocal square root and the phasor products, which the emulation does not reproduce.
  observed on MI355X: tiles70 8.3e-8, separate24x11 5.0e-8, intile40 5.7e-8 (scf: 0 on all three).
"""
import functools

import numpy as np
import pytest

import tfm_phase_numpy as TP
from oracle import tfm_numpy as T

pytestmark = pytest.mark.gpu

VCF_BAR = 3.0e-7
VCF_CAP = (4900 + 8) * 2.0 ** -23


def _case(seed, n_tx, n_rx, n_t, n_f, t0, same):
    """test_gpu_tfm_analytic.py's generator — random complex FMC; half positions from 12 samples before the record to 12 past the
    half of it; NaN, absurd (5e10 samples) and infinite legs; the last three focal points without any path — and then: a band of
    zero samples inside the record, a silent transmit row, and two rows whose squared modulus under- / overflows in fp32 (every
    non-zero magnitude stays a normal fp32 number: |N(0, 1)| x 1e-30 > 1.2e-38 down to 1e-8 of a standard deviation)"""
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
    a[:, :, 100:140] = 0
    a[1] = 0
    a[2] *= np.float32(1e-30)
    a[3] *= np.float32(1e30)
    return a, fs, t0, tt_tx, (None if same else tt_rx)


CASES = {
    "tiles70": (1, 70, 70, 500, 1000, 1.5e-6, True),        # one table, two receive tiles (70 = 4 x 16 + 6)
    "separate24x11": (2, 24, 11, 400, 1000, 2.0e-6, False),  # separate tables
    "intile40": (3, 40, 40, 300, 1000, 0.0, True),           # one table, the transmit delays read from the tile, t0 = 0
}


@functools.lru_cache(maxsize=None)
def _gpu(rtus, name):
    """the case, the library's full result and the fp32 oracle: computed once, read by every test"""
    a, fs, t0, tt_tx, tt_rx = _case(*CASES[name])
    mag = np.abs(a.view(np.float32))
    assert mag[mag > 0].min() >= np.finfo(np.float32).tiny and np.isfinite(mag).all()      # every non-zero magnitude is normal
    r = rtus.tfm_phase(a, fs, tt_tx, tt_rx, t0=t0, counts=True)
    o = TP.tfm_phase(a, fs, t0, tt_tx, tt_rx, fp32=True)
    for v in (*r.values(), *o.values(), a, tt_tx):
        v.flags.writeable = False
    return (a, fs, t0, tt_tx, tt_rx), r, o


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32 if x.dtype.itemsize % 8 else np.uint64)


def _same(x, y):
    return x.dtype == y.dtype and x.shape == y.shape and np.array_equal(_bits(x), _bits(y))


@pytest.mark.parametrize("name", list(CASES))
def test_image_is_tfm_analytic_bit_for_bit_whatever_is_asked_for(rtus, name):
    """1. every combination of the optional outputs of the C entry: the same image, and the same bits of each other"""
    (a, fs, t0, tt_tx, tt_rx), r, _ = _gpu(rtus, name)
    n_f = tt_tx.shape[1]
    assert r["image"].dtype == np.complex64 and r["image"].shape == (n_f,)
    assert r["vcf"].dtype == r["scf"].dtype == np.float32 and r["sign_sum"].dtype == r["n_pairs"].dtype == np.int32
    ref = rtus.tfm_analytic(a, fs, tt_tx, tt_rx, t0=t0)
    assert _same(r["image"], ref)
    L = rtus.lib()
    rx = tt_tx if tt_rx is None else tt_rx
    full = dict(vcf=r["vcf"], scf=r["scf"], counts=np.stack([r["sign_sum"], r["n_pairs"]], axis=1))
    for mask in range(8):
        img = np.full(n_f, np.nan, dtype=np.complex64)
        got = dict(vcf=np.full(n_f, np.nan, dtype=np.float32) if mask & 1 else None,
                   scf=np.full(n_f, np.nan, dtype=np.float32) if mask & 2 else None,
                   counts=np.full((n_f, 2), -7, dtype=np.int32) if mask & 4 else None)
        ptr = {k: (None if v is None else v.ctypes.data) for k, v in got.items()}
        st = L.rtus_tfm_phase(a.ctypes.data, a.shape[0], a.shape[1], a.shape[2], fs, t0, tt_tx.ctypes.data, rx.ctypes.data, n_f,
                              img.ctypes.data, ptr["vcf"], ptr["scf"], ptr["counts"], 0)
        assert st == 0, (mask, st)
        assert _same(img, ref), mask
        for k, v in got.items():
            assert v is None or _same(v, full[k]), (mask, k)


def test_the_cases_do_not_depend_on_a_fused_leg(rtus):
    """the legs' float32 values are the same whether t fs - t0 fs / 2 is rounded twice or once in fp64 (a compiler may contract
    it): the exact integer check below holds for either build"""
    for name in CASES:
        _, fs, t0, tt_tx, tt_rx = _gpu(rtus, name)[0]
        for t in (tt_tx,) if tt_rx is None else (tt_tx, tt_rx):
            assert _same(TP.legs_f32(t, fs, t0), TP.legs_f32(t, fs, t0, fused=True))


@pytest.mark.parametrize("name", list(CASES))
def test_counts_are_exact(rtus, name):
    """2. N and the sign sum as integers at every focal point against the fp32 oracle (the kernel's p_k): derived, no tolerance"""
    (a, fs, t0, tt_tx, tt_rx), r, o = _gpu(rtus, name)
    assert np.array_equal(r["n_pairs"], o["N"])
    bad = np.nonzero(r["sign_sum"] != o["B"])[0]
    assert bad.size == 0, (bad[:10], r["sign_sum"][bad[:10]], o["B"][bad[:10]])
    assert np.all(r["n_pairs"][-3:] == 0) and np.all(r["sign_sum"][-3:] == 0) and o["N"].max() > 0.8 * a.shape[0] * a.shape[1]
    assert np.abs(o["B"]).max() > 0


@pytest.mark.parametrize("name", list(CASES))
def test_scf_from_the_integers(rtus, name):
    """3. within 2 x 2^-24 of float32(1 - sqrt(1 - (B / N)^2)): one rounding in fp64 and one to fp32"""
    _, r, o = _gpu(rtus, name)
    want = TP.scf_of(r["sign_sum"], r["n_pairs"]).astype(np.float32)
    assert np.array_equal(np.isnan(r["scf"]), np.isnan(want)) and np.isnan(r["scf"][-3:]).all()
    fin = ~np.isnan(want)
    err = np.max(np.abs(r["scf"][fin].astype(np.float64) - want[fin]))
    print(f"{name}: scf {err:.2e}")
    assert err <= 2 * 2.0 ** -24, err
    assert np.all((r["scf"][fin] >= 0) & (r["scf"][fin] <= 1))


@pytest.mark.parametrize("name", list(CASES))
def test_vcf_against_the_oracle(rtus, name):
    """4. NaN masks, range, and VCF_BAR (module docstring) against the fp32-position oracle with fp64 phasors and sums"""
    _, r, o = _gpu(rtus, name)
    assert VCF_BAR < VCF_CAP and o["N"].max() <= 4900
    assert np.array_equal(np.isnan(r["vcf"]), np.isnan(o["vcf"])) and np.isnan(r["vcf"][-3:]).all()
    fin = ~np.isnan(o["vcf"])
    assert np.all((r["vcf"][fin] >= 0) & (r["vcf"][fin] <= 1))
    err = np.max(np.abs(r["vcf"][fin].astype(np.float64) - o["vcf"][fin]))
    print(f"{name}: vcf {err:.2e} (bar {VCF_BAR:.1e}, cap {VCF_CAP:.2e})")
    assert err <= VCF_BAR, err


def test_subsets_do_not_change_the_bits(rtus):
    """5. a reversed strided subset of the focal points, and the tables tiled to 8 workgroups (the XCD-contiguous order)"""
    (a, fs, t0, tt_tx, tt_rx), r, _ = _gpu(rtus, "separate24x11")
    keys = ("image", "vcf", "scf", "sign_sum", "n_pairs")
    sel = np.r_[np.arange(997, 3, -7), 5, 0]
    s = rtus.tfm_phase(a, fs, np.ascontiguousarray(tt_tx[:, sel]), np.ascontiguousarray(tt_rx[:, sel]), t0=t0, counts=True)
    for k in keys:
        assert _same(s[k], r[k][sel]), k
    b = rtus.tfm_phase(a, fs, np.tile(tt_tx, (1, 2)), np.tile(tt_rx, (1, 2)), t0=t0, counts=True)
    for k in keys:
        for j in range(2):
            assert _same(b[k][j * 1000:(j + 1) * 1000], r[k]), (k, j)


def test_host_device_and_graph_paths_agree(rtus):
    """6. one capture stream, pre-allocated outputs, poisoned before the replay"""
    import torch
    from importlib import import_module
    dev = import_module("ray-tracing-ultrasound_amd.device")
    (a, fs, t0, tt_tx, _), r, _ = _gpu(rtus, "intile40")
    da = torch.as_tensor(np.array(a.view(np.float32).reshape(*a.shape, 2)), device="cuda")
    tt = torch.as_tensor(np.array(tt_tx), device="cuda")
    n_f = tt_tx.shape[1]
    out = torch.empty((n_f, 2), dtype=torch.float32, device="cuda")
    vcf = torch.empty(n_f, dtype=torch.float32, device="cuda")
    scf = torch.empty(n_f, dtype=torch.float32, device="cuda")
    cnt = torch.empty((n_f, 2), dtype=torch.int32, device="cuda")

    def check():
        torch.cuda.synchronize()
        assert _same(out.cpu().numpy().view(np.complex64)[:, 0], r["image"])
        assert _same(vcf.cpu().numpy(), r["vcf"]) and _same(scf.cpu().numpy(), r["scf"])
        c = cnt.cpu().numpy()
        assert np.array_equal(c[:, 0], r["sign_sum"]) and np.array_equal(c[:, 1], r["n_pairs"])

    got = dev.tfm_phase_dev(da, fs, tt, t0=t0, out=out, vcf=vcf, scf=scf, counts=cnt)
    assert len(got) == 4 and got[0] is out and got[1] is vcf and got[2] is scf and got[3] is cnt
    check()
    plain = dev.tfm_phase_dev(da, fs, tt, tt, t0=t0)            # allocated output, nothing else, the same table twice
    o2, s2 = dev.tfm_phase_dev(da, fs, tt, t0=t0, scf=torch.empty_like(scf))
    torch.cuda.synchronize()
    assert _same(plain.cpu().numpy().view(np.complex64)[:, 0], r["image"])
    assert _same(o2.cpu().numpy().view(np.complex64)[:, 0], r["image"]) and _same(s2.cpu().numpy(), r["scf"])
    f32, f64, i32 = (lambda n: torch.empty(n, dtype=torch.float32, device="cuda")), \
        (lambda n: torch.empty(n, dtype=torch.float64, device="cuda")), (lambda n: torch.empty(n, dtype=torch.int32, device="cuda"))
    for kw in (dict(vcf=f64(n_f)), dict(vcf=f32(n_f + 1)), dict(scf=f64(n_f)), dict(scf=f32(n_f - 1)), dict(counts=f32(2 * n_f)),
               dict(counts=i32(n_f)), dict(out=f32(n_f))):
        with pytest.raises(ValueError):
            dev.tfm_phase_dev(da, fs, tt, t0=t0, **kw)
    with pytest.raises(ValueError):
        dev.tfm_phase_dev(da[..., 0].contiguous(), fs, tt)       # not [..., 2]

    def run():
        dev.tfm_phase_dev(da, fs, tt, t0=t0, out=out, vcf=vcf, scf=scf, counts=cnt)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                                 # warm-up off the default stream, as torch.cuda.graph wants
        run()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                  # one capture stream
        run()
    out.fill_(float("nan")); vcf.fill_(float("nan")); scf.fill_(float("nan")); cnt.fill_(-7)
    g.replay()
    check()


# ---------------------------------------------------------------- physics: two point scatterers (test_gpu_tfm_analytic.py's scene)
N_EL, C, FS, NT = 32, 1500.0, 50e6, 2200
SCAT = [(0.003, 0.020, 1.0), (-0.004, 0.026, 0.7)]
XS, ZS = np.meshgrid(np.linspace(-0.008, 0.008, 81), np.linspace(0.015, 0.031, 81))
XE, ZE = (np.arange(N_EL) - (N_EL - 1) / 2) * 0.6e-3, np.zeros(N_EL)


@functools.lru_cache(maxsize=None)
def _scatterers(rtus, noise):
    fmc = T.synth_fmc(XE, ZE, SCAT, C, FS, NT)
    if noise:
        fmc = (fmc + np.random.default_rng(11).normal(0.0, noise, fmc.shape)).astype(np.float32)
    tt = rtus.travel_time_layers([], [C], XE, ZE, XS.ravel(), ZS.ravel())            # the library's own table
    a = rtus.fmc_analytic(fmc)
    return fmc, a, tt, rtus.tfm_phase(a, FS, tt)


def _far():
    far = np.ones(XS.shape, bool)
    for sx, sz, _ in SCAT:
        far &= np.hypot(XS - sx, ZS - sz) > 2e-3
    return far


def _at(sx, sz):
    return int(np.argmin(np.abs(ZS[:, 0] - sz))), int(np.argmin(np.abs(XS[0] - sx)))


def test_point_scatterers_without_noise(rtus):
    """7. CPU oracle: vcf and scf 1.0000 at both scatterers; background medians 1.45e-2 (vcf) and 6.9e-5 (scf)"""
    _, _, _, r = _scatterers(rtus, 0.0)
    vcf, scf = r["vcf"].reshape(XS.shape), r["scf"].reshape(XS.shape)
    far = _far()
    bv, bs = np.median(vcf[far]), np.median(scf[far])
    print(f"background medians: vcf {bv:.2e}, scf {bs:.2e}")
    assert bv <= 0.05 and bs <= 1e-3
    for sx, sz, _ in SCAT:
        i0, j0 = _at(sx, sz)
        v, s = vcf[i0 - 1:i0 + 2, j0 - 1:j0 + 2].max(), scf[i0 - 1:i0 + 2, j0 - 1:j0 + 2].max()
        print(f"scatterer ({sx}, {sz}): vcf {v:.4f}, scf {s:.4f}")
        assert v >= 0.99 and s >= 0.99


def test_phase_weighting_raises_the_contrast_in_noise(rtus):
    """8. white noise of twice the echo amplitude (sigma 2.0, seed 11); peak (5 x 5) over background median.  CPU oracle: envelope x
    vcf beats the envelope by 14x and 10x, envelope x scf by 577x and 300x; the ``coherence=`` keyword returns tfm_phase's bits"""
    fmc, a, tt, r = _scatterers(rtus, 2.0)
    env = np.abs(r["image"]).reshape(XS.shape)
    far = _far()
    for key, gain in (("vcf", 5.0), ("scf", 100.0)):
        weighted = env * r[key].reshape(XS.shape)
        for sx, sz, _ in SCAT:
            i0, j0 = _at(sx, sz)
            r_env = env[i0 - 2:i0 + 3, j0 - 2:j0 + 3].max() / np.median(env[far])
            r_w = weighted[i0 - 2:i0 + 3, j0 - 2:j0 + 3].max() / np.median(weighted[far])
            print(f"scatterer ({sx}, {sz}): peak / background median, envelope {r_env:.1f}, envelope x {key} {r_w:.1f}")
            assert r_w >= gain * r_env, (key, r_w, r_env)
    img, vcf = rtus.tfm_analytic(a, FS, tt, coherence="vcf")
    assert _same(img, r["image"]) and _same(vcf, r["vcf"])
    img, cf = rtus.tfm_analytic(a, FS, tt, coherence="cf")
    img2, cf2 = rtus.tfm_analytic(a, FS, tt, coherence=True)
    assert _same(img, img2) and _same(cf, cf2) and _same(img, r["image"])
    views = rtus.tfm_views(fmc, FS, {"L": tt}, "L-L", envelope=True, coherence="scf")
    assert list(views) == ["L-L"]
    env_v, scf_v = views["L-L"]
    assert _same(env_v, np.abs(r["image"])) and _same(scf_v, r["scf"])


def test_pwi_image_takes_the_phase_factors(rtus):
    """8. (last item) a small plane-wave set synthesised from the noisy FMC: pwi_image(coherence="vcf") is tfm_phase over the
    analytic plane-wave data, bit for bit"""
    fmc, _, tt, _ = _scatterers(rtus, 2.0)
    ang = np.deg2rad([-10.0, 0.0, 10.0])
    pw = rtus.fmc_synth_tx(fmc, FS, rtus.pw_delays(XE, ZE, ang, C))
    sel = np.arange(0, XS.size, 7)
    tt_rx = np.ascontiguousarray(tt[:, sel])
    tt_pw = rtus.pw_travel_time_layers([], [C], ang, XE, ZE, XS.ravel()[sel], ZS.ravel()[sel])
    env, vcf = rtus.pwi_image(pw, FS, tt_pw, tt_rx, envelope=True, coherence="vcf")
    want = rtus.tfm_phase(rtus.fmc_analytic(pw), FS, tt_pw, tt_rx)
    assert _same(env, np.abs(want["image"])) and _same(vcf, want["vcf"])
    assert np.isfinite(vcf).any()
    env2, scf = rtus.pwi_image(pw, FS, tt_pw, tt_rx, envelope=True, coherence="scf")
    assert _same(env2, env) and _same(scf, want["scf"])

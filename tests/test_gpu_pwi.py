"""GPU: plane-wave imaging — the plane-wave tables (rtus_pw_layers*, rtus_pw_surface*) against the NumPy oracle
(tests/pwi_numpy.py) and against a Huygens minimum over a dense virtual aperture built with the library's own element solvers, the
synthesis of delay laws from FMC (rtus_fmc_synth_tx*) against its fp32 oracle, determinism under any sharing of the call, the
host / device / captured-graph paths, end-to-end images of a side-drilled hole, and every kernel at production shapes.

Synthesis tolerance: the oracle restates the kernel's fp32 arithmetic term by term (the fmaf through fp64, where w * d is exact),
so the two differ only where that double rounding differs from the fused one: at most one fp32 ulp of a term, accumulated over
n_tx terms: |out - oracle| <= n_tx 2^-23 sum_tx |x| (checked against the oracle of |fmc|)."""
import numpy as np
import pytest

import autofocus_numpy as AF
import pwi_numpy as P
import surface_numpy as S

pytestmark = pytest.mark.gpu

C1, C2 = 1480.0, 5900.0
X0, DX, NS = -0.02, 1e-3, 41
XE = np.linspace(-0.0096, 0.0096, 33)
ZE = np.zeros(XE.size)
X_LO, X_HI, Z_A = float(XE.min()), float(XE.max()), 0.0


def _wavy(amp=0.0015, lam=0.010, z0=0.02):
    x = X0 + DX * np.arange(NS)
    return z0 + amp * np.sin(2 * np.pi * x / lam)


def _dev():
    from importlib import import_module
    return import_module("ray-tracing-ultrasound_amd.device")


# ---------------------------------------------------------------------------------------------- 1. planar layers vs the oracle
@pytest.mark.parametrize("z_if,c", [([0.02], [C1, C2]), ([0.01, 0.025], [C1, 2330.0, C2]),
                                    ([0.008, 0.015, 0.03], [2330.0, C1, 3200.0, C2])])
def test_planar_against_the_oracle(rtus, z_if, c):
    rng = np.random.default_rng(21)
    crit = np.arcsin(c[0] / max(c))
    ang = np.r_[np.linspace(-0.26, 0.26, 15), crit - 1e-3, crit + 1e-3, -crit - 1e-3, np.nan, np.inf, np.pi / 2, -np.pi / 2 - 0.1,
                1.4, -0.0]
    xf = np.r_[rng.uniform(-0.04, 0.04, 5000), 0.0, 0.0, 0.0]
    zf = np.r_[rng.uniform(-0.005, 0.06, 5000), Z_A, Z_A - 1e-3, z_if[0]]                 # some above the array, one on it
    got = rtus.pw_travel_time_layers(z_if, c, ang, XE, ZE, xf, zf)
    ref = P.layers(z_if, c, ang, X_LO, X_HI, Z_A, xf, zf)
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    fin = np.isfinite(ref)
    assert fin.mean() > 0.1
    assert np.max(np.abs(got[fin] - ref[fin]) / ref[fin]) <= 1e-14
    assert np.isnan(got[18:22]).all()                                                   # non-finite angles, |angle| >= pi/2
    assert np.isnan(got[:, -2]).all() and np.isnan(got[:, -3]).all()                     # on / above the array


# ---------------------------------------------------------------------------------------------- 2. Huygens through the element solvers
def _huygens(d, tt):
    """min_e (d_e + tt_e(F)) with a parabolic step, and the discrete argmin -> (t [n_a, n_f], k [n_a, n_f])"""
    tot = d[:, :, None] + tt[None, :, :]                                  # [n_a, n_e, n_f]
    tot = np.where(np.isfinite(tot), tot, np.inf)
    k = np.argmin(tot, axis=1)
    n_e = tot.shape[1]
    kk = np.clip(k, 1, n_e - 2)
    y0, y1, y2 = (np.take_along_axis(tot, (kk + o)[:, None, :], axis=1)[:, 0] for o in (-1, 0, 1))
    den = y0 - 2 * y1 + y2
    with np.errstate(invalid="ignore", divide="ignore"):
        step = np.where((den > 0) & np.isfinite(den), (y0 - y2) ** 2 / (8 * den), 0.0)
    t = np.where((k == kk) & np.isfinite(y1), y1 - step, np.take_along_axis(tot, k[:, None, :], axis=1)[:, 0])
    return t, k


@pytest.mark.parametrize("kind", ["planar", "surface"])
def test_huygens_minimum_through_the_element_solvers(rtus, kind):
    """A plane wave is the envelope of the wavelets of its firing elements: with a dense virtual aperture (4096 points, pitch h) fired
    by pw_delays, min_e (d_e + tt_e(F)) is the plane-wave time.  Discrete minimum: g(x) = d(x) + tt(x, F) is smooth with
    g'' <= 1 / (c1 h0) (h0: the least vertical couplant path under the array, the wavefront from F is no more curved there), so
    the discrete minimum is within g'' h^2 / 8 of the true one, and the parabolic step only improves it; the element tables add
    1e-13 relative.  Tolerance: h^2 / (8 c1 h0) + 1e-13 t.  Planar layers: g is convex, so the bound holds for every entry, no
    virtual element beats the plane wave, and where the table is NaN because of the band the discrete argmin is an aperture end.
    A curved surface can focus the wavelets (g'' above the bound), and an out-of-band minimum of T can reach F earlier through the
    wavelets of an aperture end (an edge arrival, which the plane-wave table does not count by definition): there the comparison is
    made where the discrete argmin is inside the aperture, and 98 % of those entries must be within the tolerance."""
    n_v = 4096
    xv, zv = np.linspace(X_LO, X_HI, n_v), np.zeros(n_v)
    h = (X_HI - X_LO) / (n_v - 1)
    ang = np.array([-0.2, -0.07, 0.0, 0.05, 0.2])
    rng = np.random.default_rng(31)
    xf, zf = rng.uniform(-0.02, 0.02, 150), rng.uniform(0.026, 0.05, 150)
    d = rtus.pw_delays(xv, zv, ang, C1)
    if kind == "planar":
        pw = rtus.pw_travel_time_layers([0.02], [C1, C2], ang, xv, zv, xf, zf)
        tt = rtus.travel_time_layers([0.02], [C1, C2], xv, zv, xf, zf)
        h0 = 0.02
    else:
        zs = _wavy()
        pw = rtus.pw_travel_time_surface(X0, DX, zs, C1, C2, ang, xv, zv, xf, zf)
        tt = rtus.travel_time_surface(X0, DX, zs, C1, C2, xv, zv, xf, zf)
        h0 = float(zs.min())
    hy, k = _huygens(d, tt)
    tol = h * h / (8 * C1 * h0)
    fin = np.isfinite(pw)
    assert fin.mean() > 0.3
    if kind == "surface":
        fin &= (k > 0) & (k < n_v - 1)
        assert fin.mean() > 0.2
    err = hy[fin] - pw[fin]
    close = np.abs(err) <= tol + 1e-13 * pw[fin]
    print(f"{kind}: {fin.sum()} entries, within tolerance {close.mean():.4f}, worst |err| {np.max(np.abs(err)):.2e} s, tol {tol:.2e} s")
    assert close.mean() >= (1.0 if kind == "planar" else 0.98), float(close.mean())
    band_nan = ~fin & np.isfinite(hy)
    if kind == "planar":                                          # (here the only NaN rule that applies is the band)
        assert np.all(err >= -(tol + 1e-13 * pw[fin])), float(err.min())
        assert band_nan.sum() > 20
        assert np.all((k[band_nan] == 0) | (k[band_nan] == n_v - 1))


# ---------------------------------------------------------------------------------------------- 3. curved surface vs the oracle
def test_flat_surface_equals_pw_layers(rtus):
    rng = np.random.default_rng(41)
    ang = np.linspace(-0.22, 0.22, 9)
    xf, zf = rng.uniform(-0.018, 0.018, 2000), rng.uniform(0.021, 0.06, 2000)
    got = rtus.pw_travel_time_surface(X0, DX, np.full(NS, 0.02), C1, C2, ang, XE, ZE, xf, zf)
    ref = rtus.pw_travel_time_layers([0.02], [C1, C2], ang, XE, ZE, xf, zf)
    o = P.surface(X0, DX, np.full(NS, 0.02), C1, C2, ang, X_LO, X_HI, Z_A, xf, zf)
    ok = o["basin"] >= DX                                         # off the band edges (the guarantee's margin)
    assert ok.mean() > 0.95
    assert np.array_equal(np.isnan(got[ok]), np.isnan(o["t"][ok]))
    fin = ok & np.isfinite(o["t"])                                # (the oracle also drops entry points outside the extent)
    assert np.isfinite(ref[fin]).all()
    assert fin.sum() > 5000
    assert np.max(np.abs(got[fin] - ref[fin]) / ref[fin]) <= 1e-13


@pytest.mark.parametrize("amp,lam,seed", [(0.0015, 0.010, 51), (0.0008, 0.0065, 52)])
def test_wavy_surface_against_the_oracle_and_snell(rtus, amp, lam, seed):
    zs = _wavy(amp, lam)
    rng = np.random.default_rng(seed)
    ang = np.r_[np.linspace(-0.25, 0.25, 7), np.nan, np.pi / 2]
    xf, zf = rng.uniform(-0.022, 0.022, 1500), rng.uniform(0.012, 0.045, 1500)
    tt, xn = rtus.pw_travel_time_surface(X0, DX, zs, C1, C2, ang, XE, ZE, xf, zf, return_entry=True)
    o = P.surface(X0, DX, zs, C1, C2, ang, X_LO, X_HI, Z_A, xf, zf)
    flagged = o["basin"] < DX
    print(f"flagged: {flagged.mean():.2e}, finite {np.isfinite(o['t']).mean():.3f}")
    assert flagged.mean() <= 0.05                                 # (near band edges and neighbouring stationary points)
    ok = ~flagged
    assert np.array_equal(np.isnan(tt[ok]), np.isnan(o["t"][ok]))
    fin = ok & np.isfinite(o["t"])
    assert fin.sum() > 2000
    assert np.max(np.abs(tt[fin] - o["t"][fin]) / o["t"][fin]) <= 1e-13
    g = np.isfinite(tt)
    gg = g & np.isfinite(o["t"])
    assert np.all(tt[gg] >= o["t"][gg] * (1 - 1e-13))            # a missed minimum may only make an entry later
    assert np.isnan(tt[-2:]).all()
    # Snell at x_entry: the tangential slowness is continuous, u . T / c1 = v . T / c2 (T the unit tangent, v towards F)
    coef = S.spline(X0, DX, zs)
    a_i, f_i = np.nonzero(g)
    x = xn[a_i, f_i]
    s, s1, _ = S.spline_eval(coef, X0, DX, x)
    tl = np.hypot(1.0, s1)
    ut = (np.sin(ang[a_i]) + s1 * np.cos(ang[a_i])) / tl
    vx, vz = xf[f_i] - x, zf[f_i] - s
    vt = (vx + vz * s1) / (np.hypot(vx, vz) * tl)
    assert np.max(np.abs(ut / C1 - vt / C2)) * C1 <= 1e-9
    # insonified: the entry point traced back along u lands on the aperture
    xb = x - (s - Z_A) * np.tan(ang[a_i])
    assert np.all((xb >= X_LO) & (xb <= X_HI))


def test_surface_bits_under_subsets_shuffles_and_paths(rtus):
    import torch
    dev = _dev()
    zs = _wavy()
    rng = np.random.default_rng(61)
    ang = np.linspace(-0.25, 0.25, 13)
    xf, zf = rng.uniform(-0.022, 0.022, 3000), rng.uniform(0.012, 0.045, 3000)
    tt, xn = rtus.pw_travel_time_surface(X0, DX, zs, C1, C2, ang, XE, ZE, xf, zf, return_entry=True)
    pa, pf = rng.permutation(ang.size), rng.permutation(xf.size)
    t2 = rtus.pw_travel_time_surface(X0, DX, zs, C1, C2, ang[pa], XE, ZE, xf[pf], zf[pf])
    assert np.array_equal(t2, tt[pa][:, pf], equal_nan=True)
    for sub in ([5], [12, 0, 3], list(range(3, 11))):
        t3 = rtus.pw_travel_time_surface(X0, DX, zs, C1, C2, ang[sub], XE, ZE, xf[100:357], zf[100:357])
        assert np.array_equal(t3, tt[sub][:, 100:357], equal_nan=True)
    # planar table: the same under subsets and shuffles
    pl = rtus.pw_travel_time_layers([0.02], [C1, C2], ang, XE, ZE, xf, zf)
    assert np.array_equal(rtus.pw_travel_time_layers([0.02], [C1, C2], ang[pa], XE, ZE, xf[pf], zf[pf]), pl[pa][:, pf], equal_nan=True)
    # device and captured-graph paths
    f64 = dict(dtype=torch.float64, device="cuda")
    dzs, dang, dxf, dzf = (torch.as_tensor(v, **f64) for v in (zs, ang, xf, zf))
    out = torch.empty((ang.size, xf.size), **f64)
    xe_out = torch.empty_like(out)
    lay = torch.empty_like(out)

    def run():
        dev.pw_surface_dev(X0, DX, dzs, C1, C2, dang, X_LO, X_HI, Z_A, dxf, dzf, out=out, x_entry=xe_out)
        dev.pw_layers_dev([0.02], [C1, C2], dang, X_LO, X_HI, Z_A, dxf, dzf, out=lay)
    run()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), tt, equal_nan=True) and np.array_equal(xe_out.cpu().numpy(), xn, equal_nan=True)
    assert np.array_equal(lay.cpu().numpy(), pl, equal_nan=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    out.fill_(0.0); xe_out.fill_(0.0); lay.fill_(0.0)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), tt, equal_nan=True) and np.array_equal(xe_out.cpu().numpy(), xn, equal_nan=True)
    assert np.array_equal(lay.cpu().numpy(), pl, equal_nan=True)
    # the whole table is NaN when the profile is not strictly below the array
    hi = rtus.pw_travel_time_surface(X0, DX, zs, C1, C2, ang, XE, np.full(XE.size, float(zs.min())), xf, zf)
    assert np.isnan(hi).all()


# ---------------------------------------------------------------------------------------------- 4. synthesis vs the oracle
def _synth_case(seed, n_tx=24, n_rx=5, n_t=300, n_v=11):
    rng = np.random.default_rng(seed)
    fs = 40e6
    fmc = rng.standard_normal((n_tx, n_rx, n_t)).astype(np.float32)
    d = rng.uniform(-1.2 * n_t, 1.2 * n_t, (n_v, n_tx)) / fs                         # past both ends of the record
    d[0] = 0.0
    d[1] = np.round(d[1] * fs) / fs                                                  # whole samples
    d[2, ::3] = np.nan
    d[3, 1::4] = np.inf
    d[4, ::5] = 2e8 / fs                                                             # absurd
    d[5] = rng.uniform(-3, 3, n_tx) / fs                                             # around both record edges
    return fmc, fs, d


def test_synthesis_against_the_oracle(rtus):
    fmc, fs, d = _synth_case(71)
    got = rtus.fmc_synth_tx(fmc, fs, d)
    ref = P.synth(fmc, fs, d)
    bound = P.synth(np.abs(fmc), fs, d).astype(np.float64) * fmc.shape[0] * 2.0 ** -23 + 1e-30
    assert np.all(np.abs(got.astype(np.float64) - ref) <= bound)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    # skipped tx: the laws with NaN / inf / absurd delays equal the oracle without those tx
    for v, keep in ((2, np.isfinite(d[2])), (3, np.isfinite(d[3])), (4, np.abs(d[4] * fs) < 1e8)):
        assert np.allclose(got[v], P.synth(fmc[keep], fs, d[v:v + 1, keep])[0], rtol=0, atol=1e-4)
    # both record edges carry signal and nothing leaks past them
    assert np.any(got[5][:, 0] != 0) and np.any(got[5][:, -1] != 0)
    far = np.full((1, fmc.shape[0]), 2.0 * fmc.shape[2] / fs)
    assert not np.any(rtus.fmc_synth_tx(fmc, fs, far))
    assert not np.any(rtus.fmc_synth_tx(fmc, fs, -far))


def test_synthesis_bits_under_subsets_and_paths(rtus):
    import torch
    dev = _dev()
    fmc, fs, d = _synth_case(72, n_v=19)
    full = rtus.fmc_synth_tx(fmc, fs, d)
    for sub in ([7], [18, 2, 9], list(range(4, 17))):
        assert np.array_equal(rtus.fmc_synth_tx(fmc, fs, d[sub]), full[sub])
    dfmc, dd = torch.as_tensor(fmc, device="cuda"), torch.as_tensor(d, device="cuda")
    out = torch.empty(full.shape, dtype=torch.float32, device="cuda")
    assert dev.fmc_synth_tx_dev(dfmc, fs, dd, out=out) is out
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), full)
    with pytest.raises(ValueError):
        dev.fmc_synth_tx_dev(dfmc, fs, dd[:, :5].contiguous())
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        dev.fmc_synth_tx_dev(dfmc, fs, dd, out=out)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        dev.fmc_synth_tx_dev(dfmc, fs, dd, out=out)
    out.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), full)


# ---------------------------------------------------------------------------------------------- 5. end to end: a side-drilled hole
FS, NT, F0 = 50e6, 2600, 5e6
N_EL = 32
XA = (np.arange(N_EL) - (N_EL - 1) / 2) * 0.6e-3
ZA = np.zeros(N_EL)


def _grid(xc, zc, n=41, half=0.004):
    gx, gz = np.meshgrid(np.linspace(xc - half, xc + half, n), np.linspace(zc - half, zc + half, n))
    return gx.ravel(), gz.ravel()


def _peak_xy(img, xf, zf):
    k = int(np.nanargmax(np.abs(img)))
    return xf[k], zf[k]


@pytest.mark.parametrize("geom", ["planar", "wavy"])
def test_end_to_end_side_drilled_hole(rtus, geom):
    hole = (0.003, 0.034)
    if geom == "planar":
        tt_h = rtus.travel_time_layers([0.02], [C1, C2], XA, ZA, [hole[0]], [hole[1]])[:, 0]
        fmc = np.zeros((N_EL, N_EL, NT))
        tx, rx = np.meshgrid(np.arange(N_EL), np.arange(N_EL), indexing="ij")
        tx, rx = tx.ravel(), rx.ravel()
        AF._splat(fmc, tx, rx, tt_h[tx] + tt_h[rx], 1.0, FS, 0.0, F0, 2.5)
        fmc = fmc.astype(np.float32)
    else:
        zs = _wavy()
        fmc = AF.synth_fmc(XA, ZA, C1, FS, NT, X0, DX, zs, -0.015, 0.015, f0=F0, scatterer=(hole[0], hole[1], 1.0), c2=C2)
    xf, zf = _grid(*hole)
    ang = np.deg2rad(np.linspace(-12, 12, 21))
    pw = rtus.fmc_synth_tx(fmc, FS, rtus.pw_delays(XA, ZA, ang, C1))
    if geom == "planar":
        tt_pw = rtus.pw_travel_time_layers([0.02], [C1, C2], ang, XA, ZA, xf, zf)
        tt_rx = rtus.travel_time_layers([0.02], [C1, C2], XA, ZA, xf, zf)
    else:
        tt_pw = rtus.pw_travel_time_surface(X0, DX, zs, C1, C2, ang, XA, ZA, xf, zf)
        tt_rx = rtus.travel_time_surface(X0, DX, zs, C1, C2, XA, ZA, xf, zf)
    rf = rtus.pwi_image(pw, FS, tt_pw, tt_rx)
    env, cf = rtus.pwi_image(pw, FS, tt_pw, tt_rx, envelope=True, coherence=True)
    assert rf.dtype == np.float32 and env.shape == rf.shape == cf.shape
    step = 0.008 / 40
    for img in (rf, env, env * np.nan_to_num(cf)):
        px, pz = _peak_xy(img, xf, zf)
        assert abs(px - hole[0]) <= step * 1.01 and abs(pz - hole[1]) <= step * 1.01, (px, pz)
    # the envelope PWI and the envelope TFM of the same FMC agree on the peak within one pixel
    tfm = np.abs(rtus.tfm_analytic(rtus.fmc_analytic(fmc), FS, tt_rx))
    tx_, tz_ = _peak_xy(tfm, xf, zf)
    px, pz = _peak_xy(env, xf, zf)
    assert abs(px - tx_) <= step * 1.01 and abs(pz - tz_) <= step * 1.01


# ---------------------------------------------------------------------------------------------- 6. production shapes
def test_production_shapes(rtus):
    import torch
    dev = _dev()
    f64 = dict(dtype=torch.float64, device="cuda")
    n_e, n_t, n_a = 64, 2048, 31
    xe = (np.arange(n_e) - (n_e - 1) / 2) * 0.6e-3
    ze = np.zeros(n_e)
    ang = np.deg2rad(np.linspace(-15, 15, n_a))
    rng = np.random.default_rng(81)
    # synthesis: 31 laws x 64 x 64 x 2048
    fmc = rng.standard_normal((n_e, n_e, n_t)).astype(np.float32)
    d = rtus.pw_delays(xe, ze, ang, C1)
    dfmc, dd = torch.as_tensor(fmc, device="cuda"), torch.as_tensor(d, device="cuda")
    pw = dev.fmc_synth_tx_dev(dfmc, FS, dd)
    torch.cuda.synchronize()
    pw_h = pw.cpu().numpy()
    for v in (0, 15, 30):
        ref = P.synth(fmc, FS, d[v:v + 1])[0]
        bound = P.synth(np.abs(fmc), FS, d[v:v + 1])[0].astype(np.float64) * n_e * 2.0 ** -23 + 1e-30
        assert np.all(np.abs(pw_h[v] - ref) <= bound)
    for n in (256, 1024):
        gx, gz = torch.meshgrid(torch.linspace(-0.03, 0.03, n, **f64), torch.linspace(0.025, 0.065, n, **f64), indexing="xy")
        xf, zf = gx.reshape(-1).contiguous(), gz.reshape(-1).contiguous()
        dang = torch.as_tensor(ang, **f64)
        tt_pw = dev.pw_layers_dev([0.02], [C1, C2], dang, xe.min(), xe.max(), 0.0, xf, zf)
        tt_rx = dev.tt_layers_dev([0.02], [C1, C2], torch.as_tensor(xe, **f64), torch.as_tensor(ze, **f64), xf, zf)
        img = dev.tfm_dev(pw, FS, tt_pw, tt_rx)
        torch.cuda.synchronize()
        xfh, zfh = xf.cpu().numpy(), zf.cpu().numpy()
        sel = rng.choice(xfh.size, 20000, replace=False)
        got = tt_pw.cpu().numpy()[:, sel]
        ref = P.layers([0.02], [C1, C2], ang, xe.min(), xe.max(), 0.0, xfh[sel], zfh[sel])
        assert np.array_equal(np.isnan(got), np.isnan(ref))
        fin = np.isfinite(ref)
        assert fin.mean() > 0.2 and np.max(np.abs(got[fin] - ref[fin]) / ref[fin]) <= 1e-14
        assert torch.isfinite(img).all()
        if n == 256:
            zs = 0.02 + 0.0015 * torch.sin(2 * torch.pi * (-0.032 + 0.064 / 255 * torch.arange(256, **f64)) / 0.010)
            ts = dev.pw_surface_dev(-0.032, 0.064 / 255, zs, C1, C2, dang, xe.min(), xe.max(), 0.0, xf, zf)
            torch.cuda.synchronize()
            sub = rng.choice(xfh.size, 400, replace=False)
            a_sub = [0, 15, 30]
            o = P.surface(-0.032, 0.064 / 255, zs.cpu().numpy(), C1, C2, ang[a_sub], xe.min(), xe.max(), 0.0, xfh[sub], zfh[sub])
            g = ts.cpu().numpy()[a_sub][:, sub]
            ok = o["basin"] >= 0.064 / 255
            assert np.array_equal(np.isnan(g[ok]), np.isnan(o["t"][ok]))
            fin = ok & np.isfinite(o["t"])
            assert fin.sum() > 300 and np.max(np.abs(g[fin] - o["t"][fin]) / o["t"][fin]) <= 1e-13

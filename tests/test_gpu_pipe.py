"""GPU: lens-to-pipe-wall travel times (rtus_tt_pipe*) against the NumPy oracle (tests/pipe_numpy.py) at the corners of the
reference's sweep; the lens-only limit against rtus_tt_lens; Snell's law from the returned path; bore occlusion; bits under subsets,
shuffles, the host, device and graph-captured paths; an end-to-end wall image; the production shape."""
import time
from importlib import import_module

import numpy as np
import pytest

import pipe_numpy as O

pytestmark = pytest.mark.gpu

XE64 = (np.arange(64) - 31.5) * 0.6e-3                      # the reference aperture (main_rt.py:469-474, without the virtual centre)
ZE64 = np.full(64, O.D)
LENS = O.Lens()
CORNERS = [(r, off) for r in (0.01, 0.037, 0.06) for off in (-0.01, 0.0038, 0.01)]
# the share of an input set that the oracle may flag (entries _compare excuses for being late): tests/test_gpu_skip.py's.  The
# oracle flags nothing on the nine sweep-corner grids and on the production shape's 2000 sampled pairs.
FLAG_CAP = 2e-3


def _params(rtus, r_outer, off):
    return rtus.Params(r_outer=r_outer, pipe_offset=off)


def _compare(tt, o, label):
    """|dt| <= 1e-17 + 1e-13 t; NaN masks equal except flagged entries, which may only be later"""
    ref, flag = o["t"], o["flag"]
    both = np.isfinite(tt) & np.isfinite(ref)
    err = np.abs(tt[both] - ref[both])
    ok = err <= 1e-17 + 1e-13 * ref[both]
    late = (tt[both] > ref[both]) & flag[both]
    assert np.all(ok | late), (label, float(np.max(err / ref[both])))
    mism = np.isnan(tt) != np.isnan(ref)
    assert not np.any(mism & ~flag), (label, int(np.sum(mism & ~flag)))
    assert not np.any(np.isfinite(tt) & np.isnan(ref)), label              # flagged entries may be missed, never invented
    return both


def _t2(lens, pipe, xe, ze, xf, zf, beta):
    """T''(beta) of the oracle's problem by a central difference of T'"""
    h = 1e-6
    d_p = O._dT(lens, pipe, xe, ze, xf, zf, beta + h, -O.ALPHA_MAX, O.ALPHA_MAX)[0]
    d_m = O._dT(lens, pipe, xe, ze, xf, zf, beta - h, -O.ALPHA_MAX, O.ALPHA_MAX)[0]
    return (d_p - d_m) / (2 * h)


@pytest.mark.parametrize("r_outer,off", CORNERS)
def test_against_the_oracle_at_the_sweep_corners(rtus, r_outer, off):
    ri = 0.6 * r_outer
    p = _params(rtus, r_outer, off)
    xe, ze = XE64[::9], ZE64[::9]
    xf, zf = rtus.pipe_wall_grid(ri + 1e-4, r_outer - 1e-4, 5, 21, -0.45, 0.45, params=p)
    xf, zf = np.r_[xf, off, off, off + 2 * r_outer], np.r_[zf, 0.5 * ri, r_outer + 1e-3, 0.0]      # bore, water, far outside
    tt, al, be = rtus.travel_time_pipe(xe, ze, xf, zf, r_inner=ri, params=p, return_path=True)
    pipe = O.Pipe(r_outer, off, ri)
    o = O.table(LENS, pipe, xe, ze, xf, zf)
    assert o["flag"].mean() <= FLAG_CAP
    both = _compare(tt, o, (r_outer, off))
    assert np.isnan(tt[:, -3:]).all()
    assert both.mean() > 0.5
    ie, jf = np.nonzero(both)
    t2 = _t2(LENS, pipe, xe[ie], ze[ie], xf[jf], zf[jf], o["beta"][both])
    firm = t2 > 1e-3 * np.median(np.abs(t2))
    assert np.max(np.abs(be[both] - o["beta"][both])[firm]) <= 1e-9
    free = firm & (np.abs(o["alpha"][both]) < O.ALPHA_MAX)
    assert np.max(np.abs(al[both] - o["alpha"][both])[free], initial=0.0) <= 1e-9
    pinned = np.abs(o["alpha"][both]) == O.ALPHA_MAX
    assert np.array_equal(al[both][pinned], o["alpha"][both][pinned])


def test_equal_speeds_is_the_lens_table(rtus):
    """c3 = c2, a solid bar: the entries are rtus_tt_lens's least times to the points"""
    p = _params(rtus, 0.037, 0.0038)
    rng = np.random.default_rng(11)
    rr, th = rng.uniform(0.002, 0.0365, 700), rng.uniform(-0.6, 0.6, 700)
    xf, zf = 0.0038 + rr * np.sin(th), rr * np.cos(th)
    xe, ze = XE64[::3], ZE64[::3]
    tt = rtus.travel_time_pipe(xe, ze, xf, zf, c3=p.c2, r_inner=0.0, params=p)
    ref = rtus.travel_time_lens(xe, ze, xf, zf, params=p)
    assert np.isfinite(tt).all()
    assert np.all(np.abs(tt - ref) <= 1e-17 + 1e-13 * ref), float(np.max(np.abs(tt - ref) / ref))


@pytest.mark.parametrize("r_outer,off", [(0.037, 0.0038), (0.06, -0.01)])
def test_paths_obey_snell(rtus, r_outer, off):
    p = _params(rtus, r_outer, off)
    xf, zf = rtus.pipe_wall_grid(0.5 * r_outer, r_outer - 1e-4, 6, 31, -0.5, 0.5, params=p)
    tt, al, be = rtus.travel_time_pipe(XE64[::4], ZE64[::4], xf, zf, r_inner=0.45 * r_outer, params=p, return_path=True)
    g = np.isfinite(tt)
    assert g.mean() > 0.5
    ie, jf = np.nonzero(g)
    r1, r2 = O.snell_residuals(LENS, O.Pipe(r_outer, off, 0.0), XE64[::4][ie], ZE64[::4][ie], xf[jf], zf[jf], al[g], be[g])
    free = np.abs(al[g]) < O.ALPHA_MAX
    assert np.max(np.abs(r1[free]), initial=0.0) <= 1e-9 and np.max(np.abs(r2)) <= 1e-9


def test_bore_occlusion(rtus):
    """points just above the bore of a pipe 10 mm off the lens axis: NaN exactly where the oracle's paths cross the bore"""
    th = np.radians(np.linspace(-85, 85, 35))
    xf, zf = 0.01 + 0.0301 * np.sin(th), 0.0301 * np.cos(th)
    p = _params(rtus, 0.037, 0.01)
    xe, ze = XE64[::8], ZE64[::8]
    solid = rtus.travel_time_pipe(xe, ze, xf, zf, r_inner=0.0, params=p)
    bore = rtus.travel_time_pipe(xe, ze, xf, zf, r_inner=0.0296, params=p)
    o = O.table(LENS, O.Pipe(0.037, 0.01, 0.0296), xe, ze, xf, zf)
    _compare(bore, o, "bore")
    assert (np.isfinite(solid) & np.isnan(bore)).sum() >= 10


def test_bits_under_subsets_shuffles_and_launch_paths(rtus):
    import torch
    dev = import_module("ray-tracing-ultrasound_amd.device")
    p = _params(rtus, 0.037, 0.0038)
    xf, zf = rtus.pipe_wall_grid(0.0292, 0.0368, 20, 40, -0.5, 0.5, params=p)
    kw = dict(r_inner=0.029, params=p)
    full, fa, fb = rtus.travel_time_pipe(XE64, ZE64, xf, zf, return_path=True, **kw)
    assert np.isfinite(full).mean() > 0.9
    rows = np.array([63, 5, 6, 40, 0, 17, 18, 19, 33])
    cols = np.random.default_rng(2).permutation(xf.size)[:301]
    sub, sa, sb = rtus.travel_time_pipe(XE64[rows], ZE64[rows], xf[cols], zf[cols], return_path=True, **kw)
    assert np.array_equal(sub, full[np.ix_(rows, cols)], equal_nan=True)
    assert np.array_equal(sa, fa[np.ix_(rows, cols)], equal_nan=True) and np.array_equal(sb, fb[np.ix_(rows, cols)], equal_nan=True)
    for _ in range(2):
        assert np.array_equal(rtus.travel_time_pipe(XE64, ZE64, xf, zf, **kw), full, equal_nan=True)
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")      # noqa: E731
    dxe, dze, dxf, dzf = t(XE64), t(ZE64), t(xf), t(zf)
    out = torch.empty((64, xf.size), dtype=torch.float64, device="cuda")
    oa, ob = torch.empty_like(out), torch.empty_like(out)
    n_scan = O.default_n_scan(0.037)
    ws = torch.empty(int(rtus.lib().rtus_tt_pipe_workspace_bytes(64, n_scan)), dtype=torch.uint8, device="cuda")

    def run():
        dev.tt_pipe_dev(dxe, dze, dxf, dzf, out=out, alpha_out=oa, beta_out=ob, ws=ws, **kw)
    run()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), full, equal_nan=True)
    assert np.array_equal(oa.cpu().numpy(), fa, equal_nan=True) and np.array_equal(ob.cpu().numpy(), fb, equal_nan=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run()
    out.fill_(0.0); oa.fill_(0.0); ob.fill_(0.0)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), full, equal_nan=True)
    assert np.array_equal(oa.cpu().numpy(), fa, equal_nan=True) and np.array_equal(ob.cpu().numpy(), fb, equal_nan=True)


def _fmc(tx_t, rx_t, fs, t0, n_t, f0=5e6):
    """FMC of point scatterers from per-element times ([n_s, n_e] each): a 5 MHz Gaussian tone burst at tx_t + rx_t"""
    tax = t0 + np.arange(n_t) / fs
    a = np.zeros((tx_t.shape[1], rx_t.shape[1], n_t))
    for s in range(tx_t.shape[0]):
        u = tax[None, None, :] - (tx_t[s][:, None, None] + rx_t[s][None, :, None])
        a += np.cos(2 * np.pi * f0 * u) * np.exp(-(u * f0 / 1.2) ** 2)
    return a.astype(np.float32)


def test_wall_image_end_to_end(rtus):
    """two scatterers in the 8 mm wall (r_outer 37 mm, bore 29 mm, 3.8 mm off axis), 4 mm and 7 mm under the outer surface: the
    wall tables image them where they are; tables that take the wall for water do not"""
    p = _params(rtus, 0.037, 0.0038)
    ri, ro = 0.029, 0.037
    sr, sth = np.array([ro - 0.004, ro - 0.007]), np.radians([-4.0, 5.0])
    sx, sz = 0.0038 + sr * np.sin(sth), sr * np.cos(sth)
    o = O.table(LENS, O.Pipe(ro, 0.0038, ri), XE64, ZE64, sx, sz)
    assert np.isfinite(o["t"]).all()
    fs, t0, n_t = 50e6, 0.9e-4, 2000
    fmc = _fmc(o["t"].T, o["t"].T, fs, t0, n_t)
    n_r, n_th, th_lo, th_hi = 33, 61, np.radians(-12.0), np.radians(12.0)
    xf, zf = rtus.pipe_wall_grid(ri + 2e-4, ro - 2e-4, n_r, n_th, th_lo, th_hi, params=p)
    an = rtus.fmc_analytic(fmc)
    tt = rtus.travel_time_pipe(XE64, ZE64, xf, zf, r_inner=ri, params=p)
    img = np.abs(rtus.tfm_analytic(an, fs, tt, t0=t0)).reshape(n_r, n_th)
    rr = np.linspace(ri + 2e-4, ro - 2e-4, n_r)
    thh = np.linspace(th_lo, th_hi, n_th)
    for k in range(2):
        i0, j0 = np.argmin(np.abs(rr - sr[k])), np.argmin(np.abs(thh - sth[k]))
        win = np.zeros_like(img, dtype=bool)                     # the scatterer's neighbourhood: 1.5 mm
        pr = np.hypot(xf - sx[k], zf - sz[k]).reshape(n_r, n_th)
        win[pr <= 1.5e-3] = True
        i, j = np.unravel_index(np.argmax(np.where(win, img, -1.0)), img.shape)
        assert abs(i - i0) <= 1 and abs(j - j0) <= 1, (k, i, j, i0, j0)
    water = rtus.travel_time_lens(XE64, ZE64, xf, zf, params=p)
    iw = np.abs(rtus.tfm_analytic(an, fs, water, t0=t0))
    b = np.nanargmax(iw)
    assert np.min(np.hypot(xf[b] - sx, zf[b] - sz)) >= 2e-3


def test_production_shape(rtus):
    """the reference aperture, r_outer 37 mm, offset 3.8 mm, bore 29 mm, 128 radii x 256 angles over +-30 deg"""
    import torch
    dev = import_module("ray-tracing-ultrasound_amd.device")
    p = _params(rtus, 0.037, 0.0038)
    xf, zf = rtus.pipe_wall_grid(0.029 + 3e-5, 0.037 - 3e-5, 128, 256, -np.pi / 6, np.pi / 6, params=p)
    tt, al, be = rtus.travel_time_pipe(XE64, ZE64, xf, zf, r_inner=0.029, params=p, return_path=True)
    rng = np.random.default_rng(7)
    ie, jf = rng.integers(0, 64, 2000), rng.integers(0, xf.size, 2000)
    o = O.table(LENS, O.Pipe(0.037, 0.0038, 0.029), XE64, ZE64, xf, zf, pairs=(ie, jf))
    assert o["flag"].mean() <= FLAG_CAP
    _compare(tt[ie, jf], o, "production")
    assert np.isfinite(tt).mean() > 0.9
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")      # noqa: E731
    dxe, dze, dxf, dzf = t(XE64), t(ZE64), t(xf), t(zf)
    out = torch.empty((64, xf.size), dtype=torch.float64, device="cuda")
    dev.tt_pipe_dev(dxe, dze, dxf, dzf, out=out, r_inner=0.029, params=p)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), tt, equal_nan=True)
    reps = 5
    t0 = time.perf_counter()
    for _ in range(reps):
        dev.tt_pipe_dev(dxe, dze, dxf, dzf, out=out, r_inner=0.029, params=p)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / reps * 1e3
    print(f"\nrtus_tt_pipe_dev 64 x {xf.size}: {ms:.3f} ms per call (wall, incl. workspace allocation), "
          f"{64 * xf.size / ms * 1e-3:.3g} M solves/s")

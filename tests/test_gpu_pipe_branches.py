"""GPU: rtus_tt_pipe's decision points against the NumPy oracle (tests/pipe_numpy.py) — entries whose earliest minima are rejected
(the second and the third bracket), the general trigonometry instantiation, brackets in the first and the last scan cell and across
the scan's LDS tiles, non-finite and on-the-boundary inputs, launch shapes around the block sizes, and the whole-interval fallback
of the inner solve.  Every input set's conditions (how many entries land on the branch, how many the oracle flags) are computed by
the oracle and asserted before anything is compared."""
from functools import lru_cache
from importlib import import_module

import numpy as np
import pytest

import pipe_numpy as O
from test_gpu_pipe import LENS, XE64, ZE64, _compare, _params

pytestmark = pytest.mark.gpu

XE8, ZE8 = XE64[::9], ZE64[::9]
FLAG_CAP = 0.05             # tests/test_gpu_pwi.py's; the sets' own shares: GEOMS
GP_MIN = 0.125 * O.H0 / O.C2                                # the kernel's "suspect inner minimum" threshold on g' (rtus_lens_fermat.hip)

# thin walls and off-axis pipes: several minima of T(beta) per entry, the earliest often through the bore.  r_outer, offset, bore,
# angles over +-1.5 rad (6 radii from r_inner + 0.1 mm to r_outer - 0.1 mm, the 8 elements XE64[::9]); the oracle's figures:
#            entries   flagged   unflagged winner = 2nd / 3rd minimum   alpha pinned at an end   interior with g' < GP_MIN
#   thin10     11568    2.72 %                        1030 / 7                          5213                         774
#   wall10      2928    0.96 %                         129 / 0                          1719                          96
#   off37p      2928    0                              382 / 0                          1240                           0
#   off37m      2928    0                              382 / 0                          1240                           0
GEOMS = {"thin10": (0.01, 0.0038, 0.0095, 241), "wall10": (0.01, 0.0038, 0.008, 61), "off37p": (0.037, 0.01, 0.0296, 61),
         "off37m": (0.037, -0.01, 0.0296, 61)}


def _wall_grid(off, ri, ro, n_r, n_th, th_lo=-1.5, th_hi=1.5, margin=1e-4):
    rr, th = np.meshgrid(np.linspace(ri + margin, ro - margin, n_r), np.linspace(th_lo, th_hi, n_th), indexing="ij")
    return (off + rr * np.sin(th)).ravel(), (rr * np.cos(th)).ravel()


@lru_cache(maxsize=None)
def _geom(name):
    ro, off, ri, n_th = GEOMS[name]
    xf, zf = _wall_grid(off, ri, ro, 6, n_th)
    pipe = O.Pipe(ro, off, ri)
    return ro, off, ri, xf, zf, pipe, O.table(LENS, pipe, XE8, ZE8, xf, zf, detail=True)


def _t2(pipe, xe, ze, xf, zf, beta, a_lo=-O.ALPHA_MAX, a_hi=O.ALPHA_MAX):
    """T''(beta) of the oracle's problem by a central difference of T'"""
    h = 1e-6
    return (O._dT(LENS, pipe, xe, ze, xf, zf, beta + h, a_lo, a_hi)[0] - O._dT(LENS, pipe, xe, ze, xf, zf, beta - h, a_lo, a_hi)[0]) / (2 * h)


def _check_path(al, be, o, sel, pipe, xe, ze, xf, zf, a_lo=-O.ALPHA_MAX, a_hi=O.ALPHA_MAX):
    """test_gpu_pipe's rule on the entries sel: beta, and alpha off the interval's ends, within 1e-9 rad where T'' is firm; alpha
    pinned at an end bit-equal"""
    ie, jf = np.nonzero(sel)
    t2 = _t2(pipe, xe[ie], ze[ie], xf[jf], zf[jf], o["beta"][sel], a_lo, a_hi)
    firm = t2 > 1e-3 * np.median(np.abs(t2))
    db, da = np.abs(be[sel] - o["beta"][sel]), np.abs(al[sel] - o["alpha"][sel])
    free = firm & (o["alpha"][sel] > a_lo) & (o["alpha"][sel] < a_hi)
    print(f"  path: {int(firm.sum())} firm of {int(sel.sum())}, max |dbeta| {np.max(db[firm], initial=0.0):.2e}, "
          f"max |dalpha| (free) {np.max(da[free], initial=0.0):.2e}")
    assert np.max(db[firm], initial=0.0) <= 1e-9
    assert np.max(da[free], initial=0.0) <= 1e-9
    pinned = (o["alpha"][sel] == a_lo) | (o["alpha"][sel] == a_hi)
    assert np.array_equal(al[sel][pinned], o["alpha"][sel][pinned])


@pytest.mark.parametrize("name", list(GEOMS))
def test_second_and_third_minima(rtus, name):
    """Entries whose earliest minimum (or two) is refined and rejected by a rule: the winner is the second or the third bracket.
    The third minimum of thin10's rank-2 entries is 0.5 % later than the first one; a kernel that skips the third bracket by its
    fp32 distance from the first one alone stores NaN in all 7 (the kernel did, before this test).  Measured on MI355X: every
    unflagged entry within tolerance, |dalpha|, |dbeta| <= 7e-14 rad; the 272 (thin10) and 20 (wall10) entries later than the oracle
    are all flagged ones.  Rule 1 rejects no minimum in any of the sets (rule 2: 709-4612), so its rejection is not exercised.
    Fails with only bracket 0 refined (all sets), only brackets 0-1 refined (thin10), rule 2 dropped (all sets)."""
    ro, off, ri, xf, zf, pipe, o = _geom(name)
    unfl = ~o["flag"]
    n1, n2, share = int(((o["rank"] == 1) & unfl).sum()), int(((o["rank"] == 2) & unfl).sum()), float(o["flag"].mean())
    print(f"\n{name}: unflagged rank 1 / 2: {n1} / {n2}, most minima {int(o['n_min'].max())}, flagged {share:.4f}, rejected by "
          f"rule 1 / 2: {int(o['rej1'].sum())} / {int(o['rej2'].sum())}")
    assert n1 >= 100 and share <= FLAG_CAP
    assert n2 >= 5 or name != "thin10"
    assert o["n_min"].max() <= 3                                # PIPE_K = 3 brackets are kept
    tt, al, be = rtus.travel_time_pipe(XE8, ZE8, xf, zf, r_inner=ri, params=_params(rtus, ro, off), return_path=True)
    late = np.isfinite(o["t"]) & ~(np.abs(tt - o["t"]) <= 1e-17 + 1e-13 * o["t"])
    print(f"  entries off the oracle: {int(late.sum())} ({int((late & unfl).sum())} unflagged), of rank >= 1: "
          f"{int((late & (o['rank'] >= 1)).sum())}, of rank 2: {int((late & (o['rank'] == 2)).sum())}")
    _compare(tt, o, name)
    sel = unfl & (o["rank"] >= 1)
    assert np.isfinite(tt[sel]).all(), int(np.isnan(tt[sel]).sum())
    assert np.all(np.abs(tt[sel] - o["t"][sel]) <= 1e-17 + 1e-13 * o["t"][sel])
    _check_path(al, be, o, unfl & np.isfinite(o["t"]), pipe, XE8, ZE8, xf, zf)


@pytest.mark.parametrize("name", list(GEOMS))
def test_inner_fallback(rtus, name):
    """pipe_T's whole-interval fallback at the winning beta: the lens leg's least time pinned at an end of the alpha interval
    (alpha comes back bit-equal to the end), and interior but flat (g' below the kernel's threshold; the oracle finds such entries
    in the 10 mm geometries only: GEOMS).  The entries are on the branch and their values are checked, but the fallback itself
    is NOT pinned: with it disabled the kernel returns the same values on all four sets (the warm-started Newton solve and the
    snap onto the end reach the whole-interval solve's alpha).  Fails with the snap of alpha onto the interval's end removed."""
    ro, off, ri, xf, zf, pipe, o = _geom(name)
    fin = np.isfinite(o["t"])
    pinned = fin & (np.abs(o["alpha"]) == O.ALPHA_MAX)
    ie, jf = np.nonzero(fin)
    qx, qz, _, _ = pipe.q(o["beta"][fin])
    h = 1e-6
    gp = (O._lens_tg(LENS, o["alpha"][fin] + h, XE8[ie], ZE8[ie], qx, qz)[1]
          - O._lens_tg(LENS, o["alpha"][fin] - h, XE8[ie], ZE8[ie], qx, qz)[1]) / (2 * h)
    flat = np.zeros_like(fin)
    flat[fin] = (gp < GP_MIN) & ~pinned[fin]
    print(f"\n{name}: alpha pinned {int(pinned.sum())}, interior with g' < gp_min {int(flat.sum())}")
    assert pinned.sum() >= 500
    assert flat.sum() >= 90 or ro > 0.01
    tt, al, be = rtus.travel_time_pipe(XE8, ZE8, xf, zf, r_inner=ri, params=_params(rtus, ro, off), return_path=True)
    _compare(tt, o, name)
    for sel in (pinned & ~o["flag"], flat & ~o["flag"]):
        assert np.all(np.abs(tt[sel] - o["t"][sel]) <= 1e-17 + 1e-13 * o["t"][sel])
    sel = pinned & ~o["flag"]
    assert np.array_equal(al[sel], o["alpha"][sel])


def test_general_trigonometry(rtus):
    """alpha_lo, alpha_hi = -+1.05 rad: past +-1 both kernels run their sincos instantiation (POLY = false).  No mutation was found
    that this test alone catches: routing the instantiation to the polynomial changes no value (its truncation at 1.05 rad is
    1e-22), and sin alpha scaled by 1 + 1e-12 in that instantiation's lens_point (the path's lens point only, not lens_time) moves
    no time past the tolerance.  The test shows that the instantiation runs and agrees with the oracle, no more."""
    wide = 1.05
    ro, off, ri = 0.037, 0.0038, 0.029
    px, pz, _, _ = LENS.point(np.linspace(-wide, wide, 20001))
    assert np.isfinite(px).all() and np.isfinite(pz).all() and O.clearance(LENS, off, -wide, wide) > ro + 0.03
    xf, zf = _wall_grid(off, ri, ro, 5, 41, -1.2, 1.2)
    pipe = O.Pipe(ro, off, ri)
    ow = O.table(LENS, pipe, XE8, ZE8, xf, zf, a_lo=-wide, a_hi=wide)
    od = O.table(LENS, pipe, XE8, ZE8, xf, zf)
    beyond = np.isfinite(ow["t"]) & (np.abs(ow["alpha"]) > O.ALPHA_MAX)
    print(f"\nflagged {ow['flag'].mean():.4f} / {od['flag'].mean():.4f}, winners past ALPHA_MAX {int(beyond.sum())}")
    assert ow["flag"].mean() <= 2e-3 and od["flag"].mean() <= 2e-3 and beyond.sum() >= 200       # (the oracle flags none, 464 past)
    p = _params(rtus, ro, off)
    tw, aw, bw = rtus.travel_time_pipe(XE8, ZE8, xf, zf, r_inner=ri, params=p, alpha_lo=-wide, alpha_hi=wide, return_path=True)
    both = _compare(tw, ow, "wide")
    assert both.mean() > 0.9
    _check_path(aw, bw, ow, both & ~ow["flag"], pipe, XE8, ZE8, xf, zf, -wide, wide)
    # a winner whose alpha is inside +-ALPHA_MAX and off the ends in both calls is the same path
    td, ad, _ = rtus.travel_time_pipe(XE8, ZE8, xf, zf, r_inner=ri, params=p, return_path=True)
    _compare(td, od, "default")
    same = np.isfinite(tw) & np.isfinite(td) & (np.abs(aw) < O.ALPHA_MAX) & (np.abs(ad) < O.ALPHA_MAX)
    assert same.sum() >= 1000                                                                     # (1176 by the oracle)
    assert np.all(np.abs(tw[same] - td[same]) <= 1e-17 + 1e-13 * td[same])


# scan edges: one call per case, the window placed so that the oracle's winning beta of a chosen entry lies at a fraction fr of scan
# cell c (between the scan points c and c + 1); the scan points are tiled through LDS by 64
SCAN_PAIRS = [(3, 0.033, 0.10), (0, 0.031, -0.30)]          # element of XE8, radius and angle of the focal point
HB = np.pi / 465                                            # the default scan step of a 37 mm pipe


def _scan_cases():
    cases = []
    for m in (4, 5, 64, 65, 128, 129, None):
        n = 149 if m is None else m                          # a 0.999 rad window: default_n_scan gives 149 (asserted in the test)
        cells = [0, n - 2] + ([63] if n >= 65 else []) + ([127] if n >= 129 else [])
        for c in sorted(set(cells)):
            cases += [(m, c, fr) for fr in (0.03, 0.5, 0.97)]
        # a root within 1.4e-8 rad of the scan point on a tile's edge: the fp32 scan may bracket it in either cell
        for e in (64, 128):
            if n >= e + 2:
                cases += [(m, e - 1, 1 - 2e-6), (m, e, 2e-6)]
    # the minimum just outside the window: no interior minimum
    cases += [(m, c, fr) for m in (4, 65, None) for c, fr in ((-1, 0.97), ((149 if m is None else m) - 1, 0.03))]
    return cases


def test_scan_edges(rtus):
    """Fails with neg[e] cleared at the start of every tile.  With the refine's bracket shift (to beta_j-1 / beta_j+2) disabled it
    still passes: the fp32 and fp64 signs agree at every scan point of these cases, so the shift is not pinned."""
    ro, off, ri = 0.037, 0.0038, 0.029
    p = _params(rtus, ro, off)
    pipe = O.Pipe(ro, off, ri)
    seen = set()
    for ed, rf, th in SCAN_PAIRS:
        xf, zf = off + rf * np.sin(th + np.array([-0.02, 0.0, 0.02])), rf * np.cos(th + np.array([-0.02, 0.0, 0.02]))
        b0 = O.table(LENS, pipe, XE8, ZE8, xf, zf)["beta"][ed, 1]
        assert np.isfinite(b0)
        for m, c, fr in _scan_cases():
            if m is None:
                hb, n = 0.999 / 148, 149
            else:
                hb, n = HB, m
            b_lo = b0 - (c + fr) * hb
            b_hi = b_lo + (n - 1) * hb
            if m is None:
                assert O.default_n_scan(ro, b_lo, b_hi) == n
            o = O.table(LENS, pipe, XE8, ZE8, xf, zf, b_lo=b_lo, b_hi=b_hi, n_scan=n)
            assert o["flag"].mean() <= FLAG_CAP
            inside = 0 <= c <= n - 2
            if inside:                                        # the condition on the input: the chosen entry's winner is in cell c
                hb_ = (b_hi - b_lo) / (n - 1)
                assert abs(o["beta"][ed, 1] - b0) <= 1e-12 and int(np.floor((o["beta"][ed, 1] - b_lo) / hb_)) == c, (m, c, fr)
            else:
                assert np.isnan(o["t"][ed, 1]), (m, c, fr)
            tt, al, be = rtus.travel_time_pipe(XE8, ZE8, xf, zf, r_inner=ri, params=p, beta_lo=b_lo, beta_hi=b_hi, n_scan=m,
                                               return_path=True)
            _compare(tt, o, (ed, m, c, fr))
            if inside:
                assert abs(tt[ed, 1] - o["t"][ed, 1]) <= 1e-17 + 1e-13 * o["t"][ed, 1], (ed, m, c, fr)
                assert abs(be[ed, 1] - b0) <= 1e-9 and abs(al[ed, 1] - o["alpha"][ed, 1]) <= 1e-9, (ed, m, c, fr)
            else:
                assert np.isnan(tt[ed, 1]), (ed, m, c, fr)
            seen.add((n, c if inside else None))
    assert {(65, 63), (129, 63), (129, 127), (149, 63), (149, 127), (4, 0), (4, 2), (4, None), (149, None)} <= seen


def test_edge_inputs(rtus):
    """non-finite elements and focal points, focal points exactly on the wall's two circles and at the centre: NaN, and nothing
    else in the call changes a bit.  Fails with the wall closed (rf >= r_inner && rf <= r_outer)."""
    ro, off, ri = 0.037, 0.0038, 0.029
    p = _params(rtus, ro, off)
    xf, zf = rtus.pipe_wall_grid(ri + 1e-4, ro - 1e-4, 5, 21, -0.45, 0.45, params=p)
    kw = dict(r_inner=ri, params=p, return_path=True)
    base = rtus.travel_time_pipe(XE8, ZE8, xf, zf, **kw)
    assert np.isfinite(base[0]).mean() > 0.9
    # elements: NaN x in slot 2, inf z in slot 7 (the last row of the first block of 8), the others keep their order
    xe, ze = np.insert(XE8, [2, 6], [np.nan, 0.001]), np.insert(ZE8, [2, 6], [O.D, np.inf])
    assert xe.size == 10 and np.isnan(xe[2]) and np.isinf(ze[7])
    keep = np.array([0, 1, 3, 4, 5, 6, 8, 9])
    got = rtus.travel_time_pipe(xe, ze, xf, zf, **kw)
    for g, b in zip(got, base):
        assert np.isnan(g[[2, 7]]).all() and np.array_equal(g[keep], b, equal_nan=True)
    with np.errstate(all="ignore"):
        o = O.table(LENS, O.Pipe(ro, off, ri), xe, ze, xf, zf)
    assert o["flag"].mean() <= 2e-3
    _compare(got[0], o, "bad elements")
    # focal points
    bad_x = np.array([np.nan, off, np.inf, off, off, off, off, off])
    bad_z = np.array([0.033, -np.inf, 0.033, ri, ro, 0.0, -ri, -ro])
    at = np.array([0, 1, 50, 63, 64, 65, 104, 105])                      # slots of the untouched grid to insert before
    xg, zg = np.insert(xf, at, bad_x), np.insert(zf, at, bad_z)
    bad = np.zeros(xg.size, dtype=bool)
    bad[at + np.arange(at.size)] = True
    assert np.array_equal(xg[~bad], xf) and np.isnan(xg[0]) and zg[-1] == -ro
    got = rtus.travel_time_pipe(XE8, ZE8, xg, zg, **kw)
    for g, b in zip(got, base):
        assert np.isnan(g[:, bad]).all() and np.array_equal(g[:, ~bad], b, equal_nan=True)
    with np.errstate(all="ignore"):
        o = O.table(LENS, O.Pipe(ro, off, ri), XE8, ZE8, xg, zg)
    assert o["flag"].mean() <= 2e-3
    _compare(got[0], o, "bad points")
    # a solid bar: its centre is not in the wall (r_inner = 0 < |F - Cp| is strict)
    kw0 = dict(r_inner=0.0, params=p, return_path=True)
    base0 = rtus.travel_time_pipe(XE8, ZE8, xf, zf, **kw0)
    got = rtus.travel_time_pipe(XE8, ZE8, np.insert(xf, 40, off), np.insert(zf, 40, 0.0), **kw0)
    for g, b in zip(got, base0):
        assert np.isnan(g[:, 40]).all() and np.array_equal(np.delete(g, 40, axis=1), b, equal_nan=True)
    assert np.isfinite(base0[0]).mean() > 0.9


def test_launch_shapes(rtus):
    """n_e in {1, 8, 9, 17} x n_f in {1, 255, 256, 257} (workgroups of 8 elements x 256 focal points): every entry is the entry of
    one big call, through the host twin and on device tensors.  Fails with the Newton start moved by the parity of the slot."""
    import torch
    dev = import_module("ray-tracing-ultrasound_amd.device")
    ro, off, ri = 0.037, 0.0038, 0.029
    p = _params(rtus, ro, off)
    xe, ze = XE64[5::3][:17], ZE64[:17]
    xf, zf = _wall_grid(off, ri, ro, 1, 257, -0.6, 0.6, margin=3e-3)
    kw = dict(r_inner=ri, params=p)
    full = rtus.travel_time_pipe(xe, ze, xf, zf, return_path=True, **kw)
    assert np.isfinite(full[0]).mean() > 0.9
    t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")      # noqa: E731
    for n_e in (1, 8, 9, 17):
        for n_f in (1, 255, 256, 257):
            # the last elements and points of the big call: no entry keeps its slot
            es, fs = slice(17 - n_e, 17), slice(257 - n_f, 257)
            got = rtus.travel_time_pipe(xe[es], ze[es], xf[fs], zf[fs], return_path=True, **kw)
            out = [torch.empty((n_e, n_f), dtype=torch.float64, device="cuda") for _ in range(3)]
            dev.tt_pipe_dev(t(xe[es]), t(ze[es]), t(xf[fs]), t(zf[fs]), out=out[0], alpha_out=out[1], beta_out=out[2], **kw)
            torch.cuda.synchronize()
            for g, d, f in zip(got, out, full):
                assert np.array_equal(g, f[es, fs], equal_nan=True), (n_e, n_f)
                assert np.array_equal(d.cpu().numpy(), f[es, fs], equal_nan=True), (n_e, n_f)

"""GPU: rtus_leg_amp_surface at its decision points, against 40-digit values (tests/golden/amp_branches.npz, made by
tests/golden/make_amp_branches.py from the forward-shot paths of tests/amp_branch_cases.py; checked on the CPU by
tests/test_amp_branches_cpu.py).  No solver is in the loop: the paths are inputs.  This module reads the fixture only.

Classes (least counts and what makes a case a member: the CPU test, from the fixture's own labels and 40-digit J, p, D):
critical slownesses p c = 1 +- {1e-3, 1e-6, 1e-8} at the surface (c_l; the wave's own grazing; on the second pair, c_t < c1 < c_l,
the couplant's c1 on the up legs) and at the backwall, exact normal incidence, the directivity (width 0, either side of the first two
nulls, u < 0), the ray tube through the focus (both signs of J, |J| down to 1e-9) and on a 50 um ripple, the no-ray rule either side
of tangency, NaN and infinite paths, x_entry on and next to the spline's knots — six legs, both directions wherever the class applies.

Bars.  Masks first, exactly, for every entry of every call: NaN, inf and == 0 masks equal to the reference's (the matrix entries that
belong to no case hold a NaN path and must be NaN).  Then |amp - ref| <= 2^-23 |ref| + 16 E64 |ref| on the finite, non-zero entries:
the rounding of the two fp32 components, and 16 times the class's E64, the fp64 NumPy oracle's own largest relative error against
the reference (measured by the CPU test, stored in the fixture, tabulated in DESIGN.md; <= 1e-7 by construction of the classes).
The code under test sets no tolerance."""
import numpy as np
import pytest

import amp_branch_cases as B

pytestmark = pytest.mark.gpu

FX = B.load()
NAMES = [str(c) for c in FX["s_classes"]]
CALLS = B.calls(FX, "s_")
ZS = [B.profile(k) for k in B.PROFILES]
_done = {}


def _run(rtus, call, cols=None, rows=None, xback=True):
    """the call through the host API -> complex64 [n_e][n_f]; cols / rows: a subset, a tiling or a permutation of its points / elements"""
    k = call["key"]
    leg, med = B.LEGS[k["leg"]], B.MEDIA[k["med"]]
    cols = np.arange(call["idx"].size) if cols is None else cols
    rows = np.arange(call["xe"].size) if rows is None else rows
    xn = B.matrix(call, FX["s_xent"])[np.ix_(rows, cols)]
    xb = B.matrix(call, FX["s_xback"])[np.ix_(rows, cols)] if len(leg) == 2 else None
    idx = call["idx"][cols]
    return rtus.leg_amplitudes_surface(B.X0, B.DX, ZS[k["prof"]], med[0], med[1], med[2], med[3], med[4], B.ZB, leg, call["xe"][rows],
                                       call["ze"][rows], FX["s_xf"][idx], FX["s_zf"][idx], xn, xb, up=bool(k["up"]),
                                       element_width=float(k["width"]), f_c=float(k["fc"]))


def _amp(rtus, ci):
    if ci not in _done:
        _done[ci] = _run(rtus, CALLS[ci])
    return _done[ci]


def _bar(name):
    return 2.0 ** -23 + 16 * FX["s_E64"][NAMES.index(name)]


@pytest.mark.parametrize("name", NAMES)
def test_class_against_the_reference(rtus, name):
    k = NAMES.index(name)
    seen, worst = 0, 0.0
    for ci, call in enumerate(CALLS):
        mine = FX["s_cls"][call["idx"]] == k
        if not mine.any():
            continue
        amp = _amp(rtus, ci)
        assert amp.dtype == np.complex64 and amp.shape == (call["xe"].size, call["idx"].size)
        ref = B.matrix(call, FX["s_ref"].real) + 1j * B.matrix(call, FX["s_ref"].imag)       # NaN + NaN i off the cases
        j = np.nonzero(mine)[0]
        got, want = amp[:, j], ref[:, j]                                                       # the whole columns of this class
        assert np.array_equal(np.isnan(got.real) | np.isnan(got.imag), np.isnan(want)), f"{name}: NaN mask"
        assert np.array_equal(np.isinf(got), np.isinf(want)), f"{name}: inf mask"
        assert np.array_equal(got == 0, want == 0), f"{name}: zero mask"
        g, w = amp[call["row"][j], j].astype(np.complex128), FX["s_ref"][call["idx"][j]]
        cmp = np.isfinite(w) & (w != 0)
        err = np.abs(g[cmp] - w[cmp]) / np.abs(w[cmp])
        worst = max(worst, float(np.max(err, initial=0.0)))
        seen += int(mine.sum())
    print(f"{name}: {seen} cases, largest device error {worst:.3e} = {worst / _bar(name):.3f} of the bar {_bar(name):.3e}")
    assert seen == int(np.sum(FX["s_cls"] == k)) and seen > 0
    assert worst <= _bar(name)


def test_width_zero_ignores_f_c(rtus):
    """width = 0: f_c = 1 and f_c = 5e6 give the same bits"""
    a = [ci for ci, c in enumerate(CALLS) if c["key"]["width"] == 0 and c["key"]["fc"] == 5e6]
    assert len(a) >= 4
    for ci in a:
        twin = [cj for cj, c in enumerate(CALLS) if c["key"]["fc"] == 1.0 and all(c["key"][k] == CALLS[ci]["key"][k] for k in B.S_KEY if k != "fc")]
        sel = np.isin(FX["s_cls"][CALLS[ci]["idx"]], [NAMES.index("dir_width0_down"), NAMES.index("dir_width0_up")])
        assert sel.all() and len(twin) == 1
        t = CALLS[twin[0]]
        pos = [int(np.nonzero((FX["s_xent"][t["idx"]] == FX["s_xent"][i]) & (FX["s_xe"][t["idx"]] == FX["s_xe"][i])
                              & np.isin(FX["s_cls"][t["idx"]], [NAMES.index("dir_width0_down"), NAMES.index("dir_width0_up")]))[0][0])
               for i in CALLS[ci]["idx"]]
        a5, a1 = _amp(rtus, ci), _amp(rtus, twin[0])
        for j, (i, p) in enumerate(zip(CALLS[ci]["idx"], pos)):
            v5, v1 = a5[CALLS[ci]["row"][j], j], a1[t["row"][p], p]
            assert np.isfinite(v5) and v5 != 0 and v5.view(np.uint64) == v1.view(np.uint64)


def test_normal_incidence_is_exact(rtus):
    """x_entry == xe == xf on the flat profile: p == 0 and u == 0.0; the legs with a T in them are exactly 0 (== on the value: the signed
    zeros may differ), the others carry D == 1: the same bits as with width 0"""
    ks = [NAMES.index("normal_down"), NAMES.index("normal_up")]
    n = 0
    for ci, call in enumerate(CALLS):
        j = np.nonzero(np.isin(FX["s_cls"][call["idx"]], ks))[0]
        if j.size == 0:
            continue
        amp = _amp(rtus, ci)
        leg = B.LEGS[call["key"]["leg"]]
        v = amp[call["row"][j], j]
        if "T" in leg:
            assert np.all(v == 0)
        else:
            assert np.all(np.isfinite(v) & (v != 0))
            k = call["key"]
            med = B.MEDIA[k["med"]]
            i = call["idx"][j]
            w0 = rtus.leg_amplitudes_surface(B.X0, B.DX, ZS[k["prof"]], *med, B.ZB, leg, FX["s_xe"][i[:1]], FX["s_ze"][i[:1]], FX["s_xf"][i],
                                             FX["s_zf"][i], FX["s_xent"][i][None, :], FX["s_xback"][i][None, :] if len(leg) == 2 else None,
                                             up=bool(k["up"]))
            same = FX["s_xe"][i] == FX["s_xe"][i[0]]
            assert np.array_equal(w0[0][same].view(np.uint64), v[same].view(np.uint64)), "D == 1 exactly at u == 0"
        n += j.size
    assert n == 24


def test_x_back_is_not_read_for_direct_legs(rtus):
    """for L and T an x_back that is passed, and full of NaN, does not matter: the same bits as with a null pointer (through the C
    entry: the Python layer drops x_back for a direct leg)"""
    L = rtus.lib()
    p = lambda a: a.ctypes.data                                                 # noqa: E731
    n = 0
    for call in CALLS:
        k = call["key"]
        leg = B.LEGS[k["leg"]]
        if len(leg) == 2 or k["width"] != B.W_EL or call["idx"].size < 12:
            continue
        med = B.MEDIA[k["med"]]
        zs, xe, ze = ZS[k["prof"]], call["xe"], call["ze"]
        xf, zf = np.ascontiguousarray(FX["s_xf"][call["idx"]]), np.ascontiguousarray(FX["s_zf"][call["idx"]])
        xn = np.ascontiguousarray(B.matrix(call, FX["s_xent"]))
        nanb = np.full(xn.shape, np.nan)
        outs = []
        for xb in (None, p(nanb)):
            out = np.zeros(xn.shape, dtype=np.complex64)
            st = L.rtus_leg_amp_surface(B.X0, B.DX, p(zs), zs.size, med[0], med[1], med[2], med[3], med[4], B.ZB, int(k["leg"]), int(k["up"]),
                                        float(k["width"]), float(k["fc"]), p(xe), p(ze), xe.size, p(xf), p(zf), xf.size, p(xn), xb, p(out), 0)
            assert st == 0
            outs.append(out)
        assert np.isfinite(outs[0]).sum() == call["idx"].size
        assert np.array_equal(outs[0].view(np.uint64), outs[1].view(np.uint64))
        n += 1
    assert n >= 4


# ---------------------------------------------------------------------------------------------- launch edges
def _big_calls():
    """per leg and direction the call with the most points (the W_EL calls: plain, normal, tube, ripple and knot cases together)"""
    best = {}
    for ci, c in enumerate(CALLS):
        key = (int(c["key"]["leg"]), int(c["key"]["up"]))
        if key not in best or c["idx"].size > CALLS[best[key]]["idx"].size:
            best[key] = ci
    return [best[k] for k in sorted(best)]


def test_launch_edges_keep_every_bit(rtus):
    """an entry depends on its own inputs only: n_e = 1 (every row of every call on its own), n_f in {1, 255, 256, 257, 513} (the
    call's points tiled or truncated to that number: one thread, one short of a block, a block, one over, two blocks and one) and
    permuted columns give the bits of the plain call"""
    for ci, call in enumerate(CALLS):
        full = _amp(rtus, ci)
        for r in range(call["xe"].size):
            one = _run(rtus, call, rows=np.array([r]))
            assert np.array_equal(one.view(np.uint64), full[r:r + 1].view(np.uint64)), (ci, r)
    rng = np.random.default_rng(1)
    for ci in _big_calls():
        call, full = CALLS[ci], _amp(rtus, ci)
        assert call["idx"].size >= 8
        for n_f in (1, 255, 256, 257, 513):
            cols = np.resize(np.arange(call["idx"].size), n_f)
            got = _run(rtus, call, cols=cols)
            assert got.shape == (call["xe"].size, n_f)
            assert np.array_equal(got.view(np.uint64), full[:, cols].view(np.uint64)), (ci, n_f)
        perm = rng.permutation(call["idx"].size)
        assert np.array_equal(_run(rtus, call, cols=perm).view(np.uint64), full[:, perm].view(np.uint64)), ci


def test_device_twin_writes_its_table_only(rtus):
    """rtus_leg_amp_surface_dev into the middle of a tensor filled with a sentinel: one guard row before and two after [n_e][n_f]
    keep every bit, and the table has the host call's bits"""
    import torch
    from importlib import import_module
    dev = import_module("ray-tracing-ultrasound_amd.device")
    ci = max((c for c in _big_calls() if len(B.LEGS[CALLS[c]["key"]["leg"]]) == 2), key=lambda c: CALLS[c]["idx"].size * CALLS[c]["xe"].size)
    call, full = CALLS[ci], _amp(rtus, ci)
    k = call["key"]
    leg, med = B.LEGS[k["leg"]], B.MEDIA[k["med"]]
    n_e, n_f = full.shape
    assert n_e >= 2 and n_f % 64 != 0
    f64 = dict(dtype=torch.float64, device="cuda")
    t = [torch.as_tensor(np.ascontiguousarray(v), **f64) for v in (ZS[k["prof"]], call["xe"], call["ze"], FX["s_xf"][call["idx"]],
                                                                  FX["s_zf"][call["idx"]], B.matrix(call, FX["s_xent"]),
                                                                  B.matrix(call, FX["s_xback"]))]
    sentinel = -7.25
    big = torch.full((n_e + 3, n_f, 2), sentinel, dtype=torch.float32, device="cuda")
    dev.leg_amp_surface_dev(B.X0, B.DX, t[0], med[0], med[1], med[2], med[3], med[4], B.ZB, leg, *t[1:5], t[5], t[6], up=bool(k["up"]),
                            element_width=float(k["width"]), f_c=float(k["fc"]), out=big[1:1 + n_e])
    torch.cuda.synchronize()
    h = big.cpu().numpy()
    assert np.all(h[0] == sentinel) and np.all(h[1 + n_e:] == sentinel)
    assert np.array_equal(h[1:1 + n_e].view(np.complex64)[..., 0].view(np.uint64), full.view(np.uint64))

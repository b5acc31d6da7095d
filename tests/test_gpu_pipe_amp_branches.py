"""GPU: rtus_leg_amp_pipe at its decision points, against 40-digit values (tests/golden/amp_branches.npz, made by
tests/golden/make_amp_branches.py from the forward-shot paths of tests/amp_branch_cases.py; checked on the CPU by
tests/test_amp_branches_cpu.py).  No solver is in the loop: alpha, beta, gamma are inputs.  This module reads the fixture only.

Classes: plain paths (also with a lens interval past +-1 rad, the kernel's other sincos), critical slownesses p c_l = 1 +- {1e-3,
1e-6, 1e-8} at the outer circle and at the bore (10 mm corner), each of the six no-ray conditions failing alone either side of
tangency, the pinned alpha (the default and a caller's interval; one ulp inside is a ray), NaN in alpha, beta, gamma alone, the
tube through the focus in the wall (both signs of J, |J| down to 3e-9) and with the lens focus before the outer circle — and the
mirror image in x of every case, with its own reference value.

Bars: tests/test_gpu_amp_branches.py's — the three masks exactly for every entry of every call, then
|amp - ref| <= 2^-23 |ref| + 16 E64 |ref| per class, E64 the fp64 NumPy oracle's own error against the reference (fixture)."""
import ctypes as C

import numpy as np
import pytest

import amp_branch_cases as B

pytestmark = pytest.mark.gpu

FX = B.load()
NAMES = [str(c) for c in FX["p_classes"]]
CALLS = B.calls(FX, "p_")
RL, CTL, RW, R2, CL, CT = B.P_MEDIA
MKW = dict(c_l=CL, c_t=CT, rho_wall=R2, rho_water=RW, rho_lens=RL, ct_lens=CTL)
_done = {}


def _run(rtus, call, cols=None, rows=None):
    k = call["key"]
    leg = B.LEGS[k["leg"]]
    cols = np.arange(call["idx"].size) if cols is None else cols
    rows = np.arange(call["xe"].size) if rows is None else rows
    ix = np.ix_(rows, cols)
    al, be = B.matrix(call, FX["p_alpha"])[ix], B.matrix(call, FX["p_beta"])[ix]
    ga = B.matrix(call, FX["p_gamma"])[ix] if len(leg) == 2 else None
    idx = call["idx"][cols]
    p = rtus.Params(r_outer=float(k["ro"]), pipe_offset=float(k["xoff"]))
    return rtus.leg_amplitudes_pipe(leg, call["xe"][rows], call["ze"][rows], FX["p_xf"][idx], FX["p_zf"][idx], al, be, ga,
                                    r_inner=float(k["ri"]), params=p, up=bool(k["up"]), element_width=float(k["width"]),
                                    f_c=float(k["fc"]), alpha_lo=float(k["alo"]), alpha_hi=float(k["ahi"]), **MKW)


def _amp(rtus, ci):
    if ci not in _done:
        _done[ci] = _run(rtus, CALLS[ci])
    return _done[ci]


def _bar(name):
    return 2.0 ** -23 + 16 * FX["p_E64"][NAMES.index(name)]


@pytest.mark.parametrize("name", NAMES)
def test_class_against_the_reference(rtus, name):
    k = NAMES.index(name)
    seen, worst, mirrored = 0, 0.0, 0
    for ci, call in enumerate(CALLS):
        mine = FX["p_cls"][call["idx"]] == k
        if not mine.any():
            continue
        amp = _amp(rtus, ci)
        assert amp.dtype == np.complex64 and amp.shape == (call["xe"].size, call["idx"].size)
        ref = B.matrix(call, FX["p_ref"].real) + 1j * B.matrix(call, FX["p_ref"].imag)       # NaN + NaN i off the cases
        j = np.nonzero(mine)[0]
        got, want = amp[:, j], ref[:, j]
        assert np.array_equal(np.isnan(got), np.isnan(want)), f"{name}: NaN mask"
        assert np.array_equal(np.isinf(got), np.isinf(want)), f"{name}: inf mask"
        assert np.array_equal(got == 0, want == 0), f"{name}: zero mask"
        g, w = amp[call["row"][j], j].astype(np.complex128), FX["p_ref"][call["idx"][j]]
        cmp = np.isfinite(w) & (w != 0)
        worst = max(worst, float(np.max(np.abs(g[cmp] - w[cmp]) / np.abs(w[cmp]), initial=0.0)))
        seen += int(mine.sum())
        mirrored += int(np.sum(FX["p_mir"][call["idx"][j]] == 1))
    print(f"{name}: {seen} cases ({mirrored} mirrored), largest device error {worst:.3e} = {worst / _bar(name):.3f} of the bar {_bar(name):.3e}")
    assert seen == int(np.sum(FX["p_cls"] == k)) and seen > 0 and 2 * mirrored == seen
    assert worst <= _bar(name)


def test_gamma_is_not_read_for_direct_legs(rtus):
    """for L and T a gamma that is passed, and full of NaN, does not matter: the same bits as with a null pointer (through the C
    entry: the Python layer drops gamma for a direct leg)"""
    L = rtus.lib()
    p = lambda a: a.ctypes.data                                                 # noqa: E731
    n = 0
    for call in CALLS:
        k = call["key"]
        leg = B.LEGS[k["leg"]]
        rays = FX["p_ref"][call["idx"]]
        rays = int(np.sum(np.isfinite(rays) & (rays != 0)))
        if len(leg) == 2 or rays < 6:
            continue
        lens = rtus.Params().lens()
        pipe = rtus.Pipe(float(k["ro"]), float(k["ri"]), float(k["xoff"]), 0.0)
        media = rtus.PipeMedia(RL, CTL, RW, R2, CL, CT)
        xe, ze = call["xe"], call["ze"]
        xf, zf = np.ascontiguousarray(FX["p_xf"][call["idx"]]), np.ascontiguousarray(FX["p_zf"][call["idx"]])
        al, be = np.ascontiguousarray(B.matrix(call, FX["p_alpha"])), np.ascontiguousarray(B.matrix(call, FX["p_beta"]))
        nang = np.full(al.shape, np.nan)
        outs = []
        for ga in (None, p(nang)):
            out = np.zeros(al.shape, dtype=np.complex64)
            st = L.rtus_leg_amp_pipe(C.byref(lens), float(k["alo"]), float(k["ahi"]), C.byref(pipe), C.byref(media), int(k["leg"]),
                                     int(k["up"]), float(k["width"]), float(k["fc"]), p(xe), p(ze), xe.size, p(xf), p(zf), xf.size,
                                     p(al), p(be), ga, p(out), 0)
            assert st == 0
            outs.append(out)
        assert np.sum(np.isfinite(outs[0]) & (outs[0] != 0)) == rays
        assert np.array_equal(outs[0].view(np.uint64), outs[1].view(np.uint64))
        n += 1
    assert n >= 4


def _big_calls():
    best = {}
    for ci, c in enumerate(CALLS):
        key = (int(c["key"]["leg"]), int(c["key"]["up"]))
        if key not in best or c["idx"].size > CALLS[best[key]]["idx"].size:
            best[key] = ci
    return [best[k] for k in sorted(best)]


def test_launch_edges_keep_every_bit(rtus):
    """an entry depends on its own inputs only: n_e = 1 (every row of every call on its own), n_f in {1, 255, 256, 257, 513} (the
    call's points tiled or truncated to that number) and permuted columns give the bits of the plain call"""
    for ci, call in enumerate(CALLS):
        full = _amp(rtus, ci)
        for r in range(call["xe"].size):
            one = _run(rtus, call, rows=np.array([r]))
            assert np.array_equal(one.view(np.uint64), full[r:r + 1].view(np.uint64)), (ci, r)
    rng = np.random.default_rng(2)
    for ci in _big_calls():
        call, full = CALLS[ci], _amp(rtus, ci)
        assert call["idx"].size >= 4
        for n_f in (1, 255, 256, 257, 513):
            cols = np.resize(np.arange(call["idx"].size), n_f)
            got = _run(rtus, call, cols=cols)
            assert got.shape == (call["xe"].size, n_f)
            assert np.array_equal(got.view(np.uint64), full[:, cols].view(np.uint64)), (ci, n_f)
        perm = rng.permutation(call["idx"].size)
        assert np.array_equal(_run(rtus, call, cols=perm).view(np.uint64), full[:, perm].view(np.uint64)), ci


def test_device_twin_writes_its_table_only(rtus):
    """rtus_leg_amp_pipe_dev into the middle of a tensor filled with a sentinel: one guard row before and two after [n_e][n_f] keep
    every bit, and the table has the host call's bits"""
    import torch
    from importlib import import_module
    dev = import_module("ray-tracing-ultrasound_amd.device")
    ci = max((c for c in _big_calls() if len(B.LEGS[CALLS[c]["key"]["leg"]]) == 2), key=lambda c: CALLS[c]["idx"].size * CALLS[c]["xe"].size)
    call, full = CALLS[ci], _amp(rtus, ci)
    k = call["key"]
    leg = B.LEGS[k["leg"]]
    n_e, n_f = full.shape
    assert n_e >= 2 and n_f % 64 != 0
    f64 = dict(dtype=torch.float64, device="cuda")
    t = [torch.as_tensor(np.ascontiguousarray(v), **f64) for v in (call["xe"], call["ze"], FX["p_xf"][call["idx"]], FX["p_zf"][call["idx"]],
                                                                  B.matrix(call, FX["p_alpha"]), B.matrix(call, FX["p_beta"]),
                                                                  B.matrix(call, FX["p_gamma"]))]
    sentinel = -7.25
    big = torch.full((n_e + 3, n_f, 2), sentinel, dtype=torch.float32, device="cuda")
    p = rtus.Params(r_outer=float(k["ro"]), pipe_offset=float(k["xoff"]))
    dev.leg_amp_pipe_dev(leg, *t, r_inner=float(k["ri"]), params=p, up=bool(k["up"]), element_width=float(k["width"]), f_c=float(k["fc"]),
                         alpha_lo=float(k["alo"]), alpha_hi=float(k["ahi"]), out=big[1:1 + n_e], **MKW)
    torch.cuda.synchronize()
    h = big.cpu().numpy()
    assert np.all(h[0] == sentinel) and np.all(h[1 + n_e:] == sentinel)
    assert np.array_equal(h[1:1 + n_e].view(np.complex64)[..., 0].view(np.uint64), full.view(np.uint64))

"""GPU: the three element matchers — the stand-alone kernel's search on an ascending aperture, its full scan, and the matcher
fused into the forward trace — give np.isclose's decisions on landing points within 4 ulp of the edge of every element's
tolerance (tests/match_edge_cases.py; its premises: tests/test_match_edge_cases_cpu.py).  Every comparison is exact: hit,
first_ray and ray_hits as arrays, tof_hit bit for bit.  Each test prints how many probes, hits and differing decisions it saw."""
from importlib import import_module

import numpy as np
import pytest

import match_edge_cases as M
from conftest import D_PLANE

pytestmark = pytest.mark.gpu

KEYS = ("hit", "first_ray", "tof_hit")


def _differ(got, ref):
    """decisions that differ: elements whose hit / first_ray / tof_hit bits differ, plus rays whose ray_hits flag differs"""
    n = 0
    for k, g in got.items():
        r = ref[k]
        assert g.shape == r.shape, k
        n += int((g.view(np.uint64) != r.view(np.uint64)).sum()) if k == "tof_hit" else int((g != r).sum())
    return n


def _standalone(rtus, dev_api, torch, land, tof, x_rx, atol, rtol):
    """one row through match_elements, ray_hits and device.match_dev -> three dicts of decisions"""
    hit, th, first = rtus.match_elements(land, tof, x_rx, atol=atol, rtol=rtol)
    host = dict(hit=hit, first_ray=first, tof_hit=th, ray_hits=rtus.ray_hits(land, x_rx, atol=atol, rtol=rtol))
    t64 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")
    f, h, t = dev_api.match_dev(t64(land)[None], t64(tof)[None], t64(x_rx), atol, rtol)
    dev = dict(hit=h.cpu().numpy()[0].astype(bool), first_ray=f.cpu().numpy()[0], tof_hit=t.cpu().numpy()[0])
    return host, dev


@pytest.mark.parametrize("name,x", M.apertures())
def test_standalone_kernel_at_the_edges(rtus, name, x):
    """all orders x all nine (atol, rtol): an ascending aperture takes the kernel's windowed search, any other its full scan"""
    import torch
    dev_api = import_module("ray-tracing-ultrasound_amd.device")
    probes = hits = differ = 0
    bad = []
    for atol, rtol in M.PAIRS:
        asc = M.case(x, atol, rtol)
        by_order = {}
        for order in M.ORDERS:
            idx = M.order_index(x.size, order)
            if idx is None:
                continue
            c = M.case(x[idx], atol, rtol)
            host, dev = _standalone(rtus, dev_api, torch, c["land"], c["tof"], c["x_rx"], atol, rtol)
            d = _differ(host, c) + _differ(dev, c)
            probes += c["land"].size; hits += int(c["hit"].sum()); differ += d
            if d:
                bad.append((atol, rtol, order, d))
            # the ascending case's rays against this order of the elements: the same decisions, permuted
            h, t, f = rtus.match_elements(asc["land"], asc["tof"], x[idx], atol=atol, rtol=rtol)
            by_order[order] = dict(hit=h, first_ray=f, tof_hit=t), idx
        for order, (got, idx) in by_order.items():
            p = {k: asc[k][idx] for k in KEYS}
            d = _differ(got, p) + _differ(got, {k: by_order["ascending"][0][k][idx] for k in KEYS})
            differ += d
            if d:
                bad.append((atol, rtol, order + " as a permutation", d))
    print(f"{name}: {probes} probes, {hits} element hits, {differ} decisions differ {bad}")
    assert differ == 0, bad


def test_match_dev_into_given_tensors(rtus):
    import torch
    dev_api = import_module("ray-tracing-ultrasound_amd.device")
    t64 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")
    c = M.case(M.base_aperture(65), 2e-3, 0.0)
    out = (torch.full((1, 65), 7, dtype=torch.int32, device="cuda"), torch.full((1, 65), 7, dtype=torch.uint8, device="cuda"),
           torch.full((1, 65), 7.0, dtype=torch.float64, device="cuda"))
    back = dev_api.match_dev(t64(c["land"])[None], t64(c["tof"])[None], t64(c["x_rx"]), 2e-3, 0.0, out=out)
    assert all(a is b for a, b in zip(back, out))
    got = dict(first_ray=out[0].cpu().numpy()[0], hit=out[1].cpu().numpy()[0].astype(bool), tof_hit=out[2].cpu().numpy()[0])
    d = _differ(got, c)
    print(f"out=: {c['land'].size} probes, {int(c['hit'].sum())} element hits, {d} decisions differ")
    assert d == 0


@pytest.mark.parametrize("atol,rtol", M.SHARP)
def test_chunked_rows(rtus, atol, rtol):
    """820 rows x 5 workgroups: every workgroup of the stand-alone kernel takes two 256-ray chunks.  All rows against the rotated
    reference; rows 0, 1, 409 and 819 again from single-row calls, which run with one chunk per workgroup."""
    import torch
    dev_api = import_module("ray-tracing-ultrasound_amd.device")
    c = M.chunked_rows(atol, rtol)
    ref = dict(hit=c["hit_rows"], first_ray=c["first_rows"], tof_hit=c["tof_hit_rows"], ray_hits=c["ray_hits_rows"])
    hit, th, first = rtus.match_elements(c["land_rows"], c["tof_rows"], c["x_rx"], atol=atol, rtol=rtol)
    got = dict(hit=hit, first_ray=first, tof_hit=th, ray_hits=rtus.ray_hits(c["land_rows"], c["x_rx"], atol=atol, rtol=rtol))
    d = _differ(got, ref)
    t64 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device="cuda")
    f, h, t = dev_api.match_dev(t64(c["land_rows"]), t64(c["tof_rows"]), t64(c["x_rx"]), atol, rtol)
    d += _differ(dict(hit=h.cpu().numpy().astype(bool), first_ray=f.cpu().numpy(), tof_hit=t.cpu().numpy()), ref)
    one = 0
    for k in (0, 1, 409, 819):
        h1, t1, f1 = rtus.match_elements(c["land_rows"][k], c["tof_rows"][k], c["x_rx"], atol=atol, rtol=rtol)
        r1 = rtus.ray_hits(c["land_rows"][k], c["x_rx"], atol=atol, rtol=rtol)
        row = {key: v[k] for key, v in ref.items()}
        one += _differ(dict(hit=h1, first_ray=f1, tof_hit=t1, ray_hits=r1), row)
        one += _differ(dict(hit=h1, first_ray=f1, tof_hit=t1, ray_hits=r1), {key: v[k] for key, v in got.items()})
    print(f"atol {atol:g} rtol {rtol:g}: {c['land_rows'].size} probes in {M.ROWS} rows, {int(ref['hit'].sum())} element hits, "
          f"{d} decisions differ in the chunked calls, {one} in the single-row calls")
    assert d == 0 and one == 0


# ------------------------------------------------------------------------------------------------------------------ fused kernel
XA = np.array([0.0, -0.0123, 0.0081])
GEOM = dict(r_outer=0.037, pipe_offset=0.0038)
_traced = {}


def _trace(rtus, n, fast=False):
    """land_x [3, n] of one shoot_batch call (computed once per ray count and mode)"""
    if (n, fast) not in _traced:
        alpha = np.linspace(-rtus.ALPHA_MAX, rtus.ALPHA_MAX, n)
        b = rtus.shoot_batch(XA, np.full(3, D_PLANE), np.full(n, D_PLANE), alpha, params=rtus.Params(**GEOM), want=("land_x",), fast=fast)
        b["land_x"].setflags(write=False)
        _traced[(n, fast)] = b["land_x"][0]
    return _traced[(n, fast)]


def _fused(rtus, n, x_rx, atol, rtol, fast=False):
    """one aperture through sweep_batch twice (travel times on demand / stored) -> (probes, hits, decisions that differ)"""
    alpha = np.linspace(-rtus.ALPHA_MAX, rtus.ALPHA_MAX, n)
    a = (XA, np.full(3, D_PLANE), np.full(n, D_PLANE), alpha, x_rx)
    kw = dict(atol=atol, rtol=rtol, params=rtus.Params(**GEOM), fast=fast)
    lazy = rtus.sweep_batch(*a, want=(), **kw)
    full = rtus.sweep_batch(*a, want=("tof", "land_x"), **kw)
    land, tof = full["land_x"][0], full["tof"][0]
    assert M.same_bits(land, _trace(rtus, n, fast))          # the elements were built from these very landing points
    rows = [M.decisions(land[t], tof[t], x_rx, atol, rtol) for t in range(3)]
    ref = {k: np.stack([r[k] for r in rows]) for k in KEYS}
    hit, th, first = rtus.match_elements(land, tof, x_rx, atol=atol, rtol=rtol)
    d = _differ({k: lazy[k][0] for k in KEYS}, ref) + _differ({k: full[k][0] for k in KEYS}, ref)
    d += _differ(dict(hit=hit, first_ray=first, tof_hit=th), ref)
    return 3 * n * x_rx.size, int(ref["hit"].sum()), d


def _orders(x):
    out = [("ascending", x), ("reversed", x[::-1].copy())]
    idx = M.order_index(x.size, "seam")
    return out + ([("seam", x[idx])] if idx is not None else [])


@pytest.mark.parametrize("rtol", [0.0, 1e-5, 1.0, 3.0])
@pytest.mark.parametrize("n", [905, 1025])
def test_fused_kernel_at_the_edges(rtus, n, rtol):
    """elements solved from the traced landing points, each 0..4 ulp off the edge of its own tolerance; rtol >= 1 switches the
    per-wave prune off, and at rtol = 3 (unlike 1) the product rtol * |x_e| is rounded: a tolerance formed by one FMA shows"""
    land = _trace(rtus, n)
    probes = hits = differ = 0
    bad = []
    for atol in (1e-6, 1e-4, 2e-3):
        for j, n_rx in enumerate((63, 64, 65, 129)):
            x_rx, rays, dist = M.fused_elements(land[j % 3], n_rx, atol, rtol)
            assert dist.max() <= 8, (atol, n_rx, dist.max())
            for order, x in _orders(x_rx):
                p, h, d = _fused(rtus, n, x, atol, rtol)
                probes += p; hits += h; differ += d
                if d:
                    bad.append((atol, n_rx, order, d))
    print(f"n {n} rtol {rtol:g}: {probes} ray x element pairs, {hits} element hits, {differ} decisions differ {bad}")
    assert hits > 0 and differ == 0, bad


@pytest.mark.parametrize("n", [905, 1025])
def test_fused_kernel_on_the_element_below_ulp_of_atol(rtus, n):
    x_rx, atol, ray = M.residue_case(_trace(rtus, n)[0])
    x = _trace(rtus, n)[0][ray]
    assert x - x_rx[32] == atol and x - atol > x_rx[32]      # a hit that fl(x - atol) would prune
    probes = hits = differ = 0
    for order, xo in _orders(x_rx):
        p, h, d = _fused(rtus, n, xo, atol, 0.0)
        probes += p; hits += h; differ += d
    print(f"n {n}: atol {atol!r}, ray {ray}: {probes} ray x element pairs, {hits} element hits, {differ} decisions differ")
    assert differ == 0


def test_fused_kernel_at_the_edges_of_the_vector_form_trace(rtus):
    """fast=True: the same matcher, the elements built from that mode's landing points"""
    land = _trace(rtus, 905, fast=True)
    probes = hits = differ = 0
    for rtol in (0.0, 1e-5):
        x_rx, rays, dist = M.fused_elements(land[1], 65, 1e-4, rtol)
        assert dist.max() <= 8
        for order, x in _orders(x_rx):
            p, h, d = _fused(rtus, 905, x, 1e-4, rtol, fast=True)
            probes += p; hits += h; differ += d
    print(f"fast: {probes} ray x element pairs, {hits} element hits, {differ} decisions differ")
    assert hits > 0 and differ == 0

"""Device-resident calls: torch tensors in HBM -> the ``*_dev`` entry points of include/rtus.h.

PyTorch is only plumbing here (device memory + the current HIP stream); every kernel is
librtus.so's.  All calls are asynchronous on ``torch.cuda.current_stream()``.
"""
import ctypes as C

import torch

import numpy as np

from . import _lib
from . import api as _api
from .api import POLYLINE_READY, TAUP_TAIL, Params, _resolve


def _chk(t, name, dtype=torch.float64):
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == dtype and t.is_contiguous()):
        raise ValueError(f"{name} must be a contiguous CUDA tensor of {dtype}")
    return t


def _p(t):
    return None if t is None else t.data_ptr()


def _pair(xe, ze, xf, zf, dtype=torch.float64):
    """xe/ze [n_e] and xf/zf [n_f], checked -> (n_e, n_f)"""
    for t, n in ((xe, "xe"), (ze, "ze"), (xf, "xf"), (zf, "zf")):
        _chk(t, n, dtype)
    n_e, n_f = xe.numel(), xf.numel()
    if ze.numel() != n_e or zf.numel() != n_f:
        raise ValueError("xe/ze and xf/zf must pair up")
    return n_e, n_f


def _result(out, shape, ref, dtype=torch.float64, name="out"):
    """the caller's result tensor (checked: kind and number of values) or a fresh one of ``shape`` on ref's device"""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=ref.device)
    if _chk(out, name, dtype).numel() != int(np.prod(shape)):
        raise ValueError(f"{name} must hold {' * '.join(str(n) for n in shape)} values")
    return out


def _optional(n, dtype=torch.float64, **tensors):
    """outputs (or inputs) that may be None: each one given is checked for kind and for holding n values"""
    for name, t in tensors.items():
        if t is not None and _chk(t, name, dtype).numel() != n:
            raise ValueError(f"{name} must hold {n} values")


def _workspace(ws, need, ref):
    """the caller's uint8 workspace (its kind checked; its size is the C layer's to refuse) or a fresh one of ``need`` bytes"""
    if ws is None:
        return torch.empty(max(need, 1), dtype=torch.uint8, device=ref.device)   # (the caching allocator's blocks are 512-byte aligned)
    return _chk(ws, "ws", torch.uint8)


def _tables(tt_tx, tt_rx, data=None, analytic=False):
    """tt_tx [n_tx, n] and tt_rx [n_rx, n], with ``data`` also its [n_tx, n_rx, n_t] (analytic: [.., 2]) against them -> n"""
    ok = tt_tx.dim() == 2 and tt_rx.dim() == 2 and tt_tx.shape[1] == tt_rx.shape[1]
    if ok and data is not None:
        ok = data.dim() == (4 if analytic else 3) and (not analytic or data.shape[3] == 2) \
            and data.shape[0] == tt_tx.shape[0] and data.shape[1] == tt_rx.shape[0]
    if not ok:
        what = "" if data is None else ("analytic [n_tx, n_rx, n_t, 2], " if analytic else "fmc [n_tx, n_rx, n_t], ")
        raise ValueError(f"need {what}tt_tx [n_tx, n], tt_rx [n_rx, n]")
    return tt_tx.shape[1]


def _stream(t=None):
    """the current stream of the tensor's device (of the current device without a tensor)"""
    return torch.cuda.current_stream(None if t is None else t.device).cuda_stream


class ShootPlan:
    """Pre-allocated workspace + outputs for repeated forward traces of one shape (no allocation,
    no sync inside ``run`` — safe to capture in a hipGraph)."""

    def __init__(self, n_geom, n_tx, n_rays, *, want=("out8",), params: Params = None, fast=False, device="cuda"):
        self.p = _resolve(params)
        self.G, self.T, self.N = int(n_geom), int(n_tx), int(n_rays)
        self.ws_bytes = int(_lib.lib().rtus_shoot_workspace_bytes(self.N))
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=device)
        G, T, N = self.G, self.T, self.N
        shapes = dict(out8=(G, T, 8, N), tof4=(G, T, 4, N), tof=(G, T, N), land_x=(G, T, N), status=(G, T, N))
        self.out = {w: torch.empty(shapes[w], dtype=torch.uint8 if w == "status" else torch.float64, device=device)
                    for w in want}
        self.lens = self.p.lens()
        self.flags = _api._flags(fast)

    def run(self, geoms, x_a, z_a, alpha, z_f, polyline_ready=False):
        """polyline_ready: the previous ``run`` of this plan used the same ``alpha`` (RTUS_POLYLINE_READY)."""
        _chk(geoms, "geoms"); _chk(x_a, "x_a"); _chk(z_a, "z_a"); _chk(alpha, "alpha"); _chk(z_f, "z_f")
        if geoms.shape != (self.G, 2) or x_a.numel() != self.T or z_a.numel() != self.T \
                or alpha.numel() != self.N or z_f.numel() != self.N:
            raise ValueError("tensor shapes do not match the plan")
        o = self.out
        st = _lib.lib().rtus_shoot_dev(C.byref(self.lens), _p(geoms), self.G, _p(x_a), _p(z_a), self.T, _p(alpha),
                                       _p(z_f), self.N, _p(o.get("out8")), _p(o.get("tof4")), _p(o.get("tof")),
                                       _p(o.get("land_x")), _p(o.get("status")), _p(self.ws), self.ws_bytes,
                                       self.flags | (POLYLINE_READY if polyline_ready else 0), _stream())
        _lib.check(st, "rtus_shoot_dev")
        return o


class SweepPlan:
    """Pre-allocated workspace + outputs for the fused sweep (rtus_sweep_dev: forward trace + element matcher in one kernel,
    main_rt.py:464-501): first_ray i32 / hit u8 / tof_hit f64 [G, T, E], plus the per-ray arrays in ``want`` ("tof", "land_x":
    [G, T, N]).  No allocation, no sync inside ``run`` — capturable in a hipGraph."""

    def __init__(self, n_geom, n_tx, n_rays, n_rx, *, want=(), params: Params = None, fast=False, atol=1e-6, rtol=1e-5, device="cuda"):
        self.p = _resolve(params)
        self.G, self.T, self.N, self.E = int(n_geom), int(n_tx), int(n_rays), int(n_rx)
        self.ws_bytes = int(_lib.lib().rtus_sweep_workspace_bytes(self.N, self.G, self.T, self.E))
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=device)
        G, T, N, E = self.G, self.T, self.N, self.E
        self.out = {"first_ray": torch.empty((G, T, E), dtype=torch.int32, device=device),
                    "hit": torch.empty((G, T, E), dtype=torch.uint8, device=device),
                    "tof_hit": torch.empty((G, T, E), dtype=torch.float64, device=device)}
        for w in want:
            if w not in ("tof", "land_x"):
                raise ValueError(f"unknown output {w!r}")
            self.out[w] = torch.empty((G, T, N), dtype=torch.float64, device=device)
        self.lens = self.p.lens()
        self.flags = _api._flags(fast)
        self.atol, self.rtol = float(atol), float(rtol)

    def run(self, geoms, x_a, z_a, alpha, z_f, x_rx, polyline_ready=False):
        """polyline_ready: the previous ``run`` of this plan used the same ``alpha`` (RTUS_POLYLINE_READY)."""
        _chk(geoms, "geoms"); _chk(x_a, "x_a"); _chk(z_a, "z_a"); _chk(alpha, "alpha"); _chk(z_f, "z_f"); _chk(x_rx, "x_rx")
        if geoms.shape != (self.G, 2) or x_a.numel() != self.T or z_a.numel() != self.T \
                or alpha.numel() != self.N or z_f.numel() != self.N or x_rx.numel() != self.E:
            raise ValueError("tensor shapes do not match the plan")
        o = self.out
        st = _lib.lib().rtus_sweep_dev(C.byref(self.lens), _p(geoms), self.G, _p(x_a), _p(z_a), self.T, _p(alpha), _p(z_f), self.N,
                                       _p(x_rx), self.E, self.atol, self.rtol, _p(o["first_ray"]), _p(o["hit"]), _p(o["tof_hit"]),
                                       _p(o.get("tof")), _p(o.get("land_x")), _p(self.ws), self.ws_bytes,
                                       self.flags | (POLYLINE_READY if polyline_ready else 0), _stream())
        _lib.check(st, "rtus_sweep_dev")
        return o


class SolvePlan:
    """Pre-allocated workspace + outputs for repeated root-finding solves of one shape (rtus_solve_dev): no allocation,
    no sync inside ``run`` — capturable in a hipGraph.  tt / alpha_root [G, T, E]; with all_roots also tt_all / alpha_all
    [G, T, E, 4] and n_roots [G, T, E]."""

    def __init__(self, n_geom, n_tx, n_rays, n_rx, *, params: Params = None, fast=False, true_tangent=False,
                 analytic_lens=False, all_roots=False, device="cuda", one_lane=False, three_launches=False):
        self.p = _resolve(params)
        self.G, self.T, self.N, self.E = int(n_geom), int(n_tx), int(n_rays), int(n_rx)
        self.ws_bytes = int(_lib.lib().rtus_solve_workspace_bytes(self.N, self.G, self.T, self.E))
        self.ws = torch.empty(self.ws_bytes, dtype=torch.uint8, device=device)
        G, T, E = self.G, self.T, self.E
        f64 = dict(dtype=torch.float64, device=device)
        self.out = {"tt": torch.empty((G, T, E), **f64), "alpha_root": torch.empty((G, T, E), **f64)}
        if all_roots:
            self.out.update(tt_all=torch.empty((G, T, E, 4), **f64), alpha_all=torch.empty((G, T, E, 4), **f64),
                            n_roots=torch.empty((G, T, E), dtype=torch.uint8, device=device))
        self.lens = self.p.lens()
        self.flags = _api._flags(fast, true_tangent, analytic_lens) | (_api.SOLVE_ONE_LANE if one_lane else 0) | \
            (_api.SOLVE_THREE_LAUNCHES if three_launches else 0)

    def run(self, geoms, x_a, z_a, alpha, x_rx, z_land=None, polyline_ready=False):
        """polyline_ready: the previous ``run`` of this plan used the same ``alpha`` tensor contents (RTUS_POLYLINE_READY: the
        lens polyline in the workspace is kept instead of rebuilt)."""
        _chk(geoms, "geoms"); _chk(x_a, "x_a"); _chk(z_a, "z_a"); _chk(alpha, "alpha"); _chk(x_rx, "x_rx")
        if geoms.shape != (self.G, 2) or x_a.numel() != self.T or z_a.numel() != self.T \
                or alpha.numel() != self.N or x_rx.numel() != self.E:
            raise ValueError("tensor shapes do not match the plan")
        o = self.out
        st = _lib.lib().rtus_solve_dev(C.byref(self.lens), _p(geoms), self.G, _p(x_a), _p(z_a), self.T, _p(alpha), self.N,
                                       _p(x_rx), self.E, float(self.p.d if z_land is None else z_land), _p(o["tt"]),
                                       _p(o["alpha_root"]), _p(o.get("tt_all")), _p(o.get("alpha_all")), _p(o.get("n_roots")),
                                       _p(self.ws), self.ws_bytes, self.flags | (POLYLINE_READY if polyline_ready else 0), _stream())
        _lib.check(st, "rtus_solve_dev")
        return o


def match_dev(land_x, tof, x_rx, atol=1e-6, rtol=1e-5, out=None):
    """land_x/tof [rows, N], x_rx [E] -> (first_ray i32[rows,E], hit u8[rows,E], tof_hit f64[rows,E])."""
    _chk(land_x, "land_x"); _chk(tof, "tof"); _chk(x_rx, "x_rx")
    rows, N, E = land_x.shape[0], land_x.shape[1], x_rx.numel()
    if out is None:
        out = (torch.empty((rows, E), dtype=torch.int32, device=land_x.device),
               torch.empty((rows, E), dtype=torch.uint8, device=land_x.device),
               torch.empty((rows, E), dtype=torch.float64, device=land_x.device))
    first, hit, tof_hit = out
    st = _lib.lib().rtus_match_dev(_p(land_x), _p(tof), rows, N, _p(x_rx), E, float(atol), float(rtol), _p(first),
                                   _p(hit), _p(tof_hit), _stream())
    _lib.check(st, "rtus_match_dev")
    return out


def tt_layers_dev(z_if, c, xe, ze, xf, zf, out=None, iters=None, row0=0, n_rows_total=None, taup=False):
    """Fermat travel times through horizontal layers; z_if/c are small HOST sequences.

    row0 / n_rows_total: xe, ze are rows [row0, row0 + len(xe)) of a table of n_rows_total rows (rtus_tt_layers_rows_dev): with
    row0 a multiple of ``rows_per_block(n_rows_total, n_f)`` the block comes out with the bits the whole table's launch gives it."""
    z_if, c = _api._medium(z_if, c, flat=True)
    n_e, n_f = _pair(xe, ze, xf, zf)
    out = _result(out, (n_e, n_f), xe)
    if iters is not None and (n_rows_total is not None or taup):
        raise ValueError("iters is a whole-table diagnostic of the accurate tier")
    if n_rows_total is not None:
        st = _lib.lib().rtus_tt_layers_rows_dev(z_if.ctypes.data if z_if.size else None, c.ctypes.data, z_if.size, _p(xe), _p(ze),
                                                n_e, int(row0), int(n_e if n_rows_total is None else n_rows_total), _p(xf), _p(zf), n_f,
                                                _p(out), TAUP_TAIL if taup else 0, _stream())
        _lib.check(st, "rtus_tt_layers_rows_dev")
        return out
    st = _lib.lib().rtus_tt_layers_ex_dev(z_if.ctypes.data if z_if.size else None, c.ctypes.data, z_if.size, _p(xe),
                                          _p(ze), n_e, _p(xf), _p(zf), n_f, _p(out), _p(iters), TAUP_TAIL if taup else 0, _stream())
    _lib.check(st, "rtus_tt_layers_ex_dev")
    return out


def tt_layers_sorted_dev(z_if, c, xe, ze, xf, zf, out=None, ws=None, taup=False):
    """The planar table for an aperture handed over in ANY order (rtus_tt_layers_sorted_dev): sorted by (depth, position) on the
    device, every row stored where it belongs.  ``ws``: optional uint8 workspace tensor to reuse between calls."""
    z_if, c = _api._medium(z_if, c, flat=True)
    n_e, n_f = _pair(xe, ze, xf, zf)
    out = _result(out, (n_e, n_f), xe)
    need = int(_lib.lib().rtus_tt_layers_sort_workspace_bytes(n_e))
    if ws is None:                            # not _workspace: this entry has always taken ``ws`` as it comes and checked its size here
        ws = torch.empty(need, dtype=torch.uint8, device=xe.device)
    if ws.numel() < need:
        raise ValueError("ws is too small")
    st = _lib.lib().rtus_tt_layers_sorted_dev(z_if.ctypes.data if z_if.size else None, c.ctypes.data, z_if.size, _p(xe), _p(ze), n_e,
                                              _p(xf), _p(zf), n_f, _p(out), _p(ws), ws.numel(), TAUP_TAIL if taup else 0, _stream(xe))
    _lib.check(st, "rtus_tt_layers_sorted_dev")
    return out


def tt_layers3_dev(z_if, c, xe, ye, ze, xf, yf, zf, out=None):
    """Matrix arrays: Fermat travel times in three dimensions through horizontal layers (rtus_tt_layers3_dev) -> [n_e, n_f];
    z_if/c are small HOST sequences, the six coordinate vectors float64 CUDA tensors on one device.  Each entry depends on its own
    pair only, so a slice of the elements or of the points gives that slice of the table bit for bit.  Runs on the current stream
    of the tensors' device; with ``out`` given nothing is allocated, and nothing synchronises (capturable)."""
    z_if, c = _api._medium(z_if, c, flat=True)
    n_e, n_f = _pair(xe, ze, xf, zf)
    if _chk(ye, "ye").numel() != n_e or _chk(yf, "yf").numel() != n_f:
        raise ValueError("xe/ye/ze and xf/yf/zf must pair up")
    out = _result(out, (n_e, n_f), xe)
    if any(t.device != xe.device for t in (ye, ze, xf, yf, zf, out)):
        raise ValueError("xe, ye, ze, xf, yf, zf and out must be on one device")
    st = _lib.lib().rtus_tt_layers3_dev(z_if.ctypes.data if z_if.size else None, c.ctypes.data, z_if.size, _p(xe), _p(ye), _p(ze), n_e,
                                        _p(xf), _p(yf), _p(zf), n_f, _p(out), 0, _stream(xe))
    _lib.check(st, "rtus_tt_layers3_dev")
    return out


def rows_per_block(n_rows_total, n_f, dtype=torch.float64):
    """Rows the table kernels solve per workgroup for a table of this size: shard boundaries that are multiples of it
    reproduce the one-launch table bit for bit (rtus_table_rows_per_block)."""
    r = _lib.lib().rtus_table_rows_per_block(int(n_rows_total), int(n_f), 8 if dtype == torch.float64 else 4)
    if r < 0:
        _lib.check(r, "rtus_table_rows_per_block")
    return int(r)


def _lens_rows(kind, last, xe, ze, xf, zf, out, params, alpha_lo, alpha_hi, row0, n_rows_total):
    """rtus_tt_lens[_f32]_{rows,stats}_dev: one argument list, ``last`` being alpha_out (rows) or the counters (stats) -> n_e, n_f"""
    p = _resolve(params)
    f64 = xe.dtype == torch.float64
    n_e, n_f = _pair(xe, ze, xf, zf, xe.dtype)
    if _chk(out, "out", xe.dtype).numel() != n_e * n_f:
        raise ValueError("out must hold n_e * n_f values")
    fn = getattr(_lib.lib(), f"rtus_tt_lens{'' if f64 else '_f32'}_{kind}_dev")
    lens = p.lens()
    st = fn(C.byref(lens), -_api.ALPHA_MAX if alpha_lo is None else float(alpha_lo), _api.ALPHA_MAX if alpha_hi is None else float(alpha_hi),
            _p(xe), _p(ze), n_e, int(row0), int(n_e if n_rows_total is None else n_rows_total), _p(xf), _p(zf), n_f, _p(out), _p(last),
            _stream())
    _lib.check(st, f"rtus_tt_lens_{kind}_dev")
    return n_e, n_f


def tt_lens_rows_dev(xe, ze, xf, zf, out, *, params: Params = None, alpha_lo=None, alpha_hi=None, row0=0, n_rows_total=None):
    """Curved-lens table rows [row0, row0 + len(xe)) of an n_rows_total-row table, fp64 or fp32 by the tensors' dtype."""
    _lens_rows("rows", None, xe, ze, xf, zf, out, params, alpha_lo, alpha_hi, row0, n_rows_total)
    return out


def tt_lens_stats_dev(xe, ze, xf, zf, out, *, params: Params = None, alpha_lo=None, alpha_hi=None, row0=0, n_rows_total=None):
    """tt_lens_rows_dev + how the rows were solved (rtus_tt_lens[_f32]_stats_dev) -> (out, dict of wave-element counts)."""
    stats = torch.zeros(5, dtype=torch.int64, device=xe.device)
    n_e, n_f = _lens_rows("stats", stats, xe, ze, xf, zf, out, params, alpha_lo, alpha_hi, row0, n_rows_total)
    v = [int(x) for x in stats.cpu()]
    return out, dict(t_only=v[0], one_evaluation=v[1], iterated=v[2], scanned=v[3], iteration_evaluations=v[4],
                     wave_elements=n_e * 4 * ((n_f + 255) // 256))     # waves launched per row: whole workgroups of 256 targets


def tt_layers_batch_dev(z_if, c, xe, ze, xf, zf, out=None, taup=False):
    """B independent problems of one shape and one medium in ONE launch (rtus_tt_layers_batch_ex_dev; taup: the faster accuracy tier).

    xe/ze: [B, n_e] or [n_e] (one aperture shared by all problems); xf/zf: [B, n_f] or [n_f] (shared) -> tt [B, n_e, n_f].
    At least one of the two must carry the batch dimension."""
    z_if, c = _api._medium(z_if, c, flat=True)
    for t, n in ((xe, "xe"), (ze, "ze"), (xf, "xf"), (zf, "zf")):
        _chk(t, n)
    if xe.shape != ze.shape or xf.shape != zf.shape or xe.dim() not in (1, 2) or xf.dim() not in (1, 2):
        raise ValueError("xe/ze and xf/zf must pair up, as [B, n] or [n]")
    B = xe.shape[0] if xe.dim() == 2 else (xf.shape[0] if xf.dim() == 2 else None)
    if B is None or (xe.dim() == 2 and xf.dim() == 2 and xe.shape[0] != xf.shape[0]):
        raise ValueError("need a batch dimension on xe/ze and / or xf/zf (equal when on both)")
    n_e, n_f = xe.shape[-1], xf.shape[-1]
    out = _result(out, (B, n_e, n_f), xe)
    st = _lib.lib().rtus_tt_layers_batch_ex_dev(z_if.ctypes.data if z_if.size else None, c.ctypes.data, z_if.size, _p(xe), _p(ze),
                                                n_e, n_e if xe.dim() == 2 else 0, _p(xf), _p(zf), n_f,
                                                n_f if xf.dim() == 2 else 0, _p(out), n_e * n_f, B, TAUP_TAIL if taup else 0, _stream())
    _lib.check(st, "rtus_tt_layers_batch_ex_dev")
    return out


def tt_surface_dev(x0, dx, zs, c1, c2, xe, ze, xf, zf, out=None, x_entry=None):
    """Travel times through one curved interface (rtus_tt_surface_dev; api.travel_time_surface's definition) on float64 CUDA
    tensors -> out [n_e, n_f] (and x_entry [n_e, n_f] when a tensor is given for it).  The spline's workspace is allocated here;
    asynchronous on the current stream."""
    _chk(zs, "zs")
    n_e, n_f = _pair(xe, ze, xf, zf)
    out = _result(out, (n_e, n_f), xe)
    _optional(n_e * n_f, x_entry=x_entry)
    need = int(_lib.lib().rtus_tt_surface_workspace_bytes(zs.numel()))
    ws = _workspace(None, need, xe)
    st = _lib.lib().rtus_tt_surface_dev(float(x0), float(dx), _p(zs), zs.numel(), float(c1), float(c2), _p(xe), _p(ze), n_e, _p(xf),
                                        _p(zf), n_f, _p(out), _p(x_entry), _p(ws), need, _stream(xe))
    _lib.check(st, "rtus_tt_surface_dev")
    return out


def tt_surface_aniso_dev(x0, dx, zs, c1, slowness, xe, ze, xf, zf, out=None, x_entry=None):
    """Travel times through one curved interface into an anisotropic part (rtus_tt_aniso_surface_dev;
    aniso.travel_time_surface_aniso's definition) on float64 CUDA tensors -> out [n_e, n_f] (and x_entry [n_e, n_f] when a tensor
    is given for it).  ``slowness`` = (a, b): host vectors, the group slowness's series.  The spline's workspace is allocated here;
    asynchronous on the current stream."""
    from .aniso import _series
    _chk(zs, "zs")
    a, b, K = _series(slowness)
    n_e, n_f = _pair(xe, ze, xf, zf)
    out = _result(out, (n_e, n_f), xe)
    _optional(n_e * n_f, x_entry=x_entry)
    need = int(_lib.lib().rtus_tt_surface_workspace_bytes(zs.numel()))
    ws = _workspace(None, need, xe)
    st = _lib.lib().rtus_tt_aniso_surface_dev(float(x0), float(dx), _p(zs), zs.numel(), float(c1), a.ctypes.data, b.ctypes.data, K,
                                              _p(xe), _p(ze), n_e, _p(xf), _p(zf), n_f, _p(out), _p(x_entry), _p(ws), need, _stream(xe))
    _lib.check(st, "rtus_tt_aniso_surface_dev")
    return out


def tt_aniso_dev(slowness, xe, ze, xf, zf, out=None):
    """Contact travel times inside an anisotropic part (rtus_tt_aniso_direct_dev; aniso.travel_time_aniso's definition) on float64
    CUDA tensors -> out [n_e, n_f].  ``slowness`` = (a, b): host vectors.  No allocation beyond ``out``; asynchronous on the
    current stream."""
    from .aniso import _series
    a, b, K = _series(slowness)
    n_e, n_f = _pair(xe, ze, xf, zf)
    out = _result(out, (n_e, n_f), xe)
    st = _lib.lib().rtus_tt_aniso_direct_dev(a.ctypes.data, b.ctypes.data, K, _p(xe), _p(ze), n_e, _p(xf), _p(zf), n_f, _p(out),
                                             _stream(xe))
    _lib.check(st, "rtus_tt_aniso_direct_dev")
    return out


def focal_delays_dev(tt, out=None):
    """delays[e, f] = max_e' tt[e', f] - tt[e, f] on device (NaN-aware); ``out`` may be ``tt`` itself."""
    _chk(tt, "tt")
    if tt.dim() != 2:
        raise ValueError("tt must be [n_elem, n_focal]")
    if out is None:
        out = torch.empty_like(tt)
    _chk(out, "out")
    if out.shape != tt.shape:
        raise ValueError("out has the wrong shape")
    st = _lib.lib().rtus_focal_delays_dev(_p(tt), tt.shape[0], tt.shape[1], _p(out), _stream())
    _lib.check(st, "rtus_focal_delays_dev")
    return out


def tfm_dev(fmc, fs, tt_tx, tt_rx=None, t0=0.0, out=None):
    """TFM delay-and-sum on device: fmc float32 [n_tx, n_rx, n_t], tt_tx [n_tx, n_f], tt_rx [n_rx, n_f] (default: tt_tx)
    -> image float32 [n_f].  tt_* may be row blocks / column slices of a larger table as long as they are contiguous."""
    _chk(fmc, "fmc", torch.float32); _chk(tt_tx, "tt_tx")
    tt_rx = tt_tx if tt_rx is None else _chk(tt_rx, "tt_rx")
    n_f = _tables(tt_tx, tt_rx, fmc)
    out = _result(out, (n_f,), fmc, torch.float32)
    if not (out.device == fmc.device == tt_tx.device == tt_rx.device):
        raise ValueError("out must be on the device of fmc / tt_tx / tt_rx")
    st = _lib.lib().rtus_tfm_dev(_p(fmc), fmc.shape[0], fmc.shape[1], fmc.shape[2], float(fs), float(t0), _p(tt_tx), _p(tt_rx), n_f,
                                 _p(out), _stream(fmc))
    _lib.check(st, "rtus_tfm_dev")
    return out


def fmc_analytic_dev(fmc, n_taps=63, out=None):
    """Analytic FMC on device (rtus_fmc_analytic_dev; api.fmc_analytic's definition): fmc float32 [n_tx, n_rx, n_t] -> out float32
    [n_tx, n_rx, n_t, 2] (real, imaginary), which must not overlap fmc.  Asynchronous on the current stream."""
    _chk(fmc, "fmc", torch.float32)
    if fmc.dim() != 3:
        raise ValueError("fmc must be [n_tx, n_rx, n_t]")
    out = _result(out, (*fmc.shape, 2), fmc, torch.float32)
    if out.device != fmc.device:
        raise ValueError("out must be on the device of fmc")
    st = _lib.lib().rtus_fmc_analytic_dev(_p(fmc), fmc.shape[0], fmc.shape[1], fmc.shape[2], int(n_taps), _p(out), _stream(fmc))
    _lib.check(st, "rtus_fmc_analytic_dev")
    return out


def surface_find_dev(analytic, fs, xe, ze, c1, x0, dx, n_s, z_lo, dz, n_z, t0=0.0, z_peak=None, amp=None, image=None):
    """Couplant envelope image and column peak on device (rtus_surface_find_dev; include/rtus.h): analytic float32
    [n_e, n_e, n_t, 2], xe / ze float64 [n_e] -> (z_peak float64 [n_s], amp float32 [n_s]); ``image``: an optional float32
    [n_s, n_z] tensor that receives the envelope image.  Outputs not given are allocated here; asynchronous on the current
    stream (capturable with pre-allocated outputs)."""
    _chk(analytic, "analytic", torch.float32); _chk(xe, "xe"); _chk(ze, "ze")
    if analytic.dim() != 4 or analytic.shape[0] != analytic.shape[1] or analytic.shape[3] != 2:
        raise ValueError("analytic must be [n_e, n_e, n_t, 2]")
    n_e, n_t, n_s, n_z = analytic.shape[0], analytic.shape[2], int(n_s), int(n_z)
    if xe.numel() != n_e or ze.numel() != n_e:
        raise ValueError("xe / ze must hold one position per element")
    z_peak = _result(z_peak, (n_s,), analytic, name="z_peak")
    amp = _result(amp, (n_s,), analytic, torch.float32, "amp")
    _optional(n_s * n_z, torch.float32, image=image)
    st = _lib.lib().rtus_surface_find_dev(_p(analytic), n_e, n_t, float(fs), float(t0), _p(xe), _p(ze), float(c1), float(x0), float(dx),
                                          n_s, float(z_lo), float(dz), n_z, _p(z_peak), _p(amp), _p(image), _stream(analytic))
    _lib.check(st, "rtus_surface_find_dev")
    return z_peak, amp


def tfm_analytic_dev(analytic, fs, tt_tx, tt_rx=None, t0=0.0, out=None, cf=None):
    """Envelope TFM on device (rtus_tfm_analytic_dev; api.tfm_analytic's definition): analytic float32 [n_tx, n_rx, n_t, 2] (as
    fmc_analytic_dev makes it), tt_tx [n_tx, n_f], tt_rx [n_rx, n_f] (default: tt_tx) -> out float32 [n_f, 2] (the complex sum);
    ``cf``: an optional float32 [n_f] tensor that receives the coherence factor (then -> (out, cf)).  Asynchronous on the current
    stream (capturable with pre-allocated outputs)."""
    _chk(analytic, "analytic", torch.float32); _chk(tt_tx, "tt_tx")
    tt_rx = tt_tx if tt_rx is None else _chk(tt_rx, "tt_rx")
    n_f = _tables(tt_tx, tt_rx, analytic, analytic=True)
    out = _result(out, (n_f, 2), analytic, torch.float32)
    _optional(n_f, torch.float32, cf=cf)
    if not (out.device == analytic.device == tt_tx.device == tt_rx.device and (cf is None or cf.device == analytic.device)):
        raise ValueError("analytic, tt_tx, tt_rx, out and cf must be on one device")
    st = _lib.lib().rtus_tfm_analytic_dev(_p(analytic), analytic.shape[0], analytic.shape[1], analytic.shape[2], float(fs), float(t0),
                                          _p(tt_tx), _p(tt_rx), n_f, _p(out), _p(cf), _stream(analytic))
    _lib.check(st, "rtus_tfm_analytic_dev")
    return out if cf is None else (out, cf)


def _f_demod(f_demod, fs):
    """0 <= f_demod < fs / 2, finite (api.tfm_iq's rule) -> float"""
    f_demod, fs = float(f_demod), float(fs)
    if not (f_demod == f_demod and fs == fs and 0.0 <= f_demod < 0.5 * fs):
        raise ValueError(f"f_demod must be finite with 0 <= f_demod < fs / 2 (got {f_demod!r} at fs = {fs!r})")
    return f_demod


def tfm_iq_dev(analytic, fs, f_demod, tt_tx, tt_rx=None, t0=0.0, out=None, cf=None):
    """Envelope TFM with carrier-aware interpolation on device (rtus_tfm_iq_dev; api.tfm_iq's definition): tfm_analytic_dev's
    tensors and returns, ``f_demod`` [Hz] the carrier frequency, 0 <= f_demod < fs / 2 (0: tfm_analytic_dev's bits).  Asynchronous
    on the current stream (capturable with pre-allocated outputs)."""
    f_demod = _f_demod(f_demod, fs)
    _chk(analytic, "analytic", torch.float32); _chk(tt_tx, "tt_tx")
    tt_rx = tt_tx if tt_rx is None else _chk(tt_rx, "tt_rx")
    n_f = _tables(tt_tx, tt_rx, analytic, analytic=True)
    out = _result(out, (n_f, 2), analytic, torch.float32)
    _optional(n_f, torch.float32, cf=cf)
    if not (out.device == analytic.device == tt_tx.device == tt_rx.device and (cf is None or cf.device == analytic.device)):
        raise ValueError("analytic, tt_tx, tt_rx, out and cf must be on one device")
    st = _lib.lib().rtus_tfm_iq_dev(_p(analytic), analytic.shape[0], analytic.shape[1], analytic.shape[2], float(fs), float(t0), f_demod,
                                    _p(tt_tx), _p(tt_rx), n_f, _p(out), _p(cf), _stream(analytic))
    _lib.check(st, "rtus_tfm_iq_dev")
    return out if cf is None else (out, cf)


def fmc_pack_frames_dev(stack, out=None):
    """A frame-major RF stack on device, float32 [n_frames, n_tx, n_rx, n_t] -> its packed layout float32
    [n_pairs, n_tx, n_rx, n_t, 2] (rtus_fmc_pack_frames_dev; api.frames_pack's definition: frame 2 p and frame 2 p + 1 interleaved in
    pair p, the missing partner of an odd stack +0.0).  ``out`` must not overlap ``stack``.  Asynchronous on the current stream
    (capturable with a pre-allocated output)."""
    _chk(stack, "stack", torch.float32)
    if stack.dim() != 4 or stack.shape[0] < 1:
        raise ValueError("stack must be [n_frames, n_tx, n_rx, n_t] with at least one frame")
    n_frames, n_tx, n_rx, n_t = stack.shape
    out = _result(out, ((n_frames + 1) // 2, n_tx, n_rx, n_t, 2), stack, torch.float32)
    if out.device != stack.device:
        raise ValueError("out must be on the device of stack")
    st = _lib.lib().rtus_fmc_pack_frames_dev(_p(stack), n_frames, n_tx, n_rx, n_t, _p(out), _stream(stack))
    _lib.check(st, "rtus_fmc_pack_frames_dev")
    return out


def tfm_frames_dev(packed, n_frames, fs, tt_tx, tt_rx=None, t0=0.0, out=None):
    """TFM over a stack of RF frames on device (rtus_tfm_frames_dev; api.tfm_frames' definition): ``packed`` float32
    [n_pairs, n_tx, n_rx, n_t, 2] as fmc_pack_frames_dev makes it, ``n_frames`` = 2 n_pairs or 2 n_pairs - 1 (the last pair then
    holds one frame), tt_tx [n_tx, n_f], tt_rx [n_rx, n_f] (default: tt_tx) -> out float32 [n_frames, n_f]; row k has tfm_dev's bits
    on frame k.  One call, a few launches; asynchronous on the current stream (capturable with a pre-allocated output)."""
    _chk(packed, "packed", torch.float32); _chk(tt_tx, "tt_tx")
    tt_rx = tt_tx if tt_rx is None else _chk(tt_rx, "tt_rx")
    n_frames = int(n_frames)
    if packed.dim() != 5 or packed.shape[4] != 2 or packed.shape[0] < 1 or (n_frames + 1) // 2 != packed.shape[0] or n_frames < 1:
        raise ValueError("need packed [n_pairs, n_tx, n_rx, n_t, 2] and n_frames = 2 n_pairs or 2 n_pairs - 1")
    n_f = _tables(tt_tx, tt_rx, packed[0], analytic=True)
    out = _result(out, (n_frames, n_f), packed, torch.float32)
    if not (out.device == packed.device == tt_tx.device == tt_rx.device):
        raise ValueError("out must be on the device of packed / tt_tx / tt_rx")
    st = _lib.lib().rtus_tfm_frames_dev(_p(packed), n_frames, packed.shape[1], packed.shape[2], packed.shape[3], float(fs), float(t0),
                                        _p(tt_tx), _p(tt_rx), n_f, _p(out), _stream(packed))
    _lib.check(st, "rtus_tfm_frames_dev")
    return out


def fmc_pack_frames_i16_dev(stack, out=None):
    """A frame-major int16 stack on device, int16 [n_frames, n_tx, n_rx, n_t] -> its packed layout int16
    [n_quads, n_tx, n_rx, n_t, 4] (rtus_fmc_pack_frames_i16_dev; api.frames_pack_i16's definition: frames 4 q .. 4 q + 3 interleaved
    in quad q, the planes of absent frames 0).  ``out`` must not overlap ``stack``.  Asynchronous on the current stream (capturable
    with a pre-allocated output)."""
    _chk(stack, "stack", torch.int16)
    if stack.dim() != 4 or stack.shape[0] < 1:
        raise ValueError("stack must be [n_frames, n_tx, n_rx, n_t] with at least one frame")
    n_frames, n_tx, n_rx, n_t = stack.shape
    out = _result(out, ((n_frames + 3) // 4, n_tx, n_rx, n_t, 4), stack, torch.int16)
    if out.device != stack.device:
        raise ValueError("out must be on the device of stack")
    st = _lib.lib().rtus_fmc_pack_frames_i16_dev(_p(stack), n_frames, n_tx, n_rx, n_t, _p(out), _stream(stack))
    _lib.check(st, "rtus_fmc_pack_frames_i16_dev")
    return out


def tfm_frames_i16_dev(packed, n_frames, fs, tt_tx, tt_rx=None, t0=0.0, out=None):
    """TFM over a stack of int16 frames on device (rtus_tfm_frames_i16_dev; api.tfm_frames' definition): ``packed`` int16
    [n_quads, n_tx, n_rx, n_t, 4] as fmc_pack_frames_i16_dev makes it, ``n_frames`` in [4 n_quads - 3, 4 n_quads] (the last quad then
    holds fewer than four frames), tt_tx [n_tx, n_f], tt_rx [n_rx, n_f] (default: tt_tx) -> out float32 [n_frames, n_f]; row k has
    tfm_dev's bits on frame k converted to float32.  One call, a few launches; asynchronous on the current stream (capturable with a
    pre-allocated output)."""
    _chk(packed, "packed", torch.int16); _chk(tt_tx, "tt_tx")
    tt_rx = tt_tx if tt_rx is None else _chk(tt_rx, "tt_rx")
    n_frames = int(n_frames)
    if packed.dim() != 5 or packed.shape[4] != 4 or packed.shape[0] < 1 or (n_frames + 3) // 4 != packed.shape[0] or n_frames < 1:
        raise ValueError("need packed [n_quads, n_tx, n_rx, n_t, 4] and n_frames in [4 n_quads - 3, 4 n_quads]")
    ok = tt_tx.dim() == 2 and tt_rx.dim() == 2 and tt_tx.shape[1] == tt_rx.shape[1] \
        and packed.shape[1] == tt_tx.shape[0] and packed.shape[2] == tt_rx.shape[0]
    if not ok:
        raise ValueError("need packed [n_quads, n_tx, n_rx, n_t, 4], tt_tx [n_tx, n], tt_rx [n_rx, n]")
    n_f = tt_tx.shape[1]
    out = _result(out, (n_frames, n_f), packed, torch.float32)
    if not (out.device == packed.device == tt_tx.device == tt_rx.device):
        raise ValueError("out must be on the device of packed / tt_tx / tt_rx")
    st = _lib.lib().rtus_tfm_frames_i16_dev(_p(packed), n_frames, packed.shape[1], packed.shape[2], packed.shape[3], float(fs), float(t0),
                                            _p(tt_tx), _p(tt_rx), n_f, _p(out), _stream(packed))
    _lib.check(st, "rtus_tfm_frames_i16_dev")
    return out


def tfm_analytic_frames_dev(analytic, fs, tt_tx, tt_rx=None, t0=0.0, f_demod=0.0, out=None, cf=None):
    """Envelope TFM over a stack of analytic frames on device (rtus_tfm_analytic_frames_dev): ``analytic`` float32
    [n_frames, n_tx, n_rx, n_t, 2] (fmc_analytic_dev on the stack viewed as [n_frames n_tx, n_rx, n_t] makes it), tt_tx [n_tx, n_f],
    tt_rx [n_rx, n_f] (default: tt_tx) -> out float32 [n_frames, n_f, 2]; ``cf``: an optional float32 [n_frames, n_f] tensor that
    receives the coherence factors (then -> (out, cf)).  ``f_demod`` = 0: row k has tfm_analytic_dev's bits on frame k; > 0 (below
    fs / 2): tfm_iq_dev's.  One call, a few launches; asynchronous on the current stream (capturable with pre-allocated outputs)."""
    f_demod = _f_demod(f_demod, fs)
    _chk(analytic, "analytic", torch.float32); _chk(tt_tx, "tt_tx")
    tt_rx = tt_tx if tt_rx is None else _chk(tt_rx, "tt_rx")
    if analytic.dim() != 5 or analytic.shape[0] < 1:
        raise ValueError("analytic must be [n_frames, n_tx, n_rx, n_t, 2] with at least one frame")
    n_frames = analytic.shape[0]
    n_f = _tables(tt_tx, tt_rx, analytic[0], analytic=True)
    out = _result(out, (n_frames, n_f, 2), analytic, torch.float32)
    _optional(n_frames * n_f, torch.float32, cf=cf)
    if not (out.device == analytic.device == tt_tx.device == tt_rx.device and (cf is None or cf.device == analytic.device)):
        raise ValueError("analytic, tt_tx, tt_rx, out and cf must be on one device")
    st = _lib.lib().rtus_tfm_analytic_frames_dev(_p(analytic), n_frames, analytic.shape[1], analytic.shape[2], analytic.shape[3],
                                                 float(fs), float(t0), f_demod, _p(tt_tx), _p(tt_rx), n_f, _p(out), _p(cf),
                                                 _stream(analytic))
    _lib.check(st, "rtus_tfm_analytic_frames_dev")
    return out if cf is None else (out, cf)


def _hmc_tables(tt_tx, tt_rx, data, analytic):
    """a half-matrix capture [n_pairs, n_t] (analytic: [.., 2]) against tt_tx, tt_rx [n_e, n] both -> (n_e, n)"""
    ok = tt_tx.dim() == 2 and tt_rx.dim() == 2 and tt_tx.shape == tt_rx.shape \
        and data.dim() == (3 if analytic else 2) and (not analytic or data.shape[2] == 2)
    n_e = tt_tx.shape[0] if ok else 0
    if not ok or n_e < 1 or n_e * (n_e + 1) // 2 != data.shape[0]:
        what = "analytic [n_pairs, n_t, 2]" if analytic else "hmc [n_pairs, n_t]"
        raise ValueError(f"need {what} with n_pairs = n_e (n_e + 1) / 2, tt_tx [n_e, n], tt_rx [n_e, n]")
    return n_e, tt_tx.shape[1]


def tfm_hmc_dev(hmc, fs, tt_tx, tt_rx=None, t0=0.0, out=None):
    """TFM over a half-matrix capture on device (rtus_tfm_hmc_dev; api.tfm_hmc's definition): hmc float32 [n_pairs, n_t], tt_tx /
    tt_rx [n_e, n_f] (default: tt_tx — one table: every record gathered once) -> image float32 [n_f].  Asynchronous on the
    current stream (capturable with a pre-allocated output)."""
    _chk(hmc, "hmc", torch.float32); _chk(tt_tx, "tt_tx")
    tt_rx = tt_tx if tt_rx is None else _chk(tt_rx, "tt_rx")
    n_e, n_f = _hmc_tables(tt_tx, tt_rx, hmc, False)
    out = _result(out, (n_f,), hmc, torch.float32)
    if not (out.device == hmc.device == tt_tx.device == tt_rx.device):
        raise ValueError("out must be on the device of hmc / tt_tx / tt_rx")
    st = _lib.lib().rtus_tfm_hmc_dev(_p(hmc), n_e, hmc.shape[1], float(fs), float(t0), _p(tt_tx), _p(tt_rx), n_f, _p(out), _stream(hmc))
    _lib.check(st, "rtus_tfm_hmc_dev")
    return out


def _tfm_frames_hmc_dev(entry, per, dtype, packed, n_frames, fs, tt_tx, tt_rx, t0, out):
    """tfm_frames_hmc_i16_dev (per = 4 frames a block) and tfm_frames_hmc_dev (per = 2)"""
    _chk(packed, "packed", dtype); _chk(tt_tx, "tt_tx")
    tt_rx = tt_tx if tt_rx is None else _chk(tt_rx, "tt_rx")
    n_frames = int(n_frames)
    what = f"packed [n_blocks, n_pairs, n_t, {per}]"
    if packed.dim() != 4 or packed.shape[3] != per or packed.shape[0] < 1 or (n_frames + per - 1) // per != packed.shape[0] or n_frames < 1:
        raise ValueError(f"need {what} and n_frames in [{per} n_blocks - {per - 1}, {per} n_blocks]")
    ok = tt_tx.dim() == 2 and tt_rx.dim() == 2 and tt_tx.shape == tt_rx.shape
    n_e = tt_tx.shape[0] if ok else 0
    if not ok or n_e < 1 or n_e * (n_e + 1) // 2 != packed.shape[1]:
        raise ValueError(f"need {what} with n_pairs = n_e (n_e + 1) / 2, tt_tx [n_e, n], tt_rx [n_e, n]")
    n_f = tt_tx.shape[1]
    out = _result(out, (n_frames, n_f), packed, torch.float32)
    if not (out.device == packed.device == tt_tx.device == tt_rx.device):
        raise ValueError("out must be on the device of packed / tt_tx / tt_rx")
    st = getattr(_lib.lib(), entry)(_p(packed), n_frames, n_e, packed.shape[2], float(fs), float(t0), _p(tt_tx), _p(tt_rx), n_f, _p(out),
                                    _stream(packed))
    _lib.check(st, entry)
    return out


def tfm_frames_hmc_i16_dev(packed, n_frames, fs, tt_tx, tt_rx=None, t0=0.0, out=None):
    """TFM over a stack of int16 half-matrix frames on device (rtus_tfm_frames_hmc_i16_dev; api.tfm_frames(hmc=True)'s definition):
    ``packed`` int16 [n_quads, n_pairs, n_t, 4] — fmc_pack_frames_i16_dev(stack.view(n_frames, 1, n_pairs, n_t))[:, 0] makes it —
    ``n_frames`` in [4 n_quads - 3, 4 n_quads], tt_tx / tt_rx [n_e, n_f] (default: tt_tx — one table: every record gathered once) ->
    out float32 [n_frames, n_f]; row k has tfm_hmc_dev's bits on frame k converted to float32.  One call, a few launches;
    asynchronous on the current stream (capturable with a pre-allocated output)."""
    return _tfm_frames_hmc_dev("rtus_tfm_frames_hmc_i16_dev", 4, torch.int16, packed, n_frames, fs, tt_tx, tt_rx, t0, out)


def tfm_frames_hmc_dev(packed, n_frames, fs, tt_tx, tt_rx=None, t0=0.0, out=None):
    """TFM over a stack of float32 half-matrix frames on device (rtus_tfm_frames_hmc_dev): ``packed`` float32
    [n_fpairs, n_pairs, n_t, 2] — fmc_pack_frames_dev(stack.view(n_frames, 1, n_pairs, n_t))[:, 0] makes it — ``n_frames`` =
    2 n_fpairs or 2 n_fpairs - 1, tables as tfm_frames_hmc_i16_dev -> out float32 [n_frames, n_f]; row k has tfm_hmc_dev's bits on
    frame k.  Asynchronous on the current stream (capturable with a pre-allocated output)."""
    return _tfm_frames_hmc_dev("rtus_tfm_frames_hmc_dev", 2, torch.float32, packed, n_frames, fs, tt_tx, tt_rx, t0, out)


def fmc_analytic_i16_dev(fmc, n_taps=63, out=None):
    """fmc_analytic_dev on int16 samples (rtus_fmc_analytic_i16_dev): fmc int16 [n_tx, n_rx, n_t] -> out float32 [n_tx, n_rx, n_t, 2]
    with fmc_analytic_dev's bits on the samples as float32.  Asynchronous on the current stream."""
    _chk(fmc, "fmc", torch.int16)
    if fmc.dim() != 3:
        raise ValueError("fmc must be [n_tx, n_rx, n_t]")
    out = _result(out, (*fmc.shape, 2), fmc, torch.float32)
    if out.device != fmc.device:
        raise ValueError("out must be on the device of fmc")
    st = _lib.lib().rtus_fmc_analytic_i16_dev(_p(fmc), fmc.shape[0], fmc.shape[1], fmc.shape[2], int(n_taps), _p(out), _stream(fmc))
    _lib.check(st, "rtus_fmc_analytic_i16_dev")
    return out


def fmc_hilbert_pairs_i16_dev(stack, n_taps=63, out=None):
    """The Hilbert planes of a frame-major int16 stack [n_frames, n_scans, n_t], pair-packed (rtus_fmc_hilbert_pairs_i16_dev;
    api.frames_pack's layout on the imaginary parts) -> out float32 [n_fpairs, n_scans, n_t, 2]: what tfm_frames_hmc_dev reads, plane c of pair p the
    imaginary part of fmc_analytic_i16_dev of frame 2 p + c, the absent frame of an odd stack +0.0.  Asynchronous on the current
    stream (capturable with a pre-allocated output)."""
    _chk(stack, "stack", torch.int16)
    if stack.dim() != 3 or stack.shape[0] < 1:
        raise ValueError("stack must be [n_frames, n_scans, n_t] with at least one frame")
    n_frames, n_scans, n_t = stack.shape
    out = _result(out, ((n_frames + 1) // 2, n_scans, n_t, 2), stack, torch.float32)
    if out.device != stack.device:
        raise ValueError("out must be on the device of stack")
    st = _lib.lib().rtus_fmc_hilbert_pairs_i16_dev(_p(stack), n_frames, n_scans, n_t, int(n_taps), _p(out), _stream(stack))
    _lib.check(st, "rtus_fmc_hilbert_pairs_i16_dev")
    return out


def tfm_envelope_frames_hmc_workspace_bytes(n_frames, n_e, n_t, n_f, *, i16, f_demod=0.0, want_cf=False, magnitude=False):
    """the bytes of the ``ws`` tensor of tfm_envelope_frames_hmc[_i16]_dev for these sizes (0: refused)"""
    return int(_lib.lib().rtus_tfm_envelope_frames_hmc_workspace_bytes(int(n_frames), int(n_e), int(n_t), int(n_f), int(bool(i16)),
                                                                        float(f_demod), int(bool(want_cf)),
                                                                        _api.ENV_MAGNITUDE if magnitude else 0))


def _tfm_envelope_frames_hmc_dev(entry, dtype, stack, fs, tt_tx, tt_rx, t0, n_taps, f_demod, magnitude, out, cf, ws):
    """tfm_envelope_frames_hmc_i16_dev (int16 frames) and tfm_envelope_frames_hmc_dev (float32 frames)"""
    f_demod = _f_demod(f_demod, fs)
    _chk(stack, "stack", dtype); _chk(tt_tx, "tt_tx")
    tt_rx = tt_tx if tt_rx is None else _chk(tt_rx, "tt_rx")
    if stack.dim() != 3 or stack.shape[0] < 1:
        raise ValueError("stack must be [n_frames, n_pairs, n_t] with at least one frame")
    n_frames, n_t = stack.shape[0], stack.shape[2]
    n_e, n_f = _hmc_tables(tt_tx, tt_rx, stack[0], False)
    out = _result(out, (n_frames, n_f) if magnitude else (n_frames, n_f, 2), stack, torch.float32)
    _optional(n_frames * n_f, torch.float32, cf=cf)
    need = tfm_envelope_frames_hmc_workspace_bytes(n_frames, n_e, n_t, n_f, i16=dtype == torch.int16, f_demod=f_demod,
                                                   want_cf=cf is not None, magnitude=magnitude)
    ws = _workspace(ws, need, stack)
    if not (out.device == stack.device == tt_tx.device == tt_rx.device == ws.device and (cf is None or cf.device == stack.device)):
        raise ValueError("stack, tt_tx, tt_rx, out, cf and ws must be on one device")
    st = getattr(_lib.lib(), entry)(_p(stack), n_frames, n_e, n_t, int(n_taps), float(fs), float(t0), f_demod, _p(tt_tx), _p(tt_rx), n_f,
                                    _api.ENV_MAGNITUDE if magnitude else 0, _p(out), _p(cf), _p(ws), ws.numel(), _stream(stack))
    _lib.check(st, entry)
    return out if cf is None else (out, cf)


def tfm_envelope_frames_hmc_i16_dev(stack, fs, tt_tx, tt_rx=None, t0=0.0, n_taps=63, f_demod=0.0, magnitude=False, out=None, cf=None,
                                    ws=None):
    """Envelope TFM over a stack of int16 half-matrix frames on device (rtus_tfm_envelope_frames_hmc_i16_dev;
    api.tfm_envelope_frames' definition): ``stack`` int16 [n_frames, n_pairs, n_t], FRAME-MAJOR (the packing happens in ``ws``),
    tt_tx / tt_rx [n_e, n_f] (default: tt_tx — one table) -> out float32 [n_frames, n_f, 2], or [n_frames, n_f] with
    ``magnitude=True``; ``cf``: an optional float32 [n_frames, n_f] tensor that receives the coherence factors (then -> (out, cf)).
    ``ws``: a uint8 workspace of tfm_envelope_frames_hmc_workspace_bytes(...) bytes, allocated here when None.  Asynchronous on the
    current stream (capturable with pre-allocated out, cf and ws)."""
    return _tfm_envelope_frames_hmc_dev("rtus_tfm_envelope_frames_hmc_i16_dev", torch.int16, stack, fs, tt_tx, tt_rx, t0, n_taps, f_demod,
                                        magnitude, out, cf, ws)


def tfm_envelope_frames_hmc_dev(stack, fs, tt_tx, tt_rx=None, t0=0.0, n_taps=63, f_demod=0.0, magnitude=False, out=None, cf=None, ws=None):
    """tfm_envelope_frames_hmc_i16_dev for float32 frames (rtus_tfm_envelope_frames_hmc_dev): ``stack`` float32
    [n_frames, n_pairs, n_t]; the same tensors, returns and bits."""
    return _tfm_envelope_frames_hmc_dev("rtus_tfm_envelope_frames_hmc_dev", torch.float32, stack, fs, tt_tx, tt_rx, t0, n_taps, f_demod,
                                        magnitude, out, cf, ws)


def tfm_analytic_hmc_dev(analytic, fs, tt_tx, tt_rx=None, t0=0.0, out=None, cf=None):
    """Envelope TFM over a half-matrix capture on device (rtus_tfm_analytic_hmc_dev; api.tfm_analytic_hmc's definition): analytic
    float32 [n_pairs, n_t, 2], tt_tx / tt_rx [n_e, n_f] (default: tt_tx) -> out float32 [n_f, 2] (the complex sum); ``cf``: an
    optional float32 [n_f] tensor that receives the coherence factor (then -> (out, cf)).  Asynchronous on the current stream
    (capturable with pre-allocated outputs)."""
    _chk(analytic, "analytic", torch.float32); _chk(tt_tx, "tt_tx")
    tt_rx = tt_tx if tt_rx is None else _chk(tt_rx, "tt_rx")
    n_e, n_f = _hmc_tables(tt_tx, tt_rx, analytic, True)
    out = _result(out, (n_f, 2), analytic, torch.float32)
    _optional(n_f, torch.float32, cf=cf)
    if not (out.device == analytic.device == tt_tx.device == tt_rx.device and (cf is None or cf.device == analytic.device)):
        raise ValueError("analytic, tt_tx, tt_rx, out and cf must be on one device")
    st = _lib.lib().rtus_tfm_analytic_hmc_dev(_p(analytic), n_e, analytic.shape[1], float(fs), float(t0), _p(tt_tx), _p(tt_rx), n_f,
                                              _p(out), _p(cf), _stream(analytic))
    _lib.check(st, "rtus_tfm_analytic_hmc_dev")
    return out if cf is None else (out, cf)


def tfm_iq_hmc_dev(analytic, fs, f_demod, tt_tx, tt_rx=None, t0=0.0, out=None, cf=None):
    """tfm_iq_dev over a half-matrix capture (rtus_tfm_iq_hmc_dev; api.tfm_iq_hmc's definition): tfm_analytic_hmc_dev's tensors
    and returns, ``f_demod`` [Hz] as in tfm_iq_dev.  Asynchronous on the current stream (capturable with pre-allocated outputs)."""
    f_demod = _f_demod(f_demod, fs)
    _chk(analytic, "analytic", torch.float32); _chk(tt_tx, "tt_tx")
    tt_rx = tt_tx if tt_rx is None else _chk(tt_rx, "tt_rx")
    n_e, n_f = _hmc_tables(tt_tx, tt_rx, analytic, True)
    out = _result(out, (n_f, 2), analytic, torch.float32)
    _optional(n_f, torch.float32, cf=cf)
    if not (out.device == analytic.device == tt_tx.device == tt_rx.device and (cf is None or cf.device == analytic.device)):
        raise ValueError("analytic, tt_tx, tt_rx, out and cf must be on one device")
    st = _lib.lib().rtus_tfm_iq_hmc_dev(_p(analytic), n_e, analytic.shape[1], float(fs), float(t0), f_demod, _p(tt_tx), _p(tt_rx), n_f,
                                        _p(out), _p(cf), _stream(analytic))
    _lib.check(st, "rtus_tfm_iq_hmc_dev")
    return out if cf is None else (out, cf)


def tfm_phase_dev(analytic, fs, tt_tx, tt_rx=None, t0=0.0, out=None, vcf=None, scf=None, counts=None):
    """Phase-coherence TFM on device (rtus_tfm_phase_dev; api.tfm_phase's definition): tfm_analytic_dev's tensors -> out float32
    [n_f, 2] (the complex sum, tfm_analytic_dev's bits); ``vcf`` / ``scf``: optional float32 [n_f] tensors that receive the vector /
    sign coherence factor, ``counts``: an optional int32 [n_f, 2] tensor that receives (sign sum, number of pairs).  -> out, or the
    tuple of out followed by the optional tensors given (in that order).  Asynchronous on the current stream (capturable with
    pre-allocated outputs)."""
    _chk(analytic, "analytic", torch.float32); _chk(tt_tx, "tt_tx")
    tt_rx = tt_tx if tt_rx is None else _chk(tt_rx, "tt_rx")
    n_f = _tables(tt_tx, tt_rx, analytic, analytic=True)
    out = _result(out, (n_f, 2), analytic, torch.float32)
    _optional(n_f, torch.float32, vcf=vcf, scf=scf)
    _optional(2 * n_f, torch.int32, counts=counts)
    given = [t for t in (vcf, scf, counts) if t is not None]
    if not all(t.device == analytic.device for t in (tt_tx, tt_rx, out, *given)):
        raise ValueError("analytic, tt_tx, tt_rx, out, vcf, scf and counts must be on one device")
    st = _lib.lib().rtus_tfm_phase_dev(_p(analytic), analytic.shape[0], analytic.shape[1], analytic.shape[2], float(fs), float(t0),
                                       _p(tt_tx), _p(tt_rx), n_f, _p(out), _p(vcf), _p(scf), _p(counts), _stream(analytic))
    _lib.check(st, "rtus_tfm_phase_dev")
    return (out, *given) if given else out


def tfm_phase_hmc_dev(analytic, fs, tt_tx, tt_rx=None, t0=0.0, out=None, vcf=None, scf=None, counts=None):
    """Phase-coherence TFM over a half-matrix capture on device (rtus_tfm_phase_hmc_dev; api.tfm_phase_hmc's definition):
    tfm_analytic_hmc_dev's tensors -> out float32 [n_f, 2] (tfm_analytic_hmc_dev's bits); ``vcf`` / ``scf`` / ``counts``: the optional
    outputs of tfm_phase_dev (float32 [n_f], float32 [n_f], int32 [n_f, 2]).  -> out, or the tuple of out followed by the optional
    tensors given (in that order).  Asynchronous on the current stream (capturable with pre-allocated outputs)."""
    _chk(analytic, "analytic", torch.float32); _chk(tt_tx, "tt_tx")
    tt_rx = tt_tx if tt_rx is None else _chk(tt_rx, "tt_rx")
    n_e, n_f = _hmc_tables(tt_tx, tt_rx, analytic, True)
    out = _result(out, (n_f, 2), analytic, torch.float32)
    _optional(n_f, torch.float32, vcf=vcf, scf=scf)
    _optional(2 * n_f, torch.int32, counts=counts)
    given = [t for t in (vcf, scf, counts) if t is not None]
    if not all(t.device == analytic.device for t in (tt_tx, tt_rx, out, *given)):
        raise ValueError("analytic, tt_tx, tt_rx, out, vcf, scf and counts must be on one device")
    st = _lib.lib().rtus_tfm_phase_hmc_dev(_p(analytic), n_e, analytic.shape[1], float(fs), float(t0), _p(tt_tx), _p(tt_rx), n_f,
                                           _p(out), _p(vcf), _p(scf), _p(counts), _stream(analytic))
    _lib.check(st, "rtus_tfm_phase_hmc_dev")
    return (out, *given) if given else out


def tfm_weighted_hmc_dev(analytic, fs, tt_tx, w_tx, tt_rx=None, w_rx=None, t0=0.0, out=None, sens=None):
    """Weighted envelope TFM over a half-matrix capture on device (rtus_tfm_weighted_hmc_dev; api.tfm_weighted_hmc's definition):
    analytic float32 [n_pairs, n_t, 2], tt_tx / tt_rx float64 [n_e, n_f], w_tx / w_rx float32 [n_e, n_f, 2] (complex); tt_rx and w_rx
    default to tt_tx and w_tx (tt_rx None or tt_tx itself: one delay table, every record gathered once) -> out float32 [n_f, 2];
    ``sens``: an optional float32 [n_f] tensor that receives the sensitivity (then -> (out, sens)).  Asynchronous on the current
    stream (capturable with pre-allocated outputs)."""
    _chk(analytic, "analytic", torch.float32); _chk(tt_tx, "tt_tx"); _chk(w_tx, "w_tx", torch.float32)
    tt_rx = tt_tx if tt_rx is None else _chk(tt_rx, "tt_rx")
    w_rx = w_tx if w_rx is None else _chk(w_rx, "w_rx", torch.float32)
    n_e, n_f = _hmc_tables(tt_tx, tt_rx, analytic, True)
    if tuple(w_tx.shape) != (n_e, n_f, 2) or tuple(w_rx.shape) != (n_e, n_f, 2):
        raise ValueError(f"w_tx / w_rx must be float32 [{n_e}, {n_f}, 2]")
    out = _result(out, (n_f, 2), analytic, torch.float32)
    _optional(n_f, torch.float32, sens=sens)
    devs = {t.device for t in (analytic, tt_tx, tt_rx, w_tx, w_rx, out) + ((sens,) if sens is not None else ())}
    if len(devs) != 1:
        raise ValueError("analytic, the tables, the weights, out and sens must be on one device")
    st = _lib.lib().rtus_tfm_weighted_hmc_dev(_p(analytic), n_e, analytic.shape[1], float(fs), float(t0), _p(tt_tx), _p(tt_rx),
                                              _p(w_tx), _p(w_rx), n_f, _p(out), _p(sens), _stream(analytic))
    _lib.check(st, "rtus_tfm_weighted_hmc_dev")
    return out if sens is None else (out, sens)


class LayersPlan:
    """Pre-bound ``rtus_tt_layers_dev`` call for repeated solves of one shape: ``run()`` is a single
    ctypes call (no argument checking, no allocation, no sync) — capturable in a hipGraph."""

    def __init__(self, z_if, c, xe, ze, xf, zf, out=None, iters=None, row0=0, n_rows_total=None, taup=False):
        self.z_if, self.c = _api._medium(z_if, c, flat=True)
        self.n_e, self.n_f = _pair(xe, ze, xf, zf)
        self.out = _result(out, (self.n_e, self.n_f), xe)
        self._keep = (xe, ze, xf, zf, self.out, iters)
        self._fn = _lib.lib().rtus_tt_layers_dev
        self._args = [self.z_if.ctypes.data if self.z_if.size else None, self.c.ctypes.data, self.z_if.size,
                      _p(xe), _p(ze), self.n_e, _p(xf), _p(zf), self.n_f, _p(self.out), _p(iters)]
        if n_rows_total is not None or taup:      # a row block of a larger table and / or the tau-p tier (rtus_tt_layers_rows_dev)
            self._fn = _lib.lib().rtus_tt_layers_rows_dev
            self._args = self._args[:6] + [int(row0), int(self.n_e if n_rows_total is None else n_rows_total)] + self._args[6:10] + \
                [TAUP_TAIL if taup else 0]

    def run(self, stream=None):
        st = self._fn(*self._args, _stream() if stream is None else stream)
        if st:
            _lib.check(st, "rtus_tt_layers_dev")
        return self.out


def pw_layers_dev(z_if, c, angles, x_lo, x_hi, z_a, xf, zf, out=None):
    """Plane-wave transmit times through horizontal layers on device (rtus_pw_layers_dev; api.pw_travel_time_layers's definition):
    z_if / c small HOST sequences, angles / xf / zf float64 CUDA tensors, the aperture [x_lo, x_hi] at depth z_a -> out [n_a, n_f].
    Asynchronous on the current stream."""
    z_if, c = _api._medium(z_if, c, flat=True)
    _chk(angles, "angles"); _chk(xf, "xf"); _chk(zf, "zf")
    n_a, n_f = angles.numel(), xf.numel()
    if zf.numel() != n_f:
        raise ValueError("xf/zf must pair up")
    out = _result(out, (n_a, n_f), xf)
    st = _lib.lib().rtus_pw_layers_dev(z_if.ctypes.data if z_if.size else None, c.ctypes.data, z_if.size, _p(angles), n_a, float(x_lo),
                                       float(x_hi), float(z_a), _p(xf), _p(zf), n_f, _p(out), _stream(xf))
    _lib.check(st, "rtus_pw_layers_dev")
    return out


def pw_surface_dev(x0, dx, zs, c1, c2, angles, x_lo, x_hi, z_a, xf, zf, out=None, x_entry=None):
    """Plane-wave transmit times through one curved interface on device (rtus_pw_surface_dev; api.pw_travel_time_surface's
    definition) on float64 CUDA tensors -> out [n_a, n_f] (and x_entry [n_a, n_f] when a tensor is given for it).  The spline's
    workspace is allocated here; asynchronous on the current stream."""
    for t, n in ((zs, "zs"), (angles, "angles"), (xf, "xf"), (zf, "zf")):
        _chk(t, n)
    n_a, n_f = angles.numel(), xf.numel()
    if zf.numel() != n_f:
        raise ValueError("xf/zf must pair up")
    out = _result(out, (n_a, n_f), xf)
    _optional(n_a * n_f, x_entry=x_entry)
    need = int(_lib.lib().rtus_tt_surface_workspace_bytes(zs.numel()))
    ws = _workspace(None, need, xf)
    st = _lib.lib().rtus_pw_surface_dev(float(x0), float(dx), _p(zs), zs.numel(), float(c1), float(c2), _p(angles), n_a, float(x_lo),
                                        float(x_hi), float(z_a), _p(xf), _p(zf), n_f, _p(out), _p(x_entry), _p(ws), need, _stream(xf))
    _lib.check(st, "rtus_pw_surface_dev")
    return out


def skip_layers_dev(z_if, c, z_back, xe, ze, xf, zf, c_up=None, out=None, taup=False):
    """Skip-leg times through horizontal layers on device (api.skip_travel_time_layers's definition): tt_layers_dev on the stack
    z_if + [z_back], c + [c_up] at the mirrored depth 2 z_back - zf, then NaN outside z_if[-1] < zf < z_back.  z_if / c are small
    HOST sequences; asynchronous on the current stream (no host synchronisation)."""
    z_if, c = _api._medium(z_if, c, flat=True)
    z_back = float(z_back)
    front = float(z_if[-1]) if z_if.size else -float("inf")
    if not (z_back > front):
        raise ValueError("the backwall must lie below the last interface (z_back > z_if[-1])")
    if z_if.size + 1 > _api.MAX_LAYERS:
        raise ValueError(f"a skip leg adds an interface: at most {_api.MAX_LAYERS - 1} interfaces above the backwall")
    _chk(zf, "zf")
    c_up = float(c[-1]) if c_up is None else float(c_up)
    zm = (2.0 * z_back) - zf
    out = tt_layers_dev(np.r_[z_if, z_back], np.r_[c, c_up], xe, ze, xf, zm, out=out, taup=taup)
    ok = (zf > front) & (zf < z_back)
    out.view(-1, zf.numel()).masked_fill_(~ok.view(1, -1), float("nan"))
    return out


def tt_surface_skip_dev(x0, dx, zs, c1, c_down, c_up, z_back, xe, ze, xf, zf, out=None, x_entry=None, x_back=None):
    """Skip-leg times through one curved interface on device (rtus_tt_surface_skip_dev; api.skip_travel_time_surface's definition)
    on float64 CUDA tensors -> out [n_e, n_f] (and x_entry / x_back [n_e, n_f] when tensors are given for them).  The spline's
    workspace is allocated here; asynchronous on the current stream."""
    _chk(zs, "zs")
    n_e, n_f = _pair(xe, ze, xf, zf)
    out = _result(out, (n_e, n_f), xe)
    _optional(n_e * n_f, x_entry=x_entry, x_back=x_back)
    need = int(_lib.lib().rtus_tt_surface_workspace_bytes(zs.numel()))
    ws = _workspace(None, need, xe)
    st = _lib.lib().rtus_tt_surface_skip_dev(float(x0), float(dx), _p(zs), zs.numel(), float(c1), float(c_down), float(c_up),
                                             float(z_back), _p(xe), _p(ze), n_e, _p(xf), _p(zf), n_f, _p(out), _p(x_entry), _p(x_back),
                                             _p(ws), need, _stream(xe))
    _lib.check(st, "rtus_tt_surface_skip_dev")
    return out


def fmc_synth_tx_dev(fmc, fs, delays, out=None):
    """Synthesis of transmit delay laws on device (rtus_fmc_synth_tx_dev; api.fmc_synth_tx's definition): fmc float32
    [n_tx, n_rx, n_t], delays float64 [n_v, n_tx] (seconds) -> out float32 [n_v, n_rx, n_t], which must not overlap fmc or delays.
    Asynchronous on the current stream."""
    _chk(fmc, "fmc", torch.float32); _chk(delays, "delays")
    if fmc.dim() != 3 or delays.dim() != 2 or delays.shape[1] != fmc.shape[0]:
        raise ValueError("need fmc [n_tx, n_rx, n_t] and delays [n_v, n_tx]")
    n_v = delays.shape[0]
    out = _result(out, (n_v, fmc.shape[1], fmc.shape[2]), fmc, torch.float32)
    if not (out.device == fmc.device == delays.device):
        raise ValueError("out must be on the device of fmc / delays")
    st = _lib.lib().rtus_fmc_synth_tx_dev(_p(fmc), fmc.shape[0], fmc.shape[1], fmc.shape[2], float(fs), _p(delays), n_v, _p(out),
                                          _stream(fmc))
    _lib.check(st, "rtus_fmc_synth_tx_dev")
    return out


def leg_amp_surface_dev(x0, dx, zs, c1, rho1, c_l, c_t, rho2, z_back, leg, xe, ze, xf, zf, x_entry, x_back=None, *, up=False,
                        element_width=0.0, f_c=None, out=None, ws=None):
    """Ray amplitudes of one leg on device (rtus_leg_amp_surface_dev; api.leg_amplitudes_surface's definition): float64 CUDA tensors
    in, out float32 [n_e, n_f, 2] (interleaved complex64).  ``ws``: an optional uint8 tensor of rtus_tt_surface_workspace_bytes(n_s)
    bytes (allocated here otherwise; pass one to capture the call in a graph).  Asynchronous on the current stream."""
    if leg not in _api.LEG_CODES:
        raise ValueError(f"unknown leg {leg!r}: legs are {_api.LEGS}")
    _chk(zs, "zs"); _chk(x_entry, "x_entry")
    n_e, n_f = _pair(xe, ze, xf, zf)
    if len(leg) == 2 and x_back is None:
        raise ValueError(f"the skip leg {leg!r} needs x_back")
    _optional(n_e * n_f, x_entry=x_entry, x_back=x_back if len(leg) == 2 else None)
    if element_width > 0 and f_c is None:
        raise ValueError("an element width needs the centre frequency f_c")
    out = _result(out, (n_e, n_f, 2), xe, torch.float32)
    ws = _workspace(ws, int(_lib.lib().rtus_tt_surface_workspace_bytes(zs.numel())), xe)
    st = _lib.lib().rtus_leg_amp_surface_dev(float(x0), float(dx), _p(zs), zs.numel(), float(c1), float(rho1), float(c_l), float(c_t),
                                             float(rho2), float(z_back), _api.LEG_CODES[leg], 1 if up else 0, float(element_width),
                                             float(f_c or 0.0), _p(xe), _p(ze), n_e, _p(xf), _p(zf), n_f, _p(x_entry),
                                             _p(x_back if len(leg) == 2 else None), _p(out), _p(ws), ws.numel(), _stream(xe))
    _lib.check(st, "rtus_leg_amp_surface_dev")
    return out


def tfm_weighted_dev(analytic, fs, tt_tx, w_tx, tt_rx=None, w_rx=None, t0=0.0, out=None, sens=None):
    """Weighted envelope TFM on device (rtus_tfm_weighted_dev; api.tfm_weighted's definition): analytic float32 [n_tx, n_rx, n_t, 2],
    tt_tx [n_tx, n_f] / tt_rx [n_rx, n_f] float64 (tt_rx, w_rx default to tt_tx, w_tx), w_tx / w_rx float32 [n, n_f, 2] (complex)
    -> out float32 [n_f, 2]; ``sens``: an optional float32 [n_f] tensor that receives the sensitivity (then -> (out, sens)).
    Asynchronous on the current stream (capturable with pre-allocated outputs)."""
    _chk(analytic, "analytic", torch.float32); _chk(tt_tx, "tt_tx"); _chk(w_tx, "w_tx", torch.float32)
    if tt_rx is None:
        tt_rx = tt_tx
        w_rx = w_tx if w_rx is None else w_rx
    _chk(tt_rx, "tt_rx")
    if w_rx is None:
        raise ValueError("w_rx is needed with tt_rx")
    _chk(w_rx, "w_rx", torch.float32)
    n_f = _tables(tt_tx, tt_rx, analytic, analytic=True)
    if w_tx.numel() != 2 * tt_tx.numel() or w_rx.numel() != 2 * tt_rx.numel():
        raise ValueError("w_tx / w_rx must hold 2 * n_tx * n_f / 2 * n_rx * n_f float32 values")
    out = _result(out, (n_f, 2), analytic, torch.float32)
    _optional(n_f, torch.float32, sens=sens)
    devs = {t.device for t in (analytic, tt_tx, tt_rx, w_tx, w_rx, out) + ((sens,) if sens is not None else ())}
    if len(devs) != 1:
        raise ValueError("analytic, the tables, the weights, out and sens must be on one device")
    st = _lib.lib().rtus_tfm_weighted_dev(_p(analytic), analytic.shape[0], analytic.shape[1], analytic.shape[2], float(fs), float(t0),
                                          _p(tt_tx), _p(tt_rx), _p(w_tx), _p(w_rx), n_f, _p(out), _p(sens), _stream(analytic))
    _lib.check(st, "rtus_tfm_weighted_dev")
    return out if sens is None else (out, sens)


def _pipe_table(entry, pipe_args, c_up, xe, ze, xf, zf, out, angles, ws):
    """the body of tt_pipe_dev and tt_pipe_skip_dev: rtus_<entry>_dev with rtus_<entry>_workspace_bytes; ``c_up`` is the skip entry's
    one more argument (empty for the direct entry), ``angles`` the optional [n_e, n_f] outputs by name, in the entry's order"""
    lens, a_lo, a_hi, pipe, b_lo, b_hi, n_scan = pipe_args
    n_e, n_f = _pair(xe, ze, xf, zf)
    out = _result(out, (n_e, n_f), xe)
    _optional(n_e * n_f, **angles)
    L = _lib.lib()
    ws = _workspace(ws, int(getattr(L, f"rtus_{entry}_workspace_bytes")(n_e, n_scan)), xe)
    st = getattr(L, f"rtus_{entry}_dev")(C.byref(lens), a_lo, a_hi, C.byref(pipe), *c_up, b_lo, b_hi, n_scan, _p(xe), _p(ze), n_e, _p(xf),
                                         _p(zf), n_f, _p(out), *map(_p, angles.values()), _p(ws), ws.numel(), _stream(xe))
    _lib.check(st, f"rtus_{entry}_dev")
    return out


def tt_pipe_dev(xe, ze, xf, zf, out=None, alpha_out=None, beta_out=None, *, c3=5600.0, r_inner=0.0, params: Params = None,
                alpha_lo=None, alpha_hi=None, beta_lo=-np.pi / 2, beta_hi=np.pi / 2, n_scan=None, ws=None):
    """Lens-to-pipe-wall times on device (rtus_tt_pipe_dev; api.travel_time_pipe's definition and defaults) on float64 CUDA tensors
    -> out [n_e, n_f] (and alpha_out / beta_out [n_e, n_f] when tensors are given for them).  ``ws``: an optional uint8 tensor of
    at least rtus_tt_pipe_workspace_bytes(n_e, n_scan) bytes to reuse (a graph capture must not allocate); allocated here
    otherwise.  Asynchronous on the current stream."""
    args = _api._pipe_args(params, c3, r_inner, alpha_lo, alpha_hi, beta_lo, beta_hi, n_scan)
    return _pipe_table("tt_pipe", args, (), xe, ze, xf, zf, out, dict(alpha_out=alpha_out, beta_out=beta_out), ws)


def tt_pipe_skip_dev(xe, ze, xf, zf, out=None, alpha_out=None, beta_out=None, gamma_out=None, *, c_down, c_up=None, r_inner,
                     params: Params = None, alpha_lo=None, alpha_hi=None, beta_lo=-np.pi / 2, beta_hi=np.pi / 2, n_scan=None,
                     ws=None):
    """Bore-reflected skip legs into the pipe wall on device (rtus_tt_pipe_skip_dev; api.skip_travel_time_pipe's definition and
    defaults) on float64 CUDA tensors -> out [n_e, n_f] (and alpha_out / beta_out / gamma_out [n_e, n_f] when tensors are given for
    them).  ``ws``: an optional uint8 tensor of at least rtus_tt_pipe_skip_workspace_bytes(n_e, n_scan) bytes to reuse (a graph
    capture must not allocate); allocated here otherwise.  Asynchronous on the current stream."""
    c_up = c_down if c_up is None else c_up
    args = _api._pipe_args(params, c_down, r_inner, alpha_lo, alpha_hi, beta_lo, beta_hi, n_scan)
    return _pipe_table("tt_pipe_skip", args, (float(c_up),), xe, ze, xf, zf, out,
                       dict(alpha_out=alpha_out, beta_out=beta_out, gamma_out=gamma_out), ws)


def leg_amp_pipe_dev(leg, xe, ze, xf, zf, alpha, beta, gamma=None, *, c_l, c_t, rho_wall, rho_water, rho_lens, ct_lens, r_inner,
                     up=False, element_width=0.0, f_c=None, params: Params = None, alpha_lo=None, alpha_hi=None, out=None):
    """Ray amplitudes of one leg into the pipe wall on device (rtus_leg_amp_pipe_dev; api.leg_amplitudes_pipe's definition): float64
    CUDA tensors in (alpha, beta, gamma: n_e * n_f values each, as tt_pipe_dev / tt_pipe_skip_dev write them), out float32
    [n_e, n_f, 2] (interleaved complex64).  No workspace; asynchronous on the current stream (capturable with ``out`` given)."""
    if leg not in _api.LEG_CODES:
        raise ValueError(f"unknown leg {leg!r}: legs are {_api.LEGS}")
    _chk(alpha, "alpha"); _chk(beta, "beta")
    n_e, n_f = _pair(xe, ze, xf, zf)
    if len(leg) == 2 and gamma is None:
        raise ValueError(f"the skip leg {leg!r} needs gamma")
    _optional(n_e * n_f, alpha=alpha, beta=beta, gamma=gamma if len(leg) == 2 else None)
    if element_width > 0 and f_c is None:
        raise ValueError("an element width needs the centre frequency f_c")
    out = _result(out, (n_e, n_f, 2), xe, torch.float32)
    lens, a_lo, a_hi, pipe, media = _api._pipe_amp_args(params, r_inner, alpha_lo, alpha_hi, c_l, c_t, rho_wall, rho_water, rho_lens,
                                                        ct_lens)
    st = _lib.lib().rtus_leg_amp_pipe_dev(C.byref(lens), a_lo, a_hi, C.byref(pipe), C.byref(media), _api.LEG_CODES[leg], 1 if up else 0,
                                          float(element_width), float(f_c or 0.0), _p(xe), _p(ze), n_e, _p(xf), _p(zf), n_f, _p(alpha),
                                          _p(beta), _p(gamma if len(leg) == 2 else None), _p(out), _stream(xe))
    _lib.check(st, "rtus_leg_amp_pipe_dev")
    return out


def echo_pick_dev(analytic, fs, t_lo, t_hi, t0=0.0, t_pick=None, amp=None):
    """Echo time of every pair on device (rtus_echo_pick_dev; api.pick_echo_times' definition): analytic float32
    [n_tx, n_rx, n_t, 2]; t_lo / t_hi: a scalar each, or a float64 tensor [n_tx, n_rx] of per-pair bounds -> (t_pick float64
    [n_tx, n_rx], amp float32 [n_tx, n_rx]).  Outputs not given are allocated here; asynchronous on the current stream (capturable
    with pre-allocated outputs)."""
    _chk(analytic, "analytic", torch.float32)
    if analytic.dim() != 4 or analytic.shape[3] != 2:
        raise ValueError("analytic must be [n_tx, n_rx, n_t, 2]")
    n_tx, n_rx, n_t = analytic.shape[:3]

    def bound(v, name):
        if not isinstance(v, torch.Tensor):
            return float(v), None
        _chk(v, name)
        if v.numel() != n_tx * n_rx or v.device != analytic.device:
            raise ValueError(f"{name} must hold one bound per pair on the device of analytic")
        return 0.0, v
    lo, lo_t = bound(t_lo, "t_lo")
    hi, hi_t = bound(t_hi, "t_hi")
    t_pick = _result(t_pick, (n_tx, n_rx), analytic, name="t_pick")
    amp = _result(amp, (n_tx, n_rx), analytic, torch.float32, "amp")
    st = _lib.lib().rtus_echo_pick_dev(_p(analytic), n_tx, n_rx, n_t, float(fs), float(t0), lo, hi, _p(lo_t), _p(hi_t), _p(t_pick),
                                       _p(amp), _stream(analytic))
    _lib.check(st, "rtus_echo_pick_dev")
    return t_pick, amp


def geom_misfit_dev(tt, t_meas, weights=None, n=None, sse=None, sum_r=None, sum_w=None):
    """Misfit sums of a batch of geometries on device (rtus_geom_misfit_dev; include/rtus.h): tt float64 [G, T, E] (SolvePlan's
    ``tt``), t_meas [T, E], weights [T, E] or None -> (n int32 [G], sse, sum_r, sum_w float64 [G]).  Outputs not given are
    allocated here; asynchronous on the current stream (capturable with pre-allocated outputs)."""
    _chk(tt, "tt"); _chk(t_meas, "t_meas")
    if tt.dim() != 3 or tuple(t_meas.shape) != tuple(tt.shape[1:]):
        raise ValueError("tt must be [G, T, E] and t_meas [T, E]")
    if weights is not None:
        _chk(weights, "weights")
        if tuple(weights.shape) != tuple(t_meas.shape):
            raise ValueError("weights must have t_meas's shape")
    G = tt.shape[0]
    n = _result(n, (G,), tt, torch.int32, "n")
    sse, sum_r, sum_w = (_result(o, (G,), tt, name=name) for o, name in ((sse, "sse"), (sum_r, "sum_r"), (sum_w, "sum_w")))
    st = _lib.lib().rtus_geom_misfit_dev(_p(tt), G, tt.shape[1], tt.shape[2], _p(t_meas), _p(weights), _p(n), _p(sse), _p(sum_r),
                                         _p(sum_w), _stream(tt))
    _lib.check(st, "rtus_geom_misfit_dev")
    return n, sse, sum_r, sum_w


def specular_dev(tt_a, tt_b=None, n_refl=1, out=None, pos=None, n_min=None):
    """Specular echo times of sampled reflectors on device (rtus_specular_dev; api.specular_times' definition): tt_a float64
    [n_a, n_refl * n_p], tt_b [n_b, n_refl * n_p] (default: tt_a) -> out float64 [n_refl, n_a, n_b] (geom_misfit_dev's ``tt``);
    ``pos``: an optional float64 tensor of that size that receives the reflection point's index, ``n_min``: an optional int32 one
    that receives the number of interior minima.  -> out, or the tuple of out followed by the optional tensors given.
    Asynchronous on the current stream (capturable with pre-allocated outputs)."""
    _chk(tt_a, "tt_a")
    if tt_b is not None:
        _chk(tt_b, "tt_b")
    n_refl = int(n_refl)
    if tt_a.dim() != 2 or tt_a.numel() == 0 or n_refl < 1 or tt_a.shape[1] % n_refl:
        raise ValueError("tt_a must be [n_a, n_refl * n_p]")
    if tt_b is not None and (tt_b.dim() != 2 or tt_b.shape[0] == 0 or tt_b.shape[1] != tt_a.shape[1]):
        raise ValueError("tt_b must be [n_b, n_refl * n_p], the columns of tt_a")
    n_a, n_b = tt_a.shape[0], tt_a.shape[0] if tt_b is None else tt_b.shape[0]
    out = _result(out, (n_refl, n_a, n_b), tt_a)
    _optional(out.numel(), pos=pos)
    _optional(out.numel(), torch.int32, n_min=n_min)
    given = [t for t in (pos, n_min) if t is not None]
    if not all(t.device == tt_a.device for t in (out, *given, *(() if tt_b is None else (tt_b,)))):
        raise ValueError("tt_a, tt_b, out, pos and n_min must be on one device")
    st = _lib.lib().rtus_specular_dev(_p(tt_a), n_a, _p(tt_b), n_b, n_refl, tt_a.shape[1] // n_refl, _p(out), _p(pos), _p(n_min),
                                      _stream(tt_a))
    _lib.check(st, "rtus_specular_dev")
    return (out, *given) if given else out


def skip_reflector_dev(tt_down, xb, zb, c_up, xf, zf, out=None, pos=None, n_min=None):
    """Skip legs off a sampled backwall on device (rtus_skip_reflector_dev; api.skip_travel_time_reflector's definition): tt_down
    float64 [n_e, n_p], the reflector's points xb / zb [n_p], the up leg's speed ``c_up``, focal points xf / zf [n_f] -> out float64
    [n_e, n_f]; ``pos``: an optional float64 tensor of that size that receives the bounce point's index, ``n_min``: an optional
    int32 one that receives the number of interior minima.  -> out, or the tuple of out followed by the optional tensors given.
    Asynchronous on the current stream (capturable with pre-allocated outputs)."""
    _chk(tt_down, "tt_down")
    n_p, n_f = _pair(xb, zb, xf, zf)
    if tt_down.dim() != 2 or tt_down.numel() == 0 or tt_down.shape[1] != n_p:
        raise ValueError("tt_down must be [n_e, n_p] with one column per reflector point (xb, zb)")
    if n_f == 0:
        raise ValueError("xf / zf must hold at least one focal point")
    c_up = float(c_up)
    if not (np.isfinite(c_up) and c_up > 0):
        raise ValueError("c_up must be finite and positive")
    n_e = tt_down.shape[0]
    out = _result(out, (n_e, n_f), tt_down)
    _optional(out.numel(), pos=pos)
    _optional(out.numel(), torch.int32, n_min=n_min)
    given = [t for t in (pos, n_min) if t is not None]
    if not all(t.device == tt_down.device for t in (xb, zb, xf, zf, out, *given)):
        raise ValueError("tt_down, xb, zb, xf, zf, out, pos and n_min must be on one device")
    st = _lib.lib().rtus_skip_reflector_dev(_p(tt_down), n_e, _p(xb), _p(zb), n_p, c_up, _p(xf), _p(zf), n_f, _p(out), _p(pos),
                                            _p(n_min), _stream(tt_down))
    _lib.check(st, "rtus_skip_reflector_dev")
    return (out, *given) if given else out


def _sim_out(n_tx, n_rx, n_t, pulse, out, analytic, ref):
    """the wavelet and result checks fmc_sim_dev and fmc_sim_echo_dev share -> out"""
    _chk(pulse, "pulse", torch.float32)
    if pulse.dim() != 2 or pulse.shape[1] != 2:
        raise ValueError("pulse must be float32 [n_p, 2] (complex)")
    out = _result(out, (n_tx, n_rx, n_t, 2) if analytic else (n_tx, n_rx, n_t), ref, torch.float32)
    if out.device != ref.device or pulse.device != ref.device:
        raise ValueError("the tables, pulse and out must be on one device")
    return out


def fmc_sim_dev(tt_tx, tt_rx=None, *, fs, n_t, pulse, centre, oversample, t0=0.0, strength=None, w_tx=None, w_rx=None, analytic=False,
                accumulate=False, out=None):
    """FMC simulator on device (rtus_fmc_sim_dev; api.simulate_fmc's definition): tt_tx [n_tx, n_s] / tt_rx [n_rx, n_s] float64
    (tt_rx, w_rx default to tt_tx, w_tx); strength float32 [n_s, 2], w_tx / w_rx float32 [n, n_s, 2] (complex), each optional;
    pulse float32 [n_p, 2] -> out float32 [n_tx, n_rx, n_t] or, with ``analytic``, [n_tx, n_rx, n_t, 2].  ``accumulate`` adds onto
    ``out``.  Asynchronous on the current stream (capturable with a pre-allocated ``out``)."""
    _chk(tt_tx, "tt_tx")
    if tt_rx is None:
        tt_rx = tt_tx
        w_rx = w_tx if w_rx is None else w_rx
    _chk(tt_rx, "tt_rx")
    n_tx, n_rx, n_s = tt_tx.shape[0], tt_rx.shape[0], _tables(tt_tx, tt_rx)
    if tt_tx.device != tt_rx.device:
        raise ValueError("tt_tx and tt_rx must be on one device")
    for t, name, n in ((strength, "strength", n_s), (w_tx, "w_tx", n_tx * n_s), (w_rx, "w_rx", n_rx * n_s)):
        if t is not None:
            _chk(t, name, torch.float32)
            if t.numel() != 2 * n or t.device != tt_tx.device:
                raise ValueError(f"{name} must hold {n} complex values (float32 pairs) on the tables' device")
    if accumulate and out is None:
        raise ValueError("accumulate=True needs the FMC to add onto in ``out``")
    out = _sim_out(n_tx, n_rx, int(n_t), pulse, out, analytic, tt_tx)
    flags = (_api.SIM_ANALYTIC if analytic else 0) | (_api.SIM_ACCUMULATE if accumulate else 0)
    st = _lib.lib().rtus_fmc_sim_dev(_p(tt_tx), _p(tt_rx), n_tx, n_rx, n_s, _p(strength), _p(w_tx), _p(w_rx), _p(pulse), pulse.shape[0],
                                     int(centre), int(oversample), float(fs), float(t0), int(n_t), _p(out), flags, _stream(tt_tx))
    _lib.check(st, "rtus_fmc_sim_dev")
    return out


def fmc_sim_echo_dev(t_pair, amp=None, *, fs, n_t, pulse, centre, oversample, t0=0.0, analytic=False, accumulate=False, out=None):
    """Per-pair echoes to an FMC on device (rtus_fmc_sim_echo_dev; api.simulate_echoes' definition): t_pair float64
    [n_tx, n_rx, n_a], amp float32 [n_tx, n_rx, n_a, 2] or None; the rest as fmc_sim_dev."""
    _chk(t_pair, "t_pair")
    if t_pair.dim() != 3:
        raise ValueError("t_pair must be [n_tx, n_rx, n_a]")
    n_tx, n_rx, n_a = t_pair.shape
    if amp is not None:
        _chk(amp, "amp", torch.float32)
        if amp.numel() != 2 * t_pair.numel() or amp.device != t_pair.device:
            raise ValueError("amp must hold one complex value (a float32 pair) per arrival on t_pair's device")
    if accumulate and out is None:
        raise ValueError("accumulate=True needs the FMC to add onto in ``out``")
    out = _sim_out(n_tx, n_rx, int(n_t), pulse, out, analytic, t_pair)
    flags = (_api.SIM_ANALYTIC if analytic else 0) | (_api.SIM_ACCUMULATE if accumulate else 0)
    st = _lib.lib().rtus_fmc_sim_echo_dev(_p(t_pair), _p(amp), n_tx, n_rx, n_a, _p(pulse), pulse.shape[0], int(centre), int(oversample),
                                          float(fs), float(t0), int(n_t), _p(out), flags, _stream(t_pair))
    _lib.check(st, "rtus_fmc_sim_echo_dev")
    return out

"""Host-side mirror of the reference's call surface, on top of the C ABI (include/rtus.h).

``shoot_rays(x_a, z_a, z_f, alpha, plot=False)`` keeps the positional signature and the 8-key
dict of float64[N] of the reference (main_rt.py:337, 432-441).  The constants the reference
reads as module globals (c1, c2, l0, h0, d, r_outer, pipe_offset — main_rt.py:449-467) are an
explicit :class:`Params`; when none is given they are looked up the way the reference's scripts
define them (``configure(...)`` first, then same-named attributes of ``__main__``).

Everything here runs on the GPU through librtus.so.  There is no CPU fallback.
"""
import ctypes as C
import sys
import warnings
from dataclasses import dataclass, replace

import numpy as np

from . import _lib
from ._lib import Lens, Pipe, PipeMedia

KEYS = ("lens_1_x", "lens_1_z", "pipe_x", "pipe_z", "lens_2_x", "lens_2_z", "target_x", "target_z")


@dataclass(frozen=True)
class Params:
    """Medium + geometry constants (reference: module globals, main_rt.py:449-467)."""
    c1: float = 6400.0                     # main_rt.py:449
    c2: float = 1483.0                     # main_rt.py:450
    l0: float = 0.12156646438729327        # main_rt.py:453
    h0: float = 0.08843353561270673        # main_rt.py:454
    d: float = None                        # main_rt.py:455 (l0 + h0 when None)
    r_outer: float = 0.05                  # main_rt.py:466
    pipe_offset: float = 0.0               # main_rt.py:467

    def __post_init__(self):
        if self.d is None:
            object.__setattr__(self, "d", float(np.float64(self.l0) + np.float64(self.h0)))

    def lens(self) -> Lens:
        return Lens(float(self.c1), float(self.c2), float(self.l0), float(self.h0), float(self.d))


#: the reference's launch-angle half-aperture (main_rt.py:457)
ALPHA_MAX = float(np.float64(50.62033040986099 * (np.pi / 180)))

_configured = None


def configure(params: Params = None, **kw) -> Params:
    """Set the default Params (the explicit replacement for assigning module globals)."""
    global _configured
    base = params if params is not None else (_configured or Params())
    _configured = replace(base, **kw) if kw else base
    return _configured


def _resolve(params):
    if params is not None:
        return params
    if _configured is not None:
        return _configured
    main = sys.modules.get("__main__")
    names = ("c1", "c2", "l0", "h0", "d", "r_outer", "pipe_offset")
    if main is not None and all(hasattr(main, n) for n in names):   # main_compare.py-style script
        return Params(**{n: float(getattr(main, n)) for n in names})
    raise ValueError("no Params given: pass params=..., call configure(...), or define "
                     "c1,c2,l0,h0,d,r_outer,pipe_offset in __main__ as the reference scripts do")


def reference_elements(num_elements=64, pitch=0.0006):
    """main_rt.py:469-474 — centred linear array plus the virtual centre element at index 32."""
    x_a = np.arange(num_elements, dtype=np.float64) * np.float64(pitch)
    x_a = x_a - np.mean(x_a)
    return np.insert(x_a, num_elements // 2, np.float64(0.0))


def _f64(a, name, ndim=1):
    a = np.ascontiguousarray(a, dtype=np.float64)
    if ndim == 1:
        a = np.atleast_1d(a)
    if a.ndim != ndim:
        raise ValueError(f"{name} must be {ndim}-D, got shape {a.shape}")
    return a


def _ptr(a):
    return None if a is None else a.ctypes.data


def _medium(z_if, c, flat=False):
    """The host medium of the planar entries -> (z_if, c) as float64 vectors with len(c) == len(z_if) + 1 (the C layer reads
    c[0 .. n_if] from the host pointer)."""
    if flat:      # device.py's wrappers and fmc_table_layers have always flattened whatever shape comes; the others insist on 1-D
        z_if, c = (np.ascontiguousarray(v, dtype=np.float64).reshape(-1) for v in (z_if, c))
    else:
        z_if, c = _f64(z_if, "z_if") if np.size(z_if) else np.zeros(0), _f64(c, "c")
    if c.size != z_if.size + 1:
        raise ValueError("need len(c) == len(z_if) + 1")
    return z_if, c


def _points(xe, ze, xf, zf):
    """Elements and focal points as float64 vectors, xe/ze and xf/zf of one length each."""
    xe, ze, xf, zf = _f64(xe, "xe"), _f64(ze, "ze"), _f64(xf, "xf"), _f64(zf, "zf")
    if xe.shape != ze.shape or xf.shape != zf.shape:
        raise ValueError("xe/ze and xf/zf must pair up")
    return xe, ze, xf, zf


def _out(out, shape, dtype, name="out"):
    """The caller's result buffer (checked) or a fresh pageable one."""
    if out is None:
        return np.empty(shape, dtype=dtype)
    if not isinstance(out, np.ndarray) or out.dtype != np.dtype(dtype) or out.shape != tuple(shape) \
            or not out.flags.c_contiguous or not out.flags.writeable:
        raise ValueError(f"{name} must be a writeable C-contiguous {np.dtype(dtype).name} array of shape {tuple(shape)}")
    return out


SHOOT_FAST_MATH = 0x1       # RTUS_SHOOT_FAST_MATH
TRUE_PIPE_TANGENT = 0x2     # RTUS_TRUE_PIPE_TANGENT  (physically correct; not the reference)
ANALYTIC_LENS = 0x4         # RTUS_ANALYTIC_LENS      (physically correct; not the reference)
POLYLINE_READY = 0x8        # RTUS_POLYLINE_READY     (device entry points: the workspace holds this alpha grid's lens polyline)
MAX_ROOTS = 4               # RTUS_MAX_ROOTS


def _flags(fast=False, true_tangent=False, analytic_lens=False):
    return (SHOOT_FAST_MATH if fast else 0) | (TRUE_PIPE_TANGENT if true_tangent else 0) | \
        (ANALYTIC_LENS if analytic_lens else 0)


def shoot_batch(x_a, z_a, z_f, alpha, geoms=None, *, params: Params = None, want=("out8",), fast=False,
                true_tangent=False, analytic_lens=False, device=0):
    """Forward trace for n_geom geometries x n_tx transmit points in ONE launch.

    geoms: [n_geom, 2] of (r_outer, pipe_offset); default = the one geometry in ``params``.
    want:  any of "out8" [G,T,8,N], "tof4" [G,T,4,N], "tof" [G,T,N], "land_x" [G,T,N], "status".
    fast:  vector-form arithmetic (no trigonometry; measured 1.6-1.7x faster); the default reproduces the reference's
           angle-form arithmetic operation for operation.
    """
    p = _resolve(params)
    x_a, z_a = _f64(x_a, "x_a"), _f64(z_a, "z_a")
    alpha, z_f = _f64(alpha, "alpha"), _f64(z_f, "z_f")
    if x_a.shape != z_a.shape:
        raise ValueError("x_a and z_a must have the same length")        # main_rt.py:28-29
    if alpha.shape != z_f.shape:
        raise ValueError("alpha and z_f must have the same length")
    if alpha.size < 2:
        raise ValueError("Curve needs at least two points.")             # main_rt.py:26-27
    geoms = (np.asarray([[p.r_outer, p.pipe_offset]], dtype=np.float64) if geoms is None
             else _f64(geoms, "geoms", 2))
    if geoms.shape[1] != 2:
        raise ValueError("geoms must be [n_geom, 2] = (r_outer, pipe_offset)")
    G, T, N = geoms.shape[0], x_a.size, alpha.size
    bufs = dict(out8=None, tof4=None, tof=None, land_x=None, status=None)
    shapes = dict(out8=(G, T, 8, N), tof4=(G, T, 4, N), tof=(G, T, N), land_x=(G, T, N), status=(G, T, N))
    for w in want:
        if w not in bufs:
            raise ValueError(f"unknown output {w!r}")
        bufs[w] = np.empty(shapes[w], dtype=np.uint8 if w == "status" else np.float64)
    lens = p.lens()
    st = _lib.lib().rtus_shoot(C.byref(lens), _ptr(geoms), G, _ptr(x_a), _ptr(z_a), T, _ptr(alpha), _ptr(z_f), N,
                               _ptr(bufs["out8"]), _ptr(bufs["tof4"]), _ptr(bufs["tof"]), _ptr(bufs["land_x"]),
                               _ptr(bufs["status"]), _flags(fast, true_tangent, analytic_lens), int(device))
    _lib.check(st, "rtus_shoot")
    return {w: bufs[w] for w in want}


def shoot_rays(x_a, z_a, z_f, alpha, plot=False, *, params: Params = None, device=0, **options):
    """Drop-in for the reference's shoot_rays (main_rt.py:337): one transmit point, one geometry.

    Returns the same dict of eight float64[N] arrays (main_rt.py:432-441); invalid rays are NaN.
    ``plot`` is accepted for signature compatibility; plotting (main_rt.py:407-430) is out of scope
    and the default is False so the call never blocks on a GUI.  ``options``: fast / true_tangent /
    analytic_lens as in :func:`shoot_batch` (all off = the reference's arithmetic).

    The reference's driver calls this 210 times in a row (main_rt.py:464-482), so the wrapper itself is kept
    short: one result buffer whose eight rows are the eight arrays, no per-key copies.
    """
    if plot:
        warnings.warn("rtus.shoot_rays: plotting is not part of the accelerated path; ignoring plot=True",
                      stacklevel=2)
    if np.ndim(x_a) != 0 or np.ndim(z_a) != 0:
        raise ValueError("x_a and z_a are scalars (one transmit point), as in main_rt.py:482")
    p = _resolve(params)
    alpha = np.ascontiguousarray(alpha, dtype=np.float64)
    z_f = np.ascontiguousarray(z_f, dtype=np.float64)
    if alpha.ndim != 1 or z_f.ndim != 1:
        raise ValueError("alpha and z_f must be 1-D")
    if alpha.shape != z_f.shape:
        raise ValueError("alpha and z_f must have the same length")
    if alpha.size < 2:
        raise ValueError("Curve needs at least two points.")             # main_rt.py:26-27
    out8 = np.empty((8, alpha.size), dtype=np.float64)
    head = np.array([p.r_outer, p.pipe_offset, x_a, z_a], dtype=np.float64)   # geoms[1][2], x_a[1], z_a[1]
    hp = head.ctypes.data
    st = _lib.lib().rtus_shoot(C.byref(p.lens()), hp, 1, hp + 16, hp + 24, 1, alpha.ctypes.data, z_f.ctypes.data, alpha.size,
                               out8.ctypes.data, None, None, None, None, _flags(**options), int(device))
    _lib.check(st, "rtus_shoot")
    return dict(zip(KEYS, out8))          # eight row views of one caller-owned buffer


def match_elements(land_x, tof, x_rx, atol=1e-6, rtol=1e-5, *, device=0):
    """Element matcher (main_rt.py:487-501): per receive element the first ray within np.isclose.

    land_x, tof: [..., N]; x_rx: [E].  Returns (hit bool[..., E], tof_hit f64[..., E] (0.0 if none),
    first_ray int32[..., E] (-1 if none)).
    """
    land_x = np.ascontiguousarray(land_x, dtype=np.float64)
    tof = np.ascontiguousarray(tof, dtype=np.float64)
    if land_x.shape != tof.shape or land_x.ndim < 1:
        raise ValueError("land_x and tof must have the same shape [..., n_rays]")
    x_rx = _f64(x_rx, "x_rx")
    lead, N, E = land_x.shape[:-1], land_x.shape[-1], x_rx.size
    nb = int(np.prod(lead)) if lead else 1
    first = np.empty((nb, E), dtype=np.int32)
    hit = np.empty((nb, E), dtype=np.uint8)
    tof_hit = np.empty((nb, E), dtype=np.float64)
    st = _lib.lib().rtus_match(_ptr(land_x), _ptr(tof), nb, N, _ptr(x_rx), E, float(atol), float(rtol),
                               _ptr(first), _ptr(hit), _ptr(tof_hit), int(device))
    _lib.check(st, "rtus_match")
    return (hit.astype(bool).reshape(lead + (E,)), tof_hit.reshape(lead + (E,)), first.reshape(lead + (E,)))


def sweep_batch(x_a, z_a, z_f, alpha, x_rx, geoms=None, *, atol=1e-6, rtol=1e-5, params: Params = None, want=(), fast=False,
                true_tangent=False, analytic_lens=False, device=0):
    """One body of the reference's parameter loop (main_rt.py:464-501) for n_geom geometries x n_tx transmit points in ONE kernel:
    ``shoot_batch`` and ``match_elements`` fused — the matcher runs on the landing points while they are in registers.

    Returns {"hit" bool[G,T,E], "tof_hit" f64[G,T,E] (0.0 where no ray hits), "first_ray" int32[G,T,E] (-1 where none)} plus the
    per-ray arrays named in ``want`` ("tof", "land_x": [G,T,N]).  Bit-identical to the two calls it replaces.
    """
    p = _resolve(params)
    x_a, z_a = _f64(x_a, "x_a"), _f64(z_a, "z_a")
    alpha, z_f, x_rx = _f64(alpha, "alpha"), _f64(z_f, "z_f"), _f64(x_rx, "x_rx")
    if x_a.shape != z_a.shape:
        raise ValueError("x_a and z_a must have the same length")        # main_rt.py:28-29
    if alpha.shape != z_f.shape:
        raise ValueError("alpha and z_f must have the same length")
    if alpha.size < 2:
        raise ValueError("Curve needs at least two points.")             # main_rt.py:26-27
    geoms = (np.asarray([[p.r_outer, p.pipe_offset]], dtype=np.float64) if geoms is None
             else _f64(geoms, "geoms", 2))
    if geoms.shape[1] != 2:
        raise ValueError("geoms must be [n_geom, 2] = (r_outer, pipe_offset)")
    G, T, N, E = geoms.shape[0], x_a.size, alpha.size, x_rx.size
    bufs = dict(tof=None, land_x=None)
    for w in want:
        if w not in bufs:
            raise ValueError(f"unknown output {w!r}")
        bufs[w] = np.empty((G, T, N), dtype=np.float64)
    first = np.empty((G, T, E), dtype=np.int32)
    hit = np.empty((G, T, E), dtype=np.uint8)
    tof_hit = np.empty((G, T, E), dtype=np.float64)
    lens = p.lens()
    st = _lib.lib().rtus_sweep(C.byref(lens), _ptr(geoms), G, _ptr(x_a), _ptr(z_a), T, _ptr(alpha), _ptr(z_f), N, _ptr(x_rx), E,
                               float(atol), float(rtol), _ptr(first), _ptr(hit), _ptr(tof_hit), _ptr(bufs["tof"]), _ptr(bufs["land_x"]),
                               _flags(fast, true_tangent, analytic_lens), int(device))
    _lib.check(st, "rtus_sweep")
    out = {"hit": hit.astype(bool), "tof_hit": tof_hit, "first_ray": first}
    out.update({w: bufs[w] for w in want})
    return out


def ray_hits(land_x, x_rx, atol=1e-4, rtol=1e-5, *, device=0):
    """Per ray: does any element match (main_compare.py:518-521)."""
    land_x = np.ascontiguousarray(land_x, dtype=np.float64)
    x_rx = _f64(x_rx, "x_rx")
    lead, N = land_x.shape[:-1], land_x.shape[-1]
    nb = int(np.prod(lead)) if lead else 1
    rh = np.empty((nb, N), dtype=np.uint8)
    st = _lib.lib().rtus_ray_hits(_ptr(land_x), nb, N, _ptr(x_rx), x_rx.size, float(atol), float(rtol),
                                  _ptr(rh), int(device))
    _lib.check(st, "rtus_ray_hits")
    return rh.astype(bool).reshape(lead + (N,))


def _device_list(devices):
    d = np.ascontiguousarray(devices, dtype=np.int32).reshape(-1)
    if d.size == 0:
        raise ValueError("devices must list at least one GPU")
    return d


TAUP_TAIL = 0x1             # RTUS_TT_TAUP_TAIL (include/rtus.h)


def travel_time_layers(z_if, c, xe, ze, xf, zf, *, return_iters=False, out=None, device=0, devices=None, taup=False):
    """Element x focal-point Fermat travel times through horizontal layers -> tt[n_e, n_f].

    ``out``: optional float64 [n_e, n_f] result buffer, returned as ``tt``.
    ``devices``: a list of GPU indices — the table's rows are solved in contiguous blocks on all of them at once and each
    GPU copies its block straight into ``tt`` (rtus_tt_layers_multi_ex); the result is bit for bit the one-GPU table.
    ``taup``: the faster accuracy tier (RTUS_TT_TAUP_TAIL: the tau-p form of the travel time, <= 1.3e-10 relative at worst
    (include/rtus.h), measured 3e-17 s on BASELINE configs[2]; the default tier: <= 1e-13 relative) — the tier bench.py's headline times.
    The aperture may come in any order: the rows are solved in (depth, position) order and stored where they belong, so an
    element's bits do not depend on it (``return_iters`` takes the elements as given: it is a diagnostic of that).

    NOT in the reference (no planar interfaces there): parity unpinned, see DESIGN.md.
    """
    z_if, c = _medium(z_if, c)
    xe, ze, xf, zf = _points(xe, ze, xf, zf)
    if taup and return_iters:
        raise ValueError("return_iters is a diagnostic of the default tier")
    flags = TAUP_TAIL if taup else 0
    tt = _out(out, (xe.size, xf.size), np.float64)
    if devices is not None:
        if return_iters:
            raise ValueError("return_iters is a one-device diagnostic")
        dv = _device_list(devices)
        st = _lib.lib().rtus_tt_layers_multi_ex(_ptr(z_if) if z_if.size else None, _ptr(c), z_if.size, _ptr(xe), _ptr(ze), xe.size,
                                                _ptr(xf), _ptr(zf), xf.size, _ptr(tt), dv.ctypes.data_as(C.POINTER(C.c_int)), dv.size, flags)
        _lib.check(st, "rtus_tt_layers_multi_ex")
        return tt
    iters = np.empty((xe.size, xf.size), dtype=np.uint8) if return_iters else None
    st = _lib.lib().rtus_tt_layers_ex(_ptr(z_if) if z_if.size else None, _ptr(c), z_if.size, _ptr(xe), _ptr(ze),
                                      xe.size, _ptr(xf), _ptr(zf), xf.size, _ptr(tt), _ptr(iters), flags, int(device))
    _lib.check(st, "rtus_tt_layers_ex")
    return (tt, iters) if return_iters else tt


def travel_time_lens(xe, ze, xf, zf, *, params: Params = None, alpha_lo=None, alpha_hi=None, dtype=np.float64,
                     return_alpha=False, out=None, device=0, devices=None):
    """Element x focal-point Fermat travel times through the reference's curved lens surface
    (h(alpha) of main_rt.py:180-189): elements in the lens (c1), targets in the water (c2) -> tt[n_e, n_f].

    dtype float32 runs the fp32 kernel (BASELINE config 4).  ``return_alpha`` also returns the polar
    angle of the refraction point.  As a two-point solver this is not in the reference; it is pinned to
    it through Fermat <=> Snell (see include/rtus.h).
    """
    p = _resolve(params)
    dt = np.dtype(dtype)
    if dt not in (np.dtype(np.float64), np.dtype(np.float32)):
        raise ValueError("dtype must be float64 or float32")
    a_lo = -ALPHA_MAX if alpha_lo is None else float(alpha_lo)
    a_hi = ALPHA_MAX if alpha_hi is None else float(alpha_hi)
    arr = [np.atleast_1d(np.ascontiguousarray(v, dtype=dt)) for v in (xe, ze, xf, zf)]
    xe, ze, xf, zf = arr
    if xe.shape != ze.shape or xf.shape != zf.shape or xe.ndim != 1 or xf.ndim != 1:
        raise ValueError("xe/ze and xf/zf must be 1-D and pair up")
    tt = _out(out, (xe.size, xf.size), dt)                       # out: optional caller-owned result buffer
    al = np.empty((xe.size, xf.size), dtype=dt) if return_alpha else None
    lens = p.lens()
    if devices is not None:                      # fp32 table over several GPUs (BASELINE configs[3]): rtus_tt_lens_f32_multi
        if dt != np.float32 or return_alpha:
            raise ValueError("devices=[...] is the float32 table without the alpha output")
        dv = _device_list(devices)
        st = _lib.lib().rtus_tt_lens_f32_multi(C.byref(lens), a_lo, a_hi, _ptr(xe), _ptr(ze), xe.size, _ptr(xf), _ptr(zf), xf.size,
                                               _ptr(tt), dv.ctypes.data_as(C.POINTER(C.c_int)), dv.size)
        _lib.check(st, "rtus_tt_lens_f32_multi")
        return tt
    fn = _lib.lib().rtus_tt_lens if dt == np.float64 else _lib.lib().rtus_tt_lens_f32
    st = fn(C.byref(lens), a_lo, a_hi, _ptr(xe), _ptr(ze), xe.size, _ptr(xf), _ptr(zf), xf.size, _ptr(tt), _ptr(al),
            int(device))
    _lib.check(st, "rtus_tt_lens")
    return (tt, al) if return_alpha else tt


def fmc_table_layers(z_if, c, x_tx, x_rx, z_reflector, *, z_array=0.0, device=0, devices=None, taup=False):
    """Full-matrix-capture tx/rx travel-time table for a planar specular reflector at depth z_reflector
    under horizontal layers (BASELINE config 5).  The down-and-up path through the layers is unfolded
    about the reflector plane into a one-way path through the mirrored stack, so the table is one
    travel_time_layers call: tt[n_tx, n_rx].  Not in the reference (parity unpinned)."""
    z_if, c = _medium(z_if, c, flat=True)
    above = z_if < z_reflector
    zi, cc = z_if[above], c[:above.sum() + 1]
    z_m = np.concatenate([zi, (2.0 * z_reflector - zi)[::-1]])          # mirrored interfaces
    c_m = np.concatenate([cc, cc[::-1][1:]])                            # ... and speeds (reflector layer merged)
    x_tx, x_rx = _f64(x_tx, "x_tx"), _f64(x_rx, "x_rx")
    return travel_time_layers(z_m, c_m, x_tx, np.full(x_tx.size, float(z_array)), x_rx,
                              np.full(x_rx.size, 2.0 * z_reflector - float(z_array)), device=device, devices=devices, taup=taup)


SOLVE_ONE_LANE = 0x10       # RTUS_SOLVE_ONE_LANE (include/rtus.h)
SOLVE_THREE_LAUNCHES = 0x20
SOLVE_PATHS = ("ROW", "TRIO_MASKS", "TRIO_SCAN", "HALF", "FULL", "SCAN")      # RTUS_SOLVE_PATH_* (include/rtus.h), by value


def solve_path(n_geom, n_tx, n_rays, n_rx, *, one_lane=False, three_launches=False):
    """The refinement a solve_travel_times / SolvePlan call of this size takes (rtus_solve_path: host code, no GPU needed): one of
    SOLVE_PATHS.  ValueError for a size rtus_solve refuses."""
    r = _lib.lib().rtus_solve_path(int(n_geom), int(n_tx), int(n_rays), int(n_rx),
                                   (SOLVE_ONE_LANE if one_lane else 0) | (SOLVE_THREE_LAUNCHES if three_launches else 0))
    if not 0 <= r < len(SOLVE_PATHS):
        raise ValueError(f"no solve of {n_geom} x {n_tx} rows, {n_rays} rays, {n_rx} elements")
    return SOLVE_PATHS[r]


def solve_travel_times(x_a, z_a, x_rx, alpha, geoms=None, *, z_land=None, params: Params = None, fast=False,
                       true_tangent=False, analytic_lens=False, all_roots=False, one_lane=False, three_launches=False, device=0):
    """Pulse-echo travel times tx -> lens -> pipe -> lens -> rx by root-finding x_land(alpha) = x_rx — the
    replacement for the reference's grid scan + tolerance matcher (main_rt.py:479-501).

    Returns tt [G, T, E] (least time over the element's ray paths, NaN if none) and the launch angle
    alpha_root [G, T, E]; with all_roots also (tt_all, alpha_all) [G, T, E, 4] in ascending alpha and
    n_roots [G, T, E].  ``true_tangent`` / ``analytic_lens`` switch on the physically-correct variants.
    ``one_lane``: refine every bracket by one lane whatever the size of the call (RTUS_SOLVE_ONE_LANE; calls of up to 32,768
    (row, element) pairs otherwise use three lanes per bracket — same tolerances, other last bits).
    """
    p = _resolve(params)
    x_a, z_a = _f64(x_a, "x_a"), _f64(z_a, "z_a")
    alpha, x_rx = _f64(alpha, "alpha"), _f64(x_rx, "x_rx")
    if x_a.shape != z_a.shape:
        raise ValueError("x_a and z_a must have the same length")
    if alpha.size < 2:
        raise ValueError("Curve needs at least two points.")
    if not np.all(np.diff(alpha) > 0):
        raise ValueError("alpha must be strictly ascending (its intervals are the root brackets)")
    geoms = (np.asarray([[p.r_outer, p.pipe_offset]], dtype=np.float64) if geoms is None
             else _f64(geoms, "geoms", 2))
    G, T, E = geoms.shape[0], x_a.size, x_rx.size
    z_land = p.d if z_land is None else float(z_land)
    tt = np.empty((G, T, E)); ar = np.empty((G, T, E))
    ta = np.empty((G, T, E, MAX_ROOTS)) if all_roots else None
    aa = np.empty((G, T, E, MAX_ROOTS)) if all_roots else None
    nr = np.empty((G, T, E), dtype=np.uint8) if all_roots else None
    lens = p.lens()
    st = _lib.lib().rtus_solve(C.byref(lens), _ptr(geoms), G, _ptr(x_a), _ptr(z_a), T, _ptr(alpha), alpha.size,
                               _ptr(x_rx), E, z_land, _ptr(tt), _ptr(ar), _ptr(ta), _ptr(aa), _ptr(nr),
                               _flags(fast, true_tangent, analytic_lens) | (SOLVE_ONE_LANE if one_lane else 0) | (SOLVE_THREE_LAUNCHES if three_launches else 0),
                               int(device))
    _lib.check(st, "rtus_solve")
    return (tt, ar, ta, aa, nr) if all_roots else (tt, ar)


def travel_time_surface(x0, dx, zs, c1, c2, xe, ze, xf, zf, *, return_entry=False, out=None, device=0):
    """Element x focal-point Fermat travel times through ONE curved interface given as a sampled depth profile -> tt[n_e, n_f].

    The interface is the natural cubic spline through ``zs[k]`` at ``x0 + k*dx`` (z down); speed ``c1`` above it (couplant),
    ``c2`` below it (part).  An entry is the least travel time over the interior local minima of
    T(x) = |E - S(x)|/c1 + |S(x) - F|/c2 — the first-arriving ray obeying Snell's law at the surface — and NaN without one
    (total internal reflection, a minimum outside the extent), for an element not strictly above the whole profile, or for a
    focal point outside the extent or not below the surface.  Occlusion is not checked.  ``return_entry``: also the x of the
    winning entry point, -> (tt, x_entry).  ``out``: optional float64 [n_e, n_f] result buffer.  The table feeds
    focal_delays / tfm_image as it is.  Definition and guarantee: include/rtus.h (rtus_tt_surface).

    NOT in the reference (no measured profiles there): parity unpinned, see DESIGN.md.
    """
    zs = _f64(zs, "zs")
    xe, ze, xf, zf = _points(xe, ze, xf, zf)
    tt = _out(out, (xe.size, xf.size), np.float64)
    xn = np.empty((xe.size, xf.size), dtype=np.float64) if return_entry else None
    st = _lib.lib().rtus_tt_surface(float(x0), float(dx), _ptr(zs), zs.size, float(c1), float(c2), _ptr(xe), _ptr(ze), xe.size,
                                    _ptr(xf), _ptr(zf), xf.size, _ptr(tt), _ptr(xn), int(device))
    _lib.check(st, "rtus_tt_surface")
    return (tt, xn) if return_entry else tt


def focal_delays(tt, *, out=None, device=0):
    """Transmit focal law from a travel-time table tt[n_elem, n_focal]: the delay each element must be fired with so that
    all wavefronts reach the focal point together, delays[e, f] = max_e' tt[e', f] - tt[e, f] (elements without a ray
    path — NaN — are ignored by the maximum and stay NaN).  SURVEY 8(f) row 4; rtus_focal_delays on the GPU."""
    tt = np.ascontiguousarray(tt, dtype=np.float64)
    if tt.ndim != 2:
        raise ValueError("tt must be [n_elem, n_focal]")
    d = _out(out, tt.shape, np.float64)
    st = _lib.lib().rtus_focal_delays(_ptr(tt), tt.shape[0], tt.shape[1], _ptr(d), int(device))
    _lib.check(st, "rtus_focal_delays")
    return d


def tfm_image(fmc, fs, tt_tx, tt_rx=None, *, t0=0.0, out=None, device=0):
    """Total-focusing-method delay-and-sum over full-matrix-capture data: image[f] = sum over (tx, rx) of the A-scan
    fmc[tx, rx, :] (float32, ``fs`` samples per second, first sample at time ``t0``) linearly interpolated at
    tt_tx[tx, f] + tt_rx[rx, f]; tt_rx defaults to tt_tx (same aperture transmits and receives).  The travel-time tables
    are what travel_time_layers / travel_time_lens return.  Pairs without a ray path (NaN) contribute nothing; samples
    outside a record count as zero.  -> float32 [n_focal].  SURVEY 8(f) row 4; not in the reference."""
    fmc = np.ascontiguousarray(fmc, dtype=np.float32)
    if fmc.ndim != 3:
        raise ValueError("fmc must be [n_tx, n_rx, n_t]")
    tt_tx = np.ascontiguousarray(tt_tx, dtype=np.float64)
    same = tt_rx is None or tt_rx is tt_tx
    tt_rx = tt_tx if same else np.ascontiguousarray(tt_rx, dtype=np.float64)
    if tt_tx.ndim != 2 or tt_rx.ndim != 2 or tt_tx.shape[1] != tt_rx.shape[1]:
        raise ValueError("tt_tx / tt_rx must be [n_tx, n_focal] / [n_rx, n_focal]")
    if tt_tx.shape[0] != fmc.shape[0] or tt_rx.shape[0] != fmc.shape[1]:
        raise ValueError("fmc's first two dimensions must match the rows of tt_tx and tt_rx")
    img = _out(out, (tt_tx.shape[1],), np.float32)
    st = _lib.lib().rtus_tfm(_ptr(fmc), fmc.shape[0], fmc.shape[1], fmc.shape[2], float(fs), float(t0), _ptr(tt_tx), _ptr(tt_rx),
                             tt_tx.shape[1], _ptr(img), int(device))
    _lib.check(st, "rtus_tfm")
    return img


def fmc_analytic(fmc, n_taps=63, *, out=None, device=0):
    """Analytic signal of every A-scan of an FMC block by an FIR Hilbert transformer -> complex64 [n_tx, n_rx, n_t]:
    real part = the A-scan, imaginary part = sum_m h[m] x[n - m] with h[m] = 2/(pi m) * Hamming(m) for odd m and 0 for even m,
    ``n_taps`` = 2M + 1 odd in [3, 255]; samples outside the record count as zero.  The envelope is ``np.abs`` of the result.
    Definition: include/rtus.h (rtus_fmc_analytic).  Not in the reference."""
    fmc = np.ascontiguousarray(fmc, dtype=np.float32)
    if fmc.ndim != 3:
        raise ValueError("fmc must be [n_tx, n_rx, n_t]")
    a = _out(out, fmc.shape, np.complex64)
    st = _lib.lib().rtus_fmc_analytic(_ptr(fmc), fmc.shape[0], fmc.shape[1], fmc.shape[2], int(n_taps), _ptr(a), int(device))
    _lib.check(st, "rtus_fmc_analytic")
    return a


def _depths(z_lo, z_hi, dz):
    """number of depths z_lo + j dz up to z_hi (inclusive, to within 1e-9 dz)"""
    if not (np.isfinite(z_lo) and np.isfinite(z_hi) and np.isfinite(dz) and dz > 0 and z_hi >= z_lo):
        raise ValueError("need finite z_lo <= z_hi and dz > 0")
    return int(np.floor((z_hi - z_lo) / dz + 1e-9)) + 1


def surface_profile(x0, dx, z_peak, amp, threshold=0.1):
    """The post-processing of measure_surface on the host: valid = finite z_peak and amp >= threshold * max amp; trimmed to the
    first through last valid column; interior invalid columns filled by linear interpolation in x between the nearest valid ones.
    -> dict(x0, dx, zs, valid).  ValueError when fewer than 4 columns remain."""
    z_peak = np.asarray(z_peak, dtype=np.float64)
    amp = np.asarray(amp, dtype=np.float64)
    fin = np.isfinite(amp)
    top = amp[fin].max() if fin.any() else np.nan
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(z_peak) & fin & (amp >= threshold * top)
    idx = np.nonzero(valid)[0]
    if idx.size == 0 or idx[-1] - idx[0] + 1 < 4:
        raise ValueError(f"the surface was found in too few columns ({idx.size} valid; a profile needs 4 after trimming)")
    lo, hi = int(idx[0]), int(idx[-1])
    k = np.arange(lo, hi + 1)
    zs = np.interp(x0 + k * dx, x0 + idx * dx, z_peak[idx])
    zs[valid[lo:hi + 1]] = z_peak[lo:hi + 1][valid[lo:hi + 1]]        # (the valid columns exactly as measured)
    return dict(x0=float(x0 + lo * dx), dx=float(dx), zs=zs, valid=valid)


def measure_surface(fmc, fs, xe, ze, c1, x0, dx, n_s, z_lo, z_hi, dz, *, t0=0.0, threshold=0.1, n_taps=63, analytic=None,
                    return_image=False, device=0):
    """The surface profile under the couplant, measured from a square FMC block fmc[n_e, n_e, n_t] (element e transmits and
    receives; first sample at ``t0``, ``fs`` samples per second): an envelope TFM of the couplant (speed ``c1``, straight rays) over
    the columns x0 + k dx (k < n_s) and the depths z_lo + j dz up to z_hi, and in every column the depth of the brightest pixel,
    refined by a parabolic step (rtus_surface_find; definition and limits in include/rtus.h).  ``analytic``: an analytic FMC
    from fmc_analytic to re-use (fmc is then not read); otherwise it is formed with ``n_taps`` Hilbert taps.

    Post-processing (host): a column is valid where its peak lies inside the depth window and its amplitude is at least
    ``threshold`` times the largest; the profile is trimmed to the first through last valid column, and interior invalid columns
    are filled by linear interpolation in x.  ValueError when fewer than 4 columns remain.
    -> dict(x0, dx, zs: the profile for travel_time_surface, z_peak [n_s], amplitude [n_s], valid [n_s] bool, image [n_s, n_z]
    float32 when ``return_image``).

    The measurement assumes an aperture without grating lobes (pitch below half a wavelength in the couplant), a window that
    holds the surface echo and no other strong echo, and moderate slopes; dim columns are unreliable, hence the threshold."""
    if analytic is None:
        analytic = fmc_analytic(fmc, n_taps, device=device)
    a = np.ascontiguousarray(analytic)
    if a.dtype == np.float32 and a.ndim == 4 and a.shape[3] == 2:
        a = a.view(np.complex64)[..., 0]
    if a.dtype != np.complex64 or a.ndim != 3 or a.shape[0] != a.shape[1]:
        raise ValueError("the analytic FMC must be complex64 [n_e, n_e, n_t] (or float32 [n_e, n_e, n_t, 2])")
    xe, ze = _f64(xe, "xe"), _f64(ze, "ze")
    if xe.size != a.shape[0] or ze.size != a.shape[0]:
        raise ValueError("xe / ze must hold one position per element of the FMC")
    n_s, n_z = int(n_s), _depths(z_lo, z_hi, dz)
    z_peak = np.empty(n_s, dtype=np.float64)
    amp = np.empty(n_s, dtype=np.float32)
    img = np.empty((n_s, n_z), dtype=np.float32) if return_image else None
    st = _lib.lib().rtus_surface_find(_ptr(a), a.shape[0], a.shape[2], float(fs), float(t0), _ptr(xe), _ptr(ze), float(c1), float(x0),
                                      float(dx), n_s, float(z_lo), float(dz), n_z, _ptr(z_peak), _ptr(amp), _ptr(img), int(device))
    _lib.check(st, "rtus_surface_find")
    r = surface_profile(x0, dx, z_peak, amp, threshold)
    r.update(z_peak=z_peak, amplitude=amp)
    if return_image:
        r["image"] = img
    return r


def _complex_fmc(a):
    """complex64 [n_tx, n_rx, n_t] (a float32 [..., 2] array is viewed as one)"""
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32 and a.ndim == 4 and a.shape[3] == 2:
        a = a.view(np.complex64)[..., 0]
    if a.dtype != np.complex64 or a.ndim != 3:
        raise ValueError("the analytic FMC must be complex64 [n_tx, n_rx, n_t] (or float32 [n_tx, n_rx, n_t, 2])")
    return a


def _tfm_tables(a, tt_tx, tt_rx):
    """the tables of tfm_analytic / tfm_phase against the analytic FMC ``a`` -> (tt_tx, tt_rx, n_f)"""
    tt_tx = np.ascontiguousarray(tt_tx, dtype=np.float64)
    same = tt_rx is None or tt_rx is tt_tx
    tt_rx = tt_tx if same else np.ascontiguousarray(tt_rx, dtype=np.float64)
    if tt_tx.ndim != 2 or tt_rx.ndim != 2 or tt_tx.shape[1] != tt_rx.shape[1]:
        raise ValueError("tt_tx / tt_rx must be [n_tx, n_focal] / [n_rx, n_focal]")
    if tt_tx.shape[0] != a.shape[0] or tt_rx.shape[0] != a.shape[1]:
        raise ValueError("the analytic FMC's first two dimensions must match the rows of tt_tx and tt_rx")
    return tt_tx, tt_rx, tt_tx.shape[1]


COHERENCE = ("cf", "vcf", "scf")


def _coherence(coherence):
    """the ``coherence=`` keyword of tfm_analytic / pwi_image / tfm_views -> None, "cf", "vcf" or "scf" (True is "cf")"""
    if isinstance(coherence, str):
        if coherence not in COHERENCE:
            raise ValueError(f"unknown coherence factor {coherence!r}: False, True or one of {COHERENCE}")
        return coherence
    if coherence is None or isinstance(coherence, (bool, np.bool_)):
        return "cf" if coherence else None
    raise ValueError(f"coherence must be False, True or one of {COHERENCE}")


def tfm_analytic(analytic, fs, tt_tx, tt_rx=None, *, t0=0.0, coherence=False, out=None, device=0):
    """Envelope TFM: tfm_image's delay-and-sum over an analytic FMC (complex64 [n_tx, n_rx, n_t], e.g. from fmc_analytic, or float32
    [n_tx, n_rx, n_t, 2]) through any travel-time table of this library; tt_rx defaults to tt_tx.  Real and imaginary parts are
    interpolated separately with tfm_image's sample positions, edge rules and order, so ``image.real`` is tfm_image of
    ``analytic.real`` bit for bit (and ``image.imag`` of ``analytic.imag``).  The envelope is ``np.abs(image)``.
    -> complex64 image [n_f]; with ``coherence=True`` -> (image, cf float32 [n_f]): the coherence factor |S|^2 / (N E) of every
    focal point (Mallart & Fink; S the complex sum, E the sum of |sample|^2 over the N = T R pairs whose legs both have a path; NaN
    when N = 0).  A CF-weighted image is ``np.abs(image) * cf**p`` (p = 1 is usual).  ``coherence="cf"`` is the same as True;
    ``"vcf"`` / ``"scf"`` -> (image, that phase-coherence factor of tfm_phase): the same image bits.  Definition: include/rtus.h
    (rtus_tfm_analytic, rtus_tfm_phase).  Not in the reference."""
    mode = _coherence(coherence)
    if mode in ("vcf", "scf"):
        r = _tfm_phase(analytic, fs, tt_tx, tt_rx, t0, (mode,), False, out, device)
        return r["image"], r[mode]
    a = _complex_fmc(analytic)
    tt_tx, tt_rx, n_f = _tfm_tables(a, tt_tx, tt_rx)
    img = _out(out, (n_f,), np.complex64)
    cf = np.empty(n_f, dtype=np.float32) if mode else None
    st = _lib.lib().rtus_tfm_analytic(_ptr(a), a.shape[0], a.shape[1], a.shape[2], float(fs), float(t0), _ptr(tt_tx), _ptr(tt_rx),
                                      n_f, _ptr(img), _ptr(cf), int(device))
    _lib.check(st, "rtus_tfm_analytic")
    return (img, cf) if mode else img


# ---------------------------------------------------------------------------------------------- carrier-aware (IQ) interpolation
def _f_demod(f_demod, fs):
    """the carrier frequency of tfm_iq against the sampling rate -> float; ValueError unless 0 <= f_demod < fs / 2"""
    f_demod, fs = float(f_demod), float(fs)
    if not (np.isfinite(fs) and fs > 0.0):
        raise ValueError("fs must be finite and positive")
    if not (np.isfinite(f_demod) and 0.0 <= f_demod < 0.5 * fs):
        raise ValueError(f"f_demod must be finite with 0 <= f_demod < fs / 2 (got {f_demod!r} at fs = {fs!r})")
    return f_demod


def _iq_coherence(coherence):
    """the ``coherence=`` keyword of tfm_iq / tfm_iq_hmc -> None or "cf"; "vcf" / "scf" raise ValueError"""
    mode = _coherence(coherence)
    if mode in ("vcf", "scf"):
        raise ValueError(f"coherence={mode!r} is not available with carrier-aware interpolation (tfm_phase has no such form): use 'cf'")
    return mode


def centre_frequency(fmc, fs):
    """The centre frequency of FMC (or HMC) data [..., n_t], real or analytic -> float [Hz]: the power-weighted mean frequency of
    the mean periodogram of the A-scans over the positive bins (0 < f < fs / 2).  Host NumPy; an ``f_demod`` for tfm_iq taken from
    the data.  It need not be exact: an f_demod 10 % off the carrier costs 0.2 % of a TFM peak at 4 samples per cycle (0.995
    against 0.997 of the ideal sum at fs = 20 MHz, f0 = 5 MHz; less at higher rates: DESIGN.md §4 "Carrier-aware interpolation"),
    where linear interpolation costs 19 %."""
    a = np.asarray(fmc)
    if a.ndim < 1 or a.shape[-1] < 4 or a.size == 0:
        raise ValueError("need A-scans [..., n_t] of at least 4 samples")
    fs = float(fs)
    if not (np.isfinite(fs) and fs > 0.0):
        raise ValueError("fs must be finite and positive")
    n_t = a.shape[-1]
    a = a.reshape(-1, n_t)
    power = np.zeros(n_t, dtype=np.float64)
    for k in range(0, a.shape[0], 1024):                             # (blocks: the spectrum of a large FMC is not held at once)
        power += (np.abs(np.fft.fft(a[k:k + 1024], axis=-1)) ** 2).sum(axis=0)
    f = np.fft.fftfreq(n_t, 1.0 / fs)
    pos = (f > 0.0) & (f < 0.5 * fs)
    total = power[pos].sum()
    if not (np.isfinite(total) and total > 0.0):
        raise ValueError("the data have no power in the positive bins")
    return float((f[pos] * power[pos]).sum() / total)


def tfm_iq(analytic, fs, f_demod, tt_tx, tt_rx=None, *, t0=0.0, coherence=False, out=None, device=0):
    """Envelope TFM with carrier-aware (IQ) interpolation: tfm_analytic's inputs, layouts, positions, edge rules, order and returns,
    with the two neighbouring samples combined as baseband samples — the second turned back by one sample of the carrier
    ``f_demod`` [Hz] (0 <= f_demod < fs / 2), the two interpolated linearly, the carrier put back exactly at the fraction.  Linear
    interpolation of the analytic signal itself loses up to 1 - cos(pi f0 / fs) per term (29 % at 4 samples per cycle, a TFM
    peak 19 % low, and differently at every pixel); this loses 0.5 % per term there and 0.3 % of the peak.  ``f_demod = 0`` is
    tfm_analytic bit for bit.  ``f_demod`` may come from centre_frequency(fmc, fs); 10 % off costs 0.2 %.
    -> complex64 image [n_f]; with ``coherence=True`` or ``"cf"`` -> (image, cf float32 [n_f]).  ``"vcf"`` / ``"scf"`` raise
    ValueError: the phase-coherence kernel has no carrier-aware form.  Definition: include/rtus.h (rtus_tfm_iq).  Not in the
    reference."""
    mode = _iq_coherence(coherence)
    f_demod = _f_demod(f_demod, fs)
    a = _complex_fmc(analytic)
    tt_tx, tt_rx, n_f = _tfm_tables(a, tt_tx, tt_rx)
    img = _out(out, (n_f,), np.complex64)
    cf = np.empty(n_f, dtype=np.float32) if mode else None
    st = _lib.lib().rtus_tfm_iq(_ptr(a), a.shape[0], a.shape[1], a.shape[2], float(fs), float(t0), f_demod, _ptr(tt_tx), _ptr(tt_rx),
                                n_f, _ptr(img), _ptr(cf), int(device))
    _lib.check(st, "rtus_tfm_iq")
    return (img, cf) if mode else img


# ---------------------------------------------------------------------------------------------- a stack of frames
def frames_pack(stack):
    """A frame-major RF stack [n_frames, n_tx, n_rx, n_t] -> its packed layout float32 [n_pairs, n_tx, n_rx, n_t, 2],
    n_pairs = ceil(n_frames / 2): plane 0 of pair p is frame 2 p, plane 1 is frame 2 p + 1; plane 1 of the last pair of an odd stack is
    +0.0.  The layout rtus_tfm_frames_dev reads (include/rtus.h), restated in NumPy; device.fmc_pack_frames_dev makes it on the GPU."""
    stack = np.asarray(stack, dtype=np.float32)
    if stack.ndim != 4 or stack.shape[0] < 1:
        raise ValueError("the stack must be [n_frames, n_tx, n_rx, n_t] with at least one frame")
    n_frames = stack.shape[0]
    packed = np.zeros(((n_frames + 1) // 2,) + stack.shape[1:] + (2,), dtype=np.float32)
    packed[..., 0] = stack[0::2]
    packed[:n_frames // 2, ..., 1] = stack[1::2]
    return packed


def frames_unpack(packed, n_frames):
    """The packed layout [n_pairs, n_tx, n_rx, n_t, 2] -> the frame-major stack float32 [n_frames, n_tx, n_rx, n_t]; ``n_frames`` is
    2 n_pairs or 2 n_pairs - 1 (the second plane of the last pair is then dropped)."""
    packed = np.asarray(packed, dtype=np.float32)
    n_frames = int(n_frames)
    if packed.ndim != 5 or packed.shape[4] != 2 or packed.shape[0] < 1:
        raise ValueError("the packed stack must be [n_pairs, n_tx, n_rx, n_t, 2]")
    if (n_frames + 1) // 2 != packed.shape[0] or n_frames < 1:
        raise ValueError(f"{packed.shape[0]} pairs hold {2 * packed.shape[0] - 1} or {2 * packed.shape[0]} frames, not {n_frames}")
    stack = np.empty((n_frames,) + packed.shape[1:4], dtype=np.float32)
    stack[0::2] = packed[..., 0]
    stack[1::2] = packed[:n_frames // 2, ..., 1]
    return stack


def frames_pack_i16(stack):
    """A frame-major int16 stack [n_frames, n_tx, n_rx, n_t] -> its packed layout int16 [n_quads, n_tx, n_rx, n_t, 4],
    n_quads = ceil(n_frames / 4): plane c of quad q is frame 4 q + c; the planes of the absent frames of the last quad are 0.  The
    layout rtus_tfm_frames_i16_dev reads (include/rtus.h), restated in NumPy; device.fmc_pack_frames_i16_dev makes it on the GPU."""
    stack = np.asarray(stack)
    if stack.dtype != np.int16 or stack.ndim != 4 or stack.shape[0] < 1:
        raise ValueError("the stack must be int16 [n_frames, n_tx, n_rx, n_t] with at least one frame")
    n_frames = stack.shape[0]
    packed = np.zeros(((n_frames + 3) // 4,) + stack.shape[1:] + (4,), dtype=np.int16)
    for c in range(4):
        packed[:(n_frames - c + 3) // 4, ..., c] = stack[c::4]
    return packed


def frames_unpack_i16(packed, n_frames):
    """The packed layout int16 [n_quads, n_tx, n_rx, n_t, 4] -> the frame-major stack int16 [n_frames, n_tx, n_rx, n_t];
    ``n_frames`` is in [4 n_quads - 3, 4 n_quads] (the planes past it in the last quad are dropped)."""
    packed = np.asarray(packed)
    n_frames = int(n_frames)
    if packed.dtype != np.int16 or packed.ndim != 5 or packed.shape[4] != 4 or packed.shape[0] < 1:
        raise ValueError("the packed stack must be int16 [n_quads, n_tx, n_rx, n_t, 4]")
    if (n_frames + 3) // 4 != packed.shape[0] or n_frames < 1:
        raise ValueError(f"{packed.shape[0]} quads hold {4 * packed.shape[0] - 3} to {4 * packed.shape[0]} frames, not {n_frames}")
    stack = np.empty((n_frames,) + packed.shape[1:4], dtype=np.int16)
    for c in range(4):
        stack[c::4] = packed[:(n_frames - c + 3) // 4, ..., c]
    return stack


def _max_frames(max_frames, n_frames):
    """the ``max_frames=`` keyword of tfm_frames -> frames per call"""
    if max_frames is None:
        return n_frames
    if isinstance(max_frames, (bool, np.bool_)) or int(max_frames) != max_frames or int(max_frames) < 1:
        raise ValueError("max_frames must be a positive integer or None")
    return min(int(max_frames), n_frames)


def tfm_frames(stack, fs, tt_tx, tt_rx=None, *, t0=0.0, envelope=False, coherence=False, f_demod=None, n_taps=63, max_frames=None,
               out=None, device=0, hmc=False):
    """TFM over a stack of frames — an encoded scan: ``stack`` float32 [n_frames, n_tx, n_rx, n_t], every frame imaged through the
    same tables on the same grid -> float32 [n_frames, n_f]; row k is tfm_image(stack[k], ...) bit for bit.  The frames are paired
    on the device and each pair imaged by one 16-byte gather per (tx, rx, focal point), all pairs in one call (rtus_tfm_frames).
    A stack of dtype int16 (without ``envelope``) is uploaded as int16 and imaged four frames per gather (rtus_tfm_frames_i16): half
    the upload and the device memory, the bits of the float32 call on the same samples.
    ``envelope=True``: the analytic stack is formed first (fmc_analytic over the n_frames n_tx transmit rows, ``n_taps`` Hilbert
    taps) and imaged by rtus_tfm_analytic_frames -> complex64 [n_frames, n_f], row k = tfm_analytic(fmc_analytic(stack[k])) bit for
    bit; with ``coherence=True`` (or "cf") -> (images, cf float32 [n_frames, n_f]).  ``f_demod`` [Hz] as on tfm_views: the frames go
    through tfm_iq's carrier-aware interpolation instead; it needs ``envelope=True``.  "vcf" / "scf" have no stack form (ValueError).
    ``max_frames``: the stack is run in chunks of that many frames, which bounds device memory; no bit depends on it.  ``out``:
    the images' buffer.
    ``hmc=True``: every frame is a half-matrix capture — ``stack`` [n_frames, n_pairs, n_t], int16 or float32 (other dtypes go to
    float32), the records in hmc_index's order; tt_tx / tt_rx [n_e, n_f], ``tt_rx`` None or ``tt_tx`` itself means one table (one
    gather per record).  Row k is tfm_hmc(stack[k] as float32, ...) bit for bit; int16 frames go four per gather
    (rtus_tfm_frames_hmc_i16), float32 frames two (rtus_tfm_frames_hmc).  The packed layouts the device entries read are
    frames_pack_i16(stack[:, None])[:, 0] and frames_pack(stack[:, None])[:, 0]; device.fmc_pack_frames[_i16]_dev make them on the
    GPU from a [n_frames, 1, n_pairs, n_t] view.  ``envelope``, ``coherence`` and ``f_demod`` raise ValueError with ``hmc=True``:
    envelope images of a half-matrix stack are tfm_envelope_frames' (which forms the analytic signal on the device).
    Definition: include/rtus.h (rtus_tfm_frames, rtus_tfm_analytic_frames, rtus_tfm_frames_hmc).  Not in the reference."""
    if hmc:
        return _tfm_frames_hmc(stack, fs, tt_tx, tt_rx, t0, envelope, coherence, f_demod, max_frames, out, device)
    mode = _iq_coherence(coherence)
    if mode and not envelope:
        raise ValueError("the coherence factor needs envelope=True")
    if f_demod is not None:
        if not envelope:
            raise ValueError("f_demod (carrier-aware interpolation) needs envelope=True")
        f_demod = _f_demod(f_demod, fs)
    i16 = not envelope and getattr(stack, "dtype", None) == np.int16   # (fmc_analytic needs float32: an envelope stack is widened)
    stack = np.ascontiguousarray(stack, dtype=np.int16 if i16 else np.float32)
    if stack.ndim != 4 or stack.shape[0] < 1:
        raise ValueError("the stack must be [n_frames, n_tx, n_rx, n_t] with at least one frame")
    n_frames, n_tx, n_rx, n_t = stack.shape
    tt_tx, tt_rx, n_f = _tfm_tables(stack[0], tt_tx, tt_rx)
    per = _max_frames(max_frames, n_frames)
    if envelope and (int(n_taps) != n_taps or not 3 <= int(n_taps) <= 255 or not int(n_taps) & 1):
        raise ValueError("n_taps must be odd in [3, 255]")
    imgs = _out(out, (n_frames, n_f), np.complex64 if envelope else np.float32)
    cf = np.empty((n_frames, n_f), dtype=np.float32) if mode else None
    L = _lib.lib()
    for k in range(0, n_frames, per):
        n = min(per, n_frames - k)
        if not envelope:
            entry = "rtus_tfm_frames_i16" if i16 else "rtus_tfm_frames"
            st = getattr(L, entry)(_ptr(stack[k:k + n]), n, n_tx, n_rx, n_t, float(fs), float(t0), _ptr(tt_tx), _ptr(tt_rx), n_f,
                                   _ptr(imgs[k:k + n]), int(device))
            _lib.check(st, entry)
            continue
        a = fmc_analytic(stack[k:k + n].reshape(n * n_tx, n_rx, n_t), n_taps, device=device)
        st = L.rtus_tfm_analytic_frames(_ptr(a), n, n_tx, n_rx, n_t, float(fs), float(t0), 0.0 if f_demod is None else f_demod,
                                        _ptr(tt_tx), _ptr(tt_rx), n_f, _ptr(imgs[k:k + n]), None if cf is None else _ptr(cf[k:k + n]),
                                        int(device))
        _lib.check(st, "rtus_tfm_analytic_frames")
    return (imgs, cf) if mode else imgs


def _tfm_frames_hmc(stack, fs, tt_tx, tt_rx, t0, envelope, coherence, f_demod, max_frames, out, device):
    """tfm_frames(hmc=True): a stack of half-matrix frames [n_frames, n_pairs, n_t], int16 or float32"""
    if envelope or coherence or f_demod is not None:
        raise ValueError("hmc=True images RF frames only: envelope, coherence and f_demod have no stacked half-matrix form "
                         "(use tfm_analytic_hmc / tfm_iq_hmc frame by frame)")
    i16 = getattr(stack, "dtype", None) == np.int16
    stack = np.ascontiguousarray(stack, dtype=np.int16 if i16 else np.float32)
    if stack.ndim != 3 or stack.shape[0] < 1:
        raise ValueError("with hmc=True the stack must be [n_frames, n_pairs, n_t] with at least one frame")
    n_frames, n_pairs, n_t = stack.shape
    n_e, tt_tx, tt_rx, n_f = _hmc_tables(n_pairs, tt_tx, tt_rx)
    per = _max_frames(max_frames, n_frames)
    imgs = _out(out, (n_frames, n_f), np.float32)
    entry = "rtus_tfm_frames_hmc_i16" if i16 else "rtus_tfm_frames_hmc"
    fn = getattr(_lib.lib(), entry)
    for k in range(0, n_frames, per):
        n = min(per, n_frames - k)
        st = fn(_ptr(stack[k:k + n]), n, n_e, n_t, float(fs), float(t0), _ptr(tt_tx), _ptr(tt_rx), n_f, _ptr(imgs[k:k + n]), int(device))
        _lib.check(st, entry)
    return imgs


ENV_MAGNITUDE = 1                                                     # RTUS_ENV_MAGNITUDE (include/rtus.h)


def _n_taps(n_taps):
    """the Hilbert transformer's length -> int; ValueError unless odd in [3, 255]"""
    if isinstance(n_taps, (bool, np.bool_)) or int(n_taps) != n_taps or not 3 <= int(n_taps) <= 255 or not int(n_taps) & 1:
        raise ValueError("n_taps must be odd in [3, 255]")
    return int(n_taps)


def fmc_analytic_i16(fmc_i16, n_taps=63, *, out=None, device=0):
    """fmc_analytic on int16 samples [n_tx, n_rx, n_t], uploaded as int16 -> complex64 [n_tx, n_rx, n_t] with fmc_analytic's bits on
    the samples as float32.  Definition: include/rtus.h (rtus_fmc_analytic_i16).  Not in the reference."""
    fmc = np.ascontiguousarray(fmc_i16)
    if fmc.dtype != np.int16 or fmc.ndim != 3:
        raise ValueError("fmc_i16 must be int16 [n_tx, n_rx, n_t]")
    a = _out(out, fmc.shape, np.complex64)
    st = _lib.lib().rtus_fmc_analytic_i16(_ptr(fmc), fmc.shape[0], fmc.shape[1], fmc.shape[2], int(n_taps), _ptr(a), int(device))
    _lib.check(st, "rtus_fmc_analytic_i16")
    return a


def tfm_envelope_frames(stack, fs, tt_tx, tt_rx=None, *, t0=0.0, n_taps=63, coherence=False, f_demod=None, magnitude=False,
                        max_frames=None, out=None, device=0):
    """Envelope TFM over a stack of half-matrix frames in one call: ``stack`` [n_frames, n_pairs, n_t], int16 or float32 (other
    dtypes go to float32), the records in hmc_index's order; tt_tx / tt_rx [n_e, n_f], ``tt_rx`` None or ``tt_tx`` itself means one
    table.  The raw samples are uploaded in their own type and the analytic signal (``n_taps`` Hilbert taps) is formed on the device
    -> complex64 [n_frames, n_f]; row k is tfm_analytic_hmc(hmc_analytic(stack[k] as float32, n_taps), ...) bit for bit, with
    ``f_demod`` [Hz] tfm_iq_hmc's.  ``coherence=True`` (or "cf") -> (images, cf float32 [n_frames, n_f]), the same images; "vcf" /
    "scf" raise ValueError.  ``magnitude=True`` -> float32 [n_frames, n_f] instead: the magnitude of the complex images
    (np.sqrt(re.astype(f8)**2 + im.astype(f8)**2).astype(f4): one rounding in the sum, one in the conversion), formed
    on the device (half the download).  ``max_frames``: the stack is run in chunks of that many frames, which bounds device memory;
    no bit depends on it, nor on the dtype's route (int16 frames without ``f_demod`` and ``coherence`` are imaged plane by plane:
    three gathers per record and four frames, not four).  ``out``: the images' buffer.
    Definition: include/rtus.h (rtus_tfm_envelope_frames_hmc).  Not in the reference."""
    mode = _iq_coherence(coherence)
    f_demod = 0.0 if f_demod is None else _f_demod(f_demod, fs)
    n_taps = _n_taps(n_taps)
    i16 = getattr(stack, "dtype", None) == np.int16
    stack = np.ascontiguousarray(stack, dtype=np.int16 if i16 else np.float32)
    if stack.ndim != 3 or stack.shape[0] < 1:
        raise ValueError("the stack must be [n_frames, n_pairs, n_t] with at least one frame")
    n_frames, n_pairs, n_t = stack.shape
    n_e, tt_tx, tt_rx, n_f = _hmc_tables(n_pairs, tt_tx, tt_rx)
    per = _max_frames(max_frames, n_frames)
    imgs = _out(out, (n_frames, n_f), np.float32 if magnitude else np.complex64)
    cf = np.empty((n_frames, n_f), dtype=np.float32) if mode else None
    entry = "rtus_tfm_envelope_frames_hmc_i16" if i16 else "rtus_tfm_envelope_frames_hmc"
    fn = getattr(_lib.lib(), entry)
    for k in range(0, n_frames, per):
        n = min(per, n_frames - k)
        st = fn(_ptr(stack[k:k + n]), n, n_e, n_t, n_taps, float(fs), float(t0), f_demod, _ptr(tt_tx), _ptr(tt_rx), n_f,
                ENV_MAGNITUDE if magnitude else 0, _ptr(imgs[k:k + n]), None if cf is None else _ptr(cf[k:k + n]), int(device))
        _lib.check(st, entry)
    return (imgs, cf) if mode else imgs


# ---------------------------------------------------------------------------------------------- half-matrix capture
def _hmc_elements(n_pairs):
    """n_e with n_e (n_e + 1) / 2 == n_pairs; ValueError when n_pairs is not a triangular number"""
    n_e = (int(np.sqrt(8.0 * n_pairs + 1.0)) - 1) // 2
    for n in (n_e - 1, n_e, n_e + 1):
        if n >= 1 and n * (n + 1) // 2 == n_pairs:
            return n
    raise ValueError(f"a half-matrix capture holds n_e (n_e + 1) / 2 records: {n_pairs} is not a triangular number")


def hmc_index(n_e):
    """The (i, j) of every record of a half-matrix capture of ``n_e`` elements, in packed order -> two int arrays [n_pairs]:
    0 <= i <= j < n_e, record (i, j) at p = i n_e - i (i - 1) / 2 + (j - i) — numpy.triu_indices' order."""
    n_e = int(n_e)
    if n_e < 1:
        raise ValueError("need n_e >= 1")
    return np.triu_indices(n_e)


def hmc_pack(fmc, mode="upper"):
    """A square FMC block [n_e, n_e, n_t] (real or complex) -> its half-matrix capture [n_pairs, n_t] in hmc_index's order.
    ``mode="upper"`` keeps fmc[i, j] for i <= j; ``"mean"`` stores (fmc[i, j] + fmc[j, i]) * 0.5 in the block's precision (float32 /
    complex64): the reciprocal pairs averaged."""
    fmc = np.asarray(fmc)
    if fmc.ndim != 3 or fmc.shape[0] != fmc.shape[1]:
        raise ValueError("fmc must be a square block [n_e, n_e, n_t]")
    if mode not in ("upper", "mean"):
        raise ValueError(f"unknown mode {mode!r}: 'upper' or 'mean'")
    fmc = fmc.astype(np.complex64 if np.iscomplexobj(fmc) else np.float32, copy=False)
    i, j = hmc_index(fmc.shape[0])
    if mode == "upper":
        return np.ascontiguousarray(fmc[i, j])
    return np.ascontiguousarray((fmc[i, j] + fmc[j, i]) * np.float32(0.5))


def hmc_unpack(hmc):
    """A half-matrix capture [n_pairs, n_t] -> the symmetric full matrix [n_e, n_e, n_t] (record (i, j) at [i, j] and [j, i])."""
    hmc = np.asarray(hmc)
    if hmc.ndim != 2:
        raise ValueError("hmc must be [n_pairs, n_t]")
    n_e = _hmc_elements(hmc.shape[0])
    i, j = hmc_index(n_e)
    fmc = np.empty((n_e, n_e, hmc.shape[1]), dtype=hmc.dtype)
    fmc[i, j] = hmc
    fmc[j, i] = hmc
    return fmc


def _hmc_tables(n_pairs, tt_tx, tt_rx):
    """the tables of tfm_hmc / tfm_analytic_hmc against a block of n_pairs records -> (n_e, tt_tx, tt_rx, n_f)"""
    n_e = _hmc_elements(n_pairs)
    tt_tx = np.ascontiguousarray(tt_tx, dtype=np.float64)
    same = tt_rx is None or tt_rx is tt_tx
    tt_rx = tt_tx if same else np.ascontiguousarray(tt_rx, dtype=np.float64)
    if tt_tx.ndim != 2 or tt_rx.ndim != 2 or tt_tx.shape[1] != tt_rx.shape[1]:
        raise ValueError("tt_tx / tt_rx must be [n_e, n_focal] both")
    if tt_tx.shape[0] != n_e or tt_rx.shape[0] != n_e:
        raise ValueError(f"{n_pairs} records are a capture of {n_e} elements: tt_tx and tt_rx must have {n_e} rows")
    return n_e, tt_tx, tt_rx, tt_tx.shape[1]


def tfm_hmc(hmc, fs, tt_tx, tt_rx=None, *, t0=0.0, out=None, device=0):
    """tfm_image over a half-matrix capture: ``hmc`` float32 [n_pairs, n_t] holds the A-scans of the pairs i <= j in hmc_index's order
    (hmc_pack makes one from a square block); tt_tx / tt_rx [n_e, n_f], tt_rx defaults to tt_tx.  Each record counts for (i, j) and
    for (j, i): image[f] = sum of a_ii(s_ii) and of a_ij(s_ij) + a_ij(s_ji) for i < j, with tfm_image's positions, interpolation and
    edge rules — tfm_image of hmc_unpack(hmc) up to the order of the fp32 sum.  With one table (tt_rx None or tt_tx itself) every
    record is gathered once and counted twice: half the gathers of tfm_image, and the bits of the two-table call with equal tables.
    -> float32 [n_f].  Definition: include/rtus.h (rtus_tfm_hmc).  Not in the reference."""
    hmc = np.ascontiguousarray(hmc, dtype=np.float32)
    if hmc.ndim != 2:
        raise ValueError("hmc must be [n_pairs, n_t]")
    n_e, tt_tx, tt_rx, n_f = _hmc_tables(hmc.shape[0], tt_tx, tt_rx)
    img = _out(out, (n_f,), np.float32)
    st = _lib.lib().rtus_tfm_hmc(_ptr(hmc), n_e, hmc.shape[1], float(fs), float(t0), _ptr(tt_tx), _ptr(tt_rx), n_f, _ptr(img), int(device))
    _lib.check(st, "rtus_tfm_hmc")
    return img


def _complex_hmc(a):
    """complex64 [n_pairs, n_t] (a float32 [n_pairs, n_t, 2] array is viewed as one)"""
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32 and a.ndim == 3 and a.shape[2] == 2:
        a = a.view(np.complex64)[..., 0]
    if a.dtype != np.complex64 or a.ndim != 2:
        raise ValueError("the analytic capture must be complex64 [n_pairs, n_t] (or float32 [n_pairs, n_t, 2])")
    return a


def tfm_analytic_hmc(analytic_hmc, fs, tt_tx, tt_rx=None, *, t0=0.0, coherence=False, out=None, device=0):
    """tfm_analytic over a half-matrix capture: complex64 [n_pairs, n_t] (hmc_analytic's, or float32 [n_pairs, n_t, 2]) -> complex64
    image [n_f], each plane tfm_hmc of that plane bit for bit; with ``coherence=True`` (or "cf") -> (image, cf float32 [n_f]), the
    coherence factor of tfm_analytic with E summed over both legs of every record.  "vcf" / "scf" raise ValueError here: call
    tfm_phase_hmc, which returns the same image bits with both phase-coherence factors.  Definition: include/rtus.h
    (rtus_tfm_analytic_hmc).  Not in the reference."""
    mode = _coherence(coherence)
    if mode in ("vcf", "scf"):
        raise ValueError(f"coherence={mode!r} is not available from tfm_analytic_hmc: use 'cf', or call tfm_phase_hmc")
    a = _complex_hmc(analytic_hmc)
    n_e, tt_tx, tt_rx, n_f = _hmc_tables(a.shape[0], tt_tx, tt_rx)
    img = _out(out, (n_f,), np.complex64)
    cf = np.empty(n_f, dtype=np.float32) if mode else None
    st = _lib.lib().rtus_tfm_analytic_hmc(_ptr(a), n_e, a.shape[1], float(fs), float(t0), _ptr(tt_tx), _ptr(tt_rx), n_f, _ptr(img),
                                          _ptr(cf), int(device))
    _lib.check(st, "rtus_tfm_analytic_hmc")
    return (img, cf) if mode else img


def tfm_iq_hmc(analytic_hmc, fs, f_demod, tt_tx, tt_rx=None, *, t0=0.0, coherence=False, out=None, device=0):
    """tfm_iq over a half-matrix capture: tfm_analytic_hmc's inputs, layouts, order and returns with tfm_iq's carrier-aware step on
    every gathered pair of samples (one table: every record gathered once and counted twice).  ``f_demod = 0`` is
    tfm_analytic_hmc bit for bit.  "vcf" / "scf" raise ValueError.  Definition: include/rtus.h (rtus_tfm_iq_hmc).  Not in the
    reference."""
    mode = _iq_coherence(coherence)
    f_demod = _f_demod(f_demod, fs)
    a = _complex_hmc(analytic_hmc)
    n_e, tt_tx, tt_rx, n_f = _hmc_tables(a.shape[0], tt_tx, tt_rx)
    img = _out(out, (n_f,), np.complex64)
    cf = np.empty(n_f, dtype=np.float32) if mode else None
    st = _lib.lib().rtus_tfm_iq_hmc(_ptr(a), n_e, a.shape[1], float(fs), float(t0), f_demod, _ptr(tt_tx), _ptr(tt_rx), n_f, _ptr(img),
                                    _ptr(cf), int(device))
    _lib.check(st, "rtus_tfm_iq_hmc")
    return (img, cf) if mode else img


def hmc_analytic(hmc, n_taps=63, *, out=None, device=0):
    """Analytic signal of every A-scan of a half-matrix capture -> complex64 [n_pairs, n_t]: fmc_analytic on the block seen as
    [1, n_pairs, n_t] (the Hilbert transformer works per A-scan; rtus_fmc_analytic limits the number of A-scans, not either
    dimension)."""
    hmc = np.ascontiguousarray(hmc, dtype=np.float32)
    if hmc.ndim != 2:
        raise ValueError("hmc must be [n_pairs, n_t]")
    _hmc_elements(hmc.shape[0])
    a = _out(out, hmc.shape, np.complex64)
    fmc_analytic(hmc[None], n_taps, out=a.reshape(1, *hmc.shape), device=device)
    return a


def tfm_phase(analytic, fs, tt_tx, tt_rx=None, *, t0=0.0, counts=False, out=None, device=0):
    """Phase-coherence imaging (Camacho, Parrilla & Fritsch 2009): tfm_analytic's delay-and-sum — the same arguments, input rules and
    image bits — with the two factors that read only the phase of the aperture data at each focal point:
    ``vcf`` = |sum of the unit phasors p / |p|| / N, the vector coherence factor, and ``scf`` = 1 - sqrt(1 - (B / N)^2), the sign
    coherence factor, B the sum of sign(Re p) over the pairs; N = T R as for tfm_analytic's cf (pairs outside the record count with
    a zero phasor and sign; NaN when N = 0).  Both ignore amplitude: saturated echoes, gain differences between elements.
    -> dict(image complex64 [n_f], vcf float32 [n_f], scf float32 [n_f]); with ``counts=True`` also sign_sum (B) and n_pairs (N),
    int32 [n_f].  A weighted image is ``np.abs(image) * vcf**p`` (or scf).  Definition: include/rtus.h (rtus_tfm_phase).  Not in the
    reference."""
    return _tfm_phase(analytic, fs, tt_tx, tt_rx, t0, ("vcf", "scf"), counts, out, device)


def _tfm_phase(analytic, fs, tt_tx, tt_rx, t0, want, counts, out, device):
    """tfm_phase with only the factors named in ``want`` computed (tfm_analytic(coherence="vcf") asks for one)"""
    a = _complex_fmc(analytic)
    tt_tx, tt_rx, n_f = _tfm_tables(a, tt_tx, tt_rx)
    img = _out(out, (n_f,), np.complex64)
    r = {"image": img}
    for k in want:
        r[k] = np.empty(n_f, dtype=np.float32)
    cnt = np.empty((n_f, 2), dtype=np.int32) if counts else None
    st = _lib.lib().rtus_tfm_phase(_ptr(a), a.shape[0], a.shape[1], a.shape[2], float(fs), float(t0), _ptr(tt_tx), _ptr(tt_rx), n_f,
                                   _ptr(img), _ptr(r.get("vcf")), _ptr(r.get("scf")), _ptr(cnt), int(device))
    _lib.check(st, "rtus_tfm_phase")
    if counts:
        r["sign_sum"], r["n_pairs"] = np.ascontiguousarray(cnt[:, 0]), np.ascontiguousarray(cnt[:, 1])
    return r


def tfm_phase_hmc(analytic_hmc, fs, tt_tx, tt_rx=None, *, t0=0.0, counts=False, out=None, device=0):
    """tfm_phase over a half-matrix capture: tfm_analytic_hmc's inputs (complex64 [n_pairs, n_t] or float32 [n_pairs, n_t, 2];
    tt_tx / tt_rx [n_e, n_f], tt_rx defaults to tt_tx: one table, every record gathered once) and image bits, tfm_phase's returns:
    -> dict(image complex64 [n_f], vcf float32 [n_f], scf float32 [n_f]); with ``counts=True`` also sign_sum (B) and n_pairs (N),
    int32 [n_f].  Every record counts for (i, j) and for (j, i): the unit phasors and signs of its two samples (one on the
    diagonal) go into U and B, N = T R.  sign_sum, n_pairs and scf are tfm_phase's on hmc_unpack(analytic_hmc) bit for bit; vcf
    differs by the order of an fp32 sum.  Definition: include/rtus.h (rtus_tfm_phase_hmc).  Not in the reference."""
    a = _complex_hmc(analytic_hmc)
    n_e, tt_tx, tt_rx, n_f = _hmc_tables(a.shape[0], tt_tx, tt_rx)
    img = _out(out, (n_f,), np.complex64)
    r = {"image": img, "vcf": np.empty(n_f, dtype=np.float32), "scf": np.empty(n_f, dtype=np.float32)}
    cnt = np.empty((n_f, 2), dtype=np.int32) if counts else None
    st = _lib.lib().rtus_tfm_phase_hmc(_ptr(a), n_e, a.shape[1], float(fs), float(t0), _ptr(tt_tx), _ptr(tt_rx), n_f, _ptr(img),
                                       _ptr(r["vcf"]), _ptr(r["scf"]), _ptr(cnt), int(device))
    _lib.check(st, "rtus_tfm_phase_hmc")
    if counts:
        r["sign_sum"], r["n_pairs"] = np.ascontiguousarray(cnt[:, 0]), np.ascontiguousarray(cnt[:, 1])
    return r


def adaptive_tfm(fmc, fs, xe, ze, c1, c2, x0, dx, n_s, z_lo, z_hi, dz, xf, zf, *, t0=0.0, threshold=0.1, n_taps=63, envelope=False,
                 f_demod=None, device=0):
    """Adaptive TFM: measure the surface from the FMC (measure_surface), build the travel times through it
    (travel_time_surface, couplant ``c1`` over the part ``c2``) and image the part at the focal points (xf, zf).  By default the
    image is the RF delay-and-sum tfm_image; with ``envelope=True`` it is the envelope ``np.abs(tfm_analytic(...))`` of the analytic
    FMC, which is formed once (``n_taps`` Hilbert taps) and serves the surface measurement too.  Focal points outside the trimmed
    profile's extent get NaN times and contribute nothing.  ``f_demod`` [Hz] (needs ``envelope=True``): the part image is
    ``np.abs(tfm_iq(...))``, carrier-aware interpolation; the surface measurement stays as it is.
    -> (image float32 [n_f], surface dict of measure_surface)."""
    if f_demod is not None:
        if not envelope:
            raise ValueError("f_demod (carrier-aware interpolation) needs envelope=True")
        f_demod = _f_demod(f_demod, fs)
    analytic = fmc_analytic(fmc, n_taps, device=device) if envelope else None
    surf = measure_surface(fmc, fs, xe, ze, c1, x0, dx, n_s, z_lo, z_hi, dz, t0=t0, threshold=threshold, n_taps=n_taps,
                           analytic=analytic, device=device)
    tt = travel_time_surface(surf["x0"], surf["dx"], surf["zs"], c1, c2, xe, ze, xf, zf, device=device)
    if f_demod is not None:
        return np.abs(tfm_iq(analytic, fs, f_demod, tt, t0=t0, device=device)), surf
    if envelope:
        return np.abs(tfm_analytic(analytic, fs, tt, t0=t0, device=device)), surf
    return tfm_image(fmc, fs, tt, t0=t0, device=device), surf


# ---------------------------------------------------------------------------------------------- plane-wave imaging
def _aperture(xe, ze):
    """(x_lo, x_hi, z_a) of a linear horizontal array: all elements at one depth"""
    xe, ze = _f64(xe, "xe"), _f64(ze, "ze")
    if xe.shape != ze.shape or xe.size == 0:
        raise ValueError("xe/ze must pair up and hold at least one element")
    if not (np.all(np.isfinite(xe)) and np.all(np.isfinite(ze))):
        raise ValueError("element positions must be finite")
    if np.any(ze != ze[0]):
        raise ValueError("plane waves need a horizontal array: all ze equal")
    return float(xe.min()), float(xe.max()), float(ze[0])


def pw_delays(xe, ze, angles, c1):
    """Firing delays of plane waves -> float64 [n_a, n_e]: element e fires at (xe[e] - x_ref) sin(angle) / c1 >= 0 with
    x_ref = min(xe) for sin(angle) >= 0, else max(xe) (time zero: the first firing).  Angles in radians, measured in medium 1
    (speed ``c1``) from +z towards +x.  The array must be horizontal (equal ``ze``).  Computed on the host; a non-finite angle or
    |angle| >= pi/2 gives a NaN row (the synthesis skips NaN delays).  Definition: include/rtus.h (plane-wave imaging)."""
    x_lo, x_hi, _ = _aperture(xe, ze)
    xe = _f64(xe, "xe")
    a = _f64(angles, "angles")
    if not (np.isfinite(c1) and c1 > 0):
        raise ValueError("c1 must be a positive finite speed")
    ok = np.abs(a) < np.pi / 2
    sn = np.sin(np.where(ok, a, 0.0))
    xref = np.where(sn >= 0.0, x_lo, x_hi)
    d = (xe[None, :] - xref[:, None]) * sn[:, None] / float(c1)
    d[~ok] = np.nan
    return d


def pw_travel_time_layers(z_if, c, angles, xe, ze, xf, zf, *, out=None, device=0):
    """Plane-wave transmit times through horizontal layers -> tt[n_a, n_f]: the time from the first firing until the plane wave of
    each angle reaches each focal point.  The aperture is taken from ``xe``/``ze`` (a horizontal array above z_if[0]).  NaN where
    the wave is evanescent in a crossed layer, the focal point is not below the array, the angle is not finite or |angle| >= pi/2,
    or the focal point is not insonified (its ray traced back misses the aperture).  The table is ``tt_tx`` of tfm_image /
    tfm_analytic / pwi_image with element tables as ``tt_rx``.  Definition: include/rtus.h (rtus_pw_layers).  Not in the reference."""
    z_if, c = _medium(z_if, c)
    x_lo, x_hi, z_a = _aperture(xe, ze)
    ang = _f64(angles, "angles")
    xf, zf = _f64(xf, "xf"), _f64(zf, "zf")
    if xf.shape != zf.shape:
        raise ValueError("xf/zf must pair up")
    tt = _out(out, (ang.size, xf.size), np.float64)
    st = _lib.lib().rtus_pw_layers(_ptr(z_if) if z_if.size else None, _ptr(c), z_if.size, _ptr(ang), ang.size, x_lo, x_hi, z_a,
                                   _ptr(xf), _ptr(zf), xf.size, _ptr(tt), int(device))
    _lib.check(st, "rtus_pw_layers")
    return tt


def pw_travel_time_surface(x0, dx, zs, c1, c2, angles, xe, ze, xf, zf, *, return_entry=False, out=None, device=0):
    """Plane-wave transmit times through ONE curved interface given as a sampled depth profile -> tt[n_a, n_f] (travel_time_surface's
    spline, extent and focal-point rules; ``c1`` above, ``c2`` below).  The aperture is taken from ``xe``/``ze`` (a horizontal
    array strictly above the whole profile, else the table is NaN).  An entry is the least time over the interior local minima of
    T(x) = ((x - x_ref) sin a + (s(x) - z_a) cos a)/c1 + |S(x) - F|/c2 at insonified entry points (x - (s(x) - z_a) tan a inside the
    aperture).  ``return_entry``: also the winning entry points, -> (tt, x_entry).  Definition and guarantee: include/rtus.h
    (rtus_pw_surface).  Not in the reference."""
    zs = _f64(zs, "zs")
    x_lo, x_hi, z_a = _aperture(xe, ze)
    ang = _f64(angles, "angles")
    xf, zf = _f64(xf, "xf"), _f64(zf, "zf")
    if xf.shape != zf.shape:
        raise ValueError("xf/zf must pair up")
    tt = _out(out, (ang.size, xf.size), np.float64)
    xn = np.empty((ang.size, xf.size), dtype=np.float64) if return_entry else None
    st = _lib.lib().rtus_pw_surface(float(x0), float(dx), _ptr(zs), zs.size, float(c1), float(c2), _ptr(ang), ang.size, x_lo, x_hi, z_a,
                                    _ptr(xf), _ptr(zf), xf.size, _ptr(tt), _ptr(xn), int(device))
    _lib.check(st, "rtus_pw_surface")
    return (tt, xn) if return_entry else tt


def fmc_synth_tx(fmc, fs, delays, *, out=None, device=0):
    """Data of any transmit delay law from an FMC -> float32 [n_v, n_rx, n_t]:
    out[v, rx, n] = sum over tx of fmc[tx, rx](n - delays[v, tx] fs), linearly interpolated, samples outside the record zero.
    ``delays`` [n_v, n_tx] in seconds: plane waves (pw_delays), diverging waves, sub-apertures; a NaN (or absurd) delay does not
    fire that tx.  The output has the FMC's layout: tfm_image / fmc_analytic / tfm_analytic take it as it is.  Definition:
    include/rtus.h (rtus_fmc_synth_tx).  Not in the reference."""
    fmc = np.ascontiguousarray(fmc, dtype=np.float32)
    if fmc.ndim != 3:
        raise ValueError("fmc must be [n_tx, n_rx, n_t]")
    d = _f64(delays, "delays", ndim=2)
    if d.shape[1] != fmc.shape[0]:
        raise ValueError("delays must be [n_v, n_tx] with n_tx = fmc.shape[0]")
    o = _out(out, (d.shape[0], fmc.shape[1], fmc.shape[2]), np.float32)
    st = _lib.lib().rtus_fmc_synth_tx(_ptr(fmc), fmc.shape[0], fmc.shape[1], fmc.shape[2], float(fs), _ptr(d), d.shape[0], _ptr(o),
                                      int(device))
    _lib.check(st, "rtus_fmc_synth_tx")
    return o


def pwi_image(pw, fs, tt_pw, tt_rx, *, t0=0.0, envelope=False, coherence=False, n_taps=63, f_demod=None, device=0):
    """Plane-wave image: the delay-and-sum of plane-wave data ``pw`` [n_a, n_rx, n_t] (float32, e.g. fmc_synth_tx(fmc, fs,
    pw_delays(...)) or recorded by an instrument with those delays) through the plane-wave table ``tt_pw`` [n_a, n_f]
    (pw_travel_time_*) and an element table ``tt_rx`` [n_rx, n_f].  RF: tfm_image(pw, fs, tt_pw, tt_rx) -> float32 [n_f].  With
    ``envelope=True``: |tfm_analytic(fmc_analytic(pw, n_taps), ...)| -> float32 [n_f], and with ``coherence=True`` also the coherence
    factor, -> (envelope, cf); ``coherence="cf"`` / ``"vcf"`` / ``"scf"`` name the factor as in tfm_analytic.  ``f_demod`` [Hz]
    (needs ``envelope=True``; "vcf" / "scf" raise ValueError): tfm_iq instead of tfm_analytic, carrier-aware interpolation."""
    coherence = _coherence(coherence)
    if coherence and not envelope:
        raise ValueError("the coherence factor needs envelope=True")
    if f_demod is not None:
        if not envelope:
            raise ValueError("f_demod (carrier-aware interpolation) needs envelope=True")
        coherence, f_demod = _iq_coherence(coherence), _f_demod(f_demod, fs)
    tt_pw = np.ascontiguousarray(tt_pw, dtype=np.float64)
    tt_rx = np.ascontiguousarray(tt_rx, dtype=np.float64)
    if not envelope:
        return tfm_image(pw, fs, tt_pw, tt_rx, t0=t0, device=device)
    analytic = fmc_analytic(pw, n_taps, device=device)
    if f_demod is not None:
        r = tfm_iq(analytic, fs, f_demod, tt_pw, tt_rx, t0=t0, coherence=coherence, device=device)
    else:
        r = tfm_analytic(analytic, fs, tt_pw, tt_rx, t0=t0, coherence=coherence, device=device)
    return (np.abs(r[0]), r[1]) if coherence else np.abs(r)


# ---------------------------------------------------------------------------------------------- multi-view TFM
MAX_LAYERS = 8              # RTUS_MAX_LAYERS (include/rtus.h)
LEGS = ("L", "T", "LL", "LT", "TL", "TT")
VIEWS = ("L-L", "L-T", "T-T",
         "LL-L", "LL-T", "LT-L", "LT-T", "TL-L", "TL-T", "TT-L", "TT-T",
         "LL-LL", "LL-LT", "LL-TL", "LL-TT", "LT-LT", "LT-TL", "LT-TT", "TL-LT", "TL-TT", "TT-TT")


def reverse_leg(leg):
    """the leg read the other way: the time of path ``leg`` from the point to an element is the element-to-point leg
    ``reverse_leg(leg)`` ("LT" -> "TL"; direct legs are their own reverse)"""
    if leg not in LEGS:
        raise ValueError(f"unknown leg {leg!r}: legs are {LEGS}")
    return leg[::-1]


def view_tables(view):
    """(transmit leg, receive leg) of a view "A-B" as tfm_image takes them: (A, reverse_leg(B))"""
    parts = view.split("-") if isinstance(view, str) else ()
    if len(parts) != 2 or parts[0] not in LEGS or parts[1] not in LEGS:
        raise ValueError(f"unknown view {view!r}: a view is 'A-B' with A, B in {LEGS}")
    return parts[0], reverse_leg(parts[1])


def skip_travel_time_layers(z_if, c, z_back, xe, ze, xf, zf, *, c_up=None, taup=False, out=None, device=0, devices=None):
    """Element x focal-point times of a SKIP leg through horizontal layers -> tt[n_e, n_f]: the ray goes down through the layers
    ``z_if`` / ``c`` (``c[-1]``: the down-going speed in the part), reflects off the planar backwall at ``z_back`` and comes up to
    the point at speed ``c_up`` (default ``c[-1]``; another speed is a mode conversion at the backwall).  The time is
    travel_time_layers(z_if + [z_back], c + [c_up], ..., 2 z_back - zf) — the direct time to the mirrored point — and NaN outside
    z_if[-1] < zf < z_back.  ``taup``, ``out``, ``device``, ``devices``: travel_time_layers's.  Conventions: include/rtus.h
    (multi-view TFM)."""
    z_if, c = _medium(z_if, c)
    z_back = float(z_back)
    c_up = float(c[-1]) if c_up is None else float(c_up)
    front = float(z_if[-1]) if z_if.size else -np.inf
    if not (z_back > front):
        raise ValueError("the backwall must lie below the last interface (z_back > z_if[-1])")
    if z_if.size + 1 > MAX_LAYERS:
        raise ValueError(f"a skip leg adds an interface: at most {MAX_LAYERS - 1} interfaces above the backwall")
    xf, zf = _f64(xf, "xf"), _f64(zf, "zf")
    if xf.shape != zf.shape:
        raise ValueError("xe/ze and xf/zf must pair up")
    tt = travel_time_layers(np.r_[z_if, z_back], np.r_[c, c_up], xe, ze, xf, 2.0 * z_back - zf, out=out, device=device,
                            devices=devices, taup=taup)
    tt[:, ~((zf > front) & (zf < z_back))] = np.nan
    return tt


def skip_travel_time_surface(x0, dx, zs, c1, c2, z_back, xe, ze, xf, zf, *, c_up=None, return_entry=False, out=None, device=0):
    """Element x focal-point times of a SKIP leg through ONE curved front surface -> tt[n_e, n_f]: element -> couplant (``c1``) ->
    the surface (travel_time_surface's spline, extent and element rules) -> down at ``c2`` to the planar backwall at ``z_back`` ->
    up at ``c_up`` (default ``c2``; another speed is a mode conversion) to the point.  An entry is the least time over the
    interior local minima of T(x) = |E - S(x)|/c1 + T_in(S(x)), T_in the Fermat time below the surface via the backwall; NaN
    without one, for a point outside the extent or not strictly between the surface and the backwall, and everywhere when the
    backwall is not strictly below the whole profile.  ``return_entry``: -> (tt, x_entry, x_back), the winning entry point and
    backwall reflection point.  Definition and guarantee: include/rtus.h (rtus_tt_surface_skip).  Not in the reference."""
    zs = _f64(zs, "zs")
    xe, ze, xf, zf = _points(xe, ze, xf, zf)
    c_up = float(c2) if c_up is None else float(c_up)
    tt = _out(out, (xe.size, xf.size), np.float64)
    xn = np.empty((xe.size, xf.size), dtype=np.float64) if return_entry else None
    xb = np.empty((xe.size, xf.size), dtype=np.float64) if return_entry else None
    st = _lib.lib().rtus_tt_surface_skip(float(x0), float(dx), _ptr(zs), zs.size, float(c1), float(c2), c_up, float(z_back), _ptr(xe),
                                         _ptr(ze), xe.size, _ptr(xf), _ptr(zf), xf.size, _ptr(tt), _ptr(xn), _ptr(xb), int(device))
    _lib.check(st, "rtus_tt_surface_skip")
    return (tt, xn, xb) if return_entry else tt


def _legs_wanted(legs):
    legs = tuple(legs)
    bad = [g for g in legs if g not in LEGS]
    if bad:
        raise ValueError(f"unknown legs {bad}: legs are {LEGS}")
    return legs


def view_legs_layers(z_if, c_above, c_l, c_t, z_back, xe, ze, xf, zf, *, legs=LEGS, device=0):
    """The leg tables of multi-view TFM through horizontal layers -> {leg: tt [n_e, n_f]} for ``legs`` (default all six:
    L, T, LL, LT, TL, TT).  ``z_if`` / ``c_above``: the interfaces and the speeds above the part (len(c_above) == len(z_if)); the
    part below z_if[-1] has speeds ``c_l`` / ``c_t`` and a planar backwall at ``z_back``.  Direct legs: travel_time_layers; skip
    legs: skip_travel_time_layers.  Conventions: include/rtus.h (multi-view TFM)."""
    legs = _legs_wanted(legs)
    z_if = list(np.atleast_1d(np.asarray(z_if, dtype=np.float64)))
    c_above = list(np.atleast_1d(np.asarray(c_above, dtype=np.float64)))
    if len(c_above) != len(z_if):
        raise ValueError("need len(c_above) == len(z_if)")
    sp = {"L": float(c_l), "T": float(c_t)}
    out = {}
    for g in legs:
        if len(g) == 1:
            out[g] = travel_time_layers(z_if, c_above + [sp[g]], xe, ze, xf, zf, device=device)
        else:
            out[g] = skip_travel_time_layers(z_if, c_above + [sp[g[0]]], z_back, xe, ze, xf, zf, c_up=sp[g[1]], device=device)
    return out


# ---------------------------------------------------------------------------------------------- matrix arrays: three dimensions
LAYERS3_POINTS = 256        # RTUS_TT_LAYERS3_POINTS: focal points per workgroup of the kernel (tests of its tile seams)
LAYERS3_ROWS = 16           # RTUS_TT_LAYERS3_ROWS:   elements per workgroup


def matrix_array(n_x, n_y, pitch_x, pitch_y=None, z=0.0):
    """The elements of an ``n_x`` x ``n_y`` matrix array -> (xe, ye, ze), each [n_x * n_y]: centred on x = y = 0, x fastest
    (element ``j * n_x + i`` is column i of row j), all at depth ``z``.  ``pitch_y`` defaults to ``pitch_x``."""
    n_x, n_y = int(n_x), int(n_y)
    if n_x < 1 or n_y < 1:
        raise ValueError("need n_x >= 1 and n_y >= 1")
    pitch_y = pitch_x if pitch_y is None else pitch_y
    x = (np.arange(n_x, dtype=np.float64) - 0.5 * (n_x - 1)) * np.float64(pitch_x)
    y = (np.arange(n_y, dtype=np.float64) - 0.5 * (n_y - 1)) * np.float64(pitch_y)
    return np.tile(x, n_y), np.repeat(y, n_x), np.full(n_x * n_y, float(z))


def volume_grid(xs, ys, zs):
    """The focal points of a volume -> (xf, yf, zf, shape): every (x, y, z) of the three axes as flat vectors, x fastest, then y,
    then z; ``shape`` = (n_z, n_y, n_x), so an image over the points reads ``image.reshape(shape)[iz, iy, ix]``."""
    xs, ys, zs = _f64(xs, "xs"), _f64(ys, "ys"), _f64(zs, "zs")
    shape = (zs.size, ys.size, xs.size)
    zf, yf, xf = (np.ascontiguousarray(np.broadcast_to(v, shape).reshape(-1))
                  for v in (zs[:, None, None], ys[None, :, None], xs[None, None, :]))
    return xf, yf, zf, shape


def _points_3d(xe, ye, ze, xf, yf, zf):
    """Elements and focal points in three dimensions as float64 vectors, xe/ye/ze and xf/yf/zf of one length each."""
    xe, ye, ze = _f64(xe, "xe"), _f64(ye, "ye"), _f64(ze, "ze")
    xf, yf, zf = _f64(xf, "xf"), _f64(yf, "yf"), _f64(zf, "zf")
    if not (xe.shape == ye.shape == ze.shape and xf.shape == yf.shape == zf.shape):
        raise ValueError("xe/ye/ze and xf/yf/zf must pair up")
    return xe, ye, ze, xf, yf, zf


def travel_time_layers_3d(z_if, c, xe, ye, ze, xf, yf, zf, *, out=None, device=0):
    """Element x focal-point Fermat travel times in three dimensions through horizontal layers -> tt[n_e, n_f]: the table of a
    matrix (2-D) array over the points of a volume, which every consumer of a table (tfm_image, tfm_analytic, tfm_views,
    simulate_fmc, focal_delays ...) takes as it is.

    The stack is travel_time_layers's; elements and points may lie at any depth.  An entry is the planar time at the lateral reach
    r = sqrt((xf - xe)^2 + (yf - ye)^2) (<= 1e-13 relative), NaN where zf <= ze or a coordinate of the pair is not finite.  Each
    entry depends on its own pair only: a slice of the elements or of the points gives that slice of the table bit for bit, so
    row shards and several GPUs are slices of the inputs (include/rtus.h, rtus_tt_layers3).  ``out``: optional float64
    [n_e, n_f] result buffer.  Not in the reference."""
    z_if, c = _medium(z_if, c)
    xe, ye, ze, xf, yf, zf = _points_3d(xe, ye, ze, xf, yf, zf)
    tt = _out(out, (xe.size, xf.size), np.float64)
    st = _lib.lib().rtus_tt_layers3(_ptr(z_if) if z_if.size else None, _ptr(c), z_if.size, _ptr(xe), _ptr(ye), _ptr(ze), xe.size,
                                    _ptr(xf), _ptr(yf), _ptr(zf), xf.size, _ptr(tt), 0, int(device))
    _lib.check(st, "rtus_tt_layers3")
    return tt


def skip_travel_time_layers_3d(z_if, c, z_back, xe, ye, ze, xf, yf, zf, *, c_up=None, out=None, device=0):
    """skip_travel_time_layers for a matrix array: the SKIP leg down through ``z_if`` / ``c``, off the planar backwall at ``z_back``
    and up at ``c_up`` (default ``c[-1]``) to the point — a planar backwall keeps the symmetry about the vertical axis, so the time
    is travel_time_layers_3d(z_if + [z_back], c + [c_up], ..., 2 z_back - zf), and NaN outside z_if[-1] < zf < z_back."""
    z_if, c = _medium(z_if, c)
    z_back = float(z_back)
    c_up = float(c[-1]) if c_up is None else float(c_up)
    front = float(z_if[-1]) if z_if.size else -np.inf
    if not (z_back > front):
        raise ValueError("the backwall must lie below the last interface (z_back > z_if[-1])")
    if z_if.size + 1 > MAX_LAYERS:
        raise ValueError(f"a skip leg adds an interface: at most {MAX_LAYERS - 1} interfaces above the backwall")
    zf = _f64(zf, "zf")
    tt = travel_time_layers_3d(np.r_[z_if, z_back], np.r_[c, c_up], xe, ye, ze, xf, yf, 2.0 * z_back - zf, out=out, device=device)
    tt[:, ~((zf > front) & (zf < z_back))] = np.nan
    return tt


def view_legs_layers_3d(z_if, c_above, c_l, c_t, z_back, xe, ye, ze, xf, yf, zf, *, legs=LEGS, device=0):
    """view_legs_layers for a matrix array -> {leg: tt [n_e, n_f]} for ``legs`` (default all six), in the shape tfm_views takes:
    multi-view TFM of a volume.  Direct legs: travel_time_layers_3d; skip legs: skip_travel_time_layers_3d."""
    legs = _legs_wanted(legs)
    z_if = list(np.atleast_1d(np.asarray(z_if, dtype=np.float64)))
    c_above = list(np.atleast_1d(np.asarray(c_above, dtype=np.float64)))
    if len(c_above) != len(z_if):
        raise ValueError("need len(c_above) == len(z_if)")
    sp = {"L": float(c_l), "T": float(c_t)}
    out = {}
    for g in legs:
        if len(g) == 1:
            out[g] = travel_time_layers_3d(z_if, c_above + [sp[g]], xe, ye, ze, xf, yf, zf, device=device)
        else:
            out[g] = skip_travel_time_layers_3d(z_if, c_above + [sp[g[0]]], z_back, xe, ye, ze, xf, yf, zf, c_up=sp[g[1]],
                                                device=device)
    return out


def view_legs_surface(x0, dx, zs, c1, c_l, c_t, z_back, xe, ze, xf, zf, *, legs=LEGS, device=0):
    """The leg tables of multi-view TFM through ONE measured front surface (travel_time_surface's profile; couplant ``c1``) ->
    {leg: tt [n_e, n_f]} for ``legs`` (default all six).  The part has speeds ``c_l`` / ``c_t`` and a planar backwall at
    ``z_back``.  Direct legs: travel_time_surface; skip legs: skip_travel_time_surface.  Conventions: include/rtus.h."""
    legs = _legs_wanted(legs)
    sp = {"L": float(c_l), "T": float(c_t)}
    out = {}
    for g in legs:
        if len(g) == 1:
            out[g] = travel_time_surface(x0, dx, zs, c1, sp[g], xe, ze, xf, zf, device=device)
        else:
            out[g] = skip_travel_time_surface(x0, dx, zs, c1, sp[g[0]], z_back, xe, ze, xf, zf, c_up=sp[g[1]], device=device)
    return out


def tfm_views(fmc, fs, legs, views=VIEWS, *, t0=0.0, envelope=False, coherence=False, n_taps=63, amplitudes=None, hmc=False,
              f_demod=None, device=0):
    """Multi-view TFM: one image per view -> {view: image float32 [n_f]}.  ``legs``: {leg: tt [n_e, n_f]} (view_legs_layers /
    view_legs_surface); a view "A-B" (transmit leg A, then receive leg B from the point to the receiver) is imaged with
    tt_tx = legs[A] and tt_rx = legs[reverse_leg(B)].  RF: tfm_image.  With ``envelope=True``: |tfm_analytic| over the analytic FMC,
    formed once for all views (``n_taps`` Hilbert taps); with ``coherence=True`` too, each value is (envelope, cf), and with
    ``coherence="cf"`` / ``"vcf"`` / ``"scf"`` (envelope, that factor of tfm_analytic / tfm_phase).
    ``amplitudes``: {leg: (down, up)} complex64 [n_e, n_f] (view_amplitudes_surface; needs ``envelope=True``, excludes ``coherence``):
    each view is beamformed by tfm_weighted with w_tx = conj(down[A]) and w_rx = conj(up[reverse_leg(B)]) and the value is |S| / P,
    P the view's sensitivity (NaN where P = 0): a unit point scatterer reads 1 in every view that sees it, so views share one scale.
    ``hmc=True``: ``fmc`` is a half-matrix capture [n_pairs, n_t] (hmc_pack) and every view goes through tfm_hmc / tfm_analytic_hmc;
    ``amplitudes`` and ``coherence="vcf"`` / ``"scf"`` raise ValueError with it: loop over the views with tfm_weighted_hmc (its
    docstring shows the loop) or tfm_phase_hmc on hmc_analytic(fmc) instead.
    ``f_demod`` [Hz]: every view goes through tfm_iq / tfm_iq_hmc (carrier-aware interpolation) instead; it needs ``envelope=True``
    and raises ValueError together with ``amplitudes`` or ``coherence="vcf"`` / ``"scf"``.  None: exactly the paths above.
    An unknown view or a leg missing from ``legs`` (or ``amplitudes``) raises ValueError before any GPU call."""
    coherence = _coherence(coherence)
    if hmc and amplitudes is not None:
        raise ValueError("tfm_views does not weight a half-matrix capture: loop over the views with tfm_weighted_hmc")
    if hmc and coherence in ("vcf", "scf"):
        raise ValueError(f"tfm_views has no coherence={coherence!r} on a half-matrix capture: loop over the views with tfm_phase_hmc")
    if coherence and not envelope:
        raise ValueError("the coherence factor needs envelope=True")
    if amplitudes is not None and not envelope:
        raise ValueError("amplitude weighting needs envelope=True")
    if amplitudes is not None and coherence:
        raise ValueError("amplitude weighting and the coherence factor are exclusive")
    if f_demod is not None:
        if not envelope:
            raise ValueError("f_demod (carrier-aware interpolation) needs envelope=True")
        if amplitudes is not None:
            raise ValueError("f_demod is not available with amplitude weighting (tfm_weighted has no carrier-aware form)")
        coherence, f_demod = _iq_coherence(coherence), _f_demod(f_demod, fs)
    views = (views,) if isinstance(views, str) else tuple(views)
    pairs = {v: view_tables(v) for v in views}
    missing = sorted({g for p in pairs.values() for g in p if g not in legs})
    if missing:
        raise ValueError(f"legs {missing} are needed by the views and missing from ``legs``")
    if amplitudes is not None:
        missing = sorted({g for p in pairs.values() for g in p if g not in amplitudes})
        if missing:
            raise ValueError(f"legs {missing} are needed by the views and missing from ``amplitudes``")
    if hmc:
        if not envelope:
            return {v: tfm_hmc(fmc, fs, legs[a], legs[b], t0=t0, device=device) for v, (a, b) in pairs.items()}
        analytic = hmc_analytic(fmc, n_taps, device=device)
        out = {}
        for v, (a, b) in pairs.items():
            if f_demod is not None:
                r = tfm_iq_hmc(analytic, fs, f_demod, legs[a], legs[b], t0=t0, coherence=coherence, device=device)
            else:
                r = tfm_analytic_hmc(analytic, fs, legs[a], legs[b], t0=t0, coherence=coherence, device=device)
            out[v] = (np.abs(r[0]), r[1]) if coherence else np.abs(r)
        return out
    if not envelope:
        return {v: tfm_image(fmc, fs, legs[a], legs[b], t0=t0, device=device) for v, (a, b) in pairs.items()}
    analytic = fmc_analytic(fmc, n_taps, device=device)
    out = {}
    for v, (a, b) in pairs.items():
        if amplitudes is not None:
            w_tx = np.conj(np.asarray(amplitudes[a][0], dtype=np.complex64))
            w_rx = np.conj(np.asarray(amplitudes[b][1], dtype=np.complex64))
            img, sens = tfm_weighted(analytic, fs, legs[a], w_tx, legs[b], w_rx, t0=t0, sensitivity=True, device=device)
            with np.errstate(divide="ignore", invalid="ignore"):
                out[v] = np.where(sens > 0, np.abs(img) / sens, np.float32(np.nan)).astype(np.float32)
            continue
        if f_demod is not None:
            r = tfm_iq(analytic, fs, f_demod, legs[a], legs[b], t0=t0, coherence=coherence, device=device)
        else:
            r = tfm_analytic(analytic, fs, legs[a], legs[b], t0=t0, coherence=coherence, device=device)
        out[v] = (np.abs(r[0]), r[1]) if coherence else np.abs(r)
    return out


# ---------------------------------------------------------------------------------------------- ray amplitudes, weighted TFM
LEG_CODES = {"L": 0, "T": 1, "LL": 2, "LT": 3, "TL": 4, "TT": 5}      # RTUS_LEG_* (include/rtus.h)


def leg_amplitudes_surface(x0, dx, zs, c1, rho1, c_l, c_t, rho2, z_back, leg, xe, ze, xf, zf, x_entry, x_back=None, *, up=False,
                           element_width=0.0, f_c=None, out=None, device=0):
    """Ray amplitudes of one multi-view leg through a measured surface -> complex64 [n_e, n_f]: A = D C_S [C_B] G (element
    directivity, surface and backwall displacement coefficients, 2-D ray-tube spreading), in the analytic signal's phase convention.
    ``x_entry`` (and ``x_back`` for skip legs) are the leg's points as travel_time_surface(return_entry=True) /
    skip_travel_time_surface(return_entry=True) return them.  ``up``: the wave travels point -> element along the leg's path (the
    receive direction) instead of element -> point.  ``element_width`` [m] > 0 needs ``f_c`` [Hz], the centre frequency of the
    directivity.  The couplant has speed ``c1`` and density ``rho1``, the part ``c_l`` > ``c_t`` and ``rho2`` with a traction-free
    backwall at ``z_back``.  NaN where x_entry (or x_back) is NaN; 0 where either is infinite, as for any path that does not cross
    the surface into the part.  The path is not put to Snell's law.  Definition: include/rtus.h (rtus_leg_amp_surface).  Not in the
    reference."""
    if leg not in LEGS:
        raise ValueError(f"unknown leg {leg!r}: legs are {LEGS}")
    skip = len(leg) == 2
    zs = _f64(zs, "zs")
    xe, ze, xf, zf = _points(xe, ze, xf, zf)
    shape = (xe.size, xf.size)
    xn = _f64(x_entry, "x_entry", 2)
    if xn.shape != shape:
        raise ValueError(f"x_entry must be [n_e, n_f] = {shape}")
    xb = None
    if skip:
        if x_back is None:
            raise ValueError(f"the skip leg {leg!r} needs x_back")
        xb = _f64(x_back, "x_back", 2)
        if xb.shape != shape:
            raise ValueError(f"x_back must be [n_e, n_f] = {shape}")
    if element_width > 0 and f_c is None:
        raise ValueError("an element width needs the centre frequency f_c")
    amp = _out(out, shape, np.complex64)
    st = _lib.lib().rtus_leg_amp_surface(float(x0), float(dx), _ptr(zs), zs.size, float(c1), float(rho1), float(c_l), float(c_t),
                                         float(rho2), float(z_back), LEG_CODES[leg], 1 if up else 0, float(element_width),
                                         float(f_c or 0.0), _ptr(xe), _ptr(ze), xe.size, _ptr(xf), _ptr(zf), xf.size, _ptr(xn), _ptr(xb),
                                         _ptr(amp), int(device))
    _lib.check(st, "rtus_leg_amp_surface")
    return amp


def view_amplitudes_surface(x0, dx, zs, c1, rho1, c_l, c_t, rho2, z_back, xe, ze, xf, zf, *, legs=LEGS, element_width=0.0, f_c=None,
                            device=0):
    """The leg tables of multi-view TFM through ONE measured front surface with their ray amplitudes -> (legs_tt, amps):
    legs_tt = {leg: tt [n_e, n_f]} as view_legs_surface makes them, amps = {leg: (down, up)} complex64 [n_e, n_f]
    (leg_amplitudes_surface in both directions on the tables' own entry and backwall points).  Feed both to
    ``tfm_views(..., envelope=True, amplitudes=amps)``."""
    legs = _legs_wanted(legs)
    sp = {"L": float(c_l), "T": float(c_t)}
    tts, amps = {}, {}
    for g in legs:
        if len(g) == 1:
            tt, xn = travel_time_surface(x0, dx, zs, c1, sp[g], xe, ze, xf, zf, return_entry=True, device=device)
            xb = None
        else:
            tt, xn, xb = skip_travel_time_surface(x0, dx, zs, c1, sp[g[0]], z_back, xe, ze, xf, zf, c_up=sp[g[1]], return_entry=True,
                                                  device=device)
        tts[g] = tt
        amps[g] = tuple(leg_amplitudes_surface(x0, dx, zs, c1, rho1, c_l, c_t, rho2, z_back, g, xe, ze, xf, zf, xn, xb, up=u,
                                               element_width=element_width, f_c=f_c, device=device) for u in (False, True))
    return tts, amps


def _weights(w, n, n_f, name):
    w = np.ascontiguousarray(w, dtype=np.complex64)
    if w.shape != (n, n_f):
        raise ValueError(f"{name} must be complex64 [{n}, {n_f}]")
    return w


def tfm_weighted(analytic, fs, tt_tx, w_tx, tt_rx=None, w_rx=None, *, t0=0.0, sensitivity=False, out=None, device=0):
    """Weighted envelope TFM: S[f] = sum over (tx, rx) of w_tx[tx, f] w_rx[rx, f] a[tx, rx](tau_tx + tau_rx), with tfm_analytic's
    sample positions, interpolation, edge rules and no-path rule; a leg with a non-finite weight contributes nothing.  ``w_tx`` /
    ``w_rx``: complex64 [n_tx, n_f] / [n_rx, n_f]; tt_rx and w_rx default to tt_tx and w_tx.  -> complex64 image [n_f]; with
    ``sensitivity=True`` -> (image, P float32 [n_f]), P = (sum over tx with a path of |w_tx|^2) (sum over rx with a path of |w_rx|^2).
    With the weights conj(amplitude) P is the image of a unit point scatterer and |S| / P is sensitivity-normalised.  Definition:
    include/rtus.h (rtus_tfm_weighted).  Not in the reference."""
    a = _complex_fmc(analytic)
    tt_tx = np.ascontiguousarray(tt_tx, dtype=np.float64)
    if tt_rx is None:
        tt_rx = tt_tx
        w_rx = w_tx if w_rx is None else w_rx
    tt_rx = np.ascontiguousarray(tt_rx, dtype=np.float64)
    if w_rx is None:
        raise ValueError("w_rx is needed with tt_rx")
    if tt_tx.ndim != 2 or tt_rx.ndim != 2 or tt_tx.shape[1] != tt_rx.shape[1]:
        raise ValueError("tt_tx / tt_rx must be [n_tx, n_focal] / [n_rx, n_focal]")
    if tt_tx.shape[0] != a.shape[0] or tt_rx.shape[0] != a.shape[1]:
        raise ValueError("the analytic FMC's first two dimensions must match the rows of tt_tx and tt_rx")
    n_f = tt_tx.shape[1]
    w_tx, w_rx = _weights(w_tx, a.shape[0], n_f, "w_tx"), _weights(w_rx, a.shape[1], n_f, "w_rx")
    img = _out(out, (n_f,), np.complex64)
    sens = np.empty(n_f, dtype=np.float32) if sensitivity else None
    st = _lib.lib().rtus_tfm_weighted(_ptr(a), a.shape[0], a.shape[1], a.shape[2], float(fs), float(t0), _ptr(tt_tx), _ptr(tt_rx),
                                      _ptr(w_tx), _ptr(w_rx), n_f, _ptr(img), _ptr(sens), int(device))
    _lib.check(st, "rtus_tfm_weighted")
    return (img, sens) if sensitivity else img


def _hmc_weights(w, n_e, n_f, name):
    """a weight table of tfm_weighted_hmc -> complex64 [n_e, n_f]; a real array is refused (it is not a view's amplitude)"""
    w = np.asarray(w)
    if not np.iscomplexobj(w):
        raise ValueError(f"{name} must be complex64 [{n_e}, {n_f}] (got dtype {w.dtype})")
    return _weights(w, n_e, n_f, name)


def tfm_weighted_hmc(analytic_hmc, fs, tt_tx, w_tx, tt_rx=None, w_rx=None, *, t0=0.0, sensitivity=False, out=None, device=0):
    """tfm_weighted over a half-matrix capture: ``analytic_hmc`` complex64 [n_pairs, n_t] (hmc_analytic's, or float32
    [n_pairs, n_t, 2]); tt_tx / tt_rx float64 [n_e, n_f]; w_tx / w_rx complex64 [n_e, n_f]; tt_rx and w_rx default to tt_tx and w_tx.
    S[f] = sum over the records of W_ii a_ii(s_ii) and, for i < j, W_ij a_ij(s_ij) + W_ji a_ij(s_ji) with W_ij = w_tx[i] w_rx[j] —
    tfm_weighted of hmc_unpack(analytic_hmc) up to the order of the fp32 sum; a leg with a non-finite weight contributes nothing.
    With ONE delay table (tt_rx None or tt_tx itself; the weight tables may differ: every view "A-A") each record is gathered once
    and weighted by W_ij + W_ji.  -> complex64 image [n_f]; with ``sensitivity=True`` -> (image, P float32 [n_f]), tfm_weighted's P
    bit for bit.  Multi-view imaging of a packed capture, on one scale (tfm_views' ``amplitudes=`` for the full matrix)::

        legs, amps = view_amplitudes_surface(...)            # {leg: tt}, {leg: (down, up)}
        analytic = hmc_analytic(hmc)
        for view in views:
            a, b = view_tables(view)                         # the transmit leg A, reverse_leg(B)
            w_tx, w_rx = np.conj(amps[a][0]), np.conj(amps[b][1])
            # (a view "A-A": legs[b] is legs[a] — one delay table, two weight tables, every record gathered once)
            S, P = tfm_weighted_hmc(analytic, fs, legs[a], w_tx, legs[b], w_rx, sensitivity=True)
            with np.errstate(divide="ignore", invalid="ignore"):
                image[view] = np.where(P > 0, np.abs(S) / P, np.nan)

    Definition: include/rtus.h (rtus_tfm_weighted_hmc).  Not in the reference."""
    a = _complex_hmc(analytic_hmc)
    n_e, tt_tx, tt_rx, n_f = _hmc_tables(a.shape[0], tt_tx, tt_rx)
    w_tx = _hmc_weights(w_tx, n_e, n_f, "w_tx")
    w_rx = w_tx if w_rx is None else _hmc_weights(w_rx, n_e, n_f, "w_rx")
    img = _out(out, (n_f,), np.complex64)
    sens = np.empty(n_f, dtype=np.float32) if sensitivity else None
    st = _lib.lib().rtus_tfm_weighted_hmc(_ptr(a), n_e, a.shape[1], float(fs), float(t0), _ptr(tt_tx), _ptr(tt_rx), _ptr(w_tx),
                                          _ptr(w_rx), n_f, _ptr(img), _ptr(sens), int(device))
    _lib.check(st, "rtus_tfm_weighted_hmc")
    return (img, sens) if sensitivity else img


PIPE_SCAN_ARC = 0.25e-3     # default spacing of travel_time_pipe's scan points along the pipe's outer surface [m]


def _pipe_args(params, c3, r_inner, alpha_lo, alpha_hi, beta_lo, beta_hi, n_scan):
    p = _resolve(params)
    a_lo = -ALPHA_MAX if alpha_lo is None else float(alpha_lo)
    a_hi = ALPHA_MAX if alpha_hi is None else float(alpha_hi)
    b_lo, b_hi = float(beta_lo), float(beta_hi)
    if n_scan is None:
        n_scan = int(np.ceil(float(p.r_outer) * (b_hi - b_lo) / PIPE_SCAN_ARC)) + 1 if b_hi > b_lo else 4
        n_scan = max(n_scan, 4)
    pipe = Pipe(float(p.r_outer), float(r_inner), float(p.pipe_offset), float(c3))
    return p.lens(), a_lo, a_hi, pipe, b_lo, b_hi, int(n_scan)


def travel_time_pipe(xe, ze, xf, zf, *, c3=5600.0, r_inner=0.0, params: Params = None, alpha_lo=None, alpha_hi=None,
                     beta_lo=-np.pi / 2, beta_hi=np.pi / 2, n_scan=None, return_path=False, out=None, device=0):
    """Element x focal-point Fermat travel times from elements behind the curved lens (c1), through the water (c2), into the
    WALL of the pipe (c3) -> tt[n_e, n_f]: two curved refractions, the lens surface and the pipe's outer circle.  The pipe is the
    reference's: radius ``params.r_outer``, centre (``params.pipe_offset``, 0) (main_rt.py:466-467); ``r_inner`` is the bore (0: a
    solid bar).  An entry is the least time over the interior local minima of T(beta), beta the angle of the pipe entry point on
    [``beta_lo``, ``beta_hi``], scanned at ``n_scan`` points (default: at most 0.25 mm of arc apart); NaN for a point outside the
    wall or without a qualifying path.  ``return_path``: -> (tt, alpha, beta), the lens refraction point's and the pipe entry
    point's angles.  Definition, rules and guarantee: include/rtus.h (rtus_tt_pipe).  Not in the reference."""
    lens, a_lo, a_hi, pipe, b_lo, b_hi, n_scan = _pipe_args(params, c3, r_inner, alpha_lo, alpha_hi, beta_lo, beta_hi, n_scan)
    xe, ze, xf, zf = _points(xe, ze, xf, zf)
    tt = _out(out, (xe.size, xf.size), np.float64)
    al = np.empty((xe.size, xf.size), dtype=np.float64) if return_path else None
    be = np.empty((xe.size, xf.size), dtype=np.float64) if return_path else None
    st = _lib.lib().rtus_tt_pipe(C.byref(lens), a_lo, a_hi, C.byref(pipe), b_lo, b_hi, n_scan, _ptr(xe), _ptr(ze), xe.size, _ptr(xf),
                                 _ptr(zf), xf.size, _ptr(tt), _ptr(al), _ptr(be), int(device))
    _lib.check(st, "rtus_tt_pipe")
    return (tt, al, be) if return_path else tt


def pipe_wall_grid(r_inner, r_outer, n_r, n_theta, theta_lo, theta_hi, *, params: Params = None):
    """Focal points over the pipe wall in polar coordinates about the pipe's centre (``params.pipe_offset``, 0): ``n_r`` radii
    evenly over [r_inner, r_outer] and ``n_theta`` angles over [theta_lo, theta_hi] (radians from +z, travel_time_pipe's beta
    convention) -> (xf, zf), radius-major, so that ``tfm_image(...).reshape(n_r, n_theta)`` is the unrolled wall image (row 0 at
    r_inner).  Pass radii strictly inside the wall to keep the edge rows out of NaN: the wall is open, r_inner < r < r_outer."""
    p = _resolve(params)
    if int(n_r) < 1 or int(n_theta) < 1:
        raise ValueError("n_r and n_theta must be positive")
    r = np.linspace(float(r_inner), float(r_outer), int(n_r))
    th = np.linspace(float(theta_lo), float(theta_hi), int(n_theta))
    rr, tt = np.meshgrid(r, th, indexing="ij")
    return (float(p.pipe_offset) + rr * np.sin(tt)).ravel(), (rr * np.cos(tt)).ravel()


def skip_travel_time_pipe(xe, ze, xf, zf, *, c_down, c_up=None, r_inner, params: Params = None, alpha_lo=None, alpha_hi=None,
                          beta_lo=-np.pi / 2, beta_hi=np.pi / 2, n_scan=None, return_path=False, out=None, device=0):
    """Bore-reflected skip leg into the pipe wall -> tt[n_e, n_f]: element -> lens -> water -> the pipe's outer circle -> the wall
    at ``c_down`` -> a bounce off the bore (radius ``r_inner`` > 0) -> the wall at ``c_up`` (default ``c_down``; another speed is a
    mode conversion at the bore) -> the point.  travel_time_pipe's geometry, scan and defaults; NaN for a point outside the wall or
    without a qualifying path (no bounce that both the entry point and the point see).  ``return_path``: -> (tt, alpha, beta,
    gamma), the angles of the lens point, the entry point and the bounce.  Definition: include/rtus.h (rtus_tt_pipe_skip).  Not in
    the reference."""
    c_up = c_down if c_up is None else c_up
    lens, a_lo, a_hi, pipe, b_lo, b_hi, n_scan = _pipe_args(params, c_down, r_inner, alpha_lo, alpha_hi, beta_lo, beta_hi, n_scan)
    xe, ze, xf, zf = _points(xe, ze, xf, zf)
    tt = _out(out, (xe.size, xf.size), np.float64)
    al, be, ga = (np.empty((xe.size, xf.size), dtype=np.float64) if return_path else None for _ in range(3))
    st = _lib.lib().rtus_tt_pipe_skip(C.byref(lens), a_lo, a_hi, C.byref(pipe), float(c_up), b_lo, b_hi, n_scan, _ptr(xe), _ptr(ze), xe.size,
                                      _ptr(xf), _ptr(zf), xf.size, _ptr(tt), _ptr(al), _ptr(be), _ptr(ga), int(device))
    _lib.check(st, "rtus_tt_pipe_skip")
    return (tt, al, be, ga) if return_path else tt


def view_legs_pipe(c_l, c_t, r_inner, xe, ze, xf, zf, *, legs=LEGS, params: Params = None, alpha_lo=None, alpha_hi=None,
                   beta_lo=-np.pi / 2, beta_hi=np.pi / 2, n_scan=None, device=0):
    """The leg tables of multi-view TFM of the pipe wall -> {leg: tt [n_e, n_f]} for ``legs`` (default all six: L, T, LL, LT, TL,
    TT), in the shape tfm_views takes.  The wall has speeds ``c_l`` / ``c_t`` and the bore ``r_inner``; the pipe and the lens are
    ``params``'.  Direct legs: travel_time_pipe; skip legs (a bounce off the bore): skip_travel_time_pipe."""
    legs = _legs_wanted(legs)
    sp = {"L": float(c_l), "T": float(c_t)}
    kw = dict(r_inner=r_inner, params=params, alpha_lo=alpha_lo, alpha_hi=alpha_hi, beta_lo=beta_lo, beta_hi=beta_hi, n_scan=n_scan,
              device=device)
    out = {}
    for g in legs:
        if len(g) == 1:
            out[g] = travel_time_pipe(xe, ze, xf, zf, c3=sp[g], **kw)
        else:
            out[g] = skip_travel_time_pipe(xe, ze, xf, zf, c_down=sp[g[0]], c_up=sp[g[1]], **kw)
    return out


def _pipe_amp_args(params, r_inner, alpha_lo, alpha_hi, c_l, c_t, rho_wall, rho_water, rho_lens, ct_lens):
    p = _resolve(params)
    a_lo = -ALPHA_MAX if alpha_lo is None else float(alpha_lo)
    a_hi = ALPHA_MAX if alpha_hi is None else float(alpha_hi)
    pipe = Pipe(float(p.r_outer), float(r_inner), float(p.pipe_offset), 0.0)        # (c3 is not read: the media hold the speeds)
    media = PipeMedia(float(rho_lens), float(ct_lens), float(rho_water), float(rho_wall), float(c_l), float(c_t))
    return p.lens(), a_lo, a_hi, pipe, media


def leg_amplitudes_pipe(leg, xe, ze, xf, zf, alpha, beta, gamma=None, *, c_l, c_t, rho_wall, rho_water, rho_lens, ct_lens, r_inner,
                        up=False, element_width=0.0, f_c=None, params: Params = None, alpha_lo=None, alpha_hi=None, out=None, device=0):
    """Ray amplitudes of one multi-view leg into the pipe wall -> complex64 [n_e, n_f]: A = D C_lens C_outer [C_bore] G (element
    directivity, the displacement coefficients at the lens surface, the pipe's outer circle and the bore, 2-D ray-tube spreading
    through the three curved interfaces), in the analytic signal's phase convention.  ``alpha``, ``beta`` (and ``gamma`` for skip
    legs) [n_e, n_f] are the path as travel_time_pipe(return_path=True) / skip_travel_time_pipe(return_path=True) return it.
    ``up``: the wave travels point -> element along the same path.  The lens is a solid (``rho_lens``, L speed params.c1, shear speed
    ``ct_lens``), the water has ``rho_water`` and params.c2, the wall ``rho_wall``, ``c_l`` > ``c_t``; the pipe is ``params``' with
    the bore ``r_inner``.  ``alpha_lo`` / ``alpha_hi``: the lens interval the times were made with (a path pinned at an end of it
    carries no ray: 0).  ``element_width`` [m] > 0 needs ``f_c`` [Hz].  NaN where the path is NaN.  Definition: include/rtus.h
    (rtus_leg_amp_pipe).  Not in the reference."""
    if leg not in LEGS:
        raise ValueError(f"unknown leg {leg!r}: legs are {LEGS}")
    skip = len(leg) == 2
    xe, ze, xf, zf = _points(xe, ze, xf, zf)
    shape = (xe.size, xf.size)
    al, be = _f64(alpha, "alpha", 2), _f64(beta, "beta", 2)
    if al.shape != shape or be.shape != shape:
        raise ValueError(f"alpha and beta must be [n_e, n_f] = {shape}")
    ga = None
    if skip:
        if gamma is None:
            raise ValueError(f"the skip leg {leg!r} needs gamma")
        ga = _f64(gamma, "gamma", 2)
        if ga.shape != shape:
            raise ValueError(f"gamma must be [n_e, n_f] = {shape}")
    if element_width > 0 and f_c is None:
        raise ValueError("an element width needs the centre frequency f_c")
    lens, a_lo, a_hi, pipe, media = _pipe_amp_args(params, r_inner, alpha_lo, alpha_hi, c_l, c_t, rho_wall, rho_water, rho_lens, ct_lens)
    amp = _out(out, shape, np.complex64)
    st = _lib.lib().rtus_leg_amp_pipe(C.byref(lens), a_lo, a_hi, C.byref(pipe), C.byref(media), LEG_CODES[leg], 1 if up else 0,
                                      float(element_width), float(f_c or 0.0), _ptr(xe), _ptr(ze), xe.size, _ptr(xf), _ptr(zf), xf.size,
                                      _ptr(al), _ptr(be), _ptr(ga), _ptr(amp), int(device))
    _lib.check(st, "rtus_leg_amp_pipe")
    return amp


def view_amplitudes_pipe(xe, ze, xf, zf, *, c_l, c_t, rho_wall, rho_water, rho_lens, ct_lens, r_inner, legs=LEGS, element_width=0.0,
                         f_c=None, params: Params = None, alpha_lo=None, alpha_hi=None, beta_lo=-np.pi / 2, beta_hi=np.pi / 2,
                         n_scan=None, device=0):
    """The leg tables of multi-view TFM of the pipe wall with their ray amplitudes -> (legs_tt, amps): legs_tt = {leg: tt [n_e, n_f]}
    as view_legs_pipe makes them, amps = {leg: (down, up)} complex64 [n_e, n_f] (leg_amplitudes_pipe in both directions on the
    tables' own paths).  Feed both to ``tfm_views(..., envelope=True, amplitudes=amps)``."""
    legs = _legs_wanted(legs)
    sp = {"L": float(c_l), "T": float(c_t)}
    kw = dict(r_inner=r_inner, params=params, alpha_lo=alpha_lo, alpha_hi=alpha_hi, beta_lo=beta_lo, beta_hi=beta_hi, n_scan=n_scan,
              return_path=True, device=device)
    tts, amps = {}, {}
    for g in legs:
        if len(g) == 1:
            tt, al, be = travel_time_pipe(xe, ze, xf, zf, c3=sp[g], **kw)
            ga = None
        else:
            tt, al, be, ga = skip_travel_time_pipe(xe, ze, xf, zf, c_down=sp[g[0]], c_up=sp[g[1]], **kw)
        tts[g] = tt
        amps[g] = tuple(leg_amplitudes_pipe(g, xe, ze, xf, zf, al, be, ga, c_l=c_l, c_t=c_t, rho_wall=rho_wall, rho_water=rho_water,
                                            rho_lens=rho_lens, ct_lens=ct_lens, r_inner=r_inner, up=u, element_width=element_width,
                                            f_c=f_c, params=params, alpha_lo=alpha_lo, alpha_hi=alpha_hi, device=device)
                        for u in (False, True))
    return tts, amps


# ---------------------------------------------------------------------------------------------- pipe geometry from echo times
def pick_echo_times(fmc_or_analytic, fs, t_lo, t_hi, *, t0=0.0, n_taps=63, threshold=0.1, device=0):
    """The arrival time of the strongest echo inside a gate, for every pair of an FMC -> dict(t float64 [n_tx, n_rx], amplitude
    float32 [n_tx, n_rx], valid bool [n_tx, n_rx]).  ``fmc_or_analytic``: a real FMC [n_tx, n_rx, n_t] (its analytic signal is
    formed with ``n_taps`` Hilbert taps) or an analytic one (complex64, or float32 [..., 2]); sample i is at t0 + i / fs.  The gate
    t_lo <= t <= t_hi is two scalars or, either of them, an array [n_tx, n_rx] of per-pair bounds.  A pair's time is that of the
    first maximum of the envelope over the gate's samples, moved by a parabolic step; NaN when the maximum sits on the gate's first
    or last sample, is zero or not finite, or the gate holds no sample of the record.  A pair is valid where its time is finite and
    its amplitude is at least ``threshold`` times the largest.  Definition: include/rtus.h (rtus_echo_pick).  Not in the
    reference."""
    a = np.asarray(fmc_or_analytic)
    if a.ndim == 3 and not np.iscomplexobj(a):
        a = fmc_analytic(a, n_taps, device=device)
    a = _complex_fmc(a)

    def bound(v, name):
        if np.ndim(v) == 0:
            return float(v), None
        arr = np.ascontiguousarray(v, dtype=np.float64)
        if arr.shape != a.shape[:2]:
            raise ValueError(f"{name} must be a scalar or an array of shape {a.shape[:2]}")
        return 0.0, arr
    lo, lo_arr = bound(t_lo, "t_lo")
    hi, hi_arr = bound(t_hi, "t_hi")
    t = np.empty(a.shape[:2], dtype=np.float64)
    amp = np.empty(a.shape[:2], dtype=np.float32)
    st = _lib.lib().rtus_echo_pick(_ptr(a), a.shape[0], a.shape[1], a.shape[2], float(fs), float(t0), lo, hi, _ptr(lo_arr), _ptr(hi_arr),
                                   _ptr(t), _ptr(amp), int(device))
    _lib.check(st, "rtus_echo_pick")
    fin = np.isfinite(amp)
    top = amp[fin].max() if fin.any() else np.nan
    with np.errstate(invalid="ignore"):
        valid = np.isfinite(t) & fin & (amp >= threshold * top)
    return dict(t=t, amplitude=amp, valid=valid)


def geom_misfit(tt, t_meas, weights=None, *, device=0):
    """rtus_geom_misfit on host arrays: tt [G, T, E], t_meas [T, E], weights [T, E] or None -> (n int32 [G], sse, sum_r, sum_w
    float64 [G]) over the pairs where both times are finite and the weight is positive (include/rtus.h)."""
    tt = np.ascontiguousarray(tt, dtype=np.float64)
    tm = np.ascontiguousarray(t_meas, dtype=np.float64)
    if tt.ndim != 3 or tm.shape != tt.shape[1:]:
        raise ValueError("tt must be [G, T, E] and t_meas [T, E]")
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    if w is not None and w.shape != tm.shape:
        raise ValueError("weights must have t_meas's shape")
    G = tt.shape[0]
    n = np.empty(G, dtype=np.int32)
    sse, sr, sw = np.empty(G), np.empty(G), np.empty(G)
    st = _lib.lib().rtus_geom_misfit(_ptr(tt), G, tt.shape[1], tt.shape[2], _ptr(tm), _ptr(w), _ptr(n), _ptr(sse), _ptr(sr), _ptr(sw),
                                     int(device))
    _lib.check(st, "rtus_geom_misfit")
    return n, sse, sr, sw


def _misfit_stats(n, sse, sr, sw, fit_delay):
    """(mse, delay) per geometry from rtus_geom_misfit's sums: delay = the common offset of t_meas over the model, the weighted
    mean of t_meas - tt (0 unless fitted); mse = the weighted sum of squares left, over n (NaN where n = 0)"""
    with np.errstate(invalid="ignore", divide="ignore"):
        if fit_delay:
            delay = np.where(n > 0, -sr / sw, np.nan)
            mse = np.where(n > 0, np.maximum(sse - sr * sr / sw, 0.0) / n, np.nan)
        else:
            delay = np.where(n > 0, 0.0, np.nan)
            mse = np.where(n > 0, sse / n, np.nan)
    return mse, delay


def _meas(t_meas, x_a, x_rx, weights):
    x_a, x_rx = _f64(x_a, "x_a"), _f64(x_rx, "x_rx")
    tm = np.ascontiguousarray(t_meas, dtype=np.float64)
    if tm.shape != (x_a.size, x_rx.size):
        raise ValueError(f"t_meas must be [n_tx, n_rx] = {(x_a.size, x_rx.size)}, got {tm.shape}")
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    if w is not None and w.shape != tm.shape:
        raise ValueError("weights must have t_meas's shape")
    return tm, w


def pipe_misfit(t_meas, x_a, z_a, x_rx, alpha, geoms, *, weights=None, fit_delay=False, params: Params = None, device=0, **solve):
    """The misfit of measured pulse-echo times t_meas [n_tx, n_rx] (NaN: no echo) to the model times of every geometry of
    ``geoms`` [G, 2] = (r_outer, pipe_offset): one solve_travel_times call (its arguments x_a, z_a, x_rx, alpha and options
    ``**solve``) and one rtus_geom_misfit launch — the reference's database search (main_compare.py:526-553) on any batch of
    geometries.  -> dict(mse [G]: the weighted mean squared residual over the n [G] pairs where the model and the measurement are
    both finite and the weight positive, NaN where there is none; delay [G]: with ``fit_delay`` the common offset of the
    measurement over the model (t_meas = model + delay, removed from mse in closed form), else 0)."""
    tm, w = _meas(t_meas, x_a, x_rx, weights)
    tt = solve_travel_times(x_a, z_a, x_rx, alpha, geoms, params=params, device=device, **solve)[0]
    n, sse, sr, sw = geom_misfit(tt, tm, w, device=device)
    mse, delay = _misfit_stats(n, sse, sr, sw, fit_delay)
    return dict(mse=mse, n=n, delay=delay)


FIT_STEP = (2e-5, 2e-5)      # fit_pipe's central-difference half steps in (r_outer, pipe_offset) [m]
FIT_TOL = 1e-10              # fit_pipe stops when both components of the step are below this [m]


def pipe_clearance(pipe_offset, *, params: Params = None, alpha_lo=None, alpha_hi=None):
    """The radius a pipe centred at (pipe_offset, 0) must stay under for travel_time_pipe to take it: the least distance from its
    centre to the lens surface (rtus_pipe_clearance)."""
    p = _resolve(params)
    lens = p.lens()
    a_lo = -ALPHA_MAX if alpha_lo is None else float(alpha_lo)
    a_hi = ALPHA_MAX if alpha_hi is None else float(alpha_hi)
    return float(_lib.lib().rtus_pipe_clearance(C.byref(lens), a_lo, a_hi, float(pipe_offset)))


def fit_pipe(t_meas, x_a, z_a, x_rx, alpha, *, radii=None, offsets=None, min_pairs=8, fit_delay=False, weights=None, max_iter=40,
             params: Params = None, device=0, **solve):
    """The pipe's outer radius and offset from measured pulse-echo times t_meas [n_tx, n_rx] of its outer surface (NaN: no echo;
    pick_echo_times makes them from an FMC), by least squares against solve_travel_times' model.

    1. A coarse map: pipe_misfit over ``radii`` x ``offsets`` (default: the reference's sweep, drivers.sweep_geometries(): 1..10 cm
       by -10..10 mm).  Nodes with fewer than ``min_pairs`` counting pairs, and nodes travel_time_pipe would reject for touching
       the lens (pipe_clearance), are out.  ValueError when none is left.
    2. Levenberg-Marquardt from the best node.  Every iteration is one solve_travel_times call on five geometries — the centre and
       +-FIT_STEP in r_outer and in pipe_offset — and one rtus_geom_misfit launch: the launch gives the centre's cost (and delay),
       the five tables give the residuals and their central differences over the pairs that are finite at all five.  A step
       whose centre costs more than the last accepted one, has fewer than ``min_pairs`` pairs or would touch the lens is taken
       back and the damping raised tenfold; an accepted one lowers it tenfold.
    3. It stops when both components of the next step are below FIT_TOL (converged), or after ``max_iter`` iterations.

    -> dict(r_outer, pipe_offset, delay (0 unless ``fit_delay``), mse, n_pairs, cov [2, 2] = s^2 (J^T J)^-1 with s^2 the residual
    variance (weighted sum of squares over n_pairs - the number of fitted parameters), grid_mse [n_radii, n_offsets] (NaN where
    a node is out), iterations, converged).  The geometry returned is always one travel_time_pipe takes."""
    p = _resolve(params)
    tm, w = _meas(t_meas, x_a, x_rx, weights)
    if radii is None or offsets is None:
        from . import drivers                              # (drivers imports this module)
        ref = drivers.sweep_geometries()                   # radius-major: 10 radii x 21 offsets
        radii = ref[::21, 0] if radii is None else radii
        offsets = ref[:21, 1] if offsets is None else offsets
    radii, offsets = _f64(radii, "radii"), _f64(offsets, "offsets")
    min_pairs = int(min_pairs)
    n_par = 3 if fit_delay else 2
    if min_pairs < n_par + 1:
        raise ValueError(f"min_pairs must be at least {n_par + 1}: the fit has {n_par} parameters")
    a_lo, a_hi = float(np.min(alpha)), float(np.max(alpha))
    dr, dx = FIT_STEP

    def fits(r, x):
        """the five geometries about (r, x) are pipes below the lens"""
        return r - dr > 0 and all(r + dr < pipe_clearance(x + s, params=p, alpha_lo=a_lo, alpha_hi=a_hi) for s in (-dx, 0.0, dx))

    geoms = np.asarray([[r, x] for r in radii for x in offsets], dtype=np.float64)
    grid = pipe_misfit(tm, x_a, z_a, x_rx, alpha, geoms, weights=w, fit_delay=fit_delay, params=p, device=device, **solve)
    ok = (grid["n"] >= min_pairs) & np.isfinite(grid["mse"]) & np.asarray([fits(r, x) for r, x in geoms])
    grid_mse = np.where(ok, grid["mse"], np.nan).reshape(radii.size, offsets.size)
    if not ok.any():
        raise ValueError(f"no node of the geometry grid has {min_pairs} pairs with both a measured and a model time "
                         f"(the most: {int(grid['n'].max())})")
    x = geoms[np.nanargmin(np.where(ok, grid["mse"], np.nan))].copy()
    sw_all = np.ones_like(tm) if w is None else w
    lam, last, it, converged = 1e-3, None, 0, False      # last: the accepted state (x, mse, delay, n, JtJ, Jtr, s2)
    step = None
    while it < int(max_iter):
        if last is not None:
            x = last["x"] + step
            if not fits(x[0], x[1]):                      # no solve: the step is taken back
                lam *= 10.0
                step = _lm_step(last, lam)
                if lam > 1e12:
                    break
                continue
        it += 1
        g5 = np.asarray([x, x + [dr, 0], x - [dr, 0], x + [0, dx], x - [0, dx]], dtype=np.float64)
        tt = solve_travel_times(x_a, z_a, x_rx, alpha, g5, params=p, device=device, **solve)[0]
        n, sse, sr, sw = geom_misfit(tt, tm, w, device=device)
        mse, delay = _misfit_stats(n, sse, sr, sw, fit_delay)
        if n[0] < min_pairs or not np.isfinite(mse[0]) or (last is not None and mse[0] > last["mse"]):
            if last is None:
                raise ValueError("the best grid node lost its pairs")       # (cannot happen: the map counted them)
            lam *= 10.0
            step = _lm_step(last, lam)
            if abs(step[0]) <= FIT_TOL and abs(step[1]) <= FIT_TOL:
                converged = True                          # nothing better within a step of the tolerance
                break
            if lam > 1e12:
                break
            continue
        with np.errstate(invalid="ignore"):
            use = np.isfinite(tt).all(axis=0) & np.isfinite(tm) & (sw_all > 0)
        res = (tt[0] - tm)[use]
        J = np.stack([(tt[1] - tt[2])[use] / (2 * dr), (tt[3] - tt[4])[use] / (2 * dx)], axis=1)
        wt = sw_all[use]
        if fit_delay and wt.size:                         # the common offset projected out of the residuals and of the Jacobian
            res = res - np.sum(wt * res) / np.sum(wt)
            J = J - (wt @ J) / np.sum(wt)
        JtJ, Jtr = J.T @ (J * wt[:, None]), J.T @ (wt * res)
        dof = max(int(use.sum()) - n_par, 1)
        state = dict(x=x.copy(), mse=float(mse[0]), delay=float(delay[0]), n=int(n[0]), JtJ=JtJ, Jtr=Jtr,
                     s2=float(np.sum(wt * res * res)) / dof, n_use=int(use.sum()))
        if last is not None:
            lam = max(lam / 10.0, 1e-12)
        last = state
        if state["n_use"] < n_par or not np.all(np.isfinite(JtJ)) or np.linalg.cond(JtJ) > 1e15:
            break                                         # the pairs left do not determine a step
        step = _lm_step(last, lam)
        if abs(step[0]) <= FIT_TOL and abs(step[1]) <= FIT_TOL:
            converged = True
            break
    with np.errstate(all="ignore"):
        try:
            cov = last["s2"] * np.linalg.inv(last["JtJ"])
        except np.linalg.LinAlgError:
            cov = np.full((2, 2), np.nan)
    return dict(r_outer=float(last["x"][0]), pipe_offset=float(last["x"][1]), delay=last["delay"], mse=last["mse"], n_pairs=last["n"],
                cov=cov, grid_mse=grid_mse, iterations=it, converged=converged)


def _lm_step(state, lam):
    """(J^T J + lam diag(J^T J)) step = -J^T r"""
    A = state["JtJ"] + lam * np.diag(np.diag(state["JtJ"]))
    return -np.linalg.solve(A, state["Jtr"])


def adaptive_tfm_pipe(fmc, fs, xe, ze, xf, zf, *, t_lo, t_hi, c3, r_inner, t0=0.0, alpha=None, n_taps=63, threshold=0.1, envelope=False,
                      fit_delay=False, min_pairs=8, radii=None, offsets=None, max_iter=40, params: Params = None, device=0, **solve):
    """Adaptive TFM of a pipe wall: pick the outer-surface echo of every pair of a square FMC inside the gate [t_lo, t_hi]
    (pick_echo_times), fit the pipe's radius and offset to the valid picks (fit_pipe; the elements (xe, ze) transmit and receive,
    ``alpha``: the launch-angle grid of the model, default 905 angles over +-ALPHA_MAX as in the reference's sweep), build the
    wall's travel times for the fitted geometry (travel_time_pipe with speed ``c3`` and bore ``r_inner``) and image the points
    (xf, zf): tfm_image, or with ``envelope=True`` the envelope np.abs(tfm_analytic(...)).  The analytic FMC is formed once.
    A fitted delay shifts the record's time origin for the image (an echo the model puts at t is looked up at t + delay).
    -> (image float32 [n_f], fit dict of fit_pipe plus ``picks``: the dict of pick_echo_times)."""
    p = _resolve(params)
    fmc = np.ascontiguousarray(fmc, dtype=np.float32)
    if fmc.ndim != 3 or fmc.shape[0] != fmc.shape[1]:
        raise ValueError("fmc must be a square block [n_e, n_e, n_t]")
    xe, ze = _f64(xe, "xe"), _f64(ze, "ze")
    if xe.size != fmc.shape[0] or ze.size != fmc.shape[0]:
        raise ValueError("xe / ze must hold one position per element of the FMC")
    alpha = np.linspace(-ALPHA_MAX, ALPHA_MAX, 905) if alpha is None else _f64(alpha, "alpha")
    analytic = fmc_analytic(fmc, n_taps, device=device)
    picks = pick_echo_times(analytic, fs, t_lo, t_hi, t0=t0, threshold=threshold, device=device)
    tm = np.where(picks["valid"], picks["t"], np.nan)
    fit = fit_pipe(tm, xe, ze, xe, alpha, radii=radii, offsets=offsets, min_pairs=min_pairs, fit_delay=fit_delay, max_iter=max_iter,
                   params=p, device=device, **solve)
    fitted = replace(p, r_outer=fit["r_outer"], pipe_offset=fit["pipe_offset"])
    tt = travel_time_pipe(xe, ze, xf, zf, c3=c3, r_inner=r_inner, params=fitted, alpha_lo=float(alpha[0]), alpha_hi=float(alpha[-1]),
                          device=device)
    fit["picks"] = picks
    if envelope:
        return np.abs(tfm_analytic(analytic, fs, tt, t0=t0 - fit["delay"], device=device)), fit
    return tfm_image(fmc, fs, tt, t0=t0 - fit["delay"], device=device), fit


# ---------------------------------------------------------------------------------------------- specular echoes of a reflector
def specular_times(tt_a, tt_b=None, *, n_refl=1, return_pos=False, return_minima=False, device=0):
    """Specular echo times of ``n_refl`` sampled reflectors for every (transmitter, receiver) pair: the stationary value over a
    reflector's points of tt_a[i, j] + tt_b[k, j], refined by a parabola about the first least sum (include/rtus.h, rtus_specular).
    ``tt_a`` [n_a, n_refl * n_p]: times from the transmitters to the points, reflector g in columns [g n_p, (g + 1) n_p), its points
    in order along it — what a table call over the concatenated points returns; ``tt_b`` [n_b, n_refl * n_p]: the receivers' (None:
    tt_a).  -> t float64 [n_a, n_b], or [n_refl, n_a, n_b] when n_refl > 1; NaN where no sum is finite or the least one is not
    bracketed by the sampled span.  ``return_pos``: also the reflection point in units of the point index; ``return_minima``: also
    n_min int32, the number of strict interior minima (above 1: two paths compete) -> (t, pos, n_min), those asked for.  Not in the
    reference."""
    tt_a = np.ascontiguousarray(tt_a, dtype=np.float64)
    tt_b = None if tt_b is None else np.ascontiguousarray(tt_b, dtype=np.float64)
    n_refl = int(n_refl)
    if tt_a.ndim != 2 or tt_a.size == 0 or n_refl < 1 or tt_a.shape[1] % n_refl:
        raise ValueError("tt_a must be [n_a, n_refl * n_p]")
    if tt_b is not None and (tt_b.ndim != 2 or tt_b.shape[0] == 0 or tt_b.shape[1] != tt_a.shape[1]):
        raise ValueError("tt_b must be [n_b, n_refl * n_p], the columns of tt_a")
    n_a, n_b = tt_a.shape[0], tt_a.shape[0] if tt_b is None else tt_b.shape[0]
    shape = (n_a, n_b) if n_refl == 1 else (n_refl, n_a, n_b)
    t = np.empty(shape, dtype=np.float64)
    pos = np.empty(shape, dtype=np.float64) if return_pos else None
    n_min = np.empty(shape, dtype=np.int32) if return_minima else None
    st = _lib.lib().rtus_specular(_ptr(tt_a), n_a, _ptr(tt_b), n_b, n_refl, tt_a.shape[1] // n_refl, _ptr(t), _ptr(pos), _ptr(n_min),
                                  int(device))
    _lib.check(st, "rtus_specular")
    extra = [v for v in (pos, n_min) if v is not None]
    return (t, *extra) if extra else t


def _candidates(values, name):
    v = _f64(values, name)
    if v.size == 0:
        raise ValueError(f"{name} must hold at least one candidate")
    return v


def _span_points(lo, hi, n_p):
    if int(n_p) < 1:
        raise ValueError("n_p must be positive")
    return np.linspace(float(lo), float(hi), int(n_p))


def _echo(table, c_down, c_up, n_refl, device):
    """the two legs (one table call when the return leg has the down leg's speed) and one rtus_specular launch -> t [G, n_e, n_e]"""
    down = table(c_down)
    up = None if c_up is None or float(c_up) == float(c_down) else table(float(c_up))
    return specular_times(down, up, n_refl=n_refl, device=device).reshape(n_refl, down.shape[0], down.shape[0])


def backwall_echo_layers(z_if, c, z_back, xe, ze, x_lo, x_hi, n_p, *, c_up=None, taup=False, device=0):
    """Pulse-echo times of a planar backwall under horizontal layers, for every pair of the aperture (xe, ze) and for every
    candidate depth of ``z_back`` (a scalar or an array [G]) -> t [G, n_e, n_e].  Each backwall is sampled at ``n_p`` points evenly
    over [x_lo, x_hi]; down leg: travel_time_layers(z_if, c) to the points, up leg the same with ``c[-1]`` replaced by ``c_up``
    (skip_travel_time_layers' meaning: another speed is a mode conversion at the backwall; default c[-1]); then specular_times.
    NaN where the reflection point is not inside the sampled span.  Every candidate must lie below the last interface."""
    z_if, c = _medium(z_if, c)
    zb = _candidates(z_back, "z_back")
    if z_if.size and not np.all(zb > z_if[-1]):
        raise ValueError("the backwall must lie below the last interface (z_back > z_if[-1])")
    xs = _span_points(x_lo, x_hi, n_p)
    xf, zf = np.tile(xs, zb.size), np.repeat(zb, xs.size)
    return _echo(lambda cl: travel_time_layers(z_if, np.r_[c[:-1], cl], xe, ze, xf, zf, taup=taup, device=device), c[-1], c_up, zb.size,
                 device)


def backwall_echo_surface(x0, dx, zs, c1, c2, z_back, xe, ze, x_lo, x_hi, n_p, *, c_up=None, device=0):
    """backwall_echo_layers under ONE measured front surface (travel_time_surface's profile ``zs`` at x0 + k dx, couplant ``c1``,
    part ``c2`` on the way down and ``c_up`` on the way up; default c2) -> t [G, n_e, n_e] for the candidate depths ``z_back``."""
    zb = _candidates(z_back, "z_back")
    xs = _span_points(x_lo, x_hi, n_p)
    xf, zf = np.tile(xs, zb.size), np.repeat(zb, xs.size)
    return _echo(lambda cl: travel_time_surface(x0, dx, zs, c1, cl, xe, ze, xf, zf, device=device), float(c2), c_up, zb.size, device)


def bore_echo_pipe(r_inner, xe, ze, theta_lo, theta_hi, n_p, *, c_down, c_up=None, params: Params = None, alpha_lo=None, alpha_hi=None,
                   n_scan=None, device=0):
    """Pulse-echo times of the pipe's bore, for every pair of the aperture behind the lens and for every candidate radius of
    ``r_inner`` (a scalar or an array [G]) -> t [G, n_e, n_e].  Each bore is sampled at ``n_p`` angles evenly over
    [theta_lo, theta_hi] on the circle of that radius about the pipe's centre (pipe_wall_grid's convention); the legs are
    travel_time_pipe tables at wall speed ``c_down`` and ``c_up`` (default c_down; another speed is a mode conversion at the bore),
    called with a solid bar (its own r_inner = 0) so that every candidate lies inside the wall it accepts.  The reference's lens
    focuses on the pipe's axis: inside the wall an element's wave converges on a point near the axis, and the bore's echo is a
    LEAST time only for pairs that mirror each other about the lens axis — the others come out NaN."""
    p = _resolve(params)
    r = _candidates(r_inner, "r_inner")
    th = _span_points(theta_lo, theta_hi, n_p)
    xf = (float(p.pipe_offset) + r[:, None] * np.sin(th)[None]).ravel()
    zf = (r[:, None] * np.cos(th)[None]).ravel()
    return _echo(lambda cl: travel_time_pipe(xe, ze, xf, zf, c3=cl, r_inner=0.0, params=p, alpha_lo=alpha_lo, alpha_hi=alpha_hi,
                                             n_scan=n_scan, device=device), float(c_down), c_up, r.size, device)


def fit_reflector(t_meas, model, lo, hi, *, n_grid=33, passes=3, weights=None, fit_delay=False, min_pairs=8, device=0):
    """One parameter of a reflector (a backwall's depth, a bore's radius) from measured echo times t_meas [n_tx, n_rx] (NaN: no
    echo), by least squares over [lo, hi].  ``model(values [G]) -> tt [G, n_tx, n_rx]`` is any callable, e.g.
    ``lambda z: backwall_echo_surface(x0, dx, zs, c1, c2, z, xe, ze, x_lo, x_hi, n_p)``.

    Each of ``passes`` passes takes ``n_grid`` values evenly over the bracket (first [lo, hi]), makes one model call and one
    rtus_geom_misfit launch, and keeps the first value of least mean squared residual among those with at least ``min_pairs``
    counting pairs; the next bracket is that value's two neighbours (cut to the bracket).  After the last pass a parabola through
    the best value and its neighbours (where it is interior and all three count) gives the value, clamped to those neighbours;
    mse, n and delay are then evaluated at it.

    -> dict(value, mse, n, delay (0 unless ``fit_delay``: t_meas = model + delay), ok, history: per pass dict(values, mse, n,
    best)).  ``ok`` is False when in some pass no value reaches min_pairs (value is then NaN), or when the first pass's best is
    lo or hi: the range does not bracket the answer."""
    tm = np.ascontiguousarray(t_meas, dtype=np.float64)
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    if tm.ndim != 2 or (w is not None and w.shape != tm.shape):
        raise ValueError("t_meas must be [n_tx, n_rx] and weights of its shape")
    n_grid, passes, min_pairs = int(n_grid), int(passes), int(min_pairs)
    if n_grid < 3 or passes < 1 or not float(hi) > float(lo):
        raise ValueError("need n_grid >= 3, passes >= 1 and lo < hi")
    if min_pairs < (3 if fit_delay else 2):
        raise ValueError(f"min_pairs must be at least {3 if fit_delay else 2}: one more than the fitted parameters")

    def score(values):
        n, sse, sr, sw = geom_misfit(model(values), tm, w, device=device)
        mse, delay = _misfit_stats(n, sse, sr, sw, fit_delay)
        return np.where(n >= min_pairs, mse, np.nan), n, delay

    a, b, ok, history = float(lo), float(hi), True, []
    fail = dict(value=np.nan, mse=np.nan, n=0, delay=np.nan, ok=False, history=history)
    for it in range(passes):
        values = np.linspace(a, b, n_grid)
        mse, n, _ = score(values)
        if not np.isfinite(mse).any():
            return fail
        k = int(np.nanargmin(mse))                       # the first of least mse
        history.append(dict(values=values, mse=mse, n=n, best=k))
        if it == 0 and k in (0, n_grid - 1):
            ok = False
        a, b = values[max(k - 1, 0)], values[min(k + 1, n_grid - 1)]
    value = values[k]
    if 0 < k < n_grid - 1 and np.isfinite(mse[k - 1]) and np.isfinite(mse[k + 1]):
        d2 = (mse[k - 1] - mse[k]) + (mse[k + 1] - mse[k])
        if d2 > 0:
            value = min(max(value + 0.5 * (mse[k - 1] - mse[k + 1]) / d2 * (values[k + 1] - values[k]), a), b)
    mse, n, delay = score(np.asarray([value]))
    if not np.isfinite(mse[0]):
        return fail
    return dict(value=float(value), mse=float(mse[0]), n=int(n[0]), delay=float(delay[0]), ok=ok, history=history)


def measure_reflector(fmc_or_analytic, fs, model, lo, hi, *, t0=0.0, margin, threshold=0.1, n_taps=63, **fit):
    """The reflector's parameter from an FMC: per-pair gates from the model over fit_reflector's first-pass candidates (the least
    model time of a pair minus ``margin`` to the greatest plus ``margin``; a pair without a model time has no gate), pick_echo_times
    inside them, fit_reflector (options ``**fit``) on the valid picks -> fit_reflector's dict plus ``picks``: the dict of
    pick_echo_times."""
    tt = np.asarray(model(np.linspace(float(lo), float(hi), int(fit.get("n_grid", 33)))), dtype=np.float64)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)   # a pair that is NaN for every candidate: a NaN gate, no pick
        g_lo, g_hi = np.nanmin(tt, axis=0) - float(margin), np.nanmax(tt, axis=0) + float(margin)
    picks = pick_echo_times(fmc_or_analytic, fs, g_lo, g_hi, t0=t0, n_taps=n_taps, threshold=threshold, device=fit.get("device", 0))
    out = fit_reflector(np.where(picks["valid"], picks["t"], np.nan), model, lo, hi, **fit)
    out["picks"] = picks
    return out


# ---------------------------------------------------------------------------------------------- skip legs off a sampled backwall
def skip_travel_time_reflector(tt_down, xb, zb, c_up, xf, zf, *, return_pos=False, return_minima=False, out=None, device=0):
    """Element x focal-point times of a SKIP leg off a reflector of any sampled shape -> tt [n_e, n_f]: element -> the reflector's
    point B -> focal point F, stationary over B in tt_down[e, j] + |F - B_j| / c_up, refined by a parabola about the first least
    sum (include/rtus.h, rtus_skip_reflector: rtus_specular's rules with the up leg formed on the fly).  ``tt_down`` [n_e, n_p]:
    times from the elements to the reflector's points (xb, zb) in order along it — what any table call over (xb, zb) returns;
    ``c_up``: the speed of the up leg (another speed than the down leg's is a mode conversion at the reflector).  NaN where no sum
    is finite or the least one is not bracketed by the sampled span.  ``return_pos``: also the bounce point in units of the point
    index; ``return_minima``: also n_min int32, the number of strict interior minima (above 1: two bounce points compete) ->
    (tt, pos, n_min), those asked for.  ``out``: optional float64 [n_e, n_f] buffer for tt.

    Accuracy and sampling: the parabola's value is third order in the point spacing in general, fourth order only where the sum is
    symmetric about its minimum (the case rtus_specular quotes), and the constant grows as the focal point nears the reflector.
    One medium at 5900 m/s, 16 elements, a flat backwall at 30 mm sampled over +-20 mm, points at z 6 - 26 mm against the mirror
    image: 4.3e-10, 6.3e-11, 7.3e-12 s at 41, 81, 161 points; tilted by 5 degrees 7.2e-10, 7.3e-11, 1.0e-11 s.  Sample at a
    quarter of a millimetre or finer for points a few millimetres off the wall.  A point whose bounce falls outside the sampled
    span is NaN, so the span must overhang the image.  The straight up leg is not checked against the reflector itself.  Not in
    the reference."""
    tt_down = np.ascontiguousarray(tt_down, dtype=np.float64)
    xb, zb, xf, zf = _points(xb, zb, xf, zf)
    if tt_down.ndim != 2 or tt_down.size == 0 or tt_down.shape[1] != xb.size:
        raise ValueError("tt_down must be [n_e, n_p] with one column per reflector point (xb, zb)")
    if xf.size == 0:
        raise ValueError("xf / zf must hold at least one focal point")
    c_up = float(c_up)
    if not (np.isfinite(c_up) and c_up > 0):
        raise ValueError("c_up must be finite and positive")
    shape = (tt_down.shape[0], xf.size)
    tt = _out(out, shape, np.float64)
    pos = np.empty(shape, dtype=np.float64) if return_pos else None
    n_min = np.empty(shape, dtype=np.int32) if return_minima else None
    st = _lib.lib().rtus_skip_reflector(_ptr(tt_down), shape[0], _ptr(xb), _ptr(zb), xb.size, c_up, _ptr(xf), _ptr(zf), xf.size,
                                        _ptr(tt), _ptr(pos), _ptr(n_min), int(device))
    _lib.check(st, "rtus_skip_reflector")
    extra = [v for v in (pos, n_min) if v is not None]
    return (tt, *extra) if extra else tt


def _reflector(xb, zb):
    xb, zb = _f64(xb, "xb"), _f64(zb, "zb")
    if xb.shape != zb.shape or xb.size < 2 or not np.all(np.diff(xb) > 0):
        raise ValueError("xb / zb must pair up, hold at least two points, and xb must be strictly increasing")
    return xb, zb


def reflector_mask(xb, zb, xf, zf):
    """Which focal points a skip leg off the sampled reflector (xb, zb) can serve -> bool [n_f]: True where xb[0] <= xf <= xb[-1]
    and zf < np.interp(xf, xb, zb) — the point lies strictly above the polyline through the reflector's points (z down).  ``xb``
    must be strictly increasing.  Host only."""
    xb, zb = _reflector(xb, zb)
    xf, zf = _f64(xf, "xf"), _f64(zf, "zf")
    if xf.shape != zf.shape:
        raise ValueError("xf / zf must pair up")
    with np.errstate(invalid="ignore"):
        return (xf >= xb[0]) & (xf <= xb[-1]) & (zf < np.interp(xf, xb, zb))


def _skip_profile(down, xb, zb, c_up, xf, zf, mask, return_pos, device):
    """the kernel on a down table, the validity mask, and the bounce point in metres"""
    r = skip_travel_time_reflector(down, xb, zb, c_up, xf, zf, return_pos=return_pos, device=device)
    tt = r[0] if return_pos else r
    tt[:, ~mask] = np.nan
    if not return_pos:
        return tt
    pos = r[1]
    x_back = np.full(pos.shape, np.nan)
    fin = np.isfinite(pos)
    x_back[fin] = np.interp(pos[fin], np.arange(xb.size, dtype=np.float64), xb)
    x_back[:, ~mask] = np.nan
    return tt, x_back


def _layers_profile_args(z_if, xb, zb, xf, zf):
    """the checks and the mask the layered profile functions share -> (xb, zb, xf, zf, mask)"""
    xb, zb = _reflector(xb, zb)
    xf, zf = _f64(xf, "xf"), _f64(zf, "zf")
    if xf.shape != zf.shape:
        raise ValueError("xe/ze and xf/zf must pair up")
    front = float(z_if[-1]) if len(z_if) else -np.inf
    if not np.all(zb > front):
        raise ValueError("the backwall must lie below the last interface (every zb > z_if[-1])")
    if len(z_if) > MAX_LAYERS:
        raise ValueError(f"at most {MAX_LAYERS} interfaces above the backwall")
    with np.errstate(invalid="ignore"):
        return xb, zb, xf, zf, (zf > front) & reflector_mask(xb, zb, xf, zf)


def skip_travel_time_layers_profile(z_if, c, xb, zb, xe, ze, xf, zf, *, c_up=None, taup=False, return_pos=False, device=0):
    """skip_travel_time_layers under a backwall of any sampled shape -> tt [n_e, n_f]: down through the layers ``z_if`` / ``c`` to
    the backwall's points (xb, zb) (travel_time_layers; ``xb`` strictly increasing, every ``zb`` below z_if[-1]), then up at
    ``c_up`` (default c[-1]; another speed is a mode conversion) to the point (skip_travel_time_reflector, which also states the
    accuracy and the sampling to choose: a quarter of a millimetre or finer, the span overhanging the image).  NaN where the point
    is not strictly below z_if[-1] or ``reflector_mask`` is False, and where the bounce is not bracketed by the span.
    ``return_pos``: -> (tt, x_back), the bounce point's x in metres (np.interp of the bounce index over xb).  A tapered, corroded
    or machined backwall, a weld root; the profile may come from ``backwall_profile``.  Not in the reference."""
    z_if, c = _medium(z_if, c)
    xb, zb, xf, zf, mask = _layers_profile_args(z_if, xb, zb, xf, zf)
    c_up = float(c[-1]) if c_up is None else float(c_up)
    down = travel_time_layers(z_if, c, xe, ze, xb, zb, taup=taup, device=device)
    return _skip_profile(down, xb, zb, c_up, xf, zf, mask, return_pos, device)


def _surface_profile_args(x0, dx, zs, xb, zb, xf, zf):
    """the checks and the mask the profile functions under a measured surface share -> (xb, zb, xf, zf, mask)"""
    zs = _f64(zs, "zs")
    xb, zb = _reflector(xb, zb)
    xf, zf = _f64(xf, "xf"), _f64(zf, "zf")
    if xf.shape != zf.shape:
        raise ValueError("xe/ze and xf/zf must pair up")
    if zs.size < 2 or not float(dx) > 0:
        raise ValueError("the front profile needs at least two samples and dx > 0")
    xs = float(x0) + np.arange(zs.size) * float(dx)
    if not (xb[0] >= xs[0] and xb[-1] <= xs[-1] and np.all(zb > np.interp(xb, xs, zs))):
        raise ValueError("the backwall must lie inside the front profile's extent and strictly below it")
    with np.errstate(invalid="ignore"):
        below = (xf >= xs[0]) & (xf <= xs[-1]) & (zf > np.interp(xf, xs, zs))
    return xb, zb, xf, zf, below & reflector_mask(xb, zb, xf, zf)


def skip_travel_time_surface_profile(x0, dx, zs, c1, c2, xb, zb, xe, ze, xf, zf, *, c_up=None, return_pos=False, device=0):
    """skip_travel_time_layers_profile under ONE measured front surface (travel_time_surface's profile ``zs`` at x0 + k dx, couplant
    ``c1``, part ``c2`` on the way down and ``c_up`` on the way up; default c2) -> tt [n_e, n_f], with ``return_pos`` (tt, x_back).
    The down table is travel_time_surface to the backwall's points.  NaN where the point is outside the front profile's extent, not
    strictly below the front profile, or where ``reflector_mask`` is False.  This mask is the POLYLINE through the front profile's
    samples, not travel_time_surface's spline: a point between the two is masked by one and not the other.  The backwall must lie
    inside the extent and strictly below the polyline.  Accuracy and sampling: skip_travel_time_reflector.  Not in the reference."""
    xb, zb, xf, zf, mask = _surface_profile_args(x0, dx, zs, xb, zb, xf, zf)
    c_up = float(c2) if c_up is None else float(c_up)
    down = travel_time_surface(x0, dx, zs, c1, c2, xe, ze, xb, zb, device=device)
    return _skip_profile(down, xb, zb, c_up, xf, zf, mask, return_pos, device)


def _view_legs_profile(legs, direct, down_table, skip):
    """{leg: tt}: direct legs as today, one down table per down mode shared by the two skip legs that start in it"""
    out, down = {}, {}
    for g in legs:
        if len(g) == 1:
            out[g] = direct(g)
        else:
            if g[0] not in down:
                down[g[0]] = down_table(g[0])
            out[g] = skip(down[g[0]], g[1])
    return out


def view_legs_layers_profile(z_if, c_above, c_l, c_t, xb, zb, xe, ze, xf, zf, *, legs=LEGS, device=0):
    """view_legs_layers under a backwall of any sampled shape (xb, zb) -> {leg: tt [n_e, n_f]} in the shape tfm_views and
    simulate_views take.  Direct legs: travel_time_layers; skip legs: skip_travel_time_layers_profile's, the down table made once
    per down mode (LL and LT share the L table, TL and TT the T table)."""
    legs = _legs_wanted(legs)
    z_if = list(np.atleast_1d(np.asarray(z_if, dtype=np.float64)))
    c_above = list(np.atleast_1d(np.asarray(c_above, dtype=np.float64)))
    if len(c_above) != len(z_if):
        raise ValueError("need len(c_above) == len(z_if)")
    sp = {"L": float(c_l), "T": float(c_t)}
    xb, zb, xf, zf, mask = _layers_profile_args(z_if, xb, zb, xf, zf)
    return _view_legs_profile(
        legs, lambda m: travel_time_layers(z_if, c_above + [sp[m]], xe, ze, xf, zf, device=device),
        lambda m: travel_time_layers(z_if, c_above + [sp[m]], xe, ze, xb, zb, device=device),
        lambda down, m: _skip_profile(down, xb, zb, sp[m], xf, zf, mask, False, device))


def view_legs_surface_profile(x0, dx, zs, c1, c_l, c_t, xb, zb, xe, ze, xf, zf, *, legs=LEGS, device=0):
    """view_legs_surface under a backwall of any sampled shape (xb, zb) -> {leg: tt [n_e, n_f]}.  Direct legs: travel_time_surface;
    skip legs: skip_travel_time_surface_profile's, the down table made once per down mode.  Measure the front (measure_surface),
    the back (backwall_profile on the L-L image), then image the views through both."""
    legs = _legs_wanted(legs)
    sp = {"L": float(c_l), "T": float(c_t)}
    xb, zb, xf, zf, mask = _surface_profile_args(x0, dx, zs, xb, zb, xf, zf)
    return _view_legs_profile(
        legs, lambda m: travel_time_surface(x0, dx, zs, c1, sp[m], xe, ze, xf, zf, device=device),
        lambda m: travel_time_surface(x0, dx, zs, c1, sp[m], xe, ze, xb, zb, device=device),
        lambda down, m: _skip_profile(down, xb, zb, sp[m], xf, zf, mask, False, device))


def backwall_profile(image, x0, dx, z_lo, dz, *, z_min=None, threshold=0.1):
    """The backwall's depth profile read off an envelope image on the host.  ``image`` [n_x, n_z]: column x0 + k dx, depth
    z_lo + j dz — measure_surface's ``image`` layout, e.g. the L-L envelope TFM of the part.  In every column the brightest pixel
    at a depth >= ``z_min`` (default: the whole column; the first of equals) is refined by the three-point parabola on the
    amplitudes a, b, c about it, delta = 0.5 (a - c) / ((a - b) + (c - b)) (0 where the three are equal), depth
    z_lo + (j + delta) dz; NaN when the brightest pixel is the first allowed or the last one (the peak is not inside the window).
    Then surface_profile's rules: valid where the depth is finite and the amplitude at least ``threshold`` times the largest,
    trimmed to the first through last valid column, interior invalid columns filled by linear interpolation in x; ValueError when
    fewer than 4 columns remain.  -> dict(x0, dx, zs, valid [n_x], z_peak [n_x], amplitude [n_x]): xb = x0 + arange(len(zs)) dx and
    zb = zs feed skip_travel_time_layers_profile, view_legs_layers_profile and their surface twins."""
    img = np.asarray(image, dtype=np.float64)
    if img.ndim != 2 or img.shape[0] < 1:
        raise ValueError("image must be [n_x, n_z]")
    if not (np.isfinite(dz) and dz > 0 and np.isfinite(z_lo) and np.isfinite(x0) and np.isfinite(dx) and dx > 0):
        raise ValueError("need finite x0, z_lo and dx, dz > 0")
    n_z = img.shape[1]
    j_min = 0 if z_min is None else max(int(np.ceil((float(z_min) - float(z_lo)) / float(dz) - 1e-9)), 0)
    if n_z - j_min < 3:
        raise ValueError("the depth window at or below z_min must hold at least 3 pixels")
    j = j_min + np.argmax(np.where(np.isnan(img[:, j_min:]), -np.inf, img[:, j_min:]), axis=1)
    inside = (j > j_min) & (j < n_z - 1)
    jc = np.clip(j, 1, n_z - 2)
    k = np.arange(img.shape[0])
    a, b, c = img[k, jc - 1], img[k, jc], img[k, jc + 1]
    with np.errstate(all="ignore"):
        den = (a - b) + (c - b)
        delta = np.where(den != 0, 0.5 * (a - c) / den, 0.0)
    z_peak = np.where(inside, float(z_lo) + (jc + delta) * float(dz), np.nan)
    amp = img[k, j]
    r = surface_profile(x0, dx, z_peak, amp, threshold)
    r.update(z_peak=z_peak, amplitude=amp)
    return r


# ---------------------------------------------------------------------------------------------- the forward model: FMC simulator
SIM_ANALYTIC = 0x1          # RTUS_SIM_ANALYTIC (include/rtus.h)
SIM_ACCUMULATE = 0x2        # RTUS_SIM_ACCUMULATE
SIM_MAX_TABLE = 2048        # n_p + oversample (rtus_fmc_sim's limit)


def gaussian_pulse(f0, cycles, fs, oversample=8, *, analytic=True):
    """A Gaussian tone burst as simulate_fmc's wavelet table -> (pulse complex64 [n_p], centre): exp(-u^2 / (2 sigma^2))
    exp(2 pi i f0 u) with sigma = cycles / f0 / 2.355, sampled at u = (k - centre) / (fs oversample) for |u| <= 6 sigma (the dropped
    tail is below 1.6e-8 of the peak, under half an fp32 ulp).  ``analytic=False``: the imaginary part is zero (an RF pulse,
    exp(.) cos(2 pi f0 u))."""
    f0, cycles, fs = float(f0), float(cycles), float(fs)
    if not (f0 > 0 and cycles > 0 and fs > 0 and np.isfinite(f0 * cycles * fs)):
        raise ValueError("f0, cycles and fs must be finite and positive")
    if int(oversample) != oversample or oversample < 1:
        raise ValueError("oversample must be an integer >= 1")
    sig = cycles / f0 / 2.355
    step = 1.0 / (fs * int(oversample))
    half = int(np.floor(6.0 * sig / step))
    u = np.arange(-half, half + 1, dtype=np.float64) * step
    p = np.exp(-0.5 * (u / sig) ** 2) * np.exp(2j * np.pi * f0 * u)
    if not analytic:
        p = p.real + 0j
    return p.astype(np.complex64), half


def _sim_common(n_tx, n_rx, fs, n_t, pulse, centre, oversample, analytic, accumulate, out):
    """the checks and buffers the three simulate_* calls share -> (pulse, out, flags)"""
    if pulse is None or centre is None or oversample is None:
        raise ValueError("pulse, centre and oversample are needed (gaussian_pulse makes them)")
    pulse = np.ascontiguousarray(pulse, dtype=np.complex64)
    if pulse.ndim != 1 or pulse.size < 1:
        raise ValueError("pulse must be a 1-D complex64 table")
    if int(oversample) != oversample or oversample < 1:
        raise ValueError("oversample must be an integer >= 1")
    if int(centre) != centre or not 0 <= centre < pulse.size:
        raise ValueError("centre must be an index into pulse")
    if pulse.size + int(oversample) > SIM_MAX_TABLE:
        raise ValueError(f"len(pulse) + oversample must not exceed {SIM_MAX_TABLE}")
    if int(n_t) != n_t or n_t < 1:
        raise ValueError("n_t must be a positive integer")
    if not (np.isfinite(fs) and fs > 0):
        raise ValueError("fs must be finite and positive")
    shape = (n_tx, n_rx, int(n_t))
    dtype = np.complex64 if analytic else np.float32
    if accumulate and out is None:
        raise ValueError("accumulate=True needs the FMC to add onto in ``out``")
    return pulse, _out(out, shape, dtype), (SIM_ANALYTIC if analytic else 0) | (SIM_ACCUMULATE if accumulate else 0)


def _sim_factor(w, shape, name):
    if w is None:
        return None
    w = np.ascontiguousarray(w, dtype=np.complex64)
    if w.shape != shape:
        raise ValueError(f"{name} must be complex64 of shape {shape}")
    return w


def simulate_fmc(tt_tx, tt_rx=None, *, fs, n_t, pulse, centre, oversample, t0=0.0, strength=None, w_tx=None, w_rx=None,
                 analytic=False, accumulate=False, out=None, device=0):
    """The forward model of tfm_weighted: point scatterers to an FMC.  Scatterer s arrives in A-scan (tx, rx) at
    tt_tx[tx, s] + tt_rx[rx, s] with the complex amplitude strength[s] w_tx[tx, s] w_rx[rx, s] and adds amplitude x
    pulse(t - arrival) to the samples t = t0 + j / fs.  ``tt_tx`` [n_tx, n_s] / ``tt_rx`` [n_rx, n_s] float64: any travel-time
    table of this library over the scatterers as focal points (tt_rx defaults to tt_tx, and then w_rx to w_tx); ``strength``: a
    scalar or [n_s]; ``w_tx`` / ``w_rx``: complex64 leg amplitudes (None: 1).  ``pulse``, ``centre``, ``oversample``: the wavelet
    table (gaussian_pulse), sampled at fs oversample with time zero at index centre, interpolated linearly.  A NaN time or a
    non-finite factor drops that arrival only.  -> float32 [n_tx, n_rx, n_t] (the real part) or, with ``analytic=True``,
    complex64.  ``accumulate=True`` adds onto ``out`` (bit-identical to one call over all scatterers when the chunks are added in
    order).  Definition and the accumulation contract: include/rtus.h (rtus_fmc_sim).  Not in the reference."""
    tt_tx = np.ascontiguousarray(tt_tx, dtype=np.float64)
    if tt_rx is None:
        tt_rx = tt_tx
        w_rx = w_tx if w_rx is None else w_rx
    tt_rx = np.ascontiguousarray(tt_rx, dtype=np.float64)
    if tt_tx.ndim != 2 or tt_rx.ndim != 2 or tt_tx.shape[1] != tt_rx.shape[1] or tt_tx.size == 0 or tt_rx.size == 0:
        raise ValueError("tt_tx / tt_rx must be [n_tx, n_s] / [n_rx, n_s]")
    n_tx, n_rx, n_s = tt_tx.shape[0], tt_rx.shape[0], tt_tx.shape[1]
    q = None
    if strength is not None:
        q = np.ascontiguousarray(np.broadcast_to(np.asarray(strength, dtype=np.complex64), (n_s,)) if np.ndim(strength) == 0
                                 else strength, dtype=np.complex64)
        if q.shape != (n_s,):
            raise ValueError(f"strength must be a scalar or hold one value per scatterer ({n_s})")
    w_tx, w_rx = _sim_factor(w_tx, (n_tx, n_s), "w_tx"), _sim_factor(w_rx, (n_rx, n_s), "w_rx")
    pulse, out, flags = _sim_common(n_tx, n_rx, fs, n_t, pulse, centre, oversample, analytic, accumulate, out)
    st = _lib.lib().rtus_fmc_sim(_ptr(tt_tx), _ptr(tt_rx), n_tx, n_rx, n_s, _ptr(q), _ptr(w_tx), _ptr(w_rx), _ptr(pulse), pulse.size,
                                 int(centre), int(oversample), float(fs), float(t0), int(n_t), _ptr(out), flags, int(device))
    _lib.check(st, "rtus_fmc_sim")
    return out


def simulate_echoes(t_pair, amp=None, *, fs, n_t, pulse, centre, oversample, t0=0.0, analytic=False, accumulate=False, out=None,
                    device=0):
    """Echoes given per pair to an FMC: arrival k of pair (tx, rx) at ``t_pair[tx, rx, k]`` (float64 [n_tx, n_rx] or
    [n_tx, n_rx, n_a]; e.g. solve_travel_times' outer-surface echo) with the complex amplitude ``amp`` (same shape; None: 1).
    Wavelet, output, ``accumulate`` and the rules for NaN times: simulate_fmc's.  Definition: include/rtus.h (rtus_fmc_sim_echo)."""
    t_pair = np.ascontiguousarray(t_pair, dtype=np.float64)
    if t_pair.ndim == 2:
        t_pair = t_pair[:, :, None]
    if t_pair.ndim != 3 or t_pair.size == 0:
        raise ValueError("t_pair must be [n_tx, n_rx] or [n_tx, n_rx, n_a]")
    if amp is not None:
        amp = np.ascontiguousarray(amp, dtype=np.complex64)
        amp = _sim_factor(amp[:, :, None] if amp.ndim == 2 else amp, t_pair.shape, "amp")
    n_tx, n_rx, n_a = t_pair.shape
    pulse, out, flags = _sim_common(n_tx, n_rx, fs, n_t, pulse, centre, oversample, analytic, accumulate, out)
    st = _lib.lib().rtus_fmc_sim_echo(_ptr(t_pair), _ptr(amp), n_tx, n_rx, n_a, _ptr(pulse), pulse.size, int(centre), int(oversample),
                                      float(fs), float(t0), int(n_t), _ptr(out), flags, int(device))
    _lib.check(st, "rtus_fmc_sim_echo")
    return out


def simulate_views(legs, views=VIEWS, *, amplitudes=None, reciprocal=True, fs, n_t, pulse, centre, oversample, t0=0.0, strength=None,
                   analytic=False, accumulate=False, out=None, device=0):
    """The FMC of point scatterers seen through several views — the model tfm_views inverts.  ``legs``: {leg: tt [n_e, n_s]} over the
    scatterers (view_legs_*); a view "A-B" is simulated with tt_tx = legs[A], tt_rx = legs[reverse_leg(B)] and, with ``amplitudes``
    ({leg: (down, up)}, view_amplitudes_*), w_tx = amplitudes[A][0], w_rx = amplitudes[reverse_leg(B)][1] — not conjugated: this is
    the model, not its matched filter.  ``reciprocal=True``: a view with A != B also adds "B-A" (real data holds both).  The views
    are accumulated in the order given ("A-B" before its "B-A"), each one simulate_fmc call with accumulate=True after the first:
    the result is that chain's, bit for bit.  An unknown view or a leg missing from ``legs`` (or ``amplitudes``) raises ValueError
    before any GPU call."""
    views = (views,) if isinstance(views, str) else tuple(views)
    if not views:
        raise ValueError("at least one view is needed")
    chain = []
    for v in views:
        a, b = view_tables(v)
        chain.append((a, b))
        if reciprocal and a != reverse_leg(b):
            chain.append(view_tables("-".join(v.split("-")[::-1])))
    missing = sorted({g for p in chain for g in p if g not in legs})
    if missing:
        raise ValueError(f"legs {missing} are needed by the views and missing from ``legs``")
    if amplitudes is not None:
        missing = sorted({g for p in chain for g in p if g not in amplitudes})
        if missing:
            raise ValueError(f"legs {missing} are needed by the views and missing from ``amplitudes``")
    for i, (a, b) in enumerate(chain):
        w_tx = None if amplitudes is None else amplitudes[a][0]
        w_rx = None if amplitudes is None else amplitudes[b][1]
        out = simulate_fmc(legs[a], legs[b], fs=fs, n_t=n_t, pulse=pulse, centre=centre, oversample=oversample, t0=t0,
                           strength=strength, w_tx=w_tx, w_rx=w_rx, analytic=analytic, accumulate=accumulate or i > 0, out=out,
                           device=device)
    return out

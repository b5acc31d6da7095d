"""Throughput of the bore-reflected skip-leg table (rtus_tt_pipe_skip_dev) at scripts/pipe_throughput.py's production shape: the
reference aperture (64 x 0.6 mm behind the lens), r_outer 37 mm, pipe_offset 3.8 mm, bore 29 mm, a wall grid of 128 radii x 256
angles over +-30 deg, on torch tensors with a preallocated workspace, for the four legs LL, LT, TL and TT (c_l 5600, c_t 3230).
Prints one JSON line per leg (ms per table from CUDA-event timing); run under `rocprofv3 --kernel-trace --stats` for the set-up
and table kernels' own times."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from importlib import import_module  # noqa: E402

import rtus  # noqa: E402

dev = import_module("ray-tracing-ultrasound_amd.device")

ap = argparse.ArgumentParser()
ap.add_argument("--radii", type=int, default=128)
ap.add_argument("--angles", type=int, default=256)
ap.add_argument("--r-outer", type=float, default=0.037)
ap.add_argument("--r-inner", type=float, default=0.029)
ap.add_argument("--offset", type=float, default=0.0038)
ap.add_argument("--c-l", type=float, default=5600.0)
ap.add_argument("--c-t", type=float, default=3230.0)
ap.add_argument("--legs", default="LL,LT,TL,TT")
ap.add_argument("--reps", type=int, default=20)
a = ap.parse_args()
p = rtus.Params(r_outer=a.r_outer, pipe_offset=a.offset)
xe = (np.arange(64) - 31.5) * 0.6e-3
ze = np.full(64, p.d)
xf, zf = rtus.pipe_wall_grid(a.r_inner + 3e-5, a.r_outer - 3e-5, a.radii, a.angles, -np.pi / 6, np.pi / 6, params=p)
t = lambda v: torch.as_tensor(np.ascontiguousarray(v), dtype=torch.float64, device="cuda")      # noqa: E731
dxe, dze, dxf, dzf = t(xe), t(ze), t(xf), t(zf)
out = torch.empty((64, xf.size), dtype=torch.float64, device="cuda")
n_scan = int(np.ceil(a.r_outer * np.pi / rtus.api.PIPE_SCAN_ARC)) + 1
ws = torch.empty(int(rtus.lib().rtus_tt_pipe_skip_workspace_bytes(64, n_scan)), dtype=torch.uint8, device="cuda")
sp = {"L": a.c_l, "T": a.c_t}
for leg in a.legs.split(","):
    kw = dict(c_down=sp[leg[0]], c_up=sp[leg[1]], r_inner=a.r_inner, params=p, n_scan=n_scan, ws=ws)
    for _ in range(3):
        dev.tt_pipe_skip_dev(dxe, dze, dxf, dzf, out=out, **kw)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.reps):
        dev.tt_pipe_skip_dev(dxe, dze, dxf, dzf, out=out, **kw)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / a.reps
    n = 64 * xf.size
    print(json.dumps({"case": "tt_pipe_skip_" + leg, "n_e": 64, "n_f": int(xf.size), "n_scan": n_scan, "ms_per_table": round(ms, 4),
                      "solves_per_s": round(n / (ms * 1e-3), 1), "scan_steps_per_s": round(n * n_scan / (ms * 1e-3), 1),
                      "finite": float(np.isfinite(out.cpu().numpy()).mean())}), flush=True)

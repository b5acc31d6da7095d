"""Throughput of the skip-leg table kernel (rtus_tt_surface_skip_dev): scripts/surface_throughput.py's case (128 elements x 256^2
focal points under a 256-sample profile) with a backwall at 70 mm, on torch tensors, one line per mode pair.  Prints ms per
table from CUDA-event timing; run under `rocprofv3 --kernel-trace --stats` for kernel times."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from importlib import import_module  # noqa: E402

dev = import_module("ray-tracing-ultrasound_amd.device")

SPEEDS = {"L": 5900.0, "T": 3230.0}
ap = argparse.ArgumentParser()
ap.add_argument("--elements", type=int, default=128)
ap.add_argument("--grid", type=int, default=256)
ap.add_argument("--samples", type=int, default=256)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--modes", nargs="+", default=["LL", "LT", "TL", "TT"], choices=["LL", "LT", "TL", "TT"])
ap.add_argument("--z-back", type=float, default=0.07)
a = ap.parse_args()
f64 = dict(dtype=torch.float64, device="cuda")
x0, dx = -0.032, 0.064 / (a.samples - 1)
xs = x0 + dx * torch.arange(a.samples, **f64)
zs = 0.02 + 0.0015 * torch.sin(2 * torch.pi * xs / 0.010)
xe = torch.linspace(-0.0192, 0.0192, a.elements, **f64)
ze = torch.zeros(a.elements, **f64)
gx, gz = torch.meshgrid(torch.linspace(-0.03, 0.03, a.grid, **f64), torch.linspace(0.025, 0.065, a.grid, **f64), indexing="xy")
xf, zf = gx.reshape(-1).contiguous(), gz.reshape(-1).contiguous()
out = torch.empty((a.elements, xf.numel()), **f64)
for mode in a.modes:
    cd, cu = SPEEDS[mode[0]], SPEEDS[mode[1]]
    run = lambda: dev.tt_surface_skip_dev(x0, dx, zs, 1480.0, cd, cu, a.z_back, xe, ze, xf, zf, out=out)     # noqa: E731
    run()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(a.reps):
        run()
    t1.record()
    torch.cuda.synchronize()
    ms = t0.elapsed_time(t1) / a.reps
    solves = a.elements * xf.numel()
    m = 4 * (a.samples - 1) + 1
    print(json.dumps(dict(mode=mode, ms_per_call=ms, solves_per_s=solves / ms * 1e3, scan_points=m,
                          solve_points_per_s=solves * m / ms * 1e3, finite=float(torch.isfinite(out).double().mean()))))

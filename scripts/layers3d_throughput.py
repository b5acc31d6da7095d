"""Throughput of the matrix-array travel-time kernel (rtus_tt_layers3_dev) next to the planar kernel's default tier
(rtus_tt_layers_ex_dev, flags = 0) at equal n_e and n_f on the same stack, in the same run: 16 x 16 elements x 64 x 64 x 32 points and
32 x 32 x 64^3, two interfaces.  The planar kernel gets a linear array of n_e elements over the matrix array's width and the volume's
points with y dropped.  CUDA events around `--reps` launches after a warm-up, the two kernels alternating over `--rounds` rounds; one
JSON line per case: median (min-max) us per launch, solves/s, the ratio, and the 8 B/solve store stream as a fraction of the 6.0 TB/s
that plain coalesced 8-byte stores reach on this part (DESIGN.md section 4 "Store stream")."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from importlib import import_module  # noqa: E402

dev = import_module("ray-tracing-ultrasound_amd.device")
api = import_module("ray-tracing-ultrasound_amd.api")

STORE_STREAM = 6.0e12
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--cases", type=str, nargs="+", default=["16,64,64,32", "32,64,64,64"], help="n_side,n_x,n_y,n_z")
a = ap.parse_args()
t64 = lambda v: torch.as_tensor(np.ascontiguousarray(v, dtype=np.float64), device="cuda")
Z_IF, C = [0.010, 0.025], [1480.0, 3200.0, 5900.0]


def timed(run, reps):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        run()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps * 1e3


for case in a.cases:
    side, nx, ny, nz = (int(v) for v in case.split(","))
    xe, ye, ze = api.matrix_array(side, side, 0.6e-3)
    xf, yf, zf, shape = api.volume_grid(np.linspace(-0.02, 0.02, nx), np.linspace(-0.02, 0.02, ny), np.linspace(0.012, 0.05, nz))
    n_e, n_f = xe.size, xf.size
    x_lin = np.linspace(xe.min(), xe.max(), n_e)
    d3 = [t64(v) for v in (xe, ye, ze, xf, yf, zf)]
    d2 = [t64(v) for v in (x_lin, ze, xf, zf)]
    out = torch.empty((n_e, n_f), dtype=torch.float64, device="cuda")
    run3 = lambda: dev.tt_layers3_dev(Z_IF, C, *d3, out=out)      # noqa: E731
    run2 = lambda: dev.tt_layers_dev(Z_IF, C, *d2, out=out)       # noqa: E731
    for run in (run3, run2):                                        # warm-up: code objects, the allocator
        for _ in range(3):
            run()
    torch.cuda.synchronize()
    us3, us2 = [], []
    for _ in range(a.rounds):
        us3.append(timed(run3, a.reps))
        us2.append(timed(run2, a.reps))
    run3()
    finite = float(torch.isfinite(out).double().mean())
    m3, m2 = statistics.median(us3), statistics.median(us2)
    solves = n_e * n_f
    print(json.dumps(dict(kernel="tt_layers3", elements=n_e, points=n_f, shape=list(shape), interfaces=len(Z_IF), reps=a.reps, rounds=a.rounds,
                          us_3d=round(m3, 2), us_3d_range=[round(min(us3), 2), round(max(us3), 2)],
                          us_2d=round(m2, 2), us_2d_range=[round(min(us2), 2), round(max(us2), 2)],
                          solves_per_s_3d=solves / m3 * 1e6, solves_per_s_2d=solves / m2 * 1e6, ratio_3d_over_2d=m3 / m2,
                          store_tb_per_s_3d=8 * solves / m3 * 1e-6, store_stream_fraction_3d=8 * solves / m3 * 1e6 / STORE_STREAM,
                          store_stream_fraction_2d=8 * solves / m2 * 1e6 / STORE_STREAM, finite=finite)), flush=True)

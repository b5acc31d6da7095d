"""Throughput of the pipe-wall ray amplitude kernel (rtus_leg_amp_pipe_dev) next to the time kernel of the same leg
(rtus_tt_pipe_dev / rtus_tt_pipe_skip_dev) at the production shape: the reference aperture (64 elements), r_outer 37 mm, offset
3.8 mm, bore 29 mm, 128 radii x 256 angles over +-30 deg; every leg in both directions on the legs' own paths.  One JSON line per
case, ms per call from CUDA-event timing with preallocated outputs.  For a kernel trace run it under
rocprofv3 --kernel-trace --stats -- python scripts/pipe_amplitude_throughput.py --reps 5."""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from importlib import import_module  # noqa: E402

dev = import_module("ray-tracing-ultrasound_amd.device")
api = import_module("ray-tracing-ultrasound_amd.api")
lib = import_module("ray-tracing-ultrasound_amd._lib")

SPEEDS = {"L": 5600.0, "T": 3230.0}
MEDIA = dict(c_l=5600.0, c_t=3230.0, rho_wall=7850.0, rho_water=1000.0, rho_lens=2700.0, ct_lens=3100.0)
ap = argparse.ArgumentParser()
ap.add_argument("--radii", type=int, default=128)
ap.add_argument("--angles", type=int, default=256)
ap.add_argument("--reps", type=int, default=20)
a = ap.parse_args()
f64 = dict(dtype=torch.float64, device="cuda")


def timed(run, reps):
    run()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        run()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


p = api.Params(r_outer=0.037, pipe_offset=0.0038)
ri = 0.029
xf, zf = api.pipe_wall_grid(ri + 3e-5, 0.037 - 3e-5, a.radii, a.angles, -math.pi / 6, math.pi / 6, params=p)
xe = (torch.arange(64, **f64) - 31.5) * 0.6e-3
ze = torch.full((64,), float(p.d), **f64)
xf, zf = torch.as_tensor(xf, **f64), torch.as_tensor(zf, **f64)
n = 64 * xf.numel()
tt = torch.empty((64, xf.numel()), **f64)
al, be, ga = torch.empty_like(tt), torch.empty_like(tt), torch.empty_like(tt)
amp = torch.empty((64, xf.numel(), 2), dtype=torch.float32, device="cuda")
n_scan = max(int(math.ceil(0.037 * math.pi / api.PIPE_SCAN_ARC)) + 1, 4)
ws = torch.empty(int(lib.lib().rtus_tt_pipe_skip_workspace_bytes(64, n_scan)), dtype=torch.uint8, device="cuda")
for leg in ("L", "T", "LL", "LT", "TL", "TT"):
    if len(leg) == 1:
        run_tt = lambda: dev.tt_pipe_dev(xe, ze, xf, zf, out=tt, alpha_out=al, beta_out=be, c3=SPEEDS[leg], r_inner=ri, params=p,  # noqa: E731
                                         ws=ws)
    else:
        run_tt = lambda: dev.tt_pipe_skip_dev(xe, ze, xf, zf, out=tt, alpha_out=al, beta_out=be, gamma_out=ga, c_down=SPEEDS[leg[0]],  # noqa: E731
                                              c_up=SPEEDS[leg[1]], r_inner=ri, params=p, ws=ws)
    t_tt = timed(run_tt, a.reps)
    for up in (False, True):
        run = lambda: dev.leg_amp_pipe_dev(leg, xe, ze, xf, zf, al, be, ga if len(leg) == 2 else None, r_inner=ri, params=p, up=up,  # noqa: E731
                                           element_width=0.5e-3, f_c=5e6, out=amp, **MEDIA)
        ms = timed(run, a.reps)
        print(json.dumps(dict(kernel="leg_amp_pipe", leg=leg, up=up, elements=64, points=xf.numel(), ms_per_call=ms, time_kernel_ms=t_tt,
                              share_of_time_kernel=ms / t_tt, entries_per_s=n / ms * 1e3,
                              gb_per_s=(32 if len(leg) == 2 else 24) * n / ms / 1e6,
                              finite=float(torch.isfinite(amp).all(-1).double().mean()))))

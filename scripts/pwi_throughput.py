"""Throughput of the plane-wave imaging kernels on torch tensors: rtus_pw_layers (31 angles x 1024^2 focal points), rtus_pw_surface
(31 angles x 256^2 under a 256-sample profile), rtus_fmc_synth_tx (31 laws x 64 x 64 x 2048) and the PWI delay-and-sum through
rtus_tfm (31 x 64 pairs, 256^2) next to the 64 x 64 TFM.  CUDA-event timing; run under `rocprofv3 --kernel-trace --stats` for
kernel times."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from importlib import import_module  # noqa: E402

dev = import_module("ray-tracing-ultrasound_amd.device")
api = import_module("ray-tracing-ultrasound_amd.api")

ap = argparse.ArgumentParser()
ap.add_argument("--angles", type=int, default=31)
ap.add_argument("--reps", type=int, default=20)
a = ap.parse_args()
f64 = dict(dtype=torch.float64, device="cuda")
C1, C2, FS = 1480.0, 5900.0, 50e6
n_e, n_t = 64, 2048
xe = (np.arange(n_e) - (n_e - 1) / 2) * 0.6e-3
ang = torch.as_tensor(np.deg2rad(np.linspace(-15, 15, a.angles)), **f64)


def grid(n):
    gx, gz = torch.meshgrid(torch.linspace(-0.03, 0.03, n, **f64), torch.linspace(0.025, 0.065, n, **f64), indexing="xy")
    return gx.reshape(-1).contiguous(), gz.reshape(-1).contiguous()


def timed(fn):
    fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(a.reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / a.reps


res = {}
xf, zf = grid(1024)
out = torch.empty((a.angles, xf.numel()), **f64)
ms = timed(lambda: dev.pw_layers_dev([0.02], [C1, C2], ang, xe.min(), xe.max(), 0.0, xf, zf, out=out))
res["pw_layers_1024sq_ms"] = ms
res["pw_layers_write_TBps"] = out.numel() * 8 / ms / 1e9

xf, zf = grid(256)
x0, dx = -0.032, 0.064 / 255
zs = 0.02 + 0.0015 * torch.sin(2 * torch.pi * (x0 + dx * torch.arange(256, **f64)) / 0.010)
outs = torch.empty((a.angles, xf.numel()), **f64)
ms = timed(lambda: dev.pw_surface_dev(x0, dx, zs, C1, C2, ang, xe.min(), xe.max(), 0.0, xf, zf, out=outs))
res["pw_surface_256sq_ms"] = ms
res["pw_surface_solve_points_per_s"] = outs.numel() * (4 * 255 + 1) / ms * 1e3
res["pw_surface_finite"] = float(torch.isfinite(outs).double().mean())

fmc = torch.randn((n_e, n_e, n_t), dtype=torch.float32, device="cuda")
d = torch.as_tensor(api.pw_delays(xe, np.zeros(n_e), ang.cpu().numpy(), C1), **f64)
pw = torch.empty((a.angles, n_e, n_t), dtype=torch.float32, device="cuda")
ms = timed(lambda: dev.fmc_synth_tx_dev(fmc, FS, d, out=pw))
res["fmc_synth_tx_us"] = ms * 1e3
res["fmc_synth_tx_L2_read_TBps"] = a.angles * n_e * n_e * n_t * 4 / ms / 1e9

tt_pw = dev.pw_layers_dev([0.02], [C1, C2], ang, xe.min(), xe.max(), 0.0, xf, zf)
tt_rx = dev.tt_layers_dev([0.02], [C1, C2], torch.as_tensor(xe, **f64), torch.zeros(n_e, **f64), xf, zf)
img = torch.empty(xf.numel(), dtype=torch.float32, device="cuda")
res["pwi_tfm_256sq_us"] = timed(lambda: dev.tfm_dev(pw, FS, tt_pw, tt_rx, out=img)) * 1e3
fmc_b = torch.randn((n_e, n_e, n_t), dtype=torch.float32, device="cuda")
res["tfm_64x64_256sq_us"] = timed(lambda: dev.tfm_dev(fmc_b, FS, tt_rx, tt_rx, out=img)) * 1e3
print(json.dumps(res))

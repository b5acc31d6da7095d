"""Throughput of the adaptive-TFM kernels on torch tensors: the analytic FMC (rtus_fmc_analytic_dev) and the couplant envelope
image + column peak (rtus_surface_find_dev) at 64 elements x 2048 samples, 256 columns x 256 depths; rtus_tfm_dev over the same
256^2 pixels and FMC for comparison.  Prints gathers/s from CUDA-event timing; run under `rocprofv3 --kernel-trace --stats` for
kernel times."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from importlib import import_module  # noqa: E402

dev = import_module("ray-tracing-ultrasound_amd.device")

ap = argparse.ArgumentParser()
ap.add_argument("--elements", type=int, default=64)
ap.add_argument("--samples", type=int, default=2048)
ap.add_argument("--columns", type=int, default=256)
ap.add_argument("--depths", type=int, default=256)
ap.add_argument("--reps", type=int, default=20)
a = ap.parse_args()
n_e, n_t, n_s, n_z = a.elements, a.samples, a.columns, a.depths
fs, c1 = 50e6, 1480.0
g = torch.Generator(device="cuda").manual_seed(1)
fmc = torch.randn((n_e, n_e, n_t), generator=g, dtype=torch.float32, device="cuda")
xe = ((torch.arange(n_e, dtype=torch.float64, device="cuda") - (n_e - 1) / 2) * 0.25e-3).contiguous()
ze = torch.zeros(n_e, dtype=torch.float64, device="cuda")
x0, dx, z_lo, dz = -0.008, 0.016 / (n_s - 1), 0.004, 0.016 / (n_z - 1)    # the record holds 30 mm of water: all inside
an = dev.fmc_analytic_dev(fmc)
zp, amp = dev.surface_find_dev(an, fs, xe, ze, c1, x0, dx, n_s, z_lo, dz, n_z)
# the same pixels for rtus_tfm_dev: a straight-ray table
px = (x0 + dx * torch.arange(n_s, dtype=torch.float64, device="cuda"))[:, None].expand(n_s, n_z).reshape(-1)
pz = (z_lo + dz * torch.arange(n_z, dtype=torch.float64, device="cuda"))[None, :].expand(n_s, n_z).reshape(-1)
tt = (torch.hypot(xe[:, None] - px[None, :], ze[:, None] - pz[None, :]) / c1).contiguous()
img = dev.tfm_dev(fmc, fs, tt)
torch.cuda.synchronize()


def timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(a.reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / a.reps


ms_an = timed(lambda: dev.fmc_analytic_dev(fmc, out=an))
ms_sf = timed(lambda: dev.surface_find_dev(an, fs, xe, ze, c1, x0, dx, n_s, z_lo, dz, n_z, z_peak=zp, amp=amp))
ms_tfm = timed(lambda: dev.tfm_dev(fmc, fs, tt, out=img))
gathers = n_e * n_e * n_s * n_z
print(json.dumps(dict(elements=n_e, samples=n_t, columns=n_s, depths=n_z, ms_analytic=ms_an, ms_surface_find=ms_sf, ms_tfm=ms_tfm,
                      surface_find_gathers_per_s=gathers / ms_sf * 1e3, tfm_gathers_per_s=gathers / ms_tfm * 1e3,
                      analytic_share=ms_an / (ms_an + ms_sf), finite_peaks=int(torch.isfinite(zp).sum()))))

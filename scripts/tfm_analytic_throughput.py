"""Throughput of the envelope TFM (rtus_tfm_analytic_dev) on torch tensors, with and without the coherence factor, in the same run
as rtus_tfm_dev (8-byte real gathers) and rtus_surface_find_dev (16-byte complex gathers, straight rays): 64 elements x 2048
samples, 256^2 and 1024^2 pixels.  Also two rtus_tfm_dev calls over the split real / imaginary planes (the workaround: the same
complex sum, no cf), with and without the de-interleave.  Prints one JSON line per image size from CUDA-event timing; run under
`rocprofv3 --kernel-trace --stats` for kernel times."""
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
ap.add_argument("--sizes", type=int, nargs="+", default=[256, 1024])
ap.add_argument("--reps", type=int, default=20)
a = ap.parse_args()
n_e, n_t = a.elements, a.samples
fs, c1 = 50e6, 1480.0
g = torch.Generator(device="cuda").manual_seed(1)
fmc = torch.randn((n_e, n_e, n_t), generator=g, dtype=torch.float32, device="cuda")
xe = ((torch.arange(n_e, dtype=torch.float64, device="cuda") - (n_e - 1) / 2) * 0.25e-3).contiguous()
ze = torch.zeros(n_e, dtype=torch.float64, device="cuda")
an = dev.fmc_analytic_dev(fmc)
re, im = an[..., 0].contiguous(), an[..., 1].contiguous()


def timed(fn):
    fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(a.reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / a.reps * 1e3                              # us


for n in a.sizes:
    n_s = n_z = n
    x0, dx, z_lo, dz = -0.008, 0.016 / (n_s - 1), 0.004, 0.016 / (n_z - 1)    # the record holds 30 mm of water: all inside
    px = (x0 + dx * torch.arange(n_s, dtype=torch.float64, device="cuda"))[:, None].expand(n_s, n_z).reshape(-1)
    pz = (z_lo + dz * torch.arange(n_z, dtype=torch.float64, device="cuda"))[None, :].expand(n_s, n_z).reshape(-1)
    tt = (torch.hypot(xe[:, None] - px[None, :], ze[:, None] - pz[None, :]) / c1).contiguous()     # straight-ray table
    n_f = n_s * n_z
    img = torch.empty(n_f, dtype=torch.float32, device="cuda")
    img2 = torch.empty(n_f, dtype=torch.float32, device="cuda")
    out = torch.empty((n_f, 2), dtype=torch.float32, device="cuda")
    cf = torch.empty(n_f, dtype=torch.float32, device="cuda")
    zp = torch.empty(n_s, dtype=torch.float64, device="cuda")
    amp = torch.empty(n_s, dtype=torch.float32, device="cuda")

    def split():
        re.copy_(an[..., 0]); im.copy_(an[..., 1])
        dev.tfm_dev(re, fs, tt, out=img); dev.tfm_dev(im, fs, tt, out=img2)
    us = dict(
        tfm=timed(lambda: dev.tfm_dev(fmc, fs, tt, out=img)),
        surface_find=timed(lambda: dev.surface_find_dev(an, fs, xe, ze, c1, x0, dx, n_s, z_lo, dz, n_z, z_peak=zp, amp=amp)),
        tfm_analytic=timed(lambda: dev.tfm_analytic_dev(an, fs, tt, out=out)),
        tfm_analytic_cf=timed(lambda: dev.tfm_analytic_dev(an, fs, tt, out=out, cf=cf)),
        two_tfm_split_planes=timed(lambda: (dev.tfm_dev(re, fs, tt, out=img), dev.tfm_dev(im, fs, tt, out=img2))),
        two_tfm_with_deinterleave=timed(split))
    # the same sum: the analytic image's planes are the two rtus_tfm images, bit for bit
    dev.tfm_analytic_dev(an, fs, tt, out=out, cf=cf)
    dev.tfm_dev(re, fs, tt, out=img); dev.tfm_dev(im, fs, tt, out=img2)
    torch.cuda.synchronize()
    same = bool(torch.equal(out[:, 0], img) and torch.equal(out[:, 1], img2))
    gathers = n_e * n_e * n_f
    print(json.dumps(dict(elements=n_e, samples=n_t, pixels=f"{n_s}x{n_z}", reps=a.reps, us={k: round(v, 1) for k, v in us.items()},
                          gathers_per_s={k: float(f"{gathers / us[k] * 1e6:.3g}") for k in ("tfm", "surface_find", "tfm_analytic",
                                                                                              "tfm_analytic_cf")},
                          cf_overhead=round(us["tfm_analytic_cf"] / us["tfm_analytic"] - 1, 4),
                          vs_two_tfm_split_planes=round(us["tfm_analytic_cf"] / us["two_tfm_split_planes"], 3),
                          planes_bit_identical=same, cf_median=float(cf.median()))), flush=True)
    del tt, px, pz

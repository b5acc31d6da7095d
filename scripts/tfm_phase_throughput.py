"""Throughput of phase-coherence TFM (rtus_tfm_phase_dev) on torch tensors next to rtus_tfm_analytic_dev (with and without its
coherence factor) in the same run, at the same shapes: 64 elements x 2048 samples, 256^2 and 1024^2 pixels, with every set of
optional outputs — the image alone, vcf, scf, counts, vcf + scf, all three.  The variants are timed in turn, `--rounds` times
over (a difference is read against the spread between rounds); prints one JSON line per image size from CUDA-event timing: the
median over the rounds in us, the spread, and each variant's ratio to rtus_tfm_analytic_dev (no cf) of the same run."""
import argparse
import json
import os
import statistics
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
ap.add_argument("--rounds", type=int, default=5)
a = ap.parse_args()
n_e, n_t = a.elements, a.samples
fs, c1 = 50e6, 1480.0
g = torch.Generator(device="cuda").manual_seed(1)
fmc = torch.randn((n_e, n_e, n_t), generator=g, dtype=torch.float32, device="cuda")
xe = ((torch.arange(n_e, dtype=torch.float64, device="cuda") - (n_e - 1) / 2) * 0.25e-3).contiguous()
ze = torch.zeros(n_e, dtype=torch.float64, device="cuda")
an = dev.fmc_analytic_dev(fmc)


def timed(fn):
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
    out = torch.empty((n_f, 2), dtype=torch.float32, device="cuda")
    ref = torch.empty((n_f, 2), dtype=torch.float32, device="cuda")
    cf, vcf, scf = (torch.empty(n_f, dtype=torch.float32, device="cuda") for _ in range(3))
    cnt = torch.empty((n_f, 2), dtype=torch.int32, device="cuda")
    variants = dict(
        tfm_analytic=lambda: dev.tfm_analytic_dev(an, fs, tt, out=ref),
        tfm_analytic_cf=lambda: dev.tfm_analytic_dev(an, fs, tt, out=ref, cf=cf),
        phase_image_only=lambda: dev.tfm_phase_dev(an, fs, tt, out=out),
        phase_vcf=lambda: dev.tfm_phase_dev(an, fs, tt, out=out, vcf=vcf),
        phase_scf=lambda: dev.tfm_phase_dev(an, fs, tt, out=out, scf=scf),
        phase_counts=lambda: dev.tfm_phase_dev(an, fs, tt, out=out, counts=cnt),
        phase_vcf_scf=lambda: dev.tfm_phase_dev(an, fs, tt, out=out, vcf=vcf, scf=scf),
        phase_all=lambda: dev.tfm_phase_dev(an, fs, tt, out=out, vcf=vcf, scf=scf, counts=cnt))
    for fn in variants.values():                                             # every code object loaded, every shape warm
        fn()
    runs = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, fn in variants.items():
            runs[k].append(timed(fn))
    us = {k: statistics.median(v) for k, v in runs.items()}
    torch.cuda.synchronize()
    same = bool(torch.equal(out, ref))                                       # the same image, bit for bit
    gathers = n_e * n_e * n_f
    print(json.dumps(dict(elements=n_e, samples=n_t, pixels=f"{n_s}x{n_z}", reps=a.reps, rounds=a.rounds,
                          us={k: round(v, 1) for k, v in us.items()},
                          spread_us={k: [round(min(v), 1), round(max(v), 1)] for k, v in runs.items()},
                          ratio_to_tfm_analytic={k: round(us[k] / us["tfm_analytic"], 3) for k in us},
                          gathers_per_s={k: float(f"{gathers / us[k] * 1e6:.3g}") for k in us},
                          image_bit_identical=same, vcf_median=float(vcf.median()), scf_median=float(scf.median()))), flush=True)
    del tt, px, pz

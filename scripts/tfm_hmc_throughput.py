"""Throughput of TFM over a half-matrix capture (rtus_tfm_hmc_dev, rtus_tfm_analytic_hmc_dev) on torch tensors next to the
full-matrix kernels (rtus_tfm_dev, rtus_tfm_analytic_dev) on the unpacked block in the same run, at the same shapes: 64 elements x
2048 samples, 256^2 and 1024^2 pixels.  Variants: the full-matrix twins (the yardstick), and the one-table and the two-table
half-matrix forms (the second table is a copy of the first), real and analytic, with and without cf.  The variants are timed in
turn, `--rounds` times over (a difference is read against the spread between rounds); prints one JSON line per image size from
CUDA-event timing: the median over the rounds in us, the spread, each half-matrix variant's ratio to its full-matrix twin, whether
the one-table form's slowest round is below the twin's fastest, and the largest difference to the twin's image."""
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
iu = torch.triu_indices(n_e, n_e, device="cuda")                             # the packed order
hmc = torch.randn((iu.shape[1], n_t), generator=g, dtype=torch.float32, device="cuda")
fmc = torch.empty((n_e, n_e, n_t), dtype=torch.float32, device="cuda")       # the symmetric full matrix
fmc[iu[0], iu[1]] = hmc
fmc[iu[1], iu[0]] = hmc
xe = ((torch.arange(n_e, dtype=torch.float64, device="cuda") - (n_e - 1) / 2) * 0.25e-3).contiguous()
ze = torch.zeros(n_e, dtype=torch.float64, device="cuda")
an = dev.fmc_analytic_dev(fmc)
han = dev.fmc_analytic_dev(hmc[None])[0]                                     # [n_pairs, n_t, 2]: the same records' analytic signals


def timed(fn):
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(a.reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / a.reps * 1e3                              # us


TWIN = dict(hmc_one="tfm", hmc_two="tfm", hmc_analytic_one="tfm_analytic", hmc_analytic_two="tfm_analytic",
            hmc_analytic_cf_one="tfm_analytic_cf", hmc_analytic_cf_two="tfm_analytic_cf")

for n in a.sizes:
    n_s = n_z = n
    x0, dx, z_lo, dz = -0.008, 0.016 / (n_s - 1), 0.004, 0.016 / (n_z - 1)    # the record holds 30 mm of water: all inside
    px = (x0 + dx * torch.arange(n_s, dtype=torch.float64, device="cuda"))[:, None].expand(n_s, n_z).reshape(-1)
    pz = (z_lo + dz * torch.arange(n_z, dtype=torch.float64, device="cuda"))[None, :].expand(n_s, n_z).reshape(-1)
    tt = (torch.hypot(xe[:, None] - px[None, :], ze[:, None] - pz[None, :]) / c1).contiguous()     # straight-ray table
    tt2 = tt.clone()                                                         # another pointer: the two-table form
    n_f = n_s * n_z
    img = {k: torch.empty(n_f, dtype=torch.float32, device="cuda") for k in ("tfm", "hmc_one", "hmc_two")}
    cpx = {k: torch.empty((n_f, 2), dtype=torch.float32, device="cuda") for k in ("tfm_analytic", "hmc_analytic_one", "hmc_analytic_two")}
    cf, hcf = (torch.empty(n_f, dtype=torch.float32, device="cuda") for _ in range(2))
    variants = dict(
        tfm=lambda: dev.tfm_dev(fmc, fs, tt, out=img["tfm"]),
        tfm_analytic=lambda: dev.tfm_analytic_dev(an, fs, tt, out=cpx["tfm_analytic"]),
        tfm_analytic_cf=lambda: dev.tfm_analytic_dev(an, fs, tt, out=cpx["tfm_analytic"], cf=cf),
        hmc_one=lambda: dev.tfm_hmc_dev(hmc, fs, tt, out=img["hmc_one"]),
        hmc_two=lambda: dev.tfm_hmc_dev(hmc, fs, tt, tt2, out=img["hmc_two"]),
        hmc_analytic_one=lambda: dev.tfm_analytic_hmc_dev(han, fs, tt, out=cpx["hmc_analytic_one"]),
        hmc_analytic_two=lambda: dev.tfm_analytic_hmc_dev(han, fs, tt, tt2, out=cpx["hmc_analytic_two"]),
        hmc_analytic_cf_one=lambda: dev.tfm_analytic_hmc_dev(han, fs, tt, out=cpx["hmc_analytic_one"], cf=hcf),
        hmc_analytic_cf_two=lambda: dev.tfm_analytic_hmc_dev(han, fs, tt, tt2, out=cpx["hmc_analytic_two"], cf=hcf))
    for fn in variants.values():                                             # every code object loaded, every shape warm
        fn()
    runs = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, fn in variants.items():
            runs[k].append(timed(fn))
    us = {k: statistics.median(v) for k, v in runs.items()}
    torch.cuda.synchronize()
    one_is_two = bool(torch.equal(img["hmc_one"], img["hmc_two"]) and torch.equal(cpx["hmc_analytic_one"], cpx["hmc_analytic_two"]))
    rel = lambda x, y: float((x - y).abs().max() / y.abs().max())
    print(json.dumps(dict(elements=n_e, samples=n_t, pixels=f"{n_s}x{n_z}", reps=a.reps, rounds=a.rounds,
                          us={k: round(v, 1) for k, v in us.items()},
                          spread_us={k: [round(min(v), 1), round(max(v), 1)] for k, v in runs.items()},
                          ratio_to_full_matrix_twin={k: round(us[k] / us[t], 3) for k, t in TWIN.items()},
                          slowest_round_below_twins_fastest={k: bool(max(runs[k]) < min(runs[t])) for k, t in TWIN.items()},
                          one_table_bits_equal_two_table=one_is_two,
                          max_diff_to_full_matrix_of_image_max=dict(real=rel(img["hmc_one"], img["tfm"]),
                                                                    analytic=rel(cpx["hmc_analytic_one"], cpx["tfm_analytic"])))), flush=True)
    del tt, tt2, px, pz

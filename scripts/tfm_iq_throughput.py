"""Throughput of the carrier-aware envelope TFM (rtus_tfm_iq_dev, rtus_tfm_iq_hmc_dev) next to the linear kernels it extends
(rtus_tfm_analytic_dev, rtus_tfm_analytic_hmc_dev) in the same run, at the same shape: 64 x 64 x 2048 samples, 256^2 focal points
(--sizes for others).  Variants: full matrix, half matrix with one table and with two (the second a copy of the first), each with
and without cf, linear and carrier-aware (f_demod = fs / 4).  The variants are timed in turn after a warm-up, `--rounds` times over
(a difference is read against the spread between rounds); prints one JSON line per image size from CUDA-event timing: the minimum
and the median over the rounds in us, the spread, each carrier-aware variant's ratio to its linear twin (of the minima), and whether
f_demod = 0 gives the twin's bits."""
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
ap.add_argument("--sizes", type=int, nargs="+", default=[256])
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--rounds", type=int, default=5)
a = ap.parse_args()
n_e, n_t = a.elements, a.samples
fs, c1 = 50e6, 1480.0
f_demod = fs / 4
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


for n in a.sizes:
    n_s = n_z = n
    x0, dx, z_lo, dz = -0.008, 0.016 / (n_s - 1), 0.004, 0.016 / (n_z - 1)    # the record holds 30 mm of water: all inside
    px = (x0 + dx * torch.arange(n_s, dtype=torch.float64, device="cuda"))[:, None].expand(n_s, n_z).reshape(-1)
    pz = (z_lo + dz * torch.arange(n_z, dtype=torch.float64, device="cuda"))[None, :].expand(n_s, n_z).reshape(-1)
    tt = (torch.hypot(xe[:, None] - px[None, :], ze[:, None] - pz[None, :]) / c1).contiguous()     # straight-ray table
    tt2 = tt.clone()                                                         # another pointer: the two-table form
    n_f = n_s * n_z
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device="cuda")
    lin, iq, cf = new(n_f, 2), new(n_f, 2), new(n_f)
    full = lambda f, **k: (lambda: dev.tfm_analytic_dev(an, fs, tt, out=lin, **k)) if f is None else \
        (lambda: dev.tfm_iq_dev(an, fs, f, tt, out=iq, **k))
    half = lambda f, second, **k: (lambda: dev.tfm_analytic_hmc_dev(han, fs, tt, second, out=lin, **k)) if f is None else \
        (lambda: dev.tfm_iq_hmc_dev(han, fs, f, tt, second, out=iq, **k))
    variants = {}
    for tag, f in (("analytic", None), ("iq", f_demod)):
        variants[f"tfm_{tag}"] = full(f)
        variants[f"tfm_{tag}_cf"] = full(f, cf=cf)
        variants[f"hmc_{tag}_one"] = half(f, None)
        variants[f"hmc_{tag}_cf_one"] = half(f, None, cf=cf)
        variants[f"hmc_{tag}_two"] = half(f, tt2)
        variants[f"hmc_{tag}_cf_two"] = half(f, tt2, cf=cf)
    for fn in variants.values():                                             # every code object loaded, every shape warm
        fn()
    runs = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, fn in variants.items():
            runs[k].append(timed(fn))
    best = {k: min(v) for k, v in runs.items()}
    # f_demod = 0: the linear kernels' bits
    same = []
    for f0, ref in ((full(0.0), full(None)), (half(0.0, None), half(None, None)), (half(0.0, tt2), half(None, tt2))):
        f0(); ref()
        torch.cuda.synchronize()
        same.append(bool(torch.equal(iq, lin)))
    print(json.dumps(dict(elements=n_e, samples=n_t, pixels=f"{n_s}x{n_z}", reps=a.reps, rounds=a.rounds, f_demod_over_fs=f_demod / fs,
                          min_us={k: round(v, 1) for k, v in best.items()},
                          median_us={k: round(statistics.median(v), 1) for k, v in runs.items()},
                          spread_us={k: [round(min(v), 1), round(max(v), 1)] for k, v in runs.items()},
                          ratio_iq_to_linear={k: round(best[k] / best[k.replace("_iq", "_analytic")], 3) for k in best if "_iq" in k},
                          f_demod_zero_bits_equal_linear=same)), flush=True)
    del tt, tt2, px, pz

"""Throughput of phase-coherence and weighted TFM over a half-matrix capture (rtus_tfm_phase_hmc_dev, rtus_tfm_weighted_hmc_dev) on
torch tensors next to their full-matrix twins on the unpacked capture (rtus_tfm_phase_dev, rtus_tfm_weighted_dev) and next to
rtus_tfm_analytic_hmc_dev, all in the same run at the same shapes: 64 elements x 2048 samples, 256^2 and 1024^2 pixels, one delay
table and two, every set of outputs of the phase entry (image alone, + vcf, + scf, all) and the weighted entry with and without
sens, with one weight table and two.  The variants are timed in turn, `--rounds` times over (a difference is read against the
spread between rounds); prints one JSON line per image size and table count from CUDA-event timing: the median over the rounds in
us, the spread, each half-matrix variant's ratio to its full-matrix twin and to rtus_tfm_analytic_hmc_dev of the same run."""
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
fs, c1, c2 = 50e6, 1480.0, 1540.0
g = torch.Generator(device="cuda").manual_seed(1)
iu = torch.triu_indices(n_e, n_e, device="cuda")
hmc = torch.randn((iu.shape[1], n_t), generator=g, dtype=torch.float32, device="cuda")
an_h = dev.fmc_analytic_dev(hmc[None])[0].contiguous()                       # [n_pairs, n_t, 2]: the Hilbert filter works per A-scan
an_f = torch.empty((n_e, n_e, n_t, 2), dtype=torch.float32, device="cuda")   # the unpacked capture: record (i, j) at [i][j] and [j][i]
an_f[iu[0], iu[1]] = an_h
an_f[iu[1], iu[0]] = an_h
xe = ((torch.arange(n_e, dtype=torch.float64, device="cuda") - (n_e - 1) / 2) * 0.25e-3).contiguous()
ze = torch.zeros(n_e, dtype=torch.float64, device="cuda")


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
    d = torch.hypot(xe[:, None] - px[None, :], ze[:, None] - pz[None, :])
    tt_a, tt_b = (d / c1).contiguous(), (d / c2).contiguous()                 # straight-ray tables; the second one 4 % faster
    n_f = n_s * n_z
    w_a = torch.randn((n_e, n_f, 2), generator=g, dtype=torch.float32, device="cuda")
    w_b = torch.randn((n_e, n_f, 2), generator=g, dtype=torch.float32, device="cuda")
    out, ref = (torch.empty((n_f, 2), dtype=torch.float32, device="cuda") for _ in range(2))
    cf, vcf, scf, sens = (torch.empty(n_f, dtype=torch.float32, device="cuda") for _ in range(4))
    cnt, cnt_f = (torch.empty((n_f, 2), dtype=torch.int32, device="cuda") for _ in range(2))
    del d, px, pz
    for tables, tt_rx in (("one", None), ("two", tt_b)):
        # name -> (half-matrix call, its full-matrix twin on the unpacked capture or None)
        variants = dict(
            analytic_hmc=(lambda: dev.tfm_analytic_hmc_dev(an_h, fs, tt_a, tt_rx, out=ref), None),
            phase_image_only=(lambda: dev.tfm_phase_hmc_dev(an_h, fs, tt_a, tt_rx, out=out),
                              lambda: dev.tfm_phase_dev(an_f, fs, tt_a, tt_rx, out=ref)),
            phase_vcf=(lambda: dev.tfm_phase_hmc_dev(an_h, fs, tt_a, tt_rx, out=out, vcf=vcf),
                       lambda: dev.tfm_phase_dev(an_f, fs, tt_a, tt_rx, out=ref, vcf=cf)),
            phase_scf=(lambda: dev.tfm_phase_hmc_dev(an_h, fs, tt_a, tt_rx, out=out, scf=scf),
                       lambda: dev.tfm_phase_dev(an_f, fs, tt_a, tt_rx, out=ref, scf=cf)),
            phase_all=(lambda: dev.tfm_phase_hmc_dev(an_h, fs, tt_a, tt_rx, out=out, vcf=vcf, scf=scf, counts=cnt),
                       lambda: dev.tfm_phase_dev(an_f, fs, tt_a, tt_rx, out=ref, vcf=cf, scf=sens, counts=cnt_f)),
            weighted_w1=(lambda: dev.tfm_weighted_hmc_dev(an_h, fs, tt_a, w_a, tt_rx, w_a, out=out),
                         lambda: dev.tfm_weighted_dev(an_f, fs, tt_a, w_a, tt_rx, w_a, out=ref)),
            weighted_w1_sens=(lambda: dev.tfm_weighted_hmc_dev(an_h, fs, tt_a, w_a, tt_rx, w_a, out=out, sens=sens),
                              lambda: dev.tfm_weighted_dev(an_f, fs, tt_a, w_a, tt_rx, w_a, out=ref, sens=cf)),
            weighted_w2=(lambda: dev.tfm_weighted_hmc_dev(an_h, fs, tt_a, w_a, tt_rx, w_b, out=out),
                         lambda: dev.tfm_weighted_dev(an_f, fs, tt_a, w_a, tt_rx, w_b, out=ref)),
            weighted_w2_sens=(lambda: dev.tfm_weighted_hmc_dev(an_h, fs, tt_a, w_a, tt_rx, w_b, out=out, sens=sens),
                              lambda: dev.tfm_weighted_dev(an_f, fs, tt_a, w_a, tt_rx, w_b, out=ref, sens=cf)))
        for half, full in variants.values():                                 # every code object loaded, every shape warm
            half()
            if full:
                full()
        runs = {k: ([], []) for k in variants}
        for _ in range(a.rounds):
            for k, (half, full) in variants.items():
                runs[k][0].append(timed(half))
                if full:
                    runs[k][1].append(timed(full))
        us = {k: statistics.median(v[0]) for k, v in runs.items()}
        us_full = {k: statistics.median(v[1]) for k, v in runs.items() if v[1]}
        # checked in the run: counts and scf of the two forms are equal bit for bit; sens likewise (the last weighted variant)
        dev.tfm_phase_hmc_dev(an_h, fs, tt_a, tt_rx, out=out, scf=scf, counts=cnt)
        dev.tfm_phase_dev(an_f, fs, tt_a, tt_rx, out=ref, scf=cf, counts=cnt_f)
        torch.cuda.synchronize()
        same_counts = bool(torch.equal(cnt, cnt_f)) and bool(torch.equal(scf.view(torch.int32), cf.view(torch.int32)))
        dev.tfm_weighted_hmc_dev(an_h, fs, tt_a, w_a, tt_rx, w_b, out=out, sens=sens)
        dev.tfm_weighted_dev(an_f, fs, tt_a, w_a, tt_rx, w_b, out=ref, sens=cf)
        torch.cuda.synchronize()
        same_sens = bool(torch.equal(sens.view(torch.int32), cf.view(torch.int32)))
        rel = float((out - ref).abs().max() / ref.abs().max())
        print(json.dumps(dict(elements=n_e, samples=n_t, pixels=f"{n_s}x{n_z}", delay_tables=tables, reps=a.reps, rounds=a.rounds,
                              us={k: round(v, 1) for k, v in us.items()},
                              spread_us={k: [round(min(v[0]), 1), round(max(v[0]), 1)] for k, v in runs.items()},
                              full_matrix_us={k: round(v, 1) for k, v in us_full.items()},
                              full_matrix_spread_us={k: [round(min(v[1]), 1), round(max(v[1]), 1)] for k, v in runs.items() if v[1]},
                              ratio_to_full_matrix_twin={k: round(us[k] / us_full[k], 3) for k in us_full},
                              ratio_to_analytic_hmc={k: round(us[k] / us["analytic_hmc"], 3) for k in us},
                              counts_scf_bit_identical=same_counts, sens_bit_identical=same_sens,
                              weighted_max_diff_over_max=rel)), flush=True)
    del tt_a, tt_b, w_a, w_b

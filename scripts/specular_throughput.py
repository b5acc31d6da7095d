"""Throughput of the specular-echo kernel on torch tensors (CUDA-event timing): rtus_specular_dev at a production shape — 128 x 128
pairs, 1024 points per reflector, 33 candidate reflectors (one pass of fit_reflector at its defaults) — with one table both ways
and with two tables, all outputs and the times alone.  The time is recorded next to its two floors: the bytes (both tables read
once plus the outputs, at the HBM rate given) and the fp64-rate vector issue (the vector instructions per (pair, point) of the
kernel's unrolled loop, counted in the listing of the built source, at 4 cycles per wave-instruction and SIMD).  There is no parent
to compare with and no pass bar.  Prints one JSON line and writes profiles/specular_kernel.txt."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--elements", type=int, default=128)
ap.add_argument("--points", type=int, default=1024)
ap.add_argument("--reflectors", type=int, default=33)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--hbm-tb-s", type=float, default=8.0, help="HBM rate of the bytes floor [TB/s]")
ap.add_argument("--clock-ghz", type=float, default=2.4)
ap.add_argument("--simds", type=int, default=1024, help="256 CUs x 4 SIMDs")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "specular_kernel.txt"))
a = ap.parse_args()


def loop_instructions():
    """(vector instructions, LDS reads, scalar loads) per point in the unrolled loop of rtus_specular_kernel, and its unroll factor:
    the listing's innermost block that holds the 64-byte scalar load of the transmit row"""
    csrc = os.path.join(ROOT, "ray-tracing-ultrasound_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS\s*:=\s*(.*)$", mk, flags=re.M).group(1).replace("$(ARCH)", "gfx950").split()
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "rtus_specular.s")
        subprocess.run(["/opt/rocm/bin/hipcc"] + flags + ["--cuda-device-only", "-S", os.path.join(csrc, "rtus_specular.hip"), "-o", out],
                       check=True, capture_output=True, timeout=600)
        lines = [ln.strip() for ln in open(out)]
    blocks, cur = [], []
    for ln in lines:
        if ln.startswith(".LBB") or ln.startswith("; %bb."):
            blocks.append(cur)
            cur = []
        cur.append(ln)
    blocks.append(cur)
    body = next(b for b in blocks if any(ln.startswith("s_load_dwordx16") for ln in b))
    unroll = sum(ln.startswith("v_add_f64") for ln in body)
    valu = sum(ln.startswith("v_") for ln in body)
    lds = sum(ln.startswith("ds_read") for ln in body)
    return valu / unroll, lds / unroll, unroll


valu, lds, unroll = loop_instructions()

import numpy as np  # noqa: E402
import torch  # noqa: E402
from importlib import import_module  # noqa: E402

import rtus  # noqa: E402,F401

dev = import_module("ray-tracing-ultrasound_amd.device")
n_e, n_p, G = a.elements, a.points, a.reflectors


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


# tables of a backwall under the aperture: a smooth minimum per pair, as the model functions make them
xe = (np.arange(n_e) - (n_e - 1) / 2) * 0.6e-3
xs = np.linspace(-1.2 * abs(xe[0]) - 1e-3, 1.2 * abs(xe[0]) + 1e-3, n_p)
depth = np.linspace(0.018, 0.022, G)
tab = np.concatenate([np.hypot(xe[:, None] - xs[None, :], d) / 5900.0 for d in depth], axis=1)
ta = torch.from_numpy(tab).cuda()
tb = torch.from_numpy(tab * (5900.0 / 3230.0)).cuda()
out = torch.empty((G, n_e, n_e), dtype=torch.float64, device="cuda")
pos = torch.empty_like(out)
n_min = torch.empty((G, n_e, n_e), dtype=torch.int32, device="cuda")
dev.specular_dev(ta, n_refl=G, out=out)
torch.cuda.synchronize()
bracketed = float(torch.isfinite(out).double().mean())

ms = dict(one_table_t=timed(lambda: dev.specular_dev(ta, n_refl=G, out=out)),
          one_table_all=timed(lambda: dev.specular_dev(ta, n_refl=G, out=out, pos=pos, n_min=n_min)),
          two_tables_t=timed(lambda: dev.specular_dev(ta, tb, n_refl=G, out=out)),
          two_tables_all=timed(lambda: dev.specular_dev(ta, tb, n_refl=G, out=out, pos=pos, n_min=n_min)))
steps = G * n_e * n_e * n_p                                   # (pair, point) steps
table_bytes = G * n_p * n_e * 8
floor_bytes = {k: ((2 if "two" in k else 1) * table_bytes + G * n_e * n_e * (20 if "all" in k else 8)) / (a.hbm_tb_s * 1e12) * 1e3
               for k in ms}
floor_issue = steps / 64 * valu * 4 / (a.simds * a.clock_ghz * 1e9) * 1e3
res = dict(elements=n_e, points=n_p, reflectors=G, reps=a.reps, bracketed=bracketed, ms=ms, floor_bytes_ms=floor_bytes,
           floor_issue_ms=floor_issue, valu_per_point=valu, lds_reads_per_point=lds, unroll=unroll,
           pair_points_per_ns={k: steps / v * 1e-6 for k, v in ms.items()})
print(json.dumps(res))
with open(a.out, "w") as f:
    f.write(f"rtus_specular_dev, {n_e} x {n_e} pairs, {n_p} points, {G} reflectors ({steps:.3e} (pair, point) steps); CUDA events, "
            f"{a.reps} repetitions after a warm-up, preallocated outputs; {bracketed:.3f} of the pairs bracketed\n")
    f.write(f"unrolled loop of the listing: {valu:.2f} vector instructions and {lds:.2f} LDS reads per (pair, point), unroll {unroll}\n")
    f.write(f"floor, fp64-rate vector issue (4 cycles per wave-instruction, {a.simds} SIMDs at {a.clock_ghz} GHz): {floor_issue:.4f} ms\n")
    for k, v in ms.items():
        f.write(f"{k:16s} {v:.4f} ms   bytes floor at {a.hbm_tb_s} TB/s {floor_bytes[k]:.4f} ms   {v / floor_issue:.2f} x the issue floor\n")

"""Throughput of the skip-leg kernel off a sampled backwall on torch tensors (CUDA-event timing): rtus_skip_reflector_dev at a
production shape — 64 elements x 256^2 focal points x 321 reflector points (a backwall over 80 mm at a quarter of a millimetre) —
for the times alone and for all outputs, against the route that existed before it: the n_f x n_p table of up legs U built with torch
in fp64 (the header's operations, one elementwise kernel each) and rtus_specular_dev(tt_down, U).  That route is timed with and
without U's construction; the two routes alternate within every repetition of one run.  The fused call has to be no slower than
the existing route including U's construction: the script says which way it came out.  Next to the times stand the two floors: the
bytes (the down table and the points read once plus the outputs; for the existing route U written and read once as well, at the HBM
rate given) and the fp64-rate vector issue (the vector instructions per (element, focal point, reflector point) of the kernel's
unrolled loop plus the up leg's, formed once per 8 elements, counted in the listing of the built source, at 4 cycles per
wave-instruction and SIMD).  Prints one JSON line and writes profiles/skip_reflector_kernel.txt."""
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
ap.add_argument("--elements", type=int, default=64)
ap.add_argument("--side", type=int, default=256, help="the image is side x side focal points")
ap.add_argument("--points", type=int, default=321)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--hbm-tb-s", type=float, default=8.0, help="HBM rate of the bytes floor [TB/s]")
ap.add_argument("--clock-ghz", type=float, default=2.4)
ap.add_argument("--simds", type=int, default=1024, help="256 CUs x 4 SIMDs")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "skip_reflector_kernel.txt"))
a = ap.parse_args()
TE = 8                                                        # SKIP_TE: the elements that share one up leg


def loop_instructions():
    """per instance of rtus_skip_reflector_kernel (True: with n_min's bookkeeping) -> (vector instructions per step of the unrolled
    loop, its unroll factor, vector instructions of one up leg): the listing's innermost blocks that hold the LDS reads and the
    LDS write"""
    csrc = os.path.join(ROOT, "ray-tracing-ultrasound_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    flags = re.search(r"^CXXFLAGS\s*:=\s*(.*)$", mk, flags=re.M).group(1).replace("$(ARCH)", "gfx950").split()
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "rtus_skip_reflector.s")
        subprocess.run(["/opt/rocm/bin/hipcc"] + flags + ["--cuda-device-only", "-S", os.path.join(csrc, "rtus_skip_reflector.hip"), "-o", out],
                       check=True, capture_output=True, timeout=600)
        lines = [ln.strip() for ln in open(out)]
    res, count, blocks, cur = {}, None, [], []

    def close():
        if count is None:
            return
        body = max((b for b in blocks + [cur] if any(ln.startswith("ds_read") for ln in b)), key=len)
        fill = next(b for b in blocks + [cur] if any(ln.startswith("ds_write") for ln in b))
        unroll = sum(ln.startswith("v_add_f64") for ln in body)
        res[count] = (sum(ln.startswith("v_") for ln in body) / unroll, unroll, sum(ln.startswith("v_") for ln in fill))
    for ln in lines:
        m = re.match(r"_Z\d+rtus_skip_reflector_kernelILb([01])E\S*:", ln)
        if m or ln.startswith(".Lfunc_end"):
            close()
            count, blocks, cur = (m.group(1) == "1" if m else None), [], []
        elif ln.startswith(".LBB") or ln.startswith("; %bb."):
            blocks.append(cur)
            cur = []
        cur.append(ln)
    return res


listing = loop_instructions()

import numpy as np  # noqa: E402
import torch  # noqa: E402
from importlib import import_module  # noqa: E402

import rtus  # noqa: E402,F401

dev = import_module("ray-tracing-ultrasound_amd.device")
n_e, n_p, n_f = a.elements, a.points, a.side * a.side
C_L = 5900.0

# a tilted backwall at 30 mm under the aperture in one medium; the image between 6 and 26 mm, the span overhanging it
xe = (np.arange(n_e) - (n_e - 1) / 2) * 0.6e-3
xb = np.linspace(-0.040, 0.040, n_p)
zb = 0.030 + xb * np.tan(np.deg2rad(3.0))
gx, gz = (v.ravel() for v in np.meshgrid(np.linspace(-0.020, 0.020, a.side), np.linspace(0.006, 0.026, a.side)))
down = torch.from_numpy(np.hypot(xe[:, None] - xb[None, :], zb[None, :]) / C_L).cuda()
txb, tzb, txf, tzf = (torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in (xb, zb, gx, gz))
out = torch.empty((n_e, n_f), dtype=torch.float64, device="cuda")
out2 = torch.empty((1, n_e, n_f), dtype=torch.float64, device="cuda")
pos = torch.empty_like(out)
n_min = torch.empty((n_e, n_f), dtype=torch.int32, device="cuda")
U = torch.empty((n_f, n_p), dtype=torch.float64, device="cuda")
W = torch.empty_like(U)


def build_u():
    """the header's operations, each one elementwise kernel into preallocated tensors: dx, dz, their squares, the sum, root, / c"""
    torch.sub(txf[:, None], txb[None, :], out=U)
    torch.mul(U, U, out=U)
    torch.sub(tzf[:, None], tzb[None, :], out=W)
    torch.mul(W, W, out=W)
    torch.add(U, W, out=U)
    torch.sqrt(U, out=U)
    torch.div(U, C_L, out=U)


routes = dict(fused_t=lambda: dev.skip_reflector_dev(down, txb, tzb, C_L, txf, tzf, out=out),
              fused_all=lambda: dev.skip_reflector_dev(down, txb, tzb, C_L, txf, tzf, out=out, pos=pos, n_min=n_min),
              existing_with_u=lambda: (build_u(), dev.specular_dev(down, U, out=out2)),
              existing_without_u=lambda: dev.specular_dev(down, U, out=out2))
for fn in routes.values():                                    # warm-up; U is built before the route that takes it as given
    fn()
torch.cuda.synchronize()
# (torch's elementwise kernels are not held to the header's roundings — a division by a scalar may multiply by its reciprocal — so
# this U may differ from the header's in the last place; bit equality with U formed in NumPy is tests/test_gpu_skip_reflector.py's)
diff = float(torch.nan_to_num(out - out2[0]).abs().max())
bracketed = float(torch.isfinite(out).double().mean())
ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.reps)] for k in routes}
for r in range(a.reps):                                       # the routes alternate within every repetition
    for k, fn in routes.items():
        ev[k][r][0].record()
        fn()
        ev[k][r][1].record()
torch.cuda.synchronize()
ms = {k: float(np.mean([e0.elapsed_time(e1) for e0, e1 in v])) for k, v in ev.items()}
lo = {k: float(np.min([e0.elapsed_time(e1) for e0, e1 in v])) for k, v in ev.items()}

steps = n_e * n_f * n_p
io = (n_e * n_p + 2 * n_p + 2 * n_f) * 8
floor_bytes = dict(fused_t=io + n_e * n_f * 8, fused_all=io + n_e * n_f * 20,
                   existing_with_u=io + n_e * n_f * 8 + 2 * n_f * n_p * 8, existing_without_u=(n_e * n_p + n_f * n_p) * 8 + n_e * n_f * 8)
floor_bytes = {k: v / (a.hbm_tb_s * 1e12) * 1e3 for k, v in floor_bytes.items()}
per_step = {c: listing[c][0] + listing[c][2] / TE for c in listing}
floor_issue = {c: steps / 64 * per_step[c] * 4 / (a.simds * a.clock_ghz * 1e9) * 1e3 for c in listing}
verdict = "no slower than" if ms["fused_t"] <= ms["existing_with_u"] else "SLOWER than"
res = dict(elements=n_e, focal_points=n_f, points=n_p, reps=a.reps, bracketed=bracketed, max_diff_to_existing_route_s=diff, ms=ms, ms_min=lo,
           floor_bytes_ms=floor_bytes, floor_issue_ms={"t": floor_issue[False], "all": floor_issue[True]},
           valu_per_step={"t": per_step[False], "all": per_step[True]}, unroll=listing[True][1], valu_per_up_leg=listing[True][2],
           speedup_over_existing_with_u=ms["existing_with_u"] / ms["fused_t"], verdict=f"fused {verdict} the existing route with U")
print(json.dumps(res))
with open(a.out, "w") as f:
    f.write(f"rtus_skip_reflector_dev, {n_e} elements x {n_f} focal points x {n_p} reflector points ({steps:.3e} steps); CUDA events, "
            f"{a.reps} repetitions after a warm-up, the four routes alternating within each, preallocated outputs; {bracketed:.3f} of the "
            f"entries bracketed; max |tt - existing route's| {diff:.3e} s (torch's U is not held to the header's roundings)\n")
    f.write(f"listing: {listing[False][0]:.2f} (times alone) / {listing[True][0]:.2f} (with n_min) vector instructions per step in the loop "
            f"(unroll {listing[True][1]}), {listing[True][2]} per up leg shared by {TE} elements\n")
    f.write(f"floor, fp64-rate vector issue (4 cycles per wave-instruction, {a.simds} SIMDs at {a.clock_ghz} GHz): "
            f"{floor_issue[False]:.4f} ms times alone, {floor_issue[True]:.4f} ms all outputs\n")
    for k, v in ms.items():
        fl = floor_issue["all" in k] if k.startswith("fused") else None
        f.write(f"{k:20s} mean {v:.4f} ms  min {lo[k]:.4f} ms   bytes floor at {a.hbm_tb_s} TB/s {floor_bytes[k]:.4f} ms"
                + (f"   {v / fl:.2f} x the issue floor" if fl else "") + "\n")
    f.write(f"existing route: U ({n_f * n_p * 8 / 1e6:.0f} MB) built by seven torch elementwise kernels, then rtus_specular_dev\n")
    f.write(f"fused (times alone) is {verdict} the existing route including U's construction: {ms['existing_with_u'] / ms['fused_t']:.2f} x\n")

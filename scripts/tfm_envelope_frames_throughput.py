"""Throughput of envelope TFM over half-matrix frame stacks (rtus_tfm_envelope_frames_hmc_i16_dev) next to the per-frame loop on the
entries it replaces, in the same run: 64 elements (2080 records) x 2048 int16 samples, n_frames 8, 9 and 32, at 256^2 and 1024^2
focal points (six shapes), one table and two (an equal copy through another pointer).  Routes, times per frame:
  (L) per frame fmc_analytic_dev then tfm_analytic_hmc_dev, the frames already float32 on the device;
  (S) tfm_envelope_frames_hmc_i16_dev on its split-plane route — its pack, Hilbert and combine steps included — complex output, and
      (S_mag) magnitude output;
  (C) the same entry forced onto the complex route by asking for cf.
--host-twins adds, at 8 frames and one table, the wall time (H) of api.tfm_envelope_frames on the int16 stack from pageable memory
against the Python loop it replaces (per frame: widen to float32, hmc_analytic, tfm_analytic_hmc), with the bytes moved each way.

Each shape is one child process under its own time limit (the parent never touches the GPU and stops at the first child that fails).
In the child: CUDA events around each route, outputs and workspaces preallocated, two warm-ups of every route, then `--reps`
repetitions with the routes timed in turn WITHIN each repetition.  One JSON line per shape: medians and [5 %, 95 %] per frame in us,
the ratios of the medians to (L), and whether every route gave (L)'s bits.
    python scripts/tfm_envelope_frames_throughput.py --host-twins >> profiles/tfm_envelope_frames_hmc_kernel.txt     (twice)"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(8, 256), (9, 256), (32, 256), (8, 1024), (9, 1024), (32, 1024)]   # (n_frames, pixels per side)
ap = argparse.ArgumentParser()
ap.add_argument("--elements", type=int, default=64)
ap.add_argument("--samples", type=int, default=2048)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--limit", type=int, default=240, help="seconds a shape's child process may take")
ap.add_argument("--host-twins", action="store_true", help="also time the host twin against the Python loop route on the 8-frame shapes")
ap.add_argument("--shape", type=int, nargs=2, metavar=("N_FRAMES", "N"), help="(child) measure this one shape")
a = ap.parse_args()

if a.shape is None:
    for n_frames, n in SHAPES:
        cmd = [sys.executable, os.path.abspath(__file__), "--shape", str(n_frames), str(n), "--elements", str(a.elements),
               "--samples", str(a.samples), "--reps", str(a.reps)] + (["--host-twins"] if a.host_twins else [])
        try:
            r = subprocess.run(cmd, timeout=a.limit)
        except subprocess.TimeoutExpired:
            sys.exit(f"{n_frames} frames at {n}^2: not finished after {a.limit} s; nothing more is started")
        if r.returncode:
            sys.exit(f"{n_frames} frames at {n}^2: exit status {r.returncode}; nothing more is started")
    sys.exit(0)

sys.path.insert(0, ROOT)
import torch  # noqa: E402
from importlib import import_module  # noqa: E402

dev = import_module("ray-tracing-ultrasound_amd.device")
n_frames, n = a.shape
n_e, n_t = a.elements, a.samples
n_pairs, n_f = n_e * (n_e + 1) // 2, n * n
fs, c1 = 50e6, 1480.0
g = torch.Generator(device="cuda").manual_seed(1)
hmc_i16 = torch.randint(-32768, 32768, (n_frames, n_pairs, n_t), generator=g, dtype=torch.int16, device="cuda")
hmc_f32 = hmc_i16.to(torch.float32)
xe = ((torch.arange(n_e, dtype=torch.float64, device="cuda") - (n_e - 1) / 2) * 0.25e-3).contiguous()
ze = torch.zeros(n_e, dtype=torch.float64, device="cuda")
x0, dx, z_lo, dz = -0.008, 0.016 / (n - 1), 0.004, 0.016 / (n - 1)           # the record holds 30 mm of water: all inside
px = (x0 + dx * torch.arange(n, dtype=torch.float64, device="cuda"))[:, None].expand(n, n).reshape(-1)
pz = (z_lo + dz * torch.arange(n, dtype=torch.float64, device="cuda"))[None, :].expand(n, n).reshape(-1)
tt = (torch.hypot(xe[:, None] - px[None, :], ze[:, None] - pz[None, :]) / c1).contiguous()         # straight-ray table, one for both legs
new = lambda *shape: torch.empty(shape, dtype=torch.float32, device="cuda")   # noqa: E731


def pct(v, q):
    v = sorted(v)
    return v[min(len(v) - 1, max(0, round(q * (len(v) - 1))))]


def work(**kw):
    return torch.empty(dev.tfm_envelope_frames_hmc_workspace_bytes(n_frames, n_e, n_t, n_f, i16=True, **kw), dtype=torch.uint8, device="cuda")


an = new(1, n_pairs, n_t, 2)                                                 # (L)'s analytic frame, one at a time
w_s, w_c = work(), work(want_cf=True)
result = dict(lib=os.environ.get("RTUS_LIB", "in-tree"), elements=n_e, samples=n_t, n_frames=n_frames, pixels=f"{n}x{n}", reps=a.reps,
              workspace_MB=dict(split=round(w_s.numel() / 1e6, 1), complex=round(w_c.numel() / 1e6, 1)))
for tables, tr in (("one_table", None), ("two_tables", tt.clone())):
    out = {k: new(n_frames, n_f, 2) for k in ("L", "S", "C")}
    mag, cf = new(n_frames, n_f), new(n_frames, n_f)

    def loop():
        for k in range(n_frames):
            dev.fmc_analytic_dev(hmc_f32[k:k + 1], 63, out=an)
            dev.tfm_analytic_hmc_dev(an[0], fs, tt, tr, out=out["L"][k])
    routes = {"L_loop_of_fmc_analytic_dev_and_tfm_analytic_hmc_dev": loop,
              "S_envelope_frames_i16_dev_split_plane": lambda: dev.tfm_envelope_frames_hmc_i16_dev(hmc_i16, fs, tt, tr, out=out["S"], ws=w_s),
              "S_mag_envelope_frames_i16_dev_split_plane_magnitude": lambda: dev.tfm_envelope_frames_hmc_i16_dev(hmc_i16, fs, tt, tr, magnitude=True, out=mag, ws=w_s),
              "C_envelope_frames_i16_dev_complex_route_with_cf": lambda: dev.tfm_envelope_frames_hmc_i16_dev(hmc_i16, fs, tt, tr, out=out["C"], cf=cf, ws=w_c)}
    for _ in range(2):                                                       # code objects loaded, buffers touched
        for fn in routes.values():
            fn()
        torch.cuda.synchronize()
    runs = {k: [] for k in routes}
    for _ in range(a.reps):
        for k, fn in routes.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            t1.synchronize()
            runs[k].append(t0.elapsed_time(t1) * 1e3)                        # us
    med = {k: pct(v, 0.5) for k, v in runs.items()}
    L = med["L_loop_of_fmc_analytic_dev_and_tfm_analytic_hmc_dev"]
    result[tables] = dict(per_frame_us={k: round(v / n_frames, 1) for k, v in med.items()},
                          p05_p95_per_frame_us={k: [round(pct(v, 0.05) / n_frames, 1), round(pct(v, 0.95) / n_frames, 1)] for k, v in runs.items()},
                          ratio_to_L={k.split("_")[0] + ("_mag" if "_mag_" in k else ""): round(v / L, 3) for k, v in med.items() if not k.startswith("L_")},
                          bits_equal_the_loop=dict(S=bool(torch.equal(out["S"], out["L"])), C=bool(torch.equal(out["C"], out["L"])),
                                                   S_mag=bool(torch.equal(mag, torch.sqrt(out["L"][..., 0].double() ** 2 + out["L"][..., 1].double() ** 2).float()))))
if a.host_twins and n_frames == 8:
    import time
    import numpy as np
    rtus = import_module("ray-tracing-ultrasound_amd")
    h_i16, h_tt = hmc_i16.cpu().numpy(), tt.cpu().numpy()
    h_out = {k: np.empty((n_frames, n_f), dtype=np.complex64) for k in ("tfm_envelope_frames_int16", "python_loop_route")}
    h_mag = np.empty((n_frames, n_f), dtype=np.float32)

    def loop_route():
        for k in range(n_frames):
            rtus.tfm_analytic_hmc(rtus.hmc_analytic(h_i16[k].astype(np.float32), 63), fs, h_tt, out=h_out["python_loop_route"][k])
    calls = {"tfm_envelope_frames_int16": lambda: rtus.tfm_envelope_frames(h_i16, fs, h_tt, out=h_out["tfm_envelope_frames_int16"]),
             "tfm_envelope_frames_int16_magnitude": lambda: rtus.tfm_envelope_frames(h_i16, fs, h_tt, magnitude=True, out=h_mag),
             "python_loop_route": loop_route}
    wall = {k: [] for k in calls}
    for r in range(7):                                                       # (the first two: the arena grows, pages are touched)
        for k, fn in calls.items():
            t = time.perf_counter()
            fn()
            if r >= 2:
                wall[k].append((time.perf_counter() - t) * 1e3)
    s, tab, img = h_i16.size, h_tt.nbytes, n_frames * n_f
    result.update(host_twin_wall_ms={k: round(pct(v, 0.5), 2) for k, v in wall.items()},
                  host_twin_wall_ms_min_max={k: [round(min(v), 2), round(max(v), 2)] for k, v in wall.items()},
                  host_twin_bits_equal=bool(np.array_equal(h_out["tfm_envelope_frames_int16"], h_out["python_loop_route"])),
                  host_twin_MB_up_down={"tfm_envelope_frames_int16": [round((2 * s + tab) / 1e6, 1), round(8 * img / 1e6, 1)],
                                        "tfm_envelope_frames_int16_magnitude": [round((2 * s + tab) / 1e6, 1), round(4 * img / 1e6, 1)],
                                        "python_loop_route": [round((4 * s + 8 * s + n_frames * tab) / 1e6, 1), round((8 * s + 8 * img) / 1e6, 1)]})
print(json.dumps(result), flush=True)

"""Where a row-table workgroup's time goes, phase by phase (DESIGN.md section 4 "Start of a workgroup").

    scripts/build_variant.sh stampNew -DRTUS_EXP_STAMPS
    python scripts/stamps_planar.py variants/librtus_stampNew.so [another stamped library ...]

(The start-up as it was, stamped, for the comparison of profiles/rowtable_startup.txt: the kernel of
profiles/rowtable_startup_allparts.patch on the parent commit, built with -DRTUS_EXP_STAMPS -DRTUS_EXP_STARTUP_OFF=31.)

Builds with -DRTUS_EXP_STAMPS let one lane per workgroup record the device's constant-rate clock (100 MHz) at six points: entry,
after the records' barrier, after the node pass, after the check pass, at the first store, at the last store.  This script runs
ONE configs[2] launch (after a warm-up launch) on each library and prints, for the first round of workgroups (those that entered
before any workgroup of the launch had finished) and for the second, the median and the 10 % .. 90 % spread of every phase."""
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

TICK_US = 0.01
PHASES = ("entry -> records' barrier", "-> node pass done", "-> check pass done", "-> first store", "-> last store", "whole workgroup")


def stamps(path):
    L = C.CDLL(os.path.abspath(path), mode=C.RTLD_LOCAL)
    dp, ip, vp = C.c_void_p, C.c_int, C.c_void_p
    L.rtus_tt_layers_ex_dev.argtypes = [dp, dp, ip, dp, dp, ip, dp, dp, ip, dp, vp, C.c_uint, vp]
    L.rtus_tt_layers_ex_dev.restype = ip
    L.rtus_dbg_read_stamps.argtypes = [vp, ip]
    L.rtus_dbg_read_stamps.restype = ip
    dev = torch.device("cuda", 0)
    t64 = lambda a: torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=dev)
    W = bench.workload_inputs("cfg3_planar", 0, 1)
    z_if = np.ascontiguousarray(W["z_if"], dtype=np.float64); c = np.ascontiguousarray(W["c"], dtype=np.float64)
    xe, ze, xf, zf = t64(W["xe"]), t64(W["ze"]), t64(W["xf"]), t64(W["zf"])
    out = torch.empty((W["n_e"], W["n_f"]), dtype=torch.float64, device=dev)
    n_wg = -(-W["n_f"] // 256) * -(-W["n_e"] // 64)
    buf = np.zeros((n_wg, 8), dtype=np.uint64)
    for _ in range(2):                                        # the first launch warms up; reading clears the stamps
        st = L.rtus_tt_layers_ex_dev(z_if.ctypes.data, c.ctypes.data, z_if.size, xe.data_ptr(), ze.data_ptr(), W["n_e"], xf.data_ptr(),
                                     zf.data_ptr(), W["n_f"], out.data_ptr(), None, 1, torch.cuda.current_stream().cuda_stream)
        assert st == 0, st
        torch.cuda.synchronize()
        assert L.rtus_dbg_read_stamps(buf.ctypes.data, n_wg) == 0
    return buf[:, :6].astype(np.int64)


def report(name, s):
    served = (s > 0).all(axis=1)                              # a workgroup that took the solver leaves the table's stamps empty
    s = s[served]
    first = s[:, 0] < s[:, 5].min()
    print(f"{name}: {len(s)} served workgroups, launch {(s[:, 5].max() - s[:, 0].min()) * TICK_US:.1f} us from first entry to last store")
    for label, sel in (("first round", first), ("second round", ~first)):
        if not sel.any():
            continue
        r = s[sel]
        d = np.concatenate([np.diff(r, axis=1), (r[:, 5] - r[:, 0])[:, None]], axis=1) * TICK_US
        print(f"  {label}: {int(sel.sum())} workgroups")
        for k, ph in enumerate(PHASES):
            p10, p50, p90 = np.percentile(d[:, k], [10, 50, 90])
            print(f"    {ph:28s} median {p50:7.2f} us   10 % .. 90 %: {p10:7.2f} .. {p90:7.2f} us")


if __name__ == "__main__":
    for p in sys.argv[1:]:
        report(os.path.basename(p), stamps(p))

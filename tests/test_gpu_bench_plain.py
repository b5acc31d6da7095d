"""GPU: a plain `bench.py --gpus 1 --steps K --warmup W` is lean — it prints the headline line without the CPU baseline, the
accuracy check or the side measurements (those need --full), and spends at most 30 s outside its steps, start to exit."""
import json
import os
import subprocess
import sys
import time

import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def test_plain_run_is_the_headline_alone():
    steps, warmup = 20, 5
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup)]
    t0 = time.perf_counter()
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    wall = time.perf_counter() - t0
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["metric"].startswith("Mrays/sec") and d["unit"] == "Mrays/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f64" and d["config"]["workload"].startswith("BASELINE configs[2]")
    assert d["steps"] == steps and d["warmup"] == warmup and d["value"] > 0 and d["ms_per_step"] > 0
    assert d["roofline"]["avg_launch_ms"] > 0
    for key in ("cpu_baseline", "accuracy", "max_abs_dt_s", "extra"):
        assert key not in d, key
    outside = wall - (steps + warmup) * d["ms_per_step"] * 1e-3
    assert outside < 30.0, f"{outside:.1f} s outside the steps"

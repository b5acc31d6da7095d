"""GPU: bench.py --dump-outputs writes what the timed path computed in its last step — the whole table when it fits, a seeded
sample of it with its flat indices when it does not, under 64 MB in all — and those are the bits the NumPy API computes for
the same inputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _bench(out_dir, args):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--warmup", "1", "--no-extra", "--no-cpu-baseline",
           "--dump-outputs", str(out_dir)] + args
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def _table(wl, rtus):
    w = bench.planar_inputs(wl, 0, 1)
    return rtus.travel_time_layers(w["z_if"], w["c"], w["xe"], w["ze"], w["xf"], w["zf"], taup=True)


def test_dump_is_the_timed_steps_table(tmp_path, rtus):
    d = _bench(tmp_path, ["--workload", "cfg2_planar", "--steps", "3"])
    assert d["steps"] == 3 and d["ms_per_step"] > 0
    assert d["dump_outputs"]["arrays"]["tt"]["sampled"] is None and d["dump_outputs"]["what"] == "the whole table"
    assert sorted(os.listdir(tmp_path)) == ["tt.npy"]
    got = np.load(tmp_path / "tt.npy")
    ref = _table("cfg2_planar", rtus)
    assert got.dtype == np.float64 and got.shape == (ref.size,)
    assert np.array_equal(got, ref.ravel(), equal_nan=True), float(np.nanmax(np.abs(got - ref.ravel())))


def test_dump_of_the_headline_is_a_fixed_sample_under_64_mb(tmp_path, rtus):
    a, b = tmp_path / "a", tmp_path / "b"
    d = _bench(a, ["--steps", "2"])
    _bench(b, ["--steps", "5"])
    assert d["config"]["workload"].startswith("BASELINE configs[2]") and d["dump_outputs"]["arrays"]["tt"]["sampled"]
    assert sum(os.path.getsize(a / f) for f in os.listdir(a)) < 64 * 10 ** 6
    idx = np.load(a / "tt_sample_index.npy")
    assert idx.dtype == np.float64 and np.all(np.diff(idx) > 0)
    got = np.load(a / "tt.npy")
    assert np.array_equal(got, _table("cfg3_planar", rtus).ravel()[idx.astype(np.int64)], equal_nan=True)
    for f in ("tt.npy", "tt_sample_index.npy"):         # the same sample of the same table whatever the number of timed steps
        assert np.array_equal(np.load(a / f), np.load(b / f), equal_nan=True)

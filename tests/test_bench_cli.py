"""The bench's command line on one GPU at a small shard: a plain run prints the headline line alone
and, with --dump-outputs, writes the last timed step's hand-back — the same arrays on every run of
the same arguments; --full adds the other legs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGS = ["--gpus", "1", "--steps", "4", "--warmup", "2", "--nodes", "20000", "--report-every", "3"]
FULL_ONLY = ("roofline", "cpu_baseline", "cpu_baseline_soa", "pcie_inclusive", "patch_emit", "hbm_working_set")


def _run(extra):
    r = subprocess.run([sys.executable, "bench.py"] + ARGS + extra, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_run_dumps_the_same_outputs_every_run(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    line = _run(["--dump-outputs", str(a)])
    _run(["--dump-outputs", str(b)])
    assert line["steps"] == 4 and line["ms_per_step"] > 0 and line["value"] > 0
    assert all(line[k] is None for k in FULL_ONLY)
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b))
    assert names == ["aggregates.npy", "lengths.npy", "node_fired.npy", "pod_fired.npy", "pod_fired_segments.npy"]
    out = {n[:-4]: np.load(a / n) for n in names}
    for n in names:
        assert out[n[:-4]].dtype in (np.float32, np.float64)
        assert np.array_equal(out[n[:-4]], np.load(b / n)), n
    assert sum(os.path.getsize(a / n) for n in names) <= 64 * 10**6
    n_pod, n_seg, n_node = (int(x) for x in out["lengths"])
    assert (n_pod, n_seg, n_node) == (len(out["pod_fired"]), len(out["pod_fired_segments"]), len(out["node_fired"]))
    assert n_pod > 0 and out["pod_fired_segments"].sum() == n_pod
    # the packed node records: 27-bit slot | 5-bit stage, slots of this shard, each at most once per step
    slots = out["node_fired"].astype(np.uint64) & np.uint64((1 << 27) - 1)
    assert slots.max(initial=0) < 20000 and len(np.unique(slots)) == n_node
    agg = line["aggregates"]
    flat = list(agg["fired_per_stage"].values()) + list(agg["counts"].values()) + list(agg["usage"].values())
    assert sorted(out["aggregates"].tolist()) == sorted(float(x) for x in flat)


@pytest.mark.gpu
def test_full_run_adds_the_other_legs():
    line = _run(["--full", "--no-pmc", "--no-cpu-baseline", "--hbm-nodes", "0", "--pcie-steps", "2", "--emit-steps", "1"])
    assert line["roofline"]["bytes_per_launch"] > 0 and line["roofline"]["avg_launch_us"] > 0
    assert line["pcie_inclusive"]["n_host_equals_fired"] and line["patch_emit"]["steps"] == 1
    assert line["cpu_baseline"] is None and line["hbm_working_set"] is None

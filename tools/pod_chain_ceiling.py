"""The C5 step without a node stream: what the pod chain costs alone (the ceiling of any change that
only shortens or thins the node engine's chain).

    python tools/pod_chain_ceiling.py [--steps 50] [--warmup 10] [--reps 3] [--nodes 1000000]

One process, one pair of engines (bench.build_engines + configure_usage, bench.py's priorities and
fuse steps).  Per repetition two timed runs of `--steps` steps with a report every 10, alternating:
  pair  kwk_step_n_pair(pods, nodes) + the report over both engines   (bench.py's timed loop)
  pods  kwk_step_n(pods) + the report over the pod engine alone       (no node launches at all)
Prints one JSON line: us per step of every run and the ranges.  (No HIP events in either, so `pair`
reads ~0.9 us below bench.py's ms_per_step.)
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--report-every", type=int, default=10)
    args = ap.parse_args()
    from kwok_amd.host import abi
    from kwok_amd.host.cluster import DeviceReport, phase_masks

    seed, dt = 0x6B776F6B, 10**9
    pods, nodes, (pvars, pidx) = bench.build_engines(0, args.nodes, 100, 0, seed, 0.1)
    bench.configure_usage(pods, pvars, pidx, args.nodes, 100)
    pods.set_tuning(abi.TUNE_STREAM_PRIORITY, 1)
    nodes.set_tuning(abi.TUNE_STREAM_PRIORITY, 2)
    pods.set_tuning(abi.TUNE_FUSE_STEPS, 4)
    pm = phase_masks(pods.p, values=("Running", "Succeeded", "Failed"))
    nm = phase_masks(nodes.p, values=("Running",))
    pmask, pname = [0] + list(pm.values()), ["pods"] + [f"pods_{k}" for k in pm]
    nmask, nname = [0] + list(nm.values()), ["nodes"] + [f"nodes_{k}" for k in nm]
    rep_pair = DeviceReport([pods, nodes], [pmask, nmask], [pname, nname], usage_engine=pods, dist=None, device=None)
    rep_pods = DeviceReport([pods], [pmask], [pname], usage_engine=pods, dist=None, device=None)

    def run(mode, k0, n):
        k = k0
        while k < k0 + n:
            m = min(args.report_every, k0 + n - k)
            if mode == "pair":
                pods.step_n_pair(nodes, m, bench.NOW0 + k * dt, dt, seed, k, "packed16")
            else:
                pods.step_n(m, bench.NOW0 + k * dt, dt, seed, k, "packed16")
            k += m
            (rep_pair if mode == "pair" else rep_pods).collect(bench.NOW0 + (k - 1) * dt)
        pods.sync()
        nodes.sync()

    k = 0
    for mode in ("pair", "pods"):
        run(mode, k, args.warmup)
        k += args.warmup
    out = {"pair": [], "pods": []}
    for _ in range(args.reps):
        for mode in ("pair", "pods"):
            t0 = time.perf_counter()
            run(mode, k, args.steps)
            out[mode].append(round((time.perf_counter() - t0) / args.steps * 1e6, 2))
            k += args.steps
    print(json.dumps({"nodes": args.nodes, "steps": args.steps, "us_per_step": out,
                      "pair_range": [min(out["pair"]), max(out["pair"])],
                      "pods_range": [min(out["pods"]), max(out["pods"])]}), flush=True)
    pods.close()
    nodes.close()


if __name__ == "__main__":
    main()

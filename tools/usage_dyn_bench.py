"""kwk_usage with clock-dependent usage values (kwk_usage_config_dyn) against the constant path,
in one process on one engine: HIP-event times of kwk_usage alone for

  constant      every pod on interned constants (usage-from-annotation: usage_fast_kernel)
  no_dyn_pod    the same constants, one ramp program loaded that no pod uses (usage_kernel<WB, true>
                with the interpreter never entered: the cost of leaving the fast path)
  dyn_10pct     every 10th pod's memory on the ramp program
  dyn_all       every pod's memory on the ramp program

    python tools/usage_dyn_bench.py [--nodes 10000] [--pods-per-node 100] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

RAMP = 'Quantity("1Mi") * (pod.SinceSecond() / 60.0)'


def timed(eng, t, scrapes, warmup):
    out = []
    for r in range(warmup + scrapes):
        t[0] += 10**9
        eng.event_record(0)
        eng.usage(t[0])
        eng.event_record(1)
        eng.sync()
        if r >= warmup:
            out.append(eng.event_elapsed_ms(0, 1) * 1e3)
    return {"median_us": round(statistics.median(out), 2), "min_us": round(min(out), 2),
            "max_us": round(max(out), 2), "scrapes": scrapes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=10_000)
    ap.add_argument("--pods-per-node", type=int, default=100)
    ap.add_argument("--scrapes", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from kwok_amd.host import cel
    from kwok_amd.host.usage import OP_DTYPE, UsageProgram, load_usage_yaml, usage_columns

    n_nodes, ppn = args.nodes, args.pods_per_node
    n = n_nodes * ppn
    pods, nodes, (pvars, pidx) = bench.build_engines(0, n_nodes, ppn, 0, 0x6B776F6B, 0.1)
    for k in range(6):  # steady-state churn, as tools/agg_bench.py
        pods.step(bench.NOW0 + k * 10**9, 1, k)
    pods.sync()
    path = os.path.join(ROOT, "kwok_amd", "metrics", "usage-from-annotation.yaml")
    vkeys, cv, mv, mx, ck = usage_columns(UsageProgram(*load_usage_yaml(open(path).read())), pvars)
    keys = vkeys[pidx]
    node_ptr = np.arange(n_nodes + 1, dtype=np.uint32) * np.uint32(ppn)
    low = cel.lower_usage(cel.compile(RAMP), pod={"metadata": {"name": "p"}})
    ops = np.zeros(len(low), dtype=OP_DTYPE)
    for i, (op, x) in enumerate(low):
        ops[i] = (op, int(x), 0.0) if op == cel.OP_LOAD else (op, 0, float(x) if op == cel.OP_CONST else 0.0)
    mprogs = np.array([[0, len(low)]], dtype=np.uint32)
    ramp_id = np.uint32(len(mv))  # memory value id of program 0
    created = (bench.NOW0 - (np.arange(n, dtype=np.int64) % 3600) * 10**9)
    node_created = np.full(n_nodes, bench.NOW0 - 86400 * 10**9, dtype=np.int64)

    def on_ramp(k, sel):
        k = k.copy()
        k[sel] = (k[sel] & np.uint32(0xF0003FFF)) | (ramp_id << np.uint32(14))
        return k

    t = [bench.NOW0 + 10**10]
    res = {"pods": n, "nodes": n_nodes, "program_ops": len(low)}
    configs = [("constant", keys, False), ("no_dyn_pod", keys, True),
               ("dyn_10pct", on_ramp(keys, np.arange(n) % 10 == 0), True), ("dyn_all", on_ramp(keys, slice(None)), True)]
    for name, k, dyn in configs:
        if dyn:
            pods.usage_config(node_ptr, k, cv, mv, mx, ck, mem_progs=mprogs, ops=ops)
            pods.metrics_inputs(created, node_created, np.zeros(n_nodes), cel.zero_time_unix_second())
        else:
            pods.usage_config(node_ptr, k, cv, mv, mx, ck)
        res[name] = timed(pods, t, args.scrapes, args.warmup)
        res[name]["cluster"] = [float(x) for x in pods.usage_read(node_out=False)[1]]
    for name in ("no_dyn_pod", "dyn_10pct", "dyn_all"):
        res[name]["ratio_to_constant"] = round(res[name]["median_us"] / res["constant"]["median_us"], 3)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    pods.close()
    nodes.close()


if __name__ == "__main__":
    main()

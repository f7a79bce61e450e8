"""Incremental usage rows (kwk_usage_set_rows) against a full reconfiguration, with per-pod outputs
on: 0.1 %, 1 % and 10 % of the pods replaced by a pod whose key is already in the tables (RESET and
a new creation time).  One process per size; medians of --reps after --warmup.

  rows      per fraction: the time until kwk_usage_set_rows returns (host clock), the time until the
            stream has finished it (HIP events around the call), the next kwk_usage (HIP events),
            the counters of kwk_usage_info; then a twin engine configured from scratch with the
            final columns in the same process: the kernel both take and kwk_usage's time on each
  reconfig  the only path an engine without the entry points has, for the same final columns:
            kwk_usage_config + kwk_metrics_inputs + the kwk_usage_pods it invalidates (host clock:
            every one of them synchronises), and the next kwk_usage.  --tree DIR takes bench.py,
            the package and its built libraries from another checkout (the commit before, for the
            same-box baseline on its own build)

    python tools/usage_rows_bench.py --mode rows|reconfig [--nodes 10000] [--tree DIR] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRACTIONS = (0.001, 0.01, 0.1)


def med(xs):
    return {"median": round(statistics.median(xs), 2), "min": round(min(xs), 2), "max": round(max(xs), 2)}


def usage_us(eng, t):
    t[0] += 10**9
    eng.event_record(0)
    eng.usage(t[0])
    eng.event_record(1)
    eng.sync()
    return eng.event_elapsed_ms(0, 1) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("rows", "reconfig"), default="rows")
    ap.add_argument("--nodes", type=int, default=10_000)
    ap.add_argument("--pods-per-node", type=int, default=100)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--tree", default=ROOT, help="the checkout whose bench.py, package and libraries run")
    ap.add_argument("--tag", default="")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    sys.path.insert(0, tree)
    import bench
    from kwok_amd.host import abi, cel
    from kwok_amd.host.usage import UsageProgram, load_usage_yaml, usage_columns

    n_nodes, ppn = args.nodes, args.pods_per_node
    n = n_nodes * ppn
    path = os.path.join(tree, "kwok_amd", "metrics", "usage-from-annotation.yaml")
    node_ptr = np.arange(n_nodes + 1, dtype=np.uint32) * np.uint32(ppn)
    node_created = np.full(n_nodes, bench.NOW0 - 86400 * 10**9, dtype=np.int64)
    started = np.zeros(n_nodes)
    zero_s = cel.zero_time_unix_second()

    def engine():
        pods, nodes, (pvars, pidx) = bench.build_engines(0, n_nodes, ppn, 0, 0x6B776F6B, 0.1)
        nodes.close()
        for k in range(6):  # steady-state churn, as tools/agg_bench.py
            pods.step(bench.NOW0 + k * 10**9, 1, k)
        pods.sync()
        return pods, pvars, pidx

    pods, pvars, pidx = engine()
    vkeys, cv, mv, mx, ck = usage_columns(UsageProgram(*load_usage_yaml(open(path).read())), pvars)
    # two keys: the variants' own, and the same pod with an annotated cpu of 250m (a second cpu constant)
    cv = np.concatenate([cv, [0.25]])
    vkeys = np.array([vkeys[0], (int(vkeys[0]) & ~0x3FFF) | (len(cv) - 1)], dtype=np.uint32)
    keys = vkeys[(np.arange(n) % 3 == 0).astype(np.int64)]
    created = (bench.NOW0 - (np.arange(n, dtype=np.int64) % 3600) * 10**9)

    def configure(eng, k, c):
        eng.usage_config(node_ptr, k, cv, mv, mx, ck)
        eng.metrics_inputs(c, node_created, started, zero_s)
        eng.usage_pods(True)

    configure(pods, keys, created)
    t = [bench.NOW0 + 10**10]
    for _ in range(3):
        usage_us(pods, t)
    rng = np.random.default_rng(17)
    res = {"mode": args.mode, "tag": args.tag, "pods": n, "nodes": n_nodes, "reps": args.reps, "warmup": args.warmup,
           "tree": "this checkout" if tree == ROOT else os.path.basename(tree), "fractions": {}}
    for f in FRACTIONS:
        m = max(1, int(n * f))
        call, stream, nxt, counters = [], [], [], None
        for r in range(args.warmup + args.reps):
            slots = np.sort(rng.choice(n, m, replace=False)).astype(np.uint32)
            keys[slots] = np.where(keys[slots] == vkeys[0], vkeys[1], vkeys[0])  # the other variant's key: in the tables
            created[slots] = t[0] - 5 * 10**9
            if args.mode == "rows":
                rows = np.zeros(m, dtype=abi.USAGE_ROW_DTYPE)
                rows["slot"], rows["usage_key"], rows["created_ns"] = slots, keys[slots], created[slots]
                rows["flags"] = abi.USAGE_ROW_RESET | abi.USAGE_ROW_CREATED
                before = pods.usage_info()
                pods.sync()
                pods.event_record(0)
                t0 = time.perf_counter()
                pods.usage_set_rows(rows)
                t1 = time.perf_counter()
                pods.event_record(1)
                pods.sync()
                stream_us = pods.event_elapsed_ms(0, 1) * 1e3
                after = pods.usage_info()
                counters = {"syncs": after["syncs"] - before["syncs"], "allocs": after["allocs"] - before["allocs"]}
            else:
                pods.sync()
                t0 = time.perf_counter()
                configure(pods, keys, created)
                pods.sync()
                t1 = time.perf_counter()
                stream_us = (t1 - t0) * 1e6  # every call of a reconfiguration synchronises
            u = usage_us(pods, t)
            if r >= args.warmup:
                call.append((t1 - t0) * 1e6)
                stream.append(stream_us)
                nxt.append(u)
        res["fractions"][str(f)] = {"rows": m, "call_us": med(call), "stream_us": med(stream), "next_usage_us": med(nxt)}
        if counters is not None:
            res["fractions"][str(f)]["last_call_counters"] = counters
    res["cluster"] = [float(x) for x in pods.usage_read(node_out=False)[1]]
    if args.mode == "rows":  # a twin configured from scratch with the final columns, same process
        info = pods.usage_info()
        twin, _, _ = engine()
        configure(twin, keys, created)
        tw = [t[0]]
        for _ in range(3):
            usage_us(twin, tw)
            usage_us(pods, t)
        a, b = [], []
        for _ in range(args.reps):  # alternating
            a.append(usage_us(pods, t))
            b.append(usage_us(twin, tw))
        res["kernel"] = info["kernel"]
        res["twin_kernel"] = twin.usage_info()["kernel"]
        res["usage_us"] = med(a)
        res["twin_usage_us"] = med(b)
        assert res["kernel"] == res["twin_kernel"], res
        # the same clock on both: the instantaneous values are the twin's
        pods.usage(t[0] + 10**9)
        twin.usage(t[0] + 10**9)
        res["cluster_equals_twin"] = bool(np.array_equal(pods.usage_read(node_out=False)[1], twin.usage_read(node_out=False)[1]))
        twin.close()
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write(line + "\n")
    pods.close()


if __name__ == "__main__":
    main()

"""Time kwk_relayout against the reload path it replaces.

    python tools/relayout_bench.py --pods 1000000 --nodes 10000 [--out profiles/r21/relayout_bench.json]

A pod-fast engine in the 1-byte state with a usage configuration, per-pod usage outputs on and
kwk_metrics_inputs loaded is stepped and scraped, then relayouted three ways:
  (a) append 1 % nodes: every run is an identity, so only the new slots and the node arrays are written;
  (b) one more slot in every node: every run is shifted;
  (c) compaction after every second node is removed.
Each is timed with HIP events around the call (the device work) and by the call's wall time (its
host bookkeeping included: the usage book's mirrors are permuted on the CPU), medians of --reps after
--warmup; between two timed calls the inverse layout is applied untimed.  gather_bytes counts the
bytes the gathers write (the columns this engine has, past the identity prefix); bytes_per_s divides
them by the event time, which also holds the copies back out of the scratch buffer.
The baseline is the only path without the call: kwk_read -> permute on the host -> kwk_load +
kwk_usage_config + kwk_metrics_inputs, wall time to a synchronised stream; it also zeroes every
integrator.  It uses entry points this call does not touch.  Step time before and after (c) shows
the sweep shrinking with n_active.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NOW0, SEED = 1_700_000_000 * 10**9, 0x6B776F6B
# bytes per slot of the per-slot columns this configuration has: state id, due, deletion, record
# index, usage key (4 + 1), per-pod outputs, unit integrator, last evaluation, creation time
SLOT_BYTES = 1 + 8 + 8 + 4 + 4 + 1 + 32 + 16 + 8 + 8
NODE_BYTES = 16 + 8 + 32 + 8 + 8


def ukey(nc, cpu, mem):
    return (nc << 28) | (mem << 14) | cpu


def inverse(moves, node_moves):
    from kwok_amd.host import abi

    def inv(m):
        out = np.zeros(len(m), dtype=abi.MOVE_DTYPE)
        out["dst"], out["src"], out["n"] = m["src"], m["dst"], m["n"]
        return out[np.argsort(out["dst"], kind="stable")]
    return inv(moves), inv(node_moves)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", type=int, default=1_000_000)
    ap.add_argument("--nodes", type=int, default=10_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--baseline-reps", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from kwok_amd import workload as W
    from kwok_amd.host import abi, layout
    from kwok_amd.host.compiler import HarnessSpec, KindProgram
    from kwok_amd.host.engine import Engine, Ingest
    from kwok_amd.host.stages import load_stage_files

    n, nn = args.pods, args.nodes
    per = n // nn
    ptr = (np.arange(nn + 1, dtype=np.int64) * per).astype(np.uint32)
    n = int(ptr[-1])
    pvars = [W.pod_object("p", "n"), W.pod_object("p", "n", job=True)]
    prog = KindProgram(load_stage_files(*W.stage_paths(W.POD_FAST)), HarnessSpec())
    prog.explore(pvars)
    ing = Ingest(prog)
    idx = (np.arange(n, dtype=np.int64) * 2654435761 >> 9) % 10 == 0
    hot, dels, rec, cls = ing.variant_columns(pvars, idx.astype(np.int32))
    cpu, mem = np.array([0.0, 0.1, 0.25, 2.0]), np.array([0.0, 64.0 * 2**20, 2.0**30])
    keys = np.array([ukey(1, 1, 1), ukey(2, 2, 1), ukey(1, 3, 2)], dtype=np.uint32)[np.arange(n) % 3]
    created = NOW0 - (np.arange(n, dtype=np.int64) % 977) * 10**9
    node_created, started = np.full(nn, NOW0, dtype=np.int64), np.ones(nn)
    cap = n + n // 50 + nn + 64
    eng = Engine(prog, capacity=cap, state="auto", max_records=max(1, len(ing.records)) + 16)
    eng.load_stages()
    eng.set_harness(True)
    eng.load(hot, dels, rec, cls, ing.record_array())
    assert eng.stats()["state_bytes"] == 1
    eng.usage_config(ptr, keys, cpu, mem)
    eng.usage_pods(True)
    eng.metrics_inputs(created, node_created, started, 0.0)
    for k in range(3):
        eng.step(NOW0 + k * 10**9, SEED, k)
    eng.usage(NOW0 + 10**9)
    eng.usage(NOW0 + 3 * 10**9)
    eng.sync()
    fresh = ukey(1, 1, 1)
    result = {"pods": n, "nodes": nn, "capacity": cap, "state_bytes": 1, "slot_bytes": SLOT_BYTES, "reps": args.reps,
              "warmup": args.warmup, "layouts": {}}

    def step_us(k0):
        eng.event_record(2)
        eng.step_n(20, NOW0 + k0 * 10**9, 10**9, SEED, k0, False)
        eng.event_record(3)
        return eng.event_elapsed_ms(2, 3) * 1000.0 / 20

    def timed(name, plan):
        moves, new_ptr, node_moves = plan
        n_new, nn_new = int(new_ptr[-1]), len(new_ptr) - 1
        back_moves, back_nodes = inverse(moves, node_moves)
        keep = 0
        for m in moves:  # the identity prefix the gather leaves alone
            if int(m["dst"]) != keep or int(m["src"]) != keep:
                break
            keep += int(m["n"])
        nkeep = 0
        for m in node_moves:
            if int(m["dst"]) != nkeep or int(m["src"]) != nkeep:
                break
            nkeep += int(m["n"])
        gbytes = SLOT_BYTES * max(0, n_new - keep) + NODE_BYTES * max(0, nn_new - nkeep)
        ev, wall = [], []
        eng.usage_containers = None  # (the binding's own per-pod container mirror stays out of the call's wall time)
        for r in range(args.warmup + args.reps):
            eng.sync()
            eng.event_record(0)
            t0 = time.perf_counter()
            eng.relayout(moves, n_new, new_ptr, node_moves, fresh)
            t1 = time.perf_counter()
            eng.event_record(1)
            ms = eng.event_elapsed_ms(0, 1)
            if r >= args.warmup:
                ev.append(ms), wall.append((t1 - t0) * 1000.0)
            if r + 1 < args.warmup + args.reps:
                eng.relayout(back_moves, n, ptr, back_nodes, fresh)
        e, w = statistics.median(ev), statistics.median(wall)
        result["layouts"][name] = {"n_moves": len(moves), "n_active_new": n_new, "nodes_new": nn_new, "identity_prefix": keep,
                                   "event_ms_median": e, "event_ms": ev, "call_wall_ms_median": w, "gather_bytes": gbytes,
                                   "bytes_per_s": gbytes / (e / 1000.0) if e > 0 else None}
        print(name, json.dumps(result["layouts"][name])[:300], flush=True)
        return back_moves, back_nodes

    plans = {
        "a_append_1pct_nodes": layout.plan_layout(ptr, added_nodes=[per] * max(1, nn // 100)),
        "b_one_more_slot_per_node": layout.plan_layout(ptr, room=np.full(nn, per + 1)),
    }
    for name, plan in plans.items():
        back = timed(name, plan)
        eng.relayout(back[0], n, ptr, back[1], fresh)
    result["step_us_before_compaction"] = step_us(10)
    plan_c = layout.plan_layout(ptr, removed_nodes=list(range(1, nn, 2)))
    timed("c_compaction_every_second_node_removed", plan_c)
    result["step_us_after_compaction"] = step_us(40)
    result["n_active_after_compaction"] = int(plan_c[1][-1])

    # the baseline: read back, permute on the host, load and configure again (every integrator restarts)
    moves, new_ptr, node_moves = plans["b_one_more_slot_per_node"]
    n_new = int(new_ptr[-1])
    eng.load(hot, dels, rec, cls, ing.record_array())
    eng.usage_config(ptr, keys, cpu, mem)
    eng.metrics_inputs(created, node_created, started, 0.0)
    eng.sync()
    zero = np.zeros(1, dtype=abi.HOT_DTYPE)[0]
    base = []
    for r in range(args.baseline_reps):
        t0 = time.perf_counter()
        h, d = eng.read(0, n)
        h2, d2 = layout.apply_moves(h, moves, n_new, zero), layout.apply_moves(d, moves, n_new, abi.DEL_ABSENT)
        r2 = layout.apply_moves(rec, moves, n_new, 0)
        c2 = (h2["sched"] >> np.uint32(16)).astype(np.uint16)
        k2 = layout.apply_moves(keys, moves, n_new, fresh)
        cr2 = layout.apply_moves(created, moves, n_new, np.iinfo(np.int64).min)
        eng.load(h2, d2, r2, c2, ing.record_array())
        eng.usage_config(new_ptr, k2, cpu, mem)
        eng.metrics_inputs(cr2, node_created, started, 0.0)
        eng.sync()
        base.append((time.perf_counter() - t0) * 1000.0)
        eng.load(hot, dels, rec, cls, ing.record_array())  # back, untimed
        eng.usage_config(ptr, keys, cpu, mem)
        eng.metrics_inputs(created, node_created, started, 0.0)
    result["baseline_reload_layout_b"] = {"wall_ms_median": statistics.median(base), "wall_ms": base,
                                          "note": "kwk_read -> numpy permute -> kwk_load + kwk_usage_config + kwk_metrics_inputs, "
                                                  "same library (entry points this change does not touch); loses every integrator"}
    eng.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

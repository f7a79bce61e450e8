#!/usr/bin/env python3
"""Device patch emission from the hand-back ring, timed against the per-step path on the pod-fast
shape (the headline's: 1M nodes / 100M pods, harness churn on).

    python tools/emit_ring_bench.py [--nodes 1000000 --ppn 100] [--rounds 6 --warmup 1] [--settle 8]
                                    [--leg both|a] [--out profiles/r11/emit_ring_bench.json] [--tag run1]

Two legs in one process, alternating round by round over the same engine and emitter, four steps
per leg and round:

  (a) the per-step path: step_n(1, ..., "packed") + kwk_emit + kwk_emit_result, per step — the
      only way to get every step's patches on the device before kwk_emit_step;
  (b) the ring path: step_n(4, ..., "packed16") — one fused sweep launch and one hand-back launch —
      then four kwk_emit_step into four output sets, read afterwards.

Per leg (mean, median, min and max over the steps of the rounds after --warmup): the emission kernels' time per
step (kwk_emit_elapsed: segment bases + tile segments + size + scan + write for (b), size + scan
+ write for (a)), the step's total device time by HIP events on the engine's stream (sweep +
hand-back + emission; (b): the group's span / 4), the patch bytes written per step and GB/s of the
emission kernels.  --leg a uses only calls the parent commit has, so the same file run from a
checkout of the parent measures the parent's library in a separate process.  The result is merged
into the JSON file under --tag."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GROUP = 4


def build(n_nodes, ppn, seed):
    import bench
    from kwok_amd import workload as W
    from kwok_amd.host import emit
    from kwok_amd.host.compiler import HarnessSpec, KindProgram
    from kwok_amd.host.engine import Engine, Ingest
    from kwok_amd.host.patchtpl import PatchProgram
    from kwok_amd.host.stages import load_stage_files
    n = n_nodes * ppn
    pvars = [W.pod_object("p", "n"), W.pod_object("p", "n", job=True)]
    pidx = bench.shard_pod_variants(0, n, seed, 0.1)
    prog = KindProgram(load_stage_files(*W.stage_paths(W.POD_FAST)), HarnessSpec())
    prog.explore(pvars)
    ing = Ingest(prog)
    hot, dels, rec, cls = ing.variant_columns(pvars, pidx)
    pods = Engine(prog, capacity=n, max_records=max(1, len(ing.records)) + 16)
    pods.load_stages()
    pods.set_harness(True)
    pods.load(hot, dels, rec, cls, ing.record_array())
    del hot, dels, rec, cls
    pp = PatchProgram(prog.stages, {"NodeIPWith": lambda *a: "10.100.100.100", "PodIPWith": lambda *a: "11.100.100.100"})
    vcls = [prog.class_of(v, register=False) for v in pvars]
    ep = emit.EmitProgram(prog.stages, pp, dict(zip(vcls, pvars)), len(prog.class_ids), stride=16)
    wv = []
    for c, v in zip(vcls, pvars):
        acc = 0
        for tid in range(ep.host_tid):
            sk = ep.skel.get((c, tid))
            if sk is not None:
                acc |= int(pp.object_values(tid, [v], sk["text"], sk["calls"], ep.stride)[1][0]) << tid
        wv.append(c | ep.guard_bits(v) << 16 | acc << 32)
    em = emit.Emitter(pods, n, ep)
    chunk = 1 << 24
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        em.set_rows(a, np.asarray(wv, dtype=np.uint64)[pidx[a:b]], {})
        for c in range(ep.n_columns):
            em.set_column(c, a, bench.synth_ipv4(a, b - a, 10 + c, ep.stride))
    max_skel = max((sum(len(x.encode()) for x in sk["lits"]) + 40 * len(sk["slots"]) for sk in ep.skel.values()), default=1)
    return pods, em, max_skel


def spread(xs):
    return {"mean": round(statistics.mean(xs), 2), "median": round(statistics.median(xs), 2), "min": round(min(xs), 2),
            "max": round(max(xs), 2), "n": len(xs)}


def main():
    import bench
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--ppn", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=6,
                    help="a multiple of 3: the Job pods cycle ready / complete / delete in step, and 6 rounds of "
                         "8 steps give each leg every phase equally often")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--settle", type=int, default=8, help="steps without emission first (the churn's steady state)")
    ap.add_argument("--leg", choices=("both", "a"), default="both")
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0x6B776F6B)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "emit_ring_bench.json"))
    ap.add_argument("--tag", default="run")
    args = ap.parse_args()
    now0, dt = bench.NOW0, 10**9
    pods, em, max_skel = build(args.nodes, args.ppn, args.seed)
    n = pods.capacity
    k = 0
    pods.step_n(args.settle, now0, dt, args.seed, 0, False)
    k += args.settle
    # room: a step of the settled churn fires ~10 % of the pods; 2x that, re-reserved on KWK_ECAP
    items_cap, bytes_cap = n // 5 + 1024, (n // 5) * max_skel + 4096
    if args.leg == "both":
        pods.fired_keep(GROUP)
        em.reserve_sets(GROUP, items_cap, bytes_cap)
    else:
        em.reserve(items_cap, bytes_cap)
    legs = {"a": {"emit_us": [], "total_us": [], "bytes": [], "items": []},
            "b": {"emit_us": [], "total_us": [], "bytes": [], "items": []}}
    for rnd in range(args.rounds + args.warmup):
        keep = rnd >= args.warmup
        # ---- (a) per step: sweep + 4-byte hand-back, kwk_emit, its result
        for j in range(GROUP):
            now = now0 + k * dt
            pods.event_record(0)
            pods.step_n(1, now, dt, args.seed, k, "packed")
            em.emit(now, packed=True)
            pods.event_record(1)
            ni, nb = em.result()
            assert ni >= 0, "leg a: reservation too small"
            if keep:
                legs["a"]["emit_us"].append(em.elapsed_ms() * 1e3)
                legs["a"]["total_us"].append(pods.event_elapsed_ms(0, 1) * 1e3)
                legs["a"]["bytes"].append(nb)
                legs["a"]["items"].append(ni)
            k += 1
        if args.leg != "both":
            continue
        # ---- (b) the ring: one fused call, four emissions back to back, read afterwards
        now = now0 + k * dt
        pods.event_record(2)
        pods.step_n(GROUP, now, dt, args.seed, k, "packed16")
        for j in range(GROUP):
            em.emit_step(k + j, now + j * dt)
        pods.event_record(3)
        assert pods.last_sweep()["steps"] == GROUP, pods.last_sweep()
        total = pods.event_elapsed_ms(2, 3) * 1e3 / GROUP
        for j in range(GROUP):
            em.select(GROUP - 1 - j)
            ni, nb = em.result()
            assert ni >= 0, "leg b: reservation too small"
            if keep:
                legs["b"]["emit_us"].append(em.elapsed_ms() * 1e3)
                legs["b"]["bytes"].append(nb)
                legs["b"]["items"].append(ni)
        if keep:
            legs["b"]["total_us"].append(total)
        k += GROUP
    res = {"nodes": args.nodes, "pods": n, "rounds": args.rounds, "steps_per_leg_and_round": GROUP, "settle_steps": args.settle}
    for name, d in legs.items():
        if not d["emit_us"]:
            continue
        by = statistics.mean(d["bytes"])
        res["leg_" + name] = {
            "emit_kernels_us_per_step": spread(d["emit_us"]), "total_us_per_step": spread(d["total_us"]),
            "patch_bytes_per_step": round(by), "items_per_step": round(statistics.mean(d["items"])),
            "emit_written_GBps": round(sum(d["bytes"]) / (sum(d["emit_us"]) * 1e-6) / 1e9, 1)}
    res["note"] = ("a: step_n(1, packed) + kwk_emit + kwk_emit_result per step; b: step_n(4, packed16) + 4 kwk_emit_step, "
                   "read afterwards (total: the group's span / 4); HIP events on the engine's stream")
    em.close()
    pods.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    doc = {}
    if os.path.exists(args.out):
        doc = json.load(open(args.out))
    doc[args.tag] = res
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({args.tag: res}))


if __name__ == "__main__":
    main()

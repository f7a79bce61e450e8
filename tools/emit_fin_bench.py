#!/usr/bin/env python3
"""What the finalizer patches add to a step's emission, on the pod-general mix (pod-create adds
kwok.x-k8s.io/fake, pod-remove-finalizer and pod-delete take it away; harness churn on).

    python tools/emit_fin_bench.py [--pods 100000000] [--steps 24 --warmup 4] [--settle 8]
                                   [--out profiles/r12/emit_fin_bench.json] [--tag run1]

Two emitters over one engine's lists, loaded identically, one of them with the finalizer program
(kwk_emit_finalizers_load): every step is emitted by both, in an order that alternates step by
step, so the difference of their kwk_emit_elapsed is the three finalizer launches (size, scan,
write) on the same list.  Reported (mean, median, min, max over the steps after --warmup): the
merge-patch emission's µs per step (the emitter without the program), the µs the finalizer launches
add, the finalizer bytes and items per step and their written GB/s, and the share of the added time
in the step's total (sweep + hand-back + the emission with finalizers, HIP events on the engine's
stream).  The (a) leg of the measurement — C5 with no finalizer program against the parent commit —
is tools/emit_ring_bench.py --leg a run from both checkouts.  The result is merged into --out under
--tag."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build(n, seed):
    import bench
    from kwok_amd import workload as W
    from kwok_amd.host import emit
    from kwok_amd.host.compiler import HarnessSpec, KindProgram
    from kwok_amd.host.engine import Engine, Ingest
    from kwok_amd.host.patchtpl import PatchProgram
    from kwok_amd.host.stages import load_stage_files
    pvars, pidx = W.c2_pod_variants(0, n, seed=seed, job_frac=0.1)
    prog = KindProgram(load_stage_files(*W.stage_paths(W.POD_GENERAL + W.POD_CHAOS)), HarnessSpec())
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
    fp = emit.FinProgram(prog.finalizer_spec())
    wv, fw = [], []
    for c, v in zip(vcls, pvars):
        acc = 0
        for tid in range(ep.host_tid):
            sk = ep.skel.get((c, tid))
            if sk is not None:
                acc |= int(pp.object_values(tid, [v], sk["text"], sk["calls"], ep.stride)[1][0]) << tid
        wv.append(c | ep.guard_bits(v) << 16 | acc << 32)
        fw.append(fp.word((v.get("metadata") or {}).get("finalizers")))
    ems = [emit.Emitter(pods, n, ep), emit.Emitter(pods, n, ep)]
    ems[1].load_finalizers(fp)
    chunk = 1 << 24
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        for em in ems:
            em.set_rows(a, np.asarray(wv, dtype=np.uint64)[pidx[a:b]], {})
            for c in range(ep.n_columns):
                em.set_column(c, a, bench.synth_ipv4(a, b - a, 10 + c, ep.stride))
        ems[1].set_fin_words(a, np.asarray(fw, dtype=np.uint32)[pidx[a:b]])
    max_skel = max((sum(len(x.encode()) for x in sk["lits"]) + 40 * len(sk["slots"]) for sk in ep.skel.values()), default=1)
    return pods, ems, max_skel, ep.n_columns, prog.describe()["finalizers"], fp.values.index("kwok.x-k8s.io/fake")


def spread(xs):
    return {"mean": round(statistics.mean(xs), 2), "median": round(statistics.median(xs), 2), "min": round(min(xs), 2),
            "max": round(max(xs), 2), "n": len(xs)}


def main():
    import bench
    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--settle", type=int, default=8, help="steps without emission first")
    ap.add_argument("--frac", type=float, default=0.3, help="room reserved: this fraction of the pods fire in a step")
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0x6B776F6B)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r12", "emit_fin_bench.json"))
    ap.add_argument("--tag", default="run")
    args = ap.parse_args()
    now0, dt = bench.NOW0, 500 * 10**6
    pods, ems, max_skel, n_cols, fin_bits, fake_id = build(args.pods, args.seed)
    n = pods.capacity
    room = int(n * args.frac) + 1024
    for em in ems:
        em.reserve(2 * room, room * max_skel + 4096)
    ems[1].reserve_fin(room, room * 96 + 4096)
    # settle without emission (step 0 fires every pod), then give the order words the engine's state:
    # a pod whose finalizer bit is set carries kwok.x-k8s.io/fake
    pods.step_n(args.settle, now0, dt, args.seed, 0, False)
    k = args.settle
    bit = fin_bits["kwok.x-k8s.io/fake"]
    chunk = 1 << 24
    for a in range(0, n, chunk):
        pred = pods.read(a, min(chunk, n - a))[0]["pred"]
        ems[1].set_fin_words(a, np.where((pred >> np.uint32(bit)) & np.uint32(1), np.uint32(1 << 28 | fake_id), np.uint32(0)))
    d = {"merge_us": [], "with_fin_us": [], "total_us": [], "fin_bytes": [], "fin_items": [], "bytes": [], "items": []}
    for j in range(args.warmup + args.steps):
        now = now0 + k * dt
        keep = j >= args.warmup
        order = (0, 1) if j % 2 == 0 else (1, 0)
        pods.event_record(0)
        pods.step_n(1, now, dt, args.seed, k, "packed")
        pods.event_record(1)
        for i in order:
            ems[i].emit(now, packed=True)
        us = []
        for i in (0, 1):
            ni, nb = ems[i].result()
            assert ni >= 0, f"reservation too small (--frac): {ems[i].fin_result() if i else (ni, nb)}"
            us.append(ems[i].elapsed_ms() * 1e3)
        st, fi, fb = ems[1].fin_result()
        assert st == 0
        if keep:
            d["merge_us"].append(us[0])
            d["with_fin_us"].append(us[1])
            d["total_us"].append(pods.event_elapsed_ms(0, 1) * 1e3 + us[1])
            d["fin_bytes"].append(fb)
            d["fin_items"].append(fi)
            d["bytes"].append(nb)
            d["items"].append(ni)
        k += 1
    added = [b - a for a, b in zip(d["merge_us"], d["with_fin_us"])]
    quiet = [x for x, fi in zip(added, d["fin_items"]) if fi == 0]
    res = {"pods": n, "steps": args.steps, "settle_steps": args.settle, "value_columns": n_cols,
           "merge_emit_us_per_step": spread(d["merge_us"]), "with_finalizers_emit_us_per_step": spread(d["with_fin_us"]),
           "finalizer_added_us_per_step": spread(added),
           "finalizer_added_us_on_steps_without_an_op": spread(quiet) if quiet else None,
           "step_total_us": spread(d["total_us"]),
           "finalizer_share_of_step_total": round(sum(added) / sum(d["total_us"]), 4),
           "merge_bytes_per_step": round(statistics.mean(d["bytes"])), "merge_items_per_step": round(statistics.mean(d["items"])),
           "finalizer_bytes_per_step": round(statistics.mean(d["fin_bytes"])),
           "finalizer_items_per_step": round(statistics.mean(d["fin_items"])),
           "merge_written_GBps": round(sum(d["bytes"]) / (sum(d["merge_us"]) * 1e-6) / 1e9, 1),
           "finalizer_written_GBps": round(sum(d["fin_bytes"]) / (max(sum(added), 1e-9) * 1e-6) / 1e9, 2),
           "note": "two emitters on one engine, the second with kwk_emit_finalizers_load; added = the difference of their "
                   "kwk_emit_elapsed on the same list, order alternating step by step; total = sweep + hand-back (HIP "
                   "events) + the emission with finalizers"}
    for em in ems:
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

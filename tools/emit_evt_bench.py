#!/usr/bin/env python3
"""What the event stream adds to a step's emission, on the pod-general + chaos mix with harness
churn (pod-create records "Created", pod-remove-finalizer "Killing").

    python tools/emit_evt_bench.py [--pods 100000000] [--steps 24 --warmup 4] [--settle 8]
                                   [--out profiles/r19/emit_evt_bench.json] [--tag run1]

Two emitters over one engine's lists, loaded identically (both with the finalizer program), one of
them with the event program (kwk_evt_load): every step is emitted by both, in an order that
alternates step by step, so the difference of their kwk_emit_elapsed is the three event launches
(size, scan, write) on the same list.  Reported (mean, median, min, max over the steps after
--warmup): the µs per step of the emission without events, the µs the event launches add, the
event items and bytes per step and their written GB/s.  Identity rows are synthetic: names
pod-<slot>, namespaces ns<slot % 100>, uids 36 bytes.  The (a) leg of the measurement — C5 with no
event program against the parent commit — is tools/emit_ring_bench.py --leg a run from both
checkouts.  The result is merged into --out under --tag."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

STRIDES = (16, 8, 40)


def digits_rows(first, n, prefix, stride, mod=None, width=None):
    """[length][prefix + decimal(slot or slot % mod)] rows, vectorised."""
    v = np.arange(first, first + n, dtype=np.uint64)
    if mod:
        v %= np.uint64(mod)
    nd = np.ones(n, dtype=np.int64)
    for p in range(1, 12):
        nd += v >= np.uint64(10**p)
    rows = np.zeros((n, stride), dtype=np.uint8)
    pre = np.frombuffer(prefix.encode(), dtype=np.uint8)
    rows[:, 1:1 + len(pre)] = pre
    rows[:, 0] = len(pre) + nd
    for p in range(12):  # digit p from the right goes to column len(pre) + nd - p
        has = nd > p
        col = (1 + len(pre) + nd - 1 - p)[has]
        rows[np.flatnonzero(has), col] = (48 + (v[has] // np.uint64(10**p)) % np.uint64(10)).astype(np.uint8)
    return rows


def uid_rows(first, n, stride):
    """36 bytes of lowercase hex and dashes from the slot (a UUID's shape)."""
    v = np.arange(first, first + n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    rows = np.zeros((n, stride), dtype=np.uint8)
    rows[:, 0] = 36
    hexd = np.frombuffer(b"0123456789abcdef", dtype=np.uint8)
    for j in range(36):
        rows[:, 1 + j] = 45 if j in (8, 13, 18, 23) else hexd[((v >> np.uint64(4 * (j % 16))) & np.uint64(15)).astype(np.int64)]
    return rows


def main():
    import bench
    import emit_fin_bench as FB
    from kwok_amd import workload as W
    from kwok_amd.host import events
    from kwok_amd.host.compiler import KindProgram
    from kwok_amd.host.stages import load_stage_files
    ap = argparse.ArgumentParser()
    ap.add_argument("--pods", type=int, default=100_000_000)
    ap.add_argument("--steps", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--settle", type=int, default=8, help="steps without emission first")
    ap.add_argument("--frac", type=float, default=0.3, help="room reserved: this fraction of the pods fire in a step")
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=0x6B776F6B)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19", "emit_evt_bench.json"))
    ap.add_argument("--tag", default="run")
    args = ap.parse_args()
    now0, dt = bench.NOW0, 500 * 10**6
    pods, ems, max_skel, n_cols, fin_bits, fake_id = FB.build(args.pods, args.seed)
    n = pods.capacity
    fp = ems[1].fin_program
    ems[0].load_finalizers(fp)  # both emit the finalizer stream: the difference is the events alone
    spec = KindProgram(load_stage_files(*W.stage_paths(W.POD_GENERAL + W.POD_CHAOS))).event_spec(device=True)
    evp = events.EventProgram(spec, STRIDES)
    ems[1].load_events(evp)
    chunk = 1 << 22
    for a in range(0, n, chunk):
        m = min(chunk, n - a)
        ems[1].set_event_rows(a, {events.COL_NAME: digits_rows(a, m, "pod-", STRIDES[0]),
                                  events.COL_NAMESPACE: digits_rows(a, m, "ns", STRIDES[1], mod=100),
                                  events.COL_UID: uid_rows(a, m, STRIDES[2])})
    room = int(n * args.frac) + 1024
    for em in ems:
        em.reserve(2 * room, room * max_skel + 4096)
        em.reserve_fin(room, room * 96 + 4096)
    ems[1].reserve_events(room, room * 520 + 4096)
    pods.step_n(args.settle, now0, dt, args.seed, 0, False)
    k = args.settle
    bit = fin_bits["kwok.x-k8s.io/fake"]
    for a in range(0, n, 1 << 24):
        pred = pods.read(a, min(1 << 24, n - a))[0]["pred"]
        w = np.where((pred >> np.uint32(bit)) & np.uint32(1), np.uint32(1 << 28 | fake_id), np.uint32(0))
        for em in ems:
            em.set_fin_words(a, w)
    d = {"base_us": [], "with_evt_us": [], "evt_bytes": [], "evt_items": [], "bytes": [], "items": []}
    for j in range(args.warmup + args.steps):
        now = now0 + k * dt
        keep = j >= args.warmup
        order = (0, 1) if j % 2 == 0 else (1, 0)
        pods.step_n(1, now, dt, args.seed, k, "packed")
        for i in order:
            ems[i].emit(now, packed=True)
        us = []
        for i in (0, 1):
            ni, nb = ems[i].result()
            assert ni >= 0, f"reservation too small (--frac): {ems[i].event_result() if i else (ni, nb)}"
            us.append(ems[i].elapsed_ms() * 1e3)
        st, ei, eb, launched = ems[1].event_result()
        assert st == 0 and launched == 1
        if keep:
            d["base_us"].append(us[0])
            d["with_evt_us"].append(us[1])
            d["evt_bytes"].append(eb)
            d["evt_items"].append(ei)
            d["bytes"].append(nb)
            d["items"].append(ni)
        k += 1
    added = [b - a for a, b in zip(d["base_us"], d["with_evt_us"])]
    res = {"pods": n, "steps": args.steps, "settle_steps": args.settle, "row_strides": list(STRIDES),
           "emit_us_per_step_without_events": FB.spread(d["base_us"]), "emit_us_per_step_with_events": FB.spread(d["with_evt_us"]),
           "event_added_us_per_step": FB.spread(added),
           "event_items_per_step": FB.spread(d["evt_items"]), "event_bytes_per_step": FB.spread(d["evt_bytes"]),
           "merge_items_per_step": round(statistics.mean(d["items"])), "merge_bytes_per_step": round(statistics.mean(d["bytes"])),
           "event_written_GBps": round(sum(d["evt_bytes"]) / (max(sum(added), 1e-9) * 1e-6) / 1e9, 2),
           "note": "two emitters on one engine, both with the finalizer program, the second with kwk_evt_load; added = the "
                   "difference of their kwk_emit_elapsed on the same list, order alternating step by step"}
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

#!/usr/bin/env python3
"""Merges the side results of the event-stream measurement into the file tools/emit_evt_bench.py
writes (profiles/r19/emit_evt_bench.json), so that every section of it comes from the tree:

    python tools/emit_evt_profile.py [--out profiles/r19/emit_evt_bench.json]
        [--kernel-stats run_kernel_stats.csv [--kernel-stats-bench kt_bench.json]]
        [--resource-remarks remarks.txt] [--bench-line bench_stdout.txt] [--leg-a leg_a.json]

--kernel-stats: the CSV of `rocprofv3 --kernel-trace --stats --output-format csv -- python
  tools/emit_evt_bench.py --pods 10000000 --steps 6 --warmup 2 --tag kt --out kt_bench.json`
  (section kernel_trace_10M: the emitter's kernels; kernel_trace_10M_bench: that run's own result).
--resource-remarks: stderr of `hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -I include
  -Rpass-analysis=kernel-resource-usage kwok_amd/csrc/emit.hip ...` (section
  c_kernel_resource_usage_gfx950: SGPRs, VGPRs, scratch, LDS and occupancy per kernel).
--bench-line: stdout of `python bench.py --gpus 1 --steps 20 --warmup 5` (section bench_py_headline).
--leg-a: the --out file of `tools/emit_ring_bench.py --leg a` runs tagged this_<i> / parent_<i>
  (section a_no_event_program_C5, with the two means and the parent's range)."""
import argparse
import csv
import json
import os
import re
import statistics
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def short(name):
    return re.sub(r"\(anonymous namespace\)::|void ", "", name).split("(")[0]


def kernel_stats(path):
    out = {}
    for r in csv.DictReader(open(path)):
        if "emit_" in r.get("Name", ""):
            out[short(r["Name"])] = {"calls": int(r["Calls"]), "avg_ns": float(r["AverageNs"]),
                                     "total_ns": int(float(r["TotalDurationNs"])), "pct": float(r["Percentage"])}
    return out


def resource_remarks(path):
    keys = ["TotalSGPRs", "VGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]"]
    rows, cur = {}, None
    for line in open(path):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = rows.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z][\w /\[\]]*?): (\S+) \[-Rpass", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    names = subprocess.run(["c++filt"], input="\n".join(rows), capture_output=True, text=True).stdout.split("\n")
    return {"columns": ["SGPRs", "VGPRs", "scratch bytes/lane", "LDS bytes/block", "occupancy waves/SIMD"],
            "kernels": {short(n): [v.get(k) for k in keys] for n, v in zip(names, rows.values())}}


def leg_a(path):
    d = json.load(open(path))
    out = {"runs": d}
    for w in ("this", "parent"):
        xs = [v["leg_a"]["emit_kernels_us_per_step"]["mean"] for k, v in sorted(d.items()) if k.startswith(w + "_")]
        if xs:
            out[w] = {"emit_us_means": xs, "mean": round(statistics.mean(xs), 2), "min": min(xs), "max": max(xs)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r19", "emit_evt_bench.json"))
    ap.add_argument("--kernel-stats")
    ap.add_argument("--kernel-stats-bench")
    ap.add_argument("--resource-remarks")
    ap.add_argument("--bench-line")
    ap.add_argument("--leg-a")
    args = ap.parse_args()
    doc = json.load(open(args.out)) if os.path.exists(args.out) else {}
    if args.kernel_stats:
        doc["kernel_trace_10M"] = kernel_stats(args.kernel_stats)
    if args.kernel_stats_bench:
        doc["kernel_trace_10M_bench"] = next(iter(json.load(open(args.kernel_stats_bench)).values()))
    if args.resource_remarks:
        doc["c_kernel_resource_usage_gfx950"] = resource_remarks(args.resource_remarks)
    if args.bench_line:
        for line in open(args.bench_line):
            if line.startswith('{"metric"'):
                d = json.loads(line)
                doc["bench_py_headline"] = {k: d[k] for k in ("metric", "value", "ms_per_step", "steps", "warmup")}
    if args.leg_a:
        doc["a_no_event_program_C5"] = leg_a(args.leg_a)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: (v if k.startswith("a_") and "runs" not in v else "...") for k, v in doc.items()})[:600])


if __name__ == "__main__":
    main()

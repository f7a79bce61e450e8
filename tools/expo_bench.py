#!/usr/bin/env python3
"""Device metric exposition (kwok_expo.h) timed on the shipped Metric CR at run_metrics' C4 size,
and at a larger size in node-range chunks that fit the reservation.

    python tools/expo_bench.py [--nodes 10000 --pods 1000000] [--chunk 0] [--scrapes 10 --warmup 3]
                               [--sample 16] [--out profiles/r7/expo_bench.json] [--tag c4]
    python tools/expo_bench.py --hist [--out profiles/r8/expo_hist_bench.json] [--tag c4_hist]

Per all-node scrape, by HIP events on the engine's stream (medians over --scrapes, after --warmup):
microseconds of the lengths / scan / write kernels, the bytes written, GB/s of the write kernel and
of the three kernels together; the same with the other workgroup width.  Then the parent commit's
only path — MetricsProgram.scrape + exposition in Python — timed on --sample nodes and
extrapolated (stated as such) to every node; those nodes' device text is compared byte for byte.
The result is merged into the JSON file under --tag.

--hist: the histogram leg.  The CR is the shipped families plus one pod-dimension and one
container-dimension histogram of 5 visible buckets over pod.Usage("memory") /
pod.Usage("cpu", container.name), compiled with expo_histograms (kwk_expo_create_hist); the
scalar-only CR is measured first in the same process and recorded beside it ("scalar_same_run"),
with the histogram write pass's bytes/s relative to the scalar pass's.

--churn: the label-commit leg (default --out profiles/r10/expo_commit_bench.json --tag churn_c4).
A seeded 0.1 %, 1 % and 10 % of the pods are renamed; per fraction, in one process, the host wall
time of kwk_expo_set_labels + kwk_expo_commit_rows, the HIP-event times of its scatter and sort
kernels, and the wall time of kwk_expo_set_labels + a full kwk_expo_commit of the same changes
(medians of 5 after 1 warm-up).  The permutations and sampled nodes' text after the incremental
commit are compared with a full commit's.
"""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


LABELS = {"pod": [{"name": "namespace", "value": "pod.metadata.namespace"}, {"name": "pod", "value": "pod.metadata.name"}],
          "container": [{"name": "container", "value": "container.name"},
                        {"name": "namespace", "value": "pod.metadata.namespace"},
                        {"name": "pod", "value": "pod.metadata.name"}]}


def hist_cr_text():
    """The shipped Metric CR plus a pod and a container histogram (5 visible buckets each; the
    labels of the shipped pod / container families, so they share their label groups)."""
    import yaml
    from kwok_amd.configs import METRIC_CR
    from kwok_amd.host.metrics import load_metric_doc
    doc = load_metric_doc(open(METRIC_CR).read())
    mib, milli = 'pod.Usage("memory") / 1048576.0', 'pod.Usage("cpu", container.name) * 1000.0'
    doc["spec"]["metrics"] += [
        {"name": "pod_memory_working_set_mib", "kind": "histogram", "dimension": "pod", "help": "pod memory (MiB)",
         "labels": LABELS["pod"],
         "buckets": [{"le": le, "value": mib} for le in (16, 64, 256, 1024, 4096)]},
        {"name": "container_cpu_millicores", "kind": "histogram", "dimension": "container", "help": "container cpu (m)",
         "labels": LABELS["container"],
         "buckets": [{"le": le, "value": milli} for le in (10, 100, 500, 1000, 4000)]}]
    return yaml.safe_dump(doc)


def build_rig(n_nodes, n_pods, seed, cr_text=None):
    from kwok_amd.configs import METRIC_CR, NOW0, USAGE_YAML, c4_pod_workload
    from kwok_amd.host import cel
    from kwok_amd.host.compiler import KindProgram
    from kwok_amd.host.engine import Engine, Ingest
    from kwok_amd.host.metrics import MetricsProgram
    from kwok_amd.host.stages import load_stage_files
    from kwok_amd.host.usage import UsageProgram, load_usage_yaml, usage_columns
    from kwok_amd import workload as W
    pvars, pidx, node_ptr = c4_pod_workload(n_nodes, n_pods, seed)
    prog = KindProgram(load_stage_files(*W.stage_paths(W.POD_FAST)))
    prog.explore(pvars)
    ing = Ingest(prog)
    hot, dels, rec, cls = ing.variant_columns(pvars, pidx)
    pods = Engine(prog, capacity=n_pods, max_records=max(1, len(ing.records)) + 16)
    pods.load_stages()
    pods.load(hot, dels, rec, cls, ing.record_array())
    up = UsageProgram(*load_usage_yaml(open(USAGE_YAML).read()))
    vkeys, cv, mv, mx, ck = usage_columns(up, pvars)
    pods.usage_config(node_ptr, vkeys[pidx], cv, mv, mx, ck)
    pods.usage_pods(True)
    mp = MetricsProgram.from_native(cr_text, expo_histograms=True) if cr_text else \
        MetricsProgram.from_native(open(METRIC_CR).read())
    mp.load(pods)
    slots = np.arange(n_pods, dtype=np.int64)
    created = NOW0 - ((slots * 7919) % 86400) * 10**9 - 3600 * 10**9
    created[slots % 101 == 0] = np.iinfo(np.int64).min
    zero_unix = float(cel.wrap_int64(cel.GO_ZERO_TIME.ns)) / 1e9
    pods.metrics_inputs(created, np.full(n_nodes, np.iinfo(np.int64).min, dtype=np.int64), np.zeros(n_nodes), zero_unix)
    return pods, mp, pvars, pidx, node_ptr, NOW0


def upload_labels_native(ex, pvars, pidx, n_pods):
    """Every row through the public path (Exposition.set_pods: kwk_metric_labels_render per object).
    About 50 us per pod from Python, so --native-labels is for sizes up to ~100k pods."""
    step = 20_000
    for lo in range(0, n_pods, step):
        objs = []
        for i in range(lo, min(n_pods, lo + step)):
            o = copy.deepcopy(pvars[int(pidx[i])])
            o["metadata"]["name"] = f"pod-{i}"
            objs.append(o)
        ex.set_pods(objs, lo)


def upload_labels(ex, mp, pvars, pidx, n_pods):
    """Every pod's and container's label rows, formatted here as the native renderer renders them
    (checked against it on a sample), in chunks: at 1M pods the per-object renderer calls from
    Python would take about a minute of setup (--native-labels takes that path)."""
    from kwok_amd.host.expo import DIM_CONTAINER, DIM_POD
    ncont = np.array([len(v["spec"]["containers"]) for v in pvars])[pidx]
    step = 200_000
    for g, (dim, n_labels) in enumerate(ex.groups):
        if dim == DIM_POD:
            for lo in range(0, n_pods, step):
                hi = min(n_pods, lo + step)
                ex.set_rows(g, lo, [b'{namespace="default",pod="pod-%d"}' % i for i in range(lo, hi)],
                            [b"default\0pod-%d\0" % i for i in range(lo, hi)])
        elif dim == DIM_CONTAINER:
            for lo in range(0, n_pods, step):
                hi = min(n_pods, lo + step)
                blocks = [b'{container="container-%d",namespace="default",pod="pod-%d"}' % (j, i)
                          for i in range(lo, hi) for j in range(ncont[i])]
                keys = [b"container-%d\0default\0pod-%d\0" % (j, i) for i in range(lo, hi) for j in range(ncont[i])]
                ex.set_rows(g, int(ex.cptr[lo]), blocks, keys)
    for i in range(0, n_pods, max(1, n_pods // 50)):  # the native renderer agrees
        pod = copy.deepcopy(pvars[int(pidx[i])])
        pod["metadata"]["name"] = f"pod-{i}"
        for g, (dim, _) in enumerate(ex.groups):
            if dim == DIM_POD:
                assert mp.native.labels_render(g, None, pod)[0] == b'{namespace="default",pod="pod-%d"}' % i
            elif dim == DIM_CONTAINER:
                assert mp.native.labels_render(g, None, pod, int(ncont[i]) - 1) == (
                    b'{container="container-%d",namespace="default",pod="pod-%d"}' % (ncont[i] - 1, i),
                    b"container-%d\0default\0pod-%d\0" % (ncont[i] - 1, i))


def timed(ex, pods, t, dt, chunks, scrapes, warmup):
    """Medians over `scrapes` all-node scrapes (the chunks' times summed per scrape)."""
    rows = []
    total_bytes = 0
    for k in range(warmup + scrapes):
        pods.usage(t)
        ms = np.zeros(4)
        nbytes = 0
        for first, n in chunks:
            ex.enqueue(t, first, n)
            nbytes += ex.result()
            ms += np.array(ex.elapsed_ms())
        if k >= warmup:
            rows.append(ms)
            total_bytes = nbytes
        t += dt
    med = np.median(np.array(rows), axis=0)
    lo, hi = np.min(np.array(rows), axis=0), np.max(np.array(rows), axis=0)
    kern = float(med[1] + med[2] + med[3])
    return {"scrape_us": round(float(med[0]) * 1e3, 1), "lengths_us": round(float(med[1]) * 1e3, 1),
            "scan_us": round(float(med[2]) * 1e3, 1), "write_us": round(float(med[3]) * 1e3, 1),
            "write_us_min_max": [round(float(lo[3]) * 1e3, 1), round(float(hi[3]) * 1e3, 1)],
            "kernels_us": round(kern * 1e3, 1), "bytes": int(total_bytes),
            "write_GBps": round(total_bytes / (float(med[3]) * 1e-3) / 1e9, 1),
            "kernels_GBps": round(total_bytes / (kern * 1e-3) / 1e9, 1), "scrapes": scrapes, "warmup": warmup}, t


def _label_calls(ex, ncont, slots, version):
    """The kwk_expo_set_labels arguments (ctypes, built outside the timed region) that rename pod
    `i` of `slots` to pod-<i>-v<version>: one call per pod for the pod group and one for its
    containers' rows."""
    import ctypes as C
    from kwok_amd.host.expo import DIM_CONTAINER, DIM_POD
    calls = []
    one = (C.c_uint32 * 2)
    for g, (dim, _) in enumerate(ex.groups):
        if dim == DIM_POD:
            for i in slots:
                name = b"pod-%d-v%s" % (i, version)
                blk, key = b'{namespace="default",pod="%s"}' % name, b"default\0%s\0" % name
                calls.append((ex.h, g, int(i), 1, one(0, len(blk)), blk, one(0, len(key)), key))
        elif dim == DIM_CONTAINER:
            for i in slots:
                name = b"pod-%d-v%s" % (i, version)
                k = int(ncont[i])
                blks = [b'{container="container-%d",namespace="default",pod="%s"}' % (j, name) for j in range(k)]
                keys = [b"container-%d\0default\0%s\0" % (j, name) for j in range(k)]
                bo, ko = (C.c_uint32 * (k + 1))(), (C.c_uint32 * (k + 1))()
                for j in range(k):
                    bo[j + 1] = bo[j] + len(blks[j])
                    ko[j + 1] = ko[j] + len(keys[j])
                calls.append((ex.h, g, int(ex.cptr[i]), k, bo, b"".join(blks), ko, b"".join(keys)))
    return calls


def churn(args):
    """--churn: the cost of bringing relabelled pods' rows up to date, incremental
    (kwk_expo_commit_rows) against full (kwk_expo_commit), at 0.1 %, 1 % and 10 % of the pods."""
    from kwok_amd.host.expo import DIM_NODE, Exposition, lib
    pods, mp, pvars, pidx, node_ptr, t = build_rig(args.nodes, args.pods, args.seed, None)
    ex = Exposition(pods, mp.native)
    upload_labels(ex, mp, pvars, pidx, args.pods)
    ex.commit()
    L = lib()
    ncont = np.array([len(v["spec"]["containers"]) for v in pvars])[pidx]
    rng = np.random.default_rng(args.seed)
    reps, warm = 5, 1
    res = {"workload": f"{args.nodes} nodes / {args.pods} pods (C4 shape), metrics-resource.yaml; every relabelled pod's "
                       "pod row and container rows are set (one kwk_expo_set_labels call per pod and group) and committed",
           "method": f"medians of {reps} after {warm} warm-up, in one process, the incremental and the full leg alternating; every "
                     "round renames the same pods to a longer name than the round before, so every row outgrows its slot and "
                     "is appended (the arenas grow when the tail fills: the dearest case of the incremental path); "
                     "host_ms = wall time of the calls (kwk_expo_commit_rows only enqueues), kernels by HIP events, "
                     "done_ms = wall time until the stream has finished the commit",
           "fractions": {}}

    def set_all(calls):
        for c in calls:
            if L.kwk_expo_set_labels(*c) != 0:
                raise SystemExit("kwk_expo_set_labels: " + L.kwk_expo_last_error(ex.h).decode())

    version = 0
    for frac in (0.001, 0.01, 0.1):
        slots = np.sort(rng.choice(args.pods, size=max(1, int(args.pods * frac)), replace=False))
        rows = {"set_labels_ms": [], "commit_rows_host_ms": [], "scatter_us": [], "sort_us": [], "commit_rows_done_ms": [],
                "full_set_labels_ms": [], "full_commit_ms": []}
        for k in range(warm + reps):
            version += 1
            calls = _label_calls(ex, ncont, slots, b"%s" % (b"y" * version))
            t0 = time.perf_counter()
            set_all(calls)
            t1 = time.perf_counter()
            ex.commit_rows()
            t2 = time.perf_counter()
            scatter_ms, sort_ms = ex.commit_rows_elapsed_ms()  # waits for the kernels
            t3 = time.perf_counter()
            version += 1
            calls = _label_calls(ex, ncont, slots, b"%s" % (b"y" * version))
            t4 = time.perf_counter()
            set_all(calls)
            t5 = time.perf_counter()
            ex.commit()
            t6 = time.perf_counter()
            if k >= warm:
                for name, v in (("set_labels_ms", (t1 - t0) * 1e3), ("commit_rows_host_ms", (t2 - t1) * 1e3),
                                ("scatter_us", scatter_ms * 1e3), ("sort_us", sort_ms * 1e3),
                                ("commit_rows_done_ms", (t3 - t1) * 1e3), ("full_set_labels_ms", (t5 - t4) * 1e3),
                                ("full_commit_ms", (t6 - t5) * 1e3)):
                    rows[name].append(v)
        med = {k: round(float(np.median(v)), 3) for k, v in rows.items()}
        med["pods"] = int(len(slots))
        med["rows"] = int(len(slots) + ncont[slots].sum())
        med["nodes_touched"] = int(len(np.unique(np.searchsorted(node_ptr, slots, side="right"))))
        med["incremental_ms"] = round(med["set_labels_ms"] + med["commit_rows_done_ms"], 3)
        med["full_ms"] = round(med["full_set_labels_ms"] + med["full_commit_ms"], 3)
        med["full_over_incremental"] = round(med["full_ms"] / med["incremental_ms"], 1)
        res["fractions"]["%g%%" % (frac * 100)] = med
    # the two paths agree: the last fraction once more, incremental, against a full commit of the same state
    version += 1
    set_all(_label_calls(ex, ncont, slots, b"%s" % (b"y" * version)))
    ex.commit_rows()
    sample = [int(j) for j in np.linspace(0, args.nodes - 1, num=min(args.sample, args.nodes)).astype(int)]
    pods.usage(t)
    groups = [g for g, (dim, _) in enumerate(ex.groups) if dim != DIM_NODE]
    perms = [ex.read_perm(g).copy() for g in groups]
    texts = [ex.scrape(t, j, 1)[0] for j in sample]
    ex.commit()
    equal = all(np.array_equal(p, ex.read_perm(g)) for p, g in zip(perms, groups)) and \
        texts == [ex.scrape(t, j, 1)[0] for j in sample]
    res["equal_to_full_commit"] = {"permutations": len(groups), "sampled_nodes_text": len(sample), "equal": bool(equal)}
    assert equal, "the incremental commit differs from the full commit"
    ex.close()
    pods.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=10_000)
    ap.add_argument("--pods", type=int, default=1_000_000)
    ap.add_argument("--chunk", type=int, default=0, help="nodes per scrape call (0: all in one)")
    ap.add_argument("--scrapes", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sample", type=int, default=16, help="nodes of the Python scrape + exposition comparison")
    ap.add_argument("--seed", type=int, default=0x6B776F6B)
    ap.add_argument("--out", default=None, help="default profiles/r7/expo_bench.json (--hist: profiles/r8/expo_hist_bench.json)")
    ap.add_argument("--tag", default=None, help="default c4 (--hist: c4_hist)")
    ap.add_argument("--native-labels", action="store_true",
                    help="render every label row with kwk_metric_labels_render (Exposition.set_pods): slow from Python")
    ap.add_argument("--hist", action="store_true",
                    help="the histogram leg (and the scalar-only CR in the same process): see the module docstring")
    ap.add_argument("--churn", action="store_true",
                    help="the label-commit leg: kwk_expo_commit_rows against kwk_expo_commit (see the module docstring)")
    args = ap.parse_args()
    args.out = args.out or os.path.join(ROOT, "profiles", *(("r10", "expo_commit_bench.json") if args.churn else
                                                           ("r8", "expo_hist_bench.json") if args.hist else
                                                           ("r7", "expo_bench.json")))
    args.tag = args.tag or ("churn_c4" if args.churn else "c4_hist" if args.hist else "c4")
    if args.churn:
        res = churn(args)
    elif args.hist:
        scalar = leg(args, None)
        res = leg(args, hist_cr_text())
        res["scalar_same_run"] = scalar
        for w in [k for k in res if k.startswith("width_")]:
            res[w]["write_GBps_over_scalar"] = round(res[w]["write_GBps"] / scalar[w]["write_GBps"], 3)
    else:
        res = leg(args, None)
    out = {}
    if os.path.exists(args.out):
        out = json.load(open(args.out))
    out[args.tag] = res
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({args.tag: res}))


def leg(args, cr_text):
    """One CR (None: the shipped one) measured end to end -> its result section."""
    from kwok_amd.host.expo import Exposition
    t_setup = time.perf_counter()
    pods, mp, pvars, pidx, node_ptr, t = build_rig(args.nodes, args.pods, args.seed, cr_text)
    ex = Exposition(pods, mp.native)
    if args.native_labels:
        upload_labels_native(ex, pvars, pidx, args.pods)
    else:
        upload_labels(ex, mp, pvars, pidx, args.pods)
    t_commit = time.perf_counter()
    ex.commit()
    commit_s = time.perf_counter() - t_commit
    setup_s = time.perf_counter() - t_setup
    dt = 10 * 10**9
    chunk = args.chunk or args.nodes
    chunks = [(f, min(chunk, args.nodes - f)) for f in range(0, args.nodes, chunk)]
    # the reservation: the largest chunk's text, found by the KWK_ECAP protocol
    pods.usage(t)
    need = 0
    for first, n in chunks:
        ex.enqueue(t, first, n)
        try:
            need = max(need, ex.result())
        except Exception:
            need = max(need, ex.needed)
    ex.reserve(need + need // 16)
    t += dt
    cr_name = "metrics-resource.yaml + a pod and a container histogram (5 visible buckets)" if cr_text else \
        "metrics-resource.yaml"
    res = {"workload": f"{args.nodes} nodes / {args.pods} pods (C4 shape), {cr_name}, "
                       f"{len(chunks)} scrape call(s) of {chunk} nodes", "reserved_bytes": need + need // 16,
           "setup_s": round(setup_s, 1), "commit_s": round(commit_s, 2)}
    ppn = args.pods // max(1, args.nodes)
    auto = 256 if ppn > 256 else 64  # kwk_expo_set_width(0)'s choice (kWidePods)
    for width in (auto, 64 if auto == 256 else 256):
        ex.set_width(width)
        r, t = timed(ex, pods, t, dt, chunks, args.scrapes, args.warmup)
        res["width_%d%s" % (width, "_default" if width == auto else "")] = r
    ex.set_width(0)
    # the Python path of the parent commit on a sample of nodes; the device text of those nodes
    sample = [int(j) for j in np.linspace(0, args.nodes - 1, num=min(args.sample, args.nodes)).astype(int)]
    pods.usage(t)
    py_s, equal = 0.0, 0
    for j in sample:
        lo, hi = int(node_ptr[j]), int(node_ptr[j + 1])
        objs = []
        for i in range(lo, hi):
            o = copy.deepcopy(pvars[int(pidx[i])])
            o["metadata"]["name"] = f"pod-{i}"
            objs.append(o)
        node = {"metadata": {"name": f"node-{j}"}}
        t0 = time.perf_counter()
        text = mp.exposition(mp.scrape(pods, t, j, [node], objs, node_ptr)).encode()
        py_s += time.perf_counter() - t0
        equal += int(ex.scrape(t, j, 1)[0] == text)
    res["python_scrape_exposition"] = {
        "sampled_nodes": len(sample), "ms_per_node": round(py_s / len(sample) * 1e3, 2),
        "extrapolated_s_all_nodes": round(py_s / len(sample) * args.nodes, 1),
        "note": "an extrapolation: the sampled nodes' mean time x the node count (one Python process)",
        "device_text_equal_nodes": equal}
    assert equal == len(sample), "device text differs from the Python exposition"
    ex.close()
    pods.close()
    return res


if __name__ == "__main__":
    main()

"""Usage expressions that read the clock, evaluated by the usage kernel at every scrape
(kwk_usage_config_dyn): node sums, the cluster total, the node / pod / container integrators and
the readers, against the restatement by hand of tests/usage_dyn_util.py (1e-6 relative, the
project's usage tolerance).  The shapes are the usage kernels' own edges: 16 pods per lane, 1024
slots per wave row, a one-row chunk of 1016 pods, 128 nodes per chunk."""
import functools
import os

import numpy as np
import pytest

from kwok_amd import workload as W
from kwok_amd.host import abi, cel
from kwok_amd.host.usage import UsageProgram, load_usage_yaml, usage_columns, usage_columns_dyn
from oracle import usage_ref
from tests.usage_dyn_util import ANN, EXPR, created_ns, restate, usage_doc

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(__file__)), "kwok_amd", "metrics", "usage-from-annotation.yaml")
REL_TOL = 1e-6
T0 = 1_700_000_000 * 10**9
SCRAPES = [T0, T0 + 2_500_000_123, T0 + 9_500_000_124]   # uneven intervals
I64_MIN = np.iinfo(np.int64).min

# which fixture a pod's namespace selects: {namespace: (cpu, memory)}; "default" is all constants
BY_NS = {"ramp": ("capped", "annotated"), "age": ("node_age", "base_ramp"), "unix": ("unix", "ramp"),
         "default": ("100m", "64Mi")}


def _docs(by_ns=BY_NS):
    val = lambda v: EXPR.get(v, v)  # noqa: E731
    return "\n---\n".join(usage_doc(ns, val(c), val(m), namespaces=[ns]) for ns, (c, m) in by_ns.items())


def _stamp(ns):
    import datetime
    return datetime.datetime.fromtimestamp(ns // 10**9, datetime.timezone.utc).strftime("%Y-%m-%dT%H:%M:%SZ")


def _cluster(sizes, ns_of, containers=2, seed=11):
    """Pods over nodes of the given sizes, node-sorted; pod i is in namespace ns_of(i, node), was
    created up to 2000 s before T0 (so the 600 s cap is on both sides), every 50th has no
    creationTimestamp and every 50th is created after the first scrape; nodes alike."""
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    n = int(ptr[-1])
    cl = W.make_cluster("C4", len(sizes), n, seed=seed)
    pods = cl.pods.materialize()
    nodes = []
    for j in range(len(sizes)):
        md = {"name": f"node-{j}"}
        if j % 9 != 4:
            md["creationTimestamp"] = _stamp(T0 - (j * 7919 % 500_000) * 10**9)
        nodes.append({"metadata": md})
    node_of = np.repeat(np.arange(len(sizes)), sizes)
    for i, p in enumerate(pods):
        md = p["metadata"]
        md["namespace"] = ns_of(i, int(node_of[i]))
        md.pop("annotations", None)
        if i % 4 == 1:
            md["annotations"] = {ANN: f"{1 + i % 3}Mi"}
        if i % 50 == 9:
            md["creationTimestamp"] = _stamp(T0 + 100 * 10**9)
        elif i % 50 != 7:
            md["creationTimestamp"] = _stamp(T0 - (i * 37 % 2000) * 10**9)
        p["spec"]["nodeName"] = f"node-{node_of[i]}"
        p["spec"]["containers"] = [{"name": f"container-{c}", "image": "busybox"} for c in range(containers)]
    return cl, pods, nodes, ptr, node_of


def _engine(cl, pods, nodes, ptr, cols_dyn, state="auto", pods_out=True, inputs=True):
    from kwok_amd.host.compiler import KindProgram
    from kwok_amd.host.engine import Engine, Ingest
    from kwok_amd.host.stages import load_stage_files

    kp = KindProgram(load_stage_files(*cl.pod_stage_files))
    kp.explore(pods)
    ing = Ingest(kp)
    cols = ing.columns(pods)
    eng = Engine(kp, capacity=len(pods), state=state)
    try:
        eng.load_stages()
        eng.load(*cols, ing.record_array())
        keys, cv, mv, mx, ck, cp, mp, ops = cols_dyn
        eng.usage_config(ptr, keys, cv, mv, mx, ck, cpu_progs=cp, mem_progs=mp, ops=ops)
        if pods_out:
            eng.usage_pods(True)
        if inputs:
            _inputs(eng, pods, nodes)
    except Exception:
        eng.close()
        raise
    return eng, cols


def _inputs(eng, pods, nodes):
    pc = np.array([I64_MIN if created_ns(p) is None else created_ns(p) for p in pods], dtype=np.int64)
    nc = np.array([I64_MIN if created_ns(n) is None else created_ns(n) for n in nodes], dtype=np.int64)
    eng.metrics_inputs(pc, nc, np.zeros(len(nodes)), cel.zero_time_unix_second())


class Restated:
    """The reference's outputs scrape by scrape: container values by the fixture the pod's
    namespace (or `fixture_of`) selects, pod and node sums in spec / slot order, the integrators
    of usage_ref.Cumulative keyed per container and per node."""

    def __init__(self, pods, nodes, ptr, node_of, fixture_of):
        self.pods, self.nodes, self.ptr, self.node_of, self.fixture_of = pods, nodes, ptr, node_of, fixture_of
        self.cum = usage_ref.Cumulative()

    def scrape(self, now, alive):
        n, ptr = len(self.pods), self.ptr
        cont, pod, node = [], np.zeros((n, 4)), np.zeros((len(ptr) - 1, 4))
        for i, p in enumerate(self.pods):
            nd = self.nodes[self.node_of[i]]
            for c in p["spec"]["containers"]:
                if not alive[i]:
                    cont.append((0.0, 0.0, 0.0, 0.0))
                    continue
                fc, fm = self.fixture_of(i, c["name"])
                vc, vm = restate(fc, now, p, nd), restate(fm, now, p, nd)
                cc = self.cum.advance((i, c["name"], "cpu"), vc, now)
                cm = self.cum.advance((i, c["name"], "memory"), vm, now)
                cont.append((vc, vm, cc, cm))
                pod[i] += (vc, vm, cc, cm)
        for j in range(len(ptr) - 1):
            v = pod[ptr[j]:ptr[j + 1], :2].sum(axis=0) if ptr[j + 1] > ptr[j] else np.zeros(2)
            node[j] = (v[0], v[1], self.cum.advance((j, "cpu"), v[0], now), self.cum.advance((j, "memory"), v[1], now))
        return np.array(cont).reshape(-1, 4), pod, node


def _check(eng, want, tag, containers=True):
    cont, pod, node = want
    got_node, got_total = eng.usage_read()
    for name, g, w in (("node", got_node, node), ("pod", eng.usage_read_pods(), pod)) + \
            ((("container", eng.usage_read_containers(), cont),) if containers else ()):
        err = np.abs(g - w) / np.maximum(np.abs(w), 1e-300)
        print(tag, name, "max relative error", float(np.max(np.where(w == 0, np.abs(g), err), initial=0.0)))
        np.testing.assert_allclose(g, w, rtol=REL_TOL, atol=1e-9, err_msg=f"{tag}: {name}")
    np.testing.assert_allclose(got_total, node[:, :2].sum(axis=0), rtol=REL_TOL, err_msg=f"{tag}: cluster")


# ------------------------------------------------------------------ the kernels' edges, every state format
SIZES = [0, 1, 15, 16, 17, 1016, 1017, 1100] + [20] * 140 + [15]   # 5997 pods, 149 nodes


def _edge_ns(i, node):
    if node in (6, 7):  # 2117 pods in a row with constants only: wave rows without a program id
        return "default"
    return ("ramp", "age", "default", "unix")[i % 4]


@functools.lru_cache(maxsize=None)
def _edge_case():
    assert sum(SIZES) == 5997
    cl, pods, nodes, ptr, node_of = _cluster(SIZES, _edge_ns)
    prog = UsageProgram(*load_usage_yaml(_docs()))
    cols = usage_columns_dyn(prog, pods, {n["metadata"]["name"]: n for n in nodes})
    assert len(cols[5]) and len(cols[6]) and 0.1 in cols[1]   # programs and constants, both resources
    alive = np.ones(len(pods), dtype=bool)
    alive[np.arange(3, len(pods), 11)] = False
    ref = Restated(pods, nodes, ptr, node_of, lambda i, c: BY_NS[pods[i]["metadata"]["namespace"]])
    return cl, pods, nodes, ptr, cols, alive, [ref.scrape(t, alive) for t in SCRAPES]


@pytest.mark.parametrize("state", ["auto", "u32", "dw", "wide"])
def test_gpu_dynamic_usage_edges(state):
    cl, pods, nodes, ptr, cols, alive, want = _edge_case()
    eng, _ = _engine(cl, pods, nodes, ptr, cols, state=state)
    try:
        eng.delete(np.flatnonzero(~alive))
        for k, t in enumerate(SCRAPES):
            eng.usage(t)
            _check(eng, want[k], f"{state} scrape {k}")
            if k == 0:  # the first scrape only records the time
                assert np.all(eng.usage_read()[0][:, 2:] == 0) and np.all(eng.usage_read_pods()[:, 2:] == 0)
        node = eng.usage_read()[0]
        assert np.any(node[:, 2] != 0) and np.any(node[:, 3] != 0)
        # the values moved with the clock
        assert not np.allclose(want[1][2][:, :2], want[2][2][:, :2], rtol=1e-3)
    finally:
        eng.close()


# ------------------------------------------------------------------ mixed pods, deletion and re-creation
def _small(fixture_docs, ns_of=lambda i, node: "default", containers=2, sizes=(0, 40, 1, 63, 64, 65, 67)):
    cl, pods, nodes, ptr, node_of = _cluster(list(sizes), ns_of, containers=containers, seed=5)
    prog = UsageProgram(*load_usage_yaml(fixture_docs))
    cols = usage_columns_dyn(prog, pods, {n["metadata"]["name"]: n for n in nodes})
    return cl, pods, nodes, ptr, node_of, cols


MIXED = "\n---\n".join([usage_doc("first", EXPR["capped"], EXPR["annotated"], containers=["container-0"]),
                        usage_doc("second", "250m", EXPR["base_ramp"], containers=["container-1"]),
                        usage_doc("others", EXPR["node_age"], "8Mi")])
MIXED_FIXTURES = {"container-0": ("capped", "annotated"), "container-1": ("250m", "base_ramp"),
                  "container-2": ("node_age", "8Mi")}


def test_gpu_mixed_pods_killed_and_recreated():
    """Containers with different programs (kwk_usage_mixed, kwk_usage_read_containers); pods
    deleted between scrapes read 0 while dead and continue their integrators when re-created."""
    cl, pods, nodes, ptr, node_of, cols = _small(MIXED, containers=3)
    assert len(cols[3]) and np.all(cols[0] >> 28 == 0)   # every pod is mixed
    eng, ecols = _engine(cl, pods, nodes, ptr, cols)
    try:
        ref = Restated(pods, nodes, ptr, node_of, lambda i, c: MIXED_FIXTURES[c])
        alive = np.ones(len(pods), dtype=bool)
        gone = np.arange(0, len(pods), 5)
        t = T0
        for k in range(6):
            if k == 2:
                eng.delete(gone)
                alive[gone] = False
            if k == 4:
                hot, dels, rec, cls = ecols
                eng.upsert(gone, hot[gone], dels[gone], rec[gone], cls[gone])
                alive[gone] = True
            eng.usage(t)
            want = ref.scrape(t, alive)
            _check(eng, want, f"mixed scrape {k}")
            if k == 3:
                assert np.all(eng.usage_read_pods()[gone] == 0)
            if k == 5:  # continued: more than the two intervals since the re-creation alone would give
                i = int(gone[1])
                assert want[1][i, 2] > 0 and ref.cum.last[(i, "container-1", "cpu")] == t
            t += 1_000_000_000 + 37_000_001 * k
    finally:
        eng.close()


def test_gpu_uniform_pods_killed_and_recreated():
    cl, pods, nodes, ptr, node_of, cols = _small(_docs(), ns_of=lambda i, node: ("ramp", "age", "default")[i % 3])
    assert len(cols[3]) == 0
    eng, ecols = _engine(cl, pods, nodes, ptr, cols)
    try:
        ref = Restated(pods, nodes, ptr, node_of, lambda i, c: BY_NS[pods[i]["metadata"]["namespace"]])
        alive = np.ones(len(pods), dtype=bool)
        gone = np.arange(1, len(pods), 4)
        t = T0
        for k in range(5):
            if k == 1:
                eng.delete(gone)
                alive[gone] = False
            if k == 3:
                hot, dels, rec, cls = ecols
                eng.upsert(gone, hot[gone], dels[gone], rec[gone], cls[gone])
                alive[gone] = True
            eng.usage(t)
            _check(eng, ref.scrape(t, alive), f"uniform scrape {k}")
            t += 3_000_000_007 + 11_000_000 * k
    finally:
        eng.close()


# ------------------------------------------------------------------ tables beyond the LDS staging
CPU_ANN = "kwok.x-k8s.io/usage-cpu"
CPU_FROM_ANN = f'Quantity(pod.metadata.annotations["{CPU_ANN}"])'


def test_gpu_600_programs_beyond_lds_staging():
    """600 distinct memory programs (3600 ops) and 600 cpu constants: neither the value table
    (512), the program table (256) nor the ops (256) fit their LDS copies."""
    sizes = [300, 0, 700, 200]
    cl, pods, nodes, ptr, node_of = _cluster(sizes, lambda i, node: "default", containers=1)
    for i, p in enumerate(pods):
        p["metadata"]["annotations"] = {ANN: f"{1 + i % 600}Ki", CPU_ANN: f"{1 + i % 600}m"}
    doc = usage_doc("all", "CPU", EXPR["annotated"]).replace("{value: CPU}", "{expression: '" + CPU_FROM_ANN + "'}")
    cols = usage_columns_dyn(UsageProgram(*load_usage_yaml(doc)), pods, {})
    assert len(cols[1]) == 600 and len(cols[6]) == 600 and len(cols[7]) == 3600
    eng, _ = _engine(cl, pods, nodes, ptr, cols)
    try:
        def fixture(i, c):
            return pods[i]["metadata"]["annotations"][CPU_ANN], "annotated"
        ref = Restated(pods, nodes, ptr, node_of, fixture)
        alive = np.ones(len(pods), dtype=bool)
        for k, t in enumerate(SCRAPES):
            eng.usage(t)
            _check(eng, ref.scrape(t, alive), f"600 programs scrape {k}")
    finally:
        eng.close()


# ------------------------------------------------------------------ no programs: kwk_usage_config, bit for bit
@pytest.mark.parametrize("pods_out", [False, True])
def test_gpu_config_dyn_without_programs_is_usage_config(pods_out):
    cl = W.make_cluster("C4", 40, 6000, seed=17)
    pods = cl.pods.materialize()
    prog = UsageProgram(*load_usage_yaml(open(GOLDEN).read()))
    static = usage_columns(prog, pods)
    dyn = usage_columns_dyn(prog, pods)
    assert len(dyn[5]) == 0 and len(dyn[6]) == 0 and len(dyn[7]) == 0
    nodes = [{"metadata": {"name": f"node-{j}"}} for j in range(len(cl.node_ptr) - 1)]
    outs = []
    for cols in (static + (None, None, None), dyn):
        eng, _ = _engine(cl, pods, nodes, cl.node_ptr, cols, pods_out=pods_out, inputs=False)
        try:
            eng.delete(np.arange(3, len(pods), 11))
            for t in SCRAPES:
                eng.usage(t)
            node, total = eng.usage_read()
            n = eng.aggregate([0, 1], SCRAPES[-1] + 10**9, usage=True)
            agg = eng.aggregate_read(n)
            outs.append((node, total, agg) + ((eng.usage_read_pods(), eng.usage_read_containers()) if pods_out else ()))
        finally:
            eng.close()
    for a, b in zip(*outs):
        assert a.tobytes() == b.tobytes()


# ------------------------------------------------------------------ the readers see the evaluated values
def test_gpu_metrics_and_aggregate_see_dynamic_values():
    cl, pods, nodes, ptr, node_of, cols = _small(_docs(), ns_of=lambda i, node: ("ramp", "age", "default")[i % 3])
    eng, _ = _engine(cl, pods, nodes, ptr, cols)
    try:
        eng.metrics_load([("pod", cel.lower('pod.Usage("memory")', "pod")),
                          ("container", cel.lower('pod.Usage("memory", container.name)', "container")),
                          ("container", cel.lower('pod.Usage("cpu", container.name) * 1000.0', "container"))])
        ref = Restated(pods, nodes, ptr, node_of, lambda i, c: BY_NS[pods[i]["metadata"]["namespace"]])
        alive = np.ones(len(pods), dtype=bool)
        n_nodes = len(ptr) - 1
        for t in SCRAPES[:2]:
            eng.usage(t)
            cont, pod, node = ref.scrape(t, alive)
            got = eng.metrics_eval(t, 0, n_nodes)
            n, nc = len(pods), len(cont)
            assert len(got) == n + 2 * nc
            np.testing.assert_allclose(got[:n], pod[:, 1], rtol=REL_TOL)
            np.testing.assert_allclose(got[n:n + nc], cont[:, 1], rtol=REL_TOL)
            np.testing.assert_allclose(got[n + nc:], cont[:, 0] * 1000.0, rtol=REL_TOL)
        # kwk_aggregate runs the usage pass itself, at its own clock, through the unfused counts
        t = SCRAPES[2]
        cnt = eng.aggregate([0], t, usage=True)
        agg = eng.aggregate_read(cnt)
        cont, pod, node = ref.scrape(t, alive)
        np.testing.assert_allclose(agg[-2:], node[:, :2].sum(axis=0), rtol=REL_TOL)
        assert agg[-3] == len(pods) == int(eng.count([0])[0])
        assert not np.allclose(agg[-2:], ref.scrape(t + 60 * 10**9, alive)[2][:, :2].sum(axis=0), rtol=1e-4)
    finally:
        eng.close()


# ------------------------------------------------------------------ errors
def test_gpu_usage_needs_metrics_inputs():
    cl, pods, nodes, ptr, node_of, cols = _small(_docs(), ns_of=lambda i, node: "ramp")
    eng, _ = _engine(cl, pods, nodes, ptr, cols, inputs=False)
    try:
        with pytest.raises(abi.EngineError, match="kwk_metrics_inputs"):
            eng.usage(T0)
        assert abi.lib().kwk_usage(eng.h, T0) == abi.KWK_ESTATE
        _inputs(eng, pods, nodes)
        eng.usage(T0)
        # a new configuration needs its own inputs again
        keys, cv, mv, mx, ck, cp, mp, ops = cols
        eng.usage_config(ptr, keys, cv, mv, mx, ck, cpu_progs=cp, mem_progs=mp, ops=ops)
        eng.usage(T0)   # same shape: the inputs still fit
    finally:
        eng.close()


def _ops(*ops):
    a = np.zeros(len(ops), dtype=abi.USAGE_OP_DTYPE)
    for i, (op, x) in enumerate(ops):
        a[i] = (op, int(x), 0.0) if op == cel.OP_LOAD else (op, 0, float(x))
    return a


@pytest.mark.parametrize("case,word", [
    ("bad-op", "usage program op"), ("bad-load", "loads input 5"), ("deep", "deeper than 8"),
    ("two-values", "leaves one value"), ("underflow", "underflow"), ("range", "ops range"), ("id", "value id out of range"),
    ("select-underflow", "underflow"),
])
def test_gpu_config_dyn_rejects(case, word):
    cl, pods, nodes, ptr, node_of, cols = _small(_docs(), ns_of=lambda i, node: "ramp")
    eng, _ = _engine(cl, pods, nodes, ptr, cols)
    try:
        Cn, L = cel.OP_CONST, cel.OP_LOAD
        ops = {"bad-op": _ops((Cn, 1.0), (14, 0)), "bad-load": _ops((L, cel.IN_POD_CPU)),
               "deep": _ops(*([(Cn, 1.0)] * 9 + [(cel.OP_ADD, 0)] * 8)), "two-values": _ops((Cn, 1.0), (Cn, 2.0)),
               "underflow": _ops((Cn, 1.0), (cel.OP_LT, 0)), "range": _ops((Cn, 1.0)), "id": _ops((Cn, 1.0)),
               "select-underflow": _ops((Cn, 1.0), (Cn, 1.0), (cel.OP_SELECT, 0))}[case]
        progs = np.array([[0, len(ops) + (1 if case == "range" else 0)]], dtype=np.uint32)
        keys = np.full(len(pods), (1 << 28) | (2 if case == "id" else 1), dtype=np.uint32)   # cpu id 1 = program 0
        one = np.zeros(1)
        L_ = abi.lib()
        st = L_.kwk_usage_config_dyn(eng.h, len(ptr) - 1, abi.ptr(ptr), abi.ptr(keys), 1, abi.ptr(one), 1, abi.ptr(progs),
                                     1, abi.ptr(one), 0, None, len(ops), abi.ptr(ops))
        assert st == abi.KWK_EINVAL
        msg = L_.kwk_last_error(eng.h).decode()
        assert word in msg, msg
        # refused before anything changed: the earlier configuration still runs
        assert L_.kwk_usage(eng.h, T0) == abi.KWK_OK
    finally:
        eng.close()

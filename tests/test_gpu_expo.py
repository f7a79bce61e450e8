"""Device metric exposition (kwok_expo.h) on the GPU: every node's text equals
MetricsProgram.exposition(MetricsProgram.scrape(...)) for that node alone, byte for byte — the
values are the same doubles (one engine state), so the comparison is == on bytes."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import yaml

from kwok_amd import workload as W
from kwok_amd.host import abi, cel
from kwok_amd.host.metrics import MetricsProgram
from kwok_amd.host.usage import UsageProgram, load_usage_yaml, usage_columns
from tests.test_f64fmt import EDGES, EXPONENT_NEIGHBOURS

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
USAGE = os.path.join(os.path.dirname(HERE), "kwok_amd", "metrics", "usage-from-annotation.yaml")
METRICS = os.path.join(os.path.dirname(HERE), "kwok_amd", "metrics", "metrics-resource.yaml")
T0 = 1_700_000_000 * 10**9


def _ns(ts):
    return cel._parse_time(ts)


class Rig:
    """A pods engine with usage, the Metric CR loaded and an Exposition over it."""

    def __init__(self, cl, pods, nodes, node_ptr, usage_text=None, cr_text=None, label_pods=None):
        from kwok_amd.host.compiler import KindProgram
        from kwok_amd.host.engine import Engine, Ingest
        from kwok_amd.host.expo import Exposition
        from kwok_amd.host.stages import load_stage_files
        self.pods, self.nodes = pods, nodes
        self.node_ptr = np.ascontiguousarray(node_ptr, dtype=np.uint32)
        cols = usage_columns(UsageProgram(*load_usage_yaml(usage_text or open(USAGE).read())), pods)
        kp = KindProgram(load_stage_files(*cl.pod_stage_files))
        kp.explore(pods)
        ing = Ingest(kp)
        self.eng = Engine(kp, capacity=len(pods))
        try:
            self.eng.load_stages()
            self.eng.load(*ing.columns(pods), ing.record_array())
            self.eng.usage_config(self.node_ptr, *cols)
            self.eng.usage_pods(True)
            self.mp = MetricsProgram.from_native(cr_text or open(METRICS).read())
            self.mp.load(self.eng)
            created = np.array([_ns(p["metadata"]["creationTimestamp"]) if "creationTimestamp" in p["metadata"]
                                else np.iinfo(np.int64).min for p in pods], dtype=np.int64)
            zero_unix = float(cel.wrap_int64(cel.GO_ZERO_TIME.ns)) / 1e9
            self.eng.metrics_inputs(created, np.full(len(nodes), np.iinfo(np.int64).min, dtype=np.int64),
                                    np.zeros(len(nodes)), zero_unix)
            self.alive = np.ones(len(pods), dtype=bool)
            self.ex = Exposition(self.eng, self.mp.native)
            self.ex.set_nodes(nodes)
            self.ex.set_pods(pods if label_pods is None else label_pods, 0, nodes)
            self.ex.commit()
        except Exception:
            self.eng.close()
            raise

    def delete(self, slots):
        self.eng.delete(np.asarray(slots))
        self.alive[slots] = False

    def expected(self, t, j):
        lo, hi = int(self.node_ptr[j]), int(self.node_ptr[j + 1])
        slots = [self.pods[i] if self.alive[i] else None for i in range(lo, hi)]
        dev = self.mp.scrape(self.eng, t, j, [self.nodes[j]], slots, self.node_ptr)
        return self.mp.exposition(dev).encode(), dev

    def close(self):
        self.ex.close()
        self.eng.close()


def _mixed_cluster():
    cl = W.make_cluster("C4", 8, 200, seed=51)
    pods = cl.pods.materialize()
    extra = []
    for i, p in enumerate(pods):
        if i % 2 == 0:
            p["metadata"]["creationTimestamp"] = "2023-11-14T00:00:%02dZ" % (i % 60)
        if i % 4 == 1:  # a namespaced ResourceUsage named like the pod: containers evaluate differently
            extra.append({"apiVersion": "kwok.x-k8s.io/v1alpha1", "kind": "ResourceUsage",
                          "metadata": {"name": p["metadata"]["name"], "namespace": "default"},
                          "spec": {"usages": [{"containers": ["container-1"],
                                               "usage": {"cpu": {"value": "300m"}, "memory": {"value": "32Mi"}}},
                                              {"usage": {"cpu": {"value": "2"},
                                                         "memory": {"expression": 'Quantity("1Gi")'}}}]}})
    text = open(USAGE).read() + "\n---\n" + yaml.safe_dump_all(extra)
    return cl, pods, text


_LABEL = re.compile(r'(\w+)="((?:[^"\\]|\\.)*)"')


def _label_sets(text: bytes):
    """{family: set of label tuples} of a text's series lines."""
    out = {}
    for line in text.decode().split("\n"):
        if not line or line.startswith("#"):
            continue
        head = line.rsplit(" ", 1)[0]
        name, _, rest = head.partition("{")
        out.setdefault(name, set()).add(tuple(_LABEL.findall(rest)))
    return out


def test_mixed_container_cluster_ranges_and_oracle():
    from oracle.metrics_ref import MetricsOracle
    cl, pods, text = _mixed_cluster()
    nodes = cl.nodes.materialize()
    rig = Rig(cl, pods, nodes, cl.node_ptr, usage_text=text)
    oracle = MetricsOracle([d for d in yaml.safe_load_all(text) if d])
    try:
        t = T0
        n = len(nodes)
        for k in range(3):
            if k == 1:
                rig.delete(np.arange(3, len(pods), 11))
            rig.eng.usage(t)
            want = [rig.expected(t, j)[0] for j in range(n)]
            for width in (0, 256):
                rig.ex.set_width(width)
                assert rig.ex.scrape(t, 0, n) == want, (k, width)
            rig.ex.set_width(0)
            for j in range(n):
                assert rig.ex.scrape(t, j, 1) == [want[j]], (k, j)
            assert rig.ex.scrape(t, 3, 3) == want[3:6], k  # non-zero first pod / container of the range
            got = rig.ex.scrape(t, 0, n)
            for j in range(n):
                lo, hi = int(cl.node_ptr[j]), int(cl.node_ptr[j + 1])
                live = [pods[i] for i in range(lo, hi) if rig.alive[i]]
                exp = oracle.scrape(t, nodes[j], live, lambda p: _ns(p["metadata"]["creationTimestamp"])
                                    if "creationTimestamp" in p["metadata"] else None)
                sets = _label_sets(got[j])
                for name, series in exp.items():
                    assert sets.get(name, set()) == {lab for lab, _ in series}, (name, j, k)
            t += 2_500_000_000 + 123_457 * k
    finally:
        rig.close()


def test_skewed_node_ptr():
    """Pods per node [0, 1, 63, 64, 65, 300, 0, 207]: families without series, both sides of the
    wave boundary, a container family larger than one workgroup; both workgroup widths."""
    per = [0, 1, 63, 64, 65, 300, 0, 207]
    cl = W.make_cluster("C4", 8, sum(per), seed=9)
    pods = cl.pods.materialize()
    nodes = cl.nodes.materialize()
    node_ptr = np.concatenate([[0], np.cumsum(per)]).astype(np.uint32)
    rig = Rig(cl, pods, nodes, node_ptr)
    try:
        assert int(rig.ex.cptr[node_ptr[6]] - rig.ex.cptr[node_ptr[5]]) > 256
        t = T0
        for k in range(2):
            if k == 1:
                rig.delete(np.arange(5, len(pods), 13))
            rig.eng.usage(t)
            want = [rig.expected(t, j)[0] for j in range(len(per))]
            assert want[0].count(b"\n") == 16 + 3  # no pods: every family's two header lines, three node series
            for width in (64, 256, 0):
                rig.ex.set_width(width)
                assert rig.ex.scrape(t, 0, len(per)) == want, (k, width)
                assert rig.ex.scrape(t, 5, 3) == want[5:8], (k, width)
            t += 7_000_000_000
    finally:
        rig.close()


def test_sort_order():
    """One node; names a / a-b / a.b / a0 / A / b in two namespaces, loaded in a scrambled order:
    the first label decides before the second, bytewise."""
    names = ["b", "a0", "A", "a.b", "a", "a-b"]
    cl = W.make_cluster("C4", 1, 12, seed=4)
    pods = cl.pods.materialize()
    for i, p in enumerate(pods):
        p["metadata"]["name"] = names[i % 6]
        p["metadata"]["namespace"] = "ns-b" if i % 4 < 2 else "ns"
    nodes = cl.nodes.materialize()
    rig = Rig(cl, pods, nodes, cl.node_ptr)
    try:
        rig.eng.usage(T0)
        want, dev = rig.expected(T0, 0)
        got = rig.ex.scrape(T0, 0, 1)[0]
        assert got == want
        lines = [l for l in got.decode().split("\n") if l.startswith("pod_memory_working_set_bytes{")]
        keys = [tuple(v for _, v in _LABEL.findall(l)) for l in lines]
        assert keys == sorted(keys) and len(keys) == 12 and keys[0][0] == "ns" and keys[-1][0] == "ns-b"
    finally:
        rig.close()


def test_dead_node_and_reservation():
    cl = W.make_cluster("C4", 4, 40, seed=3)
    pods = cl.pods.materialize()
    nodes = cl.nodes.materialize()
    rig = Rig(cl, pods, nodes, cl.node_ptr)
    try:
        lo, hi = int(cl.node_ptr[2]), int(cl.node_ptr[3])
        assert hi > lo
        rig.delete(np.arange(lo, hi))
        rig.eng.usage(T0)
        want = [rig.expected(T0, j)[0] for j in range(4)]
        got = rig.ex.scrape(T0, 0, 4)
        assert got == want
        series = [l for l in got[2].decode().split("\n") if l and not l.startswith("#")]
        assert len(series) == 3 and all(l.startswith(("node_", "scrape_error")) for l in series)
        assert got[2].count(b"# TYPE ") == 8

        # one byte less than the text: KWK_ECAP, and the (fresh, sentinel-filled) buffer is untouched
        from kwok_amd.host.expo import ExpoError, lib
        total = sum(len(x) for x in want)
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        rig.ex.reserve(total - 1)
        off, buf = C.c_void_p(), C.c_void_p()
        assert lib().kwk_expo_device(rig.ex.h, C.byref(off), C.byref(buf)) == 0
        assert hip.hipMemset(buf, 0xA5, total - 1) == 0 and hip.hipDeviceSynchronize() == 0
        rig.ex.enqueue(T0, 0, 4)
        with pytest.raises(ExpoError) as e:
            rig.ex.result()
        assert e.value.status == abi.KWK_ECAP and rig.ex.needed == total
        host = np.zeros(total - 1, dtype=np.uint8)
        assert hip.hipMemcpy(abi.ptr(host), buf, total - 1, 2) == 0  # hipMemcpyDeviceToHost
        assert np.all(host == 0xA5)
        rig.ex.reserve(total)
        rig.ex.enqueue(T0, 0, 4)
        assert rig.ex.result() == total
        off, raw = rig.ex.copy(total)
        assert [raw.tobytes()[int(off[j]):int(off[j + 1])] for j in range(4)] == want
    finally:
        rig.close()


def test_device_formatter_equals_host_build():
    from kwok_amd.host import expo
    cl = W.make_cluster("C4", 1, 2, seed=1)
    rig = Rig(cl, cl.pods.materialize(), cl.nodes.materialize(), cl.node_ptr)
    try:
        rng = np.random.default_rng(77)
        vals = np.concatenate([np.array(EDGES + EXPONENT_NEIGHBOURS + [-x for x in EDGES if x == x]),
                               rng.integers(0, 2**64, size=100_000, dtype=np.uint64).view(np.float64)])
        got = rig.ex.format_values(vals)
        bad = [(float(v), g) for v, g in zip(vals, got) if g != expo.format_f64(float(v))]
        assert not bad, bad[:10]
    finally:
        rig.close()


def test_reference_vectors_gauge_counter():
    """gauge_test.go / counter_test.go's expected text (tests/golden/metric_vectors.json) in every
    node's device text, from the vector CR without its histogram family."""
    from tests.test_metric_vectors import GOLD, _metric_yaml
    doc = yaml.safe_load(_metric_yaml())
    doc["spec"]["metrics"] = [m for m in doc["spec"]["metrics"] if m["kind"] != "histogram"]
    cl = W.make_cluster("C4", 4, 40, seed=3)
    pods = cl.pods.materialize()
    nodes = cl.nodes.materialize()
    rig = Rig(cl, pods, nodes, cl.node_ptr, cr_text=yaml.safe_dump(doc))
    try:
        rig.eng.usage(T0)
        got = rig.ex.scrape(T0, 0, 4)
        assert got == [rig.expected(T0, j)[0] for j in range(4)]
        for text in got:
            for key, value in (("gauge", 42), ("counter", 84)):
                assert GOLD[key]["steps"][-1][1] == value
                want = "\n".join(GOLD[key]["want_exposition"]).replace("{value}", str(value))
                assert want in text.decode(), (key, text)
    finally:
        rig.close()


LDS_WINDOW = 12288  # expo.hip kLdsWave: a wave whose 64 lines exceed it stores them directly


def _family_lines(text: bytes, family: bytes):
    return [l + b"\n" for l in text.split(b"\n") if l.startswith(family + b"{")]


def test_long_and_escaped_names_direct_and_staged_waves():
    """Names of 200-253 characters and names with quote, backslash, newline and UTF-8, mixed with
    short ones: in node 0 the first wave of a family's sorted lines exceeds the LDS window (stored
    directly by its lanes) and later waves fit it (staged), within one 256-lane block and in
    successive 64-lane chunks; escaped label blocks reach the device.  Both widths, the whole
    range and sub-ranges."""
    per = [130, 70, 5]
    cl = W.make_cluster("C4", 3, sum(per), seed=12)
    pods = cl.pods.materialize()
    nodes = cl.nodes.materialize()
    odd = ['q"uote', "back\\slash", "new\nline", "caf\u00e9-\u65e5\u672c-\U0001F600", '"\\\n"']
    for i, p in enumerate(pods):
        md = p["metadata"]
        if i % 3 == 0:  # sorts before the short "pod-..." names
            md["name"] = ("long-%03d-" % i) + "x" * (191 + i % 54)
            assert 200 <= len(md["name"]) <= 253
        elif i % 10 == 1:
            md["name"] = odd[(i // 10) % len(odd)] + "-%d" % i
        elif i % 10 == 2:
            md["name"] = odd[(i // 10) % len(odd)] + "-" + "y" * 230
        if i % 7 == 3:
            md["namespace"] = "ns-\u00fc"
        if i % 9 == 4:
            p["spec"]["containers"][0]["name"] = 'c"\\' + "z" * (i % 5)
    node_ptr = np.concatenate([[0], np.cumsum(per)]).astype(np.uint32)
    rig = Rig(cl, pods, nodes, node_ptr)
    try:
        t = T0
        for k in range(2):
            if k == 1:
                rig.delete(np.arange(4, len(pods), 9))
            rig.eng.usage(t)
            want = [rig.expected(t, j)[0] for j in range(3)]
            # the case is what it claims: node 0's first 64 pod lines overflow the window, the next 64 fit
            if k == 0:  # (every slot is live: a wave's 64 slots are 64 lines)
                lines = _family_lines(want[0], b"pod_memory_working_set_bytes")
                assert len(lines) == per[0] and sum(map(len, lines[:64])) > LDS_WINDOW + 16
                assert sum(map(len, lines[64:128])) + 16 <= LDS_WINDOW
            assert b'\\"' in want[0] and b"\\\\" in want[0] and b"\\n" in want[0] and "\u65e5".encode() in want[0]
            for width in (64, 256, 0):
                rig.ex.set_width(width)
                assert rig.ex.scrape(t, 0, 3) == want, (k, width)
                assert rig.ex.scrape(t, 1, 2) == want[1:3], (k, width)
                assert rig.ex.scrape(t, 0, 1) == want[0:1], (k, width)
            t += 5_000_000_000
    finally:
        rig.close()


def test_live_series_without_label_row_is_refused():
    """A live pod whose label rows were never set: the scrape writes nothing and
    kwk_expo_result returns KWK_ESTATE with the count; after setting them the text is equal."""
    from kwok_amd.host.expo import ExpoError
    cl = W.make_cluster("C4", 2, 20, seed=5)
    pods = cl.pods.materialize()
    nodes = cl.nodes.materialize()
    missing = 7
    rig = Rig(cl, pods, nodes, cl.node_ptr, label_pods=[None if i == missing else p for i, p in enumerate(pods)])
    try:
        rig.eng.usage(T0)
        want = [rig.expected(T0, j)[0] for j in range(2)]
        rig.ex.reserve(sum(map(len, want)) + 64)
        rig.ex.enqueue(T0, 0, 2)
        with pytest.raises(ExpoError) as e:
            rig.ex.result()
        n_series = 2 + 3 * len(pods[missing]["spec"]["containers"])  # its pod and container families
        assert e.value.status == abi.KWK_ESTATE and str(n_series) + " live series" in str(e.value)
        rig.ex.set_pods([pods[missing]], missing, nodes)
        rig.ex.commit()
        assert rig.ex.scrape(T0, 0, 2) == want
    finally:
        rig.close()

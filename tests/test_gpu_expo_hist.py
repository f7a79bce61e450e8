"""Histogram families in the device exposition (kwk_expo_create_hist) on the GPU: every node's text
equals MetricsProgram.exposition(MetricsProgram.scrape(...)) for that node alone, byte for byte; the
counts' float64(uint64) formatting; histogram_test.go's vector; a wave of histogram lines beyond the
LDS window; the reservation / missing-row / wrong-engine protocol."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import yaml

from kwok_amd import workload as W
from kwok_amd.host import abi, cel
from kwok_amd.host.metrics import MetricsProgram, go_float, go_uint64, histogram_write
from kwok_amd.host.usage import UsageProgram, load_usage_yaml, usage_columns
from tests.test_expo_hist_program import CR, POD_LABELS

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
USAGE = os.path.join(os.path.dirname(HERE), "kwok_amd", "metrics", "usage-from-annotation.yaml")
T0 = 1_700_000_000 * 10**9
LDS_WINDOW = 12288  # expo.hip kLdsWave

CONTAINER_LABELS = POD_LABELS + [{"name": "container", "value": "container.name"}]
C_HIST = {"name": "c_hist", "kind": "histogram", "dimension": "container", "help": "container histogram",
          "labels": CONTAINER_LABELS,
          "buckets": [{"le": 0.001, "value": 'pod.Usage("cpu", container.name) * 1000.0'}, {"le": 0.25, "value": "5.0"},
                      {"le": 64, "value": 'pod.Usage("memory", container.name) / 1024.0'}]}


def _cr(*more, base=True):
    return yaml.safe_dump({"kind": "Metric", "spec": {"path": "/x", "metrics":
                                                      (CR["spec"]["metrics"] if base else []) + list(more)}})


def _ns(ts):
    return cel._parse_time(ts)


class Rig:
    """A pods engine with usage, the Metric CR (compiled with expo_histograms) loaded and an
    Exposition over it."""

    def __init__(self, cl, pods, nodes, node_ptr, cr_text, label_pods=None):
        from kwok_amd.host.compiler import KindProgram
        from kwok_amd.host.engine import Engine, Ingest
        from kwok_amd.host.expo import Exposition
        from kwok_amd.host.stages import load_stage_files
        self.pods, self.nodes = pods, nodes
        self.node_ptr = np.ascontiguousarray(node_ptr, dtype=np.uint32)
        cols = usage_columns(UsageProgram(*load_usage_yaml(open(USAGE).read())), pods)
        kp = KindProgram(load_stage_files(*cl.pod_stage_files))
        kp.explore(pods)
        ing = Ingest(kp)
        self.eng = Engine(kp, capacity=len(pods))
        try:
            self.eng.load_stages()
            self.eng.load(*ing.columns(pods), ing.record_array())
            self.eng.usage_config(self.node_ptr, *cols)
            self.eng.usage_pods(True)
            self.mp = MetricsProgram.from_native(cr_text, expo_histograms=True)
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
        return self.mp.exposition(self.mp.scrape(self.eng, t, j, [self.nodes[j]], slots, self.node_ptr)).encode()

    def close(self):
        self.ex.close()
        self.eng.close()


def _cluster(per, seed):
    cl = W.make_cluster("C4", len(per), sum(per), seed=seed)
    pods = cl.pods.materialize()
    nodes = cl.nodes.materialize()
    node_ptr = np.concatenate([[0], np.cumsum(per)]).astype(np.uint32)
    return cl, pods, nodes, node_ptr


def test_text_equals_python_path():
    """Nodes of 0, 1, 3, 70 and 300 pod slots: headers only, one series, more than one 64-lane round
    inside a family, the 256-lane block scan across waves; dead slots; a sub-range."""
    per = [0, 1, 3, 70, 300]
    cl, pods, nodes, node_ptr = _cluster(per, seed=21)
    for i, p in enumerate(pods):  # 1-2 containers per pod
        p["spec"]["containers"] = p["spec"]["containers"][:1 + i % 2]
    rig = Rig(cl, pods, nodes, node_ptr, _cr(C_HIST))
    try:
        assert rig.ex.hist_prog is not None and rig.ex.hist_prog.n_hists == 3
        t = T0
        for k in range(3):
            if k == 1:
                rig.delete(np.arange(0, len(pods), 7))
            first, n = (0, 2) if k == 2 else (0, len(per))
            rig.eng.usage(t)
            want = [rig.expected(t, j) for j in range(first, first + n)]
            if k == 0:
                head = [l for l in want[0].split(b"\n") if l]
                assert sum(l.startswith(b"#") for l in head) == 10  # five families' headers, a 0-pod node
                assert want[0].count(b"# TYPE m_hist histogram\n") == 1 and b"m_hist_bucket" not in want[0]
                assert want[3].count(b"m_hist_count{") == 70 and want[4].count(b"c_hist_sum{") > 300
            if k == 1:
                assert want[4].count(b"m_hist_count{") == int(rig.alive[int(node_ptr[4]):].sum()) < 300
            for width in (64, 256, 0):
                rig.ex.set_width(width)
                got = rig.ex.scrape(t, first, n)
                for j in range(n):
                    assert got[j] == want[j], (k, width, j)
            t += 3_000_000_000 + 977 * k
    finally:
        rig.close()


COUNTS = {"name": "k_hist", "kind": "histogram", "dimension": "node", "help": "counts",
          "buckets": [{"le": 1, "value": "999999.0"}, {"le": 2, "value": "1.0"},
                      {"le": 3, "value": "9007199253740993.0"}, {"le": 4, "value": "2.0"}]}
ONES = {"name": "ones_hist", "kind": "histogram", "dimension": "node", "help": "2^64 - 1",
        "buckets": [{"le": 1, "value": "-1.0"}]}
POD_ONES = {"name": "pod_ones_hist", "kind": "histogram", "dimension": "pod", "help": "2^64 - 1 per pod",
            "labels": POD_LABELS, "buckets": [{"le": 1, "value": "-1.0"}]}


def test_count_formatting_and_all_ones_live_record():
    """float64(uint64) of the counts: the exponent switch at 1e+06, 2^53 + 1 -> 2^53, the tie
    2^53 + 3 -> 2^53 + 4; a bucket of -1.0 is 2^64 - 1 on a live series (an all-ones record is not a
    dead slot: the alive bits decide)."""
    # the CPU restatement gives those counts
    h = histogram_write([(float(b["le"]), False) for b in COUNTS["buckets"]],
                        [go_uint64(float(b["value"])) for b in COUNTS["buckets"]])
    # (+Inf: histogram.Write adds the running count there only for a key above the last visible bound)
    assert h["counts"] == [999999, 1000000, 2**53 + 1, 2**53 + 3, 0] and h["count"] == 2**53 + 3
    assert go_uint64(-1.0) == 2**64 - 1
    o = histogram_write([(1.0, False)], [go_uint64(-1.0)])
    assert o["counts"] == [2**64 - 1, 0] and o["count"] == 2**64 - 1
    assert [go_float(float(c)) for c in h["counts"][:4]] == ["999999", "1e+06", "9.007199254740992e+15",
                                                              "9.007199254740996e+15"]
    assert go_float(float(2**64 - 1)) == "1.8446744073709552e+19"

    cl, pods, nodes, node_ptr = _cluster([3, 2], seed=8)
    rig = Rig(cl, pods, nodes, node_ptr, _cr(COUNTS, ONES, POD_ONES, base=False))
    try:
        rig.delete(np.array([1]))
        rig.eng.usage(T0)
        want = [rig.expected(T0, j) for j in range(2)]
        got = rig.ex.scrape(T0, 0, 2)
        assert got == want
        for text in got:
            for line in ('k_hist_bucket{le="1"} 999999', 'k_hist_bucket{le="2"} 1e+06',
                         'k_hist_bucket{le="3"} 9.007199254740992e+15', 'k_hist_bucket{le="4"} 9.007199254740996e+15',
                         'k_hist_bucket{le="+Inf"} 0', 'k_hist_count 9.007199254740996e+15',
                         'ones_hist_bucket{le="1"} 1.8446744073709552e+19',
                         'ones_hist_bucket{le="+Inf"} 0', 'ones_hist_sum 1.8446744073709552e+19',
                         'ones_hist_count 1.8446744073709552e+19'):
                assert (line + "\n").encode() in text, line
        # the live pods' all-ones records are written, the dead slot's is not
        assert got[0].count(b"pod_ones_hist_count{") == 2 and got[1].count(b"pod_ones_hist_count{") == 2
        name = pods[0]["metadata"]["name"]
        assert ('pod_ones_hist_bucket{namespace="default",pod="%s",le="1"} 1.8446744073709552e+19\n' % name).encode() \
            in got[0]
        assert ('pod="%s"' % pods[1]["metadata"]["name"]).encode() not in got[0]
    finally:
        rig.close()


def test_reference_vector_histogram():
    """histogram_test.go:29-96 (tests/golden/metric_vectors.json) as a node histogram: the expected
    lines are built here from the JSON alone."""
    from tests.test_metric_vectors import GOLD, _metric_yaml
    h = GOLD["histogram"]
    assert h["buckets"] == [0.5, 1, 2.5, 5, 10] and h["want_cumulative"] == [0, 3, 15, 15, 31, 63]
    total = 0.0
    for le, c in sorted(h["want_sample_sum_ascending"]):
        total += float(le) * float(c)
    lines = ['name_bucket{le="%s"} %d' % (le, c) for le, c in zip(["0.5", "1", "2.5", "5", "10", "+Inf"],
                                                                   h["want_cumulative"])]
    assert go_float(total) == repr(total)  # a plain decimal: no exponent form at this size
    lines += ["name_sum " + repr(total), "name_count %d" % h["want_sample_count"]]
    want = ("# HELP name help\n# TYPE name histogram\n" + "\n".join(lines) + "\n").encode()
    cl, pods, nodes, node_ptr = _cluster([2, 1], seed=3)
    rig = Rig(cl, pods, nodes, node_ptr, _metric_yaml())
    try:
        rig.eng.usage(T0)
        for text in rig.ex.scrape(T0, 0, 2):
            assert want in text, text
    finally:
        rig.close()


def test_histogram_wave_beyond_the_lds_window():
    """Pod names of 253 characters and a namespace with backslash, quote and newline: a wave's 64
    histogram lines exceed the LDS window and are stored directly by their lanes; the short names
    after them are staged."""
    per = [24, 3]
    cl, pods, nodes, node_ptr = _cluster(per, seed=12)
    for i, p in enumerate(pods):
        md = p["metadata"]
        md["namespace"] = 'n\\s"x\ny'
        if i % 2 == 0:  # sorts before the short "pod-..." names
            md["name"] = ("long-%03d-" % i) + "x" * 244
            assert len(md["name"]) == 253
    rig = Rig(cl, pods, nodes, node_ptr, _cr())
    try:
        rig.eng.usage(T0)
        want = [rig.expected(T0, j) for j in range(2)]
        lines = [l + b"\n" for l in want[0].split(b"\n") if l.startswith(b"m_hist_")]
        assert len(lines) == 24 * 7  # 4 visible bounds, +Inf, _sum, _count
        assert sum(map(len, lines[:64])) > LDS_WINDOW + 16 and sum(map(len, lines[128:])) + 16 <= LDS_WINDOW
        assert b'namespace="n\\\\s\\"x\\ny"' in want[0]
        for width in (64, 256, 0):
            rig.ex.set_width(width)
            assert rig.ex.scrape(T0, 0, 2) == want, width
            assert rig.ex.scrape(T0, 1, 1) == want[1:], width
    finally:
        rig.close()


def test_protocol():
    from kwok_amd.host.expo import ExpoError, lib
    cl, pods, nodes, node_ptr = _cluster([12, 8], seed=5)
    missing = 7
    rig = Rig(cl, pods, nodes, node_ptr, _cr(C_HIST), label_pods=[None if i == missing else p for i, p in enumerate(pods)])
    try:
        L = lib()
        # kwk_expo_create refuses a program with a histogram family, by name
        h = C.c_void_p()
        assert L.kwk_expo_create(rig.eng.h, len(nodes), C.byref(rig.ex.prog), C.byref(h)) == abi.KWK_EINVAL
        assert b"'c_hist'" in L.kwk_expo_last_error(None) and not h.value  # the first histogram family in name order

        rig.eng.usage(T0)
        want = [rig.expected(T0, j) for j in range(2)]
        total = sum(map(len, want))
        # a live pod without label rows: KWK_ESTATE counting series (a_gauge, m_hist, c_hist per container), not lines
        rig.ex.reserve(total + 64)
        rig.ex.enqueue(T0, 0, 2)
        with pytest.raises(ExpoError) as e:
            rig.ex.result()
        n_series = 2 + len(pods[missing]["spec"]["containers"])
        assert e.value.status == abi.KWK_ESTATE and str(n_series) + " live series" in str(e.value)
        rig.ex.set_pods([pods[missing]], missing, nodes)
        rig.ex.commit()
        rig.ex.enqueue(T0, 0, 2)
        assert rig.ex.result() == total
        off, raw = rig.ex.copy(total)
        assert [raw.tobytes()[int(off[j]):int(off[j + 1])] for j in range(2)] == want

        # one byte less than the text: KWK_ECAP, `needed` is the size, the sentinel-filled buffer is untouched
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        rig.ex.reserve(total - 1)
        offp, buf = C.c_void_p(), C.c_void_p()
        assert L.kwk_expo_device(rig.ex.h, C.byref(offp), C.byref(buf)) == 0
        assert hip.hipMemset(buf, 0xA5, total - 1) == 0 and hip.hipDeviceSynchronize() == 0
        rig.ex.enqueue(T0, 0, 2)
        with pytest.raises(ExpoError) as e:
            rig.ex.result()
        assert e.value.status == abi.KWK_ECAP and rig.ex.needed == total
        host = np.zeros(total - 1, dtype=np.uint8)
        assert hip.hipMemcpy(abi.ptr(host), buf, total - 1, 2) == 0  # hipMemcpyDeviceToHost
        assert np.all(host == 0xA5)
        assert rig.ex.scrape(T0, 0, 2) == want  # reserves more and scrapes again

        # the engine loaded with another histogram CR (one bucket fewer): the record words differ
        other = json.loads(json.dumps(C_HIST))
        other["buckets"] = other["buckets"][:2]
        MetricsProgram.from_native(_cr(other), expo_histograms=True).load(rig.eng)
        with pytest.raises(ExpoError) as e:
            rig.ex.enqueue(T0, 0, 2)
        assert e.value.status == abi.KWK_ESTATE and "record words" in str(e.value)
    finally:
        rig.close()

"""Incremental label commits of the device exposition (kwk_expo_commit_rows) on the GPU: after
relabelling some pod slots and committing only their rows, every node's text equals
MetricsProgram.exposition(MetricsProgram.scrape(...)) byte for byte, and both the text and every
group's device permutation (kwk_expo_read_perm) equal what a full kwk_expo_commit of the same host
state gives.  The engine's values follow the slot, so relabelling is a change of the Python pod
dicts and Exposition.set_pods for those slots only."""
import copy

import numpy as np
import pytest
import yaml

from kwok_amd import workload as W
from kwok_amd.host import abi
from kwok_amd.host.usage import UsageProgram, load_usage_yaml, usage_columns
from tests.test_gpu_expo import _LABEL, METRICS, T0, USAGE, Rig, _mixed_cluster

pytestmark = pytest.mark.gpu

DIM_NODE = 0


def _want(rig, t, j):
    w = rig.expected(t, j)
    return w[0] if isinstance(w, tuple) else w


def _relabel(rig, slots):
    for i in slots:
        rig.ex.set_pods([rig.pods[int(i)]], int(i), rig.nodes)


def _perms(rig):
    return {g: rig.ex.read_perm(g).copy() for g, (dim, _) in enumerate(rig.ex.groups) if dim != DIM_NODE}


def _check(rig, t, ranges=(), widths=(0,), tag=None):
    """The scrape at t equals expected() (every node, the sub-ranges, the widths); then a full commit
    of the same host state: the same scrapes and every permutation are byte-equal to the incremental
    ones."""
    n = len(rig.nodes)
    rig.eng.usage(t)
    want = [_want(rig, t, j) for j in range(n)]
    for width in widths:
        rig.ex.set_width(width)
        got = rig.ex.scrape(t, 0, n)
        for j in range(n):
            assert got[j] == want[j], (tag, width, j)
        for first, count in ranges:
            assert rig.ex.scrape(t, first, count) == want[first:first + count], (tag, width, first)
    rig.ex.set_width(0)
    texts = [rig.ex.scrape(t, 0, n)] + [rig.ex.scrape(t, first, count) for first, count in ranges]
    perms = _perms(rig)
    assert perms
    rig.ex.commit()
    assert [rig.ex.scrape(t, 0, n)] + [rig.ex.scrape(t, first, count) for first, count in ranges] == texts, tag
    full = _perms(rig)
    for g in perms:
        assert np.array_equal(perms[g], full[g]), (tag, g)
    return want


def test_relabel_equals_full_commit():
    """Pods per node [0, 1, 63, 64, 65, 300, 0, 207]; four rounds of commit_rows on one rig: a seeded
    10 % renamed shorter / as long / longer, every pod of the 65-pod node, nothing, and every pod to a
    name three times as long (the arenas' tail slack, an eighth of a full commit's bytes + 4 KiB, is
    passed several times over: they grow)."""
    per = [0, 1, 63, 64, 65, 300, 0, 207]
    cl = W.make_cluster("C4", 8, sum(per), seed=9)
    pods = cl.pods.materialize()
    nodes = cl.nodes.materialize()
    node_ptr = np.concatenate([[0], np.cumsum(per)]).astype(np.uint32)
    rig = Rig(cl, pods, nodes, node_ptr)
    try:
        rng = np.random.default_rng(1009)
        t = T0
        for k in range(4):
            if k == 0:
                slots = np.sort(rng.choice(len(pods), size=len(pods) // 10, replace=False))
                delta = set()
                for q, i in enumerate(slots):
                    old = pods[i]["metadata"]["name"]
                    pods[i]["metadata"]["name"] = [old[:-2], old[::-1], old + "-longer-%d" % i][q % 3]
                    delta.add(np.sign(len(pods[i]["metadata"]["name"]) - len(old)))
                    assert pods[i]["metadata"]["name"]
                assert delta == {-1, 0, 1}
            elif k == 1:
                slots = np.arange(node_ptr[4], node_ptr[5])
                for i in slots:
                    pods[i]["metadata"]["name"] = "n4-%03d" % (997 * int(i) % 1000)
                    pods[i]["metadata"]["namespace"] = "other" if i % 3 == 0 else "default"
            elif k == 2:
                slots = []
            else:
                slots = np.arange(len(pods))
                total = sum(len(p["metadata"]["name"]) for p in pods)
                for i in slots:
                    pods[i]["metadata"]["name"] = "-".join([pods[i]["metadata"]["name"]] * 3)[:253]
                assert sum(len(p["metadata"]["name"]) for p in pods) >= 3 * total
            _relabel(rig, slots)
            rig.ex.commit_rows()
            _check(rig, t, ranges=((5, 3),), widths=(64, 256, 0), tag=k)
            t += 7_000_000_000
    finally:
        rig.close()


# a / a-b / a.b / a0 / A / b; a prefix; big-endian order within a word; equal for 9 bytes, different in
# the 10th (the second word); bytes >= 0x80; the same name twice (stability by slot)
ORDER_NAMES = ["a", "a-b", "a.b", "a0", "A", "b", "web", "web-0", "ab", "ba", "pod-name-x1", "pod-name-x2",
               "é1", "a"]


def test_comparator_order_through_the_kernel():
    """One node whose pods get, through commit_rows, the 14 names of ORDER_NAMES in the namespaces ns
    and ns-b, in a scrambled slot order (28 slots: the listed names, one of them twice, in both
    namespaces do not fit fewer).  The text equals expected(), a family's label tuples are in sorted
    order, and the pod group's permutation is the stable sort of the slots by (namespace, name)."""
    combos = [(ns, name) for ns in ("ns", "ns-b") for name in ORDER_NAMES]
    cl = W.make_cluster("C4", 1, len(combos), seed=4)
    pods = cl.pods.materialize()
    nodes = cl.nodes.materialize()
    rig = Rig(cl, pods, nodes, cl.node_ptr)  # the generator's uniform names, full commit
    try:
        order = np.random.default_rng(28).permutation(len(combos))
        for i, p in enumerate(pods):
            p["metadata"]["namespace"], p["metadata"]["name"] = combos[order[i]]
        _relabel(rig, range(len(pods)))
        rig.ex.commit_rows()
        rig.eng.usage(T0)
        got = rig.ex.scrape(T0, 0, 1)[0]
        assert got == _want(rig, T0, 0)
        lines = [l for l in got.decode().split("\n") if l.startswith("pod_memory_working_set_bytes{")]
        keys = [tuple(v for _, v in _LABEL.findall(l)) for l in lines]
        assert keys == sorted(keys) and len(keys) == len(combos) and keys[0] == ("ns", "A") and keys[-1][0] == "ns-b"
        assert keys.count(("ns", "a")) == 2
        (g,) = [g for g, (dim, _) in enumerate(rig.ex.groups) if dim == 1]
        slot_key = [(combos[order[i]][0].encode(), combos[order[i]][1].encode()) for i in range(len(pods))]
        assert list(rig.ex.read_perm(g)) == sorted(range(len(pods)), key=lambda i: (slot_key[i], i))
        _check(rig, T0 + 10**9, tag="order")
    finally:
        rig.close()


def test_rows_that_were_never_set():
    from kwok_amd.host.expo import ExpoError
    cl = W.make_cluster("C4", 2, 20, seed=5)
    pods = cl.pods.materialize()
    nodes = cl.nodes.materialize()
    missing = [3, 7, 8, 19]
    rig = Rig(cl, pods, nodes, cl.node_ptr, label_pods=[None if i in missing else p for i, p in enumerate(pods)])
    try:
        rig.eng.usage(T0)
        want = [_want(rig, T0, j) for j in range(2)]
        rig.ex.reserve(sum(map(len, want)) + 64)
        rig.ex.enqueue(T0, 0, 2)
        with pytest.raises(ExpoError) as e:
            rig.ex.result()
        assert e.value.status == abi.KWK_ESTATE and "live series" in str(e.value)
        _relabel(rig, missing)
        rig.ex.commit_rows()
        assert rig.ex.scrape(T0, 0, 2) == want
        # dead slots beside relabelled live ones
        rig.delete(np.array([2, 8, 18]))
        for i in (1, 3, 7, 9, 17, 19):
            pods[i]["metadata"]["name"] = "neighbour-of-a-dead-slot-%d" % (19 - i)
        _relabel(rig, (1, 3, 7, 9, 17, 19))
        rig.ex.commit_rows()
        _check(rig, T0 + 3 * 10**9, ranges=((1, 1),), tag="dead")
    finally:
        rig.close()


NODE_INFO = {"name": "node_info", "kind": "gauge", "dimension": "node", "help": "a labelled node family",
             "labels": [{"name": "node", "value": "node.metadata.name"}], "value": "1.0"}


def _cr_with_node_labels():
    doc = yaml.safe_load(open(METRICS).read())
    doc["spec"]["metrics"].append(NODE_INFO)
    return yaml.safe_dump(doc)


def test_container_and_node_groups():
    """The mixed-container cluster, the shipped CR plus a node family with a label: containers
    renamed inside some pods (the container group's permutation), one node renamed (a block, no
    permutation)."""
    cl, pods, text = _mixed_cluster()
    pods = [copy.deepcopy(p) for p in pods]  # (a container renamed below is that pod's own)
    nodes = cl.nodes.materialize()
    rig = Rig(cl, pods, nodes, cl.node_ptr, usage_text=text, cr_text=_cr_with_node_labels())
    try:
        dims = [dim for dim, _ in rig.ex.groups]
        assert 0 in dims and 1 in dims and 2 in dims
        assert any(dim == 0 and n_labels == 1 for dim, n_labels in rig.ex.groups)
        slots = list(range(2, len(pods), 9))
        for q, i in enumerate(slots):
            cs = pods[i]["spec"]["containers"]
            cs[q % len(cs)]["name"] = ["z", "a-renamed-container-%d" % i, "container-0"][q % 3]
        _relabel(rig, slots)
        nodes[3]["metadata"]["name"] = "a-node-with-a-rather-longer-name-than-before"
        rig.ex.set_nodes([nodes[3]], 3)
        rig.ex.commit_rows()
        t = T0 + 5 * 10**9
        want = _check(rig, t, ranges=((3, 3),), widths=(0, 256), tag="mixed")
        assert b'node_info{node="a-node-with-a-rather-longer-name-than-before"} 1\n' in want[3]
        assert any(b'container="z"' in w for w in want)
        # after the full commit of _check: once more through the incremental path, single-node scrapes
        nodes[3]["metadata"]["name"] = "n3"
        rig.ex.set_nodes([nodes[3]], 3)
        pods[slots[0]]["spec"]["containers"][0]["name"] = "zz"
        _relabel(rig, slots[:1])
        rig.ex.commit_rows()
        for j in range(len(nodes)):
            assert rig.ex.scrape(t, j, 1) == [_want(rig, t, j)], j
    finally:
        rig.close()


def test_histogram_writer():
    """The <., ., true> kernels read the rows' pairs: a pod and a container histogram family after
    commit_rows."""
    from tests.test_gpu_expo_hist import C_HIST, Rig as HistRig, _cluster, _cr
    per = [3, 70, 5]
    cl, pods, nodes, node_ptr = _cluster(per, seed=21)
    rig = HistRig(cl, pods, nodes, node_ptr, _cr(C_HIST))
    try:
        assert rig.ex.hist_prog is not None
        slots = list(range(0, len(pods), 4))
        for i in slots:
            pods[i]["metadata"]["name"] = ["h", "hist-pod-renamed-to-a-longer-name-%d" % i][i % 8 == 0]
            pods[i]["metadata"]["namespace"] = "ns-%d" % (i % 3)
        _relabel(rig, slots)
        rig.ex.commit_rows()
        want = _check(rig, T0, ranges=((1, 2),), widths=(64, 256, 0), tag="hist")
        assert want[1].count(b"m_hist_count{") == 70 and b'pod="h"' in want[1] and b"c_hist_bucket{" in want[1]
    finally:
        rig.close()


def test_segment_beyond_the_device_limit():
    """A node of limit + 70 pods (sorted on the host, its permutation slice uploaded) beside one of 3
    (sorted by the kernel)."""
    from kwok_amd.host.expo import SORT_MAX_ROWS
    assert SORT_MAX_ROWS >= 1024
    per = [SORT_MAX_ROWS + 70, 3]
    cl = W.make_cluster("C4", 2, sum(per), seed=17)
    pods = cl.pods.materialize()
    nodes = cl.nodes.materialize()
    node_ptr = np.concatenate([[0], np.cumsum(per)]).astype(np.uint32)
    rig = Rig(cl, pods, nodes, node_ptr)
    try:
        slots = list(range(1, per[0], 37)) + [per[0], per[0] + 2]
        for i in slots:
            pods[i]["metadata"]["name"] = "%s-moved-%d" % ("az"[i % 2], i)
        _relabel(rig, slots)
        rig.ex.commit_rows()
        _check(rig, T0, ranges=((1, 1),), tag="limit")
    finally:
        rig.close()


def test_long_keys_with_a_shared_prefix():
    """150 pods renamed to 240-253 characters that share their first 200 bytes, on one node: the
    comparator's 26th and later words decide, the keys of the node (37 KB and more) are no longer a
    few cache lines, and every block outgrows its slot.  A 40-pod node beside it gets the shortest
    and the longest name."""
    per = [150, 40]
    cl = W.make_cluster("C4", 2, sum(per), seed=23)
    pods = cl.pods.materialize()
    nodes = cl.nodes.materialize()
    node_ptr = np.concatenate([[0], np.cumsum(per)]).astype(np.uint32)
    rig = Rig(cl, pods, nodes, node_ptr)
    try:
        for i in range(per[0]):
            pods[i]["metadata"]["name"] = "k" * 200 + "-%03d-" % (613 * i % 1000) + "w" * (35 + i % 14)
        assert sum(len(p["metadata"]["name"]) + 9 for p in pods[:per[0]]) > 37_000  # namespace NUL name NUL
        slots = list(range(per[0])) + [per[0] + 3, per[0] + 30]
        pods[per[0] + 3]["metadata"]["name"] = "short"
        pods[per[0] + 30]["metadata"]["name"] = "k" * 253
        _relabel(rig, slots)
        rig.ex.commit_rows()
        _check(rig, T0, ranges=((1, 1),), tag="lds")
    finally:
        rig.close()


def test_refusals():
    from kwok_amd.host.expo import ExpoError, Exposition
    cl = W.make_cluster("C4", 2, 20, seed=5)
    pods = cl.pods.materialize()
    nodes = cl.nodes.materialize()
    rig = Rig(cl, pods, nodes, cl.node_ptr, cr_text=_cr_with_node_labels())
    try:
        # a writer that was never fully committed
        fresh = Exposition(rig.eng, rig.mp.native)
        try:
            fresh.set_pods(pods, 0, nodes)
            with pytest.raises(ExpoError) as e:
                fresh.commit_rows()
            assert e.value.status == abi.KWK_ESTATE and "kwk_expo_commit" in str(e.value)
        finally:
            fresh.close()
        # no permutation for a node group
        (g_node,) = [g for g, (dim, n_labels) in enumerate(rig.ex.groups) if dim == DIM_NODE and n_labels]
        with pytest.raises(ExpoError) as e:
            rig.ex.read_perm(g_node)
        assert e.value.status == abi.KWK_EINVAL
        # nothing dirty: fine
        rig.ex.commit_rows()
        # the engine's pod count changes under the writer
        fewer = len(pods) - 4
        node_ptr = np.array(cl.node_ptr, dtype=np.uint32)
        assert node_ptr[-1] - node_ptr[-2] > 4
        node_ptr[-1] = fewer
        cols = usage_columns(UsageProgram(*load_usage_yaml(open(USAGE).read())), pods[:fewer])
        rig.eng.usage_config(node_ptr, *cols)
        pods[0]["metadata"]["name"] = "renamed"
        rig.ex.set_pods([pods[0]], 0, nodes)
        with pytest.raises(ExpoError) as e:
            rig.ex.commit_rows()
        assert e.value.status == abi.KWK_ESTATE and "kwk_expo_commit" in str(e.value)
        rig.ex.commit()
        pods[1]["metadata"]["name"] = "renamed-too"
        rig.ex.set_pods([pods[1]], 1, nodes)
        rig.ex.commit_rows()
        (g_pod,) = [g for g, (dim, _) in enumerate(rig.ex.groups) if dim == 1]
        lo = int(node_ptr[0])
        hi = int(node_ptr[1])
        names = [(p["metadata"]["namespace"].encode(), p["metadata"]["name"].encode()) for p in pods]
        assert list(rig.ex.read_perm(g_pod)[lo:hi]) == sorted(range(lo, hi), key=lambda i: (names[i], i))
    finally:
        rig.close()

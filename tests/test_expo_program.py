"""The exposition program and the native label renderer of libkwok_compiler (kwok_metrics.h:
kwk_metric_set_exposition / kwk_metric_labels_render) against the Python exposition and CEL
evaluator, the refusals (histogram, host-evaluated metric, computed label) by name, and the
exported symbols of libkwok_expo.so.  CPU only."""
import ctypes
import ctypes as C
import os
import re
import subprocess

import pytest
import yaml

from kwok_amd import workload as W
from kwok_amd.host import cel
from kwok_amd.host.metrics import MetricsProgram, _escape_label, load_metric_doc, load_metric_yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
METRICS = os.path.join(ROOT, "kwok_amd", "metrics", "metrics-resource.yaml")


@pytest.fixture(scope="module")
def nm():
    from kwok_amd import build
    build.build()
    from kwok_amd.host import native_metrics
    return native_metrics


def _set(nm, text):
    return nm.NativeMetricSet(load_metric_doc(text))


def test_shipped_cr_program(nm):
    text = open(METRICS).read()
    ms = _set(nm, text)
    prog = ms.exposition_program()
    _, configs = load_metric_yaml(text)
    assert prog.n_families == 8 and prog.n_groups == 3 and prog.n_metrics == 8
    lits = C.string_at(prog.lits, prog.n_lit_bytes)
    fams = [prog.families[i] for i in range(8)]
    names = [lits[f.name_off:f.name_off + f.name_len].decode() for f in fams]
    assert names == sorted(c.name for c in configs)
    # header bytes: exposition() of no series is every family's HELP / TYPE lines in order
    headers = b"".join(lits[f.header_off:f.header_off + f.header_len] for f in fams)
    assert headers == MetricsProgram(configs).exposition({}).encode()
    by_name = {c.name: (i, c) for i, c in enumerate(configs)}
    dims = {"node": 0, "pod": 1, "container": 2}
    groups = {}
    for f, name in zip(fams, names):
        i, c = by_name[name]
        assert f.metric == i and f.dimension == dims[c.dimension] and prog.metric_dimension[i] == f.dimension
        g = prog.groups[f.group]
        assert g.dimension == f.dimension and g.n_labels == len(c.labels)
        groups.setdefault(f.group, set()).add(tuple(k for k, _ in c.labels))
    assert sorted(groups.values(), key=sorted) == [{()}, {("container", "namespace", "pod")}, {("namespace", "pod")}]


def _group_of(ms, dim, n_labels):
    prog = ms.exposition_program()
    for g in range(prog.n_groups):
        if prog.groups[g].dimension == dim and prog.groups[g].n_labels == n_labels:
            return g
    raise AssertionError("no such group")


ODD = ['plain', 'quo"te', 'back\\slash', 'new\nline', 'café-日本-\U0001F600', '', 'x' * 253, '\\n"\\"']


def test_label_renderer_equals_cel_and_escape(nm):
    text = open(METRICS).read()
    ms = _set(nm, text)
    _, configs = load_metric_yaml(text)
    pod_labels = next(c.labels for c in configs if c.name == "pod_cpu_usage_seconds_total")
    con_labels = next(c.labels for c in configs if c.name == "container_cpu_usage_seconds_total")
    gp, gc, gn = _group_of(ms, 1, 2), _group_of(ms, 2, 3), _group_of(ms, 0, 0)
    node = {"metadata": {"name": "node-0"}}
    assert ms.labels_render(gn, node, None) == (b"", b"")
    assert ms.labels_render(gn, None, None) == (b"", b"")

    def want(labels, pod, container):
        vals = [str(cel.evaluate(e, node=node, pod=pod, container=container)) for _, e in labels]
        block = "{" + ",".join(f'{k}="{_escape_label(v)}"' for (k, _), v in zip(labels, vals)) + "}"
        return block.encode(), b"".join(v.encode() + b"\0" for v in vals)

    for name in ODD:
        for ns in ("default", ODD[1], ODD[4], ""):
            pod = W.pod_object("p", "node-0")
            pod["metadata"]["name"] = name
            pod["metadata"]["namespace"] = ns
            pod["spec"]["containers"] = [{"name": c, "image": "i"} for c in ODD]
            assert ms.labels_render(gp, node, pod) == want(pod_labels, pod, None), (name, ns)
            for j, c in enumerate(pod["spec"]["containers"]):
                assert ms.labels_render(gc, None, pod, j) == want(con_labels, pod, c), (name, ns, j)


def test_literal_and_node_labels(nm):
    doc = {"kind": "Metric", "spec": {"path": "/x", "metrics": [
        {"name": "m", "kind": "gauge", "dimension": "pod", "value": "1.0",
         "labels": [{"name": "const", "value": "'a\"b'"}, {"name": "node", "value": "node.metadata.name"},
                    {"name": "pod", "value": "pod.metadata.name"}]}]}}
    ms = nm.NativeMetricSet(doc)
    node, pod = {"metadata": {"name": "n\\1"}}, {"metadata": {"name": "p"}}
    assert ms.labels_render(0, node, pod) == (b'{const="a\\"b",node="n\\\\1",pod="p"}', b'a"b\0n\\1\0p\0')
    with pytest.raises(nm.LabelRenderError, match="node"):
        ms.labels_render(0, None, pod)


def test_key_order_is_value_list_order(nm):
    """Bytewise order of the keys is the order of the value lists, also where a value is a prefix
    of another or holds bytes below the separator."""
    doc = {"kind": "Metric", "spec": {"path": "/x", "metrics": [
        {"name": "m", "kind": "gauge", "dimension": "pod", "value": "1.0",
         "labels": [{"name": "namespace", "value": "pod.metadata.namespace"},
                    {"name": "pod", "value": "pod.metadata.name"}]}]}}
    ms = nm.NativeMetricSet(doc)
    vals = [(ns, n) for ns in ("a", "a-b", "a\x00", "a\x01", "A", "") for n in ("a", "a.b", "a0", "\x00", "\x01\x01", "b")]
    keys = [ms.labels_render(0, None, {"metadata": {"namespace": ns, "name": n}})[1] for ns, n in vals]
    order = sorted(range(len(vals)), key=lambda i: keys[i])
    assert [vals[i] for i in order] == sorted(vals, key=lambda v: [v[0], v[1]])


HIST = """
kind: Metric
spec:
  path: /h
  metrics:
  - name: fine_gauge
    kind: gauge
    dimension: pod
    labels:
    - name: pod
      value: pod.metadata.name
    value: pod.Usage("memory")
  - name: pod_memory_mib
    kind: histogram
    dimension: pod
    labels:
    - name: pod
      value: pod.metadata.name
    buckets:
    - le: 1
      value: pod.Usage("memory") / 1048576.0
"""


def _cr(metric):
    return yaml.safe_dump({"kind": "Metric", "spec": {"path": "/x", "metrics": [
        {"name": "ok_metric", "kind": "gauge", "dimension": "node", "value": "1.0"}, metric]}})


@pytest.mark.parametrize("text,names", [
    (HIST, ["pod_memory_mib", "histogram"]),
    (_cr({"name": "host_side", "kind": "gauge", "dimension": "node",
          "value": "node.status.allocatable['cpu']"}), ["host_side", "host-evaluated"]),
    (_cr({"name": "computed", "kind": "gauge", "dimension": "pod", "value": "1.0",
          "labels": [{"name": "podx", "value": 'pod.metadata.name + "x"'}]}), ["computed", "podx"]),
], ids=["histogram", "host-metric", "computed-label"])
def test_refused_all_or_nothing(nm, text, names):
    ms = _set(nm, text)
    if "host_side" in names:
        assert ms.host_metrics == ["host_side"]
    with pytest.raises(nm.NoExposition) as e:
        ms.exposition_program()
    for n in names:
        assert n in str(e.value)
    with pytest.raises(nm.NoExposition):  # no partial program: no group renders either
        ms.labels_render(0, None, None)
    prog = nm.ExpoProgramStruct()
    assert nm.lib().kwk_metric_set_exposition(ms.h, C.byref(prog)) == nm.KWK_ENOLOWER


def test_missing_key_and_non_string_leaf_are_einval(nm):
    ms = _set(nm, open(METRICS).read())
    gp, gc = _group_of(ms, 1, 2), _group_of(ms, 2, 3)
    pod = W.pod_object("p", "node-0")
    pod["metadata"].pop("namespace", None)
    with pytest.raises(nm.LabelRenderError, match="namespace"):
        ms.labels_render(gp, None, pod)
    L = nm.lib()
    bl, kl = C.c_uint32(), C.c_uint32()
    buf = C.create_string_buffer(64)
    import json
    assert L.kwk_metric_labels_render(ms.h, gp, None, json.dumps(pod).encode(), 0, buf, 64, C.byref(bl), buf, 64,
                                      C.byref(kl)) == -1  # KWK_EINVAL
    pod["metadata"]["namespace"] = 7
    with pytest.raises(nm.LabelRenderError, match="not a string"):
        ms.labels_render(gp, None, pod)
    pod["metadata"]["namespace"] = "default"
    with pytest.raises(nm.LabelRenderError, match="containers"):
        ms.labels_render(gc, None, pod, len(pod["spec"]["containers"]))
    with pytest.raises(nm.LabelRenderError, match="pod_json"):
        ms.labels_render(gp, None, None)


def test_every_expo_header_declaration_is_exported(nm):
    path = os.path.join(ROOT, "kwok_amd", "lib", "libkwok_expo.so")
    ctypes.CDLL(os.path.join(ROOT, "kwok_amd", "lib", "libkwok_engine.so"))
    ctypes.CDLL(path)
    text = open(os.path.join(ROOT, "include", "kwok_expo.h")).read()
    declared = set(re.findall(r"^\s*(?:kwk_status|const char\*|uint32_t)\s+(kwk_\w+)\s*\(", text, re.M))
    assert len(declared) >= 14 and "kwk_expo_format_f64" in declared
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (kwk_\w+)", out))
    assert declared <= exported, sorted(declared - exported)
    # and the two additions of kwok_metrics.h by libkwok_compiler.so
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "kwok_amd", "lib", "libkwok_compiler.so")],
                         capture_output=True, text=True).stdout
    assert {"kwk_metric_set_exposition", "kwk_metric_labels_render"} <= set(re.findall(r" T (kwk_\w+)", out))

"""ResourceUsage expressions that read the clock (pod / node SinceSecond, Now().UnixSecond()):
the host's partial evaluation and lowering (cel.lower_usage, usage.usage_columns_dyn) against a
restatement by hand (tests/usage_dyn_util.py) and against the project's evaluator."""
import math
import os

import numpy as np
import pytest

from kwok_amd import workload as W
from kwok_amd.host import cel
from kwok_amd.host.usage import (UsageCompileError, UsageProgram, load_usage_yaml, usage_columns, usage_columns_dyn)
from tests.usage_dyn_util import ANN, EXPR, created_ns, restate, usage_doc

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(__file__)), "kwok_amd", "metrics", "usage-from-annotation.yaml")
REL_TOL = 1e-6   # the project's usage tolerance
T0 = 1_700_000_000 * 10**9

NODE = {"metadata": {"name": "node-0", "creationTimestamp": "2023-11-01T00:00:00Z"}}


def _pod(created="2023-11-14T22:00:00Z", ann=None):
    md = {"name": "pod-0", "namespace": "default"}
    if created:
        md["creationTimestamp"] = created
    if ann is not None:
        md["annotations"] = ann
    return {"metadata": md, "spec": {"nodeName": "node-0", "containers": [{"name": "c0"}]}}


# T0 is 2023-11-14T22:13:20Z: 800 s after the pod's creation
CLOCKS = [T0, T0 + 1, T0 + 123_456_789_012, T0 - 3600 * 10**9,   # the last: now before the creation
          T0 + 40 * 365 * 86400 * 10**9]                           # decades on: the Mi ramps leave int64
PODS = {"plain": _pod(), "unset": _pod(created=None), "annotated": _pod(ann={ANN: "3Mi"}),
        "bad-annotation": _pod(ann={ANN: "three"})}


@pytest.mark.parametrize("name", sorted(EXPR))
@pytest.mark.parametrize("pod", sorted(PODS))
def test_lowering_matches_restatement_and_evaluator(name, pod):
    p = PODS[pod]
    c = p["spec"]["containers"][0]
    try:
        low = cel.lower_usage(cel.compile(EXPR[name]), pod=p, node=NODE, container=c)
    except cel.CELError:
        low = 0.0  # an error whatever the clock says: the usage is 0
    hit_min = False
    for now in CLOCKS:
        got = low if isinstance(low, float) else cel.run_usage_program(low, now, created_ns(p), created_ns(NODE))
        want = restate(name, now, p, NODE)
        try:
            ev = cel.evaluate_float64(EXPR[name], node=NODE, pod=p, container=c, env=cel.Env(now_ns=now))
        except cel.CELError:
            ev = 0.0
        print(name, pod, now, got, want, ev)
        assert got == pytest.approx(want, rel=REL_TOL, abs=0), (name, pod, now)
        assert got == pytest.approx(ev, rel=1e-12, abs=0), (name, pod, now)
        hit_min |= got == -(2.0 ** 63) * 1e-9
    if name == "ramp":  # the product beyond int64: newQuantityFromFloat64 gives INT64_MIN nano
        assert hit_min
    if pod == "unset" and name in ("ramp", "base_ramp", "capped"):
        # time.Since(zero time) saturates at MaxInt64 ns
        assert not isinstance(low, float)
        assert cel.run_usage_program([(cel.OP_LOAD, cel.IN_POD_SINCE)], T0, None, None) == 9223372036.854775807


def test_clock_free_parts_fold():
    """Annotations, `in`, Quantity(..) and creationTimestamp.UnixSecond() fold for the pod; a
    ternary with a clock-free condition lowers only the branch taken."""
    ast = cel.compile(EXPR["annotated"])
    assert cel.lower_usage(ast, pod=PODS["plain"], node=NODE, container={}) == 5.0 * 2 ** 20  # the constant fallback
    low = cel.lower_usage(ast, pod=PODS["annotated"], node=NODE, container={})
    assert [op for op, _ in low] == [cel.OP_CONST, cel.OP_LOAD, cel.OP_CONST, cel.OP_DIV, cel.OP_MUL, cel.OP_QFLOAT]
    assert low[0] == (cel.OP_CONST, 3.0 * 2 ** 20)
    with pytest.raises(cel.CELError):  # Quantity("three") errors on the branch taken, whatever the clock
        cel.lower_usage(ast, pod=PODS["bad-annotation"], node=NODE, container={})
    low = cel.lower_usage(cel.compile(EXPR["unix"]), pod=PODS["plain"], node=NODE, container={})
    assert (cel.OP_CONST, created_ns(PODS["plain"]) / 1e9) in low and (cel.OP_LOAD, cel.IN_NOW_S) in low
    capped = cel.lower_usage(cel.compile(EXPR["capped"]), pod=PODS["plain"], node=NODE, container={})
    assert [op for op, _ in capped][-1] == cel.OP_SELECT and cel.OP_LT in [op for op, _ in capped]
    # SinceSecond(pod) is the same call
    assert cel.lower_usage(cel.compile('Quantity("1Mi") * (SinceSecond(pod) / 60.0)'), pod=PODS["plain"]) == \
        cel.lower_usage(cel.compile(EXPR["ramp"]), pod=PODS["plain"])
    assert cel.lower_usage(cel.compile("UnixSecond(Now())"), pod=PODS["plain"]) == [(cel.OP_LOAD, cel.IN_NOW_S)]


def test_double_on_the_left_is_the_evaluators_answer():
    """The user guide's own example has the double on the left; the evaluator has no
    `double * Quantity` overload, so the value is 0 — and so is the lowering."""
    expr = '(pod.SinceSecond() / 60.0) * Quantity("1Mi")'
    with pytest.raises(cel.CELError):
        cel.evaluate_float64(expr, pod=PODS["plain"], env=cel.Env(now_ns=T0))
    prog = UsageProgram(*load_usage_yaml(usage_doc("left", "100m", "XX").replace("{value: XX}", "{expression: '" + expr + "'}")))
    assert prog.container_program(PODS["plain"], "c0", "memory", NODE) == 0.0
    assert prog.container_value(PODS["plain"], "c0", "memory", NODE) == 0.0


def _program_of(expr):
    return UsageProgram(*load_usage_yaml(usage_doc("x", "1m", "XX").replace("{value: XX}", '{expression: "' +
                                                                              expr.replace('"', '\\"') + '"}')))


@pytest.mark.parametrize("expr,word", [
    ('Quantity("1m") * Rand()', "Rand"),
    ('pod.Usage("cpu")', "Usage"),
    ('pod.CumulativeUsage("cpu") * 2.0', "CumulativeUsage"),
    ('node.StartedContainersTotal()', "StartedContainersTotal"),
    ('Now() - pod.metadata.creationTimestamp', r"Now\(\)"),
    ('Quantity("1m") * SinceSecond(container)', "SinceSecond of something other"),
])
def test_refused_at_compile(expr, word):
    """What the expression's text alone rules out, when the UsageProgram is built."""
    with pytest.raises(UsageCompileError, match=word):
        _program_of(expr)


SINCE = "pod.SinceSecond()"


@pytest.mark.parametrize("expr,word", [
    (f'Quantity("1m") * {SINCE} * 2', r"Quantity \* int"),
    (f'Quantity("1m") * {SINCE} / 2', r"Quantity / int"),
    (f'Quantity("1m") * {SINCE} < Quantity("1") ? Quantity("1m") : Quantity("2m")', "comparison"),
    (f'{SINCE} < 5.0 ? Quantity("1m") : Quantity("x")', "error that depends"),
    (" + ".join([SINCE] * 40), "64 ops"),
    ("(" * 9 + SINCE + "".join(f" + {SINCE})" for _ in range(9)), None),  # left-nested: shallow, accepted
    (SINCE + "".join(f" + ({SINCE}" for _ in range(9)) + ")" * 9, "depth"),
])
def test_refused_for_the_pod(expr, word):
    p = _program_of(expr)  # nothing the expression's text alone rules out
    if word is None:
        assert len(usage_columns_dyn(p, [PODS["plain"]], {"node-0": NODE})[6]) == 1
        return
    with pytest.raises(UsageCompileError, match=word):
        usage_columns_dyn(p, [PODS["plain"]], {"node-0": NODE})


def _dyn_docs():
    return "\n---\n".join([
        usage_doc("ramps", EXPR["capped"], EXPR["annotated"], match_names=["pod-1", "pod-2", "pod-3", "pod-4"]),
        usage_doc("rest", "100m", EXPR["ramp"]),
    ])


def test_columns_intern_programs():
    pods = []
    for i in range(8):
        p = _pod(ann={ANN: "3Mi"} if i in (1, 2) else {ANN: "4Mi"} if i == 3 else None)
        p["metadata"]["name"] = f"pod-{i}"
        if i >= 6:
            p["spec"]["containers"].append({"name": "c1"})
        pods.append(p)
    prog = UsageProgram(*load_usage_yaml(_dyn_docs()))
    with pytest.raises(UsageCompileError, match="usage_columns_dyn"):
        usage_columns(prog, pods, {"node-0": NODE})
    keys, cv, mv, mixed, ckeys, cprogs, mprogs, ops = usage_columns_dyn(prog, pods, {"node-0": NODE})
    assert list(cv) == [0.1] and list(mv) == [5.0 * 2 ** 20]          # "rest"'s cpu; the annotation's fallback (pod-4)
    assert len(cprogs) == 1 and len(mprogs) == 3                        # capped; ramp, 3Mi ramp, 4Mi ramp
    assert keys[1] == keys[2] and keys[1] != keys[3]                    # one program per op bytes
    cid, mid, nc = keys & 0x3FFF, (keys >> 14) & 0x3FFF, keys >> 28
    assert list(nc) == [1, 1, 1, 1, 1, 1, 2, 2] and len(mixed) == 0 and len(ckeys) == 0
    assert list(cid) == [0, 1, 1, 1, 1, 0, 0, 0]                        # id >= len(cv): program id - len(cv)
    assert mid[4] == 0 and set(mid) - {0} == {1, 2, 3}
    # the tables index the op array; running an entry gives the pod's value
    first, n = mprogs[mid[1] - len(mv)]
    entry = [(int(o["op"]), int(o["arg"]) if o["op"] == cel.OP_LOAD else float(o["value"])) for o in ops[first:first + n]]
    assert cel.run_usage_program(entry, T0, created_ns(pods[1]), None) == \
        pytest.approx(restate("annotated", T0, pods[1], NODE), rel=REL_TOL)
    assert all(int(f) + int(k) <= len(ops) for f, k in list(cprogs) + list(mprogs))


def test_mixed_pods_share_the_id_space():
    """Containers with different programs: a mixed entry whose ckeys carry program ids."""
    docs = "\n---\n".join([usage_doc("a", EXPR["capped"], EXPR["ramp"], containers=["c0"]),
                           usage_doc("b", "250m", EXPR["base_ramp"])])
    p = _pod()
    p["spec"]["containers"].append({"name": "c1"})
    keys, cv, mv, mixed, ckeys, cprogs, mprogs, ops = usage_columns_dyn(UsageProgram(*load_usage_yaml(docs)), [p, p],
                                                                        {"node-0": NODE})
    assert list(keys) == [0, 0] and list(mixed) == [0, 2] and len(ckeys) == 2
    assert list(cv) == [0.25] and len(cprogs) == 1 and len(mprogs) == 2 and list(mv) == [0.0]
    assert [int(k) & 0x3FFF for k in ckeys] == [1, 0] and [(int(k) >> 14) & 0x3FFF for k in ckeys] == [1, 2]


def test_id_space_limit_counts_programs():
    pods = []
    for i in range(16385):
        p = _pod(ann={ANN: f"{i + 1}Ki"})
        p["metadata"]["name"] = f"p{i}"
        pods.append(p)
    prog = UsageProgram(*load_usage_yaml(usage_doc("all", "1m", EXPR["annotated"])))
    with pytest.raises(UsageCompileError, match="16384"):
        usage_columns_dyn(prog, pods, {})


def test_static_program_gives_usage_columns():
    cl = W.make_cluster("C4", 30, 600, seed=21)
    pods = cl.pods.materialize()
    prog = UsageProgram(*load_usage_yaml(open(GOLDEN).read()))
    want = usage_columns(prog, pods)
    got = usage_columns_dyn(prog, pods)
    for a, b in zip(want, got[:5]):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert got[5].shape == (0, 2) and got[6].shape == (0, 2) and len(got[7]) == 0


def test_interpreter_ops():
    run = lambda ops: cel.run_usage_program(ops, T0, T0 - 10**9, None)  # noqa: E731
    C, L = cel.OP_CONST, cel.OP_LOAD
    assert run([(C, 7.0), (C, 2.0), (cel.OP_SUB, 0)]) == 5.0 and run([(C, 7.0), (C, 2.0), (cel.OP_DIV, 0)]) == 3.5
    assert run([(C, 1.0), (C, 2.0), (cel.OP_LT, 0)]) == 1.0 and run([(C, 2.0), (C, 2.0), (cel.OP_LT, 0)]) == 0.0
    assert run([(C, 2.0), (C, 2.0), (cel.OP_LE, 0)]) == 1.0 and run([(C, 2.0), (C, 2.0), (cel.OP_GE, 0)]) == 1.0
    assert run([(C, 3.0), (C, 2.0), (cel.OP_GT, 0)]) == 1.0
    assert run([(C, 1.0), (C, 10.0), (C, 20.0), (cel.OP_SELECT, 0)]) == 10.0
    assert run([(C, 0.0), (C, 10.0), (C, 20.0), (cel.OP_SELECT, 0)]) == 20.0
    assert run([(C, 0.15), (cel.OP_QFLOAT, 0)]) == 1500000000 * 1e-9 == 1.5  # the x10 of newQuantityFromFloat64
    assert run([(C, 1e30), (cel.OP_QFLOAT, 0)]) == -(2.0 ** 63) * 1e-9
    assert run([(C, math.nan), (cel.OP_QFLOAT, 0)]) == -(2.0 ** 63) * 1e-9
    assert run([(L, cel.IN_POD_SINCE)]) == 1.0 and run([(L, cel.IN_NOW_S)]) == T0 / 1e9
    assert run([(L, cel.IN_NODE_CREATED)]) == cel.zero_time_unix_second()
    with pytest.raises(ValueError):
        run([(L, cel.IN_POD_CPU)])

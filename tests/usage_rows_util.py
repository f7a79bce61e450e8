"""Shared by test_usage_rows.py / test_gpu_usage_rows.py: the usage CRs, seeded batches of pod
changes, and a pure-Python model of the engine's usage tables that applies UsageTable.rows()
results (appends, then rows) and resolves every pod through them."""
import copy
import os

import numpy as np

from kwok_amd.host import cel
from kwok_amd.host.usage import UsageProgram, load_usage_yaml
from tests.usage_dyn_util import ANN, EXPR, usage_doc

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(__file__)), "kwok_amd", "metrics", "usage-from-annotation.yaml")
CPU_ANN, MEM_ANN = "kwok.x-k8s.io/usage-cpu", "kwok.x-k8s.io/usage-memory"

# tests/test_usage.py's EXTRA, for a few pod names: container-0 evaluates apart from the others
def _named(name):
    return f"""
apiVersion: kwok.x-k8s.io/v1alpha1
kind: ResourceUsage
metadata:
  name: {name}
  namespace: default
spec:
  usages:
  - containers: [container-0]
    usage:
      cpu: {{value: 250m}}
      memory: {{value: 64Mi}}
  - usage:
      cpu: {{value: "2"}}
"""


MIXED_NAMES = ("mixed-a", "mixed-b", "mixed-c", "mixed-d", "mixed-e", "mixed-f")
STATIC_DOCS = "\n---\n".join([open(GOLDEN).read()] + [_named(n) for n in MIXED_NAMES])
# pods of namespace "ramp" read the clock (the memory ramp of tests/test_gpu_usage_dynamic.py); the rest as above
RAMP_DOC = usage_doc("ramps", EXPR["capped"], EXPR["annotated"], namespaces=["ramp"])
DYN_DOCS = "\n---\n".join([RAMP_DOC, STATIC_DOCS])


def program(dyn: bool) -> UsageProgram:
    return UsageProgram(*load_usage_yaml(DYN_DOCS if dyn else STATIC_DOCS))


def stamp(ns: int) -> str:
    import datetime
    return datetime.datetime.fromtimestamp(ns // 10**9, datetime.timezone.utc).strftime("%Y-%m-%dT%H:%M:%SZ")


T0 = 1_700_000_000 * 10**9


def make_pods(n: int, node_of):
    """n pods named pod-<i> of the default namespace, 1..3 containers, some annotated."""
    pods = []
    for i in range(n):
        md = {"name": f"pod-{i}", "namespace": "default", "creationTimestamp": stamp(T0 - (i * 37 % 2000) * 10**9)}
        if i % 3 == 0:
            md["annotations"] = {CPU_ANN: f"{100 + 50 * (i % 4)}m", MEM_ANN: f"{1 + i % 2}Mi"}
        pods.append({"metadata": md, "spec": {"nodeName": f"node-{node_of[i]}",
                                              "containers": [{"name": f"container-{c}"} for c in range(1 + i % 3)]}})
    return pods


def batch(rng, pods, t: int, n_rows: int, programs: bool, kinds=("replace", "edit", "mixed", "count", "new")):
    """One batch of changes of batch number t: -> (slots, new pods, reset flags, created_ns or None).
    replace: another pod under a new name (RESET, a new creation time); edit: the cpu annotation of
    the same pod, from a few values; new: an annotation value nobody had (a new constant); mixed: the
    slot's pod becomes one of MIXED_NAMES with 2..4 containers, or a mixed pod a plain one again
    (RESET); count: the same pod with one container more or fewer; with `programs`, some replacements
    land in the namespace whose usages read the clock."""
    slots = rng.choice(len(pods), size=n_rows, replace=False)
    out, resets, created = [], [], []
    for k, s in enumerate(slots):
        p = copy.deepcopy(pods[int(s)])
        md = p["metadata"]
        kind = kinds[int(rng.integers(len(kinds)))]
        reset, cr = False, None
        if kind == "replace":
            cr = T0 + (t * 1000 + k) * 10**9 - 1500 * 10**9
            md.update(name=f"r{t}-{int(s)}", creationTimestamp=stamp(cr),
                      namespace="ramp" if programs and rng.integers(2) else "default")
            md.pop("annotations", None)
            if rng.integers(2):
                md["annotations"] = {CPU_ANN: f"{100 + 50 * int(rng.integers(4))}m", ANN: f"{1 + int(rng.integers(3))}Mi"}
            p["spec"]["containers"] = [{"name": f"container-{c}"} for c in range(1 + int(rng.integers(3)))]
            reset = True
        elif kind == "edit":
            md.setdefault("annotations", {})[CPU_ANN] = f"{100 + 50 * int(rng.integers(4))}m"
        elif kind == "new":
            md.setdefault("annotations", {})[CPU_ANN] = f"{1000 + 16 * t + k}m"
            md["annotations"][MEM_ANN] = f"{3000 + 16 * t + k}Ki"
        elif kind == "mixed":
            if md["name"] in MIXED_NAMES:
                md["name"] = f"u{t}-{int(s)}"
            else:
                md.update(name=MIXED_NAMES[int(rng.integers(len(MIXED_NAMES)))], namespace="default")
                p["spec"]["containers"] = [{"name": f"container-{c}"} for c in range(2 + int(rng.integers(3)))]
            reset = True
        elif kind == "count":
            cs = p["spec"]["containers"]
            if len(cs) > 1 and rng.integers(2):
                cs.pop()
            else:
                cs.append({"name": f"container-{len(cs)}"})
        out.append(p)
        resets.append(reset)
        created.append(cr)
    return [int(s) for s in slots], out, resets, created


def _ops_tuple(ops):
    return tuple((int(o["op"]), int(o["arg"]) if o["op"] == cel.OP_LOAD else
                  float(o["value"]) if o["op"] == cel.OP_CONST else 0) for o in ops)


def _norm(v):
    """A value as the tables can hold it: a constant, or a program's (op, operand) tuples; a
    one-op constant program is its constant."""
    if isinstance(v, float):
        return v
    t = tuple((int(op), int(x) if op == cel.OP_LOAD else float(x) if op == cel.OP_CONST else 0) for op, x in v)
    return t[0][1] if len(t) == 1 and t[0][0] == cel.OP_CONST else t


class Model:
    """The engine's usage tables in Python: kwk_usage_config_dyn + kwk_usage_mixed of
    UsageTable.config, then kwk_usage_append / _mixed_append / _set_rows of UsageTable.rows."""

    def __init__(self, cols):
        keys, cv, mv, mixed, ckeys, cp, mp, ops = cols
        self.keys = keys.copy()
        self.const = [list(cv), list(mv)]
        self.progs = [[tuple(x) for x in cp.tolist()], [tuple(x) for x in mp.tolist()]]
        self.ops = ops.copy()
        self.mixed = list(mixed)
        self.ckeys = list(ckeys)

    def apply(self, up):
        for r, (cn, pn) in enumerate((("cpu_values", "cpu_progs"), ("mem_values", "mem_progs"))):
            if len(up[cn]):  # the id rule: constants only while no program exists
                assert not self.progs[0] and not self.progs[1], "a constant appended to tables with programs"
            self.const[r] += list(up[cn])
        self.ops = np.concatenate([self.ops, up["ops"]])
        for r, pn in enumerate(("cpu_progs", "mem_progs")):
            self.progs[r] += [tuple(x) for x in up[pn].tolist()]
            assert len(self.const[r]) + len(self.progs[r]) <= 1 << 14
            assert all(f + n <= len(self.ops) for f, n in self.progs[r])
        self.mixed += list(up["mixed"])
        self.ckeys += list(up["ckeys"])
        rows = up["rows"]
        assert len(set(rows["slot"].tolist())) == len(rows)
        self.keys[rows["slot"]] = rows["usage_key"]

    def value(self, r, vid):
        if vid < len(self.const[r]):
            return float(self.const[r][vid])
        first, n = self.progs[r][vid - len(self.const[r])]
        return _norm([(op, x) for op, x in _ops_tuple(self.ops[first:first + n])])

    def resolve(self, slot):
        """[(cpu, memory)] per container of the pod in `slot`."""
        k = int(self.keys[slot])
        if k >> 28:
            return [(self.value(0, k & 0x3FFF), self.value(1, (k >> 14) & 0x3FFF))] * (k >> 28)
        first, count = self.mixed[2 * k], self.mixed[2 * k + 1]
        return [(self.value(0, int(c) & 0x3FFF), self.value(1, (int(c) >> 14) & 0x3FFF)) for c in self.ckeys[first:first + count]]

    def check(self, prog: UsageProgram, pods, nodes=None):
        for i, p in enumerate(pods):
            node = (nodes or {}).get(p["spec"].get("nodeName", ""))
            want = [(_norm(c), _norm(m)) for c, m in prog.pod_container_programs(p, node)]
            assert self.resolve(i) == want, (i, p["metadata"]["name"], self.resolve(i), want)

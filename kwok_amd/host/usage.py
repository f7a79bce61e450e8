"""ResourceUsage / ClusterResourceUsage compilation (host side of kwk_usage).

Restates the per-container resolution of pkg/kwok/server/metrics_resource_usage.go:
``getResourceUsage`` (:226-250: a namespaced ResourceUsage named like the pod wins, else the
first ClusterResourceUsage whose ObjectSelector matches *and* has an entry for the
container), ``findUsageInUsages`` (:252-264: the entry listing the container, else the first
entry with no containers) and ``evaluateContainerResourceUsage`` (:136-168: a static
``value`` via AsApproximateFloat64, or a CEL ``expression`` evaluated with the pod, its node
and the container bound — kwok_amd/host/cel.py; any error -> 0).

A usage expression that does not read the clock is evaluated once per pod variant at ingest
and interned as a constant.  One that reads it through ``pod.SinceSecond()``,
``node.SinceSecond()`` or ``Now().UnixSecond()`` (a usage that ramps with the pod's age) is
partially evaluated for the pod — everything clock-free folds, cel.lower_usage — and the rest
becomes a postfix program the usage kernel runs at every scrape's ``now``
(``kwk_usage_config_dyn``, ``usage_columns_dyn``).  ``Rand``, other usages (``Usage``,
``CumulativeUsage``, ``StartedContainersTotal``), any other use of ``Now()`` and the forms
the program format cannot express (clock-dependent Quantity x int, Quantity comparisons,
errors under a clock-dependent condition, more than 64 ops or 8 stack entries) are refused with
``UsageCompileError`` rather than frozen.  The device gets, per pod, either one interned
cpu / memory value id (a constant or a program) and the number of containers that carry it,
or — when the pod's containers differ — a {first, count} entry into a per-container key table
(``kwk_usage_mixed``); per-node sums and all cumulative integrators run in ``usage_kernel`` /
its clock-dependent variant.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import yaml

from . import cel
from .abi import USAGE_OP_DTYPE
from .quantity import parse_quantity_or_none


class UsageCompileError(ValueError):
    pass


@dataclass
class UsageValue:
    value: Optional[str] = None        # resource.Quantity text
    expression: Optional[str] = None

    def compile(self):
        if self.value is not None:
            q = parse_quantity_or_none(str(self.value))
            if q is None:
                raise UsageCompileError(f"invalid quantity {self.value!r}")
            return ("const", q)
        if self.expression is not None:
            try:
                ast = cel.compile(self.expression)
            except cel.CELSyntaxError:
                return ("const", 0.0)  # Compile fails -> 0 (metrics_resource_usage.go:150-155)
            bad = cel.usage_refused_call(ast)
            if bad is not None:
                raise UsageCompileError(f"usage expression calls {bad}: {self.expression!r}")
            if cel.usage_reads_clock(ast):
                bad = cel.usage_bad_clock(ast)
                if bad is not None:
                    raise UsageCompileError(f"usage expression reads {bad}: {self.expression!r}")
                return ("dyn", self.expression, ast)
            return ("cel", self.expression)
        return ("const", 0.0)


@dataclass
class UsageEntry:
    containers: List[str]
    usage: Optional[Dict[str, UsageValue]]


@dataclass
class ResourceUsage:
    name: str
    namespace: str
    usages: List[UsageEntry]


@dataclass
class ClusterResourceUsage:
    name: str
    match_namespaces: List[str] = field(default_factory=list)
    match_names: List[str] = field(default_factory=list)
    usages: List[UsageEntry] = field(default_factory=list)
    has_selector: bool = False

    def match(self, name: str, namespace: str) -> bool:
        """ObjectSelector.Match (internalversion/object_selector.go:35-47)."""
        if not self.has_selector:
            return True
        if self.match_namespaces and namespace not in self.match_namespaces:
            return False
        if self.match_names and name not in self.match_names:
            return False
        return True


def _entries(spec) -> List[UsageEntry]:
    out = []
    for u in spec.get("usages") or []:
        usage = None
        if u.get("usage") is not None:
            usage = {k: UsageValue(value=None if v.get("value") is None else str(v.get("value")),
                                   expression=v.get("expression")) for k, v in u["usage"].items()}
        out.append(UsageEntry(containers=list(u.get("containers") or []), usage=usage))
    return out


def load_usage_yaml(*texts: str):
    rus, crus = [], []
    for t in texts:
        for doc in yaml.safe_load_all(t):
            if not doc:
                continue
            md = doc.get("metadata") or {}
            spec = doc.get("spec") or {}
            if doc.get("kind") == "ResourceUsage":
                rus.append(ResourceUsage(md.get("name", ""), md.get("namespace", ""), _entries(spec)))
            elif doc.get("kind") == "ClusterResourceUsage":
                sel = spec.get("selector")
                crus.append(ClusterResourceUsage(md.get("name", ""),
                                                 list((sel or {}).get("matchNamespaces") or []),
                                                 list((sel or {}).get("matchNames") or []), _entries(spec),
                                                 has_selector=sel is not None))
    return rus, crus


def find_usage(container: str, usages: List[UsageEntry]) -> Optional[UsageEntry]:
    """findUsageInUsages (metrics_resource_usage.go:252-264)."""
    default = None
    for u in usages:
        if len(u.containers) == 0 and default is None:
            default = u
            continue
        if container in u.containers:
            return u
    return default


class UsageProgram:
    RESOURCES = ("cpu", "memory")

    def __init__(self, resource_usages: Sequence[ResourceUsage], cluster_resource_usages: Sequence[ClusterResourceUsage]):
        self.rus = list(resource_usages)
        self.crus = list(cluster_resource_usages)
        self._compiled = {}
        for group in [r.usages for r in self.rus] + [c.usages for c in self.crus]:
            for e in group:
                for k, v in (e.usage or {}).items():
                    self._compiled[id(v)] = v.compile()

    def _entry(self, pod_name: str, ns: str, container: str) -> Optional[UsageEntry]:
        for r in self.rus:  # getResourceUsage (:226-250)
            if r.name == pod_name and r.namespace == ns:
                return find_usage(container, r.usages)
        for c in self.crus:
            if not c.match(pod_name, ns):
                continue
            u = find_usage(container, c.usages)
            if u is not None:
                return u
        return None

    def container_value(self, pod: dict, container: str, resource: str, node: Optional[dict] = None) -> float:
        """evaluateContainerResourceUsage (:136-168) for the container named `container` (the
        first with that name, as containerResourceUsage's slices.Find, :111-134), where it does
        not depend on the clock."""
        v = self.container_program(pod, container, resource, node)
        if not isinstance(v, float):
            raise UsageCompileError(f"the {resource} usage of container {container!r} of pod "
                                    f"{(pod.get('metadata') or {}).get('name', '')!r} depends on the clock: "
                                    "use usage_columns_dyn")
        return v

    def container_program(self, pod: dict, container: str, resource: str, node: Optional[dict] = None):
        """container_value, or — for an expression that reads the clock — its program for this pod
        (a tuple of (op, operand), cel.lower_usage)."""
        md = pod.get("metadata") or {}
        u = self._entry(md.get("name", ""), md.get("namespace", ""), container)
        if u is None or u.usage is None:
            return 0.0
        v = u.usage.get(resource)
        if v is None:
            return 0.0
        c = self._compiled[id(v)]
        if c[0] == "const":
            return c[1]
        cobj = next((x for x in (pod.get("spec") or {}).get("containers") or [] if x.get("name", "") == container), {})
        if c[0] == "dyn":
            try:
                r = cel.lower_usage(c[2], pod=pod, node=node or {}, container=cobj)
            except cel.CELError:
                return 0.0  # an error whatever the clock says
            except cel.UsageLowerError as e:
                raise UsageCompileError(f"usage expression {c[1]!r}: {e}")
            return r if isinstance(r, float) else tuple(r)
        try:
            return cel.evaluate_float64(c[1], node=node or {}, pod=pod, container=cobj)
        except cel.CELError:
            return 0.0

    def pod_container_values(self, pod: dict, node: Optional[dict] = None) -> List[Tuple[float, float]]:
        """(cpu, memory) of each of the pod's containers, in spec order."""
        names = [c.get("name", "") for c in (pod.get("spec") or {}).get("containers") or []]
        return [(self.container_value(pod, n, "cpu", node), self.container_value(pod, n, "memory", node)) for n in names]

    def pod_container_programs(self, pod: dict, node: Optional[dict] = None) -> List[tuple]:
        """pod_container_values where a value may be a program (container_program)."""
        names = [c.get("name", "") for c in (pod.get("spec") or {}).get("containers") or []]
        return [(self.container_program(pod, n, "cpu", node), self.container_program(pod, n, "memory", node))
                for n in names]


def usage_columns(program: UsageProgram, pods: Sequence[dict], nodes: Optional[Dict[str, dict]] = None):
    """-> usage_key u32[n], cpu_values f64[], mem_values f64[] (interned), and the mixed tables
    (kwk_usage_mixed): mixed u32[2 * n_mixed] = {first, count}, ckeys u32[n_containers].
    A pod whose containers all evaluate alike (1..15 of them) is one key x its container count;
    any other pod (containers differ, none, or more than 15) gets a mixed entry."""
    cpu_ids: Dict[float, int] = {}
    mem_ids: Dict[float, int] = {}
    keys = np.zeros(len(pods), dtype=np.uint32)
    mixed: List[int] = []
    ckeys: List[int] = []
    memo: Dict[tuple, int] = {}

    def vid(c, m):
        ci = cpu_ids.setdefault(c, len(cpu_ids))
        mi = mem_ids.setdefault(m, len(mem_ids))
        if ci >= 1 << 14 or mi >= 1 << 14:
            raise UsageCompileError("more than 16384 distinct usage values")
        return ci | (mi << 14)

    for i, p in enumerate(pods):
        node = (nodes or {}).get((p.get("spec") or {}).get("nodeName", ""))
        vals = program.pod_container_values(p, node)
        if 1 <= len(vals) <= 15 and all(v == vals[0] for v in vals):
            keys[i] = vid(*vals[0]) | (len(vals) << 28)
            continue
        t = tuple(vals)
        m = memo.get(t)
        if m is None:
            m = memo[t] = len(mixed) // 2
            mixed += [len(ckeys), len(vals)]
            ckeys += [vid(c, mm) for c, mm in vals]
        keys[i] = m
    cv = np.array(sorted(cpu_ids, key=cpu_ids.get), dtype=np.float64) if cpu_ids else np.zeros(1)
    mv = np.array(sorted(mem_ids, key=mem_ids.get), dtype=np.float64) if mem_ids else np.zeros(1)
    return keys, cv, mv, np.array(mixed, dtype=np.uint32), np.array(ckeys, dtype=np.uint32)


OP_DTYPE = USAGE_OP_DTYPE  # kwk_metric_op


def _pack_ops(prog) -> bytes:
    a = np.zeros(len(prog), dtype=OP_DTYPE)
    for i, (op, x) in enumerate(prog):
        a[i] = (op, int(x), 0.0) if op == cel.OP_LOAD else (op, 0, float(x) if op == cel.OP_CONST else 0.0)
    return a.tobytes()


def usage_columns_dyn(program: UsageProgram, pods: Sequence[dict], nodes: Optional[Dict[str, dict]] = None):
    """usage_columns for programs with clock-dependent expressions (kwk_usage_config_dyn):
    -> usage_key, cpu_values, mem_values, mixed, ckeys as usage_columns, then
    cpu_progs u32[n_cpu_progs, 2], mem_progs u32[n_mem_progs, 2] = {first_op, n_ops} and
    ops (OP_DTYPE).  A value id v < len(cpu_values) is the constant cpu_values[v], an id
    len(cpu_values) <= v < len(cpu_values) + len(cpu_progs) is program v - len(cpu_values); memory
    alike; constants and programs share the 14-bit id space.  Programs are interned by their op
    bytes.  Without a clock-dependent value this is usage_columns with empty program tables."""
    return UsageTable(program).config(pods, nodes)


MAX_IDS = 1 << 14          # value ids per resource (constants and programs)
MAX_MIXED = 0x0FFFFFFF     # mixed entries (kUKeyMixedIndex)


class UsageTable:
    """The interning state behind usage_columns_dyn, kept: the constants' ids, the programs' ids
    by their op bytes, the mixed entries by their containers' values.  ``config`` computes a full
    configuration (kwk_usage_config_dyn + kwk_usage_mixed); ``rows`` then turns changed pods into
    kwk_usage_set_rows records plus whatever has to be appended to the engine's tables first
    (kwk_usage_append, kwk_usage_mixed_append), with ids that continue the configuration's."""

    def __init__(self, program: UsageProgram):
        self.program = program
        self.const_ids = ({}, {})   # per resource: constant -> value id
        self.prog_ids = ({}, {})    # per resource: program op bytes -> value id
        self.n_const = [0, 0]
        self.n_progs = [0, 0]
        self.spans: Dict[bytes, Tuple[int, int]] = {}  # op bytes -> (first_op, n_ops) in the op table
        self.n_ops = 0
        self.memo: Dict[tuple, int] = {}               # a mixed pod's container values -> mixed index
        self.n_mixed = 0
        self.n_ckeys = 0

    def config(self, pods: Sequence[dict], nodes: Optional[Dict[str, dict]] = None):
        """-> usage_columns_dyn's eight arrays for `pods`; the table starts over from them."""
        program = self.program
        PROG = 1 << 20  # provisional ids of programs, rebased past the constants at the end
        ids = ({}, {})       # per resource: constant -> id
        pids = ({}, {})      # per resource: program bytes -> program index
        ptab = ([], [])      # per resource: [first_op, n_ops]
        oplist: List[bytes] = []
        interned: Dict[bytes, Tuple[int, int]] = {}
        ukeys: List[tuple] = []   # (cpu id, mem id, containers) or (mixed index,)
        mixed: List[int] = []
        cks: List[tuple] = []
        memo: Dict[tuple, int] = {}

        def one(r, v):
            if isinstance(v, float):
                return ids[r].setdefault(v, len(ids[r]))
            b = _pack_ops(v)
            i = pids[r].get(b)
            if i is None:
                span = interned.get(b)
                if span is None:
                    span = interned[b] = (len(oplist), len(v))
                    oplist.append(b)
                i = pids[r][b] = len(ptab[r])
                ptab[r].append(span)
            return PROG | i

        def vid(c, m):
            ci, mi = one(0, c), one(1, m)
            for r in (0, 1):
                if len(ids[r]) + len(ptab[r]) > MAX_IDS:
                    raise UsageCompileError("more than 16384 distinct usage values and programs")
            return ci, mi

        for p in pods:
            node = (nodes or {}).get((p.get("spec") or {}).get("nodeName", ""))
            vals = program.pod_container_programs(p, node)
            if 1 <= len(vals) <= 15 and all(v == vals[0] for v in vals):
                ukeys.append(vid(*vals[0]) + (len(vals),))
                continue
            t = tuple(vals)
            m = memo.get(t)
            if m is None:
                m = memo[t] = len(mixed) // 2
                mixed += [len(cks), len(vals)]
                cks += [vid(c, mm) for c, mm in vals]
            ukeys.append((m,))
        cv = np.array(sorted(ids[0], key=ids[0].get), dtype=np.float64) if ids[0] else np.zeros(1)
        mv = np.array(sorted(ids[1], key=ids[1].get), dtype=np.float64) if ids[1] else np.zeros(1)
        if len(cv) + len(ptab[0]) > MAX_IDS or len(mv) + len(ptab[1]) > MAX_IDS:
            raise UsageCompileError("more than 16384 distinct usage values and programs")

        def final(ci, mi):
            ci = len(cv) + (ci ^ PROG) if ci & PROG else ci
            mi = len(mv) + (mi ^ PROG) if mi & PROG else mi
            return ci | (mi << 14)

        keys = np.array([k[0] if len(k) == 1 else final(k[0], k[1]) | (k[2] << 28) for k in ukeys], dtype=np.uint32)
        ckeys = np.array([final(c, m) for c, m in cks], dtype=np.uint32)
        # the op array: each interned program's ops, in order; spans were recorded in programs, so
        # turn them into op offsets
        firsts, pos = [], 0
        for b in oplist:
            firsts.append(pos)
            pos += len(b) // OP_DTYPE.itemsize
        ops = np.frombuffer(b"".join(oplist), dtype=OP_DTYPE).copy() if oplist else np.zeros(0, dtype=OP_DTYPE)
        tabs = [np.array([[firsts[f], n] for f, n in t], dtype=np.uint32).reshape(-1, 2) for t in ptab]
        # keep the state, in the final ids (an empty constant table is the one constant 0)
        for r, vals in ((0, cv), (1, mv)):
            self.const_ids[r].clear()
            self.const_ids[r].update(ids[r] if ids[r] else {0.0: 0})
            self.n_const[r] = len(vals)
            self.n_progs[r] = len(ptab[r])
            self.prog_ids[r].clear()
            self.prog_ids[r].update({b: len(vals) + i for b, i in pids[r].items()})
        self.spans = {b: (firsts[f], n) for b, (f, n) in interned.items()}
        self.n_ops = pos
        self.memo = memo
        self.n_mixed = len(mixed) // 2
        self.n_ckeys = len(cks)
        return keys, cv, mv, np.array(mixed, dtype=np.uint32), ckeys, tabs[0], tabs[1], ops

    def rows(self, slots: Sequence[int], pods: Sequence[dict], nodes: Optional[Dict[str, dict]] = None, reset=False,
             created_ns=None) -> dict:
        """The pods now in `slots` -> {"rows": kwk_usage_row records (abi.USAGE_ROW_DTYPE), and what
        kwk_usage_append / kwk_usage_mixed_append must add first: "cpu_values", "mem_values",
        "cpu_progs", "mem_progs" ([first_op, n_ops] in the whole op table), "ops", "mixed" ({first,
        count} pairs, flat), "ckeys"}.  reset: one flag or one per row (KWK_USAGE_ROW_RESET: another
        pod took the slot); created_ns: per row, the slot's new creation time or None to keep it.
        Ids follow kwk_usage_config_dyn's rule: a new constant gets the next constant id while the
        table has no program of either resource; after that it travels as a one-op constant
        program.  A UsageCompileError (16384 ids, 2^28 - 1 mixed entries, what UsageProgram
        refuses) leaves the table as it was."""
        from .abi import USAGE_ROW_CREATED, USAGE_ROW_DTYPE, USAGE_ROW_RESET
        if len(slots) != len(pods):
            raise ValueError("one pod per slot")
        new_const = ([], [])
        new_progs = ([], [])
        new_ops: List[bytes] = []
        new_mixed: List[int] = []
        new_ckeys: List[int] = []
        undo: List[tuple] = []  # (dict, key) entries added
        saved = (list(self.n_const), list(self.n_progs), self.n_ops, self.n_mixed, self.n_ckeys)

        def put(d, k, v):
            d[k] = v
            undo.append((d, k))
            return v

        def one(r, v):
            if isinstance(v, float):
                i = self.const_ids[r].get(v)
                if i is not None:
                    return i
                if self.n_progs[0] + self.n_progs[1] == 0:
                    if self.n_const[r] >= MAX_IDS:
                        raise UsageCompileError("more than 16384 distinct usage values and programs")
                    new_const[r].append(v)
                    self.n_const[r] += 1
                    return put(self.const_ids[r], v, self.n_const[r] - 1)
                v = ((cel.OP_CONST, v),)  # ids below the constants' count are taken: a one-op program
            b = _pack_ops(v)
            i = self.prog_ids[r].get(b)
            if i is None:
                if self.n_const[r] + self.n_progs[r] >= MAX_IDS:
                    raise UsageCompileError("more than 16384 distinct usage values and programs")
                span = self.spans.get(b)
                if span is None:
                    span = put(self.spans, b, (self.n_ops, len(v)))
                    self.n_ops += len(v)
                    new_ops.append(b)
                new_progs[r].append(span)
                self.n_progs[r] += 1
                i = put(self.prog_ids[r], b, self.n_const[r] + self.n_progs[r] - 1)
            return i

        rows = np.zeros(len(slots), dtype=USAGE_ROW_DTYPE)
        try:
            for i, (slot, p) in enumerate(zip(slots, pods)):
                node = (nodes or {}).get((p.get("spec") or {}).get("nodeName", ""))
                vals = self.program.pod_container_programs(p, node)
                if 1 <= len(vals) <= 15 and all(v == vals[0] for v in vals):
                    # (both ids before the key: a constant interned after this pod's program would shift it)
                    ci, mi = one(0, vals[0][0]), one(1, vals[0][1])
                    key = ci | (mi << 14) | (len(vals) << 28)
                else:
                    t = tuple(vals)
                    key = self.memo.get(t)
                    if key is None:
                        if self.n_mixed >= MAX_MIXED:
                            raise UsageCompileError("more than 2^28 - 1 mixed usage entries")
                        cks = [one(0, c) | (one(1, m) << 14) for c, m in vals]
                        key = put(self.memo, t, self.n_mixed)
                        self.n_mixed += 1
                        new_mixed += [self.n_ckeys, len(vals)]
                        self.n_ckeys += len(vals)
                        new_ckeys += cks
                flags = USAGE_ROW_RESET if (reset if np.ndim(reset) == 0 else reset[i]) else 0
                created = None if created_ns is None else created_ns[i]
                if created is not None:
                    flags |= USAGE_ROW_CREATED
                rows[i] = (slot, key, flags, 0, 0 if created is None else int(created))
        except Exception:
            for d, k in undo:
                del d[k]
            self.n_const, self.n_progs, self.n_ops, self.n_mixed, self.n_ckeys = saved
            raise
        tabs = [np.array(t, dtype=np.uint32).reshape(-1, 2) for t in new_progs]
        ops = np.frombuffer(b"".join(new_ops), dtype=OP_DTYPE).copy() if new_ops else np.zeros(0, dtype=OP_DTYPE)
        return {"rows": rows, "cpu_values": np.array(new_const[0], dtype=np.float64),
                "mem_values": np.array(new_const[1], dtype=np.float64), "cpu_progs": tabs[0], "mem_progs": tabs[1],
                "ops": ops, "mixed": np.array(new_mixed, dtype=np.uint32), "ckeys": np.array(new_ckeys, dtype=np.uint32)}

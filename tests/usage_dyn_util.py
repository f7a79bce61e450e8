"""Shared by test_usage_dynamic.py / test_gpu_usage_dynamic.py: the fixture ResourceUsage
expressions that read the clock and their restatement by hand.

The restatements do not go through kwok_amd.host.cel: a Quantity literal is the oracle's
(usage_ref.quantity), SinceSecond is metrics_ref._since, Quantity x double is
newQuantityFromFloat64 (pkg/utils/cel/quantity.go:69-72: int64(v * 10e9) nano, Go's amd64
conversion giving INT64_MIN outside the range) followed by AsApproximateFloat64, and
Quantity + Quantity is the sum of the two doubles (exact to a rounding of the larger one).
"""
import calendar
import functools
import re

from oracle import usage_ref
from oracle.metrics_ref import _since

ANN = "kwok.x-k8s.io/usage-ramp"

EXPR = {
    "ramp": 'Quantity("1Mi") * (pod.SinceSecond() / 60.0)',
    "base_ramp": 'Quantity("10Mi") + Quantity("1Ki") * pod.SinceSecond()',
    "capped": 'pod.SinceSecond() < 600.0 ? Quantity("1m") * pod.SinceSecond() : Quantity("600m")',
    "annotated": f'"{ANN}" in pod.metadata.annotations ? Quantity(pod.metadata.annotations["{ANN}"]) * '
                 f'(pod.SinceSecond() / 60.0) : Quantity("5Mi")',
    "node_age": 'Quantity("100m") + Quantity("1m") * (node.SinceSecond() / 3600.0)',
    "unix": 'Quantity("1m") * (Now().UnixSecond() - pod.metadata.creationTimestamp.UnixSecond())',
}


def go_int64(x: float) -> int:
    if x != x or x >= 2.0 ** 63 or x < -2.0 ** 63:
        return -(1 << 63)
    return int(x)


def q_times(q: float, d: float) -> float:
    """Quantity * double, read back as a double."""
    return go_int64(q * d * 10e9) * 1e-9


@functools.lru_cache(maxsize=None)
def Q(s: str) -> float:
    return usage_ref.quantity(s)


def created_ns(obj):
    """creationTimestamp of a pod / node JSON in unix ns, None when unset."""
    ts = ((obj or {}).get("metadata") or {}).get("creationTimestamp")
    if not ts:
        return None
    m = re.fullmatch(r"(\d+)-(\d+)-(\d+)T(\d+):(\d+):(\d+)(?:\.(\d+))?Z", ts)
    secs = calendar.timegm(tuple(int(m.group(i)) for i in range(1, 7)) + (0, 0, 0))
    return secs * 10**9 + int((m.group(7) or "0").ljust(9, "0")[:9])


def _unix_second(ns) -> float:
    """Time.UnixNano() / 1e9; the zero time's UnixNano wraps around int64."""
    if ns is None:
        ns = ((-62135596800 * 10**9 + (1 << 63)) % (1 << 64)) - (1 << 63)
    return float(ns) / 1e9


def restate(name: str, now_ns: int, pod: dict, node: dict) -> float:
    """The value of fixture expression `name` for the pod at now_ns (a Quantity text that is no
    fixture: that value)."""
    if name not in EXPR:
        return Q(name)
    pc, nc = created_ns(pod), created_ns(node)
    if name == "ramp":
        return q_times(Q("1Mi"), _since(now_ns, pc) / 60.0)
    if name == "base_ramp":
        return Q("10Mi") + q_times(Q("1Ki"), _since(now_ns, pc))
    if name == "capped":
        return q_times(Q("1m"), _since(now_ns, pc)) if _since(now_ns, pc) < 600.0 else Q("600m")
    if name == "annotated":
        ann = (pod.get("metadata") or {}).get("annotations") or {}
        if ANN not in ann:
            return Q("5Mi")
        q = Q(str(ann[ANN]))
        if q is None:  # Quantity() of an invalid string errors: the usage is 0
            return 0.0
        return q_times(q, _since(now_ns, pc) / 60.0)
    if name == "node_age":
        return Q("100m") + q_times(Q("1m"), _since(now_ns, nc) / 3600.0)
    if name == "unix":
        return q_times(Q("1m"), float(now_ns) / 1e9 - _unix_second(pc))
    raise KeyError(name)


def usage_doc(name: str, cpu: str, memory: str, containers=(), match_names=(), namespaces=()) -> str:
    """A ClusterResourceUsage document with one usages entry (a fixture expression or a value)."""
    def val(v):
        return f"{{expression: '{v}'}}" if v in EXPR.values() else f"{{value: {v}}}"
    sel = ""
    if match_names or namespaces:
        sel = "  selector:\n" + (f"    matchNames: [{', '.join(match_names)}]\n" if match_names else "") + \
            (f"    matchNamespaces: [{', '.join(namespaces)}]\n" if namespaces else "")
    cs = f"  - containers: [{', '.join(containers)}]\n    usage:\n" if containers else "  - usage:\n"
    return (f"apiVersion: kwok.x-k8s.io/v1alpha1\nkind: ClusterResourceUsage\nmetadata:\n  name: {name}\nspec:\n"
            f"{sel}  usages:\n{cs}      cpu: {val(cpu)}\n      memory: {val(memory)}\n")

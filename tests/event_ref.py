"""Reference for the Events of fired Stages: a restatement of what client-go's recorder hands the
broadcaster, independent of kwok_amd (it imports nothing from the package).

Two layers:

* ``marshal``: Go's encoding/json over structs, driven by field tables transcribed from the
  struct tags of k8s.io/api v0.30.2 core/v1/types.go (Event, ObjectReference, EventSource,
  EventSeries), apimachinery's meta/v1 ObjectMeta, metav1.Time / MicroTime MarshalJSON and
  encoding/json's encode.go (struct fields in declaration order, omitempty's emptiness rule,
  string escaping with escapeHTML on).
* ``make_event`` / ``generate_event``: client-go v0.30.2 tools/record/event.go (makeEvent :478-505,
  generateEvent :331-356) building the struct value that is marshalled.

A struct value is a dict of Go field name -> value; fields that are absent hold their zero value.
"""
from __future__ import annotations

import datetime

# ---- field tables: (Go field, JSON key, omitempty, kind of value)
# kinds: "string", "int", "time" (metav1.Time), "microtime" (metav1.MicroTime), "map" (map[string]string),
# "slice" (a slice this reference never fills), ("struct", TABLE), ("ptr", TABLE), "int64ptr"

OBJECT_META = [  # apimachinery pkg/apis/meta/v1/types.go ObjectMeta
    ("Name", "name", True, "string"),
    ("GenerateName", "generateName", True, "string"),
    ("Namespace", "namespace", True, "string"),
    ("SelfLink", "selfLink", True, "string"),
    ("UID", "uid", True, "string"),
    ("ResourceVersion", "resourceVersion", True, "string"),
    ("Generation", "generation", True, "int"),
    ("CreationTimestamp", "creationTimestamp", True, "time"),  # omitempty never drops a struct
    ("DeletionTimestamp", "deletionTimestamp", True, ("ptr", None)),
    ("DeletionGracePeriodSeconds", "deletionGracePeriodSeconds", True, "int64ptr"),
    ("Labels", "labels", True, "map"),
    ("Annotations", "annotations", True, "map"),
    ("OwnerReferences", "ownerReferences", True, "slice"),
    ("Finalizers", "finalizers", True, "slice"),
    ("ManagedFields", "managedFields", True, "slice"),
]

OBJECT_REFERENCE = [  # core/v1/types.go ObjectReference
    ("Kind", "kind", True, "string"),
    ("Namespace", "namespace", True, "string"),
    ("Name", "name", True, "string"),
    ("UID", "uid", True, "string"),
    ("APIVersion", "apiVersion", True, "string"),
    ("ResourceVersion", "resourceVersion", True, "string"),
    ("FieldPath", "fieldPath", True, "string"),
]

EVENT_SOURCE = [  # core/v1/types.go EventSource
    ("Component", "component", True, "string"),
    ("Host", "host", True, "string"),
]

EVENT_SERIES = [  # core/v1/types.go EventSeries
    ("Count", "count", True, "int"),
    ("LastObservedTime", "lastObservedTime", True, "microtime"),
]

EVENT = [  # core/v1/types.go Event (TypeMeta is inlined: kind, apiVersion)
    ("Kind", "kind", True, "string"),
    ("APIVersion", "apiVersion", True, "string"),
    ("ObjectMeta", "metadata", False, ("struct", OBJECT_META)),
    ("InvolvedObject", "involvedObject", False, ("struct", OBJECT_REFERENCE)),
    ("Reason", "reason", True, "string"),
    ("Message", "message", True, "string"),
    ("Source", "source", True, ("struct", EVENT_SOURCE)),
    ("FirstTimestamp", "firstTimestamp", True, "time"),
    ("LastTimestamp", "lastTimestamp", True, "time"),
    ("Count", "count", True, "int"),
    ("Type", "type", True, "string"),
    ("EventTime", "eventTime", True, "microtime"),
    ("Series", "series", True, ("ptr", EVENT_SERIES)),
    ("Action", "action", True, "string"),
    ("Related", "related", True, ("ptr", OBJECT_REFERENCE)),
    ("ReportingController", "reportingComponent", False, "string"),
    ("ReportingInstance", "reportingInstance", False, "string"),
]


# ---- encoding/json
def go_string(s: str) -> str:
    """encode.go appendString with escapeHTML = true, for valid UTF-8 without control characters
    other than \\n \\r \\t (what the code under test accepts)."""
    out = ['"']
    for ch in s:
        c = ord(ch)
        if ch == '"' or ch == "\\":
            out.append("\\" + ch)
        elif ch == "\n":
            out.append("\\n")
        elif ch == "\r":
            out.append("\\r")
        elif ch == "\t":
            out.append("\\t")
        elif c < 0x20 or ch in "<>&":
            out.append("\\u00%02x" % c)
        elif c == 0x2028 or c == 0x2029:
            out.append("\\u%04x" % c)
        else:
            out.append(ch)
    out.append('"')
    return "".join(out)


def _rfc3339(sec: int) -> str:
    t = datetime.datetime(1970, 1, 1) + datetime.timedelta(seconds=sec)
    return "%04d-%02d-%02dT%02d:%02d:%02dZ" % (t.year, t.month, t.day, t.hour, t.minute, t.second)


def _zero(kind):
    if kind == "string":
        return ""
    if kind == "int":
        return 0
    if isinstance(kind, tuple) and kind[0] == "struct":
        return {}
    return None  # time, microtime (the zero Time), ptr, map, slice


def _is_empty(kind, v) -> bool:
    """encode.go isEmptyValue: false for every struct (Time, MicroTime and nested structs included)."""
    if kind == "string":
        return v == ""
    if kind == "int":
        return v == 0
    if kind in ("map", "slice"):
        return not v
    if kind == "int64ptr" or (isinstance(kind, tuple) and kind[0] == "ptr"):
        return v is None
    return False


def _value(kind, v) -> str:
    if kind == "string":
        return go_string(v)
    if kind == "int":
        return str(int(v))
    if kind in ("time", "microtime"):
        # Time.MarshalJSON: "null" for the zero time, else the quoted UTC RFC3339 text (whole seconds)
        return "null" if v is None else '"' + _rfc3339(v) + '"'
    if kind == "int64ptr":
        return "null" if v is None else str(int(v))
    if isinstance(kind, tuple):
        if v is None:
            return "null"
        return marshal(kind[1], v)
    raise TypeError(f"no encoder for {kind}")


def marshal(table, value: dict) -> str:
    """json.Marshal of a struct: fields in declaration order, omitempty fields dropped when empty."""
    parts = []
    for field, key, omitempty, kind in table:
        v = value.get(field, _zero(kind))
        if omitempty and _is_empty(kind, v):
            continue
        parts.append(go_string(key) + ":" + _value(kind, v))
    return "{" + ",".join(parts) + "}"


# ---- client-go tools/record/event.go
def make_event(ref: dict, event_type: str, reason: str, message: str, source: dict, now_ns: int) -> dict:
    """makeEvent: the name is "<ref.Name>.<UnixNano in hex>", the namespace the reference's or
    "default", both timestamps metav1.Time of now (whole seconds when marshalled), Count 1."""
    sec = now_ns // 10**9
    namespace = ref.get("Namespace", "") or "default"
    return {
        "ObjectMeta": {"Name": "%s.%x" % (ref.get("Name", ""), now_ns), "Namespace": namespace},
        "InvolvedObject": dict(ref),
        "Reason": reason,
        "Message": message,
        "FirstTimestamp": sec,
        "LastTimestamp": sec,
        "Count": 1,
        "Type": event_type,
        "Source": dict(source),  # recorder.generateEvent: event.Source = recorder.source
    }


def object_reference(controller_kind: str, obj: dict) -> dict:
    """The reference each controller records against: the Pod controller's ObjectReference{Kind,
    UID, Name, Namespace} (pod_controller.go:304-315), the Node controller's {Kind, UID, Name,
    Namespace: ""} (node_controller.go:369), every other kind's {APIVersion, Kind, Name, Namespace,
    UID} from the object (stage_controller.go:282)."""
    meta = obj.get("metadata") or {}
    name, ns, uid = meta.get("name") or "", meta.get("namespace") or "", meta.get("uid") or ""
    if controller_kind == "Pod":
        return {"Kind": "Pod", "UID": uid, "Name": name, "Namespace": ns}
    if controller_kind == "Node":
        return {"Kind": "Node", "UID": uid, "Name": name, "Namespace": ""}
    return {"APIVersion": obj.get("apiVersion") or "", "Kind": controller_kind, "Name": name, "Namespace": ns,
            "UID": uid}


def generate_event(ref: dict, event_type: str, reason: str, message: str, now_ns: int,
                   component: str = "kwok_controller"):
    """generateEvent: nothing for a type other than Normal / Warning ("Unsupported event type"),
    else the bytes of the made Event, with the reporting fields the recorder sets
    (ReportingController = source.Component, ReportingInstance = source.Host)."""
    if event_type not in ("Normal", "Warning"):
        return None
    source = {"Component": component}
    ev = make_event(ref, event_type, reason, message, source, now_ns)
    ev["ReportingController"] = source.get("Component", "")
    ev["ReportingInstance"] = source.get("Host", "")
    return marshal(EVENT, ev).encode()


def event_for(controller_kind: str, obj: dict, event: dict, now_ns: int):
    """The Event of a Stage's next.event ({"type", "reason", "message"}) for a fired object."""
    return generate_event(object_reference(controller_kind, obj), event.get("type", ""), event.get("reason", ""),
                          event.get("message", ""), now_ns)

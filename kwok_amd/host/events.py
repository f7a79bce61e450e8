"""The Event of a fired stage (Next.Event), host side: the Python mirror of kwk_patch_event.

playStage records the Stage's Event first, before the finalizer patch and the delete or merge
patches (pod_controller.go:304-352, node_controller.go:369, stage_controller.go:282).  The bytes
are what recorder.Event hands the broadcaster — json.Marshal of the v1.Event that client-go's
generateEvent / makeEvent build — as include/kwok_patch.h restates them; the sink-side
EventCorrelator is not applied.  ``render_event`` writes them from the event program
(KindProgram.event_spec) and an object; libkwok_patch's kwk_patch_event is the native form.
"""
from __future__ import annotations

import ctypes as C
import datetime
import json
from typing import Dict, Optional, Sequence, Tuple, Union

import numpy as np


def _quote(s: str, what: str) -> str:
    """encoding/json's string encoding with escapeHTML on; refuses what kwk_patch_event refuses."""
    out = ['"']
    for i, ch in enumerate(s):
        c = ord(ch)
        if ch in '"\\':
            out.append("\\" + ch)
        elif ch == "\n":
            out.append("\\n")
        elif ch == "\r":
            out.append("\\r")
        elif ch == "\t":
            out.append("\\t")
        elif ch in "<>&" or c in (0x2028, 0x2029):
            out.append("\\u%04x" % c)
        elif c < 0x20:
            raise ValueError(f"render_event: {what}: control byte 0x{c:02x} at offset {len(s[:i].encode())}")
        elif 0xD800 <= c <= 0xDFFF:
            raise ValueError(f"render_event: {what}: invalid UTF-8 (surrogate U+{c:04X})")
        else:
            out.append(ch)
    out.append('"')
    return "".join(out)


def event_time(now_ns: int) -> str:
    """metav1.Time.MarshalJSON's text: whole seconds, UTC, 2006-01-02T15:04:05Z."""
    t = datetime.datetime(1970, 1, 1) + datetime.timedelta(seconds=now_ns // 10**9)
    return t.strftime("%Y-%m-%dT%H:%M:%SZ")


def render_event(spec: Union[str, dict], stage: int, obj: dict, now_ns: int) -> bytes:
    """The Event body for `obj` fired by stage index `stage`; b"" when the stage records nothing."""
    if isinstance(spec, (str, bytes)):
        spec = json.loads(spec)
    if now_ns < 0:
        raise ValueError("render_event: now_ns < 0")
    st = spec["stages"][stage]
    if st is None:
        return b""
    meta = obj.get("metadata") or {}
    ns, name, uid = (meta.get(k) or "" for k in ("namespace", "name", "uid"))
    typed = spec["api_version"] == ""
    ref_ns = "" if typed and spec["kind"] == "Node" else ns
    ref_av = "" if typed else (obj.get("apiVersion") or "")
    ts, comp = event_time(now_ns), _quote(spec["component"], "component")
    o = ['{"metadata":{"name":', _quote("%s.%x" % (name, now_ns), "name"), ',"namespace":',
         _quote(ref_ns or "default", "namespace"), ',"creationTimestamp":null},"involvedObject":{"kind":',
         _quote(spec["kind"], "kind")]
    if ref_ns:
        o += [',"namespace":', _quote(ref_ns, "namespace")]
    if name:  # ObjectReference.Name is omitempty
        o += [',"name":', _quote(name, "name")]
    if uid:
        o += [',"uid":', _quote(uid, "uid")]
    if ref_av:
        o += [',"apiVersion":', _quote(ref_av, "apiVersion")]
    o.append("},")
    if st["reason"]:
        o += ['"reason":', _quote(st["reason"], "reason"), ","]
    if st["message"]:
        o += ['"message":', _quote(st["message"], "message"), ","]
    o += ['"source":{"component":', comp, '},"firstTimestamp":"', ts, '","lastTimestamp":"', ts,
          '","count":1,"type":', _quote(st["type"], "type"), ',"eventTime":null,"reportingComponent":', comp,
          ',"reportingInstance":""}']
    return "".join(o).encode()


# ------------------------------------------------------------------ the device stream (kwok_events.h)
EXPORTS = ("kwk_evt_load", "kwk_evt_check", "kwk_evt_set_rows", "kwk_evt_reserve", "kwk_evt_result", "kwk_evt_device", "kwk_evt_copy")
STAGE_EVENT = 1
COL_NAME, COL_NAMESPACE, COL_UID = 0, 1, 2
ROW_UNUSABLE = 0xFF
EVT_ITEM_DTYPE = np.dtype([("rec", "<u4"), ("status", "u1"), ("reserved", "u1", (3,))])
_REFUSED = frozenset(b'"\\<>&')


class EvtProgramStruct(C.Structure):
    _fields_ = [("kind", C.c_char_p), ("api_version", C.c_char_p), ("component", C.c_char_p), ("n_stages", C.c_uint32),
                ("stage_flags", C.c_void_p), ("text_off", C.c_void_p), ("text", C.c_char_p),
                ("stride_name", C.c_uint32), ("stride_namespace", C.c_uint32), ("stride_uid", C.c_uint32)]


def bind(L):
    """argtypes / restype of kwok_events.h's entry points on libkwok_emit.so (emit.lib() calls this)."""
    L.kwk_evt_load.argtypes = [C.c_void_p, C.POINTER(EvtProgramStruct)]
    L.kwk_evt_check.argtypes = [C.POINTER(EvtProgramStruct)]
    L.kwk_evt_set_rows.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    L.kwk_evt_reserve.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64]
    L.kwk_evt_result.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)]
    L.kwk_evt_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.kwk_evt_copy.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    for n in EXPORTS:
        getattr(L, n).restype = C.c_int32


class EventProgram:
    """kwk_evt_program of an event spec (KindProgram.event_spec(device=True) /
    kwk_program_event_spec) and the row strides of the identity columns: (name, namespace, uid),
    multiples of 4 in 4..256; namespace stride 0 is a cluster-scoped kind."""

    def __init__(self, spec, strides: Tuple[int, int, int] = (256, 64, 40)):
        self.spec = json.loads(spec) if isinstance(spec, (str, bytes)) else spec
        self.strides = tuple(int(s) for s in strides)
        st = self.spec["stages"]
        self.any_event = any(s is not None for s in st)
        flags = np.zeros(max(1, len(st)), dtype=np.uint8)
        offs = np.zeros(3 * len(st) + 1, dtype=np.uint32)
        text = b""
        for i, s in enumerate(st):
            for k, key in enumerate(("type", "reason", "message")):
                if s is not None:
                    text += s[key].encode()
                offs[3 * i + k + 1] = len(text)
            flags[i] = STAGE_EVENT if s is not None else 0
        self._keep = (flags, offs, text, self.spec["kind"].encode(), self.spec["api_version"].encode(),
                      self.spec["component"].encode())
        from . import abi
        self.struct = EvtProgramStruct(self._keep[3], self._keep[4], self._keep[5], len(st), abi.ptr(flags), abi.ptr(offs),
                                       text, *self.strides)

    def check(self):
        """kwk_evt_check: the program checked without an emitter or a device (abi.EngineError names
        what the device stream does not carry: a string, a stride, the text budget, more than 32 stages)."""
        from . import abi, emit
        st = emit.lib().kwk_evt_check(C.byref(self.struct))
        if st != 0:
            raise abi.EngineError(f"kwk_evt_check failed ({st}): {emit.lib().kwk_emit_last_error(None).decode(errors='replace')}")

    def _row(self, text: Optional[str], stride: int, usable: bool) -> bytes:
        b = (text or "").encode("utf-8", "surrogatepass")
        if not usable or len(b) > stride - 1 or len(b) >= ROW_UNUSABLE or any(c < 0x21 or c > 0x7E or c in _REFUSED for c in b):
            return bytes([ROW_UNUSABLE]) + b"\0" * (stride - 1)
        return bytes([len(b)]) + b + b"\0" * (stride - 1 - len(b))

    def rows(self, objs: Sequence[Optional[dict]]) -> Dict[int, np.ndarray]:
        """The identity columns of objects: {column: uint8 [len(objs), stride]} of [length][text]
        rows.  All three rows of an object are unusable (the host renders its Events) when the
        object is None or its apiVersion is not the program's; one row is when its text needs
        escaping or does not fit."""
        av = self.spec["api_version"]
        out = {}
        for c, key in ((COL_NAME, "name"), (COL_NAMESPACE, "namespace"), (COL_UID, "uid")):
            stride = self.strides[c]
            if not stride:
                continue
            rows = []
            for o in objs:
                ok = o is not None and (av == "" or (o.get("apiVersion") or "") == av)
                rows.append(self._row(((o or {}).get("metadata") or {}).get(key), stride, ok))
            out[c] = np.frombuffer(b"".join(rows), dtype=np.uint8).reshape(len(objs), stride).copy()
        return out

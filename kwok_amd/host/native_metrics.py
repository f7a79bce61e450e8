"""ctypes binding of the native Metric CR compiler in libkwok_compiler.so (include/kwok_metrics.h):
a Metric CR's gauge / counter / histogram values lowered to the device programs of
kwk_metrics_load / kwk_histograms_load by C++ (kwok_amd/csrc/metrics_compiler.cpp, celc.hpp) —
what a Go host calls through cgo instead of compiling CEL per scrape
(pkg/kwok/metrics/metrics.go:168-462, evaluator.go:51-144; INTEGRATION.md: LoadMetrics).

The Python lowering (cel.lower through metrics.MetricsProgram) is its CPU cross-check: the packed
arrays are byte-equal (tests/test_metric_compiler.py)."""
from __future__ import annotations

import ctypes as C
import json
from typing import List, Tuple

from . import abi, cel
from .native_compiler import lib as _compiler_lib

KWK_ENOLOWER = -5
KWK_METRICS_EXPO_HISTOGRAMS = 1   # kwk_compile_metrics_flags
KIND_SCALAR, KIND_HISTOGRAM = 0, 1  # kwk_expo_family.reserved: the kind code

_bound = False


class ExpoFamily(C.Structure):
    _fields_ = [("name_off", C.c_uint32), ("name_len", C.c_uint32), ("header_off", C.c_uint32),
                ("header_len", C.c_uint32), ("metric", C.c_uint32), ("dimension", C.c_uint32), ("group", C.c_uint32),
                ("reserved", C.c_uint32)]


class ExpoGroup(C.Structure):
    _fields_ = [("dimension", C.c_uint32), ("n_labels", C.c_uint32)]


class ExpoProgramStruct(C.Structure):
    """kwk_expo_program (include/kwok_metrics.h)."""
    _fields_ = [("n_families", C.c_uint32), ("n_groups", C.c_uint32), ("n_metrics", C.c_uint32),
                ("n_lit_bytes", C.c_uint32), ("families", C.POINTER(ExpoFamily)), ("groups", C.POINTER(ExpoGroup)),
                ("metric_dimension", C.POINTER(C.c_uint32)), ("lits", C.c_void_p)]


class ExpoHistLine(C.Structure):
    _fields_ = [("prefix_off", C.c_uint32), ("prefix_len", C.c_uint32), ("tail_off", C.c_uint32),
                ("tail_len", C.c_uint32)]


class ExpoHist(C.Structure):
    _fields_ = [("dimension", C.c_uint32), ("n_visible", C.c_uint32), ("first_line", C.c_uint32),
                ("reserved", C.c_uint32)]


class ExpoHistProgramStruct(C.Structure):
    """kwk_expo_hist_program (include/kwok_metrics.h): the histogram families' per-line tables."""
    _fields_ = [("n_hists", C.c_uint32), ("n_lines", C.c_uint32), ("hists", C.POINTER(ExpoHist)),
                ("lines", C.POINTER(ExpoHistLine))]


def lib():
    global _bound
    L = _compiler_lib()
    if not _bound:
        L.kwk_metric_set_last_error.restype = C.c_char_p
        L.kwk_metric_set_last_error.argtypes = [C.c_void_p]
        L.kwk_compile_metrics.argtypes = [C.c_char_p, C.POINTER(C.c_void_p)]
        L.kwk_compile_metrics_flags.argtypes = [C.c_char_p, C.c_uint32, C.POINTER(C.c_void_p)]
        L.kwk_metric_set_exposition_histograms.argtypes = [C.c_void_p, C.POINTER(ExpoHistProgramStruct)]
        L.kwk_metric_set_destroy.argtypes = [C.c_void_p]
        L.kwk_metric_set_programs.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_void_p),
                                              C.POINTER(C.c_uint32), C.POINTER(C.c_void_p)]
        L.kwk_metric_set_histograms.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_void_p),
                                                C.POINTER(C.c_uint32), C.POINTER(C.c_void_p),
                                                C.POINTER(C.c_uint32), C.POINTER(C.c_void_p)]
        L.kwk_metric_set_describe.argtypes = [C.c_void_p, C.POINTER(C.c_char_p)]
        L.kwk_cel_lower.argtypes = [C.c_char_p, C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint32)]
        L.kwk_metric_set_exposition.argtypes = [C.c_void_p, C.POINTER(ExpoProgramStruct)]
        L.kwk_metric_labels_render.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p, C.c_char_p, C.c_uint32, C.c_void_p,
                                               C.c_uint32, C.POINTER(C.c_uint32), C.c_void_p, C.c_uint32,
                                               C.POINTER(C.c_uint32)]
        for n in ("kwk_compile_metrics", "kwk_metric_set_destroy", "kwk_metric_set_programs",
                  "kwk_metric_set_histograms", "kwk_metric_set_describe", "kwk_cel_lower",
                  "kwk_metric_set_exposition", "kwk_metric_labels_render", "kwk_compile_metrics_flags",
                  "kwk_metric_set_exposition_histograms"):
            getattr(L, n).restype = C.c_int32
        _bound = True
    return L


class MetricCompileError(ValueError):
    pass


class NoExposition(MetricCompileError):
    """The Metric CR has no device exposition program (a host-evaluated metric, a label outside the
    supported subset, or a histogram in a set compiled without ``expo_histograms``)."""


class LabelRenderError(ValueError):
    pass


DIMS = {"node": 0, "pod": 1, "container": 2}


def cel_lower(expr: str, dimension: str) -> List[Tuple[int, float]]:
    """kwk_cel_lower in cel.lower's output form [(op, operand)] (operand: the input index for a
    load, the constant for a constant, 0.0 otherwise); cel.LowerError when the expression has no
    device form, MetricCompileError when it does not compile."""
    L = lib()
    n = C.c_uint32()
    cap = 256
    ops = (abi.MetricOp * cap)()
    st = L.kwk_cel_lower(expr.encode(), DIMS.get(dimension, 3), ops, cap, C.byref(n))
    if st == abi.KWK_ECAP and n.value > cap:  # a longer program: *n_ops = the length it needs
        cap = n.value
        ops = (abi.MetricOp * cap)()
        st = L.kwk_cel_lower(expr.encode(), DIMS.get(dimension, 3), ops, cap, C.byref(n))
    if st == KWK_ENOLOWER:
        raise cel.LowerError(L.kwk_metric_set_last_error(None).decode(errors="replace"))
    if st != 0:
        raise MetricCompileError(L.kwk_metric_set_last_error(None).decode(errors="replace"))
    out = []
    for o in ops[:n.value]:
        out.append((int(o.op), int(o.arg) if o.op == cel.OP_LOAD else float(o.value) if o.op == cel.OP_CONST else 0.0))
    return out


class NativeMetricSet:
    """One Metric CR compiled by kwk_compile_metrics; expo_histograms: by kwk_compile_metrics_flags
    with KWK_METRICS_EXPO_HISTOGRAMS, so that histogram families are part of the exposition program
    (``exposition_hist_program``) instead of refusing it."""

    def __init__(self, metric_doc: dict, expo_histograms: bool = False):
        self.h = C.c_void_p()
        self.expo_histograms = bool(expo_histograms)
        L = lib()
        if expo_histograms:
            st = L.kwk_compile_metrics_flags(json.dumps(metric_doc).encode(), KWK_METRICS_EXPO_HISTOGRAMS,
                                             C.byref(self.h))
        else:
            st = L.kwk_compile_metrics(json.dumps(metric_doc).encode(), C.byref(self.h))
        if st != 0:
            raise MetricCompileError(L.kwk_metric_set_last_error(None).decode(errors="replace"))
        s = C.c_char_p()
        L.kwk_metric_set_describe(self.h, C.byref(s))
        self.describe = json.loads(s.value.decode())
        self.host_metrics: List[str] = list(self.describe["host_metrics"])

    def close(self):
        if self.h:
            lib().kwk_metric_set_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def programs_raw(self):
        """(n_metrics, desc pointer, n_ops, op pointer) owned by the set: kwk_metrics_load's arguments."""
        n, d, no, o = C.c_uint32(), C.c_void_p(), C.c_uint32(), C.c_void_p()
        st = lib().kwk_metric_set_programs(self.h, C.byref(n), C.byref(d), C.byref(no), C.byref(o))
        if st != 0:
            raise MetricCompileError("kwk_metric_set_programs")
        return n.value, d, no.value, o

    def histograms_raw(self):
        n, d, nb, b, no, o = C.c_uint32(), C.c_void_p(), C.c_uint32(), C.c_void_p(), C.c_uint32(), C.c_void_p()
        st = lib().kwk_metric_set_histograms(self.h, C.byref(n), C.byref(d), C.byref(nb), C.byref(b), C.byref(no),
                                             C.byref(o))
        if st != 0:
            raise MetricCompileError("kwk_metric_set_histograms")
        return n.value, d, nb.value, b, no.value, o

    def programs_bytes(self) -> Tuple[bytes, bytes]:
        n, d, no, o = self.programs_raw()
        return C.string_at(d, n * C.sizeof(abi.MetricDesc)) if n else b"", \
            C.string_at(o, no * C.sizeof(abi.MetricOp)) if no else b""

    def histograms_bytes(self) -> Tuple[bytes, bytes, bytes]:
        n, d, nb, b, no, o = self.histograms_raw()
        return (C.string_at(d, n * C.sizeof(abi.HistogramDesc)) if n else b"",
                C.string_at(b, nb * C.sizeof(abi.MetricBucket)) if nb else b"",
                C.string_at(o, no * C.sizeof(abi.MetricOp)) if no else b"")

    def exposition_program(self) -> ExpoProgramStruct:
        """kwk_metric_set_exposition: the program of the device text writer (arrays owned by the
        set); NoExposition (KWK_ENOLOWER) names the metric that keeps the text on the host."""
        prog = ExpoProgramStruct()
        L = lib()
        st = L.kwk_metric_set_exposition(self.h, C.byref(prog))
        if st != 0:
            msg = L.kwk_metric_set_last_error(None).decode(errors="replace")
            raise (NoExposition if st == KWK_ENOLOWER else MetricCompileError)(msg)
        return prog

    def exposition_hist_program(self) -> ExpoHistProgramStruct:
        """kwk_metric_set_exposition_histograms: per histogram its dimension, n_visible and the
        prefix / tail byte ranges (in the exposition program's lits) of its n_visible + 3 lines."""
        prog = ExpoHistProgramStruct()
        L = lib()
        st = L.kwk_metric_set_exposition_histograms(self.h, C.byref(prog))
        if st != 0:
            msg = L.kwk_metric_set_last_error(None).decode(errors="replace")
            raise (NoExposition if st == KWK_ENOLOWER else MetricCompileError)(msg)
        return prog

    def labels_render(self, group: int, node, pod, container_index: int = 0) -> Tuple[bytes, bytes]:
        """kwk_metric_labels_render: (label block, sort key) of one object of `group`; node / pod
        are JSON objects (dict), JSON text (bytes) or None.  LabelRenderError (KWK_EINVAL) names
        the object and label whose selection fails."""
        def text(o):
            return None if o is None else o if isinstance(o, bytes) else json.dumps(o).encode()
        nj, pj = text(node), text(pod)
        L = lib()
        bl, kl = C.c_uint32(), C.c_uint32()
        cap = 256
        while True:
            b, k = C.create_string_buffer(cap), C.create_string_buffer(cap)
            st = L.kwk_metric_labels_render(self.h, group, nj, pj, container_index, b, cap, C.byref(bl), k, cap,
                                            C.byref(kl))
            if st == abi.KWK_ECAP:
                cap = max(bl.value, kl.value)
                continue
            if st != 0:
                msg = L.kwk_metric_set_last_error(None).decode(errors="replace")
                raise (NoExposition if st == KWK_ENOLOWER else LabelRenderError)(msg)
            return b.raw[:bl.value], k.raw[:kl.value]

    def load(self, pods_engine):
        """kwk_metrics_load (+ kwk_histograms_load when the CR has histograms) from the set's arrays."""
        pods_engine.metrics_load_arrays(*self.programs_raw())
        h = self.histograms_raw()
        if h[0]:
            pods_engine.histograms_load_arrays(*h)

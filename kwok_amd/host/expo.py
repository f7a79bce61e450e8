"""Device metric exposition (include/kwok_expo.h), host side: the ctypes binding of
libkwok_expo.so and ``Exposition``, which renders every object's labels through the native
renderer (kwk_metric_labels_render), uploads them, and returns a scrape's Prometheus text per node
as the GPU wrote it.

Reference: UpdateHandler.Update + promhttp's text encoder (pkg/kwok/metrics/metrics.go:480-502,
525-573, pkg/kwok/server/metrics.go:129-150).  The text of a node equals
``MetricsProgram.exposition(MetricsProgram.scrape(...))`` for that node alone, byte for byte
(tests/test_gpu_expo.py, tests/test_gpu_expo_hist.py); that Python path stays the CPU cross-check
and the only path of a CR the device program refuses (host-evaluated metrics, computed labels, and
histograms unless the set was compiled with ``expo_histograms=True``: then ``Exposition`` creates
the writer with the histogram tables, kwk_expo_create_hist).
"""
from __future__ import annotations

import ctypes as C
import os
from typing import List, Optional, Sequence

import numpy as np

from . import abi
from .native_metrics import KIND_HISTOGRAM, ExpoHistProgramStruct, ExpoProgramStruct, NativeMetricSet

LIB_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lib", "libkwok_expo.so")
DIM_NODE, DIM_POD, DIM_CONTAINER = 0, 1, 2
MAX_FLOAT_BYTES = 24
SORT_MAX_ROWS = 1024  # KWK_EXPO_SORT_MAX_ROWS: a node's rows of a group that kwk_expo_commit_rows sorts on the device

_lib = None


class ExpoError(RuntimeError):
    def __init__(self, msg: str, status: int = 0):
        super().__init__(msg)
        self.status = status


def lib():
    """Load libkwok_expo.so (built in-tree by kwok_amd.build); loading needs no GPU."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ExpoError(f"exposition library missing: {LIB_PATH} (run python -m kwok_amd.build)")
    abi.lib()  # libkwok_engine.so first (the writer links to it)
    L = C.CDLL(LIB_PATH)
    u32, u64, vp = C.c_uint32, C.c_uint64, C.c_void_p
    L.kwk_expo_last_error.restype = C.c_char_p
    L.kwk_expo_last_error.argtypes = [vp]
    L.kwk_expo_create.argtypes = [vp, u32, C.POINTER(ExpoProgramStruct), C.POINTER(vp)]
    L.kwk_expo_create_hist.argtypes = [vp, u32, C.POINTER(ExpoProgramStruct), C.POINTER(ExpoHistProgramStruct),
                                       C.POINTER(vp)]
    L.kwk_expo_destroy.argtypes = [vp]
    L.kwk_expo_set_labels.argtypes = [vp, u32, u32, u32, vp, vp, vp, vp]
    L.kwk_expo_commit.argtypes = [vp]
    L.kwk_expo_reserve.argtypes = [vp, u64]
    L.kwk_expo_scrape.argtypes = [vp, C.c_int64, u32, u32]
    L.kwk_expo_result.argtypes = [vp, C.POINTER(u64)]
    L.kwk_expo_device.argtypes = [vp, C.POINTER(vp), C.POINTER(vp)]
    L.kwk_expo_copy.argtypes = [vp, vp, vp]
    L.kwk_expo_elapsed.argtypes = [vp, C.POINTER(C.c_float)]
    L.kwk_expo_set_width.argtypes = [vp, u32]
    L.kwk_expo_format_values.argtypes = [vp, vp, u32, vp, vp]
    L.kwk_expo_format_f64.argtypes = [C.c_double, vp]
    L.kwk_expo_format_f64.restype = u32
    L.kwk_expo_commit_rows.argtypes = [vp]
    L.kwk_expo_commit_rows_elapsed.argtypes = [vp, C.POINTER(C.c_float)]
    L.kwk_expo_read_perm.argtypes = [vp, u32, vp]
    L.kwk_expo_key_compare.argtypes = [C.c_char_p, u32, C.c_char_p, u32]
    L.kwk_expo_key_compare.restype = C.c_int
    for n in ("kwk_expo_create", "kwk_expo_create_hist", "kwk_expo_destroy", "kwk_expo_set_labels", "kwk_expo_commit", "kwk_expo_reserve",
              "kwk_expo_scrape", "kwk_expo_result", "kwk_expo_device", "kwk_expo_copy", "kwk_expo_elapsed",
              "kwk_expo_set_width", "kwk_expo_format_values", "kwk_expo_commit_rows", "kwk_expo_commit_rows_elapsed",
              "kwk_expo_read_perm"):
        getattr(L, n).restype = C.c_int32
    _lib = L
    return L


def format_f64(v: float) -> bytes:
    """kwk_expo_format_f64: the host build of the device formatter (strconv 'g', -1, 64)."""
    buf = C.create_string_buffer(MAX_FLOAT_BYTES)
    n = lib().kwk_expo_format_f64(float(v), buf)
    return buf.raw[:n]


def key_compare(a: bytes, b: bytes) -> int:
    """kwk_expo_key_compare: the host build of the device sort's comparator (< 0, 0, > 0)."""
    return int(lib().kwk_expo_key_compare(a, len(a), b, len(b)))


def _pack(items: Sequence[bytes]):
    off = np.zeros(len(items) + 1, dtype=np.uint32)
    np.cumsum([len(b) for b in items], out=off[1:])
    return off, b"".join(items)


class Exposition:
    """The device text writer of one pods engine and one Metric CR.

    engine: the pods Engine after usage_config / usage_pods and ``metric_set.load(engine)``;
    metric_set: the NativeMetricSet of the CR (NoExposition when the CR has no device program)."""

    def __init__(self, engine, metric_set: NativeMetricSet):
        self.eng, self.ms = engine, metric_set
        self.prog = metric_set.exposition_program()
        self.groups = [(int(self.prog.groups[g].dimension), int(self.prog.groups[g].n_labels))
                       for g in range(self.prog.n_groups)]
        self.families = [C.string_at(self.prog.lits + self.prog.families[f].name_off,
                                     self.prog.families[f].name_len).decode() for f in range(self.prog.n_families)]
        self.n_nodes = engine.n_nodes
        self.node_ptr = np.asarray(engine._uargs[0], dtype=np.int64)
        self.cptr = np.concatenate([[0], np.cumsum(engine.usage_containers)]).astype(np.int64)
        self.h = C.c_void_p()
        L = lib()
        self.hist_prog = None
        if any(self.prog.families[f].reserved == KIND_HISTOGRAM for f in range(self.prog.n_families)):
            self.hist_prog = metric_set.exposition_hist_program()
            st = L.kwk_expo_create_hist(engine.h, self.n_nodes, C.byref(self.prog), C.byref(self.hist_prog),
                                        C.byref(self.h))
        else:
            st = L.kwk_expo_create(engine.h, self.n_nodes, C.byref(self.prog), C.byref(self.h))
        if st != 0:
            raise ExpoError("kwk_expo_create: " + L.kwk_expo_last_error(None).decode(errors="replace"), st)
        self.reserved = 0

    def close(self):
        if self.h:
            lib().kwk_expo_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, st: int, what: str):
        if st != 0:
            raise ExpoError(f"{what}: " + lib().kwk_expo_last_error(self.h).decode(errors="replace"), st)

    # labels
    def set_rows(self, group: int, first: int, blocks: Sequence[bytes], keys: Sequence[bytes]):
        """kwk_expo_set_labels over already rendered rows."""
        bo, bb = _pack(blocks)
        ko, kb = _pack(keys)
        self._check(lib().kwk_expo_set_labels(self.h, group, first, len(blocks), abi.ptr(bo), bb, abi.ptr(ko), kb),
                    "kwk_expo_set_labels")

    def set_nodes(self, nodes: Sequence[dict], first: int = 0):
        """The label rows of nodes [first, first + len(nodes)) for every node group."""
        for g, (dim, _) in enumerate(self.groups):
            if dim == DIM_NODE:
                rows = [self.ms.labels_render(g, n, None) for n in nodes]
                self.set_rows(g, first, [r[0] for r in rows], [r[1] for r in rows])

    def set_pods(self, pods: Sequence[Optional[dict]], first: int = 0, nodes: Optional[Sequence[dict]] = None):
        """The label rows of pod slots [first, first + len(pods)) for every pod and container
        group (None: a dead slot, left as it is); nodes: every node's object, for labels that
        read `node`.  One kwk_expo_set_labels call per run of consecutive live slots and group."""
        import json
        texts = [None if p is None else json.dumps(p).encode() for p in pods]
        for g, (dim, _) in enumerate(self.groups):
            if dim == DIM_NODE:
                continue
            start, blocks, keys = None, [], []

            def flush():
                nonlocal start, blocks, keys
                if blocks:
                    self.set_rows(g, start, blocks, keys)
                start, blocks, keys = None, [], []

            for i, pj in enumerate(texts):
                if pj is None:
                    flush()
                    continue
                slot = first + i
                node = None
                if nodes is not None:
                    node = nodes[int(np.searchsorted(self.node_ptr, slot, side="right")) - 1]
                if dim == DIM_POD:
                    rows = [self.ms.labels_render(g, node, pj)]
                    row0 = slot
                else:
                    row0 = int(self.cptr[slot])
                    rows = [self.ms.labels_render(g, node, pj, j) for j in range(int(self.cptr[slot + 1]) - row0)]
                if start is None:
                    start = row0
                blocks += [r[0] for r in rows]
                keys += [r[1] for r in rows]
            flush()

    def layout_changed(self):
        """After Engine.usage_set_rows returned True (some slot's container count changed): the
        container rows' places follow the engine's new layout; set the moved pods' rows again and
        commit()."""
        self.cptr = np.concatenate([[0], np.cumsum(self.eng.usage_containers)]).astype(np.int64)

    def commit(self):
        """kwk_expo_commit: the full commit (re-reads the layout, sorts and uploads every row)."""
        self._check(lib().kwk_expo_commit(self.h), "kwk_expo_commit")

    def commit_rows(self):
        """kwk_expo_commit_rows: only the rows set since the last commit, enqueued on the engine's
        stream (the scatter and sort kernels); ExpoError KWK_ESTATE when a full commit is due."""
        self._check(lib().kwk_expo_commit_rows(self.h), "kwk_expo_commit_rows")

    def commit_rows_elapsed_ms(self):
        """(scatter, sort) kernel times of the last commit_rows that enqueued work, by HIP events."""
        ms = (C.c_float * 2)()
        self._check(lib().kwk_expo_commit_rows_elapsed(self.h, ms), "kwk_expo_commit_rows_elapsed")
        return tuple(float(x) for x in ms)

    def read_perm(self, group: int) -> np.ndarray:
        """kwk_expo_read_perm: a pod or container group's device permutation (its rows)."""
        dim = self.groups[group][0] if 0 <= group < len(self.groups) else DIM_POD
        rows = int(self.node_ptr[-1]) if dim == DIM_POD else int(self.cptr[-1]) if dim == DIM_CONTAINER else 1
        out = np.zeros(max(1, rows), dtype=np.uint32)
        self._check(lib().kwk_expo_read_perm(self.h, group, abi.ptr(out)), "kwk_expo_read_perm")
        return out[:rows]

    def set_width(self, width: int):
        self._check(lib().kwk_expo_set_width(self.h, width), "kwk_expo_set_width")

    # scrapes
    def reserve(self, max_bytes: int):
        self._check(lib().kwk_expo_reserve(self.h, max_bytes), "kwk_expo_reserve")
        self.reserved = max_bytes

    def enqueue(self, now_ns: int, node_first: int, n_nodes: int):
        """kwk_expo_scrape (enqueue only), after the caller's engine.usage(now_ns)."""
        self._check(lib().kwk_expo_scrape(self.h, now_ns, node_first, n_nodes), "kwk_expo_scrape")
        self._last_nodes = n_nodes

    def result(self) -> int:
        """kwk_expo_result: the text's size (synchronises); ExpoError with status KWK_ECAP when it
        exceeds the reservation (``needed`` holds the size)."""
        n = C.c_uint64()
        st = lib().kwk_expo_result(self.h, C.byref(n))
        self.needed = int(n.value)
        self._check(st, "kwk_expo_result")
        return self.needed

    def copy(self, n_bytes: int):
        """(offsets, bytes) of the last scrape on the host."""
        off = np.zeros(self._last_nodes + 1, dtype=np.uint64)
        out = np.zeros(max(1, n_bytes), dtype=np.uint8)
        self._check(lib().kwk_expo_copy(self.h, abi.ptr(off), abi.ptr(out)), "kwk_expo_copy")
        return off, out[:n_bytes]

    def scrape(self, now_ns: int, node_first: int, n_nodes: int) -> List[bytes]:
        """One scrape of nodes [node_first, node_first + n_nodes) -> each node's text; reserves
        more and scrapes again when the text does not fit."""
        self.enqueue(now_ns, node_first, n_nodes)
        try:
            n = self.result()
        except ExpoError as e:
            if e.status != abi.KWK_ECAP:
                raise
            self.reserve(self.needed + self.needed // 8)
            self.enqueue(now_ns, node_first, n_nodes)
            n = self.result()
        off, raw = self.copy(n)
        buf = raw.tobytes()
        return [buf[int(off[j]):int(off[j + 1])] for j in range(n_nodes)]

    def elapsed_ms(self):
        """(whole scrape, lengths, scan, write) of the last scrape, by HIP events."""
        ms = (C.c_float * 4)()
        self._check(lib().kwk_expo_elapsed(self.h, ms), "kwk_expo_elapsed")
        return tuple(float(x) for x in ms)

    def format_values(self, values) -> List[bytes]:
        """kwk_expo_format_values: the device formatter over float64 values."""
        v = np.ascontiguousarray(values, dtype=np.float64)
        out = np.zeros((len(v), MAX_FLOAT_BYTES), dtype=np.uint8)
        lens = np.zeros(len(v), dtype=np.uint8)
        self._check(lib().kwk_expo_format_values(self.h, abi.ptr(v), len(v), abi.ptr(out), abi.ptr(lens)),
                    "kwk_expo_format_values")
        raw = out.tobytes()
        return [raw[i * MAX_FLOAT_BYTES:i * MAX_FLOAT_BYTES + int(lens[i])] for i in range(len(v))]

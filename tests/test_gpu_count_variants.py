"""Every count / aggregate kernel variant against a numpy reference (tests/count_util.ref_counts).

kwk_count and kwk_aggregate pick their kernel from the state word's bytes and the number of masks
(launch_count8 / launch_count in engine.hip):

    state bytes  n_masks  kernel
    1 (ids)      1-4      count8_kernel<1>
    1            5-8      count8_kernel<2>
    1            9-16     count8_kernel<4>
    1            1-4      usage_fast_kernel<1, true> with n_cmasks (kwk_aggregate with usage, the
                          1-byte key column, KWK_USAGE_AGG_FUSED and n_usage_pods == n_active)
    2            1-4      count16_lut_kernel (make_fmt leaves a 2-byte word at most 11 pred bits, so
                          pmask < 2^11 and abit > pmask always hold: count_kernel<2, 2> and <2, 4>
                          are never launched)
    2            5-8      count_kernel<2, 8>   (the SWAR body)
    2            9-16     count_kernel<2, 16>
    4            1-2      count_kernel<4, 2>
    4            3-4      count_kernel<4, 4>
    4            5-8      count_kernel<4, 8>
    4            9-16     count_kernel<4, 16>
    8            1-2 / 3-4 / 5-8 / 9-16   count_kernel<8, 2 / 4 / 8 / 16>, px = 1 for the fused
                          records ("dw"), 0 for the wide {pred, sched} words
    then kwk_count: count_total_kernel; kwk_aggregate: the count waves of agg_final_kernel

The mask sets M1, M2, M3, M4, M5, M8, M9 and M16 select every row; every case asserts
stats()["state_bytes"], so it provably runs the kernel of its row.

Columns are drawn from real rows: a pod-fast cluster (table-only, so "auto" keeps the 1-byte ids;
six pred bits in use) stepped under the harness; its rows before and after the steps are the pool, a case's column is
pool[rng.integers(len(pool), n)], and a fifth of it is deleted.  Expected counts come from the
chosen rows, and eng.read() must show the same pred bits and alive flags.

Stale rows: both ways of making an engine shorter (a second kwk_load, kwk_relayout) clear the
words past the new end, so the words the kernels' tail limit has to skip are put back by hand:
live words copied into the rest of the last chunk through kwk_device_ptrs."""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest

from kwok_amd import workload as W
from kwok_amd.host import abi
from tests import count_util as CU
from tests.count_util import ref_counts

REL_TOL = 1e-6  # BASELINE.json north_star tolerance (tests/test_usage.py)


# ---------------------------------------------------------------- the reference, on the CPU
def test_ref_counts_against_python_loop():
    rng = np.random.default_rng(7)
    n = 301
    pred = rng.integers(0, 1 << 12, n, dtype=np.uint32)
    pred[::17] |= np.uint32(0x80000000)
    pred[5:40] = 0
    alive = rng.random(n) < 0.8
    masks = [0, 1, 1 << 5, 0x80000000, 0x0A6, 0xFFFFFFFF, 1 << 20, 0, 1 << 5]
    want = []
    for m in masks:
        c = 0
        for p, a in zip(pred.tolist(), alive.tolist()):
            if a and (m == 0 or (p & m) != 0):
                c += 1
        want.append(c)
    got = ref_counts(pred, alive, masks)
    assert got.dtype == np.uint64 and got.tolist() == want
    assert want[0] == int(alive.sum()) == want[7] and want[6] == 0 and want[2] == want[8]
    assert 0 < want[5] < want[0] and len(set(want[:6])) == 6
    assert ref_counts(pred, alive, []).shape == (0,)
    assert ref_counts(pred[:0], alive[:0], [0, 1]).tolist() == [0, 0]


def test_case_generators():
    """The shapes and mask sets the GPU tests run: n = C * W - r around 1, 255-257, 1023-1025 and
    2049 chunks, mask counts 1, 2, 3, 4, 5, 8, 9, 16, and dead sets that take the first object,
    the last one and a whole chunk."""
    for fmt, wb in CU.FORMATS.items():
        w = 16 // wb
        ns = CU.sizes(w)
        assert ns[0] == 1 and ns[-1] == 2049 * w
        for c in CU.CHUNKS:
            assert c * w in ns and c * w - 1 in ns and (w <= 2 or c * w - (w - 1) in ns)
    bits = [1, 2, 4, 8, 16, 32, 64]
    sets = CU.mask_sets(bits, 128)
    assert [len(m) for m in sets.values()] == [1, 2, 3, 4, 5, 8, 9, 16]
    m16 = sets["M16"]
    assert all(b in m16 for b in bits) and m16[-1] == 128 and m16[-2] == 0xFFFFFFFF and 0 in m16[4:12]
    assert sets["M2"][-1] == 0 and sets["M4"][0] == 0 and sets["M8"][0] == sets["M8"][1]
    assert len(CU.mask_sets(bits[:5], 128)["M16"]) == 16 and len(CU.mask_sets(list(range(1, 17)), 128)["M16"]) == 16
    rng = np.random.default_rng(1)
    first = last = chunk = False
    for case in range(16):
        d = CU.dead_slots(rng, 403, 8, case)
        assert len(d) >= 80 and d.max() < 403 and len(np.unique(d)) == len(d)
        alive = np.ones(408, dtype=bool)
        alive[d] = False
        first |= not alive[0]
        last |= not alive[402]
        chunk |= bool((~alive[:400].reshape(-1, 8)).all(axis=1).any())
    assert first and last and chunk
    assert CU.dead_slots(rng, 1, 16, 0).tolist() == [] and CU.dead_slots(rng, 1, 16, 3).tolist() == [0]


# ---------------------------------------------------------------- the pool and the cases
@functools.lru_cache(maxsize=None)
def _pool():
    """(prog, hot, dels, rec, cls, records): rows of a stepped pod-fast cluster, before the steps
    (Ingest.columns) and after each of six steps (eng.read(); the class from the row's upper half).
    pod-fast under the harness shows five pred bits (deletionTimestamp, podIP, Running, the Job owner,
    Succeeded); every 16th pod starts Failed, which adds a sixth (many more start states overflow
    an id class, and the engine then leaves the 1-byte ids)."""
    from kwok_amd.host.engine import Ingest
    from tests.parity_util import NOW0, build
    cl = W.make_cluster("C1", 40, 400, seed=31)
    objs = cl.pods.materialize()
    for i, o in enumerate(objs):
        if i % 16 == 2:
            o["status"] = {"phase": "Failed", "podIP": "10.0.0.7"}
    prog, eng, _ = build(cl.pod_stage_files, objs, harness=True)
    try:
        assert eng.stats()["state_bytes"] == 1
        ing = Ingest(prog)
        hot0, dels0, rec0, cls0 = ing.columns(objs)
        records = ing.record_array()
        parts = [(hot0, dels0, rec0, cls0)]
        for k in range(6):
            eng.step(NOW0 + k * 10**9, 5, k)
            hot, dels = eng.read()
            parts.append((hot, dels, rec0, (hot["sched"] >> np.uint32(abi.CLASS_SHIFT)).astype(np.uint16)))
    finally:
        eng.close()
    hot, dels, rec, cls = (np.concatenate([p[i] for p in parts]) for i in range(4))
    return prog, hot, dels, rec, cls, records


@functools.lru_cache(maxsize=None)
def _mask_sets():
    prog, hot = _pool()[:2]
    alive = (hot["sched"] & abi.F_ALIVE) != 0
    bits = CU.bits_in_use(hot["pred"], alive)
    assert len(bits) >= 5, bits  # else the 16-mask cases degenerate
    assert not alive.all() and len({int(c) for c in ref_counts(hot["pred"], alive, bits)}) >= 4
    pb = prog.table().pred_bits
    assert 0 < pb <= 11 and max(bits) < (1 << pb)
    return CU.mask_sets(bits, 1 << pb)


def _engine(fmt, capacity):
    from kwok_amd.host.engine import Engine
    prog, records = _pool()[0], _pool()[5]
    eng = Engine(prog, capacity=capacity, state=fmt, max_records=max(1 << 16, len(records) + 16))
    eng.load_stages()
    eng.set_harness(True)
    return eng


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def _load(eng, fmt, n, rng, case=0, dead=None):
    """Loads a column of n pool rows, deletes a dead set, checks the engine's format and what
    eng.read() shows -> (pred, alive, pool indices) as the test chose them."""
    _, hot, dels, rec, cls, records = _pool()
    idx = rng.integers(len(hot), size=n)
    eng.load(hot[idx], dels[idx], rec[idx], cls[idx], records)
    assert eng.stats()["state_bytes"] == CU.FORMATS[fmt]
    pred = hot["pred"][idx].copy()
    alive = (hot["sched"][idx] & abi.F_ALIVE) != 0
    if dead is None:
        dead = CU.dead_slots(rng, n, 16 // CU.FORMATS[fmt], case) if n else np.zeros(0, dtype=np.uint32)
    if len(dead):
        eng.delete(dead)
        alive[dead] = False
    if n:
        _check_read(eng, pred, alive)
    return pred, alive, idx


def _check_read(eng, pred, alive):
    got, _ = eng.read()
    assert len(got) == len(pred)
    assert np.array_equal(got["pred"], pred)
    assert np.array_equal((got["sched"] & abi.F_ALIVE) != 0, alive)


def _check_aggregate(eng, masks, pred, alive):
    """One kwk_aggregate (the engine's own buffer) against the reference and kwk_stats."""
    names = eng.p.names
    n_out = eng.aggregate(masks)
    assert n_out == len(names) + len(masks)
    out = eng.aggregate_read(n_out)
    fired = eng.stats()["fired_per_stage"]
    assert out[:len(names)].tolist() == [float(fired[s]) for s in names]
    assert out[len(names):].tolist() == ref_counts(pred, alive, masks).astype(np.float64).tolist(), masks
    return out


FMTS = list(CU.FORMATS)


def _hip():
    """The HIP runtime the engine library is linked to (its symbols resolve through the library's
    handle).  torch bundles a runtime of its own, which finds no device in a process where the
    engine's runtime has opened it already, so the tests' own device buffer, their device copies
    and the CU count come from here."""
    L = abi.lib()
    L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]  # kind: 1 H2D, 2 D2H, 3 D2D
    L.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    L.hipFree.argtypes = [C.c_void_p]
    L.hipDeviceGetAttribute.argtypes = [C.POINTER(C.c_int), C.c_int, C.c_int]
    return L


# ---------------------------------------------------------------- kwk_count, every variant
@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FMTS)
def test_count_every_size_and_mask_set(fmt):
    """kwk_count for M1..M16 at n = C * W - r (C in 1, 255-257, 1023-1025, 2049 chunks; r in 0, 1,
    W - 1) and n = 1: a partial last chunk, each of a lane's four in-flight chunks filled or not,
    a second and a third block."""
    w = 16 // CU.FORMATS[fmt]
    sets = _mask_sets()
    ns = CU.sizes(w)
    rng = _rng("count", fmt)
    bad, first, last, chunk = [], False, False, False
    eng = _engine(fmt, max(ns))
    try:
        for case, n in enumerate(ns):
            pred, alive, _ = _load(eng, fmt, n, rng, case)
            first |= not alive[0]
            last |= not alive[-1]
            chunk |= bool((~alive[:n // w * w].reshape(-1, w)).all(axis=1).any())
            for name, masks in sets.items():
                got, want = eng.count(masks), ref_counts(pred, alive, masks)
                assert got.dtype == np.uint64
                if got.tolist() != want.tolist():
                    bad.append((n, name, got.tolist(), want.tolist()))
    finally:
        eng.close()
    assert not bad, f"{len(bad)} wrong counts, first (n, set, got, want): {bad[:4]}"
    assert first and last and chunk


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FMTS)
def test_aggregate_every_size(fmt):
    """kwk_aggregate + kwk_aggregate_read on the same columns with M3, M5 and M16: the count slots
    equal the reference, the stage slots kwk_stats, n_out = stages + masks; then again after sweeps,
    when the stage slots are no longer zero (the rows then as eng.read() shows them)."""
    from tests.parity_util import NOW0
    w = 16 // CU.FORMATS[fmt]
    sets = _mask_sets()
    rng = _rng("aggregate", fmt)
    eng = _engine(fmt, max(CU.sizes(w)))
    try:
        for case, n in enumerate(CU.sizes(w)):
            pred, alive, _ = _load(eng, fmt, n, rng, case)
            for name in ("M3", "M5", "M16"):
                _check_aggregate(eng, sets[name], pred, alive)
        for k in range(6):
            eng.step(NOW0 + k * 2 * 10**9, 9, k)
        got, _ = eng.read()
        assert sum(eng.stats()["fired_per_stage"].values()) > 0
        for name in ("M3", "M5", "M16"):
            _check_aggregate(eng, sets[name], got["pred"], (got["sched"] & abi.F_ALIVE) != 0)
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["rows512", "gridcap"])
def test_count_many_blocks_wide(which):
    """The wide format (2 objects per chunk) with M4 and M16 at more than 512 blocks (the second
    round of the row loops in count_total_block and agg_final_kernel's count waves) and past the
    grid cap of 8 blocks per CU (the grid-stride loop)."""
    cus = C.c_int(0)
    assert _hip().hipDeviceGetAttribute(C.byref(cus), 63, 0) == 0  # hipDeviceAttributeMultiprocessorCount
    cus = cus.value
    assert 1 <= cus <= 4096
    n = 2 * (512 * 1024 + 3) - 1 if which == "rows512" else 2 * (cus * 8 * 1024 + 1025) - 1
    sets = _mask_sets()
    eng = _engine("wide", n)
    try:
        pred, alive, _ = _load(eng, "wide", n, _rng("blocks", which), 15)
        for name in ("M4", "M16"):
            assert eng.count(sets[name]).tolist() == ref_counts(pred, alive, sets[name]).tolist(), name
            _check_aggregate(eng, sets[name], pred, alive)
    finally:
        eng.close()


# ---------------------------------------------------------------- stale rows, empty engines
def _plant_stale(eng, fmt, n, alive):
    """Copies live words of the column into the words past n of its last chunk (device to device,
    inside the state column's allocation) -> how many words."""
    wb = CU.FORMATS[fmt]
    w = 16 // wb
    k = -n % w
    assert 0 < k <= n
    run = np.convolve(alive.astype(np.int64), np.ones(k, dtype=np.int64), "valid") == k
    assert run.any()
    src = int(np.flatnonzero(run)[0])
    st = C.c_void_p()
    abi.check(abi.lib().kwk_device_ptrs(eng.h, C.byref(st), None, None), "kwk_device_ptrs", eng.h)
    eng.sync()
    hip = _hip()
    assert (n + k) * wb <= eng.capacity * wb
    assert hip.hipMemcpy(st.value + n * wb, st.value + src * wb, k * wb, 3) == 0  # hipMemcpyDeviceToDevice
    assert hip.hipDeviceSynchronize() == 0
    past, _ = eng.read(n, k)
    assert np.all((past["sched"] & abi.F_ALIVE) != 0)  # live rows past the end
    return k


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FMTS)
def test_counts_ignore_stale_rows_past_the_end(fmt):
    """The 1025-chunk column, then a shorter one whose end lies inside a chunk, by a second kwk_load
    and by kwk_relayout: counts follow the short column although the rest of its last chunk holds
    live words (put there by hand: both calls clear the tail themselves)."""
    w = 16 // CU.FORMATS[fmt]
    sets = _mask_sets()
    n_long = 1025 * w
    rng = _rng("stale", fmt)
    eng = _engine(fmt, n_long)
    try:
        for case, n in enumerate(sorted({n_long - 1, n_long - (w - 1), 256 * w + 1})):
            pred_l, alive_l, _ = _load(eng, fmt, n_long, rng, 5)
            assert eng.count(sets["M4"]).tolist() == ref_counts(pred_l, alive_l, sets["M4"]).tolist()
            # a second load of a shorter column (kwk_load accepts it)
            pred, alive, _ = _load(eng, fmt, n, rng, case)
            k = _plant_stale(eng, fmt, n, alive)
            for name in ("M4", "M16"):
                assert eng.count(sets[name]).tolist() == ref_counts(pred, alive, sets[name]).tolist(), (n, k, name)
                _check_aggregate(eng, sets[name], pred, alive)
            # the long column again, shortened in place by kwk_relayout (slots [0, n) stay)
            pred_l, alive_l, _ = _load(eng, fmt, n_long, rng, 6)
            eng.relayout([(0, 0, n)], n)
            assert eng.stats()["state_bytes"] == CU.FORMATS[fmt]
            pred, alive = pred_l[:n], alive_l[:n]
            _check_read(eng, pred, alive)
            k = _plant_stale(eng, fmt, n, alive)
            for name in ("M4", "M16"):
                assert eng.count(sets[name]).tolist() == ref_counts(pred, alive, sets[name]).tolist(), (n, k, name)
                _check_aggregate(eng, sets[name], pred, alive)
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FMTS)
def test_empty_engine_counts_zero(fmt):
    """No active object: zeros from kwk_count and kwk_aggregate, on a fresh engine, after an empty
    kwk_load over a loaded one and after kwk_relayout to n_active = 0."""
    w = 16 // CU.FORMATS[fmt]
    sets = _mask_sets()
    none = np.zeros(0, dtype=bool)
    eng = _engine(fmt, 257 * w)
    try:
        def zeros():
            for name in ("M1", "M4", "M16"):
                assert eng.count(sets[name]).tolist() == [0] * len(sets[name])
                _check_aggregate(eng, sets[name], none, none)
        zeros()
        rng = _rng("empty", fmt)
        pred, alive, _ = _load(eng, fmt, 257 * w - 1, rng, 0)
        _check_aggregate(eng, sets["M4"], pred, alive)  # leaves counts in the aggregate's buffer
        _load(eng, fmt, 0, rng)
        zeros()
        pred, alive, _ = _load(eng, fmt, 257 * w - 1, rng, 0)
        _check_aggregate(eng, sets["M4"], pred, alive)
        eng.relayout([], 0)
        zeros()
    finally:
        eng.close()


# ---------------------------------------------------------------- kwk_aggregate's state between calls
@pytest.mark.gpu
def test_aggregate_into_caller_buffer():
    """out_ptr: a device buffer of the caller's (hipMalloc; see _hip for why no torch tensor), filled
    with a sentinel.  After kwk_sync its first n_out doubles are the result and every double after
    them is untouched."""
    fmt, sets = "u32", _mask_sets()
    n = 1025 * 4 - 3
    hip = _hip()
    eng = _engine(fmt, n)
    buf = C.c_void_p()
    try:
        pred, alive, _ = _load(eng, fmt, n, _rng("out"), 7)
        masks = sets["M5"]
        host = np.full(64, -12345.678, dtype=np.float64)
        assert hip.hipMalloc(C.byref(buf), host.nbytes) == 0
        assert hip.hipMemcpy(buf, abi.ptr(host), host.nbytes, 1) == 0 and hip.hipDeviceSynchronize() == 0
        n_out = eng.aggregate(masks, out_ptr=buf.value)
        eng.sync()
        got = np.zeros(64, dtype=np.float64)
        assert hip.hipMemcpy(abi.ptr(got), buf, got.nbytes, 2) == 0
        n_st = len(eng.p.names)
        assert n_out == n_st + len(masks)
        assert got[:n_st].tolist() == [0.0] * n_st  # nothing has fired on this engine
        assert got[n_st:n_out].tolist() == ref_counts(pred, alive, masks).astype(np.float64).tolist()
        assert np.all(got[n_out:] == host[n_out:])
    finally:
        eng.close()
        if buf:
            hip.hipFree(buf)


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FMTS)
def test_aggregate_call_sequence(fmt):
    """One engine, changing masks and paths: the masks cached on the device, the aggregate's count
    buffer (zeroed only when no count runs) and the partial rows kwk_count shares."""
    w = 16 // CU.FORMATS[fmt]
    sets = _mask_sets()
    n = 1025 * w - 1
    rng = _rng("sequence", fmt)
    eng = _engine(fmt, n)
    try:
        pred, alive, _ = _load(eng, fmt, n, rng, 3)
        m4 = sets["M4"]
        other4 = [m4[3], m4[2], 0xFFFFFFFF, m4[1]]
        assert other4 != m4 and ref_counts(pred, alive, other4).tolist() != ref_counts(pred, alive, m4).tolist()
        _check_aggregate(eng, m4, pred, alive)            # 1
        _check_aggregate(eng, other4, pred, alive)        # 2: other masks, as many
        _check_aggregate(eng, sets["M2"], pred, alive)    # 3
        _check_aggregate(eng, sets["M16"], pred, alive)   # 4
        _check_aggregate(eng, sets["M1"], pred, alive)    # 5
        assert eng.count(sets["M8"]).tolist() == ref_counts(pred, alive, sets["M8"]).tolist()  # 6
        _check_aggregate(eng, m4, pred, alive)            # 7
        more = rng.choice(np.flatnonzero(alive), size=100, replace=False).astype(np.uint32)
        eng.delete(more)                                  # 8
        before = ref_counts(pred, alive, m4)
        alive[more] = False
        assert ref_counts(pred, alive, m4)[0] == before[0] - 100
        _check_aggregate(eng, m4, pred, alive)            # 9: the same masks, a changed state
        n_out = eng.aggregate([])                         # 10: stages only
        assert n_out == len(eng.p.names)
        assert eng.aggregate_read(n_out).tolist() == [0.0] * n_out
        _check_aggregate(eng, m4, pred, alive)
    finally:
        eng.close()


# ---------------------------------------------------------------- counts inside the usage pass
def _usage_mask_sets():
    b = _mask_sets()["M5"]
    u = b[1] | b[2]
    return [[0], [b[0]], [0, b[0]], [b[0], 0], [0, b[1], u], [b[1], 0, u], [b[1], u, 0], [0, b[0], b[1], u],
            [b[0], 0, b[1], u], [b[0], b[1], 0, u], [b[0], b[1], u, 0], [b[3], b[4], b[0], u]]


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["irregular-6000", "irregular-5997", "16-per-node"])
def test_counts_in_usage_pass(layout):
    """kwk_aggregate with usage on 1-byte ids, the 1-byte key column and uniform containers
    (usage_fast_kernel<1, true>): 1-4 masks, mask 0 first, in the middle and last, counted inside
    the usage pass (KWK_USAGE_AGG_FUSED), by the separate pass (flag off), and by the separate pass
    the engine falls back to by itself once an upsert has grown n_active past the usage
    configuration's pods.  Node layouts: empty nodes first, inside and last, 300 one-pod nodes, nodes
    of 2500, 1016 and 1017 pods and an odd chunk start (tests/test_usage._irregular_node_ptr); and
    16 pods per node, every lane's run exactly one node."""
    from tests.parity_util import NOW0
    from tests.test_usage import _irregular_node_ptr
    fmt = "auto"
    if layout == "16-per-node":
        n = 8192
        ptr = (np.arange(n // 16 + 1) * 16).astype(np.uint32)
    else:
        n = int(layout.split("-")[1])
        ptr = _irregular_node_ptr(n)
    assert ptr[-1] == n
    rng = _rng("usage", layout)
    cv, mv = rng.random(60) * 4, rng.random(70) * 2**32
    ci, mi, nc = rng.integers(0, 60, 200), rng.integers(0, 70, 200), rng.integers(1, 6, 200)
    dict_keys = (ci | (mi << 14) | (nc << 28)).astype(np.uint32)  # 200 keys, every pod's containers alike
    pick = rng.integers(0, 200, n)
    now = NOW0 + 10 * 10**9
    on, off = abi.USAGE_KEY8 | abi.USAGE_AGG_FUSED, abi.USAGE_KEY8
    eng = _engine(fmt, n + 8)
    try:
        pred, alive, _ = _load(eng, fmt, n, rng, 15)
        eng.usage_config(ptr, dict_keys[pick], cv, mv)
        n_st = len(eng.p.names)
        want_usage = np.array([np.where(alive, nc[pick] * cv[ci[pick]], 0.0).sum(),
                               np.where(alive, nc[pick] * mv[mi[pick]], 0.0).sum()])

        def run(masks, flag, fused, pred, alive):
            eng.set_tuning(abi.TUNE_USAGE, flag)
            info = eng.usage_info()
            assert info["kernel"] == "fast8"
            if len(masks) <= 4:  # (usage_info answers for 1-4 masks)
                assert info["fused_counts"] == fused, (info, flag)
            n_out = eng.aggregate(masks, now, usage=True)
            assert n_out == n_st + len(masks) + 2
            out = eng.aggregate_read(n_out)
            assert out[n_st:n_st + len(masks)].tolist() == ref_counts(pred, alive, masks).astype(np.float64).tolist(), \
                (masks, flag)
            np.testing.assert_allclose(out[-2:], want_usage, rtol=REL_TOL, atol=0)
            assert out[:n_st].tolist() == [0.0] * n_st
            return out

        for masks in _usage_mask_sets():
            a = run(masks, on, 1, pred, alive)
            b = run(masks, off, 0, pred, alive)
            assert a[-2:].tobytes() == b[-2:].tobytes()  # bit-identical usage slots
        run(_mask_sets()["M5"], on, 1, pred, alive)  # 5 masks: the separate pass, flag on
        run(_usage_mask_sets()[7], on, 1, pred, alive)
        # one more object than the usage configuration has pods: the separate pass by itself
        _, hot, dels, rec, cls, _ = _pool()
        j = int(np.flatnonzero(((hot["sched"] & abi.F_ALIVE) != 0) & (hot["pred"] != 0))[0])
        eng.upsert([n], hot[j:j + 1], dels[j:j + 1], rec[j:j + 1], cls[j:j + 1])
        assert eng.stats()["state_bytes"] == 1
        pred2, alive2 = np.append(pred, hot["pred"][j]), np.append(alive, True)
        _check_read(eng, pred2, alive2)
        for masks in _usage_mask_sets():
            run(masks, on, 0, pred2, alive2)
    finally:
        eng.close()


# ---------------------------------------------------------------- refusals
@pytest.mark.gpu
def test_too_many_masks_refused():
    """17 masks: KWK_EINVAL from kwk_count and kwk_aggregate, nothing changes, the next valid call is
    right; kwk_count of no masks returns an empty array."""
    fmt, sets = "u16", _mask_sets()
    n = 257 * 8 - 1
    eng = _engine(fmt, n)
    try:
        pred, alive, _ = _load(eng, fmt, n, _rng("refusals"), 2)
        m16 = sets["M16"]
        before = _check_aggregate(eng, m16, pred, alive)
        m17 = np.array(m16 + [1], dtype=np.uint32)
        out = np.full(17, 77, dtype=np.uint64)
        L = abi.lib()
        assert L.kwk_count(eng.h, 17, abi.ptr(m17), abi.ptr(out)) == abi.KWK_EINVAL
        assert L.kwk_last_error(eng.h).decode() == "at most 16 masks" and np.all(out == 77)
        n_out = C.c_uint32(99)
        assert L.kwk_aggregate(eng.h, 17, abi.ptr(m17), 0, 0, None, C.byref(n_out)) == abi.KWK_EINVAL
        assert L.kwk_last_error(eng.h).decode() == "at most 16 masks" and n_out.value == 99
        with pytest.raises(abi.EngineError, match="at most 16 masks"):
            eng.count(m17)
        assert eng.aggregate_read(len(before)).tolist() == before.tolist()  # the last result stands
        _check_read(eng, pred, alive)
        assert eng.count(m16).tolist() == ref_counts(pred, alive, m16).tolist()
        _check_aggregate(eng, sets["M4"], pred, alive)
        empty = eng.count([])
        assert empty.shape == (0,) and empty.dtype == np.uint64
    finally:
        eng.close()

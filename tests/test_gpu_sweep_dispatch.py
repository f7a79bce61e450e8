"""The host's kernel dispatch, pinned: which sweep launch_sweep picks for each state format and
tuning, the shape kwk_last_sweep reports for it, and which expansion the fired hand-back picks for
each record kind and list format — each selectable path stepped against the oracle.  What is
pinned is the shape the engine reports and the results: a table that swapped two instantiations
which compute the same (the two prefetch depths) would still pass, as would any persistent grid
of whole CUs.

The expected kwk_sweep_info fields are launch_sweep's rules restated here:
  * 2-byte words: q 16-byte chunks per lane (KWK_TUNE_SWEEP16), 2048 * q objects per tile; q falls
    to 1 while the tiles at q number fewer than 4 per CU.  Table-only (KWK_SWEEP_16_FSM) iff a
    transition table exists for the harness setting and the tuning's kernel is not 0.  Persistent
    iff twice the resident grid (CUs x blocks per CU, at most 8) is at most the tiles: never for
    a few tiles, always for 16 tiles per CU.  depth = the tuning's kernel when table-only and
    persistent, else 1.  steps stays 0.
  * 1-byte ids: q = 2, 8192 ids per tile, depth = the tuning's kernel when persistent (else 1),
    steps = the steps of the launch (1, 2 or 4).
  * 4- / 8-byte words and fused records: q = 4; 4096 (4-byte) or 2048 objects per tile; the grid is
    ceil(tiles / KWK_TUNE_WORD_TILES) when that is set, else min(tiles, max(ceil(tiles / (8 fused |
    4)), 5 per CU)); persistent with depth 2 iff the grid is smaller than the tiles.
Large engines are checked on a sample of slots (objects are independent within a step and the
Philox counter is the global slot: tests/test_scale_oracle.py), small ones on tile, wave and
64-slot boundaries and the lone object of the last tile."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

from kwok_amd.host import abi
from tests.parity_util import compare_state

SEED, NOW0, DT = 0x6B776F6B, 1_700_000_000 * 10**9, 10**9
FORMATS = (abi.COMPACT_REC, abi.COMPACT_PACKED, abi.COMPACT_PACKED16, abi.COMPACT_BITS)


@functools.lru_cache(maxsize=None)
def _cus():
    """Device 0's compute units, as kwk_engine_create reads them."""
    hip, v = C.CDLL("libamdhip64.so"), C.c_int(0)
    assert hip.hipDeviceGetAttribute(C.byref(v), 63, 0) == 0 and v.value > 0  # hipDeviceAttributeMultiprocessorCount
    return v.value


def _sample(n):
    """~400 slots: both sides of the first tiles' tile, wave and 64-slot boundaries, the last slots, a
    strided fill."""
    s = {0, n - 1, n - 2}
    for step, reach in ((64, 4096), (512, 4 * 8192), (2048, 16 * 8192)):
        for b in range(step, min(n, reach), step):
            s |= {b - 1, b}
    s |= set(range(3, n, max(1, n // 160)))
    return sorted(x for x in s if 0 <= x < n)


class _Run:
    """An engine of n objects tiled from a few variants, and the oracle over a sample of its slots."""

    def __init__(self, kind, state, n, harness=True):
        from bench import shard_pod_variants
        from kwok_amd import workload as W
        from kwok_amd.host.compiler import HarnessSpec, KindProgram
        from kwok_amd.host.engine import Engine, Ingest
        from kwok_amd.host.stages import load_stage_files
        from oracle.next_ref import load_stage_docs
        from oracle.sim import OracleSim
        if kind == "pod-fast":  # 3 stages, table-only: 1-byte ids with 2-byte fired records
            files = W.stage_paths(W.POD_FAST)
            variants = [W.pod_object("p", "n"), W.pod_object("p", "n", job=True)]
            docs = load_stage_docs(*files)
            self.prog = KindProgram(load_stage_files(*files), HarnessSpec())
            self.prog.explore(variants)
            idx = shard_pod_variants(0, n, SEED, 0.1)
        else:  # 6 stages, table-only: 1-byte ids whose per-stage counts do not fit scalar registers
            from tests import stage_fuzz as F
            assert not harness
            docs, variants = F.case("b8-chain-6")
            self.prog = F.compile_python(docs, variants)
            idx = np.arange(n, dtype=np.int64) % len(variants)
        ing = Ingest(self.prog)
        cols = ing.variant_columns(variants, idx)
        self.n, self.harness = n, harness
        self.eng = Engine(self.prog, capacity=n, state=state)
        try:
            self.eng.load_stages()
            self.eng.set_harness(harness)
            self.eng.load(*cols, ing.record_array())
        except Exception:
            self.eng.close()
            raise
        self.slots = _sample(n)
        self.sample = np.asarray(self.slots, dtype=np.int64)
        self.sim = OracleSim(docs, [variants[int(idx[s])] for s in self.slots], harness=harness, slots=self.slots)
        self.k = 0

    def set_harness(self, h):
        if h != self.harness:
            self.eng.set_harness(h)
            self.sim.harness = self.harness = h

    def now(self, k=None):
        return NOW0 + (self.k if k is None else k) * DT

    def check_list(self, what, slot, stage, flags):
        """The sampled slots of step self.k's list against the oracle's step; advances the step."""
        slot = np.asarray(slot).astype(np.int64)
        exp = sorted(self.sim.step(self.now(), SEED, self.k))
        sel = np.isin(slot, self.sample)
        got = sorted(zip(slot[sel].tolist(), np.asarray(stage)[sel].tolist(), np.asarray(flags)[sel].tolist()))
        assert got == exp, (what, "device-only", sorted(set(got) - set(exp))[:6], "oracle-only",
                            sorted(set(exp) - set(got))[:6])
        self.k += 1
        return len(exp)

    def check_state(self):
        from tests.test_scale_oracle import _rows_at
        compare_state(self.prog, self.eng, self.sim, self.k - 1, rows=_rows_at(self.eng, self.slots))

    def step(self, what, want, compact=None):
        """One kwk_step (or kwk_step_n of one step with a hand-back) checked: shape, list, state."""
        if compact is None:
            self.eng.step(self.now(), SEED, self.k)
        else:
            self.eng.step_n(1, self.now(), DT, SEED, self.k, compact)
        _check_info(what, self.eng.last_sweep(), want)
        if compact == "packed":
            pk = self.eng.fired_packed()
            slot, stage = pk & np.uint32(0x7FFFFFF), pk >> np.uint32(27)
            f = self.eng.fired()
            assert np.array_equal(f["slot"], slot) and np.array_equal(f["stage"], stage), what
        else:
            f = self.eng.fired()
        fired = self.check_list(what, f["slot"], f["stage"], f["flags"])
        self.check_state()
        return fired


def _check_info(what, info, want):
    """Every field of kwk_last_sweep; grid None: a persistent grid (whole CUs, at most 8 blocks each,
    the tiles at least twice as many)."""
    print(what, info)
    want = dict(want)
    if want["grid"] is None:
        cus = _cus()
        assert info["grid"] % cus == 0 and 1 <= info["grid"] // cus <= 8 and 2 * info["grid"] <= info["tiles"], (what, info)
        want["grid"] = info["grid"]
    assert info == want, (what, info, want)


def _want16(n, q, harness, lean, depth, persist=True):
    cus = _cus()
    if q > 1 and -(-n // (2048 * q)) < 4 * cus:
        q = 1
    tiles = -(-n // (2048 * q))
    w = dict(kernel=abi.SWEEP_16_FSM if lean else abi.SWEEP_16, q=q, persistent=0, depth=1, grid=tiles, tiles=tiles,
             harness=int(harness), steps=0)
    if persist and tiles >= 16 * cus:
        w.update(persistent=1, depth=depth if lean else 1, grid=None)
    else:
        assert not persist or tiles <= 2 * cus  # between the two the occupancy decides
    return w


def _want8(n, harness, depth, steps):
    cus, tiles = _cus(), -(-n // 8192)
    w = dict(kernel=abi.SWEEP_8, q=2, persistent=0, depth=1, grid=tiles, tiles=tiles, harness=int(harness), steps=steps)
    if tiles >= 16 * cus:
        w.update(persistent=1, depth=depth, grid=None)
    else:
        assert tiles <= 2 * cus
    return w


def _wantw(state, n, harness, word_tiles):
    cus = _cus()
    kernel, tile, tpb = {"u32": (abi.SWEEP_W4, 4096, 4), "wide": (abi.SWEEP_W8, 2048, 4),
                         "auto": (abi.SWEEP_WD, 2048, 8)}[state]
    tiles = -(-n // tile)
    grid = -(-tiles // word_tiles) if word_tiles else min(tiles, max(-(-tiles // tpb), cus * 5))
    return dict(kernel=kernel, q=4, persistent=int(grid < tiles), depth=2 if grid < tiles else 1, grid=grid, tiles=tiles,
                harness=int(harness), steps=0)


# the 2-byte sweep's kernels: (name, KWK_SWEEP16_SHAPE kernel, table) -> table-only?, its depth
SHAPES16 = [("table-d2", 2, 1, True), ("table-d1", 1, 1, True), ("general-d2", 2, 0, False), ("general-d1", 1, 0, False),
            ("general-k0", 0, 1, False)]


# ------------------------------------------------------------------ 2-byte words
@pytest.mark.gpu
@pytest.mark.parametrize("q", [1, 2, 4])
def test_sweep16_one_block_per_tile(q):
    """One tile plus one object at q: the last tile holds a single object, and for q > 1 the engine
    is small enough that q falls to 1.  The table-only shapes hand back inside the sweep
    (kwk_step_n with a hand-back: rec and packed), the general ones through the compaction."""
    r = _Run("pod-fast", "u16", 2048 * q + 1)
    try:
        fired = 0
        for name, kernel, table, lean in SHAPES16:
            r.eng.set_tuning(abi.TUNE_SWEEP16, abi.sweep16_shape(q=q, kernel=kernel, table=table))
            for h, compact in ((True, None), (False, True), (True, "packed")):
                r.set_harness(h)
                fired += r.step((q, name, h, compact), _want16(r.n, q, h, lean, kernel), compact)
        assert fired > len(r.slots) and r.eng.stats()["state_bytes"] == 2
    finally:
        r.eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("q", [1, 2, 4])
def test_sweep16_persistent(q):
    """16 tiles per CU at q (the last one partial): every shape runs on the persistent grid with its
    depth, and one block per tile when the tuning asks for no persistent grid."""
    r = _Run("pod-fast", "u16", 16 * _cus() * 2048 * q - 5)
    try:
        fired = 0
        for name, kernel, table, lean in SHAPES16:
            for h in (True, False):
                r.set_harness(h)
                r.eng.set_tuning(abi.TUNE_SWEEP16, abi.sweep16_shape(q=q, kernel=kernel, table=table))
                fired += r.step((q, name, h), _want16(r.n, q, h, lean, kernel))
        for name, kernel, table, lean in SHAPES16[1:3]:
            r.eng.set_tuning(abi.TUNE_SWEEP16, abi.sweep16_shape(q=q, persistent=0, kernel=kernel, table=table))
            fired += r.step((q, name, "not persistent"), _want16(r.n, q, False, lean, kernel, persist=False))
        assert fired > len(r.slots) and r.eng.stats()["state_bytes"] == 2
    finally:
        r.eng.close()


# ------------------------------------------------------------------ 1-byte ids
def _fused_steps(r, m, depth, what):
    """A launch of m steps (kwk_step_n, 2-byte hand-backs): its shape, every step's list by step."""
    from kwok_amd.host.engine import PinnedBuffer
    bufs = [(PinnedBuffer(2 * r.n + 64), PinnedBuffer(4 * (r.n // 2048 + 64))) for _ in range(m)]
    try:
        k0 = r.k
        r.eng.step_n(m, r.now(), DT, SEED, k0, "packed16")
        _check_info(what, r.eng.last_sweep(), _want8(r.n, r.harness, depth, m))
        infos = [r.eng.fetch_step(k0 + j, *bufs[j]) for j in range(m)]
        r.eng.fetch_wait()
        fired = 0
        for j, fi in enumerate(infos):
            assert fi["step"] == k0 + j and fi["format"] == abi.COMPACT_PACKED16, (what, j, fi)
            slot, stage, flags = abi.fired16_decode(bufs[j][0].array(np.uint16, fi["n_records"]),
                                                    bufs[j][1].array(np.uint32, fi["n_segs"]), fi["region_slots"])
            assert len(np.unique(slot)) == len(slot), (what, j)
            fired += r.check_list(what + (j,), slot, stage, flags)
        r.check_state()
        return fired
    finally:
        for a, b in bufs:
            a.close()
            b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("size", ["tile+1", "persistent"])
def test_sweep8_steps_per_launch(size):
    """The 1-byte sweep with 1, 2 and 4 steps per launch, both prefetch depths, the harness on and
    off; the launches of 2 and 4 steps hand every step's 2-byte list back in one launch (at most
    KWK_TUNE_COMPACT_SMALL segments) or a scan + expansion pair (one more than that)."""
    n = 8192 + 1 if size == "tile+1" else 16 * _cus() * 8192 - 5
    r = _Run("pod-fast", "auto", n)
    try:
        assert r.eng.stats()["state_bytes"] == 1
        r.eng.fired_keep(4)
        segs = 4 * -(-n // 8192)
        fired = 0
        for depth in (2, 1):
            r.eng.set_tuning(abi.TUNE_SWEEP16, abi.sweep16_shape(kernel=depth))
            for h in (True, False):
                r.set_harness(h)
                fired += r.step((size, depth, h, 1), _want8(n, h, depth, 1))
                for m in (2, 4):
                    r.eng.set_tuning(abi.TUNE_COMPACT_SMALL, min(8192, segs) - (1 if h else 0))
                    fired += _fused_steps(r, m, depth, (size, depth, h, m))
        assert fired > len(r.slots) and r.eng.stats()["state_bytes"] == 1
    finally:
        r.eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("size", ["tile+1", "persistent"])
def test_sweep8_more_than_4_stages(size):
    """Six stages: the 1-byte sweep that keeps its per-stage counts in LDS, never fused."""
    n = 8192 + 1 if size == "tile+1" else 16 * _cus() * 8192 - 5
    r = _Run("chain6", "auto", n, harness=False)
    try:
        assert r.eng.stats()["state_bytes"] == 1
        fired = 0
        for depth in (2, 1):
            r.eng.set_tuning(abi.TUNE_SWEEP16, abi.sweep16_shape(kernel=depth))
            for _ in range(2):
                fired += r.step((size, depth), _want8(n, False, depth, 1))
        r.eng.step_n(2, r.now(), DT, SEED, r.k, "packed16")  # not fused: the last launch took one step
        _check_info((size, "step_n"), r.eng.last_sweep(), _want8(n, False, 1, 1))
        assert fired > 0
    finally:
        r.eng.close()


@pytest.mark.gpu
def test_match_leaves_the_1_byte_format():
    """kwk_match on a 1-byte engine: back to the 2-byte words, the general sweep with the harness
    off, nothing fired; the steps before and after agree with the oracle."""
    r = _Run("pod-fast", "auto", 8192 + 1)
    try:
        r.step("before", _want8(r.n, True, 2, 1))
        before = r.eng.stats()["fired"]
        r.eng.match(r.now(), SEED, r.k)
        _check_info("match", r.eng.last_sweep(), _want16(r.n, 4, False, False, 2))
        st = r.eng.stats()
        assert st["state_bytes"] == 2 and st["fired"] == before
        r.step("after", _want16(r.n, 4, True, True, 2))
    finally:
        r.eng.close()


# ------------------------------------------------------------------ 4- / 8-byte words, fused records
@pytest.mark.gpu
@pytest.mark.parametrize("state", ["u32", "wide", "auto"])
def test_word_sweep_grid(state):
    """The C2 stage mix (general matcher: picks, jitter, value records) in 4-byte words, 8-byte
    words and fused records, two 4096-object tiles plus one object, every object against the oracle:
    harness on and off, KWK_TUNE_WORD_TILES unset (one tile per workgroup at this size) and 2."""
    from kwok_amd import workload as W
    from tests.parity_util import build
    cl = W.make_cluster("C2", 80, 8193, seed=31)
    objs = cl.pods.materialize()
    prog, eng, sim = build(cl.pod_stage_files, objs, harness=True, state=state)
    try:
        fired, k = 0, 0
        for h, word_tiles in ((True, 0), (True, 2), (False, 2), (False, 0)):
            eng.set_harness(h)
            sim.harness = h
            eng.set_tuning(abi.TUNE_WORD_TILES, word_tiles)
            now = NOW0 + k * 700 * 10**6
            eng.step(now, SEED, k)
            _check_info((state, h, word_tiles), eng.last_sweep(), _wantw(state, len(objs), h, word_tiles))
            got = sorted((int(x["slot"]), int(x["stage"]), int(x["flags"])) for x in eng.fired())
            exp = sorted(sim.step(now, SEED, k))
            assert got == exp, (state, k, sorted(set(got) - set(exp))[:6], sorted(set(exp) - set(got))[:6])
            compare_state(prog, eng, sim, k)
            fired += len(exp)
            k += 1
        assert fired > 0 and eng.stats()["state_bytes"] == (4 if state == "u32" else 8)
    finally:
        eng.close()


# ------------------------------------------------------------------ the hand-back's kernels
@pytest.mark.gpu
@pytest.mark.parametrize("records", ["slot", "id8", "id8-half"])
def test_handback_pick(records):
    """Each record kind the sweeps write (slot records: 2-byte words; id records: the 1-byte sweep
    with more than 4 stages; 2-byte id records: with at most 4) x the four list formats x at most
    KWK_TUNE_COMPACT_SMALL segments (one launch) and one more than that (scan + expansion): the
    list is the kwk_fired_rec list, which the oracle confirms on the sampled slots, in its order."""
    from tests.test_handback_formats import COMPACT_ARG, _check_list, _decode, _device_formats
    kind, state, tile = {"slot": ("pod-fast", "u16", 2048), "id8": ("chain6", "auto", 8192),
                         "id8-half": ("pod-fast", "auto", 8192)}[records]
    r = _Run(kind, state, 3 * tile + 1, harness=kind == "pod-fast")
    try:
        for _ in range(4):  # to a step that fires
            r.eng.step(r.now(), SEED, r.k)
            f = r.eng.fired()
            if r.check_list(records, f["slot"], f["stage"], f["flags"]) > 0:
                break
        segs = 4 * r.eng.last_sweep()["tiles"]
        assert segs == 16 and len(f) > 0 and len(np.unique(f["slot"])) == len(f)
        ref = _decode(abi.COMPACT_REC, f, None, None)
        for small in (segs, segs - 1):
            r.eng.set_tuning(abi.TUNE_COMPACT_SMALL, small)
            for fmt in FORMATS:
                what = (records, small, fmt)
                r.eng.fired_compact(COMPACT_ARG[fmt])
                left = fmt if records == "id8-half" or fmt in (abi.COMPACT_REC, abi.COMPACT_PACKED) else abi.COMPACT_PACKED
                assert _device_formats(r.eng) == [left], what
                _check_list(r.eng, left, ref, what)
                assert _device_formats(r.eng) == [left], what
    finally:
        r.eng.close()


# ------------------------------------------------------------------ error messages
def _in_thread(fn):
    out = {}
    t = threading.Thread(target=lambda: out.update(r=fn()))
    t.start()
    t.join()
    return out["r"]


def test_refused_call_without_an_engine_lands_in_the_threads_slot():
    """No device needed: a call without an engine is refused before anything else, its message is
    the calling thread's (kwk_last_error(NULL)) and no other thread's.  (Every refused call here runs
    on a thread of its own: this thread's slot stays as other tests expect it.)"""
    L = abi.lib()

    def refused():
        st = L.kwk_step(None, 0, 0, 0), L.kwk_last_error(None).decode()
        info = abi.SweepInfo()
        return st + (L.kwk_last_sweep(None, C.byref(info)), L.kwk_last_error(None).decode(),
                     L.kwk_match(None, 0, 0, 0), L.kwk_last_error(None).decode())

    before = L.kwk_last_error(None)
    assert _in_thread(refused) == (abi.KWK_EINVAL, "null engine", abi.KWK_EINVAL, "null argument", abi.KWK_EINVAL,
                                   "null engine")
    assert _in_thread(lambda: L.kwk_last_error(None).decode()) == ""
    assert L.kwk_last_error(None) == before


@pytest.mark.gpu
def test_refused_sweep_message_per_engine():
    """An engine exists only on a device: a sweep refused by launch_sweep leaves its message in its
    engine and in the calling thread's slot; a second engine's slot stays untouched."""
    from kwok_amd import workload as W
    from kwok_amd.host.compiler import KindProgram
    from kwok_amd.host.engine import Engine
    from kwok_amd.host.stages import load_stage_files
    prog = KindProgram(load_stage_files(*W.stage_paths(W.POD_FAST)))
    prog.explore([W.pod_object("p", "n")])
    e1, e2 = Engine(prog, capacity=64), Engine(prog, capacity=64)
    try:
        L = abi.lib()

        def refused():
            return L.kwk_step(e1.h, 0, 0, 0), L.kwk_last_error(None).decode()
        msg = "kwk_load_stages must be called before kwk_step"
        assert _in_thread(refused) == (abi.KWK_ESTATE, msg)
        assert L.kwk_last_error(e1.h).decode() == msg and L.kwk_last_error(e2.h).decode() == ""
        assert _in_thread(lambda: L.kwk_step_n(e2.h, 1, 0, 1, 0, 0, abi.COMPACT_REC, 0, 0)) == abi.KWK_ESTATE
        assert L.kwk_last_error(e2.h).decode() == msg and L.kwk_last_error(e1.h).decode() == msg
        no_engine = _in_thread(lambda: (L.kwk_step(None, 0, 0, 0), L.kwk_last_error(None).decode()))
        assert no_engine == (abi.KWK_EINVAL, "null engine")
        assert L.kwk_last_error(e1.h).decode() == msg  # a call without an engine touches no engine's slot
    finally:
        e1.close()
        e2.close()

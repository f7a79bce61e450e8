"""The fused 1-byte sweep's carried passes on the composite id table (id8_compose.hpp, DESIGN §5
"Composite id rows") against a twin stepped one kwk_step per call with KWK_TUNE_FUSE_STEPS 0 — that
kernel (`sweep8_kernel<..., 1>`) never reads the composite — on pod-fast with the bench harness.

The pod mix makes both paths of the fused kernels run in one launch: the first 8192-id tile holds
Job-owned pods only (the harness re-creates them for ever: 2048 items per wave, over the carry limit
of 2048 / kSteps, so the tile rebuilds its list at every step), every other pod is Job-owned with
probability 0.1 (about 205 items per wave: carried), and the last tile is partial.  Compared: the
states, EVERY step's 2-byte list and segment counts through the hand-back ring, and the fired /
matched / per-stage counts; the persistent case also compares the traffic statistics (bytes,
line_bytes) of the composite path with the one-tile kernels', which look each step up in the id table."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NOW0 = 1_700_000_000 * 10**9
DT = 10**9
SEED = 0x6B776F6B
TILE = 8192
SMALL = 4 * TILE + 5000  # five tiles, the last one partial
STEPS = 12               # launches of 4 + 4 + 4 (fuse 4) / six pairs (fuse 2); the first launch sees every pod dirty


def _program():
    from kwok_amd import workload as W
    from kwok_amd.host.compiler import HarnessSpec, KindProgram
    from kwok_amd.host.stages import load_stage_files
    pvars = [W.pod_object("p", "n"), W.pod_object("p", "n", job=True)]
    prog = KindProgram(load_stage_files(*W.stage_paths(W.POD_FAST)), HarnessSpec())
    prog.explore(pvars)
    return prog, pvars


def _mix(n):
    from bench import shard_pod_variants
    idx = shard_pod_variants(0, n, SEED, 0.1)
    idx[:TILE] = 1
    return idx


def _engine(prog, cols, records, fuse, persistent=1):
    from kwok_amd.host import abi
    from kwok_amd.host.engine import Engine
    eng = Engine(prog, capacity=len(cols[0]), state="auto")
    eng.set_tuning(abi.TUNE_FUSE_STEPS, fuse)
    if not persistent:
        eng.set_tuning(abi.TUNE_SWEEP16, abi.sweep16_shape(persistent=0))
    eng.load_stages()
    eng.set_harness(True)
    eng.load(*cols, records)
    assert eng.stats()["state_bytes"] == 1
    return eng


def _new_word_pods(k):
    """Running pods with a podIP and a finalizer: words outside the closure of the loaded pods."""
    from kwok_amd import workload as W
    out = []
    for i in range(k):
        o = W.pod_object(f"q{i}", "n", job=bool(i & 1))
        o["metadata"]["finalizers"] = ["kwok.x-k8s.io/fake"]
        o["status"] = {"phase": "Running", "podIP": "10.0.0.9"}
        out.append(o)
    return out


class _Twin:
    """The per-step reference of one size, computed once: every step's list, then states and counts
    at the steps the fused engines are compared at."""

    def __init__(self, n, upsert_slots):
        from kwok_amd.host.engine import Ingest
        self.n = n
        self.prog, self.pvars = _program()
        ing = Ingest(self.prog)
        self.idx = _mix(n)
        self.cols = ing.variant_columns(self.pvars, self.idx)
        self.records = ing.record_array()
        self.upsert_slots = np.asarray(upsert_slots, dtype=np.uint32)
        self.upsert_cols = Ingest(self.prog).columns(_new_word_pods(len(upsert_slots)))
        ref = _engine(self.prog, self.cols, self.records, 0)
        try:
            self.lists, self.marks = [], {}
            for k in range(STEPS + 4):
                if k == STEPS:
                    self.marks[STEPS] = (ref.read()[0], ref.stats())
                    ref.upsert(self.upsert_slots, *self.upsert_cols)
                ref.step(NOW0 + k * DT, SEED, k)
                ref.fired_compact("16")
                recs, segc, rs = ref.fired_packed16()
                self.lists.append((recs.copy(), segc.copy(), rs))
            self.marks[STEPS + 4] = (ref.read()[0], ref.stats())
        finally:
            ref.close()

    def check(self, eng, fuse, persistent):
        """STEPS steps in fused launches, an upsert of pods whose words extend the dictionary (both
        composites are rebuilt with the id table), four more steps."""
        from kwok_amd.host import abi
        from kwok_amd.host.engine import PinnedBuffer
        cap = eng.capacity
        bufs = [(PinnedBuffer(2 * cap + 64), PinnedBuffer(4 * (cap // 2048 + 64))) for _ in range(STEPS)]
        try:
            eng.fired_keep(16)
            for k0, n_steps in ((0, STEPS), (STEPS, 4)):
                if k0:
                    eng.upsert(self.upsert_slots, *self.upsert_cols)
                eng.step_n(n_steps, NOW0 + k0 * DT, DT, SEED, k0, "packed16")
                info = eng.last_sweep()
                assert info["kernel"] == abi.SWEEP_8 and info["steps"] == fuse and info["persistent"] == persistent, info
                infos = [eng.fetch_step(k0 + j, *bufs[j]) for j in range(n_steps)]
                eng.fetch_wait()
                for j, fi in enumerate(infos):
                    recs, segc, rs = self.lists[k0 + j]
                    out, cnt = bufs[j]
                    assert fi["format"] == abi.COMPACT_PACKED16 and fi["region_slots"] == rs, (k0 + j, fi)
                    assert fi["n_records"] == len(recs) and fi["n_segs"] == len(segc), (k0 + j, fi)
                    assert len(recs) > 0, k0 + j
                    assert np.array_equal(cnt.array(np.uint32, fi["n_segs"]), segc), k0 + j
                    assert np.array_equal(out.array(np.uint16, fi["n_records"]), recs), k0 + j
                hot, st = self.marks[k0 + n_steps]
                got = eng.read()[0]
                for col in ("pred", "sched"):
                    assert np.array_equal(got[col], hot[col]), (k0, col)
                gst = eng.stats()
                for key in ("fired", "matched", "steps", "fired_per_stage"):
                    assert gst[key] == st[key], (k0, key, gst[key], st[key])
        finally:
            for x in bufs:
                for p in x:
                    p.close()
        return eng.stats()


_twins = {}


def _twin(n):
    if n not in _twins:
        _twins.clear()  # one size's columns at a time
        # the new words land in carried tiles: the second (full) and the last (partial) one
        _twins[n] = _Twin(n, list(range(TILE + 100, TILE + 110)) + list(range(n - 7, n - 2)))
    return _twins[n]


def _persistent_size(fuse):
    """The smallest pod count whose fused launch takes the persistent grid on this device.  The sweep
    goes persistent once the tiles are twice the resident workgroups; an empty engine (one pod
    upserted at the end sets the active count) is doubled until kwk_last_sweep reports the persistent
    grid, whose size is that number of workgroups."""
    from kwok_amd.host import abi
    from kwok_amd.host.engine import Engine, Ingest
    prog, pvars = _program()
    ing = Ingest(prog)
    one = ing.variant_columns(pvars, np.zeros(1, dtype=np.int32))
    eng = Engine(prog, capacity=1 << 26, state="auto")
    try:
        eng.set_tuning(abi.TUNE_FUSE_STEPS, fuse)
        eng.load_stages()
        eng.set_harness(True)
        eng.load(*one, ing.record_array())
        tiles = 2
        while tiles * TILE <= eng.capacity:
            eng.upsert(np.array([tiles * TILE - 1]), *one)
            eng.step_n(fuse, NOW0, DT, SEED, 0, "packed16")
            info = eng.last_sweep()
            assert info["steps"] == fuse and info["tiles"] == tiles, info
            if info["persistent"]:
                assert 2 * info["grid"] <= tiles < 4 * info["grid"], info
                return (2 * info["grid"] - 1) * TILE + 5000
            tiles *= 2
    finally:
        eng.close()
    raise AssertionError("no persistent grid up to 64M pods")


@pytest.mark.parametrize("fuse", [4, 2])
def test_mixed_tiles_one_tile_grid_equal_per_step_calls(fuse):
    """Five tiles, one workgroup each (these kernels keep the id-table lookups per step): the rebuilt
    first tile, three carried tiles and the partial one, and the dictionary extension."""
    t = _twin(SMALL)
    eng = _engine(t.prog, t.cols, t.records, fuse)
    try:
        t.check(eng, fuse, 0)
    finally:
        eng.close()


@pytest.mark.parametrize("fuse", [4, 2])
def test_mixed_tiles_persistent_grid_equal_per_step_calls(fuse):
    """The same pod mix at the smallest size the fused launch runs persistent at, where the carried
    passes read the composite rows: lists, states and counts equal the per-step twin's, also after
    an upsert between two fused launches brings words that are not in the dictionary (the second
    launch steps them from rebuilt composites); and the traffic statistics equal those of the same
    launches on the one-tile kernels (KWK_TUNE_SWEEP16 without the persistent grid)."""
    n = _persistent_size(fuse)
    t = _twin(n)
    eng = _engine(t.prog, t.cols, t.records, fuse)
    try:
        st = t.check(eng, fuse, 1)
    finally:
        eng.close()
    one = _engine(t.prog, t.cols, t.records, fuse, persistent=0)
    try:
        one.step_n(STEPS, NOW0, DT, SEED, 0, "packed16")
        one.upsert(t.upsert_slots, *t.upsert_cols)
        one.step_n(4, NOW0 + STEPS * DT, DT, SEED, STEPS, "packed16")
        assert one.last_sweep()["persistent"] == 0 and one.last_sweep()["steps"] == fuse
        ost = one.stats()
        for key in ("bytes", "line_bytes", "fired", "matched", "fired_per_stage"):
            assert st[key] == ost[key], (key, st[key], ost[key])
    finally:
        one.close()


def test_fused_lists_of_sampled_slots_equal_the_oracle():
    """Every step's fetched list of a fused run at the small size, decoded on the host, against
    OracleSim on a sample of slots from every tile (rebuilt, carried, partial)."""
    from kwok_amd import workload as W
    from kwok_amd.host import abi
    from kwok_amd.host.engine import PinnedBuffer
    from oracle.next_ref import load_stage_docs
    from oracle.sim import OracleSim
    from tests.parity_util import compare_state
    t = _twin(SMALL)
    slots = list(range(3, SMALL, 97))
    sample = np.asarray(slots, dtype=np.int64)
    sim = OracleSim(load_stage_docs(*W.stage_paths(W.POD_FAST)), [t.pvars[int(t.idx[s])] for s in slots], harness=True,
                    slots=slots)
    eng = _engine(t.prog, t.cols, t.records, 4)
    bufs = [(PinnedBuffer(2 * SMALL + 64), PinnedBuffer(4 * (SMALL // 2048 + 64))) for _ in range(STEPS)]
    try:
        eng.fired_keep(16)
        eng.step_n(STEPS, NOW0, DT, SEED, 0, "packed16")
        assert eng.last_sweep()["steps"] == 4
        infos = [eng.fetch_step(k, *bufs[k]) for k in range(STEPS)]
        eng.fetch_wait()
        total = 0
        for k, fi in enumerate(infos):
            out, cnt = bufs[k]
            slot, stage, flags = abi.fired16_decode(out.array(np.uint16, fi["n_records"]),
                                                    cnt.array(np.uint32, fi["n_segs"]), fi["region_slots"])
            assert len(np.unique(slot)) == len(slot), f"step {k}: a slot fired twice"
            sel = np.isin(slot.astype(np.int64), sample)
            got = sorted(zip(slot[sel].tolist(), stage[sel].tolist(), flags[sel].tolist()))
            exp = sorted(sim.step(NOW0 + k * DT, SEED, k))
            assert got == exp, f"step {k}: device-only {sorted(set(got) - set(exp))[:6]} oracle-only " \
                               f"{sorted(set(exp) - set(got))[:6]}"
            total += len(exp)
        assert total > len(slots)
        hot, dels = eng.read()
        compare_state(t.prog, eng, sim, STEPS - 1, rows=(hot[sample], dels[sample]))
    finally:
        eng.close()
        for x in bufs:
            for p in x:
                p.close()

"""Emission from the hand-back ring on the GPU (kwk_emit_step, kwk_ring_view, the output sets;
DESIGN.md §5 "Emission from the ring"): every step of a kwk_step_n call — the fused 1-byte sweep's
2-byte KWK_COMPACT_PACKED16 lists, 4-byte and 8-byte ring lists — emitted from its ring slot, the
emissions of a call enqueued back to back into output sets of their own.

The yardstick is the per-step emitter (kwk_emit) on an unfused twin engine loaded identically:
tests/test_gpu_emit.py pins it byte for byte to kwk_patch_render.  The engine gives the same
(slot, stage) sequence in every list format and between fused and per-step sweeps, so for every step
the items (rec, tid, status), the offsets and the bytes must be IDENTICAL, and so must the
emitter's words afterwards.  Each reference run is computed once and shared."""
import functools

import numpy as np
import pytest

from kwok_amd import workload as W

pytestmark = pytest.mark.gpu

NOW0, DT, SEED = 1_700_000_000 * 10**9, 10**9, 0x6B776F6B
N_FAST = 5 * 2048 + 1500            # five whole 2048-slot segments and a partial one
# A whole segment between live ranges that must turn up with no record in a non-empty list: its pods
# are deleted before the run, and all of them are plain pods — the harness re-creates what was
# deleted (churn), so the range fires once more (pod-ready) and then stays settled for good, while
# the Job-owned pods of the segments around it keep cycling.
DEAD = (2 * 2048, 3 * 2048)
N_C2 = 5000


class Twin:
    """One engine + emitter over the bench's variant pods (words from the variants, synthetic call values)."""

    def __init__(self, mix, n, fuse, harness=True, dead=None):
        import bench
        from kwok_amd.host import abi, emit
        from kwok_amd.host.compiler import HarnessSpec, KindProgram
        from kwok_amd.host.engine import Engine, Ingest
        from kwok_amd.host.patchtpl import PatchProgram
        from kwok_amd.host.stages import load_stage_files
        if mix == "fast":
            # Job-owned pods cycle ready -> complete -> delete (no patch) -> re-created: a third of
            # them starts Running and a third with a deletionTimestamp, so every step has all three
            # kinds of record and no step's list is deletes only
            running = W.pod_object("p", "n", job=True)
            running["status"] = {"phase": "Running", "podIP": "10.0.0.9", "hostIP": "10.0.0.1",
                                 "containerStatuses": [{"name": "container-0", "ready": True}]}
            pvars = [W.pod_object("p", "n"), W.pod_object("p", "n", job=True), running,
                     W.pod_object("p", "n", job=True, deletion="2023-11-14T00:00:00Z")]
            pidx = bench.shard_pod_variants(0, n, SEED, 0.1)
            if dead:
                pidx[dead[0]:dead[1]] = 0
            jobs = np.flatnonzero(pidx == 1)
            pidx[jobs[1::3]] = 2
            pidx[jobs[2::3]] = 3
            files = W.POD_FAST
        else:
            pvars, pidx = W.c2_pod_variants(0, n, seed=SEED, job_frac=0.1)
            files = W.POD_GENERAL + W.POD_CHAOS
        prog = KindProgram(load_stage_files(*W.stage_paths(files)), HarnessSpec())
        prog.explore(pvars)
        ing = Ingest(prog)
        hot, dels, rec, cls = ing.variant_columns(pvars, pidx)
        self.n = n
        self.eng = Engine(prog, capacity=n, max_records=max(1, len(ing.records)) + 16)
        self.em = None
        try:
            if not fuse:
                self.eng.set_tuning(abi.TUNE_FUSE_STEPS, 0)
            self.eng.load_stages()
            self.eng.set_harness(harness)
            self.eng.load(hot, dels, rec, cls, ing.record_array())
            if dead:
                self.eng.delete(np.arange(*dead, dtype=np.uint32))
            pp = PatchProgram(prog.stages, {"NodeIPWith": lambda *a: "10.100.100.100",
                                            "PodIPWith": lambda *a: "11.100.100.100"})
            vcls = [prog.class_of(v, register=False) for v in pvars]
            ep = emit.EmitProgram(prog.stages, pp, dict(zip(vcls, pvars)), len(prog.class_ids), stride=16)
            wv = []
            for c, v in zip(vcls, pvars):
                acc = 0
                for tid in range(ep.host_tid):
                    sk = ep.skel.get((c, tid))
                    if sk is not None:
                        acc |= int(pp.object_values(tid, [v], sk["text"], sk["calls"], ep.stride)[1][0]) << tid
                wv.append(c | ep.guard_bits(v) << 16 | acc << 32)
            self.em = emit.Emitter(self.eng, n, ep)
            self.em.set_rows(0, np.asarray(wv, dtype=np.uint64)[pidx], {})
            for c in range(ep.n_columns):
                self.em.set_column(c, 0, bench.synth_ipv4(0, n, 10 + c, ep.stride))
        except Exception:
            self.close()
            raise

    def words(self):
        return self.em.words(0, self.n)

    def close(self):
        if self.em is not None:
            self.em.close()
        self.eng.close()


@functools.lru_cache(maxsize=None)
def reference(mix, n, steps, fmt, harness=True, dead=None):
    """The per-step emitter on the unfused twin: per step (items, offsets, bytes, words after it)."""
    t = Twin(mix, n, fuse=False, harness=harness, dead=dead)
    try:
        out = []
        for k in range(steps):
            t.eng.step(NOW0 + k * DT, SEED, k)
            t.eng.fired_compact(packed=fmt == "packed")
            items, offs, data = t.em.run(NOW0 + k * DT, packed=fmt == "packed")
            out.append((items, offs, data, t.words()))
        return out
    finally:
        t.close()


def churn_reference():
    """Twelve steps of the pod-fast twin with churn and the deleted segment (4-byte lists): three
    fused groups' worth, shared by the tests that run a prefix of them."""
    return reference("fast", N_FAST, 12, "packed", True, DEAD)


def room(ref):
    return max(len(r[0]) for r in ref) + 1, max(len(r[2]) for r in ref) + 1


def same(got, want, what):
    items, offs, data = got
    assert len(items) == len(want[0]), what
    for f in ("rec", "tid", "status"):
        assert np.array_equal(items[f], want[0][f]), (what, f)
    assert np.array_equal(offs, want[1]), what
    assert data == want[2], what


def seg_counts(eng, step):
    from kwok_amd.host.engine import PinnedBuffer
    out, cnt = PinnedBuffer(2 * eng.capacity + 64), PinnedBuffer(4 * (eng.capacity // 512 + 64))
    try:
        info = eng.fetch_step(step, out, cnt)
        eng.fetch_wait()
        return cnt.array(np.uint32, info["n_segs"]).copy(), info["n_records"]
    finally:
        out.close()
        cnt.close()


def test_fused_two_byte_lists_emit_what_the_per_step_emitter_emits():
    from kwok_amd.host import abi, emit
    ref = churn_reference()[:8]
    t = Twin("fast", N_FAST, fuse=True, dead=DEAD)
    try:
        assert t.eng.stats()["state_bytes"] == 1
        t.eng.fired_keep(8)
        t.em.reserve_sets(8, *room(ref))
        t.eng.step_n(8, NOW0, DT, SEED, 0, "packed16")
        assert t.eng.last_sweep()["steps"] == 4
        views = [t.eng.fired_view(k) for k in range(8)]
        for k, v in enumerate(views):
            assert v["format"] == abi.COMPACT_PACKED16 and v["n_segs"] >= 3 and v["step"] == k, v
            assert v["list"] and v["count"] and v["seg_counts"] and v["region_slots"] * v["n_segs"] >= N_FAST
        for k in range(8):  # back to back: no synchronisation between the emissions
            t.em.emit_step(k, NOW0 + k * DT)
        for k in range(8):
            t.em.select(7 - k)
            same(t.em.collect(), ref[k], f"step {k}")
        assert np.array_equal(t.words(), ref[7][3])
        # the lists exercised every path of the segment lookup
        big = span = hole = ragged = False
        for k in range(8):
            c, n = seg_counts(t.eng, k)
            assert n == int(c.sum()), k
            base = np.concatenate(([0], np.cumsum(c)))
            if k == 0:
                big = bool(np.any(c > 256))  # every pod fires: a segment fills whole tiles
            elif n:
                first = np.searchsorted(base, np.arange(0, n, 256), side="right") - 1
                last = np.searchsorted(base, np.minimum(np.arange(0, n, 256) + 255, n - 1), side="right") - 1
                span = span or bool(np.any(last > first))
            nz = np.flatnonzero(c)
            hole = hole or (n > 0 and bool(np.any(c[nz[0]:nz[-1] + 1] == 0)))
            ragged = ragged or n % 256 != 0
            assert n == 0 or np.any(ref[k][0]["status"] == emit.STATUS_OK), k  # no step of deletes only
        assert big and span and hole and ragged, (big, span, hole, ragged)
        status = np.concatenate([r[0]["status"] for r in ref])
        assert 2 * int((status == emit.STATUS_OK).sum()) >= len(status) > 0
    finally:
        t.close()


def test_a_run_of_empty_segments_wider_than_the_lds_window():
    """A tile whose records lie either side of 290 empty segments: its segment range does not fit
    the emitter's LDS window (264 entries), so its records are searched in global memory — over
    the tile's own range.  Step 0 (every pod fires) is compared by its totals, the later steps
    whole."""
    n, gap = 300 * 2048 + 700, (5 * 2048, 295 * 2048)
    runs = {}
    for fuse in (False, True):
        t = Twin("fast", n, fuse=fuse, dead=gap)
        try:
            if fuse:
                t.eng.fired_keep(4)
                t.em.reserve_sets(4, *runs[False]["room"])
                t.eng.step_n(4, NOW0, DT, SEED, 0, "packed16")
                assert t.eng.last_sweep()["steps"] == 4
                for k in range(4):
                    t.em.emit_step(k, NOW0 + k * DT)
                t.em.select(3)
                got = [t.em.result()]
                for k in (1, 2, 3):
                    t.em.select(3 - k)
                    got.append(t.em.collect())
                spans = 0
                for k in (1, 2, 3):
                    c, cnt = seg_counts(t.eng, k)
                    base = np.concatenate(([0], np.cumsum(c)))
                    starts = np.arange(0, cnt, 256)
                    first = np.searchsorted(base, starts, side="right") - 1
                    last = np.searchsorted(base, np.minimum(starts + 255, cnt - 1), side="right") - 1
                    spans += int(np.sum(last - first + 2 > 264))
                assert spans >= 1  # the global-memory search ran
            else:
                got = []
                for k in range(4):
                    t.eng.step(NOW0 + k * DT, SEED, k)
                    t.eng.fired_compact(packed=True)
                    if k == 0:
                        t.em.reserve(2 * n, 2048 * n)
                        t.em.emit(NOW0, packed=True)
                        got.append(t.em.result())
                        assert got[0][0] > 0
                    else:
                        got.append(t.em.run(NOW0 + k * DT, packed=True))
            runs[fuse] = {"got": got, "words": t.words(),
                          "room": (got[0][0] + 1, got[0][1] + 1)}
        finally:
            t.close()
    assert runs[True]["got"][0] == runs[False]["got"][0]
    for k in (1, 2, 3):
        assert len(runs[False]["got"][k][0]) > 0 and len(runs[False]["got"][k][2]) > 0
        same(runs[True]["got"][k], runs[False]["got"][k], f"step {k}")
    assert np.array_equal(runs[True]["words"], runs[False]["words"])


def test_a_step_in_which_nothing_fires_is_an_empty_emission():
    """No churn: the pods settle, and later steps of the fused groups fire nothing."""
    ref = reference("fast", N_FAST, 8, "packed", False, None)
    sizes = [len(r[0]) for r in ref]
    assert 0 in sizes and sizes[0] > 0, sizes
    t = Twin("fast", N_FAST, fuse=True, harness=False)
    try:
        t.eng.fired_keep(8)
        t.em.reserve_sets(8, *room(ref))
        t.eng.step_n(8, NOW0, DT, SEED, 0, "packed16")
        assert t.eng.last_sweep()["steps"] == 4
        for k in range(8):
            t.em.emit_step(k, NOW0 + k * DT)
        for k in range(8):
            t.em.select(7 - k)
            assert t.em.result() == (len(ref[k][0]), len(ref[k][2])), k
            same(t.em.collect(), ref[k], f"step {k}")
        assert np.array_equal(t.words(), ref[7][3])
    finally:
        t.close()


def test_an_engine_with_nothing_active_emits_nothing():
    """After lists of thousands of records, the engine is reloaded empty: its steps sweep nothing
    (n_segs == 0), and their emissions must not read the ring slots' earlier lengths or lists."""
    from kwok_amd.host import abi
    t = Twin("fast", N_FAST, fuse=True)
    try:
        t.eng.fired_keep(4)
        t.em.reserve_sets(4, 16 * N_FAST, 4096 * N_FAST)
        t.eng.step_n(4, NOW0, DT, SEED, 0, "packed16")
        t.em.emit_step(0, NOW0)
        assert t.em.result()[0] > 0
        before = t.words()
        t.eng.load(np.zeros(0, dtype=abi.HOT_DTYPE), [], [], [])
        t.eng.step_n(4, NOW0 + 4 * DT, DT, SEED, 4, "packed16")
        for k in range(4, 8):
            assert t.eng.fired_view(k)["n_segs"] == 0
            t.em.emit_step(k, NOW0 + k * DT)
        for k in range(4, 8):
            t.em.select(7 - k)
            assert t.em.result() == (0, 0), k
            items, offs, data = t.em.collect()
            assert len(items) == 0 and list(offs) == [0] and data == b""
        assert np.array_equal(t.words(), before)
    finally:
        t.close()


@pytest.mark.parametrize("mix,n,steps,fmt", [("fast", N_FAST, 4, "packed"), ("general", N_C2, 3, "packed"),
                                             ("general", N_C2, 3, "rec")])
def test_four_and_eight_byte_ring_lists(mix, n, steps, fmt):
    from kwok_amd.host import abi
    dead = DEAD if mix == "fast" else None
    ref = churn_reference()[:steps] if mix == "fast" else reference(mix, n, steps, fmt, True, dead)
    assert sum(len(r[0]) for r in ref) > 0
    t = Twin(mix, n, fuse=True, dead=dead)
    try:
        t.eng.fired_keep(4)
        t.eng.step_n(steps, NOW0, DT, SEED, 0, "packed" if fmt == "packed" else True)
        if mix == "fast":
            assert t.eng.last_sweep()["steps"] == 4  # fused: enqueue_compact wrote per-step 4-byte slots
        else:
            assert t.eng.last_sweep()["steps"] < 2 and t.eng.stats()["state_bytes"] > 1  # not fused
        want = abi.COMPACT_PACKED if fmt == "packed" else abi.COMPACT_REC
        for k in range(steps):
            v = t.eng.fired_view(k)
            assert v["format"] == want and v["seg_counts"] is None, v
            same(t.em.run_step(k, NOW0 + k * DT), ref[k], f"step {k}")
        assert np.array_equal(t.words(), ref[steps - 1][3])
    finally:
        t.close()


def test_overflow_with_emissions_in_flight():
    """Sets with room for the first two steps of a fused group and not for the third: the third
    and the fourth both read KWK_ECAP and leave the words as the second left them; with room, the two
    emitted again are exact."""
    from kwok_amd.host import abi
    ref = churn_reference()
    ni, nb = [len(r[0]) for r in ref], [len(r[2]) for r in ref]
    # a fused group whose third step is larger than its first two (the reference's own counts)
    groups = [g for g in (4, 8) if ni[g + 2] > max(ni[g], ni[g + 1]) or nb[g + 2] > max(nb[g], nb[g + 1])]
    assert groups, (ni, nb)
    g = groups[0]
    t = Twin("fast", N_FAST, fuse=True, dead=DEAD)
    try:
        t.eng.fired_keep(8)
        t.em.reserve_sets(8, *room(ref))
        for g0 in range(0, g, 4):  # the groups before it, emitted as usual
            t.eng.step_n(4, NOW0 + g0 * DT, DT, SEED, g0, "packed16")
            for k in range(g0, g0 + 4):
                t.em.emit_step(k, NOW0 + k * DT)
            t.em.select(0)
            assert t.em.result() == (ni[g0 + 3], nb[g0 + 3])
        assert np.array_equal(t.words(), ref[g - 1][3])
        t.em.reserve_sets(4, max(ni[g], ni[g + 1]), max(nb[g], nb[g + 1]))  # another number of sets: fresh ones
        t.eng.step_n(4, NOW0 + g * DT, DT, SEED, g, "packed16")
        assert t.eng.last_sweep()["steps"] == 4
        for k in range(g, g + 4):
            t.em.emit_step(k, NOW0 + k * DT)
        for k in (g, g + 1):
            t.em.select(g + 3 - k)
            same(t.em.collect(), ref[k], f"step {k}")
        for k in (g + 2, g + 3):
            t.em.select(g + 3 - k)
            st = emit_result_status(t.em)
            assert st == abi.KWK_ECAP, (k, st)
        assert np.array_equal(t.words(), ref[g + 1][3])
        t.em.reserve_sets(4, *room(ref))
        for k in (g + 2, g + 3):
            t.em.emit_step(k, NOW0 + k * DT)
        for k in (g + 2, g + 3):
            t.em.select(g + 3 - k)
            same(t.em.collect(), ref[k], f"step {k} again")
        assert np.array_equal(t.words(), ref[g + 3][3])
    finally:
        t.close()


def emit_result_status(em):
    import ctypes as C
    from kwok_amd.host import emit
    a, b = C.c_uint32(), C.c_uint64()
    return emit.lib().kwk_emit_result(em.h, C.byref(a), C.byref(b))


def test_refusals():
    from kwok_amd.host import abi
    t = Twin("fast", N_FAST, fuse=True)
    try:
        t.eng.fired_keep(4)
        t.eng.step_n(8, NOW0, DT, SEED, 0, "packed16")
        with pytest.raises(abi.EngineError, match=r"\(-4\).*no kept list of step 3"):
            t.em.emit_step(3, NOW0 + 3 * DT)
        with pytest.raises(abi.EngineError, match="no kept list of step 3"):
            t.eng.fired_view(3)
        # the engine's last list is a 2-byte one: kwk_emit refuses it exactly as before
        for packed in (True, False):
            with pytest.raises(abi.EngineError, match=r"\(-4\).*kwk_fired_device: kwk_fired_compact in this format"):
                t.em.emit(NOW0 + 7 * DT, packed=packed)
        assert emit_lib_status(t.em, 2) == abi.KWK_EINVAL  # KWK_COMPACT_PACKED16 is no kwk_emit source
        t.eng.step_n(4, NOW0 + 8 * DT, DT, SEED, 8, "bits")
        assert t.eng.fired_view(11)["format"] == abi.COMPACT_BITS
        with pytest.raises(abi.EngineError, match=r"\(-4\).*KWK_COMPACT_BITS"):
            t.em.emit_step(11, NOW0 + 11 * DT)
        with pytest.raises(abi.EngineError, match=r"\(-1\)"):
            t.em.reserve_sets(9, 16, 16)
        with pytest.raises(abi.EngineError, match=r"\(-1\)"):
            t.em.select(1)  # one output set
    finally:
        t.close()


def emit_lib_status(em, source):
    from kwok_amd.host import emit
    return emit.lib().kwk_emit(em.h, NOW0, source)


def test_the_single_set_path_is_unchanged():
    """kwk_emit on the default single set, select(0) in between: what the per-step reference gives."""
    ref = churn_reference()[:4]
    t = Twin("fast", N_FAST, fuse=False, dead=DEAD)
    try:
        for k in range(4):
            t.eng.step(NOW0 + k * DT, SEED, k)
            t.eng.fired_compact(packed=True)
            t.em.select(0)
            same(t.em.run(NOW0 + k * DT, packed=True), ref[k], f"step {k}")
            t.em.select(0)
            assert t.em.result() == (len(ref[k][0]), len(ref[k][2]))
            assert t.em.elapsed_ms() > 0.0
        assert np.array_equal(t.words(), ref[3][3])
    finally:
        t.close()

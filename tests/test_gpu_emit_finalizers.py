"""Finalizer JSON patches written on the GPU (kwk_emit_finalizers_load, include/kwok_emit.h
"Finalizer patches"): for every fired record whose Stage has a finalizers op, the
bytes playStage sends before the object's delete or merge patches (pod_controller.go:304-352,
next.go:43-60, finalizers.go:83-111).

Expected bytes everywhere: json.dumps(oracle.refcpu.finalizers_modify(meta, fin), separators=(",", ":"))
with `meta` the object's metadata.finalizers before the step, from the controller's cache, and no
item for [].  The order words after a step are the words of the controller's updated objects, and
their id sets are the engine's finalizer-group bits.  The merge-patch stream and the guard words of
an emitter with a finalizer program are those of a twin emitter without one."""
import copy
import functools
import json

import numpy as np
import pytest

from kwok_amd import workload as W

pytestmark = pytest.mark.gpu

FAKE = "kwok.x-k8s.io/fake"


def expected(prog, fired, pre):
    """[(rec, status, n_ops, bytes)] of a fired list against the objects before the step."""
    from kwok_amd.host import emit
    from oracle import refcpu
    want = []
    for j, r in enumerate(fired):
        f = prog.stages[int(r["stage"])].next.finalizers
        if f is None:
            continue
        meta = list((pre[int(r["slot"])].get("metadata") or {}).get("finalizers") or [])
        if len(meta) > 7:
            want.append((j, emit.STATUS_HOST, 0, b""))
            continue
        ops = refcpu.finalizers_modify(meta, {"empty": bool(f.empty), "add": [{"value": v} for v in f.add],
                                              "remove": [{"value": v} for v in f.remove]})
        if ops:
            want.append((j, emit.STATUS_OK, len(ops), json.dumps(ops, separators=(",", ":")).encode()))
    return want


def check_stream(got, want, what):
    items, offs, data = got
    assert [(int(i["rec"]), int(i["status"]), int(i["n_ops"])) for i in items] == [w[:3] for w in want], what
    pos = 0
    for n, w in enumerate(want):
        assert int(offs[n]) == pos, (what, n)
        pos += len(w[3])
    assert int(offs[len(want)]) == pos and data == b"".join(w[3] for w in want), what


class Rig:
    """Engine + native controller + two emitters over the same fired lists: `em` with the finalizer
    program, `twin` without (the merge-patch yardstick)."""

    def __init__(self, stages, objs, harness=False, fin_room=None):
        from kwok_amd.host import emit
        from kwok_amd.host.compiler import HarnessSpec, KindProgram
        from kwok_amd.host.controller import KindController
        from kwok_amd.host.encoder import NativeIngest
        from kwok_amd.host.engine import Engine, Ingest
        from tests.test_patch import FUNCS
        self.prog = prog = KindProgram(stages, HarnessSpec() if harness else None)
        prog.explore(objs)
        self.nat = NativeIngest(prog)
        hot, dels, rec, cls = self.nat.columns(objs)
        n = self.n = len(objs)
        self.eng = Engine(prog, capacity=n, max_records=len(self.nat.record_array()) + 64)
        self.ctl = KindController(prog, self.eng, Ingest(prog), objs, funcs=FUNCS, native=True)
        self.fresh = None
        if harness:  # what the harness re-creates: the object from its spec (compiler.py keep mask)
            self.fresh = []
            for o in self.ctl.objs:
                f = copy.deepcopy(o)
                f.pop("status", None)
                for k in ("finalizers", "deletionTimestamp", "deletionGracePeriodSeconds"):
                    f["metadata"].pop(k, None)
                self.fresh.append(f)
        self.classes = [prog.class_of(o, register=False) for o in self.ctl.objs]
        reps = {}
        for o, c in zip(self.ctl.objs, self.classes):
            reps.setdefault(c, o)
        self.ep = emit.EmitProgram(prog.stages, self.ctl.patcher, reps, len(prog.class_ids))
        self.fp = emit.FinProgram(prog.finalizer_spec())
        self.em = emit.Emitter(self.eng, n, self.ep)
        self.twin = emit.Emitter(self.eng, n, self.ep)
        words, cols = self.ep.rows(self.ctl.objs, self.classes)
        for e in (self.em, self.twin):
            e.set_rows(0, words, cols)
        self.em.load_finalizers(self.fp)
        self.em.set_fin_words(0, self.host_words())
        self.em.reserve_fin(*(fin_room or (n + 1, 1024 * n)))
        self.eng.load_stages()
        if harness:
            self.eng.set_harness(True)
        self.eng.load(hot, dels, rec, cls, self.nat.record_array())
        d = prog.describe()
        self.fin_bits, self.other_bit = d["finalizers"], d["finalizer_other_bit"]

    def host_words(self):
        return np.asarray([0 if o is None else self.fp.word((o.get("metadata") or {}).get("finalizers"))
                           for o in self.ctl.objs], dtype=np.uint32)

    def step(self, k, now, seed, source, require16=False, pre=None):
        """One step through `source`; returns the fired list.  Checks the finalizer stream against the
        oracle, the merge-patch stream and guard words against the twin, the order words against
        the controller's objects and the engine's finalizer bits."""
        from kwok_amd.host import abi, emit
        what = f"step {k} {source}"
        if source != "ring16":
            self.eng.step(now, seed, k)
        if source == "ring16":  # kwk_step_n's 2-byte ring list, emitted from its slot
            self.eng.step_n(1, now, 10**9, seed, k, "packed16")
            assert self.eng.fired_view(k)["format"] == abi.COMPACT_PACKED16 and self.eng.stats()["state_bytes"] == 1
            merge = self.em.run_step(k, now)
            fin = self.em.collect_fin()
            tw = self.twin.run_step(k, now)
        elif source == "packed16":
            self.eng.fired_compact(packed="16")
            # (an engine whose state is wider than one byte has no 2-byte records: its list stays 4-byte)
            assert not require16 or self.eng.fired_view()["format"] == abi.COMPACT_PACKED16
            merge = self.em.run_step(abi.STEP_LAST, now)
            fin = self.em.collect_fin()
            tw = self.twin.run_step(abi.STEP_LAST, now)
        else:
            self.eng.fired_compact(packed=source == "packed")
            if pre is not None:
                pre(self, now)
            merge = self.em.run(now, packed=source == "packed")
            fin = self.em.collect_fin()
            tw = self.twin.run(now, packed=source == "packed")
        for f in ("rec", "tid", "status"):
            assert np.array_equal(merge[0][f], tw[0][f]), (what, f)
        assert np.array_equal(merge[1], tw[1]) and merge[2] == tw[2], what
        assert np.array_equal(self.em.words(0, self.n), self.twin.words(0, self.n)), what
        self.eng.fired_compact(packed=False)
        fired = self.eng.fired()
        pre = {int(r["slot"]): self.ctl.objs[int(r["slot"])] for r in fired}
        want = expected(self.prog, fired, pre)
        check_stream(fin, want, what)
        self.ctl.handle(fired, now)
        for j, st, _, b in want:  # the controller's native path sent the same bytes
            if st == emit.STATUS_OK:
                assert self.ctl.last_fin_patches[int(fired[j]["slot"])] == b, what
        ok = {int(fired[j]["slot"]) for j, st, _, _ in want if st == emit.STATUS_OK}
        over = {int(fired[j]["slot"]) for j, st, _, _ in want if st == emit.STATUS_HOST}
        assert set(self.ctl.last_fin_patches) - over == ok, what  # no item: the reference sends nothing
        if self.fresh is not None:  # churn: the harness re-created what was deleted
            for r in fired:
                if self.ctl.objs[int(r["slot"])] is None:
                    self.ctl.objs[int(r["slot"])] = copy.deepcopy(self.fresh[int(r["slot"])])
        host = [int(fired[j]["slot"]) for j, st, _, _ in want if st == emit.STATUS_HOST]
        hw = self.host_words()
        for s in host:  # the host rendered these: it sets their words, as it does the guard words
            self.em.set_fin_words(s, hw[s:s + 1])
        dev = self.em.fin_words(0, self.n)
        assert np.array_equal(dev, hw), (what, np.flatnonzero(dev != hw)[:8])
        # the id set of every word is the engine's finalizer group
        pred = self.eng.read()[0]["pred"]
        group = sum(1 << b for b in self.fin_bits.values()) | (0 if self.other_bit is None else 1 << self.other_bit)
        bit_of = [self.fin_bits[v] for v in self.fp.values]
        for s, o in enumerate(self.ctl.objs):
            ids = emit.fin_word_ids(int(dev[s]))
            if o is None or ids is None:
                continue
            # (a set with no finalizers op has no dictionary and no group: every value is "other", no bit)
            bits = sum({1 << (self.other_bit if i == emit.FIN_OTHER else bit_of[i]) for i in ids
                        if i != emit.FIN_OTHER or self.other_bit is not None})
            assert int(pred[s]) & group == bits, (what, s, ids)
        return fired, want

    def close(self):
        self.em.close()
        self.twin.close()
        self.ctl.close()
        self.nat.close()
        self.eng.close()


# ---- 1, 2: the synthetic set
LISTS = [None, ["a"], ["x"], ["x", "a", "y"], ["a", "b", "c"], ["a", "a"], ["a", "x", "b", "y", "c", "x", "a"],
         ["a", "b", "c", "x", "y", "a", "b", "c"]]
NEXTS = [{"finalizers": {"add": [{"value": "a"}, {"value": "b"}]}},
         {"finalizers": {"remove": [{"value": "a"}]}},
         {"finalizers": {"remove": [{"value": "a"}, {"value": "c"}]}},
         {"finalizers": {"empty": True}},
         {"finalizers": {"empty": True, "add": [{"value": "b"}]}},
         {"finalizers": {"empty": True}, "delete": True},
         {"statusTemplate": "phase: Running\nreason: '{{ Now }}'\n"}]


# The 2-byte lists come from the engine's 1-byte sweep only: at most four stages, and the words
# reachable from the loaded rows (4 dictionary bits x flags x scheduled stage) within 255 ids.  The
# seven stages over the eight lists close that far in these groups (larger ones do not: the engine
# then keeps 2-byte words and hands 4-byte lists back)
HALVES = {"add": (0,), "remove-a": (1,), "remove-ac+empty": (2, 3), "empty-add+patch": (4, 6), "delete+patch": (5, 6)}


@functools.lru_cache(maxsize=None)
def synthetic_stages():
    from kwok_amd.host.stages import stage_from_v1alpha1
    return tuple(stage_from_v1alpha1({
        "apiVersion": "kwok.x-k8s.io/v1alpha1", "kind": "Stage", "metadata": {"name": f"s{i}"},
        "spec": {"resourceRef": {"apiGroup": "v1", "kind": "Pod"},
                 "selector": {"matchExpressions": [{"key": ".metadata.labels.k", "operator": "In", "values": [f"s{i}"]}] +
                              ([{"key": ".status.phase", "operator": "DoesNotExist"}] if "statusTemplate" in nx else [])},
                 "next": nx}}) for i, nx in enumerate(NEXTS))


def synthetic_objects(n, which=tuple(range(len(NEXTS)))):
    objs = []
    for i in range(n):
        md = {"name": f"p{i}", "namespace": "d", "uid": f"u{i}", "labels": {"k": f"s{which[i % len(which)]}"}}
        fins = LISTS[(i // len(which)) % len(LISTS)]
        if fins is not None:
            md["finalizers"] = list(fins)
        objs.append({"apiVersion": "v1", "kind": "Pod", "metadata": md,
                     "spec": {"nodeName": f"n{i % 5}", "containers": [{"name": "c", "image": "i"}]}})
    return objs


@pytest.mark.parametrize("source", ["rec", "packed"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 600])
def test_synthetic_set_every_list_and_size(n, source):
    from kwok_amd.host import emit
    from tests.parity_util import NOW0
    rig = Rig(list(synthetic_stages()), synthetic_objects(n))
    try:
        total = host = 0
        for k in range(3):
            fired, want = rig.step(k, NOW0 + k * 10**9, 0x51, source)
            if k == 0:
                assert len(fired) == n  # every object fires in one step: the list has exactly n records
            total += len(want)
            host += sum(1 for w in want if w[1] == emit.STATUS_HOST)
        if n >= 600:
            assert total >= 300 and host >= 8, (total, host)  # the eight-entry lists came back for the host
    finally:
        rig.close()


@pytest.mark.parametrize("half", sorted(HALVES))
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 600])
def test_synthetic_set_two_byte_lists(n, half):
    """The same stages and lists through KWK_COMPACT_PACKED16: the engine hands 2-byte records back
    only from its 1-byte sweep, so the seven stages run in the groups that sweep allows
    (kwk_step_n(..., KWK_COMPACT_PACKED16) + kwk_emit_step of the ring slot, the format asserted)."""
    from kwok_amd.host import emit
    from tests.parity_util import NOW0
    which = HALVES[half]
    rig = Rig([synthetic_stages()[i] for i in which], synthetic_objects(n, which))
    try:
        rig.eng.fired_keep(4)
        total = host = 0
        for k in range(3):
            fired, want = rig.step(k, NOW0 + k * 10**9, 0x51, "ring16")
            if k == 0:
                assert len(fired) == n
            total += len(want)
            host += sum(1 for w in want if w[1] == emit.STATUS_HOST)
        if n >= 600:
            # at least half of a group's objects sit on a finalizer stage, and step 0 alone gives at
            # least four of the eight lists an item on each of them (the eight-entry list: the host's)
            assert total >= n // 4 and host >= 8, (total, host)
    finally:
        rig.close()


def test_a_set_without_finalizer_ops_has_an_empty_stream():
    """No stage has KWK_NEXT_FIN: the program loads, the finalizer launches are skipped, every
    emission's finalizer stream is empty and the merge patches are the twin's."""
    from tests.parity_util import NOW0
    objs = [o for o in synthetic_objects(300)]
    for o in objs:
        o["metadata"].pop("finalizers", None)
    rig = Rig([synthetic_stages()[6]], objs)
    try:
        assert rig.fp.values == [] and not any(st["flags"] & 8 for st in rig.fp.stages)
        fired, want = rig.step(0, NOW0, 0x52, "packed")
        assert len(fired) > 0 and want == []
        assert rig.em.fin_result() == (0, 0, 0)
    finally:
        rig.close()


def test_one_set_finalizer_overflow_stops_the_merge_writer():
    """One output set, the finalizer stream without room: the emission reads KWK_ECAP with the
    finalizer totals, neither stream is written, the guard and the order words stay; with room
    the same list emits exactly."""
    from kwok_amd.host import abi
    from tests import test_gpu_emit_ring as R
    from tests.parity_util import NOW0
    n = 300
    rig = Rig(list(synthetic_stages()), synthetic_objects(n), fin_room=(n + 1, 16))
    seen = []

    def pre(rig, now):
        rig.em.reserve(16 * n, 4096 * n)  # the merge patches have room
        w0, f0 = rig.em.words(0, n), rig.em.fin_words(0, n)
        rig.em.emit(now, packed=True)
        assert R.emit_result_status(rig.em) == abi.KWK_ECAP
        assert "kwk_emit_reserve_fin" in emit_error(rig.em)
        st, fi, fb = rig.em.fin_result()
        assert st == abi.KWK_ECAP and fi > 0 and fb > 16
        assert np.array_equal(rig.em.words(0, n), w0) and np.array_equal(rig.em.fin_words(0, n), f0)
        rig.em.reserve_fin(fi, fb)  # exactly what it asked for
        seen.append((fi, fb))

    try:
        fired, want = rig.step(0, NOW0, 0x53, "packed", pre=pre)
        assert seen == [(len(want), sum(len(w[3]) for w in want))]
    finally:
        rig.close()


def emit_error(em):
    from kwok_amd.host import emit
    return emit.lib().kwk_emit_last_error(em.h).decode()


# ---- 3: the shipped sets, with churn
def shipped(mix, nodes, pods, steps, seed, dt_ns, seed_fake, sources):
    from kwok_amd.host import emit
    from kwok_amd.host.stages import load_stage_files
    from tests.parity_util import NOW0
    cl = W.make_cluster(mix, nodes, pods, seed=seed)
    objs = cl.pods.materialize()
    if seed_fake:
        for o in objs[::2]:
            o["metadata"]["finalizers"] = [FAKE]
    rig = Rig(load_stage_files(*cl.pod_stage_files), objs, harness=True)
    try:
        n_items = n_recreated = 0
        for k in range(steps):
            fired, want = rig.step(k, NOW0 + k * dt_ns, seed, sources[k % len(sources)], require16=True)
            n_items += sum(1 for w in want if w[1] == emit.STATUS_OK)
            n_recreated += sum(1 for r in fired if rig.prog.stages[int(r["stage"])].next.delete)
        return n_items, n_recreated
    finally:
        rig.close()


def test_pod_general_with_churn():
    items, recreated = shipped("C2", 30, 400, 30, 0x91, 500 * 10**6, False, ("rec", "packed"))
    assert items >= 400, (items, recreated)  # pod-create adds the finalizer of every pod


def test_pod_fast_with_churn():
    items, recreated = shipped("C1", 20, 300, 8, 0x92, 10**9, True, ("packed16", "rec", "packed"))
    assert items >= 1 and recreated >= 1, (items, recreated)


# ---- 4, 5: the ring and the overflow protocol, against the per-step twin
def ring_twin(fuse, harness=True, dead=True):
    """tests/test_gpu_emit_ring.py's pod-fast twin with the shipped set's finalizer program and
    order words that give pod-delete something to remove."""
    from kwok_amd.host import emit
    from tests import test_gpu_emit_ring as R
    t = R.Twin("fast", R.N_FAST, fuse=fuse, harness=harness, dead=R.DEAD if dead else None)
    try:
        fp = emit.FinProgram(t.eng.p.finalizer_spec())
        t.em.load_finalizers(fp)
        t.em.set_fin_words(0, ring_words(fp))
    except Exception:
        t.close()
        raise
    return t


def ring_words(fp):
    from tests import test_gpu_emit_ring as R
    w = np.zeros(R.N_FAST, dtype=np.uint32)
    w[0::2] = fp.word([FAKE])
    w[1::4] = fp.word(["example.com/other", FAKE])
    return w


RESET = (4, 8)  # the overflow runs: the host sets every order word again at these group boundaries


@functools.lru_cache(maxsize=None)
def ring_reference(steps, harness=True, dead=True, reset=()):
    """Per step of the unfused twin: (merge stream, finalizer stream, guard words, order words)."""
    from tests import test_gpu_emit_ring as R
    t = ring_twin(False, harness, dead)
    try:
        t.em.reserve_fin(R.N_FAST + 1, 256 * R.N_FAST)
        out = []
        for k in range(steps):
            if k in reset:
                t.em.set_fin_words(0, ring_words(t.em.fin_program))
            t.eng.step(R.NOW0 + k * R.DT, R.SEED, k)
            t.eng.fired_compact(packed=True)
            merge = t.em.run(R.NOW0 + k * R.DT, packed=True)
            out.append((merge, t.em.collect_fin(), t.words(), t.em.fin_words(0, R.N_FAST)))
        return out
    finally:
        t.close()


def same_fin(got, want, what):
    for f in ("rec", "status", "n_ops"):
        assert np.array_equal(got[0][f], want[0][f]), (what, f)
    assert np.array_equal(got[1], want[1]) and got[2] == want[2], what


def fin_room(ref):
    return max(len(r[1][0]) for r in ref) + 1, max(len(r[1][2]) for r in ref) + 1


def test_ring_two_fused_groups_into_eight_sets():
    from kwok_amd.host import abi
    from tests import test_gpu_emit_ring as R
    ref = ring_reference(8)
    assert sum(len(r[1][0]) for r in ref) > 0
    t = ring_twin(True)
    try:
        t.eng.fired_keep(8)
        t.em.reserve_sets(8, *R.room([r[0] for r in ref]))
        t.em.reserve_fin(*fin_room(ref))
        for g in (0, 4):
            t.eng.step_n(4, R.NOW0 + g * R.DT, R.DT, R.SEED, g, "packed16")
            assert t.eng.last_sweep()["steps"] == 4
        hole = False
        for k in range(8):
            assert t.eng.fired_view(k)["format"] == abi.COMPACT_PACKED16
            c, cnt = R.seg_counts(t.eng, k)
            nz = np.flatnonzero(c)
            hole = hole or (cnt > 0 and bool(np.any(c[nz[0]:nz[-1] + 1] == 0)))
        assert hole  # a list with an empty segment between live ones
        for k in range(8):
            t.em.emit_step(k, R.NOW0 + k * R.DT)
        for k in range(8):
            t.em.select(7 - k)
            R.same(t.em.collect(), ref[k][0], f"step {k}")
            same_fin(t.em.collect_fin(), ref[k][1], f"step {k}")
        assert np.array_equal(t.words(), ref[7][2])
        assert np.array_equal(t.em.fin_words(0, R.N_FAST), ref[7][3])
    finally:
        t.close()


def test_ring_a_step_that_fires_nothing():
    from tests import test_gpu_emit_ring as R
    ref = ring_reference(8, False, False)
    assert 0 in [len(r[0][0]) for r in ref]
    t = ring_twin(True, harness=False, dead=False)
    try:
        t.eng.fired_keep(8)
        t.em.reserve_sets(8, *R.room([r[0] for r in ref]))
        t.em.reserve_fin(*fin_room(ref))
        t.eng.step_n(8, R.NOW0, R.DT, R.SEED, 0, "packed16")
        for k in range(8):
            t.em.emit_step(k, R.NOW0 + k * R.DT)
        for k in range(8):
            t.em.select(7 - k)
            R.same(t.em.collect(), ref[k][0], f"step {k}")
            same_fin(t.em.collect_fin(), ref[k][1], f"step {k}")
        assert np.array_equal(t.em.fin_words(0, R.N_FAST), ref[7][3])
    finally:
        t.close()


@pytest.mark.parametrize("short", ["finalizers", "merge"])
def test_overflow_with_emissions_in_flight(short):
    """Four emissions of a fused group in flight, the second without room — one byte short in its
    finalizer stream, or short in its merge patches: it and the two behind it read KWK_ECAP, both
    word arrays are those after the first, and re-emitted with room the three are exact.  (pod-fast
    adds no finalizer, so the host gives the pods theirs again at the group boundaries RESET: every
    group has deletes with something to remove.)"""
    from kwok_amd.host import abi
    from tests import test_gpu_emit_ring as R
    ref = ring_reference(12, True, True, RESET)
    mi, mb = [len(r[0][0]) for r in ref], [len(r[0][2]) for r in ref]
    fb = [len(r[1][2]) for r in ref]
    # a fused group whose second step needs more than its first (the reference's own counts)
    if short == "finalizers":
        groups = [g for g in (0, 4, 8) if fb[g + 1] > fb[g]]
    else:
        groups = [g for g in (0, 4, 8) if mb[g + 1] > mb[g]]
    assert groups, (mb, fb)
    g = groups[0]
    t = ring_twin(True)
    try:
        t.eng.fired_keep(8)
        t.em.reserve_sets(8, *R.room([r[0] for r in ref]))
        t.em.reserve_fin(*fin_room(ref))
        for g0 in range(0, g, 4):  # the groups before it, emitted as usual
            if g0 in RESET:
                t.em.set_fin_words(0, ring_words(t.em.fin_program))
            t.eng.step_n(4, R.NOW0 + g0 * R.DT, R.DT, R.SEED, g0, "packed16")
            for k in range(g0, g0 + 4):
                t.em.emit_step(k, R.NOW0 + k * R.DT)
            t.em.select(0)
            assert t.em.result() == (mi[g0 + 3], mb[g0 + 3])
        if short == "finalizers":
            t.em.reserve_fin(fin_room(ref)[0], fb[g + 1] - 1)
            t.em.reserve_sets(4, *R.room([r[0] for r in ref]))  # another number of sets: fresh ones
        else:
            t.em.reserve_sets(4, R.room([r[0] for r in ref])[0], mb[g + 1] - 1)
        if g in RESET:
            t.em.set_fin_words(0, ring_words(t.em.fin_program))
        t.eng.step_n(4, R.NOW0 + g * R.DT, R.DT, R.SEED, g, "packed16")
        for k in range(g, g + 4):
            t.em.emit_step(k, R.NOW0 + k * R.DT)
        t.em.select(3)
        R.same(t.em.collect(), ref[g][0], f"step {g}")
        same_fin(t.em.collect_fin(), ref[g][1], f"step {g}")
        for k in (g + 1, g + 2, g + 3):
            t.em.select(g + 3 - k)
            assert R.emit_result_status(t.em) == abi.KWK_ECAP, k
            assert t.em.fin_result()[0] == abi.KWK_ECAP, k
        assert np.array_equal(t.words(), ref[g][2])
        assert np.array_equal(t.em.fin_words(0, R.N_FAST), ref[g][3])
        t.em.reserve_fin(*fin_room(ref))
        t.em.reserve_sets(4, *R.room([r[0] for r in ref]))
        for k in (g + 1, g + 2, g + 3):
            t.em.emit_step(k, R.NOW0 + k * R.DT)
        for k in (g + 1, g + 2, g + 3):
            t.em.select(g + 3 - k)
            R.same(t.em.collect(), ref[k][0], f"step {k} again")
            same_fin(t.em.collect_fin(), ref[k][1], f"step {k} again")
        assert np.array_equal(t.words(), ref[g + 3][2])
        assert np.array_equal(t.em.fin_words(0, R.N_FAST), ref[g + 3][3])
    finally:
        t.close()

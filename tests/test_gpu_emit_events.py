"""The Events of fired Stages written on the GPU (kwk_evt_load, include/kwok_events.h; DESIGN.md §5
"Events"): for every fired record whose Stage records an Event, the body playStage hands the
recorder first, before the finalizer patch and the delete or merge patches.

Expected bytes everywhere: tests/event_ref.py (client-go's generateEvent / makeEvent over an
encoding/json struct marshaller) for the object of the record's slot; KWK_EMIT_HOST and no bytes
exactly for the rows the test made unusable and the slots beyond the emitter's capacity.  The
merge-patch and finalizer streams of an emitter with an event program are those of a twin
without one."""
import copy
import functools
import json

import numpy as np
import pytest

from tests import event_ref

pytestmark = pytest.mark.gpu

LENGTHS = [1, 3, 4, 5, 16, 63, 253]  # row text lengths: every dword phase, bodies that straddle the LDS window
EVENTS = [{"type": "Normal", "reason": "Created", "message": "Created container"}, None,
          {"type": "Warning", "reason": "Backoff", "message": ""},
          {"type": "Normal", "reason": "Killing", "message": "Stopping container"}]
STRIDES = (256, 64, 256)
BAD_EVERY = 17


def text(n, salt):
    alphabet = "abcdefghijklmnopqrstuvwxyz0123456789-."
    return "".join(alphabet[(salt * 7 + j * 11) % len(alphabet)] for j in range(n))


def make_objects(n, kind, api_version, namespaced=True, n_stages=4, override=None):
    """Objects whose name / namespace / uid lengths cycle through LENGTHS (out of phase with each
    other; namespaces of at most 63 bytes, every 5th object without a uid); every 17th has a name
    that needs escaping, so the host marks its row unusable."""
    objs = []
    for i in range(n):
        md = {"name": text(LENGTHS[i % 7], i), "labels": {"k": f"s{i % n_stages}"}}
        if i % BAD_EVERY == BAD_EVERY - 1:
            md["name"] = "a<" + md["name"][:20]
        if namespaced:
            md["namespace"] = text(min(63, LENGTHS[(i // 7 + 2) % 7]), i + 3)
        if i % 5 != 4:
            md["uid"] = text(LENGTHS[(i // 3 + 4) % 7], i + 5)
        if override and i in override:  # this slot's identity, given
            md = dict(override[i], labels=md["labels"])
        o = {"apiVersion": api_version, "kind": kind, "metadata": md}
        if kind == "Pod":
            o["spec"] = {"nodeName": f"n{i % 5}", "containers": [{"name": "c", "image": "i"}]}
        objs.append(o)
    return objs


@functools.lru_cache(maxsize=None)
def synthetic_stages(kind, group, events_json):
    """Four table-only stages (no patch: the engine's 1-byte sweep hands 2-byte lists back): an
    event, no event, an event with an empty message, a delete with an event."""
    from kwok_amd.host.stages import stage_from_v1alpha1
    out = []
    for i, ev in enumerate(json.loads(events_json)):
        nx = {} if ev is None else {"event": dict(ev)}
        if i == 3:
            nx["delete"] = True
        out.append(stage_from_v1alpha1({
            "apiVersion": "kwok.x-k8s.io/v1alpha1", "kind": "Stage", "metadata": {"name": f"s{i}"},
            "spec": {"resourceRef": {"apiGroup": group, "kind": kind},
                     "selector": {"matchExpressions": [{"key": ".metadata.labels.k", "operator": "In", "values": [f"s{i}"]}]},
                     "next": nx}}))
    return tuple(out)


def expected(kind, spec, objs, fired, now, cap, usable):
    """[(rec, status, bytes)] of a fired list: an item per record of an event stage."""
    from kwok_amd.host import emit
    want = []
    for j, r in enumerate(fired):
        ev = spec["stages"][int(r["stage"])]
        if ev is None:
            continue
        s = int(r["slot"])
        if s >= cap or not usable[s]:
            want.append((j, emit.STATUS_HOST, b""))
        else:
            want.append((j, emit.STATUS_OK, event_ref.event_for(kind, objs[s], ev, now)))
    return want


def check_stream(got, want, what):
    items, offs, data = got
    assert [(int(i["rec"]), int(i["status"])) for i in items] == [w[:2] for w in want], what
    assert not items["reserved"].any(), what
    pos = 0
    for n, w in enumerate(want):
        assert int(offs[n]) == pos, (what, n)
        assert data[pos:pos + len(w[2])] == w[2], (what, n)
        pos += len(w[2])
    assert int(offs[len(want)]) == pos and len(data) == pos, what


def row_usable(prog_av, o):
    md = o["metadata"]
    ok = prog_av == "" or o["apiVersion"] == prog_av
    return ok and bool(md.get("name")) and all(all(0x21 <= ord(c) <= 0x7E and c not in '"\\<>&' for c in md.get(k, "")) for k in ("name", "namespace", "uid"))


class Synth:
    """Engine + one emitter with the event program over the synthetic set, n records per full step.
    For n > 1 the engine holds n + 1 objects and the emitter's capacity is n: the last slot (on
    stage 0) is beyond it, so its record comes back for the host, and slot 1 matches no stage, so a
    step's list has n records (a list may not be longer than the emitter's capacity rounded up to
    a tile)."""

    def __init__(self, n, kind="Pod", group="v1", namespaced=True, stage_events=EVENTS, override=None):
        from kwok_amd.host import emit, events
        from kwok_amd.host.compiler import KindProgram
        from kwok_amd.host.encoder import NativeIngest
        from kwok_amd.host.engine import Engine
        from kwok_amd.host.patchtpl import PatchProgram
        self.kind, self.n = kind, n
        m = n + 1 if n > 1 else 1
        self.objs = make_objects(m, kind, group if "/" in group else "v1", namespaced, override=override)
        if n > 1:
            self.objs[1]["metadata"]["labels"]["k"] = "none"
            self.objs[m - 1]["metadata"]["labels"]["k"] = "s0"
        self.prog = prog = KindProgram(list(synthetic_stages(kind, group, json.dumps(stage_events))))
        prog.explore(self.objs)
        self.spec = json.loads(prog.event_spec(device=True))
        self.nat = NativeIngest(prog)
        hot, dels, rec, cls = self.nat.columns(self.objs)
        self.eng = Engine(prog, capacity=m, max_records=len(self.nat.record_array()) + 64)
        self.pp = PatchProgram(prog.stages, {})
        classes = [prog.class_of(o, register=False) for o in self.objs]
        reps = {}
        for o, c in zip(self.objs, classes):
            reps.setdefault(c, o)
        self.ep = emit.EmitProgram(prog.stages, self.pp, reps, len(prog.class_ids))
        self.cap = n
        self.em = emit.Emitter(self.eng, self.cap, self.ep)
        words, cols = self.ep.rows(self.objs[:self.cap], classes[:self.cap])
        self.em.set_rows(0, words, cols)
        self.evp = events.EventProgram(self.spec, STRIDES if namespaced else (STRIDES[0], 0, STRIDES[2]))
        self.em.load_events(self.evp)
        self.em.set_event_rows(0, self.evp.rows(self.objs[:self.cap]))
        self.em.reserve_events(m, 1400 * m)
        self.usable = [row_usable(self.spec["api_version"], o) for o in self.objs]
        self.eng.load_stages()
        self.eng.load(hot, dels, rec, cls, self.nat.record_array())
        self.eng.fired_keep(4)

    def step(self, k, now, seed, source):
        """One step through `source`, its event stream checked -> (fired list, expected items)."""
        from kwok_amd.host import abi
        what = f"n={self.n} step {k} {source}"
        if source == "packed16":
            self.eng.step_n(1, now, 10**9, seed, k, "packed16")
            assert self.eng.fired_view(k)["format"] == abi.COMPACT_PACKED16 and self.eng.stats()["state_bytes"] == 1
            self.em.run_step(k, now)
        else:
            self.eng.step(now, seed, k)
            self.eng.fired_compact(packed=source == "packed")
            fmt = self.eng.fired_view()["format"]
            assert fmt == (abi.COMPACT_PACKED if source == "packed" else abi.COMPACT_REC), what
            self.em.run(now, packed=source == "packed")
        got = self.em.collect_events()
        self.eng.fired_compact(packed=False)
        fired = self.eng.fired()
        want = expected(self.kind, self.spec, self.objs, fired, now, self.cap, self.usable)
        check_stream(got, want, what)
        return fired, want

    def close(self):
        self.em.close()
        self.pp.close()
        self.nat.close()
        self.eng.close()


VEC_NOW = 1700000000123456789


@pytest.mark.parametrize("source", ["rec", "packed", "packed16"])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 600])
def test_synthetic_set_every_size_and_source(n, source):
    from kwok_amd.host import emit
    s = Synth(n)
    try:
        fired, want = s.step(0, VEC_NOW, 0x51, source)
        assert len(fired) == n  # every object fires in step 0: the list has exactly n records
        # an item for each record of the three event stages; exactly the unusable rows and the slot
        # beyond the capacity are the host's
        slots = [int(r["slot"]) for r in fired if int(r["stage"]) != 1]
        assert len(want) == len(slots) and len(slots) >= (3 * n) // 4
        host = {int(fired[j]["slot"]) for j, st, _ in want if st == emit.STATUS_HOST}
        bad = {i for i in slots if i % BAD_EVERY == BAD_EVERY - 1 or i >= s.cap}
        assert host == bad, (host, bad)
        assert n == 1 or n in host  # the slot beyond the capacity fired
        assert all(len(b) > 350 for _, st, b in want if st == emit.STATUS_OK)  # (the fixed text alone)
        if n >= 255:
            assert len(bad) >= 10 and max(len(b) for _, _, b in want) > 1000, (len(bad), max(len(b) for _, _, b in want))
        st, ni, nb, launched = s.em.event_result()
        assert (st, ni, nb, launched) == (0, len(want), sum(len(b) for _, _, b in want), 1)
        fired1, want1 = s.step(1, VEC_NOW + 10**9, 0x51, source)  # nothing changed: nothing fires
        assert len(want1) <= len(want)
    finally:
        s.close()


def test_reference_vectors_from_the_device():
    """The three vectors of tests/golden/event_vectors.json, byte for byte, out of the device stream."""
    import os
    from kwok_amd.host import emit
    vecs = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "event_vectors.json")))["vectors"][:3]
    assert [v["kind"] for v in vecs] == ["Pod", "Node", "Widget"]
    for vec in vecs:
        s = Synth(8, vec["kind"], vec["api_version"] or "v1", namespaced=vec["kind"] != "Node",
                  stage_events=[vec["event"]] + EVENTS[1:], override={0: vec["object"]["metadata"], 4: vec["object"]["metadata"]})
        try:
            assert s.usable[0] and s.usable[4]
            fired, want = s.step(0, vec["now_ns"], 1, "packed")
            bodies = {int(fired[j]["slot"]): b for j, st, b in want if st == emit.STATUS_OK}
            assert bodies[0] == vec["body"].encode() == bodies[4], vec["name"]  # (the stream equals `want`: s.step)
        finally:
            s.close()


def test_an_empty_name_is_the_hosts():
    """ObjectReference.Name is omitempty: a record whose name row has length 0 comes back for the
    host, whose renderer leaves the key out as the reference does."""
    from kwok_amd.host import emit
    from kwok_amd.host.patchtpl import PatchProgram
    s = Synth(8, override={0: {"namespace": "d", "uid": "u0"}, 4: {"name": "", "uid": "u4"}})
    try:
        assert not s.usable[0] and not s.usable[4] and s.evp.rows(s.objs[:1])[0][0, 0] == 0
        fired, want = s.step(0, VEC_NOW, 0x54, "packed")
        host = {int(fired[j]["slot"]) for j, st, _ in want if st == emit.STATUS_HOST}
        assert {0, 4} <= host
        pp = PatchProgram([], {}, events=json.dumps(s.spec))
        try:
            b = pp.event(0, "d", "", "u0", "", VEC_NOW)
        finally:
            pp.close()
        assert b == event_ref.event_for("Pod", s.objs[0], s.spec["stages"][0], VEC_NOW) and b'"name":""' not in b
    finally:
        s.close()


@pytest.mark.parametrize("n", [65, 257])
@pytest.mark.parametrize("which", ["cluster-scoped", "generic"])
def test_cluster_scoped_and_generic_kinds(which, n):
    from kwok_amd.host import emit
    s = Synth(n, "Node", "v1", namespaced=False) if which == "cluster-scoped" else Synth(n, "Widget", "example.com/v1")
    try:
        assert s.spec["api_version"] == ("" if which == "cluster-scoped" else "example.com/v1")
        for source in ("packed16", "rec"):
            fired, want = s.step(0 if source == "packed16" else 1, VEC_NOW + 999, 0x52, source)
            if source == "packed16":
                assert len(fired) == n
                ok = [b for _, st, b in want if st == emit.STATUS_OK]
                assert len(ok) >= n // 2
                if which == "generic":
                    assert all(b'"apiVersion":"example.com/v1"},' in b and b'"kind":"Widget","namespace":"' in b for b in ok)
                else:
                    assert all(b'"involvedObject":{"kind":"Node","name":"' in b and b'"namespace":"default"' in b for b in ok)
    finally:
        s.close()


def test_generic_kind_rows_of_another_api_version_are_the_hosts():
    from kwok_amd.host import emit
    s = Synth(40, "Widget", "example.com/v1")
    try:
        for i in (0, 2, 6):
            s.objs[i] = dict(s.objs[i], apiVersion="example.com/v2")
            s.usable[i] = False
        s.em.set_event_rows(0, s.evp.rows(s.objs[:s.cap]))
        fired, want = s.step(0, VEC_NOW, 0x53, "packed")
        host = {int(fired[j]["slot"]) for j, st, _ in want if st == emit.STATUS_HOST}
        assert {0, 2, 6} <= host
    finally:
        s.close()


# ---- the shipped sets: events beside the merge-patch and finalizer streams, against the twin
def event_rows_for(rig, prog):
    return prog.rows([o for o in rig.ctl.objs])


def test_pod_general_with_churn():
    """pod-general with churn, at tests/test_gpu_emit_finalizers.py::test_pod_general_with_churn's
    size: the event stream equals the reference every step; the merge-patch stream, the finalizer
    stream and both word arrays are checked by that module's rig against its twin without an event
    program and against the oracle."""
    from kwok_amd import workload as W
    from kwok_amd.host import emit, events
    from kwok_amd.host.stages import load_stage_files
    from tests import test_gpu_emit_finalizers as FT
    from tests.parity_util import NOW0
    cl = W.make_cluster("C2", 30, 400, seed=0x91)
    objs = cl.pods.materialize()
    rig = FT.Rig(load_stage_files(*cl.pod_stage_files), objs, harness=True)
    try:
        spec = json.loads(rig.prog.event_spec(device=True))
        evp = events.EventProgram(spec, (64, 64, 40))
        rig.em.load_events(evp)
        rig.em.set_event_rows(0, evp.rows(rig.ctl.objs))
        rig.em.reserve_events(len(objs) + 1, 640 * len(objs))
        n_ok = 0
        reasons = set()
        for k in range(12):
            now = NOW0 + k * 500 * 10**6
            pre = copy.deepcopy(rig.ctl.objs)
            fired, _ = rig.step(k, now, 0x91, ("rec", "packed")[k % 2])
            got = rig.em.collect_events()  # (the rig's last emission of `em`: the twin is another emitter)
            want = expected("Pod", spec, pre, fired, now, len(objs), [True] * len(objs))
            check_stream(got, want, f"step {k}")
            for j, st, b in want:
                assert st == emit.STATUS_OK
                assert rig.ctl.last_events[int(fired[j]["slot"])] == b  # what the native controller recorded
                reasons.add(json.loads(b)["reason"])
            n_ok += len(want)
        # (every item above is one the reference derives from the fired list; this only keeps the
        # run from being vacuous: pod-create fires within the twelve steps for most of the 400 pods)
        assert n_ok >= 100 and "Created" in reasons, (n_ok, reasons)
    finally:
        rig.close()


def test_pod_fast_has_no_event_and_no_launch():
    from kwok_amd import workload as W
    from kwok_amd.host import events
    from kwok_amd.host.stages import load_stage_files
    from tests import test_gpu_emit_finalizers as FT
    from tests.parity_util import NOW0
    cl = W.make_cluster("C1", 20, 300, seed=0x92)
    objs = cl.pods.materialize()
    rig = FT.Rig(load_stage_files(*cl.pod_stage_files), objs, harness=True)
    try:
        spec = json.loads(rig.prog.event_spec(device=True))
        assert not any(spec["stages"])
        evp = events.EventProgram(spec, (64, 64, 40))
        assert not evp.any_event
        rig.em.load_events(evp)
        rig.em.set_event_rows(0, evp.rows(rig.ctl.objs))
        for k in range(3):
            fired, _ = rig.step(k, NOW0 + k * 10**9, 0x92, ("packed16", "rec", "packed")[k], require16=True)
            assert len(fired) > 0
            assert rig.em.event_result() == (0, 0, 0, 0)  # an empty stream; launched = 0: no event kernel ran
            items, offs, data = rig.em.collect_events()
            assert len(items) == 0 and list(offs) == [0] and data == b""
    finally:
        rig.close()


# ---- the ring and the overflow protocol: the pod-fast twin of tests/test_gpu_emit_ring.py with an
# event program of its own (the stream needs no event in the Stage set: it is given a program)
RING_EVENTS = [{"type": "Normal", "reason": "Started", "message": "Started container"},
               {"type": "Normal", "reason": "Completed", "message": ""},
               {"type": "Warning", "reason": "Killing", "message": "Stopping container"}]
RING_STRIDES = (16, 8, 40)


def ring_identity(i):
    return {"apiVersion": "v1", "kind": "Pod",
            "metadata": {"name": "pod-%d" % i, "namespace": "ns%d" % (i % 7) if i % 3 else "", "uid": "%032x" % (i * 2654435761)}}


def ring_spec(t):
    return {"kind": "Pod", "api_version": "", "component": "kwok_controller",
            "stages": [RING_EVENTS[i % 3] for i in range(len(t.eng.p.stages))]}


def ring_twin(fuse, harness=True, dead=True):
    from kwok_amd.host import emit, events
    from tests import test_gpu_emit_finalizers as FT
    from tests import test_gpu_emit_ring as R
    t = FT.ring_twin(fuse, harness, dead)  # ... with the finalizer program loaded too
    try:
        evp = events.EventProgram(ring_spec(t), RING_STRIDES)
        t.em.load_events(evp)
        t.em.set_event_rows(0, evp.rows([ring_identity(i) for i in range(R.N_FAST)]))
    except Exception:
        t.close()
        raise
    return t


@functools.lru_cache(maxsize=None)
def ring_reference(steps, harness=True, dead=True, reset=()):
    """Per step of the unfused twin: (merge stream, finalizer stream, event stream, guard words, order
    words); the event stream is checked against the reference on the way."""
    from tests import test_gpu_emit_finalizers as FT
    from tests import test_gpu_emit_ring as R
    t = ring_twin(False, harness, dead)
    try:
        t.em.reserve_fin(R.N_FAST + 1, 256 * R.N_FAST)
        t.em.reserve_events(R.N_FAST + 1, 520 * R.N_FAST)
        spec = ring_spec(t)
        ids = [ring_identity(i) for i in range(R.N_FAST)]
        out = []
        for k in range(steps):
            if k in reset:
                t.em.set_fin_words(0, FT.ring_words(t.em.fin_program))
            now = R.NOW0 + k * R.DT
            t.eng.step(now, R.SEED, k)
            t.eng.fired_compact(packed=True)
            merge = t.em.run(now, packed=True)
            fin, evt = t.em.collect_fin(), t.em.collect_events()
            t.eng.fired_compact(packed=False)
            want = expected("Pod", spec, ids, t.eng.fired(), now, R.N_FAST, [True] * R.N_FAST)
            check_stream(evt, want, f"reference step {k}")
            out.append((merge, fin, evt, t.words(), t.em.fin_words(0, R.N_FAST)))
        return out
    finally:
        t.close()


def same_evt(got, want, what):
    for f in ("rec", "status"):
        assert np.array_equal(got[0][f], want[0][f]), (what, f)
    assert np.array_equal(got[1], want[1]) and got[2] == want[2], what


def evt_room(ref):
    return max(len(r[2][0]) for r in ref) + 1, max(len(r[2][2]) for r in ref) + 1


def ring_run(t, ref, steps_per_group, n_steps):
    from kwok_amd.host import abi
    from tests import test_gpu_emit_finalizers as FT
    from tests import test_gpu_emit_ring as R
    t.eng.fired_keep(8)
    t.em.reserve_sets(8, *R.room([r[0] for r in ref]))
    t.em.reserve_fin(*FT.fin_room(ref))
    t.em.reserve_events(*evt_room(ref))
    for g in range(0, n_steps, steps_per_group):
        t.eng.step_n(steps_per_group, R.NOW0 + g * R.DT, R.DT, R.SEED, g, "packed16")
    for k in range(n_steps):
        assert t.eng.fired_view(k)["format"] == abi.COMPACT_PACKED16
        t.em.emit_step(k, R.NOW0 + k * R.DT)
    for k in range(n_steps):
        t.em.select(n_steps - 1 - k)
        R.same(t.em.collect(), ref[k][0], f"step {k}")
        FT.same_fin(t.em.collect_fin(), ref[k][1], f"step {k}")
        same_evt(t.em.collect_events(), ref[k][2], f"step {k}")
    assert np.array_equal(t.words(), ref[n_steps - 1][3])
    assert np.array_equal(t.em.fin_words(0, R.N_FAST), ref[n_steps - 1][4])


def test_ring_two_fused_groups_into_eight_sets():
    from tests import test_gpu_emit_ring as R
    ref = ring_reference(8)
    assert sum(len(r[2][0]) for r in ref) > 1000
    t = ring_twin(True)
    try:
        ring_run(t, ref, 4, 8)
        hole = False
        for k in range(8):
            c, cnt = R.seg_counts(t.eng, k)
            nz = np.flatnonzero(c)
            hole = hole or (cnt > 0 and bool(np.any(c[nz[0]:nz[-1] + 1] == 0)))
        assert hole  # a list with an empty segment between live ones
    finally:
        t.close()


def test_ring_a_step_that_fires_nothing():
    ref = ring_reference(8, False, False)
    assert 0 in [len(r[0][0]) for r in ref] and 0 in [len(r[2][0]) for r in ref]
    t = ring_twin(True, harness=False, dead=False)
    try:
        ring_run(t, ref, 8, 8)
    finally:
        t.close()


@pytest.mark.parametrize("short", ["events", "merge"])
def test_overflow_with_emissions_in_flight(short):
    """Four emissions of a fused group in flight, the second without room — one byte short in its
    event stream, or short in its merge patches with events loaded: it and the two behind it read
    KWK_ECAP from every reader, both word arrays are those after the first (no writer ran), and
    re-emitted with room from the failed step the three are exact."""
    from kwok_amd.host import abi
    from tests import test_gpu_emit_finalizers as FT
    from tests import test_gpu_emit_ring as R
    ref = ring_reference(12, True, True, FT.RESET)
    mb = [len(r[0][2]) for r in ref]
    eb = [len(r[2][2]) for r in ref]
    groups = [g for g in (0, 4, 8) if (eb if short == "events" else mb)[g + 1] > (eb if short == "events" else mb)[g]]
    assert groups, (mb, eb)
    g = groups[0]
    t = ring_twin(True)
    try:
        t.eng.fired_keep(8)
        t.em.reserve_fin(*FT.fin_room(ref))
        t.em.reserve_events(*evt_room(ref))
        t.em.reserve_sets(8, *R.room([r[0] for r in ref]))
        for g0 in range(0, g, 4):  # the groups before it, emitted as usual
            if g0 in FT.RESET:
                t.em.set_fin_words(0, FT.ring_words(t.em.fin_program))
            t.eng.step_n(4, R.NOW0 + g0 * R.DT, R.DT, R.SEED, g0, "packed16")
            for k in range(g0, g0 + 4):
                t.em.emit_step(k, R.NOW0 + k * R.DT)
            t.em.select(0)
            same_evt(t.em.collect_events(), ref[g0 + 3][2], f"step {g0 + 3}")
        if short == "events":
            t.em.reserve_events(evt_room(ref)[0], eb[g + 1] - 1)
            t.em.reserve_sets(4, *R.room([r[0] for r in ref]))  # another number of sets: fresh ones
        else:
            t.em.reserve_sets(4, R.room([r[0] for r in ref])[0], mb[g + 1] - 1)
        if g in FT.RESET:
            t.em.set_fin_words(0, FT.ring_words(t.em.fin_program))
        t.eng.step_n(4, R.NOW0 + g * R.DT, R.DT, R.SEED, g, "packed16")
        for k in range(g, g + 4):
            t.em.emit_step(k, R.NOW0 + k * R.DT)
        t.em.select(3)
        R.same(t.em.collect(), ref[g][0], f"step {g}")
        FT.same_fin(t.em.collect_fin(), ref[g][1], f"step {g}")
        same_evt(t.em.collect_events(), ref[g][2], f"step {g}")
        for k in (g + 1, g + 2, g + 3):
            t.em.select(g + 3 - k)
            assert R.emit_result_status(t.em) == abi.KWK_ECAP, k
            assert t.em.fin_result()[0] == abi.KWK_ECAP, k
            st, ni, nb, _ = t.em.event_result()
            assert st == abi.KWK_ECAP, k
            if k == g + 1 and short == "events":  # its own stream was the short one: the message says what to reserve
                assert (ni, nb) == (len(ref[k][2][0]), eb[k])
                assert f"kwk_evt_reserve({ni}, {nb})" in FT.emit_error(t.em)
            with pytest.raises(abi.EngineError):
                t.em.collect_events()
        assert np.array_equal(t.words(), ref[g][3])
        assert np.array_equal(t.em.fin_words(0, R.N_FAST), ref[g][4])
        t.em.reserve_events(*evt_room(ref))
        t.em.reserve_sets(4, *R.room([r[0] for r in ref]))
        for k in (g + 1, g + 2, g + 3):
            t.em.emit_step(k, R.NOW0 + k * R.DT)
        for k in (g + 1, g + 2, g + 3):
            t.em.select(g + 3 - k)
            R.same(t.em.collect(), ref[k][0], f"step {k} again")
            FT.same_fin(t.em.collect_fin(), ref[k][1], f"step {k} again")
            same_evt(t.em.collect_events(), ref[k][2], f"step {k} again")
        assert np.array_equal(t.words(), ref[g + 3][3])
        assert np.array_equal(t.em.fin_words(0, R.N_FAST), ref[g + 3][4])
    finally:
        t.close()


def test_one_set_event_overflow_stops_the_merge_and_finalizer_writers():
    """One output set, the event stream without room: the emission reads KWK_ECAP naming
    kwk_evt_reserve and the totals, no stream is written (the guard and the order words stay); with
    exactly the room asked for the same list emits exactly."""
    from kwok_amd.host import abi, events
    from tests import test_gpu_emit_finalizers as FT
    from tests import test_gpu_emit_ring as R
    from tests.parity_util import NOW0
    n = 300
    objs = FT.synthetic_objects(n)
    rig = FT.Rig(list(FT.synthetic_stages()), objs)
    spec = {"kind": "Pod", "api_version": "", "component": "kwok_controller",
            "stages": [RING_EVENTS[i % 3] for i in range(len(rig.prog.stages))]}
    evp = events.EventProgram(spec, (16, 8, 16))
    rig.em.load_events(evp)
    rig.em.set_event_rows(0, evp.rows(objs))
    rig.em.reserve_events(n + 1, 16)
    seen = []

    def pre(rig, now):
        rig.em.reserve(16 * n, 4096 * n)  # the merge patches have room
        w0, f0 = rig.em.words(0, n), rig.em.fin_words(0, n)
        rig.em.emit(now, packed=True)
        assert R.emit_result_status(rig.em) == abi.KWK_ECAP
        st, ei, eb, _ = rig.em.event_result()
        assert st == abi.KWK_ECAP and ei == n and eb > 350 * n
        assert f"kwk_evt_reserve({ei}, {eb})" in FT.emit_error(rig.em)
        assert rig.em.fin_result()[0] == abi.KWK_ECAP
        assert np.array_equal(rig.em.words(0, n), w0) and np.array_equal(rig.em.fin_words(0, n), f0)
        rig.em.reserve_events(ei, eb)  # exactly what it asked for
        seen.append((ei, eb))

    try:
        fired, _ = rig.step(0, NOW0, 0x53, "packed", pre=pre)
        want = expected("Pod", spec, objs, fired, NOW0, n, [True] * n)
        check_stream(rig.em.collect_events(), want, "with room")
        assert seen == [(len(want), sum(len(w[2]) for w in want))]
    finally:
        rig.close()

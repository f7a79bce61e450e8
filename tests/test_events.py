"""The Events of fired Stages on the host: the event program both compilers emit
(KindProgram.event_spec, kwk_program_event_spec), the native renderer (kwk_patch_event,
include/kwok_patch.h), its Python mirror (kwok_amd/host/events.py render_event) and
KindController.last_events.

Expected bytes everywhere: tests/event_ref.py, a restatement of client-go's generateEvent /
makeEvent over an encoding/json struct marshaller, itself pinned by the hand-derived vectors of
tests/golden/event_vectors.json."""
import copy
import itertools
import json
import os
import random
import subprocess

import numpy as np
import pytest

from kwok_amd import workload as W
from tests import event_ref
from tests import stage_fuzz as F
from tests.test_native_compiler import SETS, _pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VECTORS = json.load(open(os.path.join(ROOT, "tests", "golden", "event_vectors.json")))["vectors"]
VEC_NOW = 1700000000123456789
# 253402300799 s is 9999-12-31T23:59:59Z, the last instant RFC 3339 can write; as nanoseconds it is
# beyond int64_t (kwk_patch_event's now_ns), so the native renderer gets the largest int64 instead
# and the wrapper must refuse the other
NOW_LAST = 253402300799 * 10**9
NOWS = [0, 1, 999999999, 10**9, VEC_NOW, NOW_LAST]
INT64_MAX = 2**63 - 1
NAME_LENGTHS = [1, 3, 4, 5, 63, 253]
NAMESPACES = ["", "default", "n" * 63]
WIDGET = os.path.join(ROOT, "tests", "golden", "custom_stages", "widget.yaml")


def spec_of(kind, api_version, events):
    return json.dumps({"kind": kind, "api_version": api_version, "component": "kwok_controller", "stages": events})


def patcher(spec):
    from kwok_amd.host.patchtpl import PatchProgram
    return PatchProgram([], {}, events=spec)


def obj_of(kind, api_version, ns, name, uid):
    m = {"name": name}
    if ns:
        m["namespace"] = ns
    if uid:
        m["uid"] = uid
    return {"apiVersion": api_version, "kind": kind, "metadata": m}


def native_event(pp, stage, obj, now_ns):
    m = obj["metadata"]
    return pp.event(stage, m.get("namespace", ""), m["name"], m.get("uid", ""), obj.get("apiVersion", ""), now_ns)


# ------------------------------------------------------------------ the vectors
def test_reference_vectors_from_the_issue():
    """The three reference vectors, byte for byte, spelled out here as well as in the golden file."""
    v = {x["name"].split(":")[0]: x for x in VECTORS}
    assert v["vector 1"]["body"] == (
        '{"metadata":{"name":"pod-0.17979cfe3d85cd15","namespace":"default","creationTimestamp":null},'
        '"involvedObject":{"kind":"Pod","namespace":"default","name":"pod-0","uid":"11111111-2222-3333-4444-555555555555"},'
        '"reason":"Created","message":"Created container","source":{"component":"kwok_controller"},'
        '"firstTimestamp":"2023-11-14T22:13:20Z","lastTimestamp":"2023-11-14T22:13:20Z","count":1,"type":"Normal",'
        '"eventTime":null,"reportingComponent":"kwok_controller","reportingInstance":""}')
    assert ('"involvedObject":{"kind":"Node","name":"node-0","uid":"11111111-2222-3333-4444-555555555555"},"reason":"R",'
            '"source":') in v["vector 2"]["body"]
    assert '"name":"node-0.17979cfe3d85cd15","namespace":"default"' in v["vector 2"]["body"]
    assert '"type":"Warning"' in v["vector 2"]["body"] and '"message"' not in v["vector 2"]["body"]
    assert ('"involvedObject":{"kind":"Widget","namespace":"ns1","name":"w","uid":"u","apiVersion":"example.com/v1"}'
            in v["vector 3"]["body"])
    assert '"name":"w.17979cfe3d85cd15","namespace":"ns1"' in v["vector 3"]["body"]


@pytest.mark.parametrize("vec", VECTORS, ids=[v["name"] for v in VECTORS])
def test_reference_renderer_and_mirror_equal_the_vectors(vec):
    from kwok_amd.host.events import render_event
    want = vec["body"].encode()
    assert vec["cites"] and json.loads(vec["body"])
    assert event_ref.event_for(vec["kind"], vec["object"], vec["event"], vec["now_ns"]) == want
    spec = spec_of(vec["kind"], vec["api_version"], [vec["event"]])
    assert render_event(spec, 0, vec["object"], vec["now_ns"]) == want
    pp = patcher(spec)
    try:
        assert native_event(pp, 0, vec["object"], vec["now_ns"]) == want
    finally:
        pp.close()


# ------------------------------------------------------------------ the sweep
def with_events(docs, rng):
    """A copy of Stage documents with next.event drawn from the seeded RNG: supported and unsupported
    types, empty and escaped strings."""
    docs = copy.deepcopy(docs)
    types = ["Normal", "Warning", "Normal", "Warning", "", "normal", "Error"]
    texts = ["", "Created", "Stopping container", 'say "hi"', "a\\b", "x<y>&z", "line\nbreak\ttab\r", "caf\u00e9",
             "sep\u2028\u2029", "\U0001F600 smile"]
    for d in docs:
        if rng.random() < 0.75:
            d["spec"].setdefault("next", {})["event"] = {"type": rng.choice(types), "reason": rng.choice(texts),
                                                         "message": rng.choice(texts)}
    return docs


def sweep_programs():
    """[(name, Stage documents)]: every shipped set as it is, the sets without events and the custom
    Widget set again with events added."""
    from kwok_amd.host.native_compiler import stage_docs_from_files
    rng = random.Random(0xE7E27)
    out = []
    for name in sorted(SETS):
        docs = stage_docs_from_files(*W.stage_paths(SETS[name][0]))
        out.append((name, docs))
        out.append((name + "+events", with_events(docs, rng)))
    out.append(("widget+events", with_events(stage_docs_from_files(WIDGET), rng)))
    return out


def sweep_cases():
    """-> [(program name, spec, controller kind, [(stage, object, now_ns, expected bytes)])]."""
    from kwok_amd.host.compiler import KindProgram
    from kwok_amd.host.stages import stage_from_v1alpha1
    rng = random.Random(0x5EED)
    alphabet = "abcdefghijklmnopqrstuvwxyz0123456789-."
    out = []
    for pname, docs in sweep_programs():
        kp = KindProgram([stage_from_v1alpha1(d) for d in docs])
        spec = kp.event_spec()
        kind = kp.stages[0].kind
        av = kp.stages[0].api_group
        cases = []
        for s, st in enumerate(kp.stages):
            ev = st.next.event
            combos = list(itertools.product(NAME_LENGTHS, NAMESPACES, (True, False)))
            for j, (nl, ns, has_uid) in enumerate(combos):
                name = "".join(rng.choice(alphabet) for _ in range(nl))
                uid = "%08x-uid-%d" % (rng.getrandbits(32), j) if has_uid else ""
                o = obj_of(kind, av, ns, name, uid)
                for now in NOWS:
                    want = None if ev is None else event_ref.event_for(
                        kind, o, {"type": ev.type, "reason": ev.reason, "message": ev.message}, now)
                    cases.append((s, o, now, want or b""))
        out.append((pname, spec, kind, cases))
    return out


def test_seeded_sweep_equals_the_reference():
    from kwok_amd.host.events import render_event
    n_bodies = n_null = 0
    kinds = set()
    for pname, spec, kind, cases in sweep_cases():
        pp = patcher(spec)
        try:
            for s, o, now, want in cases:
                assert render_event(spec, s, o, now) == want, (pname, s, o, now)
                if now > INT64_MAX:
                    with pytest.raises(ValueError, match="int64_t"):
                        native_event(pp, s, o, now)
                    # the largest instant the C signature carries
                    ev = json.loads(spec)["stages"][s]
                    w2 = event_ref.event_for(kind, o, ev, INT64_MAX) if ev else b""
                    assert native_event(pp, s, o, INT64_MAX) == w2 == render_event(spec, s, o, INT64_MAX)
                else:
                    assert native_event(pp, s, o, now) == want, (pname, s, o, now)
                n_bodies += bool(want)
                n_null += not want
                if want:
                    kinds.add(kind)
        finally:
            pp.close()
    assert n_bodies >= 1000 and n_null >= 100 and kinds == {"Pod", "Node", "Widget"}


def test_escaping_and_omission_in_every_string():
    """Each escaped character alone and next to another, U+2028, a two-byte character, in the
    object's own strings as well as the stage's; empty reason, message and uid leave their keys out."""
    from kwok_amd.host.events import render_event
    pieces = ['"', "\\", "\n", "\r", "\t", "<", ">", "&", "\u2028", "\u2029", "\u00e9"]
    texts = pieces + [a + b for a in pieces for b in pieces] + ["a" + p + "b" for p in pieces]
    spec = spec_of("Widget", "example.com/v1", [{"type": "Normal", "reason": t, "message": t[::-1]} for t in texts])
    pp = patcher(spec)
    try:
        for s, t in enumerate(texts):
            o = obj_of("Widget", "av" + t, "ns" + t, "n" + t, t)
            want = event_ref.event_for("Widget", o, {"type": "Normal", "reason": t, "message": t[::-1]}, VEC_NOW)
            assert native_event(pp, s, o, VEC_NOW) == want == render_event(spec, s, o, VEC_NOW), repr(t)
            json.loads(want)
    finally:
        pp.close()
    spec = spec_of("Pod", "", [{"type": "Warning", "reason": "", "message": ""}])
    pp = patcher(spec)
    try:
        o = obj_of("Pod", "v1", "", "p", "")
        got = native_event(pp, 0, o, VEC_NOW)
        assert got == render_event(spec, 0, o, VEC_NOW) == event_ref.event_for("Pod", o, json.loads(spec)["stages"][0], VEC_NOW)
        d = json.loads(got)
        assert "reason" not in d and "message" not in d and d["involvedObject"] == {"kind": "Pod", "name": "p"}
        assert d["metadata"]["namespace"] == "default"
    finally:
        pp.close()


# ------------------------------------------------------------------ refusals
@pytest.mark.parametrize("typ", ["", "normal", "Error"])
def test_unsupported_types_give_no_item(typ):
    from kwok_amd.host.compiler import KindProgram
    from kwok_amd.host.events import render_event
    from kwok_amd.host.native_compiler import NativeProgram
    from kwok_amd.host.stages import stage_from_v1alpha1
    docs = [event_stage("s0", {"type": typ, "reason": "R", "message": "M"}), event_stage("s1", {"type": "Normal", "reason": "R"})]
    kp = KindProgram([stage_from_v1alpha1(d) for d in docs])
    nat = NativeProgram(docs)
    try:
        spec = kp.event_spec()
        assert nat.event_spec() == spec
        assert json.loads(spec)["stages"] == [None, {"type": "Normal", "reason": "R", "message": ""}]
        assert event_ref.generate_event({"Kind": "Pod", "Name": "p"}, typ, "R", "M", VEC_NOW) is None
        o = obj_of("Pod", "v1", "d", "p", "u")
        pp = patcher(spec)
        try:
            assert native_event(pp, 0, o, VEC_NOW) == b"" == render_event(spec, 0, o, VEC_NOW)
            assert native_event(pp, 1, o, VEC_NOW)
        finally:
            pp.close()
    finally:
        nat.close()


@pytest.mark.parametrize("field", ["ns", "name", "uid", "api_version"])
@pytest.mark.parametrize("bad,match", [(b"a\x01b", "control byte 0x01"), (b"x\x1f", "control byte 0x1f"),
                                       (b"a\x08", "control byte 0x08"), (b"a\xffb", "invalid UTF-8 byte 0xff"),
                                       (b"\xc3", "invalid UTF-8 byte 0xc3"), (b"\xc0\xaf", "invalid UTF-8 byte 0xc0"),
                                       (b"\xed\xa0\x80", "invalid UTF-8 byte 0xed"), (b"\xf4\x90\x80\x80", "invalid UTF-8 byte 0xf4")])
def test_refused_bytes_are_named(field, bad, match):
    from kwok_amd.host import abi
    a = {"ns": b"d", "name": b"p", "uid": b"u", "api_version": b"example.com/v1"}
    a[field] = bad
    what = {"ns": "namespace", "api_version": "apiVersion"}.get(field, field)
    pp = patcher(spec_of("Widget", "example.com/v1", [{"type": "Normal", "reason": "R", "message": ""}]))
    try:
        with pytest.raises(abi.EngineError, match=r"failed \(-1\).*" + what + ": " + match):
            pp.event(0, a["ns"], a["name"], a["uid"], a["api_version"], VEC_NOW)
    finally:
        pp.close()


@pytest.mark.parametrize("field", ["reason", "message", "type"])
def test_refused_control_bytes_in_the_program_are_named(field):
    """A stage string reaches the renderer through the spec's JSON, which cannot carry invalid UTF-8
    but can carry a control character."""
    from kwok_amd.host import abi
    ev = {"type": "Normal", "reason": "R", "message": "M"}
    ev[field] = ev[field] + "\x0c"
    pp = patcher(spec_of("Pod", "", [ev]))
    try:
        with pytest.raises(abi.EngineError, match=r"failed \(-1\).*" + field + ": control byte 0x0c"):
            pp.event(0, "d", "p", "u", "", VEC_NOW)
    finally:
        pp.close()


def test_mirror_refuses_what_the_renderer_refuses():
    from kwok_amd.host.events import render_event
    spec = spec_of("Pod", "", [{"type": "Normal", "reason": "R", "message": ""}])
    with pytest.raises(ValueError, match="control byte 0x01"):
        render_event(spec, 0, obj_of("Pod", "v1", "d", "a\x01", "u"), VEC_NOW)
    with pytest.raises(ValueError, match="invalid UTF-8"):
        render_event(spec, 0, obj_of("Pod", "v1", "d", "a\udc80", "u"), VEC_NOW)
    with pytest.raises(ValueError, match="now_ns < 0"):
        render_event(spec, 0, obj_of("Pod", "v1", "d", "a", "u"), -1)


def test_capacity_state_and_argument_errors():
    import ctypes as C
    from kwok_amd.host import abi
    from kwok_amd.host.patchtpl import PatchProgram, lib
    vec = VECTORS[0]
    want = vec["body"].encode()
    pp = patcher(spec_of("Pod", "", [vec["event"], None]))
    try:
        n = C.c_uint64()
        args = (b"default", b"pod-0", b"11111111-2222-3333-4444-555555555555", b"")
        assert lib().kwk_patch_event(pp.h, 0, *args, VEC_NOW, None, 0, C.byref(n)) == abi.KWK_ECAP
        assert n.value == len(want)
        assert f"{len(want)} bytes needed" in lib().kwk_patch_last_error(pp.h).decode()
        small = C.create_string_buffer(len(want) - 1)
        assert lib().kwk_patch_event(pp.h, 0, *args, VEC_NOW, small, len(want) - 1, C.byref(n)) == abi.KWK_ECAP
        assert n.value == len(want)
        out = C.create_string_buffer(n.value)
        assert lib().kwk_patch_event(pp.h, 0, *args, VEC_NOW, out, n.value, C.byref(n)) == abi.KWK_OK
        assert out.raw[:n.value] == want
        n.value = 99
        assert lib().kwk_patch_event(pp.h, 1, *args, VEC_NOW, None, 0, C.byref(n)) == abi.KWK_OK and n.value == 0
        assert lib().kwk_patch_event(pp.h, 0, *args, -1, out, len(out), C.byref(n)) == abi.KWK_EINVAL
        assert "now_ns < 0" in lib().kwk_patch_last_error(pp.h).decode()
        assert lib().kwk_patch_event(pp.h, 2, *args, VEC_NOW, out, len(out), C.byref(n)) == abi.KWK_EINVAL
        # a name of 253 bytes: longer than the wrapper's first buffer, so it takes the ECAP path
        long = obj_of("Pod", "v1", "n" * 63, "x" * 253, "u" * 36)
        assert native_event(pp, 0, long, VEC_NOW) == event_ref.event_for("Pod", long, vec["event"], VEC_NOW)
    finally:
        pp.close()
    none = PatchProgram([], {})
    try:
        assert not none.has_events and "events" not in json.loads(none.spec)
        with pytest.raises(abi.EngineError, match=r"\(-4\).*no event program"):
            none.event(0, "d", "p", "u", "", VEC_NOW)
    finally:
        none.close()


# ------------------------------------------------------------------ the compilers
def event_stage(name, event, kind="Pod", group="v1"):
    return {"apiVersion": "kwok.x-k8s.io/v1alpha1", "kind": "Stage", "metadata": {"name": name},
            "spec": {"resourceRef": {"apiGroup": group, "kind": kind},
                     "selector": {"matchExpressions": [{"key": ".metadata.labels.k", "operator": "In", "values": [name]}]},
                     "next": {"event": event}}}


@pytest.mark.parametrize("name", sorted(SETS))
def test_compilers_emit_the_same_event_program_shipped(name):
    kp, nat = _pair(name, False)
    try:
        for device in (False, True):
            spec = kp.event_spec(device)
            assert nat.event_spec(device) == spec
        d = json.loads(spec)
        assert d["kind"] == kp.stages[0].kind and d["api_version"] == "" and d["component"] == "kwok_controller"
        assert len(d["stages"]) == len(kp.stages)
        for st, s in zip(kp.stages, d["stages"]):
            e = st.next.event
            assert s == (None if e is None else {"type": e.type, "reason": e.reason, "message": e.message})
        if name == "pod-general+chaos":
            got = {kp.names[i]: s for i, s in enumerate(d["stages"]) if s}
            assert got == {"pod-create": {"type": "Normal", "reason": "Created", "message": "Created container"},
                           "pod-remove-finalizer": {"type": "Normal", "reason": "Killing", "message": "Stopping container"}}
        else:
            assert not any(d["stages"])
    finally:
        nat.close()


@pytest.mark.parametrize("name", F.CASE_IDS)
def test_compilers_emit_the_same_event_program_fuzz(name):
    """The 35 generated Stage sets, events added to the generator's output from a seeded RNG."""
    from kwok_amd.host.compiler import CompileError, KindProgram
    from kwok_amd.host import native_compiler
    from kwok_amd.host.stages import stage_from_v1alpha1
    docs, _ = F.case(name)
    docs = with_events(docs, random.Random("events:" + name))
    kp = KindProgram([stage_from_v1alpha1(d) for d in docs])
    nat = native_compiler.NativeProgram(docs)
    try:
        spec = kp.event_spec()
        assert nat.event_spec() == spec
        d = json.loads(spec)
        assert d["kind"] == F.KIND and d["api_version"] == F.API_GROUP
        try:
            dev = kp.event_spec(device=True)
        except CompileError as e:
            with pytest.raises(native_compiler.CompileError, match="event program not supported on the device"):
                nat.event_spec(device=True)
            assert "event program not supported on the device" in str(e)
        else:
            assert nat.event_spec(device=True) == dev == spec
    finally:
        nat.close()


def test_fuzz_events_cover_both_outcomes():
    from kwok_amd.host.compiler import CompileError, KindProgram
    from kwok_amd.host.stages import stage_from_v1alpha1
    assert len(F.CASE_IDS) == 35
    n_events = n_null = n_refused = n_accepted = 0
    for name in F.CASE_IDS:
        docs = with_events(F.case(name)[0], random.Random("events:" + name))
        kp = KindProgram([stage_from_v1alpha1(d) for d in docs])
        st = json.loads(kp.event_spec())["stages"]
        n_events += sum(1 for s in st if s)
        n_null += sum(1 for s in st if s is None)
        try:
            kp.event_spec(device=True)
            n_accepted += 1
        except CompileError:
            n_refused += 1
    assert n_events >= 35 and n_null >= 35 and n_refused >= 5 and n_accepted >= 2


def test_api_version_of_the_program():
    from kwok_amd.host.compiler import KindProgram
    from kwok_amd.host.native_compiler import NativeProgram
    from kwok_amd.host.stages import stage_from_v1alpha1
    ev = {"type": "Normal", "reason": "R", "message": "M"}
    for kind, group, want in [("Pod", "v1", ""), ("Node", "v1", ""), ("ConfigMap", "v1", "v1"),
                              ("Widget", "example.com/v1", "example.com/v1"), ("Pod", "example.com/v1", "example.com/v1")]:
        docs = [event_stage("s0", ev, kind, group)]
        kp = KindProgram([stage_from_v1alpha1(d) for d in docs])
        nat = NativeProgram(docs)
        try:
            spec = kp.event_spec()
            assert nat.event_spec() == spec
            d = json.loads(spec)
            assert (d["kind"], d["api_version"]) == (kind, want)
        finally:
            nat.close()


@pytest.mark.parametrize("which,match", [("quote", r'stage s1 reason has byte 0x22'), ("amp", r"stage s1 message has byte 0x26"),
                                         ("newline", r"stage s1 message has byte 0x0a"), ("utf8", r"stage s1 reason has byte 0xc3"),
                                         ("del", r"stage s1 reason has byte 0x7f"),
                                         ("size", r"16385 bytes of stage text \(more than 16384\)")])
def test_device_refusals_name_their_cause(which, match):
    from kwok_amd.host.compiler import CompileError, KindProgram
    from kwok_amd.host import native_compiler
    from kwok_amd.host.events import render_event
    from kwok_amd.host.stages import stage_from_v1alpha1
    ev = {"quote": {"type": "Normal", "reason": 'a"b', "message": "m"}, "amp": {"type": "Normal", "reason": "r", "message": "a&b"},
          "newline": {"type": "Warning", "reason": "r", "message": "a\nb"}, "utf8": {"type": "Normal", "reason": "café"},
          "del": {"type": "Normal", "reason": "a\x7f"},
          "size": {"type": "Normal", "reason": "r" * 8000, "message": "m" * (16385 - 8000 - 6 - len("Normalok okfine"))}}[which]
    docs = [event_stage("s0", {"type": "Normal", "reason": "ok ok", "message": "fine"}), event_stage("s1", ev),
            event_stage("s2", {"type": "bad\n", "reason": "\x01"})]  # an unsupported type is null: never refused
    kp = KindProgram([stage_from_v1alpha1(d) for d in docs])
    nat = native_compiler.NativeProgram(docs)
    try:
        with pytest.raises(CompileError, match="not supported on the device.*" + match):
            kp.event_spec(device=True)
        with pytest.raises(native_compiler.CompileError, match="not supported on the device.*" + match):
            nat.event_spec(device=True)
        # the host form renders the refused program
        spec = kp.event_spec()
        assert nat.event_spec() == spec
        o = obj_of("Pod", "v1", "d", "p", "u")
        e = {"type": ev["type"], "reason": ev.get("reason", ""), "message": ev.get("message", "")}
        pp = patcher(spec)
        try:
            assert native_event(pp, 1, o, VEC_NOW) == event_ref.event_for("Pod", o, e, VEC_NOW) == render_event(spec, 1, o, VEC_NOW)
        finally:
            pp.close()
    finally:
        nat.close()


def test_device_form_accepts_exactly_16_kib():
    from kwok_amd.host.compiler import KindProgram
    from kwok_amd.host.native_compiler import NativeProgram
    from kwok_amd.host.stages import stage_from_v1alpha1
    docs = [event_stage("s0", {"type": "Normal", "reason": "r" * 8000, "message": "m" * (16384 - 8000 - 6)})]
    kp = KindProgram([stage_from_v1alpha1(d) for d in docs])
    nat = NativeProgram(docs)
    try:
        assert nat.event_spec(True) == kp.event_spec(True) == kp.event_spec()
    finally:
        nat.close()


# ------------------------------------------------------------------ the controller
@pytest.mark.parametrize("native", [True, False], ids=["native", "python"])
def test_controller_records_the_events_of_pod_general(native):
    """KindController over pod-general, fired lists from the oracle's CPU stepper: last_events holds
    exactly the fired pod-create / pod-remove-finalizer slots, with the reference's bytes computed
    from the objects as they were before the step's patches."""
    from kwok_amd.host.compiler import KindProgram
    from kwok_amd.host.controller import KindController
    from kwok_amd.host.engine import Ingest
    from kwok_amd.host.stages import load_stage_files
    from kwok_amd.host import abi
    from oracle.next_ref import load_stage_docs
    from oracle.sim import OracleSim
    from tests.parity_util import NOW0
    cl = W.make_cluster("C2", 8, 60, seed=71)
    objs = cl.pods.materialize()
    prog = KindProgram(load_stage_files(*cl.pod_stage_files))
    prog.explore(objs)
    ctl = KindController(prog, None, Ingest(prog), objs, native=native)
    sim = OracleSim(load_stage_docs(*cl.pod_stage_files), objs)
    event_stages = {prog.names.index("pod-create"): {"type": "Normal", "reason": "Created", "message": "Created container"},
                    prog.names.index("pod-remove-finalizer"): {"type": "Normal", "reason": "Killing",
                                                               "message": "Stopping container"}}
    seen = {s: 0 for s in event_stages}
    try:
        for k in range(40):
            now = NOW0 + k * 500 * 10**6 + 123456789
            if k == 15:  # churn: the apiserver marks every third live pod deleted (a Modified event)
                for i in range(0, len(objs), 3):
                    if sim.objs[i] is not None:
                        for o in (sim.objs[i], ctl.objs[i]):
                            o["metadata"]["deletionTimestamp"] = "2023-11-14T22:13:27Z"
                        sim.dirty[i] = True
            before = copy.deepcopy(sim.objs)
            exp = sim.step(now, 0x71, k)
            fired = np.zeros(len(exp), dtype=abi.FIRED_DTYPE)
            for j, (slot, stage, flags) in enumerate(exp):
                fired[j] = (slot, stage, flags)
            ctl.handle(fired, now)
            want = {slot: event_ref.event_for("Pod", before[slot], event_stages[stage], now)
                    for slot, stage, _ in exp if stage in event_stages}
            assert ctl.last_events == want, f"step {k}"
            assert ctl.objs == sim.objs, f"step {k}"
            for slot, stage, _ in exp:
                if stage in event_stages:
                    seen[stage] += 1
        assert all(n > 0 for n in seen.values()), seen
    finally:
        ctl.close()


# ------------------------------------------------------------------ the stand-alone program
def test_standalone_program_under_sanitizers(tmp_path):
    """tools/event_check.cpp (its own main) built with -fsanitize=address,undefined over patch.cpp and
    run on the sweep's cases and the vectors: exact-size heap buffers, no sanitizer report."""
    lines = []
    n = 0
    for pname, spec, kind, cases in sweep_cases():
        lines.append("spec " + spec)
        for s, o, now, want in cases:
            if now > INT64_MAX:
                continue
            m = o["metadata"]
            f = [x.encode().hex() or "-" for x in (m.get("namespace", ""), m["name"], m.get("uid", ""), o["apiVersion"])]
            lines.append(f"case {s} {' '.join(f)} {now} {want.hex() or '-'}")
            n += 1
    for vec in VECTORS:
        lines.append("spec " + spec_of(vec["kind"], vec["api_version"], [vec["event"]]))
        m = vec["object"]["metadata"]
        f = [x.encode().hex() or "-" for x in (m.get("namespace", ""), m["name"], m.get("uid", ""), vec["object"]["apiVersion"])]
        lines.append(f"case 0 {' '.join(f)} {vec['now_ns']} {vec['body'].encode().hex()}")
        n += 1
    (tmp_path / "cases.txt").write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "event_check")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "event_check.cpp"),
                    os.path.join(ROOT, "kwok_amd", "csrc", "patch.cpp"), "-pthread", "-o", exe], check=True)
    r = subprocess.run([exe, str(tmp_path / "cases.txt")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert f"{n} cases, 0 bad" in r.stdout and "ERROR" not in r.stderr, r.stdout + r.stderr


# ------------------------------------------------------------------ the device stream's ABI (kwok_events.h)
def test_events_header_exports():
    """kwok_events.h's declarations are exported by libkwok_emit.so and listed in events.EXPORTS;
    kwok_emit.h and emit.EXPORTS do not know them."""
    import re
    from kwok_amd import build
    from kwok_amd.host import emit, events
    build.build()
    hdr = open(os.path.join(ROOT, "include", "kwok_events.h")).read()
    declared = re.findall(r"^\s*kwk_status\s+(kwk_\w+)\s*\(", hdr, re.M)
    assert sorted(declared) == sorted(events.EXPORTS) and all(n.startswith("kwk_evt_") for n in declared)
    out = subprocess.run(["nm", "-D", "--defined-only", emit.LIB_PATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r" T (kwk_\w+)", out))
    assert set(declared) <= exported
    assert exported == set(emit.EXPORTS) | set(events.EXPORTS)
    assert not [n for n in emit.EXPORTS if "evt" in n] and len(emit.EXPORTS) == 23 and len(events.EXPORTS) == 7
    emit_hdr = open(os.path.join(ROOT, "include", "kwok_emit.h")).read()
    assert "kwk_evt" not in emit_hdr and "kwok_events" not in emit_hdr


def test_event_program_rows():
    """EventProgram.rows: [length][text] rows; 0xFF for text that needs escaping or does not fit, for
    a missing object, and for every row of an object whose apiVersion is not the program's."""
    from kwok_amd.host import events
    spec = spec_of("Widget", "example.com/v1", [{"type": "Normal", "reason": "R", "message": ""}, None])
    p = events.EventProgram(spec, (8, 4, 8))
    assert p.any_event and not events.EventProgram(spec_of("Pod", "", [None]), (8, 4, 8)).any_event
    objs = [obj_of("Widget", "example.com/v1", "ns", "abcdefg", "u"), obj_of("Widget", "example.com/v1", "nsx", "abcdefgh", ""),
            obj_of("Widget", "example.com/v2", "ns", "a", "u"), None, obj_of("Widget", "example.com/v1", "n", "a b", 'q"')]
    r = p.rows(objs)
    assert bytes(r[events.COL_NAME][0]) == b"\x07abcdefg" and bytes(r[events.COL_NAMESPACE][0]) == b"\x02ns\0"
    assert bytes(r[events.COL_UID][0]) == b"\x01u" + b"\0" * 6
    assert r[events.COL_NAME][1, 0] == 0xFF and r[events.COL_NAMESPACE][1, 0] == 3 and r[events.COL_UID][1, 0] == 0
    assert [int(r[c][2, 0]) for c in range(3)] == [0xFF] * 3 == [int(r[c][3, 0]) for c in range(3)]
    assert r[events.COL_NAME][4, 0] == 0xFF and r[events.COL_NAMESPACE][4, 0] == 1 and r[events.COL_UID][4, 0] == 0xFF
    assert sorted(events.EventProgram(spec, (8, 0, 8)).rows(objs)) == [events.COL_NAME, events.COL_UID]


def evt_program(n_stages=2, strides=(16, 8, 40), kind="Pod", events=None):
    from kwok_amd.host import events as E
    ev = {"type": "Normal", "reason": "R", "message": "M"}
    return E.EventProgram(spec_of(kind, "", events if events is not None else [ev] * n_stages), strides)


def test_event_program_check_accepts_the_shipped_program():
    from kwok_amd.host import events as E
    from kwok_amd.host.compiler import KindProgram
    from kwok_amd.host.stages import load_stage_files
    kp = KindProgram(load_stage_files(*W.stage_paths(W.POD_GENERAL + W.POD_CHAOS)))
    E.EventProgram(kp.event_spec(device=True)).check()
    evt_program(32).check()  # KWK_MAX_STAGES stages fit the kernels' tables


@pytest.mark.parametrize("which,match", [
    ("33 stages", r"33 stages \(more than 32\)"), ("255 stages", r"255 stages \(more than 32\)"),
    ("stride", r"the name stride must be a multiple of 4 in 4\.\.256"), ("uid stride", r"the uid stride must be"),
    ("string", r"reason has byte 0x22.*\(stage 1\)"), ("kind", r"kind has byte 0x3c"),
    ("text", r"16386 bytes of stage text \(more than 16384\)"), ("type", r'stage 0 has type "normal"')])
def test_event_program_check_refusals_name_their_cause(which, match):
    """kwk_evt_check, the device-free half of kwk_evt_load: what the kernels' tables cannot hold is
    refused by name before any device memory is touched — in particular more stages than the
    KWK_MAX_STAGES entries of the kernels' LDS tables."""
    from kwok_amd.host import abi
    ev = {"type": "Normal", "reason": "R", "message": "M"}
    p = {"33 stages": lambda: evt_program(33), "255 stages": lambda: evt_program(255),
         "stride": lambda: evt_program(strides=(18, 8, 40)), "uid stride": lambda: evt_program(strides=(16, 8, 260)),
         "string": lambda: evt_program(events=[ev, dict(ev, reason='a"b')]), "kind": lambda: evt_program(kind="P<d"),
         "text": lambda: evt_program(events=[dict(ev, reason="r" * 8000, message="m" * (16386 - 8000 - 6))]),
         "type": lambda: evt_program(events=[dict(ev, type="normal")])}[which]()
    with pytest.raises(abi.EngineError, match=r"kwk_evt_check failed \(-1\): event program: .*" + match):
        p.check()


def test_an_empty_name_leaves_its_key_out():
    """ObjectReference.Name is omitempty (core/v1/types.go): the native renderer and the mirror
    drop the key as the reference does; metadata.name is then ".<hex>"."""
    from kwok_amd.host.events import render_event
    spec = spec_of("Widget", "example.com/v1", [{"type": "Normal", "reason": "R", "message": ""}])
    o = {"apiVersion": "example.com/v1", "kind": "Widget", "metadata": {"namespace": "d", "uid": "u"}}
    want = event_ref.event_for("Widget", o, json.loads(spec)["stages"][0], VEC_NOW)
    assert b'"involvedObject":{"kind":"Widget","namespace":"d","uid":"u","apiVersion":"example.com/v1"}' in want
    assert b'{"metadata":{"name":".17979cfe3d85cd15",' in want
    assert render_event(spec, 0, o, VEC_NOW) == want
    pp = patcher(spec)
    try:
        assert pp.event(0, "d", "", "u", "example.com/v1", VEC_NOW) == want
    finally:
        pp.close()


@pytest.mark.parametrize("native", [True, False], ids=["native", "python"])
def test_controller_step_survives_a_refused_string(native):
    """A fired object whose name the renderer refuses has no entry in last_events and one in
    event_errors naming the byte; the step's patches are applied as before."""
    from kwok_amd.host import abi
    from kwok_amd.host.compiler import KindProgram
    from kwok_amd.host.controller import KindController
    from kwok_amd.host.engine import Ingest
    from kwok_amd.host.stages import stage_from_v1alpha1
    docs = [event_stage("s0", {"type": "Normal", "reason": "R", "message": "M"})]
    objs = [{"apiVersion": "v1", "kind": "Pod", "metadata": {"name": n, "namespace": "d", "labels": {"k": "s0"}},
             "spec": {"containers": [{"name": "c", "image": "i"}]}} for n in ("ok", "bad\x01")]
    kp = KindProgram([stage_from_v1alpha1(d) for d in docs])
    kp.explore(objs)
    ctl = KindController(kp, None, Ingest(kp), objs, native=native)
    try:
        fired = np.zeros(2, dtype=abi.FIRED_DTYPE)
        fired[0], fired[1] = (0, 0, 0), (1, 0, 0)
        ctl.handle(fired, VEC_NOW)
        assert list(ctl.last_events) == [0] and list(ctl.event_errors) == [1]
        assert "control byte 0x01" in ctl.event_errors[1]
        assert ctl.last_events[0] == event_ref.event_for("Pod", objs[0], docs[0]["spec"]["next"]["event"], VEC_NOW)
    finally:
        ctl.close()

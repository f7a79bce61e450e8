"""Generated Stage sets (tests/stage_fuzz.py) through both Stage compilers against the oracle, on
the CPU: what a user may write goes well beyond kwok's shipped sets, and the tables the compilers
emit decide which sweep kernel runs (tests/test_gpu_stage_fuzz.py runs the same corpus on the
engine).

* the native compiler (libkwok_compiler) equals the Python compiler on every corpus case: table
  bytes, deltas, describe(), classes, encoder spec; native encoder rows equal the Python Ingest's;
* along an OracleSim run every live object's compiled match mask equals the oracle's
  (refcpu Lifecycle.match_mask: lifecycle.go:125-191) and its feature bits the oracle's own jq's;
* the corpus reaches every table shape and edge listed in test_corpus_coverage (computed from the
  oracle, so the corpus cannot go vacuous);
* refusals are named and the same in both compilers;
* the two defects the generator first found, as explicit regressions: requirements on one key
  that exclude each other must compile to a stage that never matches, and the "patch already
  applied" bits are numbered in ascending stage index by both compilers.

Measured (one CPU core): compile + explore 0.04-2.4 s (Python), <= 0.2 s (native), the
12-step oracle run 0.1-1.2 s per case."""
import json

import numpy as np
import pytest

from kwok_amd.host import compiler as pycompiler
from kwok_amd.host import native_compiler
from tests import stage_fuzz as F


@pytest.fixture(scope="module")
def programs():
    """name -> (KindProgram, NativeProgram), compiled once per case; a refusal is a failure."""
    cache = {}

    def get(name):
        if name not in cache:
            docs, objs = F.case(name)
            cache[name] = (F.compile_python(docs, objs), F.compile_native(docs, objs))
        return cache[name]

    yield get
    for _, nat in cache.values():
        nat.close()


def test_corpus_shape():
    assert 28 <= len(F.CORPUS) <= 36 and len(set(F.CASE_IDS)) == len(F.CORPUS)
    for name in F.CASE_IDS:
        docs, objs = F.case(name)
        assert 300 <= len(objs) <= 600, name
        assert all("{{" not in (d["spec"]["next"].get("statusTemplate") or "") for d in docs), name
    assert sum(not v for v in F.LOOPS.values()) * 3 >= len(F.CORPUS)
    assert F.make_case(7, n_objs=20) == F.make_case(7, n_objs=20)  # deterministic


@pytest.mark.parametrize("name", F.CASE_IDS)
def test_compilers_agree(name, programs):
    from kwok_amd.host.encoder import EncoderUnsupported, NativeIngest, encoder_spec
    from kwok_amd.host.engine import Ingest
    kp, nat = programs(name)
    docs, objs = F.case(name)
    assert nat.names == kp.names
    assert bytes(nat.table(5)) == bytes(kp.table(5))
    assert np.array_equal(nat.delta_array(), kp.delta_array())
    assert nat.describe() == kp.describe()
    assert nat.class_ids == kp.class_ids and len(kp.class_ids) >= (1 if name.startswith("b8-") else 2)
    try:
        want = encoder_spec(kp)
    except EncoderUnsupported:  # applied bits: the native spec carries the patches instead
        want = None
        assert kp.applied_bits and json.loads(nat.encoder_spec())["applied"]
    if not F.LOOPS[name]:
        assert want is not None and not kp.applied_bits, "a loops=False patch must falsify its own selector"
        assert not kp.delta_conflicts
    if want is not None:
        assert nat.encoder_spec() == want
        py = Ingest(kp)
        rows = py.columns(objs)
        ni = NativeIngest(nat)
        try:
            got = ni.columns(objs)
            for w, g, col in zip(rows, got, ("hot", "deletion", "rec", "cls")):
                assert np.array_equal(w, g), col
            assert np.array_equal(py.record_array(), ni.record_array())
        finally:
            ni.close()


@pytest.mark.parametrize("name", F.HARNESS_CASES)
def test_compilers_agree_with_harness(name):
    """HarnessSpec() compiles for the generated kind (Failed is in its phase vocabulary): the
    harness masks and the churn edges' deltas are equal in both compilers, and the oracle's churn
    re-creates objects in the run."""
    docs, objs = F.case(name)
    kp = F.compile_python(docs, objs, harness=True)
    nat = F.compile_native(docs, objs, harness=True)
    try:
        assert bytes(nat.table(2)) == bytes(kp.table(2))
        assert np.array_equal(nat.delta_array(), kp.delta_array())
        assert bytes(nat.harness_struct()) == bytes(kp.harness_struct()) and kp.harness_struct().enable == 1
        assert nat.describe() == kp.describe()
        assert not kp.delta_conflicts
    finally:
        nat.close()
    run = F.oracle_run(name, harness=True)
    assert sum(run.sim.gen) > 0 and run.total > 0


@pytest.mark.parametrize("name", F.CASE_IDS)
def test_compiled_match_equals_oracle(name, programs):
    """Every live object at every step of the oracle run (identical states checked once)."""
    from oracle.sim import oracle_pred
    kp, _ = programs(name)
    run = F.oracle_run(name)
    assert run.total > 0, "the case never fires"
    desc = kp.describe()
    applied = sum(1 << b for b in kp.applied_bits.values())
    seen, bad = set(), []
    for k, st in enumerate(run.steps):
        for o in st.objs:
            if o is None:
                continue
            key = F.state_key(o)
            if key in seen:
                continue
            seen.add(key)
            pred = kp.pred_of(o)
            if pred & ~applied != oracle_pred(desc, o):
                bad.append((k, "pred", hex(pred), hex(oracle_pred(desc, o)), key))
            got, want = kp.stage_matches(pred), run.sim.lc.match_mask(o)
            if got != want:
                bad.append((k, "match", bin(got), bin(want), key))
    assert not bad, f"{len(bad)} of {len(seen)} object states differ, first: {bad[:3]}"


def test_corpus_coverage(programs):
    """The table shapes and edges the corpus must reach; the run-time ones come from the oracle
    run alone (stage_fuzz.OracleRun.seen)."""
    shapes, seen, any4 = set(), set(), False
    for name in F.CASE_IDS:
        kp, _ = programs(name)
        docs, _ = F.case(name)
        run = F.oracle_run(name)
        assert run.total > 0, name
        seen |= run.seen
        w, ns = F.word_bits(kp), len(kp.names)
        if w <= 16:
            shapes.add("w16-delay" if F.has_delay(docs) else "w16-table")
            if 5 <= ns <= 8:
                shapes.add("w16-5to8-stages")
        elif w <= 28:
            shapes.add("w28")
        elif w <= 32:
            shapes.add("w32")
        if kp.nbits == 32:
            shapes.add("pred32")
        if ns == 32:
            shapes.add("32-stages")
        any4 |= any(d.n_any == 4 and all(bin(d.any_mask[i]).count("1") > 1 for i in range(4)) for d in kp.stage_desc)
        if len(kp.applied_bits) >= 4 and max(kp.applied_bits) >= 8:
            shapes.add("4-applied-bits")
        if kp.delta_conflicts:
            shapes.add("delta-conflict")
    assert shapes == {"w16-table", "w16-delay", "w16-5to8-stages", "w28", "w32", "pred32", "32-stages",
                      "4-applied-bits", "delta-conflict"}, shapes
    assert any4, "no stage with 4 multi-value In requirements"
    assert seen >= {"3-positive-weights", "all-weights-0", "jitter-draw", "abs-past", "abs-future", "deletion-column",
                    "matcherr", "delete", "finalizers-changed", "rematch", "no-rematch"}, seen


def _stage(name, exprs, nxt=None, **spec):
    return {"apiVersion": "kwok.x-k8s.io/v1alpha1", "kind": "Stage", "metadata": {"name": name},
            "spec": dict({"resourceRef": {"apiGroup": F.API_GROUP, "kind": F.KIND},
                          "selector": {"matchExpressions": exprs}, "next": nxt or {}}, **spec)}


def _refused(docs, objs, match):
    from kwok_amd.host.stages import stage_from_v1alpha1
    with pytest.raises(pycompiler.CompileError, match=match) as e1:
        pycompiler.KindProgram([stage_from_v1alpha1(d) for d in docs]).explore(objs)
    with pytest.raises(native_compiler.CompileError, match=match) as e2:
        nat = native_compiler.NativeProgram(docs)
        try:
            nat.explore(objs)
        finally:
            nat.close()
    return str(e1.value), str(e2.value)


def test_refusals_are_named_and_equal():
    obj = {"apiVersion": F.API_GROUP, "kind": F.KIND, "metadata": {"name": "g"}, "spec": {"size": 1}}
    one = lambda i: _stage("s%02d" % i, [{"key": F.PHASE, "operator": "In", "values": ["Pending"]}])  # noqa: E731
    a, b = _refused([one(i) for i in range(33)], [obj], "33 stages > 32")
    assert a == b
    lits = ["v%d" % i for i in range(33)]
    a, b = _refused([_stage("wide", [{"key": F.PHASE, "operator": "NotIn", "values": lits}])], [obj],
                    "stage set needs more than 32 feature bits")
    assert a == b
    ins = [{"key": k, "operator": "In", "values": ["a", "b"]} for k in
           (F.PHASE, F.NUM, F.label_key("tier"), F.label_key("zone"), F.annotation_key("mode"))]
    a, b = _refused([_stage("five", ins)], [obj], "stage five: more than 4 multi-value In requirements")
    assert a == b
    # 4 are accepted, by both
    docs = [_stage("four", ins[:4])]
    nat = native_compiler.NativeProgram(docs)
    nat.close()


CONTRADICTIONS = {
    "exists": [{"key": ".status.n", "operator": "DoesNotExist"}, {"key": ".status.n", "operator": "Exists"}],
    "exists-reversed": [{"key": ".status.n", "operator": "Exists"}, {"key": ".status.n", "operator": "DoesNotExist"}],
    "deletion": [{"key": F.DELETION, "operator": "DoesNotExist"}, {"key": F.DELETION, "operator": "Exists"}],
    "in-notin": [{"key": F.PHASE, "operator": "In", "values": ["a"]}, {"key": F.PHASE, "operator": "NotIn", "values": ["a"]}],
    "notin-in": [{"key": F.PHASE, "operator": "NotIn", "values": ["a"]}, {"key": F.PHASE, "operator": "In", "values": ["a"]}],
    "finalizer-in-none": [{"key": F.FINS, "operator": "In", "values": ["f"]}, {"key": F.FINS, "operator": "DoesNotExist"}],
    "finalizer-none-in": [{"key": F.FINS, "operator": "DoesNotExist"}, {"key": F.FINS, "operator": "In", "values": ["f"]}],
    "finalizer-in-notin": [{"key": F.FINS, "operator": "In", "values": ["f"]}, {"key": F.FINS, "operator": "NotIn", "values": ["f"]}],
    # all four any slots taken by multi-value In requirements
    "no-free-any": [{"key": k, "operator": "In", "values": ["a", "b"]} for k in
                    (F.PHASE, F.label_key("tier"), F.label_key("zone"), F.annotation_key("mode"))] +
                   [{"key": ".status.n", "operator": "Exists"}, {"key": ".status.n", "operator": "DoesNotExist"}],
}


@pytest.mark.parametrize("which", sorted(CONTRADICTIONS))
def test_contradictory_requirements_never_match(which):
    """Two requirements on one key that exclude each other: the reference never matches the stage
    (every requirement must hold, lifecycle.go:286-311).  The compilers used to OR both wants into
    eq_mask / eq_val, so the want-1 survived and the stage matched wherever the key existed."""
    from kwok_amd.host.stages import stage_from_v1alpha1
    from oracle import refcpu
    docs = [_stage("never", CONTRADICTIONS[which], {"statusTemplate": "phase: b\n"})]
    objs = []
    for st in ({}, {"n": 0}, {"n": 1, "phase": "a"}, {"phase": "a"}, {"phase": "b"}):
        for md in ({}, {"finalizers": ["f"]}, {"finalizers": ["g"]}, {"deletionTimestamp": "2023-11-14T22:13:10Z"},
                   {"labels": {"tier": "a", "zone": "b"}, "annotations": {"mode": "a"}, "finalizers": ["f", "g"]}):
            objs.append({"apiVersion": F.API_GROUP, "kind": F.KIND, "metadata": dict(md, name="g%d" % len(objs)),
                         "spec": {"size": 1}, "status": dict(st)})
    lc = refcpu.Lifecycle(docs)
    kp = pycompiler.KindProgram([stage_from_v1alpha1(d) for d in docs])
    kp.explore(objs)
    nat = native_compiler.NativeProgram(docs)
    try:
        nat.explore(objs)
        assert bytes(nat.table(1)) == bytes(kp.table(1))
    finally:
        nat.close()
    for o in objs:
        assert lc.match_mask(o) == 0
        assert kp.stage_matches(kp.pred_of(o)) == 0, o
    assert kp.stage_desc[0].n_any <= 4


def test_applied_bits_numbered_by_stage_index():
    """Idempotent stages at indices {5, 6, 8, 10}: both compilers give them consecutive bits in
    ascending stage index (the Python compiler used to follow the iteration order of a set)."""
    docs = []
    for i in range(11):
        if i in (5, 6, 8, 10):  # a patch that keeps its own selector true
            docs.append(_stage("s%02d" % i, [{"key": F.label_key("tier"), "operator": "In", "values": ["t%d" % i]}],
                               {"statusTemplate": "f%d: done\n" % i}))
        else:
            docs.append(_stage("s%02d" % i, [{"key": F.PHASE, "operator": "In", "values": ["p%d" % i]}],
                               {"statusTemplate": "phase: q\n"}))
    objs = [{"apiVersion": F.API_GROUP, "kind": F.KIND, "metadata": {"name": "g%d" % i, "labels": {"tier": "t%d" % i}},
             "spec": {"size": 1}, "status": {"phase": "p%d" % i}} for i in range(11)]
    kp = F.compile_python(docs, objs)
    nat = F.compile_native(docs, objs)
    try:
        assert sorted(kp.applied_bits) == [5, 6, 8, 10]
        bits = [kp.applied_bits[s] for s in (5, 6, 8, 10)]
        assert bits == list(range(bits[0], bits[0] + 4)), kp.applied_bits
        assert nat.applied_bits == kp.applied_bits
        assert nat.describe() == kp.describe()
        assert bytes(nat.table(1)) == bytes(kp.table(1))
        assert np.array_equal(nat.delta_array(), kp.delta_array())
    finally:
        nat.close()

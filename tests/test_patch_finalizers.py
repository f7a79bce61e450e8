"""Next.Finalizers' JSON patch natively (kwk_patch_finalizers, include/kwok_patch.h) and the
finalizer program both compilers emit for it (KindProgram.finalizer_spec,
kwk_program_finalizer_spec).

Reference: pkg/utils/lifecycle/next.go:43-60, finalizers.go:83-111.  Expected bytes everywhere:
json.dumps(oracle.refcpu.finalizers_modify(meta, fin), separators=(",", ":")) and nothing for []."""
import ctypes as C
import itertools
import json
import os
import random
import subprocess

import pytest

from kwok_amd import workload as W
from oracle import refcpu
from tests import stage_fuzz as F
from tests.test_native_compiler import SETS, _pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VEC = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_unit_vectors.json")))


def stage_doc(name, fin, **nxt):
    return {"apiVersion": "kwok.x-k8s.io/v1alpha1", "kind": "Stage", "metadata": {"name": name},
            "spec": {"resourceRef": {"apiGroup": "v1", "kind": "Pod"},
                     "selector": {"matchExpressions": [{"key": ".metadata.labels.k", "operator": "In", "values": [name]}]},
                     "next": dict(nxt, finalizers=fin)}}


def fin_json(empty, add, remove):
    f = {}
    if empty:
        f["empty"] = True
    if add:
        f["add"] = [{"value": v} for v in add]
    if remove:
        f["remove"] = [{"value": v} for v in remove]
    return f


def patcher(fins):
    """A patcher over one stage per StageFinalizers JSON, its finalizer program from the compiler."""
    from kwok_amd.host.compiler import KindProgram
    from kwok_amd.host.patchtpl import PatchProgram
    from kwok_amd.host.stages import stage_from_v1alpha1
    kp = KindProgram([stage_from_v1alpha1(stage_doc(f"s{i}", f)) for i, f in enumerate(fins)])
    return PatchProgram([], {}, finalizers=kp.finalizer_spec())


def want_bytes(meta, fin):
    ops = refcpu.finalizers_modify(meta, fin)
    return json.dumps(ops, separators=(",", ":")).encode() if ops else b""


def sweep_cases():
    """(programs' StageFinalizers lists, [(program, stage, meta)]): every combination of empty / add /
    remove over {a, b, c} (add lists in both orders and with a duplicate), against seeded lists of
    0..9 values from {a, b, c, x, y}."""
    adds = [list(c) for r in range(4) for c in itertools.combinations("abc", r)] + [["b", "a"], ["c", "c"], ["c", "a", "b"]]
    removes = [list(c) for r in range(4) for c in itertools.combinations("abc", r)]
    combos = [fin_json(e, a, r) for e in (False, True) for a in adds for r in removes]
    progs = [combos[i:i + 12] for i in range(0, len(combos), 12)]  # (a program has 32 feature bits)
    rng = random.Random(0xF1A)
    cases = []
    for p, fins in enumerate(progs):
        for s in range(len(fins)):
            for _ in range(14):
                cases.append((p, s, [rng.choice("abcxy") for _ in range(rng.randrange(10))]))
    return progs, cases


def test_reference_vectors():
    for case in VEC["finalizers_modify"]:
        pp = patcher([case["fin"]])
        try:
            got = pp.finalizers(0, case["meta"])
            assert got == (json.dumps(case["want"], separators=(",", ":")).encode() if case["want"] else b""), case["ref"]
            assert got == want_bytes(case["meta"] or [], case["fin"]), case["ref"]
        finally:
            pp.close()


def test_seeded_sweep_equals_the_oracle():
    progs, cases = sweep_cases()
    assert len(cases) >= 2000
    pps = [patcher(f) for f in progs]
    try:
        n_ops = 0
        for p, s, meta in cases:
            want = want_bytes(meta, progs[p][s])
            assert pps[p].finalizers(s, meta) == want, (progs[p][s], meta)
            n_ops += bool(want)
        assert n_ops >= 1000
    finally:
        for pp in pps:
            pp.close()


def test_order_word_round_trip():
    from kwok_amd.host import emit
    pp = patcher([fin_json(False, ["a", "b", "c"], [])])
    fp = emit.FinProgram(pp.spec and json.loads(pp.spec)["finalizers"])
    try:
        rng = random.Random(7)
        for n in range(8):
            for _ in range(20):
                fins = [rng.choice("abc") for _ in range(n)]
                w = pp.finalizer_word(fins)
                assert w >> 28 == n and w == fp.word(fins)
                assert (w & 0x0FFFFFFF) >> (4 * n) == 0  # unused nibbles are 0
                assert pp.finalizer_list(w) == fins
        assert pp.finalizer_word(list("abcabcab")) == 0xF0000000 == fp.word(list("abcabcab"))
        w = pp.finalizer_word(["a", "zz", "c", "example.com/q"])
        assert w == 4 << 28 | 0 | 15 << 4 | 2 << 8 | 15 << 12 == fp.word(["a", "zz", "c", "example.com/q"])
        from kwok_amd.host import abi
        with pytest.raises(abi.EngineError, match="outside the dictionary"):
            pp.finalizer_list(w)
        with pytest.raises(abi.EngineError, match="more than 7"):
            pp.finalizer_list(0xF0000000)
        assert pp.finalizer_word(None) == 0 and pp.finalizer_list(0) == []
    finally:
        pp.close()


@pytest.mark.parametrize("name", sorted(SETS))
def test_compilers_emit_the_same_program_shipped(name):
    kp, nat = _pair(name, False)
    try:
        spec = kp.finalizer_spec()
        assert nat.finalizer_spec() == spec
        d = json.loads(spec)
        assert d["values"] == list(kp.describe()["finalizers"]) and len(d["stages"]) == len(kp.stages)
        for st, s in zip(kp.stages, d["stages"]):
            f = st.next.finalizers
            assert [d["values"][i] for i in s["add"]] == (list(f.add) if f is not None else [])
            assert {d["values"][i] for i in s["remove"]} == (set(f.remove) if f is not None else set())
            assert bool(s["flags"] & 8) == (f is not None) and bool(s["flags"] & 1) == bool(st.next.delete)
    finally:
        nat.close()


@pytest.mark.parametrize("name", F.CASE_IDS)
def test_compilers_emit_the_same_program_fuzz(name):
    docs, objs = F.case(name)
    kp, nat = F.compile_python(docs, objs), F.compile_native(docs, objs)
    try:
        assert nat.finalizer_spec() == kp.finalizer_spec()
    finally:
        nat.close()


def test_add_order_and_duplicates_are_kept():
    from kwok_amd.host.compiler import KindProgram
    from kwok_amd.host.native_compiler import NativeProgram
    from kwok_amd.host.stages import stage_from_v1alpha1
    docs = [stage_doc("s0", fin_json(False, ["b", "a", "b"], ["c", "a", "c"])), stage_doc("s1", fin_json(True, [], []), delete=True)]
    kp = KindProgram([stage_from_v1alpha1(d) for d in docs])
    nat = NativeProgram(docs)
    try:
        spec = kp.finalizer_spec()
        assert nat.finalizer_spec() == spec
        d = json.loads(spec)
        assert d["values"] == ["b", "a", "c"]
        assert d["stages"] == [{"flags": 8 | 32, "add": [0, 1, 0], "remove": [1, 2]}, {"flags": 1 | 8 | 16, "add": [], "remove": []}]
    finally:
        nat.close()


@pytest.mark.parametrize("which,match", [("many", r"16 dictionary values \(more than 15\)"),
                                         ("quote", r"byte outside \[A-Za-z0-9\._/-\].*json\.Marshal")])
def test_refusals_name_their_cause(which, match):
    from kwok_amd.host.compiler import CompileError, KindProgram
    from kwok_amd.host import native_compiler
    from kwok_amd.host.stages import stage_from_v1alpha1
    if which == "many":
        docs = [stage_doc("s0", fin_json(False, [f"example.com/f{i}" for i in range(16)], []))]
    else:
        docs = [stage_doc("s0", fin_json(False, ['example.com/a"b'], []))]
    kp = KindProgram([stage_from_v1alpha1(d) for d in docs])
    nat = native_compiler.NativeProgram(docs)
    try:
        with pytest.raises(CompileError, match=match):
            kp.finalizer_spec()
        with pytest.raises(native_compiler.CompileError, match=match):
            nat.finalizer_spec()
        assert kp.describe() == nat.describe()  # the program itself compiles: the host renders these patches
    finally:
        nat.close()


def controller_bytes(docs, objs, fired):
    """KindController's native path over a fired list (no engine: the cache and the patches only)
    -> (last_fin_patches, fin_refused, the patcher has the finalizer program)."""
    import numpy as np
    from kwok_amd.host import abi
    from kwok_amd.host.compiler import KindProgram
    from kwok_amd.host.controller import KindController
    from kwok_amd.host.engine import Ingest
    from kwok_amd.host.stages import stage_from_v1alpha1
    kp = KindProgram([stage_from_v1alpha1(d) for d in docs])
    kp.explore(objs)
    ctl = KindController(kp, None, Ingest(kp), objs, native=True)
    try:
        rec = np.zeros(len(fired), dtype=abi.FIRED_DTYPE)
        for j, (slot, stage) in enumerate(fired):
            rec[j] = (slot, stage, 0)
        ctl._apply_native(rec, 1_700_000_000 * 10**9)
        return dict(ctl.last_fin_patches), ctl.fin_refused, ctl.patcher.has_finalizers
    finally:
        ctl.close()


def pod(i, k, fins):
    md = {"name": f"p{i}", "namespace": "d", "uid": f"u{i}", "labels": {"k": k}}
    if fins is not None:
        md["finalizers"] = list(fins)
    return {"apiVersion": "v1", "kind": "Pod", "metadata": md, "spec": {"containers": [{"name": "c", "image": "i"}]}}


@pytest.mark.parametrize("which", ["native", "many", "quote"])
def test_controller_sends_the_same_bytes_natively_and_for_a_refused_program(which):
    """KindController's native path records kwk_patch_finalizers' bytes in last_fin_patches; for a
    program the compilers refuse it says why (fin_refused) and the Python mirror renders the same
    bytes; no entry where the reference sends nothing."""
    add = {"native": ["b", "a"], "many": [f"example.com/f{i}" for i in range(16)], "quote": ['example.com/a"b', "a"]}[which]
    fins = [fin_json(False, add, []), fin_json(False, [], ["a"]), fin_json(True, [], [])]
    docs = [stage_doc(f"s{i}", f) for i, f in enumerate(fins)]
    metas = [None, ["a"], ["x", "a", "a"], list("aaaaaaaaa")]
    objs = [pod(i, f"s{i % 3}", metas[(i // 3) % 4]) for i in range(12)]
    fired = [(i, i % 3) for i in range(12)]
    got, refused, has = controller_bytes(docs, objs, fired)
    if which == "native":
        assert has and refused is None
    else:
        assert not has and ("more than 15" if which == "many" else "json.Marshal") in refused
    for slot, stage in fired:
        want = want_bytes(metas[(slot // 3) % 4] or [], fins[stage])
        assert got.get(slot, b"") == want, (which, slot)
    assert len(got) >= 6


def test_patcher_bytes_on_the_shipped_set():
    """kwk_patch_finalizers on pod-general's own stages."""
    from kwok_amd.host.compiler import KindProgram
    from kwok_amd.host.patchtpl import PatchProgram
    from kwok_amd.host.stages import load_stage_files
    kp = KindProgram(load_stage_files(*W.stage_paths(W.POD_GENERAL)))
    pp = PatchProgram(kp.stages, {}, finalizers=kp.finalizer_spec())
    try:
        assert pp.has_finalizers and "finalizers" in json.loads(pp.spec)
        create = kp.names.index("pod-create")
        assert pp.finalizers(create, None) == b'[{"op":"add","path":"/metadata/finalizers","value":["kwok.x-k8s.io/fake"]}]'
        rm = kp.names.index("pod-remove-finalizer")
        assert pp.finalizers(rm, ["x", "kwok.x-k8s.io/fake"]) == b'[{"op":"remove","path":"/metadata/finalizers/1"}]'
        assert pp.finalizers(rm, ["kwok.x-k8s.io/fake"]) == b'[{"op":"remove","path":"/metadata/finalizers"}]'
        assert pp.finalizers(kp.names.index("pod-ready"), ["x"]) == b""
    finally:
        pp.close()


def test_abi_unchanged_without_a_finalizer_program():
    """The feature is additive: the engine's exports and struct sizes are the parent's, the emit
    structs keep their layout, the new emitter entry points are new names."""
    from kwok_amd.host import abi, emit
    assert C.sizeof(emit.EmitItem) == 8 and C.sizeof(emit.EmitPiece) == 8 and C.sizeof(emit.EmitSkel) == 12
    assert C.sizeof(emit.EmitProgramStruct) == 104 and emit.ITEM_DTYPE.itemsize == 8
    assert C.sizeof(emit.EmitFinItem) == 8 == emit.FIN_ITEM_DTYPE.itemsize and C.sizeof(emit.EmitFinProgramStruct) == 56
    assert not [n for n in abi.EXPORTS if "fin" in n]
    old = ("kwk_emit_last_error", "kwk_emitter_create", "kwk_emitter_destroy", "kwk_emit_set_words",
           "kwk_emit_get_words", "kwk_emit_set_column", "kwk_emit_reserve", "kwk_emit", "kwk_emit_result",
           "kwk_emit_stats", "kwk_emit_device", "kwk_emit_copy", "kwk_emit_elapsed", "kwk_emit_step",
           "kwk_emit_reserve_sets", "kwk_emit_select")
    assert emit.EXPORTS[:len(old)] == old
    assert set(emit.EXPORTS[len(old):]) == {"kwk_emit_finalizers_load", "kwk_emit_set_fin_words", "kwk_emit_get_fin_words",
                                            "kwk_emit_reserve_fin", "kwk_emit_fin_result", "kwk_emit_fin_device",
                                            "kwk_emit_fin_copy"}
    hdr = open(os.path.join(ROOT, "include", "kwok_emit.h")).read()
    for n in emit.EXPORTS:
        assert n + "(" in hdr, n
    hdr = open(os.path.join(ROOT, "include", "kwok_patch.h")).read()
    from kwok_amd.host import patchtpl
    for n in ("kwk_patch_finalizers", "kwk_patch_finalizer_word", "kwk_patch_finalizer_list"):
        assert n + "(" in hdr and hasattr(patchtpl.lib(), n)


def test_standalone_program_under_sanitizers(tmp_path):
    """tools/fin_patch_check.cpp (its own main) built with -fsanitize=address,undefined over patch.cpp
    and run on the sweep's cases and the reference vectors: exact-size heap buffers, no report."""
    progs, cases = sweep_cases()
    lines = []
    for p, fins in enumerate(progs):
        pp = patcher(fins)
        lines.append("spec " + pp.spec)
        pp.close()
        for q, s, meta in cases:
            if q == p:
                lines.append(f"case {s} {len(meta)} {','.join(meta) or '-'} {want_bytes(meta, fins[s]).hex() or '-'}")
    for case in VEC["finalizers_modify"]:
        pp = patcher([case["fin"]])
        lines.append("spec " + pp.spec)
        pp.close()
        meta = case["meta"] or []
        lines.append(f"case 0 {len(meta)} {','.join(meta) or '-'} {want_bytes(meta, case['fin']).hex() or '-'}")
    (tmp_path / "cases.txt").write_text("\n".join(lines) + "\n")
    exe = str(tmp_path / "fin_patch_check")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "fin_patch_check.cpp"),
                    os.path.join(ROOT, "kwok_amd", "csrc", "patch.cpp"), "-pthread", "-o", exe], check=True)
    r = subprocess.run([exe, str(tmp_path / "cases.txt")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "0 bad" in r.stdout and "ERROR" not in r.stderr, r.stdout + r.stderr

"""Incremental usage updates, host side (no GPU): usage.UsageTable keeps the interning state of
usage_columns_dyn, so changed pods become kwk_usage_set_rows records plus appends whose ids
continue the configuration's; a pure-Python model of the engine's tables (tests/usage_rows_util.py)
applies them and resolves every pod.  The engine's own bookkeeping of ranges, mirrors and the
1-byte dictionary (kwok_amd/csrc/usage_rows.hpp) runs in tools/usage_rows_check.cpp under
-fsanitize=address,undefined."""
import os
import subprocess

import numpy as np
import pytest

from kwok_amd.host import abi, cel
from kwok_amd.host import usage as U
from kwok_amd.host.usage import UsageCompileError, UsageProgram, UsageTable, load_usage_yaml, usage_columns_dyn
from tests import usage_rows_util as R
from tests.usage_dyn_util import ANN, EXPR, usage_doc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMPTY = ("cpu_values", "mem_values", "cpu_progs", "mem_progs", "ops", "mixed", "ckeys")


def _same(a, b):
    assert len(a) == len(b) == 8
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y)


def test_config_equals_usage_columns_dyn_static():
    """usage-from-annotation.yaml + the EXTRA CR of tests/test_usage.py, that file's cluster."""
    from tests.test_usage import _cluster, _program
    _, pods = _cluster()
    tab = UsageTable(_program())
    cols = tab.config(pods)
    _same(cols, usage_columns_dyn(_program(), pods))
    assert len(cols[3]) and len(cols[5]) == 0  # mixed pods, no programs
    # the kept state names every pod's key again and asks for nothing new
    up = tab.rows(range(len(pods)), pods)
    assert np.array_equal(up["rows"]["usage_key"], cols[0]) and all(len(up[k]) == 0 for k in EMPTY)
    assert np.array_equal(up["rows"]["slot"], np.arange(len(pods))) and not up["rows"]["flags"].any()
    R.Model(cols).check(_program(), pods)


def test_config_equals_usage_columns_dyn_clock():
    """The clock-reading CRs of tests/test_usage_dynamic.py (programs interned by op bytes, mixed
    pods whose containers carry program ids)."""
    from tests.test_usage_dynamic import NODE, _dyn_docs, _pod
    pods = []
    for i in range(8):
        p = _pod(ann={ANN: "3Mi"} if i in (1, 2) else {ANN: "4Mi"} if i == 3 else None)
        p["metadata"]["name"] = f"pod-{i}"
        if i >= 6:
            p["spec"]["containers"].append({"name": "c1"})
        pods.append(p)
    docs = [_dyn_docs(), "\n---\n".join([usage_doc("a", EXPR["capped"], EXPR["ramp"], containers=["c0"]),
                                         usage_doc("b", "250m", EXPR["base_ramp"])])]
    for d in docs:
        prog = UsageProgram(*load_usage_yaml(d))
        tab = UsageTable(prog)
        cols = tab.config(pods, {"node-0": NODE})
        _same(cols, usage_columns_dyn(prog, pods, {"node-0": NODE}))
        assert len(cols[5]) + len(cols[6]) > 0
        up = tab.rows(range(len(pods)), pods, {"node-0": NODE})
        assert np.array_equal(up["rows"]["usage_key"], cols[0]) and all(len(up[k]) == 0 for k in EMPTY)
        R.Model(cols).check(prog, pods, {"node-0": NODE})


def test_seeded_batches_resolve_through_the_tables():
    """20 batches over 300 pods: replacements, annotation edits, uniform <-> mixed, container-count
    changes, new constants before the first program (appended as constants) and after it (one-op
    programs).  After every batch each container of each pod resolves, through the model's tables,
    to the constant or program UsageProgram.pod_container_programs gives for the pod now there."""
    rng = np.random.default_rng(20261)
    node_of = np.arange(300) // 25
    pods = R.make_pods(300, node_of)
    prog = R.program(dyn=True)
    tab = UsageTable(prog)
    model = R.Model(tab.config(pods))
    model.check(prog, pods)
    assert len(model.progs[0]) + len(model.progs[1]) == 0
    seen = set()
    for t in range(20):
        programs = t >= 8  # the first program arrives with batch 8
        slots, new, resets, created = R.batch(rng, pods, t, int(rng.integers(1, 60)), programs)
        n_const = [len(c) for c in model.const]
        had_progs = bool(model.progs[0] or model.progs[1])
        up = tab.rows(slots, new, reset=resets, created_ns=created)
        for s, p in zip(slots, new):
            pods[s] = p
        model.apply(up)
        model.check(prog, pods)
        rows = up["rows"]
        assert np.array_equal(rows["flags"] & abi.USAGE_ROW_RESET != 0, np.array(resets))
        assert np.array_equal(rows["flags"] & abi.USAGE_ROW_CREATED != 0, np.array([c is not None for c in created]))
        assert [int(c) for c, x in zip(rows["created_ns"], created) if x is not None] == [c for c in created if c is not None]
        if had_progs:  # the id rule
            assert [len(c) for c in model.const] == n_const
        seen.add(("const" if len(up["cpu_values"]) else "") + ("prog" if len(up["cpu_progs"]) + len(up["mem_progs"]) else "") +
                 ("mixed" if len(up["mixed"]) else ""))
    kinds = "".join(seen)
    assert "const" in kinds and "prog" in kinds and "mixed" in kinds
    assert model.progs[0] and model.progs[1] and any(int(k) >> 28 == 0 for k in model.keys)
    # a fresh configuration of the final pods resolves alike (other ids, the same values)
    R.Model(UsageTable(prog).config(pods)).check(prog, pods)


def _one(name, ns="default", cpu=None):
    md = {"name": name, "namespace": ns, "creationTimestamp": R.stamp(R.T0 - 100 * 10**9)}
    if cpu:
        md["annotations"] = {R.CPU_ANN: cpu}
    return {"metadata": md, "spec": {"nodeName": "node-0", "containers": [{"name": "container-0"}]}}


def test_a_new_constant_after_the_first_program_is_a_one_op_program():
    prog = R.program(dyn=True)
    tab = UsageTable(prog)
    cols = tab.config([_one("a"), _one("b", cpu="300m")])
    assert list(cols[1]) == [0.001, 0.3] and len(cols[5]) == 0
    up = tab.rows([0], [_one("a", cpu="700m")])          # no program yet: the next constant id
    assert list(up["cpu_values"]) == [prog.container_value(_one("a", cpu="700m"), "container-0", "cpu")]
    assert 0.69 < up["cpu_values"][0] < 0.71 and len(up["cpu_progs"]) == 0
    assert int(up["rows"]["usage_key"][0]) & 0x3FFF == 2
    up = tab.rows([1], [_one("c", ns="ramp")], reset=True)  # the first programs (cpu: capped; memory: the 5Mi fallback)
    assert len(up["cpu_progs"]) == 1 and len(up["cpu_values"]) == 0
    assert int(up["rows"]["usage_key"][0]) & 0x3FFF == 3 and int(up["rows"]["flags"][0]) == abi.USAGE_ROW_RESET
    # memory's 5Mi is new and the table has a program now: it travels as a program
    assert len(up["mem_values"]) == 0 and len(up["mem_progs"]) == 1
    first, n = up["mem_progs"][0]
    op = up["ops"][first - (tab.n_ops - len(up["ops"]))]
    assert n == 1 and op["op"] == cel.OP_CONST and op["value"] == 5.0 * 2**20
    up = tab.rows([0], [_one("a", cpu="900m")])
    assert len(up["cpu_values"]) == 0 and len(up["cpu_progs"]) == 1 and len(up["ops"]) == 1
    assert up["ops"][0]["op"] == cel.OP_CONST
    assert up["ops"][0]["value"] == prog.container_value(_one("a", cpu="900m"), "container-0", "cpu")
    assert int(up["rows"]["usage_key"][0]) & 0x3FFF == 4  # constants 0..2, programs 3..
    again = tab.rows([1], [_one("d", cpu="900m")])      # interned: nothing new
    assert all(len(again[k]) == 0 for k in EMPTY) and int(again["rows"]["usage_key"][0]) & 0x3FFF == 4


def test_bounds_and_a_refused_batch_leaves_the_table():
    prog = R.program(dyn=False)
    tab = UsageTable(prog)
    tab.config([_one("a")])
    before = (dict(tab.const_ids[0]), list(tab.n_const), tab.n_mixed)
    many = [_one(f"p{i}", cpu=f"{i + 2}m") for i in range(U.MAX_IDS)]
    with pytest.raises(UsageCompileError, match="16384"):
        tab.rows(range(len(many)), many)
    assert (dict(tab.const_ids[0]), list(tab.n_const), tab.n_mixed) == before
    ok = tab.rows(range(U.MAX_IDS - 1), many[:U.MAX_IDS - 1])  # ids 1..16383: the last one that fits
    assert len(ok["cpu_values"]) == U.MAX_IDS - 1 and tab.n_const[0] == U.MAX_IDS
    with pytest.raises(UsageCompileError, match="16384"):
        tab.rows([0], [many[-1]])
    # mixed indices: 2^28 - 1 entries at most
    mixed_pod = _one(R.MIXED_NAMES[0])
    mixed_pod["spec"]["containers"].append({"name": "container-1"})
    tab.n_mixed = U.MAX_MIXED - 1
    up = tab.rows([0], [mixed_pod])
    assert int(up["rows"]["usage_key"][0]) == U.MAX_MIXED - 1 and list(up["mixed"]) == [0, 2]
    mixed_pod["spec"]["containers"].append({"name": "container-2"})
    with pytest.raises(UsageCompileError, match="mixed"):
        tab.rows([0], [mixed_pod])
    assert tab.n_mixed == U.MAX_MIXED and tab.n_ckeys == 2


def test_bindings_declare_the_new_entry_points():
    header = open(os.path.join(ROOT, "include", "kwok_engine.h")).read()
    for name in ("kwk_usage_set_rows", "kwk_usage_append", "kwk_usage_mixed_append", "kwk_usage_info_get"):
        assert name in abi.EXPORTS and f"kwk_status {name}(" in header
    assert "#define KWK_ABI_VERSION 3" in header and abi.USAGE_ROW_DTYPE.itemsize == 24
    L = abi.lib()
    assert L.kwk_usage_set_rows(None, 0, None, None) != 0  # a null engine is refused, not dereferenced


def test_host_bookkeeping_under_sanitizers(tmp_path):
    """tools/usage_rows_check.cpp: the seeded batch sequence through usage_rows.hpp's Book, its rows
    executed on host arrays as usage_rows_kernel executes them, against a model and a fresh
    configuration of the same columns."""
    exe = str(tmp_path / "usage_rows_check")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "usage_rows_check.cpp"), "-o", exe], check=True)
    for batches, seed in ((20, 20261), (60, 7)):
        r = subprocess.run([exe, str(batches), str(seed)], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        assert f"{batches} batches" in r.stdout and " 0 failures" in r.stdout and "ERROR" not in r.stderr, r.stdout + r.stderr
        assert " 0 dictionary drops" not in r.stdout and " 0 rebuilds" not in r.stdout and " 0 reused" not in r.stdout

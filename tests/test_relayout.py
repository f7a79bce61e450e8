"""kwk_relayout, host side (no GPU): the gather body, the usage book's relayout and every refusal
run in tools/relayout_check.cpp under -fsanitize=address,undefined (a stand-alone program: nothing
is loaded into Python under a sanitizer); layout.plan_layout / apply_moves in numpy; the bindings."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from kwok_amd.host import abi, layout

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gather_book_and_refusals_under_sanitizers(tmp_path):
    """tools/relayout_check.cpp: relayout.hpp's gather body for 1..32-byte elements against a naive
    loop (identity runs, a run of one slot, shifts that differ modulo 4 and 16, fresh holes, shrink,
    grow, an empty list, seeded lists), Book::relayout against configure() + set_mixed() of the
    permuted columns on both sides of the 256th distinct key, and each refusal by name."""
    exe = str(tmp_path / "relayout_check")
    subprocess.run(["g++", "-std=c++17", "-g", "-O1", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tools", "relayout_check.cpp"), "-o", exe], check=True)
    for rounds, seed in ((40, 1), (25, 20261)):
        r = subprocess.run([exe, str(rounds), str(seed)], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        assert f"{rounds} rounds" in r.stdout and " 0 failures" in r.stdout and "ERROR" not in r.stderr, r.stdout + r.stderr
        # the seeded part met what it is there for
        for none in (" 0 kept columns", " 0 dictionary drops", " 0 mixed moved", " 0 mixed dropped"):
            assert none not in r.stdout, r.stdout


def _node_ids(node_ptr):
    return np.repeat(np.arange(len(node_ptr) - 1), np.diff(np.asarray(node_ptr, dtype=np.int64)))


def test_plan_layout_keeps_every_surviving_pod_in_its_nodes_range():
    rng = np.random.default_rng(5)
    for case in range(30):
        n_nodes = int(rng.integers(1, 12))
        sizes = rng.integers(0, 9, n_nodes)
        ptr = np.concatenate(([0], np.cumsum(sizes)))
        removed = [int(j) for j in np.flatnonzero(rng.random(n_nodes) < 0.25)]
        room = sizes + rng.integers(0, 3, n_nodes)  # some nodes get room
        added = [int(x) for x in rng.integers(0, 6, int(rng.integers(0, 3)))]
        moves, new_ptr, node_moves = layout.plan_layout(ptr, room, removed, added)
        n_new = int(new_ptr[-1])
        layout.check_moves(moves, int(ptr[-1]), n_new)  # the rules kwk_relayout checks
        surv = [j for j in range(n_nodes) if j not in removed]
        layout.check_moves(node_moves, n_nodes, len(surv) + len(added))
        assert len(new_ptr) == len(surv) + len(added) + 1 and new_ptr[0] == 0 and np.all(np.diff(new_ptr.astype(np.int64)) >= 0)
        assert list(np.diff(new_ptr.astype(np.int64))) == [int(room[j]) for j in surv] + added
        # every surviving pod, tagged with its old node and slot, lies in that node's new range, in order
        old_node = layout.apply_moves(_node_ids(ptr), moves, n_new, -1)
        old_slot = layout.apply_moves(np.arange(int(ptr[-1])), moves, n_new, -1)
        new_of_old = layout.apply_moves(np.arange(n_nodes), node_moves, len(surv) + len(added), -1)
        assert list(new_of_old[:len(surv)]) == surv and np.all(new_of_old[len(surv):] == -1)  # added nodes are fresh
        here = _node_ids(new_ptr)
        live = old_node >= 0
        assert np.array_equal(new_of_old[here[live]], old_node[live])
        assert sorted(old_slot[live]) == [s for j in surv for s in range(int(ptr[j]), int(ptr[j + 1]))]
        for j_new, j in enumerate(surv):
            seg = old_slot[int(new_ptr[j_new]):int(new_ptr[j_new + 1])]
            k = int(sizes[j])
            assert list(seg[:k]) == list(range(int(ptr[j]), int(ptr[j + 1]))) and np.all(seg[k:] == -1)


def test_plan_layout_shapes():
    ptr = [0, 4, 8, 12]
    # nothing changes: one identity run
    moves, new_ptr, node_moves = layout.plan_layout(ptr)
    assert moves.tolist() == [(0, 0, 12)] and node_moves.tolist() == [(0, 0, 3)] and new_ptr.tolist() == ptr
    # one node grown by a slot: the later slots shift by one
    moves, new_ptr, _ = layout.plan_layout(ptr, room=[4, 5, 4])
    assert moves.tolist() == [(0, 0, 8), (9, 8, 4)] and new_ptr.tolist() == [0, 4, 9, 13]
    # a node removed in the middle, two appended
    moves, new_ptr, node_moves = layout.plan_layout(ptr, removed_nodes=[1], added_nodes=[3, 2])
    assert moves.tolist() == [(0, 0, 4), (4, 8, 4)] and new_ptr.tolist() == [0, 4, 8, 11, 13]
    assert node_moves.tolist() == [(0, 0, 1), (1, 2, 1)]
    # compaction: only the kept slots move, to the front of their shrunk ranges
    keep = np.array([1, 0, 1, 0, 0, 0, 0, 0, 1, 1, 1, 1], dtype=bool)
    moves, new_ptr, _ = layout.plan_layout(ptr, room=[2, 0, 4], keep=keep)
    assert moves.tolist() == [(0, 0, 1), (1, 2, 1), (2, 8, 4)] and new_ptr.tolist() == [0, 2, 2, 6]
    with pytest.raises(ValueError, match="node 2: 4 slots kept, room for 3"):
        layout.plan_layout(ptr, room=[2, 0, 3], keep=keep)
    # a range that shrinks without `keep` drops its last slots
    moves, _, _ = layout.plan_layout(ptr, room=[4, 2, 4])
    assert moves.tolist() == [(0, 0, 6), (6, 8, 4)]


def test_apply_moves_is_the_gather():
    a = np.arange(10) * 10
    out = layout.apply_moves(a, [(1, 4, 3), (6, 0, 2)], 9, -7)
    assert out.tolist() == [-7, 40, 50, 60, -7, -7, 0, 10, -7]
    rows = np.zeros(4, dtype=abi.HOT_DTYPE)
    rows["pred"] = [1, 2, 3, 4]
    moved = layout.apply_moves(rows, layout.as_moves([(0, 2, 2)]), 3, np.zeros(1, dtype=abi.HOT_DTYPE)[0])
    assert moved["pred"].tolist() == [3, 4, 0] and moved.dtype == abi.HOT_DTYPE
    two_d = layout.apply_moves(np.arange(8.0).reshape(4, 2), [(0, 3, 1)], 2, 0.0)
    assert two_d.tolist() == [[6.0, 7.0], [0.0, 0.0]]
    for bad in ([(0, 0, 5), (4, 6, 2)], [(3, 0, 2), (0, 4, 2)], [(0, 0, 3), (3, 2, 2)], [(0, 9, 2)], [(8, 0, 2)]):
        with pytest.raises(ValueError):
            layout.check_moves(bad, 10, 9)


def test_bindings_declare_the_new_entry_points():
    header = open(os.path.join(ROOT, "include", "kwok_engine.h")).read()
    assert "kwk_status kwk_relayout(kwk_engine* eng, const kwk_layout* to);" in header
    assert "uint64_t kwk_layout_epoch(const kwk_engine* eng);" in header
    assert "typedef struct { uint32_t dst, src, n; } kwk_move;" in header
    assert "#define KWK_ABI_VERSION 3" in header  # additions only
    assert "kwk_relayout" in abi.EXPORTS and C.sizeof(abi.Move) == 12 and C.sizeof(abi.Layout) == 56
    assert [n for n, _ in abi.Layout._fields_] == ["n_active", "n_moves", "moves", "n_nodes", "node_ptr", "n_node_moves",
                                                   "node_moves", "fresh_usage_key"]
    L = abi.lib()
    assert L.kwk_relayout(None, None) == abi.KWK_EINVAL  # a null engine is refused, not dereferenced
    assert L.kwk_layout_epoch(None) == 0
    from kwok_amd.host.engine import Engine
    assert callable(Engine.relayout) and callable(Engine.layout_epoch)

"""Fused steps of the table-only 2-byte sweep (`sweep16_fsm_kernel<..., kSteps>`, DESIGN §5 "Fused table
steps"): kwk_step_n / _pair take a 2-byte table-only engine on a one-tile-per-workgroup grid through
4, 2 or 1 steps per launch, and the group's hand-backs run as one launch into ring slots of their own.

The engine is the bench's node engine: node-initialize + node-heartbeat (delay 20 s + up to 5 s of
Philox jitter, so every heartbeat runs the cold path and stores a due time).  DT is 22 s: a heartbeat
scheduled in one step comes due in the next step when its jitter is below 2 s and the step after
otherwise, so within one launch later steps both fire stages whose due time an earlier step of the
same launch stored and leave queued ones whose time has not come.  (A node that fires in step s - 1
is re-matched, and its next due time stored, in step s — a fire marks the object dirty and the match
comes before the fire within a step — so no node fires in two successive steps; "stored in step s,
fired in step s + 1 of the same launch" is a node in the lists of steps s - 1 and s + 1.)  Every case
steps a fused engine and a per-step twin (kwk_step_n(…, 1, …) calls) and compares each step's list
from the hand-back ring byte for byte; the per-step twin and `OracleSim` decide every expected value."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NOW0, SEED = 1_700_000_000 * 10**9, 0x6B776F6B
DT = 22 * 10**9


def _program():
    from kwok_amd import workload as W
    from kwok_amd.host.compiler import KindProgram
    from kwok_amd.host.stages import load_stage_files
    files = W.stage_paths(W.NODE_FAST + W.NODE_HEARTBEAT)
    nvars = [W.node_object("n"), W.node_object("n", annotations={"example.com/zone": "b"})]
    prog = KindProgram(load_stage_files(*files))
    prog.explore(nvars)
    return prog, nvars, files


def _variants(n):
    return (np.arange(n, dtype=np.int64) * 2654435761 >> 7) & 1


def _node_engine(prog, nvars, n, fuse=None, keep=16):
    """fuse None: the defaults (KWK_TUNE_FUSE_STEPS 4); else that value."""
    from kwok_amd.host import abi
    from kwok_amd.host.engine import Engine, Ingest
    ing = Ingest(prog)
    hot, dels, rec, cls = ing.variant_columns(nvars, _variants(n))
    eng = Engine(prog, capacity=n, kind_salt=1)
    if fuse is not None:
        eng.set_tuning(abi.TUNE_FUSE_STEPS, fuse)
    eng.load_stages()
    eng.load(hot, dels, rec, cls, ing.record_array())
    assert eng.stats()["state_bytes"] == 2  # jitter: not table-only ids, the 2-byte words
    eng.fired_keep(keep)
    return eng


def _fetch(eng, steps, fmt, bufs):
    """Steps' lists from the ring as arrays (copies), each checked for its tag and format."""
    from kwok_amd.host import abi
    dtype = abi.FIRED_DTYPE if fmt == "rec" else np.uint32
    code = abi.COMPACT_REC if fmt == "rec" else abi.COMPACT_PACKED
    infos = [eng.fetch_step(k, bufs[j]) for j, k in enumerate(steps)]
    eng.fetch_wait()
    out = []
    for j, (k, fi) in enumerate(zip(steps, infos)):
        assert fi["step"] == k and fi["format"] == code, (k, fi)
        out.append(bufs[j].array(dtype, fi["n_records"]).copy())
    return out


def _same_state(f, ref):
    (r_hot, r_del), (f_hot, f_del) = ref.read(), f.read()
    for col in ("pred", "sched"):
        assert np.array_equal(f_hot[col], r_hot[col]), col
    pend = (r_hot["sched"] & 0xFF) != 0xFF
    assert pend.any()
    assert np.array_equal(f_hot["due"][pend], r_hot["due"][pend]), "due column"
    assert np.array_equal(f_del, r_del)
    assert f.stats() == ref.stats(), (f.stats(), ref.stats())


def _slots(lst, fmt):
    return lst["slot"].astype(np.int64) if fmt == "rec" else (lst & np.uint32(2**27 - 1)).astype(np.int64)


def _stored_then_fired_in_one_launch(lists, fmt, steps):
    """Nodes that fired at step s - 1 and again at s + 1, for s in `steps` (list indices; s and s + 1
    steps of one launch): their due time was stored in step s and came due in step s + 1."""
    return sum(len(np.intersect1d(_slots(lists[s - 1], fmt), _slots(lists[s + 1], fmt))) for s in steps)


@pytest.mark.parametrize("fmt", ["rec", "packed"])
@pytest.mark.parametrize("n", [1500, 5000])  # one ragged tile; three tiles, the last ragged
def test_every_steps_list_equals_the_per_step_twin(n, fmt):
    """One call of 7 steps (launches of 4 + 2 + 1) and then one of 4 against 11 one-step calls on a
    twin: every step's list byte-equal, then the state, the due column and the statistics.  The
    4-step call's launch must report 4 steps (the fused path ran), and some node's due time must be
    stored in one step of a launch and fire in the next step of the same launch."""
    from kwok_amd.host import abi
    from kwok_amd.host.engine import PinnedBuffer
    prog, nvars, _ = _program()
    f, ref = _node_engine(prog, nvars, n), _node_engine(prog, nvars, n)
    bufs = [PinnedBuffer(8 * n + 64) for _ in range(7)]
    compact = True if fmt == "rec" else "packed"
    try:
        exp = []
        for k in range(11):
            ref.step_n(1, NOW0 + k * DT, DT, SEED, k, compact)
            assert ref.last_sweep()["steps"] in (0, 1)
            exp += _fetch(ref, [k], fmt, bufs)
        f.step_n(7, NOW0, DT, SEED, 0, compact)
        got = _fetch(f, list(range(7)), fmt, bufs)
        f.step_n(4, NOW0 + 7 * DT, DT, SEED, 7, compact)
        info = f.last_sweep()
        assert info["kernel"] == abi.SWEEP_16_FSM and info["steps"] == 4 and info["persistent"] == 0, info
        got += _fetch(f, list(range(7, 11)), fmt, bufs)
        for k in range(11):
            assert got[k].tobytes() == exp[k].tobytes(), f"step {k}: {len(got[k])} records, twin {len(exp[k])}"
        assert sum(len(x) for x in exp) > 2 * n  # initialize, then heartbeats
        # launches {0..3}, {4, 5}, {6}, {7..10}: the steps s with s + 1 in the same launch
        assert _stored_then_fired_in_one_launch(exp, fmt, [1, 2, 4, 7, 8, 9]) > 0
        # and queued stages whose time had not come stayed queued: not every node fires in every step
        assert min(len(x) for x in exp[2:]) < n
        _same_state(f, ref)
    finally:
        for e in (f, ref):
            e.close()
        for b in bufs:
            b.close()


def test_every_step_against_the_oracle():
    """5,000 nodes, launches of 4 + 2 + 1 and 4 + 4 + 2: every step's records and, after each call,
    every node's state against `OracleSim` stepped one step at a time."""
    from kwok_amd.host.engine import PinnedBuffer
    from oracle.next_ref import load_stage_docs
    from oracle.sim import OracleSim
    from tests.parity_util import compare_state
    n = 5000
    prog, nvars, files = _program()
    idx = _variants(n)
    eng = _node_engine(prog, nvars, n)
    bufs = [PinnedBuffer(8 * n + 64) for _ in range(10)]
    slots = list(range(n))
    sim = OracleSim(load_stage_docs(*files), [nvars[int(idx[s])] for s in slots], harness=False, slots=slots, kind_salt=1)
    try:
        k0, total, twice = 0, 0, 0
        for m in (7, 10):
            eng.step_n(m, NOW0 + k0 * DT, DT, SEED, k0, True)
            lists = _fetch(eng, list(range(k0, k0 + m)), "rec", bufs)
            for j, lst in enumerate(lists):
                k = k0 + j
                got = sorted(zip(lst["slot"].tolist(), lst["stage"].tolist(), lst["flags"].tolist()))
                exp = sorted(sim.step(NOW0 + k * DT, SEED, k))
                assert got == exp, f"step {k}: device-only {sorted(set(got) - set(exp))[:6]} oracle-only " \
                                   f"{sorted(set(exp) - set(got))[:6]}"
                total += len(exp)
            twice += _stored_then_fired_in_one_launch(lists, "rec", [1, 2])
            k0 += m
            compare_state(prog, eng, sim, k0 - 1, rows=eng.read())
        assert total > 2 * n and twice > 0
    finally:
        eng.close()
        for b in bufs:
            b.close()


def _pod_engine(n):
    from bench import shard_pod_variants
    from kwok_amd import workload as W
    from kwok_amd.host.compiler import HarnessSpec, KindProgram
    from kwok_amd.host.engine import Engine, Ingest
    from kwok_amd.host.stages import load_stage_files
    pvars = [W.pod_object("p", "n"), W.pod_object("p", "n", job=True)]
    prog = KindProgram(load_stage_files(*W.stage_paths(W.POD_FAST)), HarnessSpec())
    prog.explore(pvars)
    ing = Ingest(prog)
    hot, dels, rec, cls = ing.variant_columns(pvars, shard_pod_variants(0, n, SEED, 0.1))
    eng = Engine(prog, capacity=n, state="auto", max_records=max(1, len(ing.records)) + 16)
    eng.load_stages()
    eng.set_harness(True)
    eng.load(hot, dels, rec, cls, ing.record_array())
    assert eng.stats()["state_bytes"] == 1
    eng.fired_keep(16)
    return eng


def test_pair_call_equals_the_per_step_pair():
    """kwk_step_n_pair over a 1-byte pod engine (20k pods) and a 5,000-node engine, 10 steps in one
    call (both engines in launches of 4 + 4 + 2) against ten one-step pair calls on twins: both
    engines' lists of every step byte-equal, then both states."""
    from kwok_amd.host import abi
    from kwok_amd.host.engine import PinnedBuffer
    n_pods, n_nodes = 20_000, 5000
    prog, nvars, _ = _program()
    pods, pods_ref = _pod_engine(n_pods), _pod_engine(n_pods)
    nodes, nodes_ref = _node_engine(prog, nvars, n_nodes), _node_engine(prog, nvars, n_nodes)
    nbufs = [PinnedBuffer(4 * n_nodes + 64) for _ in range(10)]
    pbufs = [(PinnedBuffer(2 * n_pods + 64), PinnedBuffer(4 * (n_pods // 2048 + 64))) for _ in range(10)]

    def pod_lists(eng, steps):
        infos = [eng.fetch_step(k, *pbufs[j]) for j, k in enumerate(steps)]
        eng.fetch_wait()
        out = []
        for j, (k, fi) in enumerate(zip(steps, infos)):
            assert fi["step"] == k and fi["format"] == abi.COMPACT_PACKED16, (k, fi)
            out.append((pbufs[j][0].array(np.uint16, fi["n_records"]).copy(),
                        pbufs[j][1].array(np.uint32, fi["n_segs"]).copy()))
        return out

    try:
        exp_p, exp_n = [], []
        for k in range(10):
            pods_ref.step_n_pair(nodes_ref, 1, NOW0 + k * DT, DT, SEED, k, "packed16")
            exp_p += pod_lists(pods_ref, [k])
            exp_n += _fetch(nodes_ref, [k], "packed", nbufs)
        pods.step_n_pair(nodes, 10, NOW0, DT, SEED, 0, "packed16")
        assert pods.last_sweep()["kernel"] == abi.SWEEP_8 and pods.last_sweep()["steps"] == 2
        info = nodes.last_sweep()
        assert info["kernel"] == abi.SWEEP_16_FSM and info["steps"] == 2, info
        got_p, got_n = pod_lists(pods, list(range(10))), _fetch(nodes, list(range(10)), "packed", nbufs)
        for k in range(10):
            assert got_n[k].tobytes() == exp_n[k].tobytes(), f"nodes, step {k}"
            assert got_p[k][0].tobytes() == exp_p[k][0].tobytes(), f"pods, step {k}: records"
            assert got_p[k][1].tobytes() == exp_p[k][1].tobytes(), f"pods, step {k}: segment counts"
        assert sum(len(x) for x in exp_n) > 2 * n_nodes and sum(len(r) for r, _ in exp_p) > n_pods
        assert _stored_then_fired_in_one_launch(exp_n, "packed", [1, 2, 4, 5, 6, 8]) > 0
        _same_state(nodes, nodes_ref)
        (r_hot, _), (f_hot, _) = pods_ref.read(), pods.read()
        for col in ("pred", "sched"):
            assert np.array_equal(f_hot[col], r_hot[col]), col
    finally:
        for e in (pods, pods_ref, nodes, nodes_ref):
            e.close()
        for b in nbufs:
            b.close()
        for x in pbufs:
            for b in x:
                b.close()


def test_fuse_steps_one_takes_the_per_step_path():
    """KWK_TUNE_FUSE_STEPS 1 on the node engine: one launch per step as before, the same lists."""
    from kwok_amd.host.engine import PinnedBuffer
    n = 5000
    prog, nvars, _ = _program()
    f, off = _node_engine(prog, nvars, n), _node_engine(prog, nvars, n, fuse=1)
    bufs = [PinnedBuffer(4 * n + 64) for _ in range(7)]
    try:
        f.step_n(7, NOW0, DT, SEED, 0, "packed")
        off.step_n(4, NOW0, DT, SEED, 0, "packed")
        assert off.last_sweep()["steps"] in (0, 1), off.last_sweep()
        off.step_n(3, NOW0 + 4 * DT, DT, SEED, 4, "packed")
        got, exp = _fetch(f, list(range(7)), "packed", bufs), _fetch(off, list(range(7)), "packed", bufs)
        for k in range(7):
            assert got[k].tobytes() == exp[k].tobytes(), f"step {k}"
        assert sum(len(x) for x in exp) > 2 * n
        _same_state(f, off)
    finally:
        for e in (f, off):
            e.close()
        for b in bufs:
            b.close()

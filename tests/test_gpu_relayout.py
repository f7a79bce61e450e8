"""kwk_relayout on the device: whole runs of slots moved on the engine's stream, everything an
object or node owns travelling with it.

The move set used throughout (tests/test_relayout.py checks plan_layout itself): five node ranges,
some straddling sweep-tile boundaries; the first node stays in place, node 1 grows by one slot
(every later slot shifts by one byte in the 1-byte columns), node 3 in the middle is removed, two
nodes are appended; n_active crosses a tile boundary upwards ("up") or downwards ("down").  The
largest engine has three sweep tiles (kwk_tile_objects(), never a literal).

State: engine A is loaded, stepped so that stages are pending with due times, relayouted and
stepped on; engine B is created afterwards and kwk_load'ed from layout.apply_moves of A's rows and
stepped the same steps.  Objects are independent within a step and the Philox counter is the global
slot, so every step's fired list, the final rows and the per-stage counts are equal bit for bit —
the twin and, for one case, OracleSim over a sample of the moved slots decide every expected value.
Usage: engine C never relayouts; a moved pod's values at dst in A are C's at src bit for bit (same
inputs, same per-pod arithmetic); node and cluster sums within the usage tolerance of 1e-6 relative
(lane assignment differs between layouts)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NOW0, SEED = 1_700_000_000 * 10**9, 0x6B776F6B
I64_MIN = np.iinfo(np.int64).min


def _tile():
    from kwok_amd.host import abi
    return int(abi.lib().kwk_tile_objects())


def _plan(direction):
    """-> (old node_ptr, moves, new node_ptr, node_moves)."""
    from kwok_amd.host import layout
    t = _tile()
    u = t // 2048
    # up: 3900 u slots (below 2 tiles) -> 4901 u (the third tile); down: 4200 u (the third tile) -> 3551 u
    sizes = [700 * u, 900 * u, 600 * u, 800 * u, (900 if direction == "up" else 1200) * u]
    added = [1500 * u, 300 * u] if direction == "up" else [100 * u, 50 * u]
    ptr = np.concatenate(([0], np.cumsum(sizes))).astype(np.uint32)
    room = list(sizes)
    room[1] += 1
    moves, new_ptr, node_moves = layout.plan_layout(ptr, room, removed_nodes=[3], added_nodes=added)
    n_old, n_new = int(ptr[-1]), int(new_ptr[-1])
    assert (n_old // t) != (n_new // t) and (n_new > n_old) == (direction == "up") and max(n_old, n_new) > 2 * t
    assert any(int(ptr[j]) // t != (int(ptr[j + 1]) - 1) // t for j in range(5))  # a range straddles a tile boundary
    assert moves["dst"][0] == 0 and moves["src"][0] == 0 and len(moves) == 3  # in place, shifted by one, shifted further
    return ptr, moves, new_ptr, node_moves


def _same(x, y, what):
    assert x.dtype == y.dtype and x.shape == y.shape, what
    if not np.array_equal(x, y):
        at = np.flatnonzero(x != y) if x.ndim == 1 else np.flatnonzero(np.any((x != y).reshape(len(x), -1), axis=1))
        raise AssertionError(f"{what}: {len(at)} rows differ, first {at[:5].tolist()}: {x[at[:3]]} vs {y[at[:3]]}")


def _same_rows(x, y, what):
    """kwk_read rows: pred and sched everywhere, due where a stage is pending — kwok_engine.h: "due is
    meaningful only while a stage is pending" (a fused record whose stage has fired keeps stale due
    bits, which read back relative to the engine's own epoch)."""
    from kwok_amd.host import abi
    _same(x["pred"], y["pred"], what + ": pred")
    _same(x["sched"], y["sched"], what + ": sched")
    pend = (x["sched"] & np.uint32(0xFF)) != abi.STAGE_NONE
    _same(x["due"][pend], y["due"][pend], what + ": due of pending stages")


def _sorted_fired(eng):
    f = eng.fired()
    return np.sort(f, order=["slot", "stage", "flags"])


# ------------------------------------------------------------------ 1 + 2: state, every format
def _pod_fast(n):
    from tests import test_gpu_fused_carry as F
    prog, pvars = F._program()
    return prog, pvars, F._hash_variants(n), True, 0, 10**9


def _pod_general(n):
    from kwok_amd import workload as W
    from kwok_amd.host.compiler import HarnessSpec, KindProgram
    from kwok_amd.host.stages import load_stage_files
    files = W.stage_paths(W.POD_GENERAL + W.POD_CHAOS)
    pvars, pidx = W.c2_pod_variants(0, n, seed=SEED, job_frac=0.1)
    prog = KindProgram(load_stage_files(*files), HarnessSpec())
    prog.explore(pvars)
    return prog, pvars, pidx, True, 0, 2 * 10**9


def _node_heartbeat(n):
    from kwok_amd import workload as W
    from kwok_amd.host.compiler import KindProgram
    from kwok_amd.host.stages import load_stage_files
    nvars = [W.node_object("n"), W.node_object("n", annotations={"example.com/zone": "b"})]
    prog = KindProgram(load_stage_files(*W.stage_paths(W.NODE_FAST + W.NODE_HEARTBEAT)))
    prog.explore(nvars)
    return prog, nvars, (np.arange(n, dtype=np.int64) * 2654435761 >> 7) & 1, False, 1, 4 * 10**9


CASES = {
    # name: (builder, Engine state, state bytes, direction)
    "pod-fast-1byte": (_pod_fast, "auto", 1, "up"),
    "pod-fast-2byte": (_pod_fast, "u16", 2, "down"),
    "pod-general-fused": (_pod_general, "auto", 8, "up"),
    "pod-general-split-due": (_pod_general, "u32", 4, "down"),
    "pod-general-wide": (_pod_general, "wide", 8, "up"),
    "node-heartbeat": (_node_heartbeat, "auto", 2, "down"),
}


def _stage_files(name):
    from kwok_amd import workload as W
    return W.stage_paths(W.POD_GENERAL + W.POD_CHAOS) if name.startswith("pod-general") else None


@pytest.mark.parametrize("name", list(CASES))
def test_state_travels_in_every_format(name):
    from kwok_amd.host import abi, layout
    from kwok_amd.host.engine import Engine, Ingest
    builder, state, state_bytes, direction = CASES[name]
    ptr, moves, new_ptr, _ = _plan(direction)
    n_old, n_new = int(ptr[-1]), int(new_ptr[-1])
    cap = max(n_old, n_new) + 5
    prog, variants, idx, harness, salt, dt = builder(n_old)
    idx = np.asarray(idx)
    ing = Ingest(prog)
    hot, dels, rec, cls = ing.variant_columns(variants, idx)
    # one object's pending stage is due beyond the fused records' window (~68 s): its time is in the column
    far = int(ptr[4]) + 5  # (in the last node: it shifts)
    hot["sched"][far] = (hot["sched"][far] & ~np.uint32(0xFF | abi.F_DIRTY)) | np.uint32(0)
    hot["due"][far] = NOW0 + 500 * 10**9
    records = ing.record_array()

    def engine():
        e = Engine(prog, capacity=cap, state=state, kind_salt=salt, max_records=max(1, len(ing.records)) + 16)
        e.load_stages()
        e.set_harness(harness)
        return e

    sim = None
    if name == "pod-general-fused":  # 2: the oracle over a sample of the slots that move
        from oracle.next_ref import load_stage_docs
        from oracle.sim import OracleSim
        moved_src = np.concatenate([np.arange(m["src"], m["src"] + m["n"]) for m in moves])
        moved_dst = np.concatenate([np.arange(m["dst"], m["dst"] + m["n"]) for m in moves])
        pick = np.arange(5, len(moved_src), 23)
        pick = pick[moved_src[pick] != far]
        sim = OracleSim(load_stage_docs(*_stage_files(name)), [variants[int(idx[s])] for s in moved_src[pick]], harness=True,
                        slots=[int(s) for s in moved_src[pick]])
        assert np.any(moved_src[pick] != moved_dst[pick]) and np.any(moved_src[pick] == moved_dst[pick])

    def check_sim(eng, now, k):
        if sim is None:
            return
        f = eng.fired()
        sel = f[np.isin(f["slot"].astype(np.int64), np.asarray(sim.slots, dtype=np.int64))]
        got = sorted((int(r["slot"]), int(r["stage"]), int(r["flags"])) for r in sel)
        assert got == sorted(sim.step(now, SEED, k)), f"step {k} against the oracle"

    a = engine()
    b = None
    try:
        a.load(hot, dels, rec, cls, records)
        assert a.stats()["state_bytes"] == state_bytes
        k0 = 3
        for k in range(k0):
            a.step(NOW0 + k * dt, SEED, k)
            check_sim(a, NOW0 + k * dt, k)
        before = a.stats()
        rows0, dels0 = a.read(0, n_old)
        pend = (rows0["sched"] & 0xFF) != abi.STAGE_NONE
        assert pend.sum() > (0 if name.startswith("pod-fast") else 10) and rows0["due"][far] == NOW0 + 500 * 10**9  # stages are pending with due times
        assert a.layout_epoch() == 0
        a.fired_compact()
        assert a.fired_view(k0 - 1)["step"] == k0 - 1
        a.relayout(moves, n_new)
        assert a.layout_epoch() == 1 and a.n == n_new
        if sim is not None:  # the sampled objects draw from their new slots' streams from here on
            sim.slots = [int(s) for s in moved_dst[pick]]
        zero_row = np.zeros(1, dtype=abi.HOT_DTYPE)[0]
        want_rows = layout.apply_moves(rows0, moves, n_new, zero_row)
        want_dels = layout.apply_moves(dels0, moves, n_new, abi.DEL_ABSENT)
        rows1, dels1 = a.read(0, n_new)
        _same(rows1, want_rows, "rows right after the relayout")
        _same(dels1, want_dels, "deletion column right after the relayout")
        assert a.stats()["fired"] == before["fired"] and a.stats()["state_bytes"] == state_bytes  # statistics stay
        with pytest.raises(abi.EngineError, match=r"\(%d\)" % abi.KWK_ESTATE):  # the ring is emptied
            a.fired_view(k0 - 1)
        # the twin, created afterwards, loaded in the new layout
        b = engine()
        b.load(want_rows, want_dels, layout.apply_moves(rec, moves, n_new, 0),
               (want_rows["sched"] >> np.uint32(16)).astype(np.uint16), records)
        k = k0
        for j in range(10):  # per step; pod-general: 20 s of clock, across the fused records' epoch re-encode
            now = NOW0 + k * dt
            a.step(now, SEED, k)
            b.step(now, SEED, k)
            _same(_sorted_fired(a), _sorted_fired(b), f"fired list of step {k}")
            check_sim(a, now, k)
            k += 1
        for e in (a, b):  # the fused path (where the engine fuses: kwk_step_n decides alike for both)
            e.step_n(4, NOW0 + k * dt, dt, SEED, k, True)
        _same(_sorted_fired(a), _sorted_fired(b), "fired list after kwk_step_n")
        ra, da = a.read(0, n_new)
        rb, db = b.read(0, n_new)
        _same_rows(ra, rb, "final rows")
        _same(da, db, "final deletion column")
        new_far = int(np.flatnonzero(layout.apply_moves(np.arange(n_old), moves, n_new, -1) == far)[0])
        assert new_far != far and ra["due"][new_far] == NOW0 + 500 * 10**9  # the column entry went with its object
        sa, sb = a.stats(), b.stats()
        delta = {s: sa["fired_per_stage"][s] - before["fired_per_stage"][s] for s in sa["fired_per_stage"]}
        assert delta == sb["fired_per_stage"] and sum(delta.values()) > 0, (delta, sb["fired_per_stage"])
        assert sa["matched"] - before["matched"] == sb["matched"]
    finally:
        a.close()
        if b is not None:
            b.close()


# ------------------------------------------------------------------ 6: no work, refusals
def test_identity_layout_changes_nothing_but_the_epoch():
    from kwok_amd.host import abi
    from tests import test_gpu_fused_carry as F
    prog, pvars = F._program()
    ptr, moves, new_ptr, _ = _plan("up")
    n = int(ptr[-1])
    eng = F._engine(prog, pvars, F._hash_variants(n), True)
    try:
        for k in range(3):
            eng.step(NOW0 + k * 10**9, SEED, k)
        rows0, dels0 = eng.read(0, n)
        stats0 = eng.stats()
        eng.relayout([(0, 0, 1000), (1000, 1000, n - 1000)], n)
        assert eng.layout_epoch() == 1
        rows1, dels1 = eng.read(0, n)
        _same(rows1, rows0, "rows")
        _same(dels1, dels0, "deletion column")
        assert eng.stats() == stats0
        # refusals change nothing either: each names its run
        for bad, n_new, status, needle in (
                ([(0, 0, n + 1)], n, abi.KWK_EINVAL, "run 0 {dst 0, src 0, n %d}: source beyond" % (n + 1)),
                ([(0, 0, 10), (5, 20, 10)], n, abi.KWK_EINVAL, "run 1 {dst 5, src 20, n 10}: overlaps run 0 in dst"),
                ([(0, 0, 10), (10, 5, 10)], n, abi.KWK_EINVAL, "run 1 {dst 10, src 5, n 10}: overlaps run 0 in src"),
                ([(10, 0, 5), (0, 20, 5)], n, abi.KWK_EINVAL, "run 1 {dst 0, src 20, n 5}: not sorted by dst"),
                ([(0, 0, 10)], n + 1, abi.KWK_EINVAL, "exceeds capacity")):
            with pytest.raises(abi.EngineError) as ei:
                eng.relayout(bad, n_new)
            assert ("(%d)" % status) in str(ei.value) and needle in str(ei.value), str(ei.value)
        assert eng.layout_epoch() == 1 and eng.n == n
        rows2, _ = eng.read(0, n)
        _same(rows2, rows0, "rows after the refusals")
        eng.step(NOW0 + 3 * 10**9, SEED, 3)  # and the engine goes on
        assert len(eng.fired()) > 0
    finally:
        eng.close()


# ------------------------------------------------------------------ 3: usage continuity
U_CPU = np.array([0.0, 0.1, 0.25, 2.0])
U_MEM = np.array([0.0, 64.0 * 2**20, 2.0**30])


def _ukey(nc, cpu, mem):
    return (nc << 28) | (mem << 14) | cpu


def _usage_engine(prog, pvars, pidx, cap, ptr, keys, mixed, ckeys, created, node_created, started):
    from kwok_amd.host import abi, cel
    from kwok_amd.host.engine import Engine, Ingest
    ing = Ingest(prog)
    e = Engine(prog, capacity=cap, state="auto", max_records=max(1, len(ing.records)) + 16)
    e.load_stages()
    e.set_harness(False)
    e.load(*ing.variant_columns(pvars, pidx), ing.record_array())
    ops = np.zeros(3, dtype=abi.USAGE_OP_DTYPE)  # cpu value id 4: pod.SinceSecond() * 0.001
    ops[0] = (cel.OP_LOAD, cel.IN_POD_SINCE, 0.0)
    ops[1] = (cel.OP_CONST, 0, 0.001)
    ops[2] = (cel.OP_MUL, 0, 0.0)
    e.usage_config(ptr, keys, U_CPU, U_MEM, mixed, ckeys, cpu_progs=np.array([[0, 3]], dtype=np.uint32),
                   mem_progs=np.zeros((0, 2), dtype=np.uint32), ops=ops)
    e.usage_pods(True)
    e.metrics_inputs(created, node_created, started, 0.0)
    e.metrics_load([("pod", [(cel.OP_LOAD, cel.IN_POD_CPU)]), ("pod", [(cel.OP_LOAD, cel.IN_POD_CUM_CPU)])])
    return e


def test_usage_continues_across_a_relayout():
    from kwok_amd.host import layout
    from tests import test_gpu_fused_carry as F
    prog, pvars = F._program()
    ptr, moves, new_ptr, node_moves = _plan("up")
    n_old, n_new, nn_old, nn_new = int(ptr[-1]), int(new_ptr[-1]), len(ptr) - 1, len(new_ptr) - 1
    pidx = F._hash_variants(n_old)
    keys = np.array([_ukey(1 + i % 3, i % 4, i % 3) for i in range(n_old)], dtype=np.uint32)
    mixed_slots = [5, 1000, int(ptr[3]) + 2, int(ptr[4]) + 7, n_old - 1]  # in place, shifted, dropped (node 3), shifted, shifted
    for j, s in enumerate(mixed_slots):
        keys[s] = j % 2  # mixed entries 0 and 1
    keys[int(ptr[2]) + 1] = _ukey(1, 4, 1)  # the program pod, in the node that shifts by one
    keys[40] = _ukey(2, 4, 2)               # ... and one that stays in place
    mixed = np.array([0, 2, 2, 3], dtype=np.uint32)
    ckeys = np.array([_ukey(0, 2, 1), _ukey(0, 3, 2), _ukey(0, 1, 1), _ukey(0, 4, 0), _ukey(0, 2, 2)], dtype=np.uint32)
    created = NOW0 - (np.arange(n_old, dtype=np.int64) % 977) * 10**9
    node_created = NOW0 - np.arange(nn_old, dtype=np.int64) * 10**10
    started = np.arange(nn_old, dtype=np.float64) + 1.0
    cap = n_new + 3
    a = _usage_engine(prog, pvars, pidx, cap, ptr, keys, mixed, ckeys, created, node_created, started)
    c = _usage_engine(prog, pvars, pidx, cap, ptr, keys, mixed, ckeys, created, node_created, started)
    fresh_key = _ukey(2, 1, 1)
    try:
        for e in (a, c):
            e.step(NOW0, SEED, 0)  # pods come alive
            e.usage(NOW0 + 10**9)
            e.usage(NOW0 + 3 * 10**9 + 12345)
        _same(a.usage_read_pods(0, n_old), c.usage_read_pods(0, n_old), "per-pod outputs before the relayout")
        ints0 = a.usage_info()["n_integrators"]
        a.relayout(moves, n_new, new_ptr, node_moves, fresh_key)
        info = a.usage_info()
        assert info["n_pods"] == n_new and info["kernel"] == "programs" and info["mixed_pods"] == len(mixed_slots) - 1
        assert info["n_integrators"] == ints0  # ranges stay where they lie; the dropped pod's is abandoned
        for t in (NOW0 + 5 * 10**9, NOW0 + 9 * 10**9 + 777):
            for e in (a, c):
                e.usage(t)
        pa, pc = a.usage_read_pods(0, n_new), c.usage_read_pods(0, n_old)
        want = layout.apply_moves(pc, moves, n_new, 0.0)  # fresh slots are dead: 0
        _same(pa.view(np.uint64), want.view(np.uint64), "per-pod outputs {cpu, mem, cumulative cpu, cumulative mem}")
        covered = layout.apply_moves(np.ones(n_old, dtype=bool), moves, n_new, False)
        assert np.all(pa[~covered] == 0.0) and np.any(pa[covered][:, 2] > 0.0)
        # per-container outputs: A's containers of pod dst are C's of pod src
        ca, cc = a.usage_read_containers(0, n_new), c.usage_read_containers(0, n_old)
        nc_c = c.usage_containers
        nc_a = a.usage_containers
        _same(nc_a, layout.apply_moves(nc_c, moves, n_new, fresh_key >> 28), "containers per pod")
        assert len(ca) == int(nc_a.sum()) and len(cc) == int(nc_c.sum())  # (a dropped mixed pod's range is not read)
        off_a = np.concatenate(([0], np.cumsum(nc_a)))
        off_c = np.concatenate(([0], np.cumsum(nc_c)))
        for m in moves:
            d, s, n = int(m["dst"]), int(m["src"]), int(m["n"])
            _same(ca[off_a[d]:off_a[d + n]].view(np.uint64), cc[off_c[s]:off_c[s + n]].view(np.uint64),
                  f"per-container outputs of run {d} <- {s}")
        assert np.all(ca[off_a[n_new - 1]:] == 0.0)  # a fresh slot's containers
        # pod.Usage / pod.CumulativeUsage Metric values: one series per pod slot, metric by metric
        t = NOW0 + 9 * 10**9 + 777
        ma, mc = a.metrics_eval(t, 0, nn_new).reshape(2, n_new), c.metrics_eval(t, 0, nn_old).reshape(2, n_old)
        for q in range(2):
            got, src = ma[q], layout.apply_moves(mc[q], moves, n_new, np.nan)
            _same(got[covered].view(np.uint64), src[covered].view(np.uint64), f"pod Metric {q}")
            assert np.all(np.isnan(got[~covered]))  # dead slots have no series
        # nodes: moved integrators go on, fresh nodes read 0, sums within the usage tolerance
        (na, cla), (nc_, clc) = a.usage_read(), c.usage_read()
        want_nodes = layout.apply_moves(nc_, node_moves, nn_new, 0.0)
        np.testing.assert_allclose(na, want_nodes, rtol=1e-6, atol=0.0)
        assert np.all(na[nn_new - 2:] == 0.0) and np.all(na[:nn_new - 2, 2] > 0.0)
        gone = slice(int(ptr[3]), int(ptr[4]))
        np.testing.assert_allclose(cla, clc - pc[gone, :2].sum(axis=0), rtol=1e-6)
    finally:
        a.close()
        c.close()


def test_one_byte_usage_keys_survive_or_drop_like_a_fresh_configuration():
    from tests import test_gpu_fused_carry as F
    from kwok_amd.host import layout
    prog, pvars = F._program()
    ptr, moves, new_ptr, node_moves = _plan("down")
    n_old, n_new = int(ptr[-1]), int(new_ptr[-1])
    pidx = F._hash_variants(n_old)
    cpu = np.arange(16, dtype=np.float64) * 0.125
    mem = np.arange(16, dtype=np.float64) * 2.0**20

    def configured(n, node_ptr, keys):
        e = F._engine(prog, pvars, pidx[:n], True)
        e.usage_config(node_ptr, keys, cpu, mem)
        return e

    covered = layout.apply_moves(np.ones(n_old, dtype=bool), moves, n_new, False)
    for distinct, survives in ((254, True), (255, False), (250, None)):
        pool = np.array([_ukey(1, d % 16, d // 16) for d in range(distinct)], dtype=np.uint32)
        keys = pool[np.arange(n_old) % distinct]
        fresh_key = _ukey(3, 15, 15)  # a key nobody has: the 255th or the 256th distinct one
        if survives is None:  # the column comes back: ten further keys live only in the node that is removed
            gone = np.arange(int(ptr[3]), int(ptr[4]))
            keys[gone] = np.array([_ukey(2, d, 15) for d in range(10)], dtype=np.uint32)[gone % 10]
            fresh_key = int(pool[0])
        a = configured(n_old, ptr, keys)
        twin = None
        try:
            if survives is None:
                assert a.usage_info()["kernel"] == "fast32" and a.usage_info()["n_keys8"] == 0
            else:
                assert a.usage_info()["kernel"] == "fast8" and a.usage_info()["n_keys8"] == distinct
            a.step(NOW0, SEED, 0)  # every pod is alive
            a.relayout(moves, n_new, new_ptr, node_moves, fresh_key)
            new_keys = layout.apply_moves(keys, moves, n_new, fresh_key)
            twin = configured(n_new, new_ptr, new_keys)  # freshly configured in the new layout
            ia, it = a.usage_info(), twin.usage_info()
            assert ia["kernel"] == it["kernel"] == ("fast32" if survives is False else "fast8"), (ia, it)
            assert ia["n_keys8"] == it["n_keys8"] == {True: distinct + 1, False: 0, None: distinct}[survives], (ia, it)
            assert ia["max_containers"] == it["max_containers"] == (1 if survives is None else 3) and ia["n_pods"] == n_new
            if survives:  # the checks of a usage engine's layout, through the call itself: each refused by name, nothing changed
                from kwok_amd.host import abi
                ident, nid = [(0, 0, n_new)], [(0, 0, len(new_ptr) - 1)]
                down, short = new_ptr.copy(), new_ptr.copy()
                down[2] = down[1] - 1
                short[-1] -= 1
                for args, needle in (((ident, n_new, down, nid, fresh_key), "node 1: node_ptr must be non-decreasing"),
                                     ((ident, n_new, short, nid, fresh_key), "must equal n_active"),
                                     ((ident, n_new, new_ptr, [(0, 1, len(new_ptr) - 1)], fresh_key), "node run 0"),
                                     ((ident, n_new, new_ptr, nid, 7), "a mixed key"),
                                     ((ident, n_new, new_ptr, nid, _ukey(1, 16, 0)), "value id outside the tables"),
                                     ((ident, n_new, None, None, fresh_key), "node_ptr is null")):
                    with pytest.raises(abi.EngineError) as ei:
                        a.relayout(*args)
                    assert ("(%d)" % abi.KWK_EINVAL) in str(ei.value) and needle in str(ei.value), str(ei.value)
                assert a.layout_epoch() == 1 and a.usage_info() == ia
            a.usage(NOW0 + 10**9)
            node, cluster = a.usage_read()
            pod_cpu = np.where(covered, cpu[new_keys & 0x3FFF] * (new_keys >> 28), 0.0)  # fresh slots are dead
            pod_mem = np.where(covered, mem[(new_keys >> 14) & 0x3FFF] * (new_keys >> 28), 0.0)
            edges = new_ptr.astype(np.int64)
            want = np.array([[pod_cpu[edges[j]:edges[j + 1]].sum(), pod_mem[edges[j]:edges[j + 1]].sum()]
                             for j in range(len(edges) - 1)])
            np.testing.assert_allclose(node[:, :2], want, rtol=1e-6)
            np.testing.assert_allclose(cluster, want.sum(axis=0), rtol=1e-6)
            assert np.all(node[-2:] == 0.0) and cluster[0] > 0.0  # fresh nodes
        finally:
            a.close()
            if twin is not None:
                twin.close()


# ------------------------------------------------------------------ 4: leases
def test_lease_records_travel_with_their_nodes():
    from kwok_amd.host import abi, layout
    from kwok_amd.host.engine import Engine, Ingest
    ptr, moves, new_ptr, _ = _plan("down")  # node slots here: the same runs
    n_old, n_new = int(ptr[-1]), int(new_ptr[-1])
    prog, nvars, idx, _, salt, _ = _node_heartbeat(n_old)
    cap = n_old + 3
    ing = Ingest(prog)
    cols = ing.variant_columns(nvars, idx)
    leases = np.zeros(n_old, dtype=abi.LEASE_DTYPE)
    leases["flags"] = abi.LEASE_HOLD | abi.LEASE_QUEUED
    leases["next_try_ns"] = NOW0 + (np.arange(n_old) % 7) * 10**9
    other = np.arange(n_old) % 5 == 0  # held by another holder, some expired
    leases["flags"][other] |= abi.LEASE_EXISTS | abi.LEASE_HOLDER | abi.LEASE_DURATION | abi.LEASE_RENEW
    leases["holder"][other] = 9
    leases["duration_s"][other] = 40
    leases["renew_ns"][other] = NOW0 - (np.arange(n_old)[other] % 90) * 10**9

    def engine():
        e = Engine(prog, capacity=cap, kind_salt=salt)
        e.load_stages()
        e.lease_config(holder_id=1, lease_duration_s=40)
        return e

    a, b = engine(), None
    try:
        a.load(*cols, ing.record_array())
        a.lease_set(leases)
        for k in range(2):
            a.lease_step(NOW0 + k * 10**9, SEED, k)
            a.step(NOW0 + k * 10**9, SEED, k)
        l0 = a.lease_read(0, n_old)
        rows0, dels0 = a.read(0, n_old)
        a.relayout(moves, n_new)
        want_l = layout.apply_moves(l0, moves, n_new, np.zeros(1, dtype=abi.LEASE_DTYPE)[0])
        _same(a.lease_read(0, n_new), want_l, "lease records right after the relayout")
        b = engine()
        want_rows = layout.apply_moves(rows0, moves, n_new, np.zeros(1, dtype=abi.HOT_DTYPE)[0])
        b.load(want_rows, layout.apply_moves(dels0, moves, n_new, abi.DEL_ABSENT), layout.apply_moves(cols[2], moves, n_new, 0),
               (want_rows["sched"] >> np.uint32(16)).astype(np.uint16), ing.record_array())
        b.lease_set(want_l)
        for k in range(2, 9):  # the renew interval's jitter is drawn by the new slot in both
            for e in (a, b):
                e.lease_step(NOW0 + k * 10**9, SEED, k)
            oa, ob = np.sort(a.lease_ops(), order=["slot", "stage"]), np.sort(b.lease_ops(), order=["slot", "stage"])
            _same(oa, ob, f"lease ops of step {k}")
            for e in (a, b):
                e.step(NOW0 + k * 10**9, SEED, k)
            _same(_sorted_fired(a), _sorted_fired(b), f"fired list of step {k}")
        _same(a.lease_read(0, n_new), b.lease_read(0, n_new), "lease records")
        _same_rows(a.read(0, n_new)[0], b.read(0, n_new)[0], "node rows")
    finally:
        a.close()
        if b is not None:
            b.close()


# ------------------------------------------------------------------ 4b: the pods of relayouted nodes
def test_lease_sync_marks_the_same_pods_as_a_twin_in_the_new_layout():
    """A node engine with leases and its pod engine are both relayouted (the node slots by the node
    runs, the pod slots by the slot runs); the next lease step and kwk_lease_sync_pods with the new
    node_ptr leave the pods' MANAGED / DIRTY marks, and the next step's fired list, equal to those
    of twin engines loaded in the new layout."""
    from kwok_amd.host import abi, layout
    from kwok_amd.host.engine import Engine, Ingest
    from tests import test_gpu_fused_carry as F
    ptr, moves, new_ptr, node_moves = _plan("up")
    n_old, n_new, nn_old, nn_new = int(ptr[-1]), int(new_ptr[-1]), len(ptr) - 1, len(new_ptr) - 1
    nprog, nvars, nidx, _, salt, _ = _node_heartbeat(nn_old)
    ning = Ingest(nprog)
    ncols = ning.variant_columns(nvars, nidx)
    leases = np.zeros(nn_old, dtype=abi.LEASE_DTYPE)
    leases["flags"] = abi.LEASE_HOLD | abi.LEASE_QUEUED
    leases["next_try_ns"] = NOW0 + 10**9  # every node's sync is due at the step after the relayout
    for j in (1, 4):  # held by another holder, not expired: these nodes' pods lose MANAGED
        leases["flags"][j] |= abi.LEASE_EXISTS | abi.LEASE_HOLDER | abi.LEASE_DURATION | abi.LEASE_RENEW
        leases["holder"][j], leases["duration_s"][j], leases["renew_ns"][j] = 9, 40, NOW0
    pprog, pvars = F._program()
    pidx = F._hash_variants(n_old)
    ping = Ingest(pprog)
    pcols = ping.variant_columns(pvars, pidx)

    def node_engine():
        e = Engine(nprog, capacity=nn_new + 2, kind_salt=salt)
        e.load_stages()
        e.lease_config(holder_id=1, lease_duration_s=40)
        return e

    def pod_engine():
        e = Engine(pprog, capacity=max(n_old, n_new) + 5, state="auto", max_records=max(1, len(ping.records)) + 16)
        e.load_stages()
        e.set_harness(True)
        return e

    engines = []
    try:
        na, pa = node_engine(), pod_engine()
        engines += [na, pa]
        na.load(*ncols, ning.record_array())
        na.lease_set(leases)
        pa.load(*pcols, ping.record_array())
        na.step(NOW0, SEED, 0)
        pa.step(NOW0, SEED, 0)
        nrows0, ndels0 = na.read(0, nn_old)
        l0 = na.lease_read(0, nn_old)
        prows0, pdels0 = pa.read(0, n_old)
        na.relayout(node_moves, nn_new)   # node slots: the node runs
        pa.relayout(moves, n_new)         # pod slots: the slot runs
        zero = np.zeros(1, dtype=abi.HOT_DTYPE)[0]
        nb, pb = node_engine(), pod_engine()
        engines += [nb, pb]
        nrows = layout.apply_moves(nrows0, node_moves, nn_new, zero)
        nb.load(nrows, layout.apply_moves(ndels0, node_moves, nn_new, abi.DEL_ABSENT),
                layout.apply_moves(ncols[2], node_moves, nn_new, 0), (nrows["sched"] >> np.uint32(16)).astype(np.uint16),
                ning.record_array())
        nb.lease_set(layout.apply_moves(l0, node_moves, nn_new, np.zeros(1, dtype=abi.LEASE_DTYPE)[0]))
        prows = layout.apply_moves(prows0, moves, n_new, zero)
        pb.load(prows, layout.apply_moves(pdels0, moves, n_new, abi.DEL_ABSENT), layout.apply_moves(pcols[2], moves, n_new, 0),
                (prows["sched"] >> np.uint32(16)).astype(np.uint16), ping.record_array())
        now = NOW0 + 10**9
        for nodes, pods in ((na, pa), (nb, pb)):
            nodes.lease_step(now, SEED, 1)
            nodes.lease_sync_pods(pods, new_ptr)
        ra, rb = pa.read(0, n_new)[0], pb.read(0, n_new)[0]
        _same_rows(ra, rb, "pod rows after kwk_lease_sync_pods")
        managed = (ra["sched"] & abi.F_MANAGED) != 0
        node_of = np.repeat(np.arange(nn_new), np.diff(new_ptr.astype(np.int64)))
        covered = layout.apply_moves(np.ones(n_old, dtype=bool), moves, n_new, False)
        # old node 1 is new node 1, old node 4 is new node 3: their pods are not managed any more, the others' are
        assert not managed[covered & np.isin(node_of, (1, 3))].any() and managed[covered & ~np.isin(node_of, (1, 3))].all()
        _same(np.sort(na.lease_ops(), order=["slot", "stage"]), np.sort(nb.lease_ops(), order=["slot", "stage"]), "lease ops")
        for e in (pa, pb):
            e.step(now, SEED, 1)
        _same(_sorted_fired(pa), _sorted_fired(pb), "pods' fired list after the sync")
        _same_rows(pa.read(0, n_new)[0], pb.read(0, n_new)[0], "pod rows after the step")
    finally:
        for e in engines:
            e.close()


# ------------------------------------------------------------------ 5: the libraries with per-slot state of their own
def _expo_cluster():
    from kwok_amd import workload as W
    from kwok_amd.host import layout
    per = [3, 40, 5, 6]
    cl = W.make_cluster("C4", len(per), sum(per), seed=9)
    pods, nodes = cl.pods.materialize(), cl.nodes.materialize()
    ptr = np.concatenate([[0], np.cumsum(per)]).astype(np.uint32)
    # node 1 grows by a slot, node 2 goes, a node of 2 slots is appended
    moves, new_ptr, node_moves = layout.plan_layout(ptr, room=[3, 41, 5, 6], removed_nodes=[2], added_nodes=[2])
    return cl, pods, nodes, ptr, moves, new_ptr, node_moves


def test_exposition_writer_is_for_one_layout():
    """After a kwk_relayout the old writer's calls return KWK_ESTATE naming the call to make (its node
    count and row places are the old layout's); a writer created for the new layout, with
    kwk_expo_set_labels of the moved objects and kwk_expo_commit, writes the text of a fresh writer over
    a twin engine loaded in the new layout."""
    from kwok_amd.host import abi, layout
    from kwok_amd.host.expo import ExpoError, Exposition
    from tests import test_gpu_expo as X
    cl, pods, nodes, ptr, moves, new_ptr, node_moves = _expo_cluster()
    n_old, n_new = len(pods), int(new_ptr[-1])
    rig = X.Rig(cl, pods, nodes, ptr)
    ex2 = rig2 = None
    try:
        t = NOW0
        rig.eng.usage(t)
        assert len(rig.ex.scrape(t, 0, len(nodes))) == len(nodes)
        keys = np.asarray(rig.eng._uargs[1])
        fresh_key = int(keys[(keys >> 28) != 0][0])
        rig.eng.relayout(moves, n_new, new_ptr, node_moves, fresh_key)
        assert np.array_equal(rig.eng._uargs[0], new_ptr) and len(rig.eng._uargs[1]) == n_new
        for call in (lambda: rig.ex.scrape(t, 0, 1), rig.ex.commit_rows, rig.ex.commit, lambda: rig.ex.set_nodes(nodes)):
            with pytest.raises(ExpoError, match="kwk_relayout.*kwk_expo_create") as ei:
                call()
            assert ei.value.status == abi.KWK_ESTATE
        nodes_new = [nodes[0], nodes[1], nodes[3], nodes[2]]  # (the appended node: an object of its own)
        src_of = layout.apply_moves(np.arange(n_old), moves, n_new, -1)
        pods_new = [pods[int(s)] if s >= 0 else None for s in src_of]
        assert sum(p is None for p in pods_new) == 3 and n_new == 52
        ex2 = Exposition(rig.eng, rig.mp.native)
        assert ex2.n_nodes == len(nodes_new)
        ex2.set_nodes(nodes_new)
        ex2.set_pods(pods_new, 0, nodes_new)
        ex2.commit()
        rig.eng.usage(t)
        text = ex2.scrape(t, 0, len(nodes_new))
        # the twin: loaded in the new layout (a stand-in object in the fresh slots, deleted), a fresh writer
        rig2 = X.Rig(cl, [p if p is not None else pods[0] for p in pods_new], nodes_new, new_ptr, label_pods=pods_new)
        rig2.delete([i for i, p in enumerate(pods_new) if p is None])
        rig2.eng.usage(t)
        want = rig2.ex.scrape(t, 0, len(nodes_new))
        assert text == want and len(text) == 4 and all(len(x) > 0 for x in text[:3])
    finally:
        if ex2 is not None:
            ex2.close()
        if rig2 is not None:
            rig2.close()
        rig.close()


def test_emitter_is_for_one_layout():
    """An emitter's words and columns are per slot: after a kwk_relayout kwk_emit and kwk_emit_step
    return KWK_ESTATE naming the call to make, its words stay readable (a guard bit set by an earlier
    emission is the device's own), and an emitter created for the new layout from the permuted words
    and columns emits again."""
    from kwok_amd.host import abi, emit, layout
    from kwok_amd.host.patchtpl import PatchProgram
    from tests import test_gpu_expo as X
    cl, pods, nodes, ptr, moves, new_ptr, node_moves = _expo_cluster()
    n_old, n_new = len(pods), int(new_ptr[-1])
    rig = X.Rig(cl, pods, nodes, ptr)
    em = em2 = None
    try:
        prog = rig.eng.p
        classes = [prog.class_of(o, register=False) for o in pods]
        pp = PatchProgram(prog.stages, {"NodeIPWith": lambda *a: "10.100.100.100", "PodIPWith": lambda *a: "11.100.100.100"})
        ep = emit.EmitProgram(prog.stages, pp, dict(zip(classes, pods)), len(prog.class_ids), stride=16)
        em = emit.Emitter(rig.eng, n_old, ep)
        words, cols = ep.rows(pods, classes)
        em.set_rows(0, words, cols)
        rig.eng.step(NOW0, 7, 0)
        rig.eng.fired_compact(packed=True)
        em.run(NOW0, packed=True)
        dev_words = em.words(0, n_old)
        assert em.result()[0] > 0
        keys = np.asarray(rig.eng._uargs[1])
        rig.eng.relayout(moves, n_new, new_ptr, node_moves, int(keys[(keys >> 28) != 0][0]))
        rig.eng.step(NOW0 + 10**9, 7, 1)
        rig.eng.fired_compact(packed=True)
        for call in (lambda: em.emit(NOW0 + 10**9, packed=True), lambda: em.emit_step(1, NOW0 + 10**9)):
            with pytest.raises(abi.EngineError, match=r"\(%d\).*kwk_relayout.*kwk_emitter_create" % abi.KWK_ESTATE):
                call()
        _same(em.words(0, n_old), dev_words, "the old emitter's words stay readable")
        em2 = emit.Emitter(rig.eng, n_new, ep)
        new_words = layout.apply_moves(dev_words, moves, n_new, 0)
        em2.set_rows(0, new_words, {c: layout.apply_moves(col, moves, n_new, 0) for c, col in cols.items()})
        em2.run(NOW0 + 10**9, packed=True)
        ni, nb = em2.result()
        fired = rig.eng.fired()
        assert ni <= len(fired) and (ni > 0) == (nb > 0)
    finally:
        for e in (em, em2):
            if e is not None:
                e.close()
        rig.close()

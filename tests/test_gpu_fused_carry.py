"""Fused launches of the 1-byte sweep carry work items through their steps in registers
(`sweep8_kernel<..., kSteps>`): a wave whose tile holds no queued id and at most
2048 / kSteps items builds its work list once and takes every batch through all the launch's steps;
an idle tile skips the later steps; every other tile (a queued id, more items) rebuilds its list at
each step as before.  Small engines (<= 5 tiles, the last one partial), pod-fast with the bench
harness, the Job-owned variant placed by slot so that each 2048-slot wave region's item count is
known: after a per-step warm-up the plain pods idle in Running and every Job-owned pod is one item
per step.

Every case steps a fused engine (kwk_step_n in groups of 4 and 2, every step's list fetched from
the hand-back ring) and a twin with KWK_TUNE_FUSE_STEPS 0 (kwk_step + kwk_fired_compact per step):
the state columns, every step's 2-byte records and per-segment counts as ordered arrays, the fired /
matched / per-stage / step counts, and bytes = the twin's minus (m - 1) * n per group of m steps
(only a launch's first step counts the id reads).  One case checks every step against `OracleSim`.
The per-step twin and the oracle decide every expected value."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NOW0, DT, SEED = 1_700_000_000 * 10**9, 10**9, 0x6B776F6B
WARM = 3                 # per-step warm-up: plain pods fire pod-ready, re-match, then idle
GROUPS = (4, 4, 2, 2)    # the fused engine's kwk_step_n calls after the warm-up
N_BIG = 5 * 8192 - 2048 - 777  # 5 tiles; the last: two whole wave regions, 1271 ids of the third, none of the fourth


def _program():
    from kwok_amd import workload as W
    from kwok_amd.host.compiler import HarnessSpec, KindProgram
    from kwok_amd.host.stages import load_stage_files
    pvars = [W.pod_object("p", "n"), W.pod_object("p", "n", job=True)]
    prog = KindProgram(load_stage_files(*W.stage_paths(W.POD_FAST)), HarnessSpec())
    prog.explore(pvars)
    return prog, pvars


def _hash_variants(n):
    from bench import shard_pod_variants
    return shard_pod_variants(0, n, SEED, 0.1)


def _region_variants(counts, tail=0):
    """Variant per slot: region r (2048 slots) holds counts[r] Job-owned pods at seeded random slots;
    `tail` further slots with ~10 % Job-owned."""
    rng = np.random.default_rng(5)
    idx = np.zeros(2048 * len(counts) + tail, dtype=np.int32)
    for r, c in enumerate(counts):
        idx[2048 * r + rng.choice(2048, c, replace=False)] = 1
    idx[2048 * len(counts):] = rng.random(tail) < 0.1
    return idx


def _engine(prog, pvars, pidx, fuse, queued=None):
    """queued: (slots, stage, due): those pods are loaded clean with `stage` queued for `due`."""
    from kwok_amd.host import abi
    from kwok_amd.host.engine import Engine, Ingest
    ing = Ingest(prog)
    hot, dels, rec, cls = ing.variant_columns(pvars, pidx)
    if queued is not None:
        slots, stage, due = queued
        hot["sched"][slots] = (hot["sched"][slots] & ~np.uint32(0xFF | abi.F_DIRTY)) | np.uint32(stage)
        hot["due"][slots] = due
    eng = Engine(prog, capacity=len(pidx), state="auto", max_records=max(1, len(ing.records)) + 16)
    if not fuse:
        eng.set_tuning(abi.TUNE_FUSE_STEPS, 0)
    eng.load_stages()
    eng.set_harness(True)
    eng.load(hot, dels, rec, cls, ing.record_array())
    assert eng.stats()["state_bytes"] == 1
    return eng


def _run(pidx, warm=WARM, groups=GROUPS, queued=None, sim=None, expect_min_fired=1):
    """The fused engine against the per-step twin (and `sim`, an OracleSim over sim.slots, at every
    step).  Returns each step's (records, segment counts) of the twin."""
    from kwok_amd.host import abi
    from kwok_amd.host.engine import PinnedBuffer
    prog, pvars = _program()
    n = len(pidx)
    ref, f = _engine(prog, pvars, pidx, False, queued), _engine(prog, pvars, pidx, True, queued)
    bufs = [(PinnedBuffer(2 * n + 64), PinnedBuffer(4 * (n // 2048 + 64))) for _ in range(max(groups))]
    sample = None if sim is None else np.asarray(sim.slots, dtype=np.int64)

    def oracle_step(k, recs, segc, rs):
        slot, stage, flags = abi.fired16_decode(recs, segc, rs)
        sel = np.isin(slot.astype(np.int64), sample)
        got = sorted(zip(slot[sel].tolist(), stage[sel].tolist(), flags[sel].tolist()))
        exp = sorted(sim.step(NOW0 + k * DT, SEED, k))
        assert got == exp, f"step {k}: device-only {sorted(set(got) - set(exp))[:6]} oracle-only " \
                           f"{sorted(set(exp) - set(got))[:6]}"

    try:
        for k in range(warm):
            for e in (ref, f):
                e.step(NOW0 + k * DT, SEED, k)
                e.fired_compact("16")
            if sim is not None:
                oracle_step(k, *f.fired_packed16())
        st0 = {id(e): e.stats() for e in (ref, f)}
        f.fired_keep(16)
        lists = []
        k = warm
        for m in groups:
            exp = []
            for j in range(m):
                ref.step(NOW0 + (k + j) * DT, SEED, k + j)
                ref.fired_compact("16")
                exp.append(ref.fired_packed16())
            f.step_n(m, NOW0 + k * DT, DT, SEED, k, "packed16")
            info = f.last_sweep()
            assert info["kernel"] == abi.SWEEP_8 and info["steps"] == m, info
            infos = [f.fetch_step(k + j, *bufs[j]) for j in range(m)]
            f.fetch_wait()
            for j, fi in enumerate(infos):
                recs, segc, rs = exp[j]
                out, cnt = bufs[j]
                assert fi["step"] == k + j and fi["format"] == abi.COMPACT_PACKED16 and fi["region_slots"] == rs
                assert fi["n_records"] == len(recs) and fi["n_segs"] == len(segc), (k + j, fi, len(recs))
                got_r, got_c = out.array(np.uint16, fi["n_records"]).copy(), cnt.array(np.uint32, fi["n_segs"]).copy()
                assert np.array_equal(got_c, segc), f"step {k + j}: segment counts"
                assert np.array_equal(got_r, recs), f"step {k + j}: records"
                if sim is not None:
                    oracle_step(k + j, got_r, got_c, fi["region_slots"])
                lists.append((recs, segc))
            k += m
        (r_hot, r_del), (f_hot, f_del) = ref.read(), f.read()
        for col in ("pred", "sched"):
            assert np.array_equal(f_hot[col], r_hot[col]), col
        pend = (r_hot["sched"] & 0xFF) != 0xFF
        assert np.array_equal(f_hot["due"][pend], r_hot["due"][pend])
        assert np.array_equal(f_del, r_del)
        rs, fs = ref.stats(), f.stats()
        for key in ("fired", "matched", "fired_per_stage", "steps"):
            assert fs[key] == rs[key], (key, fs[key], rs[key])
        saved = sum(m - 1 for m in groups) * n
        assert fs["bytes"] - st0[id(f)]["bytes"] == rs["bytes"] - st0[id(ref)]["bytes"] - saved
        assert sum(len(r) for r, _ in lists) >= expect_min_fired
        if sim is not None:
            from tests.parity_util import compare_state
            idx = np.asarray(sim.slots, dtype=np.int64)
            compare_state(prog, f, sim, k - 1, rows=(f_hot[idx], f_del[idx]))
        return lists
    finally:
        for e in (ref, f):
            e.close()
        for x in bufs:
            for p in x:
                p.close()


def _queued(pidx):
    """A few pods of both variants with pod-ready queued, inside region 0 (otherwise carried) and in
    the partial last tile: due between the 2nd and 3rd step of each 4-step group and of no step of it
    (after its last: the next group's first step), at the 2nd step of a 2-step group and after it."""
    prog, _ = _program()
    n = len(pidx)
    slots = np.array([5, 6, 300, 301, 1023, 1024, 2047, n - 1, n - 2, n - 700, n - 701, n - 1270], dtype=np.int64)
    assert (pidx[slots] == 1).any() and (pidx[slots] == 0).any()
    at = np.array([4.5, 6.5, 8.5, 10.5, 11.5, 12.5, 13.5, 4.5, 6.5, 11.5, 14.5, 8.5])  # in steps: WARM = 3, GROUPS
    due = NOW0 + (at * DT).astype(np.int64)
    return slots, prog.names.index("pod-ready"), due


def test_steady_state_carried():
    """(a) ~10 % cycling pods per wave region (≈ 205 items): the carried path, 4- and 2-step groups,
    the partial last tile and its wave region past the end."""
    lists = _run(_hash_variants(N_BIG))
    n_job = int(_hash_variants(N_BIG).sum())
    assert all(len(r) == n_job for r, _ in lists)  # every Job-owned pod is one item (and record) per step


def test_both_sides_of_the_cap():
    """(b) wave regions with exactly 512 / 513 cycling pods (the 4-step cap) and 1024 / 1025 (the
    2-step cap): carried and rebuilt lists side by side in one tile."""
    pidx = _region_variants([512, 513, 1024, 1025, 511, 1023], tail=900)
    lists = _run(pidx)
    assert all(len(r) == int(pidx.sum()) for r, _ in lists)


def test_first_group_from_the_loaded_state():
    """(c) no warm-up: 2048 items per wave at the first step (every list rebuilt), the plain pods
    leaving the list after their second step; the second group starts carried while the Job-owned
    pods go on."""
    _run(_hash_variants(N_BIG), warm=0, groups=(4, 4, 2))


def test_idle_region_between_working_ones():
    """(d) a wave region without work between working ones, an idle tile's worth of them, and the
    partial region."""
    _run(_region_variants([200, 0, 210, 190, 0, 0, 0, 0, 3], tail=100))


def test_queued_ids_take_the_due_test_at_each_step():
    """(e) pods loaded with a stage queued: their tiles rebuild the list at every step, and each fires
    at the first step whose own `now` reaches its due time."""
    pidx = _hash_variants(N_BIG)
    pidx[[5, 300, 1023, N_BIG - 1, N_BIG - 700]] = 1
    pidx[[6, 301, 1024, N_BIG - 2, N_BIG - 701]] = 0
    _run(pidx, queued=_queued(pidx))


def test_carried_and_queued_against_the_oracle():
    """(f) (a) + (e) at every step against OracleSim: every 37th slot and the queued pods."""
    from oracle.next_ref import load_stage_docs
    from oracle.sim import OracleSim
    from kwok_amd import workload as W
    n = 2 * 8192 + 2048 + 1271
    pidx = _hash_variants(n)
    pidx[[5, 300, 1023, n - 1, n - 700]] = 1
    pidx[[6, 301, 1024, n - 2, n - 701]] = 0
    q_slots, stage, due = _queued(pidx)
    _, pvars = _program()
    slots = sorted(set(range(3, n, 37)) | set(q_slots.tolist()))
    sim = OracleSim(load_stage_docs(*W.stage_paths(W.POD_FAST)), [pvars[int(pidx[s])] for s in slots], harness=True,
                    slots=slots)
    at = dict(zip(q_slots.tolist(), due.tolist()))
    for i, s in enumerate(slots):
        if s in at:
            sim.dirty[i], sim.pending[i], sim.due[i] = False, stage, at[s]
    _run(pidx, queued=(q_slots, stage, due), sim=sim)

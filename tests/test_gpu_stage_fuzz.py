"""The generated Stage sets of tests/stage_fuzz.py through the engine, against OracleSim bit for
bit: the tables a Stage set compiles to decide the state format and the sweep kernel (1-byte ids,
2-byte words with or without the transition table, 4-byte words, the fused 8-byte record, wide
8-byte state; delayed stages take the due paths, more than 4 stages leave the 1-byte sweep's
scalar per-stage counters), and kwok's shipped sets reach few of those combinations.

Every corpus case runs in every state format its program admits, 12 steps on a clock with 1 s
steps, a 35 s jump, a step backwards and a jump past the 60 s delays; every third case with a
non-zero kind_salt and a slot_base past 2^32.  Each step's fired list (slot, stage, flags) and
every object's row (alive, pending stage, due time in ns, feature bits, deletion column, dirty
flag) must equal the oracle's; so must kwk_stats' totals.  Everything compared is an integer:
there is no tolerance.  Cases whose deltas depend on the pre-state (KWK_DELTA_UNKNOWN) run through
KindController, as tests/test_delta_unknown.py; loops=False cases also from the native compiler
and encoder.

The boundary tests tile one case per state format to 2.5 sweep tiles plus a ragged remainder and
check a sample of slots (tile, wave and 64-slot boundaries, slot N-1) exactly, the others for
firing at most once per step, through kwk_step and through kwk_step_n + kwk_fired_fetch.

Three cases also run with the churn harness: HarnessSpec() compiles for the generated kind
(`Failed` is in its phase vocabulary)."""
import numpy as np
import pytest

from kwok_amd.host import abi
from tests import stage_fuzz as F

pytestmark = pytest.mark.gpu

FORCED_KERNEL = {"wide": abi.SWEEP_W8, "u32": abi.SWEEP_W4, "dw": abi.SWEEP_WD,
                 "u16-notable": abi.SWEEP_16, "u16-general": abi.SWEEP_16}
STATE_BYTES = {"wide": {8}, "u32": {4}, "dw": {8}, "u16": {2}, "u16-notable": {2}, "u16-general": {2}, "auto": {1, 2}}


# "auto" on these is the 1-byte dictionary format: no state has two candidate stages (no Philox
# pick), no jitter, no value record, no deletion column, so no transition is general
BYTE_CASES = {"b8-chain-4", "b8-chain-6", "b8-chain-delay"}
BYTE_STATE = {1}


def formats_of(prog):
    """The state formats a program admits (make_fmt in engine.hip)."""
    w = F.word_bits(prog)
    out = ["wide"]
    if w <= 32:
        out.append("u32")
    if w <= 28:
        out.append("dw")
    if w <= 16:
        out += ["u16", "auto", "u16-notable", "u16-general"]
    return out


@pytest.fixture(scope="module")
def compiled():
    """name -> (KindProgram, Ingest, columns, expected rows per step): compiled and encoded once."""
    from kwok_amd.host.engine import Ingest
    cache = {}

    def get(name, harness=False):
        if (name, harness) not in cache:
            docs, objs = F.case(name)
            kp = F.compile_python(docs, objs, harness)
            ing = Ingest(kp)
            cols = ing.columns(objs)
            cache[name, harness] = (kp, ing, cols, F.expected_rows(F.oracle_run(name, harness), kp.describe()))
        return cache[name, harness]

    return get


def make_engine(prog, cols, records, fmt, capacity, kind_salt=0, slot_base=0):
    from kwok_amd.host.engine import Engine
    state = {"u16-notable": "u16", "u16-general": "u16"}.get(fmt, fmt)
    eng = Engine(prog, capacity=capacity, kind_salt=kind_salt, slot_base=slot_base, state=state,
                 max_records=max(1 << 12, len(records) + 16))
    if fmt == "u16-notable":
        eng.set_tuning(abi.TUNE_SWEEP16, abi.sweep16_shape(table=0))
    elif fmt == "u16-general":
        eng.set_tuning(abi.TUNE_SWEEP16, abi.sweep16_shape(kernel=0))
    eng.load_stages()
    eng.load(*cols, records)
    return eng


def check_rows(what, prog, rows, exp, applied):
    hot, dels = rows
    alive, stage, due, pred, dele, dirty = exp
    sched = hot["sched"].astype(np.int64)
    got_alive = (sched & abi.F_ALIVE) != 0
    assert np.array_equal(got_alive, alive), (what, "alive", np.flatnonzero(got_alive != alive)[:8])
    a = alive
    st = sched & 0xFF
    bad = np.flatnonzero(a & (st != stage))
    assert not len(bad), (what, "stage", [(int(i), int(st[i]), int(stage[i])) for i in bad[:8]])
    pend = a & (stage != 0xFF)
    d = hot["due"].astype(np.int64)
    bad = np.flatnonzero(pend & (d != due))
    assert not len(bad), (what, "due", [(int(i), int(d[i]), int(due[i])) for i in bad[:8]])
    p = hot["pred"].astype(np.int64) & ~applied  # the applied bits are checked through the REMATCH flag
    bad = np.flatnonzero(a & (p != pred))
    assert not len(bad), (what, "pred", [(int(i), hex(int(p[i])), hex(int(pred[i]))) for i in bad[:8]])
    if prog.uses_deletion_column:
        bad = np.flatnonzero(a & (dels != dele))
        assert not len(bad), (what, "deletion", [(int(i), int(dels[i]), int(dele[i])) for i in bad[:8]])
    got_dirty = (sched & abi.F_DIRTY) != 0
    bad = np.flatnonzero(a & (got_dirty != dirty))
    assert not len(bad), (what, "dirty", [(int(i), bool(got_dirty[i])) for i in bad[:8]])


def triples(rec, mask=0):
    return sorted((int(r["slot"]), int(r["stage"]), int(r["flags"]) & ~mask) for r in rec)


def run_engine(name, fmt, prog, cols, records, expected, controller=None, harness=False):
    """One engine over the case's clock against the cached oracle run."""
    run = F.oracle_run(name, harness)
    rp = F.run_params(name)
    n = len(cols[0])
    applied = sum(1 << b for b in prog.applied_bits.values())
    eng = make_engine(prog, cols, records, fmt, n, **rp)
    ctl = controller(eng) if controller is not None else None
    try:
        for k, now in enumerate(F.NOWS):
            what = (name, fmt, "step", k)
            if ctl is not None:
                got = triples(ctl.step(now, F.RUN_SEED, k), abi.FIRED_DELTA_UNKNOWN)
            else:
                eng.step(now, F.RUN_SEED, k)
                got = triples(eng.fired())
            if fmt in FORCED_KERNEL:
                assert eng.last_sweep()["kernel"] == FORCED_KERNEL[fmt], (what, eng.last_sweep())
            assert eng.last_sweep()["harness"] == int(harness), (what, eng.last_sweep())
            exp = run.steps[k].fired
            assert got == exp, (what, "device-only", sorted(set(got) - set(exp))[:8], "oracle-only",
                                sorted(set(exp) - set(got))[:8])
            check_rows(what, prog, eng.read(), expected[k], applied)
            if ctl is not None:
                assert ctl.objs == run.steps[k].objs, (what, "host cache != oracle objects")
        st = eng.stats()
        want_bytes = BYTE_STATE if fmt == "auto" and name in BYTE_CASES and not harness else STATE_BYTES[fmt]
        assert st["state_bytes"] in want_bytes, (name, fmt, st["state_bytes"])
        if fmt in ("u16", "auto"):
            want = {abi.SWEEP_8} if st["state_bytes"] == 1 else {abi.SWEEP_16, abi.SWEEP_16_FSM}
            assert eng.last_sweep()["kernel"] in want, (name, fmt, eng.last_sweep())
        assert st["fired"] == run.total, (name, fmt)
        assert [st["fired_per_stage"][s] for s in prog.names] == run.per_stage, (name, fmt)
        return st["state_bytes"], eng.last_sweep()["kernel"]
    finally:
        eng.close()


@pytest.mark.parametrize("name", F.CASE_IDS)
def test_engine_equals_oracle(name, compiled):
    """Every state format the case's program admits; delta-conflict cases through KindController."""
    kp, ing, cols, expected = compiled(name)
    _, objs = F.case(name)
    controller = None
    if kp.delta_conflicts:
        from kwok_amd.host.controller import KindController
        controller = lambda eng: KindController(kp, eng, ing, objs)  # noqa: E731
    ran = []
    for fmt in formats_of(kp):
        ran.append((fmt,) + run_engine(name, fmt, kp, cols, ing.record_array(), expected, controller))
    print(name, "word bits", F.word_bits(kp), "(format, state bytes, kernel):", ran)


@pytest.mark.parametrize("name", F.HARNESS_CASES)
def test_engine_with_churn_harness(name, compiled):
    """HarnessSpec() compiles for the generated kind: the harness variants of the sweeps (terminal
    objects deleted, deleted ones re-created from their spec) in every format the program admits."""
    kp, ing, cols, expected = compiled(name, True)
    assert sum(F.oracle_run(name, True).sim.gen) > 0  # objects were re-created
    for fmt in formats_of(kp):
        run_engine(name, fmt, kp, cols, ing.record_array(), expected, harness=True)


@pytest.mark.parametrize("name", [n for n in F.CASE_IDS if not F.LOOPS[n]])
def test_engine_from_native_compiler(name, compiled):
    """The Go host's path: tables from libkwok_compiler, rows from libkwok_encoder, no Python
    compiler; in the narrowest format and in the 8-byte one."""
    from kwok_amd.host.encoder import NativeIngest
    kp, _, _, expected = compiled(name)
    docs, objs = F.case(name)
    nat = F.compile_native(docs, objs)
    ni = NativeIngest(nat)
    try:
        cols = ni.columns(objs)
        records = ni.record_array()
        w = F.word_bits(nat)
        narrowest = "auto" if w <= 16 else "dw" if w <= 28 else "u32" if w <= 32 else "wide"
        for fmt in sorted({narrowest, "wide"}):
            run_engine(name, fmt, nat, cols, records, expected)
    finally:
        ni.close()
        nat.close()


# ---------------------------------------------------------------------------------------------
BOUNDARY = {"byte-4stages": ("auto", "b8-chain-4"), "byte-6stages": ("auto", "b8-chain-6"),
            "byte-delay": ("auto", "b8-chain-delay"), "u16": ("u16", "w16-delay-jitter"), "u16-table": ("u16", "w16-table-b"),
            "dw": ("dw", "w28-getters"), "u32": ("u32", "w32-b"), "wide": ("wide", "wide-32bits")}
SEGMENTS = [(0, 4), (4, 2), (6, 1), (7, 2), (9, 3)]  # the runs of F.NOWS with 1 s steps (kwk_step_n: one dt per call)


def boundary_slots(n, tile):
    """~400 slots: both sides of every tile, wave (tile / 4) and 64-slot boundary, slot n - 1, and
    a deterministic fill."""
    s = {0, n - 1}
    for step in (64, tile // 4, tile, 4 * tile):
        for b in range(step, n, step):
            s |= {b - 1, b}
    rng = np.random.default_rng(12345)
    s |= set(int(x) for x in rng.choice(n, 240, replace=False))
    return sorted(x for x in s if 0 <= x < n)


@pytest.fixture(scope="module")
def boundary(compiled):
    """fmt -> the tiled case: program, columns of all n slots, the sampled slots' oracle run."""
    cache = {}

    def get(which):
        if which not in cache:
            fmt, name = BOUNDARY[which]
            kp, ing, _, _ = compiled(name)
            docs, objs = F.case(name)
            tile = abi.lib().kwk_tile_objects()
            n = 2 * tile + tile // 2 + 37
            cols = ing.variant_columns(objs, np.arange(n, dtype=np.int64) % len(objs))
            slots = boundary_slots(n, tile)
            run = F.OracleRun(docs, [objs[s % len(objs)] for s in slots], slots=slots, **F.run_params(name))
            cache[which] = (fmt, name, kp, ing, cols, n, np.asarray(slots, dtype=np.int64), run,
                            F.expected_rows(run, kp.describe()))
        return cache[which]

    return get


def check_list(what, slot, stage, flags, sample, exp):
    assert len(np.unique(slot)) == len(slot), (what, "a slot fired twice")
    sel = np.isin(slot.astype(np.int64), sample)
    got = sorted(zip(slot[sel].tolist(), stage[sel].tolist(), flags[sel].tolist()))
    assert got == exp, (what, "device-only", sorted(set(got) - set(exp))[:8], "oracle-only",
                        sorted(set(exp) - set(got))[:8])


@pytest.mark.parametrize("which", sorted(BOUNDARY))
def test_tile_boundaries_single_steps(which, boundary):
    fmt, name, kp, ing, cols, n, sample, run, expected = boundary(which)
    assert not kp.delta_conflicts
    applied = sum(1 << b for b in kp.applied_bits.values())
    eng = make_engine(kp, cols, ing.record_array(), fmt, n, **F.run_params(name))
    try:
        fired_before = 0
        for k, now in enumerate(F.NOWS):
            what = (name, fmt, "step", k)
            eng.step(now, F.RUN_SEED, k)
            f = eng.fired()
            check_list(what, f["slot"], f["stage"], f["flags"], sample, run.steps[k].fired)
            total = eng.stats()["fired"]
            assert len(f) == total - fired_before, what
            fired_before = total
            hot, dels = eng.read()
            check_rows(what, kp, (hot[sample], dels[sample]), expected[k], applied)
        assert eng.stats()["state_bytes"] in (BYTE_STATE if name in BYTE_CASES else STATE_BYTES[fmt])
        assert run.total > 0
    finally:
        eng.close()


@pytest.mark.parametrize("which", sorted(BOUNDARY))
def test_tile_boundaries_step_n_fetch(which, boundary):
    """kwk_step_n over each run of 1 s steps, every step's list read by kwk_fired_fetch."""
    from kwok_amd.host.engine import PinnedBuffer
    fmt, name, kp, ing, cols, n, sample, run, expected = boundary(which)
    applied = sum(1 << b for b in kp.applied_bits.values())
    eng = make_engine(kp, cols, ing.record_array(), fmt, n, **F.run_params(name))
    bufs = [PinnedBuffer(8 * n + 64) for _ in range(4)]
    try:
        eng.fired_keep(8)
        fired_before = 0
        for k0, cnt in SEGMENTS:
            assert all(F.NOWS[k0 + j] == F.NOWS[k0] + j * 10**9 for j in range(cnt))
            eng.step_n(cnt, F.NOWS[k0], 10**9, F.RUN_SEED, k0, True)
            infos = [eng.fetch_step(k0 + j, bufs[j]) for j in range(cnt)]
            eng.fetch_wait()
            listed = 0
            for j, fi in enumerate(infos):
                what = (name, fmt, "step_n", k0 + j)
                assert fi["format"] == abi.COMPACT_REC and fi["step"] == k0 + j, (what, fi)
                f = bufs[j].array(abi.FIRED_DTYPE, fi["n_records"]).copy()
                check_list(what, f["slot"], f["stage"], f["flags"], sample, run.steps[k0 + j].fired)
                listed += len(f)
            total = eng.stats()["fired"]
            assert listed == total - fired_before, (name, fmt, k0)
            fired_before = total
            assert eng.stats()["state_bytes"] in (BYTE_STATE if name in BYTE_CASES else STATE_BYTES[fmt])
            hot, dels = eng.read()
            check_rows((name, fmt, "after step", k0 + cnt - 1), kp, (hot[sample], dels[sample]), expected[k0 + cnt - 1],
                       applied)
    finally:
        eng.close()
        for b in bufs:
            b.close()

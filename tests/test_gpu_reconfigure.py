"""Every path that replaces a handle's device buffers (kwok_amd/csrc/devmem.hpp: DESIGN.md §5
"Ownership"), at the smallest sizes that reach it.  Every case has one pattern: handle X is
configured with A and then with B, a fresh handle Y with B only, both run the same calls with the
same seeds, and their outputs are bit-equal (np.array_equal on the raw arrays: the same kernels over
the same inputs); both are closed.  Where a test of the suite compares B with the oracle, B comes
from that test's builder.

The failed-allocation paths are not run here (that would take a card's memory away from others):
tests/test_devmem.py runs the owners against failing allocations on the CPU.

The exposition's arenas that outgrow their slack, and the deferred frees they leave, are the last
round of test_relabel_equals_full_commit and test_long_keys_with_a_shared_prefix
(tests/test_gpu_expo_incremental.py)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T0 = 1_700_000_000 * 10**9


def _same(x, y, what):
    assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x, y), what


# ---- 1: usage configurations that shrink and grow
U_ROW = 1024  # kURow: the pods of a wave row of the usage kernels
U_CPU = np.array([0.0, 0.1, 0.25, 2.0])
U_MEM = np.array([0.0, 64.0 * 2**20, 2.0**30])


def _ukey(nc, cpu, mem):
    return (nc << 28) | (mem << 14) | cpu


def _usage_a():
    """3 nodes with (1, 0, 9) pods."""
    keys = np.array([_ukey(1 + i % 2, 1 + i % 3, 1 + i % 2) for i in range(10)], dtype=np.uint32)
    return np.array([0, 1, 1, 10], dtype=np.uint32), keys, U_CPU, U_MEM, None, None


def _usage_b():
    """5 nodes, one with more pods than a wave row, and one pod whose two containers differ."""
    per = [3, U_ROW + 76, 0, 7, 50]
    n = sum(per)
    keys = np.array([_ukey(1 + i % 3, i % 4, i % 3) for i in range(n)], dtype=np.uint32)
    keys[5] = 0  # mixed entry 0
    mixed = np.array([0, 2], dtype=np.uint32)
    ckeys = np.array([_ukey(0, 2, 1), _ukey(0, 3, 2)], dtype=np.uint32)
    return np.concatenate([[0], np.cumsum(per)]).astype(np.uint32), keys, U_CPU, U_MEM, mixed, ckeys


def _usage_run(eng, cfg, times):
    eng.usage_config(*cfg)
    eng.usage_pods(True)
    for t in times:
        eng.usage(t)
    n = int(cfg[0][-1])
    node, cluster = eng.usage_read()
    return node, cluster, eng.usage_read_pods(0, n), eng.usage_read_containers(0, n)


def test_usage_configurations_that_shrink_and_grow():
    from tests import test_gpu_fused_carry as F
    prog, pvars = F._program()
    a, b = _usage_a(), _usage_b()
    n = int(b[0][-1])
    pidx = np.zeros(n, dtype=np.int32)
    x, y = F._engine(prog, pvars, pidx, True), F._engine(prog, pvars, pidx, True)
    times = (T0, T0 + 2_500_000_123)
    try:
        for cfg in (a, b, a):  # each used, so that its integrators are not zero when it goes
            _usage_run(x, cfg, (T0 - 10**9, T0 - 10**8))
        got, want = _usage_run(x, b, times), _usage_run(y, b, times)
        for g, w, what in zip(got, want, ("nodes", "cluster", "pods", "containers")):
            _same(g, w, what)
        node, cluster, pods, cont = want
        # B is right: every pod is alive, so a node's usage is the sum of its pods' values, and the
        # integrators started from zero (the interval between the two evaluations only)
        ptr, keys = b[0], b[1]
        cpu = np.array([U_CPU[k & 0x3FFF] * (k >> 28) for k in keys])
        cpu[5] = U_CPU[2] + U_CPU[3]
        want_cpu = np.array([cpu[ptr[j]:ptr[j + 1]].sum() for j in range(len(ptr) - 1)])
        np.testing.assert_allclose(node[:, 0], want_cpu, rtol=1e-12)
        np.testing.assert_allclose(node[:, 2], want_cpu * ((times[1] - times[0]) / 1e9), rtol=1e-9)
        np.testing.assert_allclose(pods[:, 0], cpu, rtol=1e-12)
        assert len(cont) == int(sum(max(int(k) >> 28, 0) for k in keys)) + 2
    finally:
        x.close()
        y.close()


# ---- 2: metric and histogram programs loaded twice
def test_metric_programs_loaded_twice():
    import yaml
    from kwok_amd.host import cel
    from kwok_amd.host.compiler import KindProgram
    from kwok_amd.host.engine import Engine, Ingest
    from kwok_amd.host.metrics import MetricsProgram, load_metric_yaml
    from kwok_amd.host.stages import load_stage_files
    from kwok_amd.host.usage import UsageProgram, load_usage_yaml, usage_columns
    from tests import test_metrics as M
    cl, pods, text = M._mixed_cluster()  # (test_gpu_container_usage_and_metric_scrape checks it against the oracle)
    cols = usage_columns(UsageProgram(*load_usage_yaml(text)), pods)
    kp = KindProgram(load_stage_files(*cl.pod_stage_files))
    kp.explore(pods)
    ing = Ingest(kp)
    scalar = load_metric_yaml(open(M.METRICS).read())[1]
    hist = load_metric_yaml(M.HIST_YAML)[1]
    big, small = MetricsProgram(scalar), MetricsProgram(scalar[:2])
    hbig, hsmall = MetricsProgram(hist), MetricsProgram(hist[1:2])
    assert 0 < len(small.programs) < len(big.programs) and 0 < len(hsmall.hist_programs) < len(hbig.hist_programs)
    assert sum(len(p[1]) for p in hsmall.hist_programs) < sum(len(p[1]) for p in hbig.hist_programs)
    n_nodes = len(cl.node_ptr) - 1
    created = np.array([M._ns(p["metadata"]["creationTimestamp"]) if "creationTimestamp" in p["metadata"]
                        else np.iinfo(np.int64).min for p in pods], dtype=np.int64)
    zero_unix = float(cel.wrap_int64(cel.GO_ZERO_TIME.ns)) / 1e9
    inputs = (created, np.full(n_nodes, np.iinfo(np.int64).min, dtype=np.int64), np.zeros(n_nodes), zero_unix)
    other = (np.full(len(pods), T0 - 5 * 10**9, dtype=np.int64), np.full(n_nodes, T0, dtype=np.int64), np.ones(n_nodes), 0.0)

    def engine():
        e = Engine(kp, capacity=len(pods))
        e.load_stages()
        e.load(*ing.columns(pods), ing.record_array())
        e.usage_config(cl.node_ptr, *cols)
        e.usage_pods(True)
        return e

    x, y = engine(), engine()
    try:
        x.metrics_load(small.programs)
        x.metrics_inputs(*other)
        x.metrics_load(big.programs)
        x.metrics_inputs(*inputs)
        x.histograms_load(hsmall.hist_programs)
        x.histograms_load(hbig.hist_programs)
        y.metrics_load(big.programs)
        y.metrics_inputs(*inputs)
        y.histograms_load(hbig.hist_programs)
        for e in (x, y):
            e.usage(T0)
        # a range, a strict subset of it (the output buffers are reused), every node (they grow), the range again
        for first, count in ((1, 3), (2, 1), (0, n_nodes), (1, 3)):
            mx, my = x.metrics_eval(T0, first, count), y.metrics_eval(T0, first, count)
            hx, hy = x.histograms_eval(T0, first, count), y.histograms_eval(T0, first, count)
            assert len(mx) > 0 and len(hx) > 0
            _same(mx.view(np.uint64), my.view(np.uint64), ("metrics", first, count))
            _same(hx, hy, ("histograms", first, count))
    finally:
        x.close()
        y.close()


# ---- 3: the hand-back ring rebuilt between fused launches
def test_ring_rebuilt_between_fused_launches():
    from kwok_amd.host import abi
    from kwok_amd.host.engine import PinnedBuffer
    from tests import test_gpu_fused_carry as F
    n = 2 * int(abi.lib().kwk_tile_objects())
    prog, pvars = F._program()
    pidx = F._hash_variants(n)
    x, y = F._engine(prog, pvars, pidx, True), F._engine(prog, pvars, pidx, True)
    bufs = [(PinnedBuffer(2 * n + 64), PinnedBuffer(4 * (n // 2048 + 64))) for _ in range(4)]

    def group(e, k):
        e.step_n(4, F.NOW0 + k * F.DT, F.DT, F.SEED, k, "packed16")
        assert e.last_sweep()["steps"] == 4
        infos = [e.fetch_step(k + j, *bufs[j]) for j in range(4)]
        e.fetch_wait()
        out = []
        for j, fi in enumerate(infos):
            assert fi["step"] == k + j and fi["format"] == abi.COMPACT_PACKED16
            out.append((bufs[j][0].array(np.uint16, fi["n_records"]).copy(), bufs[j][1].array(np.uint32, fi["n_segs"]).copy()))
        return out

    try:
        for k in range(F.WARM):
            for e in (x, y):
                e.step(F.NOW0 + k * F.DT, F.SEED, k)
                e.fired_compact("16")
        y.fired_keep(8)
        fired = 0
        for g, depth in enumerate((4, 2, 0, 8)):
            x.fired_keep(depth)
            k = F.WARM + 4 * g
            for j, ((rx, cx), (ry, cy)) in enumerate(zip(group(x, k), group(y, k))):
                _same(cx, cy, ("segment counts", depth, k + j))
                _same(rx, ry, ("records", depth, k + j))
                fired += len(rx)
        assert fired > 0
        _same(x.fired(), y.fired(), "the last step's list")
    finally:
        for e in (x, y):
            e.close()
        for pair in bufs:
            for p in pair:
                p.close()


# ---- 4: emitter sets reserved again, the finalizer program
def test_emitter_sets_reserved_again():
    """(A second kwk_emit_finalizers_load on an emitter that has a program is refused with KWK_ESTATE,
    before and after the owners: X's second call checks that, and that the emitter goes on with the
    program it has.)"""
    from kwok_amd import workload as W
    from kwok_amd.host import abi, emit
    from kwok_amd.host.stages import load_stage_files
    from tests import test_gpu_emit_finalizers as E
    cl = W.make_cluster("C2", 8, 64, seed=0x91)
    rig = E.Rig(load_stage_files(*cl.pod_stage_files), cl.pods.materialize(), harness=True)
    n = rig.n
    x, y = rig.twin, emit.Emitter(rig.eng, n, rig.ep)  # (rig.twin has no finalizer program yet)
    try:
        assert any(st["flags"] & 8 for st in rig.fp.stages)  # the program has a finalizer stage
        words, cols = rig.ep.rows(rig.ctl.objs, rig.classes)
        fin_words = rig.host_words()
        for k in range(8):  # a step whose list has a finalizer record
            rig.eng.step(T0 + k * 10**9, 0x91, k)
            if any(rig.prog.stages[int(r["stage"])].next.finalizers is not None for r in rig.eng.fired()):
                break
        rig.eng.fired_compact(packed=True)
        items, nbytes = n + 1, 4096 * n

        def emission(em):
            em.emit(T0, packed=True)
            ni, nb = em.result()
            assert ni > 0 and nb > 0
            return em.collect()

        x.reserve_sets(1, items, nbytes)
        first = emission(x)
        x.reserve_sets(3, items, 2 * nbytes)
        x.set_rows(0, words, cols)
        for g, w in zip(emission(x), first):
            assert np.array_equal(g, w) if isinstance(w, np.ndarray) else g == w
        x.load_finalizers(rig.fp)
        with pytest.raises(abi.EngineError, match=r"\(%d\)" % abi.KWK_ESTATE):
            x.load_finalizers(rig.fp)
        y.reserve_sets(3, items, 2 * nbytes)
        y.load_finalizers(rig.fp)
        got = []
        for em in (x, y):
            em.set_rows(0, words, cols)
            em.set_fin_words(0, fin_words)
            em.reserve_fin(n + 1, 1024 * n)
            got.append((emission(em), em.collect_fin(), em.words(0, n), em.fin_words(0, n)))
        (mx, fx, wx, fwx), (my, fy, wy, fwy) = got
        for sx, sy, what in ((mx, my, "merge patches"), (fx, fy, "finalizer patches")):
            _same(sx[0], sy[0], what + ": items")
            _same(sx[1], sy[1], what + ": offsets")
            assert sx[2] == sy[2], what + ": bytes"
        assert len(fx[0]) > 0
        _same(wx, wy, "guard words")
        _same(fwx, fwy, "order words")
    finally:
        y.close()
        rig.close()


# ---- 6: destruction order
def test_destroy_then_create_again():
    """An engine, an emitter and an exposition writer on it, each used once, destroyed with the engine
    last; then an engine of the same capacity again: its first fired list is the first engine's."""
    from kwok_amd import workload as W
    from kwok_amd.host import emit
    from kwok_amd.host.engine import Engine, Ingest
    from kwok_amd.host.patchtpl import PatchProgram
    from tests import test_gpu_expo as X
    per = [0, 40, 3]
    cl = W.make_cluster("C4", len(per), sum(per), seed=9)
    pods, nodes = cl.pods.materialize(), cl.nodes.materialize()
    rig = X.Rig(cl, pods, nodes, np.concatenate([[0], np.cumsum(per)]).astype(np.uint32))
    em = None
    try:
        prog = rig.eng.p
        classes = [prog.class_of(o, register=False) for o in pods]
        pp = PatchProgram(prog.stages, {"NodeIPWith": lambda *a: "10.100.100.100", "PodIPWith": lambda *a: "11.100.100.100"})
        ep = emit.EmitProgram(prog.stages, pp, dict(zip(classes, pods)), len(prog.class_ids), stride=16)
        em = emit.Emitter(rig.eng, len(pods), ep)
        rig.eng.step(T0, 7, 0)
        rig.eng.fired_compact(packed=True)
        em.run(T0, packed=True)
        rig.eng.usage(T0)
        assert len(rig.ex.scrape(T0, 0, len(nodes))) == len(nodes)
        first = rig.eng.fired().copy()
        assert len(first) > 0
    finally:
        if em is not None:
            em.close()
        rig.close()  # the writer, then the engine
    ing = Ingest(prog)
    again = Engine(prog, capacity=len(pods))
    try:
        again.load_stages()
        again.load(*ing.columns(pods), ing.record_array())
        again.step(T0, 7, 0)
        _same(again.fired(), first, "the first fired list")
    finally:
        again.close()

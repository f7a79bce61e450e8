"""Incremental usage updates on the GPU (kwk_usage_set_rows / _append / _mixed_append / _info_get):
an engine that follows changed pods row by row against a twin configured from scratch with the
pods as they are now (bit-identical: the same per-pod doubles, summed in slot order), its
integrators against the oracle's uninterrupted run (1e-6 relative, the usage tolerance), the
scatter kernel's shapes, the kernel the next kwk_usage takes, clock-dependent values, the
steady-state counters, refusals and the exposition."""
import copy
import functools

import numpy as np
import pytest
import yaml

from kwok_amd import workload as W
from kwok_amd.host import abi, cel
from kwok_amd.host.usage import UsageProgram, UsageTable, load_usage_yaml
from oracle import usage_ref
from tests import usage_rows_util as R
from tests.usage_dyn_util import ANN, created_ns

pytestmark = pytest.mark.gpu

REL_TOL = 1e-6
T0 = R.T0
I64_MIN = np.iinfo(np.int64).min
STATES = {"auto": 1, "u16": 2, "u32": 4, "dw": 8, "wide": 8}  # Engine(state=...) -> bytes per state word


def _irregular_node_ptr(n_pods):
    """tests/test_usage.py's layout restated: empty nodes (first, inner, trailing), 1-pod nodes
    (more than a chunk holds), a 2500-pod node spanning wave rows, 1016 / 1017-pod nodes."""
    sizes = [0, 1, 2500, 0, 0] + [1] * 300 + [7, 0, 1016, 1017, 3]
    rest = n_pods - sum(sizes)
    assert rest > 0
    while rest > 0:
        sizes.append(min(37, rest))
        rest -= sizes[-1]
    sizes += [0, 0]
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def _state_columns(n):
    """Pod-fast pods (the stage mix whose words close within 255 ids: 1-byte state where allowed)."""
    from kwok_amd.host.compiler import HarnessSpec, KindProgram
    from kwok_amd.host.engine import Ingest
    from kwok_amd.host.stages import load_stage_files
    pvars = [W.pod_object("p", "n"), W.pod_object("p", "n", job=True)]
    pidx = np.random.default_rng(5).integers(0, 2, n).astype(np.int32)
    kp = KindProgram(load_stage_files(*W.stage_paths(W.POD_FAST)), HarnessSpec())
    kp.explore(pvars)
    ing = Ingest(kp)
    return kp, ing.variant_columns(pvars, pidx), ing.record_array(), max(1, len(ing.records)) + 16


def _created(pods):
    return np.array([I64_MIN if created_ns(p) is None else created_ns(p) for p in pods], dtype=np.int64)


def _engine(ptr, cols, state="auto", pods_out=True, created=None, dead=()):
    """A pods engine over `ptr` configured with UsageTable.config's columns; created: the pods'
    creation times (kwk_metrics_inputs), dead: slots deleted."""
    from kwok_amd.host.engine import Engine
    n = int(ptr[-1])
    kp, scols, recs, max_records = _state_columns(n)
    eng = Engine(kp, capacity=n, state=state, max_records=max_records)
    try:
        eng.load_stages()
        eng.load(*scols, recs)
        keys, cv, mv, mx, ck, cp, mp, ops = cols
        eng.usage_config(ptr, keys, cv, mv, mx, ck, cpu_progs=cp, mem_progs=mp, ops=ops)
        if pods_out:
            eng.usage_pods(True)
        if created is not None:
            eng.metrics_inputs(created, np.full(len(ptr) - 1, I64_MIN, dtype=np.int64), np.zeros(len(ptr) - 1),
                               cel.zero_time_unix_second())
        if len(dead):
            eng.delete(np.asarray(dead))
    except Exception:
        eng.close()
        raise
    return eng


def _revive(eng, slots):
    _, (hot, dels, rec, cls), _, _ = _state_columns(eng.capacity)
    s = np.asarray(slots)
    eng.upsert(s, hot[s], dels[s], rec[s], cls[s])


def _read(eng, pods_out):
    node, total = eng.usage_read()
    return (node[:, :2].copy(), total.copy()) + ((eng.usage_read_pods()[:, :2].copy(),) if pods_out else ())


def _assert_twin(eng, twin, pods_out, tag):
    for name, a, b in zip(("node sums", "cluster total", "pod columns 0-1"), _read(eng, pods_out), _read(twin, pods_out)):
        assert a.tobytes() == b.tobytes(), (tag, name, float(np.abs(a - b).max()))
    assert eng.usage_info()["kernel"] == twin.usage_info()["kernel"], (tag, eng.usage_info(), twin.usage_info())


# ------------------------------------------------------------------ twin equality, every state format
@functools.lru_cache(maxsize=None)
def _scenario():
    """Five seeded batches over ~6000 pods on the irregular nodes: edits, new constants and
    replacements first (the fast path survives where per-pod outputs are off), then mixed pods and
    container-count changes, then the first programs, deletes and upserts.  Per batch: the update,
    the slots deleted / upserted before the evaluation, and the twin's configuration."""
    n = 6000
    ptr = _irregular_node_ptr(n)
    pods = R.make_pods(n, np.repeat(np.arange(len(ptr) - 1), np.diff(ptr)))
    prog = R.program(dyn=True)
    tab = UsageTable(prog)
    cols0 = tab.config(pods)
    created0 = _created(pods)
    rng = np.random.default_rng(20261)
    dead = np.zeros(n, dtype=bool)
    steps = []
    for t in range(5):
        kinds = ("edit", "new", "replace") if t == 0 else ("replace", "edit", "mixed", "count", "new")
        slots, new, resets, created = R.batch(rng, pods, t, [40, 600, 257, 64, 300][t], programs=t >= 2, kinds=kinds)
        up = tab.rows(slots, new, reset=resets, created_ns=created)
        for s, p in zip(slots, new):
            pods[s] = p
        gone, back = np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
        if t == 3:
            gone = np.arange(3, n, 11)
            dead[gone] = True
        if t == 4:
            back = np.arange(3, n, 22)
            dead[back] = False
        steps.append(dict(up=up, gone=gone, back=back, dead=np.flatnonzero(dead), twin=UsageTable(prog).config(pods),
                          created=_created(pods), now=T0 + (t + 1) * 2_500_000_123))
    assert len(steps[2]["twin"][5]) and len(steps[1]["twin"][3]) and not len(steps[0]["twin"][3])
    return ptr, cols0, created0, steps


@pytest.mark.parametrize("state,pods_out", [(s, True) for s in STATES] + [("auto", False), ("u32", False)])
def test_gpu_rows_equal_a_fresh_configuration(state, pods_out):
    ptr, cols0, created0, steps = _scenario()
    eng = _engine(ptr, cols0, state, pods_out, created0)
    try:
        assert eng.stats()["state_bytes"] == STATES[state]
        want_kernels = []
        for t, s in enumerate(steps):
            eng.usage_apply(s["up"])
            if len(s["gone"]):
                eng.delete(s["gone"])
            if len(s["back"]):
                _revive(eng, s["back"])
            eng.usage(s["now"])
            twin = _engine(ptr, s["twin"], state, pods_out, s["created"], s["dead"])
            try:
                twin.usage(s["now"])
                _assert_twin(eng, twin, pods_out, f"{state} batch {t}")
            finally:
                twin.close()
            want_kernels.append(eng.usage_info()["kernel"])
        if pods_out:
            assert want_kernels == ["general", "general", "programs", "programs", "programs"]
        else:  # the fast path while no pod is mixed and no value a program
            assert want_kernels[0] in ("fast8", "fast32") and want_kernels[1:] == ["general", "programs", "programs", "programs"]
        assert eng.usage_info()["row_calls"] == len(steps)
    finally:
        eng.close()


# ------------------------------------------------------------------ integrators against the oracle
def _oracle_eval(cum, docs, pods, ptr, t):
    """One evaluation of the reference: per container, per pod and per node {cpu, mem, cumulative
    cpu, cumulative mem}; the integrators keyed by pod name and container / by node."""
    cont, pod = [], np.zeros((len(pods), 4))
    for i, p in enumerate(pods):
        name = p["metadata"]["name"]
        for c in p["spec"]["containers"]:
            v = [usage_ref.container_usage(docs, p, c["name"], r) for r in ("cpu", "memory")]
            row = v + [cum.advance((name, c["name"], r), x, t) for r, x in zip(("cpu", "memory"), v)]
            cont.append(row)
            pod[i] += row
    node = np.zeros((len(ptr) - 1, 4))
    for j in range(len(ptr) - 1):
        v = pod[ptr[j]:ptr[j + 1], :2].sum(axis=0)
        node[j] = (v[0], v[1], cum.advance((j, "cpu"), v[0], t), cum.advance((j, "memory"), v[1], t))
    return np.array(cont), pod, node


def test_gpu_integrators_live_on_against_the_oracle():
    """Six evaluations at uneven intervals over 12 nodes / 300 pods.  Before the third: slot 10 is
    replaced (RESET) under a new name, slot 11's annotation is edited (no RESET, a new constant),
    slot 12 becomes a mixed pod (a range appended at the end).  Before the fourth: the mixed pod of
    slot 5 is replaced by one with more containers (a new range), slot 6's by one with fewer (its
    range reused).  Before the fifth, without RESET: a ResourceUsage arrives that makes the containers
    of slot 20's pod differ (uniform -> mixed: each container goes on from the total they shared), and
    slot 12's mixed pod gets a third container (its two totals carried into a larger range).  Every pod, container and node integrator equals the oracle's, whose run is never
    interrupted: a reconfiguration would zero them all."""
    n = 300
    ptr = (np.arange(13) * 25).astype(np.uint32)
    pods = R.make_pods(n, np.arange(n) // 25)
    for s, (name, nc) in {5: ("mixed-a", 2), 6: ("mixed-b", 3)}.items():
        pods[s]["metadata"]["name"] = name
        pods[s]["spec"]["containers"] = [{"name": f"container-{c}"} for c in range(nc)]
    # slot 20's pod is named like a ResourceUsage that arrives only before the fifth evaluation
    pods[20]["metadata"]["name"] = "mixed-f"
    assert len(pods[20]["spec"]["containers"]) == 3
    before_f = "\n---\n".join([open(R.GOLDEN).read()] + [R._named(x) for x in R.MIXED_NAMES if x != "mixed-f"])
    docs = [d for d in yaml.safe_load_all(before_f) if d]
    tab = UsageTable(UsageProgram(*load_usage_yaml(before_f)))
    eng = _engine(ptr, tab.config(pods))
    cum = usage_ref.Cumulative()

    def change(slot, reset, name=None, nc=None, cpu=None):
        p = copy.deepcopy(pods[slot])
        if name:
            p["metadata"]["name"] = name
        if nc:
            p["spec"]["containers"] = [{"name": f"container-{c}"} for c in range(nc)]
        if cpu:
            p["metadata"].setdefault("annotations", {})[R.CPU_ANN] = cpu
        pods[slot] = p
        return slot, p, reset

    try:
        t = T0
        info0 = eng.usage_info()
        for k in range(6):
            ch = []
            if k == 2:
                ch = [change(10, True, name="new-10", nc=2, cpu="150m"), change(11, False, cpu="777m"),
                      change(12, True, name="mixed-c", nc=2)]
            if k == 3:
                ch = [change(5, True, name="mixed-d", nc=3), change(6, True, name="mixed-e", nc=2)]
            if k == 4:  # no RESET: the CR edit that makes slot 20's containers differ; slot 12's pod with a third container
                docs = [d for d in yaml.safe_load_all(R.STATIC_DOCS) if d]
                tab.program = R.program(dyn=False)
                ch = [change(20, False), change(12, False, nc=3)]
                t_grown = t
            if ch:
                up = tab.rows([c[0] for c in ch], [c[1] for c in ch], reset=[c[2] for c in ch])
                assert eng.usage_apply(up) is True  # slot 12 (k = 2) and slots 5, 6 (k = 3) change their container counts
            eng.usage(t)
            cont, pod, node = _oracle_eval(cum, docs, pods, ptr, t)
            if k >= 4:
                # slot 12's third container: the reference starts a container's integrator at its own
                # first evaluation; the engine keeps the time of the last evaluation per pod (kwok_engine.h),
                # so the new container integrates from the pod's evaluation before the row
                row = sum(len(p["spec"]["containers"]) for p in pods[:12]) + 2
                extra = usage_ref.seconds(t_grown - t_before) * cont[row, :2]
                cont[row, 2:] += extra
                pod[12, 2:] += extra
            else:
                t_before = t
            got_node, got_total = eng.usage_read()
            got_pod, got_cont = eng.usage_read_pods(), eng.usage_read_containers()
            for name, g, w in (("node", got_node, node), ("pod", got_pod, pod), ("container", got_cont, cont)):
                err = np.abs(g - w) / np.maximum(np.abs(w), 1e-300)
                print(f"evaluation {k} {name}: max relative error", float(np.max(np.where(w == 0, np.abs(g), err))))
                np.testing.assert_allclose(g, w, rtol=REL_TOL, atol=1e-9, err_msg=f"evaluation {k}: {name}")
            np.testing.assert_allclose(got_total, node[:, :2].sum(axis=0), rtol=REL_TOL)
            if k == 2:  # the replaced pods' first evaluation only records the time; the edited one goes on
                assert np.all(got_pod[[10, 12], 2:] == 0) and got_pod[11, 2] > 0 and got_pod[9, 2] > 0
            if k == 3:
                assert np.all(got_pod[[5, 6], 2:] == 0) and np.all(got_pod[[10, 12], 2] > 0)
            t += 1_000_000_000 + 37_000_001 * k
        assert np.all(got_pod[:, 2] > 0) and np.all(got_node[:, 2] > 0)
        info = eng.usage_info()
        # appended ranges: slot 12's (2, then 3 when it grew), slot 5's (3), slot 20's (3); slot 6's reused
        assert info["n_integrators"] == info0["n_integrators"] + 11 and info["mixed_pods"] == 4  # slots 5, 6, 12, 20
    finally:
        eng.close()


# ------------------------------------------------------------------ the scatter kernel's shapes, steady state
@functools.lru_cache(maxsize=None)
def _plain():
    n = 6000
    ptr = _irregular_node_ptr(n)
    pods = R.make_pods(n, np.repeat(np.arange(len(ptr) - 1), np.diff(ptr)))
    return ptr, pods, UsageTable(R.program(dyn=False)).config(pods)


def _known_key_rows(rng, tab, pods, slots, t):
    """Replacements by pods whose values are all in the tables (other slots' pods under new names)."""
    src = rng.integers(0, len(pods), len(slots))
    new = []
    for k, (s, q) in enumerate(zip(slots, src)):
        p = copy.deepcopy(pods[int(q)])
        p["metadata"]["name"] = f"k{t}-{k}"
        p["spec"]["nodeName"] = pods[int(s)]["spec"]["nodeName"]
        new.append(p)
    up = tab.rows([int(s) for s in slots], new, reset=True)
    assert all(len(up[k]) == 0 for k in ("cpu_values", "mem_values", "cpu_progs", "mem_progs", "ops", "mixed", "ckeys"))
    return new, up


@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 255, 256, 257, 600])
def test_gpu_scatter_kernel_shapes(n_rows):
    """One call of n_rows rows (around the kernel's 256-thread blocks and 64-lane waves), naming the
    engine's first and last slot, the last slot of a node and the first of the next, and four
    adjacent slots that share a dword of the 1-byte key column: byte stores, not a read-modify-write
    of the dword.  On the fast path over 1-byte keys and, with per-pod outputs, the general kernel."""
    ptr, pods0, cols0 = _plain()
    n = len(pods0)
    fixed = [8, 9, 10, 11, 0, n - 1, int(ptr[5 + 300 + 3]) - 1, int(ptr[5 + 300 + 3]), 2499, 2500][:n_rows]
    rng = np.random.default_rng(n_rows)
    rest = rng.permutation(np.setdiff1d(np.arange(n), fixed))[:n_rows - len(fixed)]
    slots = np.concatenate([fixed, rest]).astype(np.int64)
    rng.shuffle(slots)
    for pods_out in (False, True):
        pods = list(pods0)
        tab = UsageTable(R.program(dyn=False))
        tab.config(pods)
        eng = _engine(ptr, cols0, "auto", pods_out)
        try:
            assert eng.usage_info()["kernel"] == ("general" if pods_out else "fast8")
            eng.usage(T0)
            new, up = _known_key_rows(rng, tab, pods, slots, 0)
            assert len(up["rows"]) == n_rows
            eng.usage_apply(up)
            for s, p in zip(slots, new):
                pods[int(s)] = p
            eng.usage(T0 + 10**9)
            twin = _engine(ptr, UsageTable(R.program(dyn=False)).config(pods), "auto", pods_out)
            try:
                twin.usage(T0 + 10**9)
                _assert_twin(eng, twin, pods_out, f"{n_rows} rows")
            finally:
                twin.close()
            if pods_out:  # RESET: the rows' pods read 0 at their first evaluation, the others integrated one second
                got = eng.usage_read_pods()
                untouched = np.setdiff1d(np.arange(n), slots)
                assert np.all(got[slots, 2:] == 0)
                np.testing.assert_allclose(got[untouched, 2], got[untouched, 0] * 1.0, rtol=REL_TOL)
        finally:
            eng.close()


def test_gpu_steady_state_makes_no_synchronisation_and_no_allocation():
    """After one warm call, a call of the same size whose keys are known leaves kwk_usage_info's
    synchronisation and allocation counters where they were (and a third, which reuses the first
    call's staging slot)."""
    ptr, pods0, cols0 = _plain()
    pods = list(pods0)
    tab = UsageTable(R.program(dyn=False))
    tab.config(pods)
    rng = np.random.default_rng(9)
    eng = _engine(ptr, cols0, "auto", True)
    try:
        eng.usage(T0)
        counters = []
        for t in range(3):
            slots = rng.choice(len(pods), 500, replace=False)
            new, up = _known_key_rows(rng, tab, pods, slots, t)
            for s, p in zip(slots, new):
                pods[int(s)] = p
            eng.usage_set_rows(up["rows"])
            eng.usage(T0 + (t + 1) * 10**9)
            if t == 1:
                eng.sync()  # the third call finds its staging slot's copy done
            info = eng.usage_info()
            counters.append((info["syncs"], info["allocs"]))
        assert counters[0][1] >= 1          # the warm call allocated the device rows
        assert counters[1] == counters[0] and counters[2] == counters[0], counters
        assert eng.usage_info()["row_calls"] == 3
        twin = _engine(ptr, UsageTable(R.program(dyn=False)).config(pods), "auto", True)
        try:
            twin.usage(T0 + 3 * 10**9)
            _assert_twin(eng, twin, True, "steady state")
        finally:
            twin.close()
    finally:
        eng.close()


# ------------------------------------------------------------------ which kernel the next kwk_usage takes
def _small(dyn=True, n=300):
    ptr = (np.arange(13) * (n // 12)).astype(np.uint32)
    pods = R.make_pods(n, np.arange(n) // (n // 12))
    prog = R.program(dyn=dyn)
    tab = UsageTable(prog)
    return ptr, pods, prog, tab, tab.config(pods)


def _twin_check(eng, ptr, prog, pods, pods_out, tag, t, created=None, masks=None):
    twin = _engine(ptr, UsageTable(prog).config(pods), "auto", pods_out, created)
    try:
        if masks is not None:  # kwk_aggregate runs the usage pass itself
            outs = []
            for e in (eng, twin):
                cnt = e.aggregate(masks, t, usage=True)
                outs.append(e.aggregate_read(cnt))
            assert outs[0].tobytes() == outs[1].tobytes(), (tag, outs)
            assert eng.usage_info()["fused_counts"] == twin.usage_info()["fused_counts"], tag
        eng.usage(t)
        twin.usage(t)
        _assert_twin(eng, twin, pods_out, tag)
    finally:
        twin.close()


def test_gpu_kernel_choice_follows_the_rows():
    """fast8 within the dictionary -> fast32 at the 256th distinct key -> general at the first mixed
    row -> programs at the first program (KWK_ESTATE until kwk_metrics_inputs); results and the
    kwk_aggregate(KWK_AGG_USAGE) report equal the twin's all along, through the fused-count path
    (1-byte ids, 1-byte keys) and after leaving it."""
    from kwok_amd.host.cluster import phase_masks
    ptr, pods, prog, tab, cols = _small()
    eng = _engine(ptr, cols, "auto", pods_out=False)
    try:
        masks = ([0] + list(phase_masks(eng.p, values=("Running", "Succeeded", "Failed")).values()))[:4]
        info = eng.usage_info()
        assert info["kernel"] == "fast8" and info["fused_counts"] == 1 and 0 < info["n_keys8"] <= 255
        keys0 = info["n_keys8"]

        def apply(slots, new, reset=False):
            up = tab.rows(slots, new, reset=reset)
            for s, p in zip(slots, new):
                pods[s] = p
            eng.usage_apply(up)

        def edited(slot, cpu):
            p = copy.deepcopy(pods[slot])
            p["metadata"].setdefault("annotations", {})[R.CPU_ANN] = cpu
            return p

        # within the dictionary: keys other pods have, and a few new ones
        apply([0, 1, 2, 3, 299], [edited(s, "150m") for s in (0, 1, 2, 3, 299)])
        apply([7], [edited(7, "4321m")])
        info = eng.usage_info()
        assert info["kernel"] == "fast8" and info["n_keys8"] > keys0 and info["n_cpu"] == len(cols[1]) + 1
        _twin_check(eng, ptr, prog, pods, False, "within the dictionary", T0, masks=masks)
        # 260 pods with a value of their own: past the dictionary's 255 keys
        slots = list(range(20, 280))
        apply(slots, [edited(s, f"{5000 + s}m") for s in slots])
        info = eng.usage_info()
        assert info["kernel"] == "fast32" and info["n_keys8"] == 0 and info["fused_counts"] == 0
        _twin_check(eng, ptr, prog, pods, False, "256 keys and more", T0 + 10**9, masks=masks)
        # back under 256 keys: the column comes back, as a configuration would build it
        apply(slots, [edited(s, "150m") for s in slots])
        assert eng.usage_info()["kernel"] == "fast8" and eng.usage_info()["fused_counts"] == 1
        _twin_check(eng, ptr, prog, pods, False, "keys gone again", T0 + 2 * 10**9, masks=masks)
        # the first mixed row
        mixed = copy.deepcopy(pods[40])
        mixed["metadata"]["name"] = "mixed-a"
        mixed["spec"]["containers"] = [{"name": f"container-{c}"} for c in range(3)]
        apply([40], [mixed], reset=True)
        info = eng.usage_info()
        assert info["kernel"] == "general" and info["mixed_pods"] == 1 and info["n_mixed"] == 1
        _twin_check(eng, ptr, prog, pods, False, "first mixed row", T0 + 3 * 10**9, masks=masks)
        # the first program: kwk_usage needs the creation times first
        ramp = copy.deepcopy(pods[41])
        ramp["metadata"].update(name="ramp-41", namespace="ramp", annotations={ANN: "2Mi"})
        apply([41], [ramp], reset=True)
        assert eng.usage_info()["kernel"] == "programs" and eng.usage_info()["n_cpu_progs"] == 1
        with pytest.raises(abi.EngineError, match=rf"\({abi.KWK_ESTATE}\).*kwk_metrics_inputs"):
            eng.usage(T0 + 4 * 10**9)
        created = _created(pods)
        eng.metrics_inputs(created, np.full(len(ptr) - 1, I64_MIN, dtype=np.int64), np.zeros(len(ptr) - 1),
                           cel.zero_time_unix_second())
        _twin_check(eng, ptr, prog, pods, False, "first program", T0 + 4 * 10**9, created=created, masks=masks)
    finally:
        eng.close()


def test_gpu_dictionary_values_after_the_largest_count_shrinks():
    """The only pod with 3 containers becomes a 1-container pod (its key leaves the 1-byte
    dictionary, the pod-value table needs fewer rows), then a constant is appended (the table is
    rebuilt at its new, smaller size): the dictionary's values are refreshed for the keys in use
    only, and the sums stay the twin's on the 1-byte-key fast path."""
    ptr, pods, prog, tab, _ = _small()
    for i, p in enumerate(pods):
        p["spec"]["containers"] = [{"name": f"container-{c}"} for c in range(3 if i == 7 else 1)]
    eng = _engine(ptr, tab.config(pods), "auto", pods_out=False)
    try:
        assert eng.usage_info()["kernel"] == "fast8" and eng.usage_info()["max_containers"] == 3
        one = copy.deepcopy(pods[7])
        one["spec"]["containers"] = one["spec"]["containers"][:1]
        pods[7] = one
        assert eng.usage_apply(tab.rows([7], [one])) is True
        assert eng.usage_info()["max_containers"] == 1
        new = copy.deepcopy(pods[8])
        new["metadata"].setdefault("annotations", {})[R.CPU_ANN] = "4321m"
        pods[8] = new
        up = tab.rows([8], [new])
        assert len(up["cpu_values"]) == 1
        eng.usage_apply(up)
        assert eng.usage_info()["kernel"] == "fast8"
        _twin_check(eng, ptr, prog, pods, False, "after the shrink and the append", T0)
    finally:
        eng.close()


# ------------------------------------------------------------------ clock-dependent values
def test_gpu_replaced_pod_evaluates_from_its_new_creation_time():
    """The memory ramp of tests/test_gpu_usage_dynamic.py (Quantity(annotation) * SinceSecond / 60):
    a pod replaced with KWK_USAGE_ROW_CREATED evaluates its program from the new creation time
    (cel.run_usage_program, the usage tolerance), and a pod-dimension Metric reading
    pod.SinceSecond() sees the same time."""
    ptr, pods, prog, tab, _ = _small()
    for i in range(0, 300, 3):  # a third of the pods ramp from the start
        pods[i]["metadata"].update(namespace="ramp", annotations={ANN: f"{1 + i % 3}Mi"})
    cols = tab.config(pods)
    assert len(cols[6])
    eng = _engine(ptr, cols, "auto", True, _created(pods))
    try:
        eng.metrics_load([("pod", cel.lower("pod.SinceSecond()", "pod"))])
        eng.usage(T0)
        slots = [3, 4, 150, 299]   # 3 and 150 ramped already; 4 and 299 start to
        new_created = [T0 - 45 * 10**9, T0 + 7 * 10**9, T0 - 3600 * 10**9, None]
        new = []
        for s, c in zip(slots, new_created):
            p = copy.deepcopy(pods[s])
            p["metadata"].update(name=f"fresh-{s}", namespace="ramp", annotations={ANN: "3Mi"})
            if c is None:
                p["metadata"].pop("creationTimestamp", None)
            else:
                p["metadata"]["creationTimestamp"] = R.stamp(c)
            new.append(p)
            pods[s] = p
        up = tab.rows(slots, new, reset=True, created_ns=[I64_MIN if c is None else c for c in new_created])
        eng.usage_apply(up)
        for t in (T0 + 2_500_000_123, T0 + 9_500_000_124):
            eng.usage(t)
            got = eng.usage_read_pods()
            since = eng.metrics_eval(t, 0, len(ptr) - 1)
            assert len(since) == len(pods)
            for s, c in zip(slots, new_created):
                (_, mem), = set(prog.pod_container_programs(pods[s]))
                want = cel.run_usage_program(list(mem), t, c, None) * len(pods[s]["spec"]["containers"])
                print("slot", s, "memory", got[s, 1], "expected", want)
                np.testing.assert_allclose(got[s, 1], want, rtol=REL_TOL)
                np.testing.assert_allclose(since[s], cel.run_usage_program([(cel.OP_LOAD, cel.IN_POD_SINCE)], t, c, None),
                                           rtol=REL_TOL)
            i = 6  # an untouched ramping pod
            (_, mem), = set(prog.pod_container_programs(pods[i]))
            np.testing.assert_allclose(got[i, 1], cel.run_usage_program(list(mem), t, created_ns(pods[i]), None) *
                                       len(pods[i]["spec"]["containers"]), rtol=REL_TOL)
        assert np.all(got[slots[:3], 3] > 0)  # (slot 299 has no creation time: its ramp saturates)
    finally:
        eng.close()


# ------------------------------------------------------------------ refusals
def test_gpu_refused_calls_change_nothing():
    from kwok_amd.host.engine import Engine
    ptr, pods, prog, tab, cols = _small()
    n = len(pods)
    kp, scols, recs, max_records = _state_columns(n)
    bare = Engine(kp, capacity=n, max_records=max_records)
    try:
        bare.load_stages()
        bare.load(*scols, recs)
        row = np.zeros(1, dtype=abi.USAGE_ROW_DTYPE)
        row["usage_key"] = 1 << 28
        for call in (lambda: bare.usage_set_rows(row), lambda: bare.usage_append(cpu_values=[1.0]),
                     lambda: bare.usage_mixed_append([0, 0], [])):
            with pytest.raises(abi.EngineError, match=rf"\({abi.KWK_ESTATE}\).*kwk_usage_config"):
                call()
    finally:
        bare.close()
    eng = _engine(ptr, cols, "auto", True)
    try:
        eng.usage(T0)
        before = (eng.usage_read(), eng.usage_read_pods(), eng.usage_info())

        def rows(*slot_keys):
            r = np.zeros(len(slot_keys), dtype=abi.USAGE_ROW_DTYPE)
            for i, (s, k) in enumerate(slot_keys):
                r[i] = (s, k, abi.USAGE_ROW_RESET, 0, 0)
            return r

        ok = int(cols[0][0])
        n_cpu, n_mixed = len(cols[1]), len(cols[3]) // 2
        for bad, status, word in (
                (rows((4, ok), (9, ok), (4, ok)), abi.KWK_EINVAL, "row 2: slot 4 named twice"),
                (rows((0, ok), (n, ok)), abi.KWK_EINVAL, f"row 1: slot {n} beyond"),
                (rows((0, ok), (1, (1 << 28) | n_cpu)), abi.KWK_EINVAL, "row 1: usage_key value id out of range"),
                (rows((2, n_mixed)), abi.KWK_EINVAL, "row 0: usage_key mixed index out of range")):
            with pytest.raises(abi.EngineError, match=rf"\({status}\).*{word}"):
                eng.usage_set_rows(bad)
        created = rows((0, ok))
        created["flags"] = abi.USAGE_ROW_CREATED
        with pytest.raises(abi.EngineError, match=rf"\({abi.KWK_ESTATE}\).*kwk_metrics_inputs"):
            eng.usage_set_rows(created)
        with pytest.raises(abi.EngineError, match=rf"\({abi.KWK_EINVAL}\).*beyond ckeys"):
            eng.usage_mixed_append([0, 99], [])
        # a constant appended to a table with programs
        ramp = copy.deepcopy(pods[41])
        ramp["metadata"].update(name="ramp-41", namespace="ramp", annotations={ANN: "2Mi"})
        up = tab.rows([41], [ramp], reset=True)
        eng.usage_append(up["cpu_values"], up["mem_values"], up["cpu_progs"], up["mem_progs"], up["ops"])
        with pytest.raises(abi.EngineError, match=rf"\({abi.KWK_ESTATE}\).*KWK_MOP_CONST"):
            eng.usage_append(cpu_values=[0.5])
        bad_prog = np.array([[len(up["ops"]) + 7, 3]], dtype=np.uint32)
        with pytest.raises(abi.EngineError, match=rf"\({abi.KWK_EINVAL}\).*ops range"):
            eng.usage_append(cpu_progs=bad_prog)
        # nothing of that reached the keys: the rows' slots read what they read (slot 41's row was never sent)
        eng.metrics_inputs(_created(pods), np.full(len(ptr) - 1, I64_MIN, dtype=np.int64), np.zeros(len(ptr) - 1),
                           cel.zero_time_unix_second())
        eng.usage(T0)
        after = (eng.usage_read(), eng.usage_read_pods())
        assert before[0][0][:, :2].tobytes() == after[0][0][:, :2].tobytes() and before[0][1].tobytes() == after[0][1].tobytes()
        assert before[1].tobytes() == after[1].tobytes()
        info = eng.usage_info()
        assert info["n_cpu"] == before[2]["n_cpu"] and info["n_mixed"] == before[2]["n_mixed"]
    finally:
        eng.close()


# ------------------------------------------------------------------ the exposition
def test_gpu_exposition_follows_row_updates():
    """At tests/test_gpu_expo_incremental.py's size: after a row update that keeps every container
    count the scrape's text equals the Python exposition of the current pods; after one that changes
    a count, layout_changed is set and the text is right after kwk_expo_commit (rows set again from
    the first moved pod on)."""
    from kwok_amd.host.usage import UsageProgram, load_usage_yaml
    from tests.test_gpu_expo import Rig, _mixed_cluster
    cl, pods, text = _mixed_cluster()
    nodes = [{"metadata": {"name": f"node-{j}"}} for j in range(len(cl.node_ptr) - 1)]
    rig = Rig(cl, pods, nodes, cl.node_ptr, usage_text=text)
    try:
        tab = UsageTable(UsageProgram(*load_usage_yaml(text)))
        tab.config(pods)   # the ids Rig's usage_columns gave (no programs: the same interning)
        n_nodes = len(nodes)

        def check(t, tag):
            rig.eng.usage(t)
            got = rig.ex.scrape(t, 0, n_nodes)
            for j in range(n_nodes):
                w = rig.expected(t, j)
                assert got[j] == (w[0] if isinstance(w, tuple) else w), (tag, j)

        check(T0, "configured")
        # values only: annotations of uniform pods (a known value, a new one)
        slots = [2, 6, 10]
        new = []
        for s, cpu in zip(slots, ("100m", "3210m", "100m")):
            p = copy.deepcopy(pods[s])
            p["metadata"].setdefault("annotations", {})[R.CPU_ANN] = cpu
            new.append(p)
            rig.pods[s] = p
        assert rig.eng.usage_apply(tab.rows(slots, new)) is False
        check(T0 + 10**9, "values changed")
        # a container more in slot 4, one fewer in a later uniform pod: every later container row moves
        less = next(i for i in range(8, len(pods)) if i % 4 != 1 and len(pods[i]["spec"]["containers"]) > 1)
        new = []
        for s in (4, less):
            p = copy.deepcopy(rig.pods[s])
            cs = p["spec"]["containers"]
            if s == 4:
                cs.append({"name": f"container-{len(cs)}", "image": "busybox"})
            else:
                cs.pop()
            new.append(p)
            rig.pods[s] = p
        assert rig.eng.usage_apply(tab.rows([4, less], new, reset=True)) is True
        rig.ex.layout_changed()
        rig.ex.commit()                       # the engine's new layout: the rows' arrays follow it
        rig.ex.set_pods(rig.pods[4:], 4, nodes)
        rig.ex.commit()
        check(T0 + 2 * 10**9, "counts changed")
    finally:
        rig.close()

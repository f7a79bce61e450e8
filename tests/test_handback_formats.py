"""The fired hand-back's six entry points over its four list formats (KWK_COMPACT_REC, _PACKED,
_PACKED16, _BITS in include/kwok_engine.h), at the smallest shapes that can still go wrong: a
partial tile, exactly one tile, and several segments plus a one-object tail, on every state layout
of the pod-fast program and through both compaction paths.  CPU part: the argument checks, which
need no device."""
import ctypes as C

import numpy as np
import pytest

from kwok_amd.host import abi

FORMATS = (abi.COMPACT_REC, abi.COMPACT_PACKED, abi.COMPACT_PACKED16, abi.COMPACT_BITS)
DTYPE = {abi.COMPACT_REC: abi.FIRED_DTYPE, abi.COMPACT_PACKED: np.uint32, abi.COMPACT_PACKED16: np.uint16,
         abi.COMPACT_BITS: np.uint32}
RECORD_BYTES = {abi.COMPACT_REC: 8, abi.COMPACT_PACKED: 4, abi.COMPACT_PACKED16: 2, abi.COMPACT_BITS: 0}
COMPACT_ARG = {abi.COMPACT_REC: False, abi.COMPACT_PACKED: True, abi.COMPACT_PACKED16: "16", abi.COMPACT_BITS: "bits"}
STATES = {"auto": 1, "u16": 2, "u32": 4, "wide": 8}  # Engine(state=...) -> bytes per object of the state stream
HANDBACK_PATHS = (8192, 0)  # KWK_TUNE_COMPACT_SMALL: the one-launch compaction, the scan + expansion pair
SEED, NOW0, DT = 0x6B776F6B, 1_700_000_000 * 10**9, 10**9


# ------------------------------------------------------------------ CPU: argument checks
def test_null_arguments_are_einval_without_a_device():
    """Every entry point refuses a null engine (with and without its other pointers) before it
    touches the device: the library loads and answers on a machine without a GPU."""
    from kwok_amd import build
    build.build()
    L = abi.lib()
    info, p, q, buf = abi.FetchInfo(), C.c_void_p(), C.c_void_p(), (C.c_uint32 * 4)()
    for fmt in FORMATS:
        assert L.kwk_fired_compact(None, fmt) == abi.KWK_EINVAL
        assert L.kwk_fired_read(None, fmt, buf, 16, None, 0, C.byref(info)) == abi.KWK_EINVAL
        assert L.kwk_fired_read(None, fmt, None, 0, None, 0, None) == abi.KWK_EINVAL
        assert L.kwk_fired_device(None, fmt, C.byref(p), C.byref(q)) == abi.KWK_EINVAL
        assert L.kwk_fired_device(None, fmt, None, None) == abi.KWK_EINVAL
    for step in (0, abi.STEP_LAST):
        assert L.kwk_fired_fetch(None, step, buf, 16, None, 0, C.byref(info)) == abi.KWK_EINVAL
        assert L.kwk_fired_fetch(None, step, None, 0, None, 0, None) == abi.KWK_EINVAL
    assert L.kwk_fired_keep(None, 4) == abi.KWK_EINVAL
    assert L.kwk_fired_fetch_wait(None) == abi.KWK_EINVAL
    assert b"null" in L.kwk_last_error(None)


# ------------------------------------------------------------------ GPU: the format matrix
@pytest.fixture(scope="module")
def program():
    from kwok_amd import workload as W
    from kwok_amd.host.compiler import HarnessSpec, KindProgram
    from kwok_amd.host.engine import Ingest
    from kwok_amd.host.stages import load_stage_files
    pvars = [W.pod_object("p", "n"), W.pod_object("p", "n", job=True)]
    prog = KindProgram(load_stage_files(*W.stage_paths(W.POD_FAST)), HarnessSpec())
    prog.explore(pvars)
    return prog, Ingest(prog), pvars


def _engine(program, state, n):
    from bench import shard_pod_variants
    from kwok_amd.host.engine import Engine
    prog, ing, pvars = program
    hot, dels, rec, cls = ing.variant_columns(pvars, shard_pod_variants(0, n, SEED, 0.1))
    eng = Engine(prog, capacity=n, state=state)
    eng.load_stages()
    eng.set_harness(True)
    eng.load(hot, dels, rec, cls, ing.record_array())
    assert eng.stats()["state_bytes"] == STATES[state]
    return eng


def _size(name):
    t = abi.lib().kwk_tile_objects()  # objects per sweep workgroup
    return {"partial": 1000, "tile": t, "segments+1": 3 * t + 1}[name]


def _step_until_fired(eng, k0=0, tries=8):
    for k in range(k0, k0 + tries):
        eng.step(NOW0 + k * DT, SEED, k)
        if len(eng.fired()):
            return k
    raise AssertionError("no step fired an object")


def _decode(fmt, out, cnt, info):
    """(slot, stage, flags or None) of a list as kwk_fired_read returned it."""
    if fmt == abi.COMPACT_REC:
        return out["slot"].astype(np.int64), out["stage"].astype(np.uint32), out["flags"].astype(np.uint32)
    if fmt == abi.COMPACT_PACKED:
        return (out & np.uint32(0x7FFFFFF)).astype(np.int64), out >> np.uint32(27), None
    if fmt == abi.COMPACT_PACKED16:
        return abi.fired16_decode(out, cnt, info.region_slots)
    return abi.bits_decode(out, info.n_segs, info.region_slots) + (None,)


def _check_list(eng, fmt, ref, what):
    """kwk_fired_read(fmt): the reference's (slot, stage) sequence (and flags where carried), a
    consistent kwk_fetch_info."""
    out, cnt, info = eng._read(fmt, DTYPE[fmt])
    slot, stage, flags = _decode(fmt, out, cnt, info)
    assert np.array_equal(slot, ref[0]) and np.array_equal(stage, ref[1]), what
    if flags is not None:
        assert np.array_equal(flags, ref[2]), what
    assert info.format == fmt and info.record_bytes == RECORD_BYTES[fmt] and info.n_records == len(ref[0]), what
    if fmt == abi.COMPACT_BITS:
        assert info.bytes == 4 * len(out), what
        assert int((out[:info.n_segs] & np.uint32(0xFFFF)).astype(np.int64).sum()) == info.n_records, what
    else:
        assert info.bytes == info.n_records * info.record_bytes == out.nbytes, what
    if fmt == abi.COMPACT_PACKED16:
        assert len(cnt) == info.n_segs and int(cnt.sum()) == info.n_records, what
    if fmt in (abi.COMPACT_PACKED16, abi.COMPACT_BITS):
        assert info.n_segs > 0 and info.region_slots > 0, what
    else:
        assert info.n_segs == 0 and info.region_slots == 0, what


def _device_formats(eng):
    """The formats kwk_fired_device accepts now; every other one must be KWK_ESTATE."""
    L, ok = abi.lib(), []
    for g in FORMATS:
        p, q = C.c_void_p(), C.c_void_p()
        st = L.kwk_fired_device(eng.h, g, C.byref(p), C.byref(q))
        assert st in (abi.KWK_OK, abi.KWK_ESTATE), (g, st)
        if st == abi.KWK_OK:
            assert p.value and q.value
            ok.append(g)
    return ok


@pytest.mark.gpu
@pytest.mark.parametrize("size", ["partial", "tile", "segments+1"])
@pytest.mark.parametrize("state", list(STATES))
def test_format_matrix(program, state, size):
    L = abi.lib()
    eng = _engine(program, state, _size(size))
    has16 = state == "auto"  # the 1-byte sweep of the <= 4-stage pod-fast program writes 2-byte records
    try:
        _step_until_fired(eng)
        for path in HANDBACK_PATHS:
            eng.set_tuning(abi.TUNE_COMPACT_SMALL, path)
            eng.fired_compact(False)
            r = eng.fired()
            assert len(r) > 0 and len(np.unique(r["slot"])) == len(r)
            ref = _decode(abi.COMPACT_REC, r, None, None)
            for f in FORMATS:
                what = (state, size, path, f)
                eng.fired_compact(COMPACT_ARG[f])  # falls back to the packed list without 2-byte records
                left = f if has16 or f in (abi.COMPACT_REC, abi.COMPACT_PACKED) else abi.COMPACT_PACKED
                assert _device_formats(eng) == [left], what
                if left != f:
                    info = abi.FetchInfo()
                    st = L.kwk_fired_read(eng.h, f, None, 0, None, 0, C.byref(info))
                    assert st == abi.KWK_ESTATE and b"KWK_COMPACT_PACKED" in L.kwk_last_error(eng.h), what
                    assert _device_formats(eng) == [left], what  # the refused read left the list alone
                    if f == abi.COMPACT_PACKED16:
                        from kwok_amd.host.engine import PinnedBuffer
                        pin = PinnedBuffer(4 * len(r) + 64)
                        got = eng.fetch_async(pin)
                        eng.fetch_wait()
                        assert got["format"] == abi.COMPACT_PACKED and got["n_records"] == len(r), what
                        pk = pin.array(np.uint32, got["n_records"]).copy()
                        pin.close()
                        assert np.array_equal((pk & np.uint32(0x7FFFFFF)).astype(np.int64), ref[0]), what
                    continue
                _check_list(eng, f, ref, what)
                assert _device_formats(eng) == [f], what  # reading the current format compacts nothing
                for g in FORMATS:  # every other format, re-compacted from the intact segments
                    if g == f or (not has16 and g in (abi.COMPACT_PACKED16, abi.COMPACT_BITS)):
                        continue
                    eng.fired_compact(COMPACT_ARG[f])
                    _check_list(eng, g, ref, what + (g,))
                    assert _device_formats(eng) == [g], what + (g,)
        # a null info or out-pointer on a live engine
        p = C.c_void_p()
        assert L.kwk_fired_read(eng.h, abi.COMPACT_REC, None, 0, None, 0, None) == abi.KWK_EINVAL
        assert L.kwk_fired_fetch(eng.h, abi.STEP_LAST, None, 0, None, 0, None) == abi.KWK_EINVAL
        assert L.kwk_fired_device(eng.h, abi.COMPACT_REC, None, C.byref(p)) == abi.KWK_EINVAL
        assert L.kwk_fired_device(eng.h, abi.COMPACT_REC, C.byref(p), None) == abi.KWK_EINVAL
        assert L.kwk_fired_compact(eng.h, 0) == abi.KWK_EINVAL and L.kwk_fired_compact(eng.h, 5) == abi.KWK_EINVAL
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("state", list(STATES))
def test_kept_steps_equal_call_by_call(program, state):
    """kwk_fired_keep(4), then kwk_step_n of 4 steps with KWK_COMPACT_PACKED16 (fused on the 1-byte
    engine; the 4-byte packed list elsewhere): kwk_fired_fetch of each step and of KWK_STEP_LAST equals
    a twin engine stepped and read call by call."""
    from kwok_amd.host.engine import PinnedBuffer
    n = _size("segments+1")
    eng, twin = _engine(program, state, n), _engine(program, state, n)
    has16 = state == "auto"
    pins = [(PinnedBuffer(4 * n + 64), PinnedBuffer(4 * (n // 512 + 64))) for _ in range(5)]
    try:
        k0 = _step_until_fired(eng) + 1
        assert _step_until_fired(twin) + 1 == k0
        eng.fired_keep(4)
        eng.step_n(4, NOW0 + k0 * DT, DT, SEED, k0, "packed16")
        infos = [eng.fetch_step(k0 + j, *pins[j]) for j in range(4)]
        infos.append(eng.fetch_async(*pins[4]))
        eng.fetch_wait()
        assert infos[4] == infos[3]
        fired_any = 0
        for j in range(5):
            jj = min(j, 3)
            if j < 4:
                twin.step(NOW0 + (k0 + j) * DT, SEED, k0 + j)
                want = twin.fired()
            i = infos[j]
            assert i["step"] == k0 + jj and i["n_records"] == len(want), (state, j)
            assert i["format"] == (abi.COMPACT_PACKED16 if has16 else abi.COMPACT_PACKED), (state, j)
            if has16:
                cnt = pins[j][1].array(np.uint32, i["n_segs"])
                sl, sg, fl = abi.fired16_decode(pins[j][0].array(np.uint16, i["n_records"]), cnt, i["region_slots"])
                assert np.array_equal(fl, want["flags"].astype(np.uint32)), (state, j)
            else:
                pk = pins[j][0].array(np.uint32, i["n_records"])
                sl, sg = (pk & np.uint32(0x7FFFFFF)).astype(np.int64), pk >> np.uint32(27)
            assert np.array_equal(sl, want["slot"].astype(np.int64)), (state, j)
            assert np.array_equal(sg, want["stage"].astype(np.uint32)), (state, j)
            fired_any += len(want)
        assert fired_any > 0
    finally:
        for a, b in pins:
            a.close()
            b.close()
        eng.close()
        twin.close()

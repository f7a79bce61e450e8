"""The C ABI of emission from the hand-back ring, on the CPU: the engine's by-step device view
(kwk_ring_view, kwk_fired_view) and the emitter's new calls (kwk_emit_step, kwk_emit_reserve_sets,
kwk_emit_select) exist in the built libraries, refuse null arguments before any device work, and
the Python mirror of kwk_fired_view has the header's layout.  The device paths are checked in
tests/test_gpu_emit_ring.py."""
import ctypes as C
import os
import re
import subprocess
import threading

from kwok_amd.host import abi, emit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EMIT = ("kwk_emit_step", "kwk_emit_reserve_sets", "kwk_emit_select")


def _defined(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return set(re.findall(r" T (kwk_\w+)", out))


def test_new_exports_are_defined_and_declared():
    from kwok_amd import build
    build.build()
    assert "kwk_ring_view" in _defined(abi.LIB_PATH)
    assert set(NEW_EMIT) <= _defined(emit.LIB_PATH)
    assert "kwk_ring_view" in abi.EXPORTS and set(NEW_EMIT) <= set(emit.EXPORTS)
    eng_h = open(os.path.join(ROOT, "include", "kwok_engine.h")).read()
    emit_h = open(os.path.join(ROOT, "include", "kwok_emit.h")).read()
    assert re.search(r"^kwk_status kwk_ring_view\(kwk_engine\* eng, uint64_t step, kwk_fired_view\* out\);", eng_h, re.M)
    for name in NEW_EMIT:
        assert re.search(r"^kwk_status %s\(kwk_emitter\* em, " % name, emit_h, re.M), name


def test_null_arguments_are_einval_without_a_device():
    from kwok_amd import build
    build.build()
    L, E = abi.lib(), emit.lib()
    out = {}

    def calls():  # (a thread of their own: the engine's messages without a handle are kept per thread)
        v = abi.FiredView()
        out["st"] = [L.kwk_ring_view(None, 0, C.byref(v)), L.kwk_ring_view(None, abi.STEP_LAST, None),
                     E.kwk_emit_step(None, 0, 0), E.kwk_emit_reserve_sets(None, 4, 16, 1024), E.kwk_emit_select(None, 0)]
        out["msg"] = (L.kwk_last_error(None), E.kwk_emit_last_error(None))
    t = threading.Thread(target=calls)
    t.start()
    t.join()
    assert out["st"] == [abi.KWK_EINVAL] * 5
    assert out["msg"] == (b"null argument", b"null emitter")


def test_fired_view_layout_matches_header(tmp_path):
    src = tmp_path / "v.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "kwok_emit.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %u\\n", sizeof(kwk_fired_view), '
                   'offsetof(kwk_fired_view, list), offsetof(kwk_fired_view, count), offsetof(kwk_fired_view, seg_counts), '
                   'offsetof(kwk_fired_view, format), offsetof(kwk_fired_view, n_segs), '
                   'offsetof(kwk_fired_view, region_slots), offsetof(kwk_fired_view, step), KWK_ABI_VERSION); return 0; }\n')
    exe = tmp_path / "v"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    F = abi.FiredView
    assert got[:8] == [C.sizeof(F), F.list.offset, F.count.offset, F.seg_counts.offset, F.format.offset, F.n_segs.offset,
                       F.region_slots.offset, F.step.offset]
    assert C.sizeof(F) == 48
    # an additive export: the ABI version and the structs of rounds 7-10 stay
    assert got[8] == 3 == abi.ABI_VERSION
    assert C.sizeof(abi.FetchInfo) == 40 and C.sizeof(abi.FiredRec) == 8 and C.sizeof(emit.EmitItem) == 8

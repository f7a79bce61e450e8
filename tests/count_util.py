"""Host reference and case generators for the count / aggregate kernel tests
(tests/test_gpu_count_variants.py): the numpy reference, the mask sets M1..M16, the object counts
per state format and the dead sets.  Nothing here needs a GPU."""
from __future__ import annotations

import numpy as np

# state= argument of Engine -> bytes per state word on a 16-bit table-only program (pod-fast)
FORMATS = {"auto": 1, "u16": 2, "u32": 4, "dw": 8, "wide": 8}
CHUNKS = (1, 255, 256, 257, 1023, 1024, 1025, 2049)  # 16-byte chunks: a lane's 4 in-flight chunks, blocks 1-3


def ref_counts(pred, alive, masks) -> np.ndarray:
    """counts[k] = alive objects with (pred & masks[k]) != 0; mask 0 counts every alive object."""
    pred = np.asarray(pred, dtype=np.uint32)
    alive = np.asarray(alive, dtype=bool)
    out = np.zeros(len(masks), dtype=np.uint64)
    for k, m in enumerate(masks):
        m = np.uint32(int(m) & 0xFFFFFFFF)
        hit = alive if m == 0 else alive & ((pred & m) != 0)
        out[k] = np.count_nonzero(hit)
    return out


def bits_in_use(pred, alive) -> list:
    """Single-bit masks some alive row has and some alive row lacks (so that no two of the
    interesting counts are trivially 0 or all), lowest bit first."""
    pred = np.asarray(pred, dtype=np.uint32)[np.asarray(alive, dtype=bool)]
    out = []
    for b in range(32):
        c = int(np.count_nonzero(pred & np.uint32(1 << b)))
        if 0 < c < len(pred):
            out.append(1 << b)
    return out


def mask_sets(bits, above) -> dict:
    """M1..M16 from the single-bit masks `bits` (>= 5 of them) and `above`, one bit past the
    program's pred bits (past pmask in the packed formats: class / stage / flag bits lie there,
    and a kernel that forgot `& pmask` would count them).  Mask 0 stands first (M1, M4), in the
    middle (M3, M8, M9, M16) and last (M2); M8 passes one mask twice."""
    assert len(bits) >= 5 and len(set(bits)) == len(bits)
    b = list(bits)
    every = 0xFFFFFFFF
    singles = b[:11]
    m16 = singles + [b[0] | b[1], b[2] | b[3] | b[4], b[1] | b[4], b[0] | b[2] | b[3], b[3] | b[4],
                     b[0] | b[4], b[1] | b[2] | b[3], b[0] | b[3]][:16 - 3 - len(singles)]
    m16 = m16[:7] + [0] + m16[7:] + [every, above]
    assert len(m16) == 16
    return {
        "M1": [0],
        "M2": [b[0], 0],
        "M3": [b[1], 0, b[2] | b[3]],
        "M4": [0, b[0], b[1] | b[2] | b[4], b[3]],
        "M5": [b[0], b[1], b[2], b[3], b[4]],
        "M8": [b[0], b[0], b[1] | b[2], 0, b[3], b[4], every, b[2]],
        "M9": [b[4], b[3], b[2], b[1], b[0], b[0] | b[4], 0, above, b[1] | b[3]],
        "M16": m16,
    }


def sizes(words_per_chunk: int) -> list:
    """n = C * W - r for C in CHUNKS, r in {0, 1, W - 1}, and n = 1, ascending."""
    w = words_per_chunk
    rs = {0, 1} | ({w - 1} if w > 2 else set())
    return sorted({1} | {c * w - r for c in CHUNKS for r in rs if c * w - r >= 1})


def dead_slots(rng, n: int, words_per_chunk: int, case: int) -> np.ndarray:
    """A random fifth of the slots, plus, by the case number, the first object (bit 0), the last
    one (bit 1) and one whole 16-byte chunk (bit 2; the last whole chunk on every other such case)."""
    w = words_per_chunk
    parts = [rng.choice(n, size=n // 5, replace=False)]
    if case & 1:
        parts.append([0])
    if case & 2:
        parts.append([n - 1])
    if case & 4 and n >= w:
        whole = n // w
        c = whole - 1 if case & 8 else int(rng.integers(whole))
        parts.append(np.arange(c * w, c * w + w))
    return np.unique(np.concatenate(parts)).astype(np.uint32)

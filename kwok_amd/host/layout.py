"""Slot layouts for kwk_relayout (include/kwok_engine.h): the mechanism, not the policy.

Pods are node-sorted: node j owns slots [node_ptr[j], node_ptr[j + 1]).  A running engine follows
the cluster by moving whole runs of slots: ``plan_layout`` computes the runs for "these nodes
went away, these were added, this node needs more (or fewer) slots", ``Engine.relayout`` executes
them on the device, and ``apply_moves`` is the same permutation in numpy for every host mirror that
is indexed by slot (names, uids, the emitter's host columns) and for the tests.  When to compact
is the host's decision.
"""
from __future__ import annotations

from typing import Iterable, Optional, Sequence, Tuple

import numpy as np

from . import abi


def as_moves(moves) -> np.ndarray:
    """Rows of abi.MOVE_DTYPE from such rows or from (dst, src, n) triples."""
    if isinstance(moves, np.ndarray) and moves.dtype == abi.MOVE_DTYPE:
        return np.ascontiguousarray(moves)
    out = np.zeros(len(moves), dtype=abi.MOVE_DTYPE)
    for i, (d, s, n) in enumerate(moves):
        out[i] = (d, s, n)
    return out


def _runs(dst: np.ndarray, src: np.ndarray) -> np.ndarray:
    """Single-slot moves dst[i] <- src[i] (dst ascending) merged into maximal runs."""
    if len(dst) == 0:
        return np.zeros(0, dtype=abi.MOVE_DTYPE)
    dst = dst.astype(np.int64)
    src = src.astype(np.int64)
    cut = np.flatnonzero((np.diff(dst) != 1) | (np.diff(src) != 1)) + 1
    start = np.concatenate(([0], cut))
    end = np.concatenate((cut, [len(dst)]))
    out = np.zeros(len(start), dtype=abi.MOVE_DTYPE)
    out["dst"], out["src"], out["n"] = dst[start], src[start], end - start
    return out


def plan_layout(node_ptr, room=None, removed_nodes: Iterable[int] = (), added_nodes: Sequence[int] = (),
                keep: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """-> (moves, node_ptr_new, node_moves) for Engine.relayout.

    The surviving nodes keep their order and the added ones follow them; node j's new range has
    room[j] slots (room is indexed by OLD node; entries of removed nodes are ignored; None keeps
    every range's size), an added node's range added_nodes[k] slots, all fresh.  A surviving node's
    slots move to the front of its new range in their old order — all of them, or with `keep` (a
    bool per old slot) only the kept ones, which compacts the range; slots past the new range's
    size are dropped, and ValueError says so when `keep` names more slots than room[j] holds.
    Removed nodes drop their ranges.  Adjacent single moves are merged, so a node that stays where
    it is costs one identity run and a prefix of such nodes one run."""
    ptr = np.asarray(node_ptr, dtype=np.int64)
    n_nodes = len(ptr) - 1
    size = np.diff(ptr)
    want = size.copy() if room is None else np.asarray(room, dtype=np.int64).copy()
    if len(want) != n_nodes:
        raise ValueError(f"room has {len(want)} entries for {n_nodes} nodes")
    gone = np.zeros(n_nodes, dtype=bool)
    gone[np.asarray(list(removed_nodes), dtype=np.int64)] = True
    surv = np.flatnonzero(~gone)
    new_sizes = np.concatenate((want[surv], np.asarray(added_nodes, dtype=np.int64)))
    if np.any(new_sizes < 0):
        raise ValueError("negative range size")
    new_ptr = np.concatenate(([0], np.cumsum(new_sizes)))
    if new_ptr[-1] >= 1 << 32:
        raise ValueError("more than 2^32 slots")
    node_moves = _runs(np.arange(len(surv)), surv)
    # per old slot: its node, its rank among the node's moving slots
    n_old = int(ptr[-1])
    node_of = np.repeat(np.arange(n_nodes), size)
    moving = ~gone[node_of]
    if keep is not None:
        keep = np.asarray(keep, dtype=bool)
        if len(keep) != n_old:
            raise ValueError(f"keep has {len(keep)} entries for {n_old} slots")
        moving &= keep
    before = np.concatenate(([0], np.cumsum(moving)))  # moving slots before slot i
    rank = before[:-1] - before[ptr[:-1]][node_of]
    if keep is not None:
        counts = before[ptr[1:]] - before[ptr[:-1]]
        over = np.flatnonzero(~gone & (counts > want))
        if len(over):
            j = int(over[0])
            raise ValueError(f"node {j}: {int(counts[j])} slots kept, room for {int(want[j])}")
    moving &= rank < want[node_of]
    new_index = np.full(n_nodes, -1, dtype=np.int64)
    new_index[surv] = np.arange(len(surv))
    src = np.flatnonzero(moving)
    dst = new_ptr[new_index[node_of[src]]] + rank[src]
    return _runs(dst, src), new_ptr.astype(np.uint32), node_moves


def apply_moves(array, moves, n_new: int, fill) -> np.ndarray:
    """The gather kwk_relayout performs, on a host array indexed by slot (or by node): element
    dst + i of the result is array[src + i] for every run, `fill` where no run covers it."""
    array = np.asarray(array)
    out = np.empty((int(n_new),) + array.shape[1:], dtype=array.dtype)
    out[...] = fill
    for m in as_moves(moves):
        d, s, n = int(m["dst"]), int(m["src"]), int(m["n"])
        out[d:d + n] = array[s:s + n]
    return out


def check_moves(moves, n_old: int, n_new: int) -> None:
    """The rules kwk_relayout checks, as ValueError: runs inside the old and the new slots, sorted
    by dst, disjoint in dst and in src."""
    mv = as_moves(moves)
    d, s, n = mv["dst"].astype(np.int64), mv["src"].astype(np.int64), mv["n"].astype(np.int64)
    if np.any(s + n > n_old) or np.any(d + n > n_new):
        raise ValueError("a run outside the old or the new slots")
    if np.any(np.diff(d) < 0) or np.any((d + n)[:-1] > d[1:]):
        raise ValueError("runs unsorted by dst or overlapping in dst")
    nz = n > 0
    o = np.argsort(s[nz], kind="stable")
    ss, nn = s[nz][o], n[nz][o]
    if np.any((ss + nn)[:-1] > ss[1:]):
        raise ValueError("runs overlapping in src")

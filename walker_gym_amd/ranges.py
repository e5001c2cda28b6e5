"""Walker ranges: how BatchedPhysicsEnv splits a batch into the contiguous pieces it steps on separate streams, and the
one description of such a piece (WalkerRange, built by BatchedPhysicsEnv._ranges).  numpy and ints only."""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np


class WalkerRange(NamedTuple):
    batch: object              # WgBatch: the range's view of a uniform batch, or a ragged batch's one struct
    outputs: object            # WgOutputs: o_full advanced to the range's first walker, or o_full itself (ragged)
    plan: Optional[int]        # device address of the range's slice of the block -> walker plan, or None
    plan_blocks: int
    action_offset: int         # elements from the start of a whole-batch [N, cols] action tensor to the range's rows
    row0: int                  # first caller row (ragged: first stored walker, a caller row where `contiguous`)
    n: int                     # walkers
    contiguous: Optional[bool]  # the walkers are caller rows row0 .. row0 + n - 1 (None: not determined)
    slot: int                  # stream slot: 0 the calling stream, i the env's side stream i - 1


def uniform_bounds(N: int, lanes: int) -> list:
    """Walker bounds of `lanes` ranges of a uniform batch of N, the inner ones on multiples of 64."""
    return [0] + [((N * i // lanes) + 63) // 64 * 64 for i in range(1, lanes)] + [N]


def block_bounds(plan_blocks: int, lanes: int) -> list:
    """Plan-block bounds of `lanes` even ranges of a ragged batch's plan."""
    return [plan_blocks * i // lanes for i in range(lanes)] + [plan_blocks]


def caller_bounds(plan_blocks: int, plan_host, row, lanes: int):
    """block_bounds with each split moved to the nearest block whose stored prefix holds exactly the caller rows before
    it (within an eighth of a range), and per range whether its walkers are a contiguous slice of caller rows.
    plan_host: block -> first stored walker; row: caller row of each stored walker (None: identity order)."""
    nb = plan_blocks
    if row is None:
        ok = np.ones(nb + 1, bool)   # identity order: every block boundary
    else:
        rowmax = np.maximum.accumulate(row)
        ok = np.zeros(nb + 1, bool)
        ok[0] = ok[nb] = True
        s = np.asarray(plan_host[1:nb]).astype(np.int64)
        ok[1:nb] = rowmax[s - 1] == s - 1
    good = np.flatnonzero(ok)
    even = block_bounds(nb, lanes)
    bb = [0]
    for t in even[1:-1]:
        c = int(good[np.argmin(np.abs(good - t))])
        bb.append(c if abs(c - t) <= max(1, nb // (8 * lanes)) and bb[-1] < c < nb else t)
    bb.append(nb)
    contiguous = [bool(ok[bb[i]] and ok[bb[i + 1]]) for i in range(lanes)]
    return bb, contiguous

"""Seeded segment tables for wg_adam_step (tests/test_optim_cpu.py, tests/test_gpu_optim.py): segment counts 1, 2, 7
and 32; lengths on both sides of the lane count (256) and of the chunk (4096); a chunk edge inside a segment and one
exactly at a segment's end; tables of ten chunks (the fused kernel's second round of four) and of about 2^20 elements.

A segment's four arrays start `off` floats past a 16-byte boundary (param, grad, m, v): (0, 0, 0, 0) is the 16-byte path
from the first element, (1, 1, 1, 1) the 16-byte path behind a scalar head, and unequal offsets the scalar path.
The reference is computed once per (table, variant) and shared."""
import functools

import numpy as np

from walker_gym_amd import optim

f32 = np.float32
STEPS = 3
ALIGNED, SHIFTED, MIXED = (0, 0, 0, 0), (1, 1, 1, 1), (1, 0, 2, 3)

# name -> [(length, offsets)]
TABLES = {
    "one-1": [(1, ALIGNED)],
    "one-255": [(255, SHIFTED)],
    "one-256": [(256, ALIGNED)],
    "one-257": [(257, MIXED)],
    "one-4095": [(4095, ALIGNED)],
    "one-4096": [(4096, SHIFTED)],
    "one-4097": [(4097, (3, 3, 3, 3))],
    "two-edge-inside": [(5000, SHIFTED), (3001, ALIGNED)],              # 4096 falls inside segment 0
    "two-edge-at-end": [(4096, ALIGNED), (100, MIXED)],                 # 4096 is segment 0's end
    "seven": [(1, ALIGNED), (255, SHIFTED), (256, MIXED), (257, (2, 2, 2, 2)), (4095, ALIGNED), (4097, SHIFTED),
              (33, (0, 1, 0, 1))],
    "thirty-two": [(1 + (37 * i * i + 11 * i) % 601, (ALIGNED, SHIFTED, MIXED, (2, 2, 2, 2))[i % 4]) for i in range(32)],
    "two-ten-chunks": [(20000, ALIGNED), (20001, SHIFTED)],
    "big": [(600001, ALIGNED), (448575, SHIFTED), (13, MIXED)],          # 1,048,589 elements, 257 chunks
}
NAMES = tuple(TABLES)
BOTH_PATHS = tuple(n for n in NAMES if n != "big")   # small enough to run fused and in three launches

# clip active / inactive, weight decay, maximize
VARIANTS = {f"{'clip' if c else 'noclip'}-{'wd' if w else 'nowd'}-{'max' if m else 'min'}": (c, w, m)
            for c in (True, False) for w in (True, False) for m in (False, True)}


def config(variant: str) -> dict:
    clip, wd, mx = VARIANTS[variant]
    return optim.adam_config(lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01 if wd else 0.0,
                             max_norm=1e-3 if clip else 1e9, maximize=mx)


def total(name: str) -> int:
    return sum(n for n, _ in TABLES[name])


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same(a, b) -> bool:
    """Bit for bit, a NaN equal to any NaN."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    na, nb = np.isnan(a), np.isnan(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(na, nb) and \
        np.array_equal(bits(a)[~na], bits(b)[~nb])


@functools.lru_cache(maxsize=None)
def inputs(name: str) -> dict:
    """params, m, v (a run already under way: m of both signs, v >= 0) and STEPS gradients per segment."""
    rng = np.random.default_rng(1000 + NAMES.index(name))
    lens = [n for n, _ in TABLES[name]]
    d = {"params": [rng.standard_normal(n).astype(f32) for n in lens],
         "m": [(0.1 * rng.standard_normal(n)).astype(f32) for n in lens],
         "v": [(0.01 * rng.standard_normal(n) ** 2).astype(f32) for n in lens],
         "grads": [[(rng.standard_normal(n) * 10.0 ** rng.uniform(-1, 1)).astype(f32) for n in lens] for _ in range(STEPS)]}
    for a in d["params"] + d["m"] + d["v"] + [g for step in d["grads"] for g in step]:
        a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def reference(name: str, variant: str):
    """After each of STEPS steps from a zeroed state: (params, m, v, state), copies."""
    d, cfg = inputs(name), config(variant)
    p, m, v = ([a.copy() for a in d[k]] for k in ("params", "m", "v"))
    state = np.zeros(optim.STATE_LEN, np.float64)
    out = []
    for s in range(STEPS):
        optim.adam_step_numpy(p, d["grads"][s], m, v, state, cfg)
        out.append(([a.copy() for a in p], [a.copy() for a in m], [a.copy() for a in v], state.copy()))
    return out


# the special gradients: name -> (g, v0); one segment of four elements, the first carries the case
SPECIALS = {
    "zero-g-zero-v": (0.0, 0.0),
    "denormal-square": (1e-20, 0.0),
    "vanishing-square": (1e-30, 0.0),
    "overflowing-square": (1e20, 0.0),
}

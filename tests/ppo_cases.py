"""Shared shapes and inputs of the wg_expf / wg_ppo_surrogate tests (test_ppo_cpu.py, test_gpu_ppo.py): the smallest
shapes at which the surrogate kernel can go wrong.  act_dim in {1, 3, 4, 8} (the scalar and the 16-byte load paths),
n_sets in {1, 2, N}, T * n in {1, 63, 64, 65, 255, 256, 257} against chunk_rows in {1, 7, 256}: a single chunk, a ragged
last chunk, several chunks, a tile that is exactly full and one row over.  The rows look like recorded ones:
u = RN32(y + RN32(sigma * aeps)) with aeps from pg.action_noise_numpy."""
import functools
from collections import namedtuple

import numpy as np

from walker_gym_amd import pg

f32 = np.float32
Shape = namedtuple("Shape", "name T N G C")

SHAPES = [Shape("rows1", 1, 1, 1, 1), Shape("rows1-2sets", 1, 2, 2, 3), Shape("rows63", 3, 21, 1, 3),
          Shape("rows64-2sets", 4, 32, 2, 4), Shape("rows65", 5, 13, 1, 8), Shape("rows255-2sets", 5, 102, 2, 1),
          Shape("rows256", 4, 64, 1, 4), Shape("rows257", 1, 257, 1, 8), Shape("rows257-2sets", 1, 514, 2, 3),
          Shape("set-per-walker", 5, 7, 7, 4)]
NAMES = [s.name for s in SHAPES]
CHUNKS = (1, 7, 256)
CPU_NAMES = ["rows1", "rows1-2sets", "rows65", "rows64-2sets", "set-per-walker"]   # the scalar loop's subset
CLIP = 0.2
STRUCTURED_LO, STRUCTURED_HI = -104.0, 89.0


def shape_of(name) -> Shape:
    return SHAPES[NAMES.index(name)]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


@functools.lru_cache(maxsize=None)
def inputs(name, seed=0):
    """Finite rows of shape `name`: y, u, sigma, log_sigma, old_logp, adv, value, ret, mask (uint8, about 2/3 on) and
    scale (float32 [2]).  old_logp sits near logp so that some rows are clipped on either side and some are not.
    Computed once per shape; callers copy before they write."""
    s = shape_of(name)
    rng = np.random.default_rng(1000 + NAMES.index(name) + 97 * seed)
    y = rng.normal(0.0, 0.5, (s.T, s.N, s.C)).astype(f32)
    sigma = rng.uniform(0.2, 2.0, (s.G, s.C)).astype(f32)
    log_sigma = np.log(sigma.astype(np.float64)).astype(f32)
    aeps = pg.action_noise_numpy(7 + seed, 3, s.T, 11, s.N, s.C)
    sets = np.arange(s.N) // (s.N // s.G)
    u = (y + (sigma[sets][None] * aeps).astype(f32)).astype(f32)
    logp = pg.ppo_surrogate_numpy(y, u, sigma, log_sigma)["logp"]
    old_logp = (logp - rng.choice([-0.5, -0.05, 0.0, 0.05, 0.5], (s.T, s.N)) * rng.uniform(0.5, 1.0, (s.T, s.N))).astype(f32)
    adv = (rng.normal(0.0, 1.0, (s.T, s.N))).astype(f32)
    value = rng.normal(0.0, 1.0, (s.T, s.N)).astype(f32)
    ret = rng.normal(0.0, 1.0, (s.T, s.N)).astype(f32)
    mask = (rng.uniform(size=(s.T, s.N)) < 0.67).astype(np.uint8)
    mask.flat[0], mask.flat[-1] = 0, 1      # (a single row: on)
    cnt = max(int(mask.sum()), 1)
    out = dict(y=y, u=u, sigma=sigma, log_sigma=log_sigma, old_logp=old_logp, adv=adv, value=value, ret=ret, mask=mask,
               scale=np.array([-1.0 / cnt, 1.0 / cnt], f32))
    for v in out.values():
        v.setflags(write=False)
    return out


def poisoned(inp):
    """The rows the mask skips overwritten with NaN in every per-row input: a skipped row is never looked at."""
    out = {k: v.copy() for k, v in inp.items()}
    off = inp["mask"] == 0
    for k in ("y", "u"):
        out[k][off] = np.nan
    for k in ("old_logp", "adv", "value", "ret"):
        out[k][off] = np.nan
    return out


@functools.lru_cache(maxsize=None)
def reference(name, chunk_rows, masked=True, with_value=True):
    """pg.ppo_surrogate_numpy of inputs(name), the rows behind the mask poisoned; computed once."""
    inp = poisoned(inputs(name)) if masked else inputs(name)
    return pg.ppo_surrogate_numpy(inp["y"], inp["u"], inp["sigma"], inp["log_sigma"], inp["old_logp"], inp["adv"],
                                  inp["mask"] if masked else None, CLIP, inp["scale"],
                                  inp["value"] if with_value else None, inp["ret"] if with_value else None, chunk_rows)


def structured_patterns():
    """The 2 * 2^20 float32 patterns i << 12 and (i << 12) | 0xFFF, those within [-104, 89]."""
    i = np.arange(1 << 20, dtype=np.uint32) << np.uint32(12)
    x = np.concatenate([i, i | np.uint32(0xFFF)]).view(f32)
    return x[(x >= f32(STRUCTURED_LO)) & (x <= f32(STRUCTURED_HI))]


def seeded_sample(scale=1):
    """default_rng(0): 4 M uniform in [-104, 89], 4 M uniform in [-1, 1], 2 M normal with sd 1e-3 (divided by `scale`)."""
    rng = np.random.default_rng(0)
    m = 1_000_000 // scale
    return np.concatenate([rng.uniform(-104, 89, 4 * m), rng.uniform(-1, 1, 4 * m), rng.normal(0, 1e-3, 2 * m)]).astype(f32)


SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, 88.72283, 88.72284, -103.9, -104.0, -87.33655, -87.33656, 1.0, -1.0,
                     150.0, -150.0, 151.0, 3.4e38, -3.4e38, 1e-45, -1e-45, 0.34657359, -0.34657359], f32)
NAN_BITS = np.array([0x7FC00000, 0xFFC00000, 0x7FC12345, 0x7F800001, 0xFFFFFFFF], np.uint32)

#!/usr/bin/env python3
"""A/B of the fused auto-reset (ABI 16) on the canonical workload: 65,536 walkers, max_steps = 64 with the walkers' step
counters staggered (1/64 of the batch ends an episode at every step), 1,000 steps, three ways:

  (a) run() with auto-reset off (episodes simply run on: the plain step's rate);
  (b) run() with auto-reset on (done), reset noise from a two-row pool;
  (c) a closed step() loop with the reset composed on the host side, stream-ordered and without a host sync: a masked
      restore of pos / vel / acc / muscle_x from a snapshot, a torch.randn over [P, 3], reset(noise, mask) = wg_reset of
      the done walkers + the closing observe().

The three are timed in turn, `--reps` times each (interleaved, so clock and thermal drift fall on all alike), each
timing a whole call between two synchronisations; the result is the median ms per step of each and the ratios (b)/(a)
and (c)/(b), as one JSON line (and --out FILE).

    python scripts/autoreset_ab.py [--n 65536] [--steps 1000] [--reps 3] [--out profiles/r08_autoreset_ab.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from walker_gym_amd.batched_env import BatchedPhysicsEnv   # noqa: E402
from walker_gym_amd.synthetic import canonical_walkers     # noqa: E402

MAX_STEPS = 64


def make_env(n, auto):
    spec = dict(canonical_walkers(n, seed=0))
    spec["steps"] = (np.arange(n) % MAX_STEPS).astype(np.int32)
    env = BatchedPhysicsEnv(spec, in3d=1, max_steps=MAX_STEPS, rand_sigma=0.1, seed=1)
    if auto:
        env.enable_auto_reset(on=("done",), noise_rows=2)
    return env


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def host_reset_loop(env, snap, action, steps):
    """(c): step, then put the done walkers back from the host side (no host sync: the mask stays on the device)."""
    b = env.batch
    M, A = b.M, b.A
    for _ in range(steps):
        _, _, done, _ = env.step(action)
        mm = done.repeat_interleave(M)[:, None]
        b.pos.copy_(torch.where(mm, snap["pos"], b.pos.view(-1, 3)).view(b.pos.shape))
        b.vel.copy_(torch.where(mm, snap["vel"], b.vel.view(-1, 3)).view(b.vel.shape))
        b.acc.copy_(torch.where(mm, snap["acc"], b.acc.view(-1, 3)).view(b.acc.shape))
        b.muscle_x.copy_(torch.where(done.repeat_interleave(A), snap["muscle_x"], b.muscle_x))
        env.reset(mask=done)   # randn * sigma over [P, 3], wg_reset(mask), observe()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    off, on, host = make_env(a.n, False), make_env(a.n, True), make_env(a.n, False)
    dev = off.device
    act = (torch.rand((1, a.n, off.batch.A), device=dev) * 2 - 1).contiguous()
    snap = {k: getattr(host.batch, k).clone().view(-1, 3) if k != "muscle_x" else host.batch.muscle_x.clone()
            for k in ("pos", "vel", "acc", "muscle_x")}
    runs = {
        "a_off": lambda: off.run(act, a.steps),
        "b_auto_reset": lambda: on.run(act, a.steps),
        "c_host_reset": lambda: host_reset_loop(host, snap, act[0], a.steps),
    }
    for fn in runs.values():   # warm-up: one whole call each (allocator, streams, clocks)
        timed(fn)
    ms = {k: [] for k in runs}
    for _ in range(a.reps):
        for k, fn in runs.items():
            ms[k].append(1e3 * timed(fn) / a.steps)
    med = {k: statistics.median(v) for k, v in ms.items()}
    episodes = on.batch.episodes
    res = {"workload": f"canonical x {a.n}, max_steps {MAX_STEPS} staggered, {a.steps} steps per call",
           "ms_per_step": ms, "median_ms_per_step": med,
           "env_steps_per_s": {k: a.n / (v * 1e-3) for k, v in med.items()},
           "b_over_a": med["b_auto_reset"] / med["a_off"], "c_over_b": med["c_host_reset"] / med["b_auto_reset"],
           "spread_a": max(ms["a_off"]) / min(ms["a_off"]),
           "episodes_per_walker_b": float(episodes.float().mean()),
           "nonfinite_walkers": {"a_off": int((~torch.isfinite(off.batch.pos.view(a.n, -1)).all(1)).sum()),
                                 "b_auto_reset": int((~torch.isfinite(on.batch.pos.view(a.n, -1)).all(1)).sum())},
           "device": torch.cuda.get_device_name(dev)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

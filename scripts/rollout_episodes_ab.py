#!/usr/bin/env python3
"""A/B of the multi-episode closed-loop rollout (BatchedPhysicsEnv.rollout_episodes, one wg_rollout_episodes launch per
call) against the closed loop with resets the package had before it, one box, one process:

  (a) policy_loop(graph=True), auto-reset on: one step launch plus the policy's launches per step, as captured HIP
      graphs, the replay timed (capture excluded); the policy written as a user would, clamp(relu(obs @ w1 + b1) @ w2 + b2)
  (b) rollout_episodes, every per-step buffer (obs, reward, done, action, reset, final_obs)
  (c) rollout_episodes, no per-step buffer (the episode statistics only)
  (d) rollout_policy, auto-reset off: the same kernel without the reset tail, the tail's cost floor
  (e) rollout(resident=True), open loop with precomputed actions, auto-reset on: the resident kernel's AR twin
  (f) rollout(resident=False, lanes=1), auto-reset on: one wg_step launch per step, which is what wg_rollout ran under
      auto-reset before the twin existed (the same launches in the same order)

Workloads: Balance-v0 x 4,096 and canonical x 65,536, policies H = 0 and H = 32 (one shared parameter set), max_steps =
64 with the walkers' step counters staggered by w % 64, so that 1/64 of the walkers end an episode at every step; a
two-row reset-noise pool.  Every call starts from the same entry state, snapshot and episode counts (restored and
observed before the clock starts).  After a warm-up call of every path the paths are timed in turn, `--reps` times
(interleaved, so clock and thermal drift fall on all alike), each timing a whole call between two synchronisations.
Per row and path: median, min and max ms per step, and max / min.

    python scripts/rollout_episodes_ab.py [--steps 200] [--reps 5] [--out profiles/r09_rollout_episodes_ab.json]
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
from walker_gym_amd.policy import MLPPolicy                # noqa: E402
from walker_gym_amd.synthetic import canonical_walkers     # noqa: E402
from walker_gym_amd.walker import balance_spec             # noqa: E402


STATE = ("pos", "vel", "acc", "muscle_x", "steps", "episodes")
MAX_STEPS = 64


def timed(fn, env, snap):
    for k in STATE:   # the same start for every call, outside the clock
        if getattr(env.batch, k, None) is not None:
            getattr(env.batch, k).copy_(snap[k])
    env.observe()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def weights(D, H, C, dev, seed):
    g = torch.Generator().manual_seed(seed)
    s = 0.008 if H else 0.001
    rn = lambda *shape: torch.randn(shape, generator=g)
    w1 = (rn(1, D, H) * s).to(dev) if H else None
    b1 = (rn(1, H) * s).to(dev) if H else None
    w2 = (rn(1, H if H else D, C) * (4 * s if H else s)).to(dev)
    b2 = (rn(1, C) * s).to(dev)
    return w2, b2, w1, b1


def row(name, spec, params, H, steps, reps):
    spec = dict(spec)
    n = len(spec["mass_off"]) - 1
    spec["steps"] = (np.arange(n) % MAX_STEPS).astype(np.int32)
    envs = {k: BatchedPhysicsEnv(spec, rand_sigma=0.01, seed=1, max_steps=MAX_STEPS, **params) for k in "abcdef"}
    for k, e in envs.items():
        if k != "d":
            e.enable_auto_reset(noise_rows=2, final_obs=(k == "a"))
    e0 = envs["b"]
    dev, N, D, A = e0.device, e0.N, e0.obs_dim, e0.batch.A
    w2, b2, w1, b1 = weights(D, H, A, dev, seed=H + 1)
    pol = MLPPolicy(w2, b2, w1, b1, act_limit=1.0)

    def user_policy(rows, t):   # what a user of policy_loop writes
        x = torch.relu(rows @ w1[0] + b1[0]) if H else rows
        return torch.clamp(x @ w2[0] + b2[0], -1.0, 1.0)

    buf = dict(obs_out=torch.empty((steps, N, D), device=dev), reward_out=torch.empty((steps, N), device=dev),
               done_out=torch.empty((steps, N), dtype=torch.uint8, device=dev),
               action_out=torch.empty((steps, N, A), device=dev))
    ar_buf = dict(reset_out=torch.empty((steps, N), dtype=torch.uint8, device=dev),
                  final_obs_out=torch.empty((steps, N, D), device=dev))
    acts = (torch.rand((steps, N, A), device=dev) * 2 - 1).contiguous()
    snap = {k: {s: getattr(e.batch, s).clone() for s in STATE if getattr(e.batch, s, None) is not None}
            for k, e in envs.items()}
    for e in envs.values():
        e.observe()
    # (the BLAS library initialises at its first matmul of a shape, which a capture forbids: one eager step first)
    envs["a"].policy_loop(user_policy, 1)
    torch.cuda.synchronize()
    graph = envs["a"].policy_loop(user_policy, steps, graph=True)   # capture (and one replay) outside the timing
    runs = {
        "a_policy_loop_graph_autoreset": graph.replay,
        "b_episodes_all_buffers": lambda: envs["b"].rollout_episodes(pol, steps, **buf, **ar_buf),
        "c_episodes_no_buffers": lambda: envs["c"].rollout_episodes(pol, steps),
        "d_rollout_policy_no_autoreset": lambda: envs["d"].rollout_policy(pol, steps),
        "e_open_loop_resident_autoreset": lambda: envs["e"].rollout(acts, buf["obs_out"], buf["reward_out"],
                                                                    buf["done_out"], resident=True),
        "f_open_loop_per_step_autoreset": lambda: envs["f"].rollout(acts, buf["obs_out"], buf["reward_out"],
                                                                    buf["done_out"], resident=False, lanes=1),
    }
    for k, fn in runs.items():   # warm-up: one whole call each
        timed(fn, envs[k[0]], snap[k[0]])
    ms = {k: [] for k in runs}
    for _ in range(reps):
        for k, fn in runs.items():   # (a run's env is named by the first letter of its key)
            ms[k].append(1e3 * timed(fn, envs[k[0]], snap[k[0]]) / steps)
    stat = {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "spread": max(v) / min(v)}
            for k, v in ms.items()}
    a = ms["a_policy_loop_graph_autoreset"]
    res = {"row": name, "N": N, "D": D, "H": H, "C": A, "steps_per_call": steps, "max_steps": MAX_STEPS,
           "ms_per_step": stat, "launch_geometry": e0.launch_geometry(),
           "episodes_after_one_call": {k: int(e.batch.episodes.sum()) for k, e in envs.items() if k != "d"},
           "nonfinite_walkers_after_one_call": {k: int((~torch.isfinite(e.batch.pos.view(N, -1)).all(1)).sum())
                                                for k, e in envs.items()},
           "c_slowest_below_a_fastest": max(ms["c_episodes_no_buffers"]) < min(a),
           "b_slowest_below_a_fastest": max(ms["b_episodes_all_buffers"]) < min(a),
           "c_over_a": stat["c_episodes_no_buffers"]["median"] / stat["a_policy_loop_graph_autoreset"]["median"],
           "c_over_d": stat["c_episodes_no_buffers"]["median"] / stat["d_rollout_policy_no_autoreset"]["median"],
           "e_over_f": stat["e_open_loop_resident_autoreset"]["median"] /
                       stat["f_open_loop_per_step_autoreset"]["median"]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    bal, can = balance_spec(4096), canonical_walkers(65536, seed=0)
    rows = []
    for H in (0, 32):
        rows.append(row(f"balance4096-H{H}", bal, dict(in3d=0), H, a.steps, a.reps))
        rows.append(row(f"canonical65536-H{H}", can, dict(in3d=1), H, a.steps, a.reps))
    res = {"rows": rows, "device": torch.cuda.get_device_name(0), "reps": a.reps,
           "method": "one process, warm-up call of every path, then the paths timed in turn reps times; ms per step = "
                     "wall time of a whole call between two synchronisations / steps; every call from the same entry "
                     "state, snapshot and episode counts"}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""A/B of the stochastic closed-loop rollout (BatchedPhysicsEnv.rollout_stochastic, one wg_rollout_stochastic launch per
call) against what a user had before it, and of the GAE kernel (wg_gae) against the torch backward loop; one box, one
process, the protocol of scripts/rollout_episodes_ab.py:

  (a) policy_loop(graph=True), auto-reset on, with a policy callable that adds sigma * torch.randn to its outputs: one
      step launch plus the policy's launches per step, as captured HIP graphs, the replay timed (capture excluded)
  (b) rollout_stochastic with the PPO buffers (obs, reward, done, steps, action, raw action, aeps, reset, final_obs)
  (c) rollout_stochastic with no per-step buffer
  (d) rollout_episodes with no per-step buffer: the deterministic floor ((c) / (d) is the noise's own cost)

Rows: Balance-v0 x 4,096 and canonical x 65,536, policies H = 0 and H = 32 (one shared parameter set), max_steps = 64
with the walkers' step counters staggered by w % 64, a two-row reset-noise pool.  Every call starts from the same entry
state, snapshot and episode counts.  After a warm-up call of every path the paths are timed in turn, `--reps` times
(interleaved), each timing a whole call between two synchronisations.  Per row and path: median, min and max ms per step.

GAE: T = 200, N = 4,096 and 65,536, term and cut set on 1/64 of the elements: pg.gae (one launch) against the loop a
user writes in torch (T iterations of elementwise operations), the same protocol; the kernel's time against the bytes
it moves (14 B read and 8 B written per element) at 6.3 TB/s.

    python scripts/stochastic_rollout_ab.py [--steps 200] [--reps 5] [--out profiles/r11_stochastic_rollout_ab.json]
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

from walker_gym_amd import pg                              # noqa: E402
from walker_gym_amd.batched_env import BatchedPhysicsEnv   # noqa: E402
from walker_gym_amd.policy import MLPPolicy                # noqa: E402
from walker_gym_amd.synthetic import canonical_walkers     # noqa: E402
from walker_gym_amd.walker import balance_spec             # noqa: E402

STATE = ("pos", "vel", "acc", "muscle_x", "steps", "episodes")
MAX_STEPS = 64
SIGMA = 0.1
HBM_BYTES_PER_S = 6.3e12


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


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "spread": max(v) / min(v)}


def row(name, spec, params, H, steps, reps):
    spec = dict(spec)
    n = len(spec["mass_off"]) - 1
    spec["steps"] = (np.arange(n) % MAX_STEPS).astype(np.int32)
    envs = {k: BatchedPhysicsEnv(spec, rand_sigma=0.01, seed=1, max_steps=MAX_STEPS, **params) for k in "abcd"}
    for k, e in envs.items():
        e.enable_auto_reset(noise_rows=2, final_obs=(k == "a"))
    e0 = envs["b"]
    dev, N, D, A = e0.device, e0.N, e0.obs_dim, e0.batch.A
    w2, b2, w1, b1 = weights(D, H, A, dev, seed=H + 1)
    pol = MLPPolicy(w2, b2, w1, b1, act_limit=1.0)
    sigma = torch.full((1, A), SIGMA, device=dev)

    def user_policy(rows, t):   # what a user of policy_loop writes to explore
        x = torch.relu(rows @ w1[0] + b1[0]) if H else rows
        y = x @ w2[0] + b2[0]
        return torch.clamp(y + SIGMA * torch.randn_like(y), -1.0, 1.0)

    f = lambda *s: torch.empty(s, device=dev)
    u8 = lambda *s: torch.empty(s, dtype=torch.uint8, device=dev)
    buf = dict(obs_out=f(steps, N, D), reward_out=f(steps, N), done_out=u8(steps, N),
               steps_out=torch.empty((steps, N), dtype=torch.int32, device=dev), action_out=f(steps, N, A),
               raw_action_out=f(steps, N, A), eps_out=f(steps, N, A), reset_out=u8(steps, N),
               final_obs_out=f(steps, N, D))
    snap = {k: {s: getattr(e.batch, s).clone() for s in STATE if getattr(e.batch, s, None) is not None}
            for k, e in envs.items()}
    for e in envs.values():
        e.observe()
    envs["a"].policy_loop(user_policy, 1)   # (the BLAS library initialises at its first matmul: one eager step first)
    torch.cuda.synchronize()
    graph = envs["a"].policy_loop(user_policy, steps, graph=True)   # capture (and one replay) outside the timing
    runs = {
        "a_policy_loop_graph_randn": graph.replay,
        "b_stochastic_ppo_buffers": lambda: envs["b"].rollout_stochastic(pol, steps, sigma, 1, **buf),
        "c_stochastic_no_buffers": lambda: envs["c"].rollout_stochastic(pol, steps, sigma, 1),
        "d_episodes_no_buffers": lambda: envs["d"].rollout_episodes(pol, steps),
    }
    for k, fn in runs.items():   # warm-up: one whole call each
        timed(fn, envs[k[0]], snap[k[0]])
    ms = {k: [] for k in runs}
    for _ in range(reps):
        for k, fn in runs.items():   # (a run's env is named by the first letter of its key)
            ms[k].append(1e3 * timed(fn, envs[k[0]], snap[k[0]]) / steps)
    stat = {k: stats(v) for k, v in ms.items()}
    a = ms["a_policy_loop_graph_randn"]
    return {"row": name, "N": N, "D": D, "H": H, "C": A, "steps_per_call": steps, "max_steps": MAX_STEPS, "sigma": SIGMA,
            "ms_per_step": stat, "launch_geometry": e0.launch_geometry(),
            "episodes_after_one_call": {k: int(e.batch.episodes.sum()) for k, e in envs.items()},
            "nonfinite_walkers_after_one_call": {k: int((~torch.isfinite(e.batch.pos.view(N, -1)).all(1)).sum())
                                                 for k, e in envs.items()},
            "c_slowest_below_a_fastest": max(ms["c_stochastic_no_buffers"]) < min(a),
            "b_slowest_below_a_fastest": max(ms["b_stochastic_ppo_buffers"]) < min(a),
            "c_over_a": stat["c_stochastic_no_buffers"]["median"] / stat["a_policy_loop_graph_randn"]["median"],
            "b_over_a": stat["b_stochastic_ppo_buffers"]["median"] / stat["a_policy_loop_graph_randn"]["median"],
            "c_over_d": stat["c_stochastic_no_buffers"]["median"] / stat["d_episodes_no_buffers"]["median"]}


def gae_torch_loop(r, v, nv, term, cut, gamma, lam):
    """The backward scan as a user writes it in torch: T iterations of a few elementwise launches."""
    T = r.shape[0]
    adv = torch.empty_like(r)
    carry = torch.zeros_like(r[0])
    nt, nc = 1.0 - term.float(), 1.0 - cut.float()
    for t in range(T - 1, -1, -1):
        delta = r[t] + gamma * nv[t] * nt[t] - v[t]
        carry = delta + gamma * lam * nc[t] * carry
        adv[t] = carry
    return adv, adv + v


def gae_row(N, T, reps, dev):
    g = torch.Generator().manual_seed(N)
    rn = lambda: torch.randn((T, N), generator=g).to(dev)
    r, v, nv = rn(), rn(), rn()
    term = (torch.rand((T, N), generator=g) < 1 / 64).to(torch.uint8).to(dev)
    cut = (term | (torch.rand((T, N), generator=g) < 1 / 64).to(torch.uint8).to(dev)).contiguous()
    adv, ret = torch.empty_like(r), torch.empty_like(r)
    runs = {"kernel": lambda: pg.gae(r, v, nv, term, cut, 0.99, 0.95, adv_out=adv, ret_out=ret),
            "torch_loop": lambda: gae_torch_loop(r, v, nv, term, cut, 0.99, 0.95)}

    def once(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)
    for fn in runs.values():
        once(fn)
    ms = {k: [] for k in runs}
    for _ in range(reps):
        for k, fn in runs.items():
            ms[k].append(once(fn))
    # the kernel alone, by device events over 20 back-to-back launches (the wall time above holds a launch and a sync)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        runs["kernel"]()
    e1.record()
    torch.cuda.synchronize()
    dev_ms = e0.elapsed_time(e1) / 20
    ka, kr = pg.gae(r, v, nv, term, cut, 0.99, 0.95)
    la, lr_ = gae_torch_loop(r, v, nv, term, cut, 0.99, 0.95)
    nbytes = 22 * T * N
    return {"N": N, "T": T, "ms_per_call": {k: stats(v) for k, v in ms.items()},
            "kernel_slowest_below_loop_fastest": max(ms["kernel"]) < min(ms["torch_loop"]),
            "loop_over_kernel": statistics.median(ms["torch_loop"]) / statistics.median(ms["kernel"]),
            "kernel_ms_back_to_back": dev_ms, "bytes_moved": nbytes,
            "ms_at_6.3_TB_per_s": 1e3 * nbytes / HBM_BYTES_PER_S,
            "fraction_of_6.3_TB_per_s": (nbytes / HBM_BYTES_PER_S) / (dev_ms * 1e-3),
            "max_abs_difference_to_the_loop": float((ka - la).abs().max()),
            "note": "latency-bound: 64 waves, one per workgroup" if N <= 4096 else "1,024 waves"}


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
    gae = [gae_row(N, 200, a.reps, "cuda:0") for N in (4096, 65536)]
    res = {"rows": rows, "gae": gae, "device": torch.cuda.get_device_name(0), "reps": a.reps,
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

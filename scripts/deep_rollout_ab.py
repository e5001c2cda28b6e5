#!/usr/bin/env python3
"""A/B of the resident closed loop under a policy with two hidden layers (MLPPolicy(wm=...): one wg_rollout_deep launch
per call) against what a user had before it and against the one-layer rollout of the same binary; one box, one process,
the protocol of scripts/policy_rollout_ab.py and scripts/hold_rollout_ab.py:

  b_policy_loop_graph          policy_loop(graph=True) with the torch net a user would write,
                               clamp(relu(relu(obs @ w1 + b1) @ wm + bm) @ w2 + b2, -L, L): the replay timed
  c_deep_all_buffers           rollout_policy, every per-step buffer (obs, reward, done, action)
  d_deep_no_buffers            rollout_policy, no per-step buffer
  s_deep_stochastic_all / _no  rollout_stochastic likewise (raw and eps among the buffers)
  h_shallow_h32_all / _no      rollout_policy with the one-layer H = 32 policy: the same binary's existing instance

Rows: Balance-v0 x 4,096 and canonical x 65,536, a shared (32, 32) and a shared (64, 64) policy, 200 steps per call.
(b) does the same work as (c) / (d) but not bit for bit (matmul against the contract's unfused chains).  Every call
starts from the same state, put back (and observed) before the clock starts.  After a warm-up call of every path the paths
are timed in turn, `--reps` times (interleaved), each timing a whole call between two synchronisations.  Per row and path:
median, min and max ms per step, and max / min.  No bar: rows that lose are reported as they are.

    python scripts/deep_rollout_ab.py [--steps 200] [--reps 5] [--out profiles/r16_deep_rollout_ab.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from walker_gym_amd.batched_env import BatchedPhysicsEnv   # noqa: E402
from walker_gym_amd.policy import MLPPolicy                # noqa: E402
from walker_gym_amd.synthetic import canonical_walkers     # noqa: E402
from walker_gym_amd.walker import balance_spec             # noqa: E402

STATE = ("pos", "vel", "acc", "muscle_x", "steps")
SIGMA = 0.1


def timed(fn, env, snap):
    for k in STATE:   # the same start for every call, outside the clock
        getattr(env.batch, k).copy_(snap[k])
    env.observe()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def weights(D, H1, H2, C, dev, seed):
    """A shared policy's tensors; H2 = 0: one hidden layer."""
    g = torch.Generator().manual_seed(seed)
    s = 0.008
    rn = lambda *shape: torch.randn(shape, generator=g)
    w = dict(w1=(rn(1, D, H1) * s).to(dev), b1=(rn(1, H1) * s).to(dev), wm=None, bm=None)
    if H2:
        w.update(wm=(rn(1, H1, H2) * (2.0 / H1 ** 0.5)).to(dev), bm=(rn(1, H2) * s).to(dev))
    w.update(w2=(rn(1, H2 or H1, C) * 4 * s).to(dev), b2=(rn(1, C) * s).to(dev))
    return w


def row(name, spec, params, H, steps, reps):
    envs = {k: BatchedPhysicsEnv(spec, **params) for k in "bcdsh"}
    e0 = envs["c"]
    dev, N, D, A = e0.device, e0.N, e0.obs_dim, e0.batch.A
    w = weights(D, H, H, A, dev, seed=H + 1)
    deep = MLPPolicy(w["w2"], w["b2"], w["w1"], w["b1"], act_limit=1.0, wm=w["wm"], bm=w["bm"])
    v = weights(D, 32, 0, A, dev, seed=33)
    shallow = MLPPolicy(v["w2"], v["b2"], v["w1"], v["b1"], act_limit=1.0)
    sigma = torch.full((1, A), SIGMA, device=dev)

    def user_policy(rows, t):   # what a user of policy_loop writes
        h = torch.relu(rows @ w["w1"][0] + w["b1"][0])
        h = torch.relu(h @ w["wm"][0] + w["bm"][0])
        return torch.clamp(h @ w["w2"][0] + w["b2"][0], -1.0, 1.0)

    f = lambda *s: torch.empty(s, device=dev)
    buf = dict(obs_out=f(steps, N, D), reward_out=f(steps, N), done_out=torch.empty((steps, N), dtype=torch.uint8, device=dev),
               action_out=f(steps, N, A))
    nzbuf = dict(buf, raw_action_out=f(steps, N, A), eps_out=f(steps, N, A))
    snap = {k: {s: getattr(e.batch, s).clone() for s in STATE} for k, e in envs.items()}
    envs["b"].observe()
    envs["b"].policy_loop(user_policy, 1)   # (the BLAS library initialises at its first matmul of a shape: before the capture)
    torch.cuda.synchronize()
    graph = envs["b"].policy_loop(user_policy, steps, graph=True)   # capture (and one replay) outside the timing
    runs = {"b_policy_loop_graph": graph.replay,
            "c_deep_all_buffers": lambda: envs["c"].rollout_policy(deep, steps, **buf),
            "d_deep_no_buffers": lambda: envs["d"].rollout_policy(deep, steps),
            "s_deep_stochastic_all_buffers": lambda: envs["s"].rollout_stochastic(deep, steps, sigma, 1, **nzbuf),
            "s_deep_stochastic_no_buffers": lambda: envs["s"].rollout_stochastic(deep, steps, sigma, 1),
            "h_shallow_h32_all_buffers": lambda: envs["h"].rollout_policy(shallow, steps, **buf),
            "h_shallow_h32_no_buffers": lambda: envs["h"].rollout_policy(shallow, steps)}
    for k, fn in runs.items():   # warm-up: one whole call each (a run's env is named by the first letter of its key)
        timed(fn, envs[k[0]], snap[k[0]])
    ms = {k: [] for k in runs}
    for _ in range(reps):
        for k, fn in runs.items():
            ms[k].append(1e3 * timed(fn, envs[k[0]], snap[k[0]]) / steps)
    stat = {k: {"median": statistics.median(t), "min": min(t), "max": max(t), "spread": max(t) / min(t)}
            for k, t in ms.items()}
    res = {"row": name, "N": N, "D": D, "H1": H, "H2": H, "C": A, "steps_per_call": steps, "sigma": SIGMA,
           "ms_per_step": stat, "launch_geometry": e0.launch_geometry()}
    for k in ("c_deep_all_buffers", "d_deep_no_buffers"):
        res[k + "_over_b"] = stat[k]["median"] / stat["b_policy_loop_graph"]["median"]
        res[k + "_below_b_beyond_spread"] = max(ms[k]) < min(ms["b_policy_loop_graph"])
    res["c_deep_over_shallow_h32"] = stat["c_deep_all_buffers"]["median"] / stat["h_shallow_h32_all_buffers"]["median"]
    res["d_deep_over_shallow_h32"] = stat["d_deep_no_buffers"]["median"] / stat["h_shallow_h32_no_buffers"]["median"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    bal, can = balance_spec(4096), canonical_walkers(65536, seed=0)
    rows = []
    for H in (32, 64):
        rows.append(row(f"balance4096-H{H}x{H}", bal, dict(in3d=0), H, a.steps, a.reps))
        rows.append(row(f"canonical65536-H{H}x{H}", can, dict(in3d=1), H, a.steps, a.reps))
    res = {"rows": rows, "device": torch.cuda.get_device_name(0), "reps": a.reps,
           "method": "one process, warm-up call of every path, then the paths timed in turn reps times; ms per step = "
                     "wall time of a whole call between two synchronisations / steps; every call from the same state"}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""A/B of the closed-loop resident rollout (BatchedPhysicsEnv.rollout_policy, one wg_rollout_policy launch per episode)
against the closed loops the package had before it, one box, one process:

  (a) policy_loop, eager            the policy written as a user would: clamp(relu(obs @ w1 + b1) @ w2 + b2, -L, L)
  (b) policy_loop(graph=True)       the same loop as captured HIP graphs, the replay timed (capture excluded)
  (c) rollout_policy, every per-step buffer (obs, reward, done, action)
  (d) rollout_policy, no per-step buffer (returns and lengths only)
  (e) rollout(resident=True), open loop with precomputed actions: the floor
  (c0) / (d0): (c) / (d) with WG_POLICY_STAGE=0 (the shared weights always read through L2)
  (c2) / (d2): (c) / (d) with WG_POLICY_STAGE=2 (the shared weights staged in LDS even where that costs occupancy)

Workloads: Balance-v0 x 4,096 and canonical x 65,536, 200 steps per call; policies H = 0 and H = 32, one shared
parameter set; plus one G = N row (canonical, H = 0) for information.  (a) and (b) do the same work as (c) and (d) but
not bit for bit (matmul against the contract's unfused chains).  Every call starts from the same state: the batch is put
back to its initial state (and observed) before the clock starts, because a closed loop drives some walkers to large or
non-finite values over hundreds of steps and the step's exact cold paths then cost time, so paths timed on states of
different ages do not compare.  After a warm-up call of every path the paths are timed in turn, `--reps` times
(interleaved, so clock and thermal drift fall on all alike), each timing a whole call between two synchronisations.  Per row and path: median, min and max ms per step; and whether (c) and (d) are below (b) by more
than the measured spread (max of the fused path < min of (b)).

    python scripts/policy_rollout_ab.py [--steps 200] [--reps 5] [--out profiles/r08_policy_rollout_ab.json]
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


def timed(fn, env=None, snap=None):
    if env is not None:   # the same start for every call, outside the clock
        for k in STATE:
            getattr(env.batch, k).copy_(snap[k])
        env.observe()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def weights(D, H, C, G, dev, seed):
    g = torch.Generator().manual_seed(seed)
    s = 0.008 if H else 0.001
    rn = lambda *shape: torch.randn(shape, generator=g)
    w1 = (rn(G, D, H) * s).to(dev) if H else None
    b1 = (rn(G, H) * s).to(dev) if H else None
    w2 = (rn(G, H if H else D, C) * (4 * s if H else s)).to(dev)
    b2 = (rn(G, C) * s).to(dev)
    return w2, b2, w1, b1


def row(name, spec, params, H, G, steps, reps, only_fused=False):
    envs = {k: BatchedPhysicsEnv(spec, **params) for k in (("c", "d") if only_fused else ("a", "b", "c", "d", "e"))}
    e0 = envs["c"]
    dev, N, D, A = e0.device, e0.N, e0.obs_dim, e0.batch.A
    w2, b2, w1, b1 = weights(D, H, A, G, dev, seed=H + 1)
    pol = MLPPolicy(w2, b2, w1, b1, act_limit=1.0)

    def user_policy(rows, t):   # (G = 1) what a user of policy_loop writes
        x = torch.relu(rows @ w1[0] + b1[0]) if H else rows
        return torch.clamp(x @ w2[0] + b2[0], -1.0, 1.0)

    buf = dict(obs_out=torch.empty((steps, N, D), device=dev), reward_out=torch.empty((steps, N), device=dev),
               done_out=torch.empty((steps, N), dtype=torch.uint8, device=dev),
               action_out=torch.empty((steps, N, A), device=dev))

    def staged(mode, fn):
        def run():
            os.environ["WG_POLICY_STAGE"] = str(mode)
            try:
                fn()
            finally:
                os.environ.pop("WG_POLICY_STAGE", None)
        return run

    fused_c = lambda: envs["c"].rollout_policy(pol, steps, **buf)
    fused_d = lambda: envs["d"].rollout_policy(pol, steps)
    snap = {k: {s: getattr(e.batch, s).clone() for s in STATE} for k, e in envs.items()}
    runs = {"c_fused_all_buffers": staged(1, fused_c), "d_fused_no_buffers": staged(1, fused_d)}
    if G == 1:
        runs.update({"c0_fused_all_buffers_l2_weights": staged(0, fused_c),
                     "d0_fused_no_buffers_l2_weights": staged(0, fused_d),
                     "c2_fused_all_buffers_lds_weights": staged(2, fused_c),
                     "d2_fused_no_buffers_lds_weights": staged(2, fused_d)})
    if not only_fused:
        for k in ("a", "b", "e"):
            envs[k].observe()
        acts = (torch.rand((steps, N, A), device=dev) * 2 - 1).contiguous()
        # (the BLAS library initialises at its first matmul of a shape, which a capture forbids: one eager step of
        # the same loop first, which runs the policy on every walker-range shape)
        envs["b"].policy_loop(user_policy, 1)
        torch.cuda.synchronize()
        graph = envs["b"].policy_loop(user_policy, steps, graph=True)   # capture (and one replay) outside the timing
        runs.update({"a_policy_loop_eager": lambda: envs["a"].policy_loop(user_policy, steps),
                     "b_policy_loop_graph": graph.replay,
                     "e_open_loop_resident": lambda: envs["e"].rollout(acts, buf["obs_out"], buf["reward_out"],
                                                                       buf["done_out"], resident=True)})
    for k, fn in runs.items():   # warm-up: one whole call each
        timed(fn, envs[k[0]], snap[k[0]])
    ms = {k: [] for k in runs}
    for _ in range(reps):
        for k, fn in runs.items():   # (a run's env is named by the first letter of its key)
            ms[k].append(1e3 * timed(fn, envs[k[0]], snap[k[0]]) / steps)
    stat = {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "spread": max(v) / min(v)}
            for k, v in ms.items()}
    res = {"row": name, "N": N, "D": D, "H": H, "C": A, "G": G, "steps_per_call": steps, "ms_per_step": stat,
           "launch_geometry": e0.launch_geometry(),
           "nonfinite_walkers_after_one_call": {k: int((~torch.isfinite(e.batch.pos.view(N, -1)).all(1)).sum())
                                       for k, e in envs.items()}}
    if not only_fused:
        b = ms["b_policy_loop_graph"]
        for k in ("c_fused_all_buffers", "d_fused_no_buffers"):
            res[k + "_below_b_beyond_spread"] = max(ms[k]) < min(b)
            res[k + "_over_b"] = stat[k]["median"] / stat["b_policy_loop_graph"]["median"]
    if G > 1:
        wbytes = 4 * G * ((D * H + H * A) if H else D * A)
        res["note"] = (f"information only: every walker reads its own {wbytes // G} B of weights per step, "
                       f"{wbytes / 1e6:.0f} MB per step for the batch, beside the step's own traffic of about "
                       f"{(N * (e0.batch.M * 24 + e0.batch.K * 12)) / 1e6:.0f} MB of state and spring records per "
                       "launch of the one-step kernel: the weight traffic rivals the step's")
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
        rows.append(row(f"balance4096-H{H}", bal, dict(in3d=0), H, 1, a.steps, a.reps))
        rows.append(row(f"canonical65536-H{H}", can, dict(in3d=1), H, 1, a.steps, a.reps))
    rows.append(row("canonical65536-H0-per-walker-sets", can, dict(in3d=1), 0, 65536, a.steps, a.reps, only_fused=True))
    res = {"rows": rows, "device": torch.cuda.get_device_name(0), "reps": a.reps,
           "method": "one process, warm-up call of every path, then the paths timed in turn reps times; ms per step = "
                     "wall time of a whole call between two synchronisations / steps"}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""A short clipped-surrogate (PPO) loop on Balance-v0 over pg.collect: a torch autograd actor of the MLPPolicy shape whose
weights are copied into the MLPPolicy that the rollout kernel evaluates, a torch critic, and a Gaussian log-density on
the recorded variates aeps (the library reports aeps and the raw action u = y + sigma * aeps; the density on them is
this script's choice: the variate is Irwin-Hall(8), unit variance, bounded).  Per iteration one stochastic rollout of
`--steps` steps of every walker (one launch), the GAE kernel, `--epochs` passes of minibatch updates.  Nothing is tuned
and nothing is asserted: the curve is recorded as it comes.

    python scripts/ppo_train.py [--walkers 1024] [--hidden 32] [--iterations 20] [--steps 64] [--epochs 4]
                                [--sigma 0.3] [--lr 3e-4] [--seed 0] [--out profiles/r11_ppo_balance_curve.json]
"""
import argparse
import json
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from walker_gym_amd import pg                              # noqa: E402
from walker_gym_amd.batched_env import BatchedPhysicsEnv   # noqa: E402
from walker_gym_amd.policy import MLPPolicy                # noqa: E402
from walker_gym_amd.walker import balance_spec             # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=int, default=1024)
    ap.add_argument("--hidden", type=int, default=32)
    ap.add_argument("--iterations", type=int, default=20)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--epochs", type=int, default=4)
    ap.add_argument("--minibatches", type=int, default=4)
    ap.add_argument("--sigma", type=float, default=0.3)
    ap.add_argument("--lr", type=float, default=3e-4)
    ap.add_argument("--clip", type=float, default=0.2)
    ap.add_argument("--gamma", type=float, default=0.99)
    ap.add_argument("--lam", type=float, default=0.95)
    ap.add_argument("--max-steps", type=int, default=200)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.manual_seed(a.seed)
    env = BatchedPhysicsEnv(balance_spec(a.walkers), in3d=0, max_steps=a.max_steps, rand_sigma=0.01, seed=a.seed)
    env.enable_auto_reset(on=("done", "nonfinite"), noise_rows=8, final_obs=True)   # a diverged walker starts over
    dev, N, D, A, H = env.device, env.N, env.obs_dim, env.batch.A, a.hidden
    # the actor: MLPPolicy's shape (y = relu(x @ w1 + b1) @ w2 + b2), its parameters the autograd leaves
    p = lambda *s, k=1.0: torch.nn.Parameter(torch.randn(s, device=dev) * k)
    w1, b1 = p(D, H, k=0.002), torch.nn.Parameter(torch.zeros(H, device=dev))
    w2, b2 = p(H, A, k=0.01), torch.nn.Parameter(torch.zeros(A, device=dev))
    log_sigma = torch.nn.Parameter(torch.full((A,), math.log(a.sigma), device=dev))
    critic = torch.nn.Sequential(torch.nn.Linear(D, 64), torch.nn.Tanh(), torch.nn.Linear(64, 1)).to(dev)
    opt = torch.optim.Adam([w1, b1, w2, b2, log_sigma, *critic.parameters()], lr=a.lr)
    obs_scale = 1e-2   # the rows hold accelerations in the thousands: the critic sees them scaled
    value_fn = lambda rows: critic((rows * obs_scale).clamp(-10.0, 10.0)).squeeze(-1)
    mean_of = lambda rows: torch.relu(rows @ w1 + b1) @ w2 + b2

    def log_prob(rows, u):   # Gaussian density of u around the actor's mean: eps = (u - y) / sigma
        sg = log_sigma.exp()
        z = (u - mean_of(rows)) / sg
        return (-0.5 * z * z - log_sigma - 0.5 * math.log(2 * math.pi)).sum(-1)

    curve, t0 = [], time.perf_counter()
    for it in range(a.iterations):
        with torch.no_grad():   # this iteration's weights into the policy the kernel evaluates
            pol = MLPPolicy(w2.detach().clone(), b2.detach().clone(), w1.detach().clone(), b1.detach().clone())
            sigma = log_sigma.exp().detach().reshape(1, A).contiguous()
        batch = pg.collect(env, pol, sigma, a.steps, a.seed, it * a.steps, value_fn, a.gamma, a.lam)
        rows = batch["obs_before"].reshape(-1, D)
        u = batch["raw_action"].reshape(-1, A)
        adv, ret = batch["adv"].reshape(-1), batch["ret"].reshape(-1)
        ok = torch.isfinite(adv) & torch.isfinite(ret) & torch.isfinite(rows).all(1) & torch.isfinite(u).all(1)
        adv_n = (adv - adv[ok].mean()) / (adv[ok].std() + 1e-8)
        with torch.no_grad():
            eps = batch["eps"].reshape(-1, A)   # the recorded variate is the old policy's z, exactly
            old_lp = (-0.5 * eps * eps - log_sigma - 0.5 * math.log(2 * math.pi)).sum(-1)
        idx_all = torch.nonzero(ok).squeeze(1)
        for _ in range(a.epochs):
            perm = idx_all[torch.randperm(idx_all.numel(), device=dev)]
            for mb in perm.chunk(a.minibatches):
                ratio = (log_prob(rows[mb], u[mb]) - old_lp[mb]).exp()
                surr = torch.minimum(ratio * adv_n[mb], ratio.clamp(1 - a.clip, 1 + a.clip) * adv_n[mb])
                v_loss = (value_fn(rows[mb]) - ret[mb]).pow(2).mean()
                loss = -surr.mean() + 0.5 * v_loss
                opt.zero_grad(set_to_none=True)
                loss.backward()
                torch.nn.utils.clip_grad_norm_([w1, b1, w2, b2, log_sigma, *critic.parameters()], 0.5)
                opt.step()
        n_ep = batch["episodes"].sum().clamp(min=1)
        curve.append({"iteration": it, "reward_per_step": float(batch["reward"].double().nanmean()),
                      "episodes": int(batch["episodes"].sum()),
                      "mean_episode_return": float(batch["return_sum"].double().nansum() / n_ep),
                      "mean_episode_length": float(batch["length_sum"].double().sum() / n_ep),
                      "value_loss": float(v_loss.detach()), "sigma": [float(s) for s in log_sigma.exp()],
                      "clipped_action_fraction": float((batch["raw_action"].abs() > 1).float().mean()),
                      "samples_dropped_nonfinite": int((~ok).sum())})
        print(json.dumps(curve[-1]), flush=True)
    torch.cuda.synchronize()
    res = {"env": "Balance-v0", "walkers": N, "hidden": H, "steps": a.steps, "iterations": a.iterations,
           "epochs": a.epochs, "minibatches": a.minibatches, "lr": a.lr, "clip": a.clip, "gamma": a.gamma,
           "lam": a.lam, "max_steps": a.max_steps, "seed": a.seed, "seconds": time.perf_counter() - t0,
           "device": torch.cuda.get_device_name(0), "curve": curve}
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()

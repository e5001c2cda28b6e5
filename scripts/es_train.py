#!/usr/bin/env python3
"""Train Balance-v0 with walker_gym_amd.es.EvolutionStrategy for some generations and record the fitness curve: per
generation the candidates' mean / max / min fitness (the mean return of a candidate's walkers over `--steps` steps from
the same start state) and the return of the mean policy (theta itself, one shared parameter set).  Nothing is asserted:
the curve is recorded as it comes.

    python scripts/es_train.py [--walkers 1024] [--population 1024] [--hidden 0] [--generations 30] [--steps 200]
                               [--sigma 0.001] [--lr 1e-4] [--seed 0] [--out profiles/r10_es_balance_curve.json]

--adaptive trains with AdaptiveEvolutionStrategy instead (one sigma per parameter, every entry starting at --sigma,
adapted with the class defaults) and records sigma_vec's mean / min / max per generation as well.  Its step along the
mean's estimate is sigma^2 times the scalar trainer's, so --lr is divided by --sigma^2 there: both trainers start with
the same step.
    python scripts/es_train.py --adaptive --out profiles/r13_es_adaptive_balance_curve.json

--obs-norm puts a running observation normaliser (walker_gym_amd.normalize.ObsNorm, clip 10) in front of the policy:
every generation's rollout records its rows, and the rows of every 64th walker update the statistics (the next
generation's candidates and mean policy run under them; tell() does not read them, so the update's place relative to it
changes nothing).  The rows are then of order one, so --sigma and --lr default to the trainer's own defaults (0.05,
0.05) instead of the raw rows' 0.001 and 1e-4.
    python scripts/es_train.py --adaptive --obs-norm --out profiles/r14_es_obs_norm_balance_curve.json

--act-every K: the candidates and the mean policy decide every K steps and hold their action between
(generation_step(act_every=K): the deterministic rollout_held).
    python scripts/es_train.py --act-every 4 --out profiles/r15_es_act_every4_balance_curve.json

--hidden2 H2: a deep policy, --hidden -> H2 units (the trainers' hidden2=: theta's six segments, the wg_es_*_deep
entries); --hidden defaults to H2 then.
    python scripts/es_train.py --hidden2 32 --out profiles/r17_es_deep_balance_curve.json

--adam: theta is stepped by the device optimiser (EvolutionStrategy(optimizer="adam"): wg_adam_step along the same
estimate, lr = --lr, the class's betas, no clip) instead of theta += lr * grad.  Adam's step is of the order of lr per
parameter whatever the estimate's scale, so --lr means another thing there; nothing is tuned.  Not with --adaptive.
    python scripts/es_train.py --adam --lr 1e-3 --out profiles/r31_es_adam_balance_curve.json
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from walker_gym_amd.batched_env import BatchedPhysicsEnv   # noqa: E402
from walker_gym_amd.es import AdaptiveEvolutionStrategy, EvolutionStrategy   # noqa: E402
from walker_gym_amd.normalize import ObsNorm               # noqa: E402
from walker_gym_amd.walker import balance_spec             # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=int, default=1024)
    ap.add_argument("--population", type=int, default=1024)
    ap.add_argument("--hidden", type=int, default=0)
    ap.add_argument("--hidden2", type=int, default=0)
    ap.add_argument("--generations", type=int, default=30)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--sigma", type=float, default=None)
    ap.add_argument("--lr", type=float, default=None)
    ap.add_argument("--obs-norm", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--adaptive", action="store_true")
    ap.add_argument("--act-every", type=int, default=1)
    ap.add_argument("--adam", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.adam and a.adaptive:
        ap.error("--adam is the scalar trainer's option (the adaptive theta step is inside wg_es_update_diag)")
    a.sigma = (0.05 if a.obs_norm else 0.001) if a.sigma is None else a.sigma
    a.lr = (0.05 if a.obs_norm else 1e-4) if a.lr is None else a.lr
    if a.hidden2 and not a.hidden:
        a.hidden = a.hidden2
    env = BatchedPhysicsEnv(balance_spec(a.walkers), in3d=0)
    nm = rows = mask = None
    if a.obs_norm:
        nm = ObsNorm(env.obs_dim, env.device, clip=10.0)
        rows = torch.empty((a.steps, env.N, env.obs_dim), dtype=torch.float32, device=env.device)
        mask = torch.zeros((a.steps, env.N), dtype=torch.uint8, device=env.device)
        mask[:, ::64] = 1
    if a.adaptive:
        tr = AdaptiveEvolutionStrategy(env, hidden=a.hidden, population=a.population, sigma=a.sigma,
                                       lr=a.lr / a.sigma ** 2, seed=a.seed, obs_norm=nm, hidden2=a.hidden2)
    else:
        tr = EvolutionStrategy(env, hidden=a.hidden, population=a.population, sigma=a.sigma, lr=a.lr, seed=a.seed,
                               obs_norm=nm, hidden2=a.hidden2, optimizer="adam" if a.adam else None)
    start = env.batch.state_dict()
    curve = []
    t0 = time.perf_counter()
    for g in range(a.generations):
        env.batch.load_state_dict(start)
        if a.act_every > 1:
            mean_ret = env.rollout_held(tr.mean_policy(), a.steps, a.act_every)["returns"].double().mean()
        else:
            mean_ret = env.rollout_policy(tr.mean_policy(), a.steps)["returns"].double().mean()
        out = tr.generation_step(a.steps, obs_out=rows, act_every=a.act_every)
        if nm is not None:
            nm.update(rows, mask)
        curve.append({"generation": g, "mean_policy_return": float(mean_ret),
                      "fitness_mean": float(out["fitness_mean"]), "fitness_max": float(out["fitness_max"]),
                      "fitness_min": float(out["fitness_min"]),
                      "diverged_candidates": int(torch.isnan(out["fitness"]).sum()),
                      "grad_norm": float(out["grad"].double().norm())})
        if a.adaptive:
            curve[-1].update(grad_sigma_norm=float(out["grad_sigma"].double().norm()),
                             sigma_mean=float(out["sigma_mean"]), sigma_min=float(out["sigma_min"]),
                             sigma_max=float(out["sigma_max"]))
        if nm is not None:
            curve[-1].update(obs_norm_rows=nm.count, obs_norm_scale_min=float(nm.scale.min()),
                             obs_norm_scale_max=float(nm.scale.max()))
        print(json.dumps(curve[-1]), flush=True)
    torch.cuda.synchronize()
    res = {"env": "Balance-v0", "walkers": env.N, "population": tr.G, "hidden": tr.H, "hidden2": tr.H2, "K": tr.K, "steps": a.steps,
           "trainer": type(tr).__name__, "obs_norm": bool(a.obs_norm), "act_every": a.act_every, "adam": bool(a.adam), "sigma": a.sigma if a.adaptive else tr.sigma, "lr": tr.lr, "seed": tr.seed, "seconds": time.perf_counter() - t0,
           "device": torch.cuda.get_device_name(0), "curve": curve}
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()

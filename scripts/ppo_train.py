#!/usr/bin/env python3
"""A short clipped-surrogate (PPO) loop on Balance-v0 over pg.collect and pg.policy_rows: the actor is the MLPPolicy the
rollout kernel evaluates, its tensors nn.Parameters that Adam updates in place (no second actor, no weight copy); its
mean on the recorded rows is pg.policy_rows, the kernel's own arithmetic, so on the first pass over fresh data the
mean is the y inside the recorded u = RN32(y + RN32(sigma * aeps)) bit for bit.  A torch critic, and a Gaussian
log-density on u around that mean (the density is this script's choice: the variate is Irwin-Hall(8), unit variance,
bounded).  Per iteration one stochastic rollout of `--steps` steps of every walker (one launch), the GAE kernel,
`--epochs` passes of minibatch updates, a minibatch being a row mask over the [T, N] batch.  Nothing is tuned and
nothing is asserted: the curve is recorded as it comes.

    python scripts/ppo_train.py [--walkers 1024] [--hidden 32] [--iterations 20] [--steps 64] [--epochs 4]
                                [--sigma 0.3] [--lr 3e-4] [--seed 0] [--out profiles/r12_ppo_balance_curve.json]

--obs-norm: a running observation normaliser (walker_gym_amd.normalize.ObsNorm, clip 10) in front of the actor, inside
the rollout kernel and inside pg.policy_rows alike, and in front of the critic (the same three torch operations) in place
of the ad-hoc obs_scale; updated once per iteration from batch["obs_before"], after the iteration's epochs, so that the
rows are re-evaluated under the statistics they were collected with and the first-pass ratio stays exactly 1.  The
actor's first layer then starts at 1 / sqrt(D) (unit-scale inputs) instead of 0.002.
    python scripts/ppo_train.py --obs-norm --out profiles/r14_ppo_obs_norm_balance_curve.json

--act-every K: the actor decides every K steps and holds its action between (pg.collect(act_every=K): rollout_held and
the GAE on the decision grid, `held` carried from one iteration's rollout to the next).  The update's rows are the
decided ones (the mask becomes ok & decided: the density, the surrogate and the critic's loss are put on those alone); a
row's return is the hold's summed reward plus the discounted value at the next decision.
    python scripts/ppo_train.py --act-every 4 --out profiles/r15_ppo_act_every4_balance_curve.json

--hidden2 H2: a second hidden layer of H2 units between the two (MLPPolicy(wm=..., bm=...): the rollout runs through
wg_rollout_deep, pg.policy_rows through wg_policy_forward_deep / wg_policy_backward_deep); the 64 x 64 or 32 x 32 actor of
the PPO baselines is --hidden 64 --hidden2 64.  The middle matrix starts at 1 / sqrt(hidden).
    python scripts/ppo_train.py --hidden 64 --hidden2 64

--fused-loss: the density, the ratio, the clip, the minimum, the masking and their backward in one kernel call
(pg.ppo_surrogate: wg_ppo_surrogate, its exponential the library's own wg_expf) instead of the torch composition below:
old_lp comes from pg.log_prob_rows, the minibatch loss from pg.ppo_surrogate on pg.policy_rows' mean and the critic's
values.  The first-pass ratio is still exactly 1 (exp(+0) = 1 in wg_expf).  Off by default: without the flag the script
runs as before.
    python scripts/ppo_train.py --fused-loss --out profiles/r30_ppo_fused_loss_balance_curve.json

--device-adam: the update's last part on the device too: walker_gym_amd.optim.Adam (wg_adam_step: the global-norm clip
at max_norm = 0.5 and the Adam step over the actor's tensors, log_sigma and the critic's torch parameters as ordinary
segments, one call) instead of clip_grad_norm_ + torch.optim.Adam, and pg.normalize_advantages (the masked mean and
1 / sqrt(var + eps) from wg_obs_moments' ordered sums; the population variance, where adv[ok].std() is the sample's)
instead of the boolean-indexed mean / std.  Off by default: without the flag the script runs as before.
    python scripts/ppo_train.py --fused-loss --device-adam --out profiles/r31_ppo_device_adam_balance_curve.json
"""
import argparse
import json
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from walker_gym_amd import optim, pg                       # noqa: E402
from walker_gym_amd.batched_env import BatchedPhysicsEnv   # noqa: E402
from walker_gym_amd.normalize import ObsNorm               # noqa: E402
from walker_gym_amd.policy import MLPPolicy                # noqa: E402
from walker_gym_amd.walker import balance_spec             # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=int, default=1024)
    ap.add_argument("--hidden", type=int, default=32)
    ap.add_argument("--hidden2", type=int, default=0)
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
    ap.add_argument("--obs-norm", action="store_true")
    ap.add_argument("--act-every", type=int, default=1)
    ap.add_argument("--fused-loss", action="store_true")
    ap.add_argument("--device-adam", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.manual_seed(a.seed)
    env = BatchedPhysicsEnv(balance_spec(a.walkers), in3d=0, max_steps=a.max_steps, rand_sigma=0.01, seed=a.seed)
    env.enable_auto_reset(on=("done", "nonfinite"), noise_rows=8, final_obs=True)   # a diverged walker starts over
    dev, N, D, A, H = env.device, env.N, env.obs_dim, env.batch.A, a.hidden
    # the actor: the MLPPolicy itself, its tensors the autograd leaves (kept by identity: Adam's in-place steps are what
    # the next rollout reads)
    p = lambda *s, k=1.0: torch.nn.Parameter(torch.randn(s, device=dev) * k)
    nm = ObsNorm(D, dev, clip=10.0) if a.obs_norm else None
    w1, b1 = p(1, D, H, k=D ** -0.5 if nm else 0.002), torch.nn.Parameter(torch.zeros(1, H, device=dev))
    H2 = a.hidden2
    wm, bm = (p(1, H, H2, k=H ** -0.5), torch.nn.Parameter(torch.zeros(1, H2, device=dev))) if H2 else (None, None)
    w2, b2 = p(1, H2 or H, A, k=0.01), torch.nn.Parameter(torch.zeros(1, A, device=dev))
    pol = MLPPolicy(w2, b2, w1, b1, obs_norm=nm, wm=wm, bm=bm)
    assert pol.w1 is w1 and pol.w2 is w2 and pol.wm is wm
    actor = [t for t in (w1, b1, wm, bm, w2, b2) if t is not None]
    log_sigma = torch.nn.Parameter(torch.full((A,), math.log(a.sigma), device=dev))
    critic = torch.nn.Sequential(torch.nn.Linear(D, 64), torch.nn.Tanh(), torch.nn.Linear(64, 1)).to(dev)
    trained = [*actor, log_sigma, *critic.parameters()]
    opt = optim.Adam(trained, lr=a.lr, max_norm=0.5) if a.device_adam else torch.optim.Adam(trained, lr=a.lr)

    def update():   # the gradients are in place: clip their global norm at 0.5, one Adam step
        if not a.device_adam:
            torch.nn.utils.clip_grad_norm_(trained, 0.5)
        opt.step()

    obs_scale = 1e-2   # the rows hold accelerations in the thousands: the critic sees them scaled
    if nm is not None:
        value_fn = lambda rows: critic(nm.normalize_torch(rows)).squeeze(-1)
    else:
        value_fn = lambda rows: critic((rows * obs_scale).clamp(-10.0, 10.0)).squeeze(-1)

    def log_prob(mean, u):   # Gaussian density of u around the policy's mean
        z = (u - mean) / log_sigma.exp()
        return (-0.5 * z * z - log_sigma - 0.5 * math.log(2 * math.pi)).sum(-1)

    curve, t0, held = [], time.perf_counter(), None
    for it in range(a.iterations):
        sigma = log_sigma.exp().detach().reshape(1, A).contiguous()
        batch = pg.collect(env, pol, sigma, a.steps, a.seed, it * a.steps, value_fn, a.gamma, a.lam,
                           act_every=a.act_every, held=held)
        held = batch.get("held")
        obs, u = batch["obs_before"], batch["raw_action"]          # [T, N, D], [T, N, A]
        adv, ret = batch["adv"], batch["ret"]
        ok = torch.isfinite(adv) & torch.isfinite(ret) & torch.isfinite(obs).all(-1) & torch.isfinite(u).all(-1)
        if a.act_every > 1:
            ok = ok & (batch["decided"] != 0)
        if a.device_adam:
            adv_n = pg.normalize_advantages(adv, ok)
        else:
            adv_n = torch.where(ok, (adv - adv[ok].mean()) / (adv[ok].std() + 1e-8), torch.zeros_like(adv))
        ret_0 = torch.where(ok, ret, torch.zeros_like(ret))
        with torch.no_grad():   # the old policy's density: the same function on the same rows, before any update
            if a.fused_loss:
                old_lp = pg.log_prob_rows(pg.policy_rows(pol, obs, ok), u, sigma.reshape(-1), log_sigma.detach(), ok)
            else:
                old_lp = log_prob(pg.policy_rows(pol, obs, ok), u)
            first_ratio_dev = None
        T = obs.shape[0]
        for _ in range(a.epochs):
            part = torch.randint(a.minibatches, (T, N), device=dev)
            for m in range(a.minibatches):
                mask = ok & (part == m)           # the minibatch: a row mask (skipped rows are neither read nor summed)
                cnt = mask.sum().clamp(min=1)
                mean = pg.policy_rows(pol, obs, mask)
                if a.fused_loss:
                    value = value_fn(torch.where(mask[..., None], obs, torch.zeros_like(obs)))
                    loss, info = pg.ppo_surrogate(mean, u, log_sigma, old_lp, adv_n, mask, a.clip, value=value, ret=ret_0)
                    if first_ratio_dev is None:   # exactly 0: exp(+0) = 1 in the library's own exponential
                        ratio = pg.expf(torch.where(mask, info["logp"] - old_lp, torch.zeros_like(old_lp)))
                        first_ratio_dev = float((ratio[mask] - 1).abs().max())
                    v_loss = info["value_loss"].to(torch.float32)
                    opt.zero_grad(set_to_none=True)
                    loss.backward()
                    update()
                    continue
                lp = torch.where(mask, log_prob(mean, torch.where(mask[..., None], u, torch.zeros_like(u))), old_lp)
                ratio = (lp - old_lp).exp()
                if first_ratio_dev is None:       # exactly 0: the trained function is the function the kernel ran
                    first_ratio_dev = float((ratio.detach()[mask] - 1).abs().max())
                surr = torch.minimum(ratio * adv_n, ratio.clamp(1 - a.clip, 1 + a.clip) * adv_n)
                v_err = torch.where(mask, value_fn(torch.where(mask[..., None], obs, torch.zeros_like(obs))) - ret_0,
                                    torch.zeros_like(ret))
                v_loss = v_err.pow(2).sum() / cnt
                loss = -(surr * mask).sum() / cnt + 0.5 * v_loss
                opt.zero_grad(set_to_none=True)
                loss.backward()
                update()
        if nm is not None:
            nm.update(obs, ok)
        n_ep = batch["episodes"].sum().clamp(min=1)
        curve.append({"iteration": it, "reward_per_step": float(batch["reward"].double().nanmean()),
                      "episodes": int(batch["episodes"].sum()),
                      "mean_episode_return": float(batch["return_sum"].double().nansum() / n_ep),
                      "mean_episode_length": float(batch["length_sum"].double().sum() / n_ep),
                      "value_loss": float(v_loss.detach()), "sigma": [float(s) for s in log_sigma.exp()],
                      "clipped_action_fraction": float((batch["raw_action"].abs() > 1).float().mean()),
                      "first_pass_max_ratio_minus_1": first_ratio_dev,
                      "samples_dropped_nonfinite": int((~ok).sum()) if a.act_every == 1 else
                      int((~ok & (batch["decided"] != 0)).sum()), "samples": int(ok.sum())})
        print(json.dumps(curve[-1]), flush=True)
    torch.cuda.synchronize()
    res = {"env": "Balance-v0", "walkers": N, "hidden": H, "hidden2": H2, "steps": a.steps, "iterations": a.iterations,
           "epochs": a.epochs, "minibatches": a.minibatches, "lr": a.lr, "clip": a.clip, "gamma": a.gamma,
           "lam": a.lam, "max_steps": a.max_steps, "seed": a.seed, "obs_norm": bool(a.obs_norm), "act_every": a.act_every,
           "fused_loss": bool(a.fused_loss), "device_adam": bool(a.device_adam),
           "seconds": time.perf_counter() - t0,
           "device": torch.cuda.get_device_name(0), "curve": curve}
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()

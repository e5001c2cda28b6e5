#!/usr/bin/env python3
"""A/B of the resident closed loop with an action hold (BatchedPhysicsEnv.rollout_held, one wg_rollout_held launch per
call) against the existing entries, and of the GAE kernel on the decision grid (wg_gae_held) against wg_gae; one box,
one process, the protocol of scripts/stochastic_rollout_ab.py:

  episodes / stochastic        rollout_episodes and rollout_stochastic, no per-step buffer: the existing entries
  open_loop                    rollout(resident=True) over an action array: the step without a policy
  held_det_k / held_nz_k       rollout_held at every = k in {1, 2, 4, 8}, deterministic and with the noise, no buffer

Rows: Balance-v0 x 4,096 and canonical x 65,536, policies H = 0 and H = 32 (one shared parameter set), max_steps = 64
with the walkers' step counters staggered by w % 64, a two-row reset-noise pool.  Every call starts from the same entry
state, snapshot and episode counts.  After a warm-up call of every path the paths are timed in turn, `--reps` times
(interleaved), each timing a whole call between two synchronisations.  Per row and path: median, min and max ms per step.

The bar (DESIGN 9b's rule), on the H = 32 rows: the held call's slowest run at every = 4 below the existing entry's
fastest, in both forms.  Beside every held figure the model t_open + (t_existing - t_open) / k.

The same four rows once more with the counters in phase (`-aligned`: every walker starts at step 0, so the walkers of a
wave decide at the same steps until their episodes end apart), without a bar: the wave skips the policy only at the
steps where none of its walkers decides, and the protocol's stagger of w % 64 leaves a canonical wave (four consecutive
walkers) no such step at every <= 4.

GAE: T = 200, N = 4,096 and 65,536: device events around 20 back-to-back pg.gae_held calls (decided at 1 / 4, term and
cut on 1 / 64 of the elements) against the bytes they move (15 B read and 8 B written per element) at 6.3 TB/s, and
pg.gae on the same arrays.

    python scripts/hold_rollout_ab.py [--steps 200] [--reps 5] [--out profiles/r15_hold_rollout_ab.json]
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
EVERY = (1, 2, 4, 8)
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


def row(name, spec, params, H, steps, reps, stagger=MAX_STEPS):
    spec = dict(spec)
    n = len(spec["mass_off"]) - 1
    spec["steps"] = (np.arange(n) % stagger).astype(np.int32)
    env = BatchedPhysicsEnv(spec, rand_sigma=0.01, seed=1, max_steps=MAX_STEPS, **params)
    env.enable_auto_reset(noise_rows=2)
    dev, N, D, A = env.device, env.N, env.obs_dim, env.batch.A
    w2, b2, w1, b1 = weights(D, H, A, dev, seed=H + 1)
    pol = MLPPolicy(w2, b2, w1, b1, act_limit=1.0)
    sigma = torch.full((1, A), SIGMA, device=dev)
    acts = (torch.rand((steps, N, A), generator=torch.Generator().manual_seed(3)) * 2 - 1).to(dev)
    snap = {s: getattr(env.batch, s).clone() for s in STATE if getattr(env.batch, s, None) is not None}
    env.observe()
    runs = {"episodes": lambda: env.rollout_episodes(pol, steps),
            "stochastic": lambda: env.rollout_stochastic(pol, steps, sigma, 1),
            "open_loop": lambda: env.run(acts, steps, info=False, resident=True)}
    for k in EVERY:
        runs[f"held_det_{k}"] = lambda k=k: env.rollout_held(pol, steps, k)
        runs[f"held_nz_{k}"] = lambda k=k: env.rollout_held(pol, steps, k, sigma=sigma, seed=1)
    for fn in runs.values():   # warm-up: one whole call each
        timed(fn, env, snap)
    ms = {k: [] for k in runs}
    for _ in range(reps):
        for k, fn in runs.items():
            ms[k].append(1e3 * timed(fn, env, snap) / steps)
    stat = {k: stats(v) for k, v in ms.items()}
    t_open = stat["open_loop"]["median"]
    model = {}
    for form, base in (("det", "episodes"), ("nz", "stochastic")):
        for k in EVERY:
            model[f"held_{form}_{k}"] = t_open + (stat[base]["median"] - t_open) / k
    return {"row": name, "N": N, "D": D, "H": H, "C": A, "steps_per_call": steps, "max_steps": MAX_STEPS, "sigma": SIGMA,
            "counters_staggered_by": stagger, "ms_per_step": stat, "model_ms_per_step": model, "launch_geometry": env.launch_geometry(),
            "bar_applies": H == 32 and stagger == MAX_STEPS,
            "held_det_4_slowest_below_episodes_fastest": max(ms["held_det_4"]) < min(ms["episodes"]),
            "held_nz_4_slowest_below_stochastic_fastest": max(ms["held_nz_4"]) < min(ms["stochastic"]),
            "held_det_1_over_episodes": stat["held_det_1"]["median"] / stat["episodes"]["median"],
            "held_nz_1_over_stochastic": stat["held_nz_1"]["median"] / stat["stochastic"]["median"],
            "held_det_4_over_episodes": stat["held_det_4"]["median"] / stat["episodes"]["median"],
            "held_nz_4_over_stochastic": stat["held_nz_4"]["median"] / stat["stochastic"]["median"]}


def gae_row(N, T, dev):
    g = torch.Generator().manual_seed(N)
    rn = lambda: torch.randn((T, N), generator=g).to(dev)
    r, v, nv = rn(), rn(), rn()
    term = (torch.rand((T, N), generator=g) < 1 / 64).to(torch.uint8).to(dev)
    cut = (term | (torch.rand((T, N), generator=g) < 1 / 64).to(torch.uint8).to(dev)).contiguous()
    dec = (torch.rand((T, N), generator=g) < 1 / 4).to(torch.uint8).to(dev)
    adv, ret = torch.empty_like(r), torch.empty_like(r)
    runs = {"gae_held": (lambda: pg.gae_held(r, v, nv, dec, term, cut, 0.99, 0.95, adv_out=adv, ret_out=ret), 23),
            "gae": (lambda: pg.gae(r, v, nv, term, cut, 0.99, 0.95, adv_out=adv, ret_out=ret), 22)}
    out = {"N": N, "T": T}
    for name, (fn, per) in runs.items():
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            fn()
        e1.record()
        torch.cuda.synchronize()
        dev_ms = e0.elapsed_time(e1) / 20
        nbytes = per * T * N
        out[name] = {"kernel_ms_back_to_back": dev_ms, "bytes_moved": nbytes,
                     "ms_at_6.3_TB_per_s": 1e3 * nbytes / HBM_BYTES_PER_S,
                     "fraction_of_6.3_TB_per_s": (nbytes / HBM_BYTES_PER_S) / (dev_ms * 1e-3)}
    return out


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
    for H in (0, 32):
        rows.append(row(f"balance4096-H{H}-aligned", bal, dict(in3d=0), H, a.steps, a.reps, stagger=1))
        rows.append(row(f"canonical65536-H{H}-aligned", can, dict(in3d=1), H, a.steps, a.reps, stagger=1))
    gae = [gae_row(N, 200, "cuda:0") for N in (4096, 65536)]
    res = {"rows": rows, "gae": gae, "device": torch.cuda.get_device_name(0), "reps": a.reps,
           "method": "one process, one env per row, warm-up call of every path, then the paths timed in turn reps times; "
                     "ms per step = wall time of a whole call between two synchronisations / steps; every call from the "
                     "same entry state, snapshot and episode counts"}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

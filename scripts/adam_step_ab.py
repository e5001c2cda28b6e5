#!/usr/bin/env python3
"""A/B of the device optimiser (walker_gym_amd.optim.Adam: wg_adam_step, the global-norm clip and the Adam step in one
call) against what scripts/ppo_train.py runs without --device-adam; one box, one process, DESIGN §9d's protocol: three
warm-up windows of every arm, then the arms timed in turn `--reps` times (interleaved).  One timed value is a window of
`--inner` consecutive steps between two synchronisations, divided by `--inner` (a single step is a few launches: a
window of one would time the synchronisation); the gradients are set once and stay.

  (a)  torch.nn.utils.clip_grad_norm_(params, 0.5) + torch.optim.Adam.step(), torch's default implementation
  (a') the same with Adam(fused=True), where this torch build takes it for these tensors
  (b)  optim.Adam(max_norm=0.5).step(): the fused one-launch path (WG_ADAM_FUSED_MAX above the list's size)
  (b3) the same in three launches (WG_ADAM_FUSED_MAX=0)

Parameter lists: scripts/ppo_train.py's defaults on Balance-v0 (the 32-unit actor, the 64-unit critic, log_sigma); the
canonical 152 x 64 x 64 x 8 actor with a 152 x 64 x 1 critic and log_sigma; one 2^20-element ES theta.  Criterion: (b)'s
slowest value at or below (a)'s fastest, and the same for (b3).  Then the two (b) arms over single tensors of 1 Ki ..
1 Mi elements: where they cross is WG_ADAM_FUSED_MAX's default.

    python scripts/adam_step_ab.py [--reps 5] [--inner 200] [--out profiles/r31_adam_step_ab.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from walker_gym_amd import optim   # noqa: E402

DEV = "cuda:0"


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "spread": max(v) / min(v)}


def window(fn, inner):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(inner):
        fn()
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0) / inner   # microseconds per step


def lists(obs_balance: int):
    mlp = lambda *dims: [s for i, o in zip(dims[:-1], dims[1:]) for s in ((i, o), (o,))]
    return {
        "ppo_train_defaults": mlp(obs_balance, 32, 2) + [(2,)] + mlp(obs_balance, 64, 1),
        "canonical_152x64x64x8": mlp(152, 64, 64, 8) + [(8,)] + mlp(152, 64, 1),
        "es_theta_2^20": [(1 << 20,)],
    }


def make(shapes, seed):
    g = torch.Generator().manual_seed(seed)
    params = [torch.randn(s, generator=g).to(DEV).requires_grad_(True) for s in shapes]
    for p in params:
        p.grad = torch.randn(p.shape, generator=g).to(DEV)
    return params


def arms_for(shapes, with_torch=True):
    arms = {}
    if with_torch:
        pa = make(shapes, 0)
        oa = torch.optim.Adam(pa, lr=3e-4)

        def a_torch():
            torch.nn.utils.clip_grad_norm_(pa, 0.5)
            oa.step()
        arms["a_torch_default"] = a_torch
        try:
            pf = make(shapes, 0)
            of = torch.optim.Adam(pf, lr=3e-4, fused=True)

            def a_fused():
                torch.nn.utils.clip_grad_norm_(pf, 0.5)
                of.step()
            a_fused()
            arms["a_torch_fused"] = a_fused
        except Exception as e:   # this build has no fused Adam for these tensors: said, not hidden
            arms["a_torch_fused_unavailable"] = repr(e)
    for key, limit in (("b_device_one_launch", str(1 << 30)), ("b3_device_three_launches", "0")):
        pb = make(shapes, 0)
        ob = optim.Adam(pb, lr=3e-4, max_norm=0.5)

        def b(ob=ob, limit=limit):
            os.environ["WG_ADAM_FUSED_MAX"] = limit
            ob.step()
        arms[key] = b
    return arms


def measure(arms, reps, inner):
    runs = {k: f for k, f in arms.items() if callable(f)}
    for _ in range(3):
        for fn in runs.values():
            window(fn, inner)
    us = {k: [] for k in runs}
    for _ in range(reps):
        for k, fn in runs.items():
            us[k].append(window(fn, inner))
    return us


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--obs-balance", type=int, default=0, help="Balance-v0's obs_dim (0: ask a BatchedPhysicsEnv)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    D = a.obs_balance
    if not D:
        from walker_gym_amd.batched_env import BatchedPhysicsEnv
        from walker_gym_amd.walker import balance_spec
        D = BatchedPhysicsEnv(balance_spec(64), in3d=0).obs_dim
    rows = []
    for name, shapes in lists(D).items():
        arms = arms_for(shapes)
        us = measure(arms, a.reps, a.inner)
        a_fast = min(min(v) for k, v in us.items() if k.startswith("a_"))
        row = {"list": name, "tensors": len(shapes), "elements": sum(torch.Size(s).numel() for s in shapes),
               "us_per_step": {k: stats(v) for k, v in us.items()},
               "unavailable": {k: v for k, v in arms.items() if not callable(v)},
               "b_slowest_at_or_below_a_fastest": max(us["b_device_one_launch"]) <= a_fast,
               "b3_slowest_at_or_below_a_fastest": max(us["b3_device_three_launches"]) <= a_fast}
        rows.append(row)
        print(json.dumps(row), flush=True)
    sweep = []
    for e in (10, 12, 13, 14, 15, 16, 17, 18, 20):
        us = measure(arms_for([(1 << e,)], with_torch=False), a.reps, a.inner)
        sweep.append({"elements": 1 << e, "us_per_step": {k: stats(v) for k, v in us.items()}})
        print(json.dumps(sweep[-1]), flush=True)
    os.environ.pop("WG_ADAM_FUSED_MAX", None)
    res = {"rows": rows, "one_launch_against_three": sweep, "device": torch.cuda.get_device_name(0), "reps": a.reps,
           "inner": a.inner, "torch": torch.__version__,
           "method": "one process, three warm-up windows of every arm, then the arms timed in turn reps times; a value = "
                     "wall time of `inner` consecutive steps between two synchronisations, over inner, in microseconds"}
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()

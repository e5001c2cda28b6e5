#!/usr/bin/env python3
"""A/B of the observation normaliser in the resident rollouts (wg_rollout_normalized: the ON instances of
walker_rollout_policy) against their twins, and of wg_obs_moments against the bytes it reads and against torch; one box,
one process, the protocol of scripts/stochastic_rollout_ab.py:

  (a) policy_loop(graph=True), auto-reset on, with the normalising MLPPolicy.__call__ (torch sub, mul, clamp, then the
      layers): one step launch plus the policy's launches per step, as captured HIP graphs, the replay timed
  (b) rollout_episodes, no per-step buffer, the plain policy            (c) the same with obs_norm
  (d) rollout_stochastic, no per-step buffer, the plain policy          (e) the same with obs_norm

Rows: Balance-v0 x 4,096 and canonical x 65,536, policies H = 0 and H = 32 (one shared parameter set), max_steps = 64
with the walkers' step counters staggered by w % 64, a two-row reset-noise pool.  The normaliser's statistics come from
one recorded rollout of 16 steps; clip = 10.  Every call starts from the same entry state, snapshot and episode counts.
After a warm-up call of every path the paths are timed in turn, `--reps` times (interleaved), each timing a whole call
between two synchronisations.  Per row and path: median, min and max ms per step; ON / twin is reported without a bar,
(c) against (a) by the rule "slowest fused call below the fastest torch call".

Moments: T = 200, N = 4,096 (D = 26) and 65,536 (D = 152): ObsNorm.update (two launches) by device events over 20
back-to-back calls, against the bytes it reads (4 * T * N * D) at 6.3 TB/s, and against the torch float64 sum and
square().sum of the same rows by the same rule.

    python scripts/norm_rollout_ab.py [--steps 200] [--reps 5] [--out profiles/r14_norm_rollout_ab.json]
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
from walker_gym_amd.normalize import ObsNorm               # noqa: E402
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
    envs = {k: BatchedPhysicsEnv(spec, rand_sigma=0.01, seed=1, max_steps=MAX_STEPS, **params) for k in "abcde"}
    for k, e in envs.items():
        e.enable_auto_reset(noise_rows=2, final_obs=(k == "a"))
    e0 = envs["b"]
    dev, N, D, A = e0.device, e0.N, e0.obs_dim, e0.batch.A
    w2, b2, w1, b1 = weights(D, H, A, dev, seed=H + 1)
    plain = MLPPolicy(w2, b2, w1, b1, act_limit=1.0)
    snap = {k: {s: getattr(e.batch, s).clone() for s in STATE if getattr(e.batch, s, None) is not None}
            for k, e in envs.items()}
    # the statistics: one recorded rollout of 16 steps under the plain policy, then the entry state again
    nm = ObsNorm(D, dev, clip=10.0)
    rec = torch.empty((16, N, D), device=dev)
    e0.rollout_episodes(plain, 16, obs_out=rec)
    nm.update(rec)
    del rec
    norm = MLPPolicy(w2, b2, w1, b1, act_limit=1.0, obs_norm=nm)
    sigma = torch.full((1, A), SIGMA, device=dev)
    for e in envs.values():
        e.observe()
    envs["a"].policy_loop(norm, 1)   # (one eager step first, as scripts/stochastic_rollout_ab.py)
    torch.cuda.synchronize()
    graph = envs["a"].policy_loop(norm, steps, graph=True)   # capture (and one replay) outside the timing
    runs = {
        "a_policy_loop_graph_normalising_call": graph.replay,
        "b_episodes_plain": lambda: envs["b"].rollout_episodes(plain, steps),
        "c_episodes_obs_norm": lambda: envs["c"].rollout_episodes(norm, steps),
        "d_stochastic_plain": lambda: envs["d"].rollout_stochastic(plain, steps, sigma, 1),
        "e_stochastic_obs_norm": lambda: envs["e"].rollout_stochastic(norm, steps, sigma, 1),
    }
    for k, fn in runs.items():   # warm-up: one whole call each
        timed(fn, envs[k[0]], snap[k[0]])
    ms = {k: [] for k in runs}
    for _ in range(reps):
        for k, fn in runs.items():   # (a run's env is named by the first letter of its key)
            ms[k].append(1e3 * timed(fn, envs[k[0]], snap[k[0]]) / steps)
    stat = {k: stats(v) for k, v in ms.items()}
    med = lambda k: stat[k]["median"]
    a = ms["a_policy_loop_graph_normalising_call"]
    return {"row": name, "N": N, "D": D, "H": H, "C": A, "steps_per_call": steps, "max_steps": MAX_STEPS,
            "obs_norm_rows": nm.count, "ms_per_step": stat, "launch_geometry": e0.launch_geometry(),
            "nonfinite_walkers_after_one_call": {k: int((~torch.isfinite(e.batch.pos.view(N, -1)).all(1)).sum())
                                                 for k, e in envs.items()},
            "c_slowest_below_a_fastest": max(ms["c_episodes_obs_norm"]) < min(a),
            "e_slowest_below_a_fastest": max(ms["e_stochastic_obs_norm"]) < min(a),
            "c_over_a": med("c_episodes_obs_norm") / med("a_policy_loop_graph_normalising_call"),
            "c_over_b": med("c_episodes_obs_norm") / med("b_episodes_plain"),
            "e_over_d": med("e_stochastic_obs_norm") / med("d_stochastic_plain")}


def moments_row(N, D, T, reps, dev):
    g = torch.Generator(device=dev).manual_seed(N)
    x = torch.randn((T, N, D), generator=g, device=dev) * 30
    nm = ObsNorm(D, dev)
    runs = {"kernel": lambda: nm.update(x),
            "torch_float64": lambda: (x.double().sum((0, 1)), x.double().square().sum((0, 1)))}

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
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(20):
        runs["kernel"]()
    e1.record()
    torch.cuda.synchronize()
    dev_ms = e0.elapsed_time(e1) / 20
    nm2 = ObsNorm(D, dev)
    nm2.update(x)
    s1, s2 = runs["torch_float64"]()
    nbytes = 4 * T * N * D
    from walker_gym_amd import pg
    return {"N": N, "D": D, "T": T, "chunk_rows": pg.default_chunk_rows(T, N), "ms_per_call": {k: stats(v) for k, v in ms.items()},
            "kernel_slowest_below_torch_fastest": max(ms["kernel"]) < min(ms["torch_float64"]),
            "torch_over_kernel": statistics.median(ms["torch_float64"]) / statistics.median(ms["kernel"]),
            "kernel_ms_back_to_back": dev_ms, "bytes_read": nbytes, "ms_at_6.3_TB_per_s": 1e3 * nbytes / HBM_BYTES_PER_S,
            "fraction_of_6.3_TB_per_s": (nbytes / HBM_BYTES_PER_S) / (dev_ms * 1e-3),
            "max_relative_difference_to_torch": float(max(((nm2.state[1:1 + D] - s1).abs() / s2.sqrt()).max(),
                                                          ((nm2.state[1 + D:] - s2).abs() / s2).max()))}


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
    mom = [moments_row(N, D, 200, a.reps, "cuda:0") for N, D in ((4096, 26), (65536, 152))]
    res = {"rows": rows, "obs_moments": mom, "device": torch.cuda.get_device_name(0), "reps": a.reps,
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

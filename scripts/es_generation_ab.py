#!/usr/bin/env python3
"""What one evolution-strategies generation costs (walker_gym_amd.es.EvolutionStrategy, G = N candidates), one box, one
process:

  (a) the rollout alone (rollout_policy of the candidates as last written): the floor
  (b) EvolutionStrategy.generation_step: wg_es_perturb, the rollout, the utilities, wg_es_update
  (c) the same generation as the torch composition a user writes today: a torch.randn [G/2, K] noise matrix kept for
      the update, broadcast adds into the four [G, ...] weight tensors, the rollout, a double argsort, d @ eps

Rows: Balance-v0 x 4,096 and canonical x 65,536, H = 0 and 32, and the deep 32 x 32 policy (hidden2 = 32: the six-segment
theta and the wg_es_*_deep entries; --deep-only runs these two rows alone), `--steps` steps per rollout.  Every timed call restores
the same start state inside the clock (the same copy in all three paths), runs between two device synchronisations, and
follows three warm-up calls of every path; the paths are timed in turn `--reps` times (interleaved, so clock and thermal
drift fall on all alike).  Per row and path: median, min, max ms per call and max / min.

Also per row: each new kernel's own time (events around 20 back-to-back calls) beside the larger of its two bounds
computed from the shapes, integer issue and store bandwidth, and which of them binds; and the peak device memory of (b)
and of (c) above what is allocated before the call (the policy sets, theta, the env).

    python scripts/es_generation_ab.py [--steps 200] [--reps 5] [--out profiles/r10_es_generation_ab.json]
    python scripts/es_generation_ab.py --deep-only --out profiles/r17_es_deep_generation_ab.json
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from walker_gym_amd import _lib                            # noqa: E402
from walker_gym_amd.batched_env import BatchedPhysicsEnv   # noqa: E402
from walker_gym_amd.es import EvolutionStrategy            # noqa: E402
from walker_gym_amd.synthetic import canonical_walkers     # noqa: E402
from walker_gym_amd.walker import balance_spec             # noqa: E402

# The bounds' constants.  VALU instructions executed per noise value, counted in the gfx950 ISA of es_hip.hip: a thread
# of es_perturb on its K >= 256 path whose element lies in the first segment, as nearly all do (111: the ten Philox
# rounds, the segment test and the 64-bit addresses; one value per thread), and the inner loop of es_update_partial (80:
# the rounds that depend only on k are hoisted out of it).  Each is taken at full rate, 4 cycles per wave64 instruction
# on a SIMD, the 32-bit multiplies included: at a quarter of it both kernels would run far above their bounds.  The deep
# rows use es_perturb's count for es_perturb_deep (not recounted: the first segment's path has the same steps).
VALU = {"perturb": 111, "update": 80}
SIMDS, CLOCK_HZ, HBM_BPS = 1024, 2.4e9, 6.3e12


def bounds(kernel, n_pairs, K):
    issue = n_pairs * K * VALU[kernel] * 4 / 64 / (SIMDS * CLOCK_HZ)
    store = (2 * n_pairs * K * 4 if kernel == "perturb" else (-(-n_pairs // 256)) * K * 8) / HBM_BPS
    return {"integer_issue_ms": 1e3 * issue, "store_bandwidth_ms": 1e3 * store,
            "binds": "integer issue" if issue >= store else "store bandwidth", "bound_ms": 1e3 * max(issue, store)}


def kernel_ms(fn, n=20):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def row(name, spec, params, H, steps, reps, H2=0):
    env = BatchedPhysicsEnv(spec, **params)
    N, D, A, dev = env.N, env.obs_dim, env.batch.A, env.device
    s = 0.002 if H else 0.0005
    tr = EvolutionStrategy(env, hidden=H, population=N, sigma=s, lr=1e-5, seed=1, hidden2=H2)
    G, K, n_pairs, pol = tr.G, tr.K, tr.n_pairs, tr.policy
    start = tr._state0
    theta_c = torch.zeros(K, device=dev)
    segs = [(t, t[0].numel()) for t in (pol.w1, pol.b1, pol.wm, pol.bm, pol.w2, pol.b2) if t is not None]
    c_G = 1.0 / (2 * (G - 1))

    def a_rollout():
        env.batch.load_state_dict(start)
        return env.rollout_policy(pol, steps)

    def b_generation_step():
        return tr.generation_step(steps)

    def c_torch_composition():
        env.batch.load_state_dict(start)
        eps = torch.randn((n_pairs, K), device=dev)
        o = 0
        for t, n in segs:   # broadcast adds into the four (deep: six) [G, ...] tensors
            v = t.view(n_pairs, 2, n)
            d = s * eps[:, o:o + n]
            v[:, 0] = theta_c[o:o + n] + d
            v[:, 1] = theta_c[o:o + n] - d
            o += n
        res = env.rollout_policy(pol, steps)
        fit = res["returns"]                                  # G = N: one walker per candidate
        fit = torch.where(torch.isnan(fit), torch.full_like(fit, float("-inf")), fit)
        rank = torch.argsort(torch.argsort(fit))
        util = (2 * rank - (G - 1)).float() * c_G
        grad = ((util[0::2] - util[1::2]) @ eps) / (2 * n_pairs * s)
        theta_c.add_(1e-5 * grad)
        return grad

    runs = {"a_rollout_alone": a_rollout, "b_generation_step": b_generation_step,
            "c_torch_composition": c_torch_composition}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    tr.ask()
    for _ in range(3):         # warm-up: three whole calls of every path
        for fn in runs.values():
            timed(fn)
    ms = {k: [] for k in runs}
    for _ in range(reps):
        for k, fn in runs.items():
            ms[k].append(timed(fn))
    stat = {k: {"median": statistics.median(v), "min": min(v), "max": max(v), "spread": max(v) / min(v)}
            for k, v in ms.items()}

    def peak_above(fn):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = fn()
        torch.cuda.synchronize()
        del out
        return torch.cuda.max_memory_allocated() - base

    # (b)'s own buffers live in the trainer from its construction on (the float64 workspace, grad, theta): they are not
    # in the call's peak, so they are added here; (c)'s theta likewise
    own = tr._work.numel() * 8 + tr._grad.numel() * 4 + tr.theta.numel() * 4
    mem = {"b_generation_step": peak_above(b_generation_step) + own, "b_trainer_buffers": own,
           "c_torch_composition": peak_above(c_torch_composition) + theta_c.numel() * 4}

    util = tr.utilities(torch.randn(G, device=dev)).contiguous()
    es = tr._struct()
    L, stream = _lib.load(), env._stream()
    p = lambda t: C.c_void_p(t.data_ptr())
    if H2:
        mid = _lib.WgEsMid(hidden2=H2, wm=p(pol.wm), bm=p(pol.bm))
        t_perturb = kernel_ms(lambda: L.wg_es_perturb_deep(C.byref(es), C.byref(mid), 0, n_pairs, stream))
        t_update = kernel_ms(lambda: L.wg_es_update_deep(C.byref(es), C.byref(mid), 0, n_pairs, p(util), 1.0, 0.0,
                                                         p(tr._work), p(tr._grad), None, stream))
    else:
        t_perturb = kernel_ms(lambda: L.wg_es_perturb(C.byref(es), 0, n_pairs, stream))
        t_update = kernel_ms(lambda: L.wg_es_update(C.byref(es), 0, n_pairs, p(util), 1.0, 0.0, p(tr._work), p(tr._grad),
                                                    None, stream))
    if H2:   # the per-parameter-sigma perturb of the same shape
        sg = torch.full((K,), s, device=dev)
        t_diag = kernel_ms(lambda: L.wg_es_perturb_diag_deep(C.byref(es), C.byref(mid), p(sg), 0, n_pairs, stream))
    kern = {}
    for kname, t in (("perturb", t_perturb), ("update", t_update)):
        b = bounds(kname, n_pairs, K)
        kern["wg_es_" + kname + ("_deep" if H2 else "")] = dict(b, ms=t, bound_over_measured=b["bound_ms"] / t)
    if H2:
        b = bounds("perturb", n_pairs, K)
        kern["wg_es_perturb_diag_deep"] = dict(b, ms=t_diag, bound_over_measured=b["bound_ms"] / t_diag)
    med = lambda k: stat[k]["median"]
    return {"row": name, "N": N, "G": G, "D": D, "H": H, "H2": H2, "C": A, "K": K, "steps": steps, "ms_per_call": stat,
            "kernels": kern, "peak_bytes_above_policy_sets": mem,
            "b_allocation_model_bytes": K * (-(-G // 512)) * 8 + G,
            "noise_matrix_bytes": n_pairs * K * 4, "policy_set_bytes": G * K * 4,
            "b_slowest_not_above_c_fastest": max(ms["b_generation_step"]) <= min(ms["c_torch_composition"]),
            "b_minus_a_ms": med("b_generation_step") - med("a_rollout_alone"),
            "c_minus_a_ms": med("c_torch_composition") - med("a_rollout_alone"),
            "b_over_c": med("b_generation_step") / med("c_torch_composition"),
            "launch_geometry": env.launch_geometry()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--deep-only", action="store_true")
    a = ap.parse_args()
    bal, can = balance_spec(4096), canonical_walkers(65536, seed=0)
    rows = []
    for H in (() if a.deep_only else (0, 32)):
        rows.append(row(f"balance4096-H{H}", bal, dict(in3d=0), H, a.steps, a.reps))
        rows.append(row(f"canonical65536-H{H}", can, dict(in3d=1), H, a.steps, a.reps))
    rows.append(row("balance4096-H32x32", bal, dict(in3d=0), 32, a.steps, a.reps, H2=32))
    rows.append(row("canonical65536-H32x32", can, dict(in3d=1), 32, a.steps, a.reps, H2=32))
    res = {"rows": rows, "device": torch.cuda.get_device_name(0), "reps": a.reps,
           "method": "one process, three warm-up calls of every path, then the paths timed in turn reps times; ms per call = "
                     "wall time of a whole call between two synchronisations, the restore of the start state included "
                     "in all three; kernel times from events around 20 back-to-back calls; bounds from the shapes "
                     "(every VALU instruction at full rate, 1,024 SIMDs at 2.4 GHz, 6.3 TB/s of stores)"}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

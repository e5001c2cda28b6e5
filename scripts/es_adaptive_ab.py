#!/usr/bin/env python3
"""What one adaptive evolution-strategies generation costs (walker_gym_amd.es.AdaptiveEvolutionStrategy, G = N
candidates), by scripts/es_generation_ab.py's protocol: one box, one process,

  (a) the rollout alone (rollout_policy of the candidates as last written): the floor
  (b) EvolutionStrategy.generation_step: wg_es_perturb, the rollout, the utilities, wg_es_update (one scalar sigma)
  (c) AdaptiveEvolutionStrategy.generation_step: wg_es_perturb_diag, the rollout, the utilities, wg_es_update_diag
  (d) the same PGPE generation composed in torch: a torch.randn [G/2, K] noise matrix kept for the update, broadcast
      adds into the four [G, ...] weight tensors, the rollout, a double argsort, two [G/2] @ [G/2, K] products, the
      two steps and the clamp

Rows: Balance-v0 x 4,096 and canonical x 65,536, H = 0 and 32, `--steps` steps per rollout.  Every timed call restores
the same start state inside the clock, runs between two device synchronisations, and follows three warm-up calls of
every path; the paths are timed in turn `--reps` times (interleaved).  Per row and path: median, min, max ms per call.

Also per row: the peak device memory of (c) and of (d) above what is allocated before the call, and each kernel call's
own time (events around 20 back-to-back calls): wg_es_perturb_diag and wg_es_update_diag beside wg_es_perturb and
wg_es_update in the same process, and beside the integer-issue bound computed from the shapes and the instruction
counts below.  `--alt-lib PATH` times wg_es_update_diag of a second build of the library in the same process: the A/B
of es_diag_partial's two forms (profiles/r13_es_adaptive_ab.json) was taken with the spread form in every row of the
library under test and a second build that launched the one-thread form in every row; the library has chosen between
them by the launch's size since, so without --alt-lib the rows show the form it chooses.

    python scripts/es_adaptive_ab.py [--steps 200] [--reps 5] [--alt-lib PATH] [--out profiles/r13_es_adaptive_ab.json]
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

from walker_gym_amd import _lib                                         # noqa: E402
from walker_gym_amd.batched_env import BatchedPhysicsEnv                # noqa: E402
from walker_gym_amd.es import AdaptiveEvolutionStrategy, EvolutionStrategy   # noqa: E402
from walker_gym_amd.synthetic import canonical_walkers                  # noqa: E402
from walker_gym_amd.walker import balance_spec                          # noqa: E402

# VALU instructions executed per noise value, counted in the gfx950 ISA of es_hip.hip: a thread of
# es_perturb_diag on its K >= 256 path whose element lies in the first segment; the loop body of a filling thread of
# es_diag_partial_spread (374 in its loop unrolled by four: the Philox call, the float32 and float64 operations of the two
# terms, the addresses of its two LDS stores: 93.5) plus the adding wave's loop (17 per 16 rows of 32 values on 64
# lanes: 2); the loop body of es_diag_partial_thread (89); es_update_partial's inner loop (§9d's 80).  Each taken at full
# rate, 4 cycles per wave64 instruction on a SIMD.
VALU = {"perturb_diag": 113, "update_diag": 96, "update_diag_simple": 89, "perturb": 111, "update": 80}
SIMDS, CLOCK_HZ = 1024, 2.4e9


def issue_bound_ms(kernel, n_pairs, K):
    return 1e3 * n_pairs * K * VALU[kernel] * 4 / 64 / (SIMDS * CLOCK_HZ)


def kernel_ms(fn, n=20):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        rc = fn()
    e1.record()
    torch.cuda.synchronize()
    if rc:
        raise RuntimeError(f"a timed call returned {rc}")
    return e0.elapsed_time(e1) / n


def load_alt(path):
    L = C.CDLL(path)
    L.wg_es_update_diag.argtypes = _lib.load().wg_es_update_diag.argtypes
    L.wg_es_update_diag.restype = C.c_int
    return L


def row(name, spec, params, H, steps, reps, alt):
    env = BatchedPhysicsEnv(spec, **params)
    N, D, A, dev = env.N, env.obs_dim, env.batch.A, env.device
    s = 0.002 if H else 0.0005
    tr_b = EvolutionStrategy(env, hidden=H, population=N, sigma=s, lr=1e-5, seed=1)
    # (c) shares (b)'s candidate tensors (one MLPPolicy of G sets is enough for every path) and moves neither theta
    # nor sigma far: lr and sigma_lr are small, the clamp is the default
    tr_c = AdaptiveEvolutionStrategy(env, hidden=H, population=N, sigma=s, lr=1e-5 / s ** 2, seed=1, sigma_lr=0.1)
    tr_c.policy = tr_b.policy
    G, K, n_pairs, pol = tr_b.G, tr_b.K, tr_b.n_pairs, tr_b.policy
    start = tr_b._state0
    theta_d = torch.zeros(K, device=dev)
    sigma_d = torch.full((K,), s, device=dev)
    segs = [(t, t[0].numel()) for t in (pol.w1, pol.b1, pol.w2, pol.b2) if t is not None]
    c_G = 1.0 / (2 * (G - 1))
    lr_t, lr_s = 1e-5 / s ** 2, 0.1

    def a_rollout():
        env.batch.load_state_dict(start)
        return env.rollout_policy(pol, steps)

    def b_generation_step():
        return tr_b.generation_step(steps)

    def c_adaptive_generation_step():
        return tr_c.generation_step(steps)

    def d_torch_composition():
        env.batch.load_state_dict(start)
        d = sigma_d[None, :] * torch.randn((n_pairs, K), device=dev)
        o = 0
        for t, n in segs:   # broadcast adds into the four [G, ...] tensors
            v = t.view(n_pairs, 2, n)
            v[:, 0] = theta_d[o:o + n] + d[:, o:o + n]
            v[:, 1] = theta_d[o:o + n] - d[:, o:o + n]
            o += n
        res = env.rollout_policy(pol, steps)
        fit = res["returns"]                                  # G = N: one walker per candidate
        fit = torch.where(torch.isnan(fit), torch.full_like(fit, float("-inf")), fit)
        rank = torch.argsort(torch.argsort(fit))
        util = (2 * rank - (G - 1)).float() * c_G
        g_theta = ((util[0::2] - util[1::2]) @ d) / (2 * n_pairs)
        g_sigma = (((util[0::2] + util[1::2]) * 0.5) @ (d * d - sigma_d[None, :] ** 2)) / n_pairs / sigma_d
        theta_d.add_(lr_t * g_theta)
        new = torch.minimum(torch.maximum(sigma_d + lr_s * g_sigma, sigma_d * 0.8), sigma_d * 1.2).clamp_(min=1e-8)
        sigma_d.copy_(new)
        return g_theta, g_sigma

    runs = {"a_rollout_alone": a_rollout, "b_generation_step": b_generation_step,
            "c_adaptive_generation_step": c_adaptive_generation_step, "d_torch_composition": d_torch_composition}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0)

    tr_b.ask()
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

    # (c)'s own buffers live in the trainer from its construction on: added here; (d)'s theta and sigma likewise
    own = tr_c._work.numel() * 8 + 4 * (tr_c._grad.numel() + tr_c._grad_sigma.numel() + tr_c.theta.numel() +
                                        tr_c.sigma_vec.numel())
    mem = {"c_adaptive_generation_step": peak_above(c_adaptive_generation_step) + own, "c_trainer_buffers": own,
           "d_torch_composition": peak_above(d_torch_composition) + 8 * K}

    # the kernels alone: the learning rates are zero, so that 20 calls leave theta and sigma where they are
    util = tr_b.utilities(torch.randn(G, device=dev)).contiguous()
    es_b, es_c = tr_b._struct(), tr_c._struct()
    st = _lib.WgEsDiagStep(**dict(tr_c.step_fields(), lr_theta=0.0, lr_sigma=0.0))
    L, stream = _lib.load(), env._stream()
    p = lambda t: C.c_void_p(t.data_ptr())
    diag = lambda lib: (lambda: lib.wg_es_update_diag(C.byref(es_c), p(tr_c.sigma_vec), 0, n_pairs, p(util), C.byref(st),
                                                      p(tr_c._work), p(tr_c._grad), None, p(tr_c._grad_sigma), None,
                                                      stream))
    calls = {
        "wg_es_perturb": ("perturb", lambda: L.wg_es_perturb(C.byref(es_b), 0, n_pairs, stream)),
        "wg_es_perturb_diag": ("perturb_diag", lambda: L.wg_es_perturb_diag(C.byref(es_c), p(tr_c.sigma_vec), 0, n_pairs,
                                                                           stream)),
        "wg_es_update": ("update", lambda: L.wg_es_update(C.byref(es_b), 0, n_pairs, p(util), 1.0, 0.0, p(tr_b._work),
                                                          p(tr_b._grad), None, stream)),
        "wg_es_update_diag": ("update_diag", diag(L)),
    }
    if alt is not None:
        calls["wg_es_update_diag_alt"] = ("update_diag_simple", diag(alt))
    kern = {}
    for _ in range(3):          # three passes over the calls, in turn: the slowest and the fastest of each are kept
        for cname, (kname, fn) in calls.items():
            kern.setdefault(cname, {"kernel": kname, "ms": []})["ms"].append(kernel_ms(fn))
    for cname, k in kern.items():
        b = issue_bound_ms(k["kernel"], n_pairs, K)
        k.update(median_ms=statistics.median(k["ms"]), min_ms=min(k["ms"]), max_ms=max(k["ms"]), issue_bound_ms=b,
                 bound_over_median=b / statistics.median(k["ms"]))
    med = lambda k: stat[k]["median"]
    return {"row": name, "N": N, "G": G, "D": D, "H": H, "C": A, "K": K, "steps": steps, "ms_per_call": stat,
            "kernels": kern, "peak_bytes_above_policy_sets": mem,
            "noise_matrix_bytes": n_pairs * K * 4, "policy_set_bytes": G * K * 4,
            "c_slowest_not_above_d_fastest": max(ms["c_adaptive_generation_step"]) <= min(ms["d_torch_composition"]),
            "update_diag_slowest_not_above_update_fastest": kern["wg_es_update_diag"]["max_ms"]
            <= kern["wg_es_update"]["min_ms"],
            "c_minus_a_ms": med("c_adaptive_generation_step") - med("a_rollout_alone"),
            "b_minus_a_ms": med("b_generation_step") - med("a_rollout_alone"),
            "d_minus_a_ms": med("d_torch_composition") - med("a_rollout_alone"),
            "launch_geometry": env.launch_geometry()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--alt-lib", default=None, help="a second build of libwalker_hip.so whose wg_es_update_diag is timed too")
    ap.add_argument("--alt-name", default="a build that launches es_diag_partial_thread (one thread per (chunk, k)) always")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    alt = load_alt(a.alt_lib) if a.alt_lib else None
    bal, can = balance_spec(4096), canonical_walkers(65536, seed=0)
    rows = []
    for H in (0, 32):
        rows.append(row(f"balance4096-H{H}", bal, dict(in3d=0), H, a.steps, a.reps, alt))
        rows.append(row(f"canonical65536-H{H}", can, dict(in3d=1), H, a.steps, a.reps, alt))
        print(json.dumps({"done": [r["row"] for r in rows]}), file=sys.stderr, flush=True)
    res = {"rows": rows, "device": torch.cuda.get_device_name(0), "reps": a.reps, "valu_per_noise_value": VALU,
           "alt_lib": a.alt_name if alt is not None else None,
           "method": "one process, three warm-up calls of every path, then the paths timed in turn reps times; ms per call = "
                     "wall time of a whole call between two synchronisations, the restore of the start state included "
                     "in all four; kernel times from events around 20 back-to-back calls, three passes over the calls "
                     "in turn; bounds from the shapes (every VALU instruction at full rate, 1,024 SIMDs at 2.4 GHz)"}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

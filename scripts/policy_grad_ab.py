#!/usr/bin/env python3
"""A/B of the differentiable policy rows (pg.policy_rows: wg_policy_forward / wg_policy_backward) against what a user had
before them; one box, one process, the protocol of scripts/stochastic_rollout_ab.py:

  (a) MLPPolicy._forward_torch on the rows: the only bit-identical evaluator before this one, D multiply/add launch
      pairs per layer, no backward
  (b) pg.policy_rows, forward only (one launch)
  (c) pg.policy_rows forward, (y * dy).sum().backward(): the forward launch, the two backward launches, torch's own
      multiply / sum / expand around them
  (d) torch autograd of relu(x @ w1 + b1) @ w2 + b2 through the BLAS library, the same loss, forward plus backward: not
      bit-identical to the rollout kernel, one parameter set only

Rows: Balance-v0 x 4,096 x T = 200 and canonical x 65,536 x T = 64 (the observation widths and action counts of those
envs; the values are standard normal, the kernels touch no env), H = 0 and 32, one shared parameter set.  After a
warm-up call of every path the paths are timed in turn, `--reps` times (interleaved), each timing a whole call between
two synchronisations.  Per row and path: median, min and max ms per call.  Each kernel alone, by device events over 10
back-to-back calls, against the bytes it must move (x and y, or x and dy: 4 * (D + C) per row) at 6.3 TB/s.

    python scripts/policy_grad_ab.py [--reps 5] [--out profiles/r12_policy_grad_ab.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from walker_gym_amd import pg                              # noqa: E402
from walker_gym_amd.batched_env import BatchedPhysicsEnv   # noqa: E402
from walker_gym_amd.policy import MLPPolicy                # noqa: E402
from walker_gym_amd.synthetic import canonical_walkers     # noqa: E402
from walker_gym_amd.walker import balance_spec             # noqa: E402

HBM_BYTES_PER_S = 6.3e12


def stats(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "spread": max(v) / min(v)}


def once(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def back_to_back(fn, n=10):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize()
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def row(name, T, N, D, C, H, reps, dev):
    g = torch.Generator().manual_seed(H + 1)
    rn = lambda *s, k=1.0: (torch.randn(s, generator=g) * k).to(dev)
    s = 0.008 if H else 0.001
    w1, b1 = (rn(1, D, H, k=s), rn(1, H, k=s)) if H else (None, None)
    w2, b2 = rn(1, H or D, C, k=4 * s if H else s), rn(1, C, k=s)
    x = torch.randn((T, N, D), device=dev)
    dy = torch.randn((T, N, C), device=dev)
    pol = MLPPolicy(w2, b2, w1, b1, act_limit=float("inf"))
    leaf = lambda t: None if t is None else torch.nn.Parameter(t.clone())
    gpol = MLPPolicy(leaf(w2), leaf(b2), leaf(w1), leaf(b1), act_limit=float("inf"))
    bw1, bb1, bw2, bb2 = (None if t is None else torch.nn.Parameter(t[0].clone()) for t in (w1, b1, w2, b2))
    params = [p for p in (gpol.w1, gpol.b1, gpol.w2, gpol.b2, bw1, bb1, bw2, bb2) if p is not None]
    x2 = x.reshape(T * N, D)

    def clear():
        for p in params:
            p.grad = None

    def c_rows():
        clear()
        (pg.policy_rows(gpol, x) * dy).sum().backward()

    def d_blas():
        clear()
        h = torch.relu(x2 @ bw1 + bb1) if H else x2
        ((h @ bw2 + bb2).reshape(T, N, C) * dy).sum().backward()

    runs = {"a_forward_torch_elementwise": lambda: pol._forward_torch(x2, None),
            "b_policy_rows_forward": lambda: pg.policy_rows(pol, x),
            "c_policy_rows_forward_backward": c_rows,
            "d_blas_autograd_forward_backward": d_blas}
    for fn in runs.values():
        once(fn)
    ms = {k: [] for k in runs}
    for _ in range(reps):
        for k, fn in runs.items():
            ms[k].append(once(fn))
    stat = {k: stats(v) for k, v in ms.items()}
    # the kernels alone
    chunk = pg.default_chunk_rows(T, N)
    y = torch.empty((T, N, C), device=dev)
    fwd_ms = back_to_back(lambda: pg.policy_rows_forward(pol, x, y_out=y))
    bwd_ms = back_to_back(lambda: pg.policy_rows_backward(pol, x, dy, None, chunk))
    nbytes = 4 * (D + C) * T * N
    ideal = 1e3 * nbytes / HBM_BYTES_PER_S
    # what the paths compute: (a) and (b) agree in bits; (c) and (d) to rounding
    ya, yb = pol._forward_torch(x2, None).reshape(T, N, C), pg.policy_rows(pol, x)
    c_rows()
    cw2, cw1 = gpol.w2.grad[0].clone(), (gpol.w1.grad[0].clone() if H else None)
    d_blas()
    rel = lambda p, q: float((p - q).abs().max() / q.abs().max().clamp(min=1e-30))
    return {"row": name, "T": T, "N": N, "D": D, "H": H, "C": C, "rows": T * N, "chunk_rows": chunk,
            "ms_per_call": stat,
            "b_slowest_below_a_fastest": max(ms["b_policy_rows_forward"]) < min(ms["a_forward_torch_elementwise"]),
            "a_over_b": stat["a_forward_torch_elementwise"]["median"] / stat["b_policy_rows_forward"]["median"],
            "c_over_d": stat["c_policy_rows_forward_backward"]["median"] / stat["d_blas_autograd_forward_backward"]["median"],
            "forward_kernel_ms_back_to_back": fwd_ms, "backward_kernels_ms_back_to_back": bwd_ms,
            "bytes_moved_by_each": nbytes, "ms_at_6.3_TB_per_s": ideal,
            "forward_fraction_of_6.3_TB_per_s": ideal / fwd_ms, "backward_fraction_of_6.3_TB_per_s": ideal / bwd_ms,
            "a_equals_b_in_bits": bool(torch.equal(ya.view(torch.int32), yb.view(torch.int32))),
            "c_against_d_max_relative_difference": {"w2": rel(cw2, bw2.grad),
                                                    **({"w1": rel(cw1, bw1.grad)} if H else {})}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = "cuda:0"
    bal = BatchedPhysicsEnv(balance_spec(4096), in3d=0)
    can = BatchedPhysicsEnv(canonical_walkers(65536, seed=0), in3d=1)
    shapes = {"balance4096": (200, 4096, bal.obs_dim, bal.batch.A), "canonical65536": (64, 65536, can.obs_dim, can.batch.A)}
    del bal, can
    rows = []
    for H in (0, 32):
        for name, (T, N, D, C) in shapes.items():
            rows.append(row(f"{name}-H{H}", T, N, D, C, H, a.reps, dev))
            torch.cuda.empty_cache()
            print(json.dumps(rows[-1]), flush=True)
    res = {"rows": rows, "device": torch.cuda.get_device_name(0), "reps": a.reps,
           "method": "one process, warm-up call of every path, then the paths timed in turn reps times; ms per call = "
                     "wall time of a whole call between two synchronisations; kernels alone by device events over 10 "
                     "back-to-back calls (the backward's includes its workspace allocation)"}
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""A/B of the fused PPO surrogate (pg.ppo_surrogate: wg_ppo_surrogate) against the torch composition scripts/ppo_train.py
runs without --fused-loss; one box, one process, the protocol of scripts/stochastic_rollout_ab.py: three warm-up calls of
every side, then the sides timed in turn `--reps` times (interleaved), each timing a whole call between two
synchronisations.  One call is one minibatch's loss plus its backward down to the gradients with respect to the policy's
mean, log_sigma and the critic's values (dy / g_log_sigma / dvalue):

  (a) the Gaussian log-density, the ratio, the clamp, torch.minimum, the masking and the value error as torch
      operations over [T, N, C] and [T, N], and their autograd backward
  (b) pg.ppo_surrogate and its backward: the two launches of wg_ppo_surrogate, the default scales and the loss formed by
      a few torch operations on scalars

Rows: Balance-v0 x 1,024 x T = 64 (2 action units) and canonical x 65,536 x T = 64 (8 action units); the values are
synthetic (u = y + sigma * noise, a ratio near 1, a mask of 1 / 4 of the rows: one of four minibatches), the kernels
touch no env.  The kernel pair alone is timed by device events over 10 back-to-back direct calls (pg.ppo_surrogate_rows,
its output allocations included) against the bytes it must move at 6.3 TB/s: per unskipped row it reads y and u and
writes dy (12 * C bytes), reads old_logp, adv, value and ret and writes logp and dvalue (24 bytes); the mask is one byte
per row of the batch.  Criterion: (b)'s slowest call at or below (a)'s fastest.

    python scripts/ppo_surrogate_ab.py [--reps 5] [--out profiles/r30_ppo_surrogate_ab.json]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from walker_gym_amd import pg   # noqa: E402

HBM_BYTES_PER_S = 6.3e12
CLIP = 0.2


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


def row(name, T, N, C, reps, dev, mask_share):
    g = torch.Generator().manual_seed(C)
    rn = lambda *s, k=1.0: (torch.randn(s, generator=g) * k).to(dev)
    y = rn(T, N, C, k=0.5)
    log_sigma0 = torch.full((C,), math.log(0.3), device=dev)
    sigma = log_sigma0.exp()
    u = y + sigma * rn(T, N, C)
    adv, ret, value0 = rn(T, N), rn(T, N), rn(T, N)
    mask = (torch.rand((T, N), generator=g) < mask_share).to(dev)
    old_lp = pg.log_prob_rows(y, u, sigma, log_sigma0) + rn(T, N, k=0.1)
    mean, log_sigma, value = (t.clone().requires_grad_(True) for t in (y, log_sigma0, value0))
    leaves = (mean, log_sigma, value)

    def clear():
        for p in leaves:
            p.grad = None

    def a_torch():
        clear()
        cnt = mask.sum().clamp(min=1)
        z = (torch.where(mask[..., None], u, torch.zeros_like(u)) - mean) / log_sigma.exp()
        lp = torch.where(mask, (-0.5 * z * z - log_sigma - 0.5 * math.log(2 * math.pi)).sum(-1), old_lp)
        ratio = (lp - old_lp).exp()
        surr = torch.minimum(ratio * adv, ratio.clamp(1 - CLIP, 1 + CLIP) * adv)
        v_err = torch.where(mask, value - ret, torch.zeros_like(ret))
        loss = -(surr * mask).sum() / cnt + 0.5 * v_err.pow(2).sum() / cnt
        loss.backward()
        return loss

    def b_fused():
        clear()
        loss, _ = pg.ppo_surrogate(mean, u, log_sigma, old_lp, adv, mask, CLIP, value=value, ret=ret)
        loss.backward()
        return loss

    runs = {"a_torch_composition": a_torch, "b_ppo_surrogate": b_fused}
    for _ in range(3):
        for fn in runs.values():
            once(fn)
    ms = {k: [] for k in runs}
    for _ in range(reps):
        for k, fn in runs.items():
            ms[k].append(once(fn))
    stat = {k: stats(v) for k, v in ms.items()}
    # what the sides compute agrees to rounding
    la = float(a_torch())
    ga = [p.grad.clone() for p in leaves]
    lb = float(b_fused())
    rel = lambda p, q: float((p - q).abs().max() / q.abs().max().clamp(min=1e-30))
    diff = {"loss": abs(la - lb) / abs(la), "dy": rel(mean.grad, ga[0]), "g_log_sigma": rel(log_sigma.grad, ga[1]),
            "dvalue": rel(value.grad, ga[2])}
    # the kernel pair alone
    cnt = mask.sum().clamp(min=1).to(torch.float32)
    scale = torch.stack([-1.0 / cnt, 1.0 / cnt])
    chunk = pg.default_chunk_rows(T, N)
    kernel_ms = back_to_back(lambda: pg.ppo_surrogate_rows(y, u, sigma, log_sigma0, old_lp, adv, scale, mask, CLIP, value0,
                                                           ret, chunk))
    full = torch.ones_like(mask)
    kernel_all_ms = back_to_back(lambda: pg.ppo_surrogate_rows(y, u, sigma, log_sigma0, old_lp, adv, scale, full, CLIP,
                                                               value0, ret, chunk))
    on = int(mask.sum())
    nbytes, nbytes_all = (12 * C + 24) * on + T * N, (12 * C + 25) * T * N
    return {"row": name, "T": T, "N": N, "C": C, "rows": T * N, "rows_unskipped": on, "chunk_rows": chunk,
            "ms_per_call": stat,
            "b_slowest_at_or_below_a_fastest": max(ms["b_ppo_surrogate"]) <= min(ms["a_torch_composition"]),
            "a_over_b": stat["a_torch_composition"]["median"] / stat["b_ppo_surrogate"]["median"],
            "kernels_ms_back_to_back": kernel_ms, "bytes_moved": nbytes, "ms_at_6.3_TB_per_s": 1e3 * nbytes / HBM_BYTES_PER_S,
            "fraction_of_6.3_TB_per_s": 1e3 * nbytes / HBM_BYTES_PER_S / kernel_ms,
            "every_row": {"kernels_ms_back_to_back": kernel_all_ms, "bytes_moved": nbytes_all,
                          "ms_at_6.3_TB_per_s": 1e3 * nbytes_all / HBM_BYTES_PER_S,
                          "fraction_of_6.3_TB_per_s": 1e3 * nbytes_all / HBM_BYTES_PER_S / kernel_all_ms},
            "a_against_b_max_relative_difference": diff}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = "cuda:0"
    rows = []
    for name, T, N, C in (("balance1024", 64, 1024, 2), ("canonical65536", 64, 65536, 8)):
        rows.append(row(name, T, N, C, a.reps, dev, 0.25))
        torch.cuda.empty_cache()
        print(json.dumps(rows[-1]), flush=True)
    res = {"rows": rows, "device": torch.cuda.get_device_name(0), "reps": a.reps,
           "method": "one process, three warm-up calls of every side, then the sides timed in turn reps times; ms per "
                     "call = wall time of a whole call (loss and backward) between two synchronisations; the kernel pair "
                     "alone by device events over 10 back-to-back direct calls (output and workspace allocations included)"}
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()

"""Policy-gradient support: the numpy restatements of wg_rollout_stochastic's noise contract and of wg_gae
(include/walker_hip.h), which agree with the kernels bit for bit, gae() over the kernel, and collect(), one stochastic
rollout with the buffers a PPO update reads.

Noise.  aeps(seed, t, w, c) is the ES variate (walker_gym_amd.es) on another counter domain: one Philox4x32-10 call on
the counter (c, w, t, 0x41430001) under the key (seed lo, seed hi), the eight 16-bit halves of the output added, centred
and scaled: Irwin-Hall(8), unit variance, |aeps| <= 4.899.  Output unit c of walker w at step t:
  u = RN32(y + RN32(sigma[set][c] * aeps));   a = clip(u, -L, L)
with y the unit's chain value as MLPPolicy defines it.  The library reports aeps and u; the density a caller puts on
them (scripts/ppo_train.py: a Gaussian log-density on aeps) is the caller's business.

GAE.  With gl = RN32(gamma * lam), carry = +0.0, t descending, float32, every operation rounded by itself:
  nv = term[t] ? +0.0 : next_value[t];  delta = RN32(RN32(reward[t] + RN32(gamma * nv)) - value[t])
  c = cut[t] ? +0.0 : carry;            adv[t] = carry = RN32(delta + RN32(gl * c));  ret[t] = RN32(adv[t] + value[t])
Non-finite inputs flow through; the sign and payload of a NaN the arithmetic produces are not part of the contract (the
host keeps the NaN operand of a subtraction, the GPU computes a + (-b)).
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import _lib
from .es import NOISE_SCALE, philox4x32

ACTION_NOISE_TAG = 0x41430001   # counter word 3 of every action-noise call (the ES domain: 0x45530001)


# ---------------------------------------------------------------------------------------------------- host restatements
def action_noise_numpy(seed: int, step_base: int, n_steps: int, walker_base: int, n_walkers: int, act_dim: int):
    """aeps(seed, t, w, c) for t in [step_base, step_base + n_steps), w in [walker_base, walker_base + n_walkers),
    c in [0, act_dim): float32 [n_steps, n_walkers, act_dim]."""
    seed, step_base, walker_base = int(seed), int(step_base), int(walker_base)
    if not 0 <= seed < 1 << 64:
        raise ValueError("seed is a uint64")
    if step_base < 0 or step_base + int(n_steps) > 1 << 32 or walker_base < 0 or walker_base + int(n_walkers) > 1 << 32:
        raise ValueError("step_base + n_steps and walker_base + n_walkers must stay within 2^32")
    t = (np.arange(n_steps, dtype=np.uint64) + np.uint64(step_base))[:, None, None]
    w = (np.arange(n_walkers, dtype=np.uint64) + np.uint64(walker_base))[None, :, None]
    c = np.arange(act_dim, dtype=np.uint64)[None, None, :]
    ctr = np.stack(np.broadcast_arrays(c, w, t, np.uint64(ACTION_NOISE_TAG)), axis=-1)
    out = philox4x32(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)).astype(np.int64)
    s = ((out & 0xFFFF) + (out >> 16)).sum(axis=-1)    # the eight 16-bit halves
    return (s - 262140).astype(np.float32) * NOISE_SCALE


def stochastic_forward_numpy(policy, obs_rows, sigma, seed: int, t: int, walker_base: int = 0, first_walker: int = 0,
                             n_walkers_total: Optional[int] = None):
    """MLPPolicy.forward_numpy plus the noise: obs_rows [n, D] of walkers first_walker .. of a batch of
    n_walkers_total (what selects each row's parameter set), at step counter t (step_base + s), the noise's walker
    counter walker_base + first_walker + row.  sigma: float32 [G, C] (or [C], or a number).  Returns (u, a, aeps),
    float32 [n, C] each: the raw action, the clipped action, the variate."""
    x = np.ascontiguousarray(obs_rows, dtype=np.float32)
    n = x.shape[0]
    inf = policy.__class__(policy.w2, policy.b2, policy.w1, policy.b1, act_limit=float("inf"))
    y = inf.forward_numpy(x, first_walker, n_walkers_total)            # the chain value: no clip at L = inf
    sets = policy._sets(n, first_walker, n_walkers_total)
    sg = np.asarray(sigma.detach().cpu().numpy() if hasattr(sigma, "detach") else sigma, dtype=np.float32)
    sg = np.broadcast_to(sg, (policy.G, policy.C)) if sg.ndim < 2 else sg
    if sg.shape != (policy.G, policy.C):
        raise ValueError(f"sigma has shape {sg.shape}, expected {(policy.G, policy.C)}")
    srow = np.broadcast_to(sg[0], (n, policy.C)) if sets is None else sg[sets]
    e = action_noise_numpy(seed, t, 1, int(walker_base) + int(first_walker), n, policy.C)[0]
    with np.errstate(all="ignore"):
        u = (y + (srow * e).astype(np.float32)).astype(np.float32)
        L = np.float32(policy.act_limit)
        a = np.where(u < -L, -L, np.where(u > L, L, u)).astype(np.float32)
    return u, a, e


def gae_numpy(reward, value, next_value, term=None, cut=None, gamma: float = 0.99, lam: float = 0.95):
    """wg_gae's arithmetic on [T, N] host arrays: (adv, ret), float32 [T, N] each."""
    r = np.ascontiguousarray(reward, dtype=np.float32)
    v = np.ascontiguousarray(value, dtype=np.float32)
    nvs = np.ascontiguousarray(next_value, dtype=np.float32)
    T, N = r.shape
    g = np.float32(gamma)
    zero = np.float32(0.0)
    adv, ret = np.empty((T, N), np.float32), np.empty((T, N), np.float32)
    carry = np.zeros(N, np.float32)
    with np.errstate(all="ignore"):
        gl = np.float32(g * np.float32(lam))
        for t in range(T - 1, -1, -1):
            nv = nvs[t] if term is None else np.where(np.asarray(term[t]) != 0, zero, nvs[t]).astype(np.float32)
            delta = ((r[t] + g * nv).astype(np.float32) - v[t]).astype(np.float32)
            c = carry if cut is None else np.where(np.asarray(cut[t]) != 0, zero, carry).astype(np.float32)
            carry = (delta + (gl * c).astype(np.float32)).astype(np.float32)
            adv[t] = carry
            ret[t] = carry + v[t]
    return adv, ret


# ---------------------------------------------------------------------------------------------------- the kernel
def gae(reward, value, next_value, term=None, cut=None, gamma: float = 0.99, lam: float = 0.95, adv_out=None,
        ret_out=None, want_ret: bool = True):
    """wg_gae on device tensors: reward / value / next_value float32 [T, N], term / cut uint8 (or bool) [T, N] or None,
    all contiguous on one device.  Returns (adv, ret) ([T, N] float32; ret None with want_ret=False), written into
    adv_out / ret_out where given.  One launch on the current stream; ValueError for what the library refuses."""
    import torch
    from .batched_env import require_tensor
    if not isinstance(reward, torch.Tensor) or reward.dim() != 2:
        raise ValueError("gae: reward must be a [T, N] float32 device tensor")
    T, N = (int(s) for s in reward.shape)
    dv = reward.device
    require_tensor(reward, "reward", dv, torch.float32)
    require_tensor(value, "value", dv, torch.float32, (T, N))
    require_tensor(next_value, "next_value", dv, torch.float32, (T, N))
    flags = []
    for name, t in (("term", term), ("cut", cut)):
        if t is not None:
            if isinstance(t, torch.Tensor) and t.dtype == torch.bool:
                t = t.view(torch.uint8)
            require_tensor(t, name, dv, torch.uint8, (T, N))
        flags.append(t)
    adv = torch.empty((T, N), dtype=torch.float32, device=dv) if adv_out is None else adv_out
    require_tensor(adv, "adv_out", dv, torch.float32, (T, N))
    ret = ret_out if ret_out is not None else (torch.empty((T, N), dtype=torch.float32, device=dv) if want_ret else None)
    if ret is not None:
        require_tensor(ret, "ret_out", dv, torch.float32, (T, N))
    p = _lib.ptr
    stream = torch.cuda.current_stream(dv).cuda_stream
    _lib.check(_lib.load().wg_gae(p(reward), p(value), p(next_value), p(flags[0]), p(flags[1]), T, N, N, float(gamma),
                                  float(lam), p(adv), p(ret), stream), "wg_gae")
    return adv, ret


def collect(envs, policy, sigma, n_steps: int, seed: int, step_base: int = 0, value_fn=None, gamma: float = 0.99,
            lam: float = 0.95, walker_base: int = 0) -> dict:
    """One stochastic rollout of `envs` (a BatchedPhysicsEnv with auto-reset on) under `policy` with the buffers a PPO
    update reads, and its advantages.  value_fn maps observation rows [n, D] to values [n] (or [n, 1]); it is called
    under no_grad on all T * N recorded rows at once, on the N rows the rollout starts from, and on the final_obs rows
    of the walkers reset.  Row t of 'obs_before' is what step t acted on; value[t] = V(obs_before[t]); next_value[t] =
    V(the state after step t): V(final_obs[t]) where the walker was reset at t, V(obs[t]) elsewhere.  term = done &
    (steps != max_steps): the episode ended in a terminal state and not by the step limit, so nothing is bootstrapped;
    cut = reset: the trace stops at an episode boundary.

    Returns the rollout's stats dict plus 'obs_before', 'obs', 'reward', 'done', 'steps', 'reset', 'final_obs', 'action',
    'raw_action', 'eps' ([T, N, ...] device tensors), 'value', 'next_value', 'term', 'cut', 'adv', 'ret' ([T, N])."""
    import torch
    if value_fn is None:
        raise ValueError("collect: value_fn is required")
    if not envs._ar_mode:
        raise ValueError("collect: auto-reset is off (enable_auto_reset first): a PPO batch spans episode boundaries")
    T, N, D, Cc, dv = int(n_steps), envs.N, envs.obs_dim, policy.C, envs.device
    f = lambda *s: torch.empty(s, dtype=torch.float32, device=dv)
    u8 = lambda *s: torch.empty(s, dtype=torch.uint8, device=dv)
    buf = dict(obs_out=f(T, N, D), reward_out=f(T, N), done_out=u8(T, N),
               steps_out=torch.empty((T, N), dtype=torch.int32, device=dv), action_out=f(T, N, Cc),
               raw_action_out=f(T, N, Cc), eps_out=f(T, N, Cc), reset_out=u8(T, N),
               final_obs_out=torch.zeros((T, N, D), dtype=torch.float32, device=dv))
    obs0 = envs.observe()[0].clone()
    res = envs.rollout_stochastic(policy, T, sigma, seed, step_base=step_base, walker_base=walker_base, **buf)
    obs, reset = buf["obs_out"], buf["reset_out"]
    obs_before = torch.cat([obs0[None], obs[:-1]], dim=0)
    with torch.no_grad():
        value = value_fn(obs_before.reshape(T * N, D)).reshape(T, N).to(torch.float32).contiguous()
        # V(obs[t]) is value[t + 1] for t < T - 1 (the same rows): only the closing rows are new
        v_last = value_fn(obs[-1]).reshape(1, N).to(torch.float32)
        after = torch.cat([value[1:], v_last], dim=0)
        v_final = value_fn(buf["final_obs_out"].reshape(T * N, D)).reshape(T, N).to(torch.float32)
        next_value = torch.where(reset != 0, v_final, after).contiguous()
    term = ((buf["done_out"] != 0) & (buf["steps_out"] != int(envs.params.max_steps))).to(torch.uint8).contiguous()
    adv, ret = gae(buf["reward_out"], value, next_value, term, reset, gamma, lam)
    out = dict(res)
    out.update(obs_before=obs_before, obs=obs, reward=buf["reward_out"], done=buf["done_out"], steps=buf["steps_out"],
               reset=reset, final_obs=buf["final_obs_out"], action=buf["action_out"], raw_action=buf["raw_action_out"],
               eps=buf["eps_out"], value=value, next_value=next_value, term=term, cut=reset, adv=adv, ret=ret)
    return out

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

Action hold.  wg_rollout_held's walker decides at the steps where its counter at the start of the step is a multiple of
`every` (hold_decide_numpy) and applies the action in force between; hold_reward is the running reward of the open hold.
gae_held_numpy / gae_held are the GAE on that grid: step t closes a hold iff t == T - 1 or decided[t + 1]; a closing step
sets R = hold_reward[t], nv = term[t] ? +0.0 : next_value[t], cf = cut[t]; a decided step takes
  delta = RN32(RN32(R + RN32(gamma * nv)) - value[t]);  c = cf ? +0.0 : carry;  adv[t] = carry = RN32(delta + RN32(gl * c))
and the other steps get +0.0.  The discount is per decision (a hold is one transition), not per physics step, and a hold
the rollout's end cuts bootstraps from next_value[T - 1].

Differentiable rows.  policy_rows(policy, obs) is the MLPPolicy over recorded rows [T, N, D] as the rollout kernel
evaluated it (wg_policy_forward: the chain value before the clip), a torch.autograd.Function whose backward is
wg_policy_backward: per row, float32, every operation rounded by itself,
  d = +0.0; for c ascending: d = RN32(d + RN32(dy[c] * w2[j][c]));   dh[j] = (z[j] > 0) ? d : +0.0
and per parameter set, its rows numbered rho = t * n + (w - g * n) and cut into chunks of chunk_rows, float64 sums of
exact products in a fixed order:
  P_k[e] = +0.0; rho ascending over the chunk's unskipped rows: P_k[e] = RN64(P_k[e] + a * b)
  S[e] = +0.0; k ascending: S[e] = RN64(S[e] + P_k[e]);   grad[e] = RN32(S[e])
with (a, b) = (in[i], dy[c]) for w2[i][c], (1, dy[c]) for b2[c], (x[i], dh[j]) for w1[i][j], (1, dh[j]) for b1[j].
policy_rows_numpy and policy_grad_numpy restate both on the host, bit for bit.  There is no gradient with respect to
obs.  A policy that carries an obs_norm (walker_gym_amd.normalize) is evaluated on the normalised rows xn in all of
these (wg_policy_forward_normalized / wg_policy_backward_normalized): xn[i] takes x[i]'s place as the left factor, and
there is no gradient with respect to mean or scale.

The surrogate.  expf is the library's own exponential (wg_expf: float64, every operation rounded by itself, one rounding
to float32; expf_numpy restates it).  log_prob_rows is the Gaussian log-density of the recorded raw actions around
policy_rows' mean, and ppo_surrogate the clipped surrogate of a minibatch with its gradients with respect to that mean,
log_sigma and the critic's values, one kernel call (wg_ppo_surrogate; ppo_surrogate_numpy restates it).  Per unskipped
row, float32, every operation rounded by itself, c ascending from logp = +0.0:
  z[c] = RN32(RN32(u[c] - y[c]) / sigma[c]);  q[c] = RN32(z[c] * z[c])
  logp = RN32(logp + RN32(RN32(RN32(-0.5 * q[c]) - log_sigma[c]) - K0)),   K0 = RN32(0.5 ln 2 pi)
  d = RN32(logp - old_logp);  r = expf(d);  s1 = RN32(r * A);  s2 = RN32(clip(r, lo, hi) * A);  take = s1 <= s2
  wr = RN32(scale[0] * (take ? s1 : +0.0));   dy[c] = RN32(wr * RN32(z[c] / sigma[c]))
  ev = RN32(value - ret);   dvalue = RN32(scale[1] * ev)
and per set, in policy_grad_numpy's chunks and order, float64 sums of wr * RN32(q[c] - 1) (exact products) into
g_log_sigma and of five statistics (rows, surrogate, log-ratio, clipped, squared value error) into stats.

Advantages.  normalize_advantages(adv, mask) is (adv - mean) * scale on the unmasked rows and zero elsewhere, mean and
scale = 1 / sqrt(var + eps) taken from one wg_obs_moments call on adv as one column (normalize.py's ordered float64 sums
over the rows that are unmasked and finite): no gather of the unmasked rows, nothing waits for the device.
normalize_advantages_numpy restates it.  The step that follows an update's backward is walker_gym_amd.optim.Adam.
"""
from __future__ import annotations

import math
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
    inf = policy.__class__(policy.w2, policy.b2, policy.w1, policy.b1, act_limit=float("inf"),
                           obs_norm=getattr(policy, "obs_norm", None), **_mid_of(policy))
    y = inf.forward_numpy(x, first_walker, n_walkers_total)           # the chain value: no clip at L = inf
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


def hold_decide_numpy(steps, every: int):
    """wg_rollout_held's decision rule: uint8, 1 where a walker whose counter at the start of the step is steps[w]
    decides, (uint32)steps % every == 0."""
    every = int(every)
    if every < 1:
        raise ValueError("every < 1")
    st = np.asarray(steps).astype(np.int64) & 0xFFFFFFFF
    return (st % every == 0).astype(np.uint8)


def gae_held_numpy(hold_reward, value, next_value, decided, term=None, cut=None, gamma: float = 0.99, lam: float = 0.95):
    """wg_gae_held's arithmetic on [T, N] host arrays: (adv, ret), float32 [T, N] each."""
    hr = np.ascontiguousarray(hold_reward, dtype=np.float32)
    v = np.ascontiguousarray(value, dtype=np.float32)
    nvs = np.ascontiguousarray(next_value, dtype=np.float32)
    dec = np.asarray(decided).reshape(hr.shape) != 0
    T, N = hr.shape
    g, zero = np.float32(gamma), np.float32(0.0)
    adv, ret = np.zeros((T, N), np.float32), np.zeros((T, N), np.float32)
    carry, R, nv = np.zeros(N, np.float32), np.zeros(N, np.float32), np.zeros(N, np.float32)
    cf = np.zeros(N, bool)
    closes = np.ones(N, bool)
    with np.errstate(all="ignore"):
        gl = np.float32(g * np.float32(lam))
        for t in range(T - 1, -1, -1):
            tm = np.zeros(N, bool) if term is None else np.asarray(term[t]) != 0
            ct = np.zeros(N, bool) if cut is None else np.asarray(cut[t]) != 0
            R = np.where(closes, hr[t], R).astype(np.float32)
            nv = np.where(closes, np.where(tm, zero, nvs[t]), nv).astype(np.float32)
            cf = np.where(closes, ct, cf)
            delta = ((R + g * nv).astype(np.float32) - v[t]).astype(np.float32)
            c = np.where(cf, zero, carry).astype(np.float32)
            a = (delta + (gl * c).astype(np.float32)).astype(np.float32)
            carry = np.where(dec[t], a, carry).astype(np.float32)
            adv[t] = np.where(dec[t], a, zero)
            ret[t] = np.where(dec[t], (a + v[t]).astype(np.float32), zero)
            closes = dec[t]
    return adv, ret


def _mid_of(policy) -> dict:
    """The middle layer of a deep policy as MLPPolicy's keyword arguments (empty for a shallow one)."""
    return dict(wm=policy.wm, bm=policy.bm) if getattr(policy, "H2", 0) else {}


def _sets_of(policy, N: int):
    if policy.G > 1 and N % policy.G != 0:
        raise ValueError(f"{N} walkers do not divide into {policy.G} parameter sets")
    return np.arange(N, dtype=np.int64) // (N // policy.G)


def _rows_arrays(policy, x, mask):
    x = np.ascontiguousarray(x, dtype=np.float32)
    if x.ndim != 3 or x.shape[2] != policy.D:
        raise ValueError(f"x must be [T, N, {policy.D}], got {x.shape}")
    T, N, _ = x.shape
    on = np.ones((T, N), bool) if mask is None else np.asarray(mask).reshape(T, N) != 0
    return x, on, _sets_of(policy, N)


def policy_rows_numpy(policy, x, mask=None):
    """wg_policy_forward on the host: MLPPolicy.forward_numpy at act_limit = inf, step by step over x [T, N, D].
    Returns float32 [T, N, C]; the rows mask skips (mask [T, N], 0 = skipped) are zero."""
    x, on, _ = _rows_arrays(policy, x, mask)
    T, N, _ = x.shape
    inf = policy.__class__(policy.w2, policy.b2, policy.w1, policy.b1, act_limit=float("inf"),
                           obs_norm=getattr(policy, "obs_norm", None), **_mid_of(policy))
    y = np.zeros((T, N, policy.C), np.float32)
    for t in range(T):
        y[t] = np.where(on[t][:, None], inf.forward_numpy(x[t], 0, N), np.float32(0.0))
    return y


def policy_grad_numpy(policy, x, dy, mask=None, chunk_rows: int = 256):
    """wg_policy_backward on the host: float32 chains, float64 sums, in the contract's order (see the module's
    docstring).  x [T, N, D], dy [T, N, C], mask [T, N] or None.  Returns (g_w1, g_b1, g_w2, g_b2), float32 arrays
    shaped like the policy's tensors ([G, D, H], [G, H], [G, n2, C], [G, C]), None for what the policy does not have.
    A deep policy (H2 > 0) returns six: (g_w1, g_b1, g_wm, g_bm, g_w2, g_b2), wg_policy_backward_deep's."""
    x, on, sets = _rows_arrays(policy, x, mask)
    if getattr(policy, "obs_norm", None) is not None:
        x = policy.obs_norm.normalize_numpy(x)      # the layers and both outer products see xn
    T, N, D = x.shape
    G, H, Cc = policy.G, policy.H, policy.C
    dy = np.ascontiguousarray(dy, dtype=np.float32)
    if dy.shape != (T, N, Cc):
        raise ValueError(f"dy must be {(T, N, Cc)}, got {dy.shape}")
    chunk_rows = int(chunk_rows)
    if chunk_rows < 1:
        raise ValueError("chunk_rows < 1")
    host = lambda t: None if t is None else t.detach().cpu().numpy()
    w1, b1, w2, b2 = host(policy.w1), host(policy.b1), host(policy.w2), host(policy.b2)
    H2 = getattr(policy, "H2", 0)
    wm, bm = (host(policy.wm), host(policy.bm)) if H2 else (None, None)
    n, zero = N // G, np.float32(0.0)
    with np.errstate(all="ignore"):
        inp, dh = x, None
        if H2:
            z1 = np.zeros((T, N, H), np.float32) if b1 is None else np.broadcast_to(b1[sets], (T, N, H)).copy()
            for i in range(D):
                z1 = z1 + x[:, :, i:i + 1] * w1[sets, i][None]       # RN32 of the product, then RN32 of the sum
            h1 = np.where(z1 > 0, z1, zero).astype(np.float32)
            z2 = np.zeros((T, N, H2), np.float32) if bm is None else np.broadcast_to(bm[sets], (T, N, H2)).copy()
            for j in range(H):
                z2 = z2 + h1[:, :, j:j + 1] * wm[sets, j][None]
            inp = np.where(z2 > 0, z2, zero).astype(np.float32)
            d = np.zeros((T, N, H2), np.float32)
            for c in range(Cc):
                d = d + dy[:, :, c:c + 1] * w2[sets, :, c][None]
            dh2 = np.where(z2 > 0, d, zero).astype(np.float32)
            d = np.zeros((T, N, H), np.float32)
            for k in range(H2):
                d = d + dh2[:, :, k:k + 1] * wm[sets, :, k][None]
            dh = np.where(z1 > 0, d, zero).astype(np.float32)
        elif H:
            z = np.zeros((T, N, H), np.float32) if b1 is None else np.broadcast_to(b1[sets], (T, N, H)).copy()
            for i in range(D):
                z = z + x[:, :, i:i + 1] * w1[sets, i][None]         # RN32 of the product, then RN32 of the sum
            inp = np.where(z > 0, z, zero).astype(np.float32)
            d = np.zeros((T, N, H), np.float32)
            for c in range(Cc):
                d = d + dy[:, :, c:c + 1] * w2[sets, :, c][None]
            dh = np.where(z > 0, d, zero).astype(np.float32)

        def ordered(a, b, bias):
            """S[g] over the set's rows of (a|1) (x) b: a [T, N, I], b [T, N, J] -> float32 [G, I (+ 1), J]."""
            if bias:
                a = np.concatenate([a, np.ones(a.shape[:2] + (1,), np.float32)], axis=2)
            a = a.astype(np.float64).reshape(T, G, n, -1)
            b = b.astype(np.float64).reshape(T, G, n, -1)
            v = on.reshape(T, G, n)
            S = np.zeros((G, a.shape[3], b.shape[3]), np.float64)
            P = np.zeros_like(S)
            for rho in range(T * n):
                if rho and rho % chunk_rows == 0:
                    S, P = S + P, np.zeros_like(S)
                t, r = divmod(rho, n)
                P = np.where(v[t, :, r, None, None], P + a[t, :, r, :, None] * b[t, :, r, None, :], P)
            return (S + P).astype(np.float32)

        g2 = ordered(inp, dy, b2 is not None)
        n2 = inp.shape[2]
        g_w2, g_b2 = np.ascontiguousarray(g2[:, :n2]), (None if b2 is None else np.ascontiguousarray(g2[:, n2]))
        g_w1 = g_b1 = None
        if H:
            g1 = ordered(x, dh, b1 is not None)
            g_w1, g_b1 = np.ascontiguousarray(g1[:, :D]), (None if b1 is None else np.ascontiguousarray(g1[:, D]))
        if H2:
            gm = ordered(h1, dh2, bm is not None)
            g_wm, g_bm = np.ascontiguousarray(gm[:, :H]), (None if bm is None else np.ascontiguousarray(gm[:, H]))
            return g_w1, g_b1, g_wm, g_bm, g_w2, g_b2
    return g_w1, g_b1, g_w2, g_b2


# ---------------------------------------------------------------------------------------------------- the kernels
def _rows_struct(policy, obs, mask, who):
    """(wg_policy, wg_policy_rows, T, N, the 3-D views kept alive) of obs [T, N, D] / [R, D] and mask [T, N] / [R]."""
    rows, T, N, o3, m3, flat = _rows_of(policy.D, policy.device, obs, mask, who)
    return policy.struct(N), rows, T, N, o3, m3, flat


def _rows_of(width, device, obs, mask, who):
    """_rows_struct without the policy: rows of `width` values on `device`."""
    import torch
    if not isinstance(obs, torch.Tensor) or obs.dim() not in (2, 3) or obs.dtype != torch.float32:
        raise ValueError(f"{who}: obs must be a float32 device tensor [T, N, D] or [R, D]")
    flat = obs.dim() == 2
    o3 = obs[None] if flat else obs
    T, N, D = (int(v) for v in o3.shape)
    if D != width or obs.device != device:
        raise ValueError(f"{who}: obs is [.., {D}] on {obs.device}, the policy takes {width} values on {device}")
    if T < 1 or N < 1:
        raise ValueError(f"{who}: no rows")
    if o3.stride(2) != 1 or o3.stride(1) != D or (T > 1 and o3.stride(0) < N * D):
        raise ValueError(f"{who}: only the step dimension of obs may be strided (strides {tuple(o3.stride())})")
    m3 = None
    if mask is not None:
        if not isinstance(mask, torch.Tensor) or mask.device != obs.device:
            raise ValueError(f"{who}: mask must be a uint8 or bool tensor on {obs.device}")
        if mask.dtype == torch.bool:
            mask = mask.view(torch.uint8)
        m3 = mask[None] if flat else mask
        if mask.dtype != torch.uint8 or tuple(m3.shape) != (T, N) or m3.stride(1) != 1 or (T > 1 and m3.stride(0) < N):
            raise ValueError(f"{who}: mask must be uint8 / bool {(T, N)} with only its step dimension strided")
    rows = _lib.WgPolicyRows(x=_lib.ptr(o3), x_step=o3.stride(0) if T > 1 else N * D, mask=_lib.ptr(m3),
                             mask_step=(m3.stride(0) if T > 1 else N) if m3 is not None else 0, n_steps=T, N=N)
    return rows, T, N, o3, m3, flat


def _obs_norm_of(policy, who):
    """policy.obs_norm, checked against the policy (None: a plain policy)."""
    nm = getattr(policy, "obs_norm", None)
    if nm is not None and (nm.D != policy.D or nm.device != policy.device):
        raise ValueError(f"{who}: obs_norm is [{nm.D}] on {nm.device}, the policy takes {policy.D} values on "
                         f"{policy.device}")
    return nm


def default_chunk_rows(T: int, n: int) -> int:
    """policy_rows' chunk_rows: 256 rows, more once a set has over 512 such chunks (the workspace stays near 512 K
    doubles per set)."""
    return max(256, -(-(T * n) // 512))


def policy_rows_forward(policy, obs, mask=None, y_out=None):
    """wg_policy_forward called directly (no autograd): y [T, N, C] (or [R, C]) of the rows of obs, written into y_out
    where given (float32 [T, N, C], only its step dimension strided; skipped rows of a y_out are left as they are).
    Without y_out the skipped rows are zero."""
    import torch
    pol, rows, T, N, o3, m3, flat = _rows_struct(policy, obs, mask, "policy_rows_forward")
    Cc, dv = policy.C, obs.device
    if y_out is None:
        y = (torch.empty if m3 is None else torch.zeros)((T, N, Cc), dtype=torch.float32, device=dv)
    else:
        y = y_out[None] if (flat and isinstance(y_out, torch.Tensor) and y_out.dim() == 2) else y_out
        if (not isinstance(y, torch.Tensor) or y.dtype != torch.float32 or y.device != dv or tuple(y.shape) != (T, N, Cc)
                or y.stride(2) != 1 or y.stride(1) != Cc):
            raise ValueError(f"policy_rows_forward: y_out must be float32 {(T, N, Cc)} with only its step dimension strided")
    stream = torch.cuda.current_stream(dv).cuda_stream
    nm, L = _obs_norm_of(policy, "policy_rows_forward"), _lib.load()
    if getattr(policy, "H2", 0):
        _lib.check(L.wg_policy_forward_deep(pol, policy.mid_struct(), None if nm is None else nm.struct(), rows,
                                            _lib.ptr(y), y.stride(0) if T > 1 else N * Cc, stream),
                   "wg_policy_forward_deep")
    elif nm is None:
        _lib.check(L.wg_policy_forward(pol, rows, _lib.ptr(y), y.stride(0) if T > 1 else N * Cc, stream),
                   "wg_policy_forward")
    else:
        _lib.check(L.wg_policy_forward_normalized(pol, nm.struct(), rows, _lib.ptr(y), y.stride(0) if T > 1 else N * Cc,
                                                  stream), "wg_policy_forward_normalized")
    return y[0] if flat else y


_ROWS_FN = None


def _rows_function():
    global _ROWS_FN
    if _ROWS_FN is not None:
        return _ROWS_FN
    import torch

    class PolicyRows(torch.autograd.Function):
        @staticmethod
        def forward(ctx, policy, obs, mask, chunk_rows, w1, b1, w2, b2, wm=None, bm=None):
            ctx.policy, ctx.chunk_rows = policy, chunk_rows
            ctx.save_for_backward(obs, mask)
            return policy_rows_forward(policy, obs, mask)

        @staticmethod
        def backward(ctx, dy):
            need = ctx.needs_input_grad[4:10]
            if not any(need):
                return (None,) * 10
            obs, mask = ctx.saved_tensors
            dy = dy.to(torch.float32).contiguous()
            if ctx.policy.H2:   # (the inputs are w1, b1, w2, b2, wm, bm; the deep call's order is w1, b1, wm, bm, w2, b2)
                want = (need[0], need[1], need[4], need[5], need[2], need[3])
                g = policy_rows_backward(ctx.policy, obs, dy, mask, ctx.chunk_rows, want)
                return (None, None, None, None, g[0], g[1], g[4], g[5], g[2], g[3])
            grads = policy_rows_backward(ctx.policy, obs, dy, mask, ctx.chunk_rows, need[:4])
            return (None, None, None, None, *grads, None, None)

    _ROWS_FN = PolicyRows
    return PolicyRows


def policy_rows(policy, obs, mask=None, chunk_rows: Optional[int] = None):
    """The chain values y of `policy` (an MLPPolicy: before the clip, act_limit ignored) on the recorded rows obs
    [T, N, D], or [R, D] read as T = 1, N = R: float32 [T, N, C] (or [R, C]), bit for bit what the rollout kernels add
    their noise to.  Row (t, w) uses parameter set w // (N // G).  obs is a float32 device tensor; only its step
    dimension may be strided (a window of a longer buffer passes without a copy).  mask, uint8 or bool [T, N] (or
    [R]): rows with 0 are skipped (they may hold anything, NaN included); their y is zero and they add nothing to any
    gradient: a minibatch is a row mask.

    Differentiable with respect to policy.w1 / b1 / w2 / b2 (and wm / bm of a deep policy), whichever require grad
    (MLPPolicy keeps the tensors it was given by identity: make them nn.Parameters or leaves with requires_grad); what
    the autograd engine does not need is not computed.  There is NO gradient with respect to obs: its grad stays None.  The backward's sums are ordered
    (module docstring), chunk_rows rows per float64 partial sum, default max(256, ceil(T * n / 512)); two calls give
    identical bits.  The float64 workspace is allocated per call.  ValueError for what the library refuses."""
    return _rows_function().apply(policy, obs, mask, chunk_rows, policy.w1, policy.b1, policy.w2, policy.b2,
                                  getattr(policy, "wm", None), getattr(policy, "bm", None))


def policy_rows_backward(policy, obs, dy, mask=None, chunk_rows: Optional[int] = None, want=(True, True, True, True)):
    """wg_policy_backward called directly: (g_w1, g_b1, g_w2, g_b2) of dy [T, N, C] (or [R, C]) on the rows of obs, None
    where `want` is False or the policy has no such tensor.  What policy_rows' autograd backward runs.  A deep policy
    (H2 > 0) gives six, (g_w1, g_b1, g_wm, g_bm, g_w2, g_b2), and takes a `want` of six (the default: all)."""
    import torch
    pol, rows, T, N, o3, m3, flat = _rows_struct(policy, obs, mask, "policy_rows_backward")
    dv = obs.device
    if not isinstance(dy, torch.Tensor) or dy.dtype != torch.float32 or dy.device != dv:
        raise ValueError("policy_rows_backward: dy must be a float32 tensor on the rows' device")
    d3 = dy[None] if dy.dim() == 2 else dy
    if tuple(d3.shape) != (T, N, policy.C) or d3.stride(2) != 1 or d3.stride(1) != policy.C:
        raise ValueError(f"policy_rows_backward: dy must be {(T, N, policy.C)} with only its step dimension strided")
    chunk = default_chunk_rows(T, N // policy.G) if chunk_rows is None else int(chunk_rows)
    L = _lib.load()
    deep = bool(getattr(policy, "H2", 0))
    mid = policy.mid_struct() if deep else None
    if deep:
        count = L.wg_policy_backward_deep_workspace(pol, mid, rows, chunk)
        _lib.check(count, "wg_policy_backward_deep_workspace")
        tensors = (policy.w1, policy.b1, policy.wm, policy.bm, policy.w2, policy.b2)
        want = tuple(want) if len(tuple(want)) == 6 else (True,) * 6
    else:
        count = L.wg_policy_backward_workspace(pol, rows, chunk)
        _lib.check(count, "wg_policy_backward_workspace")
        tensors = (policy.w1, policy.b1, policy.w2, policy.b2)
    ws = torch.empty(int(count), dtype=torch.float64, device=dv)
    grads = [torch.empty_like(t) if (k and t is not None) else None for t, k in zip(tensors, want)]
    p = _lib.ptr
    nm = _obs_norm_of(policy, "policy_rows_backward")
    tail = (p(d3), d3.stride(0) if T > 1 else N * policy.C, chunk, p(ws), *(p(g) for g in grads),
            torch.cuda.current_stream(dv).cuda_stream)
    if deep:
        _lib.check(L.wg_policy_backward_deep(pol, mid, None if nm is None else nm.struct(), rows, *tail),
                   "wg_policy_backward_deep")
    elif nm is None:
        _lib.check(L.wg_policy_backward(pol, rows, *tail), "wg_policy_backward")
    else:
        _lib.check(L.wg_policy_backward_normalized(pol, nm.struct(), rows, *tail), "wg_policy_backward_normalized")
    return tuple(grads)


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


def gae_held(hold_reward, value, next_value, decided, term=None, cut=None, gamma: float = 0.99, lam: float = 0.95,
             adv_out=None, ret_out=None, want_ret: bool = True):
    """wg_gae_held on device tensors: gae() on the decision grid of rollout_held.  hold_reward / value / next_value
    float32 [T, N], decided uint8 (or bool) [T, N], term / cut likewise or None, all contiguous on one device.  value is
    read on the decided steps, next_value / term / cut on the steps that close a hold.  Returns (adv, ret), zero on the
    steps that did not decide; one launch on the current stream; ValueError for what the library refuses."""
    import torch
    from .batched_env import require_tensor
    if not isinstance(hold_reward, torch.Tensor) or hold_reward.dim() != 2:
        raise ValueError("gae_held: hold_reward must be a [T, N] float32 device tensor")
    T, N = (int(s) for s in hold_reward.shape)
    dv = hold_reward.device
    require_tensor(hold_reward, "hold_reward", dv, torch.float32)
    require_tensor(value, "value", dv, torch.float32, (T, N))
    require_tensor(next_value, "next_value", dv, torch.float32, (T, N))
    if decided is None:
        raise ValueError("gae_held: decided is required")
    flags = []
    for name, t in (("decided", decided), ("term", term), ("cut", cut)):
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
    _lib.check(_lib.load().wg_gae_held(p(hold_reward), p(value), p(next_value), p(flags[0]), p(flags[1]), p(flags[2]), T,
                                       N, N, float(gamma), float(lam), p(adv), p(ret), stream), "wg_gae_held")
    return adv, ret


def _collect_held(envs, policy, sigma, T, seed, step_base, value_fn, gamma, lam, walker_base, every, held) -> dict:
    """collect() with an action hold: the rollout through rollout_held, the values on the decision grid."""
    import torch
    if not envs._ar_mode & 1:
        raise ValueError("collect: act_every > 1 needs 'done' in the auto-reset set (a hold ends with its episode)")
    N, D, Cc, dv = envs.N, envs.obs_dim, policy.C, envs.device
    f = lambda *s: torch.empty(s, dtype=torch.float32, device=dv)
    z = lambda *s: torch.zeros(s, dtype=torch.float32, device=dv)
    u8 = lambda *s: torch.empty(s, dtype=torch.uint8, device=dv)
    buf = dict(obs_out=f(T, N, D), reward_out=f(T, N), done_out=u8(T, N),
               steps_out=torch.empty((T, N), dtype=torch.int32, device=dv), action_out=f(T, N, Cc),
               raw_action_out=z(T, N, Cc), eps_out=z(T, N, Cc), reset_out=u8(T, N), final_obs_out=z(T, N, D),
               decided_out=u8(T, N), hold_reward_out=f(T, N))
    obs0 = envs.observe()[0].clone()
    res = envs.rollout_held(policy, T, every, sigma=sigma, seed=seed, step_base=step_base, walker_base=walker_base,
                            held=held, **buf)
    obs, reset, decided = buf["obs_out"], buf["reset_out"], buf["decided_out"]
    obs_before = torch.cat([obs0[None], obs[:-1]], dim=0)
    dec = decided != 0
    closes = torch.cat([dec[1:], torch.ones((1, N), dtype=torch.bool, device=dv)], dim=0)
    value, next_value = z(T, N), z(T, N)
    with torch.no_grad():
        if bool(dec.any()):
            value[dec] = value_fn(obs_before[dec]).reshape(-1).to(torch.float32)
        after = torch.where((reset != 0)[:, :, None], buf["final_obs_out"], obs)
        next_value[closes] = value_fn(after[closes]).reshape(-1).to(torch.float32)
    term = ((buf["done_out"] != 0) & (buf["steps_out"] != int(envs.params.max_steps))).to(torch.uint8).contiguous()
    adv, ret = gae_held(buf["hold_reward_out"], value, next_value, decided, term, reset, gamma, lam)
    out = dict(res)
    out.update(obs_before=obs_before, obs=obs, reward=buf["reward_out"], done=buf["done_out"], steps=buf["steps_out"],
               reset=reset, final_obs=buf["final_obs_out"], action=buf["action_out"], raw_action=buf["raw_action_out"],
               eps=buf["eps_out"], value=value, next_value=next_value, term=term, cut=reset, adv=adv, ret=ret,
               decided=decided, hold_reward=buf["hold_reward_out"])
    return out


def collect(envs, policy, sigma, n_steps: int, seed: int, step_base: int = 0, value_fn=None, gamma: float = 0.99,
            lam: float = 0.95, walker_base: int = 0, act_every: int = 1, held=None) -> dict:
    """One stochastic rollout of `envs` (a BatchedPhysicsEnv with auto-reset on) under `policy` with the buffers a PPO
    update reads, and its advantages.  value_fn maps observation rows [n, D] to values [n] (or [n, 1]); it is called
    under no_grad on all T * N recorded rows at once, on the N rows the rollout starts from, and on the final_obs rows
    of the walkers reset.  Row t of 'obs_before' is what step t acted on; value[t] = V(obs_before[t]); next_value[t] =
    V(the state after step t): V(final_obs[t]) where the walker was reset at t, V(obs[t]) elsewhere.  term = done &
    (steps != max_steps): the episode ended in a terminal state and not by the step limit, so nothing is bootstrapped;
    cut = reset: the trace stops at an episode boundary.

    Returns the rollout's stats dict plus 'obs_before', 'obs', 'reward', 'done', 'steps', 'reset', 'final_obs', 'action',
    'raw_action', 'eps' ([T, N, ...] device tensors), 'value', 'next_value', 'term', 'cut', 'adv', 'ret' ([T, N]).

    act_every > 1 (needs 'done' in the auto-reset set): the rollout is rollout_held's with that hold, `held` its in/out
    state (None: zeros; pass the returned 'held' and an advanced step_base to continue).  value_fn is then called on the
    decided rows of obs_before and on the rows that close a hold (final_obs where the walker was reset, obs elsewhere);
    'value' and 'next_value' are zero elsewhere, as are 'raw_action' / 'eps' on the held rows; 'adv' / 'ret' are
    gae_held's (zero on the held rows); 'decided', 'hold_reward' and 'held' are added.  A PPO update masks its rows
    with 'decided'."""
    import torch
    if value_fn is None:
        raise ValueError("collect: value_fn is required")
    if not envs._ar_mode:
        raise ValueError("collect: auto-reset is off (enable_auto_reset first): a PPO batch spans episode boundaries")
    if int(act_every) < 1:
        raise ValueError(f"collect: act_every {act_every} < 1")
    if int(act_every) > 1:
        return _collect_held(envs, policy, sigma, int(n_steps), seed, step_base, value_fn, gamma, lam, walker_base,
                             int(act_every), held)
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


# ---------------------------------------------------------------------------------------------------- the fused surrogate
# wg_expf (include/walker_hip.h; csrc/wg_expf.h): the library's own exponential, and wg_ppo_surrogate, the clipped
# surrogate over recorded rows.  expf_numpy / ppo_surrogate_numpy restate both contracts on the host, bit for bit;
# expf / log_prob_rows / ppo_surrogate are the device calls.
EXPF_LOG2E = float.fromhex("0x1.71547652b82fep+0")
EXPF_LN2_HI = float.fromhex("0x1.62e42fee00000p-1")
EXPF_LN2_LO = float.fromhex("0x1.a39ef35793c76p-33")
EXPF_C = tuple(1.0 / math.factorial(n) for n in range(14))   # RN64(1 / n!): n! is exact in float64 up to 13!
LOGP_K0 = np.array([0x3F6B3F8E], np.uint32).view(np.float32)[0]   # RN32(0.5 * ln(2 pi))
PPO_STATS = ("rows", "surrogate", "log_ratio", "clipped", "value_error")


def expf_numpy(x):
    """wg_expf on the host: float32 in, float32 out, every float64 operation rounded by itself (numpy never fuses)."""
    x = np.asarray(x, dtype=np.float32)
    nan = np.isnan(x)
    xd = np.clip(np.where(nan, np.float32(0.0), x).astype(np.float64), -150.0, 150.0)
    k = np.rint(xd * np.float64(EXPF_LOG2E))
    r = (xd - k * np.float64(EXPF_LN2_HI)) - k * np.float64(EXPF_LN2_LO)
    p = np.full_like(xd, EXPF_C[13])
    for n in range(12, -1, -1):
        p = p * r + np.float64(EXPF_C[n])
    with np.errstate(over="ignore", under="ignore"):
        out = np.ldexp(p, k.astype(np.int32)).astype(np.float32)
    return np.where(nan, x, out)


def ppo_surrogate_numpy(y, u, sigma, log_sigma, old_logp=None, adv=None, mask=None, clip_eps: float = 0.2, scale=None,
                        value=None, ret=None, chunk_rows: int = 256):
    """wg_ppo_surrogate on the host.  y, u [T, N, C]; sigma, log_sigma [G, C] (or [C]); old_logp, adv, value, ret, mask
    [T, N].  old_logp None: the density mode, {'logp'} alone.  Otherwise scale = (actor, value coefficient) and the
    result holds 'logp', 'dy', 'dvalue' (None without value), 'g_log_sigma' [G, C] and 'stats' float64 [5] (PPO_STATS).
    Skipped rows of logp / dy / dvalue are zero here (the kernel leaves them as they were)."""
    f32 = np.float32
    y = np.ascontiguousarray(y, dtype=f32)
    u = np.ascontiguousarray(u, dtype=f32)
    if y.ndim != 3 or u.shape != y.shape:
        raise ValueError(f"y and u must be [T, N, C] alike, got {y.shape} and {u.shape}")
    T, N, Cc = y.shape
    sg = np.asarray(sigma, dtype=f32).reshape(-1, Cc)
    ls = np.asarray(log_sigma, dtype=f32).reshape(-1, Cc)
    G = sg.shape[0]
    if ls.shape != sg.shape or N % G != 0:
        raise ValueError(f"sigma {sg.shape} / log_sigma {ls.shape} must be [G, {Cc}] alike with G dividing N = {N}")
    n = N // G
    sets = np.arange(N) // n
    on = np.ones((T, N), bool) if mask is None else np.asarray(mask).reshape(T, N) != 0
    zero = f32(0.0)
    with np.errstate(all="ignore"):
        # (skipped rows may hold anything: they are computed on zeros and dropped)
        ym, um = np.where(on[..., None], y, zero), np.where(on[..., None], u, zero)
        z = (um - ym) / sg[sets][None]
        q = z * z
        l = (f32(-0.5) * q - ls[sets][None]) - LOGP_K0
        logp = np.zeros((T, N), f32)
        for c in range(Cc):
            logp = logp + l[:, :, c]
        out = {"logp": np.where(on, logp, zero)}
        if old_logp is None:
            return out
        if adv is None or scale is None:
            raise ValueError("the loss mode needs adv and scale")
        if (value is None) != (ret is None):
            raise ValueError("value and ret go together")
        chunk_rows = int(chunk_rows)
        if chunk_rows < 1:
            raise ValueError("chunk_rows < 1")
        sc = np.asarray(scale, dtype=f32).reshape(-1)
        lo, hi = f32(1.0) - f32(clip_eps), f32(1.0) + f32(clip_eps)
        d = logp - np.where(on, np.asarray(old_logp, dtype=f32).reshape(T, N), zero)
        r = expf_numpy(d)
        A = np.where(on, np.asarray(adv, dtype=f32).reshape(T, N), zero)
        s1 = r * A
        rc = np.where(r < lo, lo, np.where(r > hi, hi, r)).astype(f32)
        s2 = rc * A
        take = s1 <= s2
        surr = np.where(take, s1, s2)
        wr = sc[0] * np.where(take, s1, zero)
        out["dy"] = np.where(on[..., None], wr[..., None] * (z / sg[sets][None]), zero)
        qm1 = q - f32(1.0)
        ev = np.zeros((T, N), f32)
        out["dvalue"] = None
        if value is not None:
            ev = np.where(on, np.asarray(value, dtype=f32).reshape(T, N) - np.asarray(ret, dtype=f32).reshape(T, N), zero)
            out["dvalue"] = np.where(on, sc[1] * ev, zero)
        f64 = np.float64
        terms = np.concatenate([wr.astype(f64)[..., None] * qm1.astype(f64), np.ones((T, N, 1)), surr.astype(f64)[..., None],
                                d.astype(f64)[..., None], (rc != r).astype(f64)[..., None],
                                (ev.astype(f64) * ev.astype(f64))[..., None]], axis=2).reshape(T, G, n, Cc + 5)
        v = on.reshape(T, G, n)
        S, P = np.zeros((G, Cc + 5)), np.zeros((G, Cc + 5))
        for rho in range(T * n):
            if rho and rho % chunk_rows == 0:
                S, P = S + P, np.zeros_like(P)
            t, i = divmod(rho, n)
            P = np.where(v[t, :, i, None], P + terms[t, :, i], P)
        S = S + P
        out["g_log_sigma"] = S[:, :Cc].astype(f32)
        stats = np.zeros(5)
        for g in range(G):
            stats = stats + S[g, Cc:]
        out["stats"] = stats
    return out


def _vec(t, who, name, dv, n=None):
    import torch
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != dv or not t.is_contiguous():
        raise ValueError(f"{who}: {name} must be a contiguous float32 tensor on {dv}")
    if n is not None and t.numel() != n:
        raise ValueError(f"{who}: {name} has {t.numel()} elements, expected {n}")
    return t


def expf(x, out=None):
    """wg_expf on a contiguous float32 device tensor: the library's exponential, elementwise (out may be x)."""
    import torch
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise ValueError("expf: x must be a float32 device tensor")
    x = _vec(x, "expf", "x", x.device)
    out = torch.empty_like(x) if out is None else _vec(out, "expf", "out", x.device, x.numel())
    if x.numel() == 0:
        return out
    _lib.check(_lib.load().wg_expf(_lib.ptr(x), x.numel(), _lib.ptr(out), torch.cuda.current_stream(x.device).cuda_stream),
               "wg_expf")
    return out


def _ppo_rows(mean, raw_action, sigma, log_sigma, mask, who):
    """(wg_ppo_rows, T, N, G, C, flat, what must stay alive) of mean / raw_action [T, N, C] or [R, C]."""
    import torch
    if not isinstance(mean, torch.Tensor) or mean.dim() not in (2, 3) or mean.dtype != torch.float32 or not mean.is_cuda:
        raise ValueError(f"{who}: mean must be a float32 device tensor [T, N, C] or [R, C]")
    Cc = int(mean.shape[-1])
    rows_y, T, N, y3, m3, flat = _rows_of(Cc, mean.device, mean, mask, who)
    if not isinstance(raw_action, torch.Tensor) or raw_action.shape != mean.shape or raw_action.dtype != torch.float32:
        raise ValueError(f"{who}: raw_action must be float32 {tuple(mean.shape)}")
    rows_u, _, _, u3, _, _ = _rows_of(Cc, mean.device, raw_action, None, who)
    ls = _vec(log_sigma, who, "log_sigma", mean.device)
    sg = _vec(sigma, who, "sigma", mean.device, ls.numel())
    if ls.dim() not in (1, 2) or ls.shape[-1] != Cc:
        raise ValueError(f"{who}: log_sigma must be [{Cc}] or [G, {Cc}], got {tuple(ls.shape)}")
    G = 1 if ls.dim() == 1 else int(ls.shape[0])
    rows = _lib.WgPpoRows(y=rows_y.x, y_step=rows_y.x_step, u=rows_u.x, u_step=rows_u.x_step, sigma=_lib.ptr(sg),
                          log_sigma=_lib.ptr(ls), mask=rows_y.mask, mask_step=rows_y.mask_step, n_steps=T, N=N, n_sets=G,
                          act_dim=Cc)
    return rows, T, N, G, Cc, flat, (y3, u3, m3, sg, ls)


def log_prob_rows(mean, raw_action, sigma, log_sigma, mask=None):
    """wg_ppo_surrogate's density mode: the Gaussian log-density of raw_action around mean, summed over the action
    units in ascending order: float32 [T, N] (or [R]); zero on the rows mask skips.  sigma and log_sigma are [C] or
    [G, C] device tensors; the kernel computes neither from the other.  No gradient."""
    import torch
    rows, T, N, G, Cc, flat, keep = _ppo_rows(mean, raw_action, sigma, log_sigma, mask, "log_prob_rows")
    dv = mean.device
    logp = (torch.empty if mask is None else torch.zeros)((T, N), dtype=torch.float32, device=dv)
    _lib.check(_lib.load().wg_ppo_surrogate(rows, None, None, N, None, None, None, 0.0, 1, None, _lib.ptr(logp), None, 0,
                                            None, None, None, torch.cuda.current_stream(dv).cuda_stream),
               "wg_ppo_surrogate")
    return logp[0] if flat else logp


def ppo_surrogate_rows(mean, raw_action, sigma, log_sigma, old_logp, adv, scale, mask=None, clip: float = 0.2, value=None,
                       ret=None, chunk_rows: Optional[int] = None, want=("logp", "dy", "dvalue", "g_log_sigma", "stats"),
                       dy_out=None):
    """wg_ppo_surrogate's loss mode called directly (no autograd): a dict of the outputs named in `want` ('dvalue' only
    with value).  scale: float32 [2] device tensor.  old_logp / adv / value / ret: contiguous float32 [T, N] (or [R]).
    dy_out: where dy is written (float32 [T, N, C], only its step dimension strided; skipped rows are left as they
    were); otherwise the skipped rows of dy, dvalue and logp are zero."""
    import torch
    who = "ppo_surrogate"
    rows, T, N, G, Cc, flat, keep = _ppo_rows(mean, raw_action, sigma, log_sigma, mask, who)
    dv = mean.device
    per_row = lambda t, name: None if t is None else _vec(t, who, name, dv, T * N)
    old_logp, adv = per_row(old_logp, "old_logp"), per_row(adv, "adv")
    value, ret = per_row(value, "value"), per_row(ret, "ret")
    if old_logp is None or adv is None:
        raise ValueError(f"{who}: old_logp and adv are required")
    scale = _vec(scale, who, "scale", dv, 2)
    chunk = default_chunk_rows(T, N // G) if chunk_rows is None else int(chunk_rows)
    L = _lib.load()
    count = _lib.check(L.wg_ppo_surrogate_workspace(rows, chunk), "wg_ppo_surrogate_workspace")
    ws = torch.empty(int(count), dtype=torch.float64, device=dv)
    new = torch.empty if mask is None else torch.zeros
    out = {}
    if "logp" in want:
        out["logp"] = new((T, N), dtype=torch.float32, device=dv)
    dy3 = None
    if dy_out is not None:
        dy3 = dy_out[None] if dy_out.dim() == 2 else dy_out
        if (dy3.dtype != torch.float32 or dy3.device != dv or tuple(dy3.shape) != (T, N, Cc) or dy3.stride(2) != 1
                or dy3.stride(1) != Cc):
            raise ValueError(f"{who}: dy_out must be float32 {(T, N, Cc)} with only its step dimension strided")
    elif "dy" in want:
        dy3 = new((T, N, Cc), dtype=torch.float32, device=dv)
    if dy3 is not None:
        out["dy"] = dy3
    if "dvalue" in want and value is not None:
        out["dvalue"] = new((T, N), dtype=torch.float32, device=dv)
    if "g_log_sigma" in want:
        out["g_log_sigma"] = torch.empty((G, Cc), dtype=torch.float32, device=dv)
    if "stats" in want:
        out["stats"] = torch.empty(5, dtype=torch.float64, device=dv)
    p = _lib.ptr
    _lib.check(L.wg_ppo_surrogate(rows, p(old_logp), p(adv), N, p(value), p(ret), p(scale), float(clip), chunk, p(ws),
                                  p(out.get("logp")), p(dy3), (dy3.stride(0) if T > 1 else N * Cc) if dy3 is not None else 0,
                                  p(out.get("dvalue")), p(out.get("g_log_sigma")), p(out.get("stats")),
                                  torch.cuda.current_stream(dv).cuda_stream), "wg_ppo_surrogate")
    if flat:
        for k in ("logp", "dy", "dvalue"):
            if k in out and (k != "dy" or dy_out is None):
                out[k] = out[k][0]
    return out


_PPO_FN = None


def _ppo_function():
    global _PPO_FN
    if _PPO_FN is not None:
        return _PPO_FN
    import torch

    class PpoSurrogate(torch.autograd.Function):
        @staticmethod
        def forward(ctx, mean, log_sigma, value, raw_action, old_logp, adv, mask, clip, scale, ret, chunk_rows):
            sigma = log_sigma.detach().exp()
            o = ppo_surrogate_rows(mean.detach(), raw_action, sigma, log_sigma.detach(), old_logp, adv, scale, mask, clip,
                                   None if value is None else value.detach().contiguous(), ret, chunk_rows)
            stats = o["stats"]
            loss = (scale[0].double() * stats[1] + 0.5 * scale[1].double() * stats[4]).to(torch.float32)
            ctx.shapes = (mean.shape, log_sigma.shape, None if value is None else value.shape)
            ctx.save_for_backward(o["dy"], o["g_log_sigma"], o.get("dvalue"))
            ctx.mark_non_differentiable(stats, o["logp"])
            return loss, stats, o["logp"]

        @staticmethod
        def backward(ctx, g_loss, g_stats, g_logp):
            dy, g_ls, dvalue = ctx.saved_tensors
            need, (s_mean, s_ls, s_value) = ctx.needs_input_grad, ctx.shapes
            g_mean = (dy * g_loss).reshape(s_mean) if need[0] else None
            g_lsig = (g_ls * g_loss).reshape(s_ls) if need[1] else None
            g_val = (dvalue * g_loss).reshape(s_value) if (need[2] and dvalue is not None) else None
            return (g_mean, g_lsig, g_val) + (None,) * 8

    _PPO_FN = PpoSurrogate
    return PpoSurrogate


def ppo_surrogate(mean, raw_action, log_sigma, old_logp, adv, mask=None, clip: float = 0.2, scale=None, value=None,
                  ret=None, value_scale=None, chunk_rows: Optional[int] = None):
    """The clipped PPO surrogate of a minibatch in one kernel call (wg_ppo_surrogate), differentiable with respect to
    mean (pg.policy_rows' output), log_sigma and value: (loss, info).

    mean, raw_action: float32 [T, N, C] (or [R, C]) device tensors, only the step dimension strided; log_sigma [C] or
    [G, C] (sigma is log_sigma.detach().exp(), what the rollout was given); old_logp (log_prob_rows before the update),
    adv, and the optional pair value / ret: contiguous [T, N]; mask as in policy_rows (a minibatch is a row mask).
    loss = scale * sum(min(r A, clip(r) A)) + 0.5 * value_scale * sum((value - ret)^2) over the unskipped rows, a
    float32 scalar formed on the device from the kernel's float64 sums; scale defaults to -1 / max(count(mask), 1) and
    value_scale to 1 / max(count(mask), 1), both computed on the device (numbers or 0-d tensors are accepted).  info:
    'stats' (float64 [5]: PPO_STATS), 'logp' [T, N], 'approx_kl' = -stats[2] / stats[0], 'clip_fraction' =
    stats[3] / stats[0], 'value_loss' = stats[4] / stats[0], all device tensors.  The backward returns the gradients
    the forward's kernel call wrote, times the upstream scalar (an upstream of 1 leaves the kernel's bits)."""
    import torch
    dv = mean.device
    T_N = mean.shape[:-1].numel()
    cnt = None
    if scale is None or (value is not None and value_scale is None):
        cnt = (mask.sum() if mask is not None else torch.tensor(T_N, device=dv)).clamp(min=1).to(torch.float32)
    as_dev = lambda v: v.to(device=dv, dtype=torch.float32).reshape(()) if isinstance(v, torch.Tensor) else \
        torch.tensor(float(v), dtype=torch.float32, device=dv)
    s0 = -1.0 / cnt if scale is None else as_dev(scale)
    s1 = torch.zeros((), dtype=torch.float32, device=dv) if value is None else \
        (1.0 / cnt if value_scale is None else as_dev(value_scale))
    sc = torch.stack([s0, s1]).detach().contiguous()
    loss, stats, logp = _ppo_function().apply(mean, log_sigma, value, raw_action, old_logp, adv, mask, float(clip), sc,
                                              ret, chunk_rows)
    rows = stats[0].clamp(min=1.0)
    info = {"stats": stats, "logp": logp, "approx_kl": -stats[2] / rows, "clip_fraction": stats[3] / rows,
            "value_loss": stats[4] / rows}
    return loss, info


# ---------------------------------------------------------------------------------------------------- advantages
def normalize_advantages_numpy(adv, mask=None, eps: float = 1e-8, chunk_rows: Optional[int] = None):
    """normalize_advantages on the host: the moments of adv [T, N] (or [R]) over the rows that are unmasked and finite
    (normalize.obs_moments_numpy with one column and bound = +inf), then float32 (adv - mean) * scale, zero where the
    mask is."""
    from .normalize import obs_moments_numpy, obs_norm_finish_numpy
    a = np.ascontiguousarray(adv, dtype=np.float32)
    a2 = a[None] if a.ndim == 1 else a
    T, N = a2.shape
    chunk = default_chunk_rows(T, N) if chunk_rows is None else int(chunk_rows)
    st = obs_moments_numpy(a2.reshape(T, N, 1), None if mask is None else np.asarray(mask).reshape(T, N), math.inf, chunk)
    fin = obs_norm_finish_numpy(st, eps)
    mean, scale = (np.float32(0.0), np.float32(1.0)) if fin is None else (fin[0][0], fin[1][0])
    with np.errstate(all="ignore"):
        out = ((a - mean).astype(np.float32) * scale).astype(np.float32)
    if mask is not None:
        out = np.where(np.asarray(mask).reshape(a.shape) != 0, out, np.float32(0.0)).astype(np.float32)
    return out


def normalize_advantages(adv, mask=None, eps: float = 1e-8, chunk_rows: Optional[int] = None):
    """(adv - mean) * scale over the unmasked rows of adv, float32 [T, N] (or [R]) on the device, zero where mask is.
    mean and scale = 1 / sqrt(var + eps) come from one wg_obs_moments call on adv viewed as [T, N, 1] with bound = +inf:
    its ordered float64 sums over the rows that are unmasked and finite (a NaN or inf advantage never enters them).
    There is no gather of the unmasked rows and nothing waits for the device; with no usable row mean = 0, scale = 1.
    normalize_advantages_numpy restates it."""
    import torch
    who = "normalize_advantages"
    if not isinstance(adv, torch.Tensor) or adv.dim() not in (1, 2) or adv.dtype != torch.float32 or not adv.is_cuda:
        raise ValueError(f"{who}: adv must be a float32 device tensor [T, N] or [R]")
    dv = adv.device
    rows, T, N, a3, m3, _ = _rows_of(1, dv, adv.unsqueeze(-1), mask, who)
    chunk = default_chunk_rows(T, N) if chunk_rows is None else int(chunk_rows)
    L = _lib.load()
    count = _lib.check(L.wg_obs_moments_workspace(rows, 1, chunk), "wg_obs_moments_workspace")
    ws = torch.empty(int(count), dtype=torch.float64, device=dv)
    state = torch.zeros(3, dtype=torch.float64, device=dv)
    mean = torch.zeros(1, dtype=torch.float32, device=dv)
    scale = torch.ones(1, dtype=torch.float32, device=dv)
    p = _lib.ptr
    _lib.check(L.wg_obs_moments(rows, 1, math.inf, chunk, p(ws), p(state), float(eps), p(mean), p(scale),
                                torch.cuda.current_stream(dv).cuda_stream), "wg_obs_moments")
    out = torch.mul(torch.sub(adv, mean), scale)
    if mask is not None:
        out = torch.where(mask.reshape(adv.shape) != 0, out, torch.zeros((), dtype=torch.float32, device=dv))
    return out

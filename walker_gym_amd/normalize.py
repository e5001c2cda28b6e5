"""Observation normalisation as part of the policy's arithmetic (wg_obs_norm in include/walker_hip.h), the moments it
is made from (wg_obs_moments), and their numpy restatements, which agree with the kernels bit for bit.

Normalised input, float32, every operation rounded by itself:
  v = RN32(RN32(x[i] - mean[i]) * scale[i]);   xn[i] = (v < -clip) ? -clip : ((v > clip) ? clip : v)    (a NaN passes)
An MLPPolicy built with obs_norm=ObsNorm(...) runs its layers on xn in every evaluator: the rollout kernels
(wg_rollout_normalized), the row kernels (wg_policy_forward_normalized / _backward_normalized), forward_numpy and the
torch restatement (sub, mul, clamp).  The rows a rollout stores stay raw.  With mean = 0, scale = 1 and clip = inf the
policy is the plain one, bit for bit, on finite rows.

Moments.  Rows [T, N, D] are numbered rho = t * N + w and cut into chunks of chunk_rows.  A row is used iff its mask is
non-zero and |x[i]| < bound for every i (a NaN or inf never enters).  Per chunk k over its used rows in ascending rho,
float64 from +0.0:  c_k += 1;  P1_k[i] += x[i];  P2_k[i] += x[i] * x[i]  (the product is exact).  The running state is
float64 [1 + 2 D] = n, S1, S2; for k ascending: n += c_k, S1 += P1_k, S2 += P2_k.  Then, with n > 0:
  m = S1 / n;  var = max(S2 / n - m * m, 0);  mean = RN32(m);  scale = RN32(1 / sqrt(var + eps))
every float64 operation rounded by itself.  The sums add, so a second update continues the first, and ranks would merge
by exchanging state.
"""
from __future__ import annotations

import math
from typing import Optional

import numpy as np

from . import _lib


# ---------------------------------------------------------------------------------------------------- host restatements
def normalize_numpy(x, mean, scale, clip: float):
    """xn of the rows x [.., D] under mean / scale [D] and clip: float32, the contract's three operations."""
    x = np.asarray(x, dtype=np.float32)
    mean, scale = np.asarray(mean, dtype=np.float32), np.asarray(scale, dtype=np.float32)
    c = np.float32(clip)
    with np.errstate(all="ignore"):
        v = ((x - mean).astype(np.float32) * scale).astype(np.float32)
        return np.where(v < -c, -c, np.where(v > c, c, v)).astype(np.float32)


def obs_moments_numpy(x, mask=None, bound: float = math.inf, chunk_rows: int = 256, state=None):
    """wg_obs_moments' sums on the host: x [T, N, D] (or [R, D]), mask [T, N] (or [R]) or None.  Returns the new state,
    float64 [1 + 2 D] = n, S1, S2, continuing `state` (None: zeros)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    D = x.shape[-1]
    x = x.reshape(-1, D)
    R = x.shape[0]
    chunk_rows = int(chunk_rows)
    if chunk_rows < 1:
        raise ValueError("chunk_rows < 1")
    on = np.ones(R, bool) if mask is None else np.asarray(mask).reshape(R) != 0
    with np.errstate(all="ignore"):
        used = on & (np.abs(x) < np.float32(bound)).all(axis=1)
    st = np.zeros(1 + 2 * D, np.float64) if state is None else np.array(state, dtype=np.float64).reshape(1 + 2 * D)
    n, S1, S2 = st[0], st[1:1 + D].copy(), st[1 + D:].copy()
    zero = np.zeros((1, D), np.float64)
    for lo in range(0, R, chunk_rows):
        v = x[lo:lo + chunk_rows][used[lo:lo + chunk_rows]].astype(np.float64)
        # ufunc.accumulate along the rows is the sequential sum: +0.0, then row after row in ascending rho
        P1 = np.add.accumulate(np.concatenate([zero, v]), axis=0)[-1]
        P2 = np.add.accumulate(np.concatenate([zero, v * v]), axis=0)[-1]      # (exact products, one rounding each)
        n, S1, S2 = n + float(v.shape[0]), S1 + P1, S2 + P2
    return np.concatenate([[n], S1, S2])


def obs_norm_finish_numpy(state, eps: float = 1e-8):
    """(mean, scale), float32 [D] each, of a state; None when n == 0 (the kernel then leaves its outputs alone)."""
    st = np.asarray(state, dtype=np.float64)
    D = (st.shape[0] - 1) // 2
    n, S1, S2 = st[0], st[1:1 + D], st[1 + D:]
    if not n > 0:
        return None
    m = S1 / n
    var = S2 / n - m * m
    var = np.where(var > 0, var, 0.0)
    return m.astype(np.float32), (1.0 / np.sqrt(var + np.float64(eps))).astype(np.float32)


# ---------------------------------------------------------------------------------------------------- the device object
class ObsNorm:
    """Running observation statistics on the device and the normaliser made from them.

    state: float64 [1 + 2 D] (n, S1, S2); mean, scale: float32 [D], updated IN PLACE by update(), so a policy that holds
    this object (MLPPolicy(..., obs_norm=nm)) sees every update with no re-wrap.  Fresh: mean 0, scale 1.  clip > 0
    (inf allowed); bound > 0: rows with an |x[i]| >= bound (or a NaN) are left out of the statistics."""

    def __init__(self, obs_dim: int, device, clip: float = 10.0, eps: float = 1e-8, bound: float = math.inf):
        import torch
        D = int(obs_dim)
        if D < 1:
            raise ValueError(f"obs_dim {obs_dim} < 1")
        if not float(clip) > 0.0:
            raise ValueError(f"clip must be > 0 (inf allowed), got {clip!r}")
        if not float(eps) >= 0.0:
            raise ValueError(f"eps must be >= 0, got {eps!r}")
        if not float(bound) > 0.0:
            raise ValueError(f"bound must be > 0 (inf allowed), got {bound!r}")
        self.clip, self.eps, self.bound = float(np.float32(clip)), float(eps), float(np.float32(bound))
        self.state = torch.zeros(1 + 2 * D, dtype=torch.float64, device=device)
        self.mean = torch.zeros(D, dtype=torch.float32, device=device)
        self.scale = torch.ones(D, dtype=torch.float32, device=device)
        self.D, self.device = D, self.mean.device      # (the tensors' own device: "cuda" has become "cuda:0")

    @property
    def count(self) -> float:
        """The rows summed so far (reads the device)."""
        return float(self.state[0].item())

    def struct(self) -> _lib.WgObsNorm:
        return _lib.WgObsNorm(mean=_lib.ptr(self.mean), scale=_lib.ptr(self.scale), clip=self.clip)

    def to(self, device) -> "ObsNorm":
        other = ObsNorm(self.D, device, self.clip, self.eps, self.bound)
        other.load_state_dict(self.state_dict())
        return other

    def update(self, obs, mask=None, chunk_rows: Optional[int] = None) -> "ObsNorm":
        """One wg_obs_moments call (two launches on the current stream): the rows of obs [T, N, D] (or [R, D]; float32
        on this device, only the step dimension strided) added to state, mean and scale rewritten in place.  mask: uint8
        or bool [T, N] (or [R]), 0 = left out.  chunk_rows: pg.default_chunk_rows' rule by default."""
        import torch
        from . import pg
        rows, T, N, o3, m3, _ = pg._rows_of(self.D, self.device, obs, mask, "ObsNorm.update")
        chunk = pg.default_chunk_rows(T, N) if chunk_rows is None else int(chunk_rows)
        L = _lib.load()
        count = L.wg_obs_moments_workspace(rows, self.D, chunk)
        _lib.check(count, "wg_obs_moments_workspace")
        ws = torch.empty(int(count), dtype=torch.float64, device=self.device)
        p = _lib.ptr
        _lib.check(L.wg_obs_moments(rows, self.D, self.bound, chunk, p(ws), p(self.state), self.eps, p(self.mean),
                                    p(self.scale), torch.cuda.current_stream(self.device).cuda_stream),
                   "wg_obs_moments")
        return self

    def state_dict(self) -> dict:
        return {"state": self.state.detach().cpu().clone(), "mean": self.mean.detach().cpu().clone(),
                "scale": self.scale.detach().cpu().clone(), "clip": self.clip, "eps": self.eps, "bound": self.bound}

    def load_state_dict(self, sd: dict) -> None:
        import torch
        for name in ("state", "mean", "scale"):
            t = torch.as_tensor(sd[name])
            if tuple(t.shape) != tuple(getattr(self, name).shape):
                raise ValueError(f"ObsNorm.load_state_dict: {name} has shape {tuple(t.shape)}")
            getattr(self, name).copy_(t)
        self.clip, self.eps = float(np.float32(sd["clip"])), float(sd["eps"])
        self.bound = float(np.float32(sd["bound"]))

    # ------------------------------------------------------------------ the restatements on this object's tensors
    def normalize_numpy(self, x):
        return normalize_numpy(x, self.mean.detach().cpu().numpy(), self.scale.detach().cpu().numpy(), self.clip)

    def normalize_torch(self, rows):
        """xn of device rows [n, D]: sub, mul, clamp (a NaN passes through torch.clamp)."""
        import torch
        v = torch.mul(torch.sub(rows, self.mean), self.scale)
        return torch.clamp(v, min=-self.clip, max=self.clip)

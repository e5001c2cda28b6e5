"""The device optimiser: a global-norm gradient clip and Adam / AdamW in pinned arithmetic (wg_adam_step in
include/walker_hip.h), its numpy restatement, and the Adam class over float32 device tensors.

Elements are numbered e = 0 .. E-1 across the tensors in list order; with maximize every gradient's sign is flipped first.

Norm.  Chunks of L = 4096 elements; within a chunk 256 float64 chains (lane j takes e = kL + j, kL + j + 256, ...) of
exact squares, a fixed tree q = q[:h] + q[h:] for h = 128 .. 1, the chunk sums added in order, one float64 sqrt.  A sum
that is not finite skips the step: nothing is written but state[3] = norm, state[4] = 0, state[5] += 1.

Scalars (float64; state = [t, b1p, b2p, norm, cf, skipped, -, -], zeroed = a fresh optimiser).  b1p and b2p are the
running products beta^t (no pow): b1p' = b1p * beta1, c1 = 1 - b1p', a = RN32(lr / c1); c2 = 1 - b2p', r2 = RN32(sqrt(c2));
cf = RN32(min(max_norm / (norm + 1e-6), 1)).

Element update (float32, every operation rounded by itself):
  gc = g * cf;  m' = beta1 * m + (1 - beta1) * gc;  v' = beta2 * v + (1 - beta2) * (gc * gc)
  den = sqrt(v') / r2 + eps;  upd = a * (m' / den);  p1 = p - (lr * weight_decay) * p (only with weight_decay);  p' = p1 - upd
adam_step_numpy is that, operation by operation, and the kernels agree with it bit for bit (tests/test_gpu_optim.py).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional

import numpy as np

from . import _lib

CHUNK = 4096      # the contract's L
LANES = 256       # chains per chunk
MAX_SEGMENTS = 32   # WG_OPT_MAX_SEGMENTS
STATE_LEN = 8


def adam_config(lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_norm=math.inf, maximize=False) -> dict:
    """The fields of wg_adam as a dict (what adam_step_numpy and the direct call take)."""
    return dict(lr=float(lr), beta1=float(betas[0]), beta2=float(betas[1]), eps=float(eps),
                weight_decay=float(weight_decay), max_norm=float(max_norm), maximize=int(bool(maximize)))


def grad_sq_sum_numpy(grads) -> np.float64:
    """S of the contract: the ordered float64 sum of the squared gradients over the concatenated elements."""
    g = np.concatenate([np.asarray(x, dtype=np.float32).reshape(-1) for x in grads]).astype(np.float64)
    S = np.float64(0.0)
    with np.errstate(all="ignore"):
        for lo in range(0, g.size, CHUNK):
            c = g[lo:lo + CHUNK]
            sq = np.zeros(((c.size + LANES - 1) // LANES) * LANES, dtype=np.float64)
            sq[:c.size] = c * c                       # exact: float32 squares in float64
            q = np.zeros(LANES, dtype=np.float64)
            for row in sq.reshape(-1, LANES):         # lane j: its elements ascending (a padded +0.0 changes nothing)
                q = q + row
            h = LANES // 2
            while h >= 1:
                q = q[:h] + q[h:]
                h //= 2
            S = S + q[0]
    return S


def adam_step_numpy(params, grads, ms, vs, state, cfg) -> dict:
    """wg_adam_step on the host: params / ms / vs (lists of float32 arrays) and state (float64 [8]) are updated in
    place, grads only read.  cfg: adam_config()'s dict.  Returns {'norm', 'cf', 'skipped'} of this step."""
    f32, f64 = np.float32, np.float64
    lr, b1, b2, eps = f32(cfg["lr"]), f32(cfg["beta1"]), f32(cfg["beta2"]), f32(cfg["eps"])
    wd, max_norm = f32(cfg["weight_decay"]), f32(cfg["max_norm"])
    with np.errstate(all="ignore"):
        S = grad_sq_sum_numpy(grads)
        norm = np.sqrt(S)
        state[3] = norm
        if not np.isfinite(S):
            state[4] = 0.0
            state[5] = state[5] + f64(1.0)
            return {"norm": norm, "cf": f32(0.0), "skipped": True}
        t = f64(state[0])
        b1p = (f64(1.0) if t == 0 else f64(state[1])) * f64(b1)
        b2p = (f64(1.0) if t == 0 else f64(state[2])) * f64(b2)
        c1, c2 = f64(1.0) - b1p, f64(1.0) - b2p
        a = f32(f64(lr) / c1)
        r2 = f32(np.sqrt(c2))
        c = f64(max_norm) / (norm + f64(1e-6))
        cf = f32(c if c < 1.0 else f64(1.0))
        state[0], state[1], state[2], state[4] = t + f64(1.0), b1p, b2p, f64(cf)
        omb1, omb2 = f32(1.0) - b1, f32(1.0) - b2
        lrwd = lr * wd
        for p, g, m, v in zip(params, grads, ms, vs):
            g = np.asarray(g, dtype=f32)
            assert p.dtype == f32 and m.dtype == f32 and v.dtype == f32
            gs = -g if cfg["maximize"] else g
            gc = gs * cf
            m1 = b1 * m + omb1 * gc
            v1 = b2 * v + omb2 * (gc * gc)
            den = np.sqrt(v1) / r2 + eps
            upd = a * (m1 / den)
            p1 = p - lrwd * p if wd != 0 else p
            p[...] = p1 - upd
            m[...] = m1
            v[...] = v1
    return {"norm": norm, "cf": cf, "skipped": False}


def _struct_cfg(cfg: dict) -> _lib.WgAdam:
    return _lib.WgAdam(lr=cfg["lr"], beta1=cfg["beta1"], beta2=cfg["beta2"], eps=cfg["eps"],
                       weight_decay=cfg["weight_decay"], max_norm=cfg["max_norm"], maximize=cfg["maximize"])


def adam_step(params, grads, ms, vs, state, cfg: dict, workspace=None):
    """One wg_adam_step call over lists of float32 contiguous device tensors (the direct call: no .grad, nothing owned).
    state: float64 [8] device tensor; workspace: float64 device tensor of wg_adam_workspace elements (made if None)."""
    import torch
    n = len(params)
    if not (len(grads) == len(ms) == len(vs) == n):
        raise ValueError("adam_step: params, grads, ms and vs must have one length")
    if n < 1 or n > MAX_SEGMENTS:
        raise ValueError(f"adam_step: {n} tensors (1..{MAX_SEGMENTS} per call)")
    dv = params[0].device
    table = (_lib.WgOptSegment * n)()
    for i, (p, g, m, v) in enumerate(zip(params, grads, ms, vs)):
        for name, t in (("param", p), ("grad", g), ("m", m), ("v", v)):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or t.device != dv or not t.is_cuda:
                raise ValueError(f"adam_step: {name} {i} must be a float32 tensor on {dv}")
            if not t.is_contiguous():
                raise ValueError(f"adam_step: {name} {i} is not contiguous")
            if t.numel() != p.numel():
                raise ValueError(f"adam_step: {name} {i} has {t.numel()} elements, its parameter {p.numel()}")
        table[i] = _lib.WgOptSegment(param=p.data_ptr(), grad=g.data_ptr(), m=m.data_ptr(), v=v.data_ptr(), n=p.numel())
    L = _lib.load()
    count = _lib.check(L.wg_adam_workspace(table, n), "wg_adam_workspace")
    if workspace is None:
        workspace = torch.empty(int(count), dtype=torch.float64, device=dv)
    elif workspace.dtype != torch.float64 or workspace.device != dv or workspace.numel() < count:
        raise ValueError(f"adam_step: workspace must be float64 [{count}] on {dv}")
    if state.dtype != torch.float64 or state.device != dv or state.numel() != STATE_LEN or not state.is_contiguous():
        raise ValueError(f"adam_step: state must be a contiguous float64 [{STATE_LEN}] tensor on {dv}")
    _lib.check(L.wg_adam_step(table, n, C.byref(_struct_cfg(cfg)), _lib.ptr(workspace), _lib.ptr(state),
                              torch.cuda.current_stream(dv).cuda_stream), "wg_adam_step")
    return workspace


class Adam:
    """Adam / AdamW with a global-norm clip over float32 contiguous device tensors, one wg_adam_step call per step().

    m, v, state and workspace are device tensors the object owns.  step(lr=None) takes the tensors' .grad; a tensor
    whose .grad is None is left out of that step (as torch does).  grad_norm, clip_coef, steps and skipped are views of
    the device state: reading them synchronises, holding them does not.  weight_decay is decoupled (AdamW)."""

    def __init__(self, params, lr=3e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, max_norm=math.inf,
                 maximize=False):
        import torch
        self.params = list(params)
        if not self.params:
            raise ValueError("Adam: no parameters")
        if len(self.params) > MAX_SEGMENTS:
            raise ValueError(f"Adam: {len(self.params)} tensors (at most {MAX_SEGMENTS} per optimiser)")
        dv = self.params[0].device
        for i, p in enumerate(self.params):
            if not isinstance(p, torch.Tensor) or p.dtype != torch.float32:
                raise ValueError(f"Adam: parameter {i} must be a float32 tensor")
            if not p.is_cuda or p.device != dv:
                raise ValueError(f"Adam: parameter {i} must be on the device {dv}")
            if not p.is_contiguous():
                raise ValueError(f"Adam: parameter {i} is not contiguous")
        self.cfg = adam_config(lr, betas, eps, weight_decay, max_norm, maximize)
        self.device = dv
        self.m = [torch.zeros_like(p, memory_format=torch.contiguous_format).detach() for p in self.params]
        self.v = [torch.zeros_like(p, memory_format=torch.contiguous_format).detach() for p in self.params]
        self.state = torch.zeros(STATE_LEN, dtype=torch.float64, device=dv)
        total = sum(p.numel() for p in self.params)
        self.workspace = torch.empty((total + CHUNK - 1) // CHUNK, dtype=torch.float64, device=dv)

    @property
    def lr(self) -> float:
        return self.cfg["lr"]

    @lr.setter
    def lr(self, value: float) -> None:
        self.cfg["lr"] = float(value)

    def step(self, lr: Optional[float] = None) -> None:
        cfg = self.cfg if lr is None else dict(self.cfg, lr=float(lr))
        ps, gs, ms, vs = [], [], [], []
        for p, m, v in zip(self.params, self.m, self.v):
            if p.grad is None:
                continue
            g = p.grad
            if g.dtype != p.dtype or not g.is_contiguous():
                raise ValueError("Adam.step: a .grad is not a contiguous float32 tensor")
            ps.append(p.detach())
            gs.append(g)
            ms.append(m)
            vs.append(v)
        if ps:
            adam_step(ps, gs, ms, vs, self.state, cfg, self.workspace)

    def zero_grad(self, set_to_none: bool = True) -> None:
        for p in self.params:
            if p.grad is None:
                continue
            if set_to_none:
                p.grad = None
            else:
                p.grad.detach_()
                p.grad.zero_()

    # device views of state: no synchronisation until a caller reads them
    @property
    def steps(self):
        return self.state[0]

    @property
    def grad_norm(self):
        return self.state[3]

    @property
    def clip_coef(self):
        return self.state[4]

    @property
    def skipped(self):
        return self.state[5]

    def state_dict(self) -> dict:
        return {"cfg": dict(self.cfg), "state": self.state.clone(), "m": [t.clone() for t in self.m],
                "v": [t.clone() for t in self.v]}

    def load_state_dict(self, sd: dict) -> None:
        if len(sd["m"]) != len(self.m) or len(sd["v"]) != len(self.v):
            raise ValueError("Adam.load_state_dict: another number of tensors")
        for mine, theirs in zip(self.m + self.v, list(sd["m"]) + list(sd["v"])):
            if mine.shape != theirs.shape:
                raise ValueError("Adam.load_state_dict: a moment of another shape")
        self.cfg = dict(sd["cfg"])
        self.state.copy_(sd["state"])
        for mine, theirs in zip(self.m + self.v, list(sd["m"]) + list(sd["v"])):
            mine.copy_(theirs)

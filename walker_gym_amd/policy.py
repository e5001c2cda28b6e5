"""MLPPolicy — the stateless piecewise-linear policy that BatchedPhysicsEnv.rollout_policy evaluates inside the
resident kernel (wg_policy in include/walker_hip.h), with two slow, exact restatements of it: forward_numpy (host) and
__call__ (torch elementwise ops on the device, for policy_loop / step loops on any batch, ragged ones included).

The arithmetic is the contract, float32 with separately rounded multiply and add, so that all three agree bit for bit:
  unit:    acc = bias; for i ascending: acc = RN32(acc + RN32(x[i] * w[i][j]))      (a missing bias is +0.0)
  hidden:  h = (z > 0) ? z : +0.0                       (a NaN becomes 0)
  output:  a = (y < -L) ? -L : ((y > L) ? L : y)        (L = act_limit > 0, inf allowed; a NaN passes through)
Weights are input-major (y = x @ w): w1 [G, D, H], b1 [G, H] (only with a hidden layer), w2 [G, H or D, C], b2 [G, C].
A deep policy has a second hidden layer between the two (wg_policy_mid): wm [G, H, H2], bm [G, H2], and w2 [G, H2, C];
its units and its ReLU are the ones above.
With obs_norm (a walker_gym_amd.normalize.ObsNorm, wg_obs_norm in the header) the layers run on the normalised row
  input:   v = RN32(RN32(x[i] - mean[i]) * scale[i]);  xn[i] = (v < -clip) ? -clip : ((v > clip) ? clip : v)
in all three and in the kernels; mean / scale [D] are shared by every parameter set and read at every call.
G parameter sets: of N walkers, walker w uses set w // (N // G) (G = 1 shared, G = N one candidate per walker).
With G > 1 the torch restatement must know which walkers its rows are: for_rows(first_walker, N) / for_row_index(rows,
N) bind it (BatchedPhysicsEnv.policy_loop does so for each of its walker ranges); unbound, __call__ raises, it never
guesses.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _lib


def _as_tensor(t, name: str):
    if isinstance(t, np.ndarray):
        if t.dtype != np.float32:
            raise ValueError(f"{name} has dtype {t.dtype}, expected float32")
        t = torch.from_numpy(np.ascontiguousarray(t))
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a float32 torch tensor (or numpy array)")
    if t.dtype != torch.float32:
        raise ValueError(f"{name} has dtype {t.dtype}, expected torch.float32")
    return t


class _BoundPolicy:
    """An MLPPolicy for the rows of known walkers of a batch of n_total (MLPPolicy.for_rows / for_row_index): rows
    w0, w0 + 1, ... or the walkers a device index tensor names.  Each row's parameter set is computed on the device
    (capturable in a HIP graph) and cached per row count."""

    def __init__(self, policy: "MLPPolicy", w0: int, n_total: int, index=None, n_rows=None):
        n_total = int(n_total)
        if policy.G > 1 and (n_total < 1 or n_total % policy.G != 0):
            raise ValueError(f"{n_total} walkers do not divide into {policy.G} parameter sets")
        self.policy, self.w0, self.n_total, self.index = policy, int(w0), n_total, index
        self._sets = {}
        # (known row counts now: a first call inside a graph capture then allocates nothing that outlives the capture)
        if index is not None:
            self._set_index(int(index.numel()), policy.device)
        elif n_rows is not None:
            self._set_index(int(n_rows), policy.device)

    def _set_index(self, n: int, device):
        pol = self.policy
        if pol.G == 1:
            return None
        if n not in self._sets:
            if self.index is not None:
                if self.index.numel() != n:
                    raise ValueError(f"{n} rows for an index of {self.index.numel()} walkers")
                w = self.index.to(device=device, dtype=torch.int64)
            else:
                if self.w0 < 0 or self.w0 + n > self.n_total:
                    raise ValueError(f"rows {self.w0} .. {self.w0 + n} outside 0 .. {self.n_total}")
                w = torch.arange(n, device=device, dtype=torch.int64) + self.w0
            self._sets[n] = torch.div(w, self.n_total // pol.G, rounding_mode="floor")
        return self._sets[n]

    def __call__(self, rows, t=0):
        return self.policy._forward_torch(rows, self._set_index(rows.shape[0], rows.device))


class MLPPolicy:
    """The policy of the module's docstring over w2 [G, H or D, C], b2 [G, C], w1 [G, D, H], b1 [G, H], and with a
    second hidden layer wm [G, H, H2], bm [G, H2] (w2 is then [G, H2, C]; .H2 is 0 without one).

    A tensor that is already contiguous and of full rank ([G, ..]) is kept by identity: an nn.Parameter (or any leaf
    that requires grad) handed in stays that object in .w1 / .b1 / .w2 / .b2.  walker_gym_amd.pg.policy_rows
    differentiates with respect to exactly those, so an optimizer over the same parameters updates the policy the
    rollout kernel reads, with no copy in between."""

    def __init__(self, w2, b2=None, w1=None, b1=None, act_limit: float = 1.0, obs_norm=None, wm=None, bm=None):
        w2 = _as_tensor(w2, "w2")
        if w2.dim() == 2:
            w2 = w2[None]
        if w2.dim() != 3 or min(w2.shape) < 1:
            raise ValueError(f"w2 must be [G, H or D, C] (or 2-D for G = 1), got {tuple(w2.shape)}")
        G, n2, Cc = w2.shape
        if w1 is None and b1 is not None:
            raise ValueError("b1 without w1")
        if wm is None and bm is not None:
            raise ValueError("bm without wm")
        if wm is not None and w1 is None:
            raise ValueError("wm without w1 (a middle layer needs a first hidden layer)")

        def bias(b, name, width):
            if b is None:
                return None
            b = _as_tensor(b, name)
            if b.dim() == 1:
                b = b[None]
            if tuple(b.shape) != (G, width):
                raise ValueError(f"{name} has shape {tuple(b.shape)}, expected {(G, width)}")
            return b

        if w1 is not None:
            w1 = _as_tensor(w1, "w1")
            if w1.dim() == 2:
                w1 = w1[None]
            if w1.dim() != 3 or min(w1.shape) < 1:
                raise ValueError(f"w1 must be [G, D, H] (or 2-D for G = 1), got {tuple(w1.shape)}")
            if w1.shape[0] != G:
                raise ValueError(f"w1 has {w1.shape[0]} parameter sets, w2 has {G}")
            if wm is None and w1.shape[2] != n2:
                raise ValueError(f"w1 has {w1.shape[2]} hidden units, w2 takes {n2} inputs")
        if wm is not None:
            wm = _as_tensor(wm, "wm")
            if wm.dim() == 2:
                wm = wm[None]
            if wm.dim() != 3 or min(wm.shape) < 1:
                raise ValueError(f"wm must be [G, H, H2] (or 2-D for G = 1), got {tuple(wm.shape)}")
            if wm.shape[0] != G:
                raise ValueError(f"wm has {wm.shape[0]} parameter sets, w2 has {G}")
            if wm.shape[1] != w1.shape[2]:
                raise ValueError(f"w1 has {w1.shape[2]} hidden units, wm takes {wm.shape[1]} inputs")
            if wm.shape[2] != n2:
                raise ValueError(f"wm has {wm.shape[2]} hidden units, w2 takes {n2} inputs")
            if wm.shape[2] > 256:
                raise ValueError(f"wm has {wm.shape[2]} hidden units, at most 256")
        b1 = bias(b1, "b1", n2 if wm is None else int(wm.shape[1]))
        bm = bias(bm, "bm", n2)
        b2 = bias(b2, "b2", Cc)
        dev = w2.device
        for name, t in (("b2", b2), ("w1", w1), ("b1", b1), ("wm", wm), ("bm", bm)):
            if t is not None and t.device != dev:
                raise ValueError(f"{name} is on {t.device}, w2 is on {dev}")
        L = float(act_limit)
        if not L > 0.0:
            raise ValueError(f"act_limit must be > 0 (inf allowed), got {act_limit!r}")
        self.w1 = None if w1 is None else w1.contiguous()
        self.b1 = None if b1 is None else b1.contiguous()
        self.wm = None if wm is None else wm.contiguous()
        self.bm = None if bm is None else bm.contiguous()
        self.w2, self.b2 = w2.contiguous(), None if b2 is None else b2.contiguous()
        self.act_limit = float(np.float32(L))
        self.G, self.C = int(G), int(Cc)
        self.H = 0 if w1 is None else int(w1.shape[2])
        self.H2 = 0 if wm is None else int(n2)    # the second hidden layer's width; 0: none
        self.D = int(n2) if w1 is None else int(w1.shape[1])
        # walker_gym_amd.normalize.ObsNorm, kept by identity: its mean / scale are updated in place.  Every evaluator
        # runs the layers on xn = clip((x - mean) * scale); None: the plain policy
        if obs_norm is not None and (obs_norm.D != self.D or obs_norm.device != dev):
            raise ValueError(f"obs_norm is [{obs_norm.D}] on {obs_norm.device}, the policy takes {self.D} values on {dev}")
        self.obs_norm = obs_norm

    @property
    def device(self):
        return self.w2.device

    def struct(self, n_walkers: int, action_out=None) -> _lib.WgPolicy:
        """wg_policy of this policy over a batch of n_walkers, writing every step's actions to action_out [T, N, C] f32
        if given; return_out / length_out (rollout_policy's per-walker sums) start NULL."""
        p = _lib.ptr
        return _lib.WgPolicy(n_sets=self.G, obs_dim=self.D, hidden=self.H, act_dim=self.C, w1=p(self.w1), b1=p(self.b1),
                             w2=p(self.w2), b2=p(self.b2), act_limit=self.act_limit, action_out=p(action_out),
                             action_out_step=n_walkers * self.C, return_out=None, length_out=None)

    def mid_struct(self) -> "_lib.WgPolicyMid":
        """wg_policy_mid of a deep policy (H2 > 0): what the *_deep entries take beside struct()."""
        return _lib.WgPolicyMid(hidden2=self.H2, wm=_lib.ptr(self.wm), bm=_lib.ptr(self.bm))

    def to(self, device) -> "MLPPolicy":
        mv = lambda t: None if t is None else t.to(device)
        return MLPPolicy(mv(self.w2), mv(self.b2), mv(self.w1), mv(self.b1), self.act_limit,
                         None if self.obs_norm is None else self.obs_norm.to(device), mv(self.wm), mv(self.bm))

    def _sets(self, n: int, first_walker: int, n_total: Optional[int]):
        """The parameter set of each of n rows starting at walker first_walker of n_total (numpy int64), or None for
        a shared policy."""
        if self.G == 1:
            return None
        n_total = n if n_total is None else int(n_total)
        if n_total % self.G != 0:
            raise ValueError(f"{n_total} walkers do not divide into {self.G} parameter sets")
        if first_walker < 0 or first_walker + n > n_total:
            raise ValueError(f"rows {first_walker} .. {first_walker + n} outside 0 .. {n_total}")
        return (np.arange(n, dtype=np.int64) + int(first_walker)) // (n_total // self.G)

    # ------------------------------------------------------------------ host restatement
    def forward_numpy(self, obs_rows, first_walker: int = 0, n_walkers_total: Optional[int] = None) -> np.ndarray:
        """The contract in numpy float32 elementwise operations (a loop over i, vectorised over rows and units):
        obs_rows [n, D] -> actions [n, C], host arrays."""
        x = np.ascontiguousarray(obs_rows, dtype=np.float32)
        if x.ndim != 2 or x.shape[1] != self.D:
            raise ValueError(f"obs_rows must be [n, {self.D}], got {x.shape}")
        sets = self._sets(x.shape[0], first_walker, n_walkers_total)
        host = lambda t: None if t is None else t.detach().cpu().numpy()
        if self.obs_norm is not None:
            x = self.obs_norm.normalize_numpy(x)

        def layer(x, w, b):
            n, J = x.shape[0], w.shape[2]
            if b is None:
                acc = np.zeros((n, J), np.float32)
            else:
                acc = np.broadcast_to(b[0], (n, J)).copy() if sets is None else b[sets].copy()
            for i in range(w.shape[1]):
                wi = w[0, i][None, :] if sets is None else w[sets, i]
                acc = acc + x[:, i:i + 1] * wi          # RN32 of the product, then RN32 of the sum
            return acc

        with np.errstate(all="ignore"):
            if self.H:
                z = layer(x, host(self.w1), host(self.b1))
                x = np.where(z > 0, z, np.float32(0.0)).astype(np.float32)
            if self.H2:
                z = layer(x, host(self.wm), host(self.bm))
                x = np.where(z > 0, z, np.float32(0.0)).astype(np.float32)
            y = layer(x, host(self.w2), host(self.b2))
            L = np.float32(self.act_limit)
            return np.where(y < -L, -L, np.where(y > L, L, y)).astype(np.float32)

    # ------------------------------------------------------------------ device restatement
    def _forward_torch(self, rows, idx):
        """idx: each row's parameter set (int64 device tensor), None for a shared policy."""
        if rows.dim() != 2 or rows.shape[1] != self.D:
            raise ValueError(f"rows must be [n, {self.D}], got {tuple(rows.shape)}")
        if rows.dtype != torch.float32 or rows.device != self.device:
            raise ValueError(f"rows are {rows.dtype} on {rows.device}, the policy is float32 on {self.device}")

        def layer(x, w, b):
            n, J = x.shape[0], w.shape[2]
            ws = w[0] if idx is None else w.index_select(0, idx)      # [I, J] shared / [n, I, J] per row
            if b is None:
                acc = torch.zeros((n, J), dtype=torch.float32, device=x.device)
            else:
                acc = b[0].expand(n, J).clone() if idx is None else b.index_select(0, idx)
            for i in range(w.shape[1]):
                wi = ws[i] if idx is None else ws[:, i]
                acc = torch.add(acc, torch.mul(x[:, i:i + 1], wi))    # two roundings: never addcmul / matmul
            return acc

        x = rows if self.obs_norm is None else self.obs_norm.normalize_torch(rows)
        if self.H:
            z = layer(x, self.w1, self.b1)
            x = torch.where(z > 0, z, torch.zeros_like(z))
        if self.H2:
            z = layer(x, self.wm, self.bm)
            x = torch.where(z > 0, z, torch.zeros_like(z))
        y = layer(x, self.w2, self.b2)
        L = torch.full_like(y, self.act_limit)
        return torch.where(y < -L, -L, torch.where(y > L, L, y)).contiguous()

    def __call__(self, rows, t=0):
        """actions [n, C] of the observation rows [n, D] (device tensors).  A policy with several parameter sets does
        not guess which walkers the rows belong to: bind it with for_rows(w0, N) (ValueError otherwise).
        BatchedPhysicsEnv.policy_loop binds it to each of its walker ranges itself."""
        if self.G > 1:
            raise ValueError(f"an MLPPolicy with {self.G} parameter sets needs the rows' walkers: call "
                             "policy.for_rows(first_walker, n_walkers_total)(rows, t), or hand the policy to "
                             "policy_loop, which binds it to each walker range")
        return self._forward_torch(rows, None)

    def for_rows(self, w0: int, n_total: int, n_rows: Optional[int] = None) -> _BoundPolicy:
        """The policy for rows that start at walker w0 of a batch of n_total walkers (what selects each row's
        parameter set when G > 1).  n_rows: the row count of the calls to come, if known (prepared now)."""
        return _BoundPolicy(self, w0, n_total, n_rows=n_rows)

    def for_row_index(self, index, n_total: int) -> _BoundPolicy:
        """The policy for the rows of walkers index[0], index[1], ... (an integer device tensor) of a batch of n_total
        walkers: what a gathered, non-contiguous set of rows needs."""
        return _BoundPolicy(self, 0, n_total, index=index)

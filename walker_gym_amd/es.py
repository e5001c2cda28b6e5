"""Evolution strategies on the device: EvolutionStrategy over wg_es_perturb / wg_es_update (include/walker_hip.h), and
the numpy restatements of their arithmetic contract, which agree with the kernels bit for bit.

The noise is a pure function of (seed, generation, pair, parameter index), one Philox4x32-10 call per value, so it is
never stored: the perturb kernel writes the G candidate parameter sets straight into the tensors an MLPPolicy hands to
rollout_policy / rollout_episodes, and the update kernel regenerates the same noise.  A rank that owns a slice of the
population needs (seed, generation) and an all-gather of G fitness scalars, nothing else.

theta is a flat float32 [K] vector: w1 (D*H, element (i, h) at i*H + h; only with a hidden layer), b1 (H; only with
biases), w2 (n2*C with n2 = H or D, element (i, c) at i*C + c), b2 (C; only with biases).  Sets 2j and 2j + 1 are
theta +- RN32(sigma * eps_j) (antithetic pairs).  The update is the centred-rank estimate
  grad[k] = scale * sum_j (util[2j] - util[2j+1]) * eps_j[k],   scale = 1 / (2 * n_pairs * sigma),
summed in float64 in a fixed order (chunks of 256 pairs), then theta += lr * grad in float32.

With hidden2 > 0 both trainers hold a deep MLPPolicy (a second hidden layer, wg_es_mid) and call the _deep entries;
theta then has six segments: w1 (D*H1), b1 (H1), wm (H1*H2, element (j, k) at j*H2 + k), bm (H2), w2 (H2*C), b2 (C), the
order of pg's gradient segments for a deep policy.  The noise, the antithetic rule and both updates are unchanged: they
see the layout through K alone.

EvolutionStrategy(optimizer="adam") takes the same estimate (wg_es_update with no theta_out) and steps theta with the
device optimiser instead (wg_adam_step over the one segment theta, maximize = 1, lr = the trainer's;
walker_gym_amd.optim.adam_step_numpy restates it): Adam's moments and an optional global-norm clip, without leaving the
device.

AdaptiveEvolutionStrategy over wg_es_perturb_diag / wg_es_update_diag keeps one sigma per parameter (a float32 [K]
device vector) and adapts it from the same samples (PGPE with symmetric sampling): with d = RN32(sigma[k] * eps),
  g_theta[k] = scale_theta * sum_j (util[2j] - util[2j+1]) * d_j[k]
  g_sigma[k] = scale_sigma * sum_j ((util[2j] + util[2j+1]) / 2 - base) * (d_j[k]^2 - sigma[k]^2) / sigma[k],
the same chunked float64 sums, then a float32 step on each and a clamp on sigma's (es_update_diag_numpy).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
NOISE_TAG = 0x45530001          # counter word 3 of every noise call
NOISE_SCALE = np.float32(1.0 / np.sqrt(8 * (65536 ** 2 - 1) / 12))   # bits 0x379CC471
CHUNK = 256                     # pairs per float64 partial sum of the update
_M32 = np.uint64(0xFFFFFFFF)


# ---------------------------------------------------------------------------------------------------- host restatements
def philox4x32(counter, key, rounds: int = 10) -> np.ndarray:
    """Philox4x32 (Random123): counter [..., 4] and key [..., 2] of 32-bit words (broadcast against each other) ->
    [..., 4] uint32."""
    c = np.asarray(counter, dtype=np.uint64)
    k = np.asarray(key, dtype=np.uint64)
    c0, c1, c2, c3 = (c[..., i] & _M32 for i in range(4))
    k0, k1 = (k[..., i] & _M32 for i in range(2))
    m0, m1 = np.uint64(PHILOX_M0), np.uint64(PHILOX_M1)
    s32 = np.uint64(32)
    for r in range(rounds):
        p0, p1 = m0 * c0, m1 * c2                      # 32 x 32 -> 64 bits, exact in uint64
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & _M32, (p0 >> s32) ^ c3 ^ k1, p0 & _M32
        k0, k1 = (k0 + np.uint64(PHILOX_W0)) & _M32, (k1 + np.uint64(PHILOX_W1)) & _M32
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


def es_noise_numpy(seed: int, generation: int, first_pair: int, n_pairs: int, K: int) -> np.ndarray:
    """eps(seed, generation, j, k) for j in [first_pair, first_pair + n_pairs), k in [0, K): float32 [n_pairs, K]."""
    seed, generation = int(seed), int(generation)
    if not 0 <= seed < 1 << 64 or not 0 <= generation < 1 << 32:
        raise ValueError("seed is a uint64 and generation a uint32")
    j = (np.arange(n_pairs, dtype=np.uint64) + np.uint64(first_pair))[:, None]
    k = np.arange(K, dtype=np.uint64)[None, :]
    ctr = np.stack(np.broadcast_arrays(k, j, np.uint64(generation), np.uint64(NOISE_TAG)), axis=-1)
    out = philox4x32(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64)).astype(np.int64)
    s = ((out & 0xFFFF) + (out >> 16)).sum(axis=-1)    # the eight 16-bit halves
    return (s - 262140).astype(np.float32) * NOISE_SCALE


def es_perturb_numpy(theta, sigma, seed: int, generation: int, first_pair: int, n_pairs: int) -> np.ndarray:
    """The candidates of pairs [first_pair, first_pair + n_pairs) as flat vectors: float32 [2 * n_pairs, K], row 2i the
    `+` member of pair first_pair + i, row 2i + 1 its `-` member.  Any K and any segment layout: the noise is a function
    of (pair, k) alone, so this restates wg_es_perturb_deep on a six-segment theta as it stands (split_theta(...,
    H2=...) cuts the rows)."""
    theta = np.ascontiguousarray(theta, dtype=np.float32)
    d = np.float32(sigma) * es_noise_numpy(seed, generation, first_pair, n_pairs, theta.shape[0])
    out = np.empty((2 * n_pairs, theta.shape[0]), np.float32)
    out[0::2] = theta[None, :] + d
    out[1::2] = theta[None, :] - d
    return out


def es_utilities_numpy(fitness) -> np.ndarray:
    """Centred ranks in [-0.5, 0.5]: NaN counts as -inf, ties break by index (stable ascending argsort)."""
    f = np.array(fitness, dtype=np.float32)
    G = f.shape[0]
    f[np.isnan(f)] = -np.inf
    order = np.argsort(f, kind="stable")
    rank = np.empty(G, np.int64)
    rank[order] = np.arange(G)
    return (2 * rank - (G - 1)).astype(np.float32) * np.float32(1.0 / (2 * (G - 1)))


def es_update_numpy(theta, util, seed: int, generation: int, first_pair: int, n_pairs: int, scale: float, lr):
    """wg_es_update's arithmetic: (grad, theta_out), float32 [K] each.  util is indexed by set ([G]).  Any K: it is
    wg_es_update_deep's arithmetic on a six-segment theta too (the update never looks at the segments)."""
    theta = np.ascontiguousarray(theta, dtype=np.float32)
    util = np.ascontiguousarray(util, dtype=np.float32)
    K = theta.shape[0]
    with np.errstate(all="ignore"):
        sets = 2 * (first_pair + np.arange(n_pairs))
        d = (util[sets] - util[sets + 1]).astype(np.float64)
        S = np.zeros(K, np.float64)
        for a in range(0, n_pairs, CHUNK):
            n = min(CHUNK, n_pairs - a)
            eps = es_noise_numpy(seed, generation, first_pair + a, n, K).astype(np.float64)
            P = np.zeros(K, np.float64)
            for i in range(n):
                P = P + d[a + i] * eps[i]
            S = S + P
        grad = (S * np.float64(scale)).astype(np.float32)
        return grad, theta + np.float32(lr) * grad


def es_perturb_diag_numpy(theta, sigma_vec, seed: int, generation: int, first_pair: int, n_pairs: int) -> np.ndarray:
    """wg_es_perturb_diag's candidates, laid out as es_perturb_numpy's: d = RN32(sigma_vec[k] * eps).  Any K and layout
    (wg_es_perturb_diag_deep's too), as es_perturb_numpy."""
    theta = np.ascontiguousarray(theta, dtype=np.float32)
    sigma_vec = np.ascontiguousarray(sigma_vec, dtype=np.float32)
    if sigma_vec.shape != theta.shape:
        raise ValueError(f"sigma_vec has shape {sigma_vec.shape}, theta {theta.shape}")
    with np.errstate(all="ignore"):
        d = sigma_vec[None, :] * es_noise_numpy(seed, generation, first_pair, n_pairs, theta.shape[0])
        out = np.empty((2 * n_pairs, theta.shape[0]), np.float32)
        out[0::2] = theta[None, :] + d
        out[1::2] = theta[None, :] - d
    return out


def diag_step(base=0.0, scale_theta=1.0, scale_sigma=1.0, lr_theta=0.0, lr_sigma=0.0, shrink=1.0, grow=1.0,
              sigma_min=1e-8, sigma_max=float("inf")) -> dict:
    """The fields of wg_es_diag_step as a dict (what es_update_diag_numpy and _lib.WgEsDiagStep(**step) take)."""
    return dict(base=base, scale_theta=scale_theta, scale_sigma=scale_sigma, lr_theta=lr_theta, lr_sigma=lr_sigma,
                shrink=shrink, grow=grow, sigma_min=sigma_min, sigma_max=sigma_max)


def es_update_diag_numpy(theta, sigma_vec, util, seed: int, generation: int, first_pair: int, n_pairs: int, step):
    """wg_es_update_diag's arithmetic: (g_theta, theta_out, g_sigma, sigma_out), float32 [K] each.  util is indexed by
    set ([G]); step holds wg_es_diag_step's fields (a dict, see diag_step).  Any K: wg_es_update_diag_deep's too."""
    f32, f64 = np.float32, np.float64
    theta = np.ascontiguousarray(theta, dtype=f32)
    sg = np.ascontiguousarray(sigma_vec, dtype=f32)
    util = np.ascontiguousarray(util, dtype=f32)
    K = theta.shape[0]
    if sg.shape != theta.shape:
        raise ValueError(f"sigma_vec has shape {sg.shape}, theta {theta.shape}")
    st = diag_step(**step)
    with np.errstate(all="ignore"):
        sets = 2 * (first_pair + np.arange(n_pairs))
        u0, u1 = util[sets], util[sets + 1]
        dm = (u0 - u1).astype(f64)
        ds = ((u0 + u1) * f32(0.5) - f32(st["base"])).astype(f64)
        ss = sg.astype(f64) * sg.astype(f64)
        Sm, Ss = np.zeros(K, f64), np.zeros(K, f64)
        for a in range(0, n_pairs, CHUNK):
            n = min(CHUNK, n_pairs - a)
            d = (sg[None, :] * es_noise_numpy(seed, generation, first_pair + a, n, K)).astype(f64)
            q = d * d - ss[None, :]
            Pm, Ps = np.zeros(K, f64), np.zeros(K, f64)
            for i in range(n):
                Pm = Pm + dm[a + i] * d[i]
                Ps = Ps + ds[a + i] * q[i]
            Sm, Ss = Sm + Pm, Ss + Ps
        g_theta = (Sm * f64(st["scale_theta"])).astype(f32)
        g_sigma = ((Ss * f64(st["scale_sigma"])) / sg.astype(f64)).astype(f32)
        theta_out = theta + f32(st["lr_theta"]) * g_theta
        s = sg + f32(st["lr_sigma"]) * g_sigma
        dn, up = sg * f32(st["shrink"]), sg * f32(st["grow"])
        lo = np.where(dn > f32(st["sigma_min"]), dn, f32(st["sigma_min"]))
        hi = np.where(up < f32(st["sigma_max"]), up, f32(st["sigma_max"]))
        sigma_out = np.where(s < lo, lo, np.where(s > hi, hi, s)).astype(f32)
        return g_theta, theta_out, g_sigma, sigma_out


def param_count(D: int, H: int, Cc: int, biases: bool, H2: int = 0) -> int:
    """K of a D -> H -> C policy (H = 0: linear), or with H2 > 0 of the deep D -> H -> H2 -> C one."""
    if H2:
        if not H:
            raise ValueError("H2 > 0 needs H > 0 (a middle layer follows a first hidden layer)")
        return D * H + H * H2 + H2 * Cc + ((H + H2 + Cc) if biases else 0)
    return (D * H + (H if biases else 0) if H else 0) + (H if H else D) * Cc + (Cc if biases else 0)


def split_theta(flat, D: int, H: int, Cc: int, biases: bool, H2: int = 0) -> dict:
    """Views of the segments of flat [..., K] as {'w1': [..., D, H], 'b1': [..., H], 'w2': [..., n2, C], 'b2': [..., C]}
    (None for an absent one); with H2 > 0 also 'wm': [..., H, H2] and 'bm': [..., H2] between b1 and w2, and n2 = H2.
    Works on numpy arrays and torch tensors."""
    if H2 and not H:
        raise ValueError("H2 > 0 needs H > 0 (a middle layer follows a first hidden layer)")
    lead, o, out = tuple(flat.shape[:-1]), 0, {}
    n2 = H2 if H2 else (H if H else D)
    segs = [("w1", (D, H), H > 0), ("b1", (H,), H > 0 and biases)]
    if H2:
        segs += [("wm", (H, H2), True), ("bm", (H2,), biases)]
    segs += [("w2", (n2, Cc), True), ("b2", (Cc,), biases)]
    for name, shape, there in segs:
        n = int(np.prod(shape)) if there else 0
        out[name] = flat[..., o:o + n].reshape(lead + shape) if there else None
        o += n
    if o != flat.shape[-1]:
        raise ValueError(f"{flat.shape[-1]} parameters, the shapes take {o}")
    return out


def theta_from_policy(policy, set_index: int = 0) -> np.ndarray:
    """The flat float32 [K] host vector of parameter set `set_index` of an MLPPolicy, shallow or deep, in theta's
    segment order: what `theta0=` takes to start a trainer from a policy trained elsewhere (walker_gym_amd.pg).  The
    trainers know one switch, biases=True or False, for all layers: a policy with some biases present and others
    absent is refused (all of b1 / bm / b2 that its shape has, or none of them)."""
    g = int(set_index)
    if not 0 <= g < policy.G:
        raise ValueError(f"set_index {set_index} outside 0..{policy.G - 1}")
    names = (["w1", "b1"] if policy.H else []) + (["wm", "bm"] if policy.H2 else []) + ["w2", "b2"]
    have = [getattr(policy, n) is not None for n in names if n.startswith("b")]
    if any(have) and not all(have):
        raise ValueError("theta_from_policy: biases partly present ("
                         + ", ".join(n for n in names if n.startswith("b") and getattr(policy, n) is not None)
                         + " set); the trainers take biases=True (every layer) or biases=False (none)")
    parts = [getattr(policy, n)[g].detach().cpu().numpy().reshape(-1) for n in names if getattr(policy, n) is not None]
    return np.ascontiguousarray(np.concatenate(parts), dtype=np.float32)


# ---------------------------------------------------------------------------------------------------- the trainer
class EvolutionStrategy:
    """Antithetic evolution strategies with centred-rank utilities over an MLPPolicy of `population` parameter sets on
    env's device.  ask() -> MLPPolicy of the generation's candidates; tell(fitness) -> the update; generation_step() a
    whole generation from the state captured at construction.  obs_norm (walker_gym_amd.normalize.ObsNorm): the
    observation normaliser every candidate and mean_policy() evaluate; the caller updates it (generation_step's obs_out
    records the rows), the trainer carries it in its state_dict.  hidden2 > 0: a deep policy, hidden -> hidden2 units
    (wm / bm in the MLPPolicy, theta's six segments, the wg_es_*_deep entries); everything else is the same.
    optimizer="adam": tell() steps theta with wg_adam_step (betas, adam_eps, max_norm; ascent along the estimate with
    lr) instead of theta += lr * grad; None is the plain step."""

    def __init__(self, env, hidden: int = 0, act_dim: Optional[int] = None, biases: bool = True,
                 population: Optional[int] = None, sigma: float = 0.05, lr: float = 0.05, seed: int = 0,
                 act_limit: float = 1.0, theta0=None, obs_norm=None, hidden2: int = 0, optimizer: Optional[str] = None,
                 betas=(0.9, 0.999), adam_eps: float = 1e-8, max_norm: float = float("inf")):
        import torch
        from .policy import MLPPolicy
        if optimizer not in (None, "adam"):
            raise ValueError(f"optimizer {optimizer!r}: None (theta += lr * grad) or 'adam'")
        if isinstance(hidden, (tuple, list)) or getattr(hidden, "ndim", 0):
            raise ValueError(f"hidden {hidden!r}: `hidden` is the width of one hidden layer (an int); the second hidden "
                             "layer of a deep policy is hidden2=")
        self.env = env
        N, D = int(env.N), int(env.obs_dim)
        H, Cc, H2 = int(hidden), int(env.batch.A if act_dim is None else act_dim), int(hidden2)
        G = N if population is None else int(population)
        if G < 2 or G % 2:
            raise ValueError(f"population {G} must be even and >= 2 (antithetic pairs)")
        if N % G:
            raise ValueError(f"population {G} does not divide N = {N}")
        if not 0 <= H <= 256:
            raise ValueError(f"hidden {H} outside 0..256")
        if not 0 <= H2 <= 256:
            raise ValueError(f"hidden2 {H2} outside 0..256")
        if H2 and not H:
            raise ValueError(f"hidden2 {H2} with hidden 0: a second hidden layer follows a first")
        if Cc < 1:
            raise ValueError(f"act_dim {Cc} < 1")
        if not (np.isfinite(sigma) and sigma > 0):
            raise ValueError(f"sigma must be finite and > 0, got {sigma!r}")
        if not np.isfinite(lr):
            raise ValueError(f"lr must be finite, got {lr!r}")
        if not 0 <= int(seed) < 1 << 64:
            raise ValueError("seed is a uint64")
        self.D, self.H, self.H2, self.C, self.G, self.biases = D, H, H2, Cc, G, bool(biases)
        self.K = param_count(D, H, Cc, self.biases, H2)
        self.sigma, self.lr, self.seed, self.generation = float(np.float32(sigma)), float(np.float32(lr)), int(seed), 0
        dv = env.device
        if theta0 is None:
            self.theta = torch.zeros(self.K, dtype=torch.float32, device=dv)
        else:
            t0 = torch.as_tensor(np.asarray(theta0.detach().cpu() if hasattr(theta0, "detach") else theta0,
                                            dtype=np.float32))
            if t0.dim() != 1 or t0.numel() != self.K:
                raise ValueError(f"theta0 has shape {tuple(t0.shape)}, expected ({self.K},)")
            self.theta = t0.to(dv).contiguous()
        # the candidates (allocated once, rewritten by every ask()), behind one MLPPolicy
        n2 = H2 if H2 else (H if H else D)
        e = lambda *s: torch.empty(s, dtype=torch.float32, device=dv)
        w1 = e(G, D, H) if H else None
        b1 = e(G, H) if H and self.biases else None
        b2 = e(G, Cc) if self.biases else None
        # obs_norm (walker_gym_amd.normalize.ObsNorm, shared by every candidate and by mean_policy(); its owner updates it)
        self.obs_norm = obs_norm
        wm = e(G, H, H2) if H2 else None
        bm = e(G, H2) if H2 and self.biases else None
        self.policy = MLPPolicy(e(G, n2, Cc), b2, w1, b1, act_limit=act_limit, obs_norm=obs_norm, wm=wm, bm=bm)
        self.act_limit = self.policy.act_limit
        self.n_pairs = G // 2
        self._work = torch.empty((-(-self.n_pairs // CHUNK), self.K), dtype=torch.float64, device=dv)
        self._grad = torch.empty(self.K, dtype=torch.float32, device=dv)
        self._state0 = env.batch.state_dict()
        self.optimizer = optimizer
        if optimizer == "adam":
            from . import optim
            self.adam_cfg = optim.adam_config(lr=self.lr, betas=betas, eps=adam_eps, max_norm=max_norm, maximize=True)
            self._m, self._v = torch.zeros_like(self.theta), torch.zeros_like(self.theta)
            self._adam_state = torch.zeros(optim.STATE_LEN, dtype=torch.float64, device=dv)
            self._adam_work = torch.empty(-(-self.K // optim.CHUNK), dtype=torch.float64, device=dv)

    # -------------------------------------------------------------------------------------------- the two kernels
    def _call(self, name: str, es, *args) -> None:
        """The entry `name` on (es, args), or with a deep policy its _deep twin on (es, mid, args)."""
        if self.H2:
            mid = _lib.WgEsMid(hidden2=self.H2, wm=_lib.ptr(self.policy.wm), bm=_lib.ptr(self.policy.bm))
            name, args = name + "_deep", (C.byref(mid),) + args
        _lib.check(getattr(_lib.load(), name)(C.byref(es), *args), name)

    def _struct(self) -> _lib.WgEs:
        p, pol = _lib.ptr, self.policy
        return _lib.WgEs(n_sets=self.G, obs_dim=self.D, hidden=self.H, act_dim=self.C, seed=self.seed,
                         generation=self.generation, sigma=self.sigma, theta=p(self.theta), w1=p(pol.w1), b1=p(pol.b1),
                         w2=p(pol.w2), b2=p(pol.b2))

    def ask(self):
        """Write the generation's candidates (wg_es_perturb, or wg_es_perturb_deep, over every pair) and return their
        MLPPolicy (the same object every time: its tensors are rewritten in place)."""
        self._call("wg_es_perturb", self._struct(), 0, self.n_pairs, self.env._stream())
        return self.policy

    def utilities(self, fitness):
        """Centred ranks of fitness [G] on the device (es_utilities_numpy's arithmetic: integer operations and one
        float32 multiply)."""
        import torch
        f = torch.as_tensor(fitness, dtype=torch.float32, device=self.theta.device).reshape(-1)
        if f.numel() != self.G:
            raise ValueError(f"fitness has {f.numel()} values, the population {self.G}")
        f = torch.where(torch.isnan(f), torch.full_like(f, float("-inf")), f)
        order = torch.argsort(f, stable=True)
        rank = torch.empty(self.G, dtype=torch.int64, device=f.device)
        rank[order] = torch.arange(self.G, dtype=torch.int64, device=f.device)
        return (2 * rank - (self.G - 1)).to(torch.float32) * float(np.float32(1.0 / (2 * (self.G - 1))))

    def tell(self, fitness) -> dict:
        """Update theta in place from the candidates' fitness [G] (higher is better; NaN ranks lowest) and move to the
        next generation.  Returns {'grad': [K] f32, the estimate theta moved along (for a caller's own optimiser)};
        with optimizer="adam" also 'grad_norm', the estimate's norm as the step computed it (a 0-d float64 device
        tensor)."""
        util = self.utilities(fitness).contiguous()
        es = self._struct()
        scale = 1.0 / (2.0 * self.n_pairs * self.sigma)
        p = _lib.ptr
        if self.optimizer == "adam":
            from . import optim
            self._call("wg_es_update", es, 0, self.n_pairs, p(util), scale, self.lr, p(self._work), p(self._grad), None,
                       self.env._stream())
            optim.adam_step([self.theta], [self._grad], [self._m], [self._v], self._adam_state,
                            dict(self.adam_cfg, lr=self.lr), self._adam_work)
            self.generation += 1
            return {"grad": self._grad.clone(), "grad_norm": self._adam_state[3].clone()}
        self._call("wg_es_update", es, 0, self.n_pairs, p(util), scale, self.lr, p(self._work), p(self._grad),
                   p(self.theta), self.env._stream())
        self.generation += 1
        return {"grad": self._grad.clone()}

    # -------------------------------------------------------------------------------------------- a whole generation
    def fitness_of(self, res: dict, n_steps: int):
        """Per-set fitness [G] f32 of a rollout's result: rollout_policy's mean return of the set's walkers, or
        rollout_episodes' reward per walker step (finished episodes and the unfinished tail), summed in float64."""
        import torch
        wps = self.env.N // self.G
        if "returns" in res:
            return (res["returns"].double().view(self.G, wps).sum(dim=1) / wps).to(torch.float32)
        tot = res["return_sum"].double() + res["tail_return"].double()
        return (tot.view(self.G, wps).sum(dim=1) / (wps * int(n_steps))).to(torch.float32)

    def generation_step(self, n_steps: int, restore: bool = True, obs_out=None, act_every: int = 1) -> dict:
        """One generation: (restore the state captured at construction,) ask, one closed-loop rollout of every
        candidate (rollout_policy, or rollout_episodes when the env has auto-reset on; obs_out [T, N, D] records its rows,
        raw, for an ObsNorm.update before the next generation), tell.  ValueError for what the
        rollout refuses (resident batches only).  Returns the generation's number, 'fitness' [G] f32, 'grad' [K] f32
        and the fitness statistics 'fitness_mean' / 'fitness_max' / 'fitness_min' over the candidates that did not
        diverge, as 0-d device tensors (nothing here waits for the device).  act_every > 1: the candidates decide every
        act_every steps and hold their action between (the deterministic rollout_held, every generation from zeros)."""
        import torch
        env = self.env
        if int(act_every) < 1:
            raise ValueError(f"generation_step: act_every {act_every} < 1")
        if restore:
            env.batch.load_state_dict(self._state0)
        pol = self.ask()
        if int(act_every) > 1:
            res = env.rollout_held(pol, n_steps, int(act_every), obs_out=obs_out)
        else:
            res = (env.rollout_episodes(pol, n_steps, obs_out=obs_out) if env._ar_mode
                   else env.rollout_policy(pol, n_steps, obs_out=obs_out))
        fit = self.fitness_of(res, n_steps)
        out = self.tell(fit)
        nan = torch.isnan(fit)
        res = {"generation": self.generation - 1, "fitness": fit, "grad": out["grad"],
               "fitness_mean": fit.double().nanmean(),
               "fitness_max": torch.where(nan, torch.full_like(fit, float("-inf")), fit).max(),
               "fitness_min": torch.where(nan, torch.full_like(fit, float("inf")), fit).min()}
        if "grad_norm" in out:
            res["grad_norm"] = out["grad_norm"]
        return res

    def mean_policy(self):
        """The G = 1 policy of theta (a copy); deep with hidden2 > 0."""
        from .policy import MLPPolicy
        seg = split_theta(self.theta.clone(), self.D, self.H, self.C, self.biases, self.H2)
        return MLPPolicy(seg["w2"], seg["b2"], seg["w1"], seg["b1"], act_limit=self.act_limit, obs_norm=self.obs_norm,
                         wm=seg.get("wm"), bm=seg.get("bm"))

    def state_dict(self) -> dict:
        sd = {"theta": self.theta.detach().cpu().clone(), "seed": self.seed, "generation": self.generation,
              "sigma": self.sigma, "lr": self.lr}
        if self.obs_norm is not None:
            sd["obs_norm"] = self.obs_norm.state_dict()
        if self.optimizer == "adam":
            sd.update(m=self._m.detach().cpu().clone(), v=self._v.detach().cpu().clone(),
                      state=self._adam_state.detach().cpu().clone())
        return sd

    def load_state_dict(self, sd: dict) -> None:
        import torch
        t = torch.as_tensor(sd["theta"], dtype=torch.float32).reshape(-1)
        if t.numel() != self.K:
            raise ValueError(f"theta has {t.numel()} elements, expected {self.K}")
        self.theta.copy_(t.to(self.theta.device))
        self.seed, self.generation = int(sd["seed"]), int(sd["generation"])
        self.sigma, self.lr = float(np.float32(sd["sigma"])), float(np.float32(sd["lr"]))
        if self.obs_norm is not None and "obs_norm" in sd:
            self.obs_norm.load_state_dict(sd["obs_norm"])
        if self.optimizer == "adam" and "state" in sd:
            for mine, key in ((self._m, "m"), (self._v, "v"), (self._adam_state, "state")):
                mine.copy_(torch.as_tensor(sd[key], dtype=mine.dtype).reshape(mine.shape).to(mine.device))


class AdaptiveEvolutionStrategy(EvolutionStrategy):
    """EvolutionStrategy with one standard deviation per parameter, adapted from the same antithetic samples (PGPE with
    symmetric sampling) by wg_es_perturb_diag / wg_es_update_diag.  `sigma` is a scalar or a [K] vector of initial
    values; sigma_vec, float32 [K] on the device, is updated in place by every tell(): a step of sigma_lr along the
    estimate, at most sigma_max_change of the value per generation, within [sigma_min, sigma_max]."""

    def __init__(self, env, hidden: int = 0, act_dim: Optional[int] = None, biases: bool = True,
                 population: Optional[int] = None, sigma=0.05, lr: float = 0.05, seed: int = 0,
                 act_limit: float = 1.0, theta0=None, sigma_lr: float = 0.1, sigma_max_change: float = 0.2,
                 sigma_min: float = 1e-8, sigma_max: float = float("inf"), obs_norm=None, hidden2: int = 0,
                 optimizer: Optional[str] = None):
        import torch
        if optimizer is not None:
            raise ValueError("AdaptiveEvolutionStrategy takes no optimizer=: its theta step is inside wg_es_update_diag")
        s0 = np.asarray(sigma.detach().cpu() if hasattr(sigma, "detach") else sigma, dtype=np.float32)
        if s0.ndim > 1:
            raise ValueError(f"sigma has shape {s0.shape}: a scalar or a [K] vector")
        if not (np.isfinite(s0).all() and (s0 > 0).all()):
            raise ValueError("sigma must be finite and > 0 in every entry")
        if not np.isfinite(sigma_lr):
            raise ValueError(f"sigma_lr must be finite, got {sigma_lr!r}")
        if not 0 <= sigma_max_change < 1:
            raise ValueError(f"sigma_max_change {sigma_max_change!r} outside [0, 1)")
        if not (np.isfinite(sigma_min) and sigma_min > 0) or not sigma_max >= sigma_min:
            raise ValueError(f"need 0 < sigma_min <= sigma_max, got {sigma_min!r}, {sigma_max!r}")
        super().__init__(env, hidden=hidden, act_dim=act_dim, biases=biases, population=population,
                         sigma=float(s0.reshape(-1)[0]), lr=lr, seed=seed, act_limit=act_limit, theta0=theta0,
                         obs_norm=obs_norm, hidden2=hidden2)
        if s0.ndim == 1 and s0.shape[0] != self.K:
            raise ValueError(f"sigma has {s0.shape[0]} entries, expected a scalar or ({self.K},)")
        self.sigma = 0.0                 # wg_es's scalar: the _diag calls do not read it
        dv = self.theta.device
        self.sigma_vec = torch.from_numpy(np.array(np.broadcast_to(s0, (self.K,)), dtype=np.float32)).to(dv).contiguous()
        f = lambda x: float(np.float32(x))
        self.sigma_lr, self.sigma_max_change = f(sigma_lr), float(sigma_max_change)
        self.sigma_min, self.sigma_max = f(sigma_min), f(sigma_max)
        self._work = torch.empty((2, -(-self.n_pairs // CHUNK), self.K), dtype=torch.float64, device=dv)
        self._grad_sigma = torch.empty(self.K, dtype=torch.float32, device=dv)

    def step_fields(self) -> dict:
        """wg_es_diag_step's fields for this trainer: base 0, the PGPE scales, shrink / grow rounded to float32."""
        return diag_step(base=0.0, scale_theta=1.0 / (2.0 * self.n_pairs), scale_sigma=1.0 / self.n_pairs,
                         lr_theta=self.lr, lr_sigma=self.sigma_lr,
                         shrink=float(np.float32(1.0 - self.sigma_max_change)),
                         grow=float(np.float32(1.0 + self.sigma_max_change)), sigma_min=self.sigma_min,
                         sigma_max=self.sigma_max)

    def ask(self):
        """Write the generation's candidates (wg_es_perturb_diag, or wg_es_perturb_diag_deep, over every pair) and
        return their MLPPolicy."""
        self._call("wg_es_perturb_diag", self._struct(), _lib.ptr(self.sigma_vec), 0, self.n_pairs, self.env._stream())
        return self.policy

    def tell(self, fitness) -> dict:
        """Update theta and sigma_vec in place from the candidates' fitness [G] and move to the next generation.
        Returns {'grad': [K] f32, 'grad_sigma': [K] f32}, the two estimates the steps were taken along."""
        util = self.utilities(fitness).contiguous()
        es, st, p = self._struct(), _lib.WgEsDiagStep(**self.step_fields()), _lib.ptr
        self._call("wg_es_update_diag", es, p(self.sigma_vec), 0, self.n_pairs, p(util), C.byref(st), p(self._work),
                   p(self._grad), p(self.theta), p(self._grad_sigma), p(self.sigma_vec), self.env._stream())
        self.generation += 1
        self._told = {"grad": self._grad.clone(), "grad_sigma": self._grad_sigma.clone()}
        return self._told

    def generation_step(self, n_steps: int, restore: bool = True, obs_out=None, act_every: int = 1) -> dict:
        """EvolutionStrategy.generation_step's dict plus 'grad_sigma' [K] f32 and the 0-d device tensors 'sigma_mean' /
        'sigma_min' / 'sigma_max' of sigma_vec after the update (nothing here waits for the device)."""
        out = super().generation_step(n_steps, restore, obs_out, act_every)
        out["grad_sigma"] = self._told["grad_sigma"]
        out["sigma_mean"] = self.sigma_vec.double().mean()
        out["sigma_min"], out["sigma_max"] = self.sigma_vec.min(), self.sigma_vec.max()
        return out

    def state_dict(self) -> dict:
        sd = super().state_dict()
        del sd["sigma"]
        sd.update(sigma_vec=self.sigma_vec.detach().cpu().clone(), sigma_lr=self.sigma_lr,
                  sigma_max_change=self.sigma_max_change, sigma_min=self.sigma_min, sigma_max=self.sigma_max)
        return sd

    def load_state_dict(self, sd: dict) -> None:
        import torch
        s = torch.as_tensor(sd["sigma_vec"], dtype=torch.float32).reshape(-1)
        if s.numel() != self.K:
            raise ValueError(f"sigma_vec has {s.numel()} elements, expected {self.K}")
        super().load_state_dict(dict(sd, sigma=0.0))
        self.sigma_vec.copy_(s.to(self.sigma_vec.device))
        f = lambda x: float(np.float32(x))
        self.sigma_lr, self.sigma_max_change = f(sd["sigma_lr"]), float(sd["sigma_max_change"])
        self.sigma_min, self.sigma_max = f(sd["sigma_min"]), f(sd["sigma_max"])

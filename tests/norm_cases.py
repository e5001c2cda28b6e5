"""The batches, normalisers, policies and references that the observation-normalisation tests share
(tests/test_norm_cpu.py checks on the CPU reference alone that every case means something,
tests/test_gpu_norm_rollout.py and tests/test_gpu_norm_rows.py compare bits on the GPU).

A case is an existing batch (policy_cases' recipes, by import: `base` names the policy_cases case whose batch and
parameters it takes; with auto-reset that is episode_cases.config(base)) with
  statistics  obs_moments_numpy over the base case's own un-normalised reference rollout, the entry rows plus every
              step's rows (policy_cases.entry_rows / oracle_rollout), finished with eps = 1e-8;
  clip        1.5;
  weights     freshly drawn (policy_cases.weights over a Case of this file's own): a linear policy's w2 at 0.05, a hidden
              layer's w1 at 0.1 and its w2 at four times that.  On normalised rows these clip a few percent to about
              two fifths of the inputs and saturate up to half of the actions at L = 1, and every walker stays finite
              (test_norm_cpu.py holds the conditions).
The Balance batches have one zero-variance column (a muscle length that never moves in the base rollout), whose scale
is then 1 / sqrt(eps) = 1e4: it is kept, the clip is what makes it harmless.

MAIN are the long cases (their base's T, done and episode boundaries); SHAPES the smallest batches that reach each path
of the in-place pass of lean_policy at T = 4:
  m4    N = 8,192 of M = 4, 16 walkers per wave, D = 26: a lane takes elements q, q + 4, ... (seven or six of them)
  m16   canonical4 with conmid, N = 2,050, 4 per wave, D = 155 (no multiple of 16), a half-full last tile, a set boundary
        at walker 410 inside a tile; G in {1, 5, N}
  m64   N = 6 of M = 64, one walker per wave, D = 596, H = 1 and shared: the one M = 64 policy whose weights are staged
  six   N = 4,096 of M = 4 with six muscles: C = 6 > M
with H in {0, 5, 33}.  COVER is the instance axis: policy_cases.COVER's ten batches, one per (IN3D, NE) of
walker_rollout_policy, each with a shared linear policy, T = 4.
"""
import functools

import numpy as np

import episode_cases as ec
import pg_cases as gc
import policy_cases as pc

CLIP = 1.5
EPS = 1e-8
SCALE_LIN, SCALE_HID = 0.05, 0.1
SEED, STEP_BASE, WALKER_BASE = gc.SEED, gc.STEP_BASE, gc.WALKER_BASE
LEVEL = 0.3          # sigma's level, as pg_cases
SLOTS = ec.SLOTS


class NormCase:
    def __init__(self, name, base, H, C, G, L, seed, T):
        b = pc.case_of(base)
        self.name, self.base, self.T = name, base, T
        self.kind, self.params, self.wpw = b.kind, b.params, b.wpw
        self.pol = pc.Case(name, b.kind, b.params, T, H=H, C=C, G=G, L=L, seed=seed,
                           scale=SCALE_HID if H else SCALE_LIN, wpw=b.wpw)
        self.H, self.C, self.G, self.L = H, C, G, L

    def __repr__(self):
        return self.name


M4, M16, M64, SIX = (pc.shape("m4", 5).name, pc.shape("m16", 33, G=5).name, pc.shape("m64", 1, G=1).name,
                     pc.shape("six", 9, C=6).name)
MAIN = [
    NormCase("canonical4-mlp-5sets", "canonical4-mlp-5sets", 24, 8, 5, 1.0, 301, 12),
    NormCase("balance16-mid-mlp-8sets", "balance16-mid-mlp-8sets", 24, 2, 8, 1.0, 302, 20),
]
SHAPES = [
    NormCase("m4-h5-c2-g8192", M4, 5, 2, 8192, 1.0, 311, 4),
    NormCase("m4-h0-shared", M4, 0, 2, 1, 0.125, 312, 4),        # (26 inputs at 0.05: |y| stays below 1)
    NormCase("m16-h33-g5", M16, 33, 8, 5, 1.0, 313, 4),
    NormCase("m16-h0-perwalker-inf", M16, 0, 8, 2050, float("inf"), 314, 4),
    NormCase("m16-h5-shared", M16, 5, 8, 1, 1.0, 315, 4),
    NormCase("m64-h1-shared", M64, 1, 20, 1, 0.25, 316, 4),     # (one hidden unit: likewise)
    NormCase("six-h5-c6-g1024", SIX, 5, 6, 1024, 1.0, 317, 4),
]
COVER = [NormCase(c.name, c.name, 0, c.C, 1, 0.125, 320 + i, 4) for i, c in enumerate(pc.COVER)]
CASES = MAIN + SHAPES
NAMES = [c.name for c in CASES]
COVER_NAMES = [c.name for c in COVER]
CPU_CHECKED = ["canonical4-mlp-5sets", "balance16-mid-mlp-8sets", "m4-h5-c2-g8192"]   # the issue's three
T_ON = 16            # auto-reset runs of MAIN and SHAPES (episode_cases' T); COVER: 4


def case_of(name):
    return next(c for c in CASES + COVER if c.name == name)


def n_walkers(case):
    return len(pc.spec_of(case.kind)["mass_off"]) - 1


def t_on(case):
    return 4 if case in COVER else T_ON


@functools.lru_cache(maxsize=None)
def stats_of(base):
    """(state, mean, scale) of a base case: the moments of its un-normalised reference rollout's rows."""
    from walker_gym_amd.normalize import obs_moments_numpy, obs_norm_finish_numpy
    rows = np.concatenate([pc.entry_rows(base)[None], pc.oracle_rollout(base)["obs"]])
    st = obs_moments_numpy(rows, chunk_rows=256)
    mean, scale = obs_norm_finish_numpy(st, EPS)
    for a in (st, mean, scale):
        a.setflags(write=False)
    return st, mean, scale


def obs_norm_of(case, device="cpu", identity=False):
    """The case's ObsNorm on `device`; identity: mean 0, scale 1, clip inf."""
    import torch
    from walker_gym_amd.normalize import ObsNorm
    D = pc.obs_dim(case.pol)
    nm = ObsNorm(D, device, clip=float("inf") if identity else CLIP, eps=EPS)
    if not identity:
        st, mean, scale = stats_of(case.base)
        nm.load_state_dict(dict(nm.state_dict(), state=torch.from_numpy(st.copy()), mean=torch.from_numpy(mean.copy()),
                                scale=torch.from_numpy(scale.copy())))
    return nm


def policy_of(case, device=None, norm=True, identity=False):
    """The case's MLPPolicy (its own weights) with its normaliser; norm=False: the same weights without one."""
    import torch
    from walker_gym_amd.policy import MLPPolicy
    mv = lambda a: None if a is None else (torch.from_numpy(a) if device is None else torch.from_numpy(a).to(device))
    w2, b2, w1, b1 = pc.weights(case.pol)
    nm = obs_norm_of(case, "cpu" if device is None else device, identity) if norm else None
    return MLPPolicy(mv(w2), mv(b2), mv(w1), mv(b1), act_limit=case.L, obs_norm=nm)


@functools.lru_cache(maxsize=None)
def sigma_of(name):
    case = case_of(name)
    s = np.random.default_rng(3000 + case.pol.seed).uniform(0.5, 1.5, (case.G, case.C)) * LEVEL
    s = s.astype(np.float32)
    s.setflags(write=False)
    return s


def config(name):
    """The auto-reset inputs of a case: episode_cases.config of its base."""
    return ec.config(case_of(name).base)


def _act(case, pol, obs, noise, t):
    from walker_gym_amd import pg
    if noise:
        return pg.stochastic_forward_numpy(pol, obs, sigma_of(case.name), SEED, STEP_BASE + t, walker_base=WALKER_BASE)
    a = pol.forward_numpy(obs)
    return None, a, None


def _freeze(res):
    for v in res.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def reference_off(name, noise=False, norm=True):
    """Auto-reset off: the reference engine driven by forward_numpy (or stochastic_forward_numpy) of the normalising
    policy on its own raw rows, case.T steps.  Every step's obs (raw) / reward / done / action (/ raw / eps), the final
    state, returns and lengths; 'xn_clipped' the share of normalised inputs at +-clip per step.  norm=False: the same
    weights without the normaliser.  Computed once per argument tuple, shared, never modified."""
    from oracle.oracle import Oracle
    case = case_of(name)
    pol = policy_of(case, norm=norm)
    orc = Oracle(pc.spec_of(case.kind), case.params, n_threads=8)
    obs = orc.observe()["obs"]
    out = dict(obs=[], reward=[], done=[], action=[], raw=[], eps=[], xn_clipped=[])
    for t in range(case.T):
        u, a, e = _act(case, pol, obs, noise, t)
        if norm:
            out["xn_clipped"].append(np.mean(np.abs(pol.obs_norm.normalize_numpy(obs)) == np.float32(CLIP)))
        r = orc.step(a)
        obs = r["obs"]
        out["obs"].append(obs.copy()); out["reward"].append(r["reward"].copy())
        out["done"].append(np.asarray(r["done"]).astype(np.uint8)); out["action"].append(a)
        if noise:
            out["raw"].append(u); out["eps"].append(e)
    res = {k: np.stack(v) for k, v in out.items() if v}
    res.update(pos=orc.pos.copy(), vel=orc.vel.copy(), acc=orc.acc.copy(), muscle_x=orc.mx.copy(),
               steps=orc.steps.copy(), contact=orc.contact.copy())
    res["returns"], res["lengths"] = pc.returns_lengths(res["reward"], res["done"])
    return _freeze(res)


@functools.lru_cache(maxsize=None)
def reference_on(name, noise=False, Tn=None):
    """Auto-reset on: test_gpu_autoreset._Composed driven the same way, t_on(case) steps (or Tn)."""
    from test_gpu_autoreset import _Composed
    case, cfg = case_of(name), config(name)
    pol = policy_of(case)
    ref = _Composed(cfg["spec"], cfg["params"], 1, cfg["pool"])
    obs = ref.orc.observe()["obs"]
    out = dict(action=[], raw=[], eps=[], obs=[], reward=[], done=[], reset=[], final_obs=[], steps=[])
    for t in range(t_on(case) if Tn is None else Tn):
        u, a, e = _act(case, pol, obs, noise, t)
        r = ref.step(a)
        obs = r["obs"]
        out["action"].append(a)
        if noise:
            out["raw"].append(u); out["eps"].append(e)
        out["obs"].append(obs.copy()); out["reward"].append(r["reward"].copy())
        out["done"].append(np.asarray(r["done"]).astype(np.uint8)); out["reset"].append(r["reset"].copy())
        out["steps"].append(np.asarray(r["steps_out"]).astype(np.int32))
        fo = np.full_like(obs, np.nan)   # final_obs: a step writes the rows of the walkers it resets only
        sel = r["reset"] != 0
        fo[sel] = ref.final_obs[sel]
        out["final_obs"].append(fo)
    res = {k: np.stack(v) for k, v in out.items() if v}
    res["state"] = ref.state()
    res["stats"] = ec.accounting(res["reward"], res["reset"], SLOTS)
    return _freeze(res)

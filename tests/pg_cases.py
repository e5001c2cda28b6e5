"""The batches, policies, noise and references that the stochastic-rollout tests share (tests/test_pg_cpu.py checks on the
CPU reference alone that every case means something, tests/test_gpu_stochastic_rollout.py compares bits on the GPU).

The batches are policy_cases' and episode_cases' recipes, by import: each case names the policy_cases case whose batch
and parameters it takes (`base`); with auto-reset that is episode_cases.config(base): max_steps = 5, staggered
counters, the sunk 1 %, the two-row pool.  The policies are this file's (policy_cases.weights over a Case of its own):
  canonical   N = 1,000, one walker per wave: H = 0, a shared policy (its weights staged in LDS), sigma per unit
  balance     N = 100, one walker per wave, NE 1: H = 5, four sets (weights through L2), sigma per set and unit
  canonical4  N = 2,050, 4 per wave, a half-full last tile: H = 5, five sets, the boundary at walker 410 inside a tile
  balance16   N = 8,200, 16 per wave, a half-full last tile: H = 0, one set per walker (sigma per walker)
  six         N = 4,096 of M = 4 with six muscles, 8 per wave: H = 5, six columns on four lanes (a lane owns two units
              and makes two Philox calls), a shared policy
sigma is drawn per (set, unit) in [0.5, 1.5] * the case's level.  The level is a condition on the inputs, held by
test_pg_cpu.py on the reference alone: every run finite, some actions clipped and some not, and RN32(sigma * aeps)
changing the bits of some unclipped action.  T = 12 without auto-reset, 16 with.
"""
import functools

import numpy as np

import episode_cases as ec
import policy_cases as pc

SEED = (5 << 32) + 1234          # above 2^32: both key words in use
STEP_BASE, WALKER_BASE = 7, 3    # non-zero counters everywhere
T_OFF, T_ON, SLOTS = 12, ec.T, ec.SLOTS


class PgCase:
    def __init__(self, name, base, H, C, G, L, seed, scale, level):
        b = pc.case_of(base)
        self.name, self.base, self.level = name, base, level
        self.kind, self.params, self.wpw = b.kind, b.params, b.wpw
        # (a policy_cases Case of this file's own: weights(), policy_of() and lds_bytes() take it as they take theirs)
        self.pol = pc.Case(name, b.kind, b.params, T_OFF, H=H, C=C, G=G, L=L, seed=seed, scale=scale, wpw=b.wpw)
        self.H, self.C, self.G, self.L = H, C, G, L

    def __repr__(self):
        return self.name


SIX = pc.shape("six", 9, C=6).name
CASES = [
    PgCase("canonical-h0-shared", "canonical-lin-shared", 0, 8, 1, 1.0, 101, pc.SCALE_LIN, 0.3),
    PgCase("balance-h5-4sets", "balance-mid-mlp-shared", 5, 2, 4, 1.0, 102, pc.SCALE_MLP, 0.3),
    PgCase("canonical4-h5-5sets", "canonical4-mlp-5sets", 5, 8, 5, 1.0, 103, pc.SCALE_MLP, 0.3),
    PgCase("balance16-h0-perwalker", "balance16-mid-mlp-8sets", 0, 2, 8200, 1.0, 104, pc.SCALE_LIN, 0.3),
    PgCase("six-h5-c6-shared", SIX, 5, 6, 1, 1.0, 105, pc.SCALE_MLP, 0.3),
]
NAMES = [c.name for c in CASES]


def case_of(name):
    return next(c for c in CASES if c.name == name)


def n_walkers(case):
    return len(pc.spec_of(case.kind)["mass_off"]) - 1


@functools.lru_cache(maxsize=None)
def sigma_of(name):
    case = case_of(name)
    s = np.random.default_rng(2000 + case.pol.seed).uniform(0.5, 1.5, (case.G, case.C)) * case.level
    s = s.astype(np.float32)
    s.setflags(write=False)
    return s


def policy_of(case, device=None):
    return pc.policy_of(case.pol, device)


def config(name):
    """The auto-reset inputs of a case: episode_cases.config of its base (spec, params, pool, N, sunk)."""
    return ec.config(case_of(name).base)


def _forward(case, pol, obs, t, first=0, total=None, walker_base=WALKER_BASE):
    from walker_gym_amd import pg
    return pg.stochastic_forward_numpy(pol, obs, sigma_of(case.name), SEED, STEP_BASE + t, walker_base=walker_base,
                                       first_walker=first, n_walkers_total=total)


@functools.lru_cache(maxsize=None)
def reference_off(name, seed=SEED):
    """Auto-reset off: the reference engine driven by stochastic_forward_numpy on its own rows.  Every step's obs /
    reward / done / action / raw / eps, the final state, returns and lengths.  Computed once, shared, never modified."""
    from oracle.oracle import Oracle
    from walker_gym_amd import pg
    case = case_of(name)
    pol = policy_of(case)
    orc = Oracle(pc.spec_of(case.kind), case.params, n_threads=8)
    obs = orc.observe()["obs"]
    out = dict(obs=[], reward=[], done=[], action=[], raw=[], eps=[])
    for t in range(T_OFF):
        u, a, e = pg.stochastic_forward_numpy(pol, obs, sigma_of(name), seed, STEP_BASE + t, walker_base=WALKER_BASE)
        r = orc.step(a)
        obs = r["obs"]
        out["obs"].append(obs.copy()); out["reward"].append(r["reward"].copy())
        out["done"].append(np.asarray(r["done"]).astype(np.uint8)); out["action"].append(a); out["raw"].append(u)
        out["eps"].append(e)
    res = {k: np.stack(v) for k, v in out.items()}
    res.update(pos=orc.pos.copy(), vel=orc.vel.copy(), acc=orc.acc.copy(), muscle_x=orc.mx.copy(),
               steps=orc.steps.copy(), contact=orc.contact.copy())
    res["returns"], res["lengths"] = pc.returns_lengths(res["reward"], res["done"])
    for v in res.values():
        v.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def reference_on(name):
    """Auto-reset on: test_gpu_autoreset._Composed driven the same way (episode_cases.reference with the noise)."""
    from test_gpu_autoreset import _Composed
    case, cfg = case_of(name), config(name)
    pol = policy_of(case)
    ref = _Composed(cfg["spec"], cfg["params"], 1, cfg["pool"])
    obs = ref.orc.observe()["obs"]
    out = dict(action=[], raw=[], eps=[], obs=[], reward=[], done=[], reset=[], final_obs=[], steps=[])
    for t in range(T_ON):
        u, a, e = _forward(case, pol, obs, t)
        r = ref.step(a)
        obs = r["obs"]
        out["action"].append(a); out["raw"].append(u); out["eps"].append(e)
        out["obs"].append(obs.copy()); out["reward"].append(r["reward"].copy())
        out["done"].append(np.asarray(r["done"]).astype(np.uint8)); out["reset"].append(r["reset"].copy())
        out["steps"].append(np.asarray(r["steps_out"]).astype(np.int32))
        fo = np.full_like(obs, np.nan)   # final_obs: a step writes the rows of the walkers it resets only
        sel = r["reset"] != 0
        fo[sel] = ref.final_obs[sel]
        out["final_obs"].append(fo)
    res = {k: np.stack(v) for k, v in out.items()}
    res["state"] = ref.state()
    res["stats"] = ec.accounting(res["reward"], res["reset"], SLOTS)
    for v in res.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return res

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
  canonical4-perwalker-c5-inf  the canonical4 batch: H = 0, one set per walker, C = 5 of the 8 muscles, act_limit = inf
              (no clip hides a wrong u: action is raw, in bits)
  wide        N = 6 of M = 64, one walker per wave, D = 596: H = 5, 20 columns, a shared policy
sigma is drawn per (set, unit) in [0.5, 1.5] * the case's level.  The level is a condition on the inputs, held by
test_pg_cpu.py on the reference alone: every run finite, some actions clipped and some not, and RN32(sigma * aeps)
changing the bits of some unclipped action.  T = 12 without auto-reset, 16 with.

COVER (outside NAMES: the parametrised tests above do not multiply) is the instance axis: policy_cases.COVER's ten
batches, one per (IN3D, NE) of walker_rollout_policy with 512 full tiles (the compact records; the 16-byte ones under
WG_EDGE8=0), each with COVER's own shared linear policy and sigma per unit.  T = COVER's 4 without auto-reset, 16 with.
"""
import functools

import numpy as np

import episode_cases as ec
import policy_cases as pc

SEED = (5 << 32) + 1234          # above 2^32: both key words in use
STEP_BASE, WALKER_BASE = 7, 3    # non-zero counters everywhere
T_OFF, T_ON, SLOTS = 12, ec.T, ec.SLOTS


class PgCase:
    def __init__(self, name, base, H, C, G, L, seed, scale, level, t_off=T_OFF, own=True):
        b = pc.case_of(base)
        self.name, self.base, self.level, self.t_off = name, base, level, t_off
        self.kind, self.params, self.wpw = b.kind, b.params, b.wpw
        # (a policy_cases Case of this file's own: weights(), policy_of() and lds_bytes() take it as they take theirs;
        # own=False: the base case's policy itself)
        self.pol = pc.Case(name, b.kind, b.params, t_off, H=H, C=C, G=G, L=L, seed=seed, scale=scale, wpw=b.wpw) \
            if own else b
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
    PgCase("canonical4-perwalker-c5-inf", "canonical4-lin-perwalker-c5-inf", 0, 5, 2050, float("inf"), 106, pc.SCALE_LIN,
           0.3),
    PgCase("wide-h5-c20-shared", "wide-mlp-shared", 5, 20, 1, 1.0, 107, pc.SCALE_MLP, 0.3),
]
NAMES = [c.name for c in CASES]

# The noise level of each instance-coverage case (test_pg_cpu.py holds the conditions on the reference alone: the other
# cases' 0.3 meets them on all ten, clipping 0.7 % (ne1-3d) to 36 % of the actions).
COVER_LEVEL = {c.name: 0.3 for c in pc.COVER}
COVER = [PgCase(c.name, c.name, c.H, c.C, c.G, c.L, c.seed, c.scale, COVER_LEVEL[c.name], t_off=c.T, own=False)
         for c in pc.COVER]
COVER_NAMES = [c.name for c in COVER]
LAST = (1 << 32)                 # the counters' end: step_base + T and walker_base + N may reach it
ZEROS = "canonical4-h5-5sets"    # the case sigma_of(.., zeros=True) is made for


def case_of(name):
    return next(c for c in CASES + COVER if c.name == name)


def n_walkers(case):
    return len(pc.spec_of(case.kind)["mass_off"]) - 1


@functools.lru_cache(maxsize=None)
def sigma_of(name, zeros=False):
    """The case's sigma [G, C]; zeros: set 1 all zero and one zero column in every other set (column (3 * g + 1) % C)."""
    case = case_of(name)
    s = np.random.default_rng(2000 + case.pol.seed).uniform(0.5, 1.5, (case.G, case.C)) * case.level
    s = s.astype(np.float32)
    if zeros:
        assert case.G > 2 and case.C > 1
        s[1] = 0.0
        for g in range(case.G):
            s[g, (3 * g + 1) % case.C] = 0.0
    s.setflags(write=False)
    return s


def policy_of(case, device=None):
    return pc.policy_of(case.pol, device)


def config(name):
    """The auto-reset inputs of a case: episode_cases.config of its base (spec, params, pool, N, sunk)."""
    return ec.config(case_of(name).base)


@functools.lru_cache(maxsize=None)
def reference_off(name, seed=SEED, step_base=STEP_BASE, walker_base=WALKER_BASE, zeros=False):
    """Auto-reset off: the reference engine driven by stochastic_forward_numpy on its own rows, case.t_off steps.  Every
    step's obs / reward / done / action / raw / eps, the final state, returns and lengths.  Computed once per argument
    tuple, shared, never modified."""
    from oracle.oracle import Oracle
    from walker_gym_amd import pg
    case = case_of(name)
    pol = policy_of(case)
    orc = Oracle(pc.spec_of(case.kind), case.params, n_threads=8)
    obs = orc.observe()["obs"]
    out = dict(obs=[], reward=[], done=[], action=[], raw=[], eps=[])
    for t in range(case.t_off):
        u, a, e = pg.stochastic_forward_numpy(pol, obs, sigma_of(name, zeros), seed, step_base + t, walker_base=walker_base)
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
def reference_on(name, step_base=STEP_BASE, walker_base=WALKER_BASE):
    """Auto-reset on: test_gpu_autoreset._Composed driven the same way (episode_cases.reference with the noise)."""
    from test_gpu_autoreset import _Composed
    from walker_gym_amd import pg
    case, cfg = case_of(name), config(name)
    pol = policy_of(case)
    ref = _Composed(cfg["spec"], cfg["params"], 1, cfg["pool"])
    obs = ref.orc.observe()["obs"]
    out = dict(action=[], raw=[], eps=[], obs=[], reward=[], done=[], reset=[], final_obs=[], steps=[])
    for t in range(T_ON):
        u, a, e = pg.stochastic_forward_numpy(pol, obs, sigma_of(name), SEED, step_base + t, walker_base=walker_base)
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

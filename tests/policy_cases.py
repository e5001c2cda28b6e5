"""The batches and policies that the closed-loop rollout tests share (tests/test_policy_cpu.py checks on the CPU that
every one of them stays finite, tests/test_gpu_policy_rollout.py compares bits on the GPU).

Shapes are the smallest that exercise each way the kernel can go wrong:
  canonical  M=16 K=40 A=8 in3d D=152, N=1000: 4 walkers per wave, a partial last block; with G=4 a parameter-set boundary
             (walker 250) falls inside a wave tile
  balance    Balance-v0 x100, M=4 A=2 2-D: the NE=1 instance, mid columns (D=29) and the G1 getstat form (midform 2);
             per-walker start velocities and step counters so that the walkers differ and `done` fires at different steps
  wide       M=64 K=150 A=20: one walker per wave (the M == 64 masks), three spring passes, D=596
  discrete   canonical with action_mode=1 and 5 action columns: `a != 0` semantics, fewer columns than muscles
The lean kernels halve a small batch's walkers per wave until it has 512 wave tiles, so at those sizes a wave holds one
walker.  Two larger batches fill the tiles (Case.wpw, asserted on the GPU):
  canonical4 N=2050: 4 walkers per wave (three spring passes, the compact spring records), 513 tiles, the last one half
             full in a partial last block; with G=5 the set boundary at walker 410 falls inside a tile
  balance16  N=8200: 16 walkers per wave, the last tile half full; with G=8 the boundary at walker 1025 inside a tile
Policies: H in {0, 24} (24 is no multiple of 16 and exceeds 4), C in {A, fewer}, G in {1, 4 or a few, N}, L in {1, inf}.
"""
import functools

import numpy as np

# Weight scales (standard deviation of the normal draws).  The rows hold accelerations in the thousands, so a closed
# loop saturates every output at much larger weights and never reaches the clip at much smaller ones: these clip a
# fifth to a half of the outputs at act_limit = 1 and leave every walker finite (test_policy_cpu.py keeps the check).
SCALE_LIN, SCALE_MLP = 0.001, 0.008   # a linear policy's w2 / a hidden layer's w1 (its w2: four times that)


class Case:
    def __init__(self, name, kind, params, T, H, C, G, L, seed, oracle=True, done=False, scale=None, wpw=1):
        self.name, self.kind, self.params, self.T = name, kind, params, T
        self.wpw = wpw   # walkers per wave tile of the launch
        self.scale = scale if scale is not None else (SCALE_MLP if H else SCALE_LIN)
        self.H, self.C, self.G, self.L, self.seed, self.oracle, self.done = H, C, G, L, seed, oracle, done

    def __repr__(self):
        return self.name


@functools.lru_cache(maxsize=None)
def spec_of(kind):
    from walker_gym_amd.synthetic import canonical_walkers
    from walker_gym_amd.walker import balance_spec
    if kind == "canonical":
        return canonical_walkers(1000, seed=31)
    if kind == "wide":
        return canonical_walkers(6, seed=7, M=64, K=150, A=20)
    if kind == "canonical4":
        return canonical_walkers(2050, seed=32)
    if kind in ("balance", "balance16"):
        n = 100 if kind == "balance" else 8200
        spec = dict(balance_spec(n))
        rng = np.random.default_rng(5)
        vel = np.array(spec["vel"], np.float32).reshape(-1, 3).copy()
        vel[:, :2] += rng.uniform(-3, 3, (vel.shape[0], 2)).astype(np.float32)
        spec["vel"] = vel
        spec["steps"] = (np.arange(n) % 7).astype(np.int32)   # done (steps >= max_steps) at differing steps
        return spec
    if kind in PASSES:   # instance coverage
        kw = dict(PASSES[kind])
        return canonical_walkers(kw.pop("N"), seed=33, **kw)
    raise KeyError(kind)


BAL = dict(in3d=0, max_steps=16)
CASES = [
    Case("canonical-lin-shared", "canonical", dict(in3d=1), 12, H=0, C=8, G=1, L=1.0, seed=1),
    Case("canonical-mlp-4sets-c5-inf", "canonical", dict(in3d=1), 12, H=24, C=5, G=4, L=float("inf"), seed=2),
    Case("canonical-mlp-perwalker", "canonical", dict(in3d=1), 12, H=24, C=8, G=1000, L=1.0, seed=3),
    Case("canonical-lin-4sets-c5", "canonical", dict(in3d=1), 12, H=0, C=5, G=4, L=1.0, seed=4),
    Case("balance-mid-mlp-shared", "balance", dict(BAL, conmid=1, midform=1), 20, H=24, C=2, G=1, L=1.0, seed=5,
         done=True),
    Case("balance-g1-lin-4sets-inf", "balance", dict(BAL, midform=2), 20, H=0, C=2, G=4, L=float("inf"), seed=6,
         done=True, scale=0.0005),   # (unclipped feedback on the G1 rows grows fastest)
    Case("balance-g1-mlp-perwalker-c1", "balance", dict(BAL, midform=2), 20, H=24, C=1, G=100, L=1.0, seed=7,
         done=True),
    Case("wide-mlp-shared", "wide", dict(in3d=1), 6, H=24, C=20, G=1, L=1.0, seed=8, oracle=False),
    Case("wide-lin-perwalker-c5-inf", "wide", dict(in3d=1), 6, H=0, C=5, G=6, L=float("inf"), seed=9, oracle=False),
    Case("discrete-mlp-4sets-c5", "canonical", dict(in3d=1, action_mode=1), 12, H=24, C=5, G=4, L=1.0, seed=10,
         oracle=False),
    Case("discrete-lin-shared-c5", "canonical", dict(in3d=1, action_mode=1), 12, H=0, C=5, G=1, L=1.0, seed=11,
         oracle=False),
    Case("canonical4-mlp-5sets", "canonical4", dict(in3d=1), 12, H=24, C=8, G=5, L=1.0, seed=12, wpw=4),
    Case("canonical4-lin-perwalker-c5-inf", "canonical4", dict(in3d=1), 12, H=0, C=5, G=2050, L=float("inf"), seed=13,
         wpw=4),
    Case("balance16-mid-mlp-8sets", "balance16", dict(BAL, conmid=1, midform=1), 20, H=24, C=2, G=8, L=1.0, seed=14,
         done=True, wpw=16),
]


# Instance coverage of the resident policy kernels (one row per (IN3D, NE, E8) of walker_rollout_policy): 512 full standard
# tiles, so that the launch reads the compact spring records (the 16-byte ones under WG_EDGE8=0), at every spring-pass
# count: 8,192 walkers of M = 4, K = 4 (16 per wave, one pass) and 512 walkers of M = 64 (one per wave: 120, 150, 200
# and 300 springs are 2, 3, 4 and 5 passes, the last on the NE 8 instance), in 2-D and 3-D, a shared linear policy.
PASSES = {"ne1": dict(N=8192, M=4, K=4, A=2), "ne2": dict(N=512, M=64, K=120, A=8), "ne3": dict(N=512, M=64, K=150, A=8),
          "ne4": dict(N=512, M=64, K=200, A=8), "ne8": dict(N=512, M=64, K=300, A=8)}
COVER = [Case(f"{kind}-{2 + d}d", kind, dict(in3d=d), 4, H=0, C=kw["A"], G=1, L=1.0, seed=21 + 2 * i + d,
              wpw=64 // kw["M"]) for i, (kind, kw) in enumerate(PASSES.items()) for d in (0, 1)]


def case_of(name):
    return next(c for c in CASES + COVER if c.name == name)


def obs_dim(case):
    spec = spec_of(case.kind)
    M = int(spec["mass_off"][1] - spec["mass_off"][0])
    A = int(np.asarray(spec["n_muscles"])[0])
    return 3 * (3 if case.params.get("in3d") else 2) * M + (3 if case.params.get("conmid") else 0) + A


def weights(case):
    """The case's parameter sets as numpy float32 arrays: (w2, b2, w1, b1), MLPPolicy's argument order."""
    rng = np.random.default_rng(1000 + case.seed)
    D, H, C, G = obs_dim(case), case.H, case.C, case.G
    n2 = H if H else D
    s = case.scale
    w1 = (rng.standard_normal((G, D, H)) * s).astype(np.float32) if H else None
    b1 = (rng.standard_normal((G, H)) * s).astype(np.float32) if H else None
    w2 = (rng.standard_normal((G, n2, C)) * (s * (4.0 if H else 1.0))).astype(np.float32)
    b2 = (rng.standard_normal((G, C)) * s).astype(np.float32) if case.seed % 2 else None   # (a NULL bias too)
    return w2, b2, w1, b1


def policy_of(case, device=None):
    import torch
    from walker_gym_amd.policy import MLPPolicy
    mv = lambda a: None if a is None else (torch.from_numpy(a) if device is None else torch.from_numpy(a).to(device))
    w2, b2, w1, b1 = weights(case)
    return MLPPolicy(mv(w2), mv(b2), mv(w1), mv(b1), act_limit=case.L)


@functools.lru_cache(maxsize=None)
def oracle_rollout(name):
    """The closed loop on the CPU reference engine: Oracle.step(policy.forward_numpy(obs)), step 0 on the entry
    state's observation.  Every step's obs / reward / done / action and the final state, as numpy arrays (shared by the
    tests that need it, never modified)."""
    from oracle.oracle import Oracle
    case = case_of(name)
    pol = policy_of(case)
    orc = Oracle(spec_of(case.kind), case.params, n_threads=8)
    obs = orc.observe()["obs"]
    out = dict(obs=[], reward=[], done=[], action=[])
    for t in range(case.T):
        a = pol.forward_numpy(obs)
        r = orc.step(a)
        obs = r["obs"]
        out["obs"].append(obs.copy()); out["reward"].append(r["reward"].copy())
        out["done"].append(r["done"].copy()); out["action"].append(a)
    res = {k: np.stack(v) for k, v in out.items()}
    res.update(pos=orc.pos.copy(), vel=orc.vel.copy(), acc=orc.acc.copy(), muscle_x=orc.mx.copy(),
               steps=orc.steps.copy(), contact=orc.contact.copy(), mass_off=orc.mass_off.copy())
    for v in res.values():
        v.setflags(write=False)
    return res


def returns_lengths(reward, done):
    """The sequential float32 return and the step count of [T, N] reward / done: rewards added in step order up to and
    including the first done step."""
    T, N = reward.shape
    ret, length, alive = np.zeros(N, np.float32), np.zeros(N, np.int32), np.ones(N, bool)
    for t in range(T):
        ret = np.where(alive, ret + reward[t].astype(np.float32), ret).astype(np.float32)
        length = length + alive.astype(np.int32)
        alive = alive & (done[t] == 0)
    return ret, length

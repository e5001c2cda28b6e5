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

SHAPES (below) is the policy's own shape axis: every hidden width at which lean_policy's unit-to-lane mapping or one of
its remainder loops takes another path, on one batch per wave tile (M = 4 with 16 and with 8 walkers per wave, M = 16,
M = 64), with act_limit = inf, so that no clip hides a wrong pre-activation.
"""
import functools

import numpy as np

# Weight scales (standard deviation of the normal draws).  The rows hold accelerations in the thousands, so a closed
# loop saturates every output at much larger weights and never reaches the clip at much smaller ones: these clip a
# fifth to a half of the outputs at act_limit = 1 and leave every walker finite (test_policy_cpu.py keeps the check).
SCALE_LIN, SCALE_MLP = 0.001, 0.008   # a linear policy's w2 / a hidden layer's w1 (its w2: four times that)


class Case:
    def __init__(self, name, kind, params, T, H, C, G, L, seed, oracle=True, done=False, scale=None, wpw=1,
                 balanced=False):
        self.name, self.kind, self.params, self.T = name, kind, params, T
        self.wpw = wpw   # walkers per wave tile of the launch
        self.balanced = balanced   # w1 shifted so that every hidden unit is on for some walkers, off for others
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
    if kind == "six":   # 8 walkers per wave, 48 muscle lanes: more action columns (6) than lanes per walker (4)
        return canonical_walkers(4096, seed=34, M=4, K=6, A=6)
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


# The policy's shape axis (walker_rollout_policy's lean_policy: lane q of a walker's M takes hidden units q, q + M, ...
# two at a time, then output columns q, q + M, ...).  One batch per wave tile, each the smallest that gives the tile:
#   m4   the `ne1` batch (N = 8192, M = 4, 16 per wave, compact records), 2-D: D = 26 (D mod 4 = 2)
#   m16  canonical4 (N = 2050, M = 16, 4 per wave, a partial last tile and block), conmid: D = 155 (D mod 4 = 3)
#   m64  wide (N = 6, M = 64, 1 per wave): D = 596
#   six  N = 4096 of M = 4, K = 6, A = 6 (8 per wave): D = 42, and C = 5, 6 > M (the output loop goes round twice)
# H per tile: 1, M - 1, M, M + 1 (a lane with one unit, a single beside a pair), 2M, 2M + 1 (a lane that ends on an odd
# unit after a full pair), H < 8 and H mod 8 != 0 (policy_unit's tail behind a hidden layer), 256 (the widest).
# G: 1; a set boundary inside a wave tile where N allows one (m4: 1024 sets of 8 walkers, m16: 5, 10 or 2 sets; an M = 64
# tile is one walker, m64 takes 2 or 3 sets); N only at H <= 33 (so m64, whose only such width is 1, has it once, and
# that width once more with G = 1, the one M = 64 policy small enough for its weights to be staged in LDS).
# H = 256 once with G = 1 and once with G = 2.  C = A but for one case per tile.  T = 3, L = inf, distinct seeds (both
# biases on the odd ones).
# Scales: a hidden case's actions at step 0 come from rows that hold positions alone (tens) through balanced units, the
# later steps' from accelerations in the thousands; every scale below keeps all walkers finite for the T steps and
# some |action| above 1 (tests/test_policy_cpu.py holds both); the wider layers take smaller weights.
def _shape(tile, H, C, G, seed, scale):
    kind, params, wpw = {"m4": ("ne1", dict(in3d=0), 16), "m16": ("canonical4", dict(in3d=1, conmid=1), 4),
                         "m64": ("wide", dict(in3d=1), 1), "six": ("six", dict(in3d=1), 8)}[tile]
    return Case(f"{tile}-h{H}-c{C}-g{G}", kind, params, 3, H=H, C=C, G=G, L=float("inf"), seed=seed, scale=scale,
                wpw=wpw, balanced=H > 0)


SHAPES = [
    _shape("m4", 1, 2, 8192, 41, 0.02),      # (0.02: 26 inputs and few units; |action| passes 1 from step 1 on)
    _shape("m4", 3, 2, 1, 42, 0.02),         # (as above)
    _shape("m4", 4, 1, 1024, 43, 0.02),      # (as above; fewer columns)
    _shape("m4", 5, 2, 8192, 44, 0.02),      # (as above)
    _shape("m4", 8, 2, 1024, 45, 0.02),      # (as above)
    _shape("m4", 9, 2, 1, 46, 0.02),         # (as above)
    _shape("m4", 256, 2, 1, 47, 0.012),      # (0.012: 256 units add up in the outputs; w2 is four times that)
    _shape("m4", 256, 2, 2, 48, 0.012),      # (as above)
    _shape("m16", 1, 8, 2050, 51, 0.016),    # (0.016: twice SCALE_MLP, whose actions stay below 1 for three steps)
    _shape("m16", 15, 5, 5, 52, 0.016),      # (as above; fewer columns)
    _shape("m16", 16, 8, 1, 53, 0.016),      # (as above)
    _shape("m16", 17, 8, 2050, 54, 0.016),   # (as above)
    _shape("m16", 32, 8, 1, 55, 0.016),      # (as above: the benchmark width)
    _shape("m16", 33, 8, 1, 56, 0.016),      # (as above)
    _shape("m16", 33, 8, 5, 57, 0.016),      # (as above; the set boundary at walker 410 inside a tile)
    _shape("m16", 40, 8, 1, 58, 0.016),      # (as above)
    _shape("m16", 64, 8, 10, 59, 0.012),     # (0.012 at 64 units)
    _shape("m16", 255, 8, 2, 60, 0.008),     # (0.008 = SCALE_MLP at the widest)
    _shape("m16", 256, 8, 1, 61, 0.008),     # (as above)
    _shape("m16", 256, 8, 2, 62, 0.008),     # (as above)
    _shape("m64", 1, 20, 6, 63, 0.02),       # (0.02: one unit)
    _shape("m64", 1, 20, 1, 74, 0.02),       # (as above; shared: the only width whose M = 64 weights fit the LDS)
    _shape("m64", 63, 7, 3, 64, 0.012),      # (0.012 around 64 units; fewer columns)
    _shape("m64", 64, 20, 1, 65, 0.012),     # (as above)
    _shape("m64", 65, 20, 2, 66, 0.012),     # (as above)
    _shape("m64", 128, 20, 3, 67, 0.008),    # (0.008 = SCALE_MLP from 128 units up)
    _shape("m64", 129, 20, 1, 68, 0.008),    # (as above)
    _shape("m64", 256, 20, 1, 69, 0.008),    # (as above)
    _shape("m64", 256, 20, 2, 70, 0.008),    # (as above)
    _shape("six", 0, 6, 1, 71, 0.005),       # (0.005: a linear policy fed back unclipped; 0.02 reaches 1e3 in three steps)
    _shape("six", 9, 5, 4096, 72, 0.02),     # (0.02, as m4)
    _shape("six", 9, 6, 1024, 73, 0.02),     # (as above; 4 walkers per set, a boundary inside every tile)
]


def case_of(name):
    return next(c for c in CASES + COVER + SHAPES if c.name == name)


def lds_bytes(case, episodes=False):
    """The host's LDS arithmetic for a case restated (lean_geo and rollout_policy in csrc/wg_host.h): the
    workgroup's bytes without staged weights, the weights' bytes, and whether WG_POLICY_STAGE = 0 / 1 / 2 stages them."""
    spec = spec_of(case.kind)
    N, K = len(spec["mass_off"]) - 1, int(spec["edge_off"][1] - spec["edge_off"][0])
    A, D, H, C, w = int(np.asarray(spec["n_muscles"])[0]), obs_dim(case), case.H, case.C, case.wpw
    a16 = lambda n: (n + 15) & ~15
    ew = w * K
    pl = (ew + 3) & ~3
    sl = a16(pl * 24) + a16(pl * 12) + a16(ew * 4 + 4) + a16(max(1, w * A) * 4)
    sl += a16(w * D * 4) + a16(max(1, w * H) * 4) + a16(w * C * 4) + w * (32 if episodes else 16)
    wpb = 1 if (N + w - 1) // w <= 1024 else 4
    lds, wts = wpb * sl, 4 * (D * H + (H if H else D) * C)
    cap = max(1, (12 if (ew + 63) // 64 > 4 else 16) // wpb)
    free = min(cap, 160 * 1024 // lds) == min(cap, 160 * 1024 // (lds + wts))
    fits = case.G == 1 and lds + wts <= 80 * 1024
    return dict(lds=lds, weights=wts, staged={0: False, 1: fits and free, 2: fits})


def shape(tile, H, G=None, C=None):
    """The SHAPES case of a tile at a width (and, where several share it, a set count or column count)."""
    hit = [c for c in SHAPES if c.name.startswith(f"{tile}-h{H}-") and G in (None, c.G) and C in (None, c.C)]
    assert len(hit) == 1, (tile, H, G, C, hit)
    return hit[0]


def obs_dim(case):
    spec = spec_of(case.kind)
    M = int(spec["mass_off"][1] - spec["mass_off"][0])
    A = int(np.asarray(spec["n_muscles"])[0])
    return 3 * (3 if case.params.get("in3d") else 2) * M + (3 if case.params.get("conmid") else 0) + A


@functools.lru_cache(maxsize=None)
def entry_rows(name):
    """The observation rows of a case's entry state (what step 0 acts on), from the reference engine."""
    from oracle.oracle import Oracle
    case = case_of(name)
    rows = Oracle(spec_of(case.kind), case.params, n_threads=8).observe()["obs"].copy()
    rows.setflags(write=False)
    return rows


def _balance(case, w1, b1):
    """A drawn w1 (and b1) adjusted so that each hidden unit's step-0 pre-activation is positive for some walkers and
    negative for others.  The entry rows of a batch are one lattice plus jitter, so a drawn unit has one sign for nearly
    every walker, at any scale: a unit that is off for all of them would hide its column of w1, one that is on for all
    its ReLU.  Each set's columns are shifted along the mean row of the set's walkers by the amount that puts the median
    walker's pre-activation at zero (a change of a few percent of the scale); where a set is one walker, the unit's
    column and bias are negated where needed for the signs to alternate with walker + unit."""
    x = entry_rows(case.name).astype(np.float64)
    G, wps = case.G, x.shape[0] // case.G
    for g in range(G):
        xs = x[g * wps:(g + 1) * wps]
        z = xs @ w1[g].astype(np.float64) + (0.0 if b1 is None else b1[g].astype(np.float64))   # [wps, H]
        if wps == 1:
            flip = (z[0] > 0) != ((g + np.arange(case.H)) % 2 == 0)
            w1[g][:, flip] *= -1
            if b1 is not None:
                b1[g][flip] *= -1
        else:
            mean = xs.mean(0)
            alpha = np.median(z / (xs @ mean)[:, None], axis=0)
            w1[g] = (w1[g] - np.outer(mean, alpha)).astype(np.float32)
    return w1, b1


@functools.lru_cache(maxsize=None)
def _weights(case):
    rng = np.random.default_rng(1000 + case.seed)
    D, H, C, G = obs_dim(case), case.H, case.C, case.G
    n2 = H if H else D
    s = case.scale
    w1 = (rng.standard_normal((G, D, H)) * s).astype(np.float32) if H else None
    b1 = (rng.standard_normal((G, H)) * s).astype(np.float32) if H else None
    w2 = (rng.standard_normal((G, n2, C)) * (s * (4.0 if H else 1.0))).astype(np.float32)
    b2 = (rng.standard_normal((G, C)) * s).astype(np.float32) if case.seed % 2 else None   # (a NULL bias too)
    if H and case.balanced:   # (SHAPES: b1 too is NULL on the even seeds)
        w1, b1 = _balance(case, w1, b1 if case.seed % 2 else None)
    return w2, b2, w1, b1


def weights(case):
    """The case's parameter sets as numpy float32 arrays: (w2, b2, w1, b1), MLPPolicy's argument order (the caller's
    own copies)."""
    return tuple(None if a is None else a.copy() for a in _weights(case))


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

"""The batches, policies and references that the action-hold tests share (tests/test_hold_cpu.py checks on the CPU
reference alone that every case means something, tests/test_gpu_held_rollout.py compares bits on the GPU).

The batches and policies are pg_cases', norm_cases' and policy_cases', by import:
  canonical4-h5-5sets, balance-h5-4sets, balance16-h0-perwalker, six-h5-c6-shared   pg_cases (policy, sigma)
  discrete-mlp-4sets-c5      policy_cases' discrete batch and policy (action_mode 1, 5 of 8 muscles), sigma drawn here
  norm-canonical4-mlp-5sets  norm_cases' case of that name: its weights, its normaliser (on), its sigma
Auto-reset on: episode_cases.config of the case's base (max_steps = 5, counters staggered by w % 5, the sunk 1 %, the
two-row pool), T = 16.  Auto-reset off: the same batch with spec["steps"] = w % 5, T = 12.  every in {2, 3}: with the
counters at w % 5, 40 % (every 2) or 60 % (every 3) of the walkers enter the call inside a hold and take their action
and running reward from `held`, which is drawn here (held_of) so that a kernel that ignored it cannot pass.

The reference is Oracle (auto-reset off) or test_gpu_autoreset._Composed (on) driven by forward_numpy /
stochastic_forward_numpy on its own rows, with the hold spelled out on the host: decided = hold_decide_numpy(the counters
at the start of the step), action = decided ? the policy's : the one in force, hr = decided ? reward : RN32(hr + reward).

COVER_ON / COVER_OFF are the instance axis (policy_cases.COVER's ten batches): norm_cases.COVER's policies with noise and
normaliser both on, pg_cases.COVER's with both off.
"""
import functools

import numpy as np

import episode_cases as ec
import norm_cases as nc
import pg_cases as gc
import policy_cases as pc

EVERY = (2, 3)
SEED, STEP_BASE, WALKER_BASE = gc.SEED, gc.STEP_BASE, gc.WALKER_BASE
T_OFF, T_ON, SLOTS = 12, ec.T, ec.SLOTS
STAGGER = ec.MAX_STEPS          # the counters at entry: w % 5 in both modes
SENTINEL = np.float32(-12345.0)  # raw / eps rows of the walkers that do not decide


class HoldCase:
    def __init__(self, name, src, mod, t_off=T_OFF, norm=False, noise_ok=True):
        self.name, self.src, self.mod, self.t_off, self.norm, self.noise_ok = name, src, mod, t_off, norm, noise_ok
        self.kind, self.params, self.wpw = src.kind, src.params, src.wpw
        self.base = getattr(src, "base", src.name)      # the policy_cases case episode_cases.config takes
        self.C, self.G = src.C, src.G

    def policy(self, device=None, norm=None):
        if self.mod is nc:
            return nc.policy_of(self.src, device, norm=self.norm if norm is None else norm)
        return gc.policy_of(self.src, device) if self.mod is gc else pc.policy_of(self.src, device)

    def sigma(self):
        if self.mod is gc:
            return gc.sigma_of(self.src.name)
        if self.mod is nc:
            return nc.sigma_of(self.src.name)
        s = np.random.default_rng(4000 + self.src.seed).uniform(0.5, 1.5, (self.G, self.C)) * 0.3
        return s.astype(np.float32)

    def __repr__(self):
        return self.name


CASES = [HoldCase(n, gc.case_of(n), gc) for n in ("canonical4-h5-5sets", "balance-h5-4sets", "balance16-h0-perwalker",
                                                  "six-h5-c6-shared")]
CASES.append(HoldCase("discrete-mlp-4sets-c5", pc.case_of("discrete-mlp-4sets-c5"), pc))
CASES.append(HoldCase("norm-canonical4-mlp-5sets", nc.case_of("canonical4-mlp-5sets"), nc, norm=True))
NAMES = [c.name for c in CASES]
COVER_ON = [HoldCase("on-" + c.name, c, nc, t_off=4, norm=True) for c in nc.COVER]
COVER_OFF = [HoldCase("off-" + c.name, c, gc, t_off=4) for c in gc.COVER]
COVER_NAMES = [c.name for c in pc.COVER]
MAIN = "canonical4-h5-5sets"     # the case the single-case tests use: 4 walkers per wave, a set boundary inside a tile


def case_of(name):
    return next(c for c in CASES + COVER_ON + COVER_OFF if c.name == name)


@functools.lru_cache(maxsize=None)
def spec_off(name):
    """Auto-reset off: the case's batch with the counters staggered by w % 5."""
    spec = dict(pc.spec_of(case_of(name).kind))
    N = len(spec["mass_off"]) - 1
    spec["steps"] = (np.arange(N) % STAGGER).astype(np.int32)
    return spec


def config(name):
    """Auto-reset on: episode_cases.config of the case's base (spec, params, pool, N, sunk)."""
    return ec.config(case_of(name).base)


def n_walkers(name):
    return len(pc.spec_of(case_of(name).kind)["mass_off"]) - 1


@functools.lru_cache(maxsize=None)
def held_of(name):
    """The `held` rows a call starts from, [N, C + 1]: actions in [-1, 1], running rewards in [-2, 2].  With discrete
    actions (action_mode 1 reads `a != 0`, and the policy's outputs are practically never zero) half of the held actions
    are +0.0: there a hold shows only where the action in force is zero and a fresh one would not be."""
    case = case_of(name)
    rng = np.random.default_rng(77)
    h = rng.uniform(-1, 1, (n_walkers(name), case.C + 1)).astype(np.float32)
    h[:, -1] *= 2
    if case.params.get("action_mode") == 1:
        h[:, :-1] *= rng.integers(0, 2, (h.shape[0], case.C)).astype(np.float32)
    h.setflags(write=False)
    return h


def _freeze(res):
    for v in res.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def reference(name, auto_reset, noise, every, Tn=None, zero_held=False):
    """The per-step loop of the contract on the CPU.  Every step's obs / reward / done / steps / action / raw / eps /
    decided / hold_reward (and reset / final_obs), the final `held`, the final state, and returns / lengths or the
    episode stats.  raw / eps hold SENTINEL where the walker did not decide.  Computed once per argument tuple, shared,
    never modified."""
    from oracle.oracle import Oracle
    from test_gpu_autoreset import _Composed
    from walker_gym_amd import pg
    case = case_of(name)
    pol, sigma = case.policy(), case.sigma()
    if auto_reset:
        cfg = config(name)
        ref = _Composed(cfg["spec"], cfg["params"], 1, cfg["pool"])
        orc = ref.orc
        Tn = T_ON if Tn is None else Tn
    else:
        ref = orc = Oracle(spec_off(name), case.params, n_threads=8)
        Tn = case.t_off if Tn is None else Tn
    N, Cc = orc.N, case.C
    h0 = np.zeros((N, Cc + 1), np.float32) if zero_held else held_of(name)
    act, hr = h0[:, :Cc].copy(), h0[:, Cc].copy()
    obs = orc.observe()["obs"]
    keys = ("obs", "reward", "done", "steps_t", "action", "raw", "eps", "decided", "hold_reward", "reset", "final_obs")
    out = {k: [] for k in keys}
    for t in range(Tn):
        dec = pg.hold_decide_numpy(orc.steps, every)
        if noise:
            u, a, e = pg.stochastic_forward_numpy(pol, obs, sigma, SEED, STEP_BASE + t, walker_base=WALKER_BASE)
        else:
            a = pol.forward_numpy(obs)
            u = e = np.zeros_like(a)
        on = dec[:, None] != 0
        act = np.where(on, a, act).astype(np.float32)
        r = ref.step(act)
        obs = r["obs"]
        rew = np.asarray(r["reward"], np.float32)
        with np.errstate(all="ignore"):
            hr = np.where(dec != 0, rew, (hr + rew).astype(np.float32)).astype(np.float32)
        out["obs"].append(obs.copy()); out["reward"].append(rew.copy())
        out["done"].append(np.asarray(r["done"]).astype(np.uint8))
        out["steps_t"].append(np.asarray(r["steps_out"] if auto_reset else orc.steps).astype(np.int32).copy())
        out["action"].append(act.copy())
        out["raw"].append(np.where(on, u, SENTINEL).astype(np.float32))
        out["eps"].append(np.where(on, e, SENTINEL).astype(np.float32))
        out["decided"].append(dec.copy()); out["hold_reward"].append(hr.copy())
        if auto_reset:
            out["reset"].append(r["reset"].copy())
            fo = np.full_like(obs, np.nan)   # final_obs: a step writes the rows of the walkers it resets only
            sel = r["reset"] != 0
            fo[sel] = ref.final_obs[sel]
            out["final_obs"].append(fo)
    res = {k: np.stack(v) for k, v in out.items() if v}
    res["held"] = np.concatenate([act, hr[:, None]], axis=1).astype(np.float32)
    if auto_reset:
        res["state"] = ref.state()
        res["stats"] = ec.accounting(res["reward"], res["reset"], SLOTS)
    else:
        res["state"] = dict(pos=orc.pos.copy(), vel=orc.vel.copy(), acc=orc.acc.copy(), mx=orc.mx.copy(),
                            steps=orc.steps.copy(), contact=orc.contact.copy())
        ret, ln = pc.returns_lengths(res["reward"], res["done"])
        res["stats"] = dict(returns=ret, lengths=ln)
    return _freeze(res)


def closed_holds(decided, every):
    """Counts of the holds of a [T, N] decided array that begin with a decision of the call and are closed by the next
    one inside it, by length 1 .. every."""
    Tn, N = decided.shape
    counts = np.zeros(every + 1, np.int64)
    for w in range(N):
        at = np.flatnonzero(decided[:, w])
        for n in np.diff(at):
            counts[n] += 1
    return counts[1:]


def mixed_tile_steps(decided, wpw):
    """The share of (step, wave tile) pairs in which a deciding and a holding walker stand side by side."""
    Tn, N = decided.shape
    n_tiles = (N + wpw - 1) // wpw
    some = np.zeros((Tn, n_tiles), bool)
    none = np.zeros((Tn, n_tiles), bool)
    for k in range(wpw):
        col = decided[:, k::wpw] != 0
        some[:, :col.shape[1]] |= col
        none[:, :col.shape[1]] |= ~col
    return float((some & none).mean())

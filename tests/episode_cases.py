"""The batches, policies and references that the multi-episode rollout tests share (tests/test_rollout_episodes_cpu.py
checks on the CPU that every case resets often enough to mean something, tests/test_gpu_rollout_episodes.py compares
bits on the GPU).

Each case is a policy_cases case (its batch, its policy) with episodes made short: max_steps = 5, the walkers' step
counters staggered by w % 5, about 1 % of the walkers (at least two) sunk to mean y = -80 so that they end an episode
at every step (as test_gpu_autoreset._config does, default_rng(11)), and a two-row reset-noise pool.  T = 16.

  canonical4-mlp-5sets             N = 2,050: 4 walkers per wave, NE 3, 8-byte records (and 16-byte with WG_EDGE8=0), a
                                   half-full last tile, a parameter-set boundary inside a tile
  canonical4-lin-perwalker-c5-inf  the same batch, a linear policy per walker, 5 of 8 muscles act, no clip
  balance16-mid-mlp-8sets          N = 8,200: 16 walkers per wave
  balance-g1-lin-4sets-inf         N = 100: the NE = 1 instance
  canonical-lin-shared             N = 1,000: one walker per wave
  wide-mlp-shared                  M = 64
  discrete-mlp-4sets-c5            action_mode 1

The reference is test_gpu_autoreset._Composed (Oracle.step + the reset spelled out on the host) driven by
policy.forward_numpy on its own observation rows, starting from Oracle.observe()."""
import functools

import numpy as np

import policy_cases as pc

T = 16
MAX_STEPS = 5
SLOTS = 4      # fewer than the sunk walkers' 16 episodes
NAMES = ["canonical4-mlp-5sets", "canonical4-lin-perwalker-c5-inf", "balance16-mid-mlp-8sets",
         "balance-g1-lin-4sets-inf", "canonical-lin-shared", "wide-mlp-shared", "discrete-mlp-4sets-c5"]


COVER_NAMES = [c.name for c in pc.COVER]   # instance coverage: every (IN3D, NE, E8) of the AR policy kernel
# policy shapes through the AR instance (its eight-word walker record holds the parameter set at another stride): M = 16
# at H = 33 with a set boundary inside a tile and at H = 40 shared, M = 4 at H = 9 with 16 walkers per wave, and the six
# action columns on four lanes
SHAPE_NAMES = [pc.shape("m16", 33, G=5).name, pc.shape("m16", 40).name, pc.shape("m4", 9).name,
               pc.shape("six", 9, C=6).name]


def case_of(name):
    return pc.case_of(name)


@functools.lru_cache(maxsize=None)
def config(name):
    """One case's inputs: spec (staggered counters, sunk walkers), params, the noise pool, the sunk walkers."""
    case = case_of(name)
    spec = dict(pc.spec_of(case.kind))
    mo = np.asarray(spec["mass_off"])
    N = len(mo) - 1
    rng = np.random.default_rng(11)
    pos = np.array(spec["pos"], np.float32).reshape(-1, 3).copy()
    sunk = rng.permutation(N)[:max(2, N // 100)]
    for w in sunk:
        a, b = mo[w], mo[w + 1]
        pos[a:b, 1] += np.float32(-80.0) - pos[a:b, 1].mean()
    spec["pos"] = pos
    spec["steps"] = (np.arange(N) % MAX_STEPS).astype(np.int32)
    pool = (rng.standard_normal((2, len(pos), 3)) * 0.5).astype(np.float32)
    params = dict(case.params, max_steps=MAX_STEPS)
    return dict(case=case, spec=spec, params=params, pool=pool, N=N, sunk=sunk)


def accounting(reward, reset, slots):
    """wg_episode_stats restated: [T, N] float32 rewards and reset flags -> the arrays of one call."""
    Tn, N = reward.shape
    cur, sm = np.zeros(N, np.float32), np.zeros(N, np.float32)
    ln, n, lsum = np.zeros(N, np.int32), np.zeros(N, np.int32), np.zeros(N, np.int32)
    ep_ret = np.full((N, max(slots, 1)), np.nan, np.float32)
    ep_len = np.full((N, max(slots, 1)), -1, np.int32)
    with np.errstate(all="ignore"):
        for t in range(Tn):
            cur = (cur + reward[t].astype(np.float32)).astype(np.float32)
            ln = ln + 1
            sel = reset[t] != 0
            w = np.flatnonzero(sel & (n < slots))
            ep_ret[w, n[w]] = cur[w]
            ep_len[w, n[w]] = ln[w]
            sm = np.where(sel, (sm + cur).astype(np.float32), sm)
            lsum = np.where(sel, lsum + ln, lsum)
            n = n + sel.astype(np.int32)
            cur = np.where(sel, np.float32(0.0), cur)
            ln = np.where(sel, 0, ln)
    res = dict(return_sum=sm, length_sum=lsum, episodes=n, tail_return=cur, tail_length=ln)
    if slots > 0:
        res.update(ep_returns=ep_ret[:, :slots], ep_lengths=ep_len[:, :slots])
    return res


@functools.lru_cache(maxsize=None)
def reference(name):
    """The composed closed loop on the CPU: every step's action / obs / reward / done / reset / final_obs, the episode
    counts before each step, the final state and the accounting.  Computed once, shared, never modified."""
    from test_gpu_autoreset import _Composed
    cfg = config(name)
    pol = pc.policy_of(cfg["case"])
    ref = _Composed(cfg["spec"], cfg["params"], 1, cfg["pool"])
    obs = ref.orc.observe()["obs"]
    out = dict(action=[], obs=[], reward=[], done=[], reset=[], final_obs=[], ep_before=[], pos=[], vel=[], acc=[])
    for t in range(T):
        a = pol.forward_numpy(obs)
        out["ep_before"].append(ref.episodes.copy())
        r = ref.step(a)
        obs = r["obs"]
        out["action"].append(a); out["obs"].append(obs.copy()); out["reward"].append(r["reward"].copy())
        out["done"].append(np.asarray(r["done"]).astype(np.uint8)); out["reset"].append(r["reset"].copy())
        # final_obs: a step writes the rows of the walkers it resets only
        fo = np.full_like(obs, np.nan)
        sel = r["reset"] != 0
        fo[sel] = ref.final_obs[sel]
        out["final_obs"].append(fo)
        out["pos"].append(ref.orc.pos.copy()); out["vel"].append(ref.orc.vel.copy()); out["acc"].append(ref.orc.acc.copy())
    res = {k: np.stack(v) for k, v in out.items()}
    res["state"] = ref.state()
    res["stats"] = accounting(res["reward"], res["reset"], SLOTS)
    for v in res.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return res

"""Non-default parameters and diverged walkers on the ON, HOLD and DEEP instances of walker_rollout_policy: the cells and
the references that tests/test_feature_cases_cpu.py (the reference alone) and tests/test_gpu_feature_instances.py (bit for
bit on the GPU) share.  No GPU import here.

A cell is (batch, condition, form, auto-reset):
  batch      one of policy_cases.COVER's ten (512 full standard tiles, one per (IN3D, NE))
  condition  scaled-run2, scaled-run2-discrete   param_cases.policy_config (observation scales, run2, pins; action_mode 1)
             diverged                            diverged_cases.policy_config (at least 20 dead walkers and 10 of every
                                                 other kind, placed by position in the wave tile)
  form       on      rollout_policy / rollout_episodes, the shared linear policy of norm_cases.COVER (H = 0: a NaN row
                     reaches the action), the normaliser: the ON instances, NZ = 0
             on-nz   rollout_stochastic, the same with the noise: the ON instances, NZ = 1
             hold    rollout_held, every = 2, the same policy, noise and normaliser, a drawn finite `held` at entry: HOLD
             deep    rollout_held, every = 3, deep_cases.cover_policy (6, 5) with the normaliser, the noise: DEEP
T = 4 without auto-reset, 8 with it (the sunk walkers, max_steps = 5, the counters at w % 5 and the pool, as the builders
make them).  The hold and deep forms stagger the counters by w % 5 without auto-reset too (hold_cases.spec_off's idea), or
every walker would decide at the same steps.

The normaliser's statistics are the batch's own under the condition and the mode: obs_moments_numpy over the entry rows
and every step's rows of the `on` form's reference WITHOUT a normaliser (the linear policy on the raw rows), with
bound = BOUND, so that the rows of dead and exploded walkers drop out; clip = norm_cases.CLIP.

Every reference is deep_cases.contract_loop, under np.errstate(all="ignore").  The `off` arguments of loop() switch one
thing off (the normaliser, the hold, the middle layer, the condition's parameters): what the CPU test compares a cell
with.  The results are large (obs and final_obs are [T, N, D]), so the cache is bounded: it serves the launches of one GPU
case and the forms of one (batch, condition, mode), which cells() puts side by side, within one test function.  Each
test function of the CPU file walks the cells once more and computes its references again (a reference takes a few
tenths of a second); the statistics, which are small, are kept for the whole session.
"""
import functools

import numpy as np

import deep_cases as dc
import diverged_cases as D
import episode_cases as ec
import norm_cases as nc
import param_cases as P
import policy_cases as pc

f32 = np.float32
BATCHES = [c.name for c in pc.COVER]
PARAM_CONDITIONS = tuple(v.name for v in P.POLICY_VARIANTS)
CONDITIONS = PARAM_CONDITIONS + ("diverged",)
FORMS = {"on": dict(noise=False, every=1, deep=False, held=False),
         "on-nz": dict(noise=True, every=1, deep=False, held=False),
         "hold": dict(noise=True, every=2, deep=False, held=True),
         "deep": dict(noise=True, every=3, deep=True, held=True)}
T = {False: 4, True: 8}
STAND_IN = ("ne1-2d", "ne1-3d")     # the batches whose instances carry the stand-in path: T = 1 as well under `diverged`
BOUND = 1.0e6                       # the statistics leave out a row with an |x| >= BOUND (or a NaN)
STAGGER = ec.MAX_STEPS
SEED, STEP_BASE, WALKER_BASE, SLOTS, SENTINEL = dc.SEED, dc.STEP_BASE, dc.WALKER_BASE, dc.SLOTS, dc.SENTINEL
MODES = ((False, "off"), (True, "ar"))


def cells():
    """Every (batch, condition, form, auto_reset), the forms of one (batch, condition, mode) side by side."""
    return [(b, c, f, ar) for b in BATCHES for c in CONDITIONS for ar, _ in MODES for f in FORMS]


def cell_id(cell):
    b, c, f, ar = cell
    return f"{b}-{c}-{f}-{'ar' if ar else 'off'}"


def steps_of(cell):
    """The step counts a cell runs at."""
    b, c, f, ar = cell
    return (T[ar],) + ((1,) if c == "diverged" and b in STAND_IN else ())


# ---------------------------------------------------------------- inputs
def config(batch, condition, form, auto_reset, default=False):
    """The cell's spec, params, pool (and kinds under `diverged`): fresh arrays.  default: the same spec under the
    default parameters (the parameter conditions only)."""
    if condition == "diverged":
        cfg = D.policy_config(batch, auto_reset)
    else:
        cfg = P.policy_config(batch, condition, auto_reset)
        cfg["N"] = len(cfg["spec"]["mass_off"]) - 1
        if default:
            keep = dict(cfg["case"].params)
            if auto_reset:
                keep["max_steps"] = cfg["params"]["max_steps"]
            cfg["params"] = keep
    if FORMS[form]["held"] and not auto_reset:
        cfg["spec"]["steps"] = (np.arange(cfg["N"]) % STAGGER).astype(np.int32)
    return cfg


def linear_weights(batch):
    """norm_cases.COVER's shared linear policy of the batch: (w2, b2, w1, b1) and its act_limit."""
    case = nc.case_of(batch)
    return pc.weights(case.pol), case.L


def _tensor(a, device):
    """A host array or tensor (or None) as a tensor on `device` (None: the host)."""
    import torch
    if a is None:
        return None
    t = a if torch.is_tensor(a) else torch.from_numpy(np.array(a))
    return t if device is None else t.to(device)


@functools.lru_cache(maxsize=None)
def entry_rows(batch, condition, auto_reset):
    from oracle.oracle import Oracle
    cfg = config(batch, condition, "on", auto_reset)
    with np.errstate(all="ignore"):
        rows = Oracle(cfg["spec"], cfg["params"], n_threads=8).observe()["obs"].copy()
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def stats_of(batch, condition, auto_reset):
    """(state, mean, scale, rows used, rows) of the cell's un-normalised reference rollout."""
    from walker_gym_amd.normalize import obs_moments_numpy, obs_norm_finish_numpy
    ref = loop(batch, condition, "on", auto_reset, off="norm")
    rows = np.concatenate([entry_rows(batch, condition, auto_reset)[None], ref["obs"]])
    st = obs_moments_numpy(rows, bound=BOUND, chunk_rows=256)
    mean, scale = obs_norm_finish_numpy(st, nc.EPS)
    for a in (st, mean, scale):
        a.setflags(write=False)
    return st, mean, scale, int(st[0]), rows.shape[0] * rows.shape[1]


def obs_norm_of(batch, condition, auto_reset, device="cpu"):
    import torch
    from walker_gym_amd.normalize import ObsNorm
    st, mean, scale, _, _ = stats_of(batch, condition, auto_reset)
    nm = ObsNorm(len(mean), device, clip=nc.CLIP, eps=nc.EPS, bound=BOUND)
    nm.load_state_dict(dict(nm.state_dict(), state=torch.from_numpy(st.copy()), mean=torch.from_numpy(mean.copy()),
                            scale=torch.from_numpy(scale.copy())))
    return nm


def policy_of(batch, condition, form, auto_reset, device=None, norm=True, shallow=False):
    """The cell's MLPPolicy.  norm=False: the same weights on the raw rows; shallow: the linear policy in a deep cell."""
    from walker_gym_amd.policy import MLPPolicy
    nm = obs_norm_of(batch, condition, auto_reset, "cpu" if device is None else device) if norm else None
    if FORMS[form]["deep"] and not shallow:
        p = dc.cover_policy(batch)
        mv = lambda t: _tensor(t, device)
        return MLPPolicy(mv(p.w2), mv(p.b2), mv(p.w1), mv(p.b1), act_limit=p.act_limit, obs_norm=nm, wm=mv(p.wm),
                         bm=mv(p.bm))
    (w2, b2, w1, b1), L = linear_weights(batch)
    return MLPPolicy(_tensor(w2, device), _tensor(b2, device), _tensor(w1, device), _tensor(b1, device), act_limit=L,
                     obs_norm=nm)


def sigma_of(batch, form):
    """float32 [1, C]: norm_cases' per unit for the linear policy, deep_cases.cover_sigma for the deep one."""
    return np.array(dc.cover_sigma(batch) if FORMS[form]["deep"] else nc.sigma_of(batch), f32)


@functools.lru_cache(maxsize=None)
def held_of(batch, condition):
    """The `held` rows a hold or deep cell starts from, [N, C + 1]: drawn and finite (actions in [-1, 1], running rewards
    in [-2, 2]), so that a kernel that ignored them cannot pass.  With discrete actions half of the held actions are +0.0
    (hold_cases.held_of's reason: action_mode 1 reads `a != 0`, and a fresh action is practically never zero)."""
    case = pc.case_of(batch)
    N = len(pc.spec_of(case.kind)["mass_off"]) - 1
    rng = np.random.default_rng(77)
    h = rng.uniform(-1, 1, (N, case.C + 1)).astype(f32)
    h[:, -1] *= 2
    if condition == "scaled-run2-discrete":
        h[:, :-1] *= rng.integers(0, 2, (N, case.C)).astype(f32)
    h.setflags(write=False)
    return h


# ---------------------------------------------------------------- references
OFF = (None, "norm", "hold", "deep", "params")


@functools.lru_cache(maxsize=12)
def loop(batch, condition, form, auto_reset, Tn=None, off=None):
    """deep_cases.contract_loop of a cell over Tn steps (T[auto_reset] by default): frozen arrays, never modified.
    off: None (the cell itself), or the cell with one thing switched off: 'norm' no normaliser, 'hold' every = 1, 'deep'
    the linear policy in place of the deep one, 'params' the default parameters on the same spec."""
    assert off in OFF
    f = FORMS[form]
    cfg = config(batch, condition, form, auto_reset, default=off == "params")
    pol = policy_of(batch, condition, form, auto_reset, norm=off != "norm", shallow=off == "deep")
    every = 1 if off == "hold" else f["every"]
    h0 = held_of(batch, condition) if f["held"] else np.zeros((cfg["N"], pol.C + 1), f32)
    sigma = sigma_of(batch, "hold" if off == "deep" else form)
    with np.errstate(all="ignore"):
        return dc.contract_loop(cfg, pol, sigma, auto_reset, f["noise"], every, T[auto_reset] if Tn is None else Tn, h0)


def reference(cell, Tn=None):
    return loop(*cell, Tn=Tn)


def normalised_inputs(batch, condition, form, auto_reset, ref):
    """The rows the policy saw, normalised: [T, N, D] (the entry rows, then the stored rows of every step but the last)."""
    pol = policy_of(batch, condition, form, auto_reset)
    rows = np.concatenate([entry_rows(batch, condition, auto_reset)[None], ref["obs"][:-1]])
    return pol.obs_norm.normalize_numpy(rows)

"""Non-default parameters and diverged walkers on every ON, HOLD and DEEP instance of walker_rollout_policy
(tests/feature_cases.py: the cells; tests/test_feature_cases_cpu.py holds on the reference alone that each means
something).  One case per (batch, condition, form, mode), two launches in each (the compact records and WG_EDGE8=0), and
on the stand-in batches under `diverged` two more of one step (the kernel stores contact after its last step only).

Everything is compared with the per-step loop of the contract on the CPU (deep_cases.contract_loop) bit for bit: float
arrays as uint32 views, a NaN equal to a NaN whatever its payload; everything that is no float exactly.  Which instance a
launch takes is the host's arithmetic: every launch asserts the walkers per wave through launch_geometry() and that the
compact records exist; the entry and the policy select the family (rollout_policy / rollout_episodes and
rollout_stochastic with a normaliser: ON; rollout_held with a one-layer policy: HOLD; with a middle layer: DEEP)."""
import numpy as np
import pytest

import feature_cases as F
import policy_cases as pc
from conftest import gpu_available
from test_gpu_deep_rollout import _KEYS, _mode_buffers
from test_gpu_edge8 import STATE, _bits, _state

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.skip("no ROCm GPU")


def _same(got, ref, what):
    """Bit for bit, NaN == NaN in float arrays; everything else exactly, the dtype included."""
    got, ref = np.asarray(got), np.asarray(ref)
    if got.dtype == np.float32:
        assert ref.dtype == np.float32, what
        _bits(got, ref, what, nan_ok=True)
    else:
        assert got.size == ref.size and np.array_equal(got.ravel().astype(np.int64), ref.ravel().astype(np.int64)), what


def _env(cfg, case, auto_reset):
    from walker_gym_amd.batched_env import BatchedPhysicsEnv
    env = BatchedPhysicsEnv(cfg["spec"], device=DEV, **cfg["params"])
    if auto_reset:
        env.enable_auto_reset(on=("done",), noise=cfg["pool"], final_obs=True)   # (not "nonfinite": the dead stay dead)
    geo = env.launch_geometry()
    assert geo["walkers_per_block"] * 64 // geo["threads"] == case.wpw, geo
    assert env.batch.edges8 is not None
    return env


def _launch(env, cell, pol, Tn):
    """One call of the public method the form belongs to, every buffer it has pre-filled (NaN, 255, the sentinel in the
    raw / eps rows)."""
    import torch
    batch, cond, form, ar = cell
    f, Cc = F.FORMS[form], pol.C
    buf = _mode_buffers(env, Tn, Cc, ar, f["noise"], f["held"])
    kw = dict(episode_slots=F.SLOTS) if ar else {}
    sigma = torch.from_numpy(F.sigma_of(batch, form)).to(DEV)
    if f["held"]:
        held = torch.from_numpy(F.held_of(batch, cond).copy()).to(DEV)
        res = env.rollout_held(pol, Tn, f["every"], sigma=sigma, seed=F.SEED, step_base=F.STEP_BASE,
                               walker_base=F.WALKER_BASE, held=held, **buf, **kw)
    elif f["noise"]:
        res = env.rollout_stochastic(pol, Tn, sigma, F.SEED, step_base=F.STEP_BASE, walker_base=F.WALKER_BASE, **buf, **kw)
    elif ar:
        res = env.rollout_episodes(pol, Tn, **buf, **kw)
    else:
        res = env.rollout_policy(pol, Tn, **buf)
    torch.cuda.synchronize()
    out = {_KEYS[k]: v.cpu().numpy() for k, v in buf.items()}
    out.update(_state(env))
    if ar:
        out["episodes"] = env.batch.episodes.detach().cpu().numpy().copy()
    res = dict(res)
    if "held" in res:
        out["held"] = res.pop("held").cpu().numpy()
    out["stats"] = {k: v.cpu().numpy() for k, v in res.items()}
    return out


def _check(got, ref, cell, what):
    batch, cond, form, ar = cell
    f = F.FORMS[form]
    step = ["obs", "reward", "done", "action"] + (["steps_t"] if f["noise"] or f["held"] else []) + \
        (["raw", "eps"] if f["noise"] else []) + (["decided", "hold_reward"] if f["held"] else []) + \
        (["reset", "final_obs"] if ar else [])
    assert set(step) == set(got) - set(STATE) - {"stats", "held", "episodes"}, sorted(got)
    for k in step:
        assert got[k].dtype == ref[k].dtype, k
        _same(got[k], ref[k], f"{k} {what}")
    if f["held"]:
        _same(got["held"], ref["held"], f"held {what}")
    st = ref["state"]
    for k, r in (("pos", "pos"), ("vel", "vel"), ("acc", "acc"), ("muscle_x", "mx")):
        _same(got[k], np.asarray(st[r], np.float32), f"{k} after the rollout {what}")
    for k in ("steps", "contact") + (("episodes",) if ar else ()):
        _same(got[k], st[k], f"{k} after the rollout {what}")
    assert set(got["stats"]) == set(ref["stats"]), (sorted(got["stats"]), sorted(ref["stats"]))
    for k, v in got["stats"].items():
        assert v.dtype == ref["stats"][k].dtype, k
        _same(v, ref["stats"][k], f"stats {k} {what}")


@pytest.mark.parametrize("cell", F.cells(), ids=F.cell_id)
def test_cell(monkeypatch, cell):
    """Every per-step array the entry has (obs: the stored rows stay raw; reward, done, action, raw, eps, steps, decided,
    hold_reward, reset, final_obs), `held`, the final state (pos, vel, acc, muscle_x, steps, contact, episodes) and the
    call's stats, with the compact records and under WG_EDGE8=0."""
    batch, cond, form, ar = cell
    case = pc.case_of(batch)
    cfg = F.config(*cell)
    pol = F.policy_of(batch, cond, form, ar, DEV)
    for Tn in F.steps_of(cell):
        ref = F.reference(cell) if Tn == F.T[ar] else F.reference(cell, Tn=Tn)
        for edge8 in ("1", "0"):
            monkeypatch.setenv("WG_EDGE8", edge8)
            env = _env(cfg, case, ar)
            got = _launch(env, cell, pol, Tn)
            monkeypatch.delenv("WG_EDGE8")
            _check(got, ref, cell, f"(T = {Tn}, WG_EDGE8={edge8})")


@pytest.mark.parametrize("auto_reset", [False, True], ids=["off", "ar"])
@pytest.mark.parametrize("batch", ["ne1-2d", "ne3-3d"])
def test_moments_over_rows_the_kernels_produced(batch, auto_reset):
    """wg_obs_moments over the rows of the un-normalised rollout of the `diverged` batch as the GPU wrote them (the entry
    rows and every step's), NaN walkers at their real positions, with the cells' bound: the state, mean and scale of
    obs_moments_numpy / obs_norm_finish_numpy over the same rows, which are the cells' statistics.  ne1-2d: D = 26, 16
    walkers per wave; ne3-3d: D = 584 (more than one column per thread), the dead-z walkers."""
    import torch
    from walker_gym_amd.normalize import ObsNorm, obs_moments_numpy, obs_norm_finish_numpy
    import norm_cases as nc
    cell = (batch, "diverged", "on", auto_reset)
    case, Tn = pc.case_of(batch), F.T[auto_reset]
    cfg = F.config(*cell)
    assert ("dead-z" in cfg["kinds"]) == (case.params["in3d"] == 1)       # (the kind that exists at IN3D 1 only)
    env = _env(cfg, case, auto_reset)
    env.observe()
    entry = env.obs.detach().clone()
    pol = F.policy_of(*cell, device=DEV, norm=False)
    obs = torch.full((Tn, env.N, env.obs_dim), float("nan"), device=DEV)
    (env.rollout_episodes if auto_reset else env.rollout_policy)(pol, Tn, obs_out=obs)
    rows = torch.cat([entry[None], obs]).contiguous()
    host = rows.cpu().numpy()
    ref = F.loop(batch, "diverged", "on", auto_reset, off="norm")
    _same(host, np.concatenate([F.entry_rows(batch, "diverged", auto_reset)[None], ref["obs"]]), "rows")
    assert np.isnan(host).any() and np.isfinite(host).any()
    nm = ObsNorm(env.obs_dim, DEV, clip=nc.CLIP, eps=nc.EPS, bound=F.BOUND)
    nm.update(rows, chunk_rows=256)
    torch.cuda.synchronize()
    st = obs_moments_numpy(host, bound=F.BOUND, chunk_rows=256)
    mean, scale = obs_norm_finish_numpy(st, nc.EPS)
    want = F.stats_of(batch, "diverged", auto_reset)
    assert 0 < st[0] < host.shape[0] * host.shape[1]          # some rows dropped out, not all
    for got, a, b, k in ((nm.state, st, want[0], "state"), (nm.mean, mean, want[1], "mean"), (nm.scale, scale, want[2], "scale")):
        g = got.cpu().numpy()
        assert g.dtype == a.dtype == b.dtype, k
        assert np.array_equal(g.view(np.uint8), a.view(np.uint8)) and np.array_equal(g.view(np.uint8), b.view(np.uint8)), k

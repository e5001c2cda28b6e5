"""Non-default parameters on every (IN3D, NE, E8, AR / FIX / WT) instance of the lean step kernels, the resident
rollout and the policy rollout (tests/param_cases.py: the shapes and the variants; tests/test_param_cases_cpu.py holds
that each cell moves what it should and stays finite).  Everything is bit for bit against the C oracle (rtol = atol = 0,
uint32 views); a NaN equals a NaN, whatever its payload, only under the pair variants, whose close opposite charges blow
some walkers up in the reference's own arithmetic.

Which instance a launch takes is the host's arithmetic: each test asserts the walkers per wave, the pass count and the
record format against launch_geometry(), and the FIX / WT launch counters around every call."""
import numpy as np
import pytest

import episode_cases as ec
import param_cases as P
import policy_cases as pc
from conftest import gpu_available
from test_gpu_edge8 import STATE, _bits, _compact, _state, _step_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.skip("no ROCm GPU")


def _counters():
    from walker_gym_amd import _lib
    lib = _lib.load()
    return np.array([lib.wg_fix_launches(), lib.wg_wt_launches()])


def _assert_instance(env, shape):
    """The launch of the whole batch takes the instance the shape is there for."""
    kw = P.SHAPES[shape]
    sel = P.select(kw["N"], kw["M"], kw["K"])
    geo = env.launch_geometry()
    wpw = geo["walkers_per_block"] // (geo["threads"] // 64)
    assert wpw == sel["wpw"], geo
    assert (wpw * env.batch.K + 63) // 64 == sel["passes"]
    assert env.batch.edges8 is not None and _compact(env) == sel["compact"]
    return sel


def _expected(shape, in3d, v, n):
    """The FIX / WT launches of n whole-batch launches under the variant."""
    kw = P.SHAPES[shape]
    return n * np.array([P.fix_expected(kw["N"], kw["M"], kw["K"], v.fix),
                         P.wt_expected(kw["N"], kw["M"], kw["K"], kw["A"], in3d, v.fix)], int)


def _finite(*dicts):
    for d in dicts:
        for k, a in d.items():
            if np.asarray(a).dtype == np.float32:
                assert np.isfinite(a).all(), f"{k}: not finite"


@pytest.mark.parametrize("cell", P.step_cells(), ids=P.cell_id)
def test_step(monkeypatch, cell):
    """Two closed-loop step()s on the default path and under WG_EDGE8=0, then one run() of three steps over two walker
    ranges (the keep_aux flip), each against the oracle."""
    import torch
    from walker_gym_amd.batched_env import BatchedPhysicsEnv
    shape, in3d, name = cell
    v, kw = P.variant(name), P.SHAPES[shape]
    spec, params = P.spec_of(shape, name), v.params(shape, in3d)
    acts = P.actions(shape, name, P.RUN_STEPS)
    sel = P.select(kw["N"], kw["M"], kw["K"])

    c0 = _counters()
    env = _step_case(monkeypatch, spec, params, P.STEPS, sel["compact"], acts=acts, nan_ok=v.pairs)
    _assert_instance(env, shape)
    assert env._step_lanes() == 1
    c1 = _counters()
    assert (c1 - c0 == _expected(shape, in3d, v, P.STEPS)).all(), (c1 - c0, "FIX / WT launches of the steps")
    if not v.pairs:
        _finite(_state(env))

    # run(): every range is a batch of its own to the selector
    ref = P.scripted(shape, in3d, name)["steps"][-1]
    ranges = P.run_ranges(kw["N"])
    runner = BatchedPhysicsEnv(spec, **params)
    assert runner._lanes(2) == len(ranges)
    runner.run(torch.as_tensor(acts, device="cuda"), P.RUN_STEPS, lanes=2)
    st = _state(runner)
    c2 = _counters()
    want = sum(P.RUN_STEPS * np.array([P.fix_expected(n, kw["M"], kw["K"], v.fix),
                                       P.wt_expected(n, kw["M"], kw["K"], kw["A"], in3d, v.fix)], int) for n in ranges)
    assert (c2 - c1 == want).all(), (c2 - c1, "FIX / WT launches of run()")
    for k in STATE:
        _bits(st[k], ref[k], f"{k} after run()", v.pairs and k not in ("steps", "contact"))
    got = dict(obs=runner.obs, reward=runner.reward, done=runner.done, centroid=runner.centroid, energy=runner.energy)
    for k, t in got.items():
        _bits(t.cpu().numpy().astype(ref[k].dtype), ref[k], f"{k} after run()", v.pairs)
    if runner.batch.radius is not None:
        assert np.array_equal(runner.batch.radius.cpu().numpy(), ref["radius"])
    if not v.pairs:
        _finite(st, {k: t.cpu().numpy() for k, t in got.items()})

    if v.fix:   # the control arms: the generic instance, then FIX with its own epilogue; the oracle's bits each time
        for knob, keep in (("WG_FIX", 0), ("WG_WT", 1)):
            monkeypatch.setenv(knob, "0")
            c3 = _counters()
            _step_case(monkeypatch, spec, params, P.STEPS, sel["compact"], acts=acts)
            want = _expected(shape, in3d, v, P.STEPS) * np.array([keep, 0])
            assert (_counters() - c3 == want).all(), f"{knob}=0: FIX / WT launches"
            monkeypatch.delenv(knob)


@pytest.mark.parametrize("cell", P.resident_cells(), ids=P.cell_id)
def test_resident(monkeypatch, cell):
    """rollout(resident=True) of three steps with the compact records and under WG_EDGE8=0."""
    import torch
    from walker_gym_amd.batched_env import BatchedPhysicsEnv
    shape, in3d, name = cell
    v = P.variant(name)
    spec, params = P.spec_of(shape, name), v.params(shape, in3d)
    acts = torch.as_tensor(P.actions(shape, name, P.RUN_STEPS), device="cuda")
    refs = P.scripted(shape, in3d, name)["steps"]
    c0 = _counters()
    for edge8 in ("1", "0"):
        env = BatchedPhysicsEnv(spec, **params)
        _assert_instance(env, shape)
        assert env.resident_ok()
        monkeypatch.setenv("WG_EDGE8", edge8)
        obs, rew, done = env.rollout(acts, resident=True)
        st = _state(env)
        monkeypatch.delenv("WG_EDGE8")
        for t, ref in enumerate(refs):
            _bits(obs[t].cpu().numpy(), ref["obs"], f"step {t} obs (WG_EDGE8={edge8})")
            _bits(rew[t].cpu().numpy(), ref["reward"], f"step {t} reward (WG_EDGE8={edge8})")
            _bits(done[t].cpu().numpy(), ref["done"], f"step {t} done (WG_EDGE8={edge8})")
        for k in STATE:
            _bits(st[k], refs[-1][k], f"{k} after rollout (WG_EDGE8={edge8})")
        _finite(st, dict(obs=obs.cpu().numpy(), reward=rew.cpu().numpy()))
    assert (_counters() == c0).all()   # the resident kernel has no FIX instance


def _ar_env(cfg, shape):
    from walker_gym_amd.batched_env import BatchedPhysicsEnv
    env = BatchedPhysicsEnv(cfg["spec"], **cfg["params"])
    env.enable_auto_reset(on=("done",), noise=cfg["pool"], final_obs=True)
    _assert_instance(env, shape)
    return env


@pytest.mark.parametrize("cell", P.auto_reset_cells(), ids=P.cell_id)
def test_auto_reset(monkeypatch, cell):
    """The AR instances of the step kernel (a step() loop) and of the resident kernel (one rollout) under the variant,
    with the compact records and under WG_EDGE8=0, against the composed oracle."""
    import torch
    from test_gpu_autoreset import _check_outputs, _check_state
    from test_gpu_parity import _close
    shape, in3d, name = cell
    cfg, ref = P.ar_config(shape, in3d, name), P.ar_reference(shape, in3d, name)
    T, N = P.AR_STEPS, cfg["N"]
    resets = np.stack([s["out"]["reset"] for s in ref])
    assert resets.any() and not resets.all()
    c0 = _counters()
    for edge8 in ("1", "0"):
        monkeypatch.setenv("WG_EDGE8", edge8)
        env = _ar_env(cfg, shape)
        for t in range(T):
            env.step(cfg["acts"][t])
            torch.cuda.synchronize()
            _check_state(env, ref[t]["state"])
            _check_outputs(env, ref[t]["out"], ref[t]["state"])
        _finite(_state(env), dict(obs=env.obs.cpu().numpy()))
        env = _ar_env(cfg, shape)
        assert env.resident_ok()
        reset = torch.full((T, N), 7, dtype=torch.uint8, device=env.device)
        obs, rew, done = env.rollout(torch.from_numpy(cfg["acts"]).to(env.device), resident=True, reset_out=reset)
        torch.cuda.synchronize()
        _close(obs.cpu().numpy(), np.stack([s["out"]["obs"] for s in ref]))
        _close(rew.cpu().numpy(), np.stack([s["out"]["reward"] for s in ref]))
        assert np.array_equal(done.cpu().numpy(), np.stack([s["out"]["done"] for s in ref]))
        assert np.array_equal(reset.cpu().numpy(), resets)
        _check_state(env, ref[-1]["state"])
        _finite(_state(env), dict(obs=obs.cpu().numpy()))
        monkeypatch.delenv("WG_EDGE8")
    assert (_counters() == c0).all()   # no AR and FIX instance


@pytest.mark.parametrize("auto_reset", [False, True], ids=["off", "ar"])
@pytest.mark.parametrize("name", [v.name for v in P.POLICY_VARIANTS])
@pytest.mark.parametrize("case", pc.COVER, ids=lambda c: c.name)
def test_policy_rollout(monkeypatch, case, name, auto_reset):
    """walker_rollout_policy at every (IN3D, NE, E8) and its AR twin under the combined variant (observation scales and
    raw positions into the policy, run2, pins; then the same with discrete actions): every step and the final state
    against the reference engine (auto-reset off) or the composed reference (on)."""
    import torch
    from test_gpu_rollout_episodes import _buffers, _check_against_reference, _host
    from test_gpu_rollout_episodes import _state as _ep_state
    from test_gpu_rollout_episodes import _stats
    from walker_gym_amd.batched_env import BatchedPhysicsEnv
    cfg, ref = P.policy_config(case.name, name, auto_reset), P.policy_reference(case.name, name, auto_reset)
    T = P.POLICY_STEPS[auto_reset]
    pol = pc.policy_of(case, "cuda:0")
    for edge8 in ("1", "0"):
        monkeypatch.setenv("WG_EDGE8", edge8)
        env = BatchedPhysicsEnv(cfg["spec"], device="cuda:0", **cfg["params"])
        if auto_reset:
            env.enable_auto_reset(on=("done",), noise=cfg["pool"], final_obs=True)
        geo = env.launch_geometry()
        assert geo["walkers_per_block"] * 64 // geo["threads"] == case.wpw, geo
        assert env.batch.edges8 is not None
        buf = _buffers(env, T, case.C)
        if auto_reset:
            res = env.rollout_episodes(pol, T, episode_slots=ec.SLOTS, **buf)
            torch.cuda.synchronize()
            _check_against_reference(dict(_host(buf), stats=_stats(res), **_ep_state(env)), ref)
        else:
            for k in ("reset_out", "final_obs_out"):
                buf.pop(k)
            env.rollout_policy(pol, T, **buf)
            torch.cuda.synchronize()
            got, st = _host(buf), _state(env)
            for k in ("action", "obs", "reward", "done"):
                _bits(got[k], ref[k], f"{k} (WG_EDGE8={edge8})")
            for k, r in (("pos", "pos"), ("vel", "vel"), ("acc", "acc"), ("muscle_x", "mx"), ("steps", "steps"),
                         ("contact", "contact")):
                _bits(st[k], ref["state"][r], f"{k} after the rollout (WG_EDGE8={edge8})")
        _finite(_state(env), {k: v.cpu().numpy() for k, v in buf.items() if k != "final_obs_out"})
        monkeypatch.delenv("WG_EDGE8")

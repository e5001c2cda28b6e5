"""The resident rollouts under a policy with a second hidden layer (wg_rollout_deep: the DEEP instances of
walker_rollout_policy) through the public methods: against the reference engine's closed loop on the CPU and the device
step loop (tests/deep_cases.py; the cases are checked on the CPU by tests/test_deep_policy_cpu.py), in every mode, and
against the shallow kernels through the identity middle layer.  Every comparison is bitwise (a NaN equals a NaN of the
same bits)."""
import functools

import numpy as np
import pytest

import deep_cases as dc
import policy_cases as pc
from conftest import gpu_available
from test_gpu_policy_rollout import STATE, _bits, _buffers, _state   # (byte views, the state, NaN-filled buffers)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
f32 = np.float32
# (case, WG_POLICY_STAGE): a shared policy with its weights through L2 (0) and staged in LDS wherever they fit (2); the
# others take the default, which never stages them
RUNS = [(c, s) for c in dc.CASES for s in ((0, 2) if c.G == 1 else (None,))]
RUN_IDS = [c.name + ("" if s is None else f"-stage{s}") for c, s in RUNS]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.skip("no ROCm GPU")


def _same(a, b):
    a, b = _bits(a), _bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def _env(kind, params):
    from walker_gym_amd.batched_env import BatchedPhysicsEnv
    return BatchedPhysicsEnv(pc.spec_of(kind), device=DEV, **params)


def _fused(kind, params, pol, T, C, wpw=None):
    import torch
    env = _env(kind, params)
    if wpw is not None:
        geo = env.launch_geometry()   # the wave tile the case is there for
        assert geo["walkers_per_block"] * 64 // geo["threads"] == wpw, geo
    buf = _buffers(env, T, C)
    res = env.rollout_policy(pol, T, **buf)
    torch.cuda.synchronize()
    return dict({k[:-4]: v.cpu().numpy() for k, v in buf.items()}, **_state(env),
                returns=res["returns"].cpu().numpy(), lengths=res["lengths"].cpu().numpy())


def _step_loop(kind, params, pol, T):
    """The device loop: env.step(policy(env.obs)) with the policy's torch restatement."""
    ref = _env(kind, params)
    ref.observe()
    loop = dict(obs=[], reward=[], done=[], action=[])
    for t in range(T):
        a = pol.for_rows(0, ref.N)(ref.obs, t)
        obs, rew, done, _ = ref.step(a)
        loop["obs"].append(obs.cpu().numpy().copy()); loop["reward"].append(rew.cpu().numpy().copy())
        loop["done"].append(done.cpu().numpy().astype(np.uint8)); loop["action"].append(a.cpu().numpy().copy())
    return dict({k: np.stack(v) for k, v in loop.items()}, **_state(ref))


@functools.lru_cache(maxsize=None)
def _loop_of(name):
    case = dc.case_of(name)
    return _step_loop(case.kind, case.params, dc.policy_of(case, DEV), case.T)


def _against_oracle(fused, ref):
    for k in ("action", "obs", "reward", "done") + STATE:
        a, b = np.ascontiguousarray(fused[k]), np.ascontiguousarray(ref[k]).reshape(fused[k].shape)
        assert a.dtype == b.dtype or k in ("contact", "done"), k
        assert np.array_equal(a.view(np.uint8), b.astype(a.dtype).view(np.uint8)), k
    ret, length = pc.returns_lengths(fused["reward"], fused["done"])
    assert _same(fused["returns"], ret) and np.array_equal(fused["lengths"], length)


# ------------------------------------------------------------------ the shape axis
@pytest.mark.parametrize("case,stage", RUNS, ids=RUN_IDS)
def test_every_shape_equals_the_reference_engine_and_the_device_loop(case, stage, monkeypatch):
    """Every byte of obs / reward / done / action, the final state, returns / lengths: against Oracle.step(
    forward_numpy(obs)) and against env.step(policy(env.obs))."""
    if stage is not None:
        monkeypatch.setenv("WG_POLICY_STAGE", str(stage))
    fused = _fused(case.kind, case.params, dc.policy_of(case, DEV), case.T, case.C, case.wpw)
    _against_oracle(fused, dc.oracle_rollout(case.name))
    loop = _loop_of(case.name)
    for k in ("action", "obs", "reward", "done") + STATE:
        assert fused[k].shape == loop[k].shape and _same(fused[k], loop[k]), k


def test_no_per_step_buffers_and_split_calls():
    """The same final state and returns without a buffer; two calls of 1 and 2 steps equal one of 3."""
    import torch
    case = dc.case_of("m16-h34x33-c8-g5")
    pol = dc.policy_of(case, DEV)
    ref = dc.oracle_rollout(case.name)
    env = _env(case.kind, case.params)
    res = env.rollout_policy(pol, case.T)
    torch.cuda.synchronize()
    for k in ("pos", "vel", "acc", "muscle_x", "steps"):
        assert _same(getattr(env, k), np.asarray(ref[k]).reshape(getattr(env, k).shape)), k
    ret, length = pc.returns_lengths(ref["reward"], ref["done"])
    assert _same(res["returns"], ret) and _same(res["lengths"], length)
    two = _env(case.kind, case.params)
    ba, bb = _buffers(two, 1, case.C), _buffers(two, 2, case.C)
    two.rollout_policy(pol, 1, **ba)
    two.rollout_policy(pol, 2, **bb)
    torch.cuda.synchronize()
    for k in ("action", "obs", "reward"):
        assert _same(torch.cat([ba[k + "_out"], bb[k + "_out"]]), ref[k]), k
    for k in ("pos", "vel", "acc"):
        assert _same(getattr(two, k), getattr(env, k)), k


@pytest.mark.parametrize("lanes,graph", [(1, False), (2, True)])
def test_policy_loop_takes_a_deep_policy(lanes, graph):
    """policy_loop closes the loop through _forward_torch, bound to each walker range (G = 5: a range boundary is no set
    boundary)."""
    import torch
    case = dc.case_of("m16-h34x33-c8-g5")
    loop = _loop_of(case.name)
    env = _env(case.kind, case.params)
    env.observe()
    env.policy_loop(dc.policy_of(case, DEV), case.T, lanes=lanes, graph=graph)
    torch.cuda.synchronize()
    for k in STATE:
        assert _same(getattr(env, k), loop[k]), k
    assert _same(env.obs, loop["obs"][-1]) and _same(env.reward, loop["reward"][-1])


def test_crafted_specials_in_the_second_layer():
    """NaN, -0.0, a subnormal and +inf reaching h2 (tests/deep_cases.py SPECIAL): the reference engine's bits, the device
    loop's, and the columns each special shows in."""
    s = dc.SPECIAL
    pol = dc.policy_from(dc.special_weights(), DEV, act_limit=1.0)
    fused = _fused(s["kind"], s["params"], pol, s["T"], s["C"], 8)
    _against_oracle(fused, dc.special_rollout())
    loop = _step_loop(s["kind"], s["params"], pol, s["T"])
    for k in ("action", "obs", "reward", "done") + STATE:
        assert _same(fused[k], loop[k]), k
    a, n = fused["action"], fused["action"].shape[1] // 2
    assert (a[:, :n, 1] == 0).all() and not np.signbit(a[:, :n, 1]).any()
    assert (a[:, :n, 2] == f32(f32(1e-40) * f32(2.0 ** 100))).all() and np.isfinite(a).all()
    assert (np.abs(a[:, n:]) == 1).all()


# ------------------------------------------------------------------ the modes, through the public methods
_KEYS = dict(obs_out="obs", reward_out="reward", done_out="done", action_out="action", raw_action_out="raw",
             eps_out="eps", steps_out="steps_t", reset_out="reset", final_obs_out="final_obs", decided_out="decided",
             hold_reward_out="hold_reward")


def _mode_env(batch, auto_reset):
    from walker_gym_amd.batched_env import BatchedPhysicsEnv
    cfg = dc.mode_config(batch)
    env = BatchedPhysicsEnv(cfg["spec"], device=DEV, **cfg["params"])
    if auto_reset:
        env.enable_auto_reset(on=("done",), noise=cfg["pool"], final_obs=True)
    return env


def _mode_buffers(env, Tn, Cc, auto_reset, noise, hold):
    import torch
    N, D = env.N, env.obs_dim
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    ff = lambda *s: torch.full(s, 255, dtype=torch.uint8, device=DEV)
    buf = dict(obs_out=nan(Tn, N, D), reward_out=nan(Tn, N), done_out=ff(Tn, N), action_out=nan(Tn, N, Cc))
    if noise or hold:
        buf.update(steps_out=torch.full((Tn, N), -7, dtype=torch.int32, device=DEV))
    if noise:   # (under a hold the rows of the walkers that do not decide keep this)
        buf.update(raw_action_out=torch.full((Tn, N, Cc), float(dc.SENTINEL), device=DEV),
                   eps_out=torch.full((Tn, N, Cc), float(dc.SENTINEL), device=DEV))
    if auto_reset:
        buf.update(reset_out=ff(Tn, N), final_obs_out=nan(Tn, N, D))
    if hold:
        buf.update(decided_out=ff(Tn, N), hold_reward_out=nan(Tn, N))
    return buf


def _mode_call(env, pol, batch, auto_reset, noise, every, Tn, step_base=dc.STEP_BASE, held=None, hold=None):
    """One call of the public method the mode belongs to: rollout_held when `hold`, else rollout_stochastic with the
    noise, else rollout_episodes / rollout_policy."""
    import torch
    hold = (every > 1) if hold is None else hold
    Cc = dc.MODES[batch]["C"]
    buf = _mode_buffers(env, Tn, Cc, auto_reset, noise, hold)
    kw = dict(episode_slots=dc.SLOTS) if auto_reset else {}
    sigma = torch.from_numpy(dc.mode_sigma(batch).copy()).to(DEV)
    if hold:
        if noise:
            kw.update(sigma=sigma, seed=dc.SEED)
        res = env.rollout_held(pol, Tn, every, step_base=step_base, walker_base=dc.WALKER_BASE, held=held, **buf, **kw)
    elif noise:
        res = env.rollout_stochastic(pol, Tn, sigma, dc.SEED, step_base=step_base, walker_base=dc.WALKER_BASE, **buf, **kw)
    elif auto_reset:
        res = env.rollout_episodes(pol, Tn, **buf, **kw)
    else:
        res = env.rollout_policy(pol, Tn, **buf)
    torch.cuda.synchronize()
    out = {_KEYS[k]: v.cpu().numpy() for k, v in buf.items()}
    out.update(_state(env))
    if auto_reset:
        out["episodes"] = env.batch.episodes.detach().cpu().numpy().copy()
    res = dict(res)
    if "held" in res:
        out["held"] = res.pop("held").cpu().numpy()
    out["stats"] = {k: v.cpu().numpy() for k, v in res.items()}
    return out


def _mode_check(got, ref, auto_reset):
    for k in got:
        if k in ("stats", "held", "episodes") or k in STATE:
            continue
        a, b = got[k], np.ascontiguousarray(ref[k]).reshape(got[k].shape)
        assert a.dtype == b.dtype and _same(a, b), k
    if "held" in got:
        assert _same(got["held"], ref["held"]), "held"
    st = ref["state"]
    names = [("pos", "pos"), ("vel", "vel"), ("acc", "acc"), ("muscle_x", "mx"), ("steps", "steps")]
    for k, r in names + ([("episodes", "episodes")] if auto_reset else []):
        assert _same(got[k], np.asarray(st[r]).reshape(got[k].shape).astype(got[k].dtype)), k
    assert np.array_equal(got["contact"].astype(np.uint8).ravel(), np.asarray(st["contact"]).astype(np.uint8).ravel())
    assert set(got["stats"]) == set(ref["stats"])
    for k, v in got["stats"].items():
        assert v.dtype == ref["stats"][k].dtype and _same(v, ref["stats"][k]), k


@pytest.mark.parametrize("batch,auto_reset,noise,norm,every,Tn", dc.MODE_RUNS)
def test_each_mode_equals_the_per_step_loop_of_the_contract(batch, auto_reset, noise, norm, every, Tn):
    """rollout_policy / rollout_episodes (done firing, the episode stats with four slots), rollout_stochastic (raw / eps
    against pg.stochastic_forward_numpy), a policy with an obs_norm (the stored rows stay raw: they are the reference's),
    and rollout_held with every = 4, `held` passed across a call split 3 + 5."""
    import torch
    env = _mode_env(batch, auto_reset)
    pol = dc.mode_policy(batch, DEV, norm=norm)
    ref = dc.mode_reference(batch, auto_reset, noise, norm, every, Tn)
    if every == 1:
        _mode_check(_mode_call(env, pol, batch, auto_reset, noise, 1, Tn), ref, auto_reset)
        return
    held = torch.from_numpy(dc.mode_held(batch).copy()).to(DEV)
    a = _mode_call(env, pol, batch, auto_reset, noise, every, 3, held=held)
    assert _same(a["held"], held)                       # the tensor given is the one returned, updated in place
    b = _mode_call(env, pol, batch, auto_reset, noise, every, Tn - 3, step_base=dc.STEP_BASE + 3, held=held)
    both = dict(b)
    for k in a:
        if k not in ("stats", "held", "episodes") and k not in STATE:
            both[k] = np.concatenate([a[k], b[k]])
    stats = both.pop("stats")                           # (the stats are per call: checked through one whole call below)
    whole = _mode_call(_mode_env(batch, auto_reset), pol, batch, auto_reset, noise, every, Tn,
                       held=torch.from_numpy(dc.mode_held(batch).copy()).to(DEV))
    _mode_check(whole, ref, auto_reset)
    both["stats"] = whole["stats"]
    _mode_check(both, ref, auto_reset)
    assert set(stats) == set(whole["stats"])
    assert not a["decided"][-1].all() and not b["decided"][0].all()    # holds open across the cut


@pytest.mark.parametrize("mode", ["off", "ar"])
@pytest.mark.parametrize("edge8", [True, False], ids=["compact", "16-byte"])
@pytest.mark.parametrize("name", [c.name for c in pc.COVER])
def test_every_deep_instance_equals_reference(name, edge8, mode, monkeypatch):
    """walker_rollout_policy's DEEP family at every (IN3D, NE, E8, AR): one launch each, against the per-step loop of the
    contract on the reference engine (auto-reset off, deterministic) or the composed reference (on, with the noise)."""
    import episode_cases as ec
    import torch
    from walker_gym_amd.batched_env import BatchedPhysicsEnv
    if not edge8:
        monkeypatch.setenv("WG_EDGE8", "0")
    ar = mode == "ar"
    cfg, case = ec.config(name), pc.case_of(name)
    env = BatchedPhysicsEnv(cfg["spec"], device=DEV, **cfg["params"])
    geo = env.launch_geometry()
    assert geo["walkers_per_block"] * 64 // geo["threads"] == case.wpw, geo
    if ar:
        env.enable_auto_reset(on=("done",), noise=cfg["pool"], final_obs=True)
    pol, Tn = dc.cover_policy(name, DEV), dc.COVER_T
    buf = _mode_buffers(env, Tn, case.C, ar, ar, False)
    if ar:
        res = env.rollout_stochastic(pol, Tn, torch.from_numpy(dc.cover_sigma(name)).to(DEV), dc.SEED,
                                     step_base=dc.STEP_BASE, walker_base=dc.WALKER_BASE, episode_slots=dc.SLOTS, **buf)
    else:
        res = env.rollout_policy(pol, Tn, **buf)
    torch.cuda.synchronize()
    got = {_KEYS[k]: v.cpu().numpy() for k, v in buf.items()}
    got.update(_state(env))
    if ar:
        got["episodes"] = env.batch.episodes.detach().cpu().numpy().copy()
    got["stats"] = {k: v.cpu().numpy() for k, v in res.items()}
    _mode_check(got, dc.cover_reference(name, ar), ar)


IDENTITY = [("balance16", False, False, False, 1, False), ("balance16", True, False, False, 1, False),
            ("canonical4", False, True, False, 1, False), ("canonical4", True, True, False, 1, False),
            ("canonical4", True, False, True, 1, False), ("canonical4", False, False, False, 1, True),
            ("canonical4", True, True, True, 3, True)]


@pytest.mark.parametrize("batch,auto_reset,noise,norm,every,hold", IDENTITY)
def test_identity_middle_layer_equals_the_shallow_kernels(batch, auto_reset, noise, norm, every, hold):
    """H2 = H1, wm = I, no bm: the deep policy through wg_rollout_deep against its one-layer twin through the existing
    entry of the mode (wg_rollout_policy / _episodes / _stochastic / _normalized / _held), every output, the final
    state, the returned arrays.  The property needs every first-layer h finite: the rows are (asserted) and the weights
    are small (tests/test_deep_policy_cpu.py computes the h of the mode runs' rows under these weights)."""
    import torch
    Tn = 6
    runs = []
    for shallow in (True, False):
        pol = dc.mode_policy(batch, DEV, norm=norm, identity=True, shallow=shallow)
        assert pol.H2 == (0 if shallow else pol.H)
        held = torch.from_numpy(dc.mode_held(batch).copy()).to(DEV) if hold else None
        runs.append(_mode_call(_mode_env(batch, auto_reset), pol, batch, auto_reset, noise, every, Tn, held=held, hold=hold))
    a, b = runs
    assert set(a) == set(b) and set(a["stats"]) == set(b["stats"])
    for k in a:
        if k != "stats":
            assert _same(a[k], b[k]), k
    for k in a["stats"]:
        assert _same(a["stats"][k], b["stats"][k]), k
    assert np.isfinite(a["obs"]).all() and not np.array_equal(a["action"][0], a["action"][-1])


# ------------------------------------------------------------------ refusals; the shallow paths
def test_refusals_leave_the_env_usable():
    import torch
    from walker_gym_amd.policy import MLPPolicy
    from walker_gym_amd.synthetic import canonical_walkers, ragged_walkers
    from walker_gym_amd.batched_env import BatchedPhysicsEnv
    z = lambda *s: torch.zeros(s, device=DEV)
    deep = lambda D=152, H1=6, H2=5, C=8, G=1: MLPPolicy(z(G, H2, C), None, z(G, D, H1), None, wm=z(G, H1, H2))
    rg = BatchedPhysicsEnv(ragged_walkers(200, seed=2), device=DEV, in3d=1)
    with pytest.raises(ValueError, match="policy_loop"):
        rg.rollout_policy(deep(rg.obs_dim, C=2), 2)
    env = BatchedPhysicsEnv(canonical_walkers(256, seed=2), device=DEV, in3d=1)
    with pytest.raises(ValueError):
        env.rollout_policy(deep(D=151), 2)
    with pytest.raises(ValueError):
        env.rollout_policy(deep(C=9), 2)
    with pytest.raises(ValueError):
        env.rollout_policy(deep(G=3), 2)
    with pytest.raises(ValueError):
        env.rollout_policy(deep(), 0)
    with pytest.raises(ValueError):                                 # host weights
        env.rollout_policy(deep().to("cpu"), 2)
    with pytest.raises(ValueError):
        env.rollout_stochastic(deep(), 2, None, 1)                  # sigma
    with pytest.raises(ValueError):
        env.rollout_held(deep(), 2, 0)                              # every
    with pytest.raises(ValueError, match="auto-reset"):
        env.rollout_episodes(deep(), 2)
    ref = BatchedPhysicsEnv(canonical_walkers(256, seed=2), device=DEV, in3d=1)
    r = env.rollout_policy(deep(), 3)                               # zero weights: zero actions
    for t in range(3):
        ref.step(z(256, 8))
    torch.cuda.synchronize()
    assert (r["lengths"] == 3).all()
    for k in STATE:
        assert _same(getattr(env, k), getattr(ref, k)), k


def test_shallow_policies_keep_their_bits():
    """rollout_policy and rollout_held (every = 1) with a one-layer policy, after the DEEP flag went into the kernel:
    the reference engine's bits, as tests/test_gpu_policy_rollout.py has them."""
    import torch
    case = pc.case_of("canonical4-mlp-5sets")
    pol = pc.policy_of(case, DEV)
    ref = pc.oracle_rollout(case.name)
    fused = _fused(case.kind, case.params, pol, case.T, case.C, case.wpw)
    _against_oracle(fused, ref)
    env = _env(case.kind, case.params)
    buf = _buffers(env, case.T, case.C)
    res = env.rollout_held(pol, case.T, 1, **buf)
    torch.cuda.synchronize()
    held = dict({k[:-4]: v.cpu().numpy() for k, v in buf.items()}, **_state(env),
                returns=res["returns"].cpu().numpy(), lengths=res["lengths"].cpu().numpy())
    _against_oracle(held, ref)

"""BatchedPhysicsEnv.rollout_held (wg_rollout_held: the resident closed loop with an action hold) against the per-step loop
of the contract on the CPU (tests/hold_cases.py), in the four modes (auto-reset off / on, noise off / on), and against
the existing entries at every = 1.  Every comparison is bitwise (a NaN equals a NaN of the same bits)."""
import ctypes as C

import numpy as np
import pytest

import es_cases as esc
import hold_cases as hc
from conftest import gpu_available

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
f32 = np.float32
STATE = ("pos", "vel", "acc", "muscle_x", "steps", "contact")
STEP = ("obs", "reward", "done", "steps_t", "action", "decided", "hold_reward")
STATS_ON = ("return_sum", "length_sum", "episodes", "tail_return", "tail_length", "ep_returns", "ep_lengths")
MODES = pytest.mark.parametrize("auto_reset,noise", [(False, False), (False, True), (True, False), (True, True)],
                                ids=["off-det", "off-nz", "ar-det", "ar-nz"])
EVERY = pytest.mark.parametrize("every", hc.EVERY)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.skip("no ROCm GPU")


def _bits(t):
    a = t.detach().cpu().contiguous().numpy() if hasattr(t, "detach") else np.ascontiguousarray(t)
    return a.view(np.uint8)


def _same(a, b):
    a, b = _bits(a), _bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def _env(name, auto_reset):
    from walker_gym_amd.batched_env import BatchedPhysicsEnv
    case = hc.case_of(name)
    if not auto_reset:
        return BatchedPhysicsEnv(hc.spec_off(name), device=DEV, **case.params)
    cfg = hc.config(name)
    env = BatchedPhysicsEnv(cfg["spec"], device=DEV, **cfg["params"])
    env.enable_auto_reset(on=("done",), noise=cfg["pool"], final_obs=True)
    return env


def _buffers(env, Tn, Cc, auto_reset, noise):
    import torch
    N, D = env.N, env.obs_dim
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)   # (a value the kernel failed to write cannot pass)
    ff = lambda *s: torch.full(s, 255, dtype=torch.uint8, device=DEV)
    buf = dict(obs_out=nan(Tn, N, D), reward_out=nan(Tn, N), done_out=ff(Tn, N), action_out=nan(Tn, N, Cc),
               steps_out=torch.full((Tn, N), -7, dtype=torch.int32, device=DEV), decided_out=ff(Tn, N),
               hold_reward_out=nan(Tn, N))
    if noise:   # (the rows of the walkers that do not decide keep this)
        buf.update(raw_action_out=torch.full((Tn, N, Cc), float(hc.SENTINEL), device=DEV),
                   eps_out=torch.full((Tn, N, Cc), float(hc.SENTINEL), device=DEV))
    if auto_reset:
        buf.update(reset_out=ff(Tn, N), final_obs_out=nan(Tn, N, D))
    return buf


_KEYS = dict(obs_out="obs", reward_out="reward", done_out="done", action_out="action", raw_action_out="raw",
             eps_out="eps", steps_out="steps_t", reset_out="reset", final_obs_out="final_obs", decided_out="decided",
             hold_reward_out="hold_reward")


def _state(env, auto_reset):
    st = {k: getattr(env, k).detach().cpu().numpy().copy() for k in STATE}
    if auto_reset:
        st["episodes"] = env.batch.episodes.detach().cpu().numpy().copy()
    return st


def _run(name, auto_reset, noise, every, Tn=None, step_base=hc.STEP_BASE, held="case", env=None, buffers=True,
         slots=hc.SLOTS, norm=None):
    """One call on a fresh env (or `env`).  held: 'case' (hold_cases.held_of), None, or a device tensor."""
    import torch
    case = hc.case_of(name)
    env = _env(name, auto_reset) if env is None else env
    Tn = (hc.T_ON if auto_reset else case.t_off) if Tn is None else Tn
    buf = _buffers(env, Tn, case.C, auto_reset, noise) if buffers else {}
    kw = dict(episode_slots=slots) if auto_reset else {}
    if noise:
        kw.update(sigma=torch.from_numpy(case.sigma().copy()).to(DEV), seed=hc.SEED)
    if isinstance(held, str):
        held = torch.from_numpy(hc.held_of(name).copy()).to(DEV)
    res = env.rollout_held(case.policy(DEV, norm=norm), Tn, every, step_base=step_base, walker_base=hc.WALKER_BASE,
                           held=held, **buf, **kw)
    torch.cuda.synchronize()
    out = {_KEYS[k]: v.cpu().numpy() for k, v in buf.items()}
    out.update(_state(env, auto_reset))
    out["held"] = res.pop("held").cpu().numpy()
    out["stats"] = {k: v.cpu().numpy() for k, v in res.items()}
    return out


def _check(got, ref, auto_reset, noise):
    keys = STEP + (("raw", "eps") if noise else ()) + (("reset", "final_obs") if auto_reset else ())
    for k in keys:
        a, b = got[k], np.ascontiguousarray(ref[k]).reshape(got[k].shape)
        assert a.dtype == b.dtype and _same(a, b), k
    assert _same(got["held"], ref["held"]), "held"
    st = ref["state"]
    names = [("pos", "pos"), ("vel", "vel"), ("acc", "acc"), ("muscle_x", "mx"), ("steps", "steps")]
    for k, r in names + ([("episodes", "episodes")] if auto_reset else []):
        assert _same(got[k], np.asarray(st[r]).reshape(got[k].shape).astype(got[k].dtype)), k
    assert np.array_equal(got["contact"].astype(np.uint8).ravel(), np.asarray(st["contact"]).astype(np.uint8).ravel())
    for k in (STATS_ON if auto_reset else ("returns", "lengths")):
        assert got["stats"][k].dtype == ref["stats"][k].dtype and _same(got["stats"][k], ref["stats"][k]), k


# ------------------------------------------------------------------ against the CPU reference
@MODES
@EVERY
@pytest.mark.parametrize("name", hc.NAMES)
def test_equals_the_per_step_loop_of_the_contract(name, every, auto_reset, noise):
    """Every per-step output, decided, hold_reward, the raw / eps rows (a sentinel where the walker did not decide),
    held, the final state, returns / lengths or the stats with four slots."""
    case = hc.case_of(name)
    env = _env(name, auto_reset)
    geo = env.launch_geometry()   # the wave tile the case is there for
    assert geo["walkers_per_block"] * 64 // geo["threads"] == case.wpw, geo
    got = _run(name, auto_reset, noise, every, env=env)
    _check(got, hc.reference(name, auto_reset, noise, every), auto_reset, noise)
    assert 0 < got["decided"].mean() < 1 and not got["decided"][0].all()


# ------------------------------------------------------------------ every = 1 is the existing entry
@MODES
@pytest.mark.parametrize("name", [hc.MAIN, "balance16-h0-perwalker", "norm-canonical4-mlp-5sets"])
def test_every_1_equals_the_existing_entry(name, auto_reset, noise):
    """rollout_policy / rollout_episodes / rollout_stochastic (through wg_rollout_normalized for the policy that carries a
    normaliser): every output they have, the final state and the returned arrays."""
    import torch
    case = hc.case_of(name)
    got = _run(name, auto_reset, noise, 1)
    assert got["decided"].all() and _same(got["hold_reward"], got["reward"])
    env = _env(name, auto_reset)
    Tn = hc.T_ON if auto_reset else case.t_off
    buf = _buffers(env, Tn, case.C, auto_reset, noise)
    for k in ("decided_out", "hold_reward_out") + (() if noise else ("steps_out",)):
        del buf[k]
    pol = case.policy(DEV)
    if noise:
        res = env.rollout_stochastic(pol, Tn, torch.from_numpy(case.sigma().copy()).to(DEV), hc.SEED,
                                     step_base=hc.STEP_BASE, walker_base=hc.WALKER_BASE, **buf,
                                     **(dict(episode_slots=hc.SLOTS) if auto_reset else {}))
    elif auto_reset:
        res = env.rollout_episodes(pol, Tn, episode_slots=hc.SLOTS, **buf)
    else:
        res = env.rollout_policy(pol, Tn, **buf)
    torch.cuda.synchronize()
    for k, v in buf.items():
        assert _same(v, got[_KEYS[k]]), k
    for k, v in _state(env, auto_reset).items():
        assert _same(v, got[k]), k
    assert set(res) == set(got["stats"])
    for k, v in res.items():
        assert _same(v, got["stats"][k]), k
    assert _same(got["held"][:, :case.C], got["action"][-1]) and _same(got["held"][:, case.C], got["reward"][-1])


# ------------------------------------------------------------------ the hold across calls
@EVERY
@pytest.mark.parametrize("name", hc.NAMES)
def test_two_calls_of_8_equal_one_of_16(name, every):
    """held passed through and step_base advanced by 8: outputs, held and the final state (auto-reset and noise on)."""
    import torch
    ref = hc.reference(name, True, True, every)
    env = _env(name, True)
    held = torch.from_numpy(hc.held_of(name).copy()).to(DEV)
    a = _run(name, True, True, every, Tn=8, env=env, held=held)
    assert _same(a["held"], held)                       # the tensor given is the one returned, updated in place
    b = _run(name, True, True, every, Tn=8, step_base=hc.STEP_BASE + 8, env=env, held=held)
    for k in STEP + ("raw", "eps", "reset", "final_obs"):
        assert _same(np.concatenate([a[k], b[k]]), np.ascontiguousarray(ref[k]).reshape((16,) + a[k].shape[1:])), k
    assert _same(b["held"], ref["held"])
    for k, r in (("pos", "pos"), ("vel", "vel"), ("muscle_x", "mx"), ("steps", "steps"), ("episodes", "episodes")):
        assert _same(b[k], np.asarray(ref["state"][r]).reshape(b[k].shape).astype(b[k].dtype)), k
    assert not a["decided"][-1].all() and not b["decided"][0].all()    # holds open across the cut


@MODES
def test_held_none_equals_explicit_zeros(auto_reset, noise):
    import torch
    name, every = hc.MAIN, 3
    none = _run(name, auto_reset, noise, every, held=None)
    zeros = _run(name, auto_reset, noise, every,
                 held=torch.zeros((hc.n_walkers(name), hc.case_of(name).C + 1), device=DEV))
    for k in none:
        if k != "stats":
            assert _same(none[k], zeros[k]), k
    _check(none, hc.reference(name, auto_reset, noise, every, zero_held=True), auto_reset, noise)
    first = none["decided"][0] == 0
    assert first.mean() > 0.5 and not none["action"][0][first].any()


def test_no_buffer_run_gives_the_same_final_state_and_held():
    name, every = hc.MAIN, 2
    for auto_reset, noise in ((False, True), (True, False)):
        full = _run(name, auto_reset, noise, every)
        bare = _run(name, auto_reset, noise, every, buffers=False)
        for k in STATE + ("held",) + (("episodes",) if auto_reset else ()):
            assert _same(full[k], bare[k]), k
        for k in full["stats"]:
            assert _same(full["stats"][k], bare["stats"][k]), k


@pytest.mark.parametrize("auto_reset", [False, True], ids=["off", "ar"])
def test_second_half_with_walker_base_equals_the_full_run(auto_reset, name="six-h5-c6-shared"):
    """(A shared policy: a view's walkers map to parameter sets by the view's own N.)  A walker-range view [N / 2, N) of the state with walker_base + N / 2 and the buffers' second halves gives the second
    half of the full run: outputs, actions, variates, decided, hold_reward, held and state; nothing else is written."""
    import torch
    from walker_gym_amd import _lib
    from walker_gym_amd.batched_env import BatchedPhysicsEnv
    case, every = hc.case_of(name), 3
    full = _run(name, auto_reset, True, every)
    Tn = hc.T_ON if auto_reset else case.t_off
    env = _env(name, auto_reset)
    N, D, Cc, M, A = env.N, env.obs_dim, case.C, env.batch.M, env.batch.A
    h = N // 2
    pol = case.policy(DEV)
    sg = torch.from_numpy(case.sigma().copy()).to(DEV)
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    obs, act, raw, eps, hrw = nan(Tn, N, D), nan(Tn, N, Cc), nan(Tn, N, Cc), nan(Tn, N, Cc), nan(Tn, N)
    dec = torch.full((Tn, N), 255, dtype=torch.uint8, device=DEV)
    held = torch.from_numpy(hc.held_of(name).copy()).to(DEV)
    o = env._outputs(obs, None, None, None, None, obs_step=N * D, out_step=N, pad_clean=True)
    o = BatchedPhysicsEnv._range_outputs(o, h)
    ps = pol.struct(N, act)
    ps.action_out = C.c_void_p(act.data_ptr() + 4 * h * Cc)
    nz = _lib.WgActionNoise(seed=hc.SEED, step_base=hc.STEP_BASE, walker_base=hc.WALKER_BASE + h, sigma=_lib.ptr(sg),
                            raw_out=C.c_void_p(raw.data_ptr() + 4 * h * Cc), raw_out_step=N * Cc,
                            eps_out=C.c_void_p(eps.data_ptr() + 4 * h * Cc), eps_out_step=N * Cc)
    hold = _lib.WgActionHold(every=every, held=C.c_void_p(held.data_ptr() + 4 * h * (Cc + 1)),
                             decided_out=C.c_void_p(dec.data_ptr() + h), decided_out_step=N,
                             hold_reward_out=C.c_void_p(hrw.data_ptr() + 4 * h), hold_reward_out_step=N)
    st = C.byref(_lib.WgEpisodeStats()) if auto_reset else None
    sub = env.batch.sub_struct(h, N)
    _lib.check(_lib.load().wg_rollout_held(C.byref(sub), C.byref(env._pstruct), C.byref(ps), None, C.byref(nz),
                                           C.byref(hold), C.byref(o), st, Tn, env._stream()), "wg_rollout_held")
    torch.cuda.synchronize()
    for got, k in ((obs, "obs"), (act, "action"), (hrw, "hold_reward"), (dec, "decided")):
        g = got.cpu().numpy()
        assert _same(g[:, h:], full[k][:, h:]), k
        assert (np.isnan(g[:, :h]).all() if g.dtype == np.float32 else (g[:, :h] == 255).all()), k
    on = full["decided"][:, h:] != 0
    for got, k in ((raw, "raw"), (eps, "eps")):
        g = got.cpu().numpy()
        assert _same(g[:, h:][on], full[k][:, h:][on]) and np.isnan(g[:, h:][~on]).all() and np.isnan(g[:, :h]).all(), k
    hg = held.cpu().numpy()
    assert _same(hg[h:], full["held"][h:]) and _same(hg[:h], hc.held_of(name)[:h])
    per = dict(pos=3 * M, vel=3 * M, acc=3 * M, muscle_x=A, steps=1)
    for k, n in per.items():
        g = getattr(env, k).cpu().numpy().reshape(-1)
        assert _same(g[h * n:], full[k].reshape(-1)[h * n:]), k


# ------------------------------------------------------------------ every HOLD instance
@pytest.mark.parametrize("auto_reset", [False, True], ids=["off", "ar"])
@pytest.mark.parametrize("edge8", [True, False], ids=["compact", "16-byte"])
@pytest.mark.parametrize("form", ["on", "off"])
@pytest.mark.parametrize("name", hc.COVER_NAMES)
def test_every_hold_instance_equals_reference(name, form, edge8, auto_reset, monkeypatch):
    """The HOLD instance of walker_rollout_policy at every (IN3D, NE, E8, AR), every = 2: policy_cases.COVER's batches,
    once with the noise and the normaliser both on (norm_cases.COVER's policies) and once with both off (the instance
    carries them as runtime options).  T = 4 without auto-reset, 16 with.  Both record formats against one reference."""
    if not edge8:
        monkeypatch.setenv("WG_EDGE8", "0")
    full = f"{form}-{name}"
    case, noise = hc.case_of(full), form == "on"
    env = _env(full, auto_reset)
    geo = env.launch_geometry()
    assert geo["walkers_per_block"] * 64 // geo["threads"] == case.wpw, geo
    _check(_run(full, auto_reset, noise, 2, env=env), hc.reference(full, auto_reset, noise, 2), auto_reset, noise)


@pytest.mark.parametrize("stage", ["0", "2"])
def test_weights_staged_and_through_l2(stage, monkeypatch):
    """WG_POLICY_STAGE 0 and 2 on the shared policy: the default run's bytes, which are the reference's."""
    name, every = "six-h5-c6-shared", 2
    want = _run(name, True, True, every)
    monkeypatch.setenv("WG_POLICY_STAGE", stage)
    got = _run(name, True, True, every)
    for k in STEP + ("raw", "eps", "held") + STATE:
        assert _same(got[k], want[k]), k
    _check(got, hc.reference(name, True, True, every), True, True)


# ------------------------------------------------------------------ refusals, and nothing else changed
def test_refusals_leave_the_env_usable():
    import torch
    from walker_gym_amd import _lib
    from walker_gym_amd.batched_env import BatchedPhysicsEnv
    from walker_gym_amd.policy import MLPPolicy
    from walker_gym_amd.synthetic import canonical_walkers, ragged_walkers
    z = lambda *s: torch.zeros(s, device=DEV)
    rg = BatchedPhysicsEnv(ragged_walkers(200, seed=2), device=DEV, in3d=1)
    with pytest.raises(ValueError, match="resident lean kernel"):            # a ragged batch
        rg.rollout_held(MLPPolicy(z(rg.obs_dim, 2)), 2, 2)
    pf = BatchedPhysicsEnv(canonical_walkers(256, seed=2), device=DEV, in3d=1, pair_mode=1)
    with pytest.raises(ValueError, match="resident lean kernel"):            # pair forces
        pf.rollout_held(MLPPolicy(z(152, 8)), 2, 2, sigma=0.1, seed=1)
    env = BatchedPhysicsEnv(canonical_walkers(256, seed=2), device=DEV, in3d=1, max_steps=3)
    good = MLPPolicy(z(152, 8))
    env.step(z(256, 8))
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8, device=DEV)
    bad = [dict(every=0), dict(every=-1), dict(n_steps=0), dict(sigma=z(2, 8)), dict(sigma=torch.zeros(1, 8)),
           dict(sigma=0.1, seed=-1), dict(sigma=0.1, step_base=(1 << 32) - 1), dict(episode_slots=2),
           dict(reset_out=u8(2, 256)), dict(final_obs_out=z(2, 256, 152)), dict(eps_out=z(2, 256, 8)),
           dict(sigma=0.1, eps_out=z(2, 256, 7)), dict(sigma=0.1, raw_action_out=z(3, 256, 8)), dict(steps_out=z(2, 256)),
           dict(held=z(256, 8)), dict(held=z(255, 9)), dict(held=torch.zeros(256, 9)), dict(decided_out=u8(2, 255)),
           dict(decided_out=z(2, 256)), dict(hold_reward_out=z(3, 256)), dict(hold_reward_out=u8(2, 256)),
           dict(policy=MLPPolicy(z(151, 8))), dict(policy=lambda rows, t: rows)]
    for kw in bad:
        args = dict(policy=good, n_steps=2, every=2)
        args.update(kw)
        with pytest.raises(ValueError):
            env.rollout_held(**args)
    assert "total_energy" in env.info()                                      # a refused call marks nothing stale
    # st in the wrong mode and the strides, at the C boundary
    pol, L = good.struct(256), _lib.load()
    dcd, hrw = u8(2, 256), z(2, 256)
    call = lambda e, hold, st: L.wg_rollout_held(C.byref(e.batch.struct), C.byref(e._pstruct), C.byref(pol), None, None,
                                                 None if hold is None else C.byref(hold), None, st, 2, e._stream())
    hold = _lib.WgActionHold(every=2)
    assert call(env, hold, C.byref(_lib.WgEpisodeStats())) == _lib.WG_EINVAL and b"st must be NULL" in L.wg_last_error()
    assert call(env, None, None) == _lib.WG_EINVAL and b"null action hold" in L.wg_last_error()
    assert call(env, _lib.WgActionHold(every=0), None) == _lib.WG_EINVAL and b"every" in L.wg_last_error()
    short = _lib.WgActionHold(every=2, decided_out=_lib.ptr(dcd), decided_out_step=255)
    assert call(env, short, None) == _lib.WG_EINVAL and b"decided_out_step" in L.wg_last_error()
    short = _lib.WgActionHold(every=2, hold_reward_out=_lib.ptr(hrw), hold_reward_out_step=255)
    assert call(env, short, None) == _lib.WG_EINVAL and b"hold_reward_out_step" in L.wg_last_error()
    env.enable_auto_reset()
    assert call(env, hold, None) == _lib.WG_EINVAL and b"null episode stats" in L.wg_last_error()
    # the env still steps, and an accepted call marks the one-step outputs stale
    ref = BatchedPhysicsEnv(canonical_walkers(256, seed=2), device=DEV, in3d=1, max_steps=3)
    ref.step(z(256, 8))
    ref.enable_auto_reset()
    r = env.rollout_held(good, 4, 2)                                         # zero weights: zero actions
    for t in range(4):
        ref.step(z(256, 8))
    torch.cuda.synchronize()
    assert (r["episodes"] == 1).all() and (r["length_sum"] == 2).all() and not r["held"][:, :8].any()
    for k in STATE:
        assert _same(getattr(env, k), getattr(ref, k)), k
    assert "total_energy" not in env.info()
    assert _same(env.step(z(256, 8))[0], ref.step(z(256, 8))[0]) and "total_energy" in env.info()


@pytest.mark.parametrize("auto_reset", [False, True])
def test_plain_entries_keep_their_bytes(auto_reset):
    """rollout_policy / rollout_episodes / rollout_stochastic give, after a held call on the same env, the bytes they gave
    before it."""
    import torch
    name = hc.MAIN
    case = hc.case_of(name)
    env = _env(name, auto_reset)
    pol = case.policy(DEV)
    sg = torch.from_numpy(case.sigma().copy()).to(DEV)
    state0 = env.batch.state_dict()

    def restore():
        env.batch.load_state_dict(state0)
        if auto_reset:
            env.batch.episodes.zero_()

    def plain():
        out = []
        for noise in (False, True):
            restore()
            N, D = env.N, env.obs_dim
            buf = dict(obs_out=torch.full((6, N, D), float("nan"), device=DEV),
                       action_out=torch.full((6, N, case.C), float("nan"), device=DEV))
            if noise:
                res = env.rollout_stochastic(pol, 6, sg, hc.SEED, **buf)
            else:
                res = env.rollout_episodes(pol, 6, **buf) if auto_reset else env.rollout_policy(pol, 6, **buf)
            torch.cuda.synchronize()
            out += [v.cpu().numpy() for v in buf.values()] + [v.cpu().numpy() for v in res.values()] + \
                list(_state(env, auto_reset).values())
        return out
    before = plain()
    restore()
    env.rollout_held(pol, 6, 3, sigma=sg, seed=hc.SEED)
    after = plain()
    assert len(before) == len(after) and all(_same(a, b) for a, b in zip(before, after))


# ------------------------------------------------------------------ evolution strategies
def test_generation_step_with_a_hold_equals_its_composition():
    """EvolutionStrategy.generation_step(act_every=2) against numpy perturb -> a second env's deterministic held rollout
    from zeros -> numpy update, two generations."""
    from walker_gym_amd.batched_env import BatchedPhysicsEnv
    from walker_gym_amd.es import EvolutionStrategy
    H, G = 5, 16
    mk = lambda: BatchedPhysicsEnv(esc.balance128(), device=DEV, **esc.PARAMS)
    env, ref_env = mk(), mk()
    tr = EvolutionStrategy(env, hidden=H, act_dim=esc.C, biases=True, population=G, sigma=esc.SIGMA[H], lr=esc.LR[H],
                           seed=esc.SEED, theta0=esc.theta0(H))
    plain = EvolutionStrategy(mk(), hidden=H, act_dim=esc.C, biases=True, population=G, sigma=esc.SIGMA[H],
                              lr=esc.LR[H], seed=esc.SEED, theta0=esc.theta0(H))
    start = ref_env.batch.state_dict()
    theta = esc.theta0(H)
    for g in range(2):
        out = tr.generation_step(esc.T, act_every=2)
        ref_env.batch.load_state_dict(start)
        res = ref_env.rollout_held(esc.numpy_policy(theta, f32(esc.SIGMA[H]), g, H, G, device=DEV), esc.T, 2)
        fit = esc.set_fitness(res["returns"].cpu().numpy(), G)
        grad, theta = esc.numpy_tell(theta, fit, g, H, G)
        assert np.isfinite(fit).all() and len(np.unique(fit)) > G // 2
        assert _same(out["fitness"], fit) and _same(out["grad"], grad) and _same(tr.theta, theta), g
        if g == 0:
            assert not _same(plain.generation_step(esc.T)["fitness"], fit)   # (the hold changes the rollouts)
    with pytest.raises(ValueError):
        tr.generation_step(esc.T, act_every=0)

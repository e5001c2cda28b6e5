"""BatchedPhysicsEnv.rollout_stochastic (wg_rollout_stochastic: the resident closed loop with seeded action noise in the
policy's output layer) against the CPU reference driven by pg.stochastic_forward_numpy on its own rows (tests/pg_cases.py),
with auto-reset off (the reference engine) and on (test_gpu_autoreset._Composed).  Every comparison is bitwise."""
import ctypes as C
import functools

import numpy as np
import pytest

import episode_cases as ec
import pg_cases as gc
import policy_cases as pc
from conftest import gpu_available

pytestmark = pytest.mark.gpu

CASES = pytest.mark.parametrize("name", gc.NAMES)
STATE = ("pos", "vel", "acc", "muscle_x", "steps", "contact")
OFF_STEP = ("obs", "reward", "done", "action", "raw", "eps")
ON_STEP = OFF_STEP + ("steps_t", "reset", "final_obs")
STATS = ("return_sum", "length_sum", "episodes", "tail_return", "tail_length", "ep_returns", "ep_lengths")
DEV = "cuda:0"


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
    case = gc.case_of(name)
    if not auto_reset:
        return BatchedPhysicsEnv(pc.spec_of(case.kind), device=DEV, **case.params)
    cfg = gc.config(name)
    env = BatchedPhysicsEnv(cfg["spec"], device=DEV, **cfg["params"])
    env.enable_auto_reset(on=("done",), noise=cfg["pool"], final_obs=True)
    return env


def _sigma(name):
    import torch
    return torch.from_numpy(gc.sigma_of(name).copy()).to(DEV)


def _buffers(env, Tn, Cc, auto_reset):
    import torch
    N, D = env.N, env.obs_dim
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)   # (a value the kernel failed to write cannot pass)
    ff = lambda *s: torch.full(s, 255, dtype=torch.uint8, device=DEV)
    buf = dict(obs_out=nan(Tn, N, D), reward_out=nan(Tn, N), done_out=ff(Tn, N), action_out=nan(Tn, N, Cc),
               raw_action_out=nan(Tn, N, Cc), eps_out=nan(Tn, N, Cc))
    if auto_reset:
        buf.update(steps_out=torch.full((Tn, N), -7, dtype=torch.int32, device=DEV), reset_out=ff(Tn, N),
                   final_obs_out=nan(Tn, N, D))
    return buf


_KEYS = dict(obs_out="obs", reward_out="reward", done_out="done", action_out="action", raw_action_out="raw",
             eps_out="eps", steps_out="steps_t", reset_out="reset", final_obs_out="final_obs")


def _host(buf):
    return {_KEYS[k]: v.cpu().numpy() for k, v in buf.items()}


def _state(env, auto_reset):
    st = {k: getattr(env, k).detach().cpu().numpy().copy() for k in STATE}
    if auto_reset:
        st["episodes"] = env.batch.episodes.detach().cpu().numpy().copy()
    return st


def _run(name, auto_reset, Tn, step_base=gc.STEP_BASE, seed=gc.SEED, buffers=True, env=None, slots=gc.SLOTS,
         walker_base=gc.WALKER_BASE, zeros=False, only=None):
    """One call on a fresh env (or `env`).  only: of the per-step buffers, the named ones alone."""
    import torch
    case = gc.case_of(name)
    env = _env(name, auto_reset) if env is None else env
    buf = _buffers(env, Tn, case.C, auto_reset) if buffers else {}
    if only is not None:
        buf = {k: v for k, v in buf.items() if k in only}
    kw = dict(episode_slots=slots) if auto_reset else {}
    sigma = torch.from_numpy(gc.sigma_of(name, zeros).copy()).to(DEV)
    res = env.rollout_stochastic(gc.policy_of(case, DEV), Tn, sigma, seed, step_base=step_base,
                                 walker_base=walker_base, **buf, **kw)
    torch.cuda.synchronize()
    out = dict(_host(buf), **_state(env, auto_reset))
    out["stats"] = {k: v.cpu().numpy() for k, v in res.items()}
    return out


@functools.lru_cache(maxsize=None)
def _off(name):
    """The fused run with every buffer and the one with none, auto-reset off (host copies, shared, never modified)."""
    case = gc.case_of(name)
    env = _env(name, False)
    geo = env.launch_geometry()   # the wave tile the case is there for
    assert geo["walkers_per_block"] * 64 // geo["threads"] == case.wpw, geo
    return _run(name, False, gc.T_OFF, env=env), _run(name, False, gc.T_OFF, buffers=False)


@functools.lru_cache(maxsize=None)
def _on(name):
    case = gc.case_of(name)
    env = _env(name, True)
    geo = env.launch_geometry()
    assert geo["walkers_per_block"] * 64 // geo["threads"] == case.wpw, geo
    return _run(name, True, gc.T_ON, env=env), _run(name, True, gc.T_ON, buffers=False, slots=0)


def _check_state(got, want, names):
    for k, r in names:
        assert _same(got[k], np.asarray(want[r]).reshape(got[k].shape).astype(got[k].dtype)), k
    assert np.array_equal(got["contact"].astype(np.uint8).ravel(), np.asarray(want["contact"]).astype(np.uint8).ravel())


def _check_off(fused, ref):
    for k in OFF_STEP:
        a, b = fused[k], np.ascontiguousarray(ref[k]).reshape(fused[k].shape)
        assert a.dtype == b.dtype and _same(a, b), k
    _check_state(fused, ref, [(k, k) for k in STATE[:-1]])
    assert _same(fused["stats"]["returns"], ref["returns"]) and _same(fused["stats"]["lengths"], ref["lengths"])


def _check_on(fused, ref):
    ref = dict(ref)
    ref["steps_t"] = ref["steps"]
    for k in ON_STEP:
        a, b = fused[k], np.ascontiguousarray(ref[k]).reshape(fused[k].shape)
        assert a.dtype == b.dtype and _same(a, b), k
    _check_state(fused, ref["state"], [("pos", "pos"), ("vel", "vel"), ("acc", "acc"), ("muscle_x", "mx"),
                                       ("steps", "steps"), ("episodes", "episodes")])
    for k in STATS:
        assert fused["stats"][k].dtype == ref["stats"][k].dtype and _same(fused["stats"][k], ref["stats"][k]), k


# ------------------------------------------------------------------ against the CPU reference
@CASES
def test_auto_reset_off_equals_reference_engine(name):
    """Every step's obs / reward / done / action / raw action / aeps, the final state, returns and lengths."""
    fused, _ = _off(name)
    _check_off(fused, gc.reference_off(name))
    assert set(fused["stats"]) == {"returns", "lengths"}


@CASES
def test_auto_reset_on_equals_composed_reference(name):
    """Per-step outputs including steps, reset and final_obs, the final state, episodes, every stats array (4 slots)."""
    fused, _ = _on(name)
    _check_on(fused, gc.reference_on(name))
    assert fused["reset"].sum(0).min() >= 2 and fused["reset"][-1].any()


@CASES
def test_no_buffer_runs_give_the_same_final_state(name):
    for auto_reset, (fused, bare) in ((False, _off(name)), (True, _on(name))):
        for k in STATE + (("episodes",) if auto_reset else ()):
            assert _same(fused[k], bare[k]), (auto_reset, k)
        for k in bare["stats"]:
            assert _same(fused["stats"][k], bare["stats"][k]), (auto_reset, k)
    assert set(_on(name)[1]["stats"]) == set(STATS[:5])


def test_weights_staged_and_through_l2(monkeypatch):
    """The shared policies' weights are staged in LDS by default and the others' read through L2 (the host's rule,
    restated by policy_cases.lds_bytes); a shared policy forced through L2 gives the staged run's bytes."""
    staged = {n: pc.lds_bytes(gc.case_of(n).pol)["staged"][1] for n in gc.NAMES}
    assert staged["canonical-h0-shared"] and staged["six-h5-c6-shared"], staged
    assert not staged["balance-h5-4sets"] and not staged["canonical4-h5-5sets"] and not staged["balance16-h0-perwalker"]
    assert not staged["canonical4-perwalker-c5-inf"] and not staged["wide-h5-c20-shared"]
    monkeypatch.setenv("WG_POLICY_STAGE", "0")
    for name in ("canonical-h0-shared", "six-h5-c6-shared"):
        l2 = _run(name, False, gc.T_OFF)
        fused, _ = _off(name)
        for k in OFF_STEP + STATE:
            assert _same(l2[k], fused[k]), (name, k)


# ------------------------------------------------------------------ every NZ instance
@pytest.mark.parametrize("auto_reset", [False, True], ids=["off", "ar"])
@pytest.mark.parametrize("edge8", [True, False], ids=["compact", "16-byte"])
@pytest.mark.parametrize("name", gc.COVER_NAMES)
def test_every_noise_instance_equals_reference(name, edge8, auto_reset, monkeypatch):
    """The NZ instance of walker_rollout_policy at every (IN3D, NE, E8, AR): pg_cases.COVER's batches (512 full tiles of
    16 walkers of M = 4, or of one of M = 64), the walkers per wave asserted from the launch geometry.  Without
    auto-reset every per-step buffer, the final state, returns and lengths; with it those buffers plus steps, reset and
    final_obs, the final state, episodes and every stats array.  Both record formats against one reference."""
    if not edge8:
        monkeypatch.setenv("WG_EDGE8", "0")
    case = gc.case_of(name)
    env = _env(name, auto_reset)
    geo = env.launch_geometry()
    assert geo["walkers_per_block"] * 64 // geo["threads"] == case.wpw, geo
    if auto_reset:
        _check_on(_run(name, True, gc.T_ON, env=env), gc.reference_on(name))
    else:
        _check_off(_run(name, False, case.t_off, env=env), gc.reference_off(name))


# ------------------------------------------------------------------ the edges of the noise's inputs
@pytest.mark.parametrize("auto_reset", [False, True], ids=["off", "ar"])
def test_largest_accepted_counters(auto_reset):
    """step_base + T = 2^32 and walker_base + N = 2^32, the largest counters wg_rollout_stochastic accepts, on the batch
    whose last tile is half full (the lanes past N of that tile wrap their 32-bit walker counter; they store nothing):
    every buffer equals the reference driven with the same counters, and the variates are not the usual run's."""
    name = gc.ZEROS
    case = gc.case_of(name)
    Tn = gc.T_ON if auto_reset else case.t_off
    env = _env(name, auto_reset)
    assert env.N % case.wpw != 0, "a partial last tile"
    sb, wb = gc.LAST - Tn, gc.LAST - env.N
    got = _run(name, auto_reset, Tn, step_base=sb, walker_base=wb, env=env)
    if auto_reset:
        _check_on(got, gc.reference_on(name, sb, wb))
    else:
        _check_off(got, gc.reference_off(name, gc.SEED, sb, wb))
    usual = (_on if auto_reset else _off)(name)[0]
    assert not _same(got["eps"], usual["eps"]) and not _same(got["action"], usual["action"])


def test_zero_sigma_entries():
    """A sigma whose set 1 is all zero and which has one zero column in every other set: bits against the reference, and
    where sigma is 0 and the chain value y is not zero, the raw action is y in bits (y from pg.policy_rows on the obs
    rows the previous step recorded).  At y == -0.0 the contract differs: u = RN32(-0.0 + RN32(0 * aeps))
    is +0.0 wherever the product is +0.0 (aeps >= 0) and -0.0 elsewhere, so those entries are left to the reference
    comparison."""
    import torch
    from walker_gym_amd import pg
    name = gc.ZEROS
    case = gc.case_of(name)
    got = _run(name, False, case.t_off, zeros=True)
    _check_off(got, gc.reference_off(name, gc.SEED, gc.STEP_BASE, gc.WALKER_BASE, True))
    assert not _same(got["raw"], _off(name)[0]["raw"])
    sg = gc.sigma_of(name, True)
    N = got["raw"].shape[1]
    zero = (sg == 0)[np.arange(N) // (N // case.G)]                     # [N, C]
    assert zero[N // case.G:2 * (N // case.G)].all() and zero.sum(1).min() == 1
    y = pg.policy_rows(gc.policy_of(case, DEV), torch.from_numpy(got["obs"][:-1].copy()).to(DEV)).cpu().numpy()
    raw = got["raw"][1:]                                                # step t acts on the rows step t - 1 recorded
    sel = zero[None] & (y != 0)
    assert sel.sum() > 0.9 * zero.sum() * len(y)
    assert np.array_equal(raw.view(np.uint32)[sel], y.view(np.uint32)[sel])
    rest = ~np.broadcast_to(zero[None], y.shape)                       # (and the other entries did get their noise)
    assert (raw.view(np.uint32)[rest] != y.view(np.uint32)[rest]).mean() > 0.9


@pytest.mark.parametrize("name,auto_reset,only", [("canonical4-h5-5sets", False, "raw_action_out"),
                                                  ("six-h5-c6-shared", True, "eps_out")])
def test_one_noise_buffer_at_a_time(name, auto_reset, only):
    """Only raw_action_out, or only eps_out (and no other per-step buffer): the buffer given carries the full run's
    bytes, and the final state and the call's statistics are the full run's."""
    full = (_on if auto_reset else _off)(name)[0]
    got = _run(name, auto_reset, gc.T_ON if auto_reset else gc.case_of(name).t_off, only=(only,))
    key = _KEYS[only]
    assert set(got) & set(_KEYS.values()) == {key}
    assert got[key].dtype == np.float32 and _same(got[key], full[key])
    for k in STATE + (("episodes",) if auto_reset else ()):
        assert _same(got[k], full[k]), k
    for k in full["stats"]:
        assert _same(got["stats"][k], full["stats"][k]), k


# ------------------------------------------------------------------ the counters
@CASES
def test_two_calls_of_8_equal_one_of_16(name):
    fused, _ = _on(name)
    env = _env(name, True)
    a = _run(name, True, 8, step_base=gc.STEP_BASE, env=env)
    b = _run(name, True, 8, step_base=gc.STEP_BASE + 8, env=env)
    for k in ON_STEP:
        assert _same(np.concatenate([a[k], b[k]]), fused[k]), k
    for k in STATE + ("episodes",):
        assert _same(b[k], fused[k]), k
    c = _run(name, True, 8, step_base=gc.STEP_BASE, env=env)   # the same counters again: other states, the same variates
    assert _same(c["eps"], a["eps"]) and not _same(c["action"], a["action"])


@pytest.mark.parametrize("name,auto_reset", [("canonical-h0-shared", False), ("six-h5-c6-shared", True)])
def test_second_half_with_walker_base_equals_the_full_run(name, auto_reset):
    """A batch of walkers [N / 2, N) (a walker-range view of the state: the same arrays, pointers offset) with
    walker_base + N / 2 gives the second half of the full run: outputs, actions, variates and state."""
    import torch
    from walker_gym_amd import _lib
    from walker_gym_amd.batched_env import BatchedPhysicsEnv
    case = gc.case_of(name)
    fused = (_on if auto_reset else _off)(name)[0]
    Tn = gc.T_ON if auto_reset else gc.T_OFF
    env = _env(name, auto_reset)
    N, D, Cc, M, A = env.N, env.obs_dim, case.C, env.batch.M, env.batch.A
    h = N // 2
    pol, sg = gc.policy_of(case, DEV), _sigma(name)
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)
    obs, act, raw, eps = nan(Tn, N, D), nan(Tn, N, Cc), nan(Tn, N, Cc), nan(Tn, N, Cc)
    reset = torch.full((Tn, N), 255, dtype=torch.uint8, device=DEV)
    o = env._outputs(obs, None, None, None, None, obs_step=N * D, out_step=N, pad_clean=True,
                     reset=reset if auto_reset else None)
    o = BatchedPhysicsEnv._range_outputs(o, h)
    ps = pol.struct(N, act)                                    # (the full buffers' step stride; rows from walker h on)
    ps.action_out = C.c_void_p(act.data_ptr() + 4 * h * Cc)
    nz = _lib.WgActionNoise(seed=gc.SEED, step_base=gc.STEP_BASE, walker_base=gc.WALKER_BASE + h, sigma=_lib.ptr(sg),
                            raw_out=C.c_void_p(raw.data_ptr() + 4 * h * Cc), raw_out_step=N * Cc,
                            eps_out=C.c_void_p(eps.data_ptr() + 4 * h * Cc), eps_out_step=N * Cc)
    st = C.byref(_lib.WgEpisodeStats()) if auto_reset else None
    sub = env.batch.sub_struct(h, N)
    _lib.check(_lib.load().wg_rollout_stochastic(C.byref(sub), C.byref(env._pstruct), C.byref(ps), C.byref(nz),
                                                 C.byref(o), st, Tn, env._stream()), "wg_rollout_stochastic")
    torch.cuda.synchronize()
    for got, k in ((obs, "obs"), (act, "action"), (raw, "raw"), (eps, "eps")) + (((reset, "reset"),) if auto_reset else ()):
        g = got.cpu().numpy()
        assert _same(g[:, h:], fused[k][:, h:]), k
        assert (np.isnan(g[:, :h]).all() if g.dtype == np.float32 else (g[:, :h] == 255).all()), k   # nothing else written
    per = dict(pos=3 * M, vel=3 * M, acc=3 * M, muscle_x=A, steps=1, contact=M)
    fresh = _state(_env(name, auto_reset), auto_reset)
    for k, n in per.items():
        g = getattr(env, k).cpu().numpy().reshape(-1)
        assert _same(g[h * n:], fused[k].reshape(-1)[h * n:]), k
        assert _same(g[:h * n], fresh[k].reshape(-1)[:h * n]), k   # the first half was not stepped


@pytest.mark.parametrize("name", ["balance-h5-4sets", "canonical4-h5-5sets"])
def test_another_seed_changes_the_actions(name):
    fused, _ = _off(name)
    other = _run(name, False, gc.T_OFF, seed=gc.SEED + 1)
    ref = gc.reference_off(name, gc.SEED + 1)
    assert not _same(other["eps"], fused["eps"]) and not _same(other["action"], fused["action"])
    for k in OFF_STEP:
        assert _same(other[k], np.ascontiguousarray(ref[k]).reshape(other[k].shape)), k


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
        rg.rollout_stochastic(MLPPolicy(z(rg.obs_dim, 2)), 2, 0.1, 1)
    pf = BatchedPhysicsEnv(canonical_walkers(256, seed=2), device=DEV, in3d=1, pair_mode=1)
    with pytest.raises(ValueError, match="resident lean kernel"):            # pair forces
        pf.rollout_stochastic(MLPPolicy(z(152, 8)), 2, 0.1, 1)
    env = BatchedPhysicsEnv(canonical_walkers(256, seed=2), device=DEV, in3d=1, max_steps=3)
    good = MLPPolicy(z(152, 8))
    env.step(z(256, 8))
    bad = [dict(sigma=None), dict(sigma=z(2, 8)), dict(sigma=torch.zeros(1, 8)), dict(seed=-1), dict(seed=1 << 64),
           dict(step_base=(1 << 32) - 1), dict(walker_base=(1 << 32) - 255), dict(n_steps=0), dict(episode_slots=2),
           dict(reset_out=torch.zeros((2, 256), dtype=torch.uint8, device=DEV)), dict(final_obs_out=z(2, 256, 152)),
           dict(eps_out=z(2, 256, 7)), dict(raw_action_out=z(3, 256, 8)), dict(steps_out=z(2, 256)),
           dict(policy=MLPPolicy(z(151, 8))), dict(policy=MLPPolicy(z(3, 152, 8))), dict(policy=lambda rows, t: rows)]
    for kw in bad:
        args = dict(policy=good, n_steps=2, sigma=0.1, seed=1)
        args.update(kw)
        with pytest.raises(ValueError):
            env.rollout_stochastic(**args)
    assert "total_energy" in env.info()                                      # a refused call marks nothing stale
    # st in the wrong mode, and a missing sigma, at the C boundary
    pol, L = good.struct(256), _lib.load()
    sg = z(1, 8)
    nz = _lib.WgActionNoise(seed=1, sigma=_lib.ptr(sg))
    call = lambda e, nz, st: L.wg_rollout_stochastic(C.byref(e.batch.struct), C.byref(e._pstruct), C.byref(pol),
                                                     None if nz is None else C.byref(nz), None, st, 2, e._stream())
    assert call(env, nz, C.byref(_lib.WgEpisodeStats())) == _lib.WG_EINVAL and b"st must be NULL" in L.wg_last_error()
    assert call(env, _lib.WgActionNoise(seed=1), None) == _lib.WG_EINVAL and b"sigma" in L.wg_last_error()
    assert call(env, None, None) == _lib.WG_EINVAL
    env.enable_auto_reset()
    assert call(env, nz, None) == _lib.WG_EINVAL and b"null episode stats" in L.wg_last_error()
    # the env still steps, and an accepted call marks the one-step outputs stale
    ref = BatchedPhysicsEnv(canonical_walkers(256, seed=2), device=DEV, in3d=1, max_steps=3)
    ref.step(z(256, 8))
    ref.enable_auto_reset()                                                  # (as env: the snapshot after one step)
    r = env.rollout_stochastic(good, 4, 0.0, 1)                              # sigma 0 on zero weights: zero actions
    for t in range(4):
        ref.step(z(256, 8))
    torch.cuda.synchronize()
    assert (r["episodes"] == 1).all() and (r["length_sum"] == 2).all() and (r["tail_length"] == 2).all()
    for k in STATE:
        assert _same(getattr(env, k), getattr(ref, k)), k
    assert "total_energy" not in env.info()
    assert _same(env.step(z(256, 8))[0], ref.step(z(256, 8))[0]) and "total_energy" in env.info()


@pytest.mark.parametrize("auto_reset", [False, True])
def test_deterministic_entries_keep_their_bytes(auto_reset):
    """rollout_policy / rollout_episodes give, after a stochastic call on the same env, the bytes they gave before it."""
    import torch
    name = "canonical4-h5-5sets"
    case = gc.case_of(name)
    env = _env(name, auto_reset)
    pol = gc.policy_of(case, DEV)
    state0 = env.batch.state_dict()

    def restore():
        env.batch.load_state_dict(state0)
        if auto_reset:
            env.batch.episodes.zero_()

    def deterministic():
        restore()
        N, D = env.N, env.obs_dim
        buf = dict(obs_out=torch.full((6, N, D), float("nan"), device=DEV),
                   action_out=torch.full((6, N, case.C), float("nan"), device=DEV))
        res = env.rollout_episodes(pol, 6, **buf) if auto_reset else env.rollout_policy(pol, 6, **buf)
        torch.cuda.synchronize()
        return [v.cpu().numpy() for v in buf.values()] + [v.cpu().numpy() for v in res.values()] + \
            list(_state(env, auto_reset).values())
    before = deterministic()
    restore()
    env.rollout_stochastic(pol, 6, _sigma(name), gc.SEED)
    after = deterministic()
    assert len(before) == len(after) and all(_same(a, b) for a, b in zip(before, after))

"""Diverged walkers on every instance that carries the stand-in path (tests/diverged_cases.py: the kinds, their places in
a wave tile, the shapes; tests/test_diverged_cases_cpu.py holds on the oracle alone that the cases are what they are meant
to be).  The ground is at the batch's median height, so the contact flags (and radii) of a dead walker's first step are
those of the y it started from: not zero where its NaN is in x or z only.

Everything is compared with the C oracle bit for bit (uint32 views); a NaN equals a NaN whatever its payload; contact,
done, steps, reset and radius exactly.  Which instance a launch takes is the host's arithmetic: every test asserts the
walkers per wave, the pass count and the record format against launch_geometry(), and the FIX / WT launch counters
around its calls."""
import numpy as np
import pytest

import diverged_cases as D
import episode_cases as ec
import param_cases as P
import pg_cases as gc
import policy_cases as pc
from conftest import gpu_available
from test_gpu_edge8 import STATE, _bits, _compact, _outs, _state

pytestmark = pytest.mark.gpu
OUT = ("obs", "reward", "done", "centroid", "energy")


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
    sel = D.select(shape)
    geo = env.launch_geometry()
    wpw = geo["walkers_per_block"] // (geo["threads"] // 64)
    assert wpw == sel["wpw"], geo
    assert (wpw * env.batch.K + 63) // 64 == sel["passes"]
    assert env.batch.edges8 is not None and _compact(env) == sel["compact"]
    return sel


def _same(got, ref, what):
    """Bit for bit, NaN == NaN in float arrays; integer arrays exactly."""
    got, ref = np.asarray(got), np.asarray(ref)
    if got.dtype == np.float32 or ref.dtype == np.float32:
        _bits(got, ref, what, nan_ok=True)
    else:
        assert np.array_equal(got.ravel().astype(np.int64), ref.ravel().astype(np.int64)), what


def _radius(env):
    return env.batch.caller("radius").cpu().numpy()


def _check(got, st, ref, what, env=None):
    for k in OUT:
        _same(got[k], ref[k], f"{what} {k}")
    for k in STATE:
        _same(st[k], ref[k], f"{what} {k}")
    if env is not None and env.batch.radius is not None:
        assert np.array_equal(_radius(env), ref["radius"]), f"{what} radius"


def _env(spec, params, radius=False):
    from walker_gym_amd.batched_env import BatchedPhysicsEnv
    env = BatchedPhysicsEnv(spec, **params)
    if radius:   # Point.r on the device: the step writes 3 / 1 with the contact flag; no FIX instance takes such a batch
        env.batch.enable_radius()
    return env


def _steps(env, acts, refs, what):
    for t, ref in enumerate(refs):
        got = _outs(*env.step(acts[t]))
        _check(got, _state(env), ref, f"{what} step {t + 1}", env)


# ---------------------------------------------------------------- walker_step_lean1 / walker_step_lean, generic, FIX, WT
STEP_CELLS = [(s, d, False) for s, d in D.cells()] + [(s, d, True) for s in ("ne3", "ne1") for d in (0, 1)]


@pytest.mark.parametrize("cell", STEP_CELLS, ids=lambda c: D.cell_id(c) + ("-radius" if c[2] else ""))
def test_step(monkeypatch, cell):
    """Three closed-loop step()s on the default path (FIX / WT where the shape has full tiles and the batch no pins or
    radii), under WG_EDGE8=0, and for the FIX shapes under WG_FIX=0 and WG_WT=0; then one run() of three steps over two
    walker ranges.  The radius variant has dead-pinned walkers and a radius array: the generic instance."""
    import torch
    shape, in3d, radius = cell
    kw = D.SHAPES[shape]
    pins = True if radius else None
    spec, params, kinds = D.case(shape, in3d, pins)
    ref = D.scripted(shape, in3d, pins)
    refs, acts = ref["steps"], D.actions(shape, D.STEPS)
    assert np.array_equal(kinds, ref["kinds"])
    fixp = not radius and not D.pins_of(shape)            # lean_fix_ok admits the batch
    want = D.STEPS * np.array([fixp and D.fix_expected(shape), fixp and D.wt_expected(shape, in3d)], int)

    c0 = _counters()
    env = _env(spec, params, radius)
    _assert_instance(env, shape)
    assert env._step_lanes() == 1
    _steps(env, acts, refs, "default")
    c1 = _counters()
    assert (c1 - c0 == want).all(), (c1 - c0, "FIX / WT launches of the steps")
    arms = [("WG_EDGE8", [0, 0])]
    if want[0]:   # the control arms: the generic instance on the compact records, then FIX with its own epilogue
        arms += [("WG_FIX", [0, 0]), ("WG_WT", [want[0], 0])]
    for knob, launches in arms:
        monkeypatch.setenv(knob, "0")
        c2 = _counters()
        _steps(_env(spec, params, radius), acts, refs, f"{knob}=0")
        assert (_counters() - c2 == launches).all(), f"{knob}=0: FIX / WT launches"
        monkeypatch.delenv(knob)

    # run(): every range is a batch of its own to the selector (the keep_aux flip at its last step)
    ranges = P.run_ranges(kw["N"])
    runner = _env(spec, params, radius)
    assert runner._lanes(2) == len(ranges)
    c3 = _counters()
    runner.run(torch.as_tensor(acts, device="cuda"), D.STEPS, lanes=2)
    st = _state(runner)
    want = sum(D.STEPS * np.array([P.fix_expected(n, kw["M"], kw["K"], fixp),
                                   P.wt_expected(n, kw["M"], kw["K"], kw["A"], in3d, fixp)], int) for n in ranges)
    assert (_counters() - c3 == want).all(), "FIX / WT launches of run()"
    got = dict(obs=runner.obs, reward=runner.reward, done=runner.done, centroid=runner.centroid, energy=runner.energy)
    _check({k: t.cpu().numpy() for k, t in got.items()}, st, refs[-1], "run()", runner)


# ---------------------------------------------------------------- walker_rollout_lean
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("cell", D.cells(), ids=D.cell_id)
def test_resident(monkeypatch, cell, T):
    """rollout(resident=True) of one step (the resident kernel stores contact after its last step only) and of three,
    with the compact records and under WG_EDGE8=0.  NE 1 runs the stand-in path; NE > 1 has none and reaches the same
    bits on the plain path.  dead-pinned walkers at every shape (the resident kernel has no FIX instance)."""
    import torch
    shape, in3d = cell
    spec, params, _ = D.case(shape, in3d, True)
    refs = D.scripted(shape, in3d, True)["steps"]
    acts = torch.as_tensor(D.actions(shape, D.STEPS)[:T], device="cuda")
    c0 = _counters()
    for edge8 in ("1", "0"):
        monkeypatch.setenv("WG_EDGE8", edge8)
        env = _env(spec, params)
        _assert_instance(env, shape)
        assert env.resident_ok()
        obs, rew, done = env.rollout(acts, resident=True)
        st = _state(env)
        monkeypatch.delenv("WG_EDGE8")
        for t in range(T):
            _same(obs[t].cpu().numpy(), refs[t]["obs"], f"step {t + 1} obs (WG_EDGE8={edge8})")
            _same(rew[t].cpu().numpy(), refs[t]["reward"], f"step {t + 1} reward (WG_EDGE8={edge8})")
            _same(done[t].cpu().numpy(), refs[t]["done"], f"step {t + 1} done (WG_EDGE8={edge8})")
        for k in STATE:
            _same(st[k], refs[T - 1][k], f"{k} after {T} steps (WG_EDGE8={edge8})")
    assert (_counters() == c0).all()


# ---------------------------------------------------------------- the AR instances of both
def _ar_env(cfg, shape):
    env = _env(cfg["spec"], cfg["params"])
    env.enable_auto_reset(on=("done",), noise=cfg["pool"], final_obs=True)   # (not "nonfinite": the dead stay dead)
    _assert_instance(env, shape)
    return env


@pytest.mark.parametrize("cell", [(s, d) for s in D.FULL for d in (0, 1)], ids=D.cell_id)
def test_auto_reset(monkeypatch, cell):
    """The AR instances of the step kernel (a step() loop of six) and of the resident kernel (rollouts of one step and
    of six), both record formats, against the composed oracle.  A dead walker whose episode ends by the step limit goes
    back to its dead snapshot."""
    import torch
    from test_gpu_autoreset import _check_outputs, _check_state
    from test_gpu_parity import _close
    shape, in3d = cell
    cfg, ref = D.ar_config(shape, in3d), D.ar_reference(shape, in3d)
    N = cfg["N"]
    c0 = _counters()
    for edge8 in ("1", "0"):
        monkeypatch.setenv("WG_EDGE8", edge8)
        env = _ar_env(cfg, shape)
        for t in range(D.AR_STEPS):
            env.step(cfg["acts"][t])
            torch.cuda.synchronize()
            _check_state(env, ref[t]["state"])
            _check_outputs(env, ref[t]["out"], ref[t]["state"])
        for T in (1, D.AR_STEPS):
            env = _ar_env(cfg, shape)
            assert env.resident_ok()
            reset = torch.full((T, N), 7, dtype=torch.uint8, device=env.device)
            obs, rew, done = env.rollout(torch.from_numpy(cfg["acts"][:T]).to(env.device), resident=True,
                                         reset_out=reset)
            torch.cuda.synchronize()
            _close(obs.cpu().numpy(), np.stack([s["out"]["obs"] for s in ref[:T]]))
            _close(rew.cpu().numpy(), np.stack([s["out"]["reward"] for s in ref[:T]]))
            assert np.array_equal(done.cpu().numpy(), np.stack([s["out"]["done"] for s in ref[:T]]))
            assert np.array_equal(reset.cpu().numpy(), np.stack([s["out"]["reset"] for s in ref[:T]]))
            _check_state(env, ref[T - 1]["state"])
        monkeypatch.delenv("WG_EDGE8")
    assert (_counters() == c0).all()   # no AR and FIX instance


# ---------------------------------------------------------------- walker_rollout_policy, its AR and NZ twins
def _policy_buffers(env, T, C, auto_reset, noise):
    import torch
    N, Dm, dv = env.N, env.obs_dim, env.device
    nan = lambda *s: torch.full(s, float("nan"), device=dv)   # (a value the kernel failed to write cannot pass)
    ff = lambda *s: torch.full(s, 255, dtype=torch.uint8, device=dv)
    buf = dict(obs_out=nan(T, N, Dm), reward_out=nan(T, N), done_out=ff(T, N), action_out=nan(T, N, C))
    if noise:
        buf.update(raw_action_out=nan(T, N, C), eps_out=nan(T, N, C))
    if auto_reset:
        buf.update(reset_out=ff(T, N), final_obs_out=nan(T, N, Dm))
        if noise:
            buf.update(steps_out=torch.full((T, N), -7, dtype=torch.int32, device=dv))
    return buf


_KEYS = dict(obs_out="obs", reward_out="reward", done_out="done", action_out="action", raw_action_out="raw",
             eps_out="eps", steps_out="steps_t", reset_out="reset", final_obs_out="final_obs")


@pytest.mark.parametrize("T", D.POLICY_T)
@pytest.mark.parametrize("noise", [False, True], ids=["det", "nz"])
@pytest.mark.parametrize("auto_reset", [False, True], ids=["off", "ar"])
@pytest.mark.parametrize("case", pc.COVER, ids=lambda c: c.name)
def test_policy_rollout(monkeypatch, case, auto_reset, noise, T):
    """walker_rollout_policy at every (IN3D, NE, E8), deterministic and with noise, auto-reset off and on, for one step
    (the kernel stores contact after its last step only) and for four: every per-step buffer, the final state and the
    call's statistics against the reference engine (auto-reset off) or the composed reference (on)."""
    import torch
    cfg, ref = D.policy_config(case.name, auto_reset), D.policy_reference(case.name, auto_reset, noise)
    pol = pc.policy_of(case, "cuda:0")
    sigma = torch.from_numpy(gc.sigma_of(case.name).copy()).to("cuda:0") if noise else None
    for edge8 in ("1", "0"):
        monkeypatch.setenv("WG_EDGE8", edge8)
        env = _env(cfg["spec"], dict(cfg["params"], device="cuda:0"))
        if auto_reset:
            env.enable_auto_reset(on=("done",), noise=cfg["pool"], final_obs=True)
        geo = env.launch_geometry()
        assert geo["walkers_per_block"] * 64 // geo["threads"] == case.wpw, geo
        assert env.batch.edges8 is not None
        buf = _policy_buffers(env, T, case.C, auto_reset, noise)
        kw = dict(episode_slots=ec.SLOTS) if auto_reset else {}
        if noise:
            res = env.rollout_stochastic(pol, T, sigma, gc.SEED, step_base=gc.STEP_BASE, walker_base=gc.WALKER_BASE,
                                         **buf, **kw)
        elif auto_reset:
            res = env.rollout_episodes(pol, T, **buf, **kw)
        else:
            res = env.rollout_policy(pol, T, **buf)
        torch.cuda.synchronize()
        monkeypatch.delenv("WG_EDGE8")
        what = f"(WG_EDGE8={edge8})"
        for k, v in buf.items():
            _same(v.cpu().numpy(), ref[_KEYS[k]][:T], f"{_KEYS[k]} {what}")
        st, want = _state(env), ref["states"][T - 1]
        for k in STATE:
            _same(st[k], want[k], f"{k} after {T} steps {what}")
        stats = {}
        with np.errstate(all="ignore"):
            if auto_reset:
                _same(env.batch.episodes.cpu().numpy(), want["episodes"], f"episodes {what}")
                stats = ec.accounting(ref["reward"][:T], ref["reset"][:T], ec.SLOTS)
            elif noise:
                stats["returns"], stats["lengths"] = pc.returns_lengths(ref["reward"][:T], ref["done"][:T])
        if isinstance(res, dict):
            assert set(stats) <= set(res) or not stats, (sorted(stats), sorted(res))
            for k, v in stats.items():
                _same(res[k].cpu().numpy(), v, f"stats {k} {what}")


# ---------------------------------------------------------------- walker_step_waves
@pytest.mark.parametrize("in3d", [0, 1])
@pytest.mark.parametrize("ne", [1, 2, 3, 4, 8])
def test_waves(monkeypatch, ne, in3d):
    """walker_step_waves at every (IN3D, NE): test_gpu_ragged's mixed batches sixteen times over, the kinds placed by walker
    slot of the planned wave tiles, with pins and a radius array; in the caller's order against the oracle, and against
    the workgroup kernel (WG_LEAN=0), which has no stand-in path."""
    import torch
    from oracle.oracle import Oracle
    from test_gpu_ragged import _wave_spec
    from walker_gym_amd import _lib
    spec, params, kinds, tiles = D.wave_case(_wave_spec(ne), in3d, 701 + 10 * ne)
    N = len(spec["mass_off"]) - 1
    M, K = int(np.diff(spec["mass_off"]).max()), int(np.diff(spec["edge_off"]).max())
    assert _lib.load().wg_wave_edge_passes(M, K) == ne
    dead = np.isin(kinds, D.DEAD)
    assert dead.sum() >= D.MIN_DEAD and (~dead).sum() >= D.MIN_DEAD
    acts = np.random.default_rng(74).uniform(-1, 1, (D.STEPS, N, int(np.max(spec["n_muscles"])))).astype(np.float32)
    env = _env(spec, params, radius=True)
    assert env.batch.ragged_kind == 2
    # the placement was by the tiles the launch has: the plan's tiles are diverged_cases.wave_tiles'
    plan, row = env.batch.plan_host, np.asarray(env.batch.host.row)
    assert len(plan) == len(tiles) + 1
    for i, t in enumerate(tiles):
        assert np.array_equal(row[plan[i]:plan[i + 1]], t), f"wave tile {i}"
    if max(len(t) for t in tiles) > 1:
        some = [dead[t] for t in tiles if len(t) > 1]
        assert any(d[0] and not d[1:].any() for d in some) and any(d[-1] and not d[:-1].any() for d in some)
        assert any(d.all() for d in some) and any(not d.any() for d in some)
    monkeypatch.setenv("WG_LEAN", "0")
    wg = _env(spec, params, radius=True)
    monkeypatch.delenv("WG_LEAN")
    assert wg.batch.ragged_kind == 1
    orc = Oracle(spec, params, n_threads=8)
    for t in range(D.STEPS):
        ref = orc.step(acts[t])
        ref = dict(ref, pos=orc.pos, vel=orc.vel, acc=orc.acc, muscle_x=orc.mx, steps=orc.steps, contact=orc.contact,
                   radius=orc.radius)
        for name, e in (("waves", env), ("workgroup", wg)):
            got = _outs(*e.step(acts[t]))
            torch.cuda.synchronize()
            _check(got, _state(e), ref, f"{name} step {t + 1}", e)
    # the stand-in path ran: NaN in every component of every mass (a drawn walker may have a mass without a spring,
    # which keeps its finite components: such a walker is not dead to the kernel either)
    mo = np.asarray(spec["mass_off"])
    gone = np.array([np.isnan(orc.pos[mo[w]:mo[w + 1]]).all() for w in range(N)])
    assert (gone & dead).sum() >= D.MIN_DEAD


# ---------------------------------------------------------------- the kernels without the path
def test_workgroup_kernel_and_pair_forces(monkeypatch):
    """M = 25 walkers on the workgroup kernel (WG_LEAN=0) and a pair-force batch on the lean kernel (pair_mode 3: the
    stand-in path is off): both compute the contact on the plain path and agree with the oracle on the new cases."""
    from oracle.oracle import Oracle
    from walker_gym_amd.synthetic import canonical_walkers
    for build, extra, pins, lean in ((lambda: canonical_walkers(200, seed=8, M=25, K=60, A=10), {}, True, "0"),
                                     (lambda: canonical_walkers(256, seed=9), dict(pair_mode=3), False, "1")):
        base = build()
        N = len(base["mass_off"]) - 1
        spec, params, kinds = D.diverge(base, 1, D.tile_groups(N, 4), 900 + int(lean), pins)
        params = dict(params, **extra)
        if extra:
            spec["charge"] = np.full(len(spec["m"]), 1e-6)
        assert np.isin(kinds, D.DEAD).sum() >= D.MIN_DEAD
        acts = np.random.default_rng(8).uniform(-1, 1, (D.STEPS, N, int(np.max(spec["n_muscles"])))).astype(np.float32)
        monkeypatch.setenv("WG_LEAN", lean)
        env = _env(spec, params)
        monkeypatch.delenv("WG_LEAN")
        orc = Oracle(spec, params, n_threads=8)
        for t in range(D.STEPS):
            ref = orc.step(acts[t])
            ref = dict(ref, pos=orc.pos, vel=orc.vel, acc=orc.acc, muscle_x=orc.mx, steps=orc.steps,
                       contact=orc.contact, radius=orc.radius)
            _check(_outs(*env.step(acts[t])), _state(env), ref, f"WG_LEAN={lean} step {t + 1}", env)

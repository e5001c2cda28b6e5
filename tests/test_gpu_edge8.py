"""The lean kernels on the compact 8-byte spring records (wg_edge8) and without the acc / contact stores of the steps
before a multi-step call's last: every output and the whole state bit for bit (rtol = atol = 0) against the C oracle
and against the same env under WG_EDGE8=0 (the 16-byte records).

A lean launch reads the compact records only with its standard tile of 64 / M walkers per wave; batches of fewer
than 512 such tiles get halved tiles and keep the 16-byte records.  So every case runs at its smallest shape (the
16-byte path with the compact records present) and, where the compact path is the point, at the smallest batch that
reaches it: 512 full tiles and one more holding a single walker (`compact` asserts which path the launch takes)."""
import numpy as np
import pytest

from conftest import gpu_available

pytestmark = pytest.mark.gpu

STATE = ("pos", "vel", "acc", "muscle_x", "steps", "contact")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.skip("no ROCm GPU")


def _bits(a, b, what, nan_ok=False):
    """Equal bit patterns; nan_ok: a NaN equals a NaN whatever its payload (the pair forces' diverged walkers only)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.size == b.size, what
    b = b.reshape(a.shape)
    both_nan = False
    if a.dtype == np.float32 or b.dtype == np.float32:
        a, b = a.astype(np.float32), b.astype(np.float32)
        if nan_ok:
            both_nan = np.isnan(a) & np.isnan(b)
        a, b = a.view(np.uint32), b.view(np.uint32)
    bad = (a != b) & ~both_nan
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ"


def _compact(env) -> bool:
    """The step launch of the whole batch reads the compact records: they exist and the tile is 64 / M walkers."""
    b, geo = env.batch, env.launch_geometry()
    return b.edges8 is not None and geo["walkers_per_block"] == (64 // b.M) * (geo["threads"] // 64)


def _state(env):
    import torch
    torch.cuda.synchronize()
    return {k: getattr(env, k).cpu().numpy().copy() for k in STATE}


def _outs(obs, rew, done, info):
    return dict(obs=obs.cpu().numpy().copy(), reward=rew.cpu().numpy().copy(),
                done=done.cpu().numpy().astype(np.uint8), centroid=info["centroid_position"].cpu().numpy().copy(),
                energy=info["total_energy"].cpu().numpy().copy())


def _against_oracle(got, st, ref, orc, t, nan_ok=False):
    for k in ("obs", "reward", "done", "centroid", "energy"):
        _bits(got[k], ref[k], f"step {t} {k} vs oracle", nan_ok)
    for k, o in (("pos", orc.pos), ("vel", orc.vel), ("acc", orc.acc), ("muscle_x", orc.mx), ("steps", orc.steps),
                 ("contact", orc.contact)):
        _bits(st[k], o, f"step {t} {k} vs oracle", nan_ok and k not in ("steps", "contact"))


def _step_case(monkeypatch, spec, params, T, compact, seed=11, acts=None, nan_ok=False):
    """T closed-loop steps: the default build path, the same env under WG_EDGE8=0, and the oracle.  acts: the [T, N, A]
    actions instead of seeded uniform ones; nan_ok: see _bits.  An env with radii (the bounce pass rewrites them)
    has them compared exactly too."""
    from oracle.oracle import Oracle
    from walker_gym_amd.batched_env import BatchedPhysicsEnv
    env, env0 = BatchedPhysicsEnv(spec, **params), BatchedPhysicsEnv(spec, **params)
    orc = Oracle(spec, params, n_threads=8)
    assert _compact(env) == compact
    A = env.batch.A
    if acts is None:
        acts = np.random.default_rng(seed).uniform(-1, 1, (T, env.N, max(A, 1))).astype(np.float32)
    for t in range(T):
        a = acts[t] if A else None
        got = _outs(*env.step(a))
        st = _state(env)
        monkeypatch.setenv("WG_EDGE8", "0")
        got0 = _outs(*env0.step(a))
        st0 = _state(env0)
        monkeypatch.delenv("WG_EDGE8")
        ref = orc.step(a)
        _against_oracle(got, st, ref, orc, t, nan_ok)
        for k in got:
            _bits(got[k], got0[k], f"step {t} {k} vs WG_EDGE8=0", nan_ok)
        for k in st:
            _bits(st[k], st0[k], f"step {t} {k} vs WG_EDGE8=0", nan_ok)
        if env.batch.radius is not None:
            for e in (env, env0):
                assert np.array_equal(e.batch.radius.cpu().numpy(), orc.radius), f"step {t} radius"
    return env


def _canonical(n, **kw):
    from walker_gym_amd.synthetic import canonical_walkers
    return canonical_walkers(n, seed=5, **kw)


# 512 full tiles of 4 canonical walkers and one more holding a single walker: its 40 springs are fewer than a pass's 64
# lanes (the load clamps, the half-filled passes)
N_CANON = 2049


@pytest.mark.parametrize("n,compact", [(5, False), (4, False), (N_CANON, True)])
def test_canonical(monkeypatch, n, compact):
    _step_case(monkeypatch, _canonical(n), dict(in3d=1), 5, compact)


@pytest.mark.parametrize("n,compact", [(17, False), (512 * 16 + 1, True)])
def test_balance(monkeypatch, n, compact):
    """Balance-v0 (M = 4, K = 5, 2D).  N = 17: halved tiles of one spring pass, the preloaded walker_step_lean1 entry
    on the 16-byte records; 8,193: 16 walkers per wave (80 springs, two passes) and a 1-walker tile, compact."""
    from walker_gym_amd.walker import balance_spec
    env = _step_case(monkeypatch, balance_spec(n), dict(in3d=0), 5, compact)
    assert env.batch.M == 4 and env.batch.K == 5


@pytest.mark.parametrize("in3d", [0, 1])
def test_lean1_compact(monkeypatch, in3d):
    """The preloaded one-pass entry (walker_step_lean1) on the compact records: M = 4, K = 4 is 64 springs per full
    tile of 16 walkers; 512 such tiles and a 1-walker tile."""
    env = _step_case(monkeypatch, _canonical(512 * 16 + 1, M=4, K=4, A=2), dict(in3d=in3d), 5, True)
    assert 16 * env.batch.K <= 64


@pytest.mark.parametrize("n,compact", [(5, False), (N_CANON, True)])
def test_no_muscles(monkeypatch, n, compact):
    _step_case(monkeypatch, _canonical(n, A=0), dict(in3d=1), 3, compact)


@pytest.mark.parametrize("n,compact", [(5, False), (N_CANON, True)])
def test_slack_string(monkeypatch, n, compact):
    """String springs (muscles and skeleton springs) whose rest length exceeds their current length: no force."""
    spec = _canonical(n)
    E = len(spec["rest"])
    fl = (np.arange(E) % 5 == 2)
    spec["flags"] = fl.astype(np.uint8)
    spec["rest"] = np.where(fl, spec["rest"] * np.float32(1.5), spec["rest"]).astype(np.float32)
    _step_case(monkeypatch, spec, dict(in3d=1), 3, compact)


@pytest.mark.parametrize("n,compact", [(5, False), (N_CANON, True)])
def test_two_classes(monkeypatch, n, compact):
    spec = _canonical(n)
    mus = (np.arange(len(spec["k"])) % 40) < 8
    spec["k"] = np.where(mus, 1000.0, 50.0).astype(np.float32)
    env = _step_case(monkeypatch, spec, dict(in3d=1), 3, compact)
    assert tuple(env.batch.kc) == (1000.0, 20.0, 50.0, 20.0)


def test_three_k_not_eligible(monkeypatch):
    """Three stiffness values: no compact records, the 16-byte path, the same results."""
    spec = _canonical(N_CANON)
    spec["k"] = np.array([1000.0, 50.0, 75.0], np.float32)[np.arange(len(spec["k"])) % 3]
    env = _step_case(monkeypatch, spec, dict(in3d=1), 3, False)
    assert env.batch.edges8 is None and not env.batch.struct.edges8


def test_set_springs_on_device(monkeypatch):
    """k edited through the API after packing: the compact records follow (two classes), then are dropped (three)."""
    from oracle.oracle import Oracle
    from walker_gym_amd.batched_env import BatchedPhysicsEnv
    spec = _canonical(N_CANON)
    E = len(spec["k"])
    mus = (np.arange(E) % 40) < 8
    k2 = np.where(mus, 1000.0, 50.0).astype(np.float32)
    k3 = k2.copy()
    k3[np.arange(E) % 40 == 20] = 75.0
    env = BatchedPhysicsEnv(spec, in3d=1)
    acts = np.random.default_rng(2).uniform(-1, 1, (2, env.N, 8)).astype(np.float32)
    v0 = env.batch.version
    for t, (k, compact) in enumerate(((k2, True), (k3, False))):
        env.batch.set_springs(k=k)
        assert _compact(env) == compact and env.batch.version > v0
        orc = Oracle(dict(spec, k=k, pos=env.pos.cpu().numpy(), vel=env.vel.cpu().numpy(), acc=env.acc.cpu().numpy(),
                          mx=env.muscle_x.cpu().numpy(), steps=env.steps.cpu().numpy()), dict(in3d=1), n_threads=8)
        got = _outs(*env.step(acts[t]))
        _against_oracle(got, _state(env), orc.step(acts[t]), orc, t)


def _run_vs_steps(monkeypatch, n, lanes, compact, extras=False):
    """run() of 3 steps (one C call, the acc / contact stores of steps 0 and 1 skipped) against three step() calls."""
    import torch
    from oracle.oracle import Oracle
    from walker_gym_amd.batched_env import BatchedPhysicsEnv
    spec, params = _canonical(n), dict(in3d=1)
    acts = np.random.default_rng(3).uniform(-1, 1, (3, n, 8)).astype(np.float32)
    ref_env, orc = BatchedPhysicsEnv(spec, **params), Oracle(spec, params, n_threads=8)
    per_step = []
    for t in range(3):
        per_step.append(_outs(*ref_env.step(acts[t])))
        oref = orc.step(acts[t])
    ref_state = _state(ref_env)
    _against_oracle(per_step[-1], ref_state, oref, orc, 2)
    dacts = torch.as_tensor(acts, device="cuda")
    for record in (False, True):
        for edge8 in ("1", "0"):
            env = BatchedPhysicsEnv(spec, **params)
            if extras:
                env.enable_info_extras()
            assert _compact(env) == compact
            assert env._lanes(lanes) == (lanes if n >= 64 * lanes else 1)
            rec = None
            if record:
                rec = {"reward": torch.empty((3, n), device="cuda"),
                       "done": torch.empty((3, n), dtype=torch.uint8, device="cuda"),
                       "energy": torch.empty((3, n), device="cuda"), "centroid": torch.empty((3, n, 3), device="cuda")}
            monkeypatch.setenv("WG_EDGE8", edge8)
            env.run(dacts, 3, lanes=lanes, record=rec)
            st = _state(env)
            monkeypatch.delenv("WG_EDGE8")
            what = f"record={record} WG_EDGE8={edge8}"
            for k in STATE:
                _bits(st[k], ref_state[k], f"{k} after run() ({what})")
            _bits(env.obs.cpu().numpy(), per_step[2]["obs"], f"obs ({what})")
            if record:
                for t in range(3):
                    for k in ("reward", "done", "energy", "centroid"):
                        _bits(rec[k][t].cpu().numpy(), per_step[t][k], f"step {t} {k} ({what})")
            else:
                for k, t_ in (("reward", env.reward), ("done", env.done), ("centroid", env.centroid), ("energy", env.energy)):
                    _bits(t_.cpu().numpy().astype(per_step[2][k].dtype), per_step[2][k], f"{k} ({what})")
                if extras:
                    from oracle.oracle import nonfinite
                    nf = nonfinite(orc.pos, orc.vel, orc.acc, orc.mass_off)
                    _bits(env.info()["nonfinite"].cpu().numpy().astype(np.uint8), nf.astype(np.uint8), "nonfinite")


# N = 8: the issue's shape (too small to split: run(lanes=2) steps it as one range); 192: two walker ranges (128 + 64,
# halved tiles); 4160: two ranges of 528 and 512 full tiles, both on the compact records
@pytest.mark.parametrize("n,compact", [(8, False), (192, False), (4160, True)])
def test_run_two_ranges(monkeypatch, n, compact):
    _run_vs_steps(monkeypatch, n, 2, compact)


@pytest.mark.parametrize("n,compact", [(8, False), (4160, True)])
def test_run_two_ranges_nonfinite(monkeypatch, n, compact):
    _run_vs_steps(monkeypatch, n, 2, compact, extras=True)


@pytest.mark.parametrize("n,compact", [(8, False), (N_CANON, True)])
def test_resident_rollout(monkeypatch, n, compact):
    _resident_case(monkeypatch, _canonical(n), dict(in3d=1), compact)


def _resident_case(monkeypatch, spec, params, compact):
    import torch
    from oracle.oracle import Oracle
    from walker_gym_amd.batched_env import BatchedPhysicsEnv
    n = len(spec["mass_off"]) - 1
    acts = np.random.default_rng(4).uniform(-1, 1, (3, n, int(np.max(spec["n_muscles"])))).astype(np.float32)
    orc = Oracle(spec, params, n_threads=8)
    refs = [orc.step(acts[t]) for t in range(3)]
    outs = {}
    for edge8 in ("1", "0"):
        env = BatchedPhysicsEnv(spec, **params)
        assert _compact(env) == compact and env.resident_ok()
        monkeypatch.setenv("WG_EDGE8", edge8)
        obs, rew, done = env.rollout(torch.as_tensor(acts, device="cuda"), resident=True)
        st = _state(env)
        monkeypatch.delenv("WG_EDGE8")
        for t in range(3):
            _bits(obs[t].cpu().numpy(), refs[t]["obs"], f"step {t} obs (WG_EDGE8={edge8})")
            _bits(rew[t].cpu().numpy(), refs[t]["reward"], f"step {t} reward (WG_EDGE8={edge8})")
            _bits(done[t].cpu().numpy(), refs[t]["done"], f"step {t} done (WG_EDGE8={edge8})")
        for k, o in (("pos", orc.pos), ("vel", orc.vel), ("acc", orc.acc), ("muscle_x", orc.mx), ("steps", orc.steps),
                     ("contact", orc.contact)):
            _bits(st[k], o, f"{k} after rollout (WG_EDGE8={edge8})")
        outs[edge8] = st
    for k in STATE:
        _bits(outs["1"][k], outs["0"][k], f"{k}: compact vs 16-byte records")


# ---- every (IN3D, NE, E8, FIX) instance of the step and resident kernels without auto-reset.  The compact records and
# the fixed-parameter instance need 512 full standard tiles: 8,192 walkers of M = 4, K = 4 (16 per wave, 64 springs: one
# pass) and 512 walkers of M = 64 (one per wave, so K alone sets the passes: 120, 150, 200 and 300 springs are 2, 3, 4
# and 5 passes, the last on the NE 8 instance).  Each case runs the default path (FIX up to four passes, the generic
# compact instance at NE 8) and WG_EDGE8=0 (the 16-byte records) in _step_case / _resident_case, then the generic
# compact instance under WG_FIX=0.
PASSES = [(1, dict(N=8192, M=4, K=4, A=2)), (2, dict(N=512, M=64, K=120, A=8)), (3, dict(N=512, M=64, K=150, A=8)),
          (4, dict(N=512, M=64, K=200, A=8)), (8, dict(N=512, M=64, K=300, A=8))]


def _passes_spec(shape):
    kw = dict(shape)
    return _canonical(kw.pop("N"), **kw)


@pytest.mark.parametrize("in3d", [0, 1])
@pytest.mark.parametrize("ne,shape", PASSES, ids=[f"ne{ne}" for ne, _ in PASSES])
def test_every_step_instance(monkeypatch, in3d, ne, shape):
    from walker_gym_amd import _lib
    lib, spec = _lib.load(), _passes_spec(shape)
    n0 = lib.wg_fix_launches()
    env = _step_case(monkeypatch, spec, dict(in3d=in3d), 2, True)
    geo = env.launch_geometry()
    wpw = geo["walkers_per_block"] // (geo["threads"] // 64)
    assert (wpw * env.batch.K + 63) // 64 == (ne if ne <= 4 else 5)
    n1 = lib.wg_fix_launches()
    assert n1 - n0 == (2 * env._step_lanes() if ne <= 4 else 0)   # the default arm's two steps: the FIX instance
    monkeypatch.setenv("WG_FIX", "0")
    _step_case(monkeypatch, spec, dict(in3d=in3d), 2, True)
    assert lib.wg_fix_launches() == n1


@pytest.mark.parametrize("in3d", [0, 1])
@pytest.mark.parametrize("ne,shape", PASSES, ids=[f"ne{ne}" for ne, _ in PASSES])
def test_every_resident_instance(monkeypatch, in3d, ne, shape):
    _resident_case(monkeypatch, _passes_spec(shape), dict(in3d=in3d), True)

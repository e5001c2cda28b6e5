"""The lean step kernel's fixed-parameter instance (FIX: full tiles, default parameters; DESIGN §5 WG_FIX) against the
generic instance it specialises (WG_FIX=0, the control arm): run() of 8 steps in one call (the acc / contact stores off
in the first seven, on in the last) on the same seeded inputs, every state tensor and every output bit for bit; the
launches that must fall back to the generic instance; and a batch with diverged walkers against the C oracle.

Which instance ran is read from launch_geometry()["fix_launches"], the library's running count of launches that took
the FIX instance.

A lean launch reads the compact spring records, which FIX needs, only with its standard tile of 64 / M walkers per
wave, and batches of fewer than 512 such tiles get halved tiles (tests/test_gpu_edge8.py).  So every shape with
M < 64 runs at its smallest size, where both arms are the generic instance, and at the smallest batch of full tiles
that reaches FIX: 512 tiles."""
import numpy as np
import pytest

from conftest import gpu_available

pytestmark = pytest.mark.gpu

STATE = ("pos", "vel", "acc", "muscle_x", "steps", "contact")
OUT = ("obs", "reward", "done", "centroid", "energy")
T = 8


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.skip("no ROCm GPU")


def _bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    if a.dtype == np.float32:
        a, b = a.view(np.uint32), b.view(np.uint32)
    bad = a != b
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ"


def _fix_launches(env) -> int:
    return env.launch_geometry()["fix_launches"]


def _snapshot(env):
    import torch
    torch.cuda.synchronize()
    d = {k: getattr(env, k).cpu().numpy().copy() for k in STATE + OUT if getattr(env, k, None) is not None}
    d["done"] = d["done"].astype(np.uint8)
    return d


def _canonical(n, **kw):
    from walker_gym_amd.synthetic import canonical_walkers
    return canonical_walkers(n, seed=5, **kw)


def _balance(n):
    from walker_gym_amd.walker import balance_spec
    return balance_spec(n)


def _both_arms(monkeypatch, spec, params, fix, lanes=1, setup=None, seed=17):
    """run() of T steps under the default knobs and under WG_FIX=0: equal bits; `fix`: the default arm took the FIX
    instance for every launch (else for none); the control arm never does."""
    import torch
    from walker_gym_amd.batched_env import BatchedPhysicsEnv
    env, env0 = BatchedPhysicsEnv(spec, **params), BatchedPhysicsEnv(spec, **params)
    for e in (env, env0):
        if setup is not None:
            setup(e)
    A = env.batch.A
    acts = torch.as_tensor(np.random.default_rng(seed).uniform(-1, 1, (T, env.N, A)).astype(np.float32), device="cuda")
    if int(env.params.action_mode) == 1:
        acts = (acts > 0).to(torch.float32).contiguous()
    n0 = _fix_launches(env)
    env.run(acts, T, lanes=lanes)
    got = _snapshot(env)
    n1 = _fix_launches(env)
    monkeypatch.setenv("WG_FIX", "0")
    env0.run(acts, T, lanes=lanes)
    ref = _snapshot(env0)
    monkeypatch.delenv("WG_FIX")
    n2 = _fix_launches(env)
    assert n2 == n1, "WG_FIX=0 launched the FIX instance"
    assert n1 - n0 == (T * env._lanes(lanes) if fix else 0), f"{n1 - n0} FIX launches"
    assert got.keys() == ref.keys() and set(STATE + OUT) <= set(got)
    for k in got:
        _bits(got[k], ref[k], k)
    assert (got["steps"] == T).all() or int(env.params.max_steps) < T or env._ar_mode
    return env


# ---------------------------------------------------------------- bit-identity with the control arm
@pytest.mark.parametrize("n,fix", [(4, False), (8, False), (2048, True), (2052, True)])
def test_canonical(monkeypatch, n, fix):
    """M = 16, K = 40, A = 8 (three spring passes, the last of 32 lanes)."""
    _both_arms(monkeypatch, _canonical(n), dict(in3d=1), fix)


def test_canonical_2d(monkeypatch):
    _both_arms(monkeypatch, _canonical(2048), dict(in3d=0), True)


def test_canonical_two_ranges(monkeypatch):
    """Two walker ranges, as the flagship steps (528 and 512 full tiles), each launch on FIX."""
    env = _both_arms(monkeypatch, _canonical(4160), dict(in3d=1), True, lanes=2)
    assert env._lanes(2) == 2


@pytest.mark.parametrize("n,fix", [(16, False), (8192, True)])
def test_balance(monkeypatch, n, fix):
    """Balance-v0, M = 4, K = 5, 2D: 16 walkers per wave, 80 springs, two passes (NE = 2)."""
    env = _both_arms(monkeypatch, _balance(n), dict(in3d=0), fix)
    assert env.batch.M == 4


@pytest.mark.parametrize("n,fix", [(2, True), (1030, True)])
def test_m64(monkeypatch, n, fix):
    """One walker per wave: M = 64, K = 120 (NE = 2), A = 8.  A one-walker tile is never halved, so two walkers reach
    FIX already (one wave per workgroup); 1,030 walkers: four waves per workgroup, the last workgroup of two."""
    _both_arms(monkeypatch, _canonical(n, M=64, K=120, A=8), dict(in3d=1), fix)


@pytest.mark.parametrize("n,fix", [(16, False), (8192, True)])
def test_one_pass(monkeypatch, n, fix):
    """NE = 1, the preloaded entry (walker_step_lean1): M = 4, K = 4 is 64 springs per full tile of 16 walkers."""
    env = _both_arms(monkeypatch, _canonical(n, M=4, K=4, A=2), dict(in3d=1), fix)
    assert 16 * env.batch.K == 64


def test_four_passes(monkeypatch):
    """NE = 4 with a full last pass: M = 16, K = 64 is 256 springs per tile."""
    _both_arms(monkeypatch, _canonical(2048, K=64), dict(in3d=1), True)


# ---------------------------------------------------------------- fallback: the generic instance runs
N_FIX = 2048   # a batch that takes FIX under the default parameters (test_canonical)


def test_fallback_partial_tile(monkeypatch):
    _both_arms(monkeypatch, _canonical(5), dict(in3d=1), False)
    _both_arms(monkeypatch, _canonical(N_FIX + 2), dict(in3d=1), False)   # 512 full tiles and one of two walkers


@pytest.mark.parametrize("params", [dict(midform=0), dict(midform=2), dict(pk=2.0), dict(mk=0.5), dict(conmid=True),
                                    dict(action_mode=1), dict(pair_mode=1), dict(integrator=2)],
                         ids=lambda p: "-".join(f"{k}={v}" for k, v in p.items()))
def test_fallback_params(monkeypatch, params):
    _both_arms(monkeypatch, _canonical(N_FIX), dict(in3d=1, **params), False)


def test_fallback_pinned(monkeypatch):
    spec = _canonical(N_FIX)
    spec["pinned"] = np.zeros(len(spec["m"]), np.uint8)
    spec["pinned"][37] = 1
    env = _both_arms(monkeypatch, spec, dict(in3d=1), False)
    assert env.batch.pinned is not None


def test_fallback_auto_reset(monkeypatch):
    env = _both_arms(monkeypatch, _canonical(N_FIX), dict(in3d=1, max_steps=3), False,
                     setup=lambda e: e.enable_auto_reset())
    assert env._ar_mode


def test_fallback_no_actions_columns(monkeypatch):
    """Fewer action columns than muscles: the muscles past them do not act (the generic instance's test)."""
    import torch
    from walker_gym_amd.batched_env import BatchedPhysicsEnv
    env = BatchedPhysicsEnv(_canonical(N_FIX), in3d=1)
    acts = torch.rand((1, env.N, 4), device="cuda") * 2 - 1
    n0 = _fix_launches(env)
    env.run(acts.contiguous(), 2)
    torch.cuda.synchronize()
    assert _fix_launches(env) == n0


# ---------------------------------------------------------------- the C oracle, diverged walkers included
def test_oracle_diverged(monkeypatch):
    """A full-tile batch with diverged walkers (every mass NaN somewhere), partly NaN walkers and walkers at +inf,
    stepped through FIX (no pins: a pinned mass takes the generic instance), against the C oracle as
    tests/test_gpu_diverged.py compares (NaN == NaN whatever the payload)."""
    from test_gpu_diverged import _compare, _diverge
    from walker_gym_amd.synthetic import canonical_walkers
    spec = _diverge(canonical_walkers(N_FIX, seed=21), np.random.default_rng(1), pin=False)
    from walker_gym_amd.batched_env import BatchedPhysicsEnv
    probe = BatchedPhysicsEnv(_canonical(4), in3d=1)
    n0 = _fix_launches(probe)
    env = _compare(spec, dict(in3d=1), 4, 5)
    assert _fix_launches(probe) - n0 == 4 * env._step_lanes()

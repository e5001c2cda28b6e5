"""BatchedPhysicsEnv.rollout_policy (wg_rollout_policy: the whole closed-loop episode in one resident launch, the
MLPPolicy evaluated inside the wave) against the same policy driven by step() in a loop on the device and by the
reference engine on the CPU.  Every comparison is bitwise; the cases (tests/policy_cases.py) are checked finite on
the CPU by tests/test_policy_cpu.py."""
import functools

import numpy as np
import pytest

import policy_cases as pc
from conftest import gpu_available

pytestmark = pytest.mark.gpu

CASES = pytest.mark.parametrize("case", pc.CASES, ids=lambda c: c.name)
STATE = ("pos", "vel", "acc", "muscle_x", "steps", "contact")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.skip("no ROCm GPU")


def _bits(t):
    a = t.detach().cpu().contiguous().numpy() if hasattr(t, "detach") else np.ascontiguousarray(t)
    return a.view(np.uint8)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _env(case):
    from walker_gym_amd.batched_env import BatchedPhysicsEnv
    return BatchedPhysicsEnv(pc.spec_of(case.kind), device="cuda:0", **case.params)


def _state(env):
    return {k: getattr(env, k).detach().cpu().numpy().copy() for k in STATE}


def _buffers(env, T, C):
    import torch
    dv, N = env.device, env.N
    # (NaN / 0xff fills: a value the kernel failed to write cannot pass for one it wrote)
    return dict(obs_out=torch.full((T, N, env.obs_dim), float("nan"), device=dv),
                reward_out=torch.full((T, N), float("nan"), device=dv),
                done_out=torch.full((T, N), 255, dtype=torch.uint8, device=dv),
                action_out=torch.full((T, N, C), float("nan"), device=dv))


@functools.lru_cache(maxsize=None)
def _runs(name):
    """One fused rollout with every per-step buffer, one with none, and the device step loop, of one case: host copies,
    computed once and shared by the tests below (never modified)."""
    import torch
    case = next(c for c in pc.CASES if c.name == name)
    pol = pc.policy_of(case, "cuda:0")
    T = case.T
    env = _env(case)
    geo = env.launch_geometry()   # the wave tile the case is there for
    assert geo["walkers_per_block"] * 64 // geo["threads"] == case.wpw, geo
    buf = _buffers(env, T, case.C)
    res = env.rollout_policy(pol, T, **buf)
    torch.cuda.synchronize()
    fused = dict({k[:-4]: v.cpu().numpy() for k, v in buf.items()}, **_state(env),
                 returns=res["returns"].cpu().numpy(), lengths=res["lengths"].cpu().numpy())
    env2 = _env(case)
    res2 = env2.rollout_policy(pol, T)
    torch.cuda.synchronize()
    bare = dict(_state(env2), returns=res2["returns"].cpu().numpy(), lengths=res2["lengths"].cpu().numpy())
    ref = _env(case)
    ref.observe()
    loop = dict(obs=[], reward=[], done=[], action=[])
    for t in range(T):
        a = pol.for_rows(0, ref.N)(ref.obs, t)
        obs, rew, done, _ = ref.step(a)
        loop["obs"].append(obs.cpu().numpy().copy()); loop["reward"].append(rew.cpu().numpy().copy())
        loop["done"].append(done.cpu().numpy().astype(np.uint8)); loop["action"].append(a.cpu().numpy().copy())
    loop = dict({k: np.stack(v) for k, v in loop.items()}, **_state(ref))
    return fused, bare, loop


@CASES
def test_fused_equals_device_step_loop(case):
    fused, _, loop = _runs(case.name)
    for k in ("action", "obs", "reward", "done") + STATE:
        assert fused[k].shape == loop[k].shape and _same(fused[k], loop[k]), k
    if np.isfinite(case.L):   # the clip engages on some outputs, not on all
        hit = np.abs(fused["action"]) == np.float32(case.L)
        assert hit.any() and not hit.all()


@pytest.mark.parametrize("case", [c for c in pc.CASES if c.oracle], ids=lambda c: c.name)
def test_fused_equals_reference_engine(case):
    from conftest import record_metric
    fused, _, _ = _runs(case.name)
    ref = pc.oracle_rollout(case.name)
    same = tot = 0
    for k in ("action", "obs", "reward", "done") + STATE:
        a, b = np.ascontiguousarray(fused[k]), np.ascontiguousarray(ref[k]).reshape(fused[k].shape)
        assert a.dtype == b.dtype or k in ("contact", "done"), k
        eq = a.view(np.uint8) == b.astype(a.dtype).view(np.uint8)
        same += int(eq.sum()); tot += eq.size
    record_metric(f"policy_rollout_bit_exact_fraction[{case.name}]", same / tot)
    assert same == tot, f"{tot - same} of {tot} bytes differ from the reference engine"


@pytest.mark.parametrize("edge8", [True, False], ids=["compact", "16-byte"])
@pytest.mark.parametrize("case", pc.COVER, ids=lambda c: c.name)
def test_every_instance_equals_reference_engine(case, edge8, monkeypatch):
    """walker_rollout_policy at every (IN3D, NE, E8): the fused rollout's every step and final state, bit for bit."""
    import torch
    if not edge8:
        monkeypatch.setenv("WG_EDGE8", "0")
    env = _env(case)
    geo = env.launch_geometry()
    assert geo["walkers_per_block"] * 64 // geo["threads"] == case.wpw, geo
    buf = _buffers(env, case.T, case.C)
    env.rollout_policy(pc.policy_of(case, "cuda:0"), case.T, **buf)
    torch.cuda.synchronize()
    fused = dict({k[:-4]: v.cpu().numpy() for k, v in buf.items()}, **_state(env))
    ref = pc.oracle_rollout(case.name)
    for k in ("action", "obs", "reward", "done") + STATE:
        a, b = np.ascontiguousarray(fused[k]), np.ascontiguousarray(ref[k]).reshape(fused[k].shape)
        assert a.dtype == b.dtype or k in ("contact", "done"), k
        assert np.array_equal(a.view(np.uint8), b.astype(a.dtype).view(np.uint8)), k


@CASES
def test_no_per_step_buffers(case):
    fused, bare, _ = _runs(case.name)
    for k in STATE + ("returns", "lengths"):
        assert _same(fused[k], bare[k]), k


@CASES
def test_returns_and_lengths(case):
    fused, _, _ = _runs(case.name)
    ret, length = pc.returns_lengths(fused["reward"], fused["done"])
    assert fused["returns"].dtype == np.float32 and fused["lengths"].dtype == np.int32
    assert _same(fused["returns"], ret) and np.array_equal(fused["lengths"], length)
    if case.done:   # every walker's done fired before T, at differing steps
        assert (fused["lengths"] < case.T).all() and len(np.unique(fused["lengths"])) >= 2
    else:
        assert (fused["lengths"] == case.T).all()


@CASES
def test_the_loop_is_closed(case):
    fused, _, _ = _runs(case.name)
    assert not np.array_equal(fused["action"][1], fused["action"][case.T - 1])


@CASES
def test_split_rollouts(case):
    """n_steps = 1 equals one step(policy(observe())); two calls of T / 2 steps equal one call of T (the second call
    starts from the stored state: its entry observation, the loaded acc included)."""
    import torch
    fused, _, _ = _runs(case.name)
    pol = pc.policy_of(case, "cuda:0")
    T, h = case.T, case.T // 2
    one = _env(case)
    b1 = _buffers(one, 1, case.C)
    one.rollout_policy(pol, 1, **b1)
    ref = _env(case)
    a = pol.for_rows(0, ref.N)(ref.observe()[0], 0)
    obs, rew, done, _ = ref.step(a)
    torch.cuda.synchronize()
    assert _same(b1["action_out"][0], a) and _same(b1["obs_out"][0], obs) and _same(b1["reward_out"][0], rew)
    assert _same(b1["done_out"][0], done.to(torch.uint8))
    for k in STATE:
        assert _same(getattr(one, k), getattr(ref, k)), k
    two = _env(case)
    ba, bb = _buffers(two, h, case.C), _buffers(two, T - h, case.C)
    two.rollout_policy(pol, h, **ba)
    two.rollout_policy(pol, T - h, **bb)
    torch.cuda.synchronize()
    for k in ("action", "obs", "reward", "done"):
        both = torch.cat([ba[k + "_out"], bb[k + "_out"]]).cpu().numpy()
        assert _same(both, fused[k]), k
    for k in STATE:
        assert _same(getattr(two, k), fused[k]), k


def test_refusals_leave_the_env_usable():
    import torch
    from walker_gym_amd.batched_env import BatchedPhysicsEnv
    from walker_gym_amd.policy import MLPPolicy
    from walker_gym_amd.synthetic import canonical_walkers, ragged_walkers
    z = lambda *s: torch.zeros(s, device="cuda:0")
    rg = BatchedPhysicsEnv(ragged_walkers(200, seed=2), device="cuda:0", in3d=1)
    with pytest.raises(ValueError, match="policy_loop"):
        rg.rollout_policy(MLPPolicy(z(rg.obs_dim, 2)), 2)
    env = BatchedPhysicsEnv(canonical_walkers(256, seed=2), device="cuda:0", in3d=1)
    good = MLPPolicy(z(152, 8))
    with pytest.raises(ValueError):
        env.rollout_policy(MLPPolicy(z(151, 8)), 2)                 # D
    with pytest.raises(ValueError):
        env.rollout_policy(MLPPolicy(z(152, 9)), 2)                 # C > A
    with pytest.raises(ValueError):
        env.rollout_policy(MLPPolicy(z(3, 152, 8)), 2)              # N % G
    with pytest.raises(ValueError):
        env.rollout_policy(good, 0)                                 # n_steps
    with pytest.raises(ValueError):
        env.rollout_policy(MLPPolicy(torch.zeros(152, 8)), 2)       # host weights
    with pytest.raises(ValueError):
        env.rollout_policy(good, 2, reward_out=z(3, 256))           # buffer shape
    with pytest.raises(ValueError):
        env.rollout_policy(lambda rows, t: rows[:, :8], 2)          # not an MLPPolicy
    env.enable_auto_reset()
    with pytest.raises(ValueError, match="auto-reset"):
        env.rollout_policy(good, 2)
    env.disable_auto_reset()
    ref = BatchedPhysicsEnv(canonical_walkers(256, seed=2), device="cuda:0", in3d=1)
    r = env.rollout_policy(good, 3)
    for t in range(3):
        ref.step(z(256, 8))
    torch.cuda.synchronize()
    assert (r["lengths"] == 3).all()
    for k in STATE:
        assert _same(getattr(env, k), getattr(ref, k)), k
    assert "total_energy" not in env.info()                         # stale, as after rollout()
    obs = env.step(z(256, 8))[0]
    assert _same(obs, ref.step(z(256, 8))[0]) and "total_energy" in env.info()


def test_no_collateral_change():
    """rollout(resident=True) and policy_loop still give the bits of step() loops."""
    import torch
    from walker_gym_amd.batched_env import BatchedPhysicsEnv
    case = pc.CASES[1]
    pol = pc.policy_of(case, "cuda:0")
    T, N = case.T, 1000
    acts = (torch.rand((T, N, 8), generator=torch.Generator().manual_seed(5)) * 2 - 1).cuda()
    ref, env = _env(case), _env(case)
    obs, rew, done = env.rollout(acts, resident=True)
    for t in range(T):
        o, r, d, _ = ref.step(acts[t])
        assert _same(obs[t], o) and _same(rew[t], r) and _same(done[t], d.to(torch.uint8)), t
    for k in STATE:
        assert _same(getattr(env, k), getattr(ref, k)), k
    ref, env = _env(case), _env(case)
    ref.observe(); env.observe()
    for t in range(T):
        ref.step(pol.for_rows(0, N)(ref.obs, t))
    env.policy_loop(pol, T, lanes=1)
    torch.cuda.synchronize()
    for k in STATE + ("obs", "reward", "done"):
        assert _same(getattr(env, k), getattr(ref, k)), k


@pytest.mark.parametrize("name,lanes,graph", [("canonical-mlp-4sets-c5-inf", 2, False), ("canonical-mlp-4sets-c5-inf", 3, True),
                                              ("canonical-mlp-perwalker", 2, True), ("canonical-lin-4sets-c5", 2, False)])
def test_policy_loop_binds_the_parameter_sets_per_range(name, lanes, graph):
    """policy_loop hands each walker range its own slice of rows: an MLPPolicy with several parameter sets is bound to
    the range's first walker (for_rows), so walker w uses set w // (N // G) in every range.  Against the step() loop
    (computed once per case by _runs), and so against the fused rollout too."""
    import torch
    case = next(c for c in pc.CASES if c.name == name)
    _, _, loop = _runs(name)
    pol = pc.policy_of(case, "cuda:0")
    env = _env(case)
    first = (env.N // lanes + 63) // 64 * 64   # the second range's first walker
    assert case.G == env.N or first % (env.N // case.G) != 0   # a range boundary is no set boundary
    env.observe()
    env.policy_loop(pol, case.T, lanes=lanes, graph=graph)
    torch.cuda.synchronize()
    for k in STATE:
        assert _same(getattr(env, k), loop[k]), k
    assert _same(env.obs, loop["obs"][-1]) and _same(env.reward, loop["reward"][-1])
    with pytest.raises(ValueError, match="for_rows"):   # unbound, the policy does not guess
        pol(env.obs, 0)


def test_policy_loop_binds_scattered_ragged_ranges(monkeypatch):
    """A ragged batch stored in one global packing: both ranges are scattered sets of caller rows, and the policy is
    bound to each range's row index (for_row_index); caller row r uses set r // (N // G)."""
    import torch
    from walker_gym_amd.batched_env import BatchedPhysicsEnv
    from walker_gym_amd.policy import MLPPolicy
    from walker_gym_amd.synthetic import ragged_walkers
    monkeypatch.setenv("WG_TILE_WINDOW", "0")
    N, T, G = 3000, 6, 3
    spec = ragged_walkers(N, seed=41, mmin=4, mmax=32)
    ref = BatchedPhysicsEnv(spec, device="cuda:0", in3d=1)
    g = torch.Generator().manual_seed(9)
    pol = MLPPolicy((torch.randn((G, ref.obs_dim, 4), generator=g) * 0.002).cuda(), act_limit=1.0)
    ref.observe()
    seen = []
    for t in range(T):
        a = pol.for_rows(0, N)(ref.obs, t)
        seen.append(a.clone())
        ref.step(a)
    env = BatchedPhysicsEnv(spec, device="cuda:0", in3d=1)
    assert env._caller_bounds(2)[1] == [False, False]
    env.observe()
    env.policy_loop(pol, T, lanes=2)
    torch.cuda.synchronize()
    for k in ("pos", "vel", "acc", "muscle_x", "obs", "reward", "done"):
        assert _same(getattr(env, k), getattr(ref, k)), k
    # the sets matter: the three thirds of the batch act differently on the same kind of rows
    assert not torch.equal(seen[1][:5], seen[1][N // G:N // G + 5])

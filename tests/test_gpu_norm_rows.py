"""wg_obs_moments against obs_moments_numpy / obs_norm_finish_numpy, wg_policy_forward_normalized /
wg_policy_backward_normalized against pg.policy_rows_numpy / pg.policy_grad_numpy of a policy that carries a normaliser,
bit for bit (NaN == NaN as in test_gpu_policy_rows.py), autograd through pg.policy_rows, the loop they close on a
pg.collect batch, and the ES trainer with an ObsNorm against its composition."""
import math

import numpy as np
import pytest

import es_cases as ec
import rows_cases as rc
from conftest import gpu_available

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32, f64 = np.float32, np.float64
BOUND = 5000.0


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.skip("no ROCm GPU")


def _host(a):
    return np.ascontiguousarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a)


def _same(a, b):
    """Bit-identical, with NaN == NaN (the sign and payload of a produced NaN are no part of the contract)."""
    if a is None or b is None:
        return a is None and b is None
    a, b = _host(a), _host(b)
    na, nb = np.isnan(a), np.isnan(b)
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(na, nb) and \
        np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def _bits_equal(a, b):
    a, b = _host(a), _host(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.array(a, copy=True)).to(DEV)


# ------------------------------------------------------------------ wg_obs_moments
def _moment_rows(T, N, D, chunk, seed):
    """[T, N, D] at mixed magnitudes (ones, tens, thousands: the sums round) with a NaN row, an inf row, a row with a
    value exactly at the bound (all three left out, the mask on), a random mask, and chunk 1 fully masked."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((T * N, D)) * rng.choice([1.0, 30.0, 2000.0], (1, D))).astype(f32)
    x = np.clip(x, -0.9 * BOUND, 0.9 * BOUND).astype(f32)
    mask = (rng.random(T * N) > 0.2).astype(np.uint8)
    R = T * N
    if R > 8:
        x[2, D // 2], x[4, 0], x[5, D - 1], x[6, D - 1] = np.nan, -np.inf, f32(BOUND), np.nextafter(f32(BOUND), f32(0))
        mask[[2, 4, 5, 6]] = 1
    if R > 2 * chunk:
        mask[chunk:2 * chunk] = 0
        x[chunk:2 * chunk] = np.nan        # (masked rows may hold anything)
    else:
        mask[:] = 1
    return x.reshape(T, N, D), mask.reshape(T, N)


def _moments(x3, m3, D, chunk, state, mean=None, scale=None, bound=BOUND, eps=1e-8):
    """wg_obs_moments called directly on device tensors (x3 [T, N, D], m3 [T, N] or None; either may be strided in its
    step dimension): state, mean and scale are updated in place."""
    import torch
    from walker_gym_amd import _lib, pg
    rows, T, N, o3, mm, _ = pg._rows_of(D, x3.device, x3, m3, "test")
    L = _lib.load()
    count = L.wg_obs_moments_workspace(rows, D, chunk)
    _lib.check(count, "wg_obs_moments_workspace")
    assert count == -(-T * N // chunk) * (1 + 2 * D)
    ws = torch.full((int(count) + 8,), float("nan"), dtype=torch.float64, device=DEV)
    p = _lib.ptr
    _lib.check(L.wg_obs_moments(rows, D, bound, chunk, p(ws), p(state), eps, p(mean), p(scale),
                                torch.cuda.current_stream().cuda_stream), "wg_obs_moments")
    torch.cuda.synchronize()
    assert bool(torch.isnan(ws[int(count):]).all()) and not bool(torch.isnan(ws[:int(count)]).any())
    return ws


@pytest.mark.parametrize("chunk", [1, 7, 256])
@pytest.mark.parametrize("D", [1, 3, 26, 155, 300])
@pytest.mark.parametrize("T,N", [(1, 1), (2, 63), (9, 65), (3, 1000)])
def test_obs_moments_equal_numpy(T, N, D, chunk):
    import torch
    from walker_gym_amd.normalize import obs_moments_numpy, obs_norm_finish_numpy
    x, mask = _moment_rows(T, N, D, chunk, 100 * T + D + chunk)
    W = 1 + 2 * D
    # strided x and mask, sentinels in the gaps (NaN / 1: a kernel that read a gap would show it)
    xbuf = torch.full((T, N * D + 5), float("nan"), device=DEV)
    xbuf[:, :N * D] = _dev(x.reshape(T, N * D))
    xs = torch.as_strided(xbuf, (T, N, D), (N * D + 5, D, 1))
    mbuf = torch.ones((T, N + 7), dtype=torch.uint8, device=DEV)
    mbuf[:, :N] = _dev(mask)
    ms = torch.as_strided(mbuf, (T, N), (N + 7, 1))
    state = torch.zeros(W, dtype=torch.float64, device=DEV)
    mean, scale = torch.full((D,), -7.0, device=DEV), torch.full((D,), -7.0, device=DEV)
    _moments(xs, ms, D, chunk, state, mean, scale)
    want = obs_moments_numpy(x, mask, BOUND, chunk)
    assert _bits_equal(state, want)
    fin = obs_norm_finish_numpy(want, 1e-8)
    if fin is None:                                    # no used row: the outputs keep what they held
        assert want[0] == 0 and bool((mean == -7.0).all()) and bool((scale == -7.0).all())
    else:
        assert _bits_equal(mean, fin[0]) and _bits_equal(scale, fin[1])
    if T * N > 8:
        assert 0 < want[0] <= T * N - 3 and np.isfinite(want).all()
    # a second call continues the state (contiguous rows, no mask), outputs NULL: the state alone
    first = state.clone()
    _moments(_dev(x), None, D, chunk, state)
    assert _bits_equal(state, obs_moments_numpy(x, None, BOUND, chunk, state=want))
    # the same call twice: identical bits
    again = first.clone()
    m2, s2 = torch.zeros(D, device=DEV), torch.zeros(D, device=DEV)
    _moments(_dev(x), None, D, chunk, again, m2, s2)
    assert _bits_equal(again, state)
    fin = obs_norm_finish_numpy(_host(state), 1e-8)
    assert fin is None or (_bits_equal(m2, fin[0]) and _bits_equal(s2, fin[1]))
    # bound = inf takes the at-bound rows too
    st = torch.zeros(W, dtype=torch.float64, device=DEV)
    _moments(_dev(x), _dev(mask), D, chunk, st, bound=math.inf)
    assert _bits_equal(st, obs_moments_numpy(x, mask, math.inf, chunk))


def test_obs_moments_on_rows_wider_than_one_pass():
    """D = 1,100: a thread's four columns cover 1,024, so the chunk is walked a second time for the rest; 14 rows to a
    tile of LDS."""
    import torch
    from walker_gym_amd.normalize import obs_moments_numpy
    T, N, D, chunk = 2, 63, 1100, 50
    x, mask = _moment_rows(T, N, D, chunk, 5)
    state = torch.zeros(1 + 2 * D, dtype=torch.float64, device=DEV)
    _moments(_dev(x), _dev(mask), D, chunk, state)
    assert _bits_equal(state, obs_moments_numpy(x, mask, BOUND, chunk))


def test_obsnorm_update_is_the_call_and_is_seen_by_the_policy_that_holds_it():
    import torch
    from walker_gym_amd import pg
    from walker_gym_amd.normalize import ObsNorm, obs_moments_numpy, obs_norm_finish_numpy
    from walker_gym_amd.policy import MLPPolicy
    T, N, D = 9, 65, 26
    x, mask = _moment_rows(T, N, D, 7, 11)
    nm = ObsNorm(D, DEV, clip=1.5, bound=BOUND)
    rng = np.random.default_rng(1)
    pol = MLPPolicy(_dev((rng.standard_normal((D, 3)) * 0.3).astype(f32)), obs_norm=nm)
    mean_ptr, scale_ptr = nm.mean.data_ptr(), nm.scale.data_ptr()
    rows = _dev(np.nan_to_num(x, nan=0.0, posinf=0.0, neginf=0.0))
    before = pg.policy_rows_forward(pol, rows).clone()
    assert nm.update(_dev(x), _dev(mask)) is nm                         # default chunk_rows: 256
    want = obs_moments_numpy(x, mask, BOUND, pg.default_chunk_rows(T, N))
    assert _bits_equal(nm.state, want) and nm.count == want[0]
    fin = obs_norm_finish_numpy(want, 1e-8)
    assert _bits_equal(nm.mean, fin[0]) and _bits_equal(nm.scale, fin[1])
    assert (nm.mean.data_ptr(), nm.scale.data_ptr()) == (mean_ptr, scale_ptr)
    after = pg.policy_rows_forward(pol, rows)                            # the same policy object, no re-wrap
    assert not _same(before, after) and _same(after, pg.policy_rows_numpy(pol.to("cpu"), _host(rows)))
    # [R, D] rows with a bool mask, an explicit chunk_rows, a second update
    nm.update(_dev(x.reshape(T * N, D)), _dev(mask.reshape(-1).astype(bool)), chunk_rows=7)
    assert _bits_equal(nm.state, obs_moments_numpy(x, mask, BOUND, 7, state=want))
    # state_dict round trip on the device; refusals
    other = ObsNorm(D, DEV)
    other.load_state_dict(nm.state_dict())
    assert _bits_equal(other.state, nm.state) and _bits_equal(other.scale, nm.scale) and other.bound == nm.bound
    for bad in (_dev(x).double(), _dev(x)[:, :, :25], _dev(x).transpose(0, 1), x):
        with pytest.raises(ValueError):
            nm.update(bad)
    with pytest.raises(ValueError):
        nm.update(_dev(x), chunk_rows=0)


# ------------------------------------------------------------------ the row kernels on xn
def _policy(seed, G, D, H, Cc, with_b1, with_b2, device=DEV):
    """test_gpu_policy_rows' policy (unit normal weights) behind a random normaliser: means at the rows' own scale,
    scales that clip about a tenth of the inputs at 1.5."""
    import torch
    from walker_gym_amd.normalize import ObsNorm
    from walker_gym_amd.policy import MLPPolicy
    rng = np.random.default_rng(seed)
    draw = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(f32)).to(device)
    w2 = draw(G, H or D, Cc)
    b2 = draw(G, Cc) if with_b2 else None
    w1 = draw(G, D, H) if H else None
    b1 = draw(G, H) if (H and with_b1) else None
    nm = ObsNorm(D, device, clip=1.5)
    nm.mean.copy_(draw(D) * 0.5)
    nm.scale.copy_(torch.from_numpy(rng.uniform(0.5, 1.5, D).astype(f32)).to(device))
    return MLPPolicy(w2, b2, w1, b1, act_limit=1.0, obs_norm=nm)


# one shape per register-block count of the backward (NT 1 .. 4) and per forward instance (staged / through L2)
ROW_SHAPES = [
    (((1, 1), 1, 1, 0, 1, False, False, 1), dict(NT=1, stage=True)),
    (((9, 65), 26, 5, 5, 5, True, False, 7), dict(NT=1, stage=False)),
    (((9, 65), 26, 8, 24, 1, True, True, 256), dict(NT=1, stage=True)),
    (((9, 65), 155, 8, 33, 65, True, True, 1), dict(NT=2, stage=False)),
    (((3, 1000), 155, 8, 64, 1, True, True, 256), dict(NT=3, stage=False)),
    (((2, 63), 191, 8, 64, 1, True, True, 7), dict(NT=4, stage=False)),
]


@pytest.mark.parametrize("shape,plan", ROW_SHAPES, ids=["T%dxN%d-D%d-C%d-H%d-G%d" % (s[0] + s[1:5]) for s, _ in ROW_SHAPES])
def test_forward_and_backward_normalized_equal_numpy(shape, plan):
    import torch
    from walker_gym_amd import pg
    (T, N), D, Cc, H, G, b1, b2, chunk = shape
    for k, v in plan.items():
        assert rc.plan_of(shape)[k] == v, k
    pol = _policy(sum(shape[1:8]) + T, G, D, H, Cc, b1, b2)
    rng = np.random.default_rng(N + D)
    x, dy = rng.standard_normal((T, N, D)).astype(f32), rng.standard_normal((T, N, Cc)).astype(f32)
    mask = None
    if T * N > 100:
        mask = (rng.random((T, N)) < 0.8).astype(np.uint8)
        x[mask == 0] = np.nan
        dy[mask == 0] = np.nan
        x[0, 1, 0] = np.nan                       # an unmasked NaN passes the clip and propagates
        mask[0, 1] = 1
    y = pg.policy_rows_forward(pol, _dev(x), _dev(mask))
    got = pg.policy_rows_backward(pol, _dev(x), _dev(dy), _dev(mask), chunk)
    torch.cuda.synchronize()
    cpu = pol.to("cpu")
    xn = cpu.obs_norm.normalize_numpy(x)
    share = np.mean(np.abs(xn[np.isfinite(xn)]) == 1.5)
    assert T * N == 1 or 0.02 < share < 0.5, share
    assert _same(y, pg.policy_rows_numpy(cpu, x, mask))
    want = pg.policy_grad_numpy(cpu, x, dy, mask, chunk)
    for name, a, b in zip(("w1", "b1", "w2", "b2"), got, want):
        assert _same(a, b), name
    # xn is the left factor: the plain kernels on the normalised rows give the same bits, and on the raw rows others
    plain = type(pol)(pol.w2, pol.b2, pol.w1, pol.b1, act_limit=1.0)
    assert _same(y, pg.policy_rows_forward(plain, _dev(xn), _dev(mask)))
    for a, b in zip(got, pg.policy_rows_backward(plain, _dev(xn), _dev(dy), _dev(mask), chunk)):
        assert _same(a, b)
    if T * N > 1:
        assert not _same(y, pg.policy_rows_forward(plain, _dev(x), _dev(mask)))


def test_crafted_rows_nan_negative_zero_and_exactly_at_the_clip():
    import torch
    from walker_gym_amd import pg
    pol = _policy(3, 1, 4, 0, 2, False, True)
    pol.obs_norm.mean.copy_(_dev(np.array([1.0, 2.0, 0.0, 0.0], f32)))
    pol.obs_norm.scale.copy_(_dev(np.array([-2.0, 1.0, 1.0, np.inf], f32)))
    x = np.array([[1.0, 3.5, -1.5, 0.0],            # -0.0 | exactly +clip | exactly -clip | 0 * inf = NaN
                  [1.0, 3.5, -1.5, 1.0],            # the same without the NaN: inf clips
                  [0.0, 9.0, -9.0, -1.0]], f32)     # beyond the clip on both sides
    cpu = pol.to("cpu")
    xn = cpu.obs_norm.normalize_numpy(x)
    assert np.signbit(xn[0, 0]) and xn[0, 0] == 0 and xn[0, 1] == 1.5 and xn[0, 2] == -1.5 and np.isnan(xn[0, 3])
    assert xn[1, 3] == 1.5 and xn[2].tolist() == [1.5, 1.5, -1.5, -1.5]
    y = pg.policy_rows_forward(pol, _dev(x))
    torch.cuda.synchronize()
    want = pg.policy_rows_numpy(cpu, x[None])[0]
    assert _same(y, want) and np.isnan(want[0]).all() and np.isfinite(want[1:]).all()


def test_identity_normaliser_gives_the_plain_kernels_bits():
    import torch
    from walker_gym_amd import pg
    from walker_gym_amd.normalize import ObsNorm
    (T, N), D, Cc, H, G, b1, b2, chunk = ROW_SHAPES[3][0]
    pol = _policy(7, G, D, H, Cc, b1, b2)
    plain = type(pol)(pol.w2, pol.b2, pol.w1, pol.b1, act_limit=1.0)
    ident = type(pol)(pol.w2, pol.b2, pol.w1, pol.b1, act_limit=1.0, obs_norm=ObsNorm(D, DEV, clip=math.inf))
    rng = np.random.default_rng(8)
    x, dy = (rng.standard_normal((T, N, D)) * 50).astype(f32), rng.standard_normal((T, N, Cc)).astype(f32)
    x[0, 0, :4] = [0.0, -0.0, 1e-42, -1e38]
    assert _bits_equal(pg.policy_rows_forward(ident, _dev(x)), pg.policy_rows_forward(plain, _dev(x)))
    for a, b in zip(pg.policy_rows_backward(ident, _dev(x), _dev(dy), None, chunk),
                    pg.policy_rows_backward(plain, _dev(x), _dev(dy), None, chunk)):
        assert _bits_equal(a, b)


def test_autograd_through_policy_rows_with_a_normaliser():
    import torch
    from walker_gym_amd import pg
    from walker_gym_amd.policy import MLPPolicy
    T, N, D, Cc, H, G, chunk = 9, 65, 26, 5, 5, 5, 7
    base = _policy(83, G, D, H, Cc, True, True)
    w1, b1, w2 = (torch.nn.Parameter(t.clone()) for t in (base.w1, base.b1, base.w2))
    pol = MLPPolicy(w2, base.b2.clone(), w1, b1, act_limit=1.0, obs_norm=base.obs_norm)
    rng = np.random.default_rng(84)
    x, dy = rng.standard_normal((T, N, D)).astype(f32), rng.standard_normal((T, N, Cc)).astype(f32)
    mask = (rng.random((T, N)) < 0.6).astype(np.uint8)
    obs = _dev(x).requires_grad_(True)
    y = pg.policy_rows(pol, obs, _dev(mask), chunk_rows=chunk)
    (y * _dev(dy)).sum().backward()
    cpu = pol.to("cpu")
    assert _same(y, pg.policy_rows_numpy(cpu, x, mask))
    want = pg.policy_grad_numpy(cpu, x, dy, mask, chunk)
    assert _same(w1.grad, want[0]) and _same(b1.grad, want[1]) and _same(w2.grad, want[2])
    assert obs.grad is None and base.obs_norm.mean.grad is None and base.obs_norm.scale.grad is None
    for bad in (dict(D=D + 1, device=DEV), dict(D=D, device="cpu")):     # a normaliser that does not fit the policy
        from walker_gym_amd.normalize import ObsNorm
        pol.obs_norm = ObsNorm(bad["D"], bad["device"])
        with pytest.raises(ValueError, match="obs_norm"):
            pg.policy_rows_forward(pol, _dev(x))


def test_the_rows_close_the_loop_of_a_normalised_stochastic_rollout():
    """pg.collect on Balance-v0 x 128, T = 16, H = 5, the policy's ObsNorm updated from a previous collect: y of the
    recorded (raw) rows plus RN32(sigma * eps) is the recorded raw action on every row, bit for bit."""
    import torch
    from walker_gym_amd import pg
    from walker_gym_amd.batched_env import BatchedPhysicsEnv
    from walker_gym_amd.normalize import ObsNorm
    from walker_gym_amd.policy import MLPPolicy
    from walker_gym_amd.walker import balance_spec
    N, T, max_steps, H = 128, 16, 6, 5
    spec = dict(balance_spec(N))
    rng = np.random.default_rng(9)
    vel = np.array(spec["vel"], f32).reshape(-1, 3).copy()
    vel[:, :2] += rng.uniform(-3, 3, (vel.shape[0], 2)).astype(f32)
    spec.update(vel=vel, steps=(np.arange(N) % max_steps).astype(np.int32))
    env = BatchedPhysicsEnv(spec, device=DEV, in3d=0, max_steps=max_steps)
    env.enable_auto_reset(final_obs=True)
    D, A = env.obs_dim, env.batch.A
    g = torch.Generator().manual_seed(3)
    mk = lambda *s: torch.nn.Parameter((torch.randn(*s, generator=g) * 0.3).to(DEV))
    nm = ObsNorm(D, DEV, clip=1.5)
    pol = MLPPolicy(mk(1, H, A), mk(1, A), mk(1, D, H), mk(1, H), obs_norm=nm)
    sigma = (torch.rand(1, A, generator=g) * 0.4 + 0.1).to(DEV)
    wv = (torch.randn(D, generator=g) * 0.01).to(DEV)
    value = lambda rows: nm.normalize_torch(rows) @ wv
    first = pg.collect(env, pol, sigma, T, 5, 0, value, 0.99, 0.95)
    nm.update(first["obs_before"])
    assert nm.count == T * N and float(nm.scale.max()) != 1.0
    batch = pg.collect(env, pol, sigma, T, 5, T, value, 0.99, 0.95)
    raw, eps = batch["raw_action"], batch["eps"]
    assert bool(torch.isfinite(raw).all()) and bool(torch.isfinite(batch["obs_before"]).all())
    xn = nm.normalize_torch(batch["obs_before"])
    clipped = float((xn.abs() == 1.5).float().mean())
    assert 0.005 < clipped < 0.5, clipped
    mean = pg.policy_rows(pol, batch["obs_before"])
    u = mean + sigma * eps                                           # RN32(sigma * eps), then RN32(y + .)
    assert torch.equal(u.view(torch.int32), raw.view(torch.int32))
    plain = MLPPolicy(pol.w2, pol.b2, pol.w1, pol.b1)
    assert not torch.equal(pg.policy_rows(plain, batch["obs_before"]), mean)     # (the normaliser matters)
    assert torch.equal(pg.policy_rows(plain, xn).view(torch.int32), mean.view(torch.int32))
    dy = (-batch["adv"][..., None] / batch["adv"].numel()).expand(T, N, A).contiguous()
    (mean * dy).sum().backward()
    want = pg.policy_rows_backward(pol, batch["obs_before"], dy)
    for p, w in zip((pol.w1, pol.b1, pol.w2, pol.b2), want):
        assert torch.equal(p.grad.view(torch.int32), w.view(torch.int32))
    assert bool((pol.w1.grad != 0).any())


# ------------------------------------------------------------------ the ES trainer with a normaliser
@pytest.mark.parametrize("adaptive", [False, True], ids=["es", "pgpe"])
def test_es_trainer_with_obs_norm_equals_its_composition(adaptive):
    """Two generations on es_cases.balance128() with H = 5, G = 16: the trainer (its candidates and its rollout's
    obs_out through generation_step, the ObsNorm updated from every 64th walker's rows) against numpy perturb -> a
    second env's rollout under a second ObsNorm -> numpy update."""
    import torch
    import es_adaptive_cases as ac
    from walker_gym_amd.batched_env import BatchedPhysicsEnv
    from walker_gym_amd.es import AdaptiveEvolutionStrategy, EvolutionStrategy
    from walker_gym_amd.normalize import ObsNorm
    H, G = 5, 16
    env, ref_env = (BatchedPhysicsEnv(ec.balance128(), device=DEV, **ec.PARAMS) for _ in range(2))
    nm, ref_nm = ObsNorm(ec.D, DEV, clip=5.0), ObsNorm(ec.D, DEV, clip=5.0)
    args = dict(hidden=H, act_dim=ec.C, biases=True, population=G, seed=ec.SEED, theta0=ec.theta0(H), obs_norm=nm)
    if adaptive:
        cls = AdaptiveEvolutionStrategy
        args.update(sigma=ac.sigma0(H), lr=ac.LR_THETA[H], sigma_lr=ac.SIGMA_LR, sigma_max_change=ac.MAX_CHANGE,
                    sigma_min=ac.SIGMA_MIN, sigma_max=ac.SIGMA_MAX)
    else:
        cls = EvolutionStrategy
        args.update(sigma=ec.SIGMA[H], lr=ec.LR[H])
    tr = cls(env, **args)
    assert tr.policy.obs_norm is nm and tr.mean_policy().obs_norm is nm
    start = ref_env.batch.state_dict()
    theta, sig = ec.theta0(H), ac.sigma0(H)
    mask = torch.zeros((ec.T, ec.N_WALKERS), dtype=torch.uint8, device=DEV)
    mask[:, ::64] = 1
    rows, ref_rows = (torch.full((ec.T, ec.N_WALKERS, ec.D), float("nan"), device=DEV) for _ in range(2))
    for g in range(2):
        out = tr.generation_step(ec.T, obs_out=rows)
        nm.update(rows, mask)
        ref_env.batch.load_state_dict(start)
        pol = (ac.numpy_policy(theta, sig, g, H, G, device=DEV) if adaptive
               else ec.numpy_policy(theta, f32(ec.SIGMA[H]), g, H, G, device=DEV))
        pol.obs_norm = ref_nm
        res = ref_env.rollout_policy(pol, ec.T, obs_out=ref_rows)
        ref_nm.update(ref_rows, mask)
        fit = ec.set_fitness(res["returns"].cpu().numpy(), G)
        assert np.isfinite(fit).all() and _same(out["fitness"], fit), g
        assert _bits_equal(rows, ref_rows) and _bits_equal(nm.state, ref_nm.state) and _bits_equal(nm.scale, ref_nm.scale)
        if adaptive:
            grad, theta, g_sigma, sig = ac.numpy_tell(theta, sig, fit, g, H, G)
            assert _same(out["grad_sigma"], g_sigma) and _same(tr.sigma_vec, sig), g
        else:
            grad, theta = ec.numpy_tell(theta, fit, g, H, G)
        assert _same(out["grad"], grad) and _same(tr.theta, theta), g
    assert nm.count == 2 * ec.T * 2 and float(nm.mean.abs().max()) > 0
    # generation 1 ran under generation 0's statistics: without them its fitness is another
    plain = ec.numpy_policy(theta, f32(ec.SIGMA[H]), 0, H, G, device=DEV)
    ref_env.batch.load_state_dict(start)
    a = ref_env.rollout_policy(plain, ec.T)["returns"].clone()
    plain.obs_norm = nm
    ref_env.batch.load_state_dict(start)
    assert not torch.equal(a, ref_env.rollout_policy(plain, ec.T)["returns"])
    sd = tr.state_dict()
    assert _bits_equal(sd["obs_norm"]["state"], nm.state)
    fresh_nm = ObsNorm(ec.D, DEV, clip=1.0)
    fresh = cls(env, **dict(args, obs_norm=fresh_nm))
    fresh.load_state_dict(sd)
    assert _bits_equal(fresh_nm.state, nm.state) and _bits_equal(fresh_nm.mean, nm.mean) and fresh_nm.clip == 5.0

"""wg_es_perturb / wg_es_update and EvolutionStrategy on the GPU against the numpy restatements of walker_gym_amd.es.
Every comparison is byte for byte; tests/test_es_cpu.py checks the restatements themselves and that the trainer cases
stay finite."""
import ctypes as C

import numpy as np
import pytest

import es_cases as ec
from conftest import gpu_available

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED = ec.SEED
SENTINEL = -7.25
f32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.skip("no ROCm GPU")


def _same(a, b):
    a = a.detach().cpu().numpy() if hasattr(a, "detach") else a
    b = b.detach().cpu().numpy() if hasattr(b, "detach") else b
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _sets(shape, G, fill=SENTINEL, empty=False):
    """The four candidate tensors of wg_policy's layout (None for an absent one)."""
    import torch
    D, H, Cc, biases = shape
    mk = (lambda *s: torch.empty(s, dtype=torch.float32, device=DEV)) if empty else \
         (lambda *s: torch.full(s, fill, dtype=torch.float32, device=DEV))
    return dict(w1=mk(G, D, H) if H else None, b1=mk(G, H) if H and biases else None,
                w2=mk(G, H if H else D, Cc), b2=mk(G, Cc) if biases else None)


def _struct(shape, G, gen, sigma, theta, sets, seed=SEED):
    from walker_gym_amd import _lib
    D, H, Cc, _ = shape
    return _lib.WgEs(n_sets=G, obs_dim=D, hidden=H, act_dim=Cc, seed=seed, generation=gen, sigma=sigma,
                     theta=_ptr(theta), **{k: _ptr(v) for k, v in sets.items()})


def _perturb(shape, G, gen, sigma, theta, sets, first, n):
    import torch
    from walker_gym_amd import _lib
    st = _struct(shape, G, gen, sigma, theta, sets)
    _lib.check(_lib.load().wg_es_perturb(C.byref(st), first, n, None), "wg_es_perturb")
    torch.cuda.synchronize()


def _flat(sets, rows=slice(None)):
    """The sets' flat parameter vectors [rows, K] on the host, segments in theta's order."""
    parts = [sets[k][rows].reshape(sets[k][rows].shape[0], -1).cpu().numpy() for k in ("w1", "b1", "w2", "b2")
             if sets[k] is not None]
    return np.concatenate(parts, axis=1)


def _theta(K, seed=0):
    import torch
    t = (np.random.default_rng(seed).standard_normal(K) * 0.3).astype(f32)
    return t, torch.from_numpy(t).to(DEV)


SHAPES = [(26, 0, 2, True), (26, 5, 2, True), (152, 24, 5, False)]


# ------------------------------------------------------------------ perturb
@pytest.mark.parametrize("G", [2, 6, 514])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "D%d-H%d-C%d-%s" % s)
def test_perturb_equals_numpy(shape, G):
    from walker_gym_amd import es
    K = es.param_count(*shape)
    assert K == {0: 54, 5: 147, 24: 152 * 24 + 24 * 5}[shape[1]]
    th, th_d = _theta(K, seed=K + G)
    sigma = f32(0.05)
    for gen in (0, 7):
        sets = _sets(shape, G)
        _perturb(shape, G, gen, float(sigma), th_d, sets, 0, G // 2)
        want = es.es_perturb_numpy(th, sigma, SEED, gen, 0, G // 2)
        got = _flat(sets)
        assert not (got == f32(SENTINEL)).any()
        assert _same(got, want), (shape, G, gen)
    assert _same(th_d, th)   # theta is read only


def test_split_perturb_equals_one_call():
    shape, G = (26, 5, 2, True), 514
    th, th_d = _theta(147, seed=3)
    one, two = _sets(shape, G), _sets(shape, G)
    _perturb(shape, G, 2, 0.05, th_d, one, 0, 257)
    _perturb(shape, G, 2, 0.05, th_d, two, 0, 100)
    _perturb(shape, G, 2, 0.05, th_d, two, 100, 157)
    assert _same(_flat(one), _flat(two)) and not (_flat(one) == f32(SENTINEL)).any()


@pytest.mark.parametrize("shape", SHAPES[:2], ids=lambda s: "D%d-H%d-C%d-%s" % s)
def test_partial_range_leaves_the_other_sets_alone(shape):
    from walker_gym_amd import es
    G = 16
    K = es.param_count(*shape)
    th, th_d = _theta(K, seed=4)
    sets = _sets(shape, G)
    _perturb(shape, G, 1, 0.05, th_d, sets, 3, 2)
    got = _flat(sets)
    assert _same(got[6:10], es.es_perturb_numpy(th, f32(0.05), SEED, 1, 3, 2))
    assert (got[:6] == f32(SENTINEL)).all() and (got[10:] == f32(SENTINEL)).all()


def test_large_offsets():
    """The last pair of 65,536 sets of a 152 -> 256 -> 8 policy: w1's last set starts past element 2^31.  The tensors
    are allocated and never touched except by the call."""
    import torch
    from walker_gym_amd import es
    shape, G = (152, 256, 8, True), 65536
    if torch.cuda.mem_get_info()[0] < 16 << 30:
        pytest.skip("under 16 GB of device memory free")
    K = es.param_count(*shape)
    assert (G - 2) * 152 * 256 > 1 << 31
    th, th_d = _theta(K, seed=5)
    sets = _sets(shape, G, empty=True)
    for t in sets.values():
        t[G - 3:].fill_(SENTINEL)
    _perturb(shape, G, 7, 0.05, th_d, sets, G // 2 - 1, 1)
    got = _flat(sets, slice(G - 3, G))
    assert (got[0] == f32(SENTINEL)).all()
    assert _same(got[1:], es.es_perturb_numpy(th, f32(0.05), SEED, 7, G // 2 - 1, 1))


# ------------------------------------------------------------------ update
def _update(shape, G, gen, theta_d, util_d, first, n, scale, lr, grad=True, out="new"):
    """wg_es_update with dummy candidate tensors (only which of them are set matters); returns (grad, theta_out)."""
    import torch
    from walker_gym_amd import _lib, es
    K = es.param_count(*shape)
    dummy = torch.zeros(1, dtype=torch.float32, device=DEV)
    sets = dict(w1=dummy if shape[1] else None, b1=dummy if shape[1] and shape[3] else None, w2=dummy,
                b2=dummy if shape[3] else None)
    st = _struct(shape, G, gen, 0.05, theta_d, sets)
    work = torch.full((-(-n // 256), K), float("nan"), dtype=torch.float64, device=DEV)
    g = torch.full((K,), SENTINEL, dtype=torch.float32, device=DEV) if grad else None
    o = theta_d if out == "inplace" else (torch.full((K,), SENTINEL, dtype=torch.float32, device=DEV) if out else None)
    _lib.check(_lib.load().wg_es_update(C.byref(st), first, n, _ptr(util_d), scale, lr, _ptr(work), _ptr(g), _ptr(o),
                                        None), "wg_es_update")
    torch.cuda.synchronize()
    return g, o


@pytest.mark.parametrize("n_pairs", [1, 3, 256, 257, 600])
@pytest.mark.parametrize("shape", SHAPES[:2], ids=lambda s: "K%d" % (54 if s[1] == 0 else 147))
def test_update_equals_numpy(shape, n_pairs):
    import torch
    from walker_gym_amd import es
    K = es.param_count(*shape)
    first = 2 if n_pairs == 3 else 0
    G = 2 * (first + n_pairs)
    rng = np.random.default_rng(n_pairs + K)
    th, _ = _theta(K, seed=6)
    scale, lr, gen = 1.0 / (2 * n_pairs * 0.05), f32(0.3), 3
    plain = es.es_utilities_numpy(rng.standard_normal(G).astype(f32))
    ties = (rng.integers(-3, 4, G) / 8).astype(f32)                       # equal utilities, pairs with d_j = 0
    nan = plain.copy()
    nan[2 * (first + n_pairs // 2)] = np.nan
    for name, util in (("plain", plain), ("ties", ties), ("nan", nan)):
        want_g, want_t = es.es_update_numpy(th, util, SEED, gen, first, n_pairs, scale, lr)
        util_d = torch.from_numpy(util).to(DEV)
        fresh = lambda: torch.from_numpy(th.copy()).to(DEV)
        g, o = _update(shape, G, gen, fresh(), util_d, first, n_pairs, scale, float(lr))          # both
        assert _same(g, want_g) and _same(o, want_t), (name, "both")
        g, o = _update(shape, G, gen, fresh(), util_d, first, n_pairs, scale, float(lr), out=None)   # grad only
        assert o is None and _same(g, want_g), (name, "grad only")
        g, o = _update(shape, G, gen, fresh(), util_d, first, n_pairs, scale, float(lr), grad=False)  # theta_out only
        assert g is None and _same(o, want_t), (name, "theta_out only")
        t = fresh()
        g, o = _update(shape, G, gen, t, util_d, first, n_pairs, scale, float(lr), out="inplace")   # in place
        assert _same(g, want_g) and _same(t, want_t), (name, "in place")
        if name == "nan":
            assert np.isnan(want_g).all()
        else:
            assert np.isfinite(want_g).all() and (name == "ties" or np.all(want_g != 0))


# ------------------------------------------------------------------ the trainer
def _env():
    from walker_gym_amd.batched_env import BatchedPhysicsEnv
    return BatchedPhysicsEnv(ec.balance128(), device=DEV, **ec.PARAMS)


def _trainer(env, H, G, **kw):
    from walker_gym_amd.es import EvolutionStrategy
    args = dict(hidden=H, act_dim=ec.C, biases=True, population=G, sigma=ec.SIGMA[H], lr=ec.LR[H], seed=SEED,
                theta0=ec.theta0(H))
    args.update(kw)
    return EvolutionStrategy(env, **args)


@pytest.mark.parametrize("H,G", ec.TRAINER_CASES)
def test_trainer_equals_its_composition(H, G):
    import torch
    env, ref_env = _env(), _env()
    assert env.obs_dim == ec.D
    tr = _trainer(env, H, G)
    start = ref_env.batch.state_dict()
    theta = ec.theta0(H)
    saved = None
    for g in range(ec.GENERATIONS):
        out = tr.generation_step(ec.T)
        ref_env.batch.load_state_dict(start)
        pol = ec.numpy_policy(theta, f32(ec.SIGMA[H]), g, H, G, device=DEV)
        res = ref_env.rollout_policy(pol, ec.T)
        fit = ec.set_fitness(res["returns"].cpu().numpy(), G)
        grad, theta = ec.numpy_tell(theta, fit, g, H, G)
        assert out["generation"] == g and tr.generation == g + 1
        assert _same(out["fitness"], fit), g
        assert _same(out["grad"], grad), g
        assert _same(tr.theta, theta), g
        assert np.isfinite(fit).all() and np.isfinite(theta).all()
        assert float(out["fitness_max"]) == float(fit.max()) and float(out["fitness_min"]) == float(fit.min())
        if g == 0:
            saved = tr.state_dict()
    # the generations agree with the reference engine's too (tests/test_es_cpu.py keeps them finite)
    assert _same(theta, ec.oracle_training(H, G)[-1]["theta"])
    # resumed from the dict taken after the first generation, a fresh trainer arrives at the same theta
    fresh = _trainer(_env(), H, G, sigma=1.0, lr=0.0, seed=0, theta0=None)
    fresh.load_state_dict(saved)
    assert fresh.generation == 1
    for g in range(1, ec.GENERATIONS):
        fresh.generation_step(ec.T)
    assert _same(fresh.theta, theta)
    # mean_policy: theta as one shared parameter set
    mp = tr.mean_policy()
    assert mp.G == 1 and (mp.D, mp.H, mp.C) == (ec.D, H, ec.C)
    assert _same(torch.cat([t.reshape(-1) for t in (mp.w1, mp.b1, mp.w2, mp.b2) if t is not None]), theta)


def test_generation_step_with_auto_reset_equals_its_composition():
    """With auto-reset on the generation runs rollout_episodes; fitness is the reward per walker step over the finished
    episodes and the unfinished tail, summed in float64 over the set's walkers."""
    H, G = 5, 16
    env, ref_env = _env(), _env()
    for e in (env, ref_env):
        e.enable_auto_reset()
    tr = _trainer(env, H, G)
    start = ref_env.batch.state_dict()
    theta = ec.theta0(H)
    for g in range(2):
        out = tr.generation_step(ec.T)
        ref_env.batch.load_state_dict(start)
        res = ref_env.rollout_episodes(ec.numpy_policy(theta, f32(ec.SIGMA[H]), g, H, G, device=DEV), ec.T)
        assert int(res["episodes"].sum()) >= ec.N_WALKERS            # max_steps = 16 < T: every walker rolled over
        tot = res["return_sum"].cpu().numpy().astype(np.float64) + res["tail_return"].cpu().numpy().astype(np.float64)
        fit = (tot.reshape(G, -1).sum(axis=1) / (ec.N_WALKERS // G * ec.T)).astype(f32)
        grad, theta = ec.numpy_tell(theta, fit, g, H, G)
        assert np.isfinite(fit).all() and len(np.unique(fit)) > G // 2
        assert _same(out["fitness"], fit) and _same(out["grad"], grad) and _same(tr.theta, theta), g


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_quadratic_descends_on_the_device(seed):
    import torch
    K, G = 54, 64
    target = torch.from_numpy(np.random.default_rng(seed).standard_normal(K).astype(f32)).to(DEV)
    tr = _trainer(_env(), 0, G, sigma=0.1, lr=0.2, seed=seed, theta0=np.zeros(K, f32))
    assert tr.K == K
    loss0 = float(((tr.theta - target).double() ** 2).sum())
    for gen in range(30):
        pol = tr.ask()
        cand = torch.cat([pol.w2.reshape(G, -1), pol.b2], dim=1)
        tr.tell(-((cand - target[None]) ** 2).sum(dim=1))
    loss = float(((tr.theta - target).double() ** 2).sum())
    print("seed", seed, "loss ratio", loss / loss0)
    assert tr.generation == 30 and loss < 0.1 * loss0


def test_trainer_refusals(monkeypatch):
    import torch
    env = _env()
    with pytest.raises(ValueError, match="even"):
        _trainer(env, 0, 3)
    with pytest.raises(ValueError, match="even"):
        _trainer(env, 0, 0)
    with pytest.raises(ValueError, match="divide"):
        _trainer(env, 0, 6)
    with pytest.raises(ValueError, match="theta0"):
        _trainer(env, 0, 16, theta0=np.zeros(55, f32))
    with pytest.raises(ValueError, match="sigma"):
        _trainer(env, 0, 16, sigma=0.0)
    tr = _trainer(env, 0, 16)
    with pytest.raises(ValueError, match="fitness"):
        tr.tell(torch.zeros(15, device=DEV))
    assert tr.generation == 0
    # the rollout's own refusal: resident batches only (nothing launched, nothing updated)
    before = tr.theta.clone()
    monkeypatch.setenv("WG_LEAN", "0")
    with pytest.raises(ValueError, match="resident"):
        tr.generation_step(ec.T)
    assert tr.generation == 0 and _same(tr.theta, before)

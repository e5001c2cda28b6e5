"""wg_es_perturb_diag / wg_es_update_diag and AdaptiveEvolutionStrategy on the GPU against the numpy restatements of
walker_gym_amd.es.  Every comparison is bit for bit (a NaN that an operation creates compares as a NaN: its sign is not
contracted); tests/test_es_adaptive_cpu.py checks the restatements themselves and the trainer cases' conditions."""
import ctypes as C

import numpy as np
import pytest

import es_adaptive_cases as ac
import es_cases as ec
from conftest import gpu_available

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED = ac.SEED
SENTINEL = -7.25
f32 = np.float32
SHAPES = [(26, 0, 2, True), (26, 5, 2, True), (152, 24, 5, False)]      # tests/test_gpu_es.py's: K = 54, 147, 3,768
# and three shapes at the size where wg_es_update_diag changes the form of its partial kernel (256 workgroups of the
# one-thread form, chunks x blocks of 256 parameters): 1 x 256 and 2 x 128 take it, 1 x 255 the spread form
SHAPE_OF_K = {54: SHAPES[0], 147: SHAPES[1], 3768: SHAPES[2], 65536: (255, 256, 1, False), 65280: (254, 256, 1, False),
              32768: (127, 256, 1, False)}


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.skip("no ROCm GPU")


def _host(a):
    return np.ascontiguousarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a)


def _same(a, b):
    a, b = _host(a), _host(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _same_nan(a, b):
    return ac.same_bits_nan_equal(_host(a), _host(b))


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _dev(a):
    import torch
    return torch.from_numpy(np.array(a, copy=True)).to(DEV)


def _sets(shape, G, fill=SENTINEL):
    import torch
    D, H, Cc, biases = shape
    mk = lambda *s: torch.full(s, fill, dtype=torch.float32, device=DEV)
    return dict(w1=mk(G, D, H) if H else None, b1=mk(G, H) if H and biases else None,
                w2=mk(G, H if H else D, Cc), b2=mk(G, Cc) if biases else None)


def _struct(shape, G, gen, theta, sets, sigma=0.0, seed=SEED):
    """es->sigma is 0 unless a test sets it: the _diag calls do not read it."""
    from walker_gym_amd import _lib
    D, H, Cc, _ = shape
    return _lib.WgEs(n_sets=G, obs_dim=D, hidden=H, act_dim=Cc, seed=seed, generation=gen, sigma=sigma,
                     theta=_ptr(theta), **{k: _ptr(v) for k, v in sets.items()})


def _perturb(shape, G, gen, theta, sigma_d, sets, first, n):
    import torch
    from walker_gym_amd import _lib
    st = _struct(shape, G, gen, theta, sets)
    _lib.check(_lib.load().wg_es_perturb_diag(C.byref(st), _ptr(sigma_d), first, n, None), "wg_es_perturb_diag")
    torch.cuda.synchronize()


def _flat(sets, rows=slice(None)):
    parts = [sets[k][rows].reshape(sets[k][rows].shape[0], -1).cpu().numpy() for k in ("w1", "b1", "w2", "b2")
             if sets[k] is not None]
    return np.concatenate(parts, axis=1)


def _theta_sigma(K, seed):
    rng = np.random.default_rng(seed)
    th = (rng.standard_normal(K) * 0.3).astype(f32)
    sg = (10.0 ** rng.uniform(-3, 1, K)).astype(f32)
    return th, sg, _dev(th), _dev(sg)


# ------------------------------------------------------------------ perturb
@pytest.mark.parametrize("G", [2, 6, 514])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "D%d-H%d-C%d-%s" % s)
def test_perturb_equals_numpy(shape, G):
    from walker_gym_amd import es
    K = es.param_count(*shape)
    th, sg, th_d, sg_d = _theta_sigma(K, K + G)
    for gen in (0, 7):
        sets = _sets(shape, G)
        _perturb(shape, G, gen, th_d, sg_d, sets, 0, G // 2)
        got = _flat(sets)
        assert not (got == f32(SENTINEL)).any()
        assert _same(got, es.es_perturb_diag_numpy(th, sg, SEED, gen, 0, G // 2)), (shape, G, gen)
    assert _same(th_d, th) and _same(sg_d, sg)          # both are read only


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "D%d-H%d-C%d-%s" % s)
def test_constant_sigma_equals_wg_es_perturb(shape):
    import torch
    from walker_gym_amd import _lib, es
    K, G, s = es.param_count(*shape), 514, float(f32(0.05))
    th, _, th_d, _ = _theta_sigma(K, 11)
    a, b = _sets(shape, G), _sets(shape, G)
    _perturb(shape, G, 4, th_d, torch.full((K,), s, dtype=torch.float32, device=DEV), a, 0, G // 2)
    st = _struct(shape, G, 4, th_d, b, sigma=s)
    _lib.check(_lib.load().wg_es_perturb(C.byref(st), 0, G // 2, None), "wg_es_perturb")
    torch.cuda.synchronize()
    assert _same(_flat(a), _flat(b)) and not (_flat(a) == f32(SENTINEL)).any()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "D%d-H%d-C%d-%s" % s)
def test_partial_range_leaves_the_other_sets_alone(shape):
    from walker_gym_amd import es
    G, K = 16, es.param_count(*shape)
    th, sg, th_d, sg_d = _theta_sigma(K, 4)
    sets = _sets(shape, G)
    _perturb(shape, G, 1, th_d, sg_d, sets, 3, 2)
    got = _flat(sets)
    assert _same(got[6:10], es.es_perturb_diag_numpy(th, sg, SEED, 1, 3, 2))
    assert (got[:6] == f32(SENTINEL)).all() and (got[10:] == f32(SENTINEL)).all()


@pytest.mark.parametrize("shape", SHAPES[1:], ids=lambda s: "D%d-H%d-C%d-%s" % s)
def test_two_half_range_calls_equal_one_call(shape):
    from walker_gym_amd import es
    G, K = 514, es.param_count(*shape)
    th, sg, th_d, sg_d = _theta_sigma(K, 3)
    one, two = _sets(shape, G), _sets(shape, G)
    _perturb(shape, G, 2, th_d, sg_d, one, 0, 257)
    _perturb(shape, G, 2, th_d, sg_d, two, 0, 100)
    _perturb(shape, G, 2, th_d, sg_d, two, 100, 157)
    assert _same(_flat(one), _flat(two)) and not (_flat(one) == f32(SENTINEL)).any()


# ------------------------------------------------------------------ update
OUTS = ("g_theta", "theta_out", "g_sigma", "sigma_out")


def _update(K, G, gen, theta, sigma, util, first, n, step, skip=(), inplace=False):
    """wg_es_update_diag with dummy candidate tensors (only which of them are set matters).  Returns the four outputs
    (None for one in `skip`; with `inplace` theta_out and sigma_out are the device copies of theta and sigma
    themselves) and the device theta and sigma."""
    import torch
    from walker_gym_amd import _lib
    shape = SHAPE_OF_K[K]
    dummy = torch.zeros(1, dtype=torch.float32, device=DEV)
    sets = dict(w1=dummy if shape[1] else None, b1=dummy if shape[1] and shape[3] else None, w2=dummy,
                b2=dummy if shape[3] else None)
    th_d, sg_d, util_d = _dev(theta), _dev(sigma), _dev(util)
    st = _struct(shape, G, gen, th_d, sets)
    work = torch.full((2, -(-n // 256), K), float("nan"), dtype=torch.float64, device=DEV)
    new = lambda: torch.full((K,), SENTINEL, dtype=torch.float32, device=DEV)
    outs = {o: None if o in skip else new() for o in OUTS}
    if inplace:
        outs["theta_out"], outs["sigma_out"] = th_d, sg_d
    cs = _lib.WgEsDiagStep(**step)
    _lib.check(_lib.load().wg_es_update_diag(C.byref(st), _ptr(sg_d), first, n, _ptr(util_d), C.byref(cs), _ptr(work),
                                             *[_ptr(outs[o]) for o in OUTS], None), "wg_es_update_diag")
    torch.cuda.synchronize()
    return [outs[o] for o in OUTS], th_d, sg_d


UPDATE_CASES = [(K, n) for K in (54, 147) for n in ac.UPDATE_PAIRS] + [(3768, 3), (3768, 257)] + \
               [(65536, 3), (65280, 3), (32768, 257)]


@pytest.mark.parametrize("K,n_pairs", UPDATE_CASES, ids=["K%d-n%d" % c for c in UPDATE_CASES])
def test_update_equals_numpy(K, n_pairs):
    """The chunk edges (1, 3, 256, 257, 600 pairs), blocks of k that no tile width divides (54, 147, 3,768), pairs from
    first_pair = 2 on; per util vector: all four outputs, each output NULL in turn, in place, and the same call twice.
    The three large K run both forms of the partial kernel on either side of the size that chooses between them (the
    two-chunk one with the centred ranks alone: its restatement takes seconds)."""
    from walker_gym_amd import es
    assert es.param_count(*SHAPE_OF_K[K]) == K
    c = ac.update_inputs(K, n_pairs)
    th, sg, G, step = c["theta"], c["sigma"], c["G"], ac.update_step(n_pairs)
    names = list(c["utils"]) if K < 32768 else (["plain"] if n_pairs > 3 else ["plain", "inf_both"])
    for name in names:
        util = c["utils"][name]
        want = ac.update_reference(K, n_pairs, name)
        run = lambda **kw: _update(K, G, ac.GEN, th, sg, util, ac.FIRST, n_pairs, step, **kw)
        got, th_d, sg_d = run()
        for o, g, w in zip(OUTS, got, want):
            assert _same_nan(g, w), (name, o)
        assert _same(th_d, th) and _same(sg_d, sg)                     # inputs untouched when the outputs are elsewhere
        again, _, _ = run()
        assert all(_same(a, b) for a, b in zip(got, again)), (name, "twice")          # NaN bits included
        if name in ("plain", "inf_both"):
            for skipped in OUTS:
                part, _, _ = run(skip=(skipped,))
                for o, g, w in zip(OUTS, part, want):
                    assert (g is None) if o == skipped else _same_nan(g, w), (name, "without " + skipped, o)
        got, th_d, sg_d = run(inplace=True)
        for o, g, w in zip(OUTS, got, want):
            assert _same_nan(g, w), (name, "in place", o)
        assert _same_nan(th_d, want[1]) and _same_nan(sg_d, want[3]), (name, "in place")


@pytest.mark.parametrize("name", sorted(ac.CLAMP_CASES))
def test_clamp_cases_equal_numpy(name):
    c = ac.update_inputs(ac.CLAMP_K, ac.CLAMP_PAIRS)
    step, want = ac.clamp_reference(name)
    got, _, _ = _update(ac.CLAMP_K, c["G"], ac.GEN, c["theta"], c["sigma"], c["utils"]["plain"], ac.FIRST,
                        ac.CLAMP_PAIRS, step)
    for o, g, w in zip(OUTS, got, want):
        assert _same(g, w), (name, o)
    br = ac.clamp_branches(c["sigma"], _host(got[2]), step)
    assert len(set(br)) >= 3        # the shares are asserted in tests/test_es_adaptive_cpu.py


# ------------------------------------------------------------------ the trainer
def _env():
    from walker_gym_amd.batched_env import BatchedPhysicsEnv
    return BatchedPhysicsEnv(ec.balance128(), device=DEV, **ec.PARAMS)


def _trainer(env, H, G, **kw):
    from walker_gym_amd.es import AdaptiveEvolutionStrategy
    args = dict(hidden=H, act_dim=ec.C, biases=True, population=G, sigma=ac.sigma0(H), lr=ac.LR_THETA[H], seed=SEED,
                theta0=ec.theta0(H), sigma_lr=ac.SIGMA_LR, sigma_max_change=ac.MAX_CHANGE, sigma_min=ac.SIGMA_MIN,
                sigma_max=ac.SIGMA_MAX)
    args.update(kw)
    return AdaptiveEvolutionStrategy(env, **args)


@pytest.mark.parametrize("H,G", ec.TRAINER_CASES)
def test_trainer_equals_its_composition(H, G):
    import torch
    env, ref_env = _env(), _env()
    tr = _trainer(env, H, G)
    assert tr.step_fields() == ac.trainer_step(H, G) and tr.sigma == 0.0
    start = ref_env.batch.state_dict()
    theta, sigma = ec.theta0(H), ac.sigma0(H)
    saved = None
    for g in range(ec.GENERATIONS):
        out = tr.generation_step(ec.T)
        ref_env.batch.load_state_dict(start)
        res = ref_env.rollout_policy(ac.numpy_policy(theta, sigma, g, H, G, device=DEV), ec.T)
        fit = ec.set_fitness(res["returns"].cpu().numpy(), G)
        g_theta, theta, g_sigma, sigma = ac.numpy_tell(theta, sigma, fit, g, H, G)
        assert out["generation"] == g and tr.generation == g + 1
        assert _same(out["fitness"], fit), g
        assert _same(out["grad"], g_theta) and _same(out["grad_sigma"], g_sigma), g
        assert _same(tr.theta, theta) and _same(tr.sigma_vec, sigma), g
        assert np.isfinite(fit).all() and np.isfinite(theta).all() and (sigma > 0).all()
        for key, want in (("sigma_min", sigma.min()), ("sigma_max", sigma.max())):
            assert isinstance(out[key], torch.Tensor) and out[key].dim() == 0 and float(out[key]) == float(want)
        assert abs(float(out["sigma_mean"]) - float(sigma.astype(np.float64).mean())) < 1e-6 * float(sigma.max())
        assert float(out["fitness_max"]) == float(fit.max()) and float(out["fitness_min"]) == float(fit.min())
        if g == 0:
            saved = tr.state_dict()
    # the generations agree with the reference engine's too (tests/test_es_adaptive_cpu.py keeps them finite)
    last = ac.oracle_training(H, G)[-1]
    assert _same(theta, last["theta"]) and _same(sigma, last["sigma"])
    # resumed from the dict taken after the first generation, a fresh trainer arrives at the same theta and sigma_vec
    fresh = _trainer(_env(), H, G, sigma=1.0, lr=0.0, seed=0, theta0=None, sigma_lr=0.5, sigma_max_change=0.5,
                     sigma_min=1e-3, sigma_max=10.0)
    fresh.load_state_dict(saved)
    assert fresh.generation == 1 and fresh.step_fields() == ac.trainer_step(H, G)
    for g in range(1, ec.GENERATIONS):
        fresh.generation_step(ec.T)
    assert _same(fresh.theta, theta) and _same(fresh.sigma_vec, sigma)
    mp = tr.mean_policy()                               # inherited: theta as one shared parameter set
    assert mp.G == 1 and (mp.D, mp.H, mp.C) == (ec.D, H, ec.C)
    assert _same(torch.cat([t.reshape(-1) for t in (mp.w1, mp.b1, mp.w2, mp.b2) if t is not None]), theta)


def test_generation_step_with_auto_reset_equals_its_composition():
    H, G = 5, 16
    env, ref_env = _env(), _env()
    for e in (env, ref_env):
        e.enable_auto_reset()
    tr = _trainer(env, H, G)
    start = ref_env.batch.state_dict()
    theta, sigma = ec.theta0(H), ac.sigma0(H)
    for g in range(2):
        out = tr.generation_step(ec.T)
        ref_env.batch.load_state_dict(start)
        res = ref_env.rollout_episodes(ac.numpy_policy(theta, sigma, g, H, G, device=DEV), ec.T)
        assert int(res["episodes"].sum()) >= ec.N_WALKERS            # max_steps = 16 < T: every walker rolled over
        tot = res["return_sum"].cpu().numpy().astype(np.float64) + res["tail_return"].cpu().numpy().astype(np.float64)
        fit = (tot.reshape(G, -1).sum(axis=1) / (ec.N_WALKERS // G * ec.T)).astype(f32)
        g_theta, theta, g_sigma, sigma = ac.numpy_tell(theta, sigma, fit, g, H, G)
        assert np.isfinite(fit).all() and len(np.unique(fit)) > G // 2
        assert _same(out["fitness"], fit) and _same(out["grad"], g_theta) and _same(out["grad_sigma"], g_sigma), g
        assert _same(tr.theta, theta) and _same(tr.sigma_vec, sigma), g


@pytest.mark.parametrize("seed", ac.QUAD_SEEDS)
def test_quadratic_on_the_device_equals_the_restatement(seed):
    """tests/test_es_adaptive_cpu.py's quadratic through ask() / tell(): theta and sigma_vec after 30 generations in
    bits.  The fitness is quadratic_fitness's sum, float32 in element order, with torch's elementwise operations."""
    import torch
    target, theta, sigma, _, _ = ac.quadratic_numpy(seed)
    K, G = ac.QUAD_K, ac.QUAD_G
    tr = _trainer(_env(), 0, G, sigma=ac.QUAD["sigma"], lr=ac.QUAD["lr"], seed=seed, theta0=np.zeros(K, f32))
    assert tr.K == K and tr.step_fields() == ac.quadratic_step()
    tg = _dev(target)
    for gen in range(ac.QUAD_GENERATIONS):
        pol = tr.ask()
        sq = (torch.cat([pol.w2.reshape(G, -1), pol.b2], dim=1) - tg[None]) ** 2
        acc = torch.zeros(G, dtype=torch.float32, device=DEV)
        for k in range(K):
            acc = acc + sq[:, k]
        out = tr.tell(-acc)
        assert set(out) == {"grad", "grad_sigma"}
    assert tr.generation == ac.QUAD_GENERATIONS
    assert _same(tr.theta, theta) and _same(tr.sigma_vec, sigma)


def test_trainer_refusals(monkeypatch):
    import torch
    env = _env()
    with pytest.raises(ValueError, match="sigma"):
        _trainer(env, 0, 16, sigma=np.full(55, 0.001, f32))                  # a wrong length
    with pytest.raises(ValueError, match="sigma"):
        _trainer(env, 0, 16, sigma=np.where(np.arange(54) == 7, 0.0, 0.001).astype(f32))   # a zero entry
    with pytest.raises(ValueError, match="sigma"):
        _trainer(env, 0, 16, sigma=np.where(np.arange(54) == 7, -0.001, 0.001).astype(f32))
    with pytest.raises(ValueError, match="sigma"):
        _trainer(env, 0, 16, sigma=0.0)
    with pytest.raises(ValueError, match="sigma"):
        _trainer(env, 0, 16, sigma=float("nan"))
    # the parent's list
    with pytest.raises(ValueError, match="even"):
        _trainer(env, 0, 3)
    with pytest.raises(ValueError, match="even"):
        _trainer(env, 0, 0)
    with pytest.raises(ValueError, match="divide"):
        _trainer(env, 0, 6)
    with pytest.raises(ValueError, match="theta0"):
        _trainer(env, 0, 16, theta0=np.zeros(55, f32))
    tr = _trainer(env, 0, 16)
    with pytest.raises(ValueError, match="fitness"):
        tr.tell(torch.zeros(15, device=DEV))
    assert tr.generation == 0
    with pytest.raises(ValueError, match="sigma_vec"):
        tr.load_state_dict(dict(tr.state_dict(), sigma_vec=torch.ones(55)))
    # the rollout's own refusal: resident batches only (nothing launched, nothing updated)
    theta, sigma = tr.theta.clone(), tr.sigma_vec.clone()
    monkeypatch.setenv("WG_LEAN", "0")
    with pytest.raises(ValueError, match="resident"):
        tr.generation_step(ec.T)
    assert tr.generation == 0 and _same(tr.theta, theta) and _same(tr.sigma_vec, sigma)

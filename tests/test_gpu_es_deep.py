"""The four wg_es_*_deep entries and the trainers with hidden2 > 0 on the GPU against the numpy restatements of
walker_gym_amd.es, which work on any K.  Every comparison is byte for byte (a NaN that an operation creates compares as a
NaN, as in tests/test_gpu_es_adaptive.py); tests/test_es_deep_cpu.py checks the layout and the trainer cases' conditions."""
import ctypes as C

import numpy as np
import pytest

import es_adaptive_cases as ac
import es_cases as ec
import es_deep_cases as dz
from conftest import gpu_available

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEED = dz.SEED
SENTINEL = -7.25
f32 = np.float32
NAMES = ("w1", "b1", "wm", "bm", "w2", "b2")


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


def _sets(shape, G, fill=SENTINEL, empty=False):
    """The six candidate tensors of a deep MLPPolicy's layout (None for an absent bias)."""
    import torch
    D, H1, H2, Cc, b1, bm, b2 = shape
    mk = (lambda *s: torch.empty(s, dtype=torch.float32, device=DEV)) if empty else \
         (lambda *s: torch.full(s, fill, dtype=torch.float32, device=DEV))
    return dict(w1=mk(G, D, H1), b1=mk(G, H1) if b1 else None, wm=mk(G, H1, H2), bm=mk(G, H2) if bm else None,
                w2=mk(G, H2, Cc), b2=mk(G, Cc) if b2 else None)


def _structs(shape, G, gen, theta, sets, sigma=0.05, seed=SEED):
    from walker_gym_amd import _lib
    D, H1, H2, Cc = shape[:4]
    es = _lib.WgEs(n_sets=G, obs_dim=D, hidden=H1, act_dim=Cc, seed=seed, generation=gen, sigma=sigma, theta=_ptr(theta),
                   w1=_ptr(sets["w1"]), b1=_ptr(sets["b1"]), w2=_ptr(sets["w2"]), b2=_ptr(sets["b2"]))
    return es, _lib.WgEsMid(hidden2=H2, wm=_ptr(sets["wm"]), bm=_ptr(sets["bm"]))


def _perturb(shape, G, gen, theta, sigma, sets, first, n):
    """wg_es_perturb_deep (a float sigma) or wg_es_perturb_diag_deep (a device vector)."""
    import torch
    from walker_gym_amd import _lib
    if isinstance(sigma, float):
        es, mid = _structs(shape, G, gen, theta, sets, sigma=sigma)
        _lib.check(_lib.load().wg_es_perturb_deep(C.byref(es), C.byref(mid), first, n, None), "wg_es_perturb_deep")
    else:
        es, mid = _structs(shape, G, gen, theta, sets, sigma=0.0)
        _lib.check(_lib.load().wg_es_perturb_diag_deep(C.byref(es), C.byref(mid), _ptr(sigma), first, n, None),
                   "wg_es_perturb_diag_deep")
    torch.cuda.synchronize()


def _flat(sets, rows=slice(None)):
    """The sets' flat parameter vectors [rows, K] on the host, the six segments in theta's order."""
    parts = [sets[k][rows].reshape(sets[k][rows].shape[0], -1).cpu().numpy() for k in NAMES if sets[k] is not None]
    return np.concatenate(parts, axis=1)


def _theta_sigma(K, seed):
    rng = np.random.default_rng(seed)
    th = (rng.standard_normal(K) * 0.3).astype(f32)
    sg = (10.0 ** rng.uniform(-3, 1, K)).astype(f32)
    return th, sg, _dev(th), _dev(sg)


def _want(diag, th, sg, gen, first, n):
    from walker_gym_amd import es
    return es.es_perturb_diag_numpy(th, sg, SEED, gen, first, n) if diag else \
        es.es_perturb_numpy(th, f32(0.05), SEED, gen, first, n)


FORMS = pytest.mark.parametrize("diag", [False, True], ids=["scalar", "diag"])


# ------------------------------------------------------------------ perturb
@FORMS
@pytest.mark.parametrize("G", [2, 6, 514])
@pytest.mark.parametrize("shape", dz.SHAPES, ids=dz.shape_id)
def test_perturb_equals_numpy(shape, G, diag):
    from walker_gym_amd import es
    K = dz.K_of(shape)
    assert SEED >> 32                                    # both key words in use
    if all(shape[4:]):
        assert es.param_count(shape[0], shape[1], shape[3], True, shape[2]) == K
    th, sg, th_d, sg_d = _theta_sigma(K, K + G)
    for gen in (0, 7):
        sets = _sets(shape, G)
        _perturb(shape, G, gen, th_d, sg_d if diag else 0.05, sets, 0, G // 2)
        got = _flat(sets)
        assert got.shape == (G, K) and not (got == f32(SENTINEL)).any()
        assert _same(got, _want(diag, th, sg, gen, 0, G // 2)), (shape, G, gen)
    assert _same(th_d, th) and _same(sg_d, sg)          # theta and sigma are read only


@FORMS
@pytest.mark.parametrize("shape", [dz.SHAPES[0], dz.SHAPES[3], dz.SHAPES[5]], ids=dz.shape_id)
def test_split_ranges_equal_one_call(shape, diag):
    G, K = 514, dz.K_of(shape)
    th, sg, th_d, sg_d = _theta_sigma(K, 3)
    s = sg_d if diag else 0.05
    one, two = _sets(shape, G), _sets(shape, G)
    _perturb(shape, G, 2, th_d, s, one, 0, 257)
    _perturb(shape, G, 2, th_d, s, two, 0, 100)
    _perturb(shape, G, 2, th_d, s, two, 100, 157)
    assert _same(_flat(one), _flat(two)) and not (_flat(one) == f32(SENTINEL)).any()


@FORMS
@pytest.mark.parametrize("shape", [dz.SHAPES[0], dz.SHAPES[2], dz.SHAPES[4]], ids=dz.shape_id)
def test_partial_range_leaves_the_other_sets_alone(shape, diag):
    G, K = 16, dz.K_of(shape)
    th, sg, th_d, sg_d = _theta_sigma(K, 4)
    sets = _sets(shape, G)
    _perturb(shape, G, 1, th_d, sg_d if diag else 0.05, sets, 3, 2)
    assert _same(_flat(sets)[6:10], _want(diag, th, sg, 1, 3, 2))
    for name in NAMES:                                                   # each of the six tensors on its own
        t = sets[name].cpu().numpy()
        assert (t[:6] == f32(SENTINEL)).all() and (t[10:] == f32(SENTINEL)).all(), name
        assert not (t[6:10] == f32(SENTINEL)).any(), name


@FORMS
@pytest.mark.parametrize("shape", [dz.SHAPES[0], dz.SHAPES[2], dz.SHAPES[3], dz.SHAPES[4]], ids=dz.shape_id)
def test_shared_prefix_equals_the_shallow_entry(shape, diag):
    """w1 / b1 of a deep call are wg_es_perturb's (wg_es_perturb_diag's) bytes on the same theta prefix: the noise is a
    function of (pair, k) only, and both layouts start with w1, b1."""
    import torch
    from walker_gym_amd import _lib
    D, H1, H2, Cc, b1 = shape[:5]
    G, K = 514, dz.K_of(shape)
    th, sg, th_d, sg_d = _theta_sigma(K, 12)
    deep = _sets(shape, G)
    _perturb(shape, G, 4, th_d, sg_d if diag else 0.05, deep, 0, G // 2)
    mk = lambda *s: torch.full(s, SENTINEL, dtype=torch.float32, device=DEV)
    sh = dict(w1=mk(G, D, H1), b1=mk(G, H1) if b1 else None, w2=mk(G, H1, Cc), b2=None)   # K' >= the prefix's length
    st = _lib.WgEs(n_sets=G, obs_dim=D, hidden=H1, act_dim=Cc, seed=SEED, generation=4, sigma=0.05, theta=_ptr(th_d),
                   **{k: _ptr(v) for k, v in sh.items()})
    assert D * H1 + (H1 if b1 else 0) + H1 * Cc <= K                    # the shallow call reads theta inside its bounds
    if diag:
        _lib.check(_lib.load().wg_es_perturb_diag(C.byref(st), _ptr(sg_d), 0, G // 2, None), "wg_es_perturb_diag")
    else:
        _lib.check(_lib.load().wg_es_perturb(C.byref(st), 0, G // 2, None), "wg_es_perturb")
    torch.cuda.synchronize()
    assert _same(deep["w1"], sh["w1"]) and not (_host(sh["w1"]) == f32(SENTINEL)).any()
    if b1:
        assert _same(deep["b1"], sh["b1"])


@FORMS
def test_large_offsets(diag):
    """The last pair of 32,772 sets of an 8 -> 256 -> 256 -> 1 policy: wm's last set starts past element 2^31.  The
    tensors are allocated and never touched except by the call (and the sentinel in the last three sets)."""
    import torch
    shape, G = (8, 256, 256, 1, True, True, True), 32772
    if torch.cuda.mem_get_info()[0] < 12 << 30:
        pytest.skip("under 12 GB of device memory free")
    K = dz.K_of(shape)
    assert (G - 1) * 256 * 256 > 1 << 31 and G * 256 * 256 * 4 < 9 << 30
    th, sg, th_d, sg_d = _theta_sigma(K, 5)
    sets = _sets(shape, G, empty=True)
    for t in sets.values():
        t[G - 3:].fill_(SENTINEL)
    _perturb(shape, G, 7, th_d, sg_d if diag else 0.05, sets, G // 2 - 1, 1)
    got = _flat(sets, slice(G - 3, G))
    assert (got[0] == f32(SENTINEL)).all()
    assert _same(got[1:], _want(diag, th, sg, 7, G // 2 - 1, 1))


# ------------------------------------------------------------------ update
DEEP_OF_K = {35: dz.SHAPES[0], 161: dz.SHAPES[2], 65536: (896, 64, 64, 64, False, False, False),
             65280: (892, 64, 64, 64, False, False, False)}
SHALLOW_OF_K = {35: (6, 0, 5, True), 161: (22, 0, 7, True), 65536: (255, 256, 1, False), 65280: (254, 256, 1, False)}
OUTS = ("g_theta", "theta_out", "g_sigma", "sigma_out")


def _dummies(K, deep):
    """(wg_es, wg_es_mid or None, what keeps their tensors alive) with dummy candidate tensors: only which are set
    matters to an update."""
    import torch
    from walker_gym_amd import _lib, es
    d = torch.zeros(1, dtype=torch.float32, device=DEV)
    if deep:
        shape = DEEP_OF_K[K]
        assert dz.K_of(shape) == K
        D, H1, H2, Cc, b1, bm, b2 = shape
        sets = dict(w1=d, b1=d if b1 else None, wm=d, bm=d if bm else None, w2=d, b2=d if b2 else None)
        return shape, sets
    shape = SHALLOW_OF_K[K]
    assert es.param_count(*shape) == K
    return shape, dict(w1=d if shape[1] else None, b1=d if shape[1] and shape[3] else None, w2=d,
                       b2=d if shape[3] else None)


def _update(K, deep, G, gen, theta, util, first, n, scale, lr, grad=True, out="new"):
    """wg_es_update_deep (deep) or wg_es_update on a layout of the same K: (grad, theta_out, the device theta)."""
    import torch
    from walker_gym_amd import _lib
    shape, sets = _dummies(K, deep)
    th_d, util_d = _dev(theta), _dev(util)
    work = torch.full((-(-n // 256), K), float("nan"), dtype=torch.float64, device=DEV)
    g = torch.full((K,), SENTINEL, dtype=torch.float32, device=DEV) if grad else None
    o = th_d if out == "inplace" else (torch.full((K,), SENTINEL, dtype=torch.float32, device=DEV) if out else None)
    tail = (first, n, _ptr(util_d), scale, lr, _ptr(work), _ptr(g), _ptr(o), None)
    if deep:
        es, mid = _structs(shape, G, gen, th_d, sets)
        _lib.check(_lib.load().wg_es_update_deep(C.byref(es), C.byref(mid), *tail), "wg_es_update_deep")
    else:
        D, H, Cc, _ = shape
        es = _lib.WgEs(n_sets=G, obs_dim=D, hidden=H, act_dim=Cc, seed=SEED, generation=gen, sigma=0.05,
                       theta=_ptr(th_d), **{k: _ptr(v) for k, v in sets.items()})
        _lib.check(_lib.load().wg_es_update(C.byref(es), *tail), "wg_es_update")
    torch.cuda.synchronize()
    return g, o, th_d


@pytest.mark.parametrize("n_pairs", [1, 3, 256, 257, 600])
@pytest.mark.parametrize("K", [35, 161])
def test_update_equals_numpy_and_the_shallow_entry(K, n_pairs):
    from walker_gym_amd import es
    first = 2 if n_pairs == 3 else 0
    G = 2 * (first + n_pairs)
    rng = np.random.default_rng(n_pairs + K)
    th = (rng.standard_normal(K) * 0.3).astype(f32)
    scale, lr, gen = 1.0 / (2 * n_pairs * 0.05), f32(0.3), 3
    plain = es.es_utilities_numpy(rng.standard_normal(G).astype(f32))
    ties = (rng.integers(-3, 4, G) / 8).astype(f32)
    nan = plain.copy()
    nan[2 * (first + n_pairs // 2)] = np.nan
    for name, util in (("plain", plain), ("ties", ties), ("nan", nan)):
        want_g, want_t = es.es_update_numpy(th, util, SEED, gen, first, n_pairs, scale, lr)
        run = lambda deep=True, **kw: _update(K, deep, G, gen, th, util, first, n_pairs, scale, float(lr), **kw)
        g, o, t = run()                                                     # both outputs
        assert _same(g, want_g) and _same(o, want_t) and _same(t, th), (name, "both")
        sg_, so_, _ = run(deep=False)                                       # the shallow entry on a layout of the same K
        assert _same(g, sg_) and _same(o, so_), (name, "shallow")
        g, o, _ = run(out=None)
        assert o is None and _same(g, want_g), (name, "grad only")
        g, o, _ = run(grad=False)
        assert g is None and _same(o, want_t), (name, "theta_out only")
        g, o, t = run(out="inplace")
        assert _same(g, want_g) and _same(t, want_t), (name, "in place")
        assert np.isnan(want_g).all() if name == "nan" else np.isfinite(want_g).all()


def _update_diag(K, deep, G, gen, theta, sigma, util, first, n, step, skip=(), inplace=False):
    import torch
    from walker_gym_amd import _lib
    shape, sets = _dummies(K, deep)
    th_d, sg_d, util_d = _dev(theta), _dev(sigma), _dev(util)
    work = torch.full((2, -(-n // 256), K), float("nan"), dtype=torch.float64, device=DEV)
    new = lambda: torch.full((K,), SENTINEL, dtype=torch.float32, device=DEV)
    outs = {o: None if o in skip else new() for o in OUTS}
    if inplace:
        outs["theta_out"], outs["sigma_out"] = th_d, sg_d
    cs = _lib.WgEsDiagStep(**step)
    tail = (_ptr(sg_d), first, n, _ptr(util_d), C.byref(cs), _ptr(work), *[_ptr(outs[o]) for o in OUTS], None)
    if deep:
        es, mid = _structs(shape, G, gen, th_d, sets, sigma=0.0)
        _lib.check(_lib.load().wg_es_update_diag_deep(C.byref(es), C.byref(mid), *tail), "wg_es_update_diag_deep")
    else:
        D, H, Cc, _ = shape
        es = _lib.WgEs(n_sets=G, obs_dim=D, hidden=H, act_dim=Cc, seed=SEED, generation=gen, sigma=0.0,
                       theta=_ptr(th_d), **{k: _ptr(v) for k, v in sets.items()})
        _lib.check(_lib.load().wg_es_update_diag(C.byref(es), *tail), "wg_es_update_diag")
    torch.cuda.synchronize()
    return [outs[o] for o in OUTS], th_d, sg_d


# (65,536 parameters with 3 pairs: 256 workgroups of the one-thread form, which takes it; 65,280: 255, the spread form)
DIAG_CASES = [(K, n) for K in (35, 161) for n in ac.UPDATE_PAIRS] + [(65536, 3), (65280, 3)]


@pytest.mark.parametrize("K,n_pairs", DIAG_CASES, ids=["K%d-n%d" % c for c in DIAG_CASES])
def test_update_diag_equals_numpy_and_the_shallow_entry(K, n_pairs):
    c = ac.update_inputs(K, n_pairs)
    th, sg, G, step = c["theta"], c["sigma"], c["G"], ac.update_step(n_pairs)
    for name in (list(c["utils"]) if K < 32768 else ["plain", "inf_both"]):
        util = c["utils"][name]
        want = ac.update_reference(K, n_pairs, name)
        run = lambda deep=True, **kw: _update_diag(K, deep, G, ac.GEN, th, sg, util, ac.FIRST, n_pairs, step, **kw)
        got, th_d, sg_d = run()
        for o, g, w in zip(OUTS, got, want):
            assert _same_nan(g, w), (name, o)
        assert _same(th_d, th) and _same(sg_d, sg)
        shallow, _, _ = run(deep=False)
        assert all(_same(a, b) for a, b in zip(got, shallow)), (name, "shallow")   # NaN bits included: the same kernels
        if name in ("plain", "inf_both"):
            for skipped in OUTS:
                part, _, _ = run(skip=(skipped,))
                for o, g, w in zip(OUTS, part, want):
                    assert (g is None) if o == skipped else _same_nan(g, w), (name, "without " + skipped, o)
        got, th_d, sg_d = run(inplace=True)
        for o, g, w in zip(OUTS, got, want):
            assert _same_nan(g, w), (name, "in place", o)
        assert _same_nan(th_d, want[1]) and _same_nan(sg_d, want[3]), (name, "in place")


# ------------------------------------------------------------------ the trainers
def _env():
    from walker_gym_amd.batched_env import BatchedPhysicsEnv
    return BatchedPhysicsEnv(ec.balance128(), device=DEV, **dz.PARAMS)


def _trainer(env, G, adaptive, **kw):
    from walker_gym_amd.es import AdaptiveEvolutionStrategy, EvolutionStrategy
    args = dict(hidden=dz.H1, hidden2=dz.H2, act_dim=dz.C, biases=True, population=G, seed=SEED, theta0=dz.theta0())
    if adaptive:
        args.update(sigma=dz.sigma0(), lr=dz.LR_THETA, sigma_lr=dz.SIGMA_LR, sigma_max_change=dz.MAX_CHANGE,
                    sigma_min=dz.SIGMA_MIN, sigma_max=dz.SIGMA_MAX)
    else:
        args.update(sigma=dz.SIGMA, lr=dz.LR)
    args.update(kw)
    return (AdaptiveEvolutionStrategy if adaptive else EvolutionStrategy)(env, **args)


def _sigma0(adaptive):
    return dz.sigma0() if adaptive else f32(dz.SIGMA)


def _tell_and_compare(tr, out, theta, sigma, fit, g, G, adaptive):
    """The numpy update of one generation, compared with what the trainer returned and holds; (theta, sigma) after."""
    res = dz.numpy_tell(theta, sigma, fit, g, G)
    assert _same(out["fitness"], fit), g
    if adaptive:
        g_theta, theta, g_sigma, sigma = res
        assert _same(out["grad"], g_theta) and _same(out["grad_sigma"], g_sigma) and _same(tr.sigma_vec, sigma), g
    else:
        grad, theta = res
        assert _same(out["grad"], grad), g
    assert _same(tr.theta, theta), g
    return theta, sigma


ADAPTIVE = pytest.mark.parametrize("adaptive", [False, True], ids=["es", "pgpe"])


@ADAPTIVE
@pytest.mark.parametrize("G", dz.TRAINER_G)
def test_trainer_equals_its_composition(G, adaptive):
    import torch
    env, ref_env = _env(), _env()
    assert env.obs_dim == dz.D
    tr = _trainer(env, G, adaptive)
    assert (tr.K, tr.H, tr.H2) == (dz.K, dz.H1, dz.H2) and tr.policy.H2 == dz.H2 and tr.policy.G == G
    start = ref_env.batch.state_dict()
    theta, sigma, saved = dz.theta0(), _sigma0(adaptive), None
    for g in range(dz.GENERATIONS):
        out = tr.generation_step(dz.T)
        if g == 0:                                   # the candidates themselves, in the six tensors of the policy
            cand = torch.cat([getattr(tr.policy, n).reshape(G, -1) for n in NAMES], dim=1)
            f = dz.numpy_policy(theta, sigma, g, G)
            assert _same(cand, np.concatenate([_host(getattr(f, n)).reshape(G, -1) for n in NAMES], axis=1))
        ref_env.batch.load_state_dict(start)
        res = ref_env.rollout_policy(dz.numpy_policy(theta, sigma, g, G, device=DEV), dz.T)
        fit = ec.set_fitness(res["returns"].cpu().numpy(), G)
        assert out["generation"] == g and tr.generation == g + 1
        theta, sigma = _tell_and_compare(tr, out, theta, sigma, fit, g, G, adaptive)
        assert np.isfinite(fit).all() and np.isfinite(theta).all()
        if g == 0:
            saved = tr.state_dict()
    # the generations agree with the reference engine's too (tests/test_es_deep_cpu.py keeps them finite)
    last = dz.oracle_training(G, adaptive)[-1]
    assert _same(theta, last["theta"]) and (not adaptive or _same(sigma, last["sigma"]))
    # resumed from the dict taken after the first generation, a fresh trainer arrives at the same theta
    kw = dict(sigma=1.0, lr=0.0, seed=0, theta0=None)
    if adaptive:
        kw.update(sigma_lr=0.5, sigma_max_change=0.5, sigma_min=1e-3, sigma_max=10.0)
    fresh = _trainer(_env(), G, adaptive, **kw)
    fresh.load_state_dict(saved)
    assert fresh.generation == 1
    for g in range(1, dz.GENERATIONS):
        fresh.generation_step(dz.T)
    assert _same(fresh.theta, theta) and (not adaptive or _same(fresh.sigma_vec, sigma))
    # mean_policy: theta as one shared deep parameter set, evaluated by the rollout kernel
    mp = tr.mean_policy()
    assert (mp.G, mp.D, mp.H, mp.H2, mp.C) == (1, dz.D, dz.H1, dz.H2, dz.C)
    assert _same(torch.cat([getattr(mp, n).reshape(-1) for n in NAMES]), theta)
    ref_env.batch.load_state_dict(start)
    rows0 = ref_env.observe()[0].cpu().numpy().copy()
    rows = torch.full((2, dz.N_WALKERS, dz.D), float("nan"), device=DEV)
    acts = torch.full((2, dz.N_WALKERS, dz.C), float("nan"), device=DEV)
    ref_env.rollout_policy(mp, 2, obs_out=rows, action_out=acts)
    host = dz.policy_of_flat(theta)
    assert _same(acts[0], host.forward_numpy(rows0)) and _same(acts[1], host.forward_numpy(rows[0].cpu().numpy()))
    assert len(np.unique(_host(acts))) > 2


@ADAPTIVE
def test_generation_step_with_auto_reset_equals_its_composition(adaptive):
    G = 16
    env, ref_env = _env(), _env()
    for e in (env, ref_env):
        e.enable_auto_reset()
    tr = _trainer(env, G, adaptive)
    start = ref_env.batch.state_dict()
    theta, sigma = dz.theta0(), _sigma0(adaptive)
    for g in range(2):
        out = tr.generation_step(dz.T)
        ref_env.batch.load_state_dict(start)
        res = ref_env.rollout_episodes(dz.numpy_policy(theta, sigma, g, G, device=DEV), dz.T)
        assert int(res["episodes"].sum()) >= dz.N_WALKERS            # max_steps = 16 < T: every walker rolled over
        tot = res["return_sum"].cpu().numpy().astype(np.float64) + res["tail_return"].cpu().numpy().astype(np.float64)
        fit = (tot.reshape(G, -1).sum(axis=1) / (dz.N_WALKERS // G * dz.T)).astype(f32)
        assert np.isfinite(fit).all() and len(np.unique(fit)) > G // 2
        theta, sigma = _tell_and_compare(tr, out, theta, sigma, fit, g, G, adaptive)


@ADAPTIVE
def test_generation_step_with_a_hold_equals_its_composition(adaptive):
    G = 16
    env, ref_env = _env(), _env()
    tr, plain = _trainer(env, G, adaptive), _trainer(_env(), G, adaptive)
    start = ref_env.batch.state_dict()
    theta, sigma = dz.theta0(), _sigma0(adaptive)
    for g in range(2):
        out = tr.generation_step(dz.T, act_every=4)
        ref_env.batch.load_state_dict(start)
        res = ref_env.rollout_held(dz.numpy_policy(theta, sigma, g, G, device=DEV), dz.T, 4)
        fit = ec.set_fitness(res["returns"].cpu().numpy(), G)
        assert np.isfinite(fit).all() and len(np.unique(fit)) > G // 2
        if g == 0:
            assert not _same(plain.generation_step(dz.T)["fitness"], fit)   # (the hold changes the rollouts)
        theta, sigma = _tell_and_compare(tr, out, theta, sigma, fit, g, G, adaptive)


@ADAPTIVE
def test_generation_step_with_obs_norm_and_obs_out_equals_its_composition(adaptive):
    """tests/test_gpu_norm_rows.py's trainer test with the deep policy: the ObsNorm updated from every 64th walker's
    rows between the generations, the rows through generation_step's obs_out."""
    import torch
    from walker_gym_amd.normalize import ObsNorm
    G = 16
    env, ref_env = _env(), _env()
    nm, ref_nm = ObsNorm(dz.D, DEV, clip=5.0), ObsNorm(dz.D, DEV, clip=5.0)
    tr = _trainer(env, G, adaptive, obs_norm=nm)
    assert tr.policy.obs_norm is nm and tr.mean_policy().obs_norm is nm and tr.mean_policy().H2 == dz.H2
    start = ref_env.batch.state_dict()
    theta, sigma = dz.theta0(), _sigma0(adaptive)
    mask = torch.zeros((dz.T, dz.N_WALKERS), dtype=torch.uint8, device=DEV)
    mask[:, ::64] = 1
    rows, ref_rows = (torch.full((dz.T, dz.N_WALKERS, dz.D), float("nan"), device=DEV) for _ in range(2))
    fits = []
    for g in range(2):
        out = tr.generation_step(dz.T, obs_out=rows)
        nm.update(rows, mask)
        ref_env.batch.load_state_dict(start)
        res = ref_env.rollout_policy(dz.numpy_policy(theta, sigma, g, G, device=DEV, obs_norm=ref_nm), dz.T,
                                     obs_out=ref_rows)
        ref_nm.update(ref_rows, mask)
        fit = ec.set_fitness(res["returns"].cpu().numpy(), G)
        assert np.isfinite(fit).all() and len(np.unique(fit)) > G // 2
        assert _same(rows, ref_rows) and _same(nm.state, ref_nm.state) and _same(nm.scale, ref_nm.scale)
        theta, sigma = _tell_and_compare(tr, out, theta, sigma, fit, g, G, adaptive)
        fits.append(fit)
    assert nm.count == 2 * dz.T * 2 and float(nm.mean.abs().max()) > 0
    sd = tr.state_dict()
    assert _same(sd["obs_norm"]["state"], nm.state)


def test_trainer_refusals(monkeypatch):
    import torch
    from walker_gym_amd.es import EvolutionStrategy
    env = _env()
    with pytest.raises(ValueError, match="hidden2"):
        _trainer(env, 16, False, hidden=0)
    with pytest.raises(ValueError, match="hidden2"):
        _trainer(env, 16, False, hidden2=257, theta0=None)
    with pytest.raises(ValueError, match="one hidden layer"):
        EvolutionStrategy(env, hidden=(5, 3))
    with pytest.raises(ValueError, match="theta0"):
        _trainer(env, 16, False, theta0=np.zeros(147, f32))                  # the shallow K of the same widths
    with pytest.raises(ValueError, match="sigma"):
        _trainer(env, 16, True, sigma=np.full(147, 0.001, f32))
    with pytest.raises(ValueError, match="even"):
        _trainer(env, 3, False)
    tr = _trainer(env, 16, True)
    with pytest.raises(ValueError, match="fitness"):
        tr.tell(torch.zeros(15, device=DEV))
    with pytest.raises(ValueError, match="sigma_vec"):
        tr.load_state_dict(dict(tr.state_dict(), sigma_vec=torch.ones(147)))
    with pytest.raises(ValueError, match="theta"):
        _trainer(env, 16, False).load_state_dict(dict(_trainer(env, 16, False).state_dict(), theta=torch.ones(147)))
    assert tr.generation == 0
    # the library's own refusal reaches Python as a ValueError that names the entry
    tr.H2 = 300
    with pytest.raises(ValueError, match="wg_es_perturb_diag_deep.*hidden2"):
        tr.ask()
    tr.H2 = dz.H2
    # the rollout's own refusal: resident batches only (nothing updated)
    before = tr.theta.clone()
    monkeypatch.setenv("WG_LEAN", "0")
    with pytest.raises(ValueError, match="resident"):
        tr.generation_step(dz.T)
    assert tr.generation == 0 and _same(tr.theta, before)


# ------------------------------------------------------------------ the shallow trainers did not move
@ADAPTIVE
@pytest.mark.parametrize("H,G", [(5, 16), (0, 128)])
def test_shallow_trainer_still_equals_its_composition(H, G, adaptive):
    """tests/test_gpu_es.py's / test_gpu_es_adaptive.py's trainer comparison for one generation, candidates included:
    the four existing entries behind a trainer without hidden2."""
    import torch
    from walker_gym_amd.es import AdaptiveEvolutionStrategy, EvolutionStrategy
    env, ref_env = _env(), _env()
    args = dict(hidden=H, act_dim=ec.C, biases=True, population=G, seed=SEED, theta0=ec.theta0(H))
    if adaptive:
        tr = AdaptiveEvolutionStrategy(env, sigma=ac.sigma0(H), lr=ac.LR_THETA[H], sigma_lr=ac.SIGMA_LR,
                                       sigma_max_change=ac.MAX_CHANGE, sigma_min=ac.SIGMA_MIN, sigma_max=ac.SIGMA_MAX, **args)
    else:
        tr = EvolutionStrategy(env, sigma=ec.SIGMA[H], lr=ec.LR[H], **args)
    assert tr.H2 == 0 and tr.policy.H2 == 0
    theta = ec.theta0(H)
    out = tr.generation_step(ec.T)
    pol = (ac.numpy_policy(theta, ac.sigma0(H), 0, H, G, device=DEV) if adaptive
           else ec.numpy_policy(theta, f32(ec.SIGMA[H]), 0, H, G, device=DEV))
    for n in ("w1", "b1", "w2", "b2"):
        a, b = getattr(tr.policy, n), getattr(pol, n)
        assert (a is None and b is None) or _same(a, b), n
    fit = ec.set_fitness(ref_env.rollout_policy(pol, ec.T)["returns"].cpu().numpy(), G)
    assert _same(out["fitness"], fit)
    if adaptive:
        g_theta, theta, g_sigma, sigma = ac.numpy_tell(theta, ac.sigma0(H), fit, 0, H, G)
        assert _same(out["grad"], g_theta) and _same(out["grad_sigma"], g_sigma) and _same(tr.sigma_vec, sigma)
    else:
        grad, theta = ec.numpy_tell(theta, fit, 0, H, G)
        assert _same(out["grad"], grad)
    assert _same(tr.theta, theta)

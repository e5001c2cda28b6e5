"""Evolution strategies over a deep policy without a GPU: the six-segment theta (param_count / split_theta /
theta_from_policy) against a scalar restatement and against pg.policy_grad_numpy's segment order, the constructors'
refusals, every WG_EINVAL of the four wg_es_*_deep entries refused before a launch and in the contract's order, wg_es_mid's
layout, and (on the reference engine) the conditions that the trainer cases of tests/test_gpu_es_deep.py rest on."""
import ctypes as C
import os
import subprocess
import types

import numpy as np
import pytest

import deep_cases as dc
import es_deep_cases as dz
from walker_gym_amd import _lib, build, es

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


# ------------------------------------------------------------------ the six segments
def _scalar_layout(D, H1, H2, Cc, b1, bm, b2):
    """theta's index of every parameter, one at a time: {(segment, i, j): k}."""
    k, where = 0, {}
    for i in range(D):
        for h in range(H1):
            where["w1", i, h] = k; k += 1
    for h in range(H1 if b1 else 0):
        where["b1", h, 0] = k; k += 1
    for j in range(H1):
        for m in range(H2):
            where["wm", j, m] = k; k += 1
    for m in range(H2 if bm else 0):
        where["bm", m, 0] = k; k += 1
    for m in range(H2):
        for c in range(Cc):
            where["w2", m, c] = k; k += 1
    for c in range(Cc if b2 else 0):
        where["b2", c, 0] = k; k += 1
    return where, k


@pytest.mark.parametrize("shape", [s for s in dz.SHAPES if len(set(s[4:])) == 1], ids=dz.shape_id)
def test_param_count_and_split_theta_against_a_scalar_restatement(shape):
    D, H1, H2, Cc, b1, _, _ = shape
    where, K = _scalar_layout(*shape)
    assert es.param_count(D, H1, Cc, b1, H2) == K == dz.K_of(shape)
    flat = np.arange(K, dtype=f32)
    seg = es.split_theta(flat, D, H1, Cc, b1, H2)
    assert list(seg) == ["w1", "b1", "wm", "bm", "w2", "b2"]
    for (name, i, j), k in where.items():
        a = seg[name]
        assert (a[i, j] if a.ndim == 2 else a[i]) == k, (name, i, j)
    assert all((seg[n] is None) == (not b1) for n in ("b1", "bm", "b2"))
    lead = es.split_theta(np.zeros((3, 2, K), f32), D, H1, Cc, b1, H2)          # leading axes are kept
    assert lead["wm"].shape == (3, 2, H1, H2) and lead["w2"].shape == (3, 2, H2, Cc)
    with pytest.raises(ValueError):
        es.split_theta(np.zeros(K + 1, f32), D, H1, Cc, b1, H2)


def test_shallow_calls_are_unchanged():
    assert es.param_count(26, 0, 2, True) == 54 and es.param_count(26, 5, 2, True) == 147
    assert es.param_count(26, 5, 2, True, 0) == 147 and es.param_count(152, 24, 5, False, H2=0) == 152 * 24 + 24 * 5
    seg = es.split_theta(np.arange(147, dtype=f32), 26, 5, 2, True)
    assert list(seg) == ["w1", "b1", "w2", "b2"]                                 # no 'wm' / 'bm' keys without H2
    assert seg["w1"][1, 0] == 5 and seg["b1"][0] == 130 and seg["w2"][1, 0] == 137 and seg["b2"][1] == 146
    with pytest.raises(ValueError):
        es.param_count(26, 0, 2, True, 3)
    with pytest.raises(ValueError):
        es.split_theta(np.zeros(10, f32), 26, 0, 2, True, 3)


def _deep_policy(D, H1, H2, Cc, G, biases=(True, True, True), seed=0):
    import torch
    from walker_gym_amd.policy import MLPPolicy
    rng = np.random.default_rng(seed)
    t = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(f32))
    return MLPPolicy(t(G, H2, Cc), t(G, Cc) if biases[2] else None, t(G, D, H1), t(G, H1) if biases[0] else None,
                     act_limit=1.0, wm=t(G, H1, H2), bm=t(G, H2) if biases[1] else None)


def test_theta_order_is_the_deep_gradients_order():
    """A flat gradient from pg and an ES theta of the same policy index the same parameters: the six arrays of
    policy_grad_numpy, raveled and concatenated in the order it returns them, split back by split_theta into views of
    exactly those arrays (every segment has its own size here, so a swapped pair cannot pass)."""
    from walker_gym_amd import pg
    D, H1, H2, Cc, G = 3, 4, 5, 2, 1
    pol = _deep_policy(D, H1, H2, Cc, G)
    rng = np.random.default_rng(1)
    x, dy = rng.standard_normal((2, 4, D)).astype(f32), rng.standard_normal((2, 4, Cc)).astype(f32)
    grads = pg.policy_grad_numpy(pol, x, dy)
    assert len(grads) == 6 and len({g.size for g in grads}) == 6
    flat = np.concatenate([g[0].reshape(-1) for g in grads])
    seg = es.split_theta(flat, D, H1, Cc, True, H2)
    for name, g in zip(("w1", "b1", "wm", "bm", "w2", "b2"), grads):
        assert seg[name].shape == g[0].shape and np.array_equal(seg[name], g[0]) and np.abs(g).max() > 0, name
    assert np.array_equal(es.theta_from_policy(pol),
                          np.concatenate([t[0].numpy().reshape(-1) for t in (pol.w1, pol.b1, pol.wm, pol.bm, pol.w2, pol.b2)]))


def _fake_env(N=16, D=7, A=2):
    """What a trainer's constructor and mean_policy() touch, on the host (no library call, no device)."""
    import torch
    return types.SimpleNamespace(N=N, obs_dim=D, device=torch.device("cpu"),
                                 batch=types.SimpleNamespace(A=A, state_dict=lambda: {}))


@pytest.mark.parametrize("cls", ["EvolutionStrategy", "AdaptiveEvolutionStrategy"])
@pytest.mark.parametrize("biases", [True, False])
def test_theta_from_policy_round_trip(cls, biases):
    D, H1, H2, Cc = 7, 4, 3, 2
    pol = _deep_policy(D, H1, H2, Cc, 3, (biases,) * 3, seed=2)
    theta = es.theta_from_policy(pol, set_index=2)
    assert theta.dtype == f32 and theta.shape == (es.param_count(D, H1, Cc, biases, H2),)
    seg = es.split_theta(theta, D, H1, Cc, biases, H2)
    for name in ("w1", "b1", "wm", "bm", "w2", "b2"):
        t = getattr(pol, name)
        assert (seg[name] is None) if t is None else np.array_equal(seg[name], t[2].numpy()), name
    tr = getattr(es, cls)(_fake_env(D=D), hidden=H1, hidden2=H2, biases=biases, population=4, theta0=theta)
    assert (tr.K, tr.H, tr.H2) == (theta.size, H1, H2)
    assert tr.policy.H2 == H2 and tuple(tr.policy.wm.shape) == (4, H1, H2) and (tr.policy.bm is None) == (not biases)
    mp = tr.mean_policy()
    assert (mp.G, mp.D, mp.H, mp.H2, mp.C) == (1, D, H1, H2, Cc)
    assert np.array_equal(es.theta_from_policy(mp), theta)
    rows = np.random.default_rng(3).standard_normal((5, D)).astype(f32)
    assert np.array_equal(mp.forward_numpy(rows), pol.forward_numpy(rows, first_walker=10, n_walkers_total=15))
    sd = tr.state_dict()                                               # round trip; a wrong K is refused
    other = getattr(es, cls)(_fake_env(D=D), hidden=H1, hidden2=H2, biases=biases, population=4)
    other.load_state_dict(sd)
    assert np.array_equal(other.theta.numpy(), theta)
    shallow = getattr(es, cls)(_fake_env(D=D), hidden=H1, biases=biases, population=4)
    with pytest.raises(ValueError, match="sigma_vec" if cls.startswith("Adaptive") else "theta"):
        shallow.load_state_dict(sd)
    # a shallow policy comes back too
    sp = shallow.mean_policy()
    assert sp.H2 == 0 and es.theta_from_policy(sp).shape == (shallow.K,)


def test_theta_from_policy_refusals():
    pol = _deep_policy(7, 4, 3, 2, 2, (True, False, True))
    with pytest.raises(ValueError, match="biases"):
        es.theta_from_policy(pol)
    with pytest.raises(ValueError, match="set_index"):
        es.theta_from_policy(_deep_policy(7, 4, 3, 2, 2), 2)


@pytest.mark.parametrize("cls", ["EvolutionStrategy", "AdaptiveEvolutionStrategy"])
def test_constructor_refusals(cls):
    T = getattr(es, cls)
    env = _fake_env()
    with pytest.raises(ValueError, match="hidden2"):
        T(env, hidden=0, hidden2=3, population=4)
    with pytest.raises(ValueError, match="hidden2"):
        T(env, hidden=5, hidden2=257, population=4)
    with pytest.raises(ValueError, match="hidden2"):
        T(env, hidden=5, hidden2=-1, population=4)
    with pytest.raises(ValueError, match="one hidden layer"):             # the existing refusal, still in force
        T(None, hidden=(64, 64))
    with pytest.raises(ValueError, match="theta0"):
        T(env, hidden=5, hidden2=3, population=4, theta0=np.zeros(es.param_count(7, 5, 2, True), f32))   # the shallow K
    if cls == "AdaptiveEvolutionStrategy":
        with pytest.raises(ValueError, match="sigma"):
            T(env, hidden=5, hidden2=3, population=4, sigma=np.full(es.param_count(7, 5, 2, True), 0.1, f32))
        tr = T(env, hidden=5, hidden2=3, population=4)
        with pytest.raises(ValueError, match="sigma_vec"):
            tr.load_state_dict(dict(tr.state_dict(), sigma_vec=np.ones(tr.K - 1, f32)))
    tr = T(env, hidden=5, hidden2=256, population=4)                        # the widest is taken
    assert tr.K == es.param_count(7, 5, 2, True, 256)


# ------------------------------------------------------------------ the C boundary
@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


NEW = ("wg_es_perturb_deep", "wg_es_update_deep", "wg_es_perturb_diag_deep", "wg_es_update_diag_deep")


def test_wg_es_mid_matches_header_and_abi_stays_16(lib, tmp_path):
    fields = [f for f, _ in _lib.WgEsMid._fields_]
    lines = "".join(f'  printf("{f} %zu\\n", offsetof(wg_es_mid, {f}));\n' for f in fields)
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "walker_hip.h"\nint main(void) {\n' + lines +
                     '  printf("sizeof %zu\\n", sizeof(wg_es_mid));\n  printf("es %zu\\n", sizeof(wg_es));\n  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(probe)], check=True)
    got = dict(line.rsplit(" ", 1) for line in
               subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().splitlines())
    assert int(got["sizeof"]) == C.sizeof(_lib.WgEsMid)
    for f in fields:
        assert getattr(_lib.WgEsMid, f).offset == int(got[f]), f
    assert int(got["es"]) == C.sizeof(_lib.WgEs)                        # wg_es itself did not move
    assert _lib.ABI_VERSION == 16 and lib.wg_abi_version() == 16
    assert set(NEW) <= set(_lib.EXPORTS)
    for sym in NEW:
        assert getattr(lib, sym).restype is C.c_int


def _es(**kw):
    """A 26 -> 5 -> (3) -> 2 policy of 8 sets whose pointers are non-NULL fakes: every call below is refused before
    anything dereferences them."""
    d = dict(n_sets=8, obs_dim=26, hidden=5, act_dim=2, seed=1, generation=0, sigma=0.05, theta=64, w1=64, w2=64, b2=64)
    d.update(kw)
    return _lib.WgEs(**d)


def _mid(**kw):
    d = dict(hidden2=3, wm=64)
    d.update(kw)
    return _lib.WgEsMid(**d)


_STEP = dict(base=0.0, scale_theta=1.0, scale_sigma=1.0, lr_theta=0.1, lr_sigma=0.1, shrink=0.8, grow=1.2, sigma_min=1e-8,
             sigma_max=float("inf"))


def _call(lib, entry, e, m, first=0, n=4, sigma=64, util=64, scale=1.0, lr=0.1, work=64, outs=(64, 64, 64, 64),
          step=_STEP):
    """One of the four entries on (es, mid) with fake device pointers."""
    e = None if e is None else C.byref(e)
    m = None if m is None else C.byref(m)
    if entry == "wg_es_perturb_deep":
        return lib.wg_es_perturb_deep(e, m, first, n, None)
    if entry == "wg_es_update_deep":
        return lib.wg_es_update_deep(e, m, first, n, util, scale, lr, work, outs[0], outs[1], None)
    if entry == "wg_es_perturb_diag_deep":
        return lib.wg_es_perturb_diag_deep(e, m, sigma, first, n, None)
    st = None if step is None else _lib.WgEsDiagStep(**step)
    return lib.wg_es_update_diag_deep(e, m, sigma, first, n, util, None if st is None else C.byref(st), work, *outs, None)


# (what, wg_es fields or None for a NULL es, wg_es_mid fields or None for a NULL mid, pair range, a word of the message)
REFUSED = [
    # the shallow entries' list, in front
    ("null es", None, {}, {}, b"null es"),
    ("null theta", dict(theta=None), {}, {}, b"theta"),
    ("null w2", dict(w2=None), {}, {}, b"w2"),
    ("hidden < 0", dict(hidden=-1), {}, {}, b"hidden -1"),
    ("hidden > 256", dict(hidden=257), {}, {}, b"hidden 257"),
    ("hidden without w1", dict(w1=None), {}, {}, b"w1"),
    ("b1 without hidden", dict(hidden=0, w1=None, b1=64), {}, {}, b"b1"),
    ("n_sets odd", dict(n_sets=7), {}, {}, b"n_sets"),
    ("n_sets 0", dict(n_sets=0), {}, {}, b"n_sets"),
    ("first_pair < 0", {}, {}, dict(first=-1), b"pairs"),
    ("range past the end", {}, {}, dict(first=3, n=2), b"pairs"),
    ("n_pairs 0", {}, {}, dict(n=0), b"n_pairs"),
    ("obs_dim 0", dict(obs_dim=0), {}, {}, b"obs_dim"),
    ("act_dim 0", dict(act_dim=0), {}, {}, b"act_dim"),
    # the new ones
    ("null mid", {}, None, {}, b"null mid"),
    ("hidden2 0", {}, dict(hidden2=0), {}, b"hidden2"),
    ("hidden2 < 0", {}, dict(hidden2=-4), {}, b"hidden2"),
    ("hidden2 > 256", {}, dict(hidden2=257), {}, b"hidden2"),
    ("no first hidden layer", dict(hidden=0, w1=None), {}, {}, b"first hidden layer"),
    ("null wm", {}, dict(wm=None), {}, b"wm"),
    ("more than 2^23 parameters", dict(obs_dim=32600, hidden=256), dict(hidden2=256), {}, b"parameters"),
    # the order: an earlier refusal wins over a later one
    ("null theta before null mid", dict(theta=None), None, {}, b"theta"),
    ("pairs before null mid", {}, None, dict(first=3, n=2), b"pairs"),
    ("null mid before hidden 0", dict(hidden=0, w1=None), None, {}, b"null mid"),
    ("hidden2 before hidden 0", dict(hidden=0, w1=None), dict(hidden2=0), {}, b"hidden2"),
    ("hidden 0 before null wm", dict(hidden=0, w1=None), dict(wm=None), {}, b"first hidden layer"),
    ("null wm before the count", dict(obs_dim=32600, hidden=256), dict(hidden2=256, wm=None), {}, b"wm"),
]


@pytest.mark.parametrize("entry", NEW)
@pytest.mark.parametrize("what,fields,mid,rng,word", REFUSED, ids=[r[0] for r in REFUSED])
def test_every_einval_is_refused_before_a_launch(lib, entry, what, fields, mid, rng, word):
    e = None if fields is None else _es(**fields)
    m = None if mid is None else _mid(**mid)
    assert _call(lib, entry, e, m, **rng) == _lib.WG_EINVAL, what
    err = lib.wg_last_error()
    assert word in err and entry.encode() + b":" in err, err


@pytest.mark.parametrize("entry", ["wg_es_perturb_deep", "wg_es_update_deep"])
def test_scalar_sigma_is_checked_by_the_scalar_entries_only(lib, entry):
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        assert _call(lib, entry, _es(sigma=bad), _mid()) == _lib.WG_EINVAL
        assert b"sigma" in lib.wg_last_error()
    assert _call(lib, entry, _es(sigma=0.0), None) == _lib.WG_EINVAL and b"sigma" in lib.wg_last_error()   # before mid
    # the _diag entries do not read es->sigma: with it 0 they go on to their next refusal
    assert _call(lib, "wg_es_perturb_diag_deep", _es(sigma=0.0), _mid(), sigma=None) == _lib.WG_EINVAL
    assert b"sigma vector" in lib.wg_last_error()
    assert _call(lib, "wg_es_update_diag_deep", _es(sigma=0.0), _mid(), util=None) == _lib.WG_EINVAL
    assert b"util" in lib.wg_last_error()


def test_the_parameter_count_includes_the_middle_segments(lib):
    """32,600 x 256 is 8,345,600 parameters of w1.  With w2 (and a narrow wm) theta stays under 2^23 and
    the call goes on to its next refusal; with wm [256, 256] it passes 2^23 and that is refused first."""
    big = dict(obs_dim=32600, hidden=256)
    assert 32600 * 256 + 256 * 1 + 1 * 2 + 2 <= 1 << 23 < 32600 * 256 + 256 * 256 + 256 * 2 + 2
    for entry, kw, word in (("wg_es_update_deep", dict(util=None), b"util"),
                            ("wg_es_perturb_diag_deep", dict(sigma=None), b"sigma vector"),
                            ("wg_es_update_diag_deep", dict(sigma=None), b"sigma vector")):
        assert _call(lib, entry, _es(**big), _mid(hidden2=1), **kw) == _lib.WG_EINVAL
        assert word in lib.wg_last_error(), lib.wg_last_error()
        assert _call(lib, entry, _es(**big), _mid(hidden2=256), **kw) == _lib.WG_EINVAL
        assert b"parameters" in lib.wg_last_error(), lib.wg_last_error()
    # 2^23 exactly is taken; bm counts: its two elements on top are refused (32,765 x 256 + 256 x 2 + 2 x 128 = 2^23)
    edge = dict(obs_dim=32765, hidden=256, act_dim=128, b2=None)
    assert 32765 * 256 + 256 * 2 + 2 * 128 == 1 << 23
    assert _call(lib, "wg_es_update_deep", _es(**edge), _mid(hidden2=2), util=None) == _lib.WG_EINVAL
    assert b"util" in lib.wg_last_error(), lib.wg_last_error()
    assert _call(lib, "wg_es_update_deep", _es(**edge), _mid(hidden2=2, bm=64), util=None) == _lib.WG_EINVAL
    assert b"parameters" in lib.wg_last_error(), lib.wg_last_error()


UPDATE_ONLY = [
    ("null util", dict(util=None), b"util"),
    ("null workspace", dict(work=None), b"workspace"),
    ("scale inf", dict(scale=float("inf")), b"scale"),
    ("lr nan", dict(lr=float("nan")), b"lr"),
    ("no output", dict(outs=(None, None, None, None)), b"both null"),
]
DIAG_ONLY = [
    ("null sigma vector", dict(sigma=None), b"sigma vector"),
    ("null util", dict(util=None), b"util"),
    ("null step", dict(step=None), b"step"),
    ("null workspace", dict(work=None), b"workspace"),
    ("base nan", dict(step=dict(_STEP, base=float("nan"))), b"base"),
    ("shrink 0", dict(step=dict(_STEP, shrink=0.0)), b"shrink"),
    ("grow < 1", dict(step=dict(_STEP, grow=0.5)), b"grow"),
    ("sigma_min 0", dict(step=dict(_STEP, sigma_min=0.0)), b"sigma_min"),
    ("sigma_max below", dict(step=dict(_STEP, sigma_max=1e-9)), b"sigma_max"),
    ("no output", dict(outs=(None, None, None, None)), b"all four"),
]


@pytest.mark.parametrize("what,kw,word", UPDATE_ONLY, ids=[r[0] for r in UPDATE_ONLY])
def test_update_deep_einval(lib, what, kw, word):
    assert _call(lib, "wg_es_update_deep", _es(), _mid(), **kw) == _lib.WG_EINVAL, what
    assert word in lib.wg_last_error() and b"wg_es_update_deep" in lib.wg_last_error(), lib.wg_last_error()


@pytest.mark.parametrize("what,kw,word", DIAG_ONLY, ids=[r[0] for r in DIAG_ONLY])
def test_update_diag_deep_einval(lib, what, kw, word):
    assert _call(lib, "wg_es_update_diag_deep", _es(), _mid(), **kw) == _lib.WG_EINVAL, what
    assert word in lib.wg_last_error() and b"wg_es_update_diag_deep" in lib.wg_last_error(), lib.wg_last_error()


# ------------------------------------------------------------------ what the GPU trainer cases rest on
def test_start_weights_are_balanced_in_both_layers():
    """Under the mean theta every unit of both hidden layers is on for some walker and off for another at step 0."""
    seg = es.split_theta(dz.theta0()[None], dz.D, dz.H1, dz.C, True, dz.H2)
    h1, h2 = dc.hidden_of(seg, dz.entry_rows(), 1)
    assert h1.shape == (dz.N_WALKERS, dz.H1) and h2.shape == (dz.N_WALKERS, dz.H2)
    for h in (h1, h2):
        assert ((h > 0).any(axis=0) & (h == 0).any(axis=0)).all()
    assert es.param_count(dz.D, dz.H1, dz.C, True, dz.H2) == dz.K == dz.theta0().size


@pytest.mark.parametrize("adaptive", [False, True], ids=["es", "pgpe"])
@pytest.mark.parametrize("G", dz.TRAINER_G)
def test_trainer_cases_hold_their_conditions(G, adaptive):
    """Every generation that tests/test_gpu_es_deep.py compares bit for bit: every walker finite, the clip engaged on
    some actions and not on all, units on and off in both hidden layers at step 0 over the generation's candidates, at
    least G / 2 distinct fitness values, and a theta (and sigma) that moves."""
    gens = dz.oracle_training(G, adaptive)
    assert len(gens) == dz.GENERATIONS == 3
    prev, sig = dz.theta0(), (dz.sigma0() if adaptive else f32(dz.SIGMA))
    for i, g in enumerate(gens):
        assert np.isfinite(g["obs"]).all() and np.isfinite(g["reward"]).all() and np.isfinite(g["action"]).all()
        assert g["nonfinite"] == 0
        hit = np.abs(g["action"]) == f32(1.0)
        assert hit.any() and not hit.all()
        f = (es.es_perturb_diag_numpy if adaptive else es.es_perturb_numpy)(prev, sig, dz.SEED, i, 0, G // 2)
        h1, h2 = dc.hidden_of(es.split_theta(f, dz.D, dz.H1, dz.C, True, dz.H2), dz.entry_rows(), G)
        for h in (h1, h2):
            assert (h > 0).any() and (h == 0).any()
        assert np.isfinite(g["fitness"]).all() and len(np.unique(g["fitness"])) >= G // 2
        assert np.isfinite(g["grad"]).all() and np.isfinite(g["theta"]).all() and (g["sigma"] > 0).all()
        assert not np.array_equal(g["theta"], prev)
        prev, sig = g["theta"], (g["sigma"] if adaptive else sig)
    if adaptive:
        assert not np.array_equal(gens[-1]["sigma"], dz.sigma0())

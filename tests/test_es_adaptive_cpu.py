"""Adaptive evolution strategies (wg_es_perturb_diag / wg_es_update_diag, AdaptiveEvolutionStrategy) without a GPU:
the numpy restatements against a scalar loop, constant sigma against es_perturb_numpy, every clamp branch, the estimates
against plain float64 sums, the quadratic on the restatement alone, every WG_EINVAL refused before a launch,
wg_es_diag_step's layout, and the conditions (on the reference engine) of the trainer cases whose bits
tests/test_gpu_es_adaptive.py compares."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import es_adaptive_cases as ac
import es_cases as ec
from walker_gym_amd import _lib, build, es

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
SEED = ac.SEED


# ------------------------------------------------------------------ a scalar restatement
def _perturb_scalar(theta, sigma, eps):
    n, K = eps.shape
    out = np.zeros((2 * n, K), f32)
    for i in range(n):
        for k in range(K):
            d = f32(sigma[k] * eps[i, k])
            out[2 * i, k] = f32(theta[k] + d)
            out[2 * i + 1, k] = f32(theta[k] - d)
    return out


def _update_scalar(theta, sigma, util, eps, first, step):
    """The header's steps 1 to 5 one scalar at a time: np.float32 scalars round every float32 operation, Python floats
    are IEEE doubles and round every float64 operation once."""
    n, K = eps.shape
    half, base = f32(0.5), f32(step["base"])
    lr_t, lr_s, shrink, grow = (f32(step[x]) for x in ("lr_theta", "lr_sigma", "shrink", "grow"))
    smin, smax = f32(step["sigma_min"]), f32(step["sigma_max"])
    out = [np.zeros(K, f32) for _ in range(4)]
    with np.errstate(all="ignore"):
        dm = [float(f32(util[2 * (first + i)] - util[2 * (first + i) + 1])) for i in range(n)]
        ds = [float(f32(f32(f32(util[2 * (first + i)] + util[2 * (first + i) + 1]) * half) - base)) for i in range(n)]
        for k in range(K):
            sg = sigma[k]
            ss = float(sg) * float(sg)
            Sm = Ss = 0.0
            for a in range(0, n, 256):
                Pm = Ps = 0.0
                for i in range(a, min(a + 256, n)):
                    d = float(f32(sg * eps[i, k]))
                    Pm = Pm + dm[i] * d
                    Ps = Ps + ds[i] * (d * d - ss)
                Sm, Ss = Sm + Pm, Ss + Ps
            gt = f32(Sm * step["scale_theta"])
            gs = f32(np.float64(Ss * step["scale_sigma"]) / np.float64(sg))    # numpy: x / 0 is inf or NaN, no exception
            s = f32(sg + f32(lr_s * gs))
            dn, up = f32(sg * shrink), f32(sg * grow)
            lo, hi = (dn if dn > smin else smin), (up if up < smax else smax)
            out[0][k], out[1][k], out[2][k] = gt, f32(theta[k] + f32(lr_t * gt)), gs
            out[3][k] = lo if s < lo else (hi if s > hi else s)
    return out


@pytest.mark.parametrize("n_pairs", ac.UPDATE_PAIRS)
@pytest.mark.parametrize("K", [54, 147])
def test_numpy_restatements_equal_scalar_loop(K, n_pairs):
    c = ac.update_inputs(K, n_pairs)
    theta, sigma = c["theta"], c["sigma"]
    assert sigma.max() / sigma.min() > 1e3 and (sigma > 0).all()          # spans more than three of the four decades
    eps = es.es_noise_numpy(SEED, ac.GEN, ac.FIRST, n_pairs, K)
    got = es.es_perturb_diag_numpy(theta, sigma, SEED, ac.GEN, ac.FIRST, n_pairs)
    assert got.dtype == f32 and ac.same_bits_nan_equal(got, _perturb_scalar(theta, sigma, eps))
    step = ac.update_step(n_pairs)
    for name, util in c["utils"].items():
        got = ac.update_reference(K, n_pairs, name)
        want = _update_scalar(theta, sigma, util, eps, ac.FIRST, step)
        for what, g, w in zip(("g_theta", "theta_out", "g_sigma", "sigma_out"), got, want):
            assert g.dtype == f32 and g.shape == (K,)
            assert ac.same_bits_nan_equal(g, w), (name, what)
        if name in ("plain", "ties"):
            assert all(np.isfinite(g).all() for g in got), name
    # what the two inf cases are there for: dm = ds = +inf reaches every parameter as an infinity, dm = NaN as a NaN in
    # the mean's outputs and an infinity in sigma's, and the clamp returns a bound for an infinite step
    g_t, t_o, g_s, s_o = ac.update_reference(K, n_pairs, "inf_one")
    assert np.isinf(g_t).sum() >= K - 1 and np.isinf(g_s).sum() >= K - 1 and np.isfinite(s_o).all()
    g_t, t_o, g_s, s_o = ac.update_reference(K, n_pairs, "inf_both")
    assert np.isnan(g_t).all() and np.isnan(t_o).all() and np.isinf(g_s).sum() >= K - 1 and np.isfinite(s_o).all()
    if n_pairs >= 256:      # the ties include pairs whose two utilities are equal: dm = 0
        assert (c["utils"]["ties"][0::2] == c["utils"]["ties"][1::2])[ac.FIRST:].any()


@pytest.mark.parametrize("K", [54, 147])
def test_constant_sigma_equals_the_scalar_perturbation(K):
    theta = ac.update_inputs(K, 3)["theta"]
    for s in (f32(0.05), f32(1.0), f32(3e-4)):
        a = es.es_perturb_diag_numpy(theta, np.full(K, s, f32), SEED, 5, 2, 7)
        b = es.es_perturb_numpy(theta, s, SEED, 5, 2, 7)
        assert a.dtype == b.dtype and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    with pytest.raises(ValueError):
        es.es_perturb_diag_numpy(theta, np.ones(K + 1, f32), SEED, 0, 0, 1)


# ------------------------------------------------------------------ the clamp
def _shares(name):
    step, (g_t, t_o, g_s, s_o) = ac.clamp_reference(name)
    sigma = ac.update_inputs(ac.CLAMP_K, ac.CLAMP_PAIRS)["sigma"]
    br = ac.clamp_branches(sigma, g_s, step)
    share = {b: float((br == b).mean()) for b in ("shrink", "grow", "sigma_min", "sigma_max", "free")}
    print(name, share)
    # every branch returns what the contract says it returns
    s = sigma + f32(step["lr_sigma"]) * g_s
    want = {"shrink": sigma * f32(step["shrink"]), "grow": sigma * f32(step["grow"]),
            "sigma_min": np.full_like(sigma, step["sigma_min"]), "sigma_max": np.full_like(sigma, step["sigma_max"]),
            "free": s}
    for b, w in want.items():
        assert np.array_equal(s_o[br == b], w[br == b]), (name, b)
    return share


def test_clamp_change_branches():
    """A step far above the allowed change: sigma * shrink binds on some parameters, sigma * grow on others, and a few
    steps stay inside; each of the three on 5 % to 95 % of the parameters."""
    share = _shares("change")
    assert all(0.05 <= share[b] <= 0.95 for b in ("shrink", "grow", "free")), share
    assert share["sigma_min"] == 0 and share["sigma_max"] == 0


def test_clamp_bound_branches():
    """sigma_min and sigma_max inside the range the steps reach: each binds on 5 % to 95 % of the parameters (and the
    change bounds on the parameters far from both)."""
    share = _shares("bounds")
    assert all(0.05 <= share[b] <= 0.95 for b in ("sigma_min", "sigma_max", "shrink", "grow")), share


def test_a_nan_step_passes_the_clamp():
    theta, sigma = np.zeros(3, f32), np.array([1.0, np.nan, 2.0], f32)
    util = np.array([0.5, -0.5, 0.25, -0.25], f32)
    g_t, t_o, g_s, s_o = es.es_update_diag_numpy(theta, sigma, util, SEED, 0, 0, 2, ac.update_step(2))
    assert np.isnan(s_o[1]) and np.isnan(g_s[1]) and np.isfinite(s_o[[0, 2]]).all()


# ------------------------------------------------------------------ the estimates against plain float64 sums
@pytest.mark.parametrize("K,n_pairs", [(54, 3), (147, 600)])
def test_estimates_equal_plain_float64_sums(K, n_pairs):
    """Small-integer utilities and power-of-two sigmas: every product and every partial sum of the contract is exact in
    float64 (or within an ulp of it, in ds * q), so the order of the additions does not matter and the only difference
    from a plain float64 evaluation of the PGPE sums is the rounding of the two outputs to float32, 2^-24 relative: the
    tolerance, 1e-6 relative, is that rounding with room for the last float64 bits."""
    rng = np.random.default_rng(K)
    G = 2 * (ac.FIRST + n_pairs)
    util = rng.integers(-4, 5, G).astype(f32)
    sigma = (2.0 ** rng.integers(-10, 4, K)).astype(f32)
    theta = np.zeros(K, f32)
    step = es.diag_step(base=1.0, scale_theta=1.0 / (2 * n_pairs), scale_sigma=1.0 / n_pairs)
    g_t, _, g_s, s_o = es.es_update_diag_numpy(theta, sigma, util, SEED, 1, ac.FIRST, n_pairs, step)
    d = sigma.astype(np.float64)[None] * es.es_noise_numpy(SEED, 1, ac.FIRST, n_pairs, K).astype(np.float64)
    u = util.astype(np.float64)[2 * ac.FIRST:].reshape(n_pairs, 2)
    want_t = (u[:, 0] - u[:, 1]) @ d / (2 * n_pairs)
    want_s = ((u[:, 0] + u[:, 1]) / 2 - 1.0) @ (d * d - sigma.astype(np.float64)[None] ** 2) / n_pairs / sigma
    np.testing.assert_allclose(g_t, want_t, rtol=1e-6, atol=0)
    np.testing.assert_allclose(g_s, want_s, rtol=1e-6, atol=0)
    assert np.array_equal(s_o, sigma)                    # lr_sigma = 0: sigma unchanged


# ------------------------------------------------------------------ sign and scaling, end to end
@pytest.mark.parametrize("seed", ac.QUAD_SEEDS)
def test_quadratic_descends_and_sigma_shrinks(seed):
    target, theta, sigma, loss0, loss = ac.quadratic_numpy(seed)
    print("seed", seed, "loss ratio", loss / loss0, "mean sigma", float(sigma.mean()))
    assert loss < 0.1 * loss0
    assert float(sigma.astype(np.float64).mean()) < ac.QUAD["sigma"] and (sigma > 0).all()


# ------------------------------------------------------------------ the C boundary
@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def test_diag_step_matches_header_and_abi_stays_16(lib, tmp_path):
    fields = [f for f, _ in _lib.WgEsDiagStep._fields_]
    assert set(fields) == {"base", "scale_theta", "scale_sigma", "lr_theta", "lr_sigma", "shrink", "grow", "sigma_min",
                           "sigma_max"}
    lines = "".join(f'  printf("{f} %zu %zu\\n", offsetof(wg_es_diag_step, {f}), sizeof(((wg_es_diag_step *)0)->{f}));\n'
                    for f in fields)
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "walker_hip.h"\nint main(void) {\n' + lines +
                     '  printf("sizeof %zu %zu\\n", sizeof(wg_es_diag_step), sizeof(wg_es));\n  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(probe)], check=True)
    got = {ln.split()[0]: [int(x) for x in ln.split()[1:]] for ln in
           subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().splitlines()}
    assert got["sizeof"] == [C.sizeof(_lib.WgEsDiagStep), C.sizeof(_lib.WgEs)]
    for f in fields:
        assert [getattr(_lib.WgEsDiagStep, f).offset, getattr(_lib.WgEsDiagStep, f).size] == got[f], f
    assert _lib.ABI_VERSION == 16 and lib.wg_abi_version() == 16
    assert {"wg_es_perturb_diag", "wg_es_update_diag"} <= set(_lib.EXPORTS)


def _es(**kw):
    """A linear 26 -> 2 policy of 8 sets whose pointers are non-NULL fakes: every call below is refused before anything
    dereferences them.  es->sigma is 0: these calls do not read it."""
    d = dict(n_sets=8, obs_dim=26, hidden=0, act_dim=2, seed=1, generation=0, sigma=0.0, theta=64, w2=64, b2=64)
    d.update(kw)
    return _lib.WgEs(**d)


def _step(**kw):
    d = es.diag_step(lr_theta=0.1, lr_sigma=0.1, shrink=0.8, grow=1.2)
    d.update(kw)
    return _lib.WgEsDiagStep(**d)


def _perturb(lib, e, first=0, n=4, sigma=64):
    return lib.wg_es_perturb_diag(None if e is None else C.byref(e), sigma, first, n, None)


def _update(lib, e, first=0, n=4, sigma=64, util=64, step=True, work=64, outs=(64, 64, 64, 64), **fields):
    st = _step(**fields)
    return lib.wg_es_update_diag(None if e is None else C.byref(e), sigma, first, n, util, C.byref(st) if step else None,
                                 work, *outs, None)


SHARED = [   # es_check's list without the scalar-sigma lines
    ("null es", None, {}, b"null es"),
    ("null theta", dict(theta=None), {}, b"theta"),
    ("null w2", dict(w2=None), {}, b"w2"),
    ("hidden < 0", dict(hidden=-1), {}, b"hidden"),
    ("hidden > 256", dict(hidden=257, w1=64), {}, b"hidden"),
    ("hidden without w1", dict(hidden=5), {}, b"w1"),
    ("b1 without hidden", dict(b1=64), {}, b"b1"),
    ("n_sets odd", dict(n_sets=7), {}, b"n_sets"),
    ("n_sets 0", dict(n_sets=0), {}, b"n_sets"),
    ("first_pair < 0", {}, dict(first=-1), b"pairs"),
    ("range past the end", {}, dict(first=3, n=2), b"pairs"),
    ("n_pairs 0", {}, dict(n=0), b"n_pairs"),
    ("obs_dim 0", dict(obs_dim=0), {}, b"obs_dim"),
    ("act_dim 0", dict(act_dim=0), {}, b"act_dim"),
    ("more than 2^23 parameters", dict(obs_dim=1 << 20, hidden=256, w1=64), {}, b"parameters"),
    ("null sigma vector", {}, dict(sigma=None), b"sigma"),
]
INF, NAN = float("inf"), float("nan")
UPDATE_ONLY = [
    ("null util", dict(util=None), b"util"),
    ("null step", dict(step=False), b"step"),
    ("null workspace", dict(work=None), b"workspace"),
    ("no output", dict(outs=(None, None, None, None)), b"outputs"),
    ("base inf", dict(base=INF), b"base"),
    ("base nan", dict(base=NAN), b"base"),
    ("scale_theta inf", dict(scale_theta=INF), b"scale_theta"),
    ("scale_theta nan", dict(scale_theta=NAN), b"scale_theta"),
    ("scale_sigma inf", dict(scale_sigma=-INF), b"scale_sigma"),
    ("scale_sigma nan", dict(scale_sigma=NAN), b"scale_sigma"),
    ("lr_theta nan", dict(lr_theta=NAN), b"lr_theta"),
    ("lr_theta inf", dict(lr_theta=INF), b"lr_theta"),
    ("lr_sigma nan", dict(lr_sigma=NAN), b"lr_sigma"),
    ("lr_sigma inf", dict(lr_sigma=INF), b"lr_sigma"),
    ("shrink 0", dict(shrink=0.0), b"shrink"),
    ("shrink < 0", dict(shrink=-0.5), b"shrink"),
    ("shrink > 1", dict(shrink=1.5), b"shrink"),
    ("shrink nan", dict(shrink=NAN), b"shrink"),
    ("grow < 1", dict(grow=0.99), b"grow"),
    ("grow inf", dict(grow=INF), b"grow"),
    ("grow nan", dict(grow=NAN), b"grow"),
    ("sigma_min 0", dict(sigma_min=0.0), b"sigma_min"),
    ("sigma_min < 0", dict(sigma_min=-1.0), b"sigma_min"),
    ("sigma_min inf", dict(sigma_min=INF), b"sigma_min"),
    ("sigma_min nan", dict(sigma_min=NAN), b"sigma_min"),
    ("sigma_max < sigma_min", dict(sigma_min=0.5, sigma_max=0.25), b"sigma_max"),
    ("sigma_max nan", dict(sigma_max=NAN), b"sigma_max"),
]


@pytest.mark.parametrize("what,fields,rng,word", SHARED, ids=[r[0] for r in SHARED])
def test_every_einval_is_refused_before_a_launch(lib, what, fields, rng, word):
    e = None if fields is None else _es(**fields)
    assert _perturb(lib, e, **rng) == _lib.WG_EINVAL, what
    assert word in lib.wg_last_error() and b"wg_es_perturb_diag" in lib.wg_last_error(), lib.wg_last_error()
    assert _update(lib, e, **rng) == _lib.WG_EINVAL, what
    assert word in lib.wg_last_error() and b"wg_es_update_diag" in lib.wg_last_error(), lib.wg_last_error()


@pytest.mark.parametrize("what,kw,word", UPDATE_ONLY, ids=[r[0] for r in UPDATE_ONLY])
def test_update_einval_is_refused_before_a_launch(lib, what, kw, word):
    assert _update(lib, _es(), **kw) == _lib.WG_EINVAL, what
    assert word in lib.wg_last_error() and b"wg_es_update_diag" in lib.wg_last_error(), lib.wg_last_error()


def test_es_sigma_is_not_read(lib):
    """es->sigma = 0, negative, NaN or inf is not what refuses a call: with a valid struct otherwise, the first refusal
    is the next check's (a NULL sigma vector), where wg_es_perturb refuses the scalar itself."""
    for s in (0.0, -1.0, NAN, INF):
        e = _es(sigma=s)
        assert _perturb(lib, e, sigma=None) == _lib.WG_EINVAL and b"null sigma vector" in lib.wg_last_error()
        assert _update(lib, e, sigma=None) == _lib.WG_EINVAL and b"null sigma vector" in lib.wg_last_error()
        assert _update(lib, e, util=None) == _lib.WG_EINVAL and b"null util" in lib.wg_last_error()
        assert lib.wg_es_perturb(C.byref(e), 0, 4, None) == _lib.WG_EINVAL and b"sigma must be" in lib.wg_last_error()
    # the limits that are allowed: shrink = 1, grow = 1, sigma_max = +inf or = sigma_min pass every step check (the
    # refusal that follows is the one provoked after them in the list: none is left, so make the output check fail)
    for kw in (dict(shrink=1.0, grow=1.0), dict(sigma_max=INF), dict(sigma_min=0.5, sigma_max=0.5)):
        assert _update(lib, _es(), outs=(None,) * 4, **kw) == _lib.WG_EINVAL and b"outputs" in lib.wg_last_error()


def test_adaptive_trainer_is_exported():
    import walker_gym_amd
    assert walker_gym_amd.AdaptiveEvolutionStrategy is es.AdaptiveEvolutionStrategy
    assert issubclass(es.AdaptiveEvolutionStrategy, es.EvolutionStrategy)
    assert walker_gym_amd.EvolutionStrategy is es.EvolutionStrategy


# ------------------------------------------------------------------ the trainer cases on the reference engine
@pytest.mark.parametrize("H,G", ec.TRAINER_CASES)
def test_trainer_cases_stay_finite_and_adapt(H, G):
    """Every generation that tests/test_gpu_es_adaptive.py compares bit for bit: rows, rewards, actions, fitness, both
    estimates, theta and sigma finite and no walker non-finite; g_sigma non-zero for most parameters; theta moved and
    sigma_vec changed in bits (in most entries) after each generation, and stayed positive."""
    gens = ac.oracle_training(H, G)
    theta, sigma = ec.theta0(H), ac.sigma0(H)
    assert len(np.unique(sigma)) == 4 and sigma.max() <= f32(1.25) * f32(ec.SIGMA[H])
    for g in gens:
        assert np.isfinite(g["obs"]).all() and np.isfinite(g["reward"]).all() and np.isfinite(g["action"]).all()
        assert g["nonfinite"] == 0
        assert np.isfinite(g["fitness"]).all() and len(np.unique(g["fitness"])) > G // 2
        for key in ("grad", "grad_sigma", "theta", "sigma"):
            assert np.isfinite(g[key]).all(), key
        assert (g["grad_sigma"] != 0).mean() > 0.9 and (g["grad"] != 0).mean() > 0.9
        assert not np.array_equal(g["theta"], theta)
        assert (g["sigma"].view(np.uint32) != sigma.view(np.uint32)).mean() > 0.9 and (g["sigma"] > 0).all()
        theta, sigma = g["theta"], g["sigma"]

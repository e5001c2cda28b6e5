"""Evolution strategies without a GPU: the Philox known answers and the noise's moments, the vectorised numpy
restatements against a scalar pure-Python one, sign and scaling of the update on a quadratic, every WG_EINVAL of
wg_es_perturb / wg_es_update refused before a launch, wg_es's layout, and the finiteness (on the reference engine) of
the closed loops whose bits tests/test_gpu_es.py compares."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import es_cases as ec
from walker_gym_amd import _lib, build, es

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
M32 = 0xFFFFFFFF


# ------------------------------------------------------------------ Philox and the noise
@pytest.mark.parametrize("ctr,key,want", [
    ("00000000 00000000 00000000 00000000", "00000000 00000000", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(ctr, key, want):
    h = lambda s: [int(w, 16) for w in s.split()]
    got = es.philox4x32(np.array(h(ctr), np.uint64), np.array(h(key), np.uint64))
    assert got.dtype == np.uint32 and [int(x) for x in got] == h(want)
    assert _philox_scalar(h(ctr), h(key)) == h(want)


def test_noise_constant_bits():
    assert es.NOISE_SCALE.dtype == f32
    assert struct.unpack("<I", es.NOISE_SCALE.tobytes())[0] == 0x379CC471 == 933020785
    assert es.NOISE_SCALE == f32(1 / np.sqrt(8 * (65536 ** 2 - 1) / 12))


def test_noise_moments():
    e = es.es_noise_numpy(123, 0, 0, 1024, 1024)
    assert e.shape == (1024, 1024) and e.dtype == f32
    mean, std = float(e.astype(np.float64).mean()), float(e.astype(np.float64).std())
    print("mean", mean, "std", std, "max |eps|", float(np.abs(e).max()))
    assert abs(mean) < 0.005 and abs(std - 1) < 0.005 and float(np.abs(e).max()) <= 4.9
    # a pure function of its arguments: a slice of the pairs is the same values; other generations / seeds are not
    assert np.array_equal(es.es_noise_numpy(123, 0, 100, 3, 1024), e[100:103])
    assert not np.array_equal(es.es_noise_numpy(123, 1, 0, 4, 64), e[:4, :64])
    assert not np.array_equal(es.es_noise_numpy(123 + (1 << 32), 0, 0, 4, 64), e[:4, :64])


# ------------------------------------------------------------------ a scalar restatement in Python integers and scalars
def _philox_scalar(c, k):
    c0, c1, c2, c3 = c
    k0, k1 = k
    for _ in range(10):
        p0, p1 = es.PHILOX_M0 * c0, es.PHILOX_M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + es.PHILOX_W0) & M32, (k1 + es.PHILOX_W1) & M32
    return [c0, c1, c2, c3]


def _eps_scalar(seed, gen, j, k):
    w = _philox_scalar([k, j, gen, 0x45530001], [seed & M32, seed >> 32])
    s = sum((x & 0xFFFF) + (x >> 16) for x in w)
    return f32(f32(s - 262140) * es.NOISE_SCALE)


def _perturb_scalar(theta, sigma, seed, gen, first, n):
    out = np.zeros((2 * n, len(theta)), f32)
    for i in range(n):
        for k in range(len(theta)):
            d = f32(f32(sigma) * _eps_scalar(seed, gen, first + i, k))
            out[2 * i, k] = f32(theta[k] + d)
            out[2 * i + 1, k] = f32(theta[k] - d)
    return out


def _utilities_scalar(fit):
    G = len(fit)
    key = [(-np.inf if np.isnan(x) else float(x)) for x in fit]
    order = sorted(range(G), key=lambda g: (key[g], g))
    util = np.zeros(G, f32)
    c = f32(1.0 / (2 * (G - 1)))
    for r, g in enumerate(order):
        util[g] = f32(f32(2 * r - (G - 1)) * c)
    return util


def _update_scalar(theta, util, seed, gen, first, n, scale, lr):
    K = len(theta)
    grad, out = np.zeros(K, f32), np.zeros(K, f32)
    with np.errstate(all="ignore"):
        for k in range(K):
            S = 0.0                                   # Python floats are IEEE doubles: every operation rounds once
            for a in range(0, n, 256):
                P = 0.0
                for jl in range(a, min(a + 256, n)):
                    j = first + jl
                    d = f32(util[2 * j] - util[2 * j + 1])
                    P = P + float(d) * float(_eps_scalar(seed, gen, j, k))
                S = S + P
            grad[k] = f32(S * float(scale))
            out[k] = f32(theta[k] + f32(f32(lr) * grad[k]))
    return grad, out


SEED = (3 << 32) + 99


@pytest.mark.parametrize("n_pairs", [1, 3, 257])
def test_numpy_restatements_equal_scalar_restatement(n_pairs):
    K, first, gen = 7, 2, 5
    rng = np.random.default_rng(n_pairs)
    theta = rng.standard_normal(K).astype(f32)
    sigma = f32(0.05)
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    got = es.es_perturb_numpy(theta, sigma, SEED, gen, first, n_pairs)
    assert got.dtype == f32 and np.array_equal(bits(got), bits(_perturb_scalar(theta, sigma, SEED, gen, first, n_pairs)))
    G = 2 * (first + n_pairs)
    fit = rng.standard_normal(G).astype(f32)
    fit[1] = fit[0]                                    # a tie breaks by index
    if G > 6:
        fit[5] = fit[0]
        fit[4] = np.nan                                # ranks lowest
    util = es.es_utilities_numpy(fit)
    assert util.dtype == f32 and np.array_equal(bits(util), bits(_utilities_scalar(fit)))
    assert util.min() == f32(-0.5) and util.max() == f32(0.5) and len(np.unique(util)) == G
    if G > 6:
        assert util[4] == f32(-0.5) and util[0] < util[1] < util[5]
    scale, lr = 1.0 / (2 * n_pairs * float(sigma)), f32(0.3)
    for u in (util, np.where(np.arange(G) == 2 * first, f32(np.nan), util).astype(f32)):   # and a NaN utility
        g, t = es.es_update_numpy(theta, u, SEED, gen, first, n_pairs, scale, lr)
        gs, ts = _update_scalar(theta, u, SEED, gen, first, n_pairs, scale, lr)
        assert g.dtype == f32 and t.dtype == f32
        assert np.array_equal(bits(g), bits(gs)) and np.array_equal(bits(t), bits(ts))
    assert np.isnan(g).all()                           # the NaN pair reaches every parameter's sum


# ------------------------------------------------------------------ sign and scaling, end to end
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_quadratic_descends(seed):
    K, G, sigma, lr = 54, 64, f32(0.1), f32(0.2)
    target = np.random.default_rng(seed).standard_normal(K).astype(f32)
    theta = np.zeros(K, f32)
    loss0 = float(((theta - target).astype(np.float64) ** 2).sum())
    for gen in range(30):
        cand = es.es_perturb_numpy(theta, sigma, seed, gen, 0, G // 2)
        fit = -((cand - target[None]) ** 2).sum(axis=1).astype(f32)
        util = es.es_utilities_numpy(fit)
        _, theta = es.es_update_numpy(theta, util, seed, gen, 0, G // 2, 1.0 / (2 * (G // 2) * float(sigma)), lr)
    loss = float(((theta - target).astype(np.float64) ** 2).sum())
    print("seed", seed, "loss ratio", loss / loss0)
    assert loss < 0.1 * loss0


# ------------------------------------------------------------------ the C boundary
@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def test_wg_es_matches_header_and_abi_stays_16(lib, tmp_path):
    fields = [f for f, _ in _lib.WgEs._fields_]
    lines = "".join(f'  printf("{f} %zu\\n", offsetof(wg_es, {f}));\n' for f in fields)
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "walker_hip.h"\nint main(void) {\n' + lines +
                     '  printf("sizeof %zu\\n", sizeof(wg_es));\n  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(probe)], check=True)
    got = dict(line.rsplit(" ", 1) for line in
               subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().splitlines())
    assert int(got["sizeof"]) == C.sizeof(_lib.WgEs)
    for f in fields:
        assert getattr(_lib.WgEs, f).offset == int(got[f]), f
    assert _lib.ABI_VERSION == 16 and lib.wg_abi_version() == 16
    assert {"wg_es_perturb", "wg_es_update"} <= set(_lib.EXPORTS)


def _es(**kw):
    """A linear 26 -> 2 policy of 8 sets whose pointers are non-NULL fakes: every call below is refused before anything
    dereferences them."""
    d = dict(n_sets=8, obs_dim=26, hidden=0, act_dim=2, seed=1, generation=0, sigma=0.05, theta=64, w2=64, b2=64)
    d.update(kw)
    return _lib.WgEs(**d)


REFUSED = [
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
    ("sigma 0", dict(sigma=0.0), {}, b"sigma"),
    ("sigma < 0", dict(sigma=-0.1), {}, b"sigma"),
    ("sigma nan", dict(sigma=float("nan")), {}, b"sigma"),
    ("sigma inf", dict(sigma=float("inf")), {}, b"sigma"),
    ("obs_dim 0", dict(obs_dim=0), {}, b"obs_dim"),
    ("act_dim 0", dict(act_dim=0), {}, b"act_dim"),
    ("more than 2^23 parameters", dict(obs_dim=1 << 20, hidden=256, w1=64), {}, b"parameters"),
]
UPDATE_ONLY = [
    ("null util", dict(util=None), b"util"),
    ("null workspace", dict(work=None), b"workspace"),
    ("scale inf", dict(scale=float("inf")), b"scale"),
    ("scale nan", dict(scale=float("nan")), b"scale"),
    ("lr nan", dict(lr=float("nan")), b"lr"),
    ("no output", dict(grad=None, out=None), b"both null"),
]


def _update(lib, e, first=0, n=4, util=64, scale=1.0, lr=0.1, work=64, grad=64, out=64):
    return lib.wg_es_update(None if e is None else C.byref(e), first, n, util, scale, lr, work, grad, out, None)


@pytest.mark.parametrize("what,fields,rng,word", REFUSED, ids=[r[0] for r in REFUSED])
def test_every_einval_is_refused_before_a_launch(lib, what, fields, rng, word):
    e = None if fields is None else _es(**fields)
    first, n = rng.get("first", 0), rng.get("n", 4)
    assert lib.wg_es_perturb(None if e is None else C.byref(e), first, n, None) == _lib.WG_EINVAL, what
    assert word in lib.wg_last_error() and b"wg_es_perturb" in lib.wg_last_error(), lib.wg_last_error()
    assert _update(lib, e, first, n) == _lib.WG_EINVAL, what
    assert word in lib.wg_last_error() and b"wg_es_update" in lib.wg_last_error(), lib.wg_last_error()


@pytest.mark.parametrize("what,kw,word", UPDATE_ONLY, ids=[r[0] for r in UPDATE_ONLY])
def test_update_einval_is_refused_before_a_launch(lib, what, kw, word):
    assert _update(lib, _es(), **kw) == _lib.WG_EINVAL, what
    assert word in lib.wg_last_error(), lib.wg_last_error()


def test_es_module_is_exported():
    import walker_gym_amd
    assert walker_gym_amd.EvolutionStrategy is es.EvolutionStrategy
    assert es.param_count(26, 0, 2, True) == 54 and es.param_count(26, 5, 2, True) == 147
    assert es.param_count(152, 24, 5, False) == 152 * 24 + 24 * 5
    seg = es.split_theta(np.arange(147, dtype=f32), 26, 5, 2, True)
    assert seg["w1"][1, 0] == 5 and seg["b1"][0] == 130 and seg["w2"][1, 0] == 137 and seg["b2"][1] == 146
    with pytest.raises(ValueError):
        es.split_theta(np.zeros(146, f32), 26, 5, 2, True)


# ------------------------------------------------------------------ the trainer cases stay finite on the reference engine
@pytest.mark.parametrize("H,G", ec.TRAINER_CASES)
def test_trainer_cases_stay_finite(H, G):
    """Every generation that tests/test_gpu_es.py compares bit for bit: all rows, rewards and actions finite, no walker
    non-finite at the end, the clip engaged on some outputs and not all, fitness values that differ (so that the ranks
    mean something), and a theta that moves."""
    gens = ec.oracle_training(H, G)
    prev = ec.theta0(H)
    for g in gens:
        assert np.isfinite(g["obs"]).all() and np.isfinite(g["reward"]).all() and np.isfinite(g["action"]).all()
        assert g["nonfinite"] == 0
        hit = np.abs(g["action"]) == f32(1.0)
        assert hit.any() and not hit.all()
        assert np.isfinite(g["fitness"]).all() and len(np.unique(g["fitness"])) > G // 2
        assert np.isfinite(g["grad"]).all() and np.isfinite(g["theta"]).all()
        assert not np.array_equal(g["theta"], prev)
        prev = g["theta"]
        first = np.where(g["done"].any(axis=0), g["done"].argmax(axis=0), ec.T)
        assert (first < ec.T).all() and len(np.unique(first)) >= 2

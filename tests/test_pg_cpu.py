"""Policy-gradient support without a GPU: the action-noise contract against a scalar pure-Python Philox, gae_numpy against
a scalar loop, every WG_EINVAL of wg_rollout_stochastic and wg_gae refused before a launch (host pointers), wg_action_noise's
layout against its ctypes mirror, and the conditions that keep tests/test_gpu_stochastic_rollout.py's cases honest, checked
on the reference engine alone."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pg_cases as gc
from walker_gym_amd import _lib, build, es, pg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
M32 = 0xFFFFFFFF
bits = lambda a: np.ascontiguousarray(a, dtype=f32).view(np.uint32)


# ------------------------------------------------------------------ the noise
def _philox_scalar(c, k):
    c0, c1, c2, c3 = c
    k0, k1 = k
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c0, 0xCD9E8D57 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & M32, (p0 >> 32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return [c0, c1, c2, c3]


def _aeps_scalar(seed, t, w, c, tag=0x41430001):
    out = _philox_scalar([c, w, t, tag], [seed & M32, seed >> 32])
    s = sum((x & 0xFFFF) + (x >> 16) for x in out)
    return f32(f32(s - 262140) * f32(np.uint32(0x379CC471).view(f32)))


@pytest.mark.parametrize("seed", [0, 77, (9 << 32) + 5, (1 << 64) - 1])
def test_action_noise_equals_scalar_philox(seed):
    sb, wb, T, N, Cc = 11, 1000, 3, 5, 4
    got = pg.action_noise_numpy(seed, sb, T, wb, N, Cc)
    assert got.shape == (T, N, Cc) and got.dtype == f32
    want = np.array([[[_aeps_scalar(seed, sb + t, wb + w, c) for c in range(Cc)] for w in range(N)] for t in range(T)], f32)
    assert np.array_equal(bits(got), bits(want))
    assert float(np.abs(got).max()) <= 4.9


def test_action_noise_domain_key_and_counters():
    seed = (3 << 32) + 99
    a = pg.action_noise_numpy(seed, 0, 4, 0, 6, 5)
    # another counter domain than the ES variate of the same (seed, t, w, c)
    assert pg.ACTION_NOISE_TAG == 0x41430001 != es.NOISE_TAG
    e = np.stack([es.es_noise_numpy(seed, t, 0, 6, 5) for t in range(4)])      # eps(seed, generation t, pair w, k c)
    assert e.shape == a.shape and (bits(e) != bits(a)).mean() > 0.99
    # the high key word counts: a seed above 2^32 is not its low word
    assert not np.array_equal(pg.action_noise_numpy(99, 0, 4, 0, 6, 5), a)
    # step_base and walker_base shift the counters, not the key: a window of a larger call is that call's window
    assert np.array_equal(pg.action_noise_numpy(seed, 2, 2, 3, 3, 5), a[2:4, 3:6])
    assert np.array_equal(pg.action_noise_numpy(seed, (1 << 32) - 2, 2, (1 << 32) - 3, 3, 2)[1, 2],
                          [_aeps_scalar(seed, M32, M32, c) for c in range(2)])
    for bad in (dict(seed=-1), dict(seed=1 << 64), dict(step_base=(1 << 32) - 1), dict(walker_base=(1 << 32) - 2)):
        kw = dict(seed=1, step_base=0, n_steps=2, walker_base=0, n_walkers=3, act_dim=1)
        kw.update(bad)
        with pytest.raises(ValueError):
            pg.action_noise_numpy(**kw)
    big = pg.action_noise_numpy(5, 0, 64, 0, 256, 16).astype(np.float64)
    assert abs(big.mean()) < 0.01 and abs(big.std() - 1) < 0.01


def test_stochastic_forward_numpy_is_forward_numpy_plus_the_noise():
    import torch
    from walker_gym_amd.policy import MLPPolicy
    rng = np.random.default_rng(3)
    n, D, H, Cc, G = 12, 7, 5, 3, 3
    t = lambda a: torch.from_numpy(a.astype(f32))
    pol = MLPPolicy(t(rng.standard_normal((G, H, Cc))), t(rng.standard_normal((G, Cc))), t(rng.standard_normal((G, D, H))),
                    t(rng.standard_normal((G, H))), act_limit=1.0)
    x = rng.standard_normal((n, D)).astype(f32)
    x[0, 0] = np.nan
    sg = rng.uniform(0.1, 1, (G, Cc)).astype(f32)
    u, a, e = pg.stochastic_forward_numpy(pol, x, sg, 42, 9, walker_base=100)
    y = MLPPolicy(pol.w2, pol.b2, pol.w1, pol.b1, act_limit=float("inf")).forward_numpy(x)
    sets = np.arange(n) // (n // G)
    for r in range(n):
        for c in range(Cc):
            ee = _aeps_scalar(42, 9, 100 + r, c)
            uu = f32(y[r, c] + f32(sg[sets[r], c] * ee))
            aa = f32(-1) if uu < -1 else (f32(1) if uu > 1 else uu)
            assert bits(e[r, c]) == bits(ee) and bits(u[r, c]) == bits(uu) and bits(a[r, c]) == bits(aa)
    # rows 4.. of the batch, named as such, are the same values
    u2, a2, e2 = pg.stochastic_forward_numpy(pol, x[4:8], sg, 42, 9, walker_base=100, first_walker=4, n_walkers_total=n)
    assert np.array_equal(bits(u2), bits(u[4:8])) and np.array_equal(bits(e2), bits(e[4:8]))
    # sigma = 0: u is y, but for y = -0.0, which becomes +0.0 where 0 * aeps is +0.0 (aeps >= 0)
    z = MLPPolicy(t(np.zeros((D, Cc))), t(np.full(Cc, -0.0)), act_limit=1.0)   # -0.0 + x * 0 = -0.0 for x < 0
    u0, a0, e0 = pg.stochastic_forward_numpy(z, -np.abs(x[1:]), 0.0, 1, 0)
    assert np.array_equal(bits(z.forward_numpy(-np.abs(x[1:]))), np.full((n - 1, Cc), 0x80000000, np.uint32))
    want0 = np.where(e0 >= 0, 0, 0x80000000).astype(np.uint32)
    assert (e0 >= 0).any() and (e0 < 0).any()
    assert np.array_equal(bits(u0), want0) and np.array_equal(bits(a0), want0)
    u1, _, _ = pg.stochastic_forward_numpy(pol, x[1:], 0.0, 1, 0, first_walker=1, n_walkers_total=n)
    assert np.array_equal(bits(u1), bits(y[1:]))


# ------------------------------------------------------------------ GAE
def _gae_scalar(r, v, nv, term, cut, gamma, lam):
    T, N = r.shape
    adv, ret = np.zeros((T, N), f32), np.zeros((T, N), f32)
    g, gl = f32(gamma), f32(f32(gamma) * f32(lam))
    with np.errstate(all="ignore"):
        for w in range(N):
            carry = f32(0.0)
            for t in range(T - 1, -1, -1):
                n = f32(0.0) if term is not None and term[t, w] else f32(nv[t, w])
                delta = f32(f32(f32(r[t, w]) + f32(g * n)) - f32(v[t, w]))
                c = f32(0.0) if cut is not None and cut[t, w] else carry
                carry = f32(delta + f32(gl * c))
                adv[t, w] = carry
                ret[t, w] = f32(carry + f32(v[t, w]))
    return adv, ret


def gae_inputs(T, N, seed):
    """[T, N] inputs with term and cut on the last step, on adjacent steps and together, and a NaN value."""
    rng = np.random.default_rng(seed)
    r, v, nv = (rng.standard_normal((T, N)).astype(f32) * s for s in (1.0, 3.0, 3.0))
    term = (rng.random((T, N)) < 0.2).astype(np.uint8)
    cut = (term | (rng.random((T, N)) < 0.2)).astype(np.uint8)
    term[-1, 0] = cut[-1, 0] = 1
    if N > 1:
        cut[-1, 1], term[-1, 1] = 1, 0
    if T > 1:
        term[T - 2:, -1] = 1
        cut[T - 2:, -1] = 1
    v[T // 2, N // 2] = np.nan
    return r, v, nv, term, cut


@pytest.mark.parametrize("T", [1, 2, 9])
@pytest.mark.parametrize("flags", ["both", "term", "cut", "none"])
def test_gae_numpy_equals_scalar_loop(T, flags):
    r, v, nv, term, cut = gae_inputs(T, 7, 10 + T)
    term = term if flags in ("both", "term") else None
    cut = cut if flags in ("both", "cut") else None
    for gamma, lam in ((0.99, 0.95), (1.0, 0.0), (1.0, 1.0)):
        adv, ret = pg.gae_numpy(r, v, nv, term, cut, gamma, lam)
        wa, wr = _gae_scalar(r, v, nv, term, cut, gamma, lam)
        assert adv.dtype == f32 and ret.dtype == f32
        assert np.array_equal(bits(adv), bits(wa)) and np.array_equal(bits(ret), bits(wr))
    assert np.isnan(adv[T // 2, 3]) and (T == 1 or np.isnan(adv[0, 3]) == (cut is None or not cut[:T // 2, 3].any()))


def test_gae_hand_case():
    """Three steps, gamma = 0.5, lam = 1: a plain trace, a cut trace, a terminal step."""
    r = np.array([[1, 1, 1], [2, 2, 2], [4, 4, 4]], f32)
    v = np.zeros((3, 3), f32)
    nv = np.array([[0, 0, 0], [0, 0, 0], [8, 8, 8]], f32)
    cut = np.array([[0, 0, 0], [0, 1, 0], [0, 0, 0]], np.uint8)
    term = np.array([[0, 0, 0], [0, 0, 0], [0, 0, 1]], np.uint8)
    adv, ret = pg.gae_numpy(r, v, nv, term, cut, 0.5, 1.0)
    assert adv[:, 0].tolist() == [1 + 0.5 * (2 + 0.5 * 8), 2 + 0.5 * 8, 8.0]
    assert adv[:, 1].tolist() == [1 + 0.5 * 2, 2.0, 8.0]
    assert adv[:, 2].tolist() == [1 + 0.5 * (2 + 0.5 * 4), 2 + 0.5 * 4, 4.0]
    assert np.array_equal(adv, ret)


# ------------------------------------------------------------------ the C boundary
@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def test_wg_action_noise_matches_header_and_abi_stays_16(lib, tmp_path):
    fields = [f for f, _ in _lib.WgActionNoise._fields_]
    lines = "".join(f'  printf("{f} %zu\\n", offsetof(wg_action_noise, {f}));\n' for f in fields)
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "walker_hip.h"\nint main(void) {\n' + lines +
                     '  printf("sizeof %zu\\n", sizeof(wg_action_noise));\n  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(probe)], check=True)
    got = dict(line.rsplit(" ", 1) for line in
               subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().splitlines())
    assert int(got["sizeof"]) == C.sizeof(_lib.WgActionNoise)
    for f in fields:
        assert getattr(_lib.WgActionNoise, f).offset == int(got[f]), f
    assert _lib.ABI_VERSION == 16 and lib.wg_abi_version() == 16
    assert "#define WG_ABI_VERSION 16" in open(os.path.join(ROOT, "include", "walker_hip.h")).read()
    assert {"wg_rollout_stochastic", "wg_gae"} <= set(_lib.EXPORTS)


def _batch(**kw):
    """A canonical-shaped uniform batch with auto-reset's pointers, all non-NULL fakes: every call below is refused
    before anything dereferences them (as tests/test_rollout_episodes_cpu.py::_batch)."""
    b = _lib.WgBatch(N=128, M=16, K=40, A=8)
    for f in ("pos", "vel", "acc", "mass", "edges", "inc", "inc_off", "muscle_x", "muscle_bounds", "steps",
              "init_pos", "init_vel", "init_acc", "init_muscle_x", "episodes"):
        setattr(b, f, 64)
    for k, v in kw.items():
        setattr(b, k, v)
    return b


def _pol(**kw):
    d = dict(n_sets=1, obs_dim=152, hidden=0, act_dim=8, w2=64, act_limit=1.0)
    d.update(kw)
    return _lib.WgPolicy(**d)


def _nz(**kw):
    d = dict(seed=1, step_base=0, walker_base=0, sigma=64)
    d.update(kw)
    return _lib.WgActionNoise(**d)


_NONE = object()
OFF, AR = dict(in3d=1), dict(in3d=1, auto_reset=1)
P = 128 * 16
ROW = 128 * 8

# (what, batch, params, policy, noise, stats, outputs, n_steps, a word of the message); stats: _NONE = a NULL pointer
BOTH_MODES = [
    ("null policy", {}, None, {}, {}, None, 1, b"null policy"),
    ("null w2", {}, dict(w2=None), {}, {}, None, 1, b"w2"),
    ("hidden < 0", {}, dict(hidden=-1), {}, {}, None, 1, b"hidden"),
    ("hidden > 256", {}, dict(hidden=257, w1=64), {}, {}, None, 1, b"hidden"),
    ("hidden without w1", {}, dict(hidden=24), {}, {}, None, 1, b"w1"),
    ("act_dim 0", {}, dict(act_dim=0), {}, {}, None, 1, b"act_dim"),
    ("act_dim > A", {}, dict(act_dim=9), {}, {}, None, 1, b"act_dim"),
    ("obs_dim", {}, dict(obs_dim=151), {}, {}, None, 1, b"obs_dim"),
    ("n_sets 0", {}, dict(n_sets=0), {}, {}, None, 1, b"n_sets"),
    ("n_sets not dividing N", {}, dict(n_sets=3), {}, {}, None, 1, b"n_sets"),
    ("n_steps 0", {}, {}, {}, {}, None, 0, b"n_steps"),
    ("act_limit", {}, dict(act_limit=0.0), {}, {}, None, 1, b"act_limit"),
    ("obs_stride", {}, {}, {}, {}, dict(obs=64, obs_stride=151), 1, b"obs_stride"),
    ("ragged", dict(ragged=2, mass_off=64, edge_off=64, muscle_off=64), {}, {}, {}, None, 1, b"lean kernel"),
    ("M not dividing 64", dict(M=12), dict(obs_dim=3 * 3 * 12 + 8), {}, {}, None, 1, b"lean kernel"),
    ("no muscle_bounds", dict(muscle_bounds=None), {}, {}, {}, None, 1, b"muscle_bounds"),
    ("nonfinite", {}, {}, {}, {}, dict(nonfinite=64), 1, b"nonfinite"),
    ("momentum", {}, {}, {}, {}, dict(momentum=64), 1, b"momentum"),
    # the noise's own
    ("null noise", {}, {}, _NONE, {}, None, 1, b"null action noise"),
    ("null sigma", {}, {}, dict(sigma=None), {}, None, 1, b"sigma"),
    ("raw_out stride", {}, {}, dict(raw_out=64, raw_out_step=ROW - 1), {}, None, 1, b"raw_out_step"),
    ("eps_out stride", {}, {}, dict(eps_out=64, eps_out_step=ROW - 1), {}, None, 1, b"eps_out_step"),
    ("eps_out stride with fewer columns", {}, dict(act_dim=5), dict(eps_out=64, eps_out_step=128 * 5 - 1), {}, None, 1,
     b"eps_out_step"),
    ("step_base wraps", {}, {}, dict(step_base=M32 - 1), {}, None, 3, b"step_base"),
    ("walker_base wraps", {}, {}, dict(walker_base=M32 - 126), {}, None, 1, b"walker_base"),
]
OFF_ONLY = [
    ("stats without auto-reset", {}, {}, {}, {}, None, 1, b"st must be NULL"),
    ("reset out", {}, {}, {}, _NONE, dict(reset=64), 1, b"reset"),
    ("final_obs out", {}, {}, {}, _NONE, dict(final_obs=64, obs_stride=152), 1, b"final_obs"),
]
AR_ONLY = [
    ("null stats", {}, {}, {}, _NONE, None, 1, b"null episode stats"),
    ("auto_reset bits", {}, {}, {}, {}, None, 1, b"bits 1"),
    ("no init_pos", dict(init_pos=None), {}, {}, {}, None, 1, b"snapshot"),
    ("no episodes", dict(episodes=None), {}, {}, {}, None, 1, b"episodes"),
    ("noise rows 0", dict(reset_noise=64, reset_noise_rows=0, reset_noise_stride=3 * P), {}, {}, {}, None, 1,
     b"reset_noise_rows"),
    ("noise stride", dict(reset_noise=64, reset_noise_rows=2, reset_noise_stride=3 * P - 1), {}, {}, {}, None, 1,
     b"reset_noise_stride"),
    ("ep_slots < 0", {}, {}, {}, dict(ep_slots=-1), None, 1, b"ep_slots"),
    ("ep_return without slots", {}, {}, {}, dict(ep_return=64), None, 1, b"ep_slots 0"),
    ("return_out", {}, dict(return_out=64), {}, {}, None, 1, b"return_out"),
    ("final_obs stride", {}, {}, {}, {}, dict(final_obs=64, obs_stride=151), 1, b"obs_stride"),
]


def _stochastic(lib, b, p, pol, nz, st, o, n_steps):
    ref = lambda x: None if x is None else C.byref(x)
    return lib.wg_rollout_stochastic(C.byref(b), C.byref(p), ref(pol), ref(nz), ref(o), ref(st), n_steps, None)


def _run(lib, mode, what, batch, pol, noise, stats, out, steps, word):
    params = dict(AR if mode == "ar" else OFF)
    if what == "auto_reset bits":
        params["auto_reset"] = 4
    if mode == "ar":
        st = None if stats is _NONE else _lib.WgEpisodeStats(**stats)
    else:   # without auto-reset st must be NULL: _NONE and {} both mean that, but for the case that sets it
        st = _lib.WgEpisodeStats() if what == "stats without auto-reset" else None
    rc = _stochastic(lib, _batch(**batch), _lib.WgParams(**params), None if pol is None else _pol(**pol),
                     None if noise is _NONE else _nz(**noise), st, None if out is None else _lib.WgOutputs(**out), steps)
    assert rc == _lib.WG_EINVAL, what
    msg = lib.wg_last_error()
    assert word in msg, (what, msg)


@pytest.mark.parametrize("mode", ["off", "ar"])
@pytest.mark.parametrize("row", BOTH_MODES, ids=[r[0] for r in BOTH_MODES])
def test_stochastic_einval_in_both_modes(lib, mode, row):
    _run(lib, mode, *row)


@pytest.mark.parametrize("row", OFF_ONLY, ids=[r[0] for r in OFF_ONLY])
def test_stochastic_einval_without_auto_reset(lib, row):
    _run(lib, "off", *row)


@pytest.mark.parametrize("row", AR_ONLY, ids=[r[0] for r in AR_ONLY])
def test_stochastic_einval_with_auto_reset(lib, row):
    _run(lib, "ar", *row)


def test_stochastic_other_refusals(lib, monkeypatch):
    b, pol, nz = _batch(), _pol(), _nz()
    assert lib.wg_rollout_stochastic(None, C.byref(_lib.WgParams(**OFF)), C.byref(pol), C.byref(nz), None, None, 1,
                                     None) == _lib.WG_EINVAL
    assert lib.wg_rollout_stochastic(C.byref(b), None, C.byref(pol), C.byref(nz), None, None, 1, None) == _lib.WG_EINVAL
    assert b"null params" in lib.wg_last_error()
    for kw in (dict(spring_mode=1), dict(pair_mode=1)):
        assert _stochastic(lib, b, _lib.WgParams(**dict(OFF, **kw)), pol, nz, None, None, 1) == _lib.WG_EINVAL
        assert b"lean kernel" in lib.wg_last_error() and b"wg_rollout_stochastic" in lib.wg_last_error()
    # the 80 KiB rule, unchanged (tests/test_rollout_episodes_cpu.py's arithmetic: 80 KiB exactly with four words)
    M, A = 64, 64
    D = 3 * 3 * M + A
    a16 = lambda n: (n + 15) & ~15

    def lds(K, H, words):
        pl = (K + 3) & ~3
        sl = a16(pl * 24) + a16(pl * 12) + a16(K * 4 + 4) + a16(A * 4)
        return 4 * (sl + a16(D * 4) + a16(H * 4) + a16(A * 4) + 4 * words)
    K, H = next((K, H) for K in range(64, 513) for H in range(4, 257, 4) if lds(K, H, 4) == 80 * 1024)
    big = _batch(N=8192, M=M, K=K, A=A)
    wide = _pol(obs_dim=D, hidden=H, w1=64, act_dim=A)
    assert _stochastic(lib, big, _lib.WgParams(**AR), wide, nz, _lib.WgEpisodeStats(), None, 1) == _lib.WG_ERANGE
    assert b"LDS" in lib.wg_last_error()
    monkeypatch.setenv("WG_LEAN", "0")
    assert _stochastic(lib, b, _lib.WgParams(**OFF), pol, nz, None, None, 1) == _lib.WG_EINVAL
    assert b"lean kernel" in lib.wg_last_error()


def _gae(lib, T=4, N=8, stride=None, gamma=0.99, lam=0.95, **ptr):
    """wg_gae over host arrays (never dereferenced: every call is refused); ptr: name -> None (NULL) or another array."""
    a = {k: np.zeros((T, stride or N), f32) for k in ("reward", "value", "next_value", "adv", "ret")}
    a.update({k: np.zeros((T, stride or N), np.uint8) for k in ("term", "cut")})
    a.update(ptr)
    p = lambda x: None if x is None else C.c_void_p(x if isinstance(x, int) else x.ctypes.data)
    rc = lib.wg_gae(p(a["reward"]), p(a["value"]), p(a["next_value"]), p(a["term"]), p(a["cut"]), T, N,
                    N if stride is None else stride, gamma, lam, p(a["adv"]), p(a["ret"]), None)
    return rc, a


def test_gae_einval_table(lib):
    for name in ("reward", "value", "next_value", "adv"):
        rc, _ = _gae(lib, **{name: None})
        assert rc == _lib.WG_EINVAL and name.encode() in lib.wg_last_error(), name
    for kw, word in ((dict(T=0), b"n_steps"), (dict(N=0, stride=8), b"N 0"), (dict(stride=7), b"step_stride"),
                     (dict(gamma=float("nan")), b"gamma"), (dict(gamma=float("inf")), b"gamma"),
                     (dict(lam=float("nan")), b"lam"), (dict(lam=float("-inf")), b"lam")):
        rc, _ = _gae(lib, **kw)
        assert rc == _lib.WG_EINVAL and word in lib.wg_last_error(), (kw, lib.wg_last_error())
    # adv or ret aliasing an input: the same array, and an overlap of one element at either end
    base = np.zeros((9, 8), f32)
    for out in ("adv", "ret"):
        for inp in ("reward", "value", "next_value"):
            for o_, i_ in ((base[:4], base[:4]), (base[:4], base[3:7].reshape(-1)[7:]), (base[4:8], base.reshape(-1)[1:])):
                rc, _ = _gae(lib, **{out: o_.ctypes.data, inp: i_.ctypes.data})
                assert rc == _lib.WG_EINVAL and b"aliases" in lib.wg_last_error(), (out, inp)
        flags = np.zeros(9 * 8 * 4, np.uint8)
        for inp in ("term", "cut"):
            rc, _ = _gae(lib, **{out: flags.ctypes.data, inp: flags.ctypes.data + 4 * 32 - 1})
            assert rc == _lib.WG_EINVAL and b"aliases" in lib.wg_last_error(), (out, inp)
    rc, _ = _gae(lib, adv=base[:4].ctypes.data, ret=base[3:7].ctypes.data)
    assert rc == _lib.WG_EINVAL and b"aliases" in lib.wg_last_error()


def test_pg_is_exported():
    import walker_gym_amd
    from walker_gym_amd.batched_env import BatchedPhysicsEnv
    assert walker_gym_amd.pg is pg
    assert walker_gym_amd.rollout_stochastic is BatchedPhysicsEnv.rollout_stochastic
    for f in ("action_noise_numpy", "stochastic_forward_numpy", "gae_numpy", "gae", "collect"):
        assert callable(getattr(pg, f))


# ------------------------------------------------------------------ the GPU cases cannot pass vacuously
def _conditions(ref, case, T):
    sg = gc.sigma_of(case.name)
    for k in ("obs", "reward", "action", "raw", "eps"):
        assert np.isfinite(ref[k]).all(), k
    u, a, e = ref["raw"], ref["action"], ref["eps"]
    clipped = np.abs(u) > f32(case.L)
    print(case.name, "clipped", float(clipped.mean()))
    if np.isinf(case.L):   # no clip: the action is the raw action, in bits, everywhere
        assert not clipped.any() and np.array_equal(bits(a), bits(u))
    else:
        assert clipped.any() and not clipped.all(), "some action is clipped and some is not"
        assert np.array_equal(np.abs(a[clipped]), np.full(int(clipped.sum()), f32(case.L)))
    # RN32(sigma * aeps) changes the bits of some unclipped action: u - d is not u there (y itself is not recorded)
    N = u.shape[1]
    srow = np.broadcast_to(sg[0], (N, case.C)) if case.G == 1 else sg[np.arange(N) // (N // case.G)]
    d = (srow[None] * e).astype(f32)
    moved = (~clipped) & (d != 0) & ((u - d).astype(f32) != u)
    assert moved.any()
    assert e.shape == (T, N, case.C) and float(np.abs(e).max()) <= 4.9


@pytest.mark.parametrize("name", gc.NAMES)
def test_cases_without_auto_reset_mean_something(name):
    case, ref = gc.case_of(name), gc.reference_off(name)
    _conditions(ref, case, gc.T_OFF)
    for k in ("pos", "vel", "acc"):
        assert np.isfinite(ref[k]).all(), k
    # another seed gives other actions
    other = gc.reference_off(name, gc.SEED + 1)
    assert not np.array_equal(other["action"], ref["action"])


@pytest.mark.parametrize("name", gc.COVER_NAMES)
def test_cover_cases_without_auto_reset_mean_something(name):
    """The instance-coverage cases (pg_cases.COVER), T = 4: finite, clipped and unclipped actions, a noise that moves
    some unclipped action's bits."""
    case, ref = gc.case_of(name), gc.reference_off(name)
    assert case.t_off == 4 and case.H == 0 and case.G == 1
    _conditions(ref, case, case.t_off)
    for k in ("pos", "vel", "acc"):
        assert np.isfinite(ref[k]).all(), k


@pytest.mark.parametrize("name", gc.COVER_NAMES)
def test_cover_cases_with_auto_reset_mean_something(name):
    """As above with auto-reset, T = 16: every walker resets at least once."""
    case, ref = gc.case_of(name), gc.reference_on(name)
    _conditions(ref, case, gc.T_ON)
    for k in ("pos", "vel", "acc"):
        assert np.isfinite(ref["state"][k]).all(), k
    assert (ref["reset"].sum(0) >= 1).all(), "every walker resets at least once"


def test_edge_inputs_mean_something():
    """The inputs of test_gpu_stochastic_rollout.py's edge tests, on the reference alone.  The largest accepted counters
    (step_base + T = walker_base + N = 2^32) give other variates than the usual ones and a finite run; the sigma with
    zero entries has set 1 all zero and one zero column in every other set, and leaves the run finite."""
    name = gc.ZEROS
    case, base = gc.case_of(name), gc.reference_off(name)
    N = gc.n_walkers(case)
    assert case.wpw == 4 and N % case.wpw == 2, "a half-full last tile"
    edge = gc.reference_off(name, gc.SEED, gc.LAST - case.t_off, gc.LAST - N)
    assert not np.array_equal(bits(edge["eps"]), bits(base["eps"]))
    assert np.array_equal(bits(edge["eps"]), bits(pg.action_noise_numpy(gc.SEED, gc.LAST - case.t_off, case.t_off,
                                                                        gc.LAST - N, N, case.C)))
    edge_on = gc.reference_on(name, gc.LAST - gc.T_ON, gc.LAST - N)
    for ref in (edge, edge_on):
        for k in ("obs", "reward", "action", "raw", "eps"):
            assert np.isfinite(ref[k]).all(), k
    assert not np.array_equal(bits(edge_on["eps"]), bits(gc.reference_on(name)["eps"]))
    sg = gc.sigma_of(name, True)
    assert not sg[1].any() and all((sg[g] == 0).sum() == 1 for g in range(case.G) if g != 1)
    zr = gc.reference_off(name, gc.SEED, gc.STEP_BASE, gc.WALKER_BASE, True)
    for k in ("obs", "reward", "action", "raw", "eps"):
        assert np.isfinite(zr[k]).all(), k
    # step 0 acts on the same rows: the raw action changes where sigma became zero, and nowhere else
    zero = (sg == 0)[np.arange(N) // (N // case.G)]
    moved = bits(zr["raw"][0]) != bits(base["raw"][0])
    assert moved[zero].mean() > 0.9 and not moved[~zero].any()


@pytest.mark.parametrize("name", gc.NAMES)
def test_cases_with_auto_reset_mean_something(name):
    case, cfg, ref = gc.case_of(name), gc.config(name), gc.reference_on(name)
    _conditions(ref, case, gc.T_ON)
    st = ref["state"]
    for k in ("pos", "vel", "acc"):
        assert np.isfinite(st[k]).all(), k
    resets = ref["reset"]
    assert (resets.sum(0) >= 2).all(), "every walker resets at least twice"
    assert resets[:, cfg["sunk"]].all() and resets[-1].any()
    term = (ref["done"] != 0) & (ref["steps"] != cfg["params"]["max_steps"])
    assert term.any() and ((ref["done"] != 0) & ~term).any(), "episodes end by the step limit and by falling"

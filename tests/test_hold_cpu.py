"""The action hold without a GPU: gae_held_numpy against a scalar loop, hold_decide_numpy, the refusals of
wg_rollout_held and wg_gae_held (host pointers, nothing launched), wg_action_hold's layout, and the conditions under
which the GPU cases of tests/hold_cases.py mean something, on the reference engine alone."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import hold_cases as hc
import test_pg_cpu as tp
from walker_gym_amd import _lib, pg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ------------------------------------------------------------------ the numpy restatements
def _gae_held_scalar(hr, v, nvs, dec, term, cut, gamma, lam):
    """The contract, one walker and one float32 operation at a time."""
    T, N = hr.shape
    adv, ret = np.zeros((T, N), f32), np.zeros((T, N), f32)
    g = f32(gamma)
    with np.errstate(all="ignore"):
        gl = f32(g * f32(lam))
        for w in range(N):
            carry, R, nv, cf = f32(0), f32(0), f32(0), False
            for t in range(T - 1, -1, -1):
                if t == T - 1 or dec[t + 1, w] != 0:
                    R = f32(hr[t, w])
                    nv = f32(0) if (term is not None and term[t, w] != 0) else f32(nvs[t, w])
                    cf = cut is not None and cut[t, w] != 0
                if dec[t, w] != 0:
                    delta = f32(f32(R + f32(g * nv)) - f32(v[t, w]))
                    c = f32(0) if cf else carry
                    carry = f32(delta + f32(gl * c))
                    adv[t, w] = carry
                    ret[t, w] = f32(carry + f32(v[t, w]))
    return adv, ret


def _gae_inputs(T, N, seed):
    rng = np.random.default_rng(seed)
    hr, v, nv = (rng.standard_normal((T, N)).astype(f32) for _ in range(3))
    dec = (rng.random((T, N)) < 1 / 3).astype(np.uint8)
    term = (rng.random((T, N)) < 0.3).astype(np.uint8)     # on closing and on non-closing steps alike
    cut = (rng.random((T, N)) < 0.3).astype(np.uint8)
    return hr, v, nv, dec, term, cut


def _same_with_nan(a, b):
    a, b = np.asarray(a, f32), np.asarray(b, f32)
    both = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.where(both, 0, bits(a)), np.where(both, 0, bits(b)))


@pytest.mark.parametrize("T", [1, 2, 9])
def test_gae_held_numpy_equals_scalar_loop(T):
    N = 12
    hr, v, nv, dec, term, cut = _gae_inputs(T, N, 10 + T)
    dec[:, 0] = 0                                   # a walker with no decision
    dec[:, 1] = 0; dec[T - 1, 1] = 1                # a decision only at the last step
    dec[0, 2] = 0                                   # an undecided first step
    if T > 1:
        dec[1, 2] = 1
        dec[:, 3] = 0; dec[0, 3] = 1                # one hold over the whole call
        term[:, 3] = 1; cut[:, 3] = 1; term[T - 1, 3] = 0; cut[T - 1, 3] = 0    # flags on non-closing steps only
        dec[:, 4] = 1; term[:, 4] = 1; cut[:, 4] = 1                             # ... and on every closing step
    hr[0, 5] = np.nan                               # a NaN
    nv[T - 1, 6] = np.inf
    for tm, ct in ((term, cut), (None, cut), (term, None), (None, None)):
        want = _gae_held_scalar(hr, v, nv, dec, tm, ct, 0.97, 0.9)
        got = pg.gae_held_numpy(hr, v, nv, dec, tm, ct, 0.97, 0.9)
        assert _same_with_nan(got[0], want[0]) and _same_with_nan(got[1], want[1])
        assert not got[0][:, 0].any() and not got[1][:, 0].any()
        assert not got[0][:T - 1, 1].any() and got[0][T - 1, 1] != 0
        assert got[0][0, 2] == 0 and got[1][0, 2] == 0
    if T > 1:   # flags on non-closing steps are not read
        a = pg.gae_held_numpy(hr, v, nv, dec, term, cut, 0.97, 0.9)[0][:, 3]
        b = pg.gae_held_numpy(hr, v, nv, dec, None, None, 0.97, 0.9)[0][:, 3]
        assert np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("T", [1, 2, 9])
def test_gae_held_numpy_with_all_ones_equals_gae_numpy(T):
    hr, v, nv, _, term, cut = _gae_inputs(T, 17, 20 + T)
    ones = np.ones((T, 17), np.uint8)
    for tm, ct in ((term, cut), (None, None)):
        a, r = pg.gae_held_numpy(hr, v, nv, ones, tm, ct, 0.99, 0.95)
        a0, r0 = pg.gae_numpy(hr, v, nv, tm, ct, 0.99, 0.95)
        assert np.array_equal(bits(a), bits(a0)) and np.array_equal(bits(r), bits(r0))


@pytest.mark.parametrize("every", [1, 2, 3, 7])
def test_hold_decide_numpy(every):
    steps = np.array([0, every - 1, every, 2 * every, 2 * every + 1, (1 << 31) - 1], np.int32)
    want = [1, int(every == 1), 1, 1, int(every == 1), int(((1 << 31) - 1) % every == 0)]
    assert pg.hold_decide_numpy(steps, every).tolist() == want
    assert pg.hold_decide_numpy(steps, every).dtype == np.uint8
    assert pg.hold_decide_numpy(np.array([-1], np.int32), 5).tolist() == [int(((1 << 32) - 1) % 5 == 0)]   # as uint32
    with pytest.raises(ValueError):
        pg.hold_decide_numpy(steps, 0)


def test_package_index():
    import walker_gym_amd as wg
    from walker_gym_amd.batched_env import BatchedPhysicsEnv
    assert wg.gae_held is pg.gae_held and wg.gae_held_numpy is pg.gae_held_numpy
    assert wg.hold_decide_numpy is pg.hold_decide_numpy and wg.rollout_held is BatchedPhysicsEnv.rollout_held


# ------------------------------------------------------------------ the C boundary: wg_rollout_held
def _hold(**kw):
    d = dict(every=2)
    d.update(kw)
    return _lib.WgActionHold(**d)


def _held(lib, b, p, pol, nm, nz, hold, st, o, n_steps):
    ref = lambda x: None if x is None else C.byref(x)
    return lib.wg_rollout_held(C.byref(b), C.byref(p), ref(pol), ref(nm), ref(nz), ref(hold), ref(o), ref(st), n_steps,
                               None)


def _nm():
    return _lib.WgObsNorm(mean=64, scale=64, clip=1.5)


def _run_row(lib, mode, noise_on, norm_on, what, batch, pol, noise, stats, out, steps, word, hold=None):
    params = dict(tp.AR if mode == "ar" else tp.OFF)
    if what == "auto_reset bits":
        params["auto_reset"] = 4
    if mode == "ar":
        st = None if stats is tp._NONE else _lib.WgEpisodeStats(**stats)
    else:
        st = _lib.WgEpisodeStats() if what == "stats without auto-reset" else None
    nz = tp._nz(**noise) if noise_on else None
    rc = _held(lib, tp._batch(**batch), _lib.WgParams(**params), None if pol is None else tp._pol(**pol),
               _nm() if norm_on else None, nz, _hold() if hold is None else hold, st,
               None if out is None else _lib.WgOutputs(**out), steps)
    assert rc == _lib.WG_EINVAL, what
    msg = lib.wg_last_error()
    assert word in msg, (what, msg)


# the existing entries' tables, by import (as tests/test_norm_cpu.py takes them): the rows about the noise itself need a
# noise, since a NULL one is the deterministic form here
_NOISE_ROWS = {"null noise", "null sigma", "raw_out stride", "eps_out stride", "eps_out stride with fewer columns",
               "step_base wraps", "walker_base wraps"}
_DET = [r for r in tp.BOTH_MODES if r[0] not in _NOISE_ROWS]
_NZ = [r for r in tp.BOTH_MODES if r[0] != "null noise"]
FORMS = pytest.mark.parametrize("noise_on,norm_on", [(False, False), (True, False), (False, True), (True, True)],
                                ids=["det", "nz", "on", "nz-on"])


@pytest.mark.parametrize("mode", ["off", "ar"])
@pytest.mark.parametrize("norm_on", [False, True])
@pytest.mark.parametrize("row", _DET, ids=[r[0] for r in _DET])
def test_held_refuses_what_the_deterministic_entries_refuse(lib, mode, norm_on, row):
    _run_row(lib, mode, False, norm_on, *row)


@pytest.mark.parametrize("mode", ["off", "ar"])
@pytest.mark.parametrize("norm_on", [False, True])
@pytest.mark.parametrize("row", _NZ, ids=[r[0] for r in _NZ])
def test_held_refuses_what_the_stochastic_entry_refuses(lib, mode, norm_on, row):
    _run_row(lib, mode, True, norm_on, *row)


@FORMS
@pytest.mark.parametrize("row", tp.OFF_ONLY, ids=[r[0] for r in tp.OFF_ONLY])
def test_held_einval_without_auto_reset(lib, row, noise_on, norm_on):
    _run_row(lib, "off", noise_on, norm_on, *row)


@FORMS
@pytest.mark.parametrize("row", tp.AR_ONLY, ids=[r[0] for r in tp.AR_ONLY])
def test_held_einval_with_auto_reset(lib, row, noise_on, norm_on):
    _run_row(lib, "ar", noise_on, norm_on, *row)


@FORMS
@pytest.mark.parametrize("mode", ["off", "ar"])
def test_held_refuses_a_bad_normaliser(lib, mode, noise_on, norm_on):
    """(a NULL nm is no normaliser; one that is given is checked as wg_rollout_normalized checks it)"""
    params = _lib.WgParams(**(tp.AR if mode == "ar" else tp.OFF))
    st = _lib.WgEpisodeStats() if mode == "ar" else None
    for nm, word in ((_lib.WgObsNorm(scale=64, clip=1.5), b"null mean"), (_lib.WgObsNorm(mean=64, clip=1.5), b"null scale"),
                     (_lib.WgObsNorm(mean=64, scale=64, clip=0.0), b"clip"),
                     (_lib.WgObsNorm(mean=64, scale=64, clip=float("nan")), b"clip")):
        rc = _held(lib, tp._batch(), params, tp._pol(), nm, tp._nz() if noise_on else None, _hold(), st, None, 1)
        assert rc == _lib.WG_EINVAL and word in lib.wg_last_error(), word


N0, C0 = 128, 8      # tp._batch's walkers, tp._pol's columns


@FORMS
@pytest.mark.parametrize("mode", ["off", "ar"])
def test_held_refuses_a_bad_hold(lib, mode, noise_on, norm_on):
    ok = ("x", {}, {}, {}, {}, None, 1)
    rows = [(_hold(every=0), b"every"), (_hold(every=-3), b"every"),
            (_hold(decided_out=64, decided_out_step=N0 - 1), b"decided_out_step"),
            (_hold(hold_reward_out=64, hold_reward_out_step=N0 - 1), b"hold_reward_out_step"),
            (_hold(decided_out=64, decided_out_step=0), b"decided_out_step")]
    for hold, word in rows:
        _run_row(lib, mode, noise_on, norm_on, *ok, word, hold=hold)
    params = _lib.WgParams(**(tp.AR if mode == "ar" else tp.OFF))
    st = _lib.WgEpisodeStats() if mode == "ar" else None
    rc = _held(lib, tp._batch(), params, tp._pol(), _nm() if norm_on else None, tp._nz() if noise_on else None, None, st,
               None, 1)
    assert rc == _lib.WG_EINVAL and b"null action hold" in lib.wg_last_error()
    b = tp._batch()
    assert lib.wg_rollout_held(C.byref(b), None, C.byref(tp._pol()), None, None, C.byref(_hold()), None, None, 1,
                               None) == _lib.WG_EINVAL and b"null params" in lib.wg_last_error()


@pytest.mark.parametrize("mode", ["off", "ar"])
def test_held_refuses_held_rows_that_alias_an_output(lib, mode):
    """`held` against every other output of the call: the same address, and one shared element at either end."""
    T = 3
    arena = np.zeros(1 << 16, f32)
    held_at = arena[32768:].ctypes.data                 # held: [N0][C0 + 1] floats from here
    held_bytes = N0 * (C0 + 1) * 4
    params = _lib.WgParams(**(tp.AR if mode == "ar" else tp.OFF))

    def call(pol=None, noise=None, hold=None, out=None, stats=None):
        st = _lib.WgEpisodeStats(**(stats or {})) if mode == "ar" else None
        return _held(lib, tp._batch(), params, tp._pol(**(pol or {})), None, tp._nz(**noise) if noise else None,
                     _hold(held=held_at, **(hold or {})), st, None if out is None else _lib.WgOutputs(**out), T)

    def cases(size):   # (the other buffer's address): the same start, its last element on held's first, its first on held's last
        return (held_at, held_at - size + 4, held_at + held_bytes - 4)

    def misses(size):  # ... and just clear of held at either end: no refusal for aliasing
        return (held_at - size, held_at + held_bytes)

    per = lambda row, elem: ((T - 1) * row + row) * elem
    rows = [("action_out", lambda a: dict(pol=dict(action_out=a, action_out_step=N0 * C0)), per(N0 * C0, 4)),
            ("raw_out", lambda a: dict(noise=dict(raw_out=a, raw_out_step=N0 * C0)), per(N0 * C0, 4)),
            ("eps_out", lambda a: dict(noise=dict(eps_out=a, eps_out_step=N0 * C0)), per(N0 * C0, 4)),
            ("decided_out", lambda a: dict(hold=dict(decided_out=a, decided_out_step=N0)), per(N0, 1)),
            ("hold_reward_out", lambda a: dict(hold=dict(hold_reward_out=a, hold_reward_out_step=N0)), per(N0, 4)),
            ("obs", lambda a: dict(out=dict(obs=a, obs_stride=152, obs_step=N0 * 152, out_step=N0)), per(N0 * 152, 4)),
            ("reward", lambda a: dict(out=dict(reward=a, out_step=N0)), per(N0, 4)),
            ("done", lambda a: dict(out=dict(done=a, out_step=N0)), per(N0, 1)),
            ("steps", lambda a: dict(out=dict(steps=a, out_step=N0)), per(N0, 4))]
    if mode == "ar":
        rows += [("reset", lambda a: dict(out=dict(reset=a, out_step=N0)), per(N0, 1)),
                 ("final_obs", lambda a: dict(out=dict(final_obs=a, obs_stride=152, obs_step=N0 * 152, out_step=N0)),
                  per(N0 * 152, 4)),
                 ("return_sum", lambda a: dict(stats=dict(return_sum=a)), N0 * 4),
                 ("tail_length", lambda a: dict(stats=dict(tail_length=a)), N0 * 4),
                 ("ep_return", lambda a: dict(stats=dict(ep_return=a, ep_slots=2)), N0 * 2 * 4)]
    else:
        rows += [("return_out", lambda a: dict(pol=dict(return_out=a)), N0 * 4),
                 ("length_out", lambda a: dict(pol=dict(length_out=a)), N0 * 4)]
    for name, make, size in rows:
        for at in cases(size):
            assert call(**make(at)) == _lib.WG_EINVAL, name
            assert b"held aliases " + name.encode() in lib.wg_last_error(), (name, lib.wg_last_error())


def test_held_other_refusals_and_the_lds_rule_with_one_more_word(lib, monkeypatch):
    b, pol = tp._batch(), tp._pol()
    for kw in (dict(spring_mode=1), dict(pair_mode=1)):
        assert _held(lib, b, _lib.WgParams(**dict(tp.OFF, **kw)), pol, None, None, _hold(), None, None, 1) == _lib.WG_EINVAL
        assert b"lean kernel" in lib.wg_last_error() and b"wg_rollout_held" in lib.wg_last_error()
    # the 80 KiB rule (tests/test_pg_cpu.py's arithmetic: 80 KiB exactly with four words per walker): the hold's word,
    # rounded up to 16 bytes per wave, passes it where the existing entry still fits
    M, A = 64, 64
    D = 3 * 3 * M + A
    a16 = lambda n: (n + 15) & ~15

    def lds(K, H, words):
        pl = (K + 3) & ~3
        sl = a16(pl * 24) + a16(pl * 12) + a16(K * 4 + 4) + a16(A * 4)
        return 4 * (sl + a16(D * 4) + a16(H * 4) + a16(A * 4) + 4 * words)
    K, H = next((K, H) for K in range(64, 513) for H in range(4, 257, 4) if lds(K, H, 4) == 80 * 1024)
    big = tp._batch(N=8192, M=M, K=K, A=A)
    wide = tp._pol(obs_dim=D, hidden=H, w1=64, act_dim=A)
    for nz in (None, tp._nz()):
        assert _held(lib, big, _lib.WgParams(**tp.OFF), wide, None, nz, _hold(), None, None, 1) == _lib.WG_ERANGE
        assert b"LDS" in lib.wg_last_error() and str(80 * 1024 + 4 * 16).encode() in lib.wg_last_error()
    monkeypatch.setenv("WG_LEAN", "0")
    assert _held(lib, b, _lib.WgParams(**tp.OFF), pol, None, None, _hold(), None, None, 1) == _lib.WG_EINVAL
    assert b"lean kernel" in lib.wg_last_error()


# ------------------------------------------------------------------ the C boundary: wg_gae_held
def _gae_held(lib, T=4, N=8, stride=None, gamma=0.99, lam=0.95, **ptr):
    a = {k: np.zeros((T, stride or N), f32) for k in ("hold_reward", "value", "next_value", "adv", "ret")}
    a.update({k: np.zeros((T, stride or N), np.uint8) for k in ("decided", "term", "cut")})
    a.update(ptr)
    p = lambda x: None if x is None else C.c_void_p(x if isinstance(x, int) else x.ctypes.data)
    return lib.wg_gae_held(p(a["hold_reward"]), p(a["value"]), p(a["next_value"]), p(a["decided"]), p(a["term"]),
                           p(a["cut"]), T, N, N if stride is None else stride, gamma, lam, p(a["adv"]), p(a["ret"]), None)


def test_gae_held_einval_table(lib):
    for name in ("hold_reward", "value", "next_value", "decided", "adv"):
        assert _gae_held(lib, **{name: None}) == _lib.WG_EINVAL and name.encode() in lib.wg_last_error(), name
    for kw, word in ((dict(T=0), b"n_steps"), (dict(N=0, stride=8), b"N 0"), (dict(stride=7), b"step_stride"),
                     (dict(gamma=float("nan")), b"gamma"), (dict(gamma=float("inf")), b"gamma"),
                     (dict(lam=float("nan")), b"lam"), (dict(lam=float("-inf")), b"lam")):
        assert _gae_held(lib, **kw) == _lib.WG_EINVAL and word in lib.wg_last_error(), (kw, lib.wg_last_error())
    base = np.zeros((9, 8), f32)
    for out in ("adv", "ret"):
        for inp in ("hold_reward", "value", "next_value"):
            for o_, i_ in ((base[:4], base[:4]), (base[:4], base[3:7].reshape(-1)[7:]), (base[4:8], base.reshape(-1)[1:])):
                rc = _gae_held(lib, **{out: o_.ctypes.data, inp: i_.ctypes.data})
                assert rc == _lib.WG_EINVAL and b"aliases" in lib.wg_last_error(), (out, inp)
        flags = np.zeros(9 * 8 * 4, np.uint8)
        for inp in ("decided", "term", "cut"):   # one shared byte
            rc = _gae_held(lib, **{out: flags.ctypes.data, inp: flags.ctypes.data + 4 * 32 - 1})
            assert rc == _lib.WG_EINVAL and b"aliases " + inp.encode() in lib.wg_last_error(), (out, inp)
    rc = _gae_held(lib, adv=base[:4].ctypes.data, ret=base[3:7].ctypes.data)
    assert rc == _lib.WG_EINVAL and b"aliases" in lib.wg_last_error()


# ------------------------------------------------------------------ the ABI
def test_wg_action_hold_matches_header_and_abi_stays_16(lib, tmp_path):
    fields = [f for f, _ in _lib.WgActionHold._fields_]
    lines = "".join(f'  printf("{f} %zu\\n", offsetof(wg_action_hold, {f}));\n' for f in fields)
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "walker_hip.h"\nint main(void) {\n' + lines +
                     '  printf("sizeof %zu\\n", sizeof(wg_action_hold));\n  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(probe)], check=True)
    got = dict(line.rsplit(" ", 1) for line in
               subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().splitlines())
    assert int(got["sizeof"]) == C.sizeof(_lib.WgActionHold) == 48
    for f in fields:
        assert getattr(_lib.WgActionHold, f).offset == int(got[f]), f
    assert _lib.ABI_VERSION == 16 and lib.wg_abi_version() == 16
    hdr = open(os.path.join(ROOT, "include", "walker_hip.h")).read()
    assert "#define WG_ABI_VERSION 16" in hdr and "ONE more word per walker" in hdr
    new = {"wg_rollout_held", "wg_gae_held"}
    assert new <= set(_lib.EXPORTS)
    for name in new:
        assert getattr(lib, name) is not None


# ------------------------------------------------------------------ the GPU cases mean something
@pytest.mark.parametrize("name", hc.NAMES)
def test_the_gpu_cases_meet_their_conditions_on_the_reference_engine(name):
    """With auto-reset and the noise on: every run finite; closed holds of every length 1 .. every; at least 10 % of them
    cut short and at least 10 % full; 40 % (every 2) / 60 % (every 3) of the walkers enter inside a hold; the final
    positions differ in bits from the every = 1 run; where a wave holds several walkers, at least half of its tile-steps
    have a deciding and a holding walker side by side."""
    case = hc.case_of(name)
    base = hc.reference(name, True, True, 1)
    assert base["decided"].all()
    for every in hc.EVERY:
        r = hc.reference(name, True, True, every)
        for k in ("obs", "reward", "action", "hold_reward", "held"):
            assert np.isfinite(r[k]).all(), (every, k)
        assert all(np.isfinite(r["state"][k]).all() for k in ("pos", "vel", "acc"))
        counts = hc.closed_holds(r["decided"], every)
        assert (counts > 0).all(), counts
        short, full = counts[:-1].sum() / counts.sum(), counts[-1] / counts.sum()
        assert short >= 0.1 and full >= 0.1, counts
        mid = 1.0 - r["decided"][0].mean()
        assert math.isclose(mid, {2: 0.4, 3: 0.6}[every], abs_tol=0.005), mid
        if case.params.get("action_mode") == 1:
            # Discrete actions read `a != 0`, and the policy's outputs are never exactly zero: a hold changes a step only
            # where the action in force came from `held` (half of those are +0.0).  With max_steps = 5 every walker is
            # reset after that, so with auto-reset the difference is in the recorded rows and gone from the final state;
            # without auto-reset it stays.
            assert not np.array_equal(bits(r["obs"]), bits(base["obs"]))
            off, off1 = hc.reference(name, False, True, every), hc.reference(name, False, True, 1)
            assert not np.array_equal(bits(off["state"]["pos"]), bits(off1["state"]["pos"]))
        else:
            assert not np.array_equal(bits(r["state"]["pos"]), bits(base["state"]["pos"]))
        if case.wpw > 1:
            assert hc.mixed_tile_steps(r["decided"], case.wpw) >= 0.5
        # what the sentinel rows and the entry rows are there for
        assert (r["raw"][r["decided"] == 0] == hc.SENTINEL).all() and (r["raw"][r["decided"] != 0] != hc.SENTINEL).all()


@pytest.mark.parametrize("name,closed", [("canonical4-h5-5sets", {2: [6384, 11366], 3: [286, 5685, 5279]}),
                                         ("balance-h5-4sets", {2: [324, 548], 3: [28, 275, 255]})])
def test_the_recorded_hold_counts(name, closed):
    """The closed holds by length of the two cases whose counts are on record."""
    for every, want in closed.items():
        assert hc.closed_holds(hc.reference(name, True, True, every)["decided"], every).tolist() == want


@pytest.mark.parametrize("name", hc.NAMES)
def test_the_other_modes_stay_finite_and_enter_mid_hold(name):
    """Auto-reset off with and without the noise, auto-reset on without it: finite, and the same shares of walkers that
    take their first action from `held`."""
    for auto_reset, noise in ((False, False), (False, True), (True, False)):
        for every in hc.EVERY:
            r = hc.reference(name, auto_reset, noise, every)
            for k in ("obs", "reward", "action", "hold_reward"):
                assert np.isfinite(r[k]).all(), (auto_reset, noise, every, k)
            assert math.isclose(1.0 - r["decided"][0].mean(), {2: 0.4, 3: 0.6}[every], abs_tol=0.005)
            assert np.array_equal(bits(r["action"][0][r["decided"][0] == 0]),
                                  bits(hc.held_of(name)[:, :-1][r["decided"][0] == 0]))

"""Observation normalisation without a GPU: the numpy restatements of walker_gym_amd.normalize against scalar
pure-Python loops, the identity normaliser, the statistics against numpy's, the refusals of the five new calls at the C
boundary (host pointers: every call here is refused before a launch, or launches nothing), wg_obs_norm's layout, and
the conditions that make the GPU cases of tests/norm_cases.py mean something, on the reference engine alone."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import norm_cases as nc
import policy_cases as pc
import test_pg_cpu as tp
import test_policy_rows_cpu as tr
from walker_gym_amd import _lib, build, pg
from walker_gym_amd.normalize import ObsNorm, normalize_numpy, obs_moments_numpy, obs_norm_finish_numpy
from walker_gym_amd.policy import MLPPolicy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


# ------------------------------------------------------------------ the restatements against scalar loops
def _normalize_scalar(x, mean, scale, clip):
    out = np.empty_like(x)
    c = f32(clip)
    with np.errstate(all="ignore"):
        for idx in np.ndindex(x.shape):
            v = f32(f32(x[idx] - mean[idx[-1]]) * scale[idx[-1]])
            out[idx] = -c if v < -c else (c if v > c else v)
    return out


def _moments_scalar(x, mask, bound, chunk_rows, state):
    """The header's loop, one Python float (a float64) at a time."""
    R, D = x.shape
    st = [0.0] * (1 + 2 * D) if state is None else [float(v) for v in state]
    for lo in range(0, R, chunk_rows):
        c, P1, P2 = 0.0, [0.0] * D, [0.0] * D
        for r in range(lo, min(R, lo + chunk_rows)):
            if mask is not None and not mask[r]:
                continue
            if not all(abs(float(v)) < float(f32(bound)) for v in x[r]):    # (a NaN compares false)
                continue
            c += 1.0
            for i in range(D):
                v = float(x[r, i])
                P1[i] = P1[i] + v
                P2[i] = P2[i] + v * v          # (exact: 24-bit factors)
        st[0] += c
        for i in range(D):
            st[1 + i] += P1[i]
            st[1 + D + i] += P2[i]
    return np.array(st, f64)


def _finish_scalar(st, eps):
    D = (len(st) - 1) // 2
    n = float(st[0])
    if not n > 0:
        return None
    mean, scale = np.empty(D, f32), np.empty(D, f32)
    for i in range(D):
        m = float(st[1 + i]) / n
        var = float(st[1 + D + i]) / n - m * m
        var = var if var > 0 else 0.0
        mean[i] = f32(m)
        scale[i] = f32(1.0 / math.sqrt(var + eps))
    return mean, scale


def _rows(R, D, seed, bound):
    """R rows of D values at mixed magnitudes with a NaN row, an inf row, a row with one value exactly at the bound
    (left out: the test is |x| < bound), one just below it (used), and a mask that drops a tenth."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((R, D)) * rng.choice([1.0, 30.0, 2000.0], (1, D))).astype(f32)
    x = np.clip(x, -0.9 * bound, 0.9 * bound).astype(f32)
    x[1, D // 2] = np.nan
    x[3, 0] = np.inf
    x[5, D - 1] = f32(bound)
    x[6, D - 1] = np.nextafter(f32(bound), f32(0))
    x[7, 0] = f32(-0.0)
    mask = (rng.random(R) > 0.1).astype(np.uint8)
    mask[[1, 3, 5, 6]] = 1
    return x, mask


@pytest.mark.parametrize("chunk_rows", [1, 3, 1000])
@pytest.mark.parametrize("D", [1, 26, 155])
def test_moments_numpy_equals_scalar_loop(D, chunk_rows):
    bound = 5000.0
    x, mask = _rows(40, D, 7 + D, bound)
    for m in (None, mask):
        got = obs_moments_numpy(x, m, bound, chunk_rows)
        want = _moments_scalar(x, m, bound, chunk_rows, None)
        assert got.dtype == f64 and np.array_equal(bits(got), bits(want))
        n_left = 3 + (0 if m is None else int((m == 0).sum()))      # the NaN, the inf and the at-bound row
        assert got[0] == 40 - n_left
        # a second update continues the state
        again = obs_moments_numpy(x[::-1], None if m is None else m[::-1], bound, chunk_rows, state=got)
        assert np.array_equal(bits(again), bits(_moments_scalar(x[::-1], None if m is None else m[::-1], bound,
                                                                chunk_rows, want)))
        for st in (got, again):
            fin, ref = obs_norm_finish_numpy(st, 1e-8), _finish_scalar(st, 1e-8)
            assert np.array_equal(bits(fin[0]), bits(ref[0])) and np.array_equal(bits(fin[1]), bits(ref[1]))
    # [T, N, D] with a [T, N] mask is the flat rows
    assert np.array_equal(bits(obs_moments_numpy(x.reshape(5, 8, D), mask.reshape(5, 8), bound, chunk_rows)),
                          bits(obs_moments_numpy(x, mask, bound, chunk_rows)))
    # bound = inf takes the at-bound rows too, never the NaN or the inf row
    assert obs_moments_numpy(x, None, math.inf, chunk_rows)[0] == 38


@pytest.mark.parametrize("chunk_rows", [1, 3, 8])
def test_two_half_updates_equal_one_when_the_halves_are_chunk_aligned(chunk_rows):
    x, mask = _rows(48, 26, 3, 5000.0)
    whole = obs_moments_numpy(x, mask, 5000.0, chunk_rows)
    half = obs_moments_numpy(x[24:], mask[24:], 5000.0, chunk_rows,
                             state=obs_moments_numpy(x[:24], mask[:24], 5000.0, chunk_rows))
    assert 24 % chunk_rows == 0 and np.array_equal(bits(whole), bits(half))
    # halves that split a chunk add in another order: the same count, and sums within rounding only
    other = obs_moments_numpy(x[25:], mask[25:], 5000.0, 8, state=obs_moments_numpy(x[:25], mask[:25], 5000.0, 8))
    assert other[0] == obs_moments_numpy(x, mask, 5000.0, 8)[0]


def test_no_used_row_leaves_the_outputs_alone():
    x = np.full((4, 3), np.nan, f32)
    st = obs_moments_numpy(x, None, math.inf, 2)
    assert np.array_equal(st, np.zeros(7)) and obs_norm_finish_numpy(st, 1e-8) is None
    st = obs_moments_numpy(np.ones((4, 3), f32), np.zeros(4, np.uint8), math.inf, 2)
    assert st[0] == 0 and obs_norm_finish_numpy(st, 1e-8) is None
    with pytest.raises(ValueError):
        obs_moments_numpy(x, None, math.inf, 0)


@pytest.mark.parametrize("D", [1, 26, 155])
def test_normalize_numpy_equals_scalar_loop(D):
    rng = np.random.default_rng(D)
    x = (rng.standard_normal((9, D)) * 100).astype(f32)
    mean, scale = (rng.standard_normal(D) * 50).astype(f32), rng.uniform(0.001, 0.1, D).astype(f32)
    x[0, 0], x[1, 0], x[2, 0] = np.nan, np.inf, -np.inf
    x[3, D - 1] = mean[D - 1] + f32(1.5) / scale[D - 1]
    for clip in (1.5, math.inf):
        got = normalize_numpy(x, mean, scale, clip)
        assert got.dtype == f32 and np.array_equal(bits(got), bits(_normalize_scalar(x, mean, scale, clip)))
    got = normalize_numpy(x, mean, scale, 1.5)
    assert np.isnan(got[0, 0]) and got[1, 0] == 1.5 and got[2, 0] == -1.5 and np.nanmax(np.abs(got)) == 1.5
    # [T, N, D] rows broadcast alike
    assert np.array_equal(bits(normalize_numpy(x.reshape(3, 3, D), mean, scale, 1.5).reshape(9, D)), bits(got))


def test_statistics_against_numpy_on_small_integer_rows():
    """Small integers: every sum is exact in float64, so mean and scale are numpy's within the float32 rounding of the
    outputs (and the float64 rounding of the variance's subtraction, far below it)."""
    rng = np.random.default_rng(2)
    x = rng.integers(-40, 41, (500, 12)).astype(f32)
    x[:, 3] = 7.0                                  # a zero-variance column
    st = obs_moments_numpy(x, None, math.inf, 64)
    assert np.array_equal(st[1:13], x.astype(f64).sum(0)) and np.array_equal(st[13:], (x.astype(f64) ** 2).sum(0))
    mean, scale = obs_norm_finish_numpy(st, 1e-8)
    m, s = x.astype(f64).mean(0), x.astype(f64).std(0)
    assert np.all(np.abs(mean - m) <= np.abs(m) * 2.0 ** -24)
    want = 1.0 / np.sqrt(s * s + 1e-8)
    assert np.all(np.abs(scale - want) <= want * 2.0 ** -22)
    assert mean[3] == 7.0 and scale[3] == f32(1e4)


# ------------------------------------------------------------------ the policy with a normaliser
def _policy(H, G, nm, seed=0):
    rng = np.random.default_rng(seed)
    D, Cc = nm.D if nm is not None else 26, 3
    import torch
    t = lambda *s: torch.from_numpy((rng.standard_normal(s) * 0.3).astype(f32))
    n2 = H or D
    w1, b1 = (t(G, D, H), t(G, H)) if H else (None, None)
    return MLPPolicy(t(G, n2, Cc), t(G, Cc), w1, b1, act_limit=1.0, obs_norm=nm)


@pytest.mark.parametrize("H,G", [(0, 1), (5, 1), (5, 4)])
def test_identity_normaliser_gives_the_plain_policy_bits(H, G):
    import torch
    rng = np.random.default_rng(4)
    x = (rng.standard_normal((8, 26)) * 50).astype(f32)
    x[0, 0], x[1, 1] = f32(-0.0), f32(0.0)
    nm = ObsNorm(26, "cpu", clip=math.inf)
    assert nm.count == 0 and float(nm.mean.abs().max()) == 0 and float(nm.scale.min()) == 1
    norm, plain = _policy(H, G, nm, 1), _policy(H, G, None, 1)
    assert np.array_equal(bits(norm.forward_numpy(x)), bits(plain.forward_numpy(x)))
    assert np.array_equal(bits(normalize_numpy(x, nm.mean.numpy(), nm.scale.numpy(), math.inf)), bits(x))   # -0.0 stays
    if G == 1:   # the torch restatement: sub, mul, clamp, then the same layers
        assert np.array_equal(bits(norm(torch.from_numpy(x)).numpy()), bits(plain.forward_numpy(x)))
    # pg's restatements honour the normaliser the same way
    x3 = x.reshape(2, 4, 26)
    assert np.array_equal(bits(pg.policy_rows_numpy(norm, x3)), bits(pg.policy_rows_numpy(plain, x3)))
    dy = rng.standard_normal((2, 4, 3)).astype(f32)
    for a, b in zip(pg.policy_grad_numpy(norm, x3, dy, chunk_rows=3), pg.policy_grad_numpy(plain, x3, dy, chunk_rows=3)):
        assert (a is None and b is None) or np.array_equal(bits(a), bits(b))


def test_a_real_normaliser_is_applied_first_and_seen_in_place():
    import torch
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((6, 26)) * 50 + 20).astype(f32)
    nm = ObsNorm(26, "cpu", clip=1.5)
    pol, plain = _policy(5, 1, nm, 2), _policy(5, 1, None, 2)
    mean, scale = (rng.standard_normal(26) * 20).astype(f32), rng.uniform(0.01, 0.05, 26).astype(f32)
    nm.mean.copy_(torch.from_numpy(mean)); nm.scale.copy_(torch.from_numpy(scale))     # in place: no re-wrap
    xn = normalize_numpy(x, mean, scale, 1.5)
    assert (np.abs(xn) == 1.5).any() and (np.abs(xn) < 1.5).any()
    want = plain.forward_numpy(xn)
    assert np.array_equal(bits(pol.forward_numpy(x)), bits(want))
    assert np.array_equal(bits(pol(torch.from_numpy(x)).numpy()), bits(want))
    assert not np.array_equal(bits(want), bits(plain.forward_numpy(x)))
    u, a, e = pg.stochastic_forward_numpy(pol, x, 0.1, 5, 0)
    u2, a2, e2 = pg.stochastic_forward_numpy(plain, xn, 0.1, 5, 0)
    assert np.array_equal(bits(u), bits(u2)) and np.array_equal(bits(a), bits(a2))
    # the weight gradients take xn as their left factor
    dy = rng.standard_normal((1, 6, 3)).astype(f32)
    for g, h in zip(pg.policy_grad_numpy(pol, x[None], dy), pg.policy_grad_numpy(plain, xn[None], dy)):
        assert np.array_equal(bits(g), bits(h))
    # state_dict round trip, and the refusals of the constructor
    other = ObsNorm(26, "cpu")
    other.load_state_dict(nm.state_dict())
    assert other.clip == 1.5 and np.array_equal(other.mean.numpy(), mean) and np.array_equal(other.scale.numpy(), scale)
    for kw in (dict(clip=0.0), dict(clip=float("nan")), dict(eps=-1.0), dict(bound=0.0)):
        with pytest.raises(ValueError):
            ObsNorm(26, "cpu", **kw)
    with pytest.raises(ValueError):
        ObsNorm(0, "cpu")
    with pytest.raises(ValueError):
        MLPPolicy(torch.zeros(26, 3), obs_norm=ObsNorm(25, "cpu"))


def test_package_index():
    import walker_gym_amd as wg
    assert wg.ObsNorm is ObsNorm and wg.normalize.obs_moments_numpy is obs_moments_numpy


# ------------------------------------------------------------------ the C boundary: wg_rollout_normalized
def _nm(**kw):
    d = dict(mean=64, scale=64, clip=1.5)
    d.update(kw)
    return _lib.WgObsNorm(**d)


def _normalized(lib, b, p, pol, nm, nz, st, o, n_steps):
    ref = lambda x: None if x is None else C.byref(x)
    return lib.wg_rollout_normalized(C.byref(b), C.byref(p), ref(pol), ref(nm), ref(nz), ref(o), ref(st), n_steps, None)


def _run_row(lib, mode, noise_on, what, batch, pol, noise, stats, out, steps, word, nm=None):
    params = dict(tp.AR if mode == "ar" else tp.OFF)
    if what == "auto_reset bits":
        params["auto_reset"] = 4
    if mode == "ar":
        st = None if stats is tp._NONE else _lib.WgEpisodeStats(**stats)
    else:
        st = _lib.WgEpisodeStats() if what == "stats without auto-reset" else None
    nz = tp._nz(**noise) if noise_on else None
    rc = _normalized(lib, tp._batch(**batch), _lib.WgParams(**params), None if pol is None else tp._pol(**pol),
                     _nm() if nm is None else nm, nz, st, None if out is None else _lib.WgOutputs(**out), steps)
    assert rc == _lib.WG_EINVAL, what
    msg = lib.wg_last_error()
    assert word in msg, (what, msg)


# the existing entries' tables, by import: the rows about the noise itself need a noise (a NULL one is the deterministic
# mode here, not a refusal)
_NOISE_ROWS = {"null noise", "null sigma", "raw_out stride", "eps_out stride", "eps_out stride with fewer columns",
               "step_base wraps", "walker_base wraps"}
_DET = [r for r in tp.BOTH_MODES if r[0] not in _NOISE_ROWS]
_NZ = [r for r in tp.BOTH_MODES if r[0] != "null noise"]


@pytest.mark.parametrize("mode", ["off", "ar"])
@pytest.mark.parametrize("row", _DET, ids=[r[0] for r in _DET])
def test_normalized_refuses_what_the_deterministic_entries_refuse(lib, mode, row):
    _run_row(lib, mode, False, *row)


@pytest.mark.parametrize("mode", ["off", "ar"])
@pytest.mark.parametrize("row", _NZ, ids=[r[0] for r in _NZ])
def test_normalized_refuses_what_the_stochastic_entry_refuses(lib, mode, row):
    _run_row(lib, mode, True, *row)


@pytest.mark.parametrize("noise_on", [False, True])
@pytest.mark.parametrize("row", tp.OFF_ONLY, ids=[r[0] for r in tp.OFF_ONLY])
def test_normalized_einval_without_auto_reset(lib, row, noise_on):
    _run_row(lib, "off", noise_on, *row)


@pytest.mark.parametrize("noise_on", [False, True])
@pytest.mark.parametrize("row", tp.AR_ONLY, ids=[r[0] for r in tp.AR_ONLY])
def test_normalized_einval_with_auto_reset(lib, row, noise_on):
    _run_row(lib, "ar", noise_on, *row)


@pytest.mark.parametrize("mode", ["off", "ar"])
@pytest.mark.parametrize("noise_on", [False, True])
def test_normalized_refuses_a_bad_normaliser(lib, mode, noise_on):
    ok = ("x", {}, {}, {}, {}, None, 1)
    for nm, word in ((_nm(mean=None), b"null mean"), (_nm(scale=None), b"null scale"), (_nm(clip=0.0), b"clip"),
                     (_nm(clip=-1.0), b"clip"), (_nm(clip=float("nan")), b"clip")):
        _run_row(lib, mode, noise_on, *ok, word, nm=nm)
    # a NULL nm
    params = _lib.WgParams(**(tp.AR if mode == "ar" else tp.OFF))
    st = _lib.WgEpisodeStats() if mode == "ar" else None
    b, pol = tp._batch(), tp._pol()
    rc = lib.wg_rollout_normalized(C.byref(b), C.byref(params), C.byref(pol), None,
                                   C.byref(tp._nz()) if noise_on else None, None, None if st is None else C.byref(st), 1,
                                   None)
    assert rc == _lib.WG_EINVAL and b"null obs norm" in lib.wg_last_error()
    # null params, and an empty batch is accepted once everything else is
    assert lib.wg_rollout_normalized(C.byref(b), None, C.byref(pol), C.byref(_nm()), None, None, None, 1,
                                     None) == _lib.WG_EINVAL


def test_normalized_other_refusals_and_the_unchanged_lds_rule(lib, monkeypatch):
    b, pol = tp._batch(), tp._pol()
    for kw in (dict(spring_mode=1), dict(pair_mode=1)):
        assert _normalized(lib, b, _lib.WgParams(**dict(tp.OFF, **kw)), pol, _nm(), None, None, None, 1) == _lib.WG_EINVAL
        assert b"lean kernel" in lib.wg_last_error() and b"wg_rollout_normalized" in lib.wg_last_error()
    # the 80 KiB rule, unchanged (tests/test_pg_cpu.py's arithmetic: 80 KiB exactly with four words per walker, so the
    # eight words of the auto-reset mode pass it), with and without the noise
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
        assert _normalized(lib, big, _lib.WgParams(**tp.AR), wide, _nm(), nz, _lib.WgEpisodeStats(), None,
                           1) == _lib.WG_ERANGE
        assert b"LDS" in lib.wg_last_error()
    monkeypatch.setenv("WG_LEAN", "0")
    assert _normalized(lib, b, _lib.WgParams(**tp.OFF), pol, _nm(), None, None, None, 1) == _lib.WG_EINVAL
    assert b"lean kernel" in lib.wg_last_error()


# ------------------------------------------------------------------ the C boundary: the row calls
class NCall(tr.Call):
    """test_policy_rows_cpu.Call through the normalised entries, with mean / scale of its own."""

    def __init__(self, **kw):
        super().__init__(**kw)
        self.store = np.zeros(1 << 14, f32)                 # mean at 1 KiB, scale at 8 KiB of an arena of its own
        self.a.update(mean=self.store[256:256 + self.D], scale=self.store[2048:2048 + self.D])
        self.clip, self.nm_null = 1.5, False

    def nm(self):
        return None if self.nm_null else C.byref(_lib.WgObsNorm(mean=self.p("mean"), scale=self.p("scale"),
                                                                 clip=self.clip))

    def forward(self, lib, pol_null=False, rows_null=False):
        pol, rows = self.structs()
        return lib.wg_policy_forward_normalized(None if pol_null else C.byref(pol), self.nm(),
                                                None if rows_null else C.byref(rows), self.p("y"), self.y_step, None)

    def backward(self, lib, pol_null=False, rows_null=False):
        pol, rows = self.structs()
        return lib.wg_policy_backward_normalized(None if pol_null else C.byref(pol), self.nm(),
                                                 None if rows_null else C.byref(rows), self.p("dy"), self.dy_step,
                                                 self.chunk, self.p("workspace"), self.p("g_w1"), self.p("g_b1"),
                                                 self.p("g_w2"), self.p("g_b2"), None)


@pytest.mark.parametrize("row", tr.SHARED + tr.FORWARD_ONLY, ids=[r[0] for r in tr.SHARED + tr.FORWARD_ONLY])
def test_forward_normalized_einval(lib, row):
    what, changes, word = row
    tr._expect(lib, tr._apply(NCall(), changes).forward(lib), _lib.WG_EINVAL, word, what)
    assert b"wg_policy_forward_normalized" in lib.wg_last_error()


@pytest.mark.parametrize("row", tr.SHARED + tr.BACKWARD_ONLY, ids=[r[0] for r in tr.SHARED + tr.BACKWARD_ONLY])
def test_backward_normalized_einval(lib, row):
    what, changes, word = row
    tr._expect(lib, tr._apply(NCall(), changes).backward(lib), _lib.WG_EINVAL, word, what)
    assert b"wg_policy_backward_normalized" in lib.wg_last_error()


def test_row_calls_refuse_a_bad_normaliser_and_its_aliases(lib):
    for fn in ("forward", "backward"):
        tr._expect(lib, getattr(NCall(), fn)(lib, pol_null=True), _lib.WG_EINVAL, b"null policy", fn)
        tr._expect(lib, getattr(NCall(), fn)(lib, rows_null=True), _lib.WG_EINVAL, b"null rows", fn)
        c = NCall(); c.nm_null = True
        tr._expect(lib, getattr(c, fn)(lib), _lib.WG_EINVAL, b"null obs norm", fn)
        tr._expect(lib, getattr(tr._apply(NCall(), [("a", "mean", None)]), fn)(lib), _lib.WG_EINVAL, b"null mean", fn)
        tr._expect(lib, getattr(tr._apply(NCall(), [("a", "scale", None)]), fn)(lib), _lib.WG_EINVAL, b"null scale", fn)
        for clip in (0.0, -2.0, float("nan")):
            tr._expect(lib, getattr(tr._apply(NCall(), [("attr", "clip", clip)]), fn)(lib), _lib.WG_EINVAL, b"clip", fn)
    # an output that shares one element with mean or scale
    T, N, D, H, Cc, G = 3, 6, 5, 4, 2, 2
    for inp in ("mean", "scale"):
        c = NCall()
        c.a["y"] = c.a[inp].ctypes.data - (T * N * Cc - 1) * 4
        tr._expect(lib, c.forward(lib), _lib.WG_EINVAL, b"y aliases " + inp.encode(), inp)
        for out, n_out in dict(g_w1=G * D * H, g_b1=G * H, g_w2=G * H * Cc, g_b2=G * Cc).items():
            c = NCall()
            c.a[out] = c.a[inp].ctypes.data - (n_out - 1) * 4
            tr._expect(lib, c.backward(lib), _lib.WG_EINVAL, f"{out} aliases {inp}".encode(), (out, inp))
    # the limits are the plain calls': K at WG_POLICY_GRAD_MAX_K passes the plan, one block more is WG_ERANGE
    big = NCall(T=1, N=1, D=1, H=0, Cc=1, G=1, chunk=1)
    big.pol.update(obs_dim=4099, act_dim=4); big.rows.update(x_step=4099); big.y_step = big.dy_step = 4
    tr._expect(lib, big.backward(lib), _lib.WG_ERANGE, b"WG_POLICY_GRAD_MAX_K", "K limit")


# ------------------------------------------------------------------ the C boundary: wg_obs_moments
class MCall:
    """One valid wg_obs_moments call over host arrays (refused before a launch, or only planned)."""

    def __init__(self, T=3, N=6, D=5, chunk=4, pad=0):
        self.T, self.N, self.D = T, N, D
        arena = np.zeros(1 << 18, np.uint8)
        at = lambda off, n, dt: arena[off:off + n * np.dtype(dt).itemsize].view(dt)
        W = 1 + 2 * D
        self.n_chunks = -(-T * N // chunk)
        self.a = dict(x=at(0, T * (N * D + pad), f32), mask=at(1 << 14, T * (N + pad), np.uint8),
                      workspace=at(1 << 15, self.n_chunks * W, f64), state=at(1 << 16, W, f64),
                      mean_out=at(3 << 15, D, f32), scale_out=at(1 << 17, D, f32))
        self.rows = dict(x_step=N * D + pad, mask_step=N + pad, n_steps=T, N=N)
        self.obs_dim, self.chunk, self.bound, self.eps, self.rows_null = D, chunk, math.inf, 1e-8, False

    def p(self, name):
        v = self.a[name]
        return None if v is None else C.c_void_p(v if isinstance(v, int) else v.ctypes.data)

    def struct(self):
        return None if self.rows_null else C.byref(_lib.WgPolicyRows(x=self.p("x"), mask=self.p("mask"), **self.rows))

    def workspace(self, lib):
        return lib.wg_obs_moments_workspace(self.struct(), self.obs_dim, self.chunk)

    def moments(self, lib):
        return lib.wg_obs_moments(self.struct(), self.obs_dim, self.bound, self.chunk, self.p("workspace"),
                                  self.p("state"), self.eps, self.p("mean_out"), self.p("scale_out"), None)


M_SHARED = [
    ("null rows", [("attr", "rows_null", True)], b"null rows"),
    ("null x", [("a", "x", None)], b"null x"),
    ("obs_dim 0", [("attr", "obs_dim", 0)], b"obs_dim"),
    ("chunk_rows 0", [("attr", "chunk", 0)], b"chunk_rows"),
    ("n_steps 0", [("rows", "n_steps", 0)], b"n_steps"),
    ("N 0", [("rows", "N", 0)], b"N 0"),
    ("x_step", [("rows", "x_step", 6 * 5 - 1)], b"x_step"),
    ("mask_step", [("rows", "mask_step", 5)], b"mask_step"),
]
M_ONLY = [
    ("null workspace", [("a", "workspace", None)], b"null workspace"),
    ("null state", [("a", "state", None)], b"null state"),
    ("bound 0", [("attr", "bound", 0.0)], b"bound"),
    ("bound < 0", [("attr", "bound", -1.0)], b"bound"),
    ("bound NaN", [("attr", "bound", float("nan"))], b"bound"),
    ("eps < 0", [("attr", "eps", -1e-9)], b"eps"),
    ("eps NaN", [("attr", "eps", float("nan"))], b"eps"),
    ("mean_out alone", [("a", "scale_out", None)], b"go together"),
    ("scale_out alone", [("a", "mean_out", None)], b"go together"),
]


@pytest.mark.parametrize("row", M_SHARED + M_ONLY, ids=[r[0] for r in M_SHARED + M_ONLY])
def test_obs_moments_einval(lib, row):
    what, changes, word = row
    tr._expect(lib, tr._apply(MCall(), changes).moments(lib), _lib.WG_EINVAL, word, what)
    assert b"wg_obs_moments" in lib.wg_last_error()


@pytest.mark.parametrize("row", M_SHARED, ids=[r[0] for r in M_SHARED])
def test_obs_moments_workspace_einval(lib, row):
    what, changes, word = row
    tr._expect(lib, tr._apply(MCall(), changes).workspace(lib), _lib.WG_EINVAL, word, what)


def test_obs_moments_workspace_count_and_aliasing(lib):
    assert MCall().workspace(lib) == 5 * 11                       # 18 rows in chunks of 4
    assert MCall(chunk=18).workspace(lib) == 11 and MCall(chunk=1 << 30).workspace(lib) == 11
    assert MCall(chunk=1).workspace(lib) == 18 * 11 and MCall(pad=3).workspace(lib) == 5 * 11
    assert MCall(T=1, N=1, D=1, chunk=1).workspace(lib) == 3
    # a mask is optional; without one mask_step is not looked at (the call stops at the next refusal)
    c = tr._apply(MCall(), [("a", "mask", None), ("rows", "mask_step", 0), ("a", "state", None)])
    tr._expect(lib, c.moments(lib), _lib.WG_EINVAL, b"null state", "no mask")
    # N * obs_dim past 2^31, and a row wider than the LDS
    c = MCall(T=1, N=1, D=1, chunk=1)
    c.rows.update(N=1 << 20, x_step=1 << 40, mask_step=1 << 20); c.obs_dim = 1 << 12
    tr._expect(lib, c.workspace(lib), _lib.WG_ERANGE, b"2^31", "N * obs_dim")
    c = MCall(T=1, N=1, D=1, chunk=1)
    c.rows.update(x_step=20000); c.obs_dim = 20000
    tr._expect(lib, c.workspace(lib), _lib.WG_ERANGE, b"LDS", "row")
    # every output against every input and against the outputs before it, one shared element
    sizes = dict(workspace=(5 * 11, 8), state=(11, 8), mean_out=(5, 4), scale_out=(5, 4))
    for out, (n, elem) in sizes.items():
        for inp in ("x", "mask"):
            c = MCall()
            c.a[out] = c.a[inp].ctypes.data + (0 if inp == "x" else 3 * 6 - 1) - (n - 1) * elem
            if inp == "mask":                                # (aligned down: the last element still covers the byte)
                c.a[out] = c.a[inp].ctypes.data + 3 * 6 - 1 - (n * elem - 1)
            tr._expect(lib, c.moments(lib), _lib.WG_EINVAL, f"{out} aliases {inp}".encode(), (out, inp))
    outs = list(sizes)
    for i, out in enumerate(outs):
        for prev in outs[:i]:
            c = MCall()
            c.a[out] = c.a[prev].ctypes.data - (sizes[out][0] - 1) * sizes[out][1]
            tr._expect(lib, c.moments(lib), _lib.WG_EINVAL, f"{out} aliases {prev}".encode(), (out, prev))


# ------------------------------------------------------------------ the ABI
def test_wg_obs_norm_matches_header_and_abi_stays_16(lib, tmp_path):
    fields = [f for f, _ in _lib.WgObsNorm._fields_]
    lines = "".join(f'  printf("{f} %zu\\n", offsetof(wg_obs_norm, {f}));\n' for f in fields)
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "walker_hip.h"\nint main(void) {\n' + lines +
                     '  printf("sizeof %zu\\n", sizeof(wg_obs_norm));\n  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(probe)], check=True)
    got = dict(line.rsplit(" ", 1) for line in
               subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().splitlines())
    assert int(got["sizeof"]) == C.sizeof(_lib.WgObsNorm) == 24
    for f in fields:
        assert getattr(_lib.WgObsNorm, f).offset == int(got[f]), f
    assert _lib.ABI_VERSION == 16 and lib.wg_abi_version() == 16
    hdr = open(os.path.join(ROOT, "include", "walker_hip.h")).read()
    assert "#define WG_ABI_VERSION 16" in hdr and "equals x bit for bit on finite values" in hdr
    new = {"wg_rollout_normalized", "wg_policy_forward_normalized", "wg_policy_backward_normalized",
           "wg_obs_moments_workspace", "wg_obs_moments"}
    assert new <= set(_lib.EXPORTS)
    for name in new:
        assert getattr(lib, name) is not None
    assert lib.wg_obs_moments_workspace.restype is C.c_int64


# ------------------------------------------------------------------ the GPU cases mean something
@pytest.mark.parametrize("name", nc.NAMES + nc.COVER_NAMES)
def test_the_gpu_cases_meet_their_conditions_on_the_reference_engine(name):
    """Every run finite; between 1 % and 50 % of all normalised inputs clipped; with a finite act_limit some action
    saturated and some not; and the normaliser changes the bits of some action against the same weights without it."""
    case = nc.case_of(name)
    runs = [nc.reference_off(name), nc.reference_off(name, True), nc.reference_on(name), nc.reference_on(name, True)]
    for r in runs:
        assert all(np.isfinite(r[k]).all() for k in ("obs", "reward", "action")), name
    for r in runs[:2]:
        assert all(np.isfinite(r[k]).all() for k in ("pos", "vel", "acc"))
    for r in runs[2:]:
        assert r["reset"].any() and all(np.isfinite(r["state"][k]).all() for k in ("pos", "vel", "acc"))
    off = runs[0]
    share = float(np.mean(off["xn_clipped"]))
    assert 0.01 <= share <= 0.50, (name, share)
    a = off["action"]
    if np.isfinite(case.L):
        sat = np.abs(a) == f32(case.L)
        assert sat.any() and not sat.all(), (name, sat.mean())
    plain = nc.reference_off(name, False, False) if name in nc.CPU_CHECKED else None
    first = nc.policy_of(case, norm=False).forward_numpy(pc.entry_rows(case.base))
    assert not np.array_equal(bits(first), bits(a[0])), name
    if plain is not None:
        assert not np.array_equal(bits(plain["action"]), bits(a))


def test_the_balance_batch_keeps_its_zero_variance_column():
    st, mean, scale = nc.stats_of("balance16-mid-mlp-8sets")
    assert (scale == f32(1e4)).sum() == 1 and st[0] == 21 * 8200

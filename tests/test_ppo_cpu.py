"""wg_expf and wg_ppo_surrogate without a GPU: the numpy restatements (pg.expf_numpy, pg.ppo_surrogate_numpy) against
scalar pure-Python restatements of the header's contract, against float64 references, and the library's refusals, its
workspace count and the ABI (host pointers: no kernel is launched)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import ppo_cases as cs
from conftest import record_metric
from walker_gym_amd import _lib, build, pg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
bits = cs.bits


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def r32(v: float) -> float:
    """RN32 of a Python float (IEEE double): one C double -> float conversion.  For +, -, *, / of two float32 values
    the double result rounded again to float32 is the correctly rounded float32 result (53 >= 2 * 24 + 2)."""
    return C.c_float(v).value


# ------------------------------------------------------------------ wg_expf
LOG2E, LN2_HI, LN2_LO = (float.fromhex(h) for h in ("0x1.71547652b82fep+0", "0x1.62e42fee00000p-1",
                                                   "0x1.a39ef35793c76p-33"))


def expf_py(x: float) -> float:
    """The header's wg_expf, one Python float operation (an IEEE double operation) per line of the contract."""
    if x != x:
        return x
    xd = min(max(x, -150.0), 150.0)
    k = round(xd * LOG2E)                     # Python's round: ties to even
    r = (xd - k * LN2_HI) - k * LN2_LO
    p = 1.0 / math.factorial(13)
    for n in range(12, -1, -1):
        p = p * r + 1.0 / math.factorial(n)
    return r32(math.ldexp(p, k))


def test_expf_numpy_equals_the_scalar_restatement():
    rng = np.random.default_rng(5)
    x = np.concatenate([cs.SPECIALS, rng.uniform(-110, 95, 2000).astype(f32), rng.uniform(-1, 1, 1000).astype(f32),
                        rng.normal(0, 1e-3, 500).astype(f32), (np.arange(-217, 218) * math.log(2) * 0.5).astype(f32)])
    got = pg.expf_numpy(x)
    want = np.array([expf_py(float(v)) for v in x], f32)
    assert np.array_equal(bits(got), bits(want))
    assert abs(round(150.0 * LOG2E)) <= 217
    # k * LN2_HI is exact for |k| <= 217: LN2_HI has 21 trailing zero bits, k needs 8
    from fractions import Fraction
    assert all(Fraction(k * LN2_HI) == k * Fraction(LN2_HI) for k in range(-217, 218))


def ulp_distance(a, b):
    ia, ib = bits(a).astype(np.int64), bits(b).astype(np.int64)
    ia = np.where(ia < 0x80000000, ia, 0x80000000 - ia)
    ib = np.where(ib < 0x80000000, ib, 0x80000000 - ib)
    return np.abs(ia - ib)


@pytest.mark.parametrize("sample", ["structured", "seeded"])
def test_expf_numpy_against_float64_exp(sample):
    """Never more than 1 ulp from RN32(np.exp(float64(x))); the number of differing values is recorded, not asserted to
    be 0 (numpy's exp is not correctly rounded by contract).  Measured here: 0 on both samples."""
    x = cs.structured_patterns() if sample == "structured" else cs.seeded_sample()
    assert x.size > (1_000_000 if sample == "structured" else 9_999_999)
    differ, worst = 0, 0
    for part in np.array_split(x, 8):
        got = pg.expf_numpy(part)
        with np.errstate(over="ignore", under="ignore"):
            want = np.exp(part.astype(np.float64)).astype(f32)
        d = ulp_distance(got, want)
        differ += int((d != 0).sum())
        worst = max(worst, int(d.max()))
    record_metric(f"expf_numpy_vs_float64_exp_{sample}_differing_of_{x.size}", differ)
    assert worst <= 1, (sample, worst, differ)


def test_expf_specials_are_exact():
    e = lambda v: pg.expf_numpy(np.array([v], f32))[0]
    assert bits(e(0.0))[()] == bits(e(-0.0))[()] == 0x3F800000
    nan_in = cs.NAN_BITS.view(f32)
    assert np.array_equal(bits(pg.expf_numpy(nan_in)), cs.NAN_BITS)            # the payload is kept
    assert e(np.inf) == np.inf and bits(e(-np.inf))[()] == 0
    assert np.isfinite(e(88.72283)) and e(88.72284) == np.inf
    assert bits(e(-103.9))[()] == 1 and bits(e(-104.0))[()] == 0               # 1e-45, then +0
    assert e(151.0) == np.inf and bits(e(-151.0))[()] == 0
    assert bits(e(1.0))[()] == bits(f32(math.e))[()]


# ------------------------------------------------------------------ wg_ppo_surrogate: the scalar restatement
K0 = float(np.array([0x3F6B3F8E], np.uint32).view(f32)[0])


def surrogate_py(inp, mask, clip_eps, with_value, chunk_rows, density=False):
    """The header's contract row by row in Python floats, every float32 operation through r32."""
    y, u, sg, ls = inp["y"], inp["u"], inp["sigma"], inp["log_sigma"]
    T, N, Cc = y.shape
    G = sg.shape[0]
    n = N // G
    J = Cc + 5
    logp_o, dy_o, dv_o = np.zeros((T, N), f32), np.zeros((T, N, Cc), f32), np.zeros((T, N), f32)
    lo, hi = r32(1.0 - r32(clip_eps)), r32(1.0 + r32(clip_eps))
    sc0, sc1 = float(inp["scale"][0]), float(inp["scale"][1])
    S = [[0.0] * J for _ in range(G)]
    for g in range(G):
        n_chunks = -(-T * n // chunk_rows)
        for k in range(n_chunks):
            P = [0.0] * J
            for rho in range(k * chunk_rows, min((k + 1) * chunk_rows, T * n)):
                t, w = rho // n, g * n + rho % n
                if mask is not None and mask[t, w] == 0:
                    continue
                logp, z, q = 0.0, [0.0] * Cc, [0.0] * Cc
                for c in range(Cc):
                    e = r32(float(u[t, w, c]) - float(y[t, w, c]))
                    z[c] = r32(e / float(sg[g, c]))
                    q[c] = r32(z[c] * z[c])
                    l = r32(r32(r32(-0.5 * q[c]) - float(ls[g, c])) - K0)
                    logp = r32(logp + l)
                logp_o[t, w] = logp
                if density:
                    continue
                d = r32(logp - float(inp["old_logp"][t, w]))
                r = expf_py(d)
                A = float(inp["adv"][t, w])
                s1 = r32(r * A)
                rc = lo if r < lo else (hi if r > hi else r)
                s2 = r32(rc * A)
                take = s1 <= s2
                surr, gl = (s1 if take else s2), (s1 if take else 0.0)
                wr = r32(sc0 * gl)
                ev = 0.0
                if with_value:
                    ev = r32(float(inp["value"][t, w]) - float(inp["ret"][t, w]))
                    dv_o[t, w] = r32(sc1 * ev)
                for c in range(Cc):
                    dy_o[t, w, c] = r32(wr * r32(z[c] / float(sg[g, c])))
                    P[c] = P[c] + wr * r32(q[c] - 1.0)          # the product is exact in float64: one rounding
                for j, term in enumerate((1.0, surr, d, 1.0 if rc != r else 0.0, ev * ev)):
                    P[Cc + j] = P[Cc + j] + term
            for j in range(J):
                S[g][j] = S[g][j] + P[j]
    stats = [0.0] * 5
    for g in range(G):
        for j in range(5):
            stats[j] = stats[j] + S[g][Cc + j]
    return dict(logp=logp_o, dy=dy_o, dvalue=dv_o if with_value else None,
                g_log_sigma=np.array([[r32(S[g][c]) for c in range(Cc)] for g in range(G)], f32),
                stats=np.array(stats, np.float64))


@pytest.mark.parametrize("name", cs.CPU_NAMES)
@pytest.mark.parametrize("chunk", cs.CHUNKS)
def test_surrogate_numpy_equals_the_scalar_restatement(name, chunk):
    """Bit for bit, with NaN rows behind the mask; without a mask; without the value pair; the density alone."""
    clean = cs.inputs(name)
    for masked, with_value in ((True, True), (False, True), (True, False)):
        inp = cs.poisoned(clean) if masked else clean
        mask = inp["mask"] if masked else None
        got = pg.ppo_surrogate_numpy(inp["y"], inp["u"], inp["sigma"], inp["log_sigma"], inp["old_logp"], inp["adv"], mask,
                                     cs.CLIP, inp["scale"], inp["value"] if with_value else None,
                                     inp["ret"] if with_value else None, chunk)
        want = surrogate_py(inp, mask, cs.CLIP, with_value, chunk)
        for key in ("logp", "dy", "g_log_sigma", "stats"):
            assert np.array_equal(bits(got[key]), bits(want[key])), (name, chunk, masked, with_value, key)
        if with_value:
            assert np.array_equal(bits(got["dvalue"]), bits(want["dvalue"]))
        else:
            assert got["dvalue"] is None and got["stats"][4] == 0.0
        assert got["stats"][0] == (mask.sum() if masked else inp["mask"].size)
        assert np.isfinite(got["stats"]).all() and np.isfinite(got["dy"]).all()
    inp = cs.poisoned(clean)
    dens = pg.ppo_surrogate_numpy(inp["y"], inp["u"], inp["sigma"], inp["log_sigma"], mask=inp["mask"])
    assert set(dens) == {"logp"}
    assert np.array_equal(bits(dens["logp"]), bits(surrogate_py(inp, inp["mask"], 0.0, False, 1, density=True)["logp"]))


def test_the_cases_clip_on_both_sides_and_not_at_all():
    for name in ("rows64-2sets", "rows257", "rows255-2sets"):
        ref = cs.reference(name, 7)
        rows, clipped = ref["stats"][0], ref["stats"][3]
        assert 0 < clipped < rows, (name, clipped, rows)
        assert (ref["dy"] != 0).any() and (ref["dy"][cs.inputs(name)["mask"] != 0] == 0).all(-1).any()


# ------------------------------------------------------------------ against torch float64 autograd
@pytest.mark.parametrize("T,N,G,Cc", [(5, 200, 2, 3), (4, 64, 1, 8), (3, 100, 100, 4)])
def test_surrogate_numpy_against_float64_autograd(T, N, G, Cc):
    """The script's own expression (scripts/ppo_train.py: log_prob, torch.minimum of the ratio and its clamp) in float64
    under torch autograd, against the float32 contract.

    Tolerance, from the count of roundings (u = 2^-24).  A unit's l = RN32(RN32(RN32(-0.5 q) - log_sigma) - K0) with
    q = RN32(z^2), z = RN32(RN32(u - y) / sigma): q carries 5 u relative, the three further operations one u each of a
    magnitude below L_c = 0.5 q + |log_sigma| + K0, so |err(l)| <= 8 u L_c; each of the C additions into logp adds u
    times a partial sum below S = sum_c L_c.  |err(logp)| <= E = (8 + C) u S, per row.  d adds u |d|, the exponential
    turns the absolute error into a relative one and rounds once, r * A, scale * gl, z / sigma and the last product
    round once each, z carries 2 u, the float32 clip bounds differ from 0.8 / 1.2 by under 2 u:
      |dy - ref| <= (E + 10 u) |ref|,  |dvalue - ref| <= 3 u |ref|,
      |g_log_sigma - ref| <= sum_rows |wr| ((E + 5 u) |q - 1| + 6 u q) + u |ref|      (q - 1 = RN32(q - 1), q off by 5 u)
      |loss - ref| <= |scale0| sum_rows (E + 6 u) |surr| + 0.5 scale1 sum_rows 3 u ev^2 + u |ref|
    (float64 sums add nothing at this size).  No row sits at a tie: asserted on the reference alone with a margin of
    1e-3, above E max r."""
    import torch
    rng = np.random.default_rng(T * 1000 + N + Cc)
    y = rng.normal(0, 0.5, (T, N, Cc)).astype(f32)
    sigma = rng.uniform(0.2, 2.0, (G, Cc)).astype(f32)
    log_sigma = np.log(sigma.astype(np.float64)).astype(f32)
    sigma = np.exp(log_sigma.astype(np.float64)).astype(f32)      # the script's sigma: exp of the float32 log_sigma
    sets = np.arange(N) // (N // G)
    u = (y + (sigma[sets][None] * pg.action_noise_numpy(3, 0, T, 0, N, Cc)).astype(f32)).astype(f32)
    mask = rng.uniform(size=(T, N)) < 0.7
    value, ret = rng.normal(0, 1, (T, N)).astype(f32), rng.normal(0, 1, (T, N)).astype(f32)
    adv = (rng.uniform(0.1, 2.0, (T, N)) * rng.choice([-1.0, 1.0], (T, N))).astype(f32)
    band = rng.integers(0, 3, (T, N))
    target = np.choose(band, [rng.uniform(0.5, 0.75, (T, N)), rng.uniform(0.9, 1.1, (T, N)), rng.uniform(1.3, 1.6, (T, N))])
    cnt = max(int(mask.sum()), 1)
    scale = np.array([-1.0 / cnt, 1.0 / cnt], f32)

    td = lambda a, g=False: torch.tensor(np.asarray(a, np.float64), requires_grad=g)
    mean_t, ls_t, val_t = td(y, True), td(log_sigma, True), td(value, True)
    m_t, u_t = torch.tensor(mask), td(u)
    # the reference runs at the float32 sigma the kernel is given, as a constant times exp(log_sigma - log_sigma.detach())
    sg_t = td(sigma)[torch.tensor(sets)][None] * (ls_t - ls_t.detach())[torch.tensor(sets)][None].exp()
    z_t = (u_t - mean_t) / sg_t
    lp_t = (-0.5 * z_t * z_t - ls_t[torch.tensor(sets)][None] - 0.5 * math.log(2 * math.pi)).sum(-1)
    old_logp = (lp_t.detach().numpy() - np.log(target)).astype(f32)
    ratio = (lp_t - td(old_logp)).exp()
    s1_t, s2_t = ratio * td(adv), ratio.clamp(1 - cs.CLIP, 1 + cs.CLIP) * td(adv)
    surr_t = torch.minimum(s1_t, s2_t)
    ev_t = val_t - td(ret)
    loss_t = float(scale[0]) * (surr_t * m_t).sum() + 0.5 * float(scale[1]) * (ev_t.pow(2) * m_t).sum()
    loss_t.backward()
    r64 = ratio.detach().numpy()
    margin = 1e-3
    assert (np.abs(r64 - 0.8) > margin).all() and (np.abs(r64 - 1.2) > margin).all()
    clipped = (r64 < 0.8) | (r64 > 1.2)
    assert (np.abs(s1_t.detach().numpy() - s2_t.detach().numpy())[clipped] > margin).all()
    assert clipped.any() and not clipped.all() and mask.sum() > 10

    got = pg.ppo_surrogate_numpy(y, u, sigma, log_sigma, old_logp, adv, mask, cs.CLIP, scale, value, ret, 64)
    uu = 2.0 ** -24
    z64 = z_t.detach().numpy()
    q64 = z64 * z64
    L = 0.5 * q64 + np.abs(log_sigma.astype(np.float64))[sets][None] + K0
    E = (8 + Cc) * uu * L.sum(-1)                                               # [T, N]
    assert E.max() * r64.max() < margin
    on = mask
    ref_dy = mean_t.grad.numpy()
    err_dy = np.abs(got["dy"].astype(np.float64) - ref_dy)
    assert (err_dy <= (E + 10 * uu)[..., None] * np.abs(ref_dy) + 1e-300).all()
    assert (got["dy"][~on] == 0).all() and (ref_dy[~on] == 0).all()
    ref_dv = val_t.grad.numpy()
    err_dv = np.abs(got["dvalue"].astype(np.float64) - ref_dv)
    assert (err_dv <= 3 * uu * np.abs(ref_dv)).all()
    wr64 = np.where(on, float(scale[0]) * np.where(clipped & (s1_t.detach().numpy() > s2_t.detach().numpy()), 0.0,
                                                  s1_t.detach().numpy()), 0.0)
    ref_ls = ls_t.grad.numpy().reshape(G, Cc)
    tol_ls = (np.abs(wr64)[..., None] * ((E + 5 * uu)[..., None] * np.abs(q64 - 1) + 6 * uu * q64)) \
        .reshape(T, G, N // G, Cc).sum(axis=(0, 2)) + uu * np.abs(ref_ls)
    err_ls = np.abs(got["g_log_sigma"].astype(np.float64) - ref_ls)
    assert (err_ls <= tol_ls).all(), (err_ls / tol_ls).max()
    loss = float(f32(float(scale[0]) * got["stats"][1] + 0.5 * float(scale[1]) * got["stats"][4]))
    surr64, ev64 = surr_t.detach().numpy(), ev_t.detach().numpy()
    tol_loss = abs(float(scale[0])) * (on * (E + 6 * uu) * np.abs(surr64)).sum() + \
        0.5 * float(scale[1]) * (on * 3 * uu * ev64 ** 2).sum() + uu * abs(float(loss_t.detach()))
    assert abs(loss - float(loss_t.detach())) <= tol_loss
    assert got["stats"][0] == mask.sum() and got["stats"][3] == (clipped & on).sum()
    rel = lambda e, r: float((e / np.maximum(np.abs(r), 1e-30)).max())
    record_metric(f"ppo_numpy_vs_float64_autograd_T{T}_N{N}_G{G}_C{Cc}_max_rel_dy_ls_dvalue_loss",
                  (rel(err_dy[on], ref_dy[on]), rel(err_ls, ref_ls), rel(err_dv[on], ref_dv[on]),
                   abs(loss - float(loss_t.detach())) / abs(float(loss_t.detach()))))


# ------------------------------------------------------------------ the library's refusals (host pointers)
class Call:
    """One wg_ppo_surrogate call on host arrays (nothing is launched: every use ends in a refusal)."""

    def __init__(self, T=3, N=6, G=2, Cc=4, chunk=4, pad=2):
        arena = np.zeros(1 << 16, np.uint8)
        at = lambda off, n, dt: arena[off:off + n * np.dtype(dt).itemsize].view(dt)
        self.n_chunks = -(-T * (N // G) // chunk)
        rows, acts = T * (N + pad), T * (N * Cc + pad)
        self.a = dict(y=at(0, acts, f32), u=at(1 << 10, acts, f32), sigma=at(2 << 10, G * Cc, f32),
                      log_sigma=at(3 << 10, G * Cc, f32), mask=at(4 << 10, rows, np.uint8), old_logp=at(5 << 10, rows, f32),
                      adv=at(6 << 10, rows, f32), value=at(7 << 10, rows, f32), ret=at(8 << 10, rows, f32),
                      scale=at(9 << 10, 2, f32), workspace=at(10 << 10, G * self.n_chunks * (Cc + 5), np.float64),
                      logp_out=at(12 << 10, rows, f32), dy=at(13 << 10, acts, f32), dvalue=at(14 << 10, rows, f32),
                      g_log_sigma=at(15 << 10, G * Cc, f32), stats=at(16 << 10, 5, np.float64))
        self.rows = dict(y_step=N * Cc + pad, u_step=N * Cc + pad, mask_step=N + pad, n_steps=T, N=N, n_sets=G, act_dim=Cc)
        self.row_step, self.dy_step, self.chunk, self.clip, self.rows_null = N + pad, N * Cc + pad, chunk, 0.2, False
        self.sizes = dict(workspace=(G * self.n_chunks * (Cc + 5), 8), logp_out=(rows - pad, 4), dy=(acts - pad, 4),
                          dvalue=(rows - pad, 4), g_log_sigma=(G * Cc, 4), stats=(5, 8))
        self.in_sizes = dict(y=(acts - pad, 4), u=(acts - pad, 4), sigma=(G * Cc, 4), log_sigma=(G * Cc, 4),
                             mask=(rows - pad, 1), old_logp=(rows - pad, 4), adv=(rows - pad, 4), value=(rows - pad, 4),
                             ret=(rows - pad, 4), scale=(2, 4))

    def density(self):
        for k in ("old_logp", "adv", "value", "ret", "scale", "workspace", "dy", "dvalue", "g_log_sigma", "stats"):
            self.a[k] = None
        return self

    def p(self, name):
        v = self.a[name]
        return None if v is None else C.c_void_p(v if isinstance(v, int) else v.ctypes.data)

    def struct(self):
        if self.rows_null:
            return None
        return C.byref(_lib.WgPpoRows(y=self.p("y"), u=self.p("u"), sigma=self.p("sigma"), log_sigma=self.p("log_sigma"),
                                      mask=self.p("mask"), **self.rows))

    def workspace(self, lib):
        return lib.wg_ppo_surrogate_workspace(self.struct(), self.chunk)

    def run(self, lib):
        p = self.p
        return lib.wg_ppo_surrogate(self.struct(), p("old_logp"), p("adv"), self.row_step, p("value"), p("ret"), p("scale"),
                                    self.clip, self.chunk, p("workspace"), p("logp_out"), p("dy"), self.dy_step,
                                    p("dvalue"), p("g_log_sigma"), p("stats"), None)


def apply(call, changes):
    for kind, key, val in changes:
        if kind == "a":
            call.a[key] = val
        elif kind == "rows":
            call.rows[key] = val
        else:
            setattr(call, key, val)
    return call


def expect(lib, rc, code, word, what):
    assert rc == code, (what, rc, lib.wg_last_error())
    assert word in lib.wg_last_error(), (what, lib.wg_last_error())


# in the header's order: each row trips its own refusal with everything before it in order
SHARED = [
    ("null rows", [("attr", "rows_null", True)], b"null rows"),
    ("null y", [("a", "y", None)], b"null y"),
    ("null u", [("a", "u", None)], b"null u"),
    ("null sigma", [("a", "sigma", None)], b"null sigma"),
    ("null log_sigma", [("a", "log_sigma", None)], b"null log_sigma"),
    ("act_dim 0", [("rows", "act_dim", 0)], b"act_dim"),
    ("act_dim 257", [("rows", "act_dim", 257)], b"act_dim"),
    ("n_steps 0", [("rows", "n_steps", 0)], b"n_steps"),
    ("N 0", [("rows", "N", 0)], b"N 0"),
    ("n_sets 0", [("rows", "n_sets", 0)], b"n_sets"),
    ("n_sets 4 of 6", [("rows", "n_sets", 4)], b"n_sets"),
    ("y_step", [("rows", "y_step", 23)], b"y_step"),
    ("u_step", [("rows", "u_step", 23)], b"u_step"),
    ("mask_step", [("rows", "mask_step", 5)], b"mask_step"),
    ("chunk_rows 0", [("attr", "chunk", 0)], b"chunk_rows"),
]
LOSS_ONLY = [
    ("row_step", [("attr", "row_step", 5)], b"row_step"),
    ("dy_step", [("attr", "dy_step", 23)], b"dy_step"),
    ("null adv", [("a", "adv", None)], b"null adv"),
    ("null scale", [("a", "scale", None)], b"null scale"),
    ("null workspace", [("a", "workspace", None)], b"null workspace"),
    ("value alone", [("a", "ret", None)], b"go together"),
    ("ret alone", [("a", "value", None), ("a", "dvalue", None)], b"go together"),
    ("dvalue without value", [("a", "value", None), ("a", "ret", None)], b"dvalue without value"),
    ("clip < 0", [("attr", "clip", -0.1)], b"clip_eps"),
    ("clip inf", [("attr", "clip", math.inf)], b"clip_eps"),
    ("clip NaN", [("attr", "clip", math.nan)], b"clip_eps"),
    ("no output", [("a", k, None) for k in ("logp_out", "dy", "dvalue", "g_log_sigma", "stats")], b"every output"),
]


@pytest.mark.parametrize("row", SHARED + LOSS_ONLY, ids=[r[0] for r in SHARED + LOSS_ONLY])
def test_ppo_surrogate_einval(lib, row):
    what, changes, word = row
    expect(lib, apply(Call(), changes).run(lib), _lib.WG_EINVAL, word, what)
    assert b"wg_ppo_surrogate" in lib.wg_last_error()


@pytest.mark.parametrize("row", SHARED, ids=[r[0] for r in SHARED])
def test_ppo_surrogate_workspace_einval(lib, row):
    what, changes, word = row
    expect(lib, apply(Call(), changes).workspace(lib), _lib.WG_EINVAL, word, what)
    expect(lib, apply(Call().density(), changes).run(lib), _lib.WG_EINVAL, word, what)   # the density mode alike


def test_ppo_surrogate_refusals_come_in_the_documented_order(lib):
    """Two faults at once: the earlier one of the header's list is reported."""
    table = SHARED + LOSS_ONLY
    for i in range(len(table) - 1):
        a, b = table[i], table[i + 1]
        if {k for _, k, _ in a[1]} & {k for _, k, _ in b[1]}:
            continue
        if a[0] == "value alone":      # (with ret NULL the next row's value NULL is no fault)
            continue
        expect(lib, apply(apply(Call(), b[1]), a[1]).run(lib), _lib.WG_EINVAL, a[2], (a[0], b[0]))


def test_ppo_surrogate_density_mode_rules(lib):
    for k in ("adv", "value", "ret", "scale", "dy", "dvalue", "g_log_sigma", "stats", "workspace"):
        c = Call()
        keep = c.a[k]
        c.density().a[k] = keep
        if k == "value":
            c.a["ret"] = Call().a["ret"]
        expect(lib, c.run(lib), _lib.WG_EINVAL, b"only logp_out may be set", k)
    c = Call().density()
    c.a["logp_out"] = None
    expect(lib, c.run(lib), _lib.WG_EINVAL, b"logp_out is required", "logp_out")
    c = Call().density()
    c.clip = -1.0
    expect(lib, c.run(lib), _lib.WG_EINVAL, b"clip_eps", "clip in density mode")
    c = Call().density()
    c.a["logp_out"] = c.a["u"].ctypes.data + 4
    expect(lib, c.run(lib), _lib.WG_EINVAL, b"logp_out aliases u", "alias in density mode")


def test_ppo_surrogate_workspace_count_and_aliasing(lib):
    assert Call().workspace(lib) == 2 * 3 * 9                         # 2 sets of 9 rows in chunks of 4, 4 + 5 elements
    assert Call(chunk=9).workspace(lib) == 2 * 9 and Call(chunk=1 << 30).workspace(lib) == 2 * 9
    assert Call(chunk=1).workspace(lib) == 2 * 9 * 9 and Call(pad=0).workspace(lib) == 2 * 3 * 9
    assert Call(T=1, N=1, G=1, Cc=1, chunk=1).workspace(lib) == 6
    assert Call(T=5, N=7, G=7, Cc=3, chunk=2).workspace(lib) == 7 * 3 * 8
    assert Call(G=1).workspace(lib) == 5 * 9             # 18 rows in chunks of 4
    # a mask is optional; without one mask_step is not looked at
    c = apply(Call(), [("a", "mask", None), ("rows", "mask_step", 0), ("a", "adv", None)])
    expect(lib, c.run(lib), _lib.WG_EINVAL, b"null adv", "no mask")
    # N * act_dim past 2^31
    c = Call()
    c.rows.update(N=1 << 24, act_dim=256, y_step=1 << 40, u_step=1 << 40, mask_step=1 << 24)
    expect(lib, c.workspace(lib), _lib.WG_ERANGE, b"2^31", "N * act_dim")
    # every output against every input and against the outputs before it, one shared element
    base = Call()
    for out, (n, elem) in base.sizes.items():
        for inp, (n_in, elem_in) in base.in_sizes.items():
            c = Call()
            c.a[out] = c.a[inp].ctypes.data - (n - 1) * elem       # the output's last element on the input's first
            expect(lib, c.run(lib), _lib.WG_EINVAL, f"{out} aliases {inp}".encode(), (out, inp))
    outs = list(base.sizes)
    for i, out in enumerate(outs):
        for prev in outs[:i]:
            c = Call()
            c.a[out] = c.a[prev].ctypes.data - (base.sizes[out][0] - 1) * base.sizes[out][1]
            expect(lib, c.run(lib), _lib.WG_EINVAL, f"{out} aliases {prev}".encode(), (out, prev))


def test_expf_einval(lib):
    x = np.zeros(16, f32)
    p = lambda a, off=0: C.c_void_p(a.ctypes.data + off)
    expect(lib, lib.wg_expf(None, 4, p(x), None), _lib.WG_EINVAL, b"null x", "x")
    expect(lib, lib.wg_expf(p(x), 4, None, None), _lib.WG_EINVAL, b"null out", "out")
    expect(lib, lib.wg_expf(p(x), 0, p(x), None), _lib.WG_EINVAL, b"n 0 < 1", "n")
    expect(lib, lib.wg_expf(None, 0, None, None), _lib.WG_EINVAL, b"null x", "order")
    expect(lib, lib.wg_expf(p(x), 0, None, None), _lib.WG_EINVAL, b"null out", "order")
    for off in (4, 12, 28):
        expect(lib, lib.wg_expf(p(x), 8, p(x, off), None), _lib.WG_EINVAL, b"overlaps", off)
        expect(lib, lib.wg_expf(p(x, off), 8, p(x), None), _lib.WG_EINVAL, b"overlaps", -off)


# ------------------------------------------------------------------ the ABI and the package
def test_wg_ppo_rows_matches_header_and_abi_stays_16(lib, tmp_path):
    fields = [f for f, _ in _lib.WgPpoRows._fields_]
    lines = "".join(f'  printf("{f} %zu\\n", offsetof(wg_ppo_rows, {f}));\n' for f in fields)
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "walker_hip.h"\nint main(void) {\n' + lines +
                     '  printf("sizeof %zu\\n", sizeof(wg_ppo_rows));\n  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(probe)], check=True)
    got = dict(line.rsplit(" ", 1) for line in
               subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().splitlines())
    assert int(got["sizeof"]) == C.sizeof(_lib.WgPpoRows) == 80
    for f in fields:
        assert getattr(_lib.WgPpoRows, f).offset == int(got[f]), f
    assert _lib.ABI_VERSION == 16 and lib.wg_abi_version() == 16
    assert "#define WG_ABI_VERSION 16" in open(os.path.join(ROOT, "include", "walker_hip.h")).read()
    new = {"wg_expf", "wg_ppo_surrogate_workspace", "wg_ppo_surrogate"}
    assert new <= set(_lib.EXPORTS)
    for name in new:
        assert getattr(lib, name) is not None
    assert lib.wg_ppo_surrogate_workspace.restype is C.c_int64


def test_wg_expf_header_compiles_as_plain_c_and_agrees(tmp_path):
    """csrc/wg_expf.h is one definition for the kernels and for host probes: a C program over it gives expf_numpy's bits."""
    x = np.concatenate([cs.SPECIALS, cs.NAN_BITS.view(f32), np.random.default_rng(2).uniform(-110, 95, 4000).astype(f32)])
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <string.h>\n#include "wg_expf.h"\nint main(void) {\n  unsigned u;\n'
                     '  while (scanf("%x", &u) == 1) { float x, r; memcpy(&x, &u, 4); r = wg_expf_scalar(x);\n'
                     '    memcpy(&u, &r, 4); printf("%08x\\n", u); }\n  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-O2", "-I", os.path.join(ROOT, "walker_gym_amd", "csrc"), "-o", str(exe), str(probe), "-lm"],
                   check=True)
    out = subprocess.run([str(exe)], input="\n".join(f"{b:08x}" for b in bits(x)), capture_output=True, text=True,
                         check=True).stdout.split()
    assert np.array_equal(np.array([int(v, 16) for v in out], np.uint32), bits(pg.expf_numpy(x)))


def test_the_package_index_has_the_new_names():
    import walker_gym_amd as wga
    for name in ("expf", "expf_numpy", "log_prob_rows", "ppo_surrogate", "ppo_surrogate_numpy"):
        assert getattr(wga, name) is getattr(pg, name)

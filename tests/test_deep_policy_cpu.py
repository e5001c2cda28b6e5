"""The deep policy (MLPPolicy with a second hidden layer: wg_policy_mid, wg_rollout_deep, wg_policy_forward_deep /
_backward_deep) without a GPU: forward_numpy and the torch restatement against a scalar restatement of the contract, the
constructor's refusals, policy_grad_numpy against a scalar restatement and against float64 autograd, the identity
property (wm = I), the conditions on the cases the GPU tests compare bit for bit (tests/deep_cases.py), and every
refusal of the C boundary, which answers before anything touches a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import deep_cases as dc
import policy_cases as pc
from test_policy_cpu import _batch, _special_rows   # (rows with NaN / inf / -0.0; a batch of non-NULL fake pointers)
from walker_gym_amd import _lib, build, pg
from walker_gym_amd.policy import MLPPolicy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


# ------------------------------------------------------------------ the contract, scalar by scalar
def _unit(v, w, b, g, j):
    acc = f32(0.0) if b is None else f32(b[g, j])
    for i in range(w.shape[1]):
        acc = f32(acc + f32(f32(v[i]) * f32(w[g, i, j])))
    return acc


def _naive(x, w, L, sets):
    """The deep contract in nested Python loops over np.float32 scalars: (y before the clip, a, z1, z2)."""
    n = x.shape[0]
    H1, H2, Cc = w["w1"].shape[2], w["wm"].shape[2], w["w2"].shape[2]
    y, z1, z2 = np.zeros((n, Cc), f32), np.zeros((n, H1), f32), np.zeros((n, H2), f32)
    with np.errstate(all="ignore"):
        for r in range(n):
            g = sets[r]
            z1[r] = [_unit(x[r], w["w1"], w["b1"], g, j) for j in range(H1)]
            h1 = [z if z > 0 else f32(0.0) for z in z1[r]]
            z2[r] = [_unit(h1, w["wm"], w["bm"], g, k) for k in range(H2)]
            h2 = [z if z > 0 else f32(0.0) for z in z2[r]]
            y[r] = [_unit(h2, w["w2"], w["b2"], g, c) for c in range(Cc)]
        lim = f32(L)
        a = np.where(y < -lim, -lim, np.where(y > lim, lim, y)).astype(f32)
    return y, a, z1, z2


def _draw(rng, G, D, H1, H2, Cc, bias, s=0.5):
    w = dict(w1=(rng.standard_normal((G, D, H1)) * s).astype(f32), wm=(rng.standard_normal((G, H1, H2)) * s).astype(f32),
             w2=(rng.standard_normal((G, H2, Cc)) * s).astype(f32), b1=None, bm=None, b2=None)
    if bias:
        w.update(b1=(rng.standard_normal((G, H1)) * s).astype(f32), bm=(rng.standard_normal((G, H2)) * s).astype(f32),
                 b2=(rng.standard_normal((G, Cc)) * s).astype(f32))
    return w


@pytest.mark.parametrize("H1,H2,G,bias,L", [(5, 4, 1, True, 1.0), (5, 4, 3, True, float("inf")), (3, 6, 3, False, 1.0),
                                            (1, 1, 1, False, float("inf")), (6, 1, 2, True, 1.0)])
def test_forward_numpy_and_torch_equal_the_scalar_restatement(H1, H2, G, bias, L):
    rng = np.random.default_rng(70 + H1 + H2 + G)
    n, D, Cc = 12, 7, 3
    x = _special_rows(n, D, rng)
    w = _draw(rng, G, D, H1, H2, Cc, bias)
    w["wm"][0, 0, 0] = -0.0
    pol = dc.policy_from(w, act_limit=L)
    assert (pol.D, pol.H, pol.H2, pol.C, pol.G) == (D, H1, H2, Cc, G)
    sets = np.arange(n) // (n // G)
    _, want, _, _ = _naive(x, w, L, sets)
    got = pol.forward_numpy(x)
    assert got.dtype == f32 and same(got, want)
    assert not np.isnan(got[0]).any()        # a NaN input is cleared by the first ReLU
    part = pol.forward_numpy(x[5:9], first_walker=5, n_walkers_total=n)
    assert same(part, want[5:9])
    # the torch restatement, on the host here: whole batch, bound slice, scattered rows, after to()
    assert same(pol.for_rows(0, n)(torch.from_numpy(x), 0).numpy(), want)
    assert same(pol.for_rows(5, n)(torch.from_numpy(x[5:9]), 3).numpy(), want[5:9])
    idx = torch.tensor([7, 2, 11, 5])
    assert same(pol.for_row_index(idx, n)(torch.from_numpy(x[idx.numpy()]), 0).numpy(), want[idx.numpy()])
    moved = pol.to("cpu")
    assert moved.H2 == H2 and same(moved.forward_numpy(x), want)
    if G == 1:
        assert same(pol(torch.from_numpy(x), 0).numpy(), want)
    else:
        with pytest.raises(ValueError, match="for_rows"):
            pol(torch.from_numpy(x), 0)
    # pg's copies at act_limit = inf carry the layer
    y, _, _, _ = _naive(x, w, float("inf"), sets)
    assert same(pg.policy_rows_numpy(pol, x[None])[0], y)
    u, a, e = pg.stochastic_forward_numpy(pol, x, 0.25, seed=9, t=2)
    with np.errstate(all="ignore"):
        assert same(u, (y + (f32(0.25) * e).astype(f32)).astype(f32))


def test_constructor_keeps_identity_and_refuses_what_does_not_fit():
    z = lambda *s: torch.zeros(s)
    wm, bm = torch.nn.Parameter(z(2, 5, 4)), torch.nn.Parameter(z(2, 4))
    pol = MLPPolicy(z(2, 4, 3), z(2, 3), z(2, 7, 5), z(2, 5), wm=wm, bm=bm)
    assert pol.wm is wm and pol.bm is bm and (pol.H, pol.H2, pol.D, pol.C) == (5, 4, 7, 3)
    shallow = MLPPolicy(z(2, 5, 3), w1=z(2, 7, 5))
    assert shallow.H2 == 0 and shallow.wm is None and shallow.bm is None
    assert MLPPolicy(z(4, 3), w1=z(7, 5), wm=z(5, 4)).G == 1          # 2-D: one shared set
    with pytest.raises(ValueError, match="wm without w1"):
        MLPPolicy(z(4, 3), wm=z(5, 4))
    with pytest.raises(ValueError, match="bm without wm"):
        MLPPolicy(z(5, 3), w1=z(7, 5), bm=z(1, 5))
    with pytest.raises(ValueError):
        MLPPolicy(z(2, 4, 3), w1=z(2, 7, 5), wm=z(2, 6, 4))          # wm's inputs against w1's units
    with pytest.raises(ValueError):
        MLPPolicy(z(2, 4, 3), w1=z(2, 7, 5), wm=z(2, 5, 3))          # wm's units against w2's inputs
    with pytest.raises(ValueError):
        MLPPolicy(z(2, 4, 3), w1=z(2, 7, 5), wm=z(3, 5, 4))          # G
    with pytest.raises(ValueError):
        MLPPolicy(z(2, 4, 3), w1=z(2, 7, 5), wm=z(2, 5, 4), bm=z(2, 5))   # bm's width
    with pytest.raises(ValueError):
        MLPPolicy(z(2, 4, 3), w1=z(2, 7, 5), wm=z(2, 5, 4), b1=z(2, 4))   # b1 is H1 wide, not H2
    with pytest.raises(ValueError):
        MLPPolicy(z(2, 4, 3), w1=z(2, 7, 5), wm=z(2, 5, 4).double())
    with pytest.raises(ValueError):
        MLPPolicy(z(257, 3), w1=z(7, 5), wm=z(5, 257))               # H2 <= 256
    with pytest.raises(ValueError):
        MLPPolicy(z(4, 3), w1=z(7, 5), wm=z(4, 5, 4))                # rank against G


def test_evolution_strategy_refuses_a_deep_shape():
    from walker_gym_amd.es import EvolutionStrategy
    with pytest.raises(ValueError, match="one hidden layer"):
        EvolutionStrategy(None, hidden=(64, 64))


# ------------------------------------------------------------------ the gradient
def _naive_grad(x, dy, on, w, G, chunk):
    """wg_policy_backward_deep restated in scalar loops: float32 chains for dh2 / dh1, float64 sums in row order with a
    partial sum per chunk.  x [T, N, D], dy [T, N, C], on [T, N] bool."""
    T, N, D = x.shape
    n = N // G
    H1, H2, Cc = w["w1"].shape[2], w["wm"].shape[2], w["w2"].shape[2]
    keys = [k for k in ("w1", "b1", "wm", "bm", "w2", "b2") if w[k] is not None]
    S = {k: np.zeros(w[k].shape, np.float64) for k in keys}
    P = {k: np.zeros(w[k].shape, np.float64) for k in keys}
    with np.errstate(all="ignore"):
        for g in range(G):
            for rho in range(T * n):
                if rho and rho % chunk == 0:
                    for k in keys:
                        S[k][g] = S[k][g] + P[k][g]
                        P[k][g] = 0.0
                t, r = divmod(rho, n)
                wk = g * n + r
                if not on[t, wk]:
                    continue
                _, _, z1, z2 = _naive(x[t, wk][None], w, float("inf"), [g])
                z1, z2 = z1[0], z2[0]
                h1 = np.where(z1 > 0, z1, f32(0.0)).astype(f32)
                h2 = np.where(z2 > 0, z2, f32(0.0)).astype(f32)
                dh2 = np.zeros(H2, f32)
                for k in range(H2):
                    d = f32(0.0)
                    for c in range(Cc):
                        d = f32(d + f32(dy[t, wk, c] * w["w2"][g, k, c]))
                    dh2[k] = d if z2[k] > 0 else f32(0.0)
                dh1 = np.zeros(H1, f32)
                for j in range(H1):
                    d = f32(0.0)
                    for k in range(H2):
                        d = f32(d + f32(dh2[k] * w["wm"][g, j, k]))
                    dh1[j] = d if z1[j] > 0 else f32(0.0)
                f64 = lambda v: np.asarray(v, np.float64)
                for k, a, b in (("w1", x[t, wk], dh1), ("wm", h1, dh2), ("w2", h2, dy[t, wk])):
                    P[k][g] = P[k][g] + np.outer(f64(a), f64(b))
                for k, b in (("b1", dh1), ("bm", dh2), ("b2", dy[t, wk])):
                    if k in P:
                        P[k][g] = P[k][g] + f64(b)
    return {k: (S[k] + P[k]).astype(f32) for k in keys}


def _grad_case(seed, G, bias, mask):
    rng = np.random.default_rng(seed)
    T, N, D, H1, H2, Cc = 3, 6, 7, 5, 6, 3
    w = _draw(rng, G, D, H1, H2, Cc, bias)
    x = rng.standard_normal((T, N, D)).astype(f32)
    dy = rng.standard_normal((T, N, Cc)).astype(f32)
    on = np.ones((T, N), bool)
    if mask:
        on[rng.random((T, N)) < 0.3] = False
        x[~on] = np.nan
    return w, x, dy, on


GRAD_CASES = [(1, 1, True, False), (2, 3, True, True), (3, 2, False, True), (4, 6, False, False)]


@pytest.mark.parametrize("seed,G,bias,mask", GRAD_CASES)
def test_policy_grad_numpy_equals_the_scalar_restatement(seed, G, bias, mask):
    w, x, dy, on = _grad_case(seed, G, bias, mask)
    pol = dc.policy_from(w)
    for chunk in (4, 256):
        got = pg.policy_grad_numpy(pol, x, dy, on.astype(np.uint8) if mask else None, chunk_rows=chunk)
        assert len(got) == 6
        want = _naive_grad(x, dy, on, w, G, chunk)
        for k, g in zip(("w1", "b1", "wm", "bm", "w2", "b2"), got):
            assert (g is None) == (w[k] is None), k
            if g is not None:
                assert g.dtype == f32 and same(g, want[k]), (k, chunk)
    # a shallow policy still returns four
    assert len(pg.policy_grad_numpy(dc.shallow_from(dict(w, w2=w["wm"], b2=w["bm"])), x, np.zeros(x.shape[:2] + (6,), f32),
                                    on.astype(np.uint8))) == 4


@pytest.mark.parametrize("seed,G,bias,mask", GRAD_CASES)
def test_policy_grad_numpy_against_float64_autograd(seed, G, bias, mask):
    """The same net in float64 through torch.autograd.  What separates the two is float32 rounding alone, as long as no
    ReLU gate differs: the test asserts that every pre-activation of both layers is further than 1e-4 from zero in
    float64 (values are O(1)), so the gates agree.  The bound: a gradient element is a sum over rows of a product of two
    factors, each the end of at most five float32 chains (three forward, two backward) of at most D + 1 = 8 rounded
    multiply-adds, so about 2 * 5 * 16 roundings of 2^-24 relative to the terms' magnitudes: 1e-5 of the tensor's
    largest |sum of |terms|| is a bound with a margin of about two.  Measured on these four cases against float64: the
    largest deviation is 1.8e-7 of that scale (the bound holds with a factor of over 50 to spare)."""
    w, x, dy, on = _grad_case(seed, G, bias, mask)
    T, N, D = x.shape
    n = N // G
    got = pg.policy_grad_numpy(dc.policy_from(w), x, dy, on.astype(np.uint8) if mask else None)
    p = {k: None if v is None else torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in w.items()}
    sets = torch.arange(N) // n
    xs = torch.tensor(np.where(on[:, :, None], x, 0.0), dtype=torch.float64)
    lin = lambda v, wt, b: torch.einsum("tni,nij->tnj", v, wt[sets]) + (0.0 if b is None else b[sets][None])
    z1 = lin(xs, p["w1"], p["b1"])
    z2 = lin(torch.relu(z1), p["wm"], p["bm"])
    y = lin(torch.relu(z2), p["w2"], p["b2"])
    onb = torch.tensor(on)
    assert (z1[onb].abs() > 1e-4).all() and (z2[onb].abs() > 1e-4).all()
    (y * torch.tensor(dy, dtype=torch.float64) * onb[:, :, None]).sum().backward()
    # the scale of each tensor's sums: the same graph with every factor's magnitude
    worst = 0.0
    for k, g in zip(("w1", "b1", "wm", "bm", "w2", "b2"), got):
        if g is None:
            continue
        ref = p[k].grad.numpy()
        scale = np.abs(ref).max() + 1.0
        dev = np.abs(g.astype(np.float64) - ref).max() / scale
        worst = max(worst, dev)
        assert dev <= 1e-5, (k, dev)
    print(f"float64 autograd: largest deviation {worst:.3g} of the tensor's scale")


# ------------------------------------------------------------------ the identity property
@pytest.mark.parametrize("G,bias", [(1, True), (3, False)])
def test_identity_middle_layer_equals_the_shallow_policy(G, bias):
    """H2 = H1, wm = I, no bm: +0 + h * 1 is exact and a finite h * 0 is +-0, which leaves a chain that started at +0.0
    where it was.  Needs every h1 finite (asserted)."""
    rng = np.random.default_rng(5 + G)
    n, D, H, Cc = 12, 7, 5, 3
    sh, dp = dc.identity_pair(D, H, Cc, G, 11 + G, 0.5, bias)
    x = (rng.standard_normal((n, D)) * 3).astype(f32)
    x[3, 3], x[4, :] = -0.0, -0.0
    a, b = dc.shallow_from(sh, act_limit=1.0), dc.policy_from(dp, act_limit=1.0)
    sets = np.arange(n) // (n // G)
    _, _, z1, _ = _naive(x, dp, 1.0, sets)
    assert np.isfinite(z1).all()
    assert same(a.forward_numpy(x), b.forward_numpy(x))
    assert same(a.for_rows(0, n)(torch.from_numpy(x), 0).numpy(), b.for_rows(0, n)(torch.from_numpy(x), 0).numpy())
    # the gradients of the shared tensors too (dh1 = dh2 gated twice by the same sign)
    dy = rng.standard_normal((1, n, Cc)).astype(f32)
    g4, g6 = pg.policy_grad_numpy(a, x[None], dy), pg.policy_grad_numpy(b, x[None], dy)
    for i4, i6 in ((0, 0), (1, 1), (2, 4), (3, 5)):
        assert (g4[i4] is None and g6[i6] is None) or same(g4[i4], g6[i6]), (i4, i6)


# ------------------------------------------------------------------ the GPU cases mean something
def test_the_case_list_covers_every_tile():
    assert len({c.name for c in dc.CASES}) == len(dc.CASES) == len({c.seed for c in dc.CASES})
    for tile, M in dc.MASSES.items():
        cases = [c for c in dc.CASES if c.tile == tile]
        N = len(pc.spec_of(cases[0].kind)["mass_off"]) - 1
        for c in cases:
            assert c.T == 3 and c.L == float("inf") and N % c.G == 0 and 1 <= c.H2 <= 256 and c.H1 >= 1
        if tile == "six":
            assert {c.C for c in cases} == {5, 6} and all(c.C > M for c in cases)
            continue
        assert {c.H2 for c in cases} >= {1, M - 1, M, M + 1, 2 * M + 1, 256}, tile
        assert {c.H1 % 4 for c in cases} >= {2, 3}, tile
        assert any(c.H2 < 8 for c in cases) and any(c.H2 % 8 for c in cases), tile
        assert any(c.G == 1 for c in cases) and any(c.G == N for c in cases), tile
        if M < 64:   # a set boundary inside a wave tile
            assert any(1 < c.G < N and (N // c.G) % c.wpw != 0 for c in cases), tile
        assert any(c.seed % 2 for c in cases) and any(c.seed % 2 == 0 for c in cases), tile
    assert {(c.H1, c.H2) for c in dc.CASES} >= {(32, 32), (64, 64)}
    # the weights' two paths: a shared case per tile is staged under WG_POLICY_STAGE = 2 (never under 0), and on the
    # M = 64 tile one is too large to stage at all
    for tile in ("m4", "m16", "m64"):
        assert any(dc.lds_bytes(c)["staged"][2] for c in dc.CASES if c.tile == tile and c.G == 1), tile
    assert not dc.lds_bytes(dc.case_of("m64-h67x256-c20-g1"))["staged"][2]
    assert all(dc.lds_bytes(c)["lds"] <= 80 * 1024 for c in dc.CASES)
    assert all(dc.lds_bytes(c, episodes=True)["lds"] <= 80 * 1024 for c in dc.CASES)


@pytest.mark.parametrize("case", dc.CASES, ids=lambda c: c.name)
def test_gpu_cases_stay_finite_and_every_unit_is_on_and_off(case):
    """From the reference alone: the closed loop stays finite for its T steps; both biases on the odd seeds and none on
    the even; at step 0 every unit of both hidden layers is on for some walker and off for another; doubling a column
    of wm (the first, the last, the last one of lane q = 0) changes the bits of some action of step 0."""
    from oracle.oracle import nonfinite
    r = dc.oracle_rollout(case.name)
    assert np.isfinite(r["obs"]).all() and np.isfinite(r["reward"]).all() and np.isfinite(r["action"]).all()
    assert int(nonfinite(r["pos"], r["vel"], r["acc"], r["mass_off"]).sum()) == 0
    assert r["action"].shape == (case.T, r["obs"].shape[1], case.C)
    assert not np.array_equal(r["action"][1], r["action"][case.T - 1])      # the loop is closed
    w = dc.weights(case)
    for k in ("b1", "bm", "b2"):
        assert (w[k] is not None) == bool(case.seed % 2), k
    h1, h2 = dc.hidden0(case)
    assert np.isfinite(h1).all() and np.isfinite(h2).all()
    assert (h1 > 0).any(axis=0).all() and (h1 == 0).any(axis=0).all()
    assert (h2 > 0).any(axis=0).all() and (h2 == 0).any(axis=0).all()
    rows = dc.entry_rows(case)
    act0 = dc.policy_of(case).forward_numpy(rows)
    assert same(act0, r["action"][0])
    M = dc.MASSES[case.tile]
    for k in sorted({0, case.H2 - 1, (case.H2 - 1) // M * M}):
        wp = dict(w, wm=w["wm"].copy())
        wp["wm"][:, :, k] *= f32(2.0)
        assert not same(dc.policy_from(wp).forward_numpy(rows), act0), k


@pytest.mark.parametrize("batch,auto_reset,noise,norm,every,Tn", dc.MODE_RUNS)
def test_the_mode_runs_mean_something(batch, auto_reset, noise, norm, every, Tn):
    """From the reference alone: finite; the clip engages on some actions and not on all; with auto-reset off `done`
    fires at differing steps, with it on every walker is reset, the sunk ones more often than there are slots; under
    the hold walkers decide and hold side by side, and some enter inside a hold; both hidden layers have units on and
    off among the walkers at step 0."""
    r = dc.mode_reference(batch, auto_reset, noise, norm, every, Tn)
    for k in ("obs", "reward", "action", "hold_reward"):
        assert np.isfinite(r[k]).all(), k
    assert all(np.isfinite(np.asarray(r["state"][k])).all() for k in ("pos", "vel", "acc"))
    hit = np.abs(r["action"]) == f32(dc.MODE_L)
    assert hit.any() and not hit.all()
    if auto_reset:
        n = r["stats"]["episodes"]
        assert (n > 0).all() and len(np.unique(n)) >= 3 and (n > dc.SLOTS).any()   # (the sunk walkers: every step)
    else:
        ln = r["stats"]["lengths"]
        assert len(np.unique(ln)) >= 3 and (ln < Tn).any()
    if every > 1:
        assert 0 < r["decided"].mean() < 1 and not r["decided"][0].all()
        assert (r["raw"][r["decided"] == 0] == dc.SENTINEL).all()
    else:
        assert r["decided"].all()
    _, w = dc._mode_weights(batch, norm, False)
    pol = dc.mode_policy(batch, norm=norm)
    x = dc.mode_rows(batch)
    h1, h2 = dc.hidden_of(w, x if pol.obs_norm is None else pol.obs_norm.normalize_numpy(x), dc.MODES[batch]["G"])
    assert np.isfinite(h1).all() and (h1 > 0).any() and (h1 == 0).any() and (h2 > 0).any() and (h2 == 0).any()
    # the identity twins: every first-layer h finite on the rows of the run (what the identity property needs)
    _, wi = dc._mode_weights(batch, norm, True)
    rows = np.concatenate([x[None], r["obs"]]).reshape(-1, x.shape[1])
    rows = rows if pol.obs_norm is None else pol.obs_norm.normalize_numpy(rows)
    sets = np.tile(np.arange(x.shape[0]) // (x.shape[0] // dc.MODES[batch]["G"]), Tn + 1)
    with np.errstate(all="ignore"):
        z = wi["b1"][sets].astype(f32)
        for i in range(rows.shape[1]):
            z = z + rows[:, i:i + 1] * wi["w1"][sets, i]
    assert np.isfinite(z).all()


@pytest.mark.parametrize("name", [c.name for c in pc.COVER])
def test_the_instance_runs_stay_finite(name):
    for auto_reset in (False, True):
        r = dc.cover_reference(name, auto_reset)
        assert all(np.isfinite(r[k]).all() for k in ("obs", "reward", "action"))
        assert not np.array_equal(r["action"][0], r["action"][-1]) and (r["action"] != 0).all()
        if auto_reset:
            assert r["reset"].any() and not r["reset"].all()


def test_the_crafted_specials_reach_the_second_layer():
    """NaN, -0.0, a subnormal and +inf in z2 / h2, and what each does to its action column (tests/deep_cases.py)."""
    w = dc.special_weights()
    r = dc.special_rollout()
    x = pc.entry_rows("six-h0-c6-g1")
    n = x.shape[0] // 2
    sets = np.arange(x.shape[0]) // n
    _, _, z1, z2 = _naive(x[[0, 1, n, n + 1]], w, 1.0, sets[[0, 1, n, n + 1]])
    assert np.isfinite(z1).all()
    assert np.isnan(z2[:2, 0]).all() and (z2[:2, 1] == 0).all() and np.signbit(z2[:2, 1]).all()
    assert (z2[:2, 2] == f32(1e-40)).all() and 0 < f32(1e-40) < np.finfo(f32).tiny
    assert np.isposinf(z2[2:, 3]).all()
    a = r["action"]
    assert np.isfinite(a).all() and np.isfinite(r["obs"]).all()
    assert (a[:, :n, 1] == 0).all() and not np.signbit(a[:, :n, 1]).any()          # +0.0, not -0.0
    assert (a[:, :n, 2] == f32(f32(1e-40) * f32(2.0 ** 100))).all() and (a[:, :n, 2] > 1e-11).all()
    assert (a[:, n:] == np.sign(w["w2"][1, 3])[None, None, :]).all()               # +-inf, clipped
    # column 0 is the drawn bias plus the cleared NaN's +0.0: the same for every walker of the set
    assert (a[:, :n, 0] == a[0, 0, 0]).all()
    assert np.unique(a[:, :n, 3:]).size > 100                                      # the drawn columns vary


# ------------------------------------------------------------------ the C boundary
@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def _pol(**kw):
    d = dict(n_sets=1, obs_dim=152, hidden=24, w1=64, act_dim=8, w2=64, act_limit=1.0)
    d.update(kw)
    return _lib.WgPolicy(**d)


def _mid(**kw):
    d = dict(hidden2=16, wm=64)
    d.update(kw)
    return _lib.WgPolicyMid(**d)


def _deep(lib, b, p, pol, mid, nm=None, nz=None, hold=None, o=None, st=None, n_steps=1):
    r = lambda s: None if s is None else C.byref(s)
    return lib.wg_rollout_deep(C.byref(b), C.byref(p), r(pol), r(mid), r(nm), r(nz), r(hold), r(o), r(st), n_steps, None)


OFF = dict(in3d=1)


def test_wg_policy_mid_matches_header_and_abi_stays_16(lib, tmp_path):
    fields = [f for f, _ in _lib.WgPolicyMid._fields_]
    lines = "".join(f'  printf("{f} %zu\\n", offsetof(wg_policy_mid, {f}));\n' for f in fields)
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "walker_hip.h"\nint main(void) {\n' + lines +
                     '  printf("sizeof %zu\\n", sizeof(wg_policy_mid));\n  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(probe)], check=True)
    got = dict(line.rsplit(" ", 1) for line in
               subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().splitlines())
    assert int(got["sizeof"]) == C.sizeof(_lib.WgPolicyMid) == 24
    for f in fields:
        assert getattr(_lib.WgPolicyMid, f).offset == int(got[f]), f
    assert _lib.ABI_VERSION == 16 and lib.wg_abi_version() == 16
    new = {"wg_rollout_deep", "wg_policy_forward_deep", "wg_policy_backward_deep_workspace", "wg_policy_backward_deep"}
    assert new <= set(_lib.EXPORTS)
    for name in new:
        assert getattr(lib, name) is not None


@pytest.mark.parametrize("what,pol,mid,word", [
    ("null mid", {}, None, b"null middle layer"),
    ("hidden2 0", {}, dict(hidden2=0), b"hidden2"),
    ("hidden2 257", {}, dict(hidden2=257), b"hidden2"),
    ("null wm", {}, dict(wm=None), b"null wm"),
    ("hidden 0", dict(hidden=0, w1=None), {}, b"hidden > 0"),
    ("hidden without w1", dict(w1=None), {}, b"w1"),
    ("null w2", dict(w2=None), {}, b"w2"),
    ("obs_dim", dict(obs_dim=151), {}, b"obs_dim"),
    ("act_dim", dict(act_dim=9), {}, b"act_dim"),
    ("n_sets", dict(n_sets=3), {}, b"n_sets"),
    ("act_limit", dict(act_limit=0.0), {}, b"act_limit"),
])
def test_rollout_deep_einval_before_a_launch(lib, what, pol, mid, word):
    rc = _deep(lib, _batch(), _lib.WgParams(**OFF), _pol(**pol), None if mid is None else _mid(**mid))
    assert rc == _lib.WG_EINVAL, what
    assert word in lib.wg_last_error() and b"wg_rollout_deep" in lib.wg_last_error(), (what, lib.wg_last_error())


def test_rollout_deep_takes_the_modes_refusals(lib, monkeypatch):
    b, pol, mid = _batch(), _pol(), _mid()
    assert _deep(lib, b, _lib.WgParams(**OFF), None, mid) == _lib.WG_EINVAL and b"null policy" in lib.wg_last_error()
    assert _deep(lib, b, _lib.WgParams(**OFF), pol, mid, n_steps=0) == _lib.WG_EINVAL and b"n_steps" in lib.wg_last_error()
    # the mode by auto_reset: stats with 0, none with 1
    assert _deep(lib, b, _lib.WgParams(**OFF), pol, mid, st=_lib.WgEpisodeStats()) == _lib.WG_EINVAL
    assert b"episode stats" in lib.wg_last_error()
    # the hold's, the noise's and the normaliser's own
    assert _deep(lib, b, _lib.WgParams(**OFF), pol, mid, hold=_lib.WgActionHold(every=0)) == _lib.WG_EINVAL
    assert b"every" in lib.wg_last_error()
    assert _deep(lib, b, _lib.WgParams(**OFF), pol, mid, nz=_lib.WgActionNoise()) == _lib.WG_EINVAL
    assert b"sigma" in lib.wg_last_error()
    assert _deep(lib, b, _lib.WgParams(**OFF), pol, mid, nm=_lib.WgObsNorm(mean=64, scale=64, clip=0.0)) == _lib.WG_EINVAL
    assert b"clip" in lib.wg_last_error()
    for kw in (dict(spring_mode=1), dict(pair_mode=1)):
        assert _deep(lib, b, _lib.WgParams(**dict(OFF, **kw)), pol, mid) == _lib.WG_EINVAL
        assert b"lean kernel" in lib.wg_last_error()
    monkeypatch.setenv("WG_LEAN", "0")
    assert _deep(lib, b, _lib.WgParams(**OFF), pol, mid) == _lib.WG_EINVAL and b"lean kernel" in lib.wg_last_error()


def test_rollout_deep_lds_rule_counts_the_second_hidden_vector(lib):
    """The 80 KiB rule with hidden2 more words per walker: a shape whose workgroup is 80 KiB exactly with the hold's
    word and an H2 of 4 (one walker per wave, four waves) is accepted up to the launch's own refusals and passes the
    limit by 4 waves * 16 bytes with H2 = 8."""
    M, A = 64, 64
    D = 3 * 3 * M + A
    a16 = lambda n: (n + 15) & ~15

    def lds(K, H, H2):
        pl = (K + 3) & ~3
        sl = a16(pl * 24) + a16(pl * 12) + a16(K * 4 + 4) + a16(A * 4)
        return 4 * (sl + a16(D * 4) + a16(H * 4) + a16(A * 4) + 16 + a16(4) + a16(H2 * 4))
    K, H = next((K, H) for K in range(64, 513) for H in range(4, 257, 4) if lds(K, H, 4) == 80 * 1024)
    big = _batch(N=8192, M=M, K=K, A=A)
    wide = _pol(obs_dim=D, hidden=H, act_dim=A)
    assert _deep(lib, big, _lib.WgParams(**OFF), wide, _mid(hidden2=8)) == _lib.WG_ERANGE
    assert b"LDS" in lib.wg_last_error() and str(80 * 1024 + 4 * 16).encode() in lib.wg_last_error()
    assert _deep(lib, big, _lib.WgParams(**OFF), wide, _mid(hidden2=256)) == _lib.WG_ERANGE


# ---- the row calls
class Rows:
    """Arguments of the three deep row calls over small host arrays (never read: every call here is refused, or only
    plans)."""

    def __init__(self, T=3, N=6, D=5, H1=4, H2=3, Cc=2, G=2, b1=True, bm=True, b2=True, chunk=4):
        z = lambda *s: np.zeros(s, f32)
        self.a = dict(x=z(T, N, D), w1=z(G, D, H1), b1=z(G, H1) if b1 else None, wm=z(G, H1, H2),
                      bm=z(G, H2) if bm else None, w2=z(G, H2, Cc), b2=z(G, Cc) if b2 else None, y=z(T, N, Cc),
                      dy=z(T, N, Cc), workspace=np.zeros(1 << 16, np.float64), g_w1=z(G, D, H1),
                      g_b1=z(G, H1) if b1 else None, g_wm=z(G, H1, H2), g_bm=z(G, H2) if bm else None, g_w2=z(G, H2, Cc),
                      g_b2=z(G, Cc) if b2 else None)
        self.pol = dict(n_sets=G, obs_dim=D, hidden=H1, act_dim=Cc, act_limit=1.0)
        self.mid = dict(hidden2=H2)
        self.rows = dict(x_step=N * D, n_steps=T, N=N)
        self.chunk, self.y_step = chunk, N * Cc
        self.mid_null = False

    def _p(self, k):
        v = self.a[k]
        return None if v is None else (v if isinstance(v, int) else v.ctypes.data)

    def structs(self):
        pol = _lib.WgPolicy(w1=self._p("w1"), b1=self._p("b1"), w2=self._p("w2"), b2=self._p("b2"), **self.pol)
        mid = None if self.mid_null else _lib.WgPolicyMid(wm=self._p("wm"), bm=self._p("bm"), **self.mid)
        return pol, mid, _lib.WgPolicyRows(x=self._p("x"), **self.rows)

    def forward(self, lib):
        pol, mid, rows = self.structs()
        return lib.wg_policy_forward_deep(pol, mid, None, rows, self._p("y"), self.y_step, None)

    def workspace(self, lib):
        pol, mid, rows = self.structs()
        return lib.wg_policy_backward_deep_workspace(pol, mid, rows, self.chunk)

    def backward(self, lib):
        pol, mid, rows = self.structs()
        return lib.wg_policy_backward_deep(pol, mid, None, rows, self._p("dy"), self.y_step, self.chunk,
                                           self._p("workspace"), *(self._p(k) for k in ("g_w1", "g_b1", "g_wm", "g_bm",
                                                                                         "g_w2", "g_b2")), None)


def _expect(lib, rc, code, word, what):
    assert rc == code, (what, rc, lib.wg_last_error())
    assert word in lib.wg_last_error(), (what, lib.wg_last_error())


def test_row_calls_einval_before_a_launch(lib):
    for fn in ("forward", "workspace", "backward"):
        c = Rows()
        c.mid_null = True
        _expect(lib, getattr(c, fn)(lib), _lib.WG_EINVAL, b"null middle layer", fn)
        for h2 in (0, 257):
            c = Rows()
            c.mid["hidden2"] = h2
            _expect(lib, getattr(c, fn)(lib), _lib.WG_EINVAL, b"hidden2", (fn, h2))
        c = Rows()
        c.a["wm"] = None
        _expect(lib, getattr(c, fn)(lib), _lib.WG_EINVAL, b"null wm", fn)
        c = Rows()
        c.pol["hidden"] = 0
        _expect(lib, getattr(c, fn)(lib), _lib.WG_EINVAL, b"hidden > 0", fn)
        c = Rows()
        c.a["w1"] = None
        _expect(lib, getattr(c, fn)(lib), _lib.WG_EINVAL, b"w1", fn)
    c = Rows()
    c.a["y"] = None
    _expect(lib, c.forward(lib), _lib.WG_EINVAL, b"null y", "y")
    c = Rows()
    c.a["dy"] = None
    _expect(lib, c.backward(lib), _lib.WG_EINVAL, b"null dy", "dy")
    c = Rows()
    for k in ("g_w1", "g_b1", "g_wm", "g_bm", "g_w2", "g_b2"):
        c.a[k] = None
    _expect(lib, c.backward(lib), _lib.WG_EINVAL, b"every gradient pointer", "all null")
    for k, kw in (("g_b1", dict(b1=False)), ("g_bm", dict(bm=False)), ("g_b2", dict(b2=False))):
        c = Rows(**kw)
        c.a[k] = np.zeros(64, f32)
        _expect(lib, c.backward(lib), _lib.WG_EINVAL, k.encode(), k)
    c = Rows()
    c.chunk = 0
    _expect(lib, c.workspace(lib), _lib.WG_EINVAL, b"chunk_rows", "chunk")
    # one shared element between an output and the middle layer's inputs
    c = Rows()
    c.a["y"] = c.a["wm"].ctypes.data - (3 * 6 * 2 - 1) * 4
    _expect(lib, c.forward(lib), _lib.WG_EINVAL, b"y aliases wm", "y / wm")
    c = Rows()
    c.a["g_wm"] = c.a["bm"].ctypes.data - (2 * 4 * 3 - 1) * 4
    _expect(lib, c.backward(lib), _lib.WG_EINVAL, b"g_wm aliases bm", "g_wm / bm")
    c = Rows()
    c.a["g_bm"] = c.a["g_wm"].ctypes.data + 4
    _expect(lib, c.backward(lib), _lib.WG_EINVAL, b"aliases", "g_bm / g_wm")


def test_row_workspace_counts_six_segments(lib):
    # [n_sets][ceil(n_steps * n / chunk_rows)][K], K = w1 + b1 + wm + bm + w2 + b2, an absent bias taking no slot
    assert Rows().workspace(lib) == 2 * 3 * (20 + 4 + 12 + 3 + 6 + 2)
    assert Rows(b1=False).workspace(lib) == 2 * 3 * (20 + 12 + 3 + 6 + 2)
    assert Rows(bm=False).workspace(lib) == 2 * 3 * (20 + 4 + 12 + 6 + 2)
    assert Rows(b2=False, G=1, chunk=1).workspace(lib) == 18 * (20 + 4 + 12 + 3 + 6)


def blocks(D, H1, H2, Cc):
    up = lambda v: (v + 3) // 4
    return 16 * (up(D + 1) * up(H1) + up(H1 + 1) * up(H2) + up(H2 + 1) * up(Cc))


def _big(D, H1, H2, Cc):
    """A shape too large to allocate honestly: the planning call never reads an array."""
    c = Rows(T=1, N=1, D=1, H1=1, H2=1, Cc=1, G=1, chunk=1)
    c.pol.update(obs_dim=D, hidden=H1, act_dim=Cc)
    c.mid.update(hidden2=H2)
    c.rows.update(x_step=D)
    c.y_step = Cc
    return c


def test_the_block_count_formula_at_its_limit(lib):
    LIM = _lib.POLICY_GRAD_MAX_K
    # the canonical rows with the 64 x 64 net of the PPO baselines
    assert blocks(152, 64, 64, 8) == 14880 <= LIM
    assert _big(152, 64, 64, 8).workspace(lib) == 152 * 64 + 64 + 64 * 64 + 64 + 64 * 8 + 8
    # exactly at the limit: 30 x 16 blocks of w1|b1, 17 x 16 of wm|bm, 17 x 16 of w2|b2 = 1,024; one more group of four
    # rows or columns is refused
    D, Cc = 119, 64
    assert blocks(D, 64, 64, Cc) == LIM == 16 * 1024
    assert _big(D, 64, 64, Cc).workspace(lib) == D * 64 + 64 + 64 * 64 + 64 + 64 * Cc + Cc
    for d, c in ((D + 4, Cc), (D, Cc + 4)):
        assert blocks(d, 64, 64, c) > LIM
        for fn in ("workspace", "backward"):
            _expect(lib, getattr(_big(d, 64, 64, c), fn)(lib), _lib.WG_ERANGE, b"WG_POLICY_GRAD_MAX_K", (fn, d, c))
    # K within the limit, the blocking beyond it: one unit per layer pads every block to four columns
    assert 4095 + 1 + 1 + 1 + 1 + 1 <= LIM
    _expect(lib, _big(4095, 1, 1, 1).workspace(lib), _lib.WG_ERANGE, b"4 x 4 blocks", "blocked count")
    # the middle product alone
    assert blocks(3, 256, 256, 4) > LIM
    _expect(lib, _big(3, 256, 256, 4).workspace(lib), _lib.WG_ERANGE, b"WG_POLICY_GRAD_MAX_K", "256 x 256")

"""wg_gae_held (the advantage scan on the decision grid of wg_rollout_held, one thread per walker) against
pg.gae_held_numpy, bit for bit, and pg.collect(act_every=3) on Balance-v0."""
import ctypes as C

import numpy as np
import pytest

from conftest import gpu_available
from test_gpu_gae import _dev, _same
from test_pg_cpu import gae_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.skip("no ROCm GPU")


def _decided(T, N, seed):
    """Random at 1 / 3; walker 0 never decides, the last walker decides at the last step only."""
    dec = (np.random.default_rng(seed).random((T, N)) < 1 / 3).astype(np.uint8)
    dec[:, 0] = 0
    if N > 1:
        dec[:, -1] = 0
        dec[-1, -1] = 1
    return dec


@pytest.mark.parametrize("T", [1, 2, 9, 64])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 1000])
def test_gae_held_equals_numpy(T, N):
    """Every (n_steps, N): term / cut each NULL or set, ret NULL, +-inf and a NaN among the inputs; decided random at
    1 / 3 with walkers that never decide, and all ones, where the results are wg_gae's too."""
    import torch
    from walker_gym_amd import pg
    r, v, nv, term, cut = gae_inputs(T, N, 100 * T + N)
    r[0, 0], nv[0, -1] = np.inf, -np.inf
    dec = _decided(T, N, 3 * T + N)
    if N > 2:
        dec[:, 1] = 1                       # (a walker that decides at every step, with a +inf reward at step 0)
        r[0, 1] = np.inf
    ones = np.ones((T, N), np.uint8)
    dr, dv, dnv = _dev(r), _dev(v), _dev(nv)
    for d in (dec, ones):
        dd = _dev(d)
        for tm, ct, gamma, lam in ((term, cut, 0.99, 0.95), (term, None, 0.99, 0.95), (None, cut, 0.99, 0.95),
                                   (None, None, 0.99, 0.95), (term, cut, 1.0, 1.0)):
            adv, ret = pg.gae_held(dr, dv, dnv, dd, _dev(tm), _dev(ct), gamma, lam)
            wa, wr = pg.gae_held_numpy(r, v, nv, d, tm, ct, gamma, lam)
            torch.cuda.synchronize()
            assert adv.dtype == torch.float32 and _same(adv, wa) and _same(ret, wr), (gamma, lam)
            if d is ones:
                ga, gr = pg.gae(dr, dv, dnv, _dev(tm), _dev(ct), gamma, lam)
                torch.cuda.synchronize()
                assert _same(adv, ga) and _same(ret, gr)
        adv2, none = pg.gae_held(dr, dv, dnv, dd, _dev(term), _dev(cut), 1.0, 1.0, want_ret=False)   # ret NULL
        torch.cuda.synchronize()
        assert none is None and _same(adv2, wa)
    wa, wr = pg.gae_held_numpy(r, v, nv, dec, term, cut, 0.99, 0.95)
    assert not wa[:, 0].any() and not wr[:, 0].any() and (N == 1 or not wa[:-1, -1].any())
    assert not wa[dec == 0].any() and (N < 3 or not np.isfinite(wa[dec != 0]).all())
    flags = pg.gae_held(dr, dv, dnv, _dev(dec.astype(bool)), _dev(term.astype(bool)), _dev(cut.astype(bool)), 0.99, 0.95)
    assert _same(flags[0], wa)              # bool flags are bytes


@pytest.mark.parametrize("T,N,stride", [(9, 65, 70), (2, 1, 3), (64, 1000, 1024)])
def test_step_stride_leaves_the_gaps_untouched(T, N, stride):
    import torch
    from walker_gym_amd import _lib, pg
    r, v, nv, term, cut = gae_inputs(T, N, 7 * T + N)
    dec = _decided(T, N, 5 * T + N)
    dec[:, N // 2] = 1

    def padded(a, fill):
        out = np.full((T, stride), fill, a.dtype)
        out[:, :N] = a
        return _dev(out)
    dr, dv, dnv = padded(r, np.nan), padded(v, np.nan), padded(nv, np.nan)
    dd, dt, dc = padded(dec, 1), padded(term, 1), padded(cut, 1)
    adv = torch.full((T, stride), -123.0, device=DEV)
    ret = torch.full((T, stride), -321.0, device=DEV)
    p = _lib.ptr
    rc = _lib.load().wg_gae_held(p(dr), p(dv), p(dnv), p(dd), p(dt), p(dc), T, N, stride, 0.99, 0.95, p(adv), p(ret),
                                 C.c_void_p(torch.cuda.current_stream().cuda_stream))
    _lib.check(rc, "wg_gae_held")
    torch.cuda.synchronize()
    wa, wr = pg.gae_held_numpy(r, v, nv, dec, term, cut, 0.99, 0.95)
    ga, gr = adv.cpu().numpy(), ret.cpu().numpy()
    assert _same(ga[:, :N], wa) and _same(gr[:, :N], wr)
    assert (ga[:, N:] == -123.0).all() and (gr[:, N:] == -321.0).all()


def test_gae_held_refuses_before_a_launch():
    import torch
    from walker_gym_amd import pg
    z = lambda *s: torch.zeros(s, device=DEV)
    u8 = lambda *s: torch.zeros(s, dtype=torch.uint8, device=DEV)
    r = z(4, 8)
    for kw in (dict(value=z(4, 7)), dict(value=z(4, 8).double()), dict(next_value=torch.zeros(4, 8)), dict(decided=None),
               dict(decided=z(4, 8)), dict(decided=u8(3, 8)), dict(term=z(4, 8)), dict(cut=u8(3, 8)), dict(adv_out=r),
               dict(ret_out=r), dict(gamma=float("nan")), dict(lam=float("inf"))):
        args = dict(hold_reward=r, value=z(4, 8), next_value=z(4, 8), decided=u8(4, 8))
        args.update(kw)
        with pytest.raises(ValueError):
            pg.gae_held(**args)


def test_collect_with_a_hold_on_balance():
    """pg.collect(act_every=3) on Balance-v0 x 128, T = 16, H = 5: adv / ret are gae_held_numpy of the returned buffers;
    on the decided rows raw_action is policy_rows(obs_before) + sigma * eps, two roundings, in bits; value / next_value
    are value_fn's on the decided / closing rows and zero elsewhere."""
    import torch
    from walker_gym_amd import pg
    from walker_gym_amd.batched_env import BatchedPhysicsEnv
    from walker_gym_amd.policy import MLPPolicy
    from walker_gym_amd.walker import balance_spec
    N, T, max_steps, H, every, sigma = 128, 16, 6, 5, 3, 0.3
    spec = dict(balance_spec(N))
    rng = np.random.default_rng(9)
    vel = np.array(spec["vel"], f32).reshape(-1, 3).copy()
    vel[:, :2] += rng.uniform(-3, 3, (vel.shape[0], 2)).astype(f32)
    pos = np.array(spec["pos"], f32).reshape(-1, 3).copy()
    for w in range(3):                                       # three walkers sunk to mean y = -80: done by falling
        pos[4 * w:4 * w + 4, 1] += f32(-80.0) - pos[4 * w:4 * w + 4, 1].mean()
    spec.update(vel=vel, pos=pos, steps=(np.arange(N) % max_steps).astype(np.int32))
    env = BatchedPhysicsEnv(spec, device=DEV, in3d=0, max_steps=max_steps)
    D, A = env.obs_dim, env.batch.A
    g = torch.Generator().manual_seed(3)
    pol = MLPPolicy((torch.randn(H, A, generator=g) * 0.03).to(DEV), None,
                    (torch.randn(D, H, generator=g) * 0.008).to(DEV), (torch.randn(H, generator=g) * 0.008).to(DEV))
    wv = (torch.randn(D, generator=g) * 0.01).to(DEV)
    value_fn = lambda rows: rows @ wv
    env.enable_auto_reset(on=("nonfinite",), final_obs=True)
    with pytest.raises(ValueError, match="done"):             # a hold needs 'done' in the auto-reset set
        pg.collect(env, pol, sigma, T, 5, 0, value_fn, 0.99, 0.95, act_every=every)
    env = BatchedPhysicsEnv(spec, device=DEV, in3d=0, max_steps=max_steps)
    env.enable_auto_reset(final_obs=True)
    with pytest.raises(ValueError):
        pg.collect(env, pol, sigma, T, 5, 0, value_fn, 0.99, 0.95, act_every=0)
    obs0 = env.observe()[0].clone()
    out = pg.collect(env, pol, sigma, T, 5, 40, value_fn, 0.99, 0.95, act_every=every)
    torch.cuda.synchronize()
    h = {k: v.cpu().numpy() for k, v in out.items()}
    dec = h["decided"] != 0
    closes = np.concatenate([dec[1:], np.ones((1, N), bool)])
    assert 0.2 < dec.mean() < 0.7 and not dec[0].all() and (h["reset"] != 0).any()
    wa, wr = pg.gae_held_numpy(h["hold_reward"], h["value"], h["next_value"], h["decided"], h["term"], h["cut"], 0.99, 0.95)
    assert _same(h["adv"], wa) and _same(h["ret"], wr) and wa[dec].any() and not h["adv"][~dec].any()
    term = (h["done"] != 0) & (h["steps"] != max_steps)
    assert np.array_equal(h["term"] != 0, term) and np.array_equal(h["cut"], h["reset"])
    # the density's inputs on the decided rows: y + sigma * eps, two roundings
    before = torch.cat([obs0[None], out["obs"][:-1]])
    assert torch.equal(out["obs_before"], before)
    y = pg.policy_rows(pol, out["obs_before"], out["decided"]).cpu().numpy()
    u = (y + (f32(sigma) * h["eps"]).astype(f32)).astype(f32)
    assert np.array_equal(u.view(np.uint32)[dec], h["raw_action"].view(np.uint32)[dec])
    assert _same(h["eps"][dec], pg.action_noise_numpy(5, 40, T, 0, N, A)[dec])
    assert not h["eps"][~dec].any() and not h["raw_action"][~dec].any()
    assert np.array_equal(h["action"][dec], np.clip(h["raw_action"][dec], -1, 1))
    # the hold: a row that did not decide applies the row above's action
    assert np.array_equal(h["action"][1:][~dec[1:]], h["action"][:-1][~dec[1:]])
    # the values are value_fn's of the rows the definition names, zero elsewhere
    vb = value_fn(before.reshape(T * N, D)).reshape(T, N).cpu().numpy()
    assert np.allclose(h["value"][dec], vb[dec], rtol=1e-5, atol=1e-6) and not h["value"][~dec].any()
    after = torch.where(out["reset"][..., None] != 0, out["final_obs"], out["obs"])
    va = value_fn(after.reshape(T * N, D)).reshape(T, N).cpu().numpy()
    assert np.allclose(h["next_value"][closes], va[closes], rtol=1e-5, atol=1e-6) and not h["next_value"][~closes].any()
    assert out["held"].shape == (N, A + 1) and _same(out["held"][:, :A], h["action"][-1])
    assert _same(out["held"][:, A], h["hold_reward"][-1])
    assert set(("return_sum", "episodes", "tail_return", "decided", "hold_reward", "held")) <= set(out)
    # continued with held and step_base: the first row of the walkers inside a hold applies the action held
    nxt = pg.collect(env, pol, sigma, 4, 5, 40 + T, value_fn, 0.99, 0.95, act_every=every, held=out["held"])
    torch.cuda.synchronize()
    d0 = nxt["decided"][0].cpu().numpy() != 0
    assert (~d0).any() and _same(nxt["action"][0].cpu().numpy()[~d0], h["action"][-1][~d0])

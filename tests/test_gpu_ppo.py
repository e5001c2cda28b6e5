"""wg_expf and wg_ppo_surrogate on the device against pg.expf_numpy / pg.ppo_surrogate_numpy, bit for bit (NaN == NaN:
the sign and payload of a produced NaN are no part of the contract), the autograd wrapper over them, and the loop closed
once on a real batch: the density of the recorded rows under the policy that produced them gives a ratio of exactly 1."""
import numpy as np
import pytest

import ppo_cases as cs
from conftest import gpu_available

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.skip("no ROCm GPU")


def _host(a):
    return np.ascontiguousarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a)


def _same(a, b):
    if a is None or b is None:
        return a is None and b is None
    a, b = _host(a), _host(b)
    na, nb = np.isnan(a), np.isnan(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(na, nb) and \
        np.array_equal(cs.bits(a)[~na], cs.bits(b)[~nb])


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.array(a, copy=True)).to(DEV)


def _window(a, pad):
    """`a` [T, N, C] as a window of a longer buffer: pad floats between its steps (a sentinel in them)."""
    import torch
    T, N, Cc = a.shape
    buf = torch.full((T, N * Cc + pad), -7.0, dtype=torch.float32, device=DEV)
    win = buf[:, :N * Cc].unflatten(1, (N, Cc))
    win.copy_(_dev(a))
    return buf, win


def _run(inp, chunk, masked=True, with_value=True, want=("logp", "dy", "dvalue", "g_log_sigma", "stats"), pad=0):
    from walker_gym_amd import pg
    d = {k: _dev(v) for k, v in inp.items()}
    bufs = None
    if pad:
        by, d["y"] = _window(inp["y"], pad)
        bu, d["u"] = _window(inp["u"], pad)
        bufs = (by, bu)
    return pg.ppo_surrogate_rows(d["y"], d["u"], d["sigma"], d["log_sigma"], d["old_logp"], d["adv"], d["scale"],
                                 d["mask"] if masked else None, cs.CLIP, d["value"] if with_value else None,
                                 d["ret"] if with_value else None, chunk, want), bufs


def _check(out, ref, keys, what):
    for k in keys:
        assert _same(out[k], ref[k]), (what, k)


# ------------------------------------------------------------------ wg_expf
def test_expf_equals_numpy_in_place_and_out_of_place():
    import torch
    from walker_gym_amd import pg
    i = np.arange(1 << 20, dtype=np.uint32) << np.uint32(12)
    x = np.concatenate([i, i | np.uint32(0xFFF), cs.bits(cs.seeded_sample(10)), cs.bits(cs.SPECIALS), cs.NAN_BITS]).view(f32)
    want = pg.expf_numpy(x)
    xd = _dev(x)
    got = pg.expf(xd)
    assert np.array_equal(cs.bits(_host(got)), cs.bits(want))          # NaN payloads kept: plain bit equality
    assert np.array_equal(cs.bits(_host(xd)), cs.bits(x))
    assert pg.expf(xd, out=xd) is xd
    assert np.array_equal(cs.bits(_host(xd)), cs.bits(want))
    one = pg.expf(torch.zeros(3, device=DEV) * torch.tensor([1.0, -1.0, 1.0], device=DEV))
    assert (_host(one).view(np.uint32) == 0x3F800000).all()


# ------------------------------------------------------------------ wg_ppo_surrogate against numpy
@pytest.mark.parametrize("chunk", cs.CHUNKS)
@pytest.mark.parametrize("name", cs.NAMES)
def test_surrogate_equals_numpy(name, chunk):
    """Mask (NaN rows behind it) and value pair; neither; twice the same bits; each optional output alone."""
    keys = ("logp", "dy", "dvalue", "g_log_sigma", "stats")
    inp, ref = cs.poisoned(cs.inputs(name)), cs.reference(name, chunk)
    out, _ = _run(inp, chunk)
    _check(out, ref, keys, (name, chunk, "masked"))
    again, _ = _run(inp, chunk)
    assert all(np.array_equal(cs.bits(_host(out[k])), cs.bits(_host(again[k]))) for k in keys)
    plain = cs.reference(name, chunk, masked=False, with_value=False)
    out, _ = _run(cs.inputs(name), chunk, masked=False, with_value=False)
    _check(out, plain, ("logp", "dy", "g_log_sigma", "stats"), (name, chunk, "plain"))
    assert "dvalue" not in out and float(out["stats"][4]) == 0.0
    for k in keys:
        out, _ = _run(inp, chunk, want=(k,))
        assert set(out) == {k} and _same(out[k], ref[k]), (name, chunk, "alone", k)


@pytest.mark.parametrize("name", cs.NAMES)
def test_density_mode_equals_numpy(name):
    import torch
    from walker_gym_amd import pg
    inp = cs.poisoned(cs.inputs(name))
    ref = pg.ppo_surrogate_numpy(inp["y"], inp["u"], inp["sigma"], inp["log_sigma"], mask=inp["mask"])["logp"]
    d = {k: _dev(v) for k, v in inp.items()}
    assert _same(pg.log_prob_rows(d["y"], d["u"], d["sigma"], d["log_sigma"], d["mask"]), ref)
    clean = cs.inputs(name)
    ref = pg.ppo_surrogate_numpy(clean["y"], clean["u"], clean["sigma"], clean["log_sigma"])["logp"]
    d = {k: _dev(v) for k, v in clean.items()}
    assert _same(pg.log_prob_rows(d["y"], d["u"], d["sigma"], d["log_sigma"]), ref)
    s = cs.shape_of(name)
    if s.G == 1:   # [R, C] rows and a [C] log_sigma
        flat = pg.log_prob_rows(d["y"].reshape(-1, s.C), d["u"].reshape(-1, s.C), d["sigma"][0], d["log_sigma"][0])
        assert flat.shape == (s.T * s.N,) and _same(flat.reshape(s.T, s.N), ref)
    _, wy = _window(clean["y"], 3)
    _, wu = _window(clean["u"], 4)
    assert _same(pg.log_prob_rows(wy, wu, d["sigma"], d["log_sigma"]), ref)


@pytest.mark.parametrize("pad", [3, 4])
@pytest.mark.parametrize("name", ["rows63", "rows64-2sets", "rows257", "set-per-walker"])
def test_strided_windows_and_skipped_rows_of_dy(name, pad):
    """y, u and dy as windows of longer buffers (pad 4 keeps the 16-byte path of act_dim 4 / 8, pad 3 leaves it); the
    rows the mask skips keep what dy held, and so do the floats between the steps."""
    import torch
    from walker_gym_amd import pg
    inp, ref = cs.poisoned(cs.inputs(name)), cs.reference(name, 7)
    s = cs.shape_of(name)
    d = {k: _dev(v) for k, v in inp.items()}
    by, wy = _window(inp["y"], pad)
    bu, wu = _window(inp["u"], pad)
    bdy, wdy = _window(np.full((s.T, s.N, s.C), 9.0, f32), pad)
    out = pg.ppo_surrogate_rows(wy, wu, d["sigma"], d["log_sigma"], d["old_logp"], d["adv"], d["scale"], d["mask"], cs.CLIP,
                                d["value"], d["ret"], 7, dy_out=wdy)
    assert out["dy"] is wdy
    on = inp["mask"] != 0
    want_dy = np.where(on[..., None], ref["dy"], f32(9.0))
    assert _same(wdy, want_dy)
    assert (_host(bdy)[:, s.N * s.C:] == -7.0).all() and (_host(by)[:, s.N * s.C:] == -7.0).all()
    _check(out, ref, ("logp", "dvalue", "g_log_sigma", "stats"), (name, pad))


@pytest.mark.parametrize("name", ["rows65", "rows64-2sets", "rows1"])
def test_nan_and_inf_rows_flow_through(name):
    """An unmasked NaN row and an unmasked inf row: every output is what the arithmetic says (the numpy restatement)."""
    from walker_gym_amd import pg
    inp = {k: v.copy() for k, v in cs.inputs(name).items()}
    inp["y"].reshape(-1, inp["y"].shape[-1])[0, 0] = np.nan
    inp["u"].reshape(-1, inp["u"].shape[-1])[-1, -1] = np.inf
    ref = pg.ppo_surrogate_numpy(inp["y"], inp["u"], inp["sigma"], inp["log_sigma"], inp["old_logp"], inp["adv"], None,
                                 cs.CLIP, inp["scale"], inp["value"], inp["ret"], 7)
    assert np.isnan(ref["stats"][1]) and np.isnan(ref["dy"]).any()
    out, _ = _run(inp, 7, masked=False)
    _check(out, ref, ("logp", "dy", "dvalue", "g_log_sigma", "stats"), name)


@pytest.mark.parametrize("Cc", [251, 252, 256])
def test_wide_rows_take_short_tiles_and_a_second_chain(Cc):
    """act_dim + 5 elements pass the workgroup's 256 threads from act_dim 252 on (threads 0..4 carry a second chain), and
    a tile holds 62 such rows: 2 * 65 rows per set are two full tiles and a ragged one."""
    import torch
    from walker_gym_amd import pg
    T, N, G = 2, 130, 2
    rng = np.random.default_rng(Cc)
    y = rng.normal(0, 0.5, (T, N, Cc)).astype(f32)
    sigma = rng.uniform(0.5, 2.0, (G, Cc)).astype(f32)
    log_sigma = np.log(sigma.astype(np.float64)).astype(f32)
    u = (y + (sigma[np.arange(N) // (N // G)][None] * pg.action_noise_numpy(5, 0, T, 0, N, Cc)).astype(f32)).astype(f32)
    logp = pg.ppo_surrogate_numpy(y, u, sigma, log_sigma)["logp"]
    inp = dict(y=y, u=u, sigma=sigma, log_sigma=log_sigma, old_logp=(logp + rng.normal(0, 0.2, (T, N))).astype(f32),
               adv=rng.normal(0, 1, (T, N)).astype(f32), value=rng.normal(0, 1, (T, N)).astype(f32),
               ret=rng.normal(0, 1, (T, N)).astype(f32), mask=(rng.uniform(size=(T, N)) < 0.8).astype(np.uint8),
               scale=np.array([-0.01, 0.02], f32))
    ref = pg.ppo_surrogate_numpy(y, u, sigma, log_sigma, inp["old_logp"], inp["adv"], inp["mask"], cs.CLIP, inp["scale"],
                                 inp["value"], inp["ret"], 256)
    assert 0 < ref["stats"][3] < ref["stats"][0]
    out, _ = _run(cs.poisoned(inp), 256)
    _check(out, ref, ("logp", "dy", "dvalue", "g_log_sigma", "stats"), Cc)


# ------------------------------------------------------------------ the autograd wrapper
def test_autograd_wrapper_returns_the_kernels_gradients():
    import torch
    from walker_gym_amd import pg
    name, chunk = "rows64-2sets", 7
    inp, ref = cs.poisoned(cs.inputs(name)), cs.reference(name, chunk)
    d = {k: _dev(v) for k, v in inp.items()}
    mean, ls, value = (d[k].clone().requires_grad_(True) for k in ("y", "log_sigma", "value"))
    sigma = ls.detach().exp()
    loss, info = pg.ppo_surrogate(mean, d["u"], ls, d["old_logp"], d["adv"], d["mask"], cs.CLIP, value=value, ret=d["ret"],
                                  chunk_rows=chunk)
    direct = pg.ppo_surrogate_rows(d["y"], d["u"], sigma, d["log_sigma"], d["old_logp"], d["adv"], d["scale"], d["mask"],
                                   cs.CLIP, d["value"], d["ret"], chunk)
    loss.backward()
    assert _same(mean.grad, direct["dy"]) and _same(ls.grad, direct["g_log_sigma"]) and _same(value.grad, direct["dvalue"])
    assert _same(info["stats"], direct["stats"]) and _same(info["logp"], direct["logp"])
    st = _host(direct["stats"])
    sc = inp["scale"].astype(np.float64)
    assert loss.dtype == torch.float32 and float(loss.detach()) == float(f32(sc[0] * st[1] + 0.5 * sc[1] * st[4]))
    assert float(info["approx_kl"]) == -st[2] / st[0] and float(info["clip_fraction"]) == st[3] / st[0]
    assert float(info["value_loss"]) == st[4] / st[0]
    # the restatement at the sigma torch's exp gave (the kernel takes sigma as an input; it computes neither from the other)
    again = pg.ppo_surrogate_numpy(inp["y"], inp["u"], _host(sigma), inp["log_sigma"], inp["old_logp"], inp["adv"],
                                   inp["mask"], cs.CLIP, inp["scale"], inp["value"], inp["ret"], chunk)
    assert _same(mean.grad, again["dy"]) and _same(ls.grad, again["g_log_sigma"])
    assert ref["stats"][0] == st[0]
    # an upstream factor scales the kept gradients
    mean2 = d["y"].clone().requires_grad_(True)
    loss2, _ = pg.ppo_surrogate(mean2, d["u"], d["log_sigma"], d["old_logp"], d["adv"], d["mask"], cs.CLIP, chunk_rows=chunk,
                                scale=float(inp["scale"][0]))
    (2.0 * loss2).backward()
    assert _same(mean2.grad, 2.0 * direct["dy"])


@pytest.mark.parametrize("deep", [False, True], ids=["shallow", "deep"])
def test_autograd_through_policy_rows(deep):
    """loss.backward() through pg.policy_rows into the policy's tensors equals policy_rows_backward fed the same dy."""
    import torch
    from walker_gym_amd import pg
    from walker_gym_amd.policy import MLPPolicy
    T, N, D, H, H2, Cc, chunk = 3, 40, 6, 5, 4, 3, 16
    rng = np.random.default_rng(11 + deep)
    draw = lambda *s, k=1.0: torch.from_numpy((rng.standard_normal(s) * k).astype(f32)).to(DEV).requires_grad_(True)
    w1, b1 = draw(1, D, H), draw(1, H)
    wm, bm = (draw(1, H, H2), draw(1, H2)) if deep else (None, None)
    w2, b2 = draw(1, H2 if deep else H, Cc, k=0.3), draw(1, Cc, k=0.1)
    pol = MLPPolicy(w2, b2, w1, b1, act_limit=1.0, wm=wm, bm=bm)
    obs = torch.from_numpy(rng.standard_normal((T, N, D)).astype(f32)).to(DEV)
    mask = torch.from_numpy((rng.uniform(size=(T, N)) < 0.7)).to(DEV)
    ls = torch.full((Cc,), -0.7, device=DEV, requires_grad=True)
    sigma = ls.detach().exp()
    with torch.no_grad():
        y0 = pg.policy_rows_forward(pol, obs, mask)
        u = y0 + sigma * torch.from_numpy(pg.action_noise_numpy(1, 0, T, 0, N, Cc)).to(DEV)
        old = pg.log_prob_rows(y0, u, sigma, ls.detach(), mask) + 0.3 * torch.randn(T, N, device=DEV)
    adv = torch.randn(T, N, device=DEV)
    loss, info = pg.ppo_surrogate(pg.policy_rows(pol, obs, mask, chunk), u, ls, old, adv, mask, chunk_rows=chunk)
    loss.backward()
    cnt = mask.sum().clamp(min=1).to(torch.float32)
    scale = torch.stack([-1.0 / cnt, torch.zeros((), device=DEV)])
    direct = pg.ppo_surrogate_rows(y0, u, sigma, ls.detach(), old, adv, scale, mask, 0.2, chunk_rows=chunk)
    grads = pg.policy_rows_backward(pol, obs, direct["dy"], mask, chunk)
    tensors = (w1, b1, wm, bm, w2, b2) if deep else (w1, b1, w2, b2)
    assert len(grads) == len(tensors)
    for t, g in zip(tensors, grads):
        assert _same(t.grad, g) and float(t.grad.abs().sum()) > 0
    assert _same(ls.grad, direct["g_log_sigma"].reshape(-1))


# ------------------------------------------------------------------ the loop closed once on a real batch
def test_first_pass_ratio_is_exactly_one_on_a_collected_batch():
    import torch
    from walker_gym_amd import pg
    from walker_gym_amd.batched_env import BatchedPhysicsEnv
    from walker_gym_amd.policy import MLPPolicy
    from walker_gym_amd.walker import balance_spec
    torch.manual_seed(0)
    env = BatchedPhysicsEnv(balance_spec(128), in3d=0, max_steps=200, rand_sigma=0.01, seed=0)
    env.enable_auto_reset(on=("done", "nonfinite"), noise_rows=8, final_obs=True)
    N, D, A, H, T = env.N, env.obs_dim, env.batch.A, 16, 8
    p = lambda *s, k: torch.randn(s, device=env.device) * k
    pol = MLPPolicy(p(1, H, A, k=0.01), torch.zeros(1, A, device=env.device), p(1, D, H, k=0.002),
                    torch.zeros(1, H, device=env.device))
    log_sigma = torch.full((A,), float(np.log(0.3)), device=env.device)
    sigma = log_sigma.exp().reshape(1, A).contiguous()
    batch = pg.collect(env, pol, sigma, T, 0, 0, lambda rows: torch.zeros(rows.shape[0], device=rows.device))
    obs, u, adv = batch["obs_before"], batch["raw_action"], batch["adv"]
    ok = torch.isfinite(adv) & torch.isfinite(obs).all(-1) & torch.isfinite(u).all(-1)
    assert int(ok.sum()) > T * N // 2
    mean = pg.policy_rows_forward(pol, obs, ok)
    old = pg.log_prob_rows(mean, u, sigma.reshape(-1), log_sigma, ok)
    cnt = ok.sum().to(torch.float32)
    scale = torch.stack([-1.0 / cnt, 1.0 / cnt])
    out = pg.ppo_surrogate_rows(mean, u, sigma.reshape(-1), log_sigma, old, adv, scale, ok, 0.2, chunk_rows=256)
    assert np.array_equal(cs.bits(_host(out["logp"])), cs.bits(_host(old)))
    d = out["logp"] - old
    assert (_host(d).view(np.uint32) == 0).all()                                     # d == +0.0 on every row
    assert (_host(pg.expf(d)).view(np.uint32)[_host(ok)] == 0x3F800000).all()        # r == 1
    st = _host(out["stats"])
    assert st[0] == int(ok.sum()) and st[2] == 0.0 and not np.signbit(st[2]) and st[3] == 0.0
    ref = pg.ppo_surrogate_numpy(_host(mean), _host(u), _host(sigma), _host(log_sigma), _host(old), _host(adv), _host(ok),
                                 0.2, _host(scale), chunk_rows=256)
    assert _same(out["dy"], ref["dy"]) and _same(out["g_log_sigma"], ref["g_log_sigma"]) and _same(out["stats"], ref["stats"])
    assert float(out["dy"].abs().sum()) > 0
    loss, info = pg.ppo_surrogate(mean, u, log_sigma, old, adv, ok)
    assert float(info["clip_fraction"]) == 0.0 and float(info["approx_kl"]) == 0.0


# ------------------------------------------------------------------ refusals with device pointers
def test_refusals_with_device_pointers():
    import torch
    from walker_gym_amd import pg
    inp = cs.inputs("rows64-2sets")
    d = {k: _dev(v) for k, v in inp.items()}
    args = lambda **kw: dict(dict(mean=d["y"], raw_action=d["u"], sigma=d["sigma"], log_sigma=d["log_sigma"],
                                  old_logp=d["old_logp"], adv=d["adv"], scale=d["scale"], mask=d["mask"], clip=cs.CLIP,
                                  value=d["value"], ret=d["ret"], chunk_rows=7), **kw)
    with pytest.raises(ValueError, match="dy aliases y"):
        pg.ppo_surrogate_rows(**args(dy_out=d["y"]))
    with pytest.raises(ValueError, match="dy aliases u"):
        pg.ppo_surrogate_rows(**args(dy_out=d["u"]))
    with pytest.raises(ValueError, match="clip_eps"):
        pg.ppo_surrogate_rows(**args(clip=-0.5))
    with pytest.raises(ValueError, match="chunk_rows"):
        pg.ppo_surrogate_rows(**args(chunk_rows=0))
    with pytest.raises(ValueError, match="go together"):
        pg.ppo_surrogate_rows(**args(ret=None))
    with pytest.raises(ValueError, match="n_sets"):
        pg.ppo_surrogate_rows(**args(sigma=d["sigma"].repeat(3, 1)[:5].contiguous(),
                                     log_sigma=d["log_sigma"].repeat(3, 1)[:5].contiguous()))
    x = torch.zeros(64, device=DEV)
    with pytest.raises(ValueError, match="overlaps"):
        pg.expf(x[:32], out=x[1:33])
    with pytest.raises(ValueError):
        pg.expf(torch.zeros(4))
    ok = pg.ppo_surrogate_rows(**args())          # and the call the refusals were variations of goes through
    assert _same(ok["dy"], cs.reference("rows64-2sets", 7)["dy"])

"""wg_adam_step on the device against optim.adam_step_numpy, bit for bit (NaN == NaN): every table of adam_cases through
three consecutive steps on one state, the fused launch against the three launches, the special gradients, the skipped
step, the refusals with device pointers, optim.Adam, and the loop closed once: a collected batch through policy_rows,
ppo_surrogate and backward into Adam.step(), and EvolutionStrategy(optimizer="adam")."""
import numpy as np
import pytest

import adam_cases as ac
from conftest import gpu_available

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32 = np.float32
SENT = -7.25          # what surrounds every buffer
PAD = 8


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.skip("no ROCm GPU")


def _host(a):
    return np.ascontiguousarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a)


def _place(arr, off=0, dtype=None):
    """`arr` on the device `off` elements into a buffer of sentinels (the buffer itself starts on a 16-byte boundary):
    (buffer, view)."""
    import torch
    t = torch.from_numpy(np.array(arr, copy=True))
    buf = torch.full((off + t.numel() + PAD,), SENT, dtype=t.dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + t.numel()]
    view.copy_(t.to(DEV))
    return buf, view


def _margins_intact(buf, view):
    off = (view.data_ptr() - buf.data_ptr()) // buf.element_size()
    b = _host(buf)
    return (b[:off] == SENT).all() and (b[off + view.numel():] == SENT).all()


class Run:
    """A table on the device: sentinels around every buffer, workspace and state included."""

    def __init__(self, name):
        import torch
        d = ac.inputs(name)
        offs = [o for _, o in ac.TABLES[name]]
        self.p = [_place(a, o[0]) for a, o in zip(d["params"], offs)]
        self.m = [_place(a, o[2]) for a, o in zip(d["m"], offs)]
        self.v = [_place(a, o[3]) for a, o in zip(d["v"], offs)]
        self.g = [[_place(a, o[1]) for a, o in zip(step, offs)] for step in d["grads"]]
        self.g_host = d["grads"]
        self.state = _place(np.zeros(8, np.float64), 1)
        self.ws = _place(np.zeros((ac.total(name) + 4095) // 4096, np.float64), 1)
        self.torch = torch

    def step(self, s, cfg):
        from walker_gym_amd import optim
        v = lambda pairs: [x[1] for x in pairs]
        optim.adam_step(v(self.p), v(self.g[s]), v(self.m), v(self.v), self.state[1], cfg, self.ws[1])

    def result(self):
        h = lambda pairs: [_host(x[1]) for x in pairs]
        return h(self.p), h(self.m), h(self.v), _host(self.state[1])

    def check_margins_and_grads(self):
        for buf, view in self.p + self.m + self.v + [self.state, self.ws] + [x for step in self.g for x in step]:
            assert _margins_intact(buf, view)
        for step, host in zip(self.g, self.g_host):
            for (_, view), want in zip(step, host):
                assert np.array_equal(ac.bits(_host(view)), ac.bits(want))        # grad is never written


def _equal(got, want, what):
    gp, gm, gv, gs = got
    wp, wm, wv, ws = want
    for i in range(len(wp)):
        assert ac.same(gp[i], wp[i]), (what, "param", i)
        assert ac.same(gm[i], wm[i]), (what, "m", i)
        assert ac.same(gv[i], wv[i]), (what, "v", i)
    assert ac.same(gs[:6], ws[:6]), (what, "state", gs, ws)
    assert (gs[6:] == 0).all()                                                    # state[6..7] are left alone


# ------------------------------------------------------------------ every table, three steps on one state
@pytest.mark.parametrize("variant", tuple(ac.VARIANTS))
@pytest.mark.parametrize("name", ac.NAMES)
def test_three_steps_equal_numpy(name, variant, monkeypatch):
    """The default path (fused up to WG_ADAM_FUSED_MAX's default, three launches above)."""
    monkeypatch.delenv("WG_ADAM_FUSED_MAX", raising=False)
    run, cfg, ref = Run(name), ac.config(variant), ac.reference(name, variant)
    for s in range(ac.STEPS):
        run.step(s, cfg)
        _equal(run.result(), ref[s], (name, variant, s))
    clip = ac.VARIANTS[variant][0]
    assert (ref[-1][3][4] < 1.0) == clip and ref[-1][3][0] == ac.STEPS and ref[-1][3][5] == 0
    run.check_margins_and_grads()


@pytest.mark.parametrize("name", ac.BOTH_PATHS)
def test_fused_and_three_launches_give_the_same_bytes(name, monkeypatch):
    variant = "clip-wd-min"
    cfg, ref = ac.config(variant), ac.reference(name, variant)
    for limit in ("0", str(1 << 30)):          # never fused; always fused
        monkeypatch.setenv("WG_ADAM_FUSED_MAX", limit)
        run = Run(name)
        for s in range(ac.STEPS):
            run.step(s, cfg)
            _equal(run.result(), ref[s], (name, limit, s))
        run.check_margins_and_grads()


def test_two_calls_from_the_same_start_agree(monkeypatch):
    monkeypatch.delenv("WG_ADAM_FUSED_MAX", raising=False)
    cfg = ac.config("clip-wd-max")
    for name in ("seven", "big"):
        a, b = Run(name), Run(name)
        a.step(0, cfg)
        b.step(0, cfg)
        ra, rb = a.result(), b.result()
        for x, y in zip(ra[0] + ra[1] + ra[2] + [ra[3]], rb[0] + rb[1] + rb[2] + [rb[3]]):
            assert np.array_equal(ac.bits(x), ac.bits(y))


# ------------------------------------------------------------------ special gradients, the skipped step
def _direct(p, g, m, v, state, cfg):
    """Host arrays through one device call and through the restatement: ((p, m, v, state) device, the same numpy)."""
    import torch
    from walker_gym_amd import optim
    dp, dg, dm, dv = (_place(a) for a in (p, g, m, v))
    ds = _place(state, 1)
    optim.adam_step([dp[1]], [dg[1]], [dm[1]], [dv[1]], ds[1], cfg)
    hp, hm, hv, hs = p.copy(), m.copy(), v.copy(), state.copy()
    optim.adam_step_numpy([hp], [g], [hm], [hv], hs, cfg)
    for buf, view in (dp, dg, dm, dv, ds):
        assert _margins_intact(buf, view)
    assert np.array_equal(ac.bits(_host(dg[1])), ac.bits(g))
    return (_host(dp[1]), _host(dm[1]), _host(dv[1]), _host(ds[1])), (hp, hm, hv, hs)


@pytest.mark.parametrize("fused", ["0", "65536"])
@pytest.mark.parametrize("case", tuple(ac.SPECIALS))
def test_special_gradients(case, fused, monkeypatch):
    from walker_gym_amd import optim
    monkeypatch.setenv("WG_ADAM_FUSED_MAX", fused)
    g0, v0 = ac.SPECIALS[case]
    p = np.array([0.5, -0.25, 1.0, 2.0], f32)
    g = np.array([g0, 0.0, -g0, 0.0], f32)
    m, v = np.zeros(4, f32), np.full(4, v0, f32)
    cfg = optim.adam_config(lr=1e-3, max_norm=np.inf)
    got, want = _direct(p, g, m, v, np.zeros(8), cfg)
    for a, b in zip(got, want):
        assert ac.same(a, b), case
    assert got[3][4] == 1.0 and got[3][5] == 0.0 and got[3][0] == 1.0           # cf == 1 exactly, not skipped
    if case == "zero-g-zero-v":
        assert (got[0] == p).all() and (got[1] == 0).all()                       # upd = +-0
    if case == "denormal-square":
        assert 0 < got[2][0] < np.finfo(f32).tiny                                # v' is a denormal, and is kept
    if case == "vanishing-square":
        assert got[2][0] == 0 and got[1][0] != 0
    if case == "overflowing-square":
        assert np.isinf(got[2][0]) and np.isfinite(got[3][3]) and got[0][0] == p[0]   # the norm is finite: no skip


@pytest.mark.parametrize("fused", ["0", "65536"])
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_non_finite_gradient_skips_the_step(bad, fused, monkeypatch):
    from walker_gym_amd import optim
    monkeypatch.setenv("WG_ADAM_FUSED_MAX", fused)
    rng = np.random.default_rng(5)
    n = 5000
    p, m = rng.standard_normal(n).astype(f32), rng.standard_normal(n).astype(f32)
    v = (rng.standard_normal(n) ** 2).astype(f32)
    g = rng.standard_normal(n).astype(f32)
    g[4321] = bad
    state = np.array([3.0, 0.9 ** 3, 0.999 ** 3, 1.5, 0.25, 2.0, 11.0, 12.0])
    got, want = _direct(p, g, m, v, state, optim.adam_config(max_norm=0.5))
    for a, b, start in zip(got[:3], want[:3], (p, m, v)):
        assert np.array_equal(ac.bits(a), ac.bits(start)) and np.array_equal(ac.bits(b), ac.bits(start))
    assert ac.same(got[3], want[3])
    assert (got[3][:3] == state[:3]).all() and got[3][4] == 0.0 and got[3][5] == 3.0 and (got[3][6:] == state[6:]).all()
    assert not np.isfinite(got[3][3])


# ------------------------------------------------------------------ refusals with device pointers
def test_refusals_with_device_pointers():
    import torch
    from walker_gym_amd import optim
    z = lambda n=64: torch.zeros(n, device=DEV)
    buf = z(256)
    p, g, m, v = buf[0:64], z(), z(), z()
    state, cfg = torch.zeros(8, dtype=torch.float64, device=DEV), optim.adam_config()
    call = lambda **kw: optim.adam_step(**dict(dict(params=[p], grads=[g], ms=[m], vs=[v], state=state, cfg=cfg), **kw))
    with pytest.raises(ValueError, match="m of segment 0 overlaps param of segment 0"):
        call(ms=[buf[63:127]])
    with pytest.raises(ValueError, match="overlaps grad"):
        call(grads=[buf[32:96]])
    with pytest.raises(ValueError, match="v of segment 0 overlaps m of segment 0"):
        call(vs=[m])
    with pytest.raises(ValueError, match="param of segment 1 overlaps param of segment 0"):
        call(params=[p, buf[60:124]], grads=[g, z()], ms=[m, z()], vs=[v, z()])
    with pytest.raises(ValueError, match="overlaps grad .segment 0"):
        call(params=[p, z()], grads=[g, z()], ms=[m, z()], vs=[v, g])
    big = torch.zeros(64, dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError, match="overlaps workspace"):
        call(params=[big.view(torch.float32)[:64]], workspace=big)
    sbuf = torch.zeros(40, dtype=torch.float64, device=DEV)                      # v ends inside the state behind it
    with pytest.raises(ValueError, match="v of segment 0 overlaps state"):
        call(vs=[sbuf.view(torch.float32)[2:66]], state=sbuf[32:40])
    for field, value, word in (("lr", np.inf, "lr"), ("beta1", 1.0, "beta1"), ("beta2", -0.1, "beta2"), ("eps", 0.0, "eps"),
                               ("weight_decay", -1.0, "weight_decay"), ("max_norm", 0.0, "max_norm"),
                               ("max_norm", np.nan, "max_norm")):
        with pytest.raises(ValueError, match=word):
            call(cfg=dict(cfg, **{field: value}))
    with pytest.raises(ValueError):
        call(params=[p] * 33, grads=[g] * 33, ms=[m] * 33, vs=[v] * 33)
    assert (_host(buf) == 0).all() and (_host(state) == 0).all()                 # nothing was launched
    call()                                                                       # and the call they vary goes through
    assert _host(state)[0] == 1.0


# ------------------------------------------------------------------ optim.Adam
def test_adam_class_equals_the_direct_call(monkeypatch):
    import torch
    from walker_gym_amd import optim
    monkeypatch.delenv("WG_ADAM_FUSED_MAX", raising=False)
    rng = np.random.default_rng(9)
    shapes = [(17, 32), (32,), (32, 3), (3,), (5, 7)]
    host = [rng.standard_normal(s).astype(f32) for s in shapes]
    params = [torch.from_numpy(a.copy()).to(DEV).requires_grad_(True) for a in host]
    opt = optim.Adam(params, lr=1e-2, weight_decay=0.01, max_norm=0.5)
    hp, hm, hv = [a.copy() for a in host], [np.zeros_like(a) for a in host], [np.zeros_like(a) for a in host]
    hs = np.zeros(8)
    for s in range(3):
        grads = [rng.standard_normal(sh).astype(f32) for sh in shapes]
        live = [i for i in range(len(shapes)) if not (s == 1 and i == 4)]           # step 1: tensor 4 has no .grad
        for i, t in enumerate(params):
            t.grad = torch.from_numpy(grads[i]).to(DEV) if i in live else None
        lr = None if s < 2 else 5e-3
        opt.step(lr=lr)
        cfg = dict(opt.cfg, lr=opt.cfg["lr"] if lr is None else lr)
        pick = lambda xs: [xs[i] for i in live]
        optim.adam_step_numpy(pick(hp), pick(grads), pick(hm), pick(hv), hs, cfg)
        for i in range(len(shapes)):
            assert ac.same(_host(params[i]), hp[i]) and ac.same(_host(opt.m[i]), hm[i]) and ac.same(_host(opt.v[i]), hv[i])
        assert ac.same(_host(opt.state), hs)
    assert float(opt.steps) == 3 and float(opt.skipped) == 0 and float(opt.grad_norm) == hs[3]
    assert float(opt.clip_coef) == hs[4] < 1
    sd = opt.state_dict()
    other = optim.Adam([torch.zeros_like(t) for t in params])
    other.load_state_dict(sd)
    assert ac.same(_host(other.state), hs) and ac.same(_host(other.m[0]), hm[0]) and other.cfg == opt.cfg
    opt.zero_grad()
    assert all(t.grad is None for t in params)
    with pytest.raises(ValueError):
        optim.Adam([torch.zeros(4, 4, device=DEV).t()])
    with pytest.raises(ValueError):
        optim.Adam([torch.zeros(4, device=DEV, dtype=torch.float64)])
    with pytest.raises(ValueError):
        optim.Adam([torch.zeros(1, device=DEV) for _ in range(33)])


# ------------------------------------------------------------------ the loop closed once on a collected batch
@pytest.mark.parametrize("deep", [False, True], ids=["shallow", "deep"])
def test_ppo_update_from_rows_to_weights(deep):
    import torch
    from walker_gym_amd import optim, pg
    from walker_gym_amd.batched_env import BatchedPhysicsEnv
    from walker_gym_amd.policy import MLPPolicy
    from walker_gym_amd.walker import balance_spec
    torch.manual_seed(0)
    env = BatchedPhysicsEnv(balance_spec(128), in3d=0, max_steps=200, rand_sigma=0.01, seed=0)
    env.enable_auto_reset(on=("done", "nonfinite"), noise_rows=8, final_obs=True)
    N, D, A, H, H2, T = env.N, env.obs_dim, env.batch.A, 16, 8, 16
    p = lambda *s, k: (torch.randn(s, device=env.device) * k).requires_grad_(True)
    w1, b1 = p(1, D, H, k=0.002), p(1, H, k=0.01)
    wm, bm = (p(1, H, H2, k=0.1), p(1, H2, k=0.01)) if deep else (None, None)
    w2, b2 = p(1, H2 if deep else H, A, k=0.01), p(1, A, k=0.01)
    pol = MLPPolicy(w2, b2, w1, b1, wm=wm, bm=bm)
    log_sigma = torch.full((A,), float(np.log(0.3)), device=env.device, requires_grad=True)
    sigma = log_sigma.detach().exp().reshape(1, A).contiguous()
    with torch.no_grad():
        batch = pg.collect(env, pol, sigma, T, 0, 0, lambda rows: torch.zeros(rows.shape[0], device=rows.device))
        obs, u = batch["obs_before"], batch["raw_action"]
        ok = torch.isfinite(batch["adv"]) & torch.isfinite(obs).all(-1) & torch.isfinite(u).all(-1)
        adv = pg.normalize_advantages(batch["adv"], ok)
        old = pg.log_prob_rows(pg.policy_rows_forward(pol, obs, ok), u, sigma.reshape(-1), log_sigma.detach(), ok)
        old = old + 0.05 * torch.randn_like(old)
    assert int(ok.sum()) > T * N // 2
    tensors = [t for t in (w1, b1, wm, bm, w2, b2, log_sigma) if t is not None]
    opt = optim.Adam(tensors, lr=3e-4, max_norm=0.5)
    loss, _ = pg.ppo_surrogate(pg.policy_rows(pol, obs, ok), u, log_sigma, old, adv, ok)
    loss.backward()
    before = [_host(t).copy() for t in tensors]
    grads = [_host(t.grad).copy() for t in tensors]
    assert all(np.abs(g).sum() > 0 for g in grads)
    opt.step()
    hm, hv, hs = [np.zeros_like(a) for a in before], [np.zeros_like(a) for a in before], np.zeros(8)
    want = [a.copy() for a in before]
    optim.adam_step_numpy(want, grads, hm, hv, hs, opt.cfg)
    for t, w, b in zip(tensors, want, before):
        assert ac.same(_host(t), w) and not np.array_equal(w, b)
    assert ac.same(_host(opt.state), hs) and hs[0] == 1


# ------------------------------------------------------------------ EvolutionStrategy(optimizer="adam")
@pytest.mark.parametrize("H2", [0, 4], ids=["shallow", "deep"])
def test_evolution_strategy_with_adam(H2):
    import torch
    from walker_gym_amd import es, optim
    from walker_gym_amd.batched_env import BatchedPhysicsEnv
    from walker_gym_amd.walker import balance_spec
    mk = lambda: BatchedPhysicsEnv(balance_spec(64), in3d=0, max_steps=200, device=DEV)
    env = mk()
    K = es.param_count(env.obs_dim, 8, env.batch.A, True, H2)
    theta0 = (0.05 * np.random.default_rng(2).standard_normal(K)).astype(f32)
    args = dict(hidden=8, hidden2=H2, population=64, sigma=0.05, lr=0.02, seed=4, theta0=theta0)
    tr = es.EvolutionStrategy(env, optimizer="adam", betas=(0.8, 0.99), max_norm=0.1, **args)
    theta, m, v, state = theta0.copy(), np.zeros(K, f32), np.zeros(K, f32), np.zeros(8)
    cfg = optim.adam_config(lr=float(f32(0.02)), betas=(0.8, 0.99), max_norm=0.1, maximize=True)
    for g in range(2):
        out = tr.generation_step(12)
        grad = _host(out["grad"])
        assert np.abs(grad).sum() > 0
        optim.adam_step_numpy([theta], [grad], [m], [v], state, cfg)
        assert ac.same(_host(tr.theta), theta), g
        assert float(out["grad_norm"]) == state[3]
    assert state[0] == 2 and not np.array_equal(theta, theta0)
    sd = tr.state_dict()
    assert ac.same(_host(sd["m"]), m) and ac.same(_host(sd["v"]), v) and ac.same(_host(sd["state"]), state)
    # optimizer=None is the plain step, as before
    plain = es.EvolutionStrategy(mk(), **args)
    out = plain.generation_step(12)
    util = _host(plain.utilities(out["fitness"]))
    want_g, want_t = es.es_update_numpy(theta0, util, 4, 0, 0, 32, 1.0 / (2.0 * 32 * plain.sigma), f32(plain.lr))
    assert ac.same(_host(out["grad"]), want_g) and ac.same(_host(plain.theta), want_t)
    assert "grad_norm" not in out and "m" not in plain.state_dict()


# ------------------------------------------------------------------ pg.normalize_advantages
def test_normalize_advantages_equals_numpy():
    import torch
    from walker_gym_amd import pg
    rng = np.random.default_rng(3)
    T, N = 37, 129
    adv = (3.0 + 2.0 * rng.standard_normal((T, N))).astype(f32)
    mask = rng.uniform(size=(T, N)) < 0.7
    adv[5][~mask[5]] = np.nan                         # a NaN row behind the mask
    adv[7, 3], mask[7, 3] = np.inf, True              # and an unmasked inf, which never enters the sums
    d_adv, d_mask = torch.from_numpy(adv).to(DEV), torch.from_numpy(mask).to(DEV)
    for chunk in (None, 100):
        got = _host(pg.normalize_advantages(d_adv, d_mask, chunk_rows=chunk))
        want = pg.normalize_advantages_numpy(adv, mask, chunk_rows=chunk)
        assert ac.same(got, want)
    fin = mask & np.isfinite(adv)
    assert (got[~mask] == 0).all() and abs(got[fin].mean()) < 1e-5 and abs(got[fin].std() - 1) < 1e-4
    assert ac.same(_host(pg.normalize_advantages(d_adv[0], d_mask[0])), pg.normalize_advantages_numpy(adv[0], mask[0]))
    assert ac.same(_host(pg.normalize_advantages(d_adv[1:3])), pg.normalize_advantages_numpy(adv[1:3]))

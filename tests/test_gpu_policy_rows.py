"""wg_policy_forward / wg_policy_backward against pg.policy_rows_numpy / pg.policy_grad_numpy, bit for bit (NaN == NaN as
in test_gpu_gae.py), the autograd function over them, and the loop they close: on a pg.collect batch the rows' chain
value plus the recorded noise is the recorded raw action, in bits.  The kernels touch no env: the shapes are free."""
import functools

import numpy as np
import pytest

import rows_cases as rc
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
    """Bit-identical, with NaN == NaN (the sign and payload of a produced NaN are no part of the contract)."""
    if a is None or b is None:
        return a is None and b is None
    a, b = _host(a), _host(b)
    na, nb = np.isnan(a), np.isnan(b)
    return a.dtype == b.dtype == np.float32 and a.shape == b.shape and np.array_equal(na, nb) and \
        np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def _dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.array(a, copy=True)).to(DEV)     # (a copy: the shared inputs are read-only)


def _policy(seed, G, D, H, Cc, with_b1, with_b2, device=DEV):
    import torch
    from walker_gym_amd.policy import MLPPolicy
    rng = np.random.default_rng(seed)
    draw = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(f32)).to(device)
    w2 = draw(G, H or D, Cc)
    b2 = draw(G, Cc) if with_b2 else None
    w1 = draw(G, D, H) if H else None
    b1 = draw(G, H) if (H and with_b1) else None
    return MLPPolicy(w2, b2, w1, b1, act_limit=1.0)


def _rows(seed, T, N, D, Cc):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((T, N, D)).astype(f32), rng.standard_normal((T, N, Cc)).astype(f32)


# (T, N), D, C, H, G, b1, b2, chunk_rows.  G = 5 of 65 / 4 of 1000 put a set boundary inside a wave; chunk_rows 1 / 7 / 256
# give a set many chunks, a short last chunk (585 = 83 * 7 + 4; 750 = 2 * 256 + 238) and a single one (126 rows).  The
# forward stages a shared policy's weights in LDS up to 32 KiB (the small G = 1 shapes) and reads the others through L2;
# the backward's register blocks per thread go 1 (small), 2 (155 x 33), 3 (155 x 64) and 4 (191 x 64).
SHAPES = [
    ((1, 1), 1, 1, 0, 1, False, False, 1),
    ((2, 63), 3, 2, 1, 1, True, True, 256),
    ((9, 65), 26, 5, 5, 5, True, False, 7),
    ((9, 65), 155, 8, 33, 65, True, True, 1),
    ((3, 1000), 155, 8, 64, 1, True, True, 256),
    ((3, 1000), 26, 2, 24, 4, False, True, 256),
    ((3, 1000), 3, 5, 0, 1000, True, True, 7),
    ((2, 63), 155, 1, 64, 1, False, False, 7),
    ((9, 65), 26, 8, 24, 1, True, True, 256),
    ((3, 1000), 1, 1, 5, 1, True, True, 7),
    ((9, 65), 155, 5, 0, 5, False, True, 7),
    ((2, 63), 191, 8, 64, 1, True, True, 7),
] + [shape for shape, _ in rc.EDGES]   # the plan's edges (tests/rows_cases.py), each asserted from the restated plan
EDGE_OF = dict(rc.EDGES)


def _blank_mask(T, N, tile, TR):
    """A mask [T, N] without forward tile `tile` (rows tile * TR .. of rho = t * N + w) and without row 0."""
    mask = np.ones(T * N, np.uint8)
    mask[tile * TR:(tile + 1) * TR] = 0
    mask[0] = 0
    return mask.reshape(T, N)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "T%dxN%d-D%d-C%d-H%d-G%d-%d%d-k%d" % (s[0] + s[1:8]))
def test_forward_and_backward_equal_numpy(shape):
    import torch
    from walker_gym_amd import pg
    (T, N), D, Cc, H, G, b1, b2, chunk = shape[:8]
    plan = rc.plan_of(shape)
    for k, v in EDGE_OF.get(shape, {}).items():
        assert plan[k] == v, (k, plan[k], v)
    pol = _policy(sum(shape[1:8]) + T, G, D, H, Cc, b1, b2)
    x, dy = _rows(N + D, T, N, D, Cc)
    mask = None
    if len(shape) > 8:   # a mask that empties one whole forward tile
        assert shape[8] < plan["n_tiles"] - 1
        mask = _blank_mask(T, N, shape[8], plan["fwd_TR"])
        x[mask == 0] = np.nan
        dy[mask == 0] = np.nan
    y = pg.policy_rows_forward(pol, _dev(x), _dev(mask))
    got = pg.policy_rows_backward(pol, _dev(x), _dev(dy), _dev(mask), chunk)
    torch.cuda.synchronize()
    cpu = pol.to("cpu")
    assert tuple(y.shape) == (T, N, Cc) and _same(y, pg.policy_rows_numpy(cpu, x, mask))
    want = pg.policy_grad_numpy(cpu, x, dy, mask, chunk)
    for name, a, b in zip(("w1", "b1", "w2", "b2"), got, want):
        assert _same(a, b), name
        assert a is None or bool(torch.isfinite(a).all())
    assert (got[0] is None) == (H == 0) and (got[1] is None) == (not (H and b1)) and (got[3] is None) == (not b2)


@functools.lru_cache(maxsize=None)
def _masked_case():
    """(9, 65) rows of five sets, chunk_rows 7: a random mask, chunk 1 of set 1 fully masked, set 3 fully masked; every
    masked row holds NaN in x and dy."""
    T, N, D, Cc, H, G, chunk = 9, 65, 26, 5, 5, 5, 7
    n = N // G
    x, dy = _rows(77, T, N, D, Cc)
    rng = np.random.default_rng(78)
    mask = (rng.random((T, N)) < 0.6).astype(np.uint8)
    for rho in range(chunk, 2 * chunk):
        mask[rho // n, 1 * n + rho % n] = 0
    mask[:, 3 * n:4 * n] = 0
    mask[0, 0], mask[0, 1] = 1, 0
    x[mask == 0] = np.nan
    dy[mask == 0] = np.nan
    for a in (x, dy, mask):
        a.setflags(write=False)
    return T, N, D, Cc, H, G, chunk, x, dy, mask


def test_masks_skip_rows_chunks_and_sets():
    import torch
    from walker_gym_amd import pg
    T, N, D, Cc, H, G, chunk, x, dy, mask = _masked_case()
    pol = _policy(79, G, D, H, Cc, True, True)
    cpu = pol.to("cpu")
    for m in (_dev(mask), _dev(mask.astype(bool))):
        y = pg.policy_rows(pol, _dev(x), m)
        got = pg.policy_rows_backward(pol, _dev(x), _dev(dy), m, chunk)
        torch.cuda.synchronize()
        assert _same(y, pg.policy_rows_numpy(cpu, x, mask)) and bool(torch.isfinite(y).all())
        assert bool((y[_dev(mask) == 0] == 0).all())
        want = pg.policy_grad_numpy(cpu, x, dy, mask, chunk)
        for a, b in zip(got, want):
            assert _same(a, b) and bool(torch.isfinite(a).all())
            assert not _host(a)[3].view(np.uint32).any(), "a fully masked set's gradient is +0.0"
            assert _host(a)[[0, 1, 2, 4]].any()
    # an unmasked NaN propagates as the arithmetic says
    x2 = x.copy()
    assert mask[0, 0]
    x2[0, 0, 3] = np.nan
    got = pg.policy_rows_backward(pol, _dev(x2), _dev(dy), _dev(mask), chunk)
    want = pg.policy_grad_numpy(cpu, x2, dy, mask, chunk)
    assert all(_same(a, b) for a, b in zip(got, want))
    assert bool(torch.isnan(got[0][0]).any()) and bool(torch.isfinite(got[0][1:]).all())
    assert _same(pg.policy_rows_forward(pol, _dev(x2), _dev(mask)), pg.policy_rows_numpy(cpu, x2, mask))
    # without a hidden layer the NaN reaches y itself
    lin = _policy(80, 1, D, 0, Cc, False, True)
    y = pg.policy_rows_forward(lin, _dev(x2), _dev(mask))
    assert _same(y, pg.policy_rows_numpy(lin.to("cpu"), x2, mask)) and bool(torch.isnan(y[0, 0]).all())
    assert bool(torch.isfinite(y[1:]).all())


@pytest.mark.parametrize("H,G", [(5, 5), (0, 1)])
def test_step_strides_leave_the_gaps_untouched(H, G):
    """x, y, dy and the mask each with a step stride above the row length: the gaps hold NaN (x, dy), 1 (mask) and a
    sentinel (y), and a skipped row of a caller's y keeps the sentinel."""
    import torch
    from walker_gym_amd import pg
    T, N, D, Cc, _, _, chunk, x, dy, mask = _masked_case()
    pol = _policy(81, G, D, H, Cc, True, True)
    cpu = pol.to("cpu")

    def padded(a, width, pad, fill):
        buf = torch.full((T, N * width + pad), fill, dtype=torch.uint8 if a.dtype == np.uint8 else torch.float32, device=DEV)
        buf[:, :N * width] = _dev(a.reshape(T, N * width))
        shape = (T, N, width) if a.ndim == 3 else (T, N)
        strides = (N * width + pad, width, 1) if a.ndim == 3 else (N + pad, 1)
        return buf, torch.as_strided(buf, shape, strides)
    _, xs = padded(x, D, 5, float("nan"))
    _, ds = padded(dy, Cc, 3, float("nan"))
    _, ms = padded(mask, 1, 7, 1)
    ybuf = torch.full((T, N * Cc + 11), -123.0, device=DEV)
    ys = torch.as_strided(ybuf, (T, N, Cc), (N * Cc + 11, Cc, 1))
    out = pg.policy_rows_forward(pol, xs, ms, y_out=ys)
    got = pg.policy_rows_backward(pol, xs, ds, ms, chunk)
    torch.cuda.synchronize()
    assert out.data_ptr() == ybuf.data_ptr()
    yh, on = ybuf.cpu().numpy(), mask != 0
    want_y = pg.policy_rows_numpy(cpu, x, mask)
    assert (yh[:, N * Cc:] == -123.0).all()
    yr = yh[:, :N * Cc].reshape(T, N, Cc)
    assert _same(yr[on], want_y[on]) and (yr[~on] == -123.0).all()
    assert all(_same(a, b) for a, b in zip(got, pg.policy_grad_numpy(cpu, x, dy, mask, chunk)))
    # a window of a longer buffer is a stride too: steps 2 .. 5 of the same rows
    win = pg.policy_rows_backward(pol, xs[2:6], ds[2:6], ms[2:6], chunk)
    assert all(_same(a, b) for a, b in zip(win, pg.policy_grad_numpy(cpu, x[2:6], dy[2:6], mask[2:6], chunk)))
    # anything else non-contiguous is refused
    with pytest.raises(ValueError):
        pg.policy_rows_forward(pol, xs.transpose(0, 1))
    with pytest.raises(ValueError):
        pg.policy_rows_forward(pol, xs, ms.t())


def test_gradient_subsets_and_determinism():
    import torch
    from walker_gym_amd import pg
    T, N, D, Cc, H, G, chunk, x, dy, mask = _masked_case()
    pol = _policy(82, G, D, H, Cc, True, True)
    args = (pol, _dev(x), _dev(dy), _dev(mask), chunk)
    full = pg.policy_rows_backward(*args)
    again = pg.policy_rows_backward(*args)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(full, again))
    y1, y2 = pg.policy_rows_forward(*args[:2]), pg.policy_rows_forward(*args[:2])
    assert _same(y1, y2)
    wants = [tuple(k != drop for k in range(4)) for drop in range(4)] + [(False, False, True, True), (True, False, False, False),
                                                                         (False, False, False, True)]
    for want in wants:
        part = pg.policy_rows_backward(*args, want=want)
        for k in range(4):
            assert (part[k] is None) == (not want[k])
            assert part[k] is None or torch.equal(part[k].view(torch.int32), full[k].view(torch.int32)), (want, k)
    with pytest.raises(ValueError):
        pg.policy_rows_backward(*args, want=(False,) * 4)
    with pytest.raises(ValueError):
        pg.policy_rows_backward(pol, _dev(x), _dev(dy), _dev(mask), 0)
    with pytest.raises(ValueError):
        pg.policy_rows_forward(pol, _dev(x[:, :63]))            # 63 walkers, five sets
    with pytest.raises(ValueError):
        pg.policy_rows_forward(pol, _dev(x).double())
    with pytest.raises(ValueError):
        pg.policy_rows_forward(pol, _dev(x), y_out=_dev(x))     # y_out of the wrong shape


@pytest.mark.parametrize("shape,full_nt", [(rc.EDGES[2][0], 4), (SHAPES[4], 3)], ids=["1024-blocks", "155x64"])
def test_layer_two_alone_drops_the_layer_one_blocks(shape, full_nt):
    """want = (False, False, True, True) on shapes whose full call is pr_grad_partial<4> / <3>: with g_w1 and g_b1 NULL
    T1 becomes 0 and the launch is <1> (64 and 34 blocks), h is recomputed without dh.  The full call's bits."""
    import torch
    from walker_gym_amd import pg
    (T, N), D, Cc, H, G, b1, b2, chunk = shape
    assert rc.plan_of(shape)["NT"] == full_nt and rc.plan_of(shape, layer1=False)["NT"] == 1
    pol = _policy(90 + D, G, D, H, Cc, b1, b2)
    x, dy = _rows(91 + D, T, N, D, Cc)
    args = (pol, _dev(x), _dev(dy), None, chunk)
    full = pg.policy_rows_backward(*args)
    part = pg.policy_rows_backward(*args, want=(False, False, True, True))
    torch.cuda.synchronize()
    assert part[0] is None and part[1] is None
    for k in (2, 3):
        assert torch.equal(part[k].view(torch.int32), full[k].view(torch.int32)), k
        assert bool(torch.isfinite(part[k]).all()) and bool((part[k] != 0).any())
    want = pg.policy_grad_numpy(pol.to("cpu"), x, dy, None, chunk)
    assert _same(part[2], want[2]) and _same(part[3], want[3])


def test_forward_walks_more_tiles_than_workgroups():
    """199,996 rows of a staged policy: 3,125 tiles of 64 rows on a grid capped at 2,048 workgroups, so 1,077 workgroups
    take a second tile (staged weights reused, xs / hs / ok rewritten behind the closing barrier) and the last tile is
    partial.  A random mask that also blanks one whole second-round tile; y_out holds a sentinel that skipped rows
    keep.  The L2 path's cap of 2^20 workgroups needs over 67 million rows and is deliberately not covered."""
    import torch
    from walker_gym_amd import pg
    (T, N), D, Cc, H, G, b1, b2 = rc.SECOND_TILE
    plan = rc.plan_of(rc.SECOND_TILE)
    assert plan["stage"] and plan["fwd_TR"] == 64 and plan["n_tiles"] == 3125 and plan["grid"] == 2048
    assert (T * N) % 64 == 60, "a partial last tile"
    pol = _policy(95, G, D, H, Cc, b1, b2)
    rng = np.random.default_rng(96)
    x = rng.standard_normal((T, N, D)).astype(f32)
    mask = (rng.random(T * N) < 0.8).astype(np.uint8)
    blank = 2048 + 700                                   # a tile of the second round
    mask[blank * 64:(blank + 1) * 64] = 0
    mask = mask.reshape(T, N)
    x[mask == 0] = np.nan
    y = torch.full((T, N, Cc), -123.0, device=DEV)
    out = pg.policy_rows_forward(pol, _dev(x), _dev(mask), y_out=y)
    torch.cuda.synchronize()
    assert out.data_ptr() == y.data_ptr()
    yh, on = y.cpu().numpy(), mask != 0
    want = pg.policy_rows_numpy(pol.to("cpu"), x, mask)
    assert not (yh[on] == -123.0).any(), "an unskipped row kept the sentinel: a tile was not walked"
    assert _same(yh[on], want[on])
    assert (yh[~on] == -123.0).all() and np.isfinite(yh).all()
    second = np.zeros(T * N, bool)
    second[2048 * 64:] = True                            # the rows only a second iteration reaches
    assert (on.reshape(-1) & second).sum() > 50000


@pytest.mark.parametrize("flat", [False, True])
def test_autograd_gives_the_direct_call(flat):
    import torch
    from walker_gym_amd import pg
    from walker_gym_amd.policy import MLPPolicy
    T, N, D, Cc, H, G, chunk, x, dy, mask = _masked_case()
    if flat:     # [R, D] reads as T = 1, N = R
        x, dy, mask = x.reshape(T * N, D), dy.reshape(T * N, Cc), mask.reshape(T * N)
    base = _policy(83, G, D, H, Cc, True, True)
    w1, b1, w2 = (torch.nn.Parameter(t.clone()) for t in (base.w1, base.b1, base.w2))
    b2 = base.b2.clone()                                         # no requires_grad: no gradient
    pol = MLPPolicy(w2, b2, w1, b1, act_limit=1.0)
    assert pol.w1 is w1 and pol.b1 is b1 and pol.w2 is w2 and pol.b2 is b2
    obs = _dev(x).requires_grad_(True)
    y = pg.policy_rows(pol, obs, _dev(mask))
    assert y.requires_grad and tuple(y.shape) == ((T * N, Cc) if flat else (T, N, Cc))
    dz = _dev(np.where((mask != 0)[..., None], dy, f32(0.5)).astype(f32))
    (y * dz).sum().backward()
    direct = pg.policy_rows_backward(pol, obs.detach(), dz, _dev(mask))
    for p, g in zip((w1, b1, w2), direct):
        assert p.grad is not None and torch.equal(p.grad.view(torch.int32), g.view(torch.int32))
    assert b2.grad is None and obs.grad is None
    x3, dz3, m3 = (x[None], _host(dz)[None], mask[None]) if flat else (x, _host(dz), mask)
    cpu = pol.to("cpu")
    want = pg.policy_grad_numpy(cpu, x3, dz3, m3, pg.default_chunk_rows(x3.shape[0], x3.shape[1] // G))
    assert _same(w1.grad, want[0]) and _same(b1.grad, want[1]) and _same(w2.grad, want[2])
    # an explicit chunk_rows reaches the backward
    for p in (w1, b1, w2):
        p.grad = None
    (pg.policy_rows(pol, obs, _dev(mask), chunk_rows=chunk) * dz).sum().backward()
    assert _same(w1.grad, pg.policy_grad_numpy(cpu, x3, dz3, m3, chunk)[0])
    # nothing that requires grad: no graph; only obs requiring grad: a backward that computes nothing, obs.grad stays None
    assert not pg.policy_rows(base, obs.detach()).requires_grad
    pg.policy_rows(base, obs).sum().backward()
    assert obs.grad is None and base.w2.grad is None


def test_the_rows_close_the_loop_of_a_stochastic_rollout():
    """pg.collect on Balance-v0 x 128, T = 16, H = 5: y of the recorded rows plus RN32(sigma * eps), two roundings, is
    the recorded raw action on every row, bit for bit -- so the first-pass PPO ratio is exactly 1."""
    import torch
    from walker_gym_amd import pg
    from walker_gym_amd.batched_env import BatchedPhysicsEnv
    from walker_gym_amd.policy import MLPPolicy
    from walker_gym_amd.walker import balance_spec
    N, T, max_steps, H = 128, 16, 6, 5
    spec = dict(balance_spec(N))
    rng = np.random.default_rng(9)
    vel = np.array(spec["vel"], f32).reshape(-1, 3).copy()
    vel[:, :2] += rng.uniform(-3, 3, (vel.shape[0], 2)).astype(f32)
    spec.update(vel=vel, steps=(np.arange(N) % max_steps).astype(np.int32))
    env = BatchedPhysicsEnv(spec, device=DEV, in3d=0, max_steps=max_steps)
    env.enable_auto_reset(final_obs=True)
    D, A = env.obs_dim, env.batch.A
    g = torch.Generator().manual_seed(3)
    mk = lambda *s: torch.nn.Parameter((torch.randn(*s, generator=g) * 0.05).to(DEV))
    pol = MLPPolicy(mk(1, H, A), mk(1, A), mk(1, D, H), mk(1, H))
    sigma = (torch.rand(1, A, generator=g) * 0.4 + 0.1).to(DEV)
    wv = (torch.randn(D, generator=g) * 0.01).to(DEV)
    batch = pg.collect(env, pol, sigma, T, 5, 40, lambda rows: rows @ wv, 0.99, 0.95)
    raw, eps = batch["raw_action"], batch["eps"]
    assert bool(torch.isfinite(raw).all()) and bool(torch.isfinite(batch["obs_before"]).all())
    mean = pg.policy_rows(pol, batch["obs_before"])
    u = mean + sigma * eps                                           # RN32(sigma * eps), then RN32(y + .)
    assert torch.equal(u.view(torch.int32), raw.view(torch.int32))
    assert bool((sigma * eps != 0).all()) and not torch.equal(mean, raw)
    # a density on u evaluated at the recorded u under the same mean bits: the first-pass PPO ratio is exactly 1
    logp = lambda m: (-0.5 * ((raw - m) / sigma) ** 2).sum(-1)
    assert torch.equal(torch.exp(logp(mean) - logp(mean.detach())), torch.ones(T, N, device=DEV))
    # and a loss on the rows differentiates: the gradient is wg_policy_backward's of the same dy
    dy = (-batch["adv"][..., None] / batch["adv"].numel()).expand(T, N, A).contiguous()
    (mean * dy).sum().backward()
    want = pg.policy_rows_backward(pol, batch["obs_before"], dy)
    for p, w in zip((pol.w1, pol.b1, pol.w2, pol.b2), want):
        assert torch.equal(p.grad.view(torch.int32), w.view(torch.int32))
    assert bool((pol.w1.grad != 0).any())

"""wg_policy_forward_deep / wg_policy_backward_deep (the row kernels over a policy with a second hidden layer) against
pg.policy_rows_numpy / pg.policy_grad_numpy for all six tensors, bit for bit (NaN == NaN by position), through
pg.policy_rows_forward / policy_rows_backward and the autograd function.  The kernels touch no env: the shapes are free."""
import numpy as np
import pytest

from conftest import gpu_available
from test_gpu_policy_rows import _dev, _host, _same   # (bit-identical with NaN == NaN by position; a device copy)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
f32 = np.float32
NAMES = ("w1", "b1", "wm", "bm", "w2", "b2")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.skip("no ROCm GPU")


def _policy(seed, G, D, H1, H2, Cc, b1, bm, b2, device=DEV, obs_norm=None, grad=False):
    import torch
    from walker_gym_amd.policy import MLPPolicy
    rng = np.random.default_rng(seed)

    def draw(*s):
        t = torch.from_numpy(rng.standard_normal(s).astype(f32)).to(device)
        return t.requires_grad_() if grad else t
    w2, vb2 = draw(G, H2, Cc), draw(G, Cc) if b2 else None
    w1, vb1 = draw(G, D, H1), draw(G, H1) if b1 else None
    wm, vbm = draw(G, H1, H2), draw(G, H2) if bm else None
    return MLPPolicy(w2, vb2, w1, vb1, act_limit=1.0, obs_norm=obs_norm, wm=wm, bm=vbm)


def _rows(seed, T, N, D, Cc):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((T, N, D)).astype(f32), rng.standard_normal((T, N, Cc)).astype(f32)


def blocks(D, H1, H2, Cc):
    up = lambda v: (v + 3) // 4
    return up(D + 1) * up(H1) + up(H1 + 1) * up(H2) + up(H2 + 1) * up(Cc)


def staged(D, H1, H2, Cc, G, b1, bm, b2):
    K = D * H1 + (H1 if b1 else 0) + H1 * H2 + (H2 if bm else 0) + H2 * Cc + (Cc if b2 else 0)
    return G == 1 and 4 * K <= 32 * 1024


# (T, N), D, H1, H2, C, G, b1, bm, b2, chunk_rows.  D + 1, H1, H1 + 1, H2, H2 + 1 and C each off and on a multiple of 4
# (the 4 x 4 blocks' padding, and the bias rows that fall into a block of their own); G = 1 staged in LDS (up to 32 KiB
# with the middle matrix counted) and through L2, G = 5 of 65 with a set boundary inside a wave, G = N; chunk_rows 1 and
# 7 (below the backward's 16-row tile, many chunks, a short last one) and 256 (600 rows: a third, short chunk); each
# bias absent somewhere; register blocks per thread 1 .. 4; the last shape sits on the block limit (1,024 blocks).
SHAPES = [
    ((2, 63), 3, 1, 1, 2, 1, True, True, True, 256),
    ((9, 65), 26, 5, 6, 5, 5, True, False, True, 7),
    ((3, 200), 155, 33, 17, 8, 1, True, True, True, 256),
    ((3, 200), 155, 64, 64, 8, 1, True, True, False, 256),
    ((3, 200), 26, 7, 3, 2, 200, False, True, False, 7),
    ((9, 65), 3, 4, 4, 4, 13, True, True, True, 256),
    ((2, 63), 27, 3, 7, 1, 1, False, False, False, 1),
    ((2, 63), 155, 48, 24, 8, 3, True, True, True, 256),
    ((2, 9), 119, 64, 64, 64, 1, True, True, True, 7),
]
IDS = ["T%dxN%d-D%d-H%dx%d-C%d-G%d-%d%d%d-k%d" % (s[0] + s[1:]) for s in SHAPES]


def test_the_shapes_are_what_they_are_there_for():
    by = lambda f: {bool(f(s)) for s in SHAPES}
    for f in (lambda s: (s[1] + 1) % 4, lambda s: s[2] % 4, lambda s: (s[2] + 1) % 4, lambda s: s[3] % 4,
              lambda s: (s[3] + 1) % 4, lambda s: s[4] % 4):
        assert by(f) == {True, False}
    assert {staged(*s[1:9]) for s in SHAPES if s[5] == 1} == {True, False}
    assert {-(-blocks(*s[1:5]) // 256) for s in SHAPES} == {1, 2, 3, 4}
    assert blocks(*SHAPES[-1][1:5]) == 1024 and blocks(152, 64, 64, 8) * 16 == 14880


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_forward_and_backward_equal_numpy(shape):
    import torch
    from walker_gym_amd import pg
    (T, N), D, H1, H2, Cc, G, b1, bm, b2, chunk = shape
    pol = _policy(sum(shape[1:]) + T, G, D, H1, H2, Cc, b1, bm, b2)
    x, dy = _rows(N + D, T, N, D, Cc)
    y = pg.policy_rows_forward(pol, _dev(x))
    got = pg.policy_rows_backward(pol, _dev(x), _dev(dy), None, chunk)
    torch.cuda.synchronize()
    cpu = pol.to("cpu")
    assert tuple(y.shape) == (T, N, Cc) and _same(y, pg.policy_rows_numpy(cpu, x))
    want = pg.policy_grad_numpy(cpu, x, dy, None, chunk)
    assert len(got) == len(want) == 6
    for name, a, b in zip(NAMES, got, want):
        assert _same(a, b), name
        assert a is None or bool(torch.isfinite(a).all())
    assert [g is None for g in got] == [False, not b1, False, not bm, False, not b2]
    # flat rows [R, D] are T = 1, N = R
    if G == 1:
        yf = pg.policy_rows_forward(pol, _dev(x.reshape(T * N, D)))
        assert tuple(yf.shape) == (T * N, Cc) and _same(yf, _host(y).reshape(T * N, Cc))


def _masked_case():
    """(9, 65) rows of five sets, chunk_rows 7: a random mask, chunk 1 of set 1 fully masked, set 3 fully masked; every
    masked row holds NaN in x and dy."""
    T, N, D, H1, H2, Cc, G, chunk = 9, 65, 26, 5, 6, 5, 5, 7
    n = N // G
    x, dy = _rows(77, T, N, D, Cc)
    mask = (np.random.default_rng(78).random((T, N)) < 0.6).astype(np.uint8)
    for rho in range(chunk, 2 * chunk):
        mask[rho // n, 1 * n + rho % n] = 0
    mask[:, 3 * n:4 * n] = 0
    mask[0, 0], mask[0, 1] = 1, 0
    x[mask == 0] = np.nan
    dy[mask == 0] = np.nan
    return T, N, D, H1, H2, Cc, G, chunk, x, dy, mask


def test_masks_skip_rows_chunks_and_sets():
    import torch
    from walker_gym_amd import pg
    T, N, D, H1, H2, Cc, G, chunk, x, dy, mask = _masked_case()
    pol = _policy(79, G, D, H1, H2, Cc, True, True, True)
    cpu = pol.to("cpu")
    for m in (_dev(mask), _dev(mask.astype(bool))):
        y = pg.policy_rows(pol, _dev(x), m)
        got = pg.policy_rows_backward(pol, _dev(x), _dev(dy), m, chunk)
        torch.cuda.synchronize()
        assert _same(y, pg.policy_rows_numpy(cpu, x, mask)) and bool(torch.isfinite(y).all())
        assert bool((y[_dev(mask) == 0] == 0).all())
        for name, a, b in zip(NAMES, got, pg.policy_grad_numpy(cpu, x, dy, mask, chunk)):
            assert _same(a, b) and bool(torch.isfinite(a).all()), name
            assert not _host(a)[3].view(np.uint32).any(), "a fully masked set's gradient is +0.0"
            assert _host(a)[[0, 1, 2, 4]].any()
    # an unmasked NaN propagates as the arithmetic says: into w1's sums through x, nowhere else (the ReLU clears it)
    x2 = x.copy()
    x2[0, 0, 3] = np.nan
    got = pg.policy_rows_backward(pol, _dev(x2), _dev(dy), _dev(mask), chunk)
    want = pg.policy_grad_numpy(cpu, x2, dy, mask, chunk)
    assert all(_same(a, b) for a, b in zip(got, want))
    assert bool(torch.isnan(got[0][0]).any()) and all(bool(torch.isfinite(g).all()) for g in got[1:])


def test_step_strides_leave_the_gaps_untouched():
    """x, y, dy and the mask each with a step stride above the row length: the gaps hold NaN (x, dy), 1 (mask) and a
    sentinel (y), and a skipped row of a caller's y keeps the sentinel."""
    import torch
    from walker_gym_amd import pg
    T, N, D, H1, H2, Cc, G, chunk, x, dy, mask = _masked_case()
    pol = _policy(81, G, D, H1, H2, Cc, True, True, True)
    cpu = pol.to("cpu")

    def padded(a, width, pad, fill):
        buf = torch.full((T, N * width + pad), fill, dtype=torch.uint8 if a.dtype == np.uint8 else torch.float32, device=DEV)
        buf[:, :N * width] = _dev(a.reshape(T, N * width))
        shape = (T, N, width) if a.ndim == 3 else (T, N)
        strides = (N * width + pad, width, 1) if a.ndim == 3 else (N + pad, 1)
        return torch.as_strided(buf, shape, strides)
    xs, ds, ms = padded(x, D, 5, float("nan")), padded(dy, Cc, 3, float("nan")), padded(mask, 1, 7, 1)
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


@pytest.mark.parametrize("want", [(True, False, False, False, False, False), (False, False, True, True, False, False),
                                  (False, False, False, False, True, True), (False, True, False, False, False, True),
                                  (False, False, False, True, False, False)])
def test_want_subsets(want):
    """A gradient that is not wanted is not computed (without w1 / b1 dh1 is not formed, without wm / bm too neither is
    dh2), and the wanted ones keep their bits."""
    import torch
    from walker_gym_amd import pg
    (T, N), D, H1, H2, Cc, G, b1, bm, b2, chunk = SHAPES[2]
    pol = _policy(91, G, D, H1, H2, Cc, b1, bm, b2)
    x, dy = _rows(92, T, N, D, Cc)
    got = pg.policy_rows_backward(pol, _dev(x), _dev(dy), None, chunk, want=want)
    torch.cuda.synchronize()
    full = pg.policy_grad_numpy(pol.to("cpu"), x, dy, None, chunk)
    for name, k, a, b in zip(NAMES, want, got, full):
        assert (a is None) if not k else _same(a, b), name


@pytest.mark.parametrize("G", [1, 5])
def test_autograd_reaches_the_middle_layer_and_repeats_its_bits(G):
    import torch
    from walker_gym_amd import pg
    T, N, D, H1, H2, Cc, chunk = 4, 65, 26, 9, 6, 3, 7
    pol = _policy(101 + G, G, D, H1, H2, Cc, True, True, True, grad=True)
    x, dy = _rows(102, T, N, D, Cc)
    xd, dyd = _dev(x), _dev(dy)
    grads = []
    for _ in range(2):
        for p in (pol.w1, pol.b1, pol.wm, pol.bm, pol.w2, pol.b2):
            p.grad = None
        y = pg.policy_rows(pol, xd, None, chunk)
        assert y.requires_grad and xd.grad is None
        (y * dyd).sum().backward()
        torch.cuda.synchronize()
        grads.append([p.grad.clone() for p in (pol.w1, pol.b1, pol.wm, pol.bm, pol.w2, pol.b2)])
    detached = _policy(101 + G, G, D, H1, H2, Cc, True, True, True, device="cpu")
    want = pg.policy_grad_numpy(detached, x, dy, None, chunk)
    for name, a, b, c in zip(NAMES, grads[0], grads[1], want):
        assert _same(a, c), name
        assert np.array_equal(_host(a).view(np.uint32), _host(b).view(np.uint32)), name
    # only what requires grad is computed: wm and bm alone
    pol2 = _policy(101 + G, G, D, H1, H2, Cc, True, True, True)
    pol2.wm.requires_grad_(); pol2.bm.requires_grad_()
    (pg.policy_rows(pol2, xd, None, chunk) * dyd).sum().backward()
    assert _same(pol2.wm.grad, want[2]) and _same(pol2.bm.grad, want[3]) and pol2.w1.grad is None and pol2.w2.grad is None


@pytest.mark.parametrize("G", [1, 5])
def test_with_an_obs_norm(G):
    """xn in front of w1 (wg_obs_norm): forward and all six gradients, w1's with xn as the left factor."""
    import torch
    from walker_gym_amd import pg
    from walker_gym_amd.normalize import ObsNorm
    T, N, D, H1, H2, Cc, chunk = 3, 65, 26, 7, 5, 3, 7
    x, dy = _rows(111, T, N, D, Cc)
    x = (x * 40 + 7).astype(f32)
    nm = ObsNorm(D, DEV, clip=1.5)
    nm.update(_dev(x))
    pol = _policy(112 + G, G, D, H1, H2, Cc, True, True, True, obs_norm=nm)
    y = pg.policy_rows_forward(pol, _dev(x))
    got = pg.policy_rows_backward(pol, _dev(x), _dev(dy), None, chunk)
    torch.cuda.synchronize()
    cpu = pol.to("cpu")
    xn = cpu.obs_norm.normalize_numpy(x)
    assert (np.abs(xn) == f32(1.5)).any() and not (np.abs(xn) == f32(1.5)).all()     # the clip engages
    assert _same(y, pg.policy_rows_numpy(cpu, x))
    for name, a, b in zip(NAMES, got, pg.policy_grad_numpy(cpu, x, dy, None, chunk)):
        assert _same(a, b), name
    plain = _policy(112 + G, G, D, H1, H2, Cc, True, True, True)
    assert not _same(y, pg.policy_rows_forward(plain, _dev(x)))


def test_the_rows_close_the_loop_of_a_deep_collect():
    """On a pg.collect batch of a deep policy the rows' chain value plus the recorded noise is the recorded raw action,
    in bits: what the update differentiates is what the rollout kernel evaluated."""
    import torch
    import deep_cases as dc
    from walker_gym_amd import pg
    from walker_gym_amd.batched_env import BatchedPhysicsEnv
    batch = "canonical4"
    cfg = dc.mode_config(batch)
    env = BatchedPhysicsEnv(cfg["spec"], device=DEV, **cfg["params"])
    env.enable_auto_reset(on=("done",), noise=cfg["pool"], final_obs=True)
    pol = dc.mode_policy(batch, DEV)
    sigma = torch.from_numpy(dc.mode_sigma(batch).copy()).to(DEV)
    out = pg.collect(env, pol, sigma, 4, dc.SEED, value_fn=lambda rows: rows[:, 0] * 0)
    y = pg.policy_rows_forward(pol, out["obs_before"])
    n = env.N // pol.G
    srow = sigma.repeat_interleave(n, dim=0)[None]
    u = torch.add(y, torch.mul(srow, out["eps"]))
    torch.cuda.synchronize()
    assert np.array_equal(_host(u).view(np.uint32), _host(out["raw_action"]).view(np.uint32))

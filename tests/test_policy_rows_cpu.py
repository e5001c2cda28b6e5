"""The differentiable policy rows without a GPU: policy_rows_numpy and policy_grad_numpy against a scalar pure-Python
loop (one row, one unit, one element at a time), the math against torch float64 autograd on inputs whose every float32
operation is exact (tolerance 0), every refusal of wg_policy_forward / wg_policy_backward_workspace / wg_policy_backward
before a launch (host pointers, never dereferenced), and the ABI."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from walker_gym_amd import _lib, build, pg
from walker_gym_amd.policy import MLPPolicy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
bits = lambda a: np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def make_policy(rng, G, D, H, Cc, with_b1, with_b2, integers=False):
    draw = (lambda *s: rng.integers(-4, 5, s).astype(f32)) if integers else (lambda *s: rng.standard_normal(s).astype(f32))
    t = torch.from_numpy
    w2 = t(draw(G, H or D, Cc))
    b2 = t(draw(G, Cc)) if with_b2 else None
    w1 = t(draw(G, D, H)) if H else None
    b1 = t(draw(G, H)) if (H and with_b1) else None
    return MLPPolicy(w2, b2, w1, b1, act_limit=1.0)


# ------------------------------------------------------------------ the scalar loop
def scalar_rows(pol, x, dy, mask, chunk_rows):
    """(y, g_w1, g_b1, g_w2, g_b2) by the contract, one scalar operation at a time.  float32 scalars for the chains,
    Python floats (float64) for the sums."""
    host = lambda t: None if t is None else t.numpy()
    w1, b1, w2, b2 = host(pol.w1), host(pol.b1), host(pol.w2), host(pol.b2)
    T, N, D = x.shape
    G, H, Cc = pol.G, pol.H, pol.C
    n, n2, zero = N // G, (H or D), f32(0.0)
    y = np.zeros((T, N, Cc), f32)
    shapes = dict(w1=(D, H) if H else None, b1=(1, H) if b1 is not None else None, w2=(n2, Cc),
                  b2=(1, Cc) if b2 is not None else None)
    out = {k: (None if s is None else np.zeros((G,) + s, f32)) for k, s in shapes.items()}
    with np.errstate(all="ignore"):
        for g in range(G):
            S = {k: [[0.0] * s[1] for _ in range(s[0])] for k, s in shapes.items() if s is not None}
            P = {k: [[0.0] * len(r) for r in v] for k, v in S.items()}

            def close():
                for k in S:
                    for i, row in enumerate(P[k]):
                        for j in range(len(row)):
                            S[k][i][j] = S[k][i][j] + row[j]
                            row[j] = 0.0
            for rho in range(T * n):
                if rho and rho % chunk_rows == 0:
                    close()
                t, r = divmod(rho, n)
                w = g * n + r
                if mask is not None and not mask[t, w]:
                    continue
                row = [f32(v) for v in x[t, w]]
                inp, z = row, None
                if H:
                    z = []
                    for j in range(H):
                        acc = zero if b1 is None else f32(b1[g, j])
                        for i in range(D):
                            acc = f32(acc + f32(row[i] * f32(w1[g, i, j])))
                        z.append(acc)
                    inp = [v if v > 0 else zero for v in z]
                for c in range(Cc):
                    acc = zero if b2 is None else f32(b2[g, c])
                    for i in range(n2):
                        acc = f32(acc + f32(inp[i] * f32(w2[g, i, c])))
                    y[t, w, c] = acc
                d_y = [f32(v) for v in dy[t, w]]
                for i in range(n2):
                    for c in range(Cc):
                        P["w2"][i][c] = P["w2"][i][c] + float(inp[i]) * float(d_y[c])
                if b2 is not None:
                    for c in range(Cc):
                        P["b2"][0][c] = P["b2"][0][c] + 1.0 * float(d_y[c])
                if H:
                    dh = []
                    for j in range(H):
                        d = zero
                        for c in range(Cc):
                            d = f32(d + f32(d_y[c] * f32(w2[g, j, c])))
                        dh.append(d if z[j] > 0 else zero)
                    for i in range(D):
                        for j in range(H):
                            P["w1"][i][j] = P["w1"][i][j] + float(row[i]) * float(dh[j])
                    if b1 is not None:
                        for j in range(H):
                            P["b1"][0][j] = P["b1"][0][j] + 1.0 * float(dh[j])
            close()
            for k in S:
                out[k][g] = np.array(S[k], np.float64).astype(f32)
    sq = lambda a: None if a is None else a[:, 0]
    return y, out["w1"], sq(out["b1"]), out["w2"], sq(out["b2"])


def same(a, b):
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and a.dtype == b.dtype == f32 and np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("H", [0, 1, 5])
@pytest.mark.parametrize("G", [1, 2, "N"])
@pytest.mark.parametrize("biases", ["both", "none", "b1", "b2"])
def test_numpy_restatements_equal_the_scalar_loop(H, G, biases):
    T, N, D, Cc = 3, 4, 3, 2
    G = N if G == "N" else G
    rng = np.random.default_rng(100 * H + 10 * G + len(biases))
    pol = make_policy(rng, G, D, H, Cc, biases in ("both", "b1"), biases in ("both", "b2"))
    x = rng.standard_normal((T, N, D)).astype(f32)
    dy = rng.standard_normal((T, N, Cc)).astype(f32)
    mask = (rng.random((T, N)) < 0.7).astype(np.uint8)
    mask[0, 0], mask[1, 1] = 0, 1
    x[0, 0] = np.nan          # a skipped row may hold anything
    for m in (None, mask):
        xm = x if m is not None else np.nan_to_num(x)
        for chunk in (1, 3, 1000):
            y, *want = scalar_rows(pol, xm, dy, m, chunk)
            got = pg.policy_grad_numpy(pol, xm, dy, m, chunk)
            for name, a, b in zip(("w1", "b1", "w2", "b2"), got, want):
                assert same(a, b), (name, chunk)
                assert a is None or np.isfinite(a).all()
        assert same(pg.policy_rows_numpy(pol, xm, m), y)
    assert (y[0, 0] == 0).all()


def test_numpy_restatements_propagate_an_unskipped_nan_and_check_shapes():
    rng = np.random.default_rng(5)
    pol = make_policy(rng, 2, 3, 5, 2, True, True)
    x = rng.standard_normal((2, 4, 3)).astype(f32)
    dy = rng.standard_normal((2, 4, 2)).astype(f32)
    x[1, 3, 0] = np.nan     # set 1
    y, *want = scalar_rows(pol, x, dy, None, 3)
    got = pg.policy_grad_numpy(pol, x, dy, None, 3)
    assert all(same(a, b) for a, b in zip(got, want))
    assert np.isnan(got[0][1]).any() and np.isfinite(got[0][0]).all()
    # the hidden layer turns a NaN z into h = 0: y and g_w2 of the row stay finite, g_w1 carries x's NaN
    assert np.isfinite(pg.policy_rows_numpy(pol, x)).all() and np.isfinite(got[2]).all()
    with pytest.raises(ValueError):
        pg.policy_grad_numpy(pol, x, dy[:, :, :1])
    with pytest.raises(ValueError):
        pg.policy_grad_numpy(pol, x, dy, None, 0)
    with pytest.raises(ValueError):
        pg.policy_rows_numpy(pol, x[:, :3])      # 3 walkers, 2 sets


# ------------------------------------------------------------------ the math, tolerance 0
@pytest.mark.parametrize("H,G,D", [(0, 1, 29), (5, 1, 29), (7, 3, 11), (4, 6, 5)])
@pytest.mark.parametrize("masked", [False, True])
def test_gradient_is_exact_on_small_integers(H, G, D, masked):
    """x, weights, dy are integers in [-4, 4] and D <= 29: every float32 product and sum is an integer below 2^24, so
    the contract's result is the real-number gradient, which torch float64 autograd also computes exactly."""
    T, N, Cc = 4, 6, 3
    rng = np.random.default_rng(H * 31 + G)
    pol = make_policy(rng, G, D, H, Cc, True, True, integers=True)
    x = rng.integers(-4, 5, (T, N, D)).astype(f32)
    dy = rng.integers(-4, 5, (T, N, Cc)).astype(f32)
    mask = (rng.random((T, N)) < 0.6).astype(np.uint8) if masked else None
    if H:   # on the inputs alone: a quarter of the hidden units on, a quarter off (z == 0 counts as off: relu'(0) = 0)
        sets = np.arange(N) // (N // G)
        z = np.einsum("tni,nij->tnj", x.astype(np.float64), pol.w1.numpy().astype(np.float64)[sets]) + \
            pol.b1.numpy().astype(np.float64)[sets][None]
        on = float((z > 0).mean())
        assert on >= 0.25 and 1 - on >= 0.25, on
    got = pg.policy_grad_numpy(pol, x, dy, mask, chunk_rows=5)
    n = N // G
    for g in range(G):
        p64 = [None if t is None else t[g].double().clone().requires_grad_(True) for t in (pol.w1, pol.b1, pol.w2, pol.b2)]
        w1, b1, w2, b2 = p64
        xs = torch.from_numpy(x[:, g * n:(g + 1) * n]).double()
        inp = torch.relu(xs @ w1 + b1) if H else xs
        yy = inp @ w2 + b2
        wgt = torch.from_numpy(dy[:, g * n:(g + 1) * n]).double()
        if masked:
            wgt = wgt * torch.from_numpy(mask[:, g * n:(g + 1) * n, None].astype(np.float64))
        (yy * wgt).sum().backward()
        for name, a, p in zip(("w1", "b1", "w2", "b2"), got, p64):
            if p is None:
                assert a is None
                continue
            assert np.array_equal(a[g].astype(np.float64), p.grad.numpy()), (name, g)
        if not masked:
            assert np.array_equal(pg.policy_rows_numpy(pol, x)[:, g * n:(g + 1) * n].astype(np.float64),
                                  yy.detach().numpy())


# ------------------------------------------------------------------ the C boundary
@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


class Call:
    """One valid call's arguments over host arrays (never dereferenced: every call made here is refused before a
    launch, or is wg_policy_backward_workspace, which launches nothing)."""

    def __init__(self, T=3, N=6, D=5, H=4, Cc=2, G=2, b1=True, b2=True, chunk=4, pad=0):
        n2 = H or D
        # one arena with 8 KiB between the arrays: a pointer moved by a few hundred bytes meets no other array
        self.arena, self.top = np.zeros(1 << 20, np.uint8), 0

        def carve(shape, dtype):
            size = int(np.prod(shape)) * np.dtype(dtype).itemsize
            at = self.top = (self.top + 8192 + 63) & ~63
            self.top += size
            return self.arena[at:at + size].view(dtype).reshape(shape)
        z = lambda *s: carve(s, f32)
        self.T, self.N, self.D, self.H, self.C, self.G, self.chunk = T, N, D, H, Cc, G, chunk
        self.a = dict(x=z(T, N * D + pad), mask=carve((T, N + pad), np.uint8), y=z(T, N * Cc + pad),
                      dy=z(T, N * Cc + pad), w1=z(G, D, max(H, 1)), b1=z(G, max(H, 1)), w2=z(G, n2, Cc), b2=z(G, Cc),
                      g_w1=z(G, D, max(H, 1)), g_b1=z(G, max(H, 1)), g_w2=z(G, n2, Cc), g_b2=z(G, Cc),
                      workspace=carve((1 << 13,), np.float64))
        if not H:
            self.a.update(w1=None, b1=None, g_w1=None, g_b1=None)
        if not b1:
            self.a.update(b1=None, g_b1=None)
        if not b2:
            self.a.update(b2=None, g_b2=None)
        self.pol = dict(n_sets=G, obs_dim=D, hidden=H, act_dim=Cc, act_limit=1.0)
        self.rows = dict(x_step=N * D + pad, mask_step=N + pad, n_steps=T, N=N)
        self.y_step = self.dy_step = N * Cc + pad

    def p(self, name):
        v = self.a[name]
        return None if v is None else C.c_void_p(v if isinstance(v, int) else v.ctypes.data)

    def structs(self):
        pol = _lib.WgPolicy(w1=self.p("w1"), b1=self.p("b1"), w2=self.p("w2"), b2=self.p("b2"), **self.pol)
        rows = _lib.WgPolicyRows(x=self.p("x"), mask=self.p("mask"), **self.rows)
        return pol, rows

    def forward(self, lib, pol_null=False, rows_null=False):
        pol, rows = self.structs()
        return lib.wg_policy_forward(None if pol_null else C.byref(pol), None if rows_null else C.byref(rows),
                                     self.p("y"), self.y_step, None)

    def workspace(self, lib, pol_null=False, rows_null=False):
        pol, rows = self.structs()
        return lib.wg_policy_backward_workspace(None if pol_null else C.byref(pol),
                                                None if rows_null else C.byref(rows), self.chunk)

    def backward(self, lib, pol_null=False, rows_null=False):
        pol, rows = self.structs()
        return lib.wg_policy_backward(None if pol_null else C.byref(pol), None if rows_null else C.byref(rows),
                                      self.p("dy"), self.dy_step, self.chunk, self.p("workspace"), self.p("g_w1"),
                                      self.p("g_b1"), self.p("g_w2"), self.p("g_b2"), None)


def _expect(lib, rc, code, word, what):
    assert rc == code, (what, rc, lib.wg_last_error())
    assert word in lib.wg_last_error(), (what, lib.wg_last_error())


# (what, changes to the call, a word of the message); the changes: ("a", name, value) an array / pointer, ("pol", ..),
# ("rows", ..) a struct field, ("attr", ..) y_step / dy_step / chunk
SHARED = [
    ("null w2", [("a", "w2", None)], b"null w2"),
    ("null x", [("a", "x", None)], b"null x"),
    ("hidden < 0", [("pol", "hidden", -1)], b"hidden"),
    ("hidden > 256", [("pol", "hidden", 257)], b"hidden"),
    ("hidden without w1", [("a", "w1", None)], b"null w1"),
    ("obs_dim 0", [("pol", "obs_dim", 0)], b"obs_dim"),
    ("act_dim 0", [("pol", "act_dim", 0)], b"act_dim"),
    ("n_sets 0", [("pol", "n_sets", 0)], b"n_sets"),
    ("n_sets not dividing N", [("pol", "n_sets", 4)], b"n_sets"),
    ("n_steps 0", [("rows", "n_steps", 0)], b"n_steps"),
    ("N 0", [("rows", "N", 0)], b"N 0"),
    ("x_step", [("rows", "x_step", 6 * 5 - 1)], b"x_step"),
    ("mask_step", [("rows", "mask_step", 5)], b"mask_step"),
    ("action_out", [("pol", "action_out", 64)], b"action_out"),
    ("return_out", [("pol", "return_out", 64)], b"return_out"),
    ("length_out", [("pol", "length_out", 64)], b"length_out"),
]
FORWARD_ONLY = [
    ("null y", [("a", "y", None)], b"null y"),
    ("y_step", [("attr", "y_step", 6 * 2 - 1)], b"y_step"),
]
BACKWARD_ONLY = [
    ("null dy", [("a", "dy", None)], b"null dy"),
    ("null workspace", [("a", "workspace", None)], b"null workspace"),
    ("dy_step", [("attr", "dy_step", 6 * 2 - 1)], b"dy_step"),
    ("chunk_rows 0", [("attr", "chunk", 0)], b"chunk_rows"),
    ("no gradient wanted", [("a", k, None) for k in ("g_w1", "g_b1", "g_w2", "g_b2")], b"every gradient"),
]


def _apply(call, changes):
    for kind, name, value in changes:
        if kind == "a":
            call.a[name] = value
        elif kind == "pol":
            call.pol[name] = value
        elif kind == "rows":
            call.rows[name] = value
        else:
            setattr(call, name, value)
    return call


@pytest.mark.parametrize("row", SHARED + FORWARD_ONLY, ids=[r[0] for r in SHARED + FORWARD_ONLY])
def test_forward_einval(lib, row):
    what, changes, word = row
    _expect(lib, _apply(Call(), changes).forward(lib), _lib.WG_EINVAL, word, what)
    assert b"wg_policy_forward" in lib.wg_last_error()


@pytest.mark.parametrize("row", SHARED + BACKWARD_ONLY, ids=[r[0] for r in SHARED + BACKWARD_ONLY])
def test_backward_einval(lib, row):
    what, changes, word = row
    _expect(lib, _apply(Call(), changes).backward(lib), _lib.WG_EINVAL, word, what)
    assert b"wg_policy_backward" in lib.wg_last_error()


@pytest.mark.parametrize("row", SHARED + [BACKWARD_ONLY[3]], ids=[r[0] for r in SHARED + [BACKWARD_ONLY[3]]])
def test_workspace_einval(lib, row):
    what, changes, word = row
    _expect(lib, _apply(Call(), changes).workspace(lib), _lib.WG_EINVAL, word, what)


def test_null_structs_and_gradients_without_their_tensor(lib):
    for fn in ("forward", "workspace", "backward"):
        _expect(lib, getattr(Call(), fn)(lib, pol_null=True), _lib.WG_EINVAL, b"null policy", fn)
        _expect(lib, getattr(Call(), fn)(lib, rows_null=True), _lib.WG_EINVAL, b"null rows", fn)
    flat = Call(H=0)
    for k in ("g_w1", "g_b1"):
        c = Call(H=0)
        c.a[k] = np.zeros(64, f32)
        _expect(lib, c.backward(lib), _lib.WG_EINVAL, b"without a hidden layer", k)
    assert flat.workspace(lib) == 2 * 3 * (5 * 2 + 2)
    c = Call(b1=False)
    c.a["g_b1"] = np.zeros(64, f32)
    _expect(lib, c.backward(lib), _lib.WG_EINVAL, b"g_b1", "g_b1 without b1")
    c = Call(b2=False)
    c.a["g_b2"] = np.zeros(64, f32)
    _expect(lib, c.backward(lib), _lib.WG_EINVAL, b"g_b2", "g_b2 without b2")
    # a mask is optional: without one mask_step is not looked at
    c = _apply(Call(), [("a", "mask", None), ("rows", "mask_step", 0), ("a", "y", None)])
    _expect(lib, c.forward(lib), _lib.WG_EINVAL, b"null y", "no mask")


def test_workspace_count(lib):
    # [n_sets][ceil(n_steps * n / chunk_rows)][K], K = w1 + b1 + w2 + b2 with absent biases taking no slot
    assert Call(T=5, N=6, D=3, H=5, Cc=2, G=2, b2=False, chunk=4).workspace(lib) == 2 * 4 * (15 + 5 + 10)
    assert Call(T=5, N=6, D=3, H=5, Cc=2, G=2, b1=False, chunk=4).workspace(lib) == 2 * 4 * (15 + 10 + 2)
    assert Call(T=5, N=6, D=3, H=5, Cc=2, G=6, chunk=5).workspace(lib) == 6 * 1 * 32
    assert Call(T=5, N=6, D=3, H=5, Cc=2, G=1, chunk=1).workspace(lib) == 30 * 32
    assert Call(T=5, N=6, D=3, H=0, Cc=2, G=1, chunk=29).workspace(lib) == 2 * 8
    assert Call(T=1, N=1, D=1, H=0, Cc=1, G=1, b2=False, chunk=1 << 30).workspace(lib) == 1


def _big(D, H, Cc, **kw):
    """Arguments of a shape too large to allocate honestly: the weights are one shared fake array, which the refusal
    under test precedes (ERANGE comes before the aliasing checks) or which wg_policy_backward_workspace never sees."""
    c = Call(T=1, N=1, D=1, H=1 if H else 0, Cc=1, G=1, chunk=1, **kw)
    c.pol.update(obs_dim=D, hidden=H, act_dim=Cc)
    c.rows.update(x_step=D)
    c.y_step = c.dy_step = Cc
    return c


def test_the_k_limit_on_both_sides(lib):
    LIM = _lib.POLICY_GRAD_MAX_K
    assert LIM >= 16384 and f"#define WG_POLICY_GRAD_MAX_K {LIM}" in open(os.path.join(ROOT, "include", "walker_hip.h")).read()
    # no hidden layer, b2 set, C = 4, D + 1 a multiple of 4: K = (D + 1) * 4 is the blocked count too
    assert _big(4095, 0, 4).workspace(lib) == LIM
    for fn in ("workspace", "backward"):
        _expect(lib, getattr(_big(4099, 0, 4), fn)(lib), _lib.WG_ERANGE, b"WG_POLICY_GRAD_MAX_K", fn)
        _expect(lib, getattr(_big(4096, 0, 4), fn)(lib), _lib.WG_ERANGE, b"WG_POLICY_GRAD_MAX_K", fn)
    # the shapes the limit must cover: canonical rows with 64 hidden units, the wide walker with 24
    assert _big(152, 64, 8).workspace(lib) == 152 * 64 + 64 + 64 * 8 + 8
    assert _big(596, 24, 8).workspace(lib) == 596 * 24 + 24 + 24 * 8 + 8
    # with a hidden layer: (D + 1) / 4 = 62 row blocks x 16 column blocks of w1|b1, 17 x 1 of w2|b2
    D, H, Cc = 4 * 62 - 1, 64, 4
    assert 16 * (62 * 16 + 17 * 1) <= LIM and _big(D, H, Cc).workspace(lib) == D * H + H + H * Cc + Cc
    D = 4 * 63 - 1                          # 63 x 16 + 17 = 1025 blocks: 16,400 slots, and K = 16,388
    _expect(lib, _big(D, 64, 4).workspace(lib), _lib.WG_ERANGE, b"WG_POLICY_GRAD_MAX_K", "hidden")
    # K itself within the limit, its 4 x 4 blocking beyond it (one hidden unit pads every block to four columns)
    c = _big(4095, 1, 1)
    assert 4095 + 1 + 1 + 1 <= LIM
    _expect(lib, c.workspace(lib), _lib.WG_ERANGE, b"4 x 4 blocks", "blocked count")
    _expect(lib, c.backward(lib), _lib.WG_ERANGE, b"4 x 4 blocks", "blocked count")
    # the forward has no such limit, only a row's LDS
    _expect(lib, _apply(_big(20000, 0, 1), [("a", "y", None)]).forward(lib), _lib.WG_EINVAL, b"null y", "forward")


def test_the_restated_plan_agrees_with_the_host_at_its_limits(lib):
    """tests/rows_cases.py::plan against wg_policy_backward_workspace, which plans without launching: the two at-limit
    shapes (1,024 blocks behind a hidden layer; K = WG_POLICY_GRAD_MAX_K without one) are accepted, each with one more
    block (one more 4-column group of C, or D + 4) is refused, and the restatement says the same; every edge shape's
    K is the host's count."""
    import rows_cases as rc
    assert rc.MAX_K == _lib.POLICY_GRAD_MAX_K
    for shape in rc.AT_LIMIT:
        _, D, Cc, H, G, b1, b2 = shape[:7]
        p = rc.plan(D, H, Cc, 1, b1, b2)
        assert p["bwd_ok"] and p["blocks"] == 1024 and p["NT"] == 4
        assert _big(D, H, Cc, b1=b1, b2=b2).workspace(lib) == p["K"]
        for d, c in ((D, Cc + 4), (D + 4, Cc)):
            q = rc.plan(d, H, c, 1, b1, b2)
            assert not q["bwd_ok"] and q["blocks"] > 1024, (d, c)
            for fn in ("workspace", "backward"):
                _expect(lib, getattr(_big(d, H, c, b1=b1, b2=b2), fn)(lib), _lib.WG_ERANGE, b"WG_POLICY_GRAD_MAX_K", (fn, d, c))
    for shape, _ in rc.EDGES:
        (T, N), D, Cc, H, G, b1, b2, chunk = shape[:8]
        p = rc.plan_of(shape)
        assert p["bwd_ok"] and 1 <= p["bwd_TR"] <= 16 and 1 <= p["fwd_TR"] <= 64
        assert _big(D, H, Cc, b1=b1, b2=b2).workspace(lib) == p["K"], shape
    # the second-tile shape: staged, 64 rows to a tile, more tiles than the staged grid's cap
    p = rc.plan_of(rc.SECOND_TILE)
    assert p["stage"] and p["fwd_TR"] == 64 and p["n_tiles"] == 3125 > p["grid"] == rc.FWD_CAP


def test_aliasing_is_refused_down_to_one_shared_element(lib):
    def share_last_first(c, out, inp, out_elems, elem=4):
        """`out` placed so that its last element is `inp`'s first."""
        c.a[out] = c.a[inp].ctypes.data - (out_elems - 1) * elem
        return c
    T, N, D, H, Cc, G = 3, 6, 5, 4, 2, 2
    # forward: y against every input
    for inp in ("x", "w1", "b1", "w2", "b2"):
        _expect(lib, share_last_first(Call(), "y", inp, T * N * Cc).forward(lib), _lib.WG_EINVAL, b"y aliases " + inp.encode(), inp)
    c = Call()
    c.a["y"] = c.a["mask"].ctypes.data + T * N - 1 - 3          # y's first float covers the mask's last byte
    _expect(lib, c.forward(lib), _lib.WG_EINVAL, b"y aliases mask", "mask")
    # backward: each output against each input, one element shared
    sizes = dict(g_w1=G * D * H, g_b1=G * H, g_w2=G * H * Cc, g_b2=G * Cc)
    for out, n_out in sizes.items():
        for inp in ("x", "dy", "w1", "b1", "w2", "b2"):
            _expect(lib, share_last_first(Call(), out, inp, n_out).backward(lib), _lib.WG_EINVAL,
                    f"{out} aliases {inp}".encode(), (out, inp))
    n_ws = G * 3 * (D * H + H + H * Cc + Cc)         # chunk_rows 4 over 9 rows per set: 3 chunks
    assert Call().workspace(lib) == n_ws
    for inp in ("x", "dy", "w2"):
        _expect(lib, share_last_first(Call(), "workspace", inp, n_ws, 8).backward(lib), _lib.WG_EINVAL,
                f"workspace aliases {inp}".encode(), inp)
    # outputs against each other
    for out, n_out in sizes.items():
        c = Call()
        c.a[out] = c.a["workspace"].ctypes.data - (n_out - 1) * 4
        _expect(lib, c.backward(lib), _lib.WG_EINVAL, b"aliases workspace", out)
    c = share_last_first(Call(), "g_b2", "g_w2", G * Cc)
    _expect(lib, c.backward(lib), _lib.WG_EINVAL, b"aliases", "g_b2 / g_w2")
    c = share_last_first(Call(), "g_w1", "g_b1", G * D * H)
    _expect(lib, c.backward(lib), _lib.WG_EINVAL, b"aliases", "g_w1 / g_b1")
    # a mask byte under a gradient
    c = Call()
    c.a["g_b2"] = c.a["mask"].ctypes.data + T * N - 1
    _expect(lib, c.backward(lib), _lib.WG_EINVAL, b"g_b2 aliases mask", "mask")


def test_strides_above_the_row_length_pass_the_checks(lib):
    # (the calls stop at the first refusal behind the stride checks)
    c = _apply(Call(pad=3), [("a", "y", None)])
    _expect(lib, c.forward(lib), _lib.WG_EINVAL, b"null y", "padded forward")
    assert Call(pad=3).workspace(lib) == 2 * 3 * (20 + 4 + 8 + 2)


# ------------------------------------------------------------------ the ABI and the package
def test_abi_stays_16_and_the_symbols_are_exported(lib, tmp_path):
    import subprocess
    assert _lib.ABI_VERSION == 16 and lib.wg_abi_version() == 16
    assert "#define WG_ABI_VERSION 16" in open(os.path.join(ROOT, "include", "walker_hip.h")).read()
    new = {"wg_policy_forward", "wg_policy_backward_workspace", "wg_policy_backward"}
    assert new <= set(_lib.EXPORTS)
    for name in new:
        assert getattr(lib, name) is not None
    fields = [f for f, _ in _lib.WgPolicyRows._fields_]
    lines = "".join(f'  printf("{f} %zu\\n", offsetof(wg_policy_rows, {f}));\n' for f in fields)
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "walker_hip.h"\nint main(void) {\n' + lines +
                     '  printf("sizeof %zu\\n", sizeof(wg_policy_rows));\n  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(probe)], check=True)
    got = dict(line.rsplit(" ", 1) for line in
               subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().splitlines())
    assert int(got["sizeof"]) == C.sizeof(_lib.WgPolicyRows)
    for f in fields:
        assert getattr(_lib.WgPolicyRows, f).offset == int(got[f]), f


def test_pg_exports_the_rows_functions():
    for f in ("policy_rows_numpy", "policy_grad_numpy", "policy_rows", "policy_rows_forward", "policy_rows_backward",
              "default_chunk_rows"):
        assert callable(getattr(pg, f))
    assert pg.default_chunk_rows(16, 128) == 256 and pg.default_chunk_rows(64, 65536) == 8192
    assert "nn.Parameter" in MLPPolicy.__doc__
    # MLPPolicy keeps a contiguous parameter by identity: what policy_rows hands to autograd is the caller's leaf
    w2 = torch.nn.Parameter(torch.zeros(1, 3, 2))
    assert MLPPolicy(w2).w2 is w2

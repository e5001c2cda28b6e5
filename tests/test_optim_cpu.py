"""The device optimiser without a GPU: optim.adam_step_numpy against a scalar loop (bit for bit) and against torch's
float64 Adam / AdamW behind clip_grad_norm_ (within a bound derived from the count of float32 roundings), the exact
cases, csrc/wg_adam.h compiled as plain C, wg_adam_step's refusals in the header's order (host placeholder pointers:
nothing is launched), the struct layouts, and the Python surface."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import adam_cases as ac
from conftest import record_metric
from walker_gym_amd import _lib, build, optim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


# ------------------------------------------------------------------ the restatement against a scalar loop
def scalar_adam_step(params, grads, ms, vs, state, cfg):
    """The contract one element and one operation at a time (numpy scalars only: every result is rounded once)."""
    g_all = [f32(x) for g in grads for x in g]
    S = f64(0.0)
    with np.errstate(all="ignore"):
        for lo in range(0, len(g_all), 4096):
            chunk = g_all[lo:lo + 4096]
            q = [f64(0.0)] * 256
            for i, x in enumerate(chunk):
                q[i % 256] = q[i % 256] + f64(x) * f64(x)
            s = 128
            while s >= 1:
                for j in range(s):
                    q[j] = q[j] + q[j + s]
                s //= 2
            S = S + q[0]
        norm = np.sqrt(S)
        state[3] = norm
        if not np.isfinite(S):
            state[4] = 0.0
            state[5] += 1.0
            return
        lr, b1, b2, eps = f32(cfg["lr"]), f32(cfg["beta1"]), f32(cfg["beta2"]), f32(cfg["eps"])
        wd = f32(cfg["weight_decay"])
        t = state[0]
        b1p = (f64(1.0) if t == 0 else state[1]) * f64(b1)
        b2p = (f64(1.0) if t == 0 else state[2]) * f64(b2)
        a, r2 = f32(f64(lr) / (f64(1.0) - b1p)), f32(np.sqrt(f64(1.0) - b2p))
        c = f64(f32(cfg["max_norm"])) / (norm + f64(1e-6))
        cf = f32(c) if c < 1 else f32(1.0)
        state[0], state[1], state[2], state[4] = t + 1.0, b1p, b2p, f64(cf)
        omb1, omb2 = f32(1.0) - b1, f32(1.0) - b2
        for p, g, m, v in zip(params, grads, ms, vs):
            for i in range(p.size):
                gi = -g[i] if cfg["maximize"] else g[i]
                gc = f32(gi * cf)
                m1 = f32(f32(b1 * m[i]) + f32(omb1 * gc))
                v1 = f32(f32(b2 * v[i]) + f32(omb2 * f32(gc * gc)))
                den = f32(f32(np.sqrt(v1) / r2) + eps)
                upd = f32(a * f32(m1 / den))
                p1 = f32(p[i] - f32(f32(lr * wd) * p[i])) if wd != 0 else p[i]
                p[i], m[i], v[i] = f32(p1 - upd), m1, v1


@pytest.mark.parametrize("variant", ["clip-wd-min", "noclip-nowd-max"])
def test_numpy_equals_the_scalar_loop(variant):
    name = "two-edge-at-end"          # 4096 + 100 elements: two chunks, a tree, a second segment
    d, cfg, ref = ac.inputs(name), ac.config(variant), ac.reference(name, variant)
    p, m, v = ([a.copy() for a in d[k]] for k in ("params", "m", "v"))
    state = np.zeros(8)
    for s in range(ac.STEPS):
        scalar_adam_step(p, d["grads"][s], m, v, state, cfg)
        for got, want in zip(p + m + v + [state], ref[s][0] + ref[s][1] + ref[s][2] + [ref[s][3]]):
            assert ac.same(got, want), (variant, s)


def test_references_are_three_real_steps():
    for name in ("one-1", "seven", "thirty-two"):
        for variant, (clip, wd, mx) in ac.VARIANTS.items():
            st = ac.reference(name, variant)[-1][3]
            assert st[0] == ac.STEPS and st[5] == 0 and (st[4] < 1) == clip and 0 < st[1] < 1 and 0 < st[2] < 1
    a, b = ac.reference("seven", "clip-wd-min")[0][0], ac.reference("seven", "clip-wd-max")[0][0]
    assert not all(np.array_equal(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------ against torch's float64 optimiser
@pytest.mark.parametrize("wd", [0.0, 0.01], ids=["adam", "adamw"])
def test_close_to_torch_float64(wd):
    """clip_grad_norm_ + torch.optim.Adam / AdamW in float64 on the same inputs.  The bound is a first-order forward
    error analysis of the float32 chain with u = 2^-24 per rounding, carried from step to step beside the float64
    reference's own values (the float64 side's errors are 2^-29 of these and are covered by gamma's denominator)."""
    import torch
    name = "seven"
    d = ac.inputs(name)
    lr, b1, b2, eps, max_norm = (float(f32(x)) for x in (3e-3, 0.9, 0.999, 1e-8, 2.0))
    cfg = optim.adam_config(lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, max_norm=max_norm)
    wd32 = float(f32(wd))
    p, m, v = ([a.copy() for a in d[k]] for k in ("params", "m", "v"))
    for a in m + v:
        a[...] = 0                       # torch starts from zero moments
    state = np.zeros(8)
    tp = [torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in d["params"]]
    opt = (torch.optim.AdamW(tp, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd32) if wd else
           torch.optim.Adam(tp, lr=lr, betas=(b1, b2), eps=eps))
    u = 2.0 ** -24
    u = u / (1 - 64 * u)                 # gamma: the second-order terms of at most 64 chained roundings
    cat = lambda xs: np.concatenate([np.asarray(x, dtype=f64).reshape(-1) for x in xs])
    e_p = np.zeros(ac.total(name))
    e_m, e_v = e_p.copy(), e_p.copy()
    M, V = e_p.copy(), e_p.copy()        # the float64 reference's moments
    worst = 0.0
    for s in range(ac.STEPS):
        for t, g in zip(tp, d["grads"][s]):
            t.grad = torch.tensor(g, dtype=torch.float64)
        norm = float(torch.nn.utils.clip_grad_norm_(tp, max_norm))
        P0 = cat([t.detach().numpy() for t in tp])
        opt.step()
        optim.adam_step_numpy(p, d["grads"][s], m, v, state, cfg)
        # the float64 values of this step and the float32 chain's error beside them, rounding by rounding
        G = cat(d["grads"][s])
        cfx = min(max_norm / (norm + 1e-6), 1.0)
        gc = G * cfx
        e_gc = 2 * u * np.abs(gc)                                            # cf, the product
        M1 = b1 * M + (1 - b1) * gc
        e_m = b1 * e_m + u * np.abs(b1 * M) + (1 - b1) * e_gc + 2 * u * np.abs((1 - b1) * gc) + u * np.abs(M1)
        V1 = b2 * V + (1 - b2) * gc * gc
        e_v = b2 * e_v + u * b2 * V + (1 - b2) * 2 * np.abs(gc) * e_gc + 3 * u * (1 - b2) * gc * gc + u * V1
        c1, c2 = 1 - b1 ** (s + 1), 1 - b2 ** (s + 1)
        a, r2 = lr / c1, math.sqrt(c2)
        root = np.sqrt(V1)
        e_root = e_v / (2 * root) + u * root
        q = root / r2
        e_q = e_root / r2 + 2 * u * q                                        # r2, the quotient
        den = q + eps
        e_den = e_q + u * den
        w = M1 / den
        e_w = e_m / den + np.abs(M1) * e_den / den ** 2 + u * np.abs(w)
        upd = a * w
        e_upd = a * e_w + 2 * u * np.abs(upd)                                # a, the product
        P1 = P0 * (1 - lr * wd32)
        e_p1 = e_p + (3 * u * np.abs(lr * wd32 * P0) + u * np.abs(P1) if wd else 0.0)
        P = cat([t.detach().numpy() for t in tp])
        e_p = e_p1 + e_upd + u * np.abs(P)
        M, V = M1, V1
        assert (V1 > 0).all()
        err = np.abs(cat(p) - P)
        worst = max(worst, float((err / e_p).max()))
        assert (err <= e_p).all(), (s, float((err / e_p).max()))
        assert abs(state[3] - norm) <= 1e-12 * norm and err.max() > 0
    record_metric(f"adam float32 vs torch float64 ({'adamw' if wd else 'adam'}): max error / derived bound", round(worst, 4))
    record_metric(f"adam float32 vs torch float64 ({'adamw' if wd else 'adam'}): max |error|", float(err.max()))


# ------------------------------------------------------------------ the exact cases
def _one(g, p=None, m=None, v=None, state=None, **kw):
    g = np.asarray(g, f32)
    p = np.linspace(-1, 1, g.size).astype(f32) if p is None else np.asarray(p, f32)
    m = np.zeros_like(g) if m is None else np.asarray(m, f32)
    v = np.zeros_like(g) if v is None else np.asarray(v, f32)
    state = np.zeros(8) if state is None else np.asarray(state, f64)
    info = optim.adam_step_numpy([p], [g], [m], [v], state, optim.adam_config(**kw))
    return p, m, v, state, info


def test_exact_cases():
    rng = np.random.default_rng(0)
    g = rng.standard_normal(300).astype(f32) * 50
    # max_norm = +inf: cf == 1 and gc is g bit for bit, so beta1 = 0 leaves m' = g
    p, m, v, st, info = _one(g, max_norm=math.inf, betas=(0.0, 0.999))
    assert info["cf"] == 1 and st[4] == 1.0 and np.array_equal(ac.bits(m), ac.bits(g))
    # a zeroed state is t = 0, b1p = b2p = 1 (whatever state[1..2] hold at t = 0)
    a = _one(g, max_norm=1.0)
    b = _one(g, max_norm=1.0, state=[0, 0.5, 0.25, 9, 9, 0, 0, 0])
    assert all(ac.same(x, y) for x, y in zip(a[:4], b[:4]))
    assert a[3][0] == 1 and a[3][1] == float(f32(0.9)) and a[3][2] == float(f32(0.999)) and a[3][4] < 1
    # g = 0 with v = 0: upd = +-0, the parameters stay
    p0 = np.linspace(-1, 1, 5).astype(f32)
    p, m, v, st, _ = _one(np.zeros(5), p=p0)
    assert np.array_equal(ac.bits(p), ac.bits(p0)) and (m == 0).all() and (v == 0).all() and st[3] == 0 and st[4] == 1
    # g = 1e-20: g * g is a float32 denormal and is kept;  g = 1e-30: g * g = 0
    p, m, v, st, _ = _one([1e-20, 0])
    assert 0 < v[0] < np.finfo(f32).tiny and np.isfinite(p).all()
    p, m, v, st, _ = _one([1e-30, 0])
    assert v[0] == 0 and m[0] > 0 and np.isfinite(p).all()
    # g = 1e20: g * g = inf in float32, the float64 norm is finite: not skipped, v' = inf, upd = 0
    p, m, v, st, info = _one([1e20, 0], p=[0.5, 0.5])
    assert not info["skipped"] and np.isinf(v[0]) and p[0] == f32(0.5) and st[0] == 1 and np.isfinite(st[3])


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_non_finite_gradient_skips_the_step(bad):
    rng = np.random.default_rng(1)
    g = rng.standard_normal(5000).astype(f32)
    g[4100] = bad
    p0, m0 = rng.standard_normal(5000).astype(f32), rng.standard_normal(5000).astype(f32)
    v0 = (rng.standard_normal(5000) ** 2).astype(f32)
    s0 = np.array([2.0, 0.81, 0.998, 1.0, 1.0, 4.0, 7.0, 8.0])
    p, m, v, st, info = _one(g, p=p0.copy(), m=m0.copy(), v=v0.copy(), state=s0.copy(), max_norm=0.5)
    assert info["skipped"]
    for got, start in ((p, p0), (m, m0), (v, v0)):
        assert got.tobytes() == start.tobytes()
    assert (st[:3] == s0[:3]).all() and not np.isfinite(st[3]) and st[4] == 0 and st[5] == 5 and (st[6:] == s0[6:]).all()


# ------------------------------------------------------------------ csrc/wg_adam.h as plain C
def test_wg_adam_h_compiles_as_c_and_gives_the_same_bits(tmp_path):
    probe = tmp_path / "probe.c"
    probe.write_text(r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "wg_adam.h"
/* stdin: lr b1 b2 eps wd max_norm maximize S n, then 8 state doubles, then n x (g p m v), all as hex bit patterns */
static float rf(void) { unsigned u; if (scanf("%x", &u) != 1) exit(2); float f; memcpy(&f, &u, 4); return f; }
static double rd(void) { unsigned long long u; if (scanf("%llx", &u) != 1) exit(2); double d; memcpy(&d, &u, 8); return d; }
int main(void) {
    float lr = rf(), b1 = rf(), b2 = rf(), eps = rf(), wd = rf(), mn = rf();
    int mx = (int)rf();
    double S = rd();
    int n = (int)rf();
    double st[8];
    for (int i = 0; i < 8; i++) st[i] = rd();
    wg_adam_consts k;
    wg_adam_fixed(lr, b1, b2, eps, wd, mx, &k);
    wg_adam_scalars(S, st, lr, b1, b2, mn, &k);
    for (int i = 0; i < 8; i++) { unsigned long long u; memcpy(&u, &st[i], 8); printf("%llx\n", u); }
    for (int i = 0; i < n; i++) {
        float g = rf(), p = rf(), m = rf(), v = rf();
        if (!k.skip) wg_adam_element(&k, g, &p, &m, &v);
        unsigned a, b, c; memcpy(&a, &p, 4); memcpy(&b, &m, 4); memcpy(&c, &v, 4);
        printf("%x %x %x\n", a, b, c);
    }
    return 0;
}
""")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-O2", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "walker_gym_amd", "csrc"), "-o",
                    str(exe), str(probe), "-lm"], check=True)
    hx = lambda x: format(int(np.asarray(x, f32).view(np.uint32)), "x")
    hd = lambda x: format(int(np.asarray(x, f64).view(np.uint64)), "x")
    rng = np.random.default_rng(4)
    n = 400
    for wd, mx, max_norm, t0 in ((0.0, 0, math.inf, 0), (0.01, 1, 0.5, 3), (0.0, 0, 1e-3, 1)):
        g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)).astype(f32)
        g[:6] = [0.0, -0.0, 1e-20, 1e-30, 1e20, -1e20] if max_norm == math.inf else g[:6]
        p, m = rng.standard_normal(n).astype(f32), (0.1 * rng.standard_normal(n)).astype(f32)
        v = (0.01 * rng.standard_normal(n) ** 2).astype(f32)
        state = np.array([t0, 0.9 ** t0, 0.999 ** t0, 0, 0, 2, 5, 6], f64)
        cfg = optim.adam_config(lr=1e-3, weight_decay=wd, max_norm=max_norm, maximize=mx)
        S = optim.grad_sq_sum_numpy([g])
        words = [hx(cfg[k]) for k in ("lr", "beta1", "beta2", "eps", "weight_decay", "max_norm")] + [hx(mx), hd(S), hx(n)]
        words += [hd(x) for x in state]
        words += [hx(x) for row in zip(g, p, m, v) for x in row]
        out = subprocess.run([str(exe)], input=" ".join(words), capture_output=True, text=True, check=True).stdout.split("\n")
        optim.adam_step_numpy([p], [g], [m], [v], state, cfg)
        got_state = np.array([int(w, 16) for w in out[:8]], np.uint64).view(f64)
        assert ac.same(got_state, state)
        got = np.array([[int(w, 16) for w in line.split()] for line in out[8:8 + n]], np.uint32).view(f32)
        assert ac.same(got[:, 0], p) and ac.same(got[:, 1], m) and ac.same(got[:, 2], v)
    # a sum that is not finite: the scalars skip
    words[7] = hd(np.inf)
    out = subprocess.run([str(exe)], input=" ".join(words), capture_output=True, text=True, check=True).stdout.split("\n")
    st = np.array([int(w, 16) for w in out[:8]], np.uint64).view(f64)
    assert np.isinf(st[3]) and st[4] == 0 and st[5] == 3


# ------------------------------------------------------------------ the C ABI without a launch
def _table(entries):
    t = (_lib.WgOptSegment * max(len(entries), 1))()
    for i, (p, g, m, v, n) in enumerate(entries):
        t[i] = _lib.WgOptSegment(param=p, grad=g, m=m, v=v, n=n)
    return t


MB = 1 << 20


def _seg(i, n=1000, **kw):
    """Placeholder addresses 16 MB apart per segment, 4 MB apart per array."""
    base = (1 + i) * 16 * MB
    d = dict(param=base, grad=base + 4 * MB, m=base + 8 * MB, v=base + 12 * MB, n=n)
    d.update(kw)
    return d["param"], d["grad"], d["m"], d["v"], d["n"]


def test_refusals_in_the_headers_order(lib):
    ok_cfg = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, max_norm=1.0, maximize=0)
    WS, ST = 1024 * MB, 1025 * MB

    def call(entries=None, n=None, cfg=None, seg=True, ws=WS, st=ST, have_cfg=True):
        entries = [_seg(0), _seg(1)] if entries is None else entries
        c = _lib.WgAdam(**dict(ok_cfg, **(cfg or {})))
        rc = lib.wg_adam_step(_table(entries) if seg else None, len(entries) if n is None else n,
                              C.byref(c) if have_cfg else None, ws, st, None)
        return rc, lib.wg_last_error().decode()

    bad_cfg = dict(lr=math.nan, beta1=1.0, beta2=1.5, eps=0.0, weight_decay=-1.0, max_norm=0.0)
    huge = [_seg(0, n=1 << 31)]
    # each row: the call, its code, a word of its message; every later fault is present in every earlier row
    rows = [
        (dict(seg=False, have_cfg=False, ws=None, st=None, n=0), _lib.WG_EINVAL, "null segment table"),
        (dict(have_cfg=False, ws=None, st=None, n=0), _lib.WG_EINVAL, "null cfg"),
        (dict(ws=None, st=None, n=0, cfg=bad_cfg), _lib.WG_EINVAL, "null workspace"),
        (dict(st=None, n=0, cfg=bad_cfg), _lib.WG_EINVAL, "null state"),
        (dict(n=0, cfg=bad_cfg), _lib.WG_EINVAL, "n_segments 0"),
        (dict(n=33, cfg=bad_cfg), _lib.WG_EINVAL, "n_segments 33"),
        (dict(entries=[_seg(0), _seg(1, grad=0), _seg(2, n=0)], cfg=bad_cfg), _lib.WG_EINVAL, "segment 1 has a null pointer"),
        (dict(entries=[_seg(0), _seg(1, n=0), _seg(2, m=0)], cfg=bad_cfg), _lib.WG_EINVAL, "segment 1: n 0 < 1"),
        (dict(entries=huge, cfg=bad_cfg), _lib.WG_EINVAL, "lr"),
        (dict(entries=huge, cfg=dict(bad_cfg, lr=1e-3)), _lib.WG_EINVAL, "beta1"),
        (dict(entries=huge, cfg=dict(bad_cfg, lr=1e-3, beta1=0.0)), _lib.WG_EINVAL, "beta2"),
        (dict(entries=huge, cfg=dict(eps=math.inf, weight_decay=math.nan, max_norm=math.nan)), _lib.WG_EINVAL, "eps"),
        (dict(entries=huge, cfg=dict(weight_decay=math.inf, max_norm=-1.0)), _lib.WG_EINVAL, "weight_decay"),
        (dict(entries=huge, cfg=dict(max_norm=math.nan)), _lib.WG_EINVAL, "max_norm"),
        (dict(entries=huge), _lib.WG_ERANGE, "2^31"),
        (dict(entries=[_seg(0, n=(1 << 31) - 1000), _seg(40, n=1000)]), _lib.WG_ERANGE, "2^31"),
        (dict(entries=[_seg(0), _seg(1, param=16 * MB + 3996)]), _lib.WG_EINVAL, "param of segment 1 overlaps param of segment 0"),
        (dict(entries=[_seg(0, v=16 * MB + 4 * MB + 40)]), _lib.WG_EINVAL, "v of segment 0 overlaps grad"),
        (dict(entries=[_seg(0, m=WS - 3996)]), _lib.WG_EINVAL, "m of segment 0 overlaps workspace"),
        (dict(entries=[_seg(0, param=ST + 60)]), _lib.WG_EINVAL, "param of segment 0 overlaps state"),
        (dict(st=WS + 4), _lib.WG_EINVAL, "workspace overlaps state"),
    ]
    for kw, code, word in rows:
        rc, msg = call(**kw)
        assert rc == code and word in msg, (kw, rc, msg)


def test_workspace_count(lib):
    count = lambda lens: lib.wg_adam_workspace(_table([_seg(i, n=n) for i, n in enumerate(lens)]), len(lens))
    assert [count([n]) for n in (1, 4095, 4096, 4097, 8192, 8193)] == [1, 1, 1, 2, 2, 3]
    assert count([4000, 96]) == 1 and count([4000, 97]) == 2 and count([1] * 32) == 1
    assert count([(1 << 31) - 1]) == 1 << 19
    for name in ac.NAMES:
        assert count([n for n, _ in ac.TABLES[name]]) == (ac.total(name) + 4095) // 4096
    assert count([1 << 31]) == _lib.WG_ERANGE and count([(1 << 31) - 1, 1]) == _lib.WG_ERANGE
    assert lib.wg_adam_workspace(None, 1) == _lib.WG_EINVAL
    t = _table([_seg(0)])
    assert lib.wg_adam_workspace(t, 0) == _lib.WG_EINVAL and lib.wg_adam_workspace(t, 33) == _lib.WG_EINVAL
    assert count([5, 0]) == _lib.WG_EINVAL
    nulls = _table([(0, 0, 0, 0, 10)])
    assert lib.wg_adam_workspace(nulls, 1) == 1          # the count looks at no pointer


def test_struct_layouts_against_a_c_probe(tmp_path):
    probe = tmp_path / "probe.c"
    probe.write_text("""
#include <stdio.h>
#include <stddef.h>
#include "walker_hip.h"
#define F(T, m) printf(#T "." #m " %zu\\n", offsetof(T, m));
int main(void) {
  printf("wg_opt_segment %zu\\nwg_adam %zu\\nmax %d\\n", sizeof(wg_opt_segment), sizeof(wg_adam), WG_OPT_MAX_SEGMENTS);
  F(wg_opt_segment, param) F(wg_opt_segment, grad) F(wg_opt_segment, m) F(wg_opt_segment, v) F(wg_opt_segment, n)
  F(wg_adam, lr) F(wg_adam, beta1) F(wg_adam, beta2) F(wg_adam, eps) F(wg_adam, weight_decay) F(wg_adam, max_norm)
  F(wg_adam, maximize)
  return 0;
}
""")
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(probe)], check=True)
    got = dict(line.rsplit(" ", 1) for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                               check=True).stdout.strip().split("\n"))
    assert int(got["wg_opt_segment"]) == C.sizeof(_lib.WgOptSegment) == 40
    assert int(got["wg_adam"]) == C.sizeof(_lib.WgAdam) == 28
    assert int(got["max"]) == _lib.OPT_MAX_SEGMENTS == optim.MAX_SEGMENTS == 32
    for T, name in ((_lib.WgOptSegment, "wg_opt_segment"), (_lib.WgAdam, "wg_adam")):
        for field, _ in T._fields_:
            assert int(got[f"{name}.{field}"]) == getattr(T, field).offset, (name, field)


def test_abi_exports_and_lazy_index(lib):
    import walker_gym_amd as wg
    assert lib.wg_abi_version() == 16 == _lib.ABI_VERSION
    assert {"wg_adam_workspace", "wg_adam_step"} <= set(_lib.EXPORTS)
    assert wg.Adam is optim.Adam and wg.adam_step_numpy is optim.adam_step_numpy and wg.optim is optim
    assert wg.normalize_advantages is wg.pg.normalize_advantages
    assert wg.normalize_advantages_numpy is wg.pg.normalize_advantages_numpy
    csrc = os.path.join(ROOT, "walker_gym_amd", "csrc")
    for f in ("opt_hip.hip", "wg_adam.h"):
        assert os.path.exists(os.path.join(csrc, f))
    assert os.path.join(csrc, "opt_hip.hip") in build.command()


# ------------------------------------------------------------------ pg.normalize_advantages_numpy
def test_normalize_advantages_numpy_against_a_scalar_loop():
    from walker_gym_amd import pg
    rng = np.random.default_rng(2)
    T, N, chunk = 9, 31, 50
    adv = (1.0 + 3.0 * rng.standard_normal((T, N))).astype(f32)
    mask = rng.uniform(size=(T, N)) < 0.6
    adv[2][~mask[2]] = np.nan
    adv[4, 4], mask[4, 4] = -np.inf, True
    n, S1, S2 = f64(0), f64(0), f64(0)
    flat_a, flat_m = adv.reshape(-1), mask.reshape(-1)
    for lo in range(0, T * N, chunk):
        c, p1, p2 = f64(0), f64(0), f64(0)
        for i in range(lo, min(lo + chunk, T * N)):
            if flat_m[i] and np.isfinite(flat_a[i]):
                x = f64(flat_a[i])
                c, p1, p2 = c + 1, p1 + x, p2 + x * x
        n, S1, S2 = n + c, S1 + p1, S2 + p2
    mean64 = S1 / n
    var = max(S2 / n - mean64 * mean64, 0.0)
    mean, scale = f32(mean64), f32(1.0 / np.sqrt(var + f64(1e-8)))
    want = np.zeros_like(adv)
    with np.errstate(all="ignore"):
        for t in range(T):
            for w in range(N):
                want[t, w] = f32(f32(adv[t, w] - mean) * scale) if mask[t, w] else f32(0)
    got = pg.normalize_advantages_numpy(adv, mask, chunk_rows=chunk)
    assert ac.same(got, want) and np.isinf(got[4, 4]) and (got[~mask] == 0).all()
    # one row without a mask; nothing usable
    one = pg.normalize_advantages_numpy(adv[0], chunk_rows=7)
    assert one.shape == adv[0].shape and one.dtype == f32 and abs(float(one.mean())) < 1e-5
    none = pg.normalize_advantages_numpy(np.full((2, 3), np.nan, f32))
    assert np.isnan(none).all()
    gone = pg.normalize_advantages_numpy(np.ones((2, 3), f32), np.zeros((2, 3), bool))
    assert (gone == 0).all()


# ------------------------------------------------------------------ the trainers' option
def test_trainers_refuse_what_they_do_not_have():
    from walker_gym_amd.es import AdaptiveEvolutionStrategy, EvolutionStrategy
    with pytest.raises(ValueError, match="optimizer"):
        EvolutionStrategy(None, optimizer="bogus")
    with pytest.raises(ValueError, match="optimizer"):
        AdaptiveEvolutionStrategy(None, optimizer="adam")

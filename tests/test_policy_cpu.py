"""The in-kernel policy of wg_rollout_policy without a GPU: MLPPolicy.forward_numpy against a naive scalar restatement
of the arithmetic contract, argument validation, wg_policy's layout against the ctypes mirror, every WG_EINVAL of the
entry point refused before a launch, and the finiteness of every closed loop that the GPU parity tests compare bit for
bit (NaN payloads are not part of the contract)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import policy_cases as pc
from walker_gym_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


# ------------------------------------------------------------------ forward_numpy == the contract, scalar by scalar
def _naive(x, w2, b2, w1, b1, L, sets):
    """The contract in nested Python loops over np.float32 scalars."""
    n = x.shape[0]
    out = np.zeros((n, w2.shape[2]), f32)
    with np.errstate(all="ignore"):
        for r in range(n):
            g = sets[r]
            v = [f32(t) for t in x[r]]
            if w1 is not None:
                h = []
                for j in range(w1.shape[2]):
                    acc = f32(0.0) if b1 is None else f32(b1[g, j])
                    for i in range(w1.shape[1]):
                        acc = f32(acc + f32(v[i] * f32(w1[g, i, j])))
                    h.append(acc if acc > 0 else f32(0.0))
                v = h
            for j in range(w2.shape[2]):
                acc = f32(0.0) if b2 is None else f32(b2[g, j])
                for i in range(w2.shape[1]):
                    acc = f32(acc + f32(v[i] * f32(w2[g, i, j])))
                lim = f32(L)
                out[r, j] = -lim if acc < -lim else (lim if acc > lim else acc)
    return out


def _special_rows(n, D, rng):
    x = (rng.standard_normal((n, D)) * 3).astype(f32)
    x[0, 0] = np.nan
    x[1, 1] = np.inf
    x[2, 2] = -np.inf
    x[3, 3] = -0.0
    x[4, :] = -0.0
    x[5, 0], x[5, 1] = np.inf, -np.inf
    return x


@pytest.mark.parametrize("H,G,bias,L", [(0, 1, True, 1.0), (5, 1, True, 1.0), (5, 3, True, float("inf")),
                                        (0, 3, False, 1.0), (5, 3, False, 1.0), (0, 1, False, float("inf"))])
def test_forward_numpy_equals_naive_scalar_restatement(H, G, bias, L):
    import torch
    from walker_gym_amd.policy import MLPPolicy
    rng = np.random.default_rng(7 + H + G)
    n, D, Cc = 12, 7, 3
    x = _special_rows(n, D, rng)
    n2 = H if H else D
    w1 = (rng.standard_normal((G, D, H)) * 0.5).astype(f32) if H else None
    b1 = (rng.standard_normal((G, H)) * 0.5).astype(f32) if H and bias else None
    w2 = (rng.standard_normal((G, n2, Cc)) * 0.5).astype(f32)
    w2[0, 0, 0] = -0.0
    b2 = (rng.standard_normal((G, Cc)) * 0.5).astype(f32) if bias else None
    t = lambda a: None if a is None else torch.from_numpy(a)
    pol = MLPPolicy(t(w2), t(b2), t(w1), t(b1), act_limit=L)
    assert (pol.D, pol.H, pol.C, pol.G) == (D, H, Cc, G)
    sets = (np.arange(n) // (n // G))
    want = _naive(x, w2, b2, w1, b1, L, sets)
    got = pol.forward_numpy(x)
    assert got.dtype == f32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # a NaN input reaches the output of a linear policy and is cleared by the hidden layer; -0.0 rows keep the bias
    assert np.isnan(got[0]).all() if H == 0 else not np.isnan(got[0]).any()
    if np.isfinite(L):
        assert np.all(np.abs(got[np.isfinite(got)]) <= f32(L))
    # a slice of the rows with its first walker gives the same actions (the parameter sets follow the walker index)
    part = pol.forward_numpy(x[5:9], first_walker=5, n_walkers_total=n)
    assert np.array_equal(part.view(np.uint32), want[5:9].view(np.uint32))
    # the torch restatement (on the host here) gives the same bits
    tt = pol.for_rows(0, n)(torch.from_numpy(x), 0).numpy()
    if G > 1:   # unbound, a policy with several sets does not guess the rows' walkers
        with pytest.raises(ValueError, match="for_rows"):
            pol(torch.from_numpy(x), 0)
    else:
        assert np.array_equal(pol(torch.from_numpy(x), 0).numpy().view(np.uint32), want.view(np.uint32))
    idx = torch.tensor([7, 2, 11, 5])
    scat = pol.for_row_index(idx, n)(torch.from_numpy(x[idx.numpy()]), 0).numpy()
    assert np.array_equal(scat.view(np.uint32), want[idx.numpy()].view(np.uint32))
    assert np.array_equal(tt.view(np.uint32), want.view(np.uint32))
    bound = pol.for_rows(5, n)(torch.from_numpy(x[5:9]), 3).numpy()
    assert np.array_equal(bound.view(np.uint32), want[5:9].view(np.uint32))


def test_mlp_policy_refuses_bad_arguments():
    import torch
    from walker_gym_amd.policy import MLPPolicy
    z = lambda *s: torch.zeros(s)
    MLPPolicy(z(7, 3))                                           # 2-D: one shared set
    assert MLPPolicy(z(2, 5, 3), z(2, 3), z(2, 7, 5), z(2, 5)).G == 2
    with pytest.raises(ValueError):
        MLPPolicy(z(7, 3).double())                              # dtype
    with pytest.raises(ValueError):
        MLPPolicy(np.zeros((7, 3)))                              # float64 numpy
    with pytest.raises(ValueError):
        MLPPolicy(z(7))                                          # rank
    with pytest.raises(ValueError):
        MLPPolicy(z(2, 5, 3), w1=z(3, 7, 5))                     # mismatched G
    with pytest.raises(ValueError):
        MLPPolicy(z(2, 5, 3), w1=z(2, 7, 4))                     # hidden width
    with pytest.raises(ValueError):
        MLPPolicy(z(2, 5, 3), b2=z(2, 4))                        # bias width
    with pytest.raises(ValueError):
        MLPPolicy(z(2, 5, 3), b2=z(3, 3))                        # bias G
    with pytest.raises(ValueError):
        MLPPolicy(z(2, 5, 3), w1=z(2, 7, 5), b1=z(2, 6))
    with pytest.raises(ValueError):
        MLPPolicy(z(7, 3), b1=z(1, 3))                           # b1 without w1
    with pytest.raises(ValueError):
        MLPPolicy(z(7, 3), act_limit=0.0)
    with pytest.raises(ValueError):
        MLPPolicy(z(7, 3), act_limit=float("nan"))
    with pytest.raises(ValueError):
        MLPPolicy(z(3, 7, 3)).forward_numpy(np.zeros((10, 7), f32))   # 10 rows do not divide into 3 sets
    with pytest.raises(ValueError):
        MLPPolicy(z(7, 3)).forward_numpy(np.zeros((10, 6), f32))      # D


# ------------------------------------------------------------------ the C boundary
@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def test_wg_policy_matches_header_and_abi_stays_16(lib, tmp_path):
    fields = [f for f, _ in _lib.WgPolicy._fields_]
    lines = "".join(f'  printf("{f} %zu\\n", offsetof(wg_policy, {f}));\n' for f in fields)
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "walker_hip.h"\nint main(void) {\n' + lines +
                     '  printf("sizeof %zu\\n", sizeof(wg_policy));\n  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(probe)], check=True)
    got = dict(line.rsplit(" ", 1) for line in
               subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().splitlines())
    assert int(got["sizeof"]) == C.sizeof(_lib.WgPolicy)
    for f in fields:
        assert getattr(_lib.WgPolicy, f).offset == int(got[f]), f
    assert _lib.ABI_VERSION == 16 and lib.wg_abi_version() == 16
    assert "wg_rollout_policy" in _lib.EXPORTS


def _batch(**kw):
    """A canonical-shaped uniform batch whose required pointers are non-NULL fakes: every call below is refused before
    anything dereferences them (as tests/test_autoreset_abi.py::_batch)."""
    b = _lib.WgBatch(N=128, M=16, K=40, A=8)
    for f in ("pos", "vel", "acc", "mass", "edges", "inc", "inc_off", "muscle_x", "muscle_bounds", "steps"):
        setattr(b, f, 64)
    for k, v in kw.items():
        setattr(b, k, v)
    return b


def _pol(**kw):
    d = dict(n_sets=1, obs_dim=152, hidden=0, act_dim=8, w2=64, act_limit=1.0)
    d.update(kw)
    return _lib.WgPolicy(**d)


def _call(lib, b, p, pol, n_steps=1, o=None):
    return lib.wg_rollout_policy(C.byref(b), C.byref(p), None if pol is None else C.byref(pol),
                                 None if o is None else C.byref(o), n_steps, None)


P3D = dict(in3d=1)


@pytest.mark.parametrize("what,batch,params,pol,steps,word", [
    ("null policy", {}, P3D, None, 1, b"null policy"),
    ("null w2", {}, P3D, dict(w2=None), 1, b"w2"),
    ("hidden < 0", {}, P3D, dict(hidden=-1), 1, b"hidden"),
    ("hidden > 256", {}, P3D, dict(hidden=257, w1=64), 1, b"hidden"),
    ("hidden without w1", {}, P3D, dict(hidden=24), 1, b"w1"),
    ("act_dim 0", {}, P3D, dict(act_dim=0), 1, b"act_dim"),
    ("act_dim > A", {}, P3D, dict(act_dim=9), 1, b"act_dim"),
    ("obs_dim", {}, P3D, dict(obs_dim=151), 1, b"obs_dim"),
    ("obs_dim 2-D", {}, dict(in3d=0), dict(obs_dim=152), 1, b"obs_dim"),
    ("obs_dim conmid", {}, dict(in3d=1, conmid=1), dict(obs_dim=152), 1, b"obs_dim"),
    ("n_sets 0", {}, P3D, dict(n_sets=0), 1, b"n_sets"),
    ("n_sets not dividing N", {}, P3D, dict(n_sets=3), 1, b"n_sets"),
    ("n_steps 0", {}, P3D, {}, 0, b"n_steps"),
    ("act_limit", {}, P3D, dict(act_limit=0.0), 1, b"act_limit"),
    ("auto_reset", {}, dict(in3d=1, auto_reset=1), {}, 1, b"auto_reset"),
    ("ragged", dict(ragged=2, mass_off=64, edge_off=64, muscle_off=64), P3D, {}, 1, b"lean kernel"),
    ("M not dividing 64", dict(M=12), P3D, dict(obs_dim=3 * 3 * 12 + 8), 1, b"lean kernel"),
    ("spring_mode", {}, dict(in3d=1, spring_mode=1), {}, 1, b"lean kernel"),
    ("pair_mode", {}, dict(in3d=1, pair_mode=1), {}, 1, b"lean kernel"),
])
def test_every_einval_is_refused_before_a_launch(lib, what, batch, params, pol, steps, word):
    rc = _call(lib, _batch(**batch), _lib.WgParams(**params), None if pol is None else _pol(**pol), steps)
    assert rc == _lib.WG_EINVAL, what
    assert word in lib.wg_last_error(), (what, lib.wg_last_error())


def test_lean_off_is_refused(lib, monkeypatch):
    monkeypatch.setenv("WG_LEAN", "0")
    assert _call(lib, _batch(), _lib.WgParams(in3d=1), _pol()) == _lib.WG_EINVAL
    assert b"lean kernel" in lib.wg_last_error()


def test_info_outputs_are_refused(lib):
    o = _lib.WgOutputs(nonfinite=64)
    assert _call(lib, _batch(), _lib.WgParams(in3d=1), _pol(), o=o) == _lib.WG_EINVAL
    assert b"nonfinite" in lib.wg_last_error()


# ------------------------------------------------------------------ the GPU parity cases stay finite on the CPU
@pytest.mark.parametrize("case", pc.CASES + pc.SHAPES, ids=lambda c: c.name)
def test_closed_loop_cases_stay_finite(case):
    """Oracle.step(policy.forward_numpy(obs)) for every (spec, params, policy, T) that the GPU tests compare bit for
    bit: no walker ends non-finite; with act_limit 1 the clip engages; in the done cases every walker's done fires
    before T and not all at the same step."""
    from oracle.oracle import nonfinite
    r = pc.oracle_rollout(case.name)
    assert np.isfinite(r["obs"]).all() and np.isfinite(r["reward"]).all() and np.isfinite(r["action"]).all()
    assert int(nonfinite(r["pos"], r["vel"], r["acc"], r["mass_off"]).sum()) == 0
    assert r["action"].shape == (case.T, r["obs"].shape[1], case.C)
    if np.isfinite(case.L):
        clipped = np.abs(r["action"]) == f32(case.L)
        assert clipped.any() and not clipped.all()
    else:
        assert (np.abs(r["action"]) > 1).any()     # the same weights would have clipped at 1
    assert not np.array_equal(r["action"][1], r["action"][case.T - 1])
    if case.done:
        first = np.where(r["done"].any(axis=0), r["done"].argmax(axis=0), case.T)
        assert (first < case.T - 1).all() and len(np.unique(first)) >= 2


# ------------------------------------------------------------------ the policy-shape cases can see what they are there for
def _masses(case):
    mo = pc.spec_of(case.kind)["mass_off"]
    return int(mo[1] - mo[0])


def test_shapes_cover_the_widths_of_every_tile():
    """The list itself: T = 3, no clip, distinct seeds, each tile's widths, G = 1 / a few / N at least twice per tile
    (N once on the M = 64 tile, whose only width of at most 33 is 1), H = 256 with one and with two sets."""
    assert len({c.seed for c in pc.CASES + pc.COVER + pc.SHAPES}) == len(pc.CASES + pc.COVER + pc.SHAPES)
    assert len({c.name for c in pc.SHAPES}) == len(pc.SHAPES)
    widths = {"m4": [1, 3, 4, 5, 8, 9, 256], "m16": [1, 15, 16, 17, 32, 33, 40, 64, 255, 256],
              "m64": [1, 63, 64, 65, 128, 129, 256], "six": [0, 9]}
    dims = {"m4": (4, 26, 2), "m16": (16, 155, 8), "m64": (64, 596, 20), "six": (4, 42, 6)}
    for tile, want in widths.items():
        cases = [c for c in pc.SHAPES if c.name.startswith(tile + "-")]
        N = len(pc.spec_of(cases[0].kind)["mass_off"]) - 1
        M, D, A = dims[tile]
        assert sorted({c.H for c in cases}) == want, tile
        for c in cases:
            assert (c.T, c.L, c.oracle) == (3, float("inf"), True) and (_masses(c), pc.obs_dim(c)) == (M, D), c
            assert c.wpw == (8 if tile == "six" else 64 // M) and N % c.G == 0 and 1 <= c.C <= A, c
            assert c.G < N or c.H <= 33, c
        if tile != "six":
            assert sorted(c.G for c in cases if c.H == 256) == [1, 2], tile
            assert sum(c.C < A for c in cases) == 1, tile
            assert sum(c.G == 1 for c in cases) >= 2 and sum(1 < c.G < N for c in cases) >= 2, tile
            assert sum(c.G == N for c in cases) >= (1 if tile == "m64" else 2), tile
            if M < 64:   # a set boundary inside a wave tile
                assert sum((N // c.G) % c.wpw != 0 for c in cases if 1 < c.G < N) >= 2, tile
    assert [(c.H, c.C) for c in pc.SHAPES if c.name.startswith("six-")] == [(0, 6), (9, 5), (9, 6)]


def _hidden0(case, w1, b1):
    """Step 0's hidden vectors [N, H], the contract restated: the bias, then the inputs in ascending order."""
    x = pc.entry_rows(case.name)
    sets = np.arange(x.shape[0]) // (x.shape[0] // case.G)
    z = np.zeros((x.shape[0], case.H), f32) if b1 is None else b1[sets].copy()
    for i in range(x.shape[1]):
        z = z + x[:, i:i + 1] * w1[sets, i]
    return np.where(z > 0, z, f32(0.0)).astype(f32)


@pytest.mark.parametrize("case", pc.SHAPES, ids=lambda c: c.name)
def test_shape_cases_can_see_a_wrong_column(case):
    """Conditions on the inputs, from the reference alone: both biases on the odd seeds and neither on the even; every
    hidden unit is on for some walker and off for some walker at step 0; doubling one unit's column of w1 (the first,
    the last, the last one of lane q = 0) changes the bits of some action of step 0; and where C > M, the columns a
    lane takes on its second round differ from those of its first."""
    import torch
    from walker_gym_amd.policy import MLPPolicy
    r = pc.oracle_rollout(case.name)
    w2, b2, w1, b1 = pc.weights(case)
    M = _masses(case)
    assert (b2 is not None) == bool(case.seed % 2)
    rows = pc.entry_rows(case.name)
    act0 = pc.policy_of(case).forward_numpy(rows)
    assert np.array_equal(act0.view(np.uint32), r["action"][0].view(np.uint32))
    if case.H:
        assert (b1 is not None) == bool(case.seed % 2)
        h = _hidden0(case, w1, b1)
        assert (h > 0).any(axis=0).all() and (h == 0).any(axis=0).all()
        t = lambda a: None if a is None else torch.from_numpy(a)
        for j in sorted({0, case.H - 1, (case.H - 1) // M * M}):
            wp = w1.copy()
            wp[:, :, j] *= f32(2.0)
            got = MLPPolicy(t(w2), t(b2), t(wp), t(b1), act_limit=case.L).forward_numpy(rows)
            assert not np.array_equal(got.view(np.uint32), act0.view(np.uint32)), j
    if case.C > M:
        a = r["action"]
        assert (a[:, :, M:] != a[:, :, :case.C - M]).any(axis=(0, 1)).all()
        assert not np.array_equal(a[0][:, M:], a[0][:, :case.C - M])

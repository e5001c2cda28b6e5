"""The FIX instances' tile epilogue through LDS (DESIGN §5 WG_WT): pos, vel and the observation rows of a full wave tile
laid out in the wave's LDS slice as they lie in HBM and stored 16 B per lane, write-through (the default, WG_WT unset
or 1), against the epilogue it replaced (WG_WT=0, the control arm) and the C oracle: every output, the whole state and
the per-step records, bit for bit.  (Round 10's A/B had a third arm, the same image with plain 16-B stores; it did not
pass the keep rule and its code is gone, docs/HISTORY.md.)

Which epilogue ran is read from launch_geometry()["wt_launches"], the library's running count of launches that took the
image epilogue.  A launch takes it only as a FIX launch (512 full tiles of 64 / M walkers at M < 64) of two or more
spring passes whose image fits the spring terms' area of the slice: the one-pass kernel (walker_step_lean1) never does
(its terms' area is at most 2,304 B, pos and vel alone are 1,536 B), so its shape checks that every setting runs
the old epilogue there.

Each shape steps one script under each setting: run() of 3 steps with one walker range and with two, the same again
into record= buffers, then one step().  The oracle steps the same 13 steps once per shape."""
import functools

import numpy as np
import pytest

from conftest import gpu_available

pytestmark = pytest.mark.gpu

STATE = ("pos", "vel", "acc", "muscle_x", "steps", "contact")
OUT = ("obs", "reward", "done", "centroid", "energy")
REC = ("reward", "done", "centroid", "energy")
T = 3
ARMS = (0, 1, None)   # WG_WT: the control arm, the image epilogue asked for, and unset (the default: the image epilogue)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not gpu_available():
        pytest.skip("no ROCm GPU")


def _same(a, b, what, nan_equal=False):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, what
    if a.dtype == np.bool_:
        a = a.astype(np.uint8)
    if b.dtype == np.bool_:
        b = b.astype(np.uint8)
    assert a.dtype == b.dtype, what
    if a.dtype == np.float32:
        both_nan = np.isnan(a) & np.isnan(b) if nan_equal else False   # (the oracle's NaN payloads are its own)
        bad = (a.view(np.uint32) != b.view(np.uint32)) & ~both_nan
    else:
        bad = a != b
    assert not bad.any(), f"{what}: {int(bad.sum())} of {bad.size} elements differ"


def _set_wt(monkeypatch, wt):
    if wt is None:
        monkeypatch.delenv("WG_WT", raising=False)
    else:
        monkeypatch.setenv("WG_WT", str(wt))


def _wt_launches(env) -> int:
    return env.launch_geometry()["wt_launches"]


def _canonical(n, seed=5, **kw):
    from walker_gym_amd.synthetic import canonical_walkers
    return canonical_walkers(n, seed=seed, **kw)


# name: (spec arguments, in3d, the standard tile's walkers, a qualifying launch takes the image epilogue)
SHAPES = {
    "canonical-2048-3d": (dict(n=2048), 1, 4, True),
    "canonical-2048-2d": (dict(n=2048), 0, 4, True),
    "canonical-4160-3d": (dict(n=4160), 1, 4, True),                 # two ranges of 528 and 512 full tiles
    "m4-one-pass-8192": (dict(n=8192, M=4, K=4, A=2), 1, 16, False),   # walker_step_lean1
    "canonical-k64-2048": (dict(n=2048, K=64), 1, 4, True),          # four full spring passes
    "canonical-k64-2048-2d": (dict(n=2048, K=64), 0, 4, True),
    "m64-256": (dict(n=256, M=64, K=120, A=8), 1, 1, True),          # one walker per wave, two passes
    "m64-256-2d": (dict(n=256, M=64, K=120, A=8), 0, 1, True),
}
# the script: (entry, walker ranges, record buffers)
SCRIPT = (("run", 1, False), ("run", 2, False), ("run", 1, True), ("run", 2, True), ("step", 1, False))
N_STEPS = sum(T if e == "run" else 1 for e, _, _ in SCRIPT)


def _spec(name):
    kw = dict(SHAPES[name][0])
    return _canonical(kw.pop("n"), **kw)


def _actions(spec, n_steps, seed=17):
    N = len(spec["mass_off"]) - 1
    A = int(np.max(spec["n_muscles"]))
    return np.random.default_rng(seed).uniform(-1, 1, (n_steps, N, A)).astype(np.float32)


def _oracle_steps(spec, params, acts):
    """The oracle's outputs of every step and its state after each."""
    from oracle.oracle import Oracle
    orc = Oracle(spec, params, n_threads=8)
    steps = []
    for a in acts:
        o = orc.step(a)
        o.update(pos=orc.pos.copy(), vel=orc.vel.copy(), acc=orc.acc.copy(), muscle_x=orc.mx.copy(),
                 steps=orc.steps.copy(), contact=orc.contact.copy())
        steps.append(o)
    return steps


@functools.lru_cache(maxsize=None)
def _oracle_script(name):
    spec = _spec(name)
    return _oracle_steps(spec, dict(in3d=SHAPES[name][1]), _actions(spec, N_STEPS))


def _snapshot(env):
    import torch
    torch.cuda.synchronize()
    return {k: getattr(env, k).cpu().numpy().copy() for k in STATE + OUT}


def _image_ranges(name, lanes):
    """How many of the `lanes` walker ranges of the shape launch the image epilogue unless WG_WT=0."""
    from walker_gym_amd.ranges import uniform_bounds
    kw, _, wpw, image = SHAPES[name]
    if not image:
        return 0
    b = uniform_bounds(kw["n"], lanes)
    sizes = [b[i + 1] - b[i] for i in range(lanes)]
    return sum(1 for n in sizes if n % wpw == 0 and (wpw == 1 or n // wpw >= 512))


def _run_script(monkeypatch, name, wt):
    """The script under WG_WT=wt: a snapshot after each phase (with the record buffers of a record phase) and the image
    launches counted."""
    import torch
    from walker_gym_amd.batched_env import BatchedPhysicsEnv
    spec = _spec(name)
    env = BatchedPhysicsEnv(spec, in3d=SHAPES[name][1])
    acts = torch.as_tensor(_actions(spec, N_STEPS), device="cuda")
    _set_wt(monkeypatch, wt)
    n0, expect, at, snaps = _wt_launches(env), 0, 0, []
    for entry, lanes, record in SCRIPT:
        if entry == "step":
            env.step(acts[at].contiguous())
            at += 1
            expect += _image_ranges(name, env._step_lanes())
            snaps.append((_snapshot(env), None))
            continue
        rec = None
        if record:
            rec = dict(reward=torch.zeros((T, env.N), device="cuda"),
                       done=torch.zeros((T, env.N), dtype=torch.uint8, device="cuda"),
                       centroid=torch.zeros((T, env.N, 3), device="cuda"), energy=torch.zeros((T, env.N), device="cuda"))
        assert env._lanes(lanes) == lanes
        env.run(acts[at:at + T].contiguous(), T, lanes=lanes, record=rec)
        at += T
        expect += T * _image_ranges(name, lanes)
        snap = _snapshot(env)
        snaps.append((snap, None if rec is None else {k: v.cpu().numpy().copy() for k, v in rec.items()}))
    took = _wt_launches(env) - n0
    monkeypatch.delenv("WG_WT", raising=False)
    assert took == (expect if wt != 0 else 0), f"WG_WT={wt}: {took} image launches, expected {expect if wt != 0 else 0}"
    return snaps


@functools.lru_cache(maxsize=None)
def _control(name):
    """WG_WT=0's snapshots of the shape, taken once."""
    mp = pytest.MonkeyPatch()
    try:
        return _run_script(mp, name, 0)
    finally:
        mp.undo()


# ---------------------------------------------------------------- case A: every epilogue, the oracle
@pytest.mark.parametrize("wt", ARMS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_script(monkeypatch, name, wt):
    snaps = _control(name) if wt == 0 else _run_script(monkeypatch, name, wt)
    ref, orc = _control(name), _oracle_script(name)
    at = 0
    for (entry, lanes, record), (snap, rec), (snap0, rec0) in zip(SCRIPT, snaps, ref):
        n = T if entry == "run" else 1
        what = f"{name} WG_WT={wt} {entry} lanes={lanes} record={record}"
        last = orc[at + n - 1]
        for k in STATE:
            _same(snap[k], snap0[k], f"{what}: {k} against WG_WT=0")
            _same(snap[k].reshape(last[k].shape), last[k], f"{what}: {k} against the oracle")
        # (a record run leaves the env's own reward / done / centroid / energy alone: they went to the buffers)
        for k in (("obs",) if record else OUT):
            _same(snap[k], snap0[k], f"{what}: {k} against WG_WT=0")
            _same(snap[k], last[k], f"{what}: {k} against the oracle")
        if record:
            for k in REC:
                _same(rec[k], rec0[k], f"{what}: record {k} against WG_WT=0")
                for s in range(T):
                    _same(rec[k][s], orc[at + s][k], f"{what}: record {k} step {s} against the oracle")
        at += n


# ---------------------------------------------------------------- case B: boundaries
N_FIX = 2048


def _arms_run(monkeypatch, spec, n_steps, image, setup=None, in3d=1, nan_equal=False, lanes=1):
    """run() of n_steps under each setting: equal bits, the oracle's bits, and the epilogue that ran."""
    import torch
    from walker_gym_amd.batched_env import BatchedPhysicsEnv
    acts_h = _actions(spec, n_steps, seed=23)
    orc = _oracle_steps(spec, dict(in3d=in3d), acts_h)[-1]
    acts = torch.as_tensor(acts_h, device="cuda")
    got = {}
    for wt in ARMS:
        env = BatchedPhysicsEnv(spec, in3d=in3d)
        if setup is not None:
            setup(env)
        _set_wt(monkeypatch, wt)
        n0 = _wt_launches(env)
        env.run(acts, n_steps, lanes=lanes)
        got[wt] = _snapshot(env)
        took = _wt_launches(env) - n0
        monkeypatch.delenv("WG_WT", raising=False)
        assert took == (n_steps if image and wt != 0 else 0), f"WG_WT={wt}: {took} image launches"
        D = orc["obs"].shape[1]
        for k in STATE + OUT:
            _same(got[wt][k], got[0][k], f"WG_WT={wt}: {k} against WG_WT=0")
            g = got[wt][k][:, :D] if k == "obs" else got[wt][k].reshape(orc[k].shape)
            _same(g, orc[k], f"WG_WT={wt}: {k} against the oracle", nan_equal=nan_equal)
        assert not got[wt]["obs"][:, D:].any(), "the rows' padding is zero"
    return got


@pytest.mark.parametrize("n_steps", [1, 2])
def test_keep_aux_flip(monkeypatch, n_steps):
    """acc and contact are stored in the last step of a call only (keep_aux): a call of one step, where the first is
    the last, and of two, where it flips between the launches."""
    _arms_run(monkeypatch, _canonical(N_FIX), n_steps, True)


def test_one_walker_short(monkeypatch):
    """2,047 walkers: 511 full tiles and one of three walkers, the generic instance and the old epilogue."""
    _arms_run(monkeypatch, _canonical(N_FIX - 1), 2, False)


def test_padded_obs_stride(monkeypatch):
    """Rows four floats longer than their content: the tile's rows are not one piece of HBM, the old epilogue."""
    import torch

    def pad(env):
        env.obs_dim += 4
        env.obs = torch.zeros((env.N, env.obs_dim), dtype=torch.float32, device=env.device)
    _arms_run(monkeypatch, _canonical(N_FIX), 2, False, setup=pad)


def test_misaligned_obs_base(monkeypatch):
    """The observation rows in a view 4 B into its buffer: no 16-B stores, the old epilogue."""
    import torch

    def shift(env):
        buf = torch.zeros(env.N * env.obs_dim + 1, dtype=torch.float32, device=env.device)
        env.obs = buf[1:].view(env.N, env.obs_dim)
        assert env.obs.data_ptr() % 16 == 4
    _arms_run(monkeypatch, _canonical(N_FIX), 2, False, setup=shift)


# ---------------------------------------------------------------- case C: a diverged walker inside a FIX tile
def test_diverged(monkeypatch):
    """Diverged walkers (the all-NaN stand-in path), partly NaN walkers and walkers at +inf in full tiles: NaN where
    the oracle has NaN (whatever the payload), its bits elsewhere, and the settings' bits equal."""
    from test_gpu_diverged import _diverge
    spec = _diverge(_canonical(N_FIX, seed=21), np.random.default_rng(1), pin=False)
    got = _arms_run(monkeypatch, spec, 3, True, nan_equal=True)
    p = got[None]["pos"].reshape(N_FIX, -1)
    assert int(np.isnan(p).all(axis=1).sum()) >= 20

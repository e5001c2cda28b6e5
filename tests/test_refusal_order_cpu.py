"""Which refusal comes first when two things are wrong at once, without a GPU: run() and rollout_policy() share their
argument checks through helpers, and each wg_* entry keeps the order in which its caller sees them.  Fake non-NULL
pointers, every call refused before a launch (as tests/test_policy_cpu.py)."""
import ctypes as C

import pytest

from walker_gym_amd import _lib, build

SNAPSHOT = ("init_pos", "init_vel", "init_acc", "init_muscle_x")


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def _batch(snapshot=True, episodes=True, **kw):
    """A canonical-shaped uniform batch whose pointers are non-NULL fakes: nothing dereferences them."""
    b = _lib.WgBatch(N=128, M=16, K=40, A=8)
    for f in ("pos", "vel", "acc", "mass", "edges", "inc", "inc_off", "muscle_x", "muscle_bounds", "steps"):
        setattr(b, f, 64)
    for f in SNAPSHOT if snapshot else ():
        setattr(b, f, 64)
    if episodes:
        b.episodes = 64
    for k, v in kw.items():
        setattr(b, k, v)
    return b


def _pol(**kw):
    d = dict(n_sets=1, obs_dim=152, hidden=0, act_dim=8, w2=64, act_limit=1.0)
    d.update(kw)
    return _lib.WgPolicy(**d)


def _step(lib, b, p):
    return lib.wg_step(C.byref(b), C.byref(p), None, 0, 0, 0, None, 1, None, 0, None), lib.wg_last_error()


def _time_step(lib, b, p):
    ms = C.c_float(-1.0)
    rc = lib.wg_time_step(C.byref(b), C.byref(p), None, 0, 0, 0, None, 1, None, 0, None, C.byref(ms))
    assert ms.value == -1.0
    return rc, lib.wg_last_error()


def _run_ranges(lib, b, p):
    rng = (_lib.WgRange * 1)()
    rng[0].batch = C.pointer(b)
    return lib.wg_run_ranges(rng, 1, C.byref(p), None, 0, 0, 0, 1, None), lib.wg_last_error()


# (batch, params, the words of the first refusal)
STEP_ROWS = [
    ("integrator before auto_reset bits", dict(), dict(integrator=3, auto_reset=4), (b"integrator",)),
    ("spring_mode before the snapshot", dict(snapshot=False), dict(spring_mode=3, auto_reset=1), (b"spring_mode",)),
    ("snapshot before episodes", dict(snapshot=False, episodes=False), dict(auto_reset=1), (b"snapshot",)),
    ("bits before the snapshot", dict(snapshot=False), dict(auto_reset=5), (b"bits",)),
    ("auto_reset's pair_mode clause", dict(), dict(auto_reset=1, pair_mode=1), (b"auto_reset", b"pair_mode")),
]


@pytest.mark.parametrize("what,batch,params,words", STEP_ROWS, ids=[r[0] for r in STEP_ROWS])
def test_wg_step_first_refusal(lib, what, batch, params, words):
    rc, err = _step(lib, _batch(**batch), _lib.WgParams(**params))
    assert rc == _lib.WG_EINVAL, what
    assert all(w in err for w in words), (what, err)


@pytest.mark.parametrize("entry", [_time_step, _run_ranges], ids=["wg_time_step", "wg_run_ranges"])
@pytest.mark.parametrize("what,batch,params,words", STEP_ROWS[:3], ids=[r[0] for r in STEP_ROWS[:3]])
def test_check_only_entries_agree_with_wg_step(lib, entry, what, batch, params, words):
    """wg_time_step and wg_run_ranges make run()'s checks through check-only: the same code, the same text."""
    want = _step(lib, _batch(**batch), _lib.WgParams(**params))
    got = entry(lib, _batch(**batch), _lib.WgParams(**params))
    assert got == want and got[0] == _lib.WG_EINVAL, (what, got, want)
    assert all(w in got[1] for w in words), (what, got[1])


_NONE = object()
EPISODE_ROWS = [
    ("act_limit before auto_reset 0", dict(), dict(in3d=1), dict(act_limit=0.0), {}, b"act_limit"),
    ("snapshot before integrator", dict(snapshot=False), dict(in3d=1, auto_reset=1, integrator=3), {}, {}, b"snapshot"),
    ("null stats before integrator", dict(), dict(in3d=1, auto_reset=1, integrator=3), {}, _NONE,
     b"null episode stats"),
]


@pytest.mark.parametrize("what,batch,params,pol,stats,word", EPISODE_ROWS, ids=[r[0] for r in EPISODE_ROWS])
def test_wg_rollout_episodes_first_refusal(lib, what, batch, params, pol, stats, word):
    b, p, pl = _batch(**batch), _lib.WgParams(**params), _pol(**pol)
    st = None if stats is _NONE else _lib.WgEpisodeStats(**stats)
    rc = lib.wg_rollout_episodes(C.byref(b), C.byref(p), C.byref(pl), None, None if st is None else C.byref(st), 1, None)
    assert rc == _lib.WG_EINVAL, what
    assert word in lib.wg_last_error(), (what, lib.wg_last_error())


POLICY_ROWS = [
    ("auto_reset before integrator", dict(in3d=1, auto_reset=1, integrator=3), None, b"auto_reset"),
    ("integrator before the info outputs", dict(in3d=1, integrator=3), dict(nonfinite=64), b"integrator"),
]


@pytest.mark.parametrize("what,params,out,word", POLICY_ROWS, ids=[r[0] for r in POLICY_ROWS])
def test_wg_rollout_policy_first_refusal(lib, what, params, out, word):
    b, p, pl = _batch(), _lib.WgParams(**params), _pol()
    o = None if out is None else _lib.WgOutputs(**out)
    rc = lib.wg_rollout_policy(C.byref(b), C.byref(p), C.byref(pl), None if o is None else C.byref(o), 1, None)
    assert rc == _lib.WG_EINVAL, what
    assert word in lib.wg_last_error(), (what, lib.wg_last_error())

"""wg_rollout_episodes without a GPU: the shared cases (tests/episode_cases.py) exercise what the GPU tests are about
(checked on the composed CPU reference alone), every refusal of the entry point happens before a launch with a message
that names its cause, and wg_episode_stats' layout matches the ctypes mirror."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import episode_cases as ec
from walker_gym_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32


# ------------------------------------------------------------------ the cases cannot pass vacuously
@pytest.mark.parametrize("name", ec.NAMES + ec.SHAPE_NAMES)
def test_cases_reset_often_and_stay_finite(name):
    cfg, ref = ec.config(name), ec.reference(name)
    case, N = cfg["case"], cfg["N"]
    for k in ("pos", "vel", "acc", "obs", "reward", "action"):
        assert np.isfinite(ref[k]).all(), k
    resets = ref["reset"]
    assert resets.shape == (ec.T, N)
    assert (resets.sum(0) >= 2).all(), "every walker resets at least twice"
    assert resets[:, cfg["sunk"]].all(), "the sunk walkers reset at every step"
    assert len(cfg["sunk"]) >= 2
    rows = set()
    for t in range(ec.T):
        rows |= set((ref["ep_before"][t][resets[t] == 1] % 2).tolist())
    assert rows == {0, 1}, "both noise rows are used"
    if case.wpw > 1:   # a wave tile with a reset and a non-reset walker in one step
        w = case.wpw
        n_full = (N // w) * w
        tiles = resets[:, :n_full].reshape(ec.T, -1, w).sum(2)
        assert ((tiles > 0) & (tiles < w)).any()
    assert resets[-1].sum() >= 1, "resets on the last step"
    if np.isfinite(case.L):
        hit = np.abs(ref["action"]) == f32(case.L)
        assert hit.any() and not hit.all()
    # the accounting has something to account: full slots for the sunk walkers, unfilled ones elsewhere
    st = ref["stats"]
    assert (st["episodes"][cfg["sunk"]] == ec.T).all() and (st["episodes"] < ec.SLOTS).any()
    assert np.array_equal(st["episodes"], ref["state"]["episodes"])
    assert np.array_equal(st["length_sum"] + st["tail_length"], np.full(N, ec.T))
    assert np.isnan(st["ep_returns"][st["episodes"] < ec.SLOTS, -1]).all()


def test_accounting_restatement_on_a_hand_case():
    """Two walkers, five steps: one episode of 2 and one of 1 steps and a tail of 2; no reset at all."""
    rew = np.array([[1, .5], [2, .25], [4, .125], [8, 1], [16, 2]], f32)
    rst = np.array([[0, 0], [1, 0], [1, 0], [0, 0], [0, 0]], np.uint8)
    a = ec.accounting(rew, rst, 1)
    assert a["return_sum"].tolist() == [7.0, 0.0] and a["length_sum"].tolist() == [3, 0]
    assert a["episodes"].tolist() == [2, 0] and a["tail_return"].tolist() == [24.0, 3.875]
    assert a["tail_length"].tolist() == [2, 5]
    assert a["ep_returns"][0, 0] == 3.0 and np.isnan(a["ep_returns"][1, 0])
    assert a["ep_lengths"][:, 0].tolist() == [2, -1]


# ------------------------------------------------------------------ the C boundary
@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def test_wg_episode_stats_matches_header(lib, tmp_path):
    fields = [f for f, _ in _lib.WgEpisodeStats._fields_]
    lines = "".join(f'  printf("{f} %zu\\n", offsetof(wg_episode_stats, {f}));\n' for f in fields)
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "walker_hip.h"\nint main(void) {\n' + lines +
                     '  printf("sizeof %zu\\n", sizeof(wg_episode_stats));\n  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(probe)], check=True)
    got = dict(line.rsplit(" ", 1) for line in
               subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().splitlines())
    assert int(got["sizeof"]) == C.sizeof(_lib.WgEpisodeStats)
    for f in fields:
        assert getattr(_lib.WgEpisodeStats, f).offset == int(got[f]), f
    assert _lib.ABI_VERSION == 16 and lib.wg_abi_version() == 16
    assert "wg_rollout_episodes" in _lib.EXPORTS


def _batch(**kw):
    """A canonical-shaped uniform batch with auto-reset's pointers, all non-NULL fakes: every call below is refused
    before anything dereferences them (as tests/test_policy_cpu.py::_batch)."""
    b = _lib.WgBatch(N=128, M=16, K=40, A=8)
    for f in ("pos", "vel", "acc", "mass", "edges", "inc", "inc_off", "muscle_x", "muscle_bounds", "steps",
              "init_pos", "init_vel", "init_acc", "init_muscle_x", "episodes"):
        setattr(b, f, 64)
    for k, v in kw.items():
        setattr(b, k, v)
    return b


def _pol(**kw):
    d = dict(n_sets=1, obs_dim=152, hidden=0, act_dim=8, w2=64, act_limit=1.0)
    d.update(kw)
    return _lib.WgPolicy(**d)


_NONE = object()


def _call(lib, b, p, pol, st, n_steps=1, o=None):
    return lib.wg_rollout_episodes(C.byref(b), C.byref(p), None if pol is None else C.byref(pol),
                                   None if o is None else C.byref(o), None if st is None else C.byref(st), n_steps, None)


AR = dict(in3d=1, auto_reset=1)
P = 128 * 16


@pytest.mark.parametrize("what,batch,params,pol,stats,out,steps,word", [
    # everything wg_rollout_policy refuses, except its auto_reset clause
    ("null policy", {}, AR, None, {}, None, 1, b"null policy"),
    ("null w2", {}, AR, dict(w2=None), {}, None, 1, b"w2"),
    ("hidden < 0", {}, AR, dict(hidden=-1), {}, None, 1, b"hidden"),
    ("hidden > 256", {}, AR, dict(hidden=257, w1=64), {}, None, 1, b"hidden"),
    ("hidden without w1", {}, AR, dict(hidden=24), {}, None, 1, b"w1"),
    ("act_dim 0", {}, AR, dict(act_dim=0), {}, None, 1, b"act_dim"),
    ("act_dim > A", {}, AR, dict(act_dim=9), {}, None, 1, b"act_dim"),
    ("obs_dim", {}, AR, dict(obs_dim=151), {}, None, 1, b"obs_dim"),
    ("obs_dim 2-D", {}, dict(in3d=0, auto_reset=1), dict(obs_dim=152), {}, None, 1, b"obs_dim"),
    ("obs_dim conmid", {}, dict(AR, conmid=1), dict(obs_dim=152), {}, None, 1, b"obs_dim"),
    ("n_sets 0", {}, AR, dict(n_sets=0), {}, None, 1, b"n_sets"),
    ("n_sets not dividing N", {}, AR, dict(n_sets=3), {}, None, 1, b"n_sets"),
    ("n_steps 0", {}, AR, {}, {}, None, 0, b"n_steps"),
    ("act_limit", {}, AR, dict(act_limit=0.0), {}, None, 1, b"act_limit"),
    ("obs_stride", {}, AR, {}, {}, dict(obs=64, obs_stride=151), 1, b"obs_stride"),
    ("ragged", dict(ragged=2, mass_off=64, edge_off=64, muscle_off=64), AR, {}, {}, None, 1, b"lean kernel"),
    ("M not dividing 64", dict(M=12), AR, dict(obs_dim=3 * 3 * 12 + 8), {}, None, 1, b"lean kernel"),
    ("spring_mode", {}, dict(AR, spring_mode=1), {}, {}, None, 1, b"lean kernel"),
    ("pair_mode", {}, dict(AR, pair_mode=1), {}, {}, None, 1, b"lean kernel"),
    ("no muscle_bounds", dict(muscle_bounds=None), AR, {}, {}, None, 1, b"muscle_bounds"),
    ("discrete without stride", {}, dict(AR, action_mode=1), {}, {}, None, 1, b"muscle_stride"),
    # instead of that clause
    ("auto_reset off", {}, dict(in3d=1), {}, {}, None, 1, b"wg_rollout_policy"),
    ("auto_reset bits", {}, dict(in3d=1, auto_reset=4), {}, {}, None, 1, b"bits 1"),
    ("no init_pos", dict(init_pos=None), AR, {}, {}, None, 1, b"snapshot"),
    ("no init_vel", dict(init_vel=None), AR, {}, {}, None, 1, b"snapshot"),
    ("no init_acc", dict(init_acc=None), AR, {}, {}, None, 1, b"snapshot"),
    ("no init_muscle_x", dict(init_muscle_x=None), AR, {}, {}, None, 1, b"snapshot"),
    ("no episodes", dict(episodes=None), AR, {}, {}, None, 1, b"episodes"),
    ("noise rows 0", dict(reset_noise=64, reset_noise_rows=0, reset_noise_stride=3 * P), AR, {}, {}, None, 1,
     b"reset_noise_rows"),
    ("noise stride", dict(reset_noise=64, reset_noise_rows=2, reset_noise_stride=3 * P - 1), AR, {}, {}, None, 1,
     b"reset_noise_stride"),
    # new refusals
    ("null stats", {}, AR, {}, _NONE, None, 1, b"null episode stats"),
    ("ep_slots < 0", {}, AR, {}, dict(ep_slots=-1), None, 1, b"ep_slots"),
    ("ep_return without slots", {}, AR, {}, dict(ep_return=64), None, 1, b"ep_slots 0"),
    ("ep_length without slots", {}, AR, {}, dict(ep_length=64), None, 1, b"ep_slots 0"),
    ("return_out", {}, AR, dict(return_out=64), {}, None, 1, b"return_out"),
    ("length_out", {}, AR, dict(length_out=64), {}, None, 1, b"length_out"),
    ("nonfinite", {}, AR, {}, {}, dict(nonfinite=64), 1, b"nonfinite"),
    ("momentum", {}, AR, {}, {}, dict(momentum=64), 1, b"momentum"),
])
def test_every_einval_is_refused_before_a_launch(lib, what, batch, params, pol, stats, out, steps, word):
    st = None if stats is _NONE else _lib.WgEpisodeStats(**stats)
    o = None if out is None else _lib.WgOutputs(**out)
    rc = _call(lib, _batch(**batch), _lib.WgParams(**params), None if pol is None else _pol(**pol), st, steps, o)
    assert rc == _lib.WG_EINVAL, what
    assert word in lib.wg_last_error(), (what, lib.wg_last_error())


def test_lean_off_is_refused(lib, monkeypatch):
    monkeypatch.setenv("WG_LEAN", "0")
    assert _call(lib, _batch(), _lib.WgParams(**AR), _pol(), _lib.WgEpisodeStats()) == _lib.WG_EINVAL
    assert b"lean kernel" in lib.wg_last_error()


def test_lds_budget_is_erange_with_this_kernels_word_count(lib):
    """The 80 KiB rule counts eight words per walker here, four in wg_rollout_policy: a batch (one M = 64 walker per
    wave, four waves per workgroup) and a hidden width chosen so that the workgroup is exactly 80 KiB with four words is
    WG_ERANGE with eight."""
    M, A = 64, 64
    D = 3 * 3 * M + A
    a16 = lambda n: (n + 15) & ~15

    def lds(K, H, words):   # lean_geo's slice + rows | hidden | actions | the walker's words, four waves
        pl = (K + 3) & ~3
        sl = a16(pl * 24) + a16(pl * 12) + a16(K * 4 + 4) + a16(A * 4)
        return 4 * (sl + a16(D * 4) + a16(H * 4) + a16(A * 4) + 4 * words)
    found = next(((K, H) for K in range(64, 513) for H in range(4, 257, 4) if lds(K, H, 4) == 80 * 1024), None)
    assert found is not None
    K, H = found
    assert lds(K, H, 8) > 80 * 1024
    b = _batch(N=8192, M=M, K=K, A=A)
    pol = _pol(obs_dim=D, hidden=H, w1=64, act_dim=A)
    assert _call(lib, b, _lib.WgParams(**AR), pol, _lib.WgEpisodeStats()) == _lib.WG_ERANGE
    assert b"LDS" in lib.wg_last_error() and b"wg_rollout_episodes" in lib.wg_last_error()

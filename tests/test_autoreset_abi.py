"""Auto-reset (ABI 16) at the C boundary, without a GPU: the new trailing fields of wg_params / wg_batch / wg_outputs sit
where the ctypes mirrors say, and every argument error of an auto-reset call is refused with WG_EINVAL and a message
that names its cause before any launch; with auto_reset = 0 and the new fields NULL a call validates as it did."""
import ctypes as C
import os
import subprocess

import pytest

from walker_gym_amd import _lib, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_FIELDS = {
    "wg_params": ("auto_reset",),
    "wg_batch": ("init_pos", "init_vel", "init_acc", "init_muscle_x", "reset_noise", "reset_noise_rows",
                 "reset_noise_stride", "episodes"),
    "wg_outputs": ("reset", "final_obs"),
}
MIRROR = {"wg_params": "WgParams", "wg_batch": "WgBatch", "wg_outputs": "WgOutputs"}


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


def test_abi_version_is_16(lib):
    assert _lib.ABI_VERSION == 16 and lib.wg_abi_version() == 16


def test_new_fields_match_header(tmp_path):
    """A C probe prints sizeof and offsetof of every ABI 16 field; the ctypes mirrors agree, and the fields are trailing
    (each struct's earlier fields keep their offsets: the last ABI 15 field comes before the first new one)."""
    lines = "".join(f'  printf("{s}.{f} %zu\\n", offsetof({s}, {f}));\n' for s, fs in NEW_FIELDS.items() for f in fs)
    probe = tmp_path / "probe.c"
    probe.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "walker_hip.h"\nint main(void) {\n' + lines +
                     '  printf("wg_params %zu\\nwg_batch %zu\\nwg_outputs %zu\\n", sizeof(wg_params), sizeof(wg_batch),'
                     ' sizeof(wg_outputs));\n  return 0;\n}\n')
    exe = tmp_path / "probe"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(probe)], check=True)
    got = dict(line.rsplit(" ", 1) for line in
               subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.strip().splitlines())
    for s, fs in NEW_FIELDS.items():
        cls = getattr(_lib, MIRROR[s])
        assert int(got[s]) == C.sizeof(cls), s
        for f in fs:
            assert getattr(cls, f).offset == int(got[f"{s}.{f}"]), f"{s}.{f}"
    assert _lib.WgParams.friction_mode.offset < _lib.WgParams.auto_reset.offset
    assert _lib.WgBatch.kc.offset < _lib.WgBatch.init_pos.offset
    assert _lib.WgOutputs.momentum.offset < _lib.WgOutputs.reset.offset < _lib.WgOutputs.final_obs.offset


def _batch(**kw):
    """A canonical-shaped uniform batch (M = 16 | 64) whose required pointers are non-NULL.  Nothing dereferences them:
    every call below is refused, or stops at a later range's error, before any launch."""
    b = _lib.WgBatch(N=128, M=16, K=40, A=8)
    for f in ("pos", "vel", "acc", "mass", "edges", "inc", "inc_off", "muscle_x", "muscle_bounds", "steps"):
        setattr(b, f, 64)
    for f in ("init_pos", "init_vel", "init_acc", "init_muscle_x", "episodes"):
        setattr(b, f, 64)
    for k, v in kw.items():
        setattr(b, k, v)
    return b


def _step(lib, b, p):
    return lib.wg_step(C.byref(b), C.byref(p), None, 0, 0, 0, None, 1, None, 0, None)


def _first_range_ok(lib, b, p):
    """Validate b / p without a launch: wg_run_ranges checks every range before it issues anything, so behind a valid
    first range the call fails on the second (a NULL batch)."""
    rng = (_lib.WgRange * 2)()
    rng[0].batch = C.pointer(b)
    ev = (C.c_void_p * 2)(1, 1)
    rc = lib.wg_run_ranges(rng, 2, C.byref(p), None, 0, 0, 0, 1, ev)
    return rc, lib.wg_last_error()


@pytest.mark.parametrize("field", ["init_pos", "init_vel", "init_acc", "init_muscle_x"])
def test_missing_snapshot_pointer(lib, field):
    p = _lib.WgParams(auto_reset=1)
    assert _step(lib, _batch(**{field: None}), p) == _lib.WG_EINVAL
    assert b"snapshot" in lib.wg_last_error()


def test_missing_episodes(lib):
    assert _step(lib, _batch(episodes=None), _lib.WgParams(auto_reset=3)) == _lib.WG_EINVAL
    assert b"episodes" in lib.wg_last_error()


def test_bad_noise_pool(lib):
    p = _lib.WgParams(auto_reset=1)
    assert _step(lib, _batch(reset_noise=64, reset_noise_rows=0, reset_noise_stride=3 * 128 * 16), p) == _lib.WG_EINVAL
    assert b"reset_noise_rows" in lib.wg_last_error()
    assert _step(lib, _batch(reset_noise=64, reset_noise_rows=2, reset_noise_stride=3 * 128 * 16 - 1), p) == _lib.WG_EINVAL
    assert b"reset_noise_stride" in lib.wg_last_error()
    # a pool that fits (and none at all) passes the check
    rc, err = _first_range_ok(lib, _batch(reset_noise=64, reset_noise_rows=2, reset_noise_stride=3 * 128 * 16), p)
    assert rc == _lib.WG_EINVAL and b"null batch" in err
    rc, err = _first_range_ok(lib, _batch(), p)
    assert rc == _lib.WG_EINVAL and b"null batch" in err


@pytest.mark.parametrize("bits", [4, 8 | 1, -1])
def test_unknown_bits(lib, bits):
    assert _step(lib, _batch(), _lib.WgParams(auto_reset=bits)) == _lib.WG_EINVAL
    assert b"auto_reset" in lib.wg_last_error() and b"bits" in lib.wg_last_error()


def test_batches_the_lean_kernel_does_not_take(lib, monkeypatch):
    import numpy as np
    plan = np.zeros(2, np.int32)
    # ragged (wave tiles)
    rb = _batch(ragged=2, mass_off=64, edge_off=64, muscle_off=64)
    p = _lib.WgParams(auto_reset=1)
    assert lib.wg_step(C.byref(rb), C.byref(p), None, 0, 0, 0, None, 1, plan.ctypes.data_as(C.c_void_p), 1,
                       None) == _lib.WG_EINVAL
    assert b"lean kernel" in lib.wg_last_error()
    # M does not divide 64
    assert _step(lib, _batch(M=12), p) == _lib.WG_EINVAL
    assert b"lean kernel" in lib.wg_last_error()
    # the G2 element, pair passes
    assert _step(lib, _batch(), _lib.WgParams(auto_reset=1, spring_mode=1)) == _lib.WG_EINVAL
    assert b"lean kernel" in lib.wg_last_error()
    assert _step(lib, _batch(), _lib.WgParams(auto_reset=1, pair_mode=1, pair_g=9.8)) == _lib.WG_EINVAL
    assert b"auto_reset" in lib.wg_last_error() and b"pair_mode" in lib.wg_last_error()
    # the barrier kernels selected from the environment
    monkeypatch.setenv("WG_LEAN", "0")
    assert _step(lib, _batch(), p) == _lib.WG_EINVAL
    assert b"lean kernel" in lib.wg_last_error()


def test_time_step_and_rollout_check_the_same(lib):
    p = _lib.WgParams(auto_reset=1)
    b = _batch(episodes=None)
    ms = C.c_float(-1.0)
    assert lib.wg_time_step(C.byref(b), C.byref(p), None, 0, 0, 0, None, 1, None, 0, None, C.byref(ms)) == _lib.WG_EINVAL
    assert b"episodes" in lib.wg_last_error() and ms.value == -1.0
    assert lib.wg_rollout(C.byref(b), C.byref(p), None, 0, 0, 0, None, 1, None, 0, None) == _lib.WG_EINVAL
    assert b"episodes" in lib.wg_last_error()


def test_off_validates_as_before(lib):
    """auto_reset = 0 with every new field NULL: the batch passes the checks (the call stops at the second range), and
    the snapshot is not asked for; the same batch with auto_reset = 1 is refused for it."""
    b = _batch(init_pos=None, init_vel=None, init_acc=None, init_muscle_x=None, episodes=None)
    rc, err = _first_range_ok(lib, b, _lib.WgParams())
    assert rc == _lib.WG_EINVAL and b"null batch" in err
    rc, err = _first_range_ok(lib, b, _lib.WgParams(auto_reset=1))
    assert rc == _lib.WG_EINVAL and b"snapshot" in err
    # observe never resets: auto_reset is a step option
    assert _lib.WgOutputs.reset.size == C.sizeof(C.c_void_p)

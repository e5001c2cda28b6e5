"""ctypes binding of libwalker_hip.so (the C ABI in include/walker_hip.h).

The library is built in-tree (walker_gym_amd/libwalker_hip.so, see walker_gym_amd/build.py) so it
travels with the repo to the GPU box.  There is no fallback: if the library is missing or its ABI
version differs, every entry point raises — the product never silently runs on the CPU.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_NAME = "libwalker_hip.so"
LIB_PATH = os.path.join(HERE, LIB_NAME)
ABI_VERSION = 16

WG_EINVAL, WG_ERANGE, WG_EHIP = -1, -2, -3

_vp = C.c_void_p


class WgParams(C.Structure):
    _fields_ = [(n, C.c_double) for n in ("g", "dampk", "ground", "groundk", "grounddamp", "friction", "dt",
                                           "pk", "vk", "ak", "mk")] + \
               [(n, C.c_int32) for n in ("in3d", "max_steps", "midform", "conmid", "spring_mode", "action_mode",
                                         "integrator", "pair_mode")] + \
               [(n, C.c_double) for n in ("pair_g", "pair_k", "pair_e", "bounce_k")] + \
               [("g3_gravity", C.c_double * 3)] + \
               [(n, C.c_double) for n in ("g3_damping", "g3_air", "g3_ground_level", "g3_restitution",
                                          "g3_friction")] + [("g3_ground", C.c_int32), ("friction_mode", C.c_int32),
                                                             ("auto_reset", C.c_int32)]   # ABI 16: 1 done, 2 non-finite


class WgBatch(C.Structure):
    _fields_ = [("N", C.c_int32), ("M", C.c_int32), ("K", C.c_int32), ("A", C.c_int32),
                ("ragged", C.c_int32),
                ("mass_off", _vp), ("edge_off", _vp), ("muscle_off", _vp),
                ("pos", _vp), ("vel", _vp), ("acc", _vp), ("mass", _vp),
                ("edges", _vp),
                ("inc", _vp), ("inc_off", _vp),
                ("muscle_x", _vp), ("muscle_bounds", _vp), ("muscle_stride", _vp),
                ("steps", _vp), ("contact", _vp), ("pinned", _vp),
                ("charge", _vp), ("radius", _vp), ("row", _vp), ("bounce_set", _vp),
                ("edges8", _vp), ("kc", C.c_float * 4),   # ABI 15: the compact spring records and their (k, c) classes
                # ABI 16, auto-reset: the episode-start snapshot, the reset-noise pool and the episode counters
                ("init_pos", _vp), ("init_vel", _vp), ("init_acc", _vp), ("init_muscle_x", _vp),
                ("reset_noise", _vp), ("reset_noise_rows", C.c_int32), ("reset_noise_stride", C.c_int64),
                ("episodes", _vp)]


class WgOutputs(C.Structure):
    _fields_ = [("obs", _vp), ("obs_stride", C.c_int32), ("reward", _vp), ("done", _vp),
                ("centroid", _vp), ("energy", _vp), ("obs_step", C.c_int64), ("out_step", C.c_int64),
                ("obs_pad_clean", C.c_int32), ("steps", _vp), ("nonfinite", _vp), ("momentum", _vp),
                ("reset", _vp), ("final_obs", _vp)]   # ABI 16, auto-reset


class WgRange(C.Structure):
    _fields_ = [("batch", C.POINTER(WgBatch)), ("outputs", C.POINTER(WgOutputs)), ("action_offset", C.c_int64),
                ("plan", _vp), ("plan_blocks", C.c_int32), ("stream", _vp)]


class WgLaunchInfo(C.Structure):
    _fields_ = [("threads", C.c_int32), ("walkers_per_block", C.c_int32), ("blocks", C.c_int32),
                ("lds_bytes", C.c_int32)]


class WgPolicy(C.Structure):
    """wg_policy: the in-kernel policy of wg_rollout_policy and its optional per-step / per-walker outputs."""
    _fields_ = [("n_sets", C.c_int32), ("obs_dim", C.c_int32), ("hidden", C.c_int32), ("act_dim", C.c_int32),
                ("w1", _vp), ("b1", _vp), ("w2", _vp), ("b2", _vp), ("act_limit", C.c_float),
                ("action_out", _vp), ("action_out_step", C.c_int64), ("return_out", _vp), ("length_out", _vp)]


class WgEpisodeStats(C.Structure):
    """wg_episode_stats: the per-episode accounting of wg_rollout_episodes (every pointer optional)."""
    _fields_ = [("return_sum", _vp), ("length_sum", _vp), ("episodes_done", _vp), ("tail_return", _vp),
                ("tail_length", _vp), ("ep_return", _vp), ("ep_length", _vp), ("ep_slots", C.c_int32)]


class WgEs(C.Structure):
    """wg_es: the seeded perturbation of wg_es_perturb / wg_es_update (theta's segments: w1, b1, w2, b2)."""
    _fields_ = [("n_sets", C.c_int32), ("obs_dim", C.c_int32), ("hidden", C.c_int32), ("act_dim", C.c_int32),
                ("seed", C.c_uint64), ("generation", C.c_uint32), ("sigma", C.c_float), ("theta", _vp),
                ("w1", _vp), ("b1", _vp), ("w2", _vp), ("b2", _vp)]


class WgEsDiagStep(C.Structure):
    """wg_es_diag_step: the scales, learning rates and sigma bounds of wg_es_update_diag."""
    _fields_ = [("scale_theta", C.c_double), ("scale_sigma", C.c_double), ("base", C.c_float), ("lr_theta", C.c_float),
                ("lr_sigma", C.c_float), ("shrink", C.c_float), ("grow", C.c_float), ("sigma_min", C.c_float),
                ("sigma_max", C.c_float)]


class WgEsMid(C.Structure):
    """wg_es_mid: the middle layer of a deep candidate set (the wg_es_*_deep entries; theta's segments: w1, b1, wm, bm,
    w2, b2)."""
    _fields_ = [("hidden2", C.c_int32), ("wm", _vp), ("bm", _vp)]


class WgActionNoise(C.Structure):
    """wg_action_noise: the seeded exploration noise of wg_rollout_stochastic and its optional per-step outputs."""
    _fields_ = [("seed", C.c_uint64), ("step_base", C.c_uint32), ("walker_base", C.c_uint32), ("sigma", _vp),
                ("raw_out", _vp), ("raw_out_step", C.c_int64), ("eps_out", _vp), ("eps_out_step", C.c_int64)]


class WgPolicyRows(C.Structure):
    """wg_policy_rows: the recorded observation rows of wg_policy_forward / wg_policy_backward."""
    _fields_ = [("x", _vp), ("x_step", C.c_int64), ("mask", _vp), ("mask_step", C.c_int64), ("n_steps", C.c_int32),
                ("N", C.c_int32)]


class WgObsNorm(C.Structure):
    """wg_obs_norm: the observation normaliser in front of wg_policy's layers."""
    _fields_ = [("mean", _vp), ("scale", _vp), ("clip", C.c_float)]


class WgActionHold(C.Structure):
    """wg_action_hold: the action hold of wg_rollout_held and its optional per-step outputs."""
    _fields_ = [("every", C.c_int32), ("held", _vp), ("decided_out", _vp), ("decided_out_step", C.c_int64),
                ("hold_reward_out", _vp), ("hold_reward_out_step", C.c_int64)]


class WgPolicyMid(C.Structure):
    """wg_policy_mid: the second hidden layer of a deep policy (wg_rollout_deep, wg_policy_forward_deep / _backward_deep)."""
    _fields_ = [("hidden2", C.c_int32), ("wm", _vp), ("bm", _vp)]


class WgPpoRows(C.Structure):
    """wg_ppo_rows: the recorded means and raw actions of wg_ppo_surrogate, and the density's sigma / log_sigma."""
    _fields_ = [("y", _vp), ("y_step", C.c_int64), ("u", _vp), ("u_step", C.c_int64), ("sigma", _vp), ("log_sigma", _vp),
                ("mask", _vp), ("mask_step", C.c_int64), ("n_steps", C.c_int32), ("N", C.c_int32), ("n_sets", C.c_int32),
                ("act_dim", C.c_int32)]


class WgOptSegment(C.Structure):
    """wg_opt_segment: one tensor of wg_adam_step's table (device pointers; the table itself is host memory)."""
    _fields_ = [("param", _vp), ("grad", _vp), ("m", _vp), ("v", _vp), ("n", C.c_int64)]


class WgAdam(C.Structure):
    """wg_adam: the hyperparameters of one wg_adam_step call."""
    _fields_ = [(n, C.c_float) for n in ("lr", "beta1", "beta2", "eps", "weight_decay", "max_norm")] + \
               [("maximize", C.c_int32)]


POLICY_GRAD_MAX_K = 16384   # WG_POLICY_GRAD_MAX_K
OPT_MAX_SEGMENTS = 32       # WG_OPT_MAX_SEGMENTS

EXPORTS = ("wg_abi_version", "wg_last_error", "wg_step", "wg_step_ranges", "wg_run_ranges", "wg_rollout", "wg_observe",
           "wg_step_simple", "wg_observe_simple", "wg_reset", "wg_reset_noise", "wg_plan_ragged", "wg_plan_waves",
           "wg_wave_edge_passes", "wg_plan_errors", "wg_launch_geometry", "wg_launch_floor", "wg_time_step",
           "wg_rollout_policy", "wg_rollout_episodes", "wg_fix_launches", "wg_wt_launches", "wg_es_perturb", "wg_es_update",
           "wg_rollout_stochastic", "wg_gae", "wg_policy_forward", "wg_policy_backward_workspace", "wg_policy_backward",
           "wg_es_perturb_diag", "wg_es_update_diag", "wg_rollout_normalized", "wg_policy_forward_normalized",
           "wg_policy_backward_normalized", "wg_obs_moments_workspace", "wg_obs_moments", "wg_rollout_held", "wg_gae_held",
           "wg_rollout_deep", "wg_policy_forward_deep", "wg_policy_backward_deep_workspace", "wg_policy_backward_deep",
           "wg_es_perturb_deep", "wg_es_update_deep", "wg_es_perturb_diag_deep", "wg_es_update_diag_deep", "wg_expf",
           "wg_ppo_surrogate_workspace", "wg_ppo_surrogate", "wg_adam_workspace", "wg_adam_step")

_lib = None
_lock = threading.Lock()


class WalkerHipError(RuntimeError):
    pass


def load(path: str | None = None):
    """Load (once) and type the library. Raises if it is missing or has the wrong ABI version."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        p = path or os.environ.get("WALKER_HIP_LIB", LIB_PATH)
        if not os.path.exists(p):
            raise WalkerHipError(
                f"{p} not found: build it with `python -m walker_gym_amd.build` (hipcc --offload-arch=gfx950); "
                "walker_gym_amd has no CPU fallback")
        L = C.CDLL(p)
        L.wg_abi_version.restype = C.c_int
        L.wg_last_error.restype = C.c_char_p
        L.wg_step.argtypes = [C.POINTER(WgBatch), C.POINTER(WgParams), _vp, C.c_int32, C.c_int32, C.c_int64,
                              C.POINTER(WgOutputs), C.c_int32, _vp, C.c_int32, _vp]
        L.wg_rollout.argtypes = L.wg_step.argtypes
        L.wg_rollout_policy.argtypes = [C.POINTER(WgBatch), C.POINTER(WgParams), C.POINTER(WgPolicy),
                                        C.POINTER(WgOutputs), C.c_int32, _vp]
        L.wg_rollout_episodes.argtypes = [C.POINTER(WgBatch), C.POINTER(WgParams), C.POINTER(WgPolicy),
                                          C.POINTER(WgOutputs), C.POINTER(WgEpisodeStats), C.c_int32, _vp]
        L.wg_rollout_stochastic.argtypes = [C.POINTER(WgBatch), C.POINTER(WgParams), C.POINTER(WgPolicy),
                                            C.POINTER(WgActionNoise), C.POINTER(WgOutputs), C.POINTER(WgEpisodeStats),
                                            C.c_int32, _vp]
        L.wg_gae.argtypes = [_vp, _vp, _vp, _vp, _vp, C.c_int32, C.c_int32, C.c_int64, C.c_float, C.c_float, _vp, _vp,
                             _vp]
        L.wg_policy_forward.argtypes = [C.POINTER(WgPolicy), C.POINTER(WgPolicyRows), _vp, C.c_int64, _vp]
        L.wg_policy_backward_workspace.argtypes = [C.POINTER(WgPolicy), C.POINTER(WgPolicyRows), C.c_int32]
        L.wg_policy_backward.argtypes = [C.POINTER(WgPolicy), C.POINTER(WgPolicyRows), _vp, C.c_int64, C.c_int32, _vp,
                                         _vp, _vp, _vp, _vp, _vp]
        L.wg_rollout_normalized.argtypes = [C.POINTER(WgBatch), C.POINTER(WgParams), C.POINTER(WgPolicy),
                                            C.POINTER(WgObsNorm), C.POINTER(WgActionNoise), C.POINTER(WgOutputs),
                                            C.POINTER(WgEpisodeStats), C.c_int32, _vp]
        L.wg_policy_forward_normalized.argtypes = [C.POINTER(WgPolicy), C.POINTER(WgObsNorm), C.POINTER(WgPolicyRows),
                                                   _vp, C.c_int64, _vp]
        L.wg_policy_backward_normalized.argtypes = [C.POINTER(WgPolicy), C.POINTER(WgObsNorm), C.POINTER(WgPolicyRows),
                                                    _vp, C.c_int64, C.c_int32, _vp, _vp, _vp, _vp, _vp, _vp]
        L.wg_rollout_held.argtypes = [C.POINTER(WgBatch), C.POINTER(WgParams), C.POINTER(WgPolicy), C.POINTER(WgObsNorm),
                                      C.POINTER(WgActionNoise), C.POINTER(WgActionHold), C.POINTER(WgOutputs),
                                      C.POINTER(WgEpisodeStats), C.c_int32, _vp]
        L.wg_rollout_deep.argtypes = [C.POINTER(WgBatch), C.POINTER(WgParams), C.POINTER(WgPolicy), C.POINTER(WgPolicyMid),
                                      C.POINTER(WgObsNorm), C.POINTER(WgActionNoise), C.POINTER(WgActionHold),
                                      C.POINTER(WgOutputs), C.POINTER(WgEpisodeStats), C.c_int32, _vp]
        L.wg_policy_forward_deep.argtypes = [C.POINTER(WgPolicy), C.POINTER(WgPolicyMid), C.POINTER(WgObsNorm),
                                             C.POINTER(WgPolicyRows), _vp, C.c_int64, _vp]
        L.wg_policy_backward_deep_workspace.argtypes = [C.POINTER(WgPolicy), C.POINTER(WgPolicyMid),
                                                        C.POINTER(WgPolicyRows), C.c_int32]
        L.wg_policy_backward_deep.argtypes = [C.POINTER(WgPolicy), C.POINTER(WgPolicyMid), C.POINTER(WgObsNorm),
                                              C.POINTER(WgPolicyRows), _vp, C.c_int64, C.c_int32, _vp, _vp, _vp, _vp, _vp,
                                              _vp, _vp, _vp]
        L.wg_gae_held.argtypes = [_vp, _vp, _vp, _vp, _vp, _vp, C.c_int32, C.c_int32, C.c_int64, C.c_float, C.c_float,
                                  _vp, _vp, _vp]
        L.wg_obs_moments_workspace.argtypes = [C.POINTER(WgPolicyRows), C.c_int32, C.c_int32]
        L.wg_obs_moments.argtypes = [C.POINTER(WgPolicyRows), C.c_int32, C.c_float, C.c_int32, _vp, _vp, C.c_double,
                                     _vp, _vp, _vp]
        L.wg_expf.argtypes = [_vp, C.c_int64, _vp, _vp]
        L.wg_ppo_surrogate_workspace.argtypes = [C.POINTER(WgPpoRows), C.c_int32]
        L.wg_ppo_surrogate.argtypes = [C.POINTER(WgPpoRows), _vp, _vp, C.c_int64, _vp, _vp, _vp, C.c_float, C.c_int32,
                                       _vp, _vp, _vp, C.c_int64, _vp, _vp, _vp, _vp]
        L.wg_adam_workspace.argtypes = [C.POINTER(WgOptSegment), C.c_int32]
        L.wg_adam_step.argtypes = [C.POINTER(WgOptSegment), C.c_int32, C.POINTER(WgAdam), _vp, _vp, _vp]
        L.wg_es_perturb.argtypes = [C.POINTER(WgEs), C.c_int32, C.c_int32, _vp]
        L.wg_es_update.argtypes = [C.POINTER(WgEs), C.c_int32, C.c_int32, _vp, C.c_double, C.c_float, _vp, _vp, _vp, _vp]
        L.wg_es_perturb_diag.argtypes = [C.POINTER(WgEs), _vp, C.c_int32, C.c_int32, _vp]
        L.wg_es_update_diag.argtypes = [C.POINTER(WgEs), _vp, C.c_int32, C.c_int32, _vp, C.POINTER(WgEsDiagStep), _vp,
                                        _vp, _vp, _vp, _vp, _vp]
        mid = C.POINTER(WgEsMid)   # the _deep twins: wg_es_mid after es, then the shallow entry's arguments
        L.wg_es_perturb_deep.argtypes = [C.POINTER(WgEs), mid] + L.wg_es_perturb.argtypes[1:]
        L.wg_es_update_deep.argtypes = [C.POINTER(WgEs), mid] + L.wg_es_update.argtypes[1:]
        L.wg_es_perturb_diag_deep.argtypes = [C.POINTER(WgEs), mid] + L.wg_es_perturb_diag.argtypes[1:]
        L.wg_es_update_diag_deep.argtypes = [C.POINTER(WgEs), mid] + L.wg_es_update_diag.argtypes[1:]
        L.wg_step_ranges.argtypes = [C.POINTER(WgRange), C.c_int32, C.POINTER(WgParams), _vp, C.c_int32, C.c_int32,
                                     C.POINTER(_vp)]
        L.wg_run_ranges.argtypes = [C.POINTER(WgRange), C.c_int32, C.POINTER(WgParams), _vp, C.c_int32, C.c_int32,
                                    C.c_int64, C.c_int32, C.POINTER(_vp)]
        L.wg_observe.argtypes = [C.POINTER(WgBatch), C.POINTER(WgParams), C.POINTER(WgOutputs), _vp, C.c_int32, _vp]
        # SURVEY §8(b)'s declared signatures (ABI 13)
        L.wg_step_simple.argtypes = [C.POINTER(WgBatch), _vp, C.POINTER(WgParams), C.c_int32, _vp]
        L.wg_observe_simple.argtypes = [C.POINTER(WgBatch), C.POINTER(WgParams), _vp, _vp, _vp, _vp, _vp, _vp]
        L.wg_reset.argtypes = [C.POINTER(WgBatch), C.POINTER(WgParams), _vp, _vp, _vp]
        L.wg_reset_noise.argtypes = [C.POINTER(WgBatch), _vp, _vp]
        L.wg_plan_ragged.argtypes = [_vp, _vp, _vp, C.c_int32, _vp, C.c_int32]
        L.wg_plan_waves.argtypes = [_vp, _vp, _vp, C.c_int32, _vp, C.c_int32]
        L.wg_wave_edge_passes.argtypes = [C.c_int32, C.c_int32]
        L.wg_plan_errors.argtypes = [C.c_int32]
        L.wg_launch_geometry.argtypes = [C.POINTER(WgBatch), C.POINTER(WgLaunchInfo)]
        L.wg_launch_floor.argtypes = [C.c_int32, C.c_int32, C.c_int32, _vp, _vp, C.c_int32, _vp]
        L.wg_time_step.argtypes = L.wg_step.argtypes + [C.POINTER(C.c_float)]   # ABI 14, measurement aid
        for f in EXPORTS[2:]:
            getattr(L, f).restype = C.c_int
        L.wg_fix_launches.restype = C.c_longlong
        L.wg_wt_launches.restype = C.c_longlong
        L.wg_policy_backward_workspace.restype = C.c_int64
        L.wg_policy_backward_deep_workspace.restype = C.c_int64
        L.wg_obs_moments_workspace.restype = C.c_int64
        L.wg_ppo_surrogate_workspace.restype = C.c_int64
        L.wg_adam_workspace.restype = C.c_int64
        v = L.wg_abi_version()
        if v != ABI_VERSION:
            raise WalkerHipError(f"{p}: ABI version {v}, expected {ABI_VERSION}")
        _lib = L
        return L


def ptr(t):
    """A device tensor's address as a C pointer argument (None stays NULL)."""
    return None if t is None else C.c_void_p(t.data_ptr())


def check(rc: int, what: str) -> int:
    if rc < 0:
        msg = load().wg_last_error().decode(errors="replace")
        exc = ValueError if rc in (WG_EINVAL, WG_ERANGE) else WalkerHipError
        raise exc(f"{what}: {msg} (code {rc})")
    return rc

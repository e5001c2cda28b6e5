"""BatchedPhysicsEnv — N independent walkers stepped by one HIP launch per env step.

The batched form of the reference's gym-style API (gym/optimized_env.py:8-269):
  reset(noise=None, mask=None)        -> obs [N, D]                     (PhysicsEnv.reset :53-68)
  step(action [N, A])                 -> obs, reward [N], done [N], info (PhysicsEnv.step :70-92)
  rollout(actions [T, N, A])          -> obs [T, N, D], reward [T, N], done [T, N]   (one C call)
  observe()                           -> obs, reward, done, info for the current state
Environment parameters keep the reference's names and defaults (PhysicsEnv.__init__ :15-17).
obs rows are Creature.getstat (gym/optimized_walker.py:129-162), zero-padded to D = max row length
for ragged batches (``obs_len`` gives each walker's length).
"""
from __future__ import annotations

import ctypes as C
import os
from dataclasses import dataclass, asdict
from typing import Optional, Sequence

import numpy as np
import torch

from . import _lib
from .device import DeviceBatch
from .layout import HostLayout, pack
from .ranges import WalkerRange, block_bounds, caller_bounds, uniform_bounds

# info() keys a call leaves stale: the per-step info of a run with info=False or record buffers, and everything that is
# "not this call's outputs" after a rollout into the caller's buffers
_INFO_STALE = frozenset({"centroid_position", "total_energy", "momentum", "nonfinite"})
_ROLLOUT_STALE = _INFO_STALE | {"reset", "final_obs"}


@dataclass
class EnvParams:
    """PhysicsEnv / Environment constructor parameters + getstat options (reference defaults)."""
    g: float = 100.0
    dampk: float = 0.0
    ground: float = 0.0           # ground_high / groundhigh
    groundk: float = 1000.0       # ground_k
    grounddamp: float = 100.0     # ground_damp
    friction: float = 100.0
    dt: float = 0.01              # PhysicsEnv.time_step (optimized_env.py:42)
    in3d: bool = False
    max_steps: int = 1000         # optimized_env.py:44
    pk: float = 1.0
    vk: float = 1.0
    ak: float = 1.0
    mk: float = 1.0
    midform: int = 1              # 1: minus the mean (G2 getstat); 2: minus the SUM (G1 getstat); 0: raw
    conmid: bool = False
    spring_mode: int = 0          # 0: engine.py resilience + damping; 1: G2 optimized_walker as written
    action_mode: int = 0          # 0: Muscle.act; 1: Muscle.actdisp
    integrator: int = 1           # 1: Point.run1 (what the envs call); 2: Point.run2 (gym/engine.py:180-190)
    pair_mode: int = 0            # bitmask, per walker after the springs: 1 Point.gravity (gym/engine.py:128-137),
                                  # 2 Point.coulomb (:139-147), 4 Point.bounce (:114-125), in that order
    pair_g: float = 9.8           # Config.g of the gravity pass (gym/engine.py:12)
    pair_k: float = 8.99e9        # Config.k of the coulomb pass (gym/engine.py:11)
    pair_e: float = 16e-20        # Point.e of every point without a spec charge (Config.e, gym/engine.py:10)
    bounce_k: float = 100.0       # Point.bounce(k) (gym/engine.py:114)
    # spring_mode 2: the G3 engine (gym/optimized_walker/env.py:10-14 defaults, update_physics :135-184)
    g3_gravity: tuple = (0.0, -9.8, 0.0)
    g3_damping: float = 0.99
    g3_air: float = 0.01
    g3_ground_level: float = -50.0
    g3_restitution: float = 0.8
    g3_friction: float = 0.5
    g3_ground: int = 1
    friction_mode: int = 0        # 0: gym/optimized_env.py:168-172 friction; 1: the G1 env's (gym/env.py:41)

    def to_struct(self) -> _lib.WgParams:
        d = asdict(self)
        if d["integrator"] in ("run1", "run2"):
            d["integrator"] = int(d["integrator"][-1])
        if int(d["integrator"]) not in (0, 1, 2):
            raise ValueError("integrator must be 1 ('run1') or 2 ('run2')")
        gv = tuple(float(x) for x in d.pop("g3_gravity"))
        if len(gv) != 3:
            raise ValueError("g3_gravity must have 3 components")
        return _lib.WgParams(g3_gravity=(C.c_double * 3)(*gv),
                             **{k: (int(v) if k in ("in3d", "max_steps", "midform", "conmid", "spring_mode",
                                                    "action_mode", "integrator", "pair_mode", "g3_ground",
                                                    "friction_mode")
                                    else float(v)) for k, v in d.items()})


def require_tensor(t, name: str, device, dtype, shape=None) -> None:
    """Refuse a tensor whose raw pointer the kernel cannot use as given: another device (host memory or another
    GPU), another dtype, a non-contiguous layout or a wrong shape.  Raises ValueError before any launch."""
    if not isinstance(t, torch.Tensor):
        raise ValueError(f"{name} must be a torch tensor on {device}")
    # (on the per-call path of run(): `torch.device.__ne__` and tuple(t.shape) cost microseconds each, == does not)
    if not (t.device == (device if isinstance(device, torch.device) else torch.device(device))):
        raise ValueError(f"{name} is on {t.device}, the batch is on {device}")
    if t.dtype != dtype:
        raise ValueError(f"{name} has dtype {t.dtype}, expected {dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    if shape is not None and not (t.shape == (shape if isinstance(shape, tuple) else tuple(shape))):
        raise ValueError(f"{name} has shape {tuple(t.shape)}, expected {tuple(shape)}")


class WalkerGraph:
    """A captured run() (BatchedPhysicsEnv.graph).  The graph holds raw pointers to the env's state and output
    tensors and the parameters as they were at capture: set_params / a reallocation of the outputs / enabling
    radii bump the env's generation, and replay() of a graph captured before that raises instead of writing
    into freed memory or silently stepping with stale parameters."""

    def __init__(self, env: "BatchedPhysicsEnv", graph, actions, info: bool = True):
        self._env, self._graph, self._gen = env, graph, env._generation
        self.actions = actions            # kept alive: the graph reads it on every replay
        # the replayed steps write info['steps'] in caller order (env.steps_out) only when captured with info
        self._writes_steps = bool(info) and env.steps_out is not None
        self._stale = frozenset() if info else _INFO_STALE

    def replay(self) -> None:
        env = self._env
        if env._generation != self._gen:
            raise RuntimeError("stale WalkerGraph: the env's parameters or buffers changed after capture; "
                               "capture a new graph")
        self._graph.replay()
        # the batch's step counters moved: steps_out is current only if the graph wrote it (a graph
        # captured with info=False left a step()'s steps_out looking valid)
        env._steps_at = env.batch.version if self._writes_steps else -1
        env._stale = self._stale


class _RangeGraphs:
    """One captured graph per walker range and the stream it replays on (graph(), policy_loop(graph=True)): replay()
    forks the ranges from the calling stream, replays each on its own stream and joins them back.  (One graph holding
    the ranges as parallel branches replayed them serially on ROCm: 36.4 against 33.5 us per canonical step direct,
    profiles/r05y_bench_graph.json.)"""

    def __init__(self, parts, cur):
        self.parts, self._cur = parts, cur

    def replay(self) -> None:
        # range 0 replays on the calling stream itself (a single range needs no fork), the others on their own streams
        cur = torch.cuda.current_stream(self._cur.device)
        for g, st in self.parts[1:]:
            st.wait_stream(cur)
        for g, st in self.parts[1:]:
            with torch.cuda.stream(st):
                g.replay()
        self.parts[0][0].replay()
        for g, st in self.parts[1:]:
            cur.wait_stream(st)


class PreparedRun:
    """run()'s C call with its arguments already built (BatchedPhysicsEnv.prepare_run): calling it issues the prepared
    steps again.  Like a WalkerGraph it refuses to run once the env's parameters or buffers have changed."""

    def __init__(self, env: "BatchedPhysicsEnv", entry: str, fn, args, keep, steps_valid: bool, stale, thunk=None):
        self._env, self._gen, self._struct = env, env._generation, env.batch.struct
        self._entry, self._fn, self._args, self._keep, self._thunk = entry, fn, args, keep, thunk
        self._steps_valid, self._stale = steps_valid, frozenset(stale)

    def __call__(self) -> None:
        env = self._env
        if env._generation != self._gen or env.batch.struct is not self._struct:
            raise RuntimeError("stale PreparedRun: the env's parameters or buffers changed after prepare_run")
        if self._thunk is not None:
            self._thunk(*self._args)
        else:
            rc = self._fn(*self._args)
            if rc:
                _lib.check(rc, self._entry)
        env._steps_at = env.batch.version if self._steps_valid else -1
        env._stale = self._stale


class BatchedPhysicsEnv:
    def __init__(self, spec_or_layout, device=None, rand_sigma: float = 0.0, seed: Optional[int] = None,
                 contact: bool = True, info_extras: bool = False, **params):
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None
        if device is None:
            raise RuntimeError("BatchedPhysicsEnv needs a ROCm GPU (libwalker_hip.so); there is no CPU path")
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        _lib.load()   # fail loudly before allocating anything
        self.params = EnvParams(**params)
        self.sigma = float(rand_sigma)
        host = spec_or_layout if isinstance(spec_or_layout, HostLayout) else pack(spec_or_layout)
        self.batch = DeviceBatch(host, device, contact=contact, wave_ok=self._wave_ok())
        if int(self.params.pair_mode) & 4:
            self.batch.enable_radius()
        self.device = device
        self.N = host.N
        self.obs_len = host.obs_len(self.params.in3d, self.params.conmid)
        self.obs_dim = int(self.obs_len.max())
        # auto-reset (enable_auto_reset): wg_params.auto_reset, info['reset'] and the optional terminal rows
        self._ar_mode, self.reset_out, self.final_obs = 0, None, None
        self._pstruct = self._make_pstruct()
        self._gen = torch.Generator(device=device)
        if seed is not None:
            self._gen.manual_seed(int(seed))
        self._generation = 0
        self._stale = frozenset()   # info() keys the last run() did not write (record buffers / info=False)
        # opt-in info (ABI 10): info['momentum'] (Point.momentum per walker, gym/engine.py:160-166) and
        # info['nonfinite'] (a walker whose state holds an inf / NaN; done is left as the reference computes it)
        self._extras = bool(info_extras)
        # caches, each rebuilt when its key moves: step()'s arguments (_step_plan), the uniform walker-range views
        # (_range_batches), wg_run_ranges' events (_range_events); and the last captured policy_loop
        self._plan_cache = self._range_cache = self._run_events = self._policy_graph = None
        self._alloc_outputs()
        # the side streams of the default walker ranges, created now: a stream's hardware queue is bound when it is
        # created, and a process has few of them (GPU_MAX_HW_QUEUES = 4).  Created after an RCCL communicator
        # (whose streams take queues of their own) a side stream can share the calling stream's queue, which
        # serialises the ranges: 52.8 against 37.5 us per canonical step (profiles/r03a_bench_nccl1.json).
        self._side = []
        self.reserve_streams(self._lanes(None))

    @classmethod
    def from_topologies(cls, topologies, n_envs: int, device=None, **params) -> "BatchedPhysicsEnv":
        """SURVEY §8(b)'s BatchedPhysicsEnv(topologies, n_envs, device, **EnvParams): n_envs walkers split into
        contiguous, near-equal blocks, one per topology in order (uniform when there is one).  A topology is
        a Creature (walker_gym_amd.walker / .topologies builders) or an env id of make_env ('Balance-v0',
        'Box-v0', gym/optimized_env.py:273-294; unknown ids raise ValueError as there)."""
        from .walker import (Creature, concat_specs, create_balance_creature, create_box_creature,
                             creatures_to_spec, replicate_spec)
        if isinstance(topologies, (str, Creature)):
            topologies = [topologies]
        topologies = list(topologies)
        if not topologies or n_envs < len(topologies):
            raise ValueError("need at least one topology and one env per topology")
        specs = []
        for t, topo in enumerate(topologies):
            if isinstance(topo, str):
                tid = topo.lower()
                if tid == "balance-v0":
                    topo = create_balance_creature()
                elif tid == "box-v0":
                    topo = create_box_creature()
                else:
                    raise ValueError(f"Unknown environment ID: {topo}")
            count = n_envs // len(topologies) + (1 if t < n_envs % len(topologies) else 0)
            specs.append(replicate_spec(creatures_to_spec([topo]), count))
        return cls(specs[0] if len(specs) == 1 else concat_specs(specs), device=device, **params)

    # ------------------------------------------------------------------ plumbing
    def _alloc_outputs(self):
        self._generation += 1
        N, D, dv = self.N, self.obs_dim, self.device
        self.obs = torch.zeros((N, D), dtype=torch.float32, device=dv)
        self.reward = torch.zeros(N, dtype=torch.float32, device=dv)
        # bool storage: the kernel writes 0 / 1 bytes, so step() returns it as is (no conversion launch per step)
        self.done = torch.zeros(N, dtype=torch.bool, device=dv)
        self.centroid = torch.zeros((N, 3), dtype=torch.float32, device=dv)
        self.energy = torch.zeros(N, dtype=torch.float32, device=dv)
        # info['steps'] of a permuted (ragged) batch in the caller's order, written by the step kernels themselves
        # (wg_outputs.steps) so that step() needs no gather; valid while _steps_at == the batch's state version
        self.steps_out = torch.zeros(N, dtype=torch.int32, device=dv) if self.batch._perm else None
        self._steps_at = -1
        self.momentum = torch.zeros((N, 3), dtype=torch.float32, device=dv) if self._extras else None
        self.nonfinite = torch.zeros(N, dtype=torch.bool, device=dv) if self._extras else None
        if self.final_obs is not None:   # (auto-reset's terminal rows follow the row length)
            self.final_obs = torch.zeros((N, D), dtype=torch.float32, device=dv)

    def _make_pstruct(self) -> _lib.WgParams:
        ps = self.params.to_struct()
        ps.auto_reset = self._ar_mode
        return ps

    # ------------------------------------------------------------------ auto-reset (ABI 16)
    _AR_BITS = {"done": 1, "nonfinite": 2}

    def enable_auto_reset(self, on=("done",), noise_rows: int = 1, final_obs: bool = False, noise=None) -> None:
        """Episodes roll over on the device: from now on a walker whose step ends its episode — its `done` is set
        ('done'), or its state after the step holds an inf / NaN ('nonfinite') — is put back to the episode start inside
        the launch that stepped it: pos / vel / acc / muscle_x from a snapshot of the CURRENT state, then reset()'s
        velocity noise and steps = 0, and its obs row is the fresh state's (what reset() returns), while reward, done
        and info keep the terminal step's values.  info() gains 'reset' (the walkers reset by the last step),
        'episodes' (resets taken so far) and, with final_obs, 'final_obs' (the terminal rows of the walkers just reset;
        other rows are left as they were).

        The noise comes from a pool of `noise_rows` draws of randn * sigma over [P, 3] from the env's generator (none
        when sigma == 0); a walker's episode e uses row e % noise_rows, and refresh_reset_noise() redraws the pool.
        noise [rows, P, 3]: a pool of the caller's instead.  Works with step, run, rollout (resident included),
        rollout_episodes, policy_loop and graph; prepared runs and graphs made before the call refuse to run.  Only batches the
        barrier-free lean kernel takes (uniform, M dividing 64, spring_mode 0, pair_mode 0): ValueError otherwise."""
        names = (on,) if isinstance(on, str) else tuple(on)
        if not names or any(n not in self._AR_BITS for n in names):
            raise ValueError(f"enable_auto_reset: on must name 'done' and / or 'nonfinite', got {on!r}")
        if not self.resident_ok():
            raise ValueError("enable_auto_reset: only batches of the lean step kernel (uniform, M dividing 64 with "
                             "M >= 4, spring_mode 0, pair_mode 0, WG_LEAN not 0); ragged batches and the workgroup "
                             "kernel have no auto-reset")
        if noise is not None:
            pool = torch.as_tensor(noise, dtype=torch.float32).to(self.device).reshape(-1, self.batch.P, 3).contiguous()
        elif self.sigma > 0:
            if int(noise_rows) < 1:
                raise ValueError("enable_auto_reset: noise_rows must be >= 1")
            pool = torch.randn((int(noise_rows), self.batch.P, 3), generator=self._gen, device=self.device) * self.sigma
        else:
            pool = None
        self.batch.set_auto_reset(pool)
        self._ar_mode = sum(self._AR_BITS[n] for n in set(names))
        self.reset_out = torch.zeros(self.N, dtype=torch.bool, device=self.device)
        self.final_obs = torch.zeros((self.N, self.obs_dim), dtype=torch.float32, device=self.device) if final_obs \
            else None
        self._pstruct = self._make_pstruct()
        self._generation += 1   # prepared runs and graphs rebuild

    def disable_auto_reset(self) -> None:
        """Turn auto-reset off: the step is the plain step again (the snapshot and the noise pool are dropped)."""
        if self._ar_mode:
            self._ar_mode, self.reset_out, self.final_obs = 0, None, None
            self.batch.clear_auto_reset()
            self._pstruct = self._make_pstruct()
            self._generation += 1

    def set_episode_start(self) -> None:
        """Take the current state as the episode start of the walkers reset from now on (stream-ordered copies into
        the existing snapshot: graphs and prepared runs stay valid)."""
        if not self._ar_mode:
            raise RuntimeError("set_episode_start: auto-reset is off (enable_auto_reset first)")
        self.batch.snapshot_episode_start()

    def refresh_reset_noise(self) -> None:
        """Redraw the reset-noise pool in place (randn * sigma from the env's generator); nothing to do without one."""
        if not self._ar_mode:
            raise RuntimeError("refresh_reset_noise: auto-reset is off (enable_auto_reset first)")
        pool = self.batch.reset_noise
        if pool is not None:
            pool.copy_(torch.randn(pool.shape, generator=self._gen, device=self.device) * self.sigma)

    def _ar_out(self) -> dict:
        """Auto-reset's outputs (or none)."""
        return {"reset": self.reset_out, "final_obs": self.final_obs} if self._ar_mode else {}

    def enable_info_extras(self) -> None:
        """Start producing info['momentum'] and info['nonfinite'] every step (one small per-walker pass after the
        step kernel).  The other output tensors stay the same objects; graphs captured before this raise on replay."""
        if not self._extras:
            # only the two new buffers (reallocating every output silently detached the tensors a caller
            # still held from step()); the generation bump makes cached plans and graphs rebuild / refuse
            self._extras = True
            self.momentum = torch.zeros((self.N, 3), dtype=torch.float32, device=self.device)
            self.nonfinite = torch.zeros(self.N, dtype=torch.bool, device=self.device)
            self._generation += 1

    def _outputs(self, obs=None, reward=None, done=None, centroid=None, energy=None, obs_step=0, out_step=0,
                 pad_clean=False, steps=None, nonfinite=None, momentum=None, reset=None, final_obs=None):
        p = _lib.ptr
        return _lib.WgOutputs(obs=p(obs), obs_stride=self.obs_dim, reward=p(reward), done=p(done),
                              centroid=p(centroid), energy=p(energy), obs_step=obs_step, out_step=out_step,
                              obs_pad_clean=int(pad_clean), steps=p(steps), nonfinite=p(nonfinite),
                              momentum=p(momentum), reset=p(reset), final_obs=p(final_obs))

    def _own_outputs(self, pad_clean: bool = True, auto_reset: bool = True):
        """The whole batch's WgOutputs over the env's own one-step tensors (step, policy_loop, observe)."""
        return self._outputs(self.obs, self.reward, self.done, self.centroid, self.energy, pad_clean=pad_clean,
                             steps=self.steps_out, **self._extra_out(), **(self._ar_out() if auto_reset else {}))

    @staticmethod
    def _range_outputs(o, w0: int):
        """The WgOutputs of a uniform walker range starting at walker w0: o's pointers advanced by w0 rows (every output
        is walker-major: obs rows of obs_stride floats, f32 reward / energy, 1-byte done / nonfinite, int32 steps,
        3 x f32 centroid / momentum).  Pointer arithmetic instead of tensor slices: no per-call tensor views."""
        def adv(ptr, nbytes):
            return None if not ptr else C.c_void_p(ptr + nbytes)
        return _lib.WgOutputs(obs=adv(o.obs, 4 * w0 * o.obs_stride), obs_stride=o.obs_stride,
                              reward=adv(o.reward, 4 * w0), done=adv(o.done, w0), centroid=adv(o.centroid, 12 * w0),
                              energy=adv(o.energy, 4 * w0), obs_step=o.obs_step, out_step=o.out_step,
                              obs_pad_clean=o.obs_pad_clean, steps=adv(o.steps, 4 * w0),
                              nonfinite=adv(o.nonfinite, w0), momentum=adv(o.momentum, 12 * w0),
                              reset=adv(o.reset, w0), final_obs=adv(o.final_obs, 4 * w0 * o.obs_stride))

    def _extra_out(self) -> dict:
        """The opt-in info outputs (or none)."""
        return {"nonfinite": self.nonfinite, "momentum": self.momentum} if self._extras else {}

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def set_params(self, **kw):
        for k, v in kw.items():
            if not hasattr(self.params, k):
                raise AttributeError(k)
            setattr(self.params, k, v)
        obs_len = self.batch.host.obs_len(self.params.in3d, self.params.conmid)
        if not np.array_equal(obs_len, self.obs_len):   # new row lengths: fresh zero-padded outputs
            self.obs_len = obs_len
            self.obs_dim = int(obs_len.max())
            self._alloc_outputs()
        if int(self.params.pair_mode) & 4:
            self.batch.enable_radius()
        if self._needs_plan() and self.batch.wave_ok != self._wave_ok():
            self.batch.replan(self._wave_ok())   # the plan kind follows the parameters (DeviceBatch.replan)
        self._pstruct = self._make_pstruct()
        self._generation += 1   # graphs captured before this replay stale parameters: WalkerGraph refuses them

    def _wave_ok(self) -> bool:
        """The parameters can run on the barrier-free wave kernels (engine.py springs, no pair forces)."""
        return int(self.params.spring_mode) == 0 and int(self.params.pair_mode) == 0

    def _needs_plan(self) -> bool:
        """Batches whose launch plan depends on the parameters: ragged, or uniform with M not dividing 64."""
        M = self.batch.M
        return bool(self.batch.host.ragged) or not (4 <= M <= 64 and 64 % M == 0)

    def resident_ok(self) -> bool:
        """wg_rollout keeps the walkers in registers across steps (one launch for every step) for this batch and
        these parameters: uniform, M | 64, engine.py springs, no pair forces (otherwise it steps like wg_step)."""
        M = self.batch.M
        return (not self.batch.ragged and 4 <= M <= 64 and 64 % M == 0 and self._wave_ok()
                and os.environ.get("WG_LEAN", "1") != "0")

    def _check_action(self, action):
        if action is None:
            return None, 0
        if (isinstance(action, torch.Tensor) and action.dim() == 2 and action.dtype == torch.float32
                and action.device == self.device and action.shape[0] == self.N and action.is_contiguous()):
            return action, action.shape[1]                      # the closed-loop fast path: used as given
        if not isinstance(action, torch.Tensor):
            action = torch.as_tensor(np.asarray(action, dtype=np.float32))
        action = action.to(self.device, torch.float32)
        if action.dim() == 1 and self.N == 1:
            action = action[None]
        if action.dim() != 2 or action.shape[0] != self.N:
            raise ValueError(f"action must be [N={self.N}, A], got {tuple(action.shape)}")
        return action.contiguous(), action.shape[1]

    # ------------------------------------------------------------------ API
    def step(self, action=None):
        """One env step for all walkers: act -> physics -> run1 -> obs/reward/done/info: one launch per walker range
        (the default ranges, forked from and joined back to the calling stream inside one wg_step_ranges call).  The
        C arguments of every range are built once and cached (_step_plan): a closed-loop caller pays one ctypes
        call per step."""
        act, cols = self._check_action(action)
        plan = self._step_plan(cols if act is not None else -1)
        cur = torch.cuda.current_stream(self.device)
        rng = plan["ranges"]
        rng[0].stream = cur.cuda_stream
        rc = plan["fn"](rng, plan["n"], self._pref, act.data_ptr() if act is not None else None, cols, cols,
                        plan["events"])
        if rc:
            _lib.check(rc, "wg_step_ranges")
        self._steps_at = self.batch.version
        self._stale = frozenset()
        if act is not None and plan["n"] > 1 and not torch.cuda.is_current_stream_capturing():
            for st in plan["side"]:
                act.record_stream(st)   # the allocator must not recycle the actions before the side streams read them
        return self.obs, self.reward, self.done, self.info()

    def _step_plan(self, cols: int) -> dict:
        """step()'s wg_step_ranges arguments for this env's own output tensors, cached per (generation, batch struct,
        action columns): one wg_range per walker range (uniform: offset batch views; ragged: plan slices), the
        outputs, the action element offset of each range, its stream, and the fork / join events."""
        key = (self._generation, id(self.batch.struct), cols)
        cached = self._plan_cache
        if cached is not None and cached["key"] == key:
            return cached
        lanes = self._step_lanes() if cols >= 0 else 1
        ranges = self._ranges(lanes, self._own_outputs(), max(cols, 0))
        events = self._make_events(lanes)
        self._pref = C.byref(self._pstruct)
        self._plan_cache = {"key": key, "fn": _lib.load().wg_step_ranges, "ranges": self._wg_ranges(ranges), "n": lanes,
                            "side": self._side[:lanes - 1], "keep": ranges, "events_obj": events[0], "events": events[1]}
        return self._plan_cache

    def _ranges(self, lanes: int, o_full, cols: int = 0, caller_rows: bool = False) -> list:
        """The one description of the batch as `lanes` walker ranges (ranges.WalkerRange) writing to o_full, the whole
        batch's WgOutputs, and reading [N, cols] actions: step, run (both issue orders) and policy_loop all step these.
        A uniform batch splits at walker bounds: each range has its cached WgBatch view, o_full advanced to its first
        walker and its action offset.  A ragged batch splits its block -> walker plan: every range has the one batch
        struct and o_full (the kernels index both by caller row), and a slice of the plan; caller_rows moves the splits
        to where the ranges are slices of caller rows (_caller_bounds; policy_loop hands each range its own rows)."""
        b = self.batch
        self.reserve_streams(lanes)
        if b.ragged:
            bb, contiguous = self._caller_bounds(lanes) if caller_rows else \
                (block_bounds(b.plan_blocks, lanes), [None] * lanes)
            first, plan = [int(b.plan_host[k]) for k in bb], b.plan.data_ptr()
            return [WalkerRange(b.struct, o_full, plan + 4 * bb[i], bb[i + 1] - bb[i], 0, first[i],
                                first[i + 1] - first[i], contiguous[i], i) for i in range(lanes)]
        if lanes == 1:
            return [WalkerRange(b.struct, o_full, None, 0, 0, 0, self.N, True, 0)]
        bounds = uniform_bounds(self.N, lanes)
        subs = self._range_batches(lanes, bounds)
        return [WalkerRange(subs[i], self._range_outputs(o_full, w0), None, 0, w0 * cols, w0, bounds[i + 1] - w0, True, i)
                for i, w0 in enumerate(bounds[:-1])]

    def _wg_ranges(self, ranges):
        """The wg_range array of wg_step_ranges / wg_run_ranges over `ranges` (which it points into: keep them), range
        0 on the current stream."""
        streams = [torch.cuda.current_stream(self.device)] + self._side
        rng = (_lib.WgRange * len(ranges))()
        for g, r in zip(rng, ranges):
            g.batch, g.outputs, g.action_offset = C.pointer(r.batch), C.pointer(r.outputs), r.action_offset
            g.plan, g.plan_blocks, g.stream = r.plan, r.plan_blocks, streams[r.slot].cuda_stream
        return rng

    @staticmethod
    def _make_events(n: int):
        """n torch events and the array of their hipEvent handles (fork / join events of the range entries)."""
        objs = [torch.cuda.Event() for _ in range(n)]
        for e in objs:
            e.record()                       # materialise the hipEvent handle
        return objs, (C.c_void_p * n)(*[e.cuda_event for e in objs])

    def rollout(self, actions, obs_out=None, reward_out=None, done_out=None, lanes: Optional[int] = None,
                resident: bool = True, reset_out=None):
        """T steps in one C call, no host sync; outputs for every step.  resident (default): wg_rollout, one launch
        for all T steps where the batch allows it (uniform M | 64, no pair forces), each walker's state kept in
        registers between steps; False: wg_step, one launch per step.  Bit-identical either way.  It is resident with
        auto-reset too (the reset tail runs inside the launch); reset_out [T, N] uint8 (optional) receives every
        step's resets."""
        if not isinstance(actions, torch.Tensor):
            actions = torch.as_tensor(np.asarray(actions, dtype=np.float32))
        actions = actions.to(self.device, torch.float32).contiguous()
        if actions.dim() != 3 or actions.shape[1] != self.N:
            raise ValueError("actions must be [T, N, A]")
        T, _, cols = actions.shape
        dv = self.device
        self._steps_at = -1   # the step counters move without the steps output: info() gathers them afterwards
        # (the per-step outputs went to the rollout's buffers: the env's own centroid / energy / extras are not current)
        self._stale = _ROLLOUT_STALE
        # zero-filled: a ragged batch's short rows then need only their own values written each step
        clean = obs_out is None
        obs_out = torch.zeros((T, self.N, self.obs_dim), dtype=torch.float32, device=dv) if obs_out is None else obs_out
        reward_out = torch.empty((T, self.N), dtype=torch.float32, device=dv) if reward_out is None else reward_out
        done_out = torch.empty((T, self.N), dtype=torch.uint8, device=dv) if done_out is None else done_out
        require_tensor(obs_out, "obs_out", dv, torch.float32, (T, self.N, self.obs_dim))
        require_tensor(reward_out, "reward_out", dv, torch.float32, (T, self.N))
        require_tensor(done_out, "done_out", dv, torch.uint8, (T, self.N))
        if reset_out is not None:
            if not self._ar_mode:
                raise ValueError("rollout(reset_out=...) needs auto-reset (enable_auto_reset)")
            require_tensor(reset_out, "reset_out", dv, torch.uint8, (T, self.N))
        # one resident launch holds its walkers for all T steps: no per-step launch tail for a second range to fill
        # (profiles/r02_ab_resident_occupancy.json: 38.2 us/step with one range, 39.6 with two)
        # (only where the resident kernel actually runs: otherwise the default walker ranges keep their overlap)
        lanes = self._lanes(1 if (resident and lanes is None and self.resident_ok()) else lanes) if T > 0 else 1
        entry = "wg_rollout" if resident else "wg_step"
        o = self._outputs(obs_out, reward_out, done_out, None, None, obs_step=self.N * self.obs_dim,
                          out_step=self.N, pad_clean=clean, reset=reset_out)
        if lanes > 1:
            self._run_lanes(actions, T, o, lanes, entry=entry)
            return obs_out, reward_out, done_out
        _lib.check(getattr(_lib.load(), entry)(
            C.byref(self.batch.struct), C.byref(self._pstruct), C.c_void_p(actions.data_ptr()), cols, cols,
            self.N * cols, C.byref(o), T, *self.batch.plan_args(), self._stream()), entry)
        return obs_out, reward_out, done_out

    def rollout_policy(self, policy, n_steps: int, obs_out=None, reward_out=None, done_out=None,
                       action_out=None) -> dict:
        """A whole closed-loop episode in ONE launch (wg_rollout_policy): the resident kernel of rollout() with each
        step's actions computed inside the wave from the walker's own observation row by `policy`, an MLPPolicy
        (walker_gym_amd.policy) on this device.  Step 0 acts on the observation of the state at entry (what observe()
        returns), step s + 1 on step s's.  No per-step host work and no action traffic; the per-step buffers are
        optional and written only when given: obs_out [T, N, D] f32, reward_out [T, N] f32, done_out [T, N] u8,
        action_out [T, N, C] f32 (the actions applied at each step).  Returns {'returns': [N] f32, the rewards added
        in step order up to and including the walker's first done step (or all T); 'lengths': [N] i32, the steps
        counted}.  Walkers keep stepping after done, as in rollout(); there is no auto-reset on this path.
        Bit-identical to `for t: env.step(policy(env.obs, t))`.  A policy that carries an obs_norm
        (walker_gym_amd.normalize.ObsNorm) is evaluated on the normalised row inside the kernel (wg_rollout_normalized,
        here and in rollout_episodes / rollout_stochastic); the rows stored in obs_out stay raw.  A policy with a
        second hidden layer (MLPPolicy(wm=...)) runs through wg_rollout_deep, here and in rollout_episodes /
        rollout_stochastic / rollout_held, with the same arguments and results.

        ValueError (nothing launched, no silent fallback) for a batch the resident kernel does not take (ragged, M not
        dividing 64, spring_mode or pair_mode set, WG_LEAN=0), with auto-reset enabled, or for a policy that does not
        fit (D, C, G): close the loop with policy_loop(policy, n_steps) instead, which takes any batch (it binds an
        MLPPolicy's parameter sets to each walker range's caller rows).  Also ValueError (WG_ERANGE) when the rows,
        hidden vectors and actions of a workgroup's walkers beside the kernel's own LDS pass 80 KiB (very wide walkers
        with a large hidden layer)."""
        N, dv = self.N, self.device
        pol, o, T = self._resident_policy("rollout_policy", False, policy, n_steps, None, obs_out, reward_out, done_out,
                                          action_out)
        returns = torch.empty(N, dtype=torch.float32, device=dv)
        lengths = torch.empty(N, dtype=torch.int32, device=dv)
        pol.return_out, pol.length_out = _lib.ptr(returns), _lib.ptr(lengths)
        if policy.H2:
            self._rollout_deep(policy, pol, None, None, o, None, T)
        elif policy.obs_norm is not None:
            self._rollout_normalized(policy, pol, None, o, None, T)
        else:
            _lib.check(_lib.load().wg_rollout_policy(C.byref(self.batch.struct), C.byref(self._pstruct), C.byref(pol),
                                                     C.byref(o), T, self._stream()), "wg_rollout_policy")
        self._steps_at = -1   # (as rollout(): the env's one-step outputs are not this call's; a refused call ran nothing)
        self._stale = _ROLLOUT_STALE
        return {"returns": returns, "lengths": lengths}

    def _rollout_normalized(self, policy, pol, nz, o, st, T):
        """The launch of a policy that carries an ObsNorm (wg_rollout_normalized): the mode is the env's auto-reset
        setting, nz / st are byref'd structs or None."""
        nm = policy.obs_norm.struct()
        _lib.check(_lib.load().wg_rollout_normalized(C.byref(self.batch.struct), C.byref(self._pstruct), C.byref(pol),
                                                     C.byref(nm), nz, C.byref(o), st, T, self._stream()),
                   "wg_rollout_normalized")

    def _rollout_deep(self, policy, pol, nz, hold, o, st, T):
        """The launch of a policy with a second hidden layer (wg_rollout_deep, whatever the public method): the mode is
        the env's auto-reset setting; nz / hold / st are byref'd structs or None; the policy's ObsNorm is honoured."""
        mid = policy.mid_struct()
        nm = C.byref(policy.obs_norm.struct()) if policy.obs_norm is not None else None
        _lib.check(_lib.load().wg_rollout_deep(C.byref(self.batch.struct), C.byref(self._pstruct), C.byref(pol),
                                               C.byref(mid), nm, nz, hold, C.byref(o), st, T, self._stream()),
                   "wg_rollout_deep")

    def _resident_policy(self, entry: str, auto_reset: bool, policy, n_steps, episode_slots, obs_out, reward_out,
                         done_out, action_out, reset_out=None, final_obs_out=None):
        """The shared prelude of rollout_policy / rollout_episodes (`entry`, which needs auto-reset off / on): every
        refusal in one order, then (the WgPolicy struct, the WgOutputs over the optional [T, ...] buffers, T)."""
        from .policy import MLPPolicy
        alt = "use policy_loop(policy, n_steps), which closes the loop with one step launch per step on any batch"
        if not isinstance(policy, MLPPolicy):
            raise ValueError(f"{entry} needs an MLPPolicy; for another callable {alt}")
        T = int(n_steps)
        if T < 1:
            raise ValueError(f"{entry}: n_steps {n_steps} < 1")
        if episode_slots is not None and int(episode_slots) < 0:
            raise ValueError(f"{entry}: episode_slots {episode_slots} < 0")
        if not self.resident_ok():
            raise ValueError(f"{entry}: only batches of the resident lean kernel (uniform, M dividing 64 with "
                             f"M >= 4, spring_mode 0, pair_mode 0, WG_LEAN not 0); {alt}")
        if self._ar_mode and not auto_reset:
            raise ValueError(f"{entry}: auto-reset is enabled and the resident loop has no reset tail; {alt}")
        if auto_reset and not self._ar_mode:
            raise ValueError(f"{entry}: auto-reset is off (enable_auto_reset first); without episode roll-over "
                             "use rollout_policy")
        if policy.D != self.obs_dim:
            raise ValueError(f"{entry}: the policy takes {policy.D} inputs, the observation rows have {self.obs_dim}")
        if policy.C > self.batch.A:
            raise ValueError(f"{entry}: the policy has {policy.C} outputs, the walkers {self.batch.A} muscles")
        if self.N % policy.G != 0:
            raise ValueError(f"{entry}: {policy.G} parameter sets do not divide N = {self.N}; {alt}")
        dv, N, D = self.device, self.N, self.obs_dim
        for name in ("w1", "b1", "wm", "bm", "w2", "b2"):
            t = getattr(policy, name)
            if t is not None:
                require_tensor(t, f"policy.{name}", dv, torch.float32)
        if policy.obs_norm is not None:
            require_tensor(policy.obs_norm.mean, "policy.obs_norm.mean", dv, torch.float32, (D,))
            require_tensor(policy.obs_norm.scale, "policy.obs_norm.scale", dv, torch.float32, (D,))
        for name, t, dt, shape in (("obs_out", obs_out, torch.float32, (T, N, D)),
                                   ("reward_out", reward_out, torch.float32, (T, N)),
                                   ("done_out", done_out, torch.uint8, (T, N)),
                                   ("action_out", action_out, torch.float32, (T, N, policy.C)),
                                   ("reset_out", reset_out, torch.uint8, (T, N)),
                                   ("final_obs_out", final_obs_out, torch.float32, (T, N, D))):
            if t is not None:
                require_tensor(t, name, dv, dt, shape)
        o = self._outputs(obs_out, reward_out, done_out, None, None, obs_step=N * D, out_step=N, pad_clean=True,
                          reset=reset_out, final_obs=final_obs_out)
        return policy.struct(N, action_out), o, T

    def rollout_episodes(self, policy, n_steps: int, obs_out=None, reward_out=None, done_out=None, action_out=None,
                         reset_out=None, final_obs_out=None, episode_slots: int = 0) -> dict:
        """n_steps closed-loop steps with episode roll-over in ONE launch (wg_rollout_episodes): rollout_policy's
        resident kernel with auto-reset (enable_auto_reset first) inside its loop.  A walker whose step ends its episode
        starts the next one in the same launch, and its next action comes from the fresh observation row.  Bit-identical
        to `for t: env.step(policy(env.obs, t))` with auto-reset on, per-step outputs, final state and info()['episodes']
        included.  The per-step buffers are optional and written only when given: obs_out [T, N, D] f32, reward_out
        [T, N] f32, done_out [T, N] u8, action_out [T, N, C] f32, reset_out [T, N] u8 (the walkers reset at each step),
        final_obs_out [T, N, D] f32 (the terminal rows of the walkers reset at each step; other rows untouched).

        Returns, per walker and for this call alone: 'return_sum' f32 and 'length_sum' i32 over the episodes finished in
        the call, 'episodes' i32 their number, 'tail_return' f32 / 'tail_length' i32 the unfinished episode at the end
        (returns add the rewards in step order in float32).  With episode_slots > 0 also 'ep_returns' [N, slots] f32
        (NaN where unfilled) and 'ep_lengths' [N, slots] i32 (-1 where unfilled): the call's first `slots` finished
        episodes of each walker.

        ValueError (nothing launched) with auto-reset off (use rollout_policy), and for everything rollout_policy
        refuses on its own account: the batch, the policy's fit, the buffers, the LDS budget."""
        N, dv = self.N, self.device
        pol, o, T = self._resident_policy("rollout_episodes", True, policy, n_steps, episode_slots, obs_out, reward_out,
                                          done_out, action_out, reset_out, final_obs_out)
        slots = int(episode_slots)
        res = {"return_sum": torch.empty(N, dtype=torch.float32, device=dv),
               "length_sum": torch.empty(N, dtype=torch.int32, device=dv),
               "episodes": torch.empty(N, dtype=torch.int32, device=dv),
               "tail_return": torch.empty(N, dtype=torch.float32, device=dv),
               "tail_length": torch.empty(N, dtype=torch.int32, device=dv)}
        if slots > 0:
            res["ep_returns"] = torch.full((N, slots), float("nan"), dtype=torch.float32, device=dv)
            res["ep_lengths"] = torch.full((N, slots), -1, dtype=torch.int32, device=dv)
        p = _lib.ptr
        st = _lib.WgEpisodeStats(return_sum=p(res["return_sum"]), length_sum=p(res["length_sum"]),
                                 episodes_done=p(res["episodes"]), tail_return=p(res["tail_return"]),
                                 tail_length=p(res["tail_length"]), ep_return=p(res.get("ep_returns")),
                                 ep_length=p(res.get("ep_lengths")), ep_slots=slots)
        if policy.H2:
            self._rollout_deep(policy, pol, None, None, o, C.byref(st), T)
        elif policy.obs_norm is not None:
            self._rollout_normalized(policy, pol, None, o, C.byref(st), T)
        else:
            _lib.check(_lib.load().wg_rollout_episodes(C.byref(self.batch.struct), C.byref(self._pstruct), C.byref(pol),
                                                       C.byref(o), C.byref(st), T, self._stream()),
                       "wg_rollout_episodes")
        self._steps_at = -1   # (as rollout_policy(): only after the call was accepted)
        self._stale = _ROLLOUT_STALE
        return res

    def rollout_stochastic(self, policy, n_steps: int, sigma, seed: int, step_base: int = 0, walker_base: int = 0,
                           obs_out=None, reward_out=None, done_out=None, steps_out=None, action_out=None,
                           raw_action_out=None, eps_out=None, reset_out=None, final_obs_out=None,
                           episode_slots: int = 0) -> dict:
        """rollout_policy (auto-reset off) or rollout_episodes (auto-reset on) with seeded exploration noise in the
        policy's output layer, in ONE launch (wg_rollout_stochastic).  Output unit c of walker w at the call's step s:
            u = y + sigma[set][c] * aeps(seed, step_base + s, walker_base + w, c);   a = clip(u, -L, L)
        with y the deterministic pre-clip output and aeps a unit-variance Irwin-Hall(8) variate, one Philox call, a pure
        function of its four arguments (walker_gym_amd.pg.action_noise_numpy restates it bit for bit).  sigma: float32
        device tensor [G, C] ([C] for a shared policy), or a number for every unit.  Beside the other entries' per-step
        buffers: steps_out [T, N] i32 (info['steps'] after each step), action_out [T, N, C] the clipped a,
        raw_action_out [T, N, C] u, eps_out [T, N, C] aeps.  The density put on aeps or u is the caller's business.
        A rank that holds walkers [w0, w0 + N) of a larger population passes walker_base = w0; a rollout split into
        several calls passes the steps already taken as step_base.

        Returns rollout_policy's dict with auto-reset off and rollout_episodes' dict with it on; the same ValueErrors as
        those two (nothing launched; batches the resident kernel does not take are refused, there is no stochastic
        policy_loop), and for a sigma that does not fit, a seed outside uint64, episode_slots / reset_out /
        final_obs_out with auto-reset off, step_base + n_steps or walker_base + N past 2^32."""
        N, dv = self.N, self.device
        entry = "rollout_stochastic"
        ar = bool(self._ar_mode)
        slots = int(episode_slots)
        if not ar and (slots != 0 or reset_out is not None or final_obs_out is not None):
            raise ValueError(f"{entry}: episode_slots / reset_out / final_obs_out need auto-reset (enable_auto_reset)")
        pol, o, T = self._resident_policy(entry, ar, policy, n_steps, slots if ar else None, obs_out, reward_out,
                                          done_out, action_out, reset_out, final_obs_out)
        G, Cc = policy.G, policy.C
        if not 0 <= int(seed) < 1 << 64:
            raise ValueError(f"{entry}: seed is a uint64")
        if not (0 <= int(step_base) and int(step_base) + T <= 1 << 32):
            raise ValueError(f"{entry}: step_base {step_base} + n_steps {T} outside 0 .. 2^32")
        if not (0 <= int(walker_base) and int(walker_base) + N <= 1 << 32):
            raise ValueError(f"{entry}: walker_base {walker_base} + N {N} outside 0 .. 2^32")
        if sigma is None:
            raise ValueError(f"{entry}: sigma is required (a [G, C] float32 device tensor, or a number)")
        if not isinstance(sigma, torch.Tensor):
            sigma = torch.full((G, Cc), float(sigma), dtype=torch.float32, device=dv)
        elif sigma.dim() == 1 and G == 1:
            sigma = sigma[None]
        require_tensor(sigma, "sigma", dv, torch.float32, (G, Cc))
        for name, t, dt, shape in (("steps_out", steps_out, torch.int32, (T, N)),
                                   ("raw_action_out", raw_action_out, torch.float32, (T, N, Cc)),
                                   ("eps_out", eps_out, torch.float32, (T, N, Cc))):
            if t is not None:
                require_tensor(t, name, dv, dt, shape)
        p = _lib.ptr
        o.steps = p(steps_out)
        nz = _lib.WgActionNoise(seed=int(seed), step_base=int(step_base), walker_base=int(walker_base), sigma=p(sigma),
                                raw_out=p(raw_action_out), raw_out_step=N * Cc, eps_out=p(eps_out), eps_out_step=N * Cc)
        if ar:
            res = {"return_sum": torch.empty(N, dtype=torch.float32, device=dv),
                   "length_sum": torch.empty(N, dtype=torch.int32, device=dv),
                   "episodes": torch.empty(N, dtype=torch.int32, device=dv),
                   "tail_return": torch.empty(N, dtype=torch.float32, device=dv),
                   "tail_length": torch.empty(N, dtype=torch.int32, device=dv)}
            if slots > 0:
                res["ep_returns"] = torch.full((N, slots), float("nan"), dtype=torch.float32, device=dv)
                res["ep_lengths"] = torch.full((N, slots), -1, dtype=torch.int32, device=dv)
            st = C.byref(_lib.WgEpisodeStats(return_sum=p(res["return_sum"]), length_sum=p(res["length_sum"]),
                                             episodes_done=p(res["episodes"]), tail_return=p(res["tail_return"]),
                                             tail_length=p(res["tail_length"]), ep_return=p(res.get("ep_returns")),
                                             ep_length=p(res.get("ep_lengths")), ep_slots=slots))
        else:
            res = {"returns": torch.empty(N, dtype=torch.float32, device=dv),
                   "lengths": torch.empty(N, dtype=torch.int32, device=dv)}
            pol.return_out, pol.length_out = p(res["returns"]), p(res["lengths"])
            st = None
        if policy.H2:
            self._rollout_deep(policy, pol, C.byref(nz), None, o, st, T)
        elif policy.obs_norm is not None:
            self._rollout_normalized(policy, pol, C.byref(nz), o, st, T)
        else:
            _lib.check(_lib.load().wg_rollout_stochastic(C.byref(self.batch.struct), C.byref(self._pstruct),
                                                         C.byref(pol), C.byref(nz), C.byref(o), st, T, self._stream()),
                       "wg_rollout_stochastic")
        self._steps_at = -1   # (as rollout_policy(): only after the call was accepted)
        self._stale = _ROLLOUT_STALE
        return res

    def rollout_held(self, policy, n_steps: int, every: int, sigma=None, seed: int = 0, step_base: int = 0,
                     walker_base: int = 0, held=None, decided_out=None, hold_reward_out=None, obs_out=None,
                     reward_out=None, done_out=None, steps_out=None, action_out=None, raw_action_out=None, eps_out=None,
                     reset_out=None, final_obs_out=None, episode_slots: int = 0) -> dict:
        """The resident closed loop with an action hold (frame skip), in ONE launch (wg_rollout_held): a walker decides
        at the steps where its step counter at the start of the step (info['steps'], which auto-reset zeroes) is a
        multiple of `every`, and applies the action in force at the steps between.  A deciding walker's action is what
        rollout_policy / rollout_episodes (auto-reset off / on) computes at that step, or with `sigma` given what
        rollout_stochastic does (noise on counter step_base + s; a held step makes no draw); policy.obs_norm is
        honoured.  action_out holds the action applied at every step; raw_action_out / eps_out are written on the
        deciding rows only; decided_out [T, N] u8 marks them; hold_reward_out [T, N] f32 is the running reward of the
        open hold after each step (reward at a decision, then added in step order in float32).  held: float32 device
        tensor [N, C + 1], in and out: each walker's action in force and the running reward of its open hold; None
        starts from zeros.  It is returned under 'held' and passed to the next call, with step_base advanced, to
        continue: two calls of a and b steps equal one of a + b.  every = 1 is the existing entry bit for bit.

        Returns the mode's dict (rollout_policy's or rollout_episodes') plus 'held'.  The ValueErrors of the mode's
        entry and of rollout_stochastic, and for every < 1 or a held / decided_out / hold_reward_out that does not
        fit."""
        N, dv = self.N, self.device
        entry = "rollout_held"
        ar = bool(self._ar_mode)
        slots = int(episode_slots)
        if not ar and (slots != 0 or reset_out is not None or final_obs_out is not None):
            raise ValueError(f"{entry}: episode_slots / reset_out / final_obs_out need auto-reset (enable_auto_reset)")
        pol, o, T = self._resident_policy(entry, ar, policy, n_steps, slots if ar else None, obs_out, reward_out,
                                          done_out, action_out, reset_out, final_obs_out)
        G, Cc = policy.G, policy.C
        if int(every) < 1:
            raise ValueError(f"{entry}: every {every} < 1")
        if not 0 <= int(seed) < 1 << 64:
            raise ValueError(f"{entry}: seed is a uint64")
        if not (0 <= int(step_base) and int(step_base) + T <= 1 << 32):
            raise ValueError(f"{entry}: step_base {step_base} + n_steps {T} outside 0 .. 2^32")
        if not (0 <= int(walker_base) and int(walker_base) + N <= 1 << 32):
            raise ValueError(f"{entry}: walker_base {walker_base} + N {N} outside 0 .. 2^32")
        if sigma is None:
            if raw_action_out is not None or eps_out is not None:
                raise ValueError(f"{entry}: raw_action_out / eps_out need sigma (the stochastic form)")
        elif not isinstance(sigma, torch.Tensor):
            sigma = torch.full((G, Cc), float(sigma), dtype=torch.float32, device=dv)
        elif sigma.dim() == 1 and G == 1:
            sigma = sigma[None]
        if sigma is not None:
            require_tensor(sigma, "sigma", dv, torch.float32, (G, Cc))
        if held is None:
            held = torch.zeros((N, Cc + 1), dtype=torch.float32, device=dv)
        for name, t, dt, shape in (("steps_out", steps_out, torch.int32, (T, N)),
                                   ("raw_action_out", raw_action_out, torch.float32, (T, N, Cc)),
                                   ("eps_out", eps_out, torch.float32, (T, N, Cc)),
                                   ("held", held, torch.float32, (N, Cc + 1)),
                                   ("decided_out", decided_out, torch.uint8, (T, N)),
                                   ("hold_reward_out", hold_reward_out, torch.float32, (T, N))):
            if t is not None:
                require_tensor(t, name, dv, dt, shape)
        p = _lib.ptr
        o.steps = p(steps_out)
        nz = None
        if sigma is not None:
            nz = C.byref(_lib.WgActionNoise(seed=int(seed), step_base=int(step_base), walker_base=int(walker_base),
                                            sigma=p(sigma), raw_out=p(raw_action_out), raw_out_step=N * Cc,
                                            eps_out=p(eps_out), eps_out_step=N * Cc))
        hold = _lib.WgActionHold(every=int(every), held=p(held), decided_out=p(decided_out), decided_out_step=N,
                                 hold_reward_out=p(hold_reward_out), hold_reward_out_step=N)
        if ar:
            res = {"return_sum": torch.empty(N, dtype=torch.float32, device=dv),
                   "length_sum": torch.empty(N, dtype=torch.int32, device=dv),
                   "episodes": torch.empty(N, dtype=torch.int32, device=dv),
                   "tail_return": torch.empty(N, dtype=torch.float32, device=dv),
                   "tail_length": torch.empty(N, dtype=torch.int32, device=dv)}
            if slots > 0:
                res["ep_returns"] = torch.full((N, slots), float("nan"), dtype=torch.float32, device=dv)
                res["ep_lengths"] = torch.full((N, slots), -1, dtype=torch.int32, device=dv)
            st = C.byref(_lib.WgEpisodeStats(return_sum=p(res["return_sum"]), length_sum=p(res["length_sum"]),
                                             episodes_done=p(res["episodes"]), tail_return=p(res["tail_return"]),
                                             tail_length=p(res["tail_length"]), ep_return=p(res.get("ep_returns")),
                                             ep_length=p(res.get("ep_lengths")), ep_slots=slots))
        else:
            res = {"returns": torch.empty(N, dtype=torch.float32, device=dv),
                   "lengths": torch.empty(N, dtype=torch.int32, device=dv)}
            pol.return_out, pol.length_out = p(res["returns"]), p(res["lengths"])
            st = None
        if policy.H2:
            self._rollout_deep(policy, pol, nz, C.byref(hold), o, st, T)
        else:
            nm = C.byref(policy.obs_norm.struct()) if policy.obs_norm is not None else None
            _lib.check(_lib.load().wg_rollout_held(C.byref(self.batch.struct), C.byref(self._pstruct), C.byref(pol), nm, nz,
                                                   C.byref(hold), C.byref(o), st, T, self._stream()), "wg_rollout_held")
        self._steps_at = -1   # (as rollout_policy(): only after the call was accepted)
        self._stale = _ROLLOUT_STALE
        res["held"] = held
        return res

    def run(self, actions, n_steps: int, info: bool = True, lanes: Optional[int] = None, resident: bool = False,
            record: Optional[dict] = None, _only: Optional[int] = None):
        """Throughput path: n_steps env steps in one C call; step s acts with actions[s % T]
        ([T, N, A] device tensor; T == n_steps or 1) and overwrites obs/reward/done(/info) each step.  resident:
        wg_rollout (one launch for all steps where the batch allows it) instead of one launch per step.

        record: every step's reward / done (and with info, energy / centroid) into caller buffers instead of the
        env's one-step outputs — {'reward': [n_steps, N] f32, 'done': [n_steps, N] bool or u8, optionally 'energy'
        [n_steps, N] f32 and 'centroid' [n_steps, N, 3] f32} — while obs keeps the last step's rows (env.obs): the
        rollout SURVEY §8(e) gathers at its end.  The same bytes as a plain run, written at per-step offsets.  After a
        record run env.reward / done / centroid / energy and the info extras are not this run's (they went to the
        record buffers, or were not computed): info() leaves those keys out until the next step() / observe() / run()
        without record."""
        self.prepare_run(actions, n_steps, info=info, lanes=lanes, resident=resident, record=record, _only=_only)()

    def prepare_run(self, actions, n_steps: int, info: bool = True, lanes: Optional[int] = None,
                    resident: bool = False, record: Optional[dict] = None,
                    _only: Optional[int] = None) -> "PreparedRun":
        """run()'s argument checks, walker ranges and C structs, built once: the returned PreparedRun issues the same
        n_steps steps with ONE C call each time it is called (on the stream that was current here), so the host time
        between a caller's clock start and the first launch is one ctypes call (bench.py builds it before its timed
        region: ~35 us of Python before the first launch otherwise).  It holds raw pointers to `actions`,
        the record buffers and the env's tensors: set_params / a reallocation of the outputs make it raise.
        (_only = i, graph() only: walker range i alone, on the calling stream.)"""
        require_tensor(actions, "actions", self.device, torch.float32)
        if actions.dim() != 3:
            raise ValueError("actions must be a contiguous [n_steps or 1, N, A] device tensor")
        T, n, cols = actions.shape
        if n != self.N or T not in (1, n_steps):
            raise ValueError("actions must be a contiguous [n_steps or 1, N, A] device tensor")
        lanes = self._lanes(1 if (resident and lanes is None and self.resident_ok()) else lanes)
        entry = "wg_rollout" if resident else "wg_step"
        so = self.steps_out if info else None
        rew, done, cen, en, out_step = self.reward, self.done, self.centroid, self.energy, 0
        stale = frozenset()
        if record is not None:
            S = int(n_steps)
            if S < 1:
                raise ValueError("run(record=...) needs n_steps >= 1")
            stale = _INFO_STALE
            rew, done = record["reward"], record["done"]
            require_tensor(rew, "record['reward']", self.device, torch.float32, (S, self.N))
            if not isinstance(done, torch.Tensor) or done.dtype not in (torch.bool, torch.uint8):
                raise ValueError("record['done'] must be a bool or uint8 tensor")
            require_tensor(done, "record['done']", self.device, done.dtype, (S, self.N))
            cen, en = record.get("centroid"), record.get("energy")
            if cen is not None:
                require_tensor(cen, "record['centroid']", self.device, torch.float32, (S, self.N, 3))
            if en is not None:
                require_tensor(en, "record['energy']", self.device, torch.float32, (S, self.N))
            rew, done = rew[0], done[0]
            cen, en = (None if cen is None else cen[0]), (None if en is None else en[0])
            so, out_step = None, self.N   # (the steps output would need [n_steps, N] too: info() gathers them)
        if not info:
            cen = en = None
            stale = _INFO_STALE
        # the opt-in info extras follow the last step only when the outputs are overwritten each step (no record)
        # (auto-reset's outputs likewise: a record run strides its outputs per step, so it takes record['reset'] [n_steps,
        # N] uint8 / bool, if given, and no final_obs)
        ar_out = self._ar_out()
        if record is not None and self._ar_mode:
            rs = record.get("reset")
            if rs is not None:
                if not isinstance(rs, torch.Tensor) or rs.dtype not in (torch.bool, torch.uint8):
                    raise ValueError("record['reset'] must be a bool or uint8 tensor")
                require_tensor(rs, "record['reset']", self.device, rs.dtype, (int(n_steps), self.N))
            ar_out = {"reset": None if rs is None else rs[0]}
            stale |= {"reset", "final_obs"}
        o = self._outputs(self.obs, rew, done, cen, en, pad_clean=True, steps=so, out_step=out_step,
                          **(self._extra_out() if (info and record is None) else {}), **ar_out)
        # every tensor whose raw pointer sits in `o`, held by the PreparedRun (a caller that drops its record
        # buffers and calls the PreparedRun again must not have the kernel write into freed memory)
        pins = [self.obs, so, actions, *(() if record is None else record.values()), *self._extra_out().values(),
                *self._ar_out().values()]
        steps_valid = so is not None
        n_steps = int(n_steps)
        if lanes > 1:
            capturing = torch.cuda.is_current_stream_capturing()
            if entry == "wg_step" and not capturing and _only is None and \
                    os.environ.get("WG_RANGE_ISSUE", "inter") != "seq":
                fn, args, keep = self._run_ranges_args(actions, n_steps, o, lanes)
                if n_steps > 0:
                    for st in self._side[:lanes - 1]:
                        actions.record_stream(st)   # the allocator must not recycle it before the side streams are done
                return PreparedRun(self, "wg_run_ranges", fn, args, keep + pins, steps_valid, stale)
            # (range-by-range issue, a resident rollout over several ranges, or a graph capture: one C call per range)
            return PreparedRun(self, entry, None, (actions, n_steps, o, lanes, entry, _only), [o] + pins, steps_valid,
                               stale, thunk=self._run_lanes)
        # (a resident launch writes the steps output only where the resident kernel runs: uniform batches, which
        # have no steps_out)
        args = (C.byref(self.batch.struct), C.byref(self._pstruct), actions.data_ptr(), cols, cols,
                0 if T == 1 else self.N * cols, C.byref(o), n_steps, *self.batch.plan_args(),
                torch.cuda.current_stream(self.device).cuda_stream)
        return PreparedRun(self, entry, getattr(_lib.load(), entry), args, [o] + pins, steps_valid, stale)

    def time_launches(self, actions, n_steps: int, info: bool = True) -> float:
        """Measurement aid (bench.py's roofline): run(actions, n_steps, lanes=1)'s steps — one full-batch launch per
        step, the same results — with each step kernel's own start and end stamped on events of its own (wg_time_step,
        hipExtLaunchKernel: the dispatch's timestamps, as a kernel trace reports them, without the gaps between
        back-to-back launches).  Waits for the calling stream; returns the mean kernel duration in ms."""
        prep = self.prepare_run(actions, n_steps, info=info, lanes=1)
        ms = C.c_float(0.0)
        _lib.check(_lib.load().wg_time_step(*prep._args, C.byref(ms)), "wg_time_step")
        self._steps_at = self.batch.version if prep._steps_valid else -1   # (as PreparedRun.__call__)
        self._stale = prep._stale
        return float(ms.value)

    def _lanes(self, lanes: Optional[int]) -> int:
        """Walker ranges run() steps on separate streams (ragged batches: ranges of plan blocks).  Default 2 for
        batches of >= 2^19 masses: measured on the canonical 65,536-walker bench (2^20 masses), 36.5 us/step
        with 2 ranges against 42.9 with 1 and 49.0 with 4; on 65,536 Balance-v0 walkers (2^18 masses, a 13 us
        launch) 2 ranges lose slightly, 13.7 against 13.3 (scripts/lanes_ab.py; bit-identical results).  Pair
        forces (O(M^2) per walker) make launches long at fewer masses: 4,096 chain walkers of 100 masses (2^18.6),
        175 us/step with 2 ranges against 210 with 1 (profiles/r02_ab_pair_markstein_chain.json), so those
        batches take 2 ranges from 2^17 masses.  WG_LANES overrides."""
        if lanes is None:
            env = os.environ.get("WG_LANES")
            heavy = int(self.params.pair_mode) != 0
            lanes = int(env) if env else (2 if self.batch.P >= (1 << (17 if heavy else 19)) else 1)
        if lanes < 1:
            raise ValueError("lanes must be >= 1")
        if self.batch.ragged:
            return max(1, min(lanes, self.batch.plan_blocks // 64))
        return 1 if self.N < 64 * lanes else lanes

    def _step_lanes(self) -> int:
        """Walker ranges of step(): 1 unless WG_STEP_LANES says otherwise.  step() joins its ranges at the end of
        every call, so a second range cannot fill the first one's launch tail with its next step (what pays in
        run()), and the fork / join events cost host time on every call: measured on the canonical 65,536-walker
        batch, a step() loop ran 47.7 us per step with 1 range against 58.5 with 2 (host 7.8 against 25.1 us per
        call; scripts/step_overhead.py, profiles/r03g_step_overhead_canonical.json)."""
        env = os.environ.get("WG_STEP_LANES")
        return self._lanes(int(env)) if env else 1

    def reserve_streams(self, lanes: int) -> None:
        """Side streams for `lanes` walker ranges (lanes - 1 of them; existing ones are kept, so their hardware
        queues stay bound).  Call before creating other streams (an RCCL process group) to keep the ranges on
        queues of their own."""
        while len(self._side) < lanes - 1:
            self._side.append(torch.cuda.Stream(device=self.device))

    def _range_batches(self, lanes: int, bounds) -> list:
        """The per-range WgBatch views of a uniform batch, cached per batch struct (rebuilt whenever the batch's
        arrays are: enable_radius) and walker ranges; the cache holds the struct, so its identity is not reused."""
        key, st = (self._generation, tuple(bounds)), self.batch.struct
        cached = self._range_cache
        if cached is None or cached[0] != key or cached[1] is not st:
            cached = self._range_cache = (key, st, [self.batch.sub_struct(bounds[i], bounds[i + 1]) for i in range(lanes)])
        return cached[2]

    def _run_ranges_args(self, actions, n_steps: int, o_full, lanes: int):
        """wg_run_ranges' arguments for n_steps of `lanes` walker ranges on the calling stream and the side streams:
        step s of every range is issued before step s + 1 of any (WG_RANGE_ISSUE=seq keeps range-by-range issue, one
        wg_step call each: the last range then starts only after the host has issued every launch of the ranges
        before it; scripts/issue_ab.sh).  Returns (function, arguments, the ctypes objects they point at)."""
        T, n, cols = actions.shape
        ranges = self._ranges(lanes, o_full, cols)
        rng = self._wg_ranges(ranges)
        args = (rng, lanes, C.byref(self._pstruct), actions.data_ptr(), cols, cols, 0 if T == 1 else self.N * cols,
                n_steps, self._range_events(lanes))
        return _lib.load().wg_run_ranges, args, [ranges, rng, o_full, actions]

    def _run_lanes(self, actions, n_steps: int, o_full, lanes: int, entry: str = "wg_step", only: Optional[int] = None):
        """n_steps with the walkers split into `lanes` contiguous ranges, each stepped by its own stream, one C call
        per range (the range-by-range form; prepare_run issues the ranges step by step through wg_run_ranges): the
        ranges are independent, so one range's step t + 1 fills the GPU while another's step t drains (the
        launch tail).  Every walker still takes every step, one launch per step per range; the calling
        stream waits for all ranges before returning (stream-ordered, no host sync).  o_full: the whole batch's
        WgOutputs (a uniform range's are its pointers advanced to the range's first walker).  only = i: range i
        alone, on the calling stream (graph() captures one graph per range)."""
        T, n, cols = actions.shape
        cur = torch.cuda.current_stream(self.device)
        fn = getattr(_lib.load(), entry)
        ranges = self._ranges(lanes, o_full, cols)
        capturing = torch.cuda.is_current_stream_capturing()
        start = torch.cuda.Event()
        if only is None:
            start.record(cur)
        done = []
        for r in (ranges if only is None else [ranges[only]]):
            st = cur if (r.slot == 0 or only is not None) else self._side[r.slot - 1]
            if st is not cur:
                st.wait_event(start)
            _lib.check(fn(C.byref(r.batch), C.byref(self._pstruct), C.c_void_p(actions.data_ptr() + 4 * r.action_offset),
                          cols, cols, 0 if T == 1 else self.N * cols, C.byref(r.outputs), n_steps, r.plan,
                          r.plan_blocks, C.c_void_p(st.cuda_stream)), entry)
            if st is not cur:
                if not capturing:
                    actions.record_stream(st)   # the allocator must not recycle it before the side stream is done
                ev = torch.cuda.Event()
                ev.record(st)
                done.append(ev)
        for ev in done:
            cur.wait_event(ev)

    def _range_events(self, lanes: int):
        """wg_run_ranges' fork / join events (hipEvent handles of torch events, created once per env and reused: each
        call records and waits on them stream-ordered)."""
        if self._run_events is None or len(self._run_events[0]) < lanes:
            self._run_events = self._make_events(lanes)
        return self._run_events[1]

    def policy_loop(self, policy, n_steps: int, lanes: Optional[int] = None, graph: bool = False):
        """A closed loop with a per-walker policy, the walker ranges pipelined: at every step, each range computes its
        actions from ITS OWN current observation rows, action = policy(obs[w0:w1], t), and launches its step right
        after, on its own stream; the ranges never wait for one another.  So one range's step t + 1 fills the other's
        launch tail, as in the open-loop run(), while every action still depends on the observation it follows.
        step() in a loop cannot do that: it returns the whole batch's obs, so each step ends at a full barrier and
        each launch drains on its own (the drain is what separates one launch from two overlapped ranges).

        policy(obs_rows [n_r, D] view, t) -> actions [n_r, A_cols] float32, contiguous, on the current (range)
        stream.  A policy that offers for_rows(first_row, N) and for_row_index(rows, N) (MLPPolicy: several parameter
        sets, caller row r using set r // (N // G)) is bound to each range's caller rows, so it never has to guess which
        walkers a slice of rows belongs to.  It must be row-wise — walker w's action a function of walker w's observation only — which is what
        makes the ranges independent; then the results are bit-identical to `for t: env.step(policy(env.obs, t))`.
        graph=True captures the n_steps x ranges loop (policy kernels included) as one HIP graph and replays it once
        (no per-step host cost; the policy must be capturable).  It then returns the captured loop: its replay() runs the
        same n_steps again from the current state (eager calls return None).  After the call obs / reward / done / info hold the last
        step's outputs.

        Ragged batches (stored in wave-tile order, wg_batch.row) run ranges of plan blocks.  The wave tiles are packed
        within windows of consecutive caller walkers (layout.wave_tile_order), so a range that ends at a block whose
        stored prefix is exactly the caller rows before it covers a contiguous slice of caller rows: the ranges are
        split at the such block nearest to an even split (_caller_bounds), and each range reads its obs rows as a
        slice and hands the kernel its actions as given.  Where no such block is near, a range's walkers are a
        scattered set of caller rows: it gathers its rows of obs (index_select), applies the policy and scatters the
        actions into its rows of one [N, A] action buffer (index_copy_), which its step reads by caller row.  Either
        way the ranges' rows are disjoint, so they never wait for one another.

        Host cost per range and step (what bounds a small batch's loop): the policy's own launches, a shape / dtype
        check against the first step's actions, and one C call; the stream is switched only when there are several
        ranges (one range runs on the calling stream as it is)."""
        b = self.batch
        lanes = self._lanes(lanes)
        L = _lib.load()
        pref, dev, f32 = C.byref(self._pstruct), self.device, torch.float32
        # (a ragged batch has no auto-reset: its _own_outputs hold none of auto-reset's outputs)
        ranges = self._ranges(lanes, self._own_outputs(), caller_rows=True)
        # per range: (obs rows or None, row index or None, n_r, batch ref, outputs ref, plan ptr, blocks): its caller
        # rows are a slice of obs, or (a ragged range of scattered rows) the rows its stored walkers name
        args = [(self.obs[r.row0:r.row0 + r.n] if r.contiguous else None,
                 None if r.contiguous else b._perm["row"][r.row0:r.row0 + r.n], r.n, C.byref(r.batch),
                 C.byref(r.outputs), None if r.plan is None else C.c_void_p(r.plan), r.plan_blocks) for r in ranges]
        # per range: the caller row its actions start at: the kernel indexes a ragged batch's actions by caller row, so
        # a slice's action pointer is moved back by that many rows (a uniform range's view indexes from its own first)
        aoff = [r.row0 if b.ragged else 0 for r in ranges]

        # a policy whose output depends on the walker index (MLPPolicy with G > 1): one bound policy per range, made
        # here (outside any capture), for the range's caller rows: a slice [row0, row0 + n_r), or a scattered ragged
        # range's row index
        pols = [policy] * lanes
        if hasattr(policy, "for_rows") and hasattr(policy, "for_row_index"):
            pols = [policy.for_rows(r.row0, self.N, r.n) if r.contiguous else policy.for_row_index(a[1], self.N)
                    for r, a in zip(ranges, args)]

        def check(a, n_r):
            require_tensor(a, "policy actions", dev, f32)
            if a.dim() != 2 or a.shape[0] != n_r:
                raise ValueError(f"policy returned {tuple(a.shape)}, expected [{n_r}, A]")

        def body(cur, only=None):
            # only = r: range r's loop alone, on `cur` (graph mode captures one graph per range)
            multi = lanes > 1 and only is None
            streams = [cur] + self._side[:lanes - 1] if only is None else [cur]
            if multi:
                start = torch.cuda.Event()
                start.record(cur)
                for st in streams[1:]:
                    st.wait_event(start)
            step = L.wg_step
            sts = [(st, st.cuda_stream) for st in streams]
            rng = list(enumerate(args)) if only is None else [(only, args[only])]
            shapes = [None] * lanes
            dix = dev.index
            # scattered ragged ranges: the [N, A] action buffer they scatter into.  Its columns are known only from the
            # first policy call, so it is allocated then, on `cur` (uninitialised: every range writes its own rows
            # before its step reads them), and an event recorded on `cur` right after the allocation orders every
            # stream that touches it after whatever `cur` ran in that memory before (the caching allocator reuses a
            # block freed on `cur` without waiting for other streams); the ranges' streams join `cur` at the end, so
            # its release on `cur` is ordered after their last reads
            abuf, abuf_ev, abuf_ok = None, None, set()
            try:
                for t in range(int(n_steps)):
                    for (r, (obs_r, idx, n_r, b_ref, o_ref, plan, nblk)), (st, st_ptr) in zip(rng, sts):
                        if multi:
                            torch.cuda.set_stream(st)
                        a = pols[r](obs_r if idx is None else self.obs.index_select(0, idx), t)
                        # the full check at a range's first step, then the same shape, dtype, device and layout
                        if shapes[r] is None:
                            check(a, n_r)
                            if r > 0 and shapes[0] is not None and a.shape[1] != shapes[0][1]:
                                raise ValueError("policy actions: every walker range must return the same columns")
                            shapes[r] = a.shape
                        elif not (a.shape == shapes[r] and a.dtype == f32 and a.get_device() == dix and
                                  a.is_contiguous()):
                            check(a, n_r)
                            raise ValueError(f"policy actions changed shape: {tuple(a.shape)} after "
                                             f"{tuple(shapes[r])}")
                        cols = a.shape[1]
                        if idx is not None:   # a scattered ragged range: its caller rows of the action buffer
                            if abuf is None:
                                with torch.cuda.stream(cur):
                                    abuf = torch.empty((self.N, cols), dtype=f32, device=dev)
                                abuf_ok.add(cur.cuda_stream)
                                if multi:   # (one stream, e.g. a captured range: nothing to order)
                                    abuf_ev = torch.cuda.Event()
                                    abuf_ev.record(cur)
                            if abuf_ev is not None and st_ptr not in abuf_ok:
                                st.wait_event(abuf_ev)
                                abuf_ok.add(st_ptr)
                            abuf.index_copy_(0, idx, a)
                            a_ptr = abuf.data_ptr()
                        else:                 # (rows aoff[r] .. of the caller's order: the pointer moved back)
                            a_ptr = a.data_ptr() - 4 * aoff[r] * cols
                        rc = step(b_ref, pref, a_ptr, cols, cols, 0, o_ref, 1, plan, nblk, st_ptr)
                        if rc:
                            _lib.check(rc, "wg_step")
            finally:
                if multi:
                    torch.cuda.set_stream(cur)
            for st in streams[1:]:
                ev = torch.cuda.Event()
                ev.record(st)
                cur.wait_event(ev)

        self._steps_at = -1
        self._stale = frozenset()
        cur = torch.cuda.current_stream(self.device)
        if not graph:
            body(cur)
            return
        # (kept until the next call: the replay may still be running)
        self._policy_graph = self._capture_ranges(lanes, lambda st, r: body(st, only=r))
        self._policy_graph.replay()
        return self._policy_graph   # replay() runs the same n_steps again from the current state

    def _capture_ranges(self, lanes: int, body) -> _RangeGraphs:
        """One HIP graph per walker range, body(stream, r) captured on a stream of its own (off the default stream, as
        torch requires): the ranges share nothing, and two graphs on two streams overlap as the eager ranges do (one
        graph with the ranges as parallel branches replayed them one after the other: 48.1 against 38.1 us per canonical
        step, round 4)."""
        cur = torch.cuda.current_stream(self.device)
        parts = []
        for r in range(lanes):
            g = torch.cuda.CUDAGraph()
            st = torch.cuda.Stream(device=self.device)
            st.wait_stream(cur)
            with torch.cuda.stream(st):
                with torch.cuda.graph(g, stream=st):
                    body(st, r)
            cur.wait_stream(st)
            parts.append((g, st))
        return _RangeGraphs(parts, cur)

    def _caller_bounds(self, lanes: int):
        """Plan-block bounds of `lanes` ragged walker ranges with the splits moved to where the ranges are slices of
        caller rows, and per range whether it is one (ranges.caller_bounds)."""
        b = self.batch
        return caller_bounds(b.plan_blocks, b.plan_host, b.host.row, lanes)

    def graph(self, actions, n_steps: int, info: bool = True, lanes: Optional[int] = None):
        """Capture run(actions, n_steps) into a HIP graph (torch.cuda.CUDAGraph over the ROCm runtime) and
        return it as a WalkerGraph; replay() then advances the batch n_steps with one host call: one graph per walker
        range, each replayed on its own stream, forked from and joined back to the calling stream (_RangeGraphs).  `actions` is kept alive by the WalkerGraph (and may be
        refilled in place); the graph reads the batch and output tensors this env owns and the parameters as
        captured, so set_params() (or any reallocation of the outputs) makes replay() raise."""
        lanes = self._lanes(lanes)
        steps_at, stale = self._steps_at, self._stale   # capture runs nothing: the outputs' validity is unchanged
        graphs = self._capture_ranges(lanes, lambda st, r: self.run(actions, n_steps, info=info, lanes=lanes,
                                                                    _only=r if lanes > 1 else None))
        self._steps_at, self._stale = steps_at, stale
        return WalkerGraph(self, graphs, actions, info=info)

    def observe(self):
        o = self._own_outputs(pad_clean=False, auto_reset=False)
        _lib.check(_lib.load().wg_observe(C.byref(self.batch.struct), C.byref(self._pstruct), C.byref(o),
                                          *self.batch.plan_args(), self._stream()), "wg_observe")
        self._steps_at = self.batch.version
        self._stale = frozenset()
        return self.obs, self.reward, self.done, self.info()

    def reset(self, noise=None, mask=None):
        """PhysicsEnv.reset: v += N(0, sigma) noise on x, y (and z if in3d); steps = 0; returns obs.
        ``noise`` [P, 3] overrides the device generator (use it for reproducible parity runs)."""
        if noise is None and self.sigma > 0:
            noise = torch.randn((self.batch.P, 3), generator=self._gen, device=self.device) * self.sigma
        if noise is not None:   # caller's mass order -> the stored order
            noise = self.batch.to_stored("mass", torch.as_tensor(noise, dtype=torch.float32).to(self.device)
                                         .reshape(self.batch.P, 3)).contiguous()
        if mask is not None:
            mask = self.batch.to_stored("walker", torch.as_tensor(mask).to(self.device, torch.uint8)).contiguous()
        _lib.check(_lib.load().wg_reset(
            C.byref(self.batch.struct), C.byref(self._pstruct),
            _lib.ptr(noise), _lib.ptr(mask), self._stream()), "wg_reset")
        return self.observe()[0]

    def seed(self, seed: Optional[int] = None) -> Sequence[int]:
        if seed is not None:
            self._gen.manual_seed(int(seed))
        return [seed] if seed is not None else []

    def info(self) -> dict:
        if self.steps_out is not None and self._steps_at == self.batch.version:
            steps = self.steps_out                 # written by the last step / observe in caller order
        else:
            steps = self.batch.caller("steps")     # a gather (after a rollout, a reset mask, or loaded state)
        info = {"steps": steps, "centroid_position": self.centroid, "total_energy": self.energy}
        if self._extras:
            info["momentum"] = self.momentum      # Point.momentum (gym/engine.py:160-166) of each walker
            info["nonfinite"] = self.nonfinite    # True: the walker's pos / vel / acc hold an inf or NaN
        if self._ar_mode:                         # auto-reset: the last step's resets, the resets taken so far
            info["reset"] = self.reset_out
            info["episodes"] = self.batch.episodes
            if self.final_obs is not None:
                info["final_obs"] = self.final_obs
        for k in self._stale:                     # not written by the last run() (record buffers, info=False)
            info.pop(k, None)
        return info

    # state accessors in the caller's order.  An unpermuted batch returns live views into its tensors; a ragged batch
    # (stored in wave-tile / size order) returns gathered COPIES, so in-place writes into them do not reach the batch:
    # assign instead (env.pos = t, env.vel[...] edits then env.vel = edited), which scatters into the stored order.
    def _set_state(self, name: str, value) -> None:
        self.batch.version += 1
        dst = getattr(self.batch, name)
        t = torch.as_tensor(value, dtype=dst.dtype).to(self.device).reshape(dst.shape)
        dst.copy_(self.batch.to_stored(self.batch.KIND[name], t))

    @property
    def pos(self):
        return self.batch.caller("pos")

    @pos.setter
    def pos(self, value):
        self._set_state("pos", value)

    @property
    def vel(self):
        return self.batch.caller("vel")

    @vel.setter
    def vel(self, value):
        self._set_state("vel", value)

    @property
    def acc(self):
        return self.batch.caller("acc")

    @acc.setter
    def acc(self, value):
        self._set_state("acc", value)

    @property
    def muscle_x(self):
        return self.batch.caller("muscle_x")

    @muscle_x.setter
    def muscle_x(self, value):
        self._set_state("muscle_x", value)

    @property
    def contact(self):
        return self.batch.caller("contact")

    @property
    def steps(self):
        return self.batch.caller("steps")

    def get_action_space(self) -> dict:
        return {"shape": (self.batch.A,), "type": "continuous", "low": -1.0, "high": 1.0}

    def get_observation_space(self) -> dict:
        return {"shape": (self.obs_dim,), "type": "continuous", "low": -np.inf, "high": np.inf}

    def launch_geometry(self) -> dict:
        return self.batch.launch_geometry()

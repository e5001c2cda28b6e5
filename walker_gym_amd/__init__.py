"""walker_gym_amd — MI355X-native batched walker physics stepper (the hot path of bluemoon-o2/walker-gym).

Product path: BatchedPhysicsEnv (walker_gym_amd.batched_env) over libwalker_hip.so (C ABI in
include/walker_hip.h, HIP kernels for gfx950).  Drop-in facades of the reference API:
  walker_gym_amd.engine        Point, Config, to_data, DingPoint            (gym/engine.py)
  walker_gym_amd.walker        Muscle, Skeleton, Creature, create_*_creature (gym/optimized_walker.py)
  walker_gym_amd.optimized_env PhysicsEnv, make_env, Environment            (gym/optimized_env.py)
  walker_gym_amd.env           Environment (G1 step(t) API)                  (gym/env.py)
  walker_gym_amd.snapshot      state.pkl read/write without unpickling       (gym/engine.py:199-212)
Training on the device: walker_gym_amd.policy.MLPPolicy (evaluated inside the rollout kernels) and
walker_gym_amd.es.EvolutionStrategy (seeded perturb / update kernels, wg_es_* in the header);
BatchedPhysicsEnv.rollout_stochastic and walker_gym_amd.pg (seeded action noise in the rollout kernel, the GAE kernel,
collect() for PPO: wg_rollout_stochastic / wg_gae; policy_rows(), the MLPPolicy over recorded rows as a
torch.autograd.Function: wg_policy_forward / wg_policy_backward); walker_gym_amd.normalize.ObsNorm, running observation
statistics on the device (wg_obs_moments) and the normaliser MLPPolicy(obs_norm=...) evaluates in every kernel
(wg_rollout_normalized, wg_policy_forward_normalized / wg_policy_backward_normalized); BatchedPhysicsEnv.rollout_held,
the resident closed loop with an action hold (decide every k steps: wg_rollout_held), and pg.gae_held on its decision
grid (wg_gae_held); MLPPolicy(wm=..., bm=...), a second hidden layer in the rollouts and the row kernels (wg_rollout_deep,
wg_policy_forward_deep / wg_policy_backward_deep); pg.expf, the library's own pinned exponential (wg_expf), and
pg.log_prob_rows / pg.ppo_surrogate, the Gaussian density and the clipped PPO surrogate with its gradients in one kernel
call (wg_ppo_surrogate); walker_gym_amd.optim.Adam, a global-norm clip and Adam / AdamW over float32 device tensors in
one call and in pinned arithmetic (wg_adam_step; adam_step_numpy restates it), EvolutionStrategy(optimizer="adam") on
top of it, and pg.normalize_advantages (the masked mean and scale from wg_obs_moments' ordered sums).
Importing the package needs no GPU; stepping does (no CPU fallback).
"""
from .engine import Config, DingPoint, Point, to_data  # noqa: F401
from .walker import (Creature, Muscle, Skeleton, balance_spec, box_spec, create_balance_creature,  # noqa: F401
                     create_box_creature, creatures_to_spec)

__version__ = "0.1.0"


def __getattr__(name):
    # torch-dependent modules load lazily so `import walker_gym_amd` stays light
    if name in ("BatchedPhysicsEnv", "EnvParams"):
        from . import batched_env
        return getattr(batched_env, name)
    if name == "MLPPolicy":
        from . import policy
        return policy.MLPPolicy
    if name in ("EvolutionStrategy", "AdaptiveEvolutionStrategy"):   # the latter: one adapted sigma per parameter (PGPE)
        from . import es
        return getattr(es, name)
    if name == "pg":   # policy-gradient support: the noise and GAE restatements, gae(), collect()
        import importlib
        return importlib.import_module(".pg", __name__)
    if name == "policy_rows":   # pg.policy_rows(policy, obs, mask=None, chunk_rows=None): differentiable in-kernel policy
        import importlib
        return importlib.import_module(".pg", __name__).policy_rows
    if name == "normalize":   # observation normalisation: ObsNorm (wg_obs_moments) and the numpy restatements
        import importlib
        return importlib.import_module(".normalize", __name__)
    if name == "ObsNorm":
        import importlib
        return importlib.import_module(".normalize", __name__).ObsNorm
    if name == "rollout_stochastic":   # BatchedPhysicsEnv.rollout_stochastic(env, policy, n_steps, sigma, seed, ...)
        from . import batched_env
        return batched_env.BatchedPhysicsEnv.rollout_stochastic
    if name == "rollout_held":   # BatchedPhysicsEnv.rollout_held(env, policy, n_steps, every, sigma=None, ...): action hold
        from . import batched_env
        return batched_env.BatchedPhysicsEnv.rollout_held
    if name in ("gae_held", "gae_held_numpy", "hold_decide_numpy"):   # pg's GAE on the hold's decision grid
        import importlib
        return getattr(importlib.import_module(".pg", __name__), name)
    if name in ("expf", "expf_numpy", "log_prob_rows", "ppo_surrogate", "ppo_surrogate_numpy"):
        # pg's pinned exponential (wg_expf) and the fused clipped surrogate over recorded rows (wg_ppo_surrogate)
        import importlib
        return getattr(importlib.import_module(".pg", __name__), name)
    if name in ("normalize_advantages", "normalize_advantages_numpy"):   # pg's masked advantage normalisation
        import importlib
        return getattr(importlib.import_module(".pg", __name__), name)
    if name == "optim":   # the device optimiser: Adam (wg_adam_step) and its numpy restatement
        import importlib
        return importlib.import_module(".optim", __name__)
    if name in ("Adam", "adam_step_numpy"):
        import importlib
        return getattr(importlib.import_module(".optim", __name__), name)
    if name in ("PhysicsEnv", "make_env"):
        from . import optimized_env
        return getattr(optimized_env, name)
    raise AttributeError(name)

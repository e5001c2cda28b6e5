"""What the evolution-strategies tests share (tests/test_es_cpu.py without a GPU, tests/test_gpu_es.py on one).

The trainer cases run Balance-v0 x 128 built by tests/policy_cases.py's `balance` recipe (per-walker start velocities
and step counters, max_steps = 16, T = 20 steps, the G1 getstat rows: D = 26, so K = 54 without a hidden layer and 147
with H = 5).  The start weights and sigma follow policy_cases' scales (the rows hold accelerations in the thousands), so
that the clip engages on some outputs and every walker stays finite: test_es_cpu.py checks that with the reference
engine before the GPU test compares bits."""
import functools

import numpy as np

import policy_cases as pc

N_WALKERS, T, GENERATIONS = 128, 20, 3
PARAMS = dict(pc.BAL, midform=2)
D, C = 26, 2
SEED = (7 << 32) + 12345          # above 2^32: both key words in use
TRAINER_CASES = [(0, 128), (0, 16), (5, 128), (5, 16)]          # (H, G)
SIGMA = {0: 0.0005, 5: 0.002}
LR = {0: 2e-5, 5: 1e-4}


@functools.lru_cache(maxsize=None)
def balance128():
    from walker_gym_amd.walker import balance_spec
    spec = dict(balance_spec(N_WALKERS))
    rng = np.random.default_rng(5)
    vel = np.array(spec["vel"], np.float32).reshape(-1, 3).copy()
    vel[:, :2] += rng.uniform(-3, 3, (vel.shape[0], 2)).astype(np.float32)
    spec["vel"] = vel
    spec["steps"] = (np.arange(N_WALKERS) % 7).astype(np.int32)
    return spec


def theta0(H):
    from walker_gym_amd.es import param_count
    rng = np.random.default_rng(40 + H)
    K = param_count(D, H, C, True)
    if not H:
        return (rng.standard_normal(K) * 0.0005).astype(np.float32)
    t = (rng.standard_normal(K) * pc.SCALE_MLP).astype(np.float32)
    t[D * H + H:D * H + H + H * C] *= np.float32(4.0)            # w2 of a hidden layer: four times w1's scale
    return t


def numpy_policy(theta, sigma, generation, H, G, device=None):
    """The generation's candidates by es_perturb_numpy, as an MLPPolicy (on `device`, or on the host)."""
    import torch
    from walker_gym_amd.es import es_perturb_numpy, split_theta
    from walker_gym_amd.policy import MLPPolicy
    seg = split_theta(es_perturb_numpy(theta, sigma, SEED, generation, 0, G // 2), D, H, C, True)
    mv = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device or "cpu")
    return MLPPolicy(mv(seg["w2"]), mv(seg["b2"]), mv(seg["w1"]), mv(seg["b1"]), act_limit=1.0)


def set_fitness(returns, G):
    """The float64 mean of each set's walkers' returns, rounded to float32."""
    r = np.asarray(returns, np.float32).astype(np.float64).reshape(G, -1)
    return (r.sum(axis=1) / r.shape[1]).astype(np.float32)


def numpy_tell(theta, fitness, generation, H, G):
    from walker_gym_amd.es import es_update_numpy, es_utilities_numpy
    sigma = float(np.float32(SIGMA[H]))
    scale = 1.0 / (2.0 * (G // 2) * sigma)
    return es_update_numpy(theta, es_utilities_numpy(fitness), SEED, generation, 0, G // 2, scale, np.float32(LR[H]))


@functools.lru_cache(maxsize=None)
def oracle_training(H, G):
    """GENERATIONS generations on the CPU reference engine, every one from the start state: per generation the
    rollout's obs / reward / action (for the finiteness check), the fitness, the gradient and theta afterwards."""
    from oracle.oracle import Oracle, nonfinite
    theta, gens = theta0(H), []
    for g in range(GENERATIONS):
        pol = numpy_policy(theta, np.float32(SIGMA[H]), g, H, G)
        orc = Oracle(balance128(), PARAMS, n_threads=8)
        obs = orc.observe()["obs"]
        rew, done, act, rows = [], [], [], []
        for t in range(T):
            a = pol.forward_numpy(obs)
            r = orc.step(a)
            obs = r["obs"]
            rows.append(obs.copy()); rew.append(r["reward"].copy()); done.append(r["done"].copy()); act.append(a)
        ret, _ = pc.returns_lengths(np.stack(rew), np.stack(done))
        fit = set_fitness(ret, G)
        grad, theta = numpy_tell(theta, fit, g, H, G)
        gens.append(dict(obs=np.stack(rows), reward=np.stack(rew), action=np.stack(act), done=np.stack(done),
                         fitness=fit, grad=grad, theta=theta.copy(),
                         nonfinite=int(nonfinite(orc.pos, orc.vel, orc.acc, orc.mass_off).sum())))
    return gens

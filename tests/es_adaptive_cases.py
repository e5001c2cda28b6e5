"""What the adaptive evolution-strategies tests share (tests/test_es_adaptive_cpu.py without a GPU,
tests/test_gpu_es_adaptive.py on one): the inputs of the update cases, the clamp cases, the quadratic run on the numpy
restatement, and the trainer cases, which are tests/es_cases.py's (Balance-v0 x 128, T = 20, D = 26, H in {0, 5},
G in {128, 16}, three generations) with one sigma per parameter.

The trainer cases' numbers.  es_cases.SIGMA[H] keeps every walker finite, so the start vector stays at or below 1.25
times it: sigma0[k] = SIGMA[H] * (0.5 + (k % 4) / 4).  PGPE's estimate of the mean is sigma^2 times the scalar
trainer's (d = sigma * eps is summed where the scalar trainer sums eps and divides by sigma), so the learning rate that
moves theta as far as es_cases.LR[H] does there is LR[H] / SIGMA[H]^2; sigma_lr and sigma_max_change are the class
defaults."""
import functools

import numpy as np

import es_cases as ec
import policy_cases as pc

f32 = np.float32
SEED = ec.SEED
LR_THETA = {H: ec.LR[H] / ec.SIGMA[H] ** 2 for H in ec.SIGMA}
SIGMA_LR, MAX_CHANGE, SIGMA_MIN, SIGMA_MAX = 0.1, 0.2, 1e-8, float("inf")
UPDATE_PAIRS = [1, 3, 256, 257, 600]
FIRST = 2                                   # every update case starts at pair 2: first_pair > 0
GEN = 3


def sigma0(H):
    from walker_gym_amd.es import param_count
    K = param_count(ec.D, H, ec.C, True)
    return (f32(ec.SIGMA[H]) * (f32(0.5) + (np.arange(K) % 4).astype(f32) / f32(4))).astype(f32)


def trainer_step(H, G):
    """AdaptiveEvolutionStrategy.step_fields() of a trainer case, restated."""
    from walker_gym_amd.es import diag_step
    n = G // 2
    return diag_step(base=0.0, scale_theta=1.0 / (2.0 * n), scale_sigma=1.0 / n, lr_theta=float(f32(LR_THETA[H])),
                     lr_sigma=float(f32(SIGMA_LR)), shrink=float(f32(1.0 - MAX_CHANGE)),
                     grow=float(f32(1.0 + MAX_CHANGE)), sigma_min=float(f32(SIGMA_MIN)), sigma_max=SIGMA_MAX)


def numpy_policy(theta, sigma_vec, generation, H, G, device=None):
    """The generation's candidates by es_perturb_diag_numpy, as an MLPPolicy (on `device`, or on the host)."""
    import torch
    from walker_gym_amd.es import es_perturb_diag_numpy, split_theta
    from walker_gym_amd.policy import MLPPolicy
    seg = split_theta(es_perturb_diag_numpy(theta, sigma_vec, SEED, generation, 0, G // 2), ec.D, H, ec.C, True)
    mv = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device or "cpu")
    return MLPPolicy(mv(seg["w2"]), mv(seg["b2"]), mv(seg["w1"]), mv(seg["b1"]), act_limit=1.0)


def numpy_tell(theta, sigma_vec, fitness, generation, H, G):
    """(g_theta, theta_out, g_sigma, sigma_out) of one generation."""
    from walker_gym_amd.es import es_update_diag_numpy, es_utilities_numpy
    return es_update_diag_numpy(theta, sigma_vec, es_utilities_numpy(fitness), SEED, generation, 0, G // 2,
                                trainer_step(H, G))


@functools.lru_cache(maxsize=None)
def oracle_training(H, G):
    """es_cases.oracle_training with the adaptive trainer's arithmetic: ec.GENERATIONS generations on the CPU reference
    engine, every one from the start state."""
    from oracle.oracle import Oracle, nonfinite
    theta, sigma, gens = ec.theta0(H), sigma0(H), []
    for g in range(ec.GENERATIONS):
        pol = numpy_policy(theta, sigma, g, H, G)
        orc = Oracle(ec.balance128(), ec.PARAMS, n_threads=8)
        obs = orc.observe()["obs"]
        rew, done, act, rows = [], [], [], []
        for t in range(ec.T):
            a = pol.forward_numpy(obs)
            r = orc.step(a)
            obs = r["obs"]
            rows.append(obs.copy()); rew.append(r["reward"].copy()); done.append(r["done"].copy()); act.append(a)
        ret, _ = pc.returns_lengths(np.stack(rew), np.stack(done))
        fit = ec.set_fitness(ret, G)
        g_theta, theta, g_sigma, sigma = numpy_tell(theta, sigma, fit, g, H, G)
        gens.append(dict(obs=np.stack(rows), reward=np.stack(rew), action=np.stack(act), fitness=fit, grad=g_theta,
                         grad_sigma=g_sigma, theta=theta.copy(), sigma=sigma.copy(),
                         nonfinite=int(nonfinite(orc.pos, orc.vel, orc.acc, orc.mass_off).sum())))
    return gens


# ------------------------------------------------------------------ the update cases
def update_step(n_pairs, **kw):
    from walker_gym_amd.es import diag_step
    d = dict(base=0.0625, scale_theta=1.0 / (2 * n_pairs), scale_sigma=1.0 / n_pairs, lr_theta=float(f32(0.3)),
             lr_sigma=float(f32(0.1)), shrink=float(f32(0.8)), grow=float(f32(1.2)), sigma_min=float(f32(1e-8)))
    d.update(kw)
    return diag_step(**d)


@functools.lru_cache(maxsize=None)
def update_inputs(K, n_pairs):
    """theta, a sigma spanning four decades (10^-3 .. 10), and the util vectors of the case: centred ranks, a vector
    with ties (pairs with dm = 0 among them), +inf in one member of a pair (dm = ds = +inf) and +inf in both members
    (dm = NaN, ds = +inf)."""
    from walker_gym_amd.es import es_utilities_numpy
    rng = np.random.default_rng(1000 * K + n_pairs)
    G = 2 * (FIRST + n_pairs)
    theta = (rng.standard_normal(K) * 0.3).astype(f32)
    sigma = (10.0 ** rng.uniform(-3, 1, K)).astype(f32)
    plain = es_utilities_numpy(rng.standard_normal(G).astype(f32))
    ties = (rng.integers(-3, 4, G) / 8).astype(f32)
    one, both = plain.copy(), plain.copy()
    one[2 * (FIRST + n_pairs // 2)] = np.inf
    both[2 * (FIRST + n_pairs // 2)] = both[2 * (FIRST + n_pairs // 2) + 1] = np.inf
    for a in (theta, sigma, plain, ties, one, both):
        a.setflags(write=False)
    return dict(G=G, theta=theta, sigma=sigma, utils=dict(plain=plain, ties=ties, inf_one=one, inf_both=both))


@functools.lru_cache(maxsize=None)
def update_reference(K, n_pairs, name):
    from walker_gym_amd.es import es_update_diag_numpy
    c = update_inputs(K, n_pairs)
    out = es_update_diag_numpy(c["theta"], c["sigma"], c["utils"][name], SEED, GEN, FIRST, n_pairs, update_step(n_pairs))
    for a in out:
        a.setflags(write=False)
    return out


def same_bits_nan_equal(a, b):
    """Equal shape and dtype, NaN in the same places, every other element equal in bits.  (A NaN that an operation
    creates, inf - inf, has no contracted sign or payload: processors differ.)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return np.array_equal(na, nb) and np.array_equal(a.view(u)[~na], b.view(u)[~nb])


# ------------------------------------------------------------------ the clamp cases
CLAMP_K, CLAMP_PAIRS = 147, 64
CLAMP_CASES = {
    # a step far larger than the allowed change: sigma[k] * shrink or sigma[k] * grow binds, or neither on a few
    "change": dict(lr_sigma=float(f32(40.0))),
    # sigma spans 10^-3 .. 10 and the bounds lie inside that range: sigma_min / sigma_max bind where the step passes them
    "bounds": dict(lr_sigma=float(f32(40.0)), sigma_min=float(f32(0.05)), sigma_max=float(f32(1.0))),
}


@functools.lru_cache(maxsize=None)
def clamp_reference(name):
    from walker_gym_amd.es import es_update_diag_numpy
    c = update_inputs(CLAMP_K, CLAMP_PAIRS)
    step = update_step(CLAMP_PAIRS, **CLAMP_CASES[name])
    out = es_update_diag_numpy(c["theta"], c["sigma"], c["utils"]["plain"], SEED, GEN, FIRST, CLAMP_PAIRS, step)
    for a in out:
        a.setflags(write=False)
    return step, out


def clamp_branches(sigma, g_sigma, step):
    """Which branch of the clamp each parameter takes, from the contract's formulas: 'shrink', 'sigma_min', 'grow',
    'sigma_max' or 'free'."""
    s = sigma + f32(step["lr_sigma"]) * g_sigma
    dn, up = sigma * f32(step["shrink"]), sigma * f32(step["grow"])
    lo_min, hi_max = ~(dn > f32(step["sigma_min"])), ~(up < f32(step["sigma_max"]))
    lo, hi = np.where(lo_min, f32(step["sigma_min"]), dn), np.where(hi_max, f32(step["sigma_max"]), up)
    out = np.full(sigma.shape, "free", dtype=object)
    out[(s < lo) & ~lo_min] = "shrink"
    out[(s < lo) & lo_min] = "sigma_min"
    out[~(s < lo) & (s > hi) & ~hi_max] = "grow"
    out[~(s < lo) & (s > hi) & hi_max] = "sigma_max"
    return out


# ------------------------------------------------------------------ the quadratic
QUAD_K, QUAD_G, QUAD_GENERATIONS, QUAD_SEEDS = 54, 64, 30, (1, 2, 3)
# lr: test_quadratic_descends_on_the_device (sigma 0.1, lr 0.2) moves theta by 0.2 / (2 n 0.1) * sum dm eps =
# (1 / n) * sum dm eps; PGPE moves it by lr / (2 n) * sum dm sigma eps, the same step at sigma0 = 1 with lr = 2
QUAD = dict(sigma=1.0, lr=2.0)


def quadratic_step():
    from walker_gym_amd.es import diag_step
    n = QUAD_G // 2
    return diag_step(base=0.0, scale_theta=1.0 / (2.0 * n), scale_sigma=1.0 / n, lr_theta=float(f32(QUAD["lr"])),
                     lr_sigma=float(f32(SIGMA_LR)), shrink=float(f32(1.0 - MAX_CHANGE)),
                     grow=float(f32(1.0 + MAX_CHANGE)), sigma_min=float(f32(SIGMA_MIN)), sigma_max=SIGMA_MAX)


@functools.lru_cache(maxsize=None)
def quadratic_numpy(seed):
    """The quadratic of tests/test_gpu_es.py (fitness -|candidate - target|^2 summed in float32 in element order) by
    the restatements alone: (target, theta, sigma_vec, loss0, loss)."""
    from walker_gym_amd import es
    target = np.random.default_rng(seed).standard_normal(QUAD_K).astype(f32)
    theta, sigma = np.zeros(QUAD_K, f32), np.full(QUAD_K, QUAD["sigma"], f32)
    loss0 = float(((theta - target).astype(np.float64) ** 2).sum())
    for gen in range(QUAD_GENERATIONS):
        cand = es.es_perturb_diag_numpy(theta, sigma, seed, gen, 0, QUAD_G // 2)
        fit = quadratic_fitness(cand, target)
        _, theta, _, sigma = es.es_update_diag_numpy(theta, sigma, es.es_utilities_numpy(fit), seed, gen, 0,
                                                     QUAD_G // 2, quadratic_step())
    return target, theta, sigma, loss0, float(((theta - target).astype(np.float64) ** 2).sum())


def quadratic_fitness(cand, target):
    """-sum_k (cand - target)^2 in float32, added in element order (a reduction whose order both numpy and a device
    loop can follow: the ranks must agree in every tie-free case)."""
    sq = (cand - target[None]) ** 2
    acc = np.zeros(cand.shape[0], f32)
    for k in range(cand.shape[1]):
        acc = acc + sq[:, k]
    return -acc

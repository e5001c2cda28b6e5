"""What the deep evolution-strategies tests share (tests/test_es_deep_cpu.py without a GPU, tests/test_gpu_es_deep.py on
one): the shapes of the six-segment theta at which wg_es_perturb_deep / wg_es_perturb_diag_deep can go wrong, and the
trainer cases.  No GPU import.

Shapes are (D, H1, H2, C, b1, bm, b2); theta's segments are w1, b1, wm, bm, w2, b2 and an absent bias takes no slot.
The perturb kernels have two forms: K < 256 puts 256 // K whole pairs into a row of 256 threads, K >= 256 one pair per row
and a block of 256 values of k per workgroup.  The asserts below keep the list at the edges the kernels have.

The trainer cases are tests/es_cases.py's recipe (Balance-v0 x 128, T = 20, max_steps = 16, D = 26, C = 2, G in {128, 16},
three generations) with (H1, H2) = (5, 3): K = 161.  The start weights are drawn at es_cases' scales and then shifted
layer by layer as tests/deep_cases.py does (its _balance_layer, one set over the 128 walkers), so that under the mean
theta every unit of both hidden layers is on for some walker and off for another at step 0.
tests/test_es_deep_cpu.py checks that, and that every generation stays finite with some actions clipped, on the
reference engine before the GPU test compares bits."""
import functools

import numpy as np

import es_cases as ec
import policy_cases as pc

f32 = np.float32
SEED = ec.SEED                     # above 2^32

SHAPES = [
    (6, 3, 2, 2, True, True, True),          # K = 35: seven pairs per row
    (6, 3, 2, 2, True, False, True),         # K = 33: bm absent alone (a zero-length segment inside the chain)
    (26, 5, 3, 2, True, True, True),         # K = 161: one pair per row of the row form
    (26, 5, 3, 2, False, True, True),        # K = 156: b1 absent alone
    (152, 23, 17, 5, True, True, True),      # K = 4,017: the block form, no boundary on a multiple of 64
    (152, 23, 17, 5, True, False, True),     # K = 4,000: bm absent alone in the block form
    (152, 23, 17, 5, False, False, False),   # K = 3,972: no bias at all
]


def shape_id(s):
    return "D%d-H%dx%d-C%d-%s" % (s[0], s[1], s[2], s[3], "".join("b" if b else "n" for b in s[4:]))


def counts(shape):
    """The six segments' element counts in theta's order (0 for an absent bias)."""
    D, H1, H2, C, b1, bm, b2 = shape
    return [D * H1, H1 if b1 else 0, H1 * H2, H2 if bm else 0, H2 * C, C if b2 else 0]


def K_of(shape):
    return sum(counts(shape))


def boundaries(shape):
    """The five interior segment boundaries, as offsets in theta."""
    return list(np.cumsum(counts(shape))[:-1])


def _check_shapes():
    Ks = [K_of(s) for s in SHAPES]
    assert Ks == [35, 33, 161, 156, 4017, 4000, 3972], Ks
    assert any(K < 256 and 256 // K > 1 for K in Ks)                     # the row form with several pairs per row
    assert any(128 <= K < 256 for K in Ks)                               # the row form, one pair per row
    full = SHAPES[4]
    assert K_of(full) >= 256 and all(b % 64 for b in boundaries(full))   # the block form, every boundary inside a wave
    edges = [0] + boundaries(full) + [K_of(full)]
    assert any(sum(1 for a, b in zip(edges[:-1], edges[1:]) if b > lo and a < lo + 256 and b > a) >= 3
               for lo in range(0, K_of(full), 256))                      # a block of 256 that holds three segments
    bias = {s[4:] for s in SHAPES}
    assert (True, False, True) in bias and (False, True, True) in bias and (False, False, False) in bias


_check_shapes()


# ------------------------------------------------------------------ the trainer cases
D, C, H1, H2 = ec.D, ec.C, 5, 3
N_WALKERS, T, GENERATIONS, PARAMS = ec.N_WALKERS, ec.T, ec.GENERATIONS, ec.PARAMS
K = D * H1 + H1 + H1 * H2 + H2 + H2 * C + C
TRAINER_G = [128, 16]
SCALE_W1, SCALE_WM, SCALE_W2 = pc.SCALE_MLP, 0.25, 0.25
SIGMA, LR = 0.002, 1e-4                       # es_cases' for H = 5
LR_THETA = LR / SIGMA ** 2                    # es_adaptive_cases' rule for the PGPE trainer
SIGMA_LR, MAX_CHANGE, SIGMA_MIN, SIGMA_MAX = 0.1, 0.2, 1e-8, float("inf")
assert K == 161


@functools.lru_cache(maxsize=None)
def entry_rows():
    """The observation rows of es_cases.balance128() at entry (reference engine)."""
    from oracle.oracle import Oracle
    rows = Oracle(ec.balance128(), PARAMS, n_threads=8).observe()["obs"].copy()
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def _theta0():
    import deep_cases as dc
    rng = np.random.default_rng(45)
    w1 = (rng.standard_normal((1, D, H1)) * SCALE_W1).astype(f32)
    b1 = (rng.standard_normal((1, H1)) * SCALE_W1).astype(f32)
    wm = (rng.standard_normal((1, H1, H2)) * SCALE_WM).astype(f32)
    bm = (rng.standard_normal((1, H2)) * SCALE_W1).astype(f32)
    w2 = (rng.standard_normal((1, H2, C)) * SCALE_W2).astype(f32)
    b2 = (rng.standard_normal((1, C)) * SCALE_W1).astype(f32)
    x = entry_rows().astype(np.float64)
    w1, b1 = dc._balance_layer(x, w1, b1, 1)
    h1 = np.maximum(dc._layer64(x, w1, b1, 1), 0.0)
    wm, bm = dc._balance_layer(h1, wm, bm, 1)
    t = np.concatenate([a.reshape(-1) for a in (w1, b1, wm, bm, w2, b2)]).astype(f32)
    t.setflags(write=False)
    return t


def theta0():
    return _theta0().copy()


def sigma0():
    return (f32(SIGMA) * (f32(0.5) + (np.arange(K) % 4).astype(f32) / f32(4))).astype(f32)


def trainer_step(G):
    """AdaptiveEvolutionStrategy.step_fields() of a trainer case, restated."""
    from walker_gym_amd.es import diag_step
    n = G // 2
    return diag_step(base=0.0, scale_theta=1.0 / (2.0 * n), scale_sigma=1.0 / n, lr_theta=float(f32(LR_THETA)),
                     lr_sigma=float(f32(SIGMA_LR)), shrink=float(f32(1.0 - MAX_CHANGE)),
                     grow=float(f32(1.0 + MAX_CHANGE)), sigma_min=float(f32(SIGMA_MIN)), sigma_max=SIGMA_MAX)


def policy_of_flat(flat, device=None, obs_norm=None):
    """Flat candidates [G, K] (or theta [K]) as a deep MLPPolicy."""
    import torch
    from walker_gym_amd.es import split_theta
    from walker_gym_amd.policy import MLPPolicy
    seg = split_theta(np.atleast_2d(flat), D, H1, C, True, H2)
    mv = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device or "cpu")
    return MLPPolicy(mv(seg["w2"]), mv(seg["b2"]), mv(seg["w1"]), mv(seg["b1"]), act_limit=1.0, obs_norm=obs_norm,
                     wm=mv(seg["wm"]), bm=mv(seg["bm"]))


def numpy_policy(theta, sigma, generation, G, device=None, obs_norm=None):
    """The generation's candidates by es_perturb_numpy (a scalar sigma) or es_perturb_diag_numpy (a [K] vector)."""
    from walker_gym_amd.es import es_perturb_diag_numpy, es_perturb_numpy
    f = es_perturb_diag_numpy if np.ndim(sigma) else es_perturb_numpy
    return policy_of_flat(f(theta, sigma, SEED, generation, 0, G // 2), device, obs_norm)


def numpy_tell(theta, sigma, fitness, generation, G):
    """One generation's update: (grad, theta) for a scalar sigma, (g_theta, theta, g_sigma, sigma) for a vector."""
    from walker_gym_amd.es import es_update_diag_numpy, es_update_numpy, es_utilities_numpy
    util = es_utilities_numpy(fitness)
    if np.ndim(sigma):
        return es_update_diag_numpy(theta, sigma, util, SEED, generation, 0, G // 2, trainer_step(G))
    s = float(f32(sigma))
    return es_update_numpy(theta, util, SEED, generation, 0, G // 2, 1.0 / (2.0 * (G // 2) * s), f32(LR))


@functools.lru_cache(maxsize=None)
def oracle_training(G, adaptive):
    """GENERATIONS generations on the CPU reference engine, every one from the start state (es_cases.oracle_training
    with the deep policy): per generation the rollout's arrays, step 0's hidden vectors under the mean theta, the
    fitness, and theta (and sigma) afterwards."""
    import deep_cases as dc
    from oracle.oracle import Oracle, nonfinite
    from walker_gym_amd.es import split_theta
    theta, sigma, gens = theta0(), (sigma0() if adaptive else f32(SIGMA)), []
    for g in range(GENERATIONS):
        seg = split_theta(theta[None], D, H1, C, True, H2)
        h1, h2 = dc.hidden_of(seg, entry_rows(), 1)
        pol = numpy_policy(theta, sigma, g, G)
        orc = Oracle(ec.balance128(), PARAMS, n_threads=8)
        obs = orc.observe()["obs"]
        rew, done, act, rows = [], [], [], []
        for t in range(T):
            a = pol.forward_numpy(obs)
            r = orc.step(a)
            obs = r["obs"]
            rows.append(obs.copy()); rew.append(r["reward"].copy()); done.append(r["done"].copy()); act.append(a)
        ret, _ = pc.returns_lengths(np.stack(rew), np.stack(done))
        fit = ec.set_fitness(ret, G)
        out = numpy_tell(theta, sigma, fit, g, G)
        if adaptive:
            grad, theta, g_sigma, sigma = out
        else:
            grad, theta = out
        gens.append(dict(obs=np.stack(rows), reward=np.stack(rew), action=np.stack(act), done=np.stack(done), h1=h1, h2=h2,
                         fitness=fit, grad=grad, theta=theta.copy(), sigma=np.array(sigma, f32),
                         nonfinite=int(nonfinite(orc.pos, orc.vel, orc.acc, orc.mass_off).sum())))
    return gens

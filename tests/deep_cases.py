"""The deep policies (MLPPolicy with a second hidden layer: wg_policy_mid) that tests/test_deep_policy_cpu.py checks on
the CPU and tests/test_gpu_deep_rollout.py / tests/test_gpu_deep_rows.py compare bit for bit on the GPU.  No GPU import.

The batches are tests/policy_cases.py's, one per wave tile of the resident kernel, each the smallest that gives the tile:
  m4   `ne1` (N = 8192, M = 4, 16 walkers per wave), 2-D: D = 26 (D mod 4 = 2), A = 2
  m16  canonical4 (N = 2050, M = 16, 4 per wave, a partial last tile) with conmid: D = 155 (D mod 4 = 3), A = 8
  m64  wide (N = 6, M = 64, one per wave): D = 596, A = 20
  six  N = 4096 of M = 4, A = 6 (8 per wave): C = 5, 6 > M (the output loop goes round twice)
T = 3, L = inf (no clip hides a wrong pre-activation).

(H1, H2) per tile.  H2 takes 1, M - 1, M, M + 1, 2M + 1 and 256: lane q of a walker's M takes units q, q + M, ... of H2
two at a time (a lane with one unit, a single beside a pair, a lane that ends on an odd unit after a full pair, the
widest).  H1 mod 4 is 2 or 3: policy_unit2 walks the H1 vector four at a time and these leave its tail.  H2 < 8 and
H2 mod 8 != 0: the output layer's policy_unit walks the H2 vector eight at a time.  The benchmark widths (32, 32) and
(64, 64) on m16 beside them.  G: 1; a set boundary inside a wave tile (m4: 1024 sets of 8 walkers, m16: 5 sets of 410);
N at small widths.  Both biases (and b2) absent on the even seeds.

Weights: drawn as policy_cases draws them; w1 then wm are shifted (policy_cases._balance's idea, applied layer by layer)
so that at step 0 every unit of both hidden layers is on for some walker and off for another: a unit that is dead
everywhere hides its column.
"""
import functools

import numpy as np

import policy_cases as pc

f32 = np.float32
TILES = {"m4": ("ne1", dict(in3d=0), 16, "m4-h3-c2-g1"), "m16": ("canonical4", dict(in3d=1, conmid=1), 4, "m16-h16-c8-g1"),
         "m64": ("wide", dict(in3d=1), 1, "m64-h64-c20-g1"), "six": ("six", dict(in3d=1), 8, "six-h0-c6-g1")}
MASSES = {"m4": 4, "m16": 16, "m64": 64, "six": 4}


class DeepCase:
    def __init__(self, tile, H1, H2, C, G, seed, scale, T=3):
        self.tile, self.H1, self.H2, self.C, self.G, self.seed, self.scale, self.T = tile, H1, H2, C, G, seed, scale, T
        self.kind, self.params, self.wpw, self.rows_of = TILES[tile]
        self.L = float("inf")
        self.name = f"{tile}-h{H1}x{H2}-c{C}-g{G}"

    def __repr__(self):
        return self.name


# (the scales: policy_cases' for the tile and width; the middle matrix and w2 take four times the scale, as w2 does there)
CASES = [
    DeepCase("m4", 6, 1, 2, 8192, 201, 0.02),
    DeepCase("m4", 7, 3, 2, 1, 202, 0.02),
    DeepCase("m4", 6, 4, 1, 1024, 203, 0.02),
    DeepCase("m4", 7, 5, 2, 8192, 204, 0.02),
    DeepCase("m4", 6, 9, 2, 1, 205, 0.02),
    DeepCase("m4", 7, 256, 2, 1, 206, 0.012),
    DeepCase("m16", 18, 1, 8, 2050, 211, 0.016),
    DeepCase("m16", 19, 15, 5, 5, 212, 0.016),
    DeepCase("m16", 22, 16, 8, 1, 213, 0.016),
    DeepCase("m16", 23, 17, 8, 2050, 214, 0.016),
    DeepCase("m16", 34, 33, 8, 5, 215, 0.016),
    DeepCase("m16", 30, 256, 8, 1, 216, 0.008),
    DeepCase("m16", 32, 32, 8, 1, 217, 0.016),
    DeepCase("m16", 64, 64, 8, 1, 218, 0.012),
    DeepCase("m64", 2, 1, 20, 6, 221, 0.02),
    DeepCase("m64", 2, 1, 20, 1, 227, 0.02),      # (shared: the one M = 64 policy small enough to be staged in LDS)
    DeepCase("m64", 66, 63, 7, 3, 222, 0.012),
    DeepCase("m64", 67, 64, 20, 1, 223, 0.012),
    DeepCase("m64", 70, 65, 20, 2, 224, 0.012),
    DeepCase("m64", 66, 129, 20, 3, 225, 0.008),
    DeepCase("m64", 67, 256, 20, 1, 226, 0.008),
    DeepCase("six", 7, 5, 6, 1024, 231, 0.02),
    DeepCase("six", 6, 9, 5, 4096, 232, 0.02),
]


def case_of(name):
    return next(c for c in CASES if c.name == name)


def obs_dim(case):
    return pc.obs_dim(pc.case_of(case.rows_of))


def entry_rows(case):
    """The observation rows of the case's entry state (policy_cases' own, shared with its cases of the same batch)."""
    return pc.entry_rows(case.rows_of)


def _layer64(x, w, b, G):
    """A layer's pre-activations in float64, set by set (a set's walkers are contiguous)."""
    wps = x.shape[0] // G
    z = np.empty((x.shape[0], w.shape[2]), np.float64)
    for g in range(G):
        z[g * wps:(g + 1) * wps] = x[g * wps:(g + 1) * wps] @ w[g].astype(np.float64) + \
            (0.0 if b is None else b[g].astype(np.float64))
    return z


def _balance_layer(x, w, b, G):
    """policy_cases._balance on any layer: x [N, I] float64 (the layer's step-0 inputs), w [G, I, J], b [G, J] or None.
    Each set's columns are shifted along the mean input row of the set's walkers so that the median walker's
    pre-activation is zero; a set of one walker has its columns (and bias) negated for the signs to alternate."""
    N, wps = x.shape[0], x.shape[0] // G
    J = w.shape[2]
    for g in range(G):
        xs = x[g * wps:(g + 1) * wps]
        z = xs @ w[g].astype(np.float64) + (0.0 if b is None else b[g].astype(np.float64))
        if wps == 1:
            flip = (z[0] > 0) != ((g + np.arange(J)) % 2 == 0)
            w[g][:, flip] *= -1
            if b is not None:
                b[g][flip] *= -1
        else:
            mean = xs.mean(0)
            along = xs @ mean
            use = along > 1e-12 * max(along.max(), 1e-300)   # (a walker whose inputs are all zero has no say)
            alpha = np.median(z[use] / along[use, None], axis=0)
            w[g] = (w[g] - np.outer(mean, alpha)).astype(f32)
    return w, b


@functools.lru_cache(maxsize=None)
def _weights(case):
    rng = np.random.default_rng(3000 + case.seed)
    D, H1, H2, C, G, s = obs_dim(case), case.H1, case.H2, case.C, case.G, case.scale
    odd = bool(case.seed % 2)
    w1 = (rng.standard_normal((G, D, H1)) * s).astype(f32)
    b1 = (rng.standard_normal((G, H1)) * s).astype(f32) if odd else None
    wm = (rng.standard_normal((G, H1, H2)) * (4.0 * s)).astype(f32)
    bm = (rng.standard_normal((G, H2)) * s).astype(f32) if odd else None
    w2 = (rng.standard_normal((G, H2, C)) * (4.0 * s)).astype(f32)
    b2 = (rng.standard_normal((G, C)) * s).astype(f32) if odd else None
    x = entry_rows(case).astype(np.float64)
    w1, b1 = _balance_layer(x, w1, b1, G)
    h1 = np.maximum(_layer64(x, w1, b1, G), 0.0)
    wm, bm = _balance_layer(h1, wm, bm, G)
    return dict(w1=w1, b1=b1, wm=wm, bm=bm, w2=w2, b2=b2)


def weights(case):
    """The case's tensors as numpy float32 arrays (the caller's own copies): w1, b1, wm, bm, w2, b2."""
    return {k: None if a is None else a.copy() for k, a in _weights(case).items()}


def policy_from(w, device=None, act_limit=float("inf"), obs_norm=None):
    import torch
    from walker_gym_amd.policy import MLPPolicy
    mv = lambda a: None if a is None else (torch.from_numpy(a) if device is None else torch.from_numpy(a).to(device))
    return MLPPolicy(mv(w["w2"]), mv(w["b2"]), mv(w["w1"]), mv(w["b1"]), act_limit=act_limit, obs_norm=obs_norm,
                     wm=mv(w["wm"]), bm=mv(w["bm"]))


def policy_of(case, device=None):
    return policy_from(weights(case), device, case.L)


def hidden0(case):
    """Step 0's two hidden vectors, the contract restated in float32: (h1 [N, H1], h2 [N, H2])."""
    return hidden_of(_weights(case), entry_rows(case), case.G)


def hidden_of(w, x, G):
    """The two hidden vectors of the rows x [N, D] under the tensors w, G sets over the N walkers."""
    sets = np.arange(x.shape[0]) // (x.shape[0] // G)

    def layer(v, wt, b):
        z = np.zeros((v.shape[0], wt.shape[2]), f32) if b is None else b[sets].copy()
        for i in range(v.shape[1]):
            z = z + v[:, i:i + 1] * wt[sets, i]
        return np.where(z > 0, z, f32(0.0)).astype(f32)

    with np.errstate(all="ignore"):
        h1 = layer(x, w["w1"], w["b1"])
        return h1, layer(h1, w["wm"], w["bm"])


def oracle_loop(spec, params, policy, T, first=None):
    """The closed loop on the CPU reference engine: Oracle.step(policy.forward_numpy(obs)), step 0 on the entry state's
    observation.  Every step's obs / reward / done / action and the final state, read-only numpy arrays."""
    from oracle.oracle import Oracle
    orc = Oracle(spec, params, n_threads=8)
    obs = orc.observe()["obs"]
    out = dict(obs=[], reward=[], done=[], action=[])
    for t in range(T):
        a = policy.forward_numpy(obs)
        r = orc.step(a)
        obs = r["obs"]
        out["obs"].append(obs.copy()); out["reward"].append(r["reward"].copy())
        out["done"].append(r["done"].copy()); out["action"].append(a)
    res = {k: np.stack(v) for k, v in out.items()}
    res.update(pos=orc.pos.copy(), vel=orc.vel.copy(), acc=orc.acc.copy(), muscle_x=orc.mx.copy(),
               steps=orc.steps.copy(), contact=orc.contact.copy(), mass_off=orc.mass_off.copy())
    for v in res.values():
        v.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def oracle_rollout(name):
    """oracle_loop of a case (computed once, shared, never modified)."""
    case = case_of(name)
    return oracle_loop(pc.spec_of(case.kind), case.params, policy_of(case), case.T)


def lds_bytes(case, episodes=False):
    """The host's LDS arithmetic of wg_rollout_deep restated (policy_cases.lds_bytes with the hold's word and the second
    hidden vector in the slice, and the middle matrix among the weights): the workgroup's bytes without staged weights,
    the weights' bytes, and whether WG_POLICY_STAGE = 0 / 1 / 2 stages them."""
    spec = pc.spec_of(case.kind)
    N, K = len(spec["mass_off"]) - 1, int(spec["edge_off"][1] - spec["edge_off"][0])
    A, D, w = int(np.asarray(spec["n_muscles"])[0]), obs_dim(case), case.wpw
    a16 = lambda n: (n + 15) & ~15
    ew = w * K
    pl = (ew + 3) & ~3
    sl = a16(pl * 24) + a16(pl * 12) + a16(ew * 4 + 4) + a16(max(1, w * A) * 4)
    sl += a16(w * D * 4) + a16(w * case.H1 * 4) + a16(w * case.C * 4) + w * (32 if episodes else 16)
    sl += a16(w * 4) + a16(w * case.H2 * 4)
    wpb = 1 if (N + w - 1) // w <= 1024 else 4
    lds, wts = wpb * sl, 4 * (D * case.H1 + case.H1 * case.H2 + case.H2 * case.C)
    cap = max(1, (12 if (ew + 63) // 64 > 4 else 16) // wpb)
    free = min(cap, 160 * 1024 // lds) == min(cap, 160 * 1024 // (lds + wts))
    fits = case.G == 1 and lds + wts <= 80 * 1024
    return dict(lds=lds, weights=wts, staged={0: False, 1: fits and free, 2: fits})


def identity_pair(D, H, C, G, seed, scale, bias=True):
    """A shallow policy's tensors and its deep twin's (H2 = H1 = H, wm = I, no bm): (shallow dict, deep dict)."""
    rng = np.random.default_rng(seed)
    w1 = (rng.standard_normal((G, D, H)) * scale).astype(f32)
    b1 = (rng.standard_normal((G, H)) * scale).astype(f32) if bias else None
    w2 = (rng.standard_normal((G, H, C)) * (4.0 * scale)).astype(f32)
    b2 = (rng.standard_normal((G, C)) * scale).astype(f32) if bias else None
    wm = np.broadcast_to(np.eye(H, dtype=f32), (G, H, H)).copy()
    return dict(w1=w1, b1=b1, w2=w2, b2=b2), dict(w1=w1, b1=b1, wm=wm, bm=None, w2=w2, b2=b2)


def shallow_from(w, device=None, act_limit=float("inf"), obs_norm=None):
    import torch
    from walker_gym_amd.policy import MLPPolicy
    mv = lambda a: None if a is None else (torch.from_numpy(a) if device is None else torch.from_numpy(a).to(device))
    return MLPPolicy(mv(w["w2"]), mv(w["b2"]), mv(w["w1"]), mv(w["b1"]), act_limit=act_limit, obs_norm=obs_norm)


# ------------------------------------------------------------------ the modes (auto-reset, noise, normaliser, hold)
# One deep policy per batch through every public method.  The batches are episode_cases' (max_steps = 5, the counters
# staggered by w % 5, about 1 % of the walkers sunk so that they end an episode at every step, a two-row reset pool), used
# with auto-reset on AND off: with it off `done` fires at differing steps, so returns / lengths mean something.
#   balance16   N = 8200, M = 4 (16 walkers per wave, the last tile half full), D = 29, G = 8: the boundary inside a tile
#   canonical4  N = 2050, M = 16 (4 per wave), D = 152, G = 5: the boundary at walker 410 inside a tile
MODES = {"balance16": dict(base="balance16-mid-mlp-8sets", H1=6, H2=5, C=2, G=8, scale=0.03, seed=241),
         "canonical4": dict(base="canonical4-mlp-5sets", H1=10, H2=7, C=8, G=5, scale=0.008, seed=242)}
MODE_L = 1.0
SEED, STEP_BASE, WALKER_BASE, SLOTS = 0x1234567890ABCDEF, 1000, 7, 4
SENTINEL = f32(-12345.0)   # raw / eps rows of the walkers that do not decide


def mode_config(batch):
    import episode_cases as ec
    return ec.config(MODES[batch]["base"])


@functools.lru_cache(maxsize=None)
def mode_rows(batch):
    from oracle.oracle import Oracle
    cfg = mode_config(batch)
    rows = Oracle(cfg["spec"], cfg["params"], n_threads=8).observe()["obs"].copy()
    rows.setflags(write=False)
    return rows


@functools.lru_cache(maxsize=None)
def _mode_weights(batch, norm, identity):
    m = MODES[batch]
    rows = mode_rows(batch)
    D, G = rows.shape[1], m["G"]
    s = 0.25 if norm else m["scale"]          # (normalised inputs are O(1), raw rows hold accelerations in the thousands)
    if identity:
        return identity_pair(D, m["H1"], m["C"], G, m["seed"] + 10, s)
    rng = np.random.default_rng(m["seed"])
    return None, dict(w1=(rng.standard_normal((G, D, m["H1"])) * s).astype(f32),
                      b1=(rng.standard_normal((G, m["H1"])) * s).astype(f32),
                      wm=(rng.standard_normal((G, m["H1"], m["H2"])) * 0.5).astype(f32),
                      bm=(rng.standard_normal((G, m["H2"])) * s).astype(f32),
                      w2=(rng.standard_normal((G, m["H2"], m["C"])) * (4.0 * m["scale"])).astype(f32),
                      b2=(rng.standard_normal((G, m["C"])) * s).astype(f32))


def mode_obs_norm(batch, device="cpu"):
    """An ObsNorm of the batch's entry rows' moments, clip 5."""
    import torch
    from walker_gym_amd.normalize import ObsNorm, obs_moments_numpy, obs_norm_finish_numpy
    rows = mode_rows(batch)
    st = obs_moments_numpy(rows[None], chunk_rows=256)
    mean, scale = obs_norm_finish_numpy(st, 1e-8)
    nm = ObsNorm(rows.shape[1], device, clip=5.0, eps=1e-8)
    nm.load_state_dict(dict(nm.state_dict(), state=torch.from_numpy(st.copy()), mean=torch.from_numpy(mean.copy()),
                            scale=torch.from_numpy(scale.copy())))
    return nm


def mode_policy(batch, device=None, norm=False, identity=False, shallow=False):
    """The batch's deep policy (act_limit 1); identity: wm = I and no bm, with shallow=True its one-layer twin."""
    sh, dp = _mode_weights(batch, norm, identity)
    nm = mode_obs_norm(batch, "cpu" if device is None else device) if norm else None
    return (shallow_from(sh, device, MODE_L, nm) if shallow else policy_from(dp, device, MODE_L, nm))


@functools.lru_cache(maxsize=None)
def mode_sigma(batch):
    m = MODES[batch]
    s = (np.random.default_rng(m["seed"] + 50).uniform(0.5, 1.5, (m["G"], m["C"])) * 0.3).astype(f32)
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def mode_held(batch):
    """The `held` rows a call starts from, [N, C + 1]: drawn, so that a kernel that ignored them cannot pass."""
    m = MODES[batch]
    h = np.random.default_rng(77).uniform(-1, 1, (mode_rows(batch).shape[0], m["C"] + 1)).astype(f32)
    h[:, -1] *= 2
    h.setflags(write=False)
    return h


@functools.lru_cache(maxsize=None)
def mode_reference(batch, auto_reset, noise, norm, every, Tn):
    """The per-step loop of the contract on the CPU (tests/hold_cases.py's, over the deep policy): Oracle (auto-reset
    off) or test_gpu_autoreset._Composed (on) driven by forward_numpy / stochastic_forward_numpy on its own rows, the
    hold spelled out on the host.  With every == 1 `held` at entry is never read."""
    return contract_loop(mode_config(batch), mode_policy(batch, norm=norm), mode_sigma(batch), auto_reset, noise, every,
                         Tn, mode_held(batch))


def contract_loop(cfg, pol, sigma, auto_reset, noise, every, Tn, h0):
    """mode_reference's loop over any episode_cases.config, policy, sigma and entry `held` rows."""
    import episode_cases as ec
    from oracle.oracle import Oracle
    from test_gpu_autoreset import _Composed
    from walker_gym_amd import pg
    Cc = pol.C
    if auto_reset:
        ref = _Composed(cfg["spec"], cfg["params"], 1, cfg["pool"])
        orc = ref.orc
    else:
        ref = orc = Oracle(cfg["spec"], cfg["params"], n_threads=8)
    act, hr = h0[:, :Cc].copy(), h0[:, Cc].copy()
    obs = orc.observe()["obs"]
    keys = ("obs", "reward", "done", "steps_t", "action", "raw", "eps", "decided", "hold_reward", "reset", "final_obs")
    out = {k: [] for k in keys}
    for t in range(Tn):
        dec = pg.hold_decide_numpy(orc.steps, every)
        if noise:
            u, a, e = pg.stochastic_forward_numpy(pol, obs, sigma, SEED, STEP_BASE + t, walker_base=WALKER_BASE)
        else:
            a = pol.forward_numpy(obs)
            u = e = np.zeros_like(a)
        on = dec[:, None] != 0
        act = np.where(on, a, act).astype(f32)
        r = ref.step(act)
        obs = r["obs"]
        rew = np.asarray(r["reward"], f32)
        with np.errstate(all="ignore"):
            hr = np.where(dec != 0, rew, (hr + rew).astype(f32)).astype(f32)
        out["obs"].append(obs.copy()); out["reward"].append(rew.copy())
        out["done"].append(np.asarray(r["done"]).astype(np.uint8))
        out["steps_t"].append(np.asarray(r["steps_out"] if auto_reset else orc.steps).astype(np.int32).copy())
        out["action"].append(act.copy())
        out["raw"].append(np.where(on, u, SENTINEL).astype(f32)); out["eps"].append(np.where(on, e, SENTINEL).astype(f32))
        out["decided"].append(dec.copy()); out["hold_reward"].append(hr.copy())
        if auto_reset:
            out["reset"].append(r["reset"].copy())
            fo = np.full_like(obs, np.nan)   # final_obs: a step writes the rows of the walkers it resets only
            sel = r["reset"] != 0
            fo[sel] = ref.final_obs[sel]
            out["final_obs"].append(fo)
    res = {k: np.stack(v) for k, v in out.items() if v}
    res["held"] = np.concatenate([act, hr[:, None]], axis=1).astype(f32)
    if auto_reset:
        res["state"] = ref.state()
        res["stats"] = ec.accounting(res["reward"], res["reset"], SLOTS)
    else:
        res["state"] = dict(pos=orc.pos.copy(), vel=orc.vel.copy(), acc=orc.acc.copy(), mx=orc.mx.copy(),
                            steps=orc.steps.copy(), contact=orc.contact.copy())
        ret, ln = pc.returns_lengths(res["reward"], res["done"])
        res["stats"] = dict(returns=ret, lengths=ln)
    for v in res.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return res


# ------------------------------------------------------------------ every DEEP instance
# One launch per (IN3D, NE, E8, AR) of the DEEP family: policy_cases.COVER's ten batches (512 full standard tiles at every
# spring-pass count, 2-D and 3-D) under episode_cases.config, a shared (6, 5) policy, T = 4; the records compact and
# 16-byte (WG_EDGE8=0) are the test's axis.  Without auto-reset the deterministic form, with it the noise too.
COVER_T = 4


def cover_policy(name, device=None):
    case = pc.case_of(name)
    rng = np.random.default_rng(2000 + case.seed)
    D, C, s = pc.obs_dim(case), case.C, 0.008
    w = dict(w1=(rng.standard_normal((1, D, 6)) * s).astype(f32), b1=(rng.standard_normal((1, 6)) * s).astype(f32),
             wm=(rng.standard_normal((1, 6, 5)) * 0.5).astype(f32), bm=(rng.standard_normal((1, 5)) * s).astype(f32),
             w2=(rng.standard_normal((1, 5, C)) * 4 * s).astype(f32), b2=(rng.standard_normal((1, C)) * s).astype(f32))
    return policy_from(w, device, MODE_L)


def cover_sigma(name):
    return np.full((1, pc.case_of(name).C), 0.2, f32)


@functools.lru_cache(maxsize=None)
def cover_reference(name, auto_reset):
    import episode_cases as ec
    cfg = ec.config(name)
    h0 = np.zeros((cfg["N"], pc.case_of(name).C + 1), f32)
    return contract_loop(cfg, cover_policy(name), cover_sigma(name), auto_reset, auto_reset, 1, COVER_T, h0)


# (batch, auto_reset, noise, norm, every, T): what tests/test_gpu_deep_rollout.py runs through the public methods
MODE_RUNS = [("balance16", False, False, False, 1, 6), ("balance16", True, False, False, 1, 8),
             ("canonical4", False, True, False, 1, 6), ("canonical4", True, True, False, 1, 8),
             ("canonical4", True, False, True, 1, 8), ("canonical4", True, True, False, 4, 8)]


# ------------------------------------------------------------------ crafted specials in the second layer
# The `six` batch (M = 4, D = 42, A = C = 6), two parameter sets, act_limit 1, H1 = 5, H2 = 6.  w1 / b1 are drawn, so h1 is
# an ordinary non-negative vector; the middle layer is crafted so that given values reach z2 / h2 whatever h1 is:
#   set 0  unit 0: wm[0][0] = NaN -> z2 = NaN -> h2 = +0.0 (a kept NaN would reach column 0 through w2[0][0] = 1)
#          unit 1: bm = -0.0 and a column of -0.0 -> z2 = -0.0 -> h2 = +0.0.  Column 1 starts at b2 = -0.0, its other
#                  weights are -0.0 (h * -0.0 = -0.0 keeps the chain at -0.0) and w2[1][1] = 1: h2 = +0.0 makes the
#                  action +0.0, a kept -0.0 would leave it -0.0
#          unit 2: bm = 1e-40 (a subnormal) and a column of +0.0 -> h2 = 1e-40; w2[2][2] = 2^100 brings it to 1.2e-10 in
#                  column 2, a flushed subnormal would give 0
#          units 3 .. 5 and columns 3 .. 5 are drawn
#   set 1  unit 3: bm = +inf -> h2 = +inf; every w2[3][c] is non-zero (inf * 0 would be NaN), so every column is +-inf
#                  and clips to +-1 by the weight's sign
SPECIAL = dict(kind="six", params=dict(in3d=1), H1=5, H2=6, C=6, G=2, T=3)


@functools.lru_cache(maxsize=None)
def _special_weights():
    rng = np.random.default_rng(251)
    D, H1, H2, C, G = 42, 5, 6, 6, 2
    w = dict(w1=(rng.standard_normal((G, D, H1)) * 0.02).astype(f32), b1=(rng.standard_normal((G, H1)) * 0.02).astype(f32),
             wm=(rng.standard_normal((G, H1, H2)) * 0.3).astype(f32), bm=(rng.standard_normal((G, H2)) * 0.02).astype(f32),
             w2=(rng.standard_normal((G, H2, C)) * 0.08).astype(f32), b2=(rng.standard_normal((G, C)) * 0.02).astype(f32))
    w["wm"][0, 0, 0] = np.nan
    w["wm"][0, :, 1], w["bm"][0, 1] = -0.0, -0.0
    w["wm"][0, :, 2], w["bm"][0, 2] = 0.0, f32(1e-40)
    w["w2"][0, :, :3] = 0.0
    w["w2"][0, 0, 0] = 1.0
    w["w2"][0, :, 1], w["w2"][0, 1, 1], w["b2"][0, 1] = -0.0, 1.0, -0.0
    w["w2"][0, 2, 2], w["b2"][0, 2] = f32(2.0 ** 100), 0.0
    w["bm"][1, 3] = np.inf
    assert (w["w2"][1, 3] != 0).all()
    return w


def special_weights():
    return {k: a.copy() for k, a in _special_weights().items()}


@functools.lru_cache(maxsize=None)
def special_rollout():
    return oracle_loop(pc.spec_of("six"), SPECIAL["params"], policy_from(special_weights(), act_limit=1.0), SPECIAL["T"])

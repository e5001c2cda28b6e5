"""Non-default parameters on every lean step and rollout instance: the shapes and the variants that
tests/test_param_cases_cpu.py (oracle only) and tests/test_gpu_param_instances.py (bit for bit on the GPU) share.  No GPU
import here.

Shapes are the smallest batches at which each instance can be selected:
  ne1 .. ne8   the five PASSES batches of tests/test_gpu_edge8.py: 8,192 walkers of M = 4, K = 4, A = 2 (16 per wave, one
               pass) and 512 walkers of M = 64 with K = 120 / 150 / 200 / 300 (one per wave: 2, 3, 4 and 5 passes, the
               last on the NE 8 instance): full tiles, the compact records, FIX / WT where the parameters allow
  ne1+1        ne1 and one walker more: 513 tiles, the last one holds a single walker (the generic instance, compact)
  canon+1      2,049 canonical walkers (M = 16, four per wave, three passes), the last tile partial
  canon5       5 canonical walkers: tiles halved to one walker per wave, 48 idle lanes, the 16-byte records although
               the compact ones are present
  m4x17        17 walkers of M = 4: halved tiles with idle lanes, as above
Each runs at IN3D 0 and 1.

A variant is a params dict (it may depend on the shape), a function that edits the spec, and a function that shapes the
actions (0 / 1 for the discrete ones).  A variant combines only parameters that do not mask each other."""
import functools

import numpy as np

STEPS, RUN_STEPS = 2, 3     # test_step: two closed-loop step()s, then one run() of three; test_resident: three
AR_STEPS = 6                # test_auto_reset
AR_MAX_STEPS = 3            # ... with episodes this short (env-runtime keeps its own max_steps = 2)
POLICY_STEPS = {False: 4, True: 8}   # test_policy_rollout: auto-reset off / on

_PASSES = [(1, dict(N=8192, M=4, K=4, A=2)), (2, dict(N=512, M=64, K=120, A=8)), (3, dict(N=512, M=64, K=150, A=8)),
           (4, dict(N=512, M=64, K=200, A=8)), (8, dict(N=512, M=64, K=300, A=8))]   # = test_gpu_edge8.PASSES
SHAPES = {f"ne{ne}": kw for ne, kw in _PASSES}
FULL = list(SHAPES)                                   # the five full-tile batches
SHAPES.update({"ne1+1": dict(N=8193, M=4, K=4, A=2), "canon+1": dict(N=2049, M=16, K=40, A=8),
               "canon5": dict(N=5, M=16, K=40, A=8), "m4x17": dict(N=17, M=4, K=4, A=2)})
PAIR_SHAPES = ["ne1", "ne2"]                          # pairs-7 / pairs-24: M = 4 and M = 64, K = 120


# ---------------------------------------------------------------- the host's selection arithmetic, restated
def select(N, M, K):
    """lean_geo / lean_passes / use_edge8 of csrc/wg_host.h for a batch whose compact records exist: walkers per wave
    (halved until there are 512 tiles), spring passes, whether the compact records are read, whether every tile is
    full.  tests/test_gpu_param_instances.py asserts it against launch_geometry() at every launch."""
    wpw = 64 // M
    while wpw > 1 and -(-N // wpw) < 512:
        wpw >>= 1
    return dict(wpw=wpw, passes=-(-wpw * K // 64), compact=wpw * M == 64, full=N % wpw == 0)


def fix_expected(N, M, K, fix_params):
    """lean_fix_ok: the compact records in one to four passes, full tiles, and parameters it does not refuse."""
    s = select(N, M, K)
    return bool(fix_params and s["compact"] and s["full"] and s["passes"] <= 4)


def wt_expected(N, M, K, A, in3d, fix_params):
    """lean_wt_ok for the env's own unpadded rows: a FIX launch of two passes or more whose tile image (pos, vel, the
    rows) is a multiple of 16 B and fits the spring terms' area of the wave's slice."""
    s = select(N, M, K)
    if not fix_expected(N, M, K, fix_params) or s["passes"] < 2:
        return False
    a16 = lambda n: (n + 15) & ~15
    pl = (s["wpw"] * K + 3) & ~3
    rows_b = s["wpw"] * (3 * (3 if in3d else 2) * M + A) * 4
    return rows_b % 16 == 0 and 2 * 768 + rows_b <= a16(pl * 24) + a16(pl * 12)


def run_ranges(N, lanes=2):
    """The walker ranges of run(lanes=...) (BatchedPhysicsEnv._lanes and ranges.uniform_bounds)."""
    if N < 64 * lanes:
        return [N]
    b = [0] + [((N * i // lanes) + 63) // 64 * 64 for i in range(1, lanes)] + [N]
    return [b[i + 1] - b[i] for i in range(lanes)]


# ---------------------------------------------------------------- specs
@functools.lru_cache(maxsize=None)
def _base_spec(shape):
    from walker_gym_amd.synthetic import canonical_walkers
    kw = dict(SHAPES[shape])
    spec = canonical_walkers(kw.pop("N"), seed=5, **kw)
    for v in spec.values():
        v.setflags(write=False)
    return spec


def _edit_none(spec, shape):
    return spec


def _edit_pinned(spec, shape):
    """About 5 % of the masses pinned (seeded), one of them in the first tile and one in the last; non-zero start
    velocities.  A pinned mass (DingPoint) takes no force but still integrates its velocity, so the pinned masses start
    at rest: their positions must not move."""
    P = len(spec["m"])
    rng = np.random.default_rng(23)
    pin = (rng.random(P) < 0.05).astype(np.uint8)
    pin[1] = pin[P - 2] = 1
    vel = rng.uniform(-3, 3, (P, 3)).astype(np.float32)
    vel[pin != 0] = 0
    spec["pinned"], spec["vel"] = pin, vel
    return spec


SHRINK = np.float32(0.4)


def _edit_pairs(spec, shape, bounce_set=True):
    """test_pair_forces_4096_vs_oracle's edits: the walker shrunk by 0.4 (the masses come within each other's radii),
    seeded charges and radii, and for pairs-all the caller / list bits of Point.bounce(k, other=<list>)."""
    P = len(spec["m"])
    spec["pos"] = (spec["pos"] * SHRINK).astype(np.float32)
    spec["rest"] = (spec["rest"] * SHRINK).astype(np.float32)
    rng = np.random.default_rng(5)
    spec["charge"] = rng.uniform(-3, 3, P)
    spec["radius"] = rng.uniform(1.5, 3.0, P)
    if bounce_set:
        spec["bounce_set"] = rng.integers(0, 4, P).astype(np.uint8)
    return spec


def _edit_pairs_plain(spec, shape):
    return _edit_pairs(spec, shape, bounce_set=False)


# ---------------------------------------------------------------- params
PAIR = dict(pair_g=2000.0, pair_k=1.0e4, bounce_k=2000.0)     # as test_pair_forces_4096_vs_oracle
OBS_SCALED = dict(midform=0, pk=0.3, vk=1.7, ak=0.011, mk=2.3)   # four different values, none a power of two


def _env_runtime(shape):
    """dampk, friction_mode 1, max_steps = 2 (done fires for every walker at the script's second step) and the ground
    raised to the walker's height + 50: done_y = ground - 50 then lies inside the batch's spread of mean heights after
    one step (the masses, all below ground, are pushed up by groundk * depth / m, and m differs per mass), so the done
    rule's height test ends some walkers and not others at step 1.  The lattice's mean height is 5 * sqrt(M) (rows at 5,
    15, ...); the offsets were chosen on the oracle alone and are held by test_param_cases_cpu.py."""
    M = SHAPES[shape]["M"]
    side = int(round(M ** 0.5))
    return dict(dampk=0.3, ground=50.0 + 5.0 * side + RUNTIME_LIFT, friction_mode=1, max_steps=2)


RUNTIME_LIFT = 2.0   # about what one step lifts the median walker's mean height, at every lattice size


class Variant:
    def __init__(self, name, params, edit=_edit_none, discrete=False, fix=False, pairs=False, moves=(), shapes=None):
        self.name, self._params, self.edit, self.discrete = name, params, edit, discrete
        self.fix = fix          # lean_fix_ok admits these parameters (full tiles take the FIX / WT instances)
        self.pairs = pairs      # NaN == NaN allowed, the finite share 95 %; step and run() only
        self.moves = moves      # the arrays that must differ from a default-parameter run of the same spec
        self.shapes = list(SHAPES) if shapes is None else shapes

    def params(self, shape, in3d):
        p = self._params(shape) if callable(self._params) else self._params
        return dict(p, in3d=in3d)

    def __repr__(self):
        return self.name


VARIANTS = [
    Variant("obs-scaled", OBS_SCALED, moves=("obs",)),
    Variant("obs-mid2", dict(midform=2, conmid=1), moves=("obs",)),   # (the oracle takes the pair in 3-D too)
    Variant("discrete", dict(action_mode=1), discrete=True, moves=("muscle_x",)),
    Variant("run2-pinned", dict(integrator=2), _edit_pinned, moves=("pos",)),
    Variant("env-runtime", _env_runtime, fix=True, moves=("done", "reward")),
    Variant("pairs-all", dict(PAIR, pair_mode=31), _edit_pairs, pairs=True, moves=("pos",)),
    Variant("pairs-7", dict(PAIR, pair_mode=7), _edit_pairs_plain, pairs=True, moves=("pos",), shapes=PAIR_SHAPES),
    Variant("pairs-24", dict(PAIR, pair_mode=24), _edit_pairs_plain, pairs=True, moves=("pos",), shapes=PAIR_SHAPES),
]
# walker_rollout_policy: one combined variant (the observation scales and raw positions feed the policy, run2 and the
# pins move the state), and the same with discrete actions, which rollout_policy accepts (check_discrete)
POLICY_VARIANTS = [
    Variant("scaled-run2", dict(OBS_SCALED, integrator=2), _edit_pinned, moves=("obs", "pos")),
    Variant("scaled-run2-discrete", dict(OBS_SCALED, integrator=2, action_mode=1), _edit_pinned, discrete=True,
            moves=("obs", "pos", "muscle_x")),
]
RESIDENT = [v for v in VARIANTS if not v.pairs]


def variant(name):
    return next(v for v in VARIANTS + POLICY_VARIANTS if v.name == name)


def step_cells():
    """(shape, in3d, variant name) of every test_step launch."""
    return [(s, d, v.name) for v in VARIANTS for s in v.shapes for d in (0, 1)]


def resident_cells():
    return [(s, d, v.name) for v in RESIDENT for s in SHAPES for d in (0, 1)]


def auto_reset_cells():
    return [(s, d, v.name) for v in RESIDENT for s in FULL for d in (0, 1)]


def cell_id(cell):
    s, d, v = cell
    return f"{v}-{s}-{2 + d}d"


def spec_of(shape, name):
    """A fresh, writable spec of the shape with the variant's edits."""
    spec = {k: np.array(a, copy=True) for k, a in _base_spec(shape).items()}
    return variant(name).edit(spec, shape)


def actions(shape, name, T, seed=11):
    """[T, N, A] float32 actions in (-1, 1); for a discrete variant 0 / 1 (Muscle.actdisp tests `a != 0`)."""
    kw = SHAPES[shape]
    a = np.random.default_rng(seed).uniform(-1, 1, (T, kw["N"], kw["A"])).astype(np.float32)
    return (a > 0).astype(np.float32) if variant(name).discrete else a


# ---------------------------------------------------------------- oracle runs (computed once, shared, never modified)
def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def scripted(shape, in3d, name, default=False):
    """The oracle after RUN_STEPS scripted steps under the variant (default: the same spec and actions under the default
    parameters): every step's outputs and the state after each step."""
    from oracle.oracle import Oracle
    v = variant(name)
    params = dict(in3d=in3d) if default else v.params(shape, in3d)
    spec = spec_of(shape, name)
    orc = Oracle(spec, params, n_threads=8)
    start = orc.pos.copy()
    steps = []
    for a in actions(shape, name, RUN_STEPS):
        out = orc.step(a)
        steps.append(_frozen(dict(out, pos=orc.pos.copy(), vel=orc.vel.copy(), acc=orc.acc.copy(),
                                  muscle_x=orc.mx.copy(), steps=orc.steps.copy(), contact=orc.contact.copy(),
                                  radius=orc.radius.copy())))
    return dict(steps=steps, start=start, mass_off=orc.mass_off.copy(),
                pinned=None if orc.pinned is None else orc.pinned.copy())


def finite_walkers(state, mass_off):
    """Per walker: every component of pos / vel / acc finite."""
    ok = np.isfinite(state["pos"]).all(1) & np.isfinite(state["vel"]).all(1) & np.isfinite(state["acc"]).all(1)
    return np.logical_and.reduceat(ok, np.asarray(mass_off[:-1], np.int64))


def ar_config(shape, in3d, name):
    """The auto-reset inputs of a cell, as tests/test_gpu_autoreset._config makes them: the variant's spec with the step
    counters staggered and about 1 % of the walkers (at least two) sunk to mean y = -80, a two-row noise pool, short
    episodes."""
    v = variant(name)
    spec = spec_of(shape, name)
    params = v.params(shape, in3d)
    params.setdefault("max_steps", AR_MAX_STEPS)
    ms = params["max_steps"]
    mo = np.asarray(spec["mass_off"])
    N = len(mo) - 1
    rng = np.random.default_rng(11)
    pos = np.array(spec["pos"], np.float32).reshape(-1, 3).copy()
    sunk = rng.permutation(N)[:max(2, N // 100)]
    for w in sunk:
        a, b = mo[w], mo[w + 1]
        pos[a:b, 1] += np.float32(-80.0) - pos[a:b, 1].mean()
    spec["pos"] = pos
    spec["steps"] = (np.arange(N) % ms).astype(np.int32)
    pool = (rng.standard_normal((2, len(pos), 3)) * 0.5).astype(np.float32)
    return dict(spec=spec, params=params, pool=pool, N=N, sunk=sunk, acts=actions(shape, name, AR_STEPS, seed=12))


@functools.lru_cache(maxsize=None)
def ar_reference(shape, in3d, name):
    """Every step's outputs and state of the composed oracle (test_gpu_autoreset._Composed) for a cell."""
    from test_gpu_autoreset import _Composed
    cfg = ar_config(shape, in3d, name)
    ref = _Composed(cfg["spec"], cfg["params"], 1, cfg["pool"])
    steps = []
    for t in range(AR_STEPS):
        out = ref.step(cfg["acts"][t])
        steps.append(dict(out=out, state=ref.state()))
    return steps


# ---------------------------------------------------------------- walker_rollout_policy
def policy_config(case_name, name, auto_reset):
    """One policy_cases.COVER batch under a POLICY_VARIANTS variant: spec, params (and, with auto-reset, the sunk walkers,
    the staggered counters and the noise pool of tests/episode_cases.config)."""
    import episode_cases as ec
    import policy_cases as pc
    case = pc.case_of(case_name)
    v = variant(name)
    spec = {k: np.array(a, copy=True) for k, a in pc.spec_of(case.kind).items()}
    spec = v.edit(spec, None)
    params = dict(v._params, **case.params)
    cfg = dict(case=case, spec=spec, params=params, pool=None)
    if auto_reset:
        mo = np.asarray(spec["mass_off"])
        N = len(mo) - 1
        rng = np.random.default_rng(11)
        pos = np.array(spec["pos"], np.float32).reshape(-1, 3).copy()
        for w in rng.permutation(N)[:max(2, N // 100)]:
            a, b = mo[w], mo[w + 1]
            pos[a:b, 1] += np.float32(-80.0) - pos[a:b, 1].mean()
        spec["pos"] = pos
        spec["steps"] = (np.arange(N) % ec.MAX_STEPS).astype(np.int32)
        cfg["pool"] = (rng.standard_normal((2, len(pos), 3)) * 0.5).astype(np.float32)
        cfg["params"] = dict(params, max_steps=ec.MAX_STEPS)
    return cfg


@functools.lru_cache(maxsize=None)
def policy_reference(case_name, name, auto_reset):
    """The closed loop on the CPU: policy.forward_numpy on the reference's own rows, through Oracle.step (auto-reset
    off, as policy_cases.oracle_rollout) or the composed reference (on, as episode_cases.reference)."""
    import episode_cases as ec
    import policy_cases as pc
    from oracle.oracle import Oracle
    from test_gpu_autoreset import _Composed
    cfg = policy_config(case_name, name, auto_reset)
    pol = pc.policy_of(cfg["case"])
    T = POLICY_STEPS[auto_reset]
    keys = ("action", "obs", "reward", "done") + (("reset", "final_obs") if auto_reset else ())
    out = {k: [] for k in keys}
    if auto_reset:
        ref = _Composed(cfg["spec"], cfg["params"], 1, cfg["pool"])
        orc = ref.orc
    else:
        ref = orc = Oracle(cfg["spec"], cfg["params"], n_threads=8)
    obs = orc.observe()["obs"]
    for t in range(T):
        a = pol.forward_numpy(obs)
        r = ref.step(a)
        obs = r["obs"]
        out["action"].append(a); out["obs"].append(obs.copy()); out["reward"].append(r["reward"].copy())
        out["done"].append(np.asarray(r["done"]).astype(np.uint8))
        if auto_reset:
            out["reset"].append(r["reset"].copy())
            fo = np.full_like(obs, np.nan)   # a step writes the rows of the walkers it resets only
            sel = r["reset"] != 0
            fo[sel] = ref.final_obs[sel]
            out["final_obs"].append(fo)
    res = {k: np.stack(x) for k, x in out.items()}
    if auto_reset:
        res["state"] = ref.state()
        res["stats"] = ec.accounting(res["reward"], res["reset"], ec.SLOTS)
    else:
        res["state"] = dict(pos=orc.pos.copy(), vel=orc.vel.copy(), acc=orc.acc.copy(), mx=orc.mx.copy(),
                            steps=orc.steps.copy(), contact=orc.contact.copy())
    res["mass_off"], res["start"] = orc.mass_off.copy(), np.array(cfg["spec"]["pos"], np.float32).reshape(-1, 3)
    res["pinned"] = None if orc.pinned is None else orc.pinned.copy()
    return _frozen(res)

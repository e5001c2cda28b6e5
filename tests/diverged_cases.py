"""Non-finite state on every instance that carries the diverged-walker stand-in path: the walker kinds, where they sit
in a wave tile, the shapes and the references that tests/test_diverged_cases_cpu.py (oracle only) and
tests/test_gpu_diverged_instances.py (bit for bit on the GPU) share.  No GPU import here.  (test_gpu_diverged._diverge is
another helper and stays as it is.)

Kinds (KINDS):
  dead-x / dead-z / dead-y   the named position component NaN in every mass (dead-z at IN3D 1 only)
  dead-mixed                 the NaN component varies per mass (mass 0: x, mass 1: z, the others drawn), every third mass
                             has two NaN components
  dead-vel                   dead-mixed with an all-NaN velocity
  part                       x NaN in mass 0 alone (more, and at M = 4 every mass has a NaN neighbour and the walker is all
                             NaN after one step like a dead one): the plain path
  inf-up / inf-down          y = +inf / -inf in every mass: the plain path; inf-down is below the ground
  dead-pinned                dead-mixed with one pinned mass: it steps exactly (only where `pins`: FIX refuses pinned
                             batches, so the cells that are there for the FIX / WT instances have none)
  alive
The ground is the batch's median starting height, so about half of the finite-y masses of dead and alive walkers alike
start in contact: the reference tests the ground on the y a step starts from, which a NaN in x or z leaves finite.

Placement is by position in the wave tile (the launch's walkers per wave; where that is one, by groups of four tiles,
the waves of a workgroup): tiles whose first walker alone is dead, whose last walker alone is dead, where dead and alive
walkers alternate, wholly dead tiles, tiles that mix the other kinds with dead and alive neighbours, the batch's last
walker (in the partial tile where the shape has one), and tiles with none of these.  The dead kinds cycle from dead-x
within every placement, so a NaN-x walker sits first in a tile and another one last.

Shapes: param_cases.SHAPES and two full-tile batches that complete the mask widths M in {4, 8, 16, 32, 64}:
  m8    4,096 walkers of M = 8 (a 2 x 4 lattice, its perimeter's 8 springs): 8 per wave, one pass
  m32   1,024 walkers of M = 32 (4 x 8, 52 lattice springs and 12 drawn): 2 per wave, two passes
The two batches of 5 and 17 walkers cannot hold the counts of the larger ones (20 dead, 10 of every other kind): they
take one walker of every kind that fits, in the same placement order."""
import functools

import numpy as np

import param_cases as P

DEAD = ("dead-x", "dead-z", "dead-y", "dead-mixed", "dead-vel")
OTHER = ("part", "inf-up", "inf-down", "dead-pinned")
KINDS = DEAD + OTHER + ("alive",)
CONTACT_DEAD = ("dead-x", "dead-z", "dead-mixed", "dead-vel")   # a finite y below the ground in some mass

STEPS = 3            # the defect at step 1, contact back to 0 at step 2, the keep_aux flip of run() at step 3
AR_STEPS = 6
AR_MAX_STEPS = 3
POLICY_T = (1, 4)

NEW = {"m8": dict(N=4096, M=8, K=8, A=2), "m32": dict(N=1024, M=32, K=64, A=8)}
SHAPES = dict(P.SHAPES, **NEW)
FULL = P.FULL + list(NEW)                       # full standard tiles, the compact records
SMALL = ("canon5", "m4x17")                     # no room for the counts
SEEDS = {s: 300 + i for i, s in enumerate(SHAPES)}
MIN_DEAD, MIN_OTHER = 20, 10


def select(shape):
    kw = SHAPES[shape]
    return P.select(kw["N"], kw["M"], kw["K"])


def fix_expected(shape):
    kw = SHAPES[shape]
    return P.fix_expected(kw["N"], kw["M"], kw["K"], True)


def wt_expected(shape, in3d):
    kw = SHAPES[shape]
    return P.wt_expected(kw["N"], kw["M"], kw["K"], kw["A"], in3d, True)


def pins_of(shape):
    """dead-pinned walkers only where the default launch is not there for FIX / WT."""
    return not fix_expected(shape)


# ---------------------------------------------------------------- the two new batches
def lattice_walkers(N, rows, cols, K, A, seed):
    """canonical_walkers' recipe on a rows x cols lattice (spacing 10, jitter 1, m ~ U(1, 5), at rest, k = 1000, c = 20,
    the first A springs muscles): the lattice springs and K - len(lattice) drawn other pairs, or, for K = M on two rows,
    the perimeter cycle alone (every mass keeps two springs)."""
    from walker_gym_amd.synthetic import norm3_f32
    M = rows * cols
    lat = [(r * cols + c, r * cols + c + 1) for r in range(rows) for c in range(cols - 1)]
    lat += [(r * cols + c, (r + 1) * cols + c) for r in range(rows - 1) for c in range(cols)]
    rng = np.random.default_rng(seed)
    m = rng.uniform(1.0, 5.0, (N, M)).astype(np.float32)
    cc, rr = np.tile(np.arange(cols), rows), np.repeat(np.arange(rows), cols)
    base = np.stack([10.0 * cc - 5.0 * (cols - 1), 10.0 * rr + 5.0, np.zeros(M)], axis=1).astype(np.float32)
    pos = (base[None] + rng.uniform(-1.0, 1.0, (N, M, 3))).astype(np.float32)
    if K < len(lat):
        assert rows == 2 and K == M
        ring = list(range(cols)) + list(range(2 * cols - 1, cols - 1, -1))
        pairs = np.array([(ring[i], ring[(i + 1) % M]) for i in range(M)], np.int32)
        pairs = np.broadcast_to(pairs, (N, K, 2))
    else:
        have = set(lat)
        others = np.array([(i, j) for i in range(M) for j in range(i + 1, M) if (i, j) not in have], np.int32)
        pick = np.argsort(rng.random((N, len(others))), axis=1)[:, :K - len(lat)]
        pairs = np.concatenate([np.broadcast_to(np.array(lat, np.int32), (N, len(lat), 2)), others[pick]], axis=1)
    ei, ej = pairs[..., 0].astype(np.int32), pairs[..., 1].astype(np.int32)
    wi = np.arange(N)[:, None]
    rest = norm3_f32(pos[wi, ei] - pos[wi, ej])
    Pn = N * M
    return dict(
        m=m.reshape(Pn), pos=pos.reshape(Pn, 3), vel=np.zeros((Pn, 3), np.float32), acc=np.zeros((Pn, 3), np.float32),
        mass_off=(np.arange(N + 1) * M).astype(np.int32), ei=ei.reshape(-1), ej=ej.reshape(-1),
        rest=rest.reshape(-1).astype(np.float32), k=np.full(N * K, 1000.0, np.float32),
        c=np.full(N * K, 20.0, np.float32), flags=np.zeros(N * K, np.uint8),
        edge_off=(np.arange(N + 1) * K).astype(np.int32), n_muscles=np.full(N, A, np.int32),
        minl=np.full(N * A, 0.1, np.float32), maxl=np.full(N * A, 1.5, np.float32),
        stride=np.full(N * A, 2.0, np.float32))


@functools.lru_cache(maxsize=None)
def _base_spec(shape):
    if shape in P.SHAPES:
        return P._base_spec(shape)
    kw = NEW[shape]
    rows = {8: 2, 32: 4}[kw["M"]]
    spec = lattice_walkers(kw["N"], rows, kw["M"] // rows, kw["K"], kw["A"], seed=5)
    for v in spec.values():
        v.setflags(write=False)
    return spec


def base_spec(shape):
    """A fresh, writable copy of the shape's batch."""
    return {k: np.array(a, copy=True) for k, a in _base_spec(shape).items()}


# ---------------------------------------------------------------- placement
def tile_groups(N, wpw):
    """The walkers of every wave tile of a uniform batch, in order (the last one may be partial)."""
    return [np.arange(s, min(s + wpw, N)) for s in range(0, N, wpw)]


def _jobs(n_tiles, g, small):
    """The placement of every tile but the last, in the order the tiles are drawn: enough of each for the counts, the
    kinds interleaved so that a batch of few tiles still gets one of each first."""
    per_other = -(-g // 3)                                   # other-kind walkers of one `mixed` tile
    want = dict(alternate=4, mixed=-(-len(OTHER) * (MIN_OTHER + 2) // per_other), whole=3, first=6, last=6)
    if small:   # (the mixed tiles first: they hold the other kinds)
        return ["mixed", "alternate", "mixed", "whole", "first", "last"][:max(0, n_tiles - 1)]
    jobs = []
    while any(want.values()):
        for k in ("alternate", "mixed", "whole", "first", "last"):
            if want[k]:
                want[k] -= 1
                jobs.append(k)
    # (a batch with room for the counts keeps at least a quarter of its tiles without any of these)
    return jobs[:3 * (n_tiles - 1) // 4]


def place(groups, in3d, seed, pins=True, small=False):
    """The kind of every walker: `groups` are the wave tiles (arrays of walker indices; where every tile is one walker,
    groups of four tiles)."""
    N = sum(len(g) for g in groups)
    if max(len(g) for g in groups) == 1:
        flat = np.concatenate(groups)
        groups = [flat[s:s + 4] for s in range(0, N, 4)]
    kinds = np.full(N, "alive", dtype="<U12")
    dead = [k for k in DEAD if in3d or k != "dead-z"]
    other = [k for k in OTHER if pins or k != "dead-pinned"]
    rng = np.random.default_rng(seed)
    g = max(len(t) for t in groups)
    order = rng.permutation(len(groups) - 1) if len(groups) > 1 else np.zeros(0, int)
    count = dict(alternate=0, whole=0, first=0, last=0, mixed=0, other=0)

    def next_dead(job):
        job = "whole" if small else job   # (a batch of few walkers: one cycle, so that it holds every dead kind)
        count[job] += 1
        return dead[(count[job] - 1) % len(dead)]

    for ti, job in zip(order, _jobs(len(groups), g, small)):
        t = groups[ti]
        if job == "first":
            kinds[t[0]] = next_dead(job)
        elif job == "last":
            kinds[t[-1]] = next_dead(job)
        elif job == "alternate":
            for w in t[(ti % 2)::2]:   # (from the first walker in even tiles, from the second in odd ones)
                kinds[w] = next_dead(job)
        elif job == "whole":
            for w in t:
                kinds[w] = next_dead(job)
        else:   # mixed: an other kind, an alive walker, a dead one, ...
            for s, w in enumerate(t):
                if s % 3 == 0:
                    kinds[w] = other[count["other"] % len(other)]
                    count["other"] += 1
                elif s % 3 == 2:
                    kinds[w] = next_dead(job)
    kinds[groups[-1][-1]] = "dead-x"   # the batch's last walker (alone in its tile where that tile is partial)
    return kinds


def apply_kinds(spec, kinds, seed, ground=True):
    """The spec with every walker made its kind, and the ground at the batch's median starting height."""
    mo = np.asarray(spec["mass_off"], np.int64)
    pos = np.array(spec["pos"], np.float32).reshape(-1, 3).copy()
    vel = np.array(spec["vel"], np.float32).reshape(-1, 3).copy()
    level = float(np.median(pos[:, 1]))
    pinned = np.zeros(len(pos), np.uint8)
    rng = np.random.default_rng(seed + 1)
    for w, kind in enumerate(kinds):
        a, b = int(mo[w]), int(mo[w + 1])
        n = b - a
        if kind == "alive":
            continue
        if kind in ("dead-x", "dead-y", "dead-z"):
            pos[a:b, "xyz".index(kind[-1])] = np.nan
        elif kind in ("dead-mixed", "dead-vel", "dead-pinned"):
            comp = rng.integers(0, 3, n)
            comp[0] = 0
            if n > 1:
                comp[1] = 2
            idx = np.arange(a, b)
            pos[idx, comp] = np.nan
            two = np.arange(n) % 3 == 2
            pos[idx[two], (comp[two] + 1) % 3] = np.nan
            if kind == "dead-vel":
                vel[a:b] = np.nan
            if kind == "dead-pinned":
                pinned[a + int(rng.integers(0, n))] = 1
        elif kind == "part":
            pos[a, 0] = np.nan
        elif kind == "inf-up":
            pos[a:b, 1] = np.inf
        elif kind == "inf-down":
            pos[a:b, 1] = -np.inf
        else:
            raise KeyError(kind)
    out = dict(spec, pos=pos, vel=vel)
    if pinned.any():
        out["pinned"] = pinned
    return out, level


def diverge(spec, in3d, groups, seed, pins=True, small=False):
    """A flat spec with diverged walkers: (the edited spec, the parameters, the kind of every walker)."""
    kinds = place(groups, in3d, seed, pins, small)
    out, level = apply_kinds(spec, kinds, seed)
    return out, dict(in3d=in3d, ground=level), kinds


def case(shape, in3d, pins=None):
    """(spec, params, kinds) of a shape: fresh arrays."""
    kw = SHAPES[shape]
    pins = pins_of(shape) if pins is None else pins
    return diverge(base_spec(shape), in3d, tile_groups(kw["N"], select(shape)["wpw"]), SEEDS[shape], pins,
                   shape in SMALL)


def actions(shape, T, seed=11):
    kw = SHAPES[shape]
    return np.random.default_rng(seed).uniform(-1, 1, (T, kw["N"], kw["A"])).astype(np.float32)


def cells():
    return [(s, d) for s in SHAPES for d in (0, 1)]


def cell_id(cell):
    return f"{cell[0]}-{2 + cell[1]}d"


# ---------------------------------------------------------------- oracle runs (computed once, shared, never modified)
def _snap(orc, out=None):
    d = dict(pos=orc.pos.copy(), vel=orc.vel.copy(), acc=orc.acc.copy(), muscle_x=orc.mx.copy(),
             steps=orc.steps.copy(), contact=orc.contact.copy(), radius=orc.radius.copy())
    if out is not None:
        d.update(out)
    return P._frozen(d)


@functools.lru_cache(maxsize=None)
def scripted(shape, in3d, pins=None):
    """The oracle's STEPS scripted steps of a cell: every step's outputs and the state after it, the start, the kinds."""
    from oracle.oracle import Oracle
    spec, params, kinds = case(shape, in3d, pins)
    orc = Oracle(spec, params, n_threads=8)
    start = orc.pos.copy()
    steps = [_snap(orc, orc.step(a)) for a in actions(shape, STEPS)]
    return dict(steps=steps, start=start, kinds=kinds, ground=params["ground"], mass_off=orc.mass_off.copy())


def ar_config(shape, in3d):
    """The auto-reset inputs of a cell (as param_cases.ar_config): the diverged spec with the step counters staggered and
    about 1 % of the alive walkers (at least two) sunk 80 below the ground, a two-row noise pool, short episodes.  A
    dead walker whose counter runs out goes back to its snapshot, which is dead again: step 1 of the path once more."""
    spec, params, kinds = case(shape, in3d, True)
    params = dict(params, max_steps=AR_MAX_STEPS)
    mo = np.asarray(spec["mass_off"])
    N = len(mo) - 1
    rng = np.random.default_rng(11)
    pos = spec["pos"]
    alive = np.flatnonzero(kinds == "alive")
    sunk = alive[rng.permutation(len(alive))[:max(2, N // 100)]]
    for w in sunk:
        a, b = mo[w], mo[w + 1]
        pos[a:b, 1] += np.float32(params["ground"] - 80.0) - pos[a:b, 1].mean()
    spec["steps"] = (np.arange(N) % AR_MAX_STEPS).astype(np.int32)
    pool = (rng.standard_normal((2, len(pos), 3)) * 0.5).astype(np.float32)
    return dict(spec=spec, params=params, pool=pool, N=N, sunk=sunk, kinds=kinds, acts=actions(shape, AR_STEPS, seed=12))


@functools.lru_cache(maxsize=None)
def ar_reference(shape, in3d):
    """Every step's outputs and state of the composed oracle (test_gpu_autoreset._Composed) for a cell."""
    from test_gpu_autoreset import _Composed
    cfg = ar_config(shape, in3d)
    ref = _Composed(cfg["spec"], cfg["params"], 1, cfg["pool"])
    steps = []
    for t in range(AR_STEPS):
        out = ref.step(cfg["acts"][t])
        steps.append(dict(out=out, state=ref.state()))
    return steps


# ---------------------------------------------------------------- walker_rollout_policy (policy_cases.COVER)
def policy_config(case_name, auto_reset):
    """One policy_cases.COVER batch (512 full tiles) with diverged walkers, and with auto-reset the sunk walkers, the
    staggered counters and the pool of episode_cases.config."""
    import episode_cases as ec
    import policy_cases as pc
    c = pc.case_of(case_name)
    spec = {k: np.array(a, copy=True) for k, a in pc.spec_of(c.kind).items()}
    N = len(spec["mass_off"]) - 1
    in3d = int(c.params["in3d"])
    spec, params, kinds = diverge(spec, in3d, tile_groups(N, c.wpw), 500 + c.seed, True)
    cfg = dict(case=c, spec=spec, params=dict(c.params, ground=params["ground"]), pool=None, kinds=kinds, N=N)
    if auto_reset:
        mo = np.asarray(spec["mass_off"])
        rng = np.random.default_rng(11)
        alive = np.flatnonzero(kinds == "alive")
        for w in alive[rng.permutation(len(alive))[:max(2, N // 100)]]:
            a, b = mo[w], mo[w + 1]
            spec["pos"][a:b, 1] += np.float32(params["ground"] - 80.0) - spec["pos"][a:b, 1].mean()
        spec["steps"] = (np.arange(N) % ec.MAX_STEPS).astype(np.int32)
        cfg["pool"] = (rng.standard_normal((2, len(spec["pos"]), 3)) * 0.5).astype(np.float32)
        cfg["params"] = dict(cfg["params"], max_steps=ec.MAX_STEPS)
    return cfg


@functools.lru_cache(maxsize=None)
def policy_reference(case_name, auto_reset, noise):
    """The closed loop on the CPU for max(POLICY_T) steps: the policy (deterministic, or pg.stochastic_forward_numpy with
    pg_cases' sigma, seed and counters) on the reference's own rows, through Oracle.step or the composed reference.
    Every step's outputs and the state after every step (a rollout of T steps ends in states[T - 1])."""
    import episode_cases as ec
    import pg_cases as gc
    import policy_cases as pc
    from oracle.oracle import Oracle
    from test_gpu_autoreset import _Composed
    cfg = policy_config(case_name, auto_reset)
    pol = pc.policy_of(cfg["case"])
    keys = ("action", "obs", "reward", "done") + (("raw", "eps") if noise else ()) + \
        (("reset", "final_obs", "steps_t") if auto_reset else ())
    out = {k: [] for k in keys}
    if auto_reset:
        ref = _Composed(cfg["spec"], cfg["params"], 1, cfg["pool"])
        orc = ref.orc
    else:
        ref = orc = Oracle(cfg["spec"], cfg["params"], n_threads=8)
    obs = orc.observe()["obs"]
    states = []
    with np.errstate(all="ignore"):
        for t in range(max(POLICY_T)):
            if noise:
                from walker_gym_amd import pg
                u, a, e = pg.stochastic_forward_numpy(pol, obs, gc.sigma_of(case_name), gc.SEED, gc.STEP_BASE + t,
                                                      walker_base=gc.WALKER_BASE)
                out["raw"].append(u); out["eps"].append(e)
            else:
                a = pol.forward_numpy(obs)
            r = ref.step(a)
            obs = r["obs"]
            out["action"].append(a); out["obs"].append(obs.copy()); out["reward"].append(r["reward"].copy())
            out["done"].append(np.asarray(r["done"]).astype(np.uint8))
            st = dict(pos=orc.pos.copy(), vel=orc.vel.copy(), acc=orc.acc.copy(), muscle_x=orc.mx.copy(),
                      steps=orc.steps.copy(), contact=orc.contact.copy())
            if auto_reset:
                out["reset"].append(r["reset"].copy())
                out["steps_t"].append(np.asarray(r["steps_out"]).astype(np.int32))
                fo = np.full_like(obs, np.nan)   # a step writes the rows of the walkers it resets only
                sel = r["reset"] != 0
                fo[sel] = ref.final_obs[sel]
                out["final_obs"].append(fo)
                st["episodes"] = ref.episodes.copy()
            states.append(P._frozen(st))
    res = {k: np.stack(x) for k, x in out.items()}
    res["states"] = states
    res["kinds"] = cfg["kinds"]
    return P._frozen(res)


# ---------------------------------------------------------------- walker_step_waves
WAVE_COPIES = 16  # test_gpu_ragged._wave_spec(ne) that many times over: enough wave tiles for every placement


def wave_tiles(spec):
    """The wave tiles of a mixed batch as the host plans them (layout.size_order's order, wg_plan_waves' greedy
    contiguous packing: 64 masses, 64 * ne springs, 64 muscles, 32 walkers): arrays of caller walker indices, each in
    its stored order, the slots of the tile."""
    from walker_gym_amd import layout
    M = np.diff(np.asarray(spec["mass_off"], np.int64))
    K = np.diff(np.asarray(spec["edge_off"], np.int64))
    A = np.asarray(spec["n_muscles"], np.int64)
    ne = layout.wave_edge_passes(int(M.max()), int(K.max()))
    assert ne > 0
    tiles, cur, use = [], [], [0, 0, 0]
    for w in layout.size_order(spec).tolist():
        m, k, a = int(M[w]), int(K[w]), int(A[w])
        if cur and (use[0] + m > 64 or use[1] + k > 64 * ne or use[2] + a > 64 or len(cur) >= 32):
            tiles.append(np.array(cur))
            cur, use = [], [0, 0, 0]
        cur.append(w)
        use = [use[0] + m, use[1] + k, use[2] + a]
    tiles.append(np.array(cur))
    return tiles


def wave_case(base, in3d, seed, pins=True):
    """WAVE_COPIES copies of a mixed batch with diverged walkers placed by slot of the planned wave tiles: (spec, params,
    kinds, tiles)."""
    from walker_gym_amd.walker import concat_specs
    spec = concat_specs([base] * WAVE_COPIES)
    tiles = wave_tiles(spec)
    out, params, kinds = diverge(spec, in3d, tiles, seed, pins)
    return out, params, kinds, tiles

"""tests/feature_cases.py on the CPU, the reference alone: every (batch, condition, form, mode) cell that
tests/test_gpu_feature_instances.py launches means something.  The statistics use enough rows, the normaliser clips a
share of its inputs (and passes a NaN under `diverged`), the feature and the condition each move the result, the hold
mixes deciding and holding walkers in a wave tile and is cut short by a reset, a dead walker's action is NaN under the
linear policy and a finite constant under the deep one, a NaN action stays in force across a held step, a dead walker
returns to its dead snapshot, the alive walkers stay finite, and a held discrete action moves the muscles.  These are
conditions on the inputs (seeds, weight scales, BOUND), so nothing here can pass or fail with a kernel."""
import numpy as np
import pytest

import diverged_cases as D
import feature_cases as F
import hold_cases as hc
import policy_cases as pc

f32 = np.float32
CELLS = F.cells()
CLIP_SHARE = (0.02, 0.40)


def _differs(a, b):
    return not np.array_equal(np.asarray(a), np.asarray(b).reshape(np.shape(a)), equal_nan=True)


def _cell(cell):
    batch, cond, form, ar = cell
    return batch, cond, form, ar, F.FORMS[form], pc.case_of(batch), F.reference(cell)


def test_the_cells_are_the_issues():
    """240 cells: ten batches, three conditions, four forms, two modes; the T = 1 runs on the stand-in batches; the forms'
    runtime settings."""
    assert len(CELLS) == len(set(CELLS)) == 240 and len({F.cell_id(c) for c in CELLS}) == 240
    assert len(F.BATCHES) == 10 and F.CONDITIONS == ("scaled-run2", "scaled-run2-discrete", "diverged")
    assert {f: (v["noise"], v["every"], v["deep"]) for f, v in F.FORMS.items()} == \
        {"on": (False, 1, False), "on-nz": (True, 1, False), "hold": (True, 2, False), "deep": (True, 3, True)}
    assert sum(len(F.steps_of(c)) for c in CELLS) == 240 + 2 * 4 * 2
    assert all(F.steps_of(c)[0] == (8 if c[3] else 4) for c in CELLS)
    for c in CELLS:
        pol = F.policy_of(*c)
        assert pol.obs_norm is not None and pol.obs_norm.clip == f32(1.5) and pol.G == 1
        assert (pol.H, pol.H2) == ((6, 5) if c[2] == "deep" else (0, 0))


@pytest.mark.parametrize("auto_reset", [False, True], ids=["off", "ar"])
@pytest.mark.parametrize("cond", F.CONDITIONS)
@pytest.mark.parametrize("batch", F.BATCHES)
def test_rows_used_for_the_statistics(batch, cond, auto_reset):
    """Every row under the parameter conditions, at least half of them under `diverged`; finite mean and scale."""
    st, mean, scale, used, rows = F.stats_of(batch, cond, auto_reset)
    assert rows == (1 + F.T[auto_reset]) * len(F.entry_rows(batch, cond, auto_reset))
    assert used == rows if cond != "diverged" else rows // 2 <= used < rows, (used, rows)
    assert np.isfinite(mean).all() and np.isfinite(scale).all() and (scale > 0).all()


@pytest.mark.parametrize("cell", CELLS, ids=F.cell_id)
def test_normaliser_inputs(cell):
    """The share of the finite normalised inputs of the deciding walkers that sit exactly at +-clip; a NaN input under
    `diverged`, none under the parameter conditions."""
    batch, cond, form, ar, f, case, ref = _cell(cell)
    xn = F.normalised_inputs(batch, cond, form, ar, ref)[ref["decided"] != 0]
    fin = np.isfinite(xn)
    share = float((np.abs(xn[fin]) == f32(1.5)).mean())
    assert CLIP_SHARE[0] <= share <= CLIP_SHARE[1], share
    assert np.isnan(xn).any() if cond == "diverged" else fin.all()


@pytest.mark.parametrize("cell", CELLS, ids=F.cell_id)
def test_the_feature_moves_the_result(cell):
    """The action rows against the same cell with the feature off: no normaliser (on, on-nz), every = 1 (hold, deep), the
    linear policy (deep).  Deliberately the first step alone, which asks more than `differs somewhere`: there both runs
    act on the same entry rows, so a difference is the feature's own and not the drift of two diverging rollouts, more
    than a quarter of the walkers must show it, and the feature-off run costs one step."""
    batch, cond, form, ar, f, case, ref = _cell(cell)
    offs = {"on": ("norm",), "on-nz": ("norm",), "hold": ("hold",), "deep": ("hold", "deep")}[form]
    for off in offs:
        other = F.loop(batch, cond, form, ar, Tn=1, off=off)
        assert other["action"].shape[1:] == ref["action"].shape[1:]
        moved = (ref["action"][0] != other["action"][0]) & ~(np.isnan(ref["action"][0]) & np.isnan(other["action"][0]))
        assert moved.any(axis=1).mean() > 0.25, (off, moved.any(axis=1).mean())


@pytest.mark.parametrize("cell", [c for c in CELLS if c[1] != "diverged"], ids=F.cell_id)
def test_the_condition_moves_the_result(cell):
    """param_cases.POLICY_VARIANTS' `moves` against the default parameters on the same spec, policy and normaliser;
    deliberately after the first step alone (both runs start from one state, so what differs is what the parameters
    moved in that step; the two one-step runs are cheap).  The pinned masses do not move; everything stays finite over
    the cell's whole run."""
    import param_cases as P
    batch, cond, form, ar, f, case, ref = _cell(cell)
    one, dflt = F.loop(batch, cond, form, ar, Tn=1), F.loop(batch, cond, form, ar, Tn=1, off="params")
    got = dict(obs=(one["obs"], dflt["obs"]), pos=(one["state"]["pos"], dflt["state"]["pos"]),
               muscle_x=(one["state"]["mx"], dflt["state"]["mx"]))
    for k in P.variant(cond).moves:
        assert _differs(*got[k]), k
    for k in ("obs", "reward", "action", "hold_reward", "held"):
        assert np.isfinite(ref[k]).all(), k
    st = ref["state"]
    assert all(np.isfinite(st[k]).all() for k in ("pos", "vel", "acc", "mx"))
    cfg = F.config(batch, cond, form, ar)
    pin = np.asarray(cfg["spec"]["pinned"]) != 0
    assert pin[:64].any() and pin[-64:].any()   # (a tile is 64 masses)
    if not ar:
        assert np.array_equal(st["pos"][pin], np.asarray(cfg["spec"]["pos"], f32).reshape(-1, 3)[pin])


def _off_grid_after_reset(decided, reset, every):
    """Walkers that reset while a hold is open (the step after the reset is off the grid of their last decision) and
    decide at that step."""
    Tn, N = decided.shape
    found = 0
    for t, w in zip(*np.nonzero(reset[:-1])):
        before = np.flatnonzero(decided[:t + 1, w])
        if len(before) and (t + 1 - before[-1]) % every != 0 and decided[t + 1, w]:
            found += 1
    return found


@pytest.mark.parametrize("cell", [c for c in CELLS if F.FORMS[c[2]]["held"]], ids=F.cell_id)
def test_hold_coverage(cell):
    batch, cond, form, ar, f, case, ref = _cell(cell)
    dec = ref["decided"]
    if case.wpw > 1:
        assert hc.mixed_tile_steps(dec, case.wpw) > 0         # deciding and holding walkers side by side in a wave tile
    else:   # a tile is one walker: the policy is skipped at some (step, tile) and runs at another, at every step
        assert ((dec == 0).any(1) & (dec != 0).any(1)).all()
    assert not dec[0].all()                                  # walkers enter the call inside a hold: `held` is read
    if ar:
        assert _off_grid_after_reset(dec, ref["reset"], f["every"]) >= 1
    if cond == "scaled-run2-discrete":   # the muscles move under an action decided at an earlier step
        A = case.C
        mus = ref["obs"][:, :, -A:]
        held_step = dec[1:] == 0
        if ar:
            held_step &= ref["reset"][1:] == 0
        assert ((mus[1:] != mus[:-1]).any(2) & held_step).any()


DIVERGED = [c for c in CELLS if c[1] == "diverged"]


def _dead_constant(pol, sigma, eps):
    """A deep policy's raw and clipped action for a row whose first hidden vector is all +0 (a NaN row: every unit's
    pre-activation is NaN, the ReLU gives +0, the second hidden vector is relu(bm)): the contract's own arithmetic over
    the output layer."""
    from walker_gym_amd.policy import MLPPolicy
    host = lambda t: None if t is None else t.detach().cpu().numpy()
    bm = np.zeros(pol.H2, f32) if pol.bm is None else host(pol.bm)[0]
    h2 = np.where(bm > 0, bm, f32(0.0)).astype(f32)
    y = MLPPolicy(pol.w2, pol.b2, act_limit=float("inf")).forward_numpy(h2[None])[0]
    u = (y[None, None] + (sigma[0] * eps).astype(f32)).astype(f32)
    L = f32(pol.act_limit)
    return u, np.where(u < -L, -L, np.where(u > L, L, u)).astype(f32), h2


@pytest.mark.parametrize("cell", DIVERGED, ids=F.cell_id)
def test_diverged_cell(cell):
    """The dead walkers' actions (NaN under the linear policy; under the deep one finite and the constant of a NaN row:
    every first-layer unit is +0, so the second hidden vector is relu(bm), not all zero, since cover_policy draws bm, and
    the action is the output layer over it plus the walker's own noise), dead walkers deciding and holding at later
    steps, a NaN action and a NaN hold_reward carried through a held step, a reset into the dead snapshot, finite alive
    walkers, and on the stand-in batches the first step's contact."""
    batch, cond, form, ar, f, case, ref = _cell(cell)
    cfg = F.config(*cell)
    kinds = cfg["kinds"]
    mo = np.asarray(cfg["spec"]["mass_off"], np.int64)
    dead, alive = np.isin(kinds, D.DEAD), kinds == "alive"
    assert dead.sum() >= D.MIN_DEAD and all((kinds == k).sum() >= D.MIN_OTHER for k in D.OTHER)
    dec, act = ref["decided"] != 0, ref["action"]
    dd = dec & dead[None]
    assert dd.any()
    if f["deep"]:   # finite, and the constant of an all-zero first hidden vector plus the walker's own noise
        pol = F.policy_of(*cell)
        u, a, h2 = _dead_constant(pol, F.sigma_of(batch, form), ref["eps"])
        assert (h2 > 0).any()                   # (bm is drawn: the output layer still has work to do)
        assert np.isfinite(act[dd]).all()
        assert np.array_equal(act[dd], a[dd]) and np.array_equal(ref["raw"][dd], u[dd])
        assert _differs(act[dec & alive[None]], a[dec & alive[None]])
    else:           # the NaN row reaches every column of the action
        assert np.isnan(act[dd]).all()
        if f["noise"]:
            assert np.isnan(ref["raw"][dd]).all() and np.isfinite(ref["eps"][dd]).all()
    if f["held"]:
        later_dec, later_held = dd[1:], ~dec[1:] & dead[None]
        assert later_dec.any() and later_held.any()
        if not f["deep"]:   # a NaN action decided in the call stays in force across a held step; so does the NaN sum
            carried = later_held & np.isnan(act[1:]).all(2) & np.isnan(ref["hold_reward"][1:])
            assert carried.any()
            # ... and a dead walker that entered inside a hold still acts on its finite `held` row at step 0
            first = ~dec[0] & dead
            assert first.any() and np.isfinite(act[0][first]).all()
        assert np.isnan(ref["hold_reward"][:, dead]).any()
    if ar:   # a dead walker's counter runs out; its fresh row is the dead snapshot's: NaN in some components only
        rs = (ref["reset"] != 0) & dead[None]
        assert rs.any() and not rs.all()
        rows = ref["obs"][rs]
        assert (np.isnan(rows).any(1) & np.isfinite(rows).any(1)).all()
        assert np.isnan(ref["final_obs"][rs]).any()
    # the alive walkers stay finite
    for k in ("obs", "reward", "action", "hold_reward"):
        assert np.isfinite(ref[k][:, alive]).all(), k
    assert np.isfinite(ref["held"][alive]).all()
    am = np.repeat(alive, np.diff(mo))
    st = ref["state"]
    assert all(np.isfinite(st[k][am]).all() for k in ("pos", "vel", "acc"))
    if batch in F.STAND_IN:   # T = 1: the contact of a dead walker's first step is that of the y it started from
        one = F.reference(cell, Tn=1)
        dm = np.repeat(dead, np.diff(mo))
        start = np.asarray(cfg["spec"]["pos"], f32).reshape(-1, 3)
        with np.errstate(invalid="ignore"):
            below = (start[:, 1] < f32(cfg["params"]["ground"])).astype(np.uint8)
        hit = np.asarray(one["state"]["contact"]).astype(np.uint8)
        assert np.array_equal(hit[dm], below[dm]) and hit[dm].any()

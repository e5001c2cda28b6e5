"""tests/diverged_cases.py on the CPU, oracle only: at every shape and IN3D the cases that
tests/test_gpu_diverged_instances.py launches are what they are meant to be.  A dead walker is NaN in every component
after one step and its contact flags are those of the y it started from (not all zero for the kinds whose NaN spares y);
the other kinds keep the plain path; the contact is back to 0 after the second step; the kinds are there in number and
in every position of a wave tile.  These are conditions on the inputs (the seeds of diverged_cases.SEEDS), so nothing
here can pass or fail with a kernel."""
import numpy as np
import pytest

import diverged_cases as D
import policy_cases as pc


def _walker_all(flag, mo):
    return np.logical_and.reduceat(flag, np.asarray(mo[:-1], np.int64))


def _all_nan(st, mo):
    """Per walker: every component of pos, vel and acc NaN."""
    return _walker_all(np.isnan(st["pos"]).all(1) & np.isnan(st["vel"]).all(1) & np.isnan(st["acc"]).all(1), mo)


def _check_steps(kinds, mo, start, ground, first, second):
    """The issue's conditions on a run's first two states.  Returns the per-mass contact expected of the dead walkers."""
    Ms = np.diff(mo)
    dead = np.isin(kinds, D.DEAD)
    dead_m = np.repeat(dead, Ms)
    nan1 = _all_nan(first, mo)
    assert nan1[dead].all(), "a dead walker is not all NaN after step 1"
    plain = np.isin(kinds, ("part", "dead-pinned"))
    assert not nan1[plain].any(), "a part / dead-pinned walker is all NaN after step 1"
    # inf-up / inf-down: y infinite in every mass makes every spring's dy inf - inf = NaN, so these walkers are all NaN
    # after one step as well, on the plain path: nothing in their starting state is NaN, which is what the kernels'
    # test reads.  Their contact is that of the starting y: none above, every mass below.
    for k, hit in (("inf-up", 0), ("inf-down", 1)):
        m = np.repeat(kinds == k, Ms)
        assert not np.isnan(start[m]).any() and np.isinf(start[m][:, 1]).all() and (first["contact"][m] == hit).all(), k
    with np.errstate(invalid="ignore"):
        below = (start[:, 1] < np.float32(ground)).astype(np.uint8)   # NaN: False
    assert np.array_equal(first["contact"][dead_m], below[dead_m]), "contact of the dead walkers = y_start < ground"
    for k in set(kinds[dead]):
        hit = first["contact"][np.repeat(kinds == k, Ms)]
        assert (hit.any() and not hit.all()) if k in D.CONTACT_DEAD else not hit.any(), k
    assert not second["contact"][dead_m].any(), "contact of the dead walkers is 0 after step 2"
    alive_m = np.repeat(kinds == "alive", Ms)
    assert 0.2 < first["contact"][alive_m].mean() < 0.8 or alive_m.sum() < 200   # the ground is at the median height
    return below


@pytest.mark.parametrize("pins", [None, True], ids=["default", "pins"])
@pytest.mark.parametrize("cell", D.cells(), ids=D.cell_id)
def test_scripted_cell(cell, pins):
    shape, in3d = cell
    if pins and D.pins_of(shape):
        pins = None   # (the same cell: lru_cache shares it)
    ref = D.scripted(shape, in3d, pins)
    kinds, mo = ref["kinds"], ref["mass_off"]
    has_pins = D.pins_of(shape) if pins is None else pins
    kw, wpw = D.SHAPES[shape], D.select(shape)["wpw"]
    N = kw["N"]
    _check_steps(kinds, mo, ref["start"], ref["ground"], ref["steps"][0], ref["steps"][1])
    dead = np.isin(kinds, D.DEAD)
    want_dead = [k for k in D.DEAD if in3d or k != "dead-z"]
    want_other = [k for k in D.OTHER if has_pins or k != "dead-pinned"]
    assert ("dead-pinned" in kinds) == (has_pins and N >= 17) and (in3d or "dead-z" not in kinds)
    if shape not in D.SMALL:
        assert dead.sum() >= D.MIN_DEAD
        for k in want_other + ["alive"]:
            assert (kinds == k).sum() >= D.MIN_OTHER, k
        for k in want_dead:
            assert (kinds == k).sum() >= 2, k
    elif N >= 17:   # m4x17: one of every kind
        assert set(want_dead + want_other + ["alive"]) <= set(kinds)
    else:           # canon5: a mixed group of four and the last walker
        assert dead.sum() == 2 and sorted(kinds[~dead]) == ["alive", "inf-up", "part"]
    # a below-ground NaN-x mass in the first walker of a tile and in the last
    c1 = np.add.reduceat(ref["steps"][0]["contact"].astype(np.int64), np.asarray(mo[:-1], np.int64))
    w = np.flatnonzero((kinds == "dead-x") & (c1 > 0))
    # (the last slot of a full tile; the batch's forced last walker counts only where it closes one)
    assert (w % wpw == 0).any() and (w % wpw == wpw - 1).any()
    assert kinds[N - 1] == "dead-x" and c1[N - 1] > 0
    # every placement (a tile of one walker: groups of four tiles)
    g = wpw if wpw > 1 else 4
    groups = [dead[s:s + g] for s in range(0, N, g)]
    full = [t for t in groups if len(t) == g]
    if shape not in D.SMALL:
        assert any(t[0] and not t[1:].any() for t in full), "first walker alone"
        assert any(t[-1] and not t[:-1].any() for t in full), "last walker alone"
        assert any(t.all() for t in full), "wholly dead"
        assert sum(not t.any() for t in full) >= len(full) // 4, "tiles with none"
        if g > 2:
            assert any((t[::2].all() and not t[1::2].any()) or (t[1::2].all() and not t[::2].any()) for t in full)
    assert any(t.any() and not t.all() for t in groups) or N < 8, "dead beside alive"


def test_the_shapes():
    sel = {s: D.select(s) for s in D.SHAPES}
    assert sel["m8"] == dict(wpw=8, passes=1, compact=True, full=True)
    assert sel["m32"] == dict(wpw=2, passes=2, compact=True, full=True)
    assert sorted({D.SHAPES[s]["M"] for s in D.SHAPES}) == [4, 8, 16, 32, 64]
    # FIX on the full tiles of up to four passes, WT from two (M = 32: 2 x (3 x d x 32 + 8) x 4 B, a multiple of 16)
    assert [s for s in D.SHAPES if D.fix_expected(s)] == ["ne1", "ne2", "ne3", "ne4", "m8", "m32"]
    assert [s for s in D.SHAPES if D.wt_expected(s, 1)] == ["ne2", "ne3", "ne4", "m32"]
    spec = D.base_spec("m8")
    deg = np.bincount(np.concatenate([spec["ei"][:8], spec["ej"][:8]]), minlength=8)
    assert (deg == 2).all()   # the perimeter cycle: every mass has its springs (a dead walker needs one per mass)


@pytest.mark.parametrize("cell", [(s, d) for s in D.FULL for d in (0, 1)], ids=D.cell_id)
def test_auto_reset_cell(cell):
    """Some walkers reset at every step (the sunk ones), dead walkers reset when their counter runs out and are dead
    again: the contact of the step after such a reset is that of the snapshot's y."""
    cfg, steps = D.ar_config(*cell), D.ar_reference(*cell)
    resets = np.stack([s["out"]["reset"] for s in steps])
    dead = np.isin(cfg["kinds"], D.DEAD)
    assert resets[:, cfg["sunk"]].all() and resets.sum() < resets.size
    assert resets[:, dead].any() and not resets[:, dead].all()
    Ms = np.diff(np.asarray(cfg["spec"]["mass_off"]))
    hits = [int(s["state"]["contact"][np.repeat(dead, Ms)].sum()) for s in steps]
    assert hits[0] > 0 and sum(h > 0 for h in hits[1:]) >= 2, hits


@pytest.mark.parametrize("noise", [False, True], ids=["det", "nz"])
@pytest.mark.parametrize("auto_reset", [False, True], ids=["off", "ar"])
@pytest.mark.parametrize("case", pc.COVER, ids=lambda c: c.name)
def test_policy_cell(case, auto_reset, noise):
    """The closed loop: the dead walkers' contact after the first step is that of their starting y (a T = 1 rollout ends
    there), and 0 after the second unless a reset brought the snapshot back."""
    ref, cfg = D.policy_reference(case.name, auto_reset, noise), D.policy_config(case.name, auto_reset)
    kinds = cfg["kinds"]
    mo = np.asarray(cfg["spec"]["mass_off"])
    dead = np.isin(kinds, D.DEAD)
    assert dead.sum() >= D.MIN_DEAD
    for k in D.OTHER:
        assert (kinds == k).sum() >= D.MIN_OTHER
    dm = np.repeat(dead, np.diff(mo))
    first = ref["states"][0]
    start = np.asarray(cfg["spec"]["pos"], np.float32).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        below = (start[:, 1] < np.float32(cfg["params"]["ground"])).astype(np.uint8)
    if not auto_reset:
        assert _all_nan(first, mo)[dead].all()
        assert not ref["states"][1]["contact"][dm].any()
    assert np.array_equal(first["contact"][dm], below[dm]) and first["contact"][dm].any()

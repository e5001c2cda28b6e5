"""tests/param_cases.py on the CPU, oracle only: every (shape, IN3D, variant) cell that tests/test_gpu_param_instances.py
launches moves what its parameters should move (a variant that changes nothing at a shape tests nothing there), stays
finite (all walkers; at least 95 % of them under the pair variants, whose close opposite charges blow some walkers up
in the reference's own arithmetic), and the auto-reset and policy cells roll episodes over."""
import numpy as np
import pytest

import param_cases as P
import policy_cases as pc

STATE = ("pos", "vel", "acc", "muscle_x")
OUT = ("obs", "reward", "done", "centroid", "energy")


def _differs(a, b):
    return not np.array_equal(np.asarray(a), np.asarray(b).reshape(np.shape(a)), equal_nan=True)


def _moved(a, b, ncommon):
    """The arrays in which two runs differ; the rows are compared in their mass columns (conmid shifts the others)."""
    cut = lambda k, x: x[:, :ncommon] if k == "obs" else x
    return [k for k in STATE + OUT if _differs(cut(k, a[k]), cut(k, b[k]))]


def test_the_cells_are_the_issues():
    assert [P.SHAPES[s] for s in P.FULL] == [kw for _, kw in P._PASSES]
    # every instance the shapes are there for, by the restated selection (asserted against launch_geometry() on the GPU)
    sel = {s: P.select(kw["N"], kw["M"], kw["K"]) for s, kw in P.SHAPES.items()}
    assert [sel[s]["passes"] for s in P.FULL] == [1, 2, 3, 4, 5]
    assert all(sel[s]["compact"] and sel[s]["full"] for s in P.FULL)
    assert sel["ne1+1"] == dict(wpw=16, passes=1, compact=True, full=False)
    assert sel["canon+1"] == dict(wpw=4, passes=3, compact=True, full=False)
    assert sel["canon5"] == dict(wpw=1, passes=1, compact=False, full=True)
    assert sel["m4x17"] == dict(wpw=1, passes=1, compact=False, full=True)
    # env-runtime is the one variant lean_fix_ok admits: FIX on the full tiles of up to four passes, WT from two
    for s, kw in P.SHAPES.items():
        for d in (0, 1):
            assert P.fix_expected(kw["N"], kw["M"], kw["K"], True) == (s in P.FULL[:4])
            assert P.wt_expected(kw["N"], kw["M"], kw["K"], kw["A"], d, True) == (s in P.FULL[1:4])
    # run(lanes=2): the M = 64 batches split into two ranges of 256 full one-walker tiles (FIX again), ne1 into two of
    # 4,096 whose tiles are halved (the generic instance on the 16-byte records)
    assert P.run_ranges(512) == [256, 256] and P.run_ranges(8192) == [4096, 4096] and P.run_ranges(17) == [17]
    assert P.select(4096, 4, 4) == dict(wpw=8, passes=1, compact=False, full=True)
    assert len(P.step_cells()) == 116 and len(P.resident_cells()) == 90 and len(P.auto_reset_cells()) == 50
    scales = [P.OBS_SCALED[k] for k in ("pk", "vk", "ak", "mk")]
    assert len(set(scales)) == 4 and all(np.frexp(x)[0] != 0.5 for x in scales)


@pytest.mark.parametrize("cell", P.step_cells(), ids=P.cell_id)
def test_scripted_cell_is_live_and_finite(cell):
    """test_step, test_resident: the scripted steps under the variant against the same spec and actions under the default
    parameters."""
    shape, in3d, name = cell
    v = P.variant(name)
    got, dflt = P.scripted(shape, in3d, name), P.scripted(shape, in3d, name, default=True)
    mo = got["mass_off"]
    for t, (a, b) in enumerate(zip(got["steps"], dflt["steps"])):
        fin = P.finite_walkers(a, mo)
        if v.pairs:
            assert fin.mean() >= 0.95, f"step {t}: {fin.mean():.3f} of the walkers finite"
        else:
            assert fin.all(), f"step {t}: {int((~fin).sum())} walkers not finite"
            assert all(np.isfinite(a[k]).all() for k in OUT)
        d, M = (3 if in3d else 2), P.SHAPES[shape]["M"]
        moved = _moved(a, b, 3 * d * M)
        if name == "obs-mid2":   # the three conmid columns hold the position sums
            assert a["obs"].shape[1] == b["obs"].shape[1] + 3 and (a["obs"][:, 3 * d * M:3 * d * M + 3] != 0).all()
        for k in v.moves:
            if k == "done" and t == 0 and name == "env-runtime":
                continue   # (checked below: some, not all)
            assert k in moved, f"step {t}: {k} does not move"
        if v.moves == ("obs",):
            assert moved == ["obs"], f"step {t}: {moved} move"
    if name == "env-runtime":
        d0, d1 = got["steps"][0]["done"], got["steps"][1]["done"]
        assert 0 < d0.sum() < d0.size, "done_y ends some walkers at step 1, not all"
        assert d1.all() and not dflt["steps"][1]["done"].any(), "max_steps ends every walker at step 2"
    if got["pinned"] is not None:
        pin = got["pinned"] != 0
        wpw = P.select(**{k: P.SHAPES[shape][k] for k in "NMK"})["wpw"]
        M = P.SHAPES[shape]["M"]
        assert 0.02 < pin.mean() < 0.1 or pin.size < 200
        assert pin[:wpw * M].any() and pin[-((P.SHAPES[shape]["N"] - 1) % wpw + 1) * M:].any()
        for a in got["steps"]:
            assert np.array_equal(a["pos"][pin], got["start"][pin])
        assert _differs(got["steps"][-1]["pos"][~pin], got["start"][~pin])
    if name == "discrete":
        acts = P.actions(shape, name, P.RUN_STEPS)
        assert set(np.unique(acts)) == {0.0, 1.0}


@pytest.mark.parametrize("cell", P.auto_reset_cells(), ids=P.cell_id)
def test_auto_reset_cell_rolls_over(cell):
    """test_auto_reset: every walker resets at least once, not all of them at every step, the sunk ones at every step (so
    both noise rows are drawn); the reference stays finite."""
    steps = P.ar_reference(*cell)
    cfg = P.ar_config(*cell)
    resets = np.stack([s["out"]["reset"] for s in steps])
    assert (resets.sum(0) >= 1).all() and resets.sum() < resets.size
    assert resets[:, cfg["sunk"]].all()
    assert (np.stack([s["state"]["episodes"] for s in steps]).max() >= 2)
    for s in steps:
        assert all(np.isfinite(s["state"][k]).all() for k in ("pos", "vel", "acc", "mx", "final_obs"))
        assert all(np.isfinite(s["out"][k]).all() for k in OUT)


@pytest.mark.parametrize("auto_reset", [False, True], ids=["off", "ar"])
@pytest.mark.parametrize("name", [v.name for v in P.POLICY_VARIANTS])
@pytest.mark.parametrize("case", pc.COVER, ids=lambda c: c.name)
def test_policy_cell_is_live_and_finite(case, name, auto_reset):
    """test_policy_rollout: finite, the pinned masses at rest (auto-reset off), resets (on), and the combined variant
    differs from the default-parameter closed loop of the same batch in obs, pos (and muscle_x when discrete)."""
    ref = P.policy_reference(case.name, name, auto_reset)
    for k in ("action", "obs", "reward"):
        assert np.isfinite(ref[k]).all(), k
    st = ref["state"]
    assert all(np.isfinite(st[k]).all() for k in ("pos", "vel", "acc", "mx"))
    pin = ref["pinned"] != 0
    assert pin[:64].any() and pin[-64:].any()   # (a tile is 64 masses)
    if auto_reset:
        assert (ref["reset"].sum(0) >= 1).all() and ref["reset"].sum() < ref["reset"].size
    else:
        assert np.array_equal(st["pos"][pin], ref["start"][pin])
        dflt = pc.oracle_rollout(case.name)
        assert _differs(ref["obs"], dflt["obs"]) and _differs(st["pos"], dflt["pos"])
        if P.variant(name).discrete:
            assert _differs(st["mx"], dflt["muscle_x"])
            assert (ref["action"] != 0).any()

"""bench.py's plain run: `--steps` sets the timed steps, `--dump-outputs` writes what the last of them returned, and what
stands beside the headline (`sustained`, the controls, the CPU baseline) is measured only with `--full`."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N, K, W = 256, 8, 2
NAMES = ("obs", "reward", "done", "centroid_position", "total_energy", "steps")


def test_options_default_off():
    import bench
    a = bench.parse([])
    assert a.full is False and a.dump_outputs is None
    a = bench.parse(["--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d"


@pytest.mark.gpu
@pytest.mark.parametrize("resident_steps,max_steps,episode_steps,sample_rows",
                         [(None, None, None, None), (3, None, None, None), (3, 5, None, None), (None, None, 5, None),
                          (None, None, None, 100)])
def test_plain_run_dumps_last_timed_step(tmp_path, monkeypatch, capsys, resident_steps, max_steps, episode_steps,
                                         sample_rows):
    """A plain two-range run of K steps after W, in this process: the dumped arrays are bit for bit what
    BatchedPhysicsEnv.run leaves after the same sequence on the same seeded inputs (the same kernels: this checks the
    bench's sequencing and its dump, not the physics).  resident_steps = 3: only 3 distinct action steps fit
    ACT_BYTES_MAX, so the K = 8 region takes actions 0 1 2 0 1 2 0 1.  max_steps = 5 / episode_steps = 5
    (EPISODE_STEPS, max_steps at its default): an episode, 5 steps from the initial state with the warm-up's 2, ends
    inside the region, so after 3 timed steps the walkers return to the initial state and take the last 5 from there.
    sample_rows = 100: DUMP_BYTES_MAX holds 100 walkers' rows, so every array keeps the same seeded 100 walkers."""
    import torch
    import bench
    from walker_gym_amd.batched_env import BatchedPhysicsEnv
    spec, params = bench.make_spec("canonical", N, seed=1000)
    if max_steps is not None:
        params = dict(params, max_steps=max_steps)
        monkeypatch.setattr(bench, "make_spec", lambda *a, **k: (spec, params))
    if episode_steps is not None:
        monkeypatch.setattr(bench, "EPISODE_STEPS", episode_steps)
    dev = torch.device("cuda", 0)
    ref = BatchedPhysicsEnv(spec, device=dev, **params)
    A = ref.batch.A
    if resident_steps is not None:
        monkeypatch.setattr(bench, "ACT_BYTES_MAX", resident_steps * N * A * 4)
    row_bytes = 4 * (ref.obs_dim + 1 + 1 + 3 + 1 + 1)   # obs, reward, done, centroid_position, total_energy, steps
    if sample_rows is not None:
        monkeypatch.setattr(bench, "DUMP_BYTES_MAX", sample_rows * row_bytes)
    out = tmp_path / "dump"
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", str(K), "--warmup", str(W), "--walkers", str(N),
                                      "--lanes", "2", "--dump-outputs", str(out)])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    bench.main()
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["steps"] == K and line["warmup"] == W and line["config"]["lanes"] == 2
    assert line["ms_per_step"] > 0 and line["unit"] == "env-steps/s" and line["higher_is_better"] is True
    # (ms_per_step is rounded to 1e-5 ms: half a unit of that on a step of >= 2 us is 2.5e-3)
    assert line["ms_per_step"] >= 2e-3
    assert line["value"] == pytest.approx(N * 1e3 / line["ms_per_step"], rel=3e-3)
    for key in ("sustained", "closed_loop", "closed_loop_policy", "cpu_baseline", "floor"):
        assert key not in line, key
    H = min(64 if episode_steps is None else episode_steps, 1000 if max_steps is None else max_steps)
    split = H < W + K
    assert line["episodes"]["steps"] == H and line["episodes"]["restores_in_timed_steps"] == int(split)

    # the same inputs: bench.py's generator, the warm-up actions drawn first
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    acts_w = (torch.rand((W, N, A), generator=gen, device=dev) * 2 - 1).contiguous()
    T = K if resident_steps is None else resident_steps
    acts = (torch.rand((T, N, A), generator=gen, device=dev) * 2 - 1).contiguous()
    seq = acts[torch.arange(K, device=dev) % T].contiguous()
    start = ref.batch.state_dict()
    ref.run(acts_w, W, lanes=2)
    if not split:
        ref.run(seq, K, lanes=2)
    else:
        first = H - W
        ref.run(seq[:first].contiguous(), first, lanes=2)
        ref.batch.load_state_dict(start)
        ref.run(seq[first:].contiguous(), K - first, lanes=2)
    torch.cuda.synchronize()
    info = ref.info()
    want = {"obs": ref.obs, "reward": ref.reward, "done": ref.done, "centroid_position": info["centroid_position"],
            "total_energy": info["total_energy"], "steps": info["steps"]}
    rows = np.arange(N)
    if sample_rows is not None:
        rows = np.sort(np.random.default_rng(0).choice(N, sample_rows, replace=False))
    assert sorted(os.listdir(out)) == sorted(f"{n}.npy" for n in NAMES)
    total = 0
    for name in NAMES:
        got = np.load(out / f"{name}.npy")
        exp = want[name].cpu().numpy().astype(np.float32)[rows]
        total += got.nbytes
        assert got.dtype == np.float32 and got.shape == exp.shape, name
        assert np.array_equal(got, exp, equal_nan=True), name
    assert total == len(rows) * row_bytes
    assert np.all(np.load(out / "steps.npy") == (K - (H - W) if split else W + K))

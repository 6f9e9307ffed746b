"""bench.py is the driver-facing benchmark contract: one JSON line with
the documented schema, runnable on CPU with small sizes. The headline
measures the BASELINE metric (wall-clock to the reference convergence
criterion on the shipped datasets); here we exercise the identical code
path on the small shipped smallGrid3D dataset so the CPU test stays
fast."""
import json
import os
import subprocess
import sys

import pytest


def test_bench_json_contract():
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run(
        [sys.executable, os.path.join(here, "bench.py"),
         "--steps", "3", "--warmup", "1", "--dataset", "smallGrid3D",
         "--agents", "4"],
        capture_output=True, text=True, timeout=600, cwd=here)
    assert out.returncode == 0, out.stderr[-2000:]
    line = out.stdout.strip().splitlines()[-1]
    o = json.loads(line)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup",
                "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config"):
        assert key in o, f"missing {key}"
    assert o["metric"] == "smallGrid3D_wall_to_gradnorm_0.1_s"
    assert o["steps"] == 3
    assert o["higher_is_better"] is False
    assert o["scaling"] == "strong"
    assert o["dtype"] == "fp64"
    assert o["value"] > 0
    assert o["config"]["converged"] is True
    assert o["config"]["iterations"] > 0
    # deterministic episodes: warmup episode matches the timed ones
    assert all(w == o["config"]["iterations"]
               for w in o["config"]["warmup_iterations"])
    # --steps is the number of timed episodes, ms_per_step one of them
    assert len(o["config"]["episode_times_s"]) == 3
    assert o["ms_per_step"] == pytest.approx(o["value"] * 1e3)


def test_bench_dump_outputs_reproducible(tmp_path):
    """--dump-outputs writes the last timed episode's outputs as float64
    .npy files; the inputs are fixed, so a second run (here with --full,
    which must not change the headline path) reproduces them. Pinned to
    the CPU path, whose arithmetic is bitwise-deterministic (the GPU
    kernels reduce with fp64 atomics, so there only to rounding)."""
    import numpy as np
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    runs = []
    for name, extra in (("a", []), ("b", ["--full"])):
        d = tmp_path / name
        out = subprocess.run(
            [sys.executable, os.path.join(here, "bench.py"),
             "--steps", "1", "--warmup", "1", "--dataset", "smallGrid3D",
             "--agents", "4", "--device", "cpu",
             "--dump-outputs", str(d)] + extra,
            capture_output=True, text=True, timeout=600, cwd=here)
        assert out.returncode == 0, out.stderr[-2000:]
        o = json.loads(out.stdout.strip().splitlines()[-1])
        arrs = {f[:-4]: np.load(str(d / f)) for f in sorted(os.listdir(d))}
        runs.append((o, arrs))
    o, arrs = runs[0]
    assert sorted(arrs) == ["X", "trace", "trajectory"]
    n, iters = o["config"]["poses"], o["config"]["iterations"]
    assert arrs["trace"].shape == (iters, 2)
    assert arrs["X"].shape == (n, 4, 5)
    assert arrs["trajectory"].shape == (3, 4 * n)
    assert all(a.dtype == np.float64 and np.all(np.isfinite(a))
               for a in arrs.values())
    assert sum(a.nbytes for a in arrs.values()) <= 64 * 2 ** 20
    # the dump is what the result line reports
    assert arrs["trace"][-1, 0] == o["config"]["final_cost"]
    assert arrs["trace"][-1, 1] == o["config"]["final_gradnorm"]
    # every pose was written: lifted rotation blocks are orthonormal
    Y = arrs["X"][:, :3, :]
    assert np.allclose(Y @ Y.transpose(0, 2, 1), np.eye(3), atol=1e-9)
    for k in arrs:
        assert np.array_equal(arrs[k], runs[1][1][k]), k

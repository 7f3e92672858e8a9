"""Run each example end-to-end with tiny budgets (mirrors the reference's
tests/test_examples.py integration strategy)."""

import os
import subprocess
import sys
import tempfile

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CASES = [
    ("examples/rastrigin_snes.py", ["--generations", "3"]),
    ("examples/cartpole_gymne.py", ["--generations", "3"]),
    ("examples/parallel_cpu_actors.py", ["--generations", "2", "--popsize", "8"]),
    ("examples/multiobjective_nsga2.py", []),
    ("examples/mapelites_illumination.py", []),
    ("examples/functional_api_batched.py", []),
    ("examples/synthetic_humanoid_pgpe.py", ["--generations", "2", "--popsize", "16", "--device", "cpu"]),
    ("examples/mnist30k_distributed.py", ["--generations", "1", "--popsize", "8"]),
    ("examples/genetic_programming.py", ["--generations", "5", "--popsize", "64"]),
    ("examples/checkpoint_resume.py", []),
    ("examples/lennard_jones_cmaes.py", ["--generations", "30"]),
    ("examples/mpc_cem_pendulum.py", ["--steps", "90"]),
    ("examples/vqe_snes.py", ["--generations", "250"]),
]


@pytest.mark.parametrize("script,args", CASES, ids=[c[0] for c in CASES])
def test_example_runs(script, args, tmp_path):
    # An example that writes a fixed name into the system temp dir gets a
    # private one, instead of meeting a file another user left there. It sits
    # directly under the system temp dir, not under tmp_path: multiprocessing
    # binds AF_UNIX sockets below TMPDIR, and their paths are limited to ~100
    # characters.
    with tempfile.TemporaryDirectory(prefix="ex") as private_tmp:
        result = subprocess.run(
            [sys.executable, os.path.join(REPO, script), *args],
            cwd=tmp_path,  # checkpoints etc. land in a temp dir
            env={**os.environ, "TMPDIR": private_tmp},
            capture_output=True,
            text=True,
            timeout=420,
        )
    assert result.returncode == 0, f"{script} failed:\n{result.stderr[-2000:]}"


def test_bench_json_contract():
    """bench.py must print ONE JSON line with the driver-contract fields
    (metric/value/unit/n_gpus/steps/warmup/ms_per_step/higher_is_better/
    scaling/vs_baseline/dtype/data/config) — run tiny on CPU."""
    import json

    out = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), "--steps", "1", "--warmup", "0",
         "--popsize", "8", "--episode-length", "5"],
        capture_output=True, text=True, timeout=600,
    )
    assert out.returncode == 0, out.stderr[-2000:]
    line = out.stdout.strip().splitlines()[-1]
    d = json.loads(line)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
                "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
        assert key in d, f"missing {key}"
    assert d["steps"] == 1 and d["warmup"] == 0
    assert d["value"] > 0 and d["ms_per_step"] > 0
    assert d["scaling"] in ("weak", "strong")
    assert isinstance(d["config"], dict) and "model" in d["config"]


def test_bench_dump_outputs_reproducible(tmp_path):
    """--dump-outputs writes the last timed step's outputs as float .npy
    arrays; the same arguments give the same inputs, so two runs agree
    exactly on CPU. --full is accepted and keeps the result line."""
    import json

    import numpy as np

    dumps = []
    for name, extra in (("a", []), ("b", ["--full"])):
        out = subprocess.run(
            [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
             "--popsize-per-gpu", "16", "--episode-length", "5", "--dump-outputs", str(tmp_path / name), *extra],
            capture_output=True, text=True, timeout=600,
        )
        assert out.returncode == 0, out.stderr[-2000:]
        d = json.loads(out.stdout.strip().splitlines()[-1])
        assert d["steps"] == 2 and d["ms_per_step"] > 0
        files = sorted(os.listdir(tmp_path / name))
        assert files == ["center.npy", "fitnesses.npy", "mean_eval.npy", "stdev.npy"]
        dumps.append({f: np.load(tmp_path / name / f) for f in files})
    a, b = dumps
    assert a["center.npy"].shape == (6409,) and a["stdev.npy"].shape == (6409,)
    assert a["fitnesses.npy"].shape == (16,) and a["mean_eval.npy"].shape == ()
    for f in a:
        assert a[f].dtype in (np.float32, np.float64)
        assert np.isfinite(a[f]).all()
        assert np.array_equal(a[f], b[f]), f
    assert sum(arr.nbytes for arr in a.values()) <= 64 * 1024 * 1024

"""bench.py's contract when no measurement is possible (CPU box, too few devices): ONE JSON line with an `error` field and
a non-zero exit code -- never a bare exit (`python bench.py --gpus 8` used to return rc 1 and print
nothing).  The self-launching N > 1 path itself needs a GPU: tests/test_gpu_ddp.py::test_bench_self_launch_clean_env."""
import json
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-device behaviour")
@pytest.mark.parametrize("gpus", [1, 8])
def test_bench_without_devices_prints_an_error_line(gpus):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(gpus), "--steps", "20", "--warmup", "5"], env=env,
                       capture_output=True, timeout=300)
    assert r.returncode != 0
    lines = [l for l in r.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout.decode()
    d = json.loads(lines[0])
    assert d["value"] is None and d["n_gpus"] == gpus and "error" in d and d["devices_visible"] == 0
    assert d["metric"].startswith("clips/s") and d["steps"] == 20 and d["warmup"] == 5


def test_bench_world_size_mismatch_is_reported():
    """started by a launcher whose WORLD_SIZE disagrees with --gpus: an error line from rank 0, not a hang or a bare exit"""
    env = dict(os.environ, RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29999")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4", "--steps", "2", "--warmup", "1"], env=env,
                       capture_output=True, timeout=300)
    assert r.returncode != 0
    lines = [l for l in r.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1 and "WORLD_SIZE" in json.loads(lines[0])["error"]


@pytest.mark.skipif(torch.cuda.is_available(), reason="checks the no-device behaviour")
def test_bench_sweep_prints_one_line_per_gpu_count():
    """`--sweep-gpus 1,2,4,8`: one child per N, one JSON line per N in order (here: error lines, no device) and a non-zero exit."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--sweep-gpus", "1,2,4,8", "--steps", "3", "--warmup", "1"], env=env,
                       capture_output=True, timeout=600)
    assert r.returncode != 0
    lines = [json.loads(l) for l in r.stdout.decode().splitlines() if l.startswith("{")]
    assert [d["n_gpus"] for d in lines] == [1, 2, 4, 8] and all(d["value"] is None and "error" in d and d["steps"] == 3 for d in lines)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--sweep-gpus", "1,x"], env=env, capture_output=True, timeout=300)
    assert r.returncode == 2 and "comma-separated" in json.loads(r.stdout.decode().strip().splitlines()[-1])["error"]


def test_instrumented_steps_stay_away_from_the_barrier():
    """bench.profiled_steps: one timed step in ten carries per-launch events, never step 0 of a run with more than one step (it
    starts on an empty queue and its first brackets would carry the host's launch latency)"""
    import bench
    assert list(bench.profiled_steps(20)) == [5, 15]
    assert list(bench.profiled_steps(5)) == [4] and list(bench.profiled_steps(2)) == [1] and list(bench.profiled_steps(1)) == [0]
    assert len(bench.profiled_steps(400)) == 40 and 0 not in bench.profiled_steps(400)


def test_bench_rejects_a_step_count_below_one():
    """--steps is the number of timed steps the line's ms_per_step divides by: 0 is an error line, not a division by zero"""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "0", "--warmup", "1"],
                       capture_output=True, timeout=300)
    assert r.returncode == 2
    lines = [l for l in r.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1 and "--steps" in json.loads(lines[0])["error"]


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_same_outputs_every_run(tmp_path):
    """A plain `bench.py --gpus 1 --steps K --warmup W` times K steps and prints the headline only (none of what --full adds);
    --dump-outputs DIR writes the last timed step's loss / parameters / gradients as float32 .npy (a fixed sample of the 86 M
    parameters, under 64 MB in all), and two runs with the same arguments write the same arrays."""
    import numpy as np
    import bench
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    dumps = []
    for run in range(2):
        out_dir = tmp_path / f"run{run}"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--batch", "4",
                            "--dump-outputs", str(out_dir)], env=env, capture_output=True, timeout=600)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        lines = [json.loads(l) for l in r.stdout.decode().splitlines() if l.startswith("{")]
        assert len(lines) == 1
        d = lines[0]
        assert "error" not in d and d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0
        assert d["value"] == pytest.approx(4 * 1e3 / d["ms_per_step"], rel=1e-3)          # clips/s of the 3 timed steps
        assert not {"roofline", "attention", "frontend", "scaling_model", "cpu_baseline", "cpu_baseline_forward",
                    "parity_mode_clips_s", "allreduce_measured"} & set(d)
        arrays = {n: np.load(str(out_dir / f"{n}.npy")) for n in ("loss", "params", "grads")}
        assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
        assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
        assert arrays["params"].shape == arrays["grads"].shape == (bench.DUMP_SAMPLE,)
        assert arrays["loss"].shape == (1,) and float(arrays["loss"][0]) == pytest.approx(d["loss"], abs=1e-6)
        assert np.abs(arrays["grads"]).max() > 0
        dumps.append(arrays)
    for n in ("loss", "params", "grads"):
        a, b = dumps[0][n], dumps[1][n]
        assert np.abs(a - b).max() <= 1e-5 * np.abs(a).max(), n

"""bench.py --gpus N started WITHOUT torch.distributed.run must start its N ranks itself (as a child process, before anything
touches the GPU) and relay rank 0's JSON line: a driver that runs `python bench.py --gpus 8` gets an 8-rank measurement."""

import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

REPO = Path(__file__).resolve().parent.parent


def run_bench(args, env_extra=None, timeout=600):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(env_extra or {})
    p = subprocess.run([sys.executable, str(REPO / "bench.py")] + args, capture_output=True, text=True, timeout=timeout, env=env, cwd=str(REPO))
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, f"exactly one JSON line expected, got {len(lines)}: {p.stdout[-500:]}"
    return json.loads(lines[0])


def test_self_launch_starts_two_ranks_dry_run():
    """No GPU needed: rendezvous on 127.0.0.1 over gloo, one all-reduce, rank 0's line."""
    r = run_bench(["--gpus", "2", "--dry-run", "--steps", "1", "--warmup", "0"])
    assert r["n_gpus"] == 2 and r["dry_run"] is True


def test_single_rank_dry_run_does_not_spawn():
    r = run_bench(["--gpus", "1", "--dry-run"])
    assert r["n_gpus"] == 1


@pytest.mark.gpu
def test_self_launch_two_ranks_on_one_gpu():
    """Two ranks sharing the one GPU of the box (MZ_BENCH_BACKEND=gloo): the real step incl. the overlapped gather of outputs."""
    r = run_bench(["--gpus", "2", "--workload", "cfg2", "--images-per-gpu", "2", "--steps", "1", "--warmup", "1", "--full", "--no-cpu-baseline",
                   "--no-microbench"], {"MZ_BENCH_BACKEND": "gloo"})
    assert r["n_gpus"] == 2 and r["value"] > 0
    assert r["config"]["global_batch"] == 4
    assert r["value_without_gather"] is not None and r["value_without_gather"] > 0
    assert "bf16" in r["config"]["workload"]


def test_bad_arguments_are_refused_before_any_work():
    for args in (["--steps", "0"], ["--dump-launches", "x.csv"]):
        p = subprocess.run([sys.executable, str(REPO / "bench.py")] + args, capture_output=True, text=True, timeout=120, cwd=str(REPO))
        assert p.returncode == 2 and "error" in p.stderr, (args, p.stderr[-500:])


def test_dump_outputs_writes_float32_and_samples_large_outputs(tmp_path, monkeypatch):
    sys.path.insert(0, str(REPO))
    import bench

    monkeypatch.setattr(bench, "DUMP_VALUES", 100)
    big = torch.arange(1000, dtype=torch.float64).reshape(10, 100)  # value == flat position
    small = torch.linspace(0, 1, 60).to(torch.bfloat16).reshape(3, 4, 5)
    bench.dump_outputs(tmp_path / "a", {"big": big, "small": small})
    bench.dump_outputs(tmp_path / "b", {"big": big})
    got = np.load(tmp_path / "a" / "big.npy")
    assert got.dtype == np.float32 and got.shape == (100,)
    assert np.array_equal(got // 10, np.arange(100)), "one position in each of the 100 equal slices"
    assert np.array_equal(got, np.load(tmp_path / "b" / "big.npy")), "the sample positions must not change from run to run"
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float32 and np.array_equal(s, small.float().numpy())


@pytest.mark.gpu
def test_plain_run_dumps_what_the_last_timed_step_computed(tmp_path):
    """A plain run reports the --steps it timed and carries none of the --full legs; --dump-outputs holds the output of the timed path on
    the benchmark's seeded inputs (here sampled: 2 images of 1080x1920 exceed the dump's limit), equal to upscale() of the same inputs."""
    r = run_bench(["--workload", "cfg2", "--images-per-gpu", "2", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path)])
    assert r["steps"] == 3 and r["ms_per_step"] > 0 and r["value"] > 0 and r["dtype"] == "bf16"
    assert not {"roofline", "cpu_baseline", "secondary"} & set(r)
    got = np.load(tmp_path / "upscale.npy")
    assert got.dtype == np.float32 and got.nbytes <= 64 << 20

    sys.path.insert(0, str(REPO))
    import bench

    cfg = bench.MODELS["2x48"]
    m = bench.MewZoom(**cfg)
    m.load_state_dict(bench.synth_weights(bench.parameter_shapes(cfg), seed=1234))
    m = m.to("cuda:0", torch.bfloat16).eval()
    want = m.upscale(bench.synth_image(2, 540, 960, seed=1000).to("cuda:0", torch.bfloat16))
    bench.dump_outputs(tmp_path / "want", {"upscale": want})
    assert np.array_equal(got, np.load(tmp_path / "want" / "upscale.npy"))

"""CPU: bench.py's step counts and its --dump-outputs files (what two builds are compared by)."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
import bench  # noqa: E402


@pytest.mark.parametrize("flags", [["--steps", "0"], ["--warmup", "-1"]])
def test_step_counts_out_of_range_are_refused(flags):
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), *flags], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and flags[0] in r.stderr, r.stderr


def test_dump_outputs_writes_float32_npy_and_keeps_the_budget(tmp_path):
    x = torch.randn(1, 16, 5, 32, 32, generator=torch.Generator().manual_seed(0))
    bench.dump_outputs(tmp_path / "out", {"latents": x})
    a = np.load(tmp_path / "out" / "latents.npy")
    assert a.dtype == np.float32 and np.array_equal(a, x.numpy())
    with pytest.raises(SystemExit, match="budget"):
        bench.dump_outputs(tmp_path / "big", {"latents": torch.zeros(bench.DUMP_MAX_BYTES // 4 + 1)})
    assert not (tmp_path / "big").exists()


def test_plain_run_makes_no_measurement_beside_its_steps():
    """Without --full nothing runs beside the warm-up and timed steps, whatever else is asked for: the CPU baseline, the
    secondary workloads and the extras all sit behind the option."""
    for argv in ([], ["--gpus", "1", "--steps", "20", "--warmup", "5"], ["--dump-outputs", "out"],
                 ["--workload", "K5"], ["--depth", "2"], ["--no-extras", "--no-cpu-baseline", "--no-k3p"]):
        args = bench.parse(argv)
        assert args.full is False
        assert not any(bench.untimed_legs(args, rank=0, world=1).values()), argv
    # a leg that only a --full run has is not dropped in silence
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--full-tta-leg"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 2 and "--full" in r.stderr, r.stderr


def test_full_run_keeps_every_leg_and_its_opt_outs():
    legs = lambda argv, rank=0, world=1: bench.untimed_legs(bench.parse(argv), rank, world)
    everything = {"cpu_baseline": True, "secondary": True, "k3p": True, "extras": True, "full_tta": False}
    assert legs(["--full"]) == everything
    assert legs(["--full", "--full-tta-leg"]) == dict(everything, full_tta=True)
    assert legs(["--full", "--no-cpu-baseline"]) == dict(everything, cpu_baseline=False)
    assert legs(["--full", "--no-k3p"]) == dict(everything, k3p=False)
    assert legs(["--full", "--no-extras", "--full-tta-leg"]) == dict.fromkeys(everything, False) | {"cpu_baseline": True}
    assert legs(["--full", "--workload", "K5"]) == dict(everything, secondary=False, k3p=False)     # secondaries belong to K3
    assert legs(["--full", "--depth", "2"]) == dict(everything, k3p=False, extras=False)            # the 48-block legs
    # more than one GPU: the denoise step alone, on every rank
    for rank in (0, 1):
        assert not any(legs(["--full", "--gpus", "2"], rank, 2).values())


def test_full_reaches_the_ranks_of_a_multi_gpu_launch():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "2", "--full", "--dry-launch"],
                       capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split()[-3:] == ["--gpus", "2", "--full"]

"""CPU: bench.py's step counts and its --dump-outputs files (what two builds are compared by)."""
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

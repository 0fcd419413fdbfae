"""GPU: the bits of the default denoise update.  lcv_cfg_euler_step and lcv_euler_step, called through the C ABI on inputs from
a seeded numpy generator, leave exactly the bytes recorded in tests/golden/cfg_euler_bits.json: the SHA-256 of `x` after the call
and, where zero-star is on, of the [B, 256, 2] partial sums.  No tolerance: test_gpu_kernel_edges.py holds the same two entry
points to 2 ulps of a float64 restatement, this file holds them to what they computed before the guidance math moved into
csrc/cfg_guidance.h.

The sizes: a single lane, a ragged wave, exactly one workgroup and one element past it, exactly one pass of the partial kernel's
stride (256 x 256) and one element past it, and a second trip of the step kernel's grid-stride loop (its grid is capped at
1024 workgroups of 256).

The golden file was written by this same file in record mode (LCV_RECORD_CFG_EULER_BITS=1) on a build of the commit before that
move (profiles/denoise_step_unify.md names it).  It is never rewritten from a later tree."""
import functools
import hashlib
import json
import os
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / "golden" / "cfg_euler_bits.json"
RECORD = os.environ.get("LCV_RECORD_CFG_EULER_BITS", "") == "1"
DEV = "cuda"
SEED = 20240607
BATCHES = (1, 2)
SIZES = (1, 7, 256, 257, 65536, 65537, 262147)
GUIDANCE, DT = 3.7, -0.0213          # neither is a power of two: every product rounds


def _call(name, *args):
    from lcv_hip import lib
    lib.call(name, *args, torch.cuda.current_stream().cuda_stream)


@functools.lru_cache(maxsize=None)
def _inputs(B, n):
    """(cond, uncond, x0) fp32 [B, n] on the device; uncond leans on cond so that the zero-star ratio is no accident of noise."""
    rng = np.random.default_rng([SEED, B, n])
    c = rng.standard_normal((B, n), dtype=np.float32)
    u = (rng.standard_normal((B, n), dtype=np.float32) * np.float32(0.8) + np.float32(0.3) * c).astype(np.float32)
    x = rng.standard_normal((B, n), dtype=np.float32)
    return tuple(torch.from_numpy(a).to(DEV) for a in (c, u, x))


def _sha(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.cpu().contiguous().numpy().tobytes()).hexdigest()


def _check(case, got):
    if RECORD:
        golden = json.loads(GOLDEN.read_text()) if GOLDEN.exists() else {}
        golden[case] = got
        GOLDEN.write_text("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(golden[k])}" for k in sorted(golden)) + "\n}\n")
    assert got == json.loads(GOLDEN.read_text())[case], case


def _cfg_cases():
    return [(B, n, zs, neg) for B in BATCHES for n in SIZES for zs in (0, 1) for neg in (0, 1)]


def _euler_cases():
    return [(n, neg) for n in SIZES for neg in (0, 1)]


@pytest.mark.parametrize("B,n,zero_star,negate", _cfg_cases())
def test_cfg_euler_step_bits(B, n, zero_star, negate):
    c, u, x0 = _inputs(B, n)
    x = x0.clone()
    ws = torch.full((B, 256, 2), float("nan"), dtype=torch.float32, device=DEV)
    _call("lcv_cfg_euler_step", c.data_ptr(), u.data_ptr(), x.data_ptr(), ws.data_ptr(), B, n, GUIDANCE, DT, negate, zero_star)
    got = {"x": _sha(x)}
    if zero_star:
        got["ws"] = _sha(ws)
    _check(f"cfg-B{B}-n{n}-zs{zero_star}-neg{negate}", got)


@pytest.mark.parametrize("n,negate", _euler_cases())
def test_euler_step_bits(n, negate):
    c, _, x0 = _inputs(1, n)
    x = x0.clone()
    _call("lcv_euler_step", c.data_ptr(), x.data_ptr(), n, DT, negate)
    _check(f"euler-n{n}-neg{negate}", {"x": _sha(x)})


def test_the_golden_file_holds_exactly_these_cases():
    want = [f"cfg-B{B}-n{n}-zs{zs}-neg{neg}" for B, n, zs, neg in _cfg_cases()] + [f"euler-n{n}-neg{neg}" for n, neg in _euler_cases()]
    assert sorted(json.loads(GOLDEN.read_text())) == sorted(want)

"""CPU: the numpy restatement of the LoRA dropout mask reproduces the published Philox4x32-10 known-answer vectors;
include/lcv_hip_lora.h is held to the rules the other headers are held to (every declared symbol exported and bound, nothing
undeclared in the table, nothing of it in the main header); the new wrappers refuse CPU tensors."""
import ctypes
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import lora_dropout_ref as R

ROOT = Path(__file__).resolve().parents[1]
HEADER = "lcv_hip_lora.h"
HOST_ONLY = {"lcv_tn_skinny_dropout_ws_bytes"}


def _declared(header: str):
    txt = (ROOT / "include" / header).read_text()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(lcv_[a-z0-9_]+)\s*\(", txt))


def _built():
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as ge
    ge.build()
    from lcv_hip import lib
    return lib, ctypes.CDLL(str(lib.lib_path()))


@pytest.mark.parametrize("ctr, key, want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(ctr, key, want):
    got = R.philox4x32_10(key, ctr)
    assert " ".join(f"{int(w):08x}" for w in got) == want


def test_mask_layout_thresholds_and_slices():
    assert R.threshold(0.1) == 6554 and R.threshold(0.5) == 32768 and R.threshold(0.25) == 16384
    assert R.threshold(1e-9) == 1 and R.threshold(1 - 1e-9) == 65535
    assert R.scale(0.5) == np.float32(2.0)
    # element e of group g is a 16-bit half of word e >> 1 of the block at counter (offset, g): low half for even e
    seed, offset, K = (5 << 32) | 1234, (1 << 32) | 8, 24
    m = R.mask(3, K, 0.5, seed, offset, row0=2)
    g = (2 + 1) * K // 8 + 2                                   # row 1 of the slice, third group
    w = R.philox4x32_10((1234, 5), (8, 1, g, 0))
    halves = [(int(w[e >> 1]) >> (16 * (e & 1))) & 0xFFFF for e in range(8)]
    assert m[1, 16:24].tolist() == [int(h >= 32768) for h in halves]
    # rows [a, b) with row0 = a are that slice of the full mask, also past 2^32 groups
    full = R.mask(9, K, 0.1, 7, 4)
    assert np.array_equal(R.mask(4, K, 0.1, 7, 4, row0=5), full[5:9])
    big = 1 << 33
    assert np.array_equal(R.mask(2, K, 0.1, 7, 4, row0=big + 1), R.mask(3, K, 0.1, 7, 4, row0=big)[1:])
    assert not np.array_equal(R.mask(2, K, 0.1, 7, 4, row0=big), R.mask(2, K, 0.1, 7, 4, row0=0))


@pytest.mark.parametrize("seed, offset, p", [(1234, 0, 0.1), (1234, 4, 0.5), (7, 8, 0.25)])
def test_restated_keep_rate(seed, offset, p):
    n = 256 * 4096
    q = 1 - R.threshold(p) / 65536
    kept = int(R.mask(256, 4096, p, seed, offset).sum())
    assert abs(kept - n * q) <= 4 * (n * q * (1 - q)) ** 0.5


def test_lora_header_symbols_are_exported_and_bound():
    lib, so = _built()
    names = _declared(HEADER)
    assert len(names) == 5, names
    missing = [n for n in names if not hasattr(so, n)]
    assert not missing, f"declared in {HEADER} but not exported: {missing}"
    assert names == set(lib._SIGNATURES_LORA) | HOST_ONLY, names ^ (set(lib._SIGNATURES_LORA) | HOST_ONLY)
    for other in (lib._SIGNATURES, lib._SIGNATURES_LPIPS, lib._SIGNATURES_DET):
        assert not set(lib._SIGNATURES_LORA) & set(other)
    # the main header's closed list is untouched
    assert not _declared("lcv_hip.h") & names
    assert HEADER not in (ROOT / "include" / "lcv_hip.h").read_text()
    so.lcv_version.restype = ctypes.c_int
    assert so.lcv_version() >= 4                      # went up with the new entry points
    q = so.lcv_tn_skinny_dropout_ws_bytes
    q.restype = ctypes.c_int64
    q.argtypes = [ctypes.c_int64] * 3
    t = so.lcv_tn_skinny_ws_bytes
    t.restype = ctypes.c_int64
    t.argtypes = [ctypes.c_int64] * 3
    for shape in ((37, 520, 1), (37, 4096, 32), (6240, 4096, 8), (25200, 12288, 8)):
        assert q(*shape) == t(*shape) > 0             # the workspace contract of lcv_tn_skinny
    assert q(0, 4096, 8) == 0


def test_every_lora_entry_point_has_a_kernel_level_test():
    import ast
    tests = {"lcv_lora_down_dropout": "test_lora_down_dropout", "lcv_tn_skinny_dropout": "test_tn_skinny_dropout",
             "lcv_lora_dx_dropout_add": "test_lora_dx_dropout_add", "lcv_lora_dropout_mask": "test_mask_equals_the_restatement"}
    assert set(tests) | HOST_ONLY == _declared(HEADER)
    tree = ast.parse((ROOT / "tests" / "test_gpu_lora_dropout.py").read_text())
    assert set(tests.values()) <= {n.name for n in ast.walk(tree) if isinstance(n, ast.FunctionDef)}


def test_the_source_uses_no_atomics_and_reads_no_environment():
    """csrc/lora.hip holds the plain and the masked adapter kernels.  Atomics: only in the body of the one publish function,
    which is called from one place, under the compile-time condition "no mask" - so no masked instantiation contains it."""
    csrc = ROOT / "longcat-video-tta_amd" / "csrc"
    src = (csrc / "lora.hip").read_text() + (csrc / "philox.h").read_text()
    assert "lcv_knob(" not in src and "getenv(" not in src and "asm" not in src
    publish = "tn_skinny_publish_atomic"
    code = " ".join(re.sub(r"//[^\n]*", "", src).split())          # comments may speak of atomics; code may not
    define = re.search(r"void %s\([^)]*\) \{[^{}]*\}" % publish, code)
    assert define and "atomicAdd(" in define.group(0)
    rest = code.replace(define.group(0), "")
    assert rest.count(publish) == 1, "the publish function is called from exactly one place"
    assert re.search(r"if constexpr \(sizeof\.\.\.\(D\) == 0\) \{? ?%s\(" % publish, rest), "not under the no-mask condition"
    assert "atomic" not in rest.replace(publish, "").lower()
    # one definition of each shared piece under csrc/, and none of them left in the files they came from
    everything = {p.name: p.read_text() for p in [*csrc.glob("*.hip"), *csrc.glob("*.h")]}
    for pattern in (r"void lora_down_kernel\(", r"void tn_skinny_kernel\(", r"void tn_skinny_reduce_kernel\(",
                    r"int64_t tn_skinny_rpb\(", r"define TN_MAXROWS\b"):
        homes = {name: len(re.findall(pattern, text)) for name, text in everything.items() if re.search(pattern, text)}
        assert homes == {"lora.hip": 1}, (pattern, homes)
    for old_home in ("gemm.hip", "elementwise_bwd.hip"):
        for word in ("lora_down", "tn_skinny", "TN_MAXROWS"):
            assert word not in everything[old_home], (old_home, word)
    assert not (csrc / "lora_dropout.hip").exists()


def test_new_ops_refuse_cpu_tensors():
    from lcv_hip import ops
    from lcv_hip.lib import LcvError
    bf = torch.bfloat16
    x, A, g = torch.zeros(4, 16, dtype=bf), torch.zeros(2, 16, dtype=bf), torch.zeros(4, 64, dtype=bf)
    with pytest.raises(LcvError, match="GPU"):
        ops.lora_down_dropout(x, A, 2.0, 0.1, 1, 0)
    with pytest.raises(LcvError, match="GPU"):
        ops.tn_skinny_dropout(g, x, 2, 0.1, 1, 0)
    with pytest.raises(LcvError, match="GPU"):
        ops.lora_dx_dropout_add(x.clone(), g, A, 0.1, 1, 0)
    with pytest.raises(LcvError, match="GPU"):
        ops.lora_dropout_mask(4, 16, 0.1, 1, 0, device="cpu")


def test_training_forward_with_dropout_refuses_cpu_tensors():
    from lcv_hip.lib import LcvError
    from tta.lora import LoRALinear
    m = LoRALinear(torch.nn.Linear(16, 8), rank=2, dropout=0.25).to(torch.bfloat16).train()
    with pytest.raises(LcvError, match="GPU"):
        m(torch.zeros(3, 16, dtype=torch.bfloat16))

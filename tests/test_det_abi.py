"""CPU: include/lcv_hip_det.h is held to the rules the other headers are held to (tests/test_lpips_abi.py): every declared
symbol is exported by the built library, the declared set equals the deterministic ctypes table plus the host-only names,
every entry point with a kernel behind it names a GPU test that exists, nothing of it appears in the main header, the new
source file reads no knob or environment variable and uses no float atomic, and the workspace sizes meet their cap."""
import ast
import ctypes
import re
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
TESTS = ROOT / "tests"
HEADER = "lcv_hip_det.h"

KERNEL_TESTS = {
    "lcv_det_adaln_modulate_bwd": [("test_gpu_deterministic_kernels.py", "test_det_adaln_modulate_bwd")],
    "lcv_det_layernorm_affine_bwd": [("test_gpu_deterministic_kernels.py", "test_det_layernorm_affine_bwd")],
    "lcv_det_gate_residual_bwd": [("test_gpu_deterministic_kernels.py", "test_det_gate_residual_bwd"),
                                  ("test_gpu_deterministic_kernels.py", "test_det_gate_residual_bwd_refuses_what_it_does_not_take")],
    "lcv_det_qknorm_rope_bwd": [("test_gpu_deterministic_kernels.py", "test_det_qknorm_rope_bwd")],
    "lcv_det_linear_f32_smallm_bwd": [("test_gpu_deterministic_kernels.py", "test_det_linear_f32_smallm_bwd")],
    "lcv_det_grad_norm_clip": [("test_gpu_deterministic_kernels.py", "test_det_grad_norm_clip_one_tensor"),
                               ("test_gpu_deterministic_kernels.py", "test_det_grad_norm_clip_700_tensors"),
                               ("test_gpu_deterministic_kernels.py", "test_det_grad_norm_clip_bf16_gradient_at_an_odd_address")],
}
HOST_ONLY = {"lcv_det_ws_bytes": "size"}
ADALN, LAYERNORM, GATE, QKNORM, SMALLM, GRAD_NORM = range(6)


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


def test_det_header_symbols_are_exported_and_bound():
    lib, so = _built()
    names = _declared(HEADER)
    assert len(names) == 7 and all(n.startswith("lcv_det_") for n in names), names
    missing = [n for n in names if not hasattr(so, n)]
    assert not missing, f"declared in {HEADER} but not exported: {missing}"
    assert names == set(lib._SIGNATURES_DET) | set(HOST_ONLY), names ^ (set(lib._SIGNATURES_DET) | set(HOST_ONLY))
    assert not set(lib._SIGNATURES_DET) & set(lib._SIGNATURES)
    assert not set(lib._SIGNATURES_DET) & set(lib._SIGNATURES_LPIPS)
    # each takes its counterpart's argument list plus (ws, ws_bytes) in front of the stream; qknorm drops dw_slots
    P, I64 = ctypes.c_void_p, ctypes.c_int64
    for name, sig in lib._SIGNATURES_DET.items():
        base = list(lib._SIGNATURES[name.replace("lcv_det_", "lcv_")])
        if name == "lcv_det_qknorm_rope_bwd":
            assert base[-2] is I64
            del base[-2]
        assert sig == base[:-1] + [P, I64] + base[-1:], name
    # the main header's closed list is untouched
    assert not _declared("lcv_hip.h") & names
    assert HEADER not in (ROOT / "include" / "lcv_hip.h").read_text()
    so.lcv_version.restype = ctypes.c_int
    assert so.lcv_version() >= 3                      # went up with the new entry points


def test_every_det_entry_point_has_a_kernel_level_test():
    declared = _declared(HEADER)
    assert not set(KERNEL_TESTS) & set(HOST_ONLY)
    assert set(KERNEL_TESTS) | set(HOST_ONLY) == declared
    cache = {}
    for name, tests in KERNEL_TESTS.items():
        assert tests, name
        for fname, fn in tests:
            if fname not in cache:
                tree = ast.parse((TESTS / fname).read_text())
                cache[fname] = {n.name for n in ast.walk(tree) if isinstance(n, ast.FunctionDef)}
            assert fn in cache[fname], f"{name}: {fname}::{fn} does not exist"


def test_no_knob_no_environment_read_and_no_float_atomic_in_the_source():
    src = (ROOT / "longcat-video-tta_amd" / "csrc" / "reduce_det.hip").read_text()
    assert "lcv_knob(" not in src and "getenv(" not in src and "atomicAdd" not in src


def test_workspace_sizes_meet_their_cap_and_are_zero_for_empty_shapes():
    _, so = _built()
    q = so.lcv_det_ws_bytes
    q.restype = ctypes.c_int64
    q.argtypes = [ctypes.c_int] + [ctypes.c_int64] * 3
    # the DiT's width at K3-TTA: 7 latent frames of 3 600 tokens = 25 200 tokens, C = 4 096, H = 32 heads of 128
    frames, S, C, H = 7, 3600, 4096, 32
    act = frames * S * C * 2                          # bytes of the bf16 activation the kernel reads (x, y, or q_in)
    for kind, dims in ((ADALN, (frames, S, C)), (LAYERNORM, (frames * S, C, 0)), (GATE, (frames, S, C)), (QKNORM, (1, frames * S, 0))):
        b = q(kind, *dims)
        assert 0 < b <= act // 8, (kind, b, act // 8)
    assert H * 128 == C
    # exact values: one 2C-float (C-float) row per 64 (32) rows of a frame, the last block of a frame ragged
    assert q(ADALN, 2, 50, 128) == 2 * 1 * 2 * 128 * 4 and q(ADALN, 1, 65, 8) == 2 * 2 * 8 * 4
    assert q(LAYERNORM, 300, 4096, 0) == 5 * 2 * 4096 * 4
    assert q(GATE, 6, 50, 520) == 6 * 2 * 520 * 4
    assert q(QKNORM, 2, 300, 0) == 600 * 256 * 4
    assert q(SMALLM, 17, 300, 512) == 2 * 17 * 512 * 4
    # the grad-norm workspace: 4 bytes per 2 048-element chunk (a 45 M-element weight: 22 000 chunks)
    assert q(GRAD_NORM, 22000, 0, 0) == 88000
    for kind, dims in ((ADALN, (0, 50, 128)), (ADALN, (2, 0, 128)), (ADALN, (2, 50, 0)), (LAYERNORM, (0, 128, 0)),
                       (GATE, (0, 1, 8)), (QKNORM, (0, 5, 0)), (QKNORM, (5, 0, 0)), (SMALLM, (0, 4, 4)), (SMALLM, (4, 0, 4)),
                       (SMALLM, (4, 4, 0)), (GRAD_NORM, (0, 0, 0))):
        assert q(kind, *dims) == 0, (kind, dims)
    assert q(99, 1, 1, 1) == -1

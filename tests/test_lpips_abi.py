"""CPU: include/lcv_hip_lpips.h is held to the rules the main header is held to (tests/test_abi_and_host.py,
tests/test_kernel_ref.py): every declared symbol is exported by the built library, the declared set equals the LPIPS
ctypes table plus the host-only names, every entry point with a kernel behind it names a GPU test that exists, and the
new entry points stay out of the main header."""
import ast
import ctypes
import re
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
TESTS = ROOT / "tests"

# entry point -> the kernel-level GPU tests that compare it with the torch restatement
KERNEL_TESTS = {
    "lcv_lpips_pack_weight": [("test_gpu_lpips.py", "test_pack_weight_layout")],
    "lcv_lpips_conv_relu": [("test_gpu_lpips.py", "test_conv_relu_layers_match_float64_conv2d"),
                            ("test_gpu_lpips.py", "test_first_layer_scales_the_frames_in_its_loader")],
    "lcv_lpips_maxpool": [("test_gpu_lpips.py", "test_maxpool_is_exact")],
    "lcv_lpips_tap_distance": [("test_gpu_lpips.py", "test_tap_distance_matches_restatement")],
}
HOST_ONLY = {"lcv_lpips_ws_bytes": "size"}


def _declared(header: str):
    txt = (ROOT / "include" / header).read_text()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(lcv_[a-z0-9_]+)\s*\(", txt))


def test_lpips_header_symbols_are_exported_and_bound():
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as ge
    ge.build()
    from lcv_hip import lib
    so = ctypes.CDLL(str(lib.lib_path()))
    names = _declared("lcv_hip_lpips.h")
    assert len(names) >= 5 and all(n.startswith("lcv_lpips_") for n in names)
    missing = [n for n in names if not hasattr(so, n)]
    assert not missing, f"declared in lcv_hip_lpips.h but not exported: {missing}"
    assert names == set(lib._SIGNATURES_LPIPS) | set(HOST_ONLY), names ^ (set(lib._SIGNATURES_LPIPS) | set(HOST_ONLY))
    assert not set(lib._SIGNATURES_LPIPS) & set(lib._SIGNATURES)
    # the main header's closed list is untouched: nothing of LPIPS is declared or called there
    assert not _declared("lcv_hip.h") & names
    assert "lcv_hip_lpips.h" not in (ROOT / "include" / "lcv_hip.h").read_text()
    so.lcv_version.restype = ctypes.c_int
    assert so.lcv_version() >= 2                      # went up with the new entry points
    # host-only size query: regions of whole 256-byte blocks, zero below the smallest legal frame
    so.lcv_lpips_ws_bytes.restype = ctypes.c_int64
    so.lcv_lpips_ws_bytes.argtypes = [ctypes.c_int64] * 3
    assert so.lcv_lpips_ws_bytes(1, 30, 40) == 0 and so.lcv_lpips_ws_bytes(1, 40, 30) == 0 and so.lcv_lpips_ws_bytes(0, 64, 64) == 0
    b = so.lcv_lpips_ws_bytes(1, 31, 31)
    want = sum((4 * n + 255) // 256 * 256 for n in (2 * 49 * 64, 2 * 9 * 64, 2 * 9 * 192, 2 * 192, 2 * 384, 2 * 256, 2 * 256, 64))
    assert b == want
    taps_480 = 2 * (119 * 207 * 64 + 59 * 103 * (64 + 192) + 29 * 51 * (192 + 384 + 256 + 256))
    assert 4 * taps_480 <= so.lcv_lpips_ws_bytes(1, 480, 832) < 4 * taps_480 + 8 * 256


def test_every_lpips_entry_point_has_a_kernel_level_test():
    declared = _declared("lcv_hip_lpips.h")
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


def test_no_new_library_knob_and_no_forbidden_environment_read():
    src = (ROOT / "longcat-video-tta_amd" / "csrc" / "lpips.hip").read_text()
    assert "lcv_knob(" not in src and "getenv(" not in src

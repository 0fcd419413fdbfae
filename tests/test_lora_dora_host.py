"""CPU: the numpy restatement of the DoRA kernels (tests/dora_ref.py) has the properties include/lcv_hip_dora.h states;
the header is held to the rules the other headers are held to; the module, the loop and the runner take `dora=` /
`dora_magnitudes=` / `--lora-dora`, refuse what they must, and hold nothing new when it is off.  On the parent commit the
flag, the arguments and the header do not exist."""
import argparse
import ctypes
import importlib.util
import inspect
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import dora_ref as D

ROOT = Path(__file__).resolve().parents[1]
PKG = ROOT / "longcat-video-tta_amd"
HEADER = "lcv_hip_dora.h"
NAMES = {"lcv_dora_weight_norm", "lcv_dora_colscale_fwd", "lcv_dora_colscale_bwd"}
SIZES = {"lcv_dora_colscale_bwd_ws_bytes"}
U = 2.0 ** -24


def _bf16(rng, *shape, scale=1.0):
    return D.bf16_rne((rng.standard_normal(shape) * scale).astype(np.float32))


# ------------------------------------------------------------------------------------------------------------ the restatement
def test_bf16_rounding_is_to_nearest_even():
    x = np.array([1.0, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -3.0, 0.0], dtype=np.float32)
    assert D.bf16_rne(x).tolist() == [1.0, 1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, -3.0, 0.0]
    t = torch.randn(4096, generator=torch.Generator().manual_seed(1))
    assert np.array_equal(D.bf16_rne(t.numpy()), t.to(torch.bfloat16).float().numpy())


def test_m_equal_to_wn_gives_a_scale_of_exactly_one():
    rng = np.random.default_rng(2)
    W, A = _bf16(rng, 20, 520), _bf16(rng, 4, 520, scale=520 ** -0.5)
    m = D.weight_norm(W)
    for s in (2.0, -2.0):
        wn = D.weight_norm(W, A, np.zeros((20, 4), dtype=np.float32), s)
        assert np.array_equal(m.view(np.uint32), wn.view(np.uint32))         # B = 0: the adapter term adds nothing, to the bit
    assert (D.col_scale(m, m) == 1).all()
    pre = _bf16(rng, 70, 20)
    assert np.array_equal(D.colscale_fwd(pre, m, m), pre)                    # c == 1: the bias-free forward is the identity
    dy = _bf16(rng, 70, 20)
    assert np.array_equal(D.colscale_bwd(dy, pre, m, m)[0], dy)


def test_the_norm_is_within_the_running_sum_bound_of_float64():
    rng = np.random.default_rng(3)
    for K, R in ((64, 1), (520, 8), (4104, 32)):
        W, A, B = _bf16(rng, 9, K), _bf16(rng, R, K, scale=K ** -0.5), _bf16(rng, 9, R, scale=0.1)
        exact = np.linalg.norm(W.astype(np.float64) + 2.0 * (B.astype(np.float64) @ A.astype(np.float64)), axis=1)
        got = D.weight_norm(W, A, B, 2.0)
        assert got.dtype == np.float32
        assert (np.abs(got - exact) / exact).max() <= 2 * (K + 2 * R + 8) * U


def test_a_zero_norm_gives_a_zero_scale_and_a_zero_magnitude_gradient():
    rng = np.random.default_rng(4)
    wn = np.array([0.0, 2.0, 0.0, 0.5], dtype=np.float32)
    m = np.array([1.0, 1.0, 0.0, 3.0], dtype=np.float32)
    assert D.col_scale(m, wn).tolist() == [0.0, 0.5, 0.0, 6.0]
    pre, dy, bias = _bf16(rng, 5, 4), _bf16(rng, 5, 4), _bf16(rng, 4)
    y = D.colscale_fwd(pre, m, wn, bias)
    assert np.array_equal(y[:, 0], bias[[0] * 5]) and np.isfinite(y).all()
    dpre, dm = D.colscale_bwd(dy, pre, m, wn)
    assert (dpre[:, [0, 2]] == 0).all() and dm[0] == 0 and dm[2] == 0 and dm[1] != 0 and np.isfinite(dm).all()


@pytest.mark.parametrize("M", [1, 15, 16, 17, 63, 64, 65, 257, 513])
def test_the_slab_sum_is_within_M_ulps_of_the_float64_sum(M):
    rng = np.random.default_rng(M)
    prod = _bf16(rng, M, 24) * _bf16(rng, M, 24)                              # exact in fp32
    got = D.slab_sum(prod)
    assert got.dtype == np.float32
    p64 = prod.astype(np.float64)
    err = np.abs(got - p64.sum(0)) / np.abs(p64).sum(0)
    assert err.max() <= M * U, err.max()
    # the order is the stated one: per slab of 64 rows four quarters of 16 from row 0, ((q0 + q1) + q2) + q3, then the slabs
    want = np.zeros(24, dtype=np.float32)
    for r0 in range(0, M, 64):
        q = [_in_order(prod[a:min(a + 16, M)]) for a in range(r0, r0 + 64, 16)]
        want = want + (((q[0] + q[1]) + q[2]) + q[3])
    assert np.array_equal(got, want)


def _in_order(rows):
    p = np.zeros(24, dtype=np.float32)
    for row in rows:
        p = p + row
    return p


# ----------------------------------------------------------------------------------------------------------- header and binding
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


def test_dora_header_symbols_are_exported_and_bound_in_a_table_of_their_own():
    lib, so = _built()
    assert _declared(HEADER) == NAMES | SIZES
    assert not [n for n in NAMES | SIZES if not hasattr(so, n)]
    assert set(lib._SIGNATURES_DORA) == NAMES
    txt = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / HEADER).read_text(), flags=re.S)
    for n in NAMES:
        args = re.search(rf"\bint {n}\s*\(([^)]*)\)", txt).group(1)
        assert len(lib._SIGNATURES_DORA[n]) == len(args.split(",")), n
        assert args.split(",")[-1].strip() == "void* stream", n
    for other in sorted((ROOT / "include").glob("*.h")):
        if other.name != HEADER:
            assert not _declared(other.name) & (NAMES | SIZES), other.name
    assert HEADER not in (ROOT / "include" / "lcv_hip.h").read_text()
    for table_name in [k for k in vars(lib) if k.startswith("_SIGNATURES") and k != "_SIGNATURES_DORA"]:
        assert not set(getattr(lib, table_name)) & NAMES, table_name
    so.lcv_version.restype = ctypes.c_int
    assert so.lcv_version() >= 15                     # went up with the new entry points
    loaded = lib.load()
    for n in NAMES:
        assert getattr(loaded, n).argtypes == lib._SIGNATURES_DORA[n] and getattr(loaded, n).restype is ctypes.c_int
    assert loaded.lcv_dora_colscale_bwd_ws_bytes.restype is ctypes.c_int64
    assert loaded.lcv_dora_colscale_bwd_ws_bytes(65, 8) == 2 * 8 * 4 and loaded.lcv_dora_colscale_bwd_ws_bytes(0, 8) < 0
    # the header's tile constants are the ones the binding and the restatement carry
    for name, value in (("LCV_DORA_NORM_KTILE", D.KTILE), ("LCV_DORA_NORM_ROWS", D.ROWS), ("LCV_DORA_SLAB", D.SLAB),
                        ("LCV_DORA_SLAB_QUARTER", D.QUARTER)):
        assert re.search(rf"#define {name} (\d+)", (ROOT / "include" / HEADER).read_text()).group(1) == str(value)
        assert getattr(lib, name) == value


def test_the_source_is_built_without_contraction_and_uses_no_atomics():
    from lcv_hip import build
    src = (PKG / "csrc" / "dora.hip").read_text()
    assert build.EXTRA["dora.hip"] == ["-ffp-contract=off"] == build.EXTRA["optim_ema.hip"]
    code = re.sub(r"//[^\n]*", "", src)
    for word in ("atomic", "asm", "getenv", "lcv_knob(", "hipMalloc"):
        assert word not in code, word
    assert '#include "lcv_hip_dora.h"' in src
    for entry in NAMES:
        assert len(re.findall(rf'extern "C" int {entry}\(', src)) == 1, entry


def test_every_entry_point_has_a_kernel_level_test():
    txt = (ROOT / "tests" / "test_gpu_lora_dora.py").read_text()
    for n in NAMES:
        assert f'lib.call("{n}"' in txt, n                                    # the bad-argument cases
    for wrapper in ("ops.dora_weight_norm(", "ops.dora_colscale_fwd(", "ops.dora_colscale_bwd("):
        assert wrapper in txt


def test_new_ops_refuse_cpu_tensors():
    from lcv_hip import ops
    from lcv_hip.lib import LcvError
    bf = torch.bfloat16
    w, m = torch.zeros(8, 16, dtype=bf), torch.ones(16)
    with pytest.raises(LcvError, match="GPU"):
        ops.dora_weight_norm(w)
    with pytest.raises(LcvError, match="GPU"):
        ops.dora_colscale_fwd(w, m, m)
    with pytest.raises(LcvError, match="GPU"):
        ops.dora_colscale_bwd(w, w.clone(), m, m)


# ------------------------------------------------------------------------------------------------------------------ the module
def _linear():
    return torch.nn.Linear(32, 24)


def test_without_dora_the_module_holds_nothing_new():
    from tta import lora as L
    plain, off = L.LoRALinear(_linear(), rank=4), L.LoRALinear(_linear(), rank=4, dora=False)
    names = [n for n, _ in plain.named_parameters()]
    assert names == [n for n, _ in off.named_parameters()] == ["original.weight", "original.bias", "lora_down.weight", "lora_up.weight"]
    assert not hasattr(off, "dora_magnitude") and L.get_dora_magnitudes([plain, off]) == []
    assert L.count_lora_parameters([off]) == {"total_lora": 32 * 24 + 24 + 4 * 32 + 24 * 4, "trainable": 4 * 32 + 24 * 4}
    assert [p.shape for p in L.get_lora_parameters([off])] == [(4, 32), (24, 4)]
    assert inspect.signature(L.LoRALinear.__init__).parameters["dora"].default is False
    assert inspect.signature(L.inject_lora_into_dit).parameters["dora"].default is False


def test_saved_keys_gain_magnitudes_only_with_dora(tmp_path):
    from tta import lora as L
    off, on = L.LoRALinear(_linear(), rank=4), L.LoRALinear(_linear(), rank=4, dora=True)
    L.save_lora_weights([off, off], str(tmp_path / "off.pt"))
    assert sorted(torch.load(tmp_path / "off.pt")) == ["lora_0.down", "lora_0.up", "lora_1.down", "lora_1.up"]
    L.save_lora_weights([off, on], str(tmp_path / "on.pt"))
    state = torch.load(tmp_path / "on.pt")
    assert sorted(state) == ["lora_0.down", "lora_0.up", "lora_1.down", "lora_1.magnitude", "lora_1.up"]
    assert state["lora_1.magnitude"].dtype == torch.float32 and state["lora_1.magnitude"].shape == (24,)
    counts = L.count_lora_parameters([off, on])
    assert counts["dora_magnitude"] == 24 and counts["trainable"] == 2 * (4 * 32 + 24 * 4) + 24


def test_the_magnitude_stays_fp32_and_keeps_its_bits_through_a_cast():
    from lcv_hip.lib import LcvError
    from tta import lora as L
    on = L.LoRALinear(_linear(), rank=4, dora=True)
    value = torch.full((24,), 1.3) + torch.arange(24) * 2.0 ** -20             # not bf16 numbers
    with torch.no_grad():
        on.dora_magnitude.copy_(value)
    param = on.dora_magnitude
    on = on.to(dtype=torch.bfloat16)
    assert on.dora_magnitude is param and param.dtype == torch.float32 and torch.equal(param.detach(), value)
    assert on.lora_down.weight.dtype == torch.bfloat16 and on.original.weight.dtype == torch.bfloat16
    assert L.get_dora_magnitudes([on]) == [param] and param.requires_grad
    assert [n for n, _ in on.named_parameters()][0] == "dora_magnitude"
    assert all(p is not param for p in L.get_lora_parameters([on]))           # the bf16 adapters only
    with pytest.raises(LcvError):                                             # no CPU path, and no silent one
        on(torch.zeros(2, 32, dtype=torch.bfloat16))


# ------------------------------------------------------------------------------------------------------- the loop and the runner
def _runner():
    spec = importlib.util.spec_from_file_location("run_lora_tta_amd_dora_host", PKG / "lora_experiment" / "scripts" / "run_lora_tta.py")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


BASE = ["--checkpoint-dir", "synthetic:2:256:64", "--data-dir", "synthetic:1", "--output-dir", "unused"]


def test_the_flag_is_off_by_default_and_parses():
    m = _runner()
    assert m.parse_args(BASE).lora_dora is False
    assert m.parse_args(BASE + ["--lora-dora"]).lora_dora is True
    args = m.parse_args(BASE + ["--lora-dora", "--lora-dropout", "0.1", "--aug-enabled"])      # what it composes with
    assert args.lora_dora and args.lora_dropout == 0.1


@pytest.mark.parametrize("extra, word", [
    (["--use-builtin-lora"], "--use-builtin-lora"), (["--master-weights"], "--master-weights"),
    (["--stochastic-rounding"], "--stochastic-rounding"),
    (["--master-weights", "--adam-8bit"], "--master-weights"), (["--master-weights", "--grad-accum", "2"], "--master-weights"),
    (["--master-weights", "--weight-ema", "0.9"], "--master-weights")])
def test_the_runner_refuses_the_combinations_from_the_command_line(extra, word):
    m = _runner()
    with pytest.raises(ValueError, match=f"--lora-dora cannot be combined with {word}"):
        m.parse_args(BASE + ["--lora-dora"] + extra)
    assert m.parse_args(BASE + extra).lora_dora is False                      # without the flag they stay legal


@pytest.mark.parametrize("field, value, word", [
    ("use_builtin_lora", True, "--use-builtin-lora"), ("master_weights", True, "--master-weights"), ("adam_8bit", True, "--adam-8bit"),
    ("grad_accum", 2, "--grad-accum"), ("weight_ema", 0.9, "--weight-ema"), ("stochastic_rounding", True, "--stochastic-rounding")])
def test_every_refusal_on_its_own_and_before_any_model_is_loaded(field, value, word):
    m = _runner()
    args = m.parse_args(BASE + ["--lora-dora"])
    setattr(args, field, value)
    with pytest.raises(ValueError, match=f"--lora-dora cannot be combined with {word}"):
        m.check_lora_dora_args(args)
    with pytest.raises(ValueError, match=word):
        m.lora_method(args)                                                   # the job's entry checks too: nothing is loaded yet
    args.lora_dora = False
    m.check_lora_dora_args(args)


class _TinyDit(torch.nn.Module):
    def __init__(self):
        super().__init__()
        blk = torch.nn.Module()
        blk.attn = torch.nn.Module()
        blk.attn.qkv, blk.attn.proj = torch.nn.Linear(16, 48), torch.nn.Linear(16, 16)
        self.blocks = torch.nn.ModuleList([blk])


@pytest.mark.parametrize("flag", [False, True])
def test_config_json_records_the_flag_and_the_injection_follows_it(flag):
    from tta import lora as L
    m = _runner()
    args = m.parse_args(BASE + (["--lora-dora"] if flag else []) + ["--lora-rank", "2"])
    dit = _TinyDit()
    cfg = m.lora_method(args).prepare(dit)
    mods = [x for x in dit.modules() if isinstance(x, L.LoRALinear)]
    assert len(mods) == 2 and all(x.dora is flag for x in mods)
    assert cfg["lora"].get("dora", False) is flag and ("dora" in cfg["lora"]) is flag
    assert cfg["lora"]["trainable_params"] == 2 * (16 + 48) + 2 * (16 + 16) + (48 + 16 if flag else 0)
    assert len(L.get_dora_magnitudes(mods)) == (2 if flag else 0)


def test_the_loops_take_the_magnitudes_and_refuse_before_building_anything():
    from tta import inner_loop as IL
    for fn in (IL.finetune_lora_on_conditioning, IL.finetune_lora_batch):
        assert inspect.signature(fn).parameters["dora_magnitudes"].default is None
    mags = [torch.nn.Parameter(torch.ones(4))]
    dit = argparse.Namespace(_sp_group=None)
    assert IL._dora_optimizer(dit, None, 1e-3, master_weights=True) is None   # no magnitudes: nothing to refuse
    for kw in ({"master_weights": True}, {"moments_8bit": True}, {"grad_accum > 1": True}, {"weight_ema": True},
               {"stochastic_rounding": True}):
        with pytest.raises(ValueError, match="DoRA magnitudes cannot be combined with " + re.escape(next(iter(kw)))):
            IL._dora_optimizer(dit, mags, 1e-3, **kw)
    with pytest.raises(ValueError, match="sequence parallelism"):
        IL._dora_optimizer(argparse.Namespace(_sp_group=(None,)), mags, 1e-3)
    with pytest.raises(ValueError, match="fp32"):
        IL._dora_optimizer(dit, [torch.nn.Parameter(torch.ones(4, dtype=torch.bfloat16))], 1e-3)

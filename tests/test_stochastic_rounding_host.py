"""CPU: the numpy restatement of the stochastic rounding (tests/sr_ref.py) has the properties include/lcv_hip_sr.h states; the
finding the header starts from - bf16 AdamW's second moment never decays under round-to-nearest - holds for every normal bf16;
the header is held to the rules the other headers are held to (every declared symbol exported and bound with its argument count,
nothing of it in another header); the runners take --stochastic-rounding and refuse it after the pinned refusals; the
optimizers refuse what the flag cannot be combined with."""
import ctypes
import importlib.util
import inspect
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import master_weights_ref as W
import sr_ref as R

ROOT = Path(__file__).resolve().parents[1]
HEADER = "lcv_hip_sr.h"
NAMES = {"lcv_sr_sgd_step", "lcv_sr_adamw_step", "lcv_sr_round"}


# ------------------------------------------------------------------------------------------------------------ the rounding
# +-1 (a binade's first bf16), the zero / denormal corner, and the last bf16 below the largest finite one: all 2^16 low halves
# times all 2^16 values of r each, 2^32 roundings per upper half
UPPER = [0x3F80, 0xBF80, 0x0000, 0xFF7E]


@pytest.mark.parametrize("upper", UPPER)
def test_rounding_is_exact_or_a_neighbour_and_goes_away_from_zero_low_half_times_in_65536(upper):
    toward, away = np.uint16(upper), np.uint16(upper + 1)
    every_r = np.arange(1 << 16, dtype=np.uint32)[None, :]
    # exact values (low half 0) pass through for every r
    assert np.all(R.sr(np.full((1, 1), upper << 16, dtype=np.uint32), every_r) == toward)
    # per low half, over every r: nothing but the two neighbours, and the number of r that give the one away from zero (read
    # off the sum: every result is `toward` or `toward + 1`); a few low halves at a time, so that a block stays in cache
    rows = 16
    for low0 in range(0, 1 << 16, rows):
        low = np.arange(low0, low0 + rows, dtype=np.uint32)
        h = R.sr(((np.uint32(upper) << np.uint32(16)) | low)[:, None], every_r)
        assert h.shape == (rows, 1 << 16) and h.min() >= toward and h.max() <= away
        n_away = h.sum(axis=1, dtype=np.int64) - (int(toward) << 16)
        assert np.array_equal(n_away, low.astype(np.int64)), low0       # probability (u & 0xffff) / 65536 exactly
    # the neighbour away from zero is the larger magnitude, for both signs
    assert abs(float(W.bf16_to_f32(np.array([away]))[0])) > abs(float(W.bf16_to_f32(np.array([toward]))[0]))


def test_rounding_of_the_edge_of_the_range_and_of_non_finite_values():
    every_r = np.arange(1 << 16, dtype=np.uint32)
    # next to the largest finite bf16: may become infinity, with the stated probability
    h = R.sr(np.full(1 << 16, 0x7F7F4000, dtype=np.uint32), every_r)
    assert int((h == 0x7F80).sum()) == 0x4000 and int((h == 0x7F7F).sum()) == (1 << 16) - 0x4000
    # infinities stay, NaNs stay NaNs (made quiet, payload's upper bits kept), for every r
    for pat, want in ((0x7F800000, 0x7F80), (0xFF800000, 0xFF80), (0x7FC00000, 0x7FC0), (0xFFFFFFFF, 0xFFFF), (0x7F800001, 0x7FC0),
                      (0xFF812345, 0xFFC1)):
        assert np.all(R.sr(np.full(1 << 16, pat, dtype=np.uint32), every_r) == want), hex(pat)
    # +-0 stay +-0; a denormal goes to 0 or to the smallest bf16 denormal
    assert np.all(R.sr(np.zeros(1 << 16, dtype=np.uint32), every_r) == 0)
    assert np.all(R.sr(np.full(1 << 16, 0x80000000, dtype=np.uint32), every_r) == 0x8000)
    assert set(R.sr(np.full(1 << 16, 0x00000001, dtype=np.uint32), every_r).tolist()) == {0, 1}


def test_the_mean_over_r_is_the_fp32_value():
    """Unbiased: the mean of float(SR(u, r)) over the 65 536 values of r is float(u) exactly (in float64), wherever both
    neighbours are finite."""
    rng = np.random.default_rng(11)
    u = W.bits(W.log_uniform(rng, 64, -20.0, 20.0))
    every_r = np.arange(1 << 16, dtype=np.uint32)
    for ui in u.tolist():
        h = R.sr(np.full(1 << 16, ui, dtype=np.uint32), every_r)
        mean = W.bf16_to_f32(h).astype(np.float64).mean()
        assert mean == float(W.floats(np.array([ui], dtype=np.uint32))[0]), hex(ui)


def test_groups_streams_and_halves():
    # the layout of the LoRA dropout mask: element e is the low (even) or high (odd) half of word e >> 1
    from lora_dropout_ref import philox4x32_10
    seed, offset = 0x0123456789ABCDEF, 0xFFFFFFFF             # offset + stream carries into the high counter word
    got = R.halves(seed, offset, 2, np.array([5, (1 << 32) + 7], dtype=np.uint64))
    for row, g in zip(got, (5, (1 << 32) + 7)):
        c = offset + 2
        w = [int(x) for x in philox4x32_10((seed & 0xFFFFFFFF, seed >> 32), (c & 0xFFFFFFFF, c >> 32, g & 0xFFFFFFFF, g >> 32))]
        assert row.tolist() == [w[0] & 0xFFFF, w[0] >> 16, w[1] & 0xFFFF, w[1] >> 16, w[2] & 0xFFFF, w[2] >> 16, w[3] & 0xFFFF,
                                w[3] >> 16]
    # over a table the group is the workgroup and thread that own the element: unique across tensors
    numels = [1, 7, 8, 9, 2047, 2048, 2049, 4099]
    firsts = R.first_chunks(numels)
    assert firsts == [0, 1, 2, 3, 4, 5, 6, 8]
    seen = set()
    for n, fc in zip(numels, firsts):
        i = np.arange(0, n, 8)
        groups = set(((fc + i // 2048) * 256 + (i % 2048) // 8).tolist())
        assert not seen & groups
        seen |= groups
    # a tensor at first_chunk 0 and a single array draw the same bits on stream 0
    assert np.array_equal(R.table_bits(4099, 0, 3, 8, 0), R.array_bits(4099, 3, 8))
    # the streams and the offsets are different draws; offset + stream is one counter
    a = R.table_bits(4099, 2, 3, 8, 0)
    assert not np.array_equal(a, R.table_bits(4099, 2, 3, 8, 1)) and not np.array_equal(a, R.table_bits(4099, 2, 3, 12, 0))
    assert np.array_equal(R.table_bits(4099, 2, 3, 8, 2), R.table_bits(4099, 2, 3, 10, 0))
    assert 0.49 < (a >= 0x8000).mean() < 0.51


# ------------------------------------------------------------------------------------------------------------ the finding
def test_bf16_second_moment_times_beta2_rounds_back_to_itself_for_every_normal_bf16():
    """v = bf16(v * 0.999f), the decay of exp_avg_sq in the plain bf16 AdamW step: the product is within half a bf16 ulp of v
    for every positive normal bf16, so round-to-nearest-even returns v.  Under the stochastic rounding the same product steps
    down with probability about 0.13 to 0.26 and the mean decays."""
    v = np.arange(0x0080, 0x7F80, dtype=np.uint16)                       # every positive normal bf16
    prod = W.bf16_to_f32(v) * np.float32(0.999)
    assert np.array_equal(W.to_bf16_bits(prod), v)
    t = torch.from_numpy(prod.copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(t, v)                                          # torch's own conversion agrees
    # the product lies below v by a quarter to a half of the step down to the next bf16
    u = W.bits(prod)
    below = (v.astype(np.uint32) << 16) - u
    frac = below / 65536.0
    assert 0.12 < frac.min() and frac.max() < 0.27
    # and SR's expectation is the product itself: the decay survives
    r = np.arange(1 << 16, dtype=np.uint32)
    h = R.sr(np.full(1 << 16, u[0x3F80 - 0x0080], dtype=np.uint32), r)      # v = 1.0
    assert abs(W.bf16_to_f32(h).astype(np.float64).mean() - float(np.float32(0.999))) < 1e-12


# ------------------------------------------------------------------------------------------------------------ the header
def _declared(header: str):
    txt = (ROOT / "include" / header).read_text()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(lcv_[a-z0-9_]+)\s*\(", txt))


def _declared_arg_counts(header: str):
    txt = (ROOT / "include" / header).read_text()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return {name: len([a for a in args.split(",") if a.strip()])
            for name, args in re.findall(r"\bint\s+(lcv_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", txt)}


def _built():
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as ge
    ge.build()
    from lcv_hip import lib
    return lib, ctypes.CDLL(str(lib.lib_path()))


def test_sr_header_symbols_are_exported_and_bound_with_the_headers_argument_counts():
    lib, so = _built()
    names = _declared(HEADER)
    assert names == NAMES, names
    missing = [n for n in names if not hasattr(so, n)]
    assert not missing, f"declared in {HEADER} but not exported: {missing}"
    assert names == set(lib._SIGNATURES_SR), names ^ set(lib._SIGNATURES_SR)
    counts = _declared_arg_counts(HEADER)
    assert set(counts) == names
    for n in names:
        assert len(lib._SIGNATURES_SR[n]) == counts[n], n
    # the steps take the master steps' arguments without `low`, and uint64 seed, offset in front of the stream
    for sr_name, master in (("lcv_sr_sgd_step", "lcv_master_sgd_step"), ("lcv_sr_adamw_step", "lcv_master_adamw_step")):
        m = lib._SIGNATURES_MASTER[master]
        assert lib._SIGNATURES_SR[sr_name] == [m[0]] + m[2:-1] + [lib.U64, lib.U64, lib.P], sr_name
    assert lib._SIGNATURES_SR["lcv_sr_round"] == [lib.P, lib.P, lib.I64, lib.U64, lib.U64, lib.P]
    # none is declared in another header or bound in another table
    for other in sorted((ROOT / "include").glob("*.h")):
        if other.name != HEADER:
            assert not _declared(other.name) & names, other.name
    assert HEADER not in (ROOT / "include" / "lcv_hip.h").read_text()
    for table_name in [k for k in vars(lib) if k.startswith("_SIGNATURES") and k != "_SIGNATURES_SR"]:
        assert not set(getattr(lib, table_name)) & names, table_name
    so.lcv_version.restype = ctypes.c_int
    assert so.lcv_version() >= 13                     # went up with the new entry points
    loaded = lib.load()
    for n in names:
        assert getattr(loaded, n).argtypes == lib._SIGNATURES_SR[n] and getattr(loaded, n).restype is ctypes.c_int


def test_the_source_shares_the_master_row_math_and_the_philox_and_is_built_without_contraction():
    from lcv_hip import build
    csrc = ROOT / "longcat-video-tta_amd" / "csrc"
    src = (csrc / "optim_sr.hip").read_text()
    assert build.EXTRA["optim_sr.hip"] == ["-ffp-contract=off"] == build.EXTRA["optim_master.hip"]
    for word in ("atomic", "fmaf", "asm", "getenv", "lcv_knob(", "hipMalloc", "__shared__", "__syncthreads"):
        assert word not in src, word
    assert '#include "lcv_hip_sr.h"' in src and '#include "master_elem.h"' in src and '#include "philox.h"' in src
    for entry in NAMES:
        assert len(re.findall(rf'extern "C" int {entry}\(', src)) == 1, entry
    for use in ("master_sgd_elem(", "master_adamw_elem(", "philox4x32_10(", "find_tensor(", "adam_scalars(", "optim_table_ok(",
                "chunk_grid("):
        assert use in src, use
    # the row math and the generator are called, not restated
    for restated in ("0xD2511F53", "0x9E3779B9", "__builtin_sqrtf", "bc2_sqrt", "0x7fffffff", "pow("):
        assert restated not in src, restated


def test_every_sr_entry_point_has_a_kernel_level_test():
    import ast
    tests = {"lcv_sr_round": "test_sr_round_bits", "lcv_sr_sgd_step": "test_sr_sgd_step_bits",
             "lcv_sr_adamw_step": "test_sr_adamw_step_bits"}
    assert set(tests) == _declared(HEADER)
    tree = ast.parse((ROOT / "tests" / "test_gpu_stochastic_rounding.py").read_text())
    assert set(tests.values()) <= {n.name for n in ast.walk(tree) if isinstance(n, ast.FunctionDef)}


# ------------------------------------------------------------------------------------------------------------ the optimizers
@pytest.mark.parametrize("cls", ["FusedSGDClip", "FusedAdamWClip"])
def test_constructors_take_the_keyword_and_refuse_cpu_and_fp32_parameters(cls):
    from lcv_hip import ops
    from lcv_hip.lib import LcvError
    make = getattr(ops, cls)
    p = inspect.signature(make.__init__).parameters["stochastic_rounding"]
    assert p.default is False
    with pytest.raises(LcvError, match="GPU"):
        make([torch.zeros(8, dtype=torch.bfloat16)], stochastic_rounding=True)
    with pytest.raises(LcvError, match="rounds nothing to bf16"):
        make([torch.zeros(8, dtype=torch.float32)], stochastic_rounding=True)
    opt = make([torch.zeros(8, dtype=torch.bfloat16)])
    assert opt.stochastic_rounding is False


def test_one_definition_of_the_generator_draw():
    """tta/lora.py's draw_dropout_offset and the optimizers' draw are one function."""
    from lcv_hip import ops
    from tta import lora
    assert lora.draw_dropout_offset is ops.draw_philox_offset
    texts = [p.read_text() for p in (ROOT / "longcat-video-tta_amd").rglob("*.py")]
    assert sum(t.count("set_offset(") for t in texts) == 1


def test_loops_take_the_keyword_before_the_keyword_only_ones_and_default_it_off():
    from tta import delta, full_tta, inner_loop
    for fn in (inner_loop.finetune_lora_on_conditioning, inner_loop.finetune_lora_batch, full_tta.finetune_full_on_conditioning,
               full_tta.finetune_full_batch, delta.optimize_norm_params):
        p = inspect.signature(fn).parameters["stochastic_rounding"]
        assert p.default is False, fn.__name__
    for fn in (delta.optimize_delta_a, delta.optimize_delta_b, delta.optimize_delta_c, delta.optimize_film_adapter):
        assert "stochastic_rounding" not in inspect.signature(fn).parameters


def test_norm_tuning_refuses_the_flag_with_an_fp32_parameter_in_the_list():
    from tta import delta
    params = [torch.nn.Parameter(torch.zeros(4, dtype=torch.bfloat16)), torch.nn.Parameter(torch.zeros(4, dtype=torch.float32))]
    with pytest.raises(ValueError, match="stochastic_rounding cannot train fp32 parameters"):
        delta.optimize_norm_params(None, params, None, None, None, None, stochastic_rounding=True)


def test_loops_refuse_the_flag_under_sequence_parallelism():
    from tta import inner_loop

    class Sharded(torch.nn.Module):
        _sp_group = object()

    with pytest.raises(ValueError, match="sequence parallelism"):
        inner_loop.refuse_stochastic_rounding_under_sp(Sharded(), True)
    assert inner_loop.refuse_stochastic_rounding_under_sp(Sharded(), False) is None
    assert inner_loop.refuse_stochastic_rounding_under_sp(torch.nn.Linear(1, 1), True) is None


# ------------------------------------------------------------------------------------------------------------ the runners
def _script(rel):
    spec = importlib.util.spec_from_file_location("sr_" + Path(rel).stem, ROOT / "longcat-video-tta_amd" / rel)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


BASE = ["--checkpoint-dir", "synthetic", "--data-dir", "synthetic:1", "--output-dir", "x"]
LORA, FULL, NORM = ("lora_experiment/scripts/run_lora_tta.py", "lora_experiment/scripts/run_full_tta.py",
                    "delta_experiment/scripts/run_norm_tune_tta.py")


@pytest.mark.parametrize("rel", [LORA, FULL, NORM])
def test_runners_take_the_flag_and_refuse_it_after_the_pinned_refusals(rel, capsys):
    from tta import cli_args as C
    mod = _script(rel)
    off, on = mod.parse_args(BASE), mod.parse_args(BASE + ["--stochastic-rounding"])
    assert off.stochastic_rounding is False and on.stochastic_rounding is True
    assert C.stochastic_rounding_record(off) == {} and C.stochastic_rounding_record(on) == {"stochastic_rounding": True}
    assert "stochastic_rounding" not in C.optimizer_kwargs(off) and C.optimizer_kwargs(on)["stochastic_rounding"] is True
    sr = "--stochastic-rounding"
    cases = [([sr, "--master-weights"], "--stochastic-rounding cannot be combined with --master-weights"),
             # the pinned refusals fire first, in their order, with the flag present
             ([sr, "--adam-8bit"], "--adam-8bit needs --master-weights"),
             ([sr, "--grad-accum", "0"], "--grad-accum must be at least 1"),
             ([sr, "--grad-accum", "2"], "--grad-accum above 1 needs --master-weights"),
             ([sr, "--master-weights", "--adam-8bit", "--grad-accum", "2"] + (["--optimizer", "adamw"] if rel == FULL else []),
              "--grad-accum above 1 cannot be combined with --adam-8bit"),
             ([sr, "--weight-ema-warmup"], "--weight-ema-warmup needs --weight-ema"),
             ([sr, "--weight-ema", "0.9"], "--weight-ema needs --master-weights"),
             ([sr, "--master-weights", "--weight-ema", "1.5"], "must be in [0, 1)")]
    if rel == FULL:
        cases.append(([sr, "--adam-8bit", "--master-weights"], "--adam-8bit needs --optimizer adamw"))
    if rel != LORA:
        cases.append(([sr, "--decay-to-base"], "--decay-to-base needs --master-weights"))
    if rel == NORM:
        cases += [([sr, "--also-tune-delta"], "--stochastic-rounding cannot be combined with --also-tune-delta"),
                  ([sr, "--also-tune-delta", "--master-weights"], "--stochastic-rounding cannot be combined with --master-weights"),
                  ([sr, "--also-tune-delta", "--master-weights", "--weight-ema", "0.9"],
                   "--weight-ema cannot be combined with --also-tune-delta")]
    for argv, message in cases:
        capsys.readouterr()
        with pytest.raises(SystemExit) as e:
            mod.parse_args(BASE + argv)
        err = capsys.readouterr().err
        assert e.value.code == 2 and message in err, (argv, err)
        assert len([ln for ln in err.strip().splitlines() if "error:" in ln]) == 1


def test_delta_and_film_runners_do_not_have_the_flag(capsys):
    for rel in ("delta_experiment/scripts/run_delta_a.py", "delta_experiment/scripts/run_film_tta.py"):
        mod = _script(rel)
        assert "--stochastic-rounding" not in {s for a in mod.build_parser()._actions for s in a.option_strings}, rel


def test_norm_tune_summary_head_carries_the_key_only_with_the_flag(monkeypatch):
    mod = _script(NORM)
    seen = []
    monkeypatch.setattr(mod.R, "run_delta_method", lambda args, method, **kw: seen.append(kw))
    mod.main(BASE)
    mod.main(BASE + ["--stochastic-rounding"])
    off, on = seen
    assert set(on["summary_head"]) - set(off["summary_head"]) == {"stochastic_rounding"}
    assert on["summary_head"]["stochastic_rounding"] is True
    assert "stochastic_rounding" not in off["result_extra"]({}) and on["result_extra"]({}) == {"stochastic_rounding": True}

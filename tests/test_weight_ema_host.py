"""CPU: the numpy restatement of the fp32 weight average (tests/ema_ref.py) has the properties the format promises (a swap is
an involution on every bit pattern, beta = 0 copies the masters, an average equal to the masters stays); include/lcv_hip_ema.h
is held to the rules the other headers are held to; the optimizers, the loops and the runners take `enable_weight_ema` /
`weight_ema` / `--weight-ema`, refuse what they must, and hold nothing when it is off."""
import ctypes
import importlib.util
import inspect
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import ema_ref as E
import master_weights_ref as W

ROOT = Path(__file__).resolve().parents[1]
HEADER = "lcv_hip_ema.h"
NAMES = {"lcv_master_ema_load", "lcv_master_ema_update", "lcv_master_ema_swap"}


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


# ------------------------------------------------------------------------------------------------------------ the restatement
def test_swap_twice_is_the_identity_on_every_bit_pattern():
    """Subnormals, +-0, +-inf and NaN payloads among them: no arithmetic touches a value on its way through."""
    m, e = W.edge_patterns(seed=11), W.edge_patterns(seed=12)[::-1].copy()
    for special in (0x00000001, 0x807FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7FFFFFFF, 0xFFFFFFFF):
        assert special in m and special in e
    h, low = W.split(m)
    assert np.array_equal(W.join(h, low), m)
    h1, l1, e1 = E.swap(h, low, e)
    assert np.array_equal(e1, m) and np.array_equal(W.join(h1, l1), e)          # a valid master of the average, and the master
    assert np.array_equal(h1, W.split(e)[0])                                    # h is the ties-away bf16 of the average
    assert not np.array_equal(h1, h)
    h2, l2, e2 = E.swap(h1, l1, e1)
    assert np.array_equal(h2, h) and np.array_equal(l2, low) and np.array_equal(e2, e)
    assert np.array_equal(E.load(h, low), m)


def _finite_nonzero(seed, n=1 << 20):
    rng = np.random.default_rng(seed)
    m = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
    exp = (m >> 23) & 0xFF
    m = m[(exp != 0xFF) & ((m & 0x7FFFFFFF) != 0)]                              # finite, no zero masters
    assert m.size > n // 2 and (exp == 0).any()                                 # subnormals stay in
    return m


def test_beta_zero_copies_the_masters_and_an_average_at_the_masters_stays():
    w = _finite_nonzero(21)
    h, low = W.split(w)
    e = np.roll(w, 1)
    # b = 0: t = 0 * d is a zero wherever d is finite (it overflows where w and e are huge and of opposite sign: left out)
    with np.errstate(all="ignore"):
        finite = np.isfinite(W.floats(w) - W.floats(e))
    assert finite.mean() > 0.9
    got = E.update(h, low, e, 0.0)
    assert np.array_equal(got[finite], w[finite])
    # w = e: d = +0, t = +-0, e = w - (+-0) = w, for every beta
    for beta in (0.0, 0.18, 0.5, 0.9, 0.999):
        assert np.array_equal(E.update(h, low, w, beta), w), beta


def test_update_is_the_convex_combination():
    rng = np.random.default_rng(3)
    h, low = W.weights(rng, 5000)
    e = W.bits(W.log_uniform(rng, 5000, -10.0, 1.0))
    w64, e64 = W.master(h, low).astype(np.float64), W.floats(e).astype(np.float64)
    for beta in (0.5, 0.9, 0.999):
        got = W.floats(E.update(h, low, e, beta)).astype(np.float64)
        b = float(np.float32(beta))
        want = b * e64 + (1.0 - b) * w64
        # three roundings, each at most 2^-24 relative of a quantity no larger than |w| + |e|
        assert np.all(np.abs(got - want) <= 3 * 2.0 ** -24 * (np.abs(w64) + np.abs(e64)))


def test_ema_beta_table():
    from lcv_hip import ops
    for fn in (ops.ema_beta, E.ema_beta):
        assert [fn(0.9, t) for t in (1, 5, 100)] == [0.9, 0.9, 0.9]
        assert [fn(0.9, t, False) for t in (1, 20)] == [0.9, 0.9]
        warm = [fn(0.9, t, True) for t in range(1, 21)]
        assert warm[0] == 2.0 / 11.0 and warm[1] == 3.0 / 12.0 and warm[9] == 11.0 / 20.0 and warm[19] == 21.0 / 30.0
        assert [round(v, 2) for v in (warm[0], warm[1], warm[9], warm[19])] == [0.18, 0.25, 0.55, 0.70]
        assert all(a < b for a, b in zip(warm, warm[1:]))
        assert fn(0.9, 79, True) == 80.0 / 89.0 and fn(0.9, 81, True) == 0.9 and fn(0.9, 10 ** 6, True) == 0.9
        assert fn(0.5, 8, True) == 0.5 and fn(0.5, 7, True) == 8.0 / 17.0 and fn(0.0, 3, True) == 0.0
    assert all(ops.ema_beta(b, t, w) == E.ema_beta(b, t, w) for b in (0.0, 0.3, 0.9, 0.999) for t in range(1, 40)
               for w in (False, True))


# ------------------------------------------------------------------------------------------------------------ the header
def test_ema_header_symbols_are_exported_and_bound():
    lib, so = _built()
    names = _declared(HEADER)
    assert names == NAMES, names
    missing = [n for n in names if not hasattr(so, n)]
    assert not missing, f"declared in {HEADER} but not exported: {missing}"
    assert names == set(lib._SIGNATURES_EMA), names ^ set(lib._SIGNATURES_EMA)
    for other in (lib._SIGNATURES, lib._SIGNATURES_LPIPS, lib._SIGNATURES_DET, lib._SIGNATURES_LORA, lib._SIGNATURES_MASTER,
                  lib._SIGNATURES_MOMENTS8, lib._SIGNATURES_ACCUM, lib._SIGNATURES_ANCHOR):
        assert not set(lib._SIGNATURES_EMA) & set(other)
    plain = [lib.P, lib.P, lib.P, lib.I64, lib.I64, lib.P]
    assert lib._SIGNATURES_EMA["lcv_master_ema_load"] == plain and lib._SIGNATURES_EMA["lcv_master_ema_swap"] == plain
    assert lib._SIGNATURES_EMA["lcv_master_ema_update"] == plain[:-1] + [lib.F64, lib.P]
    for other in ("lcv_hip.h", "lcv_hip_master.h", "lcv_hip_moments8.h", "lcv_hip_accum.h", "lcv_hip_det.h", "lcv_hip_lora.h",
                  "lcv_hip_lpips.h", "lcv_hip_anchor.h"):
        txt = (ROOT / "include" / other).read_text()
        assert not _declared(other) & names, other
        assert HEADER not in txt and not any(n in txt for n in names), other
    so.lcv_version.restype = ctypes.c_int
    assert so.lcv_version() >= 9                      # went up with the new entry points
    loaded = lib.load()
    for n in names:
        assert getattr(loaded, n).argtypes == lib._SIGNATURES_EMA[n] and getattr(loaded, n).restype is ctypes.c_int


def test_every_ema_entry_point_has_a_kernel_level_test():
    import ast
    tree = ast.parse((ROOT / "tests" / "test_gpu_weight_ema.py").read_text())
    assert {"test_load_bits", "test_update_bits", "test_swap_bits"} <= {n.name for n in ast.walk(tree)
                                                                        if isinstance(n, ast.FunctionDef)}


def test_the_source_uses_no_atomics_and_no_lds_and_shares_the_format():
    csrc = ROOT / "longcat-video-tta_amd" / "csrc"
    src = (csrc / "optim_ema.hip").read_text()
    code = re.sub(r"//[^\n]*", "", src)                                # the comments may say what the code does not use
    for word in ("atomic", "__shared__", "fmaf", "asm", "getenv", "lcv_knob(", "hipMalloc", "__syncthreads"):
        assert word not in code, word
    shared = (csrc / "master_elem.h").read_text()
    for fn in ("float master_ema_elem(", "float master_join(", "void master_split("):
        assert shared.count(fn) == 1 and fn not in src, fn
    for use in ("master_ema_elem(", "master_join(", "master_split(", "find_tensor(", "CHUNK", "__launch_bounds__(256)", "optim_table_ok("):
        assert use in src, use
    from lcv_hip import build
    assert build.EXTRA["optim_ema.hip"] == ["-ffp-contract=off"] == build.EXTRA["optim_master.hip"]


# ------------------------------------------------------------------------------------------------------------ the optimizers
@pytest.mark.parametrize("cls", ["FusedSGDClip", "FusedAdamWClip"])
def test_enable_weight_ema_refusals_and_the_optimizer_without_it(cls):
    from lcv_hip import ops
    from lcv_hip.lib import LcvError
    make = getattr(ops, cls)
    # the constructors are as they were: the average is switched on by a method
    kw_only = [p.name for p in inspect.signature(make.__init__).parameters.values() if p.kind is inspect.Parameter.KEYWORD_ONLY]
    assert kw_only == ["grad_accum", "anchor"]
    assert list(inspect.signature(make.enable_weight_ema).parameters) == ["self", "beta", "warmup"]
    assert inspect.signature(make.enable_weight_ema).parameters["warmup"].default is False
    opt = make([torch.zeros(8, dtype=torch.bfloat16)])
    assert opt.weight_ema is None and opt.ema_tensors() == [] and opt.ema_in_params is False
    assert make.weight_ema is None and "weight_ema" not in vars(opt) and "_ema" not in vars(opt)      # class-level defaults
    with pytest.raises(LcvError, match="needs master_weights=True"):
        opt.enable_weight_ema(0.9)
    for beta in (1.0, -0.1, float("nan"), 1.5):
        with pytest.raises(ValueError, match=r"must be in \[0, 1\)"):
            opt.enable_weight_ema(beta)
    for method in ("ema_swap", "ema_reset"):
        with pytest.raises(LcvError, match="needs enable_weight_ema"):
            getattr(opt, method)()
    assert opt.weight_ema is None and opt.ema_tensors() == []
    opt.weight_ema = 0.5                                               # as after a first call
    with pytest.raises(LcvError, match="already called"):
        opt.enable_weight_ema(0.9)
    assert "left alone" in make.resync.__doc__


def test_loops_take_the_two_keywords_keyword_only_in_the_stated_places():
    from tta import delta, full_tta, inner_loop
    for fn, before in ((inner_loop.finetune_lora_on_conditioning, "grad_accum"), (inner_loop.finetune_lora_batch, "grad_accum"),
                       (full_tta.finetune_full_on_conditioning, "decay_to_base"), (full_tta.finetune_full_batch, "decay_to_base"),
                       (delta.optimize_norm_params, "decay_to_base")):
        params = list(inspect.signature(fn).parameters.values())
        names = [p.name for p in params]
        at = names.index("weight_ema")
        assert names[at:at + 3] == ["weight_ema", "ema_warmup", before], fn.__name__
        assert params[at].default is None and params[at + 1].default is False
        assert params[at].kind is params[at + 1].kind is inspect.Parameter.KEYWORD_ONLY
        assert params[at - 1].kind is not inspect.Parameter.KEYWORD_ONLY            # the first keyword-only ones
        assert names[-3:] == ["grad_accum", "moments_8bit", "master_weights"]        # the pinned tails
    # the engine and the optimizer factory are as they were
    assert list(inspect.signature(inner_loop.run_adaptation).parameters)[-2:] == ["finish_eval", "grad_accum"]
    assert list(inspect.signature(full_tta._make_optimizer).parameters)[-1] == "anchor"
    for fn in (delta.optimize_delta_a,):
        assert "weight_ema" not in inspect.signature(fn).parameters


def test_norm_tuning_refuses_the_average_with_an_fp32_parameter_in_the_list():
    from tta import delta
    params = [torch.nn.Parameter(torch.zeros(4, dtype=torch.bfloat16)), torch.nn.Parameter(torch.zeros(4, dtype=torch.float32))]
    with pytest.raises(ValueError, match="weight_ema cannot train fp32 parameters"):
        delta.optimize_norm_params(None, params, None, None, None, None, weight_ema=0.9, master_weights=True)


# ------------------------------------------------------------------------------------------------------------ the runners
def _script(rel):
    spec = importlib.util.spec_from_file_location("ema_" + Path(rel).stem, ROOT / "longcat-video-tta_amd" / rel)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


BASE = ["--checkpoint-dir", "synthetic", "--data-dir", "synthetic:1", "--output-dir", "x"]
LORA, FULL, NORM = ("lora_experiment/scripts/run_lora_tta.py", "lora_experiment/scripts/run_full_tta.py",
                    "delta_experiment/scripts/run_norm_tune_tta.py")


@pytest.mark.parametrize("rel", [LORA, FULL, NORM])
def test_runners_take_weight_ema_and_refuse_it_at_parse_time(rel, capsys):
    mod = _script(rel)
    off = mod.parse_args(BASE)
    assert off.weight_ema is None and off.weight_ema_warmup is False
    on = mod.parse_args(BASE + ["--master-weights", "--weight-ema", "0.9", "--weight-ema-warmup"])
    assert on.weight_ema == 0.9 and on.weight_ema_warmup is True
    assert mod.parse_args(BASE + ["--master-weights", "--weight-ema", "0"]).weight_ema == 0.0
    if rel == LORA:
        assert mod.parse_args(BASE + ["--master-weights", "--weight-ema", "0.5", "--use-builtin-lora"]).use_builtin_lora is True
        help_text = mod.build_parser().format_help()
        assert "averaged" in help_text[help_text.rindex("--save-lora-weights"):][:400]
    cases = [(["--weight-ema", "0.9"], "--weight-ema needs --master-weights"),
             (["--master-weights", "--weight-ema", "1.0"], "must be in [0, 1)"),
             (["--master-weights", "--weight-ema", "-0.1"], "must be in [0, 1)"),
             (["--master-weights", "--weight-ema", "nan"], "must be in [0, 1)"),
             (["--master-weights", "--weight-ema-warmup"], "--weight-ema-warmup needs --weight-ema"),
             # the pinned refusals fire as before, with the flag present
             (["--weight-ema", "0.9", "--grad-accum", "2"], "--grad-accum above 1 needs --master-weights")]
    if rel == NORM:
        cases.append((["--master-weights", "--weight-ema", "0.9", "--also-tune-delta"],
                      "--weight-ema cannot be combined with --also-tune-delta"))
    if rel != LORA:
        cases.append((["--weight-ema", "0.9", "--decay-to-base"], "--decay-to-base needs --master-weights"))
    for argv, message in cases:
        capsys.readouterr()
        with pytest.raises(SystemExit) as e:
            mod.parse_args(BASE + argv)
        err = capsys.readouterr().err
        assert e.value.code == 2 and message in err, (argv, err)
        assert len([ln for ln in err.strip().splitlines() if "error:" in ln]) == 1


def test_delta_and_film_runners_reject_the_flag(capsys):
    for rel in ("delta_experiment/scripts/run_delta_a.py", "delta_experiment/scripts/run_film_tta.py"):
        mod = _script(rel)
        opts = {s for a in mod.build_parser()._actions for s in a.option_strings}
        assert "--weight-ema" not in opts and "--weight-ema-warmup" not in opts, rel
        with pytest.raises(SystemExit) as e:
            mod.build_parser().parse_args(BASE + ["--weight-ema", "0.9"])
        assert e.value.code == 2 and "unrecognized arguments" in capsys.readouterr().err


def test_records_and_keywords_are_empty_with_the_flag_off():
    from tta import cli_args as C
    mod = _script(FULL)
    off = mod.parse_args(BASE + ["--master-weights"])
    on = mod.parse_args(BASE + ["--master-weights", "--weight-ema", "0.9"])
    assert C.weight_ema_kwargs(off) == {} and C.weight_ema_record(off) == {}
    assert C.weight_ema_kwargs(on) == {"weight_ema": 0.9, "ema_warmup": False}
    assert C.weight_ema_record(on) == {"weight_ema": 0.9, "weight_ema_warmup": False}


def test_norm_tune_summary_head_carries_the_keys_only_with_the_flag(monkeypatch):
    mod = _script(NORM)
    seen = []
    monkeypatch.setattr(mod.R, "run_delta_method", lambda args, method, **kw: seen.append(kw))
    mod.main(BASE + ["--master-weights"])
    mod.main(BASE + ["--master-weights", "--weight-ema", "0.9", "--weight-ema-warmup"])
    off, on = seen
    assert set(on["summary_head"]) - set(off["summary_head"]) == {"weight_ema", "weight_ema_warmup"}
    assert on["summary_head"]["weight_ema"] == 0.9 and on["summary_head"]["weight_ema_warmup"] is True
    called = {}
    monkeypatch.setattr(mod, "optimize_norm_params", lambda *a, **kw: called.update(kw) or {})

    class _W:
        tuned_params = []
    off["optimize_fn"](_W(), None, None, None, None, "cpu", None)
    assert "weight_ema" not in called and "ema_warmup" not in called
    on["optimize_fn"](_W(), None, None, None, None, "cpu", None)
    assert called["weight_ema"] == 0.9 and called["ema_warmup"] is True

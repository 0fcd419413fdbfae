"""CPU: the numpy restatement of fp32 gradient accumulation (tests/grad_accum_ref.py) is tied to the pinned master-weight
steps (one micro-step at scale 1 reproduces them bit for bit); include/lcv_hip_accum.h is held to the rules the other headers
are held to; the optimizers, the loops and the runners take `grad_accum` / `--grad-accum` and refuse it where it cannot mean
anything."""
import ctypes
import importlib.util
import inspect
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import grad_accum_ref as R
import master_weights_ref as W

ROOT = Path(__file__).resolve().parents[1]
HEADER = "lcv_hip_accum.h"
F = np.float32
NAMES = {"lcv_grad_accumulate", "lcv_master_sgd_step_g32", "lcv_master_adamw_step_g32"}


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
def _inputs(seed, n=20000):
    rng = np.random.default_rng(seed)
    h, low = W.weights(rng, n)
    return h, low, [W.grads(rng, n) for _ in range(3)]


def test_one_micro_step_at_scale_one_is_the_widened_gradient():
    _, _, gs = _inputs(1)
    g = gs[0].copy()
    g[:4] = [0x0000, 0x8000, 0x3F80, 0xBF80]                        # +0, -0, +1, -1
    acc = R.accumulate(np.zeros(g.size, dtype=F), g, 1.0)
    assert acc.dtype == F
    want = W.bits(W.bf16_to_f32(g)).copy()
    want[1] = 0                                                     # 0 + (-0) is +0: always the add, no "first" form
    assert np.array_equal(W.bits(acc), want)
    # an inexact scale: two roundings, the product's and the sum's
    a = R.accumulate(acc, gs[1], 1.0 / 3.0)
    t = (W.bf16_to_f32(gs[1]).astype(np.float64) * float(F(1.0 / 3.0))).astype(F)
    assert np.array_equal(W.bits(a), W.bits((acc.astype(np.float64) + t.astype(np.float64)).astype(F)))


@pytest.mark.parametrize("coef", [1.0, 0.37])
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_g32_sgd_fed_the_widened_gradient_gives_the_pinned_steps_bits(coef, wd):
    h, low, gs = _inputs(2)
    hp, lp = h, low
    for g in gs:
        g32 = R.accumulate(np.zeros(g.size, dtype=F), g, 1.0)
        h, low = R.sgd_step_g32(h, low, g32, coef, 0.05, wd)
        hp, lp = W.sgd_step(hp, lp, g, coef, 0.05, wd)
        assert np.array_equal(h, hp) and np.array_equal(low, lp)
    assert (h != _inputs(2)[0]).any()


@pytest.mark.parametrize("coef", [1.0, 0.37])
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_g32_adamw_fed_the_widened_gradient_gives_the_pinned_steps_bits(coef, wd):
    h, low, gs = _inputs(3)
    m = v = np.zeros(h.size, dtype=F)
    hp, lp, mp, vp = h, low, m, v
    for k, g in enumerate(gs):
        g32 = R.accumulate(np.zeros(g.size, dtype=F), g, 1.0)
        h, low, m, v = R.adamw_step_g32(h, low, m, v, g32, coef, 1e-3, 0.9, 0.999, 1e-8, wd, k + 1)
        hp, lp, mp, vp = W.adamw_step(hp, lp, mp, vp, g, coef, 1e-3, 0.9, 0.999, 1e-8, wd, k + 1)
        assert np.array_equal(h, hp) and np.array_equal(low, lp)
        assert np.array_equal(W.bits(m), W.bits(mp)) and np.array_equal(W.bits(v), W.bits(vp))


def test_two_halves_of_one_gradient_are_that_gradient():
    _, _, gs = _inputs(4)
    a = R.accumulate(np.zeros(gs[0].size, dtype=F), gs[0], 0.5)
    a = R.accumulate(a, gs[0], 0.5)
    assert np.array_equal(W.bits(a), W.bits(W.bf16_to_f32(gs[0])))


# ------------------------------------------------------------------------------------------------------------ the header
def test_accum_header_symbols_are_exported_and_bound():
    lib, so = _built()
    names = _declared(HEADER)
    assert names == NAMES, names
    missing = [n for n in names if not hasattr(so, n)]
    assert not missing, f"declared in {HEADER} but not exported: {missing}"
    assert names == set(lib._SIGNATURES_ACCUM), names ^ set(lib._SIGNATURES_ACCUM)
    for other in (lib._SIGNATURES, lib._SIGNATURES_LPIPS, lib._SIGNATURES_DET, lib._SIGNATURES_LORA, lib._SIGNATURES_MASTER,
                  lib._SIGNATURES_MOMENTS8):
        assert not set(lib._SIGNATURES_ACCUM) & set(other)
    # the steps take exactly their counterparts' arguments: only what `grad` points to differs
    assert lib._SIGNATURES_ACCUM["lcv_master_sgd_step_g32"] == lib._SIGNATURES_MASTER["lcv_master_sgd_step"]
    assert lib._SIGNATURES_ACCUM["lcv_master_adamw_step_g32"] == lib._SIGNATURES_MASTER["lcv_master_adamw_step"]
    assert lib._SIGNATURES_ACCUM["lcv_grad_accumulate"] == [lib.P, lib.P, lib.I64, lib.I64, lib.F64, lib.P]
    # the other headers' closed lists are untouched
    for other in ("lcv_hip.h", "lcv_hip_master.h", "lcv_hip_moments8.h", "lcv_hip_det.h", "lcv_hip_lora.h", "lcv_hip_lpips.h"):
        txt = (ROOT / "include" / other).read_text()
        assert not _declared(other) & names, other
        assert HEADER not in txt and not any(n in txt for n in names), other
    so.lcv_version.restype = ctypes.c_int
    assert so.lcv_version() >= 7                      # went up with the new entry points
    loaded = lib.load()
    for n in names:
        assert getattr(loaded, n).argtypes == lib._SIGNATURES_ACCUM[n] and getattr(loaded, n).restype is ctypes.c_int


def test_every_accum_entry_point_has_a_kernel_level_test():
    import ast
    tests = {"lcv_grad_accumulate": "test_accumulate_bits", "lcv_master_sgd_step_g32": "test_sgd_g32_step_bits",
             "lcv_master_adamw_step_g32": "test_adamw_g32_step_bits"}
    assert set(tests) == _declared(HEADER)
    tree = ast.parse((ROOT / "tests" / "test_gpu_grad_accum.py").read_text())
    assert set(tests.values()) <= {n.name for n in ast.walk(tree) if isinstance(n, ast.FunctionDef)}


def test_the_source_uses_no_atomics_no_lds_and_shares_the_step_with_the_master_kernels():
    csrc = ROOT / "longcat-video-tta_amd" / "csrc"
    src = (csrc / "optim_accum.hip").read_text()
    for word in ("atomic", "fmaf", "asm", "getenv", "lcv_knob(", "hipMalloc", "__shared__", "__syncthreads"):
        assert word not in src, word
    # what is left here is the accumulate kernel and its entry point
    assert '#include "lcv_hip_accum.h"' in src and "find_tensor(" in src and "optim_table_ok(" in src
    assert re.findall(r'extern "C" int (\w+)\(', src) == ["lcv_grad_accumulate"] and "_step" not in src
    # the fp32-gradient steps are the master kernels themselves (optim_master.hip): the same word list holds there, the header
    # is included there so that the compiler checks the signatures, and the op sequences are the shared ones
    master = (csrc / "optim_master.hip").read_text()
    for word in ("atomic", "fmaf", "asm", "getenv", "lcv_knob(", "hipMalloc", "__shared__", "__syncthreads"):
        assert word not in master, word
    assert '#include "lcv_hip_accum.h"' in master and '#include "master_elem.h"' in master
    for entry in ("lcv_master_sgd_step_g32", "lcv_master_adamw_step_g32"):
        assert len(re.findall(rf'extern "C" int {entry}\(', master)) == 1, entry
    assert "void master_adamw_elem(" not in master and "master_adamw_elem(" in master
    assert "float master_sgd_elem(" not in master and "master_sgd_elem(" in master
    assert "master_join(" in master and "master_split(" in master and "find_tensor(" in master
    assert "accum_sgd_elem" not in "".join(p.read_text() for p in csrc.iterdir() if p.suffix in (".hip", ".h"))
    from lcv_hip import build
    assert build.EXTRA["optim_accum.hip"] == build.EXTRA["optim_master.hip"] == ["-ffp-contract=off"]


# ------------------------------------------------------------------------------------------------------------ the optimizers
@pytest.mark.parametrize("cls", ["FusedSGDClip", "FusedAdamWClip"])
def test_constructors_take_grad_accum_keyword_only_and_refuse_what_cannot_work(cls):
    from lcv_hip import ops
    from lcv_hip.lib import LcvError
    make = getattr(ops, cls)
    p = inspect.signature(make.__init__).parameters["grad_accum"]
    assert p.default == 1 and p.kind is inspect.Parameter.KEYWORD_ONLY
    bf = [torch.zeros(8, dtype=torch.bfloat16)]
    with pytest.raises(LcvError, match="grad_accum > 1 needs master_weights=True"):
        make(bf, grad_accum=2)
    with pytest.raises(ValueError, match="at least 1"):
        make(bf, grad_accum=0)
    with pytest.raises(ValueError, match="at least 1"):
        make(bf, grad_accum=-3)
    # the existing refusals fire first, with their messages
    with pytest.raises(LcvError, match="GPU"):
        make(bf, master_weights=True, grad_accum=2)
    with pytest.raises(LcvError, match="fp32 parameters are already exact"):
        make([torch.zeros(8, dtype=torch.float32)], master_weights=True, grad_accum=2)
    # 1, spelled out or not: today's optimizer, nothing allocated
    for opt in (make(bf), make(bf, grad_accum=1)):
        assert opt.grad_accum == 1 and opt.accumulated_grads() == []
        with pytest.raises(LcvError, match="needs grad_accum > 1"):
            opt.accumulate()
        opt.zero_grad()


def test_adamw_refuses_grad_accum_with_8bit_moments_and_the_joint_clip_refuses_it():
    from lcv_hip import ops
    from lcv_hip.lib import LcvError
    bf = [torch.zeros(8, dtype=torch.bfloat16)]
    with pytest.raises(LcvError, match="needs master_weights=True"):             # the 8-bit refusal comes first, as today
        ops.FusedAdamWClip(bf, moments_8bit=True, grad_accum=2)
    with pytest.raises(LcvError, match="GPU"):
        ops.FusedAdamWClip(bf, master_weights=True, moments_8bit=True, grad_accum=2)

    class _Eight(ops.FusedAdamWClip):                  # past the GPU refusals, on the host: the check itself
        def __init__(self):
            self.master_weights, self.moments_8bit, self.params = True, True, []
    with pytest.raises(LcvError, match="grad_accum > 1 needs moments_8bit=False"):
        _Eight()._init_accum(2)
    a, b = ops.FusedAdamWClip(bf), ops.FusedAdamWClip([torch.zeros(8)])
    b.grad_accum = 2
    with pytest.raises(LcvError, match="grad_accum > 1 cannot take part in a joint clip"):
        ops.FusedAdamWClip.joint_clip_grad_norm_([a, b], 1.0)


def test_loops_take_grad_accum_keyword_only_and_keep_master_weights_last():
    from tta import delta, full_tta, inner_loop
    for fn in (inner_loop.finetune_lora_on_conditioning, inner_loop.finetune_lora_batch, full_tta.finetune_full_on_conditioning,
               full_tta.finetune_full_batch, delta.optimize_norm_params):
        params = list(inspect.signature(fn).parameters.values())
        names = [p.name for p in params]
        p = params[names.index("grad_accum")]
        assert p.default == 1 and p.kind is inspect.Parameter.KEYWORD_ONLY, fn.__name__
        assert names[-3:] == ["grad_accum", "moments_8bit", "master_weights"], fn.__name__
    eng = inspect.signature(inner_loop.run_adaptation).parameters
    assert list(eng)[-2:] == ["finish_eval", "grad_accum"] and eng["grad_accum"].default == 1
    with pytest.raises(ValueError, match="at least 1"):
        inner_loop.run_adaptation(None, [torch.zeros(1)], [], None, None, 1, grad_accum=0)
    with pytest.raises(ValueError, match="fp32 parameters"):
        delta._optimize(None, [torch.zeros(4, dtype=torch.bfloat16), torch.zeros(4)], False, None, None, None, None, 1, 1e-3,
                        "cpu", torch.bfloat16, None, None, master_weights=True, grad_accum=2)


# ------------------------------------------------------------------------------------------------------------ the runners
def _script(rel):
    spec = importlib.util.spec_from_file_location("ga_" + Path(rel).stem, ROOT / "longcat-video-tta_amd" / rel)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


BASE = ["--checkpoint-dir", "synthetic", "--data-dir", "synthetic:1", "--output-dir", "x"]
RUNNERS = [("lora_experiment/scripts/run_lora_tta.py", False), ("lora_experiment/scripts/run_full_tta.py", True),
           ("delta_experiment/scripts/run_norm_tune_tta.py", False)]


@pytest.mark.parametrize("rel, has_optimizer", RUNNERS)
def test_runners_take_grad_accum_and_refuse_it_at_parse_time(rel, has_optimizer, capsys):
    mod = _script(rel)
    assert mod.parse_args(BASE).grad_accum == 1
    assert mod.parse_args(BASE + ["--grad-accum", "1"]).grad_accum == 1           # 1 needs nothing else
    args = mod.parse_args(BASE + ["--master-weights", "--grad-accum", "4"])
    assert args.grad_accum == 4 and args.master_weights is True
    adamw = ["--optimizer", "adamw"] if has_optimizer else []
    cases = [(["--grad-accum", "0"], "--grad-accum must be at least 1"),
             (["--master-weights", "--grad-accum", "-2"], "--grad-accum must be at least 1"),
             (["--grad-accum", "2"], "--grad-accum above 1 needs --master-weights"),
             (["--master-weights", "--adam-8bit", "--grad-accum", "2"] + adamw, "cannot be combined with --adam-8bit")]
    if "norm_tune" in rel:
        cases.append((["--master-weights", "--also-tune-delta", "--grad-accum", "2"], "cannot be combined with --also-tune-delta"))
    for argv, message in cases:
        capsys.readouterr()
        with pytest.raises(SystemExit) as e:
            mod.parse_args(BASE + argv)
        err = capsys.readouterr().err
        assert e.value.code == 2 and message in err, (argv, err)
        assert len([ln for ln in err.strip().splitlines() if "error:" in ln]) == 1


def test_delta_and_film_runners_do_not_take_the_flag():
    for rel in ("delta_experiment/scripts/run_delta_a.py", "delta_experiment/scripts/run_film_tta.py"):
        opts = {s for a in _script(rel).build_parser()._actions for s in a.option_strings}
        assert "--grad-accum" not in opts, rel
    for rel, _ in RUNNERS:
        opts = {s for a in _script(rel).build_parser()._actions for s in a.option_strings}
        assert "--grad-accum" in opts, rel

"""CPU: the sharpness-aware adaptation step (`--sam-rho`, include/lcv_hip_sam.h).  The numpy restatement (tests/sam_ref.py) is held
to float64 within the bound its docstring derives; the header is held to the rules the other headers are held to; the parser
refuses what the feature cannot do, each with one line and exit status 2; the loop replays the generator between its two passes;
nothing new is written when the flag is off."""
import argparse
import ctypes
import importlib.util
import inspect
import math
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import master_weights_ref as W
import sam_ref as S
import trust_ref as T

ROOT = Path(__file__).resolve().parents[1]
PKG = ROOT / "longcat-video-tta_amd"
HEADER = "lcv_hip_sam.h"
NAMES = {"lcv_sam_sumsq", "lcv_sam_perturb", "lcv_sam_restore"}
F = np.float32
SIZES = (1, 7, 512, 2049, 4099, 200000)


# ------------------------------------------------------------------------------------------------------------ the restatement
def _f32_tensor(seed, n):
    rng = np.random.default_rng(seed)
    return {"w": W.master(*W.weights(rng, n)), "g": W.bf16_to_f32(W.grads(rng, n))}


def _bf16_tensor(seed, n, low=True):
    rng = np.random.default_rng(seed)
    h, lw = W.weights(rng, n)
    return {"h": h, "low": lw if low else None, "g": W.grads(rng, n)}


@pytest.mark.parametrize("n", SIZES)
def test_the_plain_perturbation_has_norm_rho_within_the_derived_bound(n):
    rho = 0.05
    ts = [_f32_tensor(3, n), _f32_tensor(4, 300)]
    got = S.perturb(ts, rho)
    assert got["wrote"] and got["trace"][0] == got["sumsq"][1][0]
    d = [np.asarray(wp, np.float64) - np.asarray(t["w"], np.float64) for wp, t in zip(got["words"], ts)]
    norm, theta = S.norm64(d), S.norm64(got["words"])
    eps = S.eps_rho([n, 300])
    assert abs(norm - float(F(rho))) <= float(F(rho)) * eps + T.U * theta, (n, norm, eps)
    # and the direction is the gradient's: element by element against the float64 evaluation rho g / |g|
    g = [np.asarray(t["g"], np.float64) for t in ts]
    scale = float(F(rho)) / S.norm64(g)
    for di, gi, wp in zip(d, g, got["words"]):
        assert np.all(np.abs(di - scale * gi) <= np.abs(scale * gi) * eps + T.U * np.abs(np.asarray(wp, np.float64)))
    # the reported realized norm is the same figure up to its own summation error
    assert abs(float(got["realized"][1]) - float(F(rho))) <= float(F(rho)) * S.eps_realized([n, 300]) + T.U * theta
    assert got["realized"][1] == np.sqrt(got["realized"][0]) and got["trace"][1] == got["realized"][0]


@pytest.mark.parametrize("eta", [0.01, 0.0])
@pytest.mark.parametrize("n", SIZES)
def test_the_adaptive_perturbation_has_norm_rho_in_the_scaled_norm(n, eta):
    rho = 0.05
    ts = [_f32_tensor(5, n), _f32_tensor(6, 300)]
    got = S.perturb(ts, rho, adaptive=True, eta=eta)
    a = [np.abs(np.asarray(t["w"], np.float64)) + float(F(eta)) for t in ts]
    d = [(np.asarray(wp, np.float64) - np.asarray(t["w"], np.float64)) / ai for wp, t, ai in zip(got["words"], ts, a)]
    theta = S.norm64([np.asarray(wp, np.float64) / ai for wp, ai in zip(got["words"], a)])
    eps = S.eps_rho([n, 300], adaptive=True)
    assert abs(S.norm64(d) - float(F(rho))) <= float(F(rho)) * eps + T.U * theta, (n, eta, S.norm64(d))
    # the float64 evaluation of ASAM: e = rho T^2 g / |T g|, T = |w| + eta
    tg = [ai * np.asarray(t["g"], np.float64) for ai, t in zip(a, ts)]
    scale = float(F(rho)) / S.norm64(tg)
    for di, ti, wp, ai in zip(d, tg, got["words"], a):
        assert np.all(np.abs(di - scale * ti) <= np.abs(scale * ti) * eps + T.U * np.abs(np.asarray(wp, np.float64)) / ai)
    # the sum it was normalised by is the scaled gradient's
    exact = sum(float(np.sum(x * x)) for x in tg)
    k = T.depth([n, 300]) + 5
    assert abs(float(got["sumsq"][1][0]) - exact) <= ((1 + T.U) ** k - 1) * exact


def test_bf16_words_round_the_perturbation_and_realized_says_so():
    """A perturbation below half an ulp of its element rounds away, one above becomes a whole ulp: realized is not rho."""
    for low in (True, False):
        ts = [_bf16_tensor(7, 4099, low), _bf16_tensor(8, 7, low)]
        got = S.perturb(ts, 0.05)
        moved = sum(int(np.count_nonzero(hp != t["h"])) for hp, t in zip(got["words"], ts))
        assert 0 < moved < 4106
        d = [W.bf16_to_f32(hp).astype(np.float64) - W.bf16_to_f32(t["h"]).astype(np.float64) for hp, t in zip(got["words"], ts)]
        exact = sum(float(np.sum(x * x)) for x in d)
        k = T.depth([4099, 7]) + 3
        assert abs(float(got["realized"][0]) - exact) <= ((1 + T.U) ** k - 1) * exact
        for s, t in zip(got["saves"], ts):
            assert np.array_equal(s, t["h"]) and s is not t["h"]
        back = S.restore(got["saves"])
        assert all(np.array_equal(b, t["h"]) for b, t in zip(back, ts))
    one = _bf16_tensor(7, 4099)
    small, huge = S.perturb([one], 0.05), S.perturb([one], 100.0)        # a large rho moves more words, and further
    assert np.count_nonzero(huge["words"][0] != one["h"]) > np.count_nonzero(small["words"][0] != one["h"])
    assert huge["realized"][1] > small["realized"][1] and np.isfinite(huge["realized"][1])


@pytest.mark.parametrize("form", ["f32", "bf16"])
def test_rho_zero_a_zero_total_and_a_nan_total_write_nothing(form):
    make = _f32_tensor if form == "f32" else _bf16_tensor
    key = "w" if form == "f32" else "h"
    ts = [make(9, 2049), make(10, 7)]
    zero_g = [dict(t, g=np.zeros_like(t["g"])) for t in ts]
    cases = [("rho 0", ts, 0.0, None), ("zero total", zero_g, 0.05, None), ("nan total", ts, 0.05, F(np.nan)),
             ("inf total", ts, 0.05, F(np.inf)), ("negative total", ts, 0.05, F(-1.0))]
    for what, tensors, rho, total in cases:
        for adaptive in (False, True):
            got = S.perturb(tensors, rho, adaptive=adaptive, total=total)
            assert not got["wrote"], what
            assert all(wd is t[key] for wd, t in zip(got["words"], tensors)), what   # nothing written
            assert all(np.array_equal(s, t[key]) for s, t in zip(got["saves"], tensors)), what                   # the saves are
            assert not got["realized"].any() and not got["per"].any() and got["trace"][1] == 0, what
    assert S.sumsq(zero_g)[1][0] == 0 and S.coef(F(0), 0.05) is None and S.coef(F(4.0), 0.0) is None
    assert S.coef(F(np.nan), 0.05) is None and S.coef(F(np.inf), 0.05) is None
    assert S.coef(F(4.0), 0.5) == F(F(0.5) / F(F(2.0) + F(1e-12)))
    assert S.joint_total([F(1.0), F(2.0 ** -25), F(2.0 ** -25)]) == F(1.0)            # added in order, in fp32


# ------------------------------------------------------------------------------------------------------------ the header
def _declared(header: str):
    txt = (ROOT / "include" / header).read_text()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(lcv_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", txt, flags=re.S)}


def _built():
    sys.path.insert(0, str(ROOT))
    import __graft_entry__ as ge
    ge.build()
    from lcv_hip import lib
    return lib, ctypes.CDLL(str(lib.lib_path()))


def test_sam_header_symbols_are_exported_and_bound_in_a_table_of_their_own():
    lib, so = _built()
    protos = _declared(HEADER)
    assert set(protos) == NAMES == set(lib._SIGNATURES_SAM)
    for name, args in protos.items():
        assert hasattr(so, name), name
        assert len(args.split(",")) == len(lib._SIGNATURES_SAM[name]), name
        assert args.split(",")[-1].strip() == "void* stream", name
    assert {n: len(protos[n].split(",")) for n in NAMES} == {"lcv_sam_sumsq": 12, "lcv_sam_perturb": 16, "lcv_sam_restore": 6}
    P, I64, I, F64 = lib.P, lib.I64, lib.I, lib.F64
    assert lib._SIGNATURES_SAM["lcv_sam_sumsq"] == [P, P, I64, I64, I, I, F64, P, I64, P, P, P]
    assert lib._SIGNATURES_SAM["lcv_sam_perturb"] == [P, P, P, I64, I64, I, I, F64, F64, P, P, I64, P, P, P, P]
    assert lib._SIGNATURES_SAM["lcv_sam_restore"] == [P, P, I64, I64, I, P]
    loaded = lib.load()
    for n in NAMES:
        assert getattr(loaded, n).argtypes == lib._SIGNATURES_SAM[n] and getattr(loaded, n).restype is ctypes.c_int
    so.lcv_version.restype = ctypes.c_int
    assert so.lcv_version() >= 17                     # went up with the new entry points
    for other in sorted((ROOT / "include").glob("*.h")):              # a header of its own: the others' lists are unchanged
        if other.name != HEADER:
            txt = other.read_text()
            assert HEADER not in txt and not any(n in txt for n in NAMES), other.name
    for table_name in [k for k in vars(lib) if k.startswith("_SIGNATURES") and k != "_SIGNATURES_SAM"]:
        assert not set(getattr(lib, table_name)) & NAMES, table_name
    assert set(lib._SIGNATURES_TRUST) == {"lcv_trust_sumsq", "lcv_trust_project"}     # the ball's entry points stay


def test_the_source_uses_no_atomics_and_the_header_writes_the_order_out():
    csrc = PKG / "csrc"
    src = (csrc / "optim_sam.hip").read_text()
    for word in ("atomic", "fmaf", "asm", "getenv", "lcv_knob(", "hipMalloc"):
        assert word not in src, word
    assert '#include "lcv_hip_sam.h"' in src and '#include "master_elem.h"' in src
    assert re.findall(r'extern "C" int (\w+)\(', src) == ["lcv_sam_sumsq", "lcv_sam_perturb", "lcv_sam_restore"]
    assert "master_join(" in src and "find_tensor(" in src and "optim_table_ok(" in src and "LCV_CHECK_ARG(" in src
    from lcv_hip import build
    assert build.EXTRA["optim_sam.hip"] == build.EXTRA["optim_trust.hip"] == ["-ffp-contract=off"]
    hdr = (ROOT / "include" / HEADER).read_text()
    for phrase in ("v = v + v[lane ^ o]", "((p0 + p1) + p2) + p3", "t, t + 256", "a = fabsf(w) + eta_f;  t = a * g",
                   "q = t * t;  acc = acc + q", "n = sqrtf(s);  den = n + 1e-12f;  c = rho_f / den", "u = a * t;  e = c * u",
                   "w' = w + e", "h' = bf16_rne(w')", "No atomics", "rounds away", "never written"):
        assert phrase in hdr, phrase


# ------------------------------------------------------------------------------------------------------------ the optimizers
@pytest.mark.parametrize("cls", ["FusedSGDClip", "FusedAdamWClip"])
def test_enable_sam_signature_and_host_side_refusals(cls):
    from lcv_hip import ops, optim
    from lcv_hip.lib import LcvError
    make = getattr(ops, cls)
    sig = inspect.signature(make.enable_sam).parameters
    assert list(sig) == ["self", "rho", "adaptive", "eta", "trace_len"]
    assert sig["adaptive"].default is False and sig["eta"].default == 0.01
    for name in ("sam_perturb", "sam_restore", "sam_stats"):
        assert callable(getattr(optim, name))
    opt = make([torch.zeros(8, dtype=torch.float32)])
    assert opt.sam_rho is None and opt.sam_perturbed is False and "sam" not in opt._tables and not hasattr(opt, "_sam_save")
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(LcvError, match="rho of enable_sam.. must be finite and >= 0"):
            opt.enable_sam(bad)
        with pytest.raises(LcvError, match="eta of enable_sam.. must be finite and >= 0"):
            opt.enable_sam(0.1, True, bad)
    with pytest.raises(LcvError, match="GPU"):                           # no CPU path
        opt.enable_sam(0.1)
    for call in (opt.sam_trace, lambda: optim.sam_perturb([opt]), lambda: optim.sam_restore([opt]), lambda: optim.sam_stats([opt])):
        with pytest.raises(LcvError, match="needs enable_sam"):
            call()
    assert opt.sam_rho is None


# ------------------------------------------------------------------------------------------------------------ the loop
class _StubOpt:
    def __init__(self):
        self.zeroed = 0

    def zero_grad(self, set_to_none=True):
        self.zeroed += 1


def test_the_second_pass_replays_the_generator_and_leaves_it_where_a_plain_step_would():
    from tta import inner_loop as L
    p = torch.nn.Parameter(torch.ones(3))
    draws, events = [], []

    def loss_at(step):
        r, k = torch.rand(3), torch.randint(0, 1000, (1,)).item()
        draws.append((r.clone(), k))
        events.append("forward")
        return (p * r).sum() * (k + 1)
    opt = _StubOpt()
    torch.manual_seed(5)
    loss, loss_p = L.sam_two_passes([opt], loss_at, 0, lambda: events.append("sync"), lambda o: events.append("perturb"),
                                    lambda o: events.append("restore"), "cpu")
    after = torch.get_rng_state()
    assert events == ["forward", "sync", "perturb", "forward", "sync", "restore"] and opt.zeroed == 1
    assert torch.equal(draws[0][0], draws[1][0]) and draws[0][1] == draws[1][1]       # the second call sees the first's draws
    assert loss.item() == loss_p.item() and p.grad is not None
    torch.manual_seed(5)
    loss_at(0)                                                                       # a plain step draws once
    assert torch.equal(torch.get_rng_state(), after)                                 # and the stream stands where SAM left it
    assert torch.equal(draws[2][0], draws[0][0])


def test_the_engine_and_the_loops_take_the_keywords_and_refuse_what_they_must():
    from tta import delta, full_tta, inner_loop
    eng = inspect.signature(inner_loop.run_adaptation).parameters
    assert list(eng)[-4:] == ["sam", "after_step", "finish_eval", "grad_accum"] and eng["sam"].default is None
    for fn in (inner_loop.finetune_lora_on_conditioning, inner_loop.finetune_lora_batch, full_tta.finetune_full_on_conditioning,
               full_tta.finetune_full_batch, delta.optimize_norm_params, delta.optimize_delta_a, delta.optimize_delta_b,
               delta.optimize_delta_c, delta.optimize_film_adapter):
        p = inspect.signature(fn).parameters
        assert p["sam_rho"].default is None and p["sam_adaptive"].default is False and p["sam_eta"].default == 0.01, fn.__name__
    assert inner_loop.sam_hook([], None, False, 0.01, 4) is None         # no rho: nothing is built
    lora = dict(lora_param_fn=lambda: [torch.nn.Parameter(torch.zeros(4, dtype=torch.bfloat16))])
    plain, sp = argparse.Namespace(_sp_group=None), argparse.Namespace(_sp_group=object())
    for fn, args in ((inner_loop.finetune_lora_on_conditioning, (plain, [], None, None, None, None)),
                     (inner_loop.finetune_lora_batch, (plain, [], []))):
        with pytest.raises(ValueError, match="sam_rho cannot be combined with DoRA magnitudes"):
            fn(*args, dora_magnitudes=[torch.nn.Parameter(torch.ones(4))], sam_rho=0.1, **lora)
        with pytest.raises(ValueError, match="sam_rho cannot be combined with grad_accum > 1"):
            fn(*args, sam_rho=0.1, grad_accum=2, master_weights=True, **lora)
        with pytest.raises(ValueError, match="sam_rho cannot be combined with sequence parallelism"):
            fn(sp, *args[1:], sam_rho=0.0, **lora)
    with pytest.raises(ValueError, match="sam_rho cannot be combined with grad_accum > 1"):
        inner_loop.run_adaptation(None, [torch.zeros(1)], [], None, None, 1, sam=object(), grad_accum=2)
    with pytest.raises(ValueError, match="sam_rho cannot be combined with sequence parallelism"):
        inner_loop.refuse_sam(argparse.Namespace(dit=sp), 0.1)
    inner_loop.refuse_sam(sp, None, grad_accum=2, dora_magnitudes=[1])   # no rho: nothing is refused


# ------------------------------------------------------------------------------------------------------------ the runners
def _script(rel):
    spec = importlib.util.spec_from_file_location("sam_" + Path(rel).stem, PKG / rel)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


BASE = ["--checkpoint-dir", "synthetic", "--data-dir", "synthetic:1", "--output-dir", "x"]
LORA, FULL = "lora_experiment/scripts/run_lora_tta.py", "lora_experiment/scripts/run_full_tta.py"
NORM = "delta_experiment/scripts/run_norm_tune_tta.py"
VECTORS = ["delta_experiment/scripts/run_delta_a.py", "delta_experiment/scripts/run_delta_b.py",
           "delta_experiment/scripts/run_delta_c.py", "delta_experiment/scripts/run_film_tta.py"]


def _parse(mod, argv):
    from tta import cli_args as C
    if hasattr(mod, "parse_args"):
        return mod.parse_args(argv)
    return C.parse_with_step_cache(mod.build_parser(), argv)             # what the vector runners' main() does


def _refused(mod, argv, message, capsys):
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        _parse(mod, BASE + argv)
    err = capsys.readouterr().err
    assert e.value.code == 2 and message in err, (argv, err)
    assert len([ln for ln in err.strip().splitlines() if "error:" in ln]) == 1


@pytest.mark.parametrize("rel", [LORA, FULL, NORM] + VECTORS)
def test_every_adapting_runner_takes_the_flags_and_refuses_at_parse_time(rel, capsys):
    from tta import cli_args as C
    mod = _script(rel)
    off = _parse(mod, BASE)
    assert off.sam_rho is None and off.sam_adaptive is False and off.sam_eta is None
    assert C.sam_kwargs(off) == C.sam_record(off) == {} and C.sam_result({"losses": []}) == {}          # flag absent: nothing
    on = _parse(mod, BASE + ["--sam-rho", "0.05"])
    assert C.sam_kwargs(on) == C.sam_record(on) == {"sam_rho": 0.05, "sam_adaptive": False, "sam_eta": 0.01}
    on = _parse(mod, BASE + ["--sam-rho", "0", "--sam-adaptive", "--sam-eta", "0.1"])
    assert C.sam_kwargs(on) == {"sam_rho": 0.0, "sam_adaptive": True, "sam_eta": 0.1}
    assert C.sam_kwargs(_parse(mod, BASE + ["--sam-rho", "1", "--sam-adaptive"]))["sam_eta"] == 0.01
    assert C.sam_result({"sam": {"steps": 2}, "losses": []}) == {"sam": {"steps": 2}}
    _refused(mod, ["--sam-adaptive"], "--sam-adaptive needs --sam-rho RHO", capsys)
    _refused(mod, ["--sam-eta", "0.1"], "--sam-eta needs --sam-rho RHO", capsys)
    _refused(mod, ["--sam-rho", "0.1", "--sam-eta", "0.1"], "--sam-eta needs --sam-adaptive", capsys)
    for bad in ("-0.5", "nan", "inf"):
        _refused(mod, ["--sam-rho", bad], "--sam-rho RHO must be finite and >= 0", capsys)
        _refused(mod, ["--sam-rho", "0.1", "--sam-adaptive", "--sam-eta", bad], "--sam-eta ETA must be finite and >= 0", capsys)
    if rel in (LORA, FULL, NORM):
        _refused(mod, ["--sam-rho", "0.1", "--master-weights", "--grad-accum", "2"],
                 "--sam-rho cannot be combined with --grad-accum above 1", capsys)
        assert C.optimizer_kwargs(on)["sam_rho"] == 0.0 and "sam_rho" not in C.optimizer_kwargs(off)
        # what stays allowed
        adamw = ["--optimizer", "adamw"] if rel == FULL else []
        for extra in (["--master-weights"], ["--master-weights", "--adam-8bit"] + adamw, ["--master-weights", "--weight-ema", "0.9"],
                      ["--stochastic-rounding"], ["--master-weights", "--max-drift", "1"]):
            assert _parse(mod, BASE + ["--sam-rho", "0.1"] + extra).sam_rho == 0.1
        if rel != LORA:
            assert _parse(mod, BASE + ["--sam-rho", "0.1", "--master-weights", "--decay-to-base"]).decay_to_base is True
    if rel == LORA:
        _refused(mod, ["--sam-rho", "0.1", "--lora-dora"], "--sam-rho cannot be combined with --lora-dora", capsys)
        assert _parse(mod, BASE + ["--sam-rho", "0.1", "--lora-dropout", "0.1"]).sam_rho == 0.1
    assert _parse(mod, BASE + ["--sam-rho", "0.1", "--es-disable"]).es_disable is True                  # with or without the stopper


def test_the_baseline_runner_does_not_take_the_flags():
    opts = {s for a in _script("baseline_experiment/scripts/run_baseline.py").build_parser()._actions for s in a.option_strings}
    assert not opts & {"--sam-rho", "--sam-adaptive", "--sam-eta"}


def test_vector_runners_hand_the_keywords_to_their_loop_only_with_the_flag(monkeypatch):
    for rel in VECTORS:
        mod = _script(rel)
        seen = []
        monkeypatch.setattr(mod.R, "run_delta_method", lambda args, method, **kw: seen.append(kw))
        name = next(n for n in dir(mod) if n.startswith("optimize_"))
        called = {}
        monkeypatch.setattr(mod, name, lambda *a, **kw: called.update(kw=kw) or {})
        mod.main(BASE)
        mod.main(BASE + ["--sam-rho", "0.5", "--sam-adaptive"])
        off, on = seen
        off["optimize_fn"](None, None, None, None, None, "cpu", None)
        assert not [k for k in called["kw"] if k.startswith("sam_")], rel
        on["optimize_fn"](None, None, None, None, None, "cpu", None)
        assert (called["kw"]["sam_rho"], called["kw"]["sam_adaptive"], called["kw"]["sam_eta"]) == (0.5, True, 0.01), rel


def test_runner_files_have_no_new_key_with_the_flag_off(monkeypatch, tmp_path):
    """config.json / summary.json of jobs over no videos, with a stand-in model: the flag's keys are there exactly when the flag
    is (config.json `training` for the LoRA and full-model runners, the flat summary.json for the others)."""
    import json
    full = _script(FULL)
    net = torch.nn.Linear(4, 4).to(torch.bfloat16)
    monkeypatch.setattr(full.R, "setup_distributed", lambda args: (0, 1, "cpu"))
    monkeypatch.setattr(full.R, "load_components", lambda args, device: (net, None))
    monkeypatch.setattr(full.R, "list_eval_entries", lambda args, dit: [])
    files = {}
    for name, flags in (("off", []), ("on", ["--sam-rho", "0.5"])):
        out = tmp_path / name
        full.main(["--checkpoint-dir", "synthetic", "--data-dir", "synthetic:1", "--output-dir", str(out), "--es-disable"] + flags)
        files[name] = (json.loads((out / "config.json").read_text()), json.loads((out / "summary.json").read_text()))
    (c_off, s_off), (c_on, s_on) = files["off"], files["on"]
    assert set(c_on["training"]) - set(c_off["training"]) == {"sam_rho", "sam_adaptive", "sam_eta"} and set(c_on) == set(c_off)
    assert (c_on["training"]["sam_rho"], c_on["training"]["sam_adaptive"], c_on["training"]["sam_eta"]) == (0.5, False, 0.01)
    assert set(s_on) == set(s_off) and '"sam"' not in json.dumps(s_off) and "sam_" not in json.dumps(c_off)
    delta = _script(VECTORS[0])
    for name, flags in (("d_off", []), ("d_on", ["--sam-rho", "0", "--sam-adaptive", "--sam-eta", "0.2"])):
        out = tmp_path / name
        delta.main(["--checkpoint-dir", "synthetic", "--data-dir", "synthetic:1", "--output-dir", str(out), "--es-disable"] + flags)
        files[name] = json.loads((out / "summary.json").read_text())
    assert set(files["d_on"]) - set(files["d_off"]) == {"sam_rho", "sam_adaptive", "sam_eta"}
    assert files["d_on"]["sam_rho"] == 0.0 and files["d_on"]["sam_eta"] == 0.2 and "sam_" not in json.dumps(files["d_off"])
    assert math.isfinite(files["d_on"]["sam_rho"])

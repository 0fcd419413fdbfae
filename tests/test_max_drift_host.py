"""CPU: the trust-region cap on the drift from the base weights (`--max-drift`, include/lcv_hip_trust.h).  The numpy restatement
(tests/trust_ref.py) is held to float64 within bounds derived from its documented reduction depth; the header is held to the
rules the other headers are held to; the parser refuses what the feature cannot do, each with one line and exit status 2; the
optimizers, the loops and the runners take the flag and write nothing new when it is off."""
import argparse
import ctypes
import importlib.util
import inspect
import json
import math
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import anchor_ref as A
import master_weights_ref as W
import trust_ref as T

ROOT = Path(__file__).resolve().parents[1]
PKG = ROOT / "longcat-video-tta_amd"
HEADER = "lcv_hip_trust.h"
NAMES = {"lcv_trust_sumsq", "lcv_trust_project"}
F = np.float32
SIZES = (1, 7, 512, 2049, 4099, 200000)


# ------------------------------------------------------------------------------------------------------------ the restatement
def _tensor(seed, n, f32=False, zero_base=False):
    rng = np.random.default_rng(seed)
    h, low = W.weights(rng, n)
    h0 = W.to_bf16_bits(W.master(h, low) * F(1.015625)) if n < 5 else None
    if h0 is None:
        h0, low = A.anchors(rng, h, low)
    if zero_base:
        return T.from_words(h, low, None)
    if f32:
        return W.master(h, low), W.master(h0, rng.integers(-3000, 3000, size=n).astype(np.int16))
    return T.from_words(h, low, h0)


def _exact_sumsq(tensors):
    """The sum of squares of the exact drifts, added sequentially in float64 (math.fsum: correctly rounded)."""
    terms = []
    for w, w0 in tensors:
        d = np.asarray(w, dtype=np.float64) - np.asarray(w0, dtype=np.float64)
        terms.append(math.fsum((d * d).tolist()))
    return math.fsum(terms)


@pytest.mark.parametrize("n", SIZES)
def test_the_fixed_order_sum_is_within_its_derived_bound_of_float64(n):
    for k, kw in enumerate((dict(), dict(f32=True), dict(zero_base=True))):
        t = [_tensor(10 + k, n, **kw)]
        per, out = T.sumsq(t)
        exact = _exact_sumsq(t)
        bound = (1.0 + T.U) ** (T.depth([n]) + 3) - 1.0
        assert exact > 0 and abs(float(out[0]) - exact) <= bound * exact, (n, kw, float(out[0]), exact)
        assert per.dtype == F and per[0] == out[0] and out[1] == np.sqrt(out[0])      # one tensor: its sum is the total
    assert T.depth([n]) == 17 + 10 + 10 and T.eps_s([n]) <= T.EPS_S


@pytest.mark.parametrize("scope", ["global", "tensor"])
@pytest.mark.parametrize("n", SIZES)
def test_a_projection_holds_the_radius_within_the_stated_bound(n, scope):
    """|theta' - theta0| <= sqrt(r2) (1 + eps_s) + 2^-24 |theta'|, the norms as sequential float64 sums, eps_s = 2^-17."""
    for k, kw in enumerate((dict(), dict(f32=True), dict(zero_base=True))):
        t = [_tensor(20 + k, n, **kw), _tensor(30 + k, 300, **kw)]
        count = n + 300
        R = 0.5 * min(math.sqrt(_exact_sumsq([x]) / np.size(x[0])) for x in t)         # every ball is exceeded
        new, per, out, (s, cmin) = T.project(t, R, scope)
        assert s == out[0] and cmin < 1.0 and all(a is not b[0] for a, b in zip(new, t))
        after = [(w, x[1]) for w, x in zip(new, t)]
        theta = math.sqrt(math.fsum(float(v) ** 2 for w, _ in after for v in np.asarray(w, dtype=np.float64)))
        balls = [(after, count)] if scope == "global" else [([a], np.size(a[0])) for a in after]
        for pairs, m in balls:
            r2 = T.radius2(R, m)
            assert math.sqrt(_exact_sumsq(pairs)) <= math.sqrt(float(r2)) * (1.0 + T.EPS_S) + T.U * theta, (n, scope, kw)
            assert T.bound_holds(pairs, r2)
        # and not much below it either: the projection lands on the ball, not inside
        pairs, m = balls[0]
        assert math.sqrt(_exact_sumsq(pairs)) >= math.sqrt(float(T.radius2(R, m))) * (1.0 - 2.0 ** -10)


def test_inside_the_ball_and_on_a_nan_total_nothing_is_touched():
    t = [_tensor(40, 2049), _tensor(41, 7)]
    per, out = T.sumsq(t)
    big = 2.0 * math.sqrt(float(out[0]) / 2056)
    for scope in ("global", "tensor"):
        new, _, _, (s, cmin) = T.project(t, max(big, 2.0 * math.sqrt(float(per[1]) / 7)), scope)
        assert all(a is b[0] for a, b in zip(new, t)) and cmin == 1.0 and s == out[0]
        new, _, _, (s, cmin) = T.project(t, float("inf"), scope)
        assert all(a is b[0] for a, b in zip(new, t)) and cmin == 1.0
    new, _, _, (s, cmin) = T.project(t, 1e-9, "global", total=F(np.nan))
    assert all(a is b[0] for a, b in zip(new, t)) and cmin == 1.0 and np.isnan(s)
    assert T.coef(F(np.nan), F(1.0)) == 1.0 and T.coef(F(4.0), F(1.0)) == F(0.5) and T.coef(F(1.0), F(1.0)) == 1.0
    # tensor scope projects the tensors that exceed their ball and only them
    rms = np.sqrt(per.astype(np.float64) / np.array([2049, 7]))
    R = float(rms.min() * 1.01)
    new, _, _, _ = T.project(t, R, "tensor")
    moved = [a is not b[0] for a, b in zip(new, t)]
    assert moved == [bool(r > R) for r in rms] and sum(moved) == 1
    assert T.joint_total([F(1.0), F(2.0 ** -25), F(2.0 ** -25)]) == F(1.0)            # added in order, in fp32
    assert T.radius2(0.1, 3) == F(0.1 * 0.1 * 3.0)


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


def test_trust_header_symbols_are_exported_and_bound():
    lib, so = _built()
    protos = _declared(HEADER)
    assert set(protos) == NAMES == set(lib._SIGNATURES_TRUST)
    for name, args in protos.items():
        assert hasattr(so, name), name
        assert len(args.split(",")) == len(lib._SIGNATURES_TRUST[name]), name
    P, I64, I, F64 = lib.P, lib.I64, lib.I, lib.F64
    assert lib._SIGNATURES_TRUST["lcv_trust_sumsq"] == [P, P, P, I64, I64, I, P, I64, P, P, P]
    assert lib._SIGNATURES_TRUST["lcv_trust_project"] == [P, P, P, I64, I64, I, I, P, P, F64, P, P]
    assert (lib.LCV_TRUST_GLOBAL, lib.LCV_TRUST_TENSOR) == (0, 1)
    loaded = lib.load()
    for n in NAMES:
        assert getattr(loaded, n).argtypes == lib._SIGNATURES_TRUST[n] and getattr(loaded, n).restype is ctypes.c_int
    so.lcv_version.restype = ctypes.c_int
    assert so.lcv_version() >= 16                     # went up with the new entry points
    for other in sorted((ROOT / "include").glob("*.h")):              # a header of its own: the others' lists are unchanged
        if other.name != HEADER:
            txt = other.read_text()
            assert HEADER not in txt and not any(n in txt for n in NAMES), other.name
    # existing entry points stay: the drift norm of --decay-to-base is untouched
    assert hasattr(so, "lcv_master_drift_sumsq") and "lcv_master_drift_sumsq" in lib._SIGNATURES_ANCHOR


def test_the_source_uses_no_atomics_and_shares_the_format_and_the_element_function():
    csrc = PKG / "csrc"
    src = (csrc / "optim_trust.hip").read_text()
    for word in ("atomic", "fmaf", "asm", "getenv", "lcv_knob(", "hipMalloc"):
        assert word not in src, word
    assert '#include "lcv_hip_trust.h"' in src and '#include "master_elem.h"' in src
    assert re.findall(r'extern "C" int (\w+)\(', src) == ["lcv_trust_sumsq", "lcv_trust_project"]
    shared = (csrc / "master_elem.h").read_text()
    for fn in ("float master_trust_elem(", "float master_ema_elem(", "float master_join(", "void master_split("):
        assert shared.count(fn) == 1 and fn not in src, fn
    assert "master_trust_elem(" in src and "find_tensor(" in src and "optim_table_ok(" in src
    assert shared.index("float master_ema_elem(") < shared.index("float master_trust_elem(")
    from lcv_hip import build
    assert build.EXTRA["optim_trust.hip"] == build.EXTRA["optim_anchor.hip"] == ["-ffp-contract=off"]
    # the order is written into the header, which the restatement follows
    hdr = (ROOT / "include" / HEADER).read_text()
    for phrase in ("v = v + v[lane ^ o]", "((p0 + p1) + p2) + p3", "t, t + 256", "d = w - w0;  q = d * d;  acc = acc + q",
                   "d = w - w0;  u = c * d;  w = w0 + u", "t = r2 / s;  c = sqrtf(t)", "No atomics"):
        assert phrase in hdr, phrase


# ------------------------------------------------------------------------------------------------------------ the optimizers
@pytest.mark.parametrize("cls", ["FusedSGDClip", "FusedAdamWClip"])
def test_enable_max_drift_signature_and_host_side_refusals(cls):
    from lcv_hip import ops, optim
    from lcv_hip.lib import LcvError
    make = getattr(ops, cls)
    sig = inspect.signature(make.enable_max_drift).parameters
    assert list(sig) == ["self", "radius_rms", "scope", "anchor", "trace_len"]
    assert sig["scope"].default == "global" and sig["anchor"].default is None
    for name in ("project_max_drift", "max_drift_norm", "max_drift_stats"):
        assert callable(getattr(optim, name))
    for name in ("drift_sumsq", "max_drift_trace"):
        assert callable(getattr(make, name))
    bf, f32 = [torch.zeros(8, dtype=torch.bfloat16)], [torch.zeros(8, dtype=torch.float32)]
    opt = make(f32)
    assert opt.max_drift is None and "trust" not in opt._tables and not hasattr(opt, "_md_trace")   # nothing without the call
    for bad in (0.0, -2.0, float("nan")):
        with pytest.raises(LcvError, match="must be > 0"):
            opt.enable_max_drift(bad)
    with pytest.raises(LcvError, match="'global' or 'tensor'"):
        opt.enable_max_drift(1.0, scope="block")
    with pytest.raises(LcvError, match="needs master_weights=True .*half a bf16 ulp"):
        make(bf).enable_max_drift(1.0, anchor=[bf[0].clone()])
    with pytest.raises(LcvError, match="GPU"):                           # no CPU path
        opt.enable_max_drift(1.0)
    for call in (opt.drift_sumsq, opt.max_drift_trace, lambda: optim.project_max_drift([opt])):
        with pytest.raises(LcvError, match="needs enable_max_drift"):
            call()
    assert opt.max_drift is None


def test_the_engine_takes_after_step_in_front_of_the_pinned_tail():
    from tta import delta, full_tta, inner_loop
    eng = inspect.signature(inner_loop.run_adaptation).parameters
    assert list(eng)[-3:] == ["after_step", "finish_eval", "grad_accum"] and eng["after_step"].default is None
    for fn in (inner_loop.finetune_lora_on_conditioning, inner_loop.finetune_lora_batch, full_tta.finetune_full_on_conditioning,
               full_tta.finetune_full_batch, delta.optimize_norm_params, delta.optimize_delta_a, delta.optimize_delta_b,
               delta.optimize_delta_c, delta.optimize_film_adapter):
        p = inspect.signature(fn).parameters
        assert p["max_drift"].default is None and p["max_drift_scope"].default == "global", fn.__name__
    assert inner_loop.max_drift_hook([], None, "global", 4) is None      # no radius: nothing is built
    with pytest.raises(ValueError, match="DoRA"):
        inner_loop.finetune_lora_on_conditioning(argparse.Namespace(_sp_group=None), [], None, None, None, None,
                                                 lora_param_fn=lambda: [torch.nn.Parameter(torch.zeros(4, dtype=torch.bfloat16))],
                                                 dora_magnitudes=[torch.nn.Parameter(torch.ones(4))], max_drift=1.0)


# ------------------------------------------------------------------------------------------------------------ the runners
def _script(rel):
    spec = importlib.util.spec_from_file_location("md_" + Path(rel).stem, PKG / rel)
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
    bf16 = rel in (LORA, FULL, NORM)
    master = ["--master-weights"] if bf16 else []
    off = _parse(mod, BASE)
    assert off.max_drift is None and off.max_drift_scope is None
    assert C.max_drift_kwargs(off) == C.max_drift_record(off) == {} and C.max_drift_result({"losses": []}) == {}
    on = _parse(mod, BASE + master + ["--max-drift", "0.25"])
    assert C.max_drift_kwargs(on) == C.max_drift_record(on) == {"max_drift": 0.25, "max_drift_scope": "global"}
    on = _parse(mod, BASE + master + ["--max-drift", "inf", "--max-drift-scope", "tensor"])
    assert C.max_drift_kwargs(on) == {"max_drift": float("inf"), "max_drift_scope": "tensor"}
    loop = {"drift_norm": 1.5, "max_drift": {"steps": 2}, "losses": []}
    assert C.max_drift_result(loop) == {"drift_norm": 1.5, "max_drift": {"steps": 2}}
    for bad in ("0", "-0.5", "nan"):
        _refused(mod, master + ["--max-drift", bad], "--max-drift R must be > 0", capsys)
    _refused(mod, master + ["--max-drift-scope", "tensor"], "--max-drift-scope needs --max-drift R", capsys)
    _refused(mod, master + ["--max-drift", "1", "--max-drift-scope", "layer"], "invalid choice", capsys)
    if bf16:
        _refused(mod, ["--max-drift", "1"], "--max-drift needs --master-weights", capsys)
        _refused(mod, ["--max-drift", "1", "--stochastic-rounding"], "--max-drift cannot be combined with --stochastic-rounding",
                 capsys)
        # what stays allowed
        adamw = ["--optimizer", "adamw"] if rel == FULL else []
        for extra in (["--adam-8bit"] + adamw, ["--grad-accum", "2"], ["--weight-ema", "0.9"]):
            assert _parse(mod, BASE + master + ["--max-drift", "1"] + extra).max_drift == 1.0
        if rel != LORA:
            assert _parse(mod, BASE + master + ["--max-drift", "1", "--decay-to-base"]).decay_to_base is True
        assert C.optimizer_kwargs(on)["max_drift"] == float("inf") and "max_drift" not in C.optimizer_kwargs(off)
    if rel == LORA:
        _refused(mod, ["--max-drift", "1", "--lora-dora"], "--max-drift cannot be combined with --lora-dora", capsys)
    assert _parse(mod, BASE + master + ["--max-drift", "1", "--es-disable"]).es_disable is True      # with or without the stopper


def test_the_baseline_runner_does_not_take_the_flag():
    opts = {s for a in _script("baseline_experiment/scripts/run_baseline.py").build_parser()._actions for s in a.option_strings}
    assert "--max-drift" not in opts and "--max-drift-scope" not in opts


def test_vector_runners_hand_the_keywords_to_their_loop_only_with_the_flag(monkeypatch):
    for rel in VECTORS:
        mod = _script(rel)
        seen = []
        monkeypatch.setattr(mod.R, "run_delta_method", lambda args, method, **kw: seen.append(kw))
        name = next(n for n in dir(mod) if n.startswith("optimize_"))
        called = {}
        monkeypatch.setattr(mod, name, lambda *a, **kw: called.update(kw=kw) or {})
        mod.main(BASE)
        mod.main(BASE + ["--max-drift", "0.5", "--max-drift-scope", "tensor"])
        off, on = seen
        off["optimize_fn"](None, None, None, None, None, "cpu", None)
        assert "max_drift" not in called["kw"] and "max_drift_scope" not in called["kw"], rel
        on["optimize_fn"](None, None, None, None, None, "cpu", None)
        assert called["kw"]["max_drift"] == 0.5 and called["kw"]["max_drift_scope"] == "tensor", rel


def test_runner_files_have_no_new_key_with_the_flag_off(monkeypatch, tmp_path):
    """config.json / summary.json of jobs over no videos, with a stand-in model: the flag's keys are there exactly when the flag
    is (config.json `training` for the LoRA and full-model runners, the flat summary.json for the others)."""
    full = _script(FULL)
    net = torch.nn.Linear(4, 4).to(torch.bfloat16)
    monkeypatch.setattr(full.R, "setup_distributed", lambda args: (0, 1, "cpu"))
    monkeypatch.setattr(full.R, "load_components", lambda args, device: (net, None))
    monkeypatch.setattr(full.R, "list_eval_entries", lambda args, dit: [])
    files = {}
    for name, flags in (("off", []), ("on", ["--max-drift", "0.5"])):
        out = tmp_path / name
        full.main(["--checkpoint-dir", "synthetic", "--data-dir", "synthetic:1", "--output-dir", str(out), "--es-disable",
                   "--master-weights"] + flags)
        files[name] = (json.loads((out / "config.json").read_text()), json.loads((out / "summary.json").read_text()))
    (c_off, s_off), (c_on, s_on) = files["off"], files["on"]
    assert set(c_on["training"]) - set(c_off["training"]) == {"max_drift", "max_drift_scope"} and set(c_on) == set(c_off)
    assert c_on["training"]["max_drift"] == 0.5 and c_on["training"]["max_drift_scope"] == "global"
    assert set(s_on) == set(s_off) and "max_drift" not in json.dumps(s_off) and "max_drift" not in json.dumps(c_off)
    delta = _script(VECTORS[0])
    for name, flags in (("d_off", []), ("d_on", ["--max-drift", "inf"])):
        out = tmp_path / name
        delta.main(["--checkpoint-dir", "synthetic", "--data-dir", "synthetic:1", "--output-dir", str(out), "--es-disable"] + flags)
        files[name] = json.loads((out / "summary.json").read_text())
    assert set(files["d_on"]) - set(files["d_off"]) == {"max_drift", "max_drift_scope"}
    assert files["d_on"]["max_drift"] == float("inf") and "max_drift" not in json.dumps(files["d_off"])

"""CPU: the numpy restatement of decay toward the base weights (tests/anchor_ref.py) is tied to the pinned master-weight steps
(zero base words give the SGD step's bits, weight decay 0 gives the AdamW steps' bits); include/lcv_hip_anchor.h is held to the
rules the other headers are held to; the optimizers, the loops and the runners take `anchor` / `decay_to_base` /
`--decay-to-base`, refuse it without master weights, and write nothing new when it is off."""
import ctypes
import importlib.util
import inspect
import json
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import anchor_ref as A
import grad_accum_ref as G
import master_weights_ref as W
import moments8_ref as M8

ROOT = Path(__file__).resolve().parents[1]
HEADER = "lcv_hip_anchor.h"
F = np.float32
NAMES = {"lcv_master_sgd_step_anchor", "lcv_master_adamw_step_anchor", "lcv_master_adamw8_step_anchor", "lcv_master_drift_sumsq"}


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
    h0, low = A.anchors(rng, h, low)
    return h, low, h0, [W.grads(rng, n) for _ in range(3)]


def test_anchor_generator_gives_small_offsets_and_fixed_points():
    h, low, h0, _ = _inputs(1)
    w, w0 = W.master(h, low).astype(np.float64), W.bf16_to_f32(h0).astype(np.float64)
    assert np.array_equal(h0[::5], h[::5]) and not low[::5].any() and np.all(w[::5] == w0[::5])
    rel = np.abs(w0 - w) / np.abs(w)
    rest = np.ones(h.size, dtype=bool)
    rest[::5] = False
    # |delta| in [2^-12, 2^-4], then one bf16 rounding of relative size at most 2^-9
    assert rel[rest].max() <= 2.0 ** -4 + 2.0 ** -8 and (rel[rest] > 0).mean() > 0.5


@pytest.mark.parametrize("coef", [1.0, 0.37])
@pytest.mark.parametrize("wd", [0.0, 0.01, 0.5])
def test_sgd_with_zero_base_words_gives_the_pinned_steps_bits(coef, wd):
    h, low, _, gs = _inputs(2)
    zero = np.zeros(h.size, dtype=np.uint16)
    hp, lp, hg, lg = h, low, h, low
    for g in gs:
        h, low = A.sgd_step_anchor(h, low, zero, g, coef, 0.05, wd)
        hp, lp = W.sgd_step(hp, lp, g, coef, 0.05, wd)
        assert np.array_equal(h, hp) and np.array_equal(low, lp)
        g32 = G.accumulate(np.zeros(g.size, dtype=F), g, 1.0)
        hg, lg = A.sgd_step_anchor(hg, lg, zero, g32, coef, 0.05, wd, grad_f32=True)
        assert np.array_equal(hg, hp) and np.array_equal(lg, lp)
    assert (h != _inputs(2)[0]).any()


@pytest.mark.parametrize("coef", [1.0, 0.37])
def test_adamw_at_zero_weight_decay_gives_the_pinned_steps_bits(coef):
    h, low, h0, gs = _inputs(3)
    m = v = np.zeros(h.size, dtype=F)
    hp, lp, mp, vp = h, low, m, v
    h8, l8, st = h, low, M8.zero_state(h.size)
    hq, lq, sq = h, low, M8.zero_state(h.size)
    for k, g in enumerate(gs):
        h, low, m, v = A.adamw_step_anchor(h, low, h0, m, v, g, coef, 1e-3, 0.9, 0.999, 1e-8, 0.0, k + 1)
        hp, lp, mp, vp = W.adamw_step(hp, lp, mp, vp, g, coef, 1e-3, 0.9, 0.999, 1e-8, 0.0, k + 1)
        assert np.array_equal(h, hp) and np.array_equal(low, lp)
        assert np.array_equal(W.bits(m), W.bits(mp)) and np.array_equal(W.bits(v), W.bits(vp))
        h8, l8, *st = A.adamw8_step_anchor(h8, l8, h0, *st, g, coef, 1e-3, 0.9, 0.999, 1e-8, 0.0, k + 1)
        hq, lq, *sq = M8.adamw8_step(hq, lq, *sq, g, coef, 1e-3, 0.9, 0.999, 1e-8, 0.0, k + 1)
        assert np.array_equal(h8, hq) and np.array_equal(l8, lq) and all(np.array_equal(a, b) for a, b in zip(st, sq))


def test_decay_is_a_pull_toward_the_base_and_the_base_is_its_fixed_point():
    h, low, h0, gs = _inputs(4)
    zero_g = np.zeros(h.size, dtype=np.uint16)
    w0 = W.bf16_to_f32(h0).astype(np.float64)
    # at the base, with no gradient, nothing moves - under the plain decay the same words erode
    at0 = np.zeros(h.size, dtype=np.int16)
    hs, ls = A.sgd_step_anchor(h0, at0, h0, zero_g, 1.0, 0.1, 0.5)
    assert np.array_equal(hs, h0) and not ls.any()
    ha, la, _, _ = A.adamw_step_anchor(h0, at0, h0, np.zeros(h.size, F), np.zeros(h.size, F), zero_g, 1.0, 0.1, 0.9, 0.999, 1e-8,
                                       0.5, 1)
    assert np.array_equal(ha, h0) and not la.any()
    hp, lp = W.sgd_step(h0, at0, zero_g, 1.0, 0.1, 0.5)
    assert (hp != h0).any() or lp.any()
    # away from it, every element comes closer and the drift falls
    before = A.drift_sumsq([(h, low, h0)])
    dist = np.abs(W.master(h, low).astype(np.float64) - w0)
    for _ in range(5):
        h, low = A.sgd_step_anchor(h, low, h0, zero_g, 1.0, 0.1, 0.5)
        now = np.abs(W.master(h, low).astype(np.float64) - w0)
        assert np.all(now <= dist)
        dist = now
        after = A.drift_sumsq([(h, low, h0)])
        assert after < before
        before = after


def test_drift_sumsq_is_the_float64_sum_and_treats_missing_low_words_as_zero():
    h, low, h0, _ = _inputs(5, n=3000)
    d = W.master(h, low).astype(np.float64) - W.bf16_to_f32(h0).astype(np.float64)
    assert A.drift_sumsq([(h, low, h0)]) == pytest.approx(float(np.dot(d, d)), rel=1e-12)
    assert A.drift_sumsq([(h, None, h0)]) == A.drift_sumsq([(h, np.zeros(h.size, np.int16), h0)])
    assert A.drift_sumsq([(h0, None, h0)]) == 0.0
    assert A.drift_sumsq([(h[:10], low[:10], h0[:10]), (h[10:], low[10:], h0[10:])]) == pytest.approx(float(np.dot(d, d)), rel=1e-12)


# ------------------------------------------------------------------------------------------------------------ the header
def test_anchor_header_symbols_are_exported_and_bound():
    lib, so = _built()
    names = _declared(HEADER)
    assert names == NAMES, names
    missing = [n for n in names if not hasattr(so, n)]
    assert not missing, f"declared in {HEADER} but not exported: {missing}"
    assert names == set(lib._SIGNATURES_ANCHOR), names ^ set(lib._SIGNATURES_ANCHOR)
    for other in (lib._SIGNATURES, lib._SIGNATURES_LPIPS, lib._SIGNATURES_DET, lib._SIGNATURES_LORA, lib._SIGNATURES_MASTER,
                  lib._SIGNATURES_MOMENTS8, lib._SIGNATURES_ACCUM):
        assert not set(lib._SIGNATURES_ANCHOR) & set(other)
    # the steps take their counterparts' arguments, `anchor` after `low` (after `scales`), `grad_f32` in front of the stream
    sgd, adam, adam8 = (lib._SIGNATURES_MASTER["lcv_master_sgd_step"], lib._SIGNATURES_MASTER["lcv_master_adamw_step"],
                        lib._SIGNATURES_MOMENTS8["lcv_master_adamw8_step"])
    assert lib._SIGNATURES_ANCHOR["lcv_master_sgd_step_anchor"] == sgd[:2] + [lib.P] + sgd[2:-1] + [lib.I, lib.P]
    assert lib._SIGNATURES_ANCHOR["lcv_master_adamw_step_anchor"] == adam[:2] + [lib.P] + adam[2:-1] + [lib.I, lib.P]
    assert lib._SIGNATURES_ANCHOR["lcv_master_adamw8_step_anchor"] == adam8[:3] + [lib.P] + adam8[3:]
    assert lib._SIGNATURES_ANCHOR["lcv_master_drift_sumsq"] == [lib.P, lib.P, lib.P, lib.I64, lib.I64, lib.P, lib.I64, lib.P, lib.P]
    # the other headers' closed lists are untouched
    for other in ("lcv_hip.h", "lcv_hip_master.h", "lcv_hip_moments8.h", "lcv_hip_accum.h", "lcv_hip_det.h", "lcv_hip_lora.h",
                  "lcv_hip_lpips.h"):
        txt = (ROOT / "include" / other).read_text()
        assert not _declared(other) & names, other
        assert HEADER not in txt and not any(n in txt for n in names), other
    so.lcv_version.restype = ctypes.c_int
    assert so.lcv_version() >= 8                      # went up with the new entry points
    loaded = lib.load()
    for n in names:
        assert getattr(loaded, n).argtypes == lib._SIGNATURES_ANCHOR[n] and getattr(loaded, n).restype is ctypes.c_int


def test_every_anchor_entry_point_has_a_kernel_level_test():
    import ast
    tests = {"lcv_master_sgd_step_anchor": "test_sgd_anchor_step_bits", "lcv_master_adamw_step_anchor": "test_adamw_anchor_step_bits",
             "lcv_master_adamw8_step_anchor": "test_adamw8_anchor_step_bits", "lcv_master_drift_sumsq": "test_drift_sumsq"}
    assert set(tests) == _declared(HEADER)
    tree = ast.parse((ROOT / "tests" / "test_gpu_decay_to_base.py").read_text())
    assert set(tests.values()) <= {n.name for n in ast.walk(tree) if isinstance(n, ast.FunctionDef)}


def test_the_source_uses_no_atomics_and_shares_format_steps_and_codec():
    csrc = ROOT / "longcat-video-tta_amd" / "csrc"
    src = (csrc / "optim_anchor.hip").read_text()           # what is left here: the drift kernels and their entry point
    master = (csrc / "optim_master.hip").read_text()        # the SGD and AdamW anchor steps: forms of the master kernels
    m8 = (csrc / "optim_moments8.hip").read_text()          # the 8-bit anchor step: a form of the 8-bit kernel
    for txt in (src, master, m8):
        for word in ("atomic", "fmaf", "asm", "getenv", "lcv_knob(", "hipMalloc"):
            assert word not in txt, word
        assert '#include "lcv_hip_anchor.h"' in txt                  # the compiler checks the signatures
    for word in ("__shared__", "__syncthreads"):                    # the wave-order join of the drift sum is the only LDS
        assert word in src and word not in master and word not in m8, word
    assert re.findall(r'extern "C" int (\w+)\(', src) == ["lcv_master_drift_sumsq"]
    for entry, txt in (("lcv_master_sgd_step_anchor", master), ("lcv_master_adamw_step_anchor", master),
                       ("lcv_master_adamw8_step_anchor", m8)):
        assert len(re.findall(rf'extern "C" int {entry}\(', txt)) == 1, entry
    shared = (csrc / "master_elem.h").read_text()
    codec = (csrc / "moments8_codec.h").read_text()
    # one definition each: the element functions in master_elem.h, the codec in moments8_codec.h
    for fn in ("void master_adamw_elem(", "void master_adamw_anchor_elem(", "float master_sgd_anchor_elem(", "float master_sgd_elem(",
               "float master_join(", "void master_split("):
        assert shared.count(fn) == 1 and fn not in src and fn not in master and fn not in m8, fn
    for fn in ("m8_encode_m(float", "m8_encode_r(float", "m8_decode_m(unsigned", "m8_decode_v(unsigned", "void m8_encode_store("):
        assert codec.count(fn) == 1 and fn not in src and fn not in master and fn not in m8, fn
    assert "master_adamw_anchor_elem(" in master and "master_sgd_anchor_elem(" in master
    assert "master_adamw_anchor_elem(" in m8 and "m8_encode_store(" in m8
    for txt in (src, master, m8):
        assert "find_tensor(" in txt and "c_wd" not in txt
    assert "adam_scalars(" in master and "adam_scalars(" in m8
    # the anchor and plain decay stay two expressions: p - a * (p - w0) against p * c_wd
    assert "p = p * s.c_wd;" in shared and "p = p - t;" in shared
    from lcv_hip import build
    assert build.EXTRA["optim_anchor.hip"] == build.EXTRA["optim_master.hip"] == ["-ffp-contract=off"]


# ------------------------------------------------------------------------------------------------------------ the optimizers
@pytest.mark.parametrize("cls", ["FusedSGDClip", "FusedAdamWClip"])
def test_constructors_take_anchor_keyword_only_and_refuse_it_without_master_weights(cls):
    from lcv_hip import ops
    from lcv_hip.lib import LcvError
    make = getattr(ops, cls)
    params = list(inspect.signature(make.__init__).parameters.values())
    p = params[-1]
    assert p.name == "anchor" and p.default is None and p.kind is inspect.Parameter.KEYWORD_ONLY
    assert [q.name for q in params if q.kind is inspect.Parameter.KEYWORD_ONLY] == ["grad_accum", "anchor"]
    bf = [torch.zeros(8, dtype=torch.bfloat16)]
    with pytest.raises(LcvError, match="anchor needs master_weights=True"):
        make(bf, anchor=[torch.zeros(8, dtype=torch.bfloat16)])
    with pytest.raises(LcvError, match="GPU"):                       # the existing refusal fires first, with its message
        make(bf, master_weights=True, anchor=[torch.zeros(8, dtype=torch.bfloat16)])
    opt = make(bf)                                                   # no anchor: today's optimizer, nothing held
    assert list(opt._anchor) == [] and "drift" not in opt._tables and hasattr(opt, "drift_norm")
    with pytest.raises(LcvError, match="needs an anchor"):
        opt.drift_norm()
    with pytest.raises(LcvError, match="anchor has 2 tensors for 1"):
        opt.drift_norm(anchor=[bf[0], bf[0]])
    with pytest.raises(LcvError, match="contiguous bf16 tensor"):
        opt.drift_norm(anchor=[torch.zeros(8, dtype=torch.float32)])
    with pytest.raises(LcvError, match="contiguous bf16 tensor"):    # a CPU tensor is no anchor either
        opt.drift_norm(anchor=[torch.zeros(8, dtype=torch.bfloat16)])


def test_loops_take_decay_to_base_keyword_only_in_front_of_grad_accum():
    from tta import delta, full_tta, inner_loop
    for fn in (full_tta.finetune_full_on_conditioning, full_tta.finetune_full_batch):
        params = list(inspect.signature(fn).parameters.values())
        names = [p.name for p in params]
        assert names[-5:] == ["decay_to_base", "base_state", "grad_accum", "moments_8bit", "master_weights"], fn.__name__
        assert all(p.kind is inspect.Parameter.KEYWORD_ONLY for p in params[-5:])
        assert params[-5].default is False and params[-4].default is None
    params = list(inspect.signature(delta.optimize_norm_params).parameters.values())
    assert [p.name for p in params][-4:] == ["decay_to_base", "grad_accum", "moments_8bit", "master_weights"]
    assert params[-4].default is False and params[-4].kind is inspect.Parameter.KEYWORD_ONLY
    mk = list(inspect.signature(full_tta._make_optimizer).parameters.values())
    assert [p.name for p in mk] == ["kind", "params", "lr", "weight_decay", "master_weights", "moments_8bit", "grad_accum", "anchor"]
    assert mk[-1].default is None
    # the engine and the LoRA loops are as they were
    assert list(inspect.signature(inner_loop.run_adaptation).parameters)[-2:] == ["finish_eval", "grad_accum"]
    for fn in (inner_loop.finetune_lora_on_conditioning, inner_loop.finetune_lora_batch):
        assert "decay_to_base" not in inspect.signature(fn).parameters


def test_anchors_are_the_base_state_entries_by_name_not_copies():
    from tta import full_tta
    net = torch.nn.Sequential(torch.nn.Linear(3, 2), torch.nn.Linear(2, 2)).to(torch.bfloat16)
    net[0].bias.requires_grad = False
    base = full_tta.snapshot_base_state(net)
    got = full_tta._anchors(net, base)
    names = [n for n, p in net.named_parameters() if p.requires_grad]
    assert names == ["0.weight", "1.weight", "1.bias"] and len(got) == 3
    assert all(a is base[n] for a, n in zip(got, names))
    assert [p for p in net.parameters() if p.requires_grad] == full_tta._trainable(net)
    clones = full_tta._anchors(net, None)
    assert all(c is not p and c.data_ptr() != p.data_ptr() and torch.equal(c, p) and c.dtype == torch.bfloat16
               for c, p in zip(clones, full_tta._trainable(net)))
    del base["1.weight"]
    with pytest.raises(ValueError, match="base_state lacks 1 trainable parameters, the first: '1.weight'"):
        full_tta._anchors(net, base)


# ------------------------------------------------------------------------------------------------------------ the runners
def _script(rel):
    spec = importlib.util.spec_from_file_location("dtb_" + Path(rel).stem, ROOT / "longcat-video-tta_amd" / rel)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


BASE = ["--checkpoint-dir", "synthetic", "--data-dir", "synthetic:1", "--output-dir", "x"]
FULL, NORM = "lora_experiment/scripts/run_full_tta.py", "delta_experiment/scripts/run_norm_tune_tta.py"


@pytest.mark.parametrize("rel", [FULL, NORM])
def test_runners_take_decay_to_base_and_refuse_it_at_parse_time(rel, capsys):
    mod = _script(rel)
    assert mod.parse_args(BASE).decay_to_base is False
    args = mod.parse_args(BASE + ["--master-weights", "--decay-to-base"])
    assert args.decay_to_base is True and args.master_weights is True
    assert mod.parse_args(BASE + ["--master-weights", "--decay-to-base", "--grad-accum", "2"]).grad_accum == 2
    cases = [(["--decay-to-base"], "--decay-to-base needs --master-weights"),
             # the pinned refusals fire as before, with the flag present
             (["--decay-to-base", "--grad-accum", "2"], "--grad-accum above 1 needs --master-weights"),
             (["--decay-to-base", "--master-weights", "--adam-8bit", "--grad-accum", "2"] +
              (["--optimizer", "adamw"] if rel == FULL else []), "cannot be combined with --adam-8bit")]
    if rel == NORM:
        cases.append((["--decay-to-base", "--master-weights", "--also-tune-delta", "--grad-accum", "2"],
                      "cannot be combined with --also-tune-delta"))
    for argv, message in cases:
        capsys.readouterr()
        with pytest.raises(SystemExit) as e:
            mod.parse_args(BASE + argv)
        err = capsys.readouterr().err
        assert e.value.code == 2 and message in err, (argv, err)
        assert len([ln for ln in err.strip().splitlines() if "error:" in ln]) == 1


def test_other_runners_do_not_take_the_flag():
    for rel in ("lora_experiment/scripts/run_lora_tta.py", "delta_experiment/scripts/run_delta_a.py",
                "delta_experiment/scripts/run_film_tta.py"):
        opts = {s for a in _script(rel).build_parser()._actions for s in a.option_strings}
        assert "--decay-to-base" not in opts, rel


def test_norm_tune_summary_head_and_rows_carry_the_keys_only_with_the_flag(monkeypatch):
    mod = _script(NORM)
    seen = []
    monkeypatch.setattr(mod.R, "run_delta_method", lambda args, method, **kw: seen.append(kw))
    mod.main(BASE + ["--master-weights"])
    mod.main(BASE + ["--master-weights", "--decay-to-base"])
    off, on = seen
    assert "decay_to_base" not in off["summary_head"] and on["summary_head"]["decay_to_base"] is True
    assert set(on["summary_head"]) - set(off["summary_head"]) == {"decay_to_base"}
    row = {"losses": [1.0], "norm_param_drift": 0.5}
    assert off["result_extra"](row) == on["result_extra"](row) == {"norm_param_drift": 0.5}      # no key the loop did not return
    assert on["result_extra"]({**row, "drift_norm": 0.25}) == {"norm_param_drift": 0.5, "drift_norm": 0.25}
    # the loop is handed the flag, and returns drift_norm only under it (the GPU tests run it)
    called = {}
    monkeypatch.setattr(mod, "optimize_norm_params", lambda *a, **kw: called.update(kw) or {})

    class _W:
        tuned_params = []
    for kw, want in ((off, False), (on, True)):
        kw["optimize_fn"](_W(), None, None, None, None, "cpu", None)
        assert called["decay_to_base"] is want


def test_full_runner_files_have_no_new_key_with_the_flag_off(monkeypatch, tmp_path):
    """config.json and summary.json of a job over no videos, with a stand-in model: the flag's key is there exactly when the
    flag is."""
    mod = _script(FULL)
    net = torch.nn.Linear(4, 4).to(torch.bfloat16)
    monkeypatch.setattr(mod.R, "setup_distributed", lambda args: (0, 1, "cpu"))
    monkeypatch.setattr(mod.R, "load_components", lambda args, device: (net, None))
    monkeypatch.setattr(mod.R, "list_eval_entries", lambda args, dit: [])
    files = {}
    for name, flags in (("off", ["--master-weights"]), ("on", ["--master-weights", "--decay-to-base"])):
        out = tmp_path / name
        mod.main(["--checkpoint-dir", "synthetic", "--data-dir", "synthetic:1", "--output-dir", str(out), "--es-disable"] + flags)
        files[name] = (json.loads((out / "config.json").read_text()), json.loads((out / "summary.json").read_text()))
    (c_off, s_off), (c_on, s_on) = files["off"], files["on"]
    assert "decay_to_base" not in c_off["training"] and c_on["training"]["decay_to_base"] is True
    assert set(c_on["training"]) - set(c_off["training"]) == {"decay_to_base"} and set(c_on) == set(c_off)
    assert set(s_on) == set(s_off) and "decay_to_base" not in json.dumps(s_off) and "drift_norm" not in json.dumps(s_off)

"""CPU: the numpy restatement of the 8-bit block-scaled AdamW moments (tests/moments8_ref.py) has the properties
include/lcv_hip_moments8.h states - known-answer codes, the round trip, the error bound, clamping up and flushing down - and
its step is linked to the fp32-moment step exactly as the header says; the header is held to the rules the other headers are
held to; the optimizer and the three runners refuse the flag where it cannot mean anything."""
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
import moments8_ref as R

ROOT = Path(__file__).resolve().parents[1]
HEADER = "lcv_hip_moments8.h"
F = np.float32
NAMES = {"lcv_master_adamw8_step", "lcv_moments8_encode", "lcv_moments8_decode"}


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


def _next(x, k=1):
    return W.floats(W.bits(np.asarray(x, dtype=F)) + np.uint32(k))


def _prev(x, k=1):
    return W.floats(W.bits(np.asarray(x, dtype=F)) - np.uint32(k))


# ------------------------------------------------------------------------------------------------------------ known answers
def test_one_encodes_to_the_top_codes_and_the_named_codes_decode_to_their_constants():
    # a block whose largest element is the scale itself: ratio exactly 1.0
    m = np.array([3.0, -3.0, 0.0], dtype=F)
    v = np.array([4.0, 0.0, 4.0], dtype=F)
    cm, cr, s = R.encode(m, v)
    assert s.shape == (2, 1) and s[0, 0] == F(3.0) and s[1, 0] == F(2.0)
    assert cm.tolist() == [127, 127 | 128, 0] and cr.tolist() == [255, 0, 255]
    # decode of the named codes under unit scales
    one = np.ones((2, 1), dtype=F)
    m1, v1 = R.decode(np.array([1, 127, 129, 255, 0, 128], np.uint8), np.array([1, 255, 0, 1, 255, 0], np.uint8), one)
    assert m1.tolist() == [1.25 * 2.0 ** -16, 1.0, -1.25 * 2.0 ** -16, -1.0, 0.0, 0.0]
    r_floor = F(1.25 * 2.0 ** -32)
    assert v1.tolist() == [float(r_floor * r_floor), 1.0, 0.0, float(r_floor * r_floor), 1.0, 0.0]
    assert R.M_FLOOR == F(1.25 * 2.0 ** -16) and R.R_FLOOR == r_floor
    assert W.bits(np.array([R.M_FLOOR, R.R_FLOOR])).tolist() == [(1 + 889) << 20, (1 + 761) << 20]


def test_ties_round_away_from_zero_and_one_ulp_below_a_tie_rounds_down():
    # 3 mantissa bits: the codes next to 0.5 are 0.5 and 0.5625, the tie between them is 0.53125
    tie = F(0.53125)
    below = _prev(tie)
    lo_m, hi_m = (W.bits(np.array([0.5], dtype=F))[0] >> 20) - 889, (W.bits(np.array([0.5625], dtype=F))[0] >> 20) - 889
    assert hi_m == lo_m + 1 == 120
    ones = np.ones(1, dtype=F)
    for z, want in ((tie, hi_m), (below, lo_m), (F(0.5), lo_m), (F(0.5625), hi_m)):
        cm, cr = R.encode_scaled(np.array([z, -z], dtype=F), np.array([z, z], dtype=F), ones, ones)
        assert cm.tolist() == [want, want | 128], (z, cm)
        assert cr.tolist() == [want + 128, want + 128], (z, cr)                 # the same grid, 128 codes further up
    # the carry runs into the exponent: just under 1.0 rounds up to the code of 1.0
    cm, cr = R.encode_scaled(np.array([_prev(F(1.0))]), np.array([_prev(F(1.0))]), ones, ones)
    assert cm.tolist() == [127] and cr.tolist() == [255]
    # ... and a ratio is never above 1.0, but the clamps hold anyway
    cm, cr = R.encode_scaled(np.array([4.0], dtype=F), np.array([4.0], dtype=F), ones, ones)
    assert cm.tolist() == [127] and cr.tolist() == [255]


# ------------------------------------------------------------------------------------------------------------ properties
@pytest.mark.parametrize("scale", [1.0, 3.0, 2.0 ** -20, 1.7e5, 0.3])
def test_encode_after_decode_is_the_identity_on_every_code(scale):
    # every (cm, cr) pattern once; 0x80 (a negative flushed element) is not a code encode produces and is checked apart
    cm = np.array([c for c in range(256) if c != 128] + [127], dtype=np.uint8)
    cr = np.arange(256, dtype=np.uint8)
    scales = np.full((2, 1), scale, dtype=F)
    m, v = R.decode(cm, cr, scales)
    cm2, cr2, s2 = R.encode(m, v)
    assert np.array_equal(s2, scales)                                           # code 127 / 255 carries the scale itself
    assert np.array_equal(cm2, cm) and np.array_equal(cr2, cr)
    # a negative element that flushes: the sign bit is cleared
    tiny = np.array([scale, -scale * 2.0 ** -18, -0.0], dtype=F)
    cm3, _, _ = R.encode(tiny, np.zeros(3, dtype=F))
    assert cm3.tolist() == [127, 0, 0]
    m3, _ = R.decode(cm3, np.zeros(3, np.uint8), np.array([[scale], [0.0]], dtype=F))
    assert W.bits(m3[1:]).tolist() == [0, 0]


def test_error_bound_on_unclamped_unflushed_elements():
    """|dq(q(z)) - z| <= (2^-4 + 2^-22) |z|: half a step of a 3-bit mantissa, 2^-4 of the value at worst, plus the roundings of
    the division and of the product back (2^-24 each, on a value up to 1 + 2^-4 times z)."""
    rng = np.random.default_rng(5)
    n = 64 * R.BLOCK + 77
    m, v = R.moments(rng, n, -14.0, 0.0)
    r = np.sqrt(v)
    cm, cr, s = R.encode(m, v)
    md, vd = R.decode(cm, cr, s)
    rd = np.sqrt(vd.astype(np.float64))
    bound = 2.0 ** -4 + 2.0 ** -22
    live_m = (cm & 127) > 0                         # not flushed (the top code is 1.0 itself: the ratio is never above it)
    live_r = cr > 1                                 # not clamped up
    assert live_m.mean() > 0.9 and live_r.all()
    em = np.abs(md.astype(np.float64) - m.astype(np.float64)) / np.abs(m.astype(np.float64))
    er = np.abs(rd - r.astype(np.float64)) / r.astype(np.float64)
    print(f"largest relative error: m {em[live_m].max():.6f}  r {er[live_r].max():.6f}  bound {bound:.6f}")
    assert em[live_m].max() <= bound and er[live_r].max() <= bound
    assert np.array_equal(np.signbit(md[live_m]), np.signbit(m[live_m]))


def test_a_clamped_root_decodes_no_smaller_and_a_flushed_first_moment_decodes_to_plus_zero():
    rng = np.random.default_rng(6)
    n = R.BLOCK
    m, v = R.moments(rng, n, -4.0, 0.0)
    m[0], v[0] = 2.0 ** 40, 2.0 ** 80                                            # one element 2^40 times the rest
    cm, cr, s = R.encode(m, v)
    assert s[0, 0] == F(2.0 ** 40) and s[1, 0] == F(2.0 ** 40)
    assert cm[0] == 127 and cr[0] == 255
    assert (cm[1:] == 0).all() and (cr[1:] == 1).all()                           # flushed to +0; clamped UP to code 1
    md, vd = R.decode(cm, cr, s)
    assert W.bits(md[1:]).max() == 0
    assert (np.sqrt(vd[1:]) >= np.sqrt(v[1:])).all() and (vd[1:] > 0).all()     # a denominator is never underestimated
    assert md[0] == m[0] and vd[0] == v[0]
    # an all-zero block: scales 0, codes 0, decodes to zeros without a NaN
    cm, cr, s = R.encode(np.zeros(7, dtype=F), np.zeros(7, dtype=F))
    assert not cm.any() and not cr.any() and not s.any()
    md, vd = R.decode(cm, cr, s)
    assert W.bits(md).max() == 0 and W.bits(vd).max() == 0


def test_blocks_are_512_elements_and_the_last_may_be_short():
    rng = np.random.default_rng(7)
    n = 2 * R.BLOCK + 3
    m, v = R.moments(rng, n)
    cm, cr, s = R.encode(m, v)
    assert s.shape == (2, 3) and cm.shape == cr.shape == (n,)
    for b in range(3):
        sl = slice(b * R.BLOCK, min((b + 1) * R.BLOCK, n))
        assert s[0, b] == np.abs(m[sl]).max() and s[1, b] == np.sqrt(v[sl]).max()
        a, c, t = R.encode(m[sl], v[sl])                                         # a block is encoded on its own
        assert np.array_equal(a, cm[sl]) and np.array_equal(c, cr[sl]) and np.array_equal(t[:, 0], s[:, b])


# ------------------------------------------------------------------------------------------------------------ the step
def _step_inputs(seed, n=3 * R.BLOCK + 41):
    rng = np.random.default_rng(seed)
    h, low = W.weights(rng, n)
    return h, low, [W.grads(rng, n) for _ in range(3)]


@pytest.mark.parametrize("coef, wd", [(1.0, 0.0), (0.37, 0.01)])
def test_property_a_first_step_from_zero_state_gives_the_fp32_moment_steps_bits(coef, wd):
    h, low, gs = _step_inputs(8)
    cm, cr, s = R.zero_state(h.size)
    m0, v0 = R.decode(cm, cr, s)
    assert W.bits(m0).max() == 0 and W.bits(v0).max() == 0                       # zero is the state "all moments zero"
    h8, l8, cm, cr, s = R.adamw8_step(h, low, cm, cr, s, gs[0], coef, 1e-3, 0.9, 0.999, 1e-8, wd, 1)
    hf, lf, mf, vf = W.adamw_step(h, low, m0, v0, gs[0], coef, 1e-3, 0.9, 0.999, 1e-8, wd, 1)
    assert np.array_equal(h8, hf) and np.array_equal(l8, lf)
    a, c, t = R.encode(mf, vf)
    assert np.array_equal(a, cm) and np.array_equal(c, cr) and np.array_equal(t, s)


@pytest.mark.parametrize("coef, wd", [(1.0, 0.0), (0.37, 0.01)])
def test_property_b_any_step_gives_the_fp32_moment_steps_bits_from_the_decoded_state(coef, wd):
    h, low, gs = _step_inputs(9)
    cm, cr, s = R.zero_state(h.size)
    hf, lf, mf, vf = h, low, np.zeros(h.size, F), np.zeros(h.size, F)
    diverged = False
    for k, g in enumerate(gs):
        m0, v0 = R.decode(cm, cr, s)
        want = W.adamw_step(h, low, m0, v0, g, coef, 1e-3, 0.9, 0.999, 1e-8, wd, k + 1)
        h, low, cm, cr, s = R.adamw8_step(h, low, cm, cr, s, g, coef, 1e-3, 0.9, 0.999, 1e-8, wd, k + 1)
        assert np.array_equal(h, want[0]) and np.array_equal(low, want[1])
        hf, lf, mf, vf = W.adamw_step(hf, lf, mf, vf, g, coef, 1e-3, 0.9, 0.999, 1e-8, wd, k + 1)
        diverged = diverged or not (np.array_equal(h, hf) and np.array_equal(low, lf))
        assert diverged == (k >= 1)                                             # same after step 1, not after step 2


# ------------------------------------------------------------------------------------------------------------ the header
def test_moments8_header_symbols_are_exported_and_bound():
    lib, so = _built()
    names = _declared(HEADER)
    assert names == NAMES, names
    missing = [n for n in names if not hasattr(so, n)]
    assert not missing, f"declared in {HEADER} but not exported: {missing}"
    assert names == set(lib._SIGNATURES_MOMENTS8), names ^ set(lib._SIGNATURES_MOMENTS8)
    for other in (lib._SIGNATURES, lib._SIGNATURES_LPIPS, lib._SIGNATURES_DET, lib._SIGNATURES_LORA, lib._SIGNATURES_MASTER):
        assert not set(lib._SIGNATURES_MOMENTS8) & set(other)
    # the step takes the fp32-moment step's arguments with `scales` after `low`
    mas = lib._SIGNATURES_MASTER["lcv_master_adamw_step"]
    assert lib._SIGNATURES_MOMENTS8["lcv_master_adamw8_step"] == mas[:2] + [lib.P] + mas[2:]
    assert not _declared("lcv_hip.h") & names and not _declared("lcv_hip_master.h") & names
    assert HEADER not in (ROOT / "include" / "lcv_hip.h").read_text()
    so.lcv_version.restype = ctypes.c_int
    assert so.lcv_version() >= 6                      # went up with the new entry points
    loaded = lib.load()
    for n in names:
        assert getattr(loaded, n).argtypes == lib._SIGNATURES_MOMENTS8[n] and getattr(loaded, n).restype is ctypes.c_int


def test_every_moments8_entry_point_has_a_kernel_level_test():
    import ast
    tests = {"lcv_master_adamw8_step": "test_adamw8_step_bits", "lcv_moments8_encode": "test_encode_bits",
             "lcv_moments8_decode": "test_decode_bits"}
    assert set(tests) == _declared(HEADER)
    tree = ast.parse((ROOT / "tests" / "test_gpu_moments8.py").read_text())
    assert set(tests.values()) <= {n.name for n in ast.walk(tree) if isinstance(n, ast.FunctionDef)}


def test_the_source_uses_no_atomics_no_lds_and_shares_the_step_with_the_fp32_moment_kernel():
    csrc = ROOT / "longcat-video-tta_amd" / "csrc"
    src = (csrc / "optim_moments8.hip").read_text()
    # the file holds both 8-bit step forms (with and without an anchor): the lists of both kernels' earlier files hold here
    for word in ("atomic", "fmaf", "asm", "getenv", "lcv_knob(", "hipMalloc", "__shared__", "__syncthreads"):
        assert word not in src, word
    for entry in ("lcv_master_adamw8_step", "lcv_master_adamw8_step_anchor", "lcv_moments8_encode", "lcv_moments8_decode"):
        assert len(re.findall(rf'extern "C" int {entry}\(', src)) == 1, entry
    assert len(re.findall(r"\bvoid\s+master_adamw8_kernel\s*\(", src)) == 1 and "master_adamw8_anchor_kernel" not in src
    assert '#include "lcv_hip_anchor.h"' in src and '#include "lcv_hip_moments8.h"' in (csrc / "moments8_codec.h").read_text()
    # one definition of the op sequence, in the shared header, used by both files
    shared = (csrc / "master_elem.h").read_text()
    assert shared.count("void master_adamw_elem(") == 1
    for f in ("optim_moments8.hip", "optim_master.hip"):
        txt = (csrc / f).read_text()
        assert '#include "master_elem.h"' in txt and "void master_adamw_elem(" not in txt and "master_adamw_elem(" in txt
    from lcv_hip import build
    assert build.EXTRA["optim_moments8.hip"] == build.EXTRA["optim_master.hip"] == ["-ffp-contract=off"]


# ------------------------------------------------------------------------------------------------------------ refusals
def test_moments_8bit_is_refused_without_master_weights_and_for_fp32_or_cpu_parameters():
    from lcv_hip import ops
    from lcv_hip.lib import LcvError
    bf = [torch.zeros(8, dtype=torch.bfloat16)]
    with pytest.raises(LcvError, match="needs master_weights=True"):
        ops.FusedAdamWClip(bf, moments_8bit=True)
    with pytest.raises(LcvError, match="needs master_weights=True"):
        ops.FusedAdamWClip([torch.zeros(8, dtype=torch.float32)], moments_8bit=True)
    with pytest.raises(LcvError, match="fp32 parameters are already exact"):
        ops.FusedAdamWClip([torch.zeros(8, dtype=torch.float32)], master_weights=True, moments_8bit=True)
    with pytest.raises(LcvError, match="GPU"):
        ops.FusedAdamWClip(bf, master_weights=True, moments_8bit=True)
    with pytest.raises(TypeError):
        ops.FusedSGDClip(bf, moments_8bit=True)                                 # SGD does not take the keyword
    # off: today's optimizer - bf16 moments, 4 B / parameter of state
    opt = ops.FusedAdamWClip(bf)
    assert opt.moments_8bit is False and opt.exp_avg[0].dtype == torch.bfloat16 and opt.state_bytes() == 32
    assert ops.FusedSGDClip(bf).state_bytes() == 0 and ops.FusedSGDClip(bf).moments_8bit is False
    with pytest.raises(LcvError, match="no moments"):
        ops.FusedSGDClip(bf).moment_tensors()


def _script(rel):
    spec = importlib.util.spec_from_file_location("m8_" + Path(rel).stem, ROOT / "longcat-video-tta_amd" / rel)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


BASE = ["--checkpoint-dir", "synthetic", "--data-dir", "synthetic:1", "--output-dir", "x"]


@pytest.mark.parametrize("rel, has_optimizer", [("lora_experiment/scripts/run_lora_tta.py", False),
                                                ("lora_experiment/scripts/run_full_tta.py", True),
                                                ("delta_experiment/scripts/run_norm_tune_tta.py", False)])
def test_runners_take_adam_8bit_and_refuse_it_at_parse_time(rel, has_optimizer, capsys):
    mod = _script(rel)
    adamw = ["--optimizer", "adamw"] if has_optimizer else []
    assert mod.parse_args(BASE).adam_8bit is False
    assert mod.parse_args(BASE + ["--master-weights"]).adam_8bit is False
    args = mod.parse_args(BASE + ["--master-weights", "--adam-8bit"] + adamw)
    assert args.adam_8bit is True and args.master_weights is True
    cases = [(["--adam-8bit"] + adamw, "--adam-8bit needs --master-weights")]
    if has_optimizer:
        cases += [(["--master-weights", "--adam-8bit"], "--adam-8bit needs --optimizer adamw"),            # sgd is the default
                  (["--master-weights", "--adam-8bit", "--optimizer", "sgd"], "--adam-8bit needs --optimizer adamw")]
    for argv, message in cases:
        capsys.readouterr()
        with pytest.raises(SystemExit) as e:
            mod.parse_args(BASE + argv)
        err = capsys.readouterr().err
        assert e.value.code == 2 and message in err
        assert len([ln for ln in err.strip().splitlines() if "error:" in ln]) == 1


def test_delta_and_film_runners_do_not_take_the_flag_and_the_loops_default_it_off():
    for rel in ("delta_experiment/scripts/run_delta_a.py", "delta_experiment/scripts/run_film_tta.py"):
        opts = {s for a in _script(rel).build_parser()._actions for s in a.option_strings}
        assert "--adam-8bit" not in opts, rel
    from tta import delta, full_tta, inner_loop
    for fn in (inner_loop.finetune_lora_on_conditioning, inner_loop.finetune_lora_batch, full_tta.finetune_full_on_conditioning,
               full_tta.finetune_full_batch, delta.optimize_norm_params):
        p = inspect.signature(fn).parameters["moments_8bit"]
        assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY, fn.__name__
    with pytest.raises(ValueError, match="SGD keeps no moments"):
        full_tta._make_optimizer("sgd", [torch.zeros(8, dtype=torch.bfloat16)], 1e-5, 0.01, True, True)

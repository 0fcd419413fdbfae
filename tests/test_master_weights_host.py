"""CPU: the numpy restatement of the master-weight format (tests/master_weights_ref.py) has the properties
include/lcv_hip_master.h states, and its two steps agree with torch's fp32 optimizers on the joined masters; the header is held
to the rules the other headers are held to (every declared symbol exported and bound, the tables disjoint, nothing of it in the
main header); the optimizers refuse CPU tensors and fp32 parameters under master_weights=True."""
import ctypes
import re
import sys
from pathlib import Path

import numpy as np
import pytest
import torch

import master_weights_ref as R

ROOT = Path(__file__).resolve().parents[1]
HEADER = "lcv_hip_master.h"


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


# ------------------------------------------------------------------------------------------------------------ the format
def test_join_after_split_is_the_identity_on_every_kind_of_pattern():
    m = R.edge_patterns(n_random=1 << 20, seed=1)
    h, low = R.split(m)
    assert h.dtype == np.uint16 and low.dtype == np.int16
    assert np.array_equal(R.join(h, low), m)
    # the named ones, one by one: +-0, denormals, largest finite, infinities, NaNs
    for pat in (0x00000000, 0x80000000, 0x00000001, 0x807FFFFF, 0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000,
                0xFFFFFFFF):
        hh, ll = R.split(np.array([pat], dtype=np.uint32))
        assert int(R.join(hh, ll)[0]) == pat, hex(pat)


def test_low_word_range_and_the_meaning_of_zero():
    m = R.edge_patterns(n_random=1 << 18, seed=2)
    h, low = R.split(m)
    assert low.min() == -32768 and low.max() == 32767                   # the whole int16 range is used, nothing beyond it
    # the definition, in Python integers
    for mi, hi, li in zip(m[:64].tolist(), h[:64].tolist(), low[:64].tolist()):
        want_h = ((mi + 0x8000) & 0xFFFFFFFF) >> 16
        d = (mi - (want_h << 16)) & 0xFFFFFFFF
        assert hi == want_h and li == (d - (1 << 32) if d >= 0x80000000 else d) and -32768 <= li <= 32767
    # l == 0: the master equals the bf16 value, for every bf16 word
    every = np.arange(1 << 16, dtype=np.uint16)
    assert np.array_equal(R.join(every, np.zeros(1 << 16, dtype=np.int16)), every.astype(np.uint32) << 16)
    hh, ll = R.split(every.astype(np.uint32) << 16)
    assert np.array_equal(hh, every) and not ll.any()


def test_high_word_is_torchs_bf16_rounding_except_on_exact_ties():
    rng = np.random.default_rng(3)
    x = np.concatenate([R.log_uniform(rng, 1 << 18, -30.0, 30.0), rng.standard_normal(1 << 18).astype(np.float32)])
    m = R.bits(x)
    ties = m[: 1 << 12].copy()
    ties = (ties & np.uint32(0xFFFF0000)) | np.uint32(0x8000)          # exact ties, even and odd upper halves
    m = np.concatenate([m, ties])
    h, _ = R.split(m)
    t = torch.from_numpy(R.floats(m).copy()).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    tie = (m & np.uint32(0xFFFF)) == 0x8000
    assert np.array_equal(h[~tie], t[~tie])
    assert np.array_equal(h[~tie], R.to_bf16_bits(R.floats(m))[~tie])    # the helper that makes the tests' bf16 gradients
    # on a tie: away from zero here, to even in torch; they differ exactly where the upper half is even
    even = ((m >> 16) & 1) == 0
    assert np.array_equal(h[tie], ((m[tie] >> 16) + 1).astype(np.uint16))
    assert np.array_equal(h[tie & ~even], t[tie & ~even]) and np.all(h[tie & even] == t[tie & even] + 1)
    # about 1 in 65 536 of random data
    rnd = R.edge_patterns(n_random=1 << 22, seed=4)
    n_tie = int(((rnd & np.uint32(0xFFFF)) == 0x8000).sum())
    assert n_tie <= 4 * (1 << 22) // 65536


# ------------------------------------------------------------------------------------------------------------ the steps
def _inputs(n=20000, seed=5):
    rng = np.random.default_rng(seed)
    h, low = R.weights(rng, n)
    return h, low, [R.grads(rng, n) for _ in range(3)]


def _rel(a, b, scale):
    """Largest |a - b| relative to `scale`: per element the largest magnitude the quantity had along torch's trajectory.  A sum
    such as w - lr * g or m + (1 - b1) * (g - m) may cancel, and the rounding error of an fp32 sum is relative to its larger
    operand, not to a result that happens to be small."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b) / scale))


class _Scale:
    def __init__(self, x=None):
        self.max = None if x is None else np.abs(np.asarray(x, dtype=np.float64))

    def see(self, x):
        x = np.abs(np.asarray(x, dtype=np.float64))
        self.max = x if self.max is None else np.maximum(self.max, x)


@pytest.mark.parametrize("coef", [1.0, 0.37])
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_restated_sgd_agrees_with_torch_sgd_in_fp32(coef, wd):
    """Three free-running steps of the restatement against torch.optim.SGD(momentum=0) on the joined masters with upcast
    gradients (scaled by the clip coefficient in fp32).  Measured on the CPU, relative to each element's largest magnitude
    along the trajectory (`_rel`): 1.86e-7, 2.05e-7, 1.99e-7 and 2.18e-7 over the four cases - under two fp32 ulps; torch's
    kernels fuse alpha * x into the add.  The bound is 4x the largest, 8.8e-7."""
    h, low, gs = _inputs()
    w0 = R.master(h, low).copy()
    p = torch.nn.Parameter(torch.from_numpy(w0.copy()))
    opt = torch.optim.SGD([p], lr=0.05, momentum=0.0, weight_decay=wd)
    scale = _Scale(w0)
    for g in gs:
        h, low = R.sgd_step(h, low, g, coef, 0.05, wd)
        p.grad = torch.from_numpy(R.bf16_to_f32(g).copy()) * torch.tensor(coef, dtype=torch.float32)
        opt.step()
        scale.see(p.detach().numpy())
    rel = _rel(R.master(h, low), p.detach().numpy(), scale.max)
    print(f"sgd coef={coef} wd={wd}: largest relative difference {rel:.3e}")
    assert rel <= 8.8e-7


@pytest.mark.parametrize("coef", [1.0, 0.37])
@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_restated_adamw_agrees_with_torch_adamw_in_fp32(coef, wd):
    """Three free-running steps against torch.optim.AdamW (fp32 parameters and moments).  Measured on the CPU, relative
    to each element's largest magnitude along the trajectory (`_rel`), largest over the four cases: parameters 2.82e-7,
    exp_avg 2.13e-7, exp_avg_sq 2.01e-7 - under three fp32 ulps; torch's lerp, addcmul and addcdiv fuse their multiplies.
    The bound is 4x the largest, 1.13e-6."""
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    h, low, gs = _inputs(seed=6)
    m = np.zeros(h.shape, dtype=np.float32)
    v = np.zeros(h.shape, dtype=np.float32)
    w0 = R.master(h, low).copy()
    p = torch.nn.Parameter(torch.from_numpy(w0.copy()))
    opt = torch.optim.AdamW([p], lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd)
    sp, sm, sv = _Scale(w0), _Scale(), _Scale()
    for k, g in enumerate(gs):
        h, low, m, v = R.adamw_step(h, low, m, v, g, coef, lr, b1, b2, eps, wd, k + 1)
        p.grad = torch.from_numpy(R.bf16_to_f32(g).copy()) * torch.tensor(coef, dtype=torch.float32)
        opt.step()
        st = opt.state[p]
        sp.see(p.detach().numpy()); sm.see(st["exp_avg"].numpy()); sv.see(st["exp_avg_sq"].numpy())
    rels = (_rel(R.master(h, low), p.detach().numpy(), sp.max), _rel(m, st["exp_avg"].numpy(), sm.max),
            _rel(v, st["exp_avg_sq"].numpy(), sv.max))
    print(f"adamw coef={coef} wd={wd}: largest relative differences p {rels[0]:.3e} m {rels[1]:.3e} v {rels[2]:.3e}")
    assert max(rels) <= 1.13e-6


# ------------------------------------------------------------------------------------------------------------ the header
def test_master_header_symbols_are_exported_and_bound():
    lib, so = _built()
    names = _declared(HEADER)
    assert names == {"lcv_master_sgd_step", "lcv_master_adamw_step", "lcv_master_split", "lcv_master_join"}, names
    missing = [n for n in names if not hasattr(so, n)]
    assert not missing, f"declared in {HEADER} but not exported: {missing}"
    assert names == set(lib._SIGNATURES_MASTER), names ^ set(lib._SIGNATURES_MASTER)
    for other in (lib._SIGNATURES, lib._SIGNATURES_LPIPS, lib._SIGNATURES_DET, lib._SIGNATURES_LORA):
        assert not set(lib._SIGNATURES_MASTER) & set(other)
    # the steps take their counterparts' arguments without param_f32, and `low` after the table
    assert lib._SIGNATURES_MASTER["lcv_master_sgd_step"] == [lib.P, lib.P] + [a for a in lib._SIGNATURES["lcv_sgd_step"][1:] if a is not lib.I]
    assert lib._SIGNATURES_MASTER["lcv_master_adamw_step"] == [lib.P, lib.P] + [a for a in lib._SIGNATURES["lcv_adamw_step"][1:] if a is not lib.I]
    # the main header's closed list is untouched
    assert not _declared("lcv_hip.h") & names
    assert HEADER not in (ROOT / "include" / "lcv_hip.h").read_text()
    so.lcv_version.restype = ctypes.c_int
    assert so.lcv_version() >= 5                      # went up with the new entry points
    loaded = lib.load()
    for n in names:
        assert getattr(loaded, n).argtypes == lib._SIGNATURES_MASTER[n] and getattr(loaded, n).restype is ctypes.c_int


def test_every_master_entry_point_has_a_kernel_level_test():
    import ast
    tests = {"lcv_master_sgd_step": "test_sgd_step_bits", "lcv_master_adamw_step": "test_adamw_step_bits",
             "lcv_master_split": "test_split_bits", "lcv_master_join": "test_join_bits"}
    assert set(tests) == _declared(HEADER)
    tree = ast.parse((ROOT / "tests" / "test_gpu_master_weights.py").read_text())
    assert set(tests.values()) <= {n.name for n in ast.walk(tree) if isinstance(n, ast.FunctionDef)}


def test_the_source_uses_no_atomics_and_reads_no_environment():
    csrc = ROOT / "longcat-video-tta_amd" / "csrc"
    src = (csrc / "optim_master.hip").read_text()
    # the file holds every SGD and AdamW step form (bf16 / fp32 gradient, with / without an anchor): the lists of the files
    # those kernels came from hold here
    for word in ("atomic", "fmaf", "asm", "getenv", "lcv_knob(", "hipMalloc", "__shared__", "__syncthreads"):
        assert word not in src, word
    for header in ("lcv_hip_master.h", "lcv_hip_accum.h", "lcv_hip_anchor.h"):       # the compiler checks the signatures
        assert f'#include "{header}"' in src, header
    for entry in ("lcv_master_sgd_step", "lcv_master_sgd_step_g32", "lcv_master_sgd_step_anchor", "lcv_master_adamw_step",
                  "lcv_master_adamw_step_g32", "lcv_master_adamw_step_anchor", "lcv_master_split", "lcv_master_join"):
        assert len(re.findall(rf'extern "C" int {entry}\(', src)) == 1, entry
    for use in ("master_sgd_elem(", "master_sgd_anchor_elem(", "master_adamw_elem(", "master_adamw_anchor_elem(", "master_join(",
                "master_split(", "find_tensor(", "adam_scalars(", "optim_table_ok(", "chunk_grid("):
        assert use in src, use


def test_one_definition_of_each_step_kernel_element_function_and_host_helper():
    csrc = ROOT / "longcat-video-tta_amd" / "csrc"
    texts = {p.name: p.read_text() for p in sorted(csrc.glob("*.hip")) + sorted(csrc.glob("*.h"))}
    everything = "\n".join(texts.values())

    def defined_in(pattern):
        return [name for name, txt in texts.items() for _ in re.findall(pattern, txt)]
    # three step kernels, each a template defined once, in the file of its optimizer
    kernels = re.findall(r"__global__[^;{]*?\bvoid\s+(master_\w+_kernel)\s*\(", everything)
    assert sorted(kernels) == ["master_adamw8_kernel", "master_adamw_kernel", "master_convert_kernel", "master_ema_kernel",
                               "master_sgd_kernel"], kernels
    assert defined_in(r"\bvoid\s+master_sgd_kernel\s*\(") == defined_in(r"\bvoid\s+master_adamw_kernel\s*\(") == ["optim_master.hip"]
    assert defined_in(r"\bvoid\s+master_adamw8_kernel\s*\(") == ["optim_moments8.hip"]
    assert "template <bool G32, bool ANCHOR>\n__global__" in texts["optim_master.hip"]
    assert "template <bool ANCHOR>\n__global__" in texts["optim_moments8.hip"]
    # the element functions, once each, in the shared header
    for fn in ("float master_sgd_elem(", "float master_sgd_anchor_elem(", "void master_adamw_elem(", "void master_adamw_anchor_elem(",
               "void load8(", "void store8("):
        assert everything.count(fn) == 1 and texts["master_elem.h"].count(fn) == 1, fn
    assert "accum_sgd_elem" not in everything
    # the host helpers, once each, in optim_common.h; nothing keeps a copy under another name
    for fn in ("struct AdamScalars", "AdamScalars adam_scalars(", "bool optim_table_ok(", "bool chunk_grid("):
        assert everything.count(fn) == 1 and texts["optim_common.h"].count(fn) == 1, fn
    for gone in ("MasterAdamScalars", "master_adam_scalars", "anchor_table_ok", "ema_table_ok", "master_convert_grid", "moments8_grid",
                 "anchor_grad", "anchor_widen", "anchor_load_grads"):
        assert gone not in everything, gone
    # no optimizer entry point spells the table check out
    for name in ("optim_master.hip", "optim_moments8.hip", "optim_accum.hip", "optim_anchor.hip", "optim_ema.hip"):
        assert "0x7fffffff" not in texts[name], name
        assert "pow(" not in texts[name], name


# ------------------------------------------------------------------------------------------------------------ the optimizers
@pytest.mark.parametrize("cls", ["FusedSGDClip", "FusedAdamWClip"])
def test_master_weights_refuse_cpu_tensors_and_fp32_parameters(cls):
    from lcv_hip import ops
    from lcv_hip.lib import LcvError
    make = getattr(ops, cls)
    with pytest.raises(LcvError, match="GPU"):
        make([torch.zeros(8, dtype=torch.bfloat16)], master_weights=True)
    with pytest.raises(LcvError, match="fp32 parameters are already exact"):
        make([torch.zeros(8, dtype=torch.float32)], master_weights=True)
    # off: today's constructor, no low words, nothing to resynchronise
    opt = make([torch.zeros(8, dtype=torch.bfloat16)])
    assert opt.master_weights is False and opt.low_words == [] and opt.resync() is None
    with pytest.raises(LcvError, match="master_weights=True"):
        opt.master_tensors()


def test_loops_and_runners_take_the_flag_last_and_default_it_off():
    import importlib.util
    import inspect
    from tta import delta, full_tta, inner_loop
    for fn in (inner_loop.finetune_lora_on_conditioning, inner_loop.finetune_lora_batch, full_tta.finetune_full_on_conditioning,
               full_tta.finetune_full_batch, delta.optimize_norm_params):
        last = list(inspect.signature(fn).parameters.values())[-1]
        assert last.name == "master_weights" and last.default is False, fn.__name__
    scripts = ROOT / "longcat-video-tta_amd"
    for rel, takes in (("lora_experiment/scripts/run_lora_tta.py", True), ("lora_experiment/scripts/run_full_tta.py", True),
                       ("delta_experiment/scripts/run_norm_tune_tta.py", True), ("delta_experiment/scripts/run_delta_a.py", False),
                       ("delta_experiment/scripts/run_film_tta.py", False)):
        spec = importlib.util.spec_from_file_location("mw_" + Path(rel).stem, scripts / rel)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        opts = {s for a in mod.build_parser()._actions for s in a.option_strings}
        assert ("--master-weights" in opts) == takes, rel
        if takes:
            base = ["--checkpoint-dir", "synthetic", "--data-dir", "synthetic:1", "--output-dir", "x"]
            assert mod.build_parser().parse_args(base).master_weights is False
            assert mod.build_parser().parse_args(base + ["--master-weights"]).master_weights is True

"""ctypes binding of liblcv_hip.so (the C ABI declared in include/lcv_hip.h).

The library is the product path: when it is missing this module raises — there
is no CPU or eager-PyTorch fallback anywhere above it.
"""
import ctypes
import os
from ctypes import c_char_p, c_double, c_float, c_int, c_int64, c_uint64, c_void_p
from pathlib import Path

_LIB_PATH = Path(__file__).resolve().parent / "liblcv_hip.so"

P, I64, F32, I, F64, U64 = c_void_p, c_int64, c_float, c_int, c_double, c_uint64

# name -> argtypes (every function returns int)
_SIGNATURES = {
    "lcv_device_check": [],
    "lcv_adaln_modulate_fwd": [P, P, P, I64, I64, I64, I64, I64, I64, I64, F32, P],
    "lcv_adaln_modulate_bwd": [P, P, P, P, P, I64, I64, I64, I64, I64, I64, I64, F32, P, P],
    "lcv_layernorm_affine_fwd": [P, P, P, P, I64, I64, F32, P],
    "lcv_layernorm_affine_bwd": [P, P, P, P, P, P, I64, I64, F32, P, P],
    "lcv_gate_residual_fwd": [P, P, P, P, I64, I64, I64, I64, I64, I64, P],
    "lcv_gate_residual_bwd": [P, P, P, P, P, I64, I64, I64, I64, I64, I64, P],
    "lcv_qknorm_rope_fwd": [P, P, P, P, P, P, P, P, P, I64, I64, I64, I64, I64, I64, I64, I64, I64, I64, F32, F32, P],
    "lcv_qknorm_rope_bwd": [P, P, P, P, P, P, P, P, P, I64, I64, I64, I64, I64, I64, I64, I64, I64, I64, I64, I64, F32, F32, P, P, I64, P],
    "lcv_attn_fwd": [P, P, P, P, P, I64, I64, I64, I64] + [I64] * 12 + [F32, P],
    "lcv_attn_bwd": [P, P, P, P, P, P, P, P, P, P, I, I64, I64, I64, I64] + [I64] * 21 + [F32, P],
    "lcv_gemm_nt": [P, P, P, P, P, P, I64, I64, I64, I64, I64, I64, I64, I64, I64, I, I, P, P, I64, I64, I64, P],
    "lcv_gemm_set_workspace": [P, I64],
    "lcv_linear_f32_smallm": [P, P, P, P, I64, I64, I64, I, P],
    "lcv_lora_down": [P, P, P, I64, I64, I64, I64, I64, F32, P],
    "lcv_tn_skinny": [P, P, P, I64, I64, I64, I64, I64, F32, P, I64, P],
    "lcv_linear_f32_smallm_bwd": [P, P, P, P, I64, I64, I64, I, P],
    "lcv_timestep_embedding": [P, P, I64, I64, F32, P],
    "lcv_swiglu_fwd": [P, P, P, I64, I64, I64, P],
    "lcv_swiglu_bwd": [P, P, P, P, P, I64, I64, I64, P],
    "lcv_swiglu_bwd_interleaved": [P, P, P, I64, I64, P],
    "lcv_patchify": [P, P, I64, I64, I64, I64, I64, I64, P],
    "lcv_unpatchify": [P, P, I64, I64, I64, I64, I64, I, P],
    "lcv_unpatchify_bwd": [P, P, I64, I64, I64, I64, I64, P],
    "lcv_cfg_euler_step": [P, P, P, P, I64, I64, F32, F32, I, I, P],
    "lcv_euler_step": [P, P, I64, F32, I, P],
    "lcv_fm_noise": [P, P, P, P, I64, I64, P],
    "lcv_fm_mse": [P, P, P, P, P, P, I64, I64, I64, I64, I64, P],
    "lcv_fm_mse_samples": [P, P, P, P, P, I64, I64, I64, I64, I64, I64, I64, P],
    "lcv_grad_norm_clip": [P, I64, I64, I, F32, P, P, P],
    "lcv_adamw_step": [P, I64, I64, I, P, F64, F64, F64, F64, F64, I64, P],
    "lcv_sgd_step": [P, I64, I64, I, P, F64, F64, P],
    "lcv_transpose_pad": [P, P, I64, I64, I64, I64, P],
    "lcv_rowsum": [P, P, I64, I64, I, P],
    "lcv_linear_f32_smallm_wgrad": [P, P, P, P, I64, I64, I64, I, P],
    "lcv_gelu_tanh_fwd": [P, P, I64, P],
    "lcv_gelu_tanh_bwd": [P, P, P, I64, P],
    "lcv_causal_conv3d": [P, P, P, P, P, P, I64, I64, I64, I64, I64, I64, I64, I, I, I, I, P],
    "lcv_conv3d_strided": [P, P, P, P, P, I64, I64, I64, I64, I64, I64, I64, I, I, I, I, I, I, I64, I64, I64, P],
    "lcv_vae_rmsnorm_silu": [P, P, P, I64, I64, I64, I, P],
    "lcv_softmax_rows": [P, P, I64, I64, I64, I64, F32, P],
    "lcv_gather_rows": [P, P, P, I64, I64, I64, P],
    "lcv_t5_rmsnorm": [P, P, P, I64, I64, F32, P],
    "lcv_geglu_tanh_fwd": [P, P, P, I64, I64, I64, P],
    "lcv_t5_attention": [P, P, P, P, P, P, I64, I64, I64, I64, I64, I64, I64, P],
    "lcv_frame_metric_partials": [I64, I64, I64, I, P, P],
    "lcv_frame_sqerr": [P, P, I, P, I64, I64, P],
    "lcv_frame_ssim": [P, P, I, P, I64, I64, I64, I64, P, I, F32, I, F32, F32, P],
}

# include/lcv_hip_lpips.h (a header of its own: the on-device LPIPS entry points); same convention, every function returns int
_SIGNATURES_LPIPS = {
    "lcv_lpips_pack_weight": [P, P, I64, I64, I64, I64, I64, P],
    "lcv_lpips_conv_relu": [P, P, I, I, P, P, P, P, I64, I64, I64, I64, I64, I64, I64, I64, I64, I64, P],
    "lcv_lpips_maxpool": [P, P, I64, I64, I64, I64, P],
    "lcv_lpips_tap_distance": [P, P, P, P, I, I64, I64, I64, P],
}
LCV_LPIPS_TAP_BLOCKS = 64

# include/lcv_hip_det.h (a header of its own: the fixed-order forms of the atomic reductions); each takes its counterpart's
# arguments plus `void* ws, int64_t ws_bytes` in front of the stream (qknorm: without dw_slots); every function returns int
_SIGNATURES_DET = {
    "lcv_det_adaln_modulate_bwd": [P, P, P, P, P, I64, I64, I64, I64, I64, I64, I64, F32, P, P, I64, P],
    "lcv_det_layernorm_affine_bwd": [P, P, P, P, P, P, I64, I64, F32, P, P, I64, P],
    "lcv_det_gate_residual_bwd": [P, P, P, P, P, I64, I64, I64, I64, I64, I64, P, I64, P],
    "lcv_det_qknorm_rope_bwd": [P, P, P, P, P, P, P, P, P, I64, I64, I64, I64, I64, I64, I64, I64, I64, I64, I64, I64, F32, F32, P, P, P, I64, P],
    "lcv_det_linear_f32_smallm_bwd": [P, P, P, P, I64, I64, I64, I, P, I64, P],
    "lcv_det_grad_norm_clip": [P, I64, I64, I, F32, P, P, P, I64, P],
}
LCV_DET_ADALN, LCV_DET_LAYERNORM, LCV_DET_GATE, LCV_DET_QKNORM, LCV_DET_SMALLM, LCV_DET_GRAD_NORM = range(6)

# include/lcv_hip_lora.h (a header of its own: the LoRA dropout kernels); `p` is a double, seed / offset are uint64, row0 is the
# global index of the first row; every function returns int
_SIGNATURES_LORA = {
    "lcv_lora_down_dropout": [P, P, P, I64, I64, I64, I64, I64, F32, F64, U64, U64, I64, P],
    "lcv_tn_skinny_dropout": [P, P, P, I64, I64, I64, I64, I64, F32, F64, U64, U64, I64, P, I64, P],
    "lcv_lora_dx_dropout_add": [P, P, P, I64, I64, I64, I64, I64, F64, U64, U64, I64, P],
    "lcv_lora_dropout_mask": [P, I64, I64, F64, U64, U64, I64, P],
}

# include/lcv_hip_master.h (a header of its own: fp32 master weights for bf16 parameters); `low` is a device array of pointers
# to the int16 low words, parallel to the descriptor table; every function returns int
_SIGNATURES_MASTER = {
    "lcv_master_sgd_step": [P, P, I64, I64, P, F64, F64, P],
    "lcv_master_adamw_step": [P, P, I64, I64, P, F64, F64, F64, F64, F64, I64, P],
    "lcv_master_split": [P, P, P, I64, P],
    "lcv_master_join": [P, P, P, I64, P],
}

# include/lcv_hip_moments8.h (a header of its own: 8-bit block-scaled AdamW moments for master weights); `scales` of the step is
# a device array of pointers to fp32 [2][ceil(numel/512)], parallel to the descriptor table; every function returns int
_SIGNATURES_MOMENTS8 = {
    "lcv_master_adamw8_step": [P, P, P, I64, I64, P, F64, F64, F64, F64, F64, I64, P],
    "lcv_moments8_encode": [P, P, P, P, P, I64, P],
    "lcv_moments8_decode": [P, P, P, P, P, I64, P],
}

# include/lcv_hip_accum.h (a header of its own: fp32 gradient accumulation over micro-steps); `acc` is a device array of pointers
# to the fp32 accumulators, parallel to the descriptor table; the g32 steps take their lcv_master_* counterparts' arguments with
# `grad` of the table pointing to fp32; every function returns int
_SIGNATURES_ACCUM = {
    "lcv_grad_accumulate": [P, P, I64, I64, F64, P],
    "lcv_master_sgd_step_g32": [P, P, I64, I64, P, F64, F64, P],
    "lcv_master_adamw_step_g32": [P, P, I64, I64, P, F64, F64, F64, F64, F64, I64, P],
}

# include/lcv_hip_anchor.h (a header of its own: decay toward the base weights and the drift norm); `anchor` is a device array of
# pointers to the bf16 base words, parallel to the descriptor table; the steps take their counterparts' arguments with `anchor`
# after `low` (after `scales` in the 8-bit form) and `grad_f32` in front of the stream; every function returns int
_SIGNATURES_ANCHOR = {
    "lcv_master_sgd_step_anchor": [P, P, P, I64, I64, P, F64, F64, I, P],
    "lcv_master_adamw_step_anchor": [P, P, P, I64, I64, P, F64, F64, F64, F64, F64, I64, I, P],
    "lcv_master_adamw8_step_anchor": [P, P, P, P, I64, I64, P, F64, F64, F64, F64, F64, I64, P],
    "lcv_master_drift_sumsq": [P, P, P, I64, I64, P, I64, P, P],
}

# include/lcv_hip_ema.h (a header of its own: the fp32 weight average over the optimizer steps); `ema` is a device array of pointers
# to the fp32 averages, parallel to the descriptor table, after `low`; update takes beta in front of the stream; all return int
_SIGNATURES_EMA = {
    "lcv_master_ema_load": [P, P, P, I64, I64, P],
    "lcv_master_ema_update": [P, P, P, I64, I64, F64, P],
    "lcv_master_ema_swap": [P, P, P, I64, I64, P],
}

# include/lcv_hip_stepcache.h (a header of its own: the first-block step cache of the denoise loop); diff takes (x0, x1, prev, r_out,
# rows, n, float thr, partials, partials_bytes, out), store (xL, x1, R, total), apply (x1, R, out, total); all return int
_SIGNATURES_STEPCACHE = {
    "lcv_stepcache_diff": [P, P, P, P, I64, I64, F32, P, I64, P, P],
    "lcv_stepcache_store": [P, P, P, I64, P],
    "lcv_stepcache_apply": [P, P, P, I64, P],
}

# include/lcv_hip_solver.h (a header of its own: the linear multistep update of the denoise loop): (cond, uncond, x, f0, f1, f2, ws,
# B, n, float guidance, float w0, w1, w2, int terms, negate, use_zero_star); returns int
_SIGNATURES_SOLVER = {
    "lcv_cfg_lms_step": [P, P, P, P, P, P, P, I64, I64, F32, F32, F32, F32, I, I, I, P],
}

# include/lcv_hip_cfgreuse.h (a header of its own: the guidance reuse of the CFG denoise loop): store takes (cond, uncond, delta, ws,
# out, B, n, float guidance, int use_zero_star), apply (cond, delta, v, B, n); both return int
_SIGNATURES_CFGREUSE = {
    "lcv_cfg_delta_store": [P, P, P, P, P, I64, I64, F32, I, P],
    "lcv_cfg_delta_apply": [P, P, P, I64, I64, P],
}

# include/lcv_hip_apg.h (a header of its own: the adaptive projected guidance of the CFG denoise loop): (cond, uncond, diff, v, ws, out,
# B, n, float guidance, eta, radius, beta, int use_zero_star, have_momentum); returns int
_SIGNATURES_APG = {
    "lcv_cfg_apg": [P, P, P, P, P, P, I64, I64, F32, F32, F32, F32, I, I, P],
}

# include/lcv_hip_sr.h (a header of its own: stochastic rounding for the bf16 optimizer steps): the steps take lcv_master_*_step's
# arguments without `low` and with uint64 `seed, offset` in front of the stream; round takes (x fp32, out bf16, n, seed, offset)
_SIGNATURES_SR = {
    "lcv_sr_sgd_step": [P, I64, I64, P, F64, F64, U64, U64, P],
    "lcv_sr_adamw_step": [P, I64, I64, P, F64, F64, F64, F64, F64, I64, U64, U64, P],
    "lcv_sr_round": [P, P, I64, U64, U64, P],
}

# include/lcv_hip_dora.h (a header of its own: the row norm and the column scale of weight-decomposed LoRA): norm takes (w, a, b,
# double scaling, N, K, R, wn_out), fwd (pre, m, wn, bias, y, M, N), bwd (dy, pre, m, wn, dpre, dm, ws, ws_bytes, M, N); all return int
_SIGNATURES_DORA = {
    "lcv_dora_weight_norm": [P, P, P, F64, I64, I64, I64, P, P],
    "lcv_dora_colscale_fwd": [P, P, P, P, P, I64, I64, P],
    "lcv_dora_colscale_bwd": [P, P, P, P, P, P, P, I64, I64, I64, P],
}
LCV_DORA_NORM_KTILE, LCV_DORA_NORM_ROWS, LCV_DORA_SLAB, LCV_DORA_SLAB_QUARTER = 512, 16, 64, 16

# include/lcv_hip_trust.h (a header of its own: the trust-region cap on the drift from the base weights): sumsq takes (tensors, low,
# anchor, n_tensors, total_chunks, int param_f32, partials, partials_bytes, per_tensor, out), project (tensors, low, anchor, n_tensors,
# total_chunks, int param_f32, int scope, sumsq, per_tensor, double r2_or_R2, trace_slot); both return int
_SIGNATURES_TRUST = {
    "lcv_trust_sumsq": [P, P, P, I64, I64, I, P, I64, P, P, P],
    "lcv_trust_project": [P, P, P, I64, I64, I, I, P, P, F64, P, P],
}
LCV_TRUST_GLOBAL, LCV_TRUST_TENSOR = 0, 1

# include/lcv_hip_sam.h (a header of its own: the sharpness-aware adaptation step): sumsq takes (tensors, low, n_tensors,
# total_chunks, int param_f32, int adaptive, double eta, partials, partials_bytes, per_tensor, out), perturb (tensors, low, save,
# n_tensors, total_chunks, int param_f32, int adaptive, double eta, double rho, sumsq, partials, partials_bytes, per_tensor, realized,
# trace_slot), restore (tensors, save, n_tensors, total_chunks, int param_f32); all return int
_SIGNATURES_SAM = {
    "lcv_sam_sumsq": [P, P, I64, I64, I, I, F64, P, I64, P, P, P],
    "lcv_sam_perturb": [P, P, P, I64, I64, I, I, F64, F64, P, P, I64, P, P, P, P],
    "lcv_sam_restore": [P, P, I64, I64, I, P],
}

LCV_EPI_NONE, LCV_EPI_SWIGLU, LCV_EPI_GATE_RESIDUAL, LCV_EPI_GELU_TANH, LCV_EPI_SILU = 0, 1, 2, 3, 4


class LcvError(RuntimeError):
    """`code` is the library's return value when the error came from a C-ABI call (LCV_EINVAL -1: the caller's arguments;
    LCV_EDEVICE -2 / LCV_ELAUNCH -3: the device or a launch failed — the HIP context may be unusable afterwards)."""
    code = None

    @property
    def fatal(self) -> bool:
        return self.code in (-2, -3)


_lib = None


def lib_path() -> Path:
    return _LIB_PATH


def load():
    """Load the shared library once; raise loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not _LIB_PATH.exists():
        raise LcvError(
            f"{_LIB_PATH} is missing: build it with `python __graft_entry__.py` (hipcc, gfx950). "
            "There is no fallback path.")
    # torch first: it carries its own libamdhip64 under the soname this library links to; if the system ROCm copy were
    # loaded before it, the process would hold two HIP runtimes and torch would then find no GPU
    import torch  # noqa: F401
    lib = ctypes.CDLL(str(_LIB_PATH), mode=os.RTLD_NOW | getattr(os, "RTLD_LOCAL", 0))
    lib.lcv_version.restype = c_int
    lib.lcv_version.argtypes = []
    lib.lcv_last_error.restype = c_char_p
    lib.lcv_last_error.argtypes = []
    lib.lcv_attn_fwd_last_kernel.restype = c_char_p
    lib.lcv_attn_fwd_last_kernel.argtypes = []
    lib.lcv_knobs_list.restype = c_char_p
    lib.lcv_knobs_list.argtypes = []
    lib.lcv_knobs_reload.restype = c_int           # a count, not a status
    lib.lcv_knobs_reload.argtypes = []
    lib.lcv_conv3d_last_kernel.restype = c_char_p
    lib.lcv_conv3d_last_kernel.argtypes = []
    lib.lcv_tn_skinny_ws_bytes.restype = c_int64     # a size, not a status
    lib.lcv_tn_skinny_ws_bytes.argtypes = [I64, I64, I64]
    lib.lcv_attn_bwd_ws_floats.restype = c_int64     # likewise
    lib.lcv_attn_bwd_ws_floats.argtypes = [I64, I64, I64, I64]
    lib.lcv_lpips_ws_bytes.restype = c_int64         # likewise
    lib.lcv_lpips_ws_bytes.argtypes = [I64, I64, I64]
    lib.lcv_det_ws_bytes.restype = c_int64           # likewise
    lib.lcv_det_ws_bytes.argtypes = [I, I64, I64, I64]
    lib.lcv_tn_skinny_dropout_ws_bytes.restype = c_int64   # likewise
    lib.lcv_tn_skinny_dropout_ws_bytes.argtypes = [I64, I64, I64]
    lib.lcv_dora_colscale_bwd_ws_bytes.restype = c_int64   # likewise
    lib.lcv_dora_colscale_bwd_ws_bytes.argtypes = [I64, I64]
    for name, args in (list(_SIGNATURES.items()) + list(_SIGNATURES_LPIPS.items()) + list(_SIGNATURES_DET.items())
                       + list(_SIGNATURES_LORA.items()) + list(_SIGNATURES_MASTER.items()) + list(_SIGNATURES_MOMENTS8.items())
                       + list(_SIGNATURES_ACCUM.items()) + list(_SIGNATURES_ANCHOR.items()) + list(_SIGNATURES_EMA.items())
                       + list(_SIGNATURES_STEPCACHE.items()) + list(_SIGNATURES_SOLVER.items())
                       + list(_SIGNATURES_CFGREUSE.items()) + list(_SIGNATURES_SR.items()) + list(_SIGNATURES_APG.items())
                       + list(_SIGNATURES_DORA.items()) + list(_SIGNATURES_TRUST.items())
                       + list(_SIGNATURES_SAM.items())):
        fn = getattr(lib, name, None)
        if fn is None:
            continue  # export coverage is asserted by tests/test_abi.py against include/lcv_hip.h
        fn.restype = c_int
        fn.argtypes = args
    _lib = lib
    return lib


def reload_knobs() -> int:
    """The library reads its LCV_* A/B knobs once (include/lcv_hip.h); call this after changing one in os.environ."""
    return load().lcv_knobs_reload()


def set_knob(name: str, value) -> None:
    """Set (or, with None, unset) an A/B knob in os.environ and make the library see it."""
    if value is None:
        os.environ.pop(name, None)
    else:
        os.environ[name] = str(value)
    if _lib is not None:
        _lib.lcv_knobs_reload()


def call(name: str, *args):
    lib = load()
    fn = getattr(lib, name)
    rc = fn(*args)
    if rc != 0:
        msg = lib.lcv_last_error()
        err = LcvError(f"{name} failed ({rc}): {msg.decode() if msg else ''}")
        err.code = rc
        raise err

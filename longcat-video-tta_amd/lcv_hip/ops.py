"""Tensor-level wrappers over the C ABI (forward kernels).

PyTorch is plumbing here: it owns device memory and the stream; every op below
hands raw pointers + sizes to liblcv_hip.so.  Nothing in this module computes
with torch operators.
"""
import os
from typing import Optional, Tuple

import torch

from . import lib as _lib
from .lib import (LCV_EPI_GATE_RESIDUAL, LCV_EPI_GELU_TANH, LCV_EPI_NONE, LCV_EPI_SILU, LCV_EPI_SWIGLU,
                  call)

BF16 = torch.bfloat16
F32 = torch.float32
PROFILE = None  # set to a list by bench.py to collect (start, end, flops, Nq, Nk) per attention launch
PROFILE_BWD = None  # likewise for attention_bwd: (start, end, algorithmic flops = 10 B H Nq Nk D, Nq, Nk) per call


# Deterministic mode: the six wrappers whose default kernels finish a sum with fp32 atomics (the AdaLN / LayerNorm / gate /
# q-k-norm parameter gradients, the small-M linear's input gradient, the gradient-norm clip) call the fixed-order entry points
# of include/lcv_hip_det.h instead.  Same data gradients bit for bit; the reduced outputs become a pure function of the
# inputs, so one process gives the same bits for the same seed.  Off unless LCV_DETERMINISTIC=1 (read once, here) or
# set_deterministic(True).  It covers one process: the order inside RCCL's collectives (sequence parallelism) is not ours.
_DETERMINISTIC = os.environ.get("LCV_DETERMINISTIC", "") == "1"


def set_deterministic(flag: bool) -> None:
    global _DETERMINISTIC
    _DETERMINISTIC = bool(flag)


def is_deterministic() -> bool:
    return _DETERMINISTIC


def _det_ws(kind: int, device, d0: int, d1: int = 0, d2: int = 0):
    """(workspace, bytes) for a fixed-order entry point, from the caching allocator (as tn_skinny's)."""
    n = int(_lib.load().lcv_det_ws_bytes(kind, d0, d1, d2))
    if n < 0:
        raise _lib.LcvError(f"lcv_det_ws_bytes: unknown kind {kind}")
    return torch.empty((max(n, 16) // 4,), dtype=F32, device=device), n


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _req(t: torch.Tensor, dtype, name: str):
    if not t.is_cuda:
        raise _lib.LcvError(f"{name}: tensor must live on the GPU (no CPU path exists)")
    if t.dtype != dtype:
        raise _lib.LcvError(f"{name}: expected {dtype}, got {t.dtype}")


# ----------------------------------------------------------------- norms ---
def adaln_modulate(x: torch.Tensor, mod: torch.Tensor, shift_idx: int, scale_idx: int, T: int,
                   eps: float = 1e-6) -> torch.Tensor:
    """x [B, T*S, C] bf16; mod [B, T, k*C] fp32; chunk indices select shift/scale."""
    _req(x, BF16, "adaln_modulate.x"); _req(mod, F32, "adaln_modulate.mod")
    B, N, C = x.shape
    x = x.contiguous(); mod = mod.contiguous()
    y = torch.empty_like(x)
    call("lcv_adaln_modulate_fwd", _ptr(x), _ptr(mod), _ptr(y), B, T, N // T, C, mod.shape[-1],
         shift_idx * C, scale_idx * C, eps, _stream())
    return y


def layernorm_affine(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, eps: float = 1e-6) -> torch.Tensor:
    _req(x, BF16, "layernorm_affine.x")
    C = x.shape[-1]
    x = x.contiguous()
    wf = w.detach().to(F32).contiguous(); bf = b.detach().to(F32).contiguous()
    y = torch.empty_like(x)
    call("lcv_layernorm_affine_fwd", _ptr(x), _ptr(wf), _ptr(bf), _ptr(y), x.numel() // C, C, eps, _stream())
    return y


def gate_residual(x: torch.Tensor, y: torch.Tensor, mod: Optional[torch.Tensor], gate_idx: int, T: int) -> torch.Tensor:
    _req(x, BF16, "gate_residual.x"); _req(y, BF16, "gate_residual.y")
    B, N, C = x.shape
    x = x.contiguous(); y = y.contiguous()
    out = torch.empty_like(x)
    if mod is not None:
        _req(mod, F32, "gate_residual.mod")
        mod = mod.contiguous()
        call("lcv_gate_residual_fwd", _ptr(x), _ptr(y), _ptr(mod), _ptr(out), B, T, N // T, C, mod.shape[-1],
             gate_idx * C, _stream())
    else:
        call("lcv_gate_residual_fwd", _ptr(x), _ptr(y), None, _ptr(out), B, 1, N, C, 0, 0, _stream())
    return out


def timestep_embedding(t: torch.Tensor, dim: int, max_period: float = 10000.0) -> torch.Tensor:
    """t fp32 [n] -> [n, dim] fp32 (cos | sin)."""
    _req(t, F32, "timestep_embedding.t")
    t = t.contiguous().view(-1)
    out = torch.empty((t.numel(), dim), dtype=F32, device=t.device)
    call("lcv_timestep_embedding", _ptr(t), _ptr(out), t.numel(), dim, float(max_period), _stream())
    return out


# ------------------------------------------------------- q/k norm + rope ---
def qknorm_rope(q_in: Optional[torch.Tensor], k_in: Optional[torch.Tensor], v_in: Optional[torch.Tensor],
                q_out: Optional[torch.Tensor], k_out: Optional[torch.Tensor], v_out: Optional[torch.Tensor],
                wq: torch.Tensor, wk: torch.Tensor, cs: Optional[torch.Tensor], pos_off: int = 0,
                eps: float = 1e-6, q_scale: float = 1.0) -> None:
    """All tensors are [B, N, H, 128] views with contiguous (H, D); in-place allowed (out is in).
    q_scale multiplies the q output before its bf16 rounding (see `LOG2_QSCALE`)."""
    ref = q_in if q_in is not None else k_in
    B, N, H, D = ref.shape
    if D != 128:
        raise _lib.LcvError("qknorm_rope: head_dim must be 128")

    def chk(t, name):
        if t is None:
            return
        _req(t, BF16, name)
        if t.stride(3) != 1 or t.stride(2) != D:
            raise _lib.LcvError(f"{name}: (H, D) must be contiguous")

    for t, nme in ((q_in, "q_in"), (k_in, "k_in"), (v_in, "v_in"), (q_out, "q_out"), (k_out, "k_out"), (v_out, "v_out")):
        chk(t, "qknorm_rope." + nme)
    ins = [t for t in (q_in, k_in, v_in) if t is not None]
    if any(t.stride(0) != ins[0].stride(0) or t.stride(1) != ins[0].stride(1) for t in ins):
        raise _lib.LcvError("qknorm_rope: q_in/k_in/v_in must share strides")
    kvs = [t for t in (k_out, v_out) if t is not None]
    if kvs and any(t.stride(0) != kvs[0].stride(0) or t.stride(1) != kvs[0].stride(1) for t in kvs):
        raise _lib.LcvError("qknorm_rope: k_out/v_out must share strides")
    if cs is not None:
        _req(cs, F32, "qknorm_rope.cs")
        if cs.shape[0] < pos_off + N:
            raise _lib.LcvError("qknorm_rope: cos/sin table shorter than pos_off + N")
    qo = q_out if q_out is not None else ref
    ko = kvs[0] if kvs else ref
    call("lcv_qknorm_rope_fwd", _ptr(q_in), _ptr(k_in), _ptr(v_in), _ptr(q_out), _ptr(k_out), _ptr(v_out),
         _ptr(wq), _ptr(wk), _ptr(cs), B, N, H, ins[0].stride(0), ins[0].stride(1), qo.stride(0), qo.stride(1),
         ko.stride(0), ko.stride(1), pos_off, eps, q_scale, _stream())


# The self-attention path folds its softmax scale into q: q' = q * scale * log2(e) (in the q norm/RoPE kernel, before
# the bf16 rounding) and calls the attention kernels with scale = ln 2, so that exp(scale * q'.k) == exp2(q'.k).
LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453


def log2_qscale(scale: float) -> float:
    return scale * LOG2E


# -------------------------------------------------------------- attention ---
def attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: float,
              out: Optional[torch.Tensor] = None, need_lse: bool = False) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """q [B,Nq,H,128], k/v [B,Nk,H,128] (any strides with contiguous D) -> o [B,Nq,H,128], lse [B,H,Nq]."""
    for t, nme in ((q, "q"), (k, "k"), (v, "v")):
        _req(t, BF16, "attention." + nme)
        if t.shape[-1] != 128 or t.stride(-1) != 1:
            raise _lib.LcvError("attention: head_dim must be 128 and contiguous")
    B, Nq, H, D = q.shape
    Nk = k.shape[1]
    if out is None:
        out = torch.empty((B, Nq, H, D), dtype=BF16, device=q.device)
    lse = torch.empty((B, H, Nq), dtype=F32, device=q.device) if need_lse else None
    if PROFILE is not None:  # bench.py: HIP events on the launch stream around the dominant kernel
        ev0 = torch.cuda.Event(enable_timing=True); ev1 = torch.cuda.Event(enable_timing=True)
        ev0.record()
    call("lcv_attn_fwd", _ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(lse), B, H, Nq, Nk,
         q.stride(0), q.stride(1), q.stride(2), k.stride(0), k.stride(1), k.stride(2),
         v.stride(0), v.stride(1), v.stride(2), out.stride(0), out.stride(1), out.stride(2),
         float(scale), _stream())
    if PROFILE is not None:
        ev1.record()
        PROFILE.append((ev0, ev1, 4.0 * B * H * Nq * Nk * D, Nq, Nk, _lib.load().lcv_attn_fwd_last_kernel().decode()))
    return out, lse


# ------------------------------------------------------------------ GEMMs ---
_GEMM_WS = {}   # device index -> the split-K tail workspace handed to the library (kept alive here)
GEMM_WS_BYTES = 256 << 20


def _ensure_gemm_workspace(device: torch.device) -> None:
    """Give liblcv_hip.so its split-K tail workspace once per process (one process per GPU): the library never allocates."""
    idx = device.index if device.index is not None else torch.cuda.current_device()
    if idx not in _GEMM_WS:
        if _GEMM_WS:                       # a second device in the same process: the library holds ONE workspace
            raise _lib.LcvError(
                f"gemm_nt on cuda:{idx}, but this process already bound the library's split-K workspace to cuda:"
                f"{next(iter(_GEMM_WS))}: the build runs one process per GPU (torch.distributed), a second device in the "
                "same process would write its partial sums into the first device's memory")
        ws = torch.empty(GEMM_WS_BYTES, dtype=torch.uint8, device=device)
        call("lcv_gemm_set_workspace", _ptr(ws), GEMM_WS_BYTES)
        _GEMM_WS[idx] = ws


# Bumped by every fused optimizer step: those kernels write parameters through raw pointers, which never touches a tensor's
# `_version`.  Whoever caches something derived from TRAINABLE weights (the interleaved SwiGLU weight) keys it on this.
PARAM_EPOCH = 0


def gemm_nt(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, *,
            a2: Optional[torch.Tensor] = None, w2: Optional[torch.Tensor] = None,
            epilogue: int = LCV_EPI_NONE, out_f32: bool = False, resid: Optional[torch.Tensor] = None,
            mod: Optional[torch.Tensor] = None, gate_idx: int = 0, rows_per_frame: int = 1,
            out: Optional[torch.Tensor] = None, swiglu_aux: Optional[torch.Tensor] = None) -> torch.Tensor:
    """c[M,N] = a[M,K] @ w[N,K]^T (+ a2 @ w2^T) + bias with a fused epilogue.  `swiglu_aux` (SwiGLU epilogue only): a
    contiguous bf16 [M, N] tensor that receives the pre-activation (gate | up) rows for the backward."""
    _req(a, BF16, "gemm_nt.a"); _req(w, BF16, "gemm_nt.w")
    if a.shape[0] >= 2048:
        _ensure_gemm_workspace(a.device)
    if a.dim() != 2 or w.dim() != 2 or a.stride(1) != 1 or w.stride(1) != 1:
        raise _lib.LcvError("gemm_nt: a and w must be 2-D with contiguous rows")
    M, K = a.shape
    N = w.shape[0]
    if w.shape[1] != K:
        raise _lib.LcvError(f"gemm_nt: K mismatch ({K} vs {w.shape[1]})")
    if K % 64:  # rare (toy shapes): zero-pad the contraction dim to the kernel's 64-deep K step
        pad = 64 - K % 64
        a = torch.nn.functional.pad(a, (0, pad))
        w = torch.nn.functional.pad(w, (0, pad))
        K += pad
    K2 = 0
    if a2 is not None:
        _req(a2, BF16, "gemm_nt.a2"); _req(w2, BF16, "gemm_nt.w2")
        K2 = a2.shape[1]
    n_out = N // 2 if epilogue == LCV_EPI_SWIGLU else N
    if out is None:
        out = torch.empty((M, n_out), dtype=F32 if out_f32 else BF16, device=a.device)
    if bias is not None:
        _req(bias, BF16, "gemm_nt.bias")
    if swiglu_aux is not None:
        _req(swiglu_aux, BF16, "gemm_nt.swiglu_aux")
        if epilogue != LCV_EPI_SWIGLU or resid is not None or swiglu_aux.shape != (M, N) or not swiglu_aux.is_contiguous():
            raise _lib.LcvError("gemm_nt: swiglu_aux needs the SwiGLU epilogue and a contiguous [M, N] tensor")
        resid = swiglu_aux          # the C entry point takes it through `resid` (an output under this epilogue)
    C = N
    mod_stride = 0
    if mod is not None:
        _req(mod, F32, "gemm_nt.mod")
        mod_stride = mod.shape[-1]
    call("lcv_gemm_nt", _ptr(a), _ptr(w), _ptr(bias), _ptr(a2), _ptr(w2), _ptr(out), M, N, K, K2,
         a.stride(0), w.stride(0), a2.stride(0) if a2 is not None else 0, w2.stride(0) if w2 is not None else 0,
         out.stride(0), epilogue, 1 if out_f32 else 0, _ptr(resid), _ptr(mod), rows_per_frame, mod_stride,
         gate_idx * C, _stream())
    return out


def linear_f32_smallm(a: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], act_in: int = 0) -> torch.Tensor:
    """fp32 islands: out[M,N] fp32 = act(a fp32) @ w(bf16)^T + bias."""
    _req(a, F32, "linear_f32_smallm.a"); _req(w, BF16, "linear_f32_smallm.w")
    a = a.contiguous()
    M, K = a.shape
    N = w.shape[0]
    out = torch.empty((M, N), dtype=F32, device=a.device)
    call("lcv_linear_f32_smallm", _ptr(a), _ptr(w.contiguous()), _ptr(bias), _ptr(out), M, N, K, act_in, _stream())
    return out


def _lora_down(name: str, x: torch.Tensor, A: torch.Tensor, s: float, rpad: int, draw=()) -> torch.Tensor:
    """lcv_lora_down (draw empty) or lcv_lora_down_dropout (draw = _draw(...)): the output and the call."""
    M, K = x.shape
    h = torch.empty((M, rpad), dtype=BF16, device=x.device)
    call(name, _ptr(x), _ptr(A.contiguous()), _ptr(h), M, K, A.shape[0], rpad, x.stride(0), float(s), *draw, _stream())
    return h


def lora_down(x: torch.Tensor, A: torch.Tensor, s: float, rpad: int = 64) -> torch.Tensor:
    _req(x, BF16, "lora_down.x"); _req(A, BF16, "lora_down.A")
    return _lora_down("lcv_lora_down", x, A, s, rpad)


# ------------------------------------------------------------ LoRA dropout ---
# include/lcv_hip_lora.h: the mask is a pure function of (seed, offset, global element index); `row0` is the global index of
# the tensor's first row (0 unless the caller holds a slice of a larger matrix)
_U64 = (1 << 64) - 1


def draw_philox_offset(device: torch.device) -> Tuple[int, int]:
    """One (seed, offset) pair for one Philox draw (a LoRA dropout mask, the rounding bits of one optimizer step), from the
    device's default generator: its seed and its current Philox offset, which is then advanced by 4 (the granularity the
    generator accepts).  Host-side state only: no device-to-host sync.  It follows torch.manual_seed, and
    torch.utils.checkpoint's RNG preservation replays it for a recomputed block."""
    index = device.index if device.index is not None else torch.cuda.current_device()
    gen = torch.cuda.default_generators[index]
    seed, offset = gen.initial_seed(), gen.get_offset()
    gen.set_offset(offset + 4)
    return seed, offset


def sr_round(x: torch.Tensor, seed: int, offset: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bf16 of the fp32 `x`, rounded stochastically with stream 0 and group i >> 3 of (seed, offset) (include/lcv_hip_sr.h): the
    rounding of the --stochastic-rounding optimizer steps on an array of its own."""
    _req(x, F32, "sr_round.x")
    if not x.is_contiguous():
        raise _lib.LcvError("sr_round: x must be contiguous")
    out = torch.empty(x.shape, dtype=BF16, device=x.device) if out is None else out
    _req(out, BF16, "sr_round.out")
    if out.numel() != x.numel() or not out.is_contiguous():
        raise _lib.LcvError("sr_round: out must be contiguous with x's element count")
    if x.numel():
        call("lcv_sr_round", _ptr(x), _ptr(out), x.numel(), int(seed) & _U64, int(offset) & _U64, _stream())
    return out


def _draw(p: float, seed: int, offset: int, row0: int) -> tuple:
    """The four mask arguments as the C ABI takes them."""
    return float(p), int(seed) & _U64, int(offset) & _U64, int(row0)


def lora_down_dropout(x: torch.Tensor, A: torch.Tensor, s: float, p: float, seed: int, offset: int, rpad: int = 64,
                      row0: int = 0) -> torch.Tensor:
    """h [M, rpad] = bf16(s * bf16(xd A^T)), xd = bf16(x * mask * scale), zero padded."""
    _req(x, BF16, "lora_down_dropout.x"); _req(A, BF16, "lora_down_dropout.A")
    if x.dim() != 2 or x.stride(1) != 1:
        raise _lib.LcvError("lora_down_dropout: x must be 2-D with contiguous rows")
    return _lora_down("lcv_lora_down_dropout", x, A, s, rpad, _draw(p, seed, offset, row0))


def tn_skinny_dropout(g: torch.Tensor, x: torch.Tensor, R: int, p: float, seed: int, offset: int, scale: float = 1.0,
                      row0: int = 0) -> torch.Tensor:
    """out[R, K] fp32 = scale * g[:, :R]^T @ xd  (g [M, Rpad] bf16 contiguous, x [M, K] bf16): the mask sits on x."""
    _req(g, BF16, "tn_skinny_dropout.g"); _req(x, BF16, "tn_skinny_dropout.x")
    if x.dim() != 2 or x.stride(1) != 1 or not g.is_contiguous():
        raise _lib.LcvError("tn_skinny_dropout: x must be 2-D with contiguous rows, g contiguous")
    return _tn_skinny("lcv_tn_skinny_dropout", g, x, R, scale, _draw(p, seed, offset, row0))


def lora_dx_dropout_add(dx: torch.Tensor, g: torch.Tensor, A: torch.Tensor, p: float, seed: int, offset: int,
                        row0: int = 0) -> torch.Tensor:
    """dx[m, k] = bf16(dx[m, k] + mask * scale * sum_r g[m, r] A[r, k]) in place (dx [M, K] bf16 contiguous,
    g [M, Rpad] bf16, A [R, K] bf16); returns dx."""
    _req(dx, BF16, "lora_dx_dropout_add.dx"); _req(g, BF16, "lora_dx_dropout_add.g"); _req(A, BF16, "lora_dx_dropout_add.A")
    if dx.dim() != 2 or not dx.is_contiguous() or g.dim() != 2 or g.stride(1) != 1:
        raise _lib.LcvError("lora_dx_dropout_add: dx must be 2-D contiguous, g 2-D with contiguous rows")
    M, K = dx.shape
    R = A.shape[0]
    call("lcv_lora_dx_dropout_add", _ptr(dx), _ptr(g), _ptr(A.contiguous()), M, K, R, g.shape[1], g.stride(0),
         *_draw(p, seed, offset, row0), _stream())
    return dx


def lora_dropout_mask(M: int, K: int, p: float, seed: int, offset: int, row0: int = 0, device="cuda") -> torch.Tensor:
    """The 0 / 1 mask of rows [row0, row0 + M) as uint8 [M, K]: what the three kernels above regenerate."""
    out = torch.empty((M, K), dtype=torch.uint8, device=device)
    _req(out, torch.uint8, "lora_dropout_mask.out")
    call("lcv_lora_dropout_mask", _ptr(out), M, K, *_draw(p, seed, offset, row0), _stream())
    return out


# ---------------------------------------------------- weight-decomposed LoRA ---
# include/lcv_hip_dora.h: wn = |W + s B A| per row, and the column scale c = m / wn of the LoRA GEMM's output
def dora_weight_norm(w: torch.Tensor, A: Optional[torch.Tensor] = None, B: Optional[torch.Tensor] = None, s: float = 0.0,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """wn fp32 [N] = |w[n, :] + s * B[n, :] A|_2 (w bf16 [N, K], A bf16 [R, K], B bf16 [N, R]); without A and B, |w[n, :]|_2."""
    _req(w, BF16, "dora_weight_norm.w")
    if w.dim() != 2 or not w.is_contiguous():
        raise _lib.LcvError("dora_weight_norm: w must be 2-D and contiguous")
    N, K = w.shape
    if (A is None) != (B is None):
        raise _lib.LcvError("dora_weight_norm: A and B come together")
    R = 0
    if A is not None:
        _req(A, BF16, "dora_weight_norm.A"); _req(B, BF16, "dora_weight_norm.B")
        R = A.shape[0]
        if A.shape != (R, K) or B.shape != (N, R) or not A.is_contiguous() or not B.is_contiguous():
            raise _lib.LcvError("dora_weight_norm: A must be [R, K] and B [N, R], both contiguous")
    out = torch.empty((N,), dtype=F32, device=w.device) if out is None else out
    _req(out, F32, "dora_weight_norm.out")
    if out.shape != (N,) or not out.is_contiguous():
        raise _lib.LcvError("dora_weight_norm: out must be a contiguous [N] tensor")
    call("lcv_dora_weight_norm", _ptr(w), _ptr(A), _ptr(B), float(s), N, K, R, _ptr(out), _stream())
    return out


def _dora_req(name: str, N: int, m: torch.Tensor, wn: torch.Tensor, *mats) -> None:
    _req(m, F32, name + ".m"); _req(wn, F32, name + ".wn")
    if m.shape != (N,) or wn.shape != (N,) or not m.is_contiguous() or not wn.is_contiguous():
        raise _lib.LcvError(f"{name}: m and wn must be contiguous [N] tensors")
    for t in mats:
        _req(t, BF16, name)
        if t.dim() != 2 or t.shape != mats[0].shape or not t.is_contiguous():
            raise _lib.LcvError(f"{name}: the matrices must be 2-D, contiguous and of one shape")


def dora_colscale_fwd(pre: torch.Tensor, m: torch.Tensor, wn: torch.Tensor, bias: Optional[torch.Tensor] = None,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """y = bf16(pre * (m / wn) + bias), column-wise; `out` may be `pre` itself."""
    out = torch.empty_like(pre) if out is None else out
    _dora_req("dora_colscale_fwd", pre.shape[-1], m, wn, pre, out)
    M, N = pre.shape
    if bias is not None:
        _req(bias, BF16, "dora_colscale_fwd.bias")
        if bias.shape != (N,) or not bias.is_contiguous():
            raise _lib.LcvError("dora_colscale_fwd: bias must be a contiguous [N] tensor")
    call("lcv_dora_colscale_fwd", _ptr(pre), _ptr(m), _ptr(wn), _ptr(bias), _ptr(out), M, N, _stream())
    return out


def dora_colscale_bwd(dy: torch.Tensor, pre: torch.Tensor, m: torch.Tensor, wn: torch.Tensor):
    """(dpre bf16 [M, N], dm fp32 [N]) = (dy * (m / wn), (sum_t dy * pre) / wn), the sum in fixed slab order."""
    _dora_req("dora_colscale_bwd", pre.shape[-1], m, wn, dy, pre)
    M, N = pre.shape
    dpre = torch.empty_like(dy)
    dm = torch.empty((N,), dtype=F32, device=dy.device)
    ws_bytes = int(_lib.load().lcv_dora_colscale_bwd_ws_bytes(M, N))
    ws = torch.empty((max(ws_bytes, 16) // 4,), dtype=F32, device=dy.device)    # per-slab partial sums (caching allocator)
    call("lcv_dora_colscale_bwd", _ptr(dy), _ptr(pre), _ptr(m), _ptr(wn), _ptr(dpre), _ptr(dm), _ptr(ws), ws_bytes, M, N, _stream())
    return dpre, dm


def swiglu(gate: torch.Tensor, up: torch.Tensor) -> torch.Tensor:
    _req(gate, BF16, "swiglu.gate"); _req(up, BF16, "swiglu.up")
    rows, F = gate.shape
    if gate.stride(0) != up.stride(0) or gate.stride(1) != 1 or up.stride(1) != 1:
        raise _lib.LcvError("swiglu: gate/up must share the row stride")
    out = torch.empty((rows, F), dtype=BF16, device=gate.device)
    call("lcv_swiglu_fwd", _ptr(gate), _ptr(up), _ptr(out), rows, F, gate.stride(0), _stream())
    return out


# ------------------------------------------------------ patch (un)folding ---
def patchify(x: torch.Tensor, kpad: int) -> torch.Tensor:
    _req(x, BF16, "patchify.x")
    B, Cin, T, H, W = x.shape
    x = x.contiguous()
    tok = torch.empty((B, T * (H // 2) * (W // 2), kpad), dtype=BF16, device=x.device)
    call("lcv_patchify", _ptr(x), _ptr(tok), B, Cin, T, H, W, kpad, _stream())
    return tok


def unpatchify(tok: torch.Tensor, Cout: int, T: int, H: int, W: int) -> torch.Tensor:
    B = tok.shape[0]
    tok = tok.contiguous()
    out = torch.empty((B, Cout, T, H, W), dtype=F32, device=tok.device)
    call("lcv_unpatchify", _ptr(tok), _ptr(out), B, Cout, T, H, W, 1 if tok.dtype == F32 else 0, _stream())
    return out


# ---------------------------------------------------------- denoise glue ---
def _cfg_partials(pairs: int, B: int, device) -> torch.Tensor:
    """The [pairs, B, 256, 2] fp32 partial sums of csrc/cfg_guidance.h (256 pairs per sample and pair of sums, every slot written
    by the launch that reads it), from the caching allocator."""
    return torch.empty((pairs, int(B), 256, 2), dtype=F32, device=device)


def cfg_euler_step(cond: torch.Tensor, uncond: torch.Tensor, x: torch.Tensor, guidance: float, dt: float,
                   negate: bool = True, zero_star: bool = True) -> None:
    _req(cond, F32, "cfg_euler_step.cond"); _req(uncond, F32, "cfg_euler_step.uncond"); _req(x, F32, "cfg_euler_step.x")
    B = x.shape[0]
    n = x.numel() // B
    ws = _cfg_partials(1, B, x.device)
    call("lcv_cfg_euler_step", _ptr(cond.contiguous()), _ptr(uncond.contiguous()), _ptr(x), _ptr(ws), B, n,
         float(guidance), float(dt), 1 if negate else 0, 1 if zero_star else 0, _stream())


def euler_step(v: torch.Tensor, x: torch.Tensor, dt: float, negate: bool = True) -> None:
    _req(v, F32, "euler_step.v"); _req(x, F32, "euler_step.x")
    call("lcv_euler_step", _ptr(v.contiguous()), _ptr(x), x.numel(), float(dt), 1 if negate else 0, _stream())


def cfg_lms_step(cond: torch.Tensor, uncond: Optional[torch.Tensor], x: torch.Tensor, f0: torch.Tensor,
                 f1: Optional[torch.Tensor], f2: Optional[torch.Tensor], guidance: float, weights, negate: bool = True,
                 zero_star: bool = True) -> None:
    """The linear multistep step of include/lcv_hip_solver.h: f0 = the guided velocity of (cond, uncond) (`uncond=None`: cond
    itself), x += weights[0] f0 + weights[1] f1 + weights[2] f2 over as many terms as `weights` has (1 to 3).  x, f0, f1, f2 are
    contiguous fp32 of one size and updated / written in place; the rule behind the weights lives in longcat_video/solver.py."""
    terms = len(weights)
    hist = (f1, f2)[:max(terms - 1, 0)]
    if terms < 1 or terms > 3 or any(h is None for h in hist):
        raise _lib.LcvError(f"cfg_lms_step: {terms} weights need {max(terms - 1, 0)} earlier velocities (1 to 3 terms)")
    _req(cond, F32, "cfg_lms_step.cond"); _req(x, F32, "cfg_lms_step.x"); _req(f0, F32, "cfg_lms_step.f0")
    if uncond is not None:
        _req(uncond, F32, "cfg_lms_step.uncond")
    for name, t in (("x", x), ("f0", f0)) + tuple(zip(("f1", "f2"), hist)):
        _req(t, F32, "cfg_lms_step." + name)
        if not t.is_contiguous() or t.numel() != x.numel():
            raise _lib.LcvError(f"cfg_lms_step.{name}: needs a contiguous tensor of x's size (it is used in place)")
    if cond.numel() != x.numel() or (uncond is not None and uncond.numel() != x.numel()):
        raise _lib.LcvError("cfg_lms_step: cond and uncond must have x's size")
    B = x.shape[0]
    n = x.numel() // max(B, 1)
    ws = _cfg_partials(1, B, x.device) if (uncond is not None and zero_star) else None
    w = [float(v) for v in weights] + [0.0] * (3 - terms)
    call("lcv_cfg_lms_step", _ptr(cond.contiguous()), None if uncond is None else _ptr(uncond.contiguous()), _ptr(x), _ptr(f0),
         _ptr(hist[0]) if terms >= 2 else None, _ptr(hist[1]) if terms >= 3 else None, _ptr(ws), B, n, float(guidance),
         w[0], w[1], w[2], terms, 1 if negate else 0, 1 if zero_star else 0, _stream())


# the guidance reuse of the CFG denoise loop (include/lcv_hip_cfgreuse.h; the schedule lives in longcat_video/cfg_reuse.py)
_CFGREUSE_WS = {}    # (device index, B) -> the [2, B, 256, 2] partial sums of lcv_cfg_delta_store (kept alive here)


def cfg_reuse_workspace(B: int, device) -> torch.Tensor:
    """The zero-star partial pairs, then the drift partial pairs: 256 fp32 pairs per sample each, cached per (device, B)."""
    key = (torch.device(device).index, int(B))
    ws = _CFGREUSE_WS.get(key)
    if ws is None:
        ws = _CFGREUSE_WS[key] = _cfg_partials(2, B, device)
    return ws


def _cfgreuse_req(name: str, *tensors) -> None:
    numel = tensors[0].numel()
    for t in tensors:
        _req(t, F32, name)
        if not t.is_contiguous() or t.numel() != numel:
            raise _lib.LcvError(f"{name}: needs contiguous fp32 tensors of one size, got {tuple(t.shape)} against "
                                f"{tuple(tensors[0].shape)}")


def cfg_delta_store(cond: torch.Tensor, uncond: torch.Tensor, delta: torch.Tensor, guidance: float, zero_star: bool = True,
                    out: Optional[torch.Tensor] = None) -> None:
    """delta = v - cond, v the guided output of (cond, uncond) as lcv_cfg_lms_step forms it (before any sign), over [B, ...]
    fp32 tensors; `delta` is written in place.  With `out` ([B, 2] fp32) the old delta is read first and out[b] = (sum |new -
    old|, sum |old|) in a fixed order.  Nothing is synchronised."""
    _cfgreuse_req("cfg_delta_store", cond, uncond, delta)
    B = delta.shape[0]
    n = delta.numel() // max(B, 1)
    if out is not None:
        _req(out, F32, "cfg_delta_store.out")
        if out.numel() != 2 * B or not out.is_contiguous():
            raise _lib.LcvError(f"cfg_delta_store: out needs {2 * B} contiguous fp32 words, got {out.numel()}")
    ws = cfg_reuse_workspace(B, delta.device) if (zero_star or out is not None) else None
    call("lcv_cfg_delta_store", _ptr(cond), _ptr(uncond), _ptr(delta), _ptr(ws), _ptr(out), B, n, float(guidance),
         1 if zero_star else 0, _stream())


def cfg_delta_apply(cond: torch.Tensor, delta: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = cond + delta, a reuse step's guided output; `out` may be cond (default: a new tensor)."""
    if out is None:
        out = torch.empty_like(cond)
    _cfgreuse_req("cfg_delta_apply", cond, delta, out)
    B = cond.shape[0]
    call("lcv_cfg_delta_apply", _ptr(cond), _ptr(delta), _ptr(out), B, cond.numel() // max(B, 1), _stream())
    return out


# the adaptive projected guidance of the CFG denoise loop (include/lcv_hip_apg.h; the settings live in longcat_video/apg.py)
_APG_WS = {}         # (device index, B) -> the [2, B, 256, 4] partial sums of lcv_cfg_apg (kept alive here)


def cfg_apg_workspace(B: int, device) -> torch.Tensor:
    """The zero-star partial pairs (dot, nrm, 0, 0), then the correction's partial sums (dd, dc, cc, 0): 256 per sample each,
    every slot written by the call that reads it, cached per (device, B)."""
    key = (torch.device(device).index, int(B))
    ws = _APG_WS.get(key)
    if ws is None:
        ws = _APG_WS[key] = torch.empty((2, int(B), 256, 4), dtype=F32, device=device)
    return ws


def cfg_apg(cond: torch.Tensor, uncond: torch.Tensor, diff: torch.Tensor, guidance: float, eta: float, radius: Optional[float],
            beta: float, zero_star: bool, have_momentum: bool, out: Optional[torch.Tensor] = None,
            v: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The projected-guidance output of (cond, uncond) over [B, ...] fp32 tensors: diff = (cond - uncond') [+ beta * diff when
    `have_momentum`], written in place, then v = cond + (guidance - 1) ((s diff - p) + eta p) with p the part of s diff along
    cond and s = min(1, radius / ||diff||) (`radius` None or <= 0: no cap).  `v` may be cond (default: a new tensor); with `out`
    ([B, 4] fp32) out[b] = (<d, d>, <d, c>, <c, c>, s) in a fixed order.  Nothing is synchronised."""
    if v is None:
        v = torch.empty_like(cond)
    _cfgreuse_req("cfg_apg", cond, uncond, diff, v)
    B = diff.shape[0]
    n = diff.numel() // max(B, 1)
    if out is not None:
        _req(out, F32, "cfg_apg.out")
        if out.numel() != 4 * B or not out.is_contiguous():
            raise _lib.LcvError(f"cfg_apg: out needs {4 * B} contiguous fp32 words, got {out.numel()}")
    ws = cfg_apg_workspace(B, diff.device)
    call("lcv_cfg_apg", _ptr(cond), _ptr(uncond), _ptr(diff), _ptr(v), _ptr(ws), _ptr(out), B, n, float(guidance), float(eta),
         0.0 if radius is None else float(radius), float(beta), 1 if zero_star else 0, 1 if have_momentum else 0, _stream())
    return v


# the first-block step cache of the denoise loop (include/lcv_hip_stepcache.h; the policy lives in longcat_video/step_cache.py)
_STEPCACHE_CHUNK = 2048
_STEPCACHE_WS = {}   # (device index, rows, n) -> the partial-sum workspace of lcv_stepcache_diff (kept alive here)


def _stepcache_req(name: str, *tensors) -> None:
    shape = tensors[0].shape
    for t in tensors:
        _req(t, BF16, name)
        if not t.is_contiguous() or t.shape != shape:
            raise _lib.LcvError(f"{name}: needs contiguous bf16 tensors of one shape, got {tuple(t.shape)} against {tuple(shape)}")


def stepcache_workspace(rows: int, n: int, device) -> torch.Tensor:
    """One (num, den) fp32 pair per 2048-element chunk of a row, cached per (rows, n)."""
    key = (torch.device(device).index, int(rows), int(n))
    ws = _STEPCACHE_WS.get(key)
    if ws is None:
        chunks = rows * ((n + _STEPCACHE_CHUNK - 1) // _STEPCACHE_CHUNK)
        ws = _STEPCACHE_WS[key] = torch.empty((2 * chunks,), dtype=F32, device=device)
    return ws


def stepcache_diff(x0: torch.Tensor, x1: torch.Tensor, prev: Optional[torch.Tensor], r_out: torch.Tensor, thr: float,
                   out: torch.Tensor) -> None:
    """r_out = bf16(x1 - x0) over [rows, ...] bf16 tensors; with `prev` also out[0:rows] = per-row sum |r - prev|,
    out[rows:2 rows] = per-row sum |prev| (fixed order) and the 32-bit integer out[2 rows] = all(num < thr * den); without it
    out[2 rows] = 0.  `out` is an fp32 device tensor of 2 rows + 1 words.  Nothing is synchronised."""
    _stepcache_req("stepcache_diff", x0, x1, r_out, *(() if prev is None else (prev,)))
    _req(out, F32, "stepcache_diff.out")
    rows = x0.shape[0]
    n = x0.numel() // max(rows, 1)
    if out.numel() != 2 * rows + 1 or not out.is_contiguous():
        raise _lib.LcvError(f"stepcache_diff: out needs {2 * rows + 1} contiguous fp32 words, got {out.numel()}")
    ws = None if prev is None else stepcache_workspace(rows, n, x0.device)
    call("lcv_stepcache_diff", _ptr(x0), _ptr(x1), _ptr(prev), _ptr(r_out), rows, n, float(thr), _ptr(ws),
         0 if ws is None else ws.numel() * 4, _ptr(out), _stream())


def stepcache_store(xL: torch.Tensor, x1: torch.Tensor, R: torch.Tensor) -> None:
    """R = bf16(xL - x1): what the blocks after the first added."""
    _stepcache_req("stepcache_store", xL, x1, R)
    call("lcv_stepcache_store", _ptr(xL), _ptr(x1), _ptr(R), xL.numel(), _stream())


def stepcache_apply(x1: torch.Tensor, R: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out = bf16(x1 + R), a skipped step's stand-in for the last block's output; `out` may be x1 (default: a new tensor)."""
    if out is None:
        out = torch.empty_like(x1)
    _stepcache_req("stepcache_apply", x1, R, out)
    call("lcv_stepcache_apply", _ptr(x1), _ptr(R), _ptr(out), x1.numel(), _stream())
    return out


def fm_noise(x0: torch.Tensor, eps: torch.Tensor, sigma: torch.Tensor) -> torch.Tensor:
    _req(x0, BF16, "fm_noise.x0"); _req(eps, BF16, "fm_noise.eps"); _req(sigma, F32, "fm_noise.sigma")
    B = x0.shape[0]
    out = torch.empty_like(x0)
    call("lcv_fm_noise", _ptr(x0.contiguous()), _ptr(eps.contiguous()), _ptr(sigma), _ptr(out), B,
         x0.numel() // max(B, 1), _stream())
    return out


def fm_mse(pred: torch.Tensor, eps: torch.Tensor, x0: torch.Tensor, Tc: int, need_grad: bool = True):
    _req(pred, F32, "fm_mse.pred"); _req(eps, BF16, "fm_mse.eps"); _req(x0, BF16, "fm_mse.x0")   # the kernel reads raw bf16
    B, C, T, H, W = pred.shape
    if tuple(eps.shape) != (B, C, T - Tc, H, W) or tuple(x0.shape) != tuple(eps.shape):
        raise _lib.LcvError(f"fm_mse: eps {tuple(eps.shape)} / x0 {tuple(x0.shape)} do not match pred {tuple(pred.shape)} "
                            f"with T_cond={Tc}")
    loss = torch.empty((1,), dtype=F32, device=pred.device)
    dpred = torch.empty_like(pred) if need_grad else None
    ws = torch.empty((1024,), dtype=F32, device=pred.device)        # lcv_hip.h: LCV_FM_MSE_BLOCKS per-workgroup partial sums
    call("lcv_fm_mse", _ptr(pred.contiguous()), _ptr(eps.contiguous()), _ptr(x0.contiguous()), _ptr(loss),
         _ptr(dpred), _ptr(ws), B, C, T, Tc, H * W, _stream())
    return loss[0], dpred


def fm_mse_samples(pred: torch.Tensor, eps: torch.Tensor, x0: torch.Tensor, Tc: int) -> torch.Tensor:
    """Per-sample mean((pred[b, :, Tc:] - (eps[b] - x0[b]))^2), fp32 [B], deterministic, no gradient.
    `eps` / `x0` are bf16 [B or 1, C, Tt, H, W]; a leading 1 is shared by every sample without being expanded."""
    _req(pred, F32, "fm_mse_samples.pred"); _req(eps, BF16, "fm_mse_samples.eps"); _req(x0, BF16, "fm_mse_samples.x0")
    B, C, T, H, W = pred.shape
    per = C * (T - Tc) * H * W
    for name, t in (("eps", eps), ("x0", x0)):
        if t.shape[0] not in (1, B) or tuple(t.shape[1:]) != (C, T - Tc, H, W):
            raise _lib.LcvError(f"fm_mse_samples.{name}: shape {tuple(t.shape)} does not match pred {tuple(pred.shape)} with Tc={Tc}")
    eps, x0 = eps.contiguous(), x0.contiguous()
    loss = torch.empty((B,), dtype=F32, device=pred.device)
    ws = torch.empty((B * 256,), dtype=F32, device=pred.device)
    call("lcv_fm_mse_samples", _ptr(pred.contiguous()), _ptr(eps), _ptr(x0), _ptr(loss), _ptr(ws), B, C, T, Tc, H * W,
         per if eps.shape[0] == B and B > 1 else 0, per if x0.shape[0] == B and B > 1 else 0, _stream())
    return loss


# ===================================================================== backward kernels
def _res_grad(dres, like, name):
    """Optional second gradient w.r.t. the norm's input (the residual path of the same block), added inside the kernel."""
    if dres is None:
        return None
    _req(dres, BF16, name)
    if tuple(dres.shape) != tuple(like.shape):
        raise _lib.LcvError(f"{name}: shape {tuple(dres.shape)} does not match x {tuple(like.shape)}")
    return dres.contiguous()


def adaln_modulate_bwd(x, mod, dy, shift_idx, scale_idx, T, eps=1e-6, need_dmod=False, dres=None):
    _req(dy, BF16, "adaln_modulate_bwd.dy")
    B, N, C = x.shape
    dx = torch.empty_like(x)
    dmod = torch.zeros_like(mod) if need_dmod else None
    dres = _res_grad(dres, x, "adaln_modulate_bwd.dres")
    if _DETERMINISTIC and need_dmod:
        ws, nb = _det_ws(_lib.LCV_DET_ADALN, x.device, B * T, N // T, C)
        call("lcv_det_adaln_modulate_bwd", _ptr(x), _ptr(mod), _ptr(dy), _ptr(dx), _ptr(dmod), B, T, N // T, C,
             mod.shape[-1], shift_idx * C, scale_idx * C, eps, _ptr(dres), _ptr(ws), nb, _stream())
        return dx, dmod
    call("lcv_adaln_modulate_bwd", _ptr(x), _ptr(mod), _ptr(dy), _ptr(dx), _ptr(dmod), B, T, N // T, C,
         mod.shape[-1], shift_idx * C, scale_idx * C, eps, _ptr(dres), _stream())
    return dx, dmod


def layernorm_affine_bwd(x, w, dy, eps=1e-6, need_dw=False, dres=None):
    _req(dy, BF16, "layernorm_affine_bwd.dy")
    C = x.shape[-1]
    x = x.contiguous()
    dres = _res_grad(dres, x, "layernorm_affine_bwd.dres")
    wf = w.detach().to(F32).contiguous()
    dx = torch.empty_like(x)
    dw = torch.zeros(C, dtype=F32, device=x.device) if need_dw else None
    db = torch.zeros(C, dtype=F32, device=x.device) if need_dw else None
    if _DETERMINISTIC and need_dw:
        ws, nb = _det_ws(_lib.LCV_DET_LAYERNORM, x.device, x.numel() // C, C)
        call("lcv_det_layernorm_affine_bwd", _ptr(x), _ptr(wf), _ptr(dy), _ptr(dx), _ptr(dw), _ptr(db), x.numel() // C, C,
             eps, _ptr(dres), _ptr(ws), nb, _stream())
        return dx, dw, db
    call("lcv_layernorm_affine_bwd", _ptr(x), _ptr(wf), _ptr(dy), _ptr(dx), _ptr(dw), _ptr(db), x.numel() // C, C,
         eps, _ptr(dres), _stream())
    return dx, dw, db


def gate_residual_bwd(y, mod, dout, gate_idx, T, need_dmod=False):
    _req(dout, BF16, "gate_residual_bwd.dout")
    B, N, C = y.shape
    dy = torch.empty_like(y)
    dmod = torch.zeros_like(mod) if need_dmod else None
    if _DETERMINISTIC and need_dmod:
        ws, nb = _det_ws(_lib.LCV_DET_GATE, y.device, B * T, N // T, C)
        call("lcv_det_gate_residual_bwd", _ptr(y), _ptr(mod), _ptr(dout), _ptr(dy), _ptr(dmod), B, T, N // T, C,
             mod.shape[-1], gate_idx * C, _ptr(ws), nb, _stream())
        return dy, dmod
    call("lcv_gate_residual_bwd", _ptr(y), _ptr(mod), _ptr(dout), _ptr(dy), _ptr(dmod), B, T, N // T, C,
         mod.shape[-1], gate_idx * C, _stream())
    return dy, dmod


DW_SLOTS = 256


def qknorm_rope_bwd(q_in, k_in, dq_out, dk_out, dq_in, dk_in, wq, wk, cs, pos_off=0, eps=1e-6, q_scale=1.0,
                    dwq: Optional[torch.Tensor] = None, dwk: Optional[torch.Tensor] = None):
    """dwq / dwk: optional fp32 [128] accumulators (zeroed by the caller) for the norm-weight gradients."""
    ref = q_in if q_in is not None else k_in
    B, N, H, D = ref.shape
    go = dq_out if dq_out is not None else dk_out
    gk = dk_out if dk_out is not None else dq_out
    gi = dq_in if dq_in is not None else dk_in
    for t in (q_in, k_in, dq_out, dk_out, dq_in, dk_in):
        if t is not None and (t.stride(3) != 1 or t.stride(2) != D):
            raise _lib.LcvError("qknorm_rope_bwd: (H, D) must be contiguous")
    if _DETERMINISTIC and (dwq is not None or dwk is not None):
        # fixed-order form: per-token partials + two ordered sums, added straight into the [128] accumulators
        for t, nme in ((dwq, "dwq"), (dwk, "dwk")):
            if t is not None:
                _req(t, F32, "qknorm_rope_bwd." + nme)
                if t.numel() != D or not t.is_contiguous():
                    raise _lib.LcvError(f"qknorm_rope_bwd.{nme}: contiguous fp32 [{D}] expected")
        ws, nb = _det_ws(_lib.LCV_DET_QKNORM, ref.device, B, N)
        call("lcv_det_qknorm_rope_bwd", _ptr(q_in), _ptr(k_in), _ptr(dq_out), _ptr(dk_out), _ptr(dq_in), _ptr(dk_in),
             _ptr(wq), _ptr(wk), _ptr(cs), B, N, H, ref.stride(0), ref.stride(1), go.stride(0), go.stride(1),
             gk.stride(0), gk.stride(1), gi.stride(0), gi.stride(1), pos_off, eps, q_scale, _ptr(dwq), _ptr(dwk),
             _ptr(ws), nb, _stream())
        return
    # the norm-weight gradients are accumulated into DW_SLOTS rows (token % DW_SLOTS) and added up afterwards: one 128-float
    # target for every token of the call would serialise the kernel on those addresses
    slots = DW_SLOTS if (dwq is not None or dwk is not None) else 1
    sq = torch.zeros((slots, D), dtype=F32, device=ref.device) if dwq is not None else None
    sk = torch.zeros((slots, D), dtype=F32, device=ref.device) if dwk is not None else None
    call("lcv_qknorm_rope_bwd", _ptr(q_in), _ptr(k_in), _ptr(dq_out), _ptr(dk_out), _ptr(dq_in), _ptr(dk_in),
         _ptr(wq), _ptr(wk), _ptr(cs), B, N, H, ref.stride(0), ref.stride(1), go.stride(0), go.stride(1),
         gk.stride(0), gk.stride(1), gi.stride(0), gi.stride(1), pos_off, eps, q_scale, _ptr(sq), _ptr(sk), slots, _stream())
    if dwq is not None:
        dwq.add_(sq.sum(0))
    if dwk is not None:
        dwk.add_(sk.sum(0))


def attention_bwd(q, k, v, o, do, lse, dq, dk, dv, scale, accumulate_kv=False):
    """All [B,N,H,128] views; do must share o's strides; dq/dk/dv written (dk/dv accumulated when asked)."""
    B, Nq, H, D = q.shape
    Nk = k.shape[1]
    if do.stride() != o.stride():
        do = do.contiguous()
        if do.stride() != o.stride():
            raise _lib.LcvError("attention_bwd: dO must share O's strides")
    delta = torch.empty((max(int(_lib.load().lcv_attn_bwd_ws_floats(B, H, Nq, Nk)), 1),), dtype=F32, device=q.device)   # lcv_hip.h: delta_ws
    if PROFILE_BWD is not None:   # bench.py: HIP events on the launch stream around the whole backward of this region
        ev0 = torch.cuda.Event(enable_timing=True); ev1 = torch.cuda.Event(enable_timing=True)
        ev0.record()
    call("lcv_attn_bwd", _ptr(q), _ptr(k), _ptr(v), _ptr(o), _ptr(do), _ptr(lse), _ptr(dq), _ptr(dk), _ptr(dv),
         _ptr(delta), 1 if accumulate_kv else 0, B, H, Nq, Nk,
         q.stride(0), q.stride(1), q.stride(2), k.stride(0), k.stride(1), k.stride(2),
         v.stride(0), v.stride(1), v.stride(2), o.stride(0), o.stride(1), o.stride(2),
         dq.stride(0), dq.stride(1), dq.stride(2), dk.stride(0), dk.stride(1), dk.stride(2),
         dv.stride(0), dv.stride(1), dv.stride(2), float(scale), _stream())
    if PROFILE_BWD is not None:
        ev1.record()
        PROFILE_BWD.append((ev0, ev1, 10.0 * B * H * Nq * Nk * D, Nq, Nk))


def swiglu_bwd(gate, up, dout):
    rows, F = gate.shape
    dg = torch.empty((rows, F), dtype=BF16, device=gate.device)
    du = torch.empty((rows, F), dtype=BF16, device=gate.device)
    call("lcv_swiglu_bwd", _ptr(gate), _ptr(up), _ptr(dout), _ptr(dg), _ptr(du), rows, F, gate.stride(0), _stream())
    return dg, du


def swiglu_bwd_interleaved(gu: torch.Tensor, dout: torch.Tensor) -> torch.Tensor:
    """d[gate | up] (interleaved, [rows, 2F]) from the fused GEMM's saved pre-activations and dh [rows, F]."""
    _req(gu, BF16, "swiglu_bwd_interleaved.gu"); _req(dout, BF16, "swiglu_bwd_interleaved.dout")
    rows, F2 = gu.shape
    if not (gu.is_contiguous() and dout.is_contiguous() and dout.shape == (rows, F2 // 2)):
        raise _lib.LcvError("swiglu_bwd_interleaved: gu [rows, 2F] and dout [rows, F] must be contiguous")
    dgu = torch.empty_like(gu)
    call("lcv_swiglu_bwd_interleaved", _ptr(gu), _ptr(dout), _ptr(dgu), rows, F2 // 2, _stream())
    return dgu


def unpatchify_bwd(dout, Cout, T, H, W):
    _req(dout, F32, "unpatchify_bwd.dout")
    B = dout.shape[0]
    dtok = torch.empty((B, T * (H // 2) * (W // 2), 4 * Cout), dtype=F32, device=dout.device)
    call("lcv_unpatchify_bwd", _ptr(dout), _ptr(dtok), B, Cout, T, H, W, _stream())
    return dtok


def linear_f32_smallm_bwd(dy, w, a, act_in=0):
    _req(dy, F32, "linear_f32_smallm_bwd.dy")
    M, K = a.shape
    N = w.shape[0]
    da = torch.empty((M, K), dtype=F32, device=a.device)
    if _DETERMINISTIC:
        ws, nb = _det_ws(_lib.LCV_DET_SMALLM, a.device, M, N, K)
        call("lcv_det_linear_f32_smallm_bwd", _ptr(dy.contiguous()), _ptr(w.contiguous()), _ptr(a.contiguous()), _ptr(da),
             M, N, K, act_in, _ptr(ws), nb, _stream())
        return da
    call("lcv_linear_f32_smallm_bwd", _ptr(dy.contiguous()), _ptr(w.contiguous()), _ptr(a.contiguous()), _ptr(da),
         M, N, K, act_in, _stream())
    return da


def _tn_skinny(name, g, x, R, scale, draw=()):
    """lcv_tn_skinny (draw empty) or lcv_tn_skinny_dropout (draw = _draw(...)): the output, the workspace and the call."""
    M, K = x.shape
    out = torch.empty((R, K), dtype=F32, device=x.device)
    ws_bytes = int(getattr(_lib.load(), name + "_ws_bytes")(M, K, R))
    ws = torch.empty((max(ws_bytes, 16) // 4,), dtype=F32, device=x.device)     # per-row-group partial sums (caching allocator)
    call(name, _ptr(g), _ptr(x), _ptr(out), M, K, R, g.shape[1], x.stride(0), float(scale), *draw, _ptr(ws), ws_bytes, _stream())
    return out


def tn_skinny(g, x, R, scale=1.0):
    """out[R, K] fp32 = scale * g[:, :R]^T @ x  (g [M, Rpad] bf16, x [M, K] bf16)."""
    _req(g, BF16, "tn_skinny.g"); _req(x, BF16, "tn_skinny.x")
    return _tn_skinny("lcv_tn_skinny", g, x, R, scale)


# ------------------------------------------------------ frame evaluation ---
def gaussian_window11(sigma: float = 1.5):
    """The 11 normalised fp32 taps torchmetrics builds for SSIM (`_gaussian(kernel_size=11, sigma=1.5)`): evaluated
    here in fp32 with the same operation order so the weights are the very same floats."""
    import numpy as np
    dist = np.arange((1 - 11) / 2, (1 + 11) / 2, 1, dtype=np.float32)
    gauss = np.exp(-np.power(dist / np.float32(sigma), 2) / np.float32(2)).astype(np.float32)
    return (gauss / gauss.sum(dtype=np.float32)).astype(np.float32)


def frame_metrics(gen: torch.Tensor, gt: torch.Tensor, data_range: float = 1.0, ssim: Optional[str] = "gaussian11"):
    """gen fp32 [N,H,W,C] in [0,1]; gt fp32 or uint8, same shape.  Returns per-frame (mse fp64 [N], ssim fp64 [N] or None)
    on the host: one launch each, the partial sums added in fp64.  `ssim`: "gaussian11" (torchmetrics defaults),
    "uniform7" (skimage defaults) or None."""
    import ctypes
    import numpy as np
    _req(gen, F32, "frame_metrics.gen")
    if gt.dtype not in (torch.uint8, F32) or not gt.is_cuda:
        raise _lib.LcvError("frame_metrics.gt: fp32 or uint8 GPU tensor expected")
    if gen.shape != gt.shape or gen.dim() != 4:
        raise _lib.LcvError(f"frame_metrics: [N,H,W,C] frames of equal shape expected, got {tuple(gen.shape)} / {tuple(gt.shape)}")
    if ssim not in (None, "gaussian11", "uniform7"):
        raise _lib.LcvError(f"frame_metrics: unknown ssim variant {ssim!r}")
    gen, gt = gen.contiguous(), gt.contiguous()
    N, H, W, C = gen.shape
    win = 7 if ssim == "uniform7" else 11
    if ssim is not None and (H < win or W < win):
        raise _lib.LcvError(f"frame_metrics: a {H}x{W} frame is smaller than the window ({win}x{win})")
    n_sq, n_ss = ctypes.c_int64(0), ctypes.c_int64(0)
    call("lcv_frame_metric_partials", H, W, C, win, ctypes.byref(n_sq), ctypes.byref(n_ss))
    u8 = 1 if gt.dtype == torch.uint8 else 0
    part = torch.empty((N, n_sq.value), dtype=F32, device=gen.device)
    call("lcv_frame_sqerr", _ptr(gen), _ptr(gt), u8, _ptr(part), N, H * W * C, _stream())
    mse = part.double().sum(1).cpu() / float(H * W * C)
    out = None
    if ssim is not None:
        if ssim == "gaussian11":
            taps, cov_norm, clamp = gaussian_window11(), 1.0, 1
        else:
            taps, cov_norm, clamp = np.full(7, 1.0 / 7.0, dtype=np.float32), 49.0 / 48.0, 0
        spart = torch.empty((N, n_ss.value), dtype=F32, device=gen.device)
        call("lcv_frame_ssim", _ptr(gen), _ptr(gt), u8, _ptr(spart), N, H, W, C, taps.ctypes.data, win, cov_norm, clamp,
             (0.01 * data_range) ** 2, (0.03 * data_range) ** 2, _stream())
        out = spart.double().sum(1).cpu() / float((H - win + 1) * (W - win + 1) * C)
    return mse, out


# ------------------------------------------------------------ LPIPS (alex) ---
# AlexNet `features` as LPIPS taps it (spec/lpips.md §L): (Cin, Cout, kernel, stride, pad, 3/2 max-pool in front)
LPIPS_ALEX_LAYERS = ((3, 64, 11, 4, 2, False), (64, 192, 5, 1, 2, True), (192, 384, 3, 1, 1, True),
                     (384, 256, 3, 1, 1, False), (256, 256, 3, 1, 1, False))
LPIPS_SHIFT = (-0.030, -0.088, -0.188)
LPIPS_SCALE = (0.458, 0.448, 0.450)
LPIPS_MIN_SIDE = 31        # below it the second pool has no window
LPIPS_CHUNK = 8            # frame pairs per pass: bounds the workspace (0.30 GB at 480x832, 0.71 GB at 720x1280)
_LPIPS_WS = {}


class LpipsWeights:
    """Device-resident weights of LPIPS-alex in the layout the kernels read: `conv[i] = (packed [Cout, Kpad], bias
    [Cout])`, `lin[i] = [C_i]`, and the scaling layer's six constants (host floats)."""

    def __init__(self, conv, lin, shift=LPIPS_SHIFT, scale=LPIPS_SCALE):
        import numpy as np
        self.conv, self.lin = list(conv), list(lin)
        self.shift_scale = np.asarray(tuple(shift) + tuple(scale), dtype=np.float32)
        if len(self.conv) != 5 or len(self.lin) != 5 or self.shift_scale.shape != (6,):
            raise _lib.LcvError("LpipsWeights: five convolutions, five lin vectors, three shifts and three scales expected")
        for i, ((cin, cout, k, _, _, _), (w, b), l) in enumerate(zip(LPIPS_ALEX_LAYERS, self.conv, self.lin)):
            kpad = (k * k * cin + 31) // 32 * 32
            for t, shape, what in ((w, (cout, kpad), "packed weight"), (b, (cout,), "bias"), (l, (cout,), "lin weight")):
                _req(t, F32, f"LpipsWeights layer {i} {what}")
                if tuple(t.shape) != shape or not t.is_contiguous():
                    raise _lib.LcvError(f"LpipsWeights layer {i} {what}: contiguous {shape} expected, got {tuple(t.shape)}")


def lpips_pack_weight(w: torch.Tensor) -> torch.Tensor:
    """fp32 [Cout, Cin, KH, KW] -> fp32 [Cout, Kpad], k = (kh, kw, ci) with ci fastest, zero-padded to a multiple of 32."""
    _req(w, F32, "lpips_pack_weight.w")
    if w.dim() != 4:
        raise _lib.LcvError(f"lpips_pack_weight: [Cout,Cin,KH,KW] expected, got {tuple(w.shape)}")
    cout, cin, kh, kw = w.shape
    kpad = (kh * kw * cin + 31) // 32 * 32
    out = torch.empty((cout, kpad), dtype=F32, device=w.device)
    call("lcv_lpips_pack_weight", _ptr(w.contiguous()), _ptr(out), cout, cin, kh, kw, kpad, _stream())
    return out


def lpips_conv_relu(x: torch.Tensor, packed: torch.Tensor, bias: torch.Tensor, k: int, stride: int, pad: int,
                    out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """relu(conv2d(x) + bias) of a channels-last fp32 [B,h,w,Cin] map with a packed weight -> [B,ho,wo,Cout]."""
    _req(x, F32, "lpips_conv_relu.x"); _req(packed, F32, "lpips_conv_relu.packed"); _req(bias, F32, "lpips_conv_relu.bias")
    B, h, w, cin = x.shape
    cout, kpad = packed.shape
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    if out is None:
        out = torch.empty((B, max(ho, 0), max(wo, 0), cout), dtype=F32, device=x.device)
    call("lcv_lpips_conv_relu", _ptr(x.contiguous()), None, 0, 0, None, _ptr(packed), _ptr(bias), _ptr(out), B, h, w, cin, cout,
         k, k, stride, pad, kpad, _stream())
    return out


def lpips_conv1_relu(gen: torch.Tensor, gt: torch.Tensor, weights: LpipsWeights, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The first layer on the frames themselves: [N,H,W,3] fp32 generated + fp32 / uint8 ground truth -> tap 1
    [2N,h1,w1,64]; 2x - 1 and the scaling layer happen in the loader."""
    N, H, W, _ = gen.shape
    cin, cout, k, stride, pad, _ = LPIPS_ALEX_LAYERS[0]
    packed, bias = weights.conv[0]
    h1, w1 = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    if out is None:
        out = torch.empty((2 * N, h1, w1, cout), dtype=F32, device=gen.device)
    call("lcv_lpips_conv_relu", _ptr(gen), _ptr(gt), 1, 1 if gt.dtype == torch.uint8 else 0, weights.shift_scale.ctypes.data,
         _ptr(packed), _ptr(bias), _ptr(out), 2 * N, H, W, cin, cout, k, k, stride, pad, packed.shape[1], _stream())
    return out


def lpips_maxpool(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """MaxPool2d(3, 2), floor mode, of a channels-last fp32 [B,h,w,C] map."""
    _req(x, F32, "lpips_maxpool.x")
    B, h, w, C = x.shape
    if out is None:
        out = torch.empty((B, max((h - 3) // 2 + 1, 0), max((w - 3) // 2 + 1, 0), C), dtype=F32, device=x.device)
    call("lcv_lpips_maxpool", _ptr(x.contiguous()), _ptr(out), B, h, w, C, _stream())
    return out


def lpips_tap_distance(feats: torch.Tensor, lin: torch.Tensor, out: Optional[torch.Tensor] = None, accumulate: bool = False,
                       partials: Optional[torch.Tensor] = None) -> torch.Tensor:
    """feats fp32 [2N,h,w,C] (generated half first), lin fp32 [C] -> out[n] (+)= the tap's mean distance of pair n."""
    _req(feats, F32, "lpips_tap_distance.feats"); _req(lin, F32, "lpips_tap_distance.lin")
    B, h, w, C = feats.shape
    if B % 2 or lin.numel() != C:
        raise _lib.LcvError(f"lpips_tap_distance: 2N images and {C} lin weights expected, got {B} / {lin.numel()}")
    N = B // 2
    if out is None:
        out = torch.zeros(N, dtype=F32, device=feats.device)
    if partials is None:
        partials = torch.empty(N * _lib.LCV_LPIPS_TAP_BLOCKS, dtype=F32, device=feats.device)
    call("lcv_lpips_tap_distance", _ptr(feats.contiguous()), _ptr(lin.contiguous()), _ptr(partials), _ptr(out), 1 if accumulate else 0,
         N, h * w, C, _stream())
    return out


def _lpips_workspace(n: int, H: int, W: int, device):
    """The regions `lcv_lpips_ws_bytes` sizes for n pairs, carved from one flat allocation that is kept per frame size
    (a sweep scores one resolution; a shorter last pass reuses the front of the same buffer)."""
    key = (H, W, str(device))
    total = _lib.load().lcv_lpips_ws_bytes(n, H, W)
    held = _LPIPS_WS.get(key)
    if held is None or held.numel() * 4 < total:
        _LPIPS_WS.clear()
        held = _LPIPS_WS[key] = torch.empty(total // 4, dtype=F32, device=device)
    shapes, (h, w) = [], (H, W)
    for cin, cout, k, stride, pad, pool in LPIPS_ALEX_LAYERS:
        if pool:
            h, w = (h - 3) // 2 + 1, (w - 3) // 2 + 1
            shapes.append((2 * n, h, w, cin))
        h, w = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
        shapes.append((2 * n, h, w, cout))
    shapes.append((n * _lib.LCV_LPIPS_TAP_BLOCKS,))
    views, at = [], 0
    for s in shapes:
        count = 1
        for d in s:
            count *= d
        views.append(held[at:at + count].view(s))
        at += (count + 63) // 64 * 64
    if at * 4 != total:
        raise _lib.LcvError(f"lpips workspace: carved {at * 4} bytes, the library sizes {total}")
    return views


def lpips_alex(gen: torch.Tensor, gt: torch.Tensor, packed_weights: LpipsWeights) -> torch.Tensor:
    """LPIPS v0.1 (AlexNet) of each frame pair: gen fp32 [N,H,W,3] in [0,1], gt fp32 or uint8 of the same shape ->
    fp32 [N] on the device.  Five MFMA convolutions, two pools and five tap distances per pass of up to LPIPS_CHUNK
    pairs; deterministic (no atomics), and a pair's value does not depend on which other pairs share the call."""
    _req(gen, F32, "lpips_alex.gen")
    if gt.dtype not in (torch.uint8, F32) or not gt.is_cuda:
        raise _lib.LcvError("lpips_alex.gt: fp32 or uint8 GPU tensor expected")
    if gen.shape != gt.shape or gen.dim() != 4 or gen.shape[-1] != 3:
        raise _lib.LcvError(f"lpips_alex: [N,H,W,3] frames of equal shape expected, got {tuple(gen.shape)} / {tuple(gt.shape)}")
    if not isinstance(packed_weights, LpipsWeights):
        raise _lib.LcvError("lpips_alex: packed_weights must be an ops.LpipsWeights (tta.lpips.LpipsAlex builds one)")
    N, H, W, _ = gen.shape
    if H < LPIPS_MIN_SIDE or W < LPIPS_MIN_SIDE:
        raise _lib.LcvError(f"lpips_alex: a {H}x{W} frame is smaller than {LPIPS_MIN_SIDE}x{LPIPS_MIN_SIDE} "
                            "(the second max-pool would have no window)")
    gen, gt = gen.contiguous(), gt.contiguous()
    out = torch.empty(N, dtype=F32, device=gen.device)
    for lo in range(0, N, LPIPS_CHUNK):
        n = min(LPIPS_CHUNK, N - lo)
        t1, p1, t2, p2, t3, t4, t5, partials = _lpips_workspace(n, H, W, gen.device)
        o = out[lo:lo + n]
        conv = packed_weights.conv
        lpips_conv1_relu(gen[lo:lo + n], gt[lo:lo + n], packed_weights, out=t1)
        lpips_tap_distance(t1, packed_weights.lin[0], out=o, accumulate=False, partials=partials)
        x = t1
        for i, (tap, pooled) in enumerate(((t2, p1), (t3, p2), (t4, None), (t5, None)), start=1):
            _, _, k, stride, pad, _ = LPIPS_ALEX_LAYERS[i]
            if pooled is not None:
                x = lpips_maxpool(x, out=pooled)
            x = lpips_conv_relu(x, conv[i][0], conv[i][1], k, stride, pad, out=tap)
            lpips_tap_distance(x, packed_weights.lin[i], out=o, accumulate=True, partials=partials)
    return out


# ------------------------------------------------------- UMT5 text encoder ---
def gather_rows(table: torch.Tensor, ids: torch.Tensor) -> torch.Tensor:
    _req(table, BF16, "gather_rows.table")
    if ids.dtype != torch.int64 or not ids.is_cuda:
        raise _lib.LcvError("gather_rows.ids: int64 GPU tensor expected")
    ids = ids.contiguous().view(-1)
    V, C = table.shape
    out = torch.empty((ids.numel(), C), dtype=BF16, device=table.device)
    call("lcv_gather_rows", _ptr(table.contiguous()), _ptr(ids), _ptr(out), ids.numel(), C, V, _stream())
    return out


def t5_rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float = 1e-6) -> torch.Tensor:
    _req(x, BF16, "t5_rmsnorm.x"); _req(w, BF16, "t5_rmsnorm.w")
    x = x.contiguous()
    y = torch.empty_like(x)
    C = x.shape[-1]
    call("lcv_t5_rmsnorm", _ptr(x), _ptr(w.contiguous()), _ptr(y), x.numel() // C, C, eps, _stream())
    return y


def geglu_tanh(gate: torch.Tensor, up: torch.Tensor) -> torch.Tensor:
    _req(gate, BF16, "geglu_tanh.gate"); _req(up, BF16, "geglu_tanh.up")
    rows, F = gate.shape
    if gate.stride(0) != up.stride(0) or gate.stride(1) != 1 or up.stride(1) != 1:
        raise _lib.LcvError("geglu_tanh: gate/up must share the row stride")
    out = torch.empty((rows, F), dtype=BF16, device=gate.device)
    call("lcv_geglu_tanh_fwd", _ptr(gate), _ptr(up), _ptr(out), rows, F, gate.stride(0), _stream())
    return out


def t5_attention(qkv: torch.Tensor, H: int, bias_by_dist: torch.Tensor, key_mask: torch.Tensor) -> torch.Tensor:
    """qkv bf16 [B, S, 3*H*64] (q | k | v column blocks); bias_by_dist fp32 [H, 2S-1]; key_mask int32 [B, S].
    Returns [B, S, H*64] bf16."""
    _req(qkv, BF16, "t5_attention.qkv"); _req(bias_by_dist, F32, "t5_attention.bias")
    B, S, W3 = qkv.shape
    inner = H * 64
    if W3 != 3 * inner or qkv.stride(2) != 1:
        raise _lib.LcvError(f"t5_attention: qkv last dim {W3} != 3*{H}*64")
    if tuple(bias_by_dist.shape) != (H, 2 * S - 1) or key_mask.dtype != torch.int32 or tuple(key_mask.shape) != (B, S):
        raise _lib.LcvError("t5_attention: bias_by_dist [H, 2S-1] fp32 and key_mask [B, S] int32 expected")
    out = torch.empty((B, S, inner), dtype=BF16, device=qkv.device)
    base = qkv.data_ptr()
    call("lcv_t5_attention", base, base + inner * 2, base + 2 * inner * 2, _ptr(out), _ptr(bias_by_dist.contiguous()),
         _ptr(key_mask.contiguous()), B, S, H, qkv.stride(1), inner, qkv.stride(0), S * inner, _stream())
    return out


# ------------------------------------------------ full-model TTA (dense backward) ---
def transpose_pad(x: torch.Tensor) -> torch.Tensor:
    """bf16 [M, N] (contiguous rows) -> [N, Mpad] with Mpad = M rounded up to 64, pad columns zero."""
    _req(x, BF16, "transpose_pad.x")
    if x.dim() != 2 or x.stride(1) != 1:
        raise _lib.LcvError("transpose_pad: 2-D tensor with contiguous rows expected")
    M, N = x.shape
    Mpad = (M + 63) // 64 * 64
    out = torch.empty((N, Mpad), dtype=BF16, device=x.device)
    call("lcv_transpose_pad", _ptr(x), _ptr(out), M, N, x.stride(0), Mpad, _stream())
    return out


def rowsum(xT: torch.Tensor, dtype=BF16) -> torch.Tensor:
    _req(xT, BF16, "rowsum.x")
    xT = xT.contiguous()
    out = torch.empty((xT.shape[0],), dtype=dtype, device=xT.device)
    call("lcv_rowsum", _ptr(xT), _ptr(out), xT.shape[0], xT.shape[1], 1 if dtype == F32 else 0, _stream())
    return out


def dense_wgrad(dyT: torch.Tensor, xT: torch.Tensor) -> torch.Tensor:
    """dW [N, K] = dY^T . X from the two transposed, token-padded operands: one NT GEMM over the token axis."""
    return gemm_nt(dyT, xT, None)


def linear_f32_smallm_wgrad(dy: torch.Tensor, a: torch.Tensor, act_in: int, want_db: bool):
    _req(dy, F32, "linear_f32_smallm_wgrad.dy"); _req(a, F32, "linear_f32_smallm_wgrad.a")
    dy, a = dy.contiguous(), a.contiguous()
    M, N = dy.shape
    K = a.shape[1]
    dw = torch.empty((N, K), dtype=BF16, device=dy.device)
    db = torch.empty((N,), dtype=BF16, device=dy.device) if want_db else None
    call("lcv_linear_f32_smallm_wgrad", _ptr(dy), _ptr(a), _ptr(dw), _ptr(db), M, N, K, act_in, _stream())
    return dw, db


def gelu_tanh(x: torch.Tensor) -> torch.Tensor:
    _req(x, BF16, "gelu_tanh.x")
    x = x.contiguous()
    y = torch.empty_like(x)
    call("lcv_gelu_tanh_fwd", _ptr(x), _ptr(y), x.numel(), _stream())
    return y


def gelu_tanh_bwd(x: torch.Tensor, dy: torch.Tensor) -> torch.Tensor:
    _req(x, BF16, "gelu_tanh_bwd.x"); _req(dy, BF16, "gelu_tanh_bwd.dy")
    x, dy = x.contiguous(), dy.contiguous()
    dx = torch.empty_like(x)
    call("lcv_gelu_tanh_bwd", _ptr(x), _ptr(dy), _ptr(dx), x.numel(), _stream())
    return dx


def __getattr__(name):
    """`ops.FusedAdamWClip`, `ops.FusedSGDClip` and `ops.ema_beta`: the optimizers live in optim.py, which imports this
    module, so the three names are looked up there on first use instead of at import (either module may be imported first)."""
    if name in ("FusedAdamWClip", "FusedSGDClip", "ema_beta"):
        from . import optim
        return getattr(optim, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")

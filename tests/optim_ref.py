"""numpy restatement of the default optimizer kernels (csrc/optim.hip: lcv_adamw_step, lcv_sgd_step and the coefficient of
lcv_grad_norm_clip), in np.float32 and in the kernels' op order: every operation rounded to nearest, nothing fused, and in the
bf16 forms one rounding to bf16 (nearest even) after each operation that the header of optim.hip lists.  A helper, not a test
module."""
import numpy as np

import master_weights_ref as W
from sr_ref import CHUNK, first_chunks  # noqa: F401  (re-exported: the descriptor table's chunking)

F = np.float32


def bf(x):
    """Round fp32 values to bf16 (nearest even) and widen again: the kernels' bfround.  NaN stays NaN, as the hardware convert
    keeps it (to_bf16_bits is for finite values: its carry would turn a NaN with a full mantissa into a zero)."""
    x = np.asarray(x, dtype=F)
    out = W.bf16_to_f32(W.to_bf16_bits(x))
    nan = np.isnan(x)
    return np.where(nan, F(np.nan), out).astype(F) if nan.any() else out


def bf_bits(x):
    """fp32 -> the uint16 the kernel stores.  A NaN is stored as some NaN; the tests compare NaN-ness there, not the payload."""
    x = np.asarray(x, dtype=F)
    h = W.to_bf16_bits(x)
    nan = np.isnan(x)
    return np.where(nan, np.uint16(0x7FC0), h).astype(np.uint16) if nan.any() else h


# ---------------------------------------------------------------------------------------------------------- the clip
def clip_coef(total, max_norm, f32):
    """out[1] of lcv_grad_norm_clip from out[0] (the total norm as stored: already a bf16 value in the bf16 form)."""
    total, max_norm = F(total), F(max_norm)
    if f32:
        coef = max_norm / (total + F(1e-6))
    else:
        coef = bf(max_norm / bf(np.array([total + F(1e-6)], dtype=F)))[0]
    return min(F(coef), F(1.0))


# ---------------------------------------------------------------------------------------------------------- AdamW
def adamw_step_bf16(p, m, v, g, coef, lr, b1, b2, eps, wd, step):
    """adamw_kernel<false> on uint16 patterns; (p, m, v) uint16 out.  Nine bf16 roundings: g, p (decay), m, v twice, d three
    times, p."""
    s = W.adamw_scalars(lr, b1, b2, eps, wd, step)
    g = bf(W.bf16_to_f32(g) * F(coef))
    p = bf(W.bf16_to_f32(p) * s["c_wd"])
    m = W.bf16_to_f32(m)
    m = bf(m + s["w1"] * (g - m))
    v = bf(W.bf16_to_f32(v) * s["b2"])
    v = bf(v + (s["c2"] * g) * g)
    d = bf(np.sqrt(v))
    d = bf(d / s["bc2_sqrt"])
    d = bf(d + s["eps"])
    p = bf(p + s["step_size"] * (m / d))
    return bf_bits(p), bf_bits(m), bf_bits(v)


def adamw_step_f32(p, m, v, g, coef, lr, b1, b2, eps, wd, step):
    """adamw_kernel<true> on fp32 arrays: master_weights_ref.adamw_step's sequence on an fp32 gradient; (p, m, v) fp32 out."""
    s = W.adamw_scalars(lr, b1, b2, eps, wd, step)
    g = np.asarray(g, dtype=F) * F(coef)
    p = np.asarray(p, dtype=F) * s["c_wd"]
    m = np.asarray(m, dtype=F)
    m = m + s["w1"] * (g - m)
    v = np.asarray(v, dtype=F) * s["b2"]
    v = v + (s["c2"] * g) * g
    d = np.sqrt(v) / s["bc2_sqrt"] + s["eps"]
    p = p + s["step_size"] * (m / d)
    return p.astype(F), m.astype(F), v.astype(F)


# ---------------------------------------------------------------------------------------------------------- SGD
def sgd_step_bf16(p, g, coef, lr, wd):
    """sgd_kernel<false> on uint16 patterns (packet path and element path are this one sequence); uint16 out."""
    lr32, wd32 = F(lr), F(wd)
    p = W.bf16_to_f32(p)
    g = bf(W.bf16_to_f32(g) * F(coef))
    if wd32 != 0:
        g = bf(g + wd32 * p)
    return bf_bits(p + (-lr32) * g)


def sgd_step_f32(p, g, coef, lr, wd):
    """sgd_kernel<true> on fp32 arrays: no roundings to bf16, and the decay always added (wd = 0 adds a zero)."""
    lr32, wd32 = F(lr), F(wd)
    p = np.asarray(p, dtype=F)
    g = np.asarray(g, dtype=F) * F(coef)
    g = g + wd32 * p
    return (p + (-lr32) * g).astype(F)

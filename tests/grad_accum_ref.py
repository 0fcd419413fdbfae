"""numpy restatement of include/lcv_hip_accum.h: the fp32 accumulation of bf16 micro-gradients and the two master-weight steps
fed an fp32 gradient, in np.float32 and in the header's op order (every operation rounded to nearest, nothing fused).  Format,
scalars and input generators are those of tests/master_weights_ref.py."""
import numpy as np

import master_weights_ref as W

F = np.float32


def accumulate(acc, grad_bits, scale):
    """t = float(g) * s; a = a + t, with s = fp32(scale): two operations, and always the add."""
    s = F(scale)
    t = W.bf16_to_f32(grad_bits) * s
    return (np.asarray(acc, dtype=F) + t).astype(F)


def sgd_step_g32(h, low, grad, coef, lr, wd):
    """master_weights_ref.sgd_step with an fp32 gradient: g = grad * coef, the rest is that step's op sequence."""
    lr32, wd32, coef = F(lr), F(wd), F(coef)
    w = W.master(h, low)
    g = np.asarray(grad, dtype=F) * coef
    if wd32 != 0:
        g = g + wd32 * w
    w = w + (-lr32) * g
    return W.split(W.bits(w))


def adamw_step_g32(h, low, m, v, grad, coef, lr, beta1, beta2, eps, wd, step):
    """master_weights_ref.adamw_step with an fp32 gradient (fp32 moments); returns (h, l, m, v)."""
    s = W.adamw_scalars(lr, beta1, beta2, eps, wd, step)
    g = np.asarray(grad, dtype=F) * F(coef)
    p = W.master(h, low) * s["c_wd"]
    m = np.asarray(m, dtype=F)
    m = m + s["w1"] * (g - m)
    v = np.asarray(v, dtype=F) * s["b2"]
    v = v + (s["c2"] * g) * g
    d = np.sqrt(v) / s["bc2_sqrt"] + s["eps"]
    p = p + s["step_size"] * (m / d)
    hh, ll = W.split(W.bits(p))
    return hh, ll, m.astype(F), v.astype(F)

"""numpy restatement of include/lcv_hip_anchor.h: the master-weight steps with the decay taken on w - w0, where w0 = float(h0) is
the element's bf16 base word, and the drift |theta - theta0|, in np.float32 and in the header's op order (every operation
rounded to nearest, nothing fused).  Format, scalars and input generators are those of tests/master_weights_ref.py; the fp32
gradient of tests/grad_accum_ref.py and the codec of tests/moments8_ref.py are used as they stand."""
import numpy as np

import master_weights_ref as W
import moments8_ref as M8

F = np.float32


def _grad(grad, grad_f32):
    """The gradient as fp32: bf16 bit patterns widened, or an fp32 array (an accumulator of grad_accum_ref.accumulate)."""
    return np.asarray(grad, dtype=F) if grad_f32 else W.bf16_to_f32(grad)


def sgd_step_anchor(h, low, h0, grad, coef, lr, wd, grad_f32=False):
    """w = join(h, l); g = grad * coef; if wd != 0: d = w - w0; t = wd * d; g = g + t; u = (-lr) * g; w = w + u; split(w)."""
    lr32, wd32, coef = F(lr), F(wd), F(coef)
    w = W.master(h, low)
    g = _grad(grad, grad_f32) * coef
    if wd32 != 0:
        d = w - W.bf16_to_f32(h0)
        t = wd32 * d
        g = g + t
    u = (-lr32) * g
    w = w + u
    return W.split(W.bits(w))


def adamw_step_anchor(h, low, h0, m, v, grad, coef, lr, beta1, beta2, eps, wd, step, grad_f32=False):
    """master_weights_ref.adamw_step with d = p - w0; t = a * d; p = p - t, a = fp32(lr * wd) formed in double, in place of
    p = p * c_wd; returns (h, l, m, v)."""
    s = W.adamw_scalars(lr, beta1, beta2, eps, wd, step)
    a = F(float(lr) * float(wd))
    g = _grad(grad, grad_f32) * F(coef)
    p = W.master(h, low)
    d = p - W.bf16_to_f32(h0)
    t = a * d
    p = p - t
    m = np.asarray(m, dtype=F)
    m = m + s["w1"] * (g - m)
    v = np.asarray(v, dtype=F) * s["b2"]
    v = v + (s["c2"] * g) * g
    den = np.sqrt(v) / s["bc2_sqrt"] + s["eps"]
    p = p + s["step_size"] * (m / den)
    hh, ll = W.split(W.bits(p))
    return hh, ll, m.astype(F), v.astype(F)


def adamw8_step_anchor(h, low, h0, cm, cr, scales, grad_bits, coef, lr, beta1, beta2, eps, wd, step):
    """moments8_ref.adamw8_step with the anchor's decay: decode, adamw_step_anchor, split, encode; returns
    (h, l, cm, cr, scales)."""
    m0, v0 = M8.decode(cm, cr, scales)
    hh, ll, m, v = adamw_step_anchor(h, low, h0, m0, v0, grad_bits, coef, lr, beta1, beta2, eps, wd, step)
    cm, cr, scales = M8.encode(m, v)
    return hh, ll, cm, cr, scales


def drift_sumsq(tensors):
    """sum over (h, low, h0) triples of (join(h, l) - float(h0))^2 in float64 (low None: all low words zero); every term is
    exact in float64, the sum is rounded per addition at 2^-53."""
    total = np.float64(0.0)
    for h, low, h0 in tensors:
        low = np.zeros(np.shape(h), dtype=np.int16) if low is None else low
        d = W.master(h, low).astype(np.float64) - W.bf16_to_f32(h0).astype(np.float64)
        total += np.sum(d * d, dtype=np.float64)
    return float(total)


# ---------------------------------------------------------------------------------------------------------- inputs
def anchors(rng, h, low):
    """Base words bf16(w * (1 + delta)), |delta| log-uniform in [2^-12, 2^-4].  Every 5th element is made a fixed point of
    the pull in place: h0 = h and l = 0, so d = 0 occurs.  Returns (h0, low) - `low` is a modified copy."""
    h = np.asarray(h, dtype=np.uint16)
    low = np.array(low, dtype=np.int16, copy=True)
    w = W.master(h, low)
    delta = W.log_uniform(rng, w.size, -12.0, -4.0).reshape(w.shape)
    h0 = W.to_bf16_bits((w.astype(np.float64) * (1.0 + delta.astype(np.float64))).astype(F))
    flat0, flatl, flath = h0.reshape(-1), low.reshape(-1), h.reshape(-1)
    flat0[::5] = flath[::5]
    flatl[::5] = 0
    return h0, low

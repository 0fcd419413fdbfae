"""numpy restatement of include/lcv_hip_moments8.h: the 8-bit block-scaled AdamW moments (one byte per moment per element, one
fp32 scale per moment per 512 elements, the second moment kept as its root) and the AdamW step on them, in np.float32 and in the
header's op order.  Join, split, the scalars and the fp32 op sequence come from master_weights_ref.py, and so do the input
helpers that keep every intermediate a normal fp32 number."""
import numpy as np

import master_weights_ref as W

F = W.F
BLOCK = 512
R_BIAS, M_BIAS = 761, 889          # code c of r is the float ((c + 761) << 20), magnitude c of m is ((c + 889) << 20)
R_ONE, M_ONE = 255, 127            # the codes of 1.0
R_FLOOR = F(1.25 * 2.0 ** -32)     # r code 1
M_FLOOR = F(1.25 * 2.0 ** -16)     # m magnitude 1


def nblocks(n):
    return (int(n) + BLOCK - 1) // BLOCK


def _k(z):
    """(bits(z) + 0x80000) >> 20: z rounded to 3 mantissa bits, ties away from zero, the carry runs into the exponent."""
    return ((W.bits(z).astype(np.int64) + 0x80000) >> 20)


def _block_max(a):
    """max over each block's valid elements of a non-negative 1-D array."""
    n = a.size
    pad = np.zeros(nblocks(n) * BLOCK, dtype=F)
    pad[:n] = a
    return pad.reshape(-1, BLOCK).max(axis=1)


def _per_element(s, n):
    return np.repeat(np.asarray(s, dtype=F), BLOCK)[:n]


def _ratio(a, s):
    """a / s, one correctly rounded division; 0 where the scale is 0."""
    out = np.zeros(a.shape, dtype=F)
    np.divide(a, s, out=out, where=s != 0)
    return out


def encode_scaled(m, r, sm, sr):
    """Codes of (m, r = sqrt(v)) under given per-block scales -> (cm uint8, cr uint8)."""
    m = np.ascontiguousarray(m, dtype=F).ravel()
    r = np.ascontiguousarray(r, dtype=F).ravel()
    n = m.size
    x = _ratio(np.abs(m), _per_element(sm, n))
    y = _ratio(r, _per_element(sr, n))
    kx, ky = _k(x), _k(y)
    cr = np.where(y == 0, 0, np.clip(ky - R_BIAS, 1, R_ONE))
    mag = np.where((x == 0) | (kx < M_BIAS + 1), 0, np.minimum(kx - M_BIAS, M_ONE))
    sign = (W.bits(m) >> 31).astype(np.int64)
    cm = np.where(mag == 0, 0, mag | (sign << 7))
    return cm.astype(np.uint8), cr.astype(np.uint8)


def encode(m, v):
    """fp32 moments of one tensor -> (cm uint8 [n], cr uint8 [n], scales fp32 [2, nblocks]: the sm row, then the sr row)."""
    m = np.ascontiguousarray(m, dtype=F).ravel()
    r = np.sqrt(np.ascontiguousarray(v, dtype=F).ravel())
    sm, sr = _block_max(np.abs(m)), _block_max(r)
    cm, cr = encode_scaled(m, r, sm, sr)
    return cm, cr, np.stack([sm, sr]).astype(F)


def decode(cm, cr, scales):
    """(cm, cr, scales) -> fp32 (m, v)."""
    cm = np.asarray(cm, dtype=np.uint8).ravel().astype(np.uint32)
    cr = np.asarray(cr, dtype=np.uint8).ravel().astype(np.uint32)
    n = cm.size
    scales = np.asarray(scales, dtype=F).reshape(2, -1)
    mag = cm & 127
    x = np.where(mag != 0, W.floats((mag + M_BIAS) << 20), F(0))
    y = np.where(cr != 0, W.floats((cr + R_BIAS) << 20), F(0))
    a = x.astype(F) * _per_element(scales[0], n)
    m = np.where((cm & 128) != 0, -a, a).astype(F)
    r = y.astype(F) * _per_element(scales[1], n)
    return m, (r * r).astype(F)


def zero_state(n):
    return np.zeros(n, dtype=np.uint8), np.zeros(n, dtype=np.uint8), np.zeros((2, nblocks(n)), dtype=F)


def adamw8_step(h, low, cm, cr, scales, grad_bits, coef, lr, beta1, beta2, eps, wd, step):
    """decode, the fp32 op sequence of master_weights_ref.adamw_step, split, encode; returns (h, l, cm, cr, scales).  The
    parameter update uses the fp32 new moments before they are quantised."""
    m0, v0 = decode(cm, cr, scales)
    hh, ll, m, v = W.adamw_step(h, low, m0, v0, grad_bits, coef, lr, beta1, beta2, eps, wd, step)
    cm, cr, scales = encode(m, v)
    return hh, ll, cm, cr, scales


# ---------------------------------------------------------------------------------------------------------- inputs
def moments(rng, n, lo_exp=-12.0, hi_exp=0.0):
    """fp32 (m, v): m = +-2^u, sqrt(v) = 2^u', u and u' uniform in [lo_exp, hi_exp] - inside both formats' ranges."""
    m = W.log_uniform(rng, n, lo_exp, hi_exp)
    r = np.abs(W.log_uniform(rng, n, lo_exp, hi_exp))
    return m, (r * r).astype(F)

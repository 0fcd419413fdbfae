"""numpy restatement of include/lcv_hip_sr.h: the stochastic rounding of an fp32 bit pattern to bf16, the random bits (group
and stream rule over a descriptor table and over a single array), and the SGD and AdamW steps, in np.float32 and in the
header's op order (every operation rounded to nearest, nothing fused).  A helper, not a test module."""
import numpy as np

import master_weights_ref as W
from lora_dropout_ref import LO, S32, philox4x32_10

F = np.float32
CHUNK = 2048                     # elements per workgroup: 256 threads x 8


# -------------------------------------------------------------------------------------------------------- the rounding
def sr(u, r):
    """uint32 fp32 patterns `u`, 16-bit random values `r` -> uint16 bf16 patterns.  Exponent field not all ones:
    (u + r) >> 16.  All ones: u >> 16, with the quiet bit set when u is a NaN (what round-to-nearest-even stores)."""
    u = np.asarray(u, dtype=np.uint32)
    r = np.asarray(r).astype(np.uint32)
    assert int(r.max(initial=0)) <= 0xFFFF
    # uint32 throughout, as on the device; `u` and `r` may broadcast against each other, and what depends on `u` alone stays
    # in u's shape.  (For an all-ones exponent the sum may wrap: that lane is replaced below.)
    h = ((u + r) >> np.uint32(16)).astype(np.uint16)
    non_finite = (u & np.uint32(0x7F800000)) == np.uint32(0x7F800000)
    if not non_finite.any():
        return h
    top = (u >> np.uint32(16)).astype(np.uint16)
    special = np.where((u & np.uint32(0x007FFFFF)) != 0, top | np.uint16(0x0040), top)
    return np.where(non_finite, special, h)


# -------------------------------------------------------------------------------------------------------- the random bits
def halves(seed, offset, stream, groups):
    """The 16-bit values of the eight elements of every group in `groups` (uint64 array) -> uint64 [len(groups), 8]:
    philox4x32_10(key = (lo, hi of seed), counter = (lo, hi of offset + stream, lo, hi of group)); element e takes the low
    (even e) or high (odd e) half of word e >> 1."""
    g = np.asarray(groups, dtype=np.uint64)
    c = np.uint64((int(offset) + int(stream)) & 0xFFFFFFFFFFFFFFFF)
    words = philox4x32_10((int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF),
                          (np.full_like(g, c & LO), np.full_like(g, c >> S32), g & LO, g >> S32))
    out = np.empty((g.size, 8), dtype=np.uint64)
    for e in range(8):
        out[:, e] = (words[e >> 1] >> np.uint64(16 * (e & 1))) & np.uint64(0xFFFF)
    return out


def array_bits(n, seed, offset, stream=0):
    """r for elements 0..n-1 of a single array (lcv_sr_round): group i >> 3, element i % 8."""
    return halves(seed, offset, stream, np.arange((n + 7) // 8, dtype=np.uint64)).reshape(-1)[:n]


def first_chunks(numels):
    """first_chunk of every tensor of a descriptor table with these element counts, in order."""
    out, chunk = [], 0
    for n in numels:
        out.append(chunk)
        chunk += (n + CHUNK - 1) // CHUNK
    return out


def table_bits(numel, first_chunk, seed, offset, stream):
    """r for elements 0..numel-1 of a tensor of a descriptor table: group (first_chunk + i / 2048) * 256 + (i % 2048) / 8."""
    i = np.arange(0, numel, 8, dtype=np.uint64)
    groups = (np.uint64(first_chunk) + i // np.uint64(CHUNK)) * np.uint64(256) + (i % np.uint64(CHUNK)) // np.uint64(8)
    return halves(seed, offset, stream, groups).reshape(-1)[:numel]


def sr_round(x_bits, seed, offset):
    """lcv_sr_round on uint32 patterns."""
    x_bits = np.asarray(x_bits, dtype=np.uint32)
    return sr(x_bits, array_bits(x_bits.size, seed, offset))


# -------------------------------------------------------------------------------------------------------- the steps
def sgd_step(h, grad_bits, coef, lr, wd, first_chunk, seed, offset):
    """lcv_sr_sgd_step on one tensor of a table: lcv_master_sgd_step's sequence with the low word absent, p = SR(w, stream 0).
    uint16 in, uint16 out."""
    h = np.asarray(h, dtype=np.uint16)
    lr32, wd32 = F(lr), F(wd)
    w = W.bf16_to_f32(h)
    g = W.bf16_to_f32(grad_bits) * F(coef)
    if wd32 != 0:
        g = g + wd32 * w
    w = w + (-lr32) * g
    return sr(W.bits(w), table_bits(h.size, first_chunk, seed, offset, 0))


def adamw_step(h, m, v, grad_bits, coef, lr, beta1, beta2, eps, wd, step, first_chunk, seed, offset):
    """lcv_sr_adamw_step on one tensor of a table: the fp32 sequence of lcv_master_adamw_step (master_weights_ref.adamw_step
    with zero low words) on float(p), float(m), float(v), then SR with streams 0, 1, 2.  uint16 in, (p, m, v) uint16 out."""
    h = np.asarray(h, dtype=np.uint16)
    zero = np.zeros(h.shape, dtype=np.int16)
    hh, ll, m32, v32 = W.adamw_step(h, zero, W.bf16_to_f32(m), W.bf16_to_f32(v), grad_bits, coef, lr, beta1, beta2, eps, wd, step)
    bits = [table_bits(h.size, first_chunk, seed, offset, k) for k in range(3)]
    return sr(W.join(hh, ll), bits[0]), sr(W.bits(m32), bits[1]), sr(W.bits(v32), bits[2])

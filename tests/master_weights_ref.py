"""numpy restatement of include/lcv_hip_master.h: the (bf16 word, int16 low word) <-> fp32 master format and the two optimizer
steps, in np.float32 and in the header's op order (every operation rounded to nearest, nothing fused).  Helpers build the
tests' host-generated inputs, so that every intermediate is a normal fp32 number."""
import numpy as np

F = np.float32


# ---------------------------------------------------------------------------------------------------------- the format
def split(m):
    """uint32 master bit patterns -> (h uint16, l int16): h = (m + 0x8000) >> 16 in uint32, l = int16(m - (h << 16))."""
    m = np.asarray(m, dtype=np.uint32)
    h = ((m.astype(np.uint64) + 0x8000) & 0xFFFFFFFF) >> 16           # uint32 arithmetic, written without overflow warnings
    low = (m.astype(np.uint64) - (h << 16)) & 0xFFFF                  # the low 16 bits of the difference (mod 2^32)
    return h.astype(np.uint16), low.astype(np.uint16).view(np.int16)


def join(h, low):
    """(h uint16, l int16) -> uint32 master bit patterns: (h << 16) + l mod 2^32."""
    h = np.asarray(h, dtype=np.uint16).astype(np.int64)
    low = np.asarray(low, dtype=np.int16).astype(np.int64)
    return (((h << 16) + low) & 0xFFFFFFFF).astype(np.uint32)


def bits(x):
    return np.ascontiguousarray(x, dtype=F).view(np.uint32)


def floats(m):
    return np.ascontiguousarray(m, dtype=np.uint32).view(F)


def bf16_to_f32(h):
    return floats(np.asarray(h, dtype=np.uint16).astype(np.uint32) << 16)


def master(h, low):
    return floats(join(h, low))


# ---------------------------------------------------------------------------------------------------------- the steps
def sgd_step(h, low, grad_bits, coef, lr, wd):
    """w = join(h, l); g = float(grad) * coef; if wd != 0: g = g + wd * w; w = w + (-lr) * g; split(w)."""
    lr32, wd32, coef = F(lr), F(wd), F(coef)
    w = master(h, low)
    g = bf16_to_f32(grad_bits) * coef
    if wd32 != 0:
        g = g + wd32 * w
    w = w + (-lr32) * g
    return split(bits(w))


def adamw_scalars(lr, beta1, beta2, eps, wd, step):
    """Formed in double as torch/optim/adamw.py forms them, then narrowed to fp32 (lcv_adamw_step)."""
    bc1 = 1.0 - beta1 ** step
    bc2 = 1.0 - beta2 ** step
    return dict(c_wd=F(1.0 - lr * wd), w1=F(1.0 - beta1), b2=F(beta2), c2=F(1.0 - beta2), bc2_sqrt=F(np.sqrt(bc2)), eps=F(eps),
                step_size=F((lr / bc1) * -1.0))


def adamw_step(h, low, m, v, grad_bits, coef, lr, beta1, beta2, eps, wd, step):
    """The fp32 op sequence of lcv_adamw_step on p = join(h, l), fp32 moments; returns (h, l, m, v)."""
    s = adamw_scalars(lr, beta1, beta2, eps, wd, step)
    g = bf16_to_f32(grad_bits) * F(coef)
    p = master(h, low) * s["c_wd"]
    m = np.asarray(m, dtype=F)
    m = m + s["w1"] * (g - m)
    v = np.asarray(v, dtype=F) * s["b2"]
    v = v + (s["c2"] * g) * g
    d = np.sqrt(v) / s["bc2_sqrt"] + s["eps"]
    p = p + s["step_size"] * (m / d)
    hh, ll = split(bits(p))
    return hh, ll, m.astype(F), v.astype(F)


# ---------------------------------------------------------------------------------------------------------- inputs
def edge_patterns(n_random=1 << 16, seed=0):
    """Random 32-bit patterns plus +-0, denormals, the largest finite value, infinities, NaNs, ties and wrap-around."""
    rng = np.random.default_rng(seed)
    special = np.array([0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x807FFFFF, 0x00008000, 0x00007FFF,
                        0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00000, 0x7FFFFFFF, 0xFFFFFFFF,
                        0xFFFF8000, 0xFFFF7FFF, 0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0xBF808000, 0x7F7F8000],
                       dtype=np.uint32)
    return np.concatenate([special, rng.integers(0, 1 << 32, size=n_random, dtype=np.uint64).astype(np.uint32)])


def log_uniform(rng, n, lo_exp, hi_exp):
    """+-2^u, u uniform in [lo_exp, hi_exp], as fp32."""
    mag = np.exp2(rng.uniform(lo_exp, hi_exp, size=n))
    return (mag * rng.choice([-1.0, 1.0], size=n)).astype(F)


def to_bf16_bits(x):
    """fp32 -> bf16 bit patterns, round to nearest even (finite inputs): what `.to(torch.bfloat16)` stores."""
    u = bits(x).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)


def weights(rng, n):
    """Masters with |w| in [2^-10, 2] and all 32 bits live, as (h, l)."""
    return split(bits(log_uniform(rng, n, -10.0, 1.0)))


def grads(rng, n):
    """bf16 gradients with |g| in [2^-20, 8], as bit patterns."""
    return to_bf16_bits(log_uniform(rng, n, -20.0, 3.0))

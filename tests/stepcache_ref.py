"""numpy restatement of include/lcv_hip_stepcache.h: the three element-wise results of the first-block step cache on bf16 bit
patterns (uint16), and the two per-row sums in float64.

Every fp32 operation below is one correctly rounded numpy float32 operation and every bf16 conversion is round-to-nearest-even,
as in the header, so the element-wise results are compared bit for bit.  The sums have a fixed order on the device that numpy
does not restate: they are compared against float64 within a bound the tests derive (or bit for bit where every partial sum is
exact)."""
import numpy as np

F = np.float32


def bf16_to_f32(h):
    return (np.asarray(h, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def f32_to_bf16(x):
    """Round to nearest, ties to even; a NaN stays a (quiet) NaN."""
    x = np.asarray(x, dtype=np.float32)
    u = x.view(np.uint32)
    r = ((u + (np.uint32(0x7FFF) + ((u >> 16) & np.uint32(1)))) >> 16).astype(np.uint16)
    return np.where(np.isnan(x), ((u >> 16) | np.uint32(0x0040)).astype(np.uint16), r)


def residual(x1, x0):
    """r = bf16(float(x1) - float(x0)); also the store, R = bf16(float(xL) - float(x1))."""
    return f32_to_bf16(bf16_to_f32(x1) - bf16_to_f32(x0))


def apply(x1, R):
    """bf16(float(x1) + float(R))."""
    return f32_to_bf16(bf16_to_f32(x1) + bf16_to_f32(R))


def sums(r, p):
    """Per row of [rows, n] bit patterns: (num, den) = (sum |float(r) - float(p)|, sum |float(p)|), each term formed in fp32 as
    the kernel forms it (d = r - p rounded once, then |d|) and added in float64."""
    r, p = np.atleast_2d(r), np.atleast_2d(p)
    d = np.abs(bf16_to_f32(r) - bf16_to_f32(p))
    return d.astype(np.float64).sum(axis=1), np.abs(bf16_to_f32(p)).astype(np.float64).sum(axis=1)


def decision(num, den, thr):
    """all(num[b] < fp32(thr * den[b])) on fp32 sums: one rounded product, a strict compare."""
    num, den = np.asarray(num, dtype=F), np.asarray(den, dtype=F)
    with np.errstate(invalid="ignore", over="ignore"):
        return int(bool(np.all(num < F(thr) * den)))


def draw(rng, shape, lo=-10.0, hi=1.0):
    """bf16 bit patterns with |x| log-uniform in [2^lo, 2^hi] and both signs (the draw of the optimizer tests' weights)."""
    mag = np.exp2(rng.uniform(lo, hi, size=shape))
    return f32_to_bf16((mag * rng.choice([-1.0, 1.0], size=shape)).astype(np.float32))

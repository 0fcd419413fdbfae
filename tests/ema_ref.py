"""numpy restatement of include/lcv_hip_ema.h: the fp32 average of the masters over the optimizer steps, on the format of
master_weights_ref (join, split), in np.float32 and in the header's op order (every operation rounded to nearest, nothing fused).
Masters and averages travel as uint32 bit patterns, so that NaN payloads and the signs of zeros are compared too."""
import numpy as np

import master_weights_ref as W

F = np.float32


def load(h, low):
    """e = join(h, l): the average's bits."""
    return W.join(h, low)


def update(h, low, e_bits, beta):
    """w = join(h, l); d = w - e; t = b * d; e = w - t, with b = float32(beta).  Returns the new average's bits."""
    b = F(beta)
    w = W.floats(W.join(h, low))
    e = W.floats(e_bits)
    with np.errstate(all="ignore"):
        d = (w - e).astype(F)
        t = (b * d).astype(F)
        return W.bits((w - t).astype(F)).copy()


def swap(h, low, e_bits):
    """w = join(h, l); (h, l) = split(e); e = w.  Returns (h, l, e bits)."""
    w = W.join(h, low)
    hh, ll = W.split(np.asarray(e_bits, dtype=np.uint32))
    return hh, ll, w


def ema_beta(beta, t, warmup=False):
    """The beta of the t-th update (t from 1): beta, or under warm-up min(beta, (1 + t) / (10 + t)), in double."""
    beta = float(beta)
    return min(beta, (1.0 + t) / (10.0 + t)) if warmup else beta

"""numpy restatement of include/lcv_hip_sam.h: the sum of squares of the (plain or |w| + eta scaled) gradient in the header's
fixed order, the perturbation w' = w + c * t' with its saves and the realized move, and the restore, in np.float32 (every
operation rounded to nearest, nothing fused).  It follows the header, not the kernel.  The fixed-order reduction is
tests/trust_ref.py's (the header repeats that order word for word), the word formats are tests/master_weights_ref.py's.

A tensor is a dict: form "f32" has `w` (fp32 values) and `g` (fp32 gradients); form "bf16" has `h` (uint16 bf16 words), `low`
(int16 low words, or None: all zero) and `g` (uint16 bf16 gradient words).

The bound the tests hold the perturbation's norm to follows trust_ref's derivation.  u = 2^-24, `depth` is trust_ref.depth(), the
longest chain of fp32 additions a term passes through.
  plain:     q = fl(g^2) carries 1 rounding, so s = S (1 + e), |e| <= (1 + u)^(depth + 1) - 1, and sqrt halves it;
             c = fl(rho_f / fl(fl(sqrt(s)) + 1e-12f)) adds 3 roundings, e = fl(c g) 1:   eps = ((depth + 1) / 2 + 4) u.
  adaptive:  a = fl(|w| + eta_f) 1 rounding, t = fl(a g) 2, q = fl(t^2) 5, so k = depth + 5 against S formed from the exact
             |w| + eta_f; e = fl(c fl(a t)) carries 5 against c a^2 g, and e / a is what the scaled norm
             |e / (|w| + eta)| = rho measures:                                           eps = ((depth + 5) / 2 + 8) u.
Both are first order; one more u covers the second-order terms and the 1e-12 in the denominator (the tests' norms are above
2^-10, where 1e-12 is below u relative).  `eps_rho()` gives the figure.  The stored w' = fl(w + e) is off from w + e by at most
u |w'| per element, so for fp32 parameters
    | |w' - w| - rho_f | <= rho_f eps + u |w'|          (adaptive: both norms of the element-wise quotient by |w| + eta_f),
which is also the bound on a reported `realized` norm up to its own summation error (depth + 3 roundings, halved by the root)."""
import numpy as np

import master_weights_ref as W
import trust_ref as T

F = np.float32
TINY = F(1e-12)


def master_of(t):
    """The fp32 w of a tensor: the stored value, join(h, l), or float(h) without low words."""
    if "w" in t:
        return np.asarray(t["w"], dtype=F)
    h = np.asarray(t["h"], dtype=np.uint16)
    return W.master(h, np.zeros(h.shape, np.int16) if t.get("low") is None else t["low"])


def grad_of(t):
    return np.asarray(t["g"], dtype=F) if "w" in t else W.bf16_to_f32(t["g"])


def scaled(w, g, adaptive, eta):
    """(t, a): t = g, or a = |w| + eta_f; t = a * g."""
    g = np.asarray(g, dtype=F)
    if not adaptive:
        return g, None
    a = np.abs(np.asarray(w, dtype=F)) + F(eta)
    return (a * g).astype(F), a.astype(F)


def sumsq(tensors, adaptive=False, eta=0.01):
    """lcv_sam_sumsq: (per_tensor [n] fp32, out [2] fp32).  q = t * t; acc = acc + q in the three-stage order."""
    pairs = []
    for t in tensors:
        s, _ = scaled(master_of(t) if adaptive else None, grad_of(t), adaptive, eta)
        pairs.append((s, np.zeros(s.shape, F)))          # trust_ref squares w - w0: t - 0 is t
    return T.sumsq(pairs)


joint_total = T.joint_total


def coef(s, rho):
    """c = rho_f / (sqrtf(s) + 1e-12f), or None where nothing is written: rho_f == 0, !(s > 0) (a NaN too), s == +inf."""
    s, rho = F(s), F(rho)
    if rho == 0 or not s > 0 or np.isinf(s):
        return None
    n = F(np.sqrt(s))
    den = F(n + TINY)
    return F(rho / den)


def perturb_elem(w, g, adaptive, eta, c):
    """plain: e = c * g; adaptive: u = a * t; e = c * u; then w' = w + e."""
    t, a = scaled(w, g, adaptive, eta)
    if adaptive:
        u = (a * t).astype(F)
        e = (F(c) * u).astype(F)
    else:
        e = (F(c) * t).astype(F)
    return (np.asarray(w, dtype=F) + e).astype(F)


def perturb(tensors, rho, adaptive=False, eta=0.01, total=None):
    """lcv_sam_sumsq + lcv_sam_perturb over a list of tensors.  Returns a dict: `words` (per tensor the stored words after the
    call: uint16 h' or fp32 w'; the input array itself where nothing was written), `saves` (copies of the words the forward
    read), `per` and `realized` (the realized move's per-tensor sums and [sum, sqrt]), `sumsq` (per_tensor, out of the gradient),
    `trace` = (s, realized[0]), `wrote`.  `total`: the joint total of several tables; default this table's own."""
    per_g, out_g = sumsq(tensors, adaptive, eta)
    s = out_g[0] if total is None else F(total)
    c = coef(s, rho)
    words, saves, moves = [], [], []
    for t in tensors:
        f32 = "w" in t
        old = np.asarray(t["w"], dtype=F) if f32 else np.asarray(t["h"], dtype=np.uint16)
        saves.append(old.copy())
        if c is None:
            words.append(old)
            moves.append((np.zeros(old.shape, F), np.zeros(old.shape, F)))
            continue
        wp = perturb_elem(master_of(t), grad_of(t), adaptive, eta, c)
        if f32:
            words.append(wp)
            d = (wp - old).astype(F)
        else:
            hp = W.to_bf16_bits(wp)
            words.append(hp)
            d = (W.bf16_to_f32(hp) - W.bf16_to_f32(old)).astype(F)
        moves.append((d, np.zeros(d.shape, F)))
    per_r, out_r = T.sumsq(moves)
    return dict(words=words, saves=saves, per=per_r, realized=out_r, sumsq=(per_g, out_g), trace=(F(s), out_r[0]),
                wrote=c is not None)


def restore(saves):
    """lcv_sam_restore: param = save, word for word."""
    return [s.copy() for s in saves]


# ---------------------------------------------------------------------------------------------------------- the bound
def eps_rho(numels, adaptive=False, optimizers=1):
    """The relative error of the perturbation's (scaled) norm against rho_f before the last addition (module docstring)."""
    d = T.depth(numels, optimizers)
    return (((d + 5) / 2.0 + 8.0) if adaptive else ((d + 1) / 2.0 + 4.0)) * T.U + T.U


def eps_realized(numels, adaptive=False, optimizers=1):
    """eps_rho plus the summation error of a reported realized norm: (depth + 3) / 2 roundings more."""
    return eps_rho(numels, adaptive, optimizers) + (T.depth(numels, optimizers) + 3) / 2.0 * T.U


def norm64(arrays):
    return float(np.sqrt(sum(np.sum(np.asarray(a, dtype=np.float64) ** 2) for a in arrays)))

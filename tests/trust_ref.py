"""numpy restatement of include/lcv_hip_trust.h: the sum of squares of the drift w - w0 in the header's fixed order and the
projection w = w0 + c * (w - w0), in np.float32 (every operation rounded to nearest, nothing fused).  It follows the header, not
the kernel.  A tensor is a pair (w, w0) of fp32 arrays: for bf16 master-weight parameters w = join(h, l) and w0 = float(h0)
(`from_words`, tests/master_weights_ref.py's format), for fp32 parameters the stored values; a missing anchor is w0 = 0.

The error bound the tests hold the projection to.  u = 2^-24.  Every term q = fl(fl(w - w0)^2) carries three roundings and is
non-negative, so the computed sum is s = S (1 + e) with S the exact sum of squares of the exact drifts and
|e| <= (1 + u)^k - 1, k = depth + 3, where `depth` is the longest chain of fp32 additions a term passes through:
    chunk    8 (a thread's elements) + 6 (butterfly) + 3 (waves)                       = 17
    tensor   ceil(chunks_k / 256) (a thread's partials) + 6 + 3
    total    ceil(n_tensors / 256) + 6 + 3
    joint    one more addition per further optimizer of the ball
(`depth()` below).  The coefficient c = fl(sqrt(fl(r2 / s))) is sqrt(r2 / S) (1 + e)^-1/2 (1 + u)^1.5 at most, the projected drift
of an element fl(c * fl(w - w0)) adds (1 + u)^2, and the last addition w0 + u' is off by at most u |w'|.  Over the ball:
    |theta' - theta0| <= sqrt(r2) (1 + eps_s) + u |theta'|,      eps_s = (k / 2 + 4) u      (first order, rounded up).
For the whole model (1 022 parameter tensors, 13.58 G elements, tensors of up to 45 M elements = 22 000 chunks)
depth = 17 + (86 + 9) + (4 + 9) = 125, k = 128 and eps_s = 68 u < 2^-17 = 128 u, so EPS_S = 2^-17 serves every size up to that one;
`eps_s()` gives the figure for a concrete table.
A reported drift (`drift_norm`: the square root, in double, of lcv_trust_sumsq's fp32 totals added in double) is the exact drift
times (1 + e)^1/2 <= 1 + k u / 2 < 1 + eps_s, so a reported drift is held to the bound with one more factor (1 + eps_s).  Under
tensor scope every tensor k holds |theta'_k - theta0_k| <= sqrt(r2_k) (1 + eps_s) + u |theta'_k| with r2_k = fp32(R^2 numel_k); the
square root of the sum of squares of the right-hand sides is at most the sum of the two parts' roots (Minkowski), which is
R sqrt(N) (1 + u)^1/2 (1 + eps_s) + u |theta'|: the global form of the bound holds for the whole table there too."""
import numpy as np

import master_weights_ref as W

F = np.float32
U = 2.0 ** -24
EPS_S = 2.0 ** -17
CHUNK = 2048
_LANE = np.arange(64)


def from_words(h, low, h0):
    """(w, w0) of bf16 master-weight words: join(h, l) and float(h0); low None is all-zero low words, h0 None a zero base."""
    h = np.asarray(h, dtype=np.uint16)
    low = np.zeros(h.shape, np.int16) if low is None else low
    return W.master(h, low), (np.zeros(h.shape, F) if h0 is None else W.bf16_to_f32(h0))


def to_words(w):
    """fp32 masters -> (h, l)."""
    return W.split(W.bits(w))


def _block_sum(acc):
    """[..., 256] per-thread sums -> [...]: the butterfly of each wave (for o = 32 .. 1: v = v + v[lane ^ o]), then the four waves
    in wave order, ((p0 + p1) + p2) + p3."""
    v = np.asarray(acc, dtype=F).reshape(acc.shape[:-1] + (4, 64))
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[..., _LANE ^ o]
    p = v[..., 0]
    return ((p[..., 0] + p[..., 1]) + p[..., 2]) + p[..., 3]


def _strided_sum(x, lanes=256):
    """Thread t of `lanes` starts at 0 and adds x[t], x[t + lanes], ... in index order; returns the [lanes] per-thread sums."""
    x = np.asarray(x, dtype=F).reshape(-1)
    rows = -(-x.size // lanes)
    pad = np.zeros(rows * lanes, dtype=F)
    pad[:x.size] = x
    live = np.arange(rows * lanes) < x.size
    pad, live = pad.reshape(rows, lanes), live.reshape(rows, lanes)
    acc = np.zeros(lanes, dtype=F)
    for r in range(rows):
        acc = np.where(live[r], acc + pad[r], acc)
    return acc


def chunk_partials(w, w0):
    """Step 1: one fp32 partial per chunk of 2048 elements of one tensor."""
    w, w0 = np.asarray(w, dtype=F).reshape(-1), np.asarray(w0, dtype=F).reshape(-1)
    chunks = -(-w.size // CHUNK)
    d = np.zeros(chunks * CHUNK, dtype=F)
    d[:w.size] = w - w0
    q = (d * d).reshape(chunks, 256, 8)
    live = (np.arange(chunks * CHUNK) < w.size).reshape(chunks, 256, 8)
    acc = np.zeros((chunks, 256), dtype=F)
    for e in range(8):
        acc = np.where(live[..., e], acc + q[..., e], acc)
    return _block_sum(acc)


def sumsq(tensors):
    """lcv_trust_sumsq: (per_tensor [n] fp32, out [2] fp32) of a list of (w, w0) pairs."""
    per = np.array([_block_sum(_strided_sum(chunk_partials(w, w0))) for w, w0 in tensors], dtype=F)
    total = F(_block_sum(_strided_sum(per)))
    return per, np.array([total, np.sqrt(total)], dtype=F)


def joint_total(totals):
    """The ball's total over several optimizers: their totals added in their order in fp32."""
    acc = F(totals[0])
    for t in totals[1:]:
        acc = F(acc + F(t))
    return acc


def radius2(R, count):
    """(float)(R * R * N), formed in double and rounded once."""
    return F(float(R) * float(R) * float(count))


def coef(s, r2):
    """1 inside the ball (and for a NaN s), else sqrt(r2 / s), both correctly rounded."""
    s, r2 = F(s), F(r2)
    if not s > r2:
        return F(1.0)
    return F(np.sqrt(F(r2 / s)))


def project_elem(w, w0, c):
    """d = w - w0; u = c * d; w = w0 + u."""
    w, w0 = np.asarray(w, dtype=F), np.asarray(w0, dtype=F)
    d = w - w0
    u = F(c) * d
    return (w0 + u).astype(F)


def project(tensors, R, scope="global", total=None, count=None):
    """lcv_trust_sumsq + lcv_trust_project over a list of (w, w0): returns (new w list, per_tensor, out, trace), trace =
    (total before the projection, smallest coefficient applied).  `total` / `count`: the joint total and element count of a ball
    shared with other tables (global scope); default this table's own.  A tensor inside its ball is returned as the same array."""
    per, out = sumsq(tensors)
    s = out[0] if total is None else F(total)
    n = sum(np.size(w) for w, _ in tensors) if count is None else count
    new, cmin = [], F(1.0)
    for (w, w0), sk in zip(tensors, per):
        if scope == "tensor":
            sk, r2 = sk, radius2(R, np.size(w))
        else:
            sk, r2 = s, radius2(R, n)
        if not sk > r2:
            new.append(w)
            continue
        c = coef(sk, r2)
        cmin = min(cmin, c)
        new.append(project_elem(w, w0, c))
    return new, per, out, (s, F(cmin))


# ---------------------------------------------------------------------------------------------------------- the bound
def depth(numels, optimizers=1):
    """The longest chain of fp32 additions a term passes through (module docstring)."""
    worst = max(-(-(-(-n // CHUNK)) // 256) for n in numels)
    return 17 + (worst + 9) + (-(-len(numels) // 256) + 9) + (optimizers - 1)


def eps_s(numels, optimizers=1):
    return ((depth(numels, optimizers) + 3) / 2.0 + 4.0) * U


def drift64(tensors):
    """|theta - theta0| in float64 (every difference exact, the sum sequential in float64)."""
    acc = np.float64(0.0)
    for w, w0 in tensors:
        d = np.asarray(w, dtype=np.float64).reshape(-1) - np.asarray(w0, dtype=np.float64).reshape(-1)
        acc += np.sum(d * d, dtype=np.float64)
    return float(np.sqrt(acc))


def norm64(ws):
    return float(np.sqrt(sum(np.sum(np.asarray(w, dtype=np.float64) ** 2) for w in ws)))


def bound_holds(tensors, r2, eps=EPS_S):
    """|theta' - theta0| <= sqrt(r2) (1 + eps_s) + 2^-24 |theta'| for the projected (w', w0) pairs."""
    return drift64(tensors) <= float(np.sqrt(np.float64(r2))) * (1.0 + eps) + U * norm64([w for w, _ in tensors])

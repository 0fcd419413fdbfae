"""numpy restatement of include/lcv_hip_dora.h: the row norm of the adapted weight and the column scale of weight-decomposed
LoRA, forward and backward, every step one IEEE fp32 operation in the order the header states.  bf16 arrays travel as float32
arrays holding bf16 values (`bf16_rne` makes them); every function returns float32."""
import numpy as np

KTILE, ROWS, SLAB, QUARTER = 512, 16, 64, 16   # LCV_DORA_NORM_KTILE, LCV_DORA_NORM_ROWS, LCV_DORA_SLAB, LCV_DORA_SLAB_QUARTER
F = np.float32


def bf16_rne(x: np.ndarray) -> np.ndarray:
    """float32 -> the nearest bf16 value (ties to even), as float32.  Finite inputs."""
    u = np.ascontiguousarray(x, dtype=F).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) >> 16 << 16
    return u.astype(np.uint32).view(F).reshape(np.shape(x))


def weight_norm(W: np.ndarray, A: np.ndarray = None, B: np.ndarray = None, s: float = 0.0) -> np.ndarray:
    W = np.asarray(W, dtype=F)
    N, K = W.shape
    assert K % 8 == 0
    v = W
    if B is not None:
        A, B = np.asarray(A, dtype=F), np.asarray(B, dtype=F)
        t = np.zeros((N, K), dtype=F)
        for r in range(A.shape[0]):
            t = t + B[:, r:r + 1] * A[r:r + 1, :]          # the product of two bf16 values is exact
        u = F(s) * t
        v = W + u
    q = v * v
    tiles = -(-K // KTILE)
    qp = np.zeros((N, tiles * KTILE), dtype=F)             # columns past K add nothing
    qp[:, :K] = q
    qp = qp.reshape(N, tiles, 64, 8)
    P = np.zeros((N, 64), dtype=F)
    for t_ in range(tiles):                                 # lane l: its columns in increasing k
        for e in range(8):
            P = P + qp[:, t_, :, e]
    lanes = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        P = P + P[:, lanes ^ o]
    assert P.dtype == F
    return np.sqrt(P[:, 0])


def col_scale(m: np.ndarray, wn: np.ndarray) -> np.ndarray:
    m, wn = np.asarray(m, dtype=F), np.asarray(wn, dtype=F)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = m / wn
    return np.where(wn == 0, F(0), c).astype(F)


def colscale_fwd(pre: np.ndarray, m: np.ndarray, wn: np.ndarray, bias: np.ndarray = None) -> np.ndarray:
    y = np.asarray(pre, dtype=F) * col_scale(m, wn)[None, :]
    if bias is not None:
        y = y + np.asarray(bias, dtype=F)[None, :]
    assert y.dtype == F
    return bf16_rne(y)


def slab_sum(prod: np.ndarray) -> np.ndarray:
    """sum over rows of `prod` [M, N] in the kernel's order: per slab of SLAB rows four quarters, each row by row from 0, added
    as ((q0 + q1) + q2) + q3 (a quarter without rows is 0); then the slabs from 0."""
    prod = np.asarray(prod, dtype=F)
    M, N = prod.shape
    S = np.zeros(N, dtype=F)
    for r0 in range(0, M, SLAB):
        quarters = []
        for q0 in range(r0, r0 + SLAB, QUARTER):
            q = np.zeros(N, dtype=F)
            for r in range(q0, min(q0 + QUARTER, M)):
                q = q + prod[r]
            quarters.append(q)
        S = S + (((quarters[0] + quarters[1]) + quarters[2]) + quarters[3])
    return S


def colscale_bwd(dy: np.ndarray, pre: np.ndarray, m: np.ndarray, wn: np.ndarray):
    dy, pre, wn = np.asarray(dy, dtype=F), np.asarray(pre, dtype=F), np.asarray(wn, dtype=F)
    dpre = bf16_rne(dy * col_scale(m, wn)[None, :])
    S = slab_sum(dy * pre)                                  # exact products
    with np.errstate(divide="ignore", invalid="ignore"):
        dm = S / wn
    return dpre, np.where(wn == 0, F(0), dm).astype(F)

"""numpy restatement of the LoRA dropout mask (include/lcv_hip_lora.h): Philox4x32-10 and the element layout.  A helper,
not a test module; tests/test_lora_dropout_host.py holds it to the published known-answer vectors."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
LO = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(key, ctr):
    """key: (k0, k1) ints; ctr: four uint64 arrays (or ints) holding 32-bit values -> four uint64 arrays of 32-bit words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & LO for c in ctr)
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0 = M0 * c0
        p1 = M1 * c2
        n0 = (p1 >> S32) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> S32) ^ c3 ^ np.uint64(k1)
        c0, c1, c2, c3 = n0, p1 & LO, n2, p0 & LO
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def threshold(p: float) -> int:
    """T = round-half-even(p * 65536) clamped to 1..65535 (Python's round is half-even, as the library's lrint)."""
    return min(max(int(round(float(p) * 65536.0)), 1), 65535)


def scale(p: float) -> np.float32:
    return np.float32(65536.0) / np.float32(65536 - threshold(p))


def mask(M: int, K: int, p: float, seed: int, offset: int, row0: int = 0) -> np.ndarray:
    """uint8 [M, K]: 1 where the element of global row row0 + m, column k is kept."""
    assert K % 8 == 0
    K8 = K // 8
    g = np.uint64(row0) * np.uint64(K8) + np.arange(M * K8, dtype=np.uint64)      # ((row0 + m) * K + k) >> 3
    off = np.uint64(offset & 0xFFFFFFFFFFFFFFFF)
    words = philox4x32_10((seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF),
                          (np.full_like(g, off & LO), np.full_like(g, off >> S32), g & LO, g >> S32))
    T = np.uint64(threshold(p))
    out = np.empty((M * K8, 8), dtype=np.uint8)
    for e in range(8):
        half = (words[e >> 1] >> np.uint64(16 * (e & 1))) & np.uint64(0xFFFF)
        out[:, e] = half >= T
    return out.reshape(M, K)

"""The inputs of the flash-attention edge tests (tests/test_gpu_attn_kernel_edges.py on the GPU, tests/test_kernel_ref.py on the CPU),
built once on the CPU and never modified.  A plain helper module (compare tests/delta_cases.py, tests/kernel_ref.py).

Exact scores.  q (for the unit-scale cases already in log2 units: scale = ln 2) and k take their entries from {-1/2, 0, 1/2} on the
first 120 of the 128 dimensions; a few designated rows and keys are multiples of 1/2 of larger size.  Every partial sum of q . k in
any order is then a multiple of 1/4 far below 2^24 / 4: exact in fp32, also when the accumulator starts at minus the running
max (one of the row's scores).  The last RES = 8 dimensions carry a common offset: every key holds 1/2 there, every ordinary
query 0, so the ordinary scores do not see them.

Designated rows (all of one (batch, head) differ from every other's: the sign pattern w0 is drawn per (b, h); w1 and w2 are w0
with the signs of two different halves of the dimensions flipped, so the three are pairwise orthogonal):
  rows 0 and Nq - 1   q = w0 / 2.  The HEAVY keys - the last key, the first key of the last 64-key tile and key 0 - are A_h w0:
                      equal scores far above the rest, so each carries 1 / (their number) >= 1/4 of these rows' probability and
                      none carries all of it: counting one twice or dropping it moves the output by a large part of |v|.
and, where Nq >= 8,
  row 1               q = w1 / 2; key j1 = A_j w1 in tile t1 >= 1 (where Nk has room for it) lies far more than ATTN_RESCALE_THR
                      above whatever row 1 saw before,
  row 2               q = -w1 / 2: the same key lies far below its running max (some rows of the 32-row group rescale, not all),
  row 3               q = w2 / 2; key 3 (tile 0) = A_s w2 on n0 dimensions sets its maximum, key j2 = A_s w2 on n2 > n0 dimensions in
                      tile t2 >= 1, t2 != t1, exceeds it by a growth in (0, ATTN_RESCALE_THR] that must NOT rescale,
  row 4               an offset of -96 .. -131 (log2 units) on the reserved dimensions: ALL its scores are below -40, tile
                      0 sets a negative first maximum,
  row 5               an offset near +300: overflow if no maximum were subtracted.
v, dO (and prev_dk / prev_dv of the accumulate_kv cases): random bf16, different per (b, h).
"""
import functools
import math

import torch

BF16 = torch.bfloat16
D, RES = 128, 8
ND = D - RES
LN2 = 0.6931471805599453
GEN_SCALE = 128 ** -0.5
THR = 6.0                      # ATTN_RESCALE_THR (csrc/attn_common.h), log2 units
B0, H0 = 2, 3

# (amplitude of the heavy keys, of the jump key, of the two keys of row 3, their dimension counts, row 4's and row 5's offset entries)
_UNIT = dict(a_h=0.5, a_j=2.0, a_s=0.5, n0=80, n2=96, neg=-24.0, pos=75.0)      # scores 30 | 120 | 20 -> 24 | -96 | +300
_GEN = dict(a_h=2.0, a_j=16.0, a_s=2.0, n0=104, n2=120, neg=-256.0, pos=576.0)   # x = 0.1275 q.k: 15.3 | 122 | 13.3 -> 15.3 | -131 | +294


def f32(v: float) -> float:
    return float(torch.tensor(v, dtype=torch.float32))


def scale_of(unit: bool) -> float:
    """The fp32 scale the call passes: ln 2 for q in log2 units (the library's unit-scale bodies), head_dim^-0.5 otherwise."""
    return f32(LN2 if unit else GEN_SCALE)


def tiles(Nk: int) -> int:
    return (Nk + 63) // 64


def planted(Nq: int, Nk: int):
    """-> dict of the planted positions this shape has room for: heavy (list of keys), j0, j1, t1, j2, t2 (None where absent)."""
    nt = tiles(Nk)
    heavy = sorted({Nk - 1, 64 * (nt - 1), 0})
    out = dict(heavy=heavy, j0=None, j1=None, t1=None, j2=None, t2=None)
    if Nq < 8 or nt < 2:
        return out
    if nt >= 3:
        out["t1"] = nt - 2
    elif Nk - 64 >= 8:
        out["t1"] = 1
    if out["t1"] is not None:
        out["j1"] = 64 * out["t1"] + 5
    if nt >= 4:
        out.update(j0=3, t2=1, j2=64 + 9)
    return out


@functools.lru_cache(maxsize=None)
def inputs(Nq: int, Nk: int, unit: bool, B: int = B0, H: int = H0):
    """CPU tensors q, d_o [B, Nq, H, D] and k, v, prev_dk, prev_dv [B, Nk, H, D], bf16, as a dict with `scale`."""
    g = torch.Generator().manual_seed(977 * Nq + 31 * Nk + 7 * B + H + (500_000 if unit else 0))
    c = _UNIT if unit else _GEN
    grid = lambda n: torch.randint(-1, 2, (B, n, H, D), generator=g).to(torch.float32) / 2
    q, k = grid(Nq), grid(Nk)
    q[..., ND:] = 0.0
    k[..., ND:] = 0.5
    w0 = (torch.randint(0, 2, (B, H, ND), generator=g) * 2 - 1).to(torch.float32)
    blk = torch.arange(ND) // (ND // 4)                # four blocks of 30: w1 = w0 (+ + - -), w2 = w0 (+ - + -), pairwise orthogonal,
    w = torch.stack([w0, w0 * torch.where(blk < 2, 1.0, -1.0), w0 * torch.where(blk % 2 == 0, 1.0, -1.0)])   # so no pattern's keys weigh on another's rows
    pl = planted(Nq, Nk)
    for r in {0, Nq - 1}:
        q[:, r, :, :ND] = w[0] / 2
    if Nq >= 8:
        q[:, 1, :, :ND] = w[1] / 2
        q[:, 2, :, :ND] = -w[1] / 2
        q[:, 3, :, :ND] = w[2] / 2
        q[:, 4, :, ND:] = c["neg"]
        q[:, 5, :, ND:] = c["pos"]
    if pl["j0"] is not None:
        k[:, pl["j0"], :, :ND] = 0.0
        k[:, pl["j0"], :, :c["n0"]] = c["a_s"] * w[2][..., :c["n0"]]
        k[:, pl["j2"], :, :ND] = 0.0
        k[:, pl["j2"], :, :c["n2"]] = c["a_s"] * w[2][..., :c["n2"]]
    if pl["j1"] is not None:
        k[:, pl["j1"], :, :ND] = c["a_j"] * w[1]
    for j in pl["heavy"]:
        k[:, j, :, :ND] = c["a_h"] * w[0]
    rnd = lambda n, s=1.0: (torch.randn(B, n, H, D, generator=g) * s).to(BF16)
    out = dict(q=q.to(BF16), k=k.to(BF16), v=rnd(Nk), d_o=rnd(Nq), prev_dk=rnd(Nk, 0.5), prev_dv=rnd(Nk, 0.5), scale=scale_of(unit))
    assert torch.equal(out["q"].float(), q) and torch.equal(out["k"].float(), k)      # the grids are bf16 values
    return out


def schedule(x: torch.Tensor, group: int = 32, thr: float = THR):
    """The deferred-max schedule of the forward kernels on float64 scores x [..., Nq, Nk] (log2 units): per 64-key tile t >= 1
    and 32-row group, growth[t][..., Nq] = tile max - running max BEFORE the tile (before[t]), and rescaled[t][..., n_groups].  The running
    max of a row is raised when SOME row of its group grows by more than thr (attn_fwd.hip; sdpa_at_kernel_rounding)."""
    Nq, Nk = x.shape[-2:]
    ng = (Nq + group - 1) // group
    pad = ng * group - Nq
    m = x[..., :64].amax(-1)
    growth, rescaled, before = {}, {}, {}
    for t in range(1, tiles(Nk)):
        mx = x[..., 64 * t: 64 * t + 64].amax(-1)
        gr = mx - m
        before[t] = m
        grp = torch.nn.functional.pad(gr, (0, pad), value=-math.inf).unflatten(-1, (ng, group))
        over = (grp > thr).any(-1)
        growth[t], rescaled[t] = gr, over
        m = torch.where(over.repeat_interleave(group, -1)[..., :Nq], torch.maximum(m, mx), m)
    return growth, rescaled, before


# ---- the shapes ------------------------------------------------------------------------------------------------------------
# (body the library must pick, Nq, Nk, unit scale, LCV_ATTN_FWD_W64 value or None)
FWD_SHORT = "attn_fwd_kernel<8, 0, true, 0>"
FWD_GENERAL = "attn_fwd_kernel<8, 0, false, 1>"
FWD_W64 = "attn_fwd_w64_kernel"
FWD_PIPE = "attn_fwd_pipe_kernel"
FWD_WIDE = "attn_fwd_kernel<8, 0, false, 3>"
FWD_CASES = ([(FWD_SHORT, nq, nk, unit, None) for nk in (1, 5, 63, 64, 65, 77, 128, 129, 512) for nq in (1, 33, 257) for unit in (False, True)]
             + [(FWD_GENERAL, nq, nk, False, None) for nk in (513, 576, 641) for nq in (33, 257)]
             + [(body, nq, nk, True, knob) for body, knob in ((FWD_W64, None), (FWD_PIPE, "0"))
                for nk in (513, 576, 640, 700) for nq in (1, 63, 64, 65, 300)])
WIDE_CASE = dict(B=1, H=2, Nq=33, Nk=513)          # attn_fwd_kernel<8, 0, false, 3>: reached through a key stride, see the GPU test

BWD_CASES = [(nq, nk) for nk in (1, 5, 77, 127, 128, 129, 333) for nq in (1, 31, 32, 33, 257)]
# the split query sweep of the first-form pass A (attn_bwd_qsplit): 63 tiles (no split), 64 (4 splits, last tile one row), 65 (16/16/16/17)
SPLIT_CASES = [(nq, nk) for nq in (2016, 2017, 2080) for nk in (77, 128)]
SPLIT_PAIR = [(3, 85, 2048, 77), (2, 128, 2048, 77)]   # B H = 255: two splits; 256: none


def qsplit(B: int, H: int, Nq: int, Nk: int) -> int:
    """attn_bwd_qsplit of csrc/attn_bwd.hip, from its source comment and body: few key blocks, many query tiles."""
    kblocks, nt = (Nk + 127) // 128, (Nq + 31) // 32
    qs = 1
    if Nk <= 128 and kblocks * H * B < 256 and nt >= 64:
        qs = min(512 // (kblocks * H * B), nt // 16, 64)
    return max(qs, 1)


def ws_floats(B: int, H: int, Nq: int, Nk: int) -> int:
    """What include/lcv_hip.h documents for lcv_attn_bwd_ws_floats: delta, the two padded row-constant rows, the slices."""
    n = B * H * (Nq + 2 * ((Nq + 31) // 32 * 32))
    qs = qsplit(B, H, Nq, Nk)
    return n + (qs * B * H * Nk * 256 if qs > 1 else 0)


def is_small(B: int, H: int, Nq: int, Nk: int) -> bool:
    """The cases the CPU tests of tests/test_kernel_ref.py walk: Nq Nk <= 300 x 1088 at B H = 6."""
    return B * H * Nq * Nk <= B0 * H0 * 300 * 1088

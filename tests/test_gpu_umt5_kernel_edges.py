"""GPU: the UMT5 prompt-encoder kernels (lcv_gather_rows, lcv_t5_rmsnorm, lcv_geglu_tanh_fwd, lcv_t5_attention) element by
element against the float64 restatements of tests/kernel_ref.py (the `check_*` functions: each bound and its derivation sit
next to the assert there), at the shapes where they go wrong: a second grid-stride pass, clamped ids, C off 512, a row tail,
strided views, saturation; for the attention S = 1 / 63 / 64 / 65 / 512, masks with holes, a single valid key and a batch
row without any.  The attention's scores are made exact (see `_attn_inputs`), so that what remains to bound is the fp32
softmax, the rounding of the probabilities and the PV sum; a CPU test proves the exactness.
Conventions of tests/test_gpu_kernel_edges.py: `lib.call` with caller-owned buffers, outputs NaN-filled, every input a view
into a larger buffer whose guard rows and pad columns hold NaN, so that a read one element off shows up as a NaN.
"""
import functools

import pytest
import torch

import kernel_ref as K
from edge_buffers import (BF16, DEV, F32, GUARD, NAN, call as _call, f32, gen as _gen, guarded as _guarded,
                          nan_out as _nan_out, only_written as _only_written, ptr as _p)

gpu = pytest.mark.gpu    # per test: the file also holds the CPU proof that the attention cases' scores are exact

EPS = f32(1e-6)


# ---------------------------------------------------------------------------------------------------- lcv_gather_rows
@gpu
@pytest.mark.parametrize("n,C", [
    (16133, 520),            # 65 packets per row: 1 048 645 packets, past the cap; the last pass is a tail
    (3, 8),                  # one packet per row
])
def test_gather_rows_past_the_block_cap_with_clamped_ids(n, C):
    vocab = 37
    table = _guarded(vocab, C, C, seed=401)              # a slice of a larger buffer: the rows around it hold NaN
    ids = torch.randint(0, vocab, (n,), generator=_gen(402), device=DEV)
    ids[0], ids[n - 1] = -1, vocab                       # clamped to rows 0 and vocab - 1, never read past the table
    if n > 4:
        ids[n // 2], ids[n // 2 + 1] = vocab + 5, -7
    buf, out = _nan_out(n, C)
    _call("lcv_gather_rows", _p(table), _p(ids), _p(out), n, C, vocab)
    K.assert_bits(out, table[ids.clamp(0, vocab - 1)], what=f"gather_rows n={n} C={C}")       # rule 2
    _only_written(buf, n * C, "gather_rows")


# ----------------------------------------------------------------------------------------------------- lcv_t5_rmsnorm
@gpu
@pytest.mark.parametrize("C", [8, 520, 4096])            # one live lane; a second chunk of one lane; all 8 chunks
@pytest.mark.parametrize("rows", [1, 5])                 # three idle waves; a second workgroup of one row
def test_t5_rmsnorm_edges(rows, C):
    x = _guarded(rows, C, C, seed=411, scale=3.0)
    x[rows - 1] *= 1e-3                                   # mean(x^2) ~ 1e-5: eps = 1e-6 matters
    w = _guarded(1, C, C, seed=412, scale=0.3)[0].add_(1.0)
    buf, y = _nan_out(rows, C)
    _call("lcv_t5_rmsnorm", _p(x), _p(w), _p(y), rows, C, EPS)
    K.check_t5_rmsnorm(y, x, w, EPS, f"t5_rmsnorm rows={rows} C={C}")
    _only_written(buf, rows * C, "t5_rmsnorm")


@gpu
def test_t5_rmsnorm_rejects_c_4104():
    from lcv_hip.lib import LcvError
    x, w = _guarded(2, 4104, 4104, seed=413), _guarded(1, 4104, 4104, seed=414)
    buf, y = _nan_out(2, 4104)
    with pytest.raises(LcvError) as e:
        _call("lcv_t5_rmsnorm", _p(x), _p(w), _p(y), 2, 4104, EPS)
    assert e.value.code == -1
    torch.cuda.synchronize()
    assert torch.isnan(buf.float()).all()


# ------------------------------------------------------------------------------------------------- lcv_geglu_tanh_fwd
@gpu
@pytest.mark.parametrize("rows,F", [
    (16133, 520),            # 1 048 645 packets: a second grid-stride pass with a tail
    (3, 8),
])
def test_geglu_tanh_fwd_on_views_into_one_buffer_past_the_block_cap_and_in_saturation(rows, F):
    ld = 2 * F + 8
    gu = _guarded(rows, 2 * F, ld, seed=421, scale=2.0)
    gate, up = gu[:, :F], gu[:, F:]                      # ld_in = 2F + 8 != F
    # every third gate value spread over [-30, 30]: tanh saturates to +-1 in fp32 past |g| ~ 4
    sat = (torch.rand(rows, (F + 2) // 3, generator=_gen(422), device=DEV) * 60.0 - 30.0).to(BF16)
    gate[:, ::3] = sat
    gate[0, 0], gate[rows - 1, F - 1] = 30.0, -30.0
    buf, out = _nan_out(rows, F)
    _call("lcv_geglu_tanh_fwd", _p(gate), _p(up), _p(out), rows, F, ld)
    K.check_geglu_tanh(out, gate, up, f"geglu_tanh_fwd rows={rows} F={F}")
    _only_written(buf, rows * F, "geglu_tanh_fwd")


# --------------------------------------------------------------------------------------------------- lcv_t5_attention
# Exact scores: q and k take values in {-1/4, 0, 1/4}, so q.k is a multiple of 1/16 of magnitude <= 4 in ANY summation order
# (exact in fp32, and in bf16: at most 64 steps of 1/16); the biases are multiples of 1/16 of magnitude <= 4, so score + bias
# is a multiple of 1/16 of magnitude <= 8: 128 steps, 8 significant bits, exact in bf16.  bf16(bf16(q.k) + bias) is then the
# same number in the kernel and in float64.  The bias depends on the head AND the signed distance, and on its sign:
# ((7 d + 13 h) mod 129 - 64) / 16.
_AT_H, _AT_B = 3, 2
_MASKS = ("prefix", "holes", "last", "none")
_AT_CASES = [
    # S, batch 0's mask, batch 1's mask
    (1, "last", "none"),         # one key; batch 1 has none: exact zeros
    (63, "prefix", "holes"),     # one lane short of a wave
    (64, "holes", "last"),       # exactly one 64-key block
    (65, "last", "prefix"),      # a second block with one key (the only valid one of batch 0), a second query tile of one row
    (512, "holes", "none"),      # the largest S; a fully masked batch row
    (512, "prefix", "holes"),
]


def _mask(kind, S, g):
    m = torch.zeros(S, dtype=torch.int32)
    if kind == "prefix":
        m[: max(1, (2 * S) // 3)] = 1
    elif kind == "holes":
        m[:] = (torch.rand(S, generator=g) < 0.6).to(torch.int32)
        m[S // 2] = 1
        if S > 2:
            m[S // 3] = 0
    elif kind == "last":
        m[S - 1] = 1
    return m


@functools.lru_cache(maxsize=None)
def _attn_inputs(S, m0, m1):
    """CPU tensors: q, k, v [B, S, H, 64] bf16, bias [H, 2S - 1] fp32, mask [B, S] int32."""
    g = torch.Generator().manual_seed(4300 + S)
    q, k = (((torch.randint(-1, 2, (_AT_B, S, _AT_H, 64), generator=g)).to(torch.float32) / 4).to(BF16) for _ in range(2))
    v = torch.randn(_AT_B, S, _AT_H, 64, generator=g).to(BF16)
    d = torch.arange(-(S - 1), S)                                          # signed distance key - query
    h = torch.arange(_AT_H)
    bias = (((7 * d[None, :] + 13 * h[:, None]) % 129) - 64).to(torch.float32) / 16
    mask = torch.stack([_mask(m0, S, g), _mask(m1, S, g)])
    return q, k, v, bias, mask


@pytest.mark.parametrize("S,m0,m1", _AT_CASES)
def test_attention_cases_have_exactly_representable_scores(S, m0, m1):
    """CPU: the claim the GPU test's bound rests on."""
    q, k, v, bias, mask = _attn_inputs(S, m0, m1)
    for t in (q, k):
        assert set((t.double() * 4).unique().tolist()) <= {-1.0, 0.0, 1.0}
    qk = torch.einsum("bihd,bjhd->bhij", q.double(), k.double())
    # any partial sum in any order is a multiple of 1/16 bounded by sum |q||k| <= 4: exact in fp32 and in bf16
    assert torch.equal(qk * 16, (qk * 16).round()) and qk.abs().max() <= 4
    assert torch.equal(qk.to(BF16).double(), qk)
    assert torch.equal(bias.double() * 16, (bias.double() * 16).round()) and bias.abs().max() <= 4
    i = torch.arange(S)
    sc = qk + bias.double()[:, i[None, :] - i[:, None] + S - 1][None]
    assert sc.abs().max() <= 8 and torch.equal(sc.to(BF16).double(), sc) and torch.equal(sc.float().double(), sc)
    # the bias tells heads, distances and the sign of the distance apart
    if S > 1:
        assert not torch.equal(bias[0], bias[1]) and not torch.equal(bias, bias.flip(1)) and (bias[:, 1:] != bias[:, :-1]).all()
    # the masks are what the case names say, and differ between the batch rows
    want = {"prefix": lambda m: m[0] == 1 and m.sum() < max(S, 2) and (m.diff() <= 0).all(),
            "holes": lambda m: m.sum() >= 1 and (S < 3 or ((m.diff() != 0).sum() >= 2)),
            "last": lambda m: m.sum() == 1 and m[-1] == 1, "none": lambda m: m.sum() == 0}
    assert want[m0](mask[0]) and want[m1](mask[1]) and (S == 1 or not torch.equal(mask[0], mask[1]))


@gpu
@pytest.mark.parametrize("S,m0,m1", _AT_CASES)
def test_t5_attention_edges(S, m0, m1):
    q, k, v, bias, mask = (t.to(DEV) for t in _attn_inputs(S, m0, m1))
    H, B = _AT_H, _AT_B
    inner = H * 64
    ld = 3 * inner + 8                                    # q | k | v column blocks of one projection, 8 pad columns
    qkv = torch.full((B * S + 2 * GUARD, ld), NAN, dtype=BF16, device=DEV)
    rows = qkv[GUARD: GUARD + B * S].view(B, S, ld)
    rows[..., :inner], rows[..., inner: 2 * inner], rows[..., 2 * inner: 3 * inner] = (t.reshape(B, S, inner) for t in (q, k, v))
    bb = torch.full((H + 2, 2 * S - 1), NAN, dtype=F32, device=DEV)       # guard rows around the bias table
    bb[1: 1 + H] = bias
    mb = torch.full((B + 2, S), 1, dtype=torch.int32, device=DEV)         # a read outside the mask finds "attend"
    mb[1: 1 + B] = mask
    ld_o = inner + 8
    buf = torch.full((B * S + 2 * GUARD, ld_o), NAN, dtype=BF16, device=DEV)
    out = buf[GUARD: GUARD + B * S].view(B, S, ld_o)[..., :inner]
    base = rows.data_ptr()
    _call("lcv_t5_attention", base, base + inner * 2, base + 2 * inner * 2, _p(out), bb[1:].data_ptr(), mb[1:].data_ptr(),
          B, S, H, ld, ld_o, S * ld, S * ld_o)
    got = out.reshape(B, S, H, 64)
    K.check_t5_attention(got, q, k, v, bias, mask, f"t5_attention S={S} masks={m0}/{m1}")
    _only_written(buf, B * S * inner, "t5_attention")
    for b, kind in enumerate((m0, m1)):
        if kind == "none":                                # the kernel's `sum > 0 ? 1 / sum : 0` contract: exact zeros
            assert (got[b].view(torch.int16) == 0).all(), "a fully masked batch row must give exact +0"


@gpu
def test_t5_attention_rejects_s_513():
    from lcv_hip.lib import LcvError
    S, H = 513, 1
    qkv = torch.zeros(S, 3 * 64, dtype=BF16, device=DEV)
    out = torch.full((S, 64), NAN, dtype=BF16, device=DEV)
    bias = torch.zeros(H, 2 * S - 1, dtype=F32, device=DEV)
    mask = torch.ones(1, S, dtype=torch.int32, device=DEV)
    with pytest.raises(LcvError) as e:
        _call("lcv_t5_attention", qkv.data_ptr(), qkv.data_ptr() + 128, qkv.data_ptr() + 256, _p(out), _p(bias), _p(mask),
              1, S, H, 192, 64, S * 192, S * 64)
    assert e.value.code == -1
    torch.cuda.synchronize()
    assert torch.isnan(out.float()).all()

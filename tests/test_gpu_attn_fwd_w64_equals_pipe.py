"""GPU: the 64-rows-per-wave forward (attn_fwd_w64.hip) and the two-waves-per-SIMD forward (attn_fwd_pipe.hip) give the same
bits.  Both kernels share the operand maps, the exp2 of every score and the bf16 packing; the w64 kernel sums each query
block's row of P in the pipe kernel's order (ex[0] + ex[1] + ... + ex[31], then l_run += that), so O and the LSE must agree
exactly.  Any race or misplaced filler in the w64 gap table shows up here as a difference, not as a tolerance."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16


def _randn(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(BF16)


@pytest.mark.parametrize("B,H,Nq,Nk", [(1, 2, 600, 700), (2, 3, 257, 577), (1, 1, 64, 1024), (1, 2, 333, 641),
                                       (2, 1, 96, 3000), (1, 1, 130, 513), (1, 2, 65, 576), (1, 1, 256, 832),
                                       (1, 2, 1024, 14400), (1, 1, 512, 46800)])
def test_w64_forward_equals_the_two_wave_forward_bit_for_bit(B, H, Nq, Nk, monkeypatch):
    from lcv_hip import lib as L
    from lcv_hip import ops
    D = 128
    c = ops.log2_qscale(D ** -0.5)
    q = (_randn(B, Nq, H, D, seed=41).float() * c).to(BF16).cuda()
    k = _randn(B, Nk, H, D, seed=42)
    k[0, Nk // 3] *= 7.0                      # a running-max jump for every query: the rescale path runs
    k = k.cuda()
    v = _randn(B, Nk, H, D, seed=43).cuda()
    monkeypatch.delenv("LCV_ATTN_FWD_W64", raising=False)
    o, lse = ops.attention(q, k, v, ops.LN2, need_lse=True)
    assert L.load().lcv_attn_fwd_last_kernel().decode() == "attn_fwd_w64_kernel"
    monkeypatch.setenv("LCV_ATTN_FWD_W64", "0")
    o_pipe, lse_pipe = ops.attention(q, k, v, ops.LN2, need_lse=True)
    assert L.load().lcv_attn_fwd_last_kernel().decode() == "attn_fwd_pipe_kernel"
    assert torch.equal(o, o_pipe), (o.float() - o_pipe.float()).abs().max().item()
    assert torch.equal(lse, lse_pipe), (lse - lse_pipe).abs().max().item()

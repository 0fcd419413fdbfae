"""GPU: the level phase-2 gap table of attn_fwd_w64.hip (row-max chains, the half exchange as three table entries and the
ballots in the tail of the phase) against the two-waves-per-SIMD forward (attn_fwd_pipe.hip, LCV_ATTN_FWD_W64=0), bit for bit
on O and the LSE, as in tests/test_gpu_attn_fwd_w64_equals_pipe.py.

The rescale decision is what the moved entries compute, so the inputs force it inside the steady loop: one key of tile 5 (an
odd tile: its row max is taken in an even iteration) and one key of tile 8 (an even tile) point along a direction `u` that
every query has a component of, the second further than the first, so the running max of every row jumps twice by more than
the rescale threshold.  In the one-block cases `u` is projected out of the other query block's 32 rows of every wave: the
ballot of one block fires and the other's does not."""
import pytest
import torch

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
D = 128
ALPHA = 4.0                  # q . u of a jumping row (before the log2 scale)
JUMPS = ((5, 17, 60.0), (8, 41, 150.0))   # (tile, key inside the tile, length along u): scores of about 30 and 76 in log2 units


def _randn(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g)


def _inputs(B, H, Nq, Nk, only_block):
    from lcv_hip import ops
    u = _randn(D, seed=40)
    u = u / u.norm()
    q = _randn(B, Nq, H, D, seed=41)
    q = q - (q @ u).unsqueeze(-1) * u                         # no component along u ...
    block = (torch.arange(Nq) % 64) // 32                     # ... but in the rows that jump: query block of the row inside its wave
    jumps = torch.ones(Nq, dtype=torch.bool) if only_block is None else block == only_block
    q[:, jumps] += ALPHA * u
    q = (q * ops.log2_qscale(D ** -0.5)).to(BF16).cuda()
    k = _randn(B, Nk, H, D, seed=42)
    for tile, key, length in JUMPS:
        k[:, 64 * tile + key] = length * u
    v = _randn(B, Nk, H, D, seed=43)
    return q, k.to(BF16).cuda(), v.to(BF16).cuda()


@pytest.mark.parametrize("B,H,Nq,Nk,only_block", [
    (1, 1, 64, 1024, None),
    (1, 2, 97, 1090, None),       # ragged last tile, even tile count
    (2, 1, 256, 1153, None),      # odd tile count
    (1, 2, 97, 1090, 0),          # the jump fires in query block 0 of a wave only
    (1, 2, 97, 1090, 1),          # ... in query block 1 only
])
def test_w64_level_table_equals_the_two_wave_forward_bit_for_bit(B, H, Nq, Nk, only_block, monkeypatch):
    from lcv_hip import lib as L
    from lcv_hip import ops
    q, k, v = _inputs(B, H, Nq, Nk, only_block)
    monkeypatch.delenv("LCV_ATTN_FWD_W64", raising=False)
    o, lse = ops.attention(q, k, v, ops.LN2, need_lse=True)
    assert L.load().lcv_attn_fwd_last_kernel().decode() == "attn_fwd_w64_kernel"
    monkeypatch.setenv("LCV_ATTN_FWD_W64", "0")
    o_pipe, lse_pipe = ops.attention(q, k, v, ops.LN2, need_lse=True)
    assert L.load().lcv_attn_fwd_last_kernel().decode() == "attn_fwd_pipe_kernel"
    assert torch.isfinite(lse_pipe).all()
    assert torch.equal(o, o_pipe), (o.float() - o_pipe.float()).abs().max().item()
    assert torch.equal(lse, lse_pipe), (lse - lse_pipe).abs().max().item()
    # the jumps happened: the jumping rows' LSE sits at the second key's score, the other rows' far below it
    top = JUMPS[1][2] * ALPHA * D ** -0.5
    rows = torch.arange(Nq) % 64 // 32
    for blk in (0, 1):
        got = lse[..., (rows == blk).cuda()].float()
        if only_block is None or only_block == blk:
            assert (got > 0.9 * top).all()
        else:
            assert (got < 0.25 * top).all()

"""GPU: attn_fwd_w64_kernel against attn_fwd_pipe_kernel, bit for bit, at the edges of its pipeline (the small companion of
tests/test_gpu_attn_fwd_w64_equals_pipe.py, which holds the large shapes).

Nk = 576, 640, 700, 1 088 are 9, 10, 11 (ragged) and 17 key tiles: the steady two-iteration loop is entered and left on both
parities, with and without the single non-steady iteration behind it, and the last tile is full or ragged.  For every tile
j = 1 .. nt - 1 one case plants a key in tile j whose score is more than 2^6 above the running max of SOME rows (and far below
it for others), so the rescale of O, l and the pending score tile runs at every position of the pipeline.  H = 8 is the
model's head count per XCD group (the block remap needs 8 query blocks as well: the Nq = 2 048 case), H = 4 never remaps.
Two layouts: K and V as slices of one tensor (k_sn == v_sn, the model's) and V inside a wider tensor of its own (k_sn != v_sn).
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
D = 128
SHAPES = [(8, nq, nk) for nq in (64, 300) for nk in (576, 640, 700, 1088)] + [(4, 300, 700)]
CASES = [(h, nq, nk, j) for (h, nq, nk) in SHAPES for j in range(1, (nk + 63) // 64)]


@functools.lru_cache(maxsize=None)
def _base(H, Nq, Nk):
    """q (log2 units), k, v on the CPU, and one unit direction per head; never modified."""
    from lcv_hip import ops
    g = torch.Generator().manual_seed(1000 * H + Nq + Nk)
    q = (torch.randn(1, Nq, H, D, generator=g) * ops.log2_qscale(D ** -0.5)).to(BF16)
    k = torch.randn(1, Nk, H, D, generator=g).to(BF16)
    v = torch.randn(1, Nk, H, D, generator=g).to(BF16)
    u = torch.nn.functional.normalize(torch.randn(H, D, generator=g), dim=-1)
    return q, k, v, u


def _both(q, k, v, monkeypatch):
    from lcv_hip import lib as L
    from lcv_hip import ops
    monkeypatch.delenv("LCV_ATTN_FWD_W64", raising=False)
    o, lse = ops.attention(q, k, v, ops.LN2, need_lse=True)
    assert L.load().lcv_attn_fwd_last_kernel().decode() == "attn_fwd_w64_kernel"
    monkeypatch.setenv("LCV_ATTN_FWD_W64", "0")
    o_pipe, lse_pipe = ops.attention(q, k, v, ops.LN2, need_lse=True)
    assert L.load().lcv_attn_fwd_last_kernel().decode() == "attn_fwd_pipe_kernel"
    assert torch.isfinite(lse).all()
    assert torch.equal(o, o_pipe), (o.float() - o_pipe.float()).abs().max().item()
    assert torch.equal(lse, lse_pipe), (lse - lse_pipe).abs().max().item()


def _planted(H, Nq, Nk, j):
    """k with one key of tile j along u: a row's score there is 600 (q . u), q . u ~ N(0, 0.1275): about a fifth of the rows get
    more than 2^6 above anything they saw before (random scores stay under ~8), about half get a large negative score."""
    q, k, v, u = _base(H, Nq, Nk)
    k = k.clone()
    k[0, 64 * j + 5] = (600.0 * u).to(BF16)
    s = (q[0].float() * (600.0 * u).to(BF16).float()).sum(-1)            # [Nq, H]
    assert (s > 80).any() and (s < 0).any()                                # some rows rescale, not all
    return q, k, v


def _shared_kv(k, v):
    kv = torch.stack([k, v], dim=2).cuda()                                 # [B, Nk, 2, H, D]: the model's layout
    return kv[:, :, 0], kv[:, :, 1]


@pytest.mark.parametrize("H,Nq,Nk,j", CASES)
def test_rescale_in_tile_j_shared_strides(H, Nq, Nk, j, monkeypatch):
    q, k, v = _planted(H, Nq, Nk, j)
    ks, vs = _shared_kv(k, v)
    assert ks.stride(1) == vs.stride(1)
    _both(q.cuda(), ks, vs, monkeypatch)


@pytest.mark.parametrize("H,Nq,Nk", SHAPES)
def test_plain_scores_shared_strides(H, Nq, Nk, monkeypatch):
    q, k, v, _ = _base(H, Nq, Nk)
    ks, vs = _shared_kv(k, v)
    _both(q.cuda(), ks, vs, monkeypatch)


@pytest.mark.parametrize("H,Nq,Nk,j", [(8, 300, 700, 3), (8, 64, 1088, 16), (4, 300, 700, 10), (8, 300, 576, 8)])
def test_rescale_in_tile_j_separate_strides(H, Nq, Nk, j, monkeypatch):
    q, k, v = _planted(H, Nq, Nk, j)
    wide = torch.zeros(1, Nk, H, 2 * D, dtype=BF16)
    wide[..., :D] = v
    vs = wide.cuda()[..., :D]
    kc = k.cuda()
    assert kc.stride(1) != vs.stride(1)
    _both(q.cuda(), kc, vs, monkeypatch)


def test_block_remap_on(monkeypatch):
    """B H = 8 and 8 query blocks: the head-per-XCD block order is in force (attn_grid)."""
    q, k, v = _planted(8, 300, 640, 4)
    g = torch.Generator().manual_seed(7)
    from lcv_hip import ops
    q = (torch.randn(1, 2048, 8, D, generator=g) * ops.log2_qscale(D ** -0.5)).to(BF16)
    ks, vs = _shared_kv(k, v)
    _both(q.cuda(), ks, vs, monkeypatch)

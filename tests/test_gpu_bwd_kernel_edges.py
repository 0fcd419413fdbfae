"""GPU: lcv_linear_f32_smallm_bwd, lcv_swiglu_bwd, lcv_swiglu_bwd_interleaved and lcv_qknorm_rope_fwd / _bwd element by element
against the float64 restatements of tests/kernel_ref.py (the `check_*` functions: each bound and its derivation sit next to
the assert there), at the shapes where they go wrong: M around the 16-row launches and N around the 256-row slabs of
smallm_bwd; a second grid-stride pass, strided views and saturation for SwiGLU; head counts off a multiple of 4 (a partial
wave) and of 16 (a partial pass), q-only / k-only, no RoPE, a position offset and packed strides for the q/k norm.
Conventions of tests/test_gpu_kernel_edges.py: `lib.call` with caller-owned buffers, outputs NaN-filled, every input a view
into a larger buffer whose guard rows and pad columns hold NaN, so that a read one element off shows up as a NaN.
"""
import pytest
import torch

import kernel_ref as K
from edge_buffers import (BF16, CAP, DEV, F32, GUARD, NAN, call as _call, f32, gen as _gen, guarded as _guarded,
                          nan_out as _nan_out, only_written as _only_written, ptr as _p)

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------------------------------- lcv_linear_f32_smallm_bwd
@pytest.mark.parametrize("M,N,K_,act", [
    (1, 1, 2, 0),            # one row, one slab of one weight row, one live thread
    (17, 1, 2, 1),           # a second launch of one row; SiLU'
    (16, 255, 514, 1),       # exactly one launch; a slab one row short; K one pair past the 512 columns of a pass
    (17, 257, 1026, 1),      # a second slab of one row; a third K pass of one pair
    (33, 257, 514, 0),       # three launches, the last of one row; no activation
    (33, 255, 1026, 1),
])
def test_linear_f32_smallm_bwd_edges(M, N, K_, act):
    dy = _guarded(M, N, N, seed=201, dtype=F32)
    w = _guarded(N, K_, K_, seed=202, scale=0.5)
    a = _guarded(M, K_, K_, seed=203, scale=2.0, dtype=F32)
    buf, da = _nan_out(M, K_, F32)                      # zero-filled by the entry point itself, then accumulated into
    _call("lcv_linear_f32_smallm_bwd", _p(dy), _p(w), _p(a), _p(da), M, N, K_, act)
    K.check_linear_f32_smallm_bwd(da, dy, w, a, act, f"smallm_bwd M={M} N={N} K={K_} act={act}")
    _only_written(buf, M * K_, "smallm_bwd")


# -------------------------------------------------------------------- lcv_swiglu_bwd, lcv_swiglu_bwd_interleaved
def _saturate(g, seed):
    """Every 5th gate value becomes one of +-30, +-100 (exact in bf16): sigmoid within 1e-13 of 0 or 1, __expf overflowing."""
    vals = torch.tensor([30.0, -30.0, 100.0, -100.0], device=DEV)
    pick = torch.randint(0, 4, (g.shape[0], (g.shape[1] + 4) // 5), generator=_gen(seed), device=DEV)
    g[:, ::5] = vals[pick].to(BF16)


def test_swiglu_bwd_on_views_into_one_buffer_past_the_block_cap_and_in_saturation():
    F = 8
    rows = CAP + 1                                      # one packet per row: one packet past the cap
    gu = _guarded(rows, 2 * F, 2 * F + 8, seed=211, scale=2.0)
    gate, up = gu[:, :F], gu[:, F:]                     # views into one [rows, 2F + 8] buffer: ld_in = 2F + 8
    _saturate(gate, 212)
    dout = _guarded(rows, F, F, seed=213)
    bg, dgate = _nan_out(rows, F)
    bu, dup = _nan_out(rows, F)
    _call("lcv_swiglu_bwd", _p(gate), _p(up), _p(dout), _p(dgate), _p(dup), rows, F, 2 * F + 8)
    K.check_swiglu_bwd(dgate, dup, gate, up, dout, "swiglu_bwd")
    _only_written(bg, rows * F, "swiglu_bwd dgate")
    _only_written(bu, rows * F, "swiglu_bwd dup")


@pytest.mark.parametrize("rows,F", [
    (5, 32),                 # one 64-column group per row
    (5, 96),                 # three groups: the (c >> 5) * 64 + (c & 31) map beyond its first group
    (CAP // 4 + 1, 32),      # four packets per row: four packets past the cap
])
def test_swiglu_bwd_interleaved_edges_and_equals_swiglu_bwd_bitwise(rows, F):
    gu = _guarded(rows, 2 * F, 2 * F, seed=221, scale=2.0)
    gi, ui = K.swiglu_il_index(F, DEV)
    sat = gu[:, gi]
    _saturate(sat, 222)
    gu[:, gi] = sat
    dout = _guarded(rows, F, F, seed=223)
    buf, dgu = _nan_out(rows, 2 * F)
    _call("lcv_swiglu_bwd_interleaved", _p(gu), _p(dout), _p(dgu), rows, F)
    # the same float64 bounds on the de-interleaved result ...
    K.check_swiglu_bwd(dgu[:, gi], dgu[:, ui], gu[:, gi], gu[:, ui], dout, f"swiglu_bwd_interleaved F={F}")
    _only_written(buf, rows * 2 * F, "swiglu_bwd_interleaved")
    # ... and the same bits as lcv_swiglu_bwd on the de-interleaved operands (at F = 32 they are views of gu with ld_in = 64;
    # beyond, contiguous copies)
    if F == 32:
        gate, up, ld = gu[:, :32], gu[:, 32:], 64
    else:
        gate, up, ld = gu[:, gi].contiguous(), gu[:, ui].contiguous(), F
    _, dgate = _nan_out(rows, F)
    _, dup = _nan_out(rows, F)
    _call("lcv_swiglu_bwd", _p(gate), _p(up), _p(dout), _p(dgate), _p(dup), rows, F, ld)
    K.assert_bits(dgu[:, gi], dgate, what=f"swiglu_bwd_interleaved F={F}: dgate vs lcv_swiglu_bwd")
    K.assert_bits(dgu[:, ui], dup, what=f"swiglu_bwd_interleaved F={F}: dup vs lcv_swiglu_bwd")


# ------------------------------------------------------------------------------- lcv_qknorm_rope_fwd, lcv_qknorm_rope_bwd
D = 128
_B, _N = 2, 3
_EPS = f32(1e-6)                                   # the fp32 value the kernel receives
_QS = 261 / 2048                                    # ~ 128^-0.5 log2(e), exact in fp32
# H, which of q / k, RoPE, packed q|k|v input, q_scale, pos_off, v_out given
_QK_CASES = [
    (1, "qk", True, True, _QS, 2, True),         # a quarter wave; packed; q_scale ~ 128^-0.5 log2(e); offset into the table
    (5, "q", False, False, 1.0, 0, False),       # a partial second wave; q only; no RoPE (cross-attention); separate buffers
    (5, "k", True, False, 1.0, 3, False),        # k only
    (17, "qk", True, True, _QS, 1, True),        # a second pass of one head
    (17, "qk", False, False, 2.0, 0, True),      # no RoPE on two passes, separate buffers
]


def _tokens(width, ld, seed, scale=1.0, fill=True):
    """[B, N, width] view (token stride ld, batch stride N * ld) in a NaN buffer with GUARD token rows on either side."""
    buf = torch.full((_B * _N + 2 * GUARD, ld), NAN, dtype=BF16, device=DEV)
    view = buf[GUARD: GUARD + _B * _N].view(_B, _N, ld)[:, :, :width]
    if fill:
        view.copy_((torch.randn(_B, _N, width, generator=_gen(seed), device=DEV) * scale).to(BF16))
    return buf, view


def _qk_setup(H, which, rope, packed, pos_off):
    HD = H * D
    if packed:
        ld = 3 * HD + 8
        _, qkv = _tokens(3 * HD, ld, 301, 1.5)
        q, k, v = qkv[..., :HD], qkv[..., HD: 2 * HD], qkv[..., 2 * HD:]
    else:
        ld = HD + 8
        q, k, v = (_tokens(HD, ld, 301 + i, 1.5)[1] for i in range(3))
    # per-head magnitudes from 1e-3 to 30: r spans 3e-2 .. 1e3
    mag = torch.logspace(-3, 1.5, H, device=DEV).repeat_interleave(D)
    q.mul_(mag.to(BF16)); k.mul_(mag.flip(0).to(BF16))
    wq = _guarded(1, D, D, seed=305, scale=0.2)[0].add_(1.0)
    wk = _guarded(1, D, D, seed=306, scale=0.2)[0].add_(1.0)
    cs = None
    if rope:
        # the table is longer than pos_off + N; rows no token of this call addresses hold NaN
        cs = torch.full((pos_off + _N + 2, D // 2, 2), NAN, dtype=F32, device=DEV)
        th = torch.rand(_N, D // 2, generator=_gen(307), device=DEV, dtype=torch.float64) * 6.2832
        cs[pos_off: pos_off + _N, :, 0] = torch.cos(th).float()
        cs[pos_off: pos_off + _N, :, 1] = torch.sin(th).float()
    return dict(q=q if "q" in which else None, k=k if "k" in which else None, v=v, wq=wq, wk=wk, cs=cs, in_sn=ld, in_sb=_N * ld)


def _heads(t, H):
    return t.reshape(_B, _N, H, D)


@pytest.mark.parametrize("H,which,rope,packed,qs,pos_off,copy_v", _QK_CASES)
def test_qknorm_rope_fwd_edges(H, which, rope, packed, qs, pos_off, copy_v):
    HD = H * D
    s = _qk_setup(H, which, rope, packed, pos_off)
    q_sn, kv_sn = HD + 16, HD + 24
    bq, q_out = _tokens(HD, q_sn, 0, fill=False)
    bk, k_out = _tokens(HD, kv_sn, 0, fill=False)
    bv, v_out = _tokens(HD, kv_sn, 0, fill=False)
    _call("lcv_qknorm_rope_fwd", _p(s["q"]), _p(s["k"]), _p(s["v"]), _p(q_out) if s["q"] is not None else None,
          _p(k_out) if s["k"] is not None else None, _p(v_out) if copy_v else None, _p(s["wq"]), _p(s["wk"]), _p(s["cs"]),
          _B, _N, H, s["in_sb"], s["in_sn"], _N * q_sn, q_sn, _N * kv_sn, kv_sn, pos_off, _EPS, qs)
    rows = None if s["cs"] is None else s["cs"][pos_off: pos_off + _N]
    tag = f"qknorm_rope_fwd H={H} {which} rope={rope}"
    for x, out, buf, w, scale, name in ((s["q"], q_out, bq, s["wq"], qs, "q"), (s["k"], k_out, bk, s["wk"], 1.0, "k")):
        if x is None:
            assert torch.isnan(buf.float()).all(), f"{tag}: {name}_out written without {name}_in"
            continue
        K.check_qknorm_rope_fwd(_heads(out, H), _heads(x, H), w, rows, _EPS, scale, f"{tag} {name}")
        _only_written(buf, _B * _N * HD, f"{tag} {name}_out")
    if copy_v:
        K.assert_bits(v_out.contiguous(), s["v"].contiguous(), what=f"{tag}: v copy")
        _only_written(bv, _B * _N * HD, f"{tag} v_out")
    else:
        assert torch.isnan(bv.float()).all()


def test_qknorm_rope_fwd_leaves_v_alone_when_v_out_is_v_in():
    """v_out == v_in (the packed buffer normalised in place) skips the copy.  k_out shares v_out's strides, so it is given the
    packed buffer's token and batch strides too."""
    H, pos_off = 5, 1
    HD = H * D
    s = _qk_setup(H, "qk", True, True, pos_off)
    v0 = s["v"].clone()
    q_sn, kv_sn = HD + 16, s["in_sn"]
    bq, q_out = _tokens(HD, q_sn, 0, fill=False)
    bk, k_out = _tokens(HD, kv_sn, 0, fill=False)        # token stride in_sn, batch stride N * in_sn: what the call passes
    _call("lcv_qknorm_rope_fwd", _p(s["q"]), _p(s["k"]), _p(s["v"]), _p(q_out), _p(k_out), _p(s["v"]), _p(s["wq"]), _p(s["wk"]),
          _p(s["cs"]), _B, _N, H, s["in_sb"], s["in_sn"], _N * q_sn, q_sn, _N * kv_sn, kv_sn, pos_off, _EPS, 1.0)
    assert _N * kv_sn == s["in_sb"]
    K.assert_bits(s["v"].contiguous(), v0.contiguous(), what="qknorm_rope_fwd v_out == v_in")
    rows = s["cs"][pos_off: pos_off + _N]
    for x, out, buf, w, name in ((s["q"], q_out, bq, s["wq"], "q"), (s["k"], k_out, bk, s["wk"], "k")):
        K.check_qknorm_rope_fwd(_heads(out, H), _heads(x, H), w, rows, _EPS, 1.0, f"qknorm_rope_fwd v_out == v_in: {name}")
        _only_written(buf, _B * _N * HD, f"qknorm_rope_fwd v_out == v_in: {name}_out")


@pytest.mark.parametrize("dw_slots", [0, 1, 3])
@pytest.mark.parametrize("H,which,rope,packed,qs,pos_off,copy_v", _QK_CASES)
def test_qknorm_rope_bwd_edges(H, which, rope, packed, qs, pos_off, copy_v, dw_slots):
    HD = H * D
    s = _qk_setup(H, which, rope, packed, pos_off)
    q_sn, kv_sn = HD + 16, HD + 24
    _, dq_out = _tokens(HD, q_sn, 311)
    _, dk_out = _tokens(HD, kv_sn, 312)
    if packed:                                           # dq | dk | (dv) column blocks of one gradient buffer
        din_sn = 3 * HD + 8
        bd, dqkv = _tokens(3 * HD, din_sn, 0, fill=False)
        dq_in, dk_in, bufs = dqkv[..., :HD], dqkv[..., HD: 2 * HD], [bd]
    else:
        din_sn = HD + 32
        (b0, dq_in), (b1, dk_in) = _tokens(HD, din_sn, 0, fill=False), _tokens(HD, din_sn, 0, fill=False)
        bufs = [b0, b1]
    dwb = torch.full((2, max(dw_slots, 1) + 2 * GUARD, D), 7.5, dtype=F32, device=DEV)     # guard rows hold 7.5
    dw = dwb[:, GUARD: GUARD + max(dw_slots, 1)]
    dw.zero_()                                            # accumulated into by atomics: the caller zero-fills
    has_q, has_k = s["q"] is not None, s["k"] is not None
    _call("lcv_qknorm_rope_bwd", _p(s["q"]), _p(s["k"]), _p(dq_out) if has_q else None, _p(dk_out) if has_k else None,
          _p(dq_in) if has_q else None, _p(dk_in) if has_k else None, _p(s["wq"]), _p(s["wk"]), _p(s["cs"]), _B, _N, H,
          s["in_sb"], s["in_sn"], _N * q_sn, q_sn, _N * kv_sn, kv_sn, _N * din_sn, din_sn, pos_off, _EPS, qs,
          dwb[0, GUARD:].data_ptr() if dw_slots else None, dwb[1, GUARD:].data_ptr() if dw_slots else None, max(dw_slots, 1))
    rows = None if s["cs"] is None else s["cs"][pos_off: pos_off + _N]
    tag = f"qknorm_rope_bwd H={H} {which} rope={rope} slots={dw_slots}"
    written = 0
    for i, (x, dout, din, w, scale, name) in enumerate(((s["q"], dq_out, dq_in, s["wq"], qs, "q"),
                                                         (s["k"], dk_out, dk_in, s["wk"], 1.0, "k"))):
        if x is None:
            assert (dw[i] == 0).all(), f"{tag}: dw{name} written without {name}_in"
            continue
        K.check_qknorm_rope_bwd(_heads(din, H), dw[i] if dw_slots else None, _heads(x, H), _heads(dout, H), w, rows, _EPS, scale,
                                f"{tag} {name}")
        written += _B * _N * HD
    assert sum(int(torch.isnan(b.float()).sum()) for b in bufs) == sum(b.numel() for b in bufs) - written, f"{tag}: stray writes"
    assert (dwb[:, :GUARD] == 7.5).all() and (dwb[:, GUARD + max(dw_slots, 1):] == 7.5).all(), f"{tag}: dw guard rows"
    if not dw_slots:
        assert (dw == 0).all()

"""GPU: the fixed-order entry points of include/lcv_hip_det.h, through the C ABI, against their default counterparts.

For each entry point:
  (a) the data gradients (dx / dy / dq_in / dk_in / nothing for the clip) carry the default entry point's bits;
  (b) five calls give the same bits in every reduced output (the workspace is NaN-filled before the first call: its
      content on entry must not matter);
  (c) the reduced output is no further from the float64 restatement than 1.5 x the default entry point's, plus a floor;
  (d) a workspace one float short is an LcvError.

(c), written out.  Errors are measured in the unit of rule 3 of tests/kernel_ref.py, u * sum|terms| of an output element:
E(out) = max over elements of |out - ref| / sum|terms|.  The check is E(det) <= 1.5 * E(default) + depth * u, the floor
being rule 3 itself (depth * u * sum|terms|) with `depth` the longest chain of additions of the FIXED-ORDER form's own
summation tree, counted from the order written at the top of csrc/reduce_det.hip and stated next to each call.  (A first
version of this file used depth 1 for every kernel; that is not a bound a multi-level fp32 sum can keep - a tree of depth
24 over non-negative terms lands 1.7 u away as easily as 0.3 u - and it was replaced by the rule as kernel_ref states it.)
Both errors are measured in the same test on the same inputs and printed before the assert.
"""
import pytest
import torch

import kernel_ref as K

pytestmark = pytest.mark.gpu

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
DEV = "cuda"
U = K.U
NAN = float("nan")
REPEATS = 5
ADALN, LAYERNORM, GATE, QKNORM, SMALLM, GRAD_NORM = range(6)


def _call(name, *args):
    from lcv_hip import lib
    lib.call(name, *args, torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else t.data_ptr()


def _randn(*shape, seed, scale=1.0, dtype=BF16):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(*shape, generator=g, device=DEV) * scale).to(dtype)


def _ws(kind, d0, d1=0, d2=0):
    """A NaN-filled workspace of exactly the size the library asks for."""
    from lcv_hip import lib
    n = int(lib.load().lcv_det_ws_bytes(kind, d0, d1, d2))
    assert n > 0 and n % 4 == 0
    return torch.full((n // 4,), NAN, dtype=F32, device=DEV), n


def _too_small(fn, ws, n):
    from lcv_hip.lib import LcvError
    with pytest.raises(LcvError):
        fn(ws, n - 4)
    with pytest.raises(LcvError):
        fn(None, 0)


def _same_bits(a, b, what):
    K.assert_bits(a, b, what)


def _check_c(det, dflt, ref, terms_abs, depth, what):
    scale = terms_abs.to(F64).clamp_min(1e-300)
    e_det = float(((det.to(F64) - ref).abs() / scale).max())
    e_def = float(((dflt.to(F64) - ref).abs() / scale).max())
    print(f"{what}: E(det) = {e_det / U:.3f} u, E(default) = {e_def / U:.3f} u, depth {depth}")
    assert torch.isfinite(det).all(), what
    assert e_det <= 1.5 * e_def + depth * U, f"{what}: E(det) {e_det / U:.3f} u > 1.5 * {e_def / U:.3f} u + {depth} u"


def _repeat(fn, outs, what):
    """(b): call `fn` REPEATS times; `outs()` returns the reduced outputs of a call (fresh clones)."""
    first = None
    for i in range(REPEATS):
        fn()
        got = outs()
        if first is None:
            first = got
        else:
            for a, b in zip(first, got):
                _same_bits(b, a, f"{what}: call {i} differs from call 0")
    return first


# ------------------------------------------------------------------------------------------------ AdaLN
SHAPES = [(2, 3, 50, 4096), (2, 3, 50, 128), (2, 3, 50, 520), (1, 1, 1, 4096)]


def _rownorm_depth(rows_per_frame):
    """16 rows per wave of a 64-row workgroup, the 3 adds that join the waves, one add per workgroup of the frame, and the
    add into the output; one more for the product dy * xh folded into the chain."""
    return min(16, -(-rows_per_frame // 4)) + 3 + -(-rows_per_frame // 64) + 1 + 1


def _norm_x(B, N, C, seed):
    return (_randn(B, N, C, seed=seed, scale=0.8, dtype=F32) + 0.3).to(BF16)


@pytest.mark.parametrize("with_dres", [False, True])
@pytest.mark.parametrize("B,T,S,C", SHAPES)
def test_det_adaln_modulate_bwd(B, T, S, C, with_dres):
    eps = 1e-6
    N = T * S
    x, dy = _norm_x(B, N, C, 1), _randn(B, N, C, seed=2)
    dres = _randn(B, N, C, seed=3) if with_dres else None
    ms, sh, sc = 6 * C, 1 * C, 4 * C
    mod = _randn(B, T, ms, seed=4, scale=0.1, dtype=F32)
    dx0 = torch.full_like(x, NAN); dmod0 = torch.zeros_like(mod)
    _call("lcv_adaln_modulate_bwd", _p(x), _p(mod), _p(dy), _p(dx0), _p(dmod0), B, T, S, C, ms, sh, sc, eps, _p(dres))
    ws, n = _ws(ADALN, B * T, S, C)
    dx = torch.full_like(x, NAN); dmod = torch.zeros_like(mod)

    def run(w=ws, nb=n):
        dmod.zero_()
        _call("lcv_det_adaln_modulate_bwd", _p(x), _p(mod), _p(dy), _p(dx), _p(dmod), B, T, S, C, ms, sh, sc, eps, _p(dres), _p(w), nb)

    _repeat(run, lambda: (dmod.clone(), dx.clone()), "det_adaln_modulate_bwd")
    _same_bits(dx, dx0, "det_adaln_modulate_bwd dx vs default")                      # (a)
    keep = torch.ones(ms, dtype=torch.bool, device=DEV); keep[sh: sh + C] = False; keep[sc: sc + C] = False
    assert not dmod[:, :, keep].any()                                                 # only the two chunks are written
    xh, _, _ = K.layernorm_xhat(x, eps)
    dyf = K.f64(dy)
    depth = _rownorm_depth(S)
    for off, terms in ((sh, dyf), (sc, dyf * xh)):                                    # (c)
        t = terms.view(B, T, S, C)
        _check_c(dmod[:, :, off: off + C], dmod0[:, :, off: off + C], t.sum(2), t.abs().sum(2), depth, f"dmod[{off // C}C] C={C} S={S}")
    _too_small(run, ws, n)                                                            # (d)
    # dmod = NULL: the default path, and no workspace is needed
    dx2 = torch.full_like(x, NAN)
    _call("lcv_det_adaln_modulate_bwd", _p(x), _p(mod), _p(dy), _p(dx2), None, B, T, S, C, ms, sh, sc, eps, _p(dres), None, 0)
    dx3 = torch.full_like(x, NAN)
    _call("lcv_adaln_modulate_bwd", _p(x), _p(mod), _p(dy), _p(dx3), None, B, T, S, C, ms, sh, sc, eps, _p(dres))
    _same_bits(dx2, dx3, "det_adaln_modulate_bwd without dmod")


# ------------------------------------------------------------------------------------------------ LayerNorm affine
@pytest.mark.parametrize("with_dres", [False, True])
@pytest.mark.parametrize("rows,C", [(1, 4096), (31, 520), (33, 128), (300, 4096)])
def test_det_layernorm_affine_bwd(rows, C, with_dres):
    eps = 1e-6
    x, dy = _norm_x(1, rows, C, 5)[0], _randn(rows, C, seed=6)
    dres = _randn(rows, C, seed=7) if with_dres else None
    w = 1.0 + _randn(C, seed=8, scale=0.2, dtype=F32)
    dx0 = torch.full_like(x, NAN); dw0 = torch.zeros(C, dtype=F32, device=DEV); db0 = torch.zeros_like(dw0)
    _call("lcv_layernorm_affine_bwd", _p(x), _p(w), _p(dy), _p(dx0), _p(dw0), _p(db0), rows, C, eps, _p(dres))
    ws, n = _ws(LAYERNORM, rows, C)
    dx = torch.full_like(x, NAN); dw = torch.zeros_like(dw0); db = torch.zeros_like(dw0)

    def run(wsp=ws, nb=n):
        dw.zero_(); db.zero_()
        _call("lcv_det_layernorm_affine_bwd", _p(x), _p(w), _p(dy), _p(dx), _p(dw), _p(db), rows, C, eps, _p(dres), _p(wsp), nb)

    _repeat(run, lambda: (dw.clone(), db.clone(), dx.clone()), "det_layernorm_affine_bwd")
    _same_bits(dx, dx0, "det_layernorm_affine_bwd dx vs default")
    xh, _, _ = K.layernorm_xhat(x, eps)
    dyf = K.f64(dy)
    _check_c(db, db0, dyf.sum(0), dyf.abs().sum(0), _rownorm_depth(rows), f"db rows={rows} C={C}")
    _check_c(dw, dw0, (dyf * xh).sum(0), (dyf * xh).abs().sum(0), _rownorm_depth(rows), f"dw rows={rows} C={C}")
    _too_small(run, ws, n)


# ------------------------------------------------------------------------------------------------ gate
@pytest.mark.parametrize("B,T,S,C", SHAPES)
def test_det_gate_residual_bwd(B, T, S, C):
    N = T * S
    y, dout = _randn(B, N, C, seed=9), _randn(B, N, C, seed=10)
    ms, goff = 3 * C + 16, C + 8
    mod = _randn(B, T, ms, seed=11, dtype=F32)
    dy0 = torch.full_like(y, NAN); dmod0 = torch.zeros_like(mod)
    _call("lcv_gate_residual_bwd", _p(y), _p(mod), _p(dout), _p(dy0), _p(dmod0), B, T, S, C, ms, goff)
    ws, n = _ws(GATE, B * T, S, C)
    dy = torch.full_like(y, NAN); dmod = torch.zeros_like(mod)

    def run(w=ws, nb=n):
        dmod.zero_()
        _call("lcv_det_gate_residual_bwd", _p(y), _p(mod), _p(dout), _p(dy), _p(dmod), B, T, S, C, ms, goff, _p(w), nb)

    _repeat(run, lambda: (dmod.clone(), dy.clone()), "det_gate_residual_bwd")
    _same_bits(dy, dy0, "det_gate_residual_bwd dy vs default")
    keep = torch.ones(ms, dtype=torch.bool, device=DEV); keep[goff: goff + C] = False
    assert not dmod[:, :, keep].any()
    prod = (K.f64(dout) * K.f64(y)).view(B, T, S, C)
    depth = min(32, S) + -(-S // 32) + 1            # the thread's fma chain over its 32 rows, the frame's workgroups, the output add
    _check_c(dmod[:, :, goff: goff + C], dmod0[:, :, goff: goff + C], prod.sum(2), prod.abs().sum(2), depth, f"dgate C={C} S={S}")
    _too_small(run, ws, n)


def test_det_gate_residual_bwd_refuses_what_it_does_not_take():
    from lcv_hip.lib import LcvError
    B, T, S, C = 1, 1, 2, 4104                      # C / 8 = 513 > 512: the default form's generic kernel has no counterpart
    y, dout = _randn(B, T * S, C, seed=12), _randn(B, T * S, C, seed=13)
    mod = _randn(B, T, C, seed=14, dtype=F32)
    dy = torch.empty_like(y); dmod = torch.zeros_like(mod)
    ws = torch.empty(1 << 16, dtype=F32, device=DEV)
    with pytest.raises(LcvError, match="4096"):
        _call("lcv_det_gate_residual_bwd", _p(y), _p(mod), _p(dout), _p(dy), _p(dmod), B, T, S, C, C, 0, _p(ws), ws.numel() * 4)


# ------------------------------------------------------------------------------------------------ q/k norm + RoPE
def _qk_restatement(xin, dout, w, cs, pos_off, eps, out_scale):
    """dw[d] = sum over (b, n, h) of rope^T(out_scale * dout)[d] * (x * rsqrt(mean(x^2) + eps))[d], and its sum of magnitudes."""
    x, d = K.f64(xin), K.f64(dout) * out_scale
    B, N, H, D = x.shape
    r = 1.0 / torch.sqrt((x * x).mean(-1, keepdim=True) + eps)
    if cs is not None:
        t = K.f64(cs)[pos_off: pos_off + N].view(1, N, 1, D // 2, 2)
        c, s = t[..., 0], t[..., 1]
        d0, d1 = d.view(B, N, H, D // 2, 2)[..., 0], d.view(B, N, H, D // 2, 2)[..., 1]
        d = torch.stack((d0 * c + d1 * s, d1 * c - d0 * s), dim=-1).view(B, N, H, D)
    terms = d * (x * r)
    return terms.sum((0, 1, 2)), terms.abs().sum((0, 1, 2))


@pytest.mark.parametrize("H,N,B,which,rope,pos_off", [
    (32, 300, 2, "qk", True, 7),     # two passes of 16 heads, more tokens than one first-level group, a batch stride
    (4, 300, 1, "qk", True, 0),      # fewer heads than a pass
    (32, 1, 1, "qk", False, 0),      # one token: one partial row
    (4, 50, 2, "q", True, 0),
    (4, 50, 2, "k", False, 0),
])
def test_det_qknorm_rope_bwd(H, N, B, which, rope, pos_off):
    D, eps, qs = 128, 1e-6, 0.1275
    qkv = _randn(B, N, 3, H, D, seed=15)
    dq_out, dk_out = _randn(B, N, H, D, seed=16), _randn(B, N, H, D, seed=17)
    wq = (1 + 0.1 * _randn(D, seed=18, dtype=F32)).to(BF16); wk = (1 + 0.1 * _randn(D, seed=19, dtype=F32)).to(BF16)
    cs = None
    if rope:
        ang = _randn(pos_off + N, D // 2, seed=20, scale=3.0, dtype=F32)
        cs = torch.stack((ang.cos(), ang.sin()), dim=-1).contiguous()
    has_q, has_k = "q" in which, "k" in which
    q_in, k_in = (qkv[:, :, 0] if has_q else None), (qkv[:, :, 1] if has_k else None)
    dqo, dko = (dq_out if has_q else None), (dk_out if has_k else None)
    ref_t = q_in if has_q else k_in
    go = dqo if has_q else dko
    gk = dko if has_k else dqo

    def args(dqkv, dwq, dwk):
        dqi, dki = (dqkv[:, :, 0] if has_q else None), (dqkv[:, :, 1] if has_k else None)
        gi = dqi if has_q else dki
        return (_p(q_in), _p(k_in), _p(dqo), _p(dko), _p(dqi), _p(dki), _p(wq), _p(wk), _p(cs), B, N, H, ref_t.stride(0),
                ref_t.stride(1), go.stride(0), go.stride(1), gk.stride(0), gk.stride(1), gi.stride(0), gi.stride(1), pos_off,
                eps, qs, _p(dwq), _p(dwk))

    slots = 256
    sq = torch.zeros(slots, D, dtype=F32, device=DEV) if has_q else None
    sk = torch.zeros(slots, D, dtype=F32, device=DEV) if has_k else None
    dqkv0 = torch.full_like(qkv, NAN)
    _call("lcv_qknorm_rope_bwd", *args(dqkv0, sq, sk), slots)
    ws, n = _ws(QKNORM, B, N)
    dqkv = torch.full_like(qkv, NAN)
    dwq = torch.zeros(D, dtype=F32, device=DEV) if has_q else None
    dwk = torch.zeros(D, dtype=F32, device=DEV) if has_k else None

    def run(w=ws, nb=n):
        for t in (dwq, dwk):
            if t is not None:
                t.zero_()
        _call("lcv_det_qknorm_rope_bwd", *args(dqkv, dwq, dwk), _p(w), nb)

    written = [i for i, on in ((0, has_q), (1, has_k)) if on]       # the v slot and an absent side stay NaN: not compared
    _repeat(run, lambda: tuple(t.clone() for t in (dwq, dwk) if t is not None) + tuple(dqkv[:, :, i].clone() for i in written),
            "det_qknorm_rope_bwd")
    # heads per thread, 2 shuffles, 3 adds that join the waves, a first-level group of up to 160 tokens, the groups, the
    # output add; + 2 for the products (rope, d * n) in front of the chain
    depth = -(-H // 16) + 2 + 3 + min(160, B * N) + -(-(B * N) // 160) + 1 + 2
    for idx, on in ((0, has_q), (1, has_k)):
        if on:
            _same_bits(dqkv[:, :, idx], dqkv0[:, :, idx], f"det_qknorm_rope_bwd d{'qk'[idx]}_in vs default")
    if has_q:
        ref, mag = _qk_restatement(q_in, dq_out, wq, cs, pos_off, eps, qs)
        _check_c(dwq, sq.sum(0), ref, mag, depth, f"dwq H={H} N={N} B={B}")
    if has_k:
        ref, mag = _qk_restatement(k_in, dk_out, wk, cs, pos_off, eps, 1.0)
        _check_c(dwk, sk.sum(0), ref, mag, depth, f"dwk H={H} N={N} B={B}")
    _too_small(run, ws, n)


# ------------------------------------------------------------------------------------------------ small-M linear
@pytest.mark.parametrize("act_in", [0, 1])
@pytest.mark.parametrize("K_", [512, 4096])
@pytest.mark.parametrize("N", [300, 256])
@pytest.mark.parametrize("M", [1, 6, 17])
def test_det_linear_f32_smallm_bwd(M, N, K_, act_in):
    a = _randn(M, K_, seed=21, dtype=F32)
    w = _randn(N, K_, seed=22, scale=0.05)
    dy = _randn(M, N, seed=23, dtype=F32)
    da0 = torch.full((M, K_), NAN, dtype=F32, device=DEV)
    _call("lcv_linear_f32_smallm_bwd", _p(dy), _p(w), _p(a), _p(da0), M, N, K_, act_in)
    ws, n = _ws(SMALLM, M, N, K_)
    da = torch.full((M, K_), NAN, dtype=F32, device=DEV)

    def run(wsp=ws, nb=n):
        _call("lcv_det_linear_f32_smallm_bwd", _p(dy), _p(w), _p(a), _p(da), M, N, K_, act_in, _p(wsp), nb)

    _repeat(run, lambda: (da.clone(),), "det_linear_f32_smallm_bwd")
    af = K.f64(a)
    sig = 1.0 / (1.0 + torch.exp(-af))
    dact = sig * (1.0 + af * (1.0 - sig)) if act_in == 1 else torch.ones_like(af)
    ref = (K.f64(dy) @ K.f64(w)) * dact
    mag = (K.f64(dy).abs() @ K.f64(w).abs()) * dact.abs()
    depth = min(256, N) + -(-N // 256) + 2          # a slab's 256-term chain, the slabs, the product and the activation factor
    _check_c(da, da0, ref, mag, depth, f"da M={M} N={N} K={K_} act_in={act_in}")
    _too_small(run, ws, n)


# ------------------------------------------------------------------------------------------------ gradient-norm clip
CHUNK, SLOTS = 2048, 64
BIG = 65 * CHUNK + 3           # more than 64 chunks: the default form has several adders per slot


def _table(grads):
    rows, chunk = [], 0
    for g in grads:
        rows.append([g.data_ptr(), g.data_ptr(), g.data_ptr(), g.data_ptr(), g.numel(), chunk])   # the clip reads grad and numel only
        chunk += (g.numel() + CHUNK - 1) // CHUNK
    return torch.tensor(rows, dtype=torch.int64).to(DEV), chunk


def _clip_restatement(grads, f32, max_norm):
    """torch.nn.utils.clip_grad_norm_ with the rounding points of the foreach path: per-tensor norms and the total in the
    gradients' dtype, the coefficient likewise; float64 inside."""
    def rnd(v):
        return v if f32 else v.to(BF16).to(F64)
    sumsq = torch.stack([(K.f64(g) ** 2).sum() for g in grads])
    total = rnd(torch.sqrt((rnd(torch.sqrt(sumsq)) ** 2).sum()))
    coef = max_norm / (total + 1e-6) if f32 else rnd(max_norm / rnd(total + 1e-6))
    return sumsq, torch.stack((total, coef.clamp(max=1.0)))


def _clip_case(grads, f32, what):
    max_norm = 1.0
    n_t = len(grads)
    desc, chunks = _table(grads)
    pt0 = torch.full((n_t, SLOTS), NAN, dtype=F32, device=DEV); nc0 = torch.full((2,), NAN, dtype=F32, device=DEV)
    _call("lcv_grad_norm_clip", _p(desc), n_t, chunks, 1 if f32 else 0, max_norm, _p(pt0), _p(nc0))
    ws, n = _ws(GRAD_NORM, chunks)
    assert n == 4 * chunks
    pt = torch.full((n_t, SLOTS), NAN, dtype=F32, device=DEV); nc = torch.full((2,), NAN, dtype=F32, device=DEV)

    def run(w=ws, nb=n):
        _call("lcv_det_grad_norm_clip", _p(desc), n_t, chunks, 1 if f32 else 0, max_norm, _p(pt), _p(nc), _p(w), nb)

    _repeat(run, lambda: (nc.clone(), pt.clone()), what)
    assert not pt[:, 1:].any(), f"{what}: slots 1..63 must be zero"
    sumsq, ref_nc = _clip_restatement(grads, f32, max_norm)
    most = max(-(-g.numel() // CHUNK) for g in grads)
    depth = 8 + 6 + 2 + -(-most // 256) + 6 + 2     # the thread's 8 fmas, wave tree, waves; chunks per thread, wave tree, waves
    _check_c(pt[:, 0], pt0.sum(1), sumsq, sumsq, depth, f"{what}: per-tensor sums of squares")
    # norm_coef: the same (c) in fp32 ulps of the restatement (a bf16 total is a bf16 number: usually both are exact)
    ulp = K.fp32_ulp(ref_nc)
    e_det, e_def = (nc.to(F64) - ref_nc).abs() / ulp, (nc0.to(F64) - ref_nc).abs() / ulp
    print(f"{what}: norm_coef {nc.tolist()} default {nc0.tolist()} restatement {ref_nc.tolist()}")
    assert bool((e_det <= 1.5 * e_def + 1.0).all()), f"{what}: norm_coef {nc.tolist()} vs {ref_nc.tolist()} (default {nc0.tolist()})"
    _too_small(run, ws, n)


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("numel", [1, 2047, 2048, 2049, BIG])
def test_det_grad_norm_clip_one_tensor(numel, f32):
    g = _randn(numel, seed=24, dtype=F32 if f32 else BF16)
    _clip_case([g], f32, f"det_grad_norm_clip numel={numel} f32={f32}")


@pytest.mark.parametrize("f32", [False, True])
def test_det_grad_norm_clip_700_tensors(f32):
    sizes = [(1, 2047, 2048, 2049, 77, 4097, 640)[i % 7] for i in range(699)] + [BIG]
    flat = _randn(sum(sizes) + 8 * len(sizes), seed=25, scale=0.05, dtype=F32 if f32 else BF16)
    grads, at = [], 0
    for s in sizes:
        grads.append(flat[at: at + s])
        at += (s + 7) // 8 * 8                      # every tensor starts on a 16-byte (bf16) / 32-byte (fp32) boundary
    _clip_case(grads, f32, f"det_grad_norm_clip 700 tensors f32={f32}")


def test_det_grad_norm_clip_bf16_gradient_at_an_odd_address():
    buf = _randn(8 + 2 * CHUNK + 9, seed=26)
    g = buf[1: 1 + 2 * CHUNK + 5]                   # 2-byte aligned, not 16: the element-wise load path, three chunks
    assert g.data_ptr() % 16 == 2
    _clip_case([g], False, "det_grad_norm_clip misaligned bf16")


def test_joint_clip_over_bf16_and_fp32_optimizers_gives_the_same_total_in_both_modes():
    from lcv_hip import ops
    pb = [torch.nn.Parameter(_randn(s, seed=30 + i)) for i, s in enumerate((300, 4100, 2048))]
    pf = [torch.nn.Parameter(_randn(s, seed=40 + i, dtype=F32)) for i, s in enumerate((5, 6000))]
    for i, p in enumerate(pb + pf):
        p.grad = _randn(*p.shape, seed=50 + i, scale=0.3, dtype=p.dtype)
    ob, of = ops.FusedAdamWClip(pb), ops.FusedAdamWClip(pf)
    was = ops.is_deterministic()
    try:
        ops.set_deterministic(False)
        t_def = ops.FusedAdamWClip.joint_clip_grad_norm_([ob, of], 1.0)
        coef_def = (ob._norm_coef.clone(), of._norm_coef.clone())
        ops.set_deterministic(True)
        t_det = ops.FusedAdamWClip.joint_clip_grad_norm_([ob, of], 1.0)
        t_det2 = ops.FusedAdamWClip.joint_clip_grad_norm_([ob, of], 1.0)
    finally:
        ops.set_deterministic(was)
    ref = float(torch.sqrt(sum(((K.f64(p.grad) ** 2).sum().sqrt().to(p.dtype).to(F64)) ** 2 for p in pb + pf)))
    print(f"joint clip: default {t_def!r} deterministic {t_det!r} restatement {ref!r}")
    assert t_det == t_det2
    # "to fp32 rounding": each mode's per-tensor sum of squares is a tree of depth <= 8 (fma chain) + 6 (wave) + 2 (waves)
    # + 3 (chunks) + 64 (slots) over non-negative terms, relative error <= 83 u, halved by the square root; the two modes
    # therefore agree within 83 u, the host's float64 composition adding nothing visible
    assert abs(t_det - t_def) <= 83 * U * t_def
    assert abs(t_det - ref) <= 83 * U * ref
    for o, c in zip((ob, of), coef_def):
        assert torch.allclose(o._norm_coef, c, rtol=83 * U, atol=0)

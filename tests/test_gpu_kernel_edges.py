"""GPU: the HBM-bound kernels of the C ABI (norms, glue, VAE helpers, dense-gradient helpers) element by element against the
float64 restatements of tests/kernel_ref.py, at the shapes where such kernels go wrong: just past each launch cap (grid-stride
passes), tails that are not whole packets / rows / workgroups, pad lanes, frame switches inside a workgroup, saturation and
cancellation.  Every bound is derived from the tolerance rule of kernel_ref's docstring; the floors are written next to the
asserts.  Outputs the kernel must write in full (pads, tails) are NaN-filled first, through `lib.call` with caller-owned
buffers where the ops wrapper would allocate them; input pad channels the kernel must ignore hold a large finite value.
"""
import functools
import math

import pytest
import torch

import kernel_ref as K

gpu = pytest.mark.gpu    # per test: the file also holds CPU checks of the exact GEMM cases' own arithmetic

BF16, F32 = torch.bfloat16, torch.float32
DEV = "cuda"
U = K.U
NAN = float("nan")


def _call(name, *args):
    from lcv_hip import lib
    lib.call(name, *args, torch.cuda.current_stream().cuda_stream)


def _p(t):
    return None if t is None else t.data_ptr()


def _randn(*shape, seed, scale=1.0, dtype=BF16):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(*shape, generator=g, device=DEV) * scale).to(dtype)


def _rand(*shape, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.rand(*shape, generator=g, device=DEV, dtype=torch.float64)


def _nan(*shape, dtype=BF16):
    return torch.full(shape, NAN, dtype=dtype, device=DEV)


def _row_depth(C):
    """Longest addition chain of a row statistic in rownorm_*_kernel: 8 elements per 64-lane chunk, up to 8 chunks per lane,
    then a 6-level wave tree."""
    return 8 * math.ceil(C / 512) + 6


def _xhat_err(x, xh, rstd, C):
    """Bound on the fp32 kernel's error in xh = (x - mean) * rstd (rule 3 applied to the row statistics): the mean's
    reduction error D u mean|x| and its rounding u |mean|, the subtraction's rounding u |x - mean|, all times rstd; and the
    relative error (D + 4) u of rstd (variance reduction, rsqrt, + eps) times |xh|."""
    D = _row_depth(C)
    x = K.f64(x)
    mean = x.mean(-1, keepdim=True)
    return rstd * (D * U * x.abs().mean(-1, keepdim=True) + U * mean.abs() + U * (x - mean).abs()) + (D + 4) * U * xh.abs()


# --------------------------------------------------------------------------------------------- lcv_vae_rmsnorm_silu
@gpu
@pytest.mark.parametrize("rows,C,Cpad,silu", [
    (262161, 120, 128, 1),   # LPR 16: second row group (U = 2) and a second grid-stride pass past 8192 wg x 16 rows x 2
    (65541, 256, 256, 0),    # LPR 32 past its cap (8192 wg x 8 rows), apply_silu = 0
    (32773, 376, 384, 1),    # LPR 64 past its cap (8192 wg x 4 rows); 48 of 64 lanes live, C < Cpad
    (1000, 3, 8, 1),         # one live lane per row
])
def test_vae_rmsnorm_silu_edges(rows, C, Cpad, silu):
    x = _randn(rows, Cpad, seed=1, scale=2.0)
    x[:, C:] = 3.0e4                       # input pad: must not enter the norm
    x[::997, :C] = 0                       # zero rows: the 1e-12 clamp, output 0
    x[-1, :C] = 0
    gamma = (1.0 + _randn(Cpad, seed=2, scale=0.5, dtype=F32)).to(BF16)
    gamma[C:] = 5.0
    y = _nan(rows, Cpad)
    _call("lcv_vae_rmsnorm_silu", _p(x), _p(gamma), _p(y), rows, C, Cpad, silu)
    # rule 1, no cancellation (a norm, products, x / (1 + e^-x)): 1 bf16 ulp; pads and zero rows are exactly 0
    K.assert_within(y, K.vae_rmsnorm_silu(x, gamma, C, bool(silu)), 1.0, what=f"vae_rmsnorm rows={rows} C={C}/{Cpad}")


# ------------------------------------------------------------------------------------------------- lcv_softmax_rows
@gpu
@pytest.mark.parametrize("rows,n,ld_s,ld_p,scale", [
    (16, 14400, 14400, 14464, 384 ** -0.5),   # the 720p VAE mid-block row; p padded to 64 columns
    (5, 300, 301, 320, 0.7),                  # n not a multiple of 256, ld_s > n, ld_p > n
    (3, 1, 2, 8, 1.0),                        # one column
])
def test_softmax_rows_edges(rows, n, ld_s, ld_p, scale):
    # logits spread so that scale * (max - min) = 80: exp(-80) = 1.8e-35 is still a normal bf16
    s = (_rand(rows, ld_s, seed=3) * (80.0 / scale) - 40.0 / scale).to(F32)
    s[:, n:] = 1.0e30                          # input pad columns: never read
    p = _nan(rows, ld_p)
    _call("lcv_softmax_rows", _p(s), _p(p), rows, n, ld_s, ld_p, float(scale))
    # rule 1: exp, a sum of positive terms (depth n/256 + 8) and a division, no cancellation: 1 bf16 ulp, pads exactly 0
    K.assert_within(p, K.softmax_rows(s, n, ld_p, scale), 1.0, what=f"softmax_rows n={n}")


@gpu
@pytest.mark.parametrize("scale", [-0.05, 0.0, NAN, math.inf])
def test_softmax_rows_rejects_a_scale_the_max_shift_does_not_guard(scale):
    from lcv_hip.lib import LcvError
    s = torch.zeros(2, 300, dtype=F32, device=DEV)
    p = _nan(2, 320)
    with pytest.raises(LcvError) as e:
        _call("lcv_softmax_rows", _p(s), _p(p), 2, 300, 300, 320, scale)
    assert e.value.code == -1
    torch.cuda.synchronize()
    assert torch.isnan(p.float()).all()        # nothing ran


# ------------------------------------------------------------------------------------------ lcv_gelu_tanh_fwd / _bwd
@gpu
def test_gelu_tanh_fwd_bwd_past_the_block_cap_and_in_saturation():
    n = 4096 * 256 * 8 + 8                     # one packet past 4096 workgroups x 256 lanes x 8: a second grid-stride pass
    x = _randn(n, seed=4, scale=3.0)
    sat = _rand(n // 7, seed=5) * 5.0 + 5.0    # |x| in [5, 10): tanh saturates (to exactly +-1 in fp32 past ~9)
    x[::7][: n // 7] = (sat * torch.where(_rand(n // 7, seed=6) < 0.5, -1.0, 1.0)).to(BF16)
    dy = _randn(n, seed=7)
    y, dx = _nan(n), _nan(n)
    _call("lcv_gelu_tanh_fwd", _p(x), _p(y), n)
    _call("lcv_gelu_tanh_bwd", _p(x), _p(dy), _p(dx), n)
    xf = K.f64(x)
    # fwd: 0.5 x (1 + t) cancels at x << 0; k = 4 (tanhf <= 2 ulp, two roundings), magnitudes 0.5|x| (1 + |t|) <= |x|
    K.assert_within(y, K.gelu_tanh(x), 1.0, 4 * U * xf.abs(), what="gelu_tanh_fwd")
    # bwd: 1 + t and 1 - t^2 cancel; magnitudes |dy| (0.5 (1 + |t|) + 0.5 |x| (1 + t^2) du) <= |dy| (1 + |x| du),
    # du = sqrt(2/pi) (1 + 3 * 0.044715 x^2); k = 4 as above
    du = math.sqrt(2 / math.pi) * (1 + 3 * 0.044715 * xf * xf)
    K.assert_within(dx, K.gelu_tanh_grad(x) * K.f64(dy), 1.0, 4 * U * K.f64(dy).abs() * (1 + xf.abs() * du),
                    what="gelu_tanh_bwd")


# -------------------------------------------------------------------------------------- lcv_linear_f32_smallm_wgrad
@gpu
@pytest.mark.parametrize("M,N,K_,act,want_db", [
    (3, 6 * 4096, 300, 1, True),    # the adaLN modulation width; K tail, two x-blocks (only x-block 0 writes db)
    (64, 40, 1000, 0, False),       # K > 256: four x-blocks, db not wanted
    (2, 9, 37, 0, True),            # one partial x-block
])
def test_linear_f32_smallm_wgrad_edges(M, N, K_, act, want_db):
    dy = _randn(M, N, seed=8, dtype=F32)
    a = _randn(M, K_, seed=9, scale=2.0, dtype=F32)
    dw = _nan(N, K_)
    db = _nan(N) if want_db else None
    _call("lcv_linear_f32_smallm_wgrad", _p(dy), _p(a), _p(dw), _p(db), M, N, K_, act)
    af = K.f64(a)
    act_a = K.silu(af) if act else af
    terms = K.f64(dy).abs().t() @ act_a.abs()                        # sum_m |dy[m,n] act(a[m,k])|
    # rule 3: an fma chain over m (depth M) + 1 bf16 ulp; SiLU adds its own relative error (|a| + 2) u per term
    # (the exponent argument's rounding |a| u, __expf and the division)
    extra = (K.f64(dy).abs().t() @ (act_a.abs() * (af.abs() + 2))) if act else 0.0
    K.assert_within(dw, K.f64(dy).t() @ act_a, 1.0, M * U * terms + U * extra, what=f"smallm_wgrad dw M={M} N={N} K={K_}")
    if want_db:
        K.assert_within(db, K.f64(dy).sum(0), 1.0, M * U * K.f64(dy).abs().sum(0), what="smallm_wgrad db")


# -------------------------------------------------------------------------------------- lcv_transpose_pad, lcv_rowsum
@gpu
@pytest.mark.parametrize("M,N,ld,off", [
    (37, 130, 130, 0),     # N not a multiple of 4 (scalar path for the last packet), M < 64
    (200, 6, 8, 0),        # ld > N, N < 64: one vector packet and one scalar tail per row
    (130, 100, 104, 0),    # N a multiple of 4 but not of 64, ld > N: vector path, partial n tile
    (130, 100, 104, 1),    # the same as a view one element into its storage: the vector path must step aside
    (64, 64, 64, 0),
])
def test_transpose_pad_and_rowsum_edges(M, N, ld, off):
    buf = _randn(M * ld + 8, seed=10)
    x = buf[off: off + M * ld].view(M, ld)[:, :N]
    Mpad = (M + 63) // 64 * 64
    out = _nan(N, Mpad)
    _call("lcv_transpose_pad", _p(x), _p(out), M, N, ld, Mpad)
    ref = torch.zeros(N, Mpad, dtype=BF16, device=DEV)
    ref[:, :M] = x.t()
    K.assert_bits(out, ref, what=f"transpose_pad M={M} N={N} ld={ld} off={off}")
    # rowsum over the transposed operand (the bias gradient): cols = Mpad, rarely a multiple of 512
    _rowsum_check(ref, f"rowsum of transpose_pad M={M}")


def _rowsum_check(xin, what):
    rows, cols = xin.shape
    ref = K.f64(xin).sum(1)
    # rule 3: each lane adds 8 elements per 512-column stride, then a 6-level wave tree
    floor = (8 * math.ceil(cols / 512) + 6) * U * K.f64(xin).abs().sum(1)
    for out_f32 in (0, 1):
        o = _nan(rows, dtype=F32 if out_f32 else BF16)
        _call("lcv_rowsum", _p(xin), _p(o), rows, cols, out_f32)
        # bf16 output: + 1 bf16 ulp (rule 1); fp32 output: the sum itself is the fp32 result
        K.assert_within(o, ref, 0.0 if out_f32 else 1.0, floor, fmt="fp32" if out_f32 else "bf16",
                        what=f"{what} ({'fp32' if out_f32 else 'bf16'} out)")


@gpu
@pytest.mark.parametrize("rows,cols", [(37, 4104), (5, 8), (3, 520)])
def test_rowsum_cols_not_a_multiple_of_512(rows, cols):
    _rowsum_check(_randn(rows, cols, seed=11), f"rowsum {rows}x{cols}")


@gpu
def test_rowsum_rejects_a_misaligned_input():
    from lcv_hip.lib import LcvError
    buf = _randn(4 * 64 + 8, seed=12)
    o = _nan(4, dtype=F32)
    with pytest.raises(LcvError):
        _call("lcv_rowsum", _p(buf[1:]), _p(o), 4, 64, 1)


# ---------------------------------------------------------------------------------------------------- lcv_euler_step
@gpu
@pytest.mark.parametrize("n,negate", [(2048 * 256 + 3, 1), (2048 * 256 + 3, 0), (5, 1)])
def test_euler_step_edges(n, negate):
    dt = 0.7                                   # |dt v| ~ |x|: cancellations occur
    v = _randn(n, seed=13, dtype=F32)
    x0 = _randn(n, seed=14, dtype=F32)
    x = x0.clone()
    _call("lcv_euler_step", _p(v), _p(x), n, dt, negate)
    step = (-dt if negate else dt) * K.f64(v)
    # rule 4: 2 fp32 ulps (contraction) + u |dt v| (the product's rounding where x and dt v cancel)
    K.assert_within(x, K.f64(x0) + step, 2.0, U * step.abs(), fmt="fp32", what=f"euler_step n={n} negate={negate}")


# ---------------------------------------------------------------------------------------------- lcv_cfg_euler_step
@gpu
@pytest.mark.parametrize("zero_star,negate", [(1, 1), (1, 0), (0, 1), (0, 0)])
def test_cfg_euler_step_edges(zero_star, negate):
    B, n = 3, 1024 * 256 + 77                   # past the 1024-workgroup cap, a tail
    g, dt = 4.0, -0.05
    scl = torch.tensor([1.0, 1.0e3, 1.0e-3], device=DEV).view(B, 1)
    c = _randn(B, n, seed=15, dtype=F32) * scl
    u = (_randn(B, n, seed=16, dtype=F32) * 0.8 + 0.3 * c) * scl
    u[2] = 0                                    # all-zero uncond: st = 0 / (0 + 1e-8) = 0
    x0 = _randn(B, n, seed=17, dtype=F32)
    ws = _nan(B, 256, 2, dtype=F32)
    x = x0.clone()
    _call("lcv_cfg_euler_step", _p(c), _p(u), _p(x), _p(ws), B, n, g, dt, negate, zero_star)
    cf, uf = K.f64(c), K.f64(u)
    if zero_star:
        dot, nrm = (cf * uf).sum(1, keepdim=True), (uf * uf).sum(1, keepdim=True)
        st = dot / (nrm + 1e-8)
        # rule 3 for the two dots: per-lane chain ceil(n / 65536), wave tree 6, 4 waves 3, then the 256 partials: 6 + 3
        D = math.ceil(n / 65536) + 6 + 3 + 6 + 3
        dst = (D * U * ((cf * uf).abs().sum(1, keepdim=True) + st.abs() * nrm) / (nrm + 1e-8) + 2 * U * st.abs())
    else:
        st, dst = torch.ones(B, 1, dtype=torch.float64, device=DEV), 0.0
    us = uf * st
    vv = us + g * (cf - us)
    step = dt * (-vv if negate else vv)
    ref = K.f64(x0) + step
    # rule 4: 2 fp32 ulps + u |dt v|; plus the error carried into v: |dt| (|u| |1 - g| dst + u (|1 - g| |u st| +
    # 2 |g| |c - u st| + |v|)) - the zero-star ratio's (rule 3) and the roundings of u*st, c - u*st, g*(..) and the sum
    floor = U * step.abs() + abs(dt) * (uf.abs() * abs(1 - g) * dst + U * (abs(1 - g) * us.abs() + 2 * abs(g) * (cf - us).abs()
                                                                          + vv.abs()))
    K.assert_within(x, ref, 2.0, floor, fmt="fp32", what=f"cfg_euler zero_star={zero_star} negate={negate}")
    # one call gives the same bits every time (the partial sums are added in a fixed order)
    x2 = x0.clone()
    _call("lcv_cfg_euler_step", _p(c), _p(u), _p(x2), _p(ws), B, n, g, dt, negate, zero_star)
    assert torch.equal(x, x2)


# ------------------------------------------------------------------------------------------- lcv_gate_residual_bwd
@gpu
@pytest.mark.parametrize("B,T,S,C,want_dmod", [
    (2, 2, 37, 4096, True),     # C = 4096: both GATE_MAXPK slots; frames switch inside the 32-row workgroups
    (1, 2, 9, 4104, True),      # C > 4096: the per-element-atomic fallback
    (1, 1, 16411, 512, False),  # dmod = NULL past the 4096-workgroup cap (1 050 304 packets)
])
def test_gate_residual_bwd_edges(B, T, S, C, want_dmod):
    ms, goff = 3 * C + 16, C + 8
    y = _randn(B, T * S, C, seed=18)
    dout = _randn(B, T * S, C, seed=19)
    mod = _randn(B, T, ms, seed=20, dtype=F32)
    dmod0 = _randn(B, T, ms, seed=21, dtype=F32)          # accumulated into: start from non-zero values
    dmod = dmod0.clone() if want_dmod else None
    dy = _nan(B, T * S, C)
    _call("lcv_gate_residual_bwd", _p(y), _p(mod), _p(dout), _p(dy), _p(dmod), B, T, S, C, ms, goff)
    gate = K.f64(mod)[:, :, goff: goff + C].repeat_interleave(S, dim=1)
    K.assert_within(dy, gate * K.f64(dout), 1.0, what=f"gate_residual_bwd dy C={C}")   # rule 1: one product
    if want_dmod:
        prod = (K.f64(dout) * K.f64(y)).view(B, T, S, C)
        ref = K.f64(dmod0).clone()
        ref[:, :, goff: goff + C] += prod.sum(2)
        # rule 3 with atomics: depth S + 1 (the accumulate into the prior value)
        floor = torch.zeros_like(ref)
        floor[:, :, goff: goff + C] = (S + 1) * U * (prod.abs().sum(2) + K.f64(dmod0)[:, :, goff: goff + C].abs())
        K.assert_within(dmod, ref, 0.0, floor, fmt="fp32", what=f"gate_residual_bwd dmod C={C}")


# ---------------------------------------------------------------------------- lcv_adaln_modulate_bwd, lcv_layernorm_affine_bwd
def _norm_inputs(B, T, S, C, seed):
    x = (_randn(B, T * S, C, seed=seed, scale=0.8, dtype=F32) + 0.3).to(BF16)
    x[0, 5] = 1.25                          # constant rows: zero variance, rstd = eps^-1/2
    x[-1, -1] = -0.5
    return x


@gpu
@pytest.mark.parametrize("B,T,S,C,with_dres", [
    (2, 2, 37, 4096, True),      # the product width (LDS sums 2 x 16 KiB); S >= 32, not a multiple: one frame switch per wg
    (1, 3, 9, 4096, False),      # S < 32: several frames per workgroup
    (2, 1, 33, 520, True),       # a partial 512-channel chunk
])
def test_adaln_and_layernorm_bwd_edges(B, T, S, C, with_dres):
    eps = 1e-6
    x = _norm_inputs(B, T, S, C, 22)
    dy = _randn(B, T * S, C, seed=23)
    dres = _randn(B, T * S, C, seed=24) if with_dres else None
    ms, sh, sc = 6 * C, 1 * C, 4 * C
    mod = _randn(B, T, ms, seed=25, scale=0.1, dtype=F32)
    dmod0 = _randn(B, T, ms, seed=26, dtype=F32)
    dmod = dmod0.clone()
    dx = _nan(B, T * S, C)
    _call("lcv_adaln_modulate_bwd", _p(x), _p(mod), _p(dy), _p(dx), _p(dmod), B, T, S, C, ms, sh, sc, eps, _p(dres))
    mul = 1.0 + K.f64(mod)[:, :, sc: sc + C].repeat_interleave(S, dim=1)
    _check_rownorm_bwd(x, dy, dres, mul, dx, C, eps, f"adaln_modulate_bwd dx B={B} S={S} C={C}")
    # dmod: shift += sum dy, scale += sum dy * xh over the frame's S rows (rule 3, atomics: depth S + 1)
    xh, _, _ = K.layernorm_xhat(x, eps)
    rstd = K.layernorm_xhat(x, eps)[1]
    dxh = _xhat_err(x, xh, rstd, C)
    dyf = K.f64(dy)
    d0 = K.f64(dmod0)
    for off, terms, extra in ((sh, dyf, 0.0), (sc, dyf * xh, (dyf.abs() * dxh).view(B, T, S, C).sum(2))):
        ref, floor = d0.clone(), torch.zeros_like(d0)
        ref[:, :, off: off + C] += terms.view(B, T, S, C).sum(2)
        floor[:, :, off: off + C] = (S + 1) * U * (terms.abs().view(B, T, S, C).sum(2) + d0[:, :, off: off + C].abs()) + extra
        got = dmod.clone()
        other = [o for o in (sh, sc) if o != off][0]
        got[:, :, other: other + C] = ref[:, :, other: other + C].to(F32)   # checked in its own pass
        K.assert_within(got, ref, 0.0, floor, fmt="fp32", what=f"adaln_modulate_bwd dmod[{off // C}C]")
    # the LayerNorm form: w per channel, dw / db summed over every row
    w = (1.0 + _randn(C, seed=27, scale=0.2, dtype=F32))
    dw0, db0 = _randn(C, seed=28, dtype=F32), _randn(C, seed=29, dtype=F32)
    dw, db = dw0.clone(), db0.clone()
    dx = _nan(B, T * S, C)
    rows = B * T * S
    _call("lcv_layernorm_affine_bwd", _p(x), _p(w), _p(dy), _p(dx), _p(dw), _p(db), rows, C, eps, _p(dres))
    _check_rownorm_bwd(x, dy, dres, K.f64(w), dx, C, eps, f"layernorm_affine_bwd dx C={C}")
    dyr, xhr = dyf.reshape(rows, C), xh.reshape(rows, C)
    K.assert_within(db, K.f64(db0) + dyr.sum(0), 0.0, (rows + 1) * U * (dyr.abs().sum(0) + K.f64(db0).abs()), fmt="fp32",
                    what="layernorm_affine_bwd db")
    K.assert_within(dw, K.f64(dw0) + (dyr * xhr).sum(0), 0.0,
                    (rows + 1) * U * ((dyr * xhr).abs().sum(0) + K.f64(dw0).abs()) + (dyr.abs() * dxh.reshape(rows, C)).sum(0),
                    fmt="fp32", what="layernorm_affine_bwd dw")


def _check_rownorm_bwd(x, dy, dres, mul, dx, C, eps, what):
    ref, xh, rstd, g = K.rownorm_bwd(x, dy, mul, eps)
    dxh = _xhat_err(x, xh, rstd, C)
    D = _row_depth(C)
    mg, mgx = g.mean(-1, keepdim=True), (g * xh).mean(-1, keepdim=True)
    # rule 1 floor for dx = rstd (g - mean g - xh mean(g xh)) + dres, everything that enters the cancellation:
    #   2 u (|g| + |mean g| + |xh| |mean g xh|) rstd    the roundings of g = dy * mul and of the three-term difference
    #   D u (mean|g| + |xh| mean|g xh|) rstd           the two row reductions (rule 3, depth D)
    #   (|mean g xh| dxh + |xh| mean(|g| dxh)) rstd    the error of xh (_xhat_err) through xh * mean(g xh)
    #   (D + 4) u |ref - dres|                         rstd's relative error times the unrounded result
    #   2 u |dres|                                     the fp32 add of the residual gradient
    floor = (rstd * (2 * U * (g.abs() + mg.abs() + xh.abs() * mgx.abs())
                     + D * U * (g.abs().mean(-1, keepdim=True) + xh.abs() * (g * xh).abs().mean(-1, keepdim=True))
                     + mgx.abs() * dxh + xh.abs() * (g.abs() * dxh).mean(-1, keepdim=True))
             + (D + 4) * U * ref.abs())
    if dres is not None:
        floor = floor + 2 * U * K.f64(dres).abs()
        ref = ref + K.f64(dres)
    K.assert_within(dx, ref, 1.0, floor, what=what)


# ------------------------------------------------------ lcv_adaln_modulate_fwd, lcv_layernorm_affine_fwd, lcv_gate_residual_fwd
@gpu
@pytest.mark.parametrize("C", [8, 520, 4096])
def test_norm_and_gate_residual_fwd_edges(C):
    B, T, S, eps = 1, 3, 7, 1e-6                # 21 rows: not a multiple of 4 (one wave per row, 4 per workgroup)
    x = _norm_inputs(B, T, S, C, 30)
    ms, sh, sc, gt = 6 * C + 4, C + 4, 3 * C + 4, 5 * C + 4
    mod = _randn(B, T, ms, seed=31, scale=0.3, dtype=F32)
    y = _nan(B, T * S, C)
    _call("lcv_adaln_modulate_fwd", _p(x), _p(mod), _p(y), B, T, S, C, ms, sh, sc, eps)
    xh, rstd, _ = K.layernorm_xhat(x, eps)
    dxh = _xhat_err(x, xh, rstd, C)
    m = K.f64(mod)
    mul = 1.0 + m[:, :, sc: sc + C].repeat_interleave(S, dim=1)
    add = m[:, :, sh: sh + C].repeat_interleave(S, dim=1)
    # rule 1 floor: xh mul + add cancels: 2 u (|xh mul| + |add|) (the two roundings), |mul| dxh (the error of xh)
    K.assert_within(y, xh * mul + add, 1.0, 2 * U * ((xh * mul).abs() + add.abs()) + mul.abs() * dxh,
                    what=f"adaln_modulate_fwd C={C}")
    w = 1.0 + _randn(C, seed=32, scale=0.2, dtype=F32)
    b = _randn(C, seed=33, scale=0.5, dtype=F32)
    y = _nan(B, T * S, C)
    _call("lcv_layernorm_affine_fwd", _p(x), _p(w), _p(b), _p(y), B * T * S, C, eps)
    wf, bf = K.f64(w), K.f64(b)
    K.assert_within(y, xh * wf + bf, 1.0, 2 * U * ((xh * wf).abs() + bf.abs()) + wf.abs() * dxh,
                    what=f"layernorm_affine_fwd C={C}")
    r = _randn(B, T * S, C, seed=34)
    out = _nan(B, T * S, C)
    _call("lcv_gate_residual_fwd", _p(x), _p(r), _p(mod), _p(out), B, T, S, C, ms, gt)
    gate = m[:, :, gt: gt + C].repeat_interleave(S, dim=1)
    # rule 1 floor: x + gate * y cancels: 2 u (|x| + |gate y|)
    ref = K.f64(x) + gate * K.f64(r)
    K.assert_within(out, ref, 1.0, 2 * U * (K.f64(x).abs() + (gate * K.f64(r)).abs()), what=f"gate_residual_fwd C={C}")


@gpu
def test_gate_residual_fwd_without_gate_past_the_block_cap():
    rows, C = 16200, 520                        # 1 053 000 packets of 8: past 4096 workgroups x 256 lanes
    x, r = _randn(1, rows, C, seed=35), _randn(1, rows, C, seed=36)
    out = _nan(1, rows, C)
    _call("lcv_gate_residual_fwd", _p(x), _p(r), None, _p(out), 1, 1, rows, C, 0, 0)
    # rule 1: x + y of two bf16 values, one fp32 and one bf16 rounding; floor u (|x| + |y|)
    K.assert_within(out, K.f64(x) + K.f64(r), 1.0, U * (K.f64(x).abs() + K.f64(r).abs()), what="gate_residual_fwd gate=None")


# ------------------------------------------------------------------- lcv_swiglu_fwd, lcv_patchify, lcv_unpatchify(_bwd)
@gpu
def test_swiglu_fwd_on_views_into_one_buffer_past_the_block_cap():
    rows, F = 2049, 4104                        # 1 051 137 packets: past 4096 workgroups x 256 lanes
    gu = _randn(rows, 2 * F, seed=37, scale=2.0)
    gate, up = gu[:, :F], gu[:, F:]            # ld_in = 2F > F
    out = _nan(rows, F)
    _call("lcv_swiglu_fwd", _p(gate), _p(up), _p(out), rows, F, 2 * F)
    gf = K.f64(gate)
    # out = bf16(bf16(silu(g)) * up): the fp32 silu (x / (1 + __expf(-x))) carries a relative error <= (|g| + 4) u, so
    # where silu(g) lies that close to a bf16 midpoint the other neighbour is admissible (rule 1, second rounding)
    s, s_alt = K.bf16_neighbours(K.silu(gf), (gf.abs() + 4) * U)
    upf = K.f64(up)
    K.assert_within(out, s * upf, 1.0, alt=s_alt * upf, what="swiglu_fwd")


@gpu
def test_patchify_pad_and_unpatchify_past_the_block_cap():
    B, Cin, T, H, W, Kpad = 1, 16, 2, 258, 258, 128     # 2 x 129^2 tokens x 32 groups = 1 065 024 threads; Kpad > 4 Cin
    x = _randn(B, Cin, T, H, W, seed=38)
    N = T * (H // 2) * (W // 2)
    tok = _nan(B, N, Kpad)
    _call("lcv_patchify", _p(x), _p(tok), B, Cin, T, H, W, Kpad)
    ref = torch.zeros(B, N, Kpad, dtype=BF16, device=DEV)
    ref[:, :, :4 * Cin] = (x.view(B, Cin, T, H // 2, 2, W // 2, 2).permute(0, 2, 3, 5, 1, 4, 6).reshape(B, N, 4 * Cin))
    K.assert_bits(tok, ref, what="patchify")                   # rule 2; k = c*4 + ph*2 + pw, columns >= 4 Cin zero

    Cout, T, H, W = 16, 2, 182, 182                     # 1 059 968 output elements
    N = T * (H // 2) * (W // 2)
    for dt in (BF16, F32):
        t = _randn(B, N, 4 * Cout, seed=39, dtype=dt)
        out = _nan(B, Cout, T, H, W, dtype=F32)
        _call("lcv_unpatchify", _p(t), _p(out), B, Cout, T, H, W, 1 if dt == F32 else 0)
        ref = t.float().view(B, T, H // 2, W // 2, 2, 2, Cout).permute(0, 6, 1, 2, 4, 3, 5).reshape(B, Cout, T, H, W)
        K.assert_bits(out, ref, what=f"unpatchify tok {dt}")
    dout = _randn(B, Cout, T, H, W, seed=40, dtype=F32)
    dtok = _nan(B, N, 4 * Cout, dtype=F32)
    _call("lcv_unpatchify_bwd", _p(dout), _p(dtok), B, Cout, T, H, W)
    ref = dout.view(B, Cout, T, H // 2, 2, W // 2, 2).permute(0, 2, 3, 5, 4, 6, 1).reshape(B, N, 4 * Cout)
    K.assert_bits(dtok, ref, what="unpatchify_bwd")


# ------------------------------------------------------------------------------------------ lcv_fm_noise, lcv_fm_mse
@gpu
def test_fm_noise_past_the_block_cap():
    B, per = 2, 2048 * 256 + 40
    x0, eps = _randn(B, per, seed=41), _randn(B, per, seed=42)
    sig = torch.tensor([0.3171, 0.9012], dtype=F32, device=DEV)
    out = _nan(B, per)
    _call("lcv_fm_noise", _p(x0), _p(eps), _p(sig), _p(out), B, per)
    se = sig.view(B, 1)
    # the kernel's rounding points are torch's three fp32 ops: the same bits ...
    K.assert_bits(out, ((1.0 - se) * x0.float() + se * eps.float()).to(BF16), what="fm_noise (fp32 rounding points)")
    # ... and rule 1 against float64: (1-s) x0 + s eps cancels, floor 2 u (|(1-s) x0| + |s eps|) (+ u for 1 - s)
    s64 = K.f64(se)
    a, e = (1 - s64) * K.f64(x0), s64 * K.f64(eps)
    K.assert_within(out, a + e, 1.0, 3 * U * (a.abs() + e.abs()), what="fm_noise")


@gpu
@pytest.mark.parametrize("Tc", [0, 2, 4])
def test_fm_mse_past_the_block_cap_and_deterministic(Tc):
    B, C, T, HW = 2, 16, 5, 3300               # 528 000 elements: two grid-stride passes over 1024 x 256 lanes
    Tt = T - Tc
    pred = _randn(B, C, T, HW, seed=43, dtype=F32)
    eps, x0 = _randn(B, C, Tt, HW, seed=44), _randn(B, C, Tt, HW, seed=45)
    loss, dpred, ws = _nan(1, dtype=F32), _nan(B, C, T, HW, dtype=F32), _nan(1024, dtype=F32)
    _call("lcv_fm_mse", _p(pred), _p(eps), _p(x0), _p(loss), _p(dpred), _p(ws), B, C, T, Tc, HW)
    vt = K.f64((eps.float() - x0.float()).to(BF16))      # the velocity target, rounded to bf16 (common.py:486)
    d = K.f64(pred)[:, :, Tc:] - vt
    nt = d.numel()
    ref = (d * d).sum() / nt
    # rule 3: every term d^2 / n is positive; per term 5 u (d = pred - vt, d^2, 1/n, the product with the partial sum's
    # share), then the chain: ceil(total / 262144) per lane, 6 wave levels, 2 for the four waves, 10 for the 1024 partials
    depth = math.ceil(B * C * T * HW / (1024 * 256)) + 6 + 2 + 10
    K.assert_within(loss, ref.view(1), 0.0, (depth + 5) * U * ref, fmt="fp32", what=f"fm_mse loss Tc={Tc}")
    gref = torch.zeros_like(K.f64(pred))
    gref[:, :, Tc:] = 2 * d / nt
    # dpred = 2 d (1/n): d and 1/n are correctly rounded fp32 values (2 u |dpred|), the product's rounding is 1 fp32 ulp;
    # the conditioning slice is exactly 0
    K.assert_within(dpred, gref, 1.0, 2 * U * gref.abs(), fmt="fp32", what=f"fm_mse dpred Tc={Tc}")
    loss2, dpred2 = _nan(1, dtype=F32), _nan(B, C, T, HW, dtype=F32)
    _call("lcv_fm_mse", _p(pred), _p(eps), _p(x0), _p(loss2), _p(dpred2), _p(ws), B, C, T, Tc, HW)
    assert torch.equal(loss, loss2) and torch.equal(dpred, dpred2)       # the early stopper's strict `<` needs these bits


# ------------------------------------------------------------------------- lcv_gemm_nt: every tile mode, bit for bit
# Integer-valued bf16 operands (as in tests/conv_ref.py): a in [-3, 3], w in [-2, 2], bias and residual in [-8, 8], the gate an
# integer-valued fp32 table in [-2, 2].  With K = 128 every product and every partial sum is an integer of magnitude
# <= 3 * 2 * 128 + 8 = 776, exact in fp32 in ANY summation order and on either MFMA shape, so the kernel's output is a function
# of its rounding points alone: bf16(sum + bias), and bf16(resid + gate * bf16(sum + bias)) (include/lcv_hip.h).
# M = 300 is ragged against 128 and 256 and rows_per_frame = 110 puts frame switches inside a wave tile; N = 320 is ragged
# against 128 and 256 (and a multiple of 64, for SwiGLU); N = 512 is where LCV_GEMM_TILE=k really takes the four-wave kernel.
_GX_M, _GX_K, _GX_RPF = 300, 128, 110
_GX_MODES = ["1", "2", "6", "7", "8", "9", "k"]
_GX_NS = [320, 512]


@functools.lru_cache(maxsize=None)
def _gx_inputs(N):
    g = torch.Generator().manual_seed(7100 + N)

    def ints(lo, hi, *shape):
        return torch.randint(lo, hi + 1, shape, generator=g).to(F32)
    frames = -(-_GX_M // _GX_RPF)
    return {"a": ints(-3, 3, _GX_M, _GX_K).to(BF16), "w": ints(-2, 2, N, _GX_K).to(BF16), "bias": ints(-8, 8, N).to(BF16),
            "resid": ints(-8, 8, _GX_M, N).to(BF16), "mod": ints(-2, 2, 1, frames, 6 * N)}


_GX_GATE_IDX = 5


@functools.lru_cache(maxsize=None)
def _gx_restatement(N):
    """float64, one rounding where the header says.  -> {case: expected tensor}"""
    x = _gx_inputs(N)
    s = x["a"].double() @ x["w"].double().t()
    sb = s + x["bias"].double()
    gate = x["mod"][0, :, _GX_GATE_IDX * N:(_GX_GATE_IDX + 1) * N].double().repeat_interleave(_GX_RPF, dim=0)[:_GX_M]
    proj = sb.to(BF16).double()                         # the projection output is a bf16 tensor upstream
    return {"none": s.to(BF16), "none+bias": sb.to(BF16), "none,f32": s.to(F32), "none+bias,f32": sb.to(F32),
            "gate_residual": (x["resid"].double() + proj).to(BF16), "gate_residual+gate": (x["resid"].double() + gate * proj).to(BF16)}


@pytest.mark.parametrize("N", _GX_NS)
def test_gemm_exact_cases_are_exact_in_fp32_and_agree_with_the_oracle(N):
    """CPU: the claim the bitwise test rests on, and the restatement against oracle.linear at the same shapes."""
    from oracle import dit_oracle as orc
    x = _gx_inputs(N)
    for k, lo, hi in (("a", -3, 3), ("w", -2, 2), ("bias", -8, 8), ("resid", -8, 8), ("mod", -2, 2)):
        v = x[k].double()
        assert torch.equal(v, v.round()) and v.min() >= lo and v.max() <= hi and v.min() < 0 < v.max(), k
    # any partial sum of any order is bounded by the sum of magnitudes; the gate stage by |resid| + |gate| * that
    worst = (x["a"].double().abs() @ x["w"].double().abs().t()).max().item() + 8
    assert worst <= 776 and 8 + 2 * worst < 2 ** 24
    want = _gx_restatement(N)
    assert torch.equal(want["none+bias,f32"], orc.linear(x["a"], x["w"], x["bias"]))
    assert torch.equal(want["none,f32"], orc.linear(x["a"], x["w"]))
    assert torch.equal(want["none+bias"].float(), orc.linear(x["a"], x["w"], x["bias"], orc.bf16_round))
    gate = x["mod"][0, :, _GX_GATE_IDX * N:(_GX_GATE_IDX + 1) * N].repeat_interleave(_GX_RPF, dim=0)[:_GX_M]
    assert torch.equal(want["gate_residual+gate"].float(),
                       orc.bf16_round(x["resid"].float() + gate * orc.linear(x["a"], x["w"], x["bias"], orc.bf16_round)))


def _gx_equal(got, want, mode, case):
    got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, (mode, case, got.shape, got.dtype)
    bad = ~(got == want)
    if bad.any():
        m, n = bad.nonzero()[0].tolist()
        pytest.fail(f"LCV_GEMM_TILE={mode}, {case}: first difference at (m, n) = ({m}, {n}): got {got[m, n].item()}, "
                    f"want {want[m, n].item()}; {int(bad.sum())} of {bad.numel()} differ")


def _gx_run(N, case):
    from lcv_hip import ops
    from lcv_hip.lib import LCV_EPI_GATE_RESIDUAL, LCV_EPI_GELU_TANH, LCV_EPI_NONE, LCV_EPI_SILU, LCV_EPI_SWIGLU
    x = {k: v.to(DEV) for k, v in _gx_inputs(N).items()}
    a, w, b = x["a"], x["w"], x["bias"]
    if case.startswith("none"):
        return ops.gemm_nt(a, w, b if "+bias" in case else None, epilogue=LCV_EPI_NONE, out_f32=case.endswith(",f32"))
    if case.startswith("gate_residual"):
        gated = case.endswith("+gate")
        return ops.gemm_nt(a, w, b, epilogue=LCV_EPI_GATE_RESIDUAL, resid=x["resid"], mod=x["mod"] if gated else None,
                           gate_idx=_GX_GATE_IDX if gated else 0, rows_per_frame=_GX_RPF)
    if case == "swiglu":
        return ops.gemm_nt(a, w, b, epilogue=LCV_EPI_SWIGLU)
    if case == "swiglu+aux":
        aux = _nan(_GX_M, N)
        return torch.cat([ops.gemm_nt(a, w, b, epilogue=LCV_EPI_SWIGLU, swiglu_aux=aux), aux], dim=1)
    return ops.gemm_nt(a, w, b, epilogue={"gelu": LCV_EPI_GELU_TANH, "silu": LCV_EPI_SILU}[case])


@gpu
@pytest.mark.parametrize("mode", _GX_MODES)
@pytest.mark.parametrize("N", _GX_NS)
def test_gemm_every_tile_mode_equals_the_float64_restatement(N, mode, monkeypatch):
    """NONE (with / without bias, bf16 / fp32 output) and GATE_RESIDUAL (with / without gate) on every LCV_GEMM_TILE mode:
    the 32x32x16 kernels (1, 2), the 16x16x32 two-buffer kernels (6, 7), the 8-phase kernel (8, 9) and the four-wave kernel
    (k, taken at N = 512; at N = 320 it falls back to 9) must each reproduce the restatement bit for bit."""
    monkeypatch.setenv("LCV_GEMM_TILE", mode)
    for case, want in _gx_restatement(N).items():
        _gx_equal(_gx_run(N, case), want, mode, case)


_GX_MODE7 = {}


@gpu
@pytest.mark.parametrize("mode", [m for m in _GX_MODES if m != "7"])
@pytest.mark.parametrize("N", _GX_NS)
def test_gemm_transcendental_epilogues_equal_mode_7_bitwise(N, mode, monkeypatch):
    """SwiGLU (with and without the pre-activation output), GELU and SiLU call device transcendentals: nothing exact can be
    stated on the host, but their inputs are exact, so every mode must equal mode 7 (which the oracle tests of
    test_gpu_kernels.py bound) bit for bit."""
    cases = ["swiglu", "swiglu+aux", "gelu", "silu"]
    if N not in _GX_MODE7:
        monkeypatch.setenv("LCV_GEMM_TILE", "7")
        _GX_MODE7[N] = {case: _gx_run(N, case).cpu() for case in cases}
    monkeypatch.setenv("LCV_GEMM_TILE", mode)
    for case in cases:
        _gx_equal(_gx_run(N, case), _GX_MODE7[N][case], mode, case)


# ------------------------------------------------------------------------------------------- lcv_linear_f32_smallm (forward)
# The relative error of the kernel's SiLU (x / (1 + __expf(-x)); __expf is the hardware exp2 of x * log2(e), whose product carries
# an absolute error that grows with |x|), measured through the kernel itself by test_linear_f32_smallm_silu_error on an MI355X:
# the largest |out - silu(a)| / |silu(a)| over 1024 values of a in [-20, 20] is 8.904e-7 (14.9 u, at a = -17.5; 1.0e-7 over the
# positive half, where 1 + e^-a is close to 1).  The edge cases allow twice this per input.
SMALLM_SILU_REL = 8.904e-07


def _smallm_refused(args):
    from lcv_hip.lib import LcvError
    with pytest.raises(LcvError) as e:
        _call("lcv_linear_f32_smallm", *args)
    assert e.value.code == -1


@gpu
def test_linear_f32_smallm_silu_error():
    """N = K = 64 with the identity as the weight: out[m, n] = silu(a[m, n]) plus 63 exact zeros, so the output is the kernel's
    SiLU itself, held against the float64 SiLU of the same fp32 inputs."""
    M, N = 16, 64
    a = torch.linspace(-20.0, 20.0, M * N, dtype=torch.float64, device=DEV).to(F32).view(M, N)
    assert not (a == 0).any()
    w = torch.eye(N, dtype=BF16, device=DEV)
    out = _nan(M * N + 8, dtype=F32)
    _call("lcv_linear_f32_smallm", _p(a), _p(w), None, _p(out), M, N, N, 1)
    ref = K.silu(K.f64(a)).flatten()
    got = K.f64(out[:M * N])
    assert torch.isfinite(got).all() and torch.isnan(out[M * N:]).all()
    rel = ((got - ref).abs() / ref.abs())
    i = int(rel.argmax())
    print(f"silu_f through linear_f32_smallm: worst relative error {float(rel[i]):.3e} ({float(rel[i]) / U:.1f} u) at a = "
          f"{float(a.flatten()[i])!r}; positive a: {float(rel[a.flatten() > 0].max()):.3e}")
    assert float(rel[i]) <= 2 * SMALLM_SILU_REL


@gpu
@pytest.mark.parametrize("M,N,K_,act,has_bias", [
    (1, 1, 8, 0, False),        # one row, one column, one packet: lane 0 alone works, 15 of a workgroup's 16 columns are past N
    (16, 17, 520, 0, True),     # a full row group; N = 16 + 1: a second workgroup with one column; K = 512 + 8: lane 0 loops twice
    (17, 33, 1032, 1, True),    # a second row group of one row; SiLU on the way into LDS; K = 2 * 512 + 8
    (33, 16, 2560, 0, False),   # three row groups; 16 x 2560 x 4 B = 160 KiB of LDS exactly, the most a workgroup can have
])
def test_linear_f32_smallm_edges(M, N, K_, act, has_bias):
    a = _randn(M, K_, seed=71, scale=2.0, dtype=F32)
    w = _randn(N, K_, seed=72, scale=0.05)
    bias = _randn(N, seed=73) if has_bias else None
    out = _nan(M * N + 8, dtype=F32)           # a canary past the end, NaN everywhere the kernel must write
    _call("lcv_linear_f32_smallm", _p(a), _p(w), _p(bias), _p(out), M, N, K_, act)
    assert torch.isnan(out[M * N:]).all()
    K.check_linear_f32_smallm(out[:M * N].view(M, N), a, w, bias, act, 2 * SMALLM_SILU_REL,
                              what=f"linear_f32_smallm M={M} N={N} K={K_} act={act}")


@gpu
def test_linear_f32_smallm_refuses_what_it_cannot_stage():
    a, w, out = torch.zeros(16, dtype=F32, device=DEV), torch.zeros(16, dtype=BF16, device=DEV), _nan(16, dtype=F32)
    _smallm_refused((_p(a), _p(w), None, _p(out), 1, 1, 2568, 0))      # 16 rows x 2568 x 4 B is past 160 KiB of LDS
    _smallm_refused((_p(a), _p(w), None, _p(out), 1, 1, 12, 0))        # K is no whole number of 8-element packets
    _smallm_refused((_p(a), _p(w), None, _p(out), 1, 0, 8, 0))         # N = 0
    torch.cuda.synchronize()
    assert torch.isnan(out).all()                                      # nothing ran


# -------------------------------------------------------------------------------------------------- lcv_timestep_embedding
@gpu
@pytest.mark.parametrize("n,dim,max_period", [
    (3, 342, 10000.0),     # 3 x 171 = 513 threads: one thread in a third workgroup
    (4, 2, 10000.0),       # one frequency, f_0 = 1: [cos t, sin t]
    (4, 256, 100.0),       # another period
    (0, 256, 10000.0),     # nothing to do: `out` is left alone
])
def test_timestep_embedding_edges(n, dim, max_period):
    """Bound per element (kernel_ref.check_timestep_embedding): the existing oracle test's 2e-4 at arguments of 1000 rad, scaled
    with the argument, plus 2^-22 for cos / sin themselves and the small arguments: 2e-4 |t f_j| / 1000 + 2^-22.  t = 0 is
    exact (cos 1, sin 0).  With f_j = expf(fp32 exponent) the kernel missed this bound at arguments of 10 - 20 rad (1.41 x the
    bound at n = 3, dim = 342, element (0, 248); 1.30 x at max_period = 100, element (3, 243)): the exponent's rounding error,
    up to ln(max_period) * 2^-24 absolute, is the frequency's relative error.  The kernel now forms f_j in double."""
    t = torch.tensor([0.0, -37.5, 612.0, 1000.0][:n], dtype=F32, device=DEV)      # 612 is a bf16 value too
    if n == 3:
        t = torch.tensor([1000.0, 0.0, -37.5], dtype=F32, device=DEV)             # the largest argument in front
    out = _nan(n * dim + 8, dtype=F32)
    _call("lcv_timestep_embedding", _p(t) if n else _p(torch.zeros(1, dtype=F32, device=DEV)), _p(out), n, dim, max_period)
    assert torch.isnan(out[n * dim:]).all()
    if n == 0:
        return
    got = out[:n * dim].view(n, dim)
    K.check_timestep_embedding(got, t, dim, max_period, what=f"timestep_embedding n={n} dim={dim} P={max_period}")
    ref = K.timestep_embedding(t, dim, max_period)[0]
    zero = int((t == 0).nonzero()[0])
    assert torch.equal(got[zero], ref[zero].to(F32)) and bool((got[zero, :dim // 2] == 1).all()) and not got[zero, dim // 2:].any()


@gpu
def test_timestep_embedding_refuses_odd_dim_and_periods_up_to_one():
    from lcv_hip.lib import LcvError
    t, out = torch.ones(2, dtype=F32, device=DEV), _nan(2 * 8, dtype=F32)
    for dim, period in ((7, 10000.0), (8, 1.0), (8, 0.5), (0, 10000.0)):
        with pytest.raises(LcvError) as e:
            _call("lcv_timestep_embedding", _p(t), _p(out), 2, dim, period)
        assert e.value.code == -1
    torch.cuda.synchronize()
    assert torch.isnan(out).all()


# ------------------------------------------------------------------------------------------------------ lcv_fm_mse_samples
@gpu
@pytest.mark.parametrize("B,C,T,Tc,HW,eps_pad,shared_x0", [
    (3, 3, 2, 1, 35, 0, False),          # 105 target elements: one of the 256 part-blocks works, 255 must still write a zero
    (2, 4, 3, 0, 50, 0, False),          # Tc = 0: every frame is a target
    (1, 2, 4, 2, 33, 0, False),          # B = 1
    (2, 1, 2, 1, 64 * 256, 0, False),    # 64 whole part-blocks
    (2, 1, 2, 1, 256 * 256, 0, True),    # every lane of every part-block has exactly one element
    (2, 1, 2, 1, 256 * 256 + 1, 0, False),   # and one lane a second
    (3, 2, 3, 1, 100, 24, False),        # eps rows 24 elements apart
    (3, 2, 3, 1, 100, 0, True),          # one x0 for every sample (stride 0)
])
def test_fm_mse_samples_edges(B, C, T, Tc, HW, eps_pad, shared_x0):
    """LCV_FM_MSE_PARTS is 256: a sample is summed by 256 part-blocks of 256 lanes, so the sizes at which the code takes another
    path are 256 x 256 elements (every lane exactly one) and one more (a lane's second pass); 64 x 256 leaves 192 part-blocks
    idle.  `ws` is NaN first: a part-block that skipped its store would make the loss NaN.  Bound: kernel_ref.check_fm_mse_samples."""
    from kernel_ref import FM_MSE_PARTS
    Tt = T - Tc
    per = C * Tt * HW
    pred = _randn(B, C, T, HW, seed=81, dtype=F32)
    eps_rows = _randn(B, per + eps_pad, seed=82)
    x0 = _randn(1 if shared_x0 else B, C, Tt, HW, seed=83)
    eps = eps_rows[:, :per].reshape(B, C, Tt, HW)                        # the values the kernel reads, as a tensor of their own
    loss, ws = _nan(B + 8, dtype=F32), _nan(B * FM_MSE_PARTS, dtype=F32)  # an unwritten partial would make the loss NaN
    args = (_p(pred), _p(eps_rows), _p(x0), _p(loss), _p(ws), B, C, T, Tc, HW, per + eps_pad, 0 if shared_x0 else per)
    _call("lcv_fm_mse_samples", *args)
    assert torch.isnan(loss[B:]).all() and torch.isfinite(ws).all()
    K.check_fm_mse_samples(loss[:B], pred, eps, x0, Tc, what=f"fm_mse_samples B={B} C={C} T={T} Tc={Tc} HW={HW}")
    loss2 = _nan(B + 8, dtype=F32)
    _call("lcv_fm_mse_samples", *args[:3], _p(loss2), *args[4:])
    assert torch.equal(loss[:B], loss2[:B])                              # fixed-order partial sums: the same bits


@gpu
def test_fm_mse_samples_refuses_overlapping_strides_and_no_target_frame():
    from lcv_hip.lib import LcvError
    B, C, T, Tc, HW = 2, 2, 3, 1, 10
    per = C * (T - Tc) * HW
    pred, e, x = _randn(B, C, T, HW, seed=84, dtype=F32), _randn(B, per, seed=85), _randn(B, per, seed=86)
    loss, ws = _nan(B, dtype=F32), _nan(B * 256, dtype=F32)
    for t, tc, es, xs in ((T, Tc, per - 1, per), (T, Tc, per, 1), (T, T, per, per), (T, T + 1, per, per), (T, -1, per, per)):
        with pytest.raises(LcvError) as err:
            _call("lcv_fm_mse_samples", _p(pred), _p(e), _p(x), _p(loss), _p(ws), B, C, t, tc, HW, es, xs)
        assert err.value.code == -1
    torch.cuda.synchronize()
    assert torch.isnan(loss).all() and torch.isnan(ws).all()

"""float64 restatements of the HBM-bound kernels of the C ABI (norms, glue, VAE helpers, dense-gradient helpers; the LoRA,
SwiGLU-backward, q/k-norm and UMT5 kernels; the flash-attention forward and backward) and the per-element check they are held to in
tests/test_gpu_kernel_edges.py and tests/test_gpu_{lora,bwd,umt5,attn}_kernel_edges.py.  A plain helper module (compare tests/delta_cases.py):
nothing here calls the product's ops; every restatement is the formula of the kernel's header comment (include/lcv_hip.h)
evaluated in float64 with torch, on whatever device its inputs live on.

Tolerance rule.  Every bound below is derived from this rule, never tuned to pass.  u = 2^-24 is the fp32 unit roundoff.

  1. Kernels whose output is ONE bf16 rounding of an fp32 computation (the norms, gelu, swiglu, softmax, fm_noise,
     gate_residual): |got - ref| <= 1 bf16 ulp of the float64 value, on every element.  Rounding alone is half an ulp; the
     other half covers the fp32 arithmetic in front of it, whose relative error (a few u, or depth*u for a reduction of the
     given depth, with depth*u far below 2^-9) never reaches it.  Where the float64 value comes out of a CANCELLATION the
     fp32 error is relative to the magnitudes that cancelled, not to the result: an absolute floor
         k * u * (sum of the magnitudes that cancelled)
     is added, and each test writes that formula next to its assert.
     A kernel with a second, intermediate bf16 rounding (swiglu: bf16(bf16(silu(g)) * u)) is compared with the
     restatement at the same rounding point; where the float64 intermediate lies so close to a bf16 rounding midpoint that
     the kernel's fp32 value may round to the other neighbour, the other neighbour's result is accepted too (`alt`).
  2. Pure data movement (transpose_pad, patchify, unpatchify, gather): torch.equal with torch indexing.
  3. fp32 reductions (rowsum, smallm_wgrad, fm_mse, the zero-star dots, the dmod / dw sums): the standard bound
         depth * u * sum|terms|
     where depth is the longest chain of additions any term passes through.  For a sum in a fixed order that is the
     kernel's own summation tree (per-lane chain + wave tree + ...: Higham, Accuracy and Stability, section 4.2); for
     atomics it is the number of terms.  An output rounded to bf16 adds 1 bf16 ulp (rule 1).
  4. fp32 elementwise updates (euler_step, cfg_euler_step): <= 2 fp32 ulps of the float64 value, since hipcc may contract
     x += dt*v into an FMA (lcv_hip/build.py passes no -ffp-contract flag), plus the rule-1 floor u * |dt*v| where x and
     dt*v cancel (the product's own rounding, when it is not contracted).
  5. Chains of bf16 roundings (lora_down: bf16(s * bf16(x A^T)); t5_rmsnorm: bf16(w * bf16(x rstd)); the q/k norm:
     bf16(bf16(x r) * w), then RoPE, then one rounding; geglu: bf16(bf16(gelu(g)) * up); the T5 attention's probabilities).
     The kernel's fp32 value v' in front of an INNER rounding differs from the float64 value v by its fp32 error delta (a few
     u |v|, or depth * u * sum|terms| after a reduction), so it may round to the other bf16 neighbour:
         |bf16(v') - bf16(v)| <= delta + ulp_bf16(|v| + delta)                                   (`inner_rounding_err`)
     (half an ulp of each rounding; the ulp is taken at |v| + delta because v' may lie one binade up).  Each inner rounding
     contributes that much, and the contribution is carried LINEARLY to the output through the float64 partial derivatives of
     what follows it (|s|, |w|, |cos| + |sin|, |v_j| ...); an error that enters a further inner rounding is that rounding's
     delta.  On top come the outer rounding's 1 ulp (rule 1) and, after a reduction, depth * u * sum|terms| (rule 3) with
     depth the kernel's own summation tree, stated next to each check.  Where the fp32 error in front of the inner rounding is
     purely relative (no cancellation), the tighter statement of rule 1 is used instead: the other neighbour is admissible
     only near a midpoint (`bf16_neighbours` / `alt`: swiglu_bwd's dup, the attention's probabilities).

The flash-attention kernels (lcv_attn_fwd, lcv_attn_bwd: `check_attn_fwd`, `check_attn_bwd`; tests/test_gpu_attn_kernel_edges.py on
the inputs of tests/attn_cases.py) are held to rules 1, 3 and 5 together: the float64 formula of the header, 1 bf16 ulp for the
stored result, half a bf16 ulp per bf16 MFMA operand (P; dS) carried linearly to the output, depth * u * sum|terms| per
accumulation, the cancellation floor of dP - delta, and the fp32 error of the exponent of P.  No tile schedule is restated: P is
rounded relative to whatever running max is in force, and half an ulp is at most BF16_U = 2^-8 relative wherever that puts it.
How large these bounds are: the output's own ulp is 0.4 - 0.8 % of an element, but an element of o is a weighted MEAN of v rows
and much smaller than the |v| its operand terms scale with; on random v the median bound is 1.4 % (5 keys) to 9 % (641 keys)
of the median |o|, for dq 1.4 - 4 %, for dk and dv 2 - 13 % (the largest at 2 017 queries); lse is bounded by 5e-6 to 5e-5
absolutely.  A key that carries 1 / Nk of a row's probability therefore hides inside the bound: the cases plant HEAVY keys (a
quarter to a half of a designated row's probability) exactly where the kernels' edges are - the last key, the first key of the
last tile, the last query row - so that counting one twice, dropping it or losing a tile moves an element by many bounds
(tests/test_kernel_ref.py walks these corruptions through the very checks).

The `check_*` functions below hold the restatement, the derived bound and the assert of one entry point each, so that the GPU
tests (the kernel's result) and the CPU tests of tests/test_kernel_ref.py (deliberately wrong float64 "results") go through
the very same assert.

`assert_within` fails on the WORST element and names its index, value, reference and bound; the worst ratio of error to
bound is also recorded in conftest's parity log (the kernel_parity.json of a GPU run), so that tolerances can later be
tightened from evidence.
"""
import math

import torch

U = 2.0 ** -24          # fp32 unit roundoff


def _spacing(ref: torch.Tensor, mant_bits: int, emin: int) -> torch.Tensor:
    """Spacing of a binary format with `mant_bits` fraction bits and minimum normal exponent `emin` at each |ref|; below
    the normal range, the subnormal spacing 2^(emin - mant_bits)."""
    a = ref.detach().to(torch.float64).abs()
    _, e = torch.frexp(a)                  # a = m * 2^e, m in [0.5, 1)  ->  binade exponent e - 1
    e = torch.where(a > 0, e.to(torch.float64) - 1, float(emin)).clamp_min(emin)    # frexp(0) has exponent 0
    return torch.pow(torch.tensor(2.0, dtype=torch.float64, device=a.device), e - mant_bits)


def bf16_ulp(ref: torch.Tensor) -> torch.Tensor:
    """bf16 spacing at each element of a float64 reference (7 fraction bits; subnormal spacing 2^-133 below 2^-126)."""
    return _spacing(ref, 7, -126)


def fp32_ulp(ref: torch.Tensor) -> torch.Tensor:
    """fp32 spacing at each element (23 fraction bits; subnormal spacing 2^-149 below 2^-126)."""
    return _spacing(ref, 23, -126)


def _record(ratio: float, extra: dict):
    try:
        import conftest
    except ImportError:
        print(f"kernel_ref: worst |err|/bound = {ratio:.4g} {extra}")
        return
    conftest._record_parity(ratio, 1.0, extra)


def assert_within(got: torch.Tensor, ref: torch.Tensor, ulps: float = 1.0, abs_floor=0.0, *, fmt: str = "bf16",
                  alt: torch.Tensor = None, what: str = "") -> float:
    """|got - ref| <= ulps * ulp_fmt(ref) + abs_floor on EVERY element (fmt "bf16" or "fp32"; abs_floor a number or a
    tensor broadcast against ref).  A NaN or inf in `got` where `ref` is finite fails.  `alt` (optional, shaped like ref):
    a second admissible reference, see rule 1 of the module docstring.  Returns the worst ratio of error to bound."""
    ref = ref.detach().to(torch.float64)
    g = got.detach().to(device=ref.device, dtype=torch.float64)
    assert g.shape == ref.shape, f"{what}: shape {tuple(g.shape)} != reference {tuple(ref.shape)}"
    ulp = bf16_ulp(ref) if fmt == "bf16" else fp32_ulp(ref)
    bound = ulps * ulp + abs_floor
    err = (g - ref).abs()
    if alt is not None:
        err = torch.minimum(err, (g - alt.detach().to(device=ref.device, dtype=torch.float64)).abs())
    err = torch.where(torch.isfinite(g), err, torch.full_like(err, math.inf))
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound).flatten()     # 0 / 0 (exact where exactness is due)
    i = int(torch.argmax(ratio))
    worst = float(ratio[i])
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), ref.shape))
    _record(worst, {"metric": "worst |err|/bound", "fmt": fmt, "what": what, "n": ref.numel()})
    assert worst <= 1.0, (f"{what}: element {idx}: got {float(g.flatten()[i])!r}, reference {float(ref.flatten()[i])!r}, "
                          f"|err| {float(err.flatten()[i]):.3e} > bound {float(bound.flatten()[i] if torch.is_tensor(bound) and bound.numel() > 1 else bound):.3e} "
                          f"(ratio {worst:.3g}; {fmt} rule, {ulps} ulp + floor)")
    return worst


def assert_bits(got: torch.Tensor, ref: torch.Tensor, what: str = ""):
    """Rule 2: the same bits as torch indexing.  Names the first differing element (an unwritten NaN-filled pad included)."""
    assert got.dtype == ref.dtype and got.shape == ref.shape, f"{what}: {got.dtype} {tuple(got.shape)} vs {ref.dtype} {tuple(ref.shape)}"
    g, r = got.detach().cpu(), ref.detach().cpu()
    if torch.equal(g, r):
        return
    bad = (g.view(torch.int16 if g.element_size() == 2 else torch.int32) !=
           r.view(torch.int16 if r.element_size() == 2 else torch.int32)).flatten().nonzero()
    i = int(bad[0])
    idx = tuple(int(v) for v in torch.unravel_index(torch.tensor(i), g.shape))
    raise AssertionError(f"{what}: {bad.numel()} elements differ; first at {idx}: got {float(g.flatten()[i])!r}, "
                         f"expected {float(r.flatten()[i])!r}")


def bf16_neighbours(v: torch.Tensor, slack: float):
    """The bf16 rounding of float64 `v` and, where v lies within `slack` * |v| of a rounding midpoint (so that an fp32
    evaluation of v with relative error <= slack may round the other way), the bf16 neighbour on v's other side;
    elsewhere the rounding itself.  Returns (rounded, other) in float64."""
    v = v.to(torch.float64)
    rb = v.to(torch.bfloat16)
    r = rb.to(torch.float64)
    bits = rb.view(torch.int16).to(torch.int32)
    away = (v.abs() > r.abs()).to(torch.int32) * 2 - 1        # the other neighbour lies away from zero (+1) or towards it
    ob = (bits + away).to(torch.int16).view(torch.bfloat16).to(torch.float64)
    near = ((v - r).abs() - 0.5 * bf16_ulp(v)).abs() <= slack * v.abs()
    return r, torch.where(near & (r != 0), ob, r)


# ------------------------------------------------------------------------------------------------ restatements (fp64)
def f64(t):
    return t.detach().to(torch.float64)


def silu(x):
    return x / (1.0 + torch.exp(-x))


def vae_rmsnorm_silu(x, gamma, C: int, apply_silu: bool):
    """lcv_vae_rmsnorm_silu: y = x / max(||x||_2, 1e-12) * sqrt(C) * gamma over the first C of Cpad channels, optional SiLU,
    padding channels 0.  x [rows, Cpad], gamma [Cpad]."""
    x, gamma = f64(x), f64(gamma)
    xc = x[:, :C]
    nrm = torch.sqrt((xc * xc).sum(1, keepdim=True)).clamp_min(1e-12)
    y = xc / nrm * math.sqrt(C) * gamma[:C]
    if apply_silu:
        y = silu(y)
    out = torch.zeros_like(x)
    out[:, :C] = y
    return out


def softmax_rows(s, n: int, ld_p: int, scale: float):
    """lcv_softmax_rows: p = softmax(scale * s[:, :n]) row-wise, columns n..ld_p-1 zero."""
    z = f64(s)[:, :n] * scale
    p = torch.softmax(z, dim=1)
    out = torch.zeros(s.shape[0], ld_p, dtype=torch.float64, device=s.device)
    out[:, :n] = p
    return out


_K0, _K1 = math.sqrt(2.0 / math.pi), 0.044715


def gelu_tanh(x):
    """0.5 x (1 + tanh(sqrt(2/pi) (x + 0.044715 x^3)))."""
    x = f64(x)
    return 0.5 * x * (1.0 + torch.tanh(_K0 * (x + _K1 * x ** 3)))


def gelu_tanh_grad(x):
    """d/dx of gelu_tanh: 0.5 (1 + t) + 0.5 x (1 - t^2) sqrt(2/pi) (1 + 3 * 0.044715 x^2)."""
    x = f64(x)
    t = torch.tanh(_K0 * (x + _K1 * x ** 3))
    return 0.5 * (1.0 + t) + 0.5 * x * (1.0 - t * t) * _K0 * (1.0 + 3.0 * _K1 * x * x)


def layernorm_xhat(x, eps: float):
    """(x - mean) / sqrt(var + eps) over the last axis (biased variance), and the row's rstd."""
    x = f64(x)
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    rstd = 1.0 / torch.sqrt((d * d).mean(-1, keepdim=True) + eps)
    return d * rstd, rstd, mean


def rownorm_bwd(x, dy, mul, eps: float):
    """Backward of y = xh * mul + add w.r.t. x (mul per channel, broadcast against x): g = dy * mul,
    dx = rstd * (g - mean(g) - xh * mean(g * xh)).  Returns dx, xh, rstd, g."""
    xh, rstd, _ = layernorm_xhat(x, eps)
    g = f64(dy) * mul
    dx = rstd * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))
    return dx, xh, rstd, g


# ------------------------------------------------------------------------------- rule 5 and the entry points held to it
def bf16r(v):
    """One bf16 rounding point (round to nearest even), back in float64."""
    return v.to(torch.bfloat16).to(torch.float64)


def inner_rounding_err(v, delta=0.0):
    """Rule 5: a bound on |bf16(v') - bf16(v)| for any v' with |v' - v| <= delta."""
    v = f64(v).abs()
    return delta + bf16_ulp(v + delta)


def silu_grad(x):
    """d/dx of x * sigmoid(x): sig * (1 + x * (1 - sig))."""
    x = f64(x)
    sig = 1.0 / (1.0 + torch.exp(-x))
    return sig * (1.0 + x * (1.0 - sig))


def silu_grad_err(x):
    """Bound on the fp32 error of f = sig * (1 + x * (1 - sig)), sig = 1 / (1 + __expf(-x)) (swiglu_bwd, silu_grad_kernel).
    es = (|x| + 4) u is sig's relative error (the exponent argument's rounding |x| u, __expf, 1 + e, the division).  1 - sig
    carries sig * es + u (1 - sig); times x and rounded: |x| (sig es + 2 u (1 - sig)); 1 + that is rounded: u |inner|.  The
    outer product multiplies inner's error by sig and adds (es + u) |f|.  Where sig lies below fp32's normal range (x < -87.3:
    __expf(-x) overflows past 88.7, and a subnormal 1 / (1 + e) may be flushed) the kernel's sig may be 0: es = 1 there."""
    x = f64(x)
    sig = 1.0 / (1.0 + torch.exp(-x))
    inner = 1.0 + x * (1.0 - sig)
    es = (x.abs() + 4) * U
    es = torch.where(sig < 2.0 ** -126, torch.ones_like(es), es)
    return sig * (x.abs() * (sig * es + 2 * U * (1.0 - sig)) + U * inner.abs()) + (es + U) * (sig * inner).abs()


# ---- lcv_tn_skinny
def tn_skinny_rpb(M: int, K: int):
    """tn_skinny_rpb of csrc/lora.hip: rows per workgroup and the number of row groups (grid.y)."""
    groups = 64 if (K + 511) // 512 <= 8 else 32
    rpb = ((M + groups - 1) // groups + 31) // 32 * 32
    rpb = max(64, min(rpb, 1024))
    return rpb, (M + rpb - 1) // rpb


def tn_tail_row(g, x, R: int):
    """Make the last row heavy, in place: g[M-1, :R] = 16, x[M-1, :] = -16.  Rule 3's bound grows with depth * sum|terms|; at
    M = 66 000 (depth 325) it is about as large as one ordinary row's product, so a kernel that lost its tail row would pass.
    A product of 256 is hundreds of times that bound at every shape of the tests and adds < 1 % to sum|terms|."""
    g[-1, :R] = 16.0
    x[-1, :] = -16.0


def check_tn_skinny(got, g, x, R: int, scale: float, what: str):
    """out[r, k] = scale * sum_m g[m, r] x[m, k], fp32.  g [M, Rpad] (columns >= R are never read), x [M, K] (a view)."""
    M, K = x.shape
    gf, xf = f64(g)[:, :R], f64(x)
    ref = scale * (gf.t() @ xf)
    rpb, groups = tn_skinny_rpb(M, K)
    # rule 3.  Workspace path: a wave's fma chain over its rpb / 4 rows, 3 adds for the other waves' partials, then the row
    # groups in order; + 1 for the multiplication by scale.  Atomic path: the same count of additions in another order.
    depth = rpb // 4 + 3 + groups + 1
    return assert_within(got, ref, 0.0, depth * U * abs(scale) * (gf.abs().t() @ xf.abs()), fmt="fp32", what=what)


# ---- lcv_lora_down
def check_lora_down(got, x, A, R: int, Rpad: int, s: float, what: str):
    """h[M, Rpad] = bf16(s * bf16(x A^T)), columns R..Rpad-1 exactly +0.  x [M, K] (a view), A [R, K]."""
    K = x.shape[1]
    xf, Af = f64(x), f64(A)[:R]
    t = xf @ Af.t()
    ref = torch.zeros(x.shape[0], Rpad, dtype=torch.float64, device=x.device)
    ref[:, :R] = s * bf16r(t)
    # rule 5.  t' is an fp32 sum: each lane's chain of 8 products per 512 columns, then a 6-level wave tree (rule 3) ->
    # delta; the inner rounding's share is carried to h by |s|; the outer rounding is assert_within's 1 ulp
    delta = (8 * math.ceil(K / 512) + 6) * U * (xf.abs() @ Af.abs().t())
    floor = torch.zeros_like(ref)
    floor[:, :R] = abs(s) * inner_rounding_err(t, delta)
    worst = assert_within(got, ref, 1.0, floor, what=what)
    pad = got.detach()[:, R:].cpu()
    assert (pad.view(torch.int16) == 0).all(), f"{what}: a pad column is not +0"
    return worst


# ---- lcv_linear_f32_smallm_bwd
def check_linear_f32_smallm_bwd(got, dy, w, a, act_in: int, what: str):
    """da[M, K] fp32 = act_in'(a) * (dy[M, N] @ w[N, K])."""
    N = dy.shape[1]
    acc, terms = f64(dy) @ f64(w), f64(dy).abs() @ f64(w).abs()
    # rule 3: the thread's chain over one 256-row slab of w, then one atomic per slab
    depth = 256 + math.ceil(N / 256)
    if not act_in:
        return assert_within(got, acc, 0.0, depth * U * terms, fmt="fp32", what=what)
    f = silu_grad(a)
    # the SiLU derivative on top: |f| times the sum's error, the factor's own fp32 error (silu_grad_err) times |sum|, and
    # the rounding of the product (assert_within's 1 fp32 ulp)
    return assert_within(got, f * acc, 1.0, f.abs() * depth * U * terms + silu_grad_err(a) * acc.abs(), fmt="fp32", what=what)


# ---- lcv_linear_f32_smallm (forward)
def linear_f32_smallm(a, w, bias, act_in: int):
    """out[M, N] = act_in(a[M, K]) @ w[N, K]^T + bias -> (the float64 value, |act(a)| @ |w|^T, |bias| broadcast or 0)."""
    x = silu(f64(a)) if act_in else f64(a)
    wf = f64(w)
    b = f64(bias) if bias is not None else torch.zeros(w.shape[0], dtype=torch.float64, device=w.device)
    return x @ wf.t() + b, x.abs() @ wf.abs().t(), b.abs().expand(a.shape[0], -1)


def check_linear_f32_smallm(got, a, w, bias, act_in: int, silu_rel: float, what: str):
    """Rule 3 with the kernel's own tree: a lane's chain of 8 products per 512 columns of K, the 6-level wave tree, then the bias
    (2: its addition and the result's rounding).  act_in = 1 adds `silu_rel` (the relative error allowed to the kernel's SiLU, whose
    __expf is no correctly rounded function) times the magnitudes the activations enter with."""
    ref, mag, b = linear_f32_smallm(a, w, bias, act_in)
    depth = 8 * math.ceil(a.shape[1] / 512) + 6 + 2
    floor = depth * U * (mag + b) + (silu_rel * mag if act_in else 0.0)
    return assert_within(got, ref, 0.0, floor, fmt="fp32", what=what)


# ---- lcv_timestep_embedding
def timestep_embedding(t, dim: int, max_period: float):
    """out[i] = [cos(t_i f_j) for j < dim/2, sin(t_i f_j) for j < dim/2], f_j = exp(-ln(max_period) j / (dim/2))
    -> (the float64 value [n, dim], |t_i f_j| laid out the same way)."""
    half = dim // 2
    f = torch.exp(-math.log(max_period) * torch.arange(half, dtype=torch.float64, device=t.device) / half)
    arg = f64(t)[:, None] * f[None, :]
    return torch.cat([torch.cos(arg), torch.sin(arg)], dim=1), torch.cat([arg, arg], dim=1).abs()


def check_timestep_embedding(got, t, dim: int, max_period: float, what: str):
    """The oracle test of test_gpu_kernels.py allows 2e-4 at arguments of up to 1000 rad (the fp32 error of f_j and of the
    product t f_j moves the argument, and cos / sin have slope 1); scaled with the argument that is 2e-4 |t f_j| / 1000, and
    2^-22 on top for cos / sin themselves (a few fp32 ulps of values up to 1)."""
    ref, arg = timestep_embedding(t, dim, max_period)
    return assert_within(got, ref, 0.0, 2e-4 * arg / 1000.0 + 2.0 ** -22, fmt="fp32", what=what)


# ---- lcv_fm_mse_samples
FM_MSE_PARTS = 256       # LCV_FM_MSE_PARTS: fixed-order partial sums per sample, 256 lanes each


def fm_mse_samples(pred, eps, x0, Tc: int):
    """loss[b] = mean over sample b of (pred[b, :, Tc:] - bf16(eps[b] - x0[b]))^2; pred [B, C, T, HW] fp32, eps / x0
    [B or 1, C, T - Tc, HW] bf16.  The velocity target is the bf16 difference (common.py:486)."""
    vt = f64((eps.float() - x0.float()).to(torch.bfloat16))
    d = f64(pred)[:, :, Tc:] - vt
    return (d * d).flatten(1).mean(1)


def check_fm_mse_samples(got, pred, eps, x0, Tc: int, what: str):
    """Rule 3: every term is positive, so sum|terms| / per is the value itself; depth from fm_mse_parts_kernel and
    fm_mse_finish_kernel: a lane's loop over a stride of 256 x 256 elements, the 6-level wave tree, 2 for the four waves, 8 for
    the tree over the 256 partials."""
    ref = fm_mse_samples(pred, eps, x0, Tc)
    per = pred.shape[1] * (pred.shape[2] - Tc) * pred.shape[3]
    depth = math.ceil(per / (FM_MSE_PARTS * 256)) + 6 + 2 + 8
    return assert_within(got, ref, 0.0, depth * U * ref, fmt="fp32", what=what)


# ---- lcv_swiglu_bwd / lcv_swiglu_bwd_interleaved
def swiglu_il_index(F: int, device=None):
    """The fused layout of lcv_swiglu_bwd_interleaved: per 64 columns 32 gate values, then their 32 up partners.
    -> (columns of gate feature 0..F-1, columns of up feature 0..F-1) in a [rows, 2F] row."""
    c = torch.arange(F, device=device)
    gate = (c // 32) * 64 + c % 32
    return gate, gate + 32


def check_swiglu_bwd(dgate, dup, gate, up, dout, what: str):
    """dup = bf16(dout * bf16(silu(g))), dgate = bf16(dout * up * silu'(g))."""
    gf, uf, df = f64(gate), f64(up), f64(dout)
    # dup, rule 1 with `alt`: silu(g) = g * sig has the relative error (|g| + 4) u of sig (see silu_grad_err) and no
    # cancellation, so only next to a midpoint may the inner rounding take the other neighbour
    s, s_alt = bf16_neighbours(silu(gf), (gf.abs() + 4) * U)
    w0 = assert_within(dup, df * s, 1.0, alt=df * s_alt, what=f"{what} dup")
    # dgate, rule 1: one rounding; silu'(g) cancels (it is 0 at g = -1.278): floor |dout up| * silu_grad_err(g), + 2 u |ref|
    # for the two products in front
    ref = df * uf * silu_grad(gf)
    w1 = assert_within(dgate, ref, 1.0, (df * uf).abs() * silu_grad_err(gf) + 2 * U * ref.abs(), what=f"{what} dgate")
    return max(w0, w1)


# ---- lcv_qknorm_rope_fwd / _bwd
def _rope_pairs(t):
    return t[..., 0::2], t[..., 1::2]


def _interleave(a, b):
    return torch.stack([a, b], dim=-1).flatten(-2)


def check_qknorm_rope_fwd(got, x, w, cs, eps: float, scale: float, what: str):
    """y = bf16(scale * rope(bf16(bf16(x r) * w))), r = rsqrt(mean(x^2) + eps) over D = 128; rope on interleaved pairs:
    (y0, y1) = (n0 c - n1 s, n1 c + n0 s).  x [B, N, H, 128], w [128], cs [N, 64, 2] (the rows of the tokens) or None."""
    xf, wf = f64(x), f64(w)
    r = 1.0 / torch.sqrt((xf * xf).mean(-1, keepdim=True) + eps)
    v1 = xf * r
    n1 = bf16r(v1)
    v2 = n1 * wf
    n2 = bf16r(v2)
    # rule 5.  First inner rounding: r's fp32 error is 16 u relative (8-element chain + 4 shuffle levels for the sum, the
    # division by 128 is exact, + eps, rsqrtf <= 2 ulp), + u for x * r.  Second inner rounding: its input carries the
    # first's error times |w| (+ u |v2| for the product).
    e1 = inner_rounding_err(v1, 17 * U * v1.abs())
    e2 = inner_rounding_err(v2, e1 * wf.abs() + U * v2.abs())
    if cs is None:
        ref, floor = n2 * scale, e2 * scale
    else:
        c, s = f64(cs)[None, :, None, :, 0], f64(cs)[None, :, None, :, 1]
        a0, a1 = _rope_pairs(n2)
        f0, f1 = _rope_pairs(e2)
        ref = _interleave(a0 * c - a1 * s, a1 * c + a0 * s) * scale
        # carried through the rotation by |cos| and |sin|; the rotation itself is three fp32 roundings of terms that may
        # cancel: 2 u (|n0 c| + |n1 s|) (rule 1's floor); the product with scale is inside assert_within's 1 ulp
        floor = (_interleave(f0 * c.abs() + f1 * s.abs(), f1 * c.abs() + f0 * s.abs())
                 + 2 * U * _interleave((a0 * c).abs() + (a1 * s).abs(), (a1 * c).abs() + (a0 * s).abs())) * scale
    return assert_within(got, ref, 1.0, floor, what=what)


def qknorm_rope_bwd(x, dout, w, cs, eps: float, scale: float):
    """The backward the kernel states (weights enter as in the forward without its inner roundings): d = scale * dout,
    t = rope^T(d) = (d0 c + d1 s, d1 c - d0 s), dn = t w, n = x r, dx = r (dn - n mean(dn n)), dw = sum_{b, token, head} t n.
    -> dx, dw [128] and the intermediates the bounds need."""
    xf, wf, d = f64(x), f64(w), f64(dout) * scale
    r = 1.0 / torch.sqrt((xf * xf).mean(-1, keepdim=True) + eps)
    n = xf * r
    if cs is None:
        t, tmag = d, d.abs()
    else:
        c, s = f64(cs)[None, :, None, :, 0], f64(cs)[None, :, None, :, 1]
        d0, d1 = _rope_pairs(d)
        t = _interleave(d0 * c + d1 * s, d1 * c - d0 * s)
        m = (d0 * c).abs() + (d1 * s).abs(), (d1 * c).abs() + (d0 * s).abs()
        tmag = _interleave(*m)
    dn = t * wf
    dot = (dn * n).mean(-1, keepdim=True)
    dx = r * (dn - n * dot)
    return dx, (t * n).sum((0, 1, 2)), dict(r=r, n=n, t=t, tmag=tmag, dn=dn, dot=dot, w=wf)


def check_qknorm_rope_bwd(dx_got, dw_got, x, dout, w, cs, eps: float, scale: float, what: str):
    """dx_got [B, N, H, 128] bf16; dw_got (or None): fp32 [dw_slots, 128] as the kernel left it, summed here over its slots."""
    dx, dw, m = qknorm_rope_bwd(x, dout, w, cs, eps, scale)
    r, n, t, tmag, dn, dot, wf = (m[k] for k in ("r", "n", "t", "tmag", "dn", "dot", "w"))
    # fp32 errors of the pieces: t = rope^T(scale * dout) is a sum of two rounded products that may cancel: 3 u tmag;
    # dn = t w: + u |dn|; n = x r: r's 16 u (see the forward) + u
    et = 3 * U * tmag
    edn = et * wf.abs() + U * dn.abs()
    en = 17 * U * n.abs()
    # the dot: rule 3 at depth 12 (8-element chain + 4 shuffle levels) over |dn n| / 128, the errors of its factors, its own
    # rounding by the multiplication with 1/128
    edot = 12 * U * (dn * n).abs().mean(-1, keepdim=True) + (edn * n.abs() + dn.abs() * en).mean(-1, keepdim=True) + U * dot.abs()
    # rule 1 with the cancellation floor for r (dn - n dot): the errors that enter the difference, the roundings of n * dot
    # and of the difference (2 u of the magnitudes), all times r; r's own relative error and the last product on the result
    floor = r * (edn + en * dot.abs() + n.abs() * edot + 2 * U * (dn.abs() + (n * dot).abs())) + 18 * U * dx.abs()
    worst = assert_within(dx_got, dx, 1.0, floor, what=f"{what} dx")
    if dw_got is not None:
        B, N, H, _ = x.shape
        # rule 3 with atomics: B N H terms per channel (every token and head adds once); the terms' own errors on top
        terms = (t * n).abs().sum((0, 1, 2))
        own = (et * n.abs() + t.abs() * en + U * (t * n).abs()).sum((0, 1, 2))
        worst = max(worst, assert_within(f64(dw_got).sum(0), dw, 0.0, B * N * H * U * terms + own, fmt="fp32", what=f"{what} dw"))
    return worst


# ---- lcv_t5_rmsnorm, lcv_geglu_tanh_fwd
def check_t5_rmsnorm(got, x, w, eps: float, what: str):
    """y = bf16(w * bf16(x * rsqrt(mean(x^2) + eps)))."""
    C = x.shape[-1]
    xf, wf = f64(x), f64(w)
    v = xf / torch.sqrt((xf * xf).mean(-1, keepdim=True) + eps)
    # rule 5: rstd's relative error is (8 ceil(C / 512) + 6 + 4) u (the lane's fma chain, the wave tree; the division, + eps,
    # rsqrtf), + u for x * rstd; the inner rounding's share is carried by |w|
    delta = (8 * math.ceil(C / 512) + 6 + 4 + 1) * U * v.abs()
    return assert_within(got, wf * bf16r(v), 1.0, wf.abs() * inner_rounding_err(v, delta), what=what)


def check_geglu_tanh(got, gate, up, what: str):
    """out = bf16(bf16(gelu_new(gate)) * up)."""
    gf, uf = f64(gate), f64(up)
    v = gelu_tanh(gf)
    # rule 5, not `alt`: 0.5 g (1 + tanh) cancels at g << 0, where the fp32 error 4 u |g| (tanhf <= 2 ulp, two roundings: the
    # floor of the gelu_tanh_fwd test) spans many bf16 neighbours of a tiny gelu(g); it is carried to the output by |up|
    return assert_within(got, bf16r(v) * uf, 1.0, uf.abs() * inner_rounding_err(v, 4 * U * gf.abs()), what=what)


# ---- lcv_t5_attention
def check_t5_attention(got, q, k, v, bias, mask, what: str):
    """out[b, i, h, :] = bf16(sum_j bf16(p_ij) v_j), p = softmax_j(bf16(bf16(q_i . k_j) + bias[h, j - i + S - 1])) over the keys
    with mask[b, j] != 0; a row without a valid key is exactly 0.  q, k, v [B, S, H, 64]; bias [H, 2S - 1]; mask [B, S]."""
    B, S, H, _ = q.shape
    Spad = (S + 63) // 64 * 64
    qf, kf, vf = (f64(t).permute(0, 2, 1, 3) for t in (q, k, v))                  # [B, H, S, 64]
    i = torch.arange(S, device=q.device)
    dist = i[None, :] - i[:, None] + S - 1                                         # [query i, key j] -> j - i + S - 1
    sc = bf16r(bf16r(qf @ kf.transpose(-1, -2)) + f64(bias)[:, dist][None])        # [B, H, S, S]
    valid = (mask != 0)[:, None, None, :].expand_as(sc)
    sc = torch.where(valid, sc, torch.full_like(sc, -math.inf))
    mx = sc.amax(-1, keepdim=True)
    e = torch.where(valid, torch.exp(sc - torch.where(torch.isfinite(mx), mx, torch.zeros_like(mx))), torch.zeros_like(sc))
    den = e.sum(-1, keepdim=True)
    p = torch.where(den > 0, e / den.clamp_min(1e-300), torch.zeros_like(e))
    # the probabilities, rule 1 with `alt`: the tests' scores are exact, so p' differs from p by the fp32 softmax alone,
    # relatively: (|x| + 2) u for __expf(x), |x| <= 16; 14 u for the sum of positive terms (8 per lane + 6 wave levels);
    # 2 u for 1 / sum and the product: 34 u.  Only next to a midpoint may bf16(p') be the other neighbour.
    pb, pb_alt = bf16_neighbours(p, 34 * U)
    ref = (pb @ vf).permute(0, 2, 1, 3)
    # each probability that may round the other way moves the output by |pb_alt - pb| |v_j| (rule 5's linear carry); the PV
    # sum is one fma chain over the Spad staged keys (rule 3, depth Spad); the output's rounding is assert_within's 1 ulp
    floor = (((pb_alt - pb).abs() + Spad * U * pb) @ vf.abs()).permute(0, 2, 1, 3)
    return assert_within(got, ref, 1.0, floor, what=what)


# ---- lcv_attn_fwd / lcv_attn_bwd
LOG2E = 1.4426950408889634
BF16_U = 2.0 ** -8        # unit roundoff of bf16 (8 significant bits): half an ulp is between 2^-9 |v| (just below a power of
                          # two) and 2^-8 |v| (just above one).  With 2^-9 in its place the float64-exact tile restatement of the
                          # documented arithmetic (oracle/dit_oracle.py) fails these checks on exact-grid inputs by up to 1.4.


def _bhnd(t):
    """[B, N, H, D] as the header addresses it -> float64 [B, H, N, D]."""
    return f64(t).permute(0, 2, 1, 3)


def _f32(v: float) -> float:
    return float(torch.tensor(v, dtype=torch.float32))


def attn_fwd(q, k, v, scale: float):
    """o = softmax(q k^T scale) v, lse = logsumexp(q k^T scale) in float64.  q [B, Nq, H, D], k, v [B, Nk, H, D] ->
    o [B, H, Nq, D], lse [B, H, Nq], p [B, H, Nq, Nk], x [B, H, Nq, Nk] (the scores in log2 units)."""
    qf, kf, vf = _bhnd(q), _bhnd(k), _bhnd(v)
    s = (qf @ kf.transpose(-1, -2)) * scale
    lse = torch.logsumexp(s, dim=-1)
    p = torch.exp(s - lse.unsqueeze(-1))
    return p @ vf, lse, p, s * LOG2E


def attn_score_err(x, q, k, scale: float, exact_scores: bool, offset=None):
    """sigma_ij, a bound on the fp32 error of the exponent of P_ij in log2 units (which is also a bound on P's relative error:
    d exp2(x) / exp2(x) = ln 2 dx < dx).  x_ij c - m c (c = scale log2(e); m the running max in force, itself one of the row's
    scores; the backward has lse in m's place: `offset`, [B, H, Nq] in log2 units) is two rounded products, or one fma, and a
    difference: (|x_ij| + |m c|) u with |m c| <= max_j |x_ij|; exp2 and the difference itself: 2 u.  The unit-scale bodies start
    their score accumulators at -m instead: the same magnitudes.  The 128-term dot product in front of it: 128 u scale
    sum_d |q_id k_jd| (rule 3; with `offset` the accumulators of the unit-scale backward start at -lse and every partial sum
    is rounded at that magnitude: 128 u |lse| on top) - unless every partial sum of q . k is exactly representable
    (`exact_scores`: the grids of tests/attn_cases.py), where this part vanishes for the forward."""
    ax = x.abs()
    off = ax.amax(-1, keepdim=True) if offset is None else offset.abs().unsqueeze(-1)
    sigma = (ax + off + 2) * U
    if offset is not None:
        sigma = sigma + (128 + 1) * U * off             # the accumulation from -lse, and lse * log2(e) itself
    if not exact_scores:
        sigma = sigma + 128 * U * abs(scale) * LOG2E * (_bhnd(q).abs() @ _bhnd(k).abs().transpose(-1, -2))
    return sigma


def check_attn_fwd(o_got, lse_got, q, k, v, scale: float, what: str, exact_scores: bool = False):
    """lcv_attn_fwd: o_got [B, Nq, H, D] bf16, lse_got [B, H, Nq] fp32 or None; q, k, v as the header addresses them."""
    scale = _f32(scale)
    o, lse, p, x = attn_fwd(q, k, v, scale)
    vf = _bhnd(v)
    Nk = vf.shape[2]
    depth = (Nk + 63) // 64 * 64                        # the staged keys: one fma chain per output element (PV), one per row (l)
    sp = attn_score_err(x, q, k, scale, exact_scores) * p
    # 1 bf16 ulp of o (rule 1; its spare half ulp also holds the row sum l's own chain, depth u |o| << 2^-9 |o|)
    # + (BF16_U + depth u) sum_j p_ij |v_jd|: P is the bf16 MFMA operand, rounded relative to whatever running max is in
    #   force: half an ulp, <= BF16_U relative wherever the max puts P inside its binade, so the tile schedule need not be
    #   restated; l takes the unrounded P; the PV chain (rule 3 + rule 5)
    # + sum_j sigma_ij p_ij |v_jd - o_id| <= (sigma p) |v| + rowsum(sigma p) |o|: an error of the exponent moves numerator and l
    floor = (BF16_U + depth * U) * (p @ vf.abs()) + sp @ vf.abs() + sp.sum(-1, keepdim=True) * o.abs()
    worst = assert_within(o_got, o.permute(0, 2, 1, 3), 1.0, floor.permute(0, 2, 1, 3), what=f"{what} o")
    if lse_got is not None:
        # lse = m scale + __logf(l).  l: an fp32 sum of positive terms, depth u relative, and its terms' own errors
        # sum_j p_ij sigma_ij; both are absolute errors of log l.  __logf = v_log_f32 * ln 2: 2 u |log l| with 1 <= l <= 64 depth
        # (the largest term is >= 1, none exceeds 2^ATTN_RESCALE_THR), + 4 u where log l is near 0.  m scale: one rounding,
        # u max_j |s_ij|.  The final sum: 1 fp32 ulp of lse (assert_within).
        s_max = x.abs().amax(-1) / LOG2E
        fl = depth * U + sp.sum(-1) + 2 * U * math.log(64.0 * depth) + 4 * U + U * s_max
        worst = max(worst, assert_within(lse_got, lse, 1.0, fl, fmt="fp32", what=f"{what} lse"))
    return worst


def attn_bwd(q, k, v, o_in, d_o, lse_in, scale: float):
    """The backward as a pure function of the kernel's inputs, float64: P = exp(s - lse_in), delta = sum_d dO O_in,
    dV = P^T dO, dS = P (dO V^T - delta) scale, dQ = dS K, dK = dS^T Q.  -> dq, dk, dv [B, H, N, D] and the intermediates."""
    qf, kf, vf, of, gf = _bhnd(q), _bhnd(k), _bhnd(v), _bhnd(o_in), _bhnd(d_o)
    s = (qf @ kf.transpose(-1, -2)) * scale
    p = torch.exp(s - f64(lse_in).unsqueeze(-1))
    delta = (gf * of).sum(-1, keepdim=True)
    dsu = p * (gf @ vf.transpose(-1, -2) - delta)        # dS without the scale
    ds = dsu * scale
    return ds @ kf, ds.transpose(-1, -2) @ qf, p.transpose(-1, -2) @ gf, dict(p=p, dsu=dsu, ds=ds, x=s * LOG2E, qf=qf, kf=kf,
                                                                            vf=vf, of=of, gf=gf)


def check_attn_bwd(dq, dk, dv, q, k, v, o_in, d_o, lse_in, scale: float, scale_inside: bool, prev_dk=None, prev_dv=None,
                   what: str = "", qsplit: int = 1, exact_scores: bool = False):
    """lcv_attn_bwd: dq [B, Nq, H, D], dk, dv [B, Nk, H, D] bf16 as the kernels left them.  `scale_inside`: dS = P (dP - delta)
    scale is rounded to bf16 (the general-scale forms) or dS' = P (dP - delta) is and the scale multiplies dQ / dK afterwards
    (the unit-scale forms).  prev_dk / prev_dv: what dk / dv held before an accumulate_kv call.  qsplit: the number of
    slices the query sweep of pass A was split into (attn_bwd_qsplit)."""
    scale = _f32(scale)
    rq, rk, rv, m = attn_bwd(q, k, v, o_in, d_o, lse_in, scale)
    p, dsu, ds, x, qf, kf, vf, of, gf = (m[n] for n in ("p", "dsu", "ds", "x", "qf", "kf", "vf", "of", "gf"))
    Nq, Nk = qf.shape[2], kf.shape[2]
    depth_q = (Nq + 31) // 32 * 32 + (qsplit if qsplit > 1 else 0)    # pass A: the 32-row tiles' chain, then the slices in order
    depth_k = (Nk + 63) // 64 * 64                                    # pass B: the staged keys
    # the operands' errors in front of the MFMAs.  P: its exponent's fp32 error (attn_score_err, lse in the running max's place)
    # and its rounding to bf16: half a bf16 ulp of the fp32 value, which lies within sigma p of p (rule 5's ulp at |v| + delta)
    sigma = attn_score_err(x, q, k, scale, exact_scores, offset=f64(lse_in) * LOG2E)
    e_p = sigma * p + 0.5 * bf16_ulp(p + sigma * p)
    # dP - delta: two fp32 sums that cancel (rule 1's floor; the unit-scale forms start dP's accumulator at -delta: the same
    # magnitudes): 128 u (sum_d |dO||V| + sum_d |dO||O|), carried through P scale; P's own error and the two products on dS
    e_d = 128 * U * (gf.abs() @ vf.abs().transpose(-1, -2) + (gf.abs() * of.abs()).sum(-1, keepdim=True))
    e_dsu = p * e_d + (sigma + 3 * U) * dsu.abs()
    # its rounding to bf16, half an ulp of the value the form rounds: dS itself, or dS' = dS / scale with the scale behind it - with
    # a scale that is no power of two the two lie at different places of their binades, which is all `scale_inside` changes
    if scale_inside:
        e_ds = abs(scale) * e_dsu + 0.5 * bf16_ulp(ds.abs() + abs(scale) * e_dsu)
    else:
        e_ds = abs(scale) * (e_dsu + 0.5 * bf16_ulp(dsu.abs() + e_dsu))
    # dV = P^T dO: 1 bf16 ulp + the operand's error times |dO| + the chain over the query sweep (rule 3)
    f_v = e_p.transpose(-1, -2) @ gf.abs() + depth_q * U * (p.transpose(-1, -2) @ gf.abs())
    # dQ = dS K, dK = dS^T Q likewise (the scale behind the sum is one more fp32 rounding: u |result|)
    out = 0.0 if scale_inside else U
    f_q = e_ds @ kf.abs() + depth_k * U * (ds.abs() @ kf.abs()) + out * rq.abs()
    f_k = e_ds.transpose(-1, -2) @ qf.abs() + depth_q * U * (ds.abs().transpose(-1, -2) @ qf.abs()) + out * rk.abs()
    # accumulate_kv: the fp32 sum and what dk / dv held are added in fp32 and rounded ONCE (the store of attn_bwd_dkv_kernel,
    # attn_bwd_kv_finish_kernel, the epilogue of attn_bwd_dkv2_kernel): the reference is prev + d, still 1 bf16 ulp of it; the
    # fp32 addition sits in that ulp's spare half
    if prev_dk is not None:
        rk = rk + _bhnd(prev_dk)
    if prev_dv is not None:
        rv = rv + _bhnd(prev_dv)
    t = lambda a: a.permute(0, 2, 1, 3)
    return (assert_within(dq, t(rq), 1.0, t(f_q), what=f"{what} dq"), assert_within(dk, t(rk), 1.0, t(f_k), what=f"{what} dk"),
            assert_within(dv, t(rv), 1.0, t(f_v), what=f"{what} dv"))

"""float64 restatements of the HBM-bound kernels of the C ABI (norms, glue, VAE helpers, dense-gradient helpers) and the
per-element check they are held to in tests/test_gpu_kernel_edges.py.  A plain helper module (compare tests/delta_cases.py):
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

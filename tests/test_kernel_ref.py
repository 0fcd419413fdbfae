"""CPU: the per-element check of tests/kernel_ref.py is sensitive enough to be worth its GPU time (one element 2 bf16 ulps
off fails, one non-zero pad element fails, the exact rounding passes; every check_* of rule 5 passes a result computed another
way and fails the results a kernel bug would give), and every compute entry point that include/lcv_hip.h
declares has a kernel-level test (the coverage guard: a new entry point without one fails here, without a GPU)."""
import ast
import math
import re
from pathlib import Path

import pytest
import torch

import attn_cases as AC
import kernel_ref as K

ROOT = Path(__file__).resolve().parents[1]
TESTS = ROOT / "tests"
EDGES = "test_gpu_kernel_edges.py"
LORA_EDGES = "test_gpu_lora_kernel_edges.py"
BWD_EDGES = "test_gpu_bwd_kernel_edges.py"
UMT5_EDGES = "test_gpu_umt5_kernel_edges.py"
ATTN_EDGES = "test_gpu_attn_kernel_edges.py"
OPTIM_EDGES = "test_gpu_optim_kernel_edges.py"


# ------------------------------------------------------------------------------------------------ assert_within itself
def _ref(n=4096, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g, dtype=torch.float64) * torch.exp(torch.randn(n, generator=g, dtype=torch.float64) * 4)


def test_bf16_ulp_is_the_spacing_of_bf16():
    v = torch.tensor([1.0, 1.5, 2.0, -3.0, 0.0, 2.0 ** -126, 2.0 ** -130, 0.75], dtype=torch.float64)
    assert K.bf16_ulp(v).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -6, 2.0 ** -133, 2.0 ** -133, 2.0 ** -133,
                                      2.0 ** -8]
    # the spacing is the distance to the next bf16 value up, for random normal values
    r = _ref().abs().clamp_min(1e-30).to(torch.bfloat16)
    nxt = (r.view(torch.int16) + 1).view(torch.bfloat16)
    assert torch.equal(nxt.double() - r.double(), K.bf16_ulp(r.double()))
    assert K.fp32_ulp(torch.tensor([1.0], dtype=torch.float64)).item() == 2.0 ** -23


def test_assert_within_accepts_the_bf16_rounding():
    ref = _ref()
    assert K.assert_within(ref.to(torch.bfloat16), ref, 1.0, what="rounding") <= 0.5


def test_assert_within_rejects_one_element_two_ulps_off():
    ref = _ref()
    got = ref.to(torch.bfloat16)
    i = 1234
    bits = got.view(torch.int16)
    bits[i] += 2                                   # one element moved by 2 bf16 ulps (same binade for this seed)
    assert K.bf16_ulp(got[i].double()) == K.bf16_ulp(ref[i])
    with pytest.raises(AssertionError, match=r"element \(1234,\)"):
        K.assert_within(got, ref, 1.0, what="two ulps")


def test_assert_within_rejects_one_non_zero_pad_element_and_a_nan():
    ref = _ref(64 * 8).view(64, 8)
    ref[:, 6:] = 0                                 # pad channels
    got = ref.to(torch.bfloat16)
    got[17, 7] = 2.0 ** -120                       # a tiny non-zero pad element
    with pytest.raises(AssertionError, match=r"element \(17, 7\)"):
        K.assert_within(got, ref, 1.0, what="pad")
    got = ref.to(torch.bfloat16)
    got[3, 6] = float("nan")                       # an unwritten, NaN-filled pad
    with pytest.raises(AssertionError, match=r"element \(3, 6\)"):
        K.assert_within(got, ref, 1.0, what="nan pad")


def test_floor_and_fp32_rule():
    ref = _ref().float().double()
    got = ref.float()
    got[5] = torch.nextafter(torch.nextafter(got[5], torch.tensor(1e30)), torch.tensor(1e30))
    K.assert_within(got, ref, 2.0, fmt="fp32", what="2 fp32 ulps")
    got[5] = torch.nextafter(got[5], torch.tensor(1e30))
    with pytest.raises(AssertionError):
        K.assert_within(got, ref, 2.0, fmt="fp32", what="3 fp32 ulps")
    K.assert_within(got, ref, 2.0, K.U * ref.abs() * 2, fmt="fp32", what="with a floor")
    # a zero bound demands exactness: equal values pass (0 / 0 is no failure), any difference fails
    assert K.assert_within(ref.float(), ref, 0.0, fmt="fp32", what="exact") == 0.0
    with pytest.raises(AssertionError):
        K.assert_within(got, ref, 0.0, fmt="fp32", what="exact")


def test_assert_bits_names_the_first_difference():
    a = torch.zeros(3, 5, dtype=torch.bfloat16)
    b = a.clone()
    b[2, 1] = float("nan")
    with pytest.raises(AssertionError, match=r"first at \(2, 1\)"):
        K.assert_bits(b, a)
    K.assert_bits(a, a.clone())


def test_bf16_neighbours_admits_the_other_rounding_only_near_a_midpoint():
    v = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, 1.0 + 2.0 ** -9, -(1.0 + 3 * 2.0 ** -8)], dtype=torch.float64)
    r, o = K.bf16_neighbours(v, 2.0 ** -18)
    assert r.tolist() == [1.0, 1.0078125, 1.0, -1.015625]
    assert o.tolist() == [1.0078125, 1.0, 1.0, -1.0078125]


def test_restatements_match_the_formulas_at_hand_values():
    x = torch.tensor([[3.0, 4.0, 99.0]], dtype=torch.float64)
    y = K.vae_rmsnorm_silu(x, torch.tensor([1.0, 2.0, 7.0]), 2, False)
    assert torch.allclose(y, torch.tensor([[0.6 * 2 ** 0.5, 1.6 * 2 ** 0.5, 0.0]], dtype=torch.float64))
    p = K.softmax_rows(torch.tensor([[0.0, 1.0, 5.0]]), 2, 4, -1.0)
    assert torch.allclose(p, torch.tensor([[1 / (1 + torch.e ** -1), 1 - 1 / (1 + torch.e ** -1), 0, 0]], dtype=torch.float64))
    t = torch.linspace(-6, 6, 101, dtype=torch.float64).requires_grad_(True)
    torch.nn.functional.gelu(t, approximate="tanh").sum().backward()
    assert torch.allclose(t.grad, K.gelu_tanh_grad(t.detach()), rtol=1e-12, atol=1e-14)
    assert torch.allclose(K.gelu_tanh(t.detach()), torch.nn.functional.gelu(t.detach(), approximate="tanh"), rtol=1e-12)
    xr = torch.randn(4, 16, dtype=torch.float64, generator=torch.Generator().manual_seed(1)).requires_grad_(True)
    mul = torch.rand(16, dtype=torch.float64) + 0.5
    dy = torch.randn(4, 16, dtype=torch.float64)
    (torch.nn.functional.layer_norm(xr, (16,), eps=1e-6) * mul * dy).sum().backward()
    dx, _, _, _ = K.rownorm_bwd(xr.detach(), dy, mul, 1e-6)
    assert torch.allclose(dx, xr.grad, rtol=1e-10, atol=1e-12)


# -------------------------------------------------------- rule 5 and the check_* functions: hand values, autograd, teeth
# Each check_* of kernel_ref is fed (a) a result computed HERE in another way (autograd, torch.nn.functional, complex
# multiplication for the rotation), rounded where the kernel rounds: it must pass; (b) deliberately wrong float64 "results"
# of the kind a kernel bug produces: each must fail.  (b) is the proof that the derived bounds are not vacuous.
BF16 = torch.bfloat16
F = torch.nn.functional


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _rn(*shape, seed, scale=1.0, dtype=BF16):
    return (torch.randn(*shape, generator=_g(seed), dtype=torch.float64) * scale).to(dtype)


def _fails(fn, *args):
    with pytest.raises(AssertionError):
        fn(*args, "wrong on purpose")


def test_inner_rounding_err_bounds_the_two_roundings():
    v = _ref(20000, seed=3)
    delta = v.abs() * 2.0 ** -10 * torch.rand(v.shape, generator=_g(4), dtype=torch.float64)
    for sign in (-1.0, 1.0):
        moved = K.bf16r(v + sign * delta)
        assert ((moved - K.bf16r(v)).abs() <= K.inner_rounding_err(v, delta)).all()
    # and it is not slack beyond the rule: delta + one ulp at |v| + delta
    assert torch.equal(K.inner_rounding_err(torch.tensor([1.0, 1.99]), 0.02), 0.02 + torch.tensor([2.0 ** -7, 2.0 ** -6], dtype=torch.float64))


def test_silu_grad_and_the_interleaved_index_map():
    t = torch.linspace(-12, 12, 97, dtype=torch.float64).requires_grad_(True)
    F.silu(t).sum().backward()
    assert torch.allclose(K.silu_grad(t.detach()), t.grad, rtol=1e-13, atol=1e-15)
    assert abs(float(K.silu_grad(torch.tensor([0.0]))) - 0.5) < 1e-15 and abs(float(K.silu_grad(torch.tensor([-1.2784645427610738], dtype=torch.float64)))) < 1e-12
    # the error bound is a few u where nothing cancels and stays finite in saturation
    e = K.silu_grad_err(torch.tensor([0.0, 30.0, -30.0, 100.0, -100.0]))
    assert torch.isfinite(e).all() and 2 * K.U < float(e[0]) < 8 * K.U
    # 32 gate columns, then their 32 up partners, per 64 columns
    gi, ui = K.swiglu_il_index(96)
    assert gi.tolist() == list(range(0, 32)) + list(range(64, 96)) + list(range(128, 160))
    assert ui.tolist() == list(range(32, 64)) + list(range(96, 128)) + list(range(160, 192))
    assert sorted(gi.tolist() + ui.tolist()) == list(range(192))
    assert K.tn_skinny_rpb(1, 8) == (64, 1) and K.tn_skinny_rpb(4097, 520) == (96, 43)
    assert K.tn_skinny_rpb(66000, 8) == (1024, 65) and K.tn_skinny_rpb(2049, 4104) == (96, 22)


def test_tn_skinny_check_has_teeth():
    M, K_, R, Rpad, scale = 70, 24, 5, 8, 0.5
    g, x = _rn(M, Rpad, seed=10), _rn(M, K_, seed=11)

    def out(gm, xm):
        return (scale * gm.double().t() @ xm.double()).float()
    K.check_tn_skinny(out(g[:, :R], x), g, x, R, scale, "right")
    _fails(K.check_tn_skinny, out(g[:-1, :R], x[:-1]), g, x, R, scale)                 # the last row dropped
    _fails(K.check_tn_skinny, out(g[:, 1: R + 1], x), g, x, R, scale)                  # the rank columns shifted by one
    _fails(K.check_tn_skinny, out(g[:, :R], x) * 2, g, x, R, scale)                    # accumulated twice into a non-zero out
    # at the row-group cap (depth 325 over 66 000 terms) an ordinary tail row is below rule 3's bound; the GPU cases therefore
    # end on a heavy row (`tn_tail_row`), which is not
    M, K_, R = 66000, 8, 32
    g, x = _rn(M, R, seed=30), _rn(M, K_, seed=31)
    rpb, groups = K.tn_skinny_rpb(M, K_)
    bound = (rpb // 4 + 3 + groups + 1) * K.U * (g.double().abs().t() @ x.double().abs())      # check_tn_skinny's, at scale 1
    assert ((g[-1].double()[:, None] * x[-1].double()[None, :]).abs() < bound).any()   # the ordinary tail row could hide
    K.tn_tail_row(g, x, R)
    K.check_tn_skinny(out(g, x), g, x, R, scale, "right, heavy tail")
    _fails(K.check_tn_skinny, out(g[:-1], x[:-1]), g, x, R, scale)                     # the last row dropped
    assert ((g[-1].double()[:, None] * x[-1].double()[None, :]).abs() > 100 * bound).all()


def test_lora_down_check_has_teeth():
    M, K_, R, Rpad, s = 6, 1032, 9, 16, 0.37
    x, A = _rn(M, K_, seed=12), _rn(R, K_, seed=13, scale=0.5)

    def out(Am):
        h = torch.zeros(M, Rpad, dtype=BF16)
        h[:, :Am.shape[0]] = (s * (x.double() @ Am.double().t()).to(BF16).double()).to(BF16)
        return h
    right = out(A)
    K.check_lora_down(right, x, A, R, Rpad, s, "right")
    stale = right.clone()
    stale[3, R] = 2.0 ** -100
    _fails(K.check_lora_down, stale, x, A, R, Rpad, s)                                 # one pad column left stale
    negz = right.clone()
    negz[0, Rpad - 1] = -0.0
    _fails(K.check_lora_down, negz, x, A, R, Rpad, s)                                  # the pad is +0, not -0
    _fails(K.check_lora_down, out(A.roll(1, 0)), x, A, R, Rpad, s)                     # a rank column shifted by one
    last = right.clone()
    last[M - 1] = right[M - 2]
    _fails(K.check_lora_down, last, x, A, R, Rpad, s)                                  # the last row computed from the row before
    _fails(K.check_lora_down, (right.double() / s).to(BF16), x, A, R, Rpad, s)         # s forgotten


def test_linear_f32_smallm_bwd_check_against_autograd_and_teeth():
    M, N, K_ = 5, 300, 34
    dy, a = _rn(M, N, seed=14, dtype=torch.float32), _rn(M, K_, seed=15, scale=2.0, dtype=torch.float32)
    w = _rn(N, K_, seed=16, scale=0.5)
    for act in (0, 1):
        ad = a.double().requires_grad_(True)
        ((F.silu(ad) if act else ad) @ w.double().t() * dy.double()).sum().backward()
        K.check_linear_f32_smallm_bwd(ad.grad.float(), dy, w, a, act, "right")
        ad2 = a.double().requires_grad_(True)
        ((F.silu(ad2) if act else ad2) @ w[:-1].double().t() * dy[:, :-1].double()).sum().backward()
        _fails(K.check_linear_f32_smallm_bwd, ad2.grad.float(), dy, w, a, act)         # the last row of W dropped
        _fails(K.check_linear_f32_smallm_bwd, ad.grad.roll(1, 0).float(), dy, w, a, act)
    _fails(K.check_linear_f32_smallm_bwd, (dy.double() @ w.double()).float(), dy, w, a, 1)   # SiLU' forgotten


def test_linear_f32_smallm_forward_check_against_torch_and_teeth():
    M, N, K_ = 17, 33, 1032
    a, w, b = _rn(M, K_, seed=61, scale=2.0, dtype=torch.float32), _rn(N, K_, seed=62, scale=0.05), _rn(N, seed=63)
    for act in (0, 1):
        right = (F.silu(a.double()) if act else a.double()) @ w.double().t() + b.double()
        K.check_linear_f32_smallm(right.float(), a, w, b, act, 0.0, "right")
        K.check_linear_f32_smallm((right - b.double()).float(), a, w, None, act, 0.0, "no bias")
        _fails(K.check_linear_f32_smallm, (right - b.double()).float(), a, w, b, act, 0.0)            # the bias forgotten
        short = (F.silu(a.double()) if act else a.double())[:, :-8] @ w.double()[:, :-8].t() + b.double()
        _fails(K.check_linear_f32_smallm, short.float(), a, w, b, act, 0.0)                          # the last packet of K dropped
        _fails(K.check_linear_f32_smallm, right.roll(1, 0).float(), a, w, b, act, 0.0)               # rows off by one
        wrong = right.clone(); wrong[-1] = wrong[0]
        _fails(K.check_linear_f32_smallm, wrong.float(), a, w, b, act, 0.0)                          # the second row group reads the first
    _fails(K.check_linear_f32_smallm, (a.double() @ w.double().t() + b.double()).float(), a, w, b, 1, 1e-5)   # SiLU forgotten


def test_timestep_embedding_restatement_against_the_oracle_and_teeth():
    t = torch.tensor([0.0, -37.5, 612.0, 1000.0])
    ref, arg = K.timestep_embedding(t, 342, 10000.0)
    assert ref.shape == (4, 342) and torch.equal(ref[0, :171], torch.ones(171, dtype=torch.float64)) and not ref[0, 171:].any()
    assert float(arg.max()) == 1000.0 and torch.equal(arg[:, :171], arg[:, 171:])
    orc = _orc()
    assert (orc.timestep_embedding(t, 256).double() - K.timestep_embedding(t, 256, 10000.0)[0]).abs().max() < 2e-4
    K.check_timestep_embedding(ref.float(), t, 342, 10000.0, "right")
    _fails(K.check_timestep_embedding, torch.cat([ref[:, 171:], ref[:, :171]], 1).float(), t, 342, 10000.0)      # sin in front
    _fails(K.check_timestep_embedding, K.timestep_embedding(t, 342, 9990.0)[0].float(), t, 342, 10000.0)         # another period
    half_off = torch.exp(-math.log(10000.0) * torch.arange(171, dtype=torch.float64) / 170)                       # j / (half - 1)
    arg2 = t.double()[:, None] * half_off
    _fails(K.check_timestep_embedding, torch.cat([arg2.cos(), arg2.sin()], 1).float(), t, 342, 10000.0)


def test_fm_mse_samples_check_against_torch_and_teeth():
    B, C, T, Tc, HW = 3, 3, 2, 1, 35
    pred = _rn(B, C, T, HW, seed=64, dtype=torch.float32)
    eps, x0 = _rn(B, C, T - Tc, HW, seed=65), _rn(1, C, T - Tc, HW, seed=66)
    vt = (eps - x0).double()                                       # the bf16 subtraction, widened
    d = pred.double()[:, :, Tc:] - vt
    right = (d * d).flatten(1).mean(1)
    K.check_fm_mse_samples(right.float(), pred, eps, x0, Tc, "right")
    flat = (d * d).flatten(1)
    _fails(K.check_fm_mse_samples, (flat[:, :-1].sum(1) / flat.shape[1]).float(), pred, eps, x0, Tc)      # the last element dropped
    _fails(K.check_fm_mse_samples, right.roll(1).float(), pred, eps, x0, Tc)                               # samples off by one
    d0 = pred.double()[:, :, :T - Tc] - vt
    _fails(K.check_fm_mse_samples, (d0 * d0).flatten(1).mean(1).float(), pred, eps, x0, Tc)                # the conditioning frames read
    exact = pred.double()[:, :, Tc:] - (eps.double() - x0.double())
    _fails(K.check_fm_mse_samples, (exact * exact).flatten(1).mean(1).float(), pred, eps, x0, Tc)          # the target not rounded to bf16


def test_swiglu_bwd_check_against_autograd_and_teeth():
    rows, Fd = 7, 96
    g, u, d = _rn(rows, Fd, seed=17, scale=2.0), _rn(rows, Fd, seed=18), _rn(rows, Fd, seed=19)
    g[:, ::5] = torch.tensor([30.0, -30.0, 100.0, -100.0]).repeat(5)[: len(range(0, Fd, 5))].to(BF16)
    d[0, 15], u[0, 15] = 8.0, 4.0                        # g = -100 there: |dout up silu'| = 32 * 3.7e-42 > one bf16 subnormal step
    gd = g.double().requires_grad_(True)
    (F.silu(gd) * u.double() * d.double()).sum().backward()
    dgate = gd.grad.to(BF16)
    dup = (d.double() * F.silu(g.double()).to(BF16).double()).to(BF16)
    K.check_swiglu_bwd(dgate, dup, g, u, d, "right")
    # fp32 has no sigmoid(-100) = 3.7e-44 (__expf(100) overflows): a kernel's 0 there is inside the bound, elsewhere it is not
    gd2 = g.double()
    ref15 = (d.double() * u.double() * K.silu_grad(gd2))[0, 15]
    assert g[0, 15] == -100 and abs(float(ref15)) > 2.0 ** -133
    flushed = torch.where(gd2 == -100, torch.zeros_like(gd2), (d.double() * u.double() * K.silu_grad(gd2))).to(BF16)
    dup2 = (d.double() * F.silu(gd2).to(BF16).double()).to(BF16)
    K.check_swiglu_bwd(flushed, dup2, g, u, d, "fp32 underflow")
    _fails(K.check_swiglu_bwd, torch.where(gd2 == -30, torch.zeros_like(gd2), flushed.double()).to(BF16), dup2, g, u, d)
    _fails(K.check_swiglu_bwd, dup, dgate, g, u, d)                                    # the two outputs swapped
    last = dgate.clone()
    last[-1] = 0
    _fails(K.check_swiglu_bwd, last, dup, g, u, d)                                     # the last row dropped
    _fails(K.check_swiglu_bwd, dgate, (d.double() * F.silu(g.double())).to(BF16).roll(1, 1), g, u, d)
    # the interleaved layout read with gate and up columns exchanged
    gi, ui = K.swiglu_il_index(Fd)
    gu = torch.empty(rows, 2 * Fd, dtype=BF16)
    gu[:, gi], gu[:, ui] = g, u
    K.check_swiglu_bwd(dgate, dup, gu[:, gi], gu[:, ui], d, "right, through the layout")
    _fails(K.check_swiglu_bwd, dgate, dup, gu[:, ui], gu[:, gi], d)


def _qk_case(rope=True):
    B, N, H = 2, 3, 5
    x = _rn(B, N, H, 128, seed=20, scale=1.5)
    x = (x.double() * torch.logspace(-3, 1.5, H, dtype=torch.float64)[:, None]).to(BF16)
    w = (1.0 + _rn(128, seed=21, scale=0.2).double()).to(BF16)
    th = torch.rand(N + 1, 64, generator=_g(22), dtype=torch.float64) * 6.2832
    cs = torch.stack([torch.cos(th), torch.sin(th)], -1).float() if rope else None
    return x, w, cs, float(torch.tensor(1e-6)), 261 / 2048


def _qk_fwd(x, w, cs, eps, scale, round_inner=True):
    """The forward another way: torch's rms_norm arithmetic by hand and the rotation as a complex product."""
    rnd = (lambda t: t.to(BF16).double()) if round_inner else (lambda t: t)
    xd = x.double() if not x.requires_grad else x
    n = rnd(rnd(xd * torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + eps)) * (w if w.requires_grad else w.double()))
    if cs is not None:
        rot = torch.view_as_complex(cs.double().contiguous())[None, :, None, :]
        n = torch.view_as_real(torch.view_as_complex(n.reshape(*n.shape[:-1], 64, 2).contiguous()) * rot).flatten(-2)
    return n * scale


@pytest.mark.parametrize("rope", [True, False])
def test_qknorm_rope_fwd_check_has_teeth(rope):
    x, w, cs, eps, scale = _qk_case(rope)
    rows = None if cs is None else cs[:3]
    right = _qk_fwd(x, w, rows, eps, scale).to(BF16)
    assert K.check_qknorm_rope_fwd(right, x, w, rows, eps, scale, "right") <= 0.5
    _fails(K.check_qknorm_rope_fwd, right[:, :, [0, 1, 3, 2, 4]], x, w, rows, eps, scale)          # two heads swapped
    _fails(K.check_qknorm_rope_fwd, right.roll(1, 0), x, w, rows, eps, scale)                      # the batches exchanged
    _fails(K.check_qknorm_rope_fwd, (right.double() / scale).to(BF16), x, w, rows, eps, scale)     # q_scale forgotten
    _fails(K.check_qknorm_rope_fwd, _qk_fwd(x, w.roll(8), rows, eps, scale).to(BF16), x, w, rows, eps, scale)
    if rope:
        _fails(K.check_qknorm_rope_fwd, _qk_fwd(x, w, cs[1:4], eps, scale).to(BF16), x, w, rows, eps, scale)   # position + 1
        _fails(K.check_qknorm_rope_fwd, _qk_fwd(x, w, None, eps, scale).to(BF16), x, w, rows, eps, scale)      # no rotation
        conj = rows.clone()
        conj[..., 1] *= -1
        _fails(K.check_qknorm_rope_fwd, _qk_fwd(x, w, conj, eps, scale).to(BF16), x, w, rows, eps, scale)      # rotated backwards
    # one element moved by the outer rounding's ulp and the two inner flips (3 ulps) stays inside the bound, a fourth ulp does
    # not: the bound is rule 5, not more
    lone = right.clone()
    lone.view(torch.int16)[0, 0, 4, 7] += 3
    assert K.check_qknorm_rope_fwd(lone, x, w, rows, eps, scale, "three ulps") > 0.9
    lone.view(torch.int16)[0, 0, 4, 7] += 1
    _fails(K.check_qknorm_rope_fwd, lone, x, w, rows, eps, scale)


@pytest.mark.parametrize("rope", [True, False])
def test_qknorm_rope_bwd_restatement_against_autograd_and_teeth(rope):
    x, w, cs, eps, scale = _qk_case(rope)
    rows = None if cs is None else cs[:3]
    dout = _rn(*x.shape, seed=23)
    xd, wd = x.double().requires_grad_(True), w.double().requires_grad_(True)
    (_qk_fwd(xd, wd, rows, eps, scale, round_inner=False) * dout.double()).sum().backward()
    dx, dw, _ = K.qknorm_rope_bwd(x, dout, w, rows, eps, scale)
    assert torch.allclose(dx, xd.grad, rtol=1e-10, atol=1e-13)
    # the kernel's dw is the gradient w.r.t. the weight as it enters the forward, q_scale included
    assert torch.allclose(dw, wd.grad, rtol=1e-10, atol=1e-13)
    right_dx = xd.grad.to(BF16)
    slots = torch.zeros(3, 128, dtype=torch.float64)
    for b in range(2):                                   # token n of batch b adds into row (n + b N) % slots
        for n in range(3):
            slots[(n + b * 3) % 3] += K.qknorm_rope_bwd(x[b: b + 1, n: n + 1], dout[b: b + 1, n: n + 1], w,
                                                        None if rows is None else rows[n: n + 1], eps, scale)[1]
    right_dw = slots.float()
    K.check_qknorm_rope_bwd(right_dx, right_dw, x, dout, w, rows, eps, scale, "right")
    K.check_qknorm_rope_bwd(right_dx, None, x, dout, w, rows, eps, scale, "right, no dw")
    _fails(K.check_qknorm_rope_bwd, right_dx[:, :, [1, 0, 2, 3, 4]], right_dw, x, dout, w, rows, eps, scale)   # two heads swapped
    _fails(K.check_qknorm_rope_bwd, right_dx, right_dw[:2], x, dout, w, rows, eps, scale)                      # a slot not summed
    _fails(K.check_qknorm_rope_bwd, right_dx, right_dw / scale, x, dout, w, rows, eps, scale)                  # dw without q_scale
    _fails(K.check_qknorm_rope_bwd, (xd.grad / scale).to(BF16), None, x, dout, w, rows, eps, scale)
    nodot = (K.qknorm_rope_bwd(x, dout, w, rows, eps, scale)[2])
    _fails(K.check_qknorm_rope_bwd, (nodot["r"] * nodot["dn"]).to(BF16), None, x, dout, w, rows, eps, scale)   # the dot term dropped
    if rope:
        shifted = K.qknorm_rope_bwd(x, dout, w, cs[1:4], eps, scale)
        _fails(K.check_qknorm_rope_bwd, shifted[0].to(BF16), right_dw, x, dout, w, rows, eps, scale)           # position + 1
        _fails(K.check_qknorm_rope_bwd, right_dx, shifted[1].float()[None], x, dout, w, rows, eps, scale)


def test_t5_rmsnorm_and_geglu_checks_have_teeth():
    rows, C = 5, 520
    x, w = _rn(rows, C, seed=24, scale=3.0), (1.0 + _rn(C, seed=25, scale=0.3).double()).to(BF16)
    eps = float(torch.tensor(1e-6))
    xd = x.double()
    right = (w.double() * (xd * torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + eps)).to(BF16).double()).to(BF16)
    assert K.check_t5_rmsnorm(right, x, w, eps, "right") <= 0.5
    last = right.clone()
    last[-1] = right[-2]
    _fails(K.check_t5_rmsnorm, last, x, w, eps)                                        # the last row dropped
    _fails(K.check_t5_rmsnorm, right.roll(8, 1), x, w, eps)                            # one packet off
    mean_removed = (w.double() * F.layer_norm(xd, (C,), eps=eps)).to(BF16)
    _fails(K.check_t5_rmsnorm, mean_removed, x, w, eps)                                # a LayerNorm, not T5's RMS norm
    wrongc = (w.double() * (xd * torch.rsqrt(xd.pow(2).sum(-1, keepdim=True) / 512 + eps)).to(BF16).double()).to(BF16)
    _fails(K.check_t5_rmsnorm, wrongc, x, w, eps)                                      # mean over 512 instead of C
    g, u = _rn(rows, C, seed=26, scale=2.0), _rn(rows, C, seed=27)
    g[:, ::3] = torch.linspace(-30, 30, len(range(0, C, 3))).to(BF16)
    right = (F.gelu(g.double(), approximate="tanh").to(BF16).double() * u.double()).to(BF16)
    assert K.check_geglu_tanh(right, g, u, "right") <= 0.5
    # what fp32 does in the tail (tanhf = -1 exactly, gelu = -0) is inside the bound
    flushed = torch.where(g.double() < -6, torch.zeros_like(right), right)
    K.check_geglu_tanh(flushed, g, u, "fp32 tail")
    last = right.clone()
    last[-1] = 0
    _fails(K.check_geglu_tanh, last, g, u)                                             # the last row dropped
    _fails(K.check_geglu_tanh, (F.gelu(g.double()).to(BF16).double() * u.double()).to(BF16), g, u)   # erf form
    _fails(K.check_geglu_tanh, (F.gelu(u.double(), approximate="tanh").to(BF16).double() * g.double()).to(BF16), g, u)


def _attention_by_hand(q, k, v, bias, mask):
    """softmax with an additive -inf mask through torch.softmax; rows without a key are zero."""
    B, S, H, _ = q.shape
    i = torch.arange(S)
    sc = torch.einsum("bihd,bjhd->bhij", q.double(), k.double()).to(BF16).double()
    sc = (sc + bias.double()[:, i[None, :] - i[:, None] + S - 1][None]).to(BF16).double()
    sc = sc.masked_fill(mask[:, None, None, :] == 0, float("-inf"))
    p = torch.softmax(sc, -1).nan_to_num(0.0).to(BF16).double()
    return torch.einsum("bhij,bjhd->bihd", p, v.double()).to(BF16)


def test_t5_attention_check_has_teeth():
    B, S, H = 2, 65, 3
    g = _g(28)
    q, k = ((torch.randint(-1, 2, (B, S, H, 64), generator=g).float() / 4).to(BF16) for _ in range(2))
    v = torch.randn(B, S, H, 64, generator=g).to(BF16)
    d = torch.arange(-(S - 1), S)
    bias = (((7 * d[None, :] + 13 * torch.arange(H)[:, None]) % 129) - 64).float() / 16
    mask = torch.ones(B, S, dtype=torch.int32)
    mask[0, 40:] = 0
    mask[1, ::3] = 0
    right = _attention_by_hand(q, k, v, bias, mask)
    assert K.check_t5_attention(right, q, k, v, bias, mask, "right") <= 0.5
    _fails(K.check_t5_attention, _attention_by_hand(q, k, v, bias.flip(1), mask), q, k, v, bias, mask)      # bias by i - j
    _fails(K.check_t5_attention, _attention_by_hand(q, k, v, bias.roll(1, 0), mask), q, k, v, bias, mask)   # another head's bias
    _fails(K.check_t5_attention, _attention_by_hand(q, k, v, bias, mask[[0, 0]]), q, k, v, bias, mask)      # batch 0's mask for batch 1
    _fails(K.check_t5_attention, right[:, :, [0, 2, 1]], q, k, v, bias, mask)                               # two heads swapped
    nolast = mask.clone()
    nolast[1, S - 1] = 0
    _fails(K.check_t5_attention, _attention_by_hand(q, k, v, bias, nolast), q, k, v, bias, mask)            # the last key dropped
    _fails(K.check_t5_attention, _attention_by_hand(q / 8, k, v, bias, mask), q, k, v, bias, mask)          # a 1/sqrt(d) scaling
    # a fully masked batch row is exactly zero; anything else there fails
    mask[1] = 0
    right = _attention_by_hand(q, k, v, bias, mask)
    assert (right[1] == 0).all()
    K.check_t5_attention(right, q, k, v, bias, mask, "right, batch 1 masked")
    stale = right.clone()
    stale[1, 7, 2, 5] = 2.0 ** -100
    _fails(K.check_t5_attention, stale, q, k, v, bias, mask)


# ------------------------------------------------------------------------------ the flash-attention checks (tests/attn_cases.py)
def _t(a):
    return a.permute(0, 2, 1, 3)


def _orc():
    import sys
    if str(ROOT) not in sys.path:
        sys.path.insert(0, str(ROOT))
    from oracle import dit_oracle
    return dit_oracle


# the inputs of every small GPU case, each once: (Nq, Nk, unit, B, H)
ATTN_FWD_INPUTS = sorted({(nq, nk, unit, AC.B0, AC.H0) for _, nq, nk, unit, _ in AC.FWD_CASES}
                         | {(AC.WIDE_CASE["Nq"], AC.WIDE_CASE["Nk"], True, AC.WIDE_CASE["B"], AC.WIDE_CASE["H"])})
ATTN_BWD_INPUTS = sorted({(nq, nk, unit, AC.B0, AC.H0) for nq, nk in AC.BWD_CASES + AC.SPLIT_CASES for unit in (False, True)})
assert all(AC.is_small(b, h, nq, nk) for nq, nk, _, b, h in ATTN_FWD_INPUTS + ATTN_BWD_INPUTS)
assert not any(AC.is_small(b, h, nq, nk) for b, h, nq, nk in AC.SPLIT_PAIR)      # B H = 255 / 256: GPU only


def _ragged(nq, nk):
    return nq % 32 != 0 or nk % 64 != 0


@pytest.mark.parametrize("Nq,Nk,unit,B,H", sorted(set(ATTN_FWD_INPUTS) | set(ATTN_BWD_INPUTS)))
def test_attention_cases_hold_what_the_bounds_and_the_corruptions_rest_on(Nq, Nk, unit, B, H):
    """CPU: exactness in fp32, the heavy keys' shares, the rescale pattern per 32-row group, distinct heads."""
    c = AC.inputs(Nq, Nk, unit, B, H)
    q, k = _t(c["q"]).double(), _t(c["k"]).double()
    for x in (q, k):
        assert torch.equal(x * 2, (x * 2).round())                              # multiples of 1/2 ...
    ordinary_rows = [r for r in range(Nq) if r not in (4, 5)] if Nq >= 8 else list(range(Nq))
    pl = AC.planted(Nq, Nk)
    ordinary_keys = [j for j in range(Nk) if j not in set(pl["heavy"]) | {pl["j0"], pl["j1"], pl["j2"]}]
    assert q[:, :, ordinary_rows].abs().max() <= 0.5 and (not ordinary_keys or k[:, :, ordinary_keys].abs().max() <= 0.5)
    # ... so every partial sum of q . k, in any order and from any start that is itself such a sum (the running max), is a
    # multiple of 1/4 bounded by 2 sum |q||k| < 2^13: 15 significant bits, exact in fp32
    mag = q.abs() @ k.abs().transpose(-1, -2)
    qk = q @ k.transpose(-1, -2)
    assert 2 * mag.max() < 2 ** 13 and torch.equal(qk * 4, (qk * 4).round()) and torch.equal(qk.float().double(), qk)
    x = qk * (c["scale"] * K.LOG2E)
    p = torch.softmax(x / K.LOG2E, -1)
    # heavy keys: each carries >= 1/4 of rows 0 and Nq - 1, and (where there is more than one key) none carries all of it
    for r in {0, Nq - 1}:
        share = p[:, :, r][..., pl["heavy"]]
        assert share.min() >= 0.25 and (Nk == 1 or share.max() <= 0.75), (r, share.min(), share.max())
    assert (Nk - 1) in pl["heavy"] and 64 * ((Nk - 1) // 64) in pl["heavy"]
    if Nq >= 8:
        assert x[:, :, 4].max() < -40 and x[:, :, 5].min() > 250 and x[:, :, 5].max() < 350
        growth, rescaled, before = AC.schedule(x)
        if pl["t1"] is not None:      # tile t1: key j1 lifts row 1 by more than the threshold and lies far below row 2's running max
            t1, j1 = pl["t1"], pl["j1"]
            assert growth[t1][..., 1].min() > AC.THR and rescaled[t1][..., 0].all()
            assert (x[..., 1, j1] - before[t1][..., 1]).min() > AC.THR and (x[..., 2, j1] - before[t1][..., 2]).max() < -40
        if pl["t2"] is not None:      # tile t2: row 3 grows by (0, THR], no row of its group by more: no rescale
            g = growth[pl["t2"]]
            assert g[..., 3].min() > 0 and g[..., 3].max() <= AC.THR and not rescaled[pl["t2"]][..., 0].any()
    # every (batch, head) differs from every other in q, k, v and dO
    for name in ("q", "k", "v", "d_o"):
        flat = _t(c[name]).reshape(B * H, -1)
        assert all(not torch.equal(flat[i], flat[j]) for i in range(B * H) for j in range(i))


def test_every_forward_body_has_a_case_with_the_rescale_pattern():
    for body in (AC.FWD_SHORT, AC.FWD_GENERAL, AC.FWD_W64, AC.FWD_PIPE):
        assert any(AC.planted(nq, nk)["t1"] is not None and AC.planted(nq, nk)["t2"] is not None
                   for b, nq, nk, _, _ in AC.FWD_CASES if b == body), body
    pl = AC.planted(AC.WIDE_CASE["Nq"], AC.WIDE_CASE["Nk"])
    assert pl["t1"] is not None and pl["t2"] is not None
    # the unit-scale short-key body sees the negative first maximum of row 4 too
    assert any(b == AC.FWD_SHORT and unit and nq >= 8 for b, nq, _, unit, _ in AC.FWD_CASES)


def test_attention_workspace_formula_is_the_librarys():
    """lcv_attn_bwd_ws_floats is host-only: the size the header documents, with attn_bwd_qsplit restated from its source comment."""
    import sys
    if str(ROOT) not in sys.path:
        sys.path.insert(0, str(ROOT))
    import __graft_entry__ as ge
    ge.build()                          # (cheap when the library is up to date; this test must also pass when run alone)
    from lcv_hip import lib as L
    f = L.load().lcv_attn_bwd_ws_floats
    shapes = [(AC.B0, AC.H0, nq, nk) for nq, nk in AC.BWD_CASES + AC.SPLIT_CASES] + AC.SPLIT_PAIR
    for b, h, nq, nk in shapes:
        assert f(b, h, nq, nk) == AC.ws_floats(b, h, nq, nk), (b, h, nq, nk)
    assert [AC.qsplit(AC.B0, AC.H0, nq, 77) for nq in (2016, 2017, 2080)] == [1, 4, 4]
    assert [AC.qsplit(b, h, nq, nk) for b, h, nq, nk in AC.SPLIT_PAIR] == [2, 1]


def _fwd_parts(c):
    qf, kf, vf = (K._bhnd(c[n]) for n in ("q", "k", "v"))
    s = (qf @ kf.transpose(-1, -2)) * c["scale"]
    m = s.amax(-1, keepdim=True)
    return s, m, torch.exp(s - m), vf


def _fwd_from_weights(w_num, w_den, m, vf):
    l = w_den.sum(-1, keepdim=True)
    return _t((w_num @ vf) / l), (m + torch.log(l)).squeeze(-1)


@pytest.mark.parametrize("Nq,Nk,unit,B,H", ATTN_FWD_INPUTS)
def test_check_attn_fwd_passes_the_tile_restatement_and_fails_the_bugs(Nq, Nk, unit, B, H, capsys):
    orc = _orc()
    c = AC.inputs(Nq, Nk, unit, B, H)
    args = (c["q"], c["k"], c["v"], c["scale"])
    o, lse = orc.sdpa_at_kernel_rounding(_t(c["q"]), _t(c["k"]), _t(c["v"]), c["scale"], return_lse=True)
    worst = K.check_attn_fwd(_t(o).to(torch.bfloat16), lse, *args, "tile restatement", exact_scores=True)
    K.check_attn_fwd(_t(o).to(torch.bfloat16), lse, *args, "tile restatement, general bound")
    with capsys.disabled():
        print(f"\ncheck_attn_fwd {Nq}x{Nk} unit={unit}: restatement at {worst:.3f} of the bound", end="")
    if not _ragged(Nq, Nk):
        return
    s, m, w, vf = _fwd_parts(c)
    right = _fwd_from_weights(w, w, m, vf)
    K.check_attn_fwd(*right, *args, "float64", exact_scores=True)

    def bad(o_lse):
        _fails(lambda what: K.check_attn_fwd(*o_lse, *args, what, exact_scores=True))

    def bad_o(o_lse):                  # the output alone must give it away
        _fails(lambda what: K.check_attn_fwd(o_lse[0], None, *args, what, exact_scores=True))
    pl = AC.planted(Nq, Nk)
    if Nk > 1:
        twice = w.clone(); twice[..., Nk - 1] *= 2                      # the clamped last key counted twice
        bad_o(_fwd_from_weights(twice, twice, m, vf))
        for j in {Nk - 1, 64 * ((Nk - 1) // 64)}:                        # the last key / the first key of the last tile dropped
            drop = w.clone(); drop[..., j] = 0
            bad_o(_fwd_from_weights(drop, drop, m, vf))
    if Nq > 1 and Nk > 1:             # (with one key every row's output is v)
        swapped = right[0].clone(); swapped[:, [Nq - 2, Nq - 1]] = swapped[:, [Nq - 1, Nq - 2]]
        bad_o((swapped, right[1]))
    heads = right[0].clone(); heads[:, :, [0, 1]] = heads[:, :, [1, 0]]
    bad_o((heads, right[1]))
    for t0 in {0, 64 * ((Nk - 1) // 64)}:                                # one tile's PV contribution doubled (l is right)
        num = w.clone(); num[..., t0: t0 + 64] *= 2
        bad_o(_fwd_from_weights(num, w, m, vf))
    if pl["t1"] is not None:          # O not rescaled after the jump of row 1 in tile t1: what came before stays 2^d too large
        x = s * K.LOG2E
        d = x[..., 1, :].amax(-1) - x[..., 1, : 64 * pl["t1"]].amax(-1)
        num = w.clone(); num[..., 1, : 64 * pl["t1"]] *= torch.exp2(d).unsqueeze(-1)
        bad_o(_fwd_from_weights(num, w, m, vf))
    bad((right[0], right[1] * K.LOG2E))                                  # lse in log2 units


def _bwd_inputs(c):
    o64, lse64, _, _ = K.attn_fwd(c["q"], c["k"], c["v"], c["scale"])
    return _t(o64).to(torch.bfloat16), lse64.float()


@pytest.mark.parametrize("Nq,Nk,unit,B,H", ATTN_BWD_INPUTS)
def test_check_attn_bwd_passes_the_rounding_point_restatement_and_fails_the_bugs(Nq, Nk, unit, B, H, capsys):
    orc = _orc()
    c = AC.inputs(Nq, Nk, unit, B, H)
    o_in, lse_in = _bwd_inputs(c)
    args = (c["q"], c["k"], c["v"], o_in, c["d_o"], lse_in, c["scale"])
    qs = AC.qsplit(B, H, Nq, Nk)
    worst = [0.0, 0.0, 0.0]
    for inside in (True, False):
        got = orc.sdpa_backward_at_kernel_rounding(_t(c["q"]), _t(c["k"]), _t(c["v"]), _t(c["d_o"]), c["scale"], scale_inside=inside,
                                                   o=_t(o_in), lse=lse_in)
        got = [_t(g).to(torch.bfloat16) for g in got]
        w3 = K.check_attn_bwd(*got, *args, inside, what=f"restatement inside={inside}", qsplit=qs, exact_scores=True)
        worst = [max(a, b) for a, b in zip(worst, w3)]
        K.check_attn_bwd(*got, *args, inside, what=f"restatement inside={inside}, general bound", qsplit=qs)
    with capsys.disabled():
        print(f"\ncheck_attn_bwd {Nq}x{Nk} unit={unit}: restatement at dq {worst[0]:.3f} dk {worst[1]:.3f} dv {worst[2]:.3f} of the bound", end="")
    if not _ragged(Nq, Nk):
        return
    rq, rk, rv, m = K.attn_bwd(*args)
    ds, qf, kf = m["ds"], m["qf"], m["kf"]
    right = [_t(r) for r in (rq, rk, rv)]
    K.check_attn_bwd(*right, *args, True, what="float64", qsplit=qs, exact_scores=True)

    def bad(dq, dk, dv, inside=True, **kw):
        with pytest.raises(AssertionError):
            K.check_attn_bwd(dq, dk, dv, *args, inside, what="wrong on purpose", qsplit=qs, exact_scores=True, **kw)
    # an operand rounded more coarsely than bf16 (4 significant bits, as an fp8 e4m3 operand would be) on either side of the scale;
    # with one key dS is exactly 0 (o = v, so dP = delta)
    if Nk > 1:
        coarse = torch.ldexp(torch.round(torch.ldexp(torch.frexp(ds)[0], torch.tensor(4))), torch.frexp(ds)[1] - 4)
        for inside in (True, False):
            bad(_t(coarse @ kf), _t(coarse.transpose(-1, -2) @ qf), right[2], inside)
    last = 32 * ((Nq - 1) // 32)                                          # dK, dV without the last query tile
    if Nk > 1:
        bad(right[0], _t(ds[..., :last, :].transpose(-1, -2) @ qf[..., :last, :]), right[2])
    bad(right[0], right[1], _t(m["p"][..., :last, :].transpose(-1, -2) @ m["gf"][..., :last, :]))
    if qs > 1:                                                            # one split's slice added twice
        nt = (Nq + 31) // 32
        a, b = 32 * (nt * 1 // qs), 32 * (nt * 2 // qs)
        bad(right[0], _t(rk + ds[..., a:b, :].transpose(-1, -2) @ qf[..., a:b, :]), right[2])
    if Nq > 1 and Nk > 1:
        swapped = right[0].clone(); swapped[:, [Nq - 2, Nq - 1]] = swapped[:, [Nq - 1, Nq - 2]]
        bad(swapped, right[1], right[2])
    heads = right[2].clone(); heads[:, :, [0, 1]] = heads[:, :, [1, 0]]
    bad(right[0], right[1], heads)
    # accumulate_kv: right, ignored, applied twice
    pk, pv = c["prev_dk"], c["prev_dv"]
    K.check_attn_bwd(right[0], right[1] + pk.double(), right[2] + pv.double(), *args, True, pk, pv, what="accumulated", qsplit=qs,
                     exact_scores=True)
    bad(right[0], right[1], right[2] + pv.double(), prev_dk=pk, prev_dv=pv)
    bad(right[0], right[1] + pk.double(), right[2], prev_dk=pk, prev_dv=pv)
    bad(right[0], right[1] + 2 * pk.double(), right[2] + pv.double(), prev_dk=pk, prev_dv=pv)
    bad(right[0], right[1] + pk.double(), right[2] + 2 * pv.double(), prev_dk=pk, prev_dv=pv)


def test_the_side_of_the_scale_is_detectable_only_where_few_operands_carry_an_element():
    """dS rounded to bf16 on the WRONG side of a scale that is no power of two (dS' = dS / scale rounded where dS should be, or
    the reverse).  The two roundings differ by at most half an ulp of the coarser side, i.e. at most twice the half ulp the bound
    grants the right side, and every element also has its own output ulp and the other operands' terms on top.  So the wrong
    side is rejected only on elements that a few dS entries carry (short key or query sweeps, one dominant probability) and
    whose entries sit low in their binade on one side of the scale and high on the other; on long sweeps the difference
    averages out far below the bound.  Counted here over the short backward cases: some are rejected, most are not."""
    orc = _orc()
    rejected, total = [], 0
    for Nq, Nk, unit, B, H in ATTN_BWD_INPUTS:
        if Nq > 33 or Nk == 1:
            continue
        c = AC.inputs(Nq, Nk, unit, B, H)
        o_in, lse_in = _bwd_inputs(c)
        for inside in (True, False):
            got = orc.sdpa_backward_at_kernel_rounding(_t(c["q"]), _t(c["k"]), _t(c["v"]), _t(c["d_o"]), c["scale"], scale_inside=inside,
                                                       o=_t(o_in), lse=lse_in)
            got = [_t(g).to(torch.bfloat16) for g in got]
            total += 1
            try:
                K.check_attn_bwd(*got, c["q"], c["k"], c["v"], o_in, c["d_o"], lse_in, c["scale"], not inside, what="wrong side",
                                 exact_scores=True)
            except AssertionError:
                rejected.append((Nq, Nk, unit, inside))
    print(f"wrong side of the scale rejected in {len(rejected)} of {total} restatements: {rejected}")
    assert 0 < len(rejected) < total / 2


# ----------------------------------------------------------------------------------------------------- coverage guard
# entry point -> [(test file, test function)] that checks its kernel at kernel level
KERNEL_TESTS = {
    "lcv_adaln_modulate_fwd": [(EDGES, "test_norm_and_gate_residual_fwd_edges"), ("test_gpu_kernels.py", "test_adaln_modulate")],
    "lcv_adaln_modulate_bwd": [(EDGES, "test_adaln_and_layernorm_bwd_edges")],
    "lcv_layernorm_affine_fwd": [(EDGES, "test_norm_and_gate_residual_fwd_edges"), ("test_gpu_kernels.py", "test_layernorm_affine")],
    "lcv_layernorm_affine_bwd": [(EDGES, "test_adaln_and_layernorm_bwd_edges")],
    "lcv_gate_residual_fwd": [(EDGES, "test_norm_and_gate_residual_fwd_edges"),
                              (EDGES, "test_gate_residual_fwd_without_gate_past_the_block_cap")],
    "lcv_gate_residual_bwd": [(EDGES, "test_gate_residual_bwd_edges")],
    "lcv_qknorm_rope_fwd": [("test_gpu_kernels.py", "test_qknorm_rope"), (BWD_EDGES, "test_qknorm_rope_fwd_edges"),
                            (BWD_EDGES, "test_qknorm_rope_fwd_leaves_v_alone_when_v_out_is_v_in")],
    "lcv_qknorm_rope_bwd": [("test_gpu_backward.py", "test_qknorm_rope_backward"),
                            ("test_gpu_backward.py", "test_qk_norm_weight_gradients"), (BWD_EDGES, "test_qknorm_rope_bwd_edges")],
    "lcv_timestep_embedding": [("test_gpu_kernels.py", "test_timestep_embedding_matches_oracle"),
                               (EDGES, "test_timestep_embedding_edges"),
                               (EDGES, "test_timestep_embedding_refuses_odd_dim_and_periods_up_to_one")],
    "lcv_attn_fwd": [("test_gpu_kernels.py", "test_attention_fuzz_against_the_restatement_of_the_kernels_arithmetic"),
                     (ATTN_EDGES, "test_attn_fwd_edges"), (ATTN_EDGES, "test_attn_fwd_wide_key_stride_takes_the_64_bit_body")],
    "lcv_attn_bwd": [("test_gpu_backward.py", "test_attention_backward_fuzz_against_the_kernels_rounding_points"),
                     (ATTN_EDGES, "test_attn_bwd_edges"), (ATTN_EDGES, "test_attn_bwd_split_query_sweep"),
                     (ATTN_EDGES, "test_attn_bwd_refuses_bad_strides_and_misaligned_pointers")],
    "lcv_gemm_nt": [("test_gpu_kernels.py", "test_gemm_dispatch_fuzz_bitwise_against_the_one_barrier_kernel"),
                    ("test_gpu_kernels.py", "test_gemm_nt_lora_and_epilogues")],
    "lcv_lora_down": [("test_gpu_kernels.py", "test_gemm_nt_lora_and_epilogues"), (LORA_EDGES, "test_lora_down_edges"),
                      (LORA_EDGES, "test_lora_down_rejects_rank_33")],
    "lcv_tn_skinny": [("test_gpu_backward.py", "test_linear_f32_backward_and_tn_skinny_and_unpatchify"),
                      (LORA_EDGES, "test_tn_skinny_workspace_path_edges"), (LORA_EDGES, "test_tn_skinny_atomic_path_edges"),
                      (LORA_EDGES, "test_tn_skinny_rejects_a_small_or_misaligned_workspace")],
    "lcv_linear_f32_smallm": [("test_gpu_kernels.py", "test_linear_f32_smallm"), (EDGES, "test_linear_f32_smallm_edges"),
                              (EDGES, "test_linear_f32_smallm_silu_error"),
                              (EDGES, "test_linear_f32_smallm_refuses_what_it_cannot_stage")],
    "lcv_linear_f32_smallm_bwd": [("test_gpu_backward.py", "test_linear_f32_backward_and_tn_skinny_and_unpatchify"),
                                  (BWD_EDGES, "test_linear_f32_smallm_bwd_edges")],
    "lcv_swiglu_fwd": [(EDGES, "test_swiglu_fwd_on_views_into_one_buffer_past_the_block_cap")],
    "lcv_swiglu_bwd": [("test_gpu_backward.py", "test_norm_gate_swiglu_backward"),
                       (BWD_EDGES, "test_swiglu_bwd_on_views_into_one_buffer_past_the_block_cap_and_in_saturation")],
    "lcv_swiglu_bwd_interleaved": [("test_gpu_backward.py", "test_fused_swiglu_training_path_matches_the_unfused_form"),
                                   (BWD_EDGES, "test_swiglu_bwd_interleaved_edges_and_equals_swiglu_bwd_bitwise")],
    "lcv_patchify": [(EDGES, "test_patchify_pad_and_unpatchify_past_the_block_cap")],
    "lcv_unpatchify": [(EDGES, "test_patchify_pad_and_unpatchify_past_the_block_cap")],
    "lcv_unpatchify_bwd": [(EDGES, "test_patchify_pad_and_unpatchify_past_the_block_cap")],
    "lcv_cfg_euler_step": [(EDGES, "test_cfg_euler_step_edges")],
    "lcv_euler_step": [(EDGES, "test_euler_step_edges")],
    "lcv_fm_noise": [(EDGES, "test_fm_noise_past_the_block_cap")],
    "lcv_fm_mse": [(EDGES, "test_fm_mse_past_the_block_cap_and_deterministic")],
    "lcv_fm_mse_samples": [("test_gpu_early_stopping.py", "test_fm_mse_samples_matches_torch_and_is_deterministic"),
                           (EDGES, "test_fm_mse_samples_edges"),
                           (EDGES, "test_fm_mse_samples_refuses_overlapping_strides_and_no_target_frame")],
    "lcv_grad_norm_clip": [("test_gpu_backward.py", "test_fused_adamw_clip_matches_reference_trace"),
                           ("test_gpu_backward.py", "test_joint_clip_over_bf16_and_fp32_parameters_matches_torch"),
                           (OPTIM_EDGES, "test_step_bits"), (OPTIM_EDGES, "test_301_tensors_one_clipped_step_bits")],
    "lcv_adamw_step": [("test_gpu_backward.py", "test_fused_adamw_clip_matches_reference_trace"), (OPTIM_EDGES, "test_step_bits"),
                       (OPTIM_EDGES, "test_301_tensors_one_clipped_step_bits"),
                       (OPTIM_EDGES, "test_fp32_step_and_master_weight_step_with_fp32_gradient_are_one_arithmetic"),
                       (OPTIM_EDGES, "test_special_elements"), (OPTIM_EDGES, "test_torch_device_optimizer_against_the_restatement")],
    "lcv_sgd_step": [("test_gpu_backward.py", "test_fused_sgd_clip_matches_torch"), (OPTIM_EDGES, "test_step_bits"),
                     (OPTIM_EDGES, "test_301_tensors_one_clipped_step_bits"),
                     (OPTIM_EDGES, "test_sgd_packet_path_and_element_path_are_one_arithmetic"),
                     (OPTIM_EDGES, "test_fp32_step_and_master_weight_step_with_fp32_gradient_are_one_arithmetic"),
                     (OPTIM_EDGES, "test_special_elements"), (OPTIM_EDGES, "test_torch_device_optimizer_against_the_restatement")],
    "lcv_transpose_pad": [(EDGES, "test_transpose_pad_and_rowsum_edges")],
    "lcv_rowsum": [(EDGES, "test_transpose_pad_and_rowsum_edges"), (EDGES, "test_rowsum_cols_not_a_multiple_of_512")],
    "lcv_linear_f32_smallm_wgrad": [(EDGES, "test_linear_f32_smallm_wgrad_edges")],
    "lcv_gelu_tanh_fwd": [(EDGES, "test_gelu_tanh_fwd_bwd_past_the_block_cap_and_in_saturation")],
    "lcv_gelu_tanh_bwd": [(EDGES, "test_gelu_tanh_fwd_bwd_past_the_block_cap_and_in_saturation")],
    "lcv_causal_conv3d": [("test_gpu_vae.py", "test_conv_kernel_against_conv3d"), ("test_gpu_vae.py", "test_row_tile_conv_kernel"),
                          ("test_gpu_vae.py", "test_wide_conv_kernel_many_tiles")],
    "lcv_conv3d_strided": [("test_gpu_vae.py", "test_strided_conv_kernel_against_torch")],
    "lcv_vae_rmsnorm_silu": [(EDGES, "test_vae_rmsnorm_silu_edges")],
    "lcv_softmax_rows": [(EDGES, "test_softmax_rows_edges"), (EDGES, "test_softmax_rows_rejects_a_scale_the_max_shift_does_not_guard")],
    "lcv_frame_metric_partials": [("test_gpu_eval.py", "test_sqerr_and_gaussian_ssim_match_oracle"),
                                  ("test_gpu_eval.py", "test_rejects_bad_arguments")],
    "lcv_frame_sqerr": [("test_gpu_eval.py", "test_sqerr_and_gaussian_ssim_match_oracle")],
    "lcv_frame_ssim": [("test_gpu_eval.py", "test_sqerr_and_gaussian_ssim_match_oracle"),
                       ("test_gpu_eval.py", "test_uniform7_ssim_matches_oracle")],
    "lcv_gather_rows": [("test_gpu_umt5.py", "test_gather_norm_geglu_kernels"),
                        (UMT5_EDGES, "test_gather_rows_past_the_block_cap_with_clamped_ids")],
    "lcv_t5_rmsnorm": [("test_gpu_umt5.py", "test_gather_norm_geglu_kernels"), (UMT5_EDGES, "test_t5_rmsnorm_edges"),
                       (UMT5_EDGES, "test_t5_rmsnorm_rejects_c_4104")],
    "lcv_geglu_tanh_fwd": [("test_gpu_umt5.py", "test_gather_norm_geglu_kernels"),
                           (UMT5_EDGES, "test_geglu_tanh_fwd_on_views_into_one_buffer_past_the_block_cap_and_in_saturation")],
    "lcv_t5_attention": [("test_gpu_umt5.py", "test_attention_kernel_matches_oracle"), (UMT5_EDGES, "test_t5_attention_edges"),
                         (UMT5_EDGES, "test_t5_attention_rejects_s_513")],
}

# host-only entry points: no kernel behind them
EXEMPT = {
    "lcv_version": "version",
    "lcv_last_error": "error",
    "lcv_device_check": "device",
    "lcv_knobs_reload": "knobs",
    "lcv_knobs_list": "knobs",
    "lcv_attn_fwd_last_kernel": "introspection",
    "lcv_conv3d_last_kernel": "introspection",
    "lcv_attn_bwd_ws_floats": "size",
    "lcv_tn_skinny_ws_bytes": "size",
    "lcv_gemm_set_workspace": "registration",
}


def _declared():
    """The entry points of include/lcv_hip.h, parsed as tests/test_abi_and_host.py does."""
    txt = (ROOT / "include" / "lcv_hip.h").read_text()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return set(re.findall(r"\b(lcv_[a-z0-9_]+)\s*\(", txt))


def _functions(path: Path):
    return {n.name for n in ast.walk(ast.parse(path.read_text())) if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef))}


def test_every_declared_entry_point_has_a_kernel_level_test():
    declared = _declared()
    assert not set(KERNEL_TESTS) & set(EXEMPT)
    assert set(KERNEL_TESTS) | set(EXEMPT) == declared, {
        "declared but neither tested nor exempt": sorted(declared - set(KERNEL_TESTS) - set(EXEMPT)),
        "listed but not declared": sorted((set(KERNEL_TESTS) | set(EXEMPT)) - declared)}
    assert all(len(reason.split()) == 1 for reason in EXEMPT.values())
    cache = {}
    missing = []
    for name, tests in KERNEL_TESTS.items():
        assert tests, name
        for fname, fn in tests:
            if fname not in cache:
                cache[fname] = _functions(TESTS / fname)
            if fn not in cache[fname]:
                missing.append(f"{name}: {fname}::{fn}")
    assert not missing, missing

"""CPU: the per-element check of tests/kernel_ref.py is sensitive enough to be worth its GPU time (one element 2 bf16 ulps
off fails, one non-zero pad element fails, the exact rounding passes), and every compute entry point that include/lcv_hip.h
declares has a kernel-level test (the coverage guard: a new entry point without one fails here, without a GPU)."""
import ast
import re
from pathlib import Path

import pytest
import torch

import kernel_ref as K

ROOT = Path(__file__).resolve().parents[1]
TESTS = ROOT / "tests"
EDGES = "test_gpu_kernel_edges.py"


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
    "lcv_qknorm_rope_fwd": [("test_gpu_kernels.py", "test_qknorm_rope")],
    "lcv_qknorm_rope_bwd": [("test_gpu_backward.py", "test_qknorm_rope_backward"),
                            ("test_gpu_backward.py", "test_qk_norm_weight_gradients")],
    "lcv_timestep_embedding": [("test_gpu_kernels.py", "test_timestep_embedding_matches_oracle")],
    "lcv_attn_fwd": [("test_gpu_kernels.py", "test_attention_fuzz_against_the_restatement_of_the_kernels_arithmetic")],
    "lcv_attn_bwd": [("test_gpu_backward.py", "test_attention_backward_fuzz_against_the_kernels_rounding_points")],
    "lcv_gemm_nt": [("test_gpu_kernels.py", "test_gemm_dispatch_fuzz_bitwise_against_the_one_barrier_kernel"),
                    ("test_gpu_kernels.py", "test_gemm_nt_lora_and_epilogues")],
    "lcv_lora_down": [("test_gpu_kernels.py", "test_gemm_nt_lora_and_epilogues")],
    "lcv_tn_skinny": [("test_gpu_backward.py", "test_linear_f32_backward_and_tn_skinny_and_unpatchify")],
    "lcv_linear_f32_smallm": [("test_gpu_kernels.py", "test_linear_f32_smallm")],
    "lcv_linear_f32_smallm_bwd": [("test_gpu_backward.py", "test_linear_f32_backward_and_tn_skinny_and_unpatchify")],
    "lcv_swiglu_fwd": [(EDGES, "test_swiglu_fwd_on_views_into_one_buffer_past_the_block_cap")],
    "lcv_swiglu_bwd": [("test_gpu_backward.py", "test_norm_gate_swiglu_backward")],
    "lcv_swiglu_bwd_interleaved": [("test_gpu_backward.py", "test_fused_swiglu_training_path_matches_the_unfused_form")],
    "lcv_patchify": [(EDGES, "test_patchify_pad_and_unpatchify_past_the_block_cap")],
    "lcv_unpatchify": [(EDGES, "test_patchify_pad_and_unpatchify_past_the_block_cap")],
    "lcv_unpatchify_bwd": [(EDGES, "test_patchify_pad_and_unpatchify_past_the_block_cap")],
    "lcv_cfg_euler_step": [(EDGES, "test_cfg_euler_step_edges")],
    "lcv_euler_step": [(EDGES, "test_euler_step_edges")],
    "lcv_fm_noise": [(EDGES, "test_fm_noise_past_the_block_cap")],
    "lcv_fm_mse": [(EDGES, "test_fm_mse_past_the_block_cap_and_deterministic")],
    "lcv_fm_mse_samples": [("test_gpu_early_stopping.py", "test_fm_mse_samples_matches_torch_and_is_deterministic")],
    "lcv_grad_norm_clip": [("test_gpu_backward.py", "test_fused_adamw_clip_matches_reference_trace"),
                           ("test_gpu_backward.py", "test_joint_clip_over_bf16_and_fp32_parameters_matches_torch")],
    "lcv_adamw_step": [("test_gpu_backward.py", "test_fused_adamw_clip_matches_reference_trace")],
    "lcv_sgd_step": [("test_gpu_backward.py", "test_fused_sgd_clip_matches_torch")],
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
    "lcv_gather_rows": [("test_gpu_umt5.py", "test_gather_norm_geglu_kernels")],
    "lcv_t5_rmsnorm": [("test_gpu_umt5.py", "test_gather_norm_geglu_kernels")],
    "lcv_geglu_tanh_fwd": [("test_gpu_umt5.py", "test_gather_norm_geglu_kernels")],
    "lcv_t5_attention": [("test_gpu_umt5.py", "test_attention_kernel_matches_oracle")],
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

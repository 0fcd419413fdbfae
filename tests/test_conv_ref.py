"""CPU: the float64 restatement of the VAE convolutions (tests/conv_ref.py) against an independent gather loop and against
torch's own convolutions, the exactness claim its bitwise GPU comparisons rest on, and its layout helpers."""
import pytest
import torch
import torch.nn.functional as F

import conv_ref as R


def _gather_causal(x, w, up2x):
    """lcv_causal_conv3d's contract read literally, one tap at a time: index arithmetic only, no padded tensor."""
    B, C, T, Hin, Win = x.shape
    co, ci, kt, kh, kw = w.shape
    H, W = (2 * Hin, 2 * Win) if up2x else (Hin, Win)
    out = torch.zeros((B, co, T, H, W), dtype=torch.float64)
    for b in range(B):
        for t in range(T):
            for h in range(H):
                for ww in range(W):
                    for dt in range(kt):
                        for dh in range(kh):
                            for dw in range(kw):
                                ti, hi, wi = t + dt - (kt - 1), h + dh - kh // 2, ww + dw - kw // 2
                                if ti < 0 or hi < 0 or hi >= H or wi < 0 or wi >= W:
                                    continue
                                if up2x:
                                    hi, wi = hi // 2, wi // 2
                                out[b, :, t, h, ww] += w[:, :, dt, dh, dw] @ x[b, :, ti, hi, wi]
    return out


def _gather_strided(x, w, stride, out_thw):
    B, C, T, H, W = x.shape
    co, ci, kt, kh, kw = w.shape
    out = torch.zeros((B, co) + tuple(out_thw), dtype=torch.float64)
    for b in range(B):
        for t in range(out_thw[0]):
            for h in range(out_thw[1]):
                for ww in range(out_thw[2]):
                    for dt in range(kt):
                        for dh in range(kh):
                            for dw in range(kw):
                                ti, hi, wi = t * stride[0] + dt, h * stride[1] + dh, ww * stride[2] + dw
                                if ti < T and hi < H and wi < W:
                                    out[b, :, t, h, ww] += w[:, :, dt, dh, dw] @ x[b, :, ti, hi, wi]
    return out


@pytest.mark.parametrize("k,up2x,shape", [
    ((3, 3, 3), False, (2, 3, 4, 5)), ((3, 3, 3), False, (2, 1, 1, 1)), ((3, 3), True, (2, 2, 3, 2)), ((3, 3), False, (1, 2, 1, 4)),
    ((3, 1, 1), False, (2, 4, 2, 3)), ((1, 1, 1), False, (2, 2, 2, 3)), ((3, 3), True, (1, 1, 1, 1)),
])
def test_causal_form_equals_gather_loop_and_torch(k, up2x, shape):
    B, T, H, W = shape
    x, w = R.make_x(B, 5, T, H, W, seed=1), R.make_w(4, 5, k, seed=2)
    ref = R.causal_conv3d(x, w, up2x=up2x)
    assert torch.equal(ref, _gather_causal(x, w, up2x))
    kt, kh, kw = w.shape[2:]
    y = F.interpolate(x.view(B, 5 * T, H, W), scale_factor=(2.0, 2.0), mode="nearest-exact").view(B, 5, T, 2 * H, 2 * W) if up2x else x
    assert torch.equal(ref, F.conv3d(F.pad(y, (kw // 2, kw // 2, kh // 2, kh // 2, kt - 1, 0)), w))
    if kt == 1:                                                  # a 2-D kernel is a per-frame conv2d
        Ho, Wo = y.shape[3:]
        per_frame = F.conv2d(y.permute(0, 2, 1, 3, 4).reshape(B * T, 5, Ho, Wo), w[:, :, 0], padding=(kh // 2, kw // 2))
        assert torch.equal(ref, per_frame.view(B, T, 4, Ho, Wo).permute(0, 2, 1, 3, 4))


@pytest.mark.parametrize("k,stride,shape,out_thw", [
    ((3, 3), (1, 2, 2), (2, 2, 6, 10), (2, 3, 5)), ((3, 3), (1, 2, 2), (2, 2, 7, 9), (2, 3, 4)), ((3, 3), (1, 2, 2), (2, 1, 1, 1), (1, 1, 1)),
    ((3, 3), (1, 2, 2), (1, 2, 7, 9), (2, 2, 3)), ((3, 1, 1), (2, 1, 1), (2, 5, 2, 3), (2, 2, 3)), ((3, 1, 1), (2, 1, 1), (2, 9, 1, 2), (3, 1, 2)),
    ((3, 3, 3), (2, 2, 2), (1, 4, 5, 4), (2, 3, 2)),
])
def test_strided_form_equals_gather_loop_and_torch(k, stride, shape, out_thw):
    B, T, H, W = shape
    x, w = R.make_x(B, 5, T, H, W, seed=3), R.make_w(4, 5, k, seed=4)
    ref = R.strided_conv3d(x, w, stride, out_thw)
    assert ref.shape == (B, 4) + tuple(out_thw)
    assert torch.equal(ref, _gather_strided(x, w, stride, out_thw))
    # torch on an input zero-padded at the END of every axis (generously), cropped to the caller's extent
    full = F.conv3d(F.pad(x, (0, 3, 0, 3, 0, 3)), w, stride=stride)
    assert torch.equal(ref, full[:, :, :out_thw[0], :out_thw[1], :out_thw[2]])


def test_encoder_downsample_is_the_strided_form():
    """ZeroPad2d((0,1,0,1)) + 3x3 stride-2 conv per frame, the stage lcv_conv3d_strided was written for."""
    x, w = R.make_x(2, 5, 3, 6, 10, seed=5), R.make_w(4, 5, (3, 3), seed=6)
    ref = R.strided_conv3d(x, w, (1, 2, 2), (3, 3, 5))
    y = F.conv2d(F.pad(x.permute(0, 2, 1, 3, 4).reshape(6, 5, 6, 10), (0, 1, 0, 1)), w[:, :, 0], stride=2)
    assert torch.equal(ref, y.view(2, 3, 4, 3, 5).permute(0, 2, 1, 3, 4))


def test_fp32_evaluation_is_exact_at_the_largest_k():
    """27 taps x 384 channels: the fp32 and the float64 evaluation of the reference agree in every element (all partial sums are
    integers below 2^24), also with the terms added in another order, and the sums are large enough for bf16 to round."""
    x, w = R.make_x(2, 384, 2, 3, 4, seed=7), R.make_w(8, 384, (3, 3, 3), seed=8)
    R.check_data_rules(x, w)
    assert w.shape[1] * 27 == R.K_MAX
    r64 = R.causal_conv3d(x, w)
    r32 = R.causal_conv3d(x, w, dtype=torch.float32)
    assert r32.dtype == torch.float32 and torch.equal(r32.to(torch.float64), r64)
    perm = torch.randperm(384, generator=torch.Generator().manual_seed(9))
    assert torch.equal(R.causal_conv3d(x[:, perm].flip(1), w[:, perm].flip(1), dtype=torch.float32).to(torch.float64), r64)
    assert float(r64.abs().max()) < 2 ** 17
    # worst case by construction: every term +6
    xs, ws = torch.full((1, 384, 3, 3, 3), 3.0, dtype=torch.float64), torch.full((1, 384, 3, 3, 3), 2.0, dtype=torch.float64)
    assert R.causal_conv3d(xs, ws, dtype=torch.float32)[0, 0, 2, 1, 1].item() == 6 * R.K_MAX
    # the store rounding is exercised: every odd sum above 256 rounds (most pixels of this shape lie on a border and see
    # fewer taps; a full-K sum has a standard deviation of sqrt(8 K) = 288)
    odd_above = (r64.abs() > 256) & (r64 % 2 != 0)
    assert odd_above.sum() >= 20 and bool((r64.to(R.BF16).to(torch.float64) != r64)[odd_above].all())


def test_generated_tensors_survive_bf16_and_obey_the_rules():
    x, w = R.make_x(2, 32, 2, 3, 4, seed=10), R.make_w(6, 32, (3, 3), seed=11)
    b, r = R.make_bias(256, seed=12), R.make_resid(2, 6, 2, 3, 4, seed=13)
    R.check_data_rules(x, w, b[:6], r)
    for t, bound in ((x, 3), (w, 2), (b, 8), (r, 8)):
        assert torch.equal(t.to(R.BF16).to(torch.float64), t)
        assert t.min() == -bound and t.max() == bound
    assert w.shape == (6, 32, 1, 3, 3)
    with pytest.raises(AssertionError):
        R.check_data_rules(x * 2, w)
    with pytest.raises(AssertionError):
        R.check_data_rules(x + 0.5, w)


def test_finish_rounds_where_the_epilogue_does():
    acc = torch.tensor([257.0, 259.0, 300.0]).view(1, 3, 1, 1, 1).to(torch.float64)     # bf16 spacing 2 above 256
    bias = torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64)
    assert R.finish(acc, bias).flatten().tolist() == [256.0, 260.0, 300.0]              # ties to even; 301 is a tie -> 300
    resid = torch.tensor([1.0, 1.0, 1.0], dtype=torch.float64).view(1, 3, 1, 1, 1)
    # two roundings, not one: 257 -> 256, + 1 = 257 -> 256 (a single rounding of 258 would give 258)
    assert R.finish(acc, bias, resid).flatten().tolist() == [256.0, 260.0, 300.0]


def test_layout_helpers_round_trip_and_match_the_module():
    x = R.make_x(2, 32, 2, 3, 4, seed=14)
    cl = R.to_kernel_layout(x)
    assert cl.shape == (2, 2, 3, 4, 64) and cl.dtype == R.BF16 and float(cl[..., 32:].abs().max()) == 0
    assert cl[1, 0, 2, 3, 5].item() == x[1, 5, 0, 2, 3].item()
    assert torch.equal(R.from_kernel_layout(cl, 32), x)
    assert R.to_kernel_layout(x[:, :3], pad=False).shape == (2, 2, 3, 4, 3)
    from longcat_video.modules.vae_wan import _Conv
    for k in ((3, 3, 3), (3, 3), (1, 1, 1)):
        w = R.make_w(6, 32, k, seed=15)
        conv = _Conv(32, 6, k, device="cpu")
        with torch.no_grad():
            conv.weight.copy_(w.view(conv.weight.shape))
        packed = R.pack_weight(w)
        assert packed.shape == (6, w.shape[2] * w.shape[3] * w.shape[4] * 64) and torch.equal(packed, conv.packed())
        # K order (dt, dh, dw, cin): the last tap's channel 7 sits at (taps - 1) * 64 + 7
        assert packed[4, packed.shape[1] - 64 + 7].item() == w[4, 7, -1, -1, -1].item()

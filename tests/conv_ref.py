"""Float64 restatement of the two VAE convolution entry points (`lcv_causal_conv3d`, `lcv_conv3d_strided`) on small-integer
data - what tests/test_gpu_conv_exact.py compares every convolution kernel against, bit for bit.  It follows the contracts
in include/lcv_hip.h and shares no code with the kernels: zero-padded tensors, shifted slices and one matrix product per tap.

Why integers.  The kernels multiply bf16 x bf16 on the MFMA and add in fp32.  With x in [-3, 3] and w in [-2, 2] every product
and every partial sum is an integer of magnitude <= 6 * K + 8 (K = taps * channels <= 10 368 here), far below 2^24: exact in
fp32 in ANY summation order.  The one rounding left is the RNE store to bf16, so the output must equal bf16(float64 sum) in
every element, whatever tile shape, K permutation or split a kernel uses.

Layouts.  The reference works in torch's: x [B, C, T, H, W], w [Cout, Cin, kt, kh, kw] (a 2-D kernel is kt = 1), result
[B, Cout, T', H', W'].  `to_kernel_layout` / `from_kernel_layout` go to and from the kernels' channels-last
[B, T, H, W, pad64(C)] bf16 with zero padding channels; `pack_weight` is the kernels' [Cout, taps * pad64(Cin)] weight with K
ordered (dt, dh, dw, cin).
"""
import torch

BF16 = torch.bfloat16
X_MAX, W_MAX, B_MAX = 3, 2, 8          # |x| <= 3, |w| <= 2, |bias|, |resid| <= 8
K_MAX = 27 * 384                       # the largest reduction of the test matrix: 27 taps x 384 channels


def pad64(c: int) -> int:
    return (c + 63) // 64 * 64


def _ints(shape, bound, seed):
    g = torch.Generator().manual_seed(int(seed))
    return torch.randint(-bound, bound + 1, tuple(shape), generator=g).to(torch.float64)


def make_x(B, C, T, H, W, seed):
    return _ints((B, C, T, H, W), X_MAX, seed)


def make_w(cout, cin, k, seed):
    k = tuple(k) if len(k) == 3 else (1,) + tuple(k)
    return _ints((cout, cin) + k, W_MAX, seed)


def make_bias(cout, seed):
    return _ints((cout,), B_MAX, seed)


def make_resid(B, cout, T, H, W, seed):
    return _ints((B, cout, T, H, W), B_MAX, seed)


def check_data_rules(x, w, bias=None, resid=None):
    """The premises of the exactness argument: integer values inside the stated ranges, a reduction no longer than K_MAX."""
    for t, bound in ((x, X_MAX), (w, W_MAX), (bias, B_MAX), (resid, B_MAX)):
        if t is None:
            continue
        assert t.dtype == torch.float64 and torch.equal(t, t.round()) and float(t.abs().max()) <= bound, "data rule broken"
        assert torch.equal(t.to(BF16).to(torch.float64), t)
    assert x.shape[1] == w.shape[1] and w.shape[1] * w.shape[2] * w.shape[3] * w.shape[4] <= K_MAX
    assert X_MAX * W_MAX * K_MAX + B_MAX < 2 ** 17


def _taps(xp, w, stride, out_thw, dtype):
    """sum over taps of w[:, :, dt, dh, dw] applied to xp[t*st+dt, h*sh+dh, w*sw+dw]; xp [B, C, T, H, W] already padded."""
    B = xp.shape[0]
    co, ci, kt, kh, kw = w.shape
    st, sh, sw = stride
    To, Ho, Wo = out_thw
    xp, w = xp.to(dtype), w.to(dtype)
    out = torch.zeros((B, To, Ho, Wo, co), dtype=dtype)
    for dt in range(kt):
        for dh in range(kh):
            for dw in range(kw):
                sl = xp[:, :, dt: dt + (To - 1) * st + 1: st, dh: dh + (Ho - 1) * sh + 1: sh, dw: dw + (Wo - 1) * sw + 1: sw]
                out += sl.permute(0, 2, 3, 4, 1).reshape(-1, ci).matmul(w[:, :, dt, dh, dw].t()).view(B, To, Ho, Wo, co)
    return out.permute(0, 4, 1, 2, 3).contiguous()


def upsample2x(x):
    """Nearest 2x in h and w: output (h, w) reads input (h // 2, w // 2)."""
    return x.repeat_interleave(2, dim=3).repeat_interleave(2, dim=4)


def causal_conv3d(x, w, up2x=False, dtype=torch.float64):
    """The sum of lcv_causal_conv3d (no bias): kt - 1 zero frames in front, kh // 2 and kw // 2 zeros on every spatial side,
    stride 1; with `up2x` the taps read the nearest-2x upsampled input.  Output [B, Cout, T, H', W']."""
    co, ci, kt, kh, kw = w.shape
    assert kh % 2 == 1 and kw % 2 == 1
    if up2x:
        x = upsample2x(x)
    B, C, T, H, W = x.shape
    xp = torch.zeros((B, C, T + kt - 1, H + kh - 1, W + kw - 1), dtype=x.dtype)
    xp[:, :, kt - 1:, kh // 2: kh // 2 + H, kw // 2: kw // 2 + W] = x
    return _taps(xp, w, (1, 1, 1), (T, H, W), dtype)


def strided_conv3d(x, w, stride, out_thw, dtype=torch.float64):
    """The sum of lcv_conv3d_strided: output (t, h, w) reads input (t*st + dt, h*sh + dh, w*sw + dw), no front padding, taps
    past the input extent read zero, the caller gives the output extent (which must start inside the input)."""
    co, ci, kt, kh, kw = w.shape
    B, C, T, H, W = x.shape
    st, sh, sw = stride
    To, Ho, Wo = out_thw
    assert (To - 1) * st < T and (Ho - 1) * sh < H and (Wo - 1) * sw < W
    need = ((To - 1) * st + kt, (Ho - 1) * sh + kh, (Wo - 1) * sw + kw)
    xp = torch.zeros((B, C, max(T, need[0]), max(H, need[1]), max(W, need[2])), dtype=x.dtype)
    xp[:, :, :T, :H, :W] = x
    return _taps(xp, w, stride, out_thw, dtype)


def finish(acc, bias=None, resid=None):
    """The epilogue's rounding points: bf16(sum + bias), and with a residual bf16(resid + bf16(sum + bias))."""
    y = acc.to(torch.float64)
    if bias is not None:
        y = y + bias.to(torch.float64).view(1, -1, 1, 1, 1)
    y = y.to(BF16)
    if resid is not None:
        y = (resid.to(torch.float64) + y.to(torch.float64)).to(BF16)
    return y


def to_kernel_layout(x, pad=True):
    """[B, C, T, H, W] -> channels-last bf16 [B, T, H, W, pad64(C)] (or C when not `pad`), padding channels zero."""
    B, C, T, H, W = x.shape
    out = torch.zeros((B, T, H, W, pad64(C) if pad else C), dtype=BF16)
    out[..., :C] = x.permute(0, 2, 3, 4, 1).to(BF16)
    return out


def from_kernel_layout(y, C):
    """Channels-last [B, T, H, W, >= C] -> float64 [B, C, T, H, W]."""
    return y[..., :C].permute(0, 4, 1, 2, 3).to(torch.float64).contiguous()


def pack_weight(w):
    """[Cout, Cin, kt, kh, kw] -> bf16 [Cout, kt * kh * kw * pad64(Cin)], K ordered (dt, dh, dw, cin), padding channels zero."""
    co, ci, kt, kh, kw = w.shape
    wp = torch.zeros((co, kt, kh, kw, pad64(ci)), dtype=BF16)
    wp[..., :ci] = w.permute(0, 2, 3, 4, 1).to(BF16)
    return wp.reshape(co, -1).contiguous()

"""Restatement of LPIPS v0.1 (AlexNet backbone) in plain torch on the CPU, float64 or fp32 — what the GPU tests of the
LPIPS kernels compare against (the precedent is tests/kernel_ref.py).  It follows spec/lpips.md item by item and shares
no code with the product: `F.conv2d`, `F.max_pool2d`, NCHW.

State dicts use the `lpips.LPIPS(net="alex").state_dict()` key names (spec/lpips.md L6).
"""
import torch
import torch.nn.functional as F

SHIFT = (-0.030, -0.088, -0.188)
SCALE = (0.458, 0.448, 0.450)
# (state-dict prefix, Cin, Cout, kernel, stride, pad, max-pool 3/2 in front of the convolution)
LAYERS = (("net.slice1.0", 3, 64, 11, 4, 2, False), ("net.slice2.3", 64, 192, 5, 1, 2, True),
          ("net.slice3.6", 192, 384, 3, 1, 1, True), ("net.slice4.8", 384, 256, 3, 1, 1, False),
          ("net.slice5.10", 256, 256, 3, 1, 1, False))
MIN_SIDE = 31


def synthetic_state_dict(seed: int):
    """The draw `LpipsAlex.synthetic_state_dict` documents, restated: per layer He-normal weights, N(0, 0.05²) biases,
    U[0,1) * 2 / C lin weights, one CPU generator, in layer order."""
    g = torch.Generator().manual_seed(int(seed))
    sd = {}
    for i, (key, cin, cout, k, _, _, _) in enumerate(LAYERS):
        sd[key + ".weight"] = torch.randn((cout, cin, k, k), generator=g) * (2.0 / (cin * k * k)) ** 0.5
        sd[key + ".bias"] = torch.randn((cout,), generator=g) * 0.05
        sd[f"lin{i}.model.1.weight"] = torch.rand((1, cout, 1, 1), generator=g) * (2.0 / cout)
    return sd


def to_unit(frames: torch.Tensor, dtype) -> torch.Tensor:
    """[N,H,W,3] fp32 in [0,1] or uint8 -> the same values in `dtype` (uint8 / 255 is taken in fp32 first, as
    `frame_metrics` and numpy's `/ 255.0 -> float32` do)."""
    if frames.dtype == torch.uint8:
        frames = frames.float() / 255.0
    return frames.to(dtype)


def scale_input(frames: torch.Tensor, dtype, sd=None) -> torch.Tensor:
    """NHWC frames in [0,1] -> NCHW network input: 2x - 1, then (x - shift) / scale."""
    shift = torch.tensor(SHIFT, dtype=torch.float32) if sd is None or "scaling_layer.shift" not in sd else sd["scaling_layer.shift"].reshape(-1)
    scale = torch.tensor(SCALE, dtype=torch.float32) if sd is None or "scaling_layer.scale" not in sd else sd["scaling_layer.scale"].reshape(-1)
    x = 2.0 * to_unit(frames, dtype).permute(0, 3, 1, 2) - 1.0
    return (x - shift.to(dtype).view(1, 3, 1, 1)) / scale.to(dtype).view(1, 3, 1, 1)


def taps(frames: torch.Tensor, sd, dtype=torch.float64):
    """The five post-ReLU feature maps [N,C,h,w] of NHWC frames."""
    if frames.shape[1] < MIN_SIDE or frames.shape[2] < MIN_SIDE:
        raise ValueError(f"a {frames.shape[1]}x{frames.shape[2]} frame is smaller than {MIN_SIDE}x{MIN_SIDE}: the second pool has no window")
    x = scale_input(frames, dtype, sd)
    out = []
    for key, _, _, _, stride, pad, pool in LAYERS:
        if pool:
            x = F.max_pool2d(x, kernel_size=3, stride=2)
        x = F.relu(F.conv2d(x, sd[key + ".weight"].to(dtype), sd[key + ".bias"].to(dtype), stride=stride, padding=pad))
        out.append(x)
    return out


def tap_distance(fg: torch.Tensor, ft: torch.Tensor, lin: torch.Tensor) -> torch.Tensor:
    """NCHW features of the two halves, lin [1,C,1,1] or [C] -> [N]: unit-normalise over channels with the epsilon
    OUTSIDE the square root, squared difference, 1x1 lin weights, spatial mean."""
    ng = fg / (fg.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    nt = ft / (ft.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    d = ((ng - nt) ** 2 * lin.to(fg.dtype).reshape(1, -1, 1, 1)).sum(1)
    return d.mean(dim=(1, 2))


def lpips(gen: torch.Tensor, gt: torch.Tensor, sd, dtype=torch.float64) -> torch.Tensor:
    """Per-frame LPIPS [N] of NHWC frame stacks (fp32 in [0,1] or uint8)."""
    if gen.shape != gt.shape:
        raise ValueError(f"frame stacks differ: {tuple(gen.shape)} / {tuple(gt.shape)}")
    tg, tt = taps(gen, sd, dtype), taps(gt, sd, dtype)
    total = torch.zeros(gen.shape[0], dtype=dtype)
    for i, (a, b) in enumerate(zip(tg, tt)):
        total = total + tap_distance(a, b, sd[f"lin{i}.model.1.weight"])
    return total


def frames(N, H, W, C=3, seed=0, noise=0.08):
    """Structured ground truth + noise: the generator of tests/test_gpu_eval.py::_frames, restated (existing test files
    are not imported from: test_gpu_eval.py loads a fixture at import time)."""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    base = 0.5 + 0.35 * torch.sin(xx / 17.0 + torch.arange(N).view(N, 1, 1, 1) * 0.3) * torch.cos(yy / 11.0)
    gt = (base.view(N, H, W, 1).expand(N, H, W, C) + 0.1 * torch.rand((N, H, W, C), generator=g)).clamp(0, 1)
    gt_u8 = (gt * 255).round().to(torch.uint8)
    gen = (gt_u8.float() / 255.0 + noise * torch.randn((N, H, W, C), generator=g)).clamp(0, 1)
    return gen.contiguous(), gt_u8.contiguous()

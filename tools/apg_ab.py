#!/usr/bin/env python
"""The figures of profiles/apg.md: lcv_cfg_apg alone over the flagship latent ([1, 16, 13, 90, 160] fp32 per operand, 49 x 720p),
next to lcv_cfg_euler_step (the fused guidance + update it takes the place of) and lcv_euler_step (the unguided update that follows
it), in one process on one GPU.  Device events around each call, `--iters` calls of each form after one warm-up call; prints the
markdown table.  The bytes per element are those of include/lcv_hip_apg.h, counted from the shapes."""
import argparse
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "longcat-video-tta_amd")]

SHAPE = (1, 16, 13, 90, 160)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args(argv)
    import torch
    from lcv_hip import ops
    if not torch.cuda.is_available():
        raise SystemExit("apg_ab: no GPU (a time measured anywhere else says nothing)")
    g = torch.Generator(device="cuda").manual_seed(1)
    c = torch.randn(SHAPE, device="cuda", generator=g)
    u = 0.5 * c + 0.5 * torch.randn(SHAPE, device="cuda", generator=g)
    x = torch.randn(SHAPE, device="cuda", generator=g)
    diff, v = torch.zeros_like(c), torch.empty_like(c)
    out = torch.zeros((1, 4), device="cuda")
    n = c.numel()
    radius = 0.25 * n ** 0.5
    forms = [
        ("apg, zero-star, momentum, threshold (3 launches)", 36,
         lambda: ops.cfg_apg(c, u, diff, 4.0, 0.5, radius, -0.5, True, True, out=out, v=v)),
        ("apg, zero-star, no momentum (3 launches)", 32, lambda: ops.cfg_apg(c, u, diff, 4.0, 0.0, None, 0.0, True, False, out=out, v=v)),
        ("apg, no zero-star, momentum (2 launches)", 28, lambda: ops.cfg_apg(c, u, diff, 4.0, 0.0, None, -0.5, False, True, out=out, v=v)),
        ("apg, no zero-star, no momentum (2 launches)", 24, lambda: ops.cfg_apg(c, u, diff, 4.0, 0.0, None, 0.0, False, False, v=v)),
        ("lcv_cfg_euler_step, zero-star (2 launches)", 28, lambda: ops.cfg_euler_step(c, u, x, 4.0, 1e-3, zero_star=True)),
        ("lcv_cfg_euler_step, no zero-star", 16, lambda: ops.cfg_euler_step(c, u, x, 4.0, 1e-3, zero_star=False)),
        ("lcv_euler_step (the update after apg)", 12, lambda: ops.euler_step(c, x, 1e-3)),
    ]
    lines = [f"{n / 1e6:.2f} M fp32 elements per operand, {args.iters} calls of each form after one warm-up call, device events around "
             "each call", "", "| form | B / element | median (ms) | min | max | TB/s at the median |", "|---|---|---|---|---|---|"]
    for name, nbytes, fn in forms:
        fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(args.iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        med = statistics.median(ms)
        lines.append(f"| {name} | {nbytes} | {med:.4f} | {min(ms):.4f} | {max(ms):.4f} | {nbytes * n / (med * 1e-3) / 1e12:.2f} |")
    text = "\n".join(lines)
    print(text)
    if args.out is not None:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text(text + "\n")


if __name__ == "__main__":
    main()

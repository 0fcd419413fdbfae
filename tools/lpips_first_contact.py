#!/usr/bin/env python3
"""First contact of the on-device LPIPS with the real package (spec/lpips.md, items L1-L6).

On a machine where `lpips` imports (with its AlexNet weights available) and an MI355X is present, this compares ONE
value: `lpips.LPIPS(net="alex")(gen, gt, normalize=True)` on a seeded pair of 64x96 frames against
`tta.lpips.LpipsAlex` built from that very module's state dict.  Agreement to 1e-5 relative confirms the layer list, the
tap points, the epsilon placement, the scaling constants and the key names at once; a mismatch says which assumption
list to re-read, not which item.

Where the package is missing (the machines this project is built and tested on) it says so and exits 0: it cannot run
there, and that is not a failure.
"""
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "longcat-video-tta_amd"))


def main() -> int:
    try:
        import lpips  # noqa: F401
    except ImportError as e:
        print(f"lpips_first_contact: the `lpips` package does not import here ({e}); nothing compared. "
              "Run this where the reference's environment is installed.")
        return 0
    import torch
    if not torch.cuda.is_available():
        print("lpips_first_contact: no GPU here; the product has no CPU path, nothing compared.")
        return 0
    from tta.lpips import LpipsAlex
    net = lpips.LPIPS(net="alex").eval()
    g = torch.Generator().manual_seed(0)
    gt = torch.rand((2, 64, 96, 3), generator=g)
    gen = (gt + 0.1 * torch.randn((2, 64, 96, 3), generator=g)).clamp(0, 1)
    with torch.no_grad():
        want = net(gen.permute(0, 3, 1, 2), gt.permute(0, 3, 1, 2), normalize=True).reshape(-1).double()
    got = LpipsAlex(net.state_dict())(gen.cuda(), gt.cuda()).cpu().double()
    rel = ((got - want).abs() / want.abs().clamp_min(1e-12)).max().item()
    print(f"package {want.tolist()}  product {got.tolist()}  max relative difference {rel:.3g}")
    if rel > 1e-5:
        print("MISMATCH: re-read spec/lpips.md L1-L6 against the installed package")
        return 1
    print("spec/lpips.md L1-L6 confirmed on this pair")
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""What 8-bit block-scaled AdamW moments (include/lcv_hip_moments8.h) do to a trajectory, on the CPU, in the numpy restatement
the GPU tests hold the kernels to (tests/moments8_ref.py): `python tools/adam8_quality.py [--out profiles/adam_8bit.md]`.

The toy run: 64 blocks of 512 masters, bf16 gradients g = s_i * z with a fixed per-element scale s_i = exp(sigma * N(0, 1)) and
fresh z ~ N(0, 1) every step, AdamW (0.9, 0.999, eps 1e-8, wd 0.01) at lr 2e-4.  The same gradients drive the fp32-moment step
(master_weights_ref.adamw_step) and the 8-bit step (moments8_ref.adamw8_step).  Reported: the relative L2 distance of the two
displacements from the start, the largest distance of one element from its fp32-moment counterpart in units of lr, the share of
first moments that flushed and of roots held at the floor, and whether step 1 is bit-identical.  No GPU is needed or used."""
import argparse
import re
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(HERE / "tests"))
QUALITY_HEAD = "## Trajectory quality (CPU restatement)"
TIME_HEAD = "## Step time (GPU)"


def replace_section(path: Path, head: str, body: str, title: str) -> None:
    """Put `body` under the `## ` heading `head` of the markdown file, replacing what that section held; other sections stay."""
    text = path.read_text() if path.exists() else f"# {title}\n"
    pat = re.compile(r"^" + re.escape(head) + r"\n.*?(?=^## |\Z)", flags=re.S | re.M)
    section = head + "\n\n" + body.rstrip("\n") + "\n\n"
    text = pat.sub(lambda _m: section, text) if pat.search(text) else text.rstrip("\n") + "\n\n" + section
    path.parent.mkdir(parents=True, exist_ok=True)
    path.write_text(text.rstrip("\n") + "\n")


def run(sigma: float, steps: int, blocks: int = 64, lr: float = 2e-4, seed: int = 0):
    import master_weights_ref as W
    import moments8_ref as R
    rng = np.random.default_rng(seed)
    n = blocks * R.BLOCK
    h0, l0 = W.weights(rng, n)
    scale = np.exp(sigma * rng.standard_normal(n))
    a = dict(h=h0, l=l0, m=np.zeros(n, W.F), v=np.zeros(n, W.F))
    b = dict(h=h0, l=l0, st=R.zero_state(n))
    start = W.master(h0, l0).astype(np.float64)
    first_same = None
    flushed = floored = 0.0
    for k in range(steps):
        g = W.to_bf16_bits((scale * rng.standard_normal(n)).astype(W.F))
        a["h"], a["l"], a["m"], a["v"] = W.adamw_step(a["h"], a["l"], a["m"], a["v"], g, 1.0, lr, 0.9, 0.999, 1e-8, 0.01, k + 1)
        b["h"], b["l"], *st = R.adamw8_step(b["h"], b["l"], *b["st"], g, 1.0, lr, 0.9, 0.999, 1e-8, 0.01, k + 1)
        b["st"] = tuple(st)
        if k == 0:
            first_same = bool(np.array_equal(a["h"], b["h"]) and np.array_equal(a["l"], b["l"]))
        flushed += float(((st[0] & 127) == 0).mean()) / steps
        floored += float((st[1] <= 1).mean()) / steps
    pa = W.master(a["h"], a["l"]).astype(np.float64)
    pb = W.master(b["h"], b["l"]).astype(np.float64)
    assert np.isfinite(pb).all()
    return dict(sigma=sigma, steps=steps, decades=float(np.log10(scale.max() / scale.min())),
                rel_l2=float(np.linalg.norm(pb - pa) / np.linalg.norm(pa - start)), max_lr=float(np.abs(pb - pa).max() / lr),
                first_same=first_same, flushed=flushed, floored=floored)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", type=Path, default=None)
    args = ap.parse_args(argv)
    rows = [run(1.0, 20), run(1.0, 200), run(3.0, 20)]
    lines = ["`tools/adam8_quality.py`: 64 blocks of 512, g = s_i * z (s_i = exp(sigma * N(0, 1)) fixed, z ~ N(0, 1) per step, bf16), AdamW",
             "(0.9, 0.999, eps 1e-8, wd 0.01, lr 2e-4), numpy restatement; 8-bit moments against fp32 moments on the same gradients.",
             "Indicative figures of one seed, not thresholds.", "",
             "| sigma | decades of s_i, end to end | steps | relative L2 of the displacement | largest element distance (lr) | "
             "first moments flushed | roots at the floor | step 1 bit-identical |", "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['sigma']:g} | {r['decades']:.1f} | {r['steps']} | {r['rel_l2']:.1%} | {r['max_lr']:.1f} | {r['flushed']:.1%} | "
                     f"{r['floored']:.2%} | {'yes' if r['first_same'] else 'NO'} |")
    text = "\n".join(lines)
    print(text)
    if args.out is not None:
        replace_section(args.out, QUALITY_HEAD, text, "8-bit block-scaled AdamW moments (`--adam-8bit`)")


if __name__ == "__main__":
    main()

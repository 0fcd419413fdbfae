#!/usr/bin/env python3
"""Cost of LoRA dropout on the LoRA inner step at the reference's operating point (480p: Tc=3 + Tt=1 latent frames, 6 240
tokens, qkv + proj adapters, r = 8): `python tools/lora_dropout_ab.py [depth=48] [rounds=3] [steps=3] [out.md] [parent_lora.py]`.

One process, one model.  Three forms of the step alternate `rounds` times after one warm-up run each, `steps` optimizer steps
per run, so that clock and allocator drift hit all alike:
  parent p=0   the adapters of `parent_lora.py`, a copy of the parent commit's tta/lora.py (`git show HEAD~1:.../tta/lora.py`),
               on this library; left out when no such file is given
  p=0          this tree's adapters without dropout: the same kernels as the parent's, so the two agree within the spread
  p=0.1        the mask live in every step: lcv_lora_down_dropout, lcv_lora_dx_dropout_add, lcv_tn_skinny_dropout
Step time is the loop's own `train_time`.  Medians, spreads and the ratio to p=0 go to stdout and, as markdown, to `out.md`."""
import importlib.util
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "longcat-video-tta_amd")); sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

from lcv_hip import lib  # noqa: E402
from longcat_video.modules.longcat_video_dit import LongCatVideoTransformer3DModel  # noqa: E402
from tta import lora as this_lora  # noqa: E402
from tta.inner_loop import choose_gradient_checkpointing, finetune_lora_on_conditioning  # noqa: E402


def main():
    dev, bf = "cuda", torch.bfloat16
    depth = int(sys.argv[1]) if len(sys.argv) > 1 else 48
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    out = Path(sys.argv[4]) if len(sys.argv) > 4 else None
    forms = [("p=0", this_lora, 0.0), ("p=0.1", this_lora, 0.1)]
    if len(sys.argv) > 5:
        spec = importlib.util.spec_from_file_location("parent_tta_lora", sys.argv[5])
        parent = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(parent)
        forms.insert(0, ("parent p=0", parent, 0.0))
    (h, w), (tc, tt) = (60, 104), (3, 1)
    dit = LongCatVideoTransformer3DModel(device=dev, dtype=bf, depth=depth).eval().init_synthetic_()
    for p in dit.parameters():
        p.requires_grad = False
    tokens = (tc + tt) * (h // 2) * (w // 2)
    ckpt = choose_gradient_checkpointing(dit, tokens)
    g = torch.Generator(device=dev).manual_seed(1)
    cond = torch.randn(1, 16, tc, h, w, device=dev, generator=g).to(bf)
    train = torch.randn(1, 16, tt, h, w, device=dev, generator=g).to(bf)
    pe = torch.randn(1, 1, 512, 4096, device=dev, generator=g).to(bf)
    pm = torch.zeros(1, 512, dtype=torch.int64, device=dev); pm[:, :77] = 1

    count = []

    def run(mod, p, n):
        torch.manual_seed(1234)
        mods = mod.inject_lora_into_dit(dit, rank=8, alpha=16.0, dropout=p, target_modules=["qkv", "proj"], target_ffn=False,
                                        target_blocks="all")
        count[:] = [len(mods)]
        try:
            r = finetune_lora_on_conditioning(dit, mods, cond, train, pe, pm, num_steps=n, lr=2e-4, warmup_steps=0, device=dev,
                                              dtype=bf)
            torch.cuda.synchronize()
        finally:
            mod.remove_lora_from_dit(dit)
        return r["train_time"] / n

    for _, mod, p in forms:                             # warm-up: allocator, workspaces, kernel load
        run(mod, p, 1)
    times = {name: [] for name, _, _ in forms}
    for _ in range(rounds):
        for name, mod, p in forms:
            times[name].append(run(mod, p, steps) * 1e3)

    med = statistics.median
    base = med(times["p=0"])
    lines = [f"LoRA inner step, depth {depth}, 480p ({tokens} tokens), qkv + proj adapters ({count[0]} modules), r = 8, block "
             f"checkpointing {'on' if ckpt else 'off'}; {rounds} interleaved rounds x {steps} steps, library version "
             f"{lib.load().lcv_version()}", "", "| form | step time (ms), median | min | max | spread | ratio to p=0 |",
             "|---|---|---|---|---|---|"]
    for name, _, _ in forms:
        v = times[name]
        lines.append(f"| {name} | {med(v):.1f} | {min(v):.1f} | {max(v):.1f} | {(max(v) - min(v)) / med(v):.1%} | {med(v) / base:.4f} |")
    text = "\n".join(lines)
    print(text, flush=True)
    if out is not None:
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text(text + "\n")


if __name__ == "__main__":
    main()

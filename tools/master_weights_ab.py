#!/usr/bin/env python3
"""Cost and effect of fp32 master weights (`master_weights=True`, include/lcv_hip_master.h) at the reference's operating point
(480p: Tc=3 + Tt=1 latent frames, 6 240 tokens): `python tools/master_weights_ab.py [--depth 48] [--rounds 3] [--steps 3]
[--out profiles/master_weights.md] [--only full,opt,lora,drift] [--root TREE]`.

One process, one model; forms alternate `rounds` times after one warm-up run each, so that clock and allocator drift hit all
alike.  Four sections:
  full    the full-model step (every DiT parameter trainable, block checkpointing on, clip + SGD) with the flag off and on;
          step time is the loop's own `train_time`
  opt     the optimizer's two launches alone (gradient-norm clip, update) over the full parameter table, device events around
          `iters` back-to-back calls: SGD and AdamW, rounding form and master form, with the achieved bytes / s
  lora    the 20-step LoRA loop (qkv + proj adapters, r = 8) with the flag off and on
  drift   a 20-step full-model run at lr = 1e-5 (the reference's "inert" configuration) with the flag off and on: the share of
          parameter elements whose bf16 word changed, and the norm of master - base
`--root TREE` imports the packages from another checkout (the parent commit's, with its own built library): a tree whose loops
do not know the flag gets the off forms only, which is how the parent's own step time and run-to-run spread are measured."""
import argparse
import inspect
import statistics
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parents[1]


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--depth", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", type=Path, default=None)
    ap.add_argument("--only", type=str, default="full,opt,lora,drift")
    ap.add_argument("--root", type=Path, default=HERE)
    return ap.parse_args(argv)


def table(title, header, rows):
    return [title, "", "| " + " | ".join(header) + " |", "|" + "---|" * len(header)] + ["| " + " | ".join(r) + " |" for r in rows] + [""]


def stats_row(name, v, base):
    med = statistics.median
    return [name, f"{med(v):.2f}", f"{min(v):.2f}", f"{max(v):.2f}", f"{(max(v) - min(v)) / med(v):.1%}", f"{med(v) / base:.4f}"]


def main(argv=None):
    args = parse(argv)
    root = args.root.resolve()
    sys.path.insert(0, str(root / "longcat-video-tta_amd")); sys.path.insert(0, str(root))
    import functools
    import torch
    from torch.utils.checkpoint import checkpoint
    from lcv_hip import lib, ops
    from longcat_video.modules.longcat_video_dit import LongCatVideoTransformer3DModel
    from tta import full_tta, lora
    from tta.inner_loop import choose_gradient_checkpointing, finetune_lora_on_conditioning

    if not torch.cuda.is_available():
        raise SystemExit("master_weights_ab: no GPU; a time measured anywhere else says nothing")
    has_flag = "master_weights" in inspect.signature(full_tta.finetune_full_on_conditioning).parameters
    forms = [("off", {})] + ([("on", {"master_weights": True})] if has_flag else [])
    only = set(args.only.split(","))
    dev, bf = "cuda", torch.bfloat16
    (h, w), (tc, tt) = (60, 104), (3, 1)
    tokens = (tc + tt) * (h // 2) * (w // 2)
    dit = LongCatVideoTransformer3DModel(device=dev, dtype=bf, depth=args.depth).eval().init_synthetic_()
    g = torch.Generator(device=dev).manual_seed(1)
    cond = torch.randn(1, 16, tc, h, w, device=dev, generator=g).to(bf)
    train = torch.randn(1, 16, tt, h, w, device=dev, generator=g).to(bf)
    pe = torch.randn(1, 1, 512, 4096, device=dev, generator=g).to(bf)
    pm = torch.zeros(1, 512, dtype=torch.int64, device=dev); pm[:, :77] = 1
    n_params = sum(p.numel() for p in dit.parameters())
    lines = [f"Tree {root.name}, library version {lib.load().lcv_version()}, depth {args.depth} ({n_params / 1e9:.2f} B parameters), "
             f"480p ({tokens} tokens); {args.rounds} interleaved rounds after one warm-up run per form.  Spread = (max - min) / median.", ""]

    def full_mode():
        dit.gradient_checkpointing = True
        dit._gradient_checkpointing_func = functools.partial(checkpoint, use_reentrant=False)
        for p in dit.parameters():
            p.requires_grad = True

    def full_run(flag, n, lr=1e-5):
        r = full_tta.finetune_full_on_conditioning(dit, cond, train, pe, pm, num_steps=n, lr=lr, warmup_steps=0, device=dev, dtype=bf,
                                                   **flag)
        torch.cuda.synchronize()
        return r["train_time"] / n * 1e3

    if "full" in only:
        full_mode()
        for _, flag in forms:
            full_run(flag, 1)
        times = {name: [] for name, _ in forms}
        for _ in range(args.rounds):
            for name, flag in forms:
                times[name].append(full_run(flag, args.steps))
        lines += table(f"Full-model step (clip + SGD, block checkpointing on), {args.steps} steps per run",
                       ["master weights", "step time (ms), median", "min", "max", "spread", "ratio to off"],
                       [stats_row(name, times[name], statistics.median(times["off"])) for name, _ in forms])
        lines += [f"Peak memory {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB.", ""]

    if "opt" in only:
        full_mode()
        params = [p for p in dit.parameters()]
        for p in params:
            p.grad = torch.full_like(p, 1e-4)
        keep = [p.detach().clone() for p in params]                  # the timing loops move the weights: put them back after

        def timed(fn):
            fn(); torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.iters):
                fn()
            b.record(); torch.cuda.synchronize()
            return a.elapsed_time(b) / args.iters

        rows = []
        # algorithmic bytes per parameter: clip reads the gradient; SGD 4 + 2 (master 6 + 4); AdamW 8 + 6 (master 14 + 12)
        for kind, make, nbytes in (("SGD", lambda **k: ops.FusedSGDClip(params, lr=1e-5, **k), {"off": 6, "on": 10}),
                                   ("AdamW", lambda **k: ops.FusedAdamWClip(params, lr=1e-5, **k), {"off": 14, "on": 26})):
            for name, flag in forms:
                try:
                    opt = make(**flag)
                except torch.cuda.OutOfMemoryError:
                    rows.append([kind, name, "out of memory", "", "", ""])
                    continue
                clip = [timed(lambda: opt.clip_grad_norm_(1.0)) for _ in range(args.rounds)]
                step = [timed(opt.step) for _ in range(args.rounds)]
                ms = statistics.median(step)
                rows.append([kind, name, f"{statistics.median(clip):.2f}", f"{ms:.2f}", f"{(max(step) - min(step)) / ms:.1%}",
                             f"{n_params * nbytes[name] / ms / 1e9:.2f}"])
                del opt
                torch.cuda.empty_cache()
        with torch.no_grad():
            torch._foreach_copy_([p.detach() for p in params], keep)
        del keep
        for p in params:
            p.grad = None
        lines += table(f"Optimizer launches alone over the full parameter table ({len(params)} tensors), {args.iters} calls per timing",
                       ["optimizer", "master weights", "clip (ms), median", "update (ms), median", "update spread", "update TB/s (algorithmic)"],
                       rows)

    if "drift" in only and has_flag:
        full_mode()
        params = [p for p in dit.parameters()]
        base = [p.detach().clone() for p in params]
        made = []

        class Keep(ops.FusedSGDClip):
            def __init__(self, *a, **k):
                super().__init__(*a, **k)
                made[:] = [self]
        orig = full_tta.FusedSGDClip
        full_tta.FusedSGDClip = Keep
        rows = []
        try:
            for name, flag in forms:
                torch.manual_seed(1234)
                full_tta.finetune_full_on_conditioning(dit, cond, train, pe, pm, num_steps=20, lr=1e-5, warmup_steps=2, device=dev,
                                                       dtype=bf, **flag)
                torch.cuda.synchronize()
                lows = made[0].low_words or [None] * len(params)
                changed, sq = 0, 0.0
                for p, low, b in zip(params, lows, base):
                    changed += int((p.detach().view(torch.int16) != b.view(torch.int16)).sum().item())
                    if low is None:
                        m = p.detach().float()
                    else:
                        m = torch.empty(p.shape, dtype=torch.float32, device=dev)
                        lib.call("lcv_master_join", p.data_ptr(), low.data_ptr(), m.data_ptr(), p.numel(),
                                 torch.cuda.current_stream().cuda_stream)
                    sq += float((m - b.float()).double().pow(2).sum().item())
                    del m
                rows.append([name, f"{changed}", f"{changed / n_params:.3e}", f"{sq ** 0.5:.4e}"])
                made[:] = []
                with torch.no_grad():
                    torch._foreach_copy_([p.detach() for p in params], base)
        finally:
            full_tta.FusedSGDClip = orig
        del base
        torch.cuda.empty_cache()
        lines += table("20 full-model steps at lr = 1e-5 (SGD, wd 0.01, clip 1.0, warm-up 2), against the base weights",
                       ["master weights", "bf16 words changed", "share of elements", "norm of master - base"], rows)

    if "lora" in only:
        for p in dit.parameters():
            p.requires_grad = False
            p.grad = None
        ckpt = choose_gradient_checkpointing(dit, tokens)

        def lora_run(flag, n):
            torch.manual_seed(1234)
            mods = lora.inject_lora_into_dit(dit, rank=8, alpha=16.0, dropout=0.0, target_modules=["qkv", "proj"], target_ffn=False,
                                             target_blocks="all")
            try:
                r = finetune_lora_on_conditioning(dit, mods, cond, train, pe, pm, num_steps=n, lr=2e-4, warmup_steps=0, device=dev,
                                                  dtype=bf, **flag)
                torch.cuda.synchronize()
            finally:
                lora.remove_lora_from_dit(dit)
            return r["train_time"] * 1e3
        for _, flag in forms:
            lora_run(flag, 1)
        times = {name: [] for name, _ in forms}
        for _ in range(args.rounds):
            for name, flag in forms:
                times[name].append(lora_run(flag, 20))
        lines += table(f"20-step LoRA loop (qkv + proj adapters, r = 8, block checkpointing {'on' if ckpt else 'off'}), whole loop",
                       ["master weights", "loop time (ms), median", "min", "max", "spread", "ratio to off"],
                       [stats_row(name, times[name], statistics.median(times["off"])) for name, _ in forms])

    text = "\n".join(lines)
    print(text, flush=True)
    if args.out is not None:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text(text + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Cost of fp32 gradient accumulation (`grad_accum=N`, include/lcv_hip_accum.h) at the reference's operating point (480p:
Tc=3 + Tt=1 latent frames, 6 240 tokens): `python tools/grad_accum_ab.py [--depth 48] [--rounds 3] [--steps 10]
[--out profiles/grad_accum.md] [--only lora,kernel] [--root TREE]`.

One process, one model; forms alternate `rounds` times after one warm-up run each, so that clock and allocator drift hit all
alike.  Two sections:
  lora    the LoRA optimizer step (qkv + proj adapters, r = 8, clip + AdamW) for N = 1 (the flag absent: today's call
          sequence), 2 and 4 (with master weights); time per OPTIMIZER step is the loop's own `train_time` / steps
  kernel  lcv_grad_accumulate alone over the full parameter table (bf16 gradients, fp32 accumulators at every DiT tensor's
          size): a child process of its own under `rocprofv3 --kernel-trace --stats`, kernel time from its statistics,
          achieved bytes / s = 10 B x elements / time
`--root TREE` imports the packages from another checkout (the parent commit's, with its own built library): a tree whose loops
do not know the keyword gets N = 1 only, which is how the parent's own step time and run-to-run spread are measured."""
import argparse
import csv
import inspect
import statistics
import subprocess
import sys
import tempfile
from pathlib import Path

HERE = Path(__file__).resolve().parents[1]
KERNEL = "grad_accumulate_kernel"


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--depth", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", type=Path, default=None)
    ap.add_argument("--only", type=str, default="lora,kernel")
    ap.add_argument("--root", type=Path, default=HERE)
    ap.add_argument("--kernel-child", action="store_true", help="internal: the launches the kernel section profiles")
    return ap.parse_args(argv)


def table(title, header, rows):
    return [title, "", "| " + " | ".join(header) + " |", "|" + "---|" * len(header)] + ["| " + " | ".join(r) + " |" for r in rows] + [""]


def stats_row(name, v, base):
    med = statistics.median
    return [name, f"{med(v):.2f}", f"{min(v):.2f}", f"{max(v):.2f}", f"{(max(v) - min(v)) / med(v):.1%}", f"{med(v) / base:.4f}"]


def _imports(root: Path):
    sys.path.insert(0, str(root / "longcat-video-tta_amd")); sys.path.insert(0, str(root))


def kernel_child(args):
    """`iters` launches of lcv_grad_accumulate over one table with every DiT parameter tensor's size; prints the element count."""
    _imports(args.root.resolve())
    import torch
    from lcv_hip import lib
    from longcat_video.modules.longcat_video_dit import LongCatVideoTransformer3DModel
    numels = [p.numel() for p in LongCatVideoTransformer3DModel(device="meta", depth=args.depth).parameters()]
    dev = "cuda"
    grads = [torch.full((n,), 1e-4, dtype=torch.bfloat16, device=dev) for n in numels]
    accs = [torch.zeros(n, dtype=torch.float32, device=dev) for n in numels]
    rows, chunk = [], 0
    for g, n in zip(grads, numels):
        rows.append([0, g.data_ptr(), 0, 0, n, chunk])
        chunk += (n + 2047) // 2048
    desc = torch.tensor(rows, dtype=torch.int64).to(dev)
    ptrs = torch.tensor([a.data_ptr() for a in accs], dtype=torch.int64).to(dev)
    stream = torch.cuda.current_stream().cuda_stream
    for _ in range(args.iters + 1):                                           # the first launch is the warm-up
        lib.call("lcv_grad_accumulate", desc.data_ptr(), ptrs.data_ptr(), len(numels), chunk, 0.25, stream)
    torch.cuda.synchronize()
    print(f"ELEMENTS {sum(numels)} TENSORS {len(numels)}", flush=True)


def kernel_section(args):
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, str(Path(__file__).resolve()),
               "--kernel-child", "--depth", str(args.depth), "--iters", str(args.iters), "--root", str(args.root)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit(f"grad_accum_ab: the profiled child failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        words = next(ln for ln in r.stdout.splitlines() if ln.startswith("ELEMENTS")).split()
        elements, tensors = int(words[1]), int(words[3])
        stats = next(Path(tmp).rglob("*kernel_stats.csv"), None)
        if stats is not None:
            row = next(x for x in csv.DictReader(open(stats)) if KERNEL in x["Name"])
            calls = int(row["Calls"])
            avg, lo, hi = (float(row[k]) / 1e6 for k in ("AverageNs", "MinNs", "MaxNs"))
        else:                                  # no statistics file: the same figures from the trace's own timestamps
            trace = next(Path(tmp).rglob("*kernel_trace.csv"))
            ns = [float(x["End_Timestamp"]) - float(x["Start_Timestamp"]) for x in csv.DictReader(open(trace))
                  if KERNEL in x["Kernel_Name"]]
            calls, avg, lo, hi = len(ns), sum(ns) / len(ns) / 1e6, min(ns) / 1e6, max(ns) / 1e6
    tb = lambda ms: f"{elements * 10 / ms / 1e9:.2f}"
    return table(f"lcv_grad_accumulate alone over the full parameter table ({tensors} tensors, {elements / 1e9:.2f} B elements), "
                 f"{calls} launches under rocprofv3 --kernel-trace --stats (the first is the warm-up)",
                 ["kernel", "average (ms)", "min", "max", "TB/s at the average (10 B x elements)", "TB/s at the min"],
                 [[KERNEL, f"{avg:.2f}", f"{lo:.2f}", f"{hi:.2f}", tb(avg), tb(lo)]])


def main(argv=None):
    args = parse(argv)
    if args.kernel_child:
        return kernel_child(args)
    root = args.root.resolve()
    only = set(args.only.split(","))
    lines = []
    if "kernel" in only:                       # first: the child has the GPU to itself before this process opens it
        lines += kernel_section(args)
    if "lora" in only:
        _imports(root)
        import torch
        from lcv_hip import lib
        from longcat_video.modules.longcat_video_dit import LongCatVideoTransformer3DModel
        from tta import lora
        from tta.inner_loop import choose_gradient_checkpointing, finetune_lora_on_conditioning
        if not torch.cuda.is_available():
            raise SystemExit("grad_accum_ab: no GPU; a time measured anywhere else says nothing")
        has_flag = "grad_accum" in inspect.signature(finetune_lora_on_conditioning).parameters
        forms = [("1 (flag absent)", {})] + ([(str(n), {"master_weights": True, "grad_accum": n}) for n in (2, 4)] if has_flag else [])
        dev, bf = "cuda", torch.bfloat16
        (h, w), (tc, tt) = (60, 104), (3, 1)
        tokens = (tc + tt) * (h // 2) * (w // 2)
        dit = LongCatVideoTransformer3DModel(device=dev, dtype=bf, depth=args.depth).eval().init_synthetic_()
        g = torch.Generator(device=dev).manual_seed(1)
        cond = torch.randn(1, 16, tc, h, w, device=dev, generator=g).to(bf)
        train = torch.randn(1, 16, tt, h, w, device=dev, generator=g).to(bf)
        pe = torch.randn(1, 1, 512, 4096, device=dev, generator=g).to(bf)
        pm = torch.zeros(1, 512, dtype=torch.int64, device=dev); pm[:, :77] = 1
        for p in dit.parameters():
            p.requires_grad = False
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
            return r["train_time"] / n * 1e3
        for _, flag in forms:
            lora_run(flag, 1)
        times = {name: [] for name, _ in forms}
        for k in range(args.rounds):
            for name, flag in forms:
                times[name].append(lora_run(flag, args.steps))
            print(f"# round {k + 1} of {args.rounds} done", file=sys.stderr, flush=True)
        base = statistics.median(times[forms[0][0]])
        lines = [f"Tree {root.name}, library version {lib.load().lcv_version()}, depth {args.depth}, 480p ({tokens} tokens); "
                 f"{args.rounds} interleaved rounds after one warm-up run per form.  Spread = (max - min) / median.", ""] + lines
        lines += table(f"LoRA optimizer step (qkv + proj adapters, r = 8, block checkpointing {'on' if ckpt else 'off'}), "
                       f"{args.steps} optimizer steps per run",
                       ["micro-steps N", "time per optimizer step (ms), median", "min", "max", "spread", "ratio to N = 1"],
                       [stats_row(name, times[name], base) for name, _ in forms])
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out is not None:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text(text + "\n")


if __name__ == "__main__":
    main()

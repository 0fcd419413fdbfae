#!/usr/bin/env python3
"""Cost of the fp32 weight average (`weight_ema` / `--weight-ema`, include/lcv_hip_ema.h) at the reference's operating point
(480p: Tc=3 + Tt=1 latent frames, 6 240 tokens): `python tools/weight_ema_ab.py [--depth 48] [--rounds 3] [--steps 5]
[--out profiles/weight_ema.md] [--only regs,kernel,full,lora] [--parent TREE]`.

Four sections:
  regs    the three kernels' register counts and scratch, read from the device assembly that the library's own recipe
          (lcv_hip/build.py) gives for csrc/optim_ema.hip; needs no GPU
  kernel  every kernel of the average, and the plain master-weight SGD step as the counterpart, alone over the full parameter
          table (every DiT tensor's size): a child process of its own under `rocprofv3 --kernel-trace --stats`, kernel time from
          its trace, achieved bytes / s = the bytes per element the header states x elements / time
  full    the full-model step (SGD, clip, block checkpointing as run_full_tta.py sets it) with the flags absent, with master
          weights, and with master weights and the average; time per step is the loop's own `train_time` / steps
  lora    the LoRA step (rank 8 on qkv + proj of every block, AdamW, clip) in the same three forms
`--parent TREE` is a checkout of the parent commit with its own built library.  The step sections then run one child process
per tree, each with its own 48-block model, and the driver asks them for one run at a time, the parent's and this tree's run of a
form back to back in every round: clock and allocator drift hit both alike, and the parent's own run-to-run range is the
yardstick for this tree's flag-off medians.  A tree whose loops do not know the keyword gets the first two forms only."""
import argparse
import csv
import functools
import inspect
import re
import statistics
import subprocess
import sys
import tempfile
from pathlib import Path

HERE = Path(__file__).resolve().parents[1]
# kernel name in the trace -> (entry point, bytes read + written per element as the headers state them)
KERNELS = [("master_sgd_kernel<false, false>", "lcv_master_sgd_step (the counterpart)", 10), ("master_ema_kernel<0>", "lcv_master_ema_load", 8),
           ("master_ema_kernel<1>", "lcv_master_ema_update", 12), ("master_ema_kernel<2>", "lcv_master_ema_swap", 16)]
FORMS = [("flags absent", {}), ("--master-weights", {"master_weights": True}),
         ("--master-weights --weight-ema 0.9", {"master_weights": True, "weight_ema": 0.9})]


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--depth", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", type=Path, default=None)
    ap.add_argument("--only", type=str, default="regs,kernel,full,lora")
    ap.add_argument("--parent", type=Path, default=None)
    ap.add_argument("--root", type=Path, default=HERE, help="internal: the tree a child process imports")
    ap.add_argument("--kernel-child", action="store_true", help="internal: the launches the kernel section profiles")
    ap.add_argument("--serve", action="store_true", help="internal: one tree's model, one run per line of standard input")
    return ap.parse_args(argv)


def table(title, header, rows):
    return [title, "", "| " + " | ".join(header) + " |", "|" + "---|" * len(header)] + ["| " + " | ".join(r) + " |" for r in rows] + [""]


def _imports(root: Path):
    sys.path.insert(0, str(root / "longcat-video-tta_amd")); sys.path.insert(0, str(root))


# ------------------------------------------------------------------------------------------------------------ regs
def regs_section():
    _imports(HERE)
    from lcv_hip import build
    src = build.CSRC / "optim_ema.hip"
    with tempfile.TemporaryDirectory() as tmp:
        out = Path(tmp) / "optim_ema.s"
        cmd = [build.HIPCC, *build.FLAGS, *build.EXTRA.get(src.name, []), "--cuda-device-only", "-S", str(src), "-o", str(out)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit(f"weight_ema_ab: hipcc -S failed:\n{r.stderr[-2000:]}")
        text = out.read_text()
    rows = []
    for m in re.finditer(r"\.amdhsa_kernel\s+(\S+)(.*?)\.end_amdhsa_kernel", text, flags=re.S):
        sym, body = m.group(1), m.group(2)
        field = lambda name: re.search(rf"\.amdhsa_{name}\s+(\S+)", body).group(1)
        mode = re.search(r"master_ema_kernelILi(\d)E", sym)
        rows.append([f"`master_ema_kernel<{mode.group(1)}>`" if mode else f"`{sym}`", field("next_free_vgpr"), field("next_free_sgpr"),
                     field("accum_offset"), field("private_segment_fixed_size"), field("group_segment_fixed_size")])
    return table("Registers, scratch and LDS of the kernels (device assembly of csrc/optim_ema.hip, the library's flags; <0> load, "
                 "<1> update, <2> swap)", ["kernel", "VGPRs", "SGPRs", "AGPR offset", "scratch (B)", "LDS (B)"], rows)


# ------------------------------------------------------------------------------------------------------------ kernel
def kernel_child(args):
    """`iters` + 1 launches of every kernel over one table with every DiT parameter tensor's size; prints the element count."""
    _imports(args.root.resolve())
    import torch
    from lcv_hip import lib
    from longcat_video.modules.longcat_video_dit import LongCatVideoTransformer3DModel
    numels = [p.numel() for p in LongCatVideoTransformer3DModel(device="meta", depth=args.depth).parameters()]
    dev, stream = "cuda", torch.cuda.current_stream().cuda_stream
    n = len(numels)
    chunks = sum((m + 2047) // 2048 for m in numels)
    make = lambda dtype, value: [torch.full((m,), value, dtype=dtype, device=dev) for m in numels]
    ptrs = lambda ts: torch.tensor([t.data_ptr() for t in ts], dtype=torch.int64).to(dev)

    def run(name, *a):
        for _ in range(args.iters + 1):                                       # the first launch is the warm-up
            lib.call(name, *a, stream)
        torch.cuda.synchronize()
    P, L, G, E = make(torch.bfloat16, 1.0), make(torch.int16, 0), make(torch.bfloat16, 1e-4), make(torch.float32, 0.5)
    rows, chunk = [], 0
    for p, g, k in zip(P, G, numels):
        rows.append([p.data_ptr(), g.data_ptr(), p.data_ptr(), p.data_ptr(), k, chunk])
        chunk += (k + 2047) // 2048
    d, lp, ep = torch.tensor(rows, dtype=torch.int64).to(dev), ptrs(L), ptrs(E)
    run("lcv_master_sgd_step", d.data_ptr(), lp.data_ptr(), n, chunks, None, 1e-5, 0.01)
    run("lcv_master_ema_update", d.data_ptr(), lp.data_ptr(), ep.data_ptr(), n, chunks, 0.9)
    run("lcv_master_ema_swap", d.data_ptr(), lp.data_ptr(), ep.data_ptr(), n, chunks)
    run("lcv_master_ema_load", d.data_ptr(), lp.data_ptr(), ep.data_ptr(), n, chunks)
    print(f"ELEMENTS {sum(numels)} TENSORS {n} CHUNKS {chunks}", flush=True)


def kernel_section(args):
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, str(Path(__file__).resolve()),
               "--kernel-child", "--depth", str(args.depth), "--iters", str(args.iters)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit(f"weight_ema_ab: the profiled child failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
        words = next(ln for ln in r.stdout.splitlines() if ln.startswith("ELEMENTS")).split()
        elements, tensors = int(words[1]), int(words[3])
        trace = next(Path(tmp).rglob("*kernel_trace.csv"))
        ns = {}
        for x in csv.DictReader(open(trace)):
            ns.setdefault(x["Kernel_Name"], []).append(float(x["End_Timestamp"]) - float(x["Start_Timestamp"]))
    rows = []
    for kernel, entry, nbytes in KERNELS:
        name = next((k for k in ns if k.split("(")[0].replace("void ", "").strip().removesuffix(".kd") == kernel), None)
        if name is None:
            rows.append([kernel, entry, "not in the trace", "", "", "", ""])
            continue
        v = [t / 1e6 for t in ns[name][1:]]                                   # without the warm-up launch
        rows.append([f"`{kernel}`", entry, str(nbytes), f"{statistics.mean(v):.2f}", f"{min(v):.2f}", f"{max(v):.2f}",
                     f"{elements * nbytes / statistics.mean(v) / 1e9:.2f}"])
    return table(f"Every kernel alone over the full parameter table ({tensors} tensors, {elements / 1e9:.2f} B elements), "
                 f"{args.iters} launches each after one warm-up launch, under rocprofv3 --kernel-trace",
                 ["kernel", "entry point", "B / element", "average (ms)", "min", "max", "TB/s at the average"], rows)


# ------------------------------------------------------------------------------------------------------------ full, lora
def serve(args):
    """One tree's packages and one model; a line `full|lora FORM STEPS` on standard input runs that form once and answers
    `RESULT ms-per-step`; `forms` answers how many of FORMS this tree knows; end of input ends the process."""
    _imports(args.root.resolve())
    import torch
    from torch.utils.checkpoint import checkpoint
    from longcat_video.modules.longcat_video_dit import LongCatVideoTransformer3DModel
    from tta import full_tta, inner_loop
    from tta.lora import inject_lora_into_dit, reset_lora_weights
    if not torch.cuda.is_available():
        raise SystemExit("weight_ema_ab: no GPU; a time measured anywhere else says nothing")
    known = 3 if "weight_ema" in inspect.signature(full_tta.finetune_full_on_conditioning).parameters else 2
    dev, bf = "cuda", torch.bfloat16
    (h, w), (tc, tt) = (60, 104), (3, 1)
    dit = LongCatVideoTransformer3DModel(device=dev, dtype=bf, depth=args.depth).eval().init_synthetic_()
    dit.gradient_checkpointing = True                                         # as the runners set it at this size
    dit._gradient_checkpointing_func = functools.partial(checkpoint, use_reentrant=False)
    g = torch.Generator(device=dev).manual_seed(1)
    cond = torch.randn(1, 16, tc, h, w, device=dev, generator=g).to(bf)
    train = torch.randn(1, 16, tt, h, w, device=dev, generator=g).to(bf)
    pe = torch.randn(1, 1, 512, 4096, device=dev, generator=g).to(bf)
    pm = torch.zeros(1, 512, dtype=torch.int64, device=dev); pm[:, :77] = 1
    mods = None
    print("READY", flush=True)
    for line in sys.stdin:
        words = line.split()
        if not words:
            continue
        if words[0] == "forms":
            print(f"RESULT {known}", flush=True)
            continue
        section, flag, n = words[0], FORMS[int(words[1])][1], int(words[2])
        torch.manual_seed(1234)
        if section == "full":                      # lr 1e-5 from wherever the last run left the weights: the time does not care
            for p in dit.parameters():
                p.requires_grad = True
            r = full_tta.finetune_full_on_conditioning(dit, cond, train, pe, pm, num_steps=n, lr=1e-5, warmup_steps=0, device=dev,
                                                       dtype=bf, **flag)
        else:
            if mods is None:                       # after the full-model section: the base is frozen from here on
                for p in dit.parameters():
                    p.requires_grad = False
                mods = inject_lora_into_dit(dit, rank=8, alpha=16.0, target_modules=["qkv", "proj"], target_ffn=False,
                                            target_blocks="all")
                inner_loop.choose_gradient_checkpointing(dit, (tc + tt) * (h // 2) * (w // 2))     # as run_lora_tta.py does
            reset_lora_weights(mods)
            r = inner_loop.finetune_lora_on_conditioning(dit, mods, cond, train, pe, pm, num_steps=n, lr=2e-4, warmup_steps=0,
                                                         device=dev, dtype=bf, **flag)
        torch.cuda.synchronize()
        ms = r["train_time"] / n * 1e3
        del r            # freed blocks stay in this process's allocator: what goes back to the driver and is taken by the other
        print(f"RESULT {ms!r}", flush=True)         # tree's process costs that process seconds per run


class Tree:
    def __init__(self, name: str, root: Path, args):
        self.name = name
        cmd = [sys.executable, str(Path(__file__).resolve()), "--serve", "--root", str(root), "--depth", str(args.depth)]
        self.proc = subprocess.Popen(cmd, stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)
        self._answer("READY")
        self.forms = int(self.ask("forms"))

    def _answer(self, word: str) -> str:
        for line in self.proc.stdout:
            if line.startswith(word):
                return line[len(word):].strip()
        raise SystemExit(f"weight_ema_ab: the process of {self.name} ended ({self.proc.wait()}) before it answered")

    def ask(self, line: str) -> str:
        self.proc.stdin.write(line + "\n")
        self.proc.stdin.flush()
        return self._answer("RESULT")

    def close(self) -> None:
        self.proc.stdin.close()
        self.proc.wait(timeout=120)


def step_sections(args, only):
    trees = ([Tree("the parent commit", args.parent.resolve(), args)] if args.parent else []) + [Tree("this tree", HERE, args)]
    lines = []
    try:
        for section, title in (("full", "Full-model step (SGD, clip at 1.0, block checkpointing on)"),
                               ("lora", "LoRA step (rank 8 on qkv + proj of all blocks, AdamW, clip at 1.0, checkpointing as run_lora_tta.py chooses it)")):
            if section not in only:
                continue
            runs = [(k, t) for k in range(len(FORMS)) for t in trees if k < t.forms]
            for k, t in runs:                                                     # one warm-up run per form and tree
                t.ask(f"{section} {k} 1")
            times = {run: [] for run in runs}
            for rnd in range(args.rounds):
                for k, t in runs:
                    times[(k, t)].append(float(t.ask(f"{section} {k} {args.steps}")))
                print(f"# {section}: round {rnd + 1} of {args.rounds} done", file=sys.stderr, flush=True)
            med = statistics.median
            rows, verdicts = [], []
            for k, t in runs:
                v = times[(k, t)]
                rows.append([FORMS[k][0], t.name, f"{med(v):.2f}", f"{min(v):.2f}", f"{max(v):.2f}", f"{(max(v) - min(v)) / med(v):.1%}"])
                if args.parent and t is trees[-1] and k < trees[0].forms:
                    p = times[(k, trees[0])]
                    inside = min(p) <= med(v) <= max(p)
                    verdicts.append(f"{FORMS[k][0]}: this tree's median {med(v):.2f} ms is {'inside' if inside else 'OUTSIDE'} the "
                                    f"parent's range {min(p):.2f}-{max(p):.2f} ms (parent's median {med(p):.2f}, spread "
                                    f"{(max(p) - min(p)) / med(p):.1%})")
            lines += table(f"{title}, {args.steps} steps per run, {args.rounds} interleaved rounds after one warm-up run each",
                           ["form", "tree", "time per step (ms), median", "min", "max", "spread"], rows)
            lines += [f"- {v}" for v in verdicts] + ([""] if verdicts else [])
    finally:
        for t in trees:
            t.close()
    return lines


def main(argv=None):
    args = parse(argv)
    if args.kernel_child:
        return kernel_child(args)
    if args.serve:
        return serve(args)
    only = set(args.only.split(","))
    lines = [f"Depth {args.depth}, 480p (6240 tokens).  Spread = (max - min) / median.", ""]
    if "regs" in only:
        lines += regs_section()
    if "kernel" in only:                       # before the step sections: the profiled child has the GPU to itself
        lines += kernel_section(args)
    if only & {"full", "lora"}:
        lines += step_sections(args, only)
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out is not None:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text(text + "\n")


if __name__ == "__main__":
    main()

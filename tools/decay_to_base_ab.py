#!/usr/bin/env python3
"""Cost of decay toward the base weights (`decay_to_base` / `--decay-to-base`, include/lcv_hip_anchor.h) at the reference's
operating point (480p: Tc=3 + Tt=1 latent frames, 6 240 tokens): `python tools/decay_to_base_ab.py [--depth 48] [--rounds 3]
[--steps 5] [--out profiles/decay_to_base.md] [--only kernel,full,norm] [--root TREE]`.

One process, one model; forms alternate `rounds` times after one warm-up run each, so that clock and allocator drift hit all
alike.  Three sections:
  kernel  every anchor kernel and its non-anchor counterpart alone over the full parameter table (every DiT tensor's size):
          a child process of its own under `rocprofv3 --kernel-trace --stats`, kernel time from its statistics, achieved
          bytes / s = the bytes per element the header states x elements / time
  full    the full-model step (SGD, clip, block checkpointing as run_full_tta.py sets it) with the flags absent, with master
          weights, and with master weights and the flag; time per step is the loop's own `train_time` / steps
  norm    the norm-tuning step (all_norm) in the same three forms
`--root TREE` imports the packages from another checkout (the parent commit's, with its own built library): a tree whose loops
do not know the keyword gets the first two forms only, which is how the parent's own step time and spread are measured."""
import argparse
import csv
import functools
import inspect
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

HERE = Path(__file__).resolve().parents[1]
# kernel name in the trace -> (entry point, bytes read + written per element as the headers state them)
# (the step kernels' template arguments: <fp32 gradient, anchor>, the 8-bit one's <anchor>)
KERNELS = [("master_sgd_kernel<false, false>", "lcv_master_sgd_step", 10), ("master_sgd_kernel<false, true>", "lcv_master_sgd_step_anchor", 12),
           ("master_sgd_kernel<true, false>", "lcv_master_sgd_step_g32", 12), ("master_sgd_kernel<true, true>", "lcv_master_sgd_step_anchor, fp32 gradient", 14),
           ("master_adamw_kernel<false, false>", "lcv_master_adamw_step", 26), ("master_adamw_kernel<false, true>", "lcv_master_adamw_step_anchor", 28),
           ("master_adamw8_kernel<false>", "lcv_master_adamw8_step", 14), ("master_adamw8_kernel<true>", "lcv_master_adamw8_step_anchor", 16),
           ("drift_chunk_kernel", "lcv_master_drift_sumsq: one partial per chunk", 6), ("drift_final_kernel", "lcv_master_drift_sumsq: the partials", 0)]


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--depth", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", type=Path, default=None)
    ap.add_argument("--only", type=str, default="kernel,full,norm")
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
    """`iters` + 1 launches of every kernel over one table with every DiT parameter tensor's size; prints the element count.
    The arrays of the three groups (SGD, AdamW with fp32 moments, AdamW with 8-bit moments) are live one group at a time."""
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

    def desc(P, G, M, V):
        rows, chunk = [], 0
        for p, g, m, v, k in zip(P, G, M, V, numels):
            rows.append([p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), k, chunk])
            chunk += (k + 2047) // 2048
        return torch.tensor(rows, dtype=torch.int64).to(dev)

    def run(name, *a):
        for _ in range(args.iters + 1):                                       # the first launch is the warm-up
            lib.call(name, *a, stream)
        torch.cuda.synchronize()
    P, L, A, G = make(torch.bfloat16, 1.0), make(torch.int16, 0), make(torch.bfloat16, 1.0078125), make(torch.bfloat16, 1e-4)
    lp, apt = ptrs(L), ptrs(A)
    d = desc(P, G, P, P)
    sgd = (None, 1e-5, 0.01)
    run("lcv_master_sgd_step", d.data_ptr(), lp.data_ptr(), n, chunks, *sgd)
    run("lcv_master_sgd_step_anchor", d.data_ptr(), lp.data_ptr(), apt.data_ptr(), n, chunks, *sgd, 0)
    part, out = torch.empty(chunks, dtype=torch.float32, device=dev), torch.empty(2, dtype=torch.float32, device=dev)
    run("lcv_master_drift_sumsq", d.data_ptr(), lp.data_ptr(), apt.data_ptr(), n, chunks, part.data_ptr(), chunks * 4, out.data_ptr())
    G32 = make(torch.float32, 1e-4)
    d32 = desc(P, G32, P, P)
    run("lcv_master_sgd_step_g32", d32.data_ptr(), lp.data_ptr(), n, chunks, *sgd)
    run("lcv_master_sgd_step_anchor", d32.data_ptr(), lp.data_ptr(), apt.data_ptr(), n, chunks, *sgd, 1)
    del G32, d32
    torch.cuda.empty_cache()
    adam = (None, 1e-5, 0.9, 0.999, 1e-8, 0.01, 1)
    M, V = make(torch.float32, 0.0), make(torch.float32, 0.0)
    dm = desc(P, G, M, V)
    run("lcv_master_adamw_step", dm.data_ptr(), lp.data_ptr(), n, chunks, *adam)
    run("lcv_master_adamw_step_anchor", dm.data_ptr(), lp.data_ptr(), apt.data_ptr(), n, chunks, *adam, 0)
    del M, V, dm
    torch.cuda.empty_cache()
    CM, CR = make(torch.uint8, 0), make(torch.uint8, 0)
    S = [torch.zeros((2, (m + 511) // 512), dtype=torch.float32, device=dev) for m in numels]
    d8, sp = desc(P, G, CM, CR), ptrs(S)
    run("lcv_master_adamw8_step", d8.data_ptr(), lp.data_ptr(), sp.data_ptr(), n, chunks, *adam)
    run("lcv_master_adamw8_step_anchor", d8.data_ptr(), lp.data_ptr(), sp.data_ptr(), apt.data_ptr(), n, chunks, *adam)
    print(f"ELEMENTS {sum(numels)} TENSORS {n} CHUNKS {chunks}", flush=True)


def kernel_section(args):
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable, str(Path(__file__).resolve()),
               "--kernel-child", "--depth", str(args.depth), "--iters", str(args.iters), "--root", str(args.root)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit(f"decay_to_base_ab: the profiled child failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
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
        tb = lambda ms: f"{elements * nbytes / ms / 1e9:.2f}" if nbytes else "-"
        rows.append([f"`{kernel}`", entry, str(nbytes) if nbytes else "4 per chunk", f"{statistics.mean(v):.2f}", f"{min(v):.2f}",
                     f"{max(v):.2f}", tb(statistics.mean(v))])
    return table(f"Every kernel alone over the full parameter table ({tensors} tensors, {elements / 1e9:.2f} B elements), "
                 f"{args.iters} launches each after one warm-up launch, under rocprofv3 --kernel-trace",
                 ["kernel", "entry point", "B / element", "average (ms)", "min", "max", "TB/s at the average"], rows)


def main(argv=None):
    args = parse(argv)
    if args.kernel_child:
        return kernel_child(args)
    root = args.root.resolve()
    only = set(args.only.split(","))
    lines = []
    if "kernel" in only:                       # first: the child has the GPU to itself before this process opens it
        lines += kernel_section(args)
    if only & {"full", "norm"}:
        _imports(root)
        import torch
        from torch.utils.checkpoint import checkpoint
        from lcv_hip import lib
        from longcat_video.modules.longcat_video_dit import LongCatVideoTransformer3DModel
        from tta import delta, full_tta
        if not torch.cuda.is_available():
            raise SystemExit("decay_to_base_ab: no GPU; a time measured anywhere else says nothing")
        has_flag = "decay_to_base" in inspect.signature(full_tta.finetune_full_on_conditioning).parameters
        dev, bf = "cuda", torch.bfloat16
        (h, w), (tc, tt) = (60, 104), (3, 1)
        tokens = (tc + tt) * (h // 2) * (w // 2)
        dit = LongCatVideoTransformer3DModel(device=dev, dtype=bf, depth=args.depth).eval().init_synthetic_()
        dit.gradient_checkpointing = True                                     # as run_full_tta.py sets it
        dit._gradient_checkpointing_func = functools.partial(checkpoint, use_reentrant=False)
        g = torch.Generator(device=dev).manual_seed(1)
        cond = torch.randn(1, 16, tc, h, w, device=dev, generator=g).to(bf)
        train = torch.randn(1, 16, tt, h, w, device=dev, generator=g).to(bf)
        pe = torch.randn(1, 1, 512, 4096, device=dev, generator=g).to(bf)
        pm = torch.zeros(1, 512, dtype=torch.int64, device=dev); pm[:, :77] = 1
        base = full_tta.snapshot_base_state(dit)
        forms = [("flags absent", {}), ("--master-weights", {"master_weights": True})]
        if has_flag:
            forms.append(("--master-weights --decay-to-base", {"master_weights": True, "decay_to_base": True}))

        def full_run(flag, n):
            for p in dit.parameters():
                p.requires_grad = True
            full_tta.reset_dit_weights(dit, base)
            torch.manual_seed(1234)
            extra = {"base_state": base} if flag.get("decay_to_base") else {}
            r = full_tta.finetune_full_on_conditioning(dit, cond, train, pe, pm, num_steps=n, lr=1e-5, warmup_steps=0, device=dev,
                                                       dtype=bf, **flag, **extra)
            torch.cuda.synchronize()
            return r["train_time"] / n * 1e3, r.get("drift_norm")

        def norm_run(flag, n):
            for p in dit.parameters():
                p.requires_grad = False
            wrap = delta.NormTuneForward(dit, "all_norm").to(dev)
            torch.manual_seed(1234)
            try:
                r = delta.optimize_norm_params(wrap, wrap.tuned_params, cond, train, pe, pm, num_steps=n, lr=1e-3, device=dev, dtype=bf,
                                               **flag)
                torch.cuda.synchronize()
            finally:
                wrap.restore()
            return r

        def norm_timed(flag, n):                                              # this loop reports no time of its own
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = norm_run(flag, n)                                             # ends in a synchronise
            return (time.perf_counter() - t0) / n * 1e3, r.get("drift_norm")

        lines = [f"Tree {root.name}, library version {lib.load().lcv_version()}, depth {args.depth}, 480p ({tokens} tokens); "
                 f"{args.rounds} interleaved rounds after one warm-up run per form.  Spread = (max - min) / median.", ""] + lines
        for section, runner, title in (("full", full_run, "Full-model step (SGD, clip at 1.0, block checkpointing on)"),
                                       ("norm", norm_timed, "Norm-tuning step (all_norm, AdamW, clip at 1.0; host clock around the loop)")):
            if section not in only:
                continue
            drift = {}
            for name, flag in forms:
                runner(flag, 1)
            times = {name: [] for name, _ in forms}
            for k in range(args.rounds):
                for name, flag in forms:
                    t, dn = runner(flag, args.steps)
                    times[name].append(t)
                    drift[name] = dn
                print(f"# {section}: round {k + 1} of {args.rounds} done", file=sys.stderr, flush=True)
            b = statistics.median(times[forms[0][0]])
            lines += table(f"{title}, {args.steps} steps per run",
                           ["form", "time per step (ms), median", "min", "max", "spread", "ratio to the first row"],
                           [stats_row(name, times[name], b) for name, _ in forms])
            lines += [f"drift_norm after {args.steps} steps: " +
                      ", ".join(f"{name}: {'-' if drift[name] is None else repr(drift[name])}" for name, _ in forms), ""]
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out is not None:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text(text + "\n")


if __name__ == "__main__":
    main()

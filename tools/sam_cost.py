"""Cost record of --sam-rho (profiles/sam.md).  Needs an MI355X.

  python tools/sam_cost.py kernels [--sizes delta-a,lora-r1,full] [--out rows.json]
      lcv_sam_sumsq, lcv_sam_perturb and lcv_sam_restore at the delta-A, the LoRA r = 1 and the modelled full-model size: device
      events around repeated whole calls, the algorithmic bytes and the rate.
  python tools/sam_cost.py step [--depth 48] [--rounds 3] [--steps 5] [--parent DIR] [--out rows.json]
      one LoRA adaptation step (rank 8 on qkv + proj of all blocks, 480p: 3 + 1 latent frames, 6 240 tokens) without the flag,
      with --sam-rho 0.05, and without the flag on the tree under DIR (the parent commit, built); each tree in a process of its
      own, every form `rounds` runs of `steps` steps after one warm-up run.
"""
import argparse
import functools
import json
import statistics
import subprocess
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parents[1]
DEV = "cuda"


def _imports(root: Path):
    sys.path.insert(0, str(root / "longcat-video-tta_amd"))


# ------------------------------------------------------------------------------------------------------------ kernels
def timed(fn, warm, reps):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3          # microseconds per call


def case(name, shapes, f32, master, reps):
    import torch
    from lcv_hip import ops
    dt = torch.float32 if f32 else torch.bfloat16
    params = [torch.empty(s, dtype=dt, device=DEV).normal_(0.0, 0.05) for s in shapes]
    n = sum(p.numel() for p in params)
    opt = ops.FusedSGDClip(params, lr=1e-6, weight_decay=0.01, master_weights=master)
    opt.enable_sam(0.05)
    for p in params:
        p.grad = torch.empty_like(p).normal_(0.0, 1e-3)
    assert opt._sam_measure()
    total = opt._sam_out[:1].clone()                # a total that stays put while the words move back and forth

    def perturb():
        opt._sam_perturb(total)
    row = {"case": name, "elements": n, "tensors": len(params), "dtype": "fp32" if f32 else ("bf16+low" if master else "bf16"),
           "sumsq_us": timed(opt._sam_measure, 3, reps), "perturb_us": timed(perturb, 3, reps),
           "restore_us": timed(opt._sam_restore, 3, reps)}
    word = 4 if f32 else 2
    row["sumsq_bytes"] = word * n                                   # plain: the gradients only
    row["perturb_bytes"] = (2 * word + (2 if master else 0)) * n + 2 * word * n      # word, gradient[, low word] read; save, word written
    row["restore_bytes"] = 2 * word * n
    for k in ("sumsq", "perturb", "restore"):
        row[k + "_GBps"] = row[k + "_bytes"] / row[k + "_us"] / 1e3
    print(json.dumps(row), flush=True)
    del opt, params
    torch.cuda.empty_cache()
    return row


CASES = {
    "delta-a": lambda: case("delta-A", [(512,)], True, False, 500),
    # LoRA r = 1 on qkv (4096 -> 12288) and proj (4096 -> 4096) of 48 blocks
    "lora-r1": lambda: case("LoRA r=1", [s for _ in range(48) for s in ((1, 4096), (12288, 1), (1, 4096), (4096, 1))], False, True,
                            500),
    # the full model's element count as 302 tensors of 4096 x 11008 (the real table has 1 022 tensors of 13.58 G elements):
    # 27 GB each of weights, gradients, low words and saved words
    "full": lambda: case("full model", [(4096, 11008)] * 302, False, True, 10),
}


# ------------------------------------------------------------------------------------------------------------ one LoRA step
FORMS = [("no flag", {}), ("--sam-rho 0.05", {"sam_rho": 0.05})]


def serve(args):
    """One tree's packages and one model: every form this tree knows, `rounds` runs of `steps` steps after a warm-up run."""
    _imports(args.root.resolve())
    import inspect
    import torch
    from torch.utils.checkpoint import checkpoint
    from longcat_video.modules.longcat_video_dit import LongCatVideoTransformer3DModel
    from tta import inner_loop
    from tta.lora import inject_lora_into_dit, reset_lora_weights
    bf = torch.bfloat16
    (h, w), (tc, tt) = (60, 104), (3, 1)
    dit = LongCatVideoTransformer3DModel(device=DEV, dtype=bf, depth=args.depth).eval().init_synthetic_()
    dit.gradient_checkpointing = True
    dit._gradient_checkpointing_func = functools.partial(checkpoint, use_reentrant=False)
    g = torch.Generator(device=DEV).manual_seed(1)
    cond = torch.randn(1, 16, tc, h, w, device=DEV, generator=g).to(bf)
    train = torch.randn(1, 16, tt, h, w, device=DEV, generator=g).to(bf)
    pe = torch.randn(1, 1, 512, 4096, device=DEV, generator=g).to(bf)
    pm = torch.zeros(1, 512, dtype=torch.int64, device=DEV)
    pm[:, :77] = 1
    for p in dit.parameters():
        p.requires_grad = False
    mods = inject_lora_into_dit(dit, rank=8, alpha=16.0, target_modules=["qkv", "proj"], target_ffn=False, target_blocks="all")
    inner_loop.choose_gradient_checkpointing(dit, (tc + tt) * (h // 2) * (w // 2))     # as run_lora_tta.py does
    known = "sam_rho" in inspect.signature(inner_loop.finetune_lora_on_conditioning).parameters
    forms = FORMS if known else FORMS[:1]

    def run(flag, n):
        reset_lora_weights(mods)
        torch.manual_seed(1234)
        r = inner_loop.finetune_lora_on_conditioning(dit, mods, cond, train, pe, pm, num_steps=n, lr=2e-4, warmup_steps=0,
                                                     device=DEV, dtype=bf, **flag)
        torch.cuda.synchronize()
        return r["train_time"] / n * 1e3
    for _, flag in forms:
        run(flag, 1)
    times = {name: [] for name, _ in forms}
    for _ in range(args.rounds):
        for name, flag in forms:
            times[name].append(run(flag, args.steps))
    print("RESULT " + json.dumps(times), flush=True)


def step_section(args):
    rows = []
    trees = [("this tree", HERE)] + ([("the parent commit", args.parent.resolve())] if args.parent else [])
    for tree, root in trees:
        cmd = [sys.executable, str(Path(__file__).resolve()), "serve", "--root", str(root), "--depth", str(args.depth),
               "--rounds", str(args.rounds), "--steps", str(args.steps)]
        out = subprocess.run(cmd, capture_output=True, text=True, check=True).stdout       # a fresh child process per tree
        times = json.loads(next(ln for ln in out.splitlines() if ln.startswith("RESULT "))[7:])
        for form, v in times.items():
            med = statistics.median(v)
            rows.append({"tree": tree, "form": form, "median_ms": med, "min_ms": min(v), "max_ms": max(v),
                         "spread": (max(v) - min(v)) / med, "runs": v})
            print(json.dumps(rows[-1]), flush=True)
    return rows


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("what", choices=["kernels", "step", "serve"])
    ap.add_argument("--sizes", default="delta-a,lora-r1,full", help="comma-separated subset of: " + ", ".join(CASES))
    ap.add_argument("--depth", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--parent", type=Path, default=None, help="a built checkout of the parent commit")
    ap.add_argument("--root", type=Path, default=HERE, help="internal: the tree a child process imports")
    ap.add_argument("--out", type=Path, default=None, help="write the rows to this JSON file as well")
    args = ap.parse_args(argv)
    if args.what == "serve":
        return serve(args)
    if args.what == "kernels":
        _imports(HERE)
        names = [n.strip() for n in args.sizes.split(",") if n.strip()]
        unknown = [n for n in names if n not in CASES]
        if unknown:
            ap.error(f"unknown size(s) {unknown}; choose from {list(CASES)}")
        rows = [CASES[n]() for n in names]
    else:
        rows = step_section(args)
    if args.out is not None:
        args.out.write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()

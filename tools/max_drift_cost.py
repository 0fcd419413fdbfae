"""Cost record of --max-drift (profiles/max_drift.md): lcv_trust_sumsq and a projecting lcv_trust_project at the delta-A, the
LoRA r = 1 and the full-model size, beside the optimizer step (clip + step) at the same size.  Device events around repeated
calls; needs an MI355X.  Usage: python tools/max_drift_cost.py [--sizes delta-a,lora-r1,full] [--out rows.json]"""
import argparse
import json
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "longcat-video-tta_amd"))
from lcv_hip import lib, ops, optim  # noqa: E402

DEV = "cuda"


def timed(fn, warm, reps):
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


def case(name, shapes, f32, kind, reps):
    dt = torch.float32 if f32 else torch.bfloat16
    params = [torch.empty(s, dtype=dt, device=DEV).normal_(0.0, 0.05) for s in shapes]
    n = sum(p.numel() for p in params)
    anchors = None if f32 else [(p.float() * 1.01).to(dt) for p in params]
    if kind == "sgd":
        opt = ops.FusedSGDClip(params, lr=1e-6, weight_decay=0.01, master_weights=not f32)
    else:
        opt = ops.FusedAdamWClip(params, lr=1e-6, weight_decay=0.01, master_weights=not f32)
    opt.enable_max_drift(1e-3, "global", anchor=anchors)
    for p in params:
        p.grad = torch.empty_like(p).normal_(0.0, 1e-3)

    def step():
        opt.clip_grad_norm_(1.0)
        opt.step()
    fake = torch.tensor([1.0, 1.0], dtype=torch.float32, device=DEV)

    def project():                                   # a stale total above the radius: every call projects, c = 0.999
        ops.call("lcv_trust_project", *opt._trust_args(), lib.LCV_TRUST_GLOBAL, fake.data_ptr(), opt._md_per.data_ptr(), 0.998001,
                 None, torch.cuda.current_stream().cuda_stream)
    row = {"case": name, "elements": n, "tensors": len(params), "dtype": "fp32" if f32 else "bf16+low",
           "step_us": timed(step, 3, reps), "sumsq_us": timed(opt.drift_sumsq, 3, reps), "project_us": timed(project, 3, reps)}
    rd = (4 if f32 else 6)
    row["sumsq_bytes"] = rd * n
    row["project_bytes"] = (rd + 4) * n
    row["sumsq_GBps"] = row["sumsq_bytes"] / row["sumsq_us"] / 1e3
    row["project_GBps"] = row["project_bytes"] / row["project_us"] / 1e3
    print(json.dumps(row), flush=True)
    del opt, params, anchors
    torch.cuda.empty_cache()
    return row


CASES = {
    "delta-a": lambda: case("delta-A", [(512,)], True, "adamw", 500),
    # LoRA r = 1 on qkv (4096 -> 12288) and proj (4096 -> 4096) of 48 blocks
    "lora-r1": lambda: case("LoRA r=1", [s for _ in range(48) for s in ((1, 4096), (12288, 1), (1, 4096), (4096, 1))], False,
                            "adamw", 500),
    # the full model's element count as 302 tensors of 4096 x 11008 (the real table has 1 022 tensors of 13.58 G elements);
    # about 108 GB of weights, low words, base words and gradients
    "full": lambda: case("full model", [(4096, 11008)] * 302, False, "sgd", 10),
}


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--sizes", default="delta-a,lora-r1,full", help="comma-separated subset of: " + ", ".join(CASES))
    ap.add_argument("--out", type=Path, default=None, help="write the rows to this JSON file as well")
    args = ap.parse_args(argv)
    names = [n.strip() for n in args.sizes.split(",") if n.strip()]
    unknown = [n for n in names if n not in CASES]
    if unknown:
        ap.error(f"unknown size(s) {unknown}; choose from {list(CASES)}")
    rows = [CASES[n]() for n in names]
    if args.out is not None:
        args.out.write_text(json.dumps(rows, indent=1))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""LoRA test-time adaptation runner on MI355X — same relative path, CLI flags and artifact schemas as the reference's
`lora_experiment/scripts/run_lora_tta.py` (flags :654-741; `config.json` :855-908; per-video result keys :1174-1248;
`checkpoint.json` = {next_idx, results}; `summary.json` :1276-1324), so `sweep_experiment/sbatch/run_sweep.sbatch:375-438`
drives it unchanged.

Inputs.  The hot path starts at latents: `--data-dir` holds `latents/*.pt` files
({"latents": [1,16,T,h,w] normalised VAE latents of the conditioning window, "prompt_embeds": [1,1,L,4096],
"prompt_mask": [1,L], optional "negative_embeds"/"negative_mask", "caption"}), or is `synthetic:N` for seeded synthetic
videos (plumbing / benchmarking).  Raw-video decoding, the VAE encoder and the UMT5 text encoder are the caller-side rows
that come next; pointing `--data-dir` at raw videos raises a per-video error that is recorded exactly the
way the reference records failures (:1264-1271).

Multi-GPU.  Launched under `torch.distributed.run` the videos are sharded `idx = rank (mod world)` (one video per
GPU, no data-path collective), each rank writes `checkpoint.rank{r}.json`, rank 0 merges into the reference-format
`checkpoint.json` / `summary.json`.  sigma / eps are re-seeded per video with `seed + idx` (the reference's single RNG
stream is sequential across videos; declared deviation).
"""
import argparse
import os
import sys
from pathlib import Path

_PKG = Path(__file__).resolve().parents[2]
if str(_PKG) not in sys.path:
    sys.path.insert(0, str(_PKG))

import torch  # noqa: E402

from tta import cli_args as C  # noqa: E402
from tta import runner_common as R  # noqa: E402
from tta.inner_loop import finetune_lora_on_conditioning  # noqa: E402
from tta.lora import (count_builtin_lora_parameters, get_builtin_lora_parameters, inject_builtin_lora_into_dit,  # noqa: E402
                      reset_builtin_lora_weights, save_builtin_lora_weights)
from tta.lora import (count_lora_parameters, get_dora_magnitudes, get_lora_parameters, inject_lora_into_dit,  # noqa: E402
                      reset_lora_weights, save_lora_weights)


def build_parser():
    p = argparse.ArgumentParser(description="LoRA TTA for LongCat-Video (MI355X)")
    R.add_common_args(p)
    p.add_argument("--restart", action="store_true")
    p.add_argument("--lora-rank", type=int, default=8)
    p.add_argument("--lora-alpha", type=float, default=16.0)
    p.add_argument("--lora-dropout", type=float, default=0.0)
    p.add_argument("--lora-dora", action="store_true",
                   help="weight-decomposed LoRA: every adapted linear also trains an fp32 magnitude per output, y = (m / |W + s B A|) "
                        "(.) (x W^T + s (x A^T) B^T) + b, the row norm a constant of the backward (include/lcv_hip_dora.h); custom "
                        "implementation only, not with --master-weights, --adam-8bit, --grad-accum above 1, --weight-ema or "
                        "--stochastic-rounding")
    p.add_argument("--target-ffn", action="store_true")
    p.add_argument("--target-modules", type=str, default="qkv,proj")
    p.add_argument("--lora-target-blocks", type=str, default="all")
    p.add_argument("--use-builtin-lora", action="store_true")
    p.add_argument("--save-lora-weights", action="store_true",
                   help="write every video's adapters; with --weight-ema they are the averaged adapters")
    p.add_argument("--learning-rate", type=float, default=2e-4)
    p.add_argument("--num-steps", type=int, default=20)
    p.add_argument("--warmup-steps", type=int, default=3)
    p.add_argument("--weight-decay", type=float, default=0.01)
    p.add_argument("--max-grad-norm", type=float, default=1.0)
    C.add_optimizer_args(p, master_weights_help="fp32 master weights for the bf16 adapters (include/lcv_hip_master.h); both "
                                                "LoRA implementations")
    p.add_argument("--batch-videos", type=int, default=1)
    p.add_argument("--batch-method", type=str, default="similarity", choices=["similarity", "sequential"])
    p.add_argument("--retrieval-pool-dir", type=str, default=None)
    R.add_shared_groups(p, clip_gate=True)
    return p


def check_lora_dora_args(args) -> None:
    """--lora-dora trains fp32 magnitudes with a plain AdamW of their own beside the bf16 adapters' (tta.inner_loop); the
    combinations that optimizer pair does not cover are refused here, before a model is loaded."""
    if not getattr(args, "lora_dora", False):
        return
    refusals = [
        (args.use_builtin_lora, "--use-builtin-lora (the builtin adapters are hooked forwards without a magnitude)"),
        (args.master_weights, "--master-weights (the magnitudes are fp32 already, and the joint clip reads bf16 .grad)"),
        (args.adam_8bit, "--adam-8bit (a master-weight form)"),
        (args.grad_accum > 1, "--grad-accum above 1 (the magnitudes' optimizer has no accumulators)"),
        (args.weight_ema is not None, "--weight-ema (the average is kept beside master weights only)"),
        (args.stochastic_rounding, "--stochastic-rounding (an fp32 magnitude has nothing to round, and a joint run would mix "
                                   "the two forms)"),
    ]
    for refused, what in refusals:
        if refused:
            raise ValueError(f"--lora-dora cannot be combined with {what}")


def parse_args(argv=None):
    args = C.parse_with_step_cache(build_parser(), argv, C.parse_optimizer_args)
    check_lora_dora_args(args)
    return args


def lora_method(args) -> R.TTAMethod:
    """The LoRA job as `R.run_tta_job` takes it: adapters injected once (custom or builtin, run_lora_tta.py:783, 818-846) and
    reset for every video, `config.json` in the reference's layout, `<name>_lora.pt` under --save-lora-weights."""
    check_lora_dora_args(args)
    dora = bool(getattr(args, "lora_dora", False))
    target_modules = [m.strip() for m in args.target_modules.split(",") if m.strip()]
    impl = "builtin" if args.use_builtin_lora else "custom"
    if impl == "builtin":                                      # its injector takes no dropout
        inject, inject_kw = inject_builtin_lora_into_dit, {}
        count, get_params, reset, save = (count_builtin_lora_parameters, get_builtin_lora_parameters, reset_builtin_lora_weights,
                                          save_builtin_lora_weights)
    else:
        inject, inject_kw = inject_lora_into_dit, {"dropout": args.lora_dropout, **({"dora": True} if dora else {})}   # flag absent: today's call
        count, get_params, reset, save = count_lora_parameters, get_lora_parameters, reset_lora_weights, save_lora_weights
    lora_dir = os.path.join(args.output_dir, "lora_weights")
    lora_modules = []                                          # filled once the model is loaded

    def prepare(dit):
        # run_lora_tta.py:806-811 switches block checkpointing on unconditionally; here it is decided per video from the
        # token count (LCV_TTA_CHECKPOINT=on reproduces the reference): see tta.inner_loop.choose_gradient_checkpointing
        for p in dit.parameters():                             # :813-815
            p.requires_grad = False
        lora_modules.extend(inject(dit, rank=args.lora_rank, alpha=args.lora_alpha, target_modules=target_modules,
                                   target_ffn=args.target_ffn, target_blocks=args.lora_target_blocks, **inject_kw))
        if args.save_lora_weights:
            os.makedirs(lora_dir, exist_ok=True)
        gate = R.clip_gate_summary(args)
        return {"method": f"lora_tta_{impl}",
                "lora": {"implementation": impl, "rank": args.lora_rank, "alpha": args.lora_alpha,
                         "dropout": args.lora_dropout, **({"dora": True} if dora else {}), "target_modules": target_modules,
                         "target_blocks": args.lora_target_blocks, "target_ffn": args.target_ffn,
                         "num_modules": len(lora_modules), "trainable_params": count(lora_modules)["trainable"]},
                "training": {"learning_rate": args.learning_rate, "num_steps": args.num_steps,
                             "warmup_steps": args.warmup_steps, "weight_decay": args.weight_decay,
                             "max_grad_norm": args.max_grad_norm, "master_weights": args.master_weights,
                             "adam_8bit": args.adam_8bit, "grad_accum": args.grad_accum, **C.weight_ema_record(args),
                             **C.stochastic_rounding_record(args), **C.max_drift_record(args),
                             **C.sam_record(args)},
                "generation": {"num_cond_frames": args.num_cond_frames, "num_frames": args.num_frames,
                               "num_inference_steps": args.num_inference_steps, "guidance_scale": args.guidance_scale,
                               "resolution": args.resolution, **C.step_cache_record(args),
                               **C.solver_record(args), **C.cfg_reuse_record(args),
                               **C.apg_record(args)},
                "seed": args.seed, "max_videos": args.max_videos,
                **{k: v for k, v in gate.items() if k != "clip_gate_stats"}}

    def adapt(dit, cond, train, pe, pm, device, es, variants):
        return finetune_lora_on_conditioning(dit, lora_modules, cond, train, pe, pm, num_steps=args.num_steps,
                                             lr=args.learning_rate, warmup_steps=args.warmup_steps,
                                             weight_decay=args.weight_decay, max_grad_norm=args.max_grad_norm, device=device,
                                             dtype=torch.bfloat16, early_stopper=es,
                                             lora_param_fn=lambda: get_params(lora_modules), train_latents_variants=variants,
                                             **({"dora_magnitudes": get_dora_magnitudes(lora_modules)} if dora else {}),
                                             **C.optimizer_kwargs(args))

    def row_extra(tr, variants, blob):
        return {"num_train_steps": len(tr["losses"]),
                **({"aug_variants": [v["name"] for v in variants]} if variants is not None else {}),
                **({} if args.skip_generation else {"cond_source": blob.get("_cond_source")}),
                **C.stochastic_rounding_record(args), **C.max_drift_result(tr), **C.sam_result(tr)}

    def summary_extra(merged, ok):
        return {"lora_rank": args.lora_rank, "lora_alpha": args.lora_alpha, "learning_rate": args.learning_rate,
                "num_steps": args.num_steps, "batch_videos": args.batch_videos, "retrieval_pool_dir": args.retrieval_pool_dir,
                **R.failed_and_final_loss(merged, ok),
                "clip_gate_enabled": False, "clip_gate_stats": {"skip_rate": 0.0, "num_skipped": 0, "num_scored": 0}}

    return R.TTAMethod(name="lora_tta", label="LoRA TTA", file_suffix="lora", prepare=prepare, adapt=adapt,
                       after_variants=lambda: reset(lora_modules), row_extra=row_extra, summary_extra=summary_extra,
                       on_success=((lambda e: save(lora_modules, os.path.join(lora_dir, f"{e['name']}_lora.pt")))
                                   if args.save_lora_weights else None))


def main(argv=None):
    args = parse_args(argv)
    R.run_tta_job(args, lora_method(args))


if __name__ == "__main__":
    main()

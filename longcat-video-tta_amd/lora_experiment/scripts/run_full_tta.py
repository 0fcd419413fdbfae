#!/usr/bin/env python3
"""Full-model TTA runner on MI355X — same relative path, CLI flags and artifact schemas as the reference's
`lora_experiment/scripts/run_full_tta.py` (flags :337-376 + shared groups; `config.json` :466-510, `checkpoint.json`,
`summary.json` :864-905).  All DiT parameters are unfrozen (:452-453), block checkpointing is switched on (:444-449), the
base weights are snapshotted once and restored before every video (:462, :222-228 — on the device here), the inner loop is
`tta.full_tta.finetune_full_on_conditioning` (SGD by default, `--optimizer adamw` optional), generation and scoring are
the LoRA runner's.  One process per GPU under torch.distributed.run shards the videos (no collective on the path).
"""
import argparse
import functools
import sys
from pathlib import Path

_PKG = Path(__file__).resolve().parents[2]
if str(_PKG) not in sys.path:
    sys.path.insert(0, str(_PKG))

import torch  # noqa: E402
from torch.utils.checkpoint import checkpoint  # noqa: E402

from tta import cli_args as C  # noqa: E402
from tta import runner_common as R  # noqa: E402
from tta.full_tta import finetune_full_on_conditioning, reset_dit_weights, snapshot_base_state  # noqa: E402


def build_parser():
    p = argparse.ArgumentParser(description="Full-model TTA for LongCat-Video (MI355X)")
    R.add_common_args(p)
    p.add_argument("--restart", action="store_true")
    p.add_argument("--learning-rate", type=float, default=1e-5)
    p.add_argument("--num-steps", type=int, default=10)
    p.add_argument("--warmup-steps", type=int, default=2)
    p.add_argument("--weight-decay", type=float, default=0.01)
    p.add_argument("--max-grad-norm", type=float, default=1.0)
    p.add_argument("--optimizer", type=str, default="sgd", choices=["sgd", "adamw"])
    C.add_optimizer_args(p, decay_to_base=True, master_weights_help="fp32 master weights: +2 B / parameter of low words, fp32 "
                                                                    "moments under adamw (include/lcv_hip_master.h)")
    p.add_argument("--batch-videos", type=int, default=1)
    p.add_argument("--batch-method", type=str, default="similarity", choices=["similarity", "sequential"])
    p.add_argument("--retrieval-pool-dir", type=str, default=None)
    R.add_shared_groups(p, clip_gate=True)
    return p


def parse_args(argv=None):
    return C.parse_with_step_cache(build_parser(), argv, C.parse_optimizer_args)


def full_method(args) -> R.TTAMethod:
    """The full-model job as `R.run_tta_job` takes it: every parameter trainable, checkpointing forced on, the base weights
    snapshotted once and put back before every video is loaded, `config.json` in the reference's layout."""
    job = {}                                                   # base_state and total_params, once the model is loaded

    def prepare(dit):
        dit.gradient_checkpointing = True                                                   # :444-449
        dit._gradient_checkpointing_func = functools.partial(checkpoint, use_reentrant=False)
        for p in dit.parameters():                                                          # :452-453
            p.requires_grad = True
        job["total_params"] = sum(p.numel() for p in dit.parameters())
        trainable_params = sum(p.numel() for p in dit.parameters() if p.requires_grad)
        job["base_state"] = snapshot_base_state(dit)                                        # :462 (device-resident here)
        gate = R.clip_gate_summary(args)
        return {"method": "full_tta",
                "training": {"learning_rate": args.learning_rate, "num_steps": args.num_steps, "warmup_steps": args.warmup_steps,
                             "weight_decay": args.weight_decay, "max_grad_norm": args.max_grad_norm, "optimizer": args.optimizer,
                             "master_weights": args.master_weights, "adam_8bit": args.adam_8bit,
                             "grad_accum": args.grad_accum, **({"decay_to_base": True} if args.decay_to_base else {}),
                             **C.weight_ema_record(args), **C.stochastic_rounding_record(args), **C.max_drift_record(args),
                             **C.sam_record(args),
                             "total_params": job["total_params"], "trainable_params": trainable_params},
                "generation": {"num_cond_frames": args.num_cond_frames, "num_frames": args.num_frames,
                               "num_inference_steps": args.num_inference_steps, "guidance_scale": args.guidance_scale,
                               "resolution": args.resolution, **C.step_cache_record(args),
                               **C.solver_record(args), **C.cfg_reuse_record(args),
                               **C.apg_record(args)},
                "seed": args.seed, "max_videos": args.max_videos,
                **{k: v for k, v in gate.items() if k != "clip_gate_stats"},
                "clip_gate": {"enabled": args.clip_gate_enabled, "threshold": args.clip_gate_threshold,
                              "backend": args.clip_gate_backend, "model": args.clip_gate_model,
                              "sample_frames": args.clip_gate_sample_frames, "aggregation": args.clip_gate_aggregation,
                              "sampling_mode": gate["clip_gate_sampling_mode"], "late_fraction": args.clip_gate_late_fraction,
                              "log_only": args.clip_gate_log_only, "fail_open": args.clip_gate_fail_open}}

    def adapt(dit, cond, train, pe, pm, device, es, variants):                              # the stopper snapshots the model itself
        return finetune_full_on_conditioning(dit, cond, train, pe, pm, num_steps=args.num_steps, lr=args.learning_rate,
                                             warmup_steps=args.warmup_steps, weight_decay=args.weight_decay,
                                             max_grad_norm=args.max_grad_norm, device=device, dtype=torch.bfloat16,
                                             early_stopper=es, optimizer_type=args.optimizer, train_latents_variants=variants,
                                             # the anchors are the reset's base copy: nothing more is allocated
                                             **({"base_state": job["base_state"]} if args.decay_to_base or args.max_drift is not None
                                                else {}),
                                             **C.optimizer_kwargs(args))

    def row_extra(tr, variants, blob):
        return {"num_train_steps": len(tr["losses"]), **({"drift_norm": tr["drift_norm"]} if args.decay_to_base else {}),
                **C.stochastic_rounding_record(args), **C.max_drift_result(tr), **C.sam_result(tr)}

    def summary_extra(merged, ok):
        return {"learning_rate": args.learning_rate, "num_steps": args.num_steps, "batch_videos": args.batch_videos,
                "retrieval_pool_dir": args.retrieval_pool_dir, "total_params": job["total_params"],
                **R.failed_and_final_loss(merged, ok), **R.clip_gate_summary(args)}

    return R.TTAMethod(name="full_tta", label="Full TTA", file_suffix="full", prepare=prepare, adapt=adapt,
                       before_load=lambda dit: reset_dit_weights(dit, job["base_state"]),     # :640 per-video reset
                       choose_checkpointing=False, row_extra=row_extra, summary_extra=summary_extra)


def main(argv=None):
    args = parse_args(argv)
    R.run_tta_job(args, full_method(args))


if __name__ == "__main__":
    main()

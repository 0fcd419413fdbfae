"""argparse groups shared by the TTA runners — flag names and defaults of the reference
(delta_experiment/scripts/common.py:1404-1485, 1601-1706, 2438-2450; early_stopping.py:33-51), so
`sweep_experiment/sbatch/run_sweep.sbatch` can pass its flag set unchanged.  Flags of subsystems outside the hot path
(CLIP gate, caption guard, online FVD) are parsed and recorded; enabling one raises a clear error.  Augmentation is built
(tta/augment.py: the variants' pre-encode is row (f)1 of SURVEY §8)."""
import argparse
from typing import Any, Dict, List

from .latent_split import estimate_tta_split_budget


def add_tta_frame_args(parser):
    g = parser.add_argument_group("TTA frame split")
    g.add_argument("--tta-total-frames", type=int, default=None)
    g.add_argument("--tta-context-frames", type=int, default=None)
    return parser


def add_augmentation_args(parser):
    g = parser.add_argument_group("Augmentation")
    g.add_argument("--aug-enabled", action="store_true", default=False)
    g.add_argument("--aug-flip", action="store_true", default=False)
    g.add_argument("--aug-rotate-deg", type=float, default=10.0)
    g.add_argument("--aug-rotate-random-min", type=float, default=5.0)
    g.add_argument("--aug-rotate-random-max", type=float, default=15.0)
    g.add_argument("--aug-rotate-random-count", type=int, default=2)
    g.add_argument("--aug-rotate-random-step", type=float, default=1.0)
    g.add_argument("--no-aug-rotate-zoom", action="store_false", dest="aug_rotate_zoom")      # common.py:1697-1703
    parser.set_defaults(aug_rotate_zoom=True)
    g.add_argument("--aug-speed-factors", type=str, default="")
    return parser


def add_caption_guard_args(parser):
    g = parser.add_argument_group("Caption guard")
    g.add_argument("--caption-guard-mode", type=str, default="fail", choices=["fail", "warn", "off"])
    g.add_argument("--caption-guard-min-nonempty-ratio", type=float, default=0.95)
    g.add_argument("--caption-guard-min-unique-ratio", type=float, default=0.10)
    g.add_argument("--caption-guard-max-top1-ratio", type=float, default=0.50)
    g.add_argument("--caption-guard-max-generic-top1-ratio", type=float, default=0.20)
    g.add_argument("--caption-guard-topk", type=int, default=5)
    return parser


def add_caption_override_args(parser):
    parser.add_argument_group("Caption override").add_argument("--fixed-caption", type=str, default=None)
    return parser


def add_feature_frame_guard_args(parser):
    parser.add_argument_group("Feature frame guard").add_argument(
        "--feature-frame-guard-mode", type=str, default="fail", choices=["fail", "warn", "off"])
    return parser


def add_online_eval_args(parser):
    g = parser.add_argument_group("Online evaluation")
    g.add_argument("--compute-fvd", action="store_true", default=False)
    g.add_argument("--compute-fid", action="store_true", default=False)
    g.add_argument("--compute-vbench", action="store_true", default=False)
    g.add_argument("--min-fvd-videos", type=int, default=256)
    return parser


def add_clip_gate_args(parser):
    g = parser.add_argument_group("CLIP gate")
    g.add_argument("--clip-gate-enabled", action="store_true", default=False)
    g.add_argument("--clip-gate-threshold", type=float, default=0.0)
    g.add_argument("--clip-gate-backend", type=str, default="clip", choices=["clip", "xclip"])
    g.add_argument("--clip-gate-model", type=str, default=None)
    g.add_argument("--clip-gate-sample-frames", type=int, default=4)
    g.add_argument("--clip-gate-aggregation", type=str, default="mean", choices=["mean", "min", "max"])
    g.add_argument("--clip-gate-sampling-mode", type=str, default="full_window", choices=["full_window", "late_only"])
    g.add_argument("--clip-gate-late-fraction", type=float, default=0.4)
    g.add_argument("--clip-gate-late-only", action="store_true", default=False)
    g.add_argument("--clip-gate-fail-open", dest="clip_gate_fail_open", action="store_true", default=True)
    g.add_argument("--clip-gate-fail-closed", dest="clip_gate_fail_open", action="store_false")
    g.add_argument("--clip-gate-log-only", action="store_true", default=False)
    return parser


def add_optimizer_args(parser, *, master_weights_help, decay_to_base=False):
    """The optimizer options of the adapting runners; `--master-weights` with the runner's own help wording, `--decay-to-base`
    only for the runners whose loop takes it."""
    parser.add_argument("--master-weights", action="store_true", help=master_weights_help)
    parser.add_argument("--adam-8bit", action="store_true",
                        help="with --master-weights: AdamW moments in 1 B each plus block scales, about 2.016 B / parameter "
                             "instead of 8 (include/lcv_hip_moments8.h)")
    parser.add_argument("--grad-accum", type=int, default=1, metavar="N",
                        help="with --master-weights: every optimizer step is the mean of N micro-steps (own sigma, noise and "
                             "variant draw each), summed in fp32 accumulators, +4 B / parameter (include/lcv_hip_accum.h)")
    if decay_to_base:
        parser.add_argument("--decay-to-base", action="store_true",
                            help="with --master-weights: the weight decay pulls toward the base weights instead of toward zero, and "
                                 "every result row carries drift_norm, the distance from them (include/lcv_hip_anchor.h)")
    parser.add_argument("--weight-ema", type=float, default=None, metavar="BETA",
                        help="with --master-weights: keep an fp32 exponential moving average of the weights over the optimizer "
                             "steps (e = BETA * e + (1 - BETA) * w, +4 B / parameter, include/lcv_hip_ema.h); the early stopper "
                             "scores the average and generation (and --save-lora-weights, which then writes the averaged "
                             "adapters) reads it")
    parser.add_argument("--weight-ema-warmup", action="store_true",
                        help="with --weight-ema: BETA_t = min(BETA, (1 + t) / (10 + t)) at the t-th step, so an average that starts "
                             "at the base weights does not lag a short run")
    parser.add_argument("--stochastic-rounding", action="store_true",
                        help="without --master-weights: the optimizer step runs in fp32 and every bf16 value it stores (weights, "
                             "AdamW moments) is rounded up or down at random, unbiased, so updates below half a bf16 ulp and the "
                             "decay of the second moment survive in expectation; no extra state (include/lcv_hip_sr.h); the "
                             "rounding bits follow --seed")


def parse_optimizer_args(parser, argv=None):
    """parse_args, then the refusals of the optimizer options as the parser's own one-line errors (exit status 2), in this
    order: --adam-8bit, --grad-accum, --decay-to-base, --weight-ema, --stochastic-rounding.  `--optimizer`, `--also-tune-delta`
    and `--decay-to-base` count as adamw, off and off for a parser without them."""
    args = parser.parse_args(argv)
    master, accum, tune_delta = args.master_weights, args.grad_accum, getattr(args, "also_tune_delta", False)
    refusals = [
        (args.adam_8bit and not master,
         "--adam-8bit needs --master-weights (the 8-bit moments exist for the master-weight AdamW step only)"),
        (args.adam_8bit and getattr(args, "optimizer", "adamw") != "adamw",
         "--adam-8bit needs --optimizer adamw (SGD keeps no moments)"),
        (accum < 1, f"--grad-accum must be at least 1, got {accum}"),
        (accum > 1 and not master,
         "--grad-accum above 1 needs --master-weights (the fp32-gradient steps exist for the master-weight form only)"),
        (accum > 1 and args.adam_8bit,
         "--grad-accum above 1 cannot be combined with --adam-8bit (the 8-bit-moment step reads bf16 gradients)"),
        (accum > 1 and tune_delta,
         "--grad-accum above 1 cannot be combined with --also-tune-delta (the fp32 delta vector has no accumulators)"),
        (getattr(args, "decay_to_base", False) and not master,
         "--decay-to-base needs --master-weights (a pull of lr * wd * (w - w0) is far below half a bf16 ulp; the "
         "anchor steps exist for the master-weight form only)"),
        (args.weight_ema_warmup and args.weight_ema is None, "--weight-ema-warmup needs --weight-ema BETA"),
    ]
    if args.weight_ema is not None:
        refusals += [
            (not master,
             "--weight-ema needs --master-weights (an increment (1 - BETA) * (w - e) is far below half a bf16 ulp; the "
             "average is kept in fp32 beside the master weights only)"),
            (not 0.0 <= args.weight_ema < 1.0,         # a NaN fails both
             f"--weight-ema BETA must be in [0, 1), got {args.weight_ema}"),
            (tune_delta,
             "--weight-ema cannot be combined with --also-tune-delta (the fp32 delta vector has no master-weight form "
             "to average beside)"),
        ]
    if args.stochastic_rounding:
        refusals += [
            (master,
             "--stochastic-rounding cannot be combined with --master-weights (the master weights are already exact)"),
            (tune_delta,
             "--stochastic-rounding cannot be combined with --also-tune-delta (the fp32 delta vector has nothing to round, "
             "and a joint run would mix the two forms)"),
        ]
    for refused, message in refusals:
        if refused:
            parser.error(message)
    return args


def optimizer_kwargs(args) -> dict:
    """The loop functions' keywords for the optimizer options; a flag the parser does not have contributes nothing."""
    kw = {"master_weights": args.master_weights, "moments_8bit": args.adam_8bit, "grad_accum": args.grad_accum}
    if hasattr(args, "decay_to_base"):
        kw["decay_to_base"] = args.decay_to_base
    return {**kw, **weight_ema_kwargs(args), **stochastic_rounding_record(args), **max_drift_kwargs(args),
            **sam_kwargs(args)}


def weight_ema_kwargs(args) -> dict:
    """The loop functions' keywords for --weight-ema; nothing when the flag is absent."""
    return {} if args.weight_ema is None else {"weight_ema": args.weight_ema, "ema_warmup": args.weight_ema_warmup}


def weight_ema_record(args) -> dict:
    """What config.json (`training`) and the norm-tuning summary.json record of --weight-ema; nothing when the flag is absent."""
    return {} if args.weight_ema is None else {"weight_ema": args.weight_ema, "weight_ema_warmup": args.weight_ema_warmup}


def stochastic_rounding_record(args) -> dict:
    """`stochastic_rounding: true` for config.json (`training`), the norm-tuning summary.json, every result row and the loop
    functions' keywords; nothing when the flag is absent."""
    return {"stochastic_rounding": True} if getattr(args, "stochastic_rounding", False) else {}


def _step_cache_threshold(text: str) -> float:
    try:
        v = float(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"not a number: {text!r}")
    if not v >= 0.0:                             # a NaN fails too
        raise argparse.ArgumentTypeError(f"THRESH must be >= 0 and not NaN, got {text}")
    return v


def _step_cache_max_skip(text: str) -> int:
    try:
        v = int(text)
    except ValueError:
        raise argparse.ArgumentTypeError(f"not an integer: {text!r}")
    if v < 1:
        raise argparse.ArgumentTypeError(f"K must be >= 1, got {text}")
    return v


def add_step_cache_args(parser):
    parser.add_argument("--step-cache", type=_step_cache_threshold, default=None, metavar="THRESH",
                        help="first-block step cache of the denoise loop (include/lcv_hip_stepcache.h): a step whose block-0 "
                             "residual is within THRESH (relative L1) of the last computed step's adds that step's cached "
                             "residual of the remaining blocks instead of running them; the first and the last step are always "
                             "computed; 0 computes every step and records the distance trace (calibration); no default is "
                             "recommended")
    parser.add_argument("--step-cache-max-skip", type=_step_cache_max_skip, default=None, metavar="K",
                        help="with --step-cache: compute a step after K skipped steps in a row (default: no cap)")


def parse_with_step_cache(parser, argv=None, parse=None):
    """`parse` (default parser.parse_args), then the refusal of --step-cache-max-skip without --step-cache as the parser's own
    one-line error (exit status 2); a negative or NaN THRESH and K < 1 are refused by the arguments' types the same way."""
    args = parse(parser, argv) if parse is not None else parser.parse_args(argv)
    if args.step_cache_max_skip is not None and args.step_cache is None:
        parser.error("--step-cache-max-skip needs --step-cache THRESH")
    check_cfg_reuse_args(parser, args)
    check_apg_args(parser, args)
    check_max_drift_args(parser, args)
    check_sam_args(parser, args)
    return args


def step_cache_from_args(args):
    """A fresh `StepCache` for one continuation, or None when the flag is absent (then nothing is imported or allocated)."""
    thr = getattr(args, "step_cache", None)
    if thr is None:
        return None
    from longcat_video.step_cache import StepCache
    return StepCache(thr, max_consecutive=getattr(args, "step_cache_max_skip", None))


def step_cache_record(args) -> dict:
    """What config.json (`generation`) and the flat summary.json of the runners without one record of --step-cache; nothing
    when the flag is absent."""
    if getattr(args, "step_cache", None) is None:
        return {}
    return {"step_cache": args.step_cache, "step_cache_max_skip": args.step_cache_max_skip}


def step_cache_result(blob) -> dict:
    """The per-video `step_cache` entry (`StepCache.stats()`, left in the blob by generate_continuation); nothing without the
    flag."""
    return {"step_cache": blob["_step_cache"]} if "_step_cache" in blob else {}


def add_solver_arg(parser):
    from longcat_video.solver import SOLVERS       # the one list of rules (pure host code: no GPU, no torch)
    parser.add_argument("--solver", choices=SOLVERS, default="euler",
                        help="the rule of the denoise loop's update (include/lcv_hip_solver.h, longcat_video/solver.py): euler is "
                             "the explicit Euler step (first order); ab2 is the two-step Adams-Bashforth rule and ab2c its "
                             "predictor-corrector form, both second order over the velocities the loop has already computed "
                             "(no further forward; one latent-sized fp32 buffer per kept velocity); no step count is recommended")


def solver_from_args(args):
    """The `solver=` keyword of the denoise loop, or None for euler or an absent flag (then the call is the plain one)."""
    kind = getattr(args, "solver", None)
    return None if kind in (None, "euler") else kind


def solver_record(args) -> dict:
    """What config.json (`generation`) and the flat summary.json of the runners without one record of --solver; nothing for
    euler."""
    kind = solver_from_args(args)
    return {} if kind is None else {"solver": kind}


def _cfg_reuse_int(name: str, least: int):
    def convert(text: str) -> int:
        try:
            v = int(text)
        except ValueError:
            raise argparse.ArgumentTypeError(f"not an integer: {text!r}")
        if v < least:
            raise argparse.ArgumentTypeError(f"{name} must be >= {least}, got {text}")
        return v
    return convert


def add_cfg_reuse_args(parser):
    parser.add_argument("--cfg-reuse", type=_cfg_reuse_int("K", 1), default=None, metavar="K",
                        help="guidance reuse of the CFG denoise loop (include/lcv_hip_cfgreuse.h, longcat_video/cfg_reuse.py): "
                             "every K-th step, the first and the last run both rows and store the guidance correction; the "
                             "steps between run the prompt row alone at batch 1 and add the stored correction back; 1 runs "
                             "every step in full and records the drift trace (calibration); no interval is recommended")
    parser.add_argument("--cfg-reuse-warmup", type=_cfg_reuse_int("W", 0), default=None, metavar="W",
                        help="with --cfg-reuse: the first W steps run in full (default 0)")


def check_cfg_reuse_args(parser, args) -> None:
    """The refusals of --cfg-reuse as the parser's own one-line error (exit status 2); K < 1 and W < 0 are refused by the
    arguments' types the same way.  Called from `parse_with_step_cache`, which every runner parses through."""
    if getattr(args, "cfg_reuse_warmup", None) is not None and getattr(args, "cfg_reuse", None) is None:
        parser.error("--cfg-reuse-warmup needs --cfg-reuse K")
    if getattr(args, "cfg_reuse", None) is None:
        return
    if getattr(args, "step_cache", None) is not None:
        parser.error("--cfg-reuse cannot be combined with --step-cache (the cache's buffers are per batch shape)")
    if not args.guidance_scale > 1.0:
        parser.error(f"--cfg-reuse needs guidance: --guidance-scale must be > 1, got {args.guidance_scale}")


def cfg_reuse_from_args(args):
    """A fresh `GuidanceReuse` for one continuation, or None when the flag is absent (then nothing is imported or allocated)."""
    K = getattr(args, "cfg_reuse", None)
    if K is None:
        return None
    from longcat_video.cfg_reuse import GuidanceReuse
    return GuidanceReuse(K, warmup=getattr(args, "cfg_reuse_warmup", None) or 0)


def cfg_reuse_record(args) -> dict:
    """What config.json (`generation`) and the flat summary.json of the runners without one record of --cfg-reuse; nothing
    when the flag is absent."""
    if getattr(args, "cfg_reuse", None) is None:
        return {}
    return {"cfg_reuse": args.cfg_reuse, "cfg_reuse_warmup": getattr(args, "cfg_reuse_warmup", None) or 0}


def cfg_reuse_result(blob) -> dict:
    """The per-video `cfg_reuse` entry (`GuidanceReuse.stats()`, left in the blob by generate_continuation); nothing without the
    flag."""
    return {"cfg_reuse": blob["_cfg_reuse"]} if "_cfg_reuse" in blob else {}


class _ApgValue(argparse.Action):
    """Stores the value and notes on the namespace that the flag was given, so that a value equal to the default is still refused
    without --apg."""

    def __call__(self, parser, namespace, values, option_string=None):
        setattr(namespace, self.dest, values)
        namespace.apg_flags_given = getattr(namespace, "apg_flags_given", ()) + (option_string,)


def add_apg_args(parser):
    parser.add_argument("--apg", action="store_true",
                        help="adaptive projected guidance of the CFG denoise loop (include/lcv_hip_apg.h, longcat_video/apg.py): "
                             "the guidance correction is split into its part along the prompt row's output, which inflates the "
                             "magnitude at a large --guidance-scale, and the part orthogonal to it; no further forward pass; no "
                             "setting is recommended")
    parser.add_argument("--apg-eta", type=float, default=0.0, metavar="ETA", action=_ApgValue,
                        help="with --apg: the weight of the parallel part (default 0.0: dropped; 1 with no threshold and no "
                             "momentum is plain guidance in value)")
    parser.add_argument("--apg-norm-threshold", type=float, default=None, metavar="R", action=_ApgValue,
                        help="with --apg: cap the correction's norm at R per element (RMS), so one value serves every resolution "
                             "(default: no cap)")
    parser.add_argument("--apg-momentum", type=float, default=0.0, metavar="BETA", action=_ApgValue,
                        help="with --apg: add BETA times the previous step's correction, BETA in (-1, 1); a negative value damps "
                             "what the last steps already pushed (default 0.0)")


def check_apg_args(parser, args) -> None:
    """The refusals of --apg as the parser's own one-line error (exit status 2).  Called from `parse_with_step_cache`, which
    every runner parses through."""
    import math
    if not getattr(args, "apg", False):
        for flag in getattr(args, "apg_flags_given", ()):
            parser.error(f"{flag} needs --apg")
        return
    eta, thr, beta = args.apg_eta, args.apg_norm_threshold, args.apg_momentum
    if getattr(args, "cfg_reuse", None) is not None:
        parser.error("--apg cannot be combined with --cfg-reuse (the stored correction is the plain rule's)")
    if not args.guidance_scale > 1.0:
        parser.error(f"--apg needs guidance: --guidance-scale must be > 1, got {args.guidance_scale}")
    if not math.isfinite(eta):
        parser.error(f"--apg-eta ETA must be a finite number, got {eta}")
    if thr is not None and not (thr > 0.0 and math.isfinite(thr)):        # a NaN fails too
        parser.error(f"--apg-norm-threshold R must be a finite number > 0, got {thr}")
    if not -1.0 < beta < 1.0:                                               # likewise
        parser.error(f"--apg-momentum BETA must be in (-1, 1), got {beta}")


def apg_from_args(args):
    """A fresh `ProjectedGuidance` for one continuation, or None when the flag is absent (then nothing is imported or
    allocated)."""
    if not getattr(args, "apg", False):
        return None
    from longcat_video.apg import ProjectedGuidance
    return ProjectedGuidance(eta=args.apg_eta, norm_threshold=args.apg_norm_threshold, momentum=args.apg_momentum)


def apg_record(args) -> dict:
    """What config.json (`generation`) and the flat summary.json of the runners without one record of --apg; nothing when the
    flag is absent."""
    if not getattr(args, "apg", False):
        return {}
    return {"apg": True, "apg_eta": args.apg_eta, "apg_norm_threshold": args.apg_norm_threshold,
            "apg_momentum": args.apg_momentum}


def apg_result(blob) -> dict:
    """The per-video `apg` entry (`ProjectedGuidance.stats()`, left in the blob by generate_continuation); nothing without the
    flag."""
    return {"apg": blob["_apg"]} if "_apg" in blob else {}


def add_max_drift_args(parser):
    parser.add_argument("--max-drift", type=float, default=None, metavar="R",
                        help="trust-region cap on how far the adapted parameters travel (include/lcv_hip_trust.h): after every "
                             "optimizer step, if the drift from the values the video's adaptation started at exceeds R (RMS per "
                             "trained element, so one value serves 512 parameters and 13.6 G), it is scaled back onto that ball, "
                             "on the device; bf16 parameters need --master-weights; inf changes nothing and records the drift "
                             "trace (calibration); no radius is recommended")
    parser.add_argument("--max-drift-scope", choices=["global", "tensor"], default=None,
                        help="with --max-drift: one ball over all trained elements (global, the default) or one per parameter "
                             "tensor, so that no layer can spend the whole budget (tensor)")


def check_max_drift_args(parser, args) -> None:
    """The refusals of --max-drift as the parser's own one-line error (exit status 2).  Called from `parse_with_step_cache`,
    which every runner parses through; a parser without the flags is left alone."""
    radius = getattr(args, "max_drift", None)
    if radius is None:
        if getattr(args, "max_drift_scope", None) is not None:
            parser.error("--max-drift-scope needs --max-drift R")
        return
    if not radius > 0.0:                                                  # a NaN fails too
        parser.error(f"--max-drift R must be > 0 (inf is allowed), got {radius}")
    if getattr(args, "stochastic_rounding", False):
        parser.error("--max-drift cannot be combined with --stochastic-rounding (the ball needs --master-weights: a contraction "
                     "below half a bf16 ulp rounds back to the same word)")
    if getattr(args, "lora_dora", False):
        parser.error("--max-drift cannot be combined with --lora-dora (its bf16 adapters train without --master-weights)")
    if hasattr(args, "master_weights") and not args.master_weights:       # the runners that train bf16 parameters
        parser.error("--max-drift needs --master-weights (a contraction (1 - c) * |d| below half a bf16 ulp rounds back to the "
                     "same word, so the bound would not hold for plain bf16 parameters)")


def max_drift_kwargs(args) -> dict:
    """The loop functions' keywords for --max-drift; nothing when the flag is absent (then nothing is imported, allocated or
    launched)."""
    if getattr(args, "max_drift", None) is None:
        return {}
    return {"max_drift": args.max_drift, "max_drift_scope": args.max_drift_scope or "global"}


def max_drift_record(args) -> dict:
    """What config.json (`training`) and the flat summary.json of the runners without one record of --max-drift; nothing when
    the flag is absent."""
    return max_drift_kwargs(args)


def max_drift_result(loop) -> dict:
    """The per-video `drift_norm` and `max_drift` entry ({radius, scope, steps, projections, first_projected_step, min_coef,
    drift_rms_trace}) the loop left in its result; nothing without the flag."""
    return {"drift_norm": loop["drift_norm"], "max_drift": loop["max_drift"]} if "max_drift" in loop else {}


def add_sam_args(parser):
    parser.add_argument("--sam-rho", type=float, default=None, metavar="RHO",
                        help="sharpness-aware adaptation steps (SAM, include/lcv_hip_sam.h): every optimizer step takes its "
                             "gradient at w + RHO * g / |g|, one norm over all trained parameters, on the device; two "
                             "forward/backward passes per step under the same noise, sigma, variant and dropout draws; 0 runs "
                             "both passes, changes no bit of the run and records the gradient-norm trace (calibration); not with "
                             "--grad-accum above 1 or --lora-dora; no rho is recommended")
    parser.add_argument("--sam-adaptive", action="store_true",
                        help="with --sam-rho: the adaptive form (ASAM), the perturbation of an element scaled by (|w| + ETA)^2 "
                             "and RHO measured in the (|w| + ETA)-scaled norm")
    parser.add_argument("--sam-eta", type=float, default=None, metavar="ETA",
                        help="with --sam-adaptive: the ETA of |w| + ETA (default 0.01)")


SAM_ETA_DEFAULT = 0.01


def check_sam_args(parser, args) -> None:
    """The refusals of --sam-rho as the parser's own one-line error (exit status 2).  Called from `parse_with_step_cache`, which
    every runner parses through; a parser without the flags is left alone."""
    rho, eta = getattr(args, "sam_rho", None), getattr(args, "sam_eta", None)
    adaptive = getattr(args, "sam_adaptive", False)
    if rho is None:
        if adaptive:
            parser.error("--sam-adaptive needs --sam-rho RHO")
        if eta is not None:
            parser.error("--sam-eta needs --sam-rho RHO")
        return
    if not 0.0 <= rho < float("inf"):                                     # a NaN fails too
        parser.error(f"--sam-rho RHO must be finite and >= 0, got {rho}")
    if eta is not None and not adaptive:
        parser.error("--sam-eta needs --sam-adaptive")
    if eta is not None and not 0.0 <= eta < float("inf"):
        parser.error(f"--sam-eta ETA must be finite and >= 0, got {eta}")
    if getattr(args, "grad_accum", 1) > 1:
        parser.error("--sam-rho cannot be combined with --grad-accum above 1 (a perturbation per micro-step is a different "
                     "algorithm)")
    if getattr(args, "lora_dora", False):
        parser.error("--sam-rho cannot be combined with --lora-dora (the row norm is held constant in the backward and the "
                     "forward caches it)")


def sam_kwargs(args) -> dict:
    """The loop functions' keywords for --sam-rho; nothing when the flag is absent (then nothing is imported, allocated or
    launched)."""
    if getattr(args, "sam_rho", None) is None:
        return {}
    eta = args.sam_eta if args.sam_eta is not None else SAM_ETA_DEFAULT
    return {"sam_rho": args.sam_rho, "sam_adaptive": bool(args.sam_adaptive), "sam_eta": eta}


def sam_record(args) -> dict:
    """What config.json (`training`) and the flat summary.json of the runners without one record of --sam-rho; nothing when the
    flag is absent."""
    return sam_kwargs(args)


def sam_result(loop) -> dict:
    """The per-video `sam` entry ({rho, adaptive, eta, steps, grad_norm_trace, realized_norm_trace, perturbed_loss_trace}) the
    loop left in its result; nothing without the flag."""
    return {"sam": loop["sam"]} if "sam" in loop else {}


def normalize_tta_frame_args(args):
    """Post-parse normalisation of lora_experiment/scripts/run_lora_tta.py:743-758 (GT-leak clamp included)."""
    if args.tta_total_frames is None:
        args.tta_total_frames = args.num_cond_frames
    if args.tta_context_frames is None or args.tta_context_frames > args.tta_total_frames:
        args.tta_context_frames = args.num_cond_frames
    if args.tta_total_frames > args.gen_start_frame:
        print(f"[WARN] tta_total_frames ({args.tta_total_frames}) exceeds gen_start_frame ({args.gen_start_frame}); "
              "clamping to avoid GT leakage.")
        args.tta_total_frames = args.gen_start_frame
    if args.tta_context_frames > args.tta_total_frames:
        args.tta_context_frames = args.tta_total_frames
    return args


def validate_tta_feature_budget(args, context: str = "") -> Dict[str, Any]:
    """ES needs at least one held-out latent (common.py:1533-1598); CLIP-gate budget is not checked (gate out of scope)."""
    mode = str(getattr(args, "feature_frame_guard_mode", "fail")).lower()
    if mode not in {"fail", "warn", "off"}:
        mode = "fail"
    prefix = f"[feature_budget:{context}]" if context else "[feature_budget]"
    tta_total = int(getattr(args, "tta_total_frames", 0) or 0)
    tta_context = int(getattr(args, "tta_context_frames", 0) or 0)
    holdout = float(getattr(args, "es_holdout_fraction", 0.25) or 0.25)
    split = estimate_tta_split_budget(tta_total, tta_context, holdout_fraction=holdout)
    issues: List[str] = []
    if not bool(getattr(args, "es_disable", False)) and split["val_latents"] < 1:
        issues.append("ES is enabled but estimated val_latents=0 "
                      f"(tta_total_frames={tta_total}, tta_context_frames={tta_context}, holdout={holdout}). "
                      "Increase tta_total_frames and/or reduce tta_context_frames.")
    if mode != "off":
        print(f"{prefix} split(total={split['total_latents']}, cond={split['cond_latents']}, "
              f"train={split['train_latents']}, val={split['val_latents']})")
    if issues:
        msg = f"{prefix} " + " | ".join(issues)
        if mode == "warn":
            print(f"WARNING: {msg}")
        elif mode == "fail":
            raise RuntimeError(msg)
    return {"split_budget": split}


def reject_out_of_scope(args):
    """Subsystems outside the hot path are parsed for CLI compatibility but cannot be switched on here."""
    if getattr(args, "clip_gate_enabled", False):
        raise NotImplementedError("the CLIP gate is outside the denoise-and-adapt hot path (SURVEY §2 #15)")
    if any(getattr(args, k, False) for k in ("compute_fvd", "compute_fid", "compute_vbench")):
        raise NotImplementedError("online FVD/FID/VBench evaluation is outside the hot path (SURVEY §2 #17)")

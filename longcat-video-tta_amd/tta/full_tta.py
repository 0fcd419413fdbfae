"""Full-model TTA (`METHOD=full`): every DiT parameter is trained on the video's conditioning clip.

Contract kept from the reference (lora_experiment/scripts/run_full_tta.py:95-306, 444-462): the public
names `finetune_full_on_conditioning`, `finetune_full_batch`, `reset_dit_weights`, their arguments and defaults
(`optimizer_type` "sgd" = plain SGD with weight decay, momentum 0; "adamw" = AdamW(0.9, 0.999, eps 1e-8)), and the four
returned keys.  The loop itself is `inner_loop.run_adaptation` — the same engine the LoRA and delta methods use — with
  * the fused multi-tensor optimizers (`FusedSGDClip` / `FusedAdamWClip`: a norm launch and an update launch over the
    ~700 parameter tensors, torch's foreach rounding points);
  * the base copy for the per-video reset living in HBM (`snapshot_base_state`): the reference parks it in host memory
    because an 80-141 GB card cannot hold a second model (:459-462); 288 GB can, so the reset is one device-side
    multi-tensor copy;
  * the early stopper's best state held in one reusable 27 GB buffer set instead of a fresh state-dict clone per
    improvement, and the 27 GB of gradients released before the continuation starts.
Dense-weight gradients come from `lcv_transpose_pad` + the NT GEMM over the token axis (lcv_hip/autograd_ops.py).
"""
from typing import Dict, List, Optional

import torch
import torch.nn as nn

from lcv_hip.ops import FusedAdamWClip, FusedSGDClip

from .early_stopping import AnchoredEarlyStopper
from .inner_loop import (_OneVideo, _RoundRobin, _fm_loss, _single_optimizer_step, max_drift_hook, refuse_sam,
                         refuse_stochastic_rounding_under_sp, run_adaptation, sam_hook)


def snapshot_base_state(dit: nn.Module) -> Dict[str, torch.Tensor]:
    """Device-resident copy of every state-dict entry, taken once per job."""
    return {name: t.detach().clone() for name, t in dit.state_dict().items()}


def reset_dit_weights(dit: nn.Module, base_state: Dict[str, torch.Tensor]) -> None:
    """Per-video reset (run_full_tta.py:222-228): base values back into every named parameter, gradients dropped."""
    dst, src = [], []
    for name, p in dit.named_parameters():
        p.grad = None
        if name in base_state:
            dst.append(p.detach())
            src.append(base_state[name].to(p.device))
    if dst:
        with torch.no_grad():
            torch._foreach_copy_(dst, src)


def _trainable(dit: nn.Module) -> List[torch.Tensor]:
    params = [p for p in dit.parameters() if p.requires_grad]
    if not params:
        raise ValueError("nothing to train: unfreeze the DiT (requires_grad) before full-model TTA")
    return params


def _make_optimizer(kind: str, params, lr: float, weight_decay: float, master_weights: bool = False,
                    moments_8bit: bool = False, grad_accum: int = 1, anchor=None):
    if kind == "adamw":
        return FusedAdamWClip(params, lr=lr, betas=(0.9, 0.999), weight_decay=weight_decay, eps=1e-8,
                              master_weights=master_weights, moments_8bit=moments_8bit, grad_accum=grad_accum, anchor=anchor)
    if kind == "sgd":
        if moments_8bit:
            raise ValueError("moments_8bit is for optimizer_type 'adamw': SGD keeps no moments")
        return FusedSGDClip(params, lr=lr, weight_decay=weight_decay, master_weights=master_weights, grad_accum=grad_accum,
                            anchor=anchor)
    raise ValueError(f"unknown optimizer_type {kind!r} (sgd | adamw)")


def _make_sr_optimizer(kind: str, params, lr: float, weight_decay: float, **master_form):
    """`_make_optimizer` for `stochastic_rounding` (include/lcv_hip_sr.h): same hyper-parameters, the plain form's storage.
    `master_form` are `_make_optimizer`'s master-weight keywords, passed on so that the constructors refuse them by name."""
    if kind == "adamw":
        return FusedAdamWClip(params, lr=lr, betas=(0.9, 0.999), weight_decay=weight_decay, eps=1e-8, stochastic_rounding=True,
                              **master_form)
    if kind == "sgd":
        if master_form.pop("moments_8bit", False):
            raise ValueError("moments_8bit is for optimizer_type 'adamw': SGD keeps no moments")
        return FusedSGDClip(params, lr=lr, weight_decay=weight_decay, stochastic_rounding=True, **master_form)
    raise ValueError(f"unknown optimizer_type {kind!r} (sgd | adamw)")


def _anchors(dit: nn.Module, base_state: Optional[Dict[str, torch.Tensor]]) -> List[torch.Tensor]:
    """The base words of the trainable parameters, in `_trainable` order: the `base_state` entries matched by name (not
    copied), or bf16 clones of the parameters as they are now."""
    named = [(name, p) for name, p in dit.named_parameters() if p.requires_grad]
    if base_state is None:
        return [p.detach().clone() for _, p in named]
    missing = [name for name, _ in named if name not in base_state]
    if missing:
        raise ValueError(f"base_state lacks {len(missing)} trainable parameters, the first: {missing[0]!r}")
    return [base_state[name] for name, _ in named]


def _run(dit, feed, num_steps, lr, warmup_steps, weight_decay, max_grad_norm, device, dtype, early_stopper, optimizer_type,
         *, master_weights, moments_8bit, grad_accum, decay_to_base, base_state, weight_ema, ema_warmup,
         stochastic_rounding=False, max_drift=None, max_drift_scope="global", sam_rho=None, sam_adaptive=False, sam_eta=0.01):
    params = _trainable(dit)
    refuse_stochastic_rounding_under_sp(dit, stochastic_rounding)
    # `sam_rho`: every step is a sharpness-aware one (include/lcv_hip_sam.h): two forward/backward passes, +2 B / parameter of
    # saved words (27 GB for the whole model: a memory decision)
    refuse_sam(dit, sam_rho, grad_accum)
    # `decay_to_base`: the weight decay pulls toward the base words (include/lcv_hip_anchor.h), which are the caller's
    # `base_state` entries or, without one, +2 B / parameter of clones; a `base_state` alone only measures the drift
    # `max_drift`: after every step the weights are projected onto a ball of that RMS radius around the same base words
    # (include/lcv_hip_trust.h); with the per-video `base_state` nothing more is allocated
    want_drift = bool(decay_to_base) or base_state is not None or max_drift is not None
    anchor = _anchors(dit, base_state) if want_drift else None
    # made per call, so per video: the per-video reset writes the bf16 words, and the low words of `master_weights`
    # (+2 B / parameter; AdamW: +8 B of fp32 moments, or +2.016 B of 8-bit ones under `moments_8bit`) start at zero next to them;
    # `grad_accum` > 1 adds +4 B / parameter of fp32 accumulators (54 GB for the whole model: a memory decision)
    # `stochastic_rounding` allocates nothing: SGD stays at 0 B of state, AdamW at its two bf16 moments
    if stochastic_rounding:
        opt = _make_sr_optimizer(optimizer_type, params, lr, weight_decay, master_weights=master_weights,
                                 moments_8bit=moments_8bit, grad_accum=grad_accum, anchor=anchor if decay_to_base else None)
    else:
        opt = _make_optimizer(optimizer_type, params, lr, weight_decay, master_weights, moments_8bit, grad_accum,
                              anchor=anchor if decay_to_base else None)
    if weight_ema is not None:                 # +4 B / parameter of fp32 average (54 GB for the whole model: a memory decision);
        opt.enable_weight_ema(weight_ema, ema_warmup)   # run_adaptation scores it and leaves it in the parameters
    ball = max_drift_hook([opt], max_drift, max_drift_scope, num_steps, [anchor])
    out = run_adaptation(dit, params, [opt], _fm_loss(dit, feed, device, dtype), _single_optimizer_step(opt, max_grad_norm),
                         num_steps, lr, warmup_steps, early_stopper,
                         sam=sam_hook([opt], sam_rho, sam_adaptive, sam_eta, num_steps), after_step=ball, grad_accum=grad_accum)
    opt.zero_grad(set_to_none=True)            # the gradients of 13.6 B parameters are dead weight during generation
    if ball is not None:                       # |theta - theta0| from the ball's own fixed-order sum (lcv_trust_sumsq) and the
        ball.finish(out)                       # trace's summary: one pass, not a second one through lcv_master_drift_sumsq
    elif want_drift:                           # |theta - theta0| over the trainable parameters, read once per video (after the
        # final swap of a weight average: the drift of the weights that generate)
        out["drift_norm"] = float(opt.drift_norm(anchor).item())
    return out


def finetune_full_on_conditioning(dit: nn.Module, cond_latents: torch.Tensor, train_latents: torch.Tensor,
                                  prompt_embeds: torch.Tensor, prompt_mask: torch.Tensor, num_steps: int = 10,
                                  lr: float = 1e-5, warmup_steps: int = 2, weight_decay: float = 0.01,
                                  max_grad_norm: float = 1.0, device: str = "cuda", dtype: torch.dtype = torch.bfloat16,
                                  early_stopper: Optional[AnchoredEarlyStopper] = None,
                                  train_latents_variants: Optional[List[Dict]] = None, optimizer_type: str = "sgd",
                                  stochastic_rounding: bool = False, max_drift: Optional[float] = None,
                                  max_drift_scope: str = "global", sam_rho: Optional[float] = None,
                                  sam_adaptive: bool = False, sam_eta: float = 0.01,
                                  *, weight_ema: Optional[float] = None, ema_warmup: bool = False,
                                  decay_to_base: bool = False, base_state: Optional[Dict[str, torch.Tensor]] = None,
                                  grad_accum: int = 1, moments_8bit: bool = False, master_weights: bool = False) -> Dict:
    feed = _OneVideo(cond_latents, train_latents, prompt_embeds, prompt_mask, train_latents_variants)
    return _run(dit, feed, num_steps, lr, warmup_steps, weight_decay, max_grad_norm, device, dtype, early_stopper,
                optimizer_type, master_weights=master_weights, moments_8bit=moments_8bit, grad_accum=grad_accum,
                decay_to_base=decay_to_base, base_state=base_state, weight_ema=weight_ema, ema_warmup=ema_warmup,
                stochastic_rounding=stochastic_rounding, max_drift=max_drift, max_drift_scope=max_drift_scope,
                sam_rho=sam_rho, sam_adaptive=sam_adaptive, sam_eta=sam_eta)


def finetune_full_batch(dit: nn.Module, batch_data: List[Dict], num_steps: int = 10, lr: float = 1e-5, warmup_steps: int = 2,
                        weight_decay: float = 0.01, max_grad_norm: float = 1.0, device: str = "cuda",
                        dtype: torch.dtype = torch.bfloat16, optimizer_type: str = "sgd", stochastic_rounding: bool = False,
                        max_drift: Optional[float] = None, max_drift_scope: str = "global",
                        sam_rho: Optional[float] = None, sam_adaptive: bool = False, sam_eta: float = 0.01,
                        *, weight_ema: Optional[float] = None, ema_warmup: bool = False,
                        decay_to_base: bool = False, base_state: Optional[Dict[str, torch.Tensor]] = None,
                        grad_accum: int = 1, moments_8bit: bool = False, master_weights: bool = False) -> Dict:
    """Round-robin over the eval video and its retrieved neighbours (run_full_tta.py:230-306); no early stopping."""
    return _run(dit, _RoundRobin(batch_data, device), num_steps, lr, warmup_steps, weight_decay, max_grad_norm, device, dtype,
                None, optimizer_type, master_weights=master_weights, moments_8bit=moments_8bit, grad_accum=grad_accum,
                decay_to_base=decay_to_base, base_state=base_state, weight_ema=weight_ema, ema_warmup=ema_warmup,
                stochastic_rounding=stochastic_rounding, max_drift=max_drift, max_drift_scope=max_drift_scope,
                sam_rho=sam_rho, sam_adaptive=sam_adaptive, sam_eta=sam_eta)

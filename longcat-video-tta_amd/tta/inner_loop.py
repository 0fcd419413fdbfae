"""The test-time-adaptation inner loop as ONE engine for every method of the path.

Contract kept from the reference: the public functions `finetune_lora_on_conditioning` / `finetune_lora_batch`
(lora_experiment/scripts/run_lora_tta.py:425-634) with their argument names and defaults, and
the returned keys `losses`, `train_time`, `es_check_time`, `early_stopping_info`.  Per step: gradients dropped, linear
warm-up `lr * (step + 1) / warmup` while `step < warmup` (the last warm-up step sets exactly `lr`, nothing resets it
afterwards), a uniformly drawn augmentation variant, the conditioned flow-matching loss, backward, global-norm clip,
optimizer step, early-stopper hook; at the end the stopper's best state is written back and the model leaves train mode.

The reference carries four copies of this loop (LoRA, full model, their batch forms) plus one per delta method.  Here
`run_adaptation` is the only loop; the public functions describe WHAT is trained and WHERE the data comes from:
  * the optimizer is the fused multi-tensor clip + AdamW / SGD (two launches per step, `lcv_hip.ops`);
  * per-step losses stay on the device in a preallocated log and come to the host in one copy — the host never waits
    for a step (the reference's `loss.item()` at :516 drains the stream every step); it synchronises only where the
    early stopper needs a number, and once at the end so `train_time` covers the queued work;
  * the early stopper's snapshot is one reusable buffer set (`ParamSnapshot`), not a clone per improvement;
  * batch TTA stages every video's tensors in HBM once (288 GB) instead of a host->device copy per step (:603-606).
"""
import os
import time
from functools import partial
from typing import Callable, Dict, List, Optional, Sequence

import torch
import torch.nn as nn
from torch.utils.checkpoint import checkpoint

from lcv_hip.ops import FusedAdamWClip

from .early_stopping import AnchoredEarlyStopper, ParamSnapshot
from .flow_matching import compute_flow_matching_loss_conditioned
from .lora import get_lora_parameters

_ACT_BYTES_PER_TOKEN_BLOCK = 150e3     # measured: 3.7 GB per block at 25 200 tokens, hidden 4096, no checkpointing


def choose_gradient_checkpointing(dit: nn.Module, num_tokens: int, mode: str = None) -> bool:
    """The reference always checkpoints every block (lora_experiment/scripts/run_lora_tta.py:806-811) because an 80-141 GB
    GPU has to; an MI355X has 288 GB.  `mode` (default: env LCV_TTA_CHECKPOINT, else "auto"): "on" / "off" / "auto".
    auto keeps activations resident (no second forward, measured -23% step time at 25 200 tokens) when the estimate
    tokens x depth x 150 KB plus what is already allocated stays under 90% of the device memory."""
    mode = (mode or os.environ.get("LCV_TTA_CHECKPOINT", "auto")).lower()
    if mode == "auto":
        dev = next(dit.parameters()).device
        width = dit.config.hidden_size / 4096.0
        need = (num_tokens * len(dit.blocks) * _ACT_BYTES_PER_TOKEN_BLOCK * width + torch.cuda.memory_allocated(dev)
                + 30e9 * width * width)
        use = need > 0.90 * torch.cuda.get_device_properties(dev).total_memory
    else:
        use = mode != "off"
    dit.gradient_checkpointing = bool(use)
    dit._gradient_checkpointing_func = partial(checkpoint, use_reentrant=False) if use else None
    return bool(use)


# ------------------------------------------------------------------------------------------------ the engine
class _LossLog:
    """Per-step losses parked on the device; one device->host copy when somebody needs the numbers."""

    def __init__(self, capacity: int, device):
        self.buf = torch.zeros(max(capacity, 1), dtype=torch.float32, device=device)
        self.count = 0

    def push(self, loss: torch.Tensor) -> None:
        self.buf[self.count].copy_(loss.detach().reshape(()), non_blocking=True)
        self.count += 1

    def to_list(self) -> List[float]:
        return self.buf[:self.count].tolist()


def _variant_pool(train_latents, variants) -> List[torch.Tensor]:
    if variants is None:
        return [train_latents]
    return [v["latents"] for v in variants]


def run_adaptation(module: nn.Module, params: Sequence[torch.Tensor], optimizers: Sequence, loss_at: Callable[[int], torch.Tensor],
                   clip_and_step: Callable[[], None], num_steps: int, lr: float = 0.0, warmup_steps: int = 0,
                   early_stopper: Optional[AnchoredEarlyStopper] = None, grad_sync: Optional[Callable[[], None]] = None,
                   sam: Optional["_Sam"] = None, after_step: Optional[Callable[[], None]] = None, finish_eval: bool = True,
                   grad_accum: int = 1) -> Dict:
    """`loss_at(step)` returns the differentiable loss of that step; `clip_and_step()` owns clipping + the update.

    `grad_accum=N` with N > 1 puts N micro-steps behind every optimizer step: `loss_at(step * N + k)`, backward, `grad_sync()`
    and `opt.accumulate()` (fp32 accumulators, include/lcv_hip_accum.h) for k = 0 .. N-1, then `clip_and_step()`.  The step's
    logged loss is the micro losses added in order in fp32, times fp32(1/N), on the device.  `num_steps`, the warm-up and the
    early stopper's `check_every` count optimizer steps.

    `after_step()` runs right after every `clip_and_step()` - after the optimizer step only, never after a micro-step - and
    before the stopper looks at the parameters: the projection of `--max-drift` (`_MaxDrift`, include/lcv_hip_trust.h), so that
    what the stopper scores and snapshots are projected iterates.

    `sam` (a `_Sam`, `--sam-rho`, include/lcv_hip_sam.h) makes every optimizer step a sharpness-aware one: two forward/backward
    passes under the same generator states with the parameters perturbed in between and restored before `clip_and_step()`,
    which is unchanged.  The logged loss is the first pass's; the result gains the `sam` entry.  Not with `grad_accum` > 1.

    Optimizers that keep a weight average (`opt.weight_ema is not None`, include/lcv_hip_ema.h) have it swapped into the
    parameters around every due check of the stopper - so the average is what is scored and what `keeper.capture` snapshots,
    while training goes on from the raw masters, untouched bit for bit - and, without a stopper, once at the end, so that
    generation reads the average."""
    if grad_accum < 1:
        raise ValueError(f"grad_accum must be at least 1, got {grad_accum}")
    if sam is not None and grad_accum > 1:
        raise ValueError(SAM_REFUSALS["grad_accum"])
    averaged = [opt for opt in optimizers if getattr(opt, "weight_ema", None) is not None]
    device = params[0].device
    log = _LossLog(num_steps, device)
    keeper = None
    if early_stopper is not None:
        # the stopper's own initial snapshot (taken in setup) is refreshed in place when it covers the same tensors
        held = early_stopper.best_state
        keeper = held if isinstance(held, ParamSnapshot) and held.covers(params) else ParamSnapshot(params)
    module.train()
    es_seconds = 0.0
    started = time.perf_counter()
    for step in range(num_steps):
        for opt in optimizers:
            opt.zero_grad(set_to_none=True)
        if 0 < warmup_steps and step < warmup_steps:
            for opt in optimizers:
                for group in opt.param_groups:
                    group["lr"] = lr * (step + 1) / warmup_steps
        if grad_accum > 1:
            loss = _accumulate_micro_steps(optimizers, loss_at, grad_sync, step, grad_accum)
        elif sam is not None:
            loss = sam.two_passes(loss_at, step, grad_sync)
        else:
            loss = loss_at(step)
            loss.backward()
            if grad_sync is not None:
                grad_sync()
        clip_and_step()
        if after_step is not None:
            after_step()
        log.push(loss)
        del loss
        if early_stopper is None:
            continue
        done = step + 1
        due = done % early_stopper.check_every == 0
        if due:                       # the check's own time, not the wait for the training kernels queued before it
            torch.cuda.synchronize(device)
            tick = time.perf_counter()
            for opt in averaged:      # score the average ...
                opt.ema_swap()
        stop, info = early_stopper.step(done, save_fn=keeper.capture)
        if due:
            for opt in averaged:      # ... and train on from the masters, stop or not: swapping in and out is exact
                opt.ema_swap()
            torch.cuda.synchronize(device)
            es_seconds += time.perf_counter() - tick
        if stop:
            print(f"  early stop after step {done}: {info}")
            break
    if early_stopper is not None:
        early_stopper.restore(restore_fn=_put_back(params))
        # the snapshot holds the bf16 words that were scored, and they are what generation must use: a master-weight
        # optimizer drops the low words it accumulated past them
        for opt in optimizers:
            if hasattr(opt, "resync"):
                opt.resync()
    else:
        for opt in averaged:          # nothing was scored: the average of all steps is what generates
            opt.ema_swap()
    torch.cuda.synchronize(device)
    elapsed = time.perf_counter() - started
    if finish_eval:
        module.eval()
    return {"losses": log.to_list(), "train_time": elapsed, "es_check_time": es_seconds,
            "early_stopping_info": early_stopper.state if early_stopper is not None else None,
            **({} if sam is None else {"sam": sam.finish()})}


SAM_REFUSALS = {
    "grad_accum": "sam_rho cannot be combined with grad_accum > 1 (a perturbation per micro-step is a different algorithm)",
    "dora": "sam_rho cannot be combined with DoRA magnitudes (the row norm is held constant in the backward and the forward "
            "caches it)",
    "sp": "sam_rho cannot be combined with sequence parallelism (not exercised)",
}


def _rng_capture(device):
    """The host generator's state and, for a GPU, its default generator's: both live on the host, nothing waits for the device."""
    device = torch.device(device)
    if device.type != "cuda":
        return torch.get_rng_state(), None, None
    gen = torch.cuda.default_generators[device.index if device.index is not None else torch.cuda.current_device()]
    return torch.get_rng_state(), gen, gen.get_state()


def _rng_replay(captured) -> None:
    host, gen, state = captured
    torch.set_rng_state(host)
    if gen is not None:
        gen.set_state(state)


def sam_two_passes(optimizers, loss_at, step: int, grad_sync, perturb, restore, device):
    """One sharpness-aware step up to the optimizer's: first pass, `perturb(optimizers)`, gradients dropped, generators put
    back, second pass, `restore(optimizers)`.  The second pass sees the sigma, noise, augmentation variant and dropout masks of
    the first and leaves the generators exactly where a plain step would.  Returns (first loss, perturbed loss)."""
    captured = _rng_capture(device)
    loss = loss_at(step)
    loss.backward()
    if grad_sync is not None:
        grad_sync()
    perturb(optimizers)
    for opt in optimizers:
        opt.zero_grad(set_to_none=True)
    _rng_replay(captured)
    loss_p = loss_at(step)
    loss_p.backward()
    if grad_sync is not None:
        grad_sync()
    restore(optimizers)
    return loss, loss_p


class _Sam:
    """`--sam-rho RHO` for one adaptation (include/lcv_hip_sam.h): prepares every optimizer of the loop for one joint
    perturbation, runs the loop's two passes per step, keeps the perturbed losses in a device-side log of their own and
    afterwards gives the loop's result its `sam` entry."""

    def __init__(self, opts, rho: float, adaptive: bool, eta: float, num_steps: int):
        from lcv_hip import optim
        self._optim, self.opts = optim, list(opts)
        for opt in self.opts:
            opt.enable_sam(rho, adaptive, eta, trace_len=max(int(num_steps), 1))
        self._device = self.opts[0].params[0].device
        self._log = _LossLog(num_steps, self._device)

    def two_passes(self, loss_at, step: int, grad_sync) -> torch.Tensor:
        loss, loss_p = sam_two_passes(self.opts, loss_at, step, grad_sync, self._optim.sam_perturb, self._optim.sam_restore,
                                      self._device)
        self._log.push(loss_p)
        return loss

    def finish(self) -> Dict:
        """After the loop (after the stopper's restore): the traces in one copy per optimizer and the perturbed losses in one."""
        return {**self._optim.sam_stats(self.opts), "perturbed_loss_trace": self._log.to_list()}


def sam_hook(opts, rho: Optional[float], adaptive: bool, eta: float, num_steps: int) -> Optional[_Sam]:
    """A `_Sam` over `opts`, or None without a rho (then nothing is imported, allocated or launched)."""
    return None if rho is None else _Sam(opts, rho, adaptive, eta, num_steps)


def refuse_sam(module, sam_rho, grad_accum: int = 1, dora_magnitudes=None) -> None:
    """What the sharpness-aware step is not combined with, each with its one-line reason; nothing without a rho."""
    if sam_rho is None:
        return
    if grad_accum > 1:
        raise ValueError(SAM_REFUSALS["grad_accum"])
    if dora_magnitudes:
        raise ValueError(SAM_REFUSALS["dora"])
    if getattr(getattr(module, "dit", module), "_sp_group", None) is not None:
        raise ValueError(SAM_REFUSALS["sp"])


class _MaxDrift:
    """`--max-drift R` for one adaptation (include/lcv_hip_trust.h): puts the ball on every optimizer of the loop (one global
    ball over all of them, or one per tensor), is the loop's `after_step`, and afterwards adds `drift_norm` and the `max_drift`
    entry (the trace's summary) to the loop's result.  `anchors`: per optimizer its base values, or None for "its own anchor,
    else zeros" (fp32 vectors that start at zero)."""

    def __init__(self, opts, radius: float, scope: str, num_steps: int, anchors=None):
        from lcv_hip import optim
        self._optim, self.opts = optim, list(opts)
        for i, opt in enumerate(self.opts):
            opt.enable_max_drift(radius, scope, anchor=None if anchors is None else anchors[i], trace_len=max(int(num_steps), 1))

    def __call__(self) -> None:
        self._optim.project_max_drift(self.opts)

    def finish(self, out: Dict) -> Dict:
        """After the loop (after the stopper's restore and the final swap of a weight average): the drift of the weights that
        generate, and the trace in one copy per optimizer."""
        out["drift_norm"] = self._optim.max_drift_norm(self.opts)
        out["max_drift"] = self._optim.max_drift_stats(self.opts)
        return out


def max_drift_hook(opts, radius: Optional[float], scope: str, num_steps: int, anchors=None) -> Optional[_MaxDrift]:
    """A `_MaxDrift` over `opts`, or None without a radius (then nothing is imported, allocated or launched)."""
    return None if radius is None else _MaxDrift(opts, radius, scope, num_steps, anchors)


def _accumulate_micro_steps(optimizers, loss_at, grad_sync, step: int, n: int) -> torch.Tensor:
    """The micro-steps of optimizer step `step`; returns the step's loss for the log (fp32, on the device)."""
    total = None
    for k in range(n):
        loss = loss_at(step * n + k)
        loss.backward()
        if grad_sync is not None:        # per micro-step: sequence-parallel replicas hold identical gradients before they add
            grad_sync()
        for opt in optimizers:
            opt.accumulate()
        micro = loss.detach().reshape(()).to(torch.float32)
        total = micro if total is None else total + micro
        del loss
    return total * torch.tensor(1.0 / n, dtype=torch.float32)


def _put_back(params: Sequence[torch.Tensor]) -> Callable:
    """Restore callback accepting every snapshot form the stopper may hold: the engine's `ParamSnapshot`, a caller's
    list of tensors in parameter order (the runners' `save_fn`), or a name -> tensor mapping (the stopper's fallback)."""
    def restore(snapshot):
        if isinstance(snapshot, ParamSnapshot):
            snapshot.write_back()
            return
        with torch.no_grad():
            if isinstance(snapshot, dict):
                raise TypeError("name-keyed snapshots must be restored by the model's owner (pass restore_fn)")
            torch._foreach_copy_([p.detach() for p in params], [s.to(p.device) for s, p in zip(snapshot, params)])
    return restore


# ------------------------------------------------------------------------------------------------ data feeds
class _OneVideo:
    def __init__(self, cond, train, embeds, mask, variants):
        self.cond, self.embeds, self.mask = cond, embeds, mask
        self.pool = _variant_pool(train, variants)

    def __call__(self, step: int):
        pick = torch.randint(0, len(self.pool), (1,)).item()      # host RNG draw every step, like the reference (:499)
        return self.cond, self.pool[pick], self.embeds, self.mask


class _RoundRobin:
    """Retrieval-augmented batch TTA: step k trains on video k % n (run_lora_tta.py:596-606).  All videos are staged
    in HBM up front — a few hundred MB against 288 GB — so no step waits on a host->device copy."""

    def __init__(self, batch_data: List[Dict], device):
        def dev(t):
            return None if t is None else t.to(device, non_blocking=True)
        self.items = [(dev(b["cond_latents"]), dev(b["train_latents"]), dev(b["prompt_embeds"]), dev(b.get("prompt_mask")))
                      for b in batch_data]

    def __call__(self, step: int):
        return self.items[step % len(self.items)]


def _fm_loss(dit, feed, device, dtype):
    def at(step: int) -> torch.Tensor:
        cond, target, embeds, mask = feed(step)
        return compute_flow_matching_loss_conditioned(dit=dit, cond_latents=cond, target_latents=target, prompt_embeds=embeds,
                                                      prompt_mask=mask, device=device, dtype=dtype)
    return at


def _single_optimizer_step(opt, max_grad_norm: float) -> Callable[[], None]:
    def go():
        opt.clip_grad_norm_(max_grad_norm)
        opt.step()
    return go


def _sp_sync(dit, opt) -> Optional[Callable[[], None]]:
    # frame-sharded forward (sequence parallelism): every rank holds partial adapter gradients
    if getattr(dit, "_sp_group", None) is None:
        return None
    return lambda: dit.sequence_parallel_sync_grads(opt.params)


def refuse_stochastic_rounding_under_sp(module, stochastic_rounding: bool) -> None:
    """Every sequence-parallel rank would have to draw the same (seed, offset) pair for its replica of the parameters; the
    ranks' generators are not tied, so the combination is refused."""
    if stochastic_rounding and getattr(getattr(module, "dit", module), "_sp_group", None) is not None:
        raise ValueError("stochastic_rounding cannot be combined with sequence parallelism (every rank would have to draw "
                         "the same rounding bits)")


def _dora_optimizer(dit, dora_magnitudes, lr: float, **refused) -> Optional[FusedAdamWClip]:
    """The second optimizer of a DoRA run (tta/lora.py, include/lcv_hip_dora.h): an fp32 table over the magnitudes with the
    adapters' lr and betas and no weight decay (a decay would pull every row's length toward zero).  None without magnitudes.
    The options that belong to the bf16 master-weight forms, and sequence parallelism (the magnitudes' gradients would need a
    sync of their own), are refused before anything is built."""
    if not dora_magnitudes:
        return None
    on = [name for name, value in refused.items() if value]
    if on:
        raise ValueError(f"DoRA magnitudes cannot be combined with {', '.join(on)}: the fp32 magnitudes are stepped by a plain "
                         "AdamW tied to the adapters' by a joint clip, which those forms do not take part in")
    if getattr(getattr(dit, "dit", dit), "_sp_group", None) is not None:
        raise ValueError("DoRA magnitudes cannot be combined with sequence parallelism (their gradients are not synchronised)")
    if any(m.dtype != torch.float32 for m in dora_magnitudes):
        raise ValueError("DoRA magnitudes must be fp32 (a bf16 magnitude loses every update at these learning rates)")
    return FusedAdamWClip(list(dora_magnitudes), lr=lr, betas=(0.9, 0.999), weight_decay=0.0, eps=1e-8)


def _refuse_max_drift_with_dora(max_drift, dora_magnitudes) -> None:
    if max_drift is not None and dora_magnitudes:
        raise ValueError("max_drift cannot be combined with DoRA magnitudes (their bf16 adapters train without master weights, "
                         "which the ball needs)")


def _clones(params, max_drift):
    """The base words of a ball around what `params` hold now, as the one-optimizer `anchors` of `max_drift_hook`; None without a
    radius."""
    return None if max_drift is None else [[p.detach().clone() for p in params]]


def _joint_optimizer_step(opts, max_grad_norm: float) -> Callable[[], None]:
    """One clip coefficient over both optimizers' gradients, as the norm + delta tuning loop has it (tta/delta.py)."""
    def go():
        FusedAdamWClip.joint_clip_grad_norm_(opts, max_grad_norm)
        for opt in opts:
            opt.step()
    return go


# ------------------------------------------------------------------------------------------------ public: LoRA
def _adapter_params(lora_modules, lora_param_fn) -> List[torch.Tensor]:
    params = lora_param_fn() if lora_param_fn is not None else get_lora_parameters(lora_modules)
    if not params:
        raise ValueError("no LoRA parameters to train: inject adapters before the inner loop")
    return params


def finetune_lora_on_conditioning(dit: nn.Module, lora_modules, cond_latents: torch.Tensor,
                                  train_latents: torch.Tensor, prompt_embeds: torch.Tensor,
                                  prompt_mask: torch.Tensor, num_steps: int = 20, lr: float = 2e-4,
                                  warmup_steps: int = 3, weight_decay: float = 0.01, max_grad_norm: float = 1.0,
                                  device: str = "cuda", dtype: torch.dtype = torch.bfloat16,
                                  early_stopper: Optional[AnchoredEarlyStopper] = None, lora_param_fn=None,
                                  train_latents_variants: Optional[List[Dict]] = None, stochastic_rounding: bool = False,
                                  dora_magnitudes: Optional[Sequence[torch.Tensor]] = None,
                                  max_drift: Optional[float] = None, max_drift_scope: str = "global",
                                  sam_rho: Optional[float] = None, sam_adaptive: bool = False, sam_eta: float = 0.01,
                                  *, weight_ema: Optional[float] = None, ema_warmup: bool = False,
                                  grad_accum: int = 1, moments_8bit: bool = False, master_weights: bool = False) -> Dict:
    """`stochastic_rounding`: the bf16 adapters and moments take the fp32 step with stochastically rounded stores
    (include/lcv_hip_sr.h); no state beside them, so the stopper's snapshot and restore are the plain form's.
    `dora_magnitudes`: the fp32 magnitudes of DoRA adapters (tta.lora.get_dora_magnitudes), stepped by an optimizer of their own
    under one joint clip; the stopper's snapshot covers both lists.
    `max_drift` (with `master_weights`): after every step the adapters are projected onto a ball of that RMS radius around bf16
    clones of their freshly initialised values (+2 B / adapter parameter; include/lcv_hip_trust.h); the result gains
    `drift_norm` and `max_drift`.
    `sam_rho` (>= 0; `sam_adaptive`, `sam_eta`): every step is a sharpness-aware one (include/lcv_hip_sam.h, two
    forward/backward passes, +2 B / adapter parameter of saved words); the result gains `sam`.  Not with `grad_accum` > 1, DoRA
    magnitudes or sequence parallelism."""
    params = _adapter_params(lora_modules, lora_param_fn)
    _refuse_max_drift_with_dora(max_drift, dora_magnitudes)
    refuse_sam(dit, sam_rho, grad_accum, dora_magnitudes)
    refuse_stochastic_rounding_under_sp(dit, stochastic_rounding)
    dora_opt = _dora_optimizer(dit, dora_magnitudes, lr, master_weights=master_weights, moments_8bit=moments_8bit,
                               stochastic_rounding=stochastic_rounding, weight_ema=weight_ema is not None,
                               **{"grad_accum > 1": grad_accum > 1})
    # made per call, so per video: the low words of `master_weights` start at zero next to freshly reset adapters
    opt = FusedAdamWClip(params, lr=lr, betas=(0.9, 0.999), weight_decay=weight_decay, eps=1e-8,
                         master_weights=master_weights, moments_8bit=moments_8bit, stochastic_rounding=stochastic_rounding,
                         grad_accum=grad_accum)
    if weight_ema is not None:       # the fp32 average of the adapters (+4 B / parameter): scored by the stopper, left in the
        opt.enable_weight_ema(weight_ema, ema_warmup)    # adapters at the end (see run_adaptation)
    feed = _OneVideo(cond_latents, train_latents, prompt_embeds, prompt_mask, train_latents_variants)
    if dora_opt is not None:
        opts = [opt, dora_opt]
        return run_adaptation(dit, params + list(dora_magnitudes), opts, _fm_loss(dit, feed, device, dtype),
                              _joint_optimizer_step(opts, max_grad_norm), num_steps, lr, warmup_steps, early_stopper)
    ball = max_drift_hook([opt], max_drift, max_drift_scope, num_steps, _clones(params, max_drift))
    out = run_adaptation(dit, params, [opt], _fm_loss(dit, feed, device, dtype), _single_optimizer_step(opt, max_grad_norm),
                         num_steps, lr, warmup_steps, early_stopper, grad_sync=_sp_sync(dit, opt),
                         sam=sam_hook([opt], sam_rho, sam_adaptive, sam_eta, num_steps), after_step=ball, grad_accum=grad_accum)
    return out if ball is None else ball.finish(out)


def finetune_lora_batch(dit: nn.Module, lora_modules, batch_data: List[Dict], num_steps: int = 20, lr: float = 2e-4,
                        warmup_steps: int = 3, weight_decay: float = 0.01, max_grad_norm: float = 1.0,
                        device: str = "cuda", dtype: torch.dtype = torch.bfloat16, lora_param_fn=None,
                        stochastic_rounding: bool = False, dora_magnitudes: Optional[Sequence[torch.Tensor]] = None,
                        max_drift: Optional[float] = None, max_drift_scope: str = "global",
                        sam_rho: Optional[float] = None, sam_adaptive: bool = False, sam_eta: float = 0.01,
                        *, weight_ema: Optional[float] = None, ema_warmup: bool = False,
                        grad_accum: int = 1, moments_8bit: bool = False, master_weights: bool = False) -> Dict:
    """Shared adapters trained round-robin over the eval video and its neighbours; no early stopping (:558-634).  The feed
    receives the micro-step index, so `grad_accum` = number of videos puts every video behind each update.  `weight_ema`: the
    adapters end as their fp32 average over the steps.  `stochastic_rounding` and `dora_magnitudes`: as in
    `finetune_lora_on_conditioning`; `max_drift` and `sam_rho` likewise."""
    params = _adapter_params(lora_modules, lora_param_fn)
    _refuse_max_drift_with_dora(max_drift, dora_magnitudes)
    refuse_sam(dit, sam_rho, grad_accum, dora_magnitudes)
    refuse_stochastic_rounding_under_sp(dit, stochastic_rounding)
    dora_opt = _dora_optimizer(dit, dora_magnitudes, lr, master_weights=master_weights, moments_8bit=moments_8bit,
                               stochastic_rounding=stochastic_rounding, weight_ema=weight_ema is not None,
                               **{"grad_accum > 1": grad_accum > 1})
    opt = FusedAdamWClip(params, lr=lr, betas=(0.9, 0.999), weight_decay=weight_decay, eps=1e-8,
                         master_weights=master_weights, moments_8bit=moments_8bit, stochastic_rounding=stochastic_rounding,
                         grad_accum=grad_accum)
    if weight_ema is not None:
        opt.enable_weight_ema(weight_ema, ema_warmup)
    feed = _RoundRobin(batch_data, device)
    if dora_opt is not None:
        opts = [opt, dora_opt]
        return run_adaptation(dit, params + list(dora_magnitudes), opts, _fm_loss(dit, feed, device, dtype),
                              _joint_optimizer_step(opts, max_grad_norm), num_steps, lr, warmup_steps, None)
    ball = max_drift_hook([opt], max_drift, max_drift_scope, num_steps, _clones(params, max_drift))
    out = run_adaptation(dit, params, [opt], _fm_loss(dit, feed, device, dtype), _single_optimizer_step(opt, max_grad_norm),
                         num_steps, lr, warmup_steps, None, grad_sync=_sp_sync(dit, opt),
                         sam=sam_hook([opt], sam_rho, sam_adaptive, sam_eta, num_steps), after_step=ball, grad_accum=grad_accum)
    return out if ball is None else ball.finish(out)

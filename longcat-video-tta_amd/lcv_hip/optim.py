"""The fused multi-tensor optimizers: clip_grad_norm_ + AdamW / SGD over a parameter list in two launches.

Host code only: every method below builds a table of pointers and hands it to liblcv_hip.so through `ops.call`.  `ops`
re-exports the three public names (FusedAdamWClip, FusedSGDClip, ema_beta) and keeps the two process-wide switches the
optimizers touch: `ops.PARAM_EPOCH` is bumped here, `ops.is_deterministic()` is read here at call time.
"""
from collections import namedtuple

import torch

from . import lib as _lib
from . import ops
from .ops import BF16, F32, _U64, _ptr, _stream

# a device table: `desc` [n, 6] int64 rows of lcv_adam_tensor, `sides` name -> [n] int64 pointers parallel to it
_Table = namedtuple("_Table", "desc sides n chunks")


def ema_beta(beta: float, t: int, warmup: bool = False) -> float:
    """The beta of the t-th update (t counts from 1) of the weight average: `beta`, or under `warmup` the smaller of it and
    (1 + t) / (10 + t) - 0.18, 0.25, ..., 0.55 at t = 10, 0.70 at t = 20 - so that an average started at the base weights does
    not lag a run of 10-20 steps.  Formed in double."""
    beta = float(beta)
    return min(beta, (1.0 + t) / (10.0 + t)) if warmup else beta


# ===================================================================== fused clip + AdamW
class FusedAdamWClip:
    """clip_grad_norm_ + AdamW.step over a fixed parameter list in two launches (norm, update).

    Mirrors `AdamW(lora_params, lr, betas=(0.9, 0.999), weight_decay, eps=1e-8)` +
    `clip_grad_norm_(lora_params, max_norm)` of lora_experiment/scripts/run_lora_tta.py:462-468, 513-514,
    including the bf16 rounding points of the foreach implementation.  `param_groups` is kept so the reference's
    warm-up loop (`for pg in optimizer.param_groups: pg["lr"] = ...`) works unchanged.

    `master_weights=True` (bf16 parameters only) gives every parameter element an int16 low word (include/lcv_hip_master.h):
    the step then runs in fp32 on join(bf16 word, low word) with fp32 moments and rounds nothing to bf16 in between, so
    updates below half a bf16 ulp accumulate instead of vanishing.  The bf16 words stay where every GEMM reads them.
    Anyone else who writes the parameters (a restore, a reset) calls `resync()` afterwards.

    `moments_8bit=True` (with `master_weights=True` only) keeps each moment in one byte per element plus one fp32 scale per
    moment per 512 elements (include/lcv_hip_moments8.h): about 2.016 B / parameter of moments instead of 8.  The parameter
    update still uses the fp32 moments of the step; only what is kept between steps is quantised.

    `grad_accum=N` with N > 1 (with `master_weights=True` and fp32 moments only) makes one step the mean of N micro-steps
    (include/lcv_hip_accum.h): every parameter element gets a zeroed fp32 accumulator (+4 B / parameter); after each backward
    `accumulate()` adds `.grad * (1/N)` into it in fp32 and drops the `.grad`s; `clip_grad_norm_` and `step()` then read the
    accumulators as the (fp32) gradients, over every parameter that received a gradient in at least one micro-step, and refuse
    to run before N micro-steps are in.  `zero_grad()` zeroes the accumulators and starts the next step.

    `anchor=[...]` (with `master_weights=True` only; contiguous bf16 GPU tensors shaped like `params`, held by reference, not
    copied) turns the weight decay into a pull toward those base words instead of toward zero (include/lcv_hip_anchor.h): the
    step reads 2 B / parameter more and allocates nothing.  `drift_norm()` is the distance from them.

    `enable_weight_ema(beta)` (with `master_weights=True` only, once, before the first step) keeps an fp32 average of the masters
    (include/lcv_hip_ema.h, +4 B / parameter): every `step()` ends with e = w - beta_t * (w - e) in a launch of its own.
    `ema_swap()` exchanges the average and the masters bit for bit, so the model can be scored or run with the average and
    training can go on afterwards; while the average is in the parameters (`ema_in_params`) the optimizer refuses to train.

    `stochastic_rounding=True` (bf16 parameters only, and none of the master-weight options above) keeps the plain form's
    storage - bf16 parameters and bf16 moments, nothing beside them - and runs the master-weight form's fp32 step on them,
    rounding every stored value up or down at random so that it is an unbiased estimate of the fp32 result
    (include/lcv_hip_sr.h): updates below half a bf16 ulp and the decay of exp_avg_sq survive in expectation.  Every `step()`
    takes one (seed, offset) pair from the device's default generator (`ops.draw_philox_offset`, the generator moves on by 4),
    so the steps follow `torch.manual_seed`.

    `enable_max_drift(radius_rms, scope)` (bf16 parameters with `master_weights=True`, or fp32 parameters; once, before the first
    step) keeps the parameters inside a ball around their base values (include/lcv_hip_trust.h): the module-level
    `project_max_drift([...])`, called after the optimizers' `step()`s, measures |theta - theta0| in a fixed order and scales
    the drift back onto the ball where it has left it, on the device, with no host sync; a weight average then takes the
    projected masters.

    `enable_sam(rho, adaptive, eta)` (any parameter form; once, before the first step) prepares the sharpness-aware step
    (include/lcv_hip_sam.h, +2 B per bf16 parameter and +4 B per fp32 one of saved words): between a first and a second
    backward the module-level `sam_perturb([...])` moves the parameters to w + rho * g / |g| (one norm over every optimizer
    handed to it) and `sam_restore([...])` puts every word back, so `step()` takes the second gradient on bit-identical
    parameters.  While the parameters are perturbed (`sam_perturbed`) the optimizer refuses to clip, step, swap or project.

    A subclass supplies its `param_groups` entry (through `_init`), its moment storage (`_init_moments`), its hyper-parameter
    tuple (`_hyper`) and its `STEPS`."""
    CHUNK = 2048
    NORM_SLOTS = 64   # partial sums of squares per tensor (csrc/optim.hip)
    MOMENTS8_BLOCK = 512   # elements per scale (LCV_MOMENTS8_BLOCK)
    weight_ema = None        # the beta of enable_weight_ema(), or None: no average is kept
    ema_in_params = False    # True between an ema_swap() and the next: the parameters hold the average
    _ema = ()
    max_drift = None         # the RMS radius of enable_max_drift(), or None: no ball is kept
    sam_rho = None           # the rho of enable_sam(), or None: no sharpness-aware step is prepared
    sam_perturbed = False    # True between a sam_perturb() and its sam_restore(): the parameters hold the perturbed point

    # The step entry points as the headers list them (lcv_hip.h, lcv_hip_master.h, lcv_hip_accum.h, lcv_hip_moments8.h,
    # lcv_hip_anchor.h).  (anchor, moments_8bit, grad_accum > 1, master_weights) -> the entry point, the pointer tables that
    # follow the descriptors, whether param_f32 is passed (after the counts), whether grad_f32 is (before the stream).
    # A combination that is not here is one the constructor refuses.
    # Outside the table: the stochastic-rounding step (lcv_hip_sr.h) takes the plain table, no param_f32, and `seed, offset`
    # in front of the stream.
    SR_STEP = "lcv_sr_adamw_step"
    STEPS = {
        (False, False, False, False): ("lcv_adamw_step", (), True, False),
        (False, False, False, True): ("lcv_master_adamw_step", ("low",), False, False),
        (False, False, True, True): ("lcv_master_adamw_step_g32", ("low",), False, False),
        (False, True, False, True): ("lcv_master_adamw8_step", ("low", "scale"), False, False),
        (True, False, False, True): ("lcv_master_adamw_step_anchor", ("low", "anchor"), False, True),
        (True, False, True, True): ("lcv_master_adamw_step_anchor", ("low", "anchor"), False, True),
        (True, True, False, True): ("lcv_master_adamw8_step_anchor", ("low", "scale", "anchor"), False, False),
    }

    def __init__(self, params, lr=2e-4, betas=(0.9, 0.999), weight_decay=0.01, eps=1e-8, master_weights=False,
                 moments_8bit=False, stochastic_rounding=False, *, grad_accum: int = 1, anchor=None):
        self._init(params, dict(lr=lr, betas=betas, weight_decay=weight_decay, eps=eps), master_weights, moments_8bit,
                   grad_accum, anchor, stochastic_rounding)

    def _init(self, params, group, master_weights, moments_8bit, grad_accum, anchor, stochastic_rounding=False) -> None:
        """The constructor body of both optimizers; `group` is the `param_groups` entry without its `params`."""
        self.params = [p for p in params]
        if not self.params:
            raise ValueError("optimizer got an empty parameter list")
        dt = self.params[0].dtype
        if dt not in (BF16, F32) or any(p.dtype != dt for p in self.params):
            raise _lib.LcvError(f"{type(self).__name__}: parameters must be all bf16 or all fp32")
        self.f32 = dt == F32
        self.param_groups = [dict(params=self.params, **group)]
        self._init_stochastic_rounding(stochastic_rounding, master_weights, moments_8bit, grad_accum, anchor)
        self._init_master(master_weights)
        self._init_anchor(anchor)
        self.moments_8bit = bool(moments_8bit)
        self._scales = []
        self._init_moments()
        self._init_accum(grad_accum)
        self.step_count = 0
        dev = self.params[0].device
        self._ws = torch.zeros(len(self.params) * self.NORM_SLOTS, dtype=F32, device=dev)
        self._norm_coef = torch.zeros(2, dtype=F32, device=dev)
        self._have_coef = False
        self._tables = {}            # table name ("step", "micro", "ema", "drift") -> (key, _Table)
        self._det_ws = None

    def _init_moments(self) -> None:
        if self.moments_8bit:        # uint8 codes and fp32 block scales, zeroed: the state "all moments zero"
            if not self.master_weights:
                raise _lib.LcvError("FusedAdamWClip: moments_8bit=True needs master_weights=True (the 8-bit moments exist "
                                    "for the master-weight step only)")
            self.exp_avg = [torch.zeros(p.shape, dtype=torch.uint8, device=p.device) for p in self.params]
            self.exp_avg_sq = [torch.zeros(p.shape, dtype=torch.uint8, device=p.device) for p in self.params]
            self._scales = [torch.zeros((2, (p.numel() + self.MOMENTS8_BLOCK - 1) // self.MOMENTS8_BLOCK), dtype=F32,
                                        device=p.device) for p in self.params]
        elif self.master_weights:    # fp32 moments: +8 B / parameter
            self.exp_avg = [torch.zeros(p.shape, dtype=F32, device=p.device) for p in self.params]
            self.exp_avg_sq = [torch.zeros(p.shape, dtype=F32, device=p.device) for p in self.params]
        else:
            self.exp_avg = [torch.zeros_like(p) for p in self.params]
            self.exp_avg_sq = [torch.zeros_like(p) for p in self.params]

    def _hyper(self):
        g = self.param_groups[0]
        return (float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"]), float(g["weight_decay"]),
                self.step_count)

    def _init_master(self, master_weights: bool) -> None:
        """Zeroed int16 low words (+2 B / parameter) when master weights are on; `f32` stays False for the clip (the
        gradients are bf16, so a tensor's norm is still a bf16 number)."""
        self.master_weights = bool(master_weights)
        self._low = []
        if not self.master_weights:
            return
        name = type(self).__name__
        if self.f32:
            raise _lib.LcvError(f"{name}: master_weights=True is for bf16 parameters; fp32 parameters are already exact")
        if any(not p.is_cuda for p in self.params):
            raise _lib.LcvError(f"{name}: master_weights=True needs parameters on the GPU (no CPU path exists)")
        if any(not p.is_contiguous() for p in self.params):
            raise _lib.LcvError(f"{name}: master_weights=True needs contiguous parameters")
        self._low = [torch.zeros(p.shape, dtype=torch.int16, device=p.device) for p in self.params]

    def _init_stochastic_rounding(self, stochastic_rounding: bool, master_weights, moments_8bit, grad_accum, anchor) -> None:
        """Nothing is allocated: the storage is the plain form's.  Everything that belongs to the master-weight form is refused
        here, on the constructor's arguments, before that form's own checks ask for master_weights=True."""
        self.stochastic_rounding = bool(stochastic_rounding)
        if not self.stochastic_rounding:
            return
        name = type(self).__name__
        if self.f32:
            raise _lib.LcvError(f"{name}: stochastic_rounding=True is for bf16 parameters; an fp32 step rounds nothing to bf16")
        if any(not p.is_cuda for p in self.params):
            raise _lib.LcvError(f"{name}: stochastic_rounding=True needs parameters on the GPU (no CPU path exists)")
        if any(not p.is_contiguous() for p in self.params):
            raise _lib.LcvError(f"{name}: stochastic_rounding=True needs contiguous parameters")
        if master_weights:
            raise _lib.LcvError(f"{name}: stochastic_rounding=True cannot be combined with master_weights=True (the master "
                                "weights are already exact)")
        for on, what in ((moments_8bit, "moments_8bit=True"), (int(grad_accum) > 1, "grad_accum > 1"),
                         (anchor is not None, "anchor")):
            if on:
                raise _lib.LcvError(f"{name}: stochastic_rounding=True cannot be combined with {what} (it exists for the "
                                    "master-weight form only)")

    def _check_anchor(self, anchor, dtype=BF16):
        """A list of base words that fits `params`: contiguous bf16 GPU tensors of the parameters' shapes (fp32 ones for the
        ball of fp32 parameters, enable_max_drift)."""
        name = type(self).__name__
        anchor = [a for a in anchor]
        if len(anchor) != len(self.params):
            raise _lib.LcvError(f"{name}: anchor has {len(anchor)} tensors for {len(self.params)} parameters")
        for a, p in zip(anchor, self.params):
            if a.dtype != dtype or not a.is_cuda or not a.is_contiguous() or a.shape != p.shape or a.device != p.device:
                raise _lib.LcvError(f"{name}: every anchor must be a contiguous {'bf16' if dtype == BF16 else 'fp32'} tensor on the "
                                    f"parameter's GPU with its shape; got {a.dtype} {tuple(a.shape)} on {a.device} for "
                                    f"{tuple(p.shape)}")
        return anchor

    def _init_anchor(self, anchor) -> None:
        """The base words the decay pulls toward, held by reference; nothing without them."""
        self._anchor = []
        if anchor is None:
            return
        if not self.master_weights:
            raise _lib.LcvError(f"{type(self).__name__}: anchor needs master_weights=True (a pull of lr * wd * (w - w0) is far "
                                "below half a bf16 ulp; the anchor steps exist for the master-weight form only)")
        self._anchor = self._check_anchor(anchor)

    # ------------------------------------------------------------------------------------------------ the device tables
    def _build_table(self, sel, cols=None, **sides) -> _Table:
        """The rows [param, c1, c2, c3, numel, first_chunk] of the parameters `sel` (indices into `params`) on the device.
        `cols`: per row the three pointers of the middle columns (gradient and the two moment slots), or nothing for zeros.  `sides`: name -> list over ALL parameters whose pointers at `sel` become an array parallel to
        the rows.  The selection, the refusal of an empty one and the cache key are the caller's."""
        dev = self.params[0].device
        rows, chunk = [], 0
        for i, c in zip(sel, cols or [(0, 0, 0)] * len(sel)):
            p = self.params[i]
            rows.append([p.data_ptr(), *c, p.numel(), chunk])
            chunk += (p.numel() + self.CHUNK - 1) // self.CHUNK
        return _Table(torch.tensor(rows, dtype=torch.int64).to(dev),
                      {k: torch.tensor([ts[i].data_ptr() for i in sel], dtype=torch.int64).to(dev) for k, ts in sides.items()},
                      len(sel), chunk)

    def _cached(self, name: str, key, build) -> _Table:
        """The table `name`, built again when `key` is not the one it was built under."""
        hit = self._tables.get(name)
        if hit is None or hit[0] != key:
            hit = self._tables[name] = (key, build())
        return hit[1]

    def _with_grad(self):
        """The parameters that hold a `.grad` and those gradients, contiguous."""
        sel, grads = [], []
        for i, p in enumerate(self.params):
            if p.grad is None:
                continue
            sel.append(i)
            grads.append(p.grad if p.grad.is_contiguous() else p.grad.contiguous())
        return sel, grads

    def _nonempty(self):
        return [i for i, p in enumerate(self.params) if p.numel()]

    def drift_norm(self, anchor=None) -> torch.Tensor:
        """|theta - theta0| over ALL parameters (with or without a gradient) as a 0-dim fp32 device tensor, no host sync
        (lcv_master_drift_sumsq, fixed order): theta is join(bf16 word, low word) under master weights and the bf16 word
        without them; theta0 the optimizer's anchor, or the list passed in."""
        name = type(self).__name__
        if self.f32:
            raise _lib.LcvError(f"{name}: drift_norm() is for bf16 parameters")
        if anchor is not None:
            anchor = self._check_anchor(anchor)
        elif self._anchor:
            anchor = self._anchor
        else:
            raise _lib.LcvError(f"{name}: drift_norm() needs an anchor (the optimizer holds none)")
        if any(not p.is_cuda or not p.is_contiguous() for p in self.params):
            raise _lib.LcvError(f"{name}: drift_norm() needs contiguous parameters on the GPU")
        sel = self._nonempty()
        if not sel:
            raise _lib.LcvError(f"{name}: drift_norm() over no elements")
        key = tuple(a.data_ptr() for a in anchor) + tuple(p.data_ptr() for p in self.params)
        sides = dict(anchor=anchor, low=self._low) if self.master_weights else dict(anchor=anchor)
        t = self._cached("drift", key, lambda: self._build_table(sel, **sides))
        dev = self.params[0].device
        part = torch.empty((t.chunks,), dtype=F32, device=dev)
        out = torch.empty(2, dtype=F32, device=dev)
        ops.call("lcv_master_drift_sumsq", _ptr(t.desc), _ptr(t.sides.get("low")), _ptr(t.sides["anchor"]), t.n, t.chunks,
                 _ptr(part), t.chunks * 4, _ptr(out), _stream())
        return out[1]

    def enable_weight_ema(self, beta: float, warmup: bool = False) -> None:
        """Start the fp32 average of the masters (+4 B / parameter) at the masters themselves (lcv_master_ema_load).  Once, before
        the first `step()`.  `warmup`: the t-th update uses `ema_beta(beta, t, True)` instead of `beta`."""
        name = type(self).__name__
        if self.weight_ema is not None:
            raise _lib.LcvError(f"{name}: enable_weight_ema() was already called")
        beta = float(beta)
        if not 0.0 <= beta < 1.0:            # a NaN fails both
            raise ValueError(f"{name}: the beta of the weight average must be in [0, 1), got {beta}")
        if not self.master_weights:
            raise _lib.LcvError(f"{name}: enable_weight_ema() needs master_weights=True (an increment (1 - beta) * (w - e) is far "
                                "below half a bf16 ulp; the average is kept in fp32 beside the master weights only)")
        if self.step_count:
            raise _lib.LcvError(f"{name}: enable_weight_ema() comes before the first step(), not after {self.step_count}")
        self._ema = [torch.empty(p.shape, dtype=F32, device=p.device) for p in self.params]
        self.weight_ema = beta
        self._ema_warmup = bool(warmup)
        self.ema_in_params = False
        self.ema_reset()

    def _ema_table(self):
        """The leading arguments of the three average entry points: the descriptor table over ALL non-empty parameters (with or
        without a gradient, as drift_norm's) with the low-word and the average pointers beside it, and the counts."""
        sel = self._nonempty()
        if not sel:
            raise _lib.LcvError(f"{type(self).__name__}: a weight average over no elements")
        # keyed on the averages as well as the parameters: whoever replaces an entry of `_ema` (a test moving one into an offset
        # view) gets a new table without having to know that a cache exists
        t = self._cached("ema", tuple(t.data_ptr() for ts in (self.params, self._ema) for t in ts),
                         lambda: self._build_table(sel, low=self._low, ema=self._ema))
        return _ptr(t.desc), _ptr(t.sides["low"]), _ptr(t.sides["ema"]), t.n, t.chunks

    def _ema_needs(self, what: str) -> None:
        if self.weight_ema is None:
            raise _lib.LcvError(f"{type(self).__name__}: {what} needs enable_weight_ema()")

    def _ema_guard(self, what: str) -> None:
        """Nobody trains the average by accident."""
        if self.ema_in_params:
            raise _lib.LcvError(f"{type(self).__name__}: {what} while the parameters hold the weight average (ema_in_params); "
                                "call ema_swap() to put the masters back first")

    def ema_tensors(self):
        """The fp32 averages themselves, one per parameter in `params` order (empty without enable_weight_ema()).  While
        `ema_in_params` they hold the masters."""
        return list(self._ema)

    def ema_reset(self) -> None:
        """Load the average again from the masters and start its update count (the t of `ema_beta`) at zero."""
        self._ema_needs("ema_reset()")
        self._ema_guard("ema_reset()")
        ops.call("lcv_master_ema_load", *self._ema_table(), _stream())
        self._ema_t = 0

    def _ema_update(self) -> None:
        """What step() ends with when an average is kept: its own launch after whichever step kernel ran."""
        self._ema_t += 1
        ops.call("lcv_master_ema_update", *self._ema_table(), ema_beta(self.weight_ema, self._ema_t, self._ema_warmup), _stream())

    def ema_swap(self) -> None:
        """Exchange the average and the masters (lcv_master_ema_swap) and toggle `ema_in_params`: after one call the parameters
        are the average in valid master format (bf16 word = its round-to-nearest), after two every bit is back."""
        self._ema_needs("ema_swap()")
        self._sam_guard("ema_swap()")
        ops.call("lcv_master_ema_swap", *self._ema_table(), _stream())
        self.ema_in_params = not self.ema_in_params
        ops.PARAM_EPOCH += 1         # the parameters changed under cached copies of them, as after a step

    # ------------------------------------------------------------------------------------------------ the trust region
    MAX_DRIFT_SCOPES = ("global", "tensor")   # LCV_TRUST_GLOBAL, LCV_TRUST_TENSOR

    def enable_max_drift(self, radius_rms: float, scope: str = "global", anchor=None, trace_len: int = 4096) -> None:
        """Keep the parameters inside a ball around their base values (include/lcv_hip_trust.h): after every step,
        `project_max_drift([...])` scales the drift theta - theta0 back onto the ball when it has left it.  `radius_rms` > 0 is
        the radius in RMS per element (`inf`: nothing is ever written, the trace is still recorded); `scope` "global" is one ball
        over every optimizer handed to `project_max_drift` together, "tensor" one ball per parameter tensor.  For bf16
        parameters with `master_weights=True`, or for fp32 parameters.  `anchor`: the base values (bf16 words for bf16
        parameters, fp32 values for fp32 ones, held by reference); None reuses the optimizer's own `anchor=`, else means zeros
        for fp32 parameters and is refused for bf16 ones.  Once, before the first `step()`.  Allocates one float per chunk and
        per tensor and `trace_len` pairs of floats for the per-step trace; steps past `trace_len` are projected and not
        recorded."""
        name = type(self).__name__
        if self.max_drift is not None:
            raise _lib.LcvError(f"{name}: enable_max_drift() was already called")
        radius = float(radius_rms)
        if not radius > 0.0:                 # a NaN fails too
            raise _lib.LcvError(f"{name}: the radius of enable_max_drift() must be > 0 (RMS per element, inf allowed), got {radius}")
        if scope not in self.MAX_DRIFT_SCOPES:
            raise _lib.LcvError(f"{name}: the scope of enable_max_drift() is 'global' or 'tensor', got {scope!r}")
        if self.stochastic_rounding:
            raise _lib.LcvError(f"{name}: enable_max_drift() cannot be combined with stochastic_rounding=True (the ball needs "
                                "master weights)")
        if not self.f32 and not self.master_weights:
            raise _lib.LcvError(f"{name}: enable_max_drift() on bf16 parameters needs master_weights=True (a contraction "
                                "(1 - c) * |d| below half a bf16 ulp rounds back to the same word, so the bound would not hold)")
        if self.step_count:
            raise _lib.LcvError(f"{name}: enable_max_drift() comes before the first step(), not after {self.step_count}")
        if int(trace_len) < 1:
            raise _lib.LcvError(f"{name}: trace_len must be at least 1, got {trace_len}")
        if any(not p.is_cuda or not p.is_contiguous() for p in self.params):
            raise _lib.LcvError(f"{name}: enable_max_drift() needs contiguous parameters on the GPU (no CPU path exists)")
        if anchor is not None:
            anchor = self._check_anchor(anchor, F32 if self.f32 else BF16)
        elif self._anchor:
            anchor = self._anchor
        elif not self.f32:
            raise _lib.LcvError(f"{name}: enable_max_drift() on bf16 parameters needs an anchor (the optimizer holds none)")
        sel = self._nonempty()
        if not sel:
            raise _lib.LcvError(f"{name}: a ball over no elements")
        dev = self.params[0].device
        chunks = sum((self.params[i].numel() + self.CHUNK - 1) // self.CHUNK for i in sel)
        self._md_anchor = anchor             # a list, or None: every base value is zero
        self._md_scope = scope
        self._md_numel = sum(self.params[i].numel() for i in sel)
        self._md_part = torch.empty((chunks,), dtype=F32, device=dev)
        self._md_per = torch.empty((len(sel),), dtype=F32, device=dev)
        self._md_out = torch.zeros(2, dtype=F32, device=dev)
        self._md_trace = torch.zeros((int(trace_len), 2), dtype=F32, device=dev)
        self._md_steps = 0
        self._md_stepped = False             # a step() since the last projection: its weight average is due an update
        self.max_drift = radius

    def _md_needs(self, what: str) -> None:
        if self.max_drift is None:
            raise _lib.LcvError(f"{type(self).__name__}: {what} needs enable_max_drift()")

    def _trust_args(self):
        """The leading arguments of the two trust entry points: the descriptor table over ALL non-empty parameters (with or
        without a gradient, as drift_norm's), the low-word and base pointers beside it, the counts and param_f32."""
        sides = {k: ts for k, ts in (("low", self._low), ("anchor", self._md_anchor)) if ts}
        key = tuple(t.data_ptr() for ts in (self.params, *sides.values()) for t in ts)
        t = self._cached("trust", key, lambda: self._build_table(self._nonempty(), **sides))
        return _ptr(t.desc), _ptr(t.sides.get("low")), _ptr(t.sides.get("anchor")), t.n, t.chunks, 1 if self.f32 else 0

    def drift_sumsq(self) -> torch.Tensor:
        """|theta - theta0|^2 over ALL parameters of this optimizer as a 0-dim fp32 device tensor, no host sync (lcv_trust_sumsq,
        fixed order); the per-tensor sums are left in `_md_per`.  The tensor is the optimizer's own buffer: the next call
        overwrites it."""
        self._md_needs("drift_sumsq()")
        ops.call("lcv_trust_sumsq", *self._trust_args(), _ptr(self._md_part), self._md_part.numel() * 4, _ptr(self._md_per),
                 _ptr(self._md_out), _stream())
        return self._md_out[0]

    def _trust_project(self, sumsq: torch.Tensor, numel: int) -> None:
        """Launch this optimizer's projection against the total `sumsq` (a device tensor) of a ball of `numel` elements, and
        record the step in the trace while it has room."""
        tensor = self._md_scope == "tensor"
        rr = self.max_drift * self.max_drift * (1.0 if tensor else float(numel))      # R * R [* N], formed in double
        slot = self._md_trace[self._md_steps] if self._md_steps < self._md_trace.shape[0] else None
        ops.call("lcv_trust_project", *self._trust_args(), _lib.LCV_TRUST_TENSOR if tensor else _lib.LCV_TRUST_GLOBAL, _ptr(sumsq),
                 _ptr(self._md_per), rr, _ptr(slot), _stream())
        self._md_steps += 1

    def max_drift_trace(self) -> torch.Tensor:
        """The trace so far as a [steps, 2] fp32 CPU tensor, read in one copy: per projected step the total |theta - theta0|^2
        before the projection (of the whole ball in global scope, of this optimizer in tensor scope) and the smallest
        coefficient applied (1.0: nothing was projected)."""
        self._md_needs("max_drift_trace()")
        return self._md_trace[:min(self._md_steps, self._md_trace.shape[0])].cpu()

    # ------------------------------------------------------------------------------------------------ the sharpness-aware step
    def enable_sam(self, rho: float, adaptive: bool = False, eta: float = 0.01, trace_len: int = 4096) -> None:
        """Prepare the sharpness-aware step (include/lcv_hip_sam.h): `sam_perturb([...])` after a first backward moves the
        parameters that hold a gradient to w + rho * g / |g| (`adaptive`: ASAM's |w| + eta scaling) and `sam_restore([...])`
        after the second backward puts every word back.  `rho` >= 0 and finite (0: both passes run, nothing is written, the
        gradient-norm trace is recorded).  For every parameter form; bf16 parameters take bf16 gradients, so not with
        `grad_accum` > 1.  Once, before the first `step()`.  Allocates the saved words of all non-empty parameters (+2 B per bf16
        parameter, +4 B per fp32 one), one float per chunk and per tensor, and `trace_len` pairs of floats for the per-step
        trace; steps past `trace_len` are perturbed and not recorded."""
        name = type(self).__name__
        if self.sam_rho is not None:
            raise _lib.LcvError(f"{name}: enable_sam() was already called")
        rho, eta = float(rho), float(eta)
        if not 0.0 <= rho < float("inf"):     # a NaN fails too
            raise _lib.LcvError(f"{name}: the rho of enable_sam() must be finite and >= 0, got {rho}")
        if not 0.0 <= eta < float("inf"):
            raise _lib.LcvError(f"{name}: the eta of enable_sam() must be finite and >= 0, got {eta}")
        if self.grad_accum > 1:
            raise _lib.LcvError(f"{name}: enable_sam() cannot be combined with grad_accum > 1 (a perturbation per micro-step is a "
                                "different algorithm)")
        if self.step_count:
            raise _lib.LcvError(f"{name}: enable_sam() comes before the first step(), not after {self.step_count}")
        if int(trace_len) < 1:
            raise _lib.LcvError(f"{name}: trace_len must be at least 1, got {trace_len}")
        if any(not p.is_cuda or not p.is_contiguous() for p in self.params):
            raise _lib.LcvError(f"{name}: enable_sam() needs contiguous parameters on the GPU (no CPU path exists)")
        sel = self._nonempty()
        if not sel:
            raise _lib.LcvError(f"{name}: a perturbation over no elements")
        dev = self.params[0].device
        chunks = sum((self.params[i].numel() + self.CHUNK - 1) // self.CHUNK for i in sel)
        self._sam_adaptive, self._sam_eta = bool(adaptive), eta
        self._sam_save = [torch.empty_like(p) for p in self.params]      # the words the forward reads, saved exactly
        self._sam_part = torch.empty((chunks,), dtype=F32, device=dev)
        self._sam_per = torch.empty((len(sel),), dtype=F32, device=dev)
        self._sam_out = torch.zeros(2, dtype=F32, device=dev)
        self._sam_real = torch.zeros(2, dtype=F32, device=dev)
        self._sam_trace = torch.zeros((int(trace_len), 2), dtype=F32, device=dev)
        self._sam_steps = 0
        self._sam_live = None                # the table of the perturbation under way, kept for its restore
        self.sam_rho = rho

    def _sam_needs(self, what: str) -> None:
        if self.sam_rho is None:
            raise _lib.LcvError(f"{type(self).__name__}: {what} needs enable_sam()")

    def _sam_guard(self, what: str) -> None:
        """Nobody steps, clips, swaps or projects the perturbed point by accident."""
        if self.sam_perturbed:
            raise _lib.LcvError(f"{type(self).__name__}: {what} while the parameters are perturbed (sam_perturbed); call "
                                "sam_restore() to put them back first")

    def _sam_measure(self) -> bool:
        """lcv_sam_sumsq over the parameters that hold a gradient, into `_sam_out`; False (and nothing launched) when none does.
        The table is kept in `_sam_live` for the perturbation and its restore."""
        sel, grads = [], []
        for i, g in zip(*self._with_grad()):
            if self.params[i].numel():
                sel.append(i)
                grads.append(g)
        if not sel:
            self._sam_live = None
            return False
        if any(g.dtype != self.params[0].dtype for g in grads):
            raise _lib.LcvError(f"{type(self).__name__}: sam_perturb() takes gradients of the parameters' dtype")
        self._sam_grads = grads              # keep alive until the perturbation is launched
        sides = {k: ts for k, ts in (("low", self._low), ("save", self._sam_save)) if ts}
        key = tuple(g.data_ptr() for g in grads) + tuple(sel) + tuple(t.data_ptr() for ts in (self.params, *sides.values()) for t in ts)
        t = self._sam_live = self._cached("sam", key, lambda: self._build_table(sel, [(g.data_ptr(), 0, 0) for g in grads], **sides))
        ops.call("lcv_sam_sumsq", _ptr(t.desc), _ptr(t.sides.get("low")), t.n, t.chunks, 1 if self.f32 else 0,
                 1 if self._sam_adaptive else 0, self._sam_eta, _ptr(self._sam_part), self._sam_part.numel() * 4,
                 _ptr(self._sam_per), _ptr(self._sam_out), _stream())
        return True

    def _sam_perturb(self, sumsq: torch.Tensor) -> None:
        """Launch this optimizer's perturbation against the total `sumsq` (a device tensor) and record the step in the trace
        while it has room."""
        t = self._sam_live
        slot = self._sam_trace[self._sam_steps] if self._sam_steps < self._sam_trace.shape[0] else None
        ops.call("lcv_sam_perturb", _ptr(t.desc), _ptr(t.sides.get("low")), _ptr(t.sides["save"]), t.n, t.chunks,
                 1 if self.f32 else 0, 1 if self._sam_adaptive else 0, self._sam_eta, self.sam_rho, _ptr(sumsq),
                 _ptr(self._sam_part), self._sam_part.numel() * 4, _ptr(self._sam_per), _ptr(self._sam_real), _ptr(slot), _stream())
        self._sam_grads = None
        self.sam_perturbed = True

    def _sam_restore(self) -> None:
        t = self._sam_live
        ops.call("lcv_sam_restore", _ptr(t.desc), _ptr(t.sides["save"]), t.n, t.chunks, 1 if self.f32 else 0, _stream())
        self.sam_perturbed = False

    def sam_trace(self) -> torch.Tensor:
        """The trace so far as a [steps, 2] fp32 CPU tensor, read in one copy: per perturbed step the total sum of squares of
        the (scaled) gradient the perturbation was normalised by (of every optimizer perturbed together) and the sum of squares
        of what this optimizer's stored words really moved by; a step in which this optimizer held no gradient is a row of
        zeros."""
        self._sam_needs("sam_trace()")
        return self._sam_trace[:min(self._sam_steps, self._sam_trace.shape[0])].cpu()

    def _init_accum(self, grad_accum: int) -> None:
        """Zeroed fp32 accumulators (+4 B / parameter) when `grad_accum` > 1; nothing at 1."""
        self.grad_accum = int(grad_accum)
        self._acc = []
        self._acc_live = set()       # indices of the parameters that received a gradient in a micro-step of this step
        self._micro = 0
        if self.grad_accum < 1:
            raise ValueError(f"grad_accum must be at least 1, got {grad_accum}")
        if self.grad_accum == 1:
            return
        name = type(self).__name__
        if not self.master_weights:
            raise _lib.LcvError(f"{name}: grad_accum > 1 needs master_weights=True (the fp32-gradient steps exist for the "
                                "master-weight form only)")
        if self.moments_8bit:
            raise _lib.LcvError(f"{name}: grad_accum > 1 needs moments_8bit=False (the 8-bit-moment step reads bf16 gradients)")
        self._acc = [torch.zeros(p.shape, dtype=F32, device=p.device) for p in self.params]

    def accumulated_grads(self):
        """The fp32 accumulators, one per parameter in `params` order (empty at grad_accum=1)."""
        return list(self._acc)

    def accumulate(self) -> None:
        """One micro-step: acc += float(.grad) * (1 / grad_accum) over the parameters that hold a `.grad`
        (lcv_grad_accumulate), then those `.grad`s are dropped."""
        name = type(self).__name__
        self._ema_guard("accumulate()")
        if self.grad_accum == 1:
            raise _lib.LcvError(f"{name}: accumulate() needs grad_accum > 1")
        if self._micro >= self.grad_accum:
            raise _lib.LcvError(f"{name}: {self._micro} of {self.grad_accum} micro-steps are already accumulated; step() and "
                                "zero_grad() come next")
        sel, grads = self._with_grad()
        if not sel:
            raise _lib.LcvError(f"{name}: no parameter has a gradient")
        t = self._cached("micro", tuple(g.data_ptr() for g in grads) + tuple(sel),
                         lambda: self._build_table(sel, [(g.data_ptr(), 0, 0) for g in grads], acc=self._acc))
        ops.call("lcv_grad_accumulate", _ptr(t.desc), _ptr(t.sides["acc"]), t.n, t.chunks, 1.0 / self.grad_accum, _stream())
        for i in sel:
            self.params[i].grad = None
        self._acc_live.update(sel)
        self._micro += 1

    def _accumulated(self):
        """The active set and its gradients under grad_accum > 1: the accumulators of every parameter that received a gradient
        in at least one micro-step.  Refuses before all micro-steps are in."""
        if self._micro != self.grad_accum:
            raise _lib.LcvError(f"{type(self).__name__}: {self._micro} of {self.grad_accum} micro-steps accumulated; call "
                                "accumulate() after every backward before clipping or stepping")
        sel = sorted(self._acc_live)
        return sel, [self._acc[i] for i in sel]

    @property
    def low_words(self):
        """The int16 low-word tensors, one per parameter in `params` order (empty without master weights)."""
        return list(self._low)

    def resync(self) -> None:
        """Zero the low words: the masters become exactly the bf16 words the parameters hold now.  Call it after anyone
        but this optimizer has written the parameters.  A weight average (enable_weight_ema) is left alone: it neither moves to
        the new masters nor restarts; `ema_reset()` does that."""
        for low in self._low:
            low.zero_()

    def master_tensors(self):
        """fp32 copies of the masters, one per parameter (lcv_master_join)."""
        if not self.master_weights:
            raise _lib.LcvError(f"{type(self).__name__}: master_tensors() needs master_weights=True")
        out = []
        for p, low in zip(self.params, self._low):
            m = torch.empty(p.shape, dtype=F32, device=p.device)
            if p.numel():
                ops.call("lcv_master_join", _ptr(p), _ptr(low), _ptr(m), p.numel(), _stream())
            out.append(m)
        return out

    def moment_tensors(self):
        """fp32 copies of the moments, one (exp_avg, exp_avg_sq) pair per parameter; decoded (lcv_moments8_decode) under
        moments_8bit=True."""
        out = []
        for i, p in enumerate(self.params):
            if not self.moments_8bit:
                out.append((self.exp_avg[i].to(F32, copy=True), self.exp_avg_sq[i].to(F32, copy=True)))
                continue
            m = torch.zeros(p.shape, dtype=F32, device=p.device)
            v = torch.zeros(p.shape, dtype=F32, device=p.device)
            if p.numel():
                ops.call("lcv_moments8_decode", _ptr(self.exp_avg[i]), _ptr(self.exp_avg_sq[i]), _ptr(self._scales[i]), _ptr(m),
                         _ptr(v), p.numel(), _stream())
            out.append((m, v))
        return out

    def state_bytes(self) -> int:
        """Bytes of optimizer state: both moments and, under moments_8bit=True, their scales.  The low words are not counted."""
        return sum(t.numel() * t.element_size() for ts in (self.exp_avg, self.exp_avg_sq, self._scales) for t in ts)

    def zero_grad(self, set_to_none: bool = True):
        for p in self.params:
            p.grad = None if set_to_none else (p.grad.zero_() if p.grad is not None else None)
        self._have_coef = False
        if self._acc:                # grad_accum > 1: the next optimizer step starts from zeroed accumulators
            torch._foreach_zero_(self._acc)
            self._acc_live.clear()
            self._micro = 0

    def _step_table(self) -> _Table:
        """The table over the parameters that received a gradient (torch's AdamW and clip_grad_norm_ skip `grad is None` the
        same way), with the low-word, base-word and block-scale pointers the optimizer has beside it.  Under grad_accum > 1
        the gradients are the fp32 accumulators."""
        sel, grads = self._accumulated() if self.grad_accum > 1 else self._with_grad()
        if not sel:
            raise _lib.LcvError("FusedAdamWClip: no parameter has a gradient")
        self._grads = grads  # keep alive until the launch
        sides = {k: ts for k, ts in (("low", self._low), ("anchor", self._anchor), ("scale", self._scales)) if ts}
        m, v = self.exp_avg, self.exp_avg_sq
        return self._cached("step", tuple(g.data_ptr() for g in grads) + tuple(sel), lambda: self._build_table(
            sel, [(g.data_ptr(), m[i].data_ptr(), v[i].data_ptr()) for i, g in zip(sel, grads)], **sides))

    @property
    def _grad_f32(self) -> bool:
        """Whether the clip reads fp32 gradients: fp32 parameters, or the accumulators of grad_accum > 1 (an fp32 gradient's
        norm is an fp32 number)."""
        return self.f32 or self.grad_accum > 1

    def clip_grad_norm_(self, max_norm: float) -> torch.Tensor:
        self._ema_guard("clip_grad_norm_()")
        self._sam_guard("clip_grad_norm_()")
        t = self._step_table()
        head = (_ptr(t.desc), t.n, t.chunks, 1 if self._grad_f32 else 0, float(max_norm), _ptr(self._ws), _ptr(self._norm_coef))
        if ops.is_deterministic():   # one fp32 partial per chunk for the fixed-order clip
            if self._det_ws is None or self._det_ws.numel() != t.chunks:
                self._det_ws = torch.empty((t.chunks,), dtype=F32, device=self.params[0].device)
            ops.call("lcv_det_grad_norm_clip", *head, _ptr(self._det_ws), t.chunks * 4, _stream())
        else:
            ops.call("lcv_grad_norm_clip", *head, _stream())
        self._have_coef = True
        return self._norm_coef[0]

    @staticmethod
    def joint_clip_grad_norm_(opts, max_norm: float) -> float:
        """ONE clip over several optimizers' parameters (a bf16 list and an fp32 list under the same
        `clip_grad_norm_(all_params, max_norm)`): per-tensor norms in each tensor's own dtype, the total over their fp32
        stack, coefficient min(max_norm / (total + 1e-6), 1) — torch's rule for mixed dtypes.  Reads the per-tensor
        squares back (one sync per step); used only by the norm + delta tuning option."""
        if any(o.grad_accum > 1 for o in opts):
            raise _lib.LcvError("joint_clip_grad_norm_: an optimizer with grad_accum > 1 cannot take part in a joint clip")
        total_sq = 0.0
        live = [o for o in opts if any(p.grad is not None for p in o.params)]
        for o in live:
            o.clip_grad_norm_(max_norm)                       # fills o._ws with the per-tensor sums of squares
            n = o._tables["step"][1].n
            sq = o._ws[:n * o.NORM_SLOTS].view(n, o.NORM_SLOTS).sum(1).sqrt()
            if not o.f32:
                sq = sq.to(BF16).to(F32)                      # a bf16 tensor's norm is a bf16 number
            total_sq += float((sq * sq).sum().item())
        total = total_sq ** 0.5
        coef = min(max_norm / (total + 1e-6), 1.0)
        for o in live:
            o._norm_coef[0] = total
            o._norm_coef[1] = coef
        return total

    def step(self):
        self._ema_guard("step()")
        self._sam_guard("step()")
        t = self._step_table()
        self.step_count += 1
        coef = _ptr(self._norm_coef) if self._have_coef else None
        if self.stochastic_rounding:     # descriptors, n_active, total_chunks, coef, hyper..., seed, offset, stream
            seed, offset = ops.draw_philox_offset(self.params[0].device)
            ops.call(self.SR_STEP, _ptr(t.desc), t.n, t.chunks, coef, *self._hyper(), seed & _U64, offset & _U64, _stream())
        else:
            name, sides, param_f32, grad_f32 = self.STEPS[bool(self._anchor), self.moments_8bit, self.grad_accum > 1,
                                                          self.master_weights]
            # descriptors, tables..., n_active, total_chunks, [param_f32], coef, hyper..., [grad_f32], stream
            ops.call(name, _ptr(t.desc), *(_ptr(t.sides[s]) for s in sides), t.n, t.chunks,
                     *((1 if self.f32 else 0,) if param_f32 else ()), coef,
                     *self._hyper(), *((1 if self.grad_accum > 1 else 0,) if grad_f32 else ()), _stream())
        self._have_coef = False
        # the average follows the masters this step left (include/lcv_hip_ema.h); under enable_max_drift() those are the
        # projected ones, so the update is left to the project_max_drift() that must follow: it runs it after its projection,
        # for the optimizers that stepped
        if self.max_drift is not None:
            self._md_stepped = True
        elif self.weight_ema is not None:
            self._ema_update()
        ops.PARAM_EPOCH += 1


class FusedSGDClip(FusedAdamWClip):
    """clip_grad_norm_ + SGD(momentum=0, weight_decay).step over a parameter list in two launches — the default
    optimizer of full-model TTA (lora_experiment/scripts/run_full_tta.py:138-144, 179-180).  No optimizer state, unless
    `master_weights=True` adds the int16 low words of FusedAdamWClip's master-weight form (+2 B / parameter), and with it
    `grad_accum=N` the fp32 accumulators of FusedAdamWClip's accumulation form (+4 B / parameter), or `anchor=[...]` the
    decay toward those base words of FusedAdamWClip's anchor form (nothing allocated); `enable_weight_ema(beta)` keeps the fp32
    average of FusedAdamWClip's form (+4 B / parameter).  `stochastic_rounding=True` (without any of those) is FusedAdamWClip's
    stochastic-rounding form: the fp32 step, a stochastically rounded bf16 store, still no state."""
    SR_STEP = "lcv_sr_sgd_step"
    STEPS = {     # as FusedAdamWClip.STEPS (lcv_hip.h, lcv_hip_master.h, lcv_hip_accum.h, lcv_hip_anchor.h)
        (False, False, False, False): ("lcv_sgd_step", (), True, False),
        (False, False, False, True): ("lcv_master_sgd_step", ("low",), False, False),
        (False, False, True, True): ("lcv_master_sgd_step_g32", ("low",), False, False),
        (True, False, False, True): ("lcv_master_sgd_step_anchor", ("low", "anchor"), False, True),
        (True, False, True, True): ("lcv_master_sgd_step_anchor", ("low", "anchor"), False, True),
    }

    def __init__(self, params, lr=1e-5, weight_decay=0.01, master_weights=False, stochastic_rounding=False, *,
                 grad_accum: int = 1, anchor=None):
        self._init(params, dict(lr=lr, weight_decay=weight_decay), master_weights, False, grad_accum, anchor, stochastic_rounding)

    def _init_moments(self) -> None:
        self.exp_avg = self.params            # the descriptor table has moment slots; SGD never reads them
        self.exp_avg_sq = self.params

    def _hyper(self):
        g = self.param_groups[0]
        return float(g["lr"]), float(g["weight_decay"])

    def moment_tensors(self):
        raise _lib.LcvError("FusedSGDClip: SGD (momentum 0) keeps no moments")

    def state_bytes(self) -> int:
        return 0


# ===================================================================== the trust region over several optimizers
def _max_drift_group(opts, training: bool = False):
    """The optimizers of one ball; `training`: refuse while one of them holds its weight average in the parameters (measuring
    the drift of the average is fine, projecting it is not)."""
    opts = list(opts)
    if not opts:
        raise _lib.LcvError("project_max_drift: no optimizer")
    for o in opts:
        o._md_needs("project_max_drift()")
        if training:
            o._ema_guard("project_max_drift()")
            o._sam_guard("project_max_drift()")
    if len({(o.max_drift, o._md_scope) for o in opts}) != 1:
        raise _lib.LcvError("project_max_drift: every optimizer of one ball takes the same radius and scope")
    return opts


def project_max_drift(opts) -> None:
    """What follows the optimizers' `step()`s under enable_max_drift() (include/lcv_hip_trust.h), with no host sync: every
    optimizer's lcv_trust_sumsq; in global scope the optimizers' totals added on the device in the optimizers' order in fp32 into
    the ball's total, over N = all their elements; every optimizer's lcv_trust_project against it (in tensor scope against its
    own per-tensor sums); the trace slot moves on; then the weight averages of the optimizers that stepped since the last call
    take the projected masters (`_ema_update`, which their `step()` left to this call: with both features on, a `step()` that
    is not followed by this call leaves the average one update behind) and `ops.PARAM_EPOCH` is bumped."""
    opts = _max_drift_group(opts, training=True)
    totals = [o.drift_sumsq() for o in opts]
    numel = sum(o._md_numel for o in opts)
    joint = totals[0]
    if len(opts) > 1 and opts[0]._md_scope == "global":
        joint = totals[0].clone()
        for t in totals[1:]:
            joint += t
    for o, own in zip(opts, totals):
        if o._md_scope == "global":
            o._trust_project(joint, numel)
        else:
            o._trust_project(own, o._md_numel)
    for o in opts:                   # an optimizer that was not stepped (no gradient) keeps its average, as without the ball
        if o.weight_ema is not None and o._md_stepped:
            o._ema_update()
        o._md_stepped = False
    ops.PARAM_EPOCH += 1


def max_drift_norm(opts) -> float:
    """|theta - theta0| over every optimizer of `opts` now (one lcv_trust_sumsq each, then one read per optimizer): the
    `drift_norm` of a result row."""
    opts = _max_drift_group(opts)
    return float(sum(float(o.drift_sumsq().item()) for o in opts)) ** 0.5


def max_drift_stats(opts) -> dict:
    """The `max_drift` entry of a result row from the optimizers' traces (one copy each, after the loop): radius, scope, the
    number of recorded steps, how many of them projected (a coefficient below 1 somewhere), the first such step (counted from 1,
    None when there is none), the smallest coefficient, and per step the drift in RMS per element before the projection."""
    opts = _max_drift_group(opts)
    traces = [o.max_drift_trace().double() for o in opts]
    steps = min(t.shape[0] for t in traces)
    numel = sum(o._md_numel for o in opts)
    if opts[0]._md_scope == "global":       # every optimizer recorded the ball's total
        total = traces[0][:steps, 0]
    else:
        total = sum(t[:steps, 0] for t in traces)
    coef = torch.stack([t[:steps, 1] for t in traces]).min(0).values if steps else torch.ones(0, dtype=torch.float64)
    hit = (coef < 1.0).nonzero().flatten().tolist()
    return {"radius": opts[0].max_drift, "scope": opts[0]._md_scope, "steps": steps, "projections": len(hit),
            "first_projected_step": hit[0] + 1 if hit else None, "min_coef": float(coef.min().item()) if steps else 1.0,
            "drift_rms_trace": (total / numel).sqrt().tolist()}


# ===================================================================== the sharpness-aware step over several optimizers
def _sam_group(opts, what: str):
    """The optimizers of one perturbation: all prepared by enable_sam() with the same rho, form and eta."""
    opts = list(opts)
    if not opts:
        raise _lib.LcvError(f"{what}: no optimizer")
    for o in opts:
        o._sam_needs(f"{what}()")
    if len({(o.sam_rho, o._sam_adaptive, o._sam_eta) for o in opts}) != 1:
        raise _lib.LcvError(f"{what}: every optimizer of one perturbation takes the same rho, adaptive and eta")
    return opts


def sam_perturb(opts) -> None:
    """Between the two backward passes of a sharpness-aware step (include/lcv_hip_sam.h), with no host sync: lcv_sam_sumsq of
    every optimizer that holds a gradient; their totals added on the device in the optimizers' order in fp32 into one norm;
    every such optimizer's lcv_sam_perturb against it, which saves the words the forward reads and stores the perturbed ones;
    the trace slot moves on and `ops.PARAM_EPOCH` is bumped (the kernels write through raw pointers, so `_version` does not
    move; the cached weight copies key on the epoch).  The caller drops the gradients next; the table of what was touched is
    kept for `sam_restore`."""
    opts = _sam_group(opts, "sam_perturb")
    for o in opts:
        o._sam_guard("sam_perturb()")
        o._ema_guard("sam_perturb()")
    live = [o for o in opts if o._sam_measure()]
    if not live:
        raise _lib.LcvError("sam_perturb: no parameter has a gradient")
    joint = live[0]._sam_out[0]
    if len(live) > 1:
        joint = joint.clone()
        for o in live[1:]:
            joint += o._sam_out[0]
    for o in live:
        o._sam_perturb(joint)
    for o in opts:                   # an optimizer without a gradient leaves a row of zeros: the traces stay step-aligned
        o._sam_steps += 1
    ops.PARAM_EPOCH += 1


def sam_restore(opts) -> None:
    """Put back, word for word, exactly the tensors the last `sam_perturb` touched (lcv_sam_restore; their `.grad` may be gone,
    the table was kept) and bump `ops.PARAM_EPOCH`.  Refuses to run without a perturbation, so also twice."""
    opts = _sam_group(opts, "sam_restore")
    live = [o for o in opts if o.sam_perturbed]
    if not live:
        raise _lib.LcvError("sam_restore: the parameters are not perturbed (no sam_perturb() since the last restore)")
    for o in live:
        o._sam_restore()
    ops.PARAM_EPOCH += 1


def sam_stats(opts) -> dict:
    """The `sam` entry of a result row from the optimizers' traces (one copy each, after the loop): rho, adaptive, eta, the
    number of recorded steps, and per step the norm of the (scaled) gradient the perturbation was normalised by and the norm of
    what the stored words really moved by - for bf16 words far below rho, see the header."""
    opts = _sam_group(opts, "sam_stats")
    traces = [o.sam_trace().double() for o in opts]
    steps = min(t.shape[0] for t in traces)
    total = torch.stack([t[:steps, 0] for t in traces]).max(0).values if steps else torch.zeros(0, dtype=torch.float64)
    moved = sum(t[:steps, 1] for t in traces)
    return {"rho": opts[0].sam_rho, "adaptive": opts[0]._sam_adaptive, "eta": opts[0]._sam_eta, "steps": steps,
            "grad_norm_trace": total.sqrt().tolist(), "realized_norm_trace": moved.sqrt().tolist()}

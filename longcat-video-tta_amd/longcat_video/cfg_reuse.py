"""Guidance reuse of the CFG denoise loop (`--cfg-reuse K`, include/lcv_hip_cfgreuse.h).

Every CFG step runs the model at batch 2, and the negative row serves only the guidance correction delta = v - c (v the guided
output before the pipeline's sign, c the prompt row's output), which moves slowly from step to step.  A FULL step is today's
step, after which the correction is stored; a REUSE step runs the prompt row alone at batch 1, forms v^ = c + delta with the
stored correction and hands it to the unguided update.  Nothing is extrapolated or rescaled.

The schedule is static and lives on the host: with j = i - start, step i of a denoise over [start, stop) is full iff
j % K == 0, j < W or i == stop - 1 - so the first step (there is no correction yet), the last step and every K-th step are full.
K = 1 makes every step full: the bits of a run without the feature, plus the drift trace.

Drift: a full step that finds an earlier correction also forms num[b] = sum |new - old| and den[b] = sum |old| per sample, in a
fixed order on the device, into its row of a trace tensor [steps, B, 2].  `stats()` reads the trace back - the one
device-to-host copy the feature adds to a denoise; no step synchronises - and reports max_b num[b] / den[b] per full step, from
which a user with a real checkpoint picks an interval.  None is recommended here: quality is unmeasured.

Inference only, one GPU, no hipGraph replay (the batch changes), not together with a step cache (its buffers are per batch
shape).  A denoise split by `start_step` / `stop_step` restarts the schedule.
"""
import math
from typing import List, Optional


def full_steps(start: int, stop: int, interval: int, warmup: int = 0) -> List[int]:
    """The steps of range(start, stop) that run both rows: every `interval`-th from `start`, the first `warmup`, the last."""
    if int(interval) != interval or interval < 1:
        raise ValueError(f"cfg reuse: the interval must be an integer >= 1, got {interval!r}")
    if int(warmup) != warmup or warmup < 0:
        raise ValueError(f"cfg reuse: the warm-up must be an integer >= 0, got {warmup!r}")
    return [i for i in range(start, stop) if (i - start) % interval == 0 or i - start < warmup or i == stop - 1]


class GuidanceReuse:
    """The stored correction of one denoise: one fp32 buffer shaped like the state and the trace tensor, both allocated at first
    use for a shape and kept over `begin()`.  `backend` offers `cfg_delta_store` / `cfg_delta_apply` (default: lcv_hip.ops)."""

    def __init__(self, interval: int, warmup: int = 0, backend=None):
        full_steps(0, 0, interval, warmup)                        # the refusals
        self.interval = int(interval)
        self.warmup = int(warmup)
        self._backend = backend
        self._delta = self._trace = None
        self._start = self._stop = None
        self._clear()

    # ------------------------------------------------------------------ life cycle
    def _clear(self) -> None:
        self._have_delta = False
        self._full: List[int] = []
        self._reused: List[int] = []
        self._measured: List[int] = []                            # the full steps whose trace row was written

    def begin(self, start: int, stop: int) -> None:
        """Start a denoise over the steps [start, stop): no correction (so its first step is full), empty statistics."""
        if not 0 <= start <= stop:
            raise ValueError(f"cfg reuse: steps {start}..{stop} are no range")
        self._start, self._stop = int(start), int(stop)
        self._clear()

    def reset(self) -> None:
        """`begin()` forgotten, and the buffers are dropped."""
        self._delta = self._trace = None
        self._start = self._stop = None
        self._clear()

    def is_full(self, i: int) -> bool:
        if self._start is None:
            raise RuntimeError("GuidanceReuse.is_full before begin()")
        j = i - self._start
        return j % self.interval == 0 or j < self.warmup or i == self._stop - 1

    # ------------------------------------------------------------------ the device side
    def _ops(self):
        if self._backend is None:
            from lcv_hip import ops
            self._backend = ops
        return self._backend

    def _ensure(self, c) -> None:
        import torch
        if self._delta is None or self._delta.shape != c.shape or self._delta.device != c.device:
            self._delta = torch.empty(c.shape, dtype=torch.float32, device=c.device)
            self._have_delta = False
        steps, B = self._stop - self._start, c.shape[0]
        t = self._trace
        if t is None or t.shape[0] < steps or t.shape[1] != B or t.device != c.device:
            self._trace = torch.zeros((steps, B, 2), dtype=torch.float32, device=c.device)

    def store(self, c, u, guidance: float, zero_star: bool, i: int) -> None:
        """After a full step's update: delta = v - c; with an earlier correction also the step's (num, den) into the trace."""
        if self._start is None:
            raise RuntimeError("GuidanceReuse.store before begin()")
        if not self._start <= i < self._stop:
            raise RuntimeError(f"GuidanceReuse: step {i} is outside {self._start}..{self._stop}")
        self._ensure(c)
        out = self._trace[i - self._start] if self._have_delta else None
        self._ops().cfg_delta_store(c.contiguous(), u.contiguous(), self._delta, guidance, zero_star, out=out)
        if out is not None:
            self._measured.append(i)
        self._have_delta = True
        self._full.append(i)

    def apply(self, c):
        """On a reuse step: v^ = c + delta, written over the model output it came from (a copy when that is not contiguous).
        The step is recorded under the index after the last one seen: a denoise takes its steps in order."""
        if not self._have_delta or self._delta.shape != c.shape:
            raise RuntimeError("GuidanceReuse.apply before any store of this shape: a denoise begins with a full step")
        c = c.contiguous()
        v = self._ops().cfg_delta_apply(c, self._delta, out=c)
        self._reused.append(self._start + len(self._full) + len(self._reused))
        return v

    # ------------------------------------------------------------------ the record
    def stats(self) -> dict:
        """One device-to-host copy of the trace (none when no step measured a drift)."""
        steps = 0 if self._start is None else self._stop - self._start
        distances: List[Optional[float]] = [None] * steps
        if self._measured:
            host = self._trace[:steps].cpu().double()
            for i in self._measured:
                worst = 0.0
                for num, den in host[i - self._start].tolist():
                    d = math.inf if den == 0.0 else num / den
                    if math.isnan(d):
                        worst = d
                        break
                    worst = max(worst, d)
                distances[i - self._start] = worst
        return {"interval": self.interval, "warmup": self.warmup, "full": len(self._full), "reused": len(self._reused),
                "reused_steps": list(self._reused), "distances": distances}

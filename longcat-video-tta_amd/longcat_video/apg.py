"""Adaptive projected guidance of the CFG denoise loop (`--apg`, include/lcv_hip_apg.h).

Plain classifier-free guidance adds g - 1 times the correction d = c - u' to the prompt row's output c (u' the negative row's,
scaled by zero-star when that is on).  At a large scale the part of d parallel to c inflates the magnitude of the guided output:
the over-saturated, drifting result.  Adaptive projected guidance (Sadat et al. 2024) splits d into that part and the part
orthogonal to c and forms

    d = (c - u') + momentum * d_prev          (momentum < 0 damps what the last steps already pushed)
    s = min(1, R sqrt(n) / ||d||)             (`norm_threshold` R: an RMS per element, so one value serves every resolution)
    p = s <d, c> / <c, c> c
    v = c + (g - 1) ((s d - p) + eta p)

with the sums per sample in a fixed order on the device.  eta = 1, no threshold and no momentum is the plain rule in value;
eta = 0 drops the parallel part.  It costs no further forward pass: three launches over the two rows in place of the fused
update's guidance, and the result goes to the unguided update.  None of the three settings is recommended here: quality is
unmeasured.

Every guided step leaves (<d, d>, <d, c>, <c, c>, s) per sample in its row of a trace tensor [steps, B, 4]; `stats()` reads the
trace back - the one device-to-host copy the feature adds to a denoise; no step synchronises.

Inference only, one GPU, not together with guidance reuse (its stored correction is the plain rule's).  A denoise split by
`start_step` / `stop_step` restarts the momentum.
"""
import math
from typing import List, Optional


class ProjectedGuidance:
    """The settings and the state of one denoise: one fp32 buffer shaped like the model output (the momentum, or scratch without
    one) and the trace tensor, both allocated at first use for a shape and kept over `begin()`.  `backend` offers `cfg_apg`
    (default: lcv_hip.ops)."""

    def __init__(self, eta: float = 0.0, norm_threshold: Optional[float] = None, momentum: float = 0.0, backend=None):
        eta, momentum = float(eta), float(momentum)
        if not math.isfinite(eta):
            raise ValueError(f"apg: eta must be a finite number, got {eta!r}")
        if norm_threshold is not None:
            norm_threshold = float(norm_threshold)
            if not (norm_threshold > 0.0 and math.isfinite(norm_threshold)):
                raise ValueError(f"apg: the norm threshold must be a finite number > 0, got {norm_threshold!r}")
        if not -1.0 < momentum < 1.0:                             # a NaN fails too
            raise ValueError(f"apg: the momentum must be in (-1, 1), got {momentum!r}")
        self.eta = eta
        self.norm_threshold = norm_threshold
        self.momentum = momentum
        self._backend = backend
        self._diff = self._trace = None
        self._start = self._stop = None
        self._clear()

    # ------------------------------------------------------------------ life cycle
    def _clear(self) -> None:
        self._have_momentum = False
        self._guided: List[int] = []                              # the steps whose trace row was written

    def begin(self, start: int, stop: int) -> None:
        """Start a denoise over the steps [start, stop): no momentum, empty statistics."""
        if not 0 <= start <= stop:
            raise ValueError(f"apg: steps {start}..{stop} are no range")
        self._start, self._stop = int(start), int(stop)
        self._clear()

    def reset(self) -> None:
        """`begin()` forgotten, and the buffers are dropped."""
        self._diff = self._trace = None
        self._start = self._stop = None
        self._clear()

    # ------------------------------------------------------------------ the device side
    def _ops(self):
        if self._backend is None:
            from lcv_hip import ops
            self._backend = ops
        return self._backend

    def _ensure(self, c) -> None:
        import torch
        if self._diff is None or self._diff.shape != c.shape or self._diff.device != c.device:
            self._diff = torch.empty(c.shape, dtype=torch.float32, device=c.device)
            self._have_momentum = False
        steps, B = self._stop - self._start, c.shape[0]
        t = self._trace
        if t is None or t.shape[0] < steps or t.shape[1] != B or t.device != c.device:
            self._trace = torch.zeros((steps, B, 4), dtype=torch.float32, device=c.device)

    def radius(self, n: int) -> float:
        """The cap on the correction's norm over n elements: R sqrt(n) in double (the call rounds it to fp32 once); 0 = none."""
        return 0.0 if self.norm_threshold is None else self.norm_threshold * math.sqrt(n)

    def guide(self, c, u, guidance: float, zero_star: bool, i: int):
        """The guided output of step i from the prompt row's output c and the negative row's u, written over c (over a copy
        when c is not contiguous) and returned; the step's sums go to its trace row."""
        if self._start is None:
            raise RuntimeError("ProjectedGuidance.guide before begin()")
        if not self._start <= i < self._stop:
            raise RuntimeError(f"ProjectedGuidance: step {i} is outside {self._start}..{self._stop}")
        c = c.contiguous()
        self._ensure(c)
        n = c.numel() // max(c.shape[0], 1)
        v = self._ops().cfg_apg(c, u.contiguous(), self._diff, guidance, self.eta, self.radius(n), self.momentum, zero_star,
                                self._have_momentum, out=self._trace[i - self._start], v=c)
        self._have_momentum = True
        self._guided.append(i)
        return v

    # ------------------------------------------------------------------ the record
    def stats(self) -> dict:
        """One device-to-host copy of the trace (none when no step was guided).  Per step of the denoise (None where the step
        was not guided): `clamp`, the factor s the cap scaled the correction by, the minimum over the samples; `cosine`,
        <d, c> / sqrt(<d, d> <c, c>), the share of the correction along c, the largest in magnitude over the samples (0 where a
        norm is 0)."""
        steps = 0 if self._start is None else self._stop - self._start
        clamp: List[Optional[float]] = [None] * steps
        cosine: List[Optional[float]] = [None] * steps
        if self._guided:
            host = self._trace[:steps].cpu().double()
            for i in self._guided:
                rows = host[i - self._start].tolist()
                clamp[i - self._start] = min(s for _, _, _, s in rows)
                cos = [0.0 if dd * cc == 0.0 else dc / math.sqrt(dd * cc) for dd, dc, cc, _ in rows]
                cosine[i - self._start] = max(cos, key=abs)
        return {"eta": self.eta, "norm_threshold": self.norm_threshold, "momentum": self.momentum, "guided": len(self._guided),
                "clamp": clamp, "cosine": cosine}

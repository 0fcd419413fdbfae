"""First-block step cache of the denoise loop (`--step-cache`, include/lcv_hip_stepcache.h).

A DiT forward with a `StepCache` attached runs block 0, forms its residual r = bf16(x1 - x0) and compares it with p, the
residual of the last COMPUTED step: num[b] = sum |r - p|, den[b] = sum |p| per batch row, skip = all(num[b] < thr * den[b]),
decided on the device in a fixed summation order.  On a skip the forward adds R, the cached residual of blocks 1...L-1
(bf16(xL - x1) of the last computed step), to x1 and goes straight to the final layer; on a compute it runs the blocks, stores
a new R and makes r the new p.  One decision serves both classifier-free-guidance rows.

This class owns the three [B, N, C] bf16 buffers (p, the spare r, R), the small device result with its pinned host mirror, and
the host-side policy: a step is computed regardless of the decision when there is no p (the first step of a `begin()`), when
the caller marks it forced (`denoise` marks its first and its last step), and after `max_consecutive` skips in a row.  Each
step that has a p makes one device-to-host copy of 2 rows + 1 words; that copy is the only synchronisation the cache adds.

There is no default threshold: `threshold=0` never skips and records the distance trace (`stats()["distances"]`), from which
a user with a real checkpoint picks one.  Inference only, one GPU, no hipGraph replay (a captured forward cannot branch).
"""
import math
from typing import List, Optional

import torch

from lcv_hip import ops


class StepCache:
    def __init__(self, threshold: float, max_consecutive: Optional[int] = None):
        threshold = float(threshold)
        if not threshold >= 0.0:                                  # a NaN fails too
            raise ValueError(f"StepCache: the threshold must be >= 0 and not NaN, got {threshold}")
        if max_consecutive is not None:
            if int(max_consecutive) != max_consecutive or max_consecutive < 1:
                raise ValueError(f"StepCache: max_consecutive must be an integer >= 1 or None, got {max_consecutive!r}")
            max_consecutive = int(max_consecutive)
        self.threshold = threshold
        self.max_consecutive = max_consecutive
        self._p = self._r = self._R = None                        # [B, N, C] bf16: last computed residual, spare, blocks 1...L-1
        self._out = self._host = None                             # 2 rows + 1 words on the device, and their pinned mirror
        self.begin()

    # ------------------------------------------------------------------ life cycle
    def begin(self) -> None:
        """Start a denoise call: no p (so its first step is computed), no skips in a row, empty statistics.  Buffers stay."""
        self._have_p = False
        self._run = 0                                             # skips in a row
        self._next = None                                         # (index, forced) for the coming forward
        self._count = 0
        self._computed = 0
        self._skipped_steps: List[int] = []
        self._distances: List[Optional[float]] = []

    def reset(self) -> None:
        """`begin()`, and the buffers are dropped."""
        self._p = self._r = self._R = None
        self._out = self._host = None
        self.begin()

    def set_step(self, index: int, forced: bool = False) -> None:
        """The index the coming forward is recorded under and whether it must be computed.  Without this call a forward takes
        the next index and is not forced."""
        self._next = (int(index), bool(forced))

    def stats(self) -> dict:
        return {"threshold": self.threshold, "max_consecutive": self.max_consecutive, "computed": self._computed,
                "skipped": len(self._skipped_steps), "skipped_steps": list(self._skipped_steps),
                "distances": list(self._distances)}

    # ------------------------------------------------------------------ the device side
    def _ensure(self, x: torch.Tensor) -> None:
        if self._p is not None and self._p.shape == x.shape and self._p.device == x.device:
            return
        rows = x.shape[0]
        self._p, self._r, self._R = (torch.empty_like(x) for _ in range(3))
        self._out = torch.zeros(2 * rows + 1, dtype=torch.float32, device=x.device)
        self._host = torch.zeros(2 * rows + 1, dtype=torch.float32).pin_memory()
        self._have_p = False

    def _measure(self, x0: torch.Tensor, x1: torch.Tensor):
        """r = bf16(x1 - x0) into the spare buffer; with a p also (decision, num, den) read back from the device, else None."""
        self._ensure(x0)
        if not self._have_p:
            ops.stepcache_diff(x0, x1, None, self._r, self.threshold, self._out)
            return None
        ops.stepcache_diff(x0, x1, self._p, self._r, self.threshold, self._out)
        self._host.copy_(self._out, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        rows = x0.shape[0]
        words = self._host.numpy()
        return int(words.view("int32")[2 * rows]), [float(v) for v in words[:rows]], [float(v) for v in words[rows:2 * rows]]

    def _keep_residual(self) -> None:
        self._p, self._r = self._r, self._p                       # p <- r: a pointer swap
        self._have_p = True

    # ------------------------------------------------------------------ what the forward calls
    @staticmethod
    def _distance(num, den) -> float:
        """max over the rows of num / den in double; inf where a den is zero."""
        worst = 0.0
        for a, b in zip(num, den):
            d = math.inf if b == 0.0 else a / b
            if math.isnan(d):
                return d
            worst = max(worst, d)
        return worst

    def should_skip(self, x0: torch.Tensor, x1: torch.Tensor) -> bool:
        """After block 0: True when the forward is to add the cached residual instead of running blocks 1...L-1 (then call
        `apply`), False when it is to run them (then call `store`)."""
        index, forced = self._next if self._next is not None else (self._count, False)
        self._next = None
        self._count = index + 1
        measured = self._measure(x0, x1)
        if measured is None:
            decision = 0
            self._distances.append(None)
        else:
            decision, num, den = measured
            self._distances.append(self._distance(num, den))
        capped = self.max_consecutive is not None and self._run >= self.max_consecutive
        if decision == 1 and not forced and not capped:
            self._run += 1
            self._skipped_steps.append(index)
            return True
        self._run = 0
        self._computed += 1
        self._keep_residual()
        return False

    def store(self, xL: torch.Tensor, x1: torch.Tensor) -> None:
        """On a compute: R = bf16(xL - x1)."""
        ops.stepcache_store(xL, x1, self._R)

    def apply(self, x1: torch.Tensor) -> torch.Tensor:
        """On a skip: bf16(x1 + R) in a tensor of its own (x1 may be held by a hook on block 0)."""
        return ops.stepcache_apply(x1, self._R)

"""Second-order multistep solvers for the denoise loop (`--solver {euler,ab2,ab2c}`, include/lcv_hip_solver.h).

The loop integrates dx/dsigma = f(x, sigma) over the scheduler's host grid sigma_0 ... sigma_N (sigma_N = 0), h_i = sigma_{i+1} -
sigma_i, f_i the guided velocity with the pipeline's sign, evaluated at step i on the state the loop holds.  Euler's global error
falls like 1/N.  The two rules here reuse velocities the loop has already computed - no further forward of the model, no
synchronise - and fall like 1/N^2:

`ab2`   two-step Adams-Bashforth on the non-uniform grid.  The first step of a `denoise` call (j = i - start = 0) is Euler's,
        x += h_i f_i; after it x += a_i f_i + b_i f_{i-1} with a_i = h_i + h_i^2 / (2 h_{i-1}), b_i = -h_i^2 / (2 h_{i-1}), the
        integrals over [sigma_i, sigma_{i+1}] of the Lagrange basis through sigma_i and sigma_{i-1} (3h/2, -h/2 on a uniform grid).
`ab2c`  the same predictor with a trapezoid corrector that reuses the next step's evaluation: with (P_i0, P_i1) the predictor
        weights of step i ((h_i, 0) at j = 0, (a_i, b_i) after), step j >= 1 undoes the predictor of the previous interval,
        applies the trapezoid rule to it with the evaluation just made, and predicts the next interval, folded into one update
        x += w0 f_i + w1 f_{i-1} + w2 f_{i-2}:  w0 = P_i0 + h_{i-1}/2,  w1 = P_i1 + h_{i-1}/2 - P_{i-1,0},  w2 = -P_{i-1,1}.
        At j = 1 w2 is zero and two terms are passed; on a uniform grid from j = 2 the weights are 2h, -3h/2, h/2; they always
        sum to h_i.  The last interval is not corrected: no evaluation follows it.

All weights are formed here in float64 from the host grid and cast to fp32 once, at the call.  History restarts at every `denoise`
call, so a denoise split in two by `start_step` / `stop_step` is not bit-equal to one call under either rule.
"""
from typing import Optional, Sequence, Tuple

SOLVERS = ("euler", "ab2", "ab2c")
_HISTORY = {"ab2": 2, "ab2c": 3}       # ring buffers: the velocity being written and the one / two before it


def _predictor(sig: Sequence[float], i: int, start: int) -> Tuple[float, float]:
    h = float(sig[i + 1]) - float(sig[i])
    if i == start:
        return h, 0.0
    hp = float(sig[i]) - float(sig[i - 1])
    b = -(h * h) / (2.0 * hp)
    return h - b, b


def solver_weights(sigmas_host: Sequence[float], i: int, start: int, kind: str) -> Tuple[float, ...]:
    """The 1 to 3 float64 weights of step `i` of a denoise that began at step `start`, newest velocity first."""
    if kind not in SOLVERS:
        raise ValueError(f"unknown solver {kind!r}: one of {', '.join(SOLVERS)}")
    if not 0 <= start <= i < len(sigmas_host) - 1:
        raise ValueError(f"step {i} (start {start}) is outside a grid of {len(sigmas_host) - 1} intervals")
    if kind == "euler" or i == start:
        return (float(sigmas_host[i + 1]) - float(sigmas_host[i]),)
    p0, p1 = _predictor(sigmas_host, i, start)
    if kind == "ab2":
        return p0, p1
    hp = float(sigmas_host[i]) - float(sigmas_host[i - 1])
    q0, q1 = _predictor(sigmas_host, i - 1, start)
    w = (p0 + hp / 2.0, p1 + hp / 2.0 - q0)
    return w if i - 1 == start else w + (-q1,)


class MultistepSolver:
    """The velocity history of one denoise: a ring of fp32 buffers shaped like the state (two for `ab2`, three for `ab2c`),
    allocated at first use for a shape and rotated by reference, never copied.  `begin(start_step)` forgets the history;
    `step(...)` forms the guided velocity, keeps it and updates `x` in place (one call of lcv_cfg_lms_step)."""

    def __init__(self, kind: str):
        if kind not in _HISTORY:
            raise ValueError(f"MultistepSolver: kind must be one of {', '.join(_HISTORY)}, got {kind!r}")
        self.kind = kind
        self._ring = None
        self._start = None
        self._next = None

    def begin(self, start_step: int = 0) -> None:
        self._start = self._next = int(start_step)

    def reset(self) -> None:
        self._ring = None
        self._start = self._next = None

    def step(self, cond, uncond: Optional["torch.Tensor"], x, i: int, sigmas_host: Sequence[float], guidance: float,
             negate: bool, zero_star: bool) -> None:
        import torch
        from lcv_hip import ops
        if self._start is None:
            raise RuntimeError("MultistepSolver.step before begin()")
        if i != self._next:
            raise RuntimeError(f"MultistepSolver: step {i} after step {self._next - 1}; the history holds consecutive steps only")
        ring = self._ring
        if ring is None or ring[0].shape != x.shape or ring[0].device != x.device:
            ring = self._ring = [torch.empty(x.shape, dtype=torch.float32, device=x.device) for _ in range(_HISTORY[self.kind])]
        w = solver_weights(sigmas_host, i, self._start, self.kind)
        ops.cfg_lms_step(cond, uncond, x, ring[0], ring[1] if len(w) >= 2 else None, ring[2] if len(w) >= 3 else None,
                         guidance, w, negate=negate, zero_star=zero_star)
        self._ring = ring[-1:] + ring[:-1]             # the oldest buffer is the next step's f0; the one just written its f1
        self._next = i + 1

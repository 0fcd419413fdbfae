"""numpy restatement of include/lcv_hip_cfgreuse.h and of the schedule of longcat_video/cfg_reuse.py.  A helper, not a test module.

`delta_store` / `delta_apply` take the two element sequences one rounded fp32 operation at a time.  `drift_partials` / `drift_join`
restate the fixed-order drift sums (256 partial pairs per sample, the butterfly inside a wave, the waves in wave order) with the
summation helpers of tests/solver_ref.py; the zero-star partials and their join are that module's `partials` / `join` (the scheme
is the same, so `st` has the bits lcv_cfg_lms_step forms).  `full_steps` restates the schedule from the issue's definition,
independently of the package's code.
"""
import numpy as np

import solver_ref as S

F = np.float32
PARTS, THREADS = S.PARTS, S.THREADS


def full_steps(start, stop, K, W=0):
    return [i for i in range(start, stop) if (i - start) % K == 0 or (i - start) < W or i == stop - 1]


def delta_store(cond, uncond, guidance, st=None):
    """[B, n] fp32 -> delta [B, n]: u' = u * st (st [B] fp32 or None); d = c - u'; t = g * d; v = u' + t; e = v - c."""
    c, u = np.asarray(cond, F), np.asarray(uncond, F)
    if st is not None:
        u = (u * np.asarray(st, F)[:, None]).astype(F)
    d = (c - u).astype(F)
    t = (F(guidance) * d).astype(F)
    v = (u + t).astype(F)
    return (v - c).astype(F)


def delta_apply(cond, delta):
    return (np.asarray(cond, F) + np.asarray(delta, F)).astype(F)


def drift_terms(e, o):
    """The two summands per element: a = |e - o| (the difference rounded to fp32 first), m = |o|."""
    e, o = np.asarray(e, F), np.asarray(o, F)
    return np.abs((e - o).astype(F)), np.abs(o)


def drift_partials(e, o):
    """e (the new delta), o (the old) [B, n] fp32 -> ws [B, 256, 2] fp32 (num, den) with the store launch's bits: thread t of
    part p takes p*256 + t + k*65536 in index order; a thread past the end adds nothing."""
    a, m = drift_terms(e, o)
    B, n = a.shape
    span = PARTS * THREADS
    trips = (n + span - 1) // span
    ap = np.zeros((B, trips * span), F); ap[:, :n] = a
    mp = np.zeros((B, trips * span), F); mp[:, :n] = m
    ap, mp = ap.reshape(B, trips, PARTS, THREADS), mp.reshape(B, trips, PARTS, THREADS)
    live = (np.arange(trips * span) < n).reshape(trips, PARTS, THREADS)
    num = np.zeros((B, PARTS, THREADS), F)
    den = np.zeros((B, PARTS, THREADS), F)
    for k in range(trips):
        num = np.where(live[k], (num + ap[:, k]).astype(F), num)
        den = np.where(live[k], (den + mp[:, k]).astype(F), den)
    return np.stack([S._workgroup_sum(num), S._workgroup_sum(den)], axis=-1)


def drift_join(ws):
    """ws [B, 256, 2] fp32 -> out [B, 2] fp32 as the last launch forms it."""
    ws = np.asarray(ws, F)
    return np.stack([S._workgroup_sum(ws[..., 0]), S._workgroup_sum(ws[..., 1])], axis=-1)


def distance(out):
    """out [B, 2] -> max_b num / den in double; inf where a den is zero."""
    worst = 0.0
    for num, den in np.asarray(out, np.float64):
        worst = max(worst, float("inf") if den == 0.0 else num / den)
    return worst

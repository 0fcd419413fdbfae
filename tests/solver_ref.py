"""numpy restatement of include/lcv_hip_solver.h and of the weights of longcat_video/solver.py.  A helper, not a test module.

`lms_step` takes the element sequence one rounded fp32 operation at a time.  `partials` / `join` restate the fixed-order
zero-star sums (256 partial pairs per sample, the butterfly inside a wave, the waves in wave order) so that `st` has the
kernel's bits; `st_f64` is the float64 form the sums are bounded against.  `weights` restates the rules from the issue's
definition, independently of the package's code.
"""
import numpy as np

F = np.float32
PARTS, THREADS, WAVE = 256, 256, 64


# ------------------------------------------------------------------------------------------------------------ the weights
def _pred(sig, i, start):
    h = sig[i + 1] - sig[i]
    if i == start:
        return h, 0.0
    hp = sig[i] - sig[i - 1]
    return h + h * h / (2 * hp), -h * h / (2 * hp)


def weights(sig, i, start, kind):
    """float64 weights of step i, newest velocity first."""
    h = sig[i + 1] - sig[i]
    if kind == "euler" or i == start:
        return (h,)
    p0, p1 = _pred(sig, i, start)
    if kind == "ab2":
        return (p0, p1)
    assert kind == "ab2c"
    hp = sig[i] - sig[i - 1]
    q0, q1 = _pred(sig, i - 1, start)
    w = (p0 + hp / 2, p1 + hp / 2 - q0, -q1)
    return w[:2] if i - 1 == start else w


# ------------------------------------------------------------------------------------------------------------ the sums
def _butterfly(v):
    """[..., 64] fp32 -> the value every lane holds after v = v + v[lane ^ o], o = 32 ... 1."""
    lane = np.arange(WAVE)
    for o in (32, 16, 8, 4, 2, 1):
        v = (v + v[..., lane ^ o]).astype(F)
    return v[..., 0]


def _workgroup_sum(v):
    """[..., 256] fp32 per-thread values -> the workgroup's sum: butterfly per wave, then ((s0 + s1) + s2) + s3."""
    s = _butterfly(v.reshape(v.shape[:-1] + (THREADS // WAVE, WAVE)))
    return (((s[..., 0] + s[..., 1]).astype(F) + s[..., 2]).astype(F) + s[..., 3]).astype(F)


def partials(c, u):
    """c, u [B, n] fp32 -> ws [B, 256, 2] fp32 with the first launch's bits: thread t of part p takes p*256 + t + k*65536."""
    c, u = np.asarray(c, F), np.asarray(u, F)
    B, n = c.shape
    span = PARTS * THREADS
    trips = (n + span - 1) // span
    cp = np.zeros((B, trips * span), F); cp[:, :n] = c
    up = np.zeros((B, trips * span), F); up[:, :n] = u
    cp, up = cp.reshape(B, trips, PARTS, THREADS), up.reshape(B, trips, PARTS, THREADS)
    live = (np.arange(trips * span) < n).reshape(trips, PARTS, THREADS)
    dot = np.zeros((B, PARTS, THREADS), F)
    nrm = np.zeros((B, PARTS, THREADS), F)
    for k in range(trips):
        p = (cp[:, k] * up[:, k]).astype(F)
        q = (up[:, k] * up[:, k]).astype(F)
        dot = np.where(live[k], (dot + p).astype(F), dot)       # a thread past the end adds nothing (not even a +0)
        nrm = np.where(live[k], (nrm + q).astype(F), nrm)
    return np.stack([_workgroup_sum(dot), _workgroup_sum(nrm)], axis=-1)


def join(ws):
    """ws [B, 256, 2] fp32 -> st [B] fp32 as every workgroup of the step launch forms it."""
    ws = np.asarray(ws, F)
    dot, nrm = _workgroup_sum(ws[..., 0]), _workgroup_sum(ws[..., 1])
    return (dot / (nrm + F(1e-8)).astype(F)).astype(F)


def sums_f64(c, u):
    """float64 (<c,u>, <u,u>, sum |c u|) per sample."""
    c, u = np.asarray(c, np.float64), np.asarray(u, np.float64)
    return (c * u).sum(1), (u * u).sum(1), np.abs(c * u).sum(1)


def st_f64(c, u):
    dot, nrm, _ = sums_f64(c, u)
    return dot / (nrm + 1e-8)


# ------------------------------------------------------------------------------------------------------------ the step
def lms_step(cond, uncond, x, hist, guidance, w, negate, st=None):
    """One step on [B, n] fp32 arrays: returns (x_new, f0).  `hist` = (f1, f2) (entries past len(w) - 1 are not read), `w` the
    1 to 3 weights (any float: cast to fp32 once), `st` [B] fp32 or None for no zero-star, `uncond` None for no guidance."""
    c = np.asarray(cond, F)
    w = [F(v) for v in w]
    if uncond is not None:
        u = np.asarray(uncond, F)
        if st is not None:
            u = (u * np.asarray(st, F)[:, None]).astype(F)
        d = (c - u).astype(F)
        t = (F(guidance) * d).astype(F)
        v = (u + t).astype(F)
    else:
        v = c
    f = (-v if negate else v).astype(F)
    a = (w[0] * f).astype(F)
    for k in range(1, len(w)):
        p = (w[k] * np.asarray(hist[k - 1], F)).astype(F)
        a = (a + p).astype(F)
    return (np.asarray(x, F) + a).astype(F), f


def integrate(kind, sig, x0, field, start=0, stop=None):
    """Drive `lms_step` over the grid in fp32: field(x, sigma_i) -> dx/dsigma (no guidance, no negation)."""
    x = np.asarray(x0, F).reshape(1, -1)
    hist = []
    for i in range(start, len(sig) - 1 if stop is None else stop):
        w = weights(sig, i, start, kind)
        x, f = lms_step(np.asarray(field(x, sig[i]), F), None, x, hist, 1.0, w, False)
        hist = [f] + hist[:1]
    return x[0]

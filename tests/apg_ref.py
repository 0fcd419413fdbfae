"""numpy restatement of include/lcv_hip_apg.h.  A helper, not a test module.

`correction` / `guided` take the two element sequences one rounded fp32 operation at a time; `sum_partials` / `sum_join` restate
the fixed-order sums of the correction (256 partial triples per sample, the butterfly inside a wave, the waves in wave order)
with the summation helpers of tests/solver_ref.py, which tests/cfgreuse_ref.py shares; the zero-star partials and their join
are that module's `partials` / `join` (the scheme is the same, so `st` has the bits lcv_cfg_delta_store forms).  `apg` is one
call of lcv_cfg_apg; `apg_f64` / `plain_f64` are the same mathematics and the plain rule in float64.
"""
import numpy as np

import cfgreuse_ref as G
import solver_ref as S

F = np.float32
PARTS, THREADS = G.PARTS, G.THREADS


def correction(cond, uncond, old=None, beta=0.0, st=None):
    """[B, n] fp32 -> d [B, n]: u' = u * st (st [B] fp32 or None); d = c - u'; with `old` and beta != 0: m = beta * old; d = d + m."""
    c, u = np.asarray(cond, F), np.asarray(uncond, F)
    if st is not None:
        u = (u * np.asarray(st, F)[:, None]).astype(F)
    d = (c - u).astype(F)
    if old is not None and F(beta) != 0:
        m = (F(beta) * np.asarray(old, F)).astype(F)
        d = (d + m).astype(F)
    return d


def _thread_sums(terms):
    """terms [B, n] fp32 -> [B, 256, 256]: thread t of part p adds p*256 + t + k*65536 in index order, from 0; a thread past the
    end adds nothing."""
    B, n = terms.shape
    span = PARTS * THREADS
    trips = (n + span - 1) // span
    tp = np.zeros((B, trips * span), F); tp[:, :n] = terms
    tp = tp.reshape(B, trips, PARTS, THREADS)
    live = (np.arange(trips * span) < n).reshape(trips, PARTS, THREADS)
    acc = np.zeros((B, PARTS, THREADS), F)
    for k in range(trips):
        acc = np.where(live[k], (acc + tp[:, k]).astype(F), acc)
    return acc


def sum_partials(d, cond):
    """d, c [B, n] fp32 -> ws[1] [B, 256, 4] fp32 = (dd, dc, cc, 0) per part, every product rounded before its sum."""
    d, c = np.asarray(d, F), np.asarray(cond, F)
    cols = [S._workgroup_sum(_thread_sums((a * b).astype(F))) for a, b in ((d, d), (d, c), (c, c))]
    return np.stack(cols + [np.zeros_like(cols[0])], axis=-1)


def sum_join(ws):
    """ws[1] [B, 256, 4] fp32 -> (dd, dc, cc), each [B] fp32, as every workgroup of the last launch forms them."""
    ws = np.asarray(ws, F)
    return tuple(S._workgroup_sum(ws[..., k]) for k in range(3))


def star_partials(cond, uncond):
    """ws[0] [B, 256, 4] fp32 = (dot, nrm, 0, 0) per part."""
    pairs = S.partials(cond, uncond)
    return np.concatenate([pairs, np.zeros_like(pairs)], axis=-1)


def clamp(dd, radius):
    """s [B] fp32: 1 when radius <= 0 or dd == 0, otherwise min(1, radius / sqrt(dd)), each operation rounded."""
    dd = np.asarray(dd, F)
    s = np.ones_like(dd)
    if F(radius) > 0:
        live = dd != 0
        with np.errstate(divide="ignore", invalid="ignore"):
            q = (F(radius) / np.sqrt(dd).astype(F)).astype(F)
        s = np.where(live & (q < 1), q, s).astype(F)
    return s


def guided(cond, d, dd, dc, cc, s, guidance, eta):
    """v [B, n] fp32 from the correction and its joined sums: k = dc / (cc + 1e-8); ds = s d; p = k c; p = s p; o = ds - p;
    e = eta p; w = o + e; t = gm1 w; v = c + t, with gm1 = guidance - 1 in fp32."""
    c, d = np.asarray(cond, F), np.asarray(d, F)
    s = np.asarray(s, F)[:, None]
    k = (np.asarray(dc, F) / (np.asarray(cc, F) + F(1e-8)).astype(F)).astype(F)[:, None]
    gm1 = F(F(guidance) - F(1))
    ds = (s * d).astype(F)
    p = (k * c).astype(F)
    p = (s * p).astype(F)
    o = (ds - p).astype(F)
    e = (F(eta) * p).astype(F)
    w = (o + e).astype(F)
    t = (gm1 * w).astype(F)
    return (c + t).astype(F)


def apg(cond, uncond, old, guidance, eta, radius, beta, zero_star):
    """One lcv_cfg_apg on [B, n] fp32 arrays (`old` None: no momentum yet; radius 0 or None: no cap) ->
    dict(v, diff, ws0 (None without zero-star), ws1, out [B, 4], st)."""
    ws0 = star_partials(cond, uncond) if zero_star else None
    st = S.join(ws0[..., :2]) if zero_star else None
    d = correction(cond, uncond, old, beta, st)
    ws1 = sum_partials(d, cond)
    dd, dc, cc = sum_join(ws1)
    s = clamp(dd, radius or 0.0)
    v = guided(cond, d, dd, dc, cc, s, guidance, eta)
    return {"v": v, "diff": d, "ws0": ws0, "ws1": ws1, "out": np.stack([dd, dc, cc, s], axis=-1), "st": st}


# ------------------------------------------------------------------------------------------------------------ float64
def _star_f64(c, u, zero_star):
    return u * S.st_f64(c, u)[:, None] if zero_star else u


def apg_f64(cond, uncond, old, guidance, eta, radius, beta, zero_star):
    """The same mathematics in float64 (inputs as given; guidance, eta, radius, beta as Python floats) -> (v, d, s)."""
    c, u = np.asarray(cond, np.float64), np.asarray(uncond, np.float64)
    d = c - _star_f64(c, u, zero_star)
    if old is not None:
        d = d + beta * np.asarray(old, np.float64)
    dd, dc, cc = (d * d).sum(1), (d * c).sum(1), (c * c).sum(1)
    s = np.ones_like(dd)
    if radius and radius > 0:
        with np.errstate(divide="ignore"):
            s = np.where(dd != 0, np.minimum(1.0, radius / np.sqrt(dd)), 1.0)
    p = (s * dc / (cc + 1e-8))[:, None] * c
    v = c + (guidance - 1.0) * ((s[:, None] * d - p) + eta * p)
    return v, d, s


def plain_f64(cond, uncond, guidance, zero_star):
    """The plain rule v = u' + g (c - u') in float64."""
    c, u = np.asarray(cond, np.float64), np.asarray(uncond, np.float64)
    u = _star_f64(c, u, zero_star)
    return u + guidance * (c - u)


def plain_f32(cond, uncond, guidance, zero_star):
    """The plain rule one rounded fp32 operation at a time: cfgreuse_ref's delta_store without its last subtraction."""
    c, u = np.asarray(cond, F), np.asarray(uncond, F)
    if zero_star:
        u = (u * S.join(S.partials(c, u))[:, None]).astype(F)
    d = (c - u).astype(F)
    t = (F(guidance) * d).astype(F)
    return (u + t).astype(F)

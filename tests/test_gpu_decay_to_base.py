"""GPU: decay toward the base weights and the drift norm (include/lcv_hip_anchor.h, `anchor=` / `decay_to_base` /
`--decay-to-base`).

1. The three anchor steps through the optimizers against the numpy restatement (tests/anchor_ref.py), bit for bit on the bf16
   words, the low words and both moments (or codes and scales) after optimizer steps 1 and 3 of three: bf16 gradients, the fp32
   accumulators of grad_accum=3, 8-bit moments; with and without clip; wd in {0, 0.01, 0.5}.  Tensors: a single element, a
   sub-packet tail, one 512-block, one element past it, an exact chunk, one element past a chunk (parameter, low words,
   gradient, anchor and codes as 2-byte / 1-byte offset views: the scalar path), a tail past two chunks, plus a parameter
   without a gradient.  And, at the C ABI, one 2059-element tensor with exactly one array at a time as an offset view, against
   the all-aligned run: SGD, AdamW and 8-bit AdamW, with and without an anchor, bf16 and fp32 gradients.
2. Pins to the existing kernels: zero base words give lcv_master_sgd_step's bits, wd = 0 gives the AdamW steps' bits.
3. The base is a fixed point, the pull a contraction.
4. lcv_master_drift_sumsq: a derived error bound against float64, run-to-run bits, low = NULL, zero at the base; refusals.
5. The loops and the runners.
"""
import importlib.util
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import anchor_ref as A
import grad_accum_ref as G
import master_weights_ref as W
import moments8_ref as M8

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
PKG = ROOT / "longcat-video-tta_amd"
BF16 = torch.bfloat16
DEV = "cuda"
NUMELS = (1, 7, 512, 513, 2048, 2049, 4099)
VIEW = 5                      # the 2049-element tensor: every array of it is a [1:] view
IDLE = 300                    # an eighth parameter that never gets a gradient
N_MICRO = 3
CHUNK = 2048
LR = {"sgd": 2e-3, "adamw": 1e-3, "adamw8": 1e-3}
B1, B2, EPS = 0.9, 0.999, 1e-8


# ---------------------------------------------------------------------------------------------------------- helpers
def _bf16_dev(h):
    return torch.from_numpy(np.ascontiguousarray(h).view(np.int16).copy()).view(BF16).to(DEV)


def _i16_dev(low):
    return torch.from_numpy(np.ascontiguousarray(low, dtype=np.int16).copy()).to(DEV)


def _h_of(t):
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _bits_of(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy().view(np.uint32).ravel()


def _offset_view(t):
    """The same values in storage that starts one element late: a contiguous view whose pointer is not 16-byte aligned."""
    base = torch.zeros(t.numel() + 1, dtype=t.dtype, device=t.device)
    base[1:].copy_(t.reshape(-1))
    v = base[1:].view(t.shape)
    assert v.data_ptr() % 16 == t.element_size() and v.is_contiguous()
    return v


def _call(name, *args):
    from lcv_hip import lib
    lib.call(name, *args, torch.cuda.current_stream().cuda_stream)


def _report(what, k, got, want):
    got, want = np.asarray(got).ravel(), np.asarray(want).ravel()
    bad = np.flatnonzero(got != want)
    if bad.size:
        i = int(bad[0])
        raise AssertionError(f"{what}: tensor {k} (numel {got.size}) index {i}: got {got[i]!r} want {want[i]!r}; "
                             f"{bad.size} mismatches")


_TABLE = {}


def _table():
    """Host-generated inputs, made once and never written: |w| in [2^-10, 2], |g| in [2^-20, 8], both signs; base words
    bf16(w (1 + delta)), |delta| in [2^-12, 2^-4], every 5th element at its base (h0 = h, l = 0)."""
    if not _TABLE:
        rng = np.random.default_rng(43)
        ws = [W.weights(rng, n) for n in NUMELS + (IDLE,)]
        _TABLE["w"], _TABLE["h0"] = [], []
        for h, low in ws:
            h0, low = A.anchors(rng, h, low)
            _TABLE["w"].append((h, low))
            _TABLE["h0"].append(h0)
        _TABLE["g"] = [[[W.grads(rng, n) for n in NUMELS] for _ in range(N_MICRO)] for _ in range(3)]
        assert any((W.master(h, low) == W.bf16_to_f32(h0)).any() and (W.master(h, low) != W.bf16_to_f32(h0)).any()
                   for (h, low), h0 in zip(_TABLE["w"], _TABLE["h0"]))
    return _TABLE


def _make(kind, wd, n=1, anchor="table", words="table", lr=None, master=True):
    """An optimizer over the table's tensors.  anchor: "table", "zero" (all-zero base words) or None (the plain form);
    words: "table" or "base" (every master at its base)."""
    from lcv_hip import ops
    t = _table()
    params, anchors = [], []
    for k, (h, _) in enumerate(t["w"]):
        p = _bf16_dev(t["h0"][k] if words == "base" else h)
        a = _bf16_dev(np.zeros_like(t["h0"][k]) if anchor == "zero" else t["h0"][k])
        params.append(_offset_view(p) if k == VIEW else p)
        anchors.append(_offset_view(a) if k == VIEW else a)
    kw = dict(weight_decay=wd, master_weights=master, grad_accum=n, anchor=None if anchor is None else anchors)
    lr = LR[kind] if lr is None else lr
    if kind == "sgd":
        opt = ops.FusedSGDClip(params, lr=lr, **kw)
    else:
        opt = ops.FusedAdamWClip(params, lr=lr, betas=(B1, B2), eps=EPS, moments_8bit=kind == "adamw8", **kw)
    if master:
        opt._low[VIEW] = _offset_view(opt._low[VIEW])                 # before the first step builds the table
        if words == "table":
            for lw, (_, low) in zip(opt.low_words, t["w"]):
                lw.copy_(_i16_dev(low))
    if kind == "adamw8":
        opt.exp_avg[VIEW] = _offset_view(opt.exp_avg[VIEW])
        opt.exp_avg_sq[VIEW] = _offset_view(opt.exp_avg_sq[VIEW])
    if anchor is not None:
        assert all(a is b for a, b in zip(opt._anchor, anchors))      # held by reference, not copied
    return opt, params


def _give_grads(params, gs):
    for k in range(len(NUMELS)):
        g = _bf16_dev(gs[k])
        params[k].grad = _offset_view(g) if k == VIEW else g


def _zero_grads(params):
    for k in range(len(NUMELS)):
        g = torch.zeros_like(params[k])
        params[k].grad = _offset_view(g) if k == VIEW else g


def _feed(opt, params, step, n):
    """One optimizer step's gradients: `.grad`s at n = 1, n accumulated micro-steps otherwise.  Returns what the restatement
    reads as the gradient of each tensor."""
    t = _table()
    if n == 1:
        _give_grads(params, t["g"][step][0])
        return t["g"][step][0]
    opt.zero_grad()
    acc = [np.zeros(m, dtype=np.float32) for m in NUMELS]
    for micro in range(n):
        _give_grads(params, t["g"][step][micro])
        opt.accumulate()
        acc = [G.accumulate(a, g, 1.0 / n) for a, g in zip(acc, t["g"][step][micro])]
    return acc


def _state(opt, kind, k):
    if kind == "adamw":
        return [_bits_of(opt.exp_avg[k]), _bits_of(opt.exp_avg_sq[k])]
    if kind == "adamw8":
        return [opt.exp_avg[k].cpu().numpy().ravel(), opt.exp_avg_sq[k].cpu().numpy().ravel(), _bits_of(opt._scales[k])]
    return []


# ---------------------------------------------------------------------------------------------------------- 1. the steps
def _run_steps(kind, n, clip, wd):
    opt, params = _make(kind, wd, n)
    t = _table()
    ref = [dict(h=h.copy(), l=low.copy(), m=np.zeros(h.size, np.float32), v=np.zeros(h.size, np.float32),
                st=M8.zero_state(h.size)) for h, low in t["w"][:len(NUMELS)]]
    lr = LR[kind]
    for step in range(3):
        grads = _feed(opt, params, step, n)
        coef = 1.0
        if clip:
            opt.clip_grad_norm_(1.0)
            norm, coef = (float(x) for x in opt._norm_coef.tolist())
            assert 0.0 < coef < 1.0 and norm > 1.0            # the gradients are large: the coefficient is live
        opt.step()
        torch.cuda.synchronize()
        for k, r in enumerate(ref):
            if kind == "sgd":
                r["h"], r["l"] = A.sgd_step_anchor(r["h"], r["l"], t["h0"][k], grads[k], coef, lr, wd, grad_f32=n > 1)
            elif kind == "adamw":
                r["h"], r["l"], r["m"], r["v"] = A.adamw_step_anchor(r["h"], r["l"], t["h0"][k], r["m"], r["v"], grads[k], coef, lr,
                                                                     B1, B2, EPS, wd, step + 1, grad_f32=n > 1)
            else:
                r["h"], r["l"], *st = A.adamw8_step_anchor(r["h"], r["l"], t["h0"][k], *r["st"], grads[k], coef, lr, B1, B2, EPS,
                                                           wd, step + 1)
                r["st"] = tuple(st)
        if step in (0, 2):
            for k, r in enumerate(ref):
                what = f"{kind} n={n} clip={clip} wd={wd} step {step + 1}"
                _report(what + " h", k, _h_of(params[k]), r["h"])
                _report(what + " l", k, opt.low_words[k].cpu().numpy(), r["l"])
                want = {"sgd": [], "adamw": [W.bits(r["m"]), W.bits(r["v"])],
                        "adamw8": [r["st"][0], r["st"][1], W.bits(r["st"][2])]}[kind]
                for j, (got, w) in enumerate(zip(_state(opt, kind, k), want)):
                    _report(what + f" state {j}", k, got, w)
    # the parameter without a gradient and every base word are what they were
    h, low = t["w"][-1]
    assert np.array_equal(_h_of(params[-1]), h) and np.array_equal(opt.low_words[-1].cpu().numpy(), low)
    assert all(np.array_equal(_h_of(a), h0) for a, h0 in zip(opt._anchor, t["h0"]))
    assert sum(int((r["h"] != w[0]).sum()) for r, w in zip(ref, t["w"])) > 0


@pytest.mark.parametrize("wd", [0.0, 0.01, 0.5])
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("n", [1, N_MICRO])
def test_sgd_anchor_step_bits(n, clip, wd):
    _run_steps("sgd", n, clip, wd)


@pytest.mark.parametrize("wd", [0.0, 0.01, 0.5])
@pytest.mark.parametrize("clip", [False, True])
@pytest.mark.parametrize("n", [1, N_MICRO])
def test_adamw_anchor_step_bits(n, clip, wd):
    _run_steps("adamw", n, clip, wd)


@pytest.mark.parametrize("wd", [0.0, 0.01, 0.5])
@pytest.mark.parametrize("clip", [False, True])
def test_adamw8_anchor_step_bits(clip, wd):
    _run_steps("adamw8", 1, clip, wd)


# ------------------------------------------------------------------------------------- 1b. one misaligned array at a time
ONE = 2059                    # a full chunk, one more whole packet and a 3-element tail
_ONE = {}


def _one():
    """Host-generated arrays of one tensor, made once and never written: live low words, moments and codes."""
    if not _ONE:
        rng = np.random.default_rng(47)
        h, low = W.weights(rng, ONE)
        _ONE["A"], low = A.anchors(rng, h, low)
        _ONE["P"], _ONE["L"] = h, low
        _ONE["G"] = W.grads(rng, ONE)
        _ONE["G32"] = G.accumulate(np.zeros(ONE, dtype=np.float32), _ONE["G"], 1.0 / 3.0)
        _ONE["M"], _ONE["V"] = M8.moments(rng, ONE)
        _ONE["CM"], _ONE["CR"], _ONE["S"] = M8.encode(_ONE["M"], _ONE["V"])
    return _ONE


def _one_step(kind, anchored, g32, offset):
    """One step of the entry point for (kind, anchored, g32) over the one tensor, every array 16-byte aligned but `offset`,
    which starts one element late.  Returns every array the step writes."""
    t = _one()
    dev = {"P": _bf16_dev(t["P"]), "L": _i16_dev(t["L"]), "A": _bf16_dev(t["A"]),
           "G": torch.from_numpy(t["G32"].copy()).to(DEV) if g32 else _bf16_dev(t["G"])}
    if kind == "adamw":
        dev["M"], dev["V"] = (torch.from_numpy(t[k].copy()).to(DEV) for k in ("M", "V"))
    if kind == "adamw8":
        dev["M"], dev["V"] = (torch.from_numpy(t[k].copy()).to(DEV) for k in ("CM", "CR"))
        dev["S"] = torch.from_numpy(t["S"].copy()).to(DEV)
    assert all(x.data_ptr() % 16 == 0 for x in dev.values())
    if offset is not None:
        dev[offset] = _offset_view(dev[offset])
    ptr = lambda k: torch.tensor([dev[k].data_ptr()], dtype=torch.int64).to(DEV)
    moments = [dev[k].data_ptr() if k in dev else 0 for k in ("M", "V")]
    table = torch.tensor([[dev["P"].data_ptr(), dev["G"].data_ptr(), *moments, ONE, 0]], dtype=torch.int64).to(DEV)
    tables = [ptr("L")] + ([ptr("S")] if kind == "adamw8" else []) + ([ptr("A")] if anchored else [])
    hyper = (LR[kind], 0.01) if kind == "sgd" else (LR[kind], B1, B2, EPS, 0.01, 2)
    name = {"sgd": "lcv_master_sgd_step", "adamw": "lcv_master_adamw_step", "adamw8": "lcv_master_adamw8_step"}[kind]
    if anchored:
        name, flag = name + "_anchor", () if kind == "adamw8" else (1 if g32 else 0,)
    else:
        name, flag = name + ("_g32" if g32 else ""), ()
    _call(name, table.data_ptr(), *(x.data_ptr() for x in tables), 1, (ONE + CHUNK - 1) // CHUNK, None, *hyper, *flag)
    torch.cuda.synchronize()
    out = {"h": _h_of(dev["P"]), "l": dev["L"].cpu().numpy()}
    if kind == "adamw":
        out["m"], out["v"] = _bits_of(dev["M"]), _bits_of(dev["V"])
    if kind == "adamw8":
        out["cm"], out["cr"], out["s"] = dev["M"].cpu().numpy(), dev["V"].cpu().numpy(), _bits_of(dev["S"])
    # what the step only reads is what it was
    assert np.array_equal(_h_of(dev["A"]), t["A"])
    assert np.array_equal(_bits_of(dev["G"]), W.bits(t["G32"])) if g32 else np.array_equal(_h_of(dev["G"]), t["G"])
    return out


@pytest.mark.parametrize("anchored", [False, True])
@pytest.mark.parametrize("kind", ["sgd", "adamw", "adamw8"])
def test_one_misaligned_array_takes_the_scalar_path_to_the_same_bits(kind, anchored):
    """The packet test ORs the pointers of whichever arrays the form reads (parameter, low words, gradient, with an anchor its
    base words, both moments or both code arrays): any single one of them off a 16-byte (codes: 8-byte) boundary sends every
    thread down the scalar path, which leaves the bits of the all-aligned run.  The other tests offset all arrays of a tensor
    together."""
    t = _one()
    arrays = ["P", "L", "G"] + (["A"] if anchored else []) + (["M", "V"] if kind != "sgd" else [])
    for g32 in ([False] if kind == "adamw8" else [False, True]):
        want = _one_step(kind, anchored, g32, None)
        assert (want["h"] != t["P"]).any() or (want["l"] != t["L"]).any()           # the step moved the masters
        if kind != "sgd":
            assert any((want[k] != ref).any() for k, ref in (("m", W.bits(t["M"])), ("v", W.bits(t["V"])), ("cm", t["CM"]),
                                                             ("cr", t["CR"])) if k in want)
        for offset in arrays:
            got = _one_step(kind, anchored, g32, offset)
            assert got.keys() == want.keys()
            for key in want:
                _report(f"{kind} anchored={anchored} g32={g32}, {offset} offset: {key}", 0, got[key], want[key])


# ---------------------------------------------------------------------------------------------------------- 2. the pins
def _compare(kind, a, pa, b, pb, what):
    for k in range(len(pa)):
        _report(what + " h", k, _h_of(pa[k]), _h_of(pb[k]))
        _report(what + " l", k, a.low_words[k].cpu().numpy(), b.low_words[k].cpu().numpy())
        for j, (x, y) in enumerate(zip(_state(a, kind, k), _state(b, kind, k))):
            _report(what + f" state {j}", k, x, y)


@pytest.mark.parametrize("wd", [0.01, 0.5])
@pytest.mark.parametrize("n", [1, N_MICRO])
def test_sgd_with_zero_base_words_is_the_plain_master_step(n, wd):
    """w - (+0) is w, so wd * (w - w0) is wd * w: lcv_master_sgd_step's (n = 1) and lcv_master_sgd_step_g32's bits."""
    a, pa = _make("sgd", wd, n, anchor="zero")
    b, pb = _make("sgd", wd, n, anchor=None)
    for step in range(2):
        for opt, params in ((a, pa), (b, pb)):
            _feed(opt, params, step, n)
            opt.clip_grad_norm_(1.0)
            opt.step()
    torch.cuda.synchronize()
    _compare("sgd", a, pa, b, pb, f"sgd n={n} wd={wd}")
    assert any((_h_of(pa[k]) != _table()["w"][k][0]).any() for k in range(len(NUMELS)))


@pytest.mark.parametrize("kind, n", [("adamw", 1), ("adamw", N_MICRO), ("adamw8", 1)])
def test_adamw_at_zero_weight_decay_is_the_plain_master_step(kind, n):
    """a = 0: p - 0 * (p - w0) is p, and c_wd = 1: lcv_master_adamw_step's, _g32's and lcv_master_adamw8_step's bits."""
    a, pa = _make(kind, 0.0, n, anchor="table")
    b, pb = _make(kind, 0.0, n, anchor=None)
    for step in range(3):
        for opt, params in ((a, pa), (b, pb)):
            _feed(opt, params, step, n)
            if step == 1:
                opt.clip_grad_norm_(1.0)
            opt.step()
    torch.cuda.synchronize()
    _compare(kind, a, pa, b, pb, f"{kind} n={n}")
    assert any((_h_of(pa[k]) != _table()["w"][k][0]).any() for k in range(len(NUMELS)))


# ---------------------------------------------------------------------------------------------------------- 3. behaviour
def _words(opt, params):
    return [(_h_of(p).copy(), lw.cpu().numpy().copy()) for p, lw in zip(params, opt.low_words)]


@pytest.mark.parametrize("kind", ["sgd", "adamw", "adamw8"])
def test_the_base_is_a_fixed_point_of_the_anchor_step_and_not_of_the_plain_one(kind):
    t = _table()
    opt, params = _make(kind, 0.5, anchor="table", words="base", lr=0.1)
    for _ in range(2):
        _zero_grads(params)
        opt.step()
    torch.cuda.synchronize()
    for k, (h, low) in enumerate(_words(opt, params)):
        _report(f"{kind} h", k, h, t["h0"][k])
        assert not low.any(), (kind, k)
    assert float(opt.drift_norm().item()) == 0.0
    plain, pp = _make(kind, 0.5, anchor=None, words="base", lr=0.1)
    _zero_grads(pp)
    plain.step()
    torch.cuda.synchronize()
    moved = sum(int((h != t["h0"][k]).sum()) + int((low != 0).sum()) for k, (h, low) in enumerate(_words(plain, pp)[:len(NUMELS)]))
    assert moved > 0


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_the_pull_is_a_contraction(kind):
    t = _table()
    opt, params = _make(kind, 0.5, anchor="table", lr=0.1)
    w0 = [W.bf16_to_f32(h0).astype(np.float64) for h0 in t["h0"]]
    dist = [np.abs(W.master(h, low).astype(np.float64) - b) for (h, low), b in zip(t["w"], w0)]
    drift = float(opt.drift_norm().item())
    assert drift > 0.0
    for step in range(5):
        _zero_grads(params)
        opt.step()
        now_drift = float(opt.drift_norm().item())
        for k, (h, low) in enumerate(_words(opt, params)):
            now = np.abs(W.master(h, low).astype(np.float64) - w0[k])
            assert np.all(now <= dist[k]), (kind, step, k)      # rounding is monotone: a step toward w0 never passes it
            dist[k] = now
        print(f"{kind} step {step + 1}: drift {drift!r} -> {now_drift!r}")
        assert now_drift < drift
        drift = now_drift


# ---------------------------------------------------------------------------------------------------------- 4. the drift
def _drift_raw(params, lows, anchors, ws=None):
    rows, chunk = [], 0
    for p in params:
        rows.append([p.data_ptr(), 0, 0, 0, p.numel(), chunk])
        chunk += (p.numel() + CHUNK - 1) // CHUNK
    table = torch.tensor(rows, dtype=torch.int64).to(DEV)
    ap = torch.tensor([a.data_ptr() for a in anchors], dtype=torch.int64).to(DEV)
    lp = torch.tensor([x.data_ptr() for x in lows], dtype=torch.int64).to(DEV) if lows is not None else None
    part = torch.full((chunk + 1,), -7.0, dtype=torch.float32, device=DEV) if ws is None else ws
    out = torch.zeros(2, dtype=torch.float32, device=DEV)
    _call("lcv_master_drift_sumsq", table.data_ptr(), None if lp is None else lp.data_ptr(), ap.data_ptr(), len(rows), chunk,
          part.data_ptr(), chunk * 4, out.data_ptr())
    torch.cuda.synchronize()
    assert float(part[chunk].item()) == -7.0 or ws is not None       # nothing written past the partials
    return _bits_of(out), chunk


def _check_drift(bits, want, n_total, what):
    got = W.floats(bits).astype(np.float64)
    rel = abs(got[0] - want) / want
    bound = (n_total + 4) * 2.0 ** -24
    print(f"{what}: sum of squares {got[0]!r} float64 {want!r} rel. error {rel:.3e} bound {bound:.3e}")
    # worst-case fp32 summation of n_total non-negative terms (n_total - 1 additions at 2^-24 each), each term (w - w0)^2 with
    # three roundings (the difference, squared, and the product)
    assert rel <= bound
    assert bits[1] == W.bits(np.sqrt(W.floats(bits[:1])))[0]          # out[1] is the correctly rounded root of out[0]


def test_drift_sumsq():
    t = _table()
    n_total = sum(NUMELS) + IDLE
    opt, params = _make("sgd", 0.0, anchor="table")
    want = A.drift_sumsq([(h, low, h0) for (h, low), h0 in zip(t["w"], t["h0"])])
    raw, chunks = _drift_raw(params, opt.low_words, opt._anchor)
    assert chunks == 11
    _check_drift(raw, want, n_total, "raw ABI")
    again, _ = _drift_raw(params, opt.low_words, opt._anchor)
    assert np.array_equal(raw, again)                                 # same inputs, same bits
    # through the optimizer: all parameters, the one without a gradient too; a 0-dim fp32 device tensor
    d = opt.drift_norm()
    assert d.shape == () and d.dtype == torch.float32 and d.is_cuda
    assert _bits_of(d)[0] == raw[1] and _bits_of(opt.drift_norm())[0] == raw[1]
    # low == NULL is "all low words zero": an optimizer without master weights, the raw call, and zeroed low words agree
    want0 = A.drift_sumsq([(h, None, h0) for (h, _), h0 in zip(t["w"], t["h0"])])
    null, _ = _drift_raw(params, None, opt._anchor)
    _check_drift(null, want0, n_total, "low = NULL")
    bf, pbf = _make("sgd", 0.0, anchor=None, master=False)
    assert _bits_of(bf.drift_norm(anchor=opt._anchor))[0] == null[1]
    opt.resync()
    zeroed, _ = _drift_raw(params, opt.low_words, opt._anchor)
    assert np.array_equal(zeroed, null) and not np.array_equal(null, raw)
    # zero where the parameters equal the anchors
    same, _ = _drift_raw(opt._anchor, None, opt._anchor)
    assert not same.any()
    # a list passed in overrides nothing and is not kept
    assert _bits_of(opt.drift_norm(anchor=[p.detach().clone() for p in params]))[0] == 0
    assert _bits_of(opt.drift_norm())[0] == zeroed[1]


def test_drift_sumsq_over_more_partials_than_the_second_launch_has_threads():
    """1100 chunks and a tail: every thread of the second launch adds up to two partials, most waves of it add one."""
    n = CHUNK * 1100 + 5
    rng = np.random.default_rng(5)
    h, low = W.weights(rng, n)
    h0, low = A.anchors(rng, h, low)
    p, lw, a = _bf16_dev(h), _i16_dev(low), _bf16_dev(h0)
    bits, chunks = _drift_raw([p], [lw], [a])
    assert chunks == 1101
    _check_drift(bits, A.drift_sumsq([(h, low, h0)]), n, "1101 chunks")
    again, _ = _drift_raw([p], [lw], [a])
    assert np.array_equal(bits, again)


def test_bad_arguments_are_refused():
    from lcv_hip.lib import LcvError
    t = torch.zeros(8, dtype=torch.int64, device=DEV).data_ptr()
    sgd, adam = (None, 1e-3, 0.0), (None, 1e-3, 0.9, 0.999, 1e-8, 0.0)
    cases = []
    for name, tail, extra in (("lcv_master_sgd_step_anchor", sgd + (0,), 0), ("lcv_master_adamw_step_anchor", adam + (1, 0), 0),
                              ("lcv_master_adamw8_step_anchor", adam + (1,), 1)):
        ptrs = (t,) * (3 + extra)
        for bad in range(3 + extra):                                 # each pointer missing in turn
            cases.append((name, ptrs[:bad] + (None,) + ptrs[bad + 1:] + (1, 1) + tail))
        cases.append((name, ptrs + (0, 1) + tail))
        cases.append((name, ptrs + (1, 0) + tail))
        cases.append((name, ptrs + (1, 2 ** 31) + tail))
    cases.append(("lcv_master_sgd_step_anchor", (t, t, t, 1, 1) + sgd + (2,)))                      # grad_f32 is 0 or 1
    cases.append(("lcv_master_adamw_step_anchor", (t, t, t, 1, 1) + adam + (1, -1)))
    cases.append(("lcv_master_adamw_step_anchor", (t, t, t, 1, 1) + adam + (0, 0)))                # step >= 1
    cases.append(("lcv_master_adamw8_step_anchor", (t, t, t, t, 1, 1) + adam + (0,)))
    for args in ((None, None, t, 1, 1, t, 4, t), (t, None, None, 1, 1, t, 4, t), (t, None, t, 0, 1, t, 4, t),
                 (t, None, t, 1, 0, t, 4, t), (t, None, t, 1, 1, None, 4, t), (t, None, t, 1, 1, t, 4, None),
                 (t, None, t, 1, 3, t, 8, t)):                                                       # a workspace too small
        cases.append(("lcv_master_drift_sumsq", args))
    for name, args in cases:
        with pytest.raises(LcvError) as e:
            _call(name, *args)
        assert e.value.code == -1 and not e.value.fatal, (name, args)
    with pytest.raises(LcvError, match="anchor needs master_weights=True"):
        _make("sgd", 0.01, anchor="table", master=False)


# ---------------------------------------------------------------------------------------------------------- 5. the loops
_SHARED = {}


def _inputs():
    if not _SHARED:
        g = torch.Generator().manual_seed(7)
        r = lambda *s: torch.randn(*s, generator=g)
        _SHARED["cond"] = r(1, 16, 1, 10, 20).to(BF16).to(DEV)            # one conditioning latent frame: 5 x 10 tokens
        _SHARED["train"] = r(1, 16, 2, 10, 20).to(BF16).to(DEV)           # two target frames
        _SHARED["train2"] = r(1, 16, 2, 10, 20).to(BF16).to(DEV)          # a second video's, for the batch loop
        _SHARED["embeds"] = r(1, 1, 12, 64).to(BF16).to(DEV)
        mask = torch.ones(1, 12, dtype=torch.int64)
        mask[0, 9:] = 0
        _SHARED["mask"] = mask.to(DEV)
    return _SHARED


def _dit():
    from longcat_video.modules.longcat_video_dit import LongCatVideoTransformer3DModel
    m = LongCatVideoTransformer3DModel(device=DEV, dtype=BF16, hidden_size=256, depth=2, num_heads=2, caption_channels=64,
                                       adaln_tembed_dim=64).init_synthetic_(3, std=0.05)
    return m.eval()


@pytest.fixture
def deterministic():
    from lcv_hip import ops
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    yield ops
    ops.set_deterministic(was)


def _full(optimizer="sgd", weight_decay=0.01, with_base=False, batch=False, **flag):
    """Three optimizer steps from one seed on a fresh model."""
    from tta.full_tta import finetune_full_batch, finetune_full_on_conditioning, snapshot_base_state
    i = _inputs()
    dit = _dit()
    for p in dit.parameters():
        p.requires_grad = True
    base = snapshot_base_state(dit) if with_base else None
    if with_base:
        flag["base_state"] = base
    torch.manual_seed(1234)
    common = dict(num_steps=3, lr=1e-3 if optimizer == "sgd" else 1e-4, warmup_steps=1, weight_decay=weight_decay,
                  max_grad_norm=1.0, device=DEV, dtype=BF16, optimizer_type=optimizer)
    if batch:
        data = [dict(cond_latents=i["cond"], train_latents=tr, prompt_embeds=i["embeds"], prompt_mask=i["mask"])
                for tr in (i["train"], i["train2"])]
        res = finetune_full_batch(dit, data, **common, **flag)
    else:
        res = finetune_full_on_conditioning(dit, i["cond"], i["train"], i["embeds"], i["mask"], **common, **flag)
    torch.cuda.synchronize()
    if base is not None:                                                 # the anchors were read, never written
        fresh = snapshot_base_state(_dit())
        assert all(torch.equal(base[k], fresh[k]) for k in base)
    return [float(v).hex() for v in res["losses"]], [p.detach().clone() for p in dit.parameters()], res


def test_full_loop_with_the_flag_omitted_is_todays_run(deterministic):
    l0, w0, r0 = _full()
    l1, w1, r1 = _full(decay_to_base=False)
    assert len(l0) == 3 and l0 == l1 and all(torch.equal(a, b) for a, b in zip(w0, w1))
    assert "drift_norm" not in r0 and "drift_norm" not in r1
    m0, v0, q0 = _full(master_weights=True)
    m1, v1, q1 = _full(master_weights=True, decay_to_base=False)
    assert m0 == m1 and all(torch.equal(a, b) for a, b in zip(v0, v1)) and "drift_norm" not in q0 and "drift_norm" not in q1
    # a base_state alone measures and changes nothing else - with or without master weights
    l2, w2, r2 = _full(with_base=True)
    assert l2 == l0 and all(torch.equal(a, b) for a, b in zip(w2, w0))
    assert set(r2) - set(r0) == {"drift_norm"} and isinstance(r2["drift_norm"], float) and r2["drift_norm"] >= 0.0
    m2, v2, q2 = _full(with_base=True, master_weights=True)
    assert m2 == m0 and all(torch.equal(a, b) for a, b in zip(v2, v0)) and q2["drift_norm"] > 0.0


@pytest.mark.parametrize("optimizer, extra", [("sgd", {}), ("adamw", {}), ("adamw", {"moments_8bit": True}), ("sgd", {"grad_accum": 2})])
def test_full_loop_with_the_flag_is_reproducible_and_moves(optimizer, extra, deterministic):
    from lcv_hip.lib import LcvError
    la, wa, ra = _full(optimizer, with_base=True, master_weights=True, decay_to_base=True, **extra)
    lb, wb, rb = _full(optimizer, with_base=True, master_weights=True, decay_to_base=True, **extra)
    assert len(la) == 3 and all(np.isfinite(float.fromhex(v)) for v in la)
    assert la == lb and all(torch.equal(a, b) for a, b in zip(wa, wb)) and ra["drift_norm"] == rb["drift_norm"]
    assert ra["drift_norm"] > 0.0 and np.isfinite(ra["drift_norm"])
    if not extra:
        # without a base_state the anchors are clones taken before the first step: the same run
        lc, wc, rc = _full(optimizer, master_weights=True, decay_to_base=True)
        assert lc == la and all(torch.equal(a, b) for a, b in zip(wc, wa)) and rc["drift_norm"] == ra["drift_norm"]
        with pytest.raises(LcvError, match="anchor needs master_weights=True"):
            _full(optimizer, decay_to_base=True)


@pytest.mark.parametrize("batch", [False, True])
def test_a_strong_pull_toward_the_base_leaves_less_drift_than_a_strong_pull_toward_zero(batch, deterministic):
    wd = 0.5 / (1e-3 * 3)                                                # lr * wd * steps is about 0.5
    _, _, anchored = _full(weight_decay=wd, with_base=True, batch=batch, master_weights=True, decay_to_base=True)
    _, _, eroded = _full(weight_decay=wd, with_base=True, batch=batch, master_weights=True, decay_to_base=False)
    print(f"drift with the pull toward the base {anchored['drift_norm']!r}, toward zero {eroded['drift_norm']!r}")
    assert 0.0 < anchored["drift_norm"] < eroded["drift_norm"]


def _norm_tune(also_delta=False, **flag):
    from tta import delta as D
    i = _inputs()
    dit = _dit()
    w = D.NormTuneForward(dit, "all_norm", also_tune_delta=also_delta).to(DEV)
    start = [p.detach().clone() for p in w.norm_params]
    torch.manual_seed(1234)
    res = D.optimize_norm_params(w, w.tuned_params, i["cond"], i["train"], i["embeds"], i["mask"], num_steps=3, lr=1e-2, device=DEV,
                                 dtype=BF16, **flag)
    torch.cuda.synchronize()
    return [float(v).hex() for v in res["losses"]], [p.detach().clone() for p in w.tuned_params], res, start, w


def test_norm_tuning_loop(deterministic):
    l0, w0, r0, _, _ = _norm_tune(master_weights=True)
    l1, w1, r1, _, _ = _norm_tune(master_weights=True, decay_to_base=False)
    assert l0 == l1 and all(torch.equal(a, b) for a, b in zip(w0, w1)) and "drift_norm" not in r0 and "drift_norm" not in r1
    la, wa, ra, start, wrap = _norm_tune(master_weights=True, decay_to_base=True)
    lb, wb, rb, _, _ = _norm_tune(master_weights=True, decay_to_base=True)
    assert la == lb and all(torch.equal(a, b) for a, b in zip(wa, wb)) and ra["drift_norm"] == rb["drift_norm"]
    assert set(ra) - set(r0) == {"drift_norm"} and ra["drift_norm"] > 0.0
    # the anchors were the norm weights at entry: | |m - a| - |h - a| | <= |m - h|, and a master is within half a bf16 ulp
    # of its bf16 word
    words = sum(float(((p.detach().double() - s.double()) ** 2).sum()) for p, s in zip(wrap.norm_params, start)) ** 0.5
    half_ulp = [torch.exp2(torch.floor(torch.log2(p.detach().double().abs())) - 8.0) for p in wrap.norm_params]
    slack = sum(float((u ** 2).sum()) for u in half_ulp) ** 0.5
    print(f"norm tuning: drift_norm {ra['drift_norm']!r}, distance of the bf16 words {words!r}, slack {slack!r}")
    assert abs(ra["drift_norm"] - words) <= slack + 1e-5 * words
    # with the fp32 delta vector in the list: the bf16 optimizer is anchored, the delta keeps its decay toward zero
    ld, wd_, rd, _, wrapd = _norm_tune(also_delta=True, master_weights=True, decay_to_base=True)
    assert rd["drift_norm"] > 0.0 and rd["delta_norm"] > 0.0 and len(ld) == 3


# ---------------------------------------------------------------------------------------------------------- 6. the runners
def _main(rel, argv):
    path = PKG / rel
    spec = importlib.util.spec_from_file_location("dtb_" + path.stem, path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    m.main(argv)


COMMON = ["--checkpoint-dir", "synthetic:2:256:64", "--data-dir", "synthetic:1", "--num-cond-frames", "5", "--num-frames", "13",
          "--gen-start-frame", "40", "--tta-total-frames", "33", "--tta-context-frames", "9", "--num-inference-steps", "2"]


@pytest.mark.parametrize("rel, extra", [
    # no early stopper for the full model: a restore of the initial weights would make a drift of zero legitimate
    ("lora_experiment/scripts/run_full_tta.py", ["--num-steps", "4", "--learning-rate", "1e-4", "--no-save-videos", "--es-disable"]),
    ("delta_experiment/scripts/run_norm_tune_tta.py", ["--norm-steps", "4", "--norm-lr", "1e-2", "--es-check-every", "2",
                                                       "--es-patience", "1"]),
])
def test_runners_accept_decay_to_base_and_write_the_keys_only_with_it(tmp_path, rel, extra):
    on, off = tmp_path / "on", tmp_path / "off"
    _main(rel, COMMON + extra + ["--output-dir", str(on), "--master-weights", "--decay-to-base"])
    _main(rel, COMMON + extra + ["--output-dir", str(off), "--master-weights"])
    s_on, s_off = (json.loads((d / "summary.json").read_text()) for d in (on, off))
    for s in (s_on, s_off):
        assert s["num_videos"] == 1 and s["num_successful"] == 1 and s["results"][0]["success"]
    r_on, r_off = s_on["results"][0], s_off["results"][0]
    assert set(r_on) - set(r_off) == {"drift_norm"} and set(r_off) <= set(r_on)
    assert isinstance(r_on["drift_norm"], float) and r_on["drift_norm"] > 0.0
    if "full" in rel:
        c_on, c_off = (json.loads((d / "config.json").read_text()) for d in (on, off))
        assert c_on["training"]["decay_to_base"] is True and "decay_to_base" not in c_off["training"]
        assert set(s_on) == set(s_off)
    else:
        assert s_on["decay_to_base"] is True and set(s_on) - set(s_off) == {"decay_to_base"}

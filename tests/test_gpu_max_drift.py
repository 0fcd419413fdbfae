"""GPU: the trust-region cap on the drift from the base weights (include/lcv_hip_trust.h, `enable_max_drift` /
`project_max_drift` / `--max-drift`).

1. lcv_trust_sumsq at the C ABI against the numpy restatement (tests/trust_ref.py), bit for bit on per_tensor and out: bf16 words
   with low words, bf16 words with low = NULL, fp32 values, each with an anchor and with anchor = NULL; run-to-run bits; zero at
   the base.  Tensors: a single element, a sub-packet tail, a quarter chunk, one element past it, an exact chunk, one element
   past a chunk (every array of it a one-element offset view: the scalar path), a tail past two chunks, and a 300-element
   parameter that never gets a gradient.  Every array sits between guard elements.
2. lcv_trust_project in both scopes, bit for bit on the bf16 words, the low words and the fp32 values and on the trace slot: a
   radius that projects everything, one that in tensor scope projects some tensors and not others, one nothing exceeds (every
   buffer byte-identical afterwards, guards included), a NaN total (nothing written).  The float64 bound of trust_ref's
   docstring after every projection.  Refusals.
3. Through the optimizers: three AdamW and three SGD steps with enable_max_drift against the restated steps followed by the
   restated projection, master-weight bf16 and fp32 parameters; two optimizers under one global ball; the weight average takes
   the projected masters.
4. The delta-A, delta-B and norm-tuning loops: the ball is kept, inf changes no bit.
5. The runners on the smallest synthetic checkpoint: delta-A with the early stopper, LoRA and full-model SGD.
"""
import importlib.util
import json
import math
from pathlib import Path

import numpy as np
import pytest
import torch

import anchor_ref as A
import ema_ref as E
import master_weights_ref as W
import optim_ref as O
import trust_ref as T

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
PKG = ROOT / "longcat-video-tta_amd"
BF16 = torch.bfloat16
DEV = "cuda"
NUMELS = (1, 7, 512, 513, 2048, 2049, 4099)
VIEW = 5                      # the 2049-element tensor: every array of it starts one element late
IDLE = 300                    # an eighth parameter that never gets a gradient
ALL = NUMELS + (IDLE,)
CHUNK = 2048
GUARD = 8                     # guard elements on both sides of every array (16 bytes of bf16 / int16, 32 of fp32)
F = np.float32
_NP = {"h": np.uint16, "l": np.int16, "f": np.float32}
_SENTINEL = {"h": 0x7FC1, "l": -12345, "f": np.float32(np.nan)}


# ---------------------------------------------------------------------------------------------------------- helpers
class _Arr:
    """One array on the device between guard elements; `off` starts it one element late (no longer 16-byte aligned)."""

    def __init__(self, kind, values, off=False):
        values = np.ascontiguousarray(values, dtype=_NP[kind]).ravel()
        self.kind, self.n, self.lo = kind, values.size, GUARD + (1 if off else 0)
        host = np.full(values.size + 2 * GUARD + 1, _SENTINEL[kind], dtype=_NP[kind])
        host[self.lo:self.lo + self.n] = values
        self.host = host
        self.buf = torch.from_numpy(host.view(np.int16 if kind != "f" else np.float32).copy()).to(DEV)
        self.view = self.buf[self.lo:self.lo + self.n]
        assert self.view.data_ptr() % 16 == (self.view.element_size() if off else 0)

    def ptr(self):
        return self.view.data_ptr()

    def raw(self):
        """The whole buffer's bits, guards included."""
        return self.buf.cpu().numpy().view(np.uint32 if self.kind == "f" else np.uint16)

    def values(self):
        got = self.buf.cpu().numpy()[self.lo:self.lo + self.n]
        return got.view(np.uint32) if self.kind == "f" else got.view(_NP[self.kind])

    def pristine(self):
        return np.array_equal(self.raw(), self.host.view(np.uint32 if self.kind == "f" else np.uint16))


def _call(name, *args):
    from lcv_hip import lib
    lib.call(name, *args, torch.cuda.current_stream().cuda_stream)


def _report(what, k, got, want):
    got, want = np.asarray(got).ravel(), np.asarray(want).ravel()
    assert got.shape == want.shape, (what, k, got.shape, want.shape)
    bad = np.flatnonzero(got != want)
    if bad.size:
        i = int(bad[0])
        raise AssertionError(f"{what}: tensor {k} (numel {got.size}) index {i}: got {got[i]!r} want {want[i]!r}; "
                             f"{bad.size} mismatches")


_TABLE = {}


def _table():
    """Host-generated inputs, made once and never written: masters |w| in [2^-10, 2] with all 32 bits live; base words
    bf16(w (1 + delta)), |delta| in [2^-12, 2^-4], every 5th element at its base; fp32 base values with live low bits."""
    if not _TABLE:
        rng = np.random.default_rng(61)
        _TABLE["h"], _TABLE["l"], _TABLE["h0"], _TABLE["w0f"] = [], [], [], []
        for n in ALL:
            h, low = W.weights(rng, n)
            if n == 1:             # the generator would put the only element at its base: move the base instead
                h0 = W.to_bf16_bits(W.master(h, low) * F(1.015625))
            else:
                h0, low = A.anchors(rng, h, low)
            _TABLE["h"].append(h)
            _TABLE["l"].append(low)
            _TABLE["h0"].append(h0)
            _TABLE["w0f"].append(W.master(h0, rng.integers(-3000, 3000, size=n).astype(np.int16)))
    return _TABLE


MODES = ("bf16", "bf16_nolow", "f32")


def _ref_tensors(mode, anchored):
    """The (w, w0) pairs the restatement sees."""
    t = _table()
    out = []
    for k in range(len(ALL)):
        if mode == "f32":
            w = W.master(t["h"][k], t["l"][k])
            out.append((w, t["w0f"][k] if anchored else np.zeros(w.size, F)))
        else:
            out.append(T.from_words(t["h"][k], t["l"][k] if mode == "bf16" else None, t["h0"][k] if anchored else None))
    return out


class _Dev:
    """The same tensors on the device with the descriptor table and the side arrays of the C ABI."""

    def __init__(self, mode, anchored, at_base=False):
        t = _table()
        self.mode, self.f32 = mode, mode == "f32"
        self.P, self.L, self.A = [], [], []
        for k in range(len(ALL)):
            off = k == VIEW
            if self.f32:
                base = t["w0f"][k] if anchored else np.zeros(ALL[k], F)
                self.P.append(_Arr("f", base if at_base else W.master(t["h"][k], t["l"][k]), off))
                if anchored:
                    self.A.append(_Arr("f", t["w0f"][k], off))
            else:
                base = t["h0"][k] if anchored else np.zeros(ALL[k], np.uint16)
                self.P.append(_Arr("h", base if at_base else t["h"][k], off))
                if mode == "bf16":
                    self.L.append(_Arr("l", np.zeros(ALL[k], np.int16) if at_base else t["l"][k], off))
                if anchored:
                    self.A.append(_Arr("h", t["h0"][k], off))
        rows, chunk = [], 0
        for p in self.P:
            rows.append([p.ptr(), 0, 0, 0, p.n, chunk])
            chunk += (p.n + CHUNK - 1) // CHUNK
        self.n, self.chunks = len(rows), chunk
        self.table = torch.tensor(rows, dtype=torch.int64).to(DEV)
        self.lp = torch.tensor([x.ptr() for x in self.L], dtype=torch.int64).to(DEV) if self.L else None
        self.ap = torch.tensor([x.ptr() for x in self.A], dtype=torch.int64).to(DEV) if self.A else None
        self.part = torch.full((chunk + 1,), -7.0, dtype=torch.float32, device=DEV)
        self.per = torch.full((self.n + 1,), -7.0, dtype=torch.float32, device=DEV)
        self.out = torch.full((3,), -7.0, dtype=torch.float32, device=DEV)
        self.trace = torch.full((4,), -7.0, dtype=torch.float32, device=DEV)

    def head(self):
        return (self.table.data_ptr(), None if self.lp is None else self.lp.data_ptr(),
                None if self.ap is None else self.ap.data_ptr(), self.n, self.chunks, 1 if self.f32 else 0)

    def sumsq(self):
        _call("lcv_trust_sumsq", *self.head(), self.part.data_ptr(), self.chunks * 4, self.per.data_ptr(), self.out.data_ptr())
        torch.cuda.synchronize()
        for buf in (self.part, self.per, self.out):
            assert float(buf[-1].item()) == -7.0                         # nothing written past the workspace and the outputs
        return W.bits(self.per[:-1].cpu().numpy()), W.bits(self.out[:2].cpu().numpy())

    def project(self, scope, rr, sumsq=None, per=None):
        _call("lcv_trust_project", *self.head(), scope, (self.out if sumsq is None else sumsq).data_ptr(),
              (self.per if per is None else per).data_ptr(), rr, self.trace[1:3].data_ptr())
        torch.cuda.synchronize()
        assert float(self.trace[0].item()) == -7.0 and float(self.trace[3].item()) == -7.0
        return W.bits(self.trace[1:3].cpu().numpy())

    def arrays(self):
        return self.P + self.L + self.A


def _check_guards(d, what):
    for a in d.arrays():
        raw, lo = a.raw(), a.lo
        want = a.host.view(raw.dtype)
        assert np.array_equal(raw[:lo], want[:lo]) and np.array_equal(raw[lo + a.n:], want[lo + a.n:]), f"{what}: a guard was written"


# ---------------------------------------------------------------------------------------------------------- 1. the sum
@pytest.mark.parametrize("anchored", [True, False])
@pytest.mark.parametrize("mode", MODES)
def test_trust_sumsq(mode, anchored):
    d = _Dev(mode, anchored)
    per, out = d.sumsq()
    want_per, want_out = T.sumsq(_ref_tensors(mode, anchored))
    assert d.chunks == 11
    _report(f"{mode} anchored={anchored} per_tensor", -1, per, W.bits(want_per))
    _report(f"{mode} anchored={anchored} out", -1, out, W.bits(want_out))
    assert want_out[0] > 0 and np.all(want_per > 0)
    again_per, again_out = d.sumsq()
    assert np.array_equal(per, again_per) and np.array_equal(out, again_out)          # same inputs, same bits
    assert all(a.pristine() for a in d.arrays())                                       # the sum writes no parameter
    # the summation bound of trust_ref's docstring against float64
    exact = T.drift64(_ref_tensors(mode, anchored)) ** 2
    k = T.depth(ALL) + 3
    rel = abs(float(W.floats(out[:1])[0]) - exact) / exact
    print(f"{mode} anchored={anchored}: s {W.floats(out[:1])[0]!r} float64 {exact!r} rel {rel:.3e} bound {((1 + T.U) ** k - 1):.3e}")
    assert rel <= (1 + T.U) ** k - 1
    if mode == "bf16_nolow":           # low = NULL is "all low words zero"
        z = _Dev("bf16", anchored)
        for a in z.L:
            a.view.zero_()
        zp, zo = z.sumsq()
        assert np.array_equal(zp, per) and np.array_equal(zo, out)


@pytest.mark.parametrize("anchored", [True, False])
@pytest.mark.parametrize("mode", ["bf16", "f32"])
def test_trust_sumsq_is_zero_at_the_base(mode, anchored):
    per, out = _Dev(mode, anchored, at_base=True).sumsq()
    assert not per.any() and not out.any()


# ---------------------------------------------------------------------------------------------------------- 2. the projection
def _rms(mode, anchored):
    per, out = T.sumsq(_ref_tensors(mode, anchored))
    return np.sqrt(per.astype(np.float64) / np.array(ALL, dtype=np.float64)), math.sqrt(float(out[0]) / sum(ALL))


def _radius(case, mode, anchored):
    per_rms, all_rms = _rms(mode, anchored)
    if case == "all":
        return 0.5 * min(per_rms.min(), all_rms)
    if case == "some":
        return float(np.sort(per_rms)[len(ALL) // 2]) * 1.0001            # above half of the tensors' RMS drift, below the rest
    return 2.0 * max(per_rms.max(), all_rms)


@pytest.mark.parametrize("case", ["all", "some", "none"])
@pytest.mark.parametrize("scope", ["global", "tensor"])
@pytest.mark.parametrize("anchored", [True, False])
@pytest.mark.parametrize("mode", ["bf16", "f32"])
def test_trust_project(mode, anchored, scope, case):
    from lcv_hip import lib
    R = _radius(case, mode, anchored)
    ref = _ref_tensors(mode, anchored)
    new, want_per, want_out, want_trace = T.project(ref, R, scope)
    moved = [n is not o[0] for n, o in zip(new, ref)]
    what = f"{mode} anchored={anchored} {scope} {case}"
    if case == "all":
        assert all(moved)
    elif case == "none":
        assert not any(moved) and want_trace[1] == 1.0
    elif scope == "tensor":
        assert 0 < sum(moved) < len(ALL), moved
    d = _Dev(mode, anchored)
    d.sumsq()
    rr = float(R) * float(R) * (1.0 if scope == "tensor" else float(sum(ALL)))
    trace = d.project(lib.LCV_TRUST_TENSOR if scope == "tensor" else lib.LCV_TRUST_GLOBAL, rr)
    _report(what + " trace", -1, trace, W.bits(np.array(want_trace, dtype=F)))
    _check_guards(d, what)
    assert all(a.pristine() for a in d.A)                                # the base values are read, never written
    for k, (w, m) in enumerate(zip(new, moved)):
        if not m:                                                        # inside its ball: byte-identical, guards included
            assert d.P[k].pristine() and (not d.L or d.L[k].pristine()), (what, k)
        elif mode == "f32":
            _report(what + " w", k, d.P[k].values(), W.bits(w))
        else:
            h, low = T.to_words(w)
            _report(what + " h", k, d.P[k].values(), h)
            _report(what + " l", k, d.L[k].values(), low)
    if any(moved):
        assert any((W.bits(w) != W.bits(o[0])).any() for w, o, m in zip(new, ref, moved) if m)
        # the float64 bound: the projected balls hold their radius
        got = [(W.floats(d.P[k].values()) if mode == "f32" else W.master(d.P[k].values(), d.L[k].values()), ref[k][1])
               for k in range(len(ALL))]
        if scope == "global":
            assert T.bound_holds(got, T.radius2(R, sum(ALL)))
        else:
            for k, m in enumerate(moved):
                if m:
                    assert T.bound_holds([got[k]], T.radius2(R, ALL[k])), (what, k)
        assert T.eps_s(ALL) <= T.EPS_S


@pytest.mark.parametrize("scope", ["global", "tensor"])
@pytest.mark.parametrize("mode", ["bf16", "f32"])
def test_trust_project_writes_nothing_on_a_nan_total_or_an_infinite_radius(mode, scope):
    from lcv_hip import lib
    sc = lib.LCV_TRUST_TENSOR if scope == "tensor" else lib.LCV_TRUST_GLOBAL
    d = _Dev(mode, True)
    d.sumsq()
    nan_total = torch.full((2,), float("nan"), dtype=torch.float32, device=DEV)
    nan_per = torch.full((d.n,), float("nan"), dtype=torch.float32, device=DEV)
    trace = W.floats(d.project(sc, 1e-12, sumsq=nan_total, per=nan_per))
    assert np.isnan(trace[0]) and trace[1] == 1.0
    assert all(a.pristine() for a in d.arrays())
    trace = W.floats(d.project(sc, float("inf")))
    assert trace[0] == float(d.out[0].item()) and trace[1] == 1.0
    assert all(a.pristine() for a in d.arrays())


def test_trust_bad_arguments_are_refused():
    from lcv_hip.lib import LcvError
    t = torch.zeros(8, dtype=torch.int64, device=DEV).data_ptr()
    cases = [("lcv_trust_sumsq", a) for a in (
        (None, t, t, 1, 1, 0, t, 4, t, t), (t, t, t, 0, 1, 0, t, 4, t, t), (t, t, t, 1, 0, 0, t, 4, t, t),
        (t, t, t, 1, 2 ** 31, 0, t, 2 ** 33, t, t), (t, t, t, 1, 1, 1, t, 4, t, t),              # fp32 parameters take no low words
        (t, t, t, 1, 1, 0, None, 4, t, t), (t, t, t, 1, 3, 0, t, 8, t, t),                      # a workspace too small
        (t, t, t, 1, 1, 0, t, 4, None, t), (t, t, t, 1, 1, 0, t, 4, t, None))]
    cases += [("lcv_trust_project", a) for a in (
        (None, t, t, 1, 1, 0, 0, t, t, 1.0, None), (t, t, t, 0, 1, 0, 0, t, t, 1.0, None), (t, t, t, 1, 0, 0, 0, t, t, 1.0, None),
        (t, None, t, 1, 1, 0, 0, t, t, 1.0, None),                                              # bf16 words without low words
        (t, t, t, 1, 1, 1, 0, t, t, 1.0, None),                                                 # fp32 values with low words
        (t, t, t, 1, 1, 0, 2, t, t, 1.0, None), (t, t, t, 1, 1, 0, 0, None, t, 1.0, None),
        (t, t, t, 1, 1, 0, 1, t, None, 1.0, None),                                              # tensor scope reads per_tensor
        (t, t, t, 1, 1, 0, 0, t, t, 0.0, None), (t, t, t, 1, 1, 0, 0, t, t, -1.0, None),
        (t, t, t, 1, 1, 0, 0, t, t, float("nan"), None))]
    for name, args in cases:
        with pytest.raises(LcvError) as e:
            _call(name, *args)
        assert e.value.code == -1 and not e.value.fatal, (name, args)


# ---------------------------------------------------------------------------------------------------------- 3. the optimizers
def _bf16_dev(h):
    return torch.from_numpy(np.ascontiguousarray(h).view(np.int16).copy()).view(BF16).to(DEV)


def _offset_view(t):
    base = torch.zeros(t.numel() + 1, dtype=t.dtype, device=t.device)
    base[1:].copy_(t.reshape(-1))
    v = base[1:].view(t.shape)
    assert v.data_ptr() % 16 == t.element_size() and v.is_contiguous()
    return v


def _h_of(t):
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16).ravel()


def _bits_of(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy().view(np.uint32).ravel()


_GRADS = {}


def _grads():
    if not _GRADS:
        rng = np.random.default_rng(67)
        _GRADS["g"] = [[W.grads(rng, n) for n in NUMELS] for _ in range(3)]
    return _GRADS["g"]


LR, WD, B1, B2, EPS = {"sgd": 2e-2, "adamw": 1e-2}, 0.01, 0.9, 0.999, 1e-8


def _make_opt(kind, f32, anchored=True, ema=None):
    """An optimizer over the table's tensors (the eighth never gets a gradient) and the restatement's state."""
    from lcv_hip import ops
    t = _table()
    params, anchors, ref = [], [], []
    for k in range(len(ALL)):
        if f32:
            p = torch.from_numpy(W.master(t["h"][k], t["l"][k]).copy()).to(DEV)
            a = torch.from_numpy(t["w0f"][k].copy()).to(DEV)
            w0 = t["w0f"][k] if anchored else np.zeros(ALL[k], F)
        else:
            p, a = _bf16_dev(t["h"][k]), _bf16_dev(t["h0"][k])
            w0 = W.bf16_to_f32(t["h0"][k])
        params.append(_offset_view(p) if k == VIEW else p)
        anchors.append(_offset_view(a) if k == VIEW else a)
        ref.append(dict(w=W.master(t["h"][k], t["l"][k]), w0=w0, m=np.zeros(ALL[k], F), v=np.zeros(ALL[k], F)))
    kw = dict(weight_decay=WD, master_weights=not f32)
    opt = (ops.FusedSGDClip(params, lr=LR[kind], **kw) if kind == "sgd"
           else ops.FusedAdamWClip(params, lr=LR[kind], betas=(B1, B2), eps=EPS, **kw))
    if not f32:
        opt._low[VIEW] = _offset_view(opt._low[VIEW])
        for lw, low in zip(opt.low_words, t["l"]):
            lw.copy_(torch.from_numpy(low.copy()).to(DEV))
    if ema is not None:
        opt.enable_weight_ema(ema)
        for r in ref:
            r["e"] = W.bits(r["w"]).copy()
    return opt, params, (anchors if anchored or not f32 else None), ref


def _give(params, gs, f32):
    for k in range(len(NUMELS)):
        g = _bf16_dev(gs[k])
        g = g.float() if f32 else g
        params[k].grad = _offset_view(g) if k == VIEW else g


def _ref_step(kind, f32, ref, gs, coef, step):
    """The restated optimizer step of the tensors that have a gradient (the plain decay toward zero)."""
    for k in range(len(NUMELS)):
        r = ref[k]
        if f32:
            g = W.bf16_to_f32(gs[k])
            if kind == "sgd":
                r["w"] = O.sgd_step_f32(r["w"], g, coef, LR[kind], WD)
            else:
                r["w"], r["m"], r["v"] = O.adamw_step_f32(r["w"], r["m"], r["v"], g, coef, LR[kind], B1, B2, EPS, WD, step)
        else:
            h, low = T.to_words(r["w"])
            if kind == "sgd":
                h, low = W.sgd_step(h, low, gs[k], coef, LR[kind], WD)
            else:
                h, low, r["m"], r["v"] = W.adamw_step(h, low, r["m"], r["v"], gs[k], coef, LR[kind], B1, B2, EPS, WD, step)
            r["w"] = W.master(h, low)


def _ref_project(refs, R, scope):
    """The restated projection over one or several optimizers' tensors (one global ball, or per-tensor balls)."""
    sums = [T.sumsq([(r["w"], r["w0"]) for r in ref]) for ref in refs]
    total = T.joint_total([out[0] for _, out in sums])
    count = sum(r["w"].size for ref in refs for r in ref)
    traces = []
    for ref in refs:
        new, _, _, trace = T.project([(r["w"], r["w0"]) for r in ref], R, scope, total=total if scope == "global" else None,
                                     count=count if scope == "global" else None)
        for r, w in zip(ref, new):
            r["w"] = w
        traces.append(trace)
    return traces


def _compare(what, opt, params, ref, f32):
    for k, r in enumerate(ref):
        if f32:
            _report(what + " w", k, _bits_of(params[k]), W.bits(r["w"]))
        else:
            h, low = T.to_words(r["w"])
            _report(what + " h", k, _h_of(params[k]), h)
            _report(what + " l", k, opt.low_words[k].cpu().numpy().ravel(), low)


@pytest.mark.parametrize("scope", ["global", "tensor"])
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_optimizer_steps_with_max_drift_bits(kind, f32, scope):
    from lcv_hip import optim
    per_rms, all_rms = _rms("f32" if f32 else "bf16", True)
    R = float(np.sort(per_rms)[len(ALL) // 2]) * 1.0001 if scope == "tensor" else 0.9 * all_rms
    opt, params, anchors, ref = _make_opt(kind, f32)
    opt.enable_max_drift(R, scope, anchor=anchors, trace_len=2)
    coefs = []
    for step in range(3):
        _give(params, _grads()[step], f32)
        opt.clip_grad_norm_(1.0)
        coef = float(opt._norm_coef[1].item())
        opt.step()
        optim.project_max_drift([opt])
        torch.cuda.synchronize()
        _ref_step(kind, f32, ref, _grads()[step], coef, step + 1)
        (trace,) = _ref_project([ref], R, scope)
        what = f"{kind} f32={f32} {scope} step {step + 1}"
        _compare(what, opt, params, ref, f32)
        coefs.append(float(trace[1]))
        assert step or trace[1] < 1.0                                    # the first step leaves the ball for certain
        pairs = [(r["w"], r["w0"]) for r in ref]
        if scope == "global":
            assert T.bound_holds(pairs, T.radius2(R, sum(ALL)))
        else:
            assert all(T.bound_holds([p], T.radius2(R, n)) for p, n in zip(pairs, ALL))
        if step < 2:
            got = W.bits(opt.max_drift_trace().numpy()).ravel()[-2:]
            _report(what + " trace", -1, got, W.bits(np.array(trace, dtype=F)))
    assert opt.max_drift_trace().shape == (2, 2)                         # a full trace records no further step
    stats = optim.max_drift_stats([opt])
    assert stats["steps"] == 2 and stats["projections"] == sum(c < 1.0 for c in coefs[:2]) and stats["first_projected_step"] == 1
    assert stats["min_coef"] == min(coefs[:2]) and stats["radius"] == R and stats["scope"] == scope
    assert len(stats["drift_rms_trace"]) == 2 and (scope == "tensor" or stats["drift_rms_trace"][0] > R)
    assert abs(optim.max_drift_norm([opt]) - T.drift64([(r["w"], r["w0"]) for r in ref])) <= 1e-5 * optim.max_drift_norm([opt])


def test_two_optimizers_share_one_global_ball_and_the_average_takes_the_projected_masters():
    from lcv_hip import optim
    _, all_b = _rms("bf16", True)
    t = _table()
    zero_rms = math.sqrt(T.drift64([(W.master(h, low), np.zeros(h.size, F)) for h, low in zip(t["h"], t["l"])]) ** 2 / sum(ALL))
    R = 0.8 * math.sqrt((all_b ** 2 + zero_rms ** 2) / 2.0)              # below the joint RMS drift of both optimizers
    a, pa, anch, ra = _make_opt("adamw", False, ema=0.5)
    b, pb, none, rb = _make_opt("adamw", True, anchored=False)           # fp32 vectors around zero: anchor = None
    assert none is None
    a.enable_max_drift(R, "global", anchor=anch)
    b.enable_max_drift(R, "global")
    for step in range(3):
        for opt, params, f32 in ((a, pa, False), (b, pb, True)):
            _give(params, _grads()[step], f32)
            opt.clip_grad_norm_(1.0)
        coefs = [float(o._norm_coef[1].item()) for o in (a, b)]
        a.step()
        b.step()
        optim.project_max_drift([a, b])
        torch.cuda.synchronize()
        _ref_step("adamw", False, ra, _grads()[step], coefs[0], step + 1)
        _ref_step("adamw", True, rb, _grads()[step], coefs[1], step + 1)
        traces = _ref_project([ra, rb], R, "global")
        assert (step or traces[0][1] < 1.0) and traces[0] == traces[1]
        for r in ra:                                                    # the average follows the projected masters
            h, low = T.to_words(r["w"])
            r["e"] = E.update(h, low, r["e"], 0.5)
        what = f"joint step {step + 1}"
        _compare(what + " bf16", a, pa, ra, False)
        _compare(what + " fp32", b, pb, rb, True)
        for k, r in enumerate(ra):
            _report(what + " average", k, _bits_of(a.ema_tensors()[k]), r["e"])
        assert T.bound_holds([(r["w"], r["w0"]) for r in ra + rb], T.radius2(R, 2 * sum(ALL)), T.eps_s(ALL, optimizers=2))
        got = [W.bits(o.max_drift_trace().numpy()).ravel()[-2:] for o in (a, b)]
        assert np.array_equal(got[0], got[1])
        _report(what + " trace", -1, got[0], W.bits(np.array(traces[0], dtype=F)))


def test_enable_max_drift_refusals_on_the_device():
    from lcv_hip import ops, optim
    from lcv_hip.lib import LcvError
    bf = [torch.zeros(8, dtype=BF16, device=DEV)]
    f32 = [torch.zeros(8, dtype=torch.float32, device=DEV)]
    with pytest.raises(LcvError, match="needs master_weights=True"):
        ops.FusedAdamWClip(bf).enable_max_drift(1.0, anchor=[bf[0].clone()])
    with pytest.raises(LcvError, match="stochastic_rounding"):
        ops.FusedAdamWClip(bf, stochastic_rounding=True).enable_max_drift(1.0, anchor=[bf[0].clone()])
    with pytest.raises(LcvError, match="needs an anchor"):
        ops.FusedAdamWClip(bf, master_weights=True).enable_max_drift(1.0)
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(LcvError, match="must be > 0"):
            ops.FusedAdamWClip(f32).enable_max_drift(bad)
    with pytest.raises(LcvError, match="'global' or 'tensor'"):
        ops.FusedAdamWClip(f32).enable_max_drift(1.0, scope="layer")
    opt = ops.FusedSGDClip(f32)
    with pytest.raises(LcvError, match="needs enable_max_drift"):
        optim.project_max_drift([opt])
    opt.enable_max_drift(float("inf"))
    with pytest.raises(LcvError, match="already called"):
        opt.enable_max_drift(1.0)
    late = ops.FusedSGDClip(f32)
    f32[0].grad = torch.ones_like(f32[0])
    late.step()
    with pytest.raises(LcvError, match="before the first step"):
        late.enable_max_drift(1.0)
    # with a weight average too, step() leaves the update to project_max_drift(), which gives it to the optimizers that stepped
    both = ops.FusedSGDClip(bf, master_weights=True, anchor=[bf[0].clone()])
    both.enable_weight_ema(0.5)
    both.enable_max_drift(1.0)
    optim.project_max_drift([both])                                      # not stepped (no gradient): its average is left alone
    assert both._ema_t == 0
    bf[0].grad = torch.ones_like(bf[0])
    both.step()
    assert both._ema_t == 0
    optim.project_max_drift([both])
    assert both._ema_t == 1
    optim.project_max_drift([both])
    assert both._ema_t == 1
    bf[0].grad = None
    # an optimizer's own anchor= is reused
    own = ops.FusedSGDClip(bf, master_weights=True, anchor=[bf[0].clone()])
    own.enable_max_drift(1.0)
    assert own._md_anchor is own._anchor
    with pytest.raises(LcvError, match="same radius and scope"):
        optim.project_max_drift([own, opt])


# ---------------------------------------------------------------------------------------------------------- 4. the loops
_SHARED = {}


def _inputs():
    if not _SHARED:
        g = torch.Generator().manual_seed(7)
        r = lambda *s: torch.randn(*s, generator=g)
        _SHARED["cond"] = r(1, 16, 1, 10, 20).to(BF16).to(DEV)            # one conditioning latent frame: 5 x 10 tokens
        _SHARED["train"] = r(1, 16, 2, 10, 20).to(BF16).to(DEV)           # two target frames
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


STEPS = 4


def _delta_a(**flag):
    """Four delta-A steps from one seed on a fresh model; returns (loss bits, delta bits, result)."""
    from tta import delta as D
    i = _inputs()
    w = D.DeltaAWrapper(_dit(), adaln_tembed_dim=64).to(DEV)
    torch.manual_seed(1234)
    res = D.optimize_delta_a(w, i["cond"], i["train"], i["embeds"], i["mask"], num_steps=STEPS, lr=1e-2, device=DEV, dtype=BF16,
                             **flag)
    torch.cuda.synchronize()
    return [float(v).hex() for v in res["losses"]], _bits_of(w.delta), res


def _within(drift, R, count, theta_norm):
    """The bound of trust_ref's docstring for a REPORTED drift over a table of `count` elements whose parameters have the norm
    `theta_norm`: |theta' - theta0| <= R sqrt(N) (1 + eps_s) + 2^-24 |theta'|, and one more factor (1 + eps_s) because the report
    is the root of lcv_trust_sumsq's fp32 sum (every loop's `drift_norm` under max_drift comes from that kernel, whose reduction
    depth eps_s is derived from).  The same form covers tensor scope (Minkowski; the (1 + 2^-24)^1/2 of the per-tensor radii lies
    inside the margin between a table's eps_s, at most 68 * 2^-24 for the whole model, and EPS_S = 128 * 2^-24)."""
    return drift <= R * math.sqrt(count) * (1.0 + T.EPS_S) ** 2 + T.U * theta_norm


def test_delta_a_loop_keeps_the_ball_and_inf_changes_no_bit(deterministic):
    l0, d0, r0 = _delta_a()
    assert "max_drift" not in r0 and "drift_norm" not in r0 and len(l0) == STEPS
    free = r0["delta_norm"] / math.sqrt(64)
    li, di, ri = _delta_a(max_drift=float("inf"))
    assert li == l0 and np.array_equal(di, d0)                           # inf: no byte written, the same run
    m = ri["max_drift"]
    assert m["steps"] == STEPS and m["projections"] == 0 and m["first_projected_step"] is None and m["min_coef"] == 1.0
    assert len(m["drift_rms_trace"]) == STEPS and m["drift_rms_trace"][-1] == pytest.approx(free, rel=1e-5)
    assert ri["drift_norm"] == pytest.approx(r0["delta_norm"], rel=1e-5)
    for scope in ("global", "tensor"):
        R = 0.25 * free                                                  # a quarter of where the free run ends
        lr, dr, rr = _delta_a(max_drift=R, max_drift_scope=scope)
        m = rr["max_drift"]
        print(f"delta-A {scope}: free RMS {free!r}, R {R!r}, {m}")
        assert m["radius"] == R and m["scope"] == scope and m["steps"] == STEPS == len(m["drift_rms_trace"])
        assert m["projections"] > 0 and m["first_projected_step"] >= 1 and m["min_coef"] < 1.0
        assert _within(rr["delta_norm"], R, 64, rr["delta_norm"]) and _within(rr["drift_norm"], R, 64, rr["delta_norm"])
        assert lr[0] == l0[0] and not np.array_equal(dr, d0)             # the first loss is taken before any projection
        l2, d2, _ = _delta_a(max_drift=R, max_drift_scope=scope)
        assert l2 == lr and np.array_equal(d2, dr)                       # no atomics: the same run, the same bits


def test_delta_b_optimizers_share_one_global_ball(deterministic):
    """delta-B clips per parameter, so every group has an optimizer of its own: one joint total over all of them."""
    from tta import delta as D
    i = _inputs()

    def run(**flag):
        w = D.DeltaBWrapper(_dit(), num_groups=2, adaln_tembed_dim=64, hidden_size=256).to(DEV)
        torch.manual_seed(1234)
        res = D.optimize_delta_b(w, i["cond"], i["train"], i["embeds"], i["mask"], num_steps=STEPS, lr=1e-2, device=DEV, dtype=BF16,
                                 **flag)
        torch.cuda.synchronize()
        return res
    free = run()
    total = math.sqrt(sum(n * n for n in free["delta_norms"]))
    R = 0.25 * total / math.sqrt(128)
    got = run(max_drift=R)
    now = math.sqrt(sum(n * n for n in got["delta_norms"]))
    assert got["max_drift"]["projections"] > 0 and _within(now, R, 128, now) and _within(got["drift_norm"], R, 128, now)


def _norm_tune(also_delta=False, **flag):
    from tta import delta as D
    i = _inputs()
    w = D.NormTuneForward(_dit(), "all_norm", also_tune_delta=also_delta).to(DEV)
    torch.manual_seed(1234)
    res = D.optimize_norm_params(w, w.tuned_params, i["cond"], i["train"], i["embeds"], i["mask"], num_steps=STEPS, lr=1e-2,
                                 device=DEV, dtype=BF16, **flag)
    torch.cuda.synchronize()
    return res, w


@pytest.mark.parametrize("also_delta", [False, True])
def test_norm_tuning_loop_with_max_drift(also_delta, deterministic):
    from lcv_hip.lib import LcvError
    free, w = _norm_tune(also_delta, master_weights=True, max_drift=float("inf"))
    count = sum(p.numel() for p in w.tuned_params)
    R = 0.25 * free["drift_norm"] / math.sqrt(count)
    assert free["max_drift"]["projections"] == 0 and free["drift_norm"] > 0
    for extra in ({}, {"decay_to_base": True}, {"weight_ema": 0.5}):
        if also_delta and "weight_ema" in extra:
            continue                                                     # refused with the fp32 vector in the list, as before
        got, w = _norm_tune(also_delta, master_weights=True, max_drift=R, **extra)
        theta = math.sqrt(sum(float((p.detach().double() ** 2).sum()) for p in w.tuned_params))
        print(f"norm tuning also_delta={also_delta} {extra}: R {R!r} drift {got['drift_norm']!r} {got['max_drift']}")
        assert got["max_drift"]["projections"] > 0 and _within(got["drift_norm"], R, count, theta)
    with pytest.raises(LcvError, match="needs master_weights=True"):
        _norm_tune(also_delta, max_drift=R)


# ---------------------------------------------------------------------------------------------------------- 5. the runners
def _main(rel, argv):
    path = PKG / rel
    spec = importlib.util.spec_from_file_location("md_" + path.stem, path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    m.main(argv)


COMMON = ["--checkpoint-dir", "synthetic:2:256:64", "--data-dir", "synthetic:1", "--num-cond-frames", "5", "--num-frames", "13",
          "--gen-start-frame", "40", "--tta-total-frames", "33", "--tta-context-frames", "9", "--num-inference-steps", "2"]
DELTA_A = "delta_experiment/scripts/run_delta_a.py"


def test_delta_a_runner_with_the_early_stopper_records_the_ball(tmp_path):
    """The stopper on: what it scores, snapshots and restores are projected iterates."""
    R = 2e-3                                                             # AdamW at lr 1e-2 moves every element 1e-2 in step one
    argv = COMMON + ["--delta-steps", "4", "--delta-lr", "1e-2", "--es-check-every", "2", "--es-patience", "1", "--skip-generation"]
    _main(DELTA_A, argv + ["--output-dir", str(tmp_path / "on"), "--max-drift", str(R)])
    _main(DELTA_A, argv + ["--output-dir", str(tmp_path / "off")])
    s_on, s_off = (json.loads((tmp_path / d / "summary.json").read_text()) for d in ("on", "off"))
    r_on, r_off = s_on["results"][0], s_off["results"][0]
    assert r_on["success"] and r_off["success"]
    assert set(s_on) - set(s_off) == {"max_drift", "max_drift_scope"} and s_on["max_drift"] == R and s_on["max_drift_scope"] == "global"
    assert set(r_on) - set(r_off) == {"drift_norm", "max_drift"}
    m = r_on["max_drift"]
    assert set(m) == {"radius", "scope", "steps", "projections", "first_projected_step", "min_coef", "drift_rms_trace"}
    assert m["steps"] in (2, 4) and m["projections"] > 0 and m["first_projected_step"] == 1 and len(m["drift_rms_trace"]) == m["steps"]
    assert r_on["early_stopping_info"]["total_checks"] >= 1
    assert _within(r_on["delta_norm"], R, 512, r_on["delta_norm"]) and _within(r_on["drift_norm"], R, 512, r_on["delta_norm"])


def test_delta_a_runner_records_delta_steps_entries_and_inf_is_the_flagless_run(tmp_path, deterministic):
    """No stopper: the trace has one entry per step; under the same seed `--max-drift inf` gives the delta and the losses of a run
    without the flag (no byte is written) and still records the trace."""
    R = 2e-3
    argv = COMMON + ["--delta-steps", "4", "--delta-lr", "1e-2", "--es-disable", "--skip-generation"]
    rows = {}
    for name, flags in (("off", []), ("inf", ["--max-drift", "inf"]), ("on", ["--max-drift", str(R)])):
        _main(DELTA_A, argv + flags + ["--output-dir", str(tmp_path / name)])
        rows[name] = json.loads((tmp_path / name / "summary.json").read_text())["results"][0]
        assert rows[name]["success"]
    off, inf, on = rows["off"], rows["inf"], rows["on"]
    assert "max_drift" not in off and "drift_norm" not in off and off["delta_norm"] > 0
    assert inf["delta_norm"] == off["delta_norm"] and inf["final_loss"] == off["final_loss"]
    m = inf["max_drift"]
    assert m["steps"] == 4 == len(m["drift_rms_trace"]) and m["projections"] == 0 and m["first_projected_step"] is None
    assert m["min_coef"] == 1.0 and m["radius"] == float("inf")
    assert m["drift_rms_trace"][-1] == pytest.approx(off["delta_norm"] / math.sqrt(512), rel=1e-5)
    m = on["max_drift"]
    assert m["steps"] == 4 == len(m["drift_rms_trace"]) and m["projections"] > 0 and m["first_projected_step"] == 1
    assert off["delta_norm"] / math.sqrt(512) > R                        # the free run leaves the ball ...
    assert _within(on["delta_norm"], R, 512, on["delta_norm"]) and _within(on["drift_norm"], R, 512, on["delta_norm"])   # ... this one not
    assert on["final_loss"] != off["final_loss"]


def _synthetic_checkpoint_norm():
    """(|theta0|, elements) of the runners' `synthetic:2:256:64` checkpoint, built the way tta.runner_common.load_components does."""
    from longcat_video.modules.longcat_video_dit import LongCatVideoTransformer3DModel
    dit = LongCatVideoTransformer3DModel(device=DEV, dtype=BF16, depth=2, hidden_size=256, num_heads=2,
                                         caption_channels=64).init_synthetic_(1234)
    ps = list(dit.parameters())
    return math.sqrt(sum(float((p.detach().double() ** 2).sum()) for p in ps)), sum(p.numel() for p in ps)


@pytest.mark.parametrize("rel, extra, radius", [
    ("lora_experiment/scripts/run_lora_tta.py", ["--num-steps", "4", "--lora-rank", "4", "--lora-alpha", "8", "--save-lora-weights"],
     2e-5),
    ("lora_experiment/scripts/run_full_tta.py", ["--num-steps", "4", "--learning-rate", "1e-1"], 2e-5),
])
def test_lora_and_full_runners_stay_within_the_bound(tmp_path, rel, extra, radius):
    """No early stopper: its restore zeroes the low words, which moves a master by up to half a bf16 ulp.  |theta'| of the bound
    is the real one: the norm of the adapters the LoRA run saved (their bf16 words: within 2^-9 relative of the masters), and
    for the full model |theta0| of the synthetic checkpoint plus the drift, an upper bound on |theta'|."""
    _main(rel, COMMON + extra + ["--output-dir", str(tmp_path), "--master-weights", "--max-drift", str(radius), "--max-drift-scope",
                                 "tensor", "--es-disable", "--skip-generation"])
    cfg = json.loads((tmp_path / "config.json").read_text())
    row = json.loads((tmp_path / "summary.json").read_text())["results"][0]
    assert cfg["training"]["max_drift"] == radius and cfg["training"]["max_drift_scope"] == "tensor"
    m = row["max_drift"]
    assert row["success"] and m["steps"] == 4 and m["scope"] == "tensor" and m["projections"] > 0
    if "lora" in cfg:
        count = cfg["lora"]["trainable_params"]
        saved = torch.load(next((tmp_path / "lora_weights").glob("*_lora.pt")))
        assert sum(t.numel() for t in saved.values()) == count
        theta = math.sqrt(sum(float((t.double() ** 2).sum()) for t in saved.values())) * (1.0 + 2.0 ** -9)
    else:
        count = cfg["training"]["trainable_params"]
        theta0, n0 = _synthetic_checkpoint_norm()
        assert n0 == count
        theta = theta0 + row["drift_norm"] * (1.0 + T.EPS_S)
    slack = T.U * theta / (radius * math.sqrt(count))
    print(f"{Path(rel).stem}: {count} elements, |theta'| <= {theta!r}, drift_norm {row['drift_norm']!r} against R sqrt(N) "
          f"{radius * math.sqrt(count)!r} (the 2^-24 |theta'| term is {slack:.2e} of it), {m['projections']} of {m['steps']} steps "
          f"projected, min coef {m['min_coef']!r}")
    # per-tensor balls of RMS radius R add up to at most R sqrt(N)
    assert _within(row["drift_norm"], radius, count, theta)

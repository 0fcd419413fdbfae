"""GPU: the sharpness-aware adaptation step (include/lcv_hip_sam.h, `enable_sam` / `sam_perturb` / `sam_restore` / `--sam-rho`).

1. lcv_sam_sumsq at the C ABI against the numpy restatement (tests/sam_ref.py), bit for bit on per_tensor and out: bf16 words
   with low words, bf16 words with low = NULL, fp32 values; plain and adaptive with eta 0.01 and 0; run-to-run bits.  The tensor
   set is test_gpu_max_drift's: a single element, a sub-packet tail, a quarter chunk, one element past it, an exact chunk, one
   element past a chunk (every array of it a one-element offset view: the scalar path), a tail past two chunks, and a
   300-element parameter that never gets a gradient.  Every array sits between guard elements.
2. lcv_sam_perturb bit for bit on the words, the saves, realized and the trace slot; the low words byte-identical; a rho at which
   some bf16 perturbations round away and some do not, a large rho, a joint total from two tables; rho = 0, a zero total and a
   NaN total write the saves and no parameter byte.
3. lcv_sam_restore: every parameter buffer byte-identical to its state before the perturbation.  Refusals.
4. Through the optimizers: three AdamW and three SGD steps with sam_perturb / sam_restore against the restatement; two
   optimizers under one norm; the state guards; a weight average and a ball on top.
5. Stale caches: the second pass reads the perturbed words (LoRA adapters, and the full model with its SwiGLU cache).
6. rho = 0 changes no bit of the LoRA, delta-A, norm-tuning and full-model loops.
7. The runners on the smallest synthetic checkpoint.
"""
import json
import math

import numpy as np
import pytest
import torch

import ema_ref as E
import master_weights_ref as W
import optim_ref as O
import sam_ref as S
import trust_ref as T
import test_gpu_max_drift as M
from test_gpu_max_drift import deterministic  # noqa: F401  (a fixture: fixed-order reductions on, put back afterwards)

pytestmark = pytest.mark.gpu
BF16, DEV, F = torch.bfloat16, "cuda", np.float32
NUMELS, ALL, VIEW = M.NUMELS, M.ALL, M.VIEW
LIVE = len(NUMELS)            # the tensors that hold a gradient; the eighth (300 elements) never does
MODES = ("bf16", "bf16_nolow", "f32")
FORMS = [(False, 0.01), (True, 0.01), (True, 0.0)]
_report, _call, _Arr = M._report, M._call, M._Arr


# ---------------------------------------------------------------------------------------------------------- helpers
def _ref_tensors(mode, zero_grad=False):
    """What the restatement sees: the tensors that hold a gradient."""
    t, g = M._table(), M._grads()[0]
    out = []
    for k in range(LIVE):
        gk = np.zeros_like(g[k]) if zero_grad else g[k]
        if mode == "f32":
            out.append({"w": W.master(t["h"][k], t["l"][k]), "g": W.bf16_to_f32(gk)})
        else:
            out.append({"h": t["h"][k], "low": t["l"][k] if mode == "bf16" else None, "g": gk})
    return out


class _Dev:
    """The same tensors on the device with the descriptor table (the gradient column filled) and the side arrays of the C ABI."""

    def __init__(self, mode, zero_grad=False):
        t, g = M._table(), M._grads()[0]
        self.mode, self.f32 = mode, mode == "f32"
        self.P, self.L, self.G, self.S = [], [], [], []
        for k in range(len(ALL)):
            off = k == VIEW
            self.P.append(_Arr("f", W.master(t["h"][k], t["l"][k]), off) if self.f32 else _Arr("h", t["h"][k], off))
            if mode == "bf16":
                self.L.append(_Arr("l", t["l"][k], off))
            if k < LIVE:
                gk = np.zeros_like(g[k]) if zero_grad else g[k]
                self.G.append(_Arr("f", W.bf16_to_f32(gk), off) if self.f32 else _Arr("h", gk, off))
                self.S.append(_Arr("f", np.full(ALL[k], 7.0, F), off) if self.f32 else _Arr("h", np.full(ALL[k], 0x4100, np.uint16), off))
        rows, chunk = [], 0
        for p, gr in zip(self.P[:LIVE], self.G):
            rows.append([p.ptr(), gr.ptr(), 0, 0, p.n, chunk])
            chunk += (p.n + M.CHUNK - 1) // M.CHUNK
        self.n, self.chunks = len(rows), chunk
        self.table = torch.tensor(rows, dtype=torch.int64).to(DEV)
        self.lp = torch.tensor([x.ptr() for x in self.L[:LIVE]], dtype=torch.int64).to(DEV) if self.L else None
        self.sp = torch.tensor([x.ptr() for x in self.S], dtype=torch.int64).to(DEV)
        self.part = torch.full((chunk + 1,), -7.0, dtype=torch.float32, device=DEV)
        self.per = torch.full((self.n + 1,), -7.0, dtype=torch.float32, device=DEV)
        self.out = torch.full((3,), -7.0, dtype=torch.float32, device=DEV)
        self.real = torch.full((3,), -7.0, dtype=torch.float32, device=DEV)
        self.trace = torch.full((4,), -7.0, dtype=torch.float32, device=DEV)

    def low(self):
        return None if self.lp is None else self.lp.data_ptr()

    def sumsq(self, adaptive, eta):
        _call("lcv_sam_sumsq", self.table.data_ptr(), self.low(), self.n, self.chunks, 1 if self.f32 else 0, int(adaptive), eta,
              self.part.data_ptr(), self.chunks * 4, self.per.data_ptr(), self.out.data_ptr())
        torch.cuda.synchronize()
        for buf in (self.part, self.per, self.out):
            assert float(buf[-1].item()) == -7.0                         # nothing written past the workspace and the outputs
        return W.bits(self.per[:-1].cpu().numpy()), W.bits(self.out[:2].cpu().numpy())

    def perturb(self, adaptive, eta, rho, sumsq=None):
        _call("lcv_sam_perturb", self.table.data_ptr(), self.low(), self.sp.data_ptr(), self.n, self.chunks, 1 if self.f32 else 0,
              int(adaptive), eta, rho, (self.out if sumsq is None else sumsq).data_ptr(), self.part.data_ptr(), self.chunks * 4,
              self.per.data_ptr(), self.real.data_ptr(), self.trace[1:3].data_ptr())
        torch.cuda.synchronize()
        for buf in (self.part, self.per, self.real):
            assert float(buf[-1].item()) == -7.0
        assert float(self.trace[0].item()) == -7.0 and float(self.trace[3].item()) == -7.0
        return W.bits(self.real[:2].cpu().numpy()), W.bits(self.trace[1:3].cpu().numpy())

    def restore(self):
        _call("lcv_sam_restore", self.table.data_ptr(), self.sp.data_ptr(), self.n, self.chunks, 1 if self.f32 else 0)
        torch.cuda.synchronize()

    def arrays(self):
        return self.P + self.L + self.G + self.S


def _check_guards(d, what):
    for a in d.arrays():
        raw, lo = a.raw(), a.lo
        want = a.host.view(raw.dtype)
        assert np.array_equal(raw[:lo], want[:lo]) and np.array_equal(raw[lo + a.n:], want[lo + a.n:]), f"{what}: a guard was written"


def _word_bits(x):
    return W.bits(x) if np.asarray(x).dtype == np.float32 else np.asarray(x, dtype=np.uint16)


# ---------------------------------------------------------------------------------------------------------- 1. the sum
@pytest.mark.parametrize("adaptive, eta", FORMS)
@pytest.mark.parametrize("mode", MODES)
def test_sam_sumsq(mode, adaptive, eta):
    d = _Dev(mode)
    per, out = d.sumsq(adaptive, eta)
    want_per, want_out = S.sumsq(_ref_tensors(mode), adaptive, eta)
    assert d.chunks == 10 and d.n == LIVE
    what = f"{mode} adaptive={adaptive} eta={eta}"
    _report(what + " per_tensor", -1, per, W.bits(want_per))
    _report(what + " out", -1, out, W.bits(want_out))
    assert want_out[0] > 0 and np.all(want_per > 0) and want_out[1] == np.sqrt(want_out[0])
    again_per, again_out = d.sumsq(adaptive, eta)
    assert np.array_equal(per, again_per) and np.array_equal(out, again_out)          # same inputs, same bits
    assert all(a.pristine() for a in d.arrays())                                       # the sum writes no array, guards included
    if mode == "bf16_nolow" and adaptive:           # low = NULL is "all low words zero"
        z = _Dev("bf16")
        for a in z.L:
            a.view.zero_()
        zp, zo = z.sumsq(adaptive, eta)
        assert np.array_equal(zp, per) and np.array_equal(zo, out)
    if not adaptive:                                # plain: the parameters are not read, so the form of w does not matter
        assert np.array_equal(out, W.bits(S.sumsq(_ref_tensors("bf16_nolow" if mode != "f32" else "f32"))[1]))


# ---------------------------------------------------------------------------------------------------------- 2. the perturbation
def _compare_perturbed(what, d, got_real, got_trace, want):
    _report(what + " realized", -1, got_real, W.bits(want["realized"]))
    _report(what + " trace", -1, got_trace, W.bits(np.array(want["trace"], dtype=F)))
    _check_guards(d, what)
    for k in range(LIVE):
        _report(what + " save", k, d.S[k].values(), _word_bits(want["saves"][k]))
        if want["wrote"]:
            _report(what + " word", k, d.P[k].values(), _word_bits(want["words"][k]))
        else:
            assert d.P[k].pristine(), (what, k)
    assert d.P[LIVE].pristine()                                           # the idle parameter is in no table
    assert all(a.pristine() for a in d.L + d.G)                           # low words and gradients: read, never written


@pytest.mark.parametrize("rho", [0.05, 50.0])
@pytest.mark.parametrize("adaptive, eta", FORMS)
@pytest.mark.parametrize("mode", MODES)
def test_sam_perturb(mode, adaptive, eta, rho):
    ref = _ref_tensors(mode)
    want = S.perturb(ref, rho, adaptive, eta)
    what = f"{mode} adaptive={adaptive} eta={eta} rho={rho}"
    d = _Dev(mode)
    d.sumsq(adaptive, eta)
    real, trace = d.perturb(adaptive, eta, rho)
    _compare_perturbed(what, d, real, trace, want)
    total = sum(ALL[:LIVE])
    moved = sum(int(np.count_nonzero(_word_bits(w) != _word_bits(t["w" if mode == "f32" else "h"]))) for w, t in zip(want["words"], ref))
    print(f"{what}: {moved} of {total} words moved, realized {float(want['realized'][1])!r}")
    if mode != "f32" and rho == 0.05:
        assert 0 < moved < total                                          # some perturbations round away, some do not
    if rho == 50.0:
        small = S.perturb(ref, 0.05, adaptive, eta)
        assert want["realized"][1] > small["realized"][1] and np.isfinite(want["realized"][1])
    if mode == "f32" and not adaptive:                                    # fp32 words hold rho, to the derived bound
        theta = S.norm64(want["words"])
        assert abs(float(want["realized"][1]) - float(F(rho))) <= float(F(rho)) * S.eps_realized(ALL[:LIVE]) + T.U * theta
    # 3. the restore: every parameter buffer, guards included, is what it was
    d.restore()
    assert all(a.pristine() for a in d.P + d.L + d.G)
    _check_guards(d, what + " restore")


def test_sam_perturb_with_a_joint_total_from_two_tables():
    a, b = _Dev("bf16"), _Dev("f32")
    a.sumsq(False, 0.01)
    b.sumsq(False, 0.01)
    joint = a.out[:1].clone()
    joint += b.out[0]
    torch.cuda.synchronize()
    ra, rb = _ref_tensors("bf16"), _ref_tensors("f32")
    total = S.joint_total([S.sumsq(ra)[1][0], S.sumsq(rb)[1][0]])
    assert W.bits(joint.cpu().numpy())[0] == W.bits(np.array([total], dtype=F))[0]
    for d, ref, name in ((a, ra, "bf16"), (b, rb, "f32")):
        real, trace = d.perturb(False, 0.01, 0.25, sumsq=joint)
        want = S.perturb(ref, 0.25, total=total)
        assert want["trace"][0] == total and want["wrote"]
        _compare_perturbed("joint " + name, d, real, trace, want)
    # the two tables' realized sums add up to at most rho^2 for the fp32 part plus what bf16 rounding made of the rest; the fp32
    # table alone moved by less than rho, because the norm is shared
    assert float(b.real[1].item()) < 0.25


@pytest.mark.parametrize("case", ["rho0", "zero_total", "nan_total", "inf_total"])
@pytest.mark.parametrize("mode", MODES)
def test_sam_perturb_writes_the_saves_and_no_parameter_byte(mode, case):
    for adaptive in (False, True):
        d = _Dev(mode, zero_grad=case == "zero_total")
        d.sumsq(adaptive, 0.01)
        ref = _ref_tensors(mode, zero_grad=case == "zero_total")
        rho, given, total = 0.05, None, None
        if case == "rho0":
            rho = 0.0
        elif case in ("nan_total", "inf_total"):
            total = F(np.nan) if case == "nan_total" else F(np.inf)
            given = torch.full((2,), float(total), dtype=torch.float32, device=DEV)
        real, trace = d.perturb(adaptive, 0.01, rho, sumsq=given)
        want = S.perturb(ref, rho, adaptive, 0.01, total=total)
        assert not want["wrote"] and not real.any()                       # realized is +0
        what = f"{mode} {case} adaptive={adaptive}"
        if case == "nan_total":
            assert np.isnan(W.floats(trace[:1])[0]) and trace[1] == 0
            want = dict(want, trace=(W.floats(trace[:1])[0], F(0)))       # a NaN's payload is not compared
            _report(what + " realized", -1, real, W.bits(want["realized"]))
        else:
            _report(what + " trace", -1, trace, W.bits(np.array(want["trace"], dtype=F)))
        for k in range(LIVE):
            _report(what + " save", k, d.S[k].values(), _word_bits(want["saves"][k]))
        assert all(a.pristine() for a in d.P + d.L + d.G), what           # every parameter buffer byte-identical, guards included
        _check_guards(d, what)
        d.restore()                                                      # the saves hold the words: a restore changes nothing
        assert all(a.pristine() for a in d.P + d.L + d.G), what


def test_sam_bad_arguments_are_refused():
    from lcv_hip.lib import LcvError
    t = torch.zeros(8, dtype=torch.int64, device=DEV).data_ptr()
    nan, inf = float("nan"), float("inf")
    cases = [("lcv_sam_sumsq", a) for a in (
        (None, t, 1, 1, 0, 0, 0.01, t, 4, t, t), (t, t, 0, 1, 0, 0, 0.01, t, 4, t, t), (t, t, 1, 0, 0, 0, 0.01, t, 4, t, t),
        (t, t, 1, 1, 1, 0, 0.01, t, 4, t, t),                                                    # fp32 parameters take no low words
        (t, t, 1, 1, 0, 1, -0.01, t, 4, t, t), (t, t, 1, 1, 0, 1, nan, t, 4, t, t), (t, t, 1, 1, 0, 1, inf, t, 4, t, t),
        (t, t, 1, 1, 0, 0, 0.01, None, 4, t, t), (t, t, 1, 3, 0, 0, 0.01, t, 8, t, t),           # a workspace too small
        (t, t, 1, 1, 0, 0, 0.01, t, 4, None, t), (t, t, 1, 1, 0, 0, 0.01, t, 4, t, None))]
    cases += [("lcv_sam_perturb", a) for a in (
        (None, t, t, 1, 1, 0, 0, 0.01, 0.1, t, t, 4, t, t, None), (t, t, None, 1, 1, 0, 0, 0.01, 0.1, t, t, 4, t, t, None),
        (t, t, t, 0, 1, 0, 0, 0.01, 0.1, t, t, 4, t, t, None), (t, t, t, 1, 0, 0, 0, 0.01, 0.1, t, t, 4, t, t, None),
        (t, t, t, 1, 1, 1, 0, 0.01, 0.1, t, t, 4, t, t, None),                                   # fp32 values with low words
        (t, t, t, 1, 1, 0, 0, 0.01, -0.1, t, t, 4, t, t, None), (t, t, t, 1, 1, 0, 0, 0.01, nan, t, t, 4, t, t, None),
        (t, t, t, 1, 1, 0, 0, 0.01, inf, t, t, 4, t, t, None),
        (t, t, t, 1, 1, 0, 1, -1.0, 0.1, t, t, 4, t, t, None), (t, t, t, 1, 1, 0, 1, nan, 0.1, t, t, 4, t, t, None),
        (t, t, t, 1, 1, 0, 0, 0.01, 0.1, None, t, 4, t, t, None), (t, t, t, 1, 3, 0, 0, 0.01, 0.1, t, t, 8, t, t, None),
        (t, t, t, 1, 1, 0, 0, 0.01, 0.1, t, None, 4, t, t, None), (t, t, t, 1, 1, 0, 0, 0.01, 0.1, t, t, 4, t, None, None))]
    cases += [("lcv_sam_restore", a) for a in ((None, t, 1, 1, 0), (t, None, 1, 1, 0), (t, t, 0, 1, 0), (t, t, 1, 0, 1))]
    for name, args in cases:
        with pytest.raises(LcvError) as e:
            _call(name, *args)
        assert e.value.code == -1 and not e.value.fatal, (name, args)


# ---------------------------------------------------------------------------------------------------------- 4. the optimizers
LR, WD, B1, B2, EPS = {"sgd": 2e-2, "adamw": 1e-2}, 0.01, 0.9, 0.999, 1e-8
_COEF = {}


def _coefs():
    """Per tensor a power of two per element, 2^-3 .. 2^3: the loss 0.5 sum c p^2 has the gradient c p, exact in fp32 and in bf16
    for a bf16 p, whatever order autograd multiplies in - so numpy reproduces the gradient's bits."""
    if not _COEF:
        rng = np.random.default_rng(71)
        _COEF["c"] = [np.exp2(rng.integers(-3, 4, size=n)).astype(F) for n in NUMELS]
    return _COEF["c"]


def _make(kind, form):
    """An optimizer over the table's tensors as leaf parameters (the eighth never gets a gradient) and the restatement's state.
    form: "master" (bf16 + low words), "bf16" (plain), "f32"."""
    from lcv_hip import ops
    t = M._table()
    params, ref = [], []
    for k in range(len(ALL)):
        if form == "f32":
            p = torch.from_numpy(W.master(t["h"][k], t["l"][k]).copy()).to(DEV)
        else:
            p = M._bf16_dev(t["h"][k])
        p = M._offset_view(p) if k == VIEW else p
        params.append(p.requires_grad_(True))
        w = W.master(t["h"][k], t["l"][k]) if form != "bf16" else W.bf16_to_f32(t["h"][k])
        ref.append(dict(w=w, m=np.zeros(ALL[k], F), v=np.zeros(ALL[k], F)))
    if form == "bf16":
        for r in ref:
            r["m"], r["v"] = np.zeros(r["w"].size, np.uint16), np.zeros(r["w"].size, np.uint16)
    kw = dict(weight_decay=WD, master_weights=form == "master")
    opt = (ops.FusedSGDClip(params, lr=LR[kind], **kw) if kind == "sgd"
           else ops.FusedAdamWClip(params, lr=LR[kind], betas=(B1, B2), eps=EPS, **kw))
    if form == "master":
        opt._low[VIEW] = M._offset_view(opt._low[VIEW])
        for lw, low in zip(opt.low_words, t["l"]):
            lw.copy_(torch.from_numpy(low.copy()).to(DEV))
    return opt, params, ref


def _backward(params):
    """The toy quadratic loss over the tensors that get a gradient."""
    loss = sum((torch.from_numpy(c).to(DEV) * p.float().pow(2)).sum() for c, p in zip(_coefs(), params[:LIVE])) * 0.5
    loss.backward()
    return loss.detach()


def _read(form, r):
    """What the forward reads of a restated tensor: the fp32 value, or the bf16 word of the master."""
    return r["w"] if form == "f32" else W.bf16_to_f32(T.to_words(r["w"])[0])


def _ref_grad(form, c, read):
    g = (c * read).astype(F)                                             # exact: c is a power of two
    return g if form == "f32" else W.to_bf16_bits(g)


def _ref_tensor(form, r, g):
    if form == "f32":
        return {"w": r["w"], "g": g}
    h, low = T.to_words(r["w"])
    return {"h": h, "low": low if form == "master" else None, "g": g}


def _ref_sam_gradients(form, refs, rho, adaptive, eta):
    """First-pass gradients, the joint perturbation over `refs` (one list per optimizer), second-pass gradients at the perturbed
    words.  Returns (per optimizer the second gradients, the per-optimizer restated perturbations)."""
    firsts = [[_ref_tensor(f, r, _ref_grad(f, c, _read(f, r))) for r, c in zip(ref[:LIVE], _coefs())] for f, ref in zip(form, refs)]
    total = S.joint_total([S.sumsq(ts, adaptive, eta)[1][0] for ts in firsts])
    seconds, pert = [], []
    for f, ts in zip(form, firsts):
        want = S.perturb(ts, rho, adaptive, eta, total=total)
        pert.append(want)
        seconds.append([_ref_grad(f, c, wd if f == "f32" else W.bf16_to_f32(wd)) for wd, c in zip(want["words"], _coefs())])
    return seconds, pert


def _ref_step(kind, form, ref, gs, coef, step):
    for k in range(LIVE):
        r = ref[k]
        if form == "f32":
            if kind == "sgd":
                r["w"] = O.sgd_step_f32(r["w"], gs[k], coef, LR[kind], WD)
            else:
                r["w"], r["m"], r["v"] = O.adamw_step_f32(r["w"], r["m"], r["v"], gs[k], coef, LR[kind], B1, B2, EPS, WD, step)
        elif form == "master":
            h, low = T.to_words(r["w"])
            if kind == "sgd":
                h, low = W.sgd_step(h, low, gs[k], coef, LR[kind], WD)
            else:
                h, low, r["m"], r["v"] = W.adamw_step(h, low, r["m"], r["v"], gs[k], coef, LR[kind], B1, B2, EPS, WD, step)
            r["w"] = W.master(h, low)
        else:
            h = W.to_bf16_bits(r["w"])
            if kind == "sgd":
                h = O.sgd_step_bf16(h, gs[k], coef, LR[kind], WD)
            else:
                h, r["m"], r["v"] = O.adamw_step_bf16(h, r["m"], r["v"], gs[k], coef, LR[kind], B1, B2, EPS, WD, step)
            r["w"] = W.bf16_to_f32(h)


def _compare(what, opt, params, ref, form):
    for k, r in enumerate(ref):
        if form == "f32":
            _report(what + " w", k, M._bits_of(params[k]), W.bits(r["w"]))
        else:
            h, low = T.to_words(r["w"])
            _report(what + " h", k, M._h_of(params[k]), h)
            if form == "master":
                _report(what + " l", k, opt.low_words[k].cpu().numpy().ravel(), low)


def _sam_step(opts, params_of):
    """One sharpness-aware step on the device up to the clip: backward, perturb, drop the gradients, backward, restore."""
    from lcv_hip import optim
    for params in params_of:
        _backward(params)
    optim.sam_perturb(opts)
    during = [[M._bits_of(p) if p.dtype == torch.float32 else M._h_of(p) for p in params] for params in params_of]
    for o in opts:
        o.zero_grad()
    for params in params_of:
        _backward(params)
    optim.sam_restore(opts)
    return during


@pytest.mark.parametrize("adaptive", [False, True])
@pytest.mark.parametrize("form", ["master", "bf16", "f32"])
@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_optimizer_steps_with_sam_bits(kind, form, adaptive):
    from lcv_hip import ops, optim
    rho, eta = 0.5, 0.01
    opt, params, ref = _make(kind, form)
    opt.enable_sam(rho, adaptive, eta, trace_len=2)
    before_epoch = ops.PARAM_EPOCH
    for step in range(3):
        opt.zero_grad()
        (seconds,), (pert,) = _ref_sam_gradients([form], [ref], rho, adaptive, eta)
        (during,) = _sam_step([opt], [params])
        what = f"{kind} {form} adaptive={adaptive} step {step + 1}"
        for k in range(LIVE):                                            # the perturbed words the second pass read
            _report(what + " perturbed", k, during[k], _word_bits(pert["words"][k]))
        _compare(what + " restored", opt, params, ref, form)              # bit-identical parameters go to the optimizer
        for k in range(LIVE):                                            # ... with the gradient taken at the perturbed point
            got = M._bits_of(params[k].grad) if form == "f32" else M._h_of(params[k].grad)
            _report(what + " second gradient", k, got, _word_bits(seconds[k]))
        opt.clip_grad_norm_(1.0)
        coef = float(opt._norm_coef[1].item())
        opt.step()
        torch.cuda.synchronize()
        _ref_step(kind, form, ref, seconds, coef, step + 1)
        _compare(what, opt, params, ref, form)
        if step < 2:
            got = W.bits(opt.sam_trace().numpy()).ravel()[-2:]
            _report(what + " trace", -1, got, W.bits(np.array(pert["trace"], dtype=F)))
    assert ops.PARAM_EPOCH == before_epoch + 3 * 3                        # perturb, restore and step each bump the epoch
    assert opt.sam_trace().shape == (2, 2)                                # a full trace records no further step
    stats = optim.sam_stats([opt])
    assert stats["rho"] == rho and stats["adaptive"] is adaptive and stats["eta"] == eta and stats["steps"] == 2
    assert len(stats["grad_norm_trace"]) == len(stats["realized_norm_trace"]) == 2 and all(v > 0 for v in stats["grad_norm_trace"])
    if form == "f32" and not adaptive:
        theta = S.norm64([r["w"] for r in ref])
        assert all(v <= rho * (1.0 + S.eps_realized(ALL[:LIVE])) + T.U * theta for v in stats["realized_norm_trace"])
    assert params[LIVE].grad is None and not opt.sam_perturbed


def test_two_optimizers_share_one_norm_with_a_weight_average_and_a_ball():
    """A master-weight bf16 AdamW with a weight average and a ball, and an fp32 AdamW, perturbed under one joint norm."""
    from lcv_hip import optim
    rho = 0.5
    a, pa, ra = _make("adamw", "master")
    b, pb, rb = _make("adamw", "f32")
    anchors = [M._bf16_dev(h) for h in M._table()["h0"]]
    anchors[VIEW] = M._offset_view(anchors[VIEW])
    for r, h0 in zip(ra, M._table()["h0"]):
        r["w0"] = W.bf16_to_f32(h0)
        r["e"] = W.bits(r["w"]).copy()
    R = 0.9 * math.sqrt(T.drift64([(r["w"], r["w0"]) for r in ra]) ** 2 / sum(ALL))
    a.enable_weight_ema(0.5)
    a.enable_max_drift(R, "global", anchor=anchors)
    for o in (a, b):
        o.enable_sam(rho)
    for step in range(3):
        for o in (a, b):
            o.zero_grad()
        seconds, pert = _ref_sam_gradients(["master", "f32"], [ra, rb], rho, False, 0.01)
        assert pert[0]["trace"][0] == pert[1]["trace"][0]                 # one norm
        during = _sam_step([a, b], [pa, pb])
        what = f"joint step {step + 1}"
        for d, p, name in zip(during, pert, ("bf16", "fp32")):
            for k in range(LIVE):
                _report(f"{what} perturbed {name}", k, d[k], _word_bits(p["words"][k]))
        for o in (a, b):
            o.clip_grad_norm_(1.0)
        coefs = [float(o._norm_coef[1].item()) for o in (a, b)]
        a.step()
        b.step()
        optim.project_max_drift([a])
        torch.cuda.synchronize()
        _ref_step("adamw", "master", ra, seconds[0], coefs[0], step + 1)
        _ref_step("adamw", "f32", rb, seconds[1], coefs[1], step + 1)
        new, _, _, trace = T.project([(r["w"], r["w0"]) for r in ra], R, "global")
        for r, w in zip(ra, new):
            r["w"] = w
            r["e"] = E.update(*T.to_words(w), r["e"], 0.5)
        _compare(what + " bf16", a, pa, ra, "master")
        _compare(what + " fp32", b, pb, rb, "f32")
        for k, r in enumerate(ra):
            _report(what + " average", k, M._bits_of(a.ema_tensors()[k]), r["e"])
        _report(what + " ball trace", -1, W.bits(a.max_drift_trace().numpy()).ravel()[-2:], W.bits(np.array(trace, dtype=F)))
        got = [W.bits(o.sam_trace().numpy())[-1] for o in (a, b)]
        for g, p in zip(got, pert):
            _report(what + " sam trace", -1, g, W.bits(np.array(p["trace"], dtype=F)))
    stats = optim.sam_stats([a, b])
    assert stats["steps"] == 3 and stats["grad_norm_trace"][-1] == math.sqrt(float(pert[0]["trace"][0]))
    assert stats["realized_norm_trace"][-1] == math.sqrt(float(pert[0]["trace"][1]) + float(pert[1]["trace"][1]))


def test_sam_state_guards():
    from lcv_hip import ops, optim
    from lcv_hip.lib import LcvError
    opt, params, _ = _make("sgd", "master")
    anchors = [p.detach().clone() for p in params]
    opt.enable_weight_ema(0.5)
    opt.enable_max_drift(1.0, anchor=anchors)
    with pytest.raises(LcvError, match="needs enable_sam"):
        optim.sam_perturb([opt])
    opt.enable_sam(0.1)
    with pytest.raises(LcvError, match="already called"):
        opt.enable_sam(0.1)
    with pytest.raises(LcvError, match="not perturbed"):
        optim.sam_restore([opt])                                          # without a perturbation
    with pytest.raises(LcvError, match="no parameter has a gradient"):
        optim.sam_perturb([opt])
    _backward(params)
    optim.sam_perturb([opt])
    assert opt.sam_perturbed
    for call, name in ((lambda: opt.step(), "step"), (lambda: opt.clip_grad_norm_(1.0), "clip_grad_norm_"),
                       (lambda: opt.ema_swap(), "ema_swap"), (lambda: optim.sam_perturb([opt]), "sam_perturb"),
                       (lambda: optim.project_max_drift([opt]), "project_max_drift")):
        with pytest.raises(LcvError, match=f"{name}.. while the parameters are perturbed"):
            call()
    optim.sam_restore([opt])
    with pytest.raises(LcvError, match="not perturbed"):
        optim.sam_restore([opt])                                          # twice
    opt.ema_swap()
    with pytest.raises(LcvError, match="sam_perturb.. while the parameters hold the weight average"):
        optim.sam_perturb([opt])
    opt.ema_swap()
    other = ops.FusedSGDClip([torch.zeros(8, device=DEV)])
    other.enable_sam(0.2)
    with pytest.raises(LcvError, match="same rho, adaptive and eta"):
        optim.sam_perturb([opt, other])
    late = ops.FusedSGDClip([torch.zeros(8, device=DEV, requires_grad=True)])
    late.params[0].grad = torch.ones(8, device=DEV)
    late.step()
    with pytest.raises(LcvError, match="before the first step"):
        late.enable_sam(0.1)
    with pytest.raises(LcvError, match="grad_accum > 1"):
        ops.FusedSGDClip([torch.zeros(8, dtype=BF16, device=DEV)], master_weights=True, grad_accum=2).enable_sam(0.1)


# ---------------------------------------------------------------------------------------------------------- 5. stale caches
def _lora_model():
    from tta.lora import get_lora_parameters, inject_lora_into_dit
    dit = M._dit()
    for p in dit.parameters():
        p.requires_grad = False
    torch.manual_seed(3)
    mods = inject_lora_into_dit(dit, rank=4, alpha=8.0, target_modules=["qkv", "proj"], target_ffn=False, target_blocks="all")
    params = get_lora_parameters(mods)
    with torch.no_grad():                                                 # B starts at zero: give the adapters something to do
        g = torch.Generator().manual_seed(9)
        for p in params:
            p.copy_((torch.randn(p.shape, generator=g) * 0.05).to(BF16))
    return dit, mods, params


def _full_model():
    dit = M._dit()
    for p in dit.parameters():
        p.requires_grad = True
    return dit, None, list(dit.parameters())


@pytest.mark.parametrize("method", ["lora", "full"])
def test_the_second_pass_reads_the_perturbed_words_not_a_stale_copy(method, deterministic):
    from lcv_hip import ops, optim
    from tta import inner_loop as L
    i = M._inputs()
    rho = 2.0 if method == "lora" else 20.0
    make = _lora_model if method == "lora" else _full_model

    def loss_fn(dit):
        return L._fm_loss(dit, L._OneVideo(i["cond"], i["train"], i["embeds"], i["mask"], None), DEV, BF16)

    def replayed(fn, state, grad):
        L._rng_replay(state)
        if grad:
            return fn(0)
        with torch.no_grad():
            return fn(0)
    dit, _, params = make()
    dit.train()
    opt = ops.FusedSGDClip(params, lr=1e-3) if method == "full" else ops.FusedAdamWClip(params, lr=1e-3)
    opt.enable_sam(rho)
    at = loss_fn(dit)
    torch.manual_seed(77)
    state = L._rng_capture(torch.device(DEV))
    warm = replayed(at, state, False)                                     # fills whatever copies of the weights the forward caches
    first = replayed(at, state, True)
    first.backward()
    live = [p for p in params if p.grad is not None and p.numel()]
    ref = [{"h": M._h_of(p), "low": None, "g": M._h_of(p.grad if p.grad.is_contiguous() else p.grad.contiguous())} for p in live]
    want = S.perturb(ref, rho)
    optim.sam_perturb([opt])
    opt.zero_grad()
    second = replayed(at, state, True).detach().clone()
    second_ng = replayed(at, state, False).detach().clone()
    for p, hp in zip(live, want["words"]):
        _report(f"{method} perturbed words", -1, M._h_of(p), hp)
    optim.sam_restore([opt])
    for p, t in zip(live, ref):
        _report(f"{method} restored words", -1, M._h_of(p), t["h"])
    again = replayed(at, state, False)
    # a fresh model with the restated perturbed words written the ordinary way
    fresh, _, fparams = make()
    fresh.train()
    assert len(fparams) == len(params)
    index = {id(p): k for k, p in enumerate(params)}
    with torch.no_grad():
        for p, hp in zip(live, want["words"]):
            fparams[index[id(p)]].copy_(M._bf16_dev(hp).view(p.shape))
    fat = loss_fn(fresh)
    want_loss = replayed(fat, state, True).detach()
    want_ng = replayed(fat, state, False).detach()
    torch.cuda.synchronize()
    moved = sum(int(np.count_nonzero(hp != t["h"])) for hp, t in zip(want["words"], ref))
    print(f"{method}: first {float(first.detach())!r} second {float(second)!r} fresh {float(want_loss)!r}; {moved} words moved, realized "
          f"{float(want['realized'][1])!r} of rho {rho}")
    assert moved > 0
    assert M._bits_of(second.float())[0] == M._bits_of(want_loss.float())[0]
    assert M._bits_of(second_ng.float())[0] == M._bits_of(want_ng.float())[0]
    assert M._bits_of(second.float())[0] != M._bits_of(first.detach().float())[0]
    assert M._bits_of(again.float())[0] == M._bits_of(warm.float())[0]    # and after the restore the first point again


# ---------------------------------------------------------------------------------------------------------- 6. rho = 0 is neutral
STEPS = 3


def _rng_states():
    return torch.get_rng_state().clone(), torch.cuda.default_generators[torch.cuda.current_device()].get_state().clone()


def _run_loop(method, **flag):
    """A few steps of one loop from one seed on a fresh model; returns (loss bits, parameter bits, state bits, rng, result)."""
    from tta import delta as D
    from tta.full_tta import finetune_full_on_conditioning
    from tta.inner_loop import finetune_lora_on_conditioning
    i = M._inputs()
    args = (i["cond"], i["train"], i["embeds"], i["mask"])
    state = []
    if method == "lora":
        dit, mods, params = _lora_model()
        torch.manual_seed(1234)
        res = finetune_lora_on_conditioning(dit, mods, *args, num_steps=STEPS, lr=2e-3, warmup_steps=1, device=DEV, dtype=BF16, **flag)
    elif method == "full":
        dit, _, params = _full_model()
        torch.manual_seed(1234)
        res = finetune_full_on_conditioning(dit, *args, num_steps=STEPS, lr=1e-3, warmup_steps=1, device=DEV, dtype=BF16,
                                            optimizer_type="sgd", **flag)
    elif method == "delta_a":
        w = D.DeltaAWrapper(M._dit(), adaln_tembed_dim=64).to(DEV)
        params = [w.delta]
        torch.manual_seed(1234)
        res = D.optimize_delta_a(w, *args, num_steps=STEPS, lr=1e-2, device=DEV, dtype=BF16, **flag)
    else:
        w = D.NormTuneForward(M._dit(), "all_norm", also_tune_delta=True).to(DEV)
        params = list(w.tuned_params)
        torch.manual_seed(1234)
        res = D.optimize_norm_params(w, w.tuned_params, *args, num_steps=STEPS, lr=1e-2, device=DEV, dtype=BF16, **flag)
    torch.cuda.synchronize()
    rng = _rng_states()
    bits = [M._bits_of(p) if p.dtype == torch.float32 else M._h_of(p) for p in params]
    return [float(v).hex() for v in res["losses"]], bits, rng, res


@pytest.fixture
def made_optimizers(monkeypatch):
    """Every optimizer the loops make, to compare their state."""
    from lcv_hip import ops
    from tta import delta, full_tta, inner_loop
    seen = []

    def recording(cls):
        class Recording(cls):
            def __init__(self, *a, **k):
                super().__init__(*a, **k)
                seen.append(self)
        return Recording
    adamw, sgd = recording(ops.FusedAdamWClip), recording(ops.FusedSGDClip)
    for mod in (inner_loop, full_tta, delta):
        monkeypatch.setattr(mod, "FusedAdamWClip", adamw)
    monkeypatch.setattr(full_tta, "FusedSGDClip", sgd)
    return seen


def _state_bits(opts):
    out = []
    for o in opts:
        if isinstance(o.exp_avg, list) and o.exp_avg is not o.params:
            out += [t.detach().contiguous().view(torch.uint8).cpu().numpy() for ts in (o.exp_avg, o.exp_avg_sq) for t in ts]
        out += [t.cpu().numpy() for t in o.low_words]
        out.append(np.array([o.step_count]))
    return out


@pytest.mark.parametrize("method", ["lora", "delta_a", "norm", "full"])
def test_rho_zero_changes_no_bit_of_the_run(method, deterministic, made_optimizers):
    extra = {"lora": [{}, {"master_weights": True}], "full": [{}], "delta_a": [{}], "norm": [{}]}[method]
    for kw in extra:
        del made_optimizers[:]
        l0, p0, rng0, r0 = _run_loop(method, **kw)
        s0 = _state_bits(made_optimizers)
        assert "sam" not in r0 and len(l0) == STEPS and not any(o.sam_rho is not None for o in made_optimizers)
        del made_optimizers[:]
        l1, p1, rng1, r1 = _run_loop(method, sam_rho=0.0, **kw)
        s1 = _state_bits(made_optimizers)
        assert l1 == l0, (method, kw)
        assert len(p0) == len(p1) and all(np.array_equal(a, b) for a, b in zip(p0, p1)), (method, kw)
        assert len(s0) == len(s1) and all(np.array_equal(a, b) for a, b in zip(s0, s1)), (method, kw)
        assert torch.equal(rng0[0], rng1[0]) and torch.equal(rng0[1], rng1[1]), (method, kw)
        sam = r1["sam"]
        assert set(sam) == {"rho", "adaptive", "eta", "steps", "grad_norm_trace", "realized_norm_trace", "perturbed_loss_trace"}
        assert sam["rho"] == 0.0 and sam["steps"] == STEPS and sam["realized_norm_trace"] == [0.0] * STEPS
        assert [float(v).hex() for v in sam["perturbed_loss_trace"]] == l0          # the second pass saw the first's draws
        assert all(math.isfinite(v) and v > 0 for v in sam["grad_norm_trace"])


# ---------------------------------------------------------------------------------------------------------- 7. the runners
LORA_RUN = "lora_experiment/scripts/run_lora_tta.py"
FULL_RUN = "lora_experiment/scripts/run_full_tta.py"
KEYS = {"rho", "adaptive", "eta", "steps", "grad_norm_trace", "realized_norm_trace", "perturbed_loss_trace"}


def _rows(tmp_path, rel, argv, flags):
    out = {}
    for name, extra in (("on", flags), ("off", [])):
        M._main(rel, M.COMMON + argv + extra + ["--output-dir", str(tmp_path / name), "--skip-generation"])
        summary = json.loads((tmp_path / name / "summary.json").read_text())
        cfg = tmp_path / name / "config.json"
        out[name] = (summary, json.loads(cfg.read_text()) if cfg.exists() else None)
        assert summary["results"][0]["success"]
    return out


def _check_sam_row(row, rho, adaptive, steps):
    sam = row["sam"]
    assert set(sam) == KEYS and sam["rho"] == rho and sam["adaptive"] is adaptive and sam["eta"] == 0.01
    assert sam["steps"] in steps
    for key in ("grad_norm_trace", "realized_norm_trace", "perturbed_loss_trace"):
        assert len(sam[key]) == sam["steps"] and all(math.isfinite(v) for v in sam[key]), key
    assert all(v > 0 for v in sam["grad_norm_trace"])
    return sam


def test_lora_runner_with_the_early_stopper_records_sam(tmp_path):
    argv = ["--num-steps", "4", "--lora-rank", "4", "--lora-alpha", "8", "--es-check-every", "2", "--es-patience", "1"]
    got = _rows(tmp_path, LORA_RUN, argv, ["--sam-rho", "0.05"])
    (s_on, c_on), (s_off, c_off) = got["on"], got["off"]
    r_on, r_off = s_on["results"][0], s_off["results"][0]
    assert set(r_on) - set(r_off) == {"sam"} and set(c_on["training"]) - set(c_off["training"]) == {"sam_rho", "sam_adaptive", "sam_eta"}
    assert c_on["training"]["sam_rho"] == 0.05 and c_on["training"]["sam_adaptive"] is False and c_on["training"]["sam_eta"] == 0.01
    assert '"sam' not in json.dumps(c_off) and '"sam' not in json.dumps(s_off)
    _check_sam_row(r_on, 0.05, False, (2, 4))
    assert r_on["early_stopping_info"]["total_checks"] >= 1


def test_delta_a_runner_adaptive_keeps_rho_in_fp32(tmp_path):
    argv = ["--delta-steps", "4", "--delta-lr", "1e-2", "--es-disable"]
    for adaptive in (False, True):
        got = _rows(tmp_path / str(adaptive), M.DELTA_A, argv, ["--sam-rho", "0.05"] + (["--sam-adaptive"] if adaptive else []))
        (s_on, _), (s_off, _) = got["on"], got["off"]
        assert set(s_on) - set(s_off) == {"sam_rho", "sam_adaptive", "sam_eta"} and s_on["sam_adaptive"] is adaptive
        assert set(s_on["results"][0]) - set(s_off["results"][0]) == {"sam"} and '"sam' not in json.dumps(s_off)
        sam = _check_sam_row(s_on["results"][0], 0.05, adaptive, (4,))
        if not adaptive:
            # fp32 parameters: realized <= rho (1 + the reduction bound) + 2^-24 |theta'|; |theta'| <= |delta| + rho, and the
            # vector is far below 1 in norm after four steps at lr 1e-2 (512 elements: at most 4 * 1e-2 * sqrt(512) < 1)
            rho_f, eps, slack = float(F(0.05)), S.eps_realized([512]), T.U * (1.0 + 0.05)
            print(f"delta-A realized {sam['realized_norm_trace']} within rho (1 +- {eps!r}) +- {slack!r}")
            assert all(v <= rho_f * (1.0 + eps) + slack for v in sam["realized_norm_trace"])
            assert all(v >= rho_f * (1.0 - eps) - slack for v in sam["realized_norm_trace"])      # and not below it either


def test_full_model_sgd_runner_records_sam(tmp_path):
    got = _rows(tmp_path, FULL_RUN, ["--num-steps", "3", "--learning-rate", "1e-3", "--es-disable"], ["--sam-rho", "0.05"])
    (s_on, c_on), (s_off, c_off) = got["on"], got["off"]
    assert set(s_on["results"][0]) - set(s_off["results"][0]) == {"sam"}
    assert set(c_on["training"]) - set(c_off["training"]) == {"sam_rho", "sam_adaptive", "sam_eta"}
    sam = _check_sam_row(s_on["results"][0], 0.05, False, (3,))
    # bf16 words: what the forward saw is what survived the rounding, and the trace says so
    print(f"full model: realized {sam['realized_norm_trace']} of rho 0.05, gradient norms {sam['grad_norm_trace']}")
    assert all(v >= 0 for v in sam["realized_norm_trace"])

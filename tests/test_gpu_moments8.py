"""GPU: 8-bit block-scaled AdamW moments for master weights (include/lcv_hip_moments8.h, `moments_8bit=True` / `--adam-8bit`).

1. lcv_moments8_encode / lcv_moments8_decode against the numpy restatement (tests/moments8_ref.py), bit for bit, at every size
   around a packet, a block and a chunk, through the packet path and (one-element offset views) the scalar path, on log-uniform
   data, an all-zero block, a block with one element 2^40 times the rest (clamp and flush) and an all-negative block.
2. lcv_master_adamw8_step through the optimizer: bf16 words, low words, both code tensors and both scale rows after each of four
   steps, over a table with a sub-packet tensor, an exact block, one element past a block, one past a chunk (as offset views:
   the scalar path) and a tail past two chunks, plus a parameter without a gradient.
3. The links to the fp32-moment step on the device: (a) from zeroed state the first step gives its (h, l) bits; (b) from any
   state one step gives the (h, l) bits of that step fed the decoded moments.
4. Refused arguments, state_bytes(), moment_tensors(), accumulation of updates below half a bf16 ulp.
5. The loops and the runners.
"""
import json

import numpy as np
import pytest
import torch

import master_weights_ref as W
import moments8_ref as R
from test_gpu_master_weights import (_bf16_dev, _bits_of, _call, _dit, _eighth_ulp_case, _f32_dev, _h_of, _i16_dev, _inputs, _main,
                                     _offset_view)

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
DEV = "cuda"
SIZES = (1, 7, 8, 511, 512, 513, 2047, 2048, 2049, 2048 + 512 + 3)
CASES = ("log_uniform", "zero_block", "spike", "negative")
SENTINEL = 0xA5


# ---------------------------------------------------------------------------------------------------------- helpers
def _u8_dev(c):
    return torch.from_numpy(np.ascontiguousarray(c, dtype=np.uint8).copy()).to(DEV)


def _guarded(n, dtype, offset):
    """n elements inside a larger sentinel-filled buffer, starting at element 0 (aligned) or 1; returns (view, check) where
    check() says that nothing outside the view was written."""
    pad = 16
    base = torch.empty(n + pad + 1, dtype=dtype, device=DEV)
    base.view(torch.uint8).fill_(SENTINEL)
    lo = 1 if offset else 0
    view = base[lo:lo + n]
    assert view.is_contiguous() and view.data_ptr() % 16 == lo * base.element_size()

    def untouched():
        raw = base.view(torch.uint8)
        es = base.element_size()
        return bool((raw[:lo * es] == SENTINEL).all()) and bool((raw[(lo + n) * es:] == SENTINEL).all())
    return view, untouched


_DATA = {}


def _case(case, n):
    """Host-made fp32 (m, v) of one tensor and what the restatement makes of them, computed once per (case, n)."""
    key = (case, n)
    if key not in _DATA:
        rng = np.random.default_rng(1000 + 17 * CASES.index(case) + n)
        if case == "spike":
            m, v = R.moments(rng, n, -4.0, 0.0)
            i = min(n - 1, 5)
            m[i], v[i] = -(2.0 ** 40), 2.0 ** 80                  # 2^40 times the rest: they flush (m) and clamp up (r)
        else:
            m, v = R.moments(rng, n)
        if case == "zero_block":
            m[:R.BLOCK] = 0.0
            v[:R.BLOCK] = 0.0
        if case == "negative":
            m = -np.abs(m)
        cm, cr, s = R.encode(m, v)
        _DATA[key] = dict(m=m, v=v, cm=cm, cr=cr, s=s, dec=R.decode(cm, cr, s))
    return _DATA[key]


def _first_bad(what, n, got, want):
    bad = np.flatnonzero(np.asarray(got).ravel() != np.asarray(want).ravel())
    assert bad.size == 0, f"{what} n={n}: {bad.size} mismatches, first at {int(bad[0])}: got {np.asarray(got).ravel()[bad[0]]!r} " \
                          f"want {np.asarray(want).ravel()[bad[0]]!r}"


# ---------------------------------------------------------------------------------------------------------- 1. encode / decode
@pytest.mark.parametrize("offset", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_encode_bits(case, offset):
    flushed = clamped = 0
    for n in SIZES:
        d = _case(case, n)
        m, ok_m = _guarded(n, torch.float32, offset)
        v, ok_v = _guarded(n, torch.float32, offset)
        m.copy_(torch.from_numpy(d["m"]))
        v.copy_(torch.from_numpy(d["v"]))
        cm, ok_cm = _guarded(n, torch.uint8, offset)
        cr, ok_cr = _guarded(n, torch.uint8, offset)
        s, ok_s = _guarded(2 * R.nblocks(n), torch.float32, False)
        _call("lcv_moments8_encode", m.data_ptr(), v.data_ptr(), cm.data_ptr(), cr.data_ptr(), s.data_ptr(), n)
        torch.cuda.synchronize()
        _first_bad(f"{case} sm/sr", n, _bits_of(s), W.bits(d["s"]).ravel())
        _first_bad(f"{case} cm", n, cm.cpu().numpy(), d["cm"])
        _first_bad(f"{case} cr", n, cr.cpu().numpy(), d["cr"])
        assert ok_m() and ok_v() and ok_cm() and ok_cr() and ok_s(), f"{case} n={n}: a write outside the tensor"
        flushed += int(((d["cm"] == 0) & (d["m"] != 0)).sum())
        clamped += int(((d["cr"] == 1) & (np.sqrt(d["v"]) < R.R_FLOOR * np.repeat(d["s"][1], R.BLOCK)[:n])).sum())
    if case == "spike":
        assert flushed > 1000 and clamped > 1000               # the case does what it is there for
    if case == "negative":
        assert all((_case(case, n)["cm"] >= 128).all() for n in SIZES)
    if case == "zero_block":
        assert all(not _case(case, n)["s"][:, 0].any() for n in SIZES)


@pytest.mark.parametrize("offset", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_decode_bits(case, offset):
    for n in SIZES:
        d = _case(case, n)
        cm, _ = _guarded(n, torch.uint8, offset)
        cr, _ = _guarded(n, torch.uint8, offset)
        cm.copy_(_u8_dev(d["cm"]))
        cr.copy_(_u8_dev(d["cr"]))
        s = _f32_dev(W.bits(d["s"]).ravel())
        m, ok_m = _guarded(n, torch.float32, offset)
        v, ok_v = _guarded(n, torch.float32, offset)
        _call("lcv_moments8_decode", cm.data_ptr(), cr.data_ptr(), s.data_ptr(), m.data_ptr(), v.data_ptr(), n)
        torch.cuda.synchronize()
        _first_bad(f"{case} m", n, _bits_of(m), W.bits(d["dec"][0]))
        _first_bad(f"{case} v", n, _bits_of(v), W.bits(d["dec"][1]))
        assert ok_m() and ok_v(), f"{case} n={n}: a write outside the tensor"


def test_every_code_decodes_as_restated_and_encodes_back():
    cm = np.tile(np.array([c for c in range(256) if c != 128] + [127], dtype=np.uint8), 3)       # 768 codes: two blocks
    cr = np.tile(np.arange(256, dtype=np.uint8), 3)
    s = np.array([[3.0, 2.0 ** -20], [1.7e5, 0.3]], dtype=np.float32)
    n = cm.size
    m = torch.zeros(n, dtype=torch.float32, device=DEV)
    v = torch.zeros(n, dtype=torch.float32, device=DEV)
    dcm, dcr, ds = _u8_dev(cm), _u8_dev(cr), _f32_dev(W.bits(s).ravel())
    _call("lcv_moments8_decode", dcm.data_ptr(), dcr.data_ptr(), ds.data_ptr(), m.data_ptr(), v.data_ptr(), n)
    want = R.decode(cm, cr, s)
    assert np.array_equal(_bits_of(m), W.bits(want[0])) and np.array_equal(_bits_of(v), W.bits(want[1]))
    cm2, cr2, s2 = torch.zeros_like(dcm), torch.zeros_like(dcr), torch.zeros_like(ds)
    _call("lcv_moments8_encode", m.data_ptr(), v.data_ptr(), cm2.data_ptr(), cr2.data_ptr(), s2.data_ptr(), n)
    torch.cuda.synchronize()
    assert np.array_equal(cm2.cpu().numpy(), cm) and np.array_equal(cr2.cpu().numpy(), cr)
    assert np.array_equal(_bits_of(s2), W.bits(s).ravel())


# ---------------------------------------------------------------------------------------------------------- 2. the step
NUMELS = (3, 512, 513, 2049, 4096 + 17)
VIEW = 3                      # the 2049-element tensor: parameter, gradient and codes are [1:] views (the scalar path)
IDLE = 300                    # a sixth parameter that never gets a gradient
STEPS = 4
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
_TABLE = {}


def _table():
    """Host-generated inputs, made once: |w| in [2^-10, 2], |g| in [2^-20, 8], both signs.  Inside a block the gradients span
    23 binades, so small first moments flush."""
    if not _TABLE:
        rng = np.random.default_rng(41)
        _TABLE["w"] = [W.weights(rng, n) for n in NUMELS + (IDLE,)]
        _TABLE["g"] = [[W.grads(rng, n) for n in NUMELS] for _ in range(STEPS)]
    return _TABLE


def _make(wd, moments_8bit=True):
    from lcv_hip import ops
    t = _table()
    params = []
    for k, (h, _) in enumerate(t["w"]):
        p = _bf16_dev(h)
        params.append(_offset_view(p) if k == VIEW else p)
    opt = ops.FusedAdamWClip(params, lr=LR, betas=(B1, B2), weight_decay=wd, eps=EPS, master_weights=True, moments_8bit=moments_8bit)
    for lw, (_, low) in zip(opt.low_words, t["w"]):
        lw.copy_(_i16_dev(low))
    if moments_8bit:
        for c in opt.exp_avg + opt.exp_avg_sq:
            assert c.dtype == torch.uint8 and not c.any()
        for s, p in zip(opt._scales, params):
            assert s.dtype == torch.float32 and tuple(s.shape) == (2, R.nblocks(p.numel())) and not s.any()
        opt.exp_avg[VIEW] = _offset_view(opt.exp_avg[VIEW])           # before the first step builds the table
        opt.exp_avg_sq[VIEW] = _offset_view(opt.exp_avg_sq[VIEW])
    return opt, params


def _set_grads(params, step):
    t = _table()
    for k in range(len(NUMELS)):
        g = _bf16_dev(t["g"][step][k])
        params[k].grad = _offset_view(g) if k == VIEW else g


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("clip", [False, True])
def test_adamw8_step_bits(clip, wd):
    opt, params = _make(wd)
    t = _table()
    # the idle parameter's state is marked, to see that nobody touches it
    opt.exp_avg[-1].fill_(37); opt.exp_avg_sq[-1].fill_(201); opt._scales[-1].fill_(0.5)
    ref = [dict(h=h.copy(), l=low.copy(), st=R.zero_state(h.size)) for h, low in t["w"][:len(NUMELS)]]
    flushed = 0
    for step in range(STEPS):
        _set_grads(params, step)
        coef = 1.0
        if clip:
            opt.clip_grad_norm_(1.0)
            norm, coef = (float(x) for x in opt._norm_coef.tolist())
            assert 0.0 < coef < 1.0 and norm > 1.0
        opt.step()
        torch.cuda.synchronize()
        for k, r in enumerate(ref):
            r["h"], r["l"], *st = R.adamw8_step(r["h"], r["l"], *r["st"], t["g"][step][k], coef, LR, B1, B2, EPS, wd, step + 1)
            r["st"] = tuple(st)
            what = f"step {step + 1} tensor {k}"
            _first_bad(what + " h", NUMELS[k], _h_of(params[k]), r["h"])
            _first_bad(what + " l", NUMELS[k], opt.low_words[k].cpu().numpy(), r["l"])
            _first_bad(what + " sm/sr", NUMELS[k], _bits_of(opt._scales[k]), W.bits(st[2]))
            _first_bad(what + " cm", NUMELS[k], opt.exp_avg[k].cpu().numpy(), st[0])
            _first_bad(what + " cr", NUMELS[k], opt.exp_avg_sq[k].cpu().numpy(), st[1])
            flushed += int((st[0] == 0).sum())
    assert flushed > 0                                              # the flush path ran
    # the parameter without a gradient: words and state are what they were
    h, low = t["w"][-1]
    assert np.array_equal(_h_of(params[-1]), h) and np.array_equal(opt.low_words[-1].cpu().numpy(), low)
    assert bool((opt.exp_avg[-1] == 37).all()) and bool((opt.exp_avg_sq[-1] == 201).all()) and bool((opt._scales[-1] == 0.5).all())
    assert sum(int((r["h"] != w[0]).sum()) for r, w in zip(ref, t["w"])) > 0


# ---------------------------------------------------------------------------------------------------------- 3. the links
def _words(opt, params):
    return [(_h_of(p).copy(), lw.cpu().numpy().copy()) for p, lw in zip(params, opt.low_words)]


@pytest.mark.parametrize("clip", [False, True])
def test_property_a_first_step_from_zero_state_matches_the_fp32_moment_step(clip):
    got = []
    for m8 in (False, True):
        opt, params = _make(0.01, moments_8bit=m8)
        _set_grads(params, 0)
        if clip:
            opt.clip_grad_norm_(1.0)
        opt.step()
        torch.cuda.synchronize()
        got.append(_words(opt, params))
    for k, ((h32, l32), (h8, l8)) in enumerate(zip(*got)):
        _first_bad("h", k, h8, h32)
        _first_bad("l", k, l8, l32)
    assert any((h != w[0]).any() for (h, _), w in zip(got[0], _table()["w"]))


def test_property_b_one_step_from_any_state_matches_the_fp32_moment_step_fed_the_decoded_moments():
    o8, p8 = _make(0.01)
    for step in range(2):
        _set_grads(p8, step)
        o8.clip_grad_norm_(1.0)
        o8.step()
    # an fp32-moment optimizer on copies of the words, fed the decoded state
    o32, p32 = _make(0.01, moments_8bit=False)
    dec = o8.moment_tensors()
    for k in range(len(NUMELS)):
        p32[k].copy_(p8[k])
        o32.low_words[k].copy_(o8.low_words[k])
        o32.exp_avg[k].copy_(dec[k][0])
        o32.exp_avg_sq[k].copy_(dec[k][1])
    o32.step_count = o8.step_count
    assert any(bool(c.any()) for c in o8.exp_avg) and o32.exp_avg[0].dtype == torch.float32
    for o, p in ((o8, p8), (o32, p32)):
        _set_grads(p, 2)
        o.clip_grad_norm_(1.0)
        o.step()
    torch.cuda.synchronize()
    for k, ((h32, l32), (h8, l8)) in enumerate(zip(_words(o32, p32), _words(o8, p8))):
        _first_bad("h", k, h8, h32)
        _first_bad("l", k, l8, l32)


# ---------------------------------------------------------------------------------------------------------- 4. other checks
def test_bad_arguments_are_refused():
    from lcv_hip.lib import LcvError
    f = torch.zeros(8, dtype=torch.float32, device=DEV)
    c = torch.zeros(8, dtype=torch.uint8, device=DEV)
    step = (1, 1, None, 1e-3, 0.9, 0.999, 1e-8, 0.0)
    for name, args in (("lcv_moments8_encode", (f.data_ptr(), f.data_ptr(), c.data_ptr(), c.data_ptr(), f.data_ptr(), 0)),
                       ("lcv_moments8_encode", (f.data_ptr(), f.data_ptr(), c.data_ptr(), None, f.data_ptr(), 8)),
                       ("lcv_moments8_encode", (f.data_ptr(), f.data_ptr(), c.data_ptr(), c.data_ptr(), None, 8)),
                       ("lcv_moments8_decode", (c.data_ptr(), c.data_ptr(), f.data_ptr(), f.data_ptr(), f.data_ptr(), -1)),
                       ("lcv_moments8_decode", (c.data_ptr(), c.data_ptr(), None, f.data_ptr(), f.data_ptr(), 8)),
                       ("lcv_master_adamw8_step", (f.data_ptr(), f.data_ptr(), None) + step + (1,)),
                       ("lcv_master_adamw8_step", (f.data_ptr(), None, f.data_ptr()) + step + (1,)),
                       ("lcv_master_adamw8_step", (f.data_ptr(), f.data_ptr(), f.data_ptr()) + step + (0,)),
                       ("lcv_master_adamw8_step", (f.data_ptr(), f.data_ptr(), f.data_ptr(), 1, 0) + step[2:] + (1,))):
        with pytest.raises(LcvError) as e:
            _call(name, *args)
        assert e.value.code == -1 and not e.value.fatal
    torch.cuda.synchronize()
    assert not f.any() and not c.any()                              # nothing was launched


def test_state_bytes_and_moment_tensors():
    from lcv_hip import ops
    opt, params = _make(0.0)
    assert opt.state_bytes() == sum(2 * p.numel() + 8 * ((p.numel() + 511) // 512) for p in params)
    o32, _ = _make(0.0, moments_8bit=False)
    assert o32.state_bytes() == sum(8 * p.numel() for p in params)
    assert ops.FusedSGDClip(params, master_weights=True).state_bytes() == 0
    t = _table()
    ref = [dict(h=h.copy(), l=low.copy(), st=R.zero_state(h.size)) for h, low in t["w"][:len(NUMELS)]]
    for m, v in opt.moment_tensors():
        assert m.dtype == v.dtype == torch.float32 and not m.any() and not v.any()
    for step in range(2):
        _set_grads(params, step)
        opt.step()
        for k, r in enumerate(ref):
            r["h"], r["l"], *st = R.adamw8_step(r["h"], r["l"], *r["st"], t["g"][step][k], 1.0, LR, B1, B2, EPS, 0.0, step + 1)
            r["st"] = tuple(st)
    got = opt.moment_tensors()
    torch.cuda.synchronize()
    assert len(got) == len(params)
    for k, r in enumerate(ref):
        m, v = R.decode(*r["st"])
        assert got[k][0].shape == params[k].shape
        _first_bad("moment_tensors m", k, _bits_of(got[k][0]), W.bits(m))
        _first_bad("moment_tensors v", k, _bits_of(got[k][1]), W.bits(v))
        assert np.abs(m).max() > 0 and v.max() > 0
    assert not got[-1][0].any() and not got[-1][1].any()            # the idle parameter: zeroed state decodes to zeros
    # the fp32-moment form returns copies of what it holds
    m32 = o32.moment_tensors()
    assert m32[0][0].dtype == torch.float32 and m32[0][0].data_ptr() != o32.exp_avg[0].data_ptr()


def test_updates_below_half_a_bf16_ulp_accumulate_with_8bit_moments_as_well():
    """The weights and +-2^e gradients of the eighth-of-an-ulp case (|w| in [2^-6, 2]) under AdamW, whose step is about lr
    whatever the gradient: lr = 2^-17 is 1/16 ulp of the smallest weight and less of every other.  Without master weights every
    update is discarded.  With them and 8-bit moments the masters are the restatement's, bit for bit, and every one has moved
    against its gradient by more than 1.5 lr after 16 steps: the first step moves lr * |g| / (|g| + eps) as the fp32-moment
    step does, and at the second step m >= (0.9 * (1 - 2^-4) * 0.1 + 0.1) |g| = 0.184 |g| against bc1 = 0.19 and
    v <= (0.999 * (1 + 2^-4)^2 + 1) * 0.001 g^2 against bc2 = 0.001999, so it moves at least 0.94 lr; every later step moves
    the same way, since m keeps the sign of the constant gradient."""
    from lcv_hip import ops
    h0, gb, _ = _eighth_ulp_case()
    lr, steps = 2.0 ** -17, 16
    g = _bf16_dev(gb)
    p = _bf16_dev(h0)
    opt = ops.FusedAdamWClip([p], lr=lr, betas=(B1, B2), weight_decay=0.0, eps=EPS)
    for _ in range(steps):
        p.grad = g
        opt.step()
    torch.cuda.synchronize()
    assert np.array_equal(_h_of(p), h0)                             # today's behaviour: nothing moved
    p = _bf16_dev(h0)
    opt = ops.FusedAdamWClip([p], lr=lr, betas=(B1, B2), weight_decay=0.0, eps=EPS, master_weights=True, moments_8bit=True)
    h, low, st = h0.copy(), np.zeros(h0.size, np.int16), R.zero_state(h0.size)
    for k in range(steps):
        p.grad = g
        opt.step()
        h, low, *st = R.adamw8_step(h, low, *st, gb, 1.0, lr, B1, B2, EPS, 0.0, k + 1)
    torch.cuda.synchronize()
    _first_bad("h", h0.size, _h_of(p), h)
    _first_bad("l", h0.size, opt.low_words[0].cpu().numpy(), low)
    moved = W.master(h, low).astype(np.float64) - W.bf16_to_f32(h0).astype(np.float64)
    against = -np.sign(W.bf16_to_f32(gb).astype(np.float64)) * moved
    print(f"moved against the gradient by {against.min() / lr:.3f} .. {against.max() / lr:.3f} lr in {steps} steps")
    assert against.min() > 1.5 * lr


# ---------------------------------------------------------------------------------------------------------- 5. the loops
@pytest.fixture
def deterministic():
    from lcv_hip import ops
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    yield ops
    ops.set_deterministic(was)


@pytest.fixture
def made(monkeypatch):
    """The AdamW optimizers the loops build, with the bf16 and low words after each of their steps."""
    from lcv_hip import ops
    from tta import full_tta, inner_loop
    seen = []

    class Recording(ops.FusedAdamWClip):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            self.after = []
            seen.append(self)

        def step(self):
            super().step()
            self.after.append([p.detach().clone() for p in self.params] + [lw.clone() for lw in self.low_words])
    monkeypatch.setattr(inner_loop, "FusedAdamWClip", Recording)
    monkeypatch.setattr(full_tta, "FusedAdamWClip", Recording)
    return seen


def _adapt(method, **flag):
    """Three AdamW steps from one seed on a fresh small DiT, no early stopper."""
    from tta.full_tta import finetune_full_on_conditioning
    from tta.inner_loop import finetune_lora_on_conditioning
    from tta.lora import get_lora_parameters, inject_lora_into_dit
    i = _inputs()
    dit = _dit()
    if method == "lora":
        for p in dit.parameters():
            p.requires_grad = False
        torch.manual_seed(3)
        mods = inject_lora_into_dit(dit, rank=8, alpha=16.0, target_modules=["qkv", "proj"], target_ffn=False, target_blocks="all")
        params = get_lora_parameters(mods)
        torch.manual_seed(1234)
        res = finetune_lora_on_conditioning(dit, mods, i["cond"], i["train"], i["embeds"], i["mask"], num_steps=3, lr=2e-3,
                                            warmup_steps=1, weight_decay=0.01, max_grad_norm=1.0, device=DEV, dtype=BF16, **flag)
    else:
        for p in dit.parameters():
            p.requires_grad = True
        params = list(dit.parameters())
        torch.manual_seed(1234)
        res = finetune_full_on_conditioning(dit, i["cond"], i["train"], i["embeds"], i["mask"], num_steps=3, lr=1e-3,
                                            warmup_steps=1, weight_decay=0.01, max_grad_norm=1.0, device=DEV, dtype=BF16,
                                            optimizer_type="adamw", **flag)
    torch.cuda.synchronize()
    return [float(v).hex() for v in res["losses"]], [p.detach().clone() for p in params]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("method", ["lora", "full"])
def test_loops_flag_off_is_todays_run_flag_on_is_reproducible_and_parts_from_fp32_moments_at_step_two(method, deterministic, made):
    l0, w0 = _adapt(method)                                               # both keywords omitted
    l1, w1 = _adapt(method, moments_8bit=False)
    assert len(l0) == 3 and l0 == l1 and _same(w0, w1)
    l32, w32 = _adapt(method, master_weights=True)                        # fp32 moments
    l32b, w32b = _adapt(method, master_weights=True, moments_8bit=False)
    assert l32 == l32b and _same(w32, w32b)
    assert [(o.master_weights, o.moments_8bit) for o in made] == [(False, False)] * 2 + [(True, False)] * 2
    assert all(o.exp_avg[0].dtype == (torch.float32 if o.master_weights else BF16) for o in made)
    o32 = made[2]
    del made[:]
    la, wa = _adapt(method, master_weights=True, moments_8bit=True)
    lb, wb = _adapt(method, master_weights=True, moments_8bit=True)
    assert len(la) == 3 and all(np.isfinite(float.fromhex(v)) for v in la)
    assert la == lb and _same(wa, wb)
    assert [(o.master_weights, o.moments_8bit) for o in made] == [(True, True)] * 2
    o8 = made[0]
    assert o8.exp_avg[0].dtype == torch.uint8
    assert o32.state_bytes() == sum(8 * p.numel() for p in o32.params)
    assert o8.state_bytes() == sum(2 * p.numel() + 8 * ((p.numel() + 511) // 512) for p in o8.params) < o32.state_bytes() / 3
    assert len(o8.after) == len(o32.after) == 3
    assert _same(o8.after[0], o32.after[0])                               # property (a): step 1 is the fp32-moment step
    assert not _same(o8.after[1], o32.after[1])                           # from step 2 the quantised state shows
    assert la[:2] == l32[:2]


# ---------------------------------------------------------------------------------------------------------- 6. the runners
RUN = ["--checkpoint-dir", "synthetic:2:256:64", "--data-dir", "synthetic:1", "--num-cond-frames", "5", "--num-frames", "13",
       "--gen-start-frame", "40", "--tta-total-frames", "33", "--tta-context-frames", "9", "--num-steps", "4",
       "--num-inference-steps", "2", "--no-save-videos"]


@pytest.mark.parametrize("script, extra", [
    ("run_lora_tta.py", ["--es-disable", "--lora-rank", "4", "--lora-alpha", "8"]),
    ("run_full_tta.py", ["--es-check-every", "2", "--es-patience", "1", "--learning-rate", "1e-4", "--optimizer", "adamw"]),
])
def test_runners_accept_adam_8bit(tmp_path, script, extra):
    out = tmp_path / "run"
    _main(script, RUN + ["--output-dir", str(out), "--master-weights", "--adam-8bit"] + extra)
    cfg = json.loads((out / "config.json").read_text())
    assert cfg["training"]["master_weights"] is True and cfg["training"]["adam_8bit"] is True
    s = json.loads((out / "summary.json").read_text())
    r = s["results"][0]
    assert s["num_videos"] == 1 and s["num_successful"] == 1 and r["success"] and r["final_loss"] == r["final_loss"]
    assert 1 <= r["num_train_steps"] <= 4


def test_full_runner_refuses_adam_8bit_under_sgd_at_parse_time(tmp_path, capsys):
    out = tmp_path / "run"
    with pytest.raises(SystemExit) as e:
        _main("run_full_tta.py", RUN + ["--output-dir", str(out), "--optimizer", "sgd", "--master-weights", "--adam-8bit"])
    assert e.value.code == 2 and "--adam-8bit needs --optimizer adamw" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        _main("run_full_tta.py", RUN + ["--output-dir", str(out), "--optimizer", "sgd", "--adam-8bit"])
    assert e.value.code == 2 and "--adam-8bit needs" in capsys.readouterr().err
    assert not out.exists()                                               # refused before anything was made

"""GPU: the second-order multistep solvers of the denoise loop (include/lcv_hip_solver.h, longcat_video/solver.py,
`solver=` / `--solver`).

1. lcv_cfg_lms_step against the numpy restatement (tests/solver_ref.py), bit for bit: x, f0 and the untouched f1 / f2, over
   n = 1, 7, 255, 256, 257, 65 537 (one more than the first launch's 256 x 256 threads: a second trip of its loop) and 262 145
   (one more than the step launch's 1024 x 256), B = 1, 2, 3, 1 to 3 terms, both signs, with and without `uncond`, aligned and
   offset by one float.
2. Zero-star: on inputs whose sums are exact in any order; on random inputs the partials against float64 within the summation
   bound and against the restated order bit for bit, and x bit-equal to the restatement fed the scale joined from them.
3. Run-to-run bits; refusals.
4. `denoise(solver=...)` against a test-side loop over the same model, on all three branches, under graph replay, with a step
   cache, and the Euler spellings.
5. A stub velocity field through the real loop: the second-order ratio.
6. The baseline runner with and without the flag.
"""
import math
from pathlib import Path

import numpy as np
import pytest
import torch

import solver_ref as S

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
BF16 = torch.bfloat16
F32 = torch.float32
DEV = "cuda"
NS = (1, 7, 255, 256, 257, 65537)
BS = (1, 2, 3)
SENTINEL = 7.25


# ---------------------------------------------------------------------------------------------------------- helpers
def _report(what, got, want):
    got, want = np.asarray(got, np.float32).ravel().view(np.uint32), np.asarray(want, np.float32).ravel().view(np.uint32)
    assert got.size == want.size, (what, got.size, want.size)
    bad = np.flatnonzero(got != want)
    if bad.size:
        i = int(bad[0])
        raise AssertionError(f"{what}: index {i} of {got.size}: got {got[i]:#010x} want {want[i]:#010x}; {bad.size} mismatches")


def _place(a, offset):
    """A device copy of the host array `a`, `offset` floats past an allocation's (at least 16-byte aligned) base."""
    a = np.ascontiguousarray(a, np.float32)
    buf = torch.empty(a.size + offset, dtype=F32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    t = buf[offset:].view(a.shape)
    t.copy_(torch.from_numpy(a))
    assert t.is_contiguous() and t.data_ptr() % 16 == 4 * offset
    return t


def _raw(*args):
    from lcv_hip import lib
    lib.call("lcv_cfg_lms_step", *args, torch.cuda.current_stream().cuda_stream)


def _lms(c, u, x, f1, f2, guidance, w, negate, zero_star, offset=0, ws=None):
    """One call through the C ABI on host arrays [B, n]: (x, f0, f1, f2, ws) read back; f1 / f2 are passed whenever given."""
    B, n = x.shape
    dc, dx = _place(c, 0), _place(x, offset)
    du = None if u is None else _place(u, 0)
    d1 = None if f1 is None else _place(f1, offset)
    d2 = None if f2 is None else _place(f2, offset)
    d0 = _place(np.full((B, n), SENTINEL, np.float32), offset)
    if ws is None and u is not None and zero_star:
        ws = torch.full((B, 256, 2), SENTINEL, dtype=F32, device=DEV)
    ww = [float(v) for v in w] + [0.0] * (3 - len(w))
    _raw(dc.data_ptr(), None if du is None else du.data_ptr(), dx.data_ptr(), d0.data_ptr(),
         None if d1 is None else d1.data_ptr(), None if d2 is None else d2.data_ptr(), None if ws is None else ws.data_ptr(),
         B, n, float(guidance), ww[0], ww[1], ww[2], len(w), int(negate), int(zero_star))
    torch.cuda.synchronize()
    host = lambda t: None if t is None else t.cpu().numpy()
    _report("cond was written", host(dc), c)
    if u is not None:
        _report("uncond was written", host(du), u)
    return host(dx), host(d0), host(d1), host(d2), host(ws)


_DRAWN = {}


def _drawn(B, n):
    """Host inputs, made once per shape and never written: cond, uncond, x, f1, f2 ~ N(0, 1) fp32."""
    key = (B, n)
    if key not in _DRAWN:
        rng = np.random.default_rng(977 * B + n)
        _DRAWN[key] = tuple(rng.standard_normal((B, n)).astype(np.float32) for _ in range(5))
    return _DRAWN[key]


WEIGHTS = {1: (-0.0625,), 2: (-0.09375003, 0.031250014), 3: (-0.12109375, 0.0918, -0.0302734)}


# ---------------------------------------------------------------------------------------------------------- 1. the sequence
def _check_case(B, n, terms, negate, guided, offset):
    c, u, x, f1, f2 = _drawn(B, n)
    w = WEIGHTS[terms]
    got_x, got_f0, got_f1, got_f2, _ = _lms(c, u if guided else None, x, f1, f2, 4.0, w, negate, False, offset=offset)
    want_x, want_f0 = S.lms_step(c, u if guided else None, x, (f1, f2), 4.0, w, negate)
    what = f"B {B} n {n} terms {terms} negate {negate} guided {guided} offset {offset}"
    _report(what + ": x", got_x, want_x)
    _report(what + ": f0", got_f0, want_f0)
    _report(what + ": f1 was written", got_f1, f1)
    _report(what + ": f2 was written", got_f2, f2)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("B", BS)
def test_element_sequence_bit_for_bit(B, n):
    for terms in (1, 2, 3):
        for negate in (0, 1):
            _check_case(B, n, terms, negate, guided=True, offset=0)           # uncond, zero-star off
            _check_case(B, n, terms, negate, guided=False, offset=0)          # uncond = NULL
            _check_case(B, n, terms, negate, guided=True, offset=1)           # x and the history one float past alignment


def test_the_step_launchs_loop_takes_a_second_trip():
    n = 1024 * 256 + 1
    for guided in (True, False):
        _check_case(2, n, 3, 1, guided=guided, offset=1)


def test_history_the_terms_do_not_ask_for_is_not_read():
    """With NaNs in f1 / f2 (and in the weights that go with them) a step of fewer terms is unchanged."""
    c, u, x, f1, f2 = _drawn(2, 257)
    nan = np.full_like(f1, np.nan)
    want_x, want_f0 = S.lms_step(c, u, x, (), 4.0, WEIGHTS[1], 1)
    B, n = x.shape
    dc, du, dx, d0, dn = _place(c, 0), _place(u, 0), _place(x, 0), _place(x, 0), _place(nan, 0)
    _raw(dc.data_ptr(), du.data_ptr(), dx.data_ptr(), d0.data_ptr(), dn.data_ptr(), dn.data_ptr(), None, B, n, 4.0,
         WEIGHTS[1][0], float("nan"), float("nan"), 1, 1, 0)
    _report("x", dx.cpu().numpy(), want_x)
    _report("f0", d0.cpu().numpy(), want_f0)
    want_x, _ = S.lms_step(c, u, x, (f1,), 4.0, WEIGHTS[2], 1)
    dx, d1 = _place(x, 0), _place(f1, 0)
    _raw(dc.data_ptr(), du.data_ptr(), dx.data_ptr(), d0.data_ptr(), d1.data_ptr(), dn.data_ptr(), None, B, n, 4.0,
         WEIGHTS[2][0], WEIGHTS[2][1], float("nan"), 2, 1, 0)
    _report("x, two terms", dx.cpu().numpy(), want_x)


# ---------------------------------------------------------------------------------------------------------- 2. zero-star
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("B", BS)
def test_zero_star_on_sums_that_are_exact_in_any_order(B, n):
    """cond and uncond are integers in -3 ... 3: every product is an integer of magnitude <= 9 and every partial sum, in any
    order, an integer below 9 * 65 537 < 2^24, so both sums are exact in fp32 and st is the same fp32 in any order."""
    rng = np.random.default_rng(31 * B + n)
    c = rng.integers(-3, 4, size=(B, n)).astype(np.float32)
    u = rng.integers(-3, 4, size=(B, n)).astype(np.float32)
    u[:, 0] = 2.0                                                     # <u, u> > 0
    _, _, x, f1, f2 = _drawn(B, n)
    dot, nrm, _ = S.sums_f64(c, u)
    assert (np.abs(dot) < 2 ** 24).all() and (nrm < 2 ** 24).all()
    st = (dot.astype(np.float32) / (nrm.astype(np.float32) + np.float32(1e-8))).astype(np.float32)
    for terms, negate, offset in ((1, 0, 0), (1, 1, 1), (2, 0, 1), (2, 1, 0), (3, 0, 0), (3, 1, 1)):
        got_x, got_f0, got_f1, got_f2, ws = _lms(c, u, x, f1, f2, 4.0, WEIGHTS[terms], negate, True, offset=offset)
        want_x, want_f0 = S.lms_step(c, u, x, (f1, f2), 4.0, WEIGHTS[terms], negate, st=st)
        _report("x", got_x, want_x)
        _report("f0", got_f0, want_f0)
        _report("f1", got_f1, f1)
        _report("f2", got_f2, f2)
        _report("partials", ws, S.partials(c, u))                     # every slot written, empty slices hold 0
        assert np.array_equal(S.join(ws), st)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("B", BS)
def test_zero_star_on_random_inputs(B, n):
    """The partials against float64: fixed-order fp32 addition of m terms makes at most m - 1 rounding errors of 2^-24 relative
    on the way of any term to the total (worst case, a chain; the tree here is at most trips + 17 additions deep), and a term
    carries c = 1 rounding of its own (the product; the float64 reference's is 2^-29 of that).  Hence (m + 1) * 2^-24 *
    sum |c u| per slice of m elements, (n + 1) * 2^-24 * sum |c u| for the joined totals, and the same form with u u for the
    norm.  Then the bits: the partials are those of the restated order, and x is bit-equal to the restatement fed the st joined
    from the device's partials in the documented order (this test does the bit comparison, not the bound on st)."""
    c, u, x, f1, f2 = _drawn(B, n)
    for terms, negate, offset in ((1, 0, 0), (2, 1, 0), (2, 0, 1)):   # the other forms: the same partials, the restated x
        gx, gf, _, _, ws = _lms(c, u, x, f1, f2, 4.0, WEIGHTS[terms], negate, True, offset=offset)
        _report(f"partials, {terms} terms", ws, S.partials(c, u))
        wx, wf = S.lms_step(c, u, x, (f1, f2), 4.0, WEIGHTS[terms], negate, st=S.join(ws))
        _report(f"x, {terms} terms negate {negate} offset {offset}", gx, wx)
        _report(f"f0, {terms} terms negate {negate} offset {offset}", gf, wf)
    got_x, got_f0, _, _, ws = _lms(c, u, x, f1, f2, 4.0, WEIGHTS[3], 1, True, offset=1)
    c64, u64 = c.astype(np.float64), u.astype(np.float64)
    idx = np.arange(n)
    part = (idx // 256) % 256                                         # element i belongs to part (i / 256) mod 256
    for b in range(B):
        for col, terms in ((0, c64[b] * u64[b]), (1, u64[b] * u64[b])):
            want = np.bincount(part, weights=terms, minlength=256)
            mag = np.bincount(part, weights=np.abs(terms), minlength=256)
            m = np.bincount(part, minlength=256)
            err = np.abs(ws[b, :, col].astype(np.float64) - want)
            bound = (m + 1) * 2.0 ** -24 * mag
            worst = int(np.argmax(err - bound))
            print(f"B {B} n {n} row {b} {'dot' if col == 0 else 'nrm'}: worst slice {worst}: error {err[worst]:.3e} bound {bound[worst]:.3e}")
            assert (err <= bound).all()
            assert (ws[b, m == 0, col] == 0).all()                    # empty slices write 0
    dot, nrm, mag = S.sums_f64(c, u)
    ws32 = ws.astype(np.float32)
    jd, jn = S._workgroup_sum(ws32[..., 0]).astype(np.float64), S._workgroup_sum(ws32[..., 1]).astype(np.float64)
    print(f"B {B} n {n}: dot error {np.abs(jd - dot).max():.3e}, nrm error {np.abs(jn - nrm).max():.3e}")
    assert (np.abs(jd - dot) <= (n + 1) * 2.0 ** -24 * mag).all() and (np.abs(jn - nrm) <= (n + 1) * 2.0 ** -24 * nrm).all()
    _report("partials in the restated order", ws, S.partials(c, u))
    st = S.join(ws)
    want_x, want_f0 = S.lms_step(c, u, x, (f1, f2), 4.0, WEIGHTS[3], 1, st=st)
    _report("x", got_x, want_x)
    _report("f0", got_f0, want_f0)


# ---------------------------------------------------------------------------------------------------------- 3. determinism, refusals
def test_two_runs_give_the_same_bits():
    c, u, x, f1, f2 = _drawn(3, 65537)
    a = _lms(c, u, x, f1, f2, 4.0, WEIGHTS[3], 1, True, offset=1)
    b = _lms(c, u, x, f1, f2, 4.0, WEIGHTS[3], 1, True, offset=1)
    for name, p, q in zip(("x", "f0", "f1", "f2", "ws"), a, b):
        _report(name, p, q)


def test_bad_arguments_return_einval_without_a_launch():
    from lcv_hip import lib, ops
    B, n = 2, 300
    t = [torch.full((B, n), SENTINEL, dtype=F32, device=DEV) for _ in range(6)]
    ws = torch.full((B, 256, 2), SENTINEL, dtype=F32, device=DEV)
    c, u, x, f0, f1, f2 = (v.data_ptr() for v in t)

    def refused(*args):
        with pytest.raises(lib.LcvError) as e:
            _raw(*args)
        assert e.value.code == -1 and not e.value.fatal, e.value

    tail = (B, n, 4.0, 0.5, 0.25, 0.125)
    refused(None, u, x, f0, f1, f2, ws.data_ptr(), *tail, 3, 1, 1)            # cond
    refused(c, u, None, f0, f1, f2, ws.data_ptr(), *tail, 3, 1, 1)            # x
    refused(c, u, x, None, f1, f2, ws.data_ptr(), *tail, 3, 1, 1)             # f0
    refused(c, u, x, f0, f1, f2, ws.data_ptr(), *tail, 0, 1, 1)               # terms
    refused(c, u, x, f0, f1, f2, ws.data_ptr(), *tail, 4, 1, 1)
    refused(c, u, x, f0, f1, f2, ws.data_ptr(), *tail, -1, 1, 1)
    refused(c, u, x, f0, None, f2, ws.data_ptr(), *tail, 2, 1, 1)             # f1 at two terms
    refused(c, u, x, f0, None, f2, ws.data_ptr(), *tail, 3, 1, 1)
    refused(c, u, x, f0, f1, None, ws.data_ptr(), *tail, 3, 1, 1)             # f2 at three
    refused(c, u, x, f0, f1, f2, None, *tail, 3, 1, 1)                        # zero-star without its workspace
    for other in (x, f1, f2, c, u):                                           # f0 over another operand
        refused(c, u, x, other, f1, f2, ws.data_ptr(), *tail, 3, 1, 1)
    torch.cuda.synchronize()
    assert all((v == SENTINEL).all() for v in t) and (ws == SENTINEL).all()   # nothing was launched
    # what is not refused: empty problems, and pointers nobody asks for
    _raw(c, u, x, f0, f1, f2, ws.data_ptr(), 0, n, 4.0, 0.5, 0.25, 0.125, 3, 1, 1)
    _raw(c, u, x, f0, f1, f2, ws.data_ptr(), B, 0, 4.0, 0.5, 0.25, 0.125, 3, 1, 1)
    torch.cuda.synchronize()
    assert all((v == SENTINEL).all() for v in t) and (ws == SENTINEL).all()
    _raw(c, None, x, f0, None, None, None, *tail, 1, 0, 1)                    # no uncond: no workspace needed; one term: no history
    torch.cuda.synchronize()
    assert (t[3] == SENTINEL).all() and (t[2] == SENTINEL + 0.5 * SENTINEL).all() and (ws == SENTINEL).all()
    # the wrapper
    with pytest.raises(lib.LcvError, match="earlier velocities"):
        ops.cfg_lms_step(t[0], t[1], t[2], t[3], None, None, 4.0, (0.5, 0.25))
    with pytest.raises(lib.LcvError, match="contiguous"):
        ops.cfg_lms_step(t[0], t[1], t[2], t[3].t(), None, None, 4.0, (0.5,))
    with pytest.raises(lib.LcvError, match="expected"):
        ops.cfg_lms_step(t[0], t[1], t[2].to(BF16), t[3], None, None, 4.0, (0.5,))


def test_the_wrapper_makes_the_same_call():
    from lcv_hip import ops
    c, u, x, f1, f2 = _drawn(2, 257)
    dev = [_place(a, 0) for a in (c, u, x, f1, f2)]
    f0 = torch.empty_like(dev[2])
    ops.cfg_lms_step(dev[0], dev[1], dev[2], f0, dev[3], dev[4], 4.0, WEIGHTS[3], negate=True, zero_star=True)
    st = S.join(S.partials(c, u))
    want_x, want_f0 = S.lms_step(c, u, x, (f1, f2), 4.0, WEIGHTS[3], 1, st=st)
    _report("x", dev[2].cpu().numpy(), want_x)
    _report("f0", f0.cpu().numpy(), want_f0)
    x1 = _place(x, 0)
    ops.cfg_lms_step(dev[0], None, x1, f0, None, None, 4.0, WEIGHTS[1], negate=False)
    want_x, want_f0 = S.lms_step(c, None, x, (), 4.0, WEIGHTS[1], 0)
    _report("x, no guidance", x1.cpu().numpy(), want_x)
    _report("f0, no guidance", f0.cpu().numpy(), want_f0)


# ---------------------------------------------------------------------------------------------------------- 4. the pipeline
STEPS = 4
CASES = {"t2v": dict(guidance=4.0, ncl=0, use_kv=True), "cond_kv": dict(guidance=4.0, ncl=2, use_kv=True),
         "cond_pinned": dict(guidance=4.0, ncl=2, use_kv=False), "t2v_nocfg": dict(guidance=1.0, ncl=0, use_kv=True),
         "cond_kv_nocfg": dict(guidance=1.0, ncl=2, use_kv=True), "cond_pinned_nocfg": dict(guidance=1.0, ncl=2, use_kv=False)}
_MODEL = {}


def _pipe():
    """The model and latent of tests/test_gpu_step_cache.py: synthetic weights, depth 3, 192 tokens per row."""
    if not _MODEL:
        from longcat_video.modules.longcat_video_dit import LongCatVideoTransformer3DModel
        from longcat_video.modules.scheduling_flow_match_euler_discrete import FlowMatchEulerDiscreteScheduler
        from longcat_video.pipeline_longcat_video import LongCatVideoPipeline
        dit = LongCatVideoTransformer3DModel(device=DEV, dtype=BF16, depth=3, hidden_size=256, num_heads=2,
                                             caption_channels=64).init_synthetic_(21).eval()
        pipe = LongCatVideoPipeline(scheduler=FlowMatchEulerDiscreteScheduler(), dit=dit)
        pipe.device = torch.device(DEV)
        g = torch.Generator().manual_seed(3)
        _MODEL["pipe"] = pipe
        _MODEL["lat"] = torch.randn(1, 16, 3, 16, 16, generator=g).to(DEV)
        pe = torch.randn(1, 1, 64, 64, generator=g).to(BF16).to(DEV)
        ne = torch.randn(1, 1, 64, 64, generator=g).to(BF16).to(DEV)
        pm = torch.zeros(1, 64, dtype=torch.int64, device=DEV); pm[:, :20] = 1
        nm = torch.zeros(1, 64, dtype=torch.int64, device=DEV); nm[:, :5] = 1
        _MODEL["text"] = (pe, pm, ne, nm)
    return _MODEL["pipe"]


def _denoise(case, **kw):
    """One 4-step denoise through the pipeline: (the result, the working latents after every step)."""
    pipe = _pipe()
    c = CASES[case]
    pe, pm, ne, nm = _MODEL["text"]
    cfg = c["guidance"] > 1
    seen = []
    out = pipe.denoise(_MODEL["lat"], pe, pm, ne if cfg else None, nm if cfg else None, num_cond_latents=c["ncl"],
                       num_inference_steps=STEPS, guidance_scale=c["guidance"], use_kv_cache=c["use_kv"],
                       step_callback=lambda i, x: seen.append(x.clone()), **kw)
    torch.cuda.synchronize()
    assert len(seen) == STEPS
    return out, seen


def _torch_step(c, u, x, hist, guidance, w, negate, zero_star):
    """The restated update in torch fp32, one operation per statement; st through the numpy restatement of the sums."""
    w = [float(np.float32(v)) for v in w]
    if u is not None:
        if zero_star:
            st = S.join(S.partials(c.reshape(1, -1).cpu().numpy(), u.reshape(1, -1).cpu().numpy()))
            u = u * float(st[0])
        d = c - u
        t = d * float(np.float32(guidance))
        v = u + t
    else:
        v = c
    f = -v if negate else v.clone()
    a = f * w[0]
    for k in range(1, len(w)):
        p = hist[k - 1] * w[k]
        a = a + p
    return x + a, f


@torch.no_grad()
def _loop(case, kind):
    """The test's own denoise loop: the same dit per step, the restated weights and the restated update."""
    pipe = _pipe()
    k = CASES[case]
    pe, pm, ne, nm = _MODEL["text"]
    cfg, ncl = k["guidance"] > 1, k["ncl"]
    sched = pipe.scheduler
    sched.set_timesteps(STEPS, sigmas=pipe.get_timesteps_sigmas(STEPS), device=DEV)
    sig, timesteps = list(sched._sigmas_host), sched.timesteps.tolist()
    lat = _MODEL["lat"].to(F32, copy=True).contiguous()
    kv, cond, work = None, None, lat
    if ncl > 0 and k["use_kv"]:
        cond = lat[:, :, :ncl].contiguous()
        kv = pipe.cache_clean_latents(cond.to(BF16), pe.shape[2], pe.shape[3])
        work = lat[:, :, ncl:].contiguous()
    emb, mask = (torch.cat([ne, pe]), torch.cat([nm, pm])) if cfg else (pe, pm)
    extra = {} if kv is None else {"kv_cache_dict": kv}
    hist, seen = [], []
    for i in range(STEPS):
        x_in = work.to(BF16)
        if cfg:
            x_in = x_in.expand(2, -1, -1, -1, -1)
        ts = torch.full((emb.shape[0], work.shape[2]), timesteps[i], device=DEV, dtype=BF16)
        if kv is None and ncl > 0:
            ts[:, :ncl] = 0
        pred = pipe.dit(hidden_states=x_in, timestep=ts, encoder_hidden_states=emb, encoder_attention_mask=mask,
                        num_cond_latents=ncl, **extra)
        c, u = (pred[1:2], pred[0:1]) if cfg else (pred, None)
        w = S.weights(sig, i, 0, kind)
        if kv is None and ncl > 0:
            new, f = _torch_step(c[:, :, ncl:], None if u is None else u[:, :, ncl:], work[:, :, ncl:], hist, k["guidance"], w,
                                 pipe.negate_pred, pipe.use_zero_star)
            work = torch.cat([work[:, :, :ncl], new], dim=2)
        else:
            work, f = _torch_step(c, u, work, hist, k["guidance"], w, pipe.negate_pred, pipe.use_zero_star)
        hist = [f] + hist[:1]
        seen.append(work.clone())
    return (work if cond is None else torch.cat([cond, work], dim=2)), seen


_RUNS = {}


def _run(case, kind):
    """denoise(solver=kind), computed once per (case, kind) and never written."""
    if (case, kind) not in _RUNS:
        _RUNS[(case, kind)] = _denoise(case, solver=kind)
    return _RUNS[(case, kind)]


@pytest.mark.parametrize("kind", ["ab2", "ab2c"])
@pytest.mark.parametrize("case", list(CASES))
def test_denoise_is_the_test_side_loop_bit_for_bit(case, kind):
    assert _pipe().negate_pred and _pipe().use_zero_star
    out, seen = _run(case, kind)
    want_out, want_seen = _loop(case, kind)
    for i in range(STEPS):
        assert torch.equal(seen[i], want_seen[i]), f"step {i}"
    assert torch.equal(out, want_out) and out.shape == _MODEL["lat"].shape
    if CASES[case]["ncl"]:
        assert torch.equal(out[:, :, :2], _MODEL["lat"][:, :, :2])    # the conditioning frames are untouched


@pytest.mark.parametrize("case", ["t2v", "cond_kv", "cond_pinned"])
def test_the_rules_differ_from_euler_after_the_first_step(case):
    """Step 0 is Euler's step in value, not in bits: lcv_cfg_euler_step is built with contraction allowed (tests/kernel_ref.py
    holds it to 2 ulps of the float64 value), this kernel without.  A handful of fp32 roundings of 2^-24 each stay below 1e-6
    relative; from step 1 on the rules weigh two velocities and differ by a share of the step itself."""
    plain, plain_seen = _denoise(case)
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
    for kind in ("ab2", "ab2c"):
        out, seen = _run(case, kind)
        print(case, kind, [f"{rel(seen[i], plain_seen[i]):.2e}" for i in range(STEPS)])
        assert rel(seen[0], plain_seen[0]) < 1e-6 and rel(seen[1], plain_seen[1]) > 1e-4
        assert torch.isfinite(out).all()
    assert not torch.equal(_run(case, "ab2")[0], _run(case, "ab2c")[0])


@pytest.mark.parametrize("case", ["t2v", "cond_kv", "cond_pinned"])
def test_none_and_euler_are_the_call_without_the_keyword(case, monkeypatch):
    from longcat_video import solver as solver_mod
    from lcv_hip import ops
    plain, plain_seen = _denoise(case)

    def never(*a, **k):
        raise AssertionError("the Euler path made a multistep call")
    monkeypatch.setattr(solver_mod.MultistepSolver, "__init__", never)
    monkeypatch.setattr(ops, "cfg_lms_step", never)
    for spelling in (None, "euler"):
        out, seen = _denoise(case, solver=spelling)
        assert torch.equal(out, plain) and all(torch.equal(a, b) for a, b in zip(seen, plain_seen))


@pytest.mark.parametrize("kind", ["ab2", "ab2c"])
@pytest.mark.parametrize("case", ["t2v", "cond_kv", "cond_pinned"])
def test_graph_replay_and_a_computing_step_cache_keep_the_bits(case, kind, monkeypatch):
    want, want_seen = _run(case, kind)
    out, seen = _denoise(case, solver=kind, step_cache=0.0)           # threshold 0: every step is computed
    assert torch.equal(out, want) and all(torch.equal(a, b) for a, b in zip(seen, want_seen))
    assert _pipe().last_step_cache_stats["computed"] == STEPS
    captured = []
    real = torch.cuda.CUDAGraph

    def counting(*a, **k):
        captured.append(1)
        return real(*a, **k)
    monkeypatch.setenv("LCV_DENOISE_GRAPH", "1")
    monkeypatch.setattr(torch.cuda, "CUDAGraph", counting)
    out, seen = _denoise(case, solver=kind)
    assert captured == [1]                                            # the forward was captured and replayed
    assert torch.equal(out, want) and all(torch.equal(a, b) for a, b in zip(seen, want_seen))


def test_a_solver_object_keeps_its_buffers_and_restarts_its_history():
    from longcat_video.solver import MultistepSolver
    s = MultistepSolver("ab2c")
    want, _ = _run("cond_kv", "ab2c")
    out, _ = _denoise("cond_kv", solver=s)
    ring = {t.data_ptr() for t in s._ring}
    assert torch.equal(out, want) and len(ring) == 3
    assert all(t.shape == (1, 16, 1, 16, 16) and t.dtype == F32 for t in s._ring)     # shaped like the working latents
    out, _ = _denoise("cond_kv", solver=s)                            # a second call: history restarted, buffers kept
    assert torch.equal(out, want) and {t.data_ptr() for t in s._ring} == ring
    s2 = MultistepSolver("ab2")
    _denoise("cond_pinned", solver=s2)
    assert len(s2._ring) == 2 and s2._ring[0].shape == (1, 16, 1, 16, 16)              # the target slice
    with pytest.raises(ValueError):
        _denoise("t2v", solver="ab3")


# ---------------------------------------------------------------------------------------------------------- 5. a stub field
class _ExpField:
    """dit(...) = exp(sigma_i) * K, sigma_i the scheduler's own host value at the stub's call count (the bf16 timestep it is
    handed is too coarse to recover sigma from)."""

    def __init__(self, pipe, K):
        self.pipe, self.K, self.calls = pipe, K, 0

    def __call__(self, hidden_states=None, timestep=None, **kw):
        sigma = self.pipe.scheduler._sigmas_host[self.calls]
        self.calls += 1
        return self.K * math.exp(sigma)


def test_second_order_through_the_real_loop():
    """dx/dsigma = -exp(sigma) K (the pipeline negates the model's output): x(0) = x(1) + (e - 1) K.  Halving the step halves
    a first-order error and quarters a second-order one; 2.5 and 3.5 sit between 2^1 and 2^2.  History indexing, the start-up
    step and the sign all have to be right for the ratio to reach 4."""
    from longcat_video.modules.scheduling_flow_match_euler_discrete import FlowMatchEulerDiscreteScheduler
    from longcat_video.pipeline_longcat_video import LongCatVideoPipeline
    g = torch.Generator().manual_seed(5)
    x1 = torch.randn(1, 16, 2, 8, 8, generator=g).to(DEV)
    K = torch.randn(1, 16, 2, 8, 8, generator=g).to(DEV)
    pe = torch.zeros(1, 1, 8, 64, dtype=BF16, device=DEV)
    want = x1.double() + (math.e - 1.0) * K.double()
    err = {}
    for kind in ("euler", "ab2", "ab2c"):
        for n in (16, 32):
            pipe = LongCatVideoPipeline(scheduler=FlowMatchEulerDiscreteScheduler(), dit=None)
            pipe.device = torch.device(DEV)
            pipe.dit = _ExpField(pipe, K)
            out = pipe.denoise(x1, pe, None, num_cond_latents=0, num_inference_steps=n, guidance_scale=1.0, solver=kind)
            assert pipe.dit.calls == n
            err[kind, n] = float((out.double() - want).norm() / want.norm())
        print(kind, f"{err[kind, 16]:.3e} {err[kind, 32]:.3e} ratio {err[kind, 16] / err[kind, 32]:.2f}")
    assert err["euler", 16] / err["euler", 32] < 2.5
    for kind in ("ab2", "ab2c"):
        assert err[kind, 16] / err[kind, 32] > 3.5, kind
        assert err[kind, 32] < err["euler", 32]


# ---------------------------------------------------------------------------------------------------------- 6. a runner
BASELINE = "baseline_experiment/scripts/run_baseline.py"
TINY_BASE = ["--checkpoint-dir", "synthetic:2:256:64", "--data-dir", "synthetic:1", "--num-cond-frames", "5", "--num-inference-steps", "4",
             "--num-gen-frames", "8"]
# the keys of a run at the parent commit
BASE_SUMMARY = {"experiment", "model", "checkpoint_dir", "resolution", "num_cond_frames", "num_gen_frames", "gen_start_frame",
                "num_frames_total", "num_inference_steps", "guidance_scale", "seed", "num_videos", "num_successful", "timing",
                "metrics", "runtime"}


def test_baseline_runner_with_and_without_the_flag(tmp_path, monkeypatch):
    import importlib.util
    import json
    from longcat_video import solver as solver_mod
    path = ROOT / "longcat-video-tta_amd" / BASELINE
    spec = importlib.util.spec_from_file_location("solver_runner_baseline", path)
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    steps = []
    real = solver_mod.MultistepSolver.step

    def counted(self, *a, **k):
        steps.append(self.kind)
        return real(self, *a, **k)
    monkeypatch.setattr(solver_mod.MultistepSolver, "step", counted)
    m.main(TINY_BASE + ["--output-dir", str(tmp_path / "on"), "--solver", "ab2c"])
    s = json.loads((tmp_path / "on" / "summary.json").read_text())
    assert set(s) == BASE_SUMMARY | {"solver"} and s["solver"] == "ab2c" and s["num_successful"] == 1
    assert steps == ["ab2c"] * 4                                      # the continuation's four steps went through the solver
    for flag in ([], ["--solver", "euler"]):
        m.main(TINY_BASE + ["--output-dir", str(tmp_path / "off")] + flag)
        s = json.loads((tmp_path / "off" / "summary.json").read_text())
        assert set(s) == BASE_SUMMARY and s["num_successful"] == 1
    assert len(steps) == 4

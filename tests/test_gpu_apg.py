"""GPU: the adaptive projected guidance of the CFG denoise loop (include/lcv_hip_apg.h, longcat_video/apg.py, `apg=` / `--apg`).

1. lcv_cfg_apg against the numpy restatement (tests/apg_ref.py), bit for bit: v, diff, ws[1] and out (and ws[0] under zero-star)
   over B = 1, 2 and n = 1, 255, 256, 257, 65 535, 65 536, 65 537, 2 * 65 536 + 77 (the thread, workgroup and stride edges of the
   partial sums), zero-star on and off, a threshold that clamps, one that does not and none, eta = 0, 0.5, 1, two successive
   calls with beta = -0.5; buffers aligned and offset by one float, `v` a buffer of its own and `v == cond`, with and without
   `out`; canary words either side of every output; cond and uncond are never written (cond only where it is `v`).
2. The same call twice gives the same bits; the zero-star partials are those lcv_cfg_delta_store writes for the same rows, so
   `st` is the same.
3. Refusals without a launch; empty problems; the wrapper.
4. `denoise(apg=...)` on the model of tests/test_gpu_cfg_reuse.py: eta = 1 stays within the host test's tolerance of the plain
   run after one step; eta = 0 differs and fills `last_apg_stats`; with `solver="ab2"` the run is a test-side loop that feeds
   `lms.step` the restatement's v, bit for bit, conditioning frames untouched; the refusals.
5. The baseline runner with the flag.
"""
import math
from pathlib import Path

import numpy as np
import pytest
import torch

import apg_ref as A
import solver_ref as S
import test_apg_host as H
import test_gpu_cfg_reuse as R

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
BF16 = torch.bfloat16
F32 = torch.float32
DEV = "cuda"
NS = (1, 255, 256, 257, 65535, 65536, 65537, 2 * 65536 + 77)
BS = (1, 2)
SENTINEL = 7.25
GUARD = 8                  # canary words either side of every output
GUIDANCE = 4.0
_report = R._report


# ---------------------------------------------------------------------------------------------------------- helpers
class _Guarded:
    """A device buffer of GUARD canary words, `offset` alignment words, the payload and GUARD canary words; `view` is the
    payload, `offset` floats past a 16-byte boundary."""

    def __init__(self, a, offset, shape=None):
        if a is None:
            a = np.full(shape, SENTINEL, np.float32)
        a = np.ascontiguousarray(a, np.float32)
        assert GUARD % 4 == 0
        self.buf = torch.full((GUARD + offset + a.size + GUARD,), SENTINEL, dtype=F32, device=DEV)
        assert self.buf.data_ptr() % 16 == 0
        self.lo = GUARD + offset
        self.view = self.buf[self.lo: self.lo + a.size].view(a.shape)
        self.view.copy_(torch.from_numpy(a))
        assert self.view.is_contiguous() and self.view.data_ptr() % 16 == 4 * offset

    def ptr(self):
        return self.view.data_ptr()

    def host(self, what):
        """The payload on the host, after checking that the words either side of it still hold the canary."""
        b = self.buf.cpu().numpy()
        n = self.view.numel()
        assert (b[:self.lo] == SENTINEL).all() and (b[self.lo + n:] == SENTINEL).all(), f"{what}: written outside its buffer"
        return b[self.lo: self.lo + n].reshape(tuple(self.view.shape))


def _raw(name, *args):
    from lcv_hip import lib
    lib.call(name, *args, torch.cuda.current_stream().cuda_stream)


def _call(c, u, old, guidance, eta, radius, beta, zero_star, have_momentum, offset=0, alias=False, with_out=True):
    """One lcv_cfg_apg through the C ABI on host arrays [B, n]: dict(v, diff, ws [2, B, 256, 4], out [B, 4] or None) read back.
    `old` None fills diff with the sentinel.  Every buffer sits `offset` floats past alignment; `alias`: v is cond."""
    B, n = c.shape
    dc, du = _Guarded(c, offset), _Guarded(u, offset)
    dd = _Guarded(old, offset, (B, n))
    dv = dc if alias else _Guarded(None, offset, (B, n))
    ws = _Guarded(None, offset, (2, B, 256, 4))
    out = _Guarded(None, offset, (B, 4)) if with_out else None
    _raw("lcv_cfg_apg", dc.ptr(), du.ptr(), dd.ptr(), dv.ptr(), ws.ptr(), None if out is None else out.ptr(), B, n,
         float(guidance), float(eta), float(radius), float(beta), int(zero_star), int(have_momentum))
    torch.cuda.synchronize()
    _report("uncond was written", du.host("uncond"), u)
    if not alias:
        _report("cond was written", dc.host("cond"), c)
    return {"v": dv.host("v"), "diff": dd.host("diff"), "ws": ws.host("ws"), "out": None if out is None else out.host("out")}


def _check(what, got, want, zero_star):
    _report(what + ": diff", got["diff"], want["diff"])
    _report(what + ": ws[1]", got["ws"][1], want["ws1"])
    if zero_star:
        _report(what + ": ws[0]", got["ws"][0], want["ws0"])
    else:
        assert (got["ws"][0] == SENTINEL).all(), what + ": ws[0] was written without zero-star"
    if got["out"] is not None:
        _report(what + ": out", got["out"], want["out"])
    _report(what + ": v", got["v"], want["v"])


_DRAWN = {}


def _drawn(B, n):
    """Host inputs, made once per shape and never written: c ~ N(0, 1), u = 0.5 c + 0.5 noise, an old correction ~ N(0, 1)."""
    if (B, n) not in _DRAWN:
        rng = np.random.default_rng(733 * B + n)
        c = rng.standard_normal((B, n)).astype(np.float32)
        u = (0.5 * c + 0.5 * rng.standard_normal((B, n))).astype(np.float32)
        _DRAWN[(B, n)] = (c, u, rng.standard_normal((B, n)).astype(np.float32))
    return _DRAWN[(B, n)]


def _radii(c, u, n):
    """(a radius that clamps, one that does not, none) for these rows: a quarter and four times the correction's own RMS scale
    (||c - u'|| is about 0.7 sqrt(n) here, under zero-star too), rounded to fp32 once as the call rounds it."""
    return tuple(float(np.float32(R * math.sqrt(n))) for R in (0.25, 4.0)) + (0.0,)


# ---------------------------------------------------------------------------------------------------------- 1. the sequences
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("B", BS)
def test_apg_bit_for_bit(B, n):
    c, u, old = _drawn(B, n)
    k = 0
    for zero_star in (False, True):
        for mode, radius in zip(("clamps", "does not clamp", "none"), _radii(c, u, n)):
            for eta in (0.0, 0.5, 1.0):
                want = A.apg(c, u, None, GUIDANCE, eta, radius, 0.0, zero_star)
                s = want["out"][:, 3]
                if n > 1:                                             # one element: d may be 0 or tiny; s is what it is
                    assert ((s < 1) if mode == "clamps" else (s == 1)).all(), (mode, s)
                # the set-ups take turns over the combinations: offset, v == cond, out = NULL
                offset, alias, with_out = k % 2, (k // 2) % 2 == 1, (k // 3) % 2 == 0
                k += 1
                what = f"B {B} n {n} zero-star {zero_star} threshold {mode} eta {eta} offset {offset} alias {alias} out {with_out}"
                got = _call(c, u, None, GUIDANCE, eta, radius, 0.0, zero_star, False, offset, alias, with_out)
                _check(what, got, want, zero_star)
    # beta != 0 without a momentum yet (the sentinel in diff is not read), and with have_momentum but beta == 0
    want = A.apg(c, u, None, GUIDANCE, 0.5, 0.0, 0.0, True)
    _check("first call, beta -0.5", _call(c, u, None, GUIDANCE, 0.5, 0.0, -0.5, True, False, 1), want, True)
    _check("momentum, beta 0", _call(c, u, old, GUIDANCE, 0.5, 0.0, 0.0, True, True, 1), want, True)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("B", BS)
def test_two_successive_calls_with_a_momentum(B, n):
    c, u, _ = _drawn(B, n)
    c2, u2 = c[:, ::-1].copy(), (0.25 * c + u).astype(np.float32)[:, ::-1].copy()      # other rows for the second call
    radius = _radii(c, u, n)[0]
    for zero_star, offset, alias in ((False, 1, False), (True, 0, True)):
        w1 = A.apg(c, u, None, GUIDANCE, 0.5, radius, -0.5, zero_star)
        g1 = _call(c, u, None, GUIDANCE, 0.5, radius, -0.5, zero_star, False, offset, alias)
        _check(f"B {B} n {n} first call", g1, w1, zero_star)
        w2 = A.apg(c2, u2, w1["diff"], GUIDANCE, 0.5, radius, -0.5, zero_star)
        g2 = _call(c2, u2, g1["diff"], GUIDANCE, 0.5, radius, -0.5, zero_star, True, offset, alias)
        _check(f"B {B} n {n} second call", g2, w2, zero_star)
        if n > 1:
            assert not np.array_equal(w2["diff"], A.correction(c2, u2, st=w2["st"]))      # the momentum did enter


# ---------------------------------------------------------------------------------------------------------- 2. the same bits
@pytest.mark.parametrize("n", (257, 65537, 2 * 65536 + 77))
def test_the_same_call_twice_and_the_star_scale_of_the_reuse_store(n):
    B = 2
    c, u, old = _drawn(B, n)
    radius = _radii(c, u, n)[0]
    a = _call(c, u, old, GUIDANCE, 0.5, radius, -0.5, True, True, 1)
    b = _call(c, u, old, GUIDANCE, 0.5, radius, -0.5, True, True, 1)
    for key in ("v", "diff", "ws", "out"):
        _report(key + ", second run", b[key], a[key])
    # the partial pairs lcv_cfg_delta_store writes for the same rows: the same bits, so the same st
    delta, ws, _ = R._store(c, u, None, GUIDANCE, True, False)
    _report("against lcv_cfg_delta_store's partials", a["ws"][0][..., :2], ws[0])
    assert np.array_equal(S.join(a["ws"][0][..., :2]), S.join(ws[0]))
    assert not a["ws"][0][..., 2:].any()                              # the unused slots hold 0


# ---------------------------------------------------------------------------------------------------------- 3. refusals
def test_bad_arguments_return_einval_without_a_launch():
    from lcv_hip import lib, ops
    B, n = 2, 300
    t = [torch.full((B, n), SENTINEL, dtype=F32, device=DEV) for _ in range(4)]
    ws = torch.full((2, B, 256, 4), SENTINEL, dtype=F32, device=DEV)
    out = torch.full((B, 4), SENTINEL, dtype=F32, device=DEV)
    c, u, d, v = (x.data_ptr() for x in t)
    w, o = ws.data_ptr(), out.data_ptr()
    tail = (B, n, 4.0, 0.5, 1.0, -0.5, 1, 1)

    def refused(*args):
        with pytest.raises(lib.LcvError) as e:
            _raw("lcv_cfg_apg", *args)
        assert e.value.code == -1 and not e.value.fatal, e.value

    untouched = lambda: all((x == SENTINEL).all() for x in t) and (ws == SENTINEL).all() and (out == SENTINEL).all()
    refused(None, u, d, v, w, o, *tail)                                       # cond
    refused(c, None, d, v, w, o, *tail)                                       # uncond
    refused(c, u, None, v, w, o, *tail)                                       # diff
    refused(c, u, d, None, w, o, *tail)                                       # v
    refused(c, u, d, v, None, o, *tail)                                       # ws
    refused(c, u, d, u, w, o, *tail)                                          # v over uncond
    refused(c, u, u, v, w, o, *tail)                                          # diff over uncond
    refused(c, u, c, v, w, o, *tail)                                          # diff over cond
    refused(c, u, d, d, w, o, *tail)                                          # v over diff
    refused(c, u, d, v, w, o, 65536, *tail[1:])                               # B
    torch.cuda.synchronize()
    assert untouched()                                                        # nothing was launched
    for BB, nn in ((0, n), (B, 0)):                                           # empty problems are fine and launch nothing
        _raw("lcv_cfg_apg", c, u, d, v, w, o, BB, nn, *tail[2:])
    torch.cuda.synchronize()
    assert untouched()
    # the wrapper
    with pytest.raises(lib.LcvError, match="expected"):
        ops.cfg_apg(t[0].to(BF16), t[1], t[2], 4.0, 0.0, None, 0.0, True, False)
    with pytest.raises(lib.LcvError, match="contiguous"):
        ops.cfg_apg(t[0], t[1], t[2].t(), 4.0, 0.0, None, 0.0, True, False)
    with pytest.raises(lib.LcvError, match="one size"):
        ops.cfg_apg(t[0], t[1][:1], t[2], 4.0, 0.0, None, 0.0, True, False)
    with pytest.raises(lib.LcvError, match="fp32 words"):
        ops.cfg_apg(t[0], t[1], t[2], 4.0, 0.0, None, 0.0, True, False, out=out[:1])
    with pytest.raises(lib.LcvError, match="buffer of its own"):
        ops.cfg_apg(t[0], t[1], t[2], 4.0, 0.0, None, 0.0, True, False, v=t[2])
    assert untouched()


def test_the_wrapper_makes_the_same_call():
    from lcv_hip import ops
    c, u, old = _drawn(2, 257)
    dc, du, dd = R._place(c, 0), R._place(u, 1), R._place(old, 1)
    out = torch.full((2, 4), SENTINEL, dtype=F32, device=DEV)
    radius = _radii(c, u, 257)[0]
    v = ops.cfg_apg(dc, du, dd, GUIDANCE, 0.5, radius, -0.5, True, True, out=out)
    want = A.apg(c, u, old, GUIDANCE, 0.5, radius, -0.5, True)
    assert v.data_ptr() != dc.data_ptr()                              # a tensor of its own by default
    _report("v", v.cpu().numpy(), want["v"]); _report("diff", dd.cpu().numpy(), want["diff"]); _report("out", out.cpu().numpy(), want["out"])
    _report("cond was written", dc.cpu().numpy(), c)
    ws = ops.cfg_apg_workspace(2, dc.device)
    assert ws.shape == (2, 2, 256, 4) and ops.cfg_apg_workspace(2, dc.device) is ws        # cached per (device, B)
    assert ops.cfg_apg_workspace(3, dc.device) is not ws
    _report("ws[1]", ws[1].cpu().numpy(), want["ws1"])
    # no threshold is radius None; v over cond; no out
    assert ops.cfg_apg(dc, du, dd, GUIDANCE, 1.0, None, 0.0, False, False, v=dc) is dc
    _report("v in place", dc.cpu().numpy(), A.apg(c, u, None, GUIDANCE, 1.0, 0.0, 0.0, False)["v"])


# ---------------------------------------------------------------------------------------------------------- 4. the pipeline
# An RMS per element that clamps the correction of this model: its two rows are bf16 outputs of magnitude about 1 under different
# texts, so where they differ at all they differ by a bf16 step, about 1e-3, in some element, and one such element alone gives
# the correction a norm above 1e-5 sqrt(n) for every n here (at most 12 288).
THRESHOLD = 1e-5
def _start(case):
    """The latents the first step updates."""
    lat, k = R._MODEL["lat"], R.CASES[case]
    return lat[:, :, k["ncl"]:] if (k["ncl"] and k["use_kv"]) else lat


@pytest.mark.parametrize("case", list(R.CASES))
def test_eta_one_stays_within_the_tolerance_of_the_plain_run(case):
    """After one step x = x0 + dt v.  The two guided outputs are each within their measured distance (x 1.5, tests/test_apg_host.py)
    of the float64 plain rule, in units of max |v|, and dt max |v| is the largest move of the plain run's first step; each
    update rounds its product and its sum once, EPS of the move and of the state each, in both runs."""
    from longcat_video.apg import ProjectedGuidance
    steps = 4
    plain, plain_seen = R._denoise(case, steps)
    assert R._pipe().last_apg_stats is None
    out, seen = R._denoise(case, steps, apg=ProjectedGuidance(eta=1.0))
    x0 = _start(case).double()
    move = float((plain_seen[0].double() - x0).abs().max())
    bound = (H.IDENTITY_TOL + 1.5 * H.PLAIN_F32_DISTANCE) * move + 2 * H.EPS * (move + float(plain_seen[0].abs().max()))
    dist = float((seen[0].double() - plain_seen[0].double()).abs().max())
    print(f"{case}: after one step: distance {dist:.3e}, bound {bound:.3e} (largest move {move:.3e}); after {steps}: "
          f"{float((out.double() - plain.double()).abs().max()):.3e}")
    assert move > 0 and dist <= bound
    s = R._pipe().last_apg_stats
    assert s["eta"] == 1.0 and s["guided"] == steps and s["clamp"] == [1.0] * steps
    assert torch.isfinite(out).all() and out.shape == plain.shape
    R._denoise(case, steps)
    assert R._pipe().last_apg_stats is None                           # None again without the keyword


def test_eta_zero_differs_and_fills_the_statistics():
    from longcat_video.apg import ProjectedGuidance
    steps = 4
    plain, _ = R._denoise("cond_kv", steps)
    g = ProjectedGuidance(eta=0.0, norm_threshold=THRESHOLD)
    out, _ = R._denoise("cond_kv", steps, apg=g)
    assert not torch.equal(out, plain) and torch.isfinite(out).all()
    assert torch.equal(out[:, :, :2], R._MODEL["lat"][:, :, :2])      # the conditioning frames are untouched
    s = R._pipe().last_apg_stats
    print(s)
    assert s["eta"] == 0.0 and s["norm_threshold"] == THRESHOLD and s["momentum"] == 0.0 and s["guided"] == steps
    assert len(s["clamp"]) == len(s["cosine"]) == steps
    assert all(0 < v < 1 for v in s["clamp"]) and all(-1 <= v <= 1 and math.isfinite(v) for v in s["cosine"])
    assert g._diff.shape == (1, 16, 1, 16, 16) and g._trace.shape == (steps, 1, 4)
    ptr = g._diff.data_ptr()
    again, _ = R._denoise("cond_kv", steps, apg=g)                    # a second call: the buffers stay, the result too
    assert torch.equal(again, out) and g._diff.data_ptr() == ptr
    both, _ = R._denoise("cond_kv", steps, apg=ProjectedGuidance(eta=0.0, norm_threshold=THRESHOLD), step_cache=0.0)
    assert torch.isfinite(both).all() and R._pipe().last_apg_stats["guided"] == steps      # composes with a step cache


@torch.no_grad()
def _loop(case, steps, kind, eta, R_rms, beta):
    """The test's own denoise loop: the same dit at batch 2 per step, v through the numpy restatement, the update through
    `lms.step(v, None, ...)`."""
    from longcat_video.solver import MultistepSolver
    pipe = R._pipe()
    k = R.CASES[case]
    pe, pm, ne, nm = R._MODEL["text"]
    ncl = k["ncl"]
    sched = pipe.scheduler
    sched.set_timesteps(steps, sigmas=pipe.get_timesteps_sigmas(steps), device=DEV)
    sig, timesteps = list(sched._sigmas_host), sched.timesteps.tolist()
    lat = R._MODEL["lat"].to(F32, copy=True).contiguous()
    kv, cond, work = None, None, lat
    if ncl > 0 and k["use_kv"]:
        cond = lat[:, :, :ncl].contiguous()
        kv = pipe.cache_clean_latents(cond.to(BF16), pe.shape[2], pe.shape[3])
        work = lat[:, :, ncl:].contiguous()
    extra = {} if kv is None else {"kv_cache_dict": kv}
    pinned = kv is None and ncl > 0
    lms = MultistepSolver(kind)
    lms.begin(0)
    emb, mask = torch.cat([ne, pe]), torch.cat([nm, pm])
    old, seen = None, []
    for i in range(steps):
        x_in = work.to(BF16).expand(2, -1, -1, -1, -1)
        ts = torch.full((2, work.shape[2]), timesteps[i], device=DEV, dtype=BF16)
        if pinned:
            ts[:, :ncl] = 0
        pred = pipe.dit(hidden_states=x_in, timestep=ts, encoder_hidden_states=emb, encoder_attention_mask=mask,
                        num_cond_latents=ncl, **extra)
        cut = (lambda p: p[:, :, ncl:].contiguous()) if pinned else (lambda p: p)
        x = work[:, :, ncl:].contiguous() if pinned else work
        c, u = cut(pred[1:2]), cut(pred[0:1])
        n = c.numel()
        r = A.apg(c.reshape(1, n).cpu().numpy(), u.reshape(1, n).cpu().numpy(), old, GUIDANCE, eta,
                  float(np.float32(R_rms * math.sqrt(n))), beta, pipe.use_zero_star)
        old = r["diff"]
        v = torch.from_numpy(r["v"]).to(DEV).reshape(c.shape)
        lms.step(v, None, x, i, sig, GUIDANCE, pipe.negate_pred, pipe.use_zero_star)
        if pinned:
            work[:, :, ncl:].copy_(x)
        seen.append(work.clone())
    return (work if cond is None else torch.cat([cond, work], dim=2)), seen


@pytest.mark.parametrize("case", list(R.CASES))
def test_with_a_solver_it_is_the_test_side_loop_bit_for_bit(case):
    from longcat_video.apg import ProjectedGuidance
    steps, eta, R_rms, beta = 4, 0.5, THRESHOLD, -0.5
    assert R._pipe().negate_pred and R._pipe().use_zero_star
    out, seen = R._denoise(case, steps, solver="ab2", apg=ProjectedGuidance(eta=eta, norm_threshold=R_rms, momentum=beta))
    s = R._pipe().last_apg_stats
    want_out, want_seen = _loop(case, steps, "ab2", eta, R_rms, beta)
    for i in range(steps):
        assert torch.equal(seen[i], want_seen[i]), f"step {i}"
    assert torch.equal(out, want_out) and out.shape == R._MODEL["lat"].shape
    if R.CASES[case]["ncl"]:
        assert torch.equal(out[:, :, :2], R._MODEL["lat"][:, :, :2])  # the conditioning frames are untouched
    print(case, s)
    assert s["guided"] == steps and s["momentum"] == beta and all(0 < v < 1 for v in s["clamp"])
    plain, _ = R._denoise(case, steps, solver="ab2")
    assert not torch.equal(out, plain)


def test_the_pipeline_refuses_what_it_cannot_do(monkeypatch):
    from longcat_video.apg import ProjectedGuidance
    g = ProjectedGuidance()
    with pytest.raises(ValueError, match="cfg_reuse"):
        R._denoise("t2v", 4, apg=g, cfg_reuse=2)
    with pytest.raises(ValueError, match="guidance"):
        R._denoise("t2v", 4, guidance=1.0, apg=g)
    pipe = R._pipe()
    pe, pm, ne, nm = R._MODEL["text"]
    with pytest.raises(ValueError, match="guidance"):
        pipe.denoise(R._MODEL["lat"], pe, pm, None, None, num_inference_steps=4, guidance_scale=4.0, apg=g)
    monkeypatch.setattr(pipe.dit, "_sp_group", object(), raising=False)
    with pytest.raises(ValueError, match="sequence-parallel"):
        R._denoise("t2v", 4, apg=g)
    monkeypatch.undo()
    assert g._diff is None and pipe.last_apg_stats is None            # nothing was allocated or recorded


# ---------------------------------------------------------------------------------------------------------- 5. a runner
def test_baseline_runner_with_the_flag(tmp_path):
    import importlib.util
    import json
    path = ROOT / "longcat-video-tta_amd" / R.BASELINE
    spec = importlib.util.spec_from_file_location("apg_runner_baseline", path)
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    m.main(R.TINY_BASE + ["--output-dir", str(tmp_path / "on"), "--apg", "--apg-eta", "0.5", "--apg-norm-threshold", "0.5",
                          "--apg-momentum", "-0.25"])
    s = json.loads((tmp_path / "on" / "summary.json").read_text())
    assert set(s) == R.BASE_SUMMARY | {"apg", "apg_eta", "apg_norm_threshold", "apg_momentum", "apg_per_video"}
    assert s["apg"] is True and s["apg_eta"] == 0.5 and s["apg_norm_threshold"] == 0.5 and s["apg_momentum"] == -0.25
    assert s["num_successful"] == 1 and len(s["apg_per_video"]) == 1
    (stats,) = s["apg_per_video"].values()
    assert stats["eta"] == 0.5 and stats["norm_threshold"] == 0.5 and stats["momentum"] == -0.25 and stats["guided"] == 4
    assert len(stats["clamp"]) == len(stats["cosine"]) == 4 and all(0 < v <= 1 for v in stats["clamp"])

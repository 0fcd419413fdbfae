"""Host side of the adaptive projected guidance of the CFG denoise loop (`--apg`, longcat_video/apg.py, include/lcv_hip_apg.h):
the flags on every runner's parser with their refusals and records, the bookkeeping of `ProjectedGuidance` on a fake backend,
the properties of the numpy restatement (tests/apg_ref.py) against its float64 form, its identity with the plain rule, and the
header against the binding.  No GPU."""
import importlib.util
import math
import sys
from pathlib import Path

import numpy as np
import pytest

import apg_ref as A

ROOT = Path(__file__).resolve().parents[1]
PKG = ROOT / "longcat-video-tta_amd"
RUNNERS = ["delta_experiment/scripts/run_delta_a.py", "delta_experiment/scripts/run_delta_b.py",
           "delta_experiment/scripts/run_delta_c.py", "delta_experiment/scripts/run_film_tta.py",
           "delta_experiment/scripts/run_norm_tune_tta.py", "lora_experiment/scripts/run_full_tta.py",
           "lora_experiment/scripts/run_lora_tta.py", "baseline_experiment/scripts/run_baseline.py"]
BASE = ["--checkpoint-dir", "synthetic", "--data-dir", "synthetic:1", "--output-dir", "unused"]
EPS = 2.0 ** -24                     # half an fp32 ulp, relative: the error of one rounded operation
GUIDANCE = 4.0

# The identity with the plain rule (eta = 1, no threshold, no momentum).  Distance: max |a - ref| / max |ref| against the float64
# plain rule.  Measured here on the CPU on `_identity_inputs` (B 2, n 12 288 and 65 537, zero-star on and off), the worst case:
#   the plain rule's fp32 restatement   1.109e-07   (n 12 288, zero-star on)
#   the APG fp32 restatement            1.287e-07   (n 12 288, zero-star on)
# The tolerance is 1.5 x the APG restatement's measured distance, the project's margin; the GPU test of the pipeline uses both.
PLAIN_F32_DISTANCE = 1.109e-07
APG_F32_DISTANCE = 1.287e-07
IDENTITY_TOL = 1.5 * APG_F32_DISTANCE


def rel_distance(a, ref):
    a, ref = np.asarray(a, np.float64), np.asarray(ref, np.float64)
    return float(np.abs(a - ref).max() / np.abs(ref).max())


_INPUTS = {}


def _identity_inputs(n, B=2):
    """Seeded, made once and never written: c ~ N(0, 1), u = 0.5 c + 0.5 noise (so <d, c> and <c, c> are well conditioned), and
    an old correction ~ N(0, 1); fp32."""
    if (B, n) not in _INPUTS:
        rng = np.random.default_rng(977 * B + n)
        c = rng.standard_normal((B, n)).astype(np.float32)
        u = (0.5 * c + 0.5 * rng.standard_normal((B, n))).astype(np.float32)
        _INPUTS[(B, n)] = (c, u, rng.standard_normal((B, n)).astype(np.float32))
    return _INPUTS[(B, n)]


# ---------------------------------------------------------------------------------------------------------- the parsers
def _parser(rel):
    path = PKG / rel
    sys.path.insert(0, str(path.parent))
    try:
        spec = importlib.util.spec_from_file_location("apg_parser_" + path.stem, path)
        m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    finally:
        sys.path.remove(str(path.parent))
    if hasattr(m, "parse_args"):
        return m.parse_args
    from tta import cli_args as C
    return lambda argv: C.parse_with_step_cache(m.build_parser(), argv)


@pytest.mark.parametrize("rel", RUNNERS)
def test_every_runner_takes_the_flags(rel):
    from tta import cli_args as C
    from longcat_video.apg import ProjectedGuidance
    parse = _parser(rel)
    a = parse(BASE + ["--apg", "--apg-eta", "0.25", "--apg-norm-threshold", "1.5", "--apg-momentum", "-0.5"])
    assert a.apg is True and a.apg_eta == 0.25 and a.apg_norm_threshold == 1.5 and a.apg_momentum == -0.5
    assert C.apg_record(a) == {"apg": True, "apg_eta": 0.25, "apg_norm_threshold": 1.5, "apg_momentum": -0.5}
    g = C.apg_from_args(a)
    assert isinstance(g, ProjectedGuidance) and (g.eta, g.norm_threshold, g.momentum) == (0.25, 1.5, -0.5)
    assert C.apg_from_args(a) is not g                                # one per continuation
    a = parse(BASE + ["--apg"])                                       # the defaults
    assert a.apg is True and a.apg_eta == 0.0 and a.apg_norm_threshold is None and a.apg_momentum == 0.0
    assert C.apg_record(a) == {"apg": True, "apg_eta": 0.0, "apg_norm_threshold": None, "apg_momentum": 0.0}
    g = C.apg_from_args(a)
    assert (g.eta, g.norm_threshold, g.momentum) == (0.0, None, 0.0)
    a = parse(BASE + ["--apg", "--solver", "ab2", "--step-cache", "0.1", "--guidance-scale", "7.5"])   # composes with both
    assert a.apg and a.solver == "ab2" and a.step_cache == 0.1
    a = parse(BASE)                                                   # without the flag: nothing
    assert a.apg is False and a.apg_eta == 0.0 and a.apg_norm_threshold is None and a.apg_momentum == 0.0
    assert C.apg_record(a) == {} and C.apg_from_args(a) is None and C.apg_result({}) == {}
    assert C.apg_result({"_apg": {"guided": 2}}) == {"apg": {"guided": 2}}


@pytest.mark.parametrize("rel", RUNNERS)
@pytest.mark.parametrize("bad,said", [(["--apg-eta", "0.5"], "--apg-eta needs --apg"),
                                      (["--apg-eta", "0.0"], "--apg-eta needs --apg"),               # the default's value too
                                      (["--apg-norm-threshold", "2"], "--apg-norm-threshold needs --apg"),
                                      (["--apg-momentum", "0"], "--apg-momentum needs --apg"),
                                      (["--apg", "--cfg-reuse", "2"], "cannot be combined with --cfg-reuse"),
                                      (["--apg", "--guidance-scale", "1.0"], "--guidance-scale must be > 1"),
                                      (["--apg", "--guidance-scale", "0.5"], "--guidance-scale must be > 1"),
                                      (["--apg", "--apg-eta", "nan"], "ETA must be a finite number"),
                                      (["--apg", "--apg-eta", "inf"], "ETA must be a finite number"),
                                      (["--apg", "--apg-norm-threshold", "0"], "R must be a finite number > 0"),
                                      (["--apg", "--apg-norm-threshold", "-1"], "R must be a finite number > 0"),
                                      (["--apg", "--apg-norm-threshold", "nan"], "R must be a finite number > 0"),
                                      (["--apg", "--apg-momentum", "1"], "BETA must be in (-1, 1)"),
                                      (["--apg", "--apg-momentum", "-1.0"], "BETA must be in (-1, 1)"),
                                      (["--apg", "--apg-momentum", "nan"], "BETA must be in (-1, 1)"),
                                      (["--apg", "--apg-eta", "x"], "invalid float value")])
def test_every_runner_refuses_the_bad_combinations(rel, bad, said, capsys):
    parse = _parser(rel)
    with pytest.raises(SystemExit) as e:
        parse(BASE + bad)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert said in err and "Traceback" not in err
    assert len([line for line in err.splitlines() if "error:" in line]) == 1          # the parser's own one line


def test_the_checks_are_a_function_of_their_own_called_from_the_shared_parse():
    import inspect
    from tta import cli_args as C
    assert callable(C.check_apg_args) and "check_apg_args" in inspect.getsource(C.parse_with_step_cache)
    for name in ("add_apg_args", "apg_from_args", "apg_record", "apg_result"):
        assert callable(getattr(C, name))
    # wired in where the cfg-reuse trio is
    for rel in ("tta/runner_common.py", "baseline_experiment/scripts/run_baseline.py"):
        text = (PKG / rel).read_text()
        assert "add_apg_args" in text and "apg_result" in text and "apg_record" in text, rel
    assert "apg_from_args" in (PKG / "tta/runner_common.py").read_text()
    for rel in ("lora_experiment/scripts/run_lora_tta.py", "lora_experiment/scripts/run_full_tta.py"):
        assert "apg_record" in (PKG / rel).read_text(), rel
    sig = inspect.signature(__import__("tta.common", fromlist=["x"]).generate_video_continuation)
    assert sig.parameters["apg"].default is None


def test_nothing_is_imported_without_the_flag():
    import subprocess
    code = ("import sys; sys.path.insert(0, %r); from tta import cli_args as C; import argparse; p = argparse.ArgumentParser(); "
            "p.add_argument('--guidance-scale', type=float, default=4.0); C.add_step_cache_args(p); C.add_cfg_reuse_args(p); "
            "C.add_apg_args(p); a = C.parse_with_step_cache(p, []); assert C.apg_from_args(a) is None and C.apg_record(a) == {}; "
            "assert 'longcat_video.apg' not in sys.modules; "
            "a = C.parse_with_step_cache(p, ['--apg', '--apg-eta', '0.5']); assert C.apg_from_args(a).eta == 0.5; "
            "assert 'longcat_video.apg' in sys.modules" % str(PKG))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---------------------------------------------------------------------------------------------------------- the bookkeeping
class _FakeOps:
    """cfg_apg on CPU tensors in the header's words (float64 inside); it records every call."""

    def __init__(self):
        self.calls = []

    def cfg_apg(self, cond, uncond, diff, guidance, eta, radius, beta, zero_star, have_momentum, out=None, v=None):
        import torch
        assert not zero_star and v is cond and cond.is_contiguous() and uncond.is_contiguous()
        flat = lambda t: t.reshape(t.shape[0], -1).numpy()
        old = flat(diff).copy() if have_momentum and beta != 0 else None
        vv, d, s = A.apg_f64(flat(cond), flat(uncond), old, guidance, eta, radius, beta, False)
        c64 = flat(cond).astype(np.float64)
        out.copy_(torch.from_numpy(np.stack([(d * d).sum(1), (d * c64).sum(1), (c64 * c64).sum(1), s], axis=-1)).float())
        diff.copy_(torch.from_numpy(d).float().reshape(diff.shape))
        v.copy_(torch.from_numpy(vv).float().reshape(v.shape))
        self.calls.append({"have_momentum": bool(have_momentum), "radius": radius, "eta": eta, "beta": beta, "guidance": guidance})
        return v


def test_projected_guidance_on_a_fake_backend():
    import torch
    from longcat_video.apg import ProjectedGuidance
    fake = _FakeOps()
    g = ProjectedGuidance(eta=0.5, norm_threshold=0.25, momentum=-0.5, backend=fake)
    assert g.stats() == {"eta": 0.5, "norm_threshold": 0.25, "momentum": -0.5, "guided": 0, "clamp": [], "cosine": []}
    with pytest.raises(RuntimeError, match="begin"):
        g.guide(None, None, 4.0, False, 0)
    g.begin(1, 4)
    with pytest.raises(RuntimeError, match="outside"):
        g.guide(None, None, 4.0, False, 4)
    c0 = torch.tensor([[3.0, 0.0, 0.0, 0.0], [0.0, 2.0, 0.0, 0.0]]).reshape(2, 1, 2, 2)
    u0 = torch.tensor([[2.0, 0.0, 0.0, 0.0], [0.0, 2.0, -2.0, 0.0]]).reshape(2, 1, 2, 2)
    d = []
    for i in (1, 2, 3):
        c = c0.clone()
        v = g.guide(c, u0, 4.0, False, i)
        assert v is c                                                 # written over the model output
        d.append(g._diff.clone())
    # the radius is R sqrt(n) with n the elements per sample; the momentum is off at the first call only
    assert [k["radius"] for k in fake.calls] == [0.25 * math.sqrt(4)] * 3
    assert [k["have_momentum"] for k in fake.calls] == [False, True, True]
    assert all(k["eta"] == 0.5 and k["beta"] == -0.5 and k["guidance"] == 4.0 for k in fake.calls)
    raw = c0 - u0                                                     # row 0: (1, 0, 0, 0) along c; row 1: (0, 0, 2, 0) across c
    assert torch.equal(d[0], raw) and torch.equal(d[1], raw - 0.5 * d[0]) and torch.equal(d[2], raw - 0.5 * d[1])
    assert g._diff.shape == (2, 1, 2, 2) and g._trace.shape == (3, 2, 4) and g._trace.dtype == torch.float32
    s = g.stats()
    assert s["eta"] == 0.5 and s["norm_threshold"] == 0.25 and s["momentum"] == -0.5 and s["guided"] == 3
    # ||d|| per row and step: (1, 2), (0.5, 1), (0.75, 1.5) against the radius 0.5: the clamp is the smaller row's factor
    assert s["clamp"] == [0.25, 0.5, pytest.approx(1 / 3)]
    assert s["cosine"] == [1.0, 1.0, 1.0]                             # row 0 lies along c (row 1 across it: 0), the larger counts
    # a second denoise: the buffers stay, the statistics and the momentum do not
    diff, trace = g._diff, g._trace
    g.begin(0, 2)
    assert g.stats()["clamp"] == [None, None] and g.stats()["guided"] == 0
    g.guide(c0.clone(), u0, 4.0, False, 1)
    assert g._diff is diff and g._trace is trace
    assert fake.calls[-1]["have_momentum"] is False                   # cleared by begin()
    assert torch.equal(g._diff, raw)
    s = g.stats()
    assert s["guided"] == 1 and s["clamp"][0] is None and s["clamp"][1] == 0.25 and s["cosine"] == [None, 1.0]
    # a non-contiguous model output is copied, the copy is written and returned
    g.begin(0, 1)
    wide = torch.zeros(2, 1, 2, 4)
    wide[..., :2] = c0
    view = wide[..., :2]
    v = g.guide(view, u0, 4.0, False, 0)
    assert v is not view and v.is_contiguous() and torch.equal(wide[..., :2], c0)
    # another shape: new buffers, no momentum
    g.guide(torch.ones(1, 6), torch.zeros(1, 6), 4.0, False, 0)
    assert g._diff.shape == (1, 6) and g._trace.shape == (1, 1, 4) and fake.calls[-1]["have_momentum"] is False
    assert fake.calls[-1]["radius"] == 0.25 * math.sqrt(6)
    g.reset()
    assert g._diff is None and g._trace is None
    # no threshold: the radius handed down is 0
    fake2 = _FakeOps()
    g = ProjectedGuidance(backend=fake2)
    g.begin(0, 1)
    g.guide(c0.clone(), u0, 4.0, False, 0)
    assert fake2.calls[0]["radius"] == 0.0 and fake2.calls[0]["eta"] == 0.0 and g.stats()["clamp"] == [1.0]


def test_bad_settings_raise():
    from longcat_video.apg import ProjectedGuidance
    for eta in (math.nan, math.inf):
        with pytest.raises(ValueError, match="eta"):
            ProjectedGuidance(eta=eta)
    for thr in (0.0, -1.0, math.nan, math.inf):
        with pytest.raises(ValueError, match="threshold"):
            ProjectedGuidance(norm_threshold=thr)
    for beta in (1.0, -1.0, 2.0, math.nan):
        with pytest.raises(ValueError, match="momentum"):
            ProjectedGuidance(momentum=beta)
    g = ProjectedGuidance()
    with pytest.raises(ValueError, match="range"):
        g.begin(3, 2)


# ---------------------------------------------------------------------------------------------------------- the restatement
def test_the_restatement_by_hand():
    # g = 4 (gm1 = 3), no zero-star.  c = (2, 0), u = (1, -1): d = (1, 1); dd = 2, dc = 2, cc = 4; k = 0.5 (the 1e-8 is below
    # half an ulp of 4); p = (1, 0); o = (0, 1)
    c, u = np.float32([[2.0, 0.0]]), np.float32([[1.0, -1.0]])
    r = A.apg(c, u, None, 4.0, 0.0, 0.0, 0.0, False)
    assert r["diff"].tolist() == [[1.0, 1.0]] and r["out"].tolist() == [[2.0, 2.0, 4.0, 1.0]]
    assert r["v"].tolist() == [[2.0, 3.0]]                            # eta = 0: c + 3 o
    assert A.apg(c, u, None, 4.0, 1.0, 0.0, 0.0, False)["v"].tolist() == [[5.0, 3.0]]      # eta = 1: c + 3 d, the plain rule
    assert A.plain_f32(c, u, 4.0, False).tolist() == [[5.0, 3.0]]
    assert A.apg(c, u, None, 4.0, 0.5, 0.0, 0.0, False)["v"].tolist() == [[3.5, 3.0]]
    # a momentum: d = (1, 1) - 0.5 (2, -2) = (0, 2); without an old correction beta does nothing
    r = A.apg(c, u, np.float32([[2.0, -2.0]]), 4.0, 0.0, 0.0, -0.5, False)
    assert r["diff"].tolist() == [[0.0, 2.0]] and r["out"].tolist() == [[4.0, 0.0, 4.0, 1.0]] and r["v"].tolist() == [[2.0, 6.0]]
    assert A.apg(c, u, None, 4.0, 0.0, 0.0, -0.5, False)["diff"].tolist() == [[1.0, 1.0]]
    # a radius: d = (0, 2) has norm 2; radius 1 halves it, radius 2 and 3 do not clamp
    old = np.float32([[2.0, -2.0]])
    assert A.apg(c, u, old, 4.0, 0.0, 1.0, -0.5, False)["out"][0, 3] == 0.5
    assert A.apg(c, u, old, 4.0, 0.0, 1.0, -0.5, False)["v"].tolist() == [[2.0, 3.0]]
    assert A.apg(c, u, old, 4.0, 0.0, 2.0, -0.5, False)["out"][0, 3] == 1.0
    assert A.apg(c, u, old, 4.0, 0.0, 3.0, -0.5, False)["out"][0, 3] == 1.0
    # a zero correction: s = 1, v = c
    r = A.apg(c, c, None, 4.0, 0.0, 1.0, 0.0, False)
    assert r["out"].tolist() == [[0.0, 0.0, 4.0, 1.0]] and r["v"].tolist() == c.tolist()
    # zero-star: st = <c, u> / <u, u> = 2 / 2 = 1 here; with u = (4, 0): st = 8 / 16 = 0.5, u' = (2, 0), d = 0
    assert A.apg(c, u, None, 4.0, 0.0, 0.0, 0.0, True)["st"].tolist() == [1.0]
    r = A.apg(c, np.float32([[4.0, 0.0]]), None, 4.0, 0.0, 0.0, 0.0, True)
    assert r["st"].tolist() == [0.5] and r["diff"].tolist() == [[0.0, 0.0]]
    # the partials: every slot written, empty slices 0, slot 3 0
    e = np.ones((2, 300), np.float32); e[1] = 2.0
    ws = A.sum_partials(e, 3.0 * e)
    assert ws.shape == (2, 256, 4) and ws[0, 0].tolist() == [256.0, 768.0, 2304.0, 0.0] and ws[0, 1].tolist() == [44.0, 132.0, 396.0, 0.0]
    assert ws[1, 1].tolist() == [176.0, 528.0, 1584.0, 0.0] and not ws[:, 2:].any()
    assert [x.tolist() for x in A.sum_join(ws)] == [[300.0, 1200.0], [900.0, 3600.0], [2700.0, 10800.0]]
    w0 = A.star_partials(e, 3.0 * e)
    assert w0.shape == (2, 256, 4) and w0[0, 0].tolist() == [768.0, 2304.0, 0.0, 0.0] and not w0[..., 2:].any()


@pytest.mark.parametrize("zero_star", [False, True])
@pytest.mark.parametrize("n", [257, 12288, 65537])
def test_eta_zero_leaves_a_correction_orthogonal_to_cond(n, zero_star):
    """eta = 0: v - c = (g - 1)(s d - p) with p the part of s d along c.  In fp32 <d, c> and <c, c> are fixed-order sums of n
    rounded products: each is off by at most n EPS times the sum of its terms' magnitudes, that is n EPS ||d|| ||c|| and
    n EPS ||c||^2, so the coefficient leaves at most 2 n EPS ||d|| / ||c|| of c in the result; the element operations add at most
    8 EPS per element.  Against the orthogonal part's norm: |cos(v - c, c)| <= (2 n + 8) EPS ||d|| / ||d_orth||, and on these
    inputs ||d|| <= 2 ||d_orth|| (asserted in float64)."""
    c, u, _ = _identity_inputs(n)
    for radius in (0.0, 0.25 * math.sqrt(n)):
        r = A.apg(c, u, None, GUIDANCE, 0.0, radius, 0.0, zero_star)
        w = r["v"].astype(np.float64) - c.astype(np.float64)
        c64 = c.astype(np.float64)
        cos = (w * c64).sum(1) / np.sqrt((w * w).sum(1) * (c64 * c64).sum(1))
        _, d64, _ = A.apg_f64(c, u, None, GUIDANCE, 0.0, radius, 0.0, zero_star)
        orth = d64 - ((d64 * c64).sum(1) / (c64 * c64).sum(1))[:, None] * c64
        ratio = np.sqrt((d64 * d64).sum(1) / (orth * orth).sum(1))
        assert (ratio <= 2.0).all(), ratio
        print(f"n {n} zero-star {zero_star} radius {radius:.3g}: |cos| {np.abs(cos).max():.3e} bound {(2 * n + 8) * EPS * 2:.3e}")
        assert (np.abs(cos) <= (2 * n + 8) * EPS * 2.0).all()
        # and the value against the float64 form: the coefficient's 2 n EPS and 8 EPS per element, times g - 1, of max |c|, |d|
        v64, _, _ = A.apg_f64(c, u, None, GUIDANCE, 0.0, radius, 0.0, zero_star)
        st_err = 2 * n * EPS if zero_star else 0.0                    # st is a quotient of two such sums
        assert rel_distance(r["v"], v64) <= (2 * n + 8) * EPS * (GUIDANCE - 1.0) + st_err * GUIDANCE


@pytest.mark.parametrize("zero_star", [False, True])
@pytest.mark.parametrize("n", [257, 12288, 65537])
def test_a_threshold_caps_the_norm(n, zero_star):
    """||s d|| <= radius (1 + 2^-22), the norm in float64 over the restatement's fp32 s * d."""
    c, u, _ = _identity_inputs(n)
    c64 = c.astype(np.float64)
    for R, clamps in ((0.25, True), (4.0, False)):
        radius = float(np.float32(R * math.sqrt(n)))
        r = A.apg(c, u, None, GUIDANCE, 0.5, radius, 0.0, zero_star)
        s = r["out"][:, 3]
        ds = (s[:, None] * r["diff"]).astype(np.float32).astype(np.float64)
        norm = np.sqrt((ds * ds).sum(1))
        print(f"n {n} zero-star {zero_star} R {R}: s {s} norm / radius {norm / radius}")
        assert (norm <= radius * (1 + 2.0 ** -22)).all()
        assert ((s < 1) if clamps else (s == 1)).all()
        if clamps:
            assert (norm >= radius * (1 - 2.0 ** -22)).all()          # capped at the radius, not below it
        else:
            _report_equal(r["v"], A.apg(c, u, None, GUIDANCE, 0.5, 0.0, 0.0, zero_star)["v"])      # no clamp: no threshold
        assert np.allclose(s, A.apg_f64(c, u, None, GUIDANCE, 0.5, radius, 0.0, zero_star)[2], rtol=(n + 4) * EPS, atol=0)
        assert (c64 == c).all()


def _report_equal(a, b):
    assert np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def test_the_momentum_over_three_calls():
    """d_t = (c_t - u_t) + beta * d_{t-1} with d_{-1} absent: three calls of the restatement against the float64 recurrence.
    Each call makes three rounded operations per element (the difference, the product, the sum), each off by at most EPS of its
    result, all of magnitude at most M = max |d| over the calls (|beta| < 1): 9 EPS M after three calls."""
    n, beta = 4099, -0.5
    rng = np.random.default_rng(5)
    old32 = old64 = None
    worst = 0.0
    for t in range(3):
        c = rng.standard_normal((2, n)).astype(np.float32)
        u = (0.5 * c + 0.5 * rng.standard_normal((2, n))).astype(np.float32)
        r = A.apg(c, u, old32, GUIDANCE, 0.0, 0.0, beta, False)
        raw = c.astype(np.float64) - u.astype(np.float64)
        d64 = raw if old64 is None else raw + beta * old64
        assert np.array_equal(A.apg_f64(c, u, old64, GUIDANCE, 0.0, 0.0, beta, False)[1], d64)
        if t == 0:
            _report_equal(r["diff"], A.correction(c, u))              # the first call: no momentum term at all
        else:
            assert not np.array_equal(r["diff"], A.correction(c, u))
        worst = max(worst, float(np.abs(d64).max()))
        assert np.abs(r["diff"] - d64).max() <= 9 * EPS * worst
        old32, old64 = r["diff"], d64


@pytest.mark.parametrize("zero_star", [False, True])
@pytest.mark.parametrize("n", [12288, 65537])
def test_eta_one_is_the_plain_rule_in_value(n, zero_star):
    c, u, _ = _identity_inputs(n)
    ref = A.plain_f64(c, u, GUIDANCE, zero_star)
    plain = rel_distance(A.plain_f32(c, u, GUIDANCE, zero_star), ref)
    r = A.apg(c, u, None, GUIDANCE, 1.0, 0.0, 0.0, zero_star)
    apg = rel_distance(r["v"], ref)
    print(f"n {n} zero-star {zero_star}: plain fp32 restatement {plain:.3e}, APG fp32 restatement {apg:.3e}, tolerance {IDENTITY_TOL:.3e}")
    assert plain <= 1.5 * PLAIN_F32_DISTANCE
    assert apg <= IDENTITY_TOL
    assert (r["out"][:, 3] == 1).all()
    # the plain fp32 rule is cfgreuse_ref's: its delta is this v minus c, to the bit
    _report_equal((A.plain_f32(c, u, GUIDANCE, zero_star) - c).astype(np.float32), A.G.delta_store(c, u, GUIDANCE, st=r["st"]))


# ---------------------------------------------------------------------------------------------------------- the ABI
def test_header_and_binding_agree():
    """The header's entry point is exported, bound with the header's argument count, and the version went up."""
    import ctypes
    import re
    from lcv_hip import build, lib
    header = (ROOT / "include" / "lcv_hip_apg.h").read_text()
    protos = {m.group(1): m.group(2) for m in re.finditer(r"^int (lcv_\w+)\(([^;]*)\);", header, re.M | re.S)}
    assert set(protos) == set(lib._SIGNATURES_APG) == {"lcv_cfg_apg"}
    assert len(protos["lcv_cfg_apg"].split(",")) == len(lib._SIGNATURES_APG["lcv_cfg_apg"]) == 15
    assert lib._SIGNATURES_APG["lcv_cfg_apg"] == [lib.P] * 6 + [lib.I64] * 2 + [lib.F32] * 4 + [lib.I] * 2 + [lib.P]
    so = ctypes.CDLL(str(lib.lib_path()))
    so.lcv_version.restype = ctypes.c_int
    assert so.lcv_version() >= 14
    assert hasattr(so, "lcv_cfg_apg")
    for other in sorted((ROOT / "include").glob("*.h")):              # a header of its own
        if other.name != "lcv_hip_apg.h":
            assert "lcv_cfg_apg" not in other.read_text(), other.name
    loaded = lib.load()
    assert loaded.lcv_cfg_apg.argtypes == lib._SIGNATURES_APG["lcv_cfg_apg"] and loaded.lcv_cfg_apg.restype is ctypes.c_int
    # built without contraction, on the shared guidance header, with no atomics and no allocation
    assert build.EXTRA["cfg_apg.hip"] == ["-ffp-contract=off"] == build.EXTRA["cfg_reuse.hip"]
    src = (PKG / "csrc" / "cfg_apg.hip").read_text()
    assert '#include "cfg_guidance.h"' in src and "cfg_partial_sums<" in src and "cfg_star_scale<" in src
    for word in ("atomicAdd", "__hip_atomic", "fmaf", "asm", "hipMalloc", "getenv"):
        assert word not in src, word

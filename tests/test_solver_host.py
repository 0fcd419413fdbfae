"""Host side of the second-order multistep solvers of the denoise loop (`--solver`, longcat_video/solver.py,
include/lcv_hip_solver.h): the weights on the scheduler's own grid, the convergence order of the numpy restatement
(tests/solver_ref.py), and the flag on every runner's parser.  No GPU."""
import importlib.util
import math
import sys
from pathlib import Path

import numpy as np
import pytest

import solver_ref as S

ROOT = Path(__file__).resolve().parents[1]
PKG = ROOT / "longcat-video-tta_amd"
RUNNERS = ["delta_experiment/scripts/run_delta_a.py", "delta_experiment/scripts/run_delta_b.py",
           "delta_experiment/scripts/run_delta_c.py", "delta_experiment/scripts/run_film_tta.py",
           "delta_experiment/scripts/run_norm_tune_tta.py", "lora_experiment/scripts/run_full_tta.py",
           "lora_experiment/scripts/run_lora_tta.py", "baseline_experiment/scripts/run_baseline.py"]
BASE = ["--checkpoint-dir", "synthetic", "--data-dir", "synthetic:1", "--output-dir", "unused"]
EPS = 2.0 ** -52
KINDS = ("euler", "ab2", "ab2c")
_GRIDS = {}


def _grid(n_steps, shift):
    """`_sigmas_host` of the scheduler as the pipeline sets it: linspace(1, 0.001, N), the shift warp, the trailing 0."""
    key = (n_steps, shift)
    if key not in _GRIDS:
        from longcat_video.modules.scheduling_flow_match_euler_discrete import FlowMatchEulerDiscreteScheduler
        from longcat_video.pipeline_longcat_video import LongCatVideoPipeline
        sched = FlowMatchEulerDiscreteScheduler(shift=shift)
        sched.set_timesteps(n_steps, sigmas=LongCatVideoPipeline.get_timesteps_sigmas(n_steps))
        sig = list(sched._sigmas_host)
        assert len(sig) == n_steps + 1 and sig[0] == 1.0 and sig[-1] == 0.0 and all(a > b for a, b in zip(sig, sig[1:]))
        _GRIDS[key] = sig
    return _GRIDS[key]


# ---------------------------------------------------------------------------------------------------------- the weights
@pytest.mark.parametrize("shift", [1.0, 3.0])
@pytest.mark.parametrize("n_steps", [2, 3, 4, 50])
def test_weights_on_the_schedulers_grid(n_steps, shift):
    from longcat_video.solver import solver_weights
    sig = _grid(n_steps, shift)
    for start in (0, 1) if n_steps > 2 else (0,):
        for i in range(start, n_steps):                               # the last interval, 0.001 ... -> 0, included
            h = sig[i + 1] - sig[i]
            for kind in KINDS:
                w = solver_weights(sig, i, start, kind)
                assert all(isinstance(v, float) for v in w)
                assert w == tuple(S.weights(sig, i, start, kind)), (kind, i)        # the restatement, to the bit
                # they sum to h_i: each weight is a handful of float64 operations on values of the size of the largest weight
                assert abs(math.fsum(w) - h) <= 8 * EPS * max(abs(v) for v in w), (kind, i, w)
                if kind == "euler" or i == start:
                    assert w == (h,)                                  # j = 0 is Euler's step under every rule
                elif kind == "ab2":
                    assert len(w) == 2
                    # exact on polynomials of degree <= 1 in sigma: the integrals of 1 and of sigma over [sigma_i, sigma_i+1]
                    scale = abs(w[0]) + abs(w[1])
                    assert abs(w[0] + w[1] - h) <= 8 * EPS * scale
                    want = (sig[i + 1] ** 2 - sig[i] ** 2) / 2
                    assert abs(w[0] * sig[i] + w[1] * sig[i - 1] - want) <= 8 * EPS * scale
                else:
                    assert len(w) == (2 if i == start + 1 else 3)     # at j = 1 the third weight is zero and is not passed


def test_weights_on_a_uniform_grid():
    from longcat_video.solver import solver_weights
    sig = [1.0, 0.75, 0.5, 0.25, 0.0]                                 # h = -1/4, every value exact
    h = -0.25
    assert solver_weights(sig, 0, 0, "ab2") == solver_weights(sig, 0, 0, "ab2c") == solver_weights(sig, 0, 0, "euler") == (h,)
    for i in (1, 2, 3):
        assert solver_weights(sig, i, 0, "euler") == (h,)
        assert solver_weights(sig, i, 0, "ab2") == (1.5 * h, -0.5 * h)
    assert solver_weights(sig, 1, 0, "ab2c") == (2 * h, -h)           # j = 1: 3h/2 + h/2 and -h/2 + h/2 - h
    for i in (2, 3):
        assert solver_weights(sig, i, 0, "ab2c") == (2 * h, -1.5 * h, 0.5 * h)
    assert solver_weights(sig, 2, 2, "ab2c") == (h,) and solver_weights(sig, 3, 2, "ab2c") == (2 * h, -h)     # a later start
    with pytest.raises(ValueError):
        solver_weights(sig, 1, 0, "ab3")
    with pytest.raises(ValueError):
        solver_weights(sig, 4, 0, "ab2")                              # no interval 4
    with pytest.raises(ValueError):
        solver_weights(sig, 0, 1, "ab2")                              # before the start


def test_restated_step_by_hand():
    x, f = S.lms_step([[1.0, 2.0]], [[0.5, 1.0]], [[10.0, 10.0]], ([[1.0, 1.0]], [[2.0, 2.0]]), 4.0, (0.5, 0.25, 2.0), True,
                      st=np.float32([2.0]))
    # u = (1, 2); d = 0; v = u; f = -u; a = -0.5 u + 0.25 + 4
    assert f.tolist() == [[-1.0, -2.0]] and x.tolist() == [[13.75, 13.25]]
    x, f = S.lms_step([[1.0, 2.0]], None, [[10.0, 10.0]], (), 4.0, (0.5,), False)
    assert f.tolist() == [[1.0, 2.0]] and x.tolist() == [[10.5, 11.0]]
    x, f = S.lms_step([[3.0]], [[1.0]], [[0.0]], ([[8.0]],), 2.0, (1.0, -1.0), False)     # no zero-star: v = 1 + 2 (3 - 1) = 5
    assert f.tolist() == [[5.0]] and x.tolist() == [[-3.0]]


def test_restated_sums_by_hand():
    c = np.arange(1, 601, dtype=np.float32).reshape(2, 300)
    u = np.ones((2, 300), np.float32); u[1] = 2.0
    ws = S.partials(c, u)
    assert ws.shape == (2, 256, 2)
    assert ws[0, 0].tolist() == [sum(range(1, 257)), 256.0] and ws[0, 1].tolist() == [sum(range(257, 301)), 44.0]
    assert not ws[:, 2:].any()                                        # empty slices hold zeros
    st = S.join(ws)
    assert st.tolist() == [np.float32(45150.0) / (np.float32(300.0) + np.float32(1e-8)),
                           np.float32(2 * sum(range(301, 601))) / (np.float32(1200.0) + np.float32(1e-8))]
    assert np.allclose(st, S.st_f64(c, u), rtol=1e-6)


# ---------------------------------------------------------------------------------------------------------- the order
X0 = np.float32([1.0, -0.7, 3.0])
_ERR = {}


def _err(kind, n_steps, shift):
    """Relative L2 error at sigma = 0 of dx/dsigma = x from x(1) = X0, fp32 state, against X0 / e."""
    key = (kind, n_steps, shift)
    if key not in _ERR:
        got = S.integrate(kind, _grid(n_steps, shift), X0, lambda x, s: x).astype(np.float64)
        want = X0.astype(np.float64) * math.exp(-1.0)
        _ERR[key] = float(np.linalg.norm(got - want) / np.linalg.norm(want))
    return _ERR[key]


@pytest.mark.parametrize("shift", [1.0, 3.0])
def test_convergence_order_of_the_restatement(shift):
    """Halving the step halves a first-order method's error and quarters a second-order one's: the bounds 2.5 and 3.5 sit
    between 2^1 and 2^2."""
    for kind in KINDS:
        print(shift, kind, [f"{_err(kind, n, shift):.2e}" for n in (8, 16, 32, 64)],
              f"ratio {_err(kind, 16, shift) / _err(kind, 32, shift):.2f}")
    assert _err("euler", 16, shift) / _err("euler", 32, shift) < 2.5
    for kind in ("ab2", "ab2c"):
        assert _err(kind, 16, shift) / _err(kind, 32, shift) > 3.5, kind
    assert _err("ab2", 16, shift) < _err("euler", 64, shift)
    for n in (8, 16):
        assert _err("ab2c", n, shift) < _err("ab2", n, shift), n


def test_a_split_denoise_restarts_the_history():
    sig = _grid(8, 1.0)
    whole = S.integrate("ab2", sig, X0, lambda x, s: x)
    half = S.integrate("ab2", sig, X0, lambda x, s: x, stop=4)
    split = S.integrate("ab2", sig, half, lambda x, s: x, start=4)
    assert not np.array_equal(whole, split)                           # step 4 of the second call is an Euler step
    assert np.array_equal(S.integrate("euler", sig, S.integrate("euler", sig, X0, lambda x, s: x, stop=4), lambda x, s: x, start=4),
                          S.integrate("euler", sig, X0, lambda x, s: x))


def test_multistep_solver_refuses_what_it_cannot_do():
    from longcat_video.solver import MultistepSolver
    with pytest.raises(ValueError):
        MultistepSolver("euler")                                      # Euler has no history: the pipeline keeps its own path
    with pytest.raises(ValueError):
        MultistepSolver("ab3")
    s = MultistepSolver("ab2c")
    with pytest.raises(RuntimeError, match="begin"):
        s.step(None, None, None, 0, [1.0, 0.0], 1.0, True, True)
    s.begin(2)
    with pytest.raises(RuntimeError, match="consecutive"):
        s.step(None, None, None, 3, [1.0, 0.5, 0.25, 0.1, 0.0], 1.0, True, True)


# ---------------------------------------------------------------------------------------------------------- the parsers
def _parser(rel):
    path = PKG / rel
    sys.path.insert(0, str(path.parent))
    try:
        spec = importlib.util.spec_from_file_location("solver_parser_" + path.stem, path)
        m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    finally:
        sys.path.remove(str(path.parent))
    return m.parse_args if hasattr(m, "parse_args") else m.build_parser().parse_args


@pytest.mark.parametrize("rel", RUNNERS)
def test_every_runner_takes_the_flag(rel):
    from tta import cli_args as C
    parse = _parser(rel)
    for kind in ("ab2", "ab2c"):
        a = parse(BASE + ["--solver", kind])
        assert a.solver == kind and C.solver_record(a) == {"solver": kind} and C.solver_from_args(a) == kind
    for argv in (BASE, BASE + ["--solver", "euler"]):
        a = parse(argv)
        assert a.solver == "euler" and C.solver_record(a) == {} and C.solver_from_args(a) is None


@pytest.mark.parametrize("rel", RUNNERS)
def test_every_runner_refuses_an_unknown_solver(rel, capsys):
    parse = _parser(rel)
    with pytest.raises(SystemExit) as e:
        parse(BASE + ["--solver", "ab3"])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "--solver" in err and "invalid choice" in err and "Traceback" not in err


def test_header_and_binding_agree():
    """The header's one entry point is exported, bound with the header's argument count, and the version went up."""
    import ctypes
    import re
    from lcv_hip import lib
    header = (ROOT / "include" / "lcv_hip_solver.h").read_text()
    protos = {m.group(1): m.group(2) for m in re.finditer(r"^int (lcv_\w+)\(([^;]*)\);", header, re.M | re.S)}
    assert set(protos) == set(lib._SIGNATURES_SOLVER) == {"lcv_cfg_lms_step"}
    assert len(protos["lcv_cfg_lms_step"].split(",")) == len(lib._SIGNATURES_SOLVER["lcv_cfg_lms_step"]) == 17
    so = ctypes.CDLL(str(lib.lib_path()))
    so.lcv_version.restype = ctypes.c_int
    assert so.lcv_version() >= 11
    assert hasattr(so, "lcv_cfg_lms_step")
    for other in ("lcv_hip.h", "lcv_hip_stepcache.h"):                # a header of its own: the others' lists are unchanged
        assert "lcv_cfg_lms_step" not in (ROOT / "include" / other).read_text()

"""Host side of the guidance reuse of the CFG denoise loop (`--cfg-reuse`, longcat_video/cfg_reuse.py,
include/lcv_hip_cfgreuse.h): the schedule by hand, the bookkeeping of `GuidanceReuse` on a fake backend, the flags on every
runner's parser with their refusals and records, and the header against the binding.  No GPU."""
import importlib.util
import math
import sys
from pathlib import Path

import numpy as np
import pytest

import cfgreuse_ref as G

ROOT = Path(__file__).resolve().parents[1]
PKG = ROOT / "longcat-video-tta_amd"
RUNNERS = ["delta_experiment/scripts/run_delta_a.py", "delta_experiment/scripts/run_delta_b.py",
           "delta_experiment/scripts/run_delta_c.py", "delta_experiment/scripts/run_film_tta.py",
           "delta_experiment/scripts/run_norm_tune_tta.py", "lora_experiment/scripts/run_full_tta.py",
           "lora_experiment/scripts/run_lora_tta.py", "baseline_experiment/scripts/run_baseline.py"]
BASE = ["--checkpoint-dir", "synthetic", "--data-dir", "synthetic:1", "--output-dir", "unused"]


# ---------------------------------------------------------------------------------------------------------- the schedule
def test_the_schedule_by_hand():
    from longcat_video.cfg_reuse import full_steps
    assert full_steps(0, 10, 1) == list(range(10))                    # K = 1: every step is full
    assert full_steps(0, 10, 3) == [0, 3, 6, 9]
    assert full_steps(0, 8, 3) == [0, 3, 6, 7]                        # the last step is forced
    assert full_steps(0, 10, 3, 2) == [0, 1, 3, 6, 9]                 # the warm-up
    assert full_steps(0, 10, 4, 3) == [0, 1, 2, 4, 8, 9]
    assert full_steps(2, 10, 3) == [2, 5, 8, 9]                       # j counts from the start step
    assert full_steps(4, 9, 2, 1) == [4, 6, 8]
    assert full_steps(0, 1, 5) == [0] and full_steps(0, 2, 5) == [0, 1] and full_steps(3, 3, 2) == []
    assert full_steps(0, 50, 100) == [0, 49]                          # an interval past the end: the first and the last
    for start, stop, K, W in ((0, 10, 3, 0), (2, 10, 3, 1), (0, 50, 5, 4), (7, 8, 2, 0), (1, 30, 7, 9)):
        assert full_steps(start, stop, K, W) == G.full_steps(start, stop, K, W)


def test_is_full_follows_the_schedule():
    from longcat_video.cfg_reuse import GuidanceReuse, full_steps
    for start, stop, K, W in ((0, 10, 3, 0), (2, 10, 3, 2), (0, 8, 3, 0), (0, 6, 1, 0)):
        r = GuidanceReuse(K, W)
        r.begin(start, stop)
        assert [i for i in range(start, stop) if r.is_full(i)] == full_steps(start, stop, K, W)


# ---------------------------------------------------------------------------------------------------------- the bookkeeping
class _FakeOps:
    """The two ops on CPU tensors, in the header's words; it records every call."""

    def __init__(self):
        self.calls = []

    def cfg_delta_store(self, cond, uncond, delta, guidance, zero_star=True, out=None):
        import torch
        assert not zero_star
        v = uncond + guidance * (cond - uncond)
        e = v - cond
        if out is not None:
            flat = lambda t: t.reshape(t.shape[0], -1)
            out.copy_(torch.stack([flat((e - delta).abs()).sum(1), flat(delta.abs()).sum(1)], dim=1))
        delta.copy_(e)
        self.calls.append(("store", out is not None))

    def cfg_delta_apply(self, cond, delta, out=None):
        out = cond.clone() if out is None else out
        out.copy_(cond + delta)
        self.calls.append(("apply", out is cond))
        return out


def test_stats_on_a_fake_backend():
    import torch
    from longcat_video.cfg_reuse import GuidanceReuse
    fake = _FakeOps()
    r = GuidanceReuse(3, backend=fake)
    assert r.stats() == {"interval": 3, "warmup": 0, "full": 0, "reused": 0, "reused_steps": [], "distances": []}
    r.begin(0, 8)
    c = torch.full((2, 4), 3.0)
    for i in range(8):
        # u = c - D with D = i + 1 on row 0 and 2 (i + 1) on row 1: delta = 3 D, exact
        D = torch.tensor([[1.0], [2.0]]) * (i + 1)
        if r.is_full(i):
            r.store(c, c - D, 4.0, False, i)
        else:
            v = r.apply(c.clone())
            assert torch.equal(v, c + r._delta)
    s = r.stats()
    assert s["interval"] == 3 and s["warmup"] == 0 and s["full"] == 4 and s["reused"] == 4
    assert s["reused_steps"] == [1, 2, 4, 5]
    # full steps 0, 3, 6, 7: delta goes 3 D_0 -> 3 D_3 -> 3 D_6 -> 3 D_7 with D_i = i + 1; both rows give the same ratio
    assert s["distances"] == [None, None, None, 3.0, None, None, (7 - 4) / 4, (8 - 7) / 7]
    assert fake.calls == [("store", False), ("apply", True), ("apply", True), ("store", True), ("apply", True), ("apply", True),
                          ("store", True), ("store", True)]
    assert r._delta.shape == (2, 4) and r._trace.shape == (8, 2, 2)
    # a second denoise: the buffers stay, the statistics and the correction do not
    delta, trace = r._delta, r._trace
    r.begin(2, 6)
    with pytest.raises(RuntimeError, match="full step"):
        r.apply(c.clone())
    r.store(c, c - 1.0, 4.0, False, 2)
    assert r._delta is delta and r._trace is trace
    assert r.stats() == {"interval": 3, "warmup": 0, "full": 1, "reused": 0, "reused_steps": [], "distances": [None] * 4}
    r.apply(c.clone())
    assert r.stats()["reused_steps"] == [3]
    r.reset()
    assert r._delta is None and r._trace is None


def test_a_zero_denominator_is_an_infinite_distance():
    import torch
    from longcat_video.cfg_reuse import GuidanceReuse
    r = GuidanceReuse(1, backend=_FakeOps())
    r.begin(0, 3)
    c = torch.ones(1, 4)
    r.store(c, c, 4.0, False, 0)                                      # delta = 0
    r.store(c, c - 1.0, 4.0, False, 1)                                # |3 - 0| / |0|
    r.store(c, c - 1.0, 4.0, False, 2)
    assert r.stats()["distances"] == [None, math.inf, 0.0]
    assert G.distance([[1.0, 0.0]]) == math.inf and G.distance([[1.0, 2.0], [3.0, 4.0]]) == 0.75


def test_bad_arguments_raise():
    from longcat_video.cfg_reuse import GuidanceReuse, full_steps
    for K in (0, -1, 1.5):
        with pytest.raises(ValueError, match="interval"):
            GuidanceReuse(K)
        with pytest.raises(ValueError, match="interval"):
            full_steps(0, 4, K)
    for W in (-1, 0.5):
        with pytest.raises(ValueError, match="warm-up"):
            GuidanceReuse(2, warmup=W)
        with pytest.raises(ValueError, match="warm-up"):
            full_steps(0, 4, 2, W)
    r = GuidanceReuse(2, backend=_FakeOps())
    with pytest.raises(RuntimeError, match="begin"):
        r.is_full(0)
    with pytest.raises(RuntimeError, match="begin"):
        r.store(None, None, 4.0, False, 0)
    r.begin(0, 4)
    with pytest.raises(RuntimeError, match="full step"):
        r.apply(np.zeros((1, 2), np.float32))                         # an apply before any store
    with pytest.raises(RuntimeError, match="outside"):
        r.store(None, None, 4.0, False, 4)


def test_the_restatement_by_hand():
    # g = 4, no zero-star: e = 3 (c - u) on integers
    assert G.delta_store([[1.0, 2.0, -1.0]], [[0.0, 3.0, -1.0]], 4.0).tolist() == [[3.0, -3.0, 0.0]]
    # st = 2: u' = (2, 4); d = (-1, -2); v = (-2, -4); e = (-3, -6)
    assert G.delta_store([[1.0, 2.0]], [[1.0, 2.0]], 4.0, st=np.float32([2.0])).tolist() == [[-3.0, -6.0]]
    assert G.delta_apply([[1.0, 2.0]], [[0.5, -2.0]]).tolist() == [[1.5, 0.0]]
    e = np.arange(1, 601, dtype=np.float32).reshape(2, 300)
    o = np.ones((2, 300), np.float32); o[1] = -2.0
    ws = G.drift_partials(e, o)
    assert ws.shape == (2, 256, 2)
    assert ws[0, 0].tolist() == [sum(range(0, 256)), 256.0] and ws[0, 1].tolist() == [sum(range(256, 300)), 44.0]
    assert ws[1, 1].tolist() == [sum(range(559, 603)), 88.0]
    assert not ws[:, 2:].any()                                        # empty slices hold zeros
    assert G.drift_join(ws).tolist() == [[sum(range(0, 300)), 300.0], [sum(range(303, 603)), 600.0]]


# ---------------------------------------------------------------------------------------------------------- the parsers
def _parser(rel):
    path = PKG / rel
    sys.path.insert(0, str(path.parent))
    try:
        spec = importlib.util.spec_from_file_location("cgr_parser_" + path.stem, path)
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
    from longcat_video.cfg_reuse import GuidanceReuse
    parse = _parser(rel)
    a = parse(BASE + ["--cfg-reuse", "3", "--cfg-reuse-warmup", "2"])
    assert a.cfg_reuse == 3 and a.cfg_reuse_warmup == 2
    assert C.cfg_reuse_record(a) == {"cfg_reuse": 3, "cfg_reuse_warmup": 2}
    r = C.cfg_reuse_from_args(a)
    assert isinstance(r, GuidanceReuse) and r.interval == 3 and r.warmup == 2
    assert C.cfg_reuse_from_args(a) is not r                          # one per continuation
    a = parse(BASE + ["--cfg-reuse", "1"])
    assert a.cfg_reuse == 1 and C.cfg_reuse_record(a) == {"cfg_reuse": 1, "cfg_reuse_warmup": 0}
    assert C.cfg_reuse_from_args(a).warmup == 0
    a = parse(BASE + ["--cfg-reuse", "2", "--solver", "ab2c", "--guidance-scale", "1.5"])     # composes with the solver
    assert a.cfg_reuse == 2 and a.solver == "ab2c"
    a = parse(BASE)
    assert a.cfg_reuse is None and a.cfg_reuse_warmup is None
    assert C.cfg_reuse_record(a) == {} and C.cfg_reuse_from_args(a) is None and C.cfg_reuse_result({}) == {}
    assert C.cfg_reuse_result({"_cfg_reuse": {"full": 2}}) == {"cfg_reuse": {"full": 2}}


@pytest.mark.parametrize("rel", RUNNERS)
@pytest.mark.parametrize("bad,said", [(["--cfg-reuse", "0"], "K must be >= 1"),
                                      (["--cfg-reuse", "-2"], "K must be >= 1"),
                                      (["--cfg-reuse", "2", "--cfg-reuse-warmup", "-1"], "W must be >= 0"),
                                      (["--cfg-reuse-warmup", "2"], "needs --cfg-reuse"),
                                      (["--cfg-reuse", "2", "--step-cache", "0.1"], "cannot be combined with --step-cache"),
                                      (["--cfg-reuse", "2", "--guidance-scale", "1.0"], "--guidance-scale must be > 1"),
                                      (["--cfg-reuse", "2", "--guidance-scale", "0.5"], "--guidance-scale must be > 1")])
def test_every_runner_refuses_the_bad_combinations(rel, bad, said, capsys):
    parse = _parser(rel)
    with pytest.raises(SystemExit) as e:
        parse(BASE + bad)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert said in err and "Traceback" not in err


def test_the_checks_are_a_function_of_their_own_called_from_the_shared_parse():
    import inspect
    from tta import cli_args as C
    assert callable(C.check_cfg_reuse_args) and "check_cfg_reuse_args" in inspect.getsource(C.parse_with_step_cache)
    for rel in RUNNERS:
        assert "parse_with_step_cache" in (PKG / rel).read_text(), rel


def test_nothing_is_imported_without_the_flag():
    import subprocess
    code = ("import sys; sys.path.insert(0, %r); from tta import cli_args as C; import argparse; p = argparse.ArgumentParser(); "
            "p.add_argument('--guidance-scale', type=float, default=4.0); C.add_step_cache_args(p); C.add_cfg_reuse_args(p); "
            "a = C.parse_with_step_cache(p, []); assert C.cfg_reuse_from_args(a) is None and C.cfg_reuse_record(a) == {}; "
            "assert 'longcat_video.cfg_reuse' not in sys.modules; "
            "a = C.parse_with_step_cache(p, ['--cfg-reuse', '2']); assert C.cfg_reuse_from_args(a).interval == 2; "
            "assert 'longcat_video.cfg_reuse' in sys.modules" % str(PKG))
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ---------------------------------------------------------------------------------------------------------- the ABI
def test_header_and_binding_agree():
    """The header's entry points are exported, bound with the header's argument counts, and the version went up."""
    import ctypes
    import re
    from lcv_hip import lib
    header = (ROOT / "include" / "lcv_hip_cfgreuse.h").read_text()
    protos = {m.group(1): m.group(2) for m in re.finditer(r"^int (lcv_\w+)\(([^;]*)\);", header, re.M | re.S)}
    assert set(protos) == set(lib._SIGNATURES_CFGREUSE) == {"lcv_cfg_delta_store", "lcv_cfg_delta_apply"}
    assert len(protos["lcv_cfg_delta_store"].split(",")) == len(lib._SIGNATURES_CFGREUSE["lcv_cfg_delta_store"]) == 10
    assert len(protos["lcv_cfg_delta_apply"].split(",")) == len(lib._SIGNATURES_CFGREUSE["lcv_cfg_delta_apply"]) == 6
    so = ctypes.CDLL(str(lib.lib_path()))
    so.lcv_version.restype = ctypes.c_int
    assert so.lcv_version() >= 12
    for name in protos:
        assert hasattr(so, name)
        for other in ("lcv_hip.h", "lcv_hip_stepcache.h", "lcv_hip_solver.h"):    # a header of its own
            assert name not in (ROOT / "include" / other).read_text()

"""Host side of the first-block step cache (`--step-cache`, longcat_video/step_cache.py, include/lcv_hip_stepcache.h): the
policy of `StepCache` with the device's decision stubbed, the numpy restatement against hand-worked values, and the flags on
every runner's parser.  No GPU."""
import importlib.util
import math
import sys
from pathlib import Path

import numpy as np
import pytest

import stepcache_ref as S

ROOT = Path(__file__).resolve().parents[1]
PKG = ROOT / "longcat-video-tta_amd"
RUNNERS = ["delta_experiment/scripts/run_delta_a.py", "delta_experiment/scripts/run_delta_b.py",
           "delta_experiment/scripts/run_delta_c.py", "delta_experiment/scripts/run_film_tta.py",
           "delta_experiment/scripts/run_norm_tune_tta.py", "lora_experiment/scripts/run_full_tta.py",
           "lora_experiment/scripts/run_lora_tta.py", "baseline_experiment/scripts/run_baseline.py"]
BASE = ["--checkpoint-dir", "synthetic", "--data-dir", "synthetic:1", "--output-dir", "unused"]


# ---------------------------------------------------------------------------------------------------------- the policy
def _stubbed(threshold, answers, **kw):
    """A StepCache whose device side is replaced: step k's measurement is answers[k], (decision, num, den) or None."""
    from longcat_video.step_cache import StepCache
    cache = StepCache(threshold, **kw)
    feed = iter(answers)
    cache._measure = lambda x0, x1: next(feed)
    return cache


def _walk(cache, n, forced=()):
    """n forwards through the policy: the forward's calls minus the kernels.  Returns the indices that were computed."""
    computed = []
    for i in range(n):
        cache.set_step(i, forced=i in forced)
        if not cache.should_skip(None, None):
            computed.append(i)
    return computed


YES = (1, [1.0, 2.0], [100.0, 100.0])
NO = (0, [50.0, 2.0], [100.0, 100.0])


def test_first_and_last_step_are_computed_and_a_zero_decision_is_a_compute():
    # no p on step 0 (the device is not even asked); the device says "skip" on 1-5, but 5 is marked forced; 3 says "compute"
    cache = _stubbed(0.1, [None, YES, YES, NO, YES, YES])
    assert _walk(cache, 6, forced={0, 5}) == [0, 3, 5]
    st = cache.stats()
    assert st == {"threshold": 0.1, "max_consecutive": None, "computed": 3, "skipped": 3, "skipped_steps": [1, 2, 4],
                  "distances": [None, 0.02, 0.02, 0.5, 0.02, 0.02]}
    assert st["computed"] + st["skipped"] == 6


def test_a_forced_first_step_with_a_p_left_over_is_still_computed():
    cache = _stubbed(0.1, [YES, YES])
    assert _walk(cache, 2, forced={0}) == [0]
    assert cache.stats()["distances"] == [0.02, 0.02]                 # a forced step still records its distance


def test_cap_after_k_skips_in_a_row():
    cache = _stubbed(math.inf, [None] + [YES] * 7, max_consecutive=2)
    assert _walk(cache, 8, forced={0, 7}) == [0, 3, 6, 7]
    assert cache.stats()["skipped_steps"] == [1, 2, 4, 5] and cache.stats()["max_consecutive"] == 2
    cache = _stubbed(math.inf, [None] + [YES] * 5, max_consecutive=2)
    assert _walk(cache, 6, forced={0, 5}) == [0, 3, 5]                # the issue's six-step case
    cache = _stubbed(math.inf, [None, YES, NO, YES, YES, YES], max_consecutive=2)
    assert _walk(cache, 6) == [0, 2, 5]                               # a compute restarts the count


def test_distance_is_the_worst_row_in_double_and_inf_where_a_den_is_zero():
    cache = _stubbed(0.5, [None, (0, [1.0, 3.0], [4.0, 4.0]), (0, [1.0, 0.0], [4.0, 0.0]), (0, [math.nan, 0.0], [4.0, 1.0])])
    _walk(cache, 4)
    d = cache.stats()["distances"]
    assert d[0] is None and d[1] == 0.75 and d[2] == math.inf and math.isnan(d[3])
    third = _stubbed(0.5, [None, (0, [1.0], [3.0])])
    _walk(third, 2)
    assert third.stats()["distances"][1] == 1.0 / 3.0                 # formed in double, not in fp32


def test_steps_without_set_step_count_up_and_are_not_forced():
    cache = _stubbed(0.1, [None, YES, YES])
    assert [cache.should_skip(None, None) for _ in range(3)] == [False, True, True]
    assert cache.stats()["skipped_steps"] == [1, 2]


def test_begin_and_reset():
    cache = _stubbed(0.1, [None, YES, None, YES])
    _walk(cache, 2)
    cache._p = cache._r = cache._R = object()
    cache.begin()                                                     # a new denoise call: statistics and p go, buffers stay
    assert cache.stats() == {"threshold": 0.1, "max_consecutive": None, "computed": 0, "skipped": 0, "skipped_steps": [],
                             "distances": []}
    assert not cache._have_p and cache._R is not None
    _walk(cache, 2)
    assert cache.stats()["skipped_steps"] == [1]
    cache.reset()
    assert cache._p is None and cache._r is None and cache._R is None and cache._out is None and cache._host is None
    assert cache.stats()["computed"] == 0 and cache.stats()["distances"] == []


def test_p_follows_the_computed_steps_only():
    """p <- r is a swap of the two buffers, on a compute and never on a skip."""
    cache = _stubbed(0.1, [None, YES, NO, YES])
    a, b = object(), object()
    cache._p, cache._r = a, b
    seen = []
    for i in range(4):
        cache.should_skip(None, None)
        seen.append(cache._p)
    assert seen == [b, b, a, a]


@pytest.mark.parametrize("bad", [-1.0, -1e-9, math.nan])
def test_bad_thresholds_raise(bad):
    from longcat_video.step_cache import StepCache
    with pytest.raises(ValueError, match="threshold"):
        StepCache(bad)


@pytest.mark.parametrize("bad", [0, -3, 1.5])
def test_bad_caps_raise(bad):
    from longcat_video.step_cache import StepCache
    with pytest.raises(ValueError, match="max_consecutive"):
        StepCache(0.1, max_consecutive=bad)


# ---------------------------------------------------------------------------------------------------------- the restatement
def _bits(*values):
    return S.f32_to_bf16(np.array(values, dtype=np.float32))


def test_bf16_round_to_nearest_even_by_hand():
    # 1 + 2^-8 is a tie between 1 and 1 + 2^-7: the even word (1.0) wins; 1 + 3 * 2^-8 ties upward to 1 + 2^-6
    assert S.f32_to_bf16(np.float32(1.0 + 2.0 ** -8)) == 0x3F80
    assert S.f32_to_bf16(np.float32(1.0 + 3 * 2.0 ** -8)) == 0x3F82
    assert S.f32_to_bf16(np.float32(1.0 + 2.0 ** -8 + 2.0 ** -20)) == 0x3F81
    assert S.f32_to_bf16(np.float32(-2.5)) == 0xC020 and S.bf16_to_f32(np.uint16(0xC020)) == -2.5
    assert np.isnan(S.bf16_to_f32(S.f32_to_bf16(np.float32(np.nan))))
    assert S.f32_to_bf16(np.float32(np.inf)) == 0x7F80


def test_residual_and_apply_by_hand():
    x0, x1 = _bits(1.0, 2.0, -0.5, 3.0), _bits(1.5, 2.0, 0.25, 3.0 + 2.0 ** -6)
    r = S.residual(x1, x0)
    assert list(S.bf16_to_f32(r)) == [0.5, 0.0, 0.75, 2.0 ** -6]
    assert r[1] == 0                                                  # x - x is +0
    # 256 + 1 is not a bf16 (8 significant bits): the sum rounds to even, 256
    assert list(S.bf16_to_f32(S.apply(_bits(256.0, 1.0), _bits(1.0, 0.5)))) == [256.0, 1.5]
    assert list(S.bf16_to_f32(S.apply(_bits(256.0), _bits(3.0)))) == [260.0]      # 259 ties between 258 and 260: even


def test_sums_and_decision_by_hand():
    r = np.stack([_bits(1.0, -2.0, 0.5, 0.0), _bits(1.0, 1.0, 1.0, 1.0)])
    p = np.stack([_bits(0.5, -1.0, 0.5, 4.0), _bits(1.0, 1.0, 1.0, 1.0)])
    num, den = S.sums(r, p)
    assert list(num) == [5.5, 0.0] and list(den) == [6.0, 4.0]
    assert S.decision(num, den, 1.0) == 1 and S.decision(num, den, 0.5) == 0
    assert S.decision([3.0], [6.0], 0.5) == 0                         # equality is not "less"
    assert S.decision([3.0], [6.0], np.nextafter(np.float32(0.5), np.float32(1))) == 1
    assert S.decision([0.0], [0.0], np.inf) == 0 and S.decision([0.0], [1.0], 0.0) == 0
    assert S.decision([np.nan], [1.0], np.inf) == 0 and S.decision([1.0, 1.0], [4.0, 1.0], 0.5) == 0
    assert S.decision([1.0], [1e-30], np.inf) == 1


# ---------------------------------------------------------------------------------------------------------- the parsers
def _parser(rel):
    path = PKG / rel
    sys.path.insert(0, str(path.parent))
    try:
        spec = importlib.util.spec_from_file_location("sc_parser_" + path.stem, path)
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
    parse = _parser(rel)
    a = parse(BASE + ["--step-cache", "0.05", "--step-cache-max-skip", "2"])
    assert a.step_cache == 0.05 and a.step_cache_max_skip == 2
    assert C.step_cache_record(a) == {"step_cache": 0.05, "step_cache_max_skip": 2}
    a = parse(BASE + ["--step-cache", "0"])
    assert a.step_cache == 0.0 and C.step_cache_record(a) == {"step_cache": 0.0, "step_cache_max_skip": None}
    assert parse(BASE + ["--step-cache", "inf"]).step_cache == math.inf
    a = parse(BASE)
    assert a.step_cache is None and a.step_cache_max_skip is None
    assert C.step_cache_record(a) == {} and C.step_cache_from_args(a) is None and C.step_cache_result({}) == {}


@pytest.mark.parametrize("rel", RUNNERS)
@pytest.mark.parametrize("bad,said", [(["--step-cache", "-0.1"], "THRESH must be >= 0"),
                                      (["--step-cache", "nan"], "THRESH must be >= 0"),
                                      (["--step-cache-max-skip", "2"], "needs --step-cache"),
                                      (["--step-cache", "0.1", "--step-cache-max-skip", "0"], "K must be >= 1")])
def test_every_runner_refuses_the_bad_combinations(rel, bad, said, capsys):
    parse = _parser(rel)
    with pytest.raises(SystemExit) as e:
        parse(BASE + bad)
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert said in err and "Traceback" not in err


def test_the_runners_main_uses_the_checking_parse():
    """A main that parsed with the bare parser would accept --step-cache-max-skip alone."""
    for rel in RUNNERS:
        text = (PKG / rel).read_text()
        assert "parse_with_step_cache" in text, rel


def test_cache_from_args():
    from tta import cli_args as C
    from longcat_video.step_cache import StepCache
    a = _parser(RUNNERS[-1])(BASE + ["--step-cache", "0.25", "--step-cache-max-skip", "3"])
    cache = C.step_cache_from_args(a)
    assert isinstance(cache, StepCache) and cache.threshold == 0.25 and cache.max_consecutive == 3
    assert C.step_cache_from_args(a) is not cache                     # one per continuation
    assert C.step_cache_result({"_step_cache": {"computed": 2}}) == {"step_cache": {"computed": 2}}


def test_header_and_bindings_agree():
    """The three entry points of the header are exported, bound with the header's argument counts, and the version went up."""
    import ctypes
    import re
    from lcv_hip import lib
    header = (ROOT / "include" / "lcv_hip_stepcache.h").read_text()
    protos = {m.group(1): m.group(2) for m in re.finditer(r"^int (lcv_\w+)\(([^;]*)\);", header, re.M | re.S)}
    assert set(protos) == set(lib._SIGNATURES_STEPCACHE) == {"lcv_stepcache_diff", "lcv_stepcache_store", "lcv_stepcache_apply"}
    for name, args in protos.items():
        assert len(args.split(",")) == len(lib._SIGNATURES_STEPCACHE[name]), name
    so = ctypes.CDLL(str(lib.lib_path()))
    so.lcv_version.restype = ctypes.c_int
    assert so.lcv_version() >= 10                     # went up with the new entry points
    for name in protos:
        assert hasattr(so, name), name

"""GPU: stochastic rounding for the bf16 optimizer steps (include/lcv_hip_sr.h, `stochastic_rounding=True` /
`--stochastic-rounding`).

1. lcv_sr_round against the numpy restatement (tests/sr_ref.py), bit for bit, on every kind of 32-bit pattern, through the
   packet path and the scalar path, at sizes around a packet and around a chunk.
2. Both steps through the optimizers, bit for bit after each of three steps, over one table that covers a single element,
   sub-packet tails, an exact chunk, one element past a chunk (as a 2-byte offset view: the scalar path, first_chunk > 0) and a
   tail past two chunks, plus a parameter without a gradient.
3. What the feature is for: updates of 1/32 bf16 ulp vanish under round-to-nearest and survive in the mean under SR.
4. The ratchet: bf16 AdamW's second moment does not decay under round-to-nearest and decays in the mean under SR.
5. The optimizer object: follows torch.manual_seed, moves the generator by 4 per step, the plain form's storage, the refusals.
6. The loops (flag off: today's bits; flag on: reproducible and different) and the three runners.
"""
import importlib.util
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import master_weights_ref as W
import sr_ref as R
import test_gpu_master_weights as M

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
BF16, DEV = M.BF16, M.DEV
NUMELS = (1, 7, 8, 9, 2047, 2048, 2049, 4099)
VIEW = 6                      # the 2049-element tensor is a [1:] view: pointers at a 2-byte offset, first_chunk 6
NO_GRAD = 300                 # a ninth parameter that never receives a gradient
FIRST = R.first_chunks(NUMELS)
SEED = 0x5EED0123456789


def _gen():
    return torch.cuda.default_generators[torch.cuda.current_device()]


# ---------------------------------------------------------------------------------------------------------- 1. the rounding
@pytest.fixture(scope="module")
def patterns():
    return W.edge_patterns(n_random=1 << 16, seed=31)             # 24 specials + 2^16 random patterns: 32 chunks and a tail


@pytest.mark.parametrize("offset_view", [False, True])
@pytest.mark.parametrize("n", [1, 7, 8, 9, 2047, 2049, None])
def test_sr_round_bits(patterns, n, offset_view):
    m = patterns if n is None else patterns[:n]
    guard = 8
    src = M._f32_dev(m)
    out = torch.full((m.size + guard,), -7.0, dtype=BF16, device=DEV)       # 0xc0e0: the guard must come back untouched
    if offset_view:
        src, out = M._offset_view(src), M._offset_view(out)
    seed, offset = SEED, (1 << 32) + 5                                # both halves of the key and of the offset are live
    M._call("lcv_sr_round", src.data_ptr(), out.data_ptr(), m.size, seed, offset)
    torch.cuda.synchronize()
    got = M._h_of(out)
    want = R.sr_round(m, seed, offset)
    bad = np.flatnonzero(got[:m.size] != want)
    assert bad.size == 0, [(int(i), hex(int(m[i])), hex(int(got[i])), hex(int(want[i]))) for i in bad[:8]]
    assert np.all(got[m.size:] == 0xC0E0)
    if n is None:                                                     # the wrapper is the same call
        from lcv_hip import ops
        assert np.array_equal(M._h_of(ops.sr_round(M._f32_dev(m), seed, offset)), want)
        # the rounding went both ways: about half of the random patterns moved away from zero
        away = (want[24:] != (m[24:] >> 16)).mean()
        assert 0.45 < away < 0.55


def test_bad_arguments_are_refused():
    from lcv_hip.lib import LcvError
    t = torch.zeros(8, dtype=torch.float32, device=DEV)
    h = torch.zeros(8, dtype=BF16, device=DEV)
    big = 1 << 31
    for name, args in (("lcv_sr_round", (t.data_ptr(), h.data_ptr(), 0, 1, 0)),
                       ("lcv_sr_round", (None, h.data_ptr(), 8, 1, 0)),
                       ("lcv_sr_round", (t.data_ptr(), None, 8, 1, 0)),
                       ("lcv_sr_sgd_step", (None, 1, 1, None, 1e-3, 0.0, 1, 0)),
                       ("lcv_sr_sgd_step", (t.data_ptr(), 0, 1, None, 1e-3, 0.0, 1, 0)),
                       ("lcv_sr_sgd_step", (t.data_ptr(), 1, big, None, 1e-3, 0.0, 1, 0)),
                       ("lcv_sr_adamw_step", (None, 1, 1, None, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1, 0)),
                       ("lcv_sr_adamw_step", (t.data_ptr(), 1, 0, None, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1, 0)),
                       ("lcv_sr_adamw_step", (t.data_ptr(), big, 1, None, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1, 1, 0)),
                       ("lcv_sr_adamw_step", (t.data_ptr(), 1, 1, None, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 1, 0))):
        with pytest.raises(LcvError) as e:
            M._call(name, *args)
        assert e.value.code == -1 and not e.value.fatal


# ---------------------------------------------------------------------------------------------------------- 2. the steps
_TABLE = {}


def _table():
    """Host-generated inputs, made once: |w| in [2^-10, 2], |g| in [2^-20, 8], both signs.  Eight tensors with a gradient for
    three steps, and a ninth without one."""
    if not _TABLE:
        rng = np.random.default_rng(37)
        _TABLE["w"] = [W.weights(rng, n)[0] for n in NUMELS + (NO_GRAD,)]
        _TABLE["g"] = [[W.grads(rng, n) for n in NUMELS] for _ in range(3)]
    return _TABLE


def _make(kind, wd):
    from lcv_hip import ops
    params = []
    for k, h in enumerate(_table()["w"]):
        p = M._bf16_dev(h)
        params.append(M._offset_view(p) if k == VIEW else p)
    if kind == "sgd":
        return ops.FusedSGDClip(params, lr=2e-3, weight_decay=wd, stochastic_rounding=True), params
    opt = ops.FusedAdamWClip(params, lr=1e-3, betas=(0.9, 0.999), weight_decay=wd, eps=1e-8, stochastic_rounding=True)
    # one moment of two aligned parameters at a 2-byte offset: a single unaligned pointer sends the whole row down the scalar path
    opt.exp_avg[5] = M._offset_view(opt.exp_avg[5])
    opt.exp_avg_sq[7] = M._offset_view(opt.exp_avg_sq[7])
    return opt, params


def _report(what, k, got, want):
    bad = np.flatnonzero(got != want)
    if bad.size:
        i = int(bad[0])
        raise AssertionError(f"{what}: tensor {k} (numel {got.size}) index {i}: got {int(got[i]):#06x} want {int(want[i]):#06x}; "
                             f"{bad.size} mismatches")


def _run_steps(kind, clip, wd, seed=SEED, offset0=0):
    """Three steps on the GPU next to three steps of the restatement, compared after each; the generator's offset moves by 4
    per step and the restatement follows it."""
    t = _table()
    torch.manual_seed(seed)
    gen = _gen()
    gen.set_offset(offset0)
    opt, params = _make(kind, wd)
    ref = [dict(h=h.copy(), m=np.zeros(h.size, np.uint16), v=np.zeros(h.size, np.uint16)) for h in t["w"]]
    for step in range(3):
        for k in range(len(NUMELS)):
            g = M._bf16_dev(t["g"][step][k])
            params[k].grad = M._offset_view(g) if k == VIEW else g
        coef = 1.0
        if clip:
            opt.clip_grad_norm_(1.0)
            norm, coef = (float(x) for x in opt._norm_coef.tolist())
            assert 0.0 < coef < 1.0 and norm > 1.0            # the gradients are large: the coefficient is live
        offset = gen.get_offset()
        assert gen.initial_seed() == seed and offset == offset0 + 4 * step
        opt.step()
        torch.cuda.synchronize()
        assert gen.get_offset() == offset + 4
        for k in range(len(NUMELS)):
            r, g = ref[k], t["g"][step][k]
            if kind == "sgd":
                r["h"] = R.sgd_step(r["h"], g, coef, 2e-3, wd, FIRST[k], seed, offset)
            else:
                r["h"], r["m"], r["v"] = R.adamw_step(r["h"], r["m"], r["v"], g, coef, 1e-3, 0.9, 0.999, 1e-8, wd, step + 1, FIRST[k],
                                                      seed, offset)
        for k, r in enumerate(ref):
            _report(f"{kind} step {step + 1} p", k, M._h_of(params[k]), r["h"])
            if kind == "adamw":
                _report(f"{kind} step {step + 1} exp_avg", k, M._h_of(opt.exp_avg[k]), r["m"])
                _report(f"{kind} step {step + 1} exp_avg_sq", k, M._h_of(opt.exp_avg_sq[k]), r["v"])
    assert np.array_equal(ref[-1]["h"], t["w"][-1])               # the parameter without a gradient was skipped
    return [r["h"] for r in ref]


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("clip", [False, True])
def test_sr_sgd_step_bits(clip, wd):
    h = _run_steps("sgd", clip, wd)
    assert sum(int((a != b).sum()) for a, b in zip(h, _table()["w"])) > 0


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("clip", [False, True])
def test_sr_adamw_step_bits(clip, wd):
    h = _run_steps("adamw", clip, wd)
    assert sum(int((a != b).sum()) for a, b in zip(h, _table()["w"])) > 0


@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_same_seed_and_offset_same_bits_another_offset_other_bits(kind):
    a = _run_steps(kind, False, 0.01, offset0=8)
    b = _run_steps(kind, False, 0.01, offset0=8)
    c = _run_steps(kind, False, 0.01, offset0=12)
    d = _run_steps(kind, False, 0.01, seed=SEED + 1, offset0=8)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert any(not np.array_equal(x, y) for x, y in zip(a, c)) and any(not np.array_equal(x, y) for x, y in zip(a, d))


# ---------------------------------------------------------------------------------------------------------- 3. small updates
def test_updates_of_a_32nd_ulp_vanish_under_round_to_nearest_and_survive_in_the_mean_under_sr():
    """65 536 elements at 1.5, gradient 1, lr = 2^-12 (1/32 of the bf16 ulp 2^-7 of [1, 2)), wd 0, 64 steps: the fp32 results
    sum to 1.5 - 2^-6.  Each SR store has variance at most ulp^2 / 4 and the stores are independent, so an element's value after
    K steps has variance at most K ulp^2 / 4 and the mean over N elements has standard deviation at most
    (ulp / 2) sqrt(K / N) = 2^-8 sqrt(64 / 65 536) = 1.22e-4; the bound is six of those, 6 * 2^-7 * sqrt(64 / (4 * 65 536))
    = 7.3e-4.  The values stay in [1, 2), so the ulp is constant.  The seed is fixed: the test is deterministic."""
    from lcv_hip import ops
    n, K, lr = 1 << 16, 64, 2.0 ** -12
    g = torch.ones(n, dtype=BF16, device=DEV)
    means = {}
    for sr in (False, True):
        torch.manual_seed(41)
        p = torch.full((n,), 1.5, dtype=BF16, device=DEV)
        opt = ops.FusedSGDClip([p], lr=lr, weight_decay=0.0, stochastic_rounding=sr)
        for _ in range(K):
            p.grad = g
            opt.step()
        torch.cuda.synchronize()
        v = p.float().cpu().numpy().astype(np.float64)
        if not sr:
            assert np.all(v == 1.5)                                   # the pinned behaviour: every update is discarded
        else:
            assert v.min() >= 1.0 and v.max() < 2.0 and len(np.unique(v)) > 2
        means[sr] = float(v.mean())
    bound = 6 * 2.0 ** -7 * (K / (4.0 * n)) ** 0.5
    print(f"mean after {K} steps of 1/32 ulp: {means[True]!r}, expected {1.5 - 2.0 ** -6!r}, "
          f"off by {abs(means[True] - (1.5 - 2.0 ** -6)):.3e}, bound {bound:.3e}")
    assert 7.2e-4 < bound < 7.4e-4
    assert abs(means[True] - (1.5 - 2.0 ** -6)) <= bound


# ---------------------------------------------------------------------------------------------------------- 4. the ratchet
def test_second_moment_does_not_decay_under_round_to_nearest_and_decays_in_the_mean_under_sr():
    """AdamW with zero gradients, exp_avg_sq = 1.0, exp_avg = 0, wd 0, 200 steps over 65 536 elements.  The plain bf16 step
    leaves exp_avg_sq at 1.0 exactly (bf16(v * 0.999f) == v).  Under SR each step's expectation is the fp32 product
    v * 0.999f, so the mean follows 0.999^200 = 0.81865; v stays in [0.5, 1], where the step down is 2^-8, each store has
    variance at most 2^-16 / 4, an earlier store's error reaches the end scaled by at most 1, and so the mean over N elements
    has standard deviation at most 2^-9 sqrt(K / N) = 1.08e-4.  The bound is six of those, 6.5e-4, plus 200 fp32 roundings of
    the product (200 * 2^-24 = 1.2e-5) and the distance of 0.999f from 0.999 (200 * 1.1e-8 relative)."""
    from lcv_hip import ops
    n, K = 1 << 16, 200
    zero = torch.zeros(n, dtype=BF16, device=DEV)
    means = {}
    for sr in (False, True):
        torch.manual_seed(43)
        p = torch.full((n,), 0.25, dtype=BF16, device=DEV)
        opt = ops.FusedAdamWClip([p], lr=1e-3, betas=(0.9, 0.999), weight_decay=0.0, eps=1e-8, stochastic_rounding=sr)
        opt.exp_avg_sq[0].fill_(1.0)
        for _ in range(K):
            p.grad = zero
            opt.step()
        torch.cuda.synchronize()
        v = opt.exp_avg_sq[0].float().cpu().numpy().astype(np.float64)
        assert not opt.exp_avg[0].any() and torch.all(p == 0.25)
        if not sr:
            assert np.all(v == 1.0)                                   # the ratchet: 200 decays, nothing moved
        else:
            assert v.min() >= 0.5 and v.max() <= 1.0
        means[sr] = float(v.mean())
    want = 0.999 ** K
    bound = 6 * 2.0 ** -9 * (K / n) ** 0.5 + K * 2.0 ** -24 + K * 1.1e-8
    print(f"mean exp_avg_sq after {K} zero-gradient steps: {means[True]!r}, expected {want!r}, "
          f"off by {abs(means[True] - want):.3e}, bound {bound:.3e}")
    assert abs(means[True] - want) <= bound


# ---------------------------------------------------------------------------------------------------------- 5. the optimizer
@pytest.mark.parametrize("cls", ["FusedSGDClip", "FusedAdamWClip"])
def test_optimizer_follows_manual_seed_moves_the_generator_by_four_and_keeps_the_plain_storage(cls):
    from lcv_hip import ops
    rng = np.random.default_rng(47)
    hs = [W.weights(rng, n)[0] for n in (5, 2049)]
    gs = [[W.grads(rng, h.size) for h in hs] for _ in range(2)]
    make = getattr(ops, cls)

    def run(seed, sr=True):
        torch.manual_seed(seed)
        ps = [M._bf16_dev(h) for h in hs]
        opt = make(ps, lr=1e-3, weight_decay=0.01, stochastic_rounding=sr)
        gen = _gen()
        for step_grads in gs:
            for p, g in zip(ps, step_grads):
                p.grad = M._bf16_dev(g)
            before = gen.get_offset()
            opt.clip_grad_norm_(1.0)
            assert gen.get_offset() == before                   # the clip draws nothing
            opt.step()
            assert gen.get_offset() == before + (4 if sr else 0)
        torch.cuda.synchronize()
        state = [M._h_of(p) for p in ps]
        if cls == "FusedAdamWClip":
            state += [M._h_of(t) for ts in (opt.exp_avg, opt.exp_avg_sq) for t in ts]
        return state, opt

    a, opt = run(101)
    b, _ = run(101)
    c, _ = run(102)
    plain, plain_opt = run(101, sr=False)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert any(not np.array_equal(x, y) for x, y in zip(a, c)) and any(not np.array_equal(x, y) for x, y in zip(a, plain))
    # storage: exactly the plain form's
    assert opt.stochastic_rounding is True and opt.master_weights is False and opt.low_words == [] and opt.step_count == 2
    assert opt.state_bytes() == plain_opt.state_bytes()
    if cls == "FusedAdamWClip":
        assert opt.state_bytes() == 2 * 2 * sum(h.size for h in hs)
        for ts in (opt.exp_avg, opt.exp_avg_sq):
            assert all(t.dtype == BF16 and t.shape == p.shape for t, p in zip(ts, opt.params))
    else:
        assert opt.state_bytes() == 0


@pytest.mark.parametrize("cls", ["FusedSGDClip", "FusedAdamWClip"])
def test_optimizer_refusals(cls):
    from lcv_hip import ops
    from lcv_hip.lib import LcvError
    make = getattr(ops, cls)
    bf = lambda: [torch.zeros(16, dtype=BF16, device=DEV)]
    with pytest.raises(LcvError, match="rounds nothing to bf16"):
        make([torch.zeros(16, dtype=torch.float32, device=DEV)], stochastic_rounding=True)
    with pytest.raises(LcvError, match="needs parameters on the GPU"):
        make([torch.zeros(16, dtype=BF16)], stochastic_rounding=True)
    with pytest.raises(LcvError, match="needs contiguous parameters"):
        make([torch.zeros(4, 8, dtype=BF16, device=DEV).t()], stochastic_rounding=True)
    with pytest.raises(LcvError, match="cannot be combined with master_weights=True"):
        make(bf(), master_weights=True, stochastic_rounding=True)
    with pytest.raises(LcvError, match=r"cannot be combined with grad_accum > 1"):
        make(bf(), stochastic_rounding=True, grad_accum=2)
    with pytest.raises(LcvError, match="cannot be combined with anchor"):
        make(bf(), stochastic_rounding=True, anchor=bf())
    if cls == "FusedAdamWClip":
        with pytest.raises(LcvError, match="cannot be combined with moments_8bit=True"):
            make(bf(), moments_8bit=True, stochastic_rounding=True)
    opt = make(bf(), stochastic_rounding=True)
    with pytest.raises(LcvError, match="enable_weight_ema.. needs master_weights=True"):
        opt.enable_weight_ema(0.9)
    with pytest.raises(LcvError) as info:                       # one line each
        make(bf(), master_weights=True, stochastic_rounding=True)
    assert "\n" not in str(info.value)


# ---------------------------------------------------------------------------------------------------------- 6. loops, runners
@pytest.fixture
def deterministic():
    from lcv_hip import ops
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    yield ops
    ops.set_deterministic(was)


@pytest.mark.parametrize("method", ["lora", "full"])
def test_loops_flag_off_is_todays_run_and_flag_on_is_reproducible_and_different(method, deterministic):
    l0, w0, _ = M._adapt(method)                                  # the keyword omitted
    l1, w1, _ = M._adapt(method, stochastic_rounding=False)
    assert len(l0) == 3 and l0 == l1 and all(torch.equal(a, b) for a, b in zip(w0, w1))
    la, wa, _ = M._adapt(method, stochastic_rounding=True)
    lb, wb, _ = M._adapt(method, stochastic_rounding=True)
    assert all(np.isfinite(float.fromhex(v)) for v in la) and len(la) == 3
    assert la == lb and all(torch.equal(a, b) for a, b in zip(wa, wb))
    assert la[0] == l0[0]                                       # the first forward sees the same weights either way
    assert any(not torch.equal(a, b) for a, b in zip(wa, w0))   # and the steps are not the plain ones


def test_loops_refuse_what_the_flag_cannot_be_combined_with():
    from lcv_hip.lib import LcvError
    with pytest.raises(LcvError, match="cannot be combined with master_weights=True"):
        M._adapt("lora", stochastic_rounding=True, master_weights=True)
    with pytest.raises(LcvError, match="cannot be combined with master_weights=True"):
        M._adapt("full", stochastic_rounding=True, master_weights=True)


def _main(rel, argv):
    spec = importlib.util.spec_from_file_location("sr_" + Path(rel).stem, ROOT / "longcat-video-tta_amd" / rel)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    m.main(argv)


COMMON = ["--checkpoint-dir", "synthetic:2:256:64", "--data-dir", "synthetic:1", "--num-cond-frames", "5", "--num-frames", "13",
          "--gen-start-frame", "40", "--tta-total-frames", "33", "--tta-context-frames", "9", "--num-inference-steps", "2",
          "--no-save-videos"]


@pytest.mark.parametrize("rel, extra", [
    ("lora_experiment/scripts/run_lora_tta.py", ["--num-steps", "4", "--es-check-every", "2", "--es-patience", "1", "--lora-rank", "4",
                                                 "--lora-alpha", "8"]),
    ("lora_experiment/scripts/run_full_tta.py", ["--num-steps", "4", "--learning-rate", "1e-4", "--es-disable"]),
    ("lora_experiment/scripts/run_full_tta.py", ["--num-steps", "4", "--learning-rate", "1e-4", "--es-disable", "--optimizer", "adamw"]),
    ("delta_experiment/scripts/run_norm_tune_tta.py", ["--norm-steps", "4", "--norm-lr", "1e-2", "--es-check-every", "2",
                                                       "--es-patience", "1"]),
])
def test_runners_accept_the_flag_and_record_it(tmp_path, rel, extra):
    out = tmp_path / "run"
    _main(rel, COMMON + extra + ["--output-dir", str(out), "--stochastic-rounding"])
    s = json.loads((out / "summary.json").read_text())
    r = s["results"][0]
    assert s["num_videos"] == 1 and s["num_successful"] == 1 and r["success"] and r["final_loss"] == r["final_loss"]
    assert r["stochastic_rounding"] is True
    if "norm_tune" in rel:
        assert s["stochastic_rounding"] is True and "master_weights" not in s
    else:
        cfg = json.loads((out / "config.json").read_text())
        assert cfg["training"]["stochastic_rounding"] is True and cfg["training"]["master_weights"] is False

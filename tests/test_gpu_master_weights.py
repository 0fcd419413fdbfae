"""GPU: fp32 master weights for bf16 parameters (include/lcv_hip_master.h, `master_weights=True` / `--master-weights`).

1. lcv_master_split / lcv_master_join against the numpy restatement (tests/master_weights_ref.py), bit for bit, on every kind of
   32-bit pattern, through the packet path and the scalar path.
2. Both steps through the optimizers, bit for bit on the bf16 words, the low words and (AdamW) both fp32 moments after 1 and 3
   steps, over one table that covers a single element, a sub-packet tail, an exact chunk, one element past a chunk (as a 2-byte
   offset view: the scalar path) and a tail past two chunks, plus a parameter without a gradient.
3. Accumulation: updates of 1/8 bf16 ulp leave the rounding form where it started and move the master form exactly as restated.
4. resync() / master_tensors().
5. The loops (flag off: today's bits; flag on: finite, reproducible, low words zero after the stopper's restore) and the runners.
"""
import importlib.util
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import master_weights_ref as R

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
SCRIPTS = ROOT / "longcat-video-tta_amd" / "lora_experiment" / "scripts"
BF16 = torch.bfloat16
DEV = "cuda"
NUMELS = (1, 7, 2048, 2049, 4099)
VIEW = 3                      # the 2049-element tensor is a [1:] view: pointers at a 2-byte offset


# ---------------------------------------------------------------------------------------------------------- helpers
def _bf16_dev(h):
    return torch.from_numpy(np.ascontiguousarray(h).view(np.int16).copy()).view(BF16).to(DEV)


def _i16_dev(low):
    return torch.from_numpy(np.ascontiguousarray(low, dtype=np.int16).copy()).to(DEV)


def _f32_dev(m):
    return torch.from_numpy(np.ascontiguousarray(m, dtype=np.uint32).view(np.int32).copy()).view(torch.float32).to(DEV)


def _h_of(t):
    return t.detach().contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _bits_of(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy().view(np.uint32)


def _offset_view(t):
    """The same values in storage that starts one element late: a contiguous view whose pointer is not 16-byte aligned."""
    base = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    base[1:].copy_(t)
    v = base[1:]
    assert v.data_ptr() % 16 == t.element_size() and v.is_contiguous()
    return v


def _call(name, *args):
    from lcv_hip import lib
    lib.call(name, *args, torch.cuda.current_stream().cuda_stream)


# ---------------------------------------------------------------------------------------------------------- 1. split / join
@pytest.fixture(scope="module")
def patterns():
    m = R.edge_patterns(n_random=(1 << 16) + 5, seed=11)          # 32 packet-blocks and a tail of 5 + 24 specials
    h, low = R.split(m)
    return m, h, low


@pytest.mark.parametrize("offset", [False, True])
def test_split_bits(patterns, offset):
    m, h, low = patterns
    src = _f32_dev(m)
    hi = torch.zeros(m.size, dtype=BF16, device=DEV)
    lo = torch.zeros(m.size, dtype=torch.int16, device=DEV)
    if offset:
        src, hi, lo = _offset_view(src), _offset_view(hi), _offset_view(lo)
    _call("lcv_master_split", src.data_ptr(), hi.data_ptr(), lo.data_ptr(), m.size)
    torch.cuda.synchronize()
    got_h, got_l = _h_of(hi), lo.cpu().numpy()
    bad = np.flatnonzero((got_h != h) | (got_l != low))
    assert bad.size == 0, [(int(i), hex(int(m[i])), hex(int(got_h[i])), int(got_l[i]), hex(int(h[i])), int(low[i])) for i in bad[:8]]


@pytest.mark.parametrize("offset", [False, True])
def test_join_bits(patterns, offset):
    m, h, low = patterns
    hi, lo = _bf16_dev(h), _i16_dev(low)
    out = torch.zeros(m.size, dtype=torch.float32, device=DEV)
    if offset:
        hi, lo, out = _offset_view(hi), _offset_view(lo), _offset_view(out)
    _call("lcv_master_join", hi.data_ptr(), lo.data_ptr(), out.data_ptr(), m.size)
    torch.cuda.synchronize()
    got = _bits_of(out)
    bad = np.flatnonzero(got != m)
    assert bad.size == 0, [(int(i), hex(int(h[i])), int(low[i]), hex(int(got[i])), hex(int(m[i]))) for i in bad[:8]]


def test_bad_arguments_are_refused():
    from lcv_hip.lib import LcvError
    t = torch.zeros(8, dtype=torch.float32, device=DEV)
    hi = torch.zeros(8, dtype=BF16, device=DEV)
    lo = torch.zeros(8, dtype=torch.int16, device=DEV)
    for name, args in (("lcv_master_split", (t.data_ptr(), hi.data_ptr(), lo.data_ptr(), 0)),
                       ("lcv_master_split", (t.data_ptr(), hi.data_ptr(), None, 8)),
                       ("lcv_master_join", (hi.data_ptr(), lo.data_ptr(), None, 8)),
                       ("lcv_master_sgd_step", (t.data_ptr(), None, 1, 1, None, 1e-3, 0.0)),
                       ("lcv_master_adamw_step", (t.data_ptr(), t.data_ptr(), 1, 1, None, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0))):
        with pytest.raises(LcvError) as e:
            _call(name, *args)
        assert e.value.code == -1 and not e.value.fatal


# ---------------------------------------------------------------------------------------------------------- 2. the steps
_TABLE = {}


def _table():
    """Host-generated inputs, made once: |w| in [2^-10, 2], |g| in [2^-20, 8], both signs - every intermediate of either step
    is then a normal fp32 number.  Five tensors with a gradient for three steps, and a sixth without one."""
    if not _TABLE:
        rng = np.random.default_rng(17)
        _TABLE["w"] = [R.weights(rng, n) for n in NUMELS + (300,)]
        _TABLE["g"] = [[R.grads(rng, n) for n in NUMELS] for _ in range(3)]
    return _TABLE


def _make(kind, wd):
    from lcv_hip import ops
    t = _table()
    params = []
    for k, (h, _) in enumerate(t["w"]):
        p = _bf16_dev(h)
        params.append(_offset_view(p) if k == VIEW else p)
    if kind == "sgd":
        opt = ops.FusedSGDClip(params, lr=2e-3, weight_decay=wd, master_weights=True)
    else:
        opt = ops.FusedAdamWClip(params, lr=1e-3, betas=(0.9, 0.999), weight_decay=wd, eps=1e-8, master_weights=True)
    lows = opt.low_words
    assert len(lows) == len(params) and all(lw.dtype == torch.int16 and lw.shape == p.shape and not lw.any()
                                            for lw, p in zip(lows, params))
    for lw, (_, low) in zip(lows, t["w"]):
        lw.copy_(_i16_dev(low))
    return opt, params


def _report(what, k, got, want, words):
    bad = np.flatnonzero(got != want)
    if bad.size:
        i = int(bad[0])
        h, low, g = words
        raise AssertionError(f"{what}: tensor {k} (numel {got.size}) index {i}: got {got[i]!r} want {want[i]!r}; "
                             f"{bad.size} mismatches; words h={int(h[i]):#06x} l={int(low[i])} g={int(g[i]):#06x}")


def _run_steps(kind, clip, wd):
    """Three steps on the GPU next to three steps of the restatement; compared after the first and after the third."""
    opt, params = _make(kind, wd)
    t = _table()
    ref = [dict(h=h.copy(), l=low.copy(), m=np.zeros(h.size, np.float32), v=np.zeros(h.size, np.float32)) for h, low in t["w"]]
    lows = opt.low_words
    for step in range(3):
        for k in range(len(NUMELS)):
            g = _bf16_dev(t["g"][step][k])
            params[k].grad = _offset_view(g) if k == VIEW else g
        coef = 1.0
        if clip:
            opt.clip_grad_norm_(1.0)
            norm, coef = (float(x) for x in opt._norm_coef.tolist())
            assert 0.0 < coef < 1.0 and norm > 1.0            # the gradients are large: the coefficient is live
        before = [dict(r) for r in ref]
        opt.step()
        torch.cuda.synchronize()
        for k in range(len(NUMELS)):
            r, g = ref[k], t["g"][step][k]
            if kind == "sgd":
                r["h"], r["l"] = R.sgd_step(r["h"], r["l"], g, coef, 2e-3, wd)
            else:
                r["h"], r["l"], r["m"], r["v"] = R.adamw_step(r["h"], r["l"], r["m"], r["v"], g, coef, 1e-3, 0.9, 0.999, 1e-8, wd,
                                                              step + 1)
        if step in (0, 2):
            for k, r in enumerate(ref):
                g = t["g"][step][k] if k < len(NUMELS) else np.zeros(r["h"].size, np.uint16)
                words = (before[k]["h"], before[k]["l"], g)
                _report(f"{kind} step {step + 1} h", k, _h_of(params[k]), r["h"], words)
                _report(f"{kind} step {step + 1} l", k, lows[k].cpu().numpy(), r["l"], words)
                if kind == "adamw":
                    _report(f"{kind} step {step + 1} exp_avg", k, _bits_of(opt.exp_avg[k]), R.bits(r["m"]), words)
                    _report(f"{kind} step {step + 1} exp_avg_sq", k, _bits_of(opt.exp_avg_sq[k]), R.bits(r["v"]), words)
    # the parameter without a gradient was skipped: its words are the table's, and so is its reference
    assert np.array_equal(ref[-1]["h"], t["w"][-1][0]) and np.array_equal(ref[-1]["l"], t["w"][-1][1])
    moved = [int((ref[k]["h"] != t["w"][k][0]).sum()) for k in range(len(NUMELS))]
    return moved


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("clip", [False, True])
def test_sgd_step_bits(clip, wd):
    moved = _run_steps("sgd", clip, wd)
    assert sum(moved) > 0                                       # three steps move bf16 words, clipped or not


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("clip", [False, True])
def test_adamw_step_bits(clip, wd):
    moved = _run_steps("adamw", clip, wd)
    assert sum(moved) > 0                                       # AdamW's step is about lr whatever the gradient's scale


def test_fp32_moments_and_clip_dtype_of_a_master_optimizer():
    from lcv_hip import ops
    p = [torch.zeros(40, dtype=BF16, device=DEV)]
    a = ops.FusedAdamWClip(p, master_weights=True)
    assert a.exp_avg[0].dtype == torch.float32 and a.exp_avg_sq[0].dtype == torch.float32 and a.f32 is False
    s = ops.FusedSGDClip(p, master_weights=True)
    assert s.f32 is False and s.master_weights and s.low_words[0].dtype == torch.int16


# ---------------------------------------------------------------------------------------------------------- 3. accumulation
def _eighth_ulp_case():
    """bf16 weights over several binades and both signs; gradient +-2^e for a weight in [2^e, 2^(e+1)); lr = 2^-10.  A bf16
    ulp of such a weight is 2^(e-7), so lr * |g| = 2^(e-10) is 1/8 ulp of each weight."""
    rng = np.random.default_rng(23)
    n = 4099
    w = R.log_uniform(rng, n, -6.0, 1.0)
    w[:8] = [1.0, -1.0, 0.5, 2.0, -0.25, 1.9921875, 0.0625, -1.5]            # binade edges among them
    h = R.to_bf16_bits(w)
    e = np.floor(np.log2(np.abs(R.bf16_to_f32(h)).astype(np.float64)))
    g = (np.exp2(e) * rng.choice([-1.0, 1.0], size=n)).astype(np.float32)
    gb = R.to_bf16_bits(g)
    assert np.array_equal(R.bf16_to_f32(gb), g)
    return h, gb, 2.0 ** -10


def test_updates_of_an_eighth_ulp_vanish_without_and_accumulate_with_master_weights():
    from lcv_hip import ops
    h0, gb, lr = _eighth_ulp_case()
    results = {}
    for master in (False, True):
        p = _bf16_dev(h0)
        opt = ops.FusedSGDClip([p], lr=lr, weight_decay=0.0, master_weights=master)
        g = _bf16_dev(gb)
        for _ in range(64):
            p.grad = g
            opt.step()
        torch.cuda.synchronize()
        results[master] = (_h_of(p), opt)
    # today's behaviour, on record: every update is discarded, the parameters are bit-identical to the start
    assert np.array_equal(results[False][0], h0)
    # the restatement: 64 steps of 1/8 ulp are 8 ulps
    h, low = h0.copy(), np.zeros(h0.size, np.int16)
    for _ in range(64):
        h, low = R.sgd_step(h, low, gb, 1.0, lr, 0.0)
    got, opt = results[True]
    _report("64 steps of 1/8 ulp, h", 0, got, h, (h0, np.zeros(h0.size, np.int16), gb))
    assert np.array_equal(opt.low_words[0].cpu().numpy(), low)
    assert (got != h0).all()
    # and the master is the exact sum: the start minus 8 ulps' worth of lr * g (11 significant bits, exact in fp32)
    assert np.array_equal(R.master(h, low).astype(np.float64),
                          R.bf16_to_f32(h0).astype(np.float64) - 64 * lr * R.bf16_to_f32(gb).astype(np.float64))


# ---------------------------------------------------------------------------------------------------------- 4. resync
def test_resync_zeroes_the_low_words_and_leaves_the_bf16_words():
    from lcv_hip import ops
    from lcv_hip.lib import LcvError
    rng = np.random.default_rng(29)
    hs = [R.weights(rng, n)[0] for n in (5, 2049)]
    ps = [_bf16_dev(h) for h in hs]
    opt = ops.FusedAdamWClip(ps, lr=1e-3, master_weights=True)
    for _ in range(2):
        for p in ps:
            p.grad = _bf16_dev(R.grads(rng, p.numel()))
        opt.clip_grad_norm_(1.0)
        opt.step()
    lows = opt.low_words
    assert all(lw.any() for lw in lows)
    masters = opt.master_tensors()
    for p, lw, m in zip(ps, lows, masters):
        assert m.dtype == torch.float32 and m.shape == p.shape
        assert np.array_equal(_bits_of(m), R.join(_h_of(p), lw.cpu().numpy()))
    h_before = [_h_of(p).copy() for p in ps]
    opt.resync()
    assert all(not lw.any() for lw in opt.low_words)
    assert all(np.array_equal(_h_of(p), hb) for p, hb in zip(ps, h_before))
    for p, m in zip(ps, opt.master_tensors()):
        assert torch.equal(m, p.float())
    with pytest.raises(LcvError, match="master_weights=True"):
        ops.FusedAdamWClip(ps).master_tensors()


# ---------------------------------------------------------------------------------------------------------- 5. the loops
_SHARED = {}


def _inputs():
    if not _SHARED:
        g = torch.Generator().manual_seed(7)
        r = lambda *s: torch.randn(*s, generator=g)
        _SHARED["cond"] = r(1, 16, 1, 10, 20).to(BF16).to(DEV)            # one conditioning latent frame: 5 x 10 tokens
        _SHARED["train"] = r(1, 16, 2, 10, 20).to(BF16).to(DEV)           # two target frames
        _SHARED["val"] = r(1, 16, 1, 10, 20).to(BF16).to(DEV)             # one held-out frame for the early stopper
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


@pytest.fixture
def made(monkeypatch):
    """The optimizers the loops build, and whether their low words were live when resync() was called."""
    from lcv_hip import ops
    from tta import full_tta, inner_loop
    seen = []

    def recording(cls):
        class Recording(cls):
            def __init__(self, *a, **k):
                super().__init__(*a, **k)
                self.live_at_resync = []
                seen.append(self)

            def resync(self):
                self.live_at_resync.append(any(bool(lw.any()) for lw in self.low_words))
                super().resync()
        return Recording
    monkeypatch.setattr(inner_loop, "FusedAdamWClip", recording(ops.FusedAdamWClip))
    monkeypatch.setattr(full_tta, "FusedAdamWClip", recording(ops.FusedAdamWClip))
    monkeypatch.setattr(full_tta, "FusedSGDClip", recording(ops.FusedSGDClip))
    return seen


def _adapt(method, **flag):
    """Three steps from one seed on a fresh model with an early stopper that checks every step and restores its best state."""
    from tta.early_stopping import AnchoredEarlyStopper
    from tta.full_tta import finetune_full_on_conditioning
    from tta.inner_loop import finetune_lora_on_conditioning
    from tta.lora import get_lora_parameters, inject_lora_into_dit
    i = _inputs()
    dit = _dit()
    es = AnchoredEarlyStopper(check_every=1, patience=10)
    if method == "lora":
        for p in dit.parameters():
            p.requires_grad = False
        torch.manual_seed(3)
        mods = inject_lora_into_dit(dit, rank=8, alpha=16.0, target_modules=["qkv", "proj"], target_ffn=False, target_blocks="all")
        params = get_lora_parameters(mods)
        es.setup(dit, i["cond"], i["val"], i["embeds"], i["mask"], device=DEV, dtype=BF16, video_id="clip")
        torch.manual_seed(1234)
        res = finetune_lora_on_conditioning(dit, mods, i["cond"], i["train"], i["embeds"], i["mask"], num_steps=3, lr=2e-3,
                                            warmup_steps=1, weight_decay=0.01, max_grad_norm=1.0, device=DEV, dtype=BF16,
                                            early_stopper=es, **flag)
    else:
        for p in dit.parameters():
            p.requires_grad = True
        params = list(dit.parameters())
        es.setup(dit, i["cond"], i["val"], i["embeds"], i["mask"], device=DEV, dtype=BF16, video_id="clip")
        torch.manual_seed(1234)
        res = finetune_full_on_conditioning(dit, i["cond"], i["train"], i["embeds"], i["mask"], num_steps=3, lr=1e-3,
                                            warmup_steps=1, weight_decay=0.01, max_grad_norm=1.0, device=DEV, dtype=BF16,
                                            early_stopper=es, optimizer_type="sgd", **flag)
    torch.cuda.synchronize()
    assert res["early_stopping_info"]["total_checks"] == 4 and not dit.training
    return [float(v).hex() for v in res["losses"]], [p.detach().clone() for p in params], res


@pytest.mark.parametrize("method", ["lora", "full"])
def test_loops_flag_off_is_todays_run_and_flag_on_is_reproducible(method, deterministic, made):
    l0, w0, _ = _adapt(method)                                  # the keyword omitted
    l1, w1, _ = _adapt(method, master_weights=False)
    assert len(l0) == 3 and l0 == l1 and all(torch.equal(a, b) for a, b in zip(w0, w1))
    assert [o.master_weights for o in made] == [False, False] and all(o.low_words == [] for o in made)
    assert all(o.live_at_resync == [False] for o in made)      # called after the restore, nothing to do
    del made[:]
    la, wa, res = _adapt(method, master_weights=True)
    lb, wb, _ = _adapt(method, master_weights=True)
    assert all(np.isfinite(float.fromhex(v)) for v in la) and len(la) == 3
    assert la == lb and all(torch.equal(a, b) for a, b in zip(wa, wb))
    assert [o.master_weights for o in made] == [True, True]
    for o in made:
        assert o.live_at_resync == [True]                       # the steps had filled the low words; the restore dropped them
        assert len(o.low_words) == len(wa) and all(not lw.any() for lw in o.low_words)
    assert la[0] == l0[0]                                       # the first forward sees the same bf16 words either way


# ---------------------------------------------------------------------------------------------------------- 6. the runners
def _main(script, argv):
    spec = importlib.util.spec_from_file_location("mw_" + script[:-3], SCRIPTS / script)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    m.main(argv)


@pytest.mark.parametrize("script, extra", [
    ("run_lora_tta.py", ["--es-disable", "--lora-rank", "4", "--lora-alpha", "8"]),
    ("run_full_tta.py", ["--es-check-every", "2", "--es-patience", "1", "--learning-rate", "1e-4"]),
])
def test_runners_accept_master_weights(tmp_path, script, extra):
    out = tmp_path / "run"
    _main(script, ["--checkpoint-dir", "synthetic:2:256:64", "--data-dir", "synthetic:1", "--output-dir", str(out),
                   "--num-cond-frames", "5", "--num-frames", "13", "--gen-start-frame", "40", "--tta-total-frames", "33",
                   "--tta-context-frames", "9", "--num-steps", "4", "--num-inference-steps", "2", "--no-save-videos", "--master-weights"] + extra)
    cfg = json.loads((out / "config.json").read_text())
    assert cfg["training"]["master_weights"] is True
    s = json.loads((out / "summary.json").read_text())
    r = s["results"][0]
    assert s["num_videos"] == 1 and s["num_successful"] == 1 and r["success"] and r["final_loss"] == r["final_loss"]
    assert 1 <= r["num_train_steps"] <= 4

"""GPU: fp32 gradient accumulation over micro-steps (include/lcv_hip_accum.h, `grad_accum=N` / `--grad-accum N`).

1. lcv_grad_accumulate against the numpy restatement (tests/grad_accum_ref.py), bit for bit after every micro-step, through the
   raw ABI (N = 1 .. 4, one accumulator at a 4-byte offset) and through the optimizers.
2. Both fp32-gradient steps through the optimizers, bit for bit on the bf16 words, the low words and (AdamW) both moments after
   optimizer steps 1 and 3 of three micro-steps each, over the table of tests/test_gpu_master_weights.py: a single element, a
   sub-packet tail, an exact chunk, one element past a chunk (as a 2-byte offset view: the scalar path), a tail past two chunks,
   plus a parameter without a gradient.
3. Two equal micro-steps are one plain master-weight step; the accumulators keep what a bf16 `.grad` drops; refusals.
4. The loops (keyword omitted or 1: today's run; 2: reproducible, optimizer steps counted) and the runners.
"""
import importlib.util
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import grad_accum_ref as R
import master_weights_ref as W

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
SCRIPTS = ROOT / "longcat-video-tta_amd" / "lora_experiment" / "scripts"
BF16 = torch.bfloat16
DEV = "cuda"
NUMELS = (1, 7, 2048, 2049, 4099)
VIEW = 3                      # the 2049-element tensor is a [1:] view: pointers at a 2-byte offset
ACC_VIEW = 2                  # through the raw ABI the 2048-element tensor's accumulator is a [1:] fp32 view: a 4-byte offset
N_MICRO = 3                   # micro-steps per optimizer step in the step tests: the scale 1/3 is inexact
CHUNK = 2048


# ---------------------------------------------------------------------------------------------------------- helpers
def _bf16_dev(h):
    return torch.from_numpy(np.ascontiguousarray(h).view(np.int16).copy()).view(BF16).to(DEV)


def _i16_dev(low):
    return torch.from_numpy(np.ascontiguousarray(low, dtype=np.int16).copy()).to(DEV)


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


def _report(what, k, got, want):
    bad = np.flatnonzero(got != want)
    if bad.size:
        i = int(bad[0])
        raise AssertionError(f"{what}: tensor {k} (numel {got.size}) index {i}: got {got[i]!r} want {want[i]!r}; "
                             f"{bad.size} mismatches")


_TABLE = {}


def _table():
    """Host-generated inputs, made once: |w| in [2^-10, 2], |g| in [2^-20, 8], both signs - every intermediate is then a normal
    fp32 number.  Five tensors with a gradient for 3 optimizer steps x 4 micro-steps, and a sixth without one."""
    if not _TABLE:
        rng = np.random.default_rng(41)
        _TABLE["w"] = [W.weights(rng, n) for n in NUMELS + (300,)]
        _TABLE["g"] = [[[W.grads(rng, n) for n in NUMELS] for _ in range(4)] for _ in range(3)]
    return _TABLE


def _make(kind, wd, n, lows=True):
    from lcv_hip import ops
    t = _table()
    params = []
    for k, (h, _) in enumerate(t["w"]):
        p = _bf16_dev(h)
        params.append(_offset_view(p) if k == VIEW else p)
    if kind == "sgd":
        opt = ops.FusedSGDClip(params, lr=2e-3, weight_decay=wd, master_weights=True, grad_accum=n)
    else:
        opt = ops.FusedAdamWClip(params, lr=1e-3, betas=(0.9, 0.999), weight_decay=wd, eps=1e-8, master_weights=True,
                                 grad_accum=n)
    if lows:
        for lw, (_, low) in zip(opt.low_words, t["w"]):
            lw.copy_(_i16_dev(low))
    return opt, params


def _give_grads(params, gs):
    for k in range(len(NUMELS)):
        g = _bf16_dev(gs[k])
        params[k].grad = _offset_view(g) if k == VIEW else g


# ---------------------------------------------------------------------------------------------------------- 1. accumulate
@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_accumulate_bits(n):
    t = _table()
    scale = 1.0 / n
    # the raw ABI: a table of our own, one accumulator at a 4-byte offset
    grads = [_bf16_dev(g) for g in t["g"][0][0]]
    grads[VIEW] = _offset_view(grads[VIEW])
    accs = [torch.zeros(m, dtype=torch.float32, device=DEV) for m in NUMELS]
    accs[ACC_VIEW] = _offset_view(accs[ACC_VIEW])
    ref = [np.zeros(m, dtype=np.float32) for m in NUMELS]
    for micro in range(n):
        for k, g in enumerate(t["g"][0][micro]):
            grads[k].copy_(_bf16_dev(g))
        rows, chunk = [], 0
        for g, m in zip(grads, NUMELS):
            rows.append([0, g.data_ptr(), 0, 0, m, chunk])
            chunk += (m + CHUNK - 1) // CHUNK
        table = torch.tensor(rows, dtype=torch.int64).to(DEV)
        ptrs = torch.tensor([a.data_ptr() for a in accs], dtype=torch.int64).to(DEV)
        _call("lcv_grad_accumulate", table.data_ptr(), ptrs.data_ptr(), len(NUMELS), chunk, scale)
        torch.cuda.synchronize()
        for k in range(len(NUMELS)):
            ref[k] = R.accumulate(ref[k], t["g"][0][micro][k], scale)
            _report(f"raw accumulate N={n} micro-step {micro + 1}", k, _bits_of(accs[k]), W.bits(ref[k]))
    if n == 1:                  # scale 1 from zero: the widened gradient (the optimizers make no accumulators at 1)
        assert all(np.array_equal(r, W.bf16_to_f32(g)) for r, g in zip(ref, t["g"][0][0]))
        return
    # the optimizer: the same bits, the .grads dropped, the parameter without a gradient untouched
    opt, params = _make("sgd", 0.0, n)
    accs = opt.accumulated_grads()
    assert len(accs) == len(params) and all(a.dtype == torch.float32 and a.shape == p.shape and not a.any()
                                            for a, p in zip(accs, params))
    ref = [np.zeros(m, dtype=np.float32) for m in NUMELS]
    for micro in range(n):
        _give_grads(params, t["g"][0][micro])
        opt.accumulate()
        torch.cuda.synchronize()
        assert all(p.grad is None for p in params)
        for k in range(len(NUMELS)):
            ref[k] = R.accumulate(ref[k], t["g"][0][micro][k], scale)
            _report(f"accumulate() N={n} micro-step {micro + 1}", k, _bits_of(accs[k]), W.bits(ref[k]))
    assert not accs[-1].any()
    opt.zero_grad()
    assert all(not a.any() for a in opt.accumulated_grads())


# ---------------------------------------------------------------------------------------------------------- 2. the steps
def _run_steps(kind, clip, wd):
    """Three optimizer steps of N_MICRO micro-steps each on the GPU next to the restatement; compared after the first and the
    third."""
    opt, params = _make(kind, wd, N_MICRO)
    t = _table()
    ref = [dict(h=h.copy(), l=low.copy(), m=np.zeros(h.size, np.float32), v=np.zeros(h.size, np.float32)) for h, low in t["w"]]
    lows = opt.low_words
    n_total = sum(NUMELS)
    for step in range(3):
        opt.zero_grad()
        acc = [np.zeros(m, dtype=np.float32) for m in NUMELS]
        for micro in range(N_MICRO):
            _give_grads(params, t["g"][step][micro])
            opt.accumulate()
            acc = [R.accumulate(a, g, 1.0 / N_MICRO) for a, g in zip(acc, t["g"][step][micro])]
        coef = 1.0
        if clip:
            opt.clip_grad_norm_(1.0)
            norm, coef = (float(x) for x in opt._norm_coef.tolist())
            sumsq = sum(float(np.sum(a.astype(np.float64) ** 2)) for a in acc)
            rel = abs(norm * norm - sumsq) / sumsq
            print(f"{kind} step {step + 1}: norm {norm!r} float64 norm {sumsq ** 0.5!r} rel. error of the square {rel:.3e} "
                  f"bound {n_total * 2.0 ** -24:.3e} coef {coef!r}")
            assert 0.0 < coef < 1.0 and norm > 1.0            # the gradients are large: the coefficient is live
            assert rel <= n_total * 2.0 ** -24                # worst-case fp32 summation of n_total squares
        opt.step()
        torch.cuda.synchronize()
        for k in range(len(NUMELS)):
            r = ref[k]
            if kind == "sgd":
                r["h"], r["l"] = R.sgd_step_g32(r["h"], r["l"], acc[k], coef, 2e-3, wd)
            else:
                r["h"], r["l"], r["m"], r["v"] = R.adamw_step_g32(r["h"], r["l"], r["m"], r["v"], acc[k], coef, 1e-3, 0.9, 0.999,
                                                                  1e-8, wd, step + 1)
        if step in (0, 2):
            for k, r in enumerate(ref):
                _report(f"{kind} step {step + 1} h", k, _h_of(params[k]), r["h"])
                _report(f"{kind} step {step + 1} l", k, lows[k].cpu().numpy(), r["l"])
                if kind == "adamw":
                    _report(f"{kind} step {step + 1} exp_avg", k, _bits_of(opt.exp_avg[k]), W.bits(r["m"]))
                    _report(f"{kind} step {step + 1} exp_avg_sq", k, _bits_of(opt.exp_avg_sq[k]), W.bits(r["v"]))
    # the parameter without a gradient was skipped: its words are the table's, and so is its reference
    assert np.array_equal(ref[-1]["h"], t["w"][-1][0]) and np.array_equal(ref[-1]["l"], t["w"][-1][1])
    return [int((ref[k]["h"] != t["w"][k][0]).sum()) for k in range(len(NUMELS))]


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("clip", [False, True])
def test_sgd_g32_step_bits(clip, wd):
    moved = _run_steps("sgd", clip, wd)
    assert sum(moved) > 0


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("clip", [False, True])
def test_adamw_g32_step_bits(clip, wd):
    moved = _run_steps("adamw", clip, wd)
    assert sum(moved) > 0


# ---------------------------------------------------------------------------------------------------------- 3. properties
@pytest.mark.parametrize("kind", ["sgd", "adamw"])
def test_two_equal_micro_steps_are_one_plain_master_step(kind):
    """0.5 g + 0.5 g == g exactly, so the fp32-gradient step sees float(g): its outputs are the bf16-gradient step's bits."""
    t = _table()
    two, p2 = _make(kind, 0.01, 2)
    one, p1 = _make(kind, 0.01, 1)
    assert one.grad_accum == 1 and one.accumulated_grads() == []
    for _ in range(2):
        _give_grads(p2, t["g"][0][0])
        two.accumulate()
    _give_grads(p1, t["g"][0][0])
    two.step()
    one.step()
    torch.cuda.synchronize()
    for k in range(len(p1)):
        _report(f"{kind} h", k, _h_of(p2[k]), _h_of(p1[k]))
        _report(f"{kind} l", k, two.low_words[k].cpu().numpy(), one.low_words[k].cpu().numpy())
        if kind == "adamw":
            _report(f"{kind} exp_avg", k, _bits_of(two.exp_avg[k]), _bits_of(one.exp_avg[k]))
            _report(f"{kind} exp_avg_sq", k, _bits_of(two.exp_avg_sq[k]), _bits_of(one.exp_avg_sq[k]))
    assert any((_h_of(p1[k]) != t["w"][k][0]).any() for k in range(len(NUMELS)))     # and the step moved something


def test_fp32_accumulators_keep_what_a_bf16_grad_drops():
    from lcv_hip import ops
    n = 4099
    micro = [1.0, 2.0 ** -9, 2.0 ** -9, 2.0 ** -9]
    # what autograd does to a bf16 .grad: each addend is below half a bf16 ulp of 1.0 (2^-8) and vanishes
    bf = torch.zeros(n, dtype=BF16, device=DEV)
    for x in micro:
        bf += torch.full((n,), x, dtype=BF16, device=DEV)
    assert bool((bf == 1.0).all())
    p = torch.ones(n, dtype=BF16, device=DEV)
    opt = ops.FusedSGDClip([p], lr=1e-3, weight_decay=0.0, master_weights=True, grad_accum=4)
    for x in micro:
        p.grad = torch.full((n,), x, dtype=BF16, device=DEV)
        opt.accumulate()
    torch.cuda.synchronize()
    acc = opt.accumulated_grads()[0].cpu().numpy()
    assert np.array_equal(acc, np.full(n, 0.25 + 3 * 2.0 ** -11, dtype=np.float32))
    assert float(acc[0]) * 4 == 1.0 + 3 * 2.0 ** -9                                   # the exact mean, times N


def test_step_before_n_micro_steps_is_refused():
    from lcv_hip.lib import LcvError
    t = _table()
    for kind in ("sgd", "adamw"):
        opt, params = _make(kind, 0.0, 3)
        with pytest.raises(LcvError, match="0 of 3"):
            opt.step()
        _give_grads(params, t["g"][0][0])
        opt.accumulate()
        with pytest.raises(LcvError, match="1 of 3"):
            opt.clip_grad_norm_(1.0)
        with pytest.raises(LcvError, match="1 of 3"):
            opt.step()
        for micro in (1, 2):
            _give_grads(params, t["g"][0][micro])
            opt.accumulate()
        _give_grads(params, t["g"][0][3])
        with pytest.raises(LcvError, match="3 of 3"):                                  # a fourth micro-step has no place
            opt.accumulate()
        for p in params:
            p.grad = None
        opt.clip_grad_norm_(1.0)
        opt.step()
        opt.zero_grad()
        with pytest.raises(LcvError, match="0 of 3"):                                  # the count starts over
            opt.step()
        torch.cuda.synchronize()
        # no words moved for the parameter that never had a gradient
        assert np.array_equal(_h_of(params[-1]), t["w"][-1][0])


def test_bad_arguments_are_refused():
    from lcv_hip.lib import LcvError
    t = torch.zeros(8, dtype=torch.int64, device=DEV)
    for name, args in (("lcv_grad_accumulate", (None, t.data_ptr(), 1, 1, 1.0)),
                       ("lcv_grad_accumulate", (t.data_ptr(), None, 1, 1, 1.0)),
                       ("lcv_grad_accumulate", (t.data_ptr(), t.data_ptr(), 0, 1, 1.0)),
                       ("lcv_grad_accumulate", (t.data_ptr(), t.data_ptr(), 1, 0, 1.0)),
                       ("lcv_master_sgd_step_g32", (None, t.data_ptr(), 1, 1, None, 1e-3, 0.0)),
                       ("lcv_master_sgd_step_g32", (t.data_ptr(), None, 1, 1, None, 1e-3, 0.0)),
                       ("lcv_master_sgd_step_g32", (t.data_ptr(), t.data_ptr(), 0, 1, None, 1e-3, 0.0)),
                       ("lcv_master_sgd_step_g32", (t.data_ptr(), t.data_ptr(), 1, 0, None, 1e-3, 0.0)),
                       ("lcv_master_adamw_step_g32", (None, t.data_ptr(), 1, 1, None, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1)),
                       ("lcv_master_adamw_step_g32", (t.data_ptr(), None, 1, 1, None, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1)),
                       ("lcv_master_adamw_step_g32", (t.data_ptr(), t.data_ptr(), 0, 1, None, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1)),
                       ("lcv_master_adamw_step_g32", (t.data_ptr(), t.data_ptr(), 1, 0, None, 1e-3, 0.9, 0.999, 1e-8, 0.0, 1)),
                       ("lcv_master_adamw_step_g32", (t.data_ptr(), t.data_ptr(), 1, 1, None, 1e-3, 0.9, 0.999, 1e-8, 0.0, 0))):
        with pytest.raises(LcvError) as e:
            _call(name, *args)
        assert e.value.code == -1 and not e.value.fatal, name


# ---------------------------------------------------------------------------------------------------------- 4. the loops
_SHARED = {}


def _inputs():
    if not _SHARED:
        g = torch.Generator().manual_seed(7)
        r = lambda *s: torch.randn(*s, generator=g)
        _SHARED["cond"] = r(1, 16, 1, 10, 20).to(BF16).to(DEV)            # one conditioning latent frame: 5 x 10 tokens
        _SHARED["train"] = r(1, 16, 2, 10, 20).to(BF16).to(DEV)           # two target frames
        _SHARED["train2"] = r(1, 16, 2, 10, 20).to(BF16).to(DEV)          # a second video's, for the batch loop
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
def fed(monkeypatch):
    """The step indices the loops hand to their data feeds (`loss_at(i)` calls the feed with i)."""
    from tta import full_tta, inner_loop
    seen = []

    def recording(cls):
        class Recording(cls):
            def __call__(self, step):
                seen.append(step)
                return super().__call__(step)
        return Recording
    one, robin = recording(inner_loop._OneVideo), recording(inner_loop._RoundRobin)      # wrapped once, whoever imports them
    for mod in (inner_loop, full_tta):
        monkeypatch.setattr(mod, "_OneVideo", one)
        monkeypatch.setattr(mod, "_RoundRobin", robin)
    return seen


def _lora(dit):
    from tta.lora import get_lora_parameters, inject_lora_into_dit
    for p in dit.parameters():
        p.requires_grad = False
    torch.manual_seed(3)
    mods = inject_lora_into_dit(dit, rank=8, alpha=16.0, target_modules=["qkv", "proj"], target_ffn=False, target_blocks="all")
    return mods, get_lora_parameters(mods)


def _adapt(method, **flag):
    """Three optimizer steps from one seed on a fresh model with an early stopper that checks every step."""
    from tta.early_stopping import AnchoredEarlyStopper
    from tta.full_tta import finetune_full_on_conditioning
    from tta.inner_loop import finetune_lora_on_conditioning
    i = _inputs()
    dit = _dit()
    es = AnchoredEarlyStopper(check_every=1, patience=10)
    if method == "lora":
        mods, params = _lora(dit)
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
    # the stopper is driven by optimizer steps: its initial check and one per step, whatever the number of micro-steps
    assert res["early_stopping_info"]["total_checks"] == 4 and not dit.training
    return [float(v).hex() for v in res["losses"]], [p.detach().clone() for p in params], res


@pytest.mark.parametrize("method", ["lora", "full"])
def test_loops_at_one_are_todays_run_and_at_two_are_reproducible(method, deterministic, fed):
    l0, w0, _ = _adapt(method)                                  # the keyword omitted
    assert fed == [0, 1, 2]
    del fed[:]
    l1, w1, _ = _adapt(method, grad_accum=1)
    assert fed == [0, 1, 2]
    assert len(l0) == 3 and l0 == l1 and all(torch.equal(a, b) for a, b in zip(w0, w1))
    del fed[:]
    la, wa, _ = _adapt(method, master_weights=True, grad_accum=2)
    assert fed == [0, 1, 2, 3, 4, 5]                            # 2 x num_steps losses were computed ...
    lb, wb, _ = _adapt(method, master_weights=True, grad_accum=2)
    assert len(la) == 3 and all(np.isfinite(float.fromhex(v)) for v in la)       # ... and num_steps were logged
    assert la == lb and all(torch.equal(a, b) for a, b in zip(wa, wb))
    assert any(not torch.equal(a, b) for a, b in zip(wa, w0))                     # a different run from today's


def test_lora_batch_loop_puts_every_video_behind_each_update(deterministic, fed):
    from lcv_hip.lib import LcvError
    from tta.inner_loop import finetune_lora_batch
    i = _inputs()
    dit = _dit()
    mods, params = _lora(dit)
    start = [p.detach().clone() for p in params]
    batch = [dict(cond_latents=i["cond"], train_latents=tr, prompt_embeds=i["embeds"], prompt_mask=i["mask"])
             for tr in (i["train"], i["train2"])]
    torch.manual_seed(99)
    res = finetune_lora_batch(dit, mods, batch, num_steps=2, lr=2e-3, warmup_steps=1, weight_decay=0.01, max_grad_norm=1.0,
                              device=DEV, dtype=BF16, master_weights=True, grad_accum=2)
    torch.cuda.synchronize()
    assert fed == [0, 1, 2, 3] and [s % 2 for s in fed] == [0, 1, 0, 1]              # videos 0, 1 for every optimizer step
    assert len(res["losses"]) == 2 and all(np.isfinite(v) for v in res["losses"])
    assert any(not torch.equal(a, b) for a, b in zip(params, start))
    with pytest.raises(LcvError, match="needs master_weights=True"):
        finetune_lora_batch(dit, mods, batch, num_steps=1, device=DEV, dtype=BF16, grad_accum=2)


# ---------------------------------------------------------------------------------------------------------- 5. the runners
def _main(script, argv):
    spec = importlib.util.spec_from_file_location("ga_" + script[:-3], SCRIPTS / script)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    m.main(argv)


@pytest.mark.parametrize("script, extra", [
    ("run_lora_tta.py", ["--es-disable", "--lora-rank", "4", "--lora-alpha", "8"]),
    ("run_full_tta.py", ["--es-check-every", "2", "--es-patience", "1", "--learning-rate", "1e-4"]),
])
def test_runners_accept_grad_accum(tmp_path, script, extra):
    out = tmp_path / "run"
    _main(script, ["--checkpoint-dir", "synthetic:2:256:64", "--data-dir", "synthetic:1", "--output-dir", str(out),
                   "--num-cond-frames", "5", "--num-frames", "13", "--gen-start-frame", "40", "--tta-total-frames", "33",
                   "--tta-context-frames", "9", "--num-steps", "4", "--num-inference-steps", "2", "--no-save-videos",
                   "--master-weights", "--grad-accum", "2"] + extra)
    cfg = json.loads((out / "config.json").read_text())
    assert cfg["training"]["master_weights"] is True and cfg["training"]["grad_accum"] == 2
    s = json.loads((out / "summary.json").read_text())
    r = s["results"][0]
    assert s["num_videos"] == 1 and s["num_successful"] == 1 and r["success"] and r["final_loss"] == r["final_loss"]
    assert 1 <= r["num_train_steps"] <= 4

"""GPU: the fp32 weight average over the optimizer steps (include/lcv_hip_ema.h, `enable_weight_ema` / `weight_ema` /
`--weight-ema`).  Every comparison is exact: the kernels against the numpy restatement (tests/ema_ref.py), runs with the average
against runs without it.

1. lcv_master_ema_load / _update / _swap against the restatement, bit for bit, over the tensor table of
   test_gpu_decay_to_base.py: a single element, a sub-packet tail, 512, 513, an exact chunk, one element past a chunk (every array
   of it an offset view: the scalar path), a tail past two chunks, and a parameter that never gets a gradient; live low words.
2. A swap is an involution; beta = 0 copies the masters and writes nothing else.
3. Through the optimizers: the average follows the masters each step leaves, and the steps are the steps without it.
4. Guards and refusals.
5. The loops (the average is scored and generates, training goes on from the raw masters) and the runners.
"""
import importlib.util
import json

import numpy as np
import pytest
import torch

import ema_ref as E
import master_weights_ref as W
import test_gpu_decay_to_base as D

pytestmark = pytest.mark.gpu
BF16, DEV, CHUNK = D.BF16, D.DEV, D.CHUNK
NUMELS, VIEW = D.NUMELS + (D.IDLE,), D.VIEW
SENTINEL = 0x5A5A


# ---------------------------------------------------------------------------------------------------------- 1. the kernels
def _guarded(host, k):
    """A device copy with one element of sentinel behind it (and, for the offset tensor, one element of it in front)."""
    src = torch.from_numpy(np.ascontiguousarray(host).copy())
    lead = 1 if k == VIEW else 0
    whole = torch.full((src.numel() + lead + 1,), SENTINEL, dtype=src.dtype).to(DEV)
    view = whole[lead:lead + src.numel()]
    view.copy_(src.to(DEV))
    assert view.is_contiguous() and (view.data_ptr() % 16 != 0) == (k == VIEW)
    return view, whole


def _arrays():
    """(h, l, e) of every tensor of the table on the host, and guarded device copies.  The averages differ from the masters."""
    t = D._table()
    rng = np.random.default_rng(77)
    host, dev = [], []
    for k, (h, low) in enumerate(t["w"]):
        e = W.bits(W.log_uniform(rng, h.size, -10.0, 1.0)).copy()
        e[3::7] = W.join(h, low)[3::7]                                 # some elements already at their master
        host.append((h.copy(), low.copy(), e))
        dev.append((_guarded(h.view(np.int16), k), _guarded(low, k), _guarded(e.view(np.int32), k)))
    assert [h.size for h, _, _ in host] == list(NUMELS)
    return host, dev


def _launch(name, dev, *extra):
    rows, chunk = [], 0
    for (p, _), _, _ in dev:
        rows.append([p.data_ptr(), 0, 0, 0, p.numel(), chunk])
        chunk += (p.numel() + CHUNK - 1) // CHUNK
    table = torch.tensor(rows, dtype=torch.int64).to(DEV)
    lp = torch.tensor([x[1][0].data_ptr() for x in dev], dtype=torch.int64).to(DEV)
    ep = torch.tensor([x[2][0].data_ptr() for x in dev], dtype=torch.int64).to(DEV)
    assert chunk == 11
    D._call(name, table.data_ptr(), lp.data_ptr(), ep.data_ptr(), len(rows), chunk, *extra)
    torch.cuda.synchronize()


def _check(what, dev, want):
    """Every array of every tensor against (h, l, e bits), and nothing written in front of or behind any of them."""
    for k, (arrs, (h, low, e)) in enumerate(zip(dev, want)):
        (p, pw), (lw, lww), (ev, eww) = arrs
        D._report(what + " h", k, p.cpu().numpy().view(np.uint16), h)
        D._report(what + " l", k, lw.cpu().numpy(), low)
        D._report(what + " e", k, ev.cpu().numpy().view(np.uint32), e)
        for whole in (pw, lww, eww):
            edge = whole.cpu().numpy()
            assert edge[-1] == SENTINEL and (k != VIEW or edge[0] == SENTINEL), (what, k)


def test_load_bits():
    host, dev = _arrays()
    _launch("lcv_master_ema_load", dev)
    _check("load", dev, [(h, low, E.load(h, low)) for h, low, _ in host])
    assert all((E.load(h, low) != e).any() for h, low, e in host)                  # the averages were something else before


@pytest.mark.parametrize("beta", [0.0, 0.5, 0.9, 0.999])
def test_update_bits(beta):
    host, dev = _arrays()
    _launch("lcv_master_ema_update", dev, beta)
    want = [(h, low, E.update(h, low, e, beta)) for h, low, e in host]            # h and l are not written
    _check(f"update beta={beta}", dev, want)
    assert all((w[2] != e).any() for w, (_, _, e) in zip(want, host))
    if beta == 0.0:                                                               # the masters' bits, whatever the average was
        assert all(np.array_equal(w[2], W.join(h, low)) for w, (h, low, _) in zip(want, host))
    else:
        assert all((w[2] != W.join(h, low)).any() for w, (h, low, _) in zip(want, host) if h.size > 1)


def test_swap_bits():
    host, dev = _arrays()
    _launch("lcv_master_ema_swap", dev)
    want = [E.swap(h, low, e) for h, low, e in host]
    _check("swap", dev, want)
    for (h1, l1, e1), (h, low, e) in zip(want, host):                             # all three arrays are written
        assert (h1 != h).any() and (e1 != e).any() and (l1 != low).any() or h.size == 1
        assert np.array_equal(W.join(h1, l1), e)                                  # a valid master of the average


def test_swap_twice_restores_every_bit():
    host, dev = _arrays()
    _launch("lcv_master_ema_swap", dev)
    _launch("lcv_master_ema_swap", dev)
    _check("swap twice", dev, host)


def test_bad_arguments_are_refused_and_nothing_is_written():
    from lcv_hip.lib import LcvError
    host, dev = _arrays()
    t = torch.zeros(8, dtype=torch.int64, device=DEV).data_ptr()
    cases = []
    for name, tail in (("lcv_master_ema_load", ()), ("lcv_master_ema_swap", ()), ("lcv_master_ema_update", (0.5,))):
        for bad in range(3):                                                      # each pointer missing in turn: `ema` is the third
            ptrs = tuple(None if j == bad else t for j in range(3))
            cases.append((name, ptrs + (1, 1) + tail))
        cases += [(name, (t, t, t, 0, 1) + tail), (name, (t, t, t, 1, 0) + tail), (name, (t, t, t, 1, 2 ** 31) + tail)]
    cases += [("lcv_master_ema_update", (t, t, t, 1, 1, b)) for b in (1.0, float("nan"), -0.1, 1.5, float("inf"))]
    for name, args in cases:
        with pytest.raises(LcvError) as e:
            D._call(name, *args)
        assert e.value.code == -1 and not e.value.fatal, (name, args)
    # the same refusals over a real table: the buffers are what they were
    rows = [[dev[2][0][0].data_ptr(), 0, 0, 0, NUMELS[2], 0]]
    table = torch.tensor(rows, dtype=torch.int64).to(DEV)
    lp = torch.tensor([dev[2][1][0].data_ptr()], dtype=torch.int64).to(DEV)
    ep = torch.tensor([dev[2][2][0].data_ptr()], dtype=torch.int64).to(DEV)
    for name, args in (("lcv_master_ema_swap", (table.data_ptr(), lp.data_ptr(), None, 1, 1)),
                       ("lcv_master_ema_swap", (table.data_ptr(), lp.data_ptr(), ep.data_ptr(), 0, 1)),
                       ("lcv_master_ema_update", (table.data_ptr(), lp.data_ptr(), ep.data_ptr(), 1, 1, 1.0)),
                       ("lcv_master_ema_update", (table.data_ptr(), lp.data_ptr(), ep.data_ptr(), 1, 1, float("nan"))),
                       ("lcv_master_ema_load", (table.data_ptr(), None, ep.data_ptr(), 1, 1))):
        with pytest.raises(LcvError):
            D._call(name, *args)
    torch.cuda.synchronize()
    _check("after refusals", dev, host)


# ---------------------------------------------------------------------------------------------------------- 3. the optimizers
KINDS = [("sgd", 1, None), ("adamw", 1, None), ("adamw8", 1, None), ("adamw", D.N_MICRO, None), ("sgd", 1, "table")]


def _enable(opt, beta, warmup):
    """enable_weight_ema, then the offset tensor's average moved into an offset view like its other arrays."""
    opt.enable_weight_ema(beta, warmup)
    opt._ema[VIEW] = D._offset_view(opt._ema[VIEW])     # the average table is keyed on these pointers: it is built again
    opt.ema_reset()
    assert opt.ema_tensors()[VIEW].data_ptr() % 16 == 4


def _master_bits(opt):
    return [D._bits_of(m) for m in opt.master_tensors()]


@pytest.mark.parametrize("warmup", [False, True])
@pytest.mark.parametrize("kind, n, anchor", KINDS)
def test_the_average_follows_the_masters_and_the_steps_are_unchanged(kind, n, anchor, warmup):
    opt, params = D._make(kind, 0.01, n, anchor=anchor)
    plain, pp = D._make(kind, 0.01, n, anchor=anchor)
    assert plain.weight_ema is None and plain.ema_tensors() == []
    _enable(opt, 0.9, warmup)
    assert opt.weight_ema == 0.9 and len(opt.ema_tensors()) == len(params) and opt.ema_in_params is False
    assert all(e.dtype == torch.float32 and e.shape == p.shape for e, p in zip(opt.ema_tensors(), params))
    ref = _master_bits(opt)                                             # loaded from the masters, live low words included
    t = D._table()
    for k, (h, low) in enumerate(t["w"]):
        D._report("loaded", k, D._bits_of(opt.ema_tensors()[k]), W.join(h, low))
    for step in range(3):
        for o, ps in ((opt, params), (plain, pp)):
            D._feed(o, ps, step, n)
            if step == 1:
                o.clip_grad_norm_(1.0)
            o.step()
        torch.cuda.synchronize()
        masters = _master_bits(opt)
        beta = E.ema_beta(0.9, step + 1, warmup)
        assert beta == (0.9 if not warmup else [2 / 11, 3 / 12, 4 / 13][step])
        ref = [E.update(*W.split(m), e, beta) for m, e in zip(masters, ref)]
        for k, e in enumerate(ref):
            D._report(f"{kind} n={n} warmup={warmup} step {step + 1} average", k, D._bits_of(opt.ema_tensors()[k]), e)
    D._compare(kind, opt, params, plain, pp, f"{kind} n={n} against the run without the average")
    assert any((D._h_of(params[k]) != t["w"][k][0]).any() for k in range(len(D.NUMELS)))
    # the parameter without a gradient: its average never left its master
    D._report("idle", len(params) - 1, ref[-1], W.join(*t["w"][-1]))
    assert sum(int((e != m).sum()) for e, m in zip(ref[:-1], _master_bits(opt)[:-1])) > 0
    # ema_reset: back at the masters, and the schedule starts over
    opt.ema_reset()
    for k, m in enumerate(_master_bits(opt)):
        D._report("reset", k, D._bits_of(opt.ema_tensors()[k]), m)
    assert opt._ema_t == 0
    # resync leaves the average alone
    before = [D._bits_of(e) for e in opt.ema_tensors()]
    opt.resync()
    assert all(np.array_equal(a, D._bits_of(e)) for a, e in zip(before, opt.ema_tensors()))


def test_swap_through_the_optimizer_and_its_guards():
    from lcv_hip import ops
    from lcv_hip.lib import LcvError
    opt, params = D._make("adamw", 0.01, D.N_MICRO, anchor=None)
    _enable(opt, 0.5, False)
    D._feed(opt, params, 0, D.N_MICRO)
    opt.step()
    words = [(D._h_of(p).copy(), lw.cpu().numpy().copy(), D._bits_of(e)) for p, lw, e in zip(params, opt.low_words, opt.ema_tensors())]
    epoch = ops.PARAM_EPOCH
    opt.ema_swap()
    assert opt.ema_in_params is True and ops.PARAM_EPOCH == epoch + 1      # cached copies of the parameters are stale
    for k, (h, low, e) in enumerate(words):
        hh, ll, ee = E.swap(h, low, e)
        D._report("swapped h", k, D._h_of(params[k]), hh)
        D._report("swapped l", k, opt.low_words[k].cpu().numpy(), ll)
        D._report("swapped e", k, D._bits_of(opt.ema_tensors()[k]), ee)
    D._give_grads(params, D._table()["g"][1][0])
    for call in (opt.step, opt.accumulate, lambda: opt.clip_grad_norm_(1.0), opt.ema_reset):
        with pytest.raises(LcvError, match="ema_in_params"):
            call()
    opt.ema_swap()
    assert opt.ema_in_params is False
    for k, (h, low, e) in enumerate(words):
        D._report("back h", k, D._h_of(params[k]), h)
        D._report("back l", k, opt.low_words[k].cpu().numpy(), low)
        D._report("back e", k, D._bits_of(opt.ema_tensors()[k]), e)
    D._feed(opt, params, 1, D.N_MICRO)                                 # and training goes on
    opt.clip_grad_norm_(1.0)
    opt.step()
    with pytest.raises(LcvError, match="already called"):
        opt.enable_weight_ema(0.5)
    late, lp = D._make("sgd", 0.01)
    D._feed(late, lp, 0, 1)
    late.step()
    with pytest.raises(LcvError, match="before the first step"):
        late.enable_weight_ema(0.5)
    with pytest.raises(LcvError, match="needs master_weights=True"):
        D._make("sgd", 0.01, anchor=None, master=False)[0].enable_weight_ema(0.5)


# ---------------------------------------------------------------------------------------------------------- 5. the loops
deterministic = D.deterministic
_VAL = {}


def _val():
    if not _VAL:
        g = torch.Generator().manual_seed(8)
        _VAL["val"] = torch.randn(1, 16, 1, 10, 20, generator=g).to(BF16).to(DEV)     # one held-out frame for the early stopper
    return _VAL["val"]


METHODS = ["lora", "full_sgd", "full_adamw", "norm"]


def _adapt(method, steps=3, stopper=None, **flag):
    """`steps` optimizer steps from one seed on a fresh model; `stopper`: None, "real", or a callable params -> stopper."""
    from tta import delta as DL
    from tta.early_stopping import AnchoredEarlyStopper
    from tta.full_tta import finetune_full_on_conditioning
    from tta.inner_loop import finetune_lora_on_conditioning
    from tta.lora import get_lora_parameters, inject_lora_into_dit
    i = D._inputs()
    dit = D._dit()
    model = dit
    if method == "lora":
        for p in dit.parameters():
            p.requires_grad = False
        torch.manual_seed(3)
        mods = inject_lora_into_dit(dit, rank=8, alpha=16.0, target_modules=["qkv", "proj"], target_ffn=False, target_blocks="all")
        params = get_lora_parameters(mods)
    elif method == "norm":
        model = DL.NormTuneForward(dit, "all_norm").to(DEV)
        params = list(model.tuned_params)
    else:
        for p in dit.parameters():
            p.requires_grad = True
        params = list(dit.parameters())
    es = None
    if stopper == "real":
        es = AnchoredEarlyStopper(check_every=2, patience=10)
        es.setup(model, i["cond"], _val(), i["embeds"], i["mask"], device=DEV, dtype=BF16, video_id="clip")
    elif stopper is not None:
        es = stopper(params)
    torch.manual_seed(1234)
    data = (i["cond"], i["train"], i["embeds"], i["mask"])
    if method == "lora":
        res = finetune_lora_on_conditioning(dit, mods, *data, num_steps=steps, lr=2e-3, warmup_steps=1, weight_decay=0.01,
                                            max_grad_norm=1.0, device=DEV, dtype=BF16, early_stopper=es, **flag)
    elif method == "norm":
        res = DL.optimize_norm_params(model, params, *data, num_steps=steps, lr=1e-2, device=DEV, dtype=BF16, early_stopper=es,
                                      **flag)
    else:
        kind = method.split("_")[1]
        res = finetune_full_on_conditioning(dit, *data, num_steps=steps, lr=1e-3 if kind == "sgd" else 1e-4, warmup_steps=1,
                                            weight_decay=0.01, max_grad_norm=1.0, device=DEV, dtype=BF16, early_stopper=es,
                                            optimizer_type=kind, **flag)
    torch.cuda.synchronize()
    assert len(res["losses"]) == steps
    return [float(v).hex() for v in res["losses"]], [p.detach().clone() for p in params], res


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("method", METHODS)
def test_loops_without_the_keyword_are_todays_run(method, deterministic):
    for flag in ({}, {"master_weights": True}):
        l0, w0, _ = _adapt(method, **flag)
        l1, w1, _ = _adapt(method, weight_ema=None, **flag)
        assert l0 == l1 and _same(w0, w1), flag


@pytest.mark.parametrize("method", METHODS)
def test_average_at_beta_zero_is_the_last_iterate_and_at_point_nine_is_not(method, deterministic):
    l0, w0, _ = _adapt(method, master_weights=True)
    lz, wz, _ = _adapt(method, master_weights=True, weight_ema=0.0)
    assert lz == l0 and _same(wz, w0)                                   # the average is the last iterate
    la, wa, _ = _adapt(method, master_weights=True, weight_ema=0.9)
    assert la == l0 and not _same(wa, w0)                               # training never saw the average; generation does
    lw, ww, _ = _adapt(method, master_weights=True, weight_ema=0.9, ema_warmup=True)
    assert lw == l0 and not _same(ww, w0) and not _same(ww, wa)
    from lcv_hip.lib import LcvError
    with pytest.raises(LcvError, match="needs master_weights=True"):
        _adapt(method, weight_ema=0.9)


class _RecordingStopper:
    """Never stops; at each due check it clones the parameters it is shown; its restore is a no-op."""
    best_state = None
    state = None

    def __init__(self, params, check_every=2):
        self.params, self.check_every, self.seen = params, check_every, []

    def step(self, done, save_fn=None):
        if done % self.check_every == 0:
            save_fn()
            self.seen.append((done, [p.detach().clone() for p in self.params]))
        return False, {}

    def restore(self, restore_fn=None):
        pass


@pytest.fixture
def optimizers(monkeypatch):
    """The optimizers the loops switch an average on for, and how often each kind of call was made on them."""
    from lcv_hip import ops
    made, swaps = [], []
    enable, swap = ops.FusedAdamWClip.enable_weight_ema, ops.FusedAdamWClip.ema_swap
    monkeypatch.setattr(ops.FusedAdamWClip, "enable_weight_ema", lambda self, *a, **k: (made.append(self), enable(self, *a, **k))[1])
    monkeypatch.setattr(ops.FusedAdamWClip, "ema_swap", lambda self: (swaps.append(self.ema_in_params), swap(self))[1])
    return made, swaps


@pytest.mark.parametrize("method", ["lora", "full_sgd", "norm"])
def test_the_stopper_scores_the_average_and_training_goes_on_from_the_masters(method, deterministic, optimizers):
    made, swaps = optimizers
    flag = dict(master_weights=True, weight_ema=0.9)
    l2, w2, _ = _adapt(method, steps=2, **flag)                          # no stopper: ends with the average in the parameters
    l4, _, _ = _adapt(method, steps=4, **flag)
    assert swaps == [False, False] and all(o.ema_in_params for o in made)
    del swaps[:]
    holder = []
    ls, ws, res = _adapt(method, steps=4, stopper=lambda params: holder.append(_RecordingStopper(params)) or holder[0], **flag)
    seen = holder[0].seen
    assert [done for done, _ in seen] == [2, 4]
    assert _same(seen[0][1], w2)                                        # what was scored at step 2 is the 2-step average
    assert ls == l4 and ls[:2] == l2                                    # swapping in and out is exact
    assert swaps == [False, True, False, True]                          # in and out around each due check, none at the end
    assert not made[-1].ema_in_params and res["es_check_time"] > 0.0
    assert not _same(ws, seen[1][1])                                    # the run ended on the raw masters' words (a no-op restore)
    assert all(not lw.any() for lw in made[-1].low_words)               # ... which the final resync made the masters


@pytest.mark.parametrize("method", ["lora", "full_sgd"])
def test_with_the_real_stopper_the_run_completes_on_scored_words(method, deterministic, optimizers):
    made, swaps = optimizers
    losses, words, res = _adapt(method, steps=4, stopper="real", master_weights=True, weight_ema=0.9, ema_warmup=True)
    info = res["early_stopping_info"]
    assert info["total_checks"] == 3 and all(np.isfinite(float.fromhex(v)) for v in losses)
    assert swaps == [False, True, False, True] and len(made) == 1 and not made[0].ema_in_params
    assert all(not lw.any() for lw in made[0].low_words)                 # the restore wrote scored words, resync zeroed the rest
    assert len(made[0].ema_tensors()) == len(words)


def test_norm_tuning_refuses_the_average_beside_the_fp32_delta_vector():
    from tta import delta as DL
    i = D._inputs()
    w = DL.NormTuneForward(D._dit(), "all_norm", also_tune_delta=True).to(DEV)
    with pytest.raises(ValueError, match="weight_ema cannot train fp32 parameters"):
        DL.optimize_norm_params(w, w.tuned_params, i["cond"], i["train"], i["embeds"], i["mask"], num_steps=1, device=DEV, dtype=BF16,
                                master_weights=True, weight_ema=0.9)


def test_drift_norm_of_the_full_model_is_read_after_the_final_swap(deterministic):
    _, _, last = D._full(with_base=True, master_weights=True)
    _, _, zero = D._full(with_base=True, master_weights=True, weight_ema=0.0)
    _, _, avg = D._full(with_base=True, master_weights=True, weight_ema=0.9)
    assert zero["drift_norm"] == last["drift_norm"]                      # the average is the last iterate
    assert 0.0 < avg["drift_norm"] < last["drift_norm"]                  # an average that started at the base lags the iterate


# ---------------------------------------------------------------------------------------------------------- 6. the runners
def _main(rel, argv):
    path = D.PKG / rel
    spec = importlib.util.spec_from_file_location("ema_" + path.stem, path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    m.main(argv)


@pytest.mark.parametrize("rel, extra", [
    ("lora_experiment/scripts/run_lora_tta.py", ["--num-steps", "4", "--no-save-videos", "--es-check-every", "2", "--es-patience", "1",
                                                 "--lora-rank", "4", "--lora-alpha", "8"]),
    ("lora_experiment/scripts/run_full_tta.py", ["--num-steps", "4", "--learning-rate", "1e-4", "--no-save-videos", "--es-disable"]),
    ("delta_experiment/scripts/run_norm_tune_tta.py", ["--norm-steps", "4", "--norm-lr", "1e-2", "--es-check-every", "2",
                                                       "--es-patience", "1"]),
])
def test_runners_accept_weight_ema_and_write_the_keys_only_with_it(tmp_path, rel, extra):
    on, off = tmp_path / "on", tmp_path / "off"
    _main(rel, D.COMMON + extra + ["--output-dir", str(on), "--master-weights", "--weight-ema", "0.9", "--weight-ema-warmup"])
    _main(rel, D.COMMON + extra + ["--output-dir", str(off)])
    s_on, s_off = (json.loads((d / "summary.json").read_text()) for d in (on, off))
    for s in (s_on, s_off):
        assert s["num_videos"] == 1 and s["num_successful"] == 1 and s["results"][0]["success"]
    r_on, r_off = s_on["results"][0], s_off["results"][0]
    assert set(r_on) == set(r_off)
    assert r_on["final_loss"] == r_on["final_loss"]
    if "norm_tune" in rel:
        assert s_on["weight_ema"] == 0.9 and s_on["weight_ema_warmup"] is True
        assert set(s_on) - set(s_off) == {"master_weights", "weight_ema", "weight_ema_warmup"} and set(s_off) <= set(s_on)
    else:
        c_on, c_off = (json.loads((d / "config.json").read_text()) for d in (on, off))
        assert c_on["training"]["weight_ema"] == 0.9 and c_on["training"]["weight_ema_warmup"] is True
        assert set(c_on["training"]) - set(c_off["training"]) == {"weight_ema", "weight_ema_warmup"}
        assert set(c_off["training"]) <= set(c_on["training"]) and set(c_on) == set(c_off) and set(s_on) == set(s_off)

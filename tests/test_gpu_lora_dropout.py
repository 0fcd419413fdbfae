"""GPU: LoRA dropout (include/lcv_hip_lora.h) from the mask up to the runner.

Kernel shapes: M = 37 (no multiple of the 16-row workgroup nor of the 4-row wave), K = 520 (one ragged 512-wide lane
sweep) and 4096 (the real width), R in {1, 8, 32}, one strided x (ldx = K + 8), row0 in {0, 5, 2^33} (64-bit indexing at no
memory cost), p in {0.1, 0.5}.  The reference for every kernel is fp32 / fp64 torch with the mask of the numpy restatement
(tests/lora_dropout_ref.py) injected; the criterion for the bf16 outputs is the project's: no further from the fp32 result
than 1.5 x a bf16 torch restatement of the same formula, + 1e-3.  The contraction sums exact products in fp32: 1e-6 relative,
as lcv_tn_skinny.

Model for the checkpointing and inner-loop tests: a depth-2 DiT at hidden 256 (2 heads of 128), 2 latent frames of 4 x 4
tokens, adapters on qkv + proj, p = 0.1."""
import importlib.util
import json
from functools import partial
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lora_dropout_ref as R
from conftest import rel_l2
from oracle import dit_oracle as orc

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
RUNNER = ROOT / "longcat-video-tta_amd" / "lora_experiment" / "scripts" / "run_lora_tta.py"
BF16 = torch.bfloat16
DEV = "cuda"
M = 37
BIG = 1 << 33
# (K, R, p, row0, strided x)
CASES = [(520, 1, 0.1, 0, False), (520, 8, 0.5, 5, True), (520, 32, 0.1, BIG, False),
         (4096, 8, 0.1, 0, False), (4096, 32, 0.5, 5, False), (4096, 1, 0.5, BIG, False)]
SEED, OFFSET = (3 << 32) | 1234, (1 << 32) | 8          # both halves of seed and offset in use
_REF = {}


def _randn(*shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(BF16)


def _case(K, R_, p, row0, strided):
    """Inputs and the restated mask of one case, computed once and shared (never modified)."""
    key = (K, R_, p, row0, strided)
    if key not in _REF:
        x = _randn(M, K + 8 if strided else K, seed=K + R_)
        _REF[key] = dict(x=x[:, :K], A=_randn(R_, K, seed=K + R_ + 1, scale=K ** -0.5), g=_randn(M, 64, seed=K + R_ + 2),
                         dx=_randn(M, K, seed=K + R_ + 3),
                         mask=torch.from_numpy(R.mask(M, K, p, SEED, OFFSET, row0).astype(np.float32)),
                         scale=float(R.scale(p)))
    return _REF[key]


def _xd(c):
    """The dropped input with the kernels' rounding point: bf16(x * scale) where kept, 0 elsewhere."""
    return (c["x"].float() * c["scale"]).to(BF16) * c["mask"].to(BF16)


def _criterion(got, ref, restated, what):
    e, e_bf = rel_l2(got, ref), rel_l2(restated, ref)
    print(f"{what}: rel_l2 {e:.3e}, bf16 restatement {e_bf:.3e}")
    assert e < 1.5 * e_bf + 1e-3, (what, e, e_bf)


# ------------------------------------------------------------------------------------------------------------ 1. mask
@pytest.mark.parametrize("K, R_, p, row0, strided", CASES)
def test_mask_equals_the_restatement(K, R_, p, row0, strided):
    from lcv_hip import ops
    got = ops.lora_dropout_mask(M, K, p, SEED, OFFSET, row0)
    want = R.mask(M, K, p, SEED, OFFSET, row0)
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    assert 0 < want.sum() < want.size


def test_mask_rows_with_row0_are_a_slice_of_the_full_mask():
    from lcv_hip import ops
    full = ops.lora_dropout_mask(M, 520, 0.1, SEED, OFFSET)
    assert torch.equal(ops.lora_dropout_mask(20, 520, 0.1, SEED, OFFSET, row0=11), full[11:31])
    assert torch.equal(ops.lora_dropout_mask(3, 520, 0.1, SEED, OFFSET, row0=BIG + 2),
                       ops.lora_dropout_mask(5, 520, 0.1, SEED, OFFSET, row0=BIG)[2:])
    assert not torch.equal(ops.lora_dropout_mask(M, 520, 0.1, SEED, OFFSET + 4), full)
    assert not torch.equal(ops.lora_dropout_mask(M, 520, 0.1, SEED + 1, OFFSET), full)


@pytest.mark.parametrize("seed, offset, p", [(1234, 0, 0.1), (1234, 4, 0.5), (7, 8, 0.25)])
def test_mask_keep_rate(seed, offset, p):
    from lcv_hip import ops
    n = 256 * 4096
    q = 1 - R.threshold(p) / 65536
    kept = int(ops.lora_dropout_mask(256, 4096, p, seed, offset).sum(dtype=torch.int64).item())
    sigma = (n * q * (1 - q)) ** 0.5
    print(f"keep rate {(kept / n):.6f} vs {q:.6f}: {(kept - n * q) / sigma:+.2f} sigma")
    assert abs(kept - n * q) <= 4 * sigma


def test_bad_arguments_are_refused():
    from lcv_hip import ops
    from lcv_hip.lib import LcvError
    x, A = _randn(4, 16, seed=1).to(DEV), _randn(2, 16, seed=2).to(DEV)
    for p in (0.0, 1.0, -0.1, float("nan")):
        with pytest.raises(LcvError) as ei:
            ops.lora_down_dropout(x, A, 2.0, p, 1, 0)
        assert ei.value.code == -1
        with pytest.raises(LcvError):
            ops.lora_dropout_mask(4, 16, p, 1, 0)
    with pytest.raises(LcvError):
        ops.lora_dropout_mask(4, 12, 0.1, 1, 0)               # K % 8
    with pytest.raises(LcvError):
        ops.lora_dropout_mask(4, 16, 0.1, 1, 0, row0=-1)


# --------------------------------------------------------------------------------------------------------- 2. kernels
@pytest.mark.parametrize("K, R_, p, row0, strided", CASES)
def test_lora_down_dropout(K, R_, p, row0, strided):
    from lcv_hip import ops
    c = _case(K, R_, p, row0, strided)
    s = 2.0
    x = c["x"].to(DEV) if not strided else _strided(c["x"])
    assert x.stride(0) == (K + 8 if strided else K)
    h = ops.lora_down_dropout(x, c["A"].to(DEV), s, p, SEED, OFFSET, 64, row0)
    h2 = ops.lora_down_dropout(x, c["A"].to(DEV), s, p, SEED, OFFSET, 64, row0)
    assert torch.equal(h, h2)
    assert h.shape == (M, 64) and not h[:, R_:].any()
    ref = s * (c["x"].double() * c["mask"].double() * c["scale"]) @ c["A"].double().t()
    restated = (s * (_xd(c) @ c["A"].t())).to(BF16)
    _criterion(h[:, :R_], ref, restated, "lora_down_dropout")
    # given the mask, the kernel is lcv_lora_down on the dropped input
    assert torch.equal(h, ops.lora_down(_xd(c).to(DEV), c["A"].to(DEV), s))


def _strided(x):
    buf = torch.zeros(x.shape[0], x.shape[1] + 8, dtype=BF16, device=DEV)
    buf[:, :x.shape[1]].copy_(x)
    return buf[:, :x.shape[1]]


@pytest.mark.parametrize("K, R_, p, row0, strided", CASES)
def test_tn_skinny_dropout(K, R_, p, row0, strided):
    from lcv_hip import ops
    c = _case(K, R_, p, row0, strided)
    x = c["x"].to(DEV) if not strided else _strided(c["x"])
    g = c["g"].to(DEV)
    out = ops.tn_skinny_dropout(g, x, R_, p, SEED, OFFSET, scale=2.0, row0=row0)
    ref = 2.0 * c["g"][:, :R_].double().t() @ _xd(c).double()
    e = rel_l2(out, ref, bound=1.0e-6)
    print(f"tn_skinny_dropout: rel_l2 {e:.3e}")
    assert e < 1.0e-6
    was = ops.is_deterministic()
    try:
        for flag in (True, False):
            ops.set_deterministic(flag)
            assert torch.equal(out, ops.tn_skinny_dropout(g, x, R_, p, SEED, OFFSET, scale=2.0, row0=row0))
    finally:
        ops.set_deterministic(was)


@pytest.mark.parametrize("K, R_, p, row0, strided", CASES)
def test_lora_dx_dropout_add(K, R_, p, row0, strided):
    from lcv_hip import ops
    c = _case(K, R_, p, row0, strided)
    g = c["g"].to(DEV)
    g = g if not strided else _strided(g)                      # ldg = 72
    outs = [ops.lora_dx_dropout_add(c["dx"].to(DEV), g, c["A"].to(DEV), p, SEED, OFFSET, row0) for _ in range(2)]
    assert torch.equal(outs[0], outs[1])
    ga = c["g"][:, :R_].double() @ c["A"].double()
    ref = c["dx"].double() + c["mask"].double() * c["scale"] * ga
    restated = c["dx"] + (c["g"][:, :R_] @ c["A"]) * c["mask"].to(BF16) * torch.tensor(c["scale"]).to(BF16)
    _criterion(outs[0], ref, restated, "lora_dx_dropout_add")
    # a dropped element keeps its bits
    dropped = c["mask"] == 0
    assert torch.equal(outs[0].cpu()[dropped], c["dx"][dropped])


# ---------------------------------------------------------------------------------------------------------- 3. module
def _module(p, seed=5):
    from longcat_video.modules.layers import HipLinear
    from tta.lora import LoRALinear
    base = HipLinear(256, 384, device=DEV, dtype=BF16)
    with torch.no_grad():
        base.weight.copy_(_randn(384, 256, seed=seed, scale=256 ** -0.5))
        base.bias.copy_(_randn(384, seed=seed + 1, scale=0.1))
    base.weight.requires_grad_(False); base.bias.requires_grad_(False)
    lora = LoRALinear(base, rank=8, alpha=16.0, dropout=p).to(device=DEV, dtype=BF16)
    with torch.no_grad():
        lora.lora_down.weight.copy_(_randn(8, 256, seed=seed + 2, scale=256 ** -0.5))
        lora.lora_up.weight.copy_(_randn(384, 8, seed=seed + 3, scale=0.3))
    return lora


@pytest.fixture
def draws():
    from tta import lora as L
    seen = []
    L.DRAW_HOOK = lambda mod, seed, offset: seen.append((mod, seed, offset))
    yield seen
    L.DRAW_HOOK = None


def test_module_trains_with_dropout_and_matches_fp32_autograd(draws):
    """On the parent commit the forward raises LcvError("LoRA dropout > 0 is not fused ...")."""
    lora = _module(0.25).train()
    torch.manual_seed(11)
    x = _randn(M, 256, seed=31).to(DEV).requires_grad_(True)
    dy = _randn(M, 384, seed=32)
    y = lora(x)
    y.backward(dy.to(DEV))
    (mod, seed, offset), = draws
    assert mod is lora and seed == 11 and offset % 4 == 0
    mask = torch.from_numpy(R.mask(M, 256, 0.25, seed, offset).astype(np.float32))
    scale = float(R.scale(0.25))
    W, b = lora.original.weight.detach().cpu(), lora.original.bias.detach().cpu()
    A0, B0 = lora.lora_down.weight.detach().cpu(), lora.lora_up.weight.detach().cpu()

    def restate(dtype):
        xs, A_, B_ = (t.detach().cpu().to(dtype).requires_grad_(True) for t in (x, A0, B0))
        ms = (mask * scale).to(dtype) if dtype != BF16 else mask.to(dtype) * torch.tensor(scale).to(dtype)
        out = F.linear(xs, W.to(dtype), b.to(dtype)) + F.linear(F.linear(xs * ms, A_), B_) * lora.scaling
        out.backward(dy.to(dtype))
        return out.detach(), xs.grad, A_.grad, B_.grad
    ref, low = restate(torch.float64), restate(BF16)
    got = (y.detach(), x.grad, lora.lora_down.weight.grad, lora.lora_up.weight.grad)
    assert all(t is not None and torch.isfinite(t).all() for t in got)
    for name, a, r, l in zip(("y", "dx", "dA", "dB"), got, ref, low):
        _criterion(a, r, l, name)


def test_eval_is_the_dropout_free_module_bit_for_bit(draws, monkeypatch):
    from lcv_hip import ops
    names = []
    real = ops.call

    def recording(name, *args):
        names.append(name)
        return real(name, *args)
    monkeypatch.setattr(ops, "call", recording)
    x = _randn(M, 256, seed=41).to(DEV)
    dy = _randn(M, 384, seed=42).to(DEV)
    runs = []
    for p in (0.25, 0.0):
        lora = _module(p).eval()
        del names[:]
        xi = x.clone().requires_grad_(True)
        y = lora(xi)
        y.backward(dy)
        runs.append((list(names), y.detach(), xi.grad, lora.lora_down.weight.grad, lora.lora_up.weight.grad))
    assert not draws                                           # eval() draws nothing
    assert runs[0][0] == runs[1][0] and "lcv_lora_down" in runs[0][0] and not any("dropout" in n for n in runs[0][0])
    for a, b in zip(runs[0][1:], runs[1][1:]):
        assert torch.equal(a, b)
    # ... and in train() the new entry points are the ones that run
    lora = _module(0.25).train()
    del names[:]
    lora(x.clone().requires_grad_(True)).backward(dy)
    assert [n for n in names if "dropout" in n] == ["lcv_lora_down_dropout", "lcv_lora_dx_dropout_add", "lcv_tn_skinny_dropout"]


def test_offsets_advance_and_follow_manual_seed(draws):
    lora = _module(0.25).train()
    x = _randn(M, 256, seed=51).to(DEV)
    outs = []
    for _ in range(2):
        torch.manual_seed(77)
        outs.append([lora(x).detach() for _ in range(3)])
    first, second = [(s, o) for _, s, o in draws[:3]], [(s, o) for _, s, o in draws[3:]]
    assert first == second and len({o for _, o in first}) == 3 and all(s == 77 for s, _ in first)
    assert not torch.equal(outs[0][0], outs[0][1])             # another offset, another mask
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    torch.manual_seed(78)
    assert not torch.equal(lora(x).detach(), outs[0][0])


# --------------------------------------------------------------------------------- 4. checkpointing, 5. the inner loop
CFG = orc.small_config(hidden_size=256, depth=2, num_heads=2, caption_channels=64)
_SHARED = {}


def _inputs():
    if not _SHARED:
        g = torch.Generator().manual_seed(7)
        r = lambda *s: torch.randn(*s, generator=g)
        _SHARED["cond"] = r(1, 16, 1, 8, 8).to(BF16).to(DEV)              # one conditioning latent frame: 4 x 4 tokens
        _SHARED["train"] = r(1, 16, 1, 8, 8).to(BF16).to(DEV)             # one target frame
        _SHARED["embeds"] = r(1, 1, 12, 64).to(BF16).to(DEV)
        mask = torch.ones(1, 12, dtype=torch.int64)
        mask[0, 9:] = 0
        _SHARED["mask"] = mask.to(DEV)
        _SHARED["weights"] = orc.make_params(CFG, seed=3, std=0.05)
    return _SHARED


def _dit(p, up_seed=None):
    from longcat_video.modules.longcat_video_dit import LongCatVideoTransformer3DModel
    from tta.lora import inject_lora_into_dit
    m = LongCatVideoTransformer3DModel(device=DEV, dtype=BF16, hidden_size=256, depth=2, num_heads=2, caption_channels=64,
                                       adaln_tembed_dim=CFG["adaln_tembed_dim"])
    m.load_state_dict(_inputs()["weights"], strict=False)
    for q in m.parameters():
        q.requires_grad = False
    torch.manual_seed(3)                                       # the adapters' own initialisation
    mods = inject_lora_into_dit(m, rank=8, alpha=16.0, dropout=p, target_modules=["qkv", "proj"], target_ffn=False,
                                target_blocks="all")
    assert len(mods) == 10
    if up_seed is not None:                                    # a non-zero up-projection, so that the mask reaches the loss
        with torch.no_grad():
            for k, lm in enumerate(mods):
                lm.lora_up.weight.copy_(_randn(*lm.lora_up.weight.shape, seed=up_seed + k, scale=0.05))
    return m, mods


@pytest.fixture
def deterministic():
    from lcv_hip import ops
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    yield ops
    ops.set_deterministic(was)


def test_gradient_checkpointing_replays_the_masks(draws, deterministic):
    from torch.utils.checkpoint import checkpoint
    from tta.flow_matching import compute_flow_matching_loss_conditioned
    from tta.lora import get_lora_parameters
    i = _inputs()
    runs = []
    for ckpt in (False, True):
        dit, mods = _dit(0.1, up_seed=100)
        dit.train()
        dit.gradient_checkpointing = ckpt
        dit._gradient_checkpointing_func = partial(checkpoint, use_reentrant=False) if ckpt else None
        del draws[:]
        torch.manual_seed(21)
        loss = compute_flow_matching_loss_conditioned(dit=dit, cond_latents=i["cond"], target_latents=i["train"],
                                                      prompt_embeds=i["embeds"], prompt_mask=i["mask"], device=DEV, dtype=BF16)
        loss.backward()
        per_module = [[(s, o) for m_, s, o in draws if m_ is lm] for lm in mods]
        runs.append((loss.detach().clone(), [q.grad.clone() for q in get_lora_parameters(mods)], per_module))
    plain, ck = runs
    assert all(len(d) == 1 for d in plain[2])
    assert len({d[0] for d in plain[2]}) == 10                 # ten adapters, ten masks
    for first, again in zip(plain[2], ck[2]):
        assert len(again) == 2 and again[0] == again[1] == first[0], (first, again)   # forward + one recompute, same draw
    assert torch.equal(plain[0], ck[0])
    for a, b in zip(plain[1], ck[1]):
        assert a.abs().sum() > 0
        assert rel_l2(b, a) < 1e-3                             # the criterion with a reference that is its own restatement


def _adapt(p, seed, zero_p=False):
    from tta.inner_loop import finetune_lora_on_conditioning
    from tta.lora import get_lora_parameters
    i = _inputs()
    dit, mods = _dit(p)
    if zero_p:
        for lm in mods:
            lm.dropout.p = 0.0
    torch.manual_seed(seed)
    res = finetune_lora_on_conditioning(dit, mods, i["cond"], i["train"], i["embeds"], i["mask"], num_steps=3, lr=2e-3,
                                        warmup_steps=1, weight_decay=0.01, max_grad_norm=1.0, device=DEV, dtype=BF16)
    torch.cuda.synchronize()
    assert not dit.training                                    # the loop leaves the model in eval()
    return [float(v).hex() for v in res["losses"]], [q.detach().clone() for q in get_lora_parameters(mods)]


def test_inner_loop_same_seed_same_bits(draws, deterministic):
    l1, w1 = _adapt(0.1, 1234)
    assert len(draws) == 3 * 10 and len(l1) == 3
    l2, w2 = _adapt(0.1, 1234)
    assert l1 == l2 and all(torch.equal(a, b) for a, b in zip(w1, w2))
    l3, _ = _adapt(0.1, 4321)
    assert l3 != l1
    # p = 0 is today's path: nothing drawn, and the bits of an injection without dropout
    del draws[:]
    l0, w0 = _adapt(0.0, 1234)
    lz, wz = _adapt(0.1, 1234, zero_p=True)
    assert not draws
    assert l0 == lz and all(torch.equal(a, b) for a, b in zip(w0, wz))
    assert l0 != l1                                            # and the mask changes the run


# ---------------------------------------------------------------------------------------------------------- 6. runner
def test_runner_accepts_lora_dropout(tmp_path, draws):
    spec = importlib.util.spec_from_file_location("run_lora_tta_amd_dropout", RUNNER)
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    out = tmp_path / "run"
    m.main(["--checkpoint-dir", "synthetic:2:256:64", "--data-dir", "synthetic:1", "--output-dir", str(out), "--num-cond-frames", "5",
            "--num-frames", "13", "--gen-start-frame", "40", "--tta-total-frames", "33", "--tta-context-frames", "9", "--num-steps", "4",
            "--es-disable", "--num-inference-steps", "2", "--lora-rank", "4", "--lora-alpha", "8", "--lora-dropout", "0.1"])
    cfg = json.loads((out / "config.json").read_text())
    assert cfg["lora"]["dropout"] == 0.1 and cfg["lora"]["rank"] == 4
    s = json.loads((out / "summary.json").read_text())
    r = s["results"][0]
    assert s["num_successful"] == 1 and r["success"] and r["num_train_steps"] == 4 and r["final_loss"] == r["final_loss"]
    assert len(draws) >= 4 * 10                                # the mask was live in every step of every adapter

"""GPU: weight-decomposed LoRA (include/lcv_hip_dora.h, `LoRALinear(dora=True)`, `--lora-dora`).

1. lcv_dora_weight_norm against a float64 restatement on the same bf16 inputs, within the running-sum bound
   2 (K + 2R + 8) 2^-24 (any summation order; not a measured number), and bit for bit against tests/dora_ref.py; shapes at
   every K-tile (512) and rows-per-workgroup (16) edge of the kernel.
2. lcv_dora_colscale_fwd / _bwd bit for bit against tests/dora_ref.py, around the quarter (16) and slab (64) sizes and the issue's row counts.
3. The module against torch fp32 autograd of the formula with the norm detached, by the project's criterion
   e_hip < 1.5 e_bf16 + 1e-3; at B = 0, m = |W| a bias-free DoRA linear is plain LoRA bit for bit.
4. The cache of wn, 5. the inner loop, 6. the runner.
On the parent commit the kernel tests fail at symbol lookup and the others on the unknown argument."""
import importlib.util
import json
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dora_ref as D
import lora_dropout_ref as R
from conftest import rel_l2
from oracle import dit_oracle as orc

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]
RUNNER = ROOT / "longcat-video-tta_amd" / "lora_experiment" / "scripts" / "run_lora_tta.py"
BF16 = torch.bfloat16
DEV = "cuda"
U = 2.0 ** -24
_REF = {}


def _randn(*shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(BF16)


def _np(t):
    return t.detach().float().cpu().numpy()


def _bits(t):
    return _np(t).view(np.uint32)


# ---------------------------------------------------------------------------------------------------- 1. weight norm
S = 2.0
NORM_N = (1, 7, 15, 16, 17, 64, 130)           # the issue's rows, and 16 rows per workgroup +- 1
NORM_K = (64, 200, 504, 512, 520, 4104)        # the issue's widths, and the 512-column tile +- one packet
NORM_R = (1, 8, 32)


def _norm_case(K, R_):
    """Inputs of one (K, R) for the largest N, computed once and shared (never modified); smaller N are leading rows."""
    key = ("norm", K, R_)
    if key not in _REF:
        N = max(NORM_N)
        _REF[key] = dict(W=_randn(N, K, seed=K + R_), A=_randn(R_, K, seed=K + R_ + 1, scale=K ** -0.5),
                         B=_randn(N, R_, seed=K + R_ + 2, scale=0.1))       # s |B| |A| ~ 0.2 sqrt(R / K): well below |W| ~ 1
    return _REF[key]


@pytest.mark.parametrize("R_", NORM_R)
@pytest.mark.parametrize("K", NORM_K)
def test_weight_norm_within_the_running_sum_bound_and_bit_equal_to_the_restatement(K, R_):
    from lcv_hip import ops
    c = _norm_case(K, R_)
    Wd, Ad, Bd = (c[k].to(DEV) for k in "WAB")
    W64, A64, B64 = (c[k].double() for k in "WAB")
    exact = torch.linalg.vector_norm(W64 + S * (B64 @ A64), dim=1)
    restated = D.weight_norm(_np(c["W"]), _np(c["A"]), _np(c["B"]), S)
    bound = 2 * (K + 2 * R_ + 8) * U
    for N in NORM_N:
        got = ops.dora_weight_norm(Wd[:N].contiguous(), Ad, Bd[:N].contiguous(), S)
        again = ops.dora_weight_norm(Wd[:N].contiguous(), Ad, Bd[:N].contiguous(), S)
        assert got.shape == (N,) and got.dtype == torch.float32
        err = ((got.double().cpu() - exact[:N]).abs() / exact[:N]).max().item()
        print(f"N {N} K {K} R {R_}: max relative error {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (N, K, R_, err, bound)
        assert torch.equal(got, again)                                       # two calls, the same bits
        assert np.array_equal(_bits(got), restated[:N].view(np.uint32)), (N, K, R_)


@pytest.mark.parametrize("K", NORM_K)
def test_weight_norm_without_adapters_is_the_row_norm_and_equals_wn_at_zero_B(K):
    from lcv_hip import ops
    c = _norm_case(K, 8)
    Wd, Ad = c["W"].to(DEV), c["A"].to(DEV)
    exact = torch.linalg.vector_norm(c["W"].float().double(), dim=1)
    f32 = torch.linalg.vector_norm(Wd.float(), dim=1)
    bound = 2 * (K + 8) * U
    for N in NORM_N:
        m = ops.dora_weight_norm(Wd[:N].contiguous())
        assert ((m.double().cpu() - exact[:N]).abs() / exact[:N]).max().item() <= bound
        assert ((m - f32[:N]).abs() / f32[:N]).max().item() <= bound          # against torch's own fp32 sum, the same bound
        wn = ops.dora_weight_norm(Wd[:N].contiguous(), Ad, torch.zeros(N, 8, dtype=BF16, device=DEV), S)
        assert torch.equal(m, wn)                                            # c == 1 to the bit while B = 0
        wn = ops.dora_weight_norm(Wd[:N].contiguous(), Ad, torch.zeros(N, 8, dtype=BF16, device=DEV), -S)
        assert torch.equal(m, wn)
        assert np.array_equal(_bits(m), D.weight_norm(_np(c["W"][:N])).view(np.uint32))


def test_weight_norm_refuses_bad_arguments():
    from lcv_hip import lib
    from lcv_hip.lib import LcvError
    w = torch.zeros(16, 64, dtype=BF16, device=DEV)
    a = torch.zeros(4, 64, dtype=BF16, device=DEV)
    b = torch.zeros(16, 4, dtype=BF16, device=DEV)
    out = torch.zeros(16, dtype=torch.float32, device=DEV)
    ok = [w.data_ptr(), a.data_ptr(), b.data_ptr(), 1.0, 16, 64, 4, out.data_ptr(), None]
    lib.call("lcv_dora_weight_norm", *ok)
    bad = {"null w": (0, None), "null out": (7, None), "N < 1": (4, 0), "K < 1": (5, 0), "K % 8": (5, 60), "R = 0": (6, 0),
           "R = 33": (6, 33), "null a": (1, None), "w misaligned": (0, w.data_ptr() + 2), "a misaligned": (1, a.data_ptr() + 2)}
    for what, (slot, value) in bad.items():
        args = list(ok)
        args[slot] = value
        with pytest.raises(LcvError) as e:
            lib.call("lcv_dora_weight_norm", *args)
        assert e.value.code == -1, what
    torch.cuda.synchronize()


# --------------------------------------------------------------------------------------------------- 2. column scale
SCALE_M = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 513)  # a quarter (16) and a slab (64) of rows +- 1, the issue's row counts
SCALE_N = (8, 136, 4104)


def _scale_case(N):
    key = ("scale", N)
    if key not in _REF:
        M = max(SCALE_M)
        g = torch.Generator().manual_seed(N)
        wn = torch.rand(N, generator=g) + 0.5
        wn[N // 2] = 0.0                                                      # one dead row: c = 0 and dm = 0 there
        _REF[key] = dict(pre=_randn(M, N, seed=N + 1), dy=_randn(M, N, seed=N + 2), bias=_randn(N, seed=N + 3, scale=0.1),
                         m=torch.rand(N, generator=g) + 0.5, wn=wn)
    return _REF[key]


@pytest.mark.parametrize("N", SCALE_N)
def test_colscale_fwd_bits(N):
    from lcv_hip import ops
    c = _scale_case(N)
    m, wn, bias = c["m"].to(DEV), c["wn"].to(DEV), c["bias"].to(DEV)
    for M in SCALE_M:
        pre = c["pre"][:M].to(DEV)
        for b in (None, bias):
            want = D.colscale_fwd(_np(c["pre"][:M]), _np(c["m"]), _np(c["wn"]), None if b is None else _np(c["bias"]))
            y = ops.dora_colscale_fwd(pre, m, wn, b)
            assert y.dtype == BF16 and np.array_equal(_bits(y), want.view(np.uint32)), (M, N, b is not None)
            inplace = pre.clone()
            assert ops.dora_colscale_fwd(inplace, m, wn, b, out=inplace) is inplace      # y aliasing pre
            assert torch.equal(inplace, y)
        assert (y[:, N // 2].float() == bias[N // 2].float()).all()          # the dead row: c = 0, so y = bias


@pytest.mark.parametrize("N", SCALE_N)
def test_colscale_bwd_bits_and_dm_against_float64(N):
    from lcv_hip import ops
    c = _scale_case(N)
    m, wn = c["m"].to(DEV), c["wn"].to(DEV)
    live = _np(c["wn"]) != 0
    for M in SCALE_M:
        dy, pre = c["dy"][:M].to(DEV), c["pre"][:M].to(DEV)
        want_dpre, want_dm = D.colscale_bwd(_np(c["dy"][:M]), _np(c["pre"][:M]), _np(c["m"]), _np(c["wn"]))
        dpre, dm = ops.dora_colscale_bwd(dy, pre, m, wn)
        assert np.array_equal(_bits(dpre), want_dpre.view(np.uint32)), (M, N)
        assert np.array_equal(_bits(dm), want_dm.view(np.uint32)), (M, N)
        assert dm[N // 2].item() == 0.0 and (dpre[:, N // 2] == 0).all()
        # the only roundings are the M additions and the division: M 2^-24 of sum |dy pre| / wn
        prod = _np(c["dy"][:M]).astype(np.float64) * _np(c["pre"][:M]).astype(np.float64)
        wn64 = np.where(live, _np(c["wn"]).astype(np.float64), 1.0)
        exact, scale = prod.sum(0) / wn64, np.abs(prod).sum(0) / wn64
        err = (np.abs(_np(dm).astype(np.float64) - exact) / np.maximum(scale, 1e-300))[live].max()
        print(f"M {M} N {N}: dm error {err:.3e} of sum |dy pre| / wn, bound {M * U:.3e}")
        assert err <= M * U, (M, N, err)


def test_colscale_refuses_bad_arguments():
    from lcv_hip import lib
    from lcv_hip.lib import LcvError
    M, N = 3, 16
    pre = torch.zeros(M, N, dtype=BF16, device=DEV)
    dy, y, dpre = torch.zeros_like(pre), torch.zeros_like(pre), torch.zeros_like(pre)
    m, wn, dm = (torch.ones(N, dtype=torch.float32, device=DEV) for _ in range(3))
    ws_bytes = lib.load().lcv_dora_colscale_bwd_ws_bytes(M, N)
    assert ws_bytes == N * 4 and lib.load().lcv_dora_colscale_bwd_ws_bytes(65, N) == 2 * N * 4
    assert lib.load().lcv_dora_colscale_bwd_ws_bytes(0, N) < 0
    ws = torch.zeros(N, dtype=torch.float32, device=DEV)
    fwd = [pre.data_ptr(), m.data_ptr(), wn.data_ptr(), None, y.data_ptr(), M, N, None]
    bwd = [dy.data_ptr(), pre.data_ptr(), m.data_ptr(), wn.data_ptr(), dpre.data_ptr(), dm.data_ptr(), ws.data_ptr(), ws_bytes,
           M, N, None]
    lib.call("lcv_dora_colscale_fwd", *fwd)
    lib.call("lcv_dora_colscale_bwd", *bwd)
    cases = [("lcv_dora_colscale_fwd", fwd, s, v) for s, v in ((0, None), (1, None), (2, None), (4, None), (5, 0), (6, 0), (6, 12),
                                                               (0, pre.data_ptr() + 2), (4, y.data_ptr() + 8))]
    cases += [("lcv_dora_colscale_bwd", bwd, s, v) for s, v in ((0, None), (1, None), (2, None), (3, None), (4, None), (5, None),
                                                                (6, None), (7, ws_bytes - 4), (8, 0), (9, 0), (9, 12),
                                                                (4, pre.data_ptr()), (0, dy.data_ptr() + 2))]
    for name, ok, slot, value in cases:
        args = list(ok)
        args[slot] = value
        with pytest.raises(LcvError) as e:
            lib.call(name, *args)
        assert e.value.code == -1, (name, slot)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------- 3. module
TOK = 300


def _module(dora, p=0.0, bias=True, rank=4, seed=5, zero_up=False):
    from longcat_video.modules.layers import HipLinear
    from tta.lora import LoRALinear
    base = HipLinear(256, 384, bias=bias, device=DEV, dtype=BF16)
    with torch.no_grad():
        base.weight.copy_(_randn(384, 256, seed=seed, scale=256 ** -0.5))
        if bias:
            base.bias.copy_(_randn(384, seed=seed + 1, scale=0.1))
    for q in base.parameters():
        q.requires_grad_(False)
    kw = {"dora": True} if dora else {}
    lora = LoRALinear(base, rank=rank, alpha=2.0 * rank, dropout=p, **kw).to(device=DEV, dtype=BF16)
    with torch.no_grad():
        lora.lora_down.weight.copy_(_randn(rank, 256, seed=seed + 2, scale=256 ** -0.5))
        if not zero_up:
            lora.lora_up.weight.copy_(_randn(384, rank, seed=seed + 3, scale=0.3))
    return lora


def _criterion(got, ref, restated, what):
    e, e_bf = rel_l2(got, ref), rel_l2(restated, ref)
    print(f"{what}: rel_l2 {e:.3e}, bf16 restatement {e_bf:.3e}")
    assert e < 1.5 * e_bf + 1e-3, (what, e, e_bf)


@pytest.fixture
def draws():
    from tta import lora as L
    seen = []
    L.DRAW_HOOK = lambda mod, seed, offset: seen.append((mod, seed, offset))
    yield seen
    L.DRAW_HOOK = None


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("bias", [True, False])
def test_module_matches_fp32_autograd_of_the_formula(bias, p, draws):
    lora = _module(True, p=p, bias=bias).train()
    assert lora.dora_magnitude.dtype == torch.float32 and lora.lora_up.weight.dtype == BF16
    with torch.no_grad():                                                    # m != wn
        lora.dora_magnitude.mul_(torch.rand(384, generator=torch.Generator().manual_seed(9)).to(DEV) + 0.5)
    torch.manual_seed(11)
    x = _randn(TOK, 256, seed=31).to(DEV).requires_grad_(True)
    dy = _randn(TOK, 384, seed=32)
    y = lora(x)
    y.backward(dy.to(DEV))
    mask, scale = torch.ones(TOK, 256), 1.0
    if p:
        (mod, seed, offset), = draws
        mask, scale = torch.from_numpy(R.mask(TOK, 256, p, seed, offset).astype(np.float32)), float(R.scale(p))
    W = lora.original.weight.detach().cpu()
    b = lora.original.bias.detach().cpu() if bias else None
    A0, B0, m0 = (t.detach().cpu() for t in (lora.lora_down.weight, lora.lora_up.weight, lora.dora_magnitude))
    s = lora.scaling

    def restate(dtype):
        xs, A_, B_, m_ = (t.detach().cpu().to(dtype).requires_grad_(True) for t in (x, A0, B0, m0))
        ms = (mask * scale).to(dtype) if dtype != BF16 else mask.to(dtype) * torch.tensor(scale).to(dtype)
        Wd = W.to(dtype)
        pre = F.linear(xs, Wd) + F.linear(F.linear(xs * ms, A_), B_) * s
        wn = torch.linalg.vector_norm(Wd + s * (B_ @ A_), dim=1).detach()
        out = pre * (m_ / wn)
        if b is not None:
            out = out + b.to(dtype)
        out.backward(dy.to(dtype))
        return out.detach(), xs.grad, A_.grad, B_.grad, m_.grad
    ref, low = restate(torch.float32), restate(BF16)
    got = (y.detach(), x.grad, lora.lora_down.weight.grad, lora.lora_up.weight.grad, lora.dora_magnitude.grad)
    assert all(t is not None and torch.isfinite(t).all() for t in got)
    assert got[4].dtype == torch.float32
    for name, a, r, l in zip(("y", "dx", "dA", "dB", "dm"), got, ref, low):
        _criterion(a, r, l, name)


def test_at_zero_B_a_bias_free_dora_linear_is_plain_lora_bit_for_bit():
    x = _randn(TOK, 256, seed=41).to(DEV)
    dy = _randn(TOK, 384, seed=42).to(DEV)
    runs = []
    for dora in (False, True):
        lora = _module(dora, bias=False, zero_up=True).train()
        if dora:
            wn = lora.dora_weight_norm()
            assert torch.equal(wn, lora.dora_magnitude.detach())             # c == 1
        xi = x.clone().requires_grad_(True)
        y = lora(xi)
        y.backward(dy)
        runs.append((y.detach(), xi.grad, lora.lora_down.weight.grad, lora.lora_up.weight.grad))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


# ----------------------------------------------------------------------------------------------------------- 4. cache
@pytest.fixture
def calls(monkeypatch):
    """Names of the library calls, through the wrapper the optimizer call trace uses (tests/test_gpu_optim_call_trace.py)."""
    names = []
    for name in ("ops", "optim"):
        mod = __import__(f"lcv_hip.{name}", fromlist=[name])
        if not hasattr(mod, "call"):                                         # whichever module binds `call`
            continue
        real = mod.call

        def recording(entry, *args, _real=real):
            names.append((entry, torch.is_grad_enabled()))
            return _real(entry, *args)
        monkeypatch.setattr(mod, "call", recording)
    return names


def _norm_calls(calls):
    return sum(1 for n, _ in calls if n == "lcv_dora_weight_norm")


def test_wn_is_recomputed_when_an_adapter_changed_and_only_then(calls):
    from lcv_hip import ops
    from tta.early_stopping import ParamSnapshot
    from tta.lora import get_dora_magnitudes, get_lora_parameters, reset_lora_weights
    lora = _module(True).train()
    x = _randn(TOK, 256, seed=51).to(DEV)
    base = _norm_calls(calls)                                                # the magnitude's own initialisation
    assert base == 1

    def forwards_cost(n):
        before = _norm_calls(calls)
        for _ in range(2):
            lora(x)
        with torch.no_grad():
            lora(x)
        lora.eval(); lora(x); lora.train()
        assert _norm_calls(calls) - before == n
    forwards_cost(1)                                                         # the first forward computes it ...
    forwards_cost(0)                                                         # ... and nothing else does
    lora(x.clone().requires_grad_(True)).float().square().mean().backward()  # a backward changes nothing
    forwards_cost(0)
    params, mags = get_lora_parameters([lora]), get_dora_magnitudes([lora])
    opts = [ops.FusedAdamWClip(params, lr=1e-2, betas=(0.9, 0.999), weight_decay=0.0, eps=1e-8),
            ops.FusedAdamWClip(mags, lr=1e-2, betas=(0.9, 0.999), weight_decay=0.0, eps=1e-8)]
    snap = ParamSnapshot(params + mags).capture()
    wn0 = lora.dora_weight_norm().clone()
    ops.FusedAdamWClip.joint_clip_grad_norm_(opts, 1.0)
    for o in opts:
        o.step()                                                             # raw-pointer writes: PARAM_EPOCH
    forwards_cost(1)
    assert not torch.equal(lora.dora_weight_norm(), wn0)
    snap.write_back()                                                        # the stopper's restore
    forwards_cost(1)
    assert torch.equal(lora.dora_weight_norm(), wn0)
    with torch.no_grad():
        lora.lora_up.weight.copy_(_randn(384, 4, seed=77, scale=0.3))         # a direct copy_ into B
    forwards_cost(1)
    before = _norm_calls(calls)
    reset_lora_weights([lora])                                               # B = 0, m = |W| (one call for m) ...
    assert _norm_calls(calls) - before == 1
    forwards_cost(1)                                                         # ... and wn follows
    assert torch.equal(lora.dora_weight_norm(), lora.dora_magnitude.detach())


# ------------------------------------------------------------------------------------------------------ 5. inner loop
CFG = orc.small_config(hidden_size=256, depth=2, num_heads=2, caption_channels=64)
_SHARED = {}


def _inputs():
    if not _SHARED:
        g = torch.Generator().manual_seed(7)
        r = lambda *s: torch.randn(*s, generator=g)
        _SHARED["cond"] = r(1, 16, 1, 8, 8).to(BF16).to(DEV)
        _SHARED["train"] = r(1, 16, 1, 8, 8).to(BF16).to(DEV)
        _SHARED["embeds"] = r(1, 1, 12, 64).to(BF16).to(DEV)
        mask = torch.ones(1, 12, dtype=torch.int64)
        mask[0, 9:] = 0
        _SHARED["mask"] = mask.to(DEV)
        _SHARED["weights"] = orc.make_params(CFG, seed=3, std=0.05)
    return _SHARED


def _dit(**inject_kw):
    from longcat_video.modules.longcat_video_dit import LongCatVideoTransformer3DModel
    from tta.lora import inject_lora_into_dit
    m = LongCatVideoTransformer3DModel(device=DEV, dtype=BF16, hidden_size=256, depth=2, num_heads=2, caption_channels=64,
                                       adaln_tembed_dim=CFG["adaln_tembed_dim"])
    m.load_state_dict(_inputs()["weights"], strict=False)
    for q in m.parameters():
        q.requires_grad = False
    torch.manual_seed(3)
    mods = inject_lora_into_dit(m, rank=8, alpha=16.0, dropout=0.0, target_modules=["qkv", "proj"], target_ffn=False,
                                target_blocks="all", **inject_kw)
    assert len(mods) == 10
    return m, mods


def _adapt(seed, inject_kw, loop_kw):
    from tta.inner_loop import finetune_lora_on_conditioning
    from tta.lora import get_dora_magnitudes, get_lora_parameters
    i = _inputs()
    dit, mods = _dit(**inject_kw)
    mags = get_dora_magnitudes(mods)
    start = [q.detach().clone() for q in get_lora_parameters(mods) + mags]
    if loop_kw.get("dora_magnitudes") == "own":
        loop_kw = {**loop_kw, "dora_magnitudes": mags}
    torch.manual_seed(seed)
    res = finetune_lora_on_conditioning(dit, mods, i["cond"], i["train"], i["embeds"], i["mask"], num_steps=3, lr=2e-3,
                                        warmup_steps=1, weight_decay=0.01, max_grad_norm=1.0, device=DEV, dtype=BF16, **loop_kw)
    torch.cuda.synchronize()
    return ([float(v).hex() for v in res["losses"]], [q.detach().clone() for q in get_lora_parameters(mods) + mags], start,
            len(mags))


@pytest.fixture
def deterministic():
    from lcv_hip import ops
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    yield ops
    ops.set_deterministic(was)


def test_a_forward_recomputed_under_checkpointing_reuses_the_cached_norm(deterministic, calls):
    from functools import partial
    from torch.utils.checkpoint import checkpoint
    from tta.flow_matching import compute_flow_matching_loss_conditioned
    from tta.lora import get_dora_magnitudes, get_lora_parameters
    i = _inputs()
    runs = []
    for ckpt in (False, True):
        dit, mods = _dit(dora=True)
        with torch.no_grad():
            for k, lm in enumerate(mods):                                    # a non-zero up-projection: wn != m
                lm.lora_up.weight.copy_(_randn(*lm.lora_up.weight.shape, seed=100 + k, scale=0.05))
        dit.train()
        dit.gradient_checkpointing = ckpt
        dit._gradient_checkpointing_func = partial(checkpoint, use_reentrant=False) if ckpt else None
        del calls[:]
        torch.manual_seed(21)
        loss = compute_flow_matching_loss_conditioned(dit=dit, cond_latents=i["cond"], target_latents=i["train"],
                                                      prompt_embeds=i["embeds"], prompt_mask=i["mask"], device=DEV, dtype=BF16)
        loss.backward()
        fwd = sum(1 for c, _ in calls if c == "lcv_dora_colscale_fwd")
        runs.append((loss.detach().clone(), [q.grad.clone() for q in get_lora_parameters(mods) + get_dora_magnitudes(mods)],
                     _norm_calls(calls), fwd))
    plain, ck = runs
    assert plain[2] == ck[2] == 10 and plain[3] == 10 and ck[3] == 20        # forward + one recompute, one norm per adapter
    assert torch.equal(plain[0], ck[0])
    for a, b in zip(plain[1], ck[1]):
        assert a.abs().sum() > 0
        assert rel_l2(b, a) < 1e-3                                           # as tests/test_gpu_lora_dropout.py has it


def test_inner_loop_trains_adapters_and_magnitudes_and_repeats_bit_for_bit(deterministic, calls):
    l1, w1, w0, n_mag = _adapt(1234, {"dora": True}, {"dora_magnitudes": "own"})
    assert n_mag == 10 and len(l1) == 3 and all(np.isfinite(float.fromhex(v)) for v in l1)
    n = len(w1) - n_mag
    moved = [not torch.equal(a, b) for a, b in zip(w1, w0)]
    assert all(moved[:n]) and all(moved[n:]), moved                          # A, B and m all move
    assert all(t.dtype == torch.float32 for t in w1[n:]) and all(t.dtype == BF16 for t in w1[:n])
    assert sum(1 for c, _ in calls if c == "lcv_dora_colscale_bwd") == 3 * 10
    l2, w2, _, _ = _adapt(1234, {"dora": True}, {"dora_magnitudes": "own"})
    assert l1 == l2 and all(torch.equal(a, b) for a, b in zip(w1, w2))


def test_without_dora_the_loop_is_the_plain_one_call_for_call_and_bit_for_bit(deterministic, calls):
    runs = []
    for inject_kw, loop_kw in (({}, {}), ({"dora": False}, {"dora_magnitudes": None})):
        del calls[:]
        losses, weights, _, n_mag = _adapt(1234, inject_kw, loop_kw)
        assert n_mag == 0
        runs.append(([c for c, _ in calls], losses, weights))
    assert runs[0][0] == runs[1][0] and not any("dora" in c for c in runs[0][0])
    assert runs[0][1] == runs[1][1] and all(torch.equal(a, b) for a, b in zip(runs[0][2], runs[1][2]))


def test_inner_loop_refuses_what_the_magnitudes_optimizer_does_not_cover():
    from tta.inner_loop import finetune_lora_on_conditioning
    i = _inputs()
    dit, mods = _dit(dora=True)
    from tta.lora import get_dora_magnitudes
    mags = get_dora_magnitudes(mods)
    for kw in ({"master_weights": True}, {"master_weights": True, "moments_8bit": True}, {"master_weights": True, "grad_accum": 2},
               {"master_weights": True, "weight_ema": 0.9}, {"stochastic_rounding": True}):
        with pytest.raises(ValueError, match="DoRA"):
            finetune_lora_on_conditioning(dit, mods, i["cond"], i["train"], i["embeds"], i["mask"], num_steps=1, device=DEV,
                                          dtype=BF16, dora_magnitudes=mags, **kw)
    dit.enable_sequence_parallel(None)
    try:
        with pytest.raises(ValueError, match="sequence parallelism"):
            finetune_lora_on_conditioning(dit, mods, i["cond"], i["train"], i["embeds"], i["mask"], num_steps=1, device=DEV,
                                          dtype=BF16, dora_magnitudes=mags)
    finally:
        dit._sp_group = None


# ---------------------------------------------------------------------------------------------------------- 6. runner
def test_runner_accepts_lora_dora_and_generates_with_the_adapted_magnitudes(tmp_path, calls):
    spec = importlib.util.spec_from_file_location("run_lora_tta_amd_dora", RUNNER)
    m = importlib.util.module_from_spec(spec); spec.loader.exec_module(m)
    out = tmp_path / "run"
    m.main(["--checkpoint-dir", "synthetic:2:256:64", "--data-dir", "synthetic:1", "--output-dir", str(out), "--num-cond-frames", "5",
            "--num-frames", "13", "--gen-start-frame", "40", "--tta-total-frames", "33", "--tta-context-frames", "9", "--num-steps", "4",
            "--es-disable", "--num-inference-steps", "2", "--lora-rank", "4", "--lora-alpha", "8", "--lora-dora",
            "--save-lora-weights"])
    cfg = json.loads((out / "config.json").read_text())
    assert cfg["lora"]["dora"] is True and cfg["lora"]["rank"] == 4
    s = json.loads((out / "summary.json").read_text())
    r = s["results"][0]
    assert s["num_successful"] == 1 and r["success"] and r["num_train_steps"] == 4 and r["final_loss"] == r["final_loss"]
    assert sum(1 for c, _ in calls if c == "lcv_dora_colscale_bwd") >= 4 * 10
    assert r["gen_time"] > 0
    assert sum(1 for c, grad in calls if c == "lcv_dora_colscale_fwd" and not grad) >= 2 * 10      # the denoise runs the scale
    state = torch.load(next((out / "lora_weights").glob("*_lora.pt")))
    mags = [v for k, v in state.items() if k.endswith(".magnitude")]
    assert len(mags) == 10 and all(v.dtype == torch.float32 for v in mags) and f"lora_0.down" in state

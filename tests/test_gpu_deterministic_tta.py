"""GPU: "same seed, same bits" for every adaptation method in deterministic mode (lcv_hip.ops.set_deterministic /
LCV_DETERMINISTIC=1), end to end through the product's own loops.

Model: a depth-2 DiT at hidden 256 (2 heads of 128); 3 latent frames of 5 x 10 tokens (S = 50), the first one the
conditioning frame; three optimizer steps.  For each method, in deterministic mode, two runs from the same seed in one
process give bitwise-equal loss logs and bitwise-equal trainable parameters, and the first logged loss equals the default
mode's bitwise (the forward is untouched).  One case also runs as two fresh child processes with LCV_DETERMINISTIC=1: the
environment path, and an allocator that starts empty.  Nothing here asserts that the default mode differs between runs:
at these sizes it may not.

The LoRA case runs at r = 32, not 64: tta.lora.LoRALinear raises for a rank outside 1..32 ("for the fused kernels"), so
32 is the largest rank the product adapts at.
"""
import hashlib
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest
import torch

ROOT = Path(__file__).resolve().parents[1]
if __name__ == "__main__":                                  # the child process of the last test: conftest's path setup
    for p in (str(ROOT), str(ROOT / "longcat-video-tta_amd"), str(ROOT / "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)

from oracle import dit_oracle as orc  # noqa: E402

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
DEV = "cuda"
STEPS, SEED = 3, 1234
CFG = orc.small_config(hidden_size=256, depth=2, num_heads=2, caption_channels=64)
C, CT = CFG["hidden_size"], CFG["adaln_tembed_dim"]
CASES = ["lora_r32", "full_sgd", "full_adamw", "delta_a", "delta_b_timestep", "delta_b_hidden", "delta_c", "film_full",
         "norm_all", "norm_all_delta"]
_SHARED = {}


def _inputs():
    if not _SHARED:
        g = torch.Generator().manual_seed(7)
        r = lambda *s: torch.randn(*s, generator=g)
        _SHARED["cond"] = r(1, 16, 1, 10, 20).to(BF16).to(DEV)            # one conditioning latent frame: 5 x 10 tokens
        _SHARED["train"] = r(1, 16, 2, 10, 20).to(BF16).to(DEV)           # two target frames
        _SHARED["embeds"] = r(1, 1, 12, 64).to(BF16).to(DEV)
        mask = torch.ones(1, 12, dtype=torch.int64)
        mask[0, 9:] = 0
        _SHARED["mask"] = mask.to(DEV)
        _SHARED["weights"] = orc.make_params(CFG, seed=3, std=0.05)
    return _SHARED


def _dit():
    from longcat_video.modules.longcat_video_dit import LongCatVideoTransformer3DModel
    m = LongCatVideoTransformer3DModel(device=DEV, dtype=BF16, hidden_size=C, depth=CFG["depth"], num_heads=CFG["num_heads"],
                                       caption_channels=CFG["caption_channels"], adaln_tembed_dim=CT)
    m.load_state_dict(_inputs()["weights"], strict=False)
    return m


def run_case(name, steps=STEPS):
    """One adaptation run from SEED on a fresh model -> (loss log, trainable parameters after the last step)."""
    from tta import delta as D
    from tta.full_tta import finetune_full_on_conditioning
    from tta.inner_loop import finetune_lora_on_conditioning
    from tta.lora import get_lora_parameters, inject_lora_into_dit
    i = _inputs()
    data = (i["cond"], i["train"], i["embeds"], i["mask"])
    dit = _dit()
    torch.manual_seed(SEED)
    common = dict(num_steps=steps, device=DEV, dtype=BF16)
    if name == "lora_r32":
        for p in dit.parameters():
            p.requires_grad = False
        mods = inject_lora_into_dit(dit, rank=32, alpha=64.0, target_modules=["qkv", "proj"], target_ffn=False, target_blocks="all")
        params = get_lora_parameters(mods)
        res = finetune_lora_on_conditioning(dit, mods, *data, lr=2e-3, warmup_steps=1, weight_decay=0.01, max_grad_norm=1.0, **common)
    elif name.startswith("full_"):
        for p in dit.parameters():
            p.requires_grad = True
        params = list(dit.parameters())
        opt = name[len("full_"):]
        res = finetune_full_on_conditioning(dit, *data, lr=1e-3 if opt == "sgd" else 1e-4, warmup_steps=1, weight_decay=0.01,
                                            max_grad_norm=1.0, optimizer_type=opt, **common)
    elif name.startswith("norm_"):
        w = D.NormTuneForward(dit, "all_norm", also_tune_delta=name.endswith("_delta")).to(DEV)
        params = list(w.tuned_params)
        res = D.optimize_norm_params(w, w.tuned_params, *data, lr=1e-2, **common)
    else:
        if name == "delta_a":
            w, optimise = D.DeltaAWrapper(dit, adaln_tembed_dim=CT), D.optimize_delta_a
        elif name == "delta_b_timestep":
            w, optimise = D.DeltaBWrapper(dit, adaln_tembed_dim=CT, hidden_size=C, num_groups=2, delta_target="timestep"), D.optimize_delta_b
        elif name == "delta_b_hidden":
            w, optimise = D.DeltaBWrapper(dit, adaln_tembed_dim=CT, hidden_size=C, num_groups=2, delta_target="hidden",
                                          delta_dim=128), D.optimize_delta_b
        elif name == "delta_c":
            w, optimise = D.DeltaCWrapper(dit, "per_channel", CFG["out_channels"]), D.optimize_delta_c
        else:
            w, optimise = D.FiLMAdapterWrapper(dit, num_groups=2, hidden_size=C, film_mode="full"), D.optimize_film_adapter
        w = w.to(DEV)
        params = [p for p in w.parameters() if p.requires_grad]
        res = optimise(w, *data, lr=1e-2, **common)
    assert len(res["losses"]) == steps and params
    torch.cuda.synchronize()
    return [float(v) for v in res["losses"]], [p.detach().clone() for p in params]


def _digest(losses, params):
    h = hashlib.sha256()
    for p in params:
        h.update(p.detach().float().cpu().numpy().tobytes())
    return {"losses": [v.hex() for v in losses], "params": h.hexdigest(), "n": len(params)}


@pytest.fixture
def deterministic():
    from lcv_hip import ops
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    yield ops
    ops.set_deterministic(was)


@pytest.mark.parametrize("name", CASES)
def test_same_seed_same_bits(name, deterministic):
    ops = deterministic
    assert ops.is_deterministic()
    l1, p1 = run_case(name)
    l2, p2 = run_case(name)
    print(name, "losses", l1)
    assert [v.hex() for v in l1] == [v.hex() for v in l2], (l1, l2)
    assert len(p1) == len(p2)
    moved = 0
    for k, (a, b) in enumerate(zip(p1, p2)):
        assert torch.equal(a, b), f"{name}: trainable parameter {k} {tuple(a.shape)} differs between two runs of one seed"
        moved += int(bool(torch.isfinite(a).all()))
    assert moved == len(p1) and all(v == v for v in l1)
    assert l1[0] != l1[-1]                                   # the steps did something
    # the forward is untouched: the first logged loss is the default mode's, bit for bit
    ops.set_deterministic(False)
    l0, _ = run_case(name, steps=1)
    assert l0[0].hex() == l1[0].hex(), (l0, l1)


def test_environment_variable_in_two_fresh_processes():
    outs = []
    for _ in range(2):
        env = dict(os.environ, LCV_DETERMINISTIC="1")
        r = subprocess.run([sys.executable, str(Path(__file__).resolve()), "norm_all_delta"], env=env, capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        outs.append(json.loads(r.stdout.strip().splitlines()[-1]))
    assert outs[0]["deterministic"] is True
    assert outs[0] == outs[1], outs


if __name__ == "__main__":
    from lcv_hip import ops as _ops
    out = _digest(*run_case(sys.argv[1]))
    out["deterministic"] = _ops.is_deterministic()
    print(json.dumps(out))

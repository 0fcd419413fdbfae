#!/usr/bin/env python3
"""A/B of the deterministic mode on the full-model TTA step at the reference's operating point (480p: Tc=3 + Tt=1 latent
frames, 6 240 tokens, SGD, block checkpointing): `python tools/deterministic_ab.py [depth=48] [rounds=3] [steps=2] [out.md]`.

One process, one model.  After one warm-up step per mode the two modes alternate (default, deterministic, default, ...),
`rounds` times, `steps` optimizer steps each, so that clock and allocator drift hit both alike.  Step time is the loop's
own `train_time`; per-kernel time is the sum of HIP-event intervals around the six entry points that differ between the
modes (the interval of a call also holds whatever idle time precedes its kernels on the stream, the same in both modes).
The medians over the rounds, their spread and the ratio go to stdout and, as a markdown table, to `out.md`."""
import functools
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "longcat-video-tta_amd")); sys.path.insert(0, str(ROOT))
import torch  # noqa: E402
from torch.utils.checkpoint import checkpoint  # noqa: E402

from lcv_hip import lib, ops  # noqa: E402
from longcat_video.modules.longcat_video_dit import LongCatVideoTransformer3DModel  # noqa: E402
from tta.full_tta import finetune_full_on_conditioning  # noqa: E402

PAIRS = ["adaln_modulate_bwd", "layernorm_affine_bwd", "gate_residual_bwd", "qknorm_rope_bwd", "linear_f32_smallm_bwd",
         "grad_norm_clip"]
WATCH = {"lcv_" + n: n for n in PAIRS}
WATCH.update({"lcv_det_" + n: n for n in PAIRS})


def main():
    dev, bf = "cuda", torch.bfloat16
    depth = int(sys.argv[1]) if len(sys.argv) > 1 else 48
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 2
    out = Path(sys.argv[4]) if len(sys.argv) > 4 else None
    (h, w), (tc, tt) = (60, 104), (3, 1)
    dit = LongCatVideoTransformer3DModel(device=dev, dtype=bf, depth=depth).eval().init_synthetic_()
    dit.gradient_checkpointing = True
    dit._gradient_checkpointing_func = functools.partial(checkpoint, use_reentrant=False)
    for p in dit.parameters():
        p.requires_grad = True
    g = torch.Generator(device=dev).manual_seed(1)
    cond = torch.randn(1, 16, tc, h, w, device=dev, generator=g).to(bf)
    train = torch.randn(1, 16, tt, h, w, device=dev, generator=g).to(bf)
    pe = torch.randn(1, 1, 512, 4096, device=dev, generator=g).to(bf)
    pm = torch.zeros(1, 512, dtype=torch.int64, device=dev); pm[:, :77] = 1

    events = []
    real_call = ops.call

    def timed_call(name, *args):
        if name not in WATCH:
            return real_call(name, *args)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = real_call(name, *args)
        e1.record()
        events.append((WATCH[name], e0, e1))
        return r

    def run(det, n):
        ops.set_deterministic(det)
        events.clear()
        r = finetune_full_on_conditioning(dit, cond, train, pe, pm, num_steps=n, lr=1e-5, warmup_steps=0, device=dev, dtype=bf,
                                          optimizer_type="sgd")
        torch.cuda.synchronize()
        per = {k: 0.0 for k in PAIRS}
        calls = {k: 0 for k in PAIRS}
        for k, e0, e1 in events:
            per[k] += e0.elapsed_time(e1) / n
            calls[k] += 1
        return r["train_time"] / n, per, {k: v // n for k, v in calls.items()}

    ops.call = timed_call
    try:
        for det in (False, True):                       # warm-up: allocator, workspaces, kernel load
            run(det, 1)
        rows = {False: [], True: []}
        for _ in range(rounds):
            for det in (False, True):
                rows[det].append(run(det, steps))
    finally:
        ops.call = real_call
        ops.set_deterministic(False)

    med = lambda v: statistics.median(v)
    spread = lambda v: (max(v) - min(v)) / med(v) if med(v) else 0.0
    lines = [f"full-model TTA step, depth {depth}, 480p (6 240 tokens), SGD, block checkpointing; {rounds} interleaved rounds x {steps} steps, "
             f"library version {lib.load().lcv_version()}", "",
             "| quantity | calls / step | default (ms) | spread | deterministic (ms) | spread | ratio |", "|---|---|---|---|---|---|---|"]
    s0, s1 = [r[0] * 1e3 for r in rows[False]], [r[0] * 1e3 for r in rows[True]]
    lines.append(f"| step time | - | {med(s0):.1f} | {spread(s0):.1%} | {med(s1):.1f} | {spread(s1):.1%} | {med(s1) / med(s0):.4f} |")
    for k in PAIRS:
        a, b = [r[1][k] for r in rows[False]], [r[1][k] for r in rows[True]]
        n_calls = rows[True][0][2][k]
        ratio = f"{med(b) / med(a):.3f}" if med(a) else "-"
        lines.append(f"| `{k}` | {n_calls} | {med(a):.3f} | {spread(a):.1%} | {med(b):.3f} | {spread(b):.1%} | {ratio} |")
    ta, tb = [sum(r[1].values()) for r in rows[False]], [sum(r[1].values()) for r in rows[True]]
    lines.append(f"| the six together | - | {med(ta):.3f} | {spread(ta):.1%} | {med(tb):.3f} | {spread(tb):.1%} | {med(tb) / med(ta):.3f} |")
    text = "\n".join(lines)
    print(text, flush=True)
    if out is not None:
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text(text + "\n")


if __name__ == "__main__":
    main()

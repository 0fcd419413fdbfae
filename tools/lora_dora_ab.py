#!/usr/bin/env python3
"""Cost of DoRA (`--lora-dora`, include/lcv_hip_dora.h) on the LoRA inner step at the bench's LoRA-TTA shape (480p: Tc=3 + Tt=1
latent frames, 6 240 tokens, qkv + proj adapters, r = 8): `python tools/lora_dora_ab.py [depth=48] [rounds=3] [steps=3] [out.md]`.

One process, one model.
  1. The step with and without DoRA alternates `rounds` times after one warm-up run each, `steps` optimizer steps per run, so
     that clock and allocator drift hit both alike.  Step time is the loop's own `train_time` (host clock, ends in a device
     synchronise).
  2. The three kernels alone, at the shapes of the two self-attention adapters (qkv 12288 x 4096, proj 4096 x 4096, 6 240
     rows): call time from device events around `REPS` back-to-back launches that rotate over `SETS` buffer sets (together
     larger than the 256 MB last-level cache), after a warm-up pass over every set; achieved GB/s = the bytes the algorithm
     needs (counted here from the shapes) over that time.
Both tables go to stdout and, as markdown, to `out.md`."""
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "longcat-video-tta_amd")); sys.path.insert(0, str(ROOT))
import torch  # noqa: E402

from lcv_hip import lib, ops  # noqa: E402
from longcat_video.modules.longcat_video_dit import LongCatVideoTransformer3DModel  # noqa: E402
from tta import lora as L  # noqa: E402
from tta.inner_loop import choose_gradient_checkpointing, finetune_lora_on_conditioning  # noqa: E402

SETS, REPS, RANK = 4, 40, 8


def kernel_rows(tokens, dev):
    """(kernel, shape, bytes per call, median ms per call, GB/s) for the three kernels at the qkv and proj shapes."""
    bf, rows = torch.bfloat16, []
    g = torch.Generator(device=dev).manual_seed(2)

    def timed(calls):
        for c in calls:                                     # warm-up: every buffer set once
            c()
        torch.cuda.synchronize()
        per_call = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(REPS):
                calls[i % len(calls)]()
            b.record()
            torch.cuda.synchronize()
            per_call.append(a.elapsed_time(b) / REPS)
        return statistics.median(per_call)

    for name, N, K in (("qkv", 12288, 4096), ("proj", 4096, 4096)):
        Ws = [torch.randn(N, K, device=dev, generator=g).to(bf) for _ in range(SETS)]
        A = (torch.randn(RANK, K, device=dev, generator=g) * K ** -0.5).to(bf)
        B = (torch.randn(N, RANK, device=dev, generator=g) * 0.1).to(bf)
        out = torch.empty(N, dtype=torch.float32, device=dev)
        nbytes = N * K * 2 + -(-N // lib.LCV_DORA_NORM_ROWS) * RANK * K * 2 + N * RANK * 2 + N * 4
        ms = timed([lambda W=W: ops.dora_weight_norm(W, A, B, 2.0, out=out) for W in Ws])
        rows.append(("lcv_dora_weight_norm", f"{name}: N {N}, K {K}, R {RANK}", nbytes, ms))
        del Ws
        pres = [torch.randn(tokens, N, device=dev, generator=g).to(bf) for _ in range(SETS)]
        dys = [torch.randn(tokens, N, device=dev, generator=g).to(bf) for _ in range(SETS)]
        m, wn = torch.rand(N, device=dev, generator=g) + 0.5, torch.rand(N, device=dev, generator=g) + 0.5
        bias = torch.randn(N, device=dev, generator=g).to(bf)
        y = torch.empty_like(pres[0])
        ms = timed([lambda p=p: ops.dora_colscale_fwd(p, m, wn, bias, out=y) for p in pres])
        rows.append(("lcv_dora_colscale_fwd", f"{name}: M {tokens}, N {N}", 2 * tokens * N * 2 + N * 10, ms))
        slabs = -(-tokens // lib.LCV_DORA_SLAB)
        ms = timed([lambda p=p, d=d: ops.dora_colscale_bwd(d, p, m, wn) for p, d in zip(pres, dys)])
        rows.append(("lcv_dora_colscale_bwd", f"{name}: M {tokens}, N {N}", 3 * tokens * N * 2 + 2 * slabs * N * 4 + N * 16, ms))
        del pres, dys, y
    return rows


def main():
    dev, bf = "cuda", torch.bfloat16
    depth = int(sys.argv[1]) if len(sys.argv) > 1 else 48
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    steps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    out = Path(sys.argv[4]) if len(sys.argv) > 4 else None
    forms = [("LoRA", False), ("DoRA", True)]
    (h, w), (tc, tt) = (60, 104), (3, 1)
    dit = LongCatVideoTransformer3DModel(device=dev, dtype=bf, depth=depth).eval().init_synthetic_()
    for p in dit.parameters():
        p.requires_grad = False
    tokens = (tc + tt) * (h // 2) * (w // 2)
    ckpt = choose_gradient_checkpointing(dit, tokens)
    g = torch.Generator(device=dev).manual_seed(1)
    cond = torch.randn(1, 16, tc, h, w, device=dev, generator=g).to(bf)
    train = torch.randn(1, 16, tt, h, w, device=dev, generator=g).to(bf)
    pe = torch.randn(1, 1, 512, 4096, device=dev, generator=g).to(bf)
    pm = torch.zeros(1, 512, dtype=torch.int64, device=dev); pm[:, :77] = 1
    count = []

    def run(dora, n):
        torch.manual_seed(1234)
        mods = L.inject_lora_into_dit(dit, rank=RANK, alpha=16.0, dropout=0.0, target_modules=["qkv", "proj"], target_ffn=False,
                                      target_blocks="all", dora=dora)
        count[:] = [len(mods)]
        try:
            r = finetune_lora_on_conditioning(dit, mods, cond, train, pe, pm, num_steps=n, lr=2e-4, warmup_steps=0, device=dev,
                                              dtype=bf, dora_magnitudes=L.get_dora_magnitudes(mods) if dora else None)
            torch.cuda.synchronize()
        finally:
            L.remove_lora_from_dit(dit)
        return r["train_time"] / n

    for _, dora in forms:                               # warm-up: allocator, workspaces, kernel load
        run(dora, 1)
    times = {name: [] for name, _ in forms}
    for _ in range(rounds):
        for name, dora in forms:
            times[name].append(run(dora, steps) * 1e3)

    med = statistics.median
    base = med(times["LoRA"])
    lines = [f"`tools/lora_dora_ab.py` on {torch.cuda.get_device_name(0)}, library version {lib.load().lcv_version()}.", "",
             f"LoRA inner step, depth {depth}, 480p ({tokens} tokens), qkv + proj adapters ({count[0]} modules), r = {RANK}, block "
             f"checkpointing {'on' if ckpt else 'off'}; {rounds} interleaved rounds x {steps} steps after one warm-up run each.", "",
             "| form | step time (ms), median | min | max | spread | ratio to LoRA |", "|---|---|---|---|---|---|"]
    for name, _ in forms:
        v = times[name]
        lines.append(f"| {name} | {med(v):.1f} | {min(v):.1f} | {max(v):.1f} | {(max(v) - min(v)) / med(v):.1%} | {med(v) / base:.4f} |")
    lines += ["", f"The kernels alone: call time from device events around {REPS} back-to-back launches rotating over {SETS} buffer "
              "sets, median of 5 windows after a warm-up pass; bytes counted from the shapes (the norm: W once, A once per "
              "workgroup of 16 rows, B, wn; the forward scale: one read and one write of the output; the backward: two reads and "
              "one write, plus the slab partials written and read).", "",
              "| kernel | shape | MB per call | ms per call | GB/s |", "|---|---|---|---|---|"]
    for kernel, shape, nbytes, ms in kernel_rows(tokens, dev):
        lines.append(f"| {kernel} | {shape} | {nbytes / 1e6:.1f} | {ms:.4f} | {nbytes / ms / 1e6:.0f} |")
    text = "\n".join(lines)
    print(text, flush=True)
    if out is not None:
        out.parent.mkdir(parents=True, exist_ok=True)
        out.write_text(text + "\n")


if __name__ == "__main__":
    main()

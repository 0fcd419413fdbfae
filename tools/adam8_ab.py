#!/usr/bin/env python3
"""Step time of the 8-bit-moment AdamW step (lcv_master_adamw8_step, include/lcv_hip_moments8.h) against the fp32-moment step
(lcv_master_adamw_step): `python tools/adam8_ab.py [--large-mib 256] [--rounds 5] [--iters 20] [--out profiles/adam_8bit.md]`.

One process; both optimizers are built over the SAME parameter and gradient tensors (each keeps low words and moments of its
own), and their timings alternate `rounds` times after one warm-up call each, so that clock and allocator drift hit both alike.
A timing is `iters` back-to-back `step()` calls between two device events.  Two tables:
  large   8 tensors of `large-mib` Mi elements in all: HBM-bound, where the paper expectation is the byte ratio 26 / 14
  lora    the adapters of a 48-block DiT (qkv + proj, r = 8, hidden 4096: 192 tensors of 32 Ki to 96 Ki elements), where launch
          and table look-up dominate
The fp32-moment step is timed twice per round (its own repeat spread is the yardstick for any difference).  The result replaces
the "Step time" section of `--out`; the other sections of that file stay."""
import argparse
import statistics
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(HERE / "tools"))
FP32_BYTES, M8_BYTES = 26.0, 14.0 + 16.0 / 512            # streamed per parameter per step, read plus written


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--large-mib", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", type=Path, default=None)
    return ap.parse_args(argv)


def main(argv=None):
    args = parse(argv)
    sys.path.insert(0, str(HERE / "longcat-video-tta_amd")); sys.path.insert(0, str(HERE))
    import torch
    from adam8_quality import TIME_HEAD, replace_section
    from lcv_hip import lib, ops

    if not torch.cuda.is_available():
        raise SystemExit("adam8_ab: no GPU; a time measured anywhere else says nothing")
    dev, bf = "cuda", torch.bfloat16

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.iters):
            fn()
        b.record(); torch.cuda.synchronize()
        return a.elapsed_time(b) / args.iters * 1e3              # microseconds per step

    def measure(shapes):
        g = torch.Generator(device=dev).manual_seed(1)
        params = [(torch.randn(s, device=dev, generator=g) * 0.02).to(bf) for s in shapes]
        for p in params:
            p.grad = (torch.randn(p.shape, device=dev, generator=g) * 1e-3).to(bf)
        o32 = ops.FusedAdamWClip(params, lr=1e-5, master_weights=True)
        o8 = ops.FusedAdamWClip(params, lr=1e-5, master_weights=True, moments_8bit=True)
        for o in (o32, o8):
            o.step()
        torch.cuda.synchronize()
        t = {"fp32": [], "fp32 again": [], "8-bit": []}
        for _ in range(args.rounds):
            t["fp32"].append(timed(o32.step))
            t["8-bit"].append(timed(o8.step))
            t["fp32 again"].append(timed(o32.step))
        n = sum(p.numel() for p in params)
        return n, len(params), t, (o32.state_bytes(), o8.state_bytes())

    def rows(n, t):
        base = statistics.median(t["fp32"])
        out = []
        for name, nbytes in (("fp32", FP32_BYTES), ("fp32 again", FP32_BYTES), ("8-bit", M8_BYTES)):
            v = t[name]
            med = statistics.median(v)
            out.append([name, f"{med:.1f}", f"{min(v):.1f}", f"{max(v):.1f}", f"{(max(v) - min(v)) / med:.1%}", f"{med / base:.3f}",
                        f"{n * nbytes / med / 1e6:.2f}"])
        return out

    def table(title, header, body):
        return [title, "", "| " + " | ".join(header) + " |", "|" + "---|" * len(header)] + ["| " + " | ".join(r) + " |" for r in body] + [""]

    header = ["moments", "step (us), median", "min", "max", "spread", "ratio to fp32", "TB/s (algorithmic)"]
    lines = [f"`tools/adam8_ab.py` on {torch.cuda.get_device_name(0)}, library version {lib.load().lcv_version()}: {args.rounds} interleaved "
             f"rounds of {args.iters} back-to-back steps, one process, the same parameter and gradient tensors.  Spread = (max - min) / median.",
             f"Paper expectation at the large size: {M8_BYTES:.2f} / {FP32_BYTES:.0f} = {M8_BYTES / FP32_BYTES:.3f} of the fp32-moment step.", ""]
    verdicts = []
    per = args.large_mib * (1 << 20) // 8
    lora = [s for _ in range(48) for s in ((8, 4096), (3 * 4096, 8), (8, 4096), (4096, 8))]
    for title, shapes in ((f"Large table: 8 tensors of {per} elements", [(per,)] * 8), ("LoRA-sized table", lora)):
        n, k, t, (b32, b8) = measure(shapes)
        lines += table(f"{title} ({k} tensors, {n / 1e6:.2f} M elements; moments {b32 / 2 ** 20:.1f} MiB fp32, {b8 / 2 ** 20:.1f} MiB 8-bit)",
                       header, rows(n, t))
        m32, m8 = statistics.median(t["fp32"]), statistics.median(t["8-bit"])
        own = abs(statistics.median(t["fp32 again"]) - m32) / m32
        word = "SLOWER than" if m8 > m32 * (1 + own) else ("faster than" if m8 < m32 * (1 - own) else "within the repeat spread of")
        verdicts.append(f"{title}: the 8-bit step is {word} the fp32-moment step ({m8:.1f} us against {m32:.1f} us, ratio {m8 / m32:.3f}; "
                        f"the fp32-moment step's own repeat differs by {own:.1%}).")
        torch.cuda.empty_cache()
    lines += verdicts
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out is not None:
        replace_section(args.out, TIME_HEAD, text, "8-bit block-scaled AdamW moments (`--adam-8bit`)")


if __name__ == "__main__":
    main()

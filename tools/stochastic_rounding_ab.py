#!/usr/bin/env python3
"""Step time of the stochastic-rounding steps (lcv_sr_sgd_step, lcv_sr_adamw_step, include/lcv_hip_sr.h) against the plain bf16
steps (lcv_sgd_step, lcv_adamw_step) of another build of the library, normally the parent commit's:
`python tools/stochastic_rounding_ab.py --parent-lib PATH/liblcv_hip.so [--rounds 7] [--iters 50] [--out FILE.md]`.

One process; both libraries are loaded side by side and called through the C ABI over the SAME descriptor table, parameters,
gradients and moments, so the host path of every timed call is one ctypes call.  The timings alternate `rounds` times after a
warm-up call each; a timing is `iters` back-to-back calls between two device events.  The parent's plain step is timed twice per
round: its own repeat spread is the yardstick for any difference.  Two tables:
  lora    the adapters of a 48-block DiT at rank 8, hidden 4096 (self-attention qkv and proj, cross-attention q, kv and proj:
          480 tensors of 32 Ki to 96 Ki elements), where launch and table look-up weigh in
  large   one tensor of 4096 x 11008 = 45.1 M elements: HBM-bound
Algorithmic bytes per parameter, read + written: SGD 4 + 2 (both forms), AdamW 8 + 6 (both forms)."""
import argparse
import ctypes
import statistics
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parents[1]
CHUNK = 2048
BYTES = {"sgd": 6.0, "adamw": 14.0}


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--parent-lib", type=Path, required=True, help="liblcv_hip.so of the build whose plain bf16 steps are the baseline")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", type=Path, default=None)
    return ap.parse_args(argv)


def main(argv=None):
    args = parse(argv)
    sys.path.insert(0, str(HERE / "longcat-video-tta_amd")); sys.path.insert(0, str(HERE))
    import torch
    from lcv_hip import lib

    if not torch.cuda.is_available():
        raise SystemExit("stochastic_rounding_ab: no GPU; a time measured anywhere else says nothing")
    dev, bf = "cuda", torch.bfloat16
    new = lib.load()
    old = ctypes.CDLL(str(args.parent_lib.resolve()))
    old.lcv_version.restype = ctypes.c_int
    for name in ("lcv_sgd_step", "lcv_adamw_step"):
        fn = getattr(old, name)
        fn.restype, fn.argtypes = ctypes.c_int, lib._SIGNATURES[name]
    stream = torch.cuda.current_stream().cuda_stream

    def check(rc, what):
        if rc != 0:
            raise SystemExit(f"stochastic_rounding_ab: {what} returned {rc}")

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.iters):
            fn()
        b.record(); torch.cuda.synchronize()
        return a.elapsed_time(b) / args.iters * 1e3              # microseconds per step

    def measure(shapes):
        g = torch.Generator(device=dev).manual_seed(1)
        p = [(torch.randn(s, device=dev, generator=g) * 0.02).to(bf) for s in shapes]
        gr = [(torch.randn(s, device=dev, generator=g) * 1e-3).to(bf) for s in shapes]
        m = [torch.zeros_like(t) for t in p]
        v = [torch.zeros_like(t) for t in p]
        rows, chunk = [], 0
        for t, tg, tm, tv in zip(p, gr, m, v):
            rows.append([t.data_ptr(), tg.data_ptr(), tm.data_ptr(), tv.data_ptr(), t.numel(), chunk])
            chunk += (t.numel() + CHUNK - 1) // CHUNK
        desc = torch.tensor(rows, dtype=torch.int64).to(dev)
        d, n = desc.data_ptr(), len(rows)
        count = [0]

        def offset():                                            # a fresh counter per call, as the optimizer's draw gives
            count[0] += 4
            return count[0]
        calls = {
            ("sgd", "plain, parent"): lambda: check(old.lcv_sgd_step(d, n, chunk, 0, None, 1e-5, 0.01, stream), "lcv_sgd_step"),
            ("sgd", "plain, this tree"): lambda: check(new.lcv_sgd_step(d, n, chunk, 0, None, 1e-5, 0.01, stream), "lcv_sgd_step"),
            ("sgd", "SR"): lambda: check(new.lcv_sr_sgd_step(d, n, chunk, None, 1e-5, 0.01, 7, offset(), stream), "lcv_sr_sgd_step"),
            ("adamw", "plain, parent"): lambda: check(old.lcv_adamw_step(d, n, chunk, 0, None, 2e-4, 0.9, 0.999, 1e-8, 0.01, 3, stream),
                                                      "lcv_adamw_step"),
            ("adamw", "plain, this tree"): lambda: check(new.lcv_adamw_step(d, n, chunk, 0, None, 2e-4, 0.9, 0.999, 1e-8, 0.01, 3, stream),
                                                         "lcv_adamw_step"),
            ("adamw", "SR"): lambda: check(new.lcv_sr_adamw_step(d, n, chunk, None, 2e-4, 0.9, 0.999, 1e-8, 0.01, 3, 7, offset(), stream),
                                           "lcv_sr_adamw_step"),
        }
        out = {}
        for kind in ("sgd", "adamw"):
            forms = ["plain, parent", "SR", "plain, this tree", "plain, parent again"]
            fns = {f: calls[kind, f.replace(" again", "")] for f in forms}
            for f in forms:
                fns[f]()
            torch.cuda.synchronize()
            t = {f: [] for f in forms}
            for _ in range(args.rounds):
                for f in forms:
                    t[f].append(timed(fns[f]))
            out[kind] = t
        return sum(t.numel() for t in p), n, out

    def table(title, header, body):
        return [title, "", "| " + " | ".join(header) + " |", "|" + "---|" * len(header)] + ["| " + " | ".join(r) + " |" for r in body] + [""]

    header = ["step", "form", "step (us), median", "min", "max", "spread", "ratio to parent's plain", "TB/s (algorithmic)"]
    lines = [f"`tools/stochastic_rounding_ab.py` on {torch.cuda.get_device_name(0)}: this tree's library (version {new.lcv_version()}) and "
             f"the parent's (version {old.lcv_version()}) in one process, the same table and tensors, {args.rounds} interleaved rounds of "
             f"{args.iters} back-to-back calls between device events.  Spread = (max - min) / median.", ""]
    verdicts = []
    block = [(8, 4096), (3 * 4096, 8), (8, 4096), (4096, 8), (8, 4096), (4096, 8), (8, 4096), (2 * 4096, 8), (8, 4096), (4096, 8)]
    for title, shapes in (("LoRA table", block * 48), ("One large tensor", [(4096, 11008)])):
        nel, k, res = measure(shapes)
        body = []
        for kind, t in res.items():
            base = statistics.median(t["plain, parent"])
            for form, vals in t.items():
                med = statistics.median(vals)
                body.append([kind, form, f"{med:.1f}", f"{min(vals):.1f}", f"{max(vals):.1f}", f"{(max(vals) - min(vals)) / med:.1%}",
                             f"{med / base:.3f}", f"{nel * BYTES[kind] / med / 1e6:.2f}"])
            sr, own = statistics.median(t["SR"]), abs(statistics.median(t["plain, parent again"]) - base) / base
            word = "SLOWER than" if sr > base * (1 + own) else ("faster than" if sr < base * (1 - own) else "within the repeat spread of")
            verdicts.append(f"{title}, {kind}: the SR step is {word} the parent's plain bf16 step ({sr:.1f} us against {base:.1f} us, ratio "
                            f"{sr / base:.3f}; the plain step's own repeat differs by {own:.1%}).")
        lines += table(f"{title} ({k} tensors, {nel / 1e6:.2f} M elements)", header, body)
        torch.cuda.empty_cache()
    lines += verdicts
    text = "\n".join(lines)
    print(text, flush=True)
    if args.out is not None:
        args.out.parent.mkdir(parents=True, exist_ok=True)
        args.out.write_text(text + "\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Cost and self-consistency of the guidance reuse of the CFG denoise loop (`cfg_reuse=` / `--cfg-reuse`,
include/lcv_hip_cfgreuse.h): `python tools/cfg_reuse_ab.py [--parent TREE] [--rounds 5] [--only regs,kernel,steps,flagoff,consist]
[--out profiles/cfg_reuse.md]`.

Five sections (the helpers and the flag-off method are those of tools/solver_ab.py):
  regs      the kernels' register counts, scratch and LDS, read from the device assembly that the library's own recipe
            (lcv_hip/build.py) gives for csrc/cfg_reuse.hip; needs no GPU
  kernel    lcv_cfg_delta_store and lcv_cfg_delta_apply alone over the flagship latent ([1, 16, 13, 90, 160] fp32 per operand),
            every form the loop calls, device events around each call; achieved bytes / s from the bytes per element the header
            states
  steps     the first steps of the flagship denoise (49 x 720p, depth 48, CFG) under `cfg_reuse=2` in one process: wall time of
            the full (batch 2) and of the reuse (batch 1) steps from a synchronise in the step callback; the ratio is reported,
            not asserted
  flagoff   `bench.py --gpus 1` with the flag absent in this tree and in `--parent TREE` (a checkout of the parent commit with its
            own built library), alternating rounds: the parent's own run-to-run range is the yardstick for this tree's median
  consist   self-consistency on the random-init real architecture at a small size (1 280 tokens, shallow depth): the relative L2
            of the final latents under K = 2, 3, 5 against K = 1, and the drift trace K = 1 records
Every leg is a fresh child process under its own `timeout`; the first leg that fails ends the run."""
import argparse
import json
import re
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
import solver_ab as SA  # noqa: E402  (table, leg, result_of, the flagship model and the flag-off section)

HERE = SA.HERE
T_LAT, H_LAT, W_LAT, TOKENS, ELEMENTS, K1 = SA.T_LAT, SA.H_LAT, SA.W_LAT, SA.TOKENS, SA.ELEMENTS, SA.K1
INTERVALS = (2, 3, 5)
# form -> bytes per element: cond and uncond read (once more under zero-star), the old delta read with `out`, delta written;
# apply: cond and delta read, v written
FORMS = {"store, zero-star, with out": 4 * (4 + 1 + 1), "store, zero-star, no out": 4 * (4 + 1),
         "store, no zero-star, with out": 4 * (2 + 1 + 1), "apply, in place": 12, "apply, new buffer": 12}


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--depth", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--bench-steps", type=int, default=3)
    ap.add_argument("--bench-warmup", type=int, default=1)
    ap.add_argument("--denoise-steps", type=int, default=7)
    ap.add_argument("--consist-depth", type=int, default=4)
    ap.add_argument("--consist-steps", type=int, default=50)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--leg-timeout", type=int, default=420, help="seconds a child process may take")
    ap.add_argument("--out", type=Path, default=None)
    ap.add_argument("--only", type=str, default="regs,kernel,steps,flagoff,consist")
    ap.add_argument("--parent", type=Path, default=None)
    ap.add_argument("--kernel-child", action="store_true", help="internal: the calls the kernel section times")
    ap.add_argument("--steps-child", action="store_true", help="internal: a few flagship steps under cfg_reuse=2")
    ap.add_argument("--consist-child", action="store_true", help="internal: the self-consistency runs")
    return ap.parse_args(argv)


# ------------------------------------------------------------------------------------------------------------ regs
def regs_section():
    SA._imports(HERE)
    from lcv_hip import build
    src = build.CSRC / "cfg_reuse.hip"
    with tempfile.TemporaryDirectory() as tmp:
        out = Path(tmp) / "cfg_reuse.s"
        cmd = [build.HIPCC, *build.FLAGS, *build.EXTRA.get(src.name, []), "--cuda-device-only", "-S", str(src), "-o", str(out)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit(f"cfg_reuse_ab: hipcc -S failed:\n{r.stderr[-2000:]}")
        text = out.read_text()
    rows = []
    for m in re.finditer(r"\.amdhsa_kernel\s+(\S+)(.*?)\.end_amdhsa_kernel", text, flags=re.S):
        sym, body = m.group(1), m.group(2)
        field = lambda name: re.search(rf"\.amdhsa_{name}\s+(\S+)", body).group(1)
        name = re.search(r"cgr_\w+?_kernel", sym).group(0) + ("<%s>" % ("true" if "ILb1E" in sym else "false") if "ILb" in sym else "")
        rows.append([f"`{name}`", field("next_free_vgpr"), field("next_free_sgpr"), field("private_segment_fixed_size"),
                     field("group_segment_fixed_size")])
    return SA.table("Registers, scratch and LDS of the kernels (device assembly of csrc/cfg_reuse.hip, the library's flags; "
                    "store<true> with the drift sums, <false> without)", ["kernel", "VGPRs", "SGPRs", "scratch (B)", "LDS (B)"], rows)


# ------------------------------------------------------------------------------------------------------------ kernel
def kernel_child(args):
    SA._imports(HERE)
    import torch
    from lcv_hip import ops
    shape = (1, 16, T_LAT, H_LAT, W_LAT)
    g = torch.Generator(device="cuda").manual_seed(1)
    c, u, d, v = (torch.randn(shape, device="cuda", generator=g) for _ in range(4))
    out = torch.zeros((1, 2), device="cuda")

    def timed(fn):
        fn(); torch.cuda.synchronize()                                # the warm-up call
        ms = []
        for _ in range(args.iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return ms
    res = {"store, zero-star, with out": timed(lambda: ops.cfg_delta_store(c, u, d, 4.0, True, out=out)),
           "store, zero-star, no out": timed(lambda: ops.cfg_delta_store(c, u, d, 4.0, True)),
           "store, no zero-star, with out": timed(lambda: ops.cfg_delta_store(c, u, d, 4.0, False, out=out)),
           "apply, in place": timed(lambda: ops.cfg_delta_apply(c, d, out=c)),
           "apply, new buffer": timed(lambda: ops.cfg_delta_apply(c, d, out=v))}
    print("RESULT " + json.dumps({"elements": c.numel(), "ms": res}), flush=True)


def kernel_section(args):
    res = SA.result_of(SA.leg([sys.executable, Path(__file__).resolve(), "--kernel-child", "--iters", args.iters], args.leg_timeout))
    rows = []
    for name, ms in res["ms"].items():
        med = statistics.median(ms)
        rows.append([name, str(FORMS[name]), f"{med:.4f}", f"{min(ms):.4f}", f"{max(ms):.4f}",
                     f"{res['elements'] * FORMS[name] / med / 1e9:.2f}"])
    return SA.table(f"lcv_cfg_delta_store / lcv_cfg_delta_apply alone over the flagship latent ({res['elements'] / 1e6:.2f} M fp32 "
                    f"elements per operand), {args.iters} calls of each form after one warm-up call, device events around each call "
                    "(a zero-star store with `out` is three launches)",
                    ["form", "B / element", "median (ms)", "min", "max", "TB/s at the median"], rows)


# ------------------------------------------------------------------------------------------------------------ steps
def steps_child(args):
    """bench.py's K3 model and inputs; the first steps of a 50-step denoise under cfg_reuse=2: full and reuse steps alternate in
    one process; wall time per step from a synchronise in the step callback."""
    SA._imports(HERE)
    import torch
    from longcat_video.cfg_reuse import GuidanceReuse
    dev = torch.device("cuda", 0)
    pipe, pe, ne, pm = SA._model(args.depth, dev)
    g = torch.Generator(device=dev).manual_seed(42)
    latents = torch.randn((1, 16, T_LAT, H_LAT, W_LAT), generator=g, device=dev, dtype=torch.float32)
    reuse = GuidanceReuse(2)
    pipe.denoise(latents, pe, pm, ne, pm, num_cond_latents=0, num_inference_steps=50, stop_step=3, cfg_reuse=reuse)   # warm-up: full, reuse, full
    torch.cuda.synchronize()
    stamps = [time.perf_counter()]

    def stamp(i, x):
        torch.cuda.synchronize()
        stamps.append(time.perf_counter())
    pipe.denoise(latents, pe, pm, ne, pm, num_cond_latents=0, num_inference_steps=50, stop_step=args.denoise_steps,
                 step_callback=stamp, cfg_reuse=reuse)
    torch.cuda.synchronize()
    ms = [(b - a) * 1e3 for a, b in zip(stamps, stamps[1:])]
    full = [i for i in range(args.denoise_steps) if reuse.is_full(i)]
    res = {"full_ms": [ms[i] for i in full], "reuse_ms": [ms[i] for i in range(args.denoise_steps) if i not in full],
           "stats": pipe.last_cfg_reuse_stats}
    print("RESULT " + json.dumps(res), flush=True)


def steps_section(args):
    res = SA.result_of(SA.leg([sys.executable, Path(__file__).resolve(), "--depth", args.depth, "--denoise-steps", args.denoise_steps,
                               "--steps-child"], args.leg_timeout))
    med = statistics.median
    rows = [[name, str(len(v)), f"{med(v):.1f}", f"{min(v):.1f}", f"{max(v):.1f}"]
            for name, v in (("full (batch 2, then the store)", res["full_ms"]), ("reuse (batch 1, apply, unguided update)", res["reuse_ms"]))]
    lines = SA.table(f"The first {args.denoise_steps} steps of a 50-step denoise under `cfg_reuse=2` in one process (depth {args.depth}, "
                     f"49 x 720p, {TOKENS} tokens per row, CFG, zero-star), after a three-step warm-up; wall time per step from a "
                     "synchronise in the step callback", ["step", "steps", "ms per step, median", "min", "max"], rows)
    lines += [f"- a reuse step takes {med(res['reuse_ms']) / med(res['full_ms']):.3f} of a full step (medians); reported, not asserted",
              f"- the drift the full steps recorded (random-init weights): {res['stats']['distances']}", ""]
    return lines


# ------------------------------------------------------------------------------------------------------------ consist
def consist_child(args):
    SA._imports(HERE)
    import torch
    dev = torch.device("cuda", 0)
    pipe, pe, ne, pm = SA._model(args.consist_depth, dev)
    g = torch.Generator(device=dev).manual_seed(42)
    latents = torch.randn((1, 16) + K1, generator=g, device=dev, dtype=torch.float32)

    def run(**kw):
        out = pipe.denoise(latents, pe, pm, ne, pm, num_cond_latents=0, num_inference_steps=args.consist_steps, **kw)
        torch.cuda.synchronize()
        return out.double()
    plain = run()
    ref = run(cfg_reuse=1)
    trace = [d for d in pipe.last_cfg_reuse_stats["distances"] if d is not None]
    res = {"steps": args.consist_steps, "k1_is_plain": bool(torch.equal(plain, ref)),
           "moved": float((ref - latents.double()).norm() / ref.norm()),
           "trace": {"min": min(trace), "median": statistics.median(trace), "max": max(trace), "first": trace[0], "last": trace[-1]},
           "err": {}}
    for K in INTERVALS:
        out = run(cfg_reuse=K)
        s = pipe.last_cfg_reuse_stats
        res["err"][str(K)] = {"rel": float((out - ref).norm() / ref.norm()), "full": s["full"], "reused": s["reused"]}
    print("RESULT " + json.dumps(res), flush=True)


def consist_section(args):
    res = SA.result_of(SA.leg([sys.executable, Path(__file__).resolve(), "--consist-child", "--consist-depth", args.consist_depth,
                               "--consist-steps", args.consist_steps], args.leg_timeout))
    rows = [[f"K = {K}", str(v["full"]), str(v["reused"]), f"{v['rel']:.3e}"] for K, v in res["err"].items()]
    lines = SA.table(f"Self-consistency: relative L2 of the final latents of a {res['steps']}-step denoise against `cfg_reuse=1` from "
                     f"the same noise (random-init weights of the real architecture, depth {args.consist_depth}, "
                     f"{K1[0] * (K1[1] // 2) * (K1[2] // 2)} tokens, CFG 4.0, zero-star, Euler)",
                     ["interval", "full steps", "reuse steps", "relative L2 against K = 1"], rows)
    t = res["trace"]
    lines += [f"- `cfg_reuse=1` {'equals' if res['k1_is_plain'] else 'DIFFERS FROM'} the call without the keyword bit for bit; it moved the "
              f"latents by {res['moved']:.3e} (relative L2 against the noise it started from)",
              f"- the drift trace K = 1 recorded (sum |new - old| / sum |old| between consecutive steps): first {t['first']:.3e}, "
              f"last {t['last']:.3e}, min {t['min']:.3e}, median {t['median']:.3e}, max {t['max']:.3e}",
              "- random-init weights: these figures show that the plumbing holds together, and say nothing about the quality of a "
              "real checkpoint under any interval", ""]
    return lines


def main(argv=None):
    args = parse(argv)
    if args.kernel_child:
        return kernel_child(args)
    if args.steps_child:
        return steps_child(args)
    if args.consist_child:
        return consist_child(args)
    only = set(args.only.split(","))
    lines = [f"Depth {args.depth}, 49 x 720p ({TOKENS} tokens per row), CFG (2 rows on a full step, 1 on a reuse step); the stored "
             f"correction is {ELEMENTS * 4 / 1e6:.1f} MB of fp32.", ""]
    for name, fn in (("regs", regs_section), ("kernel", lambda: kernel_section(args)), ("steps", lambda: steps_section(args)),
                     ("flagoff", lambda: SA.flagoff_section(args)), ("consist", lambda: consist_section(args))):
        if name in only:
            lines += fn()
            if args.out is not None:                                  # what is measured so far survives a later leg's failure
                args.out.parent.mkdir(parents=True, exist_ok=True)
                args.out.write_text("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)


if __name__ == "__main__":
    main()

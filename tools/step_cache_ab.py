#!/usr/bin/env python3
"""Cost and reach of the first-block step cache (`step_cache=` / `--step-cache`, include/lcv_hip_stepcache.h) on the flagship
workload (49 x 720p, 46 800 tokens, depth 48, CFG): `python tools/step_cache_ab.py [--parent TREE] [--rounds 5]
[--only regs,kernel,flagoff,steps] [--out profiles/step_cache_measured.md]`.

Four sections:
  regs     the kernels' register counts, scratch and LDS, read from the device assembly that the library's own recipe
           (lcv_hip/build.py) gives for csrc/step_cache.hip; needs no GPU
  kernel   the three entry points alone over [2, 46 800, 4096] bf16 buffers, timed with device events around `iters`
           back-to-back launches after one warm-up launch; achieved bytes / s from the bytes per element the header states
  flagoff  `bench.py --gpus 1` with the flag absent in this tree and in `--parent TREE` (a checkout of the parent commit with its
           own built library), one run of each back to back in every round, the order alternating from round to round: the
           parent's own run-to-run range is the yardstick for this tree's median
  steps    one denoise of `--denoise-steps` steps each with the cache absent (`--absent-steps` steps), at threshold 0 (every
           step computed: the overhead, split into the diff and store kernels by device events, and the distance trace) and at
           threshold inf (every step skipped that may be: the bound on what any threshold can save)
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

HERE = Path(__file__).resolve().parents[1]
T_LAT, H_LAT, W_LAT, HIDDEN = 13, 90, 160, 4096                  # bench.py's K3
TOKENS = T_LAT * (H_LAT // 2) * (W_LAT // 2)
# entry point -> bytes read + written per element as the header states them
KERNEL_BYTES = {"lcv_stepcache_diff": 8, "lcv_stepcache_diff (prev = NULL)": 6, "lcv_stepcache_store": 6, "lcv_stepcache_apply": 6}


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--depth", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--bench-steps", type=int, default=3)
    ap.add_argument("--bench-warmup", type=int, default=1)
    ap.add_argument("--denoise-steps", type=int, default=50)
    ap.add_argument("--absent-steps", type=int, default=6)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--leg-timeout", type=int, default=420, help="seconds a child process may take")
    ap.add_argument("--out", type=Path, default=None)
    ap.add_argument("--only", type=str, default="regs,kernel,flagoff,steps")
    ap.add_argument("--parent", type=Path, default=None)
    ap.add_argument("--kernel-child", action="store_true", help="internal: the launches the kernel section times")
    ap.add_argument("--steps-child", type=str, default=None, help="internal: one denoise with the cache absent, at 0 or at inf")
    return ap.parse_args(argv)


def table(title, header, rows):
    return [title, "", "| " + " | ".join(header) + " |", "|" + "---|" * len(header)] + ["| " + " | ".join(r) + " |" for r in rows] + [""]


def _imports(root: Path):
    sys.path.insert(0, str(root / "longcat-video-tta_amd")); sys.path.insert(0, str(root))


def leg(cmd, seconds, cwd=None):
    """A fresh child process under `timeout`; its standard output, or the end of the run."""
    r = subprocess.run(["timeout", "-k", "10", str(seconds)] + [str(c) for c in cmd], capture_output=True, text=True, cwd=cwd)
    if r.returncode != 0:
        raise SystemExit(f"step_cache_ab: {' '.join(str(c) for c in cmd)} ended with status {r.returncode}; nothing more is "
                         f"started\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}")
    print(f"# leg done: {' '.join(str(c) for c in cmd[-4:])}", file=sys.stderr, flush=True)
    return r.stdout


def result_of(stdout: str) -> dict:
    return json.loads(next(ln for ln in stdout.splitlines() if ln.startswith("RESULT "))[7:])


# ------------------------------------------------------------------------------------------------------------ regs
def regs_section():
    _imports(HERE)
    from lcv_hip import build
    src = build.CSRC / "step_cache.hip"
    with tempfile.TemporaryDirectory() as tmp:
        out = Path(tmp) / "step_cache.s"
        cmd = [build.HIPCC, *build.FLAGS, *build.EXTRA.get(src.name, []), "--cuda-device-only", "-S", str(src), "-o", str(out)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit(f"step_cache_ab: hipcc -S failed:\n{r.stderr[-2000:]}")
        text = out.read_text()
    rows = []
    for m in re.finditer(r"\.amdhsa_kernel\s+(\S+)(.*?)\.end_amdhsa_kernel", text, flags=re.S):
        sym, body = m.group(1), m.group(2)
        field = lambda name: re.search(rf"\.amdhsa_{name}\s+(\S+)", body).group(1)
        name = re.search(r"stepcache_\w+?_kernel", sym).group(0) + ("<%s>" % ("true" if "ILb1E" in sym else "false") if "ILb" in sym else "")
        rows.append([f"`{name}`", field("next_free_vgpr"), field("next_free_sgpr"), field("private_segment_fixed_size"),
                     field("group_segment_fixed_size")])
    return table("Registers, scratch and LDS of the kernels (device assembly of csrc/step_cache.hip, the library's flags; diff<true> "
                 "with prev, combine<true> the store, <false> the apply)", ["kernel", "VGPRs", "SGPRs", "scratch (B)", "LDS (B)"], rows)


# ------------------------------------------------------------------------------------------------------------ kernel
def kernel_child(args):
    _imports(HERE)
    import torch
    from lcv_hip import ops
    shape = (2, TOKENS, HIDDEN)
    g = torch.Generator(device="cuda").manual_seed(1)
    x0, x1, p, xL = (torch.randn(shape, device="cuda", generator=g).to(torch.bfloat16) for _ in range(4))
    r, R, o = (torch.empty_like(x0) for _ in range(3))
    out = torch.zeros(5, dtype=torch.float32, device="cuda")

    def timed(fn):
        fn(); torch.cuda.synchronize()                                # the warm-up launch
        ms = []
        for _ in range(args.iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return ms
    res = {"lcv_stepcache_diff": timed(lambda: ops.stepcache_diff(x0, x1, p, r, 0.05, out)),
           "lcv_stepcache_diff (prev = NULL)": timed(lambda: ops.stepcache_diff(x0, x1, None, r, 0.05, out)),
           "lcv_stepcache_store": timed(lambda: ops.stepcache_store(xL, x1, R)),
           "lcv_stepcache_apply": timed(lambda: ops.stepcache_apply(x1, R, out=o))}
    print("RESULT " + json.dumps({"elements": x0.numel(), "ms": res}), flush=True)


def kernel_section(args):
    res = result_of(leg([sys.executable, Path(__file__).resolve(), "--kernel-child", "--iters", args.iters], args.leg_timeout))
    rows = []
    for name, ms in res["ms"].items():
        med = statistics.median(ms)
        rows.append([name, str(KERNEL_BYTES[name]), f"{med:.3f}", f"{min(ms):.3f}", f"{max(ms):.3f}",
                     f"{res['elements'] * KERNEL_BYTES[name] / med / 1e9:.2f}"])
    return table(f"Every entry point alone over [2, {TOKENS}, {HIDDEN}] bf16 ({res['elements'] / 1e6:.1f} M elements), {args.iters} "
                 "launches each after one warm-up launch, device events around each launch (diff is its two launches)",
                 ["entry point", "B / element", "median (ms)", "min", "max", "TB/s at the median"], rows)


# ------------------------------------------------------------------------------------------------------------ flagoff
def flagoff_section(args):
    trees = ([("the parent commit", args.parent.resolve())] if args.parent else []) + [("this tree", HERE)]
    times = {name: [] for name, _ in trees}
    for rnd in range(args.rounds):
        for name, root in (trees if rnd % 2 == 0 else trees[::-1]):    # who goes first alternates: a run warms the card for the next
            out = leg([sys.executable, root / "bench.py", "--gpus", 1, "--steps", args.bench_steps, "--warmup", args.bench_warmup,
                       "--depth", args.depth], args.leg_timeout, cwd=root)
            line = json.loads(next(ln for ln in out.splitlines() if ln.startswith("{")))
            times[name].append(line["ms_per_step"])
        print(f"# flagoff: round {rnd + 1} of {args.rounds} done", file=sys.stderr, flush=True)
    rows = [[name, f"{statistics.median(v):.1f}", f"{min(v):.1f}", f"{max(v):.1f}", " ".join(f"{x:.1f}" for x in v)]
            for name, v in times.items()]
    lines = table(f"bench.py --gpus 1 --steps {args.bench_steps} --warmup {args.bench_warmup}, flag absent, a fresh process per run, "
                  f"{args.rounds} interleaved rounds (the parent first in rounds 1, 3, ..., this tree first in rounds 2, 4, ...)", ["tree", "ms per step, median", "min", "max", "every run"], rows)
    if args.parent:
        p, v = times["the parent commit"], times["this tree"]
        med = statistics.median(v)
        lines += [f"- this tree's median {med:.1f} ms is {'inside' if min(p) <= med <= max(p) else 'OUTSIDE'} the parent's range "
                  f"{min(p):.1f}-{max(p):.1f} ms (parent's median {statistics.median(p):.1f})", ""]
    return lines


# ------------------------------------------------------------------------------------------------------------ steps
def steps_child(args):
    """bench.py's K3 model and inputs; one denoise; wall time per step from a synchronise in the step callback."""
    _imports(HERE)
    import torch
    from lcv_hip import ops
    from longcat_video.modules.longcat_video_dit import LongCatVideoTransformer3DModel
    from longcat_video.modules.scheduling_flow_match_euler_discrete import FlowMatchEulerDiscreteScheduler
    from longcat_video.pipeline_longcat_video import LongCatVideoPipeline
    from longcat_video.step_cache import StepCache
    dev = torch.device("cuda", 0)
    dit = LongCatVideoTransformer3DModel(device=dev, dtype=torch.bfloat16, depth=args.depth).eval()
    dit.init_synthetic_(seed=1234)
    pipe = LongCatVideoPipeline(scheduler=FlowMatchEulerDiscreteScheduler(), dit=dit)
    pipe.device = dev
    g = torch.Generator(device=dev).manual_seed(42)
    latents = torch.randn((1, 16, T_LAT, H_LAT, W_LAT), generator=g, device=dev, dtype=torch.float32)
    g2 = torch.Generator(device=dev).manual_seed(43)
    pe = torch.randn((1, 1, 512, 4096), generator=g2, device=dev, dtype=torch.float32).to(torch.bfloat16)
    ne = torch.randn((1, 1, 512, 4096), generator=g2, device=dev, dtype=torch.float32).to(torch.bfloat16)
    pm = torch.zeros((1, 512), dtype=torch.int64, device=dev); pm[:, :77] = 1
    mode = args.steps_child
    n = args.absent_steps if mode == "absent" else args.denoise_steps
    kw = {} if mode == "absent" else {"step_cache": StepCache(float(mode))}
    events = {"diff": [], "store": [], "apply": []}

    def with_events(name, fn):
        def wrapped(*a, **k):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record(); out = fn(*a, **k); e.record()
            events[name].append((s, e))
            return out
        return wrapped
    if mode != "absent":
        ops.stepcache_diff = with_events("diff", ops.stepcache_diff)
        ops.stepcache_store = with_events("store", ops.stepcache_store)
        ops.stepcache_apply = with_events("apply", ops.stepcache_apply)
    pipe.denoise(latents, pe, pm, ne, pm, num_cond_latents=0, num_inference_steps=50, stop_step=1)      # warm-up: one step
    for v in events.values():
        v.clear()
    torch.cuda.synchronize()
    stamps = [time.perf_counter()]

    def stamp(i, x):
        torch.cuda.synchronize()
        stamps.append(time.perf_counter())
    t0 = time.perf_counter()
    pipe.denoise(latents, pe, pm, ne, pm, num_cond_latents=0, num_inference_steps=50, stop_step=n, step_callback=stamp, **kw)
    torch.cuda.synchronize()
    total = time.perf_counter() - t0
    res = {"mode": mode, "steps": n, "total_s": total, "step_ms": [(b - a) * 1e3 for a, b in zip(stamps, stamps[1:])],
           "kernel_ms": {k: [s.elapsed_time(e) for s, e in v] for k, v in events.items()},
           "stats": pipe.last_step_cache_stats}
    print("RESULT " + json.dumps(res), flush=True)


def steps_section(args):
    me = [sys.executable, Path(__file__).resolve(), "--depth", args.depth, "--denoise-steps", args.denoise_steps,
          "--absent-steps", args.absent_steps]
    res = {m: result_of(leg(me + ["--steps-child", m], args.leg_timeout)) for m in ("absent", "0", "inf")}
    med = statistics.median
    absent, zero, inf = res["absent"], res["0"], res["inf"]
    base = med(absent["step_ms"])
    over = med(zero["step_ms"]) - base
    kd, ks = med(zero["kernel_ms"]["diff"]), med(zero["kernel_ms"]["store"])
    st = inf["stats"]
    skipped = [inf["step_ms"][i] for i in st["skipped_steps"]]
    computed = [inf["step_ms"][i] for i in range(inf["steps"]) if i not in st["skipped_steps"]]
    rows = [["cache absent", str(absent["steps"]), f"{base:.1f}", f"{min(absent['step_ms']):.1f}", f"{max(absent['step_ms']):.1f}", ""],
            ["threshold 0 (every step computed)", str(zero["steps"]), f"{med(zero['step_ms']):.1f}", f"{min(zero['step_ms']):.1f}",
             f"{max(zero['step_ms']):.1f}", f"{zero['total_s']:.1f}"],
            ["threshold inf, the computed steps", str(len(computed)), f"{med(computed):.1f}", f"{min(computed):.1f}",
             f"{max(computed):.1f}", ""],
            ["threshold inf, the skipped steps", str(len(skipped)), f"{med(skipped):.1f}", f"{min(skipped):.1f}", f"{max(skipped):.1f}",
             f"{inf['total_s']:.1f}"]]
    lines = table(f"One denoise per row in a process of its own (depth {args.depth}, 49 x 720p, CFG), wall time per step from a "
                  "synchronise in the step callback", ["run", "steps", "ms per step, median", "min", "max", "whole denoise (s)"], rows)
    lines += [f"- threshold 0 against the cache absent: {over:+.1f} ms per step at the medians; of that the diff launches take "
              f"{kd:.3f} ms and the store {ks:.3f} ms (device events, medians), which leaves {over - kd - ks:+.1f} ms for the "
              "device-to-host copy, its synchronise and the run-to-run difference of the two processes",
              f"- estimate by bytes: {2 * TOKENS * HIDDEN * 14 / 1e9:.2f} GB per step, {2 * TOKENS * HIDDEN * 14 / 6e12 * 1e3:.2f} ms "
              f"at 6 TB/s; measured in the two kernels: {kd + ks:.3f} ms",
              f"- threshold inf: {st['computed']} computed and {st['skipped']} skipped steps, {inf['total_s']:.1f} s for the "
              f"{inf['steps']}-step denoise against {zero['total_s']:.1f} s at threshold 0: the bound on what any threshold can save",
              f"- the apply launch of a skipped step: {med(inf['kernel_ms']['apply']):.3f} ms", "",
              f"Distance trace of the {zero['steps']}-step run at threshold 0 (synthetic weights; it says nothing about a real checkpoint):",
              "", "```", " ".join("null" if d is None else f"{d:.4f}" for d in zero["stats"]["distances"]), "```", ""]
    return lines


def main(argv=None):
    args = parse(argv)
    if args.kernel_child:
        return kernel_child(args)
    if args.steps_child is not None:
        return steps_child(args)
    only = set(args.only.split(","))
    lines = [f"Depth {args.depth}, 49 x 720p ({TOKENS} tokens), CFG (2 rows).", ""]
    for name, fn in (("regs", regs_section), ("kernel", lambda: kernel_section(args)), ("flagoff", lambda: flagoff_section(args)),
                     ("steps", lambda: steps_section(args))):
        if name in only:
            lines += fn()
            if args.out is not None:                                  # what is measured so far survives a later leg's failure
                args.out.parent.mkdir(parents=True, exist_ok=True)
                args.out.write_text("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)


if __name__ == "__main__":
    main()

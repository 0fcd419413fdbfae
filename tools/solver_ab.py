#!/usr/bin/env python3
"""Cost and discretisation error of the multistep solvers of the denoise loop (`solver=` / `--solver`,
include/lcv_hip_solver.h): `python tools/solver_ab.py [--parent TREE] [--rounds 5] [--only regs,kernel,flagoff,steps,converge]
[--out profiles/solver.md]`.

Five sections:
  regs      the kernels' register counts, scratch and LDS, read from the device assembly that the library's own recipe
            (lcv_hip/build.py) gives for csrc/solver_step.hip; needs no GPU
  kernel    lcv_cfg_lms_step alone over the flagship latent ([1, 16, 13, 90, 160] fp32 per operand), every form the loop
            calls, timed with device events around `iters` back-to-back calls after one warm-up call; achieved bytes / s from the
            bytes per element the header states
  flagoff   `bench.py --gpus 1` with the flag absent in this tree and in `--parent TREE` (a checkout of the parent commit with its
            own built library), one run of each back to back in every round, the order alternating from round to round: the
            parent's own run-to-run range is the yardstick for this tree's median
  steps     a few steps of the flagship denoise (49 x 720p, depth 48, CFG) under euler, ab2 and ab2c, each in a process of its
            own: wall time per step from a synchronise in the step callback
  converge  self-convergence on the random-init real architecture at a small size (K1 tokens, shallow depth): for each solver
            the relative L2 of the final latents at N in {16, 25, 50} against a 400-step Euler run from the same noise
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
T_LAT, H_LAT, W_LAT = 13, 90, 160                                 # bench.py's K3
TOKENS = T_LAT * (H_LAT // 2) * (W_LAT // 2)
ELEMENTS = 16 * T_LAT * H_LAT * W_LAT
K1 = (5, 32, 32)                                                  # 5 x 16 x 16 = 1 280 tokens
KINDS = ("euler", "ab2", "ab2c")
# form -> (terms, zero-star) ; bytes per element: cond, uncond, x and the history terms read (cond and uncond once more under
# zero-star), x and f0 written
FORMS = {"CFG, zero-star, 1 term": (1, True), "CFG, zero-star, 2 terms": (2, True), "CFG, zero-star, 3 terms": (3, True),
         "CFG, no zero-star, 3 terms": (3, False), "no guidance, 3 terms": (3, None)}


def form_bytes(terms, zero_star):
    reads = (1 if zero_star is None else 2) + 1 + (terms - 1) + (2 if zero_star else 0)
    return 4 * (reads + 2)


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--depth", type=int, default=48)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--bench-steps", type=int, default=3)
    ap.add_argument("--bench-warmup", type=int, default=1)
    ap.add_argument("--denoise-steps", type=int, default=6)
    ap.add_argument("--converge-depth", type=int, default=4)
    ap.add_argument("--converge-ref-steps", type=int, default=400)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--leg-timeout", type=int, default=420, help="seconds a child process may take")
    ap.add_argument("--out", type=Path, default=None)
    ap.add_argument("--only", type=str, default="regs,kernel,flagoff,steps,converge")
    ap.add_argument("--parent", type=Path, default=None)
    ap.add_argument("--kernel-child", action="store_true", help="internal: the calls the kernel section times")
    ap.add_argument("--steps-child", type=str, default=None, help="internal: a few flagship steps under one solver")
    ap.add_argument("--converge-child", action="store_true", help="internal: the self-convergence runs")
    return ap.parse_args(argv)


def table(title, header, rows):
    return [title, "", "| " + " | ".join(header) + " |", "|" + "---|" * len(header)] + ["| " + " | ".join(r) + " |" for r in rows] + [""]


def _imports(root: Path):
    sys.path.insert(0, str(root / "longcat-video-tta_amd")); sys.path.insert(0, str(root))


def leg(cmd, seconds, cwd=None):
    """A fresh child process under `timeout`; its standard output, or the end of the run."""
    r = subprocess.run(["timeout", "-k", "10", str(seconds)] + [str(c) for c in cmd], capture_output=True, text=True, cwd=cwd)
    if r.returncode != 0:
        raise SystemExit(f"solver_ab: {' '.join(str(c) for c in cmd)} ended with status {r.returncode}; nothing more is "
                         f"started\n{r.stdout[-2000:]}\n{r.stderr[-3000:]}")
    print(f"# leg done: {' '.join(str(c) for c in cmd[-4:])}", file=sys.stderr, flush=True)
    return r.stdout


def result_of(stdout: str) -> dict:
    return json.loads(next(ln for ln in stdout.splitlines() if ln.startswith("RESULT "))[7:])


# ------------------------------------------------------------------------------------------------------------ regs
def regs_section():
    _imports(HERE)
    from lcv_hip import build
    src = build.CSRC / "solver_step.hip"
    with tempfile.TemporaryDirectory() as tmp:
        out = Path(tmp) / "solver_step.s"
        cmd = [build.HIPCC, *build.FLAGS, *build.EXTRA.get(src.name, []), "--cuda-device-only", "-S", str(src), "-o", str(out)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit(f"solver_ab: hipcc -S failed:\n{r.stderr[-2000:]}")
        text = out.read_text()
    rows = []
    for m in re.finditer(r"\.amdhsa_kernel\s+(\S+)(.*?)\.end_amdhsa_kernel", text, flags=re.S):
        sym, body = m.group(1), m.group(2)
        field = lambda name: re.search(rf"\.amdhsa_{name}\s+(\S+)", body).group(1)
        name = re.search(r"lms_\w+?_kernel", sym).group(0) + ("<%s>" % ("true" if "ILb1E" in sym else "false") if "ILb" in sym else "")
        rows.append([f"`{name}`", field("next_free_vgpr"), field("next_free_sgpr"), field("private_segment_fixed_size"),
                     field("group_segment_fixed_size")])
    return table("Registers, scratch and LDS of the kernels (device assembly of csrc/solver_step.hip, the library's flags; "
                 "step<true> with uncond, <false> without)", ["kernel", "VGPRs", "SGPRs", "scratch (B)", "LDS (B)"], rows)


# ------------------------------------------------------------------------------------------------------------ kernel
def kernel_child(args):
    _imports(HERE)
    import torch
    from lcv_hip import ops
    shape = (1, 16, T_LAT, H_LAT, W_LAT)
    g = torch.Generator(device="cuda").manual_seed(1)
    c, u, x, f0, f1, f2 = (torch.randn(shape, device="cuda", generator=g) for _ in range(6))
    w = (-0.03, 0.02, -0.01)

    def timed(fn):
        fn(); torch.cuda.synchronize()                                # the warm-up call
        ms = []
        for _ in range(args.iters):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); fn(); b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return ms
    res = {}
    for name, (terms, zs) in FORMS.items():
        res[name] = timed(lambda: ops.cfg_lms_step(c, None if zs is None else u, x, f0, f1, f2, 4.0, w[:terms], negate=True,
                                                   zero_star=bool(zs)))
    res["lcv_cfg_euler_step (CFG, zero-star)"] = timed(lambda: ops.cfg_euler_step(c, u, x, 4.0, -0.02))
    print("RESULT " + json.dumps({"elements": x.numel(), "ms": res}), flush=True)


def kernel_section(args):
    res = result_of(leg([sys.executable, Path(__file__).resolve(), "--kernel-child", "--iters", args.iters], args.leg_timeout))
    rows = []
    for name, ms in res["ms"].items():
        nbytes = form_bytes(*FORMS[name]) if name in FORMS else 4 * 6          # Euler: cond, uncond twice, x read, x written
        med = statistics.median(ms)
        rows.append([name, str(nbytes), f"{med:.4f}", f"{min(ms):.4f}", f"{max(ms):.4f}", f"{res['elements'] * nbytes / med / 1e9:.2f}"])
    return table(f"lcv_cfg_lms_step alone over the flagship latent ({res['elements'] / 1e6:.2f} M fp32 elements per operand), "
                 f"{args.iters} calls of each form after one warm-up call, device events around each call (a zero-star call is its "
                 "two launches and the workspace's allocation from the caching allocator); the Euler step for comparison",
                 ["form", "B / element", "median (ms)", "min", "max", "TB/s at the median"], rows)


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
                  f"{args.rounds} interleaved rounds (the parent first in rounds 1, 3, ..., this tree first in rounds 2, 4, ...)",
                  ["tree", "ms per step, median", "min", "max", "every run"], rows)
    if args.parent:
        p, v = times["the parent commit"], times["this tree"]
        med = statistics.median(v)
        lines += [f"- this tree's median {med:.1f} ms is {'inside' if min(p) <= med <= max(p) else 'OUTSIDE'} the parent's range "
                  f"{min(p):.1f}-{max(p):.1f} ms (parent's median {statistics.median(p):.1f}); this tree's range "
                  f"{min(v):.1f}-{max(v):.1f} ms", ""]
    return lines


# ------------------------------------------------------------------------------------------------------------ steps
def _model(depth, dev):
    import torch
    from longcat_video.modules.longcat_video_dit import LongCatVideoTransformer3DModel
    from longcat_video.modules.scheduling_flow_match_euler_discrete import FlowMatchEulerDiscreteScheduler
    from longcat_video.pipeline_longcat_video import LongCatVideoPipeline
    dit = LongCatVideoTransformer3DModel(device=dev, dtype=torch.bfloat16, depth=depth).eval()
    dit.init_synthetic_(seed=1234)
    pipe = LongCatVideoPipeline(scheduler=FlowMatchEulerDiscreteScheduler(), dit=dit)
    pipe.device = dev
    g2 = torch.Generator(device=dev).manual_seed(43)
    pe = torch.randn((1, 1, 512, 4096), generator=g2, device=dev, dtype=torch.float32).to(torch.bfloat16)
    ne = torch.randn((1, 1, 512, 4096), generator=g2, device=dev, dtype=torch.float32).to(torch.bfloat16)
    pm = torch.zeros((1, 512), dtype=torch.int64, device=dev); pm[:, :77] = 1
    return pipe, pe, ne, pm


def steps_child(args):
    """bench.py's K3 model and inputs; the first steps of a 50-step denoise; wall time per step from a synchronise in the step
    callback, and the update alone from device events around it."""
    _imports(HERE)
    import torch
    from lcv_hip import ops
    dev = torch.device("cuda", 0)
    pipe, pe, ne, pm = _model(args.depth, dev)
    g = torch.Generator(device=dev).manual_seed(42)
    latents = torch.randn((1, 16, T_LAT, H_LAT, W_LAT), generator=g, device=dev, dtype=torch.float32)
    kind = args.steps_child
    events = []

    def with_events(fn):
        def wrapped(*a, **k):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record(); out = fn(*a, **k); e.record()
            events.append((s, e))
            return out
        return wrapped
    ops.cfg_lms_step = with_events(ops.cfg_lms_step)
    ops.cfg_euler_step = with_events(ops.cfg_euler_step)
    pipe.denoise(latents, pe, pm, ne, pm, num_cond_latents=0, num_inference_steps=50, stop_step=1, solver=kind)     # warm-up: one step
    events.clear()
    torch.cuda.synchronize()
    stamps = [time.perf_counter()]

    def stamp(i, x):
        torch.cuda.synchronize()
        stamps.append(time.perf_counter())
    pipe.denoise(latents, pe, pm, ne, pm, num_cond_latents=0, num_inference_steps=50, stop_step=args.denoise_steps,
                 step_callback=stamp, solver=kind)
    torch.cuda.synchronize()
    res = {"kind": kind, "step_ms": [(b - a) * 1e3 for a, b in zip(stamps, stamps[1:])],
           "update_ms": [s.elapsed_time(e) for s, e in events]}
    print("RESULT " + json.dumps(res), flush=True)


def steps_section(args):
    me = [sys.executable, Path(__file__).resolve(), "--depth", args.depth, "--denoise-steps", args.denoise_steps]
    res = {k: result_of(leg(me + ["--steps-child", k], args.leg_timeout)) for k in KINDS}
    med = statistics.median
    rows = [[k, str(len(r["step_ms"])), f"{med(r['step_ms']):.1f}", f"{min(r['step_ms']):.1f}", f"{max(r['step_ms']):.1f}",
             f"{med(r['update_ms']):.3f}", f"{max(r['update_ms']):.3f}"] for k, r in res.items()]
    return table(f"The first {args.denoise_steps} steps of a 50-step denoise per row in a process of its own (depth {args.depth}, "
                 "49 x 720p, CFG, zero-star), wall time per step from a synchronise in the step callback; the update alone from "
                 "device events around the call (steps from the third on carry the full history)",
                 ["solver", "steps", "ms per step, median", "min", "max", "update (ms), median", "max"], rows)


# ------------------------------------------------------------------------------------------------------------ converge
def converge_child(args):
    _imports(HERE)
    import torch
    dev = torch.device("cuda", 0)
    pipe, pe, ne, pm = _model(args.converge_depth, dev)
    g = torch.Generator(device=dev).manual_seed(42)
    latents = torch.randn((1, 16) + K1, generator=g, device=dev, dtype=torch.float32)

    def run(kind, n):
        out = pipe.denoise(latents, pe, pm, ne, pm, num_cond_latents=0, num_inference_steps=n, solver=kind)
        torch.cuda.synchronize()
        return out.double()
    ref = run("euler", args.converge_ref_steps)
    again = run("euler", args.converge_ref_steps)
    res = {"ref_steps": args.converge_ref_steps, "ref_repeat": float((again - ref).norm() / ref.norm()),
           "moved": float((ref - latents.double()).norm() / ref.norm()), "err": {}}
    for kind in KINDS:
        res["err"][kind] = {str(n): float((run(kind, n) - ref).norm() / ref.norm()) for n in (16, 25, 50)}
        print(f"# converge: {kind} done", file=sys.stderr, flush=True)
    print("RESULT " + json.dumps(res), flush=True)


def converge_section(args):
    res = result_of(leg([sys.executable, Path(__file__).resolve(), "--converge-child", "--converge-depth", args.converge_depth,
                         "--converge-ref-steps", args.converge_ref_steps], args.leg_timeout))
    rows = [[k] + [f"{v[n]:.3e}" for n in ("16", "25", "50")] for k, v in res["err"].items()]
    lines = table(f"Self-convergence: relative L2 of the final latents against a {res['ref_steps']}-step Euler run from the same "
                  f"noise (random-init weights of the real architecture, depth {args.converge_depth}, "
                  f"{K1[0] * (K1[1] // 2) * (K1[2] // 2)} tokens, CFG 4.0, zero-star)", ["solver", "N = 16", "25", "50"], rows)
    lines += [f"- the reference moved the latents by {res['moved']:.3e} (relative L2 against the noise it started from); a second "
              f"{res['ref_steps']}-step run differs from the first by {res['ref_repeat']:.1e}",
              "- this is discretisation error only, floored by the noise of the bf16 forward (every step rounds the state to bf16 on "
              "its way into the model) and by the reference's own first-order error; it says nothing about a real checkpoint", ""]
    return lines


def main(argv=None):
    args = parse(argv)
    if args.kernel_child:
        return kernel_child(args)
    if args.steps_child is not None:
        return steps_child(args)
    if args.converge_child:
        return converge_child(args)
    only = set(args.only.split(","))
    lines = [f"Depth {args.depth}, 49 x 720p ({TOKENS} tokens), CFG (2 rows); the latent is {ELEMENTS * 4 / 1e6:.1f} MB of fp32.", ""]
    for name, fn in (("regs", regs_section), ("kernel", lambda: kernel_section(args)), ("flagoff", lambda: flagoff_section(args)),
                     ("steps", lambda: steps_section(args)), ("converge", lambda: converge_section(args))):
        if name in only:
            lines += fn()
            if args.out is not None:                                  # what is measured so far survives a later leg's failure
                args.out.parent.mkdir(parents=True, exist_ok=True)
                args.out.write_text("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)


if __name__ == "__main__":
    main()

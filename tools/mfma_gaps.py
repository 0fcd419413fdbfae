#!/usr/bin/env python3
"""Issue budget of the MFMA gaps of a kernel's steady loop (hipcc `-S` text in, a gap table out).

At one wave per SIMD a `v_mfma_f32_32x32x16_bf16` holds the matrix pipe for 32 cycles and the SIMD's vector issue for 8 of them;
what the wave issues between two MFMAs is hidden while it fits the rest: at most 5 instructions whose issue costs sum to at most
24 cycles, at most one of them an 8-cycle transcendental (MI355X issue-cost constants).  A gap past that budget stretches the
MFMA cadence by its excess.  This tool prices every gap of the steady loop that way:

  * the steady loop is the innermost MFMA loop with the largest MFMA count; among equals (the peeled edge form of the same
    iteration), the one with the fewest instructions;
  * a gap is what follows one MFMA up to the next MFMA.  A gap that holds a label, a branch or an `s_barrier` is a phase
    boundary: only its TAIL (the instructions before the first of those, or before the `s_waitcnt` that precedes the barrier)
    runs in the shadow of the MFMA and is priced; the rest is reported as the boundary's remainder;
  * prices (cycles of vector / scalar issue): transcendentals 8, `v_cvt_pk_bf16_f32` 5, `s_nop N` 4 (N + 1), anything else 4.
    Every instruction but an MFMA is an issue: `s_waitcnt` and `s_nop` included.

Usage: python tools/mfma_gaps.py file.s [substring of the kernel name]     (exit code 1 when a gap is over budget)
"""
import re
import sys
from pathlib import Path
from typing import List, NamedTuple, Optional

sys.path.insert(0, str(Path(__file__).resolve().parent))
import isa_hazards as H  # noqa: E402

MAX_ISSUES = 5
MAX_CYCLES = 24
MAX_TRANS = 1
TRANS = ("v_exp_", "v_log_", "v_rcp_", "v_rsq_", "v_sqrt_", "v_sin_", "v_cos_")


def price(i: H.Inst) -> int:
    if i.op.startswith(TRANS):
        return 8
    if i.op.startswith("v_cvt_pk_bf16_f32"):
        return 5
    if i.op == "s_nop":
        return 4 * (int(i.args or 0) + 1)
    return 4


class Gap(NamedTuple):
    index: int                 # MFMA index within the loop (the gap follows that MFMA)
    insts: List[H.Inst]        # priced part
    boundary: bool             # phase boundary: label / branch / barrier after the priced part
    rest: int                  # instructions of a boundary gap past its priced part

    @property
    def issues(self) -> int:
        return len(self.insts)

    @property
    def cycles(self) -> int:
        return sum(price(i) for i in self.insts)

    @property
    def trans(self) -> int:
        return sum(i.op.startswith(TRANS) for i in self.insts)

    def over(self) -> Optional[str]:
        why = []
        if self.issues > MAX_ISSUES:
            why.append(f"{self.issues} issues > {MAX_ISSUES}")
        if self.cycles > MAX_CYCLES:
            why.append(f"{self.cycles} cyc > {MAX_CYCLES}")
        if self.trans > MAX_TRANS:
            why.append(f"{self.trans} transcendentals > {MAX_TRANS}")
        return ", ".join(why) or None


def _is_boundary(i: H.Inst) -> bool:
    return i.op == ":label" or i.op.startswith(("s_cbranch", "s_branch", "s_barrier", "s_setpc", "s_endpgm"))


def steady_loop(insts: List[H.Inst]):
    loops = H.innermost_mfma_loops(insts)
    if not loops:
        return None
    count = lambda ab: sum(x.op.startswith("v_mfma") for x in insts[ab[0]:ab[1] + 1])
    most = max(count(ab) for ab in loops)
    return min((ab for ab in loops if count(ab) == most), key=lambda ab: ab[1] - ab[0])


def gaps_of(insts: List[H.Inst]) -> List[Gap]:
    a, b = steady_loop(insts)
    body = insts[a:b + 1]
    at = [k for k, i in enumerate(body) if i.op.startswith("v_mfma")]
    out = []
    for n, k in enumerate(at):
        seg = body[k + 1:at[n + 1]] if n + 1 < len(at) else body[k + 1:]
        cut = next((m for m, i in enumerate(seg) if _is_boundary(i)), None)
        if cut is None and n + 1 < len(at):
            out.append(Gap(n, seg, False, 0))
            continue
        cut = len(seg) if cut is None else cut
        if cut > 0 and seg[cut - 1].op == "s_waitcnt" and cut < len(seg) and seg[cut].op == "s_barrier":
            cut -= 1                                     # the wait in front of the barrier belongs to the barrier
        out.append(Gap(n, seg[:cut], True, sum(i.op != ":label" for i in seg[cut:])))
    return out


def kernel_gaps(text: str, kernel: str = ""):
    ks = {k: v for k, v in H.parse_kernels(text).items() if kernel in k}
    assert len(ks) == 1, f"expected one MFMA kernel matching {kernel!r}, found {sorted(ks)}"
    (name, insts), = ks.items()
    return name, insts, gaps_of(insts)


def loop_insts(insts: List[H.Inst]) -> List[H.Inst]:
    a, b = steady_loop(insts)
    return [i for i in insts[a:b + 1] if i.op != ":label"]


def report(gaps: List[Gap]) -> str:
    lines = [" gap  iss  cyc  exp  fillers"]
    for g in gaps:
        mark = (" OVER: " + g.over()) if g.over() else ""
        tail = f"  | boundary, {g.rest} more" if g.boundary else ""
        lines.append(f"{g.index:4d} {g.issues:4d} {g.cycles:4d} {g.trans:4d}  " + " ".join(i.op for i in g.insts) + tail + mark)
    over = [g for g in gaps if g.over()]
    excess = sum(max(0, g.cycles - MAX_CYCLES) for g in gaps)
    lines.append(f"{len(gaps)} gaps, {sum(g.issues for g in gaps)} priced issues, {len(over)} over budget, "
                 f"{excess} cycles over, {sum(g.trans > 1 for g in gaps)} with > 1 transcendental")
    return "\n".join(lines)


def main(argv: Optional[List[str]] = None) -> int:
    argv = argv if argv is not None else sys.argv[1:]
    name, insts, gaps = kernel_gaps(Path(argv[0]).read_text(), argv[1] if len(argv) > 1 else "")
    print(name)
    print(report(gaps))
    return 1 if any(g.over() for g in gaps) else 0


if __name__ == "__main__":
    sys.exit(main())

"""CPU: phase 2 of the steady loop of `attn_fwd_w64_kernel` is laid out level (csrc/attn_fwd_w64.hip, W64_P2), priced by
tools/mfma_gaps.py on hipcc's output for the library's own flags (the companion of tests/test_attn_fwd_gap_trim.py).

The loop is two 64-key iterations of 32 score MFMAs (phase 1) and 32 PV MFMAs (phase 2).  Phase 1 is at its floor: two adjacent
gaps carry 3 exps, 3 adds, 1.5 packs, a fragment read and its wait, 52-56 cycles against 48.  Phase 2's work fits its budget
in aggregate, so what is held here is its placement:

  * the summed over-budget cycles of the 128 gaps are at most 406: the 530 of the table before this one minus 124, the
    smallest static change of this loop so far whose time gain counted (profiles/r09_attn_fwd_trim.md);
  * phase 2 carries less over-run than phase 1;
  * no phase-2 gap is above the bound the source asserts for its table (`w64_table_ok(W64_P2, ...)`);
  * the tail of phase 2 is used: its last six gaps are not all under 12 cycles while an earlier gap is over 24.

profiles/r10_attn_fwd_level.md has the figures of this table and of the one before it.
"""
import re
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT / "longcat-video-tta_amd"))
import mfma_gaps as G  # noqa: E402

OVER_BOUND = 406            # 530 - 124
P2_GAP_BOUND = 28           # = the max_cyc the source asserts for W64_P2
TAIL = 6
TAIL_FLOOR = 12


def phase_of(n: int, per_phase: int) -> int:
    return 1 + (n // per_phase) % 2


def figures(text: str, kernel: str = "", per_phase: int = 32):
    _, _, gaps = G.kernel_gaps(text, kernel)
    over = [max(0, g.cycles - G.MAX_CYCLES) for g in gaps]
    return {"over": sum(over),
            "over_p1": sum(o for n, o in enumerate(over) if phase_of(n, per_phase) == 1),
            "over_p2": sum(o for n, o in enumerate(over) if phase_of(n, per_phase) == 2),
            "p2": [[g.cycles for g in gaps[a:a + per_phase]] for a in range(per_phase, len(gaps), 2 * per_phase)]}


def check(text: str, kernel: str = "", per_phase: int = 32, over_bound: int = OVER_BOUND, gap_bound: int = P2_GAP_BOUND):
    """-> {name of the bound: finding} for the steady loop of the one MFMA kernel in `text`."""
    f = figures(text, kernel, per_phase)
    _, _, gaps = G.kernel_gaps(text, kernel)
    out = {}
    if f["over"] > over_bound:
        out["over"] = f"{f['over']} cycles over budget > {over_bound}"
    if not f["over_p2"] < f["over_p1"]:
        out["phases"] = f"phase 2 carries {f['over_p2']} cycles of over-run, phase 1 {f['over_p1']}"
    for it, p2 in enumerate(f["p2"]):
        high = [(j, c) for j, c in enumerate(p2) if c > gap_bound]
        if high:
            out["gap"] = f"iteration {it}: phase-2 gaps over {gap_bound}: {high}"
        base = (2 * it) * per_phase
        earlier = [g.cycles for g in gaps[base:base + 2 * per_phase - TAIL]]
        if all(c < TAIL_FLOOR for c in p2[-TAIL:]) and any(c > G.MAX_CYCLES for c in earlier):
            out["tail"] = f"iteration {it}: the last {TAIL} gaps of phase 2 are {p2[-TAIL:]} while an earlier gap has {max(earlier)}"
    return out


@pytest.fixture(scope="module")
def w64_isa(tmp_path_factory):
    from lcv_hip import build as B
    dst = tmp_path_factory.mktemp("level") / "attn_fwd_w64.s"
    name = "attn_fwd_w64.hip"
    cmd = [B.HIPCC, *B.FLAGS, *B.EXTRA.get(name, []), "--cuda-device-only", "-S", str(B.CSRC / name), "-o", str(dst)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return dst.read_text()


def test_the_gap_bound_is_the_one_the_source_asserts():
    from lcv_hip import build as B
    src = (B.CSRC / "attn_fwd_w64.hip").read_text()
    m = re.search(r"w64_table_ok\(W64_P2, 2, (\d+), (\d+)\)", src)
    assert m and int(m.group(1)) == P2_GAP_BOUND and int(m.group(2)) == 1


def test_phase_2_is_level(w64_isa):
    f = figures(w64_isa, "attn_fwd_w64_kernel")
    print(f)
    assert len(f["p2"]) == 2 and all(len(p) == 32 for p in f["p2"])
    findings = check(w64_isa, "attn_fwd_w64_kernel")
    assert not findings, "\n".join(findings.values())


# ---------------------------------------------------------------------------------------------------------------- bent stand-ins
# one iteration of 8 + 8 gaps; the loop's last gap is a boundary: only its tail (here the s_cmp) is priced
_HEAD = "_Z4bentv:\n"
_MFMA = "\tv_mfma_f32_32x32x16_bf16 v[0:15], v[100:103], a[4:7], v[0:15]\n"
_ADD = "\tv_add_f32_e32 v3, v3, v1\n"
_SMALL = {"per_phase": 8, "over_bound": 40, "gap_bound": 28}


def _kernel(p1, p2) -> str:
    """p1, p2: 8 cycle counts each (multiples of 4; the last of p2 includes the 4 of the loop's s_cmp)."""
    cyc = list(p1) + list(p2)
    cyc[-1] -= 4
    body = "".join(_MFMA + _ADD * (c // 4) for c in cyc)
    return _HEAD + ".LBB0_1:\n" + body + "\ts_cmp_lt_u32 s4, s5\n\ts_cbranch_scc1 .LBB0_1\n\ts_endpgm\n.Lfunc_end0:\n"


CLEAN = ([28] * 8, [16] * 8)                                     # phase 1: 32 over; phase 2: none, tail in use
BENT = {
    "over": ([32] * 8, [16] * 8),                                # 64 over > 40
    "phases": ([24] * 8, [16] * 8),                              # phase 2's over-run (0) is not below phase 1's (0)
    "gap": ([28] * 8, [16, 16, 32, 16, 16, 16, 16, 16]),         # one phase-2 gap past its bound; the sum is 40, still in
    "tail": ([28] * 8, [16, 16, 8, 8, 8, 8, 8, 8]),              # the last six gaps idle while phase 1 runs over
}


def test_the_stand_in_loop_is_clean():
    assert figures(_kernel(*CLEAN), per_phase=8) == {"over": 32, "over_p1": 32, "over_p2": 0, "p2": [[16] * 8]}
    assert not check(_kernel(*CLEAN), **_SMALL)


@pytest.mark.parametrize("name", sorted(BENT))
def test_each_bound_fails_on_its_own(name):
    assert sorted(check(_kernel(*BENT[name]), **_SMALL)) == [name]

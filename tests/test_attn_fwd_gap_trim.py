"""CPU: what the steady loop of `attn_fwd_w64_kernel` no longer carries, priced by tools/mfma_gaps.py on hipcc's output for the
library's own flags (the companion of tests/test_attn_fwd_gap_budget.py, which holds the per-gap bounds).

hipcc pads a gap statement (asm) that reads the result of another gap statement with an `s_nop` unless an instruction of its
own stands between the two; asm statements, the MFMA included, count for nothing there.  The loop's only such instructions
are the fragment reads and their waits, so each odd gap now OPENS with its fragment read (csrc/attn_fwd_w64.hip, w64_apart):
no add or pack of the table is padded any more.  Bounds: what the kernel compiles to, each below the parent's figure from the
same tool (profiles/r09_attn_fwd_trim.md has both sets; a gap counts as over when its priced cycles exceed the tool's 24).
"""
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT / "longcat-video-tta_amd"))
import mfma_gaps as G  # noqa: E402

PARENT = {"cycles": 3328, "over": 654, "gaps_over": 78}     # two iterations (128 gaps) of the parent's loop
BOUND = {"cycles": 3184, "over": 530, "gaps_over": 66}      # this kernel
PADDED = ("v_add_f32", "v_cvt_pk_bf16_f32")


def figures(text: str, kernel: str = ""):
    _, _, gaps = G.kernel_gaps(text, kernel)
    return {"cycles": sum(g.cycles for g in gaps),
            "over": sum(max(0, g.cycles - G.MAX_CYCLES) for g in gaps),
            "gaps_over": sum(g.cycles > G.MAX_CYCLES for g in gaps)}


def check(text: str, kernel: str = "", bound=BOUND):
    """-> list of findings for the steady loop of the one MFMA kernel in `text`."""
    _, _, gaps = G.kernel_gaps(text, kernel)
    out = []
    for g in gaps:
        for a, b in zip(g.insts, g.insts[1:]):
            if a.op == "s_nop" and b.op.startswith(PADDED):
                out.append(f"gap {g.index}: s_nop in front of `{b.text}` (line {b.line})")
    got = figures(text, kernel)
    out += [f"{k}: {got[k]} > {bound[k]}" for k in sorted(bound) if got[k] > bound[k]]
    return out


@pytest.fixture(scope="module")
def w64_isa(tmp_path_factory):
    from lcv_hip import build as B
    dst = tmp_path_factory.mktemp("trim") / "attn_fwd_w64.s"
    name = "attn_fwd_w64.hip"
    cmd = [B.HIPCC, *B.FLAGS, *B.EXTRA.get(name, []), "--cuda-device-only", "-S", str(B.CSRC / name), "-o", str(dst)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return dst.read_text()


def test_the_bounds_are_below_the_parents():
    assert all(BOUND[k] < PARENT[k] for k in PARENT)


def test_the_steady_loop_is_trimmed(w64_isa):
    print(figures(w64_isa, "attn_fwd_w64_kernel"))
    findings = check(w64_isa, "attn_fwd_w64_kernel")
    assert not findings, "\n".join(findings)


# ---------------------------------------------------------------------------------------------------------------- bent stand-ins
_HEAD = "_Z4bentv:\n"
_MFMA = "\tv_mfma_f32_32x32x16_bf16 v[0:15], v[100:103], a[4:7], v[0:15]\n"
_LOOP = ".LBB0_1:\n{body}\ts_cmp_lt_u32 s4, s5\n\ts_cbranch_scc1 .LBB0_1\n\ts_endpgm\n.Lfunc_end0:\n"
_GAP = "\tds_read_b128 v[100:103], v90\n\tv_add_f32_e32 v3, v3, v1\n\tv_exp_f32 v1, v2\n"       # 16 cycles
_SMALL = {"cycles": 3 * 16 + 12 + 4, "over": 0, "gaps_over": 0}                               # (+ 4: the s_cmp behind the last MFMA)


def _kernel(gap: str) -> str:
    return _HEAD + _LOOP.format(body=(_MFMA + _GAP) * 3 + _MFMA + gap + _MFMA)


BENT = {
    "padded_add": "\tv_exp_f32 v1, v2\n\ts_nop 0\n\tv_add_f32 v3, v3, v1\n",
    "padded_pack": "\ts_nop 0\n\tv_cvt_pk_bf16_f32 v9, v1, v2\n",
    "too_many_cycles": "\tv_add_f32_e32 v3, v3, v1\n" * 4,                  # 16: the sum goes past its bound, no gap past 24
    "over_budget": "\tv_add_f32_e32 v3, v3, v1\n" * 7,                      # 28: one gap over, by 4
}


def test_the_stand_in_loop_is_clean():
    assert not check(_kernel("\tv_add_f32_e32 v3, v3, v1\n" * 3), bound=_SMALL)


@pytest.mark.parametrize("name", sorted(BENT))
def test_the_guard_fails_on_a_bent_gap(name):
    assert check(_kernel(BENT[name]), bound=_SMALL)


def test_each_bound_is_held_on_its_own():
    got = figures(_kernel(BENT["over_budget"]))
    assert got == {"cycles": 3 * 16 + 28 + 4, "over": 4, "gaps_over": 1}
    for k in got:                                                           # every other bound wide open: this one still fails
        assert check(_kernel(BENT["over_budget"]), bound={**{j: 10 ** 6 for j in got}, k: got[k] - 1})

"""CPU: the steady loop of `attn_fwd_w64_kernel`, as hipcc compiles it with the library's flags, keeps the shape of its gap table
(csrc/attn_fwd_w64.hip, W64_P1 / W64_P2) — a guard against compiler drift, priced by tools/mfma_gaps.py.

At one wave per SIMD a 32x32x16 MFMA hides about 5 instructions / 24 issue-cycles (v_exp 8, v_cvt_pk 5, the rest 4).  One
64-key iteration carries more than its 64 gaps can hide that way (64 exp, 32 pack, 64 scalar adds, 32 max3, 48 fragment reads
and their waits, 8 LDS-DMA pieces: ~1 560 issue-cycles against 64 x 24), so the bounds held here are the table's, not the
ideal: no packed f32 between the MFMAs, at most two transcendentals and MAX_ISSUES / MAX_CYCLES per gap.  HEAD before the
table (packed row sums, the DMA pieces and the max chain stacked in the first gaps of phase 2) fails every one of them.
"""
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT / "longcat-video-tta_amd"))
import mfma_gaps as G  # noqa: E402

MAX_ISSUES = 9
MAX_CYCLES = 49
MAX_TRANS = 2


def check(text: str):
    """-> list of findings for the steady loop of the one MFMA kernel in `text`."""
    _, insts, gaps = G.kernel_gaps(text)
    out = [f"packed f32 in the steady loop: `{i.text}` (line {i.line})" for i in G.loop_insts(insts) if i.op.startswith("v_pk_") and i.op.endswith("_f32")]
    for g in gaps:
        if g.issues > MAX_ISSUES or g.cycles > MAX_CYCLES or g.trans > MAX_TRANS:
            out.append(f"gap {g.index}: {g.issues} issues, {g.cycles} cyc, {g.trans} transcendentals: " + " ".join(i.op for i in g.insts))
    return out


@pytest.fixture(scope="module")
def w64_isa(tmp_path_factory):
    from lcv_hip import build as B
    dst = tmp_path_factory.mktemp("gaps") / "attn_fwd_w64.s"
    name = "attn_fwd_w64.hip"
    cmd = [B.HIPCC, *B.FLAGS, *B.EXTRA.get(name, []), "--cuda-device-only", "-S", str(B.CSRC / name), "-o", str(dst)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return dst.read_text()


def test_the_steady_loop_keeps_the_gap_table(w64_isa):
    _, insts, gaps = G.kernel_gaps(w64_isa, "attn_fwd_w64_kernel")
    assert sum(i.op.startswith("v_mfma") for i in G.loop_insts(insts)) == 128      # two 64-key iterations
    assert sum(g.trans for g in gaps) == 128                                        # every exp inside an MFMA shadow
    findings = check(w64_isa)
    assert not findings, "\n".join(findings)


# ---------------------------------------------------------------------------------------------------------------- bent stand-ins
_HEAD = "_Z4bentv:\n"
_MFMA = "\tv_mfma_f32_32x32x16_bf16 v[0:15], v[100:103], a[4:7], v[0:15]\n"
_LOOP = ".LBB0_1:\n{body}\ts_cmp_lt_u32 s4, s5\n\ts_cbranch_scc1 .LBB0_1\n\ts_endpgm\n.Lfunc_end0:\n"


def _kernel(gap: str) -> str:
    return _HEAD + _LOOP.format(body=(_MFMA + "\tv_exp_f32 v1, v2\n\tv_add_f32_e32 v3, v3, v1\n") * 3 + _MFMA + gap + _MFMA)


BENT = {
    "packed_sum": "\tv_pk_add_f32 v[4:5], v[4:5], v[6:7]\n",
    "three_exps": "\tv_exp_f32 v1, v2\n" * 3,
    "too_many_issues": "\tv_add_f32_e32 v3, v3, v1\n" * (MAX_ISSUES + 1),
    "too_many_cycles": "\tv_exp_f32 v1, v2\n" * 2 + "\tv_cvt_pk_bf16_f32 v9, v1, v2\n" * 5 + "\ts_nop 7\n",
}


def test_the_stand_in_loop_is_clean():
    assert not check(_kernel("\tv_add_f32_e32 v3, v3, v1\n"))


@pytest.mark.parametrize("name", sorted(BENT))
def test_the_guard_fails_on_a_bent_gap(name):
    assert check(_kernel(BENT[name]))

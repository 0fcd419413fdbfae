"""CPU: the normaliser of tools/isa_equal.py on canned listings - a renamed parameter struct (the type suffix of a mangled name)
compares equal; a changed instruction, register count or kernarg size does not."""
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tools"))
import isa_equal as E  # noqa: E402

LISTING = """\t.text
\t.file\t"{file}"
\t.protected\t{sym} ; -- Begin function {sym}
\t.globl\t{sym}
\t.type\t{sym},@function
{sym}: ; @{sym}
; %bb.0:
\ts_load_dwordx2 s[2:3], s[0:1], 0x0
.LBB{fn}_1: ; =>This Inner Loop Header: Depth=1
\t{inst}
\ts_cbranch_scc1 .LBB{fn}_1
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel {sym}
\t\t.amdhsa_kernarg_size {kernarg}
\t\t.amdhsa_next_free_vgpr {vgpr}
\t.end_amdhsa_kernel
\t.text
.Lfunc_end{fn}:
\t.size\t{sym}, .Lfunc_end{fn}-{sym}
\t.ident\t"clang {file}"
\t.amdgpu_metadata
    .kernarg_segment_size: {kernarg}
    .name:           {sym}
    .symbol:         {sym}.kd
\t.end_amdgpu_metadata
"""
BASE = dict(file="a.hip", sym="_Z15attn_fwd_kernelILi8ELi0ELb1ELi0EEv13AttnFwdParams", fn=2, inst="v_exp_f32_e32 v1, v2", kernarg=176, vgpr=128)


def listing(**kw):
    return LISTING.format(**{**BASE, **kw})


def test_a_renamed_parameter_struct_file_and_function_index_compare_equal():
    new = listing(file="b.hip", sym="_Z15attn_fwd_kernelILi8ELi0ELb1ELi0EEv10FwdParams2", fn=0)
    n = E.normalise(new)
    assert set(n) == {"attn_fwd_kernelILi8ELi0ELb1ELi0EE", "(metadata)"}
    assert "v_exp_f32_e32 v1, v2" in n["attn_fwd_kernelILi8ELi0ELb1ELi0EE"] and ".amdhsa_kernarg_size 176" in n["attn_fwd_kernelILi8ELi0ELb1ELi0EE"]
    report = E.compare(listing(), new)
    assert len(report) == 2 and all("identical" in r for r in report), report


@pytest.mark.parametrize("change", [dict(inst="v_exp_f32_e32 v1, v3"), dict(vgpr=136), dict(kernarg=184)])
def test_a_changed_instruction_register_count_or_kernarg_size_compares_unequal(change):
    report = E.compare(listing(), listing(**change))
    assert any("DIFFERS" in r for r in report), report


def test_another_instantiation_is_another_kernel():
    report = E.compare(listing(), listing(sym="_Z15attn_fwd_kernelILi8ELi0ELb0ELi3EEv13AttnFwdParams"))
    assert sum("only in" in r for r in report) == 2, report

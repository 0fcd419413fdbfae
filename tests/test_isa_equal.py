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


def test_a_differing_kernel_is_told_whether_its_arithmetic_differs():
    """Registers renamed (and an fma spelled as the tied-register fmac): `same fp ops`; an fma split into a mul and an add:
    `fp ops differ`, with what went and what came.  A changed register count or LDS size is named beside either verdict."""
    lds = "\n\t\t.amdhsa_group_segment_fixed_size {}"
    body = "v_mul_f32_e32 v1, v2, v3\n\tv_fma_f32 v4, v1, v5, v6\n\tv_rcp_f32_e32 v7, v4\n\tglobal_store_dword v[8:9], v7, off"
    old = listing(inst=body, vgpr="10" + lds.format(32))
    renamed = listing(inst="v_mul_f32_e32 v2, v1, v3\n\tv_fmac_f32_e32 v6, v2, v5\n\tv_rcp_f32_e32 v7, v6\n\tglobal_store_dword v[8:9], v7, off",
                      vgpr="10" + lds.format(32))
    report = [r for r in E.compare(old, renamed) if r.startswith("attn_fwd_kernel")]
    assert len(report) == 1 and "DIFFERS" in report[0] and "same fp ops (3 floating-point VALU instructions)" in report[0], report
    assert "next_free_vgpr 10, LDS bytes 32 (unchanged)" in report[0], report
    split = listing(inst=body.replace("v_fma_f32 v4, v1, v5, v6", "v_mul_f32_e32 v4, v1, v5\n\tv_add_f32_e32 v4, v4, v6"),
                    vgpr="12" + lds.format(48))
    report = [r for r in E.compare(old, split) if r.startswith("attn_fwd_kernel")]
    assert len(report) == 1 and "DIFFERS" in report[0] and "same fp ops" not in report[0], report
    assert "fp ops differ: -1xv_fma_f32 +1xv_add_f32 +1xv_mul_f32" in report[0], report
    assert "next_free_vgpr 10 -> 12, LDS bytes 32 -> 48 (CHANGED)" in report[0], report
    assert all("fp ops" not in r for r in E.compare(old, old)), "an identical kernel gets no verdict"


def test_a_renamed_kernel_in_another_file_compares_equal_under_its_new_name():
    """--map: `tn_skinny_dropout_kernel` of one file against `tn_skinny_kernel<8, drop_args>` of another."""
    old = listing(file="lora_dropout.hip", sym="_Z24tn_skinny_dropout_kernelPKtS1_lli9drop_args", fn=1)
    plain = listing(file="lora.hip", sym="_Z16tn_skinny_kernelILi8EJEEvPKtS1_PflDpT0_", fn=3, inst="v_pk_fma_f32 v[0:1], v[2:3]")
    sym = "_Z16tn_skinny_kernelILi8EJ9drop_argsEEvPKtS1_PflDpT0_"
    rename = {"tn_skinny_dropout_kernel": "tn_skinny_kernelILi8EJ9drop_argsEE"}
    report = E.compare(old, plain + listing(file="lora.hip", sym=sym, fn=4), rename=rename)
    assert len(report) == 1 and report[0].startswith("tn_skinny_kernelILi8EJ9drop_argsEE: identical"), report   # the empty pack is another kernel
    report = E.compare(old, plain + listing(file="lora.hip", sym=sym, fn=4, inst="v_exp_f32_e32 v1, v3"), rename=rename)
    assert len(report) == 1 and "DIFFERS" in report[0], report
    assert "only in the new" in E.compare(old, plain, rename={"no_such_kernel": "tn_skinny_kernelILi8EJEE"})[0]


def test_another_instantiation_is_another_kernel():
    report = E.compare(listing(), listing(sym="_Z15attn_fwd_kernelILi8ELi0ELb0ELi3EEv13AttnFwdParams"))
    assert sum("only in" in r for r in report) == 2, report

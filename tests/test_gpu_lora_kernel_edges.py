"""GPU: the LoRA kernels (lcv_tn_skinny: every dA / dB; lcv_lora_down: every LoRA forward and g = s dy B) element by element
against the float64 restatements of tests/kernel_ref.py (`check_tn_skinny`, `check_lora_down`: the bound and its derivation
sit next to the assert there), at the shapes where they go wrong: one row, partial batches of 8 rows, a single live lane or
rank, the row-group cap, both row-group counts, a strided x, every template of lora_down at both ends of its rank range and a
K loop of one, two and three passes.  The masked forms (lcv_tn_skinny_dropout, lcv_lora_down_dropout) are held at the same shapes to
what they are by definition: the plain kernel on the dropped input, bit for bit.  Conventions of tests/test_gpu_kernel_edges.py: `lib.call` with caller-owned buffers,
outputs NaN-filled, every input a view into a larger buffer whose guard rows and pad columns hold NaN, so that a read one
element off shows up as a NaN in the result.
"""
import pytest
import torch

import kernel_ref as K
import lora_dropout_ref as D
from edge_buffers import BF16, DEV, F32, GUARD, NAN, call as _call, f32, guarded as _guarded, ptr as _p

pytestmark = pytest.mark.gpu

S037 = f32(0.37)       # the fp32 value the kernel receives for 0.37


# ------------------------------------------------------------------------------------------------------ lcv_tn_skinny
_TN_SHAPES = [
    # M, K, ldx, R, Rpad
    (1, 8, 8, 1, 8),             # one row: three waves have nothing to do, one lane has a column
    (4097, 520, 520, 9, 64),     # rpb 96, 43 groups, the last of 65 rows: a wave ends on a partial batch of 8; the second
                                 # column block has one live lane, the second rank launch one live rank
    (66000, 8, 8, 32, 32),       # rpb capped at 1024: 65 groups
    (2049, 4104, 4112, 8, 8),    # the 32-group branch (9 column blocks), a strided x
]


def _tn_inputs(M, K_, ldx, R, Rpad):
    g = _guarded(M, Rpad, Rpad, seed=101)
    g[:, R:] = NAN                                     # the pad ranks of g are never read
    x = _guarded(M, K_, ldx, seed=102)
    K.tn_tail_row(g, x, R)                             # a lost tail row must show at every depth (see tn_tail_row)
    return g, x


def _tn_ws(M, K_, R):
    from lcv_hip import lib
    need = lib.load().lcv_tn_skinny_ws_bytes(M, K_, R)
    rpb, groups = K.tn_skinny_rpb(M, K_)
    assert need == groups * R * K_ * 4, (need, rpb, groups)      # the restated tn_skinny_rpb is the code's own
    return need


@pytest.mark.parametrize("M,K_,ldx,R,Rpad", _TN_SHAPES)
def test_tn_skinny_workspace_path_edges(M, K_, ldx, R, Rpad):
    g, x = _tn_inputs(M, K_, ldx, R, Rpad)
    need = _tn_ws(M, K_, R)
    ws = torch.full((need // 4,), NAN, dtype=F32, device=DEV)
    scale = S037
    buf = torch.full((R + 2 * GUARD, K_), 7.5, dtype=F32, device=DEV)     # guard rows around `out` hold 7.5
    out = buf[GUARD: GUARD + R]
    out.fill_(NAN)                                                         # overwritten in full, never accumulated into
    _call("lcv_tn_skinny", _p(g), _p(x), _p(out), M, K_, R, Rpad, ldx, scale, _p(ws), need)
    K.check_tn_skinny(out, g, x, R, scale, f"tn_skinny ws M={M} K={K_} R={R}")
    assert (buf[:GUARD] == 7.5).all() and (buf[GUARD + R:] == 7.5).all(), "tn_skinny wrote outside out[R, K]"
    out2 = torch.full((R, K_), NAN, dtype=F32, device=DEV)
    ws.fill_(NAN)
    _call("lcv_tn_skinny", _p(g), _p(x), _p(out2), M, K_, R, Rpad, ldx, scale, _p(ws), need)
    K.assert_bits(out2, out.contiguous(), what="tn_skinny ws: a second call")      # fixed order: the same bits


@pytest.mark.parametrize("M,K_,ldx,R,Rpad", _TN_SHAPES)
def test_tn_skinny_atomic_path_edges(M, K_, ldx, R, Rpad):
    g, x = _tn_inputs(M, K_, ldx, R, Rpad)
    scale = 2.0
    buf = torch.full((R + 2 * GUARD, K_), 7.5, dtype=F32, device=DEV)
    out = buf[GUARD: GUARD + R]
    out.zero_()                                                            # ws == NULL: accumulated into, caller zero-fills
    _call("lcv_tn_skinny", _p(g), _p(x), _p(out), M, K_, R, Rpad, ldx, scale, None, 0)
    K.check_tn_skinny(out, g, x, R, scale, f"tn_skinny atomic M={M} K={K_} R={R}")
    assert (buf[:GUARD] == 7.5).all() and (buf[GUARD + R:] == 7.5).all(), "tn_skinny wrote outside out[R, K]"


def test_tn_skinny_rejects_a_small_or_misaligned_workspace():
    from lcv_hip.lib import LcvError
    M, K_, ldx, R, Rpad = 300, 520, 520, 9, 16
    g, x = _tn_inputs(M, K_, ldx, R, Rpad)
    need = _tn_ws(M, K_, R)
    ws = torch.full((need // 4 + 4,), NAN, dtype=F32, device=DEV)
    out = torch.full((R, K_), NAN, dtype=F32, device=DEV)
    for ptr, size in ((ws.data_ptr(), need - 4), (ws.data_ptr() + 4, need)):
        with pytest.raises(LcvError) as e:
            _call("lcv_tn_skinny", _p(g), _p(x), _p(out), M, K_, R, Rpad, ldx, 1.0, ptr, size)
        assert e.value.code == -1
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(ws).all()               # nothing ran


# ------------------------------------------------------------------------------------------------------ lcv_lora_down
# s = 2.0 is a power of two: bf16(2 * bf16(t)) is exact, so those cases cannot tell the outer rounding from its absence; the
# S037 cases (one per template) are the ones that exercise both roundings of rule 5.
_DOWN_SHAPES = [
    (1, 8, 1, 8, 2.0),          # <8> at R = 1; one row (three of the wave's four rows clamped), one live lane
    (5, 520, 8, 8, S037),       # <8> at R = 8 = Rpad; the K loop's second pass has one live lane; a wave with one live row
    (18, 1032, 9, 16, 2.0),     # <16> at R = 9; three K passes; two workgroups, the second with two rows
    (5, 1032, 16, 64, S037),    # <16> at R = 16, the widest pad
    (18, 520, 17, 24, 2.0),     # <32> at R = 17
    (1, 1032, 32, 32, S037),    # <32> at R = 32 = Rpad
    (18, 8, 32, 64, 2.0),       # <32> at R = 32, K of one packet, the widest pad
]


@pytest.mark.parametrize("M,K_,R,Rpad,s", _DOWN_SHAPES)
def test_lora_down_edges(M, K_, R, Rpad, s):
    x = _guarded(M, K_, K_ + 8, seed=111)                                  # ldx > K
    A = _guarded(R, K_, K_, seed=112, scale=0.5)
    h = torch.full((M + 2 * GUARD, Rpad), NAN, dtype=BF16, device=DEV)
    out = h[GUARD: GUARD + M]
    _call("lcv_lora_down", _p(x), _p(A), _p(out), M, K_, R, Rpad, K_ + 8, s)
    K.check_lora_down(out, x, A, R, Rpad, s, f"lora_down M={M} K={K_} R={R}/{Rpad} s={s}")
    assert torch.isnan(h[:GUARD].float()).all() and torch.isnan(h[GUARD + M:].float()).all(), "lora_down wrote outside h[M, Rpad]"


def test_lora_down_rejects_rank_33():
    from lcv_hip.lib import LcvError
    x, A = _guarded(4, 64, 64, seed=113), _guarded(33, 64, 64, seed=114)
    h = torch.full((4, 64), NAN, dtype=BF16, device=DEV)
    with pytest.raises(LcvError) as e:
        _call("lcv_lora_down", _p(x), _p(A), _p(h), 4, 64, 33, 64, 64, 1.0)
    assert e.value.code == -1
    torch.cuda.synchronize()
    assert torch.isnan(h.float()).all()


# ------------------------------------------------------------------------- the masked forms are the plain forms on xd
SEED, OFFSET = (3 << 32) | 1234, (1 << 32) | 8          # both halves of seed and offset in use
BIG = 1 << 33                                           # a first row whose element index needs 64 bits
_DRAWS = [(0.5, 0), (0.1, 5), (0.5, BIG), (0.1, BIG)]   # (p, row0), dealt over the shapes in turn


def _dropped(x, ld, p, row0, seed):
    """xd = bf16(x * scale) where lcv_lora_dropout_mask keeps the element and +0 where it drops it, built on the device in a
    guarded buffer of its own (NaN guard rows and pad columns, as x)."""
    M, K_ = x.shape
    mask = torch.empty((M, K_), dtype=torch.uint8, device=DEV)
    _call("lcv_lora_dropout_mask", _p(mask), M, K_, p, SEED, OFFSET, row0)
    assert 0 < int(mask.sum()) < mask.numel() or mask.numel() == 8
    xd = _guarded(M, K_, ld, seed=seed)
    xd.copy_(torch.where(mask.bool(), (x.float() * float(D.scale(p))).to(BF16), torch.zeros((), dtype=BF16, device=DEV)))
    return xd


@pytest.mark.parametrize("shape,draw", list(zip(_TN_SHAPES, _DRAWS)))
def test_tn_skinny_dropout_is_tn_skinny_on_the_dropped_input(shape, draw):
    (M, K_, ldx, R, Rpad), (p, row0) = shape, draw
    g, x = _tn_inputs(M, K_, ldx, R, Rpad)               # the heavy last row included
    xd = _dropped(x, ldx, p, row0, seed=103)
    need = _tn_ws(M, K_, R)
    from lcv_hip import lib
    assert lib.load().lcv_tn_skinny_dropout_ws_bytes(M, K_, R) == need
    ws = torch.full((need // 4,), NAN, dtype=F32, device=DEV)
    outs = []
    for name, src, draw_args in (("lcv_tn_skinny_dropout", x, (p, SEED, OFFSET, row0)), ("lcv_tn_skinny", xd, ())):
        buf = torch.full((R + 2 * GUARD, K_), 7.5, dtype=F32, device=DEV)     # guard rows around `out` hold 7.5
        out = buf[GUARD: GUARD + R]
        out.fill_(NAN)
        ws.fill_(NAN)
        _call(name, _p(g), _p(src), _p(out), M, K_, R, Rpad, ldx, S037, *draw_args, _p(ws), need)
        assert (buf[:GUARD] == 7.5).all() and (buf[GUARD + R:] == 7.5).all(), f"{name} wrote outside out[R, K]"
        outs.append(out.contiguous())
    assert not torch.isnan(outs[1]).any()
    K.assert_bits(outs[0], outs[1], what=f"tn_skinny_dropout vs tn_skinny on xd, M={M} K={K_} R={R} p={p} row0={row0}")


@pytest.mark.parametrize("shape,draw", list(zip(_DOWN_SHAPES, _DRAWS + _DRAWS)))
def test_lora_down_dropout_is_lora_down_on_the_dropped_input(shape, draw):
    (M, K_, R, Rpad, s), (p, row0) = shape, draw
    x = _guarded(M, K_, K_ + 8, seed=111)                                  # ldx = K + 8
    A = _guarded(R, K_, K_, seed=112, scale=0.5)
    xd = _dropped(x, K_ + 8, p, row0, seed=113)
    outs = []
    for name, src, draw_args in (("lcv_lora_down_dropout", x, (p, SEED, OFFSET, row0)), ("lcv_lora_down", xd, ())):
        h = torch.full((M + 2 * GUARD, Rpad), NAN, dtype=BF16, device=DEV)
        out = h[GUARD: GUARD + M]
        _call(name, _p(src), _p(A), _p(out), M, K_, R, Rpad, K_ + 8, s, *draw_args)
        assert torch.isnan(h[:GUARD].float()).all() and torch.isnan(h[GUARD + M:].float()).all(), f"{name} wrote outside h[M, Rpad]"
        outs.append(out.contiguous())
    assert not torch.isnan(outs[1].float()).any()
    K.assert_bits(outs[0], outs[1], what=f"lora_down_dropout vs lora_down on xd, M={M} K={K_} R={R}/{Rpad} p={p} row0={row0}")
    assert (outs[0][:, R:].view(torch.int16) == 0).all(), "pad columns must be exactly +0"

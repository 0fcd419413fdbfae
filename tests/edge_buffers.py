"""What the GPU edge tests of the LoRA, backward, UMT5 and attention kernels share (tests/test_gpu_{lora,bwd,umt5,attn}_kernel_edges.py): the call
through the C ABI and the guard convention.  Every input is a view into a larger buffer whose guard rows and pad columns hold
NaN, every output a NaN-filled view of the same kind, so that a read or a write one element off shows up in the result instead
of as a fault.  A plain helper module (compare tests/kernel_ref.py)."""
import torch

BF16, F32 = torch.bfloat16, torch.float32
DEV = "cuda"
NAN = float("nan")
GUARD = 2                  # guard rows in front of and behind every view
CAP = 4096 * 256           # packets of 8 one launch covers before its grid-stride loop takes a second pass


def call(name, *args):
    from lcv_hip import lib
    lib.call(name, *args, torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return None if t is None else t.data_ptr()


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def f32(v):
    """The fp32 value the kernel receives for a Python float."""
    return float(torch.tensor(v, dtype=F32))


def guarded(rows, cols, ld, seed, scale=1.0, dtype=BF16):
    """A [rows, cols] view (row stride ld >= cols) holding scale * randn inside a NaN-filled buffer with GUARD rows on either
    side."""
    buf = torch.full((rows + 2 * GUARD, ld), NAN, dtype=dtype, device=DEV)
    view = buf[GUARD: GUARD + rows, :cols]
    view.copy_((torch.randn(rows, cols, generator=gen(seed), device=DEV) * scale).to(dtype))
    return view


def nan_out(rows, cols, dtype=BF16, ld=None):
    """-> (buffer with GUARD rows on either side, its [rows, cols] middle with row stride ld), all NaN."""
    buf = torch.full((rows + 2 * GUARD, ld or cols), NAN, dtype=dtype, device=DEV)
    return buf, buf[GUARD: GUARD + rows, :cols]


def only_written(buf, n_written, what):
    """The checked views hold no NaN (assert_within fails on one), so whatever else of `buf` was written shows here."""
    assert int(torch.isnan(buf.float()).sum()) == buf.numel() - n_written, f"{what}: written outside its output view"

"""GPU: lcv_attn_fwd and lcv_attn_bwd held per element (tests/kernel_ref.py: check_attn_fwd, check_attn_bwd) at the tile and split
edges of every body the library can pick, on the inputs of tests/attn_cases.py: exact scores, heavy keys at the ragged edges, the
rescale pattern of the deferred running max, distinct heads.  What tests/test_kernel_ref.py proves about these checks on the CPU
(the documented arithmetic passes, a doubled or dropped edge key, a swapped row or head, a missed rescale, a lost tile or split
slice, a wrong accumulate_kv fail) is what makes a pass here mean something.

Layout of every case.  q and k are slots 0 and 1 of one [B, max(Nq, Nk), 2, H, D] buffer, v is slot 2 of a [B, Nk, 3, H, D] buffer
(unequal K / V row strides); the rows past Nq / Nk and the unused slots hold NaN: the header addresses only rows < N, and the
kernels clamp their tail reads to the last row.  Every output is a view into a NaN-filled buffer and nothing but the view may
be written; the backward's workspace is exactly lcv_attn_bwd_ws_floats floats between canary words.
"""
import pytest
import torch

import attn_cases as AC
import kernel_ref as K
from edge_buffers import BF16, DEV, F32, GUARD, NAN, call, only_written, ptr

pytestmark = pytest.mark.gpu

D = AC.D
CANARY, NCAN = 0x5A5A5A5A, 64


def _last_kernel():
    from lcv_hip import lib as L
    return L.load().lcv_attn_fwd_last_kernel().decode()


def _knobs():
    from lcv_hip import lib as L
    return L.load().lcv_knobs_list().decode().split()


def _slots(c, Nq, Nk):
    """q, k, v of case `c` as views into NaN-filled buffers."""
    B, _, H, _ = c["q"].shape
    qk = torch.full((B, max(Nq, Nk), 2, H, D), NAN, dtype=BF16, device=DEV)
    qkv = torch.full((B, Nk, 3, H, D), NAN, dtype=BF16, device=DEV)
    qk[:, :Nq, 0], qk[:, :Nk, 1], qkv[:, :, 2] = c["q"].to(DEV), c["k"].to(DEV), c["v"].to(DEV)
    return qk[:, :Nq, 0], qk[:, :Nk, 1], qkv[:, :, 2]


def _out(B, N, H, sh=D, shift=0):
    """-> (NaN-filled flat buffer, its [B, N, H, D] view with head stride sh, GUARD rows around every batch, `shift` elements in)."""
    sn = H * sh
    sb = (N + 2 * GUARD) * sn
    flat = torch.full((B * sb + shift + 8,), NAN, dtype=BF16, device=DEV)
    return flat, flat.as_strided((B, N, H, D), (sb, sn, sh, 1), shift + GUARD * sn)


def _lse_out(B, H, Nq):
    buf = torch.full((B * H * Nq + 16,), NAN, dtype=F32, device=DEV)
    return buf, buf[8: 8 + B * H * Nq].view(B, H, Nq)


def _st(t):
    return t.stride(0), t.stride(1), t.stride(2)


def _fwd(q, k, v, o, lse, scale, strides=None):
    B, Nq, H, _ = q.shape
    call("lcv_attn_fwd", ptr(q), ptr(k), ptr(v), ptr(o), ptr(lse), B, H, Nq, k.shape[1],
         *(strides or (*_st(q), *_st(k), *_st(v), *_st(o))), scale)


# ------------------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("body,Nq,Nk,unit,knob", AC.FWD_CASES)
def test_attn_fwd_edges(body, Nq, Nk, unit, knob, monkeypatch):
    assert "LCV_ATTN_FWD_W64" in _knobs()
    if knob is None:
        monkeypatch.delenv("LCV_ATTN_FWD_W64", raising=False)
    else:
        monkeypatch.setenv("LCV_ATTN_FWD_W64", knob)
    B, H = AC.B0, AC.H0
    c = AC.inputs(Nq, Nk, unit)
    q, k, v = _slots(c, Nq, Nk)
    # every other case: o at an 8-byte- but not 16-byte-aligned address with a head stride of 132 - what the argument check allows
    odd = (Nq + Nk) % 2 == 0
    obuf, o = _out(B, Nq, H, 132 if odd else D, 4 if odd else 0)
    assert o.data_ptr() % 16 == (8 if odd else 0)
    lbuf, lse = _lse_out(B, H, Nq)
    what = f"attn_fwd {body} Nq={Nq} Nk={Nk} unit={unit}"
    _fwd(q, k, v, o, lse, c["scale"])
    assert _last_kernel() == body
    K.check_attn_fwd(o, lse, q, k, v, c["scale"], what, exact_scores=True)
    only_written(obuf, B * Nq * H * D, what)
    only_written(lbuf, B * H * Nq, what + " lse")
    # without lse (need_lse=False): the same body, the same bits
    obuf2, o2 = _out(B, Nq, H, 132 if odd else D, 4 if odd else 0)
    _fwd(q, k, v, o2, None, c["scale"])
    assert _last_kernel() == body and torch.equal(o2, o)
    only_written(obuf2, B * Nq * H * D, what + " without lse")


def test_attn_fwd_wide_key_stride_takes_the_64_bit_body():
    """attn_fwd_kernel<8, 0, false, 3> (unit scale, Nk > 512, one (batch, head)'s keys spanning >= 4 GiB) through a key STRIDE
    instead of a very large tensor: K and V are the two slots of one uninitialised buffer whose key stride is the smallest
    multiple of 8 with Nk k_sn 2 >= 2^32; only the 513 used rows are ever written or read."""
    B, H, Nq, Nk = (AC.WIDE_CASE[n] for n in ("B", "H", "Nq", "Nk"))
    c = AC.inputs(Nq, Nk, True, B, H)
    sn = (-(-(1 << 32) // (2 * Nk)) + 7) // 8 * 8
    assert Nk * sn * 2 >= 1 << 32 > Nk * (sn - 8) * 2
    kv = torch.empty(Nk * sn, dtype=BF16, device=DEV)
    rows = kv.view(Nk, sn)[:, : 2 * H * D].unflatten(1, (2, H, D))
    rows[:, 0], rows[:, 1] = c["k"][0].to(DEV), c["v"][0].to(DEV)
    k, v = rows[:, 0].unsqueeze(0), rows[:, 1].unsqueeze(0)
    q = torch.full((B, Nq + 2 * GUARD, H, D), NAN, dtype=BF16, device=DEV)[:, GUARD: GUARD + Nq]
    q.copy_(c["q"].to(DEV))
    obuf, o = _out(B, Nq, H)
    lbuf, lse = _lse_out(B, H, Nq)
    _fwd(q, k, v, o, lse, c["scale"], strides=(*_st(q), Nk * sn, sn, D, Nk * sn, sn, D, *_st(o)))
    assert _last_kernel() == AC.FWD_WIDE
    what = f"attn_fwd {AC.FWD_WIDE} Nq={Nq} Nk={Nk} k_sn={sn}"
    K.check_attn_fwd(o, lse, q, k, v, c["scale"], what, exact_scores=True)
    only_written(obuf, B * Nq * H * D, what)
    only_written(lbuf, B * H * Nq, what + " lse")
    del kv, rows, k, v
    torch.cuda.empty_cache()


def test_attn_fwd_without_queries_is_ok_and_writes_nothing():
    c = AC.inputs(33, 77, False)
    q, k, v = _slots(c, 33, 77)
    obuf, o = _out(AC.B0, 33, AC.H0)
    lbuf, lse = _lse_out(AC.B0, AC.H0, 33)
    call("lcv_attn_fwd", ptr(q), ptr(k), ptr(v), ptr(o), ptr(lse), AC.B0, AC.H0, 0, 77, *_st(q), *_st(k), *_st(v), *_st(o), c["scale"])
    torch.cuda.synchronize()
    only_written(obuf, 0, "attn_fwd Nq=0")
    only_written(lbuf, 0, "attn_fwd Nq=0 lse")


# ----------------------------------------------------------------------------------------------------------------- backward
class _Bwd:
    """One case's device inputs: q, k, v as in the forward tests; o_in = bf16(o64) and dO as the two slots of one NaN-filled
    [B, Nq, 2, H, D] buffer (d_o shares o's strides); lse_in = fp32(logsumexp64) between NaN guards.  o_in and lse_in come from
    the float64 reference, not from the forward kernel."""

    def __init__(self, Nq, Nk, unit, B=AC.B0, H=AC.H0):
        self.B, self.H, self.Nq, self.Nk, self.unit = B, H, Nq, Nk, unit
        # (the two 255 / 256-head cases are used once: built without the cache that keeps the small ones)
        self.c = c = (AC.inputs if AC.is_small(B, H, Nq, Nk) else AC.inputs.__wrapped__)(Nq, Nk, unit, B, H)
        self.scale = c["scale"]
        self.q, self.k, self.v = _slots(c, Nq, Nk)
        o64, lse64, _, _ = K.attn_fwd(self.q, self.k, self.v, self.scale)
        og = torch.full((B, Nq, 2, H, D), NAN, dtype=BF16, device=DEV)
        og[:, :, 0], og[:, :, 1] = o64.permute(0, 2, 1, 3).to(BF16), c["d_o"].to(DEV)
        self.o_in, self.d_o = og[:, :, 0], og[:, :, 1]
        self.lbuf, self.lse_in = _lse_out(B, H, Nq)
        self.lse_in.copy_(lse64.to(F32))
        self.n_ws = AC.ws_floats(B, H, Nq, Nk)
        self.prev_dk, self.prev_dv = c["prev_dk"].to(DEV), c["prev_dv"].to(DEV)

    def run(self, accumulate=False):
        """One call into fresh NaN-filled gradient buffers and a fresh workspace -> dq, dk, dv (views).  Asserts that nothing but
        the views was written and that the canaries around the workspace are intact."""
        from lcv_hip import lib as L
        B, H, Nq, Nk = self.B, self.H, self.Nq, self.Nk
        assert L.load().lcv_attn_bwd_ws_floats(B, H, Nq, Nk) == self.n_ws
        dqk = torch.full((B, max(Nq, Nk), 2, H, D), NAN, dtype=BF16, device=DEV)
        dqkv = torch.full((B, Nk, 3, H, D), NAN, dtype=BF16, device=DEV)
        dq, dk, dv = dqk[:, :Nq, 0], dqk[:, :Nk, 1], dqkv[:, :, 2]
        if accumulate:
            dk.copy_(self.prev_dk)
            dv.copy_(self.prev_dv)
        wbuf = torch.full((self.n_ws + 2 * NCAN,), NAN, dtype=F32, device=DEV)
        can = wbuf.view(torch.int32)
        can[:NCAN] = CANARY
        can[NCAN + self.n_ws:] = CANARY
        ws = wbuf[NCAN: NCAN + self.n_ws]
        call("lcv_attn_bwd", ptr(self.q), ptr(self.k), ptr(self.v), ptr(self.o_in), ptr(self.d_o), ptr(self.lse_in),
             ptr(dq), ptr(dk), ptr(dv), ptr(ws), int(accumulate), B, H, Nq, Nk,
             *_st(self.q), *_st(self.k), *_st(self.v), *_st(self.o_in), *_st(dq), *_st(dk), *_st(dv), self.scale)
        what = f"attn_bwd Nq={Nq} Nk={Nk} unit={self.unit}"
        assert bool((can[:NCAN] == CANARY).all()) and bool((can[NCAN + self.n_ws:] == CANARY).all()), f"{what}: written outside the workspace"
        only_written(dqk, B * H * D * (Nq + Nk), what + " dq / dk")
        only_written(dqkv, B * Nk * H * D, what + " dv")
        return dq, dk, dv

    def check(self, grads, scale_inside, form, accumulate=False, qsplit=1):
        prev = (self.prev_dk, self.prev_dv) if accumulate else (None, None)
        what = f"attn_bwd {form} Nq={self.Nq} Nk={self.Nk} B={self.B} H={self.H}" + (" accumulate_kv" if accumulate else "")
        return K.check_attn_bwd(*grads, self.q, self.k, self.v, self.o_in, self.d_o, self.lse_in, self.scale, scale_inside, *prev,
                                what=what, qsplit=qsplit, exact_scores=True)

    def twice(self):
        """Two calls: the same bits."""
        a = self.run()
        b = self.run()
        assert all(torch.equal(x, y) for x, y in zip(a, b)), "attn_bwd: a second call gave other bits"
        return a


@pytest.mark.parametrize("Nq,Nk", AC.BWD_CASES)
def test_attn_bwd_edges(Nq, Nk, monkeypatch):
    knobs = _knobs()
    for name in ("LCV_ATTN_BWD_VAR", "LCV_ATTN_BWD_DQ_WAVES"):
        assert name in knobs, f"{name} is no knob of the library any more: the forms below would be one kernel run twice"
        monkeypatch.delenv(name, raising=False)
    assert AC.qsplit(AC.B0, AC.H0, Nq, Nk) == 1
    # general scale: the first form (dS = P (dP - delta) scale is the bf16 operand)
    g = _Bwd(Nq, Nk, False)
    g.check(g.twice(), True, "first form")
    g.check(g.run(accumulate=True), True, "first form", accumulate=True)
    # unit scale: the second form (dS' = P (dP - delta) is the operand, the scale follows the sum), pass B with 4 and 8 waves
    u = _Bwd(Nq, Nk, True)
    outs = {}
    for waves in ("4", "8"):
        monkeypatch.setenv("LCV_ATTN_BWD_DQ_WAVES", waves)
        outs[waves] = u.twice()
        u.check(outs[waves], False, f"second form, {waves}-wave pass B")
    assert all(torch.equal(a, b) for a, b in zip(outs["4"], outs["8"])), "the two pass-B forms differ"
    monkeypatch.delenv("LCV_ATTN_BWD_DQ_WAVES")
    u.check(u.run(accumulate=True), False, "second form", accumulate=True)
    # ... and the same unit-scale inputs through the first-form kernels
    monkeypatch.setenv("LCV_ATTN_BWD_VAR", "0")
    first = u.twice()
    u.check(first, True, "first form on unit-scale inputs")
    # the knob did select other kernels: dS is rounded on the other side of ln 2, so with more than one key some bits of dq or dk
    # differ (the rounding-point restatements of the two forms differ at every such shape)
    if Nk > 1:
        assert not (torch.equal(first[0], outs["4"][0]) and torch.equal(first[1], outs["4"][1])), "LCV_ATTN_BWD_VAR=0 changed nothing"


@pytest.mark.parametrize("Nq,Nk", AC.SPLIT_CASES)
def test_attn_bwd_split_query_sweep(Nq, Nk, monkeypatch):
    """attn_bwd_qsplit (first form, Nk <= 128): 63 query tiles (no split), 64 (4 splits, the last tile one row), 65 (16 / 16 / 16 / 17)."""
    monkeypatch.delenv("LCV_ATTN_BWD_VAR", raising=False)
    qs = AC.qsplit(AC.B0, AC.H0, Nq, Nk)
    assert qs == (1 if Nq == 2016 else 4)
    g = _Bwd(Nq, Nk, False)
    g.check(g.twice(), True, f"first form, {qs} splits", qsplit=qs)
    g.check(g.run(accumulate=True), True, f"first form, {qs} splits", accumulate=True, qsplit=qs)


@pytest.mark.parametrize("B,H,Nq,Nk", AC.SPLIT_PAIR)
def test_attn_bwd_split_heuristic_at_255_and_256_heads(B, H, Nq, Nk, monkeypatch):
    """B H = 255 splits the sweep in two, 256 does not (the formula of attn_bwd_qsplit's source comment, restated in
    tests/attn_cases.py and asserted against lcv_attn_bwd_ws_floats by every run): a changed heuristic is noticed here."""
    monkeypatch.delenv("LCV_ATTN_BWD_VAR", raising=False)
    qs = AC.qsplit(B, H, Nq, Nk)
    assert qs == (2 if B * H == 255 else 1)
    g = _Bwd(Nq, Nk, False, B, H)
    assert g.n_ws == B * H * (Nq + 2 * Nq) + (qs * B * H * Nk * 256 if qs > 1 else 0)
    g.check(g.run(), True, f"first form, {qs} splits", qsplit=qs)


def test_attn_bwd_refuses_bad_strides_and_misaligned_pointers():
    """LCV_EINVAL and nothing launched: every output and the workspace still hold their NaN fill."""
    from lcv_hip.lib import LcvError
    Nq, Nk, B, H = 33, 77, AC.B0, AC.H0
    g = _Bwd(Nq, Nk, False)
    dqk = torch.full((B, max(Nq, Nk) + 1, 2, H, D), NAN, dtype=BF16, device=DEV)
    dqkv = torch.full((B, Nk + 1, 3, H, D), NAN, dtype=BF16, device=DEV)
    dq, dk, dv = dqk[:, :Nq, 0], dqk[:, :Nk, 1], dqkv[:, :Nk, 2]
    ws = torch.full((g.n_ws + 8,), NAN, dtype=F32, device=DEV)
    ptrs = dict(q=ptr(g.q), k=ptr(g.k), v=ptr(g.v), o=ptr(g.o_in), d_o=ptr(g.d_o), lse=ptr(g.lse_in), dq=ptr(dq), dk=ptr(dk), dv=ptr(dv),
                ws=ptr(ws))
    strides = dict(q=_st(g.q), k=_st(g.k), v=_st(g.v), o=_st(g.o_in), dq=_st(dq), dk=_st(dk), dv=_st(dv))

    def refused(s=None, p=None):
        ss, pp = dict(strides, **(s or {})), dict(ptrs, **(p or {}))
        with pytest.raises(LcvError) as e:
            call("lcv_attn_bwd", *(pp[n] for n in ("q", "k", "v", "o", "d_o", "lse", "dq", "dk", "dv", "ws")), 0, B, H, Nq, Nk,
                 *(x for n in ("q", "k", "v", "o", "dq", "dk", "dv") for x in ss[n]), g.scale)
        assert e.value.code == -1, (s, p, e.value)
        torch.cuda.synchronize()
        assert bool(torch.isnan(dqk.float()).all()) and bool(torch.isnan(dqkv.float()).all()) and bool(torch.isnan(ws).all()), (s, p)

    # strides: inputs in multiples of 8 elements, gradients in multiples of 4
    for n in ("q", "k", "v", "o"):
        for i in range(3):
            refused({n: tuple(x + 4 if j == i else x for j, x in enumerate(strides[n]))})
    for n in ("dq", "dk", "dv"):
        for i in range(3):
            refused({n: tuple(x + 2 if j == i else x for j, x in enumerate(strides[n]))})
    # pointers: 16 bytes for what the packet loads read (as lcv_attn_fwd), 8 bytes for the gradient stores, 4 bytes for the fp32 rows
    for n in ("q", "k", "v", "o", "d_o"):
        refused(p={n: ptrs[n] + 8})
    for n in ("dq", "dk", "dv"):
        refused(p={n: ptrs[n] + 4})
    for n in ("lse", "ws"):
        refused(p={n: ptrs[n] + 2})
    # the aligned call with the right strides goes through (into fresh buffers: the ones above must stay NaN for the asserts)
    g.run()

#!/usr/bin/env python3
"""One sha256 per case over the raw bytes of what the backward / optimizer reductions write, default and fixed-order forms:
the listing of a refactor of csrc/bwd_rows.h, optim_common.h or their users must equal the listing of its parent, line for line.

Usage: python tools/bwd_bits.py [liblcv_hip.so]      (default: the library of this tree; each run a fresh process)

Inputs come from numpy.random.Generator(PCG64(seed)) on the host (a stream that is stable across versions).  Only outputs that
are a function of the inputs are digested: for the default forms that is dx / dy / dq_in / dk_in, and `da` / `norm_coef` where
every atomic adds once onto zero (one slab; tensors of at most 64 chunks).  Shapes: the smallest at which each kernel's edges
are live (S = 50: the default's 32-row workgroup straddles a frame, the fixed-order 64-row one stops at its end; 520 channels =
65 packets, one lane past a wave; 17 heads = a second pass of one head; 17 rows = a second launch of one row)."""
import hashlib
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "longcat-video-tta_amd"))
import torch  # noqa: E402
from lcv_hip import lib  # noqa: E402

BF16, F32, DEV = torch.bfloat16, torch.float32, "cuda"
ADALN, LAYERNORM, GATE, QKNORM, SMALLM, GRAD_NORM = range(6)
_seed = [0]


def rnd(*shape, scale=1.0, shift=0.0, dtype=BF16):
    _seed[0] += 1
    a = np.random.Generator(np.random.PCG64(_seed[0])).standard_normal(shape, dtype=np.float32) * np.float32(scale) + np.float32(shift)
    return torch.from_numpy(a).to(dtype).to(DEV)


def p(t):
    return None if t is None else t.data_ptr()


def call(name, *args):
    lib.call(name, *args, torch.cuda.current_stream().cuda_stream)


def ws(kind, d0, d1=0, d2=0):
    n = int(lib.load().lcv_det_ws_bytes(kind, d0, d1, d2))
    return torch.full((n // 4,), float("nan"), dtype=F32, device=DEV), n


def show(case, *outs):
    h = hashlib.sha256()
    for t in outs:
        h.update(t.contiguous().cpu().view(torch.uint8).numpy().tobytes())
    print(f"{case} {h.hexdigest()}", flush=True)


def rownorm_and_gate(B, T, S, C):
    eps, rows, tag = 1e-6, B * T * S, f"B{B} T{T} S{S} C{C}"
    x, dy, res = rnd(B, T * S, C, scale=0.8, shift=0.3), rnd(B, T * S, C), rnd(B, T * S, C)
    ms, sh, sc = 6 * C, 1 * C, 4 * C
    mod, w = rnd(B, T, ms, scale=0.1, dtype=F32), rnd(C, scale=0.2, shift=1.0, dtype=F32)
    for dres in (None, res):
        t = f"{tag} dres{int(dres is not None)}"
        w1, n1 = ws(ADALN, B * T, S, C)
        dx, dmod = torch.zeros_like(x), torch.zeros_like(mod)
        call("lcv_det_adaln_modulate_bwd", p(x), p(mod), p(dy), p(dx), p(dmod), B, T, S, C, ms, sh, sc, eps, p(dres), p(w1), n1)
        show(f"adaln det {t}", dx, dmod)
        w2, n2 = ws(LAYERNORM, rows, C)
        dx, dw, db = torch.zeros_like(x), torch.zeros_like(w), torch.zeros_like(w)
        call("lcv_det_layernorm_affine_bwd", p(x), p(w), p(dy), p(dx), p(dw), p(db), rows, C, eps, p(dres), p(w2), n2)
        show(f"layernorm det {t}", dx, dw, db)
        for want in (1, 0):
            dx, dmod = torch.zeros_like(x), torch.zeros_like(mod)
            call("lcv_adaln_modulate_bwd", p(x), p(mod), p(dy), p(dx), p(dmod) if want else None, B, T, S, C, ms, sh, sc, eps, p(dres))
            show(f"adaln default {t} dmod{want}", dx)
            dx, dw, db = torch.zeros_like(x), torch.zeros_like(w), torch.zeros_like(w)
            call("lcv_layernorm_affine_bwd", p(x), p(w), p(dy), p(dx), p(dw) if want else None, p(db) if want else None, rows, C, eps, p(dres))
            show(f"layernorm default {t} dw{want}", dx)
    y, dout = rnd(B, T * S, C), rnd(B, T * S, C)
    gms, goff = 3 * C + 16, C + 8
    gmod = rnd(B, T, gms, dtype=F32)
    w3, n3 = ws(GATE, B * T, S, C)
    gy, dg = torch.zeros_like(y), torch.zeros_like(gmod)
    call("lcv_det_gate_residual_bwd", p(y), p(gmod), p(dout), p(gy), p(dg), B, T, S, C, gms, goff, p(w3), n3)
    show(f"gate det {tag}", gy, dg)
    gy, dg = torch.zeros_like(y), torch.zeros_like(gmod)
    call("lcv_gate_residual_bwd", p(y), p(gmod), p(dout), p(gy), p(dg), B, T, S, C, gms, goff)
    show(f"gate default {tag}", gy)


def qknorm(H=17, N=5, B=2, pos_off=3):
    D, eps, qs = 128, 1e-6, 0.1275
    q_in, k_in, dq_out, dk_out = (rnd(B, N, H, D) for _ in range(4))
    wq, wk = rnd(D, scale=0.1, shift=1.0), rnd(D, scale=0.1, shift=1.0)
    ang = rnd(pos_off + N, D // 2, scale=3.0, dtype=F32).cpu().numpy().astype(np.float64)
    cs = torch.from_numpy(np.stack((np.cos(ang), np.sin(ang)), axis=-1).astype(np.float32)).to(DEV)   # host libm, rounded once
    sb, sn = N * H * D, H * D
    for which in ("q", "k", "qk"):
        hq, hk = "q" in which, "k" in which

        def args(dqi, dki, dwq, dwk):
            return (p(q_in) if hq else None, p(k_in) if hk else None, p(dq_out) if hq else None, p(dk_out) if hk else None,
                    p(dqi) if hq else None, p(dki) if hk else None, p(wq), p(wk), p(cs), B, N, H, sb, sn, sb, sn, sb, sn, sb, sn,
                    pos_off, eps, qs, p(dwq), p(dwk))
        dqi, dki = torch.zeros_like(q_in), torch.zeros_like(k_in)
        dwq, dwk = torch.zeros(D, dtype=F32, device=DEV), torch.zeros(D, dtype=F32, device=DEV)
        w1, n1 = ws(QKNORM, B, N)
        call("lcv_det_qknorm_rope_bwd", *args(dqi, dki, dwq if hq else None, dwk if hk else None), p(w1), n1)
        show(f"qknorm det {which}", dqi, dki, dwq, dwk)
        for want in (1, 0):
            dqi, dki = torch.zeros_like(q_in), torch.zeros_like(k_in)
            sq, sk = torch.zeros(8, D, dtype=F32, device=DEV), torch.zeros(8, D, dtype=F32, device=DEV)
            call("lcv_qknorm_rope_bwd", *args(dqi, dki, sq if want and hq else None, sk if want and hk else None), 8)
            show(f"qknorm default {which} dw{want}", dqi, dki)


def smallm(M=17, K=512):
    a = rnd(M, K, dtype=F32)
    for N in (300, 256):
        w, dy = rnd(N, K, scale=0.05), rnd(M, N, dtype=F32)
        for act_in in (0, 1):
            w1, n1 = ws(SMALLM, M, N, K)
            da = torch.zeros(M, K, dtype=F32, device=DEV)
            call("lcv_det_linear_f32_smallm_bwd", p(dy), p(w), p(a), p(da), M, N, K, act_in, p(w1), n1)
            show(f"smallm det N{N} act{act_in}", da)
            if N == 256:   # one slab: the default's atomics add each element once onto zero
                da = torch.zeros(M, K, dtype=F32, device=DEV)
                call("lcv_linear_f32_smallm_bwd", p(dy), p(w), p(a), p(da), M, N, K, act_in)
                show(f"smallm default N{N} act{act_in}", da)


def clip(f32):
    CHUNK, SLOTS = 2048, 64
    sizes = [1, 2047, 2049, 70000]
    flat = rnd(sum((s + 7) // 8 * 8 for s in sizes), scale=0.05, dtype=F32 if f32 else BF16)
    grads, at = [], 0
    for s in sizes:
        grads.append(flat[at: at + s])
        at += (s + 7) // 8 * 8
    if not f32:
        odd = rnd(8 + 2 * CHUNK + 9, scale=0.05)
        grads.append(odd[1: 1 + 2 * CHUNK + 5])      # 2-byte aligned, not 16: the element-wise load path, three chunks
        assert grads[-1].data_ptr() % 16 == 2
    rows, chunk = [], 0
    for g in grads:                                   # every tensor <= 64 chunks: each of the default's slots gets one add
        rows.append([g.data_ptr()] * 4 + [g.numel(), chunk])
        chunk += (g.numel() + CHUNK - 1) // CHUNK
    desc = torch.tensor(rows, dtype=torch.int64).to(DEV)
    for form in ("det", "default"):
        pt = torch.zeros(len(grads), SLOTS, dtype=F32, device=DEV)
        nc = torch.zeros(2, dtype=F32, device=DEV)
        if form == "det":
            w1, n1 = ws(GRAD_NORM, chunk)
            call("lcv_det_grad_norm_clip", p(desc), len(grads), chunk, int(f32), 1.0, p(pt), p(nc), p(w1), n1)
        else:
            call("lcv_grad_norm_clip", p(desc), len(grads), chunk, int(f32), 1.0, p(pt), p(nc))
        show(f"clip {form} {'f32' if f32 else 'bf16'}", nc)


def main():
    if len(sys.argv) > 1:
        lib._LIB_PATH = Path(sys.argv[1]).resolve()
    print(f"# library version {lib.load().lcv_version()}")
    rownorm_and_gate(2, 3, 50, 520)
    rownorm_and_gate(1, 1, 1, 4096)
    qknorm()
    smallm()
    clip(False)
    clip(True)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()

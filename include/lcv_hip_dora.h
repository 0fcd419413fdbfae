/*
 * lcv_hip_dora.h - C ABI of the weight-decomposed LoRA (DoRA, Liu et al. 2024) kernels of liblcv_hip.so (AMD gfx950, MI355X).
 *
 * The adapted weight W' = W + s * B A is split into a direction W' / |W'| (row norms over K) and a trainable magnitude m per
 * output:
 *   y = c (.) (x W^T + s * (x A^T) B^T) + b,    c[n] = m[n] / wn[n],    wn[n] = | W[n, :] + s * B[n, :] A |_2
 * with wn a constant of the backward.  The bracket `pre` is what the LoRA GEMM already produces in one launch (lcv_gemm_nt with
 * the rank-r term as an extra K step, bias NULL); these kernels add the row norm (one pass over the adapted weights per optimizer
 * step) and the column scale, forward and backward.  Fusing the column scale into the GEMM's epilogue is deliberately left out:
 * the separate pass costs one read and one write of the output per adapted linear, forward and backward, and leaves the
 * projection GEMM, lcv_lora_down and lcv_tn_skinny exactly as they are.
 *
 * Conventions are those of lcv_hip_ema.h / lcv_hip_sr.h: every function returns 0 or a negative LCV_E* code, takes device
 * pointers, allocates nothing and takes the hipStream_t as a trailing `void* stream`.  The kernels use no atomics; every output
 * has one writer and is a pure function of the inputs (two calls give the same bits).  Every arithmetic step is one correctly
 * rounded IEEE fp32 operation (a product of two bf16 values is exact in fp32, so where such a product is added the fused and the
 * separate form are the same operation), so a restatement in any IEEE fp32 arithmetic (numpy's, say) gives the same bits; the
 * orders are stated below.  Null pointers (other than the optional ones named), sizes < 1, R outside 1..32, K or N that is no
 * multiple of 8, and pointers of 16-byte packets that are not 16-byte aligned return LCV_EINVAL before any launch.
 */
#ifndef LCV_HIP_DORA_H
#define LCV_HIP_DORA_H

#include <stdint.h>
#include "lcv_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LCV_DORA_NORM_KTILE 512 /* columns of one K tile of lcv_dora_weight_norm: 64 lanes x one 16-byte packet */
#define LCV_DORA_NORM_ROWS 16   /* rows of one workgroup of lcv_dora_weight_norm: 4 waves x 4 rows */
#define LCV_DORA_SLAB 64        /* rows of one slab of lcv_dora_colscale_bwd's sum */
#define LCV_DORA_SLAB_QUARTER 16 /* rows of one quarter of a slab (one wave) */

/* wn_out[n] (fp32 [N]) = | W[n, :] + s * B[n, :] A |_2, with w bf16 [N, K] (row stride K), a bf16 [R, K], b bf16 [N, R],
 * s = (float)scaling.  With b == NULL (a is then ignored and may be NULL, R is not looked at) it is | W[n, :] |_2 through the
 * same code minus the adapter term - what initialises m, so that m == wn to the bit while B = 0.
 *
 * Per element, in fp32:   t = 0;  for r = 0 .. R-1: t = t + B[n, r] * A[r, k];   u = s * t;   v = W[n, k] + u      (b == NULL: v = W[n, k])
 * Per row: column k belongs to lane (k / 8) % 64.  Each lane starts at p = 0 and takes its columns in increasing k:
 * q = v * v; p = p + q.  The 64 lane sums P[0..63] are then folded six times, P[l] = P[l] + P[l ^ o] for
 * o = 32, 16, 8, 4, 2, 1 (all lanes at once), and wn = sqrt(P[0]).  Columns past K add nothing.
 *
 * One workgroup of four waves takes LCV_DORA_NORM_ROWS rows, each wave four of them; A passes through LDS in tiles of
 * LCV_DORA_NORM_KTILE columns (it is up to 32 x 11008 bf16 and does not fit whole), read once per workgroup.  W is streamed
 * exactly once: 2 B per weight element, plus R * K * 2 B of A per workgroup (from L2 after the first).  K % 8 == 0; w and a
 * 16-byte aligned. */
int lcv_dora_weight_norm(const void* w, const void* a, const void* b, double scaling, int64_t N, int64_t K, int64_t R,
                         void* wn_out, void* stream);

/* y[t, n] = bf16_rne(pre[t, n] * c[n] + bias[n]) with c[n] = m[n] / wn[n] (one IEEE division), c[n] = 0 where wn[n] == 0; the
 * product and the sum are rounded separately, and with bias == NULL there is no sum.  pre, y bf16 [M, N] contiguous (y may be
 * pre itself), m, wn fp32 [N], bias bf16 [N] or NULL.  N % 8 == 0; every pointer 16-byte aligned; M <= 64 * 65535.  One read and one write of
 * the output. */
int lcv_dora_colscale_fwd(const void* pre, const void* m, const void* wn, const void* bias, void* y, int64_t M, int64_t N,
                          void* stream);

/* Bytes of `ws` that lcv_dora_colscale_bwd needs: ceil(M / LCV_DORA_SLAB) * N floats (negative LCV_EINVAL for sizes < 1). */
int64_t lcv_dora_colscale_bwd_ws_bytes(int64_t M, int64_t N);

/* dpre[t, n] = bf16_rne(dy[t, n] * c[n])  (c as above),  dm[n] = (sum_t dy[t, n] * pre[t, n]) / wn[n], 0 where wn[n] == 0.
 * The sum: slab j holds rows [j * LCV_DORA_SLAB, (j + 1) * LCV_DORA_SLAB), in four quarters of LCV_DORA_SLAB_QUARTER rows.  A
 * quarter's partial starts at 0 and takes q = q + dy * pre row by row in increasing t (the product is exact, the sum is the only
 * rounding; a quarter without rows stays 0); the slab's partial ((q0 + q1) + q2) + q3 goes to ws[j][n]; then S starts at 0 and
 * takes S = S + ws[j][n] in increasing j; dm = S / wn.  dy and pre are each read once, in the pass that writes dpre (dpre may
 * be dy itself, but not pre).  dy, pre, dpre bf16 [M, N] contiguous, m, wn, dm fp32 [N], N % 8 == 0, every pointer
 * but dm 16-byte aligned, M <= 64 * 65535, ws_bytes >= lcv_dora_colscale_bwd_ws_bytes(M, N). */
int lcv_dora_colscale_bwd(const void* dy, const void* pre, const void* m, const void* wn, void* dpre, void* dm, void* ws,
                          int64_t ws_bytes, int64_t M, int64_t N, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LCV_HIP_DORA_H */

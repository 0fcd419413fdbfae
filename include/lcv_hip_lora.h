/*
 * lcv_hip_lora.h - C ABI of the LoRA dropout kernels of liblcv_hip.so (AMD gfx950, MI355X).
 *
 * The reference's LoRALinear computes lora_up(lora_down(dropout(x))) and trains with the mask live (run_lora_tta.py:249,
 * 259, 485).  A mask cannot ride in the extra-K GEMM step that carries the rank-r term, so the three places that touch the
 * dropped input get kernels of their own here; every GEMM stays as it is.
 *
 * The mask is a pure function of (seed, offset, global element index).  It is never stored and does not depend on launch
 * geometry:
 *   generator  Philox4x32-10, key (seed & 0xffffffff, seed >> 32),
 *              counter (offset & 0xffffffff, offset >> 32, g & 0xffffffff, g >> 32)
 *   g          ((row0 + m) * K + k) >> 3 with K the logical width (not the row stride); K % 8 == 0, so the 8 elements of
 *              a group share a row.  All index arithmetic is 64-bit.
 *   element    e = k & 7 takes a 16-bit half of output word c[e >> 1]: the low half for even e, the high half for odd e
 *   keep       iff half >= T, T = round-half-even(p * 65536) clamped to 1..65535
 *   scale      kept elements are multiplied by 65536 / (65536 - T), computed in fp32.  This makes the expectation exact
 *              for the keep rate the 16-bit threshold really has; it differs from 1 / (1 - p) by at most
 *              2^-17 / (1 - p) relative: below 1e-5 up to p = 0.23, 1.6e-5 at p = 0.5.
 *   rounding   where the dropped input is an operand (down-projection, dA) the product x * scale is rounded to bf16
 *              first: the rounding point nn.Dropout leaves on a bf16 tensor.
 * `row0` is the global index of the first row the call sees: a caller that holds rows [a, b) of a larger matrix passes
 * row0 = a and gets that slice of the full mask.  No bit parity with ATen's dropout mask is claimed (that mask depends
 * on ATen's launch geometry).
 *
 * Conventions are those of the main header (status codes and the error string come from there): every function returns 0
 * or a negative LCV_E* code, takes device pointers, allocates nothing and takes the hipStream_t as a trailing
 * `void* stream`.  p outside the open interval (0, 1) is LCV_EINVAL: p = 0 belongs to lcv_lora_down / lcv_tn_skinny and
 * the extra-K step of lcv_gemm_nt.  row0 >= 0.  The kernels use no atomics; every output is a pure function of the inputs.
 */
#ifndef LCV_HIP_LORA_H
#define LCV_HIP_LORA_H

#include <stdint.h>
#include "lcv_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* h[M, Rpad] = bf16(s * bf16(xd A^T)), xd = bf16(x * mask * scale); columns R..Rpad-1 are written as zeros.
 * Shape rules of lcv_lora_down: 1 <= R <= 32, R <= Rpad <= 64, K % 8 == 0, ldx % 8 == 0 (ldx: row stride of x). */
int lcv_lora_down_dropout(const void* x, const void* A, void* h, int64_t M, int64_t K, int64_t R, int64_t Rpad,
                          int64_t ldx, float s, double p, uint64_t seed, uint64_t offset, int64_t row0, void* stream);

/* out[R, K] fp32 = scale * g[:, :R]^T xd  (g: [M, Rpad] bf16, x: [M, K] bf16 with row stride ldx).  This is dA: the mask
 * sits on x at x's own (m, k).  Row groups leave partial sums in `ws` (16-byte aligned, at least
 * lcv_tn_skinny_dropout_ws_bytes(M, K, R) bytes, content undefined afterwards) and a second launch adds them in group
 * order: `out` is overwritten and carries the same bits on every call.  A missing, misaligned or too small workspace is
 * LCV_EINVAL.  K % 8 == 0, ldx % 8 == 0, 1 <= R <= Rpad. */
int lcv_tn_skinny_dropout(const void* g, const void* x, float* out, int64_t M, int64_t K, int64_t R, int64_t Rpad,
                          int64_t ldx, float scale, double p, uint64_t seed, uint64_t offset, int64_t row0, float* ws,
                          int64_t ws_bytes, void* stream);
int64_t lcv_tn_skinny_dropout_ws_bytes(int64_t M, int64_t K, int64_t R);

/* dx[m, k] = bf16(float(dx[m, k]) + mask * scale * sum_r g[m, r] * A[r, k]), in place, one rounding  (dx: [M, K] bf16
 * contiguous, g: [M, Rpad] bf16 with row stride ldg, A: [R, K] bf16).  Replaces the extra-K LoRA term of the dx GEMM when
 * dropout is on.  1 <= R <= 32, R <= Rpad <= ldg, K % 8 == 0, Rpad % 8 == 0, ldg % 8 == 0. */
int lcv_lora_dx_dropout_add(void* dx, const void* g, const void* A, int64_t M, int64_t K, int64_t R, int64_t Rpad,
                            int64_t ldg, double p, uint64_t seed, uint64_t offset, int64_t row0, void* stream);

/* out_u8[M, K] = the 0 / 1 mask as bytes: the bridge between the kernels and a host restatement.  K % 8 == 0,
 * out_u8 8-byte aligned. */
int lcv_lora_dropout_mask(void* out_u8, int64_t M, int64_t K, double p, uint64_t seed, uint64_t offset, int64_t row0,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LCV_HIP_LORA_H */

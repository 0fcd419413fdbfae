/*
 * lcv_hip_stepcache.h - C ABI of the first-block step cache of the denoise loop of liblcv_hip.so (AMD gfx950, MI355X).
 *
 * A 50-step denoise runs the whole block stack 50 times, and on many steps the stack produces nearly what it produced a step
 * ago.  A first-block cache runs block 0 (1/L of the stack), compares block 0's residual with the residual of the last fully
 * computed step, and if the two are close adds the cached residual of blocks 1...L-1 instead of running them.  These three
 * entry points are the residual, the comparison with its decision, and the two ends of the cached residual.
 *
 * x0 is the block stack's input (the patch embedder's output), x1 the output of block 0, xL the output of the last block:
 * [rows, n] bf16, contiguous, rows = the forward's batch (2 under classifier-free guidance), n = tokens * hidden.
 *
 * Every operation is one correctly rounded IEEE fp32 operation (there is no product that could fuse with a sum), and every
 * bf16 conversion is round-to-nearest-even, so (a.float() -/+ b.float()).bfloat16() in torch or numpy gives the same bits.
 *
 * Conventions are those of lcv_hip.h: every function returns 0 or a negative LCV_E* code, takes device pointers, allocates
 * nothing and takes the hipStream_t as a trailing `void* stream`.  All pointers are 16-byte aligned and every count is a
 * multiple of 8 (16-byte packets only; the hidden size is 4096, so every real row qualifies); anything else returns LCV_EINVAL
 * without a launch.  The kernels use no atomics; every output has one writer and is a pure function of the inputs.
 */
#ifndef LCV_HIP_STEPCACHE_H
#define LCV_HIP_STEPCACHE_H

#include <stdint.h>
#include "lcv_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* r_out = bf16(float(x1) - float(x0)), and against prev (the r of the last COMPUTED step), per row b:
 *   num[b] = sum_j |float(r[b,j]) - float(prev[b,j])|      per element d = r - p;  a = |d|;  acc = acc + a
 *   den[b] = sum_j |float(prev[b,j])|                      per element a = |p|;  acc = acc + a
 *   out[0..rows) = num, out[rows..2 rows) = den (fp32), and the 32-bit integer out[2 rows] = 1 if for every row
 *   num[b] < thr * den[b] (thr fp32, one rounded product, a strict compare, no division), else 0.
 * den = 0 or a NaN anywhere gives 0, thr = 0 gives 0, thr = +inf gives 1 whenever every den > 0 (and every num is finite).
 * Fixed order: a thread adds its 8 elements in index order, a wave joins by butterfly, the four waves of a 2048-element chunk
 * join in wave order into one partial pair per chunk (`partials`, the caller's workspace of at least
 * rows * ceil(n / 2048) * 8 bytes: all num partials, then all den partials; no chunk spans two rows); a second launch of one workgroup adds each row's partials - thread t takes t, t + 1024, ... in index order,
 * then butterfly, then the waves in wave order.  Same inputs give the same bits.
 * prev == NULL: only r_out and a zero decision are written (out[0 .. 2 rows) is left alone; partials may be NULL).
 * 1 <= rows <= 8, n >= 8, n % 8 == 0, thr >= 0 and not NaN.  r_out may be neither x0, x1 nor prev.
 * 6 B read + 2 B written per element (4 + 2 without prev). */
int lcv_stepcache_diff(const void* x0, const void* x1, const void* prev, void* r_out, int64_t rows, int64_t n, float thr,
                       float* partials, int64_t partials_bytes, float* out, void* stream);

/* R = bf16(float(xL) - float(x1)): what blocks 1...L-1 added, kept for the steps that skip them.  total >= 8, total % 8 == 0.
 * 4 B read + 2 B written per element. */
int lcv_stepcache_store(const void* xL, const void* x1, void* R, int64_t total, void* stream);

/* out = bf16(float(x1) + float(R)): a skipped step's stand-in for xL.  `out` may be x1.  total >= 8, total % 8 == 0.
 * 4 B read + 2 B written per element. */
int lcv_stepcache_apply(const void* x1, const void* R, void* out, int64_t total, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LCV_HIP_STEPCACHE_H */

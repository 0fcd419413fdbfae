/*
 * lcv_hip_ema.h - C ABI of the fp32 weight average over the optimizer steps of liblcv_hip.so (AMD gfx950, MI355X).
 *
 * One bf16 gradient - one draw of sigma, epsilon, variant and video - stands behind every update of a 10-20 step adaptation.
 * Averaging the iterates removes part of that noise for one streaming pass over the parameters per step: e, an fp32 tensor per
 * parameter, follows the masters w = join(h, l) (lcv_hip_master.h) as e = beta * e + (1 - beta) * w.  An increment
 * (1 - beta) * (w - e) is far below half a bf16 ulp of w, so the average exists for master weights only.  Because
 * join(split(m)) = m for every fp32 pattern, the average can be swapped into the parameters (where every GEMM reads its bf16
 * word) and back out without losing a bit: scoring and generating with the average need no second model.
 *
 * `ema` is a device array of n_tensors pointers to the fp32 averages, parallel to the descriptor table (as `low` is).  Of the
 * table `param`, numel and first_chunk are read; grad and the moment pointers are not.
 *
 * Every operation is one correctly rounded IEEE fp32 operation (no product fuses with the difference that takes it), so a
 * restatement in any IEEE fp32 arithmetic (numpy's, say) gives the same bits.
 *
 * Conventions are those of lcv_hip_master.h: every function returns 0 or a negative LCV_E* code, takes device pointers,
 * allocates nothing and takes the hipStream_t as a trailing `void* stream`.  The kernels use no atomics and no LDS; every output
 * has one writer and is a pure function of the inputs.
 */
#ifndef LCV_HIP_EMA_H
#define LCV_HIP_EMA_H

#include <stdint.h>
#include "lcv_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* e = join(h, l): the average starts at (or is reset to) the masters.  4 B read + 4 B written per parameter. */
int lcv_master_ema_load(const lcv_adam_tensor* tensors, void* const* low, void* const* ema, int64_t n_tensors,
                        int64_t total_chunks, void* stream);

/* One step of the average, launched after whichever step kernel ran.  Per element, with b = (float)beta:
 *   w = join(h, l);  d = w - e;  t = b * d;  e = w - t.
 * h and l are not written.  This form of beta * e + (1 - beta) * w is exact in its two degenerate cases: b = 0 gives e = w
 * (wherever w - e is finite), and w = e gives e back (up to the sign of a zero: a master of -0 may come back as +0, as in
 * lcv_hip_anchor.h).  beta outside [0, 1) or NaN returns LCV_EINVAL without a launch.  8 B read + 4 B written per parameter. */
int lcv_master_ema_update(const lcv_adam_tensor* tensors, void* const* low, void* const* ema, int64_t n_tensors,
                          int64_t total_chunks, double beta, void* stream);

/* Exchange the masters and the average.  Per element:
 *   w = join(h, l);  (h, l) = split(e);  e = w.
 * Afterwards the parameters are in valid master format - h is the round-to-nearest, ties-away bf16 of the average - and a
 * second call restores every bit of all three arrays.  8 B read + 8 B written per parameter. */
int lcv_master_ema_swap(const lcv_adam_tensor* tensors, void* const* low, void* const* ema, int64_t n_tensors,
                        int64_t total_chunks, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LCV_HIP_EMA_H */

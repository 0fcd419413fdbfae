/*
 * lcv_hip_master.h - C ABI of the fp32-master-weight optimizer kernels of liblcv_hip.so (AMD gfx950, MI355X).
 *
 * lcv_sgd_step and the bf16 branch of lcv_adamw_step reproduce torch's foreach rounding points: the parameter is rounded to
 * bf16 after every step, so an update below half a bf16 ulp of the weight is discarded and the next step starts from the same
 * bits.  At the reference's full-model operating point (lr = 1e-5, gradient norm clipped to 1 over 13.6 B elements) that is
 * every update.  The kernels here let each bf16 parameter element carry the 16 mantissa bits it is missing, in a second
 * tensor, so that small updates accumulate.  The bf16 words - what every GEMM reads - stay where and what they are.
 *
 * The format.  A bf16 parameter element has bits `h` (uint16).  Its companion `l` (int16, two's complement) lives in a separate
 * tensor of the same shape (the "low words").  Together they represent the fp32 number (the "master") with bit pattern
 *   join    m = ((uint32)h << 16) + (int32)l            (mod 2^32)
 *   split   h = (m + 0x8000) >> 16  (in uint32),  l = (int16)(m - (h << 16)),  so l is in [-32768, 32767]
 * Properties:
 *   - join(split(m)) == m for every 32-bit pattern, NaNs and infinities included (pure integer arithmetic).
 *   - l == 0 means "the master equals the bf16 value": a zero-filled low-word tensor attaches to an existing model without
 *     changing it, and zeroing the low words re-synchronises the master with whatever the bf16 words now hold.
 *   - h is the round-to-nearest bf16 of the master with TIES AWAY FROM ZERO.  It differs from torch's `.to(bfloat16)`
 *     (ties to even) only on exact ties (low 16 bits of m == 0x8000 with an even upper half), about 1 element in 65 536 of
 *     random data.  Ties-to-even would need l = +32768 there, which does not fit an int16.
 *   - Beyond the identity above nothing about non-finite masters is specified (a master next to the largest finite value
 *     may carry an h that reads as infinity).
 *
 * The steps work in fp32, round nothing to bf16 in between, and every operation in them (add, multiply, divide, square root)
 * is one correctly rounded IEEE operation: no product fuses with the sum that takes it, and the square root is not the 1-ulp
 * native one.  A restatement in any IEEE fp32 arithmetic (numpy's, say) therefore gives the same bits.  The
 * gradients are still bf16 (2^-9 relative precision per element): only their accumulation into the weights becomes exact.
 * Gradient clipping is the unchanged lcv_grad_norm_clip / lcv_det_grad_norm_clip with param_f32 = 0 over the same
 * descriptor table (they read grad, numel and first_chunk only).
 *
 * Conventions are those of the main header (status codes and the error string come from there): every function returns 0
 * or a negative LCV_E* code, takes device pointers, allocates nothing and takes the hipStream_t as a trailing
 * `void* stream`.  The kernels use no atomics; every output is a pure function of the inputs.
 */
#ifndef LCV_HIP_MASTER_H
#define LCV_HIP_MASTER_H

#include <stdint.h>
#include "lcv_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* SGD (momentum 0) on the masters of bf16 parameters.  `tensors`: the descriptor table of lcv_sgd_step (param and grad
 * bf16, moment pointers unused); `low`: device array of n_tensors pointers to the int16 low words, parallel to the table.
 * Per element:  w = join(h, l);  g = float(grad) * coef;  if (wd != 0) g = g + wd * w;  w = w + (-lr) * g;
 * (h, l) = split(w).  coef is norm_coef[1], or 1 when norm_coef is NULL.  6 B read + 4 B written per parameter. */
int lcv_master_sgd_step(const lcv_adam_tensor* tensors, void* const* low, int64_t n_tensors, int64_t total_chunks,
                        const float* norm_coef, double lr, double weight_decay, void* stream);

/* AdamW on the masters of bf16 parameters.  As above, and exp_avg / exp_avg_sq of the table point to FP32 moments.  The
 * scalars are formed in double as lcv_adamw_step forms them; per element the op sequence is that of lcv_adamw_step's fp32
 * form with p = join(h, l) on entry, (h, l) = split(p) on exit and g = float(grad) * coef:
 *   p = p * (1 - lr*wd);  m = m + (1-b1) * (g - m);  v = v * b2;  v = v + ((1-b2) * g) * g;
 *   d = sqrt(v) / sqrt(1-b2^t) + eps;  p = p + (-lr/(1-b1^t)) * (m / d)
 * 14 B read + 12 B written per parameter.  step >= 1. */
int lcv_master_adamw_step(const lcv_adam_tensor* tensors, void* const* low, int64_t n_tensors, int64_t total_chunks,
                          const float* norm_coef, double lr, double beta1, double beta2, double eps, double weight_decay,
                          int64_t step, void* stream);

/* (hi_bf16[i], low[i]) = split(master[i]) and master[i] = join(hi_bf16[i], low[i]), i < n: the bridge between the kernels
 * and a host restatement, and how a caller reads the masters back.  n >= 1. */
int lcv_master_split(const float* master, void* hi_bf16, void* low, int64_t n, void* stream);
int lcv_master_join(const void* hi_bf16, const void* low, float* master, int64_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LCV_HIP_MASTER_H */

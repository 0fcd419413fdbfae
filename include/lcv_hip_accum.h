/*
 * lcv_hip_accum.h - C ABI of fp32 gradient accumulation over micro-steps of liblcv_hip.so (AMD gfx950, MI355X).
 *
 * The master-weight steps (lcv_hip_master.h) make the accumulation of updates into the weights exact, but each update still
 * comes from one bf16 gradient: one draw of (sigma, eps, variant, video).  Calling backward() several times before a step
 * does not help at that precision: autograd adds into a bf16 `.grad`, so a micro-gradient below half a bf16 ulp of the running
 * sum vanishes, exactly as small updates vanished from bf16 weights.  The entry points here give every parameter element an
 * fp32 accumulator: each micro-step's bf16 gradient is scaled and added into it in fp32, and the master-weight steps read the
 * accumulator as the gradient.
 *
 * Every operation is one correctly rounded IEEE fp32 operation (no product fuses with the sum that takes it), so a restatement
 * in any IEEE fp32 arithmetic (numpy's, say) gives the same bits.  The two steps are lcv_master_sgd_step and
 * lcv_master_adamw_step with one difference: the table's `grad` points to fp32, so g = grad * coef without a widening.  Fed an
 * fp32 gradient that equals float(bf16 gradient) they give the bits of those steps.
 *
 * Gradient clipping is the unchanged lcv_grad_norm_clip / lcv_det_grad_norm_clip with param_f32 = 1 over a descriptor table
 * whose `grad` pointers are the accumulators (they read grad, numel and first_chunk only): an fp32 gradient's norm is an fp32
 * number.
 *
 * Conventions are those of lcv_hip_master.h: every function returns 0 or a negative LCV_E* code, takes device pointers,
 * allocates nothing and takes the hipStream_t as a trailing `void* stream`.  The kernels use no atomics and no LDS; every
 * output is a pure function of the inputs.
 */
#ifndef LCV_HIP_ACCUM_H
#define LCV_HIP_ACCUM_H

#include <stdint.h>
#include "lcv_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* acc += float(grad) * scale over a descriptor table.  `tensors`: the descriptor table of lcv_sgd_step (grad bf16; param and
 * the moment pointers unused); `acc`: device array of n_tensors pointers to the fp32 accumulators, parallel to the table.
 * Per element, with s = (float)scale:  t = float(g) * s;  a = a + t  - two operations, and always the add (there is no
 * "first micro-step" form: 0 + t keeps the sign of zero that IEEE addition gives).  6 B read + 4 B written per element. */
int lcv_grad_accumulate(const lcv_adam_tensor* tensors, void* const* acc, int64_t n_tensors, int64_t total_chunks,
                        double scale, void* stream);

/* lcv_master_sgd_step with an FP32 gradient: `grad` of the table points to fp32 (an accumulator).  Per element:
 * w = join(h, l);  g = grad * coef;  if (wd != 0) g = g + wd * w;  w = w + (-lr) * g;  (h, l) = split(w).
 * 8 B read + 4 B written per parameter. */
int lcv_master_sgd_step_g32(const lcv_adam_tensor* tensors, void* const* low, int64_t n_tensors, int64_t total_chunks,
                            const float* norm_coef, double lr, double weight_decay, void* stream);

/* lcv_master_adamw_step with an FP32 gradient: `grad` of the table points to fp32, exp_avg / exp_avg_sq to FP32 moments (there
 * is no 8-bit-moment form).  Scalars and op sequence are those of lcv_master_adamw_step with g = grad * coef.
 * 16 B read + 12 B written per parameter.  step >= 1. */
int lcv_master_adamw_step_g32(const lcv_adam_tensor* tensors, void* const* low, int64_t n_tensors, int64_t total_chunks,
                              const float* norm_coef, double lr, double beta1, double beta2, double eps, double weight_decay,
                              int64_t step, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LCV_HIP_ACCUM_H */

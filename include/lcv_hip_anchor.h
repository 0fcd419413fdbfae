/*
 * lcv_hip_anchor.h - C ABI of decay toward the base weights and of the drift norm of liblcv_hip.so (AMD gfx950, MI355X).
 *
 * Weight decay pulls every parameter toward zero.  For an adapter that is the pull toward the base model (the adapter product
 * is zero there); for a full model or its norm weights it erodes pretrained values and does not bring an adapted model back
 * to where it started.  The steps here are the master-weight steps (lcv_hip_master.h, lcv_hip_accum.h, lcv_hip_moments8.h)
 * with the decay taken on w - w0 (L2-SP), where w0 is the element's base weight, and lcv_master_drift_sumsq measures
 * |theta - theta0|.  A pull of lr * wd * (w - w0) is far below half a bf16 ulp of w per step, so the steps exist for master
 * weights only.
 *
 * `anchor` is a device array of n_tensors pointers to the bf16 base words h0, parallel to the descriptor table (as `low` is).
 * The base master of an element is w0 = float(h0) = join(h0, 0).  The base words are read, never written.
 *
 * Every operation is one correctly rounded IEEE fp32 operation (no product fuses with the sum that takes it), so a restatement
 * in any IEEE fp32 arithmetic (numpy's, say) gives the same bits.  With all-zero base words the SGD step gives the bits of
 * lcv_master_sgd_step / _g32; at weight_decay = 0 the AdamW steps give those of lcv_master_adamw_step / _g32 /
 * lcv_master_adamw8_step (up to the sign of a zero master).
 *
 * Conventions are those of lcv_hip_master.h: every function returns 0 or a negative LCV_E* code, takes device pointers,
 * allocates nothing and takes the hipStream_t as a trailing `void* stream`.  The kernels use no atomics; every output is a
 * pure function of the inputs.  Each step reads 2 B per parameter of base words more than its counterpart.
 */
#ifndef LCV_HIP_ANCHOR_H
#define LCV_HIP_ANCHOR_H

#include <stdint.h>
#include "lcv_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* lcv_master_sgd_step / lcv_master_sgd_step_g32 decaying toward w0.  grad_f32 = 0: `grad` of the table is bf16, widened;
 * grad_f32 = 1: it is fp32 (an accumulator of lcv_grad_accumulate).  Per element:
 *   w = join(h, l);  g = grad * coef;  if (wd != 0) { d = w - w0;  t = wd * d;  g = g + t; }  u = (-lr) * g;  w = w + u;
 *   (h, l) = split(w).
 * 8 B read + 4 B written per parameter (10 + 4 at grad_f32 = 1). */
int lcv_master_sgd_step_anchor(const lcv_adam_tensor* tensors, void* const* low, void* const* anchor, int64_t n_tensors,
                               int64_t total_chunks, const float* norm_coef, double lr, double weight_decay, int grad_f32,
                               void* stream);

/* lcv_master_adamw_step / lcv_master_adamw_step_g32 (FP32 moments) decaying toward w0: their op sequence with
 *   d = p - w0;  t = a * d;  p = p - t          a = (float)(lr * weight_decay), the product formed in double
 * in place of p = p * (float)(1 - lr * weight_decay), always taken (a = 0 subtracts a zero).  All other scalars are those of
 * lcv_master_adamw_step.  16 B read + 12 B written per parameter (18 + 12 at grad_f32 = 1).  step >= 1. */
int lcv_master_adamw_step_anchor(const lcv_adam_tensor* tensors, void* const* low, void* const* anchor, int64_t n_tensors,
                                 int64_t total_chunks, const float* norm_coef, double lr, double beta1, double beta2, double eps,
                                 double weight_decay, int64_t step, int grad_f32, void* stream);

/* lcv_master_adamw8_step (8-bit block-scaled moments, bf16 gradients) with the same substitution inside its
 * decode -> step -> split -> encode body.  `scales` as there.  10 B read + 6 B written per parameter.  step >= 1. */
int lcv_master_adamw8_step_anchor(const lcv_adam_tensor* tensors, void* const* low, void* const* scales, void* const* anchor,
                                  int64_t n_tensors, int64_t total_chunks, const float* norm_coef, double lr, double beta1,
                                  double beta2, double eps, double weight_decay, int64_t step, void* stream);

/* out[0] = sum over all elements of all tensors of (join(h, l) - float(h0))^2, out[1] = sqrt(out[0]).  The table's `param`,
 * numel and first_chunk are read; grad and the moment pointers are not.  low == NULL means "all low words zero": the drift of
 * a run without master weights.  Per element d = w - w0;  q = d * d;  acc = acc + q.  Fixed order: a thread adds its 8
 * elements in index order, a wave joins by butterfly, a chunk's four waves join in wave order into one fp32 partial per chunk
 * (`partials`, the caller's workspace of at least total_chunks * 4 bytes; no chunk spans two tensors); a second launch of one
 * workgroup adds the partials - thread t takes t, t + 1024, ... in index order, then butterfly, then the waves in wave order.
 * Same inputs give the same bits.  6 B read per parameter (4 B with low == NULL), nothing written but the partials. */
int lcv_master_drift_sumsq(const lcv_adam_tensor* tensors, void* const* low, void* const* anchor, int64_t n_tensors,
                           int64_t total_chunks, float* partials, int64_t partials_bytes, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LCV_HIP_ANCHOR_H */

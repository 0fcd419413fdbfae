/*
 * lcv_hip_sr.h - C ABI of the stochastic-rounding optimizer kernels of liblcv_hip.so (AMD gfx950, MI355X).
 *
 * lcv_sgd_step and the bf16 branch of lcv_adamw_step round every stored value to the nearest bf16.  Two things follow.  An
 * update below half a bf16 ulp of the weight is discarded (lcv_hip_master.h says where that is every update).  And AdamW's
 * second moment never decays: v = bf16(v * b2) with b2 = 0.999 changes v by 2^-10 relative, half a bf16 ulp is between 2^-9
 * and 2^-8 relative, so the product rounds back to v for every normal bf16 v and exp_avg_sq only ever moves when
 * (1-b2)*g*g alone clears half an ulp of it.  The kernels here keep the storage of those steps - bf16 parameters, bf16
 * moments, nothing beside them - compute the step in fp32 as the master-weight kernels do, and round what they store up or
 * down at random, so that the stored bf16 value is an unbiased estimate of the fp32 result: small updates and the decay of v
 * survive in expectation.
 *
 * The rounding.  An fp32 result has bit pattern `u` (uint32); `r` is a 16-bit random value (0 .. 65535).
 *   exponent field of u not all ones:   h = (u + r) >> 16          (in uint32; the sum cannot wrap)
 *   exponent field all ones (inf, NaN): h = the round-to-nearest-even bf16 of u, as everywhere else in the library: u >> 16,
 *                                       with the quiet bit 0x0040 set when u is a NaN
 * fp32 is sign-magnitude, so adding to the pattern moves AWAY FROM ZERO: h is the bf16 toward zero (u >> 16) or its
 * neighbour away from zero, the latter for exactly (u & 0xffff) of the 65 536 values of r - probability
 * (u & 0xffff) / 65536, the fraction of the way u lies toward that neighbour.  A result that is a bf16 value (low half 0) is
 * stored as it is for every r; +-0 stay +-0.  A finite result within one bf16 ulp of the largest finite bf16 (upper half
 * 0x7f7f, low half not 0) may be stored as infinity, with that same probability.
 *
 * The random bits.  Philox4x32-10 (csrc/philox.h), one call per eight elements and stream:
 *   philox4x32_10(key = (lo, hi of seed), counter = (lo, hi of offset + k, lo, hi of G))
 * k is the stream: 0 for the parameter, 1 for exp_avg, 2 for exp_avg_sq (offset + k in uint64).  G is the group: over a
 * descriptor table, G = (first_chunk + i / 2048) * 256 + (i % 2048) / 8 for element i of a tensor - the workgroup and thread
 * that own the element, unique over the table, so no two tensors share bits; over a single array (lcv_sr_round) G = i >> 3.
 * Element e = i % 8 of the group takes the low half of output word e >> 1 when e is even and the high half when it is odd
 * (the layout of the LoRA dropout mask, lcv_hip_lora.h).  A caller that advances `offset` by 4 per step never reuses a
 * counter.
 *
 * The steps work in fp32 on float(bf16 word), round nothing to bf16 in between, and every operation in them is one correctly
 * rounded IEEE operation, as in lcv_hip_master.h: a restatement in numpy gives the same bits.  Gradient clipping is the
 * unchanged lcv_grad_norm_clip / lcv_det_grad_norm_clip with param_f32 = 0 over the same descriptor table.
 *
 * Conventions are those of the main header (status codes and the error string come from there): every function returns 0
 * or a negative LCV_E* code, takes device pointers, allocates nothing and takes the hipStream_t as a trailing
 * `void* stream`.  The kernels use no atomics; every output is a pure function of (inputs, seed, offset).
 */
#ifndef LCV_HIP_SR_H
#define LCV_HIP_SR_H

#include <stdint.h>
#include "lcv_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* SGD (momentum 0) on bf16 parameters with a stochastically rounded store.  `tensors`: the descriptor table of lcv_sgd_step
 * (param and grad bf16, moment pointers unused).  Per element - lcv_master_sgd_step's sequence with the low word absent:
 *   w = float(p);  g = float(grad) * coef;  if (wd != 0) g = g + wd * w;  w = w + (-lr) * g;  p = SR(w, stream 0)
 * coef is norm_coef[1], or 1 when norm_coef is NULL.  4 B read + 2 B written per parameter. */
int lcv_sr_sgd_step(const lcv_adam_tensor* tensors, int64_t n_tensors, int64_t total_chunks, const float* norm_coef, double lr,
                    double weight_decay, uint64_t seed, uint64_t offset, void* stream);

/* AdamW on bf16 parameters and bf16 moments with stochastically rounded stores.  The scalars are formed in double as
 * lcv_adamw_step forms them; per element the fp32 op sequence of lcv_master_adamw_step runs on float(p), float(exp_avg),
 * float(exp_avg_sq) and g = float(grad) * coef, then p = SR(p, stream 0), exp_avg = SR(m, stream 1),
 * exp_avg_sq = SR(v, stream 2).  8 B read + 6 B written per parameter.  step >= 1. */
int lcv_sr_adamw_step(const lcv_adam_tensor* tensors, int64_t n_tensors, int64_t total_chunks, const float* norm_coef, double lr,
                      double beta1, double beta2, double eps, double weight_decay, int64_t step, uint64_t seed, uint64_t offset,
                      void* stream);

/* out_bf16[i] = SR(x[i], stream 0) with G = i >> 3, i < n: the bridge between the kernels and a host restatement.  n >= 1. */
int lcv_sr_round(const float* x, void* out_bf16, int64_t n, uint64_t seed, uint64_t offset, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LCV_HIP_SR_H */

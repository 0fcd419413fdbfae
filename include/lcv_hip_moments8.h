/*
 * lcv_hip_moments8.h - C ABI of the 8-bit block-scaled AdamW moments of liblcv_hip.so (AMD gfx950, MI355X).
 *
 * lcv_master_adamw_step (lcv_hip_master.h) keeps fp32 moments: 8 B per parameter, the one large item of the master-weight
 * AdamW state that is not forced.  The step here keeps each moment in ONE byte per parameter plus one fp32 scale per moment
 * per 512 parameters: about 2.016 B per parameter, and 14 B streamed per parameter per step (8 read, 6 written) instead of 26.
 *
 * The format.  A BLOCK is 512 consecutive elements of one tensor, starting at a multiple of 512; the last block of a tensor
 * may be short, blocks never span tensors.  A block stores two fp32 scales, sm and sr, and per element one byte cm (first
 * moment m) and one byte cr (second moment v, stored as its root r = sqrt(v)).
 *
 *   encode  r  = sqrt(v)                                   (correctly rounded)
 *           sm = max |m|,  sr = max r                      over the block's valid elements
 *           x  = |m| / sm,  y = r / sr                     (one correctly rounded division each; 0 when the scale is 0)
 *           k(z) = (bits(z) + 0x80000) >> 20               in uint32: 3 mantissa bits, ties away from zero, carry into the exponent
 *           cr = 0 if y == 0, else clamp(k(y) - 761, 1, 255)        code 255 is 1.0, code 1 is 1.25 * 2^-32; a positive ratio
 *                                                                   is clamped UP to code 1, never flushed
 *           mag = 0 if x == 0 or k(x) < 890, else min(k(x) - 889, 127)   code 127 is 1.0, code 1 is 1.25 * 2^-16; smaller
 *                                                                        first moments flush to +0
 *           cm = mag | (sign(m) << 7), the sign bit cleared when mag == 0
 *   decode  y = bitcast<float>((cr + 761) << 20) for cr >= 1, else 0;   r = y * sr;   v = r * r
 *           x = bitcast<float>(((cm & 127) + 889) << 20) for a nonzero magnitude, else 0;   m = +-(x * sm)
 *
 * Every operation is integer arithmetic or one correctly rounded fp32 operation, so a restatement in any IEEE fp32 arithmetic
 * gives the same bits.  Zeroed codes and scales are the state "all moments zero".  encode(decode(c)) == c.  Nothing is
 * specified for non-finite moments.
 *
 * Limits.  A decoded moment that was neither clamped nor flushed is within 2^-4 relative of the encoded one.  First moments
 * below 2^-16 of their block's largest restart from (1-b1)*g every step; second-moment roots more than 2^-32 below their
 * block's largest are held at that floor; both make updates smaller, never larger.  A moment that should decay by less than
 * half a code step per step does not decay.
 *
 * Conventions are those of lcv_hip_master.h: every function returns 0 or a negative LCV_E* code, takes device pointers,
 * allocates nothing and takes the hipStream_t as a trailing `void* stream`.  The kernels use no atomics and no LDS; every
 * output is a pure function of the inputs.
 */
#ifndef LCV_HIP_MOMENTS8_H
#define LCV_HIP_MOMENTS8_H

#include <stdint.h>
#include "lcv_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LCV_MOMENTS8_BLOCK 512

/* AdamW on the masters of bf16 parameters with 8-bit moments.  `tensors` and `low` as for the fp32-moment step, but exp_avg /
 * exp_avg_sq of the table point to the UINT8 code tensors (cm, cr); `scales`: device array of n_tensors pointers, parallel
 * to the table, each to fp32 [2][ceil(numel/512)]: the sm row, then the sr row.  Per element: decode (m0, v0); the op sequence
 * of the fp32-moment step on (join(h, l), m0, v0, float(grad) * coef); (h, l) = split(p); encode the new (m, v).  The parameter
 * update uses the fp32 new moments BEFORE they are quantised, so from zeroed state the first step gives the (h, l) bits of the
 * fp32-moment step, and from any state one step gives the (h, l) bits of that step fed the decoded moments.  The scalars
 * are formed in double exactly as there.  8 B read + 6 B written per parameter.  step >= 1. */
int lcv_master_adamw8_step(const lcv_adam_tensor* tensors, void* const* low, void* const* scales, int64_t n_tensors,
                           int64_t total_chunks, const float* norm_coef, double lr, double beta1, double beta2, double eps,
                           double weight_decay, int64_t step, void* stream);

/* One tensor of n >= 1 elements: fp32 moments -> codes and scales, and back.  `scales` is fp32 [2][ceil(n/512)].  The bridge
 * between the kernels and a host restatement, and how a caller reads the state; the device functions are the step's. */
int lcv_moments8_encode(const float* m_f32, const float* v_f32, void* cm, void* cr, float* scales, int64_t n, void* stream);
int lcv_moments8_decode(const void* cm, const void* cr, const float* scales, float* m_f32, float* v_f32, int64_t n,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LCV_HIP_MOMENTS8_H */

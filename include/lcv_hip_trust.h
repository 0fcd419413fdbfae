/*
 * lcv_hip_trust.h - C ABI of the trust-region cap on the adapted weights' drift of liblcv_hip.so (AMD gfx950, MI355X).
 *
 * Projected gradient descent onto a ball around the base weights: after an optimizer step, if |theta - theta0| exceeds the
 * radius, the drift theta - theta0 is scaled back onto the ball.  lcv_trust_sumsq measures the drift in a fixed order (per
 * tensor and in total), lcv_trust_project reads that measurement from device memory and rewrites the parameters whose ball
 * is exceeded; a tensor or run inside its ball has no byte written.  The host never waits for either.
 *
 * Parameters come in two forms, chosen by `param_f32`:
 *   param_f32 = 0   bf16 words `param` of the descriptor table with int16 low words `low` beside them (lcv_hip_master.h):
 *                   w = join(h, l), (h, l) = split(w) on the way out; the base is a bf16 word, w0 = float(h0).
 *   param_f32 = 1   fp32 values: `param` and the anchors are fp32, w and w0 are the stored values; `low` must be NULL.
 * `low` and `anchor` are device arrays of n_tensors pointers parallel to the descriptor table, as in lcv_hip_anchor.h.  A NULL
 * `anchor` means "every base value is zero" (the delta / FiLM vectors start at zero); in lcv_trust_sumsq a NULL `low` means
 * "every low word is zero".  The table covers whatever the caller lists - the optimizers list ALL non-empty parameters, with or
 * without a gradient; its `param`, numel and first_chunk are read, grad and the moment pointers are not.
 *
 * Every operation is one correctly rounded IEEE fp32 operation (no product fuses with the sum that takes it; the divide and the
 * square root are the correctly rounded ones), so a restatement in any IEEE fp32 arithmetic (tests/trust_ref.py) gives the same
 * bits.  Per element:
 *
 *   sumsq:    d = w - w0;  q = d * d;  acc = acc + q
 *   project:  d = w - w0;  u = c * d;  w = w0 + u
 *
 * Reduction order of the sum of squares (a chunk is 2048 consecutive elements of one tensor, chunk j of a tensor starts at
 * element 2048 * j; no chunk spans two tensors; `first_chunk` of the table numbers the chunks over all tensors):
 *   1. chunk:   thread t (0..255) starts at 0 and adds the q of elements 8 t .. 8 t + 7 of the chunk in index order (elements
 *               past the tensor's end add nothing); the 64 lanes of a wave join by butterfly - for o = 32, 16, 8, 4, 2, 1 every
 *               lane takes v = v + v[lane ^ o] - the chunk's four waves join in wave order, ((p0 + p1) + p2) + p3: one fp32
 *               partial per chunk, `partials[first_chunk + j]`.
 *   2. tensor:  one workgroup of 256 per tensor k: thread t starts at 0 and adds the tensor's partials t, t + 256, t + 512, ...
 *               in index order; butterfly within the wave; the four waves in wave order as above -> per_tensor[k].
 *   3. total:   one workgroup of 256: thread t starts at 0 and adds per_tensor[t], per_tensor[t + 256], ... in index order;
 *               butterfly; the four waves in wave order -> out[0]; out[1] = sqrt(out[0]).
 * No atomics: the same inputs give the same bits.  Where several tables form one ball, the caller adds their out[0] in fp32 in a
 * fixed order and hands the joint total to lcv_trust_project.
 *
 * Conventions are those of lcv_hip_master.h: every function returns 0 or a negative LCV_E* code, takes device pointers,
 * allocates nothing and takes the hipStream_t as a trailing `void* stream`.
 */
#ifndef LCV_HIP_TRUST_H
#define LCV_HIP_TRUST_H

#include <stdint.h>
#include "lcv_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define LCV_TRUST_GLOBAL 0   /* one ball over the whole total `sumsq[0]` */
#define LCV_TRUST_TENSOR 1   /* one ball per tensor over per_tensor[k] */

/* per_tensor[k] = sum of (w - w0)^2 over tensor k, out[0] = their total, out[1] = sqrt(out[0]), in the order above.
 * `partials` is the caller's workspace of at least total_chunks * 4 bytes, `per_tensor` holds n_tensors floats, `out` two.
 * Three launches.  Reads 6 B per parameter at param_f32 = 0 (4 B with low or anchor NULL, 2 B with both), 8 B at param_f32 = 1
 * (4 B with anchor NULL). */
int lcv_trust_sumsq(const lcv_adam_tensor* tensors, void* const* low, void* const* anchor, int64_t n_tensors,
                    int64_t total_chunks, int param_f32, float* partials, int64_t partials_bytes, float* per_tensor, float* out,
                    void* stream);

/* The projection, one launch.  The decision is read from device memory:
 *   scope = LCV_TRUST_GLOBAL:  s = sumsq[0] for every tensor;  r2 = (float)r2_or_R2, where the caller formed R * R * N in double
 *                              (N the number of elements of the whole ball);  per_tensor is not read and may be NULL.
 *   scope = LCV_TRUST_TENSOR:  s = per_tensor[k];  r2 = (float)(r2_or_R2 * (double)numel_k), the caller passing R * R, the
 *                              product formed in double and rounded once.
 *   if (!(s > r2)) the tensor is left alone: no byte of it is written (a NaN s writes nothing either);
 *   t = r2 / s;  c = sqrtf(t);  then per element d = w - w0;  u = c * d;  w = w0 + u.
 * A sum that has overflowed to +inf above a finite r2 is "outside the ball" like any other: t = 0 and c = 0, so every element
 * with a finite d goes back to its base value w0, and an element whose own d is +-inf becomes NaN (0 * inf).  A run whose
 * parameters have overflowed is lost with or without the ball; nothing is done to hide it.
 * A workgroup whose ball holds returns at once.  At param_f32 = 0 `low` is required: a plain bf16 word cannot hold the bound (a
 * contraction below half a bf16 ulp rounds back to the same word).  `sumsq` is a device pointer (the table's own out, or a joint
 * total).  trace_slot, when not NULL, receives from one thread trace_slot[0] = sumsq[0] (the total before the projection) and
 * trace_slot[1] = the smallest coefficient c applied to any tensor (1.0 when nothing was projected).  r2_or_R2 must be > 0 (it
 * may be +inf: nothing is then written).  On a projecting step 6 B read + 4 B written per parameter at param_f32 = 0 (4 + 4
 * with anchor NULL), 8 + 4 at param_f32 = 1 (4 + 4 with anchor NULL); otherwise nothing but the decision is read. */
int lcv_trust_project(const lcv_adam_tensor* tensors, void* const* low, void* const* anchor, int64_t n_tensors,
                      int64_t total_chunks, int param_f32, int scope, const float* sumsq, const float* per_tensor,
                      double r2_or_R2, float* trace_slot, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LCV_HIP_TRUST_H */

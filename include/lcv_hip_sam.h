/*
 * lcv_hip_sam.h - C ABI of the sharpness-aware adaptation step (SAM) of liblcv_hip.so (AMD gfx950, MI355X).
 *
 * SAM (Foret et al. 2021) takes the gradient of a step at the worst nearby point w + rho * g / |g| instead of at w: a first
 * forward/backward gives g, lcv_sam_sumsq measures |g| in a fixed order, lcv_sam_perturb saves every word the forward reads and
 * moves the parameters to the perturbed point, a second forward/backward gives the gradient there, and lcv_sam_restore puts the
 * saved words back, so that the optimizer steps bit-identical parameters with the second gradient.  The host never waits.
 *
 * The descriptor table lists the parameters that hold a gradient.  Its `param`, `grad`, numel and first_chunk are read, the
 * moment pointers are not.  `low` and `save` are device arrays of n_tensors pointers parallel to the table.  Parameters come in
 * two forms, chosen by `param_f32`:
 *   param_f32 = 1   fp32 parameters with fp32 gradients: w is the stored value, `low` must be NULL, a save word is the fp32 value.
 *   param_f32 = 0   bf16 words h with bf16 gradients: w = join(h, l) with the int16 low words of lcv_hip_master.h, or
 *                   w = float(h) when `low` is NULL; a save word is the bf16 word h.
 *
 * Every operation is one correctly rounded IEEE fp32 operation (no product fuses with the sum that takes it; the divide and the
 * square root are the correctly rounded ones), so a restatement in any IEEE fp32 arithmetic (tests/sam_ref.py) gives the same
 * bits.  Per element, with rho_f = (float)rho and eta_f = (float)eta:
 *
 *   plain     (adaptive = 0):  t = g
 *   adaptive  (adaptive = 1):  a = fabsf(w) + eta_f;  t = a * g            (ASAM, Kwon et al. 2021, T_w = |w| + eta)
 *
 *   sumsq:     q = t * t;  acc = acc + q
 *   perturb:   n = sqrtf(s);  den = n + 1e-12f;  c = rho_f / den
 *              plain:     e = c * g
 *              adaptive:  u = a * t;  e = c * u
 *              w' = w + e
 *
 * Reduction order of every sum of squares here (a chunk is 2048 consecutive elements of one tensor, chunk j of a tensor starts at
 * element 2048 * j; no chunk spans two tensors; `first_chunk` of the table numbers the chunks over all tensors).  It is the
 * three-stage order of the trust-region header, written out:
 *   1. chunk:   thread t (0..255) starts at 0 and adds the q of elements 8 t .. 8 t + 7 of the chunk in index order (elements
 *               past the tensor's end add nothing); the 64 lanes of a wave join by butterfly - for o = 32, 16, 8, 4, 2, 1 every
 *               lane takes v = v + v[lane ^ o] - the chunk's four waves join in wave order, ((p0 + p1) + p2) + p3: one fp32
 *               partial per chunk, `partials[first_chunk + j]`.
 *   2. tensor:  one workgroup of 256 per tensor k: thread t starts at 0 and adds the tensor's partials t, t + 256, t + 512, ...
 *               in index order; butterfly within the wave; the four waves in wave order as above -> per_tensor[k].
 *   3. total:   one workgroup of 256: thread t starts at 0 and adds per_tensor[t], per_tensor[t + 256], ... in index order;
 *               butterfly; the four waves in wave order -> out[0]; out[1] = sqrtf(out[0]).
 * No atomics: the same inputs give the same bits.  Where several tables form one ball, the caller adds their out[0] in fp32 in a
 * fixed order and hands the joint total to lcv_sam_perturb.
 *
 * Conventions are those of lcv_hip_master.h: every function returns 0 or a negative LCV_E* code, takes device pointers,
 * allocates nothing and takes the hipStream_t as a trailing `void* stream`.
 */
#ifndef LCV_HIP_SAM_H
#define LCV_HIP_SAM_H

#include <stdint.h>
#include "lcv_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* per_tensor[k] = sum of q = t * t over tensor k, out[0] = their total, out[1] = sqrtf(out[0]), in the order above.  `partials`
 * is the caller's workspace of at least total_chunks * 4 bytes, `per_tensor` holds n_tensors floats, `out` two.  Three launches.
 * With adaptive = 0 the parameters are not read: 2 B per element at param_f32 = 0, 4 B at param_f32 = 1.  With adaptive = 1 the
 * parameters are read too: 6 B per element (4 B with low NULL), 8 B at param_f32 = 1.  eta must be finite and >= 0. */
int lcv_sam_sumsq(const lcv_adam_tensor* tensors, void* const* low, int64_t n_tensors, int64_t total_chunks, int param_f32,
                  int adaptive, double eta, float* partials, int64_t partials_bytes, float* per_tensor, float* out, void* stream);

/* The perturbation.  s = sumsq[0] is read from device memory: the table's own out, or the joint total of several tables.
 * For every element the word the forward reads is first written to save[k][i] (the bf16 word h at param_f32 = 0, the fp32 value
 * at param_f32 = 1), then the perturbed word is stored:
 *   param_f32 = 0:  h' = bf16_rne(w') (round to nearest, ties to even).  The low words are read and never written: the perturbed
 *                   point exists only for the GEMMs, which read h.
 *   param_f32 = 1:  the fp32 w'.
 * When rho_f == 0, or !(s > 0) (this covers a NaN total), or s == +inf: the saves are written, no parameter byte is written and
 * realized is 0.
 * realized[0] is the sum over all elements of d * d with d = float(h') - float(h) (w' - w at param_f32 = 1), in the three-stage
 * order above through `partials` and `per_tensor` (which are overwritten); realized[1] = sqrtf(realized[0]).  This is the
 * perturbation the forward actually sees, and for bf16 words it is NOT rho: a perturbation of an element below half a bf16 ulp of
 * that element rounds away entirely, and one above half an ulp becomes a whole ulp.  A perturbation of norm rho spread over N
 * elements has rho / sqrt(N) per element in RMS; at the whole model's 13.6 G parameters that is far below half an ulp of almost
 * every weight, so almost all of it rounds away and realized[1] is a small fraction of rho (or 0).  Nothing is done to hide this:
 * the trace slot is the honest record of what the second forward saw.  fp32 parameters hold realized[1] = rho up to rounding.
 * trace_slot, when not NULL, receives from one thread trace_slot[0] = s and trace_slot[1] = realized[0].
 * rho and eta must be finite and >= 0.  Three launches.  Per element at param_f32 = 0: 6 B read (4 B with low NULL) + 4 B written;
 * at param_f32 = 1: 8 B read + 8 B written. */
int lcv_sam_perturb(const lcv_adam_tensor* tensors, void* const* low, void* const* save, int64_t n_tensors, int64_t total_chunks,
                    int param_f32, int adaptive, double eta, double rho, const float* sumsq, float* partials,
                    int64_t partials_bytes, float* per_tensor, float* realized, float* trace_slot, void* stream);

/* param[k][i] = save[k][i], word for word (2 B words at param_f32 = 0, 4 B at param_f32 = 1), one launch.  After it every
 * parameter byte is what it was before lcv_sam_perturb; no low word was ever touched. */
int lcv_sam_restore(const lcv_adam_tensor* tensors, void* const* save, int64_t n_tensors, int64_t total_chunks, int param_f32,
                    void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LCV_HIP_SAM_H */

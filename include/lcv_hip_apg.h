/*
 * lcv_hip_apg.h - C ABI of the adaptive projected guidance of the CFG denoise loop of liblcv_hip.so (AMD gfx950, MI355X).
 *
 * Plain classifier-free guidance forms v = u' + g (c - u') from the prompt row's output c and the (zero-star scaled) negative
 * row's output u'.  Adaptive projected guidance (Sadat et al. 2024) splits the correction d = c - u' into the part parallel to c,
 * which inflates the magnitude, and the part orthogonal to it; it scales the parallel part by eta, caps the correction's norm at
 * a radius and optionally carries a momentum over the steps:
 *   d = (c - u') + beta * d_old;   s = min(1, radius / ||d||);   p = s (<d, c> / <c, c>) c;   v = c + (g - 1) ((s d - p) + eta p)
 * With eta = 1, no radius and beta = 0 this is the plain rule in value (not in bits: the operations differ).  The result goes to
 * the existing unguided updates (lcv_euler_step, or lcv_cfg_lms_step with uncond = NULL).  What eta, radius and beta are, and
 * when the momentum restarts, is the caller's business (longcat_video/apg.py): this header knows none.
 *
 * cond, uncond, diff, v are [B, n] fp32, contiguous.  Every operation is one correctly rounded IEEE fp32 operation and no
 * product fuses with a sum (the source is built with -ffp-contract=off), so a numpy or torch fp32 restatement that takes the
 * operations one at a time gives the same bits.
 *
 * Conventions are those of lcv_hip_cfgreuse.h: a function returns 0 or a negative LCV_E* code, takes device pointers, allocates
 * nothing and takes the hipStream_t as a trailing `void* stream`.  Pointers need only be 4-byte aligned (a view into a larger
 * tensor is fine) and n >= 1 is arbitrary: every element takes the one scalar path.  No atomics; every output has one writer and
 * is a pure function of the inputs.
 */
#ifndef LCV_HIP_APG_H
#define LCV_HIP_APG_H

#include <stdint.h>
#include "lcv_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ws is [2][B][256][4] floats: ws[0] the zero-star partial pairs (dot, nrm, 0, 0), ws[1] the partial sums (dd, dc, cc, 0) of the
 * correction.  All sums are fixed-order, in the two-level scheme of lcv_cfg_delta_store (lcv_hip_cfgreuse.h): a launch has always
 * 256 workgroups of 256 threads per sample; thread t of workgroup `part` starts from 0 and takes the elements part * 256 + t,
 * + 65536, + 2 * 65536, ... in index order; the 64 lanes of a wave join by butterfly (v = v + v[lane ^ o] for o = 32, 16, 8, 4,
 * 2, 1), the four waves in wave order ((s0 + s1) + s2) + s3, and the sums go to ws[.][b][part][0..3]: every slot is written,
 * empty slices write 0, the unused slots hold 0.
 *
 * Launch 0 (use_zero_star only), with c = cond[b, i] and u = uncond[b, i]:
 *   p = c * u;  dot = dot + p;  q = u * u;  nrm = nrm + q                                          -> ws[0][b][part][0..1]
 * Launch 1.  Under zero-star every workgroup first adds the 256 pairs of ws[0][b] the same way (thread t holds pair t; butterfly;
 * waves in wave order) and forms st[b] = dot / (nrm + 1e-8f): one fp32 addition, one correctly rounded fp32 division - the bits
 * lcv_cfg_delta_store and lcv_cfg_lms_step form from the same cond and uncond.  Then per element, with o = diff[b, i] as it was
 * before the call:
 *   u' = u * st[b]  (use_zero_star)  or  u' = u
 *   d = c - u'
 *   m = beta * o;  d = d + m          (only when have_momentum is set and beta != 0; otherwise the old diff is not read)
 *   diff[b, i] = d
 *   p = d * d;  dd = dd + p;   q = d * c;  dc = dc + q;   r = c * c;  cc = cc + r                  -> ws[1][b][part][0..2]
 * Launch 2.  Every workgroup adds the 256 triples of ws[1][b] the same way, then forms per sample
 *   s = 1  when radius <= 0 or dd == 0;  otherwise  nrm = sqrtf(dd) (correctly rounded);  q = radius / nrm;  s = q < 1 ? q : 1
 *   den = cc + 1e-8f;  k = dc / den
 * and per element, with d = diff[b, i]:
 *   ds = s * d;  p = k * c;  p = s * p;  o = ds - p;  e = eta * p;  w = o + e;  t = gm1 * w;  v[b, i] = c + t
 * gm1 = guidance - 1.0f is one fp32 subtraction made on the host by this function, from the fp32 `guidance` it is handed.
 * With out given ([B][4] floats), workgroup 0 of each sample writes out[b] = (dd, dc, cc, s) with plain stores.
 *
 * diff is the momentum state when beta != 0 and scratch otherwise; it is always written.  v may be cond (the model output is
 * overwritten by the guided one; then cond is read by launch 1 and read and written by launch 2); otherwise cond is never
 * written, and uncond never is.  diff must not overlap cond, uncond or v anywhere, and v must not overlap uncond (the launcher
 * can only refuse equal base pointers).  LCV_EINVAL without a launch: cond, uncond, diff, v or ws NULL; v or diff equal to
 * uncond; diff equal to cond or v; B above 65535.  B == 0 or n == 0 returns LCV_OK.
 * Same inputs give the same bits.
 * Per element: 4 B of each of cond and uncond read under zero-star (launch 0); 4 B of each of cond and uncond read, 4 B of diff
 * read under momentum and 4 B written (launch 1); 4 B of each of cond and diff read and 4 B written (launch 2): 36 B under
 * zero-star with momentum, 28 B without zero-star. */
int lcv_cfg_apg(const float* cond, const float* uncond, float* diff, float* v, float* ws, float* out, int64_t B, int64_t n,
                float guidance, float eta, float radius, float beta, int use_zero_star, int have_momentum, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LCV_HIP_APG_H */

/*
 * lcv_hip_cfgreuse.h - C ABI of the guidance reuse of the CFG denoise loop of liblcv_hip.so (AMD gfx950, MI355X).
 *
 * A CFG step runs the model on the negative row only to form the guidance correction delta = v - c, v the guided output of
 * lcv_cfg_euler_step / lcv_cfg_lms_step (before the pipeline's sign) and c the prompt row's output.  The correction moves slowly
 * from step to step: a full step stores it (lcv_cfg_delta_store), a reuse step runs the prompt row alone and adds the stored
 * correction back (lcv_cfg_delta_apply); the result goes to the existing unguided updates (lcv_euler_step, or lcv_cfg_lms_step
 * with uncond = NULL).  Which steps are full is the caller's schedule (longcat_video/cfg_reuse.py): this header knows none.
 *
 * cond, uncond, delta, v are [B, n] fp32, contiguous.  Every operation is one correctly rounded IEEE fp32 operation and no
 * product fuses with a sum (the source is built with -ffp-contract=off), so a numpy or torch fp32 restatement that takes the
 * operations one at a time gives the same bits.
 *
 * Conventions are those of lcv_hip.h: a function returns 0 or a negative LCV_E* code, takes device pointers, allocates nothing
 * and takes the hipStream_t as a trailing `void* stream`.  Pointers need only be 4-byte aligned (a view into a larger tensor is
 * fine) and n >= 1 is arbitrary: every element takes the one scalar path.  No atomics, no scratch; every output has one writer
 * and is a pure function of the inputs.
 */
#ifndef LCV_HIP_CFGREUSE_H
#define LCV_HIP_CFGREUSE_H

#include <stdint.h>
#include "lcv_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Per sample b and element i, with c = cond[b, i] and o = delta[b, i] as it was before the call:
 *   u = uncond[b, i] * st[b]  (use_zero_star)  or  u = uncond[b, i]
 *   d = c - u;   t = guidance * d;   v = u + t;   e = v - c;   delta[b, i] = e
 *   out given:  q = e - o;  a = |q|;  num = num + a;   m = |o|;  den = den + m
 * cond and uncond are never written.  With out = NULL the old delta is not read, no drift partials are formed and no last
 * launch is made (the first full step of a denoise: there is no earlier correction).
 *
 * ws is [2][B][256][2] floats: ws[0] the zero-star partial pairs (dot, nrm), ws[1] the drift partial pairs (num, den).  Both
 * pairs of sums are fixed-order, in the two-level scheme of lcv_cfg_lms_step (lcv_hip_solver.h): a launch has always 256
 * workgroups of 256 threads per sample; thread t of workgroup `part` starts from 0 and takes the elements part * 256 + t,
 * + 65536, + 2 * 65536, ... in index order; the 64 lanes of a wave join by butterfly (v = v + v[lane ^ o] for o = 32, 16, 8, 4,
 * 2, 1), the four waves in wave order ((s0 + s1) + s2) + s3, and the pair goes to ws[.][b][part][0..1]: every slot is written,
 * empty slices write 0.
 *   zero-star (a launch of its own, before the store launch):  p = c * u;  dot = dot + p;  q = u * u;  nrm = nrm + q  over the
 *   raw uncond; every workgroup of the store launch then adds the 256 pairs the same way (thread t holds pair t; butterfly;
 *   waves in wave order) and forms st[b] = dot / (nrm + 1e-8f): one fp32 addition, one correctly rounded fp32 division - the bits
 *   lcv_cfg_lms_step forms from the same cond and uncond.
 *   drift (in the store launch itself; the thread that overwrites delta[b, i] has read it first):  a last launch of one
 *   256-thread workgroup per sample adds the 256 pairs the same way and one lane writes out[b][0] = num, out[b][1] = den with
 *   plain stores.  out is [B][2] floats.  The step's distance max_b num[b] / den[b] is the caller's to form.
 * Same inputs give the same bits.
 *
 * delta must not overlap cond or uncond anywhere (the launcher can only refuse equal base pointers).  LCV_EINVAL without a
 * launch: cond, uncond or delta NULL; delta equal to cond or uncond; ws NULL when use_zero_star is set or out is given; B above
 * 65535.  B == 0 or n == 0 returns LCV_OK.
 * Per element: 4 B of each of cond and uncond read (both once more under zero-star), 4 B of delta read when out is given, 4 B
 * written. */
int lcv_cfg_delta_store(const float* cond, const float* uncond, float* delta, float* ws, float* out, int64_t B, int64_t n,
                        float guidance, int use_zero_star, void* stream);

/* v[b, i] = cond[b, i] + delta[b, i]: the guided output of a reuse step, one operation per element.  v may be cond (the model
 * output is overwritten by the guided one); delta is never written.  LCV_EINVAL without a launch: cond, delta or v NULL;
 * v equal to delta.  B == 0 or n == 0 returns LCV_OK.
 * Per element: 8 B read, 4 B written. */
int lcv_cfg_delta_apply(const float* cond, const float* delta, float* v, int64_t B, int64_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LCV_HIP_CFGREUSE_H */

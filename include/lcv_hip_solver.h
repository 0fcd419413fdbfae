/*
 * lcv_hip_solver.h - C ABI of the linear multistep update of the denoise loop of liblcv_hip.so (AMD gfx950, MI355X).
 *
 * The denoise loop integrates dx/dsigma = f(x, sigma) over the scheduler's sigma grid.  lcv_cfg_euler_step / lcv_euler_step
 * (lcv_hip.h) take the explicit Euler step x += h f_i.  This entry point forms the same guided velocity f_i, keeps it, and takes
 * a linear multistep step x += w0 f_i + w1 f_{i-1} + w2 f_{i-2} over the velocities of up to two earlier steps: with the weights
 * of longcat_video/solver.py the two-step Adams-Bashforth rule (`ab2`) and its predictor-corrector form (`ab2c`), both second
 * order, neither with a further forward of the model.  The weights are the caller's: this header knows no rule.
 *
 * cond, uncond, x, f0, f1, f2 are [B, n] fp32, contiguous.  Every operation is one correctly rounded IEEE fp32 operation and no
 * product fuses with a sum (the source is built with -ffp-contract=off), so a numpy or torch fp32 restatement that takes the
 * operations one at a time gives the same bits.
 *
 * Conventions are those of lcv_hip.h: the function returns 0 or a negative LCV_E* code, takes device pointers, allocates
 * nothing and takes the hipStream_t as a trailing `void* stream`.  Pointers need only be 4-byte aligned (a view into a larger
 * tensor is fine) and n >= 1 is arbitrary: every element takes the one scalar path.  No atomics, no scratch; every output has
 * one writer and is a pure function of the inputs.
 */
#ifndef LCV_HIP_SOLVER_H
#define LCV_HIP_SOLVER_H

#include <stdint.h>
#include "lcv_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Per sample b and element i, with c = cond[b, i]:
 *   uncond given:  u = uncond[b, i] * st[b]  (use_zero_star)  or  u = uncond[b, i];   d = c - u;  t = guidance * d;  v = u + t
 *   uncond NULL:   v = c                     (no guidance; `guidance`, `use_zero_star` and `ws` are not read)
 *   f = negate ? -v : v;   f0[b, i] = f
 *   a = w0 * f;   terms >= 2:  p = w1 * f1[b, i];  a = a + p;   terms >= 3:  p = w2 * f2[b, i];  a = a + p
 *   x[b, i] = x[b, i] + a
 * f1 is read only at terms >= 2 and f2 only at terms == 3 (w1, w2 are not read below that); f1 and f2 are never written.
 *
 * The zero-star scale st[b] = <c, u> / (<u, u> + 1e-8f) (one fp32 addition, one correctly rounded fp32 division) comes from
 * fixed-order sums, in the two-level scheme of lcv_cfg_euler_step: a first launch of 256 workgroups of 256 threads per sample
 * writes 256 partial pairs (dot, nrm) to ws[b][part][2] (B * 256 * 2 floats, every slot written, empty slices write 0).  Thread
 * t of workgroup `part` starts from dot = nrm = 0 and takes the elements part * 256 + t, + 65536, + 2 * 65536, ... in index
 * order, each as  p = c * u;  dot = dot + p;  q = u * u;  nrm = nrm + q.  The 64 lanes of a wave join by butterfly
 * (v = v + v[lane ^ o] for o = 32, 16, 8, 4, 2, 1), the four waves in wave order ((s0 + s1) + s2) + s3.  Every workgroup of the
 * step launch then adds the 256 partials the same way (thread t holds partial t; butterfly; waves in wave order), so all of
 * them hold the same st.  Same inputs give the same bits.
 *
 * f0 must not overlap x, f1, f2, cond or uncond anywhere, and x must overlap none of the others (the launcher can only refuse
 * equal base pointers; a partial overlap is the caller's error and gives undefined results).  LCV_EINVAL without a launch: cond, x or f0 NULL; f0 equal to one of the other
 * pointers; terms outside 1..3; f1 NULL at terms >= 2; f2 NULL at terms == 3; ws NULL when uncond is given and use_zero_star
 * is set; B above 65535.  B == 0 or n == 0 returns LCV_OK.
 * Per element: 4 B of each of cond, uncond, x and the history terms read (cond and uncond once more under zero-star), 8 B
 * written. */
int lcv_cfg_lms_step(const float* cond, const float* uncond, float* x, float* f0, const float* f1, const float* f2, float* ws,
                     int64_t B, int64_t n, float guidance, float w0, float w1, float w2, int terms, int negate,
                     int use_zero_star, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LCV_HIP_SOLVER_H */

// The linear multistep update of the denoise loop (include/lcv_hip_solver.h): the guided velocity f_i of lcv_cfg_euler_step,
// kept in f0, and x += w0 f_i + w1 f_{i-1} + w2 f_{i-2} over the velocities of up to two earlier steps.  HBM-bound fp32
// streaming, one scalar path for every element (pointers are only 4-byte aligned, n is arbitrary), grid-stride loops.  Built
// with -ffp-contract=off: every operation below is one rounded fp32 operation, written one per statement.  The zero-star sums,
// st and the guided value are csrc/cfg_guidance.h's, the one definition this file shares with elementwise.hip and
// cfg_reuse.hip; LDS holds the wave-order join only.  No atomics.
#include "lcv_common.h"   // the argument and launch checks
#include "lcv_hip_solver.h"

#pragma clang fp contract(off)   // ahead of the shared helpers: in this file they do not contract either
#include "cfg_guidance.h"

static constexpr int LMS_MAX_BLOCKS = 1024;

__global__ __launch_bounds__(CFG_THREADS) void lms_dot_kernel(const float* __restrict__ cond, const float* __restrict__ uncond,
                                                              float* __restrict__ ws, int64_t n) {
  __shared__ CfgJoinLds sa, sb;
  cfg_partial_sums(cond, uncond, ws, n, sa, sb);
}

// GUIDED: uncond is given.  f1 / f2 are read only where `terms` asks for them.
template <bool GUIDED>
__global__ __launch_bounds__(CFG_THREADS) void lms_step_kernel(const float* __restrict__ cond, const float* __restrict__ uncond,
                                                               float* __restrict__ x, float* __restrict__ f0,
                                                               const float* __restrict__ f1, const float* __restrict__ f2,
                                                               const float* __restrict__ ws, int64_t n, float guidance, float w0,
                                                               float w1, float w2, int terms, int negate, int use_zero_star) {
  __shared__ CfgJoinLds sa, sb;
  const int64_t b = blockIdx.y;
  float st = 1.0f;
  if (GUIDED && use_zero_star) st = cfg_star_scale(ws, b, sa, sb);
  const int64_t base = b * n;
  for (int64_t i = (int64_t)blockIdx.x * CFG_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * CFG_THREADS) {
    const int64_t at = base + i;
    float v = cond[at];
    if (GUIDED) v = cfg_guided(v, uncond[at], st, guidance, use_zero_star);
    const float f = negate ? -v : v;
    f0[at] = f;
    float a = w0 * f;
    if (terms >= 2) {
      const float p = w1 * f1[at];
      a = a + p;
    }
    if (terms >= 3) {
      const float p = w2 * f2[at];
      a = a + p;
    }
    x[at] = x[at] + a;
  }
}

extern "C" int lcv_cfg_lms_step(const float* cond, const float* uncond, float* x, float* f0, const float* f1, const float* f2,
                                float* ws, int64_t B, int64_t n, float guidance, float w0, float w1, float w2, int terms,
                                int negate, int use_zero_star, void* stream) {
  LCV_CHECK_ARG(cond && x && f0, "cfg_lms_step: cond, x or f0 is a null pointer");
  LCV_CHECK_ARG(terms >= 1 && terms <= 3, "cfg_lms_step: terms must be in 1..3, got %d", terms);
  LCV_CHECK_ARG(terms < 2 || f1, "cfg_lms_step: %d terms need f1", terms);
  LCV_CHECK_ARG(terms < 3 || f2, "cfg_lms_step: 3 terms need f2");
  LCV_CHECK_ARG(f0 != x && f0 != cond && f0 != uncond && f0 != f1 && f0 != f2, "cfg_lms_step: f0 must be a buffer of its own");
  LCV_CHECK_ARG(!(uncond && use_zero_star) || ws, "cfg_lms_step: zero-star needs the workspace");
  LCV_CHECK_ARG(B >= 0 && n >= 0 && B <= 65535, "cfg_lms_step: B must be in 0..65535 and n >= 0, got %ld and %ld", (long)B, (long)n);
  if (B == 0 || n == 0) return LCV_OK;
  hipStream_t s = (hipStream_t)stream;
  int64_t bx = (n + CFG_THREADS - 1) / CFG_THREADS;
  if (bx > LMS_MAX_BLOCKS) bx = LMS_MAX_BLOCKS;
  const dim3 grid((unsigned)bx, (unsigned)B), block(CFG_THREADS);
  if (!uncond) {
    hipLaunchKernelGGL(lms_step_kernel<false>, grid, block, 0, s, cond, (const float*)nullptr, x, f0, f1, f2,
                       (const float*)nullptr, n, guidance, w0, w1, w2, terms, negate, 0);
    LCV_LAUNCH_CHECK("cfg_lms_step");
    return LCV_OK;
  }
  if (use_zero_star) {   // always CFG_PARTS workgroups per sample: every partial slot is written (empty slices write 0)
    hipLaunchKernelGGL(lms_dot_kernel, dim3(CFG_PARTS, (unsigned)B), block, 0, s, cond, uncond, ws, n);
    LCV_LAUNCH_CHECK("cfg_lms_step: sums");
  }
  hipLaunchKernelGGL(lms_step_kernel<true>, grid, block, 0, s, cond, uncond, x, f0, f1, f2, (const float*)ws, n, guidance, w0, w1,
                     w2, terms, negate, use_zero_star);
  LCV_LAUNCH_CHECK("cfg_lms_step");
  return LCV_OK;
}

// The linear multistep update of the denoise loop (include/lcv_hip_solver.h): the guided velocity f_i of lcv_cfg_euler_step,
// kept in f0, and x += w0 f_i + w1 f_{i-1} + w2 f_{i-2} over the velocities of up to two earlier steps.  HBM-bound fp32
// streaming, one scalar path for every element (pointers are only 4-byte aligned, n is arbitrary), grid-stride loops.  Built
// with -ffp-contract=off: every operation below is one rounded fp32 operation, written one per statement.  The zero-star sums
// are fixed-order, in the two-level scheme of cfg_dot_kernel / cfg_euler_kernel (elementwise.hip); LDS holds the wave-order
// join only.  No atomics.
#include "lcv_common.h"   // wave_sum, the argument and launch checks
#include "lcv_hip_solver.h"

#pragma clang fp contract(off)

static constexpr int LMS_PARTS = 256;     // workgroups (= partial pairs) per sample of the zero-star sums
static constexpr int LMS_THREADS = 256;   // one thread per partial in the step launch's join: must equal LMS_PARTS
static constexpr int LMS_MAX_BLOCKS = 1024;

// ws[b][part][2] = the (dot, nrm) of the elements part * 256 + t + k * 65536 of sample b; every slot is written
__global__ __launch_bounds__(LMS_THREADS) void lms_dot_kernel(const float* __restrict__ cond, const float* __restrict__ uncond,
                                                              float* __restrict__ ws, int64_t n) {
  __shared__ float sd[LMS_THREADS / LCV_WAVE], sn[LMS_THREADS / LCV_WAVE];
  const int64_t b = blockIdx.y;
  const float* c = cond + b * n;
  const float* u = uncond + b * n;
  float dot = 0.f, nrm = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * LMS_THREADS + threadIdx.x; i < n; i += (int64_t)LMS_PARTS * LMS_THREADS) {
    const float cv = c[i], uv = u[i];
    const float p = cv * uv;
    dot = dot + p;
    const float q = uv * uv;
    nrm = nrm + q;
  }
  dot = wave_sum(dot);
  nrm = wave_sum(nrm);
  if ((threadIdx.x & (LCV_WAVE - 1)) == 0) { sd[threadIdx.x / LCV_WAVE] = dot; sn[threadIdx.x / LCV_WAVE] = nrm; }
  __syncthreads();
  if (threadIdx.x == 0) {
    float* o = ws + (b * LMS_PARTS + blockIdx.x) * 2;
    o[0] = ((sd[0] + sd[1]) + sd[2]) + sd[3];
    o[1] = ((sn[0] + sn[1]) + sn[2]) + sn[3];
  }
}

// GUIDED: uncond is given.  f1 / f2 are read only where `terms` asks for them.
template <bool GUIDED>
__global__ __launch_bounds__(LMS_THREADS) void lms_step_kernel(const float* __restrict__ cond, const float* __restrict__ uncond,
                                                               float* __restrict__ x, float* __restrict__ f0,
                                                               const float* __restrict__ f1, const float* __restrict__ f2,
                                                               const float* __restrict__ ws, int64_t n, float guidance, float w0,
                                                               float w1, float w2, int terms, int negate, int use_zero_star) {
  __shared__ float sd[LMS_THREADS / LCV_WAVE], sn[LMS_THREADS / LCV_WAVE];
  const int64_t b = blockIdx.y;
  float st = 1.0f;
  if (GUIDED && use_zero_star) {   // every workgroup adds the 256 partial pairs in the same order (2 KiB from L2)
    const float* o = ws + (b * LMS_PARTS + threadIdx.x) * 2;
    const float d = wave_sum(o[0]), q = wave_sum(o[1]);
    if ((threadIdx.x & (LCV_WAVE - 1)) == 0) { sd[threadIdx.x / LCV_WAVE] = d; sn[threadIdx.x / LCV_WAVE] = q; }
    __syncthreads();
    const float dot = ((sd[0] + sd[1]) + sd[2]) + sd[3];
    const float nrm = ((sn[0] + sn[1]) + sn[2]) + sn[3];
    const float den = nrm + 1e-8f;
    st = dot / den;
  }
  const int64_t base = b * n;
  for (int64_t i = (int64_t)blockIdx.x * LMS_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * LMS_THREADS) {
    const int64_t at = base + i;
    float v = cond[at];
    if (GUIDED) {
      float u = uncond[at];
      if (use_zero_star) u = u * st;
      const float d = v - u;
      const float t = guidance * d;
      v = u + t;
    }
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
  int64_t bx = (n + LMS_THREADS - 1) / LMS_THREADS;
  if (bx > LMS_MAX_BLOCKS) bx = LMS_MAX_BLOCKS;
  const dim3 grid((unsigned)bx, (unsigned)B), block(LMS_THREADS);
  if (!uncond) {
    hipLaunchKernelGGL(lms_step_kernel<false>, grid, block, 0, s, cond, (const float*)nullptr, x, f0, f1, f2,
                       (const float*)nullptr, n, guidance, w0, w1, w2, terms, negate, 0);
    LCV_LAUNCH_CHECK("cfg_lms_step");
    return LCV_OK;
  }
  if (use_zero_star) {   // always LMS_PARTS workgroups per sample: every partial slot is written (empty slices write 0)
    hipLaunchKernelGGL(lms_dot_kernel, dim3(LMS_PARTS, (unsigned)B), block, 0, s, cond, uncond, ws, n);
    LCV_LAUNCH_CHECK("cfg_lms_step: sums");
  }
  hipLaunchKernelGGL(lms_step_kernel<true>, grid, block, 0, s, cond, uncond, x, f0, f1, f2, (const float*)ws, n, guidance, w0, w1,
                     w2, terms, negate, use_zero_star);
  LCV_LAUNCH_CHECK("cfg_lms_step");
  return LCV_OK;
}

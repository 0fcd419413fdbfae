// Adaptive projected guidance of the CFG denoise loop (include/lcv_hip_apg.h): the correction d = c - u' is split into the part
// parallel to the prompt row's output c and the part orthogonal to it, the parallel part is scaled by eta, the correction's norm
// is capped at a radius and it may carry a momentum over the steps.  HBM-bound fp32 streaming, one scalar path for every element
// (pointers are only 4-byte aligned, n is arbitrary).  Built with -ffp-contract=off: every operation below is one rounded fp32
// operation, written one per statement.  The zero-star sums, st and the pair join are csrc/cfg_guidance.h's, the one definition
// this file shares with elementwise.hip, solver_step.hip and cfg_reuse.hip; the three sums of the correction are joined the same
// way, with a third LDS array beside the pair's.  No atomics.
#include "lcv_common.h"   // the argument and launch checks
#include "lcv_hip_apg.h"

#pragma clang fp contract(off)   // ahead of the shared helpers: in this file they do not contract either
#include "cfg_guidance.h"

static constexpr int APG_SLOTS = 4;   // floats per part in ws: (dot, nrm, 0, 0) and (dd, dc, cc, 0)

// The workgroup's sums of one triple per thread: the third value's wave sums go to LDS ahead of the pair's, whose barrier covers
// them.  apg_triple_total: the four waves in wave order, for whichever threads want the totals.
__device__ __forceinline__ void apg_triple_waves(float a, float b, float c, CfgJoinLds& sa, CfgJoinLds& sb, CfgJoinLds& sc) {
  c = wave_sum(c);
  if ((threadIdx.x & (LCV_WAVE - 1)) == 0) sc[threadIdx.x / LCV_WAVE] = c;
  cfg_pair_waves(a, b, sa, sb);
}
__device__ __forceinline__ void apg_triple_total(float& a, float& b, float& c, const CfgJoinLds& sa, const CfgJoinLds& sb,
                                                 const CfgJoinLds& sc) {
  cfg_pair_total(a, b, sa, sb);
  c = ((sc[0] + sc[1]) + sc[2]) + sc[3];
}

// launch 0: the zero-star partial pairs into the first two of a part's four slots, 0 into the other two
__global__ __launch_bounds__(CFG_THREADS) void apg_dot_kernel(const float* __restrict__ cond, const float* __restrict__ uncond,
                                                              float* __restrict__ ws, int64_t n) {
  __shared__ CfgJoinLds sa, sb;
  cfg_partial_sums<APG_SLOTS>(cond, uncond, ws, n, sa, sb);
  if (threadIdx.x == 0) {
    float* o = ws + ((int64_t)blockIdx.y * CFG_PARTS + blockIdx.x) * APG_SLOTS;
    o[2] = 0.f;
    o[3] = 0.f;
  }
}

// launch 1: diff = (c - u') [+ beta * diff], and (dd, dc, cc, 0) of part blockIdx.x to ws_sums[b][part][4].  Always CFG_PARTS
// workgroups per sample, so the slices are those of apg_dot_kernel.  MOMENTUM: the old diff is read before it is overwritten.
template <bool MOMENTUM>
__global__ __launch_bounds__(CFG_THREADS) void apg_diff_kernel(const float* __restrict__ cond, const float* __restrict__ uncond,
                                                               float* diff, const float* __restrict__ ws_star,
                                                               float* __restrict__ ws_sums, int64_t n, float beta,
                                                               int use_zero_star) {
  __shared__ CfgJoinLds sa, sb, sc;
  const int64_t b = blockIdx.y;
  float st = 1.0f;
  if (use_zero_star) {
    st = cfg_star_scale<APG_SLOTS>(ws_star, b, sa, sb);
    __syncthreads();   // the join below writes the same LDS words
  }
  const int64_t base = b * n;
  float dd = 0.f, dc = 0.f, cc = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * CFG_THREADS + threadIdx.x; i < n; i += (int64_t)CFG_PARTS * CFG_THREADS) {
    const int64_t at = base + i;
    const float c = cond[at];
    float u = uncond[at];
    if (use_zero_star) u = u * st;
    float d = c - u;
    if (MOMENTUM) {
      const float m = beta * diff[at];
      d = d + m;
    }
    diff[at] = d;
    const float p = d * d;
    dd = dd + p;
    const float q = d * c;
    dc = dc + q;
    const float r = c * c;
    cc = cc + r;
  }
  apg_triple_waves(dd, dc, cc, sa, sb, sc);
  if (threadIdx.x == 0) {
    apg_triple_total(dd, dc, cc, sa, sb, sc);
    float* o = ws_sums + (b * CFG_PARTS + blockIdx.x) * APG_SLOTS;
    o[0] = dd;
    o[1] = dc;
    o[2] = cc;
    o[3] = 0.f;
  }
}

// launch 2: every workgroup adds the 256 triples again, forms s and k, and writes v over its slice; v may be cond (each element
// is read and written by one thread), so neither carries __restrict__
__global__ __launch_bounds__(CFG_THREADS) void apg_apply_kernel(const float* cond, const float* __restrict__ diff, float* v,
                                                                const float* __restrict__ ws_sums, float* __restrict__ out,
                                                                int64_t n, float gm1, float eta, float radius) {
  __shared__ CfgJoinLds sa, sb, sc;
  const int64_t b = blockIdx.y;
  const float* o = ws_sums + (b * CFG_PARTS + threadIdx.x) * APG_SLOTS;
  float dd = o[0], dc = o[1], cc = o[2];
  apg_triple_waves(dd, dc, cc, sa, sb, sc);
  apg_triple_total(dd, dc, cc, sa, sb, sc);
  float s = 1.0f;
  if (radius > 0.f && dd != 0.f) {
    const float nrm = sqrtf(dd);
    const float q = radius / nrm;
    s = q < 1.0f ? q : 1.0f;
  }
  const float den = cc + 1e-8f;
  const float k = dc / den;
  if (out && blockIdx.x == 0 && threadIdx.x == 0) {
    float* r = out + b * 4;
    r[0] = dd;
    r[1] = dc;
    r[2] = cc;
    r[3] = s;
  }
  const int64_t base = b * n;
  for (int64_t i = (int64_t)blockIdx.x * CFG_THREADS + threadIdx.x; i < n; i += (int64_t)CFG_PARTS * CFG_THREADS) {
    const int64_t at = base + i;
    const float c = cond[at];
    const float d = diff[at];
    const float ds = s * d;
    float p = k * c;
    p = s * p;
    const float orth = ds - p;
    const float e = eta * p;
    const float w = orth + e;
    const float t = gm1 * w;
    v[at] = c + t;
  }
}

extern "C" int lcv_cfg_apg(const float* cond, const float* uncond, float* diff, float* v, float* ws, float* out, int64_t B,
                           int64_t n, float guidance, float eta, float radius, float beta, int use_zero_star, int have_momentum,
                           void* stream) {
  LCV_CHECK_ARG(cond && uncond && diff && v && ws, "cfg_apg: cond, uncond, diff, v or ws is a null pointer");
  LCV_CHECK_ARG(v != uncond && diff != uncond, "cfg_apg: v and diff must not be uncond (v may be cond)");
  LCV_CHECK_ARG(diff != cond && diff != v, "cfg_apg: diff must be a buffer of its own");
  LCV_CHECK_ARG(B >= 0 && n >= 0 && B <= 65535, "cfg_apg: B must be in 0..65535 and n >= 0, got %ld and %ld", (long)B, (long)n);
  if (B == 0 || n == 0) return LCV_OK;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(CFG_PARTS, (unsigned)B), block(CFG_THREADS);   // always CFG_PARTS workgroups per sample: every slot is written
  const float* ws_star = ws;
  float* ws_sums = ws + B * CFG_PARTS * APG_SLOTS;
  const float gm1 = guidance - 1.0f;   // one fp32 subtraction, here on the host (the header says so)
  if (use_zero_star) {
    hipLaunchKernelGGL(apg_dot_kernel, grid, block, 0, s, cond, uncond, ws, n);
    LCV_LAUNCH_CHECK("cfg_apg: zero-star sums");
  }
  if (have_momentum && beta != 0.f)
    hipLaunchKernelGGL(apg_diff_kernel<true>, grid, block, 0, s, cond, uncond, diff, ws_star, ws_sums, n, beta, use_zero_star);
  else
    hipLaunchKernelGGL(apg_diff_kernel<false>, grid, block, 0, s, cond, uncond, diff, ws_star, ws_sums, n, beta, use_zero_star);
  LCV_LAUNCH_CHECK("cfg_apg: correction");
  hipLaunchKernelGGL(apg_apply_kernel, grid, block, 0, s, cond, (const float*)diff, v, (const float*)ws_sums, out, n, gm1, eta,
                     radius);
  LCV_LAUNCH_CHECK("cfg_apg");
  return LCV_OK;
}

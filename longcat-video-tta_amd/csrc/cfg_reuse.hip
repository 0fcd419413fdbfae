// Guidance reuse of the CFG denoise loop (include/lcv_hip_cfgreuse.h): a full step stores the correction delta = v - c of the
// guided output over the prompt row's, a reuse step adds it back to a prompt-only output.  HBM-bound fp32 streaming, one scalar
// path for every element (pointers are only 4-byte aligned, n is arbitrary).  Built with -ffp-contract=off: every operation
// below is one rounded fp32 operation, written one per statement.  The zero-star sums, st, the guided value and the pair join that
// the drift sums use too are csrc/cfg_guidance.h's, the one definition this file shares with elementwise.hip and
// solver_step.hip; LDS holds the wave-order join only.  No atomics.
#include "lcv_common.h"   // the argument and launch checks
#include "lcv_hip_cfgreuse.h"

#pragma clang fp contract(off)   // ahead of the shared helpers: in this file they do not contract either
#include "cfg_guidance.h"

static constexpr int CGR_MAX_BLOCKS = 1024;

__global__ __launch_bounds__(CFG_THREADS) void cgr_dot_kernel(const float* __restrict__ cond, const float* __restrict__ uncond,
                                                              float* __restrict__ ws, int64_t n) {
  __shared__ CfgJoinLds sa, sb;
  cfg_partial_sums(cond, uncond, ws, n, sa, sb);
}

// DRIFT: the old delta is read before it is overwritten and (num, den) of part blockIdx.x goes to ws_drift[b][part][2].
// Always CFG_PARTS workgroups per sample, so the slices are those of cgr_dot_kernel.
template <bool DRIFT>
__global__ __launch_bounds__(CFG_THREADS) void cgr_store_kernel(const float* __restrict__ cond, const float* __restrict__ uncond,
                                                                float* delta, const float* __restrict__ ws_star,
                                                                float* __restrict__ ws_drift, int64_t n, float guidance,
                                                                int use_zero_star) {
  __shared__ CfgJoinLds sa, sb;
  const int64_t b = blockIdx.y;
  float st = 1.0f;
  if (use_zero_star) {
    st = cfg_star_scale(ws_star, b, sa, sb);
    if (DRIFT) __syncthreads();   // the drift join below writes the same LDS words
  }
  const int64_t base = b * n;
  float num = 0.f, den = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * CFG_THREADS + threadIdx.x; i < n; i += (int64_t)CFG_PARTS * CFG_THREADS) {
    const int64_t at = base + i;
    const float c = cond[at];
    const float v = cfg_guided(c, uncond[at], st, guidance, use_zero_star);
    const float e = v - c;
    if (DRIFT) {
      const float o = delta[at];
      const float q = e - o;
      const float a = fabsf(q);
      num = num + a;
      const float m = fabsf(o);
      den = den + m;
    }
    delta[at] = e;
  }
  if (DRIFT) {
    cfg_pair_join(num, den, sa, sb);
    if (threadIdx.x == 0) {
      float* o = ws_drift + (b * CFG_PARTS + blockIdx.x) * 2;
      o[0] = num;
      o[1] = den;
    }
  }
}

// one workgroup per sample: out[b][0..1] = the 256 drift partial pairs, added as every join here adds
__global__ __launch_bounds__(CFG_THREADS) void cgr_drift_join_kernel(const float* __restrict__ ws_drift, float* __restrict__ out) {
  __shared__ CfgJoinLds sa, sb;
  const int64_t b = blockIdx.x;
  const float* o = ws_drift + (b * CFG_PARTS + threadIdx.x) * 2;
  float num = o[0], den = o[1];
  cfg_pair_join(num, den, sa, sb);
  if (threadIdx.x == 0) {
    out[b * 2 + 0] = num;
    out[b * 2 + 1] = den;
  }
}

__global__ __launch_bounds__(CFG_THREADS) void cgr_apply_kernel(const float* cond, const float* __restrict__ delta, float* v,
                                                                int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * CFG_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * CFG_THREADS) {
    const float c = cond[i];
    v[i] = c + delta[i];
  }
}

extern "C" int lcv_cfg_delta_store(const float* cond, const float* uncond, float* delta, float* ws, float* out, int64_t B,
                                   int64_t n, float guidance, int use_zero_star, void* stream) {
  LCV_CHECK_ARG(cond && uncond && delta, "cfg_delta_store: cond, uncond or delta is a null pointer");
  LCV_CHECK_ARG(delta != cond && delta != uncond, "cfg_delta_store: delta must be a buffer of its own");
  LCV_CHECK_ARG(!(use_zero_star || out) || ws, "cfg_delta_store: zero-star and the drift sums need the workspace");
  LCV_CHECK_ARG(B >= 0 && n >= 0 && B <= 65535, "cfg_delta_store: B must be in 0..65535 and n >= 0, got %ld and %ld", (long)B,
                (long)n);
  if (B == 0 || n == 0) return LCV_OK;
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid(CFG_PARTS, (unsigned)B), block(CFG_THREADS);   // always CFG_PARTS workgroups per sample: every slot is written
  const float* ws_star = ws;
  float* ws_drift = ws ? ws + B * CFG_PARTS * 2 : nullptr;
  if (use_zero_star) {
    hipLaunchKernelGGL(cgr_dot_kernel, grid, block, 0, s, cond, uncond, ws, n);
    LCV_LAUNCH_CHECK("cfg_delta_store: sums");
  }
  if (!out) {
    hipLaunchKernelGGL(cgr_store_kernel<false>, grid, block, 0, s, cond, uncond, delta, ws_star, (float*)nullptr, n, guidance,
                       use_zero_star);
    LCV_LAUNCH_CHECK("cfg_delta_store");
    return LCV_OK;
  }
  hipLaunchKernelGGL(cgr_store_kernel<true>, grid, block, 0, s, cond, uncond, delta, ws_star, ws_drift, n, guidance, use_zero_star);
  LCV_LAUNCH_CHECK("cfg_delta_store");
  hipLaunchKernelGGL(cgr_drift_join_kernel, dim3((unsigned)B), block, 0, s, (const float*)ws_drift, out);
  LCV_LAUNCH_CHECK("cfg_delta_store: join");
  return LCV_OK;
}

extern "C" int lcv_cfg_delta_apply(const float* cond, const float* delta, float* v, int64_t B, int64_t n, void* stream) {
  LCV_CHECK_ARG(cond && delta && v, "cfg_delta_apply: cond, delta or v is a null pointer");
  LCV_CHECK_ARG(v != delta, "cfg_delta_apply: v must not be delta (v may be cond)");
  LCV_CHECK_ARG(B >= 0 && n >= 0, "cfg_delta_apply: B and n must be >= 0, got %ld and %ld", (long)B, (long)n);
  if (B == 0 || n == 0) return LCV_OK;
  const int64_t total = B * n;
  int64_t bx = (total + CFG_THREADS - 1) / CFG_THREADS;
  if (bx > CGR_MAX_BLOCKS) bx = CGR_MAX_BLOCKS;
  hipLaunchKernelGGL(cgr_apply_kernel, dim3((unsigned)bx), dim3(CFG_THREADS), 0, (hipStream_t)stream, cond, delta, v, total);
  LCV_LAUNCH_CHECK("cfg_delta_apply");
  return LCV_OK;
}

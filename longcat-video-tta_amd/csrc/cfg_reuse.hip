// Guidance reuse of the CFG denoise loop (include/lcv_hip_cfgreuse.h): a full step stores the correction delta = v - c of the
// guided output over the prompt row's, a reuse step adds it back to a prompt-only output.  HBM-bound fp32 streaming, one scalar
// path for every element (pointers are only 4-byte aligned, n is arbitrary).  Built with -ffp-contract=off: every operation
// below is one rounded fp32 operation, written one per statement.  The zero-star sums and the drift sums are fixed-order, in the
// two-level scheme of lms_dot_kernel / lms_step_kernel (solver_step.hip), restated here so that file stays as it is; LDS holds
// the wave-order join only.  No atomics.
#include "lcv_common.h"   // wave_sum, the argument and launch checks
#include "lcv_hip_cfgreuse.h"

#pragma clang fp contract(off)

static constexpr int CGR_PARTS = 256;     // workgroups (= partial pairs) per sample of either pair of sums
static constexpr int CGR_THREADS = 256;   // one thread per partial in the joins: must equal CGR_PARTS
static constexpr int CGR_MAX_BLOCKS = 1024;
static_assert(CGR_PARTS == CGR_THREADS && CGR_THREADS == 4 * LCV_WAVE, "the joins hold one partial per thread, four waves");

// the workgroup's sum of one value pair per thread: butterfly inside a wave, the four waves in wave order; every thread gets it
__device__ __forceinline__ void cgr_join(float& a, float& b, float (&sa)[CGR_THREADS / LCV_WAVE], float (&sb)[CGR_THREADS / LCV_WAVE]) {
  a = wave_sum(a);
  b = wave_sum(b);
  if ((threadIdx.x & (LCV_WAVE - 1)) == 0) { sa[threadIdx.x / LCV_WAVE] = a; sb[threadIdx.x / LCV_WAVE] = b; }
  __syncthreads();
  a = ((sa[0] + sa[1]) + sa[2]) + sa[3];
  b = ((sb[0] + sb[1]) + sb[2]) + sb[3];
}

// ws[b][part][2] = the (dot, nrm) of the elements part * 256 + t + k * 65536 of sample b; every slot is written
__global__ __launch_bounds__(CGR_THREADS) void cgr_dot_kernel(const float* __restrict__ cond, const float* __restrict__ uncond,
                                                              float* __restrict__ ws, int64_t n) {
  __shared__ float sd[CGR_THREADS / LCV_WAVE], sn[CGR_THREADS / LCV_WAVE];
  const int64_t b = blockIdx.y;
  const float* c = cond + b * n;
  const float* u = uncond + b * n;
  float dot = 0.f, nrm = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * CGR_THREADS + threadIdx.x; i < n; i += (int64_t)CGR_PARTS * CGR_THREADS) {
    const float cv = c[i], uv = u[i];
    const float p = cv * uv;
    dot = dot + p;
    const float q = uv * uv;
    nrm = nrm + q;
  }
  cgr_join(dot, nrm, sd, sn);
  if (threadIdx.x == 0) {
    float* o = ws + (b * CGR_PARTS + blockIdx.x) * 2;
    o[0] = dot;
    o[1] = nrm;
  }
}

// DRIFT: the old delta is read before it is overwritten and (num, den) of part blockIdx.x goes to ws_drift[b][part][2].
// Always CGR_PARTS workgroups per sample, so the slices are those of cgr_dot_kernel.
template <bool DRIFT>
__global__ __launch_bounds__(CGR_THREADS) void cgr_store_kernel(const float* __restrict__ cond, const float* __restrict__ uncond,
                                                                float* delta, const float* __restrict__ ws_star,
                                                                float* __restrict__ ws_drift, int64_t n, float guidance,
                                                                int use_zero_star) {
  __shared__ float sa[CGR_THREADS / LCV_WAVE], sb[CGR_THREADS / LCV_WAVE];
  const int64_t b = blockIdx.y;
  float st = 1.0f;
  if (use_zero_star) {   // every workgroup adds the 256 partial pairs in the same order (2 KiB from L2)
    const float* o = ws_star + (b * CGR_PARTS + threadIdx.x) * 2;
    float dot = o[0], nrm = o[1];
    cgr_join(dot, nrm, sa, sb);
    const float den = nrm + 1e-8f;
    st = dot / den;
    if (DRIFT) __syncthreads();   // the drift join below writes the same LDS words
  }
  const int64_t base = b * n;
  float num = 0.f, den = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * CGR_THREADS + threadIdx.x; i < n; i += (int64_t)CGR_PARTS * CGR_THREADS) {
    const int64_t at = base + i;
    const float c = cond[at];
    float u = uncond[at];
    if (use_zero_star) u = u * st;
    const float d = c - u;
    const float t = guidance * d;
    const float v = u + t;
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
    cgr_join(num, den, sa, sb);
    if (threadIdx.x == 0) {
      float* o = ws_drift + (b * CGR_PARTS + blockIdx.x) * 2;
      o[0] = num;
      o[1] = den;
    }
  }
}

// one workgroup per sample: out[b][0..1] = the 256 drift partial pairs, added as every join here adds
__global__ __launch_bounds__(CGR_THREADS) void cgr_drift_join_kernel(const float* __restrict__ ws_drift, float* __restrict__ out) {
  __shared__ float sa[CGR_THREADS / LCV_WAVE], sb[CGR_THREADS / LCV_WAVE];
  const int64_t b = blockIdx.x;
  const float* o = ws_drift + (b * CGR_PARTS + threadIdx.x) * 2;
  float num = o[0], den = o[1];
  cgr_join(num, den, sa, sb);
  if (threadIdx.x == 0) {
    out[b * 2 + 0] = num;
    out[b * 2 + 1] = den;
  }
}

__global__ __launch_bounds__(CGR_THREADS) void cgr_apply_kernel(const float* cond, const float* __restrict__ delta, float* v,
                                                                int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * CGR_THREADS + threadIdx.x; i < total; i += (int64_t)gridDim.x * CGR_THREADS) {
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
  const dim3 grid(CGR_PARTS, (unsigned)B), block(CGR_THREADS);   // always CGR_PARTS workgroups per sample: every slot is written
  const float* ws_star = ws;
  float* ws_drift = ws ? ws + B * CGR_PARTS * 2 : nullptr;
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
  int64_t bx = (total + CGR_THREADS - 1) / CGR_THREADS;
  if (bx > CGR_MAX_BLOCKS) bx = CGR_MAX_BLOCKS;
  hipLaunchKernelGGL(cgr_apply_kernel, dim3((unsigned)bx), dim3(CGR_THREADS), 0, (hipStream_t)stream, cond, delta, v, total);
  LCV_LAUNCH_CHECK("cfg_delta_apply");
  return LCV_OK;
}

// fp32 master weights for bf16 parameters (include/lcv_hip_master.h): every bf16 element h carries an int16 low word l in a
// second tensor, join(h, l) is an fp32 number, and the optimizer steps run on that number with no bf16 rounding in between.
// Same descriptor table, chunking (optim_common.h) and 16-byte packet / scalar-tail split as optim.hip.  HBM-bound streaming
// kernels: SGD 6 B read + 4 B written per parameter (4 + 2 for the rounding form), AdamW 14 + 12.
#include "master_elem.h"   // join, split, AdamW's scalars and per-element op sequence (shared with optim_moments8.hip)

__device__ __forceinline__ float master_sgd_elem(float w, float g, float coef, float lr, float wd) {
  g = g * coef;
  if (wd != 0.f) {
    const float d = wd * w;
    g = g + d;
  }
  const float u = -lr * g;
  return w + u;
}

__global__ __launch_bounds__(256) void master_sgd_kernel(const lcv_adam_tensor* __restrict__ tensors, void* const* __restrict__ low,
                                                         int n, const float* __restrict__ clip, float lr, float wd) {
  const int ti = find_tensor(tensors, n, blockIdx.x);
  const lcv_adam_tensor t = tensors[ti];
  const int64_t base = ((int64_t)blockIdx.x - t.first_chunk) * CHUNK + threadIdx.x * 8;
  const float coef = clip ? clip[1] : 1.0f;
  bf16_t* P = (bf16_t*)t.param;
  short* L = (short*)low[ti];
  const bf16_t* G = (const bf16_t*)t.grad;
  if (base + 8 <= t.numel && ((((uintptr_t)P) | ((uintptr_t)G) | ((uintptr_t)L)) & 15) == 0) {   // whole 16-byte packets
    u16x8 hv = *reinterpret_cast<const u16x8*>(P + base);
    s16x8 lv = *reinterpret_cast<const s16x8*>(L + base);
    const u16x8 gv = *reinterpret_cast<const u16x8*>(G + base);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float w = master_sgd_elem(master_join(hv[e], lv[e]), bf2f(gv[e]), coef, lr, wd);
      bf16_t h; short l;
      master_split(w, h, l);
      hv[e] = h; lv[e] = l;
    }
    *reinterpret_cast<u16x8*>(P + base) = hv;
    *reinterpret_cast<s16x8*>(L + base) = lv;
    return;
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int64_t i = base + e;
    if (i >= t.numel) break;
    const float w = master_sgd_elem(master_join(P[i], L[i]), bf2f(G[i]), coef, lr, wd);
    master_split(w, P[i], L[i]);
  }
}

__global__ __launch_bounds__(256) void master_adamw_kernel(const lcv_adam_tensor* __restrict__ tensors, void* const* __restrict__ low,
                                                           int n, const float* __restrict__ clip, const MasterAdamScalars s) {
  const int ti = find_tensor(tensors, n, blockIdx.x);
  const lcv_adam_tensor t = tensors[ti];
  const int64_t base = ((int64_t)blockIdx.x - t.first_chunk) * CHUNK + threadIdx.x * 8;
  const float coef = clip ? clip[1] : 1.0f;
  bf16_t* P = (bf16_t*)t.param;
  short* L = (short*)low[ti];
  const bf16_t* G = (const bf16_t*)t.grad;
  float* M = (float*)t.exp_avg;
  float* V = (float*)t.exp_avg_sq;
  if (base + 8 <= t.numel &&
      ((((uintptr_t)P) | ((uintptr_t)G) | ((uintptr_t)L) | ((uintptr_t)M) | ((uintptr_t)V)) & 15) == 0) {   // whole 16-byte packets
    u16x8 hv = *reinterpret_cast<const u16x8*>(P + base);
    s16x8 lv = *reinterpret_cast<const s16x8*>(L + base);
    const u16x8 gv = *reinterpret_cast<const u16x8*>(G + base);
    f32x4 mv[2], vv[2];
    mv[0] = *reinterpret_cast<const f32x4*>(M + base); mv[1] = *reinterpret_cast<const f32x4*>(M + base + 4);
    vv[0] = *reinterpret_cast<const f32x4*>(V + base); vv[1] = *reinterpret_cast<const f32x4*>(V + base + 4);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float p = master_join(hv[e], lv[e]), m = mv[e >> 2][e & 3], v = vv[e >> 2][e & 3];
      master_adamw_elem(p, m, v, bf2f(gv[e]), coef, s);
      bf16_t h; short l;
      master_split(p, h, l);
      hv[e] = h; lv[e] = l; mv[e >> 2][e & 3] = m; vv[e >> 2][e & 3] = v;
    }
    *reinterpret_cast<u16x8*>(P + base) = hv;
    *reinterpret_cast<s16x8*>(L + base) = lv;
    *reinterpret_cast<f32x4*>(M + base) = mv[0]; *reinterpret_cast<f32x4*>(M + base + 4) = mv[1];
    *reinterpret_cast<f32x4*>(V + base) = vv[0]; *reinterpret_cast<f32x4*>(V + base + 4) = vv[1];
    return;
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int64_t i = base + e;
    if (i >= t.numel) break;
    float p = master_join(P[i], L[i]), m = M[i], v = V[i];
    master_adamw_elem(p, m, v, bf2f(G[i]), coef, s);
    master_split(p, P[i], L[i]);
    M[i] = m; V[i] = v;
  }
}

// SPLIT: master -> (hi, low); otherwise (hi, low) -> master.  One workgroup per CHUNK elements.
template <bool SPLIT>
__global__ __launch_bounds__(256) void master_convert_kernel(float* __restrict__ master, bf16_t* __restrict__ hi,
                                                             short* __restrict__ low, int64_t n) {
  const int64_t base = (int64_t)blockIdx.x * CHUNK + threadIdx.x * 8;
  if (base + 8 <= n && ((((uintptr_t)master) | ((uintptr_t)hi) | ((uintptr_t)low)) & 15) == 0) {   // whole 16-byte packets
    if (SPLIT) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(master + base), b = *reinterpret_cast<const f32x4*>(master + base + 4);
      u16x8 hv; s16x8 lv;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        bf16_t h; short l;
        master_split(e < 4 ? a[e & 3] : b[e & 3], h, l);
        hv[e] = h; lv[e] = l;
      }
      *reinterpret_cast<u16x8*>(hi + base) = hv;
      *reinterpret_cast<s16x8*>(low + base) = lv;
    } else {
      const u16x8 hv = *reinterpret_cast<const u16x8*>(hi + base);
      const s16x8 lv = *reinterpret_cast<const s16x8*>(low + base);
      f32x4 a, b;
#pragma unroll
      for (int e = 0; e < 4; ++e) { a[e] = master_join(hv[e], lv[e]); b[e] = master_join(hv[e + 4], lv[e + 4]); }
      *reinterpret_cast<f32x4*>(master + base) = a;
      *reinterpret_cast<f32x4*>(master + base + 4) = b;
    }
    return;
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int64_t i = base + e;
    if (i >= n) break;
    if (SPLIT) master_split(master[i], hi[i], low[i]);
    else master[i] = master_join(hi[i], low[i]);
  }
}

extern "C" int lcv_master_sgd_step(const lcv_adam_tensor* tensors, void* const* low, int64_t n_tensors, int64_t total_chunks,
                                   const float* norm_coef, double lr, double weight_decay, void* stream) {
  LCV_CHECK_ARG(tensors && low && n_tensors > 0 && n_tensors <= 0x7fffffff && total_chunks > 0 && total_chunks <= 0x7fffffff,
                "master_sgd_step: bad arguments");
  hipLaunchKernelGGL(master_sgd_kernel, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)stream, tensors, low,
                     (int)n_tensors, norm_coef, (float)lr, (float)weight_decay);
  LCV_LAUNCH_CHECK("master_sgd_step");
  return LCV_OK;
}

extern "C" int lcv_master_adamw_step(const lcv_adam_tensor* tensors, void* const* low, int64_t n_tensors, int64_t total_chunks,
                                     const float* norm_coef, double lr, double beta1, double beta2, double eps,
                                     double weight_decay, int64_t step, void* stream) {
  LCV_CHECK_ARG(tensors && low && n_tensors > 0 && n_tensors <= 0x7fffffff && total_chunks > 0 && total_chunks <= 0x7fffffff &&
                    step >= 1, "master_adamw_step: bad arguments");
  const MasterAdamScalars sc = master_adam_scalars(lr, beta1, beta2, eps, weight_decay, step);
  hipLaunchKernelGGL(master_adamw_kernel, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)stream, tensors, low,
                     (int)n_tensors, norm_coef, sc);
  LCV_LAUNCH_CHECK("master_adamw_step");
  return LCV_OK;
}

static bool master_convert_grid(int64_t n, unsigned& blocks) {
  if (n < 1) return false;
  const int64_t b = (n + CHUNK - 1) / CHUNK;
  if (b > 0x7fffffff) return false;
  blocks = (unsigned)b;
  return true;
}

extern "C" int lcv_master_split(const float* master, void* hi_bf16, void* low, int64_t n, void* stream) {
  unsigned blocks = 0;
  LCV_CHECK_ARG(master && hi_bf16 && low && master_convert_grid(n, blocks), "master_split: bad arguments");
  hipLaunchKernelGGL(master_convert_kernel<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (float*)master,
                     (bf16_t*)hi_bf16, (short*)low, n);
  LCV_LAUNCH_CHECK("master_split");
  return LCV_OK;
}

extern "C" int lcv_master_join(const void* hi_bf16, const void* low, float* master, int64_t n, void* stream) {
  unsigned blocks = 0;
  LCV_CHECK_ARG(master && hi_bf16 && low && master_convert_grid(n, blocks), "master_join: bad arguments");
  hipLaunchKernelGGL(master_convert_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, master, (bf16_t*)hi_bf16,
                     (short*)low, n);
  LCV_LAUNCH_CHECK("master_join");
  return LCV_OK;
}

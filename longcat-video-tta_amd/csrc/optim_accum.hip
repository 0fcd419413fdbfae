// fp32 gradient accumulation over micro-steps (include/lcv_hip_accum.h): every parameter element carries an fp32 accumulator,
// each micro-step's bf16 gradient is scaled and added into it, and the master-weight steps read it as the gradient.
// Same descriptor table, chunking (optim_common.h) and 16-byte packet / scalar-tail split as optim_master.hip; the format and
// AdamW's op sequence are that file's (master_elem.h).  HBM-bound streaming kernels: accumulate 6 B read + 4 B written per
// element, SGD 8 + 4, AdamW 16 + 12.  Built with -ffp-contract=off: a product never fuses with the sum that takes it.
#include "master_elem.h"   // join, split, AdamW's scalars and per-element op sequence
#include "lcv_hip_accum.h"

// t = float(g) * s;  a = a + t  - always the add, so 0 + t carries IEEE addition's sign of zero
__device__ __forceinline__ float accum_elem(float a, float g, float s) {
  const float t = g * s;
  return a + t;
}

// the op order of master_sgd_elem (optim_master.hip)
__device__ __forceinline__ float accum_sgd_elem(float w, float g, float coef, float lr, float wd) {
  g = g * coef;
  if (wd != 0.f) {
    const float d = wd * w;
    g = g + d;
  }
  const float u = -lr * g;
  return w + u;
}

__global__ __launch_bounds__(256) void grad_accumulate_kernel(const lcv_adam_tensor* __restrict__ tensors,
                                                              void* const* __restrict__ acc, int n, float s) {
  const int ti = find_tensor(tensors, n, blockIdx.x);
  const lcv_adam_tensor t = tensors[ti];
  const int64_t base = ((int64_t)blockIdx.x - t.first_chunk) * CHUNK + threadIdx.x * 8;
  const bf16_t* G = (const bf16_t*)t.grad;
  float* A = (float*)acc[ti];
  if (base + 8 <= t.numel && ((((uintptr_t)G) | ((uintptr_t)A)) & 15) == 0) {   // whole 16-byte packets
    const u16x8 gv = *reinterpret_cast<const u16x8*>(G + base);
    f32x4 av[2];
    av[0] = *reinterpret_cast<const f32x4*>(A + base); av[1] = *reinterpret_cast<const f32x4*>(A + base + 4);
#pragma unroll
    for (int e = 0; e < 8; ++e) av[e >> 2][e & 3] = accum_elem(av[e >> 2][e & 3], bf2f(gv[e]), s);
    *reinterpret_cast<f32x4*>(A + base) = av[0]; *reinterpret_cast<f32x4*>(A + base + 4) = av[1];
    return;
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int64_t i = base + e;
    if (i >= t.numel) break;
    A[i] = accum_elem(A[i], bf2f(G[i]), s);
  }
}

__global__ __launch_bounds__(256) void master_sgd_g32_kernel(const lcv_adam_tensor* __restrict__ tensors,
                                                             void* const* __restrict__ low, int n,
                                                             const float* __restrict__ clip, float lr, float wd) {
  const int ti = find_tensor(tensors, n, blockIdx.x);
  const lcv_adam_tensor t = tensors[ti];
  const int64_t base = ((int64_t)blockIdx.x - t.first_chunk) * CHUNK + threadIdx.x * 8;
  const float coef = clip ? clip[1] : 1.0f;
  bf16_t* P = (bf16_t*)t.param;
  short* L = (short*)low[ti];
  const float* G = (const float*)t.grad;
  if (base + 8 <= t.numel && ((((uintptr_t)P) | ((uintptr_t)G) | ((uintptr_t)L)) & 15) == 0) {   // whole 16-byte packets
    u16x8 hv = *reinterpret_cast<const u16x8*>(P + base);
    s16x8 lv = *reinterpret_cast<const s16x8*>(L + base);
    f32x4 gv[2];
    gv[0] = *reinterpret_cast<const f32x4*>(G + base); gv[1] = *reinterpret_cast<const f32x4*>(G + base + 4);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float w = accum_sgd_elem(master_join(hv[e], lv[e]), gv[e >> 2][e & 3], coef, lr, wd);
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
    const float w = accum_sgd_elem(master_join(P[i], L[i]), G[i], coef, lr, wd);
    master_split(w, P[i], L[i]);
  }
}

__global__ __launch_bounds__(256) void master_adamw_g32_kernel(const lcv_adam_tensor* __restrict__ tensors,
                                                               void* const* __restrict__ low, int n,
                                                               const float* __restrict__ clip, const MasterAdamScalars s) {
  const int ti = find_tensor(tensors, n, blockIdx.x);
  const lcv_adam_tensor t = tensors[ti];
  const int64_t base = ((int64_t)blockIdx.x - t.first_chunk) * CHUNK + threadIdx.x * 8;
  const float coef = clip ? clip[1] : 1.0f;
  bf16_t* P = (bf16_t*)t.param;
  short* L = (short*)low[ti];
  const float* G = (const float*)t.grad;
  float* M = (float*)t.exp_avg;
  float* V = (float*)t.exp_avg_sq;
  if (base + 8 <= t.numel &&
      ((((uintptr_t)P) | ((uintptr_t)G) | ((uintptr_t)L) | ((uintptr_t)M) | ((uintptr_t)V)) & 15) == 0) {   // whole 16-byte packets
    u16x8 hv = *reinterpret_cast<const u16x8*>(P + base);
    s16x8 lv = *reinterpret_cast<const s16x8*>(L + base);
    f32x4 gv[2], mv[2], vv[2];
    gv[0] = *reinterpret_cast<const f32x4*>(G + base); gv[1] = *reinterpret_cast<const f32x4*>(G + base + 4);
    mv[0] = *reinterpret_cast<const f32x4*>(M + base); mv[1] = *reinterpret_cast<const f32x4*>(M + base + 4);
    vv[0] = *reinterpret_cast<const f32x4*>(V + base); vv[1] = *reinterpret_cast<const f32x4*>(V + base + 4);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float p = master_join(hv[e], lv[e]), m = mv[e >> 2][e & 3], v = vv[e >> 2][e & 3];
      master_adamw_elem(p, m, v, gv[e >> 2][e & 3], coef, s);
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
    master_adamw_elem(p, m, v, G[i], coef, s);
    master_split(p, P[i], L[i]);
    M[i] = m; V[i] = v;
  }
}

extern "C" int lcv_grad_accumulate(const lcv_adam_tensor* tensors, void* const* acc, int64_t n_tensors, int64_t total_chunks,
                                   double scale, void* stream) {
  LCV_CHECK_ARG(tensors && acc && n_tensors > 0 && n_tensors <= 0x7fffffff && total_chunks > 0 && total_chunks <= 0x7fffffff,
                "grad_accumulate: bad arguments");
  hipLaunchKernelGGL(grad_accumulate_kernel, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)stream, tensors, acc,
                     (int)n_tensors, (float)scale);
  LCV_LAUNCH_CHECK("grad_accumulate");
  return LCV_OK;
}

extern "C" int lcv_master_sgd_step_g32(const lcv_adam_tensor* tensors, void* const* low, int64_t n_tensors, int64_t total_chunks,
                                       const float* norm_coef, double lr, double weight_decay, void* stream) {
  LCV_CHECK_ARG(tensors && low && n_tensors > 0 && n_tensors <= 0x7fffffff && total_chunks > 0 && total_chunks <= 0x7fffffff,
                "master_sgd_step_g32: bad arguments");
  hipLaunchKernelGGL(master_sgd_g32_kernel, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)stream, tensors, low,
                     (int)n_tensors, norm_coef, (float)lr, (float)weight_decay);
  LCV_LAUNCH_CHECK("master_sgd_step_g32");
  return LCV_OK;
}

extern "C" int lcv_master_adamw_step_g32(const lcv_adam_tensor* tensors, void* const* low, int64_t n_tensors,
                                         int64_t total_chunks, const float* norm_coef, double lr, double beta1, double beta2,
                                         double eps, double weight_decay, int64_t step, void* stream) {
  LCV_CHECK_ARG(tensors && low && n_tensors > 0 && n_tensors <= 0x7fffffff && total_chunks > 0 && total_chunks <= 0x7fffffff &&
                    step >= 1, "master_adamw_step_g32: bad arguments");
  const MasterAdamScalars sc = master_adam_scalars(lr, beta1, beta2, eps, weight_decay, step);
  hipLaunchKernelGGL(master_adamw_g32_kernel, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)stream, tensors, low,
                     (int)n_tensors, norm_coef, sc);
  LCV_LAUNCH_CHECK("master_adamw_step_g32");
  return LCV_OK;
}

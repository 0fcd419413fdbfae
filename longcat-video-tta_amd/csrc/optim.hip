// Fused multi-tensor gradient-norm clip + AdamW for the TTA inner loop: one launch over every adapter tensor
// (240 adapters = 480 tensors at qkv+proj) instead of torch's ~10 foreach launches.
//
// The reference trains bf16 adapters with torch.optim.AdamW(foreach) after torch.nn.utils.clip_grad_norm_
// (lora_experiment/scripts/run_lora_tta.py:462-468, 513-514), i.e. every intermediate of the update is ROUNDED
// TO bf16.  The kernel reproduces that op sequence and its rounding points exactly (tests/optim_ref.py restates it in numpy and
// tests/test_gpu_optim_kernel_edges.py pins it bit for bit):
//   g  = bf16(g * coef)                                   clip_grad_norm_   (coef is a bf16 value)
//   p  = bf16(p * (1 - lr*wd))                            _foreach_mul_
//   m  = bf16(m + (1-b1) * (g - m))                       _foreach_lerp_    (weight < 0.5 form)
//   v  = bf16(v * b2);  v = bf16(v + ((1-b2) * g) * g)    _foreach_mul_, _foreach_addcmul_
//   d  = bf16(sqrt(v)); d = bf16(d / sqrt(1-b2^t)); d = bf16(d + eps)
//   p  = bf16(p + (-lr/(1-b1^t)) * (m / d))               _foreach_addcdiv_
// For fp32 parameters (the delta methods) the same sequence runs without the bf16 roundings: master_adamw_elem (master_elem.h),
// the one definition the master-weight kernels use too.
// Every fp32 operation is one correctly rounded IEEE operation: plain operators, `/` and __builtin_sqrtf, and the file is built
// with -ffp-contract=off (lcv_hip/build.py; master_elem.h's pragma says the same), so no product fuses with the sum that takes
// it.  (hipcc's __fmul_rn / __fadd_rn are plain operators that contract under its default, and its __fsqrt_rn is the 1-ulp
// native square root: they are not used.)  The clip's sums of squares (grad_chunk_sumsq's packet path) keep their explicit fmaf.
// Algorithmic bytes: 14 B / parameter (bf16: p, g, m, v read; p, m, v written).
#include "master_elem.h"
#include <math.h>

template <bool F32>
__global__ __launch_bounds__(256) void grad_sumsq_kernel(const lcv_adam_tensor* __restrict__ tensors, int n,
                                                         float* __restrict__ per_tensor) {
  const int ti = find_tensor(tensors, n, blockIdx.x);
  const lcv_adam_tensor t = tensors[ti];
  const int64_t chunk = (int64_t)blockIdx.x - t.first_chunk;
  const float sumsq = grad_chunk_sumsq<F32>(t, chunk);
  if (threadIdx.x == 0) atomicAdd(per_tensor + (int64_t)ti * NORM_SLOTS + (chunk % NORM_SLOTS), sumsq);
}

// total norm exactly as clip_grad_norm_ composes it: per-tensor norms (rounded to the grad dtype), then the
// norm of those; out[0] = total norm, out[1] = clip coefficient min(max_norm / (total + 1e-6), 1).
template <bool F32>
__global__ __launch_bounds__(256) void clip_coef_kernel(const float* __restrict__ per_tensor, int n, float max_norm,
                                                        float* __restrict__ out) {
  __shared__ float part[4];
  float acc = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) {
    float sumsq = 0.f;
    for (int k = 0; k < NORM_SLOTS; ++k) sumsq += per_tensor[(int64_t)i * NORM_SLOTS + k];
    float nrm = sqrtf(sumsq);
    if (!F32) nrm = bfround(nrm);
    acc += nrm * nrm;
  }
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float total = sqrtf(part[0] + part[1] + part[2] + part[3]);
    float coef;
    if (F32) {
      coef = max_norm / (total + 1e-6f);
    } else {
      total = bfround(total);
      coef = bfround(max_norm / bfround(total + 1e-6f));
    }
    out[0] = total;
    out[1] = fminf(coef, 1.0f);
  }
}

void clip_coef_launch(const float* per_tensor, int n, float max_norm, float* out, bool f32, hipStream_t s) {
  if (f32) hipLaunchKernelGGL(clip_coef_kernel<true>, dim3(1), dim3(256), 0, s, per_tensor, n, max_norm, out);
  else hipLaunchKernelGGL(clip_coef_kernel<false>, dim3(1), dim3(256), 0, s, per_tensor, n, max_norm, out);
}

template <bool F32>
__global__ __launch_bounds__(256) void adamw_kernel(const lcv_adam_tensor* __restrict__ tensors, int n,
                                                    const float* __restrict__ clip, const AdamScalars s) {
  const int ti = find_tensor(tensors, n, blockIdx.x);
  const lcv_adam_tensor t = tensors[ti];
  const int64_t base = ((int64_t)blockIdx.x - t.first_chunk) * CHUNK + threadIdx.x * 8;
  const float coef = clip ? clip[1] : 1.0f;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int64_t i = base + e;
    if (i >= t.numel) break;
    if (F32) {
      float* P = (float*)t.param; float* M = (float*)t.exp_avg; float* V = (float*)t.exp_avg_sq;
      float p = P[i], m = M[i], v = V[i];
      master_adamw_elem(p, m, v, ((const float*)t.grad)[i], coef, s);
      P[i] = p; M[i] = m; V[i] = v;
    } else {
      bf16_t* P = (bf16_t*)t.param; bf16_t* M = (bf16_t*)t.exp_avg; bf16_t* V = (bf16_t*)t.exp_avg_sq;
      const float g = bfround(bf2f(((const bf16_t*)t.grad)[i]) * coef);
      float p = bfround(bf2f(P[i]) * s.c_wd);
      float m = bf2f(M[i]);
      m = bfround(m + s.w1 * (g - m));
      float v = bfround(bf2f(V[i]) * s.b2);
      v = bfround(v + (s.c2 * g) * g);
      float d = bfround(__builtin_sqrtf(v));
      d = bfround(d / s.bc2_sqrt);
      d = bfround(d + s.eps);
      p = bfround(p + s.step_size * (m / d));
      P[i] = f2bf(p); M[i] = f2bf(m); V[i] = f2bf(v);
    }
  }
}

extern "C" int lcv_grad_norm_clip(const lcv_adam_tensor* tensors, int64_t n_tensors, int64_t total_chunks,
                                  int param_f32, float max_norm, float* per_tensor_ws, float* norm_coef_out,
                                  void* stream) {
  LCV_CHECK_ARG(tensors && per_tensor_ws && norm_coef_out && n_tensors > 0 && total_chunks > 0, "grad_norm_clip: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(per_tensor_ws, 0, sizeof(float) * n_tensors * NORM_SLOTS, s) != hipSuccess) {
    lcv_set_error("grad_norm_clip: memset failed");
    return LCV_EDEVICE;
  }
  if (param_f32)
    hipLaunchKernelGGL(grad_sumsq_kernel<true>, dim3((unsigned)total_chunks), dim3(256), 0, s, tensors, (int)n_tensors, per_tensor_ws);
  else
    hipLaunchKernelGGL(grad_sumsq_kernel<false>, dim3((unsigned)total_chunks), dim3(256), 0, s, tensors, (int)n_tensors, per_tensor_ws);
  LCV_LAUNCH_CHECK("grad_sumsq");
  clip_coef_launch(per_tensor_ws, (int)n_tensors, max_norm, norm_coef_out, param_f32 != 0, s);
  LCV_LAUNCH_CHECK("clip_coef");
  return LCV_OK;
}

extern "C" int lcv_adamw_step(const lcv_adam_tensor* tensors, int64_t n_tensors, int64_t total_chunks, int param_f32,
                              const float* norm_coef, double lr, double beta1, double beta2, double eps,
                              double weight_decay, int64_t step, void* stream) {
  LCV_CHECK_ARG(tensors && n_tensors > 0 && total_chunks > 0 && step >= 1, "adamw_step: bad arguments");
  const AdamScalars sc = adam_scalars(lr, beta1, beta2, eps, weight_decay, step);
  if (param_f32)
    hipLaunchKernelGGL(adamw_kernel<true>, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)stream, tensors, (int)n_tensors, norm_coef, sc);
  else
    hipLaunchKernelGGL(adamw_kernel<false>, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)stream, tensors, (int)n_tensors, norm_coef, sc);
  LCV_LAUNCH_CHECK("adamw_step");
  return LCV_OK;
}

// ---------------------------------------------------------------------------
// SGD (momentum 0) with weight decay, the default optimizer of full-model TTA
// (lora_experiment/scripts/run_full_tta.py:138-144: SGD(params, lr, momentum=0.0, weight_decay)), in the op order
// and bf16 rounding points of torch.optim.SGD's foreach path after clip_grad_norm_:
//   g = bf16(g * coef);  g = bf16(g + wd * p) if wd != 0;  p = bf16(p + (-lr) * g)
// with -lr in fp32, as torch's device kernels hold alpha.  fp32 parameters: the same without the roundings, and the decay always
// added (wd = 0 adds a zero; master_sgd_elem skips it, which differs only where g * coef is -0 or p is not finite).  The 16-byte
// packet path and the per-element path are one arithmetic.  Every operation correctly rounded, nothing fused (see the top).
// Same descriptor table as AdamW (exp_avg / exp_avg_sq unused).  8 B / parameter read, 2 written.
// ---------------------------------------------------------------------------
template <bool F32>
__global__ __launch_bounds__(256) void sgd_kernel(const lcv_adam_tensor* __restrict__ tensors, int n,
                                                  const float* __restrict__ clip, float lr, float wd) {
  const int ti = find_tensor(tensors, n, blockIdx.x);
  const lcv_adam_tensor t = tensors[ti];
  const int64_t base = ((int64_t)blockIdx.x - t.first_chunk) * CHUNK + threadIdx.x * 8;
  const float coef = clip ? clip[1] : 1.0f;
  if (!F32 && base + 8 <= t.numel && ((((uintptr_t)t.param) | ((uintptr_t)t.grad)) & 15) == 0) {   // whole 16-byte packets
    float p[8], g[8];
    bf16_t* P = (bf16_t*)t.param + base;
    unpack8(*reinterpret_cast<const u16x8*>(P), p);
    unpack8(*reinterpret_cast<const u16x8*>((const bf16_t*)t.grad + base), g);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float gg = bfround(g[e] * coef);
      if (wd != 0.f) gg = bfround(gg + wd * p[e]);
      p[e] = p[e] + (-lr) * gg;
    }
    *reinterpret_cast<u16x8*>(P) = pack8(p);
    return;
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int64_t i = base + e;
    if (i >= t.numel) break;
    if (F32) {
      float* P = (float*)t.param;
      float g = ((const float*)t.grad)[i] * coef;
      g = g + wd * P[i];
      P[i] = P[i] + (-lr) * g;
    } else {
      bf16_t* P = (bf16_t*)t.param;
      const float p = bf2f(P[i]);
      float g = bfround(bf2f(((const bf16_t*)t.grad)[i]) * coef);
      if (wd != 0.f) g = bfround(g + wd * p);
      P[i] = f2bf(p + (-lr) * g);
    }
  }
}

extern "C" int lcv_sgd_step(const lcv_adam_tensor* tensors, int64_t n_tensors, int64_t total_chunks, int param_f32,
                            const float* norm_coef, double lr, double weight_decay, void* stream) {
  LCV_CHECK_ARG(tensors && n_tensors > 0 && total_chunks > 0 && total_chunks <= 0x7fffffff, "sgd_step: bad arguments");
  if (param_f32)
    hipLaunchKernelGGL(sgd_kernel<true>, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)stream, tensors, (int)n_tensors,
                       norm_coef, (float)lr, (float)weight_decay);
  else
    hipLaunchKernelGGL(sgd_kernel<false>, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)stream, tensors, (int)n_tensors,
                       norm_coef, (float)lr, (float)weight_decay);
  LCV_LAUNCH_CHECK("sgd_step");
  return LCV_OK;
}

// fp32 master weights for bf16 parameters (include/lcv_hip_master.h): every bf16 element h carries an int16 low word l in a
// second tensor, join(h, l) is an fp32 number, and the optimizer steps run on that number with no bf16 rounding in between.
// One step kernel per optimizer serves every form of it: the gradient is bf16 or an fp32 accumulator
// (include/lcv_hip_accum.h), and the decay pulls toward zero or toward a bf16 base word (include/lcv_hip_anchor.h).
// Same descriptor table, chunking (optim_common.h) and 16-byte packet / scalar-tail split as optim.hip.  HBM-bound streaming
// kernels, per parameter: SGD 6 B read + 4 B written, AdamW 14 + 12; an fp32 gradient and a base word add 2 B read each.
// Built with -ffp-contract=off.  Every output has one writer; no LDS.
#include "master_elem.h"   // join, split, a thread's 8 floats, the per-element op sequences (shared with optim_moments8.hip)
#include "lcv_hip_master.h"
#include "lcv_hip_accum.h"
#include "lcv_hip_anchor.h"

// G32: the gradient's element type, one element widened, and a thread's 8 gradients from one bf16 packet or two fp32 packets
template <bool G32> struct grad { typedef bf16_t type; };
template <> struct grad<true> { typedef float type; };
__device__ __forceinline__ float widen(bf16_t g) { return bf2f(g); }
__device__ __forceinline__ float widen(float g) { return g; }
__device__ __forceinline__ void load_grads(const bf16_t* G, float (&g)[8]) { unpack8(*reinterpret_cast<const u16x8*>(G), g); }
__device__ __forceinline__ void load_grads(const float* G, float (&g)[8]) { load8(G, g); }

// ANCHOR: the decay is wd * (w - w0) with w0 = float(anchor word); without it `anchor` is not read
template <bool G32, bool ANCHOR>
__global__ __launch_bounds__(256) void master_sgd_kernel(const lcv_adam_tensor* __restrict__ tensors, void* const* __restrict__ low,
                                                         int n, const float* __restrict__ clip, float lr, float wd,
                                                         void* const* __restrict__ anchor) {
  typedef typename grad<G32>::type grad_t;
  const int ti = find_tensor(tensors, n, blockIdx.x);
  const lcv_adam_tensor t = tensors[ti];
  const int64_t base = ((int64_t)blockIdx.x - t.first_chunk) * CHUNK + threadIdx.x * 8;
  const float coef = clip ? clip[1] : 1.0f;
  bf16_t* P = (bf16_t*)t.param;
  short* L = (short*)low[ti];
  const bf16_t* A = ANCHOR ? (const bf16_t*)anchor[ti] : nullptr;
  const grad_t* G = (const grad_t*)t.grad;
  const auto step = [&](float w, float w0, float g) {
    return ANCHOR ? master_sgd_anchor_elem(w, w0, g, coef, lr, wd) : master_sgd_elem(w, g, coef, lr, wd);
  };
  if (base + 8 <= t.numel && ((((uintptr_t)P) | ((uintptr_t)G) | ((uintptr_t)L) | ((uintptr_t)A)) & 15) == 0) {   // whole 16-byte packets
    u16x8 hv = *reinterpret_cast<const u16x8*>(P + base);
    s16x8 lv = *reinterpret_cast<const s16x8*>(L + base);
    u16x8 av = {0, 0, 0, 0, 0, 0, 0, 0};
    if (ANCHOR) av = *reinterpret_cast<const u16x8*>(A + base);
    float g[8];
    load_grads(G + base, g);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float w = step(master_join(hv[e], lv[e]), bf2f(av[e]), g[e]);
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
    const float w = step(master_join(P[i], L[i]), ANCHOR ? bf2f(A[i]) : 0.f, widen(G[i]));
    master_split(w, P[i], L[i]);
  }
}

// ANCHOR: the decay is p = p - a * (p - w0), a = (float)(lr * weight_decay); without it `anchor` and `a` are not read
template <bool G32, bool ANCHOR>
__global__ __launch_bounds__(256) void master_adamw_kernel(const lcv_adam_tensor* __restrict__ tensors, void* const* __restrict__ low,
                                                           int n, const float* __restrict__ clip, const AdamScalars s,
                                                           void* const* __restrict__ anchor, float a) {
  typedef typename grad<G32>::type grad_t;
  const int ti = find_tensor(tensors, n, blockIdx.x);
  const lcv_adam_tensor t = tensors[ti];
  const int64_t base = ((int64_t)blockIdx.x - t.first_chunk) * CHUNK + threadIdx.x * 8;
  const float coef = clip ? clip[1] : 1.0f;
  bf16_t* P = (bf16_t*)t.param;
  short* L = (short*)low[ti];
  const bf16_t* A = ANCHOR ? (const bf16_t*)anchor[ti] : nullptr;
  const grad_t* G = (const grad_t*)t.grad;
  float* M = (float*)t.exp_avg;
  float* V = (float*)t.exp_avg_sq;
  const auto step = [&](float& p, float& m, float& v, float w0, float g) {
    if (ANCHOR) master_adamw_anchor_elem(p, m, v, w0, g, coef, a, s);
    else master_adamw_elem(p, m, v, g, coef, s);
  };
  if (base + 8 <= t.numel && ((((uintptr_t)P) | ((uintptr_t)G) | ((uintptr_t)L) | ((uintptr_t)A) | ((uintptr_t)M) |
                                ((uintptr_t)V)) & 15) == 0) {   // whole 16-byte packets
    u16x8 hv = *reinterpret_cast<const u16x8*>(P + base);
    s16x8 lv = *reinterpret_cast<const s16x8*>(L + base);
    u16x8 av = {0, 0, 0, 0, 0, 0, 0, 0};
    if (ANCHOR) av = *reinterpret_cast<const u16x8*>(A + base);
    float g[8], m[8], v[8];
    load_grads(G + base, g);
    load8(M + base, m);
    load8(V + base, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float p = master_join(hv[e], lv[e]);
      step(p, m[e], v[e], bf2f(av[e]), g[e]);
      bf16_t h; short l;
      master_split(p, h, l);
      hv[e] = h; lv[e] = l;
    }
    *reinterpret_cast<u16x8*>(P + base) = hv;
    *reinterpret_cast<s16x8*>(L + base) = lv;
    store8(M + base, m);
    store8(V + base, v);
    return;
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int64_t i = base + e;
    if (i >= t.numel) break;
    float p = master_join(P[i], L[i]), m = M[i], v = V[i];
    step(p, m, v, ANCHOR ? bf2f(A[i]) : 0.f, widen(G[i]));
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
      float w[8];
      load8(master + base, w);
      u16x8 hv; s16x8 lv;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        bf16_t h; short l;
        master_split(w[e], h, l);
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

// ---- host: one launcher per optimizer; the instantiation follows (grad_f32, anchor != nullptr) ----
static int master_sgd_launch(const char* name, const lcv_adam_tensor* tensors, void* const* low, void* const* anchor,
                             int64_t n_tensors, int64_t total_chunks, const float* norm_coef, double lr, double weight_decay,
                             bool grad_f32, void* stream) {
  const auto kernel = grad_f32 ? (anchor ? master_sgd_kernel<true, true> : master_sgd_kernel<true, false>)
                               : (anchor ? master_sgd_kernel<false, true> : master_sgd_kernel<false, false>);
  hipLaunchKernelGGL(kernel, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)stream, tensors, low, (int)n_tensors,
                     norm_coef, (float)lr, (float)weight_decay, anchor);
  LCV_LAUNCH_CHECK(name);
  return LCV_OK;
}

static int master_adamw_launch(const char* name, const lcv_adam_tensor* tensors, void* const* low, void* const* anchor,
                               int64_t n_tensors, int64_t total_chunks, const float* norm_coef, double lr, double beta1,
                               double beta2, double eps, double weight_decay, int64_t step, bool grad_f32, void* stream) {
  const auto kernel = grad_f32 ? (anchor ? master_adamw_kernel<true, true> : master_adamw_kernel<true, false>)
                               : (anchor ? master_adamw_kernel<false, true> : master_adamw_kernel<false, false>);
  hipLaunchKernelGGL(kernel, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)stream, tensors, low, (int)n_tensors,
                     norm_coef, adam_scalars(lr, beta1, beta2, eps, weight_decay, step), anchor, (float)(lr * weight_decay));
  LCV_LAUNCH_CHECK(name);
  return LCV_OK;
}

extern "C" int lcv_master_sgd_step(const lcv_adam_tensor* tensors, void* const* low, int64_t n_tensors, int64_t total_chunks,
                                   const float* norm_coef, double lr, double weight_decay, void* stream) {
  LCV_CHECK_ARG(tensors && low && optim_table_ok(n_tensors, total_chunks), "master_sgd_step: bad arguments");
  return master_sgd_launch("master_sgd_step", tensors, low, nullptr, n_tensors, total_chunks, norm_coef, lr, weight_decay, false,
                           stream);
}

extern "C" int lcv_master_sgd_step_g32(const lcv_adam_tensor* tensors, void* const* low, int64_t n_tensors, int64_t total_chunks,
                                       const float* norm_coef, double lr, double weight_decay, void* stream) {
  LCV_CHECK_ARG(tensors && low && optim_table_ok(n_tensors, total_chunks), "master_sgd_step_g32: bad arguments");
  return master_sgd_launch("master_sgd_step_g32", tensors, low, nullptr, n_tensors, total_chunks, norm_coef, lr, weight_decay,
                           true, stream);
}

extern "C" int lcv_master_sgd_step_anchor(const lcv_adam_tensor* tensors, void* const* low, void* const* anchor, int64_t n_tensors,
                                          int64_t total_chunks, const float* norm_coef, double lr, double weight_decay,
                                          int grad_f32, void* stream) {
  LCV_CHECK_ARG(tensors && low && anchor && optim_table_ok(n_tensors, total_chunks) && (grad_f32 == 0 || grad_f32 == 1),
                "master_sgd_step_anchor: bad arguments");
  return master_sgd_launch("master_sgd_step_anchor", tensors, low, anchor, n_tensors, total_chunks, norm_coef, lr, weight_decay,
                           grad_f32 != 0, stream);
}

extern "C" int lcv_master_adamw_step(const lcv_adam_tensor* tensors, void* const* low, int64_t n_tensors, int64_t total_chunks,
                                     const float* norm_coef, double lr, double beta1, double beta2, double eps,
                                     double weight_decay, int64_t step, void* stream) {
  LCV_CHECK_ARG(tensors && low && optim_table_ok(n_tensors, total_chunks) && step >= 1, "master_adamw_step: bad arguments");
  return master_adamw_launch("master_adamw_step", tensors, low, nullptr, n_tensors, total_chunks, norm_coef, lr, beta1, beta2, eps,
                             weight_decay, step, false, stream);
}

extern "C" int lcv_master_adamw_step_g32(const lcv_adam_tensor* tensors, void* const* low, int64_t n_tensors,
                                         int64_t total_chunks, const float* norm_coef, double lr, double beta1, double beta2,
                                         double eps, double weight_decay, int64_t step, void* stream) {
  LCV_CHECK_ARG(tensors && low && optim_table_ok(n_tensors, total_chunks) && step >= 1, "master_adamw_step_g32: bad arguments");
  return master_adamw_launch("master_adamw_step_g32", tensors, low, nullptr, n_tensors, total_chunks, norm_coef, lr, beta1, beta2,
                             eps, weight_decay, step, true, stream);
}

extern "C" int lcv_master_adamw_step_anchor(const lcv_adam_tensor* tensors, void* const* low, void* const* anchor,
                                            int64_t n_tensors, int64_t total_chunks, const float* norm_coef, double lr,
                                            double beta1, double beta2, double eps, double weight_decay, int64_t step,
                                            int grad_f32, void* stream) {
  LCV_CHECK_ARG(tensors && low && anchor && optim_table_ok(n_tensors, total_chunks) && step >= 1 &&
                    (grad_f32 == 0 || grad_f32 == 1), "master_adamw_step_anchor: bad arguments");
  return master_adamw_launch("master_adamw_step_anchor", tensors, low, anchor, n_tensors, total_chunks, norm_coef, lr, beta1, beta2,
                             eps, weight_decay, step, grad_f32 != 0, stream);
}

extern "C" int lcv_master_split(const float* master, void* hi_bf16, void* low, int64_t n, void* stream) {
  unsigned blocks = 0;
  LCV_CHECK_ARG(master && hi_bf16 && low && chunk_grid(n, blocks), "master_split: bad arguments");
  hipLaunchKernelGGL(master_convert_kernel<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (float*)master,
                     (bf16_t*)hi_bf16, (short*)low, n);
  LCV_LAUNCH_CHECK("master_split");
  return LCV_OK;
}

extern "C" int lcv_master_join(const void* hi_bf16, const void* low, float* master, int64_t n, void* stream) {
  unsigned blocks = 0;
  LCV_CHECK_ARG(master && hi_bf16 && low && chunk_grid(n, blocks), "master_join: bad arguments");
  hipLaunchKernelGGL(master_convert_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, master, (bf16_t*)hi_bf16,
                     (short*)low, n);
  LCV_LAUNCH_CHECK("master_join");
  return LCV_OK;
}

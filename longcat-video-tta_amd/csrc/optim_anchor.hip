// Decay toward the base weights, and the drift from them (include/lcv_hip_anchor.h): the master-weight steps with the decay
// term taken on w - w0, where w0 = float(h0) is the bf16 base word of the element, and the sum of squares of w - w0.
// Same descriptor table, chunking (optim_common.h) and 16-byte packet / scalar-tail split as optim_master.hip and
// optim_accum.hip; the format, AdamW's scalars and the op sequences are master_elem.h's, the 8-bit codec moments8_codec.h's.
// HBM-bound streaming kernels, per parameter: SGD 8 B read + 4 B written (10 + 4 with an fp32 gradient), AdamW 16 + 12
// (18 + 12), 8-bit AdamW 10 + 6, drift 6 + 0 (4 + 0 without low words).  Built with -ffp-contract=off.  Every output has
// one writer and every sum a fixed order.
#include "moments8_codec.h"   // and through it master_elem.h
#include "lcv_hip_anchor.h"

template <bool G32> struct anchor_grad { typedef bf16_t type; };
template <> struct anchor_grad<true> { typedef float type; };
__device__ __forceinline__ float anchor_widen(bf16_t g) { return bf2f(g); }
__device__ __forceinline__ float anchor_widen(float g) { return g; }

// a thread's 8 gradients: one bf16 packet or two fp32 packets
template <bool G32>
__device__ __forceinline__ void anchor_load_grads(const typename anchor_grad<G32>::type* G, int64_t base, float (&g)[8]) {
  if (G32) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(G + base), b = *reinterpret_cast<const f32x4*>(G + base + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) { g[e] = a[e]; g[e + 4] = b[e]; }
  } else {
    unpack8(*reinterpret_cast<const u16x8*>(G + base), g);
  }
}

template <bool G32>
__global__ __launch_bounds__(256) void master_sgd_anchor_kernel(const lcv_adam_tensor* __restrict__ tensors,
                                                                void* const* __restrict__ low, void* const* __restrict__ anchor,
                                                                int n, const float* __restrict__ clip, float lr, float wd) {
  typedef typename anchor_grad<G32>::type grad_t;
  const int ti = find_tensor(tensors, n, blockIdx.x);
  const lcv_adam_tensor t = tensors[ti];
  const int64_t base = ((int64_t)blockIdx.x - t.first_chunk) * CHUNK + threadIdx.x * 8;
  const float coef = clip ? clip[1] : 1.0f;
  bf16_t* P = (bf16_t*)t.param;
  short* L = (short*)low[ti];
  const bf16_t* A = (const bf16_t*)anchor[ti];
  const grad_t* G = (const grad_t*)t.grad;
  if (base + 8 <= t.numel && ((((uintptr_t)P) | ((uintptr_t)G) | ((uintptr_t)L) | ((uintptr_t)A)) & 15) == 0) {   // whole 16-byte packets
    u16x8 hv = *reinterpret_cast<const u16x8*>(P + base);
    s16x8 lv = *reinterpret_cast<const s16x8*>(L + base);
    const u16x8 av = *reinterpret_cast<const u16x8*>(A + base);
    float g[8];
    anchor_load_grads<G32>(G, base, g);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float w = master_sgd_anchor_elem(master_join(hv[e], lv[e]), bf2f(av[e]), g[e], coef, lr, wd);
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
    const float w = master_sgd_anchor_elem(master_join(P[i], L[i]), bf2f(A[i]), anchor_widen(G[i]), coef, lr, wd);
    master_split(w, P[i], L[i]);
  }
}

template <bool G32>
__global__ __launch_bounds__(256) void master_adamw_anchor_kernel(const lcv_adam_tensor* __restrict__ tensors,
                                                                  void* const* __restrict__ low, void* const* __restrict__ anchor,
                                                                  int n, const float* __restrict__ clip, const MasterAdamScalars s,
                                                                  float a) {
  typedef typename anchor_grad<G32>::type grad_t;
  const int ti = find_tensor(tensors, n, blockIdx.x);
  const lcv_adam_tensor t = tensors[ti];
  const int64_t base = ((int64_t)blockIdx.x - t.first_chunk) * CHUNK + threadIdx.x * 8;
  const float coef = clip ? clip[1] : 1.0f;
  bf16_t* P = (bf16_t*)t.param;
  short* L = (short*)low[ti];
  const bf16_t* A = (const bf16_t*)anchor[ti];
  const grad_t* G = (const grad_t*)t.grad;
  float* M = (float*)t.exp_avg;
  float* V = (float*)t.exp_avg_sq;
  if (base + 8 <= t.numel && ((((uintptr_t)P) | ((uintptr_t)G) | ((uintptr_t)L) | ((uintptr_t)A) | ((uintptr_t)M) |
                                ((uintptr_t)V)) & 15) == 0) {   // whole 16-byte packets
    u16x8 hv = *reinterpret_cast<const u16x8*>(P + base);
    s16x8 lv = *reinterpret_cast<const s16x8*>(L + base);
    const u16x8 av = *reinterpret_cast<const u16x8*>(A + base);
    float g[8];
    anchor_load_grads<G32>(G, base, g);
    f32x4 mv[2], vv[2];
    mv[0] = *reinterpret_cast<const f32x4*>(M + base); mv[1] = *reinterpret_cast<const f32x4*>(M + base + 4);
    vv[0] = *reinterpret_cast<const f32x4*>(V + base); vv[1] = *reinterpret_cast<const f32x4*>(V + base + 4);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float p = master_join(hv[e], lv[e]), m = mv[e >> 2][e & 3], v = vv[e >> 2][e & 3];
      master_adamw_anchor_elem(p, m, v, bf2f(av[e]), g[e], coef, a, s);
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
    master_adamw_anchor_elem(p, m, v, bf2f(A[i]), anchor_widen(G[i]), coef, a, s);
    master_split(p, P[i], L[i]);
    M[i] = m; V[i] = v;
  }
}

// master_adamw8_kernel (optim_moments8.hip) with the anchor's decay: a wave owns a 512-element block of codes
__global__ __launch_bounds__(256) void master_adamw8_anchor_kernel(const lcv_adam_tensor* __restrict__ tensors,
                                                                   void* const* __restrict__ low, void* const* __restrict__ scales,
                                                                   void* const* __restrict__ anchor, int n,
                                                                   const float* __restrict__ clip, const MasterAdamScalars s, float a) {
  const int ti = find_tensor(tensors, n, blockIdx.x);
  const lcv_adam_tensor t = tensors[ti];
  const int64_t chunk0 = ((int64_t)blockIdx.x - t.first_chunk) * CHUNK;
  const int64_t wave0 = chunk0 + (int64_t)(threadIdx.x & ~(LCV_WAVE - 1)) * 8;      // where this wave's block starts
  if (wave0 >= t.numel) return;                                                     // the whole wave: no such block
  const int64_t base = chunk0 + threadIdx.x * 8;
  const int64_t nblocks = (t.numel + M8_BLOCK - 1) / M8_BLOCK, blk = wave0 / M8_BLOCK;
  const float coef = clip ? clip[1] : 1.0f;
  bf16_t* P = (bf16_t*)t.param;
  short* L = (short*)low[ti];
  const bf16_t* A = (const bf16_t*)anchor[ti];
  const bf16_t* G = (const bf16_t*)t.grad;
  u8_t* CM = (u8_t*)t.exp_avg;
  u8_t* CR = (u8_t*)t.exp_avg_sq;
  float* S = (float*)scales[ti];
  const float sm0 = S[blk], sr0 = S[nblocks + blk];
  const int nvalid = m8_nvalid(base, t.numel);
  // whole packets: 16 bytes of h, l, h0 and g, 8 bytes of each code
  const bool packet = nvalid == 8 && ((((uintptr_t)P) | ((uintptr_t)G) | ((uintptr_t)L) | ((uintptr_t)A)) & 15) == 0 &&
                      ((((uintptr_t)CM) | ((uintptr_t)CR)) & 7) == 0;
  u16x8 hv, gv, av;
  s16x8 lv;
  unsigned int cm[8], cr[8];
  if (packet) {
    hv = *reinterpret_cast<const u16x8*>(P + base);
    lv = *reinterpret_cast<const s16x8*>(L + base);
    gv = *reinterpret_cast<const u16x8*>(G + base);
    av = *reinterpret_cast<const u16x8*>(A + base);
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const bool in = e < nvalid;
      hv[e] = in ? P[base + e] : (bf16_t)0;
      lv[e] = in ? L[base + e] : (short)0;
      gv[e] = in ? G[base + e] : (bf16_t)0;
      av[e] = in ? A[base + e] : (bf16_t)0;
    }
  }
  m8_load_codes(CM, base, packet, nvalid, cm);
  m8_load_codes(CR, base, packet, nvalid, cr);
  float m[8], r[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    m[e] = 0.f; r[e] = 0.f;
    if (e < nvalid) {
      float p = master_join(hv[e], lv[e]), v = m8_decode_v(cr[e], sr0);
      m[e] = m8_decode_m(cm[e], sm0);
      master_adamw_anchor_elem(p, m[e], v, bf2f(av[e]), bf2f(gv[e]), coef, a, s);
      bf16_t h; short l;
      master_split(p, h, l);
      hv[e] = h; lv[e] = l;
      r[e] = __builtin_sqrtf(v);                                // the root the step took
    }
  }
  if (packet) {
    *reinterpret_cast<u16x8*>(P + base) = hv;
    *reinterpret_cast<s16x8*>(L + base) = lv;
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e)
      if (e < nvalid) { P[base + e] = hv[e]; L[base + e] = lv[e]; }
  }
  m8_encode_store(m, r, CM, CR, S, nblocks, blk, base, packet, nvalid);
}

// ---- drift: sum over all elements of (join(h, l) - float(h0))^2, in a fixed order ----
// a = a + d * d, the product rounded before the sum
__device__ __forceinline__ float drift_elem(float acc, float w, float w0) {
  const float d = w - w0;
  const float q = d * d;
  return acc + q;
}

// one fp32 partial per chunk: a thread's 8 elements in index order, the wave's butterfly, then the four waves in wave order
__global__ __launch_bounds__(256) void drift_chunk_kernel(const lcv_adam_tensor* __restrict__ tensors, void* const* __restrict__ low,
                                                          void* const* __restrict__ anchor, int n, float* __restrict__ partials) {
  const int ti = find_tensor(tensors, n, blockIdx.x);
  const lcv_adam_tensor t = tensors[ti];
  const int64_t base = ((int64_t)blockIdx.x - t.first_chunk) * CHUNK + threadIdx.x * 8;
  const bf16_t* P = (const bf16_t*)t.param;
  const short* L = low ? (const short*)low[ti] : nullptr;       // no low words: every one of them is zero
  const bf16_t* A = (const bf16_t*)anchor[ti];
  float acc = 0.f;
  if (base + 8 <= t.numel && ((((uintptr_t)P) | ((uintptr_t)L) | ((uintptr_t)A)) & 15) == 0) {   // whole 16-byte packets
    const u16x8 hv = *reinterpret_cast<const u16x8*>(P + base);
    const u16x8 av = *reinterpret_cast<const u16x8*>(A + base);
    s16x8 lv = {0, 0, 0, 0, 0, 0, 0, 0};
    if (L) lv = *reinterpret_cast<const s16x8*>(L + base);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc = drift_elem(acc, master_join(hv[e], lv[e]), bf2f(av[e]));
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int64_t i = base + e;
      if (i < t.numel) acc = drift_elem(acc, master_join(P[i], L ? L[i] : (short)0), bf2f(A[i]));
    }
  }
  __shared__ float part[4];
  acc = wave_sum(acc);
  if ((threadIdx.x & (LCV_WAVE - 1)) == 0) part[threadIdx.x / LCV_WAVE] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = ((part[0] + part[1]) + part[2]) + part[3];
}

// one workgroup: thread t adds partials t, t + 1024, ... in index order, the wave's butterfly, then the waves in wave order
static constexpr int DRIFT_FINAL_THREADS = 1024;
__global__ __launch_bounds__(DRIFT_FINAL_THREADS) void drift_final_kernel(const float* __restrict__ partials, int total,
                                                                          float* __restrict__ out) {
  float acc = 0.f;
#pragma unroll 8
  for (int c = threadIdx.x; c < total; c += DRIFT_FINAL_THREADS) acc = acc + partials[c];
  __shared__ float part[DRIFT_FINAL_THREADS / LCV_WAVE];
  acc = wave_sum(acc);
  if ((threadIdx.x & (LCV_WAVE - 1)) == 0) part[threadIdx.x / LCV_WAVE] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    float s = part[0];
    for (int w = 1; w < DRIFT_FINAL_THREADS / LCV_WAVE; ++w) s = s + part[w];
    out[0] = s;
    out[1] = __builtin_sqrtf(s);
  }
}

static bool anchor_table_ok(const void* tensors, const void* a, const void* b, int64_t n_tensors, int64_t total_chunks) {
  return tensors && a && b && n_tensors > 0 && n_tensors <= 0x7fffffff && total_chunks > 0 && total_chunks <= 0x7fffffff;
}

extern "C" int lcv_master_sgd_step_anchor(const lcv_adam_tensor* tensors, void* const* low, void* const* anchor, int64_t n_tensors,
                                          int64_t total_chunks, const float* norm_coef, double lr, double weight_decay,
                                          int grad_f32, void* stream) {
  LCV_CHECK_ARG(anchor_table_ok(tensors, low, anchor, n_tensors, total_chunks) && (grad_f32 == 0 || grad_f32 == 1),
                "master_sgd_step_anchor: bad arguments");
  const dim3 grid((unsigned)total_chunks), block(256);
  if (grad_f32)
    hipLaunchKernelGGL(master_sgd_anchor_kernel<true>, grid, block, 0, (hipStream_t)stream, tensors, low, anchor, (int)n_tensors,
                       norm_coef, (float)lr, (float)weight_decay);
  else
    hipLaunchKernelGGL(master_sgd_anchor_kernel<false>, grid, block, 0, (hipStream_t)stream, tensors, low, anchor, (int)n_tensors,
                       norm_coef, (float)lr, (float)weight_decay);
  LCV_LAUNCH_CHECK("master_sgd_step_anchor");
  return LCV_OK;
}

extern "C" int lcv_master_adamw_step_anchor(const lcv_adam_tensor* tensors, void* const* low, void* const* anchor,
                                            int64_t n_tensors, int64_t total_chunks, const float* norm_coef, double lr,
                                            double beta1, double beta2, double eps, double weight_decay, int64_t step,
                                            int grad_f32, void* stream) {
  LCV_CHECK_ARG(anchor_table_ok(tensors, low, anchor, n_tensors, total_chunks) && step >= 1 && (grad_f32 == 0 || grad_f32 == 1),
                "master_adamw_step_anchor: bad arguments");
  const MasterAdamScalars sc = master_adam_scalars(lr, beta1, beta2, eps, weight_decay, step);
  const float a = (float)(lr * weight_decay);
  const dim3 grid((unsigned)total_chunks), block(256);
  if (grad_f32)
    hipLaunchKernelGGL(master_adamw_anchor_kernel<true>, grid, block, 0, (hipStream_t)stream, tensors, low, anchor,
                       (int)n_tensors, norm_coef, sc, a);
  else
    hipLaunchKernelGGL(master_adamw_anchor_kernel<false>, grid, block, 0, (hipStream_t)stream, tensors, low, anchor,
                       (int)n_tensors, norm_coef, sc, a);
  LCV_LAUNCH_CHECK("master_adamw_step_anchor");
  return LCV_OK;
}

extern "C" int lcv_master_adamw8_step_anchor(const lcv_adam_tensor* tensors, void* const* low, void* const* scales,
                                             void* const* anchor, int64_t n_tensors, int64_t total_chunks, const float* norm_coef,
                                             double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step,
                                             void* stream) {
  LCV_CHECK_ARG(anchor_table_ok(tensors, low, anchor, n_tensors, total_chunks) && scales && step >= 1,
                "master_adamw8_step_anchor: bad arguments");
  const MasterAdamScalars sc = master_adam_scalars(lr, beta1, beta2, eps, weight_decay, step);
  hipLaunchKernelGGL(master_adamw8_anchor_kernel, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)stream, tensors, low,
                     scales, anchor, (int)n_tensors, norm_coef, sc, (float)(lr * weight_decay));
  LCV_LAUNCH_CHECK("master_adamw8_step_anchor");
  return LCV_OK;
}

extern "C" int lcv_master_drift_sumsq(const lcv_adam_tensor* tensors, void* const* low, void* const* anchor, int64_t n_tensors,
                                      int64_t total_chunks, float* partials, int64_t partials_bytes, float* out, void* stream) {
  LCV_CHECK_ARG(anchor_table_ok(tensors, anchor, out, n_tensors, total_chunks), "master_drift_sumsq: bad arguments");
  LCV_CHECK_ARG(partials && partials_bytes >= total_chunks * 4 && ((uintptr_t)partials % 4) == 0,
                "master_drift_sumsq: workspace of %ld bytes is missing or too small (need %ld)", (long)partials_bytes,
                (long)(total_chunks * 4));
  hipLaunchKernelGGL(drift_chunk_kernel, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)stream, tensors, low, anchor,
                     (int)n_tensors, partials);
  LCV_LAUNCH_CHECK("master_drift_sumsq: chunks");
  hipLaunchKernelGGL(drift_final_kernel, dim3(1), dim3(DRIFT_FINAL_THREADS), 0, (hipStream_t)stream, partials, (int)total_chunks,
                     out);
  LCV_LAUNCH_CHECK("master_drift_sumsq: total");
  return LCV_OK;
}

// 8-bit block-scaled AdamW moments for master weights (include/lcv_hip_moments8.h): one byte per moment per parameter plus one
// fp32 scale per moment per 512 parameters, the second moment stored as its root.  Same descriptor table, chunking and
// thread-to-element mapping as optim_master.hip: a thread owns 8 consecutive elements (one 16-byte bf16 packet), so a wave
// owns 512 = one block, and a workgroup's CHUNK is four blocks.  The block maxima are a wave_max over registers, and a max
// does not depend on the order it is taken in; every output has one writer.  HBM-bound: 8 B read + 6 B written per
// parameter, 2 B more read with the decay toward a base word (include/lcv_hip_anchor.h).
#include "master_elem.h"   // join, split and AdamW's per-element op sequences; contraction off from there on
#include "moments8_codec.h"   // the codes, a thread's packets of them, a wave's block maxima
#include "lcv_hip_anchor.h"

// ANCHOR: the decay is p = p - a * (p - w0), a = (float)(lr * weight_decay); without it `anchor` and `a` are not read
template <bool ANCHOR>
__global__ __launch_bounds__(256) void master_adamw8_kernel(const lcv_adam_tensor* __restrict__ tensors, void* const* __restrict__ low,
                                                            void* const* __restrict__ scales, int n, const float* __restrict__ clip,
                                                            const AdamScalars s, void* const* __restrict__ anchor, float a) {
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
  const bf16_t* A = ANCHOR ? (const bf16_t*)anchor[ti] : nullptr;
  const bf16_t* G = (const bf16_t*)t.grad;
  u8_t* CM = (u8_t*)t.exp_avg;
  u8_t* CR = (u8_t*)t.exp_avg_sq;
  float* S = (float*)scales[ti];
  const float sm0 = S[blk], sr0 = S[nblocks + blk];
  const int nvalid = m8_nvalid(base, t.numel);
  // whole packets: 16 bytes of h, l, g (and h0), 8 bytes of each code
  const bool packet = nvalid == 8 && ((((uintptr_t)P) | ((uintptr_t)G) | ((uintptr_t)L) | ((uintptr_t)A)) & 15) == 0 &&
                      ((((uintptr_t)CM) | ((uintptr_t)CR)) & 7) == 0;
  u16x8 hv, gv, av = {0, 0, 0, 0, 0, 0, 0, 0};
  s16x8 lv;
  unsigned int cm[8], cr[8];
  if (packet) {
    hv = *reinterpret_cast<const u16x8*>(P + base);
    lv = *reinterpret_cast<const s16x8*>(L + base);
    gv = *reinterpret_cast<const u16x8*>(G + base);
    if (ANCHOR) av = *reinterpret_cast<const u16x8*>(A + base);
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const bool in = e < nvalid;
      hv[e] = in ? P[base + e] : (bf16_t)0;
      lv[e] = in ? L[base + e] : (short)0;
      gv[e] = in ? G[base + e] : (bf16_t)0;
      if (ANCHOR) av[e] = in ? A[base + e] : (bf16_t)0;
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
      // the update uses the fp32 moments, before they are quantised
      if (ANCHOR) master_adamw_anchor_elem(p, m[e], v, bf2f(av[e]), bf2f(gv[e]), coef, a, s);
      else master_adamw_elem(p, m[e], v, bf2f(gv[e]), coef, s);
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

// one tensor, fp32 moments -> codes and scales.  One workgroup per CHUNK elements.
__global__ __launch_bounds__(256) void moments8_encode_kernel(const float* __restrict__ M, const float* __restrict__ V, u8_t* __restrict__ CM,
                                                              u8_t* __restrict__ CR, float* __restrict__ S, int64_t n) {
  const int64_t chunk0 = (int64_t)blockIdx.x * CHUNK;
  const int64_t wave0 = chunk0 + (int64_t)(threadIdx.x & ~(LCV_WAVE - 1)) * 8;
  if (wave0 >= n) return;
  const int64_t base = chunk0 + threadIdx.x * 8;
  const int nvalid = m8_nvalid(base, n);
  const bool packet = nvalid == 8 && ((((uintptr_t)M) | ((uintptr_t)V)) & 15) == 0 && ((((uintptr_t)CM) | ((uintptr_t)CR)) & 7) == 0;
  float m[8], r[8];
  if (packet) {
    const f32x4 m0 = *reinterpret_cast<const f32x4*>(M + base), m1 = *reinterpret_cast<const f32x4*>(M + base + 4);
    const f32x4 v0 = *reinterpret_cast<const f32x4*>(V + base), v1 = *reinterpret_cast<const f32x4*>(V + base + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      m[e] = m0[e]; m[e + 4] = m1[e];
      r[e] = __builtin_sqrtf(v0[e]); r[e + 4] = __builtin_sqrtf(v1[e]);
    }
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      m[e] = e < nvalid ? M[base + e] : 0.f;
      r[e] = e < nvalid ? __builtin_sqrtf(V[base + e]) : 0.f;
    }
  }
  m8_encode_store(m, r, CM, CR, S, (n + M8_BLOCK - 1) / M8_BLOCK, wave0 / M8_BLOCK, base, packet, nvalid);
}

__global__ __launch_bounds__(256) void moments8_decode_kernel(const u8_t* __restrict__ CM, const u8_t* __restrict__ CR,
                                                              const float* __restrict__ S, float* __restrict__ M, float* __restrict__ V,
                                                              int64_t n) {
  const int64_t base = (int64_t)blockIdx.x * CHUNK + threadIdx.x * 8;
  const int nvalid = m8_nvalid(base, n);
  if (nvalid == 0) return;
  const int64_t nblocks = (n + M8_BLOCK - 1) / M8_BLOCK, blk = base / M8_BLOCK;
  const float sm = S[blk], sr = S[nblocks + blk];
  const bool packet = nvalid == 8 && ((((uintptr_t)M) | ((uintptr_t)V)) & 15) == 0 && ((((uintptr_t)CM) | ((uintptr_t)CR)) & 7) == 0;
  unsigned int cm[8], cr[8];
  m8_load_codes(CM, base, packet, nvalid, cm);
  m8_load_codes(CR, base, packet, nvalid, cr);
  if (packet) {
    f32x4 m0, m1, v0, v1;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      m0[e] = m8_decode_m(cm[e], sm); m1[e] = m8_decode_m(cm[e + 4], sm);
      v0[e] = m8_decode_v(cr[e], sr); v1[e] = m8_decode_v(cr[e + 4], sr);
    }
    *reinterpret_cast<f32x4*>(M + base) = m0; *reinterpret_cast<f32x4*>(M + base + 4) = m1;
    *reinterpret_cast<f32x4*>(V + base) = v0; *reinterpret_cast<f32x4*>(V + base + 4) = v1;
    return;
  }
#pragma unroll
  for (int e = 0; e < 8; ++e)
    if (e < nvalid) {
      M[base + e] = m8_decode_m(cm[e], sm);
      V[base + e] = m8_decode_v(cr[e], sr);
    }
}

extern "C" int lcv_master_adamw8_step(const lcv_adam_tensor* tensors, void* const* low, void* const* scales, int64_t n_tensors,
                                      int64_t total_chunks, const float* norm_coef, double lr, double beta1, double beta2,
                                      double eps, double weight_decay, int64_t step, void* stream) {
  LCV_CHECK_ARG(tensors && low && scales && optim_table_ok(n_tensors, total_chunks) && step >= 1,
                "master_adamw8_step: bad arguments");
  hipLaunchKernelGGL(master_adamw8_kernel<false>, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)stream, tensors, low,
                     scales, (int)n_tensors, norm_coef, adam_scalars(lr, beta1, beta2, eps, weight_decay, step), nullptr, 0.f);
  LCV_LAUNCH_CHECK("master_adamw8_step");
  return LCV_OK;
}

extern "C" int lcv_master_adamw8_step_anchor(const lcv_adam_tensor* tensors, void* const* low, void* const* scales,
                                             void* const* anchor, int64_t n_tensors, int64_t total_chunks, const float* norm_coef,
                                             double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step,
                                             void* stream) {
  LCV_CHECK_ARG(tensors && low && anchor && scales && optim_table_ok(n_tensors, total_chunks) && step >= 1,
                "master_adamw8_step_anchor: bad arguments");
  hipLaunchKernelGGL(master_adamw8_kernel<true>, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)stream, tensors, low,
                     scales, (int)n_tensors, norm_coef, adam_scalars(lr, beta1, beta2, eps, weight_decay, step), anchor,
                     (float)(lr * weight_decay));
  LCV_LAUNCH_CHECK("master_adamw8_step_anchor");
  return LCV_OK;
}

extern "C" int lcv_moments8_encode(const float* m_f32, const float* v_f32, void* cm, void* cr, float* scales, int64_t n,
                                   void* stream) {
  unsigned blocks = 0;
  LCV_CHECK_ARG(m_f32 && v_f32 && cm && cr && scales && chunk_grid(n, blocks), "moments8_encode: bad arguments");
  hipLaunchKernelGGL(moments8_encode_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, m_f32, v_f32, (u8_t*)cm, (u8_t*)cr,
                     scales, n);
  LCV_LAUNCH_CHECK("moments8_encode");
  return LCV_OK;
}

extern "C" int lcv_moments8_decode(const void* cm, const void* cr, const float* scales, float* m_f32, float* v_f32, int64_t n,
                                   void* stream) {
  unsigned blocks = 0;
  LCV_CHECK_ARG(m_f32 && v_f32 && cm && cr && scales && chunk_grid(n, blocks), "moments8_decode: bad arguments");
  hipLaunchKernelGGL(moments8_decode_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, (const u8_t*)cm, (const u8_t*)cr,
                     scales, m_f32, v_f32, n);
  LCV_LAUNCH_CHECK("moments8_decode");
  return LCV_OK;
}

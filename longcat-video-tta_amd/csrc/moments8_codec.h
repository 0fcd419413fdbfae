// The 8-bit block-scaled moment codec (include/lcv_hip_moments8.h) of the kernels that keep AdamW moments in it
// (optim_moments8.hip): codes, a thread's 8-code packets, a wave's block maxima and scales.
#pragma once
#include "master_elem.h"   // contraction off from there on
#include "lcv_hip_moments8.h"

typedef unsigned char u8_t;
static constexpr int M8_BLOCK = LCV_MOMENTS8_BLOCK;
static_assert(M8_BLOCK == LCV_WAVE * 8 && CHUNK == 4 * M8_BLOCK, "one block per wave, four per chunk");

// ---- the codes ----
// round to 3 mantissa bits, ties away from zero, the carry runs into the exponent: sign(0) | exponent(8) | mantissa(3)
__device__ __forceinline__ unsigned int m8_k(float z) { return (__builtin_bit_cast(unsigned int, z) + 0x80000u) >> 20; }

__device__ __forceinline__ unsigned int m8_encode_m(float m, float sm) {
  const float x = sm == 0.f ? 0.f : __builtin_fabsf(m) / sm;
  const unsigned int k = m8_k(x);
  if (x == 0.f || k < 890u) return 0u;                                   // flushed to +0: no sign
  const unsigned int mag = k - 889u < 127u ? k - 889u : 127u;
  return mag | ((__builtin_bit_cast(unsigned int, m) >> 31) << 7);
}
__device__ __forceinline__ unsigned int m8_encode_r(float r, float sr) {
  const float y = sr == 0.f ? 0.f : r / sr;
  if (y == 0.f) return 0u;
  const int c = (int)m8_k(y) - 761;
  return (unsigned int)(c < 1 ? 1 : (c > 255 ? 255 : c));                // clamped up, never flushed
}
__device__ __forceinline__ float m8_decode_m(unsigned int c, float sm) {
  const unsigned int mag = c & 127u;
  const float x = mag ? __builtin_bit_cast(float, (mag + 889u) << 20) : 0.f;
  const float a = x * sm;
  return (c & 128u) ? -a : a;
}
__device__ __forceinline__ float m8_decode_v(unsigned int c, float sr) {
  const float y = c ? __builtin_bit_cast(float, (c + 761u) << 20) : 0.f;
  const float r = y * sr;
  return r * r;
}

// ---- a thread's 8 codes: one 8-byte packet, or byte by byte for the first nvalid ----
__device__ __forceinline__ void m8_load_codes(const u8_t* C, int64_t base, bool packet, int nvalid, unsigned int (&c)[8]) {
  if (packet) {
    const u32x2 w = *reinterpret_cast<const u32x2*>(C + base);
#pragma unroll
    for (int e = 0; e < 8; ++e) c[e] = (w[e >> 2] >> (8 * (e & 3))) & 255u;
    return;
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) c[e] = e < nvalid ? C[base + e] : 0u;
}
__device__ __forceinline__ void m8_store_codes(u8_t* C, int64_t base, bool packet, int nvalid, const unsigned int (&c)[8]) {
  if (packet) {
    u32x2 w;
    w[0] = c[0] | (c[1] << 8) | (c[2] << 16) | (c[3] << 24);
    w[1] = c[4] | (c[5] << 8) | (c[6] << 16) | (c[7] << 24);
    *reinterpret_cast<u32x2*>(C + base) = w;
    return;
  }
#pragma unroll
  for (int e = 0; e < 8; ++e)
    if (e < nvalid) C[base + e] = (u8_t)c[e];
}

// Encode a thread's 8 fresh moments (missing elements are m = r = 0: they add 0 to the maxima and store nothing) and store
// codes and scales.  Every lane of the wave that owns block `blk` calls this; the scales go out from lane 0.
__device__ __forceinline__ void m8_encode_store(const float (&m)[8], const float (&r)[8], u8_t* CM, u8_t* CR, float* S,
                                                int64_t nblocks, int64_t blk, int64_t base, bool packet, int nvalid) {
  float am = 0.f, ar = 0.f;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    am = fmaxf(am, __builtin_fabsf(m[e]));
    ar = fmaxf(ar, r[e]);
  }
  const float sm = wave_max(am), sr = wave_max(ar);
  unsigned int cm[8], cr[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    cm[e] = m8_encode_m(m[e], sm);
    cr[e] = m8_encode_r(r[e], sr);
  }
  m8_store_codes(CM, base, packet, nvalid, cm);
  m8_store_codes(CR, base, packet, nvalid, cr);
  if ((threadIdx.x & (LCV_WAVE - 1)) == 0) {
    S[blk] = sm;
    S[nblocks + blk] = sr;
  }
}

// elements of this thread that exist: 8, fewer in a tensor's last packet, 0 past it
__device__ __forceinline__ int m8_nvalid(int64_t base, int64_t numel) {
  const int64_t left = numel - base;
  return left >= 8 ? 8 : (left > 0 ? (int)left : 0);
}

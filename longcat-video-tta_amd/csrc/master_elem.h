// What the master-weight optimizer kernels share (optim_master.hip, optim_moments8.hip, optim_accum.hip, optim_anchor.hip,
// optim_ema.hip, optim_trust.hip), and the default kernels' fp32 AdamW (optim.hip):
// the (bf16 word, int16 low word) <-> fp32 master format, a thread's eight fp32 values, and the per-element op sequences of SGD
// and AdamW (their scalars are optim_common.h's).  All of them are built with -ffp-contract=off.
#pragma once
#include "optim_common.h"

typedef __attribute__((ext_vector_type(8))) short s16x8;

// Every fp32 operation below is one correctly rounded IEEE operation and stays one: contraction is off for the including file,
// and the arithmetic is written with plain operators.  (hipcc's __fmul_rn / __fadd_rn are `x * y` / `x + y` compiled under the
// default -ffp-contract=fast, so a product and the sum that takes it may still fuse into one fma; its __fsqrt_rn is the
// 1-ulp native square root.  `/` and __builtin_sqrtf are the correctly rounded forms, hipcc's default for fp32.  No optimizer
// kernel uses those intrinsics: optim.hip is written and built the same way.)
#pragma clang fp contract(off)

__device__ __forceinline__ float master_join(bf16_t h, short l) {
  return __builtin_bit_cast(float, ((unsigned int)h << 16) + (unsigned int)(int)l);
}
// h: round to nearest bf16, ties away from zero; l: what is left, in [-32768, 32767].  Integer arithmetic mod 2^32.
__device__ __forceinline__ void master_split(float w, bf16_t& h, short& l) {
  const unsigned int m = __builtin_bit_cast(unsigned int, w);
  const unsigned int hh = (m + 0x8000u) >> 16;
  h = (bf16_t)hh;
  l = (short)(unsigned short)(m - (hh << 16));
}

// a thread's 8 consecutive fp32 values (a moment, a gradient, an average): two 16-byte packets
__device__ __forceinline__ void load8(const float* p, float (&v)[8]) {
  const f32x4 a = *reinterpret_cast<const f32x4*>(p), b = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
  for (int e = 0; e < 4; ++e) { v[e] = a[e]; v[e + 4] = b[e]; }
}
__device__ __forceinline__ void store8(float* p, const float (&v)[8]) {
  f32x4 a, b;
#pragma unroll
  for (int e = 0; e < 4; ++e) { a[e] = v[e]; b[e] = v[e + 4]; }
  *reinterpret_cast<f32x4*>(p) = a;
  *reinterpret_cast<f32x4*>(p + 4) = b;
}

// SGD (momentum 0): g is scaled by the clip coefficient, takes the decay, and moves w
__device__ __forceinline__ float master_sgd_elem(float w, float g, float coef, float lr, float wd) {
  g = g * coef;
  if (wd != 0.f) {
    const float d = wd * w;
    g = g + d;
  }
  const float u = -lr * g;
  return w + u;
}

// AdamW after the decay: both moments, then the parameter.  g is already scaled by the clip coefficient.
__device__ __forceinline__ void master_adamw_moments_update(float& p, float& m, float& v, float g, const AdamScalars& s) {
  const float dm = s.w1 * (g - m);
  m = m + dm;
  v = v * s.b2;
  const float dv = (s.c2 * g) * g;
  v = v + dv;
  const float d = __builtin_sqrtf(v) / s.bc2_sqrt + s.eps;
  const float dp = s.step_size * (m / d);
  p = p + dp;
}

// the fp32 AdamW op sequence, each operation correctly rounded; p, m, v in and out.  adamw_kernel<true> (optim.hip) is this
// function, and its bf16 form is the same sequence with a bf16 rounding after each operation of its header's list
__device__ __forceinline__ void master_adamw_elem(float& p, float& m, float& v, float g, float coef, const AdamScalars& s) {
  g = g * coef;
  p = p * s.c_wd;
  master_adamw_moments_update(p, m, v, g, s);
}

// ---- decay toward a base weight w0 instead of toward zero (include/lcv_hip_anchor.h) ----
// master_sgd_elem with wd * (w - w0) in place of wd * w
__device__ __forceinline__ float master_sgd_anchor_elem(float w, float w0, float g, float coef, float lr, float wd) {
  g = g * coef;
  if (wd != 0.f) {
    const float d = w - w0;
    const float t = wd * d;
    g = g + t;
  }
  const float u = -lr * g;
  return w + u;
}

// master_adamw_elem with p = p - a * (p - w0) in place of p = p * c_wd; a = (float)(lr * weight_decay).  Always taken: a = 0
// subtracts a zero.
__device__ __forceinline__ void master_adamw_anchor_elem(float& p, float& m, float& v, float w0, float g, float coef, float a,
                                                         const AdamScalars& s) {
  g = g * coef;
  const float d = p - w0;
  const float t = a * d;
  p = p - t;
  master_adamw_moments_update(p, m, v, g, s);
}

// ---- the fp32 average of the masters over the steps (include/lcv_hip_ema.h) ----
// e = beta * e + (1 - beta) * w in the form w - b * (w - e): b = 0 gives w and w = e gives e back, both exactly
__device__ __forceinline__ float master_ema_elem(float w, float e, float b) {
  const float d = w - e;
  const float t = b * d;
  return w - t;
}

// ---- the projection onto the ball around the base weights (include/lcv_hip_trust.h) ----
// the drift w - w0 scaled by c and put back on w0: c = 1 gives w back up to the rounding of (w - w0) + w0
__device__ __forceinline__ float master_trust_elem(float w, float w0, float c) {
  const float d = w - w0;
  const float u = c * d;
  return w0 + u;
}

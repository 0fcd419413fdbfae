// The CFG-zero-star guidance math of the denoise step, defined once for the files that use it: elementwise.hip (the fused
// Euler step), solver_step.hip (the multistep step), cfg_reuse.hip (the stored correction) and cfg_apg.hip (the projected
// guidance: the sums, st and the joins; its rule for v is its own).
//
//   st = <c, u> / (<u, u> + 1e-8) per sample,   u' = u * st,   v = u' + g * (c - u')
//
// The two sums are fixed-order and two-level: CFG_PARTS workgroups per sample each leave one (dot, nrm) pair in ws[b][part][2],
// and every workgroup of the consuming launch adds the CFG_PARTS pairs again, in the same order (2 KiB from L2).  Within a
// workgroup a pair is joined by the wave butterfly, then the four waves in index order through LDS.  No atomics: two runs give
// the same bits, and the three files give the same partials (tests/test_gpu_cfg_reuse.py compares them).
//
// Every helper is one rounded fp32 operation per statement.  Whether a product may fuse with the sum that takes it is NOT said
// here: no fp-contract pragma.  The including translation unit decides (lcv_hip/build.py, EXTRA): elementwise.hip is built with
// contraction allowed, the other two with -ffp-contract=off, so the Euler step and step 0 of the multistep rules agree in value
// and not in bits (tests/kernel_ref.py).
#pragma once
#include "lcv_common.h"   // wave_sum, LCV_WAVE

static constexpr int CFG_PARTS = 256;     // workgroups (= partial pairs) per sample of a pair of sums
static constexpr int CFG_THREADS = 256;   // one thread per partial pair in the joins
static constexpr int CFG_WAVES = CFG_THREADS / LCV_WAVE;
static_assert(CFG_PARTS == CFG_THREADS && CFG_WAVES == 4, "the joins hold one partial per thread, four waves");

typedef float CfgJoinLds[CFG_WAVES];   // one value's words of the wave-order join: a kernel owns a pair, __shared__

// The workgroup's sum of one value pair per thread, in two halves.  cfg_pair_waves: butterfly inside a wave, the four wave sums
// into LDS, barrier.  cfg_pair_total: the four waves in wave order, for whichever threads want the total.  Two joins through
// one pair of arrays need a __syncthreads() between them.
__device__ __forceinline__ void cfg_pair_waves(float a, float b, CfgJoinLds& sa, CfgJoinLds& sb) {
  a = wave_sum(a);
  b = wave_sum(b);
  if ((threadIdx.x & (LCV_WAVE - 1)) == 0) { sa[threadIdx.x / LCV_WAVE] = a; sb[threadIdx.x / LCV_WAVE] = b; }
  __syncthreads();
}
__device__ __forceinline__ void cfg_pair_total(float& a, float& b, const CfgJoinLds& sa, const CfgJoinLds& sb) {
  a = ((sa[0] + sa[1]) + sa[2]) + sa[3];
  b = ((sb[0] + sb[1]) + sb[2]) + sb[3];
}
// both halves: every thread gets the total
__device__ __forceinline__ void cfg_pair_join(float& a, float& b, CfgJoinLds& sa, CfgJoinLds& sb) {
  cfg_pair_waves(a, b, sa, sb);
  cfg_pair_total(a, b, sa, sb);
}

// The body of the partial-sum kernel, launched CFG_PARTS x B workgroups of CFG_THREADS: ws[b][part][2] = the (dot, nrm) of the
// elements part * 256 + t + k * 65536 of sample b.  The stride is fixed, so every slot is written (an empty slice writes 0).
// SLOTS: the floats a part owns in ws; the pair sits in the first two (cfg_apg.hip keeps four per part, the others keep the pair).
// (The pointers carry no __restrict__ here: the kernels' own parameters do, and the inlined copies only add alias scopes.)
template <int SLOTS = 2>
__device__ __forceinline__ void cfg_partial_sums(const float* cond, const float* uncond, float* ws, int64_t n, CfgJoinLds& sa,
                                                 CfgJoinLds& sb) {
  const int64_t b = blockIdx.y;
  const float* c = cond + b * n;
  const float* u = uncond + b * n;
  float dot = 0.f, nrm = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * CFG_THREADS + threadIdx.x; i < n; i += (int64_t)CFG_PARTS * CFG_THREADS) {
    const float cv = c[i], uv = u[i];
    const float p = cv * uv;
    dot = dot + p;
    const float q = uv * uv;
    nrm = nrm + q;
  }
  cfg_pair_waves(dot, nrm, sa, sb);
  if (threadIdx.x == 0) {
    float part_dot, part_nrm;
    cfg_pair_total(part_dot, part_nrm, sa, sb);
    float* o = ws + (b * CFG_PARTS + blockIdx.x) * SLOTS;
    o[0] = part_dot;
    o[1] = part_nrm;
  }
}

// st of sample b from its CFG_PARTS partial pairs; all CFG_THREADS threads of the workgroup call it
template <int SLOTS = 2>
__device__ __forceinline__ float cfg_star_scale(const float* ws, int64_t b, CfgJoinLds& sa, CfgJoinLds& sb) {
  const float* o = ws + (b * CFG_PARTS + threadIdx.x) * SLOTS;
  float dot = o[0], nrm = o[1];
  cfg_pair_join(dot, nrm, sa, sb);
  const float den = nrm + 1e-8f;
  return dot / den;
}

// v of one element.  `rescale`: u is multiplied by st first.  The Euler step passes true always (its st is 1 when zero-star is
// off), the other two pass use_zero_star: each keeps the operations it had.
__device__ __forceinline__ float cfg_guided(float c, float u, float st, float guidance, bool rescale) {
  if (rescale) u = u * st;
  const float d = c - u;
  const float t = guidance * d;
  return u + t;
}

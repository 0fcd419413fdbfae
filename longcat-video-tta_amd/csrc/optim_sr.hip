// Stochastic rounding for the bf16 optimizer steps (include/lcv_hip_sr.h): the storage of optim.hip's bf16 steps - bf16
// parameters and moments, nothing beside them - with the fp32 op sequences of optim_master.hip (master_elem.h) in between, and
// every store rounded up or down by 16 random bits so that it is an unbiased estimate of the fp32 result.  A thread owns eight
// elements and one Philox4x32-10 call (philox.h) yields eight 16-bit halves: one call per thread and stored tensor.
// Same descriptor table, chunking (optim_common.h) and 16-byte packet / scalar-tail split as optim_master.hip.  HBM-bound
// streaming kernels, per parameter: SGD 4 B read + 2 B written, AdamW 8 + 6.  Built with -ffp-contract=off.  Every output has
// one writer; no LDS.
#include "master_elem.h"   // a thread's 8 floats, the per-element op sequences
#include "philox.h"
#include "lcv_hip_sr.h"

// the 16 random bits of each of a thread's eight elements: stream k of group G
struct sr_bits {
  philox_out r;
  __device__ __forceinline__ sr_bits(uint64_t seed, uint64_t offset, uint64_t k, uint64_t G) {
    const uint64_t c = offset + k;
    r = philox4x32_10((uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)c, (uint32_t)(c >> 32), (uint32_t)G, (uint32_t)(G >> 32));
  }
  // element e takes the low (even e) or high (odd e) half of word e >> 1
  __device__ __forceinline__ uint32_t half(int e) const { return (r.c[e >> 1] >> (16 * (e & 1))) & 0xffffu; }
};

// h = (u + r) >> 16: away from zero with probability (u & 0xffff) / 65536.  Exponent all ones: the upper half, made quiet when
// it is a NaN - what f2bf's round to nearest even stores for these.
__device__ __forceinline__ bf16_t sr_round(float w, uint32_t r) {
  const uint32_t u = __builtin_bit_cast(uint32_t, w);
  if ((u & 0x7f800000u) == 0x7f800000u) return (bf16_t)((u >> 16) | ((u & 0x007fffffu) ? 0x0040u : 0u));
  return (bf16_t)((u + r) >> 16);
}

__device__ __forceinline__ u16x8 sr_pack8(const float (&f)[8], const sr_bits& b) {
  u16x8 v;
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = sr_round(f[e], b.half(e));
  return v;
}

__global__ __launch_bounds__(256) void sr_sgd_kernel(const lcv_adam_tensor* __restrict__ tensors, int n,
                                                     const float* __restrict__ clip, float lr, float wd, uint64_t seed,
                                                     uint64_t offset) {
  const int ti = find_tensor(tensors, n, blockIdx.x);
  const lcv_adam_tensor t = tensors[ti];
  const int64_t base = ((int64_t)blockIdx.x - t.first_chunk) * CHUNK + threadIdx.x * 8;
  if (base >= t.numel) return;
  const float coef = clip ? clip[1] : 1.0f;
  bf16_t* P = (bf16_t*)t.param;
  const bf16_t* G = (const bf16_t*)t.grad;
  const sr_bits bp(seed, offset, 0, (uint64_t)blockIdx.x * 256 + threadIdx.x);
  if (base + 8 <= t.numel && ((((uintptr_t)P) | ((uintptr_t)G)) & 15) == 0) {   // whole 16-byte packets
    float p[8], g[8];
    unpack8(*reinterpret_cast<const u16x8*>(P + base), p);
    unpack8(*reinterpret_cast<const u16x8*>(G + base), g);
#pragma unroll
    for (int e = 0; e < 8; ++e) p[e] = master_sgd_elem(p[e], g[e], coef, lr, wd);
    *reinterpret_cast<u16x8*>(P + base) = sr_pack8(p, bp);
    return;
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int64_t i = base + e;
    if (i >= t.numel) break;
    P[i] = sr_round(master_sgd_elem(bf2f(P[i]), bf2f(G[i]), coef, lr, wd), bp.half(e));
  }
}

__global__ __launch_bounds__(256) void sr_adamw_kernel(const lcv_adam_tensor* __restrict__ tensors, int n,
                                                       const float* __restrict__ clip, const AdamScalars s, uint64_t seed,
                                                       uint64_t offset) {
  const int ti = find_tensor(tensors, n, blockIdx.x);
  const lcv_adam_tensor t = tensors[ti];
  const int64_t base = ((int64_t)blockIdx.x - t.first_chunk) * CHUNK + threadIdx.x * 8;
  if (base >= t.numel) return;
  const float coef = clip ? clip[1] : 1.0f;
  bf16_t* P = (bf16_t*)t.param;
  const bf16_t* G = (const bf16_t*)t.grad;
  bf16_t* M = (bf16_t*)t.exp_avg;
  bf16_t* V = (bf16_t*)t.exp_avg_sq;
  const uint64_t group = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const sr_bits bp(seed, offset, 0, group), bm(seed, offset, 1, group), bv(seed, offset, 2, group);
  if (base + 8 <= t.numel && ((((uintptr_t)P) | ((uintptr_t)G) | ((uintptr_t)M) | ((uintptr_t)V)) & 15) == 0) {   // whole packets
    float p[8], g[8], m[8], v[8];
    unpack8(*reinterpret_cast<const u16x8*>(P + base), p);
    unpack8(*reinterpret_cast<const u16x8*>(G + base), g);
    unpack8(*reinterpret_cast<const u16x8*>(M + base), m);
    unpack8(*reinterpret_cast<const u16x8*>(V + base), v);
#pragma unroll
    for (int e = 0; e < 8; ++e) master_adamw_elem(p[e], m[e], v[e], g[e], coef, s);
    *reinterpret_cast<u16x8*>(P + base) = sr_pack8(p, bp);
    *reinterpret_cast<u16x8*>(M + base) = sr_pack8(m, bm);
    *reinterpret_cast<u16x8*>(V + base) = sr_pack8(v, bv);
    return;
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int64_t i = base + e;
    if (i >= t.numel) break;
    float p = bf2f(P[i]), m = bf2f(M[i]), v = bf2f(V[i]);
    master_adamw_elem(p, m, v, bf2f(G[i]), coef, s);
    P[i] = sr_round(p, bp.half(e));
    M[i] = sr_round(m, bm.half(e));
    V[i] = sr_round(v, bv.half(e));
  }
}

// one workgroup per CHUNK elements of a single array: G = i >> 3, stream 0
__global__ __launch_bounds__(256) void sr_round_kernel(const float* __restrict__ x, bf16_t* __restrict__ out, int64_t n,
                                                       uint64_t seed, uint64_t offset) {
  const int64_t base = (int64_t)blockIdx.x * CHUNK + threadIdx.x * 8;
  if (base >= n) return;
  const sr_bits b(seed, offset, 0, (uint64_t)base >> 3);
  if (base + 8 <= n && ((((uintptr_t)x) | ((uintptr_t)out)) & 15) == 0) {   // whole 16-byte packets
    float w[8];
    load8(x + base, w);
    *reinterpret_cast<u16x8*>(out + base) = sr_pack8(w, b);
    return;
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int64_t i = base + e;
    if (i >= n) break;
    out[i] = sr_round(x[i], b.half(e));
  }
}

extern "C" int lcv_sr_sgd_step(const lcv_adam_tensor* tensors, int64_t n_tensors, int64_t total_chunks, const float* norm_coef,
                               double lr, double weight_decay, uint64_t seed, uint64_t offset, void* stream) {
  LCV_CHECK_ARG(tensors && optim_table_ok(n_tensors, total_chunks), "sr_sgd_step: bad arguments");
  hipLaunchKernelGGL(sr_sgd_kernel, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)stream, tensors, (int)n_tensors,
                     norm_coef, (float)lr, (float)weight_decay, seed, offset);
  LCV_LAUNCH_CHECK("sr_sgd_step");
  return LCV_OK;
}

extern "C" int lcv_sr_adamw_step(const lcv_adam_tensor* tensors, int64_t n_tensors, int64_t total_chunks, const float* norm_coef,
                                 double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step,
                                 uint64_t seed, uint64_t offset, void* stream) {
  LCV_CHECK_ARG(tensors && optim_table_ok(n_tensors, total_chunks) && step >= 1, "sr_adamw_step: bad arguments");
  hipLaunchKernelGGL(sr_adamw_kernel, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)stream, tensors, (int)n_tensors,
                     norm_coef, adam_scalars(lr, beta1, beta2, eps, weight_decay, step), seed, offset);
  LCV_LAUNCH_CHECK("sr_adamw_step");
  return LCV_OK;
}

extern "C" int lcv_sr_round(const float* x, void* out_bf16, int64_t n, uint64_t seed, uint64_t offset, void* stream) {
  unsigned blocks = 0;
  LCV_CHECK_ARG(x && out_bf16 && chunk_grid(n, blocks), "sr_round: bad arguments");
  hipLaunchKernelGGL(sr_round_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, (bf16_t*)out_bf16, n, seed, offset);
  LCV_LAUNCH_CHECK("sr_round");
  return LCV_OK;
}

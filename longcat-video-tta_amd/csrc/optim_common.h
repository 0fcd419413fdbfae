// What the optimizer kernels (optim.hip) and the fixed-order gradient-norm clip (reduce_det.hip) share: the chunking of the
// descriptor table, one chunk's sum of squares, and the launcher of the clip coefficient; and what every optimizer entry point
// over that table shares on the host (the master-weight files too): AdamW's scalars, the table check, a single array's grid.
#pragma once
#include "lcv_common.h"
#include <math.h>

static constexpr int CHUNK = 2048;  // elements per workgroup (256 threads x 8)
// per-tensor sum-of-squares accumulators: chunk c of a tensor adds into slot c % NORM_SLOTS of that tensor's row, the
// coefficient kernel adds the row up.  One slot per tensor makes a 45 M-element weight (22 000 chunks) a queue on one address.
// (The fixed-order form writes a tensor's whole sum to slot 0 and zeros to the rest.)
static constexpr int NORM_SLOTS = 64;

__device__ __forceinline__ int find_tensor(const lcv_adam_tensor* t, int n, int64_t chunk) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (t[mid].first_chunk <= chunk) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// sum of squares of chunk `chunk` of tensor t's gradient, one workgroup of 256: fma chain (whole bf16 packet) or mul + add per
// thread, wave_sum, then w0 + w1 + w2 + w3 (every thread returns the block's sum; the caller stores it from thread 0).
template <bool F32>
__device__ __forceinline__ float grad_chunk_sumsq(const lcv_adam_tensor& t, int64_t chunk) {
  const int64_t base = chunk * CHUNK + threadIdx.x * 8;
  float acc = 0.f;
  if (!F32 && base + 8 <= t.numel && (((uintptr_t)t.grad) & 15) == 0) {      // whole 16-byte packet
    float g[8];
    unpack8(*reinterpret_cast<const u16x8*>((const bf16_t*)t.grad + base), g);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc = fmaf(g[e], g[e], acc);
  } else {
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int64_t i = base + e;
      if (i < t.numel) {
        const float g = F32 ? ((const float*)t.grad)[i] : bf2f(((const bf16_t*)t.grad)[i]);
        acc += g * g;
      }
    }
  }
  __shared__ float part[4];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  return part[0] + part[1] + part[2] + part[3];
}

// ---- host: what the entry points over a descriptor table share ----
// AdamW's scalars, formed in double exactly as torch/optim/adamw.py forms them, then narrowed to the kernels' opmath (fp32)
struct AdamScalars {
  float c_wd, w1, b2, c2, bc2_sqrt, eps, step_size;
};

static inline AdamScalars adam_scalars(double lr, double beta1, double beta2, double eps, double weight_decay, int64_t step) {
  const double bc1 = 1.0 - pow(beta1, (double)step);
  const double bc2 = 1.0 - pow(beta2, (double)step);
  AdamScalars sc;
  sc.c_wd = (float)(1.0 - lr * weight_decay);
  sc.w1 = (float)(1.0 - beta1);
  sc.b2 = (float)beta2;
  sc.c2 = (float)(1.0 - beta2);
  sc.bc2_sqrt = (float)sqrt(bc2);
  sc.eps = (float)eps;
  sc.step_size = (float)((lr / bc1) * -1.0);
  return sc;
}

// a table's counts fit the kernels' int arguments and the grid
static inline bool optim_table_ok(int64_t n_tensors, int64_t total_chunks) {
  return n_tensors > 0 && n_tensors <= 0x7fffffff && total_chunks > 0 && total_chunks <= 0x7fffffff;
}

// one workgroup per CHUNK of a single array of n elements
static inline bool chunk_grid(int64_t n, unsigned& blocks) {
  if (n < 1) return false;
  const int64_t b = (n + CHUNK - 1) / CHUNK;
  if (b > 0x7fffffff) return false;
  blocks = (unsigned)b;
  return true;
}

// ---- host: internal launcher shared by the two clip entry points (the caller runs LCV_LAUNCH_CHECK under its own name) ----
// optim.hip: out[0] = total norm over the n rows of per_tensor, out[1] = min(max_norm / (total + 1e-6), 1)
void clip_coef_launch(const float* per_tensor, int n, float max_norm, float* out, bool f32, hipStream_t s);

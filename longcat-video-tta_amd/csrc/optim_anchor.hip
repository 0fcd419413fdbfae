// The drift from the base weights (include/lcv_hip_anchor.h): the sum of squares of w - w0 over every element, where
// w = join(h, l) and w0 = float(h0) is the bf16 base word of the element.  (The steps that decay toward w0 are forms of the
// master-weight step kernels: optim_master.hip, optim_moments8.hip.)  Same descriptor table, chunking (optim_common.h) and
// 16-byte packet / scalar-tail split as optim_master.hip; the format is master_elem.h's.  HBM-bound streaming kernel: 6 B read
// per parameter (4 B without low words).  Built with -ffp-contract=off.  Every output has one writer and every sum a fixed
// order.
#include "master_elem.h"
#include "lcv_hip_anchor.h"

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

extern "C" int lcv_master_drift_sumsq(const lcv_adam_tensor* tensors, void* const* low, void* const* anchor, int64_t n_tensors,
                                      int64_t total_chunks, float* partials, int64_t partials_bytes, float* out, void* stream) {
  LCV_CHECK_ARG(tensors && anchor && out && optim_table_ok(n_tensors, total_chunks), "master_drift_sumsq: bad arguments");
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

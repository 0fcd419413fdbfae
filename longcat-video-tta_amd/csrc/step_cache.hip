// The first-block step cache of the denoise loop (include/lcv_hip_stepcache.h): block 0's residual r = bf16(x1 - x0), its L1
// distance to the residual p of the last computed step with the skip decision, and the two ends of the cached residual of
// blocks 1...L-1 (store R = bf16(xL - x1), apply out = bf16(x1 + R)).  HBM-bound streaming kernels over whole 16-byte packets
// (every count is a multiple of 8 and every pointer 16-byte aligned: the launchers refuse anything else), per element: diff
// 6 B read + 2 B written (4 + 2 without p), store and apply 4 + 2.  Built with -ffp-contract=off.  Every output has one writer
// and every sum a fixed order, in the manner of drift_chunk_kernel / drift_final_kernel (optim_anchor.hip); LDS holds the
// wave-order join only.
#include "optim_common.h"   // CHUNK and, through lcv_common.h, the packet types and wave_sum
#include "lcv_hip_stepcache.h"

#pragma clang fp contract(off)

static constexpr int SC_MAX_ROWS = 8;
static constexpr int SC_FINAL_THREADS = 1024;

// One workgroup per 2048-element chunk of a row, chunks_per_row of them per row; the last chunk of a row may be partly (in
// whole packets) past its end, and those threads add zeros.  PREV: also the chunk's partial pair, num partials first.
template <bool PREV>
__global__ __launch_bounds__(256) void stepcache_diff_kernel(const bf16_t* __restrict__ x0, const bf16_t* __restrict__ x1,
                                                             const bf16_t* __restrict__ prev, bf16_t* __restrict__ r_out,
                                                             int64_t n, int chunks_per_row, int total_chunks,
                                                             float* __restrict__ partials, unsigned int* __restrict__ decision) {
  const int row = blockIdx.x / chunks_per_row, c = blockIdx.x - row * chunks_per_row;
  const int64_t col = (int64_t)c * CHUNK + threadIdx.x * 8;
  float num = 0.f, den = 0.f;
  if (col < n) {                                                         // n % 8 == 0: a whole packet or none
    const int64_t at = (int64_t)row * n + col;
    const u16x8 a = *reinterpret_cast<const u16x8*>(x0 + at);
    const u16x8 b = *reinterpret_cast<const u16x8*>(x1 + at);
    u16x8 pv = {0, 0, 0, 0, 0, 0, 0, 0};
    if (PREV) pv = *reinterpret_cast<const u16x8*>(prev + at);
    u16x8 rv;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float d0 = bf2f(b[e]) - bf2f(a[e]);
      rv[e] = f2bf(d0);
      if (PREV) {
        const float p = bf2f(pv[e]);
        const float d = bf2f(rv[e]) - p;
        num = num + __builtin_fabsf(d);
        den = den + __builtin_fabsf(p);
      }
    }
    *reinterpret_cast<u16x8*>(r_out + at) = rv;
  }
  if (!PREV) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *decision = 0u;             // no p: the step is computed
    return;
  }
  __shared__ float part[2][4];
  num = wave_sum(num);
  den = wave_sum(den);
  if ((threadIdx.x & (LCV_WAVE - 1)) == 0) { part[0][threadIdx.x / LCV_WAVE] = num; part[1][threadIdx.x / LCV_WAVE] = den; }
  __syncthreads();
  if (threadIdx.x == 0) {
    partials[blockIdx.x] = ((part[0][0] + part[0][1]) + part[0][2]) + part[0][3];
    partials[(int64_t)total_chunks + blockIdx.x] =((part[1][0] + part[1][1]) + part[1][2]) + part[1][3];
  }
}

// the workgroup's sum of v[0 .. count): thread t adds t, t + 1024, ... in index order, the wave's butterfly, then the waves in
// wave order; thread 0 holds the result
__device__ __forceinline__ float stepcache_row_sum(const float* __restrict__ v, int count, float (&part)[SC_FINAL_THREADS / LCV_WAVE]) {
  float acc = 0.f;
#pragma unroll 8
  for (int c = threadIdx.x; c < count; c += SC_FINAL_THREADS) acc = acc + v[c];
  acc = wave_sum(acc);
  __syncthreads();                                                       // the previous sum's readers are done with part[]
  if ((threadIdx.x & (LCV_WAVE - 1)) == 0) part[threadIdx.x / LCV_WAVE] = acc;
  __syncthreads();
  float s = 0.f;
  if (threadIdx.x == 0) {
    s = part[0];
    for (int w = 1; w < SC_FINAL_THREADS / LCV_WAVE; ++w) s = s + part[w];
  }
  return s;
}

// one workgroup, the rows one after the other: out[b] = num[b], out[rows + b] = den[b], then the decision over all rows
__global__ __launch_bounds__(SC_FINAL_THREADS) void stepcache_final_kernel(const float* __restrict__ partials, int rows,
                                                                           int chunks_per_row, float thr, float* __restrict__ out) {
  __shared__ float part[SC_FINAL_THREADS / LCV_WAVE];
  const int total_chunks = rows * chunks_per_row;
  bool skip = true;
  for (int b = 0; b < rows; ++b) {
    const float num = stepcache_row_sum(partials + (int64_t)b * chunks_per_row, chunks_per_row, part);
    const float den = stepcache_row_sum(partials + total_chunks + (int64_t)b * chunks_per_row, chunks_per_row, part);
    if (threadIdx.x == 0) {
      out[b] = num;
      out[rows + b] = den;
      const float bound = thr * den;
      skip = skip && (num < bound);                                      // false for a NaN on either side and for den = 0
    }
  }
  if (threadIdx.x == 0) reinterpret_cast<unsigned int*>(out)[2 * rows] = skip ? 1u : 0u;
}

// SUB: o = bf16(a - b), else o = bf16(a + b).  o may be a (each thread reads its packet before it writes it).
template <bool SUB>
__global__ __launch_bounds__(256) void stepcache_combine_kernel(const bf16_t* a, const bf16_t* __restrict__ b, bf16_t* o,
                                                                int64_t total) {
  const int64_t at = (int64_t)blockIdx.x * CHUNK + threadIdx.x * 8;
  if (at >= total) return;                                               // total % 8 == 0: a whole packet or none
  const u16x8 av = *reinterpret_cast<const u16x8*>(a + at);
  const u16x8 bv = *reinterpret_cast<const u16x8*>(b + at);
  u16x8 ov;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const float x = bf2f(av[e]), y = bf2f(bv[e]);
    ov[e] = f2bf(SUB ? x - y : x + y);
  }
  *reinterpret_cast<u16x8*>(o + at) = ov;
}

static bool sc_aligned(const void* p) { return (((uintptr_t)p) & 15) == 0; }

extern "C" int lcv_stepcache_diff(const void* x0, const void* x1, const void* prev, void* r_out, int64_t rows, int64_t n, float thr,
                                  float* partials, int64_t partials_bytes, float* out, void* stream) {
  LCV_CHECK_ARG(x0 && x1 && r_out && out && sc_aligned(x0) && sc_aligned(x1) && sc_aligned(prev) && sc_aligned(r_out) &&
                    (((uintptr_t)out) & 3) == 0,
                "stepcache_diff: a pointer is missing or not 16-byte aligned");
  LCV_CHECK_ARG(r_out != x0 && r_out != x1 && r_out != prev, "stepcache_diff: r_out must be a buffer of its own");
  LCV_CHECK_ARG(rows >= 1 && rows <= SC_MAX_ROWS, "stepcache_diff: rows must be in 1..%d, got %ld", SC_MAX_ROWS, (long)rows);
  LCV_CHECK_ARG(n >= 8 && n % 8 == 0, "stepcache_diff: n must be a positive multiple of 8, got %ld", (long)n);
  LCV_CHECK_ARG(thr >= 0.f, "stepcache_diff: the threshold must be >= 0 and not NaN, got %g", (double)thr);   // NaN fails
  const int64_t cpr = (n + CHUNK - 1) / CHUNK, total = rows * cpr;
  LCV_CHECK_ARG(total <= 0x7fffffff, "stepcache_diff: %ld chunks are more than one launch takes", (long)total);
  const dim3 grid((unsigned)total), block(256);
  unsigned int* decision = reinterpret_cast<unsigned int*>(out) + 2 * rows;
  if (!prev) {
    hipLaunchKernelGGL(stepcache_diff_kernel<false>, grid, block, 0, (hipStream_t)stream, (const bf16_t*)x0, (const bf16_t*)x1,
                       (const bf16_t*)nullptr, (bf16_t*)r_out, n, (int)cpr, (int)total, (float*)nullptr, decision);
    LCV_LAUNCH_CHECK("stepcache_diff");
    return LCV_OK;
  }
  LCV_CHECK_ARG(partials && partials_bytes >= total * 8 && ((uintptr_t)partials % 4) == 0,
                "stepcache_diff: workspace of %ld bytes is missing or too small (need %ld)", (long)partials_bytes,
                (long)(total * 8));
  hipLaunchKernelGGL(stepcache_diff_kernel<true>, grid, block, 0, (hipStream_t)stream, (const bf16_t*)x0, (const bf16_t*)x1,
                     (const bf16_t*)prev, (bf16_t*)r_out, n, (int)cpr, (int)total, partials, decision);
  LCV_LAUNCH_CHECK("stepcache_diff: chunks");
  hipLaunchKernelGGL(stepcache_final_kernel, dim3(1), dim3(SC_FINAL_THREADS), 0, (hipStream_t)stream, partials, (int)rows,
                     (int)cpr, thr, out);
  LCV_LAUNCH_CHECK("stepcache_diff: rows");
  return LCV_OK;
}

static int stepcache_combine(bool sub, const void* a, const void* b, void* o, int64_t total, void* stream, const char* name) {
  LCV_CHECK_ARG(a && b && o && sc_aligned(a) && sc_aligned(b) && sc_aligned(o), "%s: a pointer is missing or not 16-byte aligned",
                name);
  LCV_CHECK_ARG(total >= 8 && total % 8 == 0, "%s: total must be a positive multiple of 8, got %ld", name, (long)total);
  const int64_t chunks = (total + CHUNK - 1) / CHUNK;
  LCV_CHECK_ARG(chunks <= 0x7fffffff, "%s: %ld chunks are more than one launch takes", name, (long)chunks);
  if (sub)
    hipLaunchKernelGGL(stepcache_combine_kernel<true>, dim3((unsigned)chunks), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)a,
                       (const bf16_t*)b, (bf16_t*)o, total);
  else
    hipLaunchKernelGGL(stepcache_combine_kernel<false>, dim3((unsigned)chunks), dim3(256), 0, (hipStream_t)stream,
                       (const bf16_t*)a, (const bf16_t*)b, (bf16_t*)o, total);
  LCV_LAUNCH_CHECK(name);
  return LCV_OK;
}

extern "C" int lcv_stepcache_store(const void* xL, const void* x1, void* R, int64_t total, void* stream) {
  LCV_CHECK_ARG(R != xL && R != x1, "stepcache_store: R must be a buffer of its own");
  return stepcache_combine(true, xL, x1, R, total, stream, "stepcache_store");
}

extern "C" int lcv_stepcache_apply(const void* x1, const void* R, void* out, int64_t total, void* stream) {
  LCV_CHECK_ARG(out != R, "stepcache_apply: out may be x1 but not R");
  return stepcache_combine(false, x1, R, out, total, stream, "stepcache_apply");
}

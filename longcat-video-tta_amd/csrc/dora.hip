// Weight-decomposed LoRA (include/lcv_hip_dora.h): the row norm of the adapted weight W + s B A, and the column scale
// c = m / wn on the output of the LoRA GEMM, forward and backward.  HBM-bound row and column work: the norm reads W once
// (2 B per element) and A once per workgroup through LDS, the scales read and write the output once each.  Built with
// -ffp-contract=off: every step is one correctly rounded fp32 operation in the order the header states.  A product of two bf16
// values is exact in fp32, so __builtin_fmaf(b, a, t) below is the header's t + b * a, in one instruction.  Every output has
// one writer; no atomics.
#include "lcv_common.h"
#include "lcv_hip_dora.h"

#define DORA_KTILE LCV_DORA_NORM_KTILE
#define DORA_ROWS LCV_DORA_NORM_ROWS
#define DORA_WROWS 4            // rows of one wave of the norm kernel
#define DORA_SLAB LCV_DORA_SLAB
#define DORA_QUARTER LCV_DORA_SLAB_QUARTER   // rows of one wave of the backward scale
#define DORA_FWD_ROWS 64        // rows of one workgroup of the forward scale: 4 waves x 16 rows

static_assert(DORA_KTILE == 64 * 8 && DORA_ROWS == 4 * DORA_WROWS && DORA_SLAB == 4 * DORA_QUARTER,
              "one packet per lane per tile, four waves");

// ------------------------------------------------------------------ wn[n] = | W[n, :] + s * B[n, :] A | ---
// Workgroup: 256 threads, DORA_ROWS rows; wave w takes rows row0 + 4 w .. + 3, lane l the packet of columns k0 + 8 l .. + 7 of
// every tile.  The A tile [R][512] sits in LDS (16-byte reads at 16 * lane: contiguous), B of the wave's rows beside it as
// [r][4] floats, one broadcast 16-byte read per r.
template <bool ADAPT>
__global__ __launch_bounds__(256) void dora_weight_norm_kernel(const bf16_t* __restrict__ W, const bf16_t* __restrict__ A,
                                                               const bf16_t* __restrict__ B, float s, int64_t N, int K, int R,
                                                               float* __restrict__ wn) {
  __shared__ __attribute__((aligned(16))) bf16_t As[ADAPT ? 32 * DORA_KTILE : 8];
  __shared__ __attribute__((aligned(16))) float Bs[ADAPT ? 4 * 32 * DORA_WROWS : 4];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int64_t row0 = (int64_t)blockIdx.x * DORA_ROWS + wave * DORA_WROWS;
  if (ADAPT) {
    for (int i = tid; i < 4 * 32 * DORA_WROWS; i += 256) {          // Bs[w][r][j] = B[row(w, j), r], 0 outside
      const int w = i / (32 * DORA_WROWS), r = (i / DORA_WROWS) % 32, j = i % DORA_WROWS;
      const int64_t n = (int64_t)blockIdx.x * DORA_ROWS + w * DORA_WROWS + j;
      Bs[i] = (r < R && n < N) ? bf2f(B[n * R + r]) : 0.f;
    }
  }
  float acc[DORA_WROWS] = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < K; k0 += DORA_KTILE) {
    const int k = k0 + lane * 8;
    u16x8 wv[DORA_WROWS];
#pragma unroll
    for (int j = 0; j < DORA_WROWS; ++j) {                            // W: in flight while A is staged
      wv[j] = (u16x8){0, 0, 0, 0, 0, 0, 0, 0};
      if (k < K && row0 + j < N) wv[j] = *reinterpret_cast<const u16x8*>(W + (row0 + j) * K + k);
    }
    float t[DORA_WROWS][8];
#pragma unroll
    for (int j = 0; j < DORA_WROWS; ++j)
#pragma unroll
      for (int e = 0; e < 8; ++e) t[j][e] = 0.f;
    if (ADAPT) {
      if (k0) __syncthreads();                                        // the previous tile has been read
      for (int i = tid; i < R * 64; i += 256) {
        const int r = i >> 6, kk = k0 + (i & 63) * 8;
        u16x8 av = {0, 0, 0, 0, 0, 0, 0, 0};
        if (kk < K) av = *reinterpret_cast<const u16x8*>(A + (int64_t)r * K + kk);
        *reinterpret_cast<u16x8*>(&As[r * DORA_KTILE + (i & 63) * 8]) = av;
      }
      __syncthreads();
      for (int r = 0; r < R; ++r) {
        float af[8];
        unpack8(*reinterpret_cast<const u16x8*>(&As[r * DORA_KTILE + lane * 8]), af);
        const f32x4 b4 = *reinterpret_cast<const f32x4*>(&Bs[(wave * 32 + r) * DORA_WROWS]);
#pragma unroll
        for (int j = 0; j < DORA_WROWS; ++j)
#pragma unroll
          for (int e = 0; e < 8; ++e) t[j][e] = __builtin_fmaf(b4[j], af[e], t[j][e]);   // exact product: t + b * a
      }
    }
    if (k < K) {
#pragma unroll
      for (int j = 0; j < DORA_WROWS; ++j) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float v = bf2f(wv[j][e]);
          if (ADAPT) { const float u = s * t[j][e]; v = v + u; }
          const float q = v * v;
          acc[j] = acc[j] + q;
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < DORA_WROWS; ++j) {
    const float p = wave_sum(acc[j]);                                 // P[l] += P[l ^ o], o = 32 .. 1
    if (lane == 0 && row0 + j < N) wn[row0 + j] = __builtin_sqrtf(p);
  }
}

extern "C" int lcv_dora_weight_norm(const void* w, const void* a, const void* b, double scaling, int64_t N, int64_t K, int64_t R,
                                    void* wn_out, void* stream) {
  LCV_CHECK_ARG(w && wn_out && N >= 1 && K >= 1, "dora_weight_norm: null pointer or size < 1");
  LCV_CHECK_ARG(K % 8 == 0 && K <= (int64_t)1 << 30 && N <= ((int64_t)1 << 31) - 1 - DORA_ROWS && ((uintptr_t)w & 15) == 0 &&
                    ((uintptr_t)wn_out & 3) == 0,
                "dora_weight_norm: K must be a multiple of 8 (16-byte rows) and w 16-byte aligned");
  const unsigned grid = (unsigned)((N + DORA_ROWS - 1) / DORA_ROWS);
  if (b) {
    LCV_CHECK_ARG(a && R >= 1 && R <= 32, "dora_weight_norm: a is null or R is outside 1..32");
    LCV_CHECK_ARG(((uintptr_t)a & 15) == 0 && ((uintptr_t)b & 1) == 0, "dora_weight_norm: a must be 16-byte aligned");
    hipLaunchKernelGGL(dora_weight_norm_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)w,
                       (const bf16_t*)a, (const bf16_t*)b, (float)scaling, N, (int)K, (int)R, (float*)wn_out);
  } else {
    hipLaunchKernelGGL(dora_weight_norm_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)w,
                       (const bf16_t*)nullptr, (const bf16_t*)nullptr, 0.f, N, (int)K, 0, (float*)wn_out);
  }
  LCV_LAUNCH_CHECK("dora_weight_norm");
  return LCV_OK;
}

// ------------------------------------------------------------------------------------- c = m / wn ---
__device__ __forceinline__ void dora_scale8(const float* __restrict__ m, const float* __restrict__ wn, int64_t n, float (&c)[8]) {
  const f32x4 m0 = *reinterpret_cast<const f32x4*>(m + n), m1 = *reinterpret_cast<const f32x4*>(m + n + 4);
  const f32x4 w0 = *reinterpret_cast<const f32x4*>(wn + n), w1 = *reinterpret_cast<const f32x4*>(wn + n + 4);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    c[e] = w0[e] == 0.f ? 0.f : m0[e] / w0[e];
    c[e + 4] = w1[e] == 0.f ? 0.f : m1[e] / w1[e];
  }
}

// grid (ceil(N / 512), ceil(M / 64)); lane = one 16-byte packet of columns, wave w rows r0 + w, r0 + w + 4, ...
template <bool BIAS>
__global__ __launch_bounds__(256) void dora_colscale_fwd_kernel(const bf16_t* pre, const float* __restrict__ m,
                                                                const float* __restrict__ wn, const bf16_t* __restrict__ bias,
                                                                bf16_t* y, int64_t M, int64_t N) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t n = ((int64_t)blockIdx.x * 64 + lane) * 8;
  if (n >= N) return;
  float c[8], bv[8];
  dora_scale8(m, wn, n, c);
  if (BIAS) unpack8(*reinterpret_cast<const u16x8*>(bias + n), bv);
  const int64_t r0 = (int64_t)blockIdx.y * DORA_FWD_ROWS;
  const int64_t r1 = r0 + DORA_FWD_ROWS < M ? r0 + DORA_FWD_ROWS : M;
#pragma unroll 4
  for (int64_t r = r0 + wave; r < r1; r += 4) {
    float f[8];
    unpack8(*reinterpret_cast<const u16x8*>(pre + r * N + n), f);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      f[e] = f[e] * c[e];
      if (BIAS) f[e] = f[e] + bv[e];
    }
    *reinterpret_cast<u16x8*>(y + r * N + n) = pack8(f);
  }
}

extern "C" int lcv_dora_colscale_fwd(const void* pre, const void* m, const void* wn, const void* bias, void* y, int64_t M,
                                     int64_t N, void* stream) {
  LCV_CHECK_ARG(pre && m && wn && y && M >= 1 && N >= 1, "dora_colscale_fwd: null pointer or size < 1");
  LCV_CHECK_ARG(N % 8 == 0 && ((((uintptr_t)pre) | ((uintptr_t)y) | ((uintptr_t)bias) | ((uintptr_t)m) | ((uintptr_t)wn)) & 15) == 0,
                "dora_colscale_fwd: N must be a multiple of 8 and every pointer 16-byte aligned");
  const int64_t gx = (N / 8 + 63) / 64, gy = (M + DORA_FWD_ROWS - 1) / DORA_FWD_ROWS;
  LCV_CHECK_ARG(gx <= 0x7fffffff && gy <= 65535,"dora_colscale_fwd: too many rows or columns");
  const dim3 grid((unsigned)gx, (unsigned)gy);
  if (bias)
    hipLaunchKernelGGL(dora_colscale_fwd_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)pre, (const float*)m,
                       (const float*)wn, (const bf16_t*)bias, (bf16_t*)y, M, N);
  else
    hipLaunchKernelGGL(dora_colscale_fwd_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)pre, (const float*)m,
                       (const float*)wn, (const bf16_t*)nullptr, (bf16_t*)y, M, N);
  LCV_LAUNCH_CHECK("dora_colscale_fwd");
  return LCV_OK;
}

// grid (ceil(N / 512), slabs); one workgroup per slab of 64 rows: wave w takes the quarter of rows 16 w .. 16 w + 15 row by row,
// four rows in flight at a time; waves 1 .. 3 hand their partials to wave 0 through LDS, which adds them in quarter order
__global__ __launch_bounds__(256) void dora_colscale_bwd_kernel(const bf16_t* dy, const bf16_t* __restrict__ pre,
                                                                const float* __restrict__ m, const float* __restrict__ wn,
                                                                bf16_t* dpre, float* __restrict__ ws, int64_t M, int64_t N) {
  __shared__ float part[3][8][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t n = ((int64_t)blockIdx.x * 64 + lane) * 8;
  const int64_t slab = blockIdx.y;
  const int64_t r0 = slab * DORA_SLAB + wave * DORA_QUARTER;
  const int64_t r1 = r0 + DORA_QUARTER < M ? r0 + DORA_QUARTER : M;    // r1 <= r0: a quarter without rows adds +0
  const bool live = n < N;
  float c[8], p[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) { c[e] = 0.f; p[e] = 0.f; }
  if (live) {
    dora_scale8(m, wn, n, c);
    for (int64_t r = r0; r < r1; r += 4) {
      u16x8 gv[4], xv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (r + i < r1) {
          gv[i] = *reinterpret_cast<const u16x8*>(dy + (r + i) * N + n);
          xv[i] = *reinterpret_cast<const u16x8*>(pre + (r + i) * N + n);
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (r + i < r1) {
          float g[8], x[8];
          unpack8(gv[i], g); unpack8(xv[i], x);
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            p[e] = p[e] + g[e] * x[e];
            g[e] = g[e] * c[e];
          }
          *reinterpret_cast<u16x8*>(dpre + (r + i) * N + n) = pack8(g);
        }
      }
    }
  }
  if (wave) {
#pragma unroll
    for (int e = 0; e < 8; ++e) part[wave - 1][e][lane] = p[e];
  }
  __syncthreads();
  if (wave == 0 && live) {
#pragma unroll
    for (int q = 0; q < 3; ++q)
#pragma unroll
      for (int e = 0; e < 8; ++e) p[e] = p[e] + part[q][e][lane];
    float* out = ws + slab * N + n;
    *reinterpret_cast<f32x4*>(out) = (f32x4){p[0], p[1], p[2], p[3]};
    *reinterpret_cast<f32x4*>(out + 4) = (f32x4){p[4], p[5], p[6], p[7]};
  }
}

__global__ __launch_bounds__(256) void dora_dm_reduce_kernel(const float* __restrict__ ws, const float* __restrict__ wn,
                                                             float* __restrict__ dm, int64_t slabs, int64_t N) {
  const int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  float s = 0.f;
#pragma unroll 16
  for (int64_t j = 0; j < slabs; ++j) s = s + ws[j * N + n];     // sixteen loads in flight, added in slab order
  const float w = wn[n];
  dm[n] = w == 0.f ? 0.f : s / w;
}

extern "C" int64_t lcv_dora_colscale_bwd_ws_bytes(int64_t M, int64_t N) {
  if (M < 1 || N < 1) return LCV_EINVAL;
  return (M + DORA_SLAB - 1) / DORA_SLAB * N * (int64_t)sizeof(float);
}

extern "C" int lcv_dora_colscale_bwd(const void* dy, const void* pre, const void* m, const void* wn, void* dpre, void* dm, void* ws,
                                     int64_t ws_bytes, int64_t M, int64_t N, void* stream) {
  LCV_CHECK_ARG(dy && pre && m && wn && dpre && dm && ws && M >= 1 && N >= 1, "dora_colscale_bwd: null pointer or size < 1");
  LCV_CHECK_ARG(N % 8 == 0 && ((((uintptr_t)dy) | ((uintptr_t)pre) | ((uintptr_t)dpre) | ((uintptr_t)ws) | ((uintptr_t)m) |
                                ((uintptr_t)wn)) & 15) == 0 && ((uintptr_t)dm & 3) == 0 && dpre != pre,
                "dora_colscale_bwd: N must be a multiple of 8, every pointer 16-byte aligned, dpre not pre");
  LCV_CHECK_ARG(ws_bytes >= lcv_dora_colscale_bwd_ws_bytes(M, N), "dora_colscale_bwd: workspace of %lld bytes, %lld needed",
                (long long)ws_bytes, (long long)lcv_dora_colscale_bwd_ws_bytes(M, N));
  const int64_t slabs = (M + DORA_SLAB - 1) / DORA_SLAB, gx = (N / 8 + 63) / 64, gy = slabs;
  LCV_CHECK_ARG(gx <= 0x7fffffff && gy <= 65535, "dora_colscale_bwd: too many rows or columns");
  hipLaunchKernelGGL(dora_colscale_bwd_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)dy, (const bf16_t*)pre, (const float*)m, (const float*)wn, (bf16_t*)dpre, (float*)ws, M, N);
  LCV_LAUNCH_CHECK("dora_colscale_bwd");
  hipLaunchKernelGGL(dora_dm_reduce_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const float*)ws,
                     (const float*)wn, (float*)dm, slabs, N);
  LCV_LAUNCH_CHECK("dora_colscale_bwd (reduce)");
  return LCV_OK;
}

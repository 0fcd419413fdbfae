// LoRA dropout (include/lcv_hip_lora.h): the three places of a LoRALinear training step that touch the dropped input
// xd = bf16(x * mask * scale), plus the mask itself as bytes.
//   forward   h  = bf16(s * bf16(xd A^T))                     lora_down_dropout      (lcv_lora_down with the mask on x)
//   backward  dA = scale * g^T xd                             tn_skinny_dropout      (lcv_tn_skinny with the mask on x)
//             dx += mask * scale * (g A)                      lora_dx_dropout_add    (in place, after the dx GEMM)
// The mask is regenerated from (seed, offset, global element index) wherever it is needed (philox.h) and never stored: one
// Philox4x32-10 block per 8 elements, i.e. per 16-byte load of a lane.  All four kernels stream x / dx once and are
// HBM-bound; the generator costs ~70 integer VALU operations per 16 bytes.
// The down-projection and the contraction restate lora_down_kernel (gemm.hip) and tn_skinny_kernel (elementwise_bwd.hip)
// with the mask applied to the unpacked x values: same tiling, same summation order, same workspace layout.
// No atomics: the contraction always goes through per-row-group partials and a fixed-order reduce.
#include "lcv_common.h"
#include "philox.h"
#include "../../include/lcv_hip_lora.h"
#include <math.h>

struct drop_args {
  uint64_t seed, offset;
  int64_t row0;     // global index of the call's first row
  uint32_t T;       // keep iff half >= T
  float scale;      // 65536 / (65536 - T)
};

// the 8 values of one 16-byte piece of x at (global row, k): dropped and rescaled, rounded to bf16
__device__ __forceinline__ void drop8(const u16x8& raw, const drop_args& d, int64_t row, int64_t K, int64_t k, float (&f)[8]) {
  const unsigned keep = lora_keep8(d.seed, d.offset, ((uint64_t)(d.row0 + row) * (uint64_t)K + (uint64_t)k) >> 3, d.T);
#pragma unroll
  for (int e = 0; e < 8; ++e) f[e] = ((keep >> e) & 1u) ? bfround(bf2f(raw[e]) * d.scale) : 0.f;
}

// ---------------------------------------------------------------------------
// h[M, Rpad] = bf16(s * bf16(xd A^T)), zero padded.  One wave owns 4 rows (16 rows per workgroup), lanes sweep K in steps
// of 512 columns; every 16-byte piece of A is reused 4 times.
// ---------------------------------------------------------------------------
template <int RMAX>
__global__ __launch_bounds__(256) void lora_down_dropout_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ A,
                                                                bf16_t* __restrict__ hout, int64_t M, int K, int R, int Rpad,
                                                                int64_t ldx, float s, drop_args d) {
  const int lane = threadIdx.x & 63;
  const int64_t row0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 4;
  if (row0 >= M) return;
  int64_t rows[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) rows[i] = (row0 + i < M) ? row0 + i : M - 1;
  float acc[4][RMAX];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < RMAX; ++j) acc[i][j] = 0.f;
  for (int k = lane * 8; k < K; k += 512) {
    float xf[4][8];
#pragma unroll
    for (int i = 0; i < 4; ++i) drop8(*reinterpret_cast<const u16x8*>(x + rows[i] * ldx + k), d, rows[i], K, k, xf[i]);
#pragma unroll
    for (int j = 0; j < RMAX; ++j) {
      if (j < R) {
        float af[8];
        unpack8(*reinterpret_cast<const u16x8*>(A + (int64_t)j * K + k), af);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[i][j] += xf[i][e] * af[e];
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float mine = 0.f;  // lane j keeps column j
#pragma unroll
    for (int j = 0; j < RMAX; ++j) {
      if (j < R) {
        const float t = wave_sum(acc[i][j]);
        if (lane == j) mine = t;
      }
    }
    if (row0 + i < M && lane < Rpad) hout[(row0 + i) * Rpad + lane] = (lane < R) ? f2bf(s * bfround(mine)) : (bf16_t)0;
  }
}

// ---------------------------------------------------------------------------
// part[group][r][k] = sum over the group's rows of g[m, r] * xd[m, k]; out = scale * sum over groups, in group order.
// A workgroup owns 512 columns (4 waves x the same 64 lanes x 8 columns) and `rpb` rows; its 4 waves each take a quarter
// of those rows and their sums meet in LDS as ((w0 + w1) + w2) + w3.  8 ranks per launch.
// ---------------------------------------------------------------------------
#define TND_MAXROWS 1024
#define TND_RC 8
__global__ __launch_bounds__(256) void tn_skinny_dropout_kernel(const bf16_t* __restrict__ g, const bf16_t* __restrict__ x,
                                                                int64_t M, int64_t K, int R, int Rpad, int64_t ldx, int r0,
                                                                int rpb, float* __restrict__ part, drop_args d) {
  __shared__ float smem[3 * 64 * TND_RC * 8];             // 48 KB: first the g rows [rpb][RC], then 3 waves' partials
  static_assert(3 * 64 * TND_RC * 8 >= TND_MAXROWS * TND_RC, "LDS image too small for the g rows");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t m0 = (int64_t)blockIdx.y * rpb;
  const int64_t k = ((int64_t)blockIdx.x * 64 + lane) * 8;
  const int nrows = (int)((M - m0) < rpb ? (M - m0) : rpb);
  for (int i = threadIdx.x; i < rpb * TND_RC; i += 256) {
    const int m = i / TND_RC, rr = i - m * TND_RC;
    smem[i] = (m < nrows && r0 + rr < R) ? bf2f(g[(m0 + m) * Rpad + r0 + rr]) : 0.f;
  }
  __syncthreads();
  float acc[TND_RC][8];
#pragma unroll
  for (int rr = 0; rr < TND_RC; ++rr)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[rr][e] = 0.f;
  const int q = rpb / 4;                                   // rows per wave (rpb % 32 == 0: whole batches of 8, so a batch never
  const int mb = wave * q, me = min(mb + q, nrows);        // reaches into the next wave's rows; rows >= nrows have g = 0 in LDS)
  if (k < K && mb < me) {
    // two batches of 8 rows in flight: the loads of batch i+1 are issued before the generator and the FMAs of batch i
    auto load8 = [&](u16x8 (&raw)[8], int m) {
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int mm = m + u < nrows ? m + u : nrows - 1;  // clamped address; its weight in LDS is zero
        raw[u] = *reinterpret_cast<const u16x8*>(x + (m0 + mm) * ldx + k);
      }
    };
    auto fma8 = [&](const u16x8 (&raw)[8], int m) {
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int mm = m + u < nrows ? m + u : nrows - 1;
        float xf[8];
        drop8(raw[u], d, m0 + mm, K, k, xf);
        const f32x4 g0 = *reinterpret_cast<const f32x4*>(smem + (m + u) * TND_RC);
        const f32x4 g1 = *reinterpret_cast<const f32x4*>(smem + (m + u) * TND_RC + 4);
#pragma unroll
        for (int rr = 0; rr < TND_RC; ++rr) {
          const float gv = rr < 4 ? g0[rr & 3] : g1[rr & 3];
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[rr][e] = fmaf(gv, xf[e], acc[rr][e]);
        }
      }
    };
    u16x8 ra[8], rb[8];
    load8(ra, mb);
    for (int m = mb; m < me; m += 16) {
      if (m + 8 < me) load8(rb, m + 8);
      fma8(ra, m);
      if (m + 8 < me) {
        if (m + 16 < me) load8(ra, m + 16);
        fma8(rb, m + 8);
      }
    }
  }
  __syncthreads();                                         // every wave is done with the g rows
  if (wave > 0) {
    float* dst = smem + ((wave - 1) * 64 + lane) * TND_RC * 8;
#pragma unroll
    for (int rr = 0; rr < TND_RC; ++rr)
#pragma unroll
      for (int e = 0; e < 8; ++e) dst[rr * 8 + e] = acc[rr][e];
  }
  __syncthreads();
  if (wave == 0 && k < K) {
#pragma unroll
    for (int rr = 0; rr < TND_RC; ++rr) {
      if (r0 + rr < R) {
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          v[e] = acc[rr][e];
#pragma unroll
          for (int w2 = 0; w2 < 3; ++w2) v[e] += smem[(w2 * 64 + lane) * TND_RC * 8 + rr * 8 + e];
        }
        float* dst = part + ((int64_t)blockIdx.y * R + r0 + rr) * K + k;   // this row group's slice; 32-byte aligned
        *reinterpret_cast<f32x4*>(dst) = f32x4{v[0], v[1], v[2], v[3]};
        *reinterpret_cast<f32x4*>(dst + 4) = f32x4{v[4], v[5], v[6], v[7]};
      }
    }
  }
}

__global__ __launch_bounds__(256) void tn_skinny_dropout_reduce_kernel(const float* __restrict__ part, float* __restrict__ out,
                                                                       int64_t n, int groups, float scale) {
  const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= n) return;
  f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int g = 0; g < groups; ++g) acc += *reinterpret_cast<const f32x4*>(part + (int64_t)g * n + i);
  *reinterpret_cast<f32x4*>(out + i) = acc * scale;
}

// ---------------------------------------------------------------------------
// dx[m, k] = bf16(dx[m, k] + mask * scale * sum_r g[m, r] A[r, k]), in place.  One wave owns 4 rows x 512 columns (a
// workgroup: 16 rows); the rank is walked in steps of 8: one 16-byte broadcast load of g per row and step, one 16-byte
// load of A (L2-resident, <= 256 KB) per rank, reused by the 4 rows.  Each element is read and written by one lane.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lora_dx_dropout_add_kernel(bf16_t* __restrict__ dx, const bf16_t* __restrict__ g,
                                                                  const bf16_t* __restrict__ A, int64_t M, int K, int R,
                                                                  int64_t ldg, drop_args d) {
  const int lane = threadIdx.x & 63;
  const int64_t row0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 4;
  const int k = ((int)blockIdx.y * 64 + lane) * 8;
  if (row0 >= M || k >= K) return;
  int64_t rows[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) rows[i] = (row0 + i < M) ? row0 + i : M - 1;
  float acc[4][8];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[i][e] = 0.f;
  for (int rc = 0; rc < R; rc += 8) {                      // rc + 8 <= Rpad <= ldg (Rpad % 8 == 0)
    float gf[4][8];
#pragma unroll
    for (int i = 0; i < 4; ++i) unpack8(*reinterpret_cast<const u16x8*>(g + rows[i] * ldg + rc), gf[i]);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (rc + j < R) {
        float af[8];
        unpack8(*reinterpret_cast<const u16x8*>(A + (int64_t)(rc + j) * K + k), af);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int e = 0; e < 8; ++e) acc[i][e] += gf[i][j] * af[e];
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (row0 + i < M) {
      bf16_t* p = dx + (row0 + i) * K + k;
      const u16x8 raw = *reinterpret_cast<const u16x8*>(p);
      const unsigned keep =
          lora_keep8(d.seed, d.offset, ((uint64_t)(d.row0 + row0 + i) * (uint64_t)K + (uint64_t)k) >> 3, d.T);
      float o[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = bf2f(raw[e]) + (((keep >> e) & 1u) ? d.scale * acc[i][e] : 0.f);
      *reinterpret_cast<u16x8*>(p) = pack8(o);
    }
  }
}

// one thread per group of 8 elements: out is contiguous [M, K], so local group i is global group row0 * (K / 8) + i
__global__ __launch_bounds__(256) void lora_dropout_mask_kernel(uint8_t* __restrict__ out, int64_t groups, int64_t K8,
                                                                drop_args d) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= groups) return;
  const unsigned keep = lora_keep8(d.seed, d.offset, (uint64_t)d.row0 * (uint64_t)K8 + (uint64_t)i, d.T);
  u32x2 v;
  v[0] = (keep & 1u) | ((keep >> 1 & 1u) << 8) | ((keep >> 2 & 1u) << 16) | ((keep >> 3 & 1u) << 24);
  v[1] = (keep >> 4 & 1u) | ((keep >> 5 & 1u) << 8) | ((keep >> 6 & 1u) << 16) | ((keep >> 7 & 1u) << 24);
  *reinterpret_cast<u32x2*>(out + i * 8) = v;
}

// ---------------------------------------------------------------------------------------------------------------- host
// p in (0, 1) (NaN fails the test), rows [row0, row0 + M) x K within 63 bits
static bool drop_setup(double p, uint64_t seed, uint64_t offset, int64_t row0, int64_t M, int64_t K, drop_args* d) {
  if (!(p > 0.0 && p < 1.0) || row0 < 0 || M < 0 || K < 1) return false;
  if (row0 > INT64_MAX / K - M - 1) return false;
  long T = lrint(p * 65536.0);                             // round-half-even in the default rounding mode
  T = T < 1 ? 1 : (T > 65535 ? 65535 : T);
  d->seed = seed;
  d->offset = offset;
  d->row0 = row0;
  d->T = (uint32_t)T;
  d->scale = 65536.0f / (float)(65536 - T);
  return true;
}
#define DROP_SETUP(who)                                                                                               \
  drop_args d;                                                                                                        \
  LCV_CHECK_ARG(drop_setup(p, seed, offset, row0, M, K, &d), who ": p = %g outside (0, 1), or row0 = %ld / the shape " \
                "out of range", p, (long)row0)

extern "C" int lcv_lora_down_dropout(const void* x, const void* A, void* h, int64_t M, int64_t K, int64_t R, int64_t Rpad,
                                     int64_t ldx, float s, double p, uint64_t seed, uint64_t offset, int64_t row0,
                                     void* stream) {
  LCV_CHECK_ARG(x && A && h, "lora_down_dropout: null pointer");
  LCV_CHECK_ARG(R >= 1 && R <= 32 && Rpad >= R && Rpad <= 64, "lora_down_dropout: rank %ld unsupported (1..32, Rpad <= 64)", (long)R);
  LCV_CHECK_ARG(K >= 8 && K % 8 == 0 && ldx % 8 == 0 && ldx >= K && K <= INT32_MAX - 512,
                "lora_down_dropout: K and ldx must be multiples of 8, ldx >= K");
  DROP_SETUP("lora_down_dropout");
  if (M == 0) return LCV_OK;
  LCV_CHECK_ARG((M + 15) / 16 <= INT32_MAX, "lora_down_dropout: M = %ld too large", (long)M);
  const unsigned blocks = (unsigned)((M + 15) / 16);
  hipStream_t st = (hipStream_t)stream;
  if (R <= 8)
    hipLaunchKernelGGL(lora_down_dropout_kernel<8>, dim3(blocks), dim3(256), 0, st, (const bf16_t*)x, (const bf16_t*)A, (bf16_t*)h, M, (int)K, (int)R, (int)Rpad, ldx, s, d);
  else if (R <= 16)
    hipLaunchKernelGGL(lora_down_dropout_kernel<16>, dim3(blocks), dim3(256), 0, st, (const bf16_t*)x, (const bf16_t*)A, (bf16_t*)h, M, (int)K, (int)R, (int)Rpad, ldx, s, d);
  else
    hipLaunchKernelGGL(lora_down_dropout_kernel<32>, dim3(blocks), dim3(256), 0, st, (const bf16_t*)x, (const bf16_t*)A, (bf16_t*)h, M, (int)K, (int)R, (int)Rpad, ldx, s, d);
  LCV_LAUNCH_CHECK("lora_down_dropout");
  return LCV_OK;
}

// rows per workgroup, as lcv_tn_skinny: ~32 row groups per call, ~64 when there are few column blocks (K <= 4096)
static int64_t tnd_rpb(int64_t M, int64_t K) {
  const int64_t groups = (K + 511) / 512 <= 8 ? 64 : 32;
  int64_t rpb = ((M + groups - 1) / groups + 31) / 32 * 32;
  if (rpb > TND_MAXROWS) rpb = TND_MAXROWS;
  if (rpb < 64) rpb = 64;
  return rpb;
}

extern "C" int64_t lcv_tn_skinny_dropout_ws_bytes(int64_t M, int64_t K, int64_t R) {
  if (M <= 0 || K <= 0 || R <= 0) return 0;
  const int64_t rpb = tnd_rpb(M, K);
  return ((M + rpb - 1) / rpb) * R * K * 4;
}

extern "C" int lcv_tn_skinny_dropout(const void* g, const void* x, float* out, int64_t M, int64_t K, int64_t R, int64_t Rpad,
                                     int64_t ldx, float scale, double p, uint64_t seed, uint64_t offset, int64_t row0,
                                     float* ws, int64_t ws_bytes, void* stream) {
  LCV_CHECK_ARG(g && x && out, "tn_skinny_dropout: null pointer");
  LCV_CHECK_ARG(K >= 8 && K % 8 == 0 && ldx % 8 == 0 && ldx >= K && R >= 1 && R <= Rpad && R <= 65535,
                "tn_skinny_dropout: bad shape");
  DROP_SETUP("tn_skinny_dropout");
  if (M == 0) return LCV_OK;
  const int64_t rpb = tnd_rpb(M, K);
  const int64_t col_blocks = (K + 511) / 512, groups = (M + rpb - 1) / rpb;
  LCV_CHECK_ARG(col_blocks <= INT32_MAX && groups <= 65535, "tn_skinny_dropout: shape too large");
  const int64_t need = groups * R * K * 4;
  LCV_CHECK_ARG(ws && ws_bytes >= need && ((uintptr_t)ws % 16) == 0 && ((uintptr_t)out % 16) == 0,
                "tn_skinny_dropout: workspace of %ld bytes is missing, too small or misaligned (need %ld)", (long)ws_bytes,
                (long)need);
  const dim3 grid((unsigned)col_blocks, (unsigned)groups);
  for (int r0 = 0; r0 < R; r0 += TND_RC) {
    hipLaunchKernelGGL(tn_skinny_dropout_kernel, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)g, (const bf16_t*)x, M,
                       K, (int)R, (int)Rpad, ldx, r0, (int)rpb, ws, d);
    LCV_LAUNCH_CHECK("tn_skinny_dropout");
  }
  const int64_t n = R * K;   // K % 8 == 0: whole float4s
  LCV_CHECK_ARG((n / 4 + 255) / 256 <= INT32_MAX, "tn_skinny_dropout: shape too large");
  hipLaunchKernelGGL(tn_skinny_dropout_reduce_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     ws, out, n, (int)groups, scale);
  LCV_LAUNCH_CHECK("tn_skinny_dropout_reduce");
  return LCV_OK;
}

extern "C" int lcv_lora_dx_dropout_add(void* dx, const void* g, const void* A, int64_t M, int64_t K, int64_t R, int64_t Rpad,
                                       int64_t ldg, double p, uint64_t seed, uint64_t offset, int64_t row0, void* stream) {
  LCV_CHECK_ARG(dx && g && A, "lora_dx_dropout_add: null pointer");
  LCV_CHECK_ARG(R >= 1 && R <= 32 && Rpad >= R && Rpad % 8 == 0 && ldg >= Rpad && ldg % 8 == 0,
                "lora_dx_dropout_add: rank %ld / Rpad %ld / ldg %ld unsupported (R 1..32, Rpad and ldg multiples of 8)", (long)R,
                (long)Rpad, (long)ldg);
  LCV_CHECK_ARG(K >= 8 && K % 8 == 0 && (K + 511) / 512 <= 65535, "lora_dx_dropout_add: K must be a multiple of 8 (<= 65535 * 512)");
  DROP_SETUP("lora_dx_dropout_add");
  if (M == 0) return LCV_OK;
  LCV_CHECK_ARG((M + 15) / 16 <= INT32_MAX, "lora_dx_dropout_add: M = %ld too large", (long)M);
  const dim3 grid((unsigned)((M + 15) / 16), (unsigned)((K + 511) / 512));
  hipLaunchKernelGGL(lora_dx_dropout_add_kernel, grid, dim3(256), 0, (hipStream_t)stream, (bf16_t*)dx, (const bf16_t*)g,
                     (const bf16_t*)A, M, (int)K, (int)R, ldg, d);
  LCV_LAUNCH_CHECK("lora_dx_dropout_add");
  return LCV_OK;
}

extern "C" int lcv_lora_dropout_mask(void* out_u8, int64_t M, int64_t K, double p, uint64_t seed, uint64_t offset,
                                     int64_t row0, void* stream) {
  LCV_CHECK_ARG(out_u8 && ((uintptr_t)out_u8 % 8) == 0, "lora_dropout_mask: null or misaligned pointer");
  LCV_CHECK_ARG(K >= 8 && K % 8 == 0, "lora_dropout_mask: K must be a multiple of 8");
  DROP_SETUP("lora_dropout_mask");
  if (M == 0) return LCV_OK;
  const int64_t groups = M * (K / 8);
  LCV_CHECK_ARG((groups + 255) / 256 <= INT32_MAX, "lora_dropout_mask: shape too large");
  hipLaunchKernelGGL(lora_dropout_mask_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (uint8_t*)out_u8, groups, K / 8, d);
  LCV_LAUNCH_CHECK("lora_dropout_mask");
  return LCV_OK;
}

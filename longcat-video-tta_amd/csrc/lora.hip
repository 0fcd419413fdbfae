// The LoRA adapter kernels: the three places of a LoRALinear step that stream x or dy against a rank-r matrix, each in its
// plain form (include/lcv_hip.h) and with the dropout mask on x (include/lcv_hip_lora.h), plus the mask itself as bytes.
//   forward   h  = bf16(s * bf16(x A^T))        lora_down_kernel<RMAX, D...>     lcv_lora_down / lcv_lora_down_dropout
//   backward  dA = scale * g^T x                tn_skinny_kernel<RC, D...>       lcv_tn_skinny / lcv_tn_skinny_dropout
//             dx += mask * scale * (g A)        lora_dx_dropout_add_kernel       (in place, after the dx GEMM; masked only)
// One definition per kernel.  The trailing parameter pack D is empty for the plain form and holds one drop_args for the masked
// one; the only place the two forms differ is x8(), the 8 values a lane makes of one 16-byte piece of x: the values
// themselves, or xd = bf16(x * mask * scale).  An empty pack leaves the plain kernel's signature - its kernarg segment - as
// it is.  Tiling, summation order and workspace layout are therefore the same in both forms: the masked kernel on x gives
// the bits of the plain kernel on xd.
// The mask is regenerated from (seed, offset, global element index) wherever it is needed (philox.h) and never stored: one
// Philox4x32-10 block per 8 elements, i.e. per 16-byte load of a lane.  All kernels stream x / dx once and are HBM-bound;
// the generator costs ~70 integer VALU operations per 16 bytes.
// Atomics: only tn_skinny_publish_atomic, which only the plain contraction without a workspace (ws == NULL) calls.  A masked
// contraction always goes through per-row-group partials and the fixed-order reduce.
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

// the 8 values of one 16-byte piece of x at (global row, k) ...
__device__ __forceinline__ void x8(const u16x8& raw, int64_t, int64_t, int64_t, float (&f)[8]) { unpack8(raw, f); }
// ... and with a mask: dropped and rescaled, rounded to bf16
__device__ __forceinline__ void x8(const u16x8& raw, int64_t row, int64_t K, int64_t k, float (&f)[8], const drop_args& d) {
  const unsigned keep = lora_keep8(d.seed, d.offset, ((uint64_t)(d.row0 + row) * (uint64_t)K + (uint64_t)k) >> 3, d.T);
#pragma unroll
  for (int e = 0; e < 8; ++e) f[e] = ((keep >> e) & 1u) ? bfround(bf2f(raw[e]) * d.scale) : 0.f;
}

// ---------------------------------------------------------------------------
// LoRA down-projection: h[M, Rpad] = bf16(s * bf16(x[M, K] A[R, K]^T)), zero padded to Rpad columns.
// Also serves the backward g = s * dy B (x := dy, A := B^T).  HBM-bound on x (rank r flop/B): one wave owns
// 4 rows (16 rows per workgroup), lanes sweep K in steps of 512 columns, so every 16-byte piece of A (L1/L2-resident,
// <= 800 KB) is reused 4 times.
// ---------------------------------------------------------------------------
template <int RMAX, class... D>
__global__ __launch_bounds__(256) void lora_down_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ A,
                                                        bf16_t* __restrict__ hout, int64_t M, int K, int R, int Rpad,
                                                        int64_t ldx, float s, D... d) {
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
    for (int i = 0; i < 4; ++i) x8(*reinterpret_cast<const u16x8*>(x + rows[i] * ldx + k), rows[i], K, k, xf[i], d...);
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
// Skinny token contraction for the LoRA parameter gradients:
//   out[r, k] = scale * sum_m g[m, r] * x[m, k]      (g: [M, Rpad] bf16, x: [M, K] bf16, out: [R, K] fp32)
// dA = (s dy B)^T x  and  dB^T = h^T dy  are both of this form.  HBM-bound on x (read once per 8 ranks).
// Layout: a workgroup owns 512 columns (4 waves x the SAME 64 lanes x 8 columns) and `rpb` rows; its 4 waves each take a
// quarter of those rows, their partial sums meet in LDS as ((w0 + w1) + w2) + w3 and ONE wave publishes them: into this row
// group's slice of `part` (summed in group order by tn_skinny_reduce_kernel), or, without a workspace, with fp32 atomics
// into a zero-filled `out`.  The atomics are the cross-workgroup part of the reduction and were the bound of the first
// version (one set per 128 rows: 6.4 M atomics per call at 25 200 tokens, ~1 TB/s); with ~32 row groups per call they are
// 1 M and the kernel streams x.
// ---------------------------------------------------------------------------
#define TN_MAXROWS 1024

// the ws == NULL publish of the plain contraction: the only atomics of this file
__device__ __forceinline__ void tn_skinny_publish_atomic(float* out, float v) { atomicAdd(out, v); }

template <int RC, class... D>
__global__ __launch_bounds__(256) void tn_skinny_kernel(const bf16_t* __restrict__ g, const bf16_t* __restrict__ x,
                                                        float* __restrict__ out, int64_t M, int64_t K, int R,
                                                        int Rpad, int64_t ldx, int r0, float scale, int rpb,
                                                        float* __restrict__ part, D... d) {
  __shared__ float smem[3 * 64 * RC * 8];                 // 48 KB: first the g rows [rpb][RC], then 3 waves' partials
  static_assert(3 * 64 * RC * 8 >= TN_MAXROWS * RC, "LDS image too small for the g rows");
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t m0 = (int64_t)blockIdx.y * rpb;
  const int64_t k = ((int64_t)blockIdx.x * 64 + lane) * 8;
  const int nrows = (int)((M - m0) < rpb ? (M - m0) : rpb);
  for (int i = threadIdx.x; i < rpb * RC; i += 256) {
    const int m = i / RC, rr = i - m * RC;
    smem[i] = (m < nrows && r0 + rr < R) ? bf2f(g[(m0 + m) * Rpad + r0 + rr]) : 0.f;
  }
  __syncthreads();
  typedef __attribute__((ext_vector_type(2))) float f32x2;
  f32x2 acc[RC][4];                                        // packed pairs of columns: v_pk_fma_f32 (32 per row instead of 64)
#pragma unroll
  for (int rr = 0; rr < RC; ++rr)
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[rr][e] = f32x2{0.f, 0.f};
  const int q = rpb / 4;                                   // rows per wave (rpb % 32 == 0: whole batches of 8, so a batch never
  const int mb = wave * q, me = min(mb + q, nrows);        // reaches into the next wave's rows; rows >= nrows have g = 0 in LDS)
  if (k < K && mb < me) {
    // Two batches of 8 rows in flight: the loads of batch i+1 are issued before the FMAs (and the generator) of batch i
    // (with one wave per SIMD and load -> wait -> compute the kernel sat at ~1 TB/s: nothing was in flight while a wave
    // computed).
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
        const int mm = m + u < nrows ? m + u : nrows - 1;  // the row that was loaded: the mask is the one of its index
        float xs[8];
        x8(raw[u], m0 + mm, K, k, xs, d...);
        f32x2 xf[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) xf[e] = f32x2{xs[2 * e], xs[2 * e + 1]};
        static_assert(RC == 8, "the g row is read as two float4");
        const f32x4 g0 = *reinterpret_cast<const f32x4*>(smem + (m + u) * RC);
        const f32x4 g1 = *reinterpret_cast<const f32x4*>(smem + (m + u) * RC + 4);
#pragma unroll
        for (int rr = 0; rr < RC; ++rr) {
          const float gv = rr < 4 ? g0[rr & 3] : g1[rr & 3];
          const f32x2 gvv = f32x2{gv, gv};
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[rr][e] = __builtin_elementwise_fma(gvv, xf[e], acc[rr][e]);
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
    float* dst = smem + ((wave - 1) * 64 + lane) * RC * 8;
#pragma unroll
    for (int rr = 0; rr < RC; ++rr)
#pragma unroll
      for (int e = 0; e < 8; ++e) dst[rr * 8 + e] = acc[rr][e >> 1][e & 1];
  }
  __syncthreads();
  if (wave == 0 && k < K) {
#pragma unroll
    for (int rr = 0; rr < RC; ++rr) {
      if (r0 + rr < R) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          float v = acc[rr][e >> 1][e & 1];
#pragma unroll
          for (int w2 = 0; w2 < 3; ++w2) v += smem[(w2 * 64 + lane) * RC * 8 + rr * 8 + e];
          if (sizeof...(D) > 0 || part) part[((int64_t)blockIdx.y * R + r0 + rr) * K + k + e] = v;   // this row group's slice
          else if constexpr (sizeof...(D) == 0)            // no mask: a call without a workspace publishes with atomics
            tn_skinny_publish_atomic(out + (int64_t)(r0 + rr) * K + k + e, v * scale);
        }
      }
    }
  }
}

// out[r, k] = scale * sum over row groups of part[group][r][k]: a fixed order (bit-reproducible, unlike the atomics), no
// zero-fill of `out`, and 64 x fewer L2 atomics - with ~64 row groups the atomics were the larger half of the kernel's time
__global__ __launch_bounds__(256) void tn_skinny_reduce_kernel(const float* __restrict__ part, float* __restrict__ out,
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
static const char* const DROP_REFUSED = "%s: p = %g outside (0, 1), or row0 = %ld / the shape out of range";

// the rank-to-template dispatch of both down-projections; `d` is empty or one drop_args
template <class... D>
static void lora_down_launch(const void* x, const void* A, void* h, int64_t M, int64_t K, int64_t R, int64_t Rpad, int64_t ldx,
                             float s, void* stream, D... d) {
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)((M + 15) / 16)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x,
                       (const bf16_t*)A, (bf16_t*)h, M, (int)K, (int)R, (int)Rpad, ldx, s, d...);
  };
  if (R <= 8) go(lora_down_kernel<8, D...>);
  else if (R <= 16) go(lora_down_kernel<16, D...>);
  else go(lora_down_kernel<32, D...>);
}

extern "C" int lcv_lora_down(const void* x, const void* A, void* h, int64_t M, int64_t K, int64_t R,
                             int64_t Rpad, int64_t ldx, float s, void* stream) {
  LCV_CHECK_ARG(x && A && h, "lora_down: null pointer");
  LCV_CHECK_ARG(R >= 1 && R <= 32 && Rpad >= R && Rpad <= 64, "lora_down: rank %ld unsupported (1..32, Rpad <= 64)", (long)R);
  LCV_CHECK_ARG(K % 8 == 0 && ldx % 8 == 0, "lora_down: K and ldx must be multiples of 8");
  if (M == 0) return LCV_OK;
  lora_down_launch(x, A, h, M, K, R, Rpad, ldx, s, stream);
  LCV_LAUNCH_CHECK("lora_down");
  return LCV_OK;
}

extern "C" int lcv_lora_down_dropout(const void* x, const void* A, void* h, int64_t M, int64_t K, int64_t R, int64_t Rpad,
                                     int64_t ldx, float s, double p, uint64_t seed, uint64_t offset, int64_t row0,
                                     void* stream) {
  LCV_CHECK_ARG(x && A && h, "lora_down_dropout: null pointer");
  LCV_CHECK_ARG(R >= 1 && R <= 32 && Rpad >= R && Rpad <= 64, "lora_down_dropout: rank %ld unsupported (1..32, Rpad <= 64)", (long)R);
  LCV_CHECK_ARG(K >= 8 && K % 8 == 0 && ldx % 8 == 0 && ldx >= K && K <= INT32_MAX - 512,
                "lora_down_dropout: K and ldx must be multiples of 8, ldx >= K");
  drop_args d;
  LCV_CHECK_ARG(drop_setup(p, seed, offset, row0, M, K, &d), DROP_REFUSED, "lora_down_dropout", p, (long)row0);
  if (M == 0) return LCV_OK;
  LCV_CHECK_ARG((M + 15) / 16 <= INT32_MAX, "lora_down_dropout: M = %ld too large", (long)M);
  lora_down_launch(x, A, h, M, K, R, Rpad, ldx, s, stream, d);
  LCV_LAUNCH_CHECK("lora_down_dropout");
  return LCV_OK;
}

// rows per workgroup: ~32 row groups per call; ~64 when there are few column blocks (K <= 4096: 8), so that two workgroups share a CU
static int64_t tn_skinny_rpb(int64_t M, int64_t K) {
  const int64_t groups = (K + 511) / 512 <= 8 ? 64 : 32;
  int64_t rpb = ((M + groups - 1) / groups + 31) / 32 * 32;
  if (rpb > TN_MAXROWS) rpb = TN_MAXROWS;
  if (rpb < 64) rpb = 64;
  return rpb;
}

extern "C" int64_t lcv_tn_skinny_ws_bytes(int64_t M, int64_t K, int64_t R) {
  const int64_t rpb = tn_skinny_rpb(M, K);
  return ((M + rpb - 1) / rpb) * R * K * 4;
}

extern "C" int64_t lcv_tn_skinny_dropout_ws_bytes(int64_t M, int64_t K, int64_t R) {
  return (M <= 0 || K <= 0 || R <= 0) ? 0 : lcv_tn_skinny_ws_bytes(M, K, R);
}

// the launches of both contractions: 8 ranks at a time, then (with partials) the reduce; `who` names the caller in a launch
// error, `d` is empty or one drop_args
template <class... D>
static int tn_skinny_launch(const char* who, const char* who_reduce, const void* g, const void* x, float* out, int64_t M,
                            int64_t K, int64_t R, int64_t Rpad, int64_t ldx, float scale, float* part, void* stream, D... d) {
  const int64_t rpb = tn_skinny_rpb(M, K);
  const dim3 grid((unsigned)((K + 511) / 512), (unsigned)((M + rpb - 1) / rpb));
  for (int r0 = 0; r0 < R; r0 += 8) {
    hipLaunchKernelGGL((tn_skinny_kernel<8, D...>), grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)g,
                       (const bf16_t*)x, out, M, K, (int)R, (int)Rpad, ldx, r0, scale, (int)rpb, part, d...);
    LCV_LAUNCH_CHECK(who);
  }
  if (part) {
    const int64_t n = R * K;   // K % 8 == 0: whole float4s
    hipLaunchKernelGGL(tn_skinny_reduce_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, part,
                       out, n, (int)grid.y, scale);
    LCV_LAUNCH_CHECK(who_reduce);
  }
  return LCV_OK;
}

extern "C" int lcv_tn_skinny(const void* g, const void* x, float* out, int64_t M, int64_t K, int64_t R,
                             int64_t Rpad, int64_t ldx, float scale, float* ws, int64_t ws_bytes, void* stream) {
  LCV_CHECK_ARG(g && x && out, "tn_skinny: null pointer");
  LCV_CHECK_ARG(K % 8 == 0 && ldx % 8 == 0 && R >= 1 && R <= Rpad, "tn_skinny: bad shape");
  if (M == 0) return LCV_OK;
  // with a workspace of >= lcv_tn_skinny_ws_bytes(M, K, R): per-group partial sums + a fixed-order reduction (`out` need not
  // be zeroed and is overwritten); without: fp32 atomics into a zero-filled `out`
  const int64_t need = lcv_tn_skinny_ws_bytes(M, K, R);
  float* part = (ws && ws_bytes >= need && ((uintptr_t)ws % 16) == 0) ? ws : nullptr;
  LCV_CHECK_ARG(ws == nullptr || part != nullptr, "tn_skinny: workspace of %ld bytes is too small or misaligned (need %ld)",
                (long)ws_bytes, (long)need);
  return tn_skinny_launch("tn_skinny", "tn_skinny_reduce", g, x, out, M, K, R, Rpad, ldx, scale, part, stream);
}

extern "C" int lcv_tn_skinny_dropout(const void* g, const void* x, float* out, int64_t M, int64_t K, int64_t R, int64_t Rpad,
                                     int64_t ldx, float scale, double p, uint64_t seed, uint64_t offset, int64_t row0,
                                     float* ws, int64_t ws_bytes, void* stream) {
  LCV_CHECK_ARG(g && x && out, "tn_skinny_dropout: null pointer");
  LCV_CHECK_ARG(K >= 8 && K % 8 == 0 && ldx % 8 == 0 && ldx >= K && R >= 1 && R <= Rpad && R <= 65535,
                "tn_skinny_dropout: bad shape");
  drop_args d;
  LCV_CHECK_ARG(drop_setup(p, seed, offset, row0, M, K, &d), DROP_REFUSED, "tn_skinny_dropout", p, (long)row0);
  if (M == 0) return LCV_OK;
  const int64_t rpb = tn_skinny_rpb(M, K);
  LCV_CHECK_ARG((K + 511) / 512 <= INT32_MAX && (M + rpb - 1) / rpb <= 65535, "tn_skinny_dropout: shape too large");
  const int64_t need = lcv_tn_skinny_ws_bytes(M, K, R);
  LCV_CHECK_ARG(ws && ws_bytes >= need && ((uintptr_t)ws % 16) == 0 && ((uintptr_t)out % 16) == 0,
                "tn_skinny_dropout: workspace of %ld bytes is missing, too small or misaligned (need %ld)", (long)ws_bytes,
                (long)need);
  LCV_CHECK_ARG((R * K / 4 + 255) / 256 <= INT32_MAX, "tn_skinny_dropout: shape too large");
  return tn_skinny_launch("tn_skinny_dropout", "tn_skinny_dropout_reduce", g, x, out, M, K, R, Rpad, ldx, scale, ws, stream, d);
}

extern "C" int lcv_lora_dx_dropout_add(void* dx, const void* g, const void* A, int64_t M, int64_t K, int64_t R, int64_t Rpad,
                                       int64_t ldg, double p, uint64_t seed, uint64_t offset, int64_t row0, void* stream) {
  LCV_CHECK_ARG(dx && g && A, "lora_dx_dropout_add: null pointer");
  LCV_CHECK_ARG(R >= 1 && R <= 32 && Rpad >= R && Rpad % 8 == 0 && ldg >= Rpad && ldg % 8 == 0,
                "lora_dx_dropout_add: rank %ld / Rpad %ld / ldg %ld unsupported (R 1..32, Rpad and ldg multiples of 8)", (long)R,
                (long)Rpad, (long)ldg);
  LCV_CHECK_ARG(K >= 8 && K % 8 == 0 && (K + 511) / 512 <= 65535, "lora_dx_dropout_add: K must be a multiple of 8 (<= 65535 * 512)");
  drop_args d;
  LCV_CHECK_ARG(drop_setup(p, seed, offset, row0, M, K, &d), DROP_REFUSED, "lora_dx_dropout_add", p, (long)row0);
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
  drop_args d;
  LCV_CHECK_ARG(drop_setup(p, seed, offset, row0, M, K, &d), DROP_REFUSED, "lora_dropout_mask", p, (long)row0);
  if (M == 0) return LCV_OK;
  const int64_t groups = M * (K / 8);
  LCV_CHECK_ARG((groups + 255) / 256 <= INT32_MAX, "lora_dropout_mask: shape too large");
  hipLaunchKernelGGL(lora_dropout_mask_kernel, dim3((unsigned)((groups + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     (uint8_t*)out_u8, groups, K / 8, d);
  LCV_LAUNCH_CHECK("lora_dropout_mask");
  return LCV_OK;
}

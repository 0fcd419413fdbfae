// Fixed-order forms of the reductions that the default backward / optimizer kernels finish with fp32 atomics
// (include/lcv_hip_det.h): the AdaLN / LayerNorm parameter gradients, dgate, the q/k norm-weight gradients, the small-M
// linear's input gradient and the per-tensor sums of squares of the gradient-norm clip.
//
// Row math: the gate, q/k-norm and grad-norm kernels below call the functions their counterparts of elementwise_bwd.hip /
// optim.hip call (bwd_rows.h: gate_bwd_row, qknorm_rope_bwd_token / qknorm_dw_stage; optim_common.h: grad_chunk_sumsq), and
// the SiLU derivative and the clip coefficient ARE the default kernels (silu_grad_launch, clip_coef_launch).  The rownorm and
// small-M kernels restate their counterparts operation for operation (same loads, same wave_sum use, same dres add): shared
// functions cost those four a measurable ~1 % (profiles/bwd_rows.md).  Either way dx / dy / dq_in / dk_in carry the same
// bits, and only where a sum leaves the thread differs.
// Nothing here uses a float read-modify-write that another thread can interleave with, in global memory or LDS.
//
// Summation order (the output is a pure function of the inputs and the shapes):
//   rownorm (AdaLN, LayerNorm affine)  a workgroup owns DET_ROWNORM_RPB consecutive rows OF ONE FRAME; wave w takes rows
//       w, w+4, w+8, ... of them and adds each channel's terms in that row order in a register; the four waves' sums go
//       to separate LDS rows and wave 0 adds them as ((w0 + w1) + w2) + w3; the workgroup's sums are one row of the
//       workspace [frames * bpf][2][C]; colsum adds a frame's bpf rows in index order and adds the result to the output.
//   gate       thread t owns packets t, t+256 of every row of its workgroup's DET_GATE_RPB rows of one frame (fma in row
//       order); workspace [frames * bpf][C]; colsum over a frame's rows in index order.
//   q/k norm   one workgroup per token: heads in steps of 16 per thread, shfl_xor 16 then 32, the four waves through LDS
//       as w0 + w1 + w2 + w3; workspace [B * N][256] (dwq | dwk); colsum over groups of DET_QK_GROUP consecutive tokens in
//       index order (in place, into the group's first row), then over the groups in index order.
//   small-M linear   per 256-row slab of W as in the default kernel; workspace [slabs][M][K]; colsum over slabs in index order.
//   grad norm  one partial per 2 048-element chunk (fma chain per thread, wave_sum, w0 + w1 + w2 + w3); per tensor one
//       workgroup: thread t adds chunks t, t+256, ... in that order, then wave_sum and w0 + w1 + w2 + w3.
#include "bwd_rows.h"
#include "optim_common.h"
#include "../../include/lcv_hip_det.h"

#define DET_ROWNORM_RPB 64   // rows per workgroup: 2*C floats of workspace per 64 rows of C bf16 = 1/16 of x's bytes
#define DET_GATE_RPB 32      // C floats per 32 rows = 1/16 of y's bytes
#define DET_QK_GROUP 160     // ~sqrt(25 200): tokens per first-level group of the norm-weight sums

// out[g * out_gstride + w] (+)= sum over p in [0, np) of part[(g * P + p) * pstride + w], p ascending, np = min(P, total - g*P).
// One thread per (g, w).  `out` may be the group's own first row (the thread reads its column before it writes).
__global__ __launch_bounds__(256) void det_colsum_kernel(const float* part, int64_t total, int P, int64_t pstride, int W,
                                                         float* out, int64_t out_gstride, int accumulate) {
  const int w = blockIdx.y * 256 + threadIdx.x;
  if (w >= W) return;
  const int64_t g = blockIdx.x;
  const int64_t p0 = g * P;
  const int np = (int)((total - p0) < P ? (total - p0) : P);
  const float* src = part + p0 * pstride + w;
  float acc = 0.f;
#pragma unroll 8   // eight loads in flight, added in index order
  for (int p = 0; p < np; ++p) acc += src[(int64_t)p * pstride];
  float* o = out + g * out_gstride + w;
  *o = accumulate ? *o + acc : acc;
}

static int det_colsum(const float* part, int64_t total, int64_t P, int64_t pstride, int64_t W, float* out,
                      int64_t out_gstride, int accumulate, hipStream_t s, const char* name) {
  const int64_t groups = (total + P - 1) / P;
  hipLaunchKernelGGL(det_colsum_kernel, dim3((unsigned)groups, (unsigned)((W + 255) / 256)), dim3(256), 0, s, part, total,
                     (int)P, pstride, (int)W, out, out_gstride, accumulate);
  LCV_LAUNCH_CHECK(name);
  return LCV_OK;
}

// ---------------------------------------------------------------------------
// LayerNorm backward, one wave per row (rownorm_bwd_kernel with the sums kept per wave).
//   MODE 0 (AdaLN): g = dy*(1+scale) ; dshift += dy ; dscale += dy*xh        MODE 1 (affine): g = dy*w ; db += dy ; dw += dy*xh
// blockIdx.x = frame * bpf + j: rows [frame*S + j*RPB, min(.. + RPB, (frame+1)*S)).  The accumulating wave holds
// 8 x ROWNORM_MAXCH x 2 sums per lane next to the row's 2 x 64 values: one wave per SIMD (launch bounds 256), no scratch.
// ---------------------------------------------------------------------------
template <int MODE>
__global__ __launch_bounds__(256) void rownorm_bwd_det_kernel(
    const bf16_t* __restrict__ x, const float* __restrict__ p_mul, const bf16_t* __restrict__ dy,
    bf16_t* __restrict__ dx, float* __restrict__ part, int C, int64_t S, int bpf, int64_t mod_stride, float eps,
    const bf16_t* __restrict__ dres) {
  __shared__ __attribute__((aligned(16))) float s_row[3][ROWNORM_MAXCH * 64 * 8];   // waves 1..3, one kind of sum at a time
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t frame = blockIdx.x / bpf;
  const int64_t lo = frame * S + (int64_t)(blockIdx.x - frame * bpf) * DET_ROWNORM_RPB;
  const int64_t hi = (lo + DET_ROWNORM_RPB < (frame + 1) * S) ? lo + DET_ROWNORM_RPB : (frame + 1) * S;
  const float* pm = p_mul + frame * mod_stride;
  float a_add[ROWNORM_MAXCH][8], a_mul[ROWNORM_MAXCH][8];
#pragma unroll
  for (int ch = 0; ch < ROWNORM_MAXCH; ++ch)
#pragma unroll
    for (int i = 0; i < 8; ++i) { a_add[ch][i] = 0.f; a_mul[ch][i] = 0.f; }
  for (int it = 0; it < DET_ROWNORM_RPB; it += 4) {
    const int64_t row = lo + it + wave;
    if (row >= hi) continue;
    const bf16_t* xr = x + row * C;
    const bf16_t* gr = dy + row * C;
    float v[ROWNORM_MAXCH][8], g[ROWNORM_MAXCH][8];
    float sum = 0.f;
#pragma unroll
    for (int ch = 0; ch < ROWNORM_MAXCH; ++ch) {
      const int c = (ch * 64 + lane) * 8;
      if (c < C) {
        unpack8(*reinterpret_cast<const u16x8*>(xr + c), v[ch]);
        unpack8(*reinterpret_cast<const u16x8*>(gr + c), g[ch]);
#pragma unroll
        for (int i = 0; i < 8; ++i) sum += v[ch][i];
      } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) { v[ch][i] = 0.f; g[ch][i] = 0.f; }
      }
    }
    const float mean = wave_sum(sum) / (float)C;
    float sq = 0.f;
#pragma unroll
    for (int ch = 0; ch < ROWNORM_MAXCH; ++ch) {
      const int c = (ch * 64 + lane) * 8;
      if (c < C) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float d = v[ch][i] - mean;
          sq += d * d;
        }
      }
    }
    const float rstd = rsqrtf(wave_sum(sq) / (float)C + eps);
    float sg = 0.f, sgx = 0.f;
#pragma unroll
    for (int ch = 0; ch < ROWNORM_MAXCH; ++ch) {
      const int c = (ch * 64 + lane) * 8;
      if (c < C) {
        const f32x4 m0 = *reinterpret_cast<const f32x4*>(pm + c);
        const f32x4 m1 = *reinterpret_cast<const f32x4*>(pm + c + 4);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float xh = (v[ch][i] - mean) * rstd;
          const float dyv = g[ch][i];
          a_add[ch][i] += dyv;              // parameter / modulation gradients: this wave's rows, in row order
          a_mul[ch][i] += dyv * xh;
          const float mul = ((i < 4) ? m0[i] : m1[i - 4]) + ((MODE == 0) ? 1.0f : 0.0f);
          const float gg = dyv * mul;
          v[ch][i] = xh;
          g[ch][i] = gg;
          sg += gg;
          sgx += gg * xh;
        }
      }
    }
    const float mg = wave_sum(sg) / (float)C;
    const float mgx = wave_sum(sgx) / (float)C;
    bf16_t* dr = dx + row * C;
#pragma unroll
    for (int ch = 0; ch < ROWNORM_MAXCH; ++ch) {
      const int c = (ch * 64 + lane) * 8;
      if (c < C) {
        float o[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] = rstd * (g[ch][i] - mg - v[ch][i] * mgx);
        if (dres) {   // the gradient that reaches x through the residual path of the same block, summed here in fp32
          float rr[8];
          unpack8(*reinterpret_cast<const u16x8*>(dres + row * C + c), rr);
#pragma unroll
          for (int i = 0; i < 8; ++i) o[i] += rr[i];
        }
        *reinterpret_cast<u16x8*>(dr + c) = pack8(o);
      }
    }
  }
  // the four waves' sums: waves 1..3 to their own LDS row, wave 0 adds them in wave order and writes the workgroup's row
  float* prow = part + (int64_t)blockIdx.x * 2 * C;
  auto combine = [&](float (&acc)[ROWNORM_MAXCH][8], float* dst) {
    if (wave > 0) {
#pragma unroll
      for (int ch = 0; ch < ROWNORM_MAXCH; ++ch) {
        const int c = (ch * 64 + lane) * 8;
        if (c < C) {
          *reinterpret_cast<f32x4*>(&s_row[wave - 1][c]) = f32x4{acc[ch][0], acc[ch][1], acc[ch][2], acc[ch][3]};
          *reinterpret_cast<f32x4*>(&s_row[wave - 1][c + 4]) = f32x4{acc[ch][4], acc[ch][5], acc[ch][6], acc[ch][7]};
        }
      }
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int ch = 0; ch < ROWNORM_MAXCH; ++ch) {
        const int c = (ch * 64 + lane) * 8;
        if (c < C) {
          f32x4 t0 = f32x4{acc[ch][0], acc[ch][1], acc[ch][2], acc[ch][3]};
          f32x4 t1 = f32x4{acc[ch][4], acc[ch][5], acc[ch][6], acc[ch][7]};
#pragma unroll
          for (int w2 = 0; w2 < 3; ++w2) {
            t0 += *reinterpret_cast<const f32x4*>(&s_row[w2][c]);
            t1 += *reinterpret_cast<const f32x4*>(&s_row[w2][c + 4]);
          }
          *reinterpret_cast<f32x4*>(dst + c) = t0;
          *reinterpret_cast<f32x4*>(dst + c + 4) = t1;
        }
      }
    }
    __syncthreads();
  };
  combine(a_add, prow);
  combine(a_mul, prow + C);
}

static bool det_ws_ok(const void* ws, int64_t ws_bytes, int64_t need) {
  return ws != nullptr && ws_bytes >= need && ((uintptr_t)ws % 16) == 0;
}

extern "C" int64_t lcv_det_ws_bytes(int kind, int64_t d0, int64_t d1, int64_t d2) {
  switch (kind) {
    case LCV_DET_ADALN:      // frames, S, C
      return (d0 <= 0 || d1 <= 0 || d2 <= 0) ? 0 : d0 * ((d1 + DET_ROWNORM_RPB - 1) / DET_ROWNORM_RPB) * 2 * d2 * 4;
    case LCV_DET_LAYERNORM:  // rows, C
      return (d0 <= 0 || d1 <= 0) ? 0 : ((d0 + DET_ROWNORM_RPB - 1) / DET_ROWNORM_RPB) * 2 * d1 * 4;
    case LCV_DET_GATE:       // frames, S, C
      return (d0 <= 0 || d1 <= 0 || d2 <= 0) ? 0 : d0 * ((d1 + DET_GATE_RPB - 1) / DET_GATE_RPB) * d2 * 4;
    case LCV_DET_QKNORM:     // B, N
      return (d0 <= 0 || d1 <= 0) ? 0 : d0 * d1 * 256 * 4;
    case LCV_DET_SMALLM:     // M, N, K
      return (d0 <= 0 || d1 <= 0 || d2 <= 0) ? 0 : ((d1 + 255) / 256) * d0 * d2 * 4;
    case LCV_DET_GRAD_NORM:  // total_chunks
      return d0 <= 0 ? 0 : d0 * 4;
    default:
      return -1;
  }
}

extern "C" int lcv_det_adaln_modulate_bwd(const void* x, const float* mod, const void* dy, void* dx, float* dmod,
                                          int64_t B, int64_t T, int64_t S, int64_t C, int64_t mod_stride,
                                          int64_t shift_off, int64_t scale_off, float eps, const void* dres, void* ws,
                                          int64_t ws_bytes, void* stream) {
  if (!dmod)   // nothing to reduce: the default kernel has no order-dependent sum on this path
    return lcv_adaln_modulate_bwd(x, mod, dy, dx, nullptr, B, T, S, C, mod_stride, shift_off, scale_off, eps, dres, stream);
  LCV_CHECK_ARG(x && mod && dy && dx, "det_adaln_modulate_bwd: null pointer");
  LCV_CHECK_ARG(C > 0 && C % 8 == 0 && C <= 4096, "det_adaln_modulate_bwd: C must be a multiple of 8 and <= 4096");
  LCV_CHECK_ARG(scale_off % 4 == 0 && mod_stride % 4 == 0, "det_adaln_modulate_bwd: scale_off and mod_stride must be multiples of 4");
  const int64_t frames = B * T;
  if (frames * S == 0) return LCV_OK;
  const int64_t bpf = (S + DET_ROWNORM_RPB - 1) / DET_ROWNORM_RPB;
  const int64_t need = lcv_det_ws_bytes(LCV_DET_ADALN, frames, S, C);
  LCV_CHECK_ARG(frames * bpf <= 0x7fffffff, "det_adaln_modulate_bwd: too many workgroups");
  LCV_CHECK_ARG(det_ws_ok(ws, ws_bytes, need), "det_adaln_modulate_bwd: workspace of %ld bytes is missing, too small or misaligned (need %ld)",
                (long)ws_bytes, (long)need);
  hipStream_t s = (hipStream_t)stream;
  float* part = (float*)ws;
  hipLaunchKernelGGL(rownorm_bwd_det_kernel<0>, dim3((unsigned)(frames * bpf)), dim3(256), 0, s, (const bf16_t*)x,
                     mod + scale_off, (const bf16_t*)dy, (bf16_t*)dx, part, (int)C, S, (int)bpf, mod_stride, eps,
                     (const bf16_t*)dres);
  LCV_LAUNCH_CHECK("det_adaln_modulate_bwd");
  int rc = det_colsum(part, frames * bpf, bpf, 2 * C, C, dmod + shift_off, mod_stride, 1, s, "det_adaln_modulate_bwd: dshift");
  if (rc != LCV_OK) return rc;
  return det_colsum(part + C, frames * bpf, bpf, 2 * C, C, dmod + scale_off, mod_stride, 1, s, "det_adaln_modulate_bwd: dscale");
}

extern "C" int lcv_det_layernorm_affine_bwd(const void* x, const float* w, const void* dy, void* dx, float* dw, float* db,
                                            int64_t rows, int64_t C, float eps, const void* dres, void* ws,
                                            int64_t ws_bytes, void* stream) {
  LCV_CHECK_ARG((dw == nullptr) == (db == nullptr), "det_layernorm_affine_bwd: dw and db go together");
  if (!dw) return lcv_layernorm_affine_bwd(x, w, dy, dx, nullptr, nullptr, rows, C, eps, dres, stream);
  LCV_CHECK_ARG(x && w && dy && dx, "det_layernorm_affine_bwd: null pointer");
  LCV_CHECK_ARG(C > 0 && C % 8 == 0 && C <= 4096, "det_layernorm_affine_bwd: C must be a multiple of 8 and <= 4096");
  if (rows == 0) return LCV_OK;
  const int64_t nb = (rows + DET_ROWNORM_RPB - 1) / DET_ROWNORM_RPB;
  const int64_t need = lcv_det_ws_bytes(LCV_DET_LAYERNORM, rows, C, 0);
  LCV_CHECK_ARG(nb <= 0x7fffffff, "det_layernorm_affine_bwd: too many workgroups");
  LCV_CHECK_ARG(det_ws_ok(ws, ws_bytes, need), "det_layernorm_affine_bwd: workspace of %ld bytes is missing, too small or misaligned (need %ld)",
                (long)ws_bytes, (long)need);
  hipStream_t s = (hipStream_t)stream;
  float* part = (float*)ws;
  hipLaunchKernelGGL(rownorm_bwd_det_kernel<1>, dim3((unsigned)nb), dim3(256), 0, s, (const bf16_t*)x, w,
                     (const bf16_t*)dy, (bf16_t*)dx, part, (int)C, rows, (int)nb, (int64_t)0, eps, (const bf16_t*)dres);
  LCV_LAUNCH_CHECK("det_layernorm_affine_bwd");
  int rc = det_colsum(part, nb, nb, 2 * C, C, db, 0, 1, s, "det_layernorm_affine_bwd: db");
  if (rc != LCV_OK) return rc;
  return det_colsum(part + C, nb, nb, 2 * C, C, dw, 0, 1, s, "det_layernorm_affine_bwd: dw");
}

// ---------------------------------------------------------------------------
// gated residual backward: dy = gate * dout ; dgate[frame] += dout * y   (gate_residual_bwd_dgate_kernel, per frame)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gate_residual_bwd_det_kernel(const bf16_t* __restrict__ y, const float* __restrict__ gate,
                                                                    const bf16_t* __restrict__ dout, bf16_t* __restrict__ dy,
                                                                    float* __restrict__ part, int cpk, int64_t S, int bpf,
                                                                    int64_t mod_stride) {
  const int64_t frame = blockIdx.x / bpf;
  const int64_t lo = frame * S + (int64_t)(blockIdx.x - frame * bpf) * DET_GATE_RPB;
  const int64_t hi = (lo + DET_GATE_RPB < (frame + 1) * S) ? lo + DET_GATE_RPB : (frame + 1) * S;
  float acc[GATE_MAXPK][8];
#pragma unroll
  for (int u = 0; u < GATE_MAXPK; ++u)
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[u][i] = 0.f;
  for (int64_t row = lo; row < hi; ++row) gate_bwd_row(y, gate, dout, dy, row, frame, cpk, mod_stride, acc);
  float* prow = part + (int64_t)blockIdx.x * cpk * 8;
#pragma unroll
  for (int u = 0; u < GATE_MAXPK; ++u) {
    const int pkc = threadIdx.x + u * 256;
    if (pkc < cpk) {
      *reinterpret_cast<f32x4*>(prow + pkc * 8) = f32x4{acc[u][0], acc[u][1], acc[u][2], acc[u][3]};
      *reinterpret_cast<f32x4*>(prow + pkc * 8 + 4) = f32x4{acc[u][4], acc[u][5], acc[u][6], acc[u][7]};
    }
  }
}

extern "C" int lcv_det_gate_residual_bwd(const void* y, const float* mod, const void* dout, void* dy, float* dmod,
                                         int64_t B, int64_t T, int64_t S, int64_t C, int64_t mod_stride,
                                         int64_t gate_off, void* ws, int64_t ws_bytes, void* stream) {
  if (!dmod) return lcv_gate_residual_bwd(y, mod, dout, dy, nullptr, B, T, S, C, mod_stride, gate_off, stream);
  LCV_CHECK_ARG(y && mod && dout && dy, "det_gate_residual_bwd: null pointer");
  LCV_CHECK_ARG(C % 8 == 0 && gate_off % 4 == 0 && mod_stride % 4 == 0, "det_gate_residual_bwd: bad alignment");
  LCV_CHECK_ARG(C / 8 <= 256 * GATE_MAXPK, "det_gate_residual_bwd: C=%ld is above the %d channels the fixed-order form takes",
                (long)C, 256 * GATE_MAXPK * 8);
  const int64_t frames = B * T;
  if (frames * S * C == 0) return LCV_OK;
  const int64_t bpf = (S + DET_GATE_RPB - 1) / DET_GATE_RPB;
  const int64_t need = lcv_det_ws_bytes(LCV_DET_GATE, frames, S, C);
  LCV_CHECK_ARG(frames * bpf <= 0x7fffffff, "det_gate_residual_bwd: too many workgroups");
  LCV_CHECK_ARG(det_ws_ok(ws, ws_bytes, need), "det_gate_residual_bwd: workspace of %ld bytes is missing, too small or misaligned (need %ld)",
                (long)ws_bytes, (long)need);
  hipStream_t s = (hipStream_t)stream;
  float* part = (float*)ws;
  hipLaunchKernelGGL(gate_residual_bwd_det_kernel, dim3((unsigned)(frames * bpf)), dim3(256), 0, s, (const bf16_t*)y,
                     mod + gate_off, (const bf16_t*)dout, (bf16_t*)dy, part, (int)(C / 8), S, (int)bpf, mod_stride);
  LCV_LAUNCH_CHECK("det_gate_residual_bwd");
  return det_colsum(part, frames * bpf, bpf, C, C, dmod + gate_off, mod_stride, 1, s, "det_gate_residual_bwd: dgate");
}

// ---------------------------------------------------------------------------
// q/k RMSNorm + RoPE backward:  dx = r * (dn - n * mean(dn * n)),  dn = w * rope^T(dout)   (qknorm_rope_bwd_kernel)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void qknorm_rope_bwd_det_kernel(
    const bf16_t* __restrict__ q_in, const bf16_t* __restrict__ k_in, const bf16_t* __restrict__ dq_out,
    const bf16_t* __restrict__ dk_out, bf16_t* __restrict__ dq_in, bf16_t* __restrict__ dk_in,
    const bf16_t* __restrict__ wq, const bf16_t* __restrict__ wk, const float* __restrict__ cs_tab, int H,
    int64_t in_sb, int64_t in_sn, int64_t q_sb, int64_t q_sn, int64_t kv_sb, int64_t kv_sn, int64_t din_sb,
    int64_t din_sn, int64_t pos_off, float eps, float q_scale, bool want_dwq, bool want_dwk, float* __restrict__ part) {
  __shared__ float s_dw[2][4][128];
  const int64_t n = blockIdx.x, b = blockIdx.y;
  float dwq_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, dwk_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  qknorm_rope_bwd_token(q_in, k_in, dq_out, dk_out, dq_in, dk_in, wq, wk, cs_tab, H, in_sb, in_sn, q_sb, q_sn, kv_sb, kv_sn,
                        din_sb, din_sn, pos_off, eps, q_scale, n, b, want_dwq, want_dwk, dwq_acc, dwk_acc);
  // this token's norm-weight gradients: the wave's 4 heads-in-flight by shuffles, the 4 waves through LDS in wave order,
  // then the token's own row of the workspace (dwq | dwk); a side that was not asked for or has no input is written as zeros
  qknorm_dw_stage(dwq_acc, dwk_acc, s_dw);
  float* prow = part + (b * gridDim.x + n) * 256;
  if (threadIdx.x < 128) {
    const int d = threadIdx.x;
    prow[d] = (want_dwq && q_in) ? s_dw[0][0][d] + s_dw[0][1][d] + s_dw[0][2][d] + s_dw[0][3][d] : 0.f;
  } else {
    const int d = threadIdx.x - 128;
    prow[128 + d] = (want_dwk && k_in) ? s_dw[1][0][d] + s_dw[1][1][d] + s_dw[1][2][d] + s_dw[1][3][d] : 0.f;
  }
}

extern "C" int lcv_det_qknorm_rope_bwd(const void* q_in, const void* k_in, const void* dq_out, const void* dk_out,
                                       void* dq_in, void* dk_in, const void* wq, const void* wk, const void* cs, int64_t B,
                                       int64_t N, int64_t H, int64_t in_sb, int64_t in_sn, int64_t q_sb, int64_t q_sn,
                                       int64_t kv_sb, int64_t kv_sn, int64_t din_sb, int64_t din_sn, int64_t pos_off,
                                       float eps, float q_scale, float* dwq, float* dwk, void* ws, int64_t ws_bytes,
                                       void* stream) {
  if (!dwq && !dwk)
    return lcv_qknorm_rope_bwd(q_in, k_in, dq_out, dk_out, dq_in, dk_in, wq, wk, cs, B, N, H, in_sb, in_sn, q_sb, q_sn,
                               kv_sb, kv_sn, din_sb, din_sn, pos_off, eps, q_scale, nullptr, nullptr, 1, stream);
  LCV_CHECK_ARG((q_in || k_in) && wq && wk, "det_qknorm_rope_bwd: null pointer");
  LCV_CHECK_ARG(!q_in || (dq_out && dq_in), "det_qknorm_rope_bwd: q gradients missing");
  LCV_CHECK_ARG(!k_in || (dk_out && dk_in), "det_qknorm_rope_bwd: k gradients missing");
  LCV_CHECK_ARG(in_sn % 8 == 0 && q_sn % 8 == 0 && kv_sn % 8 == 0 && din_sn % 8 == 0, "det_qknorm_rope_bwd: strides % 8");
  LCV_CHECK_ARG(B <= 65535, "det_qknorm_rope_bwd: B above 65535");
  if (B == 0 || N == 0) return LCV_OK;
  const int64_t need = lcv_det_ws_bytes(LCV_DET_QKNORM, B, N, 0);
  LCV_CHECK_ARG(det_ws_ok(ws, ws_bytes, need), "det_qknorm_rope_bwd: workspace of %ld bytes is missing, too small or misaligned (need %ld)",
                (long)ws_bytes, (long)need);
  hipStream_t s = (hipStream_t)stream;
  float* part = (float*)ws;
  hipLaunchKernelGGL(qknorm_rope_bwd_det_kernel, dim3((unsigned)N, (unsigned)B), dim3(256), 0, s, (const bf16_t*)q_in,
                     (const bf16_t*)k_in, (const bf16_t*)dq_out, (const bf16_t*)dk_out, (bf16_t*)dq_in, (bf16_t*)dk_in,
                     (const bf16_t*)wq, (const bf16_t*)wk, (const float*)cs, (int)H, in_sb, in_sn, q_sb, q_sn, kv_sb, kv_sn,
                     din_sb, din_sn, pos_off, eps, q_scale, dwq != nullptr, dwk != nullptr, part);
  LCV_LAUNCH_CHECK("det_qknorm_rope_bwd");
  const int64_t tokens = B * N, groups = (tokens + DET_QK_GROUP - 1) / DET_QK_GROUP;
  // level 1: each group of DET_QK_GROUP token rows into the group's first row; level 2: the groups' first rows into dwq / dwk
  int rc = det_colsum(part, tokens, DET_QK_GROUP, 256, 256, part, (int64_t)DET_QK_GROUP * 256, 0, s, "det_qknorm_rope_bwd: groups");
  if (rc != LCV_OK) return rc;
  if (dwq && q_in) {
    rc = det_colsum(part, groups, groups, (int64_t)DET_QK_GROUP * 256, 128, dwq, 0, 1, s, "det_qknorm_rope_bwd: dwq");
    if (rc != LCV_OK) return rc;
  }
  if (dwk && k_in) rc = det_colsum(part + 128, groups, groups, (int64_t)DET_QK_GROUP * 256, 128, dwk, 0, 1, s, "det_qknorm_rope_bwd: dwk");
  return rc;
}

// ---------------------------------------------------------------------------
// fp32 small-M linear backward w.r.t. its input:  da[m,k] = act'(a[m,k]) * sum_n dy[m,n] W[n,k]
// (linear_f32_smallm_bwd_kernel; each 256-row slab of W leaves its partial in the workspace, `da` is overwritten)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void linear_f32_smallm_bwd_det_kernel(const float* __restrict__ dy,
                                                                        const bf16_t* __restrict__ w,
                                                                        float* __restrict__ part, int M, int64_t N, int K,
                                                                        int nchunk, int64_t slab_stride) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* sdy = reinterpret_cast<float*>(smem);  // [M][nchunk]
  const int64_t n0 = (int64_t)blockIdx.x * nchunk;
  const int nn = (int)((N - n0) < nchunk ? (N - n0) : nchunk);
  for (int i = threadIdx.x; i < M * nchunk; i += 256) {
    const int m = i / nchunk, j = i - m * nchunk;
    sdy[i] = (j < nn) ? dy[(int64_t)m * N + n0 + j] : 0.f;
  }
  __syncthreads();
  float* pslab = part + (int64_t)blockIdx.x * slab_stride;
  for (int k0 = threadIdx.x * 2; k0 < K; k0 += 512) {
    float acc0[16], acc1[16];
#pragma unroll
    for (int m = 0; m < 16; ++m) { acc0[m] = 0.f; acc1[m] = 0.f; }
    for (int j = 0; j < nn; ++j) {
      const u16x2 wv = *reinterpret_cast<const u16x2*>(w + (n0 + j) * K + k0);
      const float w0 = bf2f(wv[0]), w1 = bf2f(wv[1]);
#pragma unroll
      for (int m = 0; m < 16; ++m) {
        if (m < M) {
          const float d = sdy[m * nchunk + j];
          acc0[m] += d * w0;
          acc1[m] += d * w1;
        }
      }
    }
#pragma unroll
    for (int m = 0; m < 16; ++m) {
      if (m < M) {
        pslab[(int64_t)m * K + k0] = acc0[m];
        pslab[(int64_t)m * K + k0 + 1] = acc1[m];
      }
    }
  }
}

extern "C" int lcv_det_linear_f32_smallm_bwd(const float* dy, const void* w, const float* a, float* da, int64_t M,
                                             int64_t N, int64_t K, int act_in, void* ws, int64_t ws_bytes, void* stream) {
  LCV_CHECK_ARG(dy && w && a && da, "det_linear_f32_smallm_bwd: null pointer");
  LCV_CHECK_ARG(K % 2 == 0, "det_linear_f32_smallm_bwd: K must be even");
  LCV_CHECK_ARG(M > 0 && N > 0 && K > 0, "det_linear_f32_smallm_bwd: empty shape");
  LCV_CHECK_ARG((M * K + 255) / 256 <= 65535, "det_linear_f32_smallm_bwd: M*K=%ld is above what the fixed-order sum takes", (long)(M * K));
  const int nchunk = 256;
  const int64_t slabs = (N + nchunk - 1) / nchunk;
  const int64_t need = lcv_det_ws_bytes(LCV_DET_SMALLM, M, N, K);
  LCV_CHECK_ARG(det_ws_ok(ws, ws_bytes, need), "det_linear_f32_smallm_bwd: workspace of %ld bytes is missing, too small or misaligned (need %ld)",
                (long)ws_bytes, (long)need);
  hipStream_t s = (hipStream_t)stream;
  float* part = (float*)ws;
  for (int64_t m0 = 0; m0 < M; m0 += 16) {
    const int Mc = (int)((M - m0) < 16 ? (M - m0) : 16);
    hipLaunchKernelGGL(linear_f32_smallm_bwd_det_kernel, dim3((unsigned)slabs), dim3(256), (size_t)Mc * nchunk * 4, s,
                       dy + m0 * N, (const bf16_t*)w, part + m0 * K, Mc, N, (int)K, nchunk, M * K);
    LCV_LAUNCH_CHECK("det_linear_f32_smallm_bwd");
  }
  int rc = det_colsum(part, slabs, slabs, M * K, M * K, da, 0, 0, s, "det_linear_f32_smallm_bwd: slabs");
  if (rc != LCV_OK) return rc;
  if (act_in == 1) {
    silu_grad_launch(a, da, M * K, s);
    LCV_LAUNCH_CHECK("det_silu_grad");
  }
  return LCV_OK;
}

// ---------------------------------------------------------------------------
// gradient-norm clip (grad_sumsq_kernel / clip_coef_kernel of optim.hip): one partial per chunk, one workgroup per tensor
// ---------------------------------------------------------------------------
template <bool F32>
__global__ __launch_bounds__(256) void grad_sumsq_det_kernel(const lcv_adam_tensor* __restrict__ tensors, int n,
                                                             float* __restrict__ chunk_part) {
  const int ti = find_tensor(tensors, n, blockIdx.x);
  const lcv_adam_tensor t = tensors[ti];
  const int64_t chunk = (int64_t)blockIdx.x - t.first_chunk;
  const float sumsq = grad_chunk_sumsq<F32>(t, chunk);
  if (threadIdx.x == 0) chunk_part[blockIdx.x] = sumsq;
}

// tensor blockIdx.x: its chunks' partials in a block-wide fixed tree; the sum goes to slot 0 of the tensor's row, zeros to the rest
__global__ __launch_bounds__(256) void tensor_sumsq_det_kernel(const lcv_adam_tensor* __restrict__ tensors,
                                                               const float* __restrict__ chunk_part,
                                                               float* __restrict__ per_tensor) {
  const lcv_adam_tensor t = tensors[blockIdx.x];
  const int64_t nchunks = (t.numel + CHUNK - 1) / CHUNK;
  const float* src = chunk_part + t.first_chunk;
  float acc = 0.f;
  for (int64_t c = threadIdx.x; c < nchunks; c += 256) acc += src[c];
  __shared__ float part[4];
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x < NORM_SLOTS)
    per_tensor[(int64_t)blockIdx.x * NORM_SLOTS + threadIdx.x] = threadIdx.x == 0 ? part[0] + part[1] + part[2] + part[3] : 0.f;
}

extern "C" int lcv_det_grad_norm_clip(const lcv_adam_tensor* tensors, int64_t n_tensors, int64_t total_chunks,
                                      int param_f32, float max_norm, float* per_tensor_ws, float* norm_coef_out, void* ws,
                                      int64_t ws_bytes, void* stream) {
  LCV_CHECK_ARG(tensors && per_tensor_ws && norm_coef_out && n_tensors > 0 && total_chunks > 0, "det_grad_norm_clip: bad arguments");
  LCV_CHECK_ARG(n_tensors <= 0x7fffffff && total_chunks <= 0x7fffffff, "det_grad_norm_clip: too many tensors or chunks");
  const int64_t need = lcv_det_ws_bytes(LCV_DET_GRAD_NORM, total_chunks, 0, 0);
  LCV_CHECK_ARG(ws != nullptr && ws_bytes >= need && ((uintptr_t)ws % 4) == 0,
                "det_grad_norm_clip: workspace of %ld bytes is missing or too small (need %ld)", (long)ws_bytes, (long)need);
  hipStream_t s = (hipStream_t)stream;
  float* chunk_part = (float*)ws;
  if (param_f32)
    hipLaunchKernelGGL(grad_sumsq_det_kernel<true>, dim3((unsigned)total_chunks), dim3(256), 0, s, tensors, (int)n_tensors, chunk_part);
  else
    hipLaunchKernelGGL(grad_sumsq_det_kernel<false>, dim3((unsigned)total_chunks), dim3(256), 0, s, tensors, (int)n_tensors, chunk_part);
  LCV_LAUNCH_CHECK("det_grad_sumsq");
  hipLaunchKernelGGL(tensor_sumsq_det_kernel, dim3((unsigned)n_tensors), dim3(256), 0, s, tensors, chunk_part, per_tensor_ws);
  LCV_LAUNCH_CHECK("det_tensor_sumsq");
  clip_coef_launch(per_tensor_ws, (int)n_tensors, max_norm, norm_coef_out, param_f32 != 0, s);   // clip_coef_kernel of optim.hip
  LCV_LAUNCH_CHECK("det_clip_coef");
  return LCV_OK;
}

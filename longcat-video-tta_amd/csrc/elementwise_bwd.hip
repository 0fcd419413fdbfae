// Backward kernels of the HBM-bound block pieces (TTA inner loop): AdaLN / LayerNorm, gated residual,
// q/k RMSNorm + RoPE, SwiGLU, unpatchify and the fp32 small-M linear (the skinny token contraction that
// yields the LoRA dA / dB lives in lora.hip).  bf16 roundings of the forward are treated as identity
// (straight-through), as autograd does for the reference's bf16 modules.
#include "bwd_rows.h"

// ---------------------------------------------------------------------------
// LayerNorm backward, one wave per row.
//   MODE 0 (AdaLN): y = xh*(1+scale)+shift ; g = dy*(1+scale) ; dshift += dy ; dscale += dy*xh
//   MODE 1 (affine): y = xh*w+b            ; g = dy*w         ; db += dy     ; dw += dy*xh
//   dx = rstd * (g - mean(g) - xh * mean(g*xh))
// ---------------------------------------------------------------------------
// Rows per workgroup when the parameter / modulation gradients are wanted: each wave walks ROWNORM_RPB/4 rows and the
// per-channel sums of the whole workgroup are kept in LDS (ds_add_f32), so the global fp32 atomics are one per channel per
// ROWNORM_RPB rows instead of one per channel per row (51 M -> 1.6 M per call at 6 240 tokens: the kernel was atomic-bound).
#define ROWNORM_RPB 32

template <int MODE>
__global__ __launch_bounds__(256) void rownorm_bwd_kernel(
    const bf16_t* __restrict__ x, const float* __restrict__ p_mul, const bf16_t* __restrict__ dy,
    bf16_t* __restrict__ dx, float* __restrict__ d_add, float* __restrict__ d_mul, int64_t rows, int C,
    int64_t S, int64_t mod_stride, float eps, int rows_per_block, const bf16_t* __restrict__ dres) {
  __shared__ float s_add[ROWNORM_MAXCH * 64 * 8], s_mul[ROWNORM_MAXCH * 64 * 8];
  const int lane = threadIdx.x & 63;
  const bool want_d = d_add != nullptr;
  const int64_t row0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t frame0 = (MODE == 0) ? row0 / S : 0;          // the frame the LDS sums belong to
  if (want_d) {
    for (int i = threadIdx.x; i < C; i += 256) { s_add[i] = 0.f; s_mul[i] = 0.f; }
    __syncthreads();
  }
  for (int it = 0; it < rows_per_block; it += 4) {
    const int64_t row = row0 + it + (threadIdx.x >> 6);
    if (row >= rows) continue;
    const bf16_t* xr = x + row * C;
    const bf16_t* gr = dy + row * C;
    const int64_t frame = (MODE == 0) ? row / S : 0;
    const float* pm = p_mul + frame * mod_stride;
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
    const bool in_lds = frame == frame0;      // a workgroup that straddles two frames sends the second one's rows directly
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
          if (want_d) {  // parameter / modulation gradients
            if (in_lds) {
              atomicAdd(&s_add[c + i], dyv);
              atomicAdd(&s_mul[c + i], dyv * xh);
            } else {
              atomicAdd(d_add + frame * mod_stride + c + i, dyv);
              atomicAdd(d_mul + frame * mod_stride + c + i, dyv * xh);
            }
          }
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
  if (want_d) {
    __syncthreads();
    for (int i = threadIdx.x; i < C; i += 256) {
      atomicAdd(d_add + frame0 * mod_stride + i, s_add[i]);
      atomicAdd(d_mul + frame0 * mod_stride + i, s_mul[i]);
    }
  }
}

extern "C" int lcv_adaln_modulate_bwd(const void* x, const float* mod, const void* dy, void* dx, float* dmod,
                                      int64_t B, int64_t T, int64_t S, int64_t C, int64_t mod_stride,
                                      int64_t shift_off, int64_t scale_off, float eps, const void* dres, void* stream) {
  LCV_CHECK_ARG(x && mod && dy && dx, "adaln_modulate_bwd: null pointer");
  LCV_CHECK_ARG(C > 0 && C % 8 == 0 && C <= 4096, "adaln_modulate_bwd: C must be a multiple of 8 and <= 4096");
  const int64_t rows = B * T * S;
  if (rows == 0) return LCV_OK;
  const int rpb = dmod ? ROWNORM_RPB : 4;
  hipLaunchKernelGGL(rownorm_bwd_kernel<0>, dim3((unsigned)((rows + rpb - 1) / rpb)), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)x, mod + scale_off, (const bf16_t*)dy, (bf16_t*)dx,
                     dmod ? dmod + shift_off : nullptr, dmod ? dmod + scale_off : nullptr, rows, (int)C, S,
                     mod_stride, eps, rpb, (const bf16_t*)dres);
  LCV_LAUNCH_CHECK("adaln_modulate_bwd");
  return LCV_OK;
}

extern "C" int lcv_layernorm_affine_bwd(const void* x, const float* w, const void* dy, void* dx, float* dw,
                                        float* db, int64_t rows, int64_t C, float eps, const void* dres, void* stream) {
  LCV_CHECK_ARG(x && w && dy && dx, "layernorm_affine_bwd: null pointer");
  LCV_CHECK_ARG((dw == nullptr) == (db == nullptr), "layernorm_affine_bwd: dw and db go together");
  LCV_CHECK_ARG(C > 0 && C % 8 == 0 && C <= 4096, "layernorm_affine_bwd: C must be a multiple of 8 and <= 4096");
  if (rows == 0) return LCV_OK;
  const int rpb = dw ? ROWNORM_RPB : 4;
  hipLaunchKernelGGL(rownorm_bwd_kernel<1>, dim3((unsigned)((rows + rpb - 1) / rpb)), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)x, w, (const bf16_t*)dy, (bf16_t*)dx, db, dw, rows, (int)C, (int64_t)1,
                     (int64_t)0, eps, rpb, (const bf16_t*)dres);
  LCV_LAUNCH_CHECK("layernorm_affine_bwd");
  return LCV_OK;
}

// ---------------------------------------------------------------------------
// gated residual backward: dy = gate * dout ; dgate[frame] += dout * y
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gate_residual_bwd_kernel(const bf16_t* __restrict__ y,
                                                                const float* __restrict__ gate,
                                                                const bf16_t* __restrict__ dout,
                                                                bf16_t* __restrict__ dy, float* __restrict__ dgate,
                                                                int64_t n_packets, int cpk, int64_t S,
                                                                int64_t mod_stride) {
  for (int64_t pk = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; pk < n_packets;
       pk += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = pk / cpk;
    const int c = (int)(pk - row * cpk) * 8;
    const int64_t goff = (row / S) * mod_stride + c;
    float d[8], o[8];
    unpack8(*reinterpret_cast<const u16x8*>(dout + pk * 8), d);
    const f32x4 g0 = *reinterpret_cast<const f32x4*>(gate + goff);
    const f32x4 g1 = *reinterpret_cast<const f32x4*>(gate + goff + 4);
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = d[i] * ((i < 4) ? g0[i] : g1[i - 4]);
    *reinterpret_cast<u16x8*>(dy + pk * 8) = pack8(o);
    if (dgate) {
      float yf[8];
      unpack8(*reinterpret_cast<const u16x8*>(y + pk * 8), yf);
#pragma unroll
      for (int i = 0; i < 8; ++i) atomicAdd(dgate + goff + i, d[i] * yf[i]);
    }
  }
}

// dgate wanted: a workgroup owns GATE_RPB consecutive rows; thread t owns the same 8-channel packets (t, t+256, ...) in
// every row, so the per-channel products accumulate in registers and reach memory as one atomic per channel per
// GATE_RPB rows (flushed early when the rows cross into the next frame).
#define GATE_RPB 32
__global__ __launch_bounds__(256) void gate_residual_bwd_dgate_kernel(const bf16_t* __restrict__ y, const float* __restrict__ gate,
                                                                      const bf16_t* __restrict__ dout, bf16_t* __restrict__ dy,
                                                                      float* __restrict__ dgate, int64_t rows, int cpk, int64_t S,
                                                                      int64_t mod_stride) {
  const int64_t row0 = (int64_t)blockIdx.x * GATE_RPB;
  float acc[GATE_MAXPK][8];
#pragma unroll
  for (int u = 0; u < GATE_MAXPK; ++u)
#pragma unroll
    for (int i = 0; i < 8; ++i) acc[u][i] = 0.f;
  int64_t cur_frame = row0 / S;
  auto flush = [&](int64_t frame) {
#pragma unroll
    for (int u = 0; u < GATE_MAXPK; ++u) {
      const int pkc = threadIdx.x + u * 256;
      if (pkc < cpk) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          atomicAdd(dgate + frame * mod_stride + pkc * 8 + i, acc[u][i]);
          acc[u][i] = 0.f;
        }
      }
    }
  };
  for (int r = 0; r < GATE_RPB; ++r) {
    const int64_t row = row0 + r;
    if (row >= rows) break;
    const int64_t frame = row / S;
    if (frame != cur_frame) { flush(cur_frame); cur_frame = frame; }
    gate_bwd_row(y, gate, dout, dy, row, frame, cpk, mod_stride, acc);
  }
  flush(cur_frame);
}

extern "C" int lcv_gate_residual_bwd(const void* y, const float* mod, const void* dout, void* dy, float* dmod,
                                     int64_t B, int64_t T, int64_t S, int64_t C, int64_t mod_stride,
                                     int64_t gate_off, void* stream) {
  LCV_CHECK_ARG(y && mod && dout && dy, "gate_residual_bwd: null pointer");
  LCV_CHECK_ARG(C % 8 == 0 && gate_off % 4 == 0 && mod_stride % 4 == 0, "gate_residual_bwd: bad alignment");
  const int64_t n_packets = B * T * S * (C / 8);
  if (n_packets == 0) return LCV_OK;
  if (dmod && C / 8 <= 256 * GATE_MAXPK) {
    const int64_t rows = B * T * S;
    hipLaunchKernelGGL(gate_residual_bwd_dgate_kernel, dim3((unsigned)((rows + GATE_RPB - 1) / GATE_RPB)), dim3(256), 0,
                       (hipStream_t)stream, (const bf16_t*)y, mod + gate_off, (const bf16_t*)dout, (bf16_t*)dy, dmod + gate_off,
                       rows, (int)(C / 8), S, mod_stride);
    LCV_LAUNCH_CHECK("gate_residual_bwd");
    return LCV_OK;
  }
  int64_t blocks = (n_packets + 255) / 256;
  if (blocks > 256 * 16) blocks = 256 * 16;
  hipLaunchKernelGGL(gate_residual_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)y, mod + gate_off, (const bf16_t*)dout, (bf16_t*)dy,
                     dmod ? dmod + gate_off : nullptr, n_packets, (int)(C / 8), S, mod_stride);
  LCV_LAUNCH_CHECK("gate_residual_bwd");
  return LCV_OK;
}

// ---------------------------------------------------------------------------
// q/k RMSNorm + RoPE backward (weights frozen):  dx = r * (dn - n * mean(dn * n)),  dn = w * rope^T(dout)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void qknorm_rope_bwd_kernel(
    const bf16_t* __restrict__ q_in, const bf16_t* __restrict__ k_in, const bf16_t* __restrict__ dq_out,
    const bf16_t* __restrict__ dk_out, bf16_t* __restrict__ dq_in, bf16_t* __restrict__ dk_in,
    const bf16_t* __restrict__ wq, const bf16_t* __restrict__ wk, const float* __restrict__ cs_tab, int H,
    int64_t in_sb, int64_t in_sn, int64_t q_sb, int64_t q_sn, int64_t kv_sb, int64_t kv_sn, int64_t din_sb,
    int64_t din_sn, int64_t pos_off, float eps, float q_scale, float* __restrict__ dwq, float* __restrict__ dwk,
    int dw_slots) {
  __shared__ float s_dw[2][4][128];
  const int64_t n = blockIdx.x, b = blockIdx.y;
  float dwq_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, dwk_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  qknorm_rope_bwd_token(q_in, k_in, dq_out, dk_out, dq_in, dk_in, wq, wk, cs_tab, H, in_sb, in_sn, q_sb, q_sn, kv_sb, kv_sn,
                        din_sb, din_sn, pos_off, eps, q_scale, n, b, dwq != nullptr, dwk != nullptr, dwq_acc, dwk_acc);
  // norm-weight gradients (only when asked for): sum over the wave's 4 heads-in-flight, then over the 4 waves through
  // LDS, then ONE atomic per dim per workgroup into accumulator row (token % dw_slots) — every token of every layer
  // call lands on the same 128 floats otherwise, and the kernel becomes a queue on those addresses
  if (dwq != nullptr || dwk != nullptr) {
    qknorm_dw_stage(dwq_acc, dwk_acc, s_dw);
    const int slot = (int)((n + b * gridDim.x) % dw_slots);
    if (threadIdx.x < 128) {
      const int d = threadIdx.x;
      if (dwq != nullptr && q_in) atomicAdd(dwq + slot * 128 + d, s_dw[0][0][d] + s_dw[0][1][d] + s_dw[0][2][d] + s_dw[0][3][d]);
    } else {
      const int d = threadIdx.x - 128;
      if (dwk != nullptr && k_in) atomicAdd(dwk + slot * 128 + d, s_dw[1][0][d] + s_dw[1][1][d] + s_dw[1][2][d] + s_dw[1][3][d]);
    }
  }
}

extern "C" int lcv_qknorm_rope_bwd(const void* q_in, const void* k_in, const void* dq_out, const void* dk_out,
                                   void* dq_in, void* dk_in, const void* wq, const void* wk, const void* cs,
                                   int64_t B, int64_t N, int64_t H, int64_t in_sb, int64_t in_sn, int64_t q_sb,
                                   int64_t q_sn, int64_t kv_sb, int64_t kv_sn, int64_t din_sb, int64_t din_sn,
                                   int64_t pos_off, float eps, float q_scale, float* dwq, float* dwk, int64_t dw_slots,
                                   void* stream) {
  LCV_CHECK_ARG((q_in || k_in) && wq && wk, "qknorm_rope_bwd: null pointer");
  LCV_CHECK_ARG(!q_in || (dq_out && dq_in), "qknorm_rope_bwd: q gradients missing");
  LCV_CHECK_ARG(!k_in || (dk_out && dk_in), "qknorm_rope_bwd: k gradients missing");
  LCV_CHECK_ARG(in_sn % 8 == 0 && q_sn % 8 == 0 && kv_sn % 8 == 0 && din_sn % 8 == 0, "qknorm_rope_bwd: strides % 8");
  LCV_CHECK_ARG((!dwq && !dwk) || (dw_slots >= 1 && dw_slots <= 65536), "qknorm_rope_bwd: dw_slots");
  if (B == 0 || N == 0) return LCV_OK;
  hipLaunchKernelGGL(qknorm_rope_bwd_kernel, dim3((unsigned)N, (unsigned)B), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)q_in, (const bf16_t*)k_in, (const bf16_t*)dq_out, (const bf16_t*)dk_out,
                     (bf16_t*)dq_in, (bf16_t*)dk_in, (const bf16_t*)wq, (const bf16_t*)wk, (const float*)cs,
                     (int)H, in_sb, in_sn, q_sb, q_sn, kv_sb, kv_sn, din_sb, din_sn, pos_off, eps, q_scale, dwq, dwk,
                     (int)(dw_slots < 1 ? 1 : dw_slots));
  LCV_LAUNCH_CHECK("qknorm_rope_bwd");
  return LCV_OK;
}

// ---------------------------------------------------------------------------
// SwiGLU backward
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void swiglu_bwd_kernel(const bf16_t* __restrict__ gate,
                                                         const bf16_t* __restrict__ up,
                                                         const bf16_t* __restrict__ dout,
                                                         bf16_t* __restrict__ dgate, bf16_t* __restrict__ dup,
                                                         int64_t rows, int fpk, int64_t ld_in) {
  const int64_t n_packets = rows * fpk;
  for (int64_t pk = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; pk < n_packets;
       pk += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = pk / fpk;
    const int c = (int)(pk - row * fpk) * 8;
    float g[8], u[8], d[8], og[8], ou[8];
    unpack8(*reinterpret_cast<const u16x8*>(gate + row * ld_in + c), g);
    unpack8(*reinterpret_cast<const u16x8*>(up + row * ld_in + c), u);
    unpack8(*reinterpret_cast<const u16x8*>(dout + pk * 8), d);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float sig = 1.0f / (1.0f + __expf(-g[i]));
      const float s = g[i] * sig;
      ou[i] = d[i] * bfround(s);
      og[i] = d[i] * u[i] * (sig * (1.0f + g[i] * (1.0f - sig)));
    }
    *reinterpret_cast<u16x8*>(dgate + pk * 8) = pack8(og);
    *reinterpret_cast<u16x8*>(dup + pk * 8) = pack8(ou);
  }
}

// The same on the fused GEMM's layout: `gu` [rows, 2F] holds, per 64 columns, 32 gate values then their 32 up partners
// (LCV_EPI_SWIGLU's auxiliary output); `dgu` gets the gradients in that layout, ready to be the A operand of ONE GEMM
// against the transposed interleaved weight (dx = dgate W1 + dup W3 without a second GEMM and an add).
__global__ __launch_bounds__(256) void swiglu_bwd_il_kernel(const bf16_t* __restrict__ gu, const bf16_t* __restrict__ dout,
                                                            bf16_t* __restrict__ dgu, int64_t rows, int fpk) {
  const int64_t n_packets = rows * fpk;
  for (int64_t pk = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; pk < n_packets;
       pk += (int64_t)gridDim.x * blockDim.x) {
    const int64_t row = pk / fpk;
    const int c = (int)(pk - row * fpk) * 8;                       // feature index
    const int64_t at = row * (int64_t)(fpk * 16) + (c >> 5) * 64 + (c & 31);   // its gate column in the interleaved row
    float g[8], u[8], d[8], og[8], ou[8];
    unpack8(*reinterpret_cast<const u16x8*>(gu + at), g);
    unpack8(*reinterpret_cast<const u16x8*>(gu + at + 32), u);
    unpack8(*reinterpret_cast<const u16x8*>(dout + pk * 8), d);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float sig = 1.0f / (1.0f + __expf(-g[i]));
      const float s = g[i] * sig;
      ou[i] = d[i] * bfround(s);
      og[i] = d[i] * u[i] * (sig * (1.0f + g[i] * (1.0f - sig)));
    }
    *reinterpret_cast<u16x8*>(dgu + at) = pack8(og);
    *reinterpret_cast<u16x8*>(dgu + at + 32) = pack8(ou);
  }
}

extern "C" int lcv_swiglu_bwd_interleaved(const void* gu, const void* dout, void* dgu, int64_t rows, int64_t F, void* stream) {
  LCV_CHECK_ARG(gu && dout && dgu, "swiglu_bwd_interleaved: null pointer");
  LCV_CHECK_ARG(F % 32 == 0, "swiglu_bwd_interleaved: F=%ld must be a multiple of 32", (long)F);
  const int64_t n_packets = rows * (F / 8);
  if (n_packets == 0) return LCV_OK;
  int64_t blocks = (n_packets + 255) / 256;
  if (blocks > 256 * 16) blocks = 256 * 16;
  hipLaunchKernelGGL(swiglu_bwd_il_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)gu,
                     (const bf16_t*)dout, (bf16_t*)dgu, rows, (int)(F / 8));
  LCV_LAUNCH_CHECK("swiglu_bwd_interleaved");
  return LCV_OK;
}

extern "C" int lcv_swiglu_bwd(const void* gate, const void* up, const void* dout, void* dgate, void* dup,
                              int64_t rows, int64_t F, int64_t ld_in, void* stream) {
  LCV_CHECK_ARG(gate && up && dout && dgate && dup, "swiglu_bwd: null pointer");
  LCV_CHECK_ARG(F % 8 == 0 && ld_in % 8 == 0, "swiglu_bwd: F and ld_in must be multiples of 8");
  const int64_t n_packets = rows * (F / 8);
  if (n_packets == 0) return LCV_OK;
  int64_t blocks = (n_packets + 255) / 256;
  if (blocks > 256 * 16) blocks = 256 * 16;
  hipLaunchKernelGGL(swiglu_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream,
                     (const bf16_t*)gate, (const bf16_t*)up, (const bf16_t*)dout, (bf16_t*)dgate, (bf16_t*)dup, rows,
                     (int)(F / 8), ld_in);
  LCV_LAUNCH_CHECK("swiglu_bwd");
  return LCV_OK;
}

// ---------------------------------------------------------------------------
// unpatchify backward: dout [B,Cout,T,H,W] fp32 -> dtok [B, N, (ph pw c)] fp32
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void unpatchify_bwd_kernel(const float* __restrict__ dout,
                                                             float* __restrict__ dtok, int64_t B, int Cout, int T,
                                                             int H, int W) {
  const int Hh = H / 2, Wh = W / 2;
  const int64_t total = (int64_t)B * T * Hh * Wh * 4 * Cout;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int k = (int)(i % (4 * Cout));
    int64_t tkn = i / (4 * Cout);
    const int c = k % Cout;
    const int pp = k / Cout;  // ph*2 + pw
    const int wq = (int)(tkn % Wh);
    int64_t r = tkn / Wh;
    const int hq = (int)(r % Hh);
    r /= Hh;
    const int t = (int)(r % T);
    const int64_t b = r / T;
    dtok[i] = dout[(((b * Cout + c) * T + t) * H + 2 * hq + (pp >> 1)) * (int64_t)W + 2 * wq + (pp & 1)];
  }
}

extern "C" int lcv_unpatchify_bwd(const float* dout, float* dtok, int64_t B, int64_t Cout, int64_t T, int64_t H,
                                  int64_t W, void* stream) {
  LCV_CHECK_ARG(dout && dtok, "unpatchify_bwd: null pointer");
  const int64_t total = B * Cout * T * H * W;
  if (total == 0) return LCV_OK;
  int64_t blocks = (total + 255) / 256;
  if (blocks > 256 * 16) blocks = 256 * 16;
  hipLaunchKernelGGL(unpatchify_bwd_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, dout, dtok,
                     B, (int)Cout, (int)T, (int)H, (int)W);
  LCV_LAUNCH_CHECK("unpatchify_bwd");
  return LCV_OK;
}

// ---------------------------------------------------------------------------
// fp32 small-M linear backward w.r.t. its input:  da[m,k] = act'(a[m,k]) * sum_n dy[m,n] W[n,k]
// Partial sums over 256-row slabs of W are accumulated with fp32 atomics into `da` (zero-filled here);
// a second tiny launch applies the SiLU derivative.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void linear_f32_smallm_bwd_kernel(const float* __restrict__ dy,
                                                                    const bf16_t* __restrict__ w,
                                                                    float* __restrict__ da, int M, int64_t N, int K,
                                                                    int nchunk) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* sdy = reinterpret_cast<float*>(smem);  // [M][nchunk]
  const int64_t n0 = (int64_t)blockIdx.x * nchunk;
  const int nn = (int)((N - n0) < nchunk ? (N - n0) : nchunk);
  for (int i = threadIdx.x; i < M * nchunk; i += 256) {
    const int m = i / nchunk, j = i - m * nchunk;
    sdy[i] = (j < nn) ? dy[(int64_t)m * N + n0 + j] : 0.f;
  }
  __syncthreads();
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
        atomicAdd(da + (int64_t)m * K + k0, acc0[m]);
        atomicAdd(da + (int64_t)m * K + k0 + 1, acc1[m]);
      }
    }
  }
}

__global__ __launch_bounds__(256) void silu_grad_kernel(const float* __restrict__ a, float* __restrict__ da,
                                                        int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) {
    const float x = a[i];
    const float sig = 1.0f / (1.0f + __expf(-x));
    da[i] *= sig * (1.0f + x * (1.0f - sig));
  }
}

void silu_grad_launch(const float* a, float* da, int64_t n, hipStream_t s) {
  hipLaunchKernelGGL(silu_grad_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a, da, n);
}

extern "C" int lcv_linear_f32_smallm_bwd(const float* dy, const void* w, const float* a, float* da, int64_t M,
                                         int64_t N, int64_t K, int act_in, void* stream) {
  LCV_CHECK_ARG(dy && w && a && da, "linear_f32_smallm_bwd: null pointer");
  LCV_CHECK_ARG(K % 2 == 0, "linear_f32_smallm_bwd: K must be even");
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(da, 0, sizeof(float) * M * K, s) != hipSuccess) {
    lcv_set_error("linear_f32_smallm_bwd: memset failed");
    return LCV_EDEVICE;
  }
  const int nchunk = 256;
  for (int64_t m0 = 0; m0 < M; m0 += 16) {
    const int Mc = (int)((M - m0) < 16 ? (M - m0) : 16);
    hipLaunchKernelGGL(linear_f32_smallm_bwd_kernel, dim3((unsigned)((N + nchunk - 1) / nchunk)), dim3(256),
                       (size_t)Mc * nchunk * 4, s, dy + m0 * N, (const bf16_t*)w, da + m0 * K, Mc, N, (int)K, nchunk);
    LCV_LAUNCH_CHECK("linear_f32_smallm_bwd");
  }
  if (act_in == 1) {
    silu_grad_launch(a, da, M * K, s);
    LCV_LAUNCH_CHECK("silu_grad");
  }
  return LCV_OK;
}

// What the default backward kernels (elementwise_bwd.hip) and their fixed-order forms (reduce_det.hip) share: ONE definition
// each of the gate and q/k-norm row math that dy / dq_in / dk_in come from.  A pair of kernels differs only where a sum leaves
// the thread (atomics in the default form, registers + a workspace row in the fixed-order form), and that part stays in the
// kernel.  (The LayerNorm row and the small-M slab are still written out in both of their kernels: profiles/bwd_rows.md.)
#pragma once
#include "lcv_common.h"

#define ROWNORM_MAXCH 8   // C <= 4096: 8 packets of 8 channels per lane
#define GATE_MAXPK 2      // C <= 4096: 512 packets per row over 256 threads

// ---- gated residual backward: thread t's packets (t, t+256, ...) of one row:  dy = gate * dout ; acc += dout * y ----
__device__ __forceinline__ void gate_bwd_row(const bf16_t* y, const float* gate, const bf16_t* dout, bf16_t* dy, int64_t row,
                                             int64_t frame, int cpk, int64_t mod_stride, float (&acc)[GATE_MAXPK][8]) {
#pragma unroll
  for (int u = 0; u < GATE_MAXPK; ++u) {
    const int pkc = threadIdx.x + u * 256;
    if (pkc < cpk) {
      const int64_t pk = row * cpk + pkc;
      const int64_t goff = frame * mod_stride + pkc * 8;
      float d[8], o[8], yf[8];
      unpack8(*reinterpret_cast<const u16x8*>(dout + pk * 8), d);
      unpack8(*reinterpret_cast<const u16x8*>(y + pk * 8), yf);
      const f32x4 g0 = *reinterpret_cast<const f32x4*>(gate + goff);
      const f32x4 g1 = *reinterpret_cast<const f32x4*>(gate + goff + 4);
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        o[i] = d[i] * ((i < 4) ? g0[i] : g1[i - 4]);
        acc[u][i] = fmaf(d[i], yf[i], acc[u][i]);
      }
      *reinterpret_cast<u16x8*>(dy + pk * 8) = pack8(o);
    }
  }
}

// ---- q/k RMSNorm + RoPE backward (weights frozen):  dx = r * (dn - n * mean(dn * n)),  dn = w * rope^T(dout) ----
__device__ __forceinline__ void norm_rope_bwd_vec(const bf16_t* xin, const bf16_t* dout, bf16_t* dxin,
                                                  const float (&w)[8], const float (&cs)[8], bool do_rope,
                                                  float eps, float out_scale, float (&dwacc)[8], bool want_dw) {
  float x[8], d[8];
  unpack8(*reinterpret_cast<const u16x8*>(xin), x);
  unpack8(*reinterpret_cast<const u16x8*>(dout), d);
#pragma unroll
  for (int i = 0; i < 8; ++i) d[i] *= out_scale;  // the forward multiplied its output by out_scale
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) ss += x[i] * x[i];
  ss += __shfl_xor(ss, 8, 64);
  ss += __shfl_xor(ss, 4, 64);
  ss += __shfl_xor(ss, 2, 64);
  ss += __shfl_xor(ss, 1, 64);
  const float r = rsqrtf(ss * (1.0f / 128.0f) + eps);
  float dn[8], n[8];
  float dot = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float d0 = d[2 * i], d1 = d[2 * i + 1];
    if (do_rope) {
      const float c = cs[2 * i], s = cs[2 * i + 1];
      const float t0 = d0 * c + d1 * s;
      const float t1 = d1 * c - d0 * s;
      d0 = t0;
      d1 = t1;
    }
    dn[2 * i] = d0 * w[2 * i];
    dn[2 * i + 1] = d1 * w[2 * i + 1];
    if (want_dw) {  // y = rope(n * w): dw += rope^T(dout) * n (norm-weight tuning, run_norm_tune_tta.py:87-98)
      dwacc[2 * i] += d0 * (x[2 * i] * r);
      dwacc[2 * i + 1] += d1 * (x[2 * i + 1] * r);
    }
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    n[i] = x[i] * r;
    dot += dn[i] * n[i];
  }
  dot += __shfl_xor(dot, 8, 64);
  dot += __shfl_xor(dot, 4, 64);
  dot += __shfl_xor(dot, 2, 64);
  dot += __shfl_xor(dot, 1, 64);
  dot *= (1.0f / 128.0f);
  float o[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) o[i] = r * (dn[i] - n[i] * dot);
  *reinterpret_cast<u16x8*>(dxin) = pack8(o);
}

// token n of batch b, one workgroup: cos/sin and weights of this thread's 8 dims, then every head (16 in flight, 16 threads
// each).  Writes dq_in / dk_in; this thread's norm-weight terms are added to dwq_acc / dwk_acc where wanted.
__device__ __forceinline__ void qknorm_rope_bwd_token(
    const bf16_t* q_in, const bf16_t* k_in, const bf16_t* dq_out, const bf16_t* dk_out, bf16_t* dq_in, bf16_t* dk_in,
    const bf16_t* wq, const bf16_t* wk, const float* cs_tab, int H, int64_t in_sb, int64_t in_sn, int64_t q_sb, int64_t q_sn,
    int64_t kv_sb, int64_t kv_sn, int64_t din_sb, int64_t din_sn, int64_t pos_off, float eps, float q_scale, int64_t n,
    int64_t b, bool want_dwq, bool want_dwk, float (&dwq_acc)[8], float (&dwk_acc)[8]) {
  const int sub = threadIdx.x & 15;
  const int hl = threadIdx.x >> 4;
  float cs[8] = {1, 0, 1, 0, 1, 0, 1, 0};
  const bool do_rope = cs_tab != nullptr;
  if (do_rope) {
    const float* p = cs_tab + ((pos_off + n) * 64 + sub * 4) * 2;
    const f32x4 a = *reinterpret_cast<const f32x4*>(p);
    const f32x4 c = *reinterpret_cast<const f32x4*>(p + 4);
    cs[0] = a[0]; cs[1] = a[1]; cs[2] = a[2]; cs[3] = a[3];
    cs[4] = c[0]; cs[5] = c[1]; cs[6] = c[2]; cs[7] = c[3];
  }
  float wqf[8], wkf[8];
  unpack8(*reinterpret_cast<const u16x8*>(wq + sub * 8), wqf);
  unpack8(*reinterpret_cast<const u16x8*>(wk + sub * 8), wkf);
  for (int h0 = 0; h0 < H; h0 += 16) {
    const int h = h0 + hl;
    if (h >= H) continue;
    const int64_t off = (int64_t)h * 128 + sub * 8;
    if (q_in)
      norm_rope_bwd_vec(q_in + b * in_sb + n * in_sn + off, dq_out + b * q_sb + n * q_sn + off,
                        dq_in + b * din_sb + n * din_sn + off, wqf, cs, do_rope, eps, q_scale, dwq_acc, want_dwq);
    if (k_in)
      norm_rope_bwd_vec(k_in + b * in_sb + n * in_sn + off, dk_out + b * kv_sb + n * kv_sn + off,
                        dk_in + b * din_sb + n * din_sn + off, wkf, cs, do_rope, eps, 1.0f, dwk_acc, want_dwk);
  }
}

// the workgroup's norm-weight sums: the wave's 4 heads-in-flight by shuffles, then each wave's 128 sums to its LDS row.
// On return s_dw[q|k][wave][dim] is filled and synchronised; the reader adds the waves as w0 + w1 + w2 + w3.
__device__ __forceinline__ void qknorm_dw_stage(const float (&dwq_acc)[8], const float (&dwk_acc)[8], float (&s_dw)[2][4][128]) {
  const int sub = threadIdx.x & 15;
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    float a = dwq_acc[i], c = dwk_acc[i];
    a += __shfl_xor(a, 16, 64); a += __shfl_xor(a, 32, 64);
    c += __shfl_xor(c, 16, 64); c += __shfl_xor(c, 32, 64);
    if ((threadIdx.x & 63) < 16) {
      s_dw[0][wave][sub * 8 + i] = a;
      s_dw[1][wave][sub * 8 + i] = c;
    }
  }
  __syncthreads();
}

// ---- host: internal launcher shared by the two small-M entry points (the caller runs LCV_LAUNCH_CHECK under its own name) ----
void silu_grad_launch(const float* a, float* da, int64_t n, hipStream_t s);   // elementwise_bwd.hip: da *= silu'(a)

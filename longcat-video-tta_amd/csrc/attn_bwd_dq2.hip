// Attention backward, pass B (dQ), second form - for the self-attention path where q is pre-scaled into log2 units
// (scale * log2(e) == 1; attn_fwd.hip, VAR bit 1).  Same geometry as attn_bwd_dq_kernel (8 waves x 32 query rows, 64-key tiles,
// query on the lane, S^T = K Q^T, dP^T = V dO^T, dQ^T += K^T dS^T), rebuilt like the forward kernel:
//   * K / V tiles by LDS-DMA from per-lane pointers that advance one tile per iteration (no staging registers, no ds_write);
//   * the last (possibly ragged) tile peeled, so the steady-state body has neither mask code nor ragged-row code;
//   * row constants as the initial accumulator (cdna_hip_programming.md, attention backward): the score accumulators START at
//     -lse (log2 units), so P = exp2(accumulator) needs no multiply-subtract, and the softmax scale is applied once to dQ in the
//     epilogue instead of to every dS:  dS' = P * (dP - delta)  is 2 vector instructions per score instead of 5.
//   * (round 4) a 64-key tile is worked through as two 32-key halves - S / dP of a half (16 MFMAs), its dS', its 8 dQ MFMAs - so
//     the score accumulators take 32 registers instead of 64, and the 32 freed hold fragment reads two MFMA pairs ahead.  At 256
//     registers hipcc had put 29 of the 64 fragment reads of a tile directly in front of their MFMA behind `lgkmcnt(0)`
//     (SQ_WAIT_ANY 0.41 of the wave cycles -> 0.15 now).  Bit-identical (same products, same order per accumulator); +3 % only:
//     with the waits gone the chip lowers its clock (1.74 -> 1.65 GHz at MFMA busy 0.64 -> 0.70): profiles/r04_attn_bwd_passB.md.
// This loop, like the forward, is vector-issue bound: the file is built without SLP vectorisation (lcv_hip/build.py).
#include "attn_common.h"
#include <stdlib.h>
#include <type_traits>

struct AttnBwdDq2Params {
  const bf16_t* q;
  const bf16_t* k;
  const bf16_t* v;
  const bf16_t* d_o;
  const float* lse;
  const float* delta;
  bf16_t* dq;
  AttnDims d;
  int64_t dq_sb, dq_sn, dq_sh;
  float scale;
  int gx, xcd_remap;   // blocks per (batch, head); head-per-XCD block order (ATTN_BLOCK_DECODE)
};

// <NW, NS>: waves per workgroup (32 query rows each) and K / V stages.  <8, 4>: one workgroup per CU, DMA three tiles ahead.
// <4, 2>: TWO workgroups per CU (128 KiB of LDS together) whose barriers are independent - within one workgroup the barrier
// per tile starts every wave's MFMA phase at the same moment, so one wave's exp / convert work never sits under another's
// MFMAs (the lockstep the forward kernel had before it was software-pipelined); two workgroups drift apart and overlap, at the
// price of streaming K / V into LDS twice.
template <int NW, int NS>
__global__ __launch_bounds__(NW * 64) __attribute__((amdgpu_waves_per_eu(2, 2))) void attn_bwd_dq2_kernel(const AttnBwdDq2Params p) {
  constexpr int QROWS = NW * 32;
  constexpr int NP = 16 / NW;                  // one-KiB DMA pieces per wave, tile and tensor (4 rows each)
  constexpr int TILE_BYTES = 64 * 256;
  constexpr int ROW_AHEAD = 2, TR_AHEAD = 2;   // fragment reads in flight ahead of their MFMAs: K / V row fragments (pairs), K^T fragments
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  lds_u8* lds = (lds_u8*)smem;  // [NS][K tile | V tile]

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  int qb, head;
  int64_t b;
  ATTN_BLOCK_DECODE(p, qb, head, b);
  const int64_t q0 = (int64_t)qb * QROWS + wave * 32;
  const bf16_t* kbase = p.k + b * p.d.k_sb + (int64_t)head * p.d.k_sh;
  const bf16_t* vbase = p.v + b * p.d.v_sb + (int64_t)head * p.d.v_sh;

  bf16x8 qf[8], dof[8];
  float sinit;   // -lse (log2 units) of this lane's query: every element of the score accumulators starts there
  float delta_q;
  {
    int64_t qrow = q0 + r;
    if (qrow > p.d.Nq - 1) qrow = p.d.Nq - 1;
    const bf16_t* qp = p.q + b * p.d.q_sb + qrow * p.d.q_sn + (int64_t)head * p.d.q_sh + 8 * h;
    const bf16_t* dp_ = p.d_o + b * p.d.o_sb + qrow * p.d.o_sn + (int64_t)head * p.d.o_sh + 8 * h;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
      qf[ks] = *reinterpret_cast<const bf16x8*>(qp + 16 * ks);
      dof[ks] = *reinterpret_cast<const bf16x8*>(dp_ + 16 * ks);
    }
    sinit = -p.lse[(b * p.d.H + head) * p.d.Nq + qrow] * 1.4426950408889634f;
    delta_q = p.delta[(b * p.d.H + head) * p.d.Nq + qrow];
  }

  // LDS-DMA roles (as attn_fwd.hip): wave w fills rows 8 w .. 8 w + 7 of both tiles, 2 + 2 one-KiB instructions.  Source = a
  // scalar tile base (advanced one tile per issue by scalar adds) + a per-lane 32-bit byte offset that never changes; issued from
  // asm (lcv_common.h: a builtin DMA would be waited for before the next fragment read) and waited for at the end of the tile.
  // <4, 2> keeps ONE offset per piece (with eight the loop spilled, and a spill reload's vmcnt wait drains the DMA queue): the V
  // offset of piece i is the K offset + row_i * D, D = (v_sn - k_sn) * 2 bytes (K and V are slices of two different packed
  // tensors in the product: strides 2 H 128 and 3 H 128); row_i = (4 NP wave + 4 i) + (lane >> 4), so the first part goes into
  // the scalar base of the piece and the second is one more register.
  constexpr bool ONE_OFF = NW == 4;
  unsigned koff[NP], voff[ONE_OFF ? 1 : NP];
  const int64_t kv_delta = (p.d.v_sn - p.d.k_sn) * 2;
  auto lane16 = []() -> int { return (int)((unsigned)lane_now() >> 4); };
  auto dma_row_of = [&](int i) { return 4 * NP * wave + 4 * i + lane16(); };
  // recomputed from the hardware lane id at every use: a register held across the loop for it tipped three offsets into scratch
  // (wraps for a negative delta; the SUM with koff is a true offset >= 0)
  auto vlane = [&]() -> unsigned { return (unsigned)lane16() * (unsigned)kv_delta; };
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const int row = 4 * NP * wave + 4 * i + (lane >> 4);
    const int col = 8 * ((lane & 15) ^ attn_swz(row));
    koff[i] = (unsigned)((row * p.d.k_sn + col) * 2);
    if constexpr (!ONE_OFF) voff[i] = (unsigned)((row * p.d.v_sn + col) * 2);
  }
  const char* kbase_u = lcv_uniform_ptr(kbase);
  const char* vbase_u = lcv_uniform_ptr(vbase);
  const unsigned lds_addr0 = (unsigned)(uintptr_t)lds;
  auto dma_tile = [&](int t, int buf, auto full_c) {
    constexpr bool FULL = decltype(full_c)::value;
    const unsigned dst = lds_addr0 + (unsigned)(buf * 2 * TILE_BYTES) + (unsigned)wave * (unsigned)(NP * 1024);
    const char* kt = kbase_u + (int64_t)t * (128 * p.d.k_sn);   // scalar: 64 rows x stride x 2 bytes per tile
    const char* vt = vbase_u + (int64_t)t * (128 * p.d.v_sn);
    if (FULL || (int64_t)t * 64 + 64 <= p.d.Nk) {
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        lcv_lds_dma16_sv(koff[i], kt, dst + 1024u * i);
        if constexpr (ONE_OFF) lcv_lds_dma16_sv(koff[i] + vlane(), vt + (4 * NP * wave + 4 * i) * kv_delta, dst + (unsigned)TILE_BYTES + 1024u * i);
        else lcv_lds_dma16_sv(voff[i], vt, dst + (unsigned)TILE_BYTES + 1024u * i);
      }
    } else {  // ragged last tile (once per workgroup): rows past Nk re-read the last key (masked below)
#pragma unroll
      for (int i = 0; i < NP; ++i) {
        int64_t back = (int64_t)t * 64 + dma_row_of(i) - (p.d.Nk - 1);
        if (back < 0) back = 0;
        lcv_lds_dma16(kt + koff[i] - back * p.d.k_sn * 2, dst + 1024u * i);
        const int64_t vo = ONE_OFF ? (int64_t)koff[i] + (int64_t)dma_row_of(i) * kv_delta : (int64_t)voff[ONE_OFF ? 0 : i];
        lcv_lds_dma16(vt + vo - back * p.d.v_sn * 2, dst + (unsigned)TILE_BYTES + 1024u * i);
      }
    }
  };

  const int kfz = attn_swz(r);
  const int k_row_off = 256 * r;
  const int q4 = (lane >> 2) & 3, p4 = lane & 3, g1 = (lane >> 4) & 1;
  int t_base[2], t_low[2];
#pragma unroll
  for (int half = 0; half < 2; ++half) {
    t_base[half] = 256 * (4 * h + 8 * half + q4) + 8 * (p4 & 1);
    t_low[half] = (2 * g1 + (p4 >> 1)) ^ (h + 2 * half);
  }

  f32x16 dqacc[4];
#pragma unroll
  for (int d = 0; d < 4; ++d)
#pragma unroll
    for (int e = 0; e < 16; ++e) dqacc[d][e] = 0.f;

  // K / V stages: a ring of NS = 4 (128 KiB; one workgroup per CU anyway: ~220 registers per wave), the DMA runs three tiles
  // ahead.  With two stages a tile had one tile's worth of MFMAs (~1.6 us) to land and the waves still waited 45 % of their
  // cycles; counted waits: at the end of tile t only tile t+1 has to be in, t+2 and t+3 stay in flight (4 pieces each).
  static_assert((NW == 8 && NS == 4) || (NW == 4 && NS == 2), "the counted waits below are written for these two forms");
  const int nt = (int)((p.d.Nk + 63) / 64);
#pragma unroll
  for (int i = 0; i < NS - 1; ++i)
    if (i < nt) dma_tile(i, i, std::false_type{});
  if (NS == 4 && nt >= 3) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
  else if (NS == 4 && nt == 2) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  else __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0), visible to hipcc's wait insertion (an asm wait is not): no conservative vmcnt(N) for the row constants inside the loop
  __syncthreads();

  auto tile_body = [&](const int t, auto last_c, auto full_dma_c) {
    constexpr bool has_next = !decltype(last_c)::value;
    const int buf = t & (NS - 1);
    if (decltype(full_dma_c)::value || t + NS - 1 < nt) dma_tile(t + NS - 1, (t + NS - 1) & (NS - 1), full_dma_c);   // the stage tile t-1 has just left
    const lds_u8* kb = lds + buf * 2 * TILE_BYTES;
    const lds_u8* vb = kb + TILE_BYTES;

    // two 32-key halves, one after the other (see the head of the file); dS' = P * (dP - delta), P = exp2(S - lse): the scale is
    // applied to dQ once, in the epilogue.  (Starting the dP accumulators at -delta, as the scores start at -lse, saves the 32
    // subtractions but needs a second resident 16-register tuple: not kept, round 3.)
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const lds_u8* kh = kb + half * 32 * 256 + k_row_off;
      const lds_u8* vh = vb + half * 32 * 256 + k_row_off;
      auto co = [&](int ks) { return 16 * ((2 * ks + h) ^ kfz); };
      f32x16 s, d;
#pragma unroll
      for (int e = 0; e < 16; ++e) { s[e] = sinit; d[e] = 0.f; }
      bf16x8 af[ROW_AHEAD + 1], cf[ROW_AHEAD + 1];
#pragma unroll
      for (int i = 0; i < ROW_AHEAD; ++i) {
        af[i] = *reinterpret_cast<const AS3 bf16x8*>(kh + co(i));
        cf[i] = *reinterpret_cast<const AS3 bf16x8*>(vh + co(i));
      }
#pragma unroll
      for (int ks = 0; ks < 8; ++ks) {
        if (ks + ROW_AHEAD < 8) {
          af[(ks + ROW_AHEAD) % (ROW_AHEAD + 1)] = *reinterpret_cast<const AS3 bf16x8*>(kh + co(ks + ROW_AHEAD));
          cf[(ks + ROW_AHEAD) % (ROW_AHEAD + 1)] = *reinterpret_cast<const AS3 bf16x8*>(vh + co(ks + ROW_AHEAD));
        }
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[ks % (ROW_AHEAD + 1)], qf[ks], s, 0, 0, 0);
        d = __builtin_amdgcn_mfma_f32_32x32x16_bf16(cf[ks % (ROW_AHEAD + 1)], dof[ks], d, 0, 0, 0);
      }
      if (!has_next && (p.d.Nk & 63)) {  // last tile only
        const int valid = (int)(p.d.Nk - (int64_t)t * 64) - 32 * half;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int key = (e & 3) + 8 * (e >> 2) + 4 * h;
          if (key >= valid) s[e] = -INFINITY;
        }
      }
      // K^T fragments of this half's 8 dQ products (i = 2 kk2 + ... : kk2 = i >> 2, dd = i & 3), TR_AHEAD products ahead; the
      // first ones are requested BEFORE the vector work on the scores, which hides their latency
      auto ktf_read = [&](int i) {
        const int kk = 2 * half + (i >> 2), dd = i & 3;
        const int dx = 64 * (dd ^ q4);
        const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((AS3 s16x4*)(kb + t_base[0] + 4096 * kk + dx + 16 * t_low[0]));
        const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((AS3 s16x4*)(kb + t_base[1] + 4096 * kk + dx + 16 * t_low[1]));
        return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
      };
      bf16x8 ktf[TR_AHEAD + 1];
#pragma unroll
      for (int i = 0; i < TR_AHEAD; ++i) ktf[i] = ktf_read(i);
#pragma unroll
      for (int e = 0; e < 16; ++e) s[e] = __builtin_amdgcn_exp2f(s[e]) * (d[e] - delta_q);
      bf16x8 dsb[2];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        dsb[0][j] = (__bf16)s[j];
        dsb[1][j] = (__bf16)s[8 + j];
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        if (i + TR_AHEAD < 8) ktf[(i + TR_AHEAD) % (TR_AHEAD + 1)] = ktf_read(i + TR_AHEAD);
        dqacc[i & 3] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ktf[i % (TR_AHEAD + 1)], dsb[i >> 2], dqacc[i & 3], 0, 0, 0);
      }
    }
    if (has_next) {   // tile t+1 is in; what was requested after it may still be in flight
      const int later = nt - 2 - t;   // tiles requested after t+1 (at most NS - 2 of them are outstanding)
      if (NS == 4 && later >= 2) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
      else if (NS == 4 && later == 1) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      else lcv_dma_wait_all();
    }
    __syncthreads();
  };
  // steady state: the tile requested (t + NS - 1) is a whole one - no ragged-row code, and none of its values, in the loop
  int t = 0;
  for (; t + NS - 1 < nt - 1; ++t) tile_body(t, std::false_type{}, std::true_type{});
  for (; t + 1 < nt; ++t) tile_body(t, std::false_type{}, std::false_type{});
  tile_body(nt - 1, std::true_type{}, std::false_type{});   // the (possibly ragged) last tile: the only body with mask code

  const int64_t qrow = q0 + r;
  if (qrow < p.d.Nq) {
    bf16_t* dqp = p.dq + b * p.dq_sb + qrow * p.dq_sn + (int64_t)head * p.dq_sh;
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        u16x4 pk;
#pragma unroll
        for (int e = 0; e < 4; ++e) pk[e] = f2bf(dqacc[d][4 * i + e] * p.scale);
        *reinterpret_cast<u16x4*>(dqp + 32 * d + 8 * i + 4 * h) = pk;
      }
  }
}

// called by lcv_attn_bwd (attn_bwd.hip) when scale * log2(e) == 1 and LCV_ATTN_BWD_VAR != 0
int attn_bwd_dq2_launch(const AttnArgs& a, hipStream_t s) {
  const char* we = lcv_knob("LCV_ATTN_BWD_DQ_WAVES");   // A/B knob: 8 = one 8-wave workgroup per CU (4 stages), 4 = two 4-wave ones
  const int nw = (we && we[0] == '8') ? 8 : 4;
  constexpr size_t STAGE = 2 * 64 * 256;   // K tile | V tile
  const size_t lds = (nw == 8 ? 4 : 2) * STAGE;
  ATTN_RAISE_LDS_ONCE("attn_bwd", attn_raise_lds((const void*)attn_bwd_dq2_kernel<8, 4>, 4 * STAGE) &&
                                      attn_raise_lds((const void*)attn_bwd_dq2_kernel<4, 2>, 2 * STAGE));
  // A/B knob LCV_ATTN_BWD_XCD=1 enables the head-per-XCD block order.  OFF by default: at the K3-TTA shapes (25 200 keys x 32
  // heads) it measured 27.06 vs 26.51 ms per layer in one process - unlike the forward, these passes are not helped by it
  const char* xe = lcv_knob("LCV_ATTN_BWD_XCD");
  const AttnGrid g = attn_grid(a.B, a.H, (a.Nq + nw * 32 - 1) / (nw * 32), xe && xe[0] == '1');
  AttnBwdDq2Params p;
  p.q = (const bf16_t*)a.q; p.k = (const bf16_t*)a.k; p.v = (const bf16_t*)a.v; p.d_o = (const bf16_t*)a.d_o;
  p.lse = a.lse; p.delta = a.delta_ws; p.dq = (bf16_t*)a.dq;
  p.d = attn_dims(a);
  p.dq_sb = a.dq_sb; p.dq_sn = a.dq_sn; p.dq_sh = a.dq_sh; p.scale = a.scale;
  p.gx = g.gx; p.xcd_remap = g.xcd_remap;
  if (nw == 8) hipLaunchKernelGGL((attn_bwd_dq2_kernel<8, 4>), g.grid, dim3(512), lds, s, p);
  else hipLaunchKernelGGL((attn_bwd_dq2_kernel<4, 2>), g.grid, dim3(256), lds, s, p);
  LCV_LAUNCH_CHECK("attn_bwd_dq2");
  return LCV_OK;
}

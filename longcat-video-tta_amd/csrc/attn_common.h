// What the attention kernels (attn_fwd*.hip, attn_bwd*.hip) share: ONE definition each of the half-wave exchange, the gap
// instructions, the K / V tile swizzle, the block order, the arguments and the internal launchers.
#pragma once
#include "lcv_common.h"

#define AS3 __attribute__((address_space(3)))
typedef AS3 unsigned char lds_u8;
typedef __attribute__((address_space(1))) void gbl_void_t;   // operand types of __builtin_amdgcn_global_load_lds
typedef AS3 void lds_void_t;
#define SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
#define ATTN_RESCALE_THR 6.0f  // log2 units: the running max may lag by up to 2^6 before O and l are rescaled

// ---- device: lane id, half-wave exchange, gap instructions ----
// The lane id re-derived from the hardware (v_mbcnt): for code after a register-hungry loop that must not keep a register live
// across it for the lane id (or for anything computed from it)
__device__ __forceinline__ int lane_now() { return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

// exchange with the partner lane (l ^ 32) by ONE v_permlane32_swap: r[0] = low-half values, r[1] = high-half values in
// every lane.  The two operands must be distinct registers (the instruction swaps halves BETWEEN them; the compiler
// folds identical operands into one register and the swap degenerates), hence the opaque copy.
__device__ __forceinline__ void half_pair(float v, float& lo, float& hi) {
  // inline asm on purpose: hipcc 7.2 folds the two results of __builtin_amdgcn_permlane32_swap into one value when
  // both operands derive from the same variable (observed: `lo + hi` became `lo + lo`).  The leading s_nop 1 covers
  // the "VALU write -> v_permlane read" hazard (2 wait states) that the compiler does not pad inside an asm string.
  float a = v, b = v;
  asm volatile("s_nop 1\n\tv_permlane32_swap_b32 %0, %1\n\ts_nop 0" : "+v"(a), "+v"(b));
  lo = a;  // [low-half value | low-half value]
  hi = b;  // [high-half value | high-half value]
}
__device__ __forceinline__ float half_max(float v) {
  float lo, hi;
  half_pair(v, lo, hi);
  return fmaxf(lo, hi);
}
__device__ __forceinline__ float half_sum(float v) {
  float lo, hi;
  half_pair(v, lo, hi);
  return lo + hi;
}

// The vector instructions of the MFMA gaps are asm volatile ON PURPOSE: hipcc's instruction selection is free to hoist a pure
// builtin (it gathered all 24 exponentials of phase 1 behind the second MFMA), while volatile statements keep their program order
// among themselves and against sched_barrier(0).  Every result is consumed at least one gap later, so no statement needs a wait
// state inside it (a transcendental's result is not read by the next instruction, an MFMA operand not written just before it).
__device__ __forceinline__ float gap_exp2(float x) { float y; asm volatile("v_exp_f32 %0, %1" : "=v"(y) : "v"(x)); return y; }
__device__ __forceinline__ float gap_add(float a, float b) { float y; asm volatile("v_add_f32 %0, %1, %2" : "=v"(y) : "v"(a), "v"(b)); return y; }
__device__ __forceinline__ float gap_max3(float a, float b, float c) { float y; asm volatile("v_max3_f32 %0, %1, %2, %3" : "=v"(y) : "v"(a), "v"(b), "v"(c)); return y; }
__device__ __forceinline__ unsigned gap_pack(float lo, float hi) { unsigned y; asm volatile("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(y) : "v"(lo), "v"(hi)); return y; }

// ---- device: the LDS image of a [rows][128] bf16 tile (K, V, Q, dO alike) ----
// 256-byte rows of sixteen 16-byte chunks; chunk ch of row `row` sits at chunk ch ^ attn_swz(row): conflict-free for row
// reads (ds_read_b128) and transposed reads (ds_read_b64_tr_b16) alike.  Every writer (staging stores, LDS-DMA source columns)
// and every reader of the family goes through these two (one marked exception: the read offsets of attn_fwd_w64.hip).
__device__ __forceinline__ int attn_swz(int row) { return ((row & 3) << 2) | ((row >> 2) & 3); }
__device__ __forceinline__ int attn_tile_off(int row, int ch) { return 256 * row + 16 * (ch ^ attn_swz(row)); }

// ---- block order: device decode and host grid ----
// Speed only, never correctness: workgroup ids are dealt round-robin over the 8 XCDs, so with the remap every XCD walks the
// blocks of ITS OWN (batch, head) pairs and that head's streamed operand (K / V for the query-block kernels: 24 MB at K3;
// Q / dO for the key-block pass) goes through one 4 MiB L2 instead of eight.  `blk` is the block index in the tile dimension.
// p: the kernel's parameter struct (gx, xcd_remap, d.H).  A macro, not a function: blockIdx is a call into the device library, and
// with the two arms in a function of their own hipcc hoists that call out of them before it inlines the function, which
// reorders the head of every kernel; as text in the kernel the code compiles as it always did.
#define ATTN_BLOCK_DECODE(p, blk, head, b)            \
  {                                                   \
    if ((p).xcd_remap) {                              \
      const int id = blockIdx.x;                      \
      const int xcd = id & 7, j = id >> 3;            \
      const int pair = (j / (p).gx) * 8 + xcd;        \
      blk = j - (j / (p).gx) * (p).gx;                \
      head = pair % (p).d.H;                          \
      b = pair / (p).d.H;                             \
    } else {                                          \
      blk = blockIdx.x; head = blockIdx.y; b = blockIdx.z; \
    }                                                 \
  }
struct AttnGrid { int gx, xcd_remap; dim3 grid; };   // gx: blocks per (batch, head)
static inline AttnGrid attn_grid(int64_t B, int64_t H, int64_t blocks, bool enabled) {
  AttnGrid g;
  g.gx = (int)blocks;
  g.xcd_remap = (enabled && (B * H) % 8 == 0 && blocks >= 8) ? 1 : 0;
  g.grid = g.xcd_remap ? dim3((unsigned)blocks * (unsigned)(H * B)) : dim3((unsigned)blocks, (unsigned)H, (unsigned)B);
  return g;
}

// ---- arguments ----
// host: what lcv_attn_fwd / lcv_attn_bwd were called with, filled once and handed to the internal launchers
struct AttnArgs {
  const void *q, *k, *v;
  void* o;             // forward: output; backward: the forward's output
  const void* d_o;
  float* lse;          // forward: output (may be null); backward: input
  float* delta_ws;     // backward: workspace (lcv_attn_bwd_ws_floats)
  void *dq, *dk, *dv;
  int64_t B, H, Nq, Nk;
  int64_t q_sb, q_sn, q_sh, k_sb, k_sn, k_sh, v_sb, v_sn, v_sh, o_sb, o_sn, o_sh;   // d_o shares o's strides
  int64_t dq_sb, dq_sn, dq_sh, dk_sb, dk_sn, dk_sh, dv_sb, dv_sn, dv_sh;
  float scale;
  int accumulate_kv;
};
// kernel side: sizes and input strides, the 120 bytes every attention kernel's parameter struct carries behind its pointers
struct AttnDims {
  int64_t Nq, Nk;
  int H;
  int64_t q_sb, q_sn, q_sh, k_sb, k_sn, k_sh, v_sb, v_sn, v_sh, o_sb, o_sn, o_sh;
};
static inline AttnDims attn_dims(const AttnArgs& a) {
  return {a.Nq, a.Nk, (int)a.H, a.q_sb, a.q_sn, a.q_sh, a.k_sb, a.k_sn, a.k_sh, a.v_sb, a.v_sn, a.v_sh, a.o_sb, a.o_sn, a.o_sh};
}
// the leading 160 bytes of the three forward kernels' parameter structs (the backward kernels' pointer lists differ from one
// another, so they share AttnDims only)
struct AttnFwdLead {
  const bf16_t* q;
  const bf16_t* k;
  const bf16_t* v;
  bf16_t* o;
  float* lse;
  AttnDims d;
};
static inline AttnFwdLead attn_fwd_lead(const AttnArgs& a) {
  return {(const bf16_t*)a.q, (const bf16_t*)a.k, (const bf16_t*)a.v, (bf16_t*)a.o, a.lse, attn_dims(a)};
}

// ---- host: launch plumbing ----
// raise a kernel's dynamic-LDS cap ONCE (function-local static: initialised on the first call, thread-safe); `ok` is the
// && of attn_raise_lds calls for every instantiation the launcher may pick
static inline bool attn_raise_lds(const void* kern, size_t bytes) {
  return hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess;
}
#define ATTN_RAISE_LDS_ONCE(name, ok)                        \
  do {                                                       \
    static const bool attr_ok__ = (ok);                      \
    if (!attr_ok__) {                                        \
      lcv_set_error("%s: cannot raise dynamic LDS", name);   \
      return LCV_EDEVICE;                                    \
    }                                                        \
  } while (0)

// the internal launchers behind lcv_attn_fwd (attn_fwd.hip) and lcv_attn_bwd (attn_bwd.hip), all for q pre-scaled into log2
// units (scale * log2(e) == 1)
int attn_fwd_w64_launch(const AttnArgs& a, bool xcd_ok, hipStream_t s);    // attn_fwd_w64.hip
int attn_fwd_pipe_launch(const AttnArgs& a, bool xcd_ok, hipStream_t s);   // attn_fwd_pipe.hip
int attn_bwd_dq2_launch(const AttnArgs& a, hipStream_t s);                 // attn_bwd_dq2.hip: pass B, second form
int attn_bwd_dkv2_launch(const AttnArgs& a, hipStream_t s);                // attn_bwd_dkv2.hip: pass A, second form

// Flash attention forward, 64 query rows per wave on ONE wave per SIMD (4 waves x 64 rows = the same 256-row block as
// attn_fwd_pipe_kernel, same 64-key tiles, same LDS images of K and V, same operand maps: S^T = K Q^T on
// v_mfma_f32_32x32x16_bf16 with the query on the lane, P^T straight from the accumulators as the B operand of O^T += V^T P^T).
//
// Why.  The ablation builds of the two-waves-per-SIMD kernel (scratch/attn_lab/build_pipe.sh ablation, profiles/r03_attn_fwd_lab.md)
// price its instruction classes at: K fragment reads 22 %, vector work 16 %, V fragment reads 14 %, LDS-DMA requests 10 % of the
// launch, against an MFMA-only loop that runs at 0.84 of the nominal peak.  Every wave of that kernel reads the WHOLE K and V tile
// from LDS for 32 query rows: 8 x 32 KiB = 256 KiB of LDS reads per 64 keys, ~2 000 of an iteration's ~3 000 cycles of LDS pipe.
// With 64 rows per wave a K fragment feeds two score MFMAs and a V^T fragment two PV MFMAs: half the LDS reads per MFMA, Q never
// leaves registers.  The price is the register file of a whole SIMD for one wave (O 128 + Q 64 accumulator registers, two score
// sets 128 + packs + fragments in arch VGPRs), i.e. nothing else issues while this wave waits.
//
// Structure (the software pipeline of attn_fwd_pipe.hip with two query blocks nb = 0, 1 per wave):
//   iteration t:   phase 1   S(t+1) = K(t+1) Q^T      32 MFMA   ||  P(t) = exp2(S(t)) elements 0-23 of both blocks, sums, packs
//                  barrier   K(t+2), V(t+1) in LDS for every wave
//                  phase 2   O += V(t)^T P(t)^T       32 MFMA   ||  elements 24-31, row max of S(t+1), 8 LDS-DMA requests of
//                                                                   K(t+3) / V(t+2), first fragments of K(t+2)
//                  (the first PD + 1 fragments of V(t) are read in the last gaps of phase 1: V(t) landed a barrier earlier)
//                  post      rare: rescale O, l and S(t+1) of a block whose running max grew by more than 2^RESCALE_THR
// MFMAs are issued from asm with the register class pinned (score sets in arch VGPRs, O in AGPRs, Q fragments as AGPR B
// operands): left alone hipcc puts every MFMA result of a > 256-register kernel into AGPRs (round 3, scratch/tried/attn_bwd_dkv3_r3_one_wave_per_simd.hip.txt).  asm is opaque
// to the hazard recogniser: see GUARD below and profiles/r03_attn_bwd_lab.md for the four ways that went wrong before.
#include "attn_common.h"
#include <type_traits>

struct AttnFwdW64Params : AttnFwdLead {
  float scale;
  int gx, xcd_remap;
};

// ---- the gap table of the steady loop: what follows each MFMA of phase 1 (score MFMA i) and phase 2 (PV MFMA j) ----
// At one wave per SIMD a v_mfma_f32_32x32x16_bf16 hides about 5 single-issue instructions / 24 issue-cycles with at most one
// 8-cycle transcendental (MI355X issue-cost constants: v_exp 8, v_cvt_pk 5, the rest 4).  An iteration carries more than the
// 64 gaps can hide once the row sums are scalar (64 exp, 32 pack, 64 add, 32 max3, 48 fragment reads and their waits, 8 DMA
// pieces, 8 offset moves: ~1 560 issue-cycles against 64 x 24), so the table spreads the load: 3 exps per 2 gaps in phase 1
// with the pair on the read-free (even) gaps.  Phase 2 is laid out level: gap 0 holds one exp only, its DMA pieces sit on the
// read-free even gaps 2..16 with what their compiled scalar extras leave room for, its exps run one per gap over gaps 0..11 and
// 18..22 (the last pack two gaps ahead of the PV MFMA that reads it), and the two row-max chains run one behind the other (block
// 0 in gaps 12..22, block 1 in gaps 19..27) so that no odd gap carries two max steps; the row sums of elements 28..31, the half
// exchanges and the ballots fill the tail.  tools/mfma_gaps.py prices the compiler's output gap by gap;
// tests/test_attn_fwd_gap_budget.py and tests/test_attn_fwd_gap_level.py hold it there.
// Order inside a gap is the order of the entries: packs / adds of earlier exps first, the gap's own exps last, and every pack
// far ahead of the PV MFMA that reads it.  Every odd gap OPENS with the fragment read that the MFMA after it used to ask for (its
// ring slot is free: the MFMA in front of the gap was the last to read it) and closes with the wait of an earlier one.  Those
// two are what keeps hipcc from padding the adds and packs with s_nops: see w64_apart below.
template <int I, int N, class F>
__device__ __forceinline__ void w64_static_for(F&& f) {
  if constexpr (I < N) { f(std::integral_constant<int, I>{}); w64_static_for<I + 1, N>(f); }
}
enum : unsigned char { W64_NONE, W64_EXP, W64_ADD, W64_PACK, W64_LRUN, W64_VOFF, W64_MAX, W64_HCPY, W64_HSWAP, W64_HMAX, W64_BALLOT, W64_M0, W64_DMA };
struct W64Op { unsigned char kind, b, e; };   // b: query block (or DMA piece / offset index), e: element / pair / max step
constexpr int W64_SLOTS = 6;
// EXP b e: ex[b][e] = exp2(S(t)[b][e]) | ADD b e: psum[b] += ex[b][e] (e = 1: psum = ex[0] + ex[1]), the two-wave kernel's
// order | PACK b m: pw[b][m] = bf16(ex[b][2m], ex[b][2m+1]) | LRUN b: l_run[b] += psum[b] | VOFF k: V read offset k to tile
// t's slot | MAX b s: step s of block b's two max3 chains over S(t+1) | HCPY b, HSWAP b, HMAX b: the exchange with the partner
// half as three entries (copy, v_permlane32_swap, max: half_max() of attn_common.h, its wait states covered by table work:
// w64_issues_between) | BALLOT b: rescale test | M0 d / DMA d: LDS destination and request of DMA piece d (d < 4: K(t+3), else V(t+2)), one gap apart or more
// (the number after each row: the gap's issue-cycles at the prices above, its fragment read and wait included)
constexpr W64Op W64_P1[32][W64_SLOTS] = {
  {{W64_EXP, 0, 0}, {W64_EXP, 1, 0}},   //  0: 16
  {{W64_EXP, 0, 1}},   //  1: 16
  {{W64_PACK, 0, 0}, {W64_ADD, 0, 1}, {W64_EXP, 1, 1}, {W64_EXP, 0, 2}},   //  2: 25
  {{W64_ADD, 0, 2}, {W64_PACK, 1, 0}, {W64_ADD, 1, 1}, {W64_EXP, 1, 2}},   //  3: 29
  {{W64_ADD, 1, 2}, {W64_EXP, 0, 3}, {W64_EXP, 1, 3}},   //  4: 20
  {{W64_PACK, 0, 1}, {W64_ADD, 0, 3}, {W64_PACK, 1, 1}, {W64_ADD, 1, 3}, {W64_EXP, 0, 4}},   //  5: 34
  {{W64_ADD, 0, 4}, {W64_EXP, 1, 4}, {W64_EXP, 0, 5}},   //  6: 20
  {{W64_PACK, 0, 2}, {W64_ADD, 0, 5}, {W64_ADD, 1, 4}, {W64_EXP, 1, 5}},   //  7: 29
  {{W64_PACK, 1, 2}, {W64_ADD, 1, 5}, {W64_EXP, 0, 6}, {W64_EXP, 1, 6}},   //  8: 25
  {{W64_ADD, 0, 6}, {W64_ADD, 1, 6}, {W64_EXP, 0, 7}},   //  9: 24
  {{W64_VOFF, 0, 0}, {W64_PACK, 0, 3}, {W64_ADD, 0, 7}, {W64_EXP, 1, 7}, {W64_EXP, 0, 8}},   // 10: 29
  {{W64_VOFF, 1, 0}, {W64_ADD, 0, 8}, {W64_PACK, 1, 3}, {W64_ADD, 1, 7}, {W64_EXP, 1, 8}},   // 11: 33
  {{W64_VOFF, 2, 0}, {W64_ADD, 1, 8}, {W64_EXP, 0, 9}, {W64_EXP, 1, 9}},   // 12: 24
  {{W64_VOFF, 3, 0}, {W64_PACK, 0, 4}, {W64_ADD, 0, 9}, {W64_PACK, 1, 4}, {W64_ADD, 1, 9}, {W64_EXP, 0, 10}},   // 13: 38
  {{W64_VOFF, 4, 0}, {W64_ADD, 0, 10}, {W64_EXP, 1, 10}, {W64_EXP, 0, 11}},   // 14: 24
  {{W64_VOFF, 5, 0}, {W64_PACK, 0, 5}, {W64_ADD, 0, 11}, {W64_ADD, 1, 10}, {W64_EXP, 1, 11}},   // 15: 33
  {{W64_VOFF, 6, 0}, {W64_PACK, 1, 5}, {W64_ADD, 1, 11}, {W64_EXP, 0, 12}, {W64_EXP, 1, 12}},   // 16: 29
  {{W64_VOFF, 7, 0}, {W64_ADD, 0, 12}, {W64_ADD, 1, 12}, {W64_EXP, 0, 13}},   // 17: 28
  {{W64_PACK, 0, 6}, {W64_ADD, 0, 13}, {W64_EXP, 1, 13}, {W64_EXP, 0, 14}},   // 18: 25
  {{W64_ADD, 0, 14}, {W64_PACK, 1, 6}, {W64_ADD, 1, 13}, {W64_EXP, 1, 14}},   // 19: 29
  {{W64_ADD, 1, 14}, {W64_EXP, 0, 15}, {W64_EXP, 1, 15}},   // 20: 20
  {{W64_PACK, 0, 7}, {W64_ADD, 0, 15}, {W64_PACK, 1, 7}, {W64_ADD, 1, 15}, {W64_EXP, 0, 16}},   // 21: 34
  {{W64_ADD, 0, 16}, {W64_EXP, 1, 16}, {W64_EXP, 0, 17}},   // 22: 20
  {{W64_PACK, 0, 8}, {W64_ADD, 0, 17}, {W64_ADD, 1, 16}, {W64_EXP, 1, 17}},   // 23: 29
  {{W64_PACK, 1, 8}, {W64_ADD, 1, 17}, {W64_EXP, 0, 18}, {W64_EXP, 1, 18}},   // 24: 25
  {{W64_ADD, 0, 18}, {W64_ADD, 1, 18}, {W64_EXP, 0, 19}},   // 25: 24
  {{W64_PACK, 0, 9}, {W64_ADD, 0, 19}, {W64_EXP, 1, 19}, {W64_EXP, 0, 20}},   // 26: 25
  {{W64_ADD, 0, 20}, {W64_PACK, 1, 9}, {W64_ADD, 1, 19}, {W64_EXP, 1, 20}},   // 27: 33
  {{W64_ADD, 1, 20}, {W64_EXP, 0, 21}, {W64_EXP, 1, 21}},   // 28: 20
  {{W64_PACK, 0, 10}, {W64_ADD, 0, 21}, {W64_PACK, 1, 10}, {W64_ADD, 1, 21}, {W64_EXP, 0, 22}},   // 29: 38
  {{W64_ADD, 0, 22}, {W64_EXP, 1, 22}, {W64_EXP, 0, 23}},   // 30: 20
  {{W64_PACK, 0, 11}, {W64_ADD, 0, 23}, {W64_ADD, 1, 22}, {W64_EXP, 1, 23}},   // 31: 29
};
constexpr W64Op W64_P2[32][W64_SLOTS] = {
  {{W64_EXP, 0, 24}},   //  0: 8
  {{W64_ADD, 1, 23}, {W64_EXP, 1, 24}},   //  1: 24
  {{W64_M0, 0, 0}, {W64_EXP, 0, 25}, {W64_DMA, 0, 0}},   //  2: 16
  {{W64_ADD, 0, 24}, {W64_EXP, 1, 25}},   //  3: 24
  {{W64_M0, 1, 0}, {W64_PACK, 1, 11}, {W64_ADD, 0, 25}, {W64_EXP, 0, 26}, {W64_DMA, 1, 0}},   //  4: 25
  {{W64_ADD, 1, 24}, {W64_EXP, 1, 26}},   //  5: 24
  {{W64_M0, 2, 0}, {W64_PACK, 0, 12}, {W64_EXP, 0, 27}, {W64_DMA, 2, 0}},   //  6: 21
  {{W64_ADD, 1, 25}, {W64_EXP, 1, 27}},   //  7: 24
  {{W64_M0, 3, 0}, {W64_ADD, 0, 26}, {W64_EXP, 0, 28}, {W64_DMA, 3, 0}},   //  8: 20
  {{W64_PACK, 1, 12}, {W64_EXP, 1, 28}},   //  9: 25
  {{W64_M0, 4, 0}, {W64_ADD, 0, 27}, {W64_DMA, 4, 0}},   // 10: 12
  {{W64_ADD, 1, 26}, {W64_EXP, 0, 29}},   // 11: 24
  {{W64_M0, 5, 0}, {W64_MAX, 0, 0}, {W64_DMA, 5, 0}},   // 12: 16
  {{W64_PACK, 0, 13}, {W64_MAX, 0, 1}},   // 13: 25
  {{W64_M0, 6, 0}, {W64_MAX, 0, 2}, {W64_DMA, 6, 0}},   // 14: 16
  {{W64_PACK, 1, 13}, {W64_MAX, 0, 3}},   // 15: 25
  {{W64_M0, 7, 0}, {W64_MAX, 0, 4}, {W64_DMA, 7, 0}},   // 16: 16
  {{W64_ADD, 0, 28}, {W64_MAX, 0, 5}},   // 17: 24
  {{W64_PACK, 0, 14}, {W64_ADD, 1, 27}, {W64_MAX, 0, 6}, {W64_EXP, 1, 29}},   // 18: 25
  {{W64_MAX, 1, 0}, {W64_EXP, 0, 30}},   // 19: 28
  {{W64_PACK, 1, 14}, {W64_MAX, 0, 7}, {W64_MAX, 1, 1}, {W64_EXP, 1, 30}},   // 20: 25
  {{W64_MAX, 1, 2}, {W64_EXP, 0, 31}},   // 21: 28
  {{W64_PACK, 0, 15}, {W64_MAX, 0, 8}, {W64_MAX, 1, 3}, {W64_EXP, 1, 31}},   // 22: 25
  {{W64_PACK, 1, 15}, {W64_MAX, 1, 4}},   // 23: 25
  {{W64_ADD, 0, 29}, {W64_ADD, 1, 28}, {W64_HCPY, 0, 0}, {W64_MAX, 1, 5}},   // 24: 20
  {{W64_ADD, 0, 30}, {W64_MAX, 1, 6}},   // 25: 24
  {{W64_ADD, 0, 31}, {W64_ADD, 1, 29}, {W64_MAX, 1, 7}, {W64_HSWAP, 0, 0}},   // 26: 16
  {{W64_ADD, 1, 30}, {W64_MAX, 1, 8}, {W64_HMAX, 0, 0}},   // 27: 20
  {{W64_LRUN, 0, 0}, {W64_ADD, 1, 31}, {W64_BALLOT, 0, 0}, {W64_HCPY, 1, 0}},   // 28: 16
  {{W64_HSWAP, 1, 0}},   // 29: 12
  {{W64_LRUN, 1, 0}, {W64_HMAX, 1, 0}},   // 30: 8
  {{W64_BALLOT, 1, 0}},   // 31: 4
};
// issue-cycle price of a table entry, and of the fragment read at the head of an odd gap i and the wait at its end
constexpr int w64_op_cost(W64Op o) {
  return o.kind == W64_EXP ? 8 : o.kind == W64_PACK ? 5 : o.kind == W64_MAX ? (o.e < 7 ? 8 : 4) : o.kind == W64_NONE ? 0 : 4;
}
constexpr bool w64_read_first(int phase, int i) { return (i & 1) && (phase == 1 || i <= 29); }   // a fragment read opens the gap
constexpr bool w64_wait_last(int phase, int i) { return (i & 1) && (phase == 1 || i <= 29); }    // a wait (phase 1, gap 31: the barrier's) closes it
constexpr int w64_read_cost(int phase, int i) {
  const bool v = phase == 1 ? i >= 27 : i <= 25;   // a V^T fragment is two ds_read_b64_tr_b16, a K fragment one ds_read_b128
  return (w64_read_first(phase, i) ? (v ? 8 : 4) : 0) + (w64_wait_last(phase, i) && i <= 29 ? 4 : 0);
}
constexpr bool w64_table_ok(const W64Op (&t)[32][W64_SLOTS], int phase, int max_cyc, int max_exp) {
  for (int i = 0; i < 32; ++i) {
    int c = w64_read_cost(phase, i), ex = 0;
    for (int s = 0; s < W64_SLOTS; ++s) { c += w64_op_cost(t[i][s]); ex += t[i][s].kind == W64_EXP; }
    if (c > max_cyc || ex > max_exp) return false;
  }
  return true;
}
// hipcc pads a gap statement that reads the result of another one with an s_nop unless an instruction of ITS OWN stands between
// the two: asm statements, the MFMA included, count for nothing there, however many they are.  The loop's only such instructions
// are the fragment reads and their waits, so a result is read no sooner than behind the next of those.  Positions are 8 gap + slot.
constexpr bool w64_apart(int from, int to) {
  const int gf = from / 8, gt = to / 8;
  for (int g = gf; g <= gt; ++g) {
    const int ph = g < 32 ? 1 : 2, i = g & 31;
    if ((g > gf && w64_read_first(ph, i)) || (g < gt && w64_wait_last(ph, i))) return true;
  }
  return false;
}
// instructions issued between two table positions: table entries (a MAX step below 7 is two), the MFMAs, the fragment reads
// (a V^T fragment counted once) and the waits.  v_permlane32_swap needs 2 wait states behind a VALU write of either operand.
constexpr int w64_issues_between(int from, int to) {
  int n = 0;
  for (int at = from + 1; at < to; ++at) {
    const int g = at / 8, s = at % 8, ph = g < 32 ? 1 : 2, i = g & 31;
    if (s < W64_SLOTS) { const W64Op o = ph == 1 ? W64_P1[i][s] : W64_P2[i][s]; n += o.kind == W64_NONE ? 0 : (o.kind == W64_MAX && o.e < 7) ? 2 : 1; }
    if (s == W64_SLOTS && w64_wait_last(ph, i)) ++n;
    if (s == W64_SLOTS + 1) n += 1 + (w64_read_first(g + 1 < 32 ? 1 : 2, (g + 1) & 31) ? 1 : 0);   // the MFMA, the next gap's read
  }
  return n;
}
constexpr bool w64_table_complete() {   // every exp, add, pack exactly once; each after what it reads, and no s_nop in front of it
  int exp_at[2][32] = {}, add_at[2][32] = {}, pack_at[2][16] = {}, max_at[2][9] = {}, cpy_at[2] = {-1, -1}, swap_at[2] = {-1, -1}, hmax_at[2] = {-1, -1}, n = 0;
  for (int b = 0; b < 2; ++b) for (int m = 0; m < 9; ++m) max_at[b][m] = -1;
  for (int b = 0; b < 2; ++b) for (int e = 0; e < 32; ++e) { exp_at[b][e] = -1; add_at[b][e] = -1; }
  for (int b = 0; b < 2; ++b) for (int m = 0; m < 16; ++m) pack_at[b][m] = -1;
  for (int g = 0; g < 64; ++g)
    for (int s = 0; s < W64_SLOTS; ++s) {
      const W64Op o = g < 32 ? W64_P1[g][s] : W64_P2[g - 32][s];
      const int at = 8 * g + s;
      if (o.kind == W64_EXP) { if (exp_at[o.b][o.e] >= 0) return false; exp_at[o.b][o.e] = at; ++n; }
      if (o.kind == W64_ADD) { if (o.e == 0 || exp_at[o.b][o.e] < 0 || (o.e > 1 && add_at[o.b][o.e - 1] < 0)) return false; add_at[o.b][o.e] = at; }
      if (o.kind == W64_PACK) { if (exp_at[o.b][2 * o.e] < 0 || exp_at[o.b][2 * o.e + 1] < 0) return false; pack_at[o.b][o.e] = at; }
      if (o.kind == W64_LRUN && add_at[o.b][31] < 0) return false;
      if (o.kind == W64_MAX) { if (o.e > 0 && max_at[o.b][o.e - 1] < 0) return false; max_at[o.b][o.e] = at; }
      if (o.kind == W64_HCPY) { if (max_at[o.b][8] < 0 || cpy_at[o.b] >= 0) return false; cpy_at[o.b] = at; }
      if (o.kind == W64_HSWAP) { if (cpy_at[o.b] < 0 || swap_at[o.b] >= 0) return false; swap_at[o.b] = at; }
      if (o.kind == W64_HMAX) { if (swap_at[o.b] < 0 || hmax_at[o.b] >= 0) return false; hmax_at[o.b] = at; }
      if (o.kind == W64_BALLOT && hmax_at[o.b] < 0) return false;
      if (o.kind == W64_ADD && !(w64_apart(exp_at[o.b][o.e], at) && w64_apart(o.e == 1 ? exp_at[o.b][0] : add_at[o.b][o.e - 1], at))) return false;
      if (o.kind == W64_PACK && !(w64_apart(exp_at[o.b][2 * o.e], at) && w64_apart(exp_at[o.b][2 * o.e + 1], at))) return false;
      if (o.kind == W64_LRUN && !w64_apart(add_at[o.b][31], at)) return false;
      if (o.kind == W64_MAX && o.e > 0 && !w64_apart(max_at[o.b][o.e - 1], at)) return false;
      if (o.kind == W64_HCPY && !w64_apart(max_at[o.b][8], at)) return false;
      if (o.kind == W64_HSWAP && !(w64_apart(cpy_at[o.b], at) && w64_issues_between(cpy_at[o.b], at) >= 2 && w64_issues_between(max_at[o.b][8], at) >= 2)) return false;
      if (o.kind == W64_HMAX && !w64_apart(swap_at[o.b], at)) return false;
    }
  for (int b = 0; b < 2; ++b)
    for (int m = 0; m < 16; ++m)   // pack of k-step m / 4 before PV MFMA 8 (m / 4) + b of phase 2 (MFMA j follows gap j - 1)
      if (pack_at[b][m] < 0 || pack_at[b][m] >= 8 * (32 + 8 * (m / 4) + b - 1) + W64_SLOTS) return false;
  return n == 64 && hmax_at[0] >= 0 && hmax_at[1] >= 0;
}
static_assert(w64_table_complete(), "attn_fwd_w64 gap table: an exp, add or pack is missing, doubled, out of order or right behind what it reads");
static_assert(w64_table_ok(W64_P1, 1, 38, 2) && w64_table_ok(W64_P2, 2, 28, 1), "attn_fwd_w64 gap table over its budget");

// GUARD: wait states in front of the MFMA wherever hipcc may have placed a register copy of one of its operands right before the
// statement: everywhere outside the straight-line steady loop.  Inside it the first MFMAs of a phase carried the guard too (16
// cycles each); the compiled loop has no operand copy there (a fragment read and its wait, or the barrier, stand in front of
// them, and the rare rescale path ends in fence_o), and tests/test_isa_hazards.py fails on the build that places one.
template <bool GUARD>
__device__ __forceinline__ void mfma_s(f32x16& c, const bf16x8& a, const bf16x8& b) {   // score chain link: VGPR accumulator, B in AGPRs
  if constexpr (GUARD) asm volatile("s_nop 3\n\tv_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(c) : "v"(a), "a"(b));
  else asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+v"(c) : "v"(a), "a"(b));
}
template <bool GUARD>
__device__ __forceinline__ void mfma_s_first(f32x16& d, const f32x16& c, const bf16x8& a, const bf16x8& b) {   // D != C: the resident -max tuple survives
  if constexpr (GUARD) asm volatile("s_nop 3\n\tv_mfma_f32_32x32x16_bf16 %0, %2, %3, %1" : "=&v"(d) : "v"(c), "v"(a), "a"(b));
  else asm volatile("v_mfma_f32_32x32x16_bf16 %0, %2, %3, %1" : "=&v"(d) : "v"(c), "v"(a), "a"(b));
}
template <bool GUARD>
__device__ __forceinline__ void mfma_o(f32x16& c, const bf16x8& a, const bf16x8& b) {   // O^T accumulator in AGPRs
  if constexpr (GUARD) asm volatile("s_nop 3\n\tv_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+a"(c) : "v"(a), "v"(b));
  else asm volatile("v_mfma_f32_32x32x16_bf16 %0, %1, %2, %0" : "+a"(c) : "v"(a), "v"(b));
}

// element j (0..31) of the 64 scores a lane holds for one tile and one query block: j < 16 -> key block 0, else key block 1
#define SCW(S, nb, j) (S[(j) >> 4][nb][(j) & 15])

__global__ __launch_bounds__(256) void attn_fwd_w64_kernel(const AttnFwdW64Params p) {
  constexpr int TILE = 64 * 256;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  lds_u8* lds = (lds_u8*)smem;  // K buffers 0, 1 | V buffers 0, 1, 2
  constexpr int V_REGION = 2 * TILE;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = lane & 31, h = lane >> 5;
  int qb, head;
  int64_t b;
  ATTN_BLOCK_DECODE(p, qb, head, b);   // head-per-XCD block order (speed only)
  const int64_t q0 = (int64_t)qb * 256 + wave * 64;
  const int nt = (int)((p.d.Nk + 63) / 64);
  const bool ragged = (p.d.Nk & 63) != 0;
  const char* kbase_u = lcv_uniform_ptr(p.k + b * p.d.k_sb + (int64_t)head * p.d.k_sh);
  const char* vbase_u = lcv_uniform_ptr(p.v + b * p.d.v_sb + (int64_t)head * p.d.v_sh);

  // ---- LDS-DMA roles: wave w fills rows 16 w .. 16 w + 15 of a tile with four 1-KiB requests (scalar tile base + a constant
  // per-lane 32-bit byte offset: row 16 w + 4 i + (lane >> 4), swizzled 16-byte column) ----
  auto dma_row_of = [&](int ln, int i) { return 16 * wave + 4 * i + (ln >> 4); };
  auto dma_colb_of = [&](int ln, int i) {
    const int row = dma_row_of(ln, i);
    return 16 * ((ln & 15) ^ attn_swz(row));
  };
  unsigned koff[4], voff[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    koff[i] = (unsigned)(dma_row_of(lane, i) * p.d.k_sn * 2 + dma_colb_of(lane, i));
    voff[i] = (unsigned)(dma_row_of(lane, i) * p.d.v_sn * 2 + dma_colb_of(lane, i));
  }
  auto last_off = [&](int i, int64_t sn) {   // the last tile's rows past Nk re-read the last key (their scores are masked)
    const int ln = lane_now();
    int64_t row = (int64_t)(nt - 1) * 64 + dma_row_of(ln, i);
    if (row > p.d.Nk - 1) row = p.d.Nk - 1;
    return (unsigned)(row * sn * 2 + dma_colb_of(ln, i));
  };
  const unsigned lds_wave = (unsigned)(uintptr_t)lds + (unsigned)wave * 4096u;   // this wave's 4 KiB slice of every tile
  // piece i (0..3) of tile `tile` of K (which = 0) or V (which = 1) to the buffer at LDS byte offset `dst_tile`
  // (which / i are plain ints that fold once the calling loop is unrolled: ONE copy of this body per gap, or the unroller gives up)
  auto dma_one = [&](int which, int i, int dst_tile, int tile, bool known_full) __attribute__((always_inline)) {
    const int64_t sn = which ? p.d.v_sn : p.d.k_sn;
    const char* base = which ? vbase_u : kbase_u;
    unsigned off = which ? voff[i] : koff[i];
    if (!known_full && tile == nt - 1) off = last_off(i, sn);
    else base += (int64_t)tile * (128 * sn);
    // (M0 carries the LDS destination; nothing else in this kernel uses it, so it is declared clobbered instead of saved and
    // restored around every request: two scalar instructions less per request on a wave whose issue slots are the budget)
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1"
                 :: "v"(off), "s"(base), "s"(lds_wave + (unsigned)dst_tile + 1024u * i) : "memory", "m0");
  };
  // the same request in two statements, for the steady loop: the m0 write one or more instructions ahead of the request (the
  // one wait state an LDS-DMA needs after an m0 write is then already there: no s_nop)
  auto dma_m0 = [&](int i, int dst_tile) __attribute__((always_inline)) {
    asm volatile("s_mov_b32 m0, %0" :: "s"(lds_wave + (unsigned)dst_tile + 1024u * i) : "memory", "m0");
  };
  auto dma_req = [&](int which, int i, int tile, bool known_full) __attribute__((always_inline)) {
    const int64_t sn = which ? p.d.v_sn : p.d.k_sn;
    const char* base = which ? vbase_u : kbase_u;
    unsigned off = which ? voff[i] : koff[i];
    if (!known_full && tile == nt - 1) off = last_off(i, sn);
    else base += (int64_t)tile * (128 * sn);
    asm volatile("global_load_lds_dwordx4 %0, %1" :: "v"(off), "s"(base) : "memory");
  };
  auto dma_tile = [&](int which, int dst_tile, int tile) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 4; ++i) dma_one(which, i, dst_tile, tile, false);
  };
  constexpr int KOP = 0, VOP = 1;
  auto dma_wait_and_barrier = [&]() { asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory"); };

  // ---- per-lane LDS read offsets (the images of attn_fwd_pipe.hip) ----
  int k_off[8];
  int v_off[2][4];
  auto set_read_offsets = [&](int ln, int slot) {
    const int rr = ln & 31, hh = ln >> 5;
    const int kfz = ((rr & 3) << 2) | ((rr >> 2) & 3);   // = attn_swz(rr), written out: through the function this kernel allocates its registers differently
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) k_off[ks] = 256 * rr + 16 * ((2 * ks + hh) ^ kfz);
    const int q4 = (ln >> 2) & 3, p4 = ln & 3, g1 = (ln >> 4) & 1;
#pragma unroll
    for (int half = 0; half < 2; ++half)
#pragma unroll
      for (int d = 0; d < 4; ++d)
        v_off[half][d] = (int)(unsigned)(uintptr_t)lds + V_REGION + slot * TILE + 256 * (4 * hh + 8 * half + q4) + 8 * (p4 & 1) + 64 * (d ^ q4) +
                         16 * ((2 * g1 + (p4 >> 1)) ^ (hh + 2 * half));   // ABSOLUTE LDS byte address: no base add per read
  };
  set_read_offsets(lane, 2);   // (V slot 2: iteration 0 rotates the offsets to slot 0)
  auto read_k = [&](const lds_u8* kb, int f) __attribute__((always_inline)) -> bf16x8 {   // K fragment f: k-step f >> 1, key block f & 1
    return *reinterpret_cast<const AS3 bf16x8*>(kb + (f & 1) * 32 * 256 + k_off[f >> 1]);
  };
  auto read_v = [&](int g) __attribute__((always_inline)) -> bf16x8 {   // V^T fragment g: k-step g >> 2, dim block g & 3, of the slot the offsets point at
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((AS3 s16x4*)(uintptr_t)(unsigned)(v_off[0][g & 3] + 4096 * (g >> 2)));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((AS3 s16x4*)(uintptr_t)(unsigned)(v_off[1][g & 3] + 4096 * (g >> 2)));
    return __builtin_bit_cast(bf16x8, __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7));
  };

  // Q fragments (B operands of the score MFMAs), resident in AGPRs for the whole sweep: qf[nb][ks] = Q[q0 + 32 nb + r][16 ks + 8 h ..]
  bf16x8 qf[2][8];
#pragma unroll
  for (int nb = 0; nb < 2; ++nb) {
    int64_t qrow = q0 + 32 * nb + r;
    if (qrow > p.d.Nq - 1) qrow = p.d.Nq - 1;
    const bf16_t* qp = p.q + b * p.d.q_sb + qrow * p.d.q_sn + (int64_t)head * p.d.q_sh + 8 * h;
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) qf[nb][ks] = *reinterpret_cast<const bf16x8*>(qp + 16 * ks);
  }
#pragma unroll
  for (int nb = 0; nb < 2; ++nb)
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) asm volatile("" : "+a"(qf[nb][ks]));   // into AGPRs here, far from the first MFMA that reads them

  f32x16 oacc[2][4];   // [query block][dim block]
#pragma unroll
  for (int nb = 0; nb < 2; ++nb)
#pragma unroll
    for (int d = 0; d < 4; ++d) {
#pragma unroll
      for (int e = 0; e < 16; ++e) oacc[nb][d][e] = 0.f;
      asm volatile("" : "+a"(oacc[nb][d]));
    }
  float m_run[2] = {0.f, 0.f}, l_run[2] = {0.f, 0.f};
  f32x16 minit[2];   // -m_run of a query block in every element: the C operand of its chains' first MFMAs
#pragma unroll
  for (int nb = 0; nb < 2; ++nb)
#pragma unroll
    for (int e = 0; e < 16; ++e) minit[nb][e] = 0.f;
  f32x16 sa[2][2], sb[2][2];   // score sets A and B: [key block][query block]

  auto mask_last = [&](f32x16 (&s)[2][2]) __attribute__((always_inline)) {   // scores of the ragged last tile past Nk -> -inf
    const int valid = (int)(p.d.Nk - (int64_t)(nt - 1) * 64);
    const int hh_ = lane_now() >> 5;
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int key = (e & 3) + 8 * (e >> 2) + 4 * hh_;
        if (key >= valid) s[0][nb][e] = -INFINITY;
        if (key + 32 >= valid) s[1][nb][e] = -INFINITY;
      }
  };
  // all accumulators through one statement that carries wait states: whatever hipcc does with them next (copies for a join,
  // v_accvgpr_read for the rescale) sits behind the MFMAs' write-back
  auto fence_o = [&]() __attribute__((always_inline)) {
    asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15"
                 : "+a"(oacc[0][0]), "+a"(oacc[0][1]), "+a"(oacc[0][2]), "+a"(oacc[0][3]), "+a"(oacc[1][0]), "+a"(oacc[1][1]),
                   "+a"(oacc[1][2]), "+a"(oacc[1][3]));
  };
  auto fence_s = [&](f32x16 (&s)[2][2]) __attribute__((always_inline)) {
    asm volatile("s_nop 15\n\ts_nop 15\n\ts_nop 15\n\ts_nop 15" : "+v"(s[0][0]), "+v"(s[0][1]), "+v"(s[1][0]), "+v"(s[1][1]));
  };
  // row max of a query block's score tile relative to its running max, and the (rare) rescale it may trigger
  auto settle = [&](f32x16 (&s)[2][2], auto nb_c, float mx, bool first, bool need) __attribute__((always_inline)) {
    constexpr int nb = decltype(nb_c)::value;
    if (need || first) {   // need: some lane's row max exceeds the threshold (a ballot the caller took inside an MFMA gap)
      fence_o();
      const float d = first ? mx : fmaxf(mx, 0.f);
      const float alpha = __builtin_amdgcn_exp2f(-d);
      m_run[nb] += d;
      l_run[nb] *= alpha;
#pragma unroll
      for (int dd = 0; dd < 4; ++dd)
#pragma unroll
        for (int e = 0; e < 16; ++e) oacc[nb][dd][e] *= alpha;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        s[0][nb][e] -= d;
        s[1][nb][e] -= d;
        // an in-place update as far as hipcc can tell: a fresh splat here made it copy the whole tuple (8 v_mov_b64 per query
        // block) on the COMMON path of every iteration to merge the two versions
        asm volatile("v_mov_b32 %0, %1" : "+v"(minit[nb][e]) : "v"(-m_run[nb]));
      }
      fence_o();
    }
  };

#ifndef W64_PD
#define W64_PD 2
#endif
  constexpr int PD = W64_PD, RING = PD + 1;   // fragments are requested PD fragments (= 2 PD MFMAs) ahead of their first use
  bf16x8 kfr[RING], vfr[RING];
  int v_slot = 2;
  auto next_v_slot = [&]() __attribute__((always_inline)) -> int {
    v_slot = (v_slot == 2) ? 0 : v_slot + 1;
    return (v_slot == 0) ? -2 * TILE : TILE;
  };

  // ---- prologue: K(0), V(0), K(1), V(1) requested; S(0) computed plainly and settled; then K(2) into K(0)'s buffer ----
  dma_tile(KOP, 0, 0);                  // (the launcher guarantees nt >= 6)
  dma_tile(VOP, V_REGION, 0);
  dma_tile(KOP, TILE, 1);
  dma_tile(VOP, V_REGION + TILE, 1);
  dma_wait_and_barrier();
  {
#pragma unroll
    for (int kb_ = 0; kb_ < 2; ++kb_)
#pragma unroll
      for (int nb = 0; nb < 2; ++nb)
#pragma unroll
        for (int e = 0; e < 16; ++e) sa[kb_][nb][e] = 0.f;
#pragma unroll
    for (int f = 0; f < 16; ++f) {
      const bf16x8 a = read_k(lds, f);
      mfma_s<true>(sa[f & 1][0], a, qf[0][f >> 1]);
      mfma_s<true>(sa[f & 1][1], a, qf[1][f >> 1]);
    }
    fence_s(sa);
    auto first_settle = [&](auto nb_c) __attribute__((always_inline)) {
      constexpr int nb = decltype(nb_c)::value;
      float mx = sa[0][nb][0];
#pragma unroll
      for (int e = 1; e < 16; ++e) mx = fmaxf(mx, sa[0][nb][e]);
#pragma unroll
      for (int e = 0; e < 16; ++e) mx = fmaxf(mx, sa[1][nb][e]);
      settle(sa, nb_c, half_max(mx), true, true);
    };
    first_settle(std::integral_constant<int, 0>{});
    first_settle(std::integral_constant<int, 1>{});
  }
  __syncthreads();                        // every wave has read K(0)
  dma_tile(KOP, 0, 2);                  // K(2) -> K buffer 0; waited for at the barrier of iteration 0
#pragma unroll
  for (int i = 0; i < PD; ++i) kfr[i] = read_k(lds + TILE, i);   // first fragments of K(1): what an iteration expects

  // ---- one pipelined iteration.  PAR = t & 1: K(t+1) in K buffer PAR ^ 1, K(t+2) in buffer PAR, K(t+3) requested into buffer
  // PAR ^ 1 after the barrier; V(t) in slot t % 3, V(t+2) requested into slot (t + 2) % 3.  c = S(t), settled; n receives S(t+1).
  // STEADY: tiles up to t + 3 exist and are full, no edge condition is evaluated and the code is straight-line.
  auto iteration = [&](const int t, auto par_c, auto steady_c, f32x16 (&c)[2][2], f32x16 (&n)[2][2]) __attribute__((always_inline)) {
    constexpr int PAR = decltype(par_c)::value;
    constexpr bool STEADY = decltype(steady_c)::value;
    const lds_u8* kb = lds + (PAR ^ 1) * TILE;      // K(t+1)
    const lds_u8* kb_next = lds + PAR * TILE;        // K(t+2)
    const bool has_k3 = STEADY || t + 3 < nt;
    const bool has_v2 = STEADY || t + 2 < nt;
    const int v_delta = next_v_slot();                // v_slot == t % 3 from here on
    const int v_dst = V_REGION + ((v_slot == 0) ? 2 : v_slot - 1) * TILE;   // slot (t + 2) % 3
    float psum[2];        // row sums of P(t), one chain per query block in element order (attn_fwd_pipe.hip's order)
    float ex[2][32];      // P(t) in fp32
    unsigned pw[2][16];   // P(t) as packed bf16 pairs: word m = elements (2m, 2m + 1)
    float mxa[2] = {0.f, 0.f}, mxb[2] = {0.f, 0.f}, mxc[2] = {0.f, 0.f}, mxh[2] = {0.f, 0.f};
    bool need[2] = {false, false};
    // one entry of the gap table (every field folds to a constant once the phase loops are unrolled)
    auto run_op = [&](auto phase_c, auto gap_c, auto slot_c) __attribute__((always_inline)) {
      constexpr W64Op o = decltype(phase_c)::value == 1 ? W64_P1[decltype(gap_c)::value][decltype(slot_c)::value]
                                                        : W64_P2[decltype(gap_c)::value][decltype(slot_c)::value];
      constexpr int b_ = o.b, e = o.e;
      if constexpr (o.kind == W64_EXP) ex[b_][e] = gap_exp2(SCW(c, b_, e));
      if constexpr (o.kind == W64_ADD) psum[b_] = gap_add((e == 1) ? ex[b_][0] : psum[b_], ex[b_][e]);
      if constexpr (o.kind == W64_PACK) pw[b_][e] = gap_pack(ex[b_][2 * e], ex[b_][2 * e + 1]);
      if constexpr (o.kind == W64_LRUN) l_run[b_] = gap_add(l_run[b_], psum[b_]);
      if constexpr (o.kind == W64_VOFF) asm volatile("v_add_u32 %0, %1, %0" : "+v"(v_off[b_ >> 2][b_ & 3]) : "s"(v_delta));
      if constexpr (o.kind == W64_MAX) {   // two chains of 8 max3 per query block; steps 7 and 8 fold chain b into a and a into b: the full maximum
        if constexpr (e == 0) {
          mxa[b_] = gap_max3(n[0][b_][0], n[0][b_][1], n[0][b_][2]);
          mxb[b_] = gap_max3(n[1][b_][0], n[1][b_][1], n[1][b_][2]);
        } else if constexpr (e < 7) {
          mxa[b_] = gap_max3(mxa[b_], n[0][b_][2 * e + 1], n[0][b_][2 * e + 2]);
          mxb[b_] = gap_max3(mxb[b_], n[1][b_][2 * e + 1], n[1][b_][2 * e + 2]);
        } else if constexpr (e == 7) {
          mxa[b_] = gap_max3(mxa[b_], n[0][b_][15], mxb[b_]);
        } else {
          mxb[b_] = gap_max3(mxa[b_], n[1][b_][15], n[1][b_][14]);
        }
      }
      // half_max(mxb) in three statements: the copy the swap needs (two distinct registers), the swap, the maximum of the halves
      if constexpr (o.kind == W64_HCPY) asm volatile("v_mov_b32 %0, %1" : "=v"(mxc[b_]) : "v"(mxb[b_]));
      if constexpr (o.kind == W64_HSWAP) asm volatile("v_permlane32_swap_b32 %0, %1" : "+v"(mxb[b_]), "+v"(mxc[b_]));
      if constexpr (o.kind == W64_HMAX) asm volatile("v_max_f32 %0, %1, %2" : "=v"(mxh[b_]) : "v"(mxb[b_]), "v"(mxc[b_]));
      if constexpr (o.kind == W64_BALLOT) need[b_] = __builtin_amdgcn_ballot_w64(mxh[b_] > ATTN_RESCALE_THR) != 0ull;
      // the eight LDS-DMA requests of this iteration: K(t+3) into K(t+1)'s buffer, V(t+2) into V(t-1)'s slot (both free since
      // the barrier); waited for at the next barrier, a whole iteration away
      if constexpr (o.kind == W64_M0) {
        if constexpr (b_ < 4) { if (has_k3) dma_m0(b_, (PAR ^ 1) * TILE); }
        else { if (has_v2) dma_m0(b_ & 3, v_dst); }
      }
      if constexpr (o.kind == W64_DMA) {
        if constexpr (b_ < 4) { if (has_k3) dma_req(KOP, b_, t + 3, STEADY); }
        else { if (has_v2) dma_req(VOP, b_ & 3, t + 2, STEADY); }
      }
    };
    SCHED_FENCE();
    // ---------------- phase 1: 32 score MFMAs of tile t+1; exp2 / sums / packs of elements 0..23 of both query blocks ----------
    w64_static_for<0, 32>([&](auto i_c) __attribute__((always_inline)) {
      constexpr int i = decltype(i_c)::value;
      const int f = i >> 1, nb = i & 1;               // fragment f = (k-step f >> 1, key block f & 1) feeds MFMAs 2 f, 2 f + 1
      if (i == 0) kfr[PD % RING] = read_k(kb, PD);
      if (f < 2) mfma_s_first<!STEADY>(n[f & 1][nb], minit[nb], kfr[f % RING], qf[nb][0]);
      else mfma_s<!STEADY>(n[f & 1][nb], kfr[f % RING], qf[nb][f >> 1]);
      SCHED_FENCE();
      if (nb == 1) {   // the read of fragment f + 1 + PD, into the ring slot MFMA i was the last to read (see above the table)
        const int fn = f + 1;
        if (fn + PD < 16) kfr[(fn + PD) % RING] = read_k(kb, fn + PD);
        else if (fn < 16) vfr[fn - (16 - PD)] = read_v(fn - (16 - PD));   // first fragments of V(t) (landed since the last barrier)
        else vfr[PD % RING] = read_v(PD);
        SCHED_FENCE();
      }
      w64_static_for<0, W64_SLOTS>([&](auto s_c) { run_op(std::integral_constant<int, 1>{}, i_c, s_c); });
      SCHED_FENCE();
    });
    if constexpr (!STEADY) {
      fence_s(n);
      if (t + 1 == nt - 1 && ragged) mask_last(n);   // scalar branch, taken once
    }
    // the one barrier: K(t+2) and V(t+1) are in LDS for every wave; every wave has finished reading K(t+1) and V(t-1)
    dma_wait_and_barrier();
    // ---------------- phase 2: 32 PV MFMAs of tile t; the rest of P(t); row max of S(t+1); next requests and fragments --------
    SCHED_FENCE();
    w64_static_for<0, 32>([&](auto j_c) __attribute__((always_inline)) {
      constexpr int j = decltype(j_c)::value;
      const int g = j >> 1, nb = j & 1;               // fragment g = (k-step g >> 2, dim block g & 3) feeds MFMAs 2 g, 2 g + 1
      const int kk = g >> 2;
      const u32x4 pbw = {pw[nb][4 * kk], pw[nb][4 * kk + 1], pw[nb][4 * kk + 2], pw[nb][4 * kk + 3]};
      mfma_o<!STEADY>(oacc[nb][g & 3], vfr[g % RING], __builtin_bit_cast(bf16x8, pbw));
      SCHED_FENCE();
      if (nb == 1 && g + 1 < 16) {   // (V fragment PD was read behind the last score MFMA)
        const int gn = g + 1;
        if (gn + PD < 16) vfr[(gn + PD) % RING] = read_v(gn + PD);
        else kfr[gn - (16 - PD)] = read_k(kb_next, gn - (16 - PD));   // first fragments of K(t+2)
        SCHED_FENCE();
      }
      w64_static_for<0, W64_SLOTS>([&](auto s_c) { run_op(std::integral_constant<int, 2>{}, j_c, s_c); });
      SCHED_FENCE();
    });
    settle(n, std::integral_constant<int, 0>{}, mxh[0], false, need[0]);
    settle(n, std::integral_constant<int, 1>{}, mxh[1], false, need[1]);
  };

  // last tile: nothing left to overlap with; c = S(nt - 1), settled; its V tile landed before the last barrier
  auto final_tile = [&](f32x16 (&c)[2][2]) __attribute__((always_inline)) {
    const int v_delta = next_v_slot();
#pragma unroll
    for (int i = 0; i < 8; ++i) v_off[i >> 2][i & 3] += v_delta;
    unsigned pw[2][16];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
      float psum = 0.f;
      float ex[32];
#pragma unroll
      for (int j = 0; j < 32; ++j) {
        ex[j] = __builtin_amdgcn_exp2f(SCW(c, nb, j));
        psum += ex[j];
      }
      l_run[nb] += psum;
#pragma unroll
      for (int m = 0; m < 16; ++m) pw[nb][m] = gap_pack(ex[2 * m], ex[2 * m + 1]);
    }
#pragma unroll
    for (int g = 0; g < 16; ++g) {
      const bf16x8 vf_ = read_v(g);
      const int kk = g >> 2;
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) {
        const u32x4 pbw = {pw[nb][4 * kk], pw[nb][4 * kk + 1], pw[nb][4 * kk + 2], pw[nb][4 * kk + 3]};
        mfma_o<true>(oacc[nb][g & 3], vf_, __builtin_bit_cast(bf16x8, pbw));
      }
    }
    fence_o();
  };

  {
    using P0 = std::integral_constant<int, 0>;
    using P1 = std::integral_constant<int, 1>;
    int t = 0;
    for (; t + 5 < nt; t += 2) {           // steady state: tiles up to t + 4 exist and are FULL (t + 4 is not the last, maybe ragged, one)
      iteration(t, P0{}, std::true_type{}, sa, sb);
      iteration(t + 1, P1{}, std::true_type{}, sb, sa);
    }
    fence_o(); fence_s(sa); fence_s(sb);
    for (; t + 1 <= nt - 2; t += 2) {
      iteration(t, P0{}, std::false_type{}, sa, sb);
      iteration(t + 1, P1{}, std::false_type{}, sb, sa);
    }
    if (t == nt - 2) iteration(t, P0{}, std::false_type{}, sa, sb);
    fence_o(); fence_s(sa); fence_s(sb);
    set_read_offsets(lane_now(), v_slot);   // (fresh copies for the last tile)
    if ((nt - 1) & 1) final_tile(sb);
    else final_tile(sa);
  }

  // ---- epilogue ----
  const int lane_l = lane_now();
  const int r_l = lane_l & 31, h_l = lane_l >> 5;
#pragma unroll
  for (int nb = 0; nb < 2; ++nb) {
    const float l_tot = half_sum(l_run[nb]);
    const float inv = 1.0f / l_tot;
    const int64_t qrow = q0 + 32 * nb + r_l;
    if (qrow < p.d.Nq) {
      bf16_t* op = p.o + b * p.d.o_sb + qrow * p.d.o_sn + (int64_t)head * p.d.o_sh;
#pragma unroll
      for (int d = 0; d < 4; ++d)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          u16x4 pk;
#pragma unroll
          for (int e = 0; e < 4; ++e) pk[e] = f2bf(oacc[nb][d][4 * i + e] * inv);
          *reinterpret_cast<u16x4*>(op + 32 * d + 8 * i + 4 * h_l) = pk;
        }
      if (p.lse && h_l == 0) p.lse[(b * p.d.H + head) * p.d.Nq + qrow] = m_run[nb] * p.scale + __logf(l_tot);
    }
  }
}

// called by lcv_attn_fwd (attn_fwd.hip) for unit-scale self-attention with Nk > 512: the default since round 3 (LCV_ATTN_FWD_W64=0
// selects attn_fwd_pipe.hip instead)
int attn_fwd_w64_launch(const AttnArgs& a, bool xcd_ok, hipStream_t s) {
  const AttnGrid g = attn_grid(a.B, a.H, (a.Nq + 255) / 256, xcd_ok);
  const AttnFwdW64Params p = {attn_fwd_lead(a), a.scale, g.gx, g.xcd_remap};
  const size_t lds = 5 * 64 * 256;   // K x2, V x3
  ATTN_RAISE_LDS_ONCE("attn_fwd_w64", attn_raise_lds((const void*)attn_fwd_w64_kernel, lds));
  hipLaunchKernelGGL(attn_fwd_w64_kernel, g.grid, dim3(256), lds, s, p);
  LCV_LAUNCH_CHECK("attn_fwd_w64");
  return LCV_OK;
}

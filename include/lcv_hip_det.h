/*
 * lcv_hip_det.h - C ABI of the fixed-order (bit-reproducible) forms of the reductions that the default backward and
 * optimizer kernels of liblcv_hip.so finish with fp32 atomics (AMD gfx950, MI355X).
 *
 * The reference seeds every run (torch.manual_seed(args.seed) in each runner) and compares methods on fractions of a
 * dB; the training loss, the attention backward, lcv_tn_skinny and the metrics are already fixed-order.  The entry
 * points below close the list: with them one adaptation step gives the same bits for the same seed inside one process.
 * They are opt-in.  The caller chooses the mode by the entry point it calls: there is no knob and no environment read.
 *
 * Conventions are those of the main header (status codes, the error string and lcv_adam_tensor come from there): every
 * function returns 0 or a negative LCV_E* code, takes device pointers, allocates nothing and takes the hipStream_t as a
 * trailing `void* stream`.  Each lcv_det_X takes the argument list of lcv_X plus `void* ws, int64_t ws_bytes`: a
 * 16-byte-aligned fp32 workspace of at least lcv_det_ws_bytes(...) bytes whose content on entry does not matter and is
 * undefined afterwards.  A missing, misaligned or too small workspace is LCV_EINVAL, as is every shape that the
 * fixed-order form does not take; nothing falls back to the atomic form.
 *
 * Contract of every entry point: the data gradients (dx / dy / dq_in / dk_in) carry the same bits as those of the
 * default entry point on the same inputs; the reduced outputs are a pure function of the inputs and the shapes (each
 * workgroup leaves one partial per output element in the workspace, a second launch adds the partials in index order;
 * the order is written out at the top of csrc/reduce_det.hip).  When no reduced output is asked for (NULL), the call is
 * the default entry point's and the workspace is not touched.
 *
 * Scope: one process.  Under sequence parallelism the order inside the collectives is the communication library's.
 */
#ifndef LCV_HIP_DET_H
#define LCV_HIP_DET_H

#include <stdint.h>
#include "lcv_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* `kind` of the size query, and the meaning of its three dimensions */
#define LCV_DET_ADALN 0      /* d0 = B*T frames, d1 = S rows per frame, d2 = C */
#define LCV_DET_LAYERNORM 1  /* d0 = rows, d1 = C */
#define LCV_DET_GATE 2       /* d0 = B*T frames, d1 = S, d2 = C */
#define LCV_DET_QKNORM 3     /* d0 = B, d1 = N */
#define LCV_DET_SMALLM 4     /* d0 = M, d1 = N, d2 = K */
#define LCV_DET_GRAD_NORM 5  /* d0 = total_chunks */

/* Host-only: bytes of workspace the entry point of `kind` needs at these sizes (unused dimensions are ignored); 0 for
 * an empty shape, -1 for an unknown kind.
 *   ADALN, LAYERNORM  2*C floats per 64 rows of a frame        (1/16 of the bytes of x, plus the ragged last block per frame)
 *   GATE              C floats per 32 rows of a frame          (1/16 of the bytes of y, likewise)
 *   QKNORM            256 floats per token                     (1/8 of one [N, 32, 128] bf16 input)
 *   SMALLM            M*K floats per 256 rows of W
 *   GRAD_NORM         one float per 2 048-element chunk, next to the [n_tensors, 64] rows the default form also takes */
int64_t lcv_det_ws_bytes(int kind, int64_t d0, int64_t d1, int64_t d2);

/* lcv_adaln_modulate_bwd with fixed-order dshift / dscale.  One workgroup per 64 rows of ONE frame (no workgroup spans
 * two frames).  dmod is ADDED to, one adder per element, as the default form adds.  C % 8 == 0, C <= 4096. */
int lcv_det_adaln_modulate_bwd(const void* x, const float* mod, const void* dy, void* dx, float* dmod, int64_t B,
                               int64_t T, int64_t S, int64_t C, int64_t mod_stride, int64_t shift_off, int64_t scale_off,
                               float eps, const void* dres, void* ws, int64_t ws_bytes, void* stream);

/* lcv_layernorm_affine_bwd with fixed-order dw / db (added to).  C % 8 == 0, C <= 4096. */
int lcv_det_layernorm_affine_bwd(const void* x, const float* w, const void* dy, void* dx, float* dw, float* db,
                                 int64_t rows, int64_t C, float eps, const void* dres, void* ws, int64_t ws_bytes,
                                 void* stream);

/* lcv_gate_residual_bwd with fixed-order dgate (added to).  One workgroup per 32 rows of one frame.  With dmod:
 * C / 8 <= 512 (LCV_EINVAL above; the default form's generic kernel has no fixed-order counterpart). */
int lcv_det_gate_residual_bwd(const void* y, const float* mod, const void* dout, void* dy, float* dmod, int64_t B,
                              int64_t T, int64_t S, int64_t C, int64_t mod_stride, int64_t gate_off, void* ws,
                              int64_t ws_bytes, void* stream);

/* lcv_qknorm_rope_bwd without dw_slots: dwq / dwk are fp32 [128] and are ADDED to directly (one adder per element), so a
 * caller may hand the same accumulator to successive calls on one stream.  D = 128. */
int lcv_det_qknorm_rope_bwd(const void* q_in, const void* k_in, const void* dq_out, const void* dk_out, void* dq_in,
                            void* dk_in, const void* wq, const void* wk, const void* cs, int64_t B, int64_t N, int64_t H,
                            int64_t in_sb, int64_t in_sn, int64_t q_sb, int64_t q_sn, int64_t kv_sb, int64_t kv_sn,
                            int64_t din_sb, int64_t din_sn, int64_t pos_off, float eps, float q_scale, float* dwq,
                            float* dwk, void* ws, int64_t ws_bytes, void* stream);

/* lcv_linear_f32_smallm_bwd with the 256-row slabs of W added in slab order.  `da` is overwritten (no zero-fill).
 * M, N, K >= 1, K even, M*K <= 65535 * 256. */
int lcv_det_linear_f32_smallm_bwd(const float* dy, const void* w, const float* a, float* da, int64_t M, int64_t N,
                                  int64_t K, int act_in, void* ws, int64_t ws_bytes, void* stream);

/* lcv_grad_norm_clip with one partial per chunk and a block-wide fixed tree per tensor.  The per-tensor sum of squares
 * lands in slot 0 of the tensor's row of per_tensor_ws [n_tensors, 64], slots 1..63 are written as zeros; the
 * coefficient arithmetic (bf16 rounding points of the per-tensor and total norms) is the default form's. */
int lcv_det_grad_norm_clip(const lcv_adam_tensor* tensors, int64_t n_tensors, int64_t total_chunks, int param_f32,
                           float max_norm, float* per_tensor_ws, float* norm_coef_out, void* ws, int64_t ws_bytes,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LCV_HIP_DET_H */

/*
 * lcv_hip_lpips.h - C ABI of the on-device LPIPS v0.1 (AlexNet backbone) of liblcv_hip.so (AMD gfx950, MI355X).
 *
 * The third quality column of every result row of the reference: its runners call `lpips.LPIPS(net="alex")` on each
 * generated / ground-truth frame pair after every generation (delta_experiment/scripts/common.py:648-660, 740-757;
 * baseline_experiment/scripts/run_baseline.py:148-165, 442).  The arithmetic restated here is listed, assumption by
 * assumption, in spec/lpips.md.
 *
 * Conventions are those of the main header (status codes and the error string come from there): every function returns
 * 0 or a negative LCV_E* code, takes device pointers, allocates nothing, and takes the hipStream_t as a trailing
 * `void* stream`.  Everything is fp32; activations are channels-last [B, h, w, C] with B = 2N images - the N generated
 * frames first, their N ground-truth frames after them - so that one launch per layer serves both halves of every pair.
 */
#ifndef LCV_HIP_LPIPS_H
#define LCV_HIP_LPIPS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Per-frame partial-sum slots one tap-distance launch may fill (the caller's `partials` holds N * this many floats). */
#define LCV_LPIPS_TAP_BLOCKS 64

/* Repack one convolution weight, done once when the weights are loaded: w fp32 [Cout, Cin, KH, KW] (the state-dict
 * layout) -> packed fp32 [Cout, Kpad], k = (kh * KW + kw) * Cin + ci, zeros from KH*KW*Cin up to Kpad.  Kpad is a
 * multiple of 32 (the K step of the convolution's tile) and >= KH*KW*Cin: conv1 has K = 363 -> Kpad = 384. */
int lcv_lpips_pack_weight(const float* w, float* packed, int64_t Cout, int64_t Cin, int64_t KH, int64_t KW,
                          int64_t Kpad, void* stream);

/* One `features` layer of AlexNet: out = relu(conv2d(in, w) + bias), an implicit GEMM on the f32-input MFMA
 * (M = B*Ho*Wo output pixels, N = Cout, K = KH*KW*Cin).  in: fp32 [B, Hin, Win, Cin]; wpacked: [Cout, Kpad] from
 * lcv_lpips_pack_weight; bias: [Cout]; out: fp32 [B, Ho, Wo, Cout], Ho = (Hin + 2*pad - KH) / stride + 1.
 * Cout % 64 == 0; Cin % 32 == 0 unless first_layer.
 * first_layer != 0 (Cin == 3): `in` holds the B/2 generated frames [B/2, Hin, Win, 3] fp32 in [0,1] and `in_gt` their
 * ground truth, fp32 or raw uint8 (gt_is_u8: divided by 255 in the loader); the loader applies 2*x - 1 and the scaling
 * layer (v - shift[c]) / scale[c] on the fly (`shift_scale`: 6 HOST floats, shift then scale), so no normalised copy of
 * the frames exists.  Otherwise in_gt and shift_scale are ignored (NULL).
 * lpips/pretrained_networks.py (alexnet slices 1-5) under lpips.LPIPS.forward; common.py:648-660. */
int lcv_lpips_conv_relu(const void* in, const void* in_gt, int first_layer, int gt_is_u8, const float* shift_scale,
                        const float* wpacked, const float* bias, float* out, int64_t B, int64_t Hin, int64_t Win,
                        int64_t Cin, int64_t Cout, int64_t KH, int64_t KW, int64_t stride, int64_t pad, int64_t Kpad,
                        void* stream);

/* MaxPool2d(kernel 3, stride 2, no padding, floor mode), channels-last: in [B, h, w, C] -> out [B, (h-3)/2+1,
 * (w-3)/2+1, C]; C % 4 == 0, h, w >= 3.  AlexNet `features` 2 and 5. */
int lcv_lpips_maxpool(const float* in, float* out, int64_t B, int64_t h, int64_t w, int64_t C, void* stream);

/* Distance of one tap: feats fp32 [2N, P, C] (P = h*w pixels; image n is generated frame n, image N + n its ground
 * truth), lin fp32 [C] the tap's 1x1 weights.  Per pixel f / (sqrt(sum_c f_c^2) + 1e-10) on both halves, then
 * sum_c lin_c * (difference)^2; out[n] (+)= mean over the P pixels.  Two launches: per-workgroup sums into
 * partials [N, LCV_LPIPS_TAP_BLOCKS], then a fixed-order sum per frame - no atomics, the same bits on every run.
 * accumulate != 0 adds to out[n] (taps 2-5), 0 overwrites it (tap 1).  C % 64 == 0, C <= 384.
 * lpips.LPIPS.forward (normalize_tensor, lins, spatial_average); common.py:753 takes the mean over frames. */
int lcv_lpips_tap_distance(const float* feats, const float* lin, float* partials, float* out, int accumulate, int64_t N,
                           int64_t P, int64_t C, void* stream);

/* Host-only: bytes of the workspace one N-pair evaluation of HxW frames carves its five taps, two pooled maps and the
 * partial sums from (each region rounded up to 256 bytes, in the order tap1, pool1, tap2, pool2, tap3, tap4, tap5,
 * partials); 0 when the frame is smaller than 31x31 (the second pool would have no window). */
int64_t lcv_lpips_ws_bytes(int64_t N, int64_t H, int64_t W);

#ifdef __cplusplus
}
#endif
#endif /* LCV_HIP_LPIPS_H */

// On-device LPIPS v0.1, AlexNet backbone, forward only, fp32 (include/lcv_hip_lpips.h; the arithmetic is itemised in
// spec/lpips.md).  The reference scores every generated clip with `lpips.LPIPS(net="alex")` frame pair by frame pair
// (delta_experiment/scripts/common.py:648-660, 740-757; baseline_experiment/scripts/run_baseline.py:148-165, 442).
//
// Layout: activations are channels-last [B, h, w, C], B = 2N images (generated frames first, ground truth after), so
// the K axis of every convolution's implicit GEMM - (kh, kw, ci) with ci fastest - is contiguous in memory per filter
// tap, and the channel reduction of the tap distance is a contiguous run per pixel.
//
// Kernels:
//   conv_relu_kernel     implicit GEMM on v_mfma_f32_32x32x2_f32 (exact fp32: a k-ordered fma chain per 32-k chunk,
//                        the chunk sums added with compensation).
//                        Block tile 128 pixels x 64 channels x 32 k, four waves of 32 x 64 (two independent 32x32
//                        accumulators each).  Every Cout of the network (64, 192, 384, 256) is a multiple of 64, so no
//                        N tile has empty columns; 128-pixel M tiles leave at most one partly filled tile per launch.
//   maxpool3s2_kernel    3x3 / stride 2, HBM-bound.  A kernel of its own: the un-pooled map is a tap and has to reach
//                        HBM in full anyway, and a pool folded into the next layer's loader would read 9 values per
//                        element for each of its 25 (conv2) or 9 (conv3) filter taps instead of once.
//   tap_distance_kernel  16 lanes per pixel, channel sums by butterfly inside the wave, one partial sum per workgroup;
//   tap_reduce_kernel    adds a frame's partials in a fixed order (no atomics anywhere: results are bit-reproducible).
#include "lcv_common.h"
#include "../../include/lcv_hip_lpips.h"

namespace {

constexpr int CV_BM = 128, CV_BN = 64, CV_BK = 32;
constexpr int CV_LD = CV_BK + 4;   // LDS row stride in floats: 16-byte aligned rows, 8 consecutive rows cover all 64 banks

struct ConvParams {
  const void* in;
  const void* in_gt;
  const float* w;
  const float* bias;
  float* out;
  int M;                 // B * Ho * Wo output pixels
  int Nhalf;             // first layer: images [0, Nhalf) come from `in`, the rest from `in_gt`
  int Hin, Win, Cin, Cout, KW, stride, pad, Ho, Wo, Kpad, Kreal;
  float shift[3], scale[3];
};

__device__ __forceinline__ float u8_to_unit(unsigned int u) { return (float)((double)u * (1.0 / 255.0)); }   // as eval_metrics.hip

template <bool FIRST, bool GT_U8>
__global__ __launch_bounds__(256) void conv_relu_kernel(ConvParams p) {
  __shared__ __attribute__((aligned(16))) float As[2][CV_BM * CV_LD];
  __shared__ __attribute__((aligned(16))) float Bs[2][CV_BN * CV_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int tiles_n = p.Cout / CV_BN;
  // the channel tile varies fastest: the blocks that share a pixel tile run together and its input stays in L2
  const int n0 = (int)(blockIdx.x % tiles_n) * CV_BN;
  const int m0 = (int)(blockIdx.x / tiles_n) * CV_BM;

  // ---- A loader geometry.  General layers: a 32-float k chunk lies inside one filter tap (Cin % 32 == 0), so a row
  // of the tile is 8 packets of 16 bytes; thread t owns packet t % 8 of rows t / 8 + 32 i.  First layer (Cin = 3):
  // thread t owns 16 consecutive k of row t / 2 and decodes (kh, kw, ci) per element.
  constexpr int NROW = FIRST ? 1 : 4;
  int r_img[NROW], r_iy[NROW], r_ix[NROW];
  bool r_ok[NROW];
#pragma unroll
  for (int i = 0; i < NROW; ++i) {
    const int row = FIRST ? (tid >> 1) : (tid >> 3) + 32 * i;
    const int m = m0 + row;
    r_ok[i] = m < p.M;
    const int mm = r_ok[i] ? m : 0;
    const int img = mm / (p.Ho * p.Wo), rem = mm - img * (p.Ho * p.Wo);
    const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
    r_img[i] = img;
    r_iy[i] = oy * p.stride - p.pad;
    r_ix[i] = ox * p.stride - p.pad;
  }

  f32x4 pa[4], pb[2];
  auto fetch = [&](int chunk) {
    const int k0 = chunk * CV_BK;
#pragma unroll
    for (int i = 0; i < 2; ++i) {               // weights: Cout % 64 == 0 and Kpad % 32 == 0, every packet is inside the buffer
      const int col = (tid >> 3) + 32 * i;
      pb[i] = *(const f32x4*)(p.w + (int64_t)(n0 + col) * p.Kpad + k0 + 4 * (tid & 7));
    }
    if constexpr (FIRST) {
      const bool from_gt = r_img[0] >= p.Nhalf;
      const int64_t frame = (int64_t)(from_gt ? r_img[0] - p.Nhalf : r_img[0]) * p.Hin * p.Win * 3;
      const int row_k = p.KW * 3;               // 33 contiguous floats of one input row per kh
      const int kfirst = k0 + 16 * (tid & 1);
      int kh = kfirst / row_k, kw = (kfirst - kh * row_k) / 3, ci = kfirst - kh * row_k - kw * 3;
#pragma unroll
      for (int e = 0; e < 16; ++e, ++ci) {      // (kh, kw, ci) counts up with k: one division per chunk, not per element
        const int k = kfirst + e;
        if (ci == 3) { ci = 0; ++kw; }
        if (kw == p.KW) { kw = 0; ++kh; }
        const int iy = r_iy[0] + kh, ix = r_ix[0] + kw;
        const bool ok = r_ok[0] && k < p.Kreal && iy >= 0 && iy < p.Hin && ix >= 0 && ix < p.Win;
        float v = 0.f;
        if (ok) {
          const int64_t at = frame + ((int64_t)iy * p.Win + ix) * 3 + ci;
          float x;
          if (!from_gt) x = ((const float*)p.in)[at];
          else if constexpr (GT_U8) x = u8_to_unit(((const unsigned char*)p.in_gt)[at]);
          else x = ((const float*)p.in_gt)[at];
          const float sh = ci == 0 ? p.shift[0] : (ci == 1 ? p.shift[1] : p.shift[2]);
          const float sc = ci == 0 ? p.scale[0] : (ci == 1 ? p.scale[1] : p.scale[2]);
          v = ((2.f * x - 1.f) - sh) / sc;      // padding is zero AFTER the scaling layer, as conv2d pads its input
        }
        pa[e >> 2][e & 3] = v;
      }
    } else {
      const int tap = k0 / p.Cin, ci0 = k0 - tap * p.Cin;
      const int kh = tap / p.KW, kw = tap - kh * p.KW;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int iy = r_iy[i] + kh, ix = r_ix[i] + kw;
        const bool ok = r_ok[i] && iy >= 0 && iy < p.Hin && ix >= 0 && ix < p.Win;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (ok)
          v = *(const f32x4*)((const float*)p.in + (((int64_t)r_img[i] * p.Hin + iy) * p.Win + ix) * p.Cin + ci0 + 4 * (tid & 7));
        pa[i] = v;
      }
    }
  };
  auto put = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 2; ++i) *(f32x4*)(&Bs[buf][((tid >> 3) + 32 * i) * CV_LD + 4 * (tid & 7)]) = pb[i];
    if constexpr (FIRST) {
#pragma unroll
      for (int i = 0; i < 4; ++i) *(f32x4*)(&As[buf][(tid >> 1) * CV_LD + 16 * (tid & 1) + 4 * i]) = pa[i];
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i) *(f32x4*)(&As[buf][((tid >> 3) + 32 * i) * CV_LD + 4 * (tid & 7)]) = pa[i];
    }
  };

  // An MFMA accumulates as one k-ordered fp32 fma chain; over K = 3456 that chain alone would cost ~1e-6 relative
  // (u sqrt(K) / 2.4).  So the chain restarts from zero every 32-k chunk (error ~1.4e-7) and the chunk sums are added
  // with Kahan compensation on the VALU: 4 instructions per accumulator register per chunk, beside 32 MFMAs of 64 cycles.
  f32x16 tot0, tot1, cmp0, cmp1, zero16;
#pragma unroll
  for (int i = 0; i < 16; ++i) tot0[i] = tot1[i] = cmp0[i] = cmp1[i] = zero16[i] = 0.f;
  auto fold = [](f32x16& tot, f32x16& cmp, const f32x16& part) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const float y = part[i] - cmp[i];
      const float t = tot[i] + y;
      cmp[i] = (t - tot[i]) - y;
      tot[i] = t;
    }
  };

  const int nchunks = p.Kpad / CV_BK;
  fetch(0);
  put(0);
  __syncthreads();
  // 32x32x2 operands: lane l holds A[row l & 31][k = l >> 5] and B[k = l >> 5][col l & 31].  Which k a lane half feeds
  // to a given MFMA is free as long as A and B agree, so each lane reads 4 consecutive k per 16-byte LDS read (half h of
  // the wave takes k = 8 j + 4 h + e in step e): one ds_read_b128 per operand per 4 MFMA steps.
  const int frag = (lane & 31) * CV_LD + 4 * (lane >> 5);
  for (int c = 0; c < nchunks; ++c) {
    const int buf = c & 1;
    if (c + 1 < nchunks) fetch(c + 1);          // global -> registers ahead of this chunk's 32 MFMAs
    const float* a = &As[buf][wave * 32 * CV_LD + frag];
    const float* b = &Bs[buf][frag];
    f32x16 acc0 = zero16, acc1 = zero16;
#pragma unroll
    for (int j = 0; j < CV_BK / 8; ++j) {
      const f32x4 av = *(const f32x4*)(a + 8 * j);
      const f32x4 b0 = *(const f32x4*)(b + 8 * j);
      const f32x4 b1 = *(const f32x4*)(b + 32 * CV_LD + 8 * j);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[e], b0[e], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[e], b1[e], acc1, 0, 0, 0);
      }
    }
    fold(tot0, cmp0, acc0);
    fold(tot1, cmp1, acc1);
    if (c + 1 < nchunks) put(buf ^ 1);          // the other buffer: last read before the barrier that ended chunk c - 1
    __syncthreads();
  }

  // C/D map of the 32x32 forms: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  const int co = n0 + (lane & 31);
  const float bias0 = p.bias[co], bias1 = p.bias[co + 32];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = m0 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    if (m < p.M) {
      float* o = p.out + (int64_t)m * p.Cout + co;
      o[0] = fmaxf(tot0[r] + bias0, 0.f);
      o[32] = fmaxf(tot1[r] + bias1, 0.f);
    }
  }
}

__global__ __launch_bounds__(256) void maxpool3s2_kernel(const float* __restrict__ in, float* __restrict__ out, int64_t total,
                                                         int h, int w, int C4, int ho, int wo) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c4 = (int)(i % C4);
    int64_t t = i / C4;
    const int ox = (int)(t % wo); t /= wo;
    const int oy = (int)(t % ho);
    const int64_t img = t / ho;
    const f32x4* src = (const f32x4*)in + ((img * h + 2 * oy) * w + 2 * ox) * C4 + c4;   // 2 o + 2 <= h - 1: floor mode
    f32x4 m = src[0];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        const f32x4 v = src[((int64_t)dy * w + dx) * C4];
#pragma unroll
        for (int e = 0; e < 4; ++e) m[e] = fmaxf(m[e], v[e]);
      }
    ((f32x4*)out)[i] = m;
  }
}

__global__ __launch_bounds__(256) void pack_weight_kernel(const float* __restrict__ w, float* __restrict__ packed, int64_t total,
                                                          int Cin, int KH, int KW, int Kpad) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int k = (int)(i % Kpad);
    const int64_t co = i / Kpad;
    float v = 0.f;
    if (k < KH * KW * Cin) {
      const int tap = k / Cin, ci = k - tap * Cin, kh = tap / KW, kw = tap - kh * KW;
      v = w[((co * Cin + ci) * KH + kh) * KW + kw];
    }
    packed[i] = v;
  }
}

__device__ __forceinline__ float group16_sum(float v) {
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// V packets of 16 bytes per lane: C = 64 V channels, 16 lanes per pixel, 16 pixels per workgroup pass
template <int V>
__global__ __launch_bounds__(256) void tap_distance_kernel(const float* __restrict__ feats, const float* __restrict__ lin,
                                                           float* __restrict__ partials, int N, int P) {
  __shared__ float red[4];
  constexpr int C = 64 * V;
  const int tid = threadIdx.x, gl = tid & 15, grp = tid >> 4;
  const int n = blockIdx.y;
  const float* fg = feats + (int64_t)n * P * C;
  const float* ft = feats + (int64_t)(n + N) * P * C;
  f32x4 wv[V];
#pragma unroll
  for (int v = 0; v < V; ++v) wv[v] = *(const f32x4*)(lin + 4 * (gl + 16 * v));
  float acc = 0.f;
  const int step = gridDim.x * 16;
  const int trips = (P + step - 1) / step;      // the same count for every lane: the butterflies below never diverge
  for (int it = 0; it < trips; ++it) {
    const int px = it * step + blockIdx.x * 16 + grp;
    const bool ok = px < P;
    f32x4 g[V], t[V];
    float sg = 0.f, st = 0.f;
#pragma unroll
    for (int v = 0; v < V; ++v) {
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
      const int64_t at = (int64_t)(ok ? px : 0) * C + 4 * (gl + 16 * v);
      g[v] = ok ? *(const f32x4*)(fg + at) : z;
      t[v] = ok ? *(const f32x4*)(ft + at) : z;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        sg = fmaf(g[v][e], g[v][e], sg);
        st = fmaf(t[v][e], t[v][e], st);
      }
    }
    const float ng = sqrtf(group16_sum(sg)) + 1e-10f, nt = sqrtf(group16_sum(st)) + 1e-10f;
    float d = 0.f;
#pragma unroll
    for (int v = 0; v < V; ++v)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float df = g[v][e] / ng - t[v][e] / nt;
        d = fmaf(wv[v][e] * df, df, d);
      }
    d = group16_sum(d);
    if (gl == 0 && ok) acc += d;
  }
  acc = wave_sum(acc);
  if ((tid & 63) == 0) red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) partials[(int64_t)n * LCV_LPIPS_TAP_BLOCKS + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

__global__ __launch_bounds__(64) void tap_reduce_kernel(const float* __restrict__ partials, float* __restrict__ out, int nb, int P,
                                                        int accumulate) {
  const int n = blockIdx.x, lane = threadIdx.x;
  const float v = wave_sum(lane < nb ? partials[(int64_t)n * LCV_LPIPS_TAP_BLOCKS + lane] : 0.f) / (float)P;
  if (lane == 0) out[n] = accumulate ? out[n] + v : v;
}

inline int64_t round_up(int64_t v, int64_t a) { return (v + a - 1) / a * a; }
inline unsigned stride_grid(int64_t total) {
  const int64_t b = (total + 255) / 256;
  return (unsigned)(b < 1 ? 1 : (b > 8192 ? 8192 : b));
}

}  // namespace

extern "C" int lcv_lpips_pack_weight(const float* w, float* packed, int64_t Cout, int64_t Cin, int64_t KH, int64_t KW,
                                     int64_t Kpad, void* stream) {
  LCV_CHECK_ARG(w && packed, "lpips_pack_weight: null pointer");
  LCV_CHECK_ARG(Cout > 0 && Cin > 0 && KH > 0 && KW > 0 && Cout <= 4096 && Cin <= 4096 && KH <= 31 && KW <= 31,
                "lpips_pack_weight: weight [%ld,%ld,%ld,%ld]", (long)Cout, (long)Cin, (long)KH, (long)KW);
  LCV_CHECK_ARG(Kpad % CV_BK == 0 && Kpad >= KH * KW * Cin && Kpad < KH * KW * Cin + CV_BK,
                "lpips_pack_weight: Kpad=%ld must be K=%ld rounded up to a multiple of %d", (long)Kpad, (long)(KH * KW * Cin), CV_BK);
  const int64_t total = Cout * Kpad;
  hipLaunchKernelGGL(pack_weight_kernel, dim3(stride_grid(total)), dim3(256), 0, (hipStream_t)stream, w, packed, total, (int)Cin,
                     (int)KH, (int)KW, (int)Kpad);
  LCV_LAUNCH_CHECK("lpips_pack_weight");
  return LCV_OK;
}

extern "C" int lcv_lpips_conv_relu(const void* in, const void* in_gt, int first_layer, int gt_is_u8, const float* shift_scale,
                                   const float* wpacked, const float* bias, float* out, int64_t B, int64_t Hin, int64_t Win,
                                   int64_t Cin, int64_t Cout, int64_t KH, int64_t KW, int64_t stride, int64_t pad, int64_t Kpad,
                                   void* stream) {
  LCV_CHECK_ARG(in && wpacked && bias && out, "lpips_conv_relu: null pointer");
  LCV_CHECK_ARG(B > 0 && Hin > 0 && Win > 0 && Hin < (1 << 20) && Win < (1 << 20) && KH > 0 && KW > 0 && KH <= 31 && KW <= 31 &&
                stride > 0 && stride <= 8 && pad >= 0 && pad < KH && pad < KW,
                "lpips_conv_relu: B=%ld %ldx%ld input, %ldx%ld filter, stride %ld, pad %ld", (long)B, (long)Hin, (long)Win,
                (long)KH, (long)KW, (long)stride, (long)pad);
  LCV_CHECK_ARG(Hin + 2 * pad >= KH && Win + 2 * pad >= KW, "lpips_conv_relu: a %ldx%ld input is smaller than the %ldx%ld filter",
                (long)Hin, (long)Win, (long)KH, (long)KW);
  LCV_CHECK_ARG(Cout > 0 && Cout % CV_BN == 0, "lpips_conv_relu: Cout=%ld must be a multiple of %d", (long)Cout, CV_BN);
  const int64_t K = KH * KW * Cin;
  LCV_CHECK_ARG(Cin > 0 && Kpad % CV_BK == 0 && Kpad >= K && Kpad < K + CV_BK && Kpad < (1 << 24),
                "lpips_conv_relu: Kpad=%ld must be K=%ld rounded up to a multiple of %d", (long)Kpad, (long)K, CV_BK);
  if (first_layer) {
    LCV_CHECK_ARG(Cin == 3 && in_gt && shift_scale && B % 2 == 0,
                  "lpips_conv_relu: the first layer takes N generated + N ground-truth RGB frames and the scaling constants");
    for (int c = 0; c < 3; ++c) LCV_CHECK_ARG(shift_scale[3 + c] != 0.f, "lpips_conv_relu: scaling layer scale[%d] is zero", c);
  } else {
    LCV_CHECK_ARG(Cin % CV_BK == 0, "lpips_conv_relu: Cin=%ld must be a multiple of %d (or the first layer's 3)", (long)Cin, CV_BK);
  }
  const int64_t Ho = (Hin + 2 * pad - KH) / stride + 1, Wo = (Win + 2 * pad - KW) / stride + 1;
  const int64_t M = B * Ho * Wo;
  const int64_t tiles = (M + CV_BM - 1) / CV_BM * (Cout / CV_BN);
  LCV_CHECK_ARG(M < (1ll << 31) - CV_BM && tiles < (1ll << 31), "lpips_conv_relu: %ld output pixels in one launch (split the batch)", (long)M);
  ConvParams p;
  p.in = in; p.in_gt = in_gt; p.w = wpacked; p.bias = bias; p.out = out;
  p.M = (int)M; p.Nhalf = (int)(B / 2);
  p.Hin = (int)Hin; p.Win = (int)Win; p.Cin = (int)Cin; p.Cout = (int)Cout; p.KW = (int)KW; p.stride = (int)stride; p.pad = (int)pad;
  p.Ho = (int)Ho; p.Wo = (int)Wo; p.Kpad = (int)Kpad; p.Kreal = (int)K;
  for (int c = 0; c < 3; ++c) {
    p.shift[c] = first_layer ? shift_scale[c] : 0.f;
    p.scale[c] = first_layer ? shift_scale[3 + c] : 1.f;
  }
  const dim3 grid((unsigned)tiles), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (!first_layer) hipLaunchKernelGGL((conv_relu_kernel<false, false>), grid, block, 0, s, p);
  else if (gt_is_u8) hipLaunchKernelGGL((conv_relu_kernel<true, true>), grid, block, 0, s, p);
  else hipLaunchKernelGGL((conv_relu_kernel<true, false>), grid, block, 0, s, p);
  LCV_LAUNCH_CHECK("lpips_conv_relu");
  return LCV_OK;
}

extern "C" int lcv_lpips_maxpool(const float* in, float* out, int64_t B, int64_t h, int64_t w, int64_t C, void* stream) {
  LCV_CHECK_ARG(in && out, "lpips_maxpool: null pointer");
  LCV_CHECK_ARG(B > 0 && C > 0 && C % 4 == 0 && C <= 4096, "lpips_maxpool: B=%ld images of C=%ld channels (C %% 4 == 0)", (long)B, (long)C);
  LCV_CHECK_ARG(h >= 3 && w >= 3 && h < (1 << 20) && w < (1 << 20), "lpips_maxpool: a %ldx%ld map is smaller than the 3x3 window",
                (long)h, (long)w);
  const int64_t ho = (h - 3) / 2 + 1, wo = (w - 3) / 2 + 1;
  const int64_t total = B * ho * wo * (C / 4);
  hipLaunchKernelGGL(maxpool3s2_kernel, dim3(stride_grid(total)), dim3(256), 0, (hipStream_t)stream, in, out, total, (int)h, (int)w,
                     (int)(C / 4), (int)ho, (int)wo);
  LCV_LAUNCH_CHECK("lpips_maxpool");
  return LCV_OK;
}

extern "C" int lcv_lpips_tap_distance(const float* feats, const float* lin, float* partials, float* out, int accumulate, int64_t N,
                                      int64_t P, int64_t C, void* stream) {
  LCV_CHECK_ARG(feats && lin && partials && out, "lpips_tap_distance: null pointer");
  LCV_CHECK_ARG(N > 0 && N <= 65535 && P > 0 && P < (1ll << 31) - 16 * LCV_LPIPS_TAP_BLOCKS,
                "lpips_tap_distance: N=%ld pairs of P=%ld pixels", (long)N, (long)P);
  LCV_CHECK_ARG(C % 64 == 0 && C >= 64 && C <= 384, "lpips_tap_distance: C=%ld channels (a multiple of 64, at most 384)", (long)C);
  int64_t nb = (P + 15) / 16;
  if (nb > LCV_LPIPS_TAP_BLOCKS) nb = LCV_LPIPS_TAP_BLOCKS;
  const dim3 grid((unsigned)nb, (unsigned)N), block(256);
  hipStream_t s = (hipStream_t)stream;
  switch (C / 64) {
    case 1: hipLaunchKernelGGL(tap_distance_kernel<1>, grid, block, 0, s, feats, lin, partials, (int)N, (int)P); break;
    case 2: hipLaunchKernelGGL(tap_distance_kernel<2>, grid, block, 0, s, feats, lin, partials, (int)N, (int)P); break;
    case 3: hipLaunchKernelGGL(tap_distance_kernel<3>, grid, block, 0, s, feats, lin, partials, (int)N, (int)P); break;
    case 4: hipLaunchKernelGGL(tap_distance_kernel<4>, grid, block, 0, s, feats, lin, partials, (int)N, (int)P); break;
    case 5: hipLaunchKernelGGL(tap_distance_kernel<5>, grid, block, 0, s, feats, lin, partials, (int)N, (int)P); break;
    default: hipLaunchKernelGGL(tap_distance_kernel<6>, grid, block, 0, s, feats, lin, partials, (int)N, (int)P); break;
  }
  LCV_LAUNCH_CHECK("lpips_tap_distance");
  hipLaunchKernelGGL(tap_reduce_kernel, dim3((unsigned)N), dim3(64), 0, s, (const float*)partials, out, (int)nb, (int)P, accumulate);
  LCV_LAUNCH_CHECK("lpips_tap_distance (reduce)");
  return LCV_OK;
}

extern "C" int64_t lcv_lpips_ws_bytes(int64_t N, int64_t H, int64_t W) {
  if (N <= 0 || H < 31 || W < 31) return 0;
  const int64_t h1 = (H + 4 - 11) / 4 + 1, w1 = (W + 4 - 11) / 4 + 1;      // conv1: k11 s4 p2
  const int64_t h2 = (h1 - 3) / 2 + 1, w2 = (w1 - 3) / 2 + 1;              // pool; conv2 keeps the size (k5 p2)
  const int64_t h3 = (h2 - 3) / 2 + 1, w3 = (w2 - 3) / 2 + 1;              // pool; conv3-5 keep the size (k3 p1)
  const int64_t B = 2 * N;
  int64_t bytes = 0;
  const int64_t regions[8] = {B * h1 * w1 * 64, B * h2 * w2 * 64, B * h2 * w2 * 192, B * h3 * w3 * 192,
                              B * h3 * w3 * 384, B * h3 * w3 * 256, B * h3 * w3 * 256, N * LCV_LPIPS_TAP_BLOCKS};
  for (int i = 0; i < 8; ++i) bytes += round_up(regions[i] * 4, 256);
  return bytes;
}

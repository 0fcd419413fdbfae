// The fp32 average of the masters over the optimizer steps (include/lcv_hip_ema.h): load e = join(h, l), update
// e = w - b * (w - e), and the swap that puts the average into the parameters (as a valid master) and the master into the
// average.  Same descriptor table, chunking (optim_common.h) and 16-byte packet / scalar-tail split as optim_master.hip and
// optim_anchor.hip; the format and the op sequence are master_elem.h's.  HBM-bound streaming kernels, per parameter: load
// 4 B read + 4 B written, update 8 + 4, swap 8 + 8.  Built with -ffp-contract=off.  Every output has one writer; no atomics,
// no LDS.
#include "master_elem.h"
#include "lcv_hip_ema.h"

enum { EMA_LOAD = 0, EMA_UPDATE = 1, EMA_SWAP = 2 };

// what one element does: `e` is written in every mode, (h, l) by the swap alone
template <int MODE>
__device__ __forceinline__ void ema_elem(bf16_t& h, short& l, float& e, float b) {
  const float w = master_join(h, l);
  if (MODE == EMA_LOAD) {
    e = w;
  } else if (MODE == EMA_UPDATE) {
    e = master_ema_elem(w, e, b);
  } else {
    master_split(e, h, l);
    e = w;
  }
}

template <int MODE>
__global__ __launch_bounds__(256) void master_ema_kernel(const lcv_adam_tensor* __restrict__ tensors, void* const* __restrict__ low,
                                                         void* const* __restrict__ ema, int n, float b) {
  const int ti = find_tensor(tensors, n, blockIdx.x);
  const lcv_adam_tensor t = tensors[ti];
  const int64_t base = ((int64_t)blockIdx.x - t.first_chunk) * CHUNK + threadIdx.x * 8;
  bf16_t* P = (bf16_t*)t.param;
  short* L = (short*)low[ti];
  float* E = (float*)ema[ti];
  if (base + 8 <= t.numel && ((((uintptr_t)P) | ((uintptr_t)L) | ((uintptr_t)E)) & 15) == 0) {   // whole 16-byte packets
    u16x8 hv = *reinterpret_cast<const u16x8*>(P + base);
    s16x8 lv = *reinterpret_cast<const s16x8*>(L + base);
    f32x4 ev[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
    if (MODE != EMA_LOAD) {
      ev[0] = *reinterpret_cast<const f32x4*>(E + base); ev[1] = *reinterpret_cast<const f32x4*>(E + base + 4);
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      bf16_t h = hv[e]; short l = lv[e];
      float a = ev[e >> 2][e & 3];
      ema_elem<MODE>(h, l, a, b);
      hv[e] = h; lv[e] = l; ev[e >> 2][e & 3] = a;
    }
    if (MODE == EMA_SWAP) {
      *reinterpret_cast<u16x8*>(P + base) = hv;
      *reinterpret_cast<s16x8*>(L + base) = lv;
    }
    *reinterpret_cast<f32x4*>(E + base) = ev[0]; *reinterpret_cast<f32x4*>(E + base + 4) = ev[1];
    return;
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int64_t i = base + e;
    if (i >= t.numel) break;
    bf16_t h = P[i]; short l = L[i];
    float a = MODE != EMA_LOAD ? E[i] : 0.f;
    ema_elem<MODE>(h, l, a, b);
    if (MODE == EMA_SWAP) { P[i] = h; L[i] = l; }
    E[i] = a;
  }
}

extern "C" int lcv_master_ema_load(const lcv_adam_tensor* tensors, void* const* low, void* const* ema, int64_t n_tensors,
                                   int64_t total_chunks, void* stream) {
  LCV_CHECK_ARG(tensors && low && ema && optim_table_ok(n_tensors, total_chunks), "master_ema_load: bad arguments");
  hipLaunchKernelGGL(master_ema_kernel<EMA_LOAD>, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)stream, tensors, low,
                     ema, (int)n_tensors, 0.f);
  LCV_LAUNCH_CHECK("master_ema_load");
  return LCV_OK;
}

extern "C" int lcv_master_ema_update(const lcv_adam_tensor* tensors, void* const* low, void* const* ema, int64_t n_tensors,
                                     int64_t total_chunks, double beta, void* stream) {
  LCV_CHECK_ARG(tensors && low && ema && optim_table_ok(n_tensors, total_chunks), "master_ema_update: bad arguments");
  LCV_CHECK_ARG(beta >= 0.0 && beta < 1.0, "master_ema_update: beta must be in [0, 1), got %g", beta);   // NaN fails both
  hipLaunchKernelGGL(master_ema_kernel<EMA_UPDATE>, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)stream, tensors,
                     low, ema, (int)n_tensors, (float)beta);
  LCV_LAUNCH_CHECK("master_ema_update");
  return LCV_OK;
}

extern "C" int lcv_master_ema_swap(const lcv_adam_tensor* tensors, void* const* low, void* const* ema, int64_t n_tensors,
                                   int64_t total_chunks, void* stream) {
  LCV_CHECK_ARG(tensors && low && ema && optim_table_ok(n_tensors, total_chunks), "master_ema_swap: bad arguments");
  hipLaunchKernelGGL(master_ema_kernel<EMA_SWAP>, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)stream, tensors, low,
                     ema, (int)n_tensors, 0.f);
  LCV_LAUNCH_CHECK("master_ema_swap");
  return LCV_OK;
}

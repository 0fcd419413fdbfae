// The sharpness-aware adaptation step (include/lcv_hip_sam.h): the sum of squares of the (plain or |w| + eta scaled) gradient per
// tensor and in total, in the fixed order the header writes down; the perturbation w' = w + rho * t / |t| with an exact save of
// every word the forward reads, decided on the device from that sum, and the sum of squares of what the stored words really
// moved by; and the restore of the saved words.  w is join(h, l) of a bf16 master-weight parameter, float(h) of a plain bf16
// one, or an fp32 value.  Same descriptor table, chunking (optim_common.h) and 16-byte packet / scalar-tail split as
// optim_trust.hip, whose reduction order this file repeats; the format is master_elem.h's.  HBM-bound streaming kernels (bytes
// per parameter in the header).  Built with -ffp-contract=off.  Every output has one writer and every sum a fixed order.
#include "master_elem.h"
#include "lcv_hip_sam.h"

// a workgroup of 256: the wave's butterfly, then the four waves in wave order; the sum is valid in thread 0
__device__ __forceinline__ float sam_block_sum(float acc) {
  __shared__ float part[4];
  acc = wave_sum(acc);
  if ((threadIdx.x & (LCV_WAVE - 1)) == 0) part[threadIdx.x / LCV_WAVE] = acc;
  __syncthreads();
  return ((part[0] + part[1]) + part[2]) + part[3];
}

// t = g, or (|w| + eta) * g; a is left for the perturbation
template <bool ADAPT>
__device__ __forceinline__ float sam_scaled(float w, float g, float eta, float& a) {
  if (!ADAPT) return g;
  a = __builtin_fabsf(w) + eta;
  return a * g;
}
// acc = acc + t * t, the product rounded before the sum
__device__ __forceinline__ float sam_sq_elem(float acc, float t) {
  const float q = t * t;
  return acc + q;
}
// w' = w + c * g, or w + c * ((|w| + eta) * t)
template <bool ADAPT>
__device__ __forceinline__ float sam_perturb_elem(float w, float g, float eta, float c) {
  float a = 0.f;
  const float t = sam_scaled<ADAPT>(w, g, eta, a);
  float e;
  if (ADAPT) {
    const float u = a * t;
    e = c * u;
  } else {
    e = c * g;
  }
  return w + e;
}

// ---- step 1 of the gradient's sum: one fp32 partial per chunk, a thread's 8 elements in index order ----
template <bool F32, bool ADAPT>
__global__ __launch_bounds__(256) void sam_chunk_kernel(const lcv_adam_tensor* __restrict__ tensors, void* const* __restrict__ low,
                                                        int n, float eta, float* __restrict__ partials) {
  const int ti = find_tensor(tensors, n, blockIdx.x);
  const lcv_adam_tensor t = tensors[ti];
  const int64_t base = ((int64_t)blockIdx.x - t.first_chunk) * CHUNK + threadIdx.x * 8;
  float acc = 0.f, a = 0.f;
  if (F32) {
    const float* P = (const float*)t.param;
    const float* G = (const float*)t.grad;
    if (base + 8 <= t.numel && ((((uintptr_t)G) | (ADAPT ? (uintptr_t)P : 0)) & 15) == 0) {     // whole 16-byte packets
      float g[8], w[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      load8(G + base, g);
      if (ADAPT) load8(P + base, w);                                   // plain: the parameters are not read
#pragma unroll
      for (int e = 0; e < 8; ++e) acc = sam_sq_elem(acc, sam_scaled<ADAPT>(w[e], g[e], eta, a));
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int64_t i = base + e;
        if (i < t.numel) acc = sam_sq_elem(acc, sam_scaled<ADAPT>(ADAPT ? P[i] : 0.f, G[i], eta, a));
      }
    }
  } else {
    const bf16_t* P = (const bf16_t*)t.param;
    const bf16_t* G = (const bf16_t*)t.grad;
    const short* L = (ADAPT && low) ? (const short*)low[ti] : nullptr;  // no low words: every one of them is zero
    if (base + 8 <= t.numel && ((((uintptr_t)G) | (ADAPT ? ((uintptr_t)P | (uintptr_t)L) : 0)) & 15) == 0) {
      const u16x8 gv = *reinterpret_cast<const u16x8*>(G + base);
      u16x8 hv = {0, 0, 0, 0, 0, 0, 0, 0};
      s16x8 lv = {0, 0, 0, 0, 0, 0, 0, 0};
      if (ADAPT) hv = *reinterpret_cast<const u16x8*>(P + base);
      if (L) lv = *reinterpret_cast<const s16x8*>(L + base);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc = sam_sq_elem(acc, sam_scaled<ADAPT>(master_join(hv[e], lv[e]), bf2f(gv[e]), eta, a));
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int64_t i = base + e;
        if (i < t.numel) {
          const float w = ADAPT ? master_join(P[i], L ? L[i] : (short)0) : 0.f;
          acc = sam_sq_elem(acc, sam_scaled<ADAPT>(w, bf2f(G[i]), eta, a));
        }
      }
    }
  }
  const float s = sam_block_sum(acc);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// ---- step 2: one workgroup per tensor adds that tensor's partials, thread t taking t, t + 256, ... in index order ----
__global__ __launch_bounds__(256) void sam_tensor_kernel(const lcv_adam_tensor* __restrict__ tensors,
                                                         const float* __restrict__ partials, float* __restrict__ per_tensor) {
  const lcv_adam_tensor t = tensors[blockIdx.x];
  const int64_t chunks = (t.numel + CHUNK - 1) / CHUNK;
  const float* p = partials + t.first_chunk;
  float acc = 0.f;
  for (int64_t c = threadIdx.x; c < chunks; c += 256) acc = acc + p[c];
  const float s = sam_block_sum(acc);
  if (threadIdx.x == 0) per_tensor[blockIdx.x] = s;
}

// ---- step 3: one workgroup adds per_tensor[0..n), thread t taking t, t + 256, ... in index order; the perturbation's record ----
__global__ __launch_bounds__(256) void sam_total_kernel(const float* __restrict__ per_tensor, int n, float* __restrict__ out,
                                                        const float* __restrict__ sumsq, float* __restrict__ trace) {
  float acc = 0.f;
  for (int k = threadIdx.x; k < n; k += 256) acc = acc + per_tensor[k];
  const float s = sam_block_sum(acc);
  if (threadIdx.x == 0) {
    out[0] = s;
    out[1] = __builtin_sqrtf(s);
    if (trace) {                         // the step's record: the gradient's total and what the stored words moved by
      trace[0] = sumsq[0];
      trace[1] = s;
    }
  }
}

// ---- the perturbation: save the word the forward reads, store the perturbed word, one partial of the realized move per chunk ----
template <bool F32, bool ADAPT>
__global__ __launch_bounds__(256) void sam_perturb_kernel(const lcv_adam_tensor* __restrict__ tensors, void* const* __restrict__ low,
                                                          void* const* __restrict__ save, int n, float eta, float rho,
                                                          const float* __restrict__ sumsq, float* __restrict__ partials) {
  const int ti = find_tensor(tensors, n, blockIdx.x);
  const lcv_adam_tensor t = tensors[ti];
  const int64_t base = ((int64_t)blockIdx.x - t.first_chunk) * CHUNK + threadIdx.x * 8;
  const float s = sumsq[0];
  // rho = 0, a zero, negative or NaN total, an overflowed total: the saves are written and no parameter byte is
  const bool move = rho != 0.f && s > 0.f && s != __builtin_inff();
  float c = 0.f;
  if (move) {
    const float nrm = __builtin_sqrtf(s);
    const float den = nrm + 1e-12f;
    c = rho / den;
  }
  float acc = 0.f;
  if (F32) {
    float* P = (float*)t.param;
    const float* G = (const float*)t.grad;
    float* S = (float*)save[ti];
    if (base + 8 <= t.numel && ((((uintptr_t)P) | ((uintptr_t)G) | ((uintptr_t)S)) & 15) == 0) {     // whole 16-byte packets
      float w[8], g[8];
      load8(P + base, w);
      store8(S + base, w);
      if (move) {
        load8(G + base, g);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float wp = sam_perturb_elem<ADAPT>(w[e], g[e], eta, c);
          const float d = wp - w[e];
          acc = sam_sq_elem(acc, d);
          w[e] = wp;
        }
        store8(P + base, w);
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int64_t i = base + e;
        if (i >= t.numel) break;
        const float w = P[i];
        S[i] = w;
        if (move) {
          const float wp = sam_perturb_elem<ADAPT>(w, G[i], eta, c);
          const float d = wp - w;
          acc = sam_sq_elem(acc, d);
          P[i] = wp;
        }
      }
    }
  } else {
    bf16_t* P = (bf16_t*)t.param;
    const bf16_t* G = (const bf16_t*)t.grad;
    const short* L = low ? (const short*)low[ti] : nullptr;           // no low words: every one of them is zero
    bf16_t* S = (bf16_t*)save[ti];
    if (base + 8 <= t.numel && ((((uintptr_t)P) | ((uintptr_t)G) | ((uintptr_t)L) | ((uintptr_t)S)) & 15) == 0) {
      u16x8 hv = *reinterpret_cast<const u16x8*>(P + base);
      *reinterpret_cast<u16x8*>(S + base) = hv;
      if (move) {
        const u16x8 gv = *reinterpret_cast<const u16x8*>(G + base);
        s16x8 lv = {0, 0, 0, 0, 0, 0, 0, 0};
        if (L) lv = *reinterpret_cast<const s16x8*>(L + base);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const bf16_t hp = f2bf(sam_perturb_elem<ADAPT>(master_join(hv[e], lv[e]), bf2f(gv[e]), eta, c));
          const float d = bf2f(hp) - bf2f(hv[e]);
          acc = sam_sq_elem(acc, d);
          hv[e] = hp;
        }
        *reinterpret_cast<u16x8*>(P + base) = hv;                     // the low words are read, never written
      }
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int64_t i = base + e;
        if (i >= t.numel) break;
        const bf16_t h = P[i];
        S[i] = h;
        if (move) {
          const bf16_t hp = f2bf(sam_perturb_elem<ADAPT>(master_join(h, L ? L[i] : (short)0), bf2f(G[i]), eta, c));
          const float d = bf2f(hp) - bf2f(h);
          acc = sam_sq_elem(acc, d);
          P[i] = hp;
        }
      }
    }
  }
  const float r = sam_block_sum(acc);
  if (threadIdx.x == 0) partials[blockIdx.x] = r;
}

// ---- the restore: param = save, word for word ----
template <bool F32>
__global__ __launch_bounds__(256) void sam_restore_kernel(const lcv_adam_tensor* __restrict__ tensors, void* const* __restrict__ save,
                                                          int n) {
  const int ti = find_tensor(tensors, n, blockIdx.x);
  const lcv_adam_tensor t = tensors[ti];
  const int64_t base = ((int64_t)blockIdx.x - t.first_chunk) * CHUNK + threadIdx.x * 8;
  if (F32) {
    float* P = (float*)t.param;
    const float* S = (const float*)save[ti];
    if (base + 8 <= t.numel && ((((uintptr_t)P) | ((uintptr_t)S)) & 15) == 0) {
      float w[8];
      load8(S + base, w);
      store8(P + base, w);
      return;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int64_t i = base + e;
      if (i >= t.numel) break;
      P[i] = S[i];
    }
  } else {
    bf16_t* P = (bf16_t*)t.param;
    const bf16_t* S = (const bf16_t*)save[ti];
    if (base + 8 <= t.numel && ((((uintptr_t)P) | ((uintptr_t)S)) & 15) == 0) {
      *reinterpret_cast<u16x8*>(P + base) = *reinterpret_cast<const u16x8*>(S + base);
      return;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int64_t i = base + e;
      if (i >= t.numel) break;
      P[i] = S[i];
    }
  }
}

// finite and >= 0 (a NaN fails the first comparison)
static inline bool sam_scalar_ok(double v) { return v >= 0.0 && v <= 3.4028234663852886e38; }

// launch KERNEL<F32, ADAPT> over `grid` on stream `s` (both the caller's locals)
#define SAM_PICK(KERNEL, f32, adapt, ...)                                                                        \
  do {                                                                                                           \
    if (f32 && adapt) hipLaunchKernelGGL((KERNEL<true, true>), grid, dim3(256), 0, s, __VA_ARGS__);               \
    else if (f32) hipLaunchKernelGGL((KERNEL<true, false>), grid, dim3(256), 0, s, __VA_ARGS__);                  \
    else if (adapt) hipLaunchKernelGGL((KERNEL<false, true>), grid, dim3(256), 0, s, __VA_ARGS__);                \
    else hipLaunchKernelGGL((KERNEL<false, false>), grid, dim3(256), 0, s, __VA_ARGS__);                          \
  } while (0)

extern "C" int lcv_sam_sumsq(const lcv_adam_tensor* tensors, void* const* low, int64_t n_tensors, int64_t total_chunks,
                             int param_f32, int adaptive, double eta, float* partials, int64_t partials_bytes, float* per_tensor,
                             float* out, void* stream) {
  LCV_CHECK_ARG(tensors && per_tensor && out && optim_table_ok(n_tensors, total_chunks), "sam_sumsq: bad arguments");
  LCV_CHECK_ARG(!(param_f32 && low), "sam_sumsq: param_f32 = 1 takes no low words (low must be NULL)");
  LCV_CHECK_ARG(sam_scalar_ok(eta), "sam_sumsq: eta must be finite and >= 0, got %g", eta);
  LCV_CHECK_ARG(partials && partials_bytes >= total_chunks * 4 && ((uintptr_t)partials % 4) == 0,
                "sam_sumsq: workspace of %ld bytes is missing or too small (need %ld)", (long)partials_bytes,
                (long)(total_chunks * 4));
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)total_chunks);
  SAM_PICK(sam_chunk_kernel, param_f32, adaptive, tensors, low, (int)n_tensors, (float)eta, partials);
  LCV_LAUNCH_CHECK("sam_sumsq: chunks");
  hipLaunchKernelGGL(sam_tensor_kernel, dim3((unsigned)n_tensors), dim3(256), 0, s, tensors, partials, per_tensor);
  LCV_LAUNCH_CHECK("sam_sumsq: tensors");
  hipLaunchKernelGGL(sam_total_kernel, dim3(1), dim3(256), 0, s, per_tensor, (int)n_tensors, out, (const float*)nullptr,
                     (float*)nullptr);
  LCV_LAUNCH_CHECK("sam_sumsq: total");
  return LCV_OK;
}

extern "C" int lcv_sam_perturb(const lcv_adam_tensor* tensors, void* const* low, void* const* save, int64_t n_tensors,
                               int64_t total_chunks, int param_f32, int adaptive, double eta, double rho, const float* sumsq,
                               float* partials, int64_t partials_bytes, float* per_tensor, float* realized, float* trace_slot,
                               void* stream) {
  LCV_CHECK_ARG(tensors && save && sumsq && per_tensor && realized && optim_table_ok(n_tensors, total_chunks),
                "sam_perturb: bad arguments");
  LCV_CHECK_ARG(!(param_f32 && low), "sam_perturb: param_f32 = 1 takes no low words (low must be NULL)");
  LCV_CHECK_ARG(sam_scalar_ok(rho), "sam_perturb: rho must be finite and >= 0, got %g", rho);
  LCV_CHECK_ARG(sam_scalar_ok(eta), "sam_perturb: eta must be finite and >= 0, got %g", eta);
  LCV_CHECK_ARG(partials && partials_bytes >= total_chunks * 4 && ((uintptr_t)partials % 4) == 0,
                "sam_perturb: workspace of %ld bytes is missing or too small (need %ld)", (long)partials_bytes,
                (long)(total_chunks * 4));
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((unsigned)total_chunks);
  SAM_PICK(sam_perturb_kernel, param_f32, adaptive, tensors, low, save, (int)n_tensors, (float)eta, (float)rho, sumsq, partials);
  LCV_LAUNCH_CHECK("sam_perturb: chunks");
  hipLaunchKernelGGL(sam_tensor_kernel, dim3((unsigned)n_tensors), dim3(256), 0, s, tensors, partials, per_tensor);
  LCV_LAUNCH_CHECK("sam_perturb: tensors");
  hipLaunchKernelGGL(sam_total_kernel, dim3(1), dim3(256), 0, s, per_tensor, (int)n_tensors, realized, sumsq, trace_slot);
  LCV_LAUNCH_CHECK("sam_perturb: total");
  return LCV_OK;
}

extern "C" int lcv_sam_restore(const lcv_adam_tensor* tensors, void* const* save, int64_t n_tensors, int64_t total_chunks,
                               int param_f32, void* stream) {
  LCV_CHECK_ARG(tensors && save && optim_table_ok(n_tensors, total_chunks), "sam_restore: bad arguments");
  hipStream_t s = (hipStream_t)stream;
  if (param_f32)
    hipLaunchKernelGGL(sam_restore_kernel<true>, dim3((unsigned)total_chunks), dim3(256), 0, s, tensors, save, (int)n_tensors);
  else
    hipLaunchKernelGGL(sam_restore_kernel<false>, dim3((unsigned)total_chunks), dim3(256), 0, s, tensors, save, (int)n_tensors);
  LCV_LAUNCH_CHECK("sam_restore");
  return LCV_OK;
}

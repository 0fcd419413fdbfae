// The trust-region cap on the drift from the base weights (include/lcv_hip_trust.h): the sum of squares of w - w0 per tensor
// and in total, in the fixed order the header writes down, and the projection w = w0 + c * (w - w0) of the tensors whose ball
// is exceeded, decided on the device from that sum.  w is join(h, l) of a bf16 master-weight parameter or an fp32 value; w0 the
// bf16 base word widened, the fp32 base value, or zero without an anchor.  Same descriptor table, chunking (optim_common.h) and
// 16-byte packet / scalar-tail split as optim_anchor.hip and optim_ema.hip; the format and the element op sequence are
// master_elem.h's.  HBM-bound streaming kernels (bytes per parameter in the header).  Built with -ffp-contract=off.  Every output
// has one writer and every sum a fixed order.
#include "master_elem.h"
#include "lcv_hip_trust.h"

// a = a + d * d, the product rounded before the sum
__device__ __forceinline__ float trust_sq_elem(float acc, float w, float w0) {
  const float d = w - w0;
  const float q = d * d;
  return acc + q;
}

// a workgroup of 256: the wave's butterfly, then the four waves in wave order; the sum is valid in thread 0
__device__ __forceinline__ float trust_block_sum(float acc) {
  __shared__ float part[4];
  acc = wave_sum(acc);
  if ((threadIdx.x & (LCV_WAVE - 1)) == 0) part[threadIdx.x / LCV_WAVE] = acc;
  __syncthreads();
  return ((part[0] + part[1]) + part[2]) + part[3];
}

// ---- step 1: one fp32 partial per chunk, a thread's 8 elements in index order ----
template <bool F32>
__global__ __launch_bounds__(256) void trust_chunk_kernel(const lcv_adam_tensor* __restrict__ tensors, void* const* __restrict__ low,
                                                          void* const* __restrict__ anchor, int n, float* __restrict__ partials) {
  const int ti = find_tensor(tensors, n, blockIdx.x);
  const lcv_adam_tensor t = tensors[ti];
  const int64_t base = ((int64_t)blockIdx.x - t.first_chunk) * CHUNK + threadIdx.x * 8;
  float acc = 0.f;
  if (F32) {
    const float* P = (const float*)t.param;
    const float* A = anchor ? (const float*)anchor[ti] : nullptr;     // no anchor: every base value is zero
    if (base + 8 <= t.numel && ((((uintptr_t)P) | ((uintptr_t)A)) & 15) == 0) {     // whole 16-byte packets
      float w[8], a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      load8(P + base, w);
      if (A) load8(A + base, a);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc = trust_sq_elem(acc, w[e], a[e]);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int64_t i = base + e;
        if (i < t.numel) acc = trust_sq_elem(acc, P[i], A ? A[i] : 0.f);
      }
    }
  } else {
    const bf16_t* P = (const bf16_t*)t.param;
    const short* L = low ? (const short*)low[ti] : nullptr;           // no low words: every one of them is zero
    const bf16_t* A = anchor ? (const bf16_t*)anchor[ti] : nullptr;
    if (base + 8 <= t.numel && ((((uintptr_t)P) | ((uintptr_t)L) | ((uintptr_t)A)) & 15) == 0) {
      const u16x8 hv = *reinterpret_cast<const u16x8*>(P + base);
      u16x8 av = {0, 0, 0, 0, 0, 0, 0, 0};
      s16x8 lv = {0, 0, 0, 0, 0, 0, 0, 0};
      if (A) av = *reinterpret_cast<const u16x8*>(A + base);
      if (L) lv = *reinterpret_cast<const s16x8*>(L + base);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc = trust_sq_elem(acc, master_join(hv[e], lv[e]), bf2f(av[e]));
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const int64_t i = base + e;
        if (i < t.numel) acc = trust_sq_elem(acc, master_join(P[i], L ? L[i] : (short)0), A ? bf2f(A[i]) : 0.f);
      }
    }
  }
  const float s = trust_block_sum(acc);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

// ---- step 2: one workgroup per tensor adds that tensor's partials, thread t taking t, t + 256, ... in index order ----
__global__ __launch_bounds__(256) void trust_tensor_kernel(const lcv_adam_tensor* __restrict__ tensors,
                                                           const float* __restrict__ partials, float* __restrict__ per_tensor) {
  const lcv_adam_tensor t = tensors[blockIdx.x];
  const int64_t chunks = (t.numel + CHUNK - 1) / CHUNK;
  const float* p = partials + t.first_chunk;
  float acc = 0.f;
  for (int64_t c = threadIdx.x; c < chunks; c += 256) acc = acc + p[c];
  const float s = trust_block_sum(acc);
  if (threadIdx.x == 0) per_tensor[blockIdx.x] = s;
}

// ---- step 3: one workgroup adds per_tensor[0..n), thread t taking t, t + 256, ... in index order ----
__global__ __launch_bounds__(256) void trust_total_kernel(const float* __restrict__ per_tensor, int n, float* __restrict__ out) {
  float acc = 0.f;
  for (int k = threadIdx.x; k < n; k += 256) acc = acc + per_tensor[k];
  const float s = trust_block_sum(acc);
  if (threadIdx.x == 0) {
    out[0] = s;
    out[1] = __builtin_sqrtf(s);
  }
}

// ---- the projection ----
// the radius of tensor numel's ball, squared: (float)(R * R * N), the caller's product for the whole run, or R * R times the
// tensor's element count, formed in double and rounded once
__device__ __forceinline__ float trust_r2(int scope, double rr, int64_t numel) {
  return scope == LCV_TRUST_TENSOR ? (float)(rr * (double)numel) : (float)rr;
}
// 1 inside the ball (and for a NaN s), else sqrt(r2 / s), both correctly rounded
__device__ __forceinline__ float trust_coef(float s, float r2) {
  if (!(s > r2)) return 1.f;
  const float q = r2 / s;
  return __builtin_sqrtf(q);
}

template <bool F32>
__global__ __launch_bounds__(256) void trust_project_kernel(const lcv_adam_tensor* __restrict__ tensors, void* const* __restrict__ low,
                                                            void* const* __restrict__ anchor, int n, int scope,
                                                            const float* __restrict__ sumsq, const float* __restrict__ per_tensor,
                                                            double rr, float* __restrict__ trace) {
  if (blockIdx.x == 0 && trace) {        // the step's record: the total before the projection and the smallest coefficient
    float cmin = 1.f;
    if (scope == LCV_TRUST_TENSOR) {
      for (int k = threadIdx.x; k < n; k += 256) cmin = fminf(cmin, trust_coef(per_tensor[k], trust_r2(scope, rr, tensors[k].numel)));
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) cmin = fminf(cmin, __shfl_xor(cmin, o, 64));
      __shared__ float cpart[4];
      if ((threadIdx.x & (LCV_WAVE - 1)) == 0) cpart[threadIdx.x / LCV_WAVE] = cmin;
      __syncthreads();
      cmin = fminf(fminf(cpart[0], cpart[1]), fminf(cpart[2], cpart[3]));
    } else {
      cmin = trust_coef(sumsq[0], trust_r2(scope, rr, 0));
    }
    if (threadIdx.x == 0) {
      trace[0] = sumsq[0];
      trace[1] = cmin;
    }
  }
  const int ti = find_tensor(tensors, n, blockIdx.x);
  const lcv_adam_tensor t = tensors[ti];
  const float s = scope == LCV_TRUST_TENSOR ? per_tensor[ti] : sumsq[0];
  const float r2 = trust_r2(scope, rr, t.numel);
  if (!(s > r2)) return;                 // inside the ball (or a NaN sum): nothing of this tensor is written
  const float q = r2 / s;
  const float c = __builtin_sqrtf(q);
  const int64_t base = ((int64_t)blockIdx.x - t.first_chunk) * CHUNK + threadIdx.x * 8;
  if (F32) {
    float* P = (float*)t.param;
    const float* A = anchor ? (const float*)anchor[ti] : nullptr;
    if (base + 8 <= t.numel && ((((uintptr_t)P) | ((uintptr_t)A)) & 15) == 0) {     // whole 16-byte packets
      float w[8], a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      load8(P + base, w);
      if (A) load8(A + base, a);
#pragma unroll
      for (int e = 0; e < 8; ++e) w[e] = master_trust_elem(w[e], a[e], c);
      store8(P + base, w);
      return;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int64_t i = base + e;
      if (i >= t.numel) break;
      P[i] = master_trust_elem(P[i], A ? A[i] : 0.f, c);
    }
  } else {
    bf16_t* P = (bf16_t*)t.param;
    short* L = (short*)low[ti];
    const bf16_t* A = anchor ? (const bf16_t*)anchor[ti] : nullptr;
    if (base + 8 <= t.numel && ((((uintptr_t)P) | ((uintptr_t)L) | ((uintptr_t)A)) & 15) == 0) {
      u16x8 hv = *reinterpret_cast<const u16x8*>(P + base);
      s16x8 lv = *reinterpret_cast<const s16x8*>(L + base);
      u16x8 av = {0, 0, 0, 0, 0, 0, 0, 0};
      if (A) av = *reinterpret_cast<const u16x8*>(A + base);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        bf16_t h; short l;
        master_split(master_trust_elem(master_join(hv[e], lv[e]), bf2f(av[e]), c), h, l);
        hv[e] = h; lv[e] = l;
      }
      *reinterpret_cast<u16x8*>(P + base) = hv;
      *reinterpret_cast<s16x8*>(L + base) = lv;
      return;
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int64_t i = base + e;
      if (i >= t.numel) break;
      bf16_t h; short l;
      master_split(master_trust_elem(master_join(P[i], L[i]), A ? bf2f(A[i]) : 0.f, c), h, l);
      P[i] = h; L[i] = l;
    }
  }
}

extern "C" int lcv_trust_sumsq(const lcv_adam_tensor* tensors, void* const* low, void* const* anchor, int64_t n_tensors,
                               int64_t total_chunks, int param_f32, float* partials, int64_t partials_bytes, float* per_tensor,
                               float* out, void* stream) {
  LCV_CHECK_ARG(tensors && per_tensor && out && optim_table_ok(n_tensors, total_chunks), "trust_sumsq: bad arguments");
  LCV_CHECK_ARG(!(param_f32 && low), "trust_sumsq: param_f32 = 1 takes no low words (low must be NULL)");
  LCV_CHECK_ARG(partials && partials_bytes >= total_chunks * 4 && ((uintptr_t)partials % 4) == 0,
                "trust_sumsq: workspace of %ld bytes is missing or too small (need %ld)", (long)partials_bytes,
                (long)(total_chunks * 4));
  hipStream_t s = (hipStream_t)stream;
  if (param_f32)
    hipLaunchKernelGGL(trust_chunk_kernel<true>, dim3((unsigned)total_chunks), dim3(256), 0, s, tensors, low, anchor, (int)n_tensors,
                       partials);
  else
    hipLaunchKernelGGL(trust_chunk_kernel<false>, dim3((unsigned)total_chunks), dim3(256), 0, s, tensors, low, anchor,
                       (int)n_tensors, partials);
  LCV_LAUNCH_CHECK("trust_sumsq: chunks");
  hipLaunchKernelGGL(trust_tensor_kernel, dim3((unsigned)n_tensors), dim3(256), 0, s, tensors, partials, per_tensor);
  LCV_LAUNCH_CHECK("trust_sumsq: tensors");
  hipLaunchKernelGGL(trust_total_kernel, dim3(1), dim3(256), 0, s, per_tensor, (int)n_tensors, out);
  LCV_LAUNCH_CHECK("trust_sumsq: total");
  return LCV_OK;
}

extern "C" int lcv_trust_project(const lcv_adam_tensor* tensors, void* const* low, void* const* anchor, int64_t n_tensors,
                                 int64_t total_chunks, int param_f32, int scope, const float* sumsq, const float* per_tensor,
                                 double r2_or_R2, float* trace_slot, void* stream) {
  LCV_CHECK_ARG(tensors && sumsq && optim_table_ok(n_tensors, total_chunks), "trust_project: bad arguments");
  LCV_CHECK_ARG(scope == LCV_TRUST_GLOBAL || scope == LCV_TRUST_TENSOR, "trust_project: scope must be 0 (global) or 1 (tensor), got %d",
                scope);
  LCV_CHECK_ARG(scope == LCV_TRUST_GLOBAL || per_tensor, "trust_project: tensor scope reads per_tensor");
  LCV_CHECK_ARG(r2_or_R2 > 0.0, "trust_project: the squared radius must be > 0, got %g", r2_or_R2);      // a NaN fails too
  if (param_f32)
    LCV_CHECK_ARG(!low, "trust_project: param_f32 = 1 takes no low words (low must be NULL)");
  else
    LCV_CHECK_ARG(low, "trust_project: bf16 parameters need their low words (a plain bf16 word cannot hold the bound)");
  hipStream_t s = (hipStream_t)stream;
  if (param_f32)
    hipLaunchKernelGGL(trust_project_kernel<true>, dim3((unsigned)total_chunks), dim3(256), 0, s, tensors, low, anchor,
                       (int)n_tensors, scope, sumsq, per_tensor, r2_or_R2, trace_slot);
  else
    hipLaunchKernelGGL(trust_project_kernel<false>, dim3((unsigned)total_chunks), dim3(256), 0, s, tensors, low, anchor,
                       (int)n_tensors, scope, sumsq, per_tensor, r2_or_R2, trace_slot);
  LCV_LAUNCH_CHECK("trust_project");
  return LCV_OK;
}

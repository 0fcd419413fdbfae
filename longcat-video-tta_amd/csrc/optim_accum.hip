// fp32 gradient accumulation over micro-steps (include/lcv_hip_accum.h): every parameter element carries an fp32 accumulator,
// each micro-step's bf16 gradient is scaled and added into it, and the master-weight steps read it as the gradient (their
// fp32-gradient forms: optim_master.hip).  Same descriptor table, chunking (optim_common.h) and 16-byte packet / scalar-tail
// split as optim_master.hip.  HBM-bound streaming kernel: 6 B read + 4 B written per element.  Built with -ffp-contract=off:
// a product never fuses with the sum that takes it.
#include "master_elem.h"   // contraction off from there on
#include "lcv_hip_accum.h"

// t = float(g) * s;  a = a + t  - always the add, so 0 + t carries IEEE addition's sign of zero
__device__ __forceinline__ float accum_elem(float a, float g, float s) {
  const float t = g * s;
  return a + t;
}

__global__ __launch_bounds__(256) void grad_accumulate_kernel(const lcv_adam_tensor* __restrict__ tensors,
                                                              void* const* __restrict__ acc, int n, float s) {
  const int ti = find_tensor(tensors, n, blockIdx.x);
  const lcv_adam_tensor t = tensors[ti];
  const int64_t base = ((int64_t)blockIdx.x - t.first_chunk) * CHUNK + threadIdx.x * 8;
  const bf16_t* G = (const bf16_t*)t.grad;
  float* A = (float*)acc[ti];
  if (base + 8 <= t.numel && ((((uintptr_t)G) | ((uintptr_t)A)) & 15) == 0) {   // whole 16-byte packets
    const u16x8 gv = *reinterpret_cast<const u16x8*>(G + base);
    f32x4 av[2];
    av[0] = *reinterpret_cast<const f32x4*>(A + base); av[1] = *reinterpret_cast<const f32x4*>(A + base + 4);
#pragma unroll
    for (int e = 0; e < 8; ++e) av[e >> 2][e & 3] = accum_elem(av[e >> 2][e & 3], bf2f(gv[e]), s);
    *reinterpret_cast<f32x4*>(A + base) = av[0]; *reinterpret_cast<f32x4*>(A + base + 4) = av[1];
    return;
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int64_t i = base + e;
    if (i >= t.numel) break;
    A[i] = accum_elem(A[i], bf2f(G[i]), s);
  }
}

extern "C" int lcv_grad_accumulate(const lcv_adam_tensor* tensors, void* const* acc, int64_t n_tensors, int64_t total_chunks,
                                   double scale, void* stream) {
  LCV_CHECK_ARG(tensors && acc && optim_table_ok(n_tensors, total_chunks), "grad_accumulate: bad arguments");
  hipLaunchKernelGGL(grad_accumulate_kernel, dim3((unsigned)total_chunks), dim3(256), 0, (hipStream_t)stream, tensors, acc,
                     (int)n_tensors, (float)scale);
  LCV_LAUNCH_CHECK("grad_accumulate");
  return LCV_OK;
}

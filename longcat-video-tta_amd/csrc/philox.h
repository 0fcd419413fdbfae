// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11) and the LoRA dropout mask built on
// it (include/lcv_hip_lora.h has the definition; tests/lora_dropout_ref.py restates it in numpy).  Plain integer C++ for
// host and device: the known-answer vectors of the paper's reference code hold for both.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define LCV_PHILOX_FN __host__ __device__ __forceinline__
#else
#define LCV_PHILOX_FN inline
#endif

struct philox_out {
  uint32_t c[4];
};

LCV_PHILOX_FN philox_out philox4x32_10(uint32_t k0, uint32_t k1, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
    const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;   // the key schedule: bumped after every round (the bump after the tenth is unused)
    k1 += 0xBB67AE85u;
  }
  return philox_out{{c0, c1, c2, c3}};
}

// Keep bits of the 8 elements of group `g` (g = global element index >> 3): bit e is set iff element e is kept.
// Element e takes the low (even e) or high (odd e) 16-bit half of output word e >> 1 and is kept iff half >= T.
LCV_PHILOX_FN unsigned lora_keep8(uint64_t seed, uint64_t offset, uint64_t g, uint32_t T) {
  const philox_out r = philox4x32_10((uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)offset, (uint32_t)(offset >> 32),
                                     (uint32_t)g, (uint32_t)(g >> 32));
  unsigned keep = 0;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const uint32_t half = (r.c[e >> 1] >> (16 * (e & 1))) & 0xffffu;
    keep |= (half >= T ? 1u : 0u) << e;
  }
  return keep;
}

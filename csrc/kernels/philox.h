// Counter-based Philox4x32-10, shared by the shard generator (datagen.hip) and the input
// pipeline (cnn_aux.hip input_aug_kernel, input_mix_kernel).  The fourth counter word names the
// stream, so two users never collide under one seed: 0 = shard generation, 1 = epoch shuffle,
// 2 = crop / flip, 3 = mixup / CutMix.
// numpy twin: serverless_learn_amd/data/device_synth.py philox4x32_10.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace sl {

struct U4 {
  uint32_t x, y, z, w;
};

__device__ __host__ inline U4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                            uint32_t k1) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)M0 * c0, p1 = (uint64_t)M1 * c2;
    const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
    const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
    const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    k0 += W0; k1 += W1;
  }
  return U4{c0, c1, c2, c3};
}

}  // namespace sl

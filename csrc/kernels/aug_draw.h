// The per-sample draw of the training input pipeline, shared by cnn_aux.hip (input_aug_kernel,
// input_mix_kernel), input_ta.hip (input_ta_kernel) and input_rrc.hip (input_rrc_kernel, the record
// alone): one copy, so the kernels agree on the record, the offsets and the flip of a sample bit for bit.
#pragma once
#include <stdint.h>

#include "philox.h"

namespace sl {

// murmur3 finalizer: the round function of the shuffle's Feistel network
__device__ __forceinline__ uint32_t fmix32(uint32_t x) {
  x ^= x >> 16;
  x *= 0x85EBCA6Bu;
  x ^= x >> 13;
  x *= 0xC2B2AE35u;
  x ^= x >> 16;
  return x;
}

// (record, oy, ox, flip) of sample j of the batch at cursor t (serverless_learn_amd/data/augment.py
// is the definition): record perm_e(b*B + j) of the shard (e = t / nb, b = t % nb; a 4-round Feistel
// bijection of [0, 2^(2h)) keyed by Philox(e; stream 1), cycle-walked into [0, N)), offsets and flip
// from Philox(t, j; stream 2).  Everything depends on kernel arguments, j and the cursor alone: with
// j uniform in a workgroup it is computed once per workgroup, in scalar registers.
// flags: 1 = shuffle, 2 = crop + flip.
struct AugDraw {
  uint32_t rec;
  int oy, ox, flip;
};

__device__ __forceinline__ AugDraw aug_draw(uint32_t j, uint32_t t, uint32_t n_records, uint32_t batch, int pad,
                                            int flags, int half_bits, uint32_t k0, uint32_t k1) {
  const uint32_t nb = n_records / batch;
  const uint32_t e = t / nb, b = t - e * nb;
  uint32_t rec = b * batch + j;  // < nb * batch <= n_records
  if (flags & 1) {
    const U4 key = philox4x32_10(e, 0u, 0u, 1u, k0, k1);
    const uint32_t kk[4] = {key.x, key.y, key.z, key.w};
    const uint32_t mask = (1u << half_bits) - 1u;
    // a bijection of [0, 2^(2h)) iterated from a value below n_records comes back below it: the
    // walk ends, and rec < n_records keeps every load inside the shard
    do {
      uint32_t L = rec >> half_bits, R = rec & mask;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const uint32_t nr = L ^ (fmix32(R + kk[i]) & mask);
        L = R;
        R = nr;
      }
      rec = (L << half_bits) | R;
    } while (rec >= n_records);
  }
  int oy = pad, ox = pad, flip = 0;
  if (flags & 2) {
    const U4 r = philox4x32_10(t, 0u, j, 2u, k0, k1);
    const uint32_t span = 2u * (uint32_t)pad + 1u;
    oy = (int)(r.x % span);
    ox = (int)(r.y % span);
    flip = (int)(r.z & 1u);
  }
  return AugDraw{rec, oy, ox, flip};
}

// One augmented pixel of a sample, as input_aug reads it: u8 channels in the low three bytes.
__device__ __forceinline__ uint32_t aug_pixel(const uint8_t* __restrict__ src, const AugDraw& d, int py, int px,
                                              int H, int W, int pad) {
  const int sy = py + d.oy - pad, sx = (d.flip ? W - 1 - px : px) + d.ox - pad;
  uint32_t v = 0;  // outside the image: black
  if ((unsigned)sy < (unsigned)H && (unsigned)sx < (unsigned)W) {
    const uint8_t* s = src + ((long)sy * W + sx) * 3;
    v = (uint32_t)s[0] | (uint32_t)s[1] << 8 | (uint32_t)s[2] << 16;
  }
  return v;
}

}  // namespace sl

// Memory-bound companions of the implicit-GEMM convolutions for the
// ResNet-18-shaped CNN (K6, K10, K11, K12, K4 of SURVEY.md §2.5).  All
// activations are NHWC bf16 with C a multiple of 8, so every kernel moves
// 16 B (8 channels) per thread per access; per-channel reductions keep a
// thread's 8 channels in registers, fold rows through LDS and finish with one
// fp32 atomic per channel per workgroup.
//
//   input_norm      u8 [N][H][W][3] -> bf16 [N][H][W][8] ((x/255 - mean_c)/std_c, pad channels 0),
//                   batch chosen by a device cursor (hipGraph replay)
//   input_aug       the same, with the records drawn through a per-epoch permutation and/or a random
//                   crop (zero padding) + horizontal flip, all a pure function of (seed, cursor, sample)
//   input_mix       input_aug, then mixup or CutMix with another sample of the batch (integer blend)
//   bn_finalize     conv-epilogue sums -> scale/shift/mean/rstd, running-stat update
//   bn_apply        y = relu?(x*scale + shift + r), r = 0 | res | res*rscale + rshift
//   bn_bwd_reduce   dz = dy*1[y>0]; per-channel sum(dz), sum(dz*x) (+ dz out for the skip)
//   bn_bwd_finalize -> dgamma, dbeta (into the flat gradient) and dx = a*dz + b*x + c coefficients
//   bn_bwd_apply    dx = a*dz + b*x + c
//   maxpool / avgpool fwd+bwd, softmax cross-entropy (loss, correct, dlogits, dbias), against
//                   one-hot labels or soft targets (label smoothing, the label pair of a mixed sample)
#include "common.h"
#include "bn_fwd.h"
#include "philox.h"

#include <tuple>

using namespace sl;

// Grid cap of the streaming BN apply kernels; SL_BN_APPLY_BLOCKS overrides it for A/B runs.
static int bn_apply_cap() {
  static int cap = -1;
  if (cap < 0) {
    const char* e = getenv("SL_BN_APPLY_BLOCKS");
    cap = e ? atoi(e) : 1024;  // 1024 vs 4096: ResNet-18 +0.6-1.3 % (profiles/r05_sweep)
    if (cap < 1) cap = 1024;
  }
  return cap;
}

static int blocks_for(long items, int cap = 4096) {
  long b = (items + 255) / 256;
  if (b > cap) b = cap;
  return b < 1 ? 1 : (int)b;
}

// ---------------------------------------------------------------------------
// (a*v + b per channel) of a pixel's three u8 values: a = 1/(255 std_c), b = -mean_c/std_c
struct NormCoef {
  float a0, a1, a2, b0, b1, b2;
};

// One pixel's three channels, in pixel units (0..255, fractions allowed) -> 8 bf16 (channels 3-7
// zero).  The one copy of the arithmetic: input_norm, input_aug and input_mix give the same values
// the same bits.  Each channel is one fused multiply-add (v_fma_f32 / v_pk_fma_f32 in all three
// kernels): the contraction of `v * a + b` is asked for here and not left to the build's default,
// so a reference knows what to emulate -- round(v * a + b) once to fp32.  (fmaf() gives the same
// instructions in another register allocation, which would move input_norm_kernel's code.)
__device__ __forceinline__ short8_t norm_pack8(float r, float g, float b, const NormCoef& c) {
#pragma clang fp contract(fast)
  float f[8] = {r * c.a0 + c.b0, g * c.a1 + c.b1, b * c.a2 + c.b2, 0.f, 0.f, 0.f, 0.f, 0.f};
  return pack8(f);
}

__device__ __forceinline__ short8_t norm_pack8(uint8_t r, uint8_t g, uint8_t b, const NormCoef& c) {
  return norm_pack8((float)(int)r, (float)(int)g, (float)(int)b, c);
}

// Batch `cursor % n_batches` of a device-resident u8 shard -> normalised bf16
// (and its labels), so a captured step replays on fresh data with no host work.
__global__ __launch_bounds__(256) void input_norm_kernel(const uint8_t* __restrict__ x, const uint8_t* __restrict__ lab,
                                                         const int* __restrict__ cursor, int n_batches, int batch,
                                                         long img_pixels, uint16_t* __restrict__ y,
                                                         uint8_t* __restrict__ lab_out, NormCoef c) {
  const long b = cursor ? (long)(*cursor % n_batches) : 0;
  const long pixels = (long)batch * img_pixels;
  const uint8_t* src = x + b * pixels * 3;
  for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < pixels; p += (long)gridDim.x * blockDim.x) {
    const uint8_t* s = src + p * 3;
    *reinterpret_cast<short8_t*>(y + p * 8) = norm_pack8(s[0], s[1], s[2], c);
    if (lab_out && p < batch) lab_out[p] = lab[b * batch + p];
  }
}

// Pixels per thread of input_aug_kernel (256 apart, so a wave's accesses stay contiguous).  The
// per-image prologue is ~450 scalar instructions in every wave; at one pixel per thread it bound the
// kernel with both parts on (12.9-13.0 us at B = 1024, 32x32, against 10.7-11.0 us at 2, 4 or 8
// in the same run: profiles/r13_input).
constexpr int AUG_PX = 4;

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

// Input pipeline of a training step: sample j = blockIdx.y takes the record of aug_draw, shifted by
// (oy - pad, ox - pad) with black padding and mirrored when flip.  A thread then does what
// input_norm's does, for up to AUG_PX pixels of the image: three byte loads (none for padding),
// one 16-B store.
__global__ __launch_bounds__(256) void input_aug_kernel(const uint8_t* __restrict__ x, const uint8_t* __restrict__ lab,
                                                        const int* __restrict__ cursor, uint32_t n_records,
                                                        uint32_t batch, int H, int W, int pad, int flags, int half_bits,
                                                        uint32_t k0, uint32_t k1, uint16_t* __restrict__ y,
                                                        uint8_t* __restrict__ lab_out, int* __restrict__ params_out,
                                                        NormCoef c) {
  const uint32_t j = blockIdx.y;
  const uint32_t t = (uint32_t)*cursor;  // a non-negative int32
  const AugDraw d = aug_draw(j, t, n_records, batch, pad, flags, half_bits, k0, k1);
  const uint32_t rec = d.rec;
  const int oy = d.oy, ox = d.ox, flip = d.flip;
  const int p0 = blockIdx.x * (256 * AUG_PX) + threadIdx.x;
  if (p0 == 0) {
    if (params_out) *reinterpret_cast<int4*>(params_out + 4 * j) = make_int4((int)rec, oy, ox, flip);
    if (lab_out) lab_out[j] = lab[rec];
  }
  const int img = H * W;
  const uint8_t* src = x + (long)rec * img * 3;
  uint16_t* dst = y + (long)j * img * 8;
#pragma unroll
  for (int k = 0; k < AUG_PX; ++k) {
    const int p = p0 + k * 256;
    if (p >= img) break;
    const int py = p / W, px = p - py * W;
    const int sy = py + oy - pad, sx = (flip ? W - 1 - px : px) + ox - pad;
    uint8_t v0 = 0, v1 = 0, v2 = 0;  // outside the image: black before normalisation
    if ((unsigned)sy < (unsigned)H && (unsigned)sx < (unsigned)W) {
      const uint8_t* s = src + ((long)sy * W + sx) * 3;
      v0 = s[0];
      v1 = s[1];
      v2 = s[2];
    }
    *reinterpret_cast<short8_t*>(dst + (long)p * 8) = norm_pack8(v0, v1, v2, c);
  }
}

// Entries of one mix table (data/augment.py MIX_L): the index is the top 12 bits of a Philox word.
constexpr int MIX_L = 4096;

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

// input_aug followed by mixup or CutMix (data/augment.py): the batch draws M = Philox(t, 0, 0;
// stream 3) and Nn = Philox(t, 1, 0; stream 3); sample j mixes with sample pj = (j + r) % B of the
// same batch, r = 1 + M.y % (B - 1), taken after its own shuffle / crop / flip.  table is
// int32 [2][MIX_L], row 0 mixup's and row 1 CutMix's, entry M.x >> 20 packing k = round(256 lambda)
// (low half) and c = round(256 sqrt(1 - lambda)) (high half).  Mixup: every channel is
// (k ua + (256 - k) ub) / 256, exact in fp32; CutMix: a (W c + 128 >> 8) x (H c + 128 >> 8) box
// centred at (Nn.x % W, Nn.y % H), clipped, shows the partner.  All of this and both samples'
// aug_draw are uniform in the workgroup: scalar registers.  modes: 1 = mixup, 2 = CutMix, 3 = the
// batch is CutMix when M.z & 1.  mix_out row j: (pj, num, den, mode, x0, y0, x1, y1), num / den the
// weight of the partner's label.
__global__ __launch_bounds__(256) void input_mix_kernel(const uint8_t* __restrict__ x, const uint8_t* __restrict__ lab,
                                                        const int* __restrict__ cursor, uint32_t n_records,
                                                        uint32_t batch, int H, int W, int pad, int flags, int half_bits,
                                                        uint32_t k0, uint32_t k1, const int* __restrict__ table,
                                                        int modes, uint16_t* __restrict__ y,
                                                        uint8_t* __restrict__ lab_out, int* __restrict__ params_out,
                                                        int* __restrict__ mix_out, NormCoef c) {
  const uint32_t j = blockIdx.y;
  const uint32_t t = (uint32_t)*cursor;  // a non-negative int32
  const U4 m = philox4x32_10(t, 0u, 0u, 3u, k0, k1);
  const uint32_t pj = (j + 1u + m.y % (batch - 1u)) % batch;  // batch >= 2 (sl_input_mix)
  const int mode = modes == 3 ? ((m.z & 1u) ? 2 : 1) : modes;
  const uint32_t entry = (uint32_t)table[(mode - 1) * MIX_L + (int)(m.x >> 20)];
  const AugDraw da = aug_draw(j, t, n_records, batch, pad, flags, half_bits, k0, k1);
  const AugDraw db = aug_draw(pj, t, n_records, batch, pad, flags, half_bits, k0, k1);
  int k = 256, x0 = 0, y0 = 0, x1 = 0, y1 = 0, num, den;
  if (mode == 1) {
    k = min((int)(entry & 0xFFFFu), 256);
    num = 256 - k;
    den = 256;
  } else {
    const U4 nn = philox4x32_10(t, 1u, 0u, 3u, k0, k1);
    const int cc = min((int)(entry >> 16), 256);
    const int bw = (W * cc + 128) >> 8, bh = (H * cc + 128) >> 8;
    if (bw > 0 && bh > 0) {
      const int bx = (int)(nn.x % (uint32_t)W) - bw / 2, by = (int)(nn.y % (uint32_t)H) - bh / 2;
      x0 = max(bx, 0);
      x1 = min(bx + bw, W);
      y0 = max(by, 0);
      y1 = min(by + bh, H);
    }
    num = (x1 - x0) * (y1 - y0);
    den = H * W;
  }
  const int p0 = blockIdx.x * (256 * AUG_PX) + threadIdx.x;
  if (p0 == 0) {
    if (params_out) *reinterpret_cast<int4*>(params_out + 4 * j) = make_int4((int)da.rec, da.oy, da.ox, da.flip);
    if (mix_out) {
      *reinterpret_cast<int4*>(mix_out + 8 * j) = make_int4((int)pj, num, den, mode);
      *reinterpret_cast<int4*>(mix_out + 8 * j + 4) = make_int4(x0, y0, x1, y1);
    }
    if (lab_out) lab_out[j] = lab[da.rec];
  }
  const int img = H * W;
  const uint8_t* srca = x + (long)da.rec * img * 3;
  const uint8_t* srcb = x + (long)db.rec * img * 3;
  uint16_t* dst = y + (long)j * img * 8;
#pragma unroll
  for (int q = 0; q < AUG_PX; ++q) {
    const int p = p0 + q * 256;
    if (p >= img) break;
    const int py = p / W, px = p - py * W;
    float f0, f1, f2;
    if (mode == 1) {
      const uint32_t ua = aug_pixel(srca, da, py, px, H, W, pad), ub = aug_pixel(srcb, db, py, px, H, W, pad);
      const int kb = 256 - k;
      // n = k ua + (256 - k) ub <= 65280: n / 256 is exact in fp32
      f0 = (float)(k * (int)(ua & 255u) + kb * (int)(ub & 255u)) * (1.f / 256.f);
      f1 = (float)(k * (int)((ua >> 8) & 255u) + kb * (int)((ub >> 8) & 255u)) * (1.f / 256.f);
      f2 = (float)(k * (int)(ua >> 16) + kb * (int)(ub >> 16)) * (1.f / 256.f);
    } else {
      const bool in = px >= x0 && px < x1 && py >= y0 && py < y1;  // the partner's pixel at (y, x)
      const uint32_t u = aug_pixel(in ? srcb : srca, in ? db : da, py, px, H, W, pad);
      f0 = (float)(u & 255u);
      f1 = (float)((u >> 8) & 255u);
      f2 = (float)(u >> 16);
    }
    *reinterpret_cast<short8_t*>(dst + (long)p * 8) = norm_pack8(f0, f1, f2, c);
  }
}

__global__ void cursor_bump_kernel(int* cursor) { *cursor += 1; }

// coef layout [4][C]: scale, shift, mean, rstd
__global__ void bn_finalize_kernel(const float* __restrict__ stats, const float* __restrict__ gamma,
                                   const float* __restrict__ beta, float* __restrict__ coef,
                                   float* __restrict__ run_mean, float* __restrict__ run_var, int C, float count,
                                   float eps, float momentum) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float mean = stats[c] / count;
  const float var = fmaxf(stats[C + c] / count - mean * mean, 0.f);
  const float rstd = rsqrtf(var + eps);
  const float sc = gamma[c] * rstd;
  coef[c] = sc;
  coef[C + c] = beta[c] - mean * sc;
  coef[2 * C + c] = mean;
  coef[3 * C + c] = rstd;
  if (run_mean) {
    run_mean[c] = (1.f - momentum) * run_mean[c] + momentum * mean;
    run_var[c] = (1.f - momentum) * run_var[c] + momentum * var * (count / fmaxf(count - 1.f, 1.f));
  }
}

// mode: 0 = none, 1 = identity residual, 2 = residual through its own BN (rcoef)
__global__ __launch_bounds__(256) void bn_apply_kernel(const uint16_t* __restrict__ x, const float* __restrict__ coef,
                                                       const uint16_t* __restrict__ res,
                                                       const float* __restrict__ rcoef, uint16_t* __restrict__ y,
                                                       long rows, int C, int relu, int mode) {
  const int cpr = C >> 3;
  const long total = rows * cpr;
  for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (long)gridDim.x * blockDim.x) {
    const int c0 = (int)(q % cpr) * 8;
    float f[8];
    unpack8(ld8(x + q * 8), f);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = f[j] * coef[c0 + j] + coef[C + c0 + j];
    if (mode) {
      float r[8];
      unpack8(ld8(res + q * 8), r);
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] += mode == 2 ? r[j] * rcoef[c0 + j] + rcoef[C + c0 + j] : r[j];
    }
    if (relu) {
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] = fmaxf(f[j], 0.f);
    }
    *reinterpret_cast<short8_t*>(y + q * 8) = pack8(f);
  }
}

// Per-channel sums of dz = dy*1[y>0] and dz*x.  Thread layout: TPR = C/8
// threads per row, 256/TPR rows per pass; partials folded through LDS, then
// across workgroups through an rsum buffer (result at rsum_result(sums, 2C)).
// ReLU mask of y = relu(x*scale + shift) re-derived from the BN input x and the
// forward coefficients (coef rows 0/1 = scale/shift, written by bn_publish), so
// the backward of a non-residual BN+ReLU never reads y: 2 streams instead of 3.
__device__ __forceinline__ void relu_mask_coef8(const float* __restrict__ coef, int C, int c0, float (&sc)[8],
                                                float (&sh)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    sc[j] = coef[c0 + j];
    sh[j] = coef[C + c0 + j];
  }
}

__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const uint16_t* __restrict__ dy,
                                                            const uint16_t* __restrict__ y,
                                                            const uint16_t* __restrict__ x,
                                                            const float* __restrict__ mcoef,
                                                            const uint8_t* __restrict__ ymask,
                                                            uint16_t* __restrict__ dz_out, float* __restrict__ sums,
                                                            const uint16_t* __restrict__ x2,
                                                            float* __restrict__ sums2, long rows, int C) {
  // x2/sums2: a second BN fed by the same dz (the downsample shortcut's), whose
  // sums ride along so dz is not read back: sums2 = (sum dz, sum dz*x2).
  __shared__ float part[256][25];
  const int tpr = C >> 3, rpp = 256 / tpr;
  const int tid = threadIdx.x;
  const int cg = tid % tpr, rsub = tid / tpr;
  float s[8] = {0.f}, d[8] = {0.f}, d2[8] = {0.f};
  float msc[8], msh[8];
  if (mcoef) relu_mask_coef8(mcoef, C, cg * 8, msc, msh);
  if (rsub < rpp) {
    for (long r = (long)blockIdx.x * rpp + rsub; r < rows; r += (long)gridDim.x * rpp) {
      const long off = r * C + cg * 8;
      float g[8], xv[8];
      unpack8(ld8(dy + off), g);
      unpack8(ld8(x + off), xv);
      if (y) {
        float yv[8];
        unpack8(ld8(y + off), yv);
#pragma unroll
        for (int j = 0; j < 8; ++j) g[j] = yv[j] > 0.f ? g[j] : 0.f;
      } else if (ymask) {
        const unsigned m = ymask[off >> 3];
#pragma unroll
        for (int j = 0; j < 8; ++j) g[j] = (m >> j) & 1u ? g[j] : 0.f;
      } else if (mcoef) {
#pragma unroll
        for (int j = 0; j < 8; ++j) g[j] = xv[j] * msc[j] + msh[j] > 0.f ? g[j] : 0.f;
      }
      if (dz_out) *reinterpret_cast<short8_t*>(dz_out + off) = pack8(g);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        s[j] += g[j];
        d[j] += g[j] * xv[j];
      }
      if (x2) {
        float x2v[8];
        unpack8(ld8(x2 + off), x2v);
#pragma unroll
        for (int j = 0; j < 8; ++j) d2[j] += g[j] * x2v[j];
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    part[tid][j] = s[j];
    part[tid][8 + j] = d[j];
    part[tid][16 + j] = d2[j];
  }
  __syncthreads();
  // fold the rpp row-groups: thread t < 2*C (4*C with x2) handles one (quantity, channel);
  // quantities 0/1 -> sums, 2/3 -> sums2 (2 is sum dz again, 3 is sum dz*x2)
  float* rep = rsum_replica(sums, 2 * C);
  float* rep2 = x2 ? rsum_replica(sums2, 2 * C) : nullptr;
  const int nq = x2 ? 4 * C : 2 * C;
  for (int t = tid; t < nq; t += 256) {
    const int qsel = t / C, c = t - qsel * C;
    const int g = c >> 3, j = c & 7;
    const int col = (qsel == 2 ? 0 : qsel == 3 ? 16 : qsel * 8) + j;
    float acc = 0.f;
    for (int r = 0; r < rpp; ++r) acc += part[r * tpr + g][col];
    if (qsel < 2) rsum_add(rep, qsel * C + c, acc);
    else rsum_add(rep2, (qsel - 2) * C + c, acc);
  }
}

// dcoef layout [3][C]: a, b, c with dx = a*dz + b*x + c.  grad_gamma/beta += (flat gradient).
__global__ void bn_bwd_finalize_kernel(const float* __restrict__ sums, const float* __restrict__ coef,
                                       float* __restrict__ dcoef, float* __restrict__ grad_gamma,
                                       float* __restrict__ grad_beta, int C, float count) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float s0 = sums[c], s1 = sums[C + c];
  const float sc = coef[c], mean = coef[2 * C + c], rstd = coef[3 * C + c];
  const float sdxh = rstd * (s1 - mean * s0);  // sum(dz * xhat)
  const float b = -sc * rstd * sdxh / count;
  dcoef[c] = sc;
  dcoef[C + c] = b;
  dcoef[2 * C + c] = -sc * s0 / count - b * mean;
  if (grad_gamma) grad_gamma[c] += sdxh;
  if (grad_beta) grad_beta[c] += s0;
}

// dx = a*dz + b*x + c; dz = dy*1[y>0] recomputed (or read directly when y == null)
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const uint16_t* __restrict__ dy,
                                                           const uint16_t* __restrict__ y,
                                                           const uint16_t* __restrict__ x,
                                                           const float* __restrict__ dcoef,
                                                           uint16_t* __restrict__ dx, long rows, int C) {
  const int cpr = C >> 3;
  const long total = rows * cpr;
  for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (long)gridDim.x * blockDim.x) {
    const int c0 = (int)(q % cpr) * 8;
    float g[8], xv[8];
    unpack8(ld8(dy + q * 8), g);
    if (y) {
      float yv[8];
      unpack8(ld8(y + q * 8), yv);
#pragma unroll
      for (int j = 0; j < 8; ++j) g[j] = yv[j] > 0.f ? g[j] : 0.f;
    }
    unpack8(ld8(x + q * 8), xv);
#pragma unroll
    for (int j = 0; j < 8; ++j) g[j] = dcoef[c0 + j] * g[j] + dcoef[C + c0 + j] * xv[j] + dcoef[2 * C + c0 + j];
    *reinterpret_cast<short8_t*>(dx + q * 8) = pack8(g);
  }
}

// ---------------------------------------------------------------------------
// Fused forms used by the engine: the per-channel finalize folds into the
// element-wise pass (each thread owns 8 fixed channels, so it derives their
// coefficients once from the raw sums), and workgroup 0 publishes the
// coefficients / running statistics / dgamma, dbeta.  Two fewer launches per
// BatchNorm per direction (a 1-WG kernel costs ~4.5 us of serialised time).
// BnStats, bn_coef8, bn_publish: bn_fwd.h

// y = relu?(bn(x) + r), r = 0 | res | bn_r(res) | relu(bn_r(res)) (modes 0-3); grid stride is a
// multiple of C/8.
__global__ __launch_bounds__(256) void bn_apply_stats_kernel(const uint16_t* __restrict__ x, BnStats b,
                                                             const uint16_t* __restrict__ res, BnStats rb,
                                                             uint16_t* __restrict__ y, uint8_t* __restrict__ mask_out,
                                                             long rows, int C, int relu, int mode, float count,
                                                             float eps, float momentum) {
  const int cpr = C >> 3;
  const long total = rows * cpr;
  const long t0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int c0 = (int)(t0 % cpr) * 8;
  float sc[8], sh[8], rsc[8], rsh[8];
  bn_coef8(b, C, c0, count, eps, sc, sh);
  if (mode >= 2) bn_coef8(rb, C, c0, count, eps, rsc, rsh);
  for (long q = t0; q < total; q += (long)gridDim.x * blockDim.x) {
    float f[8];
    unpack8(ld8(x + q * 8), f);
#pragma unroll
    for (int j = 0; j < 8; ++j) f[j] = f[j] * sc[j] + sh[j];
    if (mode == 3) {
      // residual = relu(bn_r(res)) rounded to bf16: the stored tensor it replaces (BN-on-load)
      float r[8];
      const uint4 rv = bn_relu_chunk(*reinterpret_cast<const uint4*>(res + q * 8), rsc, rsh);
      unpack8(__builtin_bit_cast(short8_t, rv), r);
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] += r[j];
    } else if (mode) {
      float r[8];
      unpack8(ld8(res + q * 8), r);
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] += mode == 2 ? r[j] * rsc[j] + rsh[j] : r[j];
    }
    if (relu) {
#pragma unroll
      for (int j = 0; j < 8; ++j) f[j] = fmaxf(f[j], 0.f);
    }
    const short8_t yv = pack8(f);
    *reinterpret_cast<short8_t*>(y + q * 8) = yv;
    if (mask_out) {  // bit j = (stored bf16 y > 0), 1 B per 8 channels
      unsigned m = 0;
#pragma unroll
      for (int j = 0; j < 8; ++j) m |= (unsigned)(yv[j] > 0) << j;
      mask_out[q] = (uint8_t)m;
    }
  }
  if (blockIdx.x == 0) {
    bn_publish(b, C, count, eps, momentum);
    if (mode == 2) bn_publish(rb, C, count, eps, momentum);  // mode 3: published by the BN-on-load conv
  }
}

// dx = a*dz + b*x + c with (a, b, c) derived per channel from the reduce
// kernel's sums and the forward coefficients; workgroup 0 adds dgamma, dbeta.
__global__ __launch_bounds__(256) void bn_bwd_apply_sums_kernel(const uint16_t* __restrict__ dy,
                                                                const uint16_t* __restrict__ y,
                                                                const uint16_t* __restrict__ x,
                                                                const float* __restrict__ mcoef,
                                                                const float* __restrict__ sums,
                                                                const float* __restrict__ coef,
                                                                float* __restrict__ grad_gamma,
                                                                float* __restrict__ grad_beta,
                                                                uint16_t* __restrict__ dx, long rows, int C,
                                                                float count) {
  const int cpr = C >> 3;
  const long total = rows * cpr;
  const long t0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int c0 = (int)(t0 % cpr) * 8;
  float ca[8], cb[8], cc[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = c0 + j;
    const float s0 = sums[c], s1 = sums[C + c];
    const float sc = coef[c], mean = coef[2 * C + c], rstd = coef[3 * C + c];
    const float sdxh = rstd * (s1 - mean * s0);
    ca[j] = sc;
    cb[j] = -sc * rstd * sdxh / count;
    cc[j] = -sc * s0 / count - cb[j] * mean;
  }
  float msc[8], msh[8];
  if (mcoef) relu_mask_coef8(mcoef, C, c0, msc, msh);
  for (long q = t0; q < total; q += (long)gridDim.x * blockDim.x) {
    float g[8], xv[8];
    unpack8(ld8(dy + q * 8), g);
    unpack8(ld8(x + q * 8), xv);
    if (y) {
      float yv[8];
      unpack8(ld8(y + q * 8), yv);
#pragma unroll
      for (int j = 0; j < 8; ++j) g[j] = yv[j] > 0.f ? g[j] : 0.f;
    } else if (mcoef) {
#pragma unroll
      for (int j = 0; j < 8; ++j) g[j] = xv[j] * msc[j] + msh[j] > 0.f ? g[j] : 0.f;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) g[j] = ca[j] * g[j] + cb[j] * xv[j] + cc[j];
    *reinterpret_cast<short8_t*>(dx + q * 8) = pack8(g);
  }
  if (blockIdx.x == 0) {
    for (int c = threadIdx.x; c < C; c += blockDim.x) {
      const float s0 = sums[c], s1 = sums[C + c];
      const float mean = coef[2 * C + c], rstd = coef[3 * C + c];
      if (grad_gamma) grad_gamma[c] += rstd * (s1 - mean * s0);
      if (grad_beta) grad_beta[c] += s0;
    }
  }
}

// One BN of a pair fed by the same dz (bn_bwd_apply_dual_kernel).
struct BnBwdSide {
  const uint16_t* x;
  const float* sums;
  const float* coef;
  float* grad_gamma;
  float* grad_beta;
  uint16_t* dx;
};

__device__ __forceinline__ void bn_bwd_abc8(const BnBwdSide& b, int C, int c0, float count, float (&ca)[8],
                                            float (&cb)[8], float (&cc)[8]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = c0 + j;
    const float s0 = b.sums[c], s1 = b.sums[C + c];
    const float sc = b.coef[c], mean = b.coef[2 * C + c], rstd = b.coef[3 * C + c];
    const float sdxh = rstd * (s1 - mean * s0);
    ca[j] = sc;
    cb[j] = -sc * rstd * sdxh / count;
    cc[j] = -sc * s0 / count - cb[j] * mean;
  }
}

// bn_bwd_apply_sums for the two BNs of a downsample block (bn2 on c2, the
// shortcut's BN on cs), which share dz: dz is read once for both dx outputs.
__global__ __launch_bounds__(256) void bn_bwd_apply_dual_kernel(const uint16_t* __restrict__ dz, BnBwdSide a,
                                                                BnBwdSide b, long rows, int C, float count) {
  const int cpr = C >> 3;
  const long total = rows * cpr;
  const long t0 = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int c0 = (int)(t0 % cpr) * 8;
  float aa[8], ab[8], ac[8], ba[8], bb[8], bc[8];
  bn_bwd_abc8(a, C, c0, count, aa, ab, ac);
  bn_bwd_abc8(b, C, c0, count, ba, bb, bc);
  for (long q = t0; q < total; q += (long)gridDim.x * blockDim.x) {
    float g[8], xa[8], xb[8], oa[8], ob[8];
    unpack8(ld8(dz + q * 8), g);
    unpack8(ld8(a.x + q * 8), xa);
    unpack8(ld8(b.x + q * 8), xb);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      oa[j] = aa[j] * g[j] + ab[j] * xa[j] + ac[j];
      ob[j] = ba[j] * g[j] + bb[j] * xb[j] + bc[j];
    }
    *reinterpret_cast<short8_t*>(a.dx + q * 8) = pack8(oa);
    *reinterpret_cast<short8_t*>(b.dx + q * 8) = pack8(ob);
  }
  if (blockIdx.x == 0) {
    for (int c = threadIdx.x; c < 2 * C; c += blockDim.x) {
      const BnBwdSide& s = c < C ? a : b;
      const int k = c < C ? c : c - C;
      const float s0 = s.sums[k], s1 = s.sums[C + k];
      const float mean = s.coef[2 * C + k], rstd = s.coef[3 * C + k];
      if (s.grad_gamma) s.grad_gamma[k] += rstd * (s1 - mean * s0);
      if (s.grad_beta) s.grad_beta[k] += s0;
    }
  }
}

// ---------------------------------------------------------------------------
// Max pool (KxK, stride s, pad p) with a per-output argmax tap (u8) for backward.
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const uint16_t* __restrict__ x, uint16_t* __restrict__ y,
                                                          uint8_t* __restrict__ arg, int N, int H, int W, int C,
                                                          int OH, int OW, int K, int s, int p) {
  const int cpr = C >> 3;
  const long total = (long)N * OH * OW * cpr;
  for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (long)gridDim.x * blockDim.x) {
    const int c0 = (int)(q % cpr) * 8;
    const long pix = q / cpr;
    const int ow = (int)(pix % OW);
    const int oh = (int)((pix / OW) % OH);
    const int n = (int)(pix / ((long)OW * OH));
    float best[8];
    uint8_t bi[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { best[j] = -INFINITY; bi[j] = 0; }
    for (int kh = 0; kh < K; ++kh)
      for (int kw = 0; kw < K; ++kw) {
        const int ih = oh * s - p + kh, iw = ow * s - p + kw;
        if ((unsigned)ih >= (unsigned)H || (unsigned)iw >= (unsigned)W) continue;
        float v[8];
        unpack8(ld8(x + (((long)n * H + ih) * W + iw) * C + c0), v);
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (v[j] > best[j]) { best[j] = v[j]; bi[j] = (uint8_t)(kh * K + kw); }
      }
    *reinterpret_cast<short8_t*>(y + pix * C + c0) = pack8(best);
#pragma unroll
    for (int j = 0; j < 8; ++j) arg[pix * C + c0 + j] = bi[j];
  }
}

// Gather form: each input pixel sums the gradients of the windows whose argmax it is.
__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const uint16_t* __restrict__ dy,
                                                          const uint8_t* __restrict__ arg, uint16_t* __restrict__ dx,
                                                          int N, int H, int W, int C, int OH, int OW, int K, int s,
                                                          int p) {
  const int cpr = C >> 3;
  const long total = (long)N * H * W * cpr;
  for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (long)gridDim.x * blockDim.x) {
    const int c0 = (int)(q % cpr) * 8;
    const long pix = q / cpr;
    const int w = (int)(pix % W);
    const int h = (int)((pix / W) % H);
    const int n = (int)(pix / ((long)W * H));
    float acc[8] = {0.f};
    for (int kh = 0; kh < K; ++kh) {
      const int th = h + p - kh;
      if (th < 0 || th % s) continue;
      const int oh = th / s;
      if (oh >= OH) continue;
      for (int kw = 0; kw < K; ++kw) {
        const int tw = w + p - kw;
        if (tw < 0 || tw % s) continue;
        const int ow = tw / s;
        if (ow >= OW) continue;
        const long o = (((long)n * OH + oh) * OW + ow) * C + c0;
        float g[8];
        unpack8(ld8(dy + o), g);
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (arg[o + j] == (uint8_t)(kh * K + kw)) acc[j] += g[j];
      }
    }
    *reinterpret_cast<short8_t*>(dx + pix * C + c0) = pack8(acc);
  }
}

// Global average pool [N][HW][C] -> [N][C]; backward broadcasts dy/HW.
__global__ __launch_bounds__(256) void avgpool_fwd_kernel(const uint16_t* __restrict__ x, uint16_t* __restrict__ y,
                                                          int N, int HW, int C) {
  const int cpr = C >> 3;
  const long total = (long)N * cpr;
  for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (long)gridDim.x * blockDim.x) {
    const int n = (int)(q / cpr), c0 = (int)(q % cpr) * 8;
    float acc[8] = {0.f};
    for (int i = 0; i < HW; ++i) {
      float v[8];
      unpack8(ld8(x + ((long)n * HW + i) * C + c0), v);
#pragma unroll
      for (int j = 0; j < 8; ++j) acc[j] += v[j];
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] *= 1.f / HW;
    *reinterpret_cast<short8_t*>(y + (long)n * C + c0) = pack8(acc);
  }
}

__global__ __launch_bounds__(256) void avgpool_bwd_kernel(const uint16_t* __restrict__ dy, uint16_t* __restrict__ dx,
                                                          int N, int HW, int C) {
  const int cpr = C >> 3;
  const long total = (long)N * HW * cpr;
  for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (long)gridDim.x * blockDim.x) {
    const long pix = q / cpr;
    const int c0 = (int)(q % cpr) * 8;
    const int n = (int)(pix / HW);
    float g[8];
    unpack8(ld8(dy + (long)n * C + c0), g);
#pragma unroll
    for (int j = 0; j < 8; ++j) g[j] *= 1.f / HW;
    *reinterpret_cast<short8_t*>(dx + pix * C + c0) = pack8(g);
  }
}

// ---------------------------------------------------------------------------
#if SL_DETERMINISTIC
__device__ unsigned long long g_dbias_fix[32];  // fixed-point (hi, lo) bias-gradient pairs (zero between launches)
__device__ unsigned g_dbias_ticket;
#endif
// Softmax cross-entropy over fp32 logits [N][ncls] (ncls <= 16); one row per
// 16-lane group.  dlogits (bf16, [N][ldd], zero beyond ncls) are scaled by
// grad_scale; the bias gradient (sum over rows of dlogits) is folded per
// workgroup and added atomically.
// SOFT: the target of row i is q_c = (1 - eps)(wa [c = la] + wb [c = lb]) + eps / ncls instead of
// one-hot la = lab[i]: row i of mix (int32 [N][8], input_mix's mix_out; null = smoothing alone) names
// the partner pj and its weight wb = num / den, lb = lab[pj], wa = 1 - wb.  loss = logsumexp(z) -
// sum_c q_c z_c, dz = (softmax(z) - q) grad_scale; correct stays argmax against la.
// The soft form's two extra arguments, (const int* mix, float eps), are a trailing pack that is
// empty for the one-hot form, whose argument list and code are then exactly what they were.
template <bool SOFT, class... Soft>
__global__ __launch_bounds__(256) void softmax_ce_kernel(const float* __restrict__ z, const uint8_t* __restrict__ lab,
                                                         float* __restrict__ loss, float* __restrict__ correct,
                                                         uint16_t* __restrict__ dz, int ldd, float* __restrict__ dbias,
                                                         int N, int ncls, float grad_scale, Soft... soft) {
  __shared__ float bsum[16][16];
  const int tid = threadIdx.x, c = tid & 15, grp = tid >> 4;
  const int row = blockIdx.x * 16 + grp;
  float dv = 0.f;
  if (row < N) {
    const float v = c < ncls ? z[(long)row * ncls + c] : -INFINITY;
    float mx = v;
    mx = fmaxf(mx, __shfl_xor(mx, 1));
    mx = fmaxf(mx, __shfl_xor(mx, 2));
    mx = fmaxf(mx, __shfl_xor(mx, 4));
    mx = fmaxf(mx, __shfl_xor(mx, 8));
    const float e = c < ncls ? __expf(v - mx) : 0.f;
    float s = e;
    s += __shfl_xor(s, 1);
    s += __shfl_xor(s, 2);
    s += __shfl_xor(s, 4);
    s += __shfl_xor(s, 8);
    int l = lab[row];
    l = l < ncls ? l : 0;
    float zl, q = 0.f;
    if constexpr (SOFT) {
      const auto [mix, eps] = std::tuple<const int*, float>(soft...);
      int lb = l;
      float wb = 0.f;
      if (mix) {
        const int pj = mix[8 * row];
        lb = (unsigned)pj < (unsigned)N ? lab[pj] : l;
        lb = lb < ncls ? lb : 0;
        wb = (float)mix[8 * row + 1] / (float)mix[8 * row + 2];
      }
      // lanes beyond ncls hold -inf: they take no part in sum_c q_c z_c
      q = c < ncls ? (1.f - eps) * ((c == l ? 1.f - wb : 0.f) + (c == lb ? wb : 0.f)) + eps / (float)ncls : 0.f;
      zl = c < ncls ? q * v : 0.f;
      zl += __shfl_xor(zl, 1);
      zl += __shfl_xor(zl, 2);
      zl += __shfl_xor(zl, 4);
      zl += __shfl_xor(zl, 8);
    } else {
      zl = __shfl(v, (tid & 63 & ~15) | l);
    }
    int idx = v == mx ? c : 16;
    idx = min(idx, __shfl_xor(idx, 1));
    idx = min(idx, __shfl_xor(idx, 2));
    idx = min(idx, __shfl_xor(idx, 4));
    idx = min(idx, __shfl_xor(idx, 8));
    if (c == 0) {
      if (loss) loss[row] = mx + __logf(s) - zl;
      if (correct) correct[row] = idx == l ? 1.f : 0.f;
    }
    if constexpr (SOFT) dv = c < ncls ? (e / s - q) * grad_scale : 0.f;
    else dv = c < ncls ? (e / s - (c == l ? 1.f : 0.f)) * grad_scale : 0.f;
    if (c < ldd) dz[(long)row * ldd + c] = f2bf(dv);
  }
  bsum[grp][c] = dv;
  __syncthreads();
  if (dbias && tid < ncls) {
    float acc = 0.f;
    for (int g2 = 0; g2 < 16; ++g2) acc += bsum[g2][tid];
#if SL_DETERMINISTIC
    fix_add(&g_dbias_fix[2 * tid], acc);
#else
    atomicAdd(dbias + tid, acc);
#endif
  }
#if SL_DETERMINISTIC
  // the last workgroup to finish adds the fixed-point total into dbias and resets the
  // accumulator (all in wave 0: the fence covers every lane that added)
  if (dbias) {
    __shared__ int last;
    if (tid == 0) {
      __threadfence();
      last = atomicAdd(&g_dbias_ticket, 1u) == gridDim.x - 1;
    }
    __syncthreads();
    if (last && tid < ncls) {
      __threadfence();
      unsigned long long v[2];
      v[0] = atomicExch(&g_dbias_fix[2 * tid], 0ull);
      v[1] = atomicExch(&g_dbias_fix[2 * tid + 1], 0ull);
      dbias[tid] += (float)fix_value(v);
    }
    if (last && tid == 0) atomicExch(&g_dbias_ticket, 0u);
  }
#endif
}

// ---------------------------------------------------------------------------
// Softmax cross-entropy over 17..256 classes: the narrow kernel's formulas with one row on a whole
// wave.  Lane c owns the four adjacent classes 4c .. 4c + 3, so 64 lanes cover 256 classes; the
// lane's logits are one 16-B load where every row starts on a 16-B boundary (VEC: ncls % 4 == 0)
// and four guarded dword loads otherwise; its four dz values leave as one 8-B store (ldd is a power
// of two >= 32, so lanes 4c < ldd cover exactly columns [0, ldd) and columns [ncls, ldd) get
// zeros).  Maximum, sum, first-maximum index and sum_c q_c z_c are 64-lane butterflies, whose
// result is the same bits in every lane.  A wave takes rows_per_wave consecutive rows and keeps its
// four bias-gradient partial sums in registers.
//
// Bias gradient, with no float atomic and no SL_DETERMINISTIC branch: the four waves of a workgroup
// are added through LDS in wave order, the workgroup stores one partial row ws[blockIdx][ldd], and
// softmax_ce_wide_fold_kernel (a second, one-workgroup launch) adds the partial rows in workgroup
// order into dbias.  Grid and order depend on N alone: the same bits from call to call, in both
// builds.
constexpr int CEW_WAVES = 4;

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v = fmaxf(v, __shfl_xor(v, m));
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
  return v;
}
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v = min(v, __shfl_xor(v, m));
  return v;
}

template <bool SOFT, bool VEC>
__global__ __launch_bounds__(256) void softmax_ce_wide_kernel(const float* __restrict__ z,
                                                              const uint8_t* __restrict__ lab,
                                                              float* __restrict__ loss, float* __restrict__ correct,
                                                              uint16_t* __restrict__ dz, int ldd,
                                                              float* __restrict__ ws, int N, int ncls,
                                                              float grad_scale, const int* __restrict__ mix,
                                                              float eps, int rows_per_wave) {
  __shared__ float bsum[CEW_WAVES][256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c0 = 4 * lane;
  const int row0 = (blockIdx.x * CEW_WAVES + wave) * rows_per_wave;
  float bacc[4] = {0.f, 0.f, 0.f, 0.f};
  for (int i = 0; i < rows_per_wave; ++i) {
    const int row = row0 + i;
    if (row >= N) break;  // (the same for all 64 lanes)
    const float* zr = z + (long)row * ncls;
    float v[4];
    if constexpr (VEC) {
      // ncls % 4 == 0: a lane's four classes are all inside the row or all outside it
      if (c0 < ncls) {
        const float4 t = *reinterpret_cast<const float4*>(zr + c0);
        v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
      } else {
        v[0] = v[1] = v[2] = v[3] = -INFINITY;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = c0 + j < ncls ? zr[c0 + j] : -INFINITY;
    }
    const float mx = wave_max(fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])));
    float e[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) e[j] = c0 + j < ncls ? __expf(v[j] - mx) : 0.f;
    const float s = wave_sum((e[0] + e[1]) + (e[2] + e[3]));
    int l = lab[row];
    l = l < ncls ? l : 0;
    float q[4] = {0.f, 0.f, 0.f, 0.f};
    float zl;
    if constexpr (SOFT) {
      int lb = l;
      float wb = 0.f;
      if (mix) {
        const int pj = mix[8 * row];
        lb = (unsigned)pj < (unsigned)N ? lab[pj] : l;
        lb = lb < ncls ? lb : 0;
        wb = (float)mix[8 * row + 1] / (float)mix[8 * row + 2];
      }
      float t = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = c0 + j;
        // classes beyond ncls hold -inf: they take no part in sum_c q_c z_c
        q[j] = c < ncls ? (1.f - eps) * ((c == l ? 1.f - wb : 0.f) + (c == lb ? wb : 0.f)) + eps / (float)ncls : 0.f;
        t += c < ncls ? q[j] * v[j] : 0.f;
      }
      zl = wave_sum(t);
    } else {
      const int j = l & 3;
      zl = __shfl(j == 0 ? v[0] : j == 1 ? v[1] : j == 2 ? v[2] : v[3], l >> 2);
#pragma unroll
      for (int k = 0; k < 4; ++k) q[k] = c0 + k == l ? 1.f : 0.f;
    }
    // the lowest index among the maxima (classes beyond ncls hold -inf but never win: 4 * 64 = 256)
    int idx = 256;
#pragma unroll
    for (int j = 3; j >= 0; --j) idx = (c0 + j < ncls && v[j] == mx) ? c0 + j : idx;
    idx = wave_min(idx);
    if (lane == 0) {
      if (loss) loss[row] = mx + __logf(s) - zl;
      if (correct) correct[row] = idx == l ? 1.f : 0.f;
    }
    float dv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      dv[j] = c0 + j < ncls ? (e[j] / s - q[j]) * grad_scale : 0.f;
      bacc[j] += dv[j];
    }
    if (c0 < ldd) *reinterpret_cast<uint2*>(dz + (long)row * ldd + c0) = make_uint2(pack2(dv[0], dv[1]), pack2(dv[2], dv[3]));
  }
  if (!ws) return;  // (a kernel argument: the whole workgroup leaves)
#pragma unroll
  for (int j = 0; j < 4; ++j) bsum[wave][c0 + j] = bacc[j];
  __syncthreads();
  if (tid < ldd) {
    float acc = bsum[0][tid];
#pragma unroll
    for (int w = 1; w < CEW_WAVES; ++w) acc += bsum[w][tid];
    ws[(long)blockIdx.x * ldd + tid] = acc;
  }
}

// dbias[c] += ((ws[0][c] + ws[1][c]) + ...) + ws[parts - 1][c]: one workgroup, workgroup order
__global__ __launch_bounds__(256) void softmax_ce_wide_fold_kernel(const float* __restrict__ ws, int parts, int ldd,
                                                                   int ncls, float* __restrict__ dbias) {
  const int c = threadIdx.x;
  if (c >= ncls) return;
  float acc = 0.f;
  int g = 0;
  // eight loads in flight at a time, added in workgroup order
  for (; g + 8 <= parts; g += 8) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = ws[(long)(g + j) * ldd + c];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc += v[j];
  }
  for (; g < parts; ++g) acc += ws[(long)g * ldd + c];
  dbias[c] += acc;
}

// Rows per workgroup of softmax_ce_wide_kernel (a multiple of its four waves; 16 as in the narrow
// kernel); SL_CE_WIDE_ROWS overrides it for A/B runs (profiles/r18_classes).
static int ce_wide_rows_per_wave() {
  static int rows = -1;
  if (rows < 0) {
    const char* e = getenv("SL_CE_WIDE_ROWS");
    const int per_wg = e ? atoi(e) : 16;
    rows = per_wg >= CEW_WAVES && per_wg <= 256 && per_wg % CEW_WAVES == 0 ? per_wg / CEW_WAVES : 16 / CEW_WAVES;
  }
  return rows;
}

static long ce_wide_parts(int N) {
  const int per_wg = CEW_WAVES * ce_wide_rows_per_wave();
  return ((long)N + per_wg - 1) / per_wg;
}

// ---------------------------------------------------------------------------
static NormCoef norm_coef(float m0, float m1, float m2, float s0, float s1, float s2) {
  return NormCoef{1.f / (255.f * s0), 1.f / (255.f * s1), 1.f / (255.f * s2), -m0 / s0, -m1 / s1, -m2 / s2};
}

extern "C" {

long sl_rsum_floats(int n) { return rsum_floats(n); }
long sl_rsum_result_offset(int n) { return (long)SL_REP * n; }
int sl_deterministic() { return SL_DETERMINISTIC; }

int sl_input_norm(const uint8_t* x, const uint8_t* lab, const int* cursor, int n_batches, int batch,
                  long img_pixels, uint16_t* y, uint8_t* lab_out, float m0, float m1, float m2, float s0, float s1,
                  float s2, hipStream_t stream) {
  if (n_batches < 1 || batch < 1) return -1;
  hipLaunchKernelGGL(input_norm_kernel, dim3(blocks_for((long)batch * img_pixels)), dim3(256), 0, stream, x, lab,
                     cursor, n_batches, batch, img_pixels, y, lab_out, norm_coef(m0, m1, m2, s0, s1, s2));
  SL_CHECK_LAUNCH();
  return 0;
}

// flags: 1 = epoch shuffle, 2 = random crop (zero padding `pad`) + horizontal flip.  The grid is
// (pixel tiles, batch): a function of (batch, H, W) alone, so a captured graph replays it.
int sl_input_aug(const uint8_t* x, const uint8_t* lab, const int* cursor, int n_records, int batch, int H, int W,
                 int pad, int flags, unsigned long long seed, uint16_t* y, uint8_t* lab_out, int* params_out, float m0,
                 float m1, float m2, float s0, float s1, float s2, hipStream_t stream) {
  if (!x || !cursor || !y || (lab_out && !lab)) return -2;
  if (batch < 1 || batch > 65535 || n_records < batch || H < 1 || W < 1 || (long)H * W > (1L << 30)) return -1;
  if (pad < 0 || pad >= H || pad >= W || (flags & ~3)) return -1;
  // the Feistel network's half width: an even number of bits that holds n_records - 1
  int bits = 0;
  while (bits < 32 && ((unsigned long long)(n_records - 1) >> bits)) ++bits;
  if (bits < 2) bits = 2;
  const int half_bits = (bits + 1) / 2;
  hipLaunchKernelGGL(input_aug_kernel, dim3((H * W + 256 * AUG_PX - 1) / (256 * AUG_PX), batch), dim3(256), 0,
                     stream, x, lab, cursor,
                     (uint32_t)n_records, (uint32_t)batch, H, W, pad, flags, half_bits, (uint32_t)seed,
                     (uint32_t)(seed >> 32), y, lab_out, params_out, norm_coef(m0, m1, m2, s0, s1, s2));
  SL_CHECK_LAUNCH();
  return 0;
}

// sl_input_aug followed by mixup / CutMix with another sample of the batch.  table: int32 [2][4096]
// (mixup's row, CutMix's row); modes: 1 = mixup, 2 = CutMix, 3 = either, drawn per batch.  mix_out:
// int32 [batch][8].  Reads cursor and table on the device: a captured graph replays it.
int sl_input_mix(const uint8_t* x, const uint8_t* lab, const int* cursor, int n_records, int batch, int H, int W,
                 int pad, int flags, unsigned long long seed, const int* table, int modes, uint16_t* y,
                 uint8_t* lab_out, int* params_out, int* mix_out, float m0, float m1, float m2, float s0, float s1,
                 float s2, hipStream_t stream) {
  if (!x || !cursor || !y || !table || (lab_out && !lab)) return -2;
  if (batch < 2 || batch > 65535 || n_records < batch || H < 1 || W < 1 || (long)H * W > (1L << 22)) return -1;
  if (pad < 0 || pad >= H || pad >= W || (flags & ~3) || modes < 1 || modes > 3) return -1;
  int bits = 0;  // the Feistel network's half width, as in sl_input_aug
  while (bits < 32 && ((unsigned long long)(n_records - 1) >> bits)) ++bits;
  if (bits < 2) bits = 2;
  const int half_bits = (bits + 1) / 2;
  hipLaunchKernelGGL(input_mix_kernel, dim3((H * W + 256 * AUG_PX - 1) / (256 * AUG_PX), batch), dim3(256), 0,
                     stream, x, lab, cursor, (uint32_t)n_records, (uint32_t)batch, H, W, pad, flags, half_bits,
                     (uint32_t)seed, (uint32_t)(seed >> 32), table, modes, y, lab_out, params_out, mix_out,
                     norm_coef(m0, m1, m2, s0, s1, s2));
  SL_CHECK_LAUNCH();
  return 0;
}

int sl_cursor_bump(int* cursor, hipStream_t stream) {
  hipLaunchKernelGGL(cursor_bump_kernel, dim3(1), dim3(1), 0, stream, cursor);
  SL_CHECK_LAUNCH();
  return 0;
}

int sl_bn_finalize(const float* stats, const float* gamma, const float* beta, float* coef, float* run_mean,
                   float* run_var, int C, float count, float eps, float momentum, hipStream_t stream) {
  hipLaunchKernelGGL(bn_finalize_kernel, dim3((C + 255) / 256), dim3(256), 0, stream, stats, gamma, beta, coef,
                     run_mean, run_var, C, count, eps, momentum);
  SL_CHECK_LAUNCH();
  return 0;
}

int sl_bn_apply(const uint16_t* x, const float* coef, const uint16_t* res, const float* rcoef, uint16_t* y, long rows,
                int C, int relu, int mode, hipStream_t stream) {
  if (C & 7) return -1;
  if (mode && !res) return -2;
  if (mode == 2 && !rcoef) return -2;
  hipLaunchKernelGGL(bn_apply_kernel, dim3(blocks_for(rows * (C / 8))), dim3(256), 0, stream, x, coef, res, rcoef, y,
                     rows, C, relu, mode);
  SL_CHECK_LAUNCH();
  return 0;
}

int sl_bn_bwd_reduce(const uint16_t* dy, const uint16_t* y, const uint16_t* x, const float* mcoef,
                     const uint8_t* ymask, uint16_t* dz_out, float* sums, const uint16_t* x2, float* sums2,
                     long rows, int C, hipStream_t stream) {
  if ((C & 7) || C > 2048 || (C & (C - 1))) return -1;
  if ((x2 == nullptr) != (sums2 == nullptr)) return -2;
  const int rpp = 256 / (C / 8);
  static int cap = -1;  // grid cap; SL_BNRED_BLOCKS overrides it for A/B runs
  if (cap < 0) {
    const char* e = getenv("SL_BNRED_BLOCKS");
    cap = e ? atoi(e) : 512;  // measured: 128/256/384/512/768/1024/2048/4096 -> profiles/r01_v16
    if (cap < 1) cap = 512;
  }
  long blocks = (rows + rpp * 8 - 1) / (rpp * 8);  // >= 8 rows per thread
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(bn_bwd_reduce_kernel, dim3(blocks), dim3(256), 0, stream, dy, y, x, mcoef, ymask, dz_out, sums, x2, sums2, rows,
                     C);
  SL_CHECK_LAUNCH();
  if (int rc = sl_rsum_fold2(sums, x2 ? sums2 : nullptr, 2 * C, stream)) return rc;
  return 0;
}

int sl_bn_bwd_finalize(const float* sums, const float* coef, float* dcoef, float* grad_gamma, float* grad_beta, int C,
                       float count, hipStream_t stream) {
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((C + 255) / 256), dim3(256), 0, stream, sums, coef, dcoef,
                     grad_gamma, grad_beta, C, count);
  SL_CHECK_LAUNCH();
  return 0;
}

int sl_bn_bwd_apply(const uint16_t* dy, const uint16_t* y, const uint16_t* x, const float* dcoef, uint16_t* dx,
                    long rows, int C, hipStream_t stream) {
  if (C & 7) return -1;
  hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(blocks_for(rows * (C / 8))), dim3(256), 0, stream, dy, y, x, dcoef,
                     dx, rows, C);
  SL_CHECK_LAUNCH();
  return 0;
}

int sl_bn_apply_stats(const uint16_t* x, const float* stats, const float* gamma, const float* beta, float* coef,
                      float* run_mean, float* run_var, const uint16_t* res, const float* rstats, const float* rgamma,
                      const float* rbeta, float* rcoef, float* rrun_mean, float* rrun_var, uint16_t* y,
                      uint8_t* mask_out, long rows, int C, int relu, int mode, float count, float eps, float momentum,
                      hipStream_t stream) {
  if ((C & 7) || 256 % (C / 8) != 0) return -1;
  if (mode && !res) return -2;
  if (mode >= 2 && !rstats) return -2;
  if (mode > 3) return -1;
  BnStats b{stats, gamma, beta, coef, run_mean, run_var};
  BnStats rb{rstats, rgamma, rbeta, rcoef, rrun_mean, rrun_var};
  hipLaunchKernelGGL(bn_apply_stats_kernel, dim3(blocks_for(rows * (C / 8), bn_apply_cap())), dim3(256), 0, stream, x, b, res, rb, y,
                     mask_out, rows, C, relu, mode, count, eps, momentum);
  SL_CHECK_LAUNCH();
  return 0;
}

int sl_bn_bwd_apply_dual(const uint16_t* dz, const uint16_t* xa, const float* sums_a, const float* coef_a,
                         float* gg_a, float* gb_a, uint16_t* dx_a, const uint16_t* xb, const float* sums_b,
                         const float* coef_b, float* gg_b, float* gb_b, uint16_t* dx_b, long rows, int C,
                         float count, hipStream_t stream) {
  if ((C & 7) || 256 % (C / 8) != 0) return -1;
  BnBwdSide a{xa, sums_a, coef_a, gg_a, gb_a, dx_a};
  BnBwdSide b{xb, sums_b, coef_b, gg_b, gb_b, dx_b};
  hipLaunchKernelGGL(bn_bwd_apply_dual_kernel, dim3(blocks_for(rows * (C / 8), bn_apply_cap())), dim3(256), 0,
                     stream, dz, a, b, rows, C, count);
  SL_CHECK_LAUNCH();
  return 0;
}

int sl_bn_bwd_apply_sums(const uint16_t* dy, const uint16_t* y, const uint16_t* x, const float* mcoef, const float* sums,
                         const float* coef, float* grad_gamma, float* grad_beta, uint16_t* dx, long rows, int C,
                         float count, hipStream_t stream) {
  if ((C & 7) || 256 % (C / 8) != 0) return -1;
  hipLaunchKernelGGL(bn_bwd_apply_sums_kernel, dim3(blocks_for(rows * (C / 8), bn_apply_cap())), dim3(256), 0, stream, dy, y, x, mcoef,
                     sums, coef, grad_gamma, grad_beta, dx, rows, C, count);
  SL_CHECK_LAUNCH();
  return 0;
}

int sl_maxpool_fwd(const uint16_t* x, uint16_t* y, uint8_t* arg, int N, int H, int W, int C, int OH, int OW, int K,
                   int s, int p, hipStream_t stream) {
  if ((C & 7) || K * K > 255) return -1;
  hipLaunchKernelGGL(maxpool_fwd_kernel, dim3(blocks_for((long)N * OH * OW * (C / 8))), dim3(256), 0, stream, x, y,
                     arg, N, H, W, C, OH, OW, K, s, p);
  SL_CHECK_LAUNCH();
  return 0;
}

int sl_maxpool_bwd(const uint16_t* dy, const uint8_t* arg, uint16_t* dx, int N, int H, int W, int C, int OH, int OW,
                   int K, int s, int p, hipStream_t stream) {
  if (C & 7) return -1;
  hipLaunchKernelGGL(maxpool_bwd_kernel, dim3(blocks_for((long)N * H * W * (C / 8))), dim3(256), 0, stream, dy, arg,
                     dx, N, H, W, C, OH, OW, K, s, p);
  SL_CHECK_LAUNCH();
  return 0;
}

int sl_avgpool_fwd(const uint16_t* x, uint16_t* y, int N, int HW, int C, hipStream_t stream) {
  if (C & 7) return -1;
  hipLaunchKernelGGL(avgpool_fwd_kernel, dim3(blocks_for((long)N * (C / 8))), dim3(256), 0, stream, x, y, N, HW, C);
  SL_CHECK_LAUNCH();
  return 0;
}

int sl_avgpool_bwd(const uint16_t* dy, uint16_t* dx, int N, int HW, int C, hipStream_t stream) {
  if (C & 7) return -1;
  hipLaunchKernelGGL(avgpool_bwd_kernel, dim3(blocks_for((long)N * HW * (C / 8))), dim3(256), 0, stream, dy, dx, N,
                     HW, C);
  SL_CHECK_LAUNCH();
  return 0;
}

int sl_softmax_ce(const float* z, const uint8_t* lab, float* loss, float* correct, uint16_t* dz, int ldd,
                  float* dbias, int N, int ncls, float grad_scale, hipStream_t stream) {
  if (ncls > 16 || ldd > 16 || ldd < ncls) return -1;
  hipLaunchKernelGGL(softmax_ce_kernel<false>, dim3((N + 15) / 16), dim3(256), 0, stream, z, lab, loss, correct, dz, ldd,
                     dbias, N, ncls, grad_scale);
  SL_CHECK_LAUNCH();
  return 0;
}

// Soft-target form: mix (int32 [N][8], nullable) pairs each row with a partner row and its weight,
// eps is the label smoothing; with mix null and eps 0 it computes what sl_softmax_ce does.
int sl_softmax_ce_soft(const float* z, const uint8_t* lab, float* loss, float* correct, uint16_t* dz, int ldd,
                       float* dbias, int N, int ncls, float grad_scale, const int* mix, float eps,
                       hipStream_t stream) {
  if (ncls > 16 || ncls < 1 || ldd > 16 || ldd < ncls || !(eps >= 0.f && eps < 1.f)) return -1;
  hipLaunchKernelGGL((softmax_ce_kernel<true, const int*, float>), dim3((N + 15) / 16), dim3(256), 0, stream, z, lab, loss, correct, dz,
                     ldd, dbias, N, ncls, grad_scale, mix, eps);
  SL_CHECK_LAUNCH();
  return 0;
}

// fp32 words of the bias-gradient workspace that sl_softmax_ce_wide needs for N rows at stride ldd
long sl_softmax_ce_wide_ws_floats(int N, int ldd) { return N < 1 || ldd < 1 ? 0 : ce_wide_parts(N) * ldd; }

// The loss over 17..256 classes (softmax_ce_wide_kernel).  soft = 0: one-hot labels, mix and eps
// ignored; soft = 1: sl_softmax_ce_soft's targets.  ldd: a power of two with max(32, ncls) <= ldd <=
// 256 (the FC data gradient reads dz as an ldd-channel image).  ws: caller-owned fp32 workspace of
// ws_floats >= sl_softmax_ce_wide_ws_floats(N, ldd) words, needed when dbias is given; it holds
// nothing between calls.  Anything else is refused before any launch.
int sl_softmax_ce_wide(const float* z, const uint8_t* lab, float* loss, float* correct, uint16_t* dz, int ldd,
                       float* dbias, int N, int ncls, float grad_scale, const int* mix, float eps, int soft,
                       float* ws, long ws_floats, hipStream_t stream) {
  if (ncls < 17 || ncls > 256 || N < 1) return -1;
  if (ldd < 32 || ldd > 256 || (ldd & (ldd - 1)) || ldd < ncls) return -1;
  if (soft && !(eps >= 0.f && eps < 1.f)) return -1;
  if (!z || !lab || !dz || ((uintptr_t)dz & 7)) return -2;
  const long parts = ce_wide_parts(N);
  if (dbias && (!ws || ws_floats < parts * ldd)) return -1;
  if (parts > 0x7fffffffL) return -1;
  const bool vec = ncls % 4 == 0 && ((uintptr_t)z & 15) == 0;
  const dim3 grid((unsigned)parts), block(256);
  float* part = dbias ? ws : nullptr;
  const int rpw = ce_wide_rows_per_wave();
  if (soft) {
    if (vec)
      hipLaunchKernelGGL((softmax_ce_wide_kernel<true, true>), grid, block, 0, stream, z, lab, loss, correct, dz, ldd,
                         part, N, ncls, grad_scale, mix, eps, rpw);
    else
      hipLaunchKernelGGL((softmax_ce_wide_kernel<true, false>), grid, block, 0, stream, z, lab, loss, correct, dz, ldd,
                         part, N, ncls, grad_scale, mix, eps, rpw);
  } else {
    if (vec)
      hipLaunchKernelGGL((softmax_ce_wide_kernel<false, true>), grid, block, 0, stream, z, lab, loss, correct, dz, ldd,
                         part, N, ncls, grad_scale, (const int*)nullptr, 0.f, rpw);
    else
      hipLaunchKernelGGL((softmax_ce_wide_kernel<false, false>), grid, block, 0, stream, z, lab, loss, correct, dz,
                         ldd, part, N, ncls, grad_scale, (const int*)nullptr, 0.f, rpw);
  }
  SL_CHECK_LAUNCH();
  if (dbias) {
    hipLaunchKernelGGL(softmax_ce_wide_fold_kernel, dim3(1), dim3(256), 0, stream, ws, (int)parts, ldd, ncls, dbias);
    SL_CHECK_LAUNCH();
  }
  return 0;
}

}  // extern "C"

// TrivialAugment Wide for the ResNet trainers' input pipeline (auto_augment="trivial-wide";
// serverless_learn_amd/data/augment.py ta_table / ta_params / ta_apply is the definition, in integers,
// and this kernel equals it bit for bit): after shuffle / crop / flip every sample of the batch gets
// ONE of torchvision's 14 TrivialAugmentWide operations, at one of 31 strengths and a random sign,
// drawn from T = Philox(t, 0, j; stream 4): op = T.x % 14, bin = T.y % 31, neg = T.z & 1.
//
//    0 Identity      1 ShearX       2 ShearY     3 TranslateX    4 TranslateY
//    5 Rotate        6 Brightness   7 Color      8 Contrast      9 Sharpness
//   10 Posterize    11 Solarize    12 AutoContrast              13 Equalize
//
// Work split.  Half of these need the whole image (a histogram and its prefix sums, a minimum and a
// maximum, a mean, a 3x3 filter, an affine resample), so unlike the per-pixel gathers of cnn_aux.hip
// one 256-thread workgroup OWNS one sample and keeps its image in LDS: one packed word
// r | g << 8 | b << 16 per pixel, at most TA_MAX_PX = 4096 of them (16 KB).  Thread tid handles the
// pixels p = tid + 256 k, k < 16, so a wave's LDS and global accesses stay contiguous.
//
//   prologue  aug_draw (record, oy, ox, flip), the TrivialAugment draw and the operation's eight table
//             integers: functions of kernel arguments, blockIdx and the cursor alone, so the compiler
//             keeps them in scalar registers, once per wave
//   stage 1   gather the cropped / flipped source image into LDS (aug_pixel, as input_aug reads it)
//   stage 2   a switch on op, uniform in the workgroup, so every barrier inside a case is reached by
//             all threads.  Results stay in registers (16 words a thread, statically indexed):
//               geometric   the integer inverse map per output pixel, one LDS read of the source word
//               Sharpness   the eight neighbours from LDS
//               Contrast    sum of L: a thread's pixels, xor shuffles across the wave, one LDS
//                           integer add per wave
//               AutoContrast  per-channel min / max the same way (LDS integer min / max)
//               Equalize    three 256-bin histograms by LDS integer atomics; thread v owns level v of
//                           each channel: an in-wave inclusive prefix by shuffles, wave totals through
//                           LDS; the level whose prefix reaches H W with a non-zero count is the largest
//                           occupied one; then a 3 x 256 LUT over the histograms
//   stage 3   after a barrier the registers go back to LDS as the image's 3 H W bytes, and leave as a
//             contiguous stream of whole dwords (bytes when 3 H W is no multiple of 4) into the u8
//             staging batch ta_x [B][H][W][3]; thread 0 writes the label and the two parameter rows
//
// Only integers are accumulated, so the order of the atomics and shuffles cannot matter: the same
// bits on every run and in both builds.  Every float of the method was rounded once on the host into
// the table (int32 [14][31][2][8]); nothing here multiplies a float.
//
// Downstream the unchanged input_norm (or input_mix, over the staging batch as a "shard" of B
// records with no shuffle, crop or padding) produces the bf16 batch the network reads.
#include "common.h"
#include "aug_draw.h"

using namespace sl;

namespace {

constexpr int TA_THREADS = 256;
constexpr int TA_WAVES = TA_THREADS / 64;
constexpr int TA_MAX_PX = 4096;               // data/augment.py TA_MAX_PIXELS
constexpr int TA_PX = TA_MAX_PX / TA_THREADS; // pixels per thread
constexpr int TA_OPS = 14, TA_BINS = 31;      // data/augment.py TA_OPS, TA_BINS

// slots of the small LDS scratch
enum { RED_SUM = 0, RED_LO = 1, RED_HI = 4, RED_LAST = 8, RED_N = 12 };

__device__ __forceinline__ int wave_sum(int a) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) a += __shfl_xor(a, m);
  return a;
}

__device__ __forceinline__ int wave_min(int a) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) a = min(a, __shfl_xor(a, m));
  return a;
}

__device__ __forceinline__ int wave_max(int a) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) a = max(a, __shfl_xor(a, m));
  return a;
}

__device__ __forceinline__ int ch(uint32_t w, int c) { return (int)((w >> (8 * c)) & 255u); }

__device__ __forceinline__ uint32_t pack3(int r, int g, int b) {
  return (uint32_t)r | (uint32_t)g << 8 | (uint32_t)b << 16;
}

// the grey of a pixel: (77 r + 150 g + 29 b + 128) >> 8, at most 255
__device__ __forceinline__ int grey(uint32_t w) {
  return (77 * ch(w, 0) + 150 * ch(w, 1) + 29 * ch(w, 2) + 128) >> 8;
}

// a blended with the degenerate value d: a at F = 256, d at F = 0 (arithmetic shift: floor)
__device__ __forceinline__ int blend(int a, int d, int F) {
  return min(max((256 * d + F * (a - d) + 128) >> 8, 0), 255);
}

__device__ __forceinline__ uint32_t blend3(uint32_t w, int d0, int d1, int d2, int F) {
  return pack3(blend(ch(w, 0), d0, F), blend(ch(w, 1), d1, F), blend(ch(w, 2), d2, F));
}

// f(p, word of pixel p) -> the new word, for each of this thread's pixels
template <typename F>
__device__ __forceinline__ void each_pixel(uint32_t (&r)[TA_PX], int tid, int img, F f) {
#pragma unroll
  for (int k = 0; k < TA_PX; ++k) {
    const int p = tid + TA_THREADS * k;
    if (p < img) r[k] = f(p, r[k]);
  }
}

__global__ __launch_bounds__(TA_THREADS) void input_ta_kernel(
    const uint8_t* __restrict__ x, const uint8_t* __restrict__ lab, const int* __restrict__ cursor, uint32_t n_records,
    uint32_t batch, int H, int W, int pad, int flags, int half_bits, uint32_t k0, uint32_t k1,
    const int* __restrict__ table, uint8_t* __restrict__ ta_x, uint8_t* __restrict__ ta_lab,
    int* __restrict__ params_out, int* __restrict__ ta_out, int force) {
  __shared__ uint32_t img_s[TA_MAX_PX];   // the source image as packed words, then the result as bytes
  __shared__ int aux[3 * 256];            // Equalize: the histograms, then the LUT
  __shared__ int red[RED_N];              // sum of L | lo[3] | hi[3] | count of the largest level [3]
  __shared__ int wtot[3 * TA_WAVES];      // Equalize: each wave's total per channel

  // ---- prologue: uniform in the workgroup ----
  const uint32_t j = blockIdx.x;
  const uint32_t t = (uint32_t)*cursor;  // a non-negative int32
  const AugDraw d = aug_draw(j, t, n_records, batch, pad, flags, half_bits, k0, k1);
  int op, bin, neg;
  if (force >= 0) {  // (sl_input_ta checked the ranges)
    op = force & 255;
    bin = (force >> 8) & 255;
    neg = (force >> 16) & 1;
  } else {
    const U4 T = philox4x32_10(t, 0u, j, 4u, k0, k1);
    op = (int)(T.x % (uint32_t)TA_OPS);
    bin = (int)(T.y % (uint32_t)TA_BINS);
    neg = (int)(T.z & 1u);
  }
  const int* e = table + ((op * TA_BINS + bin) * 2 + neg) * 8;
  const int e0 = e[0], e1 = e[1], e2 = e[2], e3 = e[3], e4 = e[4], e5 = e[5];

  const int tid = threadIdx.x;
  const int img = H * W;  // <= TA_MAX_PX (sl_input_ta)
  if (tid < RED_N) red[tid] = (tid >= RED_LO && tid < RED_HI) ? 255 : 0;
  if (op == 13) {
#pragma unroll
    for (int c = 0; c < 3; ++c) aux[c * 256 + tid] = 0;
  }

  // ---- stage 1: the cropped / flipped image -> LDS ----
  const uint8_t* src = x + (long)d.rec * img * 3;
#pragma unroll
  for (int k = 0; k < TA_PX; ++k) {
    const int p = tid + TA_THREADS * k;
    if (p < img) {
      const int py = p / W, px = p - py * W;
      img_s[p] = aug_pixel(src, d, py, px, H, W, pad);
    }
  }
  __syncthreads();

  // ---- stage 2: the operation, results in registers ----
  uint32_t r[TA_PX];
#pragma unroll
  for (int k = 0; k < TA_PX; ++k) {
    const int p = tid + TA_THREADS * k;
    r[k] = p < img ? img_s[p] : 0u;
  }
  switch (op) {
    case 1: case 2: case 3: case 4: case 5: {  // ShearX, ShearY, TranslateX, TranslateY, Rotate
      // doubled centred coordinates u = 2x - (W-1), v = 2y - (H-1); the source's in Q16; |values| stay
      // below 2^30 for H W <= 4096 (|u| + |v| < 4097, coefficients <= 2^16, translations <= 2^22)
      const int bx = (W - 1) * 65536 + 65536, by = (H - 1) * 65536 + 65536;
      each_pixel(r, tid, img, [&](int p, uint32_t) {
        const int py = p / W, px = p - py * W;
        const int u = 2 * px - (W - 1), v = 2 * py - (H - 1);
        const int sx = (e0 * u + e1 * v + e2 + bx) >> 17, sy = (e3 * u + e4 * v + e5 + by) >> 17;
        const bool in = (unsigned)sx < (unsigned)W && (unsigned)sy < (unsigned)H;
        return in ? img_s[sy * W + sx] : 0u;  // black outside
      });
      break;
    }
    case 6:  // Brightness: towards black
      each_pixel(r, tid, img, [&](int, uint32_t w) { return blend3(w, 0, 0, 0, e0); });
      break;
    case 7:  // Color: towards the pixel's grey
      each_pixel(r, tid, img, [&](int, uint32_t w) {
        const int L = grey(w);
        return blend3(w, L, L, L, e0);
      });
      break;
    case 8: {  // Contrast: towards the image's mean grey
      int s = 0;
#pragma unroll
      for (int k = 0; k < TA_PX; ++k)
        if (tid + TA_THREADS * k < img) s += grey(r[k]);
      s = wave_sum(s);
      if ((tid & 63) == 0) atomicAdd(&red[RED_SUM], s);
      __syncthreads();
      const int mean = (int)((uint32_t)(red[RED_SUM] + img / 2) / (uint32_t)img);
      each_pixel(r, tid, img, [&](int, uint32_t w) { return blend3(w, mean, mean, mean, e0); });
      break;
    }
    case 9:  // Sharpness: towards the 3x3 smooth (sum of 9 + 4 centre + 6) / 13, the border kept
      each_pixel(r, tid, img, [&](int p, uint32_t w) {
        const int py = p / W, px = p - py * W;
        if (px < 1 || py < 1 || px > W - 2 || py > H - 2) return w;  // blend(a, a, F) = a
        int s0 = 0, s1 = 0, s2 = 0;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
          for (int dx = -1; dx <= 1; ++dx) {
            const uint32_t q = img_s[p + dy * W + dx];
            s0 += ch(q, 0);
            s1 += ch(q, 1);
            s2 += ch(q, 2);
          }
        return blend3(w, (s0 + 4 * ch(w, 0) + 6) / 13, (s1 + 4 * ch(w, 1) + 6) / 13, (s2 + 4 * ch(w, 2) + 6) / 13,
                      e0);
      });
      break;
    case 10:  // Posterize: e0 is the mask of the kept high bits
      each_pixel(r, tid, img, [&](int, uint32_t w) { return w & ((uint32_t)e0 * 0x010101u); });
      break;
    case 11:  // Solarize: invert at and above the threshold
      each_pixel(r, tid, img, [&](int, uint32_t w) {
        const int a0 = ch(w, 0), a1 = ch(w, 1), a2 = ch(w, 2);
        return pack3(a0 < e0 ? a0 : 255 - a0, a1 < e0 ? a1 : 255 - a1, a2 < e0 ? a2 : 255 - a2);
      });
      break;
    case 12: {  // AutoContrast: stretch each channel's [lo, hi] to [0, 255]
      int lo[3] = {255, 255, 255}, hi[3] = {0, 0, 0};
#pragma unroll
      for (int k = 0; k < TA_PX; ++k)
        if (tid + TA_THREADS * k < img) {
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            lo[c] = min(lo[c], ch(r[k], c));
            hi[c] = max(hi[c], ch(r[k], c));
          }
        }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        lo[c] = wave_min(lo[c]);
        hi[c] = wave_max(hi[c]);
        if ((tid & 63) == 0) {
          atomicMin(&red[RED_LO + c], lo[c]);
          atomicMax(&red[RED_HI + c], hi[c]);
        }
      }
      __syncthreads();
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        lo[c] = red[RED_LO + c];
        hi[c] = red[RED_HI + c] - lo[c];  // the span
      }
      each_pixel(r, tid, img, [&](int, uint32_t w) {
        int o[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const int a = ch(w, c);
          // rounded (a - lo) 255 / span; a constant channel (span 0) is left alone
          o[c] = hi[c] ? (int)((uint32_t)((a - lo[c]) * 510 + hi[c]) / (uint32_t)(2 * hi[c])) : a;
        }
        return pack3(o[0], o[1], o[2]);
      });
      break;
    }
    case 13: {  // Equalize (PIL's rule), per channel
#pragma unroll
      for (int k = 0; k < TA_PX; ++k)
        if (tid + TA_THREADS * k < img) {
#pragma unroll
          for (int c = 0; c < 3; ++c) atomicAdd(&aux[c * 256 + ch(r[k], c)], 1);
        }
      __syncthreads();
      // thread v owns level v: h = its count, incl = the counts of levels <= v
      const int lane = tid & 63, wave = tid >> 6;
      int h[3], incl[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        h[c] = incl[c] = aux[c * 256 + tid];
#pragma unroll
        for (int m = 1; m < 64; m <<= 1) {
          const int up = __shfl_up(incl[c], m);
          if (lane >= m) incl[c] += up;
        }
        if (lane == 63) wtot[c * TA_WAVES + wave] = incl[c];
      }
      __syncthreads();
#pragma unroll
      for (int c = 0; c < 3; ++c) {
#pragma unroll
        for (int w = 0; w < TA_WAVES - 1; ++w)
          if (w < wave) incl[c] += wtot[c * TA_WAVES + w];
        // every level from the largest occupied one up has incl = H W; only that one has h > 0
        if (h[c] > 0 && incl[c] == img) red[RED_LAST + c] = h[c];
      }
      __syncthreads();
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const uint32_t step = (uint32_t)(img - red[RED_LAST + c]) / 255u;
        // (thread v alone read aux[c][v] above, so the LUT can take the histogram's place)
        aux[c * 256 + tid] = step ? (int)min(255u, (step / 2u + (uint32_t)(incl[c] - h[c])) / step) : tid;
      }
      __syncthreads();
      each_pixel(r, tid, img, [&](int, uint32_t w) {
        return pack3(aux[ch(w, 0)], aux[256 + ch(w, 1)], aux[512 + ch(w, 2)]);
      });
      break;
    }
    default:  // Identity
      break;
  }

  // ---- stage 3: registers -> LDS bytes -> one contiguous stream ----
  __syncthreads();  // every read of the source words is done
  uint8_t* out_s = reinterpret_cast<uint8_t*>(img_s);
#pragma unroll
  for (int k = 0; k < TA_PX; ++k) {
    const int p = tid + TA_THREADS * k;
    if (p < img) {
      out_s[3 * p] = (uint8_t)ch(r[k], 0);
      out_s[3 * p + 1] = (uint8_t)ch(r[k], 1);
      out_s[3 * p + 2] = (uint8_t)ch(r[k], 2);
    }
  }
  __syncthreads();
  const int nbytes = 3 * img;
  uint8_t* dst = ta_x + (long)j * nbytes;
  if ((nbytes & 3) == 0) {  // then every sample's slice of ta_x starts on a dword
    uint32_t* dst4 = reinterpret_cast<uint32_t*>(dst);
    for (int i = tid; i < nbytes / 4; i += TA_THREADS) dst4[i] = img_s[i];
  } else {
    for (int i = tid; i < nbytes; i += TA_THREADS) dst[i] = out_s[i];
  }
  if (tid == 0) {
    ta_lab[j] = lab[d.rec];
    *reinterpret_cast<int4*>(params_out + 4 * j) = make_int4((int)d.rec, d.oy, d.ox, d.flip);
    *reinterpret_cast<int4*>(ta_out + 4 * j) = make_int4(op, bin, neg, 0);
  }
}

}  // namespace

extern "C" {

// One TrivialAugment Wide operation per sample of the batch at the cursor, after sl_input_aug's
// shuffle / crop / flip (flags, pad, seed as there): u8 ta_x [batch][H][W][3] and ta_lab [batch],
// params_out int32 [batch][4] = (record, oy, ox, flip), ta_out int32 [batch][4] = (op, bin, neg, 0).
// table: int32 [14][31][2][8] (data/augment.py ta_table).  force: -1 = draw, else
// op | bin << 8 | neg << 16 for every sample (tests).  Reads cursor and table on the device: a
// captured graph replays it.  The grid is one workgroup per sample.
int sl_input_ta(const uint8_t* x, const uint8_t* lab, const int* cursor, int n_records, int batch, int H, int W,
                int pad, int flags, unsigned long long seed, const int* table, uint8_t* ta_x, uint8_t* ta_lab,
                int* params_out, int* ta_out, int force, hipStream_t stream) {
  if (!x || !lab || !cursor || !table || !ta_x || !ta_lab || !params_out || !ta_out) return -2;
  if (batch < 1 || n_records < batch || H < 1 || W < 1 || (long)H * W > TA_MAX_PX) return -1;
  if (pad < 0 || pad >= H || pad >= W || (flags & ~3)) return -1;
  if (force < -1 || (force >= 0 && ((force & 255) >= TA_OPS || ((force >> 8) & 255) >= TA_BINS || (force >> 17))))
    return -1;
  // the Feistel network's half width, as in sl_input_aug
  int bits = 0;
  while (bits < 32 && ((unsigned long long)(n_records - 1) >> bits)) ++bits;
  if (bits < 2) bits = 2;
  const int half_bits = (bits + 1) / 2;
  hipLaunchKernelGGL(input_ta_kernel, dim3(batch), dim3(TA_THREADS), 0, stream, x, lab, cursor, (uint32_t)n_records,
                     (uint32_t)batch, H, W, pad, flags, half_bits, (uint32_t)seed, (uint32_t)(seed >> 32), table, ta_x,
                     ta_lab, params_out, ta_out, force);
  SL_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"

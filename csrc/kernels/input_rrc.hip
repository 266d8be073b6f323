// RandomResizedCrop + horizontal flip for the ResNet trainers' input pipeline (augment="rrc-flip";
// serverless_learn_amd/data/augment.py rrc_table / rrc_params / rrc_apply is the definition, in integers,
// and this kernel equals it bit for bit): sample j of the batch at cursor t takes a box of random
// area and aspect ratio out of its record and resizes it back to the O x O input, bilinearly with
// half-pixel centres, mirrored at random.  The first kernel of the pipeline that interpolates.
//
// Work split.  One 256-thread workgroup owns one image and one BAND of RRC_BAND = 16 output rows:
// grid (ceil(O / 16), B).  A 224 x 224 image never has to sit on chip whole, and a batch of 32 x 32
// images still spreads over 2 B workgroups.
//
//   prologue  the record (aug_draw.h, the draw the other input kernels share), the ten-try box draw
//             from R_k = Philox(t, k, j; stream 5) through the table, and the flip: functions of kernel
//             arguments, blockIdx and the cursor alone, so the compiler keeps them in scalar
//             registers, once per wave.  Every band of an image derives the same box; band 0 writes
//             the image's rrc_out / params_out rows and its label
//   taps      thread x < O does the one integer division of output column x, the flip folded into
//             the column order, and stores (x0, x1, fx) as one LDS word; sixteen lanes do the same
//             for the band's rows: (y0, y1, fy), rows counted from the band's first source row
//   pass 1    horizontal.  The crop is never larger than the output, so 16 output rows lie between at
//             most RRC_ROWS - 1 = 17 source rows (rrc_band below).  For every pixel of those rows a thread
//             reads the two tap pixels straight from the shard -- bytes of one contiguous row, and the
//             shard's rows stay in L2 -- and writes hr = a (256 - fx) + b fx, exact in 16 bits, as
//             four u16 (8 bytes) into the LDS image hr_s, at most 18 x 256 x 8 = 36 KB.  A source byte
//             is read once per band, not once per output pixel, and an output pixel costs two taps
//             here and two in pass 2 instead of four 2-D ones
//   pass 2    vertical, after a barrier.  A thread produces four adjacent output pixels from four
//             16-byte LDS reads (two source rows), rounds once, (hr0 (256 - fy) + hr1 fy + 32768) >> 16,
//             packs the twelve bytes and stores three dwords; a band's output is one contiguous range
//
// No atomics, no state, no floats: the same bits on every run and in both builds.  Every float of
// the method was rounded once on the host into the table (int32 [256][256], w | h << 16 or 0).
//
// Downstream the unchanged input_ta, input_mix or input_norm reads the staging batch rrc_x as a
// "shard" of B records with no shuffle, crop or padding.
#include "common.h"
#include "aug_draw.h"

using namespace sl;

namespace {

constexpr int RRC_THREADS = 256;
constexpr int RRC_BAND = 16;     // output rows per workgroup
constexpr int RRC_ROWS = 18;     // rows of the LDS image (17 are reachable)
constexpr int RRC_MAX_O = 256;   // data/augment.py RRC_MAX_HW
constexpr int RRC_L = 256;       // data/augment.py RRC_L
constexpr int RRC_TRIES = 10;    // data/augment.py RRC_TRIES
constexpr uint32_t RRC_STREAM = 5u;

// Output position i along an axis whose crop is n long (data/augment.py rrc_taps): the floor s of
// the source coordinate ((2i + 1) n - O) / 2O, which is -1 at the least, and its fraction in Q8.
__device__ __forceinline__ void rrc_tap(int i, int n, int O, int& s, int& f) {
  const uint32_t num = (uint32_t)((2 * i + 1) * n + O);  // < 2 * 256 * 256 + 256
  const uint32_t q = num / (uint32_t)(2 * O);
  s = (int)q - 1;
  f = (int)(((num - q * (uint32_t)(2 * O)) * 256u + (uint32_t)O) / (uint32_t)(2 * O));  // 0..256
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

__global__ __launch_bounds__(RRC_THREADS) void input_rrc_kernel(
    const uint8_t* __restrict__ x, const uint8_t* __restrict__ lab, const int* __restrict__ cursor, uint32_t n_records,
    uint32_t batch, int O, int flags, int half_bits, uint32_t k0, uint32_t k1, const int* __restrict__ table,
    uint8_t* __restrict__ rrc_x, uint8_t* __restrict__ rrc_lab, int* __restrict__ params_out,
    int* __restrict__ rrc_out) {
  __shared__ uint4 hr_s[RRC_ROWS * RRC_MAX_O / 2];  // [row][column] of (r, g, b, 0) as u16: 8 bytes a pixel
  __shared__ uint32_t col_s[RRC_MAX_O];             // x0 | x1 << 8 | fx << 16, columns of the record
  __shared__ uint32_t row_s[RRC_BAND];              // y0 | y1 << 8 | fy << 16, rows of hr_s

  // ---- prologue: uniform in the workgroup ----
  const uint32_t j = blockIdx.y;
  const int band = blockIdx.x;
  const uint32_t t = (uint32_t)*cursor;  // a non-negative int32
  const uint32_t rec = aug_draw(j, t, n_records, batch, 0, flags & 1, half_bits, k0, k1).rec;
  int w = O, h = O, top = 0, left = 0, tries = RRC_TRIES, fallback = 1;  // ten misses: the whole image
  for (int k = 0; k < RRC_TRIES; ++k) {
    const U4 R = philox4x32_10(t, (uint32_t)k, j, RRC_STREAM, k0, k1);
    const int e = table[(R.x >> 24) * RRC_L + (R.y >> 24)];
    const int ew = e & 0xFFFF, eh = (e >> 16) & 0xFFFF;
    // (a box that does not fit is a miss whatever the table says: no load can leave the record)
    if (ew > 0 && ew <= O && eh > 0 && eh <= O) {
      w = ew;
      h = eh;
      top = (int)(R.z % (uint32_t)(O - h + 1));
      left = (int)(R.w % (uint32_t)(O - w + 1));
      tries = k + 1;
      fallback = 0;
      break;
    }
  }
  const int flip = (int)(philox4x32_10(t, (uint32_t)RRC_TRIES, j, RRC_STREAM, k0, k1).x & 1u);

  // the band's output rows [y_lo, y_hi] and the source rows [r_lo, r_hi] of the crop they touch.
  // s grows with y, by at most 15 over 15 rows because h <= O, so r_hi - r_lo <= 16: 17 rows
  const int y_lo = band * RRC_BAND, y_hi = min(y_lo + RRC_BAND, O) - 1;
  int s_lo, s_hi, f_unused;
  rrc_tap(y_lo, h, O, s_lo, f_unused);
  rrc_tap(y_hi, h, O, s_hi, f_unused);
  const int r_lo = clampi(s_lo, 0, h - 1), r_hi = clampi(s_hi + 1, 0, h - 1);
  const int n_rows = r_hi - r_lo + 1;

  // ---- taps ----
  const int tid = threadIdx.x;
  if (tid < O) {
    int s, f;
    rrc_tap(flip ? O - 1 - tid : tid, w, O, s, f);
    col_s[tid] = (uint32_t)(left + clampi(s, 0, w - 1)) | (uint32_t)(left + clampi(s + 1, 0, w - 1)) << 8 |
                 (uint32_t)f << 16;
  }
  if (tid <= y_hi - y_lo) {
    int s, f;
    rrc_tap(y_lo + tid, h, O, s, f);
    row_s[tid] = (uint32_t)(clampi(s, 0, h - 1) - r_lo) | (uint32_t)(clampi(s + 1, 0, h - 1) - r_lo) << 8 |
                 (uint32_t)f << 16;
  }
  __syncthreads();

  // ---- pass 1: horizontal, source rows r_lo .. r_hi of the crop -> hr_s ----
  // pixel p = tid + 256 k of the n_rows x O rows: its (row, column) advances without a division
  uint2* hr2 = reinterpret_cast<uint2*>(hr_s);
  const uint8_t* src = x + ((long)rec * O + (top + r_lo)) * O * 3;
  const int d_row = RRC_THREADS / O, d_col = RRC_THREADS - d_row * O;
  int pr = tid / O, pc = tid - pr * O;
  while (pr < n_rows) {
    const uint32_t c = col_s[pc];
    const int fx = (int)(c >> 16);
    const uint8_t* a = src + (pr * O + (int)(c & 255u)) * 3;
    const uint8_t* b = src + (pr * O + (int)((c >> 8) & 255u)) * 3;
    const uint32_t v0 = (uint32_t)(a[0] * (256 - fx) + b[0] * fx), v1 = (uint32_t)(a[1] * (256 - fx) + b[1] * fx),
                   v2 = (uint32_t)(a[2] * (256 - fx) + b[2] * fx);  // each <= 255 * 256
    hr2[pr * O + pc] = make_uint2(v0 | v1 << 16, v2);
    pr += d_row;
    pc += d_col;
    if (pc >= O) {
      pc -= O;
      ++pr;
    }
  }
  __syncthreads();

  // ---- pass 2: vertical, four adjacent output pixels a thread ----
  const int quads = O / 4;  // per row; O % 4 == 0 (sl_input_rrc)
  uint32_t* dst = reinterpret_cast<uint32_t*>(rrc_x + ((long)j * O + y_lo) * O * 3);  // 4-byte aligned: O % 4 == 0
  const int d_qrow = RRC_THREADS / quads, d_qcol = RRC_THREADS - d_qrow * quads;
  int qr = tid / quads, qc = tid - qr * quads;
  while (qr <= y_hi - y_lo) {
    const uint32_t rw = row_s[qr];
    const uint32_t fy = rw >> 16, gy = 256u - fy;
    const uint4* p0 = hr_s + ((int)(rw & 255u) * O + 4 * qc) / 2;
    const uint4* p1 = hr_s + ((int)((rw >> 8) & 255u) * O + 4 * qc) / 2;
    uint32_t o[12];
#pragma unroll
    for (int k = 0; k < 2; ++k) {  // two pixels per 16-byte read
      const uint4 u = p0[k], v = p1[k];
      o[6 * k + 0] = ((u.x & 0xFFFFu) * gy + (v.x & 0xFFFFu) * fy + 32768u) >> 16;
      o[6 * k + 1] = ((u.x >> 16) * gy + (v.x >> 16) * fy + 32768u) >> 16;
      o[6 * k + 2] = (u.y * gy + v.y * fy + 32768u) >> 16;
      o[6 * k + 3] = ((u.z & 0xFFFFu) * gy + (v.z & 0xFFFFu) * fy + 32768u) >> 16;
      o[6 * k + 4] = ((u.z >> 16) * gy + (v.z >> 16) * fy + 32768u) >> 16;
      o[6 * k + 5] = (u.w * gy + v.w * fy + 32768u) >> 16;
    }
    uint32_t* d = dst + (qr * O + 4 * qc) * 3 / 4;
    d[0] = o[0] | o[1] << 8 | o[2] << 16 | o[3] << 24;
    d[1] = o[4] | o[5] << 8 | o[6] << 16 | o[7] << 24;
    d[2] = o[8] | o[9] << 8 | o[10] << 16 | o[11] << 24;
    qr += d_qrow;
    qc += d_qcol;
    if (qc >= quads) {
      qc -= quads;
      ++qr;
    }
  }

  if (band == 0 && tid == 0) {
    rrc_lab[j] = lab[rec];
    *reinterpret_cast<int4*>(params_out + 4 * j) = make_int4((int)rec, top, left, flip);
    *reinterpret_cast<int4*>(rrc_out + 8 * j) = make_int4((int)rec, top, left, h);
    *reinterpret_cast<int4*>(rrc_out + 8 * j + 4) = make_int4(w, flip, tries, fallback);
  }
}

}  // namespace

extern "C" {

// RandomResizedCrop + flip of the batch at the cursor (data/augment.py rrc_params / rrc_apply): u8
// rrc_x [batch][O][O][3] and rrc_lab [batch], params_out int32 [batch][4] = (record, top, left, flip),
// rrc_out int32 [batch][8] = (record, top, left, h, w, flip, tries, fallback).  flags: 1 = shuffle
// (sl_input_aug's; no other bit).  table: int32 [256][256] (data/augment.py rrc_table).  Square images
// only, O = H = W a multiple of 4 in 4..256.  Reads cursor and table on the device: a captured graph
// replays it.  The grid is (bands of 16 output rows, samples).
int sl_input_rrc(const uint8_t* x, const uint8_t* lab, const int* cursor, int n_records, int batch, int H, int W,
                 int flags, unsigned long long seed, const int* table, uint8_t* rrc_x, uint8_t* rrc_lab,
                 int* params_out, int* rrc_out, hipStream_t stream) {
  if (!x || !lab || !cursor || !table || !rrc_x || !rrc_lab || !params_out || !rrc_out) return -2;
  if (H != W || H < 4 || H > RRC_MAX_O || H % 4 != 0) return -1;
  if (batch < 1 || batch > 65535 || n_records < batch || (flags & ~1)) return -1;
  // the Feistel network's half width, as in sl_input_aug
  int bits = 0;
  while (bits < 32 && ((unsigned long long)(n_records - 1) >> bits)) ++bits;
  if (bits < 2) bits = 2;
  const int half_bits = (bits + 1) / 2;
  hipLaunchKernelGGL(input_rrc_kernel, dim3((H + RRC_BAND - 1) / RRC_BAND, batch), dim3(RRC_THREADS), 0, stream, x,
                     lab, cursor, (uint32_t)n_records, (uint32_t)batch, H, flags, half_bits, (uint32_t)seed,
                     (uint32_t)(seed >> 32), table, rrc_x, rrc_lab, params_out, rrc_out);
  SL_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"

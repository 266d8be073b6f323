// GroupNorm for the ResNet trainers (norm="group"): statistics, normalisation, residual, ReLU
// and the ReLU mask in one kernel per direction, one read and one write of the tensor.
//
// Layout is the engine's, NHWC bf16 x[N][HW][C], with G groups of cpg = C / G contiguous
// channels.  Statistics are per (sample, group) over the HW * cpg stored bf16 values: mean, and
// the biased variance as the mean of squared deviations.
//
// Work split.  One 256-thread workgroup owns one (sample, 64-channel slab): C = 64 is one
// workgroup per sample, C = 512 eight.  A pixel's 64 channels of the slab are 128 B, one cache
// line, read as eight 16-byte chunks by eight neighbouring lanes: thread t owns chunk column
// t & 7 (channels 8 (t & 7) .. + 7 of the slab, the same eight for its whole life, so their
// gamma / beta / mean / rstd are fetched once) and the pixel rows (t >> 3) + 32 i.  Groups never
// straddle a slab, so cpg is one of 1, 2, 4, 8, 16, 32, 64, and a slab has at most HW = 1024
// rows (128 KB); anything else is refused by the launchers.
//
// The slab lives in REGISTERS, not LDS.  At HW = 1024 a thread holds 32 chunks = 128 VGPRs; the
// workgroup is four waves, one per SIMD, so each wave may use the SIMD's whole 512-entry file and
// 128 KB (forward: x) or 256 KB (backward: x and dz) fit with room for the arithmetic.  LDS
// (160 KB per CU) could hold the forward's slab but not the backward's two, it would cost a
// store and two loads per element on top of the global traffic, and every pass over the slab is
// over a thread's own elements anyway: only the 64 per-channel partial sums ever cross threads.
// The kernels are instantiated for 1, 2, 8 and 32 rows per thread (HW <= 32, 64, 256, 1024: the
// CIFAR ResNet-18's 4x4, 8x8, 16x16 and 32x32 maps), so the register arrays index statically.
//
// Reductions (slab_reduce) have a fixed order and use no atomics: a thread sums its own rows
// in row order (at most 32 additions), the eight lanes of a wave that share a chunk column fold
// by three xor shuffles (8, 16, 32), the four waves' rows of 64 channel sums go through LDS and
// are added in wave order (3 additions), and one thread per group adds its cpg channel totals in
// channel order (at most 63): a chain of at most 32 + 3 + 3 + 63 = 101 additions, the same bits
// from call to call and in both builds.  The variance is a second pass over the registers'
// deviations from the mean, not E[x^2] - E[x]^2.
//
// Precision.  The forward statistics (slab_stats) and the normalisation (gn_norm) run in fp64,
// which this GPU's vector units do at the fp32 rate and the kernels, bound by their 2 + 2 bytes
// per element, have room for: where gamma * xhat cancels against beta, an fp32 mean alone (one
// rounding, 6e-8 of |x|) is more than the 2^-9 of the result that the bf16 store leaves.  So y is
// the exact value rounded (to fp32, then to bf16), and mean / rstd are stored as the fp64 values
// rounded once.  The backward's arithmetic is fp32 on those stored statistics; only where it
// re-derives the ReLU mask of relu(gn(x)) it rebuilds the fp64 statistics from its own copy of
// the slab with the same code, so the mask is bit for bit the sign the forward stored.
//
//   gn_fwd         y = relu?(gamma (x - mean) rstd + beta (+ res)), mean / rstd [N][G] for the
//                  backward, optionally the 1-bit mask of y in bn_apply_stats's format
//   gn_bwd         dz = dy * mask (mask: 1-bit image of y | recomputed sign | none), dx, and one
//                  row of per-channel dgamma / dbeta partials per sample into ws[N][2][C]
//   gn_param_fold  adds the N rows in sample order into the flat gradient
#include "common.h"
#include "bn_fwd.h"

using namespace sl;

namespace {

constexpr int GN_SLAB = 64;               // channels per workgroup
constexpr int GN_THREADS = 256;
constexpr int GN_ROWS = GN_THREADS / 8;   // pixel rows per pass of the workgroup
constexpr int GN_MAX_HW = 1024;           // rows of the largest slab (32 per thread)

template <class T>
struct GnLds {
  T part[2][GN_THREADS / 64][GN_SLAB];  // each wave's per-channel sums (up to two quantities)
  T ch[2][GN_SLAB];                     // per-channel totals
  T grp[2][GN_SLAB];                    // per channel: its group's two values
};

// Per-channel totals of Q quantities over the slab -> s.ch[q][c]; v[q][j] is this thread's sum for
// channel 8 (t & 7) + j.  Fixed order: lanes by xor shuffles, waves through LDS in wave order.
template <int Q, class T>
__device__ __forceinline__ void slab_reduce(T (&v)[Q][8], GnLds<T>& s) {
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
#pragma unroll
  for (int q = 0; q < Q; ++q)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      T a = v[q][j];
      a += __shfl_xor(a, 8);
      a += __shfl_xor(a, 16);
      a += __shfl_xor(a, 32);
      if (lane < 8) s.part[q][wave][lane * 8 + j] = a;
    }
  __syncthreads();
  if (t < Q * GN_SLAB) {
    const int q = t >> 6, c = t & 63;
    s.ch[q][c] = ((s.part[q][0][c] + s.part[q][1][c]) + s.part[q][2][c]) + s.part[q][3][c];
  }
  __syncthreads();
}

// A chunk of the slab as the optimiser cannot relate it to its register: every pass over the slab
// then unpacks (and widens to fp64) a row at a time.  Left to itself the compiler keeps the
// widened values of the whole slab from one pass to the next, four times the registers of the
// bf16 copy, and spills.
__device__ __forceinline__ short8_t row_chunk(short8_t c) {
  asm volatile("" : "+v"(c));
  return c;
}

// The normalised value, one definition for both directions: the backward's recomputed ReLU mask
// must see the bits the forward stored.  fma, not a contraction left to the compiler.
__device__ __forceinline__ double gn_norm(float x, double mu, double rs, float ga, float be) {
  return fma((double)ga, ((double)x - mu) * rs, (double)be);
}

// Each group's mean and rstd of the slab in xr (rows beyond HW hold zeros), in fp64:
// s.grp[0][c] / s.grp[1][c] for every channel c of the slab.  Two passes: sum, then squared deviations.
template <int NI>
__device__ __forceinline__ void slab_stats(const short8_t (&xr)[NI], int HW, int cpg, float eps, GnLds<double>& s) {
  const int t = threadIdx.x, cc = t & 7, r0 = t >> 3, gps = GN_SLAB / cpg;
  const double m = (double)HW * (double)cpg;
  double v[1][8];
#pragma unroll
  for (int j = 0; j < 8; ++j) v[0][j] = 0.0;
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    float f[8];
    unpack8(row_chunk(xr[i]), f);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[0][j] += (double)f[j];
  }
  slab_reduce<1>(v, s);
  if (t < gps) {
    double a = 0.0;
    for (int c = t * cpg; c < (t + 1) * cpg; ++c) a += s.ch[0][c];
    a /= m;
    for (int c = t * cpg; c < (t + 1) * cpg; ++c) s.grp[0][c] = a;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 8; ++j) v[0][j] = 0.0;
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    if (r0 + GN_ROWS * i < HW) {
      float f[8];
      unpack8(row_chunk(xr[i]), f);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const double d = (double)f[j] - s.grp[0][cc * 8 + j];
        v[0][j] += d * d;
      }
    }
  }
  slab_reduce<1>(v, s);
  if (t < gps) {
    double a = 0.0;
    for (int c = t * cpg; c < (t + 1) * cpg; ++c) a += s.ch[0][c];
    const double r = 1.0 / sqrt(a / m + (double)eps);
    for (int c = t * cpg; c < (t + 1) * cpg; ++c) s.grp[1][c] = r;
  }
  __syncthreads();
}

// bit j = (the stored bf16 of relu(f[j]) > 0): bn_apply_stats_kernel's mask
__device__ __forceinline__ unsigned relu_bits(const short8_t& yv) {
  unsigned m = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) m |= (unsigned)(yv[j] > 0) << j;
  return m;
}

template <int NI>
__global__ __launch_bounds__(GN_THREADS) void gn_fwd_kernel(const uint16_t* __restrict__ x,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ beta,
                                                            const uint16_t* __restrict__ res,
                                                            uint16_t* __restrict__ y, uint8_t* __restrict__ mask_out,
                                                            float* __restrict__ mean_out,
                                                            float* __restrict__ rstd_out, int HW, int C, int cpg,
                                                            int relu, float eps) {
  __shared__ GnLds<double> s;
  const int t = threadIdx.x, cc = t & 7, r0 = t >> 3;
  const int slabs = C / GN_SLAB, n = blockIdx.x / slabs, slab = blockIdx.x % slabs;
  const int c0 = slab * GN_SLAB + cc * 8;            // this thread's first channel
  const long base = (long)n * HW * C + c0;           // ... of pixel row 0
  const int gps = GN_SLAB / cpg, G = C / cpg;        // groups per slab, per sample

  short8_t xr[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int row = r0 + GN_ROWS * i;
    xr[i] = row < HW ? ld8(x + base + (long)row * C) : zero8();
  }
  slab_stats<NI>(xr, HW, cpg, eps, s);
  if (t < gps) {  // the fp64 statistics rounded once, for the backward
    mean_out[(long)n * G + slab * gps + t] = (float)s.grp[0][t * cpg];
    rstd_out[(long)n * G + slab * gps + t] = (float)s.grp[1][t * cpg];
  }
  double mu[8], rs[8];
  float ga[8], be[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    mu[j] = s.grp[0][cc * 8 + j];
    rs[j] = s.grp[1][cc * 8 + j];
    ga[j] = gamma[c0 + j];
    be[j] = beta[c0 + j];
  }
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int row = r0 + GN_ROWS * i;
    if (row < HW) {
      const long off = base + (long)row * C;
      float f[8], r[8];
      unpack8(row_chunk(xr[i]), f);
      unpack8(res ? ld8(res + off) : zero8(), r);
#pragma unroll
      for (int j = 0; j < 8; ++j) {  // fp64 up to the one rounding to fp32 (then to bf16)
        const double d = gn_norm(f[j], mu[j], rs[j], ga[j], be[j]) + (double)r[j];
        f[j] = (float)(relu ? fmax(d, 0.0) : d);
      }
      const short8_t yv = pack8(f);
      *reinterpret_cast<short8_t*>(y + off) = yv;
      if (mask_out) mask_out[off >> 3] = (uint8_t)relu_bits(yv);
    }
  }
}

// mask_mode: 0 none, 1 the 1-bit image of y (ymask), 2 the sign of the recomputed relu(gn(x))
template <int NI>
__global__ __launch_bounds__(GN_THREADS) void gn_bwd_kernel(const uint16_t* __restrict__ dy,
                                                            const uint16_t* __restrict__ x,
                                                            const float* __restrict__ mean,
                                                            const float* __restrict__ rstd,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ beta,
                                                            const uint8_t* __restrict__ ymask, int mask_mode,
                                                            uint16_t* __restrict__ dz_out, uint16_t* __restrict__ dx,
                                                            float* __restrict__ ws, int HW, int C, int cpg,
                                                            float eps) {
  __shared__ GnLds<float> s;
  __shared__ GnLds<double> sd;  // mask_mode 2: the forward's fp64 statistics, rebuilt
  const int t = threadIdx.x, cc = t & 7, r0 = t >> 3;
  const int slabs = C / GN_SLAB, n = blockIdx.x / slabs, slab = blockIdx.x % slabs;
  const int c0 = slab * GN_SLAB + cc * 8;
  const long base = (long)n * HW * C + c0;
  const int gps = GN_SLAB / cpg, G = C / cpg;
  const float m = (float)HW * (float)cpg;

  float mu[8], rs[8], ga[8], be[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const long g = (long)n * G + (c0 + j) / cpg;
    mu[j] = mean[g];
    rs[j] = rstd[g];
    ga[j] = gamma[c0 + j];
    be[j] = mask_mode == 2 ? beta[c0 + j] : 0.f;
  }
  // the slab of x and of dz = dy * mask, both kept for the second pass
  short8_t xr[NI], dr[NI];
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int row = r0 + GN_ROWS * i;
    xr[i] = row < HW ? ld8(x + base + (long)row * C) : zero8();
  }
  double mud[8] = {}, rsd[8] = {};
  if (mask_mode == 2) {  // (the same for every thread of the grid)
    slab_stats<NI>(xr, HW, cpg, eps, sd);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      mud[j] = sd.grp[0][cc * 8 + j];
      rsd[j] = sd.grp[1][cc * 8 + j];
    }
  }
  float v[2][8];  // [0] sum dz xh (dgamma), [1] sum dz (dbeta)
#pragma unroll
  for (int j = 0; j < 8; ++j) v[0][j] = v[1][j] = 0.f;
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int row = r0 + GN_ROWS * i;
    dr[i] = zero8();
    if (row < HW) {
      const long off = base + (long)row * C;
      short8_t d = ld8(dy + off);
      float f[8], dz[8];
      unpack8(row_chunk(xr[i]), f);
      unsigned keep = 0xffu;
      if (mask_mode == 1) {
        keep = ymask[off >> 3];
      } else if (mask_mode == 2) {
        float a[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] = (float)fmax(gn_norm(f[j], mud[j], rsd[j], ga[j], be[j]), 0.0);
        keep = relu_bits(pack8(a));
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) d[j] = (keep >> j & 1) ? d[j] : (short)0;
      dr[i] = d;
      if (dz_out) *reinterpret_cast<short8_t*>(dz_out + off) = d;
      unpack8(d, dz);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        v[0][j] += dz[j] * ((f[j] - mu[j]) * rs[j]);
        v[1][j] += dz[j];
      }
    }
  }
  slab_reduce<2>(v, s);
  if (t < 2 * GN_SLAB) {  // this sample's row of partials: ws[n][0][C] dgamma, ws[n][1][C] dbeta
    const int q = t >> 6, c = t & 63;
    ws[((long)n * 2 + q) * C + slab * GN_SLAB + c] = s.ch[q][c];
  }
  if (t < gps) {
    float a = 0.f, b = 0.f;  // sum_g gamma dz, sum_g gamma dz xh
    for (int c = t * cpg; c < (t + 1) * cpg; ++c) {
      const float g = gamma[slab * GN_SLAB + c];
      a += g * s.ch[1][c];
      b += g * s.ch[0][c];
    }
    a /= m;
    b /= m;
    for (int c = t * cpg; c < (t + 1) * cpg; ++c) {
      s.grp[0][c] = a;
      s.grp[1][c] = b;
    }
  }
  __syncthreads();
  float k1[8], k2[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    k1[j] = s.grp[0][cc * 8 + j];
    k2[j] = s.grp[1][cc * 8 + j];
  }
#pragma unroll
  for (int i = 0; i < NI; ++i) {
    const int row = r0 + GN_ROWS * i;
    if (row < HW) {
      float f[8], dz[8];
      unpack8(row_chunk(xr[i]), f);
      unpack8(dr[i], dz);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float xh = (f[j] - mu[j]) * rs[j];
        f[j] = rs[j] * (ga[j] * dz[j] - k1[j] - xh * k2[j]);
      }
      *reinterpret_cast<short8_t*>(dx + base + (long)row * C) = pack8(f);
    }
  }
}

// g[c] += ((p_0 + p_1) + ...) + p_{N-1}, the rows in sample order
__global__ __launch_bounds__(256) void gn_param_fold_kernel(const float* __restrict__ ws, int N, int C,
                                                            float* __restrict__ grad_gamma,
                                                            float* __restrict__ grad_beta) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= 2 * C) return;
  const int q = t / C, c = t % C;
  float a = ws[(long)q * C + c];
  for (int n = 1; n < N; ++n) a += ws[((long)n * 2 + q) * C + c];
  float* g = q ? grad_beta : grad_gamma;
  g[c] += a;
}

// the shapes the split serves; cpg a power of two up to the slab
bool gn_shape_ok(int N, int HW, int C, int G) {
  if (N < 1 || HW < 1 || HW > GN_MAX_HW || C < GN_SLAB || C % GN_SLAB || G < 1 || C % G) return false;
  const int cpg = C / G;
  return cpg <= GN_SLAB && (cpg & (cpg - 1)) == 0;
}

}  // namespace

extern "C" {

// y [N][HW][C] = relu?(gn(x) (+ res)); mean / rstd [N][G]; mask_out (optional) N HW C / 8 bytes.
// Non-zero (nothing launched) for HW > 1024, C not a multiple of 64 or C / G not in 1, 2, .. 64.
int sl_gn_fwd(const uint16_t* x, const float* gamma, const float* beta, const uint16_t* res, uint16_t* y,
              uint8_t* mask_out, float* mean, float* rstd, int N, int HW, int C, int G, int relu, float eps,
              hipStream_t stream) {
  if (!gn_shape_ok(N, HW, C, G)) return -1;
  if (!x || !gamma || !beta || !y || !mean || !rstd) return -2;
  const dim3 grid((unsigned)((long)N * (C / GN_SLAB))), block(GN_THREADS);
  const int cpg = C / G;
#define SL_GN_FWD(NI) \
  hipLaunchKernelGGL(gn_fwd_kernel<NI>, grid, block, 0, stream, x, gamma, beta, res, y, mask_out, mean, rstd, HW, C, \
                     cpg, relu, eps)
  if (HW <= GN_ROWS) SL_GN_FWD(1);
  else if (HW <= 2 * GN_ROWS) SL_GN_FWD(2);
  else if (HW <= 8 * GN_ROWS) SL_GN_FWD(8);
  else SL_GN_FWD(32);
#undef SL_GN_FWD
  SL_CHECK_LAUNCH();
  return 0;
}

// dx (and optionally dz = dy * mask) of y = relu?(gn(x) (+ res)) from the forward's mean / rstd;
// mask_mode 0 none, 1 ymask (the forward's mask_out), 2 recomputed from x, gamma, beta, eps.
// ws [N][2][C]: each sample's per-channel dgamma, dbeta (sl_gn_param_fold adds them up).
int sl_gn_bwd(const uint16_t* dy, const uint16_t* x, const float* mean, const float* rstd, const float* gamma,
              const float* beta, const uint8_t* ymask, int mask_mode, uint16_t* dz_out, uint16_t* dx, float* ws,
              int N, int HW, int C, int G, float eps, hipStream_t stream) {
  if (!gn_shape_ok(N, HW, C, G) || mask_mode < 0 || mask_mode > 2) return -1;
  if (!dy || !x || !mean || !rstd || !gamma || !dx || !ws) return -2;
  if ((mask_mode == 1 && !ymask) || (mask_mode == 2 && !beta)) return -2;
  const dim3 grid((unsigned)((long)N * (C / GN_SLAB))), block(GN_THREADS);
  const int cpg = C / G;
#define SL_GN_BWD(NI) \
  hipLaunchKernelGGL(gn_bwd_kernel<NI>, grid, block, 0, stream, dy, x, mean, rstd, gamma, beta, ymask, mask_mode, \
                     dz_out, dx, ws, HW, C, cpg, eps)
  if (HW <= GN_ROWS) SL_GN_BWD(1);
  else if (HW <= 2 * GN_ROWS) SL_GN_BWD(2);
  else if (HW <= 8 * GN_ROWS) SL_GN_BWD(8);
  else SL_GN_BWD(32);
#undef SL_GN_BWD
  SL_CHECK_LAUNCH();
  return 0;
}

// grad_gamma[c] += sum_n ws[n][0][c], grad_beta[c] += sum_n ws[n][1][c], n in order
int sl_gn_param_fold(const float* ws, int N, int C, float* grad_gamma, float* grad_beta, hipStream_t stream) {
  if (N < 1 || C < 1 || !ws || !grad_gamma || !grad_beta) return -1;
  hipLaunchKernelGGL(gn_param_fold_kernel, dim3((2 * C + 255) / 256), dim3(256), 0, stream, ws, N, C, grad_gamma,
                     grad_beta);
  SL_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"

// Weight standardization for the ResNet trainers (weight_std=True): every convolution filter is
// re-centred and re-scaled over its fan-in on the way from the fp32 master weights to the bf16
// shadow the convolutions read, and the weight gradient is taken back through that map.
//
// A conv bank is W[m = cout][n = k k cin], stored [cout][k][k][cin]; column j is real when
// j % cin < cin_real (only the stem has padding columns: cin 8, cin_real 3), R real columns a row.
//
//   forward   mu = mean_real(w), var = mean_real((w - mu)^2), r = 1 / sqrt(var + eps),
//             what_j = (w_j - mu) r on real columns and exactly 0 on padding; shadow = bf16(what)
//   backward  G = dL/dwhat (what conv_wgrad left in the flat gradient), a = mean_real(G),
//             b = mean_real(G what): dL/dw_j = r (G_j - a - what_j b), 0 on padding, over G in place
//             (the bf16 rounding is the identity to the backward; what is the unrounded value)
//
// Work split.  Each direction is ONE grouped launch over all banks.  A 256-thread workgroup is four
// waves and one wave owns one filter row, held in registers: lane l of round k holds float4 number
// l + 64 k of the row, so a wave's load is 1 KB contiguous and a round is predicated on
// 4 (l + 64 k) < n (n % 4 == 0: no scalar tail).  Rounds per lane are NV = ceil(n / 256) <= 18; the
// body is instantiated for 1, 3, 5, 9 and 18 and a wave-uniform switch on the bank's n picks one,
// so the register arrays index statically and all of a row's loads are issued before the first
// use.  A work table maps each workgroup to (bank, first row), the longest rows first, so the
// grid's tail is the short rows.  No LDS, no barrier, no atomics, no state between calls: the sums
// of a row cross lanes by xor shuffles only (two in the forward, two more in the backward).  The
// backward holds the w row and the G row (36 float4 a lane at n = 4608) and rebuilds mu and r with
// the forward's own code, so no stale statistic can reach it.
//
// Arithmetic is fp64, as in gn_fwd: the kernels are bound by their bytes.  A lane sums its elements
// in round order, x y z w within a float4, then the xor shuffles run over 1, 2, .. 32: a fixed
// order, the same bits from call to call and in both builds.  The variance is a second pass over
// the registers' deviations, not E[x^2] - mu^2.  what is formed in fp64 and rounded once to fp32,
// then to bf16.  A constant row has mu = w exactly (R w and its partial sums are exact in fp64), so
// its what is exactly 0.
#include "common.h"

using namespace sl;

namespace {

constexpr int WS_THREADS = 256;
constexpr int WS_WAVES = WS_THREADS / 64;  // rows per workgroup
constexpr int WS_MAX_N = 4608;             // 18 rounds of 64 float4
constexpr int WS_FIELDS = 8;               // ints per bank of the tensor table

// one bank of the plan's tensor table (ops/cnn.py wstd_plan): off in elements of the flat vector,
// row0 the bank's first row in plan order (where its rows' statistics go)
struct WsTensor {
  int off, rows, n, cin, cin_real, row0, pad0, pad1;
};
static_assert(sizeof(WsTensor) == WS_FIELDS * sizeof(int), "ops/cnn.py WSTD_FIELDS");

// A float4 of the row as the optimiser cannot relate it to its register (groupnorm.hip's device):
// left to itself the compiler keeps the fp64-widened row from one pass to the next and spills.
__device__ __forceinline__ floatx4_t row_chunk(floatx4_t c) {
  asm volatile("" : "+v"(c));
  return c;
}

__device__ __forceinline__ double wave_sum(double a) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) a += __shfl_xor(a, m);
  return a;
}

// bit e = element j0 + e of the row exists and is a real column.  The column test runs only for a
// bank with padding (pad: wave-uniform).
__device__ __forceinline__ unsigned real4(int j0, const WsTensor& t, bool pad) {
  if (j0 >= t.n) return 0u;
  if (!pad) return 0xfu;
  unsigned m = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) m |= (unsigned)((j0 + e) % t.cin < t.cin_real) << e;
  return m;
}

template <int NV>
__device__ __forceinline__ void load_row(const float* __restrict__ p, int n, int lane, floatx4_t (&x)[NV]) {
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int j0 = 4 * (lane + 64 * k);
    x[k] = j0 < n ? *reinterpret_cast<const floatx4_t*>(p + j0) : zero4();
  }
}

// mu and r of the row in x, one definition for both directions.  Two passes: sum, then squared deviations.
template <int NV>
__device__ __forceinline__ void row_stats(const floatx4_t (&x)[NV], const WsTensor& t, bool pad, int lane, double eps,
                                          double& mu, double& r) {
  const double R = (double)(t.n / t.cin * t.cin_real);
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const floatx4_t c = row_chunk(x[k]);
    const unsigned m = real4(4 * (lane + 64 * k), t, pad);
#pragma unroll
    for (int e = 0; e < 4; ++e) s += (m >> e & 1) ? (double)c[e] : 0.0;
  }
  mu = wave_sum(s) / R;
  double v = 0.0;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const floatx4_t c = row_chunk(x[k]);
    const unsigned m = real4(4 * (lane + 64 * k), t, pad);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const double d = (m >> e & 1) ? (double)c[e] - mu : 0.0;
      v = fma(d, d, v);
    }
  }
  r = 1.0 / sqrt(wave_sum(v) / R + eps);
}

template <int NV>
__device__ __forceinline__ void fwd_row(const float* __restrict__ w, uint16_t* __restrict__ sh, float* stat,
                                        const WsTensor& t, int lane, double eps) {
  floatx4_t x[NV];
  load_row<NV>(w, t.n, lane, x);
  const bool pad = t.cin_real != t.cin;
  double mu, r;
  row_stats<NV>(x, t, pad, lane, eps, mu, r);
  if (stat && lane == 0) *reinterpret_cast<float2*>(stat) = make_float2((float)mu, (float)r);
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int j0 = 4 * (lane + 64 * k);
    if (j0 < t.n) {
      const floatx4_t c = row_chunk(x[k]);
      const unsigned m = real4(j0, t, pad);
      float f[4];
#pragma unroll
      for (int e = 0; e < 4; ++e)  // fp64 up to the one rounding to fp32 (then to bf16)
        f[e] = (m >> e & 1) ? (float)(((double)c[e] - mu) * r) : 0.f;
      *reinterpret_cast<uint2*>(sh + j0) = make_uint2(pack2(f[0], f[1]), pack2(f[2], f[3]));
    }
  }
}

template <int NV>
__device__ __forceinline__ void bwd_row(const float* __restrict__ w, float* __restrict__ g, const WsTensor& t,
                                        int lane, double eps) {
  floatx4_t x[NV], d[NV];
  load_row<NV>(w, t.n, lane, x);
  load_row<NV>(g, t.n, lane, d);
  const bool pad = t.cin_real != t.cin;
  double mu, r;
  row_stats<NV>(x, t, pad, lane, eps, mu, r);
  const double R = (double)(t.n / t.cin * t.cin_real);
  double sa = 0.0, sb = 0.0;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const floatx4_t c = row_chunk(x[k]), gc = row_chunk(d[k]);
    const unsigned m = real4(4 * (lane + 64 * k), t, pad);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const double ge = (m >> e & 1) ? (double)gc[e] : 0.0;
      sa += ge;
      sb = fma(ge, ((double)c[e] - mu) * r, sb);
    }
  }
  const double a = wave_sum(sa) / R, b = wave_sum(sb) / R;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int j0 = 4 * (lane + 64 * k);
    if (j0 < t.n) {
      const floatx4_t c = row_chunk(x[k]), gc = row_chunk(d[k]);
      const unsigned m = real4(j0, t, pad);
      floatx4_t o;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double wh = ((double)c[e] - mu) * r;
        o[e] = (m >> e & 1) ? (float)(r * (((double)gc[e] - a) - wh * b)) : 0.f;
      }
      *reinterpret_cast<floatx4_t*>(g + j0) = o;
    }
  }
}

// the instantiation that serves rows of n elements (n is the same for a whole workgroup)
#define WS_DISPATCH(BODY)        \
  do {                           \
    if (t.n <= 256) BODY(1);     \
    else if (t.n <= 768) BODY(3);  \
    else if (t.n <= 1280) BODY(5); \
    else if (t.n <= 2304) BODY(9); \
    else BODY(18);               \
  } while (0)

__global__ __launch_bounds__(WS_THREADS) void wstd_fwd_kernel(const float* __restrict__ w,
                                                              uint16_t* __restrict__ shadow,
                                                              float* __restrict__ stats,
                                                              const WsTensor* __restrict__ tensors,
                                                              const int2* __restrict__ work, double eps) {
  const int2 wk = work[blockIdx.x];
  const WsTensor t = tensors[wk.x];
  const int lane = threadIdx.x & 63, row = wk.y + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (row >= t.rows) return;  // (a bank's last workgroup may be partial; nothing follows but the end)
  const long base = (long)t.off + (long)row * t.n;
  float* st = stats ? stats + 2 * (long)(t.row0 + row) : nullptr;
#define WS_FWD(NV) fwd_row<NV>(w + base, shadow + base, st, t, lane, eps)
  WS_DISPATCH(WS_FWD);
#undef WS_FWD
}

__global__ __launch_bounds__(WS_THREADS) void wstd_bwd_kernel(const float* __restrict__ w, float* __restrict__ grad,
                                                              const WsTensor* __restrict__ tensors,
                                                              const int2* __restrict__ work, double eps) {
  const int2 wk = work[blockIdx.x];
  const WsTensor t = tensors[wk.x];
  const int lane = threadIdx.x & 63, row = wk.y + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (row >= t.rows) return;
  const long base = (long)t.off + (long)row * t.n;
#define WS_BWD(NV) bwd_row<NV>(w + base, grad + base, t, lane, eps)
  WS_DISPATCH(WS_BWD);
#undef WS_BWD
}

// The plan as the launchers accept it, checked on its host copy: every bank inside [0, total) with
// n % 4 == 0, 4 <= n <= 4608 and an offset on a 16-byte boundary of the fp32 vector (so of 8 bytes
// of the bf16 one), its rows numbered in plan order; every work item a bank's row block.
bool wstd_plan_ok(const int* tensors_h, int T, const int* work_h, int n_work, long total) {
  if (!tensors_h || !work_h || T < 1 || n_work < 1 || total < 1) return false;
  const WsTensor* ts = reinterpret_cast<const WsTensor*>(tensors_h);
  long rows = 0;
  for (int i = 0; i < T; ++i) {
    const WsTensor& t = ts[i];
    if (t.n < 4 || t.n > WS_MAX_N || t.n % 4 || t.rows < 1 || t.off < 0 || t.off % 4) return false;
    if (t.cin < 1 || t.cin_real < 1 || t.cin_real > t.cin || t.n % t.cin || t.row0 != rows) return false;
    if ((long)t.off + (long)t.rows * t.n > total) return false;
    rows += t.rows;
  }
  for (int i = 0; i < n_work; ++i) {
    const int b = work_h[2 * i], r = work_h[2 * i + 1];
    if (b < 0 || b >= T || r < 0 || r >= ts[b].rows || r % WS_WAVES) return false;
  }
  return true;
}

bool ws_aligned(const void* p, unsigned mask) { return p && ((uintptr_t)p & mask) == 0; }

}  // namespace

extern "C" {

// shadow[bank] = bf16(standardized w[bank]) for every bank of the plan, zeros on padding columns;
// stats_out (optional): (float mu, float r) of every row in plan order.  w / shadow: the flat fp32
// vector and its bf16 image, `total` elements.  tensors_h / tensors: the int32 [T][8] table
// (offset, rows, n, cin, cin_real, first row, 0, 0) on the host and on the device; work_h / work:
// int32 [n_work][2] = (bank, first row), four rows each.  Non-zero, with nothing launched, for
// n % 4 != 0, n > 4608, n < 4, an offset that is not 16-byte aligned, a bank beyond `total`, or a
// null pointer.
int sl_wstd_fwd(const float* w, uint16_t* shadow, float* stats_out, long total, const int* tensors_h,
                const int* tensors, int T, const int* work_h, const int* work, int n_work, double eps,
                hipStream_t stream) {
  if (!ws_aligned(w, 15) || !ws_aligned(shadow, 7) || (stats_out && ((uintptr_t)stats_out & 7))) return -2;
  if (!ws_aligned(tensors, 3) || !ws_aligned(work, 7) || !(eps > 0.0)) return -2;
  if (!wstd_plan_ok(tensors_h, T, work_h, n_work, total)) return -1;
  hipLaunchKernelGGL(wstd_fwd_kernel, dim3(n_work), dim3(WS_THREADS), 0, stream, w, shadow, stats_out,
                     reinterpret_cast<const WsTensor*>(tensors), reinterpret_cast<const int2*>(work), eps);
  SL_CHECK_LAUNCH();
  return 0;
}

// grad[bank] = dL/dw from grad[bank] = dL/dwhat, in place, for every bank of the plan (0 on padding
// columns); the statistics are rebuilt from w.  Arguments and refusals as sl_wstd_fwd's.
int sl_wstd_bwd(const float* w, float* grad, long total, const int* tensors_h, const int* tensors, int T,
                const int* work_h, const int* work, int n_work, double eps, hipStream_t stream) {
  if (!ws_aligned(w, 15) || !ws_aligned(grad, 15) || w == grad) return -2;
  if (!ws_aligned(tensors, 3) || !ws_aligned(work, 7) || !(eps > 0.0)) return -2;
  if (!wstd_plan_ok(tensors_h, T, work_h, n_work, total)) return -1;
  hipLaunchKernelGGL(wstd_bwd_kernel, dim3(n_work), dim3(WS_THREADS), 0, stream, w, grad,
                     reinterpret_cast<const WsTensor*>(tensors), reinterpret_cast<const int2*>(work), eps);
  SL_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"

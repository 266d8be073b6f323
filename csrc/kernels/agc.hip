// Adaptive gradient clipping (Brock et al. 2021) for the ResNet trainers (agc_clip > 0): every unit
// of the flat gradient -- one filter row W[co][k k cin] of a conv bank, or one whole norm scale /
// shift vector -- is clipped against the norm of the same unit of the fp32 master weights:
//     wn = ||w_u||, gn = ||g_u|| over the real columns (j % cin < cin_real; only the stem pads),
//     t = clip max(wn, eps);   gn > t:  g_u *= float(t / gn), padding columns included
// and a unit that is not clipped (gn <= t, gn = 0, or either norm NaN) is not written at all.
// Semantics and the host-side plan: serverless_learn_amd/ops/optim.py agc_clip_reference / agc_plan.
//
// Work split.  ONE grouped launch over all units.  A 256-thread workgroup is four waves and one wave
// owns one unit; the unit table is sorted longest first, so the grid's tail is the short units, and
// the work table gives each workgroup (first unit, unit count): the waves past the count exit before
// any shuffle.  Waves of one workgroup may own units of different lengths; each picks its own body.
//
// Data movement.  Lane l of round k holds float4 number l + 64 k of the unit, a round predicated on
// 4 (l + 64 k) < n (n % 4 == 0), NV = ceil(n / 256) <= 18 rounds, instantiated for 1, 3, 5, 9 and 18
// so the register arrays index statically.  All 2 NV 16-byte loads, the g row's and the w row's, are
// issued before the first use: both streams are in flight together.  The w row is only passed
// through: its registers are dead once its norm is folded.  The g row stays in registers from its
// load to its store, so a clipped unit costs one read and one write of g and an unclipped one a
// read alone: at a usual clip most of the launch is read-only.  No LDS, no barrier, no atomics, no
// tickets, no state between calls.
//
// Norms.  Two passes over the registers, so that a row at either end of the fp32 range has the norm
// its elements have: (a) amax = max |x| over the real columns, taken as an unsigned maximum of the
// sign-less bit patterns (exact, subnormals included, and a NaN pattern is above Inf's, so a NaN
// wins); (b) the fp64 sum of (x r)^2 with r = 1 / amax, formed once per wave (0 where amax is 0, Inf
// or NaN: no division by 0, and an Inf or NaN element times 0 is NaN); (c) norm = amax sqrt(sum).
// A row of zeros has norm 0; a row holding an Inf or a NaN has a NaN norm and fails gn > t, so it
// is left alone (a squared norm of +Inf would have been "clipped" by a factor 0).  A lane sums its
// elements in round order, x y z w within a float4, each term one explicit fma; both folds are xor
// butterflies over 1, 2, .. 32, so every lane ends with the same bits, the decision and the factor
// are wave-uniform, and the result is the same from call to call and in both builds.
#include "common.h"

using namespace sl;

namespace {

constexpr int AGC_THREADS = 256;
constexpr int AGC_WAVES = AGC_THREADS / 64;  // units per workgroup (ops/optim.py AGC_UNITS_PER_WG)
constexpr int AGC_MAX_N = 4608;              // 18 rounds of 64 float4

// one unit of the plan's table (ops/optim.py agc_plan): off in elements of the flat vector; a 1-D
// unit has cin = cin_real = n
struct AgcUnit {
  int off, n, cin, cin_real;
};
static_assert(sizeof(AgcUnit) == sizeof(int4), "ops/optim.py AGC_FIELDS");

// (weight_std.hip's device: the optimiser must not keep an fp64-widened row between the passes)
__device__ __forceinline__ floatx4_t agc_chunk(floatx4_t c) {
  asm volatile("" : "+v"(c));
  return c;
}

__device__ __forceinline__ unsigned wave_umax(unsigned a) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    const unsigned b = (unsigned)__shfl_xor((int)a, m);
    a = a > b ? a : b;
  }
  return a;
}

__device__ __forceinline__ double wave_dsum(double a) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) a += __shfl_xor(a, m);
  return a;
}

// bit e = element j0 + e of the unit exists and is a real column (pad: wave-uniform, the stem only)
__device__ __forceinline__ unsigned agc_real4(int j0, const AgcUnit& u, bool pad) {
  if (j0 >= u.n) return 0u;
  if (!pad) return 0xfu;
  unsigned m = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) m |= (unsigned)((j0 + e) % u.cin < u.cin_real) << e;
  return m;
}

template <int NV>
__device__ __forceinline__ void agc_load(const float* __restrict__ p, int n, int lane, floatx4_t (&x)[NV]) {
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int j0 = 4 * (lane + 64 * k);
    x[k] = j0 < n ? *reinterpret_cast<const floatx4_t*>(p + j0) : zero4();
  }
}

// ||x|| over the real columns of the row in x, in fp64: the two passes of the header
template <int NV>
__device__ __forceinline__ double agc_norm(const floatx4_t (&x)[NV], const AgcUnit& u, bool pad, int lane) {
  unsigned top = 0;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const floatx4_t c = agc_chunk(x[k]);
    const unsigned m = agc_real4(4 * (lane + 64 * k), u, pad);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const unsigned b = (m >> e & 1) ? __float_as_uint(c[e]) & 0x7fffffffu : 0u;
      top = top > b ? top : b;
    }
  }
  const double amax = (double)__uint_as_float(wave_umax(top));
  const double r = (amax > 0.0 && amax < HUGE_VAL) ? 1.0 / amax : 0.0;  // (a NaN fails both tests)
  double s = 0.0;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const floatx4_t c = agc_chunk(x[k]);
    const unsigned m = agc_real4(4 * (lane + 64 * k), u, pad);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const double q = (m >> e & 1) ? (double)c[e] * r : 0.0;
      s = fma(q, q, s);
    }
  }
  return amax * sqrt(wave_dsum(s));
}

template <int NV>
__device__ __forceinline__ void agc_unit(const float* __restrict__ w, float* __restrict__ g, float* __restrict__ stat,
                                         const AgcUnit& u, int lane, double clip, double eps) {
  floatx4_t gv[NV], wv[NV];
  agc_load<NV>(g, u.n, lane, gv);
  agc_load<NV>(w, u.n, lane, wv);
  const bool pad = u.cin_real != u.cin;
  const double wn = agc_norm<NV>(wv, u, pad, lane);
  const double gn = agc_norm<NV>(gv, u, pad, lane);
  const double t = clip * (wn < eps ? eps : wn);  // (a NaN wn stays: t is NaN and nothing is clipped)
  const bool clipped = gn > t;
  const float s = clipped ? (float)(t / gn) : 1.f;
  if (lane == 0) {
    stat[0] = (float)wn;
    stat[1] = (float)gn;
    stat[2] = s;
  }
  if (!clipped) return;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const int j0 = 4 * (lane + 64 * k);
    if (j0 < u.n) *reinterpret_cast<floatx4_t*>(g + j0) = gv[k] * s;
  }
}

__global__ __launch_bounds__(AGC_THREADS) void agc_clip_kernel(const float* __restrict__ w, float* __restrict__ g,
                                                               const AgcUnit* __restrict__ units,
                                                               const int2* __restrict__ work,
                                                               float* __restrict__ stats, double clip, double eps) {
  const int2 wk = work[blockIdx.x];  // (first unit, units)
  const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (wave >= wk.y) return;  // (a tail workgroup's idle waves: before any shuffle)
  const int i = wk.x + wave;
  const AgcUnit u = units[i];
  float* st = stats + 3 * (long)i;
#define AGC_BODY(NV) agc_unit<NV>(w + u.off, g + u.off, st, u, lane, clip, eps)
  if (u.n <= 256) AGC_BODY(1);
  else if (u.n <= 768) AGC_BODY(3);
  else if (u.n <= 1280) AGC_BODY(5);
  else if (u.n <= 2304) AGC_BODY(9);
  else AGC_BODY(18);
#undef AGC_BODY
}

// The plan as the launcher accepts it, checked on its host copy: every unit inside [0, total) with
// n % 4 == 0, 4 <= n <= 4608 and an offset on a 16-byte boundary; every work item 1 .. 4 units of
// the table.
bool agc_plan_ok(const int* units_h, int n_units, const int* work_h, int n_work, long total) {
  if (!units_h || !work_h || n_units < 1 || n_work < 1 || total < 1) return false;
  const AgcUnit* us = reinterpret_cast<const AgcUnit*>(units_h);
  for (int i = 0; i < n_units; ++i) {
    const AgcUnit& u = us[i];
    if (u.n < 4 || u.n > AGC_MAX_N || u.n % 4 || u.off < 0 || u.off % 4) return false;
    if (u.cin < 1 || u.cin_real < 1 || u.cin_real > u.cin || u.n % u.cin) return false;
    if ((long)u.off + u.n > total) return false;
  }
  for (int i = 0; i < n_work; ++i) {
    const int first = work_h[2 * i], count = work_h[2 * i + 1];
    if (first < 0 || count < 1 || count > AGC_WAVES || (long)first + count > n_units) return false;
  }
  return true;
}

bool agc_aligned(const void* p, unsigned mask) { return p && ((uintptr_t)p & mask) == 0; }

}  // namespace

extern "C" {

// Adaptive gradient clipping of grad against w, in place, for every unit of the plan; stats[u] =
// (float wn, float gn, the factor or 1.0f) in plan order, rewritten whole by every call.  w / grad:
// the flat fp32 vectors, `total` elements.  units_h / units: the int32 [n_units][4] table (offset,
// n, cin, cin_real) on the host and on the device; work_h / work: int32 [n_work][2] = (first unit,
// unit count <= 4).  The units must not overlap (the caller's plan).  Non-zero, with nothing
// launched, for n % 4 != 0, n > 4608, n < 4, an offset that is not 16-byte aligned, a unit beyond
// `total`, cin_real > cin, n % cin != 0, a null pointer, or clip / eps not finite and > 0.
int sl_agc_clip(const float* w, float* grad, long total, const int* units_h, const int* units, int n_units,
                const int* work_h, const int* work, int n_work, double clip, double eps, float* stats,
                hipStream_t stream) {
  if (!agc_aligned(w, 15) || !agc_aligned(grad, 15) || w == grad || !agc_aligned(stats, 3)) return -2;
  if (!agc_aligned(units, 15) || !agc_aligned(work, 7)) return -2;
  if (!(clip > 0.0 && clip < HUGE_VAL) || !(eps > 0.0 && eps < HUGE_VAL)) return -2;  // (NaN fails every comparison)
  if (!agc_plan_ok(units_h, n_units, work_h, n_work, total)) return -1;
  hipLaunchKernelGGL(agc_clip_kernel, dim3(n_work), dim3(AGC_THREADS), 0, stream, w, grad,
                     reinterpret_cast<const AgcUnit*>(units), reinterpret_cast<const int2*>(work), stats, clip, eps);
  SL_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"

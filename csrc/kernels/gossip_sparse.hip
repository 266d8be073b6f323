// Top-k sparse gossip: exact on-device selection of the k largest |m - o| and the sparse
// apply (parallel/gossip.py make_sparse_delta / absorb_sparse / unsend).
//
// d_i = float(double(m_i) - double(o_i)); the order is by key_i = bits(d_i) & 0x7fffffff as
// uint32, larger first, equal keys to the lower index; key 0 (d = +-0) is never selected.
//
// sl_gossip_topk is a 3-digit (11 + 10 + 10 bit) radix select followed by an ordered
// compaction, every step a launch of its own so that the kernel boundary is the only
// cross-workgroup ordering there is:
//   hist<0>  d -> workspace (4 B per element for every later pass), histogram of key >> 20
//   pick     one workgroup: the bin in which the k-th largest key lies, k reduced by the keys above
//   hist<1>, pick, hist<2>, pick   the same on the next digits of the keys that share the prefix
//            -> threshold key T, need_eq = how many keys equal to T are admitted, count
//   count    per workgroup: keys > T and keys == T in its contiguous chunk
//   scatter  each workgroup sums the counts of the workgroups before it (fixed order), scans its
//            chunk tile by tile and writes (index, d) at
//                pos = #above before i + min(#equal before i, need_eq)
//            which is ascending in i and admits the lowest-index ties; o[i] += d there.
// Histograms use integer atomics only (exact in any order); there is no float atomic, so the
// bytes written do not depend on grid size, timing or the build (default / deterministic).
#include "common.h"

namespace {

constexpr int TPB = 256;
constexpr int VEC = 4;
constexpr int TILE = TPB * VEC;
constexpr int WAVES = TPB / 64;
constexpr int MAX_WGS = 1024;
constexpr int MAX_BINS = 2048;
constexpr uint32_t KEY_MASK = 0x7fffffffu;

struct SelState {
  uint32_t prefix;   // digits of T found so far (in place)
  uint32_t krem;     // keys still to take from the bins at and below the prefix
  uint32_t need_eq;  // final: keys equal to T admitted (0 when T == 0)
  uint32_t count;    // final: entries written
};

// workspace, in 4-byte words: d[n rounded up to 4] | SelState | hist[3][MAX_BINS] | wg counts [MAX_WGS][2]
constexpr long CTRL_WORDS = 4;
constexpr long HIST_WORDS = 3L * MAX_BINS;
constexpr long WGC_WORDS = 2L * MAX_WGS;
__host__ __device__ constexpr long d_words(long n) { return (n + 3) & ~3L; }

__device__ __forceinline__ int digit_shift(int pass) { return pass == 0 ? 20 : (pass == 1 ? 10 : 0); }
__device__ __forceinline__ int digit_bins(int pass) { return pass == 0 ? 2048 : 1024; }

// 4 consecutive floats at p[i..i+3]; 16-byte load when `vec` (p 16-byte aligned; i is a multiple of 4)
// and the tile is whole, scalar with zeros past n otherwise
__device__ __forceinline__ void load4(const float* __restrict__ p, long i, long n, bool vec, float v[VEC]) {
  if (vec && i + VEC <= n) {
    const float4 t = *reinterpret_cast<const float4*>(p + i);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
#pragma unroll
    for (int j = 0; j < VEC; ++j) v[j] = (i + j < n) ? p[i + j] : 0.f;
  }
}

template <int PASS>
__global__ __launch_bounds__(TPB) void topk_hist_kernel(const float* __restrict__ m, const float* __restrict__ o,
                                                        float* __restrict__ d, const SelState* __restrict__ st,
                                                        uint32_t* __restrict__ hist, long n, long chunk, int vec_mo) {
  __shared__ uint32_t h[WAVES][MAX_BINS];  // one private histogram per wave
  constexpr int shift = PASS == 0 ? 20 : (PASS == 1 ? 10 : 0);
  constexpr int bins = PASS == 0 ? 2048 : 1024;
  for (int b = threadIdx.x; b < WAVES * MAX_BINS; b += TPB) (&h[0][0])[b] = 0;
  __syncthreads();
  const uint32_t prefix = PASS == 0 ? 0u : st->prefix;
  uint32_t* hw = h[threadIdx.x >> 6];
  const long lo = (long)blockIdx.x * chunk;
  const long hi = lo + chunk < n ? lo + chunk : n;
  for (long i = lo + (long)threadIdx.x * VEC; i < hi; i += TILE) {
    float dv[VEC];
    if (PASS == 0) {
      float mv[VEC], ov[VEC];
      load4(m, i, n, vec_mo != 0, mv);
      load4(o, i, n, vec_mo != 0, ov);
#pragma unroll
      for (int j = 0; j < VEC; ++j) dv[j] = (float)((double)mv[j] - (double)ov[j]);
      if (i + VEC <= n) {
        *reinterpret_cast<float4*>(d + i) = make_float4(dv[0], dv[1], dv[2], dv[3]);
      } else {
#pragma unroll
        for (int j = 0; j < VEC; ++j)
          if (i + j < n) d[i + j] = dv[j];
      }
    } else {
      load4(d, i, n, true, dv);
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      if (i + j >= n) continue;
      const uint32_t key = __float_as_uint(dv[j]) & KEY_MASK;
      // the digits above this pass's must equal the prefix (shift + 10/11 <= 31: no 32-bit shift)
      if (PASS != 0 && (key >> (shift + 10)) != (prefix >> (shift + 10))) continue;
      atomicAdd(&hw[(key >> shift) & (bins - 1)], 1u);
    }
  }
  __syncthreads();
  for (int b = threadIdx.x; b < bins; b += TPB) {
    uint32_t s = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) s += h[w][b];
    if (s) atomicAdd(&hist[b], s);
  }
}

// One workgroup.  Bins are walked from the top: thread t owns `per` bins, bins - 1 - t*per downwards.
__global__ __launch_bounds__(TPB) void topk_pick_kernel(SelState* __restrict__ st, const uint32_t* __restrict__ hist,
                                                        int pass, uint32_t k, uint32_t* __restrict__ count_out) {
  __shared__ uint32_t scan[2][TPB];
  const int bins = digit_bins(pass), shift = digit_shift(pass), per = bins / TPB;
  const int t = threadIdx.x;
  const uint32_t krem = pass == 0 ? k : st->krem;
  const uint32_t prefix = pass == 0 ? 0u : st->prefix;
  uint32_t own = 0;
  for (int j = 0; j < per; ++j) own += hist[bins - 1 - (t * per + j)];
  // inclusive scan over the threads (Hillis-Steele, double buffered)
  int cur = 0;
  scan[0][t] = own;
  __syncthreads();
  for (int off = 1; off < TPB; off <<= 1) {
    uint32_t v = scan[cur][t];
    if (t >= off) v += scan[cur][t - off];
    scan[cur ^ 1][t] = v;
    cur ^= 1;
    __syncthreads();
  }
  uint32_t above = scan[cur][t] - own;  // keys in the bins above this thread's
  // exactly one thread holds the crossing: above < krem <= above + own (the pass's keys number >= krem)
  if (above < krem && krem <= above + own) {
    for (int j = 0; j < per; ++j) {
      const int b = bins - 1 - (t * per + j);
      const uint32_t c = hist[b];
      if (krem <= above + c) {
        const uint32_t T = prefix | ((uint32_t)b << shift);
        const uint32_t rem = krem - above;  // 1 <= rem <= c
        st->prefix = T;
        st->krem = rem;
        if (pass == 2) {
          st->need_eq = T ? rem : 0u;      // T == 0: fewer than k non-zero deltas, zeros are dropped
          st->count = T ? k : k - rem;
          *count_out = st->count;
        }
        break;
      }
      above += c;
    }
  }
}

__global__ __launch_bounds__(TPB) void topk_count_kernel(const float* __restrict__ d, const SelState* __restrict__ st,
                                                         uint32_t* __restrict__ wgc, long n, long chunk) {
  __shared__ uint32_t red[2][WAVES];
  const uint32_t T = st->prefix;
  const long lo = (long)blockIdx.x * chunk;
  const long hi = lo + chunk < n ? lo + chunk : n;
  uint32_t na = 0, ne = 0;
  for (long i = lo + (long)threadIdx.x * VEC; i < hi; i += TILE) {
    float dv[VEC];
    load4(d, i, n, true, dv);
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      if (i + j >= n) continue;
      const uint32_t key = __float_as_uint(dv[j]) & KEY_MASK;
      na += key > T;
      ne += key == T;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    na += __shfl_down(na, off, 64);
    ne += __shfl_down(ne, off, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = na;
    red[1][threadIdx.x >> 6] = ne;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t a = 0, e = 0;
    for (int w = 0; w < WAVES; ++w) { a += red[0][w]; e += red[1][w]; }
    wgc[2 * blockIdx.x] = a;
    wgc[2 * blockIdx.x + 1] = e;
  }
}

__global__ __launch_bounds__(TPB) void topk_scatter_kernel(const float* __restrict__ d, float* __restrict__ o,
                                                           const SelState* __restrict__ st,
                                                           const uint32_t* __restrict__ wgc,
                                                           uint32_t* __restrict__ index_out,
                                                           float* __restrict__ value_out, long n, long chunk,
                                                           uint32_t k) {
  __shared__ uint32_t red[2][WAVES];
  __shared__ uint32_t wsum[2][WAVES];  // per-wave tile totals (above | equal << 16), double buffered
  const uint32_t T = st->prefix, need_eq = st->need_eq;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  // keys above / equal to T in the workgroups before this one
  uint32_t pa = 0, pe = 0;
  for (int j = threadIdx.x; j < (int)blockIdx.x; j += TPB) {
    pa += wgc[2 * j];
    pe += wgc[2 * j + 1];
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    pa += __shfl_down(pa, off, 64);
    pe += __shfl_down(pe, off, 64);
  }
  if (lane == 0) {
    red[0][wave] = pa;
    red[1][wave] = pe;
  }
  __syncthreads();
  uint32_t run_a = 0, run_e = 0;
  for (int w = 0; w < WAVES; ++w) { run_a += red[0][w]; run_e += red[1][w]; }

  const long lo = (long)blockIdx.x * chunk;
  const long hi = lo + chunk < n ? lo + chunk : n;
  int buf = 0;
  for (long base = lo; base < hi; base += TILE, buf ^= 1) {  // uniform trip count: barriers inside
    const long i = base + (long)threadIdx.x * VEC;
    float dv[VEC];
    load4(d, i, n, true, dv);
    uint32_t fa = 0, fe = 0;  // bit j: element j is above / equal
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      if (i + j >= n) continue;
      const uint32_t key = __float_as_uint(dv[j]) & KEY_MASK;
      fa |= (uint32_t)(key > T) << j;
      fe |= (uint32_t)(key == T) << j;
    }
    const uint32_t own = (uint32_t)__popc(fa) | ((uint32_t)__popc(fe) << 16);  // <= 1024 each per tile
    uint32_t inc = own;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const uint32_t v = __shfl_up(inc, off, 64);
      if (lane >= off) inc += v;
    }
    if (lane == 63) wsum[buf][wave] = inc;
    __syncthreads();
    uint32_t before = inc - own, total = 0;
    for (int w = 0; w < WAVES; ++w) {
      const uint32_t s = wsum[buf][w];
      if (w < wave) before += s;
      total += s;
    }
    uint32_t a_before = run_a + (before & 0xffffu), e_before = run_e + (before >> 16);
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      const bool is_a = (fa >> j) & 1u, is_e = (fe >> j) & 1u;
      if (is_a || (is_e && e_before < need_eq)) {
        const uint32_t pos = a_before + (e_before < need_eq ? e_before : need_eq);
        if (pos < k) {  // always true for consistent counts; never write past the k-entry outputs
          index_out[pos] = (uint32_t)(i + j);
          value_out[pos] = dv[j];
          o[i + j] = (float)((double)o[i + j] + (double)dv[j]);
        }
      }
      a_before += is_a;
      e_before += is_e;
    }
    run_a += total & 0xffffu;
    run_e += total >> 16;
  }
}

// absorb_sparse: m[i] += a*v, o[i] += a*v.   sign_o_only != 0 (unsend: -1): o[i] += sign*v only.
// Products and sums are rounded one by one (no fused multiply-add), as the CPU rule does.
__global__ __launch_bounds__(TPB) void gossip_scatter_kernel(float* __restrict__ m, float* __restrict__ o,
                                                             const uint32_t* __restrict__ index,
                                                             const float* __restrict__ value, long count, long n,
                                                             double a, int sign_o_only) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < count; p += stride) {
    const long i = (long)index[p];
    if (i >= n) continue;
    const double v = (double)value[p];
    if (sign_o_only) {
      o[i] = (float)__dadd_rn((double)o[i], sign_o_only < 0 ? -v : v);
    } else {
      const double av = __dmul_rn(a, v);
      m[i] = (float)__dadd_rn((double)m[i], av);
      o[i] = (float)__dadd_rn((double)o[i], av);
    }
  }
}

}  // namespace

extern "C" {

// bytes of workspace sl_gossip_topk needs for an n-element model
long sl_gossip_topk_workspace(long n) {
  return 4 * (d_words(n < 0 ? 0 : n) + CTRL_WORDS + HIST_WORDS + WGC_WORDS);
}

// index_out[k] (uint32), value_out[k] (f32), count_out[1] (uint32), workspace: 16-byte aligned device memory
int sl_gossip_topk(const float* m, float* o, long n, long k, uint32_t* index_out, float* value_out,
                   uint32_t* count_out, void* workspace, hipStream_t stream) {
  if (n <= 0 || k <= 0) return hipMemsetAsync(count_out, 0, 4, stream) == hipSuccess ? 0 : -2;
  if (n > 0xffffffffL || ((uintptr_t)workspace & 15)) return -1;
  if (k > n) k = n;
  float* d = (float*)workspace;
  uint32_t* ctrl = (uint32_t*)workspace + d_words(n);
  SelState* st = (SelState*)ctrl;
  uint32_t* hist = ctrl + CTRL_WORDS;
  uint32_t* wgc = hist + HIST_WORDS;
  if (hipMemsetAsync(ctrl, 0, 4 * (CTRL_WORDS + HIST_WORDS), stream) != hipSuccess) return -2;
  const long tiles = (n + TILE - 1) / TILE;
  const int wgs = (int)(tiles < MAX_WGS ? tiles : MAX_WGS);
  const long chunk = ((tiles + wgs - 1) / wgs) * TILE;
  const int vec_mo = (((uintptr_t)m | (uintptr_t)o) & 15) == 0;
  const dim3 grid(wgs), block(TPB);
  hipLaunchKernelGGL(topk_hist_kernel<0>, grid, block, 0, stream, m, o, d, st, hist, n, chunk, vec_mo);
  hipLaunchKernelGGL(topk_pick_kernel, dim3(1), block, 0, stream, st, hist, 0, (uint32_t)k, count_out);
  hipLaunchKernelGGL(topk_hist_kernel<1>, grid, block, 0, stream, m, o, d, st, hist + MAX_BINS, n, chunk, vec_mo);
  hipLaunchKernelGGL(topk_pick_kernel, dim3(1), block, 0, stream, st, hist + MAX_BINS, 1, (uint32_t)k, count_out);
  hipLaunchKernelGGL(topk_hist_kernel<2>, grid, block, 0, stream, m, o, d, st, hist + 2 * MAX_BINS, n, chunk, vec_mo);
  hipLaunchKernelGGL(topk_pick_kernel, dim3(1), block, 0, stream, st, hist + 2 * MAX_BINS, 2, (uint32_t)k, count_out);
  hipLaunchKernelGGL(topk_count_kernel, grid, block, 0, stream, d, st, wgc, n, chunk);
  hipLaunchKernelGGL(topk_scatter_kernel, grid, block, 0, stream, d, o, st, wgc, index_out, value_out, n, chunk,
                     (uint32_t)k);
  SL_CHECK_LAUNCH();
  return 0;
}

int sl_gossip_scatter(float* m, float* o, const uint32_t* index, const float* value, long count, long n, double a,
                      int sign_o_only, hipStream_t stream) {
  if (count <= 0) return 0;
  if (n <= 0 || count > n) return -1;
  long blocks = (count + TPB - 1) / TPB;
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(gossip_scatter_kernel, dim3((int)blocks), dim3(TPB), 0, stream, m, o, index, value, count, n, a,
                     sign_o_only);
  SL_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"

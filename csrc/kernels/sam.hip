// K5h -- sharpness-aware minimization (SAM, Foret et al. 2021) and its scale-invariant form ASAM
// (Kwon et al. 2021) over the ResNet trainers' flat parameter vector.  With g the first pass's
// local dL/dw and T_i = |w_i| + eta for a class-0 element of an adaptive step, 1 otherwise:
//     nrm = sqrt(sum_i (T_i g_i)^2),  scale = rho / (nrm + 1e-12)  (0 where nrm is not finite),
//     w'_i = float32(w_i + scale T_i T_i g_i)
// and the second pass runs at w'.  Semantics: serverless_learn_amd/ops/optim.py
// sam_perturb_reference.
//
// Three launches, ordered by their launch boundaries alone: no atomics, no tickets, no state
// between calls, grids that depend on n only.  Every sum has one fixed order and no product is
// contracted into an fma, so the bits are the same from call to call and in both builds, and a
// captured graph replays all three.
//   1. sam_norms_kernel: one workgroup per SAM_CHUNK elements writes one double, the chunk's
//      sum of (T g)^2.
//   2. sam_scale_kernel: one wave folds the chunk sums in chunk order and stores (nrm, scale).
//   3. sam_perturb_kernel: the walk and grid of opt_flat_groups_kernel (elementwise.hip); every
//      float4 saves w, stores w' and its bf16 shadow.
// The way back is a copy of the saved vector (sl_accum_flat, add = 0): exact, where subtracting
// the perturbation again would round.
#include "common.h"

using namespace sl;

// Everything below is arithmetic whose bits are pinned to the float64 reference: each operator
// rounds once, in the order written.
#pragma clang fp contract(off)

constexpr int SAM_CHUNK = 4096;  // elements per chunk (ops/optim.py SAM_CHUNK; sl_sam_chunk)
constexpr int SAM_WG = 256;
constexpr int SAM_VPL = SAM_CHUNK / (4 * SAM_WG);  // float4 loads per lane and array
static_assert(SAM_VPL * 4 * SAM_WG == SAM_CHUNK, "a full chunk is a whole number of float4 rounds");

// T of one element: the class byte is that of the element's 64-element block.
template <bool ADAPTIVE>
__device__ __forceinline__ double sam_t(float w, int cls, double eta) {
  if constexpr (ADAPTIVE) return cls == 0 ? fabs((double)w) + eta : 1.0;
  return 1.0;
}

// acc += (T g)^2 for the four elements of one float4, x y z w in order.  Plain: g g is exact in
// fp64 (48 significant bits) and the addition is the only rounding.  Adaptive: |w| + eta, the
// product with g and the square each round once, as the reference's do.
template <bool ADAPTIVE>
__device__ __forceinline__ void sam_sq4(double& acc, const float4& wv, const float4& gv, int cls, double eta) {
  const float wa[4] = {wv.x, wv.y, wv.z, wv.w}, ga[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const double t = sam_t<ADAPTIVE>(wa[j], cls, eta) * (double)ga[j];
    const double sq = t * t;
    acc = acc + sq;
  }
}

// Chunk c is elements [c SAM_CHUNK, min(n, (c + 1) SAM_CHUNK)); n is a multiple of 64, so every
// chunk is a whole number of float4s and of class blocks.  Lane l of round k takes float4
// l + 256 k of the chunk: a wave's load is 1 KB contiguous, and the 16 lanes of a class block
// read one byte of the map.  All loads of a lane -- SAM_VPL of g, and under ADAPTIVE as many of w
// and of the class map -- are issued before the first product: up to 8 x 16 bytes in flight per
// lane.  A full chunk takes the branch with no bounds test; the last one predicates each round
// on its float4 lying inside the vector.  Nothing at or beyond n is read.
// Fold: per lane rounds 0 .. 3 in order, xor butterflies across the wave, the four waves' sums
// from LDS in wave order.
template <bool ADAPTIVE>
__global__ __launch_bounds__(SAM_WG) void sam_norms_kernel(const float* __restrict__ w, const float* __restrict__ g,
                                                           const uint8_t* __restrict__ cls, long n, double eta,
                                                           double* __restrict__ partials) {
  __shared__ double lds[SAM_WG / 64];
  const long base = (long)blockIdx.x * SAM_CHUNK;
  const long left = n - base;
  const int nvec = (int)((left < SAM_CHUNK ? left : SAM_CHUNK) >> 2);
  const float4* wp = reinterpret_cast<const float4*>(w + base);
  const float4* gp = reinterpret_cast<const float4*>(g + base);
  const uint8_t* cp = cls + (base >> 6);
  const int lane = threadIdx.x;
  float4 wv[SAM_VPL], gv[SAM_VPL];
  int cv[SAM_VPL];
#pragma unroll
  for (int k = 0; k < SAM_VPL; ++k) {
    wv[k] = gv[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    cv[k] = 1;
  }
  if (nvec == SAM_CHUNK / 4) {
#pragma unroll
    for (int k = 0; k < SAM_VPL; ++k) gv[k] = gp[lane + k * SAM_WG];
    if constexpr (ADAPTIVE) {
#pragma unroll
      for (int k = 0; k < SAM_VPL; ++k) wv[k] = wp[lane + k * SAM_WG];
#pragma unroll
      for (int k = 0; k < SAM_VPL; ++k) cv[k] = cp[(lane + k * SAM_WG) >> 4];
    }
  } else {
#pragma unroll
    for (int k = 0; k < SAM_VPL; ++k) {  // (an if around the loads, not a select between two addresses)
      if (lane + k * SAM_WG < nvec) {
        gv[k] = gp[lane + k * SAM_WG];
        if constexpr (ADAPTIVE) {
          wv[k] = wp[lane + k * SAM_WG];
          cv[k] = cp[(lane + k * SAM_WG) >> 4];
        }
      }
    }
  }
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < SAM_VPL; ++k) sam_sq4<ADAPTIVE>(acc, wv[k], gv[k], cv[k], eta);
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) acc = acc + __shfl_xor(acc, m);
  if ((lane & 63) == 0) lds[lane >> 6] = acc;
  __syncthreads();
  if (lane == 0) {
    double s = lds[0];
#pragma unroll
    for (int v = 1; v < SAM_WG / 64; ++v) s = s + lds[v];
    partials[blockIdx.x] = s;
  }
}

constexpr int SAM_TILE = 2048;  // chunk sums staged in LDS at a time (16 KB)

// One wave.  The chunk sums are folded strictly in chunk order, ((p_0 + p_1) + p_2) + ..., which
// is the reference's order: the wave copies SAM_TILE of them into LDS with coalesced loads, then
// every lane runs the same chain of additions over the tile, reading each value by an LDS
// broadcast.  The reads do not depend on the sum, so they run ahead of it eight at a time; the
// chain of n_chunks dependent fp64 additions is the launch's whole cost (2,729 of them for a
// ResNet-18).  (Passing the values from lane to lane by lane reads instead took 116 us
// against 26: profiles/r28_sam.)
// out[0] = nrm, out[1] = scale = rho / (nrm + 1e-12), or 0 where nrm is an Inf or a NaN: the
// perturb launch then leaves the weights as they are.
__global__ __launch_bounds__(64) void sam_scale_kernel(const double* __restrict__ partials, int n_chunks, double rho,
                                                       double* __restrict__ out) {
  __shared__ double tile[SAM_TILE];
  const int lane = threadIdx.x;
  double s = 0.0;
  for (int base = 0; base < n_chunks; base += SAM_TILE) {
    const int cnt = n_chunks - base < SAM_TILE ? n_chunks - base : SAM_TILE;
    for (int j = lane; j < cnt; j += 64) tile[j] = partials[base + j];
    __syncthreads();
#pragma unroll 8
    for (int j = 0; j < cnt; ++j) s = s + tile[j];
    __syncthreads();
  }
  if (lane == 0) {
    const double nrm = sqrt(s);
    const bool finite = nrm == nrm && nrm <= 1.7976931348623157e308;
    out[0] = nrm;
    out[1] = finite ? rho / (nrm + 1e-12) : 0.0;
  }
}

// The perturbation.  Per float4: saved = w, w = w', shadow = bf16(w'): three streams in (w, g,
// and a byte of the class map per 64 elements under ADAPTIVE), three out, 18 bytes per
// parameter.  scale sits at one address for the whole grid, so it is read once per workgroup by
// a scalar load, with eta and the flag among the wave-uniform scalars.  Per element, in fp64 and
// left to right as the reference writes it: ((scale T) T) g, then w + that, then one conversion
// to fp32 -- five fp64 operations per element on a GPU whose fp64 vector rate is its fp32 rate,
// under a kernel bound by its bytes.  scale == 0 (a non-finite norm) copies w through, whatever
// g holds.  n is a multiple of 64: there is no scalar tail.
template <bool ADAPTIVE>
__global__ __launch_bounds__(256) void sam_perturb_kernel(float* __restrict__ w, const float* __restrict__ g,
                                                          float* __restrict__ saved, uint16_t* __restrict__ shadow,
                                                          long n, const uint8_t* __restrict__ cls, double eta,
                                                          const double* __restrict__ sam_buf) {
  const double scale = sam_buf[1];
  const bool on = scale != 0.0;
  const long stride = (long)gridDim.x * blockDim.x * 4;
  for (long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += stride) {
    const float4 wv = *reinterpret_cast<const float4*>(w + i);
    const float4 gv = *reinterpret_cast<const float4*>(g + i);
    int c = 1;
    if constexpr (ADAPTIVE) c = cls[i >> 6];
    const float wa[4] = {wv.x, wv.y, wv.z, wv.w}, ga[4] = {gv.x, gv.y, gv.z, gv.w};
    float wn[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double t = sam_t<ADAPTIVE>(wa[j], c, eta);
      const double st = scale * t;
      const double stt = st * t;
      const double d = stt * (double)ga[j];
      const double s = (double)wa[j] + d;
      wn[j] = on ? (float)s : wa[j];
    }
    *reinterpret_cast<float4*>(saved + i) = wv;
    *reinterpret_cast<float4*>(w + i) = make_float4(wn[0], wn[1], wn[2], wn[3]);
    uint2 pk;
    pk.x = pack2(wn[0], wn[1]);
    pk.y = pack2(wn[2], wn[3]);
    *reinterpret_cast<uint2*>(shadow + i) = pk;
  }
}

// what every launcher asks of the vector: n > 0, a multiple of the class block, below 2^31 chunks
static bool sam_n_ok(long n) { return n > 0 && n % 64 == 0 && (n + SAM_CHUNK - 1) / SAM_CHUNK < (1L << 31); }

extern "C" {

// the chunk size: ops/optim.py checks its SAM_CHUNK against this one
int sl_sam_chunk() { return SAM_CHUNK; }

// partials[c] = sum over chunk c of (T_i g_i)^2, c < n_chunks = ceil(n / SAM_CHUNK).  cls: one
// byte per 64 elements, n / 64 of them; adaptive: T_i = |w_i| + eta where cls is 0, else T_i = 1
// (w and cls are then not read, but must still be given).  partials is rewritten whole.
int sl_sam_norms(const float* w, const float* g, const uint8_t* cls, long n, int adaptive, double eta,
                 double* partials, int n_chunks, hipStream_t stream) {
  if (!w || !g || !cls || !partials || !sam_n_ok(n)) return -1;
  if (n_chunks != (n + SAM_CHUNK - 1) / SAM_CHUNK) return -1;
  if ((((uintptr_t)w | (uintptr_t)g) & 15) || ((uintptr_t)partials & 7)) return -1;
  if (adaptive && !(eta > 0.0 && eta <= 1.7976931348623157e308)) return -1;  // (NaN fails every comparison)
  if (adaptive)
    hipLaunchKernelGGL(sam_norms_kernel<true>, dim3(n_chunks), dim3(SAM_WG), 0, stream, w, g, cls, n, eta, partials);
  else
    hipLaunchKernelGGL(sam_norms_kernel<false>, dim3(n_chunks), dim3(SAM_WG), 0, stream, w, g, cls, n, eta, partials);
  SL_CHECK_LAUNCH();
  return 0;
}

// sam_buf[0] = nrm = sqrt(partials[0] + ... + partials[n_chunks - 1]), sam_buf[1] = scale.
int sl_sam_scale(const double* partials, int n_chunks, double rho, double* sam_buf, hipStream_t stream) {
  if (!partials || !sam_buf || n_chunks < 1) return -1;
  if (((uintptr_t)partials | (uintptr_t)sam_buf) & 7) return -1;
  if (!(rho > 0.0 && rho <= 1.7976931348623157e308)) return -1;
  hipLaunchKernelGGL(sam_scale_kernel, dim3(1), dim3(64), 0, stream, partials, n_chunks, rho, sam_buf);
  SL_CHECK_LAUNCH();
  return 0;
}

// saved[0, n) = w, w = w', shadow = bf16(w') with the scale sl_sam_scale left in sam_buf.  The four
// vectors do not overlap; cls, adaptive and eta are sl_sam_norms's.
int sl_sam_perturb(float* w, const float* g, float* saved, uint16_t* shadow, long n, const uint8_t* cls, int adaptive,
                   double eta, const double* sam_buf, hipStream_t stream) {
  if (!w || !g || !saved || !shadow || !cls || !sam_buf || !sam_n_ok(n)) return -1;
  if ((((uintptr_t)w | (uintptr_t)g | (uintptr_t)saved) & 15) || ((uintptr_t)shadow & 7) || ((uintptr_t)sam_buf & 7))
    return -1;
  if (w == saved || w == g || g == saved) return -1;
  if (adaptive && !(eta > 0.0 && eta <= 1.7976931348623157e308)) return -1;
  long blocks = (n + 1023) / 1024;  // (grid_for(n, 4) of elementwise.hip)
  if (blocks > 2048) blocks = 2048;
  if (adaptive)
    hipLaunchKernelGGL(sam_perturb_kernel<true>, dim3((int)blocks), dim3(256), 0, stream, w, g, saved, shadow, n, cls,
                       eta, sam_buf);
  else
    hipLaunchKernelGGL(sam_perturb_kernel<false>, dim3((int)blocks), dim3(256), 0, stream, w, g, saved, shadow, n,
                       cls, eta, sam_buf);
  SL_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"

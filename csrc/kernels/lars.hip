// K5f -- LARS (layer-wise adaptive rate scaling, You et al. 2017) over the ResNet trainers' flat
// parameter vector: for every conv / linear weight tensor T
//     trust_T = eta ||w_T|| / (||g_T|| + wd ||w_T|| + eps)        (1 where either norm is 0)
// and element-wise d = trust_T (g + wd_c w), m = mu m + d, w -= lr m; norm scales / shifts and
// biases (decay classes 1 and 2) keep trust 1 and their own decay.  Semantics and the host-side
// plan: serverless_learn_amd/ops/optim.py lars_update / lars_plan.
//
// Three launches, ordered by their launch boundaries alone: no atomics, no tickets, no state
// between calls, grids that depend on the plan only.  Every sum has one fixed order, so the bits
// are the same from call to call, in both builds and on every rank, and a captured graph replays
// all three.
//   1. lars_norms_kernel: the plan cuts every adapted tensor into chunks of at most LARS_CHUNK
//      elements that never straddle a tensor; one workgroup per chunk writes one double2
//      (sum w^2, sum g^2).  The flat vector is ~60 tensors of 1.7 K to 2.4 M elements, but the
//      chunks are equal (only a tensor's last one is short), so ~2,700 of them spread over the
//      CUs evenly whatever the tensors' sizes.
//   2. lars_trust_kernel: one wave per adapted tensor folds its chunks' partials and forms
//      (||w||, ||g||, trust) in fp64, each rounded once to fp32.
//   3. lars_update_kernel: the walk, grid and shadow store of opt_flat_groups_kernel
//      (elementwise.hip); a float4 at element i reads its class from cls[i >> 6] and its tensor
//      from tmap[i >> 6].
#include "common.h"

using namespace sl;

constexpr int LARS_CHUNK = 4096;  // elements per chunk (ops/optim.py LARS_CHUNK; sl_lars_chunk)
constexpr int LARS_WG = 256;
constexpr int LARS_VPL = LARS_CHUNK / (4 * LARS_WG);  // float4 loads per lane and array
static_assert(LARS_VPL * 4 * LARS_WG == LARS_CHUNK, "a full chunk is a whole number of float4 rounds");

// Sum of squares of one float4 into acc, x y z w in order.  A product of two fp32 values is
// exact in fp64 (48 significant bits), so each element costs one fp64 rounding, the addition,
// whether or not the compiler contracts it into an fma.
__device__ __forceinline__ void lars_sq4(double& acc, const float4& v) {
  const double a = v.x, b = v.y, c = v.z, d = v.w;
  acc += a * a;
  acc += b * b;
  acc += c * c;
  acc += d * d;
}

// chunks[c] = (offset, count): count in 1 .. LARS_CHUNK, offset a multiple of 4 (16-byte loads).
// Lane l of round k takes float4 l + 256 k of the chunk, so a wave's load is 1 KB contiguous.  All
// LARS_VPL loads of w and of g are issued before the first square: 2 LARS_VPL x 16 bytes in flight
// per lane, 32 KB per workgroup.  A full chunk (all but each tensor's last) takes the branch with
// no bounds test at all; a short one predicates each load on its float4 lying inside the chunk,
// and the count % 4 elements after the last whole float4 go to lanes 0 .. 2 as scalars.  Nothing
// outside [offset, offset + count) is read.
// Fold: per lane rounds 0 .. 3 in order (then the tail element), xor shuffles across the wave,
// the four waves' sums from LDS in wave order.
__global__ __launch_bounds__(LARS_WG) void lars_norms_kernel(const float* __restrict__ w, const float* __restrict__ g,
                                                             const int2* __restrict__ chunks,
                                                             double2* __restrict__ partials) {
  __shared__ double lds[2][LARS_WG / 64];
  const int2 ck = chunks[blockIdx.x];  // (workgroup-uniform: a scalar load)
  const float4* wp = reinterpret_cast<const float4*>(w + ck.x);
  const float4* gp = reinterpret_cast<const float4*>(g + ck.x);
  const int lane = threadIdx.x;
  float4 wv[LARS_VPL], gv[LARS_VPL];
  double aw = 0.0, ag = 0.0;
  if (ck.y == LARS_CHUNK) {
#pragma unroll
    for (int k = 0; k < LARS_VPL; ++k) wv[k] = wp[lane + k * LARS_WG];
#pragma unroll
    for (int k = 0; k < LARS_VPL; ++k) gv[k] = gp[lane + k * LARS_WG];
  } else {
    const int nvec = ck.y >> 2;
#pragma unroll
    for (int k = 0; k < LARS_VPL; ++k) {  // (an if around the loads, not a select between two addresses)
      wv[k] = gv[k] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (lane + k * LARS_WG < nvec) {
        wv[k] = wp[lane + k * LARS_WG];
        gv[k] = gp[lane + k * LARS_WG];
      }
    }
  }
#pragma unroll
  for (int k = 0; k < LARS_VPL; ++k) {
    lars_sq4(aw, wv[k]);
    lars_sq4(ag, gv[k]);
  }
  if (ck.y != LARS_CHUNK && lane < (ck.y & 3)) {
    const int i = ck.x + (ck.y & ~3) + lane;
    const double a = w[i], b = g[i];
    aw += a * a;
    ag += b * b;
  }
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    aw += __shfl_xor(aw, m);
    ag += __shfl_xor(ag, m);
  }
  if ((lane & 63) == 0) {
    lds[0][lane >> 6] = aw;
    lds[1][lane >> 6] = ag;
  }
  __syncthreads();
  if (lane == 0) {
    double sw = lds[0][0], sg = lds[1][0];
#pragma unroll
    for (int v = 1; v < LARS_WG / 64; ++v) {
      sw += lds[0][v];
      sg += lds[1][v];
    }
    partials[blockIdx.x] = make_double2(sw, sg);
  }
}

// tensors[t] = (offset, numel, first chunk, chunk count).  One wave per tensor: lane l adds
// partials first + l, first + l + 64, ... in that order, then the xor-shuffle tree; lane 0 forms
// the three results in fp64 and rounds each once to fp32.
__global__ __launch_bounds__(64) void lars_trust_kernel(const double2* __restrict__ partials,
                                                        const int4* __restrict__ tensors, double eta, double eps,
                                                        double wd, float* __restrict__ out) {
  const int4 t = tensors[blockIdx.x];
  double sw = 0.0, sg = 0.0;
  for (int c = threadIdx.x; c < t.w; c += 64) {
    const double2 p = partials[t.z + c];
    sw += p.x;
    sg += p.y;
  }
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    sw += __shfl_xor(sw, m);
    sg += __shfl_xor(sg, m);
  }
  if (threadIdx.x == 0) {
    const double wn = sqrt(sw), gn = sqrt(sg);
    const double trust = (wn > 0.0 && gn > 0.0) ? eta * wn / (gn + wd * wn + eps) : 1.0;
    float* o = out + 3 * (long)blockIdx.x;
    o[0] = (float)wn;
    o[1] = (float)gn;
    o[2] = (float)trust;
  }
}

// The update.  A sibling of opt_flat_groups_kernel and not a flag of it: the existing kernels'
// contractions must stay what they are (elementwise.hip records why).  Here the rule is three
// explicit fmafs and one product, the same in the float4 body and the scalar tail:
//     d = trust * fmaf(wd_c, w, g);  m = fmaf(mu, m, d);  w = fmaf(-lr, m, w)
// Every tensor starts on a 64-element boundary, so a float4 never straddles two classes or two
// tensors.  tmap[i >> 6] is the adapted tensor that owns element i (trust = out[3 t + 2] of
// lars_trust_kernel) or anything >= T (0xFFFF) for none: trust 1, and d is the fmaf itself.
struct LarsOpt {
  const int* step;      // updates applied so far (read only; the engine bumps it afterwards)
  const float* lr_tab;  // lr_tab[min(step, lr_last)] is this step's lr; nullptr: lr
  int lr_last;
  float lr, mu, wd, wd_norm, wd_bias;
  const uint8_t* cls;    // decay class of every 64-element block
  const uint16_t* tmap;  // adapted tensor of every 64-element block
  const float* trust;    // [T][3]: (||w||, ||g||, trust)
  int T;
};

__global__ __launch_bounds__(256) void lars_update_kernel(float* __restrict__ w, const float* __restrict__ g,
                                                          float* __restrict__ mom, uint16_t* __restrict__ shadow,
                                                          long n, LarsOpt o) {
  const int k = *o.step;
  const float lr = o.lr_tab ? o.lr_tab[k < 0 ? 0 : k < o.lr_last ? k : o.lr_last] : o.lr;
  auto decay_of = [&](long i) __attribute__((always_inline)) {
    const int c = o.cls[i >> 6];
    return c == 0 ? o.wd : c == 1 ? o.wd_norm : o.wd_bias;
  };
  auto trust_of = [&](long i) __attribute__((always_inline)) {
    const int t = o.tmap[i >> 6];
    return t < o.T ? o.trust[3 * t + 2] : 1.f;
  };
  auto apply = [&](float& wj, float gj, float& mj, float wdc, float tr) __attribute__((always_inline)) {
    float d = tr * fmaf(wdc, wj, gj);
    if (mom) { d = fmaf(o.mu, mj, d); mj = d; }
    wj = fmaf(-lr, d, wj);
  };
  const long stride = (long)gridDim.x * blockDim.x * 4;
  for (long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += stride) {
    if (i + 4 <= n) {
      const float4 wv = *reinterpret_cast<const float4*>(w + i);
      const float4 gv = *reinterpret_cast<const float4*>(g + i);
      float wa[4] = {wv.x, wv.y, wv.z, wv.w};
      const float ga[4] = {gv.x, gv.y, gv.z, gv.w};
      float ma[4] = {0.f, 0.f, 0.f, 0.f};
      if (mom) {
        const float4 mv = *reinterpret_cast<const float4*>(mom + i);
        ma[0] = mv.x; ma[1] = mv.y; ma[2] = mv.z; ma[3] = mv.w;
      }
      const float wdc = decay_of(i), tr = trust_of(i);
#pragma unroll
      for (int j = 0; j < 4; ++j) apply(wa[j], ga[j], ma[j], wdc, tr);
      *reinterpret_cast<float4*>(w + i) = make_float4(wa[0], wa[1], wa[2], wa[3]);
      if (mom) *reinterpret_cast<float4*>(mom + i) = make_float4(ma[0], ma[1], ma[2], ma[3]);
      if (shadow) {
        uint2 pk;
        pk.x = pack2(wa[0], wa[1]);
        pk.y = pack2(wa[2], wa[3]);
        *reinterpret_cast<uint2*>(shadow + i) = pk;
      }
    } else {
      for (long q = i; q < n; ++q) {
        float wq = w[q], mq = mom ? mom[q] : 0.f;
        apply(wq, g[q], mq, decay_of(q), trust_of(q));
        w[q] = wq;
        if (mom) mom[q] = mq;
        if (shadow) shadow[q] = f2bf(wq);
      }
    }
  }
}

extern "C" {

// the plan's chunk size: ops/optim.py checks its LARS_CHUNK against this one
int sl_lars_chunk() { return LARS_CHUNK; }

// partials[c] = (sum w^2, sum g^2) over chunk c of the plan, c < n_chunks.  chunks: int32
// [n_chunks][2] = (offset, count) on the device, each inside the vectors (the caller's plan; the
// host cannot read it back here).  partials: [n_chunks][2] fp64, rewritten whole by every call.
int sl_lars_norms(const float* w, const float* g, const int* chunks, int n_chunks, double* partials,
                  hipStream_t stream) {
  if (!w || !g || !chunks || !partials || n_chunks < 1) return -1;
  if ((((uintptr_t)w | (uintptr_t)g | (uintptr_t)partials) & 15) || ((uintptr_t)chunks & 7)) return -1;
  hipLaunchKernelGGL(lars_norms_kernel, dim3(n_chunks), dim3(LARS_WG), 0, stream, w, g,
                     reinterpret_cast<const int2*>(chunks), reinterpret_cast<double2*>(partials));
  SL_CHECK_LAUNCH();
  return 0;
}

// out[t] = (||w_t||, ||g_t||, trust_t) as fp32 for the T adapted tensors.  tensors: int32 [T][4] =
// (offset, numel, first chunk, chunk count) on the device.
int sl_lars_trust(const double* partials, const int* tensors, int T, double eta, double eps, double wd, float* out,
                  hipStream_t stream) {
  if (!partials || !tensors || !out || T < 1) return -1;
  if ((((uintptr_t)partials | (uintptr_t)tensors) & 15) || ((uintptr_t)out & 3)) return -1;
  if (!(eta > 0.0) || !(eps >= 0.0) || !(wd >= 0.0)) return -1;  // (NaN fails every comparison)
  hipLaunchKernelGGL(lars_trust_kernel, dim3(T), dim3(64), 0, stream, reinterpret_cast<const double2*>(partials),
                     reinterpret_cast<const int4*>(tensors), eta, eps, wd, out);
  SL_CHECK_LAUNCH();
  return 0;
}

// The LARS update of w[0, n) at the learning rate lr_tab[min(*step, lr_n - 1)] (nullptr: lr).
// cls / tmap: one entry per 64 elements, (n + 63) / 64 of each; trust: sl_lars_trust's out.
// The caller advances *step after this launch.
int sl_sgd_flat_lars(float* w, const float* g, float* mom, uint16_t* shadow, long n, const int* step,
                     const float* lr_tab, int lr_n, float lr, float mu, float wd, float wd_norm, float wd_bias,
                     const uint8_t* cls, const uint16_t* tmap, const float* trust, int T, hipStream_t stream) {
  if (!w || !g || !step || !cls || !tmap || !trust || n < 1 || T < 1 || (lr_tab && lr_n < 1)) return -1;
  if (((uintptr_t)w | (uintptr_t)g | (uintptr_t)(mom ? mom : w)) & 15) return -1;
  if ((shadow && ((uintptr_t)shadow & 7)) || ((uintptr_t)tmap & 1) || ((uintptr_t)trust & 3)) return -1;
  if (!(wd >= 0.f) || !(wd_norm >= 0.f) || !(wd_bias >= 0.f)) return -1;
  long blocks = (n + 1023) / 1024;  // (grid_for(n, 4) of elementwise.hip)
  if (blocks > 2048) blocks = 2048;
  const LarsOpt o = {step, lr_tab, lr_tab ? lr_n - 1 : 0, lr, mu, wd, wd_norm, wd_bias, cls, tmap, trust, T};
  hipLaunchKernelGGL(lars_update_kernel, dim3((int)blocks), dim3(256), 0, stream, w, g, mom, shadow, n, o);
  SL_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"

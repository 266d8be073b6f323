// Memory-bound helper kernels: gossip delta-apply (K7), flat fused SGD (K5), gradient clipping,
// gradient accumulation and the weight EMA.
#include "common.h"

using namespace sl;

// K7 -- gossip delta-apply, fused, on the device-resident f32 model.
// Server side of an exchange (/root/reference/src/worker.cc:81-100) and the
// client-side absorb (:155-164) are the same three updates:
//     m += alpha * d_in      (d_in arrives as wire f64; absent past its length)
//     d_out = m - o          (f64, straight into the reply buffer)
//     o = m
// One pass, 4 elements per thread, no temporaries.
__global__ __launch_bounds__(256) void gossip_apply_kernel(float* __restrict__ m, float* __restrict__ o,
                                                           const double* __restrict__ din, long kin, double alpha,
                                                           double* __restrict__ dout, long n) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    double mi = (double)m[i];
    if (din && i < kin) mi += alpha * din[i];
    const float mf = (float)mi;
    if (dout) dout[i] = (double)mf - (double)o[i];
    m[i] = mf;
    o[i] = mf;
  }
}

// K7b -- client-side absorb of a reply r while training may have advanced m during the RPC:
//     m += alpha * r
//     o += sent + alpha * r   (sent = the delta this client put on the wire; absent if a
//                              server-side exchange reset o in the meantime)
// so o advances by exactly what was shared and steps taken during the RPC stay unshared.
__global__ __launch_bounds__(256) void gossip_absorb_kernel(float* __restrict__ m, float* __restrict__ o,
                                                            const double* __restrict__ r, long kr, double alpha,
                                                            const double* __restrict__ sent, long ks, long n) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const double ar = (i < kr) ? alpha * r[i] : 0.0;
    double oi = (double)o[i];
    if (sent && i < ks) oi += sent[i];
    m[i] = (float)((double)m[i] + ar);
    o[i] = (float)(oi + ar);
  }
}

// K5 -- flat fused SGD over a whole model's parameter vector (one launch for
// every tensor): torch.optim.SGD semantics (dampening 0, no nesterov), with
// optional momentum buffer and optional bf16 shadow copy for the GEMM kernels.
__global__ __launch_bounds__(256) void sgd_flat_kernel(float* __restrict__ w, const float* __restrict__ g,
                                                       float* __restrict__ mom, uint16_t* __restrict__ shadow,
                                                       long n, float lr, float mu, float wd, float gscale) {
  const long stride = (long)gridDim.x * blockDim.x * 4;
  for (long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += stride) {
    if (i + 4 <= n) {
      float4 wv = *reinterpret_cast<float4*>(w + i);
      const float4 gv = *reinterpret_cast<const float4*>(g + i);
      float wa[4] = {wv.x, wv.y, wv.z, wv.w};
      const float ga[4] = {gv.x, gv.y, gv.z, gv.w};
      float ma[4] = {0.f, 0.f, 0.f, 0.f};
      if (mom) {
        const float4 mv = *reinterpret_cast<const float4*>(mom + i);
        ma[0] = mv.x; ma[1] = mv.y; ma[2] = mv.z; ma[3] = mv.w;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float d = ga[j] * gscale + wd * wa[j];
        if (mom) { d = mu * ma[j] + d; ma[j] = d; }
        wa[j] -= lr * d;
      }
      *reinterpret_cast<float4*>(w + i) = make_float4(wa[0], wa[1], wa[2], wa[3]);
      if (mom) *reinterpret_cast<float4*>(mom + i) = make_float4(ma[0], ma[1], ma[2], ma[3]);
      if (shadow) {
        uint2 pk;
        pk.x = pack2(wa[0], wa[1]);
        pk.y = pack2(wa[2], wa[3]);
        *reinterpret_cast<uint2*>(shadow + i) = pk;
      }
    } else {
      for (long k = i; k < n; ++k) {
        float d = g[k] * gscale + wd * w[k];
        if (mom) { d = mu * mom[k] + d; mom[k] = d; }
        w[k] -= lr * d;
        if (shadow) shadow[k] = f2bf(w[k]);
      }
    }
  }
}

// K5 under a rule that depends on the optimizer step (a device-resident counter, so a captured
// graph replays it with a moving learning rate): AdamW (torch.optim.AdamW: decoupled weight
// decay, bias correction, no amsgrad; mom is the first moment, v the second) or momentum SGD
// with a scheduled learning rate.  Same walk as sgd_flat_kernel.  This launch only reads the
// step; the engine bumps it with its cursor launcher afterwards.
struct FlatOpt {
  const int* step;      // updates applied so far
  const float* lr_tab;  // lr_tab[min(step, lr_last)] is this step's lr; nullptr: lr
  int lr_last;
  float lr, mu, wd, gscale;
  // from the host, each computed in double and rounded once (1 - 0.999f is 3e-5 off; 1 - b^t
  // cancels at small t: ln b and expm1)
  float b1, b2, omb1, omb2, lnb1, lnb2, eps;
};

template <bool ADAMW>
__global__ __launch_bounds__(256) void opt_flat_kernel(float* __restrict__ w, const float* __restrict__ g,
                                                       float* __restrict__ mom, float* __restrict__ v,
                                                       uint16_t* __restrict__ shadow, long n, FlatOpt o) {
  // wave-uniform scalars of the step, ahead of the loads
  const int k = *o.step;
  const float lr = o.lr_tab ? o.lr_tab[k < o.lr_last ? k : o.lr_last] : o.lr;
  float keep = 1.f, ssz = 0.f, rbc2 = 0.f;
  if constexpr (ADAMW) {
    const float t = (float)k + 1.f;
    keep = 1.f - lr * o.wd;
    ssz = lr / -expm1f(t * o.lnb1);
    rbc2 = 1.f / sqrtf(-expm1f(t * o.lnb2));
  }
  auto apply = [&](float& wj, float gj, float& mj, float& vj) __attribute__((always_inline)) {
    const float gs = gj * o.gscale;
    if constexpr (ADAMW) {
      mj = fmaf(o.b1, mj, o.omb1 * gs);
      vj = fmaf(o.b2, vj, o.omb2 * gs * gs);
      wj = fmaf(-ssz, mj / fmaf(sqrtf(vj), rbc2, o.eps), wj * keep);
    } else {
      float d = gs + o.wd * wj;
      if (mom) { d = o.mu * mj + d; mj = d; }
      wj -= lr * d;
    }
  };
  const long stride = (long)gridDim.x * blockDim.x * 4;
  for (long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += stride) {
    if (i + 4 <= n) {
      float4 wv = *reinterpret_cast<float4*>(w + i);
      const float4 gv = *reinterpret_cast<const float4*>(g + i);
      float wa[4] = {wv.x, wv.y, wv.z, wv.w};
      const float ga[4] = {gv.x, gv.y, gv.z, gv.w};
      float ma[4] = {0.f, 0.f, 0.f, 0.f}, va[4] = {0.f, 0.f, 0.f, 0.f};
      if (mom) {
        const float4 mv = *reinterpret_cast<const float4*>(mom + i);
        ma[0] = mv.x; ma[1] = mv.y; ma[2] = mv.z; ma[3] = mv.w;
      }
      if constexpr (ADAMW) {
        const float4 vv = *reinterpret_cast<const float4*>(v + i);
        va[0] = vv.x; va[1] = vv.y; va[2] = vv.z; va[3] = vv.w;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) apply(wa[j], ga[j], ma[j], va[j]);
      *reinterpret_cast<float4*>(w + i) = make_float4(wa[0], wa[1], wa[2], wa[3]);
      if (mom) *reinterpret_cast<float4*>(mom + i) = make_float4(ma[0], ma[1], ma[2], ma[3]);
      if constexpr (ADAMW) *reinterpret_cast<float4*>(v + i) = make_float4(va[0], va[1], va[2], va[3]);
      if (shadow) {
        uint2 pk;
        pk.x = pack2(wa[0], wa[1]);
        pk.y = pack2(wa[2], wa[3]);
        *reinterpret_cast<uint2*>(shadow + i) = pk;
      }
    } else {
      for (long q = i; q < n; ++q) {
        float wq = w[q], mq = mom ? mom[q] : 0.f, vq = 0.f;
        if constexpr (ADAMW) vq = v[q];
        apply(wq, g[q], mq, vq);
        w[q] = wq;
        if (mom) mom[q] = mq;
        if constexpr (ADAMW) v[q] = vq;
        if (shadow) shadow[q] = f2bf(wq);
      }
    }
  }
}

// opt_flat_kernel with a weight decay per class: element i has class cls[i >> 6] (0 weight, 1 norm,
// 2 bias; every tensor of the vector starts on a 64-element boundary, so a float4 chunk never
// straddles two classes and a wave's 256 elements read four bytes of the map).  Class 0 decays by
// FlatOpt's wd.  Same walk and grid; the three decays (SGD) / keep factors (AdamW) are
// wave-uniform scalars computed once per thread.
//
// A sibling kernel and not a template flag of opt_flat_kernel: routing both through one inlined
// body changed which product the compiler contracts in the ungrouped SGD rule (its float4 chunks
// compute fma(gscale, g, wd w), its scalar tail fma(wd, w, gscale g)), and an ungrouped trainer
// must keep its bits.  Here every contraction is written out to match that kernel, so that a
// grouped launch leaves in each element exactly what opt_flat_kernel leaves with that class's
// decay (tests/test_decay_groups_gpu.py compares them bit for bit).
struct FlatGroups {
  const uint8_t* cls;
  float wd_norm, wd_bias;  // the decay of classes 1 and 2
};

template <bool ADAMW>
__global__ __launch_bounds__(256) void opt_flat_groups_kernel(float* __restrict__ w, const float* __restrict__ g,
                                                              float* __restrict__ mom, float* __restrict__ v,
                                                              uint16_t* __restrict__ shadow, long n, FlatOpt o,
                                                              FlatGroups gr) {
  // wave-uniform scalars of the step, ahead of the loads
  const int k = *o.step;
  const float lr = o.lr_tab ? o.lr_tab[k < o.lr_last ? k : o.lr_last] : o.lr;
  float ssz = 0.f, rbc2 = 0.f;
  // per class: the decay (SGD) or the keep factor 1 - lr wd (AdamW)
  float dk[3] = {o.wd, gr.wd_norm, gr.wd_bias};
  if constexpr (ADAMW) {
    const float t = (float)k + 1.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) dk[c] = 1.f - lr * dk[c];
    ssz = lr / -expm1f(t * o.lnb1);
    rbc2 = 1.f / sqrtf(-expm1f(t * o.lnb2));
  }
  auto class_of = [&](long i) __attribute__((always_inline)) {
    const int c = gr.cls[i >> 6];
    return c == 0 ? dk[0] : c == 1 ? dk[1] : dk[2];
  };
  // TAIL: the scalar tail's contraction of the SGD rule (see above)
  auto apply = [&](float& wj, float gj, float& mj, float& vj, float dkc, bool tail) __attribute__((always_inline)) {
    if constexpr (ADAMW) {
      const float gs = gj * o.gscale;
      mj = fmaf(o.b1, mj, o.omb1 * gs);
      vj = fmaf(o.b2, vj, o.omb2 * gs * gs);
      wj = fmaf(-ssz, mj / fmaf(sqrtf(vj), rbc2, o.eps), wj * dkc);
    } else {
      float d = tail ? fmaf(dkc, wj, gj * o.gscale) : fmaf(gj, o.gscale, dkc * wj);
      if (mom) { d = fmaf(o.mu, mj, d); mj = d; }
      wj = fmaf(-lr, d, wj);
    }
  };
  const long stride = (long)gridDim.x * blockDim.x * 4;
  for (long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += stride) {
    if (i + 4 <= n) {
      float4 wv = *reinterpret_cast<float4*>(w + i);
      const float4 gv = *reinterpret_cast<const float4*>(g + i);
      float wa[4] = {wv.x, wv.y, wv.z, wv.w};
      const float ga[4] = {gv.x, gv.y, gv.z, gv.w};
      float ma[4] = {0.f, 0.f, 0.f, 0.f}, va[4] = {0.f, 0.f, 0.f, 0.f};
      if (mom) {
        const float4 mv = *reinterpret_cast<const float4*>(mom + i);
        ma[0] = mv.x; ma[1] = mv.y; ma[2] = mv.z; ma[3] = mv.w;
      }
      if constexpr (ADAMW) {
        const float4 vv = *reinterpret_cast<const float4*>(v + i);
        va[0] = vv.x; va[1] = vv.y; va[2] = vv.z; va[3] = vv.w;
      }
      const float dkc = class_of(i);
#pragma unroll
      for (int j = 0; j < 4; ++j) apply(wa[j], ga[j], ma[j], va[j], dkc, false);
      *reinterpret_cast<float4*>(w + i) = make_float4(wa[0], wa[1], wa[2], wa[3]);
      if (mom) *reinterpret_cast<float4*>(mom + i) = make_float4(ma[0], ma[1], ma[2], ma[3]);
      if constexpr (ADAMW) *reinterpret_cast<float4*>(v + i) = make_float4(va[0], va[1], va[2], va[3]);
      if (shadow) {
        uint2 pk;
        pk.x = pack2(wa[0], wa[1]);
        pk.y = pack2(wa[2], wa[3]);
        *reinterpret_cast<uint2*>(shadow + i) = pk;
      }
    } else {
      for (long q = i; q < n; ++q) {
        float wq = w[q], mq = mom ? mom[q] : 0.f, vq = 0.f;
        if constexpr (ADAMW) vq = v[q];
        apply(wq, g[q], mq, vq, class_of(q), true);
        w[q] = wq;
        if (mom) mom[q] = mq;
        if constexpr (ADAMW) v[q] = vq;
        if (shadow) shadow[q] = f2bf(wq);
      }
    }
  }
}

// K5c -- global-norm gradient clipping (torch.nn.utils.clip_grad_norm_) over the flat fp32
// gradient, as two launches with no atomics and no state a graph replay would have to reset:
//   1. clip_sumsq_kernel: grid-stride float4 walk (scalar tail for n % 4), squares accumulated
//      in fp64 per thread, folded across the wave by xor shuffles and across the four waves
//      through LDS in wave order; one fp64 partial per workgroup.
//   2. clip_scale_kernel: every workgroup sums all partials in the same fixed order, so all of
//      them hold the same total = (float)sqrt(sum) and coef = min(1, max_norm / (total + 1e-6));
//      each scales its share of g (skipped at coef == 1: a multiply by 1.0 is the identity) and
//      workgroup 0 stores total, the norm before clipping.
// The grid (hence the partition and the summation order) depends on n alone: the result is
// bit-identical from call to call and from rank to rank.
constexpr int CLIP_WG = 256;
constexpr int CLIP_MAX_BLOCKS = 1024;  // one pass of the full grid covers 1024 * 256 * 4 floats

static int clip_blocks(long n) {
  const long blocks = (n + CLIP_WG * 4L - 1) / (CLIP_WG * 4L);
  return (int)(blocks > CLIP_MAX_BLOCKS ? CLIP_MAX_BLOCKS : blocks < 1 ? 1 : blocks);
}

// sum of v over the workgroup, the same bits in every thread: butterfly within the wave (both
// lanes of a pair add the same two values), then the waves' sums from LDS in wave order
__device__ __forceinline__ double clip_block_sum(double v, double* lds) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) v += __shfl_xor(v, m);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = lds[0];
#pragma unroll
  for (int w = 1; w < CLIP_WG / 64; ++w) t += lds[w];
  return t;
}

__global__ __launch_bounds__(CLIP_WG) void clip_sumsq_kernel(const float* __restrict__ g, long n,
                                                              double* __restrict__ partials) {
  __shared__ double lds[CLIP_WG / 64];
  double acc = 0.0;
  const long stride = (long)gridDim.x * CLIP_WG * 4;
  for (long i = ((long)blockIdx.x * CLIP_WG + threadIdx.x) * 4; i < n; i += stride) {
    if (i + 4 <= n) {
      const float4 v = *reinterpret_cast<const float4*>(g + i);
      const double a = v.x, b = v.y, c = v.z, d = v.w;
      acc += a * a;
      acc += b * b;
      acc += c * c;
      acc += d * d;
    } else {
      for (long k = i; k < n; ++k) {
        const double a = g[k];
        acc += a * a;
      }
    }
  }
  const double t = clip_block_sum(acc, lds);
  if (threadIdx.x == 0) partials[blockIdx.x] = t;
}

__global__ __launch_bounds__(CLIP_WG) void clip_scale_kernel(float* __restrict__ g, long n, float max_norm,
                                                              const double* __restrict__ partials,
                                                              float* __restrict__ norm_out) {
  __shared__ double lds[CLIP_WG / 64];
  double acc = 0.0;
  for (int p = threadIdx.x; p < (int)gridDim.x; p += CLIP_WG) acc += partials[p];  // launch 1 ran this grid
  const float total = (float)sqrt(clip_block_sum(acc, lds));
  const float coef = fminf(1.f, max_norm / (total + 1e-6f));
  if (blockIdx.x == 0 && threadIdx.x == 0) *norm_out = total;
  if (coef == 1.f) return;
  const long stride = (long)gridDim.x * CLIP_WG * 4;
  for (long i = ((long)blockIdx.x * CLIP_WG + threadIdx.x) * 4; i < n; i += stride) {
    if (i + 4 <= n) {
      float4 v = *reinterpret_cast<float4*>(g + i);
      v.x *= coef; v.y *= coef; v.z *= coef; v.w *= coef;
      *reinterpret_cast<float4*>(g + i) = v;
    } else {
      for (long k = i; k < n; ++k) g[k] *= coef;
    }
  }
}

// K5d -- gradient accumulation: dst[i] = add ? dst[i] + src[i] : src[i] over two fp32 ranges that
// do not overlap.  One rounding per element, no atomics, no state: the same bits in both builds.
// The ranges need only 4-byte alignment (the ResNet engine folds grad[lo:hi] bucket views whose lo
// is a tensor boundary of the flat layout): `head` elements (< 4, from the launcher) bring dst to
// a 16-byte boundary and are done one per thread, as is the tail past the last whole float4; the
// body moves 16 bytes per lane on the dst side and, where src shares dst's misalignment (SRC16,
// every caller in the engines), on the src side too -- dword loads otherwise.
template <bool SRC16>
__global__ __launch_bounds__(256) void accum_flat_kernel(float* __restrict__ dst, const float* __restrict__ src,
                                                         long n, int head, int add) {
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long body = (n - head) >> 2;  // whole float4s after the head
  const long tail0 = head + 4 * body;
  if (tid < head + (n - tail0)) {  // at most 6 threads of workgroup 0
    const long i = tid < head ? tid : tail0 + (tid - head);
    dst[i] = add ? dst[i] + src[i] : src[i];
  }
  float* d = dst + head;
  const float* s = src + head;
  const long stride = (long)gridDim.x * blockDim.x;
  for (long q = tid; q < body; q += stride) {
    float4 sv;
    if constexpr (SRC16) {
      sv = *reinterpret_cast<const float4*>(s + 4 * q);
    } else {
      sv = make_float4(s[4 * q], s[4 * q + 1], s[4 * q + 2], s[4 * q + 3]);
    }
    if (add) {
      const float4 dv = *reinterpret_cast<const float4*>(d + 4 * q);
      sv.x = dv.x + sv.x; sv.y = dv.y + sv.y; sv.z = dv.z + sv.z; sv.w = dv.w + sv.w;
    }
    *reinterpret_cast<float4*>(d + 4 * q) = sv;
  }
}

// K5e -- weight EMA: e <- e + omd * (w - e) over the flat fp32 parameters, after the update launch,
// with omd = omd_tab[min(*step, tab_last)] (float32(1 - decay_t), from the host).  Three fp32
// operations, each rounded once and none contracted into an fma, so torch's e + omd * (w - e) gives
// the same bits (ops/optim.py ema_update_) and w == e is a fixed point.  Same walk as sgd_flat_kernel
// over two whole allocations; the n % 4 tail is done by the first lanes of workgroup 0.  Every
// workgroup reads the step once at its start (wave-uniform; the table entry is a scalar load of a
// kernel-argument pointer at a uniform index) and the launch advances it at its end with the ticket
// protocol of mlp_fused.hip opt_end: one launch per step, no bump launch, no float atomics.
// (Plain operators under contract(off), not __fsub_rn / __fmul_rn / __fadd_rn: those are inline
// functions over the same operators, compiled under the translation unit's fast contraction, and the
// multiply and the add came out as one v_fma.  The pragma takes the contract flag off these three.)
__device__ __forceinline__ float ema_one(float e, float w, float omd) {
#pragma clang fp contract(off)
  const float d = w - e;
  const float p = omd * d;
  return e + p;
}

__global__ __launch_bounds__(256) void ema_flat_kernel(float* __restrict__ ema, const float* __restrict__ w, long n,
                                                       int* step, unsigned* ticket,
                                                       const float* __restrict__ omd_tab, int tab_last) {
  const int k = __builtin_amdgcn_readfirstlane(__hip_atomic_load(step, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  const float omd = omd_tab[k < 0 ? 0 : k < tab_last ? k : tab_last];
  const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const long body = n >> 2;  // whole float4s
  const long stride = (long)gridDim.x * blockDim.x;
  for (long q = tid; q < body; q += stride) {
    float4 e = *reinterpret_cast<const float4*>(ema + 4 * q);
    const float4 x = *reinterpret_cast<const float4*>(w + 4 * q);
    e.x = ema_one(e.x, x.x, omd);
    e.y = ema_one(e.y, x.y, omd);
    e.z = ema_one(e.z, x.z, omd);
    e.w = ema_one(e.w, x.w, omd);
    *reinterpret_cast<float4*>(ema + 4 * q) = e;
  }
  if (tid < (n & 3)) {  // at most 3 lanes of workgroup 0
    const long i = 4 * body + tid;
    ema[i] = ema_one(ema[i], w[i], omd);
  }
  // every workgroup of this launch has read the step before the last ticket is drawn (opt_end)
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (t + 1u == gridDim.x) {
      __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __hip_atomic_store(step, k + 1, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}

// f32 -> bf16 copy (shadow refresh after load / broadcast).
__global__ __launch_bounds__(256) void to_bf16_kernel(const float* __restrict__ src, uint16_t* __restrict__ dst, long n) {
  const long stride = (long)gridDim.x * blockDim.x;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) dst[i] = f2bf(src[i]);
}

static int grid_for(long n, int per_thread) {
  long blocks = (n + 256L * per_thread - 1) / (256L * per_thread);
  if (blocks > 2048) blocks = 2048;
  return blocks < 1 ? 1 : (int)blocks;
}

extern "C" {

int sl_gossip_apply(float* m, float* o, const double* din, long kin, double alpha, double* dout, long n,
                    hipStream_t stream) {
  if (n <= 0) return 0;
  if (kin > n) return -1;
  hipLaunchKernelGGL(gossip_apply_kernel, dim3(grid_for(n, 1)), dim3(256), 0, stream, m, o, din, kin, alpha, dout, n);
  SL_CHECK_LAUNCH();
  return 0;
}

int sl_gossip_absorb(float* m, float* o, const double* r, long kr, double alpha, const double* sent, long ks,
                     long n, hipStream_t stream) {
  if (n <= 0) return 0;
  if (kr > n || ks > n) return -1;
  hipLaunchKernelGGL(gossip_absorb_kernel, dim3(grid_for(n, 1)), dim3(256), 0, stream, m, o, r, kr, alpha, sent, ks, n);
  SL_CHECK_LAUNCH();
  return 0;
}

int sl_sgd_flat(float* w, const float* g, float* mom, uint16_t* shadow, long n, float lr, float mu, float wd,
                float gscale, hipStream_t stream) {
  if (n <= 0) return 0;
  if (((uintptr_t)w | (uintptr_t)g | (uintptr_t)(mom ? mom : w)) & 15) return -1;
  if (shadow && ((uintptr_t)shadow & 7)) return -1;
  hipLaunchKernelGGL(sgd_flat_kernel, dim3(grid_for(n, 4)), dim3(256), 0, stream, w, g, mom, shadow, n, lr, mu, wd, gscale);
  SL_CHECK_LAUNCH();
  return 0;
}

static bool flat_opt_ok(const float* w, const float* g, const float* mom, const float* v, const uint16_t* shadow,
                        const int* step, const float* lr_tab, int lr_n) {
  if (!w || !g || !step || (lr_tab && lr_n < 1)) return false;
  if (((uintptr_t)w | (uintptr_t)g | (uintptr_t)(mom ? mom : w) | (uintptr_t)(v ? v : w)) & 15) return false;
  return !(shadow && ((uintptr_t)shadow & 7));
}

// AdamW over the flat vector; the learning rate of step *step is lr_tab[min(*step, lr_n - 1)]
// (nullptr: lr).  The caller advances *step after this launch.
int sl_adamw_flat(float* w, const float* g, float* mom, float* v, uint16_t* shadow, long n, const int* step,
                  const float* lr_tab, int lr_n, float lr, float wd, float gscale, float b1, float b2, float omb1,
                  float omb2, float lnb1, float lnb2, float eps, hipStream_t stream) {
  if (n <= 0) return 0;
  if (!mom || !v || !flat_opt_ok(w, g, mom, v, shadow, step, lr_tab, lr_n)) return -1;
  if (!(lnb1 < 0.f) || !(lnb2 < 0.f) || !(eps > 0.f)) return -1;  // bias corrections divide by 1 - b^t
  const FlatOpt o = {step, lr_tab, lr_tab ? lr_n - 1 : 0, lr, 0.f, wd, gscale, b1, b2, omb1, omb2, lnb1, lnb2, eps};
  hipLaunchKernelGGL(opt_flat_kernel<true>, dim3(grid_for(n, 4)), dim3(256), 0, stream, w, g, mom, v, shadow, n, o);
  SL_CHECK_LAUNCH();
  return 0;
}

static bool flat_groups_ok(const uint8_t* cls, float wd, float wd_norm, float wd_bias) {
  return cls && wd >= 0.f && wd_norm >= 0.f && wd_bias >= 0.f;  // (NaN fails every comparison)
}

// sl_adamw_flat with a weight decay per class: element i decays by wd (cls[i >> 6] == 0), wd_norm
// (1) or wd_bias (2).  cls: one byte per 64 elements, (n + 63) / 64 of them, each 0, 1 or 2.
int sl_adamw_flat_groups(float* w, const float* g, float* mom, float* v, uint16_t* shadow, long n, const int* step,
                         const float* lr_tab, int lr_n, float lr, float wd, float gscale, float b1, float b2,
                         float omb1, float omb2, float lnb1, float lnb2, float eps, const uint8_t* cls, float wd_norm,
                         float wd_bias, hipStream_t stream) {
  if (n <= 0) return 0;
  if (!mom || !v || !flat_opt_ok(w, g, mom, v, shadow, step, lr_tab, lr_n)) return -1;
  if (!(lnb1 < 0.f) || !(lnb2 < 0.f) || !(eps > 0.f) || !flat_groups_ok(cls, wd, wd_norm, wd_bias)) return -1;
  const FlatOpt o = {step, lr_tab, lr_tab ? lr_n - 1 : 0, lr, 0.f, wd, gscale, b1, b2, omb1, omb2, lnb1, lnb2, eps};
  hipLaunchKernelGGL(opt_flat_groups_kernel<true>, dim3(grid_for(n, 4)), dim3(256), 0, stream, w, g, mom, v, shadow,
                     n, o, FlatGroups{cls, wd_norm, wd_bias});
  SL_CHECK_LAUNCH();
  return 0;
}

// sl_sgd_flat_lr with a weight decay per class (see sl_adamw_flat_groups); without a table the
// learning rate is lr
int sl_sgd_flat_lr_groups(float* w, const float* g, float* mom, uint16_t* shadow, long n, const int* step,
                          const float* lr_tab, int lr_n, float lr, float mu, float wd, float gscale,
                          const uint8_t* cls, float wd_norm, float wd_bias, hipStream_t stream) {
  if (n <= 0) return 0;
  if (!flat_opt_ok(w, g, mom, nullptr, shadow, step, lr_tab, lr_n) || !flat_groups_ok(cls, wd, wd_norm, wd_bias))
    return -1;
  const FlatOpt o = {step, lr_tab, lr_tab ? lr_n - 1 : 0, lr, mu, wd, gscale, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  hipLaunchKernelGGL(opt_flat_groups_kernel<false>, dim3(grid_for(n, 4)), dim3(256), 0, stream, w, g, mom,
                     static_cast<float*>(nullptr), shadow, n, o, FlatGroups{cls, wd_norm, wd_bias});
  SL_CHECK_LAUNCH();
  return 0;
}

// sl_sgd_flat with the learning rate of step *step from a table (see sl_adamw_flat)
int sl_sgd_flat_lr(float* w, const float* g, float* mom, uint16_t* shadow, long n, const int* step,
                   const float* lr_tab, int lr_n, float mu, float wd, float gscale, hipStream_t stream) {
  if (n <= 0) return 0;
  if (!lr_tab || !flat_opt_ok(w, g, mom, nullptr, shadow, step, lr_tab, lr_n)) return -1;
  const FlatOpt o = {step, lr_tab, lr_n - 1, 0.f, mu, wd, gscale, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  hipLaunchKernelGGL(opt_flat_kernel<false>, dim3(grid_for(n, 4)), dim3(256), 0, stream, w, g, mom,
                     static_cast<float*>(nullptr), shadow, n, o);
  SL_CHECK_LAUNCH();
  return 0;
}

// fp64 partials sl_clip_grad_norm needs for a vector of n floats (its grid; 0 for n <= 0)
int sl_clip_grad_partials(long n) { return n <= 0 ? 0 : clip_blocks(n); }

// g *= min(1, max_norm / (||g||_2 + 1e-6)) over g[0, n) in place, *norm_out = ||g||_2 before
// the scaling (max_norm = inf: measured, never scaled).  partials: scratch, rewritten whole by
// every call.
int sl_clip_grad_norm(float* g, long n, float max_norm, double* partials, int n_partials, float* norm_out,
                      hipStream_t stream) {
  if (n <= 0) return 0;
  if (!g || ((uintptr_t)g & 15) || !partials || ((uintptr_t)partials & 7) || !norm_out) return -1;
  if (!(max_norm > 0.f)) return -1;
  const int blocks = clip_blocks(n);
  if (n_partials < blocks) return -1;
  hipLaunchKernelGGL(clip_sumsq_kernel, dim3(blocks), dim3(CLIP_WG), 0, stream, g, n, partials);
  SL_CHECK_LAUNCH();
  hipLaunchKernelGGL(clip_scale_kernel, dim3(blocks), dim3(CLIP_WG), 0, stream, g, n, max_norm, partials, norm_out);
  SL_CHECK_LAUNCH();
  return 0;
}

// dst[0, n) = add ? dst + src : src for two ranges that do not overlap (the caller's contract),
// each 4-byte aligned.  The grid depends on n alone.
int sl_accum_flat(float* dst, const float* src, long n, int add, hipStream_t stream) {
  if (n <= 0) return 0;
  if (!dst || !src || (((uintptr_t)dst | (uintptr_t)src) & 3)) return -1;
  long head = (long)((16 - ((uintptr_t)dst & 15)) & 15) / 4;  // floats before dst's next 16-byte boundary
  if (head > n) head = n;
  const dim3 grid(grid_for(n, 4)), wg(256);
  if (((uintptr_t)(src + head) & 15) == 0) {
    hipLaunchKernelGGL(accum_flat_kernel<true>, grid, wg, 0, stream, dst, src, n, (int)head, add);
  } else {
    hipLaunchKernelGGL(accum_flat_kernel<false>, grid, wg, 0, stream, dst, src, n, (int)head, add);
  }
  SL_CHECK_LAUNCH();
  return 0;
}

// ema[0, n) += omd * (w - ema) with omd = omd_tab[min(*step, tab_n - 1)], then *step += 1, in one
// launch (ema_flat_kernel).  ema and w are whole 16-byte-aligned allocations that do not overlap;
// *ticket is 0 between launches.  The grid depends on n alone.
int sl_ema_flat(float* ema, const float* w, long n, int* step, unsigned* ticket, const float* omd_tab, int tab_n,
                hipStream_t stream) {
  if (n <= 0) return 0;
  if (!ema || !w || !step || !ticket || !omd_tab || tab_n < 1) return -1;
  if (((uintptr_t)ema | (uintptr_t)w) & 15) return -1;
  if (((uintptr_t)step | (uintptr_t)ticket | (uintptr_t)omd_tab) & 3) return -1;
  hipLaunchKernelGGL(ema_flat_kernel, dim3(grid_for(n, 4)), dim3(256), 0, stream, ema, w, n, step, ticket, omd_tab,
                     tab_n - 1);
  SL_CHECK_LAUNCH();
  return 0;
}

int sl_to_bf16(const float* src, uint16_t* dst, long n, hipStream_t stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(to_bf16_kernel, dim3(grid_for(n, 1)), dim3(256), 0, stream, src, dst, n);
  SL_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"

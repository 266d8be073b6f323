// Shared CDNA4 (gfx950) helpers for the serverless_learn_amd kernels.
//
// Everything here targets wave64 / MFMA 16x16x32 bf16.  Fragment maps
// (cdna_hip_programming.md §3; a wrong map moves or mixes output elements, which the
// element-exact integer cases of tests/test_conv_exact_gpu.py catch for every convolution
// kernel, and the logits / gradient references of tests/test_mlp_fused_gpu.py for the MLP):
//   A frag  : lane l holds A[row = l&15][k = 8*(l>>4) + j], j = 0..7
//   B frag  : lane l holds B[k = 8*(l>>4) + j][col = l&15]
//   C/D     : lane l holds C[row = 4*(l>>4) + r][col = l&15], r = 0..3
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

typedef __bf16 bf16x8_t __attribute__((ext_vector_type(8)));
typedef short short8_t __attribute__((ext_vector_type(8)));
typedef short short4_t __attribute__((ext_vector_type(4)));
typedef float floatx4_t __attribute__((ext_vector_type(4)));
typedef float floatx16_t __attribute__((ext_vector_type(16)));
typedef _Float16 halfx8_t __attribute__((ext_vector_type(8)));

#define SL_LDS __attribute__((address_space(3)))

namespace sl {

__device__ __forceinline__ floatx4_t mfma16(const short8_t& a, const short8_t& b, const floatx4_t& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16((bf16x8_t)a, (bf16x8_t)b, c, 0, 0, 0);
}
// the same MFMA on fp16 operands (same cycles on gfx950)
__device__ __forceinline__ floatx4_t mfma16h(const short8_t& a, const short8_t& b, const floatx4_t& c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(halfx8_t, a), __builtin_bit_cast(halfx8_t, b), c,
                                                0, 0, 0);
}

// 32x32x16 forms: lane l holds A[row l&31][k 8(l>>5)+j], B[k 8(l>>5)+j][col l&31];
// C/D: lane l, register r holds C[row (r&3) + 8(r>>2) + 4(l>>5)][col l&31]
__device__ __forceinline__ floatx16_t mfma32(const short8_t& a, const short8_t& b, const floatx16_t& c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16((bf16x8_t)a, (bf16x8_t)b, c, 0, 0, 0);
}
__device__ __forceinline__ floatx16_t mfma32h(const short8_t& a, const short8_t& b, const floatx16_t& c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(halfx8_t, a), __builtin_bit_cast(halfx8_t, b), c,
                                                0, 0, 0);
}
// compile-time loop: fn(std::integral_constant<int, I>) for I in [I0, I1)
template <int I0, int I1, class Fn>
__device__ __forceinline__ void static_for(Fn&& fn) {
  if constexpr (I0 < I1) {
    fn(std::integral_constant<int, I0>{});
    static_for<I0 + 1, I1>(fn);
  }
}

// fp32 -> bf16 bits, round-to-nearest-even.  A plain cast lowers to the
// hardware v_cvt_pk_bf16_f32 on gfx950 (keeps NaN a NaN; MI355X_MICROARCH.md
// "Correctness boundaries"), far cheaper than integer rounding on the bits.
__device__ __forceinline__ uint16_t f2bf(float f) { return __builtin_bit_cast(uint16_t, (__bf16)f); }
__device__ __forceinline__ float bf2f(uint16_t h) { return __uint_as_float(((uint32_t)h) << 16); }

__device__ __forceinline__ uint32_t pack2(float a, float b) {
  typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
  bf16x2_t v = {(__bf16)a, (__bf16)b};
  return __builtin_bit_cast(uint32_t, v);
}

__device__ __forceinline__ floatx4_t zero4() { return floatx4_t{0.f, 0.f, 0.f, 0.f}; }

__device__ __forceinline__ short8_t zero8() {
  short8_t z;
#pragma unroll
  for (int i = 0; i < 8; ++i) z[i] = 0;
  return z;
}

// 16-byte global load of 8 bf16.
__device__ __forceinline__ short8_t ld8(const uint16_t* p) { return *reinterpret_cast<const short8_t*>(p); }

// 16-byte LDS load of 8 bf16 (ds_read_b128).
__device__ __forceinline__ short8_t lds8(const uint16_t* p) { return *reinterpret_cast<const short8_t*>(p); }

// Two transposed LDS reads (ds_read_b64_tr_b16) that build a B fragment
// from a row-major [k][n] bf16 image: rows k0..k0+7 of the lane's
// 8-row group, column n0 + (lane&15).  `ld` is the row stride in elements.
__device__ __forceinline__ short8_t lds_tr8(const uint16_t* base, int ld, int lane) {
  const int g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
  const uint16_t* a0 = base + (8 * g + q) * ld + 4 * p;
  const uint16_t* a1 = a0 + 4 * ld;
  short4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((SL_LDS short4_t*)(a0));
  short4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((SL_LDS short4_t*)(a1));
  short8_t r;
  r[0] = lo[0]; r[1] = lo[1]; r[2] = lo[2]; r[3] = lo[3];
  r[4] = hi[0]; r[5] = hi[1]; r[6] = hi[2]; r[7] = hi[3];
  return r;
}

// Unpack 8 bytes of uint8 pixels, normalise (x*a + b) and pack to bf16x8.
__device__ __forceinline__ short8_t u8x8_to_bf16(uint2 v, float a, float b) {
  short8_t r;
#pragma unroll
  for (int j = 0; j < 4; ++j) r[j] = (short)f2bf((float)((v.x >> (8 * j)) & 0xffu) * a + b);
#pragma unroll
  for (int j = 0; j < 4; ++j) r[4 + j] = (short)f2bf((float)((v.y >> (8 * j)) & 0xffu) * a + b);
  return r;
}

// XCD-aware bijective remap of a 1-D grid (cdna_hip_programming.md §5 T1):
// consecutive logical tiles land on the same XCD so they share its L2.
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7, idx = bid >> 3;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + idx;
}

// ---------------------------------------------------------------------------
// Contention-free cross-workgroup sums of n values (per-channel statistics).
// A thousand workgroups atomically adding into the same n words serialise on
// those words (MI355X_MICROARCH.md "Global float atomics", contention row), so
// each workgroup adds into replica (blockIdx % SL_REP) of a [SL_REP][n] array
// and a separate launch, rsum_fold_kernel (conv.hip, sl_rsum_fold), folds the replicas
// into out[n] once the producers are done: the kernel boundary orders the replica
// atomics for free.  The two in-kernel alternatives measured slower and were removed.
// Folding in the producer launch's last-arriving workgroup (one ticket per workgroup)
// makes every producer grow by about what its fold launch cost: ResNet-18 -1.3 %
// (profiles/r05_arrive; with a release fence per workgroup ~1 ms per step,
// profiles/r02_rsum).  Folding in each consumer's prologue costs every consumer
// workgroup a 16 KB fold, more than the launch it removes: -1.6 % (profiles/r05_cons,
// r06_cons).
// Buffer layout (rsum_floats(n) floats, replicas zeroed before the producers):
//   [SL_REP][n] replicas | [n] result | 4 pad
// ---------------------------------------------------------------------------
constexpr int SL_REP = 32;
__host__ __device__ constexpr long rsum_floats(int n) { return (long)(SL_REP + 1) * n + 4; }

// Deterministic build (SL_DETERMINISTIC=1, libslkernels_det.so, loaded when the
// SL_DETERMINISTIC env var is set): the float atomics' order varies from run to run, so
// every cross-workgroup sum is instead kept in 64-bit fixed point.  Integer addition is
// associative: the folded result is bit-identical for any workgroup order.
//
// One fixed-point scale cannot cover both a BatchNorm sum of squares over millions of
// pixels (|sum| up to ~1e10) and a tiny gradient sum, so each value v is added as a pair
// of int64 atomics (fix_add): hi = rn(v * 2^8), lo = rn((v - hi / 2^8) * 2^40).  Each value
// is kept to 2^-41; hi wraps only past |sum| = 2^55 and lo (|lo| <= 2^31 per value) only
// past 2^32 values per entry.  The pairs sit interleaved at the start of the replica area
// ([n][2] int64 = 16 n bytes of the [SL_REP][n] floats).
#ifndef SL_DETERMINISTIC
#define SL_DETERMINISTIC 0
#endif
constexpr double SL_FIX_HI = 256.0;
constexpr double SL_FIX_LO = 1099511627776.0;  // 2^40
// launcher return code: a deterministic build needs a bigger split-K workspace for this call
// (the python wrapper grows it and calls again; the other builds fall back to atomics)
constexpr int SL_NEED_WS = 7;

// p[0] += hi(v), p[1] += lo(v)
__device__ __forceinline__ void fix_add(unsigned long long* p, float v) {
  const double d = (double)v;
  const double h = rint(d * SL_FIX_HI);
  atomicAdd(p, (unsigned long long)(long long)h);
  atomicAdd(p + 1, (unsigned long long)__double2ll_rn((d - h * (1.0 / SL_FIX_HI)) * SL_FIX_LO));
}
__host__ __device__ __forceinline__ double fix_value(const unsigned long long* p) {
  return (double)(long long)p[0] * (1.0 / SL_FIX_HI) + (double)(long long)p[1] * (1.0 / SL_FIX_LO);
}

__device__ __forceinline__ float* rsum_replica(float* buf, int n) {
  return SL_DETERMINISTIC ? buf : buf + (long)(blockIdx.x % SL_REP) * n;
}
__device__ __forceinline__ float* rsum_result(float* buf, int n) { return buf + (long)SL_REP * n; }
// add v to entry i of a replica returned by rsum_replica
__device__ __forceinline__ void rsum_add(float* rep, long i, float v) {
#if SL_DETERMINISTIC
  fix_add(reinterpret_cast<unsigned long long*>(rep) + 2 * i, v);
#else
  atomicAdd(rep + i, v);
#endif
}

}  // namespace sl

// Convolution kernel families, one bit each in the host-side record of what was launched since
// the last clear (conv.hip sl_conv_kernels_seen; names in ops/cnn.py KERNEL_FAMILIES).  Tests
// assert that a shape reached the kernel it is there for; nothing on the device reads this.
enum SlConvFamily {
  SL_KF_GEMM_64x64 = 0, SL_KF_GEMM_64x128, SL_KF_GEMM_128x64, SL_KF_GEMM_128x128,        // conv_gemm_kernel<.., false>
  SL_KF_GEMM_T_64x64, SL_KF_GEMM_T_64x128, SL_KF_GEMM_T_128x64, SL_KF_GEMM_T_128x128,    // ... transposed gathers
  SL_KF_BIG, SL_KF_BIG_T,            // conv_gemm_big_kernel
  SL_KF_WIDE, SL_KF_WIDE_T,          // conv_gemm_wide_kernel<., 256>
  SL_KF_WIDE128, SL_KF_WIDE128_T,    // conv_gemm_wide_kernel<., 128>
  SL_KF_DGRAD_S2,                    // conv_dgrad_s2_kernel<128, 64, 3, 2>
  SL_KF_DGRAD_S2_ALT,                // ... its SL_CONV_S2_WIDE tile shapes
  SL_KF_WGRAD_64, SL_KF_WGRAD_64_LEAN, SL_KF_WGRAD_128, SL_KF_WGRAD_128_LEAN,  // conv_wgrad_kernel
  SL_KF_WGRAD_BIG, SL_KF_WGRAD_BIG_LEAN,                                       // conv_wgrad_big_kernel
  SL_KF_HALO_FWD_C64, SL_KF_HALO_FWD_C8, SL_KF_HALO_DGRAD, SL_KF_HALO_WGRAD,   // conv3x3_halo.hip
  SL_KF_COUNT
};

#include "sl_api.h"  // every exported sl_* entry point, declared once

#define SL_CHECK_LAUNCH() \
  do { hipError_t _e = hipGetLastError(); if (_e != hipSuccess) return (int)_e; } while (0)

// Held-out evaluation metrics, accumulated on the device (ops/evalmetrics.py eval_reference is
// the specification; tests/test_eval_gpu.py compares every field exactly).
//
//   eval_accum_wide  the same over up to 256 classes, into int64 [8 + ncls * ncls] (further down)
//   eval_accum   fp32 logits [rows][ld] (ncls <= 16 classes), u8 labels, the fp32 per-row loss the
//                forward pass wrote  ->  adds into acc, int64 [8 + 256]:
//                  [0] n   [1] bad   [2] top1   [3] topk   [4] loss_fix   [5..7] zero
//                  [8 + 16 l + pred]  confusion (label l, prediction pred)
//
// The shape of softmax_ce_kernel (cnn_aux.hip): 256-thread workgroups, one row per 16-lane group,
// lane c holds z_c; the maximum, the first index that reaches it and the label's rank are cross-lane
// folds inside the group.  A workgroup keeps its counters and its 256-bin confusion histogram in LDS
// (integer LDS atomics) and, after a barrier, adds only its non-zero bins to acc with 64-bit integer
// global atomics.  Everything summed is an integer (the loss as rn(loss * 2^24)), so the result does
// not depend on the order of the workgroups: there is no SL_DETERMINISTIC branch, no float atomic, no
// ticket, no state between launches and nothing to fold afterwards.  The caller zeroes acc once per
// evaluation; rows >= n_valid (the zero padding of the last batch) are never read.
#include "common.h"

namespace {

constexpr int EV_CLS = 16;                  // classes per 16-lane group (and the confusion matrix's stride)
constexpr int EV_HEAD = 8;                  // counters in front of the confusion matrix
constexpr float EV_LOSS_MAX = 65536.f;      // |loss| at or past 2^16 marks a bad row
constexpr double EV_LOSS_FIX = 16777216.0;  // 2^24

// Inf or NaN, from the bits (no floating-point comparison for an optimisation to assume away)
__device__ __forceinline__ bool nonfinite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

__device__ __forceinline__ int group_or(int v) {
  v |= __shfl_xor(v, 1);
  v |= __shfl_xor(v, 2);
  v |= __shfl_xor(v, 4);
  v |= __shfl_xor(v, 8);
  return v;
}
__device__ __forceinline__ int group_sum(int v) {
  v += __shfl_xor(v, 1);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 4);
  v += __shfl_xor(v, 8);
  return v;
}

}  // namespace

__global__ __launch_bounds__(256) void eval_accum_kernel(const float* __restrict__ z, int ld,
                                                         const uint8_t* __restrict__ lab,
                                                         const float* __restrict__ loss, int n_valid, int ncls,
                                                         int topk, unsigned long long* __restrict__ acc) {
  __shared__ unsigned hist[EV_CLS * EV_CLS];
  __shared__ unsigned cnt[4];  // n, bad, top1, topk
  __shared__ unsigned long long lfix;
  const int tid = threadIdx.x, c = tid & 15, grp = tid >> 4;
  const int row = blockIdx.x * 16 + grp;
  hist[tid] = 0u;
  if (tid < 4) cnt[tid] = 0u;
  if (tid == 0) lfix = 0ull;
  __syncthreads();
  if (row < n_valid) {  // (the same for all 16 lanes of a group: the folds below stay inside it)
    const bool live = c < ncls;
    const float v = live ? z[(long)row * ld + c] : -INFINITY;
    const int nf = group_or(live && nonfinite(v) ? 1 : 0);
    float mx = v;
    mx = fmaxf(mx, __shfl_xor(mx, 1));
    mx = fmaxf(mx, __shfl_xor(mx, 2));
    mx = fmaxf(mx, __shfl_xor(mx, 4));
    mx = fmaxf(mx, __shfl_xor(mx, 8));
    int idx = v == mx ? c : 16;  // the lowest index among the maxima (softmax_ce_kernel's tie rule)
    idx = min(idx, __shfl_xor(idx, 1));
    idx = min(idx, __shfl_xor(idx, 2));
    idx = min(idx, __shfl_xor(idx, 4));
    idx = min(idx, __shfl_xor(idx, 8));
    int l = lab[row];
    l = l < ncls ? l : 0;
    const float zl = __shfl(v, (tid & 63 & ~15) | l);
    // classes ranked ahead of the label: a larger logit, or an equal one at a lower index
    const int rank = group_sum(live && (v > zl || (v == zl && c < l)) ? 1 : 0);
    if (c == 0) {
      const float lo = loss[row];
      atomicAdd(&cnt[0], 1u);
      if (nf || nonfinite(lo) || fabsf(lo) >= EV_LOSS_MAX) {
        atomicAdd(&cnt[1], 1u);  // a bad row counts in n and bad only
      } else {
        // all logits finite: mx is one of them, so idx < ncls
        if (rank == 0) atomicAdd(&cnt[2], 1u);
        if (rank < topk) atomicAdd(&cnt[3], 1u);
        atomicAdd(&hist[EV_CLS * l + idx], 1u);
        atomicAdd(&lfix, (unsigned long long)__double2ll_rn((double)lo * EV_LOSS_FIX));
      }
    }
  }
  __syncthreads();
  const unsigned h = hist[tid];
  if (h) atomicAdd(acc + EV_HEAD + tid, (unsigned long long)h);
  if (tid < 4 && cnt[tid]) atomicAdd(acc + tid, (unsigned long long)cnt[tid]);
  if (tid == 4 && lfix) atomicAdd(acc + 4, lfix);
}

// The same metrics over up to 256 classes, in the row layout of softmax_ce_wide_kernel (cnn_aux.hip):
// one row on a whole wave, lane c holds the four adjacent classes 4c .. 4c + 3 (one 16-B load where
// every row starts on a 16-B boundary, VEC, and guarded dword loads otherwise), the folds are
// 64-lane butterflies.  A wave takes EVW_ROWS consecutive rows.  acc is int64 [8 + ncls * ncls] with
// the confusion matrix at stride ncls: a 65,536-bin histogram does not fit in LDS, so lane 0 adds a
// good row's bin straight to acc (one 64-bit integer global atomic per good row).  The five
// counters are kept in the wave's registers, folded through LDS per workgroup and leave as at most
// five 64-bit integer atomics.  Integers only: no float atomic, no ticket, any workgroup order.
constexpr int EVW_ROWS = 8;  // rows per wave; a workgroup has four waves

template <bool VEC>
__global__ __launch_bounds__(256) void eval_accum_wide_kernel(const float* __restrict__ z, int ld,
                                                              const uint8_t* __restrict__ lab,
                                                              const float* __restrict__ loss, int n_valid, int ncls,
                                                              int topk, unsigned long long* __restrict__ acc) {
  __shared__ unsigned cnt[4];  // n, bad, top1, topk
  __shared__ unsigned long long lfix;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c0 = 4 * lane;
  if (tid < 4) cnt[tid] = 0u;
  if (tid == 0) lfix = 0ull;
  __syncthreads();
  unsigned n = 0u, bad = 0u, top1 = 0u, topk_n = 0u;
  unsigned long long fix = 0ull;
  const int row0 = (blockIdx.x * 4 + wave) * EVW_ROWS;
  for (int i = 0; i < EVW_ROWS; ++i) {
    const int row = row0 + i;
    if (row >= n_valid) break;  // (the same for all 64 lanes)
    const float* zr = z + (long)row * ld;
    float v[4];
    if constexpr (VEC) {
      // ncls % 4 == 0: a lane's four classes are all inside the row or all outside it
      if (c0 < ncls) {
        const float4 t = *reinterpret_cast<const float4*>(zr + c0);
        v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
      } else {
        v[0] = v[1] = v[2] = v[3] = -INFINITY;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = c0 + j < ncls ? zr[c0 + j] : -INFINITY;
    }
    bool nfl = false;
#pragma unroll
    for (int j = 0; j < 4; ++j) nfl |= c0 + j < ncls && nonfinite(v[j]);
    const bool nf = __ballot(nfl) != 0ull;
    float mx = fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3]));
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) mx = fmaxf(mx, __shfl_xor(mx, m));
    int idx = 256;  // the lowest index among the maxima (softmax_ce_kernel's tie rule)
#pragma unroll
    for (int j = 3; j >= 0; --j) idx = (c0 + j < ncls && v[j] == mx) ? c0 + j : idx;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) idx = min(idx, __shfl_xor(idx, m));
    int l = lab[row];
    l = l < ncls ? l : 0;
    const int jl = l & 3;
    const float zl = __shfl(jl == 0 ? v[0] : jl == 1 ? v[1] : jl == 2 ? v[2] : v[3], l >> 2);
    // classes ranked ahead of the label: a larger logit, or an equal one at a lower index
    int rank = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) rank += (c0 + j < ncls && (v[j] > zl || (v[j] == zl && c0 + j < l))) ? 1 : 0;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) rank += __shfl_xor(rank, m);
    if (lane == 0) {
      const float lo = loss[row];
      n += 1u;
      if (nf || nonfinite(lo) || fabsf(lo) >= EV_LOSS_MAX) {
        bad += 1u;  // a bad row counts in n and bad only
      } else {
        // all logits finite: mx is one of them, so idx < ncls
        top1 += rank == 0 ? 1u : 0u;
        topk_n += rank < topk ? 1u : 0u;
        fix += (unsigned long long)__double2ll_rn((double)lo * EV_LOSS_FIX);
        atomicAdd(acc + EV_HEAD + (long)l * ncls + idx, 1ull);
      }
    }
  }
  if (lane == 0 && n) {
    atomicAdd(&cnt[0], n);
    if (bad) atomicAdd(&cnt[1], bad);
    if (top1) atomicAdd(&cnt[2], top1);
    if (topk_n) atomicAdd(&cnt[3], topk_n);
    if (fix) atomicAdd(&lfix, fix);
  }
  __syncthreads();
  if (tid < 4 && cnt[tid]) atomicAdd(acc + tid, (unsigned long long)cnt[tid]);
  if (tid == 4 && lfix) atomicAdd(acc + 4, lfix);
}

extern "C" {

// acc: device int64 [8 + ncls * ncls], added into (1 <= ncls <= 256; the confusion matrix at stride ncls).
int sl_eval_accum_wide(const float* logits, int ld, const uint8_t* lab, const float* loss_rows, int rows, int n_valid,
                       int ncls, int topk, long long* acc, hipStream_t stream) {
  if (ncls < 1 || ncls > 256 || ld < ncls || topk < 1 || topk > ncls) return -1;
  if (rows < 0 || n_valid < 0 || n_valid > rows || rows > (1 << 22)) return -1;
  if (n_valid == 0) return 0;
  if (!logits || !lab || !loss_rows || !acc) return -2;
  const int per_wg = 4 * EVW_ROWS;
  const dim3 grid((n_valid + per_wg - 1) / per_wg), block(256);
  auto* a = reinterpret_cast<unsigned long long*>(acc);
  if (ncls % 4 == 0 && ld % 4 == 0 && ((uintptr_t)logits & 15) == 0)
    hipLaunchKernelGGL(eval_accum_wide_kernel<true>, grid, block, 0, stream, logits, ld, lab, loss_rows, n_valid, ncls,
                       topk, a);
  else
    hipLaunchKernelGGL(eval_accum_wide_kernel<false>, grid, block, 0, stream, logits, ld, lab, loss_rows, n_valid,
                       ncls, topk, a);
  SL_CHECK_LAUNCH();
  return 0;
}

// acc: device int64 [8 + 256], added into.  Rows [0, n_valid) of the `rows` the buffers hold take part.
int sl_eval_accum(const float* logits, int ld, const uint8_t* lab, const float* loss_rows, int rows, int n_valid,
                  int ncls, int topk, long long* acc, hipStream_t stream) {
  if (ncls < 1 || ncls > EV_CLS || ld < ncls || topk < 1 || topk > ncls) return -1;
  if (rows < 0 || n_valid < 0 || n_valid > rows || rows > (1 << 22)) return -1;
  if (n_valid == 0) return 0;
  if (!logits || !lab || !loss_rows || !acc) return -2;
  hipLaunchKernelGGL(eval_accum_kernel, dim3((n_valid + 15) / 16), dim3(256), 0, stream, logits, ld, lab, loss_rows,
                     n_valid, ncls, topk, reinterpret_cast<unsigned long long*>(acc));
  SL_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"

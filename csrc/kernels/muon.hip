// K5g -- Muon (momentum orthogonalised by Newton-Schulz) over the ResNet trainers' flat parameter
// vector.  Every conv filter bank but the stem is the matrix W[m = cout][n = k k cin] that the flat
// vector already stores row-major; its update is the momentum matrix pushed towards the nearest
// semi-orthogonal matrix by `steps` Newton-Schulz iterations in bf16 with fp32 accumulation:
//     mom = fma(mu, mom, g);  u = nesterov ? fma(mu, mom, g) : mom;  X = bf16(u / (||u||_F + 1e-7))
//     (tall tensors, m > n, are worked on transposed: every GEMM below sees rows <= cols)
//     A = bf16(X X^T);  B = bf16(b A + c A A);  X = bf16(a X + B X)        (a, b, c) = NS_A/B/C
//     w = w (1 - lr r wd) - lr r sqrt(max(1, m / n)) O                     O: the last X
// and everything else in the vector follows the grouped momentum-SGD rule of
// opt_flat_groups_kernel bit for bit.  Semantics and the host-side plan:
// serverless_learn_amd/ops/optim.py muon_update / newton_schulz / muon_plan.
//
// All launches are grouped over every Muon tensor through tile tables the plan builds once, and
// ordered by their launch boundaries alone: no atomics, no tickets, no state between calls, so
// the bits are the same from call to call, in both builds and on every rank, and a captured
// graph replays them.
//   sl_muon_prep   muon_mom_kernel: one workgroup per 4096-element chunk (a Muon tensor is a whole
//                  number of them: both sides are multiples of 64) updates the momentum and
//                  writes the chunk's fp64 sum of u^2 in a fixed order.  muon_x0_kernel: one
//                  workgroup per 64 x 64 tile of the wide-orientation X folds its tensor's chunk
//                  sums (every wave the same fixed order), scales u in fp64 and writes the bf16
//                  tile through LDS, transposing the tall tensors there.
//   sl_muon_gram   muon_gram_kernel: 64 x 64 tiles on or below the diagonal, times split-K
//                  slices of at most `kslice` columns; both MFMA operands are rows of X, so
//                  fragments are 16-byte global loads with no LDS.  fp32 partials go to a
//                  workspace; muon_fold_kernel adds them in slice order, rounds once and writes
//                  the tile and its mirror.
//   sl_muon_poly   the same row x row tile product on the symmetric A (A A = A A^T), one
//                  rounding of b A + c acc in the epilogue.
//   sl_muon_apply  64 x 64 tiles of X' = a X + B X.  B's rows are the K-contiguous operand
//                  (global fragments); X's reduction index is its row index, so 64 x 64 slabs of
//                  it are staged in LDS (the next slab's global loads in flight under the MFMAs)
//                  and read with ds_read_b64_tr_b16 (lds_tr8).  The a X term is picked out of
//                  the staged slab whose rows are the output tile's.
//   sl_sgd_flat_muon  the walk, grid and shadow store of lars_update_kernel.
//
// One tile shape, 64 x 64 with four waves of 32 x 32, serves every tensor because 64 is the
// granularity of the shapes (layer1's banks are 64 x 576); it was chosen for that, not measured
// against the 128 x 128 tiles a 512-row tensor could also take.
#include "common.h"

using namespace sl;

constexpr int MU_TILE = 64;
constexpr int MU_CHUNK = MU_TILE * MU_TILE;  // elements per chunk of the momentum launch (ops/optim.py MUON_CHUNK)
constexpr int MU_WG = 256;
constexpr int MU_VPL = MU_CHUNK / (4 * MU_WG);  // float4 per lane and array
constexpr int MU_MAX_SIDE = 512;                // the working (wide-orientation) row count's limit
constexpr int MU_LD = MU_TILE + 8;              // LDS row stride in bf16: 144 bytes, 16-byte aligned rows
constexpr float NS_A = 3.4445f, NS_B = -4.7750f, NS_C = 2.0315f;
constexpr double MU_EPS = 1e-7;

// int32 [T][12], ops/optim.py MuonPlan.tensors.  m x n is the tensor as the flat vector stores it
// at `off`; the work buffers hold it as rows() x cols() at xoff, its Gram matrices as rows() x
// rows() at aoff, its split-K partials as [slices][rows()][rows()] fp32 at poff.
struct MuonTensor {
  int off, m, n, transposed, xoff, aoff, poff, slices, chunk0, chunks, kslice, pad;
  __host__ __device__ int rows() const { return transposed ? n : m; }
  __host__ __device__ int cols() const { return transposed ? m : n; }
};
static_assert(sizeof(MuonTensor) == 48, "the plan's rows are twelve int32");

__device__ __forceinline__ float muon_u(float mu, float m_new, float g, int nesterov) {
  return nesterov ? fmaf(mu, m_new, g) : m_new;
}

// chunks[c]: the offset of MU_CHUNK elements inside one Muon tensor (16-byte aligned: tensors
// start on 64-element boundaries).  Lane l of round k takes float4 l + 256 k.  Fold as
// lars_norms_kernel: per lane in element order, xor shuffles, the four waves in wave order.
__global__ __launch_bounds__(MU_WG) void muon_mom_kernel(const float* __restrict__ g, float* __restrict__ mom,
                                                         const int* __restrict__ chunks, float mu, int nesterov,
                                                         double* __restrict__ partials) {
  __shared__ double lds[MU_WG / 64];
  const long base = chunks[blockIdx.x];
  const float4* gp = reinterpret_cast<const float4*>(g + base);
  float4* mp = reinterpret_cast<float4*>(mom + base);
  const int lane = threadIdx.x;
  float4 gv[MU_VPL], mv[MU_VPL];
#pragma unroll
  for (int k = 0; k < MU_VPL; ++k) gv[k] = gp[lane + k * MU_WG];
#pragma unroll
  for (int k = 0; k < MU_VPL; ++k) mv[k] = mp[lane + k * MU_WG];
  double acc = 0.0;
#pragma unroll
  for (int k = 0; k < MU_VPL; ++k) {
    const float ga[4] = {gv[k].x, gv[k].y, gv[k].z, gv[k].w};
    float ma[4] = {mv[k].x, mv[k].y, mv[k].z, mv[k].w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      ma[j] = fmaf(mu, ma[j], ga[j]);
      const double u = muon_u(mu, ma[j], ga[j], nesterov);
      acc += u * u;  // (exact product, one fp64 rounding)
    }
    mp[lane + k * MU_WG] = make_float4(ma[0], ma[1], ma[2], ma[3]);
  }
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) acc += __shfl_xor(acc, s);
  if ((lane & 63) == 0) lds[lane >> 6] = acc;
  __syncthreads();
  if (lane == 0) {
    double t = lds[0];
#pragma unroll
    for (int v = 1; v < MU_WG / 64; ++v) t += lds[v];
    partials[blockIdx.x] = t;
  }
}

// tiles[b] = (tensor, row tile i, column tile j, -) of the wide-orientation X.  Every wave folds
// the tensor's chunk sums in the same order (lane l takes chunks l, l + 64, ...; then the xor
// tree), so all lanes hold the same ||u||^2 and no barrier is needed before the scale.
__global__ __launch_bounds__(MU_WG) void muon_x0_kernel(const float* __restrict__ g, const float* __restrict__ mom,
                                                        const MuonTensor* __restrict__ tensors,
                                                        const int4* __restrict__ tiles,
                                                        const double* __restrict__ partials, float mu, int nesterov,
                                                        uint16_t* __restrict__ x0, float* __restrict__ norms) {
  __shared__ __attribute__((aligned(16))) uint16_t T[MU_TILE * MU_LD];
  const int4 tl = tiles[blockIdx.x];
  const MuonTensor mt = tensors[tl.x];
  const int tid = threadIdx.x;
  double ss = 0.0;
  for (int c = tid & 63; c < mt.chunks; c += 64) ss += partials[mt.chunk0 + c];
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) ss += __shfl_xor(ss, s);
  const double nrm = sqrt(ss), inv = 1.0 / (nrm + MU_EPS);
  if (tl.y == 0 && tl.z == 0 && tid == 0) norms[tl.x] = (float)nrm;
  // the source tile: wide tile (i, j) of a tall tensor is source tile (j, i), transposed
  const int sr0 = (mt.transposed ? tl.z : tl.y) * MU_TILE, sc0 = (mt.transposed ? tl.y : tl.z) * MU_TILE;
  const long src = (long)mt.off + (long)sr0 * mt.n + sc0;
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    const int r = (tid >> 4) + 16 * p, c = (tid & 15) * 4;
    const float4 gv = *reinterpret_cast<const float4*>(g + src + (long)r * mt.n + c);
    const float4 mv = *reinterpret_cast<const float4*>(mom + src + (long)r * mt.n + c);
    const float ga[4] = {gv.x, gv.y, gv.z, gv.w}, ma[4] = {mv.x, mv.y, mv.z, mv.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const uint16_t x = f2bf((float)((double)muon_u(mu, ma[j], ga[j], nesterov) * inv));
      if (mt.transposed) T[(c + j) * MU_LD + r] = x;
      else T[r * MU_LD + c + j] = x;
    }
  }
  __syncthreads();
  const int ld = mt.cols();
  uint16_t* dst = x0 + mt.xoff + (long)tl.y * MU_TILE * ld + tl.z * MU_TILE;
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int idx = tid + p * MU_WG, r = idx >> 3, sg = (idx & 7) * 8;
    *reinterpret_cast<short8_t*>(dst + (long)r * ld + sg) = lds8(T + r * MU_LD + sg);
  }
}

// acc += P[row0 .. +32][k0 .. k1) . P[col0 .. +32][k0 .. k1)^T for one wave: 2 x 2 fragments of
// 16 x 16, K in steps of 32.  Both operands are rows of the row-major P (stride ld), so the A
// fragment of lane l is the 16 bytes at P[row0 + (l & 15)][k + 8 (l >> 4)] and the B fragment the
// same of the column tile's rows.  k1 - k0 is a multiple of 64.
__device__ __forceinline__ void muon_nt(const uint16_t* __restrict__ P, int ld, int row0, int col0, int k0, int k1,
                                        floatx4_t (&acc)[2][2], int lane) {
  const uint16_t* ap = P + (long)(row0 + (lane & 15)) * ld + 8 * (lane >> 4);
  const uint16_t* bp = P + (long)(col0 + (lane & 15)) * ld + 8 * (lane >> 4);
#pragma unroll 2
  for (int k = k0; k < k1; k += 32) {
    const short8_t a0 = ld8(ap + k), a1 = ld8(ap + 16L * ld + k);
    const short8_t b0 = ld8(bp + k), b1 = ld8(bp + 16L * ld + k);
    acc[0][0] = mfma16(a0, b0, acc[0][0]);
    acc[0][1] = mfma16(a0, b1, acc[0][1]);
    acc[1][0] = mfma16(a1, b0, acc[1][0]);
    acc[1][1] = mfma16(a1, b1, acc[1][1]);
  }
}

// tiles[b] = (tensor, i, j <= i, slice).  ws[poff + slice rows^2 + r rows + c] receives the
// slice's partial of A[r][c] for the tile's 64 x 64 elements.
__global__ __launch_bounds__(MU_WG) void muon_gram_kernel(const uint16_t* __restrict__ x,
                                                          const MuonTensor* __restrict__ tensors,
                                                          const int4* __restrict__ tiles, float* __restrict__ ws) {
  const int4 tl = tiles[blockIdx.x];
  const MuonTensor mt = tensors[tl.x];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m = mt.rows(), n = mt.cols();
  const int r0 = tl.y * MU_TILE + (wave >> 1) * 32, c0 = tl.z * MU_TILE + (wave & 1) * 32;
  const int k0 = tl.w * mt.kslice, k1 = k0 + mt.kslice < n ? k0 + mt.kslice : n;
  floatx4_t acc[2][2] = {{zero4(), zero4()}, {zero4(), zero4()}};
  muon_nt(x + mt.xoff, n, r0, c0, k0, k1, acc, lane);
  float* out = ws + mt.poff + (long)tl.w * m * m;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        out[(long)(r0 + 16 * i + 4 * (lane >> 4) + r) * m + c0 + 16 * j + (lane & 15)] = acc[i][j][r];
}

// tiles[b] = (tensor, i, j <= i, -): A[r][c] = A[c][r] = bf16(sum over slices, in slice order).
// A diagonal tile keeps its lower half only, so A is symmetric bit for bit.
__global__ __launch_bounds__(MU_WG) void muon_fold_kernel(const float* __restrict__ ws,
                                                          const MuonTensor* __restrict__ tensors,
                                                          const int4* __restrict__ tiles, uint16_t* __restrict__ a) {
  const int4 tl = tiles[blockIdx.x];
  const MuonTensor mt = tensors[tl.x];
  const int m = mt.rows();
  const float* in = ws + mt.poff;
  uint16_t* A = a + mt.aoff;
#pragma unroll 4
  for (int p = 0; p < MU_CHUNK / MU_WG; ++p) {
    const int idx = threadIdx.x + p * MU_WG;
    const int r = tl.y * MU_TILE + (idx >> 6), c = tl.z * MU_TILE + (idx & 63);
    if (c > r) continue;
    float s = in[(long)r * m + c];
    for (int q = 1; q < mt.slices; ++q) s += in[(long)q * m * m + (long)r * m + c];
    const uint16_t v = f2bf(s);
    A[(long)r * m + c] = v;
    A[(long)c * m + r] = v;
  }
}

// tiles[b] = (tensor, i, j, -), every tile: B = bf16(b A + c A A), with A A taken as A A^T.
__global__ __launch_bounds__(MU_WG) void muon_poly_kernel(const uint16_t* __restrict__ a,
                                                          const MuonTensor* __restrict__ tensors,
                                                          const int4* __restrict__ tiles, uint16_t* __restrict__ b) {
  const int4 tl = tiles[blockIdx.x];
  const MuonTensor mt = tensors[tl.x];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int m = mt.rows();
  const int r0 = tl.y * MU_TILE + (wave >> 1) * 32, c0 = tl.z * MU_TILE + (wave & 1) * 32;
  const uint16_t* A = a + mt.aoff;
  uint16_t* B = b + mt.aoff;
  floatx4_t acc[2][2] = {{zero4(), zero4()}, {zero4(), zero4()}};
  muon_nt(A, m, r0, c0, 0, m, acc, lane);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long e = (long)(r0 + 16 * i + 4 * (lane >> 4) + r) * m + c0 + 16 * j + (lane & 15);
        B[e] = f2bf(fmaf(NS_C, acc[i][j][r], NS_B * bf2f(A[e])));
      }
}

// tiles[b] = (tensor, i, j, -) of X': xout = bf16(a xin + B xin) on rows 64 i .., columns 64 j ..
__global__ __launch_bounds__(MU_WG) void muon_apply_kernel(const uint16_t* __restrict__ xin,
                                                           const uint16_t* __restrict__ b,
                                                           const MuonTensor* __restrict__ tensors,
                                                           const int4* __restrict__ tiles,
                                                           uint16_t* __restrict__ xout) {
  __shared__ __attribute__((aligned(16))) uint16_t T[MU_TILE * MU_LD];
  const int4 tl = tiles[blockIdx.x];
  const MuonTensor mt = tensors[tl.x];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m = mt.rows(), n = mt.cols();
  const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;
  const uint16_t* X = xin + mt.xoff + tl.z * MU_TILE;  // the column panel
  const uint16_t* bp = b + mt.aoff + (long)(tl.y * MU_TILE + wr + (lane & 15)) * m + 8 * (lane >> 4);
  const int sr[2] = {tid >> 3, (tid + MU_WG) >> 3}, sg = (tid & 7) * 8;  // this thread's two 16-byte pieces
  short8_t pre[2];
#pragma unroll
  for (int p = 0; p < 2; ++p) pre[p] = ld8(X + (long)sr[p] * n + sg);
  floatx4_t acc[2][2] = {{zero4(), zero4()}, {zero4(), zero4()}};
  float ax[2][2][4];
  const int kt_n = m / MU_TILE;
  for (int kt = 0; kt < kt_n; ++kt) {
    __syncthreads();  // the previous slab's fragments have been read
#pragma unroll
    for (int p = 0; p < 2; ++p) *reinterpret_cast<short8_t*>(T + sr[p] * MU_LD + sg) = pre[p];
    __syncthreads();
    if (kt + 1 < kt_n) {
#pragma unroll
      for (int p = 0; p < 2; ++p) pre[p] = ld8(X + (long)((kt + 1) * MU_TILE + sr[p]) * n + sg);
    }
    if (kt == tl.y) {  // this slab's rows are the output tile's: keep a X's X
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            ax[i][j][r] = bf2f(T[(wr + 16 * i + 4 * (lane >> 4) + r) * MU_LD + wc + 16 * j + (lane & 15)]);
    }
#pragma unroll
    for (int kk = 0; kk < MU_TILE; kk += 32) {
      const short8_t a0 = ld8(bp + kt * MU_TILE + kk), a1 = ld8(bp + 16L * m + kt * MU_TILE + kk);
      const short8_t b0 = lds_tr8(T + kk * MU_LD + wc, MU_LD, lane);
      const short8_t b1 = lds_tr8(T + kk * MU_LD + wc + 16, MU_LD, lane);
      acc[0][0] = mfma16(a0, b0, acc[0][0]);
      acc[0][1] = mfma16(a0, b1, acc[0][1]);
      acc[1][0] = mfma16(a1, b0, acc[1][0]);
      acc[1][1] = mfma16(a1, b1, acc[1][1]);
    }
  }
  uint16_t* out = xout + mt.xoff + (long)(tl.y * MU_TILE + wr) * n + tl.z * MU_TILE + wc;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        out[(long)(16 * i + 4 * (lane >> 4) + r) * n + 16 * j + (lane & 15)] =
            f2bf(fmaf(NS_A, ax[i][j][r], acc[i][j][r]));
}

// The update: lars_update_kernel's walk.  tmap[i >> 6] is the Muon tensor that owns element i or
// anything >= T for none.  A Muon element's momentum was written by muon_mom_kernel; it takes
//     lrr = lr r;  w = fma(-(lrr s_T), O, w fma(-lrr, wd, 1))      s_T = sqrt(max(1, m / n))
// with O read from the last X (un-transposing a tall tensor's).  Every other element runs
// opt_flat_groups_kernel's SGD rule with its contractions written out as there (float4 body:
// fma(g, gscale, wd_c w); scalar tail: fma(wd_c, w, g gscale); gscale arrives as a launch
// argument, 1, so that the compiler folds neither), so its bits are that launch's.
struct MuonOpt {
  const int* step;
  const float* lr_tab;
  int lr_last;
  float lr, mu, wd, wd_norm, wd_bias, gscale, ratio;
  const uint8_t* cls;
  const uint16_t* tmap;
  const MuonTensor* tensors;
  const uint16_t* o;  // the orthogonalised momentum, in the work buffers' layout
  int T;
};

__global__ __launch_bounds__(256) void muon_update_kernel(float* __restrict__ w, const float* __restrict__ g,
                                                          float* __restrict__ mom, uint16_t* __restrict__ shadow,
                                                          long n, MuonOpt o) {
  const int k = *o.step;
  const float lr = o.lr_tab ? o.lr_tab[k < 0 ? 0 : k < o.lr_last ? k : o.lr_last] : o.lr;
  const float lrr = lr * o.ratio, keep = fmaf(-lrr, o.wd, 1.f);
  auto decay_of = [&](long i) __attribute__((always_inline)) {
    const int c = o.cls[i >> 6];
    return c == 0 ? o.wd : c == 1 ? o.wd_norm : o.wd_bias;
  };
  auto sgd = [&](float& wj, float gj, float& mj, float wdc, bool tail) __attribute__((always_inline)) {
    float d = tail ? fmaf(wdc, wj, gj * o.gscale) : fmaf(gj, o.gscale, wdc * wj);
    d = fmaf(o.mu, mj, d);
    mj = d;
    wj = fmaf(-lr, d, wj);
  };
  // O of the `cnt` elements from flat index i on, all in one row of tensor mt
  auto ortho = [&](const MuonTensor& mt, long i, float* ov, int cnt) __attribute__((always_inline)) {
    const int e = (int)(i - mt.off), row = e / mt.n, col = e - row * mt.n;
    for (int q = 0; q < cnt; ++q)
      ov[q] = bf2f(mt.transposed ? o.o[mt.xoff + (long)(col + q) * mt.m + row] : o.o[mt.xoff + e + q]);
  };
  auto muon = [&](const MuonTensor& mt, float& wj, float ov) __attribute__((always_inline)) {
    const float s = sqrtf(fmaxf(1.f, (float)mt.m / (float)mt.n));
    wj = fmaf(-(lrr * s), ov, wj * keep);
  };
  const long stride = (long)gridDim.x * blockDim.x * 4;
  for (long i = ((long)blockIdx.x * blockDim.x + threadIdx.x) * 4; i < n; i += stride) {
    const int t = o.tmap[i >> 6];
    if (i + 4 <= n) {
      const float4 wv = *reinterpret_cast<const float4*>(w + i);
      float wa[4] = {wv.x, wv.y, wv.z, wv.w};
      if (t < o.T) {
        const MuonTensor mt = o.tensors[t];
        float ov[4];
        ortho(mt, i, ov, 4);
#pragma unroll
        for (int j = 0; j < 4; ++j) muon(mt, wa[j], ov[j]);
      } else {
        const float4 gv = *reinterpret_cast<const float4*>(g + i);
        const float4 mv = *reinterpret_cast<const float4*>(mom + i);
        const float ga[4] = {gv.x, gv.y, gv.z, gv.w};
        float ma[4] = {mv.x, mv.y, mv.z, mv.w};
        const float wdc = decay_of(i);
#pragma unroll
        for (int j = 0; j < 4; ++j) sgd(wa[j], ga[j], ma[j], wdc, false);
        *reinterpret_cast<float4*>(mom + i) = make_float4(ma[0], ma[1], ma[2], ma[3]);
      }
      *reinterpret_cast<float4*>(w + i) = make_float4(wa[0], wa[1], wa[2], wa[3]);
      if (shadow) {
        uint2 pk;
        pk.x = pack2(wa[0], wa[1]);
        pk.y = pack2(wa[2], wa[3]);
        *reinterpret_cast<uint2*>(shadow + i) = pk;
      }
    } else {
      for (long q = i; q < n; ++q) {  // (never a Muon element: those tensors are whole chunks)
        float wq = w[q], mq = mom[q];
        sgd(wq, g[q], mq, decay_of(q), true);
        w[q] = wq;
        mom[q] = mq;
        if (shadow) shadow[q] = f2bf(wq);
      }
    }
  }
}

// The host copy of the tensor table, which a launcher can read: both sides multiples of 64, the
// working row count at most MU_MAX_SIDE, offsets that keep every 16-byte access aligned.
static bool muon_tensors_ok(const int* th, int T) {
  if (!th || T < 1 || T >= 0xFFFF) return false;
  const MuonTensor* t = reinterpret_cast<const MuonTensor*>(th);
  for (int i = 0; i < T; ++i) {
    if (t[i].m < MU_TILE || t[i].n < MU_TILE || t[i].m % MU_TILE || t[i].n % MU_TILE) return false;
    if (t[i].transposed != (t[i].m > t[i].n) || t[i].rows() > MU_MAX_SIDE) return false;
    if (t[i].off < 0 || t[i].off % MU_TILE || t[i].xoff < 0 || t[i].xoff % 8 || t[i].aoff < 0 || t[i].aoff % 8) return false;
    if (t[i].poff < 0 || t[i].kslice < MU_TILE || t[i].kslice % MU_TILE) return false;
    if (t[i].slices != (t[i].cols() + t[i].kslice - 1) / t[i].kslice) return false;
    if (t[i].chunk0 < 0 || t[i].chunks != t[i].m / MU_TILE * (t[i].n / MU_TILE)) return false;
  }
  return true;
}

static bool muon_aligned(const void* p, unsigned mask) { return p && !((uintptr_t)p & mask); }

extern "C" {

// the plan's chunk size: ops/optim.py checks its MUON_CHUNK against this one
int sl_muon_chunk() { return MU_CHUNK; }

// mom = fma(mu, mom, g) over the plan's chunks, partials[c] = the chunk's sum of u^2, then the
// scaled bf16 X0 of every Muon tensor into x0 (wide orientation) and ||u||_F into norms[t].
// chunks: int32 [n_chunks] offsets; tensors_h / tensors: the [T][12] table on the host and on the
// device; tiles: int32 [n_tiles][4] = (tensor, i, j, -), every 64 x 64 tile of every X.
int sl_muon_prep(const float* g, float* mom, const int* chunks, int n_chunks, float mu, int nesterov,
                 double* partials, const int* tensors_h, const int* tensors, int T, const int* tiles, int n_tiles,
                 uint16_t* x0, float* norms, hipStream_t stream) {
  if (!muon_aligned(g, 15) || !muon_aligned(mom, 15) || !muon_aligned(chunks, 3) || !muon_aligned(partials, 7)) return -1;
  if (!muon_aligned(tensors, 15) || !muon_aligned(tiles, 15) || !muon_aligned(x0, 15) || !muon_aligned(norms, 3)) return -1;
  if (n_chunks < 1 || n_tiles < 1 || !(mu >= 0.f) || !muon_tensors_ok(tensors_h, T)) return -1;
  hipLaunchKernelGGL(muon_mom_kernel, dim3(n_chunks), dim3(MU_WG), 0, stream, g, mom, chunks, mu, nesterov ? 1 : 0,
                     partials);
  hipLaunchKernelGGL(muon_x0_kernel, dim3(n_tiles), dim3(MU_WG), 0, stream, g, mom,
                     reinterpret_cast<const MuonTensor*>(tensors), reinterpret_cast<const int4*>(tiles), partials, mu,
                     nesterov ? 1 : 0, x0, norms);
  SL_CHECK_LAUNCH();
  return 0;
}

// a = bf16(x x^T) per tensor.  gtiles: [n_gtiles][4] = (tensor, i, j <= i, slice); ttiles:
// [n_ttiles][4] = (tensor, i, j <= i, -); ws: the fp32 split-K partials.
int sl_muon_gram(const uint16_t* x, const int* tensors_h, const int* tensors, int T, const int* gtiles, int n_gtiles,
                 float* ws, const int* ttiles, int n_ttiles, uint16_t* a, hipStream_t stream) {
  if (!muon_aligned(x, 15) || !muon_aligned(tensors, 15) || !muon_aligned(gtiles, 15) || !muon_aligned(ws, 15)) return -1;
  if (!muon_aligned(ttiles, 15) || !muon_aligned(a, 15)) return -1;
  if (n_gtiles < 1 || n_ttiles < 1 || !muon_tensors_ok(tensors_h, T)) return -1;
  const MuonTensor* td = reinterpret_cast<const MuonTensor*>(tensors);
  hipLaunchKernelGGL(muon_gram_kernel, dim3(n_gtiles), dim3(MU_WG), 0, stream, x, td,
                     reinterpret_cast<const int4*>(gtiles), ws);
  hipLaunchKernelGGL(muon_fold_kernel, dim3(n_ttiles), dim3(MU_WG), 0, stream, ws, td,
                     reinterpret_cast<const int4*>(ttiles), a);
  SL_CHECK_LAUNCH();
  return 0;
}

// b = bf16(NS_B a + NS_C a a) per tensor.  tiles: [n_tiles][4] = (tensor, i, j, -), all of them.
int sl_muon_poly(const uint16_t* a, const int* tensors_h, const int* tensors, int T, const int* tiles, int n_tiles,
                 uint16_t* b, hipStream_t stream) {
  if (!muon_aligned(a, 15) || !muon_aligned(tensors, 15) || !muon_aligned(tiles, 15) || !muon_aligned(b, 15)) return -1;
  if (a == b || n_tiles < 1 || !muon_tensors_ok(tensors_h, T)) return -1;
  hipLaunchKernelGGL(muon_poly_kernel, dim3(n_tiles), dim3(MU_WG), 0, stream, a,
                     reinterpret_cast<const MuonTensor*>(tensors), reinterpret_cast<const int4*>(tiles), b);
  SL_CHECK_LAUNCH();
  return 0;
}

// xout = bf16(NS_A xin + b xin) per tensor.  tiles: sl_muon_prep's.
int sl_muon_apply(const uint16_t* xin, const uint16_t* b, const int* tensors_h, const int* tensors, int T,
                  const int* tiles, int n_tiles, uint16_t* xout, hipStream_t stream) {
  if (!muon_aligned(xin, 15) || !muon_aligned(b, 15) || !muon_aligned(tensors, 15) || !muon_aligned(tiles, 15)) return -1;
  if (!muon_aligned(xout, 15) || xin == xout || n_tiles < 1 || !muon_tensors_ok(tensors_h, T)) return -1;
  hipLaunchKernelGGL(muon_apply_kernel, dim3(n_tiles), dim3(MU_WG), 0, stream, xin, b,
                     reinterpret_cast<const MuonTensor*>(tensors), reinterpret_cast<const int4*>(tiles), xout);
  SL_CHECK_LAUNCH();
  return 0;
}

// The Muon update of w[0, n) at the learning rate lr_tab[min(*step, lr_n - 1)] (nullptr: lr).
// x0 / x1: the two work buffers; after `steps` iterations O is in x0 (steps even) or x1.  cls /
// tmap: one entry per 64 elements.  The caller advances *step after this launch.
int sl_sgd_flat_muon(float* w, const float* g, float* mom, uint16_t* shadow, long n, const int* step,
                     const float* lr_tab, int lr_n, float lr, float mu, float wd, float wd_norm, float wd_bias,
                     float gscale, float ratio, const uint8_t* cls, const uint16_t* tmap, const int* tensors_h,
                     const int* tensors, int T, const uint16_t* x0, const uint16_t* x1, int steps,
                     hipStream_t stream) {
  if (!muon_aligned(w, 15) || !muon_aligned(g, 15) || !muon_aligned(mom, 15) || !step || !cls) return -1;
  if (!muon_aligned(tmap, 1) || !muon_aligned(tensors, 15) || !muon_aligned(x0, 15) || !muon_aligned(x1, 15)) return -1;
  if ((shadow && ((uintptr_t)shadow & 7)) || n < 1 || (lr_tab && lr_n < 1) || steps < 1 || steps > 8) return -1;
  if (!(wd >= 0.f) || !(wd_norm >= 0.f) || !(wd_bias >= 0.f) || !(ratio > 0.f) || !(mu >= 0.f)) return -1;
  if (!muon_tensors_ok(tensors_h, T)) return -1;
  long blocks = (n + 1023) / 1024;  // (grid_for(n, 4) of elementwise.hip)
  if (blocks > 2048) blocks = 2048;
  const MuonOpt o = {step, lr_tab, lr_tab ? lr_n - 1 : 0, lr, mu, wd, wd_norm, wd_bias, gscale, ratio, cls, tmap,
                     reinterpret_cast<const MuonTensor*>(tensors), (steps & 1) ? x1 : x0, T};
  hipLaunchKernelGGL(muon_update_kernel, dim3((int)blocks), dim3(256), 0, stream, w, g, mom, shadow, n, o);
  SL_CHECK_LAUNCH();
  return 0;
}

}  // extern "C"

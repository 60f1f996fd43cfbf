// The fp32 matrix steps of the evaluation rows on v_mfma_f32_16x16x4_f32, stated once (device code only): the k-tile step over a
// k-major LDS image (mma_ktile), the two ways of summing k-tiles (ChainSum, TileKahanSum: DESIGN.md 4.4), the walk of one 64 x 64 tile
// with the caller's A rows and epilogue (tile_walk: the Inception convolution), its dense-row, + bias form that the CLIP towers', the
// compatibility scorer's, the ranking's and the Inception classifier's Linears run (gemm_tile), the one-wave-a-row LayerNorm (layernorm_row) and the max-pool update of the two convnets (pool_max).
// Users: clip.hip (clip_gemm_f32_kernel, clip_layernorm_kernel), eval_scores.hip (compat_gemm_f32_kernel, compat_ln_relu_kernel),
// eval_rank.hip (the ranking GEMM), lpips.hip (lpips_conv3x3_relu_kernel, lpips_finish_kernel, lpips_maxpool2x2_kernel),
// inception.hip (incep_conv_kernel: the im2col use of tile_walk; incep_fc_kernel, incep_pool_kernel).  fp32 in both storage builds; whether a * b + c contracts is the
// including file's -ffp-contract setting (Makefile), nothing here sets it.
#pragma once
#include "dfh_common.h"

namespace dfh {

// sum += x with the rounding error of the add carried in comp (Kahan); T: float or f32x4_t
template <class T>
DFH_DEVICE void kahan_add(T& sum, T& comp, const T x) {
  const T y = x - comp;
  const T s = sum + y;
  comp = (s - sum) - y;
  sum = s;
}

// torch's max-pool update: a NaN wins and stays
DFH_DEVICE float pool_max(float m, float v) { return (v > m || v != v) ? v : m; }

// KT k-rows of a k-major LDS image pair: per k-quad q the lane reads MF A and NF B fragment values at k-row 4 q + fk and issues
// MF x NF MFMAs into accumulator set q % NACC.  a / b: the lane's element of the first fragment at k-row 0; rows a_ld / b_ld floats
// apart (both 16 mod 32: the four k-rows of a fragment read fall on disjoint banks), A fragments a_frag_stride apart, B fragments 16.
template <int NACC, int MF, int NF, int KT>
DFH_DEVICE void mma_ktile(const float* a, int a_ld, int a_frag_stride, const float* b, int b_ld, int fk, f32x4_t (&t)[NACC][MF][NF]) {
#pragma unroll
  for (int kk = 0; kk < KT; kk += 4) {
    float av[MF], bv[NF];
#pragma unroll
    for (int i = 0; i < MF; ++i) av[i] = a[(kk + fk) * a_ld + i * a_frag_stride];
#pragma unroll
    for (int j = 0; j < NF; ++j) bv[j] = b[(kk + fk) * b_ld + 16 * j];
#pragma unroll
    for (int i = 0; i < MF; ++i)
#pragma unroll
      for (int j = 0; j < NF; ++j)
        t[(kk >> 2) % NACC][i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[j], t[(kk >> 2) % NACC][i][j], 0, 0, 0);
  }
}

template <int NACC, int MF, int NF>
DFH_DEVICE void zero_acc(f32x4_t (&t)[NACC][MF][NF]) {
#pragma unroll
  for (int q = 0; q < NACC; ++q)
#pragma unroll
    for (int i = 0; i < MF; ++i)
#pragma unroll
      for (int j = 0; j < NF; ++j) t[q][i][j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
}

// ------------------------------------------------------------------ the 64 x 64 tile of out[m][n] = sum_k A[m][k] W[n][k]
// Four waves, 32 x 32 each = 2 x 2 MFMA blocks, K in steps of 32.  Operand tiles sit k-major in LDS ([k][row], row stride 80 floats):
// a fragment read (lane -> row l % 16, k l / 16) touches 64 distinct banks, and the transposing store of a float4 along k writes
// consecutive rows of one k.
constexpr int GT_M = 64, GT_N = 64, GT_K = 32, GT_LD = 80;

// How a wave sums its k-tiles: tile(a, b, fk) takes one staged k-tile, at(i, j, r) is element r of block (i, j) of the result.
// ChainSum: one accumulator down all of K.  The rounding error of the chain grows like sqrt(K); the towers agree with the fp32
// reference class to summation-order noise (1e-6) under it.
struct ChainSum {
  f32x4_t acc[1][2][2];
  DFH_DEVICE ChainSum() { zero_acc(acc); }
  DFH_DEVICE void tile(const float* a, const float* b, int fk) { mma_ktile<1, 2, 2, GT_K>(a, GT_LD, 16, b, GT_LD, fk, acc); }
  DFH_DEVICE float at(int i, int j, int r) const { return acc[0][i][j][r]; }
};
// TileKahanSum: every k-tile is summed on its own into two fresh accumulators (even / odd k-quads: chains of four instructions), and
// (even + odd) is added to the running result with the compensated add, so the error does not grow with K.
struct TileKahanSum {
  f32x4_t sum[1][2][2], comp[1][2][2];
  DFH_DEVICE TileKahanSum() { zero_acc(sum); zero_acc(comp); }
  DFH_DEVICE void tile(const float* a, const float* b, int fk) {
    f32x4_t t[2][2][2];
    zero_acc(t);
    mma_ktile<2, 2, 2, GT_K>(a, GT_LD, 16, b, GT_LD, fk, t);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) kahan_add(sum[0][i][j], comp[0][i][j], t[0][i][j] + t[1][i][j]);
  }
  DFH_DEVICE float at(int i, int j, int r) const { return sum[0][i][j][r]; }
};

// The walk of one workgroup's tile (256 threads) whose origin is (m0, n0), stated once: two k-major LDS images, staging thread ->
// (row tile_stage_row(), k-quads tid / 64 and tid / 64 + 4), the next k-tile's global loads issued before the current tile's MFMAs
// (register prefetch), the k-tiles summed under Sum, and the walk over the C layout.  K is a multiple of 4.  The caller supplies
//   a_quad(k)  : the four A values at k .. k + 3 of ITS staging row (called for k < K only; beyond K the image holds zeros);
//   w_row      : the W row of its staging row, 16-byte aligned (read for k < K);
//   column(n)  : what the epilogue needs of column n < N, read once a column;
//   store(m, n, sum, column value) for every element with m < M, n < N.
// Which row a staging row beyond M / N reads is the caller's choice (the GEMMs and the conv clamp to the last one): such rows are
// never stored.  Row: the type of a row index (int for the GEMMs, long for the conv, whose rows are the pixels of a batch).
DFH_DEVICE int tile_stage_row() { return threadIdx.x & 63; }

template <class Sum, class Row, class AQuad, class Column, class Store>
DFH_DEVICE void tile_walk(Row m0, int n0, Row M, int N, int K, const float* __restrict__ w_row, AQuad a_quad, Column column, Store store) {
  __shared__ float As[GT_K * GT_LD];
  __shared__ float Ws[GT_K * GT_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
  const int srow = tile_stage_row(), sq = tid >> 6;
  float4 ra[2], rw[2];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int k = k0 + (sq + 4 * j) * 4;
      ra[j] = rw[j] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (k < K) {
        rw[j] = *(const float4*)(w_row + k);
        ra[j] = a_quad(k);
      }
    }
  };
  auto stash = [&]() {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int kk = (sq + 4 * j) * 4;
      As[(kk + 0) * GT_LD + srow] = ra[j].x; As[(kk + 1) * GT_LD + srow] = ra[j].y;
      As[(kk + 2) * GT_LD + srow] = ra[j].z; As[(kk + 3) * GT_LD + srow] = ra[j].w;
      Ws[(kk + 0) * GT_LD + srow] = rw[j].x; Ws[(kk + 1) * GT_LD + srow] = rw[j].y;
      Ws[(kk + 2) * GT_LD + srow] = rw[j].z; Ws[(kk + 3) * GT_LD + srow] = rw[j].w;
    }
  };
  Sum sum;
  const int fr = lane & 15, fk = lane >> 4;
  fetch(0);
  for (int k0 = 0; k0 < K; k0 += GT_K) {
    __syncthreads();                       // the previous tile's fragment reads are done
    stash();
    __syncthreads();
    if (k0 + GT_K < K) fetch(k0 + GT_K);
    sum.tile(As + wm + fr, Ws + wn + fr, fk);
  }
  // C layout of 16x16x4: acc[r] = C[4 * (lane / 16) + r][lane % 16]
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = n0 + wn + 16 * j + fr;
      if (n >= N) continue;
      const auto cv = column(n);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const Row m = m0 + wm + 16 * i + 4 * fk + r;
        if (m < M) store(m, n, sum.at(i, j, r), cv);
      }
    }
}

// gemm_tile is the dense-row, + bias form of the same walk and keeps a body of its own: written as a call of tile_walk its users measured
// 0.4 - 2.2 % slower on an MI355X under both formulations of the fetch that were tried (profiles/eval_tile_walk/bench_ab.txt, DESIGN.md
// 4.4), so the two bodies below and above must be changed together: same LDS images, staging, k loop and C-layout walk.
// One workgroup's tile (blockIdx.x: N tile, blockIdx.y: M tile; 256 threads): A rows lda floats apart, W [N][K] rows ldw apart, K a
// multiple of 4, rows 16-byte aligned.  The next k-tile's global loads are issued before the current tile's MFMAs (register prefetch);
// rows beyond M / N read the last row and are never stored.  store(m, n, value) is called for every in-range element with
// value = sum + bias[n] (bias may be null: + 0; it is read once a column).
// w_rows (null: W row n is row n): row n of the operand is W row w_rows[n], clamped into [0, w_row_count) before it addresses anything --
// the gather rides in the tile's own global loads (eval_rank.hip).  The null default folds away in the callers that do not pass it.
template <class Sum, class Store>
DFH_DEVICE void gemm_tile(const float* __restrict__ A, int lda, const float* __restrict__ W, int ldw, const float* __restrict__ bias, int M,
                          int N, int K, Store store, const int64_t* __restrict__ w_rows = nullptr, int w_row_count = 0) {
  __shared__ float As[GT_K * GT_LD];
  __shared__ float Ws[GT_K * GT_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.y * GT_M, n0 = blockIdx.x * GT_N;
  const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
  // staging: thread -> (row = tid % 64, k-quads tid / 64 and tid / 64 + 4)
  const int srow = tid & 63, sq = tid >> 6;
  const float* ap = A + (long)min(m0 + srow, M - 1) * lda;
  long wrow = min(n0 + srow, N - 1);
  if (w_rows) wrow = min(max(w_rows[wrow], (int64_t)0), (int64_t)w_row_count - 1);
  const float* wp = W + wrow * ldw;
  float4 ra[2], rw[2];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int k = k0 + (sq + 4 * j) * 4;
      ra[j] = k < K ? *(const float4*)(ap + k) : make_float4(0.f, 0.f, 0.f, 0.f);
      rw[j] = k < K ? *(const float4*)(wp + k) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto stash = [&]() {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int kk = (sq + 4 * j) * 4;
      As[(kk + 0) * GT_LD + srow] = ra[j].x; As[(kk + 1) * GT_LD + srow] = ra[j].y;
      As[(kk + 2) * GT_LD + srow] = ra[j].z; As[(kk + 3) * GT_LD + srow] = ra[j].w;
      Ws[(kk + 0) * GT_LD + srow] = rw[j].x; Ws[(kk + 1) * GT_LD + srow] = rw[j].y;
      Ws[(kk + 2) * GT_LD + srow] = rw[j].z; Ws[(kk + 3) * GT_LD + srow] = rw[j].w;
    }
  };
  Sum sum;
  const int fr = lane & 15, fk = lane >> 4;
  fetch(0);
  for (int k0 = 0; k0 < K; k0 += GT_K) {
    __syncthreads();                       // the previous tile's fragment reads are done
    stash();
    __syncthreads();
    if (k0 + GT_K < K) fetch(k0 + GT_K);
    sum.tile(As + wm + fr, Ws + wn + fr, fk);
  }
  // C layout of 16x16x4: acc[r] = C[4 * (lane / 16) + r][lane % 16]
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int n = n0 + wn + 16 * j + fr;
      if (n >= N) continue;
      const float bv = bias ? bias[n] : 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + wm + 16 * i + 4 * fk + r;
        if (m < M) store(m, n, sum.at(i, j, r) + bv);
      }
    }
}

// ------------------------------------------------------------------ LayerNorm over the last dim, fp32 in / out, one wave per row
// y[row][:] = LayerNorm(x[row * ldx : row * ldx + D]) * g + b, through max(., 0) when RELU; two-pass mean / biased variance like
// torch.nn.functional.layer_norm.  Four rows a 256-thread workgroup, D a multiple of 4, output rows dense.
template <bool RELU>
DFH_DEVICE void layernorm_row(const float* __restrict__ x, long ldx, const float* __restrict__ g, const float* __restrict__ b,
                              float* __restrict__ y, int M, int D, float eps) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= M) return;                    // whole waves leave: the shuffles below see 64 live lanes
  const float4* r = (const float4*)(x + (long)row * ldx);
  float s = 0.f;
  for (int c = lane; c < D / 4; c += 64) { const float4 v = r[c]; s += (v.x + v.y) + (v.z + v.w); }
  const float mean = wave_sum(s) / (float)D;
  float q = 0.f;
  for (int c = lane; c < D / 4; c += 64) {
    const float4 v = r[c];
    const float d0 = v.x - mean, d1 = v.y - mean, d2 = v.z - mean, d3 = v.w - mean;
    q += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
  }
  const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + eps);
  auto norm = [&](float v, float gg, float bb) {
    const float o = (v - mean) * rstd * gg + bb;
    return RELU ? fmaxf(o, 0.f) : o;
  };
  float4* o = (float4*)(y + (long)row * D);
  for (int c = lane; c < D / 4; c += 64) {
    const float4 v = r[c], gg = ((const float4*)g)[c], bb = ((const float4*)b)[c];
    o[c] = make_float4(norm(v.x, gg.x, bb.x), norm(v.y, gg.y, bb.y), norm(v.z, gg.z, bb.z), norm(v.w, gg.w, bb.w));
  }
}

}  // namespace dfh

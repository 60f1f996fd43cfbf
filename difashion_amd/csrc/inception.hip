// Inception v3 for FID and the Inception Score: pytorch_fid's FIDInceptionV3 (variant FID) and torchvision's
// inception_v3 under the reference's fine-tuned classifier (variant TV), as Evaluation/eval_utils.py:17-89, :137-337 and :339-406 run them.
//
// Replaces (arithmetic):
//   * F.interpolate(size=(299, 299), mode='bilinear', align_corners=False), 2 x - 1 and torchvision's transform_input: incep_prep_kernel;
//   * every BasicConv2d (conv without bias -> BatchNorm2d(eps 1e-3, running statistics) -> ReLU), whatever its filter, stride and
//     padding: ONE implicit GEMM on v_mfma_f32_16x16x4_f32 (incep_conv_kernel), rows = output pixels of the whole batch, K = taps x input
//     channels, BatchNorm as a per-channel scale / shift in the epilogue, written into a channel slice of the block's concatenation;
//   * the four 3 x 3 pools (incep_pool_kernel) and the global spatial mean (incep_mean_kernel<float>);
//   * fc + softmax (incep_fc_kernel over gemm_tile, incep_softmax_kernel), the per-image terms of the customised Inception Score
//     (incep_is_rows_kernel) and its split means (incep_is_splits_kernel);
//   * np.mean / np.cov of the float64 copy of the activations on v_mfma_f64_16x16x4_f64 (incep_mean_kernel<double>, incep_cov_kernel).
//
// Activations are NHWC fp32; fp32 (statistics: fp64) only, the same in both storage builds; no atomics; nothing is allocated here.  Every
// per-image value is a function of its image alone: an output element's products are summed in an order that depends on the layer only.
//
// Accumulation contract of the conv: K is walked in k-tiles of 32 (k = tap * C_in + channel) by the tile walk of f32_tile.h (tile_walk);
// each tile is summed in fresh accumulators and added to the running sum with a compensated add (TileKahanSum), so the rounding error
// does not grow with K.
//
// The host side plans the whole walk in one pure function (build_plan): a list of launches with kind, geometry, source / destination
// region, ldc and channel offset.  dfh_incep_forward runs exactly that list; dfh_incep_plan_* show it without a GPU.
//
// This file is compiled with -ffp-contract=off (Makefile): prep follows torch's separate fp32 ops.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <utility>

#include "../../include/difashion_hip.h"
#include "dfh_common.h"
#include "f32_tile.h"

namespace {

constexpr int THREADS = 256;
constexpr int SIDE = DFH_INCEP_SIDE, NBLOCK = DFH_INCEP_NUM_BLOCKS;
constexpr int TAP_C[NBLOCK] = {64, 192, 768, 2048};
constexpr int MAX_SIDE = 8192, MAX_CLASSES = 4096;
constexpr float BN_EPS = 1e-3f;
typedef __attribute__((ext_vector_type(4))) double f64x4_t;

// ------------------------------------------------------------------ prep: bilinear to 299 x 299 -> 2 x - 1 -> transform_input -> NHWC, 4 channels
// torch's source index and weights in fp32 (area_pixel_compute_source_index, align_corners=False): scale = float(in) / out,
// src = max((dst + 0.5f) * scale - 0.5f, 0), i0 = (int)src, i1 = min(i0 + 1, in - 1), l1 = src - i0, l0 = 1 - l1.  The multiply-add of src and
// of every weighted pair is ONE fused operation, as torch's CPU kernel is compiled (explicit fmaf: the file itself is built without
// contraction), so the indices, the weights and the interpolated values are torch's bit for bit
struct Axis { int i0, i1; float l0, l1; };
DFH_DEVICE Axis source_axis(int dst, int in, float scale) {
  float src = fmaf((float)dst + 0.5f, scale, -0.5f);
  src = src < 0.0f ? 0.0f : src;
  Axis a;
  a.i0 = (int)src;
  a.i1 = min(a.i0 + 1, in - 1);
  a.l1 = src - (float)a.i0;
  a.l0 = 1.0f - a.l1;
  return a;
}

struct Affine { float a[3], b[3]; };

__global__ __launch_bounds__(THREADS) void incep_prep_kernel(const float* __restrict__ src, float4* __restrict__ out, int H, int W, int OH, int OW,
                                                             int resize, int normalize, int affine, const Affine af, long total) {
  const long t = (long)blockIdx.x * THREADS + threadIdx.x;
  if (t >= total) return;
  const int ox = (int)(t % OW);
  long r = t / OW;
  const int oy = (int)(r % OH);
  const long img = r / OH;
  const float* s = src + img * 3 * (long)H * W;
  float v[3];
  if (resize) {
    const Axis ay = source_axis(oy, H, (float)H / (float)OH), ax = source_axis(ox, W, (float)W / (float)OW);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float* p = s + (long)c * H * W;
      const float top = fmaf(ax.l0, p[(long)ay.i0 * W + ax.i0], ax.l1 * p[(long)ay.i0 * W + ax.i1]);
      const float bot = fmaf(ax.l0, p[(long)ay.i1 * W + ax.i0], ax.l1 * p[(long)ay.i1 * W + ax.i1]);
      v[c] = fmaf(ay.l0, top, ay.l1 * bot);
    }
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = s[(long)c * H * W + (long)oy * W + ox];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (normalize) v[c] = 2.0f * v[c] - 1.0f;
    if (affine) v[c] = v[c] * af.a[c] + af.b[c];
  }
  out[t] = make_float4(v[0], v[1], v[2], 0.0f);
}

// ------------------------------------------------------------------ weights: torch [C_out][w_cin][KH][KW] -> [C_out][tap][C_in], BN -> scale / shift
__global__ __launch_bounds__(THREADS) void incep_pack_conv_kernel(const float* __restrict__ w, const float* __restrict__ bn_w,
                                                                  const float* __restrict__ bn_b, const float* __restrict__ bn_mean,
                                                                  const float* __restrict__ bn_var, float* __restrict__ packed, int w_cin, int cin,
                                                                  int taps, int C_out) {
  const long K = (long)taps * cin, total = K * C_out;
  const long t = (long)blockIdx.x * THREADS + threadIdx.x;
  if (t < total) {
    const int n = (int)(t / K);
    const int k = (int)(t - (long)n * K);
    const int tap = k / cin, c = k - tap * cin;
    packed[t] = c < w_cin ? w[((long)n * w_cin + c) * taps + tap] : 0.0f;      // channels beyond w_cin (the first layer's fourth): 0
  }
  if (t < C_out) {
    const float scale = bn_w[t] / sqrtf(bn_var[t] + BN_EPS);
    packed[total + t] = scale;
    packed[total + C_out + t] = bn_b[t] - bn_mean[t] * scale;
  }
}

// ------------------------------------------------------------------ out slice = relu(conv(x) * scale + shift), NHWC fp32
// The im2col use of the tile walk of f32_tile.h (tile_walk under TileKahanSum): row m = output pixel (img, oy, ox) of the whole batch
// (64-bit), k = tap * C_in + channel, the A quad of a row gathered from the image (zeros outside it and for rows beyond M), the epilogue
// BatchNorm's scale / shift and ReLU into a channel slice.  blockIdx.x = (M tile, N tile), the N tile fastest.
struct ConvGeom { int H, W, C_in, OH, OW, C_out, KW, stride, padH, padW, ldc, offset, K; long M; };

__global__ __launch_bounds__(THREADS) void incep_conv_kernel(const float* __restrict__ x, const float* __restrict__ wp, const float* __restrict__ scale,
                                                             const float* __restrict__ shift, float* __restrict__ out, const ConvGeom g) {
  using namespace dfh;
  const int ntn = (g.C_out + GT_N - 1) / GT_N;
  const long mt = blockIdx.x / ntn;
  const int n0 = (int)(blockIdx.x - mt * ntn) * GT_N;
  const long m0 = mt * GT_M;
  const long m = m0 + tile_stage_row();
  const bool row_ok = m < g.M;
  const long mm = row_ok ? m : g.M - 1;
  const long ohw = (long)g.OH * g.OW;
  const long img = mm / ohw;
  const int rem = (int)(mm - img * ohw);
  const int oy = rem / g.OW, ox = rem - oy * g.OW;
  const int iy0 = oy * g.stride - g.padH, ix0 = ox * g.stride - g.padW;
  const float* xin = x + img * (long)g.H * g.W * g.C_in;
  float* slice = out + g.offset;
  const long ldc = g.ldc;
  tile_walk<TileKahanSum>(
      m0, n0, g.M, g.C_out, g.K, wp + (long)min(n0 + tile_stage_row(), g.C_out - 1) * g.K,
      [&](int k) {
        const int tap = k / g.C_in, c = k - tap * g.C_in;
        const int ky = tap / g.KW, kx = tap - ky * g.KW;
        const int iy = iy0 + ky, ix = ix0 + kx;
        if (row_ok && iy >= 0 && iy < g.H && ix >= 0 && ix < g.W) return *(const float4*)(xin + ((long)iy * g.W + ix) * g.C_in + c);
        return make_float4(0.f, 0.f, 0.f, 0.f);
      },
      [&](int n) { return make_float2(scale[n], shift[n]); },
      [&](long row, int n, float sum, float2 ss) {
        const float v = sum * ss.x + ss.y;
        slice[row * ldc + n] = v <= 0.0f ? 0.0f : v;      // torch's relu: a NaN stays a NaN
      });
}

// ------------------------------------------------------------------ the 3 x 3 pools, NHWC, float4 along channels, into a channel slice
__global__ __launch_bounds__(THREADS) void incep_pool_kernel(const float4* __restrict__ x, float* __restrict__ out, int mode, int H, int W, int C4,
                                                             int OH, int OW, int ldc, int offset, long total) {
  const long t = (long)blockIdx.x * THREADS + threadIdx.x;
  if (t >= total) return;
  const int c = (int)(t % C4);
  long r = t / C4;
  const int ox = (int)(r % OW);
  r /= OW;
  const int oy = (int)(r % OH);
  const long n = r / OH;
  const bool is_max = mode == DFH_INCEP_POOL_MAX_S2 || mode == DFH_INCEP_POOL_MAX_S1;
  const int stride = mode == DFH_INCEP_POOL_MAX_S2 ? 2 : 1, pad = mode == DFH_INCEP_POOL_MAX_S2 ? 0 : 1;
  float4 a = is_max ? make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY) : make_float4(0.f, 0.f, 0.f, 0.f);
  int inside = 0;
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const int iy = oy * stride - pad + dy, ix = ox * stride - pad + dx;
      if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
      const float4 v = x[((n * H + iy) * W + ix) * C4 + c];
      ++inside;
      if (is_max) { using dfh::pool_max; a.x = pool_max(a.x, v.x); a.y = pool_max(a.y, v.y); a.z = pool_max(a.z, v.z); a.w = pool_max(a.w, v.w); }
      else { a.x += v.x; a.y += v.y; a.z += v.z; a.w += v.w; }
    }
  if (!is_max) {
    const float d = mode == DFH_INCEP_POOL_AVG_INCL ? 9.0f : (float)inside;
    a.x /= d; a.y /= d; a.z /= d; a.w /= d;
  }
  *(float4*)(out + ((n * OH + oy) * OW + ox) * ldc + offset + 4 * c) = a;
}

// ------------------------------------------------------------------ out [n][C] = mean over the HW rows of image n, fp64 sums in a fixed order
// grid (ceil(C / 64), n); thread -> (channel tid % 64, row group tid / 64): the group sums rows g, g + 4, ... in index order, the four
// groups are added as ((g0 + g1) + g2) + g3 and divided in fp64; Out = float (the global spatial mean of a block's pixels) rounds that
// once, Out = double with n = 1 is the column mean of the statistics.
template <class Out>
__global__ __launch_bounds__(THREADS) void incep_mean_kernel(const float* __restrict__ x, Out* __restrict__ out, int HW, int C) {
  __shared__ double part[4][64];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), grp = threadIdx.x >> 6;
  const long n = blockIdx.y;
  double s = 0.0;
  if (c < C)
    for (int p = grp; p < HW; p += 4) s += (double)x[(n * HW + p) * C + c];
  part[grp][threadIdx.x & 63] = s;
  __syncthreads();
  if (grp == 0 && c < C) {
    const int l = threadIdx.x;
    out[n * C + c] = (Out)((((part[0][l] + part[1][l]) + part[2][l]) + part[3][l]) / (double)HW);
  }
}

// ------------------------------------------------------------------ the head: fc (compensated k-tiles), softmax, the score terms
__global__ __launch_bounds__(THREADS) void incep_fc_kernel(const float* __restrict__ feat, const float* __restrict__ w, const float* __restrict__ bias,
                                                           float* __restrict__ logits, int M, int N, int K) {
  dfh::gemm_tile<dfh::TileKahanSum>(feat, K, w, K, bias, M, N, K, [&](int m, int n, float v) { logits[(long)m * N + n] = v; });
}

// one wave a row (four rows a workgroup): torch's softmax, exp(x - max) / sum, every sum a per-lane chain in index order then one wave tree
__global__ __launch_bounds__(THREADS) void incep_softmax_kernel(const float* __restrict__ logits, float* __restrict__ probs, int rows, int N) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;                 // whole waves leave
  const float* x = logits + (long)row * N;
  float mx = -INFINITY;
  for (int c = lane; c < N; c += 64) mx = fmaxf(mx, x[c]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  float s = 0.0f;
  for (int c = lane; c < N; c += 64) s += expf(x[c] - mx);
  s = wave_sum(s);
  for (int c = lane; c < N; c += 64) probs[(long)row * N + c] = expf(x[c] - mx) / s;
}

__global__ __launch_bounds__(THREADS) void incep_is_rows_kernel(const float* __restrict__ probs, const int64_t* __restrict__ cate, int rows, int N,
                                                                float eps, int64_t* __restrict__ label, float* __restrict__ ent,
                                                                float* __restrict__ kl, float* __restrict__ correct) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;                 // whole waves leave
  const float* p = probs + (long)row * N;
  const float log_uniform = logf(1.0f / (float)N);
  float e = 0.0f, k = 0.0f, best = -INFINITY;
  int bi = 0x7fffffff;
  bool nan = false;
  for (int c = lane; c < N; c += 64) {
    const float v = p[c], lg = logf(v + eps);
    e += -v * lg;
    k += v * (lg - log_uniform);
    // torch.argmax: a NaN is the maximum, the lowest index wins among equals
    const bool vnan = v != v;
    if (!nan && (vnan || v > best || bi == 0x7fffffff)) { best = v; bi = c; nan = vnan; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float ob = __shfl_xor(best, o, 64);
    const int oi = __shfl_xor(bi, o, 64);
    const bool on = ob != ob;
    const bool take = nan ? (on && oi < bi) : (on || ob > best || (ob == best && oi < bi));
    if (take) { best = ob; bi = oi; nan = on; }
  }
  e = wave_sum(e);
  k = wave_sum(k);
  if (lane == 0) {
    label[row] = bi;
    ent[row] = e;
    kl[row] = k;
    correct[row] = cate && cate[row] == (int64_t)bi ? 1.0f : 0.0f;
  }
}

// One workgroup a split: images [s n / splits, (s + 1) n / splits); thread t sums images t, t + 256, ... in index order (compensated),
// the 256 partial sums meet in a fixed tree.  out[s] = (mean ent, exp(mean kl), sum correct)
__global__ __launch_bounds__(THREADS) void incep_is_splits_kernel(const float* __restrict__ ent, const float* __restrict__ kl,
                                                                  const float* __restrict__ correct, int n, int splits, float* __restrict__ out) {
  __shared__ float red[3][THREADS];
  const int s = blockIdx.x, tid = threadIdx.x;
  const long lo = (long)s * n / splits, hi = (long)(s + 1) * n / splits;
  float a[3] = {0.f, 0.f, 0.f}, comp[3] = {0.f, 0.f, 0.f};
  for (long i = lo + tid; i < hi; i += THREADS) {
    dfh::kahan_add(a[0], comp[0], ent[i]);
    dfh::kahan_add(a[1], comp[1], kl[i]);
    dfh::kahan_add(a[2], comp[2], correct[i]);
  }
#pragma unroll
  for (int q = 0; q < 3; ++q) red[q][tid] = a[q];
  __syncthreads();
  for (int w = THREADS / 2; w > 0; w >>= 1) {
    if (tid < w)
#pragma unroll
      for (int q = 0; q < 3; ++q) red[q][tid] += red[q][tid + w];
    __syncthreads();
  }
  if (tid == 0) {
    const float cnt = (float)(hi - lo);
    out[3 * s + 0] = red[0][0] / cnt;
    out[3 * s + 1] = expf(red[1][0] / cnt);
    out[3 * s + 2] = red[2][0];
  }
}

// ------------------------------------------------------------------ statistics in fp64: column means (incep_mean_kernel<double>, one
// "image" of N rows), then the covariance on the fp64 MFMA
// sigma[i][j] = sum_r (act[r][i] - mu[i]) (act[r][j] - mu[j]) / (N - 1): 64 x 64 tile a workgroup (grid: (column tile, row tile), only
// tiles with column tile >= row tile work), four waves of 32 x 32 = 2 x 2 blocks of v_mfma_f64_16x16x4_f64, rows in steps of 16 through
// k-major LDS images of the centred values.  Elements on and above the diagonal are written together with their mirror image.
constexpr int CV_K = 16, CV_LD = 72;
__global__ __launch_bounds__(THREADS) void incep_cov_kernel(const float* __restrict__ act, const double* __restrict__ mu, double* __restrict__ sigma,
                                                            int N, int D) {
  if (blockIdx.x < blockIdx.y) return;
  __shared__ double Xi[CV_K * CV_LD];
  __shared__ double Xj[CV_K * CV_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int i0 = blockIdx.y * 64, j0 = blockIdx.x * 64;
  const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
  const int scol = tid & 63, srow = tid >> 6;
  const int ci = min(i0 + scol, D - 1), cj = min(j0 + scol, D - 1);
  const double mi = mu[ci], mj = mu[cj];
  const int fr = lane & 15, fk = lane >> 4;
  f64x4_t acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = f64x4_t{0.0, 0.0, 0.0, 0.0};
  for (int r0 = 0; r0 < N; r0 += CV_K) {
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int kr = srow + 4 * q, r = r0 + kr;
      Xi[kr * CV_LD + scol] = r < N ? (double)act[(long)r * D + ci] - mi : 0.0;
      Xj[kr * CV_LD + scol] = r < N ? (double)act[(long)r * D + cj] - mj : 0.0;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < CV_K; kk += 4) {
      double av[2], bv[2];
#pragma unroll
      for (int a = 0; a < 2; ++a) av[a] = Xi[(kk + fk) * CV_LD + wm + 16 * a + fr];
#pragma unroll
      for (int b = 0; b < 2; ++b) bv[b] = Xj[(kk + fk) * CV_LD + wn + 16 * b + fr];
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[a], bv[b], acc[a][b], 0, 0, 0);
    }
  }
  // C layout of the f64 16x16x4: acc[r] = C[lane / 16 + 4 r][lane % 16]
  const double div = (double)(N - 1);
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int i = i0 + wm + 16 * a + fk + 4 * r, j = j0 + wn + 16 * b + fr;
        if (i < D && j < D && j >= i) {
          const double v = acc[a][b][r] / div;
          sigma[(long)i * D + j] = v;
          sigma[(long)j * D + i] = v;
        }
      }
}

// ------------------------------------------------------------------ host: the layer list
struct ConvDesc { std::string name; int cin, cin_pad, cout, kh, kw, stride, ph, pw, wi; size_t packed_off; };      // wi: table index of conv.weight

using dfh::aligned16;
size_t conv_packed_floats(int cin_pad, int cout, int kh, int kw) { return (size_t)cout * ((size_t)kh * kw * cin_pad + 2); }

// ------------------------------------------------------------------ host: launchers
int launch_prep(const float* src, int n, int H, int W, int resize, int normalize, int affine, float* out, hipStream_t s) {
  const int OH = resize ? SIDE : H, OW = resize ? SIDE : W;
  const long total = (long)n * OH * OW;
  Affine af;
  // torchvision's _transform_input: x * (0.229 / 0.5) + (0.485 - 0.5) / 0.5, the Python doubles rounded to fp32 as torch rounds a scalar operand
  const double sd[3] = {0.229, 0.224, 0.225}, mean[3] = {0.485, 0.456, 0.406};
  for (int c = 0; c < 3; ++c) { af.a[c] = (float)(sd[c] / 0.5); af.b[c] = (float)((mean[c] - 0.5) / 0.5); }
  hipLaunchKernelGGL(incep_prep_kernel, dim3((unsigned)((total + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, src, (float4*)out, H, W, OH, OW, resize,
                     normalize, affine, af, total);
  return dfh::check_launch("incep_prep_kernel");
}

int launch_pack(const float* w, const float* const* bn, float* packed, int w_cin, int cin, int taps, int cout, hipStream_t s) {
  const long total = (long)taps * cin * cout;
  hipLaunchKernelGGL(incep_pack_conv_kernel, dim3((unsigned)((total + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, w, bn[0], bn[1], bn[2], bn[3], packed,
                     w_cin, cin, taps, cout);
  return dfh::check_launch("incep_pack_conv_kernel");
}

int launch_conv(const float* x, const float* packed, float* out, int n, const dfh_incep_launch& L, hipStream_t s) {
  ConvGeom g;
  g.H = L.Hin; g.W = L.Win; g.C_in = L.Cin; g.OH = L.Hout; g.OW = L.Wout; g.C_out = L.Cout; g.KW = L.KW; g.stride = L.stride;
  g.padH = L.padH; g.padW = L.padW; g.ldc = L.ldc; g.offset = L.offset; g.K = L.KH * L.KW * L.Cin; g.M = (long)n * L.Hout * L.Wout;
  const long tiles = (g.M + dfh::GT_M - 1) / dfh::GT_M * ((g.C_out + dfh::GT_N - 1) / dfh::GT_N);
  if (tiles > 0x7fffffffL) { dfh::set_error("incep_conv_kernel: more than 2^31 tiles"); return -1; }
  const float* scale = packed + (size_t)g.C_out * g.K;
  dfh::ProfScope ps(dfh::PC_CONV3, 2.0 * g.M * g.K * g.C_out, 4.0 * ((double)n * g.H * g.W * g.C_in + (double)g.M * g.C_out + (double)g.K * g.C_out), s);
  hipLaunchKernelGGL(incep_conv_kernel, dim3((unsigned)tiles), dim3(THREADS), 0, s, x, packed, scale, scale + g.C_out, out, g);
  return dfh::check_launch("incep_conv_kernel");
}

int launch_pool(const float* x, float* out, int mode, int n, int H, int W, int C, int OH, int OW, int ldc, int offset, hipStream_t s) {
  const long total = (long)n * OH * OW * (C / 4);
  hipLaunchKernelGGL(incep_pool_kernel, dim3((unsigned)((total + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, (const float4*)x, out, mode, H, W, C / 4,
                     OH, OW, ldc, offset, total);
  return dfh::check_launch("incep_pool_kernel");
}

template <class Out>
int launch_mean(const float* x, Out* out, int n, int HW, int C, hipStream_t s) {
  hipLaunchKernelGGL(incep_mean_kernel<Out>, dim3((unsigned)((C + 63) / 64), (unsigned)n), dim3(THREADS), 0, s, x, out, HW, C);
  return dfh::check_launch("incep_mean_kernel");
}

int launch_fc(const float* feat, const float* w, const float* bias, float* logits, int n, int K, int classes, hipStream_t s) {
  hipLaunchKernelGGL(incep_fc_kernel, dim3((unsigned)((classes + dfh::GT_N - 1) / dfh::GT_N), (unsigned)((n + dfh::GT_M - 1) / dfh::GT_M)), dim3(THREADS), 0,
                     s, feat, w, bias, logits, n, classes, K);
  return dfh::check_launch("incep_fc_kernel");
}

int launch_softmax(const float* logits, float* probs, int n, int classes, hipStream_t s) {
  hipLaunchKernelGGL(incep_softmax_kernel, dim3((unsigned)((n + 3) / 4)), dim3(THREADS), 0, s, logits, probs, n, classes);
  return dfh::check_launch("incep_softmax_kernel");
}

int pool_out(int mode, int v) { return mode == DFH_INCEP_POOL_MAX_S2 ? (v - 3) / 2 + 1 : v; }

}  // namespace

struct dfh_incep {
  dfh_incep_config cfg;
  dfh::ParamList t;
  std::vector<ConvDesc> conv;
  int fc_w = -1, fc_b = -1, last_block = 0;
  size_t packed_floats = 0;

  int add_conv(const std::string& name, int cin, int cout, int kh, int kw, int stride, int ph, int pw) {
    ConvDesc c;
    c.name = name; c.cin = cin; c.cin_pad = (cin + 3) & ~3; c.cout = cout; c.kh = kh; c.kw = kw; c.stride = stride; c.ph = ph; c.pw = pw;
    c.wi = t.add_param(name + ".conv.weight", {cout, cin, kh, kw});
    for (const char* leaf : {".bn.weight", ".bn.bias", ".bn.running_mean", ".bn.running_var"}) t.add_param(name + leaf, {cout});
    c.packed_off = packed_floats;
    packed_floats += conv_packed_floats(c.cin_pad, cout, kh, kw);
    conv.push_back(c);
    return (int)conv.size() - 1;
  }

  explicit dfh_incep(const dfh_incep_config& c) : cfg(c) {
    for (int b = 0; b < NBLOCK; ++b)
      if (cfg.block_mask >> b & 1) last_block = b;
    // torchvision's module order, which is its state dict's
    add_conv("Conv2d_1a_3x3", 3, 32, 3, 3, 2, 0, 0);
    add_conv("Conv2d_2a_3x3", 32, 32, 3, 3, 1, 0, 0);
    add_conv("Conv2d_2b_3x3", 32, 64, 3, 3, 1, 1, 1);
    add_conv("Conv2d_3b_1x1", 64, 80, 1, 1, 1, 0, 0);
    add_conv("Conv2d_4a_3x3", 80, 192, 3, 3, 1, 0, 0);
    const int pool_features[3] = {32, 64, 64};
    const char* a_names[3] = {"Mixed_5b", "Mixed_5c", "Mixed_5d"};
    int cin = 192;
    for (int i = 0; i < 3; ++i) {
      const std::string p = std::string(a_names[i]) + ".";
      add_conv(p + "branch1x1", cin, 64, 1, 1, 1, 0, 0);
      add_conv(p + "branch5x5_1", cin, 48, 1, 1, 1, 0, 0);
      add_conv(p + "branch5x5_2", 48, 64, 5, 5, 1, 2, 2);
      add_conv(p + "branch3x3dbl_1", cin, 64, 1, 1, 1, 0, 0);
      add_conv(p + "branch3x3dbl_2", 64, 96, 3, 3, 1, 1, 1);
      add_conv(p + "branch3x3dbl_3", 96, 96, 3, 3, 1, 1, 1);
      add_conv(p + "branch_pool", cin, pool_features[i], 1, 1, 1, 0, 0);
      cin = 224 + pool_features[i];
    }
    add_conv("Mixed_6a.branch3x3", 288, 384, 3, 3, 2, 0, 0);
    add_conv("Mixed_6a.branch3x3dbl_1", 288, 64, 1, 1, 1, 0, 0);
    add_conv("Mixed_6a.branch3x3dbl_2", 64, 96, 3, 3, 1, 1, 1);
    add_conv("Mixed_6a.branch3x3dbl_3", 96, 96, 3, 3, 2, 0, 0);
    const int c7s[4] = {128, 160, 160, 192};
    const char* c_names[4] = {"Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"};
    for (int i = 0; i < 4; ++i) {
      const std::string p = std::string(c_names[i]) + ".";
      const int c7 = c7s[i];
      add_conv(p + "branch1x1", 768, 192, 1, 1, 1, 0, 0);
      add_conv(p + "branch7x7_1", 768, c7, 1, 1, 1, 0, 0);
      add_conv(p + "branch7x7_2", c7, c7, 1, 7, 1, 0, 3);
      add_conv(p + "branch7x7_3", c7, 192, 7, 1, 1, 3, 0);
      add_conv(p + "branch7x7dbl_1", 768, c7, 1, 1, 1, 0, 0);
      add_conv(p + "branch7x7dbl_2", c7, c7, 7, 1, 1, 3, 0);
      add_conv(p + "branch7x7dbl_3", c7, c7, 1, 7, 1, 0, 3);
      add_conv(p + "branch7x7dbl_4", c7, c7, 7, 1, 1, 3, 0);
      add_conv(p + "branch7x7dbl_5", c7, 192, 1, 7, 1, 0, 3);
      add_conv(p + "branch_pool", 768, 192, 1, 1, 1, 0, 0);
    }
    add_conv("Mixed_7a.branch3x3_1", 768, 192, 1, 1, 1, 0, 0);
    add_conv("Mixed_7a.branch3x3_2", 192, 320, 3, 3, 2, 0, 0);
    add_conv("Mixed_7a.branch7x7x3_1", 768, 192, 1, 1, 1, 0, 0);
    add_conv("Mixed_7a.branch7x7x3_2", 192, 192, 1, 7, 1, 0, 3);
    add_conv("Mixed_7a.branch7x7x3_3", 192, 192, 7, 1, 1, 3, 0);
    add_conv("Mixed_7a.branch7x7x3_4", 192, 192, 3, 3, 2, 0, 0);
    const char* e_names[2] = {"Mixed_7b", "Mixed_7c"};
    cin = 1280;
    for (int i = 0; i < 2; ++i) {
      const std::string p = std::string(e_names[i]) + ".";
      add_conv(p + "branch1x1", cin, 320, 1, 1, 1, 0, 0);
      add_conv(p + "branch3x3_1", cin, 384, 1, 1, 1, 0, 0);
      add_conv(p + "branch3x3_2a", 384, 384, 1, 3, 1, 0, 1);
      add_conv(p + "branch3x3_2b", 384, 384, 3, 1, 1, 1, 0);
      add_conv(p + "branch3x3dbl_1", cin, 448, 1, 1, 1, 0, 0);
      add_conv(p + "branch3x3dbl_2", 448, 384, 3, 3, 1, 1, 1);
      add_conv(p + "branch3x3dbl_3a", 384, 384, 1, 3, 1, 0, 1);
      add_conv(p + "branch3x3dbl_3b", 384, 384, 3, 1, 1, 1, 0);
      add_conv(p + "branch_pool", cin, 192, 1, 1, 1, 0, 0);
      cin = 2048;
    }
    if (cfg.variant == DFH_INCEP_VARIANT_TV) {
      fc_w = t.add_param("fc.weight", {cfg.num_classes, 2048});
      fc_b = t.add_param("fc.bias", {cfg.num_classes});
    }
  }

  int require_params(const float* const* params, int count, const char* who) const {
    return dfh::require_params(t, params, count, who, "dfh_incep_num_params (" + std::to_string(t.num_params()) + ")");
  }
};

namespace {

// ------------------------------------------------------------------ host: the plan (pure arithmetic)
struct Tensor { int region, H, W, C; };
struct Plan {
  std::vector<dfh_incep_launch> launches;
  size_t region_floats[5] = {0, 0, 0, 0, 0};      // per call (n images), rounded to 64 floats; 4: the logits
  size_t region_off[5] = {0, 0, 0, 0, 0};
  size_t total_floats = 0;
  std::string error;
};

struct Planner {
  const dfh_incep& m;
  int n;
  Plan& p;
  int ci = 0;                                      // the next convolution of the layer list
  Planner(const dfh_incep& model, int images, Plan& plan) : m(model), n(images), p(plan) {}

  size_t floats(const Tensor& t) const { return (size_t)n * t.H * t.W * t.C; }
  Tensor place(int region, int H, int W, int C) {
    const Tensor t{region, H, W, C};
    p.region_floats[region] = std::max(p.region_floats[region], (floats(t) + 63) / 64 * 64);
    return t;
  }
  dfh_incep_launch& add(int kind, const char* name) {
    dfh_incep_launch L;
    std::memset(&L, 0, sizeof L);
    L.kind = kind; L.conv = -1; L.block = -1; L.pool_mode = -1;
    std::strncpy(L.name, name, sizeof L.name - 1);
    p.launches.push_back(L);
    return p.launches.back();
  }
  void io(dfh_incep_launch& L, const Tensor* src, const Tensor* dst) {
    if (src) { L.src_region = src->region; L.src_floats = floats(*src); L.Hin = src->H; L.Win = src->W; L.Cin = src->C; }
    if (dst) { L.dst_region = dst->region; L.dst_floats = floats(*dst); L.ldc = dst->C; }
  }
  // the next convolution of the list, from x into channels [offset, offset + C_out) of y (y.region < 0: a new dense tensor in `region`)
  Tensor conv(const Tensor& x, Tensor y, int offset, int region = -1) {
    const ConvDesc& d = m.conv[ci];
    const int OH = (x.H + 2 * d.ph - d.kh) / d.stride + 1, OW = (x.W + 2 * d.pw - d.kw) / d.stride + 1;
    if (y.region < 0) y = place(region, OH, OW, d.cout);
    if (x.C != d.cin_pad || y.H != OH || y.W != OW || offset + d.cout > y.C || x.region == y.region) p.error = "plan: geometry mismatch at " + d.name;
    dfh_incep_launch& L = add(DFH_INCEP_K_CONV, d.name.c_str());
    io(L, &x, &y);
    L.conv = ci++; L.KH = d.kh; L.KW = d.kw; L.stride = d.stride; L.padH = d.ph; L.padW = d.pw;
    L.Hout = OH; L.Wout = OW; L.Cout = d.cout; L.offset = offset;
    return y;
  }
  Tensor pool(const Tensor& x, int mode, Tensor y, int offset, const char* name, int region = -1) {
    const int OH = pool_out(mode, x.H), OW = pool_out(mode, x.W);
    if (y.region < 0) y = place(region, OH, OW, x.C);
    if (y.H != OH || y.W != OW || offset + x.C > y.C || x.region == y.region) p.error = std::string("plan: geometry mismatch at ") + name;
    dfh_incep_launch& L = add(DFH_INCEP_K_POOL, name);
    io(L, &x, &y);
    L.pool_mode = mode; L.KH = L.KW = 3; L.stride = mode == DFH_INCEP_POOL_MAX_S2 ? 2 : 1; L.padH = L.padW = mode == DFH_INCEP_POOL_MAX_S2 ? 0 : 1;
    L.Hout = OH; L.Wout = OW; L.Cout = x.C; L.offset = offset;
    return y;
  }
  void tap(const Tensor& x, int block) {
    if (!(m.cfg.block_mask >> block & 1)) return;
    dfh_incep_launch& L = add(DFH_INCEP_K_GMEAN, "tap");
    io(L, &x, nullptr);
    L.block = block; L.dst_region = DFH_INCEP_REGION_TAP; L.dst_floats = (size_t)n * x.C;
    L.Hout = L.Wout = 1; L.Cout = L.ldc = x.C;
  }
};

const Tensor NEW{-1, 0, 0, 0};

void build_plan(const dfh_incep& m, int n, int H, int W, Plan& p) {
  Planner b(m, n, p);
  const bool fid = m.cfg.variant == DFH_INCEP_VARIANT_FID;
  const int avg = fid ? DFH_INCEP_POOL_AVG_EXCL : DFH_INCEP_POOL_AVG_INCL;
  const int OH = m.cfg.resize_input ? SIDE : H, OW = m.cfg.resize_input ? SIDE : W;
  Tensor x = b.place(0, OH, OW, 4);
  {
    dfh_incep_launch& L = b.add(DFH_INCEP_K_PREP, "prep");
    b.io(L, nullptr, &x);
    L.src_region = DFH_INCEP_REGION_INPUT; L.src_floats = (size_t)n * 3 * H * W;
    L.Hin = H; L.Win = W; L.Cin = 3; L.Hout = OH; L.Wout = OW; L.Cout = 4;
  }
  // block 0
  x = b.conv(x, NEW, 0, 1);
  x = b.conv(x, NEW, 0, 0);
  x = b.conv(x, NEW, 0, 1);
  x = b.pool(x, DFH_INCEP_POOL_MAX_S2, NEW, 0, "maxpool1", 0);
  b.tap(x, 0);
  if (m.last_block >= 1) {
    x = b.conv(x, NEW, 0, 1);
    x = b.conv(x, NEW, 0, 0);
    x = b.pool(x, DFH_INCEP_POOL_MAX_S2, NEW, 0, "maxpool2", 1);
    b.tap(x, 1);
  }
  // the mixed blocks: x in one of regions 0 / 1, the concatenation y in the other, branch temporaries in regions 2 and 3
  auto other = [&](const Tensor& t) { return t.region == 0 ? 1 : 0; };
  if (m.last_block >= 2) {
    for (int i = 0; i < 3; ++i) {                                                  // InceptionA
      const int pf = m.conv[b.ci + 6].cout;
      Tensor y = b.place(other(x), x.H, x.W, 224 + pf);
      b.conv(x, y, 0);
      Tensor t = b.conv(x, NEW, 0, 2);
      b.conv(t, y, 64);
      t = b.conv(x, NEW, 0, 2);
      t = b.conv(t, NEW, 0, 3);
      b.conv(t, y, 128);
      t = b.pool(x, avg, NEW, 0, "branch_pool.avg", 2);
      b.conv(t, y, 224);
      x = y;
    }
    {                                                                              // InceptionB
      Tensor y = b.place(other(x), (x.H - 3) / 2 + 1, (x.W - 3) / 2 + 1, 768);
      b.conv(x, y, 0);
      Tensor t = b.conv(x, NEW, 0, 2);
      t = b.conv(t, NEW, 0, 3);
      b.conv(t, y, 384);
      b.pool(x, DFH_INCEP_POOL_MAX_S2, y, 480, "Mixed_6a.max");
      x = y;
    }
    for (int i = 0; i < 4; ++i) {                                                  // InceptionC
      Tensor y = b.place(other(x), x.H, x.W, 768);
      b.conv(x, y, 0);
      Tensor t = b.conv(x, NEW, 0, 2);
      t = b.conv(t, NEW, 0, 3);
      b.conv(t, y, 192);
      t = b.conv(x, NEW, 0, 2);
      t = b.conv(t, NEW, 0, 3);
      t = b.conv(t, NEW, 0, 2);
      t = b.conv(t, NEW, 0, 3);
      b.conv(t, y, 384);
      t = b.pool(x, avg, NEW, 0, "branch_pool.avg", 2);
      b.conv(t, y, 576);
      x = y;
    }
    b.tap(x, 2);
  }
  if (m.last_block >= 3) {
    {                                                                              // InceptionD
      Tensor y = b.place(other(x), (x.H - 3) / 2 + 1, (x.W - 3) / 2 + 1, 1280);
      Tensor t = b.conv(x, NEW, 0, 2);
      b.conv(t, y, 0);
      t = b.conv(x, NEW, 0, 2);
      t = b.conv(t, NEW, 0, 3);
      t = b.conv(t, NEW, 0, 2);
      b.conv(t, y, 320);
      b.pool(x, DFH_INCEP_POOL_MAX_S2, y, 512, "Mixed_7a.max");
      x = y;
    }
    for (int i = 0; i < 2; ++i) {                                                  // InceptionE
      Tensor y = b.place(other(x), x.H, x.W, 2048);
      b.conv(x, y, 0);
      Tensor t = b.conv(x, NEW, 0, 2);
      b.conv(t, y, 320);
      b.conv(t, y, 704);
      t = b.conv(x, NEW, 0, 2);
      t = b.conv(t, NEW, 0, 3);
      b.conv(t, y, 1088);
      b.conv(t, y, 1472);
      t = b.pool(x, fid && i == 1 ? DFH_INCEP_POOL_MAX_S1 : avg, NEW, 0, fid && i == 1 ? "branch_pool.max" : "branch_pool.avg", 2);
      b.conv(t, y, 1856);
      x = y;
    }
    b.tap(x, 3);
    if (!fid) {
      const int classes = m.cfg.num_classes;
      p.region_floats[4] = ((size_t)n * classes + 63) / 64 * 64;
      dfh_incep_launch& F = b.add(DFH_INCEP_K_FC, "fc");
      F.src_region = DFH_INCEP_REGION_TAP; F.block = 3; F.src_floats = (size_t)n * 2048; F.Hin = F.Win = F.Hout = F.Wout = 1; F.Cin = 2048;
      F.Cout = F.ldc = classes; F.dst_region = 4; F.dst_floats = (size_t)n * classes;
      dfh_incep_launch& S = b.add(DFH_INCEP_K_SOFTMAX, "softmax");
      S.src_region = 4; S.src_floats = (size_t)n * classes; S.Hin = S.Win = S.Hout = S.Wout = 1; S.Cin = S.Cout = S.ldc = classes;
      S.dst_region = DFH_INCEP_REGION_PROBS; S.dst_floats = (size_t)n * classes;
    }
  }
  size_t off = 0;
  for (int r = 0; r < 5; ++r) { p.region_off[r] = off; off += p.region_floats[r]; }
  p.total_floats = off;
  for (dfh_incep_launch& L : p.launches) {
    if (L.src_region >= 0) L.src_off = p.region_off[L.src_region];
    if (L.dst_region >= 0) L.dst_off = p.region_off[L.dst_region];
  }
}

// what a call's (n, H, W) must satisfy; on a refusal the message is set and -1 returned
int require_shape(const dfh_incep* c, int n, int H, int W, const char* who) {
  auto refuse = [&](const std::string& msg) { dfh::set_error(std::string(who) + ": " + msg); return -1; };
  if (!c) return refuse("null argument: ctx");
  if (n < 1 || n > 65535) return refuse("n must be in [1, 65535] a call");
  if (H < 1 || W < 1 || H > MAX_SIDE || W > MAX_SIDE) return refuse("H and W must be in [1, 8192]");
  if (!c->cfg.resize_input && (H < 75 || W < 75)) return refuse("without resize_input H and W must be at least 75: Mixed_7a would be empty below that");
  return 0;
}

}  // namespace

extern "C" {

int dfh_incep_create(const dfh_incep_config* cfg, dfh_incep** out) {
  DFH_REQUIRE(cfg && out, "null argument");
  DFH_REQUIRE(cfg->variant == DFH_INCEP_VARIANT_TV || cfg->variant == DFH_INCEP_VARIANT_FID,
              "unsupported variant " + std::to_string(cfg->variant) + ": 0 (torchvision's inception_v3) or 1 (pytorch_fid's fid_inception_v3)");
  DFH_REQUIRE(cfg->block_mask >= 1 && cfg->block_mask < (1 << NBLOCK), "block_mask must name at least one of the blocks 0 .. 3");
  if (cfg->variant == DFH_INCEP_VARIANT_TV) {
    DFH_REQUIRE(cfg->num_classes >= 1 && cfg->num_classes <= MAX_CLASSES, "num_classes must be in [1, 4096]");
    DFH_REQUIRE(cfg->block_mask & 8, "the classifier variant runs the whole network: block_mask must include block 3");
  }
  dfh_incep* p = new (std::nothrow) dfh_incep(*cfg);
  DFH_REQUIRE(p != nullptr, "out of host memory");
  *out = p;
  return 0;
}

void dfh_incep_destroy(dfh_incep* c) { delete c; }
int dfh_incep_num_params(const dfh_incep* c) { return c ? c->t.num_params() : 0; }
const char* dfh_incep_param_name(const dfh_incep* c, int i) { return c ? c->t.param_name(i) : ""; }
int dfh_incep_param_ndim(const dfh_incep* c, int i) { return c ? c->t.param_ndim(i) : 0; }
int dfh_incep_param_dim(const dfh_incep* c, int i, int d) { return c ? c->t.param_dim(i, d) : 0; }
size_t dfh_incep_packed_bytes(const dfh_incep* c) { return c ? c->packed_floats * sizeof(float) : 0; }

int dfh_incep_pack(dfh_incep* c, const float* const* params, int count, void* packed, void* stream) {
  DFH_REQUIRE(c, "null argument: ctx");
  if (int rc = c->require_params(params, count, "dfh_incep_pack")) return rc;
  DFH_REQUIRE(packed, "null argument: packed");
  DFH_REQUIRE(aligned16(packed), "packed must be 16-byte aligned");
  for (const ConvDesc& d : c->conv)
    if (int rc = launch_pack(params[d.wi], params + d.wi + 1, (float*)packed + d.packed_off, d.cin, d.cin_pad, d.kh * d.kw, d.cout, (hipStream_t)stream))
      return rc;
  return 0;
}

int dfh_incep_plan_count(const dfh_incep* c, int n, int H, int W) {
  if (int rc = require_shape(c, n, H, W, "dfh_incep_plan_count")) return rc;
  Plan p;
  build_plan(*c, n, H, W, p);
  if (!p.error.empty()) { dfh::set_error(p.error); return -1; }
  return (int)p.launches.size();
}

int dfh_incep_plan_entry(const dfh_incep* c, int n, int H, int W, int i, dfh_incep_launch* out) {
  if (int rc = require_shape(c, n, H, W, "dfh_incep_plan_entry")) return rc;
  DFH_REQUIRE(out, "null argument: out");
  Plan p;
  build_plan(*c, n, H, W, p);
  DFH_REQUIRE(p.error.empty(), p.error);
  DFH_REQUIRE(i >= 0 && i < (int)p.launches.size(), "launch index out of range");
  *out = p.launches[i];
  return 0;
}

size_t dfh_incep_workspace_bytes(const dfh_incep* c, int n, int H, int W) {
  if (require_shape(c, n, H, W, "dfh_incep_workspace_bytes")) return 0;
  Plan p;
  build_plan(*c, n, H, W, p);
  if (!p.error.empty()) { dfh::set_error(p.error); return 0; }
  return p.total_floats * sizeof(float) + 256;
}

int dfh_incep_forward(dfh_incep* c, const float* const* params, int count, const void* packed, const float* in, int n, int H, int W,
                      float* const* taps, float* probs, void* workspace, size_t workspace_bytes, void* stream) {
  DFH_REQUIRE(c, "null argument: ctx");
  if (int rc = c->require_params(params, count, "dfh_incep_forward")) return rc;
  DFH_REQUIRE(packed, "null argument: packed");
  DFH_REQUIRE(in, "null argument: in");
  DFH_REQUIRE(taps, "null argument: taps");
  DFH_REQUIRE(workspace, "null argument: workspace");
  const bool tv = c->cfg.variant == DFH_INCEP_VARIANT_TV;
  for (int b = 0; b < NBLOCK; ++b)
    if (c->cfg.block_mask >> b & 1) {
      DFH_REQUIRE(taps[b], "null argument: taps[" + std::to_string(b) + "] (block_mask names the block)");
      DFH_REQUIRE(aligned16(taps[b]), "taps[" + std::to_string(b) + "] must be 16-byte aligned");
    }
  DFH_REQUIRE(!tv || probs, "null argument: probs (the classifier variant writes the softmax)");
  DFH_REQUIRE(aligned16(packed), "packed must be 16-byte aligned");
  DFH_REQUIRE(aligned16(in), "in must be 16-byte aligned");
  DFH_REQUIRE(((uintptr_t)workspace & 255) == 0, "workspace must be 256-byte aligned");
  if (int rc = require_shape(c, n, H, W, "dfh_incep_forward")) return rc;
  Plan p;
  build_plan(*c, n, H, W, p);
  DFH_REQUIRE(p.error.empty(), p.error);
  DFH_REQUIRE(workspace_bytes >= p.total_floats * sizeof(float) + 256, "workspace smaller than dfh_incep_workspace_bytes");
  hipStream_t s = (hipStream_t)stream;
  float* ws = (float*)workspace;
  for (const dfh_incep_launch& L : p.launches) {
    const float* src = L.src_region >= 0 ? ws + L.src_off : L.src_region == DFH_INCEP_REGION_TAP ? taps[L.block] : in;
    float* dst = L.dst_region >= 0 ? ws + L.dst_off : L.dst_region == DFH_INCEP_REGION_TAP ? taps[L.block] : probs;
    int rc = 0;
    switch (L.kind) {
      case DFH_INCEP_K_PREP: rc = launch_prep(src, n, H, W, c->cfg.resize_input, c->cfg.normalize_input, tv, dst, s); break;
      case DFH_INCEP_K_CONV: rc = launch_conv(src, (const float*)packed + c->conv[L.conv].packed_off, dst, n, L, s); break;
      case DFH_INCEP_K_POOL: rc = launch_pool(src, dst, L.pool_mode, n, L.Hin, L.Win, L.Cin, L.Hout, L.Wout, L.ldc, L.offset, s); break;
      case DFH_INCEP_K_GMEAN: rc = launch_mean(src, dst, n, L.Hin * L.Win, L.Cin, s); break;
      case DFH_INCEP_K_FC: rc = launch_fc(src, params[c->fc_w], params[c->fc_b], dst, n, L.Cin, L.Cout, s); break;
      case DFH_INCEP_K_SOFTMAX: rc = launch_softmax(src, dst, n, L.Cout, s); break;
      default: DFH_REQUIRE(false, "unknown launch kind in the plan");
    }
    if (rc) return rc;
  }
  return 0;
}

// ---- op level
int dfh_incep_prep(const float* src, int n, int H, int W, int resize, int normalize, int affine, float* out, void* stream) {
  DFH_REQUIRE(src && out, "null argument");
  DFH_REQUIRE(aligned16(out), "out must be 16-byte aligned");
  DFH_REQUIRE(n >= 1 && H >= 1 && W >= 1 && H <= MAX_SIDE && W <= MAX_SIDE, "n / H / W must be positive, H and W at most 8192");
  return launch_prep(src, n, H, W, resize != 0, normalize != 0, affine != 0, out, (hipStream_t)stream);
}

int dfh_incep_conv_bn_relu(const float* x, const float* weight, int w_cin, const float* const* bn, float* packed, float* out, int n, int H, int W,
                           int C_in, int C_out, int KH, int KW, int stride, int padH, int padW, int ldc, int offset, void* stream) {
  DFH_REQUIRE(x && weight && bn && packed && out, "null argument");
  DFH_REQUIRE(bn[0] && bn[1] && bn[2] && bn[3], "null argument: bn weight / bias / running_mean / running_var");
  DFH_REQUIRE(C_in >= 4 && C_in % 4 == 0, "C_in must be a multiple of 4");
  DFH_REQUIRE(w_cin >= 1 && w_cin <= C_in, "w_cin must be in [1, C_in]");
  DFH_REQUIRE(C_out >= 1, "C_out must be positive");
  DFH_REQUIRE(KH >= 1 && KH <= 7 && KW >= 1 && KW <= 7 && (KH & 1) && (KW & 1), "KH and KW must be 1, 3, 5 or 7");
  DFH_REQUIRE(stride == 1 || stride == 2, "stride must be 1 or 2");
  DFH_REQUIRE(padH >= 0 && padH <= KH / 2 && padW >= 0 && padW <= KW / 2, "padH / padW must be in [0, K / 2]");
  DFH_REQUIRE(n >= 1 && n <= 65535 && H >= 1 && W >= 1 && H <= MAX_SIDE && W <= MAX_SIDE, "n must be in [1, 65535], H and W in [1, 8192]");
  DFH_REQUIRE(H + 2 * padH >= KH && W + 2 * padW >= KW, "the padded image is smaller than the filter");
  DFH_REQUIRE(offset >= 0 && ldc >= 1 && offset + C_out <= ldc, "the slice [offset, offset + C_out) must lie inside ldc");
  DFH_REQUIRE(aligned16(x) && aligned16(packed), "x / packed must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  if (int rc = launch_pack(weight, bn, packed, w_cin, C_in, KH * KW, C_out, s)) return rc;
  dfh_incep_launch L;
  std::memset(&L, 0, sizeof L);
  L.Hin = H; L.Win = W; L.Cin = C_in; L.KH = KH; L.KW = KW; L.stride = stride; L.padH = padH; L.padW = padW;
  L.Hout = (H + 2 * padH - KH) / stride + 1; L.Wout = (W + 2 * padW - KW) / stride + 1; L.Cout = C_out; L.ldc = ldc; L.offset = offset;
  return launch_conv(x, packed, out, n, L, s);
}

int dfh_incep_pool(const float* x, float* out, int mode, int n, int H, int W, int C, int ldc, int offset, void* stream) {
  DFH_REQUIRE(x && out, "null argument");
  DFH_REQUIRE(mode >= DFH_INCEP_POOL_MAX_S2 && mode <= DFH_INCEP_POOL_AVG_EXCL, "mode must be one of DFH_INCEP_POOL_*");
  DFH_REQUIRE(C >= 4 && C % 4 == 0 && ldc % 4 == 0 && offset % 4 == 0, "C, ldc and offset must be multiples of 4");
  DFH_REQUIRE(offset >= 0 && offset + C <= ldc, "the slice [offset, offset + C) must lie inside ldc");
  DFH_REQUIRE(n >= 1 && H >= 1 && W >= 1 && H <= MAX_SIDE && W <= MAX_SIDE, "n must be positive, H and W in [1, 8192]");
  DFH_REQUIRE(mode != DFH_INCEP_POOL_MAX_S2 || (H >= 3 && W >= 3), "the stride-2 pool needs H and W of at least 3");
  DFH_REQUIRE(aligned16(x) && aligned16(out), "x / out must be 16-byte aligned");
  return launch_pool(x, out, mode, n, H, W, C, pool_out(mode, H), pool_out(mode, W), ldc, offset, (hipStream_t)stream);
}

int dfh_incep_global_mean(const float* x, float* out, int n, int HW, int C, void* stream) {
  DFH_REQUIRE(x && out, "null argument");
  DFH_REQUIRE(n >= 1 && n <= 65535 && HW >= 1 && C >= 1, "n must be in [1, 65535], HW and C positive");
  return launch_mean(x, out, n, HW, C, (hipStream_t)stream);
}

int dfh_incep_fc_softmax(const float* feat, const float* weight, const float* bias, float* logits, float* probs, int n, int K, int classes,
                         void* stream) {
  DFH_REQUIRE(feat && weight && bias && logits && probs, "null argument");
  DFH_REQUIRE(n >= 1 && K >= 4 && K % 4 == 0 && classes >= 1 && classes <= MAX_CLASSES, "n positive, K a multiple of 4, classes in [1, 4096]");
  DFH_REQUIRE(aligned16(feat) && aligned16(weight), "feat / weight must be 16-byte aligned");
  if (int rc = launch_fc(feat, weight, bias, logits, n, K, classes, (hipStream_t)stream)) return rc;
  return launch_softmax(logits, probs, n, classes, (hipStream_t)stream);
}

int dfh_incep_is_rows(const float* probs, const int64_t* cate, int n, int classes, float eps, int64_t* label, float* ent, float* kl,
                      float* correct, void* stream) {
  DFH_REQUIRE(probs && label && ent && kl && correct, "null argument");
  DFH_REQUIRE(n >= 1 && classes >= 1, "n / classes must be positive");
  hipLaunchKernelGGL(incep_is_rows_kernel, dim3((unsigned)((n + 3) / 4)), dim3(THREADS), 0, (hipStream_t)stream, probs, cate, n, classes, eps, label, ent,
                     kl, correct);
  return dfh::check_launch("incep_is_rows_kernel");
}

int dfh_incep_is_splits(const float* ent, const float* kl, const float* correct, int n, int splits, float* out, void* stream) {
  DFH_REQUIRE(ent && kl && correct && out, "null argument");
  DFH_REQUIRE(n >= 1 && splits >= 1 && splits <= n, "splits must be in [1, n]");
  hipLaunchKernelGGL(incep_is_splits_kernel, dim3((unsigned)splits), dim3(THREADS), 0, (hipStream_t)stream, ent, kl, correct, n, splits, out);
  return dfh::check_launch("incep_is_splits_kernel");
}

int dfh_incep_stats(const float* act, int N, int D, double* mu, double* sigma, void* stream) {
  DFH_REQUIRE(act && mu && sigma, "null argument");
  DFH_REQUIRE(N >= 2, "the covariance needs at least two rows (N - 1 divides), got N = " + std::to_string(N));
  DFH_REQUIRE(D >= 1 && D <= 46336, "D must be in [1, 46336]");
  const unsigned tiles = (unsigned)((D + 63) / 64);
  if (int rc = launch_mean(act, mu, 1, N, D, (hipStream_t)stream)) return rc;
  hipLaunchKernelGGL(incep_cov_kernel, dim3(tiles, tiles), dim3(THREADS), 0, (hipStream_t)stream, act, mu, sigma, N, D);
  return dfh::check_launch("incep_cov_kernel");
}

}  // extern "C"

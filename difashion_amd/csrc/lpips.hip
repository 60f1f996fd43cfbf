// LPIPS on VGG16: lpips.LPIPS(net="vgg", version="0.1", spatial=False) as the reference's evaluation calls it
// (Evaluation/eval_utils.py:473-501, :769-821).
//
// Replaces (arithmetic):
//   * im2tensor_lpips for uint8 images (a 256-entry table the caller hands in) and the ScalingLayer (x - shift[c]) / scale[c]:
//     lpips_prep_kernel, bit for bit torch's separate ops;
//   * torchvision's vgg16().features up to relu5_3: thirteen relu(conv2d(x, w, b, padding=1)) on v_mfma_f32_16x16x4_f32 as an implicit
//     GEMM (lpips_conv3x3_relu_kernel) and four max_pool2d(2, 2) (lpips_maxpool2x2_kernel);
//   * normalize_tensor (eps OUTSIDE the root), the squared difference, the 1 x 1 lin conv and the spatial mean of the five taps, and
//     their sum: lpips_layer_score_kernel + lpips_finish_kernel;
//   * torch.argmin over the K candidates of a row (:787, :814): lpips_group_argmin_kernel.
//
// Activations are NHWC fp32, the two images of pair p ride as images p and pairs + p of ONE batch.  fp32 only, the same in both storage
// builds; no atomics; nothing is allocated here.  Every output value is a function of its own pair alone: the conv tile, the score grid
// and the order of every sum depend on (H, W) and the layer, never on the batch.
//
// Accumulation contract of the conv: per input-channel chunk of 32 (288 products; the first layer is one chunk of 4 padded channels,
// 36 products) the nine taps accumulate into FRESH accumulators, and the chunk's sum is then added to the running sum with a plain
// fp32 add.  One accumulator run down all of K (up to 4608 products) is a chain whose rounding error grows with K.
//
// This file is compiled with -ffp-contract=off (Makefile): prep and the pair score follow torch's separate ops.
#include <algorithm>
#include <cmath>
#include <new>
#include <utility>

#include "../../include/difashion_hip.h"
#include "dfh_common.h"
#include "f32_tile.h"

namespace {

constexpr int THREADS = 256;
// the conv tile: 8 x 16 output pixels x 64 output channels a workgroup; wave w owns patch rows MF w .. MF w + MF - 1 (MF = 2 M fragments,
// one patch row of 16 pixels each) x all 64 channels (four N fragments)
constexpr int TH = 8, TW = 16, BN = 64, CHUNK = 32, MF = TH / 4;
constexpr int HALO_W = TW + 2, HALO_PIX = (TH + 2) * HALO_W;      // 18, 180: the patch with its one-pixel halo
// k-major LDS images: In[channel][halo pixel], Ws[channel][C_out]; both row strides are 16 mod 32, so the four k-rows that the 64 lanes
// of a fragment read (lane / 16) fall on disjoint bank ranges in each 32-lane half (clip_gemm_f32_kernel's layout)
constexpr int IN_LD = 208, W_LD = 80;
constexpr int PART = 256;                                        // partial sums a (pair, layer): DFH_LPIPS_PARTIALS
constexpr int NCONV = 13, NTAP = 5;

static_assert(IN_LD >= HALO_PIX && IN_LD % 32 == 16 && W_LD % 32 == 16 && W_LD >= BN, "LDS row strides");
static_assert(PART == DFH_LPIPS_PARTIALS && NTAP == DFH_LPIPS_NUM_LAYERS, "header constants");

// ------------------------------------------------------------------ prep: (source form) -> ScalingLayer -> NHWC, 4 channels
__global__ __launch_bounds__(THREADS) void lpips_prep_kernel(const void* __restrict__ src, int src_kind, const float* __restrict__ lut,
                                                             const float* __restrict__ shift, const float* __restrict__ scale, int normalize,
                                                             float4* __restrict__ out, long total, long HW) {
  const long t = (long)blockIdx.x * THREADS + threadIdx.x;
  if (t >= total) return;
  float v[3];
  if (src_kind == DFH_LPIPS_SRC_U8_HWC) {
    const uint8_t* s = (const uint8_t*)src + t * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = lut[s[c]];
  } else {
    const long img = t / HW, p = t - img * HW;
    const float* s = (const float*)src + img * 3 * HW + p;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      v[c] = s[c * HW];
      if (normalize) v[c] = 2.0f * v[c] - 1.0f;
    }
  }
  out[t] = make_float4((v[0] - shift[0]) / scale[0], (v[1] - shift[1]) / scale[1], (v[2] - shift[2]) / scale[2], 0.0f);
}

// ------------------------------------------------------------------ weights: torch [C_out][w_cin][3][3] -> [chunk][tap][channel][C_out]
__global__ __launch_bounds__(THREADS) void lpips_pack_conv_kernel(const float* __restrict__ w, float* __restrict__ packed, int w_cin, int cc,
                                                                  int C_out, long total) {
  const long t = (long)blockIdx.x * THREADS + threadIdx.x;
  if (t >= total) return;
  const int n = (int)(t % C_out);
  long r = t / C_out;
  const int c = (int)(r % cc);
  r /= cc;
  const int tap = (int)(r % 9), chunk = (int)(r / 9);
  const int ci = chunk * cc + c;
  packed[t] = ci < w_cin ? w[((long)n * w_cin + ci) * 9 + tap] : 0.0f;         // channels beyond w_cin (the first layer's fourth): 0
}

// ------------------------------------------------------------------ out = relu(conv3x3(x, pad 1) + bias), NHWC fp32
// CC: input channels a chunk (32; 4 for the first layer).  grid: x = (spatial tile, C_out tile) with the C_out tile fastest, z = image.
template <int CC>
__global__ __launch_bounds__(THREADS) void lpips_conv3x3_relu_kernel(const float* __restrict__ x, const float* __restrict__ wp,
                                                                     const float* __restrict__ bias, float* __restrict__ out, int H, int W,
                                                                     int C_in, int C_out, int tiles_x) {
  __shared__ float In[CC * IN_LD];
  __shared__ __attribute__((aligned(16))) float Ws[CC * W_LD];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nco = C_out / BN;
  const int tile = blockIdx.x / nco, co0 = (blockIdx.x - tile * nco) * BN;
  const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
  const int y0 = ty * TH, x0 = tx * TW;
  const long img = blockIdx.z;
  const float* xin = x + img * H * W * C_in;
  const int fr = lane & 15, fk = lane >> 4;

  // one tap's weights of one chunk: CC rows of 64 floats = CC * 16 float4, two a thread at CC = 32 (named registers: an array indexed
  // in a rolled loop goes to scratch)
  constexpr int WV = CC * (BN / 4);
  static_assert(WV == 2 * THREADS || WV <= THREADS, "weight stage: at most two float4 a thread");
  constexpr bool W2 = WV > THREADS;
  const int wk = tid >> 4, wn = 4 * (tid & 15);
  float4 rw0 = make_float4(0.f, 0.f, 0.f, 0.f), rw1 = rw0;
  auto fetch_w = [&](int chunk, int tap) {
    const float* base = wp + ((long)(chunk * 9 + tap) * CC) * C_out + co0 + wn;
    if (tid < WV) rw0 = *(const float4*)(base + (long)wk * C_out);
    if (W2) rw1 = *(const float4*)(base + (long)(wk + 16) * C_out);
  };
  auto stash_w = [&]() {
    if (tid < WV) *(float4*)&Ws[wk * W_LD + wn] = rw0;
    if (W2) *(float4*)&Ws[(wk + 16) * W_LD + wn] = rw1;
  };
  // the patch with its halo, zeros outside the image, ONCE a chunk: consecutive lanes take consecutive pixels of one channel quad
  auto stage_input = [&](int chunk) {
    for (int idx = tid; idx < (CC / 4) * HALO_PIX; idx += THREADS) {
      const int c4 = idx / HALO_PIX, p = idx - c4 * HALO_PIX;
      const int py = p / HALO_W, px = p - py * HALO_W;
      const int gy = y0 + py - 1, gx = x0 + px - 1;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (gy >= 0 && gy < H && gx >= 0 && gx < W) v = *(const float4*)(xin + ((long)gy * W + gx) * C_in + chunk * CC + 4 * c4);
      float* d = &In[(4 * c4) * IN_LD + p];
      d[0] = v.x; d[IN_LD] = v.y; d[2 * IN_LD] = v.z; d[3 * IN_LD] = v.w;
    }
  };

  const f32x4_t zero = f32x4_t{0.f, 0.f, 0.f, 0.f};
  f32x4_t sum[MF][4];
#pragma unroll
  for (int i = 0; i < MF; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) sum[i][j] = zero;

  const int nchunks = C_in / CC;
  fetch_w(0, 0);
  for (int chunk = 0; chunk < nchunks; ++chunk) {
    f32x4_t t[1][MF][4];                               // FRESH accumulators: this chunk's nine taps
#pragma unroll
    for (int i = 0; i < MF; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) t[0][i][j] = zero;
#pragma unroll 1
    for (int tap = 0; tap < 9; ++tap) {
      __syncthreads();                                 // the previous step's fragment reads are done
      stash_w();
      if (tap == 0) stage_input(chunk);
      __syncthreads();
      if (tap < 8) fetch_w(chunk, tap + 1);
      else if (chunk + 1 < nchunks) fetch_w(chunk + 1, 0);
      const int ky = tap / 3, kx = tap - ky * 3;
      // A fragment i: patch row MF wave + i shifted by the tap, one halo row (HALO_W) below fragment i - 1
      dfh::mma_ktile<1, MF, 4, CC>(&In[(MF * wave + ky) * HALO_W + kx + fr], IN_LD, HALO_W, Ws + fr, W_LD, fk, t);
    }
#pragma unroll
    for (int i = 0; i < MF; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) sum[i][j] = sum[i][j] + t[0][i][j];      // the plain fp32 add of the contract
  }
  // C layout of 16x16x4: acc[r] = C[4 * (lane / 16) + r][lane % 16] = (pixel 4 fk + r of the patch row, channel fr of the fragment)
#pragma unroll
  for (int i = 0; i < MF; ++i) {
    const int y = y0 + MF * wave + i;
    if (y >= H) continue;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = co0 + 16 * j + fr;
      const float bv = bias[n];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int xx = x0 + 4 * fk + r;
        const float v = sum[i][j][r] + bv;
        if (xx < W) out[((img * H + y) * W + xx) * C_out + n] = v <= 0.0f ? 0.0f : v;      // torch's relu: a NaN stays a NaN
      }
    }
  }
}

// ------------------------------------------------------------------ max_pool2d(2, 2), floor mode, NHWC, float4 along channels
__global__ __launch_bounds__(THREADS) void lpips_maxpool2x2_kernel(const float4* __restrict__ x, float4* __restrict__ out, int H, int W, int C4,
                                                                   int OH, int OW, long total) {
  const long t = (long)blockIdx.x * THREADS + threadIdx.x;
  if (t >= total) return;
  const int c = (int)(t % C4);
  long r = t / C4;
  const int ox = (int)(r % OW);
  r /= OW;
  const int oy = (int)(r % OH);
  const long n = r / OH;
  float4 m = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
#pragma unroll
  for (int dy = 0; dy < 2; ++dy)
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
      const float4 v = x[((n * H + 2 * oy + dy) * W + 2 * ox + dx) * C4 + c];
      using dfh::pool_max;
      m.x = pool_max(m.x, v.x); m.y = pool_max(m.y, v.y); m.z = pool_max(m.z, v.z); m.w = pool_max(m.w, v.w);
    }
  out[t] = m;
}

// ------------------------------------------------------------------ one tap layer of every pair -> partial sums
// grid (G, pairs), G = score_groups(HW): workgroup g's wave w walks pixels 4 g + w, 4 g + w + 4 G, ...; one wave per pixel: it
// wave-reduces sum x^2 and sum y^2, and every lane adds its channels' share of
//   sum_c w_c (x_c / (sqrt(sum x^2) + 1e-10) - y_c / (sqrt(sum y^2) + 1e-10))^2
// to a running sum of its own (a short chain: HW / (4 G) pixels); the lanes meet in one wave tree at the end.
// partial[pair * part_stride + g] = ((wave 0 + wave 1) + wave 2) + wave 3
__global__ __launch_bounds__(THREADS) void lpips_layer_score_kernel(const float* __restrict__ feat, const float* __restrict__ lw,
                                                                    float* __restrict__ partial, int pairs, long HW, int C, int G,
                                                                    int part_stride) {
  __shared__ float wsum[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = blockIdx.x, pair = blockIdx.y;
  const float* xb = feat + (long)pair * HW * C;
  const float* yb = feat + ((long)pairs + pair) * HW * C;
  float wl[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) wl[q] = lane + 64 * q < C ? lw[lane + 64 * q] : 0.0f;
  float acc = 0.0f;
  for (long pix = 4L * g + wave; pix < HW; pix += 4L * G) {              // wave-uniform trip count: the shuffles see 64 live lanes
    const float* xp = xb + pix * C;
    const float* yp = yb + pix * C;
    float xv[8], yv[8], sx = 0.0f, sy = 0.0f;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int c = lane + 64 * q;
      xv[q] = c < C ? xp[c] : 0.0f;
      yv[q] = c < C ? yp[c] : 0.0f;
      sx = fmaf(xv[q], xv[q], sx);
      sy = fmaf(yv[q], yv[q], sy);
    }
    const float nx = sqrtf(wave_sum(sx)) + 1e-10f, ny = sqrtf(wave_sum(sy)) + 1e-10f;      // the eps is OUTSIDE the root
    float d = 0.0f;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const float df = xv[q] / nx - yv[q] / ny;
      d = fmaf(wl[q], df * df, d);
    }
    acc += d;
  }
  acc = wave_sum(acc);
  if (lane == 0) wsum[wave] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partial[(long)pair * part_stride + g] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

struct FinishArgs { int layers; int G[NTAP]; float hw[NTAP]; };

// One workgroup a pair.  per_layer[pair][l] = (the partials of (pair, l) added in index order) / pixels; the add is compensated
// (Kahan), so its error does not grow with the number of partials: a plain chain over 256 of them alone sits at 2e-7 of the sum, four
// times torch's own fp32 distance from fp64 on a 16 x 16 image.  distance[pair] = the layers added in order 0 .. 4 with plain adds.
__global__ __launch_bounds__(THREADS) void lpips_finish_kernel(const float* __restrict__ partial, const FinishArgs a, float* __restrict__ distance,
                                                               float* __restrict__ per_layer) {
  __shared__ float part[NTAP * PART];
  __shared__ float layer[NTAP];
  const int pair = blockIdx.x;
  for (int i = threadIdx.x; i < a.layers * PART; i += THREADS) {
    const int l = i / PART, g = i - l * PART;
    part[i] = g < a.G[l] ? partial[((long)pair * a.layers + l) * PART + g] : 0.0f;
  }
  __syncthreads();
  if ((int)threadIdx.x < a.layers) {
    const int l = threadIdx.x;
    float s = 0.0f, comp = 0.0f;
    for (int g = 0; g < a.G[l]; ++g) dfh::kahan_add(s, comp, part[l * PART + g]);
    layer[l] = s / a.hw[l];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float total = 0.0f;
    for (int l = 0; l < a.layers; ++l) {
      if (per_layer) per_layer[(long)pair * a.layers + l] = layer[l];
      total += layer[l];
    }
    if (distance) distance[pair] = total;
  }
}

// torch.argmin's order: a NaN is the minimum, the lowest index wins among equals (and among NaNs)
__global__ __launch_bounds__(THREADS) void lpips_group_argmin_kernel(const float* __restrict__ scores, int64_t* __restrict__ pred, int rows, int K) {
  const int r = blockIdx.x * THREADS + threadIdx.x;
  if (r >= rows) return;
  const float* s = scores + (long)r * K;
  float best = s[0];
  int bk = 0;
  for (int k = 1; k < K; ++k) {
    const float v = s[k];
    if (best != best) break;                             // the first NaN stays
    if (v != v || v < best) { best = v; bk = k; }
  }
  pred[r] = bk;
}

// ------------------------------------------------------------------ host: the plan
struct ConvDesc { int cin, cin_pad, cout, level, wi, bi; size_t packed_off; };      // wi, bi: table indices; packed_off in floats
constexpr int VGG_COUT[NCONV] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
constexpr int VGG_LEVEL[NCONV] = {0, 0, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4};
constexpr int VGG_INDEX[NCONV] = {0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28};      // torchvision's vgg16().features
constexpr int TAP_C[NTAP] = {64, 128, 256, 512, 512};
constexpr int MAX_SIDE = 8192, MAX_IMAGES = 65535;

int score_groups(long HW) { return (int)std::min<long>(PART, (HW + 3) / 4); }

// ping | pong (2 pairs images x H x W x 64 floats each: the widest activation is the first level's) | partial sums
struct LpipsWorkspace : dfh::WorkspaceCarve {
  float *ping, *pong, *partial;
  LpipsWorkspace(void* base, size_t pairs, size_t H, size_t W) : dfh::WorkspaceCarve(base, 1) {
    const size_t act = 2 * pairs * H * W * 64;
    ping = take(act); pong = take(act); partial = take(pairs * NTAP * PART);
  }
};

using dfh::aligned16;

int launch_prep(const void* src, int src_kind, const float* lut, const float* shift, const float* scale, int normalize, float* out, long n,
                int H, int W, hipStream_t s) {
  const long total = n * H * W;
  hipLaunchKernelGGL(lpips_prep_kernel, dim3((unsigned)((total + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, src, src_kind, lut, shift, scale,
                     normalize, (float4*)out, total, (long)H * W);
  return dfh::check_launch("lpips_prep_kernel");
}

int launch_pack(const float* w, float* packed, int w_cin, int cin_pad, int cout, hipStream_t s) {
  const long total = 9L * cin_pad * cout;
  hipLaunchKernelGGL(lpips_pack_conv_kernel, dim3((unsigned)((total + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, w, packed, w_cin,
                     std::min(cin_pad, CHUNK), cout, total);
  return dfh::check_launch("lpips_pack_conv_kernel");
}

int launch_conv(const float* x, const float* wp, const float* bias, float* out, int n, int H, int W, int cin, int cout, hipStream_t s) {
  const int tiles_x = (W + TW - 1) / TW, tiles_y = (H + TH - 1) / TH;
  const dim3 grid((unsigned)(tiles_x * tiles_y * (cout / BN)), 1, (unsigned)n);
  const double px = (double)n * H * W;
  dfh::ProfScope ps(dfh::PC_CONV3, 2.0 * px * 9 * cin * cout, 4.0 * (px * (cin + cout) + 9.0 * cin * cout), s);
  if (cin == 4) hipLaunchKernelGGL(lpips_conv3x3_relu_kernel<4>, grid, dim3(THREADS), 0, s, x, wp, bias, out, H, W, cin, cout, tiles_x);
  else hipLaunchKernelGGL(lpips_conv3x3_relu_kernel<CHUNK>, grid, dim3(THREADS), 0, s, x, wp, bias, out, H, W, cin, cout, tiles_x);
  return dfh::check_launch("lpips_conv3x3_relu_kernel");
}

int launch_pool(const float* x, float* out, int n, int H, int W, int C, hipStream_t s) {
  const int OH = H / 2, OW = W / 2;
  const long total = (long)n * OH * OW * (C / 4);
  hipLaunchKernelGGL(lpips_maxpool2x2_kernel, dim3((unsigned)((total + THREADS - 1) / THREADS)), dim3(THREADS), 0, s, (const float4*)x, (float4*)out,
                     H, W, C / 4, OH, OW, total);
  return dfh::check_launch("lpips_maxpool2x2_kernel");
}

int launch_score(const float* feat, const float* lw, float* partial, int pairs, int H, int W, int C, int part_stride, hipStream_t s) {
  const long HW = (long)H * W;
  const int G = score_groups(HW);
  hipLaunchKernelGGL(lpips_layer_score_kernel, dim3((unsigned)G, (unsigned)pairs), dim3(THREADS), 0, s, feat, lw, partial, pairs, HW, C, G,
                     part_stride);
  return dfh::check_launch("lpips_layer_score_kernel");
}

int launch_finish(const float* partial, const FinishArgs& a, float* distance, float* per_layer, int pairs, hipStream_t s) {
  hipLaunchKernelGGL(lpips_finish_kernel, dim3((unsigned)pairs), dim3(THREADS), 0, s, partial, a, distance, per_layer);
  return dfh::check_launch("lpips_finish_kernel");
}

}  // namespace

struct dfh_lpips {
  dfh::ParamList t;
  int shift, scale, lin[NTAP];
  ConvDesc conv[NCONV];
  size_t packed_floats;

  dfh_lpips() {
    shift = t.add_param("scaling_layer.shift", {1, 3, 1, 1});
    scale = t.add_param("scaling_layer.scale", {1, 3, 1, 1});
    int cin = 3;
    packed_floats = 0;
    for (int i = 0; i < NCONV; ++i) {
      ConvDesc& c = conv[i];
      const std::string p = "net.slice" + std::to_string(VGG_LEVEL[i] + 1) + "." + std::to_string(VGG_INDEX[i]) + ".";
      c.cin = cin; c.cin_pad = (cin + 3) & ~3; c.cout = VGG_COUT[i]; c.level = VGG_LEVEL[i];
      c.wi = t.add_param(p + "weight", {c.cout, c.cin, 3, 3});
      c.bi = t.add_param(p + "bias", {c.cout});
      c.packed_off = packed_floats;
      packed_floats += (size_t)9 * c.cin_pad * c.cout;
      cin = c.cout;
    }
    for (int l = 0; l < NTAP; ++l) lin[l] = t.add_param("lin" + std::to_string(l) + ".model.1.weight", {1, TAP_C[l], 1, 1});
  }

  // what every entry point that takes the parameter table requires of it, on the host, before any HIP call
  int require_params(const float* const* params, int count, const char* who) const {
    return dfh::require_params(t, params, count, who, "dfh_lpips_num_params (" + std::to_string(DFH_LPIPS_NUM_PARAMS) + ")");
  }
};

extern "C" {

int dfh_lpips_create(const dfh_lpips_config* cfg, dfh_lpips** out) {
  DFH_REQUIRE(cfg && out, "null argument");
  DFH_REQUIRE(cfg->net == DFH_LPIPS_NET_VGG16, "unsupported network " + std::to_string(cfg->net) +
              ": only VGG16 (DFH_LPIPS_NET_VGG16, lpips' net='vgg') is built; 'alex' and 'squeeze' are out of scope");
  dfh_lpips* p = new (std::nothrow) dfh_lpips();
  DFH_REQUIRE(p != nullptr, "out of host memory");
  *out = p;
  return 0;
}

void dfh_lpips_destroy(dfh_lpips* c) { delete c; }
int dfh_lpips_num_params(const dfh_lpips* c) { return c ? c->t.num_params() : 0; }
const char* dfh_lpips_param_name(const dfh_lpips* c, int i) { return c ? c->t.param_name(i) : ""; }
int dfh_lpips_param_ndim(const dfh_lpips* c, int i) { return c ? c->t.param_ndim(i) : 0; }
int dfh_lpips_param_dim(const dfh_lpips* c, int i, int d) { return c ? c->t.param_dim(i, d) : 0; }
size_t dfh_lpips_packed_bytes(const dfh_lpips* c) { return c ? c->packed_floats * sizeof(float) : 0; }

size_t dfh_lpips_workspace_bytes(const dfh_lpips* c, int pairs, int H, int W) {
  if (!c || pairs < 1 || H < 16 || W < 16 || H > MAX_SIDE || W > MAX_SIDE) return 0;
  return LpipsWorkspace(nullptr, pairs, H, W).bytes();
}

int dfh_lpips_pack(dfh_lpips* c, const float* const* params, int count, void* packed, void* stream) {
  DFH_REQUIRE(c, "null argument: ctx");
  if (int rc = c->require_params(params, count, "dfh_lpips_pack")) return rc;
  DFH_REQUIRE(packed, "null argument: packed");
  DFH_REQUIRE(aligned16(packed), "packed must be 16-byte aligned");
  for (const ConvDesc& d : c->conv)
    if (int rc = launch_pack(params[d.wi], (float*)packed + d.packed_off, d.cin, d.cin_pad, d.cout, (hipStream_t)stream)) return rc;
  return 0;
}

int dfh_lpips_forward(dfh_lpips* c, const float* const* params, int count, const void* packed, const void* in0, const void* in1, int src_kind,
                      const float* lut, int normalize, int pairs, int H, int W, float* distance, float* per_layer, void* workspace,
                      size_t workspace_bytes, void* stream) {
  DFH_REQUIRE(c, "null argument: ctx");
  if (int rc = c->require_params(params, count, "dfh_lpips_forward")) return rc;
  DFH_REQUIRE(packed, "null argument: packed");
  DFH_REQUIRE(in0, "null argument: in0");
  DFH_REQUIRE(in1, "null argument: in1");
  DFH_REQUIRE(distance, "null argument: distance");
  DFH_REQUIRE(workspace, "null argument: workspace");
  DFH_REQUIRE(src_kind == DFH_LPIPS_SRC_U8_HWC || src_kind == DFH_LPIPS_SRC_F32_CHW, "src_kind must be 0 (uint8 HWC) or 1 (fp32 CHW)");
  DFH_REQUIRE(src_kind != DFH_LPIPS_SRC_U8_HWC || lut, "null argument: lut (the uint8 form reads the 256-entry table)");
  DFH_REQUIRE(src_kind != DFH_LPIPS_SRC_U8_HWC || !normalize, "normalize applies to the fp32 form only (uint8 images go through the table)");
  DFH_REQUIRE(aligned16(packed), "packed must be 16-byte aligned");
  DFH_REQUIRE(aligned16(in0), "in0 must be 16-byte aligned");
  DFH_REQUIRE(aligned16(in1), "in1 must be 16-byte aligned");
  DFH_REQUIRE(aligned16(lut), "lut must be 16-byte aligned");
  DFH_REQUIRE(((uintptr_t)workspace & 255) == 0, "workspace must be 256-byte aligned");
  DFH_REQUIRE(H >= 16 && W >= 16, "H and W must be at least 16: four 2 x 2 pools leave the fifth level empty below that");
  DFH_REQUIRE(H <= MAX_SIDE && W <= MAX_SIDE, "H and W must be at most 8192");
  DFH_REQUIRE(pairs >= 1 && 2 * pairs <= MAX_IMAGES, "pairs must be in [1, 32767] a call");
  DFH_REQUIRE(workspace_bytes >= dfh_lpips_workspace_bytes(c, pairs, H, W), "workspace smaller than dfh_lpips_workspace_bytes");
  hipStream_t s = (hipStream_t)stream;
  const LpipsWorkspace w(workspace, pairs, H, W);
  const float* const* P = params;
  const int n = 2 * pairs;
  float *cur = w.pong, *other = w.ping;
  if (int rc = launch_prep(in0, src_kind, lut, P[c->shift], P[c->scale], normalize, cur, pairs, H, W, s)) return rc;
  if (int rc = launch_prep(in1, src_kind, lut, P[c->shift], P[c->scale], normalize, cur + (size_t)pairs * H * W * 4, pairs, H, W, s)) return rc;
  FinishArgs fa;
  fa.layers = NTAP;
  int h = H, wd = W, ci = 0, ch = 4;
  for (int level = 0; level < NTAP; ++level) {
    if (level > 0) {
      if (int rc = launch_pool(cur, other, n, h, wd, ch, s)) return rc;
      std::swap(cur, other);
      h /= 2; wd /= 2;
    }
    for (; ci < NCONV && c->conv[ci].level == level; ++ci) {
      const ConvDesc& d = c->conv[ci];
      if (int rc = launch_conv(cur, (const float*)packed + d.packed_off, P[d.bi], other, n, h, wd, d.cin_pad, d.cout, s)) return rc;
      std::swap(cur, other);
      ch = d.cout;
    }
    // the tap is read where the conv left it; nothing of it is kept
    if (int rc = launch_score(cur, P[c->lin[level]], w.partial + (size_t)level * PART, pairs, h, wd, ch, NTAP * PART, s)) return rc;
    fa.G[level] = score_groups((long)h * wd);
    fa.hw[level] = (float)((long)h * wd);
  }
  return launch_finish(w.partial, fa, distance, per_layer, pairs, s);
}

int dfh_lpips_group_argmin(const float* scores, int64_t* pred, int rows, int K, void* stream) {
  DFH_REQUIRE(scores, "null argument: scores");
  DFH_REQUIRE(pred, "null argument: pred");
  DFH_REQUIRE(rows >= 1 && K >= 1, "rows / K must be positive");
  hipLaunchKernelGGL(lpips_group_argmin_kernel, dim3((unsigned)((rows + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)stream, scores, pred,
                     rows, K);
  return dfh::check_launch("lpips_group_argmin_kernel");
}

// ---- op level
int dfh_lpips_prep(const void* src, int src_kind, const float* lut, const float* shift, const float* scale, int normalize, float* out, int n,
                   int H, int W, void* stream) {
  DFH_REQUIRE(src, "null argument: src");
  DFH_REQUIRE(shift && scale, "null argument: shift / scale");
  DFH_REQUIRE(out, "null argument: out");
  DFH_REQUIRE(src_kind == DFH_LPIPS_SRC_U8_HWC || src_kind == DFH_LPIPS_SRC_F32_CHW, "src_kind must be 0 (uint8 HWC) or 1 (fp32 CHW)");
  DFH_REQUIRE(src_kind != DFH_LPIPS_SRC_U8_HWC || lut, "null argument: lut (the uint8 form reads the 256-entry table)");
  DFH_REQUIRE(src_kind != DFH_LPIPS_SRC_U8_HWC || !normalize, "normalize applies to the fp32 form only (uint8 images go through the table)");
  DFH_REQUIRE(aligned16(out), "out must be 16-byte aligned");
  DFH_REQUIRE(n >= 1 && H >= 1 && W >= 1 && H <= MAX_SIDE && W <= MAX_SIDE, "n / H / W must be positive, H and W at most 8192");
  return launch_prep(src, src_kind, lut, shift, scale, normalize, out, n, H, W, (hipStream_t)stream);
}

int dfh_lpips_conv3x3_relu(const float* x, const float* weight, int w_cin, const float* bias, float* packed, float* out, int n, int H, int W,
                           int C_in, int C_out, void* stream) {
  DFH_REQUIRE(x && weight && bias && packed && out, "null argument");
  DFH_REQUIRE(C_in == 4 || (C_in >= CHUNK && C_in % CHUNK == 0), "C_in must be 4 (the padded first layer) or a multiple of 32");
  DFH_REQUIRE(w_cin >= 1 && w_cin <= C_in, "w_cin must be in [1, C_in]");
  DFH_REQUIRE(C_out >= BN && C_out % BN == 0, "C_out must be a multiple of 64");
  DFH_REQUIRE(n >= 1 && n <= MAX_IMAGES && H >= 1 && W >= 1 && H <= MAX_SIDE && W <= MAX_SIDE, "n must be in [1, 65535], H and W in [1, 8192]");
  DFH_REQUIRE(aligned16(x) && aligned16(packed) && aligned16(out), "x / packed / out must be 16-byte aligned");
  if (int rc = launch_pack(weight, packed, w_cin, C_in, C_out, (hipStream_t)stream)) return rc;
  return launch_conv(x, packed, bias, out, n, H, W, C_in, C_out, (hipStream_t)stream);
}

int dfh_lpips_maxpool2x2(const float* x, float* out, int n, int H, int W, int C, void* stream) {
  DFH_REQUIRE(x && out, "null argument");
  DFH_REQUIRE(C >= 4 && C % 4 == 0, "C must be a multiple of 4");
  DFH_REQUIRE(n >= 1 && H >= 2 && W >= 2 && H <= MAX_SIDE && W <= MAX_SIDE, "n must be positive, H and W in [2, 8192]");
  DFH_REQUIRE(aligned16(x) && aligned16(out), "x / out must be 16-byte aligned");
  return launch_pool(x, out, n, H, W, C, (hipStream_t)stream);
}

int dfh_lpips_layer_score(const float* feat, const float* lin_weight, int pairs, int H, int W, int C, float* partial, float* out, void* stream) {
  DFH_REQUIRE(feat && lin_weight && partial && out, "null argument");
  DFH_REQUIRE(C >= 1 && C <= 512, "C must be in [1, 512]");
  DFH_REQUIRE(pairs >= 1 && pairs <= MAX_IMAGES && H >= 1 && W >= 1 && H <= MAX_SIDE && W <= MAX_SIDE, "pairs must be in [1, 65535], H and W in [1, 8192]");
  if (int rc = launch_score(feat, lin_weight, partial, pairs, H, W, C, PART, (hipStream_t)stream)) return rc;
  FinishArgs fa;
  fa.layers = 1;
  fa.G[0] = score_groups((long)H * W);
  fa.hw[0] = (float)((long)H * W);
  return launch_finish(partial, fa, nullptr, out, pairs, (hipStream_t)stream);
}

}  // extern "C"

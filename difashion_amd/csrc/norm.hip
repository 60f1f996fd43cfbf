// GroupNorm(32)(+SiLU) and LayerNorm for NHWC bf16 activations on gfx950.
// Reference call sites: diffusers ResnetBlock2D norm1/norm2 + SiLU, conv_norm_out, Transformer2DModel.norm
// (eps 1e-6, no activation) and BasicTransformerBlock norm1/2/3 reached through
// DiFashion/models/difashion.py:249-253,518-523.
//
// HBM-bound kernels (DESIGN.md "Kernels/norm"): every access is a 16-byte bf16x8 vector, each
// thread owns a fixed channel octet so per-channel scale/shift live in registers, statistics are
// reduced deterministically (fixed order, no float atomics): per-thread registers -> LDS ->
// 32 group lanes -> [B][chunk][32][2] partials -> summed in chunk order by the apply kernel.
// The channel concat of the up-path (torch.cat([h, skip], dim=1)) is fused into the read: an
// octet below C0/8 comes from src0, the rest from src1.
#include "dfh_common.h"
#include "norm.h"
#include "norm_steps.h"
#include "walk_knobs.h"
#include <cstring>
#include <cstdlib>

namespace {

// the accumulation body of gn_stats_kernel (a function, not a lambda as in gn_bwd_stats_kernel: with a lambda the compiler schedules
// the load batches into 154 VGPRs instead of 94, three waves a SIMD instead of five)
DFH_DEVICE void gn_sum_sq(const uint4& raw, float* s, float* q) {
  float f[8];
  unpack8(raw, f);
#pragma unroll
  for (int k = 0; k < 8; ++k) { s[k] += f[k]; q[k] += f[k] * f[k]; }
}

// grid (chunks, B); block = roundup64(C8 * PL) threads; thread -> (pixel lane pl, octet o)
// (<= 512 threads: C <= 4096; without the bound the compiler budgets for 1024 threads, 128 VGPRs, and spills 28 of them inside the load loop)
__global__ __launch_bounds__(512) void gn_stats_kernel(const GnArgs a) {
  extern __shared__ __attribute__((aligned(16))) float red[];   // [PL][C][2]
  const int C8 = a.C >> 3;
  const int tid = threadIdx.x;
  const int o = tid % C8, pl = tid / C8;
  const int b = blockIdx.y;
  const int p_begin = blockIdx.x * a.pix_per_chunk;
  const int p_end = min(a.HW, p_begin + a.pix_per_chunk);
  float s[8], q[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) { s[k] = 0.f; q[k] = 0.f; }
  if (pl < a.PL) {
    // batches of 8, then 4 independent 16-byte loads in flight per thread (a single dependent load per iteration is
    // latency-bound at ~1 TB/s); accumulation order stays p-ascending, so results are unchanged.
    int p = p_begin + pl;
    for (; p + 7 * a.PL < p_end; p += 8 * a.PL) {
      uint4 v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = *gn_src(a, b, p + u * a.PL, o);
#pragma unroll
      for (int u = 0; u < 8; ++u) gn_sum_sq(v[u], s, q);
    }
    for (; p + 3 * a.PL < p_end; p += 4 * a.PL) {
      uint4 v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) v[u] = *gn_src(a, b, p + u * a.PL, o);
#pragma unroll
      for (int u = 0; u < 4; ++u) gn_sum_sq(v[u], s, q);
    }
    for (; p < p_end; p += a.PL) gn_sum_sq(*gn_src(a, b, p, o), s, q);
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      red[((pl * a.C) + o * 8 + k) * 2 + 0] = s[k];
      red[((pl * a.C) + o * 8 + k) * 2 + 1] = q[k];
    }
  }
  __syncthreads();
  if (tid < a.G) {
    const int cpg = a.C / a.G;
    float ss = 0.f, qq = 0.f;
    for (int l = 0; l < a.PL; ++l)
      for (int c = tid * cpg; c < (tid + 1) * cpg; ++c) {
        ss += red[(l * a.C + c) * 2 + 0];
        qq += red[(l * a.C + c) * 2 + 1];
      }
    // [b][group][chunk][2]: a group's partials are contiguous, the apply kernel reads them as float4s
    float* dst = a.partial + (((long)b * a.G + tid) * gridDim.x + blockIdx.x) * 2;
    dst[0] = ss; dst[1] = qq;
  }
}

// grid (achunks, B); same thread mapping; normalise (+SiLU) and write bf16 [B][HW][C].  The first GN_PRE pixels of a thread are
// loaded BEFORE the statistics are reduced: partials -> barrier -> gamma / beta -> data were three dependent memory round
// trips per block, and a block only lives for a handful of pixels per thread.
constexpr int GN_PRE = 6;
__global__ void gn_apply_kernel(const GnArgs a) {
  __shared__ float mean_s[64], rstd_s[64];
  const int C8 = a.C >> 3;
  const int tid = threadIdx.x;
  const int o = tid % C8, pl = tid / C8;
  const int b = blockIdx.y;
  const int cpg = a.C / a.G;
  const int p_begin = blockIdx.x * a.apix_per_chunk;
  const int p_end = min(a.HW, p_begin + a.apix_per_chunk);
  const bool live = pl < a.PL;
  uint4 pre[GN_PRE];
#pragma unroll
  for (int u = 0; u < GN_PRE; ++u) {
    const int p = p_begin + pl + u * a.PL;
    pre[u] = make_uint4(0u, 0u, 0u, 0u);
    if (live && p < p_end) pre[u] = *gn_src(a, b, p, o);
  }
  float gmr[8], btr[8];
  if (live && !a.out8) { load8f(a.gamma + o * 8, gmr); load8f(a.beta + o * 8, btr); }
  // statistics: the eight-runs order whenever the block has eight threads per group
  __shared__ float2 run_s[64][8];
  const float2 sums = gn_chunk_sums(a.partial, a.chunks, a.G, b, blockDim.x >= (unsigned)a.G * 8u, run_s);
  if (tid < a.G) {
    const float2 mr = gn_mean_rstd(sums, (float)a.HW * (float)cpg, a.eps);
    mean_s[tid] = mr.x;
    rstd_s[tid] = mr.y;
    if (a.stats_out && blockIdx.x == 0) {
      a.stats_out[((long)b * a.G + tid) * 2 + 0] = mr.x;
      a.stats_out[((long)b * a.G + tid) * 2 + 1] = mr.y;
    }
  }
  __syncthreads();
  if (!live) return;
  float sc[8], sh[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int c = o * 8 + k;
    const int g = c / cpg;
    const float w = (a.out8 ? a.q_mul : gmr[k]) * rstd_s[g];
    sc[k] = w;
    sh[k] = (a.out8 ? 0.f : btr[k]) - mean_s[g] * w;
  }
  auto emit = [&](const uint4& raw, int p) {
    float f[8];
    unpack8(raw, f);
    if (a.out8) {                                    // e4m3 of the normalised value under the static scale (GnArgs::out8)
#pragma unroll
      for (int k = 0; k < 8; ++k) f[k] = sat_e4m3(f[k] * sc[k] + sh[k]);
      uint2 w;
      w.x = pack4_e4m3(f[0], f[1], f[2], f[3]);
      w.y = pack4_e4m3(f[4], f[5], f[6], f[7]);
      *(uint2*)(a.out8 + ((long)(b * a.HW + p) * a.C + o * 8)) = w;
      return;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      float y = f[k] * sc[k] + sh[k];
      f[k] = a.silu ? silu_f(y) : y;
    }
    *(uint4*)(a.out + ((long)(b * a.HW + p) * a.C + o * 8)) = pack8(f);
  };
#pragma unroll
  for (int u = 0; u < GN_PRE; ++u) {
    const int p = p_begin + pl + u * a.PL;
    if (p < p_end) emit(pre[u], p);
  }
  int p = p_begin + pl + GN_PRE * a.PL;
  for (; p + 3 * a.PL < p_end; p += 4 * a.PL) {      // 4 loads in flight per thread
    uint4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = *gn_src(a, b, p + u * a.PL, o);
#pragma unroll
    for (int u = 0; u < 4; ++u) emit(v[u], p + u * a.PL);
  }
  for (; p < p_end; p += a.PL) emit(*gn_src(a, b, p, o), p);
}

// one wave per R token rows; exact two-pass variance in registers (C <= 8*64*MAXO).  The loads of all R rows (and gamma / beta)
// are issued before anything is reduced (norm_steps.h).
template <int MAXO, int R>
__global__ __launch_bounds__(256) void layernorm_kernel(const bf16_t* __restrict__ x, const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, bf16_t* __restrict__ y,
                                                        int M, int C, float eps) {
  const int lane = threadIdx.x & 63;
  const int row0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * R;
  if (row0 >= M) return;
  const int C8 = C >> 3;
  uint4 raw[R][MAXO];
  ln_load_rows<MAXO, R>(x, row0, M, C, lane, raw);
  float gg[MAXO][8], bb[MAXO][8];
#pragma unroll
  for (int i = 0; i < MAXO; ++i) {
    const int o = lane + i * 64;
    if (o < C8) { load8f(gamma + o * 8, gg[i]); load8f(beta + o * 8, bb[i]); }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (row0 + r >= M) break;
    float v[MAXO][8];
#pragma unroll
    for (int i = 0; i < MAXO; ++i) unpack8(raw[r][i], v[i]);
    ln_centre<MAXO>(v, lane, C);
    float q = 0.f;
    {
      // every square is ROUNDED before it is added: what this kernel has always computed (the compiler multiplied in pairs,
      // v_pk_mul_f32, and added the products one by one), but only by its own choice; stated here
#pragma clang fp contract(off)
#pragma unroll
      for (int i = 0; i < MAXO; ++i) {
        if (lane + i * 64 < C8) {
#pragma unroll
          for (int k = 0; k < 8; ++k) q += v[i][k] * v[i][k];
        }
      }
    }
    const float rstd = rsqrtf(wave_sum(q) / (float)C + eps);
#pragma unroll
    for (int i = 0; i < MAXO; ++i) {
      const int o = lane + i * 64;
      if (o < C8) {
        float f[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) f[k] = v[i][k] * rstd * gg[i][k] + bb[i][k];
        *(uint4*)(y + (long)(row0 + r) * C + o * 8) = pack8(f);
      }
    }
  }
}

}  // namespace

// ---- small tensors (16x16 / 8x8 levels): ONE launch.  A block owns one (batch, group) slab of
// HW x cpg <= 32768 elements, reads it once into registers (8-byte units = 4 channels of a pixel), reduces it in a fixed
// order (two-pass variance from the registers), normalises and writes.  The two-kernel path above spends ~2 x 8 us of launch
// and dependency latency on tensors that hold a few hundred KB.
template <int UNITS>
__global__ __launch_bounds__(256) void gn_small_kernel(const GnArgs a) {
  const int g = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int cpg = a.C / a.G, upp = cpg >> 2, total = a.HW * upp;
  const int cg = g * cpg;                                     // first channel of the group in the concatenated tensor
  const bool first = cg < a.C0;
  const bf16_t* src = first ? a.src0 + (long)b * a.HW * a.C0 + cg : a.src1 + (long)b * a.HW * a.C1 + (cg - a.C0);
  const int ldc = first ? a.C0 : a.C1;
  __shared__ float red[8];
  // the group's gamma / beta go to LDS once: read per unit from global they were two more loads for every 8-byte data load
  __shared__ __attribute__((aligned(16))) float gam_s[256], bet_s[256];
  const bool gb_lds = cpg <= 256;
  if (gb_lds && tid < cpg && !a.out8) { gam_s[tid] = a.gamma[cg + tid]; bet_s[tid] = a.beta[cg + tid]; }
  float v[UNITS][4];
  int pix[UNITS], ch[UNITS];
  float s = 0.f;
#pragma unroll
  for (int u = 0; u < UNITS; ++u) {
    const int idx = tid + u * 256;
    pix[u] = -1; ch[u] = 0;
    v[u][0] = v[u][1] = v[u][2] = v[u][3] = 0.f;
    if (idx < total) {
      const int p = idx / upp, j = idx - p * upp;
      pix[u] = p; ch[u] = j * 4;
      const uint2 r = *(const uint2*)(src + (long)p * ldc + j * 4);
      v[u][0] = h16lo(r.x); v[u][1] = h16hi(r.x);
      v[u][2] = h16lo(r.y); v[u][3] = h16hi(r.y);
      s += (v[u][0] + v[u][1]) + (v[u][2] + v[u][3]);
    }
  }
  const float n = (float)a.HW * (float)cpg;
  const float mean = block_sum4(s, red) / n;
  float q = 0.f;
#pragma unroll
  for (int u = 0; u < UNITS; ++u)
    if (pix[u] >= 0) {
#pragma unroll
      for (int k = 0; k < 4; ++k) { const float d = v[u][k] - mean; q += d * d; }
    }
  const float rstd = rsqrtf(block_sum4(q, red + 4) / n + a.eps);
  if (a.stats_out && tid == 0) { a.stats_out[((long)b * a.G + g) * 2] = mean; a.stats_out[((long)b * a.G + g) * 2 + 1] = rstd; }
  if (a.out8) {                                      // e4m3 of the normalised value under the static scale (GnArgs::out8)
    uint8_t* dst8 = a.out8 + (long)b * a.HW * a.C + cg;
    const float w = rstd * a.q_mul;
#pragma unroll
    for (int u = 0; u < UNITS; ++u)
      if (pix[u] >= 0) {
        float y[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) y[k] = sat_e4m3((v[u][k] - mean) * w);
        *(unsigned*)(dst8 + (long)pix[u] * a.C + ch[u]) = pack4_e4m3(y[0], y[1], y[2], y[3]);
      }
    return;
  }
  bf16_t* dst = a.out + (long)b * a.HW * a.C + cg;
#pragma unroll
  for (int u = 0; u < UNITS; ++u)
    if (pix[u] >= 0) {
      const float4 gm = gb_lds ? *(const float4*)(gam_s + ch[u]) : *(const float4*)(a.gamma + cg + ch[u]);
      const float4 bt = gb_lds ? *(const float4*)(bet_s + ch[u]) : *(const float4*)(a.beta + cg + ch[u]);
      float y[4] = {(v[u][0] - mean) * rstd * gm.x + bt.x, (v[u][1] - mean) * rstd * gm.y + bt.y,
                    (v[u][2] - mean) * rstd * gm.z + bt.z, (v[u][3] - mean) * rstd * gm.w + bt.w};
      if (a.silu) {
#pragma unroll
        for (int k = 0; k < 4; ++k) y[k] = silu_f(y[k]);
      }
      uint2 o; o.x = pack2bf(y[0], y[1]); o.y = pack2bf(y[2], y[3]);
      *(uint2*)(dst + (long)pix[u] * a.C + ch[u]) = o;
    }
}

// ---- mid-size tensors (everything below the 64x64 level): ONE launch, coalesced.  gn_small_kernel above gives a block one
// (image, group) slab: cpg * 2 = 40..160 contiguous bytes per pixel at a stride of the whole channel count, so every 128-byte line is
// fetched by the 2-4 blocks whose groups share it (usually on different XCDs), and gamma / beta are re-read per 8-byte unit.
// Here a block owns GQ ADJACENT groups of one image (160-640 contiguous bytes per pixel), a thread owns a FIXED 4-channel unit
// of that span (gamma / beta / group index live in registers) and walks pixels; the slab stays in registers as packed bf16
// (2 VGPRs per unit), the statistics are reduced in a fixed order through LDS (two-pass variance), one read, one write.
//   threads = PPB pixel lanes x UPPB units per pixel (UPPB = GQ * cpg / 4), thread -> (pp = tid / UPPB, j = tid % UPPB)
//   MAXT: largest block the instantiation is launched with.  More than 16 units per thread (64+ VGPRs of slab plus as many load addresses
//   in flight) do not fit the 128 VGPRs of a 1024-thread block (the 24-unit variant spilled 22 registers): it runs with at
//   most 512 threads (256 VGPRs), gn_select picks the geometry accordingly.
template <int UNITS, int MAXT = 1024>
__global__ __launch_bounds__(MAXT) void gn_mid_kernel(const GnArgs a, const int gq, const int ppb) {
  __shared__ float red[MAXT];
  __shared__ float colsum[2][256];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int cpg = a.C / a.G, upp = cpg >> 2, uppb = gq * upp;
  const int g0 = blockIdx.x * gq, cg0 = g0 * cpg;
  const bool active = tid < ppb * uppb;
  const int pp = tid / uppb, j = tid - pp * uppb;
  const int c = cg0 + j * 4;                                   // this thread's four channels in the concatenated tensor
  const bool first = c < a.C0;
  const bf16_t* src = first ? a.src0 + (long)b * a.HW * a.C0 + c : a.src1 + (long)b * a.HW * a.C1 + (c - a.C0);
  const int ldc = first ? a.C0 : a.C1;
  uint2 v[UNITS];
  float s = 0.f;
#pragma unroll
  for (int u = 0; u < UNITS; ++u) {
    const int p = pp + u * ppb;
    v[u] = uint2{0u, 0u};
    if (active && p < a.HW) v[u] = *(const uint2*)(src + (long)p * ldc);
  }
#pragma unroll
  for (int u = 0; u < UNITS; ++u)      // out-of-range units hold zeros: they add nothing here and are masked in the second pass
    s += (h16lo(v[u].x) + h16hi(v[u].x)) +
         (h16lo(v[u].y) + h16hi(v[u].y));
  const float n = (float)a.HW * (float)cpg;
  const int gi = j / upp;                                       // group of this thread inside the block
  auto group_total = [&](float x, int slot) -> float {
    red[tid] = active ? x : 0.f;
    __syncthreads();
    if (tid < uppb) {
      float t = 0.f;
      for (int q = 0; q < ppb; ++q) t += red[q * uppb + tid];
      colsum[slot][tid] = t;
    }
    __syncthreads();
    float t = 0.f;
    for (int k = 0; k < upp; ++k) t += colsum[slot][gi * upp + k];
    return t;
  };
  const float mean = group_total(s, 0) / n;
  float q = 0.f;
#pragma unroll
  for (int u = 0; u < UNITS; ++u) {
    if (pp + u * ppb < a.HW) {
      const float d0 = h16lo(v[u].x) - mean, d1 = h16hi(v[u].x) - mean;
      const float d2 = h16lo(v[u].y) - mean, d3 = h16hi(v[u].y) - mean;
      q += (d0 * d0 + d1 * d1) + (d2 * d2 + d3 * d3);
    }
  }
  const float rstd = rsqrtf(group_total(q, 1) / n + a.eps);
  if (!active) return;
  if (a.stats_out && pp == 0 && j == gi * upp) {
    a.stats_out[((long)b * a.G + g0 + gi) * 2] = mean; a.stats_out[((long)b * a.G + g0 + gi) * 2 + 1] = rstd;
  }
  const float4 gm = *(const float4*)(a.gamma + c), bt = *(const float4*)(a.beta + c);
  const float w0 = rstd * gm.x, w1 = rstd * gm.y, w2 = rstd * gm.z, w3 = rstd * gm.w;
  bf16_t* dst = a.out + (long)b * a.HW * a.C + c;
#pragma unroll
  for (int u = 0; u < UNITS; ++u) {
    const int p = pp + u * ppb;
    if (p < a.HW) {
      float y[4] = {(h16lo(v[u].x) - mean) * w0 + bt.x, (h16hi(v[u].x) - mean) * w1 + bt.y,
                    (h16lo(v[u].y) - mean) * w2 + bt.z, (h16hi(v[u].y) - mean) * w3 + bt.w};
      if (a.silu) {
#pragma unroll
        for (int k = 0; k < 4; ++k) y[k] = silu_f(y[k]);
      }
      uint2 o; o.x = pack2bf(y[0], y[1]); o.y = pack2bf(y[2], y[3]);
      *(uint2*)(dst + (long)p * a.C) = o;
    }
  }
}

namespace {
// grid (N / 8, B), 256 threads: the image's group statistics from the partials (as gn_apply_kernel), then eight rows of the projection,
// two per wave (a lane takes 8-column chunks lane, lane + 64, ...).
__global__ __launch_bounds__(256) void gn_fold_kernel(const GnFoldArgs a, const float* __restrict__ partial, int chunks) {
  __shared__ float mean_s[64], rstd_s[64];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int cpg = a.C / a.G;
  // the one-thread order, always: a 256-thread block has eight threads per group, but this kernel never summed in eight runs
  const float2 sums = gn_chunk_sums(partial, chunks, a.G, b, false, nullptr);
  if (tid < a.G) {
    const float2 mr = gn_mean_rstd(sums, (float)a.HW * (float)cpg, a.eps);
    mean_s[tid] = mr.x;
    rstd_s[tid] = mr.y;
  }
  __syncthreads();
  const int wave = tid >> 6, lane = tid & 63;
  for (int r = wave; r < 8; r += 4) {
    const int n = blockIdx.x * 8 + r;
    if (n >= a.N) break;
    float acc = 0.f;
    for (int ch = lane; ch < (a.C >> 3); ch += 64) {
      float w[8], o[8];
      unpack8(*(const uint4*)(a.W + (long)n * a.ldw + ch * 8), w);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int c = ch * 8 + k, g = c / cpg;
        o[k] = w[k] * a.gamma[c] * rstd_s[g];
      }
      const uint4 packed = pack8(o);
      float wr[8];
      unpack8(packed, wr);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int c = ch * 8 + k;
        acc += w[k] * a.beta[c] - wr[k] * mean_s[c / cpg];
      }
      *(uint4*)(a.Wimg + ((long)b * a.N + n) * a.C + ch * 8) = packed;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (lane == 0) a.rv[(long)b * a.N + n] = (a.bias ? a.bias[n] : 0.f) + acc;
  }
}
}  // namespace

namespace dfh {

namespace {
// Which kernels a GroupNorm runs as: a pure function of the shape and the probe switches.
enum GnPath { GN_PRODUCER_STATS, GN_ONE_SLAB, GN_GROUP_QUAD, GN_TWO_KERNEL };
struct GnPlan {
  GnPath path;
  int units;                 // the UNITS instantiation of gn_small_kernel / gn_mid_kernel
  int gq, ppb, threads;      // gn_mid_kernel: groups per block, pixel lanes per block, block size
};

GnPlan gn_select(const GnArgs& a, const WalkKnobs& knobs) {
  // the producer's epilogue already summed the tensor (one source, its own group structure): normalise only
  if (a.pre) return {GN_PRODUCER_STATS, 0, 0, 0, 0};
  const int cpg = a.C / a.G, upp = cpg >> 2;
  // small tensors (16x16 / 8x8 levels), one (image, group) slab per block.  DFH_GN_SMALL_MAX, probe knob; > 16 units per thread
  // (32x32 x 640) the two-kernel path is faster since its prologue fix: 25.6 -> 21.3 us
  const long slab = (long)a.HW * upp;
  const bool one_source_per_group = a.C1 == 0 || a.C0 % cpg == 0;
  if ((cpg & 3) == 0 && slab <= 256 * knobs.gn_small_max && one_source_per_group && (long)a.B * a.G >= 64)
    return {GN_ONE_SLAB, slab <= 256 * 8 ? 8 : slab <= 256 * 16 ? 16 : 32, 0, 0, 256};
  // (tests/helpers_norm.py group_quad_geometry restates the rule below for the summation depth of its bounds: change the two together)
  // mid path (16x16 / 8x8 tensors the one-slab kernel cannot take: groups that straddle the two concat sources, e.g. 1280 + 640
  // channels): GQ adjacent groups per block.  Measured against the alternatives (scripts/norm_microbench.py): 24.4 -> 13.4 us
  // on 16x16 x (1280 + 640); where gn_small_kernel is eligible it is faster (its blocks are four waves, the reductions here
  // run across up to sixteen), and at 32x32 the two-kernel path is, so this is the fallback between them.  DFH_GN_MID=0: off.
  if (knobs.gn_mid && !a.out8 && (cpg & 3) == 0 && a.HW <= 256 && a.G % 2 == 0) {
    for (int gq = 4; gq >= 2; gq >>= 1) {
      if (a.G % gq || (long)a.B * (a.G / gq) < 128 || gq * upp > 256) continue;
      const int uppb = gq * upp;
      int threads = 256;
      auto units_at = [&](int t) { return t / uppb < 1 ? 1 << 30 : (a.HW + t / uppb - 1) / (t / uppb); };
      while (threads < 1024 && units_at(threads) > 24) threads *= 2;
      // 1024-thread blocks hold at most 16 units per thread in registers (128 VGPRs); 17..24 units run as 512-thread blocks
      if (threads == 1024 && units_at(1024) > 16) threads = 512;
      const int ppb = threads / uppb;
      if (ppb < 1) continue;
      const int units = (a.HW + ppb - 1) / ppb;
      // more than the widest instantiation holds: refused.  (25..32 never comes out of the rule above -- only the 1024 -> 512 step
      // could give it, and that takes units_at(1024) > 16 with units_at(512) <= 32 -- so this refuses what `units > 32` did.)
      if (units > 24) continue;
      return {GN_GROUP_QUAD, units <= 4 ? 4 : units <= 8 ? 8 : units <= 16 ? 16 : 24, gq, ppb, threads};
    }
  }
  return {GN_TWO_KERNEL, 0, 0, 0, 0};
}
}  // namespace

int groupnorm_launch(GnArgs a, hipStream_t stream) {
  a.C = a.C0 + a.C1;
  DFH_REQUIRE(a.C % 8 == 0 && a.C0 % 8 == 0 && a.C1 % 8 == 0, "channels must be multiples of 8");
  DFH_REQUIRE(a.G > 0 && a.G <= 64 && a.C % a.G == 0, "bad group count");
  // the statistics / apply kernels run one thread per 8 channels in blocks of at most 512 threads (their launch bounds): 4096 channels,
  // 3.2 x the widest tensor of the SD U-Nets (1280 + 1280 concatenated = 2560)
  DFH_REQUIRE(a.C <= 4096, "GroupNorm over more than 4096 channels is not supported");
  DFH_REQUIRE((a.partial != nullptr || a.pre != nullptr) && (a.out != nullptr || a.out8 != nullptr) && a.src0 != nullptr, "null pointer");
  if (a.out8) DFH_REQUIRE(a.C1 == 0 && !a.silu && a.q_mul > 0.f && !a.stats_out, "e4m3 GroupNorm output: one source, no SiLU, a positive scale");
  DFH_REQUIRE(a.C1 == 0 || a.src1 != nullptr, "second source missing");
  if (a.pre) DFH_REQUIRE(a.C1 == 0 && a.pre_chunks > 0 && a.pre_chunks <= (int)GN_MAX_CHUNKS, "producer statistics: one source, 1..64 chunks");
  const WalkKnobs& knobs = WalkKnobs::get();
  const GnPlan plan = gn_select(a, knobs);
  GnTwoKernel tk{};
  if (plan.path == GN_PRODUCER_STATS || plan.path == GN_TWO_KERNEL)
    if (int rc = gn_two_kernel_geometry(a, knobs.gn_sc, knobs.gn_ac, &tk)) return rc;    // DFH_GN_SC / DFH_GN_AC: probe knobs
  ProfScope ps(PC_GNORM, 0.0, (a.out8 ? 3.0 : 4.0) * a.B * (double)a.HW * a.C, stream);   // algorithmic: one read + one write (bf16)
  switch (plan.path) {
    case GN_PRODUCER_STATS:
      a.partial = const_cast<float*>(a.pre); a.chunks = a.pre_chunks;
      census(CK_GN_PRE);
      break;
    case GN_ONE_SLAB: {
      const auto kernel = plan.units == 8 ? gn_small_kernel<8> : plan.units == 16 ? gn_small_kernel<16> : gn_small_kernel<32>;
      census(CK_GN_SMALL);
      hipLaunchKernelGGL(kernel, dim3(a.G, a.B), dim3(plan.threads), 0, stream, a);
      return check_launch("gn_small_kernel");
    }
    case GN_GROUP_QUAD: {
      const auto kernel = plan.units == 4 ? gn_mid_kernel<4> : plan.units == 8 ? gn_mid_kernel<8> : plan.units == 16 ? gn_mid_kernel<16>
                                                                                                  : gn_mid_kernel<24, 512>;   // threads <= 512 there
      census(CK_GN_MID);
      hipLaunchKernelGGL(kernel, dim3(a.G / plan.gq, a.B), dim3(plan.threads), 0, stream, a, plan.gq, plan.ppb);
      return check_launch("gn_mid_kernel");
    }
    case GN_TWO_KERNEL:
      census(CK_GN_STATS);
      hipLaunchKernelGGL(gn_stats_kernel, dim3(a.chunks, a.B), dim3(tk.block), tk.lds, stream, a);
      if (int rc = check_launch("gn_stats_kernel")) return rc;
      break;
  }
  hipLaunchKernelGGL(gn_apply_kernel, dim3(tk.achunks, a.B), dim3(tk.block), 0, stream, a);
  return check_launch("gn_apply_kernel");
}

int groupnorm_fold_launch(GnFoldArgs f, hipStream_t stream) {
  DFH_REQUIRE(f.x && f.gamma && f.beta && f.W && f.Wimg && f.rv && (f.pre || f.partial), "groupnorm fold: null pointer");
  DFH_REQUIRE(f.C % 8 == 0 && f.G > 0 && f.G <= 64 && f.C % f.G == 0 && f.C <= 4096 && f.ldw % 8 == 0 && f.ldw >= f.C && f.N > 0, "groupnorm fold: bad shape");
  const float* partial = f.pre;
  int chunks = f.pre_chunks;
  if (!partial) {
    GnArgs a; std::memset(&a, 0, sizeof(a));
    a.src0 = f.x; a.C0 = a.C = f.C; a.B = f.B; a.HW = f.HW; a.G = f.G; a.partial = f.partial;
    GnTwoKernel tk;
    if (int rc = gn_two_kernel_geometry(a, WalkKnobs::get().gn_sc, WalkKnobs::get().gn_ac, &tk)) return rc;
    ProfScope ps(PC_GNORM, 0.0, 2.0 * a.B * (double)a.HW * a.C, stream);        // one read of the tensor
    census(CK_GN_STATS);
    hipLaunchKernelGGL(gn_stats_kernel, dim3(a.chunks, a.B), dim3(tk.block), tk.lds, stream, a);
    if (int rc = check_launch("gn_stats_kernel")) return rc;
    partial = f.partial; chunks = a.chunks;
  } else {
    DFH_REQUIRE(chunks > 0 && chunks <= (int)GN_MAX_CHUNKS, "producer statistics: 1..64 chunks");
  }
  ProfScope ps(PC_GNORM, 0.0, (double)f.N * f.C * 2.0 * (1.0 + f.B), stream);
  census(CK_GN_FOLDED);
  hipLaunchKernelGGL(gn_fold_kernel, dim3((f.N + 7) / 8, f.B), dim3(256), 0, stream, f, partial, chunks);
  return check_launch("gn_fold_kernel");
}

int layernorm_launch(const bf16_t* x, const float* gamma, const float* beta, bf16_t* y, int M, int C, float eps,
                     hipStream_t stream) {
  DFH_REQUIRE(C % 8 == 0 && C <= 8 * 64 * 4, "LayerNorm width must be a multiple of 8 and <= 2048");
  const dim3 block(256);
  ProfScope ps(PC_LNORM, 0.0, 4.0 * (double)M * C, stream);
  census(CK_LAYERNORM);
  if (C <= 512) hipLaunchKernelGGL((layernorm_kernel<1, 4>), dim3((M + 15) / 16), block, 0, stream, x, gamma, beta, y, M, C, eps);
  else if (C <= 1024) hipLaunchKernelGGL((layernorm_kernel<2, 2>), dim3((M + 7) / 8), block, 0, stream, x, gamma, beta, y, M, C, eps);
  else hipLaunchKernelGGL((layernorm_kernel<4, 1>), dim3((M + 3) / 4), block, 0, stream, x, gamma, beta, y, M, C, eps);
  return check_launch("layernorm_kernel");
}

}  // namespace dfh

// Device steps the normalisation kernels share (norm.hip, norm_bwd.hip, the LayerNorm quantiser of gemm_fp8.hip, the GroupNorm prologue
// of winograd.hip).  Each is stated once because its copies had to stay bit-compatible: the ORDER of every sum below is part of the
// contract (forward and backward agree on the statistics, two builds of the library on every bit).
#pragma once
#include "dfh_common.h"

// 16 bytes of channel octet o at pixel p of image b of the channel concat [src0 | src1] (GnArgs, GnBwdArgs): an octet below C0 / 8
// comes from src0, the rest from src1
template <class Args>
DFH_DEVICE const uint4* gn_src(const Args& a, int b, int p, int o) {
  const int o0 = a.C0 >> 3;
  if (o < o0) return (const uint4*)(a.src0 + ((long)(b * a.HW + p) * a.C0 + o * 8));
  return (const uint4*)(a.src1 + ((long)(b * a.HW + p) * a.C1 + (o - o0) * 8));
}

// eight consecutive floats (32-byte aligned: gamma / beta of a channel octet) as two 16-byte loads
DFH_DEVICE void load8f(const float* p, float* f) {
  const float4 lo = *(const float4*)p, hi = *(const float4*)(p + 4);
  f[0] = lo.x; f[1] = lo.y; f[2] = lo.z; f[3] = lo.w; f[4] = hi.x; f[5] = hi.y; f[6] = hi.z; f[7] = hi.w;
}

// The image's `chunks` partials per group ([b][group][chunk][2], contiguous per group) summed to the group's two totals, which thread
// tid < G receives for group tid (other threads: zeros).  wide: eight threads per group each sum a contiguous run of chunks in
// ascending order, then the eight runs are summed in ascending order (needs 8 * G threads and run_s; contains a barrier, so `wide`
// must be uniform over the block).  Otherwise one thread per group sums every chunk in ascending order (run_s unused).  Summed by one
// thread per group the prologue of gn_apply_kernel was a chain of 8-16 dependent load batches per block and paced the whole kernel
// (37 -> 28 us on 64x64 x 320 with it gone).  The two orders give different bits: a kernel states the one it has always used.
DFH_DEVICE float2 gn_chunk_sums(const float* partial, int chunks, int G, int b, bool wide, float2 (*run_s)[8]) {
  const int tid = threadIdx.x;
  if (wide) {
    if (tid < G * 8) {
      const int g = tid >> 3, sub = tid & 7;
      const int per = (chunks + 7) >> 3, c0 = sub * per, c1 = min(chunks, c0 + per);
      const float2* src = (const float2*)(partial + ((long)b * G + g) * chunks * 2);
      float ss = 0.f, qq = 0.f;
      for (int c = c0; c < c1; ++c) { const float2 v = src[c]; ss += v.x; qq += v.y; }
      run_s[g][sub] = float2{ss, qq};
    }
    __syncthreads();
  }
  float ss = 0.f, qq = 0.f;
  if (tid < G) {
    if (wide) {
#pragma unroll
      for (int sub = 0; sub < 8; ++sub) { ss += run_s[tid][sub].x; qq += run_s[tid][sub].y; }
    } else {
      const float2* src = (const float2*)(partial + ((long)b * G + tid) * chunks * 2);
      for (int c = 0; c < chunks; ++c) { ss += src[c].x; qq += src[c].y; }
    }
  }
  return float2{ss, qq};
}

// (sum, sum of squares) over n elements -> (mean, rstd); the one-pass variance is clamped at zero
DFH_DEVICE float2 gn_mean_rstd(float2 sums, float n, float eps) {
  const float mean = sums.x / n;
  const float var = fmaxf(sums.y / n - mean * mean, 0.f);
  return float2{mean, rsqrtf(var + eps)};
}

// sum of x over a 256-thread block: wave sums through red4[0..3], then (r0 + r1) + (r2 + r3).  Contains a barrier; two sums in one
// kernel use two sets of slots (no barrier in between protects a reuse).
DFH_DEVICE float block_sum4(float x, float* red4) {
  x = wave_sum(x);
  if ((threadIdx.x & 63) == 0) red4[threadIdx.x >> 6] = x;
  __syncthreads();
  return (red4[0] + red4[1]) + (red4[2] + red4[3]);
}

// ---- LayerNorm, one wave per row of C = 8 * C8 values: lane l holds the octets l, l + 64, ... (MAXO of them, past C8: zeros)
// R rows of a wave, every load issued before anything is reduced: with one 640-byte row per wave the chip had ~5 MB in flight, half of
// what 5 TB/s needs at ~2 us of loaded latency
template <int MAXO, int R>
DFH_DEVICE void ln_load_rows(const bf16_t* __restrict__ x, int row0, int M, int C, int lane, uint4 (&raw)[R][MAXO]) {
  const int C8 = C >> 3;
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int i = 0; i < MAXO; ++i) {
      const int o = lane + i * 64;
      raw[r][i] = make_uint4(0u, 0u, 0u, 0u);
      if (o < C8 && row0 + r < M) raw[r][i] = *(const uint4*)(x + (long)(row0 + r) * C + o * 8);
    }
}
// first pass of the exact two-pass statistics: the row's mean, subtracted from v in place (octets past C8 untouched)
template <int MAXO>
DFH_DEVICE void ln_centre(float (&v)[MAXO][8], int lane, int C) {
  const int C8 = C >> 3;
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < MAXO; ++i) {
    if (lane + i * 64 < C8) {
#pragma unroll
      for (int k = 0; k < 8; ++k) s += v[i][k];
    }
  }
  const float mean = wave_sum(s) / (float)C;
#pragma unroll
  for (int i = 0; i < MAXO; ++i) {
    if (lane + i * 64 < C8) {
#pragma unroll
      for (int k = 0; k < 8; ++k) v[i][k] -= mean;
    }
  }
}
// (The second pass, the sum of the centred squares, is each kernel's own: layernorm_kernel rounds every square before it adds it,
// layernorm_fp8_kernel fuses the two -- other bits.)

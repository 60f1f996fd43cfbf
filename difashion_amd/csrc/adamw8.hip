// AdamW with block-wise 8-bit optimizer states (reference: DiFashion/train.py:573-593, bnb.optim.AdamW8bit under --use_8bit_adam).
// The format is the dynamic (tree) 8-bit type of Dettmers et al., "8-bit Optimizers via Block-wise Quantization": a block is 64
// consecutive elements at a flat offset that is a multiple of 64 (training._align's granule), each block has one fp32 absmax per
// moment and each element one uint8 code per moment; x = table[code] * absmax.  Bit-compatibility with bitsandbytes' stored state is
// NOT claimed.  One deliberate deviation (DESIGN.md "8-bit optimizer states"): a second moment v > 0 never takes code 0.
//
// Layout of every kernel here: four consecutive elements per lane (float4 p / g / shadow, one dword of four codes per moment), so a
// block is one 16-lane DPP row and the absmax reductions never leave a row: no LDS round trip, no barrier, no atomics.  The tables
// (4 KB) are staged into LDS once per workgroup, which then strides over the buffer.
#include <map>
#include <mutex>
#include "dfh_common.h"
#include "bwd_elementwise.h"

namespace {

// value[0] / mid[0]: unsigned table (exp_avg_sq), value[1] / mid[1]: signed table (exp_avg).  mid[t][k] is the midpoint of entries k and
// k + 1: the code of a normalised value a is the number of midpoints below it.
struct Q8Tables { float value[2][256]; float mid[2][256]; };

constexpr double q8_entry(int i, int j, int fine) {
  constexpr double P10[7] = {1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1, 1.0};
  return P10[i] * (0.1 + 0.9 * (double)(2 * j + 1) / (double)(1 << (i + 1 + fine)));
}
// both tables in ascending order by construction (level i lies inside (0.1, 1) * 10^(i-6), slots ascend inside a level): evaluated in
// double, rounded once to fp32
constexpr Q8Tables make_q8_tables() {
  Q8Tables t{};
  int k = 0;
  t.value[0][k++] = 0.0f;
  for (int i = 0; i < 7; ++i)
    for (int j = 0; j < (2 << i); ++j) t.value[0][k++] = (float)q8_entry(i, j, 1);
  t.value[0][k++] = 1.0f;
  k = 0;
  for (int i = 6; i >= 0; --i)
    for (int j = (1 << i) - 1; j >= 0; --j) t.value[1][k++] = (float)-q8_entry(i, j, 0);
  t.value[1][k++] = 0.0f;                                  // index 127
  for (int i = 0; i < 7; ++i)
    for (int j = 0; j < (1 << i); ++j) t.value[1][k++] = (float)q8_entry(i, j, 0);
  t.value[1][k++] = 1.0f;                                  // there is no -1
  for (int s = 0; s < 2; ++s) {
    for (int m = 0; m < 255; ++m) t.mid[s][m] = (float)(((double)t.value[s][m] + (double)t.value[s][m + 1]) * 0.5);
    t.mid[s][255] = 2.0f;                                  // never read by the search (index <= 254)
  }
  return t;
}
constexpr Q8Tables Q8_HOST = make_q8_tables();
__constant__ Q8Tables q8_dev = Q8_HOST;

constexpr int Q8_THREADS = 256;
constexpr int Q8_MAX_BLOCKS = 256 * 8;                     // quantise / dequantise: 8 workgroups of 4 waves per CU; the grid strides over the rest

struct Q8Lds { float value[2][256]; float mid[2][256]; };
DFH_DEVICE void q8_stage(Q8Lds& lds) {
  const float* src = (const float*)&q8_dev;
  float* dst = (float*)&lds;
#pragma unroll
  for (int k = 0; k < 4; ++k) dst[k * Q8_THREADS + threadIdx.x] = src[k * Q8_THREADS + threadIdx.x];
  __syncthreads();
}

// max over the 16 lanes of a DPP row, left in every lane: xor 1, xor 2 (quad_perm), row_half_mirror, row_mirror
DFH_DEVICE unsigned row_umax(unsigned u) {
  u = max(u, (unsigned)__builtin_amdgcn_update_dpp(0, (int)u, 0xB1, 0xF, 0xF, false));
  u = max(u, (unsigned)__builtin_amdgcn_update_dpp(0, (int)u, 0x4E, 0xF, 0xF, false));
  u = max(u, (unsigned)__builtin_amdgcn_update_dpp(0, (int)u, 0x141, 0xF, 0xF, false));
  u = max(u, (unsigned)__builtin_amdgcn_update_dpp(0, (int)u, 0x140, 0xF, 0xF, false));
  return u;
}
// absmax of a block = max |x| over the row, exactly.  Compared as unsigned integers: for |x| that is the float order, and a NaN
// (above +Inf as an integer) or an Inf wins, so a block with a non-finite value stores a non-finite absmax (fmaxf would drop the NaN)
DFH_DEVICE float q8_block_absmax(const float x[4]) {
  unsigned u = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) u = max(u, __float_as_uint(x[k]) & 0x7fffffffu);
  return __uint_as_float(row_umax(u));
}
// The normalisation a = x / absmax without a division per element: one IEEE reciprocal per lane and moment, then a product and one
// residual correction, a0 = x r, a = a0 + (x - a0 d) r with both steps fused -- within (1 + 4 * 2^-24) of one rounding of the exact
// quotient.  Block and elements are first scaled by an exact power of two when absmax is so small or so large that 1 / absmax would
// leave the normal range (a block of subnormals, values near FLT_MAX).  An all-zero block divides by 1, not by 0.
struct Q8Norm { float sc, d, r; };
DFH_DEVICE Q8Norm q8_norm(float absmax) {
  Q8Norm q;
  q.sc = absmax < 0x1p-64f ? 0x1p64f : (absmax > 0x1p64f ? 0x1p-64f : 1.0f);
  q.d = absmax == 0.f ? 1.f : absmax * q.sc;
  q.r = 1.0f / q.d;
  return q;
}
// code of x: the number of midpoints below a (a branch-free binary search of the LDS table).  The running index is kept in bytes, so a
// step is one LDS read at an immediate offset, one compare, one select and one or.
template <int SIGNED>
DFH_DEVICE unsigned q8_code(float x, const Q8Norm& q, const float* mid) {
  const float xs = x * q.sc, a0 = xs * q.r;
  const float a = fmaf(fmaf(-a0, q.d, xs), q.r, a0);
  unsigned c4 = 0;
#pragma unroll
  for (int s = 128; s > 0; s >>= 1) c4 |= (a > *(const float*)((const char*)mid + c4 + 4 * (s - 1))) ? 4u * s : 0u;
  if (!SIGNED && x > 0.f && c4 == 0) c4 = 4;               // the floor: a positive second moment never rounds to 0
  return c4 >> 2;
}
template <int SIGNED>
DFH_DEVICE unsigned q8_codes4(const float x[4], float absmax, const float* mid) {
  const Q8Norm q = q8_norm(absmax);
  return q8_code<SIGNED>(x[0], q, mid) | (q8_code<SIGNED>(x[1], q, mid) << 8) | (q8_code<SIGNED>(x[2], q, mid) << 16) |
         (q8_code<SIGNED>(x[3], q, mid) << 24);
}
DFH_DEVICE void q8_decode4(unsigned codes, float absmax, const float* value, float x[4]) {
#pragma unroll
  for (int k = 0; k < 4; ++k) x[k] = value[(codes >> (8 * k)) & 255u] * absmax;
}

// fp32 -> (codes, absmax) of one moment type; i counts quads of elements, n4 is a multiple of 16 (whole rows)
template <int SIGNED>
__global__ __launch_bounds__(Q8_THREADS) void q8_quantize_kernel(const float* __restrict__ x, unsigned* __restrict__ codes,
                                                                  float* __restrict__ absmax, long n4) {
  __shared__ Q8Lds lds;
  q8_stage(lds);
  const long stride = (long)gridDim.x * Q8_THREADS;
  for (long i = (long)blockIdx.x * Q8_THREADS + threadIdx.x; i < n4; i += stride) {
    const float4 v = ((const float4*)x)[i];
    const float f[4] = {v.x, v.y, v.z, v.w};
    const float am = q8_block_absmax(f);
    codes[i] = q8_codes4<SIGNED>(f, am, lds.mid[SIGNED]);
    if ((i & 15) == 0) absmax[i >> 4] = am;
  }
}
template <int SIGNED>
__global__ __launch_bounds__(Q8_THREADS) void q8_dequantize_kernel(const unsigned* __restrict__ codes, const float* __restrict__ absmax,
                                                                    float* __restrict__ x, long n4) {
  __shared__ Q8Lds lds;
  q8_stage(lds);
  const long stride = (long)gridDim.x * Q8_THREADS;
  for (long i = (long)blockIdx.x * Q8_THREADS + threadIdx.x; i < n4; i += stride) {
    float f[4];
    q8_decode4(codes[i], absmax[i >> 4], lds.value[SIGNED], f);
    ((float4*)x)[i] = float4{f[0], f[1], f[2], f[3]};
  }
}

// adamw_kernel (bwd_elementwise.hip) on 8-bit moments: dequantise, the same fp32 update (the parameter moves by the UNQUANTISED new
// moments), the block's two new absmax, quantise, store.  One pass, 24.25 B per element with the EMA shadow, 16.25 B without.
__global__ __launch_bounds__(Q8_THREADS) void adamw8_kernel(float* __restrict__ p, const float* __restrict__ g, unsigned* __restrict__ m8,
                                                            float* __restrict__ m_absmax, unsigned* __restrict__ v8,
                                                            float* __restrict__ v_absmax, long n4, float lr, float beta1, float beta2,
                                                            float eps, float wd, float bc1, float bc2, const float* __restrict__ sumsq,
                                                            float max_norm, float* __restrict__ shadow, float ema_omd) {
  __shared__ Q8Lds lds;
  q8_stage(lds);
  float clip = 1.0f;
  if (sumsq) { const float nrm = sqrtf(*sumsq); clip = fminf(1.0f, max_norm / (nrm + 1e-6f)); }
  // uniform factors, once: sqrt(v) / sqrt(bc2) is taken as sqrt(v) * (1 / sqrt(bc2))
  const float decay = 1.0f - lr * wd, omb1 = 1.0f - beta1, omb2 = 1.0f - beta2, rsq_bc2 = 1.0f / sqrtf(bc2), lr_bc1 = lr / bc1;
  const long stride = (long)gridDim.x * Q8_THREADS;
  for (long i = (long)blockIdx.x * Q8_THREADS + threadIdx.x; i < n4; i += stride) {
    const float4 p4 = ((const float4*)p)[i], g4 = ((const float4*)g)[i];
    float4 s4 = float4{0.f, 0.f, 0.f, 0.f};
    if (shadow) s4 = ((const float4*)shadow)[i];      // issued with the other loads: behind the update it would cost a second round trip
    float pi[4] = {p4.x, p4.y, p4.z, p4.w};
    const float gi[4] = {g4.x * clip, g4.y * clip, g4.z * clip, g4.w * clip};
    float m[4], v[4];
    q8_decode4(m8[i], m_absmax[i >> 4], lds.value[1], m);
    q8_decode4(v8[i], v_absmax[i >> 4], lds.value[0], v);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      pi[k] = pi[k] * decay;
      m[k] = beta1 * m[k] + omb1 * gi[k];
      v[k] = beta2 * v[k] + omb2 * gi[k] * gi[k];
      const float denom = sqrtf(v[k]) * rsq_bc2 + eps;
      pi[k] -= lr_bc1 * (m[k] / denom);
    }
    ((float4*)p)[i] = float4{pi[0], pi[1], pi[2], pi[3]};
    if (shadow) {                  // diffusers EMAModel.step folded into the same pass: shadow -= (1 - decay) * (shadow - p)
      ((float4*)shadow)[i] = float4{s4.x - ema_omd * (s4.x - pi[0]), s4.y - ema_omd * (s4.y - pi[1]), s4.z - ema_omd * (s4.z - pi[2]),
                                    s4.w - ema_omd * (s4.w - pi[3])};
    }
    const float mam = q8_block_absmax(m), vam = q8_block_absmax(v);
    m8[i] = q8_codes4<1>(m, mam, lds.mid[1]);
    v8[i] = q8_codes4<0>(v, vam, lds.mid[0]);
    if ((i & 15) == 0) { m_absmax[i >> 4] = mam; v_absmax[i >> 4] = vam; }
  }
}

// The update kernel's grid is exactly what is resident at once (CUs x workgroups per CU at its register count): with more workgroups
// than that the surplus would run as a tail round on a fraction of the CUs.  Asked of the runtime once per device.
int adamw8_resident_blocks() {
  static std::mutex mu;
  static std::map<int, int> table;
  std::lock_guard<std::mutex> lock(mu);
  int dev = 0, cus = 0, per_cu = 0;
  if (hipGetDevice(&dev) != hipSuccess) return Q8_MAX_BLOCKS;
  auto it = table.find(dev);
  if (it != table.end()) return it->second;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
      hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, adamw8_kernel, Q8_THREADS, 0) != hipSuccess || cus <= 0 || per_cu <= 0)
    return Q8_MAX_BLOCKS;
  return table[dev] = cus * per_cu;
}
inline dim3 q8_grid(long n4) { return dim3((unsigned)std::min<long>((n4 + Q8_THREADS - 1) / Q8_THREADS, Q8_MAX_BLOCKS)); }
inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

namespace dfh {
void q8_table_host(int is_signed, float* out256) {
  for (int k = 0; k < 256; ++k) out256[k] = Q8_HOST.value[is_signed ? 1 : 0][k];
}
int q8_quantize_launch(const float* x, unsigned char* codes, float* absmax, long n, int is_signed, hipStream_t s) {
  DFH_REQUIRE(n >= 0 && n % 64 == 0, "q8_quantize: the element count must be a multiple of the 64-element block");
  DFH_REQUIRE(aligned(x, 16) && aligned(codes, 4) && aligned(absmax, 4), "q8_quantize: x must be 16-byte aligned, codes and absmax 4-byte aligned");
  if (n == 0) return 0;
  ProfScope ps(PC_OPTIM, 0.0, (5.0 + 4.0 / 64) * n, s);
  if (is_signed) hipLaunchKernelGGL(q8_quantize_kernel<1>, q8_grid(n / 4), dim3(Q8_THREADS), 0, s, x, (unsigned*)codes, absmax, n / 4);
  else hipLaunchKernelGGL(q8_quantize_kernel<0>, q8_grid(n / 4), dim3(Q8_THREADS), 0, s, x, (unsigned*)codes, absmax, n / 4);
  return check_launch("q8_quantize_kernel");
}
int q8_dequantize_launch(const unsigned char* codes, const float* absmax, float* x, long n, int is_signed, hipStream_t s) {
  DFH_REQUIRE(n >= 0 && n % 64 == 0, "q8_dequantize: the element count must be a multiple of the 64-element block");
  DFH_REQUIRE(aligned(x, 16) && aligned(codes, 4) && aligned(absmax, 4), "q8_dequantize: x must be 16-byte aligned, codes and absmax 4-byte aligned");
  if (n == 0) return 0;
  ProfScope ps(PC_OPTIM, 0.0, (5.0 + 4.0 / 64) * n, s);
  if (is_signed) hipLaunchKernelGGL(q8_dequantize_kernel<1>, q8_grid(n / 4), dim3(Q8_THREADS), 0, s, (const unsigned*)codes, absmax, x, n / 4);
  else hipLaunchKernelGGL(q8_dequantize_kernel<0>, q8_grid(n / 4), dim3(Q8_THREADS), 0, s, (const unsigned*)codes, absmax, x, n / 4);
  return check_launch("q8_dequantize_kernel");
}
int adamw8_launch(float* p, const float* g, unsigned char* m8, float* m_absmax, unsigned char* v8, float* v_absmax, float* shadow, long n,
                  float lr, float beta1, float beta2, float eps, float wd, int step, const float* sumsq, float max_norm, float ema_decay,
                  hipStream_t s) {
  DFH_REQUIRE(n >= 0 && n % 64 == 0, "adamw8: the element count must be a multiple of the 64-element block");
  DFH_REQUIRE(aligned(p, 16) && aligned(g, 16) && aligned(shadow, 16), "adamw8: p, g and shadow must be 16-byte aligned");
  DFH_REQUIRE(aligned(m8, 4) && aligned(v8, 4) && aligned(m_absmax, 4) && aligned(v_absmax, 4), "adamw8: codes and absmax must be 4-byte aligned");
  if (n == 0) return 0;
  const float bc1 = 1.0f - powf(beta1, (float)step), bc2 = 1.0f - powf(beta2, (float)step);
  ProfScope ps(PC_OPTIM, 0.0, (shadow ? 24.25 : 16.25) * n, s);      // p r+w, g r, two codes r+w, two absmax r+w per 64 (+ shadow r+w)
  const dim3 grid((unsigned)std::min<long>((n / 4 + Q8_THREADS - 1) / Q8_THREADS, adamw8_resident_blocks()));
  hipLaunchKernelGGL(adamw8_kernel, grid, dim3(Q8_THREADS), 0, s, p, g, (unsigned*)m8, m_absmax, (unsigned*)v8, v_absmax, n / 4, lr,
                     beta1, beta2, eps, wd, bc1, bc2, sumsq, max_norm, shadow, 1.0f - ema_decay);
  return check_launch("adamw8_kernel");
}
}  // namespace dfh

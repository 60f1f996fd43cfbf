// HBM-bound elementwise / glue kernels of the DiFashion denoising path on gfx950.
// Each kernel cites the reference lines it replaces (DiFashion/models/difashion.py = "df.py").
// fp32 glue arithmetic is written with explicit __fmul_rn/__fadd_rn/__fsub_rn so the compiler
// cannot contract it into FMAs: results are bit-identical to the reference's separate torch ops.
#include "dfh_common.h"
#include "elementwise.h"

namespace {

constexpr int EW_BLOCK = 256;
DFH_DEVICE long gtid() { return (long)blockIdx.x * blockDim.x + threadIdx.x; }
inline dim3 ew_grid(long n) { return dim3((unsigned)((n + EW_BLOCK - 1) / EW_BLOCK)); }

// diffusers get_timestep_embedding(flip_sin_to_cos=True, freq_shift=0): [cos | sin], SURVEY A.2
__global__ void timestep_embed_kernel(const float* __restrict__ t, bf16_t* __restrict__ out, int B, int dim) {
  const long i = gtid();
  const int half = dim >> 1;
  if (i >= (long)B * half) return;
  const int b = (int)(i / half), k = (int)(i - (long)b * half);
  const float freq = expf(-9.210340371976184f * (float)k / (float)half);   // ln(10000)
  const float arg = t[b] * freq;
  out[(long)b * dim + k] = f2bf(cosf(arg));
  out[(long)b * dim + half + k] = f2bf(sinf(arg));
}

// NCHW (fp32 or bf16) -> NHWC bf16; one thread per (b, pixel, 8-channel octet)
template <typename T>
__global__ void nchw_to_nhwc_kernel(const T* __restrict__ x, bf16_t* __restrict__ out, int B, int C, int HW) {
  const long i = gtid();
  const int C8 = (C + 7) >> 3, Cp = C8 * 8;      // output channels padded to a multiple of 8 with zeros
  if (i >= (long)B * HW * C8) return;
  const int o = (int)(i % C8);
  const long bp = i / C8;
  const int p = (int)(bp % HW), b = (int)(bp / HW);
  float f[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int c = o * 8 + k;
    f[k] = 0.f;
    if (c < C) {
      const T v = x[((long)b * C + c) * HW + p];
      if constexpr (sizeof(T) == 4) f[k] = v; else f[k] = bf2f(v);
    }
  }
  *(uint4*)(out + (bp * Cp + o * 8)) = pack8(f);
}

__global__ void cast_f32_to_bf16_kernel(const float* __restrict__ x, bf16_t* __restrict__ y, long n8) {
  const long i = gtid();
  if (i >= n8) return;
  const float4 a = *(const float4*)(x + i * 8), b = *(const float4*)(x + i * 8 + 4);
  const float f[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
  *(uint4*)(y + i * 8) = pack8(f);
}

// df.py:160-170 (training, w = 1/(olen-1)) and df.py:475-489 (sampling, w = 1): for output row j,
//   acc = 0; for k in slots: acc = acc + w_k * src_k        (same order as the reference's sum([...]))
// table[j][k] >= 0 : row of ``gen`` (current generated / noisy latents)
// table[j][k] <  0 : row -(v+1) of ``given`` (clean latents of the given items); own slot -> w = 0.
__global__ void mutual_reduce_kernel(const float* __restrict__ gen, const float* __restrict__ given,
                                     const int* __restrict__ table, const float* __restrict__ wtab,
                                     bf16_t* __restrict__ out, float* __restrict__ out_f32, int rows, int olen, int L) {
  const long i = gtid();
  if (i >= (long)rows * L) return;
  const int j = (int)(i / L), e = (int)(i - (long)j * L);
  float acc = 0.f;
  for (int k = 0; k < olen; ++k) {
    const int v = table[j * olen + k];
    const float x = v >= 0 ? gen[(long)v * L + e] : given[(long)(-(v + 1)) * L + e];
    acc = __fadd_rn(acc, __fmul_rn(wtab[j * olen + k], x));
  }
  out[i] = f2bf(acc);
  if (out_f32) out_f32[i] = acc;
}

// df.py:215-216 / :514-515 with the CFG replica stacking of :388-406,:458-469,:494-512 folded in:
//   x[r*F+j][0:4] = (1-eta)*lat[j] + eta*(mutual_real[r] ? mutual[j] : null)
//   x[r*F+j][4:8] = hist_real[r] ? hist[j] : null
// training (R = 1) passes per-row masks instead of per-replica flags.
__global__ void assemble_input_kernel(const float* __restrict__ lat, const float* __restrict__ mutual,
                                      const float* __restrict__ hist, const float* __restrict__ null_latent,
                                      const unsigned char* __restrict__ mutual_real, const unsigned char* __restrict__ hist_real,
                                      float* __restrict__ x, int R, int F, int CL, float one_minus_eta, float eta, int per_row_flags) {
  const long i = gtid();
  const long n = (long)R * F * CL;
  if (i >= n) return;
  const int e = (int)(i % CL);
  const long row = i / CL;
  const int j = (int)(row % F), r = (int)(row / F);
  const int fl = per_row_flags ? (int)row : r;
  const float m = mutual_real[fl] ? mutual[(long)j * CL + e] : null_latent[e];
  const float h = hist_real[fl] ? hist[(long)j * CL + e] : null_latent[e];
  float* dst = x + row * 2 * CL;
  dst[e] = __fadd_rn(__fmul_rn(one_minus_eta, lat[(long)j * CL + e]), __fmul_rn(eta, m));
  dst[CL + e] = h;
}

// df.py:525-566 (guidance combination, evaluated left-to-right like the reference expression)
DFH_DEVICE float cfg_combine(int mode, const float* __restrict__ eps, long stride, long i, float sc, float sh, float sm) {
  const float e0 = eps[i];
  if (mode == CFG_NONE) return e0;
  const float e1 = eps[i + stride];
  if (mode == CFG_FULL) {
    const float cm = e1, c = eps[i + 2 * stride], u = eps[i + 3 * stride];
    float v = __fadd_rn(u, __fmul_rn(sh, __fsub_rn(e0, cm)));
    v = __fadd_rn(v, __fmul_rn(sm, __fsub_rn(cm, c)));
    return __fadd_rn(v, __fmul_rn(sc, __fsub_rn(c, u)));
  }
  if (mode == CFG_CATE_HIST || mode == CFG_CATE_MUTUAL) {
    const float c = e1, u = eps[i + 2 * stride];
    const float s1 = mode == CFG_CATE_HIST ? sh : sm;
    float v = __fadd_rn(u, __fmul_rn(s1, __fsub_rn(e0, c)));
    return __fadd_rn(v, __fmul_rn(sc, __fsub_rn(c, u)));
  }
  const float u = e1;
  const float s1 = mode == CFG_CATE ? sc : (mode == CFG_MUTUAL ? sm : sh);
  return __fadd_rn(u, __fmul_rn(s1, __fsub_rn(e0, u)));
}

// df.py:525-569 fused: guidance combine + scheduler.step.  kind 0 = DDIM (eta = 0 part; the
// stochastic term, if any, is added from ``noise``), kind 1 = "linear" x' = ca*x - cb*eps (PNDM
// transfer formula with the multistep-blended epsilon supplied in eps_blend).
__global__ void cfg_step_kernel(const float* __restrict__ eps_all, float* __restrict__ lat, float* __restrict__ eps_out,
                                const float* __restrict__ noise, long n, int mode, float sc, float sh, float sm,
                                StepCoef k) {
  const long i = gtid();
  if (i >= n) return;
  const float eps = cfg_combine(mode, eps_all, n, i, sc, sh, sm);
  if (eps_out) eps_out[i] = eps;
  if (k.kind == STEP_NONE) return;
  const float x = lat[i];
  float prev;
  if (k.kind == STEP_DDIM) {
    float x0, pe;
    if (k.vpred) {
      x0 = __fsub_rn(__fmul_rn(k.sqrt_a_t, x), __fmul_rn(k.sqrt_b_t, eps));
      pe = __fadd_rn(__fmul_rn(k.sqrt_a_t, eps), __fmul_rn(k.sqrt_b_t, x));
    } else {
      x0 = __fdiv_rn(__fsub_rn(x, __fmul_rn(k.sqrt_b_t, eps)), k.sqrt_a_t);
      pe = eps;
    }
    prev = __fadd_rn(__fmul_rn(k.sqrt_a_prev, x0), __fmul_rn(k.dir_coef, pe));
    if (noise) prev = __fadd_rn(prev, __fmul_rn(k.std_dev, noise[i]));
  } else {
    prev = __fsub_rn(__fmul_rn(k.sqrt_a_t, x), __fmul_rn(k.sqrt_b_t, eps));
  }
  lat[i] = prev;
}

// V consecutive floats at p[i]: one 16-byte access (V = 4) or the scalar form (V = 1)
template <int V>
DFH_DEVICE void ew_load(const float* p, long i, float (&v)[V]) {
  if constexpr (V == 4) {
    const float4 t = *(const float4*)(p + i);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    v[0] = p[i];
  }
}
template <int V>
DFH_DEVICE void ew_store(float* p, long i, const float (&v)[V]) {
  if constexpr (V == 4) *(float4*)(p + i) = make_float4(v[0], v[1], v[2], v[3]);
  else p[i] = v[0];
}

DFH_DEVICE int cfg_branches(int mode) {
  return mode == CFG_NONE ? 1 : (mode == CFG_FULL ? 4 : ((mode == CFG_CATE_HIST || mode == CFG_CATE_MUTUAL) ? 3 : 2));
}

// df.py:525-569 for the multistep schedulers (PNDM's PLMS branch, DPM-Solver++ 2M) in one launch: guidance combine, conversion of
// the combined output (none | x0 from eps | x0 from v), the update over the history h1..h3 (newest first) and the taps.  x_src may
// be lat itself: every load of an element comes before its stores, and an element belongs to one thread.
//   PLMS: b = w0*q; b = b + w_j*h_j (j = 1..terms-1); x' = cx*x - ce*b
//   DPM1: x' = cx*x - cd0*q            DPM2: D1 = cr*(q - h1); x' = (cx*x - cd0*q) - cd1*D1
template <int V>
__global__ void cfg_multistep_kernel(MultistepArgs a) {
  const long i = gtid() * V;
  if (i >= a.n) return;
  const MultistepCoef& k = a.k;
  const int R = cfg_branches(a.mode);
  float o[4 * V];                       // [branch][lane]: cfg_combine reads it with stride V
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float t[V] = {};
    if (r < R) ew_load<V>(a.out_all + (long)r * a.n, i, t);
#pragma unroll
    for (int l = 0; l < V; ++l) o[r * V + l] = t[l];
  }
  const bool plms = k.kind == MS_PLMS;
  const bool need1 = k.kind == MS_DPM2 || (plms && k.terms >= 2), need2 = plms && k.terms >= 3, need3 = plms && k.terms >= 4;
  float x[V], h1[V] = {}, h2[V] = {}, h3[V] = {};
  ew_load<V>(a.x_src, i, x);
  if (need1) ew_load<V>(a.h1, i, h1);
  if (need2) ew_load<V>(a.h2, i, h2);
  if (need3) ew_load<V>(a.h3, i, h3);
  float m[V], q[V], y[V];
#pragma unroll
  for (int l = 0; l < V; ++l) {
    m[l] = cfg_combine(a.mode, o, V, l, a.sc, a.sh, a.sm);
    if (k.conv == MS_CONV_X0_EPS) q[l] = __fdiv_rn(__fsub_rn(x[l], __fmul_rn(k.c1, m[l])), k.c0);
    else if (k.conv == MS_CONV_X0_V) q[l] = __fsub_rn(__fmul_rn(k.c0, x[l]), __fmul_rn(k.c1, m[l]));
    else q[l] = m[l];
    if (plms) {
      float b = __fmul_rn(k.w[0], q[l]);
      if (need1) b = __fadd_rn(b, __fmul_rn(k.w[1], h1[l]));
      if (need2) b = __fadd_rn(b, __fmul_rn(k.w[2], h2[l]));
      if (need3) b = __fadd_rn(b, __fmul_rn(k.w[3], h3[l]));
      y[l] = __fsub_rn(__fmul_rn(k.cx, x[l]), __fmul_rn(k.ce, b));
    } else {
      y[l] = __fsub_rn(__fmul_rn(k.cx, x[l]), __fmul_rn(k.cd0, q[l]));
      if (k.kind == MS_DPM2) y[l] = __fsub_rn(y[l], __fmul_rn(k.cd1, __fmul_rn(k.cr, __fsub_rn(q[l], h1[l]))));
    }
  }
  if (a.m_out) ew_store<V>(a.m_out, i, m);
  if (a.x_save) ew_store<V>(a.x_save, i, x);
  if (a.q_out) ew_store<V>(a.q_out, i, q);
  ew_store<V>(a.lat, i, y);
}

// scheduler.add_noise / get_velocity (df.py:158,:244): per-row coefficients from device tables
__global__ void noise_mix_kernel(const float* __restrict__ x0, const float* __restrict__ noise,
                                 const long* __restrict__ t, const float* __restrict__ sqrt_a, const float* __restrict__ sqrt_1ma,
                                 float* __restrict__ noisy, float* __restrict__ velocity, int rows, int L) {
  const long i = gtid();
  if (i >= (long)rows * L) return;
  const int r = (int)(i / L);
  const float a = sqrt_a[t[r]], s = sqrt_1ma[t[r]];
  if (noisy) noisy[i] = __fadd_rn(__fmul_rn(a, x0[i]), __fmul_rn(s, noise[i]));
  if (velocity) velocity[i] = __fsub_rn(__fmul_rn(a, noise[i]), __fmul_rn(s, x0[i]));
}

// df.py:255-265: per-row mean squared error (fp32), deterministic: one workgroup per row
__global__ void mse_rows_kernel(const float* __restrict__ pred, const float* __restrict__ target, float* __restrict__ out, int L) {
  __shared__ float red[4];
  const int r = blockIdx.x;
  float s = 0.f;
  for (int e = threadIdx.x; e < L; e += blockDim.x) {
    const float d = pred[(long)r * L + e] - target[(long)r * L + e];
    s += d * d;
  }
  s = wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[r] = (red[0] + red[1] + red[2] + red[3]) / (float)L;
}

// ------------------------------------------------------------------ weight packing (fp32 master -> kernel layouts)
// conv3x3 OIHW fp32 -> bf16 [o][col_off + (ky*3+kx)*Cin + c]
__global__ void pack_conv3x3_kernel(const float* __restrict__ w, bf16_t* __restrict__ out, int Cout, int Cin, int ldw, int col_off, int cin_pad) {
  const long i = gtid();
  if (i >= (long)Cout * Cin * 9) return;
  const int t = (int)(i % 9);
  const long oc = i / 9;
  const int c = (int)(oc % Cin), o = (int)(oc / Cin);
  out[(long)o * ldw + col_off + t * cin_pad + c] = f2bf(w[i]);   // columns c >= Cin of a padded tap stay zero
}

// [N][K] fp32 -> bf16 [row_off + perm(n)][col_off + k]; geglu: value/gate halves interleaved in 16-row blocks
DFH_DEVICE int geglu_row(int n, int N) {
  const int half = N >> 1;
  const int j = n < half ? n : n - half;
  return (j >> 4) * 32 + (n < half ? 0 : 16) + (j & 15);
}
__global__ void pack_matrix_kernel(const float* __restrict__ w, bf16_t* __restrict__ out, int N, int K, int ldw,
                                   int row_off, int col_off, int geglu) {
  const long i = gtid();
  if (i >= (long)N * K) return;
  const int n = (int)(i / K), k = (int)(i - (long)n * K);
  const int r = geglu ? geglu_row(n, N) : n;
  out[(long)(row_off + r) * ldw + col_off + k] = f2bf(w[i]);
}
__global__ void pack_vector_kernel(const float* __restrict__ v, float* __restrict__ out, int N, int off, int geglu, int accumulate) {
  const long i = gtid();
  if (i >= N) return;
  const int r = geglu ? geglu_row((int)i, N) : (int)i;
  out[off + r] = accumulate ? out[off + r] + v[i] : v[i];
}

}  // namespace

namespace dfh {

int timestep_embed_launch(const float* t, bf16_t* out, int B, int dim, hipStream_t s) {
  DFH_REQUIRE(dim % 2 == 0, "embedding dim must be even");
  hipLaunchKernelGGL(timestep_embed_kernel, ew_grid((long)B * dim / 2), dim3(EW_BLOCK), 0, s, t, out, B, dim);
  return check_launch("timestep_embed_kernel");
}

int nchw_to_nhwc_launch(const void* x, int is_bf16, bf16_t* out, int B, int C, int HW, hipStream_t s) {
  const long n = (long)B * HW * ((C + 7) / 8);
  if (is_bf16) hipLaunchKernelGGL(nchw_to_nhwc_kernel<bf16_t>, ew_grid(n), dim3(EW_BLOCK), 0, s, (const bf16_t*)x, out, B, C, HW);
  else hipLaunchKernelGGL(nchw_to_nhwc_kernel<float>, ew_grid(n), dim3(EW_BLOCK), 0, s, (const float*)x, out, B, C, HW);
  return check_launch("nchw_to_nhwc_kernel");
}

int cast_f32_to_bf16_launch(const float* x, bf16_t* y, long n, hipStream_t s) {
  DFH_REQUIRE(n % 8 == 0, "length must be a multiple of 8");
  hipLaunchKernelGGL(cast_f32_to_bf16_kernel, ew_grid(n / 8), dim3(EW_BLOCK), 0, s, x, y, n / 8);
  return check_launch("cast_f32_to_bf16_kernel");
}

int mutual_reduce_launch(const float* gen, const float* given, const int* table, const float* wtab, bf16_t* out,
                         float* out_f32, int rows, int olen, int L, hipStream_t s) {
  hipLaunchKernelGGL(mutual_reduce_kernel, ew_grid((long)rows * L), dim3(EW_BLOCK), 0, s, gen, given, table, wtab, out,
                     out_f32, rows, olen, L);
  return check_launch("mutual_reduce_kernel");
}

int assemble_input_launch(const float* lat, const float* mutual, const float* hist, const float* null_latent,
                          const unsigned char* mutual_real, const unsigned char* hist_real, float* x, int R, int F, int CL,
                          float one_minus_eta, float eta, int per_row_flags, hipStream_t s) {
  hipLaunchKernelGGL(assemble_input_kernel, ew_grid((long)R * F * CL), dim3(EW_BLOCK), 0, s, lat, mutual, hist, null_latent,
                     mutual_real, hist_real, x, R, F, CL, one_minus_eta, eta, per_row_flags);
  return check_launch("assemble_input_kernel");
}

int cfg_step_launch(const float* eps_all, float* lat, float* eps_out, const float* noise, long n, int mode, float sc,
                    float sh, float sm, StepCoef k, hipStream_t s) {
  DFH_REQUIRE(mode >= CFG_NONE && mode <= CFG_MUTUAL, "bad guidance mode");
  hipLaunchKernelGGL(cfg_step_kernel, ew_grid(n), dim3(EW_BLOCK), 0, s, eps_all, lat, eps_out, noise, n, mode, sc, sh, sm, k);
  return check_launch("cfg_step_kernel");
}

int cfg_multistep_launch(const MultistepArgs& a, hipStream_t s) {
  const void* ptrs[] = {a.out_all, a.x_src, a.lat, a.m_out, a.q_out, a.x_save, a.h1, a.h2, a.h3};
  bool vec = a.n % 4 == 0;              // 16-byte accesses: whole groups of four, every buffer that is given 16-byte aligned
  for (const void* p : ptrs) vec = vec && ((uintptr_t)p & 15) == 0;
  if (vec) hipLaunchKernelGGL(cfg_multistep_kernel<4>, ew_grid(a.n / 4), dim3(EW_BLOCK), 0, s, a);
  else hipLaunchKernelGGL(cfg_multistep_kernel<1>, ew_grid(a.n), dim3(EW_BLOCK), 0, s, a);
  return check_launch("cfg_multistep_kernel");
}

int noise_mix_launch(const float* x0, const float* noise, const long* t, const float* sqrt_a, const float* sqrt_1ma,
                     float* noisy, float* velocity, int rows, int L, hipStream_t s) {
  hipLaunchKernelGGL(noise_mix_kernel, ew_grid((long)rows * L), dim3(EW_BLOCK), 0, s, x0, noise, t, sqrt_a, sqrt_1ma, noisy,
                     velocity, rows, L);
  return check_launch("noise_mix_kernel");
}

int mse_rows_launch(const float* pred, const float* target, float* out, int rows, int L, hipStream_t s) {
  hipLaunchKernelGGL(mse_rows_kernel, dim3(rows), dim3(256), 0, s, pred, target, out, L);
  return check_launch("mse_rows_kernel");
}

int pack_conv3x3_launch(const float* w, bf16_t* out, int Cout, int Cin, int ldw, int col_off, hipStream_t s, int cin_pad) {
  if (cin_pad <= 0) cin_pad = Cin;
  hipLaunchKernelGGL(pack_conv3x3_kernel, ew_grid((long)Cout * Cin * 9), dim3(EW_BLOCK), 0, s, w, out, Cout, Cin, ldw, col_off, cin_pad);
  return check_launch("pack_conv3x3_kernel");
}
int pack_matrix_launch(const float* w, bf16_t* out, int N, int K, int ldw, int row_off, int col_off, int geglu, hipStream_t s) {
  hipLaunchKernelGGL(pack_matrix_kernel, ew_grid((long)N * K), dim3(EW_BLOCK), 0, s, w, out, N, K, ldw, row_off, col_off, geglu);
  return check_launch("pack_matrix_kernel");
}
int pack_vector_launch(const float* v, float* out, int N, int off, int geglu, int accumulate, hipStream_t s) {
  hipLaunchKernelGGL(pack_vector_kernel, ew_grid(N), dim3(EW_BLOCK), 0, s, v, out, N, off, geglu, accumulate);
  return check_launch("pack_vector_kernel");
}

}  // namespace dfh

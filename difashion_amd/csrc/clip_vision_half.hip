// CLIP image encoder in the library's 16-bit storage format: the `dfh_clipvh_*` family.
//
// Replaces (arithmetic) the half-precision forms of the tower the reference's evaluation calls through ``encode_image``
// (Evaluation/extract_hist_embs.py:83-100, Evaluation/eval_utils.py:91-135, :503-535): open_clip's precision="bf16" / "fp16",
// transformers' torch_dtype= / .half().  The fp32 walk (clip_vision.hip) is untouched and stays the default.
//
// "16-bit" is the storage format of the library this file is compiled into (bf16; fp16 under -DDFH_F16), as for the U-Net.  The walk
// runs on the project's 16-bit kernels: the tile GEMM (gemm.hip, planned by gemm_plan.hip), dfh_layernorm's kernel (norm.hip) and
// the flash attention kernels (attention.hip / attention_x32.hip).  The residual stream is 16-bit between launches, as in the real
// half-precision classes; every accumulation, LayerNorm statistic, softmax and activation is fp32.  New here:
//   * half_plan(): ONE host function with the geometry of every launch and the workspace carve (C ABI: dfh_clipvh_plan), recorded
//     through clip_tower_half.h, which also holds the per-layer packed copy and the walk over the blocks (shared with the text tower);
//   * im2col into 16-bit rows whose K is zero-padded to a multiple of 8 (16-byte rows for the GEMM's staging);
//   * class token + position embeddings + pre_layrnorm in one launch (16-bit patch rows in, fp32 arithmetic, 16-bit out);
//   * the fp32 upcasts that leave as last_hidden_state / hidden_states, and the class rows for the fp32 tail.
// Ragged sequences (T = 257, 197, 50; M = batch * T is no multiple of a row tile) -- what was read in the kernels the walk launches:
//   * gemm_bf16_kernel: rows beyond M are staged from the zero page (generic k-loop) or clamped to row M - 1 (LEAN); every store
//     path tests m < M and n < N.  The q | k | v launch writes V^T through the second destination (GemmArgs::out2) with
//     rows_per_b = T: its transposed STAGED epilogue needs rows_per_b % 8 == 0 and a tile inside one image, so at these lengths the
//     V^T column tiles leave through the per-element transposed path (m / rows_per_b per row), which is correct for any T.
//   * attention_kernel (16x16x32; taken at T = 197 / 50 and at head dim 64 below 1024 tokens): K rows beyond Nk are not loaded (zeros),
//     V^T chunks beyond Nk are zeros and a straddling chunk has its padding keys masked to zero bits (whatever the 7 padding columns
//     of a V^T row hold), scores of keys >= Nk are -inf before the running max, every tile holds at least one real key so the
//     deferred-max offset stays finite; query rows >= Nq load zeros and are not stored.
//   * attention_x32_kernel (32x32x16; taken at head dim 80 from 256 tokens on: ViT-H/14): K through a buffer descriptor that ends
//     with the last real key (rows beyond read zeros), V^T chunks masked as above, keys >= Nk carry 1.0 in the mask slot against
//     -30000 on the Q side (exp2 -> 0), the ragged last tile's mask column is rewritten when it lands in its buffer; the second
//     workgroup of a 257-token head holds one real query.  Nothing had to be changed in either kernel.
// No atomics anywhere: a rerun is bit-identical.  A row's result may depend on the batch it rides in (the GEMM plan, hence the
// summation order of split-K launches, depends on M).
#include <cmath>
#include <cstring>

#include "attention.h"
#include "clip_tower_half.h"
#include "clip_vision_model.h"
#include "gemm_plan.h"
#include "norm_steps.h"
#include "walk_knobs.h"

namespace dfh {
bool attention_x32_eligible(const AttnArgs& a);      // attention_x32.hip
}

namespace {

// ------------------------------------------------------------------ im2col of the patch conv, 16-bit rows
// col[b * P * P + py * P + px][c * p * p + ky * p + kx] for k < K, zeros for K <= k < Kpad; one thread = 8 consecutive k = one 16-byte store
template <bool PX16>
__global__ __launch_bounds__(256) void clipvh_im2col_kernel(const void* __restrict__ px, bf16_t* __restrict__ col, int C, int S, int p, int P,
                                                            int K, int Kpad, long chunks) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= chunks) return;
  const int c8 = Kpad >> 3;
  const long m = e / c8;
  const int k0 = (int)(e - m * c8) * 8;
  const int b = (int)(m / (P * P)), pp = (int)(m - (long)b * P * P), py = pp / P, pxx = pp - py * P;
  float f[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int k = k0 + i;
    f[i] = 0.f;
    if (k < K) {
      const int c = k / (p * p), ky = (k - c * p * p) / p, kx = k - c * p * p - ky * p;
      const long src = (((long)b * C + c) * S + py * p + ky) * S + pxx * p + kx;
      f[i] = PX16 ? bf2f(((const bf16_t*)px)[src]) : ((const float*)px)[src];
    }
  }
  *(uint4*)(col + m * Kpad + k0) = pack8(f);
}

// ------------------------------------------------------------------ class token + position embeddings + pre_layrnorm
// v = (t == 0 ? class_embedding : patch[b][t - 1]) + pos[t]; x[b][t] = LayerNorm(v) * g + b.  One wave per token row, the row in
// registers (D <= 2048: four 16-byte chunks a lane), exact two-pass variance in fp32.
__global__ __launch_bounds__(256) void clipvh_embed_ln_kernel(const bf16_t* __restrict__ patch, const float* __restrict__ cls,
                                                              const float* __restrict__ pos, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, bf16_t* __restrict__ x, int M, int T, int D, float eps) {
  const int lane = threadIdx.x & 63;
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= M) return;
  const int t = m % T, b = m / T, C8 = D >> 3;
  float v[4][8];
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int o = lane + i * 64;
    if (o < C8) {
      float q[8];
      load8f(pos + (long)t * D + o * 8, q);
      if (t == 0) load8f(cls + o * 8, v[i]);
      else unpack8(*(const uint4*)(patch + ((long)b * (T - 1) + (t - 1)) * D + o * 8), v[i]);
#pragma unroll
      for (int k = 0; k < 8; ++k) { v[i][k] += q[k]; sum += v[i][k]; }
    }
  }
  const float mean = wave_sum(sum) / (float)D;
  float sq = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (lane + i * 64 < C8) {
#pragma unroll
      for (int k = 0; k < 8; ++k) { v[i][k] -= mean; sq = fmaf(v[i][k], v[i][k], sq); }
    }
  }
  const float rstd = rsqrtf(wave_sum(sq) / (float)D + eps);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int o = lane + i * 64;
    if (o < C8) {
      float g[8], bb[8], f[8];
      load8f(gamma + o * 8, g); load8f(beta + o * 8, bb);
#pragma unroll
      for (int k = 0; k < 8; ++k) f[k] = fmaf(v[i][k] * rstd, g[k], bb[k]);
      *(uint4*)(x + (long)m * D + o * 8) = pack8(f);
    }
  }
}

// ------------------------------------------------------------------ 16-bit rows -> fp32 (exact): out[r][:] = x[r * row_stride : + D]
// row_stride = D: the whole stream (hidden_states, last_hidden_state); row_stride = T * D: the class row of every image
__global__ __launch_bounds__(256) void clipvh_upcast_kernel(const bf16_t* __restrict__ x, float* __restrict__ out, long rows, int D, long row_stride) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  const int C8 = D >> 3;
  if (e >= rows * C8) return;
  const long r = e / C8;
  const int o = (int)(e - r * C8);
  float f[8];
  unpack8(*(const uint4*)(x + r * row_stride + o * 8), f);
  float4* dst = (float4*)(out + r * D + o * 8);
  dst[0] = make_float4(f[0], f[1], f[2], f[3]);
  dst[1] = make_float4(f[4], f[5], f[6], f[7]);
}

int upcast(const bf16_t* x, float* out, long rows, int D, long row_stride, hipStream_t s) {
  const long chunks = rows * (D >> 3);
  dfh::ProfScope ps(dfh::PC_OTHER, 0.0, 6.0 * rows * D, s);
  hipLaunchKernelGGL(clipvh_upcast_kernel, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, s, x, out, rows, D, row_stride);
  return dfh::check_launch("clipvh_upcast_kernel");
}

// ------------------------------------------------------------------ the plan: geometry of every launch, workspace carve, packed layout
enum Region { R_ZERO = 0, R_COL, R_PATCH, R_X, R_LN, R_QK, R_VT, R_ATT, R_HID, R_PARTIAL, R_CLS, R_POOLED, R_COUNT };
enum Launch { L_PATCH = 0, L_QKV, L_OUT, L_FC1, L_FC2, L_COUNT };

bool head_dim_supported(int d) { return d == 32 || d == 40 || d == 64 || d == 80 || d == 128 || d == 160; }

// packed copy: patch [D][Kpad] (16-bit), then the layers (clip_tower_half.h)
struct PackedLayout : dfh::HalfLayerPack {
  size_t patch = 0, layer0, total;
  PackedLayout(int D, int I, int Kpad, int L) : dfh::HalfLayerPack(D, I), layer0(dfh::half_round_up((size_t)D * Kpad * 2)) { total = layer0 + L * per_layer; }
};

int half_plan(const dfh_clipv* c, int batch, dfh_clipvh_plan_info* p) {
  dfh::HalfPlanRecorder<dfh_clipvh_plan_info> r{p, __func__};
  if (int rc = r.open(c, batch)) return rc;
  const dfh_clipv_config& g = c->cfg;
  const int D = g.hidden_size, I = g.intermediate_size, H = g.num_attention_heads, d = D / H, T = c->T, K = c->Kp;
  DFH_REQUIRE(head_dim_supported(d), "the 16-bit tower runs on dfh_attention's kernels: head dim " + std::to_string(d) +
                                         " is not built (supported: 32, 40, 64, 80, 128, 160); the fp32 tower takes any multiple of 4 up to 128");
  DFH_REQUIRE(D % 8 == 0 && I % 8 == 0 && D <= 2048, "the 16-bit tower needs hidden / intermediate sizes that are multiples of 8, hidden <= 2048");
  if (int rc = r.offsets_fit(batch, T, D, I)) return rc;
  const int Kpad = (K + 7) / 8 * 8, M = batch * T, Mp = batch * (T - 1), ldvt = (T + 7) / 8 * 8;
  r.scalars(batch, T, D, I, H, g.num_hidden_layers);
  p->projection_dim = g.projection_dim; p->patch_k = K; p->patch_k_padded = Kpad; p->patch_rows = Mp; p->ldvt = ldvt;
  {
    AttnArgs a; std::memset(&a, 0, sizeof(a));
    a.B = batch; a.H = H; a.D = d; a.Nq = T; a.Nk = T;
    p->attention_x32 = dfh::WalkKnobs::get().attn_x32 && dfh::attention_x32_eligible(a) ? 1 : 0;
  }
  r.launch(L_PATCH, "patch", Mp, D, Kpad, D, ACT_NONE, 0, 0, R_COL, R_PATCH);
  // q | k row-major; V leaves transposed per image through the GEMM's second destination
  dfh_clipvh_launch& qkv = r.launch(L_QKV, "qkv", M, 3 * D, D, 2 * D, ACT_NONE, 0, 1, R_LN, R_QK);
  qkv.n_split = 2 * D; qkv.ld_out2 = ldvt; qkv.rows_per_b = T; qkv.out2_region = R_VT;
  r.launch(L_OUT, "out_proj", M, D, D, D, ACT_NONE, 1, 1, R_ATT, R_X);
  r.launch(L_FC1, "fc1", M, I, D, I, dfh::half_act(g.hidden_act), 0, 1, R_LN, R_HID);
  r.launch(L_FC2, "fc2", M, D, I, D, ACT_NONE, 1, 1, R_HID, R_X);
  {
    // the q | k | v launch writes V^T through the GEMM's second destination, which begins at a column-tile edge: 2 D must be a whole
    // number of the column tiles that launch gets (160 when 3 D is a multiple of 160 or no multiple of 128, else 128)
    GemmArgs a = dfh::half_linear_args(p->launches[L_QKV]);
    int tile = 0;
    dfh::gemm_pick_split(a, &tile);
    const int bn = dfh::kGemmTiles[tile].bn;
    DFH_REQUIRE((2 * D) % bn == 0, "the 16-bit tower's q | k | v launch runs on " + std::to_string(bn) + "-column tiles at hidden size " + std::to_string(D) +
                                       " and writes V^T from column 2 x hidden on: 2 x hidden must be a multiple of " + std::to_string(bn) +
                                       " (hidden a multiple of 64 when 3 x hidden is a multiple of 128, else of 80); the fp32 tower takes this config");
  }
  // the q | k | v launch and fc1 are single-pass by construction
  const size_t partial = r.partial_floats({L_PATCH, L_OUT, L_FC2});
  r.region(R_ZERO, "zero", 256);
  r.region(R_COL, "im2col", (size_t)Mp * Kpad * 2);
  r.region(R_PATCH, "patch", (size_t)Mp * D * 2);
  r.region(R_X, "x", (size_t)M * D * 2);
  r.region(R_LN, "ln", (size_t)M * D * 2);
  r.region(R_QK, "qk", (size_t)M * 2 * D * 2);
  r.region(R_VT, "vt", (size_t)batch * D * ldvt * 2);
  r.region(R_ATT, "attention", (size_t)M * D * 2);
  r.region(R_HID, "mlp_hidden", (size_t)M * I * 2);
  r.region(R_PARTIAL, "splitk_partial", partial * sizeof(float));
  r.region(R_CLS, "class_rows", (size_t)batch * D * sizeof(float));
  r.region(R_POOLED, "pooled", (size_t)batch * D * sizeof(float));
  p->packed_bytes = PackedLayout(D, I, Kpad, g.num_hidden_layers).total;
  return 0;
}

}  // namespace

extern "C" {

int dfh_clipvh_plan(const dfh_clipv* c, int batch, dfh_clipvh_plan_info* out) { return half_plan(c, batch, out); }

size_t dfh_clipvh_packed_bytes(const dfh_clipv* c) {
  dfh_clipvh_plan_info p;
  return half_plan(c, 1, &p) ? 0 : p.packed_bytes;
}

size_t dfh_clipvh_workspace_bytes(const dfh_clipv* c, int batch) {
  dfh_clipvh_plan_info p;
  return half_plan(c, batch, &p) ? 0 : p.workspace_bytes;
}

int dfh_clipvh_pack(dfh_clipv* c, const float* const* master_params, int count, void* packed, void* stream) {
  DFH_REQUIRE(c && master_params && packed, "null argument");
  if (int rc = dfh::require_params(*c, master_params, count, "dfh_clipv")) return rc;
  DFH_REQUIRE(((uintptr_t)packed & 255) == 0, "the packed copy must be 256-byte aligned");
  dfh_clipvh_plan_info p;
  if (int rc = half_plan(c, 1, &p)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const int D = p.hidden, K = p.patch_k, Kpad = p.patch_k_padded;
  const PackedLayout lay(D, p.intermediate, Kpad, p.layers);
  unsigned char* base = (unsigned char*)packed;
  // the K padding of the patch weight must read as zeros
  if (hipMemsetAsync(base + lay.patch, 0, (size_t)D * Kpad * 2, s) != hipSuccess) { dfh::set_error("dfh_clipvh_pack: memset failed"); return -2; }
  if (int rc = dfh::pack_matrix_launch(master_params[c->patch], (bf16_t*)(base + lay.patch), D, K, Kpad, 0, 0, 0, s)) return rc;
  return dfh::pack_encoder_layers(master_params, c->layers, lay, base + lay.layer0, s);
}

int dfh_clipvh_encode(dfh_clipv* c, const float* const* master_params, int count, const void* packed, const void* pixel_values,
                      int pixel_dtype, int batch, float* last_hidden_state, float* pooler_output, float* image_embeds,
                      float* const* hidden_states, void* workspace, size_t workspace_bytes, void* stream) {
  DFH_REQUIRE(c && master_params && packed && pixel_values && last_hidden_state && workspace, "null argument");
  if (int rc = dfh::require_params(*c, master_params, count, "dfh_clipv")) return rc;
  DFH_REQUIRE(pixel_dtype == 0 || pixel_dtype == 1, "pixel_dtype: 0 = fp32, 1 = the library's 16-bit storage format");
  dfh_clipvh_plan_info p;
  if (int rc = half_plan(c, batch, &p)) return rc;
  hipStream_t s = (hipStream_t)stream;
  const dfh::HalfWalk<dfh_clipvh_plan_info> w{(unsigned char*)workspace, (const unsigned char*)packed, p, s, R_ZERO, R_PARTIAL};
  if (int rc = w.check_buffers(__func__, "dfh_clipvh_workspace_bytes", workspace_bytes)) return rc;
  // im2col reads the pixels one element at a time; the outputs (and the taps) are written as float4; require_params has checked the masters
  DFH_REQUIRE(((uintptr_t)pixel_values & (pixel_dtype ? 1 : 3)) == 0, "pixel_values must be aligned to its element size");
  DFH_REQUIRE((((uintptr_t)last_hidden_state | (uintptr_t)pooler_output | (uintptr_t)image_embeds) & 15) == 0, "outputs must be 16-byte aligned");
  if (hidden_states)
    for (int l = 0; l <= p.layers; ++l)
      DFH_REQUIRE(((uintptr_t)hidden_states[l] & 15) == 0, "hidden_states[" + std::to_string(l) + "] must be 16-byte aligned");
  const dfh_clipv_config& g = c->cfg;
  const int T = p.tokens, D = p.hidden, H = p.heads, d = p.head_dim, M = p.rows, Mp = p.patch_rows;
  const float eps = g.layer_norm_eps, scale = 1.0f / sqrtf((float)d);
  const float* const* P = master_params;
  bf16_t* x = (bf16_t*)w.reg(R_X);
  const PackedLayout lay(D, p.intermediate, p.patch_k_padded, p.layers);
  if (int rc = w.clear_zero_page(__func__)) return rc;
  auto tap = [&](int l) { return hidden_states && hidden_states[l] ? upcast(x, hidden_states[l], M, D, D, s) : 0; };

  // embeddings: im2col -> patch GEMM -> class token + positions + pre_layrnorm
  {
    dfh::census(dfh::CK_CLIPV_EMBED);
    const long chunks = (long)Mp * (p.patch_k_padded >> 3);
    {
      dfh::ProfScope ps(dfh::PC_OTHER, 0.0, (pixel_dtype ? 2.0 : 4.0) * Mp * p.patch_k + 2.0 * Mp * p.patch_k_padded, s);
      const dim3 grid((unsigned)((chunks + 255) / 256));
      if (pixel_dtype) hipLaunchKernelGGL(clipvh_im2col_kernel<true>, grid, dim3(256), 0, s, pixel_values, (bf16_t*)w.reg(R_COL), g.num_channels,
                                          g.image_size, g.patch_size, c->grid, p.patch_k, p.patch_k_padded, chunks);
      else hipLaunchKernelGGL(clipvh_im2col_kernel<false>, grid, dim3(256), 0, s, pixel_values, (bf16_t*)w.reg(R_COL), g.num_channels,
                              g.image_size, g.patch_size, c->grid, p.patch_k, p.patch_k_padded, chunks);
      if (int rc = dfh::check_launch("clipvh_im2col_kernel")) return rc;
    }
    if (int rc = w.linear(L_PATCH, w.pk + lay.patch, nullptr)) return rc;
    {
      dfh::ProfScope ps(dfh::PC_LNORM, 8.0 * M * D, 12.0 * M * D, s);
      hipLaunchKernelGGL(clipvh_embed_ln_kernel, dim3((M + 3) / 4), dim3(256), 0, s, (const bf16_t*)w.reg(R_PATCH), P[c->cls], P[c->pos],
                         P[c->prew], P[c->preb], x, M, T, D, eps);
      if (int rc = dfh::check_launch("clipvh_embed_ln_kernel")) return rc;
    }
  }
  if (int rc = tap(0)) return rc;
  // dfh_attention's kernels over q k [M][2 D] | V^T [batch][D][ldvt]
  auto attention = [&]() {
    AttnArgs a; std::memset(&a, 0, sizeof(a));
    const bf16_t* qk = (const bf16_t*)w.reg(R_QK);
    a.Q = qk; a.ldq = 2 * D; a.K = qk + D; a.ldk = 2 * D; a.Vt = (const bf16_t*)w.reg(R_VT); a.ldvt = p.ldvt;
    a.O = (bf16_t*)w.reg(R_ATT); a.ldo = D; a.B = batch; a.H = H; a.D = d; a.Nq = T; a.Nk = T; a.scale = scale;
    return dfh::attention_launch(a, s);
  };
  if (int rc = dfh::half_blocks(w, L_QKV, P, c->layers, lay, w.pk + lay.layer0, eps, attention, tap)) return rc;
  if (int rc = upcast(x, last_hidden_state, M, D, D, s)) return rc;
  if (pooler_output || image_embeds) {
    // the tail in fp32 arithmetic on the pooled rows only: the fp32 tower's LayerNorm and linear kernels (clip_kernels.h)
    float* cls32 = (float*)w.reg(R_CLS);
    float* pl = pooler_output ? pooler_output : (float*)w.reg(R_POOLED);
    if (int rc = upcast(x, cls32, batch, D, (long)T * D, s)) return rc;
    {
      dfh::ProfScope ps(dfh::PC_LNORM, 8.0 * batch * D, 8.0 * batch * D, s);
      if (int rc = dfh::clip_layernorm(cls32, D, P[c->postw], P[c->postb], pl, batch, D, eps, s)) return rc;
    }
    if (image_embeds)
      if (int rc = dfh::clip_linear(pl, D, P[c->proj], D, nullptr, nullptr, 0, image_embeds, g.projection_dim, batch, g.projection_dim,
                                    dfh::CLIP_ACT_NONE, dfh::PC_LINEAR, s)) return rc;
  }
  return 0;
}

}  // extern "C"

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
//   * half_plan(): ONE host function with the geometry of every launch and the workspace carve (C ABI: dfh_clipvh_plan);
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
#include "clip_vision_model.h"
#include "elementwise.h"
#include "gemm.h"
#include "gemm_plan.h"
#include "norm.h"
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
constexpr size_t ALIGN = 256;
size_t round_up(size_t n) { return (n + ALIGN - 1) / ALIGN * ALIGN; }
enum Region { R_ZERO = 0, R_COL, R_PATCH, R_X, R_LN, R_QK, R_VT, R_ATT, R_HID, R_PARTIAL, R_CLS, R_POOLED, R_COUNT };
enum Launch { L_PATCH = 0, L_QKV, L_OUT, L_FC1, L_FC2, L_COUNT };

bool head_dim_supported(int d) { return d == 32 || d == 40 || d == 64 || d == 80 || d == 128 || d == 160; }

// one plain-segment linear of the walk as the GEMM launcher takes it (pointers filled in by the walk; null in the plan)
GemmArgs linear_args(const dfh_clipvh_launch& l) {
  GemmArgs g;
  std::memset(&g, 0, sizeof(g));
  g.nplain = 1; g.p_c[0] = l.K; g.ldw = l.ldw; g.M = l.M; g.N = l.N; g.act = l.act;
  g.ld_out = l.ld_out; g.ld_res = l.ld_out; g.out_mode = OUT_BF16; g.rows_per_b = l.rows_per_b;
  g.n_split = l.n_split; g.ld_out2 = l.ld_out2;
  return g;
}

// packed copy: patch [D][Kpad]; per layer wqkv [3 D][D], wo [D][D], w1 [I][D], w2 [D][I] (16-bit) and bqkv [3 D] (fp32)
struct PackedLayout {
  size_t patch, layer0, wqkv, wo, w1, w2, bqkv, per_layer, total;
  PackedLayout(int D, int I, int Kpad, int L) {
    patch = 0; layer0 = round_up((size_t)D * Kpad * 2);
    wqkv = 0; wo = wqkv + round_up((size_t)3 * D * D * 2); w1 = wo + round_up((size_t)D * D * 2); w2 = w1 + round_up((size_t)I * D * 2);
    bqkv = w2 + round_up((size_t)D * I * 2); per_layer = bqkv + round_up((size_t)3 * D * 4);
    total = layer0 + (size_t)L * per_layer;
  }
};

int half_plan(const dfh_clipv* c, int batch, dfh_clipvh_plan_info* p) {
  DFH_REQUIRE(c && p, "null argument");
  std::memset(p, 0, sizeof(*p));
  DFH_REQUIRE(batch > 0 && batch <= 65535, "batch must be in [1, 65535]");
  const dfh_clipv_config& g = c->cfg;
  const int D = g.hidden_size, I = g.intermediate_size, H = g.num_attention_heads, d = D / H, T = c->T, K = c->Kp;
  DFH_REQUIRE(head_dim_supported(d), "the 16-bit tower runs on dfh_attention's kernels: head dim " + std::to_string(d) +
                                         " is not built (supported: 32, 40, 64, 80, 128, 160); the fp32 tower takes any multiple of 4 up to 128");
  DFH_REQUIRE(D % 8 == 0 && I % 8 == 0 && D <= 2048, "the 16-bit tower needs hidden / intermediate sizes that are multiples of 8, hidden <= 2048");
  DFH_REQUIRE((double)batch * T * (3.0 * D > I ? 3.0 * D : I) < 2.0e9, "batch x tokens x width beyond 32-bit element offsets");
  const int Kpad = (K + 7) / 8 * 8, M = batch * T, Mp = batch * (T - 1), ldvt = (T + 7) / 8 * 8;
  p->batch = batch; p->tokens = T; p->hidden = D; p->intermediate = I; p->heads = H; p->head_dim = d; p->layers = g.num_hidden_layers;
  p->projection_dim = g.projection_dim; p->patch_k = K; p->patch_k_padded = Kpad; p->rows = M; p->patch_rows = Mp; p->ldvt = ldvt;
  {
    AttnArgs a; std::memset(&a, 0, sizeof(a));
    a.B = batch; a.H = H; a.D = d; a.Nq = T; a.Nk = T;
    p->attention_x32 = dfh::WalkKnobs::get().attn_x32 && dfh::attention_x32_eligible(a) ? 1 : 0;
  }
  const int gact = g.hidden_act == dfh::CLIP_ACT_GELU ? ACT_GELU : ACT_QUICK_GELU;
  auto launch = [&](int id, const char* name, int M_, int N, int K_, int ld_out, int act, int resid, int per_layer, int a_reg, int out_reg) {
    dfh_clipvh_launch& l = p->launches[id];
    std::strncpy(l.name, name, sizeof(l.name) - 1);
    l.M = M_; l.N = N; l.K = K_; l.lda = K_; l.ldw = K_; l.ld_out = ld_out; l.rows_per_b = M_; l.act = act; l.resid = resid;
    l.per_layer = per_layer; l.a_region = a_reg; l.out_region = out_reg; l.out2_region = -1;
  };
  launch(L_PATCH, "patch", Mp, D, Kpad, D, ACT_NONE, 0, 0, R_COL, R_PATCH);
  launch(L_QKV, "qkv", M, 3 * D, D, 2 * D, ACT_NONE, 0, 1, R_LN, R_QK);
  p->launches[L_QKV].n_split = 2 * D; p->launches[L_QKV].ld_out2 = ldvt; p->launches[L_QKV].rows_per_b = T; p->launches[L_QKV].out2_region = R_VT;
  launch(L_OUT, "out_proj", M, D, D, D, ACT_NONE, 1, 1, R_ATT, R_X);
  launch(L_FC1, "fc1", M, I, D, I, gact, 0, 1, R_LN, R_HID);
  launch(L_FC2, "fc2", M, D, I, D, ACT_NONE, 1, 1, R_HID, R_X);
  p->num_launches = L_COUNT;
  {
    // the q | k | v launch writes V^T through the GEMM's second destination, which begins at a column-tile edge: 2 D must be a whole
    // number of the column tiles that launch gets (160 when 3 D is a multiple of 160 or no multiple of 128, else 128)
    GemmArgs a = linear_args(p->launches[L_QKV]);
    int tile = 0;
    dfh::gemm_pick_split(a, &tile);
    const int bn = dfh::kGemmTiles[tile].bn;
    DFH_REQUIRE((2 * D) % bn == 0, "the 16-bit tower's q | k | v launch runs on " + std::to_string(bn) + "-column tiles at hidden size " + std::to_string(D) +
                                       " and writes V^T from column 2 x hidden on: 2 x hidden must be a multiple of " + std::to_string(bn) +
                                       " (hidden a multiple of 64 when 3 x hidden is a multiple of 128, else of 80); the fp32 tower takes this config");
  }
  // split-K slabs of the launches that follow the heuristics (the q | k | v launch and fc1 are single-pass by construction)
  size_t partial = 0;
  for (int id : {(int)L_PATCH, (int)L_OUT, (int)L_FC2}) {
    GemmArgs a = linear_args(p->launches[id]);
    if (p->launches[id].resid) a.resid = (const bf16_t*)p;           // presence only
    const size_t f = dfh::gemm_partial_floats(a);
    partial = f > partial ? f : partial;
  }
  size_t off = 0;
  auto region = [&](int id, const char* name, size_t bytes) {
    dfh_clipvh_region& r = p->regions[id];
    std::strncpy(r.name, name, sizeof(r.name) - 1);
    r.offset = off; r.bytes = bytes;
    off += round_up(bytes);
  };
  region(R_ZERO, "zero", 256);
  region(R_COL, "im2col", (size_t)Mp * Kpad * 2);
  region(R_PATCH, "patch", (size_t)Mp * D * 2);
  region(R_X, "x", (size_t)M * D * 2);
  region(R_LN, "ln", (size_t)M * D * 2);
  region(R_QK, "qk", (size_t)M * 2 * D * 2);
  region(R_VT, "vt", (size_t)batch * D * ldvt * 2);
  region(R_ATT, "attention", (size_t)M * D * 2);
  region(R_HID, "mlp_hidden", (size_t)M * I * 2);
  region(R_PARTIAL, "splitk_partial", partial * sizeof(float));
  region(R_CLS, "class_rows", (size_t)batch * D * sizeof(float));
  region(R_POOLED, "pooled", (size_t)batch * D * sizeof(float));
  p->num_regions = R_COUNT;
  p->workspace_bytes = off;                                           // the caller hands in a 256-byte aligned block
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
  const int D = p.hidden, I = p.intermediate, K = p.patch_k, Kpad = p.patch_k_padded;
  const PackedLayout lay(D, I, Kpad, p.layers);
  unsigned char* base = (unsigned char*)packed;
  const float* const* P = master_params;
  // the K padding of the patch weight must read as zeros
  if (hipMemsetAsync(base + lay.patch, 0, (size_t)D * Kpad * 2, s) != hipSuccess) { dfh::set_error("dfh_clipvh_pack: memset failed"); return -2; }
  if (int rc = dfh::pack_matrix_launch(P[c->patch], (bf16_t*)(base + lay.patch), D, K, Kpad, 0, 0, 0, s)) return rc;
  for (size_t l = 0; l < c->layers.size(); ++l) {
    const dfh::ClipLayer& L = c->layers[l];
    unsigned char* lb = base + lay.layer0 + l * lay.per_layer;
    bf16_t* wqkv = (bf16_t*)(lb + lay.wqkv);
    float* bqkv = (float*)(lb + lay.bqkv);
    const int w3[3] = {L.qw, L.kw, L.vw}, b3[3] = {L.qb, L.kb, L.vb};
    for (int j = 0; j < 3; ++j) {
      if (int rc = dfh::pack_matrix_launch(P[w3[j]], wqkv, D, D, D, j * D, 0, 0, s)) return rc;
      if (int rc = dfh::pack_vector_launch(P[b3[j]], bqkv, D, j * D, 0, 0, s)) return rc;
    }
    if (int rc = dfh::pack_matrix_launch(P[L.ow], (bf16_t*)(lb + lay.wo), D, D, D, 0, 0, 0, s)) return rc;
    if (int rc = dfh::pack_matrix_launch(P[L.f1w], (bf16_t*)(lb + lay.w1), I, D, D, 0, 0, 0, s)) return rc;
    if (int rc = dfh::pack_matrix_launch(P[L.f2w], (bf16_t*)(lb + lay.w2), D, I, I, 0, 0, 0, s)) return rc;
  }
  return 0;
}

int dfh_clipvh_encode(dfh_clipv* c, const float* const* master_params, int count, const void* packed, const void* pixel_values,
                      int pixel_dtype, int batch, float* last_hidden_state, float* pooler_output, float* image_embeds,
                      float* const* hidden_states, void* workspace, size_t workspace_bytes, void* stream) {
  DFH_REQUIRE(c && master_params && packed && pixel_values && last_hidden_state && workspace, "null argument");
  if (int rc = dfh::require_params(*c, master_params, count, "dfh_clipv")) return rc;
  DFH_REQUIRE(pixel_dtype == 0 || pixel_dtype == 1, "pixel_dtype: 0 = fp32, 1 = the library's 16-bit storage format");
  dfh_clipvh_plan_info p;
  if (int rc = half_plan(c, batch, &p)) return rc;
  DFH_REQUIRE(workspace_bytes >= p.workspace_bytes, "workspace smaller than dfh_clipvh_workspace_bytes");
  DFH_REQUIRE((((uintptr_t)workspace | (uintptr_t)packed) & 255) == 0, "workspace / packed copy must be 256-byte aligned");
  // im2col reads the pixels one element at a time; the outputs (and the taps) are written as float4; require_params has checked the masters
  DFH_REQUIRE(((uintptr_t)pixel_values & (pixel_dtype ? 1 : 3)) == 0, "pixel_values must be aligned to its element size");
  DFH_REQUIRE((((uintptr_t)last_hidden_state | (uintptr_t)pooler_output | (uintptr_t)image_embeds) & 15) == 0, "outputs must be 16-byte aligned");
  if (hidden_states)
    for (int l = 0; l <= p.layers; ++l)
      DFH_REQUIRE(((uintptr_t)hidden_states[l] & 15) == 0, "hidden_states[" + std::to_string(l) + "] must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const dfh_clipv_config& g = c->cfg;
  const int T = p.tokens, D = p.hidden, I = p.intermediate, H = p.heads, d = p.head_dim, M = p.rows, Mp = p.patch_rows;
  const float eps = g.layer_norm_eps, scale = 1.0f / sqrtf((float)d);
  const float* const* P = master_params;
  unsigned char* ws = (unsigned char*)workspace;
  auto reg = [&](int id) { return ws + p.regions[id].offset; };
  const bf16_t* zero = (const bf16_t*)reg(R_ZERO);
  bf16_t* x = (bf16_t*)reg(R_X);
  bf16_t* ln = (bf16_t*)reg(R_LN);
  const PackedLayout lay(D, I, p.patch_k_padded, p.layers);
  const unsigned char* pk = (const unsigned char*)packed;
  if (hipMemsetAsync(reg(R_ZERO), 0, 256, s) != hipSuccess) { dfh::set_error("dfh_clipvh_encode: memset failed"); return -2; }

  // one GEMM launch of the plan: A rows and the output are regions of the workspace, W a matrix of the packed copy
  auto linear = [&](int id, const void* W, const float* bias) {
    const dfh_clipvh_launch& l = p.launches[id];
    GemmArgs a = linear_args(l);
    a.p_src[0] = (const bf16_t*)reg(l.a_region); a.W = (const bf16_t*)W; a.bias = bias; a.zero = zero;
    a.out = reg(l.out_region);
    if (l.resid) a.resid = (const bf16_t*)reg(l.out_region);
    a.partial = (float*)reg(R_PARTIAL);
    if (l.out2_region >= 0) a.out2 = reg(l.out2_region);
    // the second destination and the activation epilogues are single-pass launches: no K split
    const int force_split = (l.out2_region >= 0 || gemm_act_is_xact(l.act)) ? 1 : 0;
    return dfh::gemm_launch(a, s, 0, force_split);
  };
  auto tap = [&](int l) {
    float* dst = hidden_states ? hidden_states[l] : nullptr;
    return dst ? upcast(x, dst, M, D, D, s) : 0;
  };

  // embeddings: im2col -> patch GEMM -> class token + positions + pre_layrnorm
  {
    dfh::census(dfh::CK_CLIPV_EMBED);
    const long chunks = (long)Mp * (p.patch_k_padded >> 3);
    {
      dfh::ProfScope ps(dfh::PC_OTHER, 0.0, (pixel_dtype ? 2.0 : 4.0) * Mp * p.patch_k + 2.0 * Mp * p.patch_k_padded, s);
      const dim3 grid((unsigned)((chunks + 255) / 256));
      if (pixel_dtype) hipLaunchKernelGGL(clipvh_im2col_kernel<true>, grid, dim3(256), 0, s, pixel_values, (bf16_t*)reg(R_COL), g.num_channels,
                                          g.image_size, g.patch_size, c->grid, p.patch_k, p.patch_k_padded, chunks);
      else hipLaunchKernelGGL(clipvh_im2col_kernel<false>, grid, dim3(256), 0, s, pixel_values, (bf16_t*)reg(R_COL), g.num_channels,
                              g.image_size, g.patch_size, c->grid, p.patch_k, p.patch_k_padded, chunks);
      if (int rc = dfh::check_launch("clipvh_im2col_kernel")) return rc;
    }
    if (int rc = linear(L_PATCH, pk + lay.patch, nullptr)) return rc;
    {
      dfh::ProfScope ps(dfh::PC_LNORM, 8.0 * M * D, 12.0 * M * D, s);
      hipLaunchKernelGGL(clipvh_embed_ln_kernel, dim3((M + 3) / 4), dim3(256), 0, s, (const bf16_t*)reg(R_PATCH), P[c->cls], P[c->pos],
                         P[c->prew], P[c->preb], x, M, T, D, eps);
      if (int rc = dfh::check_launch("clipvh_embed_ln_kernel")) return rc;
    }
  }
  if (int rc = tap(0)) return rc;
  for (size_t l = 0; l < c->layers.size(); ++l) {
    const dfh::ClipLayer& L = c->layers[l];
    const unsigned char* lb = pk + lay.layer0 + l * lay.per_layer;
    if (int rc = dfh::layernorm_launch(x, P[L.ln1w], P[L.ln1b], ln, M, D, eps, s)) return rc;
    if (int rc = linear(L_QKV, lb + lay.wqkv, (const float*)(lb + lay.bqkv))) return rc;
    {
      AttnArgs a; std::memset(&a, 0, sizeof(a));
      const bf16_t* qk = (const bf16_t*)reg(R_QK);
      a.Q = qk; a.ldq = 2 * D; a.K = qk + D; a.ldk = 2 * D; a.Vt = (const bf16_t*)reg(R_VT); a.ldvt = p.ldvt;
      a.O = (bf16_t*)reg(R_ATT); a.ldo = D; a.B = batch; a.H = H; a.D = d; a.Nq = T; a.Nk = T; a.scale = scale;
      if (int rc = dfh::attention_launch(a, s)) return rc;
    }
    if (int rc = linear(L_OUT, lb + lay.wo, P[L.ob])) return rc;                    // x += out_proj(attention)
    if (int rc = dfh::layernorm_launch(x, P[L.ln2w], P[L.ln2b], ln, M, D, eps, s)) return rc;
    if (int rc = linear(L_FC1, lb + lay.w1, P[L.f1b])) return rc;
    if (int rc = linear(L_FC2, lb + lay.w2, P[L.f2b])) return rc;                   // x += fc2(act(fc1(.)))
    if (int rc = tap((int)l + 1)) return rc;
  }
  if (int rc = upcast(x, last_hidden_state, M, D, D, s)) return rc;
  if (pooler_output || image_embeds) {
    // the tail in fp32 arithmetic on the pooled rows only: the fp32 tower's LayerNorm and linear kernels (clip_kernels.h)
    float* cls32 = (float*)reg(R_CLS);
    float* pl = pooler_output ? pooler_output : (float*)reg(R_POOLED);
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

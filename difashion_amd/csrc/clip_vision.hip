// CLIP image encoder: vision tower + projection.
//
// Replaces (arithmetic): the OpenCLIP ViT-H/14 ``encode_image`` of the reference's evaluation scripts -- the shared feature extractor of
// Evaluation/extract_hist_embs.py:83-100 (per-user history embeddings), Evaluation/eval_utils.py:91-135 (CLIP score, CLIP image score)
// and :503-535 (personalisation similarity) -- under the architecture and state-dict names of transformers'
// CLIPVisionModelWithProjection, against which it is pinned (tests/golden/make_golden_clip_vision.py).
//
// fp32 end to end like the text tower (clip.hip), whose linear and LayerNorm kernels it launches through clip_kernels.h.  New here:
//   * the patch embedding (a stride-p conv without bias) as an im2col pass + that linear, then class token + position embeddings;
//   * bidirectional attention for sequences that do not fit LDS (ViT-H/14: 257 tokens x head dim 80, K and V of one head = 164 KB):
//     K / V stream through LDS in key tiles under a running maximum / denominator, both products on v_mfma_f32_16x16x4_f32.
// No atomics anywhere: reruns are bit-identical, and a row's result does not depend on the batch it rides in.
#include <cmath>

#include "clip_vision_model.h"

namespace {

// ------------------------------------------------------------------ im2col of the patch conv: col[b * P * P + py * P + px][c * p * p + ky * p + kx]
// (the K order of the conv weight [hidden][C][p][p] read as [hidden][C p p]); pixel_values NCHW
__global__ __launch_bounds__(256) void clipv_im2col_kernel(const float* __restrict__ px, float* __restrict__ col, int C, int S, int p, int P,
                                                           long total) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const int K = C * p * p;
  const long m = e / K;
  const int k = (int)(e - m * K);
  const int c = k / (p * p), ky = (k - c * p * p) / p, kx = k - c * p * p - ky * p;
  const int b = (int)(m / (P * P)), pp = (int)(m - (long)b * P * P), py = pp / P, pxx = pp - py * P;
  col[e] = px[(((long)b * C + c) * S + py * p + ky) * S + pxx * p + kx];
}

// x[b][0] = class_embedding + pos[0];  x[b][1 + i] = patch[b][i] + pos[1 + i]   (CLIPVisionEmbeddings.forward)
__global__ __launch_bounds__(256) void clipv_embed_kernel(const float* __restrict__ patch, const float* __restrict__ cls,
                                                          const float* __restrict__ pos, float* __restrict__ x, int T, int D) {
  const int m = blockIdx.x, t = m % T, b = m / T;
  const float4* a = (const float4*)(t == 0 ? cls : patch + ((long)b * (T - 1) + (t - 1)) * D);
  const float4* q = (const float4*)(pos + (long)t * D);
  float4* o = (float4*)(x + (long)m * D);
  for (int c = threadIdx.x; c < D / 4; c += 256) {
    const float4 u = a[c], v = q[c];
    o[c] = make_float4(u.x + v.x, u.y + v.y, u.z + v.z, u.w + v.w);
  }
}

// ------------------------------------------------------------------ bidirectional attention, any sequence length
// qkv [B * T][3 D] fp32 (q | k | v), O [B * T][D].  Workgroup = (64-query tile, head, image); a wave owns 16 queries.  Keys arrive in
// tiles of KT through LDS; per tile and wave
//   S^T = K Q^T   (A = K fragment from LDS, B = the wave's Q fragment, held in registers for the whole kernel)
//   O^T += V^T P^T (A = V fragment from LDS, B = the probabilities straight from the S^T accumulators)
// With the products transposed, the C layout of 16x16x4 (acc[r] = C[4 * (lane / 16) + r][lane % 16]) puts QUERY lane % 16 in every
// lane of both accumulators: lane (fr, fk) holds S[query fr][key 16 j + 4 fk + r], which is exactly a B operand
// (B[k = fk][column = fr]) of the PV product once the four keys of a 16-key block that share r are taken as one k-group -- the
// contraction order is free as long as A follows it (A = V[key 16 j + 4 fk + r][channel]).  So P never goes through LDS, the softmax
// statistics of a query live in the four lanes fr, fr + 16, fr + 32, fr + 48 (rows_max / rows_sum: two permlane swaps), and the
// rescale of O by exp(m_old - m_new) is a per-lane scalar.
// LDS rows: K stride d + 2 (fragment read: bank = (2 odd fr + fk) mod 32 -> the 32 lanes of a ds_read_b32 group hit 32 banks),
// V stride = 4 mod 8 (bank = (16 fk + fr + const) mod 32).  Ragged ends: key rows beyond T are loaded from row T - 1 (finite) and
// their scores set to -inf; query rows beyond T compute on row T - 1 and are not stored.  Head dims that are not a multiple of 16
// leave V columns d .. 16 NB - 1 undefined: they feed only output rows (channels) that are never stored.
template <int NB, int KT>
__global__ __launch_bounds__(256) void clipv_attention_kernel(const float* __restrict__ qkv, float* __restrict__ O, int T, int D, int d,
                                                              float scale) {
  extern __shared__ float smem[];
  const int ldk = d + 2, ldv = (d & 4) ? d + 8 : d + 4;
  float* Ks = smem;                  // [KT][ldk]
  float* Vs = smem + KT * ldk;       // [KT][ldv] (+ slack for the channel over-read of the last row)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, fr = lane & 15, fk = lane >> 4;
  const int h = blockIdx.y, b = blockIdx.z, q0 = blockIdx.x * 64 + wave * 16;
  const float* base = qkv + (long)b * T * 3 * D + h * d;
  const int qrow = min(q0 + fr, T - 1);
  float q[NB * 4];
#pragma unroll
  for (int s = 0; s < NB * 4; ++s) q[s] = 4 * s < d ? base[(long)qrow * 3 * D + 4 * s + fk] : 0.f;
  f32x4_t oacc[NB];
#pragma unroll
  for (int n = 0; n < NB; ++n) oacc[n] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.f;
  const int d2 = d >> 1, d4 = d >> 2;
  for (int k0 = 0; k0 < T; k0 += KT) {
    __syncthreads();                                   // the previous tile's fragment reads are done
    for (int e = tid; e < KT * d2; e += 256) {
      const int r = e / d2, c = (e - r * d2) * 2;
      const int key = min(k0 + r, T - 1);
      *(float2*)(Ks + r * ldk + c) = *(const float2*)(base + (long)key * 3 * D + D + c);
    }
    for (int e = tid; e < KT * d4; e += 256) {
      const int r = e / d4, c = (e - r * d4) * 4;
      const int key = min(k0 + r, T - 1);
      *(float4*)(Vs + r * ldv + c) = *(const float4*)(base + (long)key * 3 * D + 2 * D + c);
    }
    __syncthreads();
    f32x4_t sacc[KT / 16];
#pragma unroll
    for (int j = 0; j < KT / 16; ++j) sacc[j] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < NB * 4; ++s) {
      if (4 * s < d) {
#pragma unroll
        for (int j = 0; j < KT / 16; ++j)
          sacc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(Ks[(16 * j + fr) * ldk + 4 * s + fk], q[s], sacc[j], 0, 0, 0);
      }
    }
    // sacc[j][r] = S[query fr][key k0 + 16 j + 4 fk + r]
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < KT / 16; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float v = k0 + 16 * j + 4 * fk + r < T ? sacc[j][r] * scale : -INFINITY;
        sacc[j][r] = v;
        mx = fmaxf(mx, v);
      }
    const float m_new = fmaxf(m_run, rows_max(mx));     // finite: key k0 of every tile is a real key
    const float alpha = expf(m_run - m_new);            // first tile: exp(-inf) = 0
    float ls = 0.f;
#pragma unroll
    for (int j = 0; j < KT / 16; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float pv = expf(sacc[j][r] - m_new);
        sacc[j][r] = pv;
        ls += pv;
      }
    l_run = l_run * alpha + rows_sum(ls);
    m_run = m_new;
#pragma unroll
    for (int n = 0; n < NB; ++n) oacc[n] *= alpha;
#pragma unroll
    for (int j = 0; j < KT / 16; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float* vr = Vs + (16 * j + 4 * fk + r) * ldv + fr;
#pragma unroll
        for (int n = 0; n < NB; ++n) oacc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(vr[16 * n], sacc[j][r], oacc[n], 0, 0, 0);
      }
  }
  // oacc[n][r] = O[query fr][channel 16 n + 4 fk + r] * l_run
  if (q0 + fr < T) {
    const float inv = 1.0f / l_run;
    float* orow = O + ((long)b * T + q0 + fr) * D + h * d;
#pragma unroll
    for (int n = 0; n < NB; ++n) {
      const int c = 16 * n + 4 * fk;
      if (c < d) *(float4*)(orow + c) = make_float4(oacc[n][0] * inv, oacc[n][1] * inv, oacc[n][2] * inv, oacc[n][3] * inv);
    }
  }
}

template <int NB, int KT>
int launch_attention(const float* qkv, float* out, int batch, int T, int H, int d, float scale, hipStream_t s) {
  const int ldk = d + 2, ldv = (d & 4) ? d + 8 : d + 4;
  const size_t lds = ((size_t)KT * (ldk + ldv) + 64) * sizeof(float);
  dfh::ProfScope ps(dfh::PC_ATTN, 4.0 * batch * H * (double)T * T * d, 4.0 * 4.0 * batch * (double)T * H * d, s);
  dfh::census(dfh::CK_CLIPV_ATTN);
  hipLaunchKernelGGL((clipv_attention_kernel<NB, KT>), dim3((T + 63) / 64, H, batch), dim3(256), lds, s, qkv, out, T, H * d, d, scale);
  return dfh::check_launch("clipv_attention_kernel");
}

int clipv_attention(const float* qkv, float* out, int batch, int T, int H, int d, float scale, hipStream_t s) {
  if (d <= 64) return launch_attention<4, 64>(qkv, out, batch, T, H, d, scale, s);
  if (d <= 80) return launch_attention<5, 64>(qkv, out, batch, T, H, d, scale, s);
  return launch_attention<8, 32>(qkv, out, batch, T, H, d, scale, s);      // key tiles of 32: K + V tile of d = 128 stays at 34 KB
}

}  // namespace

extern "C" {

int dfh_clipv_create(const dfh_clipv_config* cfg, dfh_clipv** out) {
  DFH_REQUIRE(cfg && out, "null argument");
  DFH_REQUIRE(cfg->hidden_size > 0 && cfg->hidden_size % 4 == 0 && cfg->intermediate_size > 0 && cfg->intermediate_size % 4 == 0,
              "hidden / intermediate size must be multiples of 4");
  DFH_REQUIRE(cfg->num_attention_heads > 0 && cfg->hidden_size % cfg->num_attention_heads == 0, "hidden_size must divide into the heads");
  const int d = cfg->hidden_size / cfg->num_attention_heads;
  DFH_REQUIRE(d % 4 == 0 && d <= 128, "head dim must be a multiple of 4, at most 128 (in use: 64, 80)");
  DFH_REQUIRE(cfg->patch_size > 0 && cfg->image_size >= cfg->patch_size && cfg->image_size % cfg->patch_size == 0,
              "image_size must be a positive multiple of patch_size");
  DFH_REQUIRE(cfg->num_channels > 0 && (cfg->num_channels * cfg->patch_size * cfg->patch_size) % 4 == 0,
              "num_channels * patch_size^2 must be a multiple of 4 (the patch-embedding weight rows are read as float4)");
  DFH_REQUIRE(cfg->image_size <= 4096, "image_size beyond 4096");
  DFH_REQUIRE(cfg->hidden_act == dfh::CLIP_ACT_QUICK_GELU || cfg->hidden_act == dfh::CLIP_ACT_GELU, "hidden_act: 1 = quick_gelu, 2 = gelu");
  DFH_REQUIRE(cfg->num_hidden_layers > 0 && cfg->projection_dim > 0, "num_hidden_layers / projection_dim");
  DFH_REQUIRE(cfg->layer_norm_eps > 0.f, "layer_norm_eps must be positive");
  dfh_clipv* c = new dfh_clipv();
  c->cfg = *cfg;
  c->grid = cfg->image_size / cfg->patch_size;
  c->T = 1 + c->grid * c->grid;
  c->Kp = cfg->num_channels * cfg->patch_size * cfg->patch_size;
  const int D = cfg->hidden_size, I = cfg->intermediate_size;
  // state-dict names and order of transformers' CLIPVisionModelWithProjection
  const std::string vm = "vision_model.";
  c->cls = c->add_param(vm + "embeddings.class_embedding", {D});
  c->patch = c->add_param(vm + "embeddings.patch_embedding.weight", {D, cfg->num_channels, cfg->patch_size, cfg->patch_size});
  c->pos = c->add_param(vm + "embeddings.position_embedding.weight", {c->T, D});
  c->prew = c->add_param(vm + "pre_layrnorm.weight", {D});
  c->preb = c->add_param(vm + "pre_layrnorm.bias", {D});
  c->layers = dfh::add_encoder_layers(*c, vm, cfg->num_hidden_layers, D, I);
  c->postw = c->add_param(vm + "post_layernorm.weight", {D});
  c->postb = c->add_param(vm + "post_layernorm.bias", {D});
  c->proj = c->add_param("visual_projection.weight", {cfg->projection_dim, D});
  *out = c;
  return 0;
}
void dfh_clipv_destroy(dfh_clipv* c) { delete c; }
int dfh_clipv_num_params(const dfh_clipv* c) { return c->num_params(); }
const char* dfh_clipv_param_name(const dfh_clipv* c, int i) { return c->param_name(i); }
int dfh_clipv_param_ndim(const dfh_clipv* c, int i) { return c->param_ndim(i); }
int dfh_clipv_param_dim(const dfh_clipv* c, int i, int d) { return c->param_dim(i, d); }
size_t dfh_clipv_workspace_bytes(const dfh_clipv* c, int batch) { return (c && batch > 0) ? c->workspace(nullptr, batch).bytes() : 0; }

int dfh_clipv_attention(const float* qkv, float* out, int batch, int T, int heads, int head_dim, float scale, void* stream) {
  DFH_REQUIRE(qkv && out, "null argument");
  DFH_REQUIRE(batch > 0 && T > 0 && heads > 0, "batch / T / heads must be positive");
  DFH_REQUIRE(batch <= 65535 && heads <= 65535, "batch / heads beyond the grid limit of 65535");
  DFH_REQUIRE(head_dim > 0 && head_dim % 4 == 0 && head_dim <= 128, "head dim must be a multiple of 4, at most 128");
  DFH_REQUIRE((((uintptr_t)qkv | (uintptr_t)out) & 15) == 0, "qkv / out must be 16-byte aligned");
  return clipv_attention(qkv, out, batch, T, heads, head_dim, scale, (hipStream_t)stream);
}

int dfh_clipv_encode(dfh_clipv* c, const float* const* master_params, int count, const float* pixel_values, int batch,
                     float* last_hidden_state, float* pooler_output, float* image_embeds, float* const* hidden_states,
                     void* workspace, size_t workspace_bytes, void* stream) {
  DFH_REQUIRE(c && master_params && pixel_values && last_hidden_state && workspace, "null argument");
  if (int rc = dfh::require_params(*c, master_params, count, "dfh_clipv")) return rc;
  DFH_REQUIRE(batch > 0 && batch <= 65535, "batch must be in [1, 65535]");
  DFH_REQUIRE(workspace_bytes >= dfh_clipv_workspace_bytes(c, batch), "workspace smaller than dfh_clipv_workspace_bytes");
  DFH_REQUIRE(((uintptr_t)workspace & 255) == 0, "workspace must be 256-byte aligned");
  DFH_REQUIRE((((uintptr_t)pixel_values | (uintptr_t)last_hidden_state | (uintptr_t)pooler_output | (uintptr_t)image_embeds) & 15) == 0,
              "pixel_values / outputs must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const dfh_clipv_config& g = c->cfg;
  const int T = c->T, D = g.hidden_size, I = g.intermediate_size, H = g.num_attention_heads, d = D / H, K = c->Kp;
  const int M = batch * T, Mp = batch * (T - 1);
  DFH_REQUIRE((double)batch * T < 2.0e9 / (3.0 * D > I ? 3.0 * D : I), "batch x tokens x width beyond 32-bit row offsets");
  const dfh::ClipWorkspace w = c->workspace(workspace, batch);
  const float* const* P = master_params;
  const float eps = g.layer_norm_eps, scale = 1.0f / sqrtf((float)d);
  const size_t hs_bytes = (size_t)M * D * sizeof(float);
  const dfh::ClipAccounting acct = {dfh::PC_LINEAR, dfh::CK_CLIPV_LINEAR, dfh::PC_LNORM, dfh::CK_CLIPV_LAYERNORM};
  // hidden_states[l]: entry l of an array of pointers, any of which may be null
  auto tap = [&](int l, const float* src) {
    return dfh::tower_copy(hidden_states ? hidden_states[l] : nullptr, src, hs_bytes, s, "dfh_clipv_encode: hidden_states");
  };
  auto attention = [&](const float* qkv, float* att) { return clipv_attention(qkv, att, batch, T, H, d, scale, s); };
  // embeddings: im2col -> qkv region, patch conv as a linear -> att region, + class token + positions -> ln, pre_layrnorm -> x
  {
    dfh::census(dfh::CK_CLIPV_EMBED);
    const long total = (long)Mp * K;
    {
      dfh::ProfScope ps(dfh::PC_OTHER, 0.0, 8.0 * total, s);
      hipLaunchKernelGGL(clipv_im2col_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, pixel_values, w.qkv, g.num_channels,
                         g.image_size, g.patch_size, c->grid, total);
      if (int rc = dfh::check_launch("clipv_im2col_kernel")) return rc;
    }
    if (int rc = dfh::clip_linear(w.qkv, K, P[c->patch], K, nullptr, nullptr, 0, w.att, D, Mp, D, dfh::CLIP_ACT_NONE, dfh::PC_OTHER, s)) return rc;
    {
      dfh::ProfScope ps(dfh::PC_OTHER, 1.0 * M * D, 8.0 * M * D, s);
      hipLaunchKernelGGL(clipv_embed_kernel, dim3(M), dim3(256), 0, s, w.att, P[c->cls], P[c->pos], w.ln, T, D);
      if (int rc = dfh::check_launch("clipv_embed_kernel")) return rc;
    }
  }
  if (int rc = dfh::tower_layernorm(acct, w.ln, D, P[c->prew], P[c->preb], w.x, M, D, eps, s)) return rc;
  if (int rc = tap(0, w.x)) return rc;
  if (int rc = dfh::clip_blocks(P, c->layers, w, M, D, I, g.hidden_act, eps, acct, s, attention, tap)) return rc;
  if (int rc = dfh::tower_copy(last_hidden_state, w.x, hs_bytes, s, "dfh_clipv_encode: last_hidden_state")) return rc;
  if (pooler_output || image_embeds) {
    float* pl = pooler_output ? pooler_output : w.tail;
    if (int rc = dfh::tower_layernorm(acct, w.x, (long)T * D, P[c->postw], P[c->postb], pl, batch, D, eps, s)) return rc;   // the class-token row of every image
    if (image_embeds)
      if (int rc = dfh::tower_linear(acct, pl, D, P[c->proj], D, nullptr, nullptr, image_embeds, g.projection_dim, batch, g.projection_dim,
                                     dfh::CLIP_ACT_NONE, s)) return rc;
  }
  return 0;
}

}  // extern "C"

// CLIP text encoder: the frozen prompt encoder on either side of the denoising path.
//
// Replaces (arithmetic): transformers CLIPTextModel as the reference builds and calls it -- constructed at
// DiFashion/models/difashion.py:66-75, run on the category prompts of every training batch (:218-224, null prompt :226-234) and once
// per sampling call (:340-353); only ``[0]`` (last_hidden_state) is consumed.  The reference pins transformers 4.32.1 (README.md:24);
// the arithmetic is restated in oracle/clip_ref.py and PINNED against the installed transformers class (tests/golden/make_golden_clip.py).
//
// Design: the prompts are a closed set (one sentence per category + the empty prompt: <= 51 sequences of 77 tokens, data_utils.py:96-111),
// encoded ONCE per run and reused by every denoising step of every outfit (difashion_amd/prompts.py PromptTable).  The whole encoder is
// 0.67 TFLOP (CLIP-L) / 2.1 TFLOP (OpenCLIP-H) -- a few ms on any MFMA path -- while its output conditions all 50 x 16 U-Net forwards.
// So this file buys PRECISION, not speed: everything stays fp32, the linears run on the fp32 matrix instruction
// (v_mfma_f32_16x16x4_f32, 256 FLOP / clk / CU), weights are read in place from the fp32 master parameters (nn.Linear layout [N][K],
// K contiguous: no packed copy, no arena), and the result agrees with the fp32 reference class to summation-order noise (1e-6),
// not to bf16 noise.  No atomics: reruns are bit-identical.
#include "clip_text_model.h"
#include "f32_tile.h"

namespace {

// ------------------------------------------------------------------ embeddings: x[b][t] = token_embedding[ids[b][t]] + position_embedding[t]
// (CLIPTextEmbeddings.forward; position_ids = arange(T))
__global__ __launch_bounds__(256) void clip_embed_kernel(const int64_t* __restrict__ ids, const float* __restrict__ tok,
                                                         const float* __restrict__ pos, float* __restrict__ x, int T, int D, int vocab) {
  const int m = blockIdx.x, t = m % T;
  long id = ids[m];
  id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);          // the host side refuses out-of-range ids before the launch
  const float4* a = (const float4*)(tok + id * (long)D);
  const float4* p = (const float4*)(pos + (long)t * D);
  float4* o = (float4*)(x + (long)m * D);
  for (int c = threadIdx.x; c < D / 4; c += 256) {
    const float4 u = a[c], v = p[c];
    o[c] = make_float4(u.x + v.x, u.y + v.y, u.z + v.z, u.w + v.w);
  }
}

// ------------------------------------------------------------------ LayerNorm over the last dim, fp32 in / out, one wave per row
// (f32_tile.h layernorm_row); input rows ldx floats apart, output rows dense
__global__ __launch_bounds__(256) void clip_layernorm_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                             const float* __restrict__ b, float* __restrict__ y, int M, int D, float eps, long ldx) {
  dfh::layernorm_row<false>(x, ldx, g, b, y, M, D, eps);
}

// ------------------------------------------------------------------ fp32 linear on the fp32 matrix pipe
//   out[m][n] = act(sum_k A[m][k] W[n][k] + bias[n]) (+ resid[m][n])
// The 64 x 64 tile of f32_tile.h (gemm_tile) with one accumulator down all of K (ChainSum).
using dfh::GT_M; using dfh::GT_N;
using dfh::CLIP_ACT_NONE; using dfh::CLIP_ACT_QUICK_GELU; using dfh::CLIP_ACT_GELU;

DFH_DEVICE float clip_act(float v, int act) {
  if (act == CLIP_ACT_QUICK_GELU) return v / (1.0f + expf(-1.702f * v));           // x * sigmoid(1.702 x)
  if (act == CLIP_ACT_GELU) return 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f));
  return v;
}

__global__ __launch_bounds__(256) void clip_gemm_f32_kernel(const float* __restrict__ A, int lda, const float* __restrict__ W, int ldw,
                                                            const float* __restrict__ bias, const float* resid, int ld_res,
                                                            float* out, int ld_out, int M, int N, int K, int act) {
  dfh::gemm_tile<dfh::ChainSum>(A, lda, W, ldw, bias, M, N, K, [=](int m, int n, float acc) {
    float v = clip_act(acc, act);
    if (resid) v += resid[(long)m * ld_res + n];
    out[(long)m * ld_out + n] = v;
  });
}

// ------------------------------------------------------------------ causal self-attention over one (sequence, head): T <= 128 tokens
// qkv [B * T][3 D] fp32 (q | k | v), O [B * T][D].  K (row stride d + 1) and V of the head sit in LDS; a wave owns query rows
// wave, wave + 4, ...: lane j scores keys j and j + 64 (masked beyond the query position: CLIPTextModel's causal mask, no padding
// mask -- the reference passes input_ids only), softmax in fp32 with the row maximum, then lane c accumulates output channel c.
__global__ __launch_bounds__(256) void clip_attention_kernel(const float* __restrict__ qkv, float* __restrict__ O, int T, int D, int d,
                                                             float scale) {
  extern __shared__ float smem[];
  float* Ks = smem;                         // [T][d + 1]
  float* Vs = Ks + T * (d + 1);             // [T][d]
  float* Qw = Vs + T * d;                   // [4][d]
  float* Pw = Qw + 4 * d;                   // [4][128]
  const int h = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* base = qkv + (long)b * T * 3 * D + h * d;
  for (int e = tid; e < T * d; e += 256) {
    const int t = e / d, c = e - t * d;
    Ks[t * (d + 1) + c] = base[(long)t * 3 * D + D + c];
    Vs[t * d + c] = base[(long)t * 3 * D + 2 * D + c];
  }
  __syncthreads();
  float* q = Qw + wave * d;
  float* p = Pw + wave * 128;
  for (int i = wave; i < T; i += 4) {
    for (int c = lane; c < d; c += 64) q[c] = base[(long)i * 3 * D + c];
    __builtin_amdgcn_wave_barrier();
    float s[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int j = lane + 64 * u;
      float a = -INFINITY;
      if (j <= i) {
        a = 0.f;
        const float* kr = Ks + j * (d + 1);
        for (int c = 0; c < d; ++c) a = fmaf(q[c], kr[c], a);
        a *= scale;
      }
      s[u] = a;
    }
    float mx = fmaxf(s[0], s[1]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    const float e0 = lane <= i ? expf(s[0] - mx) : 0.f, e1 = lane + 64 <= i ? expf(s[1] - mx) : 0.f;
    float sum = e0 + e1;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    const float inv = 1.0f / sum;
    p[lane] = e0 * inv; p[lane + 64] = e1 * inv;
    __builtin_amdgcn_wave_barrier();
    for (int c = lane; c < d; c += 64) {
      float o = 0.f;
      for (int j = 0; j <= i; ++j) o = fmaf(p[j], Vs[j * d + c], o);
      O[((long)b * T + i) * D + h * d + c] = o;
    }
    __builtin_amdgcn_wave_barrier();
  }
}

// pooler_output[b] = last_hidden_state[b][pos]: pos = argmax(ids) when eos_token_id == 2 (the legacy rule of transformers 4.32.1's
// CLIPTextTransformer), else the first position holding eos_token_id (0 when there is none: argmax of an all-false row)
__global__ __launch_bounds__(256) void clip_pool_kernel(const int64_t* __restrict__ ids, const float* __restrict__ y, float* __restrict__ pooled,
                                                        int T, int D, int eos) {
  __shared__ int pos;
  const int b = blockIdx.x;
  if (threadIdx.x == 0) {
    int best = 0;
    if (eos == 2) {
      long mx = ids[(long)b * T];
      for (int t = 1; t < T; ++t) if (ids[(long)b * T + t] > mx) { mx = ids[(long)b * T + t]; best = t; }
    } else {
      for (int t = 0; t < T; ++t) if (ids[(long)b * T + t] == eos) { best = t; break; }
    }
    pos = best;
  }
  __syncthreads();
  for (int c = threadIdx.x; c < D; c += 256) pooled[(long)b * D + c] = y[((long)b * T + pos) * D + c];
}

}  // namespace

extern "C" {

int dfh_clip_create(const dfh_clip_config* cfg, dfh_clip** out) {
  DFH_REQUIRE(cfg && out, "null argument");
  DFH_REQUIRE(cfg->hidden_size > 0 && cfg->hidden_size % 4 == 0 && cfg->intermediate_size % 4 == 0, "hidden / intermediate size must be multiples of 4");
  DFH_REQUIRE(cfg->num_attention_heads > 0 && cfg->hidden_size % cfg->num_attention_heads == 0, "hidden_size must divide into the heads");
  DFH_REQUIRE(cfg->max_position_embeddings > 0 && cfg->max_position_embeddings <= 128, "at most 128 positions (CLIP: 77)");
  DFH_REQUIRE(cfg->hidden_act == CLIP_ACT_QUICK_GELU || cfg->hidden_act == CLIP_ACT_GELU, "hidden_act: 1 = quick_gelu, 2 = gelu");
  DFH_REQUIRE(cfg->vocab_size > 0 && cfg->num_hidden_layers > 0, "vocab_size / num_hidden_layers");
  dfh_clip* c = new dfh_clip();
  c->cfg = *cfg;
  const int D = cfg->hidden_size, I = cfg->intermediate_size;
  // transformers 4.32.1 state-dict names and order (CLIPTextModel -> text_model.*)
  const std::string tm = "text_model.";
  c->tok = c->add_param(tm + "embeddings.token_embedding.weight", {cfg->vocab_size, D});
  c->pos = c->add_param(tm + "embeddings.position_embedding.weight", {cfg->max_position_embeddings, D});
  c->layers = dfh::add_encoder_layers(*c, tm, cfg->num_hidden_layers, D, I);
  c->fw = c->add_param(tm + "final_layer_norm.weight", {D});
  c->fb = c->add_param(tm + "final_layer_norm.bias", {D});
  *out = c;
  return 0;
}
void dfh_clip_destroy(dfh_clip* c) { delete c; }
int dfh_clip_num_params(const dfh_clip* c) { return c->num_params(); }
const char* dfh_clip_param_name(const dfh_clip* c, int i) { return c->param_name(i); }
int dfh_clip_param_ndim(const dfh_clip* c, int i) { return c->param_ndim(i); }
int dfh_clip_param_dim(const dfh_clip* c, int i, int d) { return c->param_dim(i, d); }
size_t dfh_clip_workspace_bytes(const dfh_clip* c, int batch, int seq_len) { return c->workspace(nullptr, batch, seq_len).bytes(); }

}  // extern "C"

// the two launchers the vision tower (clip_vision.hip) shares with this file: clip_kernels.h
namespace dfh {
int clip_linear(const float* A, int lda, const float* W, int K, const float* bias, const float* resid, int ld_res, float* out,
                int ld_out, int M, int N, int act, int prof_class, hipStream_t s) {
  ProfScope ps(prof_class, 2.0 * M * N * K, 4.0 * ((double)M * K + (double)N * K + (double)M * N), s);
  const dim3 grid((N + GT_N - 1) / GT_N, (M + GT_M - 1) / GT_M);
  hipLaunchKernelGGL(clip_gemm_f32_kernel, grid, dim3(256), 0, s, A, lda, W, K, bias, resid, ld_res, out, ld_out, M, N, K, act);
  return check_launch("clip_gemm_f32_kernel");
}
int clip_layernorm(const float* x, long ldx, const float* g, const float* b, float* y, int M, int D, float eps, hipStream_t s) {
  hipLaunchKernelGGL(clip_layernorm_kernel, dim3((M + 3) / 4), dim3(256), 0, s, x, g, b, y, M, D, eps, ldx);
  return check_launch("clip_layernorm_kernel");
}
}  // namespace dfh

namespace {

// What the two text entry points share: the checks of an encode call, the embeddings and the pre-LN blocks over w.x (hidden_states taps
// on the way).  Leaves the last block's output, not yet normalised, in w.x.  who: the entry point, for the messages.
int clip_text_walk(const char* who, dfh_clip* c, const float* const* master_params, int count, const int64_t* input_ids,
                   float* hidden_states, void* workspace, size_t workspace_bytes, int batch, int seq_len, hipStream_t s) {
  auto refuse = [&](const char* msg) { dfh::set_error(std::string(who) + ": " + msg); return -1; };
  if (int rc = dfh::require_params(*c, master_params, count, "dfh_clip")) return rc;
  if (!(batch > 0 && seq_len > 0 && seq_len <= c->cfg.max_position_embeddings))
    return refuse("sequence length must be in [1, max_position_embeddings] (CLIPTextEmbeddings raises too)");
  if (workspace_bytes < dfh_clip_workspace_bytes(c, batch, seq_len)) return refuse("workspace smaller than dfh_clip_workspace_bytes");
  if (((uintptr_t)workspace & 255) != 0) return refuse("workspace must be 256-byte aligned");
  const int T = seq_len, D = c->cfg.hidden_size, I = c->cfg.intermediate_size, H = c->cfg.num_attention_heads, d = D / H;
  const int M = batch * T;
  const size_t lds = ((size_t)T * (2 * d + 1) + 4 * d + 4 * 128) * sizeof(float);
  if (lds > 64 * 1024) return refuse("head_dim x sequence length does not fit the attention kernel's LDS tile");
  const dfh::ClipWorkspace w = c->workspace(workspace, batch, T);
  const float* const* P = master_params;
  const float eps = c->cfg.layer_norm_eps, scale = 1.0f / sqrtf((float)d);
  hipLaunchKernelGGL(clip_embed_kernel, dim3(M), dim3(256), 0, s, input_ids, P[c->tok], P[c->pos], w.x, T, D, c->cfg.vocab_size);
  if (int rc = dfh::check_launch("clip_embed_kernel")) return rc;
  const std::string what = std::string(who) + ": hidden_states";
  // hidden_states[l]: slice l of one buffer
  auto tap = [&](int l, const float* src) {
    return dfh::tower_copy(hidden_states ? hidden_states + l * (size_t)M * D : nullptr, src, (size_t)M * D * sizeof(float), s, what.c_str());
  };
  auto attention = [&](const float* qkv, float* att) {
    hipLaunchKernelGGL(clip_attention_kernel, dim3(H, batch), dim3(256), lds, s, qkv, att, T, D, d, scale);
    return dfh::check_launch("clip_attention_kernel");
  };
  if (int rc = tap(0, w.x)) return rc;
  const dfh::ClipAccounting acct = {dfh::PC_OTHER, -1, -1, -1};
  return dfh::clip_blocks(P, c->layers, w, M, D, I, c->cfg.hidden_act, eps, acct, s, attention, tap);
}

}  // namespace

extern "C" {

int dfh_clip_encode(dfh_clip* c, const float* const* master_params, int count, const int64_t* input_ids, float* last_hidden_state,
                    float* pooler_output, int eos_token_id, float* hidden_states, void* workspace, size_t workspace_bytes, int batch,
                    int seq_len, void* stream) {
  DFH_REQUIRE(c && master_params && input_ids && last_hidden_state && workspace, "null argument");
  hipStream_t s = (hipStream_t)stream;
  if (int rc = clip_text_walk("dfh_clip_encode", c, master_params, count, input_ids, hidden_states, workspace, workspace_bytes, batch, seq_len, s))
    return rc;
  const int T = seq_len, D = c->cfg.hidden_size, M = batch * T;
  const dfh::ClipWorkspace w = c->workspace(workspace, batch, T);
  const float* const* P = master_params;
  if (int rc = dfh::clip_layernorm(w.x, D, P[c->fw], P[c->fb], last_hidden_state, M, D, c->cfg.layer_norm_eps, s)) return rc;
  if (pooler_output) {
    hipLaunchKernelGGL(clip_pool_kernel, dim3(batch), dim3(256), 0, s, input_ids, last_hidden_state, pooler_output, T, D, eos_token_id);
    if (int rc = dfh::check_launch("clip_pool_kernel")) return rc;
  }
  return 0;
}

// CLIPTextModelWithProjection / open_clip's encode_text: the same walk, then the tail runs on the pooled rows alone.  LayerNorm is
// row-local (one wave a row, the same kernel), so gather-then-normalise gives the bits normalise-then-gather gives in dfh_clip_encode.
// The gathered rows and (when pooler_output is not asked for) the normalised rows live in the attention / ln regions of the workspace,
// both free once the last block is done.
int dfh_clip_text_embeds(dfh_clip* c, const float* const* master_params, int count, const float* text_projection, int projection_dim,
                         const int64_t* input_ids, float* text_embeds, float* pooler_output, float* last_hidden_state, int eos_token_id,
                         float* hidden_states, void* workspace, size_t workspace_bytes, int batch, int seq_len, void* stream) {
  DFH_REQUIRE(c && master_params && text_projection && input_ids && text_embeds && workspace, "null argument");
  DFH_REQUIRE(projection_dim > 0, "projection_dim must be positive");
  DFH_REQUIRE(((uintptr_t)text_projection & 15) == 0, "text_projection must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  if (int rc = clip_text_walk("dfh_clip_text_embeds", c, master_params, count, input_ids, hidden_states, workspace, workspace_bytes, batch,
                              seq_len, s)) return rc;
  const int T = seq_len, D = c->cfg.hidden_size, M = batch * T;
  const dfh::ClipWorkspace w = c->workspace(workspace, batch, T);
  const float* const* P = master_params;
  const float eps = c->cfg.layer_norm_eps;
  if (last_hidden_state)
    if (int rc = dfh::clip_layernorm(w.x, D, P[c->fw], P[c->fb], last_hidden_state, M, D, eps, s)) return rc;
  float* rows = w.att;                                       // [batch][D]: the last block's output at the pooled positions
  float* pooled = pooler_output ? pooler_output : w.ln;
  hipLaunchKernelGGL(clip_pool_kernel, dim3(batch), dim3(256), 0, s, input_ids, w.x, rows, T, D, eos_token_id);
  if (int rc = dfh::check_launch("clip_pool_kernel")) return rc;
  if (int rc = dfh::clip_layernorm(rows, D, P[c->fw], P[c->fb], pooled, batch, D, eps, s)) return rc;
  return dfh::clip_linear(pooled, D, text_projection, D, nullptr, nullptr, 0, text_embeds, projection_dim, batch, projection_dim,
                          CLIP_ACT_NONE, dfh::PC_OTHER, s);
}

}  // extern "C"

// CLIP text encoder in the library's 16-bit storage format: the `dfh_cliph_*` family on a dfh_clip context.
//
// Replaces (arithmetic) the half-precision form of the tower the reference trains and samples with: CLIPTextModel under
// `--mixed_precision fp16` autocast (DiFashion/run_eta0.1.sh:1, run_inf4eval.sh:1, inf4eval.py:713-715; called at
// models/difashion.py:218-239 on every training step and :340-353 on every sampling call), transformers' torch_dtype= / .half().
// The fp32 walk (clip.hip) is untouched and stays the default.
//
// "16-bit" is the storage format of the library this file is compiled into (bf16; fp16 under -DDFH_F16).  The walk runs on the tile GEMM
// (gemm.hip, planned by gemm_plan.hip) and dfh_layernorm's kernel (norm.hip); the residual stream is 16-bit between launches, every
// accumulation, LayerNorm statistic, softmax and activation is fp32.  New here:
//   * cliph_plan(): ONE host function with the geometry of every launch and the workspace carve (C ABI: dfh_cliph_plan), recorded
//     through clip_tower_half.h, which also holds the per-layer packed copy and the walk over the blocks (shared with the image tower);
//   * token gather + position add in fp32, rounded once to the 16-bit stream;
//   * causal self-attention for sequences of at most 128 tokens at head dim 64 on the 16-bit 16x16x32 MFMA: one workgroup per
//     (sequence, head), the whole score row resident (exact maximum, no online rescaling);
//   * the eos pooling on the 16-bit stream and the fp32 tail (final_layer_norm, text_projection) on the fp32 tower's launchers.
// No atomics anywhere: a rerun is bit-identical.  A row's result may depend on the batch it rides in (the GEMM plan depends on M), and
// never on a later position of its own sequence (the GEMMs, LayerNorms and embeddings are row-local; the attention kernel below).
#include <cmath>
#include <cstring>

#include "clip_text_model.h"
#include "clip_tower_half.h"
#include "norm_steps.h"

namespace {

// ------------------------------------------------------------------ embeddings: x[b][t] = round16(token_embedding[ids[b][t]] + position_embedding[t])
// one thread = 8 consecutive channels = one 16-byte store; ids clamped as in clip_embed_kernel (the Python side refuses them first)
__global__ __launch_bounds__(256) void cliph_embed_kernel(const int64_t* __restrict__ ids, const float* __restrict__ tok,
                                                          const float* __restrict__ pos, bf16_t* __restrict__ x, int T, int D, int vocab, long chunks) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= chunks) return;
  const int C8 = D >> 3;
  const long m = e / C8;
  const int o = (int)(e - m * C8) * 8, t = (int)(m % T);
  long id = ids[m];
  id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
  float a[8], p[8];
  load8f(tok + id * (long)D + o, a);
  load8f(pos + (long)t * D + o, p);
#pragma unroll
  for (int k = 0; k < 8; ++k) a[k] += p[k];
  *(uint4*)(x + m * D + o) = pack8(a);
}

// ------------------------------------------------------------------ 16-bit rows -> fp32 (exact): out[r][:] = x[r][:]
__global__ __launch_bounds__(256) void cliph_upcast_kernel(const bf16_t* __restrict__ x, float* __restrict__ out, long chunks) {
  const long e = (long)blockIdx.x * 256 + threadIdx.x;
  if (e >= chunks) return;
  float f[8];
  unpack8(*(const uint4*)(x + e * 8), f);
  float4* dst = (float4*)(out + e * 8);
  dst[0] = make_float4(f[0], f[1], f[2], f[3]);
  dst[1] = make_float4(f[4], f[5], f[6], f[7]);
}

// ------------------------------------------------------------------ eos pooling (clip_pool_kernel's rule, clip.hip)
// pos = argmax(ids) when eos == 2 (the legacy rule of transformers 4.32.1), else the first position holding eos (0 when there is none).
// SRC16: rows of the 16-bit stream, upcast exactly; else fp32 rows.  pooled[b][:] = y[b][pos][:]
template <bool SRC16>
__global__ __launch_bounds__(256) void cliph_pool_kernel(const int64_t* __restrict__ ids, const void* __restrict__ y, float* __restrict__ pooled,
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
  const long row = ((long)b * T + pos) * D;
  for (int c = threadIdx.x; c < D; c += 256)
    pooled[(long)b * D + c] = SRC16 ? bf2f(((const bf16_t*)y)[row + c]) : ((const float*)y)[row + c];
}

// ------------------------------------------------------------------ causal self-attention, T <= 128, head dim 64, 16-bit MFMA
// qkv [B * T][ld] 16-bit rows (q at column 0, k at column koff, v at column voff, heads contiguous inside each); O [B * T][ldo].
// One workgroup (4 waves) per (head, sequence).  K of the head sits in LDS row-major (pitch 72), V transposed while staging
// (Vt[channel][key], pitch 136); key rows T .. 127 of both are written as ZEROS.
// Products are computed transposed so that a lane owns ONE query (column lane & 15):
//   S^T = K Q^T   A = K rows   (lane: K[16 kt + lane % 16][32 kk + 8 (lane / 16) + j]),  B = Q^T (lane: Q[q0 + lane % 16][the same 8 channels]);
//                 acc[r] = S[query q0 + lane % 16][key 16 kt + 4 (lane / 16) + r]
//   O^T = V^T P^T A = V^T rows (lane: Vt[16 dt + lane % 16][keys]),  B = P^T (lane: P[query lane % 16][keys]);
//                 the 32 contraction slots of chunk c are keys 32 c + 4 g + j (j < 4) and 32 c + 16 + 4 g + j - 4 (j >= 4), g = lane / 16:
//                 exactly the keys whose scores the lane holds from key tiles 2 c and 2 c + 1, so P never leaves its registers.
// A wave owns 16-query slabs: with nt slabs, wave w takes slab nt - 1 - w and slab nt - 8 + w (the triangle's long and short rows pair up).
// Slab qt needs key tiles 0 .. qt only (wave-uniform); only tile qt is masked per element.  The whole score row of a query is in
// registers, so the maximum is exact and every probability is <= 1 (fp16 build: nothing to overflow).  Sum in fp32 over the unrounded
// probabilities; they are rounded to the storage type for the MFMA; the division by the sum follows the MFMA.
constexpr int CA_D = 64, CA_TMAX = 128, CA_KP = 72, CA_VP = 136;
constexpr int CA_LDS_BYTES = (CA_TMAX * CA_KP + CA_D * CA_VP) * 2;

__global__ __launch_bounds__(256) void cliph_causal_attention_kernel(const bf16_t* __restrict__ qkv, bf16_t* __restrict__ O, int T, int ld, int koff,
                                                                     int voff, int ldo, float scale_log2e) {
  __shared__ __attribute__((aligned(16))) bf16_t Ks[CA_TMAX * CA_KP];
  __shared__ __attribute__((aligned(16))) bf16_t Vt[CA_D * CA_VP];
  const int h = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nt = (T + 15) >> 4, Tp = nt << 4;
  const bf16_t* base = qkv + (long)b * T * ld + h * CA_D;
  // K rows: 8 chunks of 16 bytes a row, zeros beyond T
  for (int e = tid; e < Tp * 8; e += 256) {
    const int key = e >> 3, c = (e & 7) * 8;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (key < T) v = *(const uint4*)(base + (long)key * ld + koff + c);
    *(uint4*)(Ks + key * CA_KP + c) = v;
  }
  // V transposed: consecutive lanes take consecutive keys of one 8-channel chunk (their 2-byte stores fall side by side), zeros beyond T
  for (int e = tid; e < Tp * 8; e += 256) {
    const int c = (e / Tp) * 8, key = e - (e / Tp) * Tp;
    uint4 v = make_uint4(0, 0, 0, 0);
    if (key < T) v = *(const uint4*)(base + (long)key * ld + voff + c);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      Vt[(c + 2 * i) * CA_VP + key] = (bf16_t)(w[i] & 0xffffu);
      Vt[(c + 2 * i + 1) * CA_VP + key] = (bf16_t)(w[i] >> 16);
    }
  }
  __syncthreads();
  const int col = lane & 15, g = lane >> 4;
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {
    const int qt = pass == 0 ? nt - 1 - wave : nt - 8 + wave;              // wave-uniform
    if (qt < 0) continue;
    const int q = qt * 16 + col;                                           // this lane's query
    // Q fragments straight from global memory (rows beyond T: zeros, never read)
    uint4 qf[2] = {make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)};
    if (q < T) {
      const bf16_t* qp = base + (long)q * ld + 8 * g;
      qf[0] = *(const uint4*)qp;
      qf[1] = *(const uint4*)(qp + 32);
    }
    float s[8][4];
    float mx = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 8; ++kt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) s[kt][r] = -INFINITY;
      if (kt <= qt) {
        f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          const uint4 kf = *(const uint4*)(Ks + (kt * 16 + col) * CA_KP + kk * 32 + 8 * g);
          acc = DFH_MFMA_16x16x32(__builtin_bit_cast(h16x8_t, kf), __builtin_bit_cast(h16x8_t, qf[kk]), acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float v = acc[r] * scale_log2e;
          if (kt == qt && 4 * g + r > col) v = -INFINITY;                  // the diagonal tile: key > query
          s[kt][r] = v;
          mx = fmaxf(mx, v);
        }
      }
    }
    mx = rows_max(mx);                                                     // key 0 is never masked: finite
    float sum = 0.f;
#pragma unroll
    for (int kt = 0; kt < 8; ++kt) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[kt][r] = kt <= qt ? __builtin_amdgcn_exp2f(s[kt][r] - mx) : 0.f;  // exp2(-inf) = 0 for masked keys; skipped tiles: 0
        sum += s[kt][r];
      }
    }
    sum = rows_sum(sum);
    f32x4_t o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (2 * c <= qt) {
        const bool hi = 2 * c + 1 <= qt;                                   // wave-uniform: the upper 16 keys of the chunk lie above the slab
        uint4 pf;
        pf.x = pack2bf(s[2 * c][0], s[2 * c][1]); pf.y = pack2bf(s[2 * c][2], s[2 * c][3]);
        pf.z = pack2bf(s[2 * c + 1][0], s[2 * c + 1][1]); pf.w = pack2bf(s[2 * c + 1][2], s[2 * c + 1][3]);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          const bf16_t* vp = Vt + (dt * 16 + col) * CA_VP + c * 32 + 4 * g;
          const uint2 lo = *(const uint2*)vp;
          uint2 up = make_uint2(0, 0);
          if (hi) up = *(const uint2*)(vp + 16);
          const uint4 vf = make_uint4(lo.x, lo.y, up.x, up.y);
          o[dt] = DFH_MFMA_16x16x32(__builtin_bit_cast(h16x8_t, vf), __builtin_bit_cast(h16x8_t, pf), o[dt], 0, 0, 0);
        }
      }
    }
    if (q < T) {
      const float inv = 1.0f / sum;
      bf16_t* op = O + ((long)b * T + q) * ldo + h * CA_D + 4 * g;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        uint2 w;
        w.x = pack2bf(o[dt][0] * inv, o[dt][1] * inv); w.y = pack2bf(o[dt][2] * inv, o[dt][3] * inv);
        *(uint2*)(op + dt * 16) = w;
      }
    }
  }
}

int causal_attention_launch(const bf16_t* qkv, bf16_t* out, int batch, int T, int H, int ld, int koff, int voff, int ldo, float scale, hipStream_t s) {
  dfh::census(dfh::CK_CLIPH_ATTN);
  dfh::ProfScope ps(dfh::PC_ATTN, 2.0 * batch * H * (double)T * T * CA_D, 2.0 * batch * T * H * CA_D * 4.0, s);
  hipLaunchKernelGGL(cliph_causal_attention_kernel, dim3(H, batch), dim3(256), 0, s, qkv, out, T, ld, koff, voff, ldo,
                     scale * 1.44269504088896340736f);
  return dfh::check_launch("cliph_causal_attention_kernel");
}

int upcast(const bf16_t* x, float* out, long elems, hipStream_t s) {
  const long chunks = elems >> 3;
  dfh::ProfScope ps(dfh::PC_OTHER, 0.0, 6.0 * elems, s);
  hipLaunchKernelGGL(cliph_upcast_kernel, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, s, x, out, chunks);
  return dfh::check_launch("cliph_upcast_kernel");
}

// ------------------------------------------------------------------ the plan: geometry of every launch, workspace carve, packed layout
enum Region { R_ZERO = 0, R_X, R_LN, R_QKV, R_ATT, R_HID, R_PARTIAL, R_X32, R_ROWS, R_POOLED, R_COUNT };
enum Launch { L_QKV = 0, L_OUT, L_FC1, L_FC2, L_COUNT };
const char* const kFp32 = "; the fp32 tower (dfh_clip_encode) takes this config";

// the packed copy is the layers alone (clip_tower_half.h), layer 0 at its base
int cliph_plan(const dfh_clip* c, int batch, int seq_len, dfh_cliph_plan_info* p) {
  dfh::HalfPlanRecorder<dfh_cliph_plan_info> r{p, __func__};
  if (int rc = r.open(c, batch)) return rc;
  const dfh_clip_config& g = c->cfg;
  const int D = g.hidden_size, I = g.intermediate_size, H = g.num_attention_heads, d = D / H, T = seq_len;
  DFH_REQUIRE(T >= 1 && T <= CA_TMAX && T <= g.max_position_embeddings,
              "the 16-bit tower's causal attention kernel holds a whole sequence in one workgroup: the sequence length must be in [1, " +
                  std::to_string(g.max_position_embeddings < CA_TMAX ? g.max_position_embeddings : CA_TMAX) + "], got " + std::to_string(T) + kFp32 +
                  " up to max_position_embeddings");
  DFH_REQUIRE(D % 8 == 0 && I % 8 == 0, "the 16-bit tower needs hidden / intermediate sizes that are multiples of 8 (16-byte rows), got " +
                                            std::to_string(D) + " / " + std::to_string(I) + kFp32);
  DFH_REQUIRE(d == CA_D, "the 16-bit tower's causal attention kernel is built for head dim 64 (CLIP-L/14, OpenCLIP-H/14, B/32): head dim " +
                             std::to_string(d) + " is not built" + kFp32);
  if (int rc = r.offsets_fit(batch, T, D, I)) return rc;
  const int M = batch * T;
  r.scalars(batch, T, D, I, H, g.num_hidden_layers);
  p->attention_lds_bytes = CA_LDS_BYTES;
  r.launch(L_QKV, "qkv", M, 3 * D, D, 3 * D, ACT_NONE, 0, 1, R_LN, R_QKV);
  r.launch(L_OUT, "out_proj", M, D, D, D, ACT_NONE, 1, 1, R_ATT, R_X);
  r.launch(L_FC1, "fc1", M, I, D, I, dfh::half_act(g.hidden_act), 0, 1, R_LN, R_HID);
  r.launch(L_FC2, "fc2", M, D, I, D, ACT_NONE, 1, 1, R_HID, R_X);
  // fc1's activation epilogue is single-pass by construction
  const size_t partial = r.partial_floats({L_QKV, L_OUT, L_FC2});
  r.region(R_ZERO, "zero", 256);
  r.region(R_X, "x", (size_t)M * D * 2);
  r.region(R_LN, "ln", (size_t)M * D * 2);
  r.region(R_QKV, "qkv", (size_t)M * 3 * D * 2);
  r.region(R_ATT, "attention", (size_t)M * D * 2);
  r.region(R_HID, "mlp_hidden", (size_t)M * I * 2);
  r.region(R_PARTIAL, "splitk_partial", partial * sizeof(float));
  r.region(R_X32, "x_fp32", (size_t)M * D * sizeof(float));
  r.region(R_ROWS, "eos_rows", (size_t)batch * D * sizeof(float));
  r.region(R_POOLED, "pooled", (size_t)batch * D * sizeof(float));
  p->packed_bytes = (size_t)g.num_hidden_layers * dfh::HalfLayerPack(D, I).per_layer;
  return 0;
}

// What the two encode entry points share: the checks, the embeddings and the pre-LN blocks.  Leaves the last block's output, not yet
// normalised, in the 16-bit stream (region x).
int cliph_walk(dfh_clip* c, const float* const* master_params, int count, const void* packed, const int64_t* input_ids, float* hidden_states,
               void* workspace, size_t workspace_bytes, int batch, int seq_len, hipStream_t s, dfh_cliph_plan_info& p) {
  if (int rc = dfh::require_params(*c, master_params, count, "dfh_clip")) return rc;
  if (int rc = cliph_plan(c, batch, seq_len, &p)) return rc;
  const dfh::HalfWalk<dfh_cliph_plan_info> w{(unsigned char*)workspace, (const unsigned char*)packed, p, s, R_ZERO, R_PARTIAL};
  if (int rc = w.check_buffers(__func__, "dfh_cliph_workspace_bytes", workspace_bytes)) return rc;
  DFH_REQUIRE(((uintptr_t)input_ids & 7) == 0, "input_ids must be 8-byte aligned");
  DFH_REQUIRE(((uintptr_t)hidden_states & 15) == 0, "hidden_states must be 16-byte aligned");
  const int T = p.tokens, D = p.hidden, H = p.heads, M = p.rows;
  const float scale = 1.0f / sqrtf((float)p.head_dim);
  const float* const* P = master_params;
  bf16_t* x = (bf16_t*)w.reg(R_X);
  if (int rc = w.clear_zero_page("dfh_cliph_encode")) return rc;
  auto tap = [&](int l) { return hidden_states ? upcast(x, hidden_states + (size_t)l * M * D, (long)M * D, s) : 0; };

  {
    dfh::census(dfh::CK_CLIPH_EMBED);
    const long chunks = (long)M * (D >> 3);
    dfh::ProfScope ps(dfh::PC_OTHER, 1.0 * M * D, 10.0 * M * D, s);
    hipLaunchKernelGGL(cliph_embed_kernel, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, s, input_ids, P[c->tok], P[c->pos], x, T, D,
                       c->cfg.vocab_size, chunks);
    if (int rc = dfh::check_launch("cliph_embed_kernel")) return rc;
  }
  if (int rc = tap(0)) return rc;
  auto attention = [&]() {
    return causal_attention_launch((const bf16_t*)w.reg(R_QKV), (bf16_t*)w.reg(R_ATT), batch, T, H, 3 * D, D, 2 * D, D, scale, s);
  };
  return dfh::half_blocks(w, L_QKV, P, c->layers, dfh::HalfLayerPack(D, p.intermediate), w.pk, c->cfg.layer_norm_eps, attention, tap);
}

// final_layer_norm over all rows in fp32 arithmetic on the upcast stream -> last_hidden_state
int final_norm_all(dfh_clip* c, const float* const* P, const dfh_cliph_plan_info& p, void* workspace, float* last_hidden_state, hipStream_t s) {
  unsigned char* ws = (unsigned char*)workspace;
  float* x32 = (float*)(ws + p.regions[R_X32].offset);
  if (int rc = upcast((const bf16_t*)(ws + p.regions[R_X].offset), x32, (long)p.rows * p.hidden, s)) return rc;
  dfh::ProfScope ps(dfh::PC_LNORM, 8.0 * p.rows * p.hidden, 8.0 * p.rows * p.hidden, s);
  return dfh::clip_layernorm(x32, p.hidden, P[c->fw], P[c->fb], last_hidden_state, p.rows, p.hidden, c->cfg.layer_norm_eps, s);
}

}  // namespace

extern "C" {

int dfh_cliph_plan(const dfh_clip* c, int batch, int seq_len, dfh_cliph_plan_info* out) { return cliph_plan(c, batch, seq_len, out); }

size_t dfh_cliph_packed_bytes(const dfh_clip* c) {
  dfh_cliph_plan_info p;
  return cliph_plan(c, 1, 1, &p) ? 0 : p.packed_bytes;
}

size_t dfh_cliph_workspace_bytes(const dfh_clip* c, int batch, int seq_len) {
  dfh_cliph_plan_info p;
  return cliph_plan(c, batch, seq_len, &p) ? 0 : p.workspace_bytes;
}

int dfh_cliph_pack(dfh_clip* c, const float* const* master_params, int count, void* packed, void* stream) {
  DFH_REQUIRE(c && master_params && packed, "null argument");
  if (int rc = dfh::require_params(*c, master_params, count, "dfh_clip")) return rc;
  DFH_REQUIRE(((uintptr_t)packed & 255) == 0, "the packed copy must be 256-byte aligned");
  dfh_cliph_plan_info p;
  if (int rc = cliph_plan(c, 1, 1, &p)) return rc;
  return dfh::pack_encoder_layers(master_params, c->layers, dfh::HalfLayerPack(p.hidden, p.intermediate), (unsigned char*)packed, (hipStream_t)stream);
}

int dfh_cliph_encode(dfh_clip* c, const float* const* master_params, int count, const void* packed, const int64_t* input_ids,
                     float* last_hidden_state, float* pooler_output, int eos_token_id, float* hidden_states, void* workspace,
                     size_t workspace_bytes, int batch, int seq_len, void* stream) {
  DFH_REQUIRE(c && master_params && packed && input_ids && last_hidden_state && workspace, "null argument");
  DFH_REQUIRE((((uintptr_t)last_hidden_state | (uintptr_t)pooler_output) & 15) == 0, "outputs must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  dfh_cliph_plan_info p;
  if (int rc = cliph_walk(c, master_params, count, packed, input_ids, hidden_states, workspace, workspace_bytes, batch, seq_len, s, p)) return rc;
  if (int rc = final_norm_all(c, master_params, p, workspace, last_hidden_state, s)) return rc;
  if (pooler_output) {
    hipLaunchKernelGGL(cliph_pool_kernel<false>, dim3(batch), dim3(256), 0, s, input_ids, (const void*)last_hidden_state, pooler_output, p.tokens,
                       p.hidden, eos_token_id);
    if (int rc = dfh::check_launch("cliph_pool_kernel")) return rc;
  }
  return 0;
}

// CLIPTextModelWithProjection: the same walk, then the eos rows are gathered from the 16-bit stream (exact upcasts) and the tail --
// final_layer_norm and text_projection -- runs in fp32 on those `batch` rows only, on the fp32 tower's launchers.  LayerNorm is
// row-local (one wave a row, the same kernel), so pooler_output has the bits dfh_cliph_encode gives.
int dfh_cliph_text_embeds(dfh_clip* c, const float* const* master_params, int count, const void* packed, const float* text_projection,
                          int projection_dim, const int64_t* input_ids, float* text_embeds, float* pooler_output, float* last_hidden_state,
                          int eos_token_id, float* hidden_states, void* workspace, size_t workspace_bytes, int batch, int seq_len, void* stream) {
  DFH_REQUIRE(c && master_params && packed && text_projection && input_ids && text_embeds && workspace, "null argument");
  DFH_REQUIRE(projection_dim > 0, "projection_dim must be positive");
  DFH_REQUIRE(((uintptr_t)text_projection & 15) == 0, "text_projection must be 16-byte aligned");
  DFH_REQUIRE((((uintptr_t)last_hidden_state | (uintptr_t)pooler_output | (uintptr_t)text_embeds) & 15) == 0, "outputs must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  dfh_cliph_plan_info p;
  if (int rc = cliph_walk(c, master_params, count, packed, input_ids, hidden_states, workspace, workspace_bytes, batch, seq_len, s, p)) return rc;
  const float* const* P = master_params;
  if (last_hidden_state)
    if (int rc = final_norm_all(c, P, p, workspace, last_hidden_state, s)) return rc;
  unsigned char* ws = (unsigned char*)workspace;
  float* rows = (float*)(ws + p.regions[R_ROWS].offset);
  float* pooled = pooler_output ? pooler_output : (float*)(ws + p.regions[R_POOLED].offset);
  hipLaunchKernelGGL(cliph_pool_kernel<true>, dim3(batch), dim3(256), 0, s, input_ids, (const void*)(ws + p.regions[R_X].offset), rows, p.tokens,
                     p.hidden, eos_token_id);
  if (int rc = dfh::check_launch("cliph_pool_kernel")) return rc;
  if (int rc = dfh::clip_layernorm(rows, p.hidden, P[c->fw], P[c->fb], pooled, batch, p.hidden, c->cfg.layer_norm_eps, s)) return rc;
  return dfh::clip_linear(pooled, p.hidden, text_projection, p.hidden, nullptr, nullptr, 0, text_embeds, projection_dim, batch, projection_dim,
                          dfh::CLIP_ACT_NONE, dfh::PC_OTHER, s);
}

// the attention kernel on its own (tests, microbenchmarks): qkv [batch * T][3 * heads * 64] 16-bit (q | k | v), out [batch * T][heads * 64]
int dfh_causal_attention(const void* qkv, void* out, int batch, int T, int heads, int head_dim, float scale, void* stream) {
  DFH_REQUIRE(qkv && out, "null argument");
  DFH_REQUIRE(head_dim == CA_D, "built for head dim 64");
  DFH_REQUIRE(T >= 1 && T <= CA_TMAX, "the sequence length must be in [1, 128]");
  DFH_REQUIRE(batch >= 1 && batch <= 65535 && heads >= 1, "batch must be in [1, 65535], heads >= 1");
  DFH_REQUIRE((((uintptr_t)qkv | (uintptr_t)out) & 15) == 0, "qkv / out must be 16-byte aligned");
  const int D = heads * CA_D;
  return causal_attention_launch((const bf16_t*)qkv, (bf16_t*)out, batch, T, heads, 3 * D, D, 2 * D, D, scale, (hipStream_t)stream);
}

}  // extern "C"

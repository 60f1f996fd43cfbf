// Host side of what the two 16-bit CLIP towers (clip_text_half.hip: dfh_cliph_*, clip_vision_half.hip: dfh_clipvh_*) share: the
// per-layer part of the packed copy and the loop that writes it, the recorder both plan functions fill their public struct through,
// one encode's view of its plan (regions, zero page, GEMM launches) and the walk over the pre-LN blocks on the 16-bit stream.  Each
// tower keeps its kernels, its embeddings, its attention launch, what follows the last block and the refusals that are its own.  No
// kernel lives here: the launchers are declared in gemm.h, norm.h and elementwise.h.
#pragma once
#include <cstring>
#include <initializer_list>

#include "../../include/difashion_hip.h"
#include "clip_tower.h"
#include "elementwise.h"
#include "gemm.h"
#include "norm.h"

namespace dfh {

// a refusal stated once and made on behalf of `who`, the function whose name the message carries (as DFH_REQUIRE's does)
inline int half_refuse(const char* who, const std::string& msg) { set_error(std::string(who) + ": " + msg); return -1; }

constexpr size_t HALF_ALIGN = 256;                           // of every workspace region and every matrix of the packed copy
inline size_t half_round_up(size_t n) { return (n + HALF_ALIGN - 1) / HALF_ALIGN * HALF_ALIGN; }
inline int half_act(int hidden_act) { return hidden_act == CLIP_ACT_GELU ? ACT_GELU : ACT_QUICK_GELU; }

// one plain-segment linear of the walk as the GEMM launcher takes it (pointers filled in by the walk; null in the plan)
inline GemmArgs half_linear_args(const dfh_clipvh_launch& l) {
  GemmArgs g;
  std::memset(&g, 0, sizeof(g));
  g.nplain = 1; g.p_c[0] = l.K; g.ldw = l.ldw; g.M = l.M; g.N = l.N; g.act = l.act;
  g.ld_out = l.ld_out; g.ld_res = l.ld_out; g.out_mode = OUT_BF16; g.rows_per_b = l.rows_per_b;
  g.n_split = l.n_split; g.ld_out2 = l.ld_out2;
  return g;
}

// packed copy, per layer: wqkv [3 D][D], wo [D][D], w1 [I][D], w2 [D][I] (16-bit) and bqkv [3 D] (fp32); offsets from the layer's base
struct HalfLayerPack {
  int D, I;
  size_t wqkv, wo, w1, w2, bqkv, per_layer;
  HalfLayerPack(int D_, int I_) : D(D_), I(I_) {
    wqkv = 0; wo = wqkv + half_round_up((size_t)3 * D * D * 2); w1 = wo + half_round_up((size_t)D * D * 2); w2 = w1 + half_round_up((size_t)I * D * 2);
    bqkv = w2 + half_round_up((size_t)D * I * 2); per_layer = bqkv + half_round_up((size_t)3 * D * 4);
  }
};

// writes the packed copy of every layer from the fp32 masters P; layer l begins at first_layer + l * lay.per_layer
inline int pack_encoder_layers(const float* const* P, const std::vector<ClipLayer>& layers, const HalfLayerPack& lay, unsigned char* first_layer,
                               hipStream_t s) {
  const int D = lay.D, I = lay.I;
  for (size_t l = 0; l < layers.size(); ++l) {
    const ClipLayer& L = layers[l];
    unsigned char* lb = first_layer + l * lay.per_layer;
    bf16_t* wqkv = (bf16_t*)(lb + lay.wqkv);
    float* bqkv = (float*)(lb + lay.bqkv);
    const int w3[3] = {L.qw, L.kw, L.vw}, b3[3] = {L.qb, L.kb, L.vb};
    for (int j = 0; j < 3; ++j) {
      if (int rc = pack_matrix_launch(P[w3[j]], wqkv, D, D, D, j * D, 0, 0, s)) return rc;
      if (int rc = pack_vector_launch(P[b3[j]], bqkv, D, j * D, 0, 0, s)) return rc;
    }
    if (int rc = pack_matrix_launch(P[L.ow], (bf16_t*)(lb + lay.wo), D, D, D, 0, 0, 0, s)) return rc;
    if (int rc = pack_matrix_launch(P[L.f1w], (bf16_t*)(lb + lay.w1), I, D, D, 0, 0, 0, s)) return rc;
    if (int rc = pack_matrix_launch(P[L.f2w], (bf16_t*)(lb + lay.w2), D, I, I, 0, 0, 0, s)) return rc;
  }
  return 0;
}

// What a plan function fills its public struct through.  Plan: dfh_clipvh_plan_info / dfh_cliph_plan_info (launches[], regions[], their
// counts, workspace_bytes and the common scalars).  who: the plan function.  Launches and regions are recorded in the order of their ids.
template <class Plan>
struct HalfPlanRecorder {
  Plan* p;
  const char* who;
  size_t off = 0;                                            // of the next workspace region

  int open(const void* ctx, int batch) {                     // the first refusals of either plan; leaves *p zeroed
    if (!(ctx && p)) return half_refuse(who, "null argument");
    std::memset(p, 0, sizeof(*p));
    return batch > 0 && batch <= 65535 ? 0 : half_refuse(who, "batch must be in [1, 65535]");
  }
  int offsets_fit(int batch, int T, int D, int I) const {    // the last refusal by size of either plan
    return (double)batch * T * (3.0 * D > I ? 3.0 * D : I) < 2.0e9 ? 0 : half_refuse(who, "batch x tokens x width beyond 32-bit element offsets");
  }
  void scalars(int batch, int T, int D, int I, int H, int layers) {
    p->batch = batch; p->tokens = T; p->hidden = D; p->intermediate = I; p->heads = H; p->head_dim = D / H; p->layers = layers;
    p->rows = batch * T;
  }
  dfh_clipvh_launch& launch(int id, const char* name, int M, int N, int K, int ld_out, int act, int resid, int per_layer, int a_reg, int out_reg) {
    dfh_clipvh_launch& l = p->launches[id];
    std::strncpy(l.name, name, sizeof(l.name) - 1);
    l.M = M; l.N = N; l.K = K; l.lda = K; l.ldw = K; l.ld_out = ld_out; l.rows_per_b = M; l.act = act; l.resid = resid;
    l.per_layer = per_layer; l.a_region = a_reg; l.out_region = out_reg; l.out2_region = -1;
    p->num_launches = id + 1;
    return l;
  }
  // split-K slabs of the launches that follow the heuristics: the largest need among `ids`
  size_t partial_floats(std::initializer_list<int> ids) const {
    size_t partial = 0;
    for (int id : ids) {
      GemmArgs a = half_linear_args(p->launches[id]);
      if (p->launches[id].resid) a.resid = (const bf16_t*)p;           // presence only
      const size_t f = gemm_partial_floats(a);
      partial = f > partial ? f : partial;
    }
    return partial;
  }
  void region(int id, const char* name, size_t bytes) {
    dfh_clipvh_region& r = p->regions[id];
    std::strncpy(r.name, name, sizeof(r.name) - 1);
    r.offset = off; r.bytes = bytes;
    off += half_round_up(bytes);
    p->num_regions = id + 1; p->workspace_bytes = off;                 // the caller hands in a 256-byte aligned block
  }
};

// One encode's view of its plan: the workspace regions, the packed copy and the GEMM launches.  zero_region / partial_region: the
// tower's region ids of the zero page and the split-K slabs.
template <class Plan>
struct HalfWalk {
  unsigned char* ws;
  const unsigned char* pk;
  const Plan& p;
  hipStream_t s;
  int zero_region, partial_region;

  unsigned char* reg(int id) const { return ws + p.regions[id].offset; }
  // what an encode requires of the two blocks it is handed.  size_query: the family's workspace size query
  int check_buffers(const char* who, const char* size_query, size_t workspace_bytes) const {
    if (workspace_bytes < p.workspace_bytes) return half_refuse(who, std::string("workspace smaller than ") + size_query);
    return (((uintptr_t)ws | (uintptr_t)pk) & 255) == 0 ? 0 : half_refuse(who, "workspace / packed copy must be 256-byte aligned");
  }
  int clear_zero_page(const char* entry) const {
    if (hipMemsetAsync(reg(zero_region), 0, 256, s) == hipSuccess) return 0;
    set_error(std::string(entry) + ": memset failed");
    return -2;
  }
  // one GEMM launch of the plan: A rows and the output are regions of the workspace, W a matrix of the packed copy
  int linear(int id, const void* W, const float* bias) const {
    const dfh_clipvh_launch& l = p.launches[id];
    GemmArgs a = half_linear_args(l);
    a.p_src[0] = (const bf16_t*)reg(l.a_region); a.W = (const bf16_t*)W; a.bias = bias; a.zero = (const bf16_t*)reg(zero_region);
    a.out = reg(l.out_region); a.partial = (float*)reg(partial_region);
    if (l.resid) a.resid = (const bf16_t*)reg(l.out_region);
    if (l.out2_region >= 0) a.out2 = reg(l.out2_region);
    // the second destination and the activation epilogues are single-pass launches: no K split
    const int force_split = (l.out2_region >= 0 || gemm_act_is_xact(l.act)) ? 1 : 0;
    return gemm_launch(a, s, 0, force_split);
  }
};

// The pre-LN blocks over the 16-bit stream, in place.  The plan holds a block's four launches from id `qkv` on (qkv, out_proj, fc1,
// fc2) and names their regions: the stream is what out_proj adds to, the LayerNorm output what the q | k | v launch reads.  P: the
// master parameters; layer l's matrices begin at first_layer + l * lay.per_layer; attention() launches the tower's attention from the
// q | k | v launch's output into out_proj's input; tap(l) receives the output of block l - 1 (hidden_states[l]).
template <class Plan, class Attention, class Tap>
int half_blocks(const HalfWalk<Plan>& w, int qkv, const float* const* P, const std::vector<ClipLayer>& layers, const HalfLayerPack& lay,
                const unsigned char* first_layer, float eps, Attention attention, Tap tap) {
  const int out = qkv + 1, fc1 = qkv + 2, fc2 = qkv + 3, M = w.p.rows, D = w.p.hidden;
  bf16_t* x = (bf16_t*)w.reg(w.p.launches[out].out_region);
  bf16_t* ln = (bf16_t*)w.reg(w.p.launches[qkv].a_region);
  for (size_t l = 0; l < layers.size(); ++l) {
    const ClipLayer& L = layers[l];
    const unsigned char* lb = first_layer + l * lay.per_layer;
    if (int rc = layernorm_launch(x, P[L.ln1w], P[L.ln1b], ln, M, D, eps, w.s)) return rc;
    if (int rc = w.linear(qkv, lb + lay.wqkv, (const float*)(lb + lay.bqkv))) return rc;
    if (int rc = attention()) return rc;
    if (int rc = w.linear(out, lb + lay.wo, P[L.ob])) return rc;                    // x += out_proj(attention)
    if (int rc = layernorm_launch(x, P[L.ln2w], P[L.ln2b], ln, M, D, eps, w.s)) return rc;
    if (int rc = w.linear(fc1, lb + lay.w1, P[L.f1b])) return rc;
    if (int rc = w.linear(fc2, lb + lay.w2, P[L.f2b])) return rc;                   // x += fc2(act(fc1(.)))
    if (int rc = tap((int)l + 1)) return rc;
  }
  return 0;
}

}  // namespace dfh

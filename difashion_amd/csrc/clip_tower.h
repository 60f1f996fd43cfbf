// Host side of what the two CLIP towers (clip.hip: text, clip_vision.hip: image) share: the parameter table, the encoder layer, the
// workspace layout and the walk over the pre-LN blocks.  Each tower keeps its embeddings, its attention kernel, what follows the last
// block and its config checks.  No kernel lives here: the shared launchers are declared in clip_kernels.h.
#pragma once
#include "clip_kernels.h"
#include "dfh_common.h"

namespace dfh {

// what an encode entry point requires of master_params (dfh_common.h require_params).  family: "dfh_clip" / "dfh_clipv"
inline int require_params(const ParamList& t, const float* const* master_params, int count, const std::string& family) {
  return require_params(t, master_params, count, family + "_encode", family + "_num_params", "master_params");
}

// table indices of one CLIPEncoderLayer
struct ClipLayer { int kw, kb, vw, vb, qw, qb, ow, ob, ln1w, ln1b, f1w, f1b, f2w, f2b, ln2w, ln2b; };

// registers <prefix>encoder.layers.<l>.* for l < L in transformers' state-dict order
inline std::vector<ClipLayer> add_encoder_layers(ParamList& t, const std::string& prefix, int L, int D, int I) {
  std::vector<ClipLayer> layers(L);
  for (int l = 0; l < L; ++l) {
    const std::string p = prefix + "encoder.layers." + std::to_string(l) + ".";
    ClipLayer& y = layers[l];
    y.kw = t.add_param(p + "self_attn.k_proj.weight", {D, D}); y.kb = t.add_param(p + "self_attn.k_proj.bias", {D});
    y.vw = t.add_param(p + "self_attn.v_proj.weight", {D, D}); y.vb = t.add_param(p + "self_attn.v_proj.bias", {D});
    y.qw = t.add_param(p + "self_attn.q_proj.weight", {D, D}); y.qb = t.add_param(p + "self_attn.q_proj.bias", {D});
    y.ow = t.add_param(p + "self_attn.out_proj.weight", {D, D}); y.ob = t.add_param(p + "self_attn.out_proj.bias", {D});
    y.ln1w = t.add_param(p + "layer_norm1.weight", {D}); y.ln1b = t.add_param(p + "layer_norm1.bias", {D});
    y.f1w = t.add_param(p + "mlp.fc1.weight", {I, D}); y.f1b = t.add_param(p + "mlp.fc1.bias", {I});
    y.f2w = t.add_param(p + "mlp.fc2.weight", {D, I}); y.f2b = t.add_param(p + "mlp.fc2.bias", {D});
    y.ln2w = t.add_param(p + "layer_norm2.weight", {D}); y.ln2b = t.add_param(p + "layer_norm2.bias", {D});
  }
  return layers;
}

// Workspace of an encode over M rows: x | ln | q k v (qkv_width floats a row) | attention | MLP hidden | tail, + 64 floats of slack.
struct ClipWorkspace : WorkspaceCarve {
  float *x, *ln, *qkv, *att, *hid, *tail;
  ClipWorkspace(void* base, size_t M, size_t D, size_t I, size_t qkv_width, size_t tail_floats) : WorkspaceCarve(base, 1) {
    x = take(M * D); ln = take(M * D); qkv = take(M * qkv_width); att = take(M * D); hid = take(M * I); tail = take(tail_floats);
    take(64);                                                    // the slack
  }
};

// How a tower's launches are accounted: the ProfClass of its linears / LayerNorms (< 0: not timed), the census counters they bump (< 0: none)
struct ClipAccounting { int linear_class, linear_census, lnorm_class, lnorm_census; };

inline int tower_linear(const ClipAccounting& a, const float* A, int lda, const float* W, int K, const float* bias, const float* resid,
                        float* out, int ld_out, int M, int N, int act, hipStream_t s) {
  if (a.linear_census >= 0) census(a.linear_census);
  return clip_linear(A, lda, W, K, bias, resid, resid ? ld_out : 0, out, ld_out, M, N, act, a.linear_class, s);
}
inline int tower_layernorm(const ClipAccounting& a, const float* x, long ldx, const float* g, const float* b, float* y, int M, int D, float eps,
                           hipStream_t s) {
  if (a.lnorm_class < 0) return clip_layernorm(x, ldx, g, b, y, M, D, eps, s);
  ProfScope ps(a.lnorm_class, 8.0 * M * D, 8.0 * M * D, s);
  if (a.lnorm_census >= 0) census(a.lnorm_census);
  return clip_layernorm(x, ldx, g, b, y, M, D, eps, s);
}

// a hidden_states / last_hidden_state copy out of the workspace; dst may be null (not asked for).  what: "<entry point>: <tensor>"
inline int tower_copy(float* dst, const float* src, size_t bytes, hipStream_t s, const char* what) {
  if (!dst || hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, s) == hipSuccess) return 0;
  set_error(std::string(what) + " copy failed");
  return -2;
}

// The pre-LN blocks over w.x [M][D], in place.  P: the master parameters; attention(qkv, out) launches the tower's attention over
// w.qkv [M][3 D] (q | k | v) into w.att; tap(l, x) receives the output of block l - 1 (hidden_states[l]).
template <class Attention, class Tap>
int clip_blocks(const float* const* P, const std::vector<ClipLayer>& layers, const ClipWorkspace& w, int M, int D, int I, int act, float eps,
                const ClipAccounting& a, hipStream_t s, Attention attention, Tap tap) {
  for (size_t l = 0; l < layers.size(); ++l) {
    const ClipLayer& L = layers[l];
    if (int rc = tower_layernorm(a, w.x, D, P[L.ln1w], P[L.ln1b], w.ln, M, D, eps, s)) return rc;
    if (int rc = tower_linear(a, w.ln, D, P[L.qw], D, P[L.qb], nullptr, w.qkv, 3 * D, M, D, CLIP_ACT_NONE, s)) return rc;
    if (int rc = tower_linear(a, w.ln, D, P[L.kw], D, P[L.kb], nullptr, w.qkv + D, 3 * D, M, D, CLIP_ACT_NONE, s)) return rc;
    if (int rc = tower_linear(a, w.ln, D, P[L.vw], D, P[L.vb], nullptr, w.qkv + 2 * D, 3 * D, M, D, CLIP_ACT_NONE, s)) return rc;
    if (int rc = attention(w.qkv, w.att)) return rc;
    if (int rc = tower_linear(a, w.att, D, P[L.ow], D, P[L.ob], w.x, w.x, D, M, D, CLIP_ACT_NONE, s)) return rc;      // x += out_proj(attention)
    if (int rc = tower_layernorm(a, w.x, D, P[L.ln2w], P[L.ln2b], w.ln, M, D, eps, s)) return rc;
    if (int rc = tower_linear(a, w.ln, D, P[L.f1w], D, P[L.f1b], nullptr, w.hid, I, M, I, act, s)) return rc;
    if (int rc = tower_linear(a, w.hid, I, P[L.f2w], I, P[L.f2b], w.x, w.x, D, M, D, CLIP_ACT_NONE, s)) return rc;    // x += fc2(act(fc1(.)))
    if (int rc = tap((int)l + 1, w.x)) return rc;
  }
  return 0;
}

}  // namespace dfh

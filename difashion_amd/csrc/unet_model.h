// The U-Net runtime object: its layer records and struct dfh_unet with its data and the declarations of what works on it.  The bodies:
// unet_build.hip (layers, packing plans, fp8 and training layouts), unet_derive.hip (packing, fp8 copies, folds), unet_walk.hip (the
// inference walk and the run cache), unet_train.hip (training forward / backward), unet.hip (C ABI).  The parameter table, the workspace
// layout and the launch context it shares with the VAE and the training walk live in walk_common.h.
#pragma once
#include <map>

#include "walk_common.h"
#include "gemm_plan.h"
#include "walk_knobs.h"
#include "elementwise.h"
#include "mlp_fused.h"
#ifdef DFH_PROBES
#include "token_linear.h"
#endif
#include "bwd_elementwise.h"

namespace dfhm {

// transposed pack (training): master weight -> arena16t, see bwd_elementwise.hip pack_*_t kernels
struct TPackOp { int param, conv; size_t dst; int N, K, ldt, t_row_off, t_col_off, geglu, o_pad; };
inline void OpTable::add(void* src, const TPackOp& op) {
  if (op.conv) add(src, TAB_PACKT_CONV, (long)op.dst, op.N, op.K, op.ldt, 0, op.t_col_off, 0, op.o_pad, (long)op.N * op.K * 9);
  else add(src, TAB_PACKT_MAT, (long)op.dst, op.N, op.K, op.ldt, op.t_row_off, op.t_col_off, op.geglu, 0, (long)op.N * op.K);
}

// fp8 [N][K] at arena8 + off, per-row scales (floats) at arena8 + soff; boff: a derived bias (floats) for the matrices that fold a norm's
// affine into themselves (proj_in), else unused
struct Mat8 { size_t off = 0, soff = 0, boff = 0; int N = 0, K = 0; bool on = false; };

struct ResL {
  int cin = 0, cout = 0, temb_off = 0; bool shortcut = false;
  int p_tw = -1, p_tb = -1;             // parameter indices of time_emb_proj.weight / .bias (rows of the batched matrix: packed at the end of build())
  Vec n1w, n1b, b1, n2w, n2b, b2; Mat w1, w2;
  std::string pre; Mat w1t, w2t, wst;   // training: transposed packs for the data-gradient GEMMs
  // Winograd F(2x2, 3x3) weights U [16][cout][cin] of conv1 / conv2 in the fold region (winograd.hip), allocated for the deep levels
  size_t u1 = 0, u2 = 0; bool has_u = false;
};
// A LayerNorm-fed projection with the LayerNorm folded in (lnfold.hip): W' (bf16 elements) / s / b' (floats) offsets inside the fold
// region at the head of the workspace
struct Fold { size_t w = 0, s = 0, b = 0; int N = 0, K = 0; };

struct AttL {
  int C = 0, heads = 0, x_off = 0;   // x_off: this layer's row offset in the batched cross K / V matrices
  int idx = 0;                       // position in walk order (the per-layer slots of the fp8 path's V maxima)
  int p_k2 = -1, p_v2 = -1;          // parameter indices of attn2.to_k / to_v (rows of the batched text K / V matrices)
  Fold fqkv, fqk, fv, fq2, fff1;
  // ff.net.2 and proj_out folded into ONE linear over [GEGLU output | h2] (inference walk): W = [pout . ff2 | pout] ([C][5C]), bias =
  // pout . ff2b + poutb -- proj_out(ff2(f) + ff2b + h2) + poutb as written, minus one launch, one bf16 rounding and one round trip
  // of a [tokens][C] tensor per transformer block
  Fold fffp;
  // C = 320 (the 64x64 level): the whole feed-forward + proj_out as ONE kernel (mlp_fused2.hip); its weight image (fragment-major LDS
  // image of fff1 and fffp, 2.7 MB) in the fold region
  size_t mlp_img = 0; bool has_mlp = false;
  // ... and its four K = N = C projections (proj_in, attn1.to_out, attn2.to_q folded, attn2.to_out) as register-resident token linears
  // (mlp_fused2.hip token_linear_kernel): their weight images in the fold region
  size_t tl_pin = 0, tl_o1 = 0, tl_q2 = 0, tl_o2 = 0; bool has_tl = false;
  Vec nw, nb, pinb, l1w, l1b, o1b, l2w, l2b, o2b, l3w, l3b, ff1b, ff2b, poutb;
  Mat pin, qk, v, o1, q2, o2, ff1, ff2, pout;
  std::string pre; Mat pint, qkvt, o1t, q2t, o2t, ff1t, ff2t, poutt;
  Mat8 qk8, v8, q28, ff18;           // fp8 copies of the LayerNorm-fed projections (gemm_fp8.hip), when enabled
  // round 4 (BASELINE configs[4] as named: "attention + 1x1-conv path"): to_out of both attentions, ff.net.2, proj_out, and proj_in with
  // the GroupNorm affine folded in (W . diag(gamma), bias + W . beta: the GroupNorm kernel then emits the normalised value as e4m3)
  Mat8 o18, o28, ff28, pout8, pin8;
  // fp8 attention products (attention_fp8.hip): operand factors rq | rk | rv ([C] each) and the per-head softmax factor ([heads]) as
  // floats at arena8 + f8a_off, derived from the LayerNorm-folded q | k | v weights at pack time; f8a: allocated for this layer
  size_t f8a_off = 0; bool f8a = false;
};
struct ConvL {
  Mat w; Vec b; int cin = 0, cout = 0; std::string pre; Mat wt;
  // upsamplers: summed phase weights [4][cout][4 * cin] in the fold region (gemm.h GemmArgs::phase2x), has_ph when allocated
  size_t ph = 0; bool has_ph = false;
};

}  // namespace dfhm
using namespace dfhm;


struct dfh_unet : ParamTable {
  dfh_unet_config cfg{};
  // layers
  ConvL conv_in, conv_out;
  Mat te1, te2, tproj, kx_all, vx_all; Vec te1b, te2b, tprojb, cnw, cnb;
  int temb_total = 0, x_total = 0;   // x_total: sum of C over all transformer layers (batched text K/V)
  // folded-LayerNorm copies of the LayerNorm-fed projections (derived data, re-made by every pack): they live at the head of the
  // WORKSPACE, not in arena16 / arena32 -- the training path sizes its gradient arenas and its all-reduce by those
  size_t fold16 = 0, fold32 = 0; bool fold_valid = false, fold_dirty = false;
  size_t fold_bytes() const { return ((fold16 * 2 + 255) & ~(size_t)255) + ((fold32 * 4 + 255) & ~(size_t)255); }
  bf16_t* fold_w() const { return (bf16_t*)ws; }
  float* fold_v() const { return (float*)(ws + ((fold16 * 2 + 255) & ~(size_t)255)); }
  Fold fold_alloc(int N, int K);
  std::vector<std::vector<ResL>> down_res, up_res;
  std::vector<std::vector<AttL>> down_att, up_att;
  std::vector<ConvL> down_samp, up_samp;
  ResL mid_res[2]; AttL mid_att;
  // every resnet / transformer layer in walk order (down blocks, mid, up blocks): filled once at the end of build(), what "all layers" means
  std::vector<ResL*> ress; std::vector<AttL*> atts;
  // bound memory (the arenas: ParamTable)
  char* ws = nullptr; size_t ws_bytes = 0; int max_batch = 0;
  // the workspace behind the fold region as the last dry walk planned it
  WorkspacePlan plan;
  size_t plan_total() const { return fold_bytes() + plan.total(); }
  size_t walk_bytes() const { return ws_bytes > fold_bytes() ? ws_bytes - fold_bytes() : 0; }      // what the walk may lay out at ws + fold_bytes()
  // fp8 linears (BASELINE configs[4]): e4m3 copies of qk / v / q2 / ff1 + per-row scales, in one caller-owned arena
  bool fp8 = false; unsigned char* arena8 = nullptr; size_t a8 = 0;
  // fp8 walk: also the self-attention products QK^T / PV on the e4m3 MFMA (attention_fp8.hip).  OFF by default: built, parity-tested and
  // measured slower than the bf16 kernels at every head dim of this model (profiles/r04/attn_fp8_microbench.txt)
  bool fp8_attention = false;
  // taps of the last forward
  std::map<std::string, Tensor> taps; int last_batch = 0;
  int dup_tail = 0;          // one-shot hint for the next forward (dfh_unet_set_dup_tail): trailing images that repeat the inputs of the ones before them
  // ---- training state (unet_train.hip)
  std::vector<TPackOp> tpacks; size_t a16t = 0; bool train_built = false;
  Mat te2t, tprojt;
  bf16_t* arena16t = nullptr; float* grad16 = nullptr; float* grad32 = nullptr;   // grad16/32: fp32, packed layouts of arena16/32
  char* tws = nullptr; size_t tws_bytes = 0; int train_max_batch = 0;
  struct TrainRun; TrainRun* tr = nullptr;
  // gradient checkpointing of the training walk (dfh_unet_set_checkpointing): 0 off, 1 recompute the internals of every resnet /
  // transformer layer in the backward, 2 the same but the attention outputs are kept.  Read when a step begins (TrainRun) and by plan_train
  int ckpt = 0;
  // backward walk: the weight-gradient GEMM of a layer runs on a second stream beside the data-gradient GEMM of the same layer
  // (both only read dY): the tail round of one is filled with blocks of the other (unet_train.hip TrainRun::wgrad / join)
  hipStream_t side_stream = nullptr; hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  // dfh_unet_grad_sumsq: the un-pack of the backward also leaves the sum of the squares of every gradient value it wrote in *grad_sumsq_out
  // (the clip norm of the optimizer without another pass over 3.4 GB); per-block partials + a fixed-order reduce, no float atomics
  float* grad_sumsq_out = nullptr; float* sq_partials = nullptr; size_t sq_cap = 0; float* sq_scratch = nullptr;
  int build_train();                           // unet_build.hip
  WorkspacePlan plan_train(int B);             // the training workspace is its total() + 256
  int forward_train(const void* sample, int sample_bf16, const float* timestep, const void* ehs, int ehs_bf16, float* out, int B,
                    hipStream_t s);
  int backward(const float* d_out, float* d_sample, float* const* master_grads, int count, hipStream_t s, int overwrite);
  // the same backward in pieces, for a data-parallel caller that all-reduces finished ranges of grad16 while the walk goes on
  int backward_begin(const float* d_out, float* d_sample, size_t bucket_floats, hipStream_t s);
  int backward_next(size_t* lo, size_t* hi, hipStream_t s);             // 1: grad16[lo, hi) is final; 0: tape done; < 0: error
  int backward_finish(float* const* master_grads, int count, hipStream_t s, int overwrite);
  ~dfh_unet();

  // ---------------------------------------------------------------- build (unet_build.hip)
  // largest image (pixels) whose wide resnet convs take Winograd: 256 = the 16x16 level (default); DFH_WINO_MAXHW=1024 adds the 32x32 level
  // (the A/B of profiles/r04: measured, not the default)
  static int wino_max_hw() { return dfh::WalkKnobs::get().wino_maxhw; }
  void build_resnet(const std::string& pre, int cin, int cout, ResL& r, int res);      // res: side of the (square) image this resnet runs on
  void build_attn(const std::string& pre, int C, int heads, AttL& a);
  void build_conv(const std::string& pre, int cout, int cin, ConvL& c);
  int build();

  // ---------------------------------------------------------------- fp8
  static constexpr float GN_Z = 32.0f;   // |normalised GroupNorm value| representable in the e4m3 proj_in operand (static scale 448 / GN_Z)
  size_t a8_slab_off = 0; int n_att = 0; std::vector<int> slab_host;
  int enable_fp8();                            // unet_build.hip
  const int* slab_row0() const { return (const int*)(arena8 + a8_slab_off); }
  const int* slab_rows() const { return slab_row0() + n_att; }

  // ---------------------------------------------------------------- derived weights (unet_derive.hip)
  OpTable tab_packt, tab_unpack, tab_pack2;
  int pack(const float* const* master, int count, hipStream_t s);
  int pack_train(const float* const* master, int count, hipStream_t s);
  int pack_all(const float* const* master, int count, hipStream_t s);      // training: pack() + pack_train() with one read of the weights
  int quantize_fp8(hipStream_t s);
  // W' / s / b' of every LayerNorm-fed projection from the freshly packed bf16 matrices (needs the workspace: after dfh_unet_bind)
  int fold_layernorms(hipStream_t s);

  // ---------------------------------------------------------------- run (unet_walk.hip)
  struct Run;
  // Per-run constants of a sampling loop (reference DiFashion/models/difashion.py:340-357: the prompt states are fixed for the run;
  // :456: the timesteps are the schedule's): the cross-attention K / V^T of every transformer block and the time-embedding rows
  // (all time_emb_proj outputs) per schedule entry, computed once by run_cache() into a caller-owned buffer.
  struct RunCache { const bf16_t* kx = nullptr; const bf16_t* vxt = nullptr; const float* temb_row = nullptr; const float* xamax = nullptr; };
  // fp8 walk: the largest |V| of every layer's cross-attention per batch element, [n_att][B] floats behind the time-embedding table
  size_t cache_xamax_bytes(int B) const { return fp8 ? (((size_t)n_att * B * 4 + 255) & ~(size_t)255) : 0; }
  static size_t cache_kx_bytes(const dfh_unet& u, int B) { return ((size_t)B * u.cfg.text_len * u.x_total * 2 + 255) & ~(size_t)255; }
  static size_t cache_vxt_bytes(const dfh_unet& u, int B) { return ((size_t)B * u.x_total * ((u.cfg.text_len + 7) & ~7) * 2 + 255) & ~(size_t)255; }
  size_t run_cache_bytes(int B, int n_t) const {
    return cache_kx_bytes(*this, B) + cache_vxt_bytes(*this, B) + (((size_t)n_t * temb_total * 4 + 255) & ~(size_t)255) + cache_xamax_bytes(B);
  }
  int cross_amax(const bf16_t* vxt, int B, float* out, hipStream_t s);     // amax_cross[layer][b] = max |V^T| of the layer's slice of the batched text V^T
  int run(const void* sample, int sample_bf16, const float* timestep, const void* ehs, int ehs_bf16, float* out, int B,
          hipStream_t s, bool dry, const RunCache* rcache = nullptr);
  // Fills a run cache (layout: kx | vxt | temb table [n_t][temb_total] fp32).  Uses the bound workspace as scratch, in chunks of the
  // planned batch so that every launch has a shape the workspace plan covered (split-K slabs included).
  int run_cache(const void* ehs, int ehs_bf16, int B, const float* timesteps, int n_t, void* cache, hipStream_t s);
};

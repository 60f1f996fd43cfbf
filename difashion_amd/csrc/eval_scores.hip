// Embedding-side metrics of the reference's evaluation: what it computes from the CLIP embeddings after
// encode_image / encode_text.
//
// Replaces (arithmetic):
//   * 100 * F.cosine_similarity of normalised rows -- CLIP score, CLIP image score (Evaluation/eval_utils.py:101-135) and the
//     personalisation similarity (:503-538): dfh_embed_pair_cosine;
//   * the retrieval of :652-723 (5 candidates a row): cosine against gathered table rows + argmax: dfh_embed_candidates (the ranking of
//     a whole category per row, :725-767, is eval_rank.hip);
//   * FashionEvaluator (Evaluation/compatibility_evaluator/compatibility_net.py:14-81) under the gather of
//     CompatibilityEvaluator.evaluate_compatibility (eval_utils.py:574-588): dfh_compat_score.  The reference runs one outfit at a
//     time in a Python loop; here all outfits of a call go through every layer together.
//
// fp32 in both storage builds.  The Linears run on the fp32 matrix instruction in the CLIP towers' tile with a compensated accumulation
// over the k-tiles (compat_gemm_f32_kernel below).
// No atomics anywhere: reruns are bit-identical and a row's result does not depend on the batch it rides in.
#include <cmath>

#include "../../include/difashion_hip.h"
#include "clip_kernels.h"
#include "f32_tile.h"

namespace {

// <a, b>, <a, a>, <b, b> of one row pair over the 64 lanes of a wave: per lane a run of dim / 64 fused multiply-adds, then the wave tree
DFH_DEVICE void wave_dot3(const float* __restrict__ a, const float* __restrict__ b, int dim, bool vec, int lane, float& ab, float& aa,
                          float& bb) {
  float sab = 0.f, saa = 0.f, sbb = 0.f;
  if (vec) {
    const float4* a4 = (const float4*)a;
    const float4* b4 = (const float4*)b;
    for (int c = lane; c < dim / 4; c += 64) {
      const float4 u = a4[c], v = b4[c];
      sab = fmaf(u.x, v.x, sab); sab = fmaf(u.y, v.y, sab); sab = fmaf(u.z, v.z, sab); sab = fmaf(u.w, v.w, sab);
      saa = fmaf(u.x, u.x, saa); saa = fmaf(u.y, u.y, saa); saa = fmaf(u.z, u.z, saa); saa = fmaf(u.w, u.w, saa);
      sbb = fmaf(v.x, v.x, sbb); sbb = fmaf(v.y, v.y, sbb); sbb = fmaf(v.z, v.z, sbb); sbb = fmaf(v.w, v.w, sbb);
    }
  } else {
    for (int c = lane; c < dim; c += 64) {
      const float u = a[c], v = b[c];
      sab = fmaf(u, v, sab); saa = fmaf(u, u, saa); sbb = fmaf(v, v, sbb);
    }
  }
  ab = wave_sum(sab); aa = wave_sum(saa); bb = wave_sum(sbb);
}

// one wave per row, four rows per workgroup.  vec: dim is a multiple of 4 and both bases are 16-byte aligned
__global__ __launch_bounds__(256) void embed_pair_cosine_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                float* __restrict__ out, int rows, int dim, float scale, int vec) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;                       // whole waves leave: the shuffles below see 64 live lanes
  float ab, aa, bb;
  wave_dot3(a + (long)row * dim, b + (long)row * dim, dim, vec != 0, lane, ab, aa, bb);
  if (lane == 0) out[row] = scale * (ab / (sqrtf(aa) * sqrtf(bb)));       // a zero row: 0 / 0 = NaN, as x / x.norm() gives
}

// torch.argmax order: a NaN is the maximum, the first of equals wins
DFH_DEVICE bool beats(float v, int k, float best, int bk) {
  const bool vn = v != v, bn = best != best;
  if (vn != bn) return vn;
  if (!vn && v != best) return v > best;
  return k < bk;
}

// one workgroup per generated row: wave w scores candidates w, w + 4, ...; every score is one wave's reduction, so sims do not depend
// on K or on the grid; the four waves' running maxima meet in LDS.
__global__ __launch_bounds__(256) void embed_candidates_kernel(const float* __restrict__ gen, const float* __restrict__ table,
                                                               const int64_t* __restrict__ cand, float* __restrict__ sims,
                                                               int64_t* __restrict__ pred, int K, int dim, int table_rows, int vec) {
  __shared__ float bestv[4];
  __shared__ int bestk[4];
  const int r = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* g = gen + (long)r * dim;
  float best = -INFINITY;
  int bk = 0x7fffffff;
  for (int k = wave; k < K; k += 4) {
    long id = cand[(long)r * K + k];
    id = id < 0 ? 0 : (id >= table_rows ? table_rows - 1 : id);          // the host side refuses out-of-range ids before the launch
    float ab, aa, bb;
    wave_dot3(g, table + id * (long)dim, dim, vec != 0, lane, ab, aa, bb);
    const float v = ab / (sqrtf(aa) * sqrtf(bb));
    if (lane == 0) sims[(long)r * K + k] = v;
    if (beats(v, k, best, bk)) { best = v; bk = k; }
  }
  if (lane == 0) { bestv[wave] = best; bestk[wave] = bk; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w)
      if (bestk[w] != 0x7fffffff && beats(bestv[w], bestk[w], best, bk)) { best = bestv[w]; bk = bestk[w]; }
    pred[r] = bk;
  }
}

// ------------------------------------------------------------------ compatibility scorer
// x[o * items + i] = id <= 0 ? feats_gen[-id] : feats_real[id]   (evaluate_compatibility's loop), ids clamped into their table
__global__ __launch_bounds__(256) void compat_gather_kernel(const float* __restrict__ real, int real_rows, const float* __restrict__ genf,
                                                            int gen_rows, const int64_t* __restrict__ olists, float* __restrict__ x, int dim) {
  const long id = olists[blockIdx.x];
  const float* src;
  if (id <= 0 && genf) {
    const long g = -id;
    src = genf + (g >= gen_rows ? gen_rows - 1 : g) * (long)dim;
  } else {
    src = real + (id < 0 ? 0 : (id >= real_rows ? real_rows - 1 : id)) * (long)dim;
  }
  const float4* s4 = (const float4*)src;
  float4* o = (float4*)(x + (long)blockIdx.x * dim);
  for (int c = threadIdx.x; c < dim / 4; c += 256) o[c] = s4[c];
}

// pairs[(o * npairs + p)] = [f[o][i_p] | f[o][j_p]], (i_p, j_p) the p-th of itertools.combinations(range(items), 2); F floats a row
__global__ __launch_bounds__(256) void compat_pairs_kernel(const float* __restrict__ f, float* __restrict__ pairs, int items, int npairs, int F) {
  const int o = blockIdx.x / npairs, p = blockIdx.x - o * npairs;
  int i = 0, rem = p;
  while (rem >= items - 1 - i) { rem -= items - 1 - i; ++i; }
  const int j = i + 1 + rem;
  const float4* fi = (const float4*)(f + ((long)o * items + i) * F);
  const float4* fj = (const float4*)(f + ((long)o * items + j) * F);
  float4* out = (float4*)(pairs + (long)blockIdx.x * 2 * F);
  for (int c = threadIdx.x; c < F / 4; c += 256) { out[c] = fi[c]; out[F / 4 + c] = fj[c]; }
}

// y = relu(LayerNorm(x) * g + b): the towers' one-wave-a-row LayerNorm (f32_tile.h layernorm_row) with the ReLU folded in
__global__ __launch_bounds__(256) void compat_ln_relu_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                             const float* __restrict__ b, float* __restrict__ y, int M, int D, float eps) {
  dfh::layernorm_row<true>(x, D, g, b, y, M, D, eps);
}

// outfit_emb[o][c] = mean over the outfit's pairs of e[o * npairs + p][c]  (torch.mean(relation_embs, dim=0))
__global__ __launch_bounds__(256) void compat_pair_mean_kernel(const float* __restrict__ e, float* __restrict__ out, int npairs, int D, long total) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const long o = t / D;
  const int c = (int)(t - o * D);
  float s = 0.f;
  for (int p = 0; p < npairs; ++p) s += e[(o * npairs + p) * D + c];
  out[t] = s / (float)npairs;
}

// logits[o] = <h[o], w> + bias (the Linear 32 -> 1), scores[o] = sigmoid(logits[o]); one thread per outfit
__global__ __launch_bounds__(256) void compat_tail_kernel(const float* __restrict__ h, const float* __restrict__ w, const float* __restrict__ bias,
                                                          float* __restrict__ logits, float* __restrict__ scores, int outfits, int D) {
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= outfits) return;
  float s = 0.f;
  for (int c = 0; c < D; ++c) s = fmaf(h[(long)o * D + c], w[c], s);
  s += bias[0];
  if (logits) logits[o] = s;
  if (scores) scores[o] = 1.0f / (1.0f + expf(-s));
}

// ------------------------------------------------------------------ the scorer's Linear: out[m][n] = sum_k A[m][k] W[n][k] + bias[n]
// The 64 x 64 tile of f32_tile.h (gemm_tile), the one the CLIP towers run, under the other summation policy: the towers' ChainSum runs
// ONE accumulator down all of K, a chain whose rounding error grows like sqrt(K); measured on an MI355X that put outfit_emb 3.9 x and
// the single-outfit logit 9 x beyond the real class's own fp32 distance from fp64 (K = 2048 in emb_layer.0; torch's CPU sgemm sums in
// blocks).  TileKahanSum sums every 32-wide k-tile on its own and adds the tile sums with a compensated (Kahan) add, so the error no
// longer grows with K.  Same operands, same products, another summation order.
using dfh::GT_M; using dfh::GT_N;

__global__ __launch_bounds__(256) void compat_gemm_f32_kernel(const float* __restrict__ A, int lda, const float* __restrict__ W, int ldw,
                                                              const float* __restrict__ bias, float* __restrict__ out, int ld_out, int M,
                                                              int N, int K) {
  dfh::gemm_tile<dfh::TileKahanSum>(A, lda, W, ldw, bias, M, N, K, [=](int m, int n, float acc) { out[(long)m * ld_out + n] = acc; });
}

// A [M][K] dense, W [N][K] (nn.Linear layout, read in place), K a multiple of 4, rows 16-byte aligned
int compat_linear(const float* A, const float* W, int K, const float* bias, float* out, int M, int N, hipStream_t s) {
  dfh::ProfScope ps(dfh::PC_OTHER, 2.0 * M * N * K, 4.0 * ((double)M * K + (double)N * K + (double)M * N), s);
  hipLaunchKernelGGL(compat_gemm_f32_kernel, dim3((N + GT_N - 1) / GT_N, (M + GT_M - 1) / GT_M), dim3(256), 0, s, A, K, W, K, bias, out, N, M, N, K);
  return dfh::check_launch("compat_gemm_f32_kernel");
}

// table indices of FashionEvaluator's state dict (compatibility_net.py:18-52): weight at the index, bias behind it
enum { CP_FEAT = 0, CP_EMB = 2, CP_EVAL = 18, CP_TAIL = 30 };
constexpr int FEAT = 1024, EMB = 256, TAIL_IN = 32;
constexpr int EMB_DIMS[5] = {2 * FEAT, 512, 512, 256, EMB};
constexpr int EVAL_DIMS[4] = {EMB, 128, 128, TAIL_IN};
constexpr float LN_EPS = 1e-5f;                   // nn.LayerNorm's default

// x | f | pairs | ping | pong | emb, every region a multiple of 64 floats
struct CompatWorkspace : dfh::WorkspaceCarve {
  float *x, *f, *pairs, *ping, *pong, *emb;
  CompatWorkspace(void* base, size_t outfits, size_t items, size_t dim) : dfh::WorkspaceCarve(base, 64) {
    const size_t R = outfits * items, P = outfits * (items * (items - 1) / 2);
    x = take(R * dim); f = take(R * FEAT); pairs = take(P * 2 * FEAT); ping = take(P * 512); pong = take(P * 512); emb = take(outfits * EMB);
  }
};

int check_params(const float* const* params, int count, const char* who) {
  auto refuse = [&](const std::string& msg) { dfh::set_error(std::string(who) + ": " + msg); return -1; };
  if (!params) return refuse("null argument");
  if (count != DFH_COMPAT_NUM_PARAMS) return refuse("params count must be DFH_COMPAT_NUM_PARAMS (32)");
  return dfh::check_param_pointers(params, count, who, [](int i) { return " at index " + std::to_string(i); });
}

// n x (Linear, LayerNorm, ReLU) over M rows: dims[l] -> dims[l + 1], parameters from index p0 (weight, bias, ln weight, ln bias a layer).
// The Linear writes ping, the fused LayerNorm + ReLU writes pong, which the next Linear reads: in is left alone, the result is in pong
const float* mlp_stack(const float* const* P, int p0, const int* dims, int n, const float* in, float* ping, float* pong, int M,
                       hipStream_t s, int& rc) {
  const float* cur = in;
  for (int l = 0; l < n; ++l) {
    const int K = dims[l], N = dims[l + 1];
    if ((rc = compat_linear(cur, P[p0 + 4 * l], K, P[p0 + 4 * l + 1], ping, M, N, s))) return nullptr;
    hipLaunchKernelGGL(compat_ln_relu_kernel, dim3((M + 3) / 4), dim3(256), 0, s, ping, P[p0 + 4 * l + 2], P[p0 + 4 * l + 3], pong, M, N, LN_EPS);
    if ((rc = dfh::check_launch("compat_ln_relu_kernel"))) return nullptr;
    cur = pong;
  }
  return cur;
}

int pred_score(const float* const* P, const float* emb, int outfits, float* logits, float* scores, float* ping, float* pong, hipStream_t s) {
  int rc = 0;
  const float* h = mlp_stack(P, CP_EVAL, EVAL_DIMS, 3, emb, ping, pong, outfits, s, rc);
  if (!h) return rc;
  hipLaunchKernelGGL(compat_tail_kernel, dim3((outfits + 255) / 256), dim3(256), 0, s, h, P[CP_TAIL], P[CP_TAIL + 1], logits, scores, outfits, TAIL_IN);
  return dfh::check_launch("compat_tail_kernel");
}

bool vec_ok(int dim, const void* a, const void* b) { return dim % 4 == 0 && (((uintptr_t)a | (uintptr_t)b) & 15) == 0; }

}  // namespace

extern "C" {

int dfh_embed_pair_cosine(const float* a, const float* b, float* out, int rows, int dim, float scale, void* stream) {
  DFH_REQUIRE(a && b && out, "null argument");
  DFH_REQUIRE(rows > 0 && dim > 0, "rows / dim must be positive");
  hipLaunchKernelGGL(embed_pair_cosine_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, a, b, out, rows, dim, scale,
                     vec_ok(dim, a, b) ? 1 : 0);
  return dfh::check_launch("embed_pair_cosine_kernel");
}

int dfh_embed_candidates(const float* gen, const float* table, const int64_t* cand, float* sims, int64_t* pred, int rows, int K, int dim,
                         int table_rows, void* stream) {
  DFH_REQUIRE(gen && table && cand && sims && pred, "null argument");
  DFH_REQUIRE(rows > 0 && K > 0 && dim > 0 && table_rows > 0, "rows / K / dim / table_rows must be positive");
  hipLaunchKernelGGL(embed_candidates_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, gen, table, cand, sims, pred, K, dim, table_rows,
                     vec_ok(dim, gen, table) ? 1 : 0);
  return dfh::check_launch("embed_candidates_kernel");
}

size_t dfh_compat_workspace_bytes(int outfits, int items, int feat_dim) {
  if (outfits <= 0 || items < 2 || items > 8 || feat_dim <= 0) return 0;
  return CompatWorkspace(nullptr, outfits, items, feat_dim).bytes();
}

int dfh_compat_pred_score(const float* const* params, int count, const float* outfit_emb, int outfits, float* logits, float* scores,
                          void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = check_params(params, count, "dfh_compat_pred_score")) return rc;
  DFH_REQUIRE(outfit_emb && workspace, "null argument");
  DFH_REQUIRE(outfits > 0 && outfits <= (1 << 21), "outfits must be in [1, 2^21]");
  DFH_REQUIRE(((uintptr_t)outfit_emb & 15) == 0, "outfit_emb must be 16-byte aligned");
  DFH_REQUIRE(((uintptr_t)workspace & 255) == 0, "workspace must be 256-byte aligned");
  DFH_REQUIRE(workspace_bytes >= dfh_compat_workspace_bytes(outfits, 2, 4), "workspace smaller than dfh_compat_workspace_bytes(outfits, 2, 4)");
  const CompatWorkspace w(workspace, outfits, 2, 4);
  return pred_score(params, outfit_emb, outfits, logits, scores, w.ping, w.pong, (hipStream_t)stream);
}

int dfh_compat_score(const float* const* params, int count, int feat_dim, const float* feats_real, int real_rows, const float* feats_gen,
                     int gen_rows, const int64_t* olists, int outfits, int items, float* outfit_emb, float* logits, float* scores,
                     void* workspace, size_t workspace_bytes, void* stream) {
  if (int rc = check_params(params, count, "dfh_compat_score")) return rc;
  DFH_REQUIRE(feats_real && workspace, "null argument");
  DFH_REQUIRE(feat_dim > 0 && feat_dim % 4 == 0, "feat_dim must be a positive multiple of 4");
  DFH_REQUIRE(items >= 2 && items <= 8, "items must be in [2, 8]");
  DFH_REQUIRE(outfits > 0 && outfits <= (1 << 17), "outfits must be in [1, 2^17] a call");
  DFH_REQUIRE(real_rows > 0 && gen_rows >= 0 && (feats_gen != nullptr) == (gen_rows > 0), "real_rows / gen_rows do not match the feature tables");
  DFH_REQUIRE(olists || real_rows == outfits * items, "without olists, feats_real is the gathered [outfits][items][feat_dim] tensor");
  DFH_REQUIRE((((uintptr_t)feats_real | (uintptr_t)feats_gen | (uintptr_t)outfit_emb) & 15) == 0, "features / outfit_emb must be 16-byte aligned");
  DFH_REQUIRE(((uintptr_t)workspace & 255) == 0, "workspace must be 256-byte aligned");
  DFH_REQUIRE(workspace_bytes >= dfh_compat_workspace_bytes(outfits, items, feat_dim), "workspace smaller than dfh_compat_workspace_bytes");
  hipStream_t s = (hipStream_t)stream;
  const CompatWorkspace w(workspace, outfits, items, feat_dim);
  const float* const* P = params;
  const int R = outfits * items, npairs = items * (items - 1) / 2, NP = outfits * npairs;
  const float* x = feats_real;
  if (olists) {
    hipLaunchKernelGGL(compat_gather_kernel, dim3(R), dim3(256), 0, s, feats_real, real_rows, feats_gen, gen_rows, olists, w.x, feat_dim);
    if (int rc = dfh::check_launch("compat_gather_kernel")) return rc;
    x = w.x;
  }
  if (int rc = compat_linear(x, P[CP_FEAT], feat_dim, P[CP_FEAT + 1], w.f, R, FEAT, s)) return rc;
  hipLaunchKernelGGL(compat_pairs_kernel, dim3(NP), dim3(256), 0, s, w.f, w.pairs, items, npairs, FEAT);
  if (int rc = dfh::check_launch("compat_pairs_kernel")) return rc;
  int rc = 0;
  const float* e = mlp_stack(P, CP_EMB, EMB_DIMS, 4, w.pairs, w.ping, w.pong, NP, s, rc);
  if (!e) return rc;
  float* emb = outfit_emb ? outfit_emb : w.emb;
  const long total = (long)outfits * EMB;
  hipLaunchKernelGGL(compat_pair_mean_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, e, emb, npairs, EMB, total);
  if (int rc2 = dfh::check_launch("compat_pair_mean_kernel")) return rc2;
  if (!logits && !scores) return 0;
  return pred_score(P, emb, outfits, logits, scores, w.ping, w.pong, s);
}

}  // extern "C"

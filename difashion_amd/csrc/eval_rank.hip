// Grounding retrieval of the reference's evaluation: every generated row is ranked against ALL items of its
// category -- a candidate set of its own length per category -- and the best nmax are kept in order.
//
// Replaces (arithmetic) the loop of clip_og_retrieval_given_data (Evaluation/eval_utils.py:725-767): per image a gather of the whole
// category, F.cosine_similarity, torch.topk and candidates[pred_idxs]; then `grd in topN_iids[:N]` per cutoff.
//
//   embed_row_norms_kernel   |x_r| of table rows and generated rows, one wave a row (the table's once for many batches)
//   embed_rank_gemm_kernel   sims = <g_m, table[cand[n]]> / (|g_m| |t|) for the rows of ONE candidate set: the 64 x 64 tile of f32_tile.h on
//                            v_mfma_f32_16x16x4_f32 under TileKahanSum, the B rows gathered in the tile's global loads
//   embed_rank_select_kernel per row the nmax best of its similarities, in torch.topk's order with a defined tie rule
//   embed_hit_pos_kernel / embed_hits_kernel   recall: first rank of the ground truth, hits per cutoff
//
// fp32 in both storage builds.  No atomics, nothing allocated, no scratch: reruns are bit-identical, and a row's similarities depend on
// K alone (every element is one tile-local chain per 32-wide k-tile plus the compensated add over k-tiles) -- not on the rows that share
// its tile, not on the set's length, not on the grid.
#include <cmath>

#include "../../include/difashion_hip.h"
#include "f32_tile.h"

namespace {

constexpr int RANK_NMAX = DFH_EMBED_RANK_NMAX;       // 128
constexpr int SEL_THREADS = 256;
constexpr int SEL_KEYS = 512;                        // the sorted list (first RANK_NMAX slots) + the pending survivors
constexpr int SEL_PENDING = SEL_KEYS - RANK_NMAX;    // 384

// norms[r] = sqrt(sum x_r^2): embed_pair_cosine_kernel's reduction (per lane a run of fused multiply-adds, then the wave tree)
__global__ __launch_bounds__(256) void embed_row_norms_kernel(const float* __restrict__ x, float* __restrict__ norms, int rows, int dim) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;                       // whole waves leave: the shuffles below see 64 live lanes
  const float4* r = (const float4*)(x + (long)row * dim);
  float s = 0.f;
  for (int c = lane; c < dim / 4; c += 64) {
    const float4 v = r[c];
    s = fmaf(v.x, v.x, s); s = fmaf(v.y, v.y, s); s = fmaf(v.z, v.z, s); s = fmaf(v.w, v.w, s);
  }
  s = wave_sum(s);
  if (lane == 0) norms[row] = sqrtf(s);
}

// One candidate set: gen [M][K] (the rows that rank against it), cand [N] ids into table [table_rows][K], sims [M][ld].
// blockIdx.x: 64 candidates, blockIdx.y: 64 rows.  A zero row on either side divides by 0: NaN (or inf) in its own scores only.
__global__ __launch_bounds__(256) void embed_rank_gemm_kernel(const float* __restrict__ gen, const float* __restrict__ gen_norms,
                                                              const float* __restrict__ table, const float* __restrict__ table_norms,
                                                              const int64_t* __restrict__ cand, float* __restrict__ sims, long ld, int M, int N,
                                                              int K, int table_rows) {
  dfh::gemm_tile<dfh::TileKahanSum>(gen, K, table, K, nullptr, M, N, K, [=](int m, int n, float acc) {
    const int64_t id = min(max(cand[n], (int64_t)0), (int64_t)table_rows - 1);
    sims[(long)m * ld + n] = acc / (gen_norms[m] * table_norms[id]);
  }, cand, table_rows);
}

// The order of the ranking in ONE unsigned comparison: high word = order-preserving image of the fp32 value (-0 counts as +0, a NaN
// stands above +inf), low word = ~position, so among equal values the lower position is the larger key.  No key is 0 (positions are
// below 2^31): 0 is the empty slot.
DFH_DEVICE unsigned long long rank_key(float v, int pos) {
  unsigned u = __float_as_uint(v);
  if (v != v) u = 0xffffffffu;
  else {
    if (u == 0x80000000u) u = 0u;
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  }
  return ((unsigned long long)u << 32) | (unsigned)~pos;
}

// keys[0 .. 512) descending, 256 threads (a bitonic network: 45 compare-exchange steps, one barrier each)
DFH_DEVICE void sort_keys_desc(unsigned long long* keys, int t) {
  for (int k = 2; k <= SEL_KEYS; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1)), l = i | j;
      const unsigned long long a = keys[i], b = keys[l];
      if ((a < b) == ((i & k) == 0)) { keys[i] = b; keys[l] = a; }
      __syncthreads();
    }
}

// One workgroup per row.  The row's similarities stream through in batches of 256; a value enters the pending list only if its key
// beats the current nmax-th best (everything, until the list is full), its slot found from wave ballots and the four waves' counts --
// no atomics; keys are distinct, so the outcome does not depend on the arrival order.  When another batch might not fit, the 512 keys
// are sorted and the first 128 stay.  4 KiB of LDS and a handful of registers: the kernel is bound by reading the row once.
__global__ __launch_bounds__(SEL_THREADS) void embed_rank_select_kernel(const float* __restrict__ sims, long ld, int len,
                                                                        const int64_t* __restrict__ cand, int nmax,
                                                                        int64_t* __restrict__ out_ids, int64_t* __restrict__ out_pos,
                                                                        float* __restrict__ out_sims, int* __restrict__ out_counts) {
  __shared__ unsigned long long keys[SEL_KEYS];
  __shared__ int wcount[2][4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const float* row = sims + (long)blockIdx.x * ld;
  keys[t] = 0ull; keys[t + SEL_THREADS] = 0ull;
  __syncthreads();
  unsigned long long thr = 0ull;                 // the nmax-th best so far (0: the list is not full)
  int npend = 0, flip = 0;
  for (int base = 0; base < len; base += SEL_THREADS, flip ^= 1) {
    const int pos = base + t;
    unsigned long long key = 0ull;
    if (pos < len) key = rank_key(row[pos], pos);
    const bool keep = key > thr;
    const unsigned long long vote = __ballot(keep);
    if (lane == 0) wcount[flip][wave] = __popcll(vote);
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) { const int c = wcount[flip][w]; before += w < wave ? c : 0; total += c; }
    if (keep) keys[RANK_NMAX + npend + before + __popcll(vote & ((1ull << lane) - 1ull))] = key;
    npend += total;
    if (npend > SEL_PENDING - SEL_THREADS) {     // the next batch might not fit: fold the pending keys into the list
      __syncthreads();
      sort_keys_desc(keys, t);
      thr = keys[nmax - 1];
      __syncthreads();
      if (t < SEL_PENDING - SEL_THREADS) keys[RANK_NMAX + SEL_THREADS + t] = 0ull;
      keys[RANK_NMAX + t] = 0ull;
      npend = 0;
      __syncthreads();
    }
  }
  __syncthreads();
  if (npend > 0) sort_keys_desc(keys, t);
  const long o = (long)blockIdx.x * nmax;
  if (t < nmax) {
    const unsigned long long key = keys[t];
    if (key != 0ull) {
      const int pos = (int)~(unsigned)key;
      out_ids[o + t] = cand[pos]; out_pos[o + t] = pos; out_sims[o + t] = row[pos];     // the value itself: the sign of a zero, a NaN's bits
    } else {
      out_ids[o + t] = -1; out_pos[o + t] = -1; out_sims[o + t] = -INFINITY;
    }
  }
  if (t == 0) out_counts[blockIdx.x] = len < nmax ? len : nmax;
}

// hit_pos[r] = the first rank j < counts[r] with ids[r][j] == grd[r], -1 if none; one wave a row
__global__ __launch_bounds__(256) void embed_hit_pos_kernel(const int64_t* __restrict__ ids, const int* __restrict__ counts,
                                                            const int64_t* __restrict__ grd, int* __restrict__ hit_pos, int rows, int nmax) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  const int n = min(counts[row], nmax);
  const int64_t want = grd[row];
  int first = 0x7fffffff;
  for (int j = lane; j < n; j += 64)
    if (ids[(long)row * nmax + j] == want) { first = j; break; }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) first = min(first, __shfl_xor(first, o, 64));
  if (lane == 0) hit_pos[row] = first == 0x7fffffff ? -1 : first;
}

// hits[c] = #{r : 0 <= hit_pos[r] < cutoffs[c]}: ONE workgroup, integer counts through an LDS tree
__global__ __launch_bounds__(256) void embed_hits_kernel(const int* __restrict__ hit_pos, int rows, const int* __restrict__ cutoffs, int ncut,
                                                         int64_t* __restrict__ hits) {
  __shared__ int part[256];
  for (int c = 0; c < ncut; ++c) {
    const int cut = cutoffs[c];
    int n = 0;
    for (int r = threadIdx.x; r < rows; r += 256) { const int h = hit_pos[r]; n += (h >= 0 && h < cut) ? 1 : 0; }
    part[threadIdx.x] = n;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
      __syncthreads();
    }
    if (threadIdx.x == 0) hits[c] = part[0];
    __syncthreads();
  }
}

long round64(long n) { return (n + 63) / 64 * 64; }

}  // namespace

extern "C" {

int dfh_embed_row_norms(const float* x, float* norms, int rows, int dim, void* stream) {
  DFH_REQUIRE(x && norms, "null argument");
  DFH_REQUIRE(rows > 0 && dim > 0, "rows / dim must be positive");
  DFH_REQUIRE(dim % 4 == 0 && ((uintptr_t)x & 15) == 0, "dim must be a multiple of 4 and x 16-byte aligned (rows are read as float4)");
  hipLaunchKernelGGL(embed_row_norms_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, x, norms, rows, dim);
  return dfh::check_launch("embed_row_norms_kernel");
}

size_t dfh_embed_rank_workspace_bytes(int rows, long max_set_len, int nmax) {
  if (rows <= 0 || max_set_len < 0 || max_set_len > 0x7fffffffL - 64 || nmax < 1 || nmax > RANK_NMAX) return 0;
  return (size_t)rows * (size_t)round64(max_set_len > 0 ? max_set_len : 1) * sizeof(float) + 256;
}

int dfh_embed_rank(const float* gen, const float* gen_norms, int rows, int dim, const float* table, const float* table_norms, int table_rows,
                   const int64_t* cand_ids, const int64_t* set_off, int nsets, const int* row_set, int nmax, void* workspace,
                   size_t workspace_bytes, int64_t* out_ids, int64_t* out_pos, float* out_sims, int* out_counts, void* stream) {
  DFH_REQUIRE(gen && gen_norms && table && table_norms && cand_ids && set_off && row_set && workspace && out_ids && out_pos && out_sims && out_counts,
              "null argument");
  DFH_REQUIRE(rows > 0 && dim > 0 && table_rows > 0 && nsets > 0, "rows / dim / table_rows / nsets must be positive");
  DFH_REQUIRE(dim % 4 == 0, "dim must be a multiple of 4 (rows are read as float4)");
  DFH_REQUIRE((((uintptr_t)gen | (uintptr_t)table) & 15) == 0, "gen / table must be 16-byte aligned");
  DFH_REQUIRE(((uintptr_t)workspace & 255) == 0, "workspace must be 256-byte aligned");
  DFH_REQUIRE(nmax >= 1 && nmax <= RANK_NMAX, "nmax must be in [1, DFH_EMBED_RANK_NMAX (128)]");
  DFH_REQUIRE(set_off[0] >= 0, "set_off must start at 0 or above");
  for (int s = 0; s < nsets; ++s)
    DFH_REQUIRE(set_off[s + 1] >= set_off[s] && set_off[s + 1] - set_off[s] <= 0x7fffffffL - 64, "set_off must be monotone, a set below 2^31 ids");
  long max_len = 0;
  for (int r = 0; r < rows; ++r) {
    DFH_REQUIRE(row_set[r] >= 0 && row_set[r] < nsets, "row_set names a set outside [0, nsets)");
    DFH_REQUIRE(r == 0 || row_set[r] >= row_set[r - 1], "rows must arrive grouped by set (row_set ascending)");
    const long len = set_off[row_set[r] + 1] - set_off[row_set[r]];
    max_len = len > max_len ? len : max_len;
  }
  DFH_REQUIRE(workspace_bytes >= dfh_embed_rank_workspace_bytes(rows, max_len, nmax),
              "workspace smaller than dfh_embed_rank_workspace_bytes(rows, the longest set of these rows, nmax)");
  hipStream_t s = (hipStream_t)stream;
  float* sims = (float*)workspace;
  const long ld = round64(max_len > 0 ? max_len : 1);
  for (int r0 = 0; r0 < rows;) {
    int r1 = r0 + 1;
    while (r1 < rows && row_set[r1] == row_set[r0]) ++r1;
    const int M = r1 - r0;
    const int64_t off = set_off[row_set[r0]];
    const int len = (int)(set_off[row_set[r0] + 1] - off);
    if (len > 0) {
      dfh::ProfScope ps(dfh::PC_OTHER, 2.0 * M * len * dim, 4.0 * ((double)M * dim + (double)len * dim + (double)M * len), s);
      hipLaunchKernelGGL(embed_rank_gemm_kernel, dim3((len + dfh::GT_N - 1) / dfh::GT_N, (M + dfh::GT_M - 1) / dfh::GT_M), dim3(256), 0, s,
                         gen + (long)r0 * dim, gen_norms + r0, table, table_norms, cand_ids + off, sims + r0 * ld, ld, M, len, dim, table_rows);
      if (int rc = dfh::check_launch("embed_rank_gemm_kernel")) return rc;
    }
    hipLaunchKernelGGL(embed_rank_select_kernel, dim3(M), dim3(SEL_THREADS), 0, s, sims + r0 * ld, ld, len, cand_ids + off, nmax,
                       out_ids + (long)r0 * nmax, out_pos + (long)r0 * nmax, out_sims + (long)r0 * nmax, out_counts + r0);
    if (int rc = dfh::check_launch("embed_rank_select_kernel")) return rc;
    r0 = r1;
  }
  return 0;
}

int dfh_embed_recall(const int64_t* ids, const int* counts, int rows, int nmax, const int64_t* grd, const int* cutoffs, int ncut, int* hit_pos,
                     int64_t* hits, void* stream) {
  DFH_REQUIRE(ids && counts && grd && hit_pos, "null argument");
  DFH_REQUIRE(rows > 0, "rows must be positive");
  DFH_REQUIRE(nmax >= 1 && nmax <= RANK_NMAX, "nmax must be in [1, DFH_EMBED_RANK_NMAX (128)]");
  DFH_REQUIRE(ncut >= 0 && ncut <= 64 && (ncut == 0 || (cutoffs && hits)), "cutoffs / hits: up to 64 cutoffs, both pointers or none");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(embed_hit_pos_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, ids, counts, grd, hit_pos, rows, nmax);
  if (int rc = dfh::check_launch("embed_hit_pos_kernel")) return rc;
  if (ncut == 0) return 0;
  hipLaunchKernelGGL(embed_hits_kernel, dim3(1), dim3(256), 0, s, hit_pos, rows, cutoffs, ncut, hits);
  return dfh::check_launch("embed_hits_kernel");
}

}  // extern "C"

// Fused softmax(Q K^T / sqrt(d)) V on v_mfma_f32_32x32x16_bf16 for the U-Net's long self-attention launches
// (SD-1.5: (N, d) = (4096, 40) and (1024, 80): 90 % of the attention time of a sampling step).
// Reference call sites: diffusers Attention (attn1 of BasicTransformerBlock) reached via
// DiFashion/models/difashion.py:249-253,518-523 (xformers memory_efficient_attention there, difashion.py:118).
//
// Why a second kernel (attention.hip stays for head dims > 80, short / ragged key ranges and the training LSE path it
// was tuned for): at d = 40 the 16x16x32 kernel pads the contraction 40 -> 64 and spends 165 VALU instructions per 32 x 64
// score tile -- the softmax VALU work, not the MFMA pipe, paces it (round-1 PMC: VALU active 70 %, MFMA busy 34 %).
// This kernel removes both costs:
//   * 32x32x16 MFMA: the contraction is padded to a multiple of 16 (40 -> 48), a 32x32x16 issues at 32 cycles
//     (1024 flop/cycle/SIMD) where the 16x16x32 measured 19.5-20 (820 flop/cycle) -- profiles/r02/mfma_rate2.txt.
//   * scores are computed transposed, S^T = K . Q^T (keys = rows): a lane owns ONE query (column lane & 31) and
//     16 keys per 32-key block, so the softmax needs no cross-lane traffic, and the C layout of S^T IS the B layout of
//     the P^T operand of O^T = V^T . P^T (lane half hi holds k-slots 8 hi .. 8 hi + 7 of every 16-key MFMA) once the K
//     rows of a block are read in the order key = swap_bits_2_3(slot): probabilities never leave registers and need
//     no permutes at all.
//   * the two free contraction slots of the padding carry the softmax bookkeeping: K column d = D is 1.0 and
//     Q column D is -m (the running max, kept bf16-exact), Q is pre-scaled by scale * log2(e) -> the MFMA delivers
//     s * c - m directly: no multiply / subtract per score.  K column D+1 is 1.0 for keys beyond Nk and Q column D+1 is
//     -30000 -> ragged key ranges are masked by the MFMA as well.  V^T row D is all ones, so O^T row D accumulates the
//     softmax denominator: no per-score add.
//   * what is left per score: one v_exp_f32, half a v_cvt_pk_bf16_f32, half a v_max3_f32 (the deferred-max check:
//     the running max only moves when some score exceeds it by 2^8, a wave-uniform rare branch).
//   * 4 waves x 64 queries (two 32-query blocks: every K / V^T fragment read feeds two MFMAs) = 256 queries per
//     workgroup, ~240 VGPRs, two workgroups per CU: while one wave of a SIMD is in its exp / pack phase its neighbour
//     issues MFMAs.  K / V^T tiles of 64 keys are double-buffered in LDS (issue-early / write-late register staging through
//     buffer loads, one barrier per tile), 16-byte slots XOR-swizzled so every ds_read_b128 fragment read is conflict-free.
//
// What bounds it (profiles/r02/coissue.txt, valu_rate.txt -- scripts/probes/coissue.hip): per SIMD a v_exp_f32 occupies the
// VALU port for ~8.7 cycles and any other VALU instruction for ~4.6, whichever wave issues it, and one wave mixing MFMAs with
// exps overlaps them only partially (7 MFMA + 16 exp + 8 cvt: 328 cycles alone, 279 each for two co-resident waves, against
// 224 of matrix-pipe time).  A 64-query x 64-key tile costs 28 MFMAs = 896 matrix-pipe cycles and 64 exp + 32 cvt + ~30 other
// = ~840 VALU-port cycles: the two are balanced, so d = 40 attention cannot approach the MFMA roof the way d = 128 does
// (one exp per 4 x 56 padded flop instead of per 4 x 128).  Measured: 2130 cycles per tile with one wave per SIMD, 1830 per SIMD
// with two; a software-pipelined variant (S of block i+1 and P.V of block i-1 issued around the exps of block i, LDS-DMA
// staging) and s_setprio around the MFMA clusters were both measured and were not faster (555 / 475 vs 470 us).
#include "attention_x32_steps.h"
#include "walk_knobs.h"

#include <algorithm>
#include <type_traits>
#ifdef DFH_PROBES   // experiments that lost their same-box comparison: the in-wave pipeline of QB = 4, the phase-stamp printout
#include "attention_x32_probe.h"
#endif

namespace {

// QB = 32-query blocks per wave (2: 256 queries per workgroup; 1: 128, for head dims whose accumulators would not fit)
template <int D, int QB, int MINW, bool PROF = false>
__global__ __launch_bounds__(256, MINW) void attention_x32_kernel(const AttnArgs a) {
  constexpr int NBUF = 2;                                  // K / V^T tile buffers in LDS
  using G = X32Geom<D>;
  constexpr int DCH = G::DCH, NKI = G::NKI, NVI = G::NVI;
  constexpr int WQ = QB * 32;                              // queries per wave
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ql = lane & 31, hi = lane >> 5;

  // one (batch, head) per group of consecutive logical blocks, and consecutive logical blocks on ONE XCD: the 16 workgroups
  // of a (batch, head) share its K / V^T through one L2 instead of fetching them on all eight
  const int nqb = (a.Nq + 4 * WQ - 1) / (4 * WQ);
  const int lb = xcd_remap(blockIdx.x, gridDim.x);
  const int bh = lb / nqb, qblk = lb - bh * nqb;
  const int b = bh / a.H, h = bh - b * a.H;
  const int q0 = qblk * 4 * WQ + wave * WQ;

  const bf16_t* Qb = a.Q + (long)b * a.Nq * a.ldq + h * D;
  const bf16_t* Kb = a.K + (long)b * a.Nk * a.ldk + h * D;
  const bf16_t* Vb = a.Vt + (long)b * (a.vt_bstride ? a.vt_bstride : (long)a.H * D * a.ldvt) + (long)h * D * a.ldvt;

  X32Wave<D, QB> w;
  {
    uint4 qraw[QB][G::KS];
    x32_fetch_q<D, QB>(qraw, a, Qb, q0, ql, hi);
    x32_q_frags(w, qraw, a, q0, ql, hi);
  }

  // ---- staging bookkeeping (fixed per thread).  Chunk ids wrap around the tile: the threads left over in the last round
  //      re-stage a chunk another thread stages too (same bytes to the same address) -- no divergent branch in the loop
  int k_goff[NKI], k_lds[NKI];
#pragma unroll
  for (int i = 0; i < NKI; ++i) {
    const int idx = (tid + i * 256) % (KVT * DCH);
    const int key = idx / DCH, ch = idx - key * DCH;
    k_goff[i] = key * a.ldk + ch * 8;
    k_lds[i] = k_slot<D>(key, ch);
  }
  int v_goff[NVI], v_lds[NVI], v_k0[NVI];
#pragma unroll
  for (int i = 0; i < NVI; ++i) {
    const int idx = (tid + i * 256) % (D * 8);
    const int row = idx >> 3, ch = idx & 7;
    v_goff[i] = row * a.ldvt + ch * 8;
    v_k0[i] = ch * 8;
    v_lds[i] = G::K_BYTES + v_slot(row, ch);
  }
  uint4 kreg[NKI], vreg[NVI];

  // K / V^T tiles are fetched with buffer loads: one descriptor per operand in SGPRs (built from wave-uniform values), a
  // 32-bit per-lane byte offset fixed for the kernel and the tile's byte offset in an SGPR -- no 64-bit address VGPRs in the
  // loop (as pointers they cost 8 VGPRs that hipcc spilled to scratch and reloaded, ~500 cycles each, at the top of every
  // tile).  The K descriptor ends with the last valid key row, so rows beyond Nk read as zeros without a predicate.
  typedef __attribute__((ext_vector_type(4))) unsigned u32x4_t;
  const unsigned k_bytes = a.Nk > 0 ? (unsigned)(((long)(a.Nk - 1) * a.ldk + D) * 2) : 0u;
  const unsigned v_bytes = (unsigned)(((long)(D - 1) * a.ldvt + a.ldvt) * 2);
  const auto k_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)Kb, 0, k_bytes, 0x00020000);
  const auto v_rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)Vb, 0, v_bytes, 0x00020000);
  auto load_tile = [&](int kv0, auto full_c) {   // global -> registers (zeros beyond Nk)
    constexpr bool FULL = decltype(full_c)::value;
    const int k_soff = kv0 * a.ldk * 2, v_soff = kv0 * 2;                    // wave-uniform byte offsets of the tile
#pragma unroll
    for (int i = 0; i < NKI; ++i) {
      const u32x4_t r = __builtin_amdgcn_raw_buffer_load_b128(k_rsrc, k_goff[i] * 2, k_soff, 0);
      kreg[i] = uint4{r[0], r[1], r[2], r[3]};
    }
#pragma unroll
    for (int i = 0; i < NVI; ++i) {
      const u32x4_t r = __builtin_amdgcn_raw_buffer_load_b128(v_rsrc, v_goff[i] * 2, v_soff, 0);
      uint4 v = uint4{r[0], r[1], r[2], r[3]};
      if (!FULL) {
        const int k0 = kv0 + v_k0[i];
        if (k0 >= a.Nk) v = uint4{0u, 0u, 0u, 0u};
        else if (k0 + 8 > a.Nk) x32_zero_tail(v, a.Nk - k0);
      }
      vreg[i] = v;
    }
  };
  auto store_tile = [&](int buf) {               // registers -> swizzled LDS image
    unsigned char* Bs = smem + buf * G::BUF;
#pragma unroll
    for (int i = 0; i < NKI; ++i) *(uint4*)(Bs + k_lds[i]) = kreg[i];
#pragma unroll
    for (int i = 0; i < NVI; ++i) *(uint4*)(Bs + v_lds[i]) = vreg[i];
  };
  auto store_const = [&](int buf, int first_masked) { x32_store_const<D>(smem + buf * G::BUF, tid, first_masked); };

  const X32Frag<D> fr = x32_frag<D>(ql, hi);
  const int ntiles = (a.Nk + KVT - 1) / KVT;
  const int tail_valid = a.Nk - (ntiles - 1) * KVT;          // valid keys of the last tile (KVT when Nk % 64 == 0)
  const int nfast = a.Nk / KVT - 1;                          // tiles whose successor is a full tile
  unsigned* poison_flag = (unsigned*)(smem + NBUF * G::BUF); // one word behind the tile buffers
  if (tid == 0) *poison_flag = 0u;

  // One pass over the keys.  SAFE = false (the fast pass): after the first tile there is NO per-score max -- the running
  // offset m only has to keep 2^(s - m) inside the fp32 / bf16 exponent range (both carry 8 exponent bits, so the relative
  // precision of P does not depend on its magnitude), which one compare per tile on the softmax denominator (row D of O^T)
  // guarantees: when it passes 2^24 the wave divides O by an exact power of two and raises m by that integer (m stays an
  // integer, hence bf16-exact in its contraction slot).  A score more than ~100 log2 units above m inside ONE tile would
  // overflow the exp before the compare sees it: the denominator then reads >= 2^100 / inf / NaN, the wave raises the
  // workgroup's poison flag and the whole workgroup repeats the pass with SAFE = true -- the exact deferred-max scheme
  // (lane-local v_max3 tree before the exp, rescale when a score exceeds m by 2^8) that is also used for tile 0.
  auto pass = [&](auto safe_c) {
    constexpr bool SAFE = decltype(safe_c)::value;
    x32_reset(w, hi);
    bool poison = false;
    store_const(0, ntiles == 1 ? tail_valid : KVT);
    store_const(1, ntiles == 2 ? tail_valid : KVT);
    load_tile(0, std::false_type{});
    store_tile(0);
    __syncthreads();

    // precheck_c: lane-local max tree + deferred-max rescale BEFORE the exp (tile 0 and the SAFE pass)
    auto tile = [&](int t, auto fast_c, auto precheck_c) {
      constexpr bool FAST = decltype(fast_c)::value;            // this tile's successor exists and is a full tile
      constexpr bool PRE = decltype(precheck_c)::value;
      const int kv0 = t * KVT;
      const bool more = FAST || t + 1 < ntiles;
      if (FAST) load_tile(kv0 + KVT, std::true_type{});
      else if (more) load_tile(kv0 + KVT, std::false_type{});
      const unsigned char* Ks = smem + (t & 1) * G::BUF;
      const unsigned char* Vs = Ks + G::K_BYTES;
      const bool stamp = PROF && a.prof && blockIdx.x == 0 && wave == 0 && lane == 0 && t < 64;
      auto mark = [&](int i) {          // diagnosis build only: wave-issue timeline (s_memtime = shader cycles)
        if (PROF) { __builtin_amdgcn_sched_barrier(0); if (stamp) a.prof[t * 8 + i] = __builtin_readcyclecounter(); __builtin_amdgcn_sched_barrier(0); }
      };
      mark(0);
#ifdef DFH_PROBES
      if constexpr (QB == 4 && !PRE) x32_tile_pipelined(w, fr, Ks, Vs, hi, mark); else
#endif
      {
        f32x16_t s[2][QB];                             // [kb] 32 keys x [qb] 32 queries
        x32_scores(s[0], w, fr, Ks);
        x32_scores(s[1], w, fr, Ks + 32 * G::KROW);
        mark(1);
        if (PRE) x32_deferred_max<!SAFE>(w, s, t == 0, hi);     // the fast pass needs an integer offset of its first tile
        uint32_t pw[2][QB][8];
        x32_exp_pack(pw[0], w, s[0]);
        x32_exp_pack(pw[1], w, s[1]);
        mark(2);
        x32_pv(w, fr, Vs, 0, hi, pw[0]);
        x32_pv(w, fr, Vs, 1, hi, pw[1]);
        mark(3);
      }
      if (more) {
        store_tile((t + 1) & 1);                     // the other buffer: last read one barrier ago
        // a ragged last tile changes the mask column of the buffer it lands in (buffers 0 / 1 were initialised for tiles 0 / 1)
        if (!FAST && t + 2 == ntiles && t + 1 >= 2 && tail_valid != KVT) store_const((t + 1) & 1, tail_valid);
      }
      if (!PRE) {
        // ---- fast pass: watch the denominator (lanes of half L_HI hold it; the other half holds a zero row of O^T)
        bool big = false;
#pragma unroll
        for (int qb = 0; qb < QB; ++qb) big |= !(x32_den(w, qb) <= 16777216.0f);      // 2^24; also true for NaN
        if (__any(big)) {
#pragma unroll
          for (int qb = 0; qb < QB; ++qb) {
            const float l = x32_den_total(w, qb, hi);
            poison |= !(l < 1.2676506e30f);          // 2^100: an exp may already have overflowed
            // exponent of l as an integer-valued float, kept a multiple of the bf16 spacing of the new m
            float m_new = w.m_run[qb] + (l > 2.0f ? floorf(__builtin_amdgcn_logf(l)) : 0.0f);      // v_log_f32 = log2
            m_new = bf2f(f2bf(m_new));
            const float delta = m_new - w.m_run[qb];   // an integer >= 0 (both are bf16-exact integers)
            w.m_run[qb] = m_new;
            x32_scale_o(w, qb, __builtin_amdgcn_exp2f(-delta));      // exact power of two
            x32_set_pad(w, qb, -m_new, hi);
          }
        }
      }
      mark(4);
      __syncthreads();
      mark(5);
    };
    if (SAFE) {
      int t = 0;
      for (; t < nfast; ++t) tile(t, std::true_type{}, std::true_type{});
      for (; t < ntiles; ++t) tile(t, std::false_type{}, std::true_type{});
    } else {
      if (nfast > 0) tile(0, std::true_type{}, std::true_type{});
      else tile(0, std::false_type{}, std::true_type{});
      int t = 1;
      for (; t < nfast; ++t) tile(t, std::true_type{}, std::false_type{});
      for (; t < ntiles; ++t) tile(t, std::false_type{}, std::false_type{});
    }
    return poison;
  };

  if constexpr (DFH_H16_WIDE_EXPONENT) {
    const bool poisoned = pass(std::false_type{});
    if (__any(poisoned) && lane == 0) *poison_flag = 1u;
    __syncthreads();
    if (*poison_flag) {            // workgroup-uniform and essentially never: an in-tile score jump of > 2^100
      __syncthreads();
      (void)pass(std::true_type{});
    }
  } else {
    // a storage type with a 5-bit exponent cannot hold the fast pass's unchecked 2^(s - m): every tile takes the exact
    // deferred-max form, which keeps the probabilities at or below 2^THR
    (void)pass(std::true_type{});
  }

  // ---- normalise and store
  const float qmul = attn_qmul(a, b);
#pragma unroll
  for (int qb = 0; qb < QB; ++qb) {
    const float l = x32_den_total(w, qb, hi);
    const int q = q0 + qb * 32 + ql;
    if (q >= a.Nq) continue;
    if (a.lse && hi == 0) a.lse[((long)b * a.H + h) * a.Nq + q] = w.m_run[qb] + __builtin_amdgcn_logf(l);   // v_log_f32 = log2
    x32_store_row(a, w, qb, ((long)b * a.Nq + q) * a.ldo + h * D, qmul / l, hi);
  }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Short key ranges: the cross-attention over the 77 text tokens (attn2 of BasicTransformerBlock, reference difashion.py:518-523).
// With at most 2 * KVT keys the whole K / V^T of a (batch, head) fits the two LDS buffers: they are staged ONCE, and then every wave
// walks `qrep` blocks of 32 * QB queries with no further barrier -- Q in, two score tiles, softmax, P.V, O out.  In the streaming
// kernel above such a launch is all prologue and epilogue (one dependent chain of Q load -> tile staging -> barrier -> ... per 256
// queries: 44 us for 84 MB at the 64x64 level); here the chain is paid once per workgroup and the per-block work of the four
// waves of a workgroup (and of the two workgroups of a CU) overlaps freely.  The softmax is the exact deferred-max form of the
// streaming kernel's SAFE pass on both tiles (two tiles: nothing to win from the fast pass), same tile steps, same numerics.
template <int D, int QB>
__global__ __launch_bounds__(256, 2) void attention_xs_kernel(const AttnArgs a, const int qrep) {
  using G = X32Geom<D>;
  static_assert(!G::LSUM, "the short-key kernel reads the denominator from the ones row of V^T");
  constexpr int DCH = G::DCH;
  constexpr int WQ = QB * 32;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ql = lane & 31, hi = lane >> 5;
  const int per_wg = 4 * WQ * qrep;
  const int nqb = (a.Nq + per_wg - 1) / per_wg;
  const int lb = xcd_remap(blockIdx.x, gridDim.x);
  const int bh = lb / nqb, qblk = lb - bh * nqb;
  const int b = bh / a.H, h = bh - b * a.H;
  const bf16_t* Qb = a.Q + (long)b * a.Nq * a.ldq + h * D;
  const bf16_t* Kb = a.K + (long)b * a.Nk * a.ldk + h * D;
  const bf16_t* Vb = a.Vt + (long)b * (a.vt_bstride ? a.vt_bstride : (long)a.H * D * a.ldvt) + (long)h * D * a.ldvt;
  const int ntiles = (a.Nk + KVT - 1) / KVT;                 // 1 or 2 (the launcher guarantees Nk <= 2 * KVT)
  const int tail_valid = a.Nk - (ntiles - 1) * KVT;

  // ---- stage every key once: tile t -> buffer t (ragged tail zero-filled, mask column set)
  for (int t = 0; t < ntiles; ++t) {
    unsigned char* Ks = smem + t * G::BUF;
    unsigned char* Vs = Ks + G::K_BYTES;
    const int kv0 = t * KVT;
    for (int idx = tid; idx < KVT * DCH; idx += 256) {
      const int key = idx / DCH, ch = idx - key * DCH;
      uint4 v = uint4{0u, 0u, 0u, 0u};
      if (kv0 + key < a.Nk) v = *(const uint4*)(Kb + (long)(kv0 + key) * a.ldk + ch * 8);
      *(uint4*)(Ks + k_slot<D>(key, ch)) = v;
    }
    for (int idx = tid; idx < D * 8; idx += 256) {
      const int row = idx >> 3, ch = idx & 7;
      const int k0 = kv0 + ch * 8;
      uint4 v = uint4{0u, 0u, 0u, 0u};
      if (k0 < a.Nk) {
        v = *(const uint4*)(Vb + (long)row * a.ldvt + k0);       // ldvt >= roundup8(Nk): the chunk exists
        if (k0 + 8 > a.Nk) x32_zero_tail(v, a.Nk - k0);
      }
      *(uint4*)(Vs + v_slot(row, ch)) = v;
    }
    x32_store_const<D>(Ks, tid, t == ntiles - 1 ? tail_valid : KVT);
  }
  __syncthreads();
  const X32Frag<D> fr = x32_frag<D>(ql, hi);

  // the Q rows of the NEXT block are requested before the current block is computed: load -> scores -> softmax -> P.V -> store was one
  // dependent chain per block and wave, with nothing in flight while it computed
  constexpr bool PREFETCH_Q = QB == 1;
  uint4 qraw[QB][G::KS];
  if (PREFETCH_Q) x32_fetch_q<D, QB>(qraw, a, Qb, qblk * per_wg + wave * WQ, ql, hi);
  for (int rep = 0; rep < qrep; ++rep) {
    const int q0 = qblk * per_wg + rep * 4 * WQ + wave * WQ;
    if (q0 >= a.Nq) break;                                    // wave-uniform
    if (!PREFETCH_Q) x32_fetch_q<D, QB>(qraw, a, Qb, q0, ql, hi);
    X32Wave<D, QB> w;
    x32_q_frags(w, qraw, a, q0, ql, hi);
    if (PREFETCH_Q && rep + 1 < qrep) x32_fetch_q<D, QB>(qraw, a, Qb, q0 + 4 * WQ, ql, hi);
    x32_reset(w, hi);

    for (int t = 0; t < ntiles; ++t) {
      const unsigned char* Ks = smem + t * G::BUF;
      const unsigned char* Vs = Ks + G::K_BYTES;
      // second 32-key block of the tile entirely beyond Nk (77 text tokens: keys 96..127): its scores are the mask value, its
      // probabilities zero -- no MFMA, no exponentials, no P.V for it (a quarter of the launch's matrix and VALU work)
      const bool kb1 = t * KVT + 32 < a.Nk;                  // workgroup-uniform
      f32x16_t s[2][QB];
      x32_scores(s[0], w, fr, Ks);
      if (kb1) {
        x32_scores(s[1], w, fr, Ks + 32 * G::KROW);
      } else {
#pragma unroll
        for (int qb = 0; qb < QB; ++qb)
#pragma unroll
          for (int r = 0; r < 16; ++r) s[1][qb][r] = MASK_Q;
      }
      x32_deferred_max<false>(w, s, t == 0, hi);
      uint32_t pw[2][QB][8];
      x32_exp_pack(pw[0], w, s[0]);
      if (kb1) x32_exp_pack(pw[1], w, s[1]);
      x32_pv(w, fr, Vs, 0, hi, pw[0]);
      if (kb1) x32_pv(w, fr, Vs, 1, hi, pw[1]);
    }
    // ---- normalise and store.  bf16 output: the wave's WQ x D block is turned through a wave-private LDS region so that a row leaves as
    // D / 8 consecutive 16-byte stores (one 2 * D-byte run per row) -- straight from the accumulator layout a row left in 16-byte pieces
    // from five different instructions, and this launch is nothing but Q in / O out (84 MB at the 64x64 level)
    if (!a.O8) {
      unsigned char* st = smem + 2 * G::BUF + 16 + wave * (WQ * D * 2);
#pragma unroll
      for (int qb = 0; qb < QB; ++qb) {
        const float inv = 1.0f / x32_den_total(w, qb, hi);
#pragma unroll
        for (int db = 0; db < G::DB; ++db)
#pragma unroll
          for (int g = 0; g < 4; ++g) {
            const int d0 = db * 32 + g * 8 + hi * 4;
            if (d0 < D) {
              uint2 v;
              v.x = pack2bf(w.o[db][qb][4 * g] * inv, w.o[db][qb][4 * g + 1] * inv);
              v.y = pack2bf(w.o[db][qb][4 * g + 2] * inv, w.o[db][qb][4 * g + 3] * inv);
              *(uint2*)(st + (qb * 32 + ql) * (D * 2) + d0 * 2) = v;
            }
          }
      }
      constexpr int CH = D / 8;                                // 16-byte chunks per row
#pragma unroll
      for (int i0 = 0; i0 < WQ * CH; i0 += 64) {
        const int i = i0 + lane;
        const int row = i / CH, ch = i - row * CH;
        const int q = q0 + row;
        if (i < WQ * CH && q < a.Nq)
          *(uint4*)(a.O + ((long)b * a.Nq + q) * a.ldo + h * D + ch * 8) = *(const uint4*)(st + row * (D * 2) + ch * 16);
      }
      continue;
    }
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
      const float inv = attn_qmul(a, b) / x32_den_total(w, qb, hi);
      const int q = q0 + qb * 32 + ql;
      if (q >= a.Nq) continue;
      x32_store_row(a, w, qb, ((long)b * a.Nq + q) * a.ldo + h * D, inv, hi);
    }
  }
}

// one launch of KERN over nblk workgroups per (batch, head): the dynamic-LDS attribute once per kernel, the profile scope, the launch check
template <auto KERN, class... Extra>
int launch_attn(const char* name, int lds, int nblk, const AttnArgs& a, hipStream_t stream, Extra... extra) {
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)KERN, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
    attr_set = true;
  }
  dfh::ProfScope ps(dfh::PC_ATTN, 4.0 * a.B * a.H * (double)a.Nq * a.Nk * a.D,
                    2.0 * a.B * a.H * a.D * (2.0 * a.Nq + 2.0 * a.Nk), stream);
  hipLaunchKernelGGL(KERN, dim3(nblk * a.H * a.B), dim3(256), lds, stream, a, extra...);
  return dfh::check_launch(name);
}

template <int D, int QB>
int launch_xs(const AttnArgs& a, hipStream_t stream) {
  constexpr int lds = 2 * X32Geom<D>::BUF + 16 + 4 * QB * 32 * D * 2;      // + the four waves' output staging blocks
  static_assert(lds <= 160 * 1024, "LDS");
  // query blocks per wave: enough workgroups to give every CU its two, few enough to amortise the one-time K / V^T staging
  const long units = (long)a.B * a.H * ((a.Nq + 128 * QB - 1) / (128 * QB));
  const int qrep = (int)std::max(1L, std::min(8L, units / 512));
  const int nqb = (a.Nq + 128 * QB * qrep - 1) / (128 * QB * qrep);
  return launch_attn<attention_xs_kernel<D, QB>>("attention_xs_kernel", lds, nqb, a, stream, qrep);
}

template <int D, int QB, int MINW, bool PROF = false>
int launch_x32(const AttnArgs& a, hipStream_t stream) {
  constexpr int lds = 2 * X32Geom<D>::BUF + 16;
  const int nqb = (a.Nq + 128 * QB - 1) / (128 * QB);
  return launch_attn<attention_x32_kernel<D, QB, MINW, PROF>>("attention_x32_kernel", lds, nqb, a, stream);
}

}  // namespace

namespace dfh {

// 0 = not handled here (the caller falls back to attention_kernel).  The backward depends on this answer too, through takes_x32 /
// attention_fwd_q_prescaled in attention.hip: at d = 64 it rounds Q as this kernel does exactly where this says yes.
bool attention_x32_eligible(const AttnArgs& a) {
  // 40 / 80: SD-1.5 (8 heads); 64: SD-2-base, the reference's own default (stabilityai/stable-diffusion-2-base, train.py:44,
  // inf4eval.py:65: head dim 64 at every level)
  if (a.D != 40 && a.D != 64 && a.D != 80) return false;
  // d = 64: only the long self-attention launches (64x64 level 478 -> 412 us, 32x32 level equal); below that and for the 77 text keys
  // the 16x16x32 kernel measures the same or a little better (profiles/r04/attn_sd2_microbench.txt)
  if (a.D == 64) return a.Nq >= 1024 && a.Nk >= 1024;
  return a.Nq >= 256 && a.Nk >= 64;
}

int attention_x32_launch(const AttnArgs& a, hipStream_t stream) {
  census(CK_ATTN_X32);
  // short key ranges (cross-attention): keys staged once, waves stream query blocks.  DFH_ATTN_XS=0 turns it off (A/B).
  // d = 64 never arrives here: attention_x32_eligible admits it only with Nk >= 1024
  const bool xs_off = !WalkKnobs::get().attn_xs;
  if (!xs_off && a.Nk <= 2 * KVT && a.lse == nullptr) {
    if (a.D == 40) return launch_xs<40, 2>(a, stream);
    if (a.D == 80) return launch_xs<80, 1>(a, stream);
  }
#ifdef DFH_PROBES   // experiment instantiations (one / four query blocks per wave, phase stamps): probe builds only (scripts/probes/Makefile)
  const int variant = WalkKnobs::get().attn_variant;   // DFH_ATTN_VARIANT: experiments
  switch (a.D) {
    case 40:
      if (variant == 9) return x32_launch_stamped(a, stream, launch_x32<40, 2, 2, true>);   // diagnosis: one launch with the phase stamps
      if (variant == 1) return launch_x32<40, 1, 3>(a, stream);      // experiments: one 32-query block per wave at 3 / 4 waves per SIMD
      if (variant == 2) return launch_x32<40, 1, 4>(a, stream);
      // four blocks per wave, ONE wave per SIMD: 14 fragment reads per 56 MFMAs.  Round 2, plain order: 524 vs 458 us; round 5, with the in-wave
      // software pipeline of the steady-state tiles (x32_tile_pipelined): 506 vs 473 us -- a wave does not overlap its own MFMAs with its own VALU issue
      if (variant == 3 && a.Nq >= 512 && a.Nk >= 128) return launch_x32<40, 4, 1>(a, stream);
      break;
    case 80:
      if (variant == 1) return launch_x32<80, 1, 3>(a, stream);
      break;
    default: break;
  }
#endif
  switch (a.D) {
    case 40: return launch_x32<40, 2, 2>(a, stream);
    case 64: {
      const int qb64 = WalkKnobs::get().attn_qb64;     // DFH_ATTN_QB64: probe knob
      return qb64 == 1 ? launch_x32<64, 1, 2>(a, stream) : launch_x32<64, 2, 2>(a, stream);
    }
    case 80: return launch_x32<80, 1, 2>(a, stream);
    default: break;
  }
  set_error("attention_x32_launch: unsupported head dim");
  return -1;
}

}  // namespace dfh

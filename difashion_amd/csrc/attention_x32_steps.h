// The tile steps of the 32x32x16 attention kernels (attention_x32.hip: the streaming kernel and the short-key kernel; the layouts and
// the reasons for them are explained at the top of that file).  Every step is a forced-inline function over the geometry X32Geom<D> and
// the per-wave state X32Wave<D, QB>, so the state stays in registers; the two kernels are their own control flow over these steps and
// cannot drift apart in the mask slot, the swizzle, the running offset or the order of the floating-point operations.
#pragma once
#include "dfh_common.h"
#include "attention.h"

namespace {

typedef __attribute__((ext_vector_type(16))) float f32x16_t;

constexpr int KVT = 64;               // keys per LDS tile (two 32-key MFMA blocks)
constexpr float THR = 8.0f;           // deferred max: rescale when a score exceeds the running max by 2^8 (log2 domain)
constexpr float MASK_Q = -30000.0f;   // Q-side value of the mask slot (bf16-representable to 3 digits; exp2 -> 0)

template <int D> struct X32Geom {
  static_assert(D % 8 == 0, "head dim must be a multiple of 8");
  static constexpr int DCH = D / 8;                        // 16-byte data chunks per K row
  static constexpr int KS = (D + 2 + 15) / 16;             // 16-deep contraction steps incl. the two bookkeeping slots
  static constexpr int NCH = 2 * KS;                       // chunks per K row in LDS (data + pad chunk + zero chunks)
  // LSUM (head dims that are whole 32-row blocks of O^T, d = 64: SD-2-base): the ones row of V^T would open a block of its own -- a third
  // of the P.V MFMAs and 16 accumulator registers per query block for ONE useful row (the instantiation spilled 13 VGPRs).  The softmax
  // denominator is summed on the VALU instead: one v_dot2_f32_bf16 per packed pair of probabilities against (1, 1), i.e. the sum of the
  // ROUNDED probabilities the MFMA multiplies, exactly what the ones row delivers; each lane half sums the keys it holds.
  static constexpr bool LSUM = D % 32 == 0;
  static constexpr int DB = LSUM ? D / 32 : (D + 1 + 31) / 32;   // 32-row blocks of O^T (incl. the ones row unless LSUM)
  static constexpr int KROW = NCH <= 8 ? 128 : 256;        // K row stride (bytes)
  static constexpr int K_BYTES = KVT * KROW;
  static constexpr int VROWS = D + 2;                      // data rows, the ones row (D), the zero row (D + 1)
  static constexpr int V_BYTES = VROWS * 128;
  static constexpr int BUF = K_BYTES + V_BYTES;
  static constexpr int PAD_KS = DCH / 2, PAD_HI = DCH & 1; // fragment (k-step, lane half) holding slots D, D + 1
  static constexpr int NKI = (KVT * DCH + 255) / 256;      // K staging chunks per thread
  static constexpr int NVI = (D * 8 + 255) / 256;          // V^T staging chunks per thread
  static constexpr int LR = D % 32;                        // row of the softmax denominator inside O^T block D / 32
  static constexpr int L_HI = (LR >> 2) & 1, L_REG = (LR & 3) | ((LR >> 3) << 2);
  static_assert((D % 8) == 0 && (D + 1) / 8 == DCH, "slots D, D+1 must share one chunk");
};

template <int KROW> DFH_DEVICE int k_swz(int key) { return KROW == 128 ? ((key >> 1) & 7) : (key & 15); }
DFH_DEVICE int swap23(int i) { return (i & ~12) | ((i & 4) << 1) | ((i & 8) >> 1); }
// byte offsets of 16-byte chunk ch of K row `key` / V^T row `row` inside a tile buffer's K / V^T image (XOR-swizzled)
template <int D> DFH_DEVICE int k_slot(int key, int ch) { return key * X32Geom<D>::KROW + ((ch ^ k_swz<X32Geom<D>::KROW>(key)) << 4); }
DFH_DEVICE int v_slot(int row, int ch) { return row * 128 + ((ch ^ ((row >> 1) & 7)) << 4); }

// what a wave carries across the key tiles of its QB 32-query blocks; lane (query ql = lane & 31, half hi = lane >> 5)
template <int D, int QB> struct X32Wave {
  using G = X32Geom<D>;
  uint4 qf[QB][G::KS];          // Q fragments (B operand of S^T = K . Q^T): d = 16 ks + 8 hi .. + 8, pre-scaled by scale * log2(e);
                                // the pad chunk holds {-m, MASK_Q, 0 ...}
  f32x16_t o[G::DB][QB];        // O^T accumulators: O[q][d = 32 db + 8 (r >> 2) + 4 hi + (r & 3)]
  float m_run[QB];              // the running offset m (bf16-exact: it rides in a contraction slot of Q)
  float l_acc[QB];              // LSUM: this lane half's part of the softmax denominator
};

// fragment read offsets (fixed per lane)
template <int D> struct X32Frag {
  int k_off[X32Geom<D>::KS];                               // K fragment of k-step ks inside a 32-key block
  int v_row[X32Geom<D>::DB], v_sw[X32Geom<D>::DB];         // V^T row (bytes) and its swizzle of O^T block db
};
template <int D> DFH_DEVICE X32Frag<D> x32_frag(int ql, int hi) {
  using G = X32Geom<D>;
  X32Frag<D> f;
  const int kkey = swap23(ql);                    // K row of S^T row slot ql inside a 32-key block
#pragma unroll
  for (int ks = 0; ks < G::KS; ++ks) f.k_off[ks] = k_slot<D>(kkey, 2 * ks + hi);
#pragma unroll
  for (int db = 0; db < G::DB; ++db) {
    const int pr = min(db * 32 + ql, D + 1);      // rows beyond the ones row read the zero row
    f.v_row[db] = pr * 128; f.v_sw[db] = (pr >> 1) & 7;
  }
  return f;
}

// constant parts of a tile buffer: K chunks DCH .. NCH-1 ({1, mask, 0 ..} then zeros), V^T ones row and zero row.
// first_masked = first key of the tile that lies beyond Nk (KVT: none)
template <int D> DFH_DEVICE void x32_store_const(unsigned char* Ks, int tid, int first_masked) {
  using G = X32Geom<D>;
  constexpr int NC = G::NCH - G::DCH;
  unsigned char* Vs = Ks + G::K_BYTES;
  for (int idx = tid; idx < KVT * NC; idx += 256) {
    const int key = idx / NC, ch = G::DCH + (idx - key * NC);
    uint4 v = uint4{0u, 0u, 0u, 0u};
    if (ch == G::DCH) v.x = key >= first_masked ? DFH_H16_ONE2 : DFH_H16_ONE_LO;      // {1.0, mask}
    *(uint4*)(Ks + k_slot<D>(key, ch)) = v;
  }
  if (tid < 16) {
    const int row = D + (tid >> 3), ch = tid & 7;
    const uint32_t w = row == D ? DFH_H16_ONE2 : 0u;
    *(uint4*)(Vs + v_slot(row, ch)) = uint4{w, w, w, w};
  }
}

// ragged tail of a V^T chunk: zero the padding keys valid .. 7 (they may hold anything, NaN included)
DFH_DEVICE void x32_zero_tail(uint4& v, int valid) {
  uint32_t* w = (uint32_t*)&v;
#pragma unroll
  for (int e = 0; e < 8; ++e)
    if (e >= valid) w[e >> 1] &= (e & 1) ? 0x0000ffffu : 0xffff0000u;
}

// the raw Q chunks of this lane for the query blocks from q0 on (zeros beyond D and beyond Nq), and the fragments made of them
template <int D, int QB>
DFH_DEVICE void x32_fetch_q(uint4 (&qraw)[QB][X32Geom<D>::KS], const AttnArgs& a, const bf16_t* Qb, int q0, int ql, int hi) {
#pragma unroll
  for (int qb = 0; qb < QB; ++qb) {
    const int q = q0 + qb * 32 + ql;
#pragma unroll
    for (int ks = 0; ks < X32Geom<D>::KS; ++ks) {
      const int ch = 2 * ks + hi;
      qraw[qb][ks] = uint4{0u, 0u, 0u, 0u};
      if (ch < X32Geom<D>::DCH && q < a.Nq) qraw[qb][ks] = *(const uint4*)(Qb + (long)q * a.ldq + ch * 8);
    }
  }
}
template <int D, int QB>
DFH_DEVICE void x32_q_frags(X32Wave<D, QB>& w, const uint4 (&qraw)[QB][X32Geom<D>::KS], const AttnArgs& a, int q0, int ql, int hi) {
  const float c = a.scale * 1.44269504088896340736f;
#pragma unroll
  for (int qb = 0; qb < QB; ++qb) {
    const int q = q0 + qb * 32 + ql;
#pragma unroll
    for (int ks = 0; ks < X32Geom<D>::KS; ++ks) {
      uint4 v = uint4{0u, 0u, 0u, 0u};
      const int ch = 2 * ks + hi;
      if (ch < X32Geom<D>::DCH && q < a.Nq) {
        float f[8];
        unpack8(qraw[qb][ks], f);
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] *= c;
        v = pack8(f);
      } else if (ch == X32Geom<D>::DCH) {
        v.x = pack2bf(0.0f, MASK_Q);
      }
      w.qf[qb][ks] = v;
    }
  }
}
// the pad chunk of query block qb: contraction slot D = neg_m (minus the running offset), slot D + 1 = the mask value
template <int D, int QB> DFH_DEVICE void x32_set_pad(X32Wave<D, QB>& w, int qb, float neg_m, int hi) {
  using G = X32Geom<D>;
  if (hi == G::PAD_HI) w.qf[qb][G::PAD_KS].x = pack2bf(neg_m, MASK_Q);
}
template <int D, int QB> DFH_DEVICE void x32_reset(X32Wave<D, QB>& w, int hi) {
#pragma unroll
  for (int db = 0; db < X32Geom<D>::DB; ++db)
#pragma unroll
    for (int qb = 0; qb < QB; ++qb)
#pragma unroll
      for (int r = 0; r < 16; ++r) w.o[db][qb][r] = 0.f;
#pragma unroll
  for (int qb = 0; qb < QB; ++qb) {
    w.m_run[qb] = 0.f; w.l_acc[qb] = 0.f;
    x32_set_pad(w, qb, 0.0f, hi);
  }
}

// S^T = K . Q'^T - m of one 32-key block (Kb = its first K row in LDS) x [qb] 32 queries
template <int D, int QB>
DFH_DEVICE void x32_scores(f32x16_t (&s)[QB], const X32Wave<D, QB>& w, const X32Frag<D>& fr, const unsigned char* Kb) {
#pragma unroll
  for (int ks = 0; ks < X32Geom<D>::KS; ++ks) {
    const h16x8_t kf = *(const h16x8_t*)(Kb + fr.k_off[ks]);
#pragma unroll
    for (int qb = 0; qb < QB; ++qb) {
      if (ks == 0) {
        f32x16_t z;
#pragma unroll
        for (int r = 0; r < 16; ++r) z[r] = 0.f;
        s[qb] = DFH_MFMA_32x32x16(kf, __builtin_bit_cast(h16x8_t, w.qf[qb][ks]), z, 0, 0, 0);
      } else {
        s[qb] = DFH_MFMA_32x32x16(kf, __builtin_bit_cast(h16x8_t, w.qf[qb][ks]), s[qb], 0, 0, 0);
      }
    }
  }
}

// lane-local maximum of a query block's scores over both 32-key blocks (a tree: four independent chains)
DFH_DEVICE float x32_lane_max(const f32x16_t& s0, const f32x16_t& s1) {
  float c4[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    c4[j] = fmaxf(s0[4 * j], s1[4 * j]);
#pragma unroll
    for (int r = 1; r < 4; ++r) c4[j] = fmaxf(fmaxf(c4[j], s0[4 * j + r]), s1[4 * j + r]);
  }
  return fmaxf(fmaxf(c4[0], c4[1]), fmaxf(c4[2], c4[3]));
}
// O (and the LSUM denominator) of query block qb times alpha
template <int D, int QB> DFH_DEVICE void x32_scale_o(X32Wave<D, QB>& w, int qb, float alpha) {
#pragma unroll
  for (int db = 0; db < X32Geom<D>::DB; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) w.o[db][qb][r] *= alpha;
  if constexpr (X32Geom<D>::LSUM) w.l_acc[qb] *= alpha;
}
// deferred max, BEFORE the exp: lane-local maxima, one wave-uniform test; the running offset only moves when some score exceeds it
// by 2^THR (always on the first tile, where O is still zero and alpha may overflow).  INTEGER: the offset is kept an integer (the
// streaming kernel's fast pass needs that of the offset its first tile leaves).
template <bool INTEGER, int D, int QB>
DFH_DEVICE void x32_deferred_max(X32Wave<D, QB>& w, f32x16_t (&s)[2][QB], bool first, int hi) {
  float mx[QB];
  bool over = false;
#pragma unroll
  for (int qb = 0; qb < QB; ++qb) {
    mx[qb] = x32_lane_max(s[0][qb], s[1][qb]);
    over |= mx[qb] > THR;
  }
  if (!first && !__any(over)) return;
#pragma unroll
  for (int qb = 0; qb < QB; ++qb) {
    const float ml = fmaxf(mx[qb], lane_xor32(mx[qb]));       // both halves of the query's column
    float m_new = w.m_run[qb] + ml;
    if (!first) m_new = fmaxf(m_new, w.m_run[qb]);
    m_new = bf2f(f2bf(INTEGER ? ceilf(m_new) : m_new));       // bf16-exact: it rides in a bf16 contraction slot of Q
    const float delta = m_new - w.m_run[qb];
    w.m_run[qb] = m_new;
    const float alpha = __builtin_amdgcn_exp2f(-delta);
#pragma unroll
    for (int kb = 0; kb < 2; ++kb)
#pragma unroll
      for (int r = 0; r < 16; ++r) s[kb][qb][r] -= delta;
    if (!first) x32_scale_o(w, qb, alpha);
    x32_set_pad(w, qb, -m_new, hi);
  }
}

// P = 2^S of one 32-key block, packed in place into the B fragments of O^T += V^T . P^T
template <int D, int QB> DFH_DEVICE void x32_exp_pack(uint32_t (&pw)[QB][8], X32Wave<D, QB>& w, const f32x16_t (&s)[QB]) {
#pragma unroll
  for (int qb = 0; qb < QB; ++qb)
#pragma unroll
    for (int r = 0; r < 16; r += 2) {
      pw[qb][r >> 1] = pack2bf(__builtin_amdgcn_exp2f(s[qb][r]), __builtin_amdgcn_exp2f(s[qb][r + 1]));
      if constexpr (X32Geom<D>::LSUM) w.l_acc[qb] = h16_dot2(pw[qb][r >> 1], DFH_H16_ONE2, w.l_acc[qb]);
    }
}
// O^T += V^T . P^T over 32-key block kb of the tile whose V^T image is Vs
template <int D, int QB>
DFH_DEVICE void x32_pv(X32Wave<D, QB>& w, const X32Frag<D>& fr, const unsigned char* Vs, int kb, int hi, const uint32_t (&pw)[QB][8]) {
#pragma unroll
  for (int m2 = 0; m2 < 2; ++m2)
#pragma unroll
    for (int db = 0; db < X32Geom<D>::DB; ++db) {
      const h16x8_t vf = *(const h16x8_t*)(Vs + fr.v_row[db] + (((kb * 4 + m2 * 2 + hi) ^ fr.v_sw[db]) << 4));
#pragma unroll
      for (int qb = 0; qb < QB; ++qb) {
        const uint4 pv = uint4{pw[qb][4 * m2], pw[qb][4 * m2 + 1], pw[qb][4 * m2 + 2], pw[qb][4 * m2 + 3]};
        w.o[db][qb] = DFH_MFMA_32x32x16(vf, __builtin_bit_cast(h16x8_t, pv), w.o[db][qb], 0, 0, 0);
      }
    }
}

// the softmax denominator of query block qb as this lane sees it, and combined over the two lane halves
template <int D, int QB> DFH_DEVICE float x32_den(const X32Wave<D, QB>& w, int qb) {
  if constexpr (X32Geom<D>::LSUM) return w.l_acc[qb];
  else return w.o[D / 32][qb][X32Geom<D>::L_REG];
}
template <int D, int QB> DFH_DEVICE float x32_den_total(const X32Wave<D, QB>& w, int qb, int hi) {
  const float lv = x32_den(w, qb), lo = lane_xor32(lv);
  if constexpr (X32Geom<D>::LSUM) return lv + lo;             // the two halves hold different keys of the query
  else return hi == X32Geom<D>::L_HI ? lv : lo;               // lanes of half L_HI hold it; the other half holds a zero row of O^T
}
// this lane's part of output row `orow` (elements from the start of O) of query block qb, times inv
template <int D, int QB> DFH_DEVICE void x32_store_row(const AttnArgs& a, const X32Wave<D, QB>& w, int qb, long orow, float inv, int hi) {
#pragma unroll
  for (int db = 0; db < X32Geom<D>::DB; ++db)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      const int d0 = db * 32 + g * 8 + hi * 4;
      const f32x16_t& o = w.o[db][qb];
      if (d0 < D) attn_store4(a, orow, d0, o[4 * g] * inv, o[4 * g + 1] * inv, o[4 * g + 2] * inv, o[4 * g + 3] * inv);
    }
}

}  // namespace

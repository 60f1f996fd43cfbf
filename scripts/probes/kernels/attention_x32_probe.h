// Probe-only parts of the 32x32x16 attention kernel (difashion_amd/csrc/attention_x32.hip includes this under -DDFH_PROBES only):
// the in-wave software pipeline of the QB = 4 instantiation (DFH_ATTN_VARIANT=3), which lost its same-box comparison in rounds 2 and 5,
// and the host side of the phase stamps (DFH_ATTN_VARIANT=9).  Both work on the product's tile steps and state (attention_x32_steps.h).
#pragma once
#include "attention_x32_steps.h"

#include <cstdio>

namespace {

// ---- four query blocks per wave, ONE wave per SIMD (QB = 4, steady-state tiles): nothing else on the SIMD can fill the matrix pipe
//      while this wave runs its exponentials, so the tile is software-pipelined INSIDE the wave, in source order and pinned there
//      by scheduling barriers: every MFMA of a product is followed by a slice of the exponentials of the PREVIOUS score block --
//      S(kb 0) | S(kb 1) + exp of the first key half of block 0 | P.V(block 0, keys 0-15) + the second half | P.V(block 0, keys
//      16-31) + exp(block 1, first half) | P.V(block 1, 0-15) + exp(block 1, second half) | P.V(block 1, 16-31).  An MFMA occupies
//      the pipe for 32 cycles after a 4-cycle issue; the VALU instructions behind it issue in its shadow.  Each K / V^T fragment
//      read feeds FOUR MFMAs (14 reads per 56 MFMAs; the two-block kernel: 14 per 28).
// One tile (K / V^T images Ks / Vs) without a max check; mark(1..3) are the kernel's phase stamps.
template <int D, int QB, class Mark>
DFH_DEVICE void x32_tile_pipelined(X32Wave<D, QB>& w, const X32Frag<D>& fr, const unsigned char* Ks, const unsigned char* Vs, int hi, Mark mark) {
  using G = X32Geom<D>;
  constexpr int KS = G::KS, DB = G::DB, KROW = G::KROW;
  f32x16_t s[2][QB];
  uint32_t pw[2][QB][8];
  // unit u of score block kb: query block u & 3, register pair u >> 2 -- units 0..15 are the keys of the first 16-key MFMA (m2 = 0)
  auto exp_unit = [&](int kb, int u) {
    const int qb = u & 3, pi = u >> 2;
    pw[kb][qb][pi] = pack2bf(__builtin_amdgcn_exp2f(s[kb][qb][2 * pi]), __builtin_amdgcn_exp2f(s[kb][qb][2 * pi + 1]));
    if constexpr (G::LSUM)
      w.l_acc[qb] = h16_dot2(pw[kb][qb][pi], DFH_H16_ONE2, w.l_acc[qb]);
  };
  auto fence = [] { __builtin_amdgcn_sched_barrier(0); };
  // S of score block kb, with `units` exponential units of block ekb (from u0 on) spread behind its MFMAs
  auto s_block = [&](int kb, int ekb, int u0, int units) {
    h16x8_t kf[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) kf[ks] = *(const h16x8_t*)(Ks + kb * 32 * KROW + fr.k_off[ks]);
#pragma unroll
    for (int ks = 0; ks < KS; ++ks)
#pragma unroll
      for (int qb = 0; qb < QB; ++qb) {
        // scores in VGPRs (the exponentials read them), the Q fragments -- read-only B operands, 48 registers -- from the AGPR half.
        // No VALU instruction reads a score block before at least four further MFMAs have issued behind the one that completed
        // it (the pipe is serial: 32 cycles each), so the XDL-write -> VALU-read wait states the compiler cannot see are covered.
        if (ks == 0)
          asm volatile(DFH_MFMA_32x32x16_ASM " %0, %1, %2, 0" : "=&v"(s[kb][qb]) : "v"(kf[ks]), "a"(__builtin_bit_cast(h16x8_t, w.qf[qb][ks])));
        else
          asm volatile(DFH_MFMA_32x32x16_ASM " %0, %1, %2, %0" : "+v"(s[kb][qb]) : "v"(kf[ks]), "a"(__builtin_bit_cast(h16x8_t, w.qf[qb][ks])));
        if (units > 0) {
          fence();
          const int from = ((ks * QB + qb) * units) / (KS * QB), upto = ((ks * QB + qb + 1) * units) / (KS * QB);
#pragma unroll
          for (int u = from; u < upto; ++u) exp_unit(ekb, u0 + u);
          fence();
        }
      }
  };
  // P.V of (score block kb, 16-key half m2), with `units` exponential units of block ekb (from u0 on) behind its MFMAs
  auto pv_half = [&](int kb, int m2, int ekb, int u0, int units) {
    h16x8_t vf[DB];
#pragma unroll
    for (int db = 0; db < DB; ++db) vf[db] = *(const h16x8_t*)(Vs + fr.v_row[db] + (((kb * 4 + m2 * 2 + hi) ^ fr.v_sw[db]) << 4));
#pragma unroll
    for (int db = 0; db < DB; ++db)
#pragma unroll
      for (int qb = 0; qb < QB; ++qb) {
        const uint4 pv = uint4{pw[kb][qb][4 * m2], pw[kb][qb][4 * m2 + 1], pw[kb][qb][4 * m2 + 2], pw[kb][qb][4 * m2 + 3]};
        // the O^T accumulators (128 registers) are pinned in the AGPR half of the register file: the VALU never touches them inside
        // the loop (one denominator register per query block aside), while S^T -- which the exponentials read -- stays in VGPRs.
        // The builtin leaves that choice to one per-function switch; with both accumulator sets in VGPRs the allocator shuffled
        // ~300 v_accvgpr_read / write / mov per tile through the VALU this pipeline is built to keep free.
        asm volatile(DFH_MFMA_32x32x16_ASM " %0, %1, %2, %0" : "+a"(w.o[db][qb]) : "v"(vf[db]), "v"(__builtin_bit_cast(h16x8_t, pv)));
        if (units > 0) {
          fence();
          const int from = ((db * QB + qb) * units) / (DB * QB), upto = ((db * QB + qb + 1) * units) / (DB * QB);
#pragma unroll
          for (int u = from; u < upto; ++u) exp_unit(ekb, u0 + u);
          fence();
        }
      }
  };
  fence();
  s_block(0, 0, 0, 0);
  fence();
  s_block(1, 0, 0, 16);
  mark(1);
  pv_half(0, 0, 0, 16, 16);
  pv_half(0, 1, 1, 0, 16);
  mark(2);
  pv_half(1, 0, 1, 16, 16);
  pv_half(1, 1, 0, 0, 0);
  fence();
  // the compiler's hazard recogniser does not look inside inline asm: a VALU read of an accumulator (the denominator check that
  // follows the tile) needs 18 wait states behind the 16-pass MFMA that wrote it
  asm volatile("s_nop 15\n\ts_nop 3" ::: "memory");
  mark(3);
}

// diagnosis (DFH_ATTN_VARIANT=9): one launch of the stamped instantiation, its phase stamps printed as per-phase cycle averages
template <class Launch>
int x32_launch_stamped(const AttnArgs& a, hipStream_t stream, Launch launch) {
  static unsigned long long* buf = nullptr;
  if (!buf && hipMalloc((void**)&buf, 64 * 8 * 8) != hipSuccess) return -1;
  (void)hipMemsetAsync(buf, 0, 64 * 8 * 8, stream);
  AttnArgs b = a; b.prof = buf;
  const int rc = launch(b, stream);
  unsigned long long h[64 * 8];
  (void)hipStreamSynchronize(stream);
  (void)hipMemcpy(h, buf, sizeof(h), hipMemcpyDeviceToHost);
  double ph[6] = {0, 0, 0, 0, 0, 0}; int n = 0;
  for (int t = 4; t < 60; ++t) {
    if (!h[t * 8] || !h[(t + 1) * 8]) continue;
    for (int i = 0; i < 5; ++i) ph[i] += (double)(h[t * 8 + i + 1] - h[t * 8 + i]);
    ph[5] += (double)(h[(t + 1) * 8] - h[t * 8 + 5]); ++n;
  }
  if (n) fprintf(stderr, "[attn prof] cycles per tile (wave 0 of workgroup 0, %d tiles): S-issue %.0f | exp+pack %.0f | PV-issue %.0f | "
                         "stage-store+check %.0f | barrier %.0f | loop-back %.0f\n", n, ph[0] / n, ph[1] / n, ph[2] / n, ph[3] / n, ph[4] / n, ph[5] / n);
  return rc;
}

}  // namespace

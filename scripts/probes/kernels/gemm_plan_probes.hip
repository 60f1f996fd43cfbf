// Probe builds only: where the probe kernels enter the GEMM plan (gemm_plan.hip) and its dispatch (gemm.hip).  Host code.
//   tile ids 11 / 12 = the wave-specialised kernel (gemm_ws.hip, opt-in DFH_GEMM_WS=1), 20 = the halo-patch conv kernel (gemm_halo.hip,
//   DFH_GEMM_HALO=1): both lost their A/B (profiles/r02/gemm_ws_probe.txt; conv3x3 class 6.96 -> 6.93 ms);
//   the persistent GEGLU rows kernel (gemm_geglu.hip, opt-in DFH_GEGLU_ROWS=1) in place of the 256 x 256 tile;
//   tile id 24, or DFH_PERSIST=1 / 2 for every eligible launch with >= 512 / >= 1 tiles = the persistent 128 x 160 kernel (gemm_persist.hip):
//   bit-identical to the tile kernel and 1.2-1.5 x slower (profiles/r06/persistent_lean_gemm.md);
//   tile id 30 = the launch as a register-resident token linear (token_linear.hip).
// All are kept as measurements, not as product code.
#include <string>

#include "gemm_plan.h"
#include "token_linear.h"

namespace dfh {

int gemm_plan_probes(GemmArgs& a, const GemmForce& f, const GemmKnobs& k, GemmPlan& p, bool wide_ok) {
  if (f.token) {
    p.kernel = GK_TOKEN_LINEAR; p.census = -1;
    p.rowstat_bn = a.rowstat ? a.N : 0;
    return 1;
  }
  const bool heur = f.none() && f.split == 0;
  if (wide_ok && !f.deep) {
    const int ws = f.ws ? (gemm_ws_pick(a, 1) ? f.ws : 0) : (heur && k.ws_on) ? gemm_ws_pick(a, 224) : 0;
    const bool halo = gemm_halo_eligible(a) && (f.halo || (p.kernel == GK_WIDE && p.wide == 1 && !f.kernel_pinned() && k.halo_on));
    if (halo) { p.kernel = GK_HALO; return 0; }
    if (ws) { p.kernel = GK_WS; p.bn = ws; return 0; }
  }
  if (p.kernel == GK_BIG_GEGLU && f.tile == 0 && !f.bigg && gemm_geglu_rows_ok(a)) { p.kernel = GK_GEGLU_ROWS; return 0; }   // opt-in DFH_GEGLU_ROWS=1
  if (f.persist) p.tile = kEightWave;
  bool persist = false;
  if (p.kernel == GK_TILE && p.tile == kEightWave && !f.deep && (f.tile == 0 || f.persist)) {
    GemmArgs t = a; GemmPlan q = p;          // gemm_persist_ok looks at the statistics pointers the eight-wave tile would be left with
    gemm_plan_stats(t, k, q);
    persist = gemm_persist_ok(t) && (f.persist || (k.persist_mode != 0 && (long)(a.M / 128) * (a.N / 160) >= (k.persist_mode >= 2 ? 1 : 512)));
  }
  if (f.persist && !persist) { set_error("gemm_launch: tile id 24: this launch cannot run on the persistent kernel (gemm_persist_ok)"); return -1; }
  if (persist) p.kernel = GK_PERSIST;
  return 0;
}

int gemm_launch_probes(const GemmPlan& p, const GemmArgs& a, hipStream_t stream) {
  if (p.kernel == GK_TOKEN_LINEAR) return token_linear_from_gemm(a, stream);
  const GemmWork w = gemm_work(a);
  prof_note_saved(w.saved);
  ProfScope ps(w.cls, w.flops, w.bytes, stream);
  const int rc = p.kernel == GK_HALO ? gemm_halo_launch(a, stream) : p.kernel == GK_WS ? gemm_ws_launch(a, stream, p.bn) :
                 p.kernel == GK_GEGLU_ROWS ? gemm_geglu_rows_launch(a, stream) : gemm_persist_launch(a, stream);
  if (p.kernel == GK_PERSIST) census(CK_GEMM_PERSIST);
  census(p.census);
  if (a.gstat) census(CK_GSTAT_WRITTEN);
  return rc;
}

}  // namespace dfh

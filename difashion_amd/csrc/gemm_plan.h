// Which kernel a gemm_launch runs, as a value.  gemm_plan() (gemm_plan.hip, host code only) takes the decision; gemm_launch (gemm.hip) dispatches
// it.  Everything here is a host rule about WHICH kernel runs -- the kernels, launch_tile and wide_launch_t stay in gemm.hip / gemm_wide.hip.
#pragma once
#include <stddef.h>
#include "gemm.h"
#include "norm.h"   // GN_MAX_CHUNKS: what the consuming GroupNorm kernels accept per (image, group)

namespace dfh {

// force_tile / force_split / force_order of a launch, decoded once (gemm_force_decode) from the public ids (gemm.h GemmForceTile)
struct GemmForce {
  int tile;        // GF_TILE_* 1..5: a gemm_bf16_kernel tile of kGemmTiles; 0 = none (a negative id pins nothing but still switches the heuristics off)
  bool deep;       // GF_8WAVE: the eight-wave 128 x 160 tile, one tile per workgroup
  bool big, bigg;  // GF_BIG / GF_BIG_GEGLU: the 256 x 320 / 256 x 256 eight-wave tiles where the launch can take them
  int wide;        // a gemm_wide_launch variant (GF_WIDE .. GF_WIDE_SIB: 1..4; probe ablations 8..13; unknown ids end in that launcher's refusal)
  int ws;          // probe: the wave-specialised kernel's column tile (160 / 128)
  bool halo, persist, token;   // probe kernels: GF_HALO, GF_PERSIST, GF_TOKEN_LINEAR
  int split, order;
  bool kernel_pinned() const { return wide || ws || halo; }     // an id of the wide family that is still to be resolved against the launch
  bool none() const { return tile == 0 && !kernel_pinned(); }   // (deep / big / bigg / persist are tested by name where they matter)
};
GemmForce gemm_force_decode(int force_tile, int force_split, int force_order);

// every DFH_* switch of the selection; from_env() reads the environment once per process (the table is in DESIGN.md 4.1)
struct GemmKnobs {
  bool deep4_off, deep4_all;   // DFH_DEEP4: unset = the 4-stage ring for every launch of <= 320 workgroups, 1 = batched launches only, 0 = off
  int tmap_xm, tmap_gm;        // DFH_TMAP="xm,gm": pins the tile order of every launch (xm < 0: the measured rules)
  int big_mode;                // DFH_GEMM_BIG: 0 off, 1 convs, 2 + deep linears (default), 3 + all linears
  int bigg_mode;               // DFH_GEMM_BIGG: 0 = no 256 x 256 GEGLU tile
  bool w_blocked_off;          // DFH_W_BLOCKED=0
  int wino_tile;               // DFH_WINO_TILE: tile id of the batched transform-domain GEMM (< 0: the default)
  bool batch_big_off;          // DFH_BATCH_BIG=0
  bool batch_nmajor_off;       // DFH_BATCH_NMAJOR=0
  bool gstat128_off;           // DFH_GSTAT128=0
  bool ws_on, halo_on;         // probe builds: DFH_GEMM_WS=1, DFH_GEMM_HALO=1
  int persist_mode;            // probe builds: DFH_PERSIST
  static GemmKnobs defaults();
  static const GemmKnobs& from_env();
};

enum GemmKernel { GK_TILE = 0, GK_BIG, GK_BIG_GEGLU, GK_WIDE,                       // gemm_bf16_kernel tiles, its 256 x 320 / 256 x 256 tiles, gemm_wide_kernel
                  GK_WS, GK_HALO, GK_GEGLU_ROWS, GK_PERSIST, GK_TOKEN_LINEAR,      // probe builds only (scripts/probes/kernels)
                  GK_COUNT };
struct GemmTile { int bm, bn, stages; };
extern const GemmTile kGemmTiles[6];     // ids 1..5 of force_tile, then the eight-wave 128 x 160 tile (GF_8WAVE, the default)
constexpr int kEightWave = 5;

struct GemmPlan {
  int kernel;               // GemmKernel
  int tile;                 // index into kGemmTiles: the tile that runs (GK_TILE / GK_PERSIST), else the heuristic tile the checks were made against
  int bm, bn, stages, lean; // the instantiation that runs (stages / lean 0 for the probe kernels)
  int wide;                 // GK_WIDE: the gemm_wide_launch variant
  int split;                // K slices; > 1: the split-K reduce follows
  int n_major, tm_xm, tm_gm;
  int gstat_rows;           // pixel rows per statistics chunk the kernel fills a.gstat with (256 / 128), 0 = it cannot (a.gstat is nulled)
  int rowstat_bn;           // column tile of the a.rowstat records, 0 = none (a.rowstat is nulled)
  int census;               // CensusId of the launch
};

// The decision for one launch.  A pure function of its arguments: no HIP call, no census, no profiling, no getenv, no allocation unless it
// refuses.  Does to `a` what the launch needs (rows_per_b, ksteps, ksplit, n_major, tm_xm / tm_gm; gstat / rowstat nulled when the chosen
// kernel cannot write them).  Returns 0, or -1 with the refusal in set_error (worded as gemm_launch's: that is where callers meet it).
int gemm_plan(GemmArgs& a, const GemmForce& f, const GemmKnobs& k, GemmPlan& p);

// pieces of the plan that other rules are built from (gemm_pick_split, gemm.h: the tile and K split a launch gets from its shape alone)
bool gemm_lean_plain(const GemmArgs& a);              // one or two plain K segments of whole 64-channel slices: the LEAN k-loop applies
void gemm_plan_stats(GemmArgs& a, const GemmKnobs& k, GemmPlan& p);   // gstat_rows / rowstat_bn of p.kernel; nulls a.gstat / a.rowstat where it cannot write them
inline bool gstat_chunks_fit(int hw, int rows) { return hw % rows == 0 && hw / rows <= (int)GN_MAX_CHUNKS; }   // chunks of `rows` pixel rows per image

// algorithmic work of a launch for the profile: 2 M N K over the real K, each operand once + the output
struct GemmWork { double flops, saved, bytes; int cls; };
GemmWork gemm_work(const GemmArgs& a);

// one text line per launch: the shape key of `a` as the caller gave it, then the plan -- or the refusal.  DFH_GEMM_PLAN_DUMP and dfh_gemm_plan share it.
const char* gemm_kernel_name(int kernel);
int gemm_plan_format(char* buf, size_t n, const GemmArgs& given, const GemmPlan* p, const char* refusal);

#ifdef DFH_PROBES
// the probe kernels' one entry into the plan (gemm_plan.hip) and into the dispatch (gemm.hip)
// (scripts/probes/kernels/gemm_plan_probes.hip)  gemm_plan_probes sees the product's candidate in p.kernel / p.wide / p.tile and may replace it;
// returns 0 = go on, 1 = the plan is complete, -1 = refused.  gemm_launch_probes runs a plan whose kernel is one of the probe kinds.
int gemm_plan_probes(GemmArgs& a, const GemmForce& f, const GemmKnobs& k, GemmPlan& p, bool wide_ok);
int gemm_launch_probes(const GemmPlan& p, const GemmArgs& a, hipStream_t stream);
#endif
}  // namespace dfh

// Host code only: which kernel, tile, K split, tile order and statistics chunk a gemm_launch gets (gemm_plan.h).  No __global__ code and
// no HIP call in this file; the kernels and their launchers are in gemm.hip / gemm_wide.hip.
#include "gemm_plan.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

namespace dfh {

namespace {
constexpr int BK = 64;      // k-step depth of gemm_bf16_kernel (gemm_kiter.h)
constexpr int BKW = 32;     // ... and of gemm_wide_kernel
constexpr int kNumTiles = 5;                      // ids 1..5 of force_tile; the eight-wave 128 x 160 variant is GF_8WAVE
}  // namespace

// variant ids (force_tile - 1):
//   0: 256x160 8 waves 3 stages   1: 256x128 8 waves 3 stages   2: 128x64 4 waves 3 stages
//   3: 128x160 4 waves 2 stages   4: 128x128 4 waves 2 stages
//   5: 128x160 EIGHT waves (4 x 2, 32 x 80 each) 2 stages, external id 10 (ids 6-9 are the wide kernel) -- the default
//      128 x 160 kernel: issuing a k-step's 36 LDS-DMA pieces costs a wave ~100 cycles apiece during which it issues no
//      MFMA, so with one wave per SIMD (a 4-wave workgroup alone on its CU: the 256-tile launches of the 16x16 level) a
//      k-step takes 0.93 us against 0.29 us of MFMA work; two waves per SIMD overlap the two (0.75 us; 12.6 / 25.0 / 69.2
//      vs 15.0 / 28.3 / 78.5 us on 4096 x 1280 x {320, 1280, 5120}), and at two workgroups per CU (122 VGPRs: 16 waves
//      fit) it still wins 4-5 % (scripts/gemm_deepring_probe.py).  A 4-stage ring on the 4-wave tile gained nothing.
const GemmTile kGemmTiles[6] = {{256, 160, 3}, {256, 128, 3}, {128, 64, 3}, {128, 160, 2}, {128, 128, 2}, {128, 160, 2}};

GemmForce gemm_force_decode(int force_tile, int force_split, int force_order) {
  GemmForce f{};
  f.split = force_split; f.order = force_order;
  switch (force_tile) {
    case GF_8WAVE: f.deep = true; break;
    case GF_WS_160: f.ws = 160; break;
    case GF_WS_128: f.ws = 128; break;
    case GF_HALO: f.halo = true; break;
    case GF_BIG: f.big = true; break;
    case GF_BIG_GEGLU: f.bigg = true; break;
    case GF_PERSIST: f.persist = true; break;
    case GF_TOKEN_LINEAR: f.token = true;      // a probe kernel; the product build lets the id through to the wide launcher like any unknown one
    default:
      if (force_tile > kNumTiles) f.wide = force_tile - GF_WIDE + 1;
      else f.tile = force_tile;
  }
  return f;
}

GemmKnobs GemmKnobs::defaults() {
  GemmKnobs k{};
  k.deep4_all = true; k.tmap_xm = -1; k.big_mode = 2; k.bigg_mode = 1; k.wino_tile = -1;
  return k;
}

const GemmKnobs& GemmKnobs::from_env() {
  static const GemmKnobs knobs = [] {
    GemmKnobs k = defaults();
    const auto is = [](const char* name, char c) { const char* e = getenv(name); return e && e[0] == c; };
    const auto num = [](const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; };
    k.deep4_off = is("DFH_DEEP4", '0');
    k.deep4_all = !is("DFH_DEEP4", '1');       // 1: batched launches only (A/B: 16.32 -> 16.25 ms with single launches too)
    if (const char* e = getenv("DFH_TMAP")) { const char* c = strchr(e, ','); k.tmap_xm = atoi(e); k.tmap_gm = c ? atoi(c + 1) : 0; }
    k.big_mode = num("DFH_GEMM_BIG", k.big_mode);
    k.bigg_mode = num("DFH_GEMM_BIGG", k.bigg_mode);
    k.w_blocked_off = is("DFH_W_BLOCKED", '0');
    k.wino_tile = num("DFH_WINO_TILE", k.wino_tile);
    k.batch_big_off = is("DFH_BATCH_BIG", '0');
    k.batch_nmajor_off = is("DFH_BATCH_NMAJOR", '0');
    k.gstat128_off = is("DFH_GSTAT128", '0');
    k.ws_on = is("DFH_GEMM_WS", '1'); k.halo_on = is("DFH_GEMM_HALO", '1'); k.persist_mode = num("DFH_PERSIST", 0);
    return k;
  }();
  return knobs;
}

int gemm_count_ksteps(const GemmArgs& a) {
  int n = a.ntaps * ((a.conv_c + BK - 1) / BK);
  for (int i = 0; i < a.nplain; ++i) n += (a.p_c[i] + BK - 1) / BK;
  return n;
}

int gemm_wide_ksteps(const GemmArgs& a) {
  int n = a.ntaps * ((a.conv_c + BKW - 1) / BKW);
  for (int i = 0; i < a.nplain; ++i) n += (a.p_c[i] + BKW - 1) / BKW;
  return n;
}

// one plain K segment of a multiple of 64 channels, W rows long enough: the LEAN k-loop applies
bool gemm_lean_plain(const GemmArgs& a) {
  // same-box A/B (scripts/gemm_lean_probe.py): 4096 x 1280 x {1280, 5120} 26.8 -> 25.7 / 77 -> 71 us (one workgroup per CU),
  // 0-3 % at two workgroups per CU -- the LDS-DMA issue itself (~100 cycles per 1-KB piece), not its address arithmetic,
  // is what paces the loop
  if (a.ntaps != 0 || a.nplain < 1 || a.p_c[0] % BK != 0 || a.p_c[0] <= 0) return false;
  // 32-bit byte offsets from the segment / weight-plane bases inside the kernel
  const double amax = (double)a.M * std::max(a.p_c[0], a.nplain > 1 ? a.p_c[1] : 0) * 2.0, wmax = (double)a.N * a.ldw * 2.0;
  if (amax >= 4.0e9 || wmax >= 4.0e9) return false;
  return a.nplain == 1 || (a.p_c[1] % BK == 0 && a.p_c[1] > 0);
}

int gemm_pick_split(const GemmArgs& a, int* tile_out) {
  // column tile: 160 when it divides N (320/640/1280/...), else 128 (GEGLU needs 32-aligned pairs), 64 for N <= 64
  const bool geglu = a.act == ACT_GEGLU;
  const bool n160 = !geglu && (a.N % 160 == 0 || (a.N % 128 != 0 && a.N > 128));
  // Measured on MI355X (scripts/gemm_microbench.py): the 128-row / 4-wave / 2-stage variants at two
  // workgroups per CU beat the 256-row / 8-wave / 3-stage ring on every U-Net shape except the 8x8 level.
  const int ksteps = gemm_count_ksteps(a);
  if (gemm_act_is_xact(a.act)) {       // only the XACT instantiations of the eight-wave 128 x 160 tile know these activations; the reduce kernel does not
    if (tile_out) *tile_out = kEightWave;
    return 1;
  }
  int tile;
  if (a.N <= 64 && !geglu) tile = 2;
  else if (a.M > 128 && a.M <= 1024 && ksteps >= 64) tile = n160 ? 0 : 1;
  else tile = n160 ? kEightWave : 4;   // same-box A/B over the whole step: linear class 7.65 -> 7.33 ms, conv3x3 6.92 -> 6.87 ms
  const GemmTile ti = kGemmTiles[tile];
  const int blocks = ((a.M + ti.bm - 1) / ti.bm) * ((a.N + ti.bn - 1) / ti.bn);
  int split = 1;
  if (!geglu && blocks < 384 && ksteps >= (a.ntaps ? 64 : 160)) {     // plain K = 5120 (80 k-steps) loses: 67 -> 72 us
    // deep-K launches that leave CUs idle or at one workgroup each (16x16 level at batch 16: 256 tiles; 8x8 level: 64-128):
    // split K until about 512 workgroups are resident.  The slab round trip pays for itself on the 3x3 convs
    // (M=4096: 205 -> 149 us with 2 slices; M=2048: 111 -> 78 us with 4; scripts/gemm_split_probe*.py)
    const int target = ti.bm == 256 ? 256 : 512;        // the 8-wave 256-row tiles run one workgroup per CU
    split = std::max(1, std::min((target + blocks / 2) / blocks, ksteps / 16));
  } else if (!geglu && blocks < 160 && ksteps >= 16) {
    // shallow K (1x1 / linear): more than two slices cost more in slab traffic than they win
    split = std::min({(256 + blocks - 1) / blocks, ksteps / 8, 64});
    if (split < 1) split = 1;
  }
  if (tile_out) *tile_out = tile;
  return split;
}

size_t gemm_partial_floats(const GemmArgs& a) {
  if (a.nbatch > 1) return 0;     // batched launches never split K
  const int s = gemm_pick_split(a, nullptr);
  return s > 1 ? (size_t)s * a.M * a.N : 0;
}

// a second destination: single pass, n_split a whole number of column tiles of `tile`
static bool out2_fits(const GemmArgs& a, int tile, int split) {
  return split == 1 && a.n_split > 0 && a.n_split % kGemmTiles[tile].bn == 0 && a.out_mode == OUT_BF16 && a.act != ACT_GEGLU && !a.resid;
}
// the folded-LayerNorm fix-up: the split-K reduce does not implement it, nor does the unstaged GEGLU branch
static bool ln_single_pass(const GemmArgs& a, int split) { return split == 1 && !a.rowvec && !a.resid; }
static bool ln_geglu_staged(const GemmArgs& a) { return a.act != ACT_GEGLU || (a.ld_out & 7) == 0; }

// (both ask the HEURISTIC tile and split, as their callers do before any launch exists)
bool gemm_out2_ok(GemmArgs a) {
  int tile;
  const int split = gemm_pick_split(a, &tile);
  return a.out2 != nullptr && a.n_split < a.N && out2_fits(a, tile, split);
}

bool gemm_ln_consumer_ok(GemmArgs a) {
  return ln_single_pass(a, gemm_pick_split(a, nullptr)) && ln_geglu_staged(a) && (a.act != ACT_GEGLU || a.N % 32 == 0) && a.ntaps == 0;
}

// Tile order of a launch (dfh_common.h tile_coords) for a bm x bn tile.  DFH_TMAP="xm,gm" pins it for every launch (probe).
// The rules are the measured ones (scripts/pmc_traffic_calib.sh + scripts/tile_order_probe.py, profiles/r02): launch TIME does
// not depend on the order (+-2 %: the over-fetched bytes come out of the Infinity Cache), fabric traffic does --
//   * many column tiles over a weight matrix that cannot stay in one XCD's L2 (GEGLU projections at the 32x32 / 16x16 levels:
//     40 / 80 column tiles, 6.5 / 26 MB of weights): groups of 8 row tiles walked column by column, FETCH 11-12 x -> 5 x the
//     algorithmic bytes;
//   * single-pass 3x3 convs with few column tiles and big weights (32x32 level: 128 x 4 tiles, 7-22 MB): a 4 x 2 grid of XCDs
//     (each XCD streams half of the weights instead of all of them), 3.0 / 4.2 x -> 2.5 / 3.1 x; not at the 64x64 level, where
//     splitting the column tiles over XCDs doubles the (20 x larger) pixel traffic.
static void gemm_pick_tile_order(GemmArgs& a, const GemmKnobs& k, int split, int bm, int bn) {
  a.tm_xm = 0; a.tm_gm = 0;
  if (k.tmap_xm >= 0) {         // probe knob; xm must divide the 8 XCDs (anything else would enumerate some tiles twice and others never)
    a.tm_xm = (k.tmap_xm == 1 || k.tmap_xm == 2 || k.tmap_xm == 4 || k.tmap_xm == 8) ? k.tmap_xm : 0; a.tm_gm = k.tmap_gm; return;
  }
  if (split > 1 || a.n_major) return;
  double kk = (double)a.ntaps * a.conv_c;
  for (int i = 0; i < a.nplain; ++i) kk += a.p_c[i];
  const double w_bytes = (double)a.N * kk * 2.0;
  const double a_bytes = a.ntaps ? (double)(a.M / (a.Hout * a.Wout)) * a.Hin * a.Win * a.conv_c * 2.0 : (double)a.M * kk * 2.0;
  const int ntm = (a.M + bm - 1) / bm, ntn = (a.N + bn - 1) / bn;
  if (w_bytes <= 2.0e6 || ntm < 16) return;          // the weights stay resident in every L2: nothing to order
  if (ntn >= 16) { a.tm_gm = 8; return; }
  if (!a.ntaps) return;
  // few column tiles: an xm x (8 / xm) grid of XCDs fetches (8 / xm) x the pixels + xm x the weights in total (xm = 8 is the
  // legacy order: every XCD streams all the weights).  Measured 4 x 2 against 8 x 1: better on the 32x32-level convs (21 + 8 x 7
  // MB -> 2 x 21 + 4 x 7), WORSE at 64x64 where the pixels outweigh the weights 20 : 1 -- so pick the minimum of the model.
  int best = 8; double cost = a_bytes + 8.0 * w_bytes;
  for (int xm = 4; xm >= 2; xm >>= 1) {
    if (ntm % xm || ntn % (8 / xm)) continue;
    const double c = (8.0 / xm) * a_bytes + xm * w_bytes;
    if (c < 0.95 * cost) { cost = c; best = xm; }
  }
  if (best != 8) { a.tm_xm = best; a.tm_gm = 8; }
}

// whole rounds of the 256 CUs for the one-workgroup-per-CU tiles (a 257th tile would run alone for a whole round)
static bool whole_rounds(long tiles, long always_from) {
  const long rem = tiles % 256;
  return tiles >= 224 && (rem == 0 || rem >= 224 || tiles >= always_from);
}

// Launches for the 256 x 320 tile.  DFH_GEMM_BIG=0 turns it off, =3 also sends the short plain linears there (A/B).
static bool gemm_big_pick(const GemmArgs& a, const GemmKnobs& k) {
  if (k.big_mode == 0) return false;
  if (a.out_mode != OUT_BF16 || a.act == ACT_GEGLU || a.ln_stat) return false;
  if (a.N % 320 != 0 || (a.ld_out & 7) || (a.resid && (a.ld_res & 7))) return false;
  if (a.ksteps < 16 && (a.ntaps || k.big_mode < 3)) return false;   // conv_in (K = 72): prologue + four-pass epilogue outweigh two k-steps (34.6 vs 24.3 us)
  if (a.ntaps == 0 && k.big_mode < 2) return false;
  return whole_rounds((long)((a.M + 255) / 256) * (a.N / 320), 1024);
}

// GEGLU projections for the 256 x 256 tile: whole rounds of the CUs, as above.  DFH_GEMM_BIGG=0 turns it off (A/B).
static bool gemm_big_geglu_pick(const GemmArgs& a, const GemmKnobs& k) {
  if (k.bigg_mode == 0 || a.act != ACT_GEGLU || a.out_mode != OUT_BF16 || a.resid || a.rowvec) return false;
  if (a.N % 256 != 0 || (a.ld_out & 7)) return false;
  // (16x16 level: 640 tiles = 2.5 rounds, still 5 % ahead of the 256 x 128 tile in isolation: profiles/r03/geglu_tile_probe.txt)
  return whole_rounds((long)((a.M + 255) / 256) * (a.N / 256), 512);
}

// Batched launches (Winograd planes, phase planes of an upsample conv) for the 256 x 320 eight-wave tile: planes of at least 512 rows whose
// tiles together make whole rounds of the CUs (16x16-level Winograd: 16 planes x 16 tiles = 256 workgroups, 78.7 us on the 128 x 160 tile -> 67.1 us).
// DFH_BATCH_BIG=0 turns it off (A/B).
static bool batched_big_pick(const GemmArgs& a, const GemmKnobs& k) {
  if (k.batch_big_off || a.nbatch <= 1 || a.M < 512 || a.N % 320 != 0) return false;
  return whole_rounds((long)((a.M + 255) / 256) * (a.N / 320) * a.nbatch, 1024);
}

bool wino_blocked(int N, int C) {
  return !GemmKnobs::from_env().w_blocked_off && N % 160 == 0 && C % 64 == 0;   // the batched launch then runs on a LEAN instantiation (128 x 160 eight-wave / 256 x 320)
}

int wino_gemm_tile(const GemmArgs&) {
  const int pin = GemmKnobs::from_env().wino_tile;      // probe
  return pin >= 0 ? pin : 0;
}

// bf16 row-major output, no GEGLU / split-K, 16-byte aligned rows, and enough tiles to give every CU its two workgroups
// 1 = 256 x 160, 4 = 256 x 128 (N a multiple of 128 but not of 160), 0 = not eligible; 2 / 3 are experiment variants
int gemm_wide_pick(const GemmArgs& a) {
  if (a.out_mode != OUT_BF16) return 0;
  if (a.ln_stat && !(a.act == ACT_GEGLU && a.N % 128 == 0)) return 0;   // only the in-register GEGLU epilogue implements the LayerNorm fix-up
  if (a.act == ACT_GEGLU && (a.resid || a.rowvec)) return 0;
  if ((a.N & 7) || (a.ld_out & 7) || (a.resid && (a.ld_res & 7))) return 0;
  // GEGLU: the 256 x 128 sibling keeps whole (value, gate) block pairs inside a wave -> epilogue in registers
  if (a.act == ACT_GEGLU && a.N % 128 == 0) return (long)((a.M + 255) / 256) * (a.N / 128) >= 448 ? 4 : 0;
  if (a.act == ACT_GEGLU && a.N % 160 != 0) return 0;
  if (a.N % 160 != 0 && a.N % 128 == 0) {       // 128 / 256 / 512 / 1024 output channels (the VAE): the 256 x 128 sibling
    return (long)((a.M + 255) / 256) * (a.N / 128) >= 448 ? 4 : 0;
  }
  if (a.N % 160 != 0 && a.N < 640) return 0;
  // plain linears / 1x1 convs (no taps): the eight-wave 128 x 160 kernel of gemm.hip is as fast or faster since its epilogue
  // stopped serialising the bias loads and its residual loads moved behind the prologue (scripts/gemm_shortk2_probe.py,
  // profiles/r02/gemm_shortk2_probe.txt: 65536 x 960 x 320 72.7 -> 60.2 us, 65536 x 320 x 1280 + residual 75.3 -> 67.7 us,
  // 16384 x 1920 x 640 63.4 -> 47.6 us); the 3x3 convs keep the wide tile, and so do the K = 320 linears with a residual, whose
  // coalesced one-pass-ahead residual reads win (same-box A/B: 31.4 vs 33.7 us)
  // (with row statistics for a folded LayerNorm the eight-wave kernel wins again: the 256-row epilogue pays ~4.5 us per launch for them)
  if (a.ntaps == 0 && a.N % 160 == 0 && !(a.resid && a.nplain == 1 && a.p_c[0] <= 320 && !a.rowstat)) return 0;
  const long nt = (a.N + 159) / 160;
  // the 128-row sibling (variant 2) is kept for experiments only: at equal tile size the 64-deep two-stage kernel of
  // gemm.hip wins (848 vs 724 TFLOP/s on conv 320->320 @64): the gain of this file is the larger tile
  return (long)((a.M + 255) / 256) * nt >= 448 ? 1 : 0;
}

bool gemm_wide_eligible(const GemmArgs& a) {
  if (a.out_mode != OUT_BF16) return false;
  if (a.act == ACT_GEGLU && (a.N % 160 != 0 || a.resid || a.rowvec)) return false;
  if ((a.N & 7) || (a.ld_out & 7) || (a.resid && (a.ld_res & 7))) return false;
  if (a.N % 160 != 0 && a.N < 640) return false;
  const long tiles = (long)((a.M + 255) / 256) * ((a.N + 159) / 160);
  return tiles >= 448;
}

// Output statistics of the chosen kernel; nulls a.gstat / a.rowstat when it cannot write them.
//   gstat (the consuming GroupNorm's): the 256-row epilogues (256 x 160 wide, 256 x 320) and the staged epilogue of the eight-wave 128 x 160
//     tile write them, on full tiles inside one image; gstat_rows = pixel rows per statistics chunk
//   rowstat (a LayerNorm folded into the consumer): the staged bf16 epilogue of gemm_bf16_kernel and the 256-row epilogue, on whole column tiles
void gemm_plan_stats(GemmArgs& a, const GemmKnobs& k, GemmPlan& p) {
  const bool big = p.kernel == GK_BIG, wide1 = p.kernel == GK_WIDE && p.wide == 1, halo = p.kernel == GK_HALO;
  const bool tile = p.kernel == GK_TILE || p.kernel == GK_PERSIST;     // the persistent probe kernel is the eight-wave tile's twin
  const bool staged = p.split == 1 && a.out_mode == OUT_BF16 && (a.N & 7) == 0 && (a.ld_out & 7) == 0;
  const int gbn = big ? 320 : 160;
  const bool gst256 = (halo || big || wide1) && a.M % 256 == 0 && gstat_chunks_fit(a.gstat_hw, 256);
  const bool gst128 = !k.gstat128_off && tile && p.tile == kEightWave && staged && a.M % 128 == 0 && gstat_chunks_fit(a.gstat_hw, 128) &&
                      a.nbatch <= 1 && !a.phase2x && a.out2 == nullptr;      // the transposed / out2 column tiles return before the statistics block
  const bool gst_ok = a.gstat && (gst256 || gst128) && a.gstat_cpg > 0 && gbn % a.gstat_cpg == 0 && a.N % gbn == 0 &&
                      a.N % a.gstat_cpg == 0 && a.act != ACT_GEGLU;
  p.gstat_rows = !gst_ok ? 0 : gst256 ? 256 : 128;
  if (!gst_ok) a.gstat = nullptr;
  const int bn = big ? 320 : wide1 ? 160 : (p.kernel == GK_WIDE && (p.wide == 4 || p.wide == 5)) ? 128 : (tile || p.kernel == GK_BIG_GEGLU) ? kGemmTiles[p.tile].bn : 0;
  const bool rs_ok = a.rowstat && bn > 0 && staged && a.act != ACT_GEGLU && a.N % bn == 0;
  p.rowstat_bn = rs_ok ? bn : 0;
  if (!rs_ok) a.rowstat = nullptr;
}

#define PLAN_REQUIRE(cond, msg) \
  do { if (!(cond)) { set_error(std::string("gemm_launch: ") + (msg)); return -1; } } while (0)

int gemm_plan(GemmArgs& a, const GemmForce& f, const GemmKnobs& k, GemmPlan& p) {
  p = GemmPlan{};
  PLAN_REQUIRE(a.M > 0 && a.N > 0, "empty GEMM");
  PLAN_REQUIRE(a.N % 4 == 0, "N must be a multiple of 4");
  PLAN_REQUIRE(a.ntaps == 0 || a.ntaps == 9 || (a.ntaps == 4 && a.phase2x), "ntaps must be 0 or 9 (4 for the phase planes of an upsample conv)");
  PLAN_REQUIRE(a.ntaps + a.nplain >= 1, "no K segment");
  PLAN_REQUIRE(a.ntaps == 0 || a.conv_c % 8 == 0, "conv channels must be a multiple of 8");
  for (int i = 0; i < a.nplain; ++i) PLAN_REQUIRE(a.p_c[i] % 8 == 0, "segment length must be a multiple of 8");
  PLAN_REQUIRE(a.zero != nullptr, "zero page missing");
  if (a.rows_per_b <= 0) a.rows_per_b = a.M;
  a.ksteps = gemm_count_ksteps(a);

  // ---- tile and K split: the shape's heuristic, then the force ids
  int tile;
  int split = gemm_pick_split(a, &tile);
  if (f.deep) tile = kEightWave;
  if (f.tile > 0) tile = f.tile - 1;
  if (f.split > 0) split = f.split;
  if (a.act == ACT_GEGLU) {
    PLAN_REQUIRE(a.N % 32 == 0 && kGemmTiles[tile].bn != 160 && split == 1, "GEGLU needs N % 32 == 0, a 64/128-wide tile and no split-K");
    PLAN_REQUIRE(a.out_mode == OUT_BF16 && !a.resid && !a.rowvec, "GEGLU epilogue is bias-only, bf16 out");
  }
  const bool xact = gemm_act_is_xact(a.act);
  if (xact) {
    PLAN_REQUIRE(a.out_mode == OUT_BF16 && a.ntaps == 0 && a.nbatch <= 1 && !a.out2 && !a.pre_out && !a.ln_stat && !a.w_img_bs && !a.w_blocked &&
                 !a.phase2x && (a.N & 7) == 0 && (a.ld_out & 7) == 0 && (!a.resid || (a.ld_res & 7) == 0),
                 "GELU / quick-GELU epilogue: plain linears with a row-major 16-bit output and 16-byte aligned rows only");
    tile = kEightWave; split = 1;      // whatever the force ids say: no other instantiation carries these activations
  }
  split = std::min(split, a.ksteps);
  {
    double kk = (double)a.ntaps * a.conv_c;
    for (int i = 0; i < a.nplain; ++i) kk += a.p_c[i];
    const double w_bytes = (double)a.N * kk, a_bytes = (double)a.M * (a.ntaps ? (double)a.conv_c : kk);
    // measured (scripts/gemm_nmajor_probe.py): +12 % / +6 % on the 16x16-level 3x3 convs, -4 % on the linear shapes -> convs only
    // batched planes (Winograd): each plane is its own weight-heavy GEMM -- same rule (DFH_BATCH_NMAJOR=0: m-major, A/B)
    const bool conv_like = a.ntaps || (a.nbatch > 1 && !k.batch_nmajor_off);
    a.n_major = (f.order == 2 || (f.order < 0 && conv_like && w_bytes > a_bytes && a.N > 160)) ? 1 : 0;   // force_order 2 / 3 pin it (probe)
  }
  if (a.nbatch > 1) {
    // the split heuristic sees one plane's tiles: a batched launch has nbatch times as many, and its planes are independent problems
    split = 1;
    PLAN_REQUIRE(((a.ntaps == 0 && a.nplain == 1) || (a.phase2x && a.nplain == 0)) && a.out_mode == OUT_BF16 && a.act != ACT_GEGLU &&
                 !a.resid && !a.rowvec && !a.out2 && !a.rowstat && !a.ln_stat && (a.N & 7) == 0 && (a.ld_out & 7) == 0 && f.split <= 1,
                 "batched launch: one plain segment (or the four phase planes of an upsample conv), plain bf16 row-major output, no split-K");
    a.gstat = nullptr;
    // one plane alone would pick the 256-row tile at the 8x8 level (M <= 1024): the planes together fill the chip with the 128-row tiles
    if (f.tile == 0 && !f.deep) tile = (a.N % 160 == 0) ? kEightWave : 4;
  }
  PLAN_REQUIRE(!a.phase2x || (a.nbatch == 4 && a.ntaps == 4 && a.stride == 1 && a.ups == 0 && !a.pad0 && a.Hin == a.Hout && a.Win == a.Wout &&
                              a.M % (a.Hout * a.Wout) == 0), "phase planes of an upsample conv: four planes over the source image");
  if (split > 1) PLAN_REQUIRE(a.partial != nullptr, "split-K needs a partial buffer");
  if (a.ln_stat) {
    PLAN_REQUIRE(ln_single_pass(a, split) && a.ln_parts > 0 && a.ln_cnt > 0 && a.ln_s != nullptr,
                 "folded LayerNorm: single-pass launches without rowvec / residual only (gemm_ln_consumer_ok)");
    PLAN_REQUIRE(ln_geglu_staged(a), "folded LayerNorm + GEGLU needs 16-byte aligned output rows");
  }
  if (a.w_img_bs) {
    split = 1;
    PLAN_REQUIRE(a.ntaps == 0 && a.nbatch <= 1 && !a.w_blocked && a.rows_per_b % kGemmTiles[tile].bm == 0 && a.M % a.rows_per_b == 0,
                 "per-image weights: plain segments, images of whole row tiles");
  }
  if (a.w_blocked) PLAN_REQUIRE(gemm_lean_plain(a) && a.N % 16 == 0 && a.ldw % 64 == 0 && a.N % 160 == 0 && f.tile == 0 && split == 1,
                                "blocked W: LEAN launches (plain 64-multiple segments) on the 128 x 160 / 256 x 320 tiles only");
  if (a.out2) PLAN_REQUIRE(out2_fits(a, tile, split) && f.tile == 0, "second destination: single pass, n_split a multiple of the column tile (gemm_out2_ok)");
  if (a.resid) PLAN_REQUIRE((double)a.M * a.ld_res * 2.0 < 4.0e9, "residual tensor must be smaller than 4 GB (32-bit lane offsets)");
  a.ksplit = p.split = split;
  p.tile = tile;

  // ---- kernel: 256 x 256 GEGLU tile, 256 x 320 tile, a wide variant, else `tile`.  A forced kernel the launch cannot take (fp32 / transposed
  //      outputs, GEGLU, N % 8) falls back to the heuristic tile; without force ids the *_pick rules decide.
  const bool wide_ok0 = !xact && split == 1 && a.out2 == nullptr && a.out_mode == OUT_BF16 && (a.act != ACT_GEGLU || a.N % 160 == 0 || a.N % 128 == 0) && (a.N & 7) == 0 &&
                        (a.ld_out & 7) == 0 && (!a.resid || (a.ld_res & 7) == 0);
  const bool wide_ok = wide_ok0 && a.nbatch <= 1 && !a.w_img_bs;       // batched launches / per-image weights: gemm_bf16_kernel tiles only (the 256 x 320 one when pinned)
  const bool heur = f.none() && f.split == 0;
  const bool force_big = f.big || (a.nbatch > 1 && f.none() && !f.bigg && !f.persist && !f.deep && batched_big_pick(a, k));
  const bool pre = a.pre_out != nullptr;      // training GEGLU with its pre-activations as a second output: the 256 x 128 wide tile only
  if (pre) PLAN_REQUIRE(wide_ok && a.act == ACT_GEGLU && a.N % 128 == 0 && !a.ln_stat && !a.resid && !a.rowvec && (a.ld_pre & 7) == 0 && a.ld_pre >= a.N,
                        "pre_out: GEGLU launches with N % 128 == 0, no split-K, no folded LayerNorm");
  const bool bigg = !pre && wide_ok && !f.deep && !f.persist && a.act == ACT_GEGLU && a.N % 32 == 0 && !a.resid && !a.rowvec &&
                    (f.bigg || (heur && gemm_big_geglu_pick(a, k)));
  const bool big = wide_ok0 && !f.deep && a.act != ACT_GEGLU && !a.ln_stat && (a.nbatch <= 1 || force_big) && !a.w_img_bs && !f.persist &&
                   (force_big || (heur && gemm_big_pick(a, k)));
  p.wide = pre ? 5 : (!wide_ok || f.deep || big || force_big || bigg || f.bigg || f.persist) ? 0 : f.kernel_pinned() ? f.wide : heur ? gemm_wide_pick(a) : 0;
  p.kernel = bigg ? GK_BIG_GEGLU : big ? GK_BIG : p.wide ? GK_WIDE : GK_TILE;
#ifdef DFH_PROBES
  if (const int r = gemm_plan_probes(a, f, k, p, wide_ok)) return r < 0 ? r : 0;       // 1: the plan is complete (the token linear)
#else
  PLAN_REQUIRE(!f.ws && !f.halo && !(f.wide >= 8 && f.wide <= 14),
               "tile ids 11-20 are probe kernels: build scripts/probes (make -C scripts/probes) and load it with DFH_LIB");
  PLAN_REQUIRE(!f.persist, "tile id 24 is a probe kernel: build scripts/probes (make -C scripts/probes) and load it with DFH_LIB");
#endif

  // ---- the instantiation that runs, its tile order, what its epilogue can write, its census id
  const bool lean = gemm_lean_plain(a);
  switch (p.kernel) {
    case GK_BIG_GEGLU: case GK_GEGLU_ROWS: p.bm = 256; p.bn = 256; p.stages = 2; p.lean = lean; break;
    case GK_BIG: p.bm = 256; p.bn = 320; p.stages = 2; p.lean = lean; break;
    case GK_WIDE: case GK_HALO: p.bm = p.wide == 2 ? 128 : 256; p.bn = p.wide == 3 ? 320 : (p.wide == 4 || p.wide == 5) ? 128 : 160; p.stages = p.wide == 3 ? 4 : 3; break;
    case GK_WS: p.bm = 256; break;      // (the probe hook set bn)
    default: {
      const GemmTile t = kGemmTiles[p.tile];
      p.bm = t.bm; p.bn = t.bn; p.stages = t.stages;
      if (p.tile == kEightWave) {
        // launches of at most ~one workgroup per CU (the 8x8-level Winograd GEMM: 16 planes x 256 rows = 256 workgroups; the 16x16-level token
        // linears), each a chain of k-steps that wait for lines requested one stage ahead: a 4-stage ring keeps three stages in flight.
        const long wgs = (long)((a.M + 127) / 128) * ((a.N + 159) / 160) * (a.nbatch > 1 ? a.nbatch : 1) * a.ksplit;
        if (!xact && !k.deep4_off && (a.nbatch > 1 || k.deep4_all) && wgs <= 320) p.stages = 4;
        p.lean = lean;
      }
    }
  }
  gemm_pick_tile_order(a, k, split, p.bm, p.bn);
  p.n_major = a.n_major; p.tm_xm = a.tm_xm; p.tm_gm = a.tm_gm;
  gemm_plan_stats(a, k, p);
  p.census = (big || bigg) ? CK_GEMM_ROW : (p.kernel == GK_WIDE || p.kernel == GK_HALO) ? CK_GEMM_WIDE :
             (p.kernel != GK_WS && p.tile == kEightWave) ? (lean ? CK_GEMM_LEAN : CK_GEMM_8WAVE) : CK_GEMM_OTHER;
  return 0;
}

GemmWork gemm_work(const GemmArgs& a) {
  // algorithmic work of this launch: 2*M*N*K over the REAL K (padding excluded); bytes = each operand once + output
  double kreal = (double)a.ntaps * a.conv_c;
  double abytes = a.ntaps ? (double)(a.M / (a.Hout * a.Wout)) * a.Hin * a.Win * a.conv_c * 2.0 : 0.0;
  for (int i = 0; i < a.nplain; ++i) { kreal += a.p_c[i]; abytes += (double)a.M * a.p_c[i] * 2.0; }
  const double obytes = (double)a.M * (a.act == ACT_GEGLU ? a.N / 2 : a.N) * ((a.out_mode == OUT_F32 || a.out_mode == OUT_F32_T) ? 4.0 : 2.0) +
                        (a.resid ? (double)a.M * a.N * 2.0 : 0.0) +     // the residual is an operand too: read once
                        (a.pre_out ? (double)a.M * a.N * 2.0 : 0.0);
  const double planes = a.nbatch > 1 ? (double)a.nbatch : 1.0;       // a phase launch reads its source image once for all four planes
  // algorithmic multiply-adds = the reference algorithm's: the four phase planes of an upsample conv stand for the
  // 3x3 conv over the upsampled image (9 taps per output pixel, of which the planes execute 4)
  GemmWork w;
  w.flops = a.prof_flops > 0.0 ? a.prof_flops : (a.phase2x ? 9.0 / 4.0 : 1.0) * planes * 2.0 * a.M * a.N * kreal;
  w.saved = w.flops - planes * 2.0 * a.M * a.N * kreal;
  w.bytes = (a.phase2x == 1 ? abytes : planes * abytes) + planes * ((double)a.N * kreal * 2.0 + obytes);
  w.cls = (a.ntaps || a.prof_flops > 0.0) ? PC_CONV3 : PC_LINEAR;
  return w;
}

const char* gemm_kernel_name(int kernel) {
  static const char* const names[GK_COUNT] = {"tile", "big", "big_geglu", "wide", "ws", "halo", "geglu_rows", "persist", "token_linear"};
  return kernel >= 0 && kernel < GK_COUNT ? names[kernel] : "?";
}

int gemm_plan_format(char* buf, size_t n, const GemmArgs& g, const GemmPlan* p, const char* refusal) {
  int len = snprintf(buf, n, "M=%d N=%d K=%dx%d+%d+%d stride=%d ups=%d nbatch=%d phase=%d act=%d out=%d resid=%d rowvec=%d gstat=%d rowstat=%d ln=%d out2=%d pre=%d wimg=%d |",
                     g.M, g.N, g.ntaps, g.ntaps ? g.conv_c : 0, g.nplain > 0 ? g.p_c[0] : 0, g.nplain > 1 ? g.p_c[1] : 0, g.stride, g.ups, g.nbatch, g.phase2x,
                     g.act, g.out_mode, g.resid != nullptr, g.rowvec != nullptr, g.gstat != nullptr, g.rowstat != nullptr, g.ln_stat != nullptr,
                     g.out2 != nullptr, g.pre_out != nullptr, g.w_img_bs != 0);
  if (len < 0 || (size_t)len >= n) return len;
  if (!p) return len + snprintf(buf + len, n - len, " refused: %s", refusal ? refusal : "");
  return len + snprintf(buf + len, n - len, " kernel=%s tile=%d %dx%d stages=%d lean=%d wide=%d split=%d n_major=%d tm=%d,%d gstat_rows=%d rowstat_bn=%d census=%d",
                        gemm_kernel_name(p->kernel), p->tile, p->bm, p->bn, p->stages, p->lean, p->wide, p->split, p->n_major, p->tm_xm, p->tm_gm,
                        p->gstat_rows, p->rowstat_bn, p->census);
}

}  // namespace dfh

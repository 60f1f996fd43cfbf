// Host-only walk over gemm_plan for a sanitizer build (CPU machine, no GPU, never loaded into python):
//
//   cd difashion_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined gemm_plan.hip ../../scripts/gemm_plan_host_check.hip -o /tmp/gemm_plan_host_check
//   /tmp/gemm_plan_host_check ../../tests/golden/gemm_plan_table.txt
//
// Re-plans every launch of tests/golden/gemm_plan_table.txt (the [default] section: the shape key of a line is enough to rebuild its
// GemmArgs for an unforced launch; lines of forced launches are planned too, under every force id) and compares the unforced ones with
// the recorded text; then plans degenerate inputs that must be refused, not crash.  gemm_plan.hip calls no HIP API, so nothing here can
// reach a device.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "../difashion_amd/csrc/gemm_plan.h"

static std::string g_err;
namespace dfh {   // what gemm_plan.hip needs of api.hip
void set_error(const std::string& msg) { g_err = msg; }
const char* last_error() { return g_err.c_str(); }
}  // namespace dfh

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "line %d: %s  (last error: %s)\n", __LINE__, #cond, g_err.c_str()); return 1; } } while (0)
static float present[4];

static bool parse_key(const char* line, GemmArgs& g) {
  std::memset(&g, 0, sizeof(g));
  int taps, cc, p0, p1, resid, rowvec, gstat, rowstat, ln, out2, pre, wimg;
  if (std::sscanf(line, "M=%d N=%d K=%dx%d+%d+%d stride=%d ups=%d nbatch=%d phase=%d act=%d out=%d resid=%d rowvec=%d gstat=%d rowstat=%d ln=%d out2=%d pre=%d wimg=%d",
                  &g.M, &g.N, &taps, &cc, &p0, &p1, &g.stride, &g.ups, &g.nbatch, &g.phase2x, &g.act, &g.out_mode, &resid, &rowvec, &gstat, &rowstat,
                  &ln, &out2, &pre, &wimg) != 20) return false;
  g.ntaps = taps; g.conv_c = cc; g.conv_src = taps ? (const bf16_t*)present : nullptr;
  g.Hin = g.Win = g.Hout = g.Wout = 1;      // the key does not carry the image size: one-pixel images, M of them
  if (p0) { g.p_src[0] = (const bf16_t*)present; g.p_c[0] = p0; g.nplain = 1; }
  if (p1) { g.p_src[1] = (const bf16_t*)present; g.p_c[1] = p1; g.nplain = 2; }
  g.ldw = taps * cc + p0 + p1; g.W = (const bf16_t*)present; g.zero = (const bf16_t*)present; g.partial = present; g.out = present;
  g.ld_out = g.act == ACT_GEGLU ? g.N / 2 : g.N; g.ld_res = g.N; g.rv_ld = g.N; g.ld_pre = g.N;
  if (resid) g.resid = (const bf16_t*)present;
  if (rowvec) g.rowvec = present;
  if (rowstat) g.rowstat = present;
  if (pre) g.pre_out = present;
  return true;
}

int main(int argc, char** argv) {
  CHECK(argc == 2);
  FILE* f = std::fopen(argv[1], "r");
  CHECK(f != nullptr);
  const dfh::GemmKnobs knobs = dfh::GemmKnobs::defaults();
  static const int ids[] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 18, 19, 20, 21, 22, 23, 24, 30, 31, -1};
  char line[1024], text[512];
  int planned = 0, refused = 0, compared = 0, lines = 0;
  while (std::fgets(line, sizeof(line), f) && std::strncmp(line, "[DFH", 4) != 0) {
    GemmArgs key;
    if (!parse_key(line, key)) continue;
    ++lines;
    for (int id : ids) for (int split : {0, 1, 3, 1000}) for (int order : {-1, 2, 3}) {
      GemmArgs g = key;
      dfh::GemmPlan p;
      const int rc = dfh::gemm_plan(g, dfh::gemm_force_decode(id, split, order), knobs, p);
      rc ? ++refused : ++planned;
      CHECK(dfh::gemm_plan_format(text, sizeof(text), key, rc ? nullptr : &p, rc ? g_err.c_str() : nullptr) < (int)sizeof(text));
      if (rc == 0) {
        CHECK(p.kernel >= 0 && p.kernel <= dfh::GK_WIDE && p.tile >= 0 && p.tile < 6 && p.split >= 1 && p.split <= g.ksteps && g.ksplit == p.split);
        CHECK((p.gstat_rows != 0) == (g.gstat != nullptr) && (p.rowstat_bn != 0) == (g.rowstat != nullptr));
      }
      // a line whose key says everything about its launch (no conv geometry, no statistics, no extras) must come out as recorded
      if (id == 0 && split == 0 && order == -1 && key.ntaps == 0 && !std::strstr(line, "gstat=1") && !std::strstr(line, "ln=1") &&
          !std::strstr(line, "out2=1") && !std::strstr(line, "wimg=1") && key.out_mode == 0 && key.nbatch <= 1 && !std::strstr(line, "refused")) {
        line[std::strcspn(line, "\n")] = 0;
        if (std::strcmp(text, line) == 0) ++compared;      // (forced rows of the table share keys with unforced ones: count, do not require)
      }
    }
  }
  std::fclose(f);
  CHECK(lines > 250 && compared > 40);

  // degenerate inputs: refused, never a crash
  auto refuses = [&](GemmArgs g, int id, int split, const char* with) {
    dfh::GemmPlan p;
    return dfh::gemm_plan(g, dfh::gemm_force_decode(id, split, -1), knobs, p) != 0 && g_err.find(with) != std::string::npos;
  };
  GemmArgs ok;
  CHECK(parse_key("M=4096 N=320 K=0x0+320+0 stride=0 ups=0 nbatch=0 phase=0 act=0 out=0 resid=0 rowvec=0 gstat=0 rowstat=0 ln=0 out2=0 pre=0 wimg=0", ok));
  { dfh::GemmPlan p; GemmArgs g = ok; CHECK(dfh::gemm_plan(g, dfh::gemm_force_decode(0, 0, -1), knobs, p) == 0 && p.tile == dfh::kEightWave); }
  { GemmArgs g = ok; g.M = 0; CHECK(refuses(g, 0, 0, "gemm_launch: empty GEMM")); }
  { GemmArgs g = ok; g.N = 0; CHECK(refuses(g, 0, 0, "empty GEMM")); }
  { GemmArgs g = ok; g.M = -5; CHECK(refuses(g, 0, 0, "empty GEMM")); }
  { GemmArgs g = ok; g.N = 322; CHECK(refuses(g, 0, 0, "N must be a multiple of 4")); }
  { GemmArgs g = ok; g.nplain = 0; CHECK(refuses(g, 0, 0, "no K segment")); }
  { GemmArgs g = ok; g.ntaps = 5; CHECK(refuses(g, 0, 0, "ntaps must be 0 or 9")); }
  { GemmArgs g = ok; g.p_c[0] = 100; CHECK(refuses(g, 0, 0, "segment length must be a multiple of 8")); }
  { GemmArgs g = ok; g.zero = nullptr; CHECK(refuses(g, 0, 0, "zero page missing")); }
  { GemmArgs g = ok; g.partial = nullptr; CHECK(refuses(g, 0, 2, "split-K needs a partial buffer")); }
  { GemmArgs g = ok; g.phase2x = 1; CHECK(refuses(g, 0, 0, "phase planes of an upsample conv")); }
  // ksteps smaller than the forced split: the split is clamped to the k-steps (5 here), the launch is planned
  { dfh::GemmPlan p; GemmArgs g = ok; CHECK(dfh::gemm_plan(g, dfh::gemm_force_decode(0, 100, -1), knobs, p) == 0 && p.split == 5 && g.ksplit == 5); }
  { GemmArgs g = ok; CHECK(refuses(g, 24, 0, "tile id 24 is a probe kernel") && refuses(g, 11, 0, "tile ids 11-20 are probe kernels") && refuses(g, 19, 0, "tile ids 11-20")); }
  std::printf("gemm_plan_host_check: %d table lines, %d plans and %d refusals over every force id / split / order, %d lines equal to the recorded text; "
              "degenerate inputs refused; no sanitizer report\n", lines, planned, refused, compared);
  return 0;
}

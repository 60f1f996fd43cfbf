// Stand-alone host check of the FID / Inception Score row: built by tests/test_inception_cpu.py together with
// csrc/inception.hip under -fsanitize=address,undefined on the host side, and run as a program of its own.  For both variants it walks
// the parameter table, prints the packed and workspace sizes and the launch plan of the shapes given on the command line ("n H W" each),
// and drives every host guard of dfh_incep_create / _forward / _pack and the op-level entries with made-up addresses: each must refuse
// before any HIP call.  No GPU call is made; the few dfh:: services the product file takes from api.hip are stubbed here, and a launch
// that a guard lets through is counted by the stub and fails the program.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/difashion_hip.h"
#include "../../difashion_amd/csrc/dfh_common.h"

namespace dfh {
static std::string g_err;
static int g_launches = 0;
void set_error(const std::string& msg) { g_err = msg; }
const char* last_error() { return g_err.c_str(); }
int check_launch(const char*) { ++g_launches; return 0; }
void census(int) {}
bool prof_enabled() { return false; }
void prof_open(int, double, double, hipStream_t) {}
void prof_close(hipStream_t) {}
}  // namespace dfh

static int failures = 0;

static void expect_refusal(const char* what, int rc, const char* needle) {
  const bool ok = rc != 0 && std::strstr(dfh::last_error(), needle) != nullptr;
  std::printf("guard %s: %s (%s)\n", what, ok ? "refused" : "NOT REFUSED", rc != 0 ? dfh::last_error() : "accepted");
  if (!ok) ++failures;
}

static void walk(const char* tag, const dfh_incep_config& cfg, int argc, char** argv) {
  dfh_incep* c = nullptr;
  if (dfh_incep_create(&cfg, &c) != 0) { std::printf("create failed: %s\n", dfh::last_error()); ++failures; return; }
  const int n = dfh_incep_num_params(c);
  size_t floats = 0;
  for (int i = 0; i < n; ++i) {
    std::printf("param %s %d %s", tag, i, dfh_incep_param_name(c, i));
    size_t count = 1;
    for (int d = 0; d < dfh_incep_param_ndim(c, i); ++d) { std::printf(" %d", dfh_incep_param_dim(c, i, d)); count *= dfh_incep_param_dim(c, i, d); }
    std::printf("\n");
    floats += count;
  }
  if (dfh_incep_param_name(c, -1)[0] || dfh_incep_param_name(c, n)[0] || dfh_incep_param_ndim(c, n) || dfh_incep_param_dim(c, 0, 4)) ++failures;
  std::printf("params %s %d floats %zu packed %zu\n", tag, n, floats, dfh_incep_packed_bytes(c));
  for (int i = 1; i + 2 < argc; i += 3) {
    const int imgs = std::atoi(argv[i]), H = std::atoi(argv[i + 1]), W = std::atoi(argv[i + 2]);
    const size_t ws = dfh_incep_workspace_bytes(c, imgs, H, W);
    const int count = dfh_incep_plan_count(c, imgs, H, W);
    std::printf("workspace %s %d %d %d -> %zu launches %d\n", tag, imgs, H, W, ws, count);
    for (int k = 0; k < count; ++k) {
      dfh_incep_launch L;
      if (dfh_incep_plan_entry(c, imgs, H, W, k, &L) != 0) { ++failures; break; }
      std::printf("launch %s %d kind %d %s %dx%dx%d -> %dx%dx%d ldc %d off %d k %dx%d s %d p %d,%d src %d@%zu+%zu dst %d@%zu+%zu\n", tag, k, L.kind, L.name,
                  L.Hin, L.Win, L.Cin, L.Hout, L.Wout, L.Cout, L.ldc, L.offset, L.KH, L.KW, L.stride, L.padH, L.padW, L.src_region, L.src_off, L.src_floats,
                  L.dst_region, L.dst_off, L.dst_floats);
      // what the plan promises: every workspace access inside the workspace
      if (L.src_region >= 0 && 4 * (L.src_off + L.src_floats) + 256 > ws) ++failures;
      if (L.dst_region >= 0 && 4 * (L.dst_off + L.dst_floats) + 256 > ws) ++failures;
    }
    dfh_incep_launch L;
    expect_refusal("plan index", dfh_incep_plan_entry(c, imgs, H, W, count, &L), "out of range");
  }

  // the guards: every address is made up, nothing may be launched
  std::vector<const float*> good((size_t)n, (const float*)(uintptr_t)4096), with_null = good, misaligned = good;
  with_null[6] = nullptr;
  misaligned[n - 1] = (const float*)(uintptr_t)4100;
  void* buf = (void*)(uintptr_t)8192;
  float* out = (float*)(uintptr_t)8192;
  float* taps[4] = {out, out, out, out};
  float* no_tap[4] = {out, out, out, nullptr};
  const bool tv = cfg.variant == DFH_INCEP_VARIANT_TV;
  const size_t need = dfh_incep_workspace_bytes(c, 2, 80, 80);
  auto fwd = [&](const float* const* P, int count, const void* packed, const float* in, int H, int W, float* const* tp, float* probs, void* ws,
                 size_t ws_bytes) { return dfh_incep_forward(c, P, count, packed, in, 2, H, W, tp, probs, ws, ws_bytes, nullptr); };
  expect_refusal("count", fwd(good.data(), n - 1, buf, out, 80, 80, taps, out, buf, need), "count does not match");
  expect_refusal("null params", fwd(nullptr, n, buf, out, 80, 80, taps, out, buf, need), "null argument: params");
  expect_refusal("null parameter", fwd(with_null.data(), n, buf, out, 80, 80, taps, out, buf, need), "null parameter pointer: Conv2d_2a_3x3.bn.weight");
  expect_refusal("misaligned parameter", fwd(misaligned.data(), n, buf, out, 80, 80, taps, out, buf, need),
                 tv ? "not 16-byte aligned: fc.bias" : "not 16-byte aligned: Mixed_7c.branch_pool.bn.running_var");
  expect_refusal("null packed", fwd(good.data(), n, nullptr, out, 80, 80, taps, out, buf, need), "null argument: packed");
  expect_refusal("null in", fwd(good.data(), n, buf, nullptr, 80, 80, taps, out, buf, need), "null argument: in");
  expect_refusal("null taps", fwd(good.data(), n, buf, out, 80, 80, nullptr, out, buf, need), "null argument: taps");
  expect_refusal("missing tap", fwd(good.data(), n, buf, out, 80, 80, no_tap, out, buf, need), "null argument: taps[3]");
  if (tv) expect_refusal("null probs", fwd(good.data(), n, buf, out, 80, 80, taps, nullptr, buf, need), "null argument: probs");
  expect_refusal("null workspace", fwd(good.data(), n, buf, out, 80, 80, taps, out, nullptr, need), "null argument: workspace");
  expect_refusal("misaligned in", fwd(good.data(), n, buf, (const float*)(uintptr_t)8196, 80, 80, taps, out, buf, need), "in must be 16-byte aligned");
  expect_refusal("misaligned packed", fwd(good.data(), n, (void*)(uintptr_t)8200, out, 80, 80, taps, out, buf, need), "packed must be 16-byte aligned");
  expect_refusal("misaligned workspace", fwd(good.data(), n, buf, out, 80, 80, taps, out, (void*)(uintptr_t)8208, need), "workspace must be 256-byte aligned");
  expect_refusal("H of 0", fwd(good.data(), n, buf, out, 0, 80, taps, out, buf, need), "must be in [1, 8192]");
  expect_refusal("W beyond 8192", fwd(good.data(), n, buf, out, 80, 9000, taps, out, buf, need), "must be in [1, 8192]");
  expect_refusal("small workspace", fwd(good.data(), n, buf, out, 80, 80, taps, out, buf, need - 1), "workspace smaller");
  expect_refusal("pack count", dfh_incep_pack(c, good.data(), n + 1, buf, nullptr), "count does not match");
  expect_refusal("pack null packed", dfh_incep_pack(c, good.data(), n, nullptr, nullptr), "null argument: packed");
  dfh_incep_destroy(c);
}

int main(int argc, char** argv) {
  if ((argc - 1) % 3 != 0) { std::fprintf(stderr, "usage: [n H W] ...\n"); return 2; }
  dfh_incep* c = nullptr;
  dfh_incep_config bad = {2, 50, 1, 1, 8};
  expect_refusal("variant", dfh_incep_create(&bad, &c), "unsupported variant");
  expect_refusal("null config", dfh_incep_create(nullptr, &c), "null argument");
  dfh_incep_config no_block = {DFH_INCEP_VARIANT_FID, 0, 1, 1, 0};
  expect_refusal("empty block mask", dfh_incep_create(&no_block, &c), "block_mask");
  dfh_incep_config tv_mask = {DFH_INCEP_VARIANT_TV, 50, 1, 1, 7};
  expect_refusal("classifier block mask", dfh_incep_create(&tv_mask, &c), "block_mask must include block 3");
  dfh_incep_config tv_classes = {DFH_INCEP_VARIANT_TV, 0, 1, 1, 8};
  expect_refusal("classes", dfh_incep_create(&tv_classes, &c), "num_classes");

  const dfh_incep_config fid = {DFH_INCEP_VARIANT_FID, 0, 1, 1, 15}, tv = {DFH_INCEP_VARIANT_TV, 50, 1, 1, 8};
  walk("fid", fid, argc, argv);
  walk("tv", tv, argc, argv);
  // without the resize the image itself walks the network: below 75 a side Mixed_7a would be empty
  const dfh_incep_config raw = {DFH_INCEP_VARIANT_FID, 0, 0, 1, 8};
  if (dfh_incep_create(&raw, &c) == 0) {
    if (dfh_incep_workspace_bytes(c, 1, 74, 80) != 0 || dfh_incep_workspace_bytes(c, 1, 75, 75) == 0) ++failures;
    expect_refusal("below 75 without resize", dfh_incep_plan_count(c, 1, 74, 80) < 0 ? -1 : 0, "at least 75");
    dfh_incep_destroy(c);
  } else ++failures;

  // the op-level guards
  void* buf = (void*)(uintptr_t)8192;
  float* f = (float*)buf;
  const float* bn[4] = {f, f, f, f};
  const float* bn_null[4] = {f, f, nullptr, f};
  expect_refusal("conv C_in", dfh_incep_conv_bn_relu(f, f, 3, bn, f, f, 1, 8, 8, 3, 32, 3, 3, 1, 0, 0, 32, 0, nullptr), "C_in must be a multiple of 4");
  expect_refusal("conv filter", dfh_incep_conv_bn_relu(f, f, 4, bn, f, f, 1, 8, 8, 4, 32, 2, 3, 1, 0, 0, 32, 0, nullptr), "KH and KW must be 1, 3, 5 or 7");
  expect_refusal("conv stride", dfh_incep_conv_bn_relu(f, f, 4, bn, f, f, 1, 8, 8, 4, 32, 3, 3, 3, 0, 0, 32, 0, nullptr), "stride must be 1 or 2");
  expect_refusal("conv slice", dfh_incep_conv_bn_relu(f, f, 4, bn, f, f, 1, 8, 8, 4, 32, 3, 3, 1, 0, 0, 48, 32, nullptr), "must lie inside ldc");
  expect_refusal("conv small image", dfh_incep_conv_bn_relu(f, f, 4, bn, f, f, 1, 2, 8, 4, 32, 3, 3, 1, 0, 0, 32, 0, nullptr), "smaller than the filter");
  expect_refusal("conv null bn", dfh_incep_conv_bn_relu(f, f, 4, bn_null, f, f, 1, 8, 8, 4, 32, 3, 3, 1, 0, 0, 32, 0, nullptr), "null argument: bn");
  expect_refusal("pool mode", dfh_incep_pool(f, f, 4, 1, 8, 8, 16, 16, 0, nullptr), "mode must be");
  expect_refusal("pool channels", dfh_incep_pool(f, f, 0, 1, 8, 8, 6, 8, 0, nullptr), "multiples of 4");
  expect_refusal("pool slice", dfh_incep_pool(f, f, 0, 1, 8, 8, 16, 16, 4, nullptr), "must lie inside ldc");
  expect_refusal("pool small image", dfh_incep_pool(f, f, 0, 1, 2, 8, 16, 16, 0, nullptr), "at least 3");
  expect_refusal("stats one row", dfh_incep_stats(f, 1, 64, (double*)buf, (double*)buf, nullptr), "at least two rows");
  expect_refusal("stats null", dfh_incep_stats(f, 4, 64, nullptr, (double*)buf, nullptr), "null argument");
  expect_refusal("splits beyond n", dfh_incep_is_splits(f, f, f, 3, 4, f, nullptr), "splits must be in [1, n]");
  expect_refusal("rows null", dfh_incep_is_rows(f, nullptr, 3, 50, 1e-16f, nullptr, f, f, f, nullptr), "null argument");
  expect_refusal("fc K", dfh_incep_fc_softmax(f, f, f, f, f, 2, 2046, 50, nullptr), "K a multiple of 4");
  expect_refusal("gmean null", dfh_incep_global_mean(f, nullptr, 1, 4, 64, nullptr), "null argument");
  expect_refusal("prep null", dfh_incep_prep(nullptr, 1, 8, 8, 1, 1, 0, f, nullptr), "null argument");
  dfh_incep_destroy(nullptr);
  std::printf("launches %d failures %d\n", dfh::g_launches, failures);
  return failures == 0 && dfh::g_launches == 0 ? 0 : 1;
}

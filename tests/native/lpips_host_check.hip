// Stand-alone host check of the LPIPS row: built by tests/test_lpips_cpu.py together with csrc/lpips.hip under
// -fsanitize=address,undefined on the host side, and run as a program of its own.  It walks the parameter table, prints the packed and
// workspace sizes of the shapes given on the command line ("pairs H W" each), and drives every host guard of dfh_lpips_forward /
// dfh_lpips_pack with made-up addresses: each must refuse before any HIP call.  No GPU call is made; the few dfh:: services the product
// file takes from api.hip are stubbed here, and a launch that a guard lets through is counted by the stub and fails the program.
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

int main(int argc, char** argv) {
  if ((argc - 1) % 3 != 0) { std::fprintf(stderr, "usage: [pairs H W] ...\n"); return 2; }
  dfh_lpips* c = nullptr;
  dfh_lpips_config bad = {1};
  expect_refusal("net", dfh_lpips_create(&bad, &c), "only VGG16");
  expect_refusal("null config", dfh_lpips_create(nullptr, &c), "null argument");
  dfh_lpips_config cfg = {DFH_LPIPS_NET_VGG16};
  if (dfh_lpips_create(&cfg, &c) != 0) { std::printf("create failed: %s\n", dfh::last_error()); return 1; }
  const int n = dfh_lpips_num_params(c);
  size_t floats = 0;
  for (int i = 0; i < n; ++i) {
    std::printf("param %d %s", i, dfh_lpips_param_name(c, i));
    size_t count = 1;
    for (int d = 0; d < dfh_lpips_param_ndim(c, i); ++d) { std::printf(" %d", dfh_lpips_param_dim(c, i, d)); count *= dfh_lpips_param_dim(c, i, d); }
    std::printf("\n");
    floats += count;
  }
  if (dfh_lpips_param_name(c, -1)[0] || dfh_lpips_param_name(c, n)[0] || dfh_lpips_param_ndim(c, n) || dfh_lpips_param_dim(c, 0, 4)) ++failures;
  std::printf("params %d floats %zu packed %zu\n", n, floats, dfh_lpips_packed_bytes(c));
  for (int i = 1; i + 2 < argc; i += 3) {
    const int pairs = std::atoi(argv[i]), H = std::atoi(argv[i + 1]), W = std::atoi(argv[i + 2]);
    std::printf("workspace %d %d %d -> %zu\n", pairs, H, W, dfh_lpips_workspace_bytes(c, pairs, H, W));
  }

  // the guards: every address is made up, nothing may be launched
  std::vector<const float*> good((size_t)n, (const float*)(uintptr_t)4096), with_null = good, misaligned = good;
  with_null[5] = nullptr;
  misaligned[n - 1] = (const float*)(uintptr_t)4100;
  void* buf = (void*)(uintptr_t)8192;
  float* out = (float*)(uintptr_t)8192;
  const size_t need = dfh_lpips_workspace_bytes(c, 2, 16, 16);
  auto fwd = [&](const float* const* P, int count, const void* packed, const void* in0, const void* in1, int kind, const float* lut, int norm,
                 int H, int W, float* dist, void* ws, size_t ws_bytes) {
    return dfh_lpips_forward(c, P, count, packed, in0, in1, kind, lut, norm, 2, H, W, dist, nullptr, ws, ws_bytes, nullptr);
  };
  expect_refusal("count", fwd(good.data(), n - 1, buf, buf, buf, 1, nullptr, 0, 16, 16, out, buf, need), "count does not match");
  expect_refusal("null params", fwd(nullptr, n, buf, buf, buf, 1, nullptr, 0, 16, 16, out, buf, need), "null argument: params");
  expect_refusal("null parameter", fwd(with_null.data(), n, buf, buf, buf, 1, nullptr, 0, 16, 16, out, buf, need),
                 "null parameter pointer: net.slice1.2.bias");
  expect_refusal("misaligned parameter", fwd(misaligned.data(), n, buf, buf, buf, 1, nullptr, 0, 16, 16, out, buf, need),
                 "not 16-byte aligned: lin4.model.1.weight");
  expect_refusal("null packed", fwd(good.data(), n, nullptr, buf, buf, 1, nullptr, 0, 16, 16, out, buf, need), "null argument: packed");
  expect_refusal("null in0", fwd(good.data(), n, buf, nullptr, buf, 1, nullptr, 0, 16, 16, out, buf, need), "null argument: in0");
  expect_refusal("null in1", fwd(good.data(), n, buf, buf, nullptr, 1, nullptr, 0, 16, 16, out, buf, need), "null argument: in1");
  expect_refusal("null distance", fwd(good.data(), n, buf, buf, buf, 1, nullptr, 0, 16, 16, nullptr, buf, need), "null argument: distance");
  expect_refusal("null workspace", fwd(good.data(), n, buf, buf, buf, 1, nullptr, 0, 16, 16, out, nullptr, need), "null argument: workspace");
  expect_refusal("null lut", fwd(good.data(), n, buf, buf, buf, 0, nullptr, 0, 16, 16, out, buf, need), "null argument: lut");
  expect_refusal("uint8 normalize", fwd(good.data(), n, buf, buf, buf, 0, out, 1, 16, 16, out, buf, need), "normalize applies");
  expect_refusal("src_kind", fwd(good.data(), n, buf, buf, buf, 2, nullptr, 0, 16, 16, out, buf, need), "src_kind");
  expect_refusal("misaligned in1", fwd(good.data(), n, buf, buf, (void*)(uintptr_t)8196, 1, nullptr, 0, 16, 16, out, buf, need),
                 "in1 must be 16-byte aligned");
  expect_refusal("misaligned packed", fwd(good.data(), n, (void*)(uintptr_t)8200, buf, buf, 1, nullptr, 0, 16, 16, out, buf, need),
                 "packed must be 16-byte aligned");
  expect_refusal("H below 16", fwd(good.data(), n, buf, buf, buf, 1, nullptr, 0, 15, 16, out, buf, need), "at least 16");
  expect_refusal("W below 16", fwd(good.data(), n, buf, buf, buf, 1, nullptr, 0, 16, 8, out, buf, need), "at least 16");
  expect_refusal("small workspace", fwd(good.data(), n, buf, buf, buf, 1, nullptr, 0, 16, 16, out, buf, need - 1), "workspace smaller");
  expect_refusal("pack count", dfh_lpips_pack(c, good.data(), n + 1, buf, nullptr), "count does not match");
  expect_refusal("pack null packed", dfh_lpips_pack(c, good.data(), n, nullptr, nullptr), "null argument: packed");
  dfh_lpips_destroy(c);
  dfh_lpips_destroy(nullptr);
  std::printf("launches %d failures %d\n", dfh::g_launches, failures);
  return failures == 0 && dfh::g_launches == 0 ? 0 : 1;
}

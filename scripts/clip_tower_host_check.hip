// Host-only walk over the C ABI of the two CLIP towers for a sanitizer build (CPU machine, no GPU, never loaded into python):
//
//   cd difashion_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined clip.hip clip_vision.hip ../../scripts/clip_tower_host_check.hip -o /tmp/clip_tower_host_check
//   /tmp/clip_tower_host_check
//
// Creates and destroys both towers for a tiny config, walks every table accessor (out-of-range indices and dimensions included),
// calls both *_workspace_bytes, and calls both encodes with arguments they must refuse.  No kernel is launched: every encode below
// has to return before its first launch, and the stand-ins for api.hip's helpers abort the program if a launch is reached.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/difashion_hip.h"
#include "../difashion_amd/csrc/dfh_common.h"

static std::string g_err;
namespace dfh {   // what clip.hip / clip_vision.hip need of api.hip
void set_error(const std::string& msg) { g_err = msg; }
int check_launch(const char* what) { std::fprintf(stderr, "a kernel was launched: %s\n", what); std::abort(); }
void census(int) {}
bool prof_enabled() { return false; }
void prof_open(int, double, double, hipStream_t) {}
void prof_close(hipStream_t) {}
}  // namespace dfh

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "line %d: %s  (last error: %s)\n", __LINE__, #cond, g_err.c_str()); return 1; } } while (0)
static bool refused(int rc, const char* with) { return rc != 0 && g_err.find(with) != std::string::npos; }

template <class H, class Num, class Name, class Ndim, class Dim>
static int walk_table(const H* h, Num num, Name name, Ndim ndim, Dim dim, const char* first, size_t* values) {
  const int n = num(h);
  CHECK(n > 0 && std::strcmp(name(h, 0), first) == 0);
  *values = 0;
  for (int i = 0; i < n; ++i) {
    size_t v = 1;
    CHECK(std::strlen(name(h, i)) > 0 && ndim(h, i) >= 1);
    for (int d = 0; d < ndim(h, i); ++d) { CHECK(dim(h, i, d) > 0); v *= dim(h, i, d); }
    CHECK(dim(h, i, -1) == 0 && dim(h, i, ndim(h, i)) == 0);
    *values += v;
  }
  for (int i : {-1, n, n + 1, 1 << 30, -(1 << 30)}) CHECK(name(h, i)[0] == 0 && ndim(h, i) == 0 && dim(h, i, 0) == 0);
  return 0;
}

int main() {
  float* const fake = (float*)4096;          // made-up, aligned addresses: never dereferenced
  void* const ws = (void*)8192;
  size_t values = 0;

  dfh_clip_config tc = {100, 64, 128, 2, 4, 77, 1, 1e-5f};
  dfh_clip* t = nullptr;
  CHECK(dfh_clip_create(nullptr, &t) != 0);
  tc.hidden_size = 30; CHECK(refused(dfh_clip_create(&tc, &t), "multiples of 4")); tc.hidden_size = 64;
  CHECK(dfh_clip_create(&tc, &t) == 0 && t);
  CHECK(walk_table(t, dfh_clip_num_params, dfh_clip_param_name, dfh_clip_param_ndim, dfh_clip_param_dim,
                   "text_model.embeddings.token_embedding.weight", &values) == 0);
  CHECK(dfh_clip_num_params(t) == 2 + 16 * 2 + 2 && values == 100 * 64 + 77 * 64 + 2 * (4 * (64 * 64 + 64) + 2 * 64 * 128 + 128 + 64 + 4 * 64) + 2 * 64);
  const size_t tneed = dfh_clip_workspace_bytes(t, 2, 16);
  CHECK(tneed == (2 * 16 * (6 * 64 + 128) + 64) * 4 + 256);
  {
    const int n = dfh_clip_num_params(t);
    std::vector<const float*> p(n, fake);
    const int64_t* ids = (const int64_t*)fake;
    auto enc = [&](const float* const* arr, int cnt, void* w, size_t wb, int T) {
      return dfh_clip_encode(t, arr, cnt, ids, fake, nullptr, 2, nullptr, w, wb, 2, T, nullptr);
    };
    CHECK(refused(enc(nullptr, n, ws, tneed, 16), "null argument"));
    CHECK(refused(enc(p.data(), n - 1, ws, tneed, 16), "count does not match dfh_clip_num_params"));
    p[1] = nullptr; CHECK(refused(enc(p.data(), n, ws, tneed, 16), "null parameter pointer: text_model.embeddings.position_embedding.weight")); p[1] = fake;
    p[n - 1] = fake + 1; CHECK(refused(enc(p.data(), n, ws, tneed, 16), "not 16-byte aligned: text_model.final_layer_norm.bias")); p[n - 1] = fake;
    CHECK(refused(enc(p.data(), n, ws, tneed, 78), "sequence length"));
    CHECK(refused(enc(p.data(), n, ws, tneed - 1, 16), "workspace smaller"));
    CHECK(refused(enc(p.data(), n, (char*)ws + 16, tneed, 16), "256-byte aligned"));
  }
  dfh_clip_destroy(t);

  dfh_clipv_config vc = {64, 128, 2, 4, 56, 14, 3, 32, 2, 1e-5f};          // C p^2 = 588 > 3 D: the q k v region is im2col-wide
  dfh_clipv* v = nullptr;
  vc.image_size = 60; CHECK(refused(dfh_clipv_create(&vc, &v), "multiple of patch_size")); vc.image_size = 56;
  CHECK(dfh_clipv_create(&vc, &v) == 0 && v);
  CHECK(walk_table(v, dfh_clipv_num_params, dfh_clipv_param_name, dfh_clipv_param_ndim, dfh_clipv_param_dim,
                   "vision_model.embeddings.class_embedding", &values) == 0);
  CHECK(dfh_clipv_num_params(v) == 5 + 16 * 2 + 3);
  const size_t vneed = dfh_clipv_workspace_bytes(v, 2);
  CHECK(vneed == (2 * 17 * (3 * 64 + 588 + 128) + 2 * 64 + 64) * 4 + 256 && dfh_clipv_workspace_bytes(v, 0) == 0 && dfh_clipv_workspace_bytes(nullptr, 2) == 0);
  {
    const int n = dfh_clipv_num_params(v);
    std::vector<const float*> p(n, fake);
    auto enc = [&](const float* const* arr, int cnt, const float* px, void* w, size_t wb, int B) {
      return dfh_clipv_encode(v, arr, cnt, px, B, fake, nullptr, nullptr, nullptr, w, wb, nullptr);
    };
    CHECK(refused(enc(p.data(), n, nullptr, ws, vneed, 2), "null argument"));
    CHECK(refused(enc(p.data(), n + 1, fake, ws, vneed, 2), "count does not match dfh_clipv_num_params"));
    p[3] = nullptr; CHECK(refused(enc(p.data(), n, fake, ws, vneed, 2), "null parameter pointer: vision_model.pre_layrnorm.weight")); p[3] = fake;
    p[5] = fake + 1; CHECK(refused(enc(p.data(), n, fake, ws, vneed, 2), "not 16-byte aligned: vision_model.encoder.layers.0.self_attn.k_proj.weight")); p[5] = fake;
    CHECK(refused(enc(p.data(), n, fake, ws, vneed, 0), "batch must be"));
    CHECK(refused(enc(p.data(), n, fake, ws, vneed - 1, 2), "workspace smaller"));
    CHECK(refused(enc(p.data(), n, fake, (char*)ws + 16, vneed, 2), "256-byte aligned"));
    CHECK(refused(enc(p.data(), n, fake + 1, ws, vneed, 2), "outputs must be 16-byte aligned"));
    CHECK(refused(dfh_clipv_attention(nullptr, fake, 1, 8, 2, 64, 1.0f, nullptr), "null argument"));
    CHECK(refused(dfh_clipv_attention(fake, fake, 1, 8, 2, 130, 1.0f, nullptr), "head dim"));
  }
  dfh_clipv_destroy(v);
  std::puts("clip_tower_host_check: both towers created, walked, refused and destroyed; no kernel launched");
  return 0;
}

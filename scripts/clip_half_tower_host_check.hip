// Host-only walk over the C ABI of the two 16-bit CLIP towers (dfh_cliph_*, dfh_clipvh_*: csrc/clip_tower_half.h and the host side of
// clip_text_half.hip / clip_vision_half.hip) for a sanitizer build (CPU machine, no GPU, never loaded into python):
//
//   cd difashion_amd/csrc && hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined clip.hip clip_vision.hip clip_text_half.hip clip_vision_half.hip gemm_plan.hip walk_knobs.hip \
//       ../../scripts/clip_half_tower_host_check.hip -o /tmp/clip_half_tower_host_check
//   /tmp/clip_half_tower_host_check
//
// Creates both contexts for a tiny config, plans both walks at several (batch, T) and checks what the plans promise each other (the
// size queries, the launches' regions, the packed copy as the per-layer layout gives it), then calls _pack / _encode / _text_embeds /
// dfh_causal_attention with arguments they must refuse.  No kernel is launched: every call below has to return before its first launch,
// and the stand-ins for the launchers and for api.hip's helpers abort the program if one is reached.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../include/difashion_hip.h"
#include "../difashion_amd/csrc/attention.h"
#include "../difashion_amd/csrc/clip_tower_half.h"

static std::string g_err;
[[noreturn]] static void launched(const char* what) { std::fprintf(stderr, "a launch was reached: %s\n", what); std::abort(); }
namespace dfh {   // what the four CLIP files need of api.hip and of the kernel files
void set_error(const std::string& msg) { g_err = msg; }
const char* last_error() { return g_err.c_str(); }
int check_launch(const char* what) { launched(what); }
void census(int) {}
bool prof_enabled() { return false; }
void prof_open(int, double, double, hipStream_t) {}
void prof_close(hipStream_t) {}
int gemm_launch(GemmArgs, hipStream_t, int, int, int, int*, int*) { launched("gemm_launch"); }
int layernorm_launch(const bf16_t*, const float*, const float*, bf16_t*, int, int, float, hipStream_t) { launched("layernorm_launch"); }
int attention_launch(const AttnArgs&, hipStream_t) { launched("attention_launch"); }
int pack_matrix_launch(const float*, bf16_t*, int, int, int, int, int, int, hipStream_t) { launched("pack_matrix_launch"); }
int pack_vector_launch(const float*, float*, int, int, int, int, hipStream_t) { launched("pack_vector_launch"); }
bool attention_x32_eligible(const AttnArgs&) { return false; }   // stand-in for attention_x32.hip: the flag is not what is checked here
}  // namespace dfh

#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "line %d: %s  (last error: %s)\n", __LINE__, #cond, g_err.c_str()); return 1; } } while (0)
static bool refused(int rc, const char* with) { return rc != 0 && g_err.find(with) != std::string::npos; }
static size_t up(size_t n) { return (n + 255) / 256 * 256; }

// what either plan promises: regions in order, aligned and inside the workspace; every launch's buffers inside its regions
template <class Plan>
static int check_plan(const Plan& p, size_t workspace_query) {
  CHECK(p.num_launches > 0 && p.num_launches <= DFH_CLIPVH_MAX_LAUNCHES && p.num_regions > 0 && p.num_regions <= DFH_CLIPVH_MAX_REGIONS);
  size_t end = 0;
  for (int i = 0; i < p.num_regions; ++i) {
    CHECK(p.regions[i].offset % 256 == 0 && p.regions[i].offset >= end && std::strlen(p.regions[i].name) > 0);
    end = p.regions[i].offset + p.regions[i].bytes;
  }
  CHECK(end <= p.workspace_bytes && p.workspace_bytes == workspace_query && p.workspace_bytes < end + 256);
  for (int i = 0; i < p.num_launches; ++i) {
    const dfh_clipvh_launch& l = p.launches[i];
    CHECK(l.a_region >= 0 && l.a_region < p.num_regions && l.out_region >= 0 && l.out_region < p.num_regions && l.out2_region < p.num_regions);
    CHECK(p.regions[l.a_region].bytes >= (size_t)l.M * l.lda * 2 && p.regions[l.out_region].bytes >= (size_t)l.M * l.ld_out * 2);
  }
  return 0;
}

int main() {
  float* const fake = (float*)4096;          // made-up, aligned addresses: never dereferenced
  void* const ws = (void*)8192;
  void* const packed = (void*)16384;
  const int D = 128, I = 256, L = 2;
  const size_t per_layer = up(3 * D * D * 2) + up(D * D * 2) + 2 * up(D * I * 2) + up(3 * D * 4);
  CHECK(dfh::HalfLayerPack(D, I).per_layer == per_layer && dfh::HalfLayerPack(D, I).bqkv + up(3 * D * 4) == per_layer);

  // ---- text: hidden 128, 2 heads of 64, 77 positions
  dfh_clip_config tc = {1000, D, I, L, 2, 77, 1, 1e-5f};
  dfh_clip* t = nullptr;
  CHECK(dfh_clip_create(&tc, &t) == 0 && t);
  CHECK(dfh_cliph_packed_bytes(t) == L * per_layer && dfh_cliph_packed_bytes(nullptr) == 0);
  dfh_cliph_plan_info tp;
  for (int B : {1, 3, 64}) for (int T : {1, 16, 20, 77}) {
    CHECK(dfh_cliph_plan(t, B, T, &tp) == 0 && tp.rows == B * T && tp.head_dim == 64 && tp.num_launches == 4 && tp.packed_bytes == L * per_layer);
    CHECK(check_plan(tp, dfh_cliph_workspace_bytes(t, B, T)) == 0);
  }
  CHECK(refused(dfh_cliph_plan(t, 0, 20, &tp), "cliph_plan: batch must be in") && refused(dfh_cliph_plan(t, 2, 78, &tp), "sequence length must be in [1, 77], got 78"));
  CHECK(refused(dfh_cliph_plan(nullptr, 2, 20, &tp), "cliph_plan: null argument") && refused(dfh_cliph_plan(t, 2, 20, nullptr), "null argument"));
  CHECK(dfh_cliph_workspace_bytes(t, 2, 0) == 0 && dfh_cliph_workspace_bytes(t, 65536, 20) == 0);
  const size_t tneed = dfh_cliph_workspace_bytes(t, 2, 16);
  {
    const int n = dfh_clip_num_params(t);
    std::vector<const float*> p(n, fake);
    const int64_t* ids = (const int64_t*)fake;
    CHECK(refused(dfh_cliph_pack(t, nullptr, n, packed, nullptr), "dfh_cliph_pack: null argument"));
    CHECK(refused(dfh_cliph_pack(t, p.data(), n - 1, packed, nullptr), "count does not match dfh_clip_num_params"));
    CHECK(refused(dfh_cliph_pack(t, p.data(), n, (char*)packed + 16, nullptr), "dfh_cliph_pack: the packed copy must be 256-byte aligned"));
    auto enc = [&](const float* const* arr, int cnt, const int64_t* id, float* last, float* hs, void* w, size_t wb, const void* pk, int B, int T) {
      return dfh_cliph_encode(t, arr, cnt, pk, id, last, nullptr, 2, hs, w, wb, B, T, nullptr);
    };
    CHECK(refused(enc(nullptr, n, ids, fake, nullptr, ws, tneed, packed, 2, 16), "dfh_cliph_encode: null argument"));
    CHECK(refused(enc(p.data(), n, ids, fake + 1, nullptr, ws, tneed, packed, 2, 16), "dfh_cliph_encode: outputs must be 16-byte aligned"));
    CHECK(refused(enc(p.data(), n + 1, ids, fake, nullptr, ws, tneed, packed, 2, 16), "count does not match dfh_clip_num_params"));
    p[1] = nullptr; CHECK(refused(enc(p.data(), n, ids, fake, nullptr, ws, tneed, packed, 2, 16), "null parameter pointer")); p[1] = fake;
    p[n - 1] = fake + 1; CHECK(refused(enc(p.data(), n, ids, fake, nullptr, ws, tneed, packed, 0, 16), "not 16-byte aligned")); p[n - 1] = fake;   // before the plan
    CHECK(refused(enc(p.data(), n, ids, fake, nullptr, ws, tneed, packed, 0, 16), "cliph_plan: batch must be in"));
    CHECK(refused(enc(p.data(), n, ids, fake, nullptr, ws, tneed, packed, 2, 78), "cliph_plan: the 16-bit tower's causal attention kernel holds"));
    CHECK(refused(enc(p.data(), n, ids, fake, nullptr, ws, tneed - 1, packed, 2, 16), "cliph_walk: workspace smaller than dfh_cliph_workspace_bytes"));
    CHECK(refused(enc(p.data(), n, ids, fake, nullptr, (char*)ws + 16, tneed, packed, 2, 16), "cliph_walk: workspace / packed copy must be 256-byte aligned"));
    CHECK(refused(enc(p.data(), n, ids, fake, nullptr, ws, tneed, (char*)packed + 128, 2, 16), "workspace / packed copy must be 256-byte aligned"));
    CHECK(refused(enc(p.data(), n, (const int64_t*)((char*)fake + 4), fake, nullptr, ws, tneed, packed, 2, 16), "input_ids must be 8-byte aligned"));
    CHECK(refused(enc(p.data(), n, ids, fake, fake + 1, ws, tneed, packed, 2, 16), "hidden_states must be 16-byte aligned"));
    auto emb = [&](const float* proj, int pdim, float* out, void* w, size_t wb) {
      return dfh_cliph_text_embeds(t, p.data(), n, packed, proj, pdim, ids, out, nullptr, nullptr, 2, nullptr, w, wb, 2, 16, nullptr);
    };
    CHECK(refused(emb(nullptr, 64, fake, ws, tneed), "dfh_cliph_text_embeds: null argument") && refused(emb(fake, 0, fake, ws, tneed), "projection_dim must be positive"));
    CHECK(refused(emb(fake + 1, 64, fake, ws, tneed), "text_projection must be 16-byte aligned") && refused(emb(fake, 64, fake + 2, ws, tneed), "outputs must be 16-byte aligned"));
    CHECK(refused(emb(fake, 64, fake, ws, tneed - 256), "workspace smaller") && refused(emb(fake, 64, fake, (char*)ws + 64, tneed), "256-byte aligned"));
    CHECK(refused(dfh_causal_attention(nullptr, ws, 1, 8, 1, 64, 0.125f, nullptr), "null argument"));
    CHECK(refused(dfh_causal_attention(ws, ws, 1, 8, 1, 32, 0.125f, nullptr), "built for head dim 64"));
    CHECK(refused(dfh_causal_attention(ws, ws, 1, 129, 1, 64, 0.125f, nullptr), "sequence length must be in [1, 128]"));
    CHECK(refused(dfh_causal_attention(ws, ws, 0, 8, 1, 64, 0.125f, nullptr), "batch must be in"));
    CHECK(refused(dfh_causal_attention((char*)ws + 2, ws, 1, 8, 1, 64, 0.125f, nullptr), "16-byte aligned"));
  }
  dfh_clip_destroy(t);

  // ---- image: hidden 128, 2 heads of 64, 56 pixels in patches of 8 (T = 50, patch K = 192); then patches of 14 (K = 588 -> 592)
  dfh_clipv_config vc = {D, I, L, 2, 56, 8, 3, 32, 2, 1e-5f};
  dfh_clipv* v = nullptr;
  CHECK(dfh_clipv_create(&vc, &v) == 0 && v);
  CHECK(dfh_clipvh_packed_bytes(v) == up(D * 192 * 2) + L * per_layer && dfh_clipvh_packed_bytes(nullptr) == 0);
  dfh_clipvh_plan_info vp;
  for (int B : {1, 2, 7, 64}) {
    CHECK(dfh_clipvh_plan(v, B, &vp) == 0 && vp.rows == B * 50 && vp.patch_rows == B * 49 && vp.head_dim == 64 && vp.num_launches == 5 && vp.ldvt == 56);
    CHECK(vp.packed_bytes == up(D * 192 * 2) + L * per_layer && check_plan(vp, dfh_clipvh_workspace_bytes(v, B)) == 0);
    CHECK(vp.launches[1].out2_region >= 0 && vp.regions[vp.launches[1].out2_region].bytes >= (size_t)B * D * vp.ldvt * 2);
  }
  CHECK(refused(dfh_clipvh_plan(v, 0, &vp), "half_plan: batch must be in") && refused(dfh_clipvh_plan(nullptr, 1, &vp), "half_plan: null argument"));
  CHECK(dfh_clipvh_workspace_bytes(v, 0) == 0 && dfh_clipvh_workspace_bytes(v, 65536) == 0);
  const size_t vneed = dfh_clipvh_workspace_bytes(v, 2);
  {
    const int n = dfh_clipv_num_params(v);
    std::vector<const float*> p(n, fake);
    std::vector<float*> hs(L + 1, fake);
    CHECK(refused(dfh_clipvh_pack(v, p.data(), n, nullptr, nullptr), "dfh_clipvh_pack: null argument"));
    CHECK(refused(dfh_clipvh_pack(v, p.data(), n + 1, packed, nullptr), "count does not match dfh_clipv_num_params"));
    CHECK(refused(dfh_clipvh_pack(v, p.data(), n, (char*)packed + 16, nullptr), "dfh_clipvh_pack: the packed copy must be 256-byte aligned"));
    auto enc = [&](const float* const* arr, int cnt, const void* px, int dt, int B, float* last, float* const* taps, void* w, size_t wb, const void* pk) {
      return dfh_clipvh_encode(v, arr, cnt, pk, px, dt, B, last, nullptr, nullptr, taps, w, wb, nullptr);
    };
    CHECK(refused(enc(p.data(), n, nullptr, 0, 2, fake, nullptr, ws, vneed, packed), "dfh_clipvh_encode: null argument"));
    CHECK(refused(enc(p.data(), n - 1, fake, 0, 2, fake, nullptr, ws, vneed, packed), "count does not match dfh_clipv_num_params"));
    p[3] = fake + 1; CHECK(refused(enc(p.data(), n, fake, 2, 0, fake, nullptr, ws, vneed, packed), "not 16-byte aligned")); p[3] = fake;   // before pixel_dtype and the plan
    CHECK(refused(enc(p.data(), n, fake, 2, 0, fake, nullptr, ws, vneed, packed), "dfh_clipvh_encode: pixel_dtype"));                 // before the plan
    CHECK(refused(enc(p.data(), n, fake, 0, 0, fake, nullptr, ws, vneed, packed), "half_plan: batch must be in"));
    CHECK(refused(enc(p.data(), n, fake, 0, 2, fake, nullptr, ws, vneed - 1, packed), "dfh_clipvh_encode: workspace smaller than dfh_clipvh_workspace_bytes"));
    CHECK(refused(enc(p.data(), n, fake, 0, 2, fake, nullptr, (char*)ws + 16, vneed, packed), "dfh_clipvh_encode: workspace / packed copy must be 256-byte aligned"));
    CHECK(refused(enc(p.data(), n, fake, 0, 2, fake, nullptr, ws, vneed, (char*)packed + 128), "workspace / packed copy must be 256-byte aligned"));
    CHECK(refused(enc(p.data(), n, (char*)fake + 2, 0, 2, fake, nullptr, ws, vneed, packed), "pixel_values must be aligned to its element size"));
    CHECK(refused(enc(p.data(), n, (char*)fake + 1, 1, 2, fake, nullptr, ws, vneed, packed), "pixel_values must be aligned to its element size"));
    CHECK(refused(enc(p.data(), n, fake, 0, 2, fake + 1, nullptr, ws, vneed, packed), "outputs must be 16-byte aligned"));
    hs[L] = fake + 2; CHECK(refused(enc(p.data(), n, fake, 0, 2, fake, hs.data(), ws, vneed, packed), "hidden_states[2] must be 16-byte aligned"));
  }
  dfh_clipv_destroy(v);
  vc.patch_size = 14;
  CHECK(dfh_clipv_create(&vc, &v) == 0 && v);
  CHECK(dfh_clipvh_plan(v, 3, &vp) == 0 && vp.patch_k == 588 && vp.patch_k_padded == 592 && vp.tokens == 17 && vp.ldvt == 24);
  CHECK(vp.packed_bytes == up(D * 592 * 2) + L * per_layer && check_plan(vp, dfh_clipvh_workspace_bytes(v, 3)) == 0);
  dfh_clipv_destroy(v);
  vc.hidden_size = 192; vc.intermediate_size = 768; vc.num_attention_heads = 3;     // 576 columns on 160-column tiles: V^T would begin inside one
  CHECK(dfh_clipv_create(&vc, &v) == 0 && v);
  CHECK(refused(dfh_clipvh_plan(v, 3, &vp), "2 x hidden must be a multiple of 160") && dfh_clipvh_packed_bytes(v) == 0);
  dfh_clipv_destroy(v);
  std::puts("clip_half_tower_host_check: both 16-bit towers planned, their plans and packed layouts checked, every bad call refused; no launch reached");
  return 0;
}

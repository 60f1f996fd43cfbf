// Host-only walk over everything the U-Net and VAE runtime objects decide before a kernel runs, for a sanitizer build and for comparing
// two trees as text (CPU machine, no GPU, never loaded into python).  Nothing here launches a kernel.  This file includes unet_train.hip
// and vae.hip (TrainRun and dfh_vae are defined there), so it takes their place in the source list of the tree it lies in:
//
//   cd difashion_amd/csrc && mkdir -p /tmp/hc && SRCS=$(sed -n 's/^SRCS = //p' Makefile) && \
//   for f in $SRCS ../../scripts/unet_model_host_check.hip; do case $f in unet_train.hip|vae.hip) continue;; esac; echo $f; done | \
//     xargs -P 8 -I{} sh -c 'hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//       -Xarch_host -fno-sanitize-recover=undefined -c {} -o /tmp/hc/$(basename {} .hip).o' && \
//   hipcc -fsanitize=address,undefined /tmp/hc/*.o -o /tmp/hc/unet_model_host_check && /tmp/hc/unet_model_host_check > new.txt
//
// Copied into a checkout of the commit before unet_model.h was split, the same file compiles there with -DHOST_CHECK_BEFORE_SPLIT (that
// tree kept the plan in separate members, and has no bounded allocators to check); the two outputs are equal as text
// (profiles/unet_split/host_check.txt).
//
// Prints, for the sd15 / sd2base / tiny / glue configs of scripts/walk_plans.py: packs and tpacks, the arena / fold / fp8-arena layout of
// every layer, and persist / temp / slab bytes of the dry inference walk (bf16 and fp8 contexts), the run-cache sizes and the dry training
// walk at batch 1 and 16; the same for the smallest VAE.  Then binds a WalkBase to a region one byte too small and allocates past the caps
// of a bound one: both must be refused with rc set.
#include <cstdio>
#include <cstdlib>

#include "../difashion_amd/csrc/unet_train.hip"
#include "../difashion_amd/csrc/vae.hip"

namespace dfh { const char* last_error(); }
#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "line %d: %s  (last error: %s)\n", __LINE__, #cond, dfh::last_error()); return 1; } } while (0)

struct Plan3 { size_t persist, temp, slab; };
#ifdef HOST_CHECK_BEFORE_SPLIT
static Plan3 plan_of(const dfh_unet& u) { return {u.plan_persist, u.plan_temp, u.plan_partial}; }
static Plan3 plan_of(const dfh_vae& v) { return {v.plan_persist, v.plan_temp, v.plan_partial}; }
static size_t total_of(const dfh_unet& u) { return u.plan_total; }
#else
static Plan3 plan_of(const dfh_unet& u) { return {u.plan.persist, u.plan.temp, u.plan.slab}; }
static Plan3 plan_of(const dfh_vae& v) { return {v.plan.persist, v.plan.temp, v.plan.slab}; }
static size_t total_of(const dfh_unet& u) { return u.plan_total(); }
#endif
static char* const kFake = (char*)(uintptr_t)(1 << 20);
static size_t up256(size_t n) { return (n + 255) & ~(size_t)255; }

struct Spec { const char* name; int size, boc[4], xdim, heads[4], linproj; };
static const Spec kUnets[] = {
  {"sd15", 64, {320, 640, 1280, 1280}, 768, {8, 8, 8, 8}, 0},
  {"sd2base", 64, {320, 640, 1280, 1280}, 1024, {5, 10, 20, 20}, 1},
  {"tiny", 16, {64, 128, 256, 256}, 64, {2, 2, 2, 2}, 0},
  {"glue", 16, {32, 64, 128, 128}, 64, {1, 2, 2, 2}, 0},
};

static dfh_unet* make_unet(const Spec& sp) {
  dfh_unet_config c{};
  c.sample_size = sp.size; c.in_channels = 8; c.out_channels = 4; c.num_blocks = 4;
  for (int i = 0; i < 4; ++i) { c.block_out_channels[i] = sp.boc[i]; c.num_heads[i] = sp.heads[i]; c.down_attn[i] = i < 3; }
  c.layers_per_block = 2; c.cross_attention_dim = sp.xdim; c.use_linear_projection = sp.linproj;
  c.norm_num_groups = 32; c.norm_eps = 1e-5f; c.text_len = 77;
  dfh_unet* u = nullptr;
  return dfh_unet_create(&c, &u) == 0 ? u : nullptr;
}
// made-up, aligned addresses, never dereferenced: the dry walks offset from them
static void fake_bind(dfh_unet* u) {
  u->arena16 = (bf16_t*)kFake; u->arena32 = (float*)kFake; u->ws = kFake; u->arena8 = (unsigned char*)kFake;
  u->arena16t = (bf16_t*)kFake; u->grad16 = (float*)kFake; u->grad32 = (float*)kFake;
}

static void print_packs(const ParamTable& t) {
  for (const PackOp& o : t.packs)
    std::printf("  pack %s kind=%d dst=%zu N=%d K=%d ldw=%d row=%d col=%d geglu=%d acc=%d cin_pad=%d\n", t.params[o.param].name.c_str(), o.kind, o.dst,
                o.N, o.K, o.ldw, o.row_off, o.col_off, o.geglu, o.accumulate, o.cin_pad);
  std::printf("  a16=%zu a32=%zu\n", t.a16, t.a32);
}
static void print_m8(const char* n, const Mat8& m) { std::printf(" %s=%zu/%zu/%zu/%dx%d/%d", n, m.off, m.soff, m.boff, m.N, m.K, (int)m.on); }
static void print_res(const ResL& r) {
  std::printf("  res %s cin=%d cout=%d temb_off=%d sc=%d w1=%zu w2=%zu n1=%zu/%zu b1=%zu n2=%zu/%zu b2=%zu u=%d/%zu/%zu t=%zu/%zu/%zu\n", r.pre.c_str(), r.cin,
              r.cout, r.temb_off, (int)r.shortcut, r.w1.off, r.w2.off, r.n1w.off, r.n1b.off, r.b1.off, r.n2w.off, r.n2b.off, r.b2.off, (int)r.has_u, r.u1,
              r.u2, r.w1t.off, r.w2t.off, r.wst.off);
}
static void print_att(const AttL& a) {
  std::printf("  att %s C=%d heads=%d x_off=%d idx=%d mats=%zu/%zu/%zu/%zu/%zu/%zu/%zu/%zu/%zu", a.pre.c_str(), a.C, a.heads, a.x_off, a.idx, a.pin.off, a.qk.off,
              a.v.off, a.o1.off, a.q2.off, a.o2.off, a.ff1.off, a.ff2.off, a.pout.off);
  for (const Vec* v : {&a.nw, &a.nb, &a.pinb, &a.l1w, &a.l1b, &a.o1b, &a.l2w, &a.l2b, &a.o2b, &a.l3w, &a.l3b, &a.ff1b, &a.ff2b, &a.poutb}) std::printf(" v%zu", v->off);
  for (const Fold* f : {&a.fqkv, &a.fqk, &a.fv, &a.fq2, &a.fff1, &a.fffp}) std::printf(" f%zu/%zu/%zu/%dx%d", f->w, f->s, f->b, f->N, f->K);
  std::printf(" mlp=%d/%zu tl=%d t=%zu/%zu/%zu/%zu/%zu/%zu/%zu/%zu", (int)a.has_mlp, a.mlp_img, (int)a.has_tl, a.pint.off, a.qkvt.off, a.o1t.off, a.q2t.off,
              a.o2t.off, a.ff1t.off, a.ff2t.off, a.poutt.off);
  print_m8("qk8", a.qk8); print_m8("v8", a.v8); print_m8("q28", a.q28); print_m8("ff18", a.ff18); print_m8("o18", a.o18); print_m8("o28", a.o28);
  print_m8("ff28", a.ff28); print_m8("pout8", a.pout8); print_m8("pin8", a.pin8);
  std::printf(" f8a=%d/%zu\n", (int)a.f8a, a.f8a_off);
}
static void print_conv(const ConvL& c) {
  std::printf("  conv %s cin=%d cout=%d w=%zu b=%zu ph=%d/%zu t=%zu\n", c.pre.c_str(), c.cin, c.cout, c.w.off, c.b.off, (int)c.has_ph, c.ph, c.wt.off);
}
// every layer, in the order the walk visits them
static void print_layers(dfh_unet& u) {
  print_conv(u.conv_in);
  for (size_t i = 0; i < u.down_res.size(); ++i) {
    for (size_t j = 0; j < u.down_res[i].size(); ++j) { print_res(u.down_res[i][j]); if (!u.down_att[i].empty()) print_att(u.down_att[i][j]); }
    if (i + 1 < u.down_res.size()) print_conv(u.down_samp[i]);
  }
  print_res(u.mid_res[0]); print_att(u.mid_att); print_res(u.mid_res[1]);
  for (size_t i = 0; i < u.up_res.size(); ++i) {
    for (size_t j = 0; j < u.up_res[i].size(); ++j) { print_res(u.up_res[i][j]); if (!u.up_att[i].empty()) print_att(u.up_att[i][j]); }
    if (i + 1 < u.up_res.size()) print_conv(u.up_samp[i]);
  }
  print_conv(u.conv_out);
  std::printf("  te1=%zu te2=%zu tproj=%zu kx_all=%zu vx_all=%zu te2t=%zu tprojt=%zu temb_total=%d x_total=%d\n", u.te1.off, u.te2.off, u.tproj.off,
              u.kx_all.off, u.vx_all.off, u.te2t.off, u.tprojt.off, u.temb_total, u.x_total);
  std::printf("  fold16=%zu fold32=%zu fold_bytes=%zu a16t=%zu a8=%zu a8_slab_off=%zu n_att=%d\n", u.fold16, u.fold32, u.fold_bytes(), u.a16t, u.a8,
              u.a8_slab_off, u.n_att);
}
static int print_walks(dfh_unet& u, const char* what) {
  for (int B : {1, 16}) {
    CHECK(dfh_unet_workspace_bytes(&u, B) == total_of(u));
    const Plan3 p = plan_of(u);
    std::printf("  %s walk B=%d persist=%zu temp=%zu slab=%zu total=%zu run_cache(n_t=50)=%zu xamax=%zu\n", what, B, p.persist, p.temp, p.slab, total_of(u),
                u.run_cache_bytes(B, 50), u.cache_xamax_bytes(B));
  }
  return 0;
}

#ifndef HOST_CHECK_BEFORE_SPLIT
static bool refused(const char* with) { return std::string(dfh::last_error()).find(with) != std::string::npos; }
static int check_bounds() {
  ParamTable pt;
  static char region[4 << 20];
  WalkBase dry(pt, 32, 2, nullptr, true);
  CHECK(dry.persist.base != nullptr && dry.persist.rc == nullptr);
  (void)dry.persist.alloc(1000); (void)dry.temp.alloc(3000); (void)dry.temp.alloc(1 << 20);      // a dry walk is unbounded
  dry.temp.off = 0;
  CHECK(dry.rc == 0 && dry.temp.peak > (1 << 20));
  dry.temp.peak = 3000;
  const WorkspacePlan p = dry.plan();
  CHECK(p.persist == 1024 && p.temp == 3072 && p.slab == 0 && p.batch == 2 && p.total() == WorkspaceHead(nullptr, 2, 0).bytes + 4096 && p.total() < sizeof(region));
  {   // one byte short: refused before anything is laid out or enqueued
    WalkBase w(pt, 32, 2, nullptr, false);
    CHECK(!w.bind(region, p.total() - 1, p) && w.rc == -1 && refused("workspace too small") && w.zero == nullptr && w.persist.base == nullptr);
  }
  {   // another batch than the planned one
    WalkBase w(pt, 32, 3, nullptr, false);
    CHECK(!w.bind(region, sizeof(region), p) && w.rc == -1 && refused("planned batch"));
  }
  {   // a bound walk: inside the caps everything is handed out, past them nothing is.  (Without a device the zero-page memset of bind()
      // fails: its rc is cleared here, the layout it made is what is under test.)
    WalkBase w(pt, 32, 2, nullptr, false);
    (void)w.bind(region, p.total(), p);
    CHECK(w.zero == (bf16_t*)region && w.persist.base == region + WorkspaceHead(nullptr, 2, 0).bytes && w.temp.base == w.persist.base + 1024);
    w.rc = 0;
    CHECK(w.persist.alloc(1024) == w.persist.base && w.rc == 0);
    CHECK(w.persist.alloc(1) == w.persist.base && w.rc == -1 && refused("workspace region too small: persist"));
    w.rc = 0;
    CHECK(w.temp.alloc(3000) == w.temp.base && w.rc == 0);
    w.temp.off = 0;
    CHECK(w.temp.alloc(3073) == w.temp.base && w.rc == -1 && refused("workspace region too small: temp") && w.temp.off == 0);
    GemmArgs g = WalkBase::base(8, 8);
    w.gemm(g);                                 // rc is set: nothing further is launched (a launch would fail otherwise: no operands)
    CHECK(w.rc == -1 && refused("region too small: temp"));
  }
  return 0;
}
#endif

int main() {
  for (const Spec& sp : kUnets) {
    std::printf("unet %s\n", sp.name);
    dfh_unet* u = make_unet(sp);
    CHECK(u != nullptr);
    fake_bind(u);
    print_packs(*u);
    CHECK(print_walks(*u, "bf16") == 0);
    CHECK(u->build_train() == 0);
    for (const TPackOp& o : u->tpacks)
      std::printf("  tpack %s conv=%d dst=%zu N=%d K=%d ldt=%d row=%d col=%d geglu=%d o_pad=%d\n", u->params[o.param].name.c_str(), o.conv, o.dst, o.N, o.K,
                  o.ldt, o.t_row_off, o.t_col_off, o.geglu, o.o_pad);
    print_layers(*u);
    for (int B : {1, 16}) {
      dfh_unet::TrainRun r(u, B, nullptr, true);
      r.walk(nullptr, 0, nullptr, nullptr, 0, nullptr);
      const size_t entries = r.tape.size();
      for (int i = (int)entries - 1; i >= 0; --i) { r.cur_entry = i; r.tape[i](); }
      CHECK(r.rc == 0);
      std::printf("  train walk B=%d persist=%zu temp=%zu slab=%zu tape=%zu writes=%zu workspace=%zu\n", B, up256(r.persist.peak), up256(r.temp.peak),
                  up256(r.partial_need), entries, r.writes.size(), dfh_unet_train_workspace_bytes(u, B));
    }
    dfh_unet_destroy(u);
    for (int attn : {0, 1}) {
      u = make_unet(sp);
      CHECK(u && dfh_unet_enable_fp8_attention(u, attn) == 0 && dfh_unet_enable_fp8(u) == 0);
      fake_bind(u);
      std::printf(" fp8 attention=%d arena8_bytes=%zu\n", attn, dfh_unet_arena8_bytes(u));
      print_layers(*u);
      CHECK(print_walks(*u, "fp8") == 0);
      dfh_unet_destroy(u);
    }
  }
  {
    std::printf("vae tiny_vae\n");
    dfh_vae_config c{3, 3, 4, 4, {32, 64, 64, 64}, 2, 32};
    dfh_vae* v = nullptr;
    CHECK(dfh_vae_create(&c, &v) == 0 && v);
    v->arena16 = (bf16_t*)kFake; v->arena32 = (float*)kFake;
    print_packs(*v);
    for (int B : {1, 16}) for (int enc : {1, 0}) {
      const size_t total = dfh_vae_workspace_bytes(v, enc, B, enc ? 32 : 4);
      const Plan3 p = plan_of(*v);
      std::printf("  %s walk B=%d persist=%zu temp=%zu slab=%zu total=%zu\n", enc ? "encode" : "decode", B, p.persist, p.temp, p.slab, total);
    }
    dfh_vae_destroy(v);
  }
#ifndef HOST_CHECK_BEFORE_SPLIT
  if (check_bounds()) return 1;
  std::fprintf(stderr, "unet_model_host_check: bounded allocators and bind() refusals as specified; no sanitizer report\n");
#endif
  return 0;
}

// What the three model walks share (the U-Net inference walk of unet_walk.hip, the training walk of unet_train.hip, the VAE of vae.hip):
// the plain types, the parameter table with its packing plan (ParamTable), the layout of a workspace (WorkspaceHead, WorkspacePlan) and the
// launch context of a walk (WalkBase: arenas, bounded allocators, split-K slab planning, the descriptor fills every walk repeats).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/difashion_hip.h"
#include "attention.h"
#include "dfh_common.h"
#include "gemm.h"
#include "norm.h"
#include "packtab.h"

namespace dfhm {

struct Mat { size_t off = 0; int N = 0, K = 0; };    // bf16 [N][K] at arena16 + off (elements)
struct Vec { size_t off = 0; int N = 0; };           // fp32 [N] at arena32 + off (elements)

enum PackKind { PK_VEC = 0, PK_MAT = 1, PK_CONV3 = 2 };      // in the order of TabKind's PACK_* and UNPACK_* triples (OpTable::add)
struct TPackOp;
struct PackOp {
  int param, kind;
  size_t dst;
  int N, K, ldw, row_off, col_off, geglu, accumulate;
  int cin_pad = 0;   // PK_CONV3: channels per tap in the packed layout (conv_in pads 4 -> 8)
};

struct Tensor {
  bf16_t* p = nullptr; int H = 0, W = 0, C = 0;
  // GroupNorm statistics of this tensor written by the GEMM epilogue that produced it (gemm.h GemmArgs::gstat); null when the
  // launch ran on a kernel that does not write them -- the consuming GroupNorm then computes its own
  const float* gst = nullptr; int gst_cpg = 0, gst_chunks = 0;
};

// A region of a workspace handed out front to back.  A planning (dry) walk leaves it unbounded and reads `peak`; WalkBase::bind gives the
// region of a real walk its planned size (cap) and the walk's error slot (rc): an allocation past the cap is refused there, and with rc
// set the walk launches nothing further.
struct Bump {
  char* base = nullptr; size_t cap = 0, off = 0, peak = 0;
  const char* name = ""; int* rc = nullptr;          // rc != null: bounded by cap
  void* alloc(size_t bytes) {
    off = (off + 255) & ~(size_t)255;
    if (rc && off + bytes > cap) { dfh::set_error(std::string("workspace region too small: ") + name); *rc = -1; return base; }
    char* p = (char*)((uintptr_t)base + off);        // (planning arithmetic runs on a null base: WorkspaceHead)
    off += bytes;
    if (off > peak) peak = off;
    return p;
  }
};

// host copy + device copy of a TabOp table; re-uploaded only when an entry (e.g. a master pointer) changed
struct OpTable {
  std::vector<TabOp> host, uploaded; TabOp* dev = nullptr; size_t cap = 0; unsigned blocks = 0;
  void clear() { host.clear(); blocks = 0; }
  void add(void* master, int kind, long dst, int N, int K, int ld, int p0, int p1, int p2, int p3, long /*elems*/) {
    TabOp op; std::memset(&op, 0, sizeof(op));
    op.master = master; op.dst = dst; op.kind = kind; op.N = N; op.K = K; op.ld = ld; op.p0 = p0; op.p1 = p1; op.p2 = p2; op.p3 = p3;
    op.first_block = blocks;
    blocks += dfh::tab_blocks(kind, N, K);
    host.push_back(op);
  }
  // a PackOp as the table op of its kind.  unpack < 0: the pack (master -> arena); 0 / 1: the un-pack of its gradient (arena -> master),
  // added onto / overwriting the master's
  void add(void* src, const PackOp& op, int unpack = -1) {
    const int k = unpack < 0 ? TAB_PACK_VEC : TAB_UNPACK_VEC, flag = unpack < 0 ? op.accumulate : unpack;
    if (op.kind == PK_VEC) add(src, k + PK_VEC, (long)op.dst, op.N, 0, 0, op.geglu, flag, 0, 0, op.N);
    else if (op.kind == PK_MAT) add(src, k + PK_MAT, (long)op.dst, op.N, op.K, op.ldw, op.row_off, op.col_off, op.geglu, unpack < 0 ? 0 : unpack, (long)op.N * op.K);
    else add(src, k + PK_CONV3, (long)op.dst, op.N, op.K, op.ldw, unpack < 0 ? 0 : unpack, op.col_off, 0, op.cin_pad, (long)op.N * op.K * 9);
  }
  void add(void* src, const TPackOp& op);            // the transposed pack of the training path (unet_model.h, where TPackOp lives)
  // a PACK2 op: the plain pack (dst .. p3 as in add) and the transposed pack (dst2, ld2, q0 = t_row_off, q1 = t_col_off, q3 = o_pad) of one master
  void add2(void* master, int kind, long dst, int N, int K, int ld, int p0, int p1, int p2, int p3, long dst2, int ld2, int q0, int q1, int q3) {
    add(master, kind, dst, N, K, ld, p0, p1, p2, p3, 0);
    TabOp& op = host.back();
    op.dst2 = dst2; op.ld2 = ld2; op.q0 = q0; op.q1 = q1; op.q3 = q3;
  }
  int launch(void* arena_vec, void* arena_mat, hipStream_t s, void* arena_mat2 = nullptr, float* sq_partials = nullptr) {
    if (host.empty()) return 0;
    const size_t bytes = host.size() * sizeof(TabOp);
    if (host.size() != uploaded.size() || std::memcmp(host.data(), uploaded.data(), bytes) != 0) {
      if (host.size() > cap) {
        if (dev) (void)hipFree(dev);
        if (hipMalloc((void**)&dev, bytes) != hipSuccess) { dfh::set_error("hipMalloc of an op table failed"); return -1; }
        cap = host.size();
      }
      // rare (first use / parameters re-homed): stream-ordered with respect to earlier launches that read the old table
      if (hipStreamSynchronize(s) != hipSuccess || hipMemcpy(dev, host.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) {
        dfh::set_error("uploading an op table failed"); return -1;
      }
      uploaded = host;
    }
    return dfh::table_launch(dev, (int)host.size(), blocks, arena_vec, arena_mat, s, arena_mat2, sq_partials);
  }
  ~OpTable() { if (dev) (void)hipFree(dev); }
};

// Parameter table + packing plan of a model: the master parameters in checkpoint order (params), where each goes in the packed bf16 /
// fp32 arenas (packs), and the arenas themselves.  The model's build() fills it through the helpers; pack_params() runs the plan.
struct ParamTable : dfh::ParamList {
  std::vector<PackOp> packs;
  size_t a16 = 0, a32 = 0;         // arena sizes in elements
  bf16_t* arena16 = nullptr; float* arena32 = nullptr;
  OpTable tab_pack, tab_pack_acc;

  size_t alloc16(size_t n) { size_t o = a16; a16 += (n + 127) & ~(size_t)127; return o; }
  size_t alloc32(size_t n) { size_t o = a32; a32 += (n + 63) & ~(size_t)63; return o; }

  // npad: the vector is allocated (and read by the kernels) npad long; the rows past N stay zero
  Vec vec(const std::string& name, int N, int npad = 0) {
    Vec v; v.N = npad ? npad : N; v.off = alloc32(v.N);
    int p = add_param(name, {N});
    packs.push_back({p, PK_VEC, v.off, N, 0, 0, 0, 0, 0, 0});
    return v;
  }
  // packs a vector parameter into an existing fp32 range (batched biases / fused shortcut bias)
  void vec_into(const std::string& name, int N, size_t dst, int geglu, int accumulate) {
    int p = add_param(name, {N});
    packs.push_back({p, PK_VEC, dst, N, 0, 0, 0, 0, geglu, accumulate});
  }
  Mat mat_alloc(int N, int K) { Mat m; m.N = N; m.K = K; m.off = alloc16((size_t)N * K); return m; }
  void mat_into(const std::string& name, int N, int K, bool as_conv1x1, const Mat& dst, int row_off, int col_off, int geglu) {
    std::vector<int> shape = as_conv1x1 ? std::vector<int>{N, K, 1, 1} : std::vector<int>{N, K};
    int p = add_param(name, shape);
    packs.push_back({p, PK_MAT, dst.off, N, K, dst.K, row_off, col_off, geglu, 0});
  }
  Mat mat(const std::string& name, int N, int K, bool as_conv1x1 = false, int geglu = 0) {
    Mat m = mat_alloc(N, K);
    mat_into(name, N, K, as_conv1x1, m, 0, 0, geglu);
    return m;
  }
  void conv_into(const std::string& name, int cout, int cin, const Mat& dst, int col_off, int cin_pad = 0) {
    int p = add_param(name, {cout, cin, 3, 3});
    PackOp op{p, PK_CONV3, dst.off, cout, cin, dst.K, 0, col_off, 0, 0};
    op.cin_pad = cin_pad ? cin_pad : cin;
    packs.push_back(op);
  }

  // every PackOp in one launch (plus one for the few biases that ADD onto an already packed vector)
  int pack_params(const float* const* master, int count, hipStream_t s) {
    DFH_REQUIRE(count == (int)params.size(), "parameter count mismatch");
    DFH_REQUIRE(arena16 && arena32, "arenas not bound");
    tab_pack.clear(); tab_pack_acc.clear();
    for (const PackOp& op : packs) {
      void* src = (void*)master[op.param];
      DFH_REQUIRE(src != nullptr, "null master parameter: " + params[op.param].name);
      (op.kind == PK_VEC && op.accumulate ? tab_pack_acc : tab_pack).add(src, op);
    }
    if (int rc = tab_pack.launch(arena32, arena16, s)) return rc;
    return tab_pack_acc.launch(arena32, arena16, s);
  }

  // bodies of the dfh_{unet,vae}_arena*_bytes entry points (the table's own: dfh::ParamList)
  size_t arena16_bytes() const { return a16 * 2 + 256; }
  size_t arena32_bytes() const { return a32 * 4 + 256; }
};

// The head of every walk's workspace: a 256-byte zero page, the GroupNorm partial sums of a batch of B, then n split-K slab regions of
// slab_bytes each.  The same layout serves the live walk (base = where the head starts) and the planning arithmetic (base = null, only
// `bytes` is read).
struct WorkspaceHead {
  bf16_t* zero; float* gn_partial; float* slab[2]; size_t slab_bytes;
  size_t bytes;                    // the whole head, rounded to 256: what follows starts at base + bytes
  WorkspaceHead(char* base, int B, size_t slab_bytes_, int n = 1) : slab_bytes(slab_bytes_) {
    Bump h; h.base = base;
    zero = (bf16_t*)h.alloc(256);
    gn_partial = (float*)h.alloc((size_t)B * GN_MAX_CHUNKS * 64 * 2 * sizeof(float));
    slab[0] = slab[1] = nullptr;
    for (int i = 0; i < n; ++i) slab[i] = (float*)h.alloc(slab_bytes);
    bytes = (h.off + 255) & ~(size_t)255;
  }
};

// What a planning (dry) walk found a workspace needs behind its head: the two allocator regions and the split-K slab bytes (each rounded
// to 256), for which batch, and how many slab regions the head holds (2: the training walk's side stream has its own).  recomp: the
// recompute region of a checkpointing training walk (unet_train.hip), behind the other two; 0 everywhere else, which leaves the layout
// of head | persist | temp what it is without it.
struct WorkspacePlan {
  size_t persist = 0, temp = 0, slab = 0; int batch = 0, nslab = 1; size_t recomp = 0;
  size_t head() const { return WorkspaceHead(nullptr, batch, slab, nslab).bytes; }
  size_t total() const { return batch ? head() + persist + temp + recomp : 0; }
};

// Launch context of one walk over a model: the batch, the stream, dry (planning: allocate and size, launch nothing), the first error, the
// two bump allocators (and the recompute region only a checkpointing training walk allocates from), and the split-K slab region with the
// size the dry run found it needs.
struct WalkBase {
  const ParamTable& pt; int groups;            // groups: GroupNorm groups of the model
  int B; hipStream_t s; bool dry;
  Bump persist, temp, recomp; size_t partial_need = 0;
  float* partial = nullptr; size_t partial_cap = 0;
  float* partial2 = nullptr;                   // the second slab region of a two-slab head (else null)
  float* gn_partial = nullptr; bf16_t* zero = nullptr;
  int rc = 0;
  WalkBase(const ParamTable& pt_, int groups_, int B_, hipStream_t s_, bool dry_) : pt(pt_), groups(groups_), B(B_), s(s_), dry(dry_) {
    // a planning walk hands out addresses that are never dereferenced: from a made-up base, so that offsets from them are defined
    if (dry) persist.base = temp.base = recomp.base = (char*)(uintptr_t)(1 << 20);
  }
  WalkBase(const WalkBase&) = delete;          // the allocators of a bound walk point at its rc

  // what this (dry) walk needs
  WorkspacePlan plan(int nslab = 1) const {
    auto up = [](size_t n) { return (n + 255) & ~(size_t)255; };
    WorkspacePlan p; p.persist = up(persist.peak); p.temp = up(temp.peak); p.slab = up(partial_need); p.batch = B; p.nslab = nslab;
    p.recomp = up(recomp.peak);
    return p;
  }
  // A real walk over [base, base + bytes): head | persist | temp | recomp as planned, the allocators bounded by their planned sizes, the zero
  // page cleared on the stream.  Refuses (rc, false) a plan for another batch and a workspace smaller than the plan.
  bool bind(char* base, size_t bytes, const WorkspacePlan& p) {
    if (B != p.batch) { dfh::set_error("walk batch differs from the planned batch"); rc = -1; return false; }
    if (p.total() > bytes) { dfh::set_error("workspace too small"); rc = -1; return false; }
    const WorkspaceHead h(base, B, p.slab, p.nslab);
    zero = h.zero; gn_partial = h.gn_partial; partial = h.slab[0]; partial2 = h.slab[1]; partial_cap = h.slab_bytes;
    persist = Bump{base + h.bytes, p.persist, 0, 0, "persist", &rc};
    temp = Bump{base + h.bytes + p.persist, p.temp, 0, 0, "temp", &rc};
    recomp = Bump{base + h.bytes + p.persist + p.temp, p.recomp, 0, 0, "recompute", &rc};
    if (hipMemsetAsync(zero, 0, 256, s) != hipSuccess) { dfh::set_error("hipMemsetAsync failed (zero page)"); rc = -2; }
    return rc == 0;
  }

  bf16_t* w16(const Mat& m) const { return pt.arena16 + m.off; }
  float* v32(const Vec& v) const { return pt.arena32 + v.off; }

  // zero page and slab region of a launch; false when there is nothing to launch: the dry run (records the slab need) or slabs too small
  bool gemm_ready(GemmArgs& g) {
    g.zero = zero; g.partial = partial;
    if (dry) { partial_need = std::max(partial_need, dfh::gemm_partial_floats(g) * sizeof(float)); return false; }
    if (dfh::gemm_partial_floats(g) * sizeof(float) > partial_cap) { dfh::set_error("split-K partial buffer too small"); rc = -1; return false; }
    return true;
  }
  void gemm(GemmArgs g) {
    if (rc) return;
    if (gemm_ready(g)) rc = dfh::gemm_launch(g, s);
  }
  static GemmArgs base(int M, int N) {
    GemmArgs g; std::memset(&g, 0, sizeof(g));
    g.M = M; g.N = N; g.rows_per_b = M; g.out_mode = OUT_BF16; g.ld_out = N;
    return g;
  }
  // out = x . W^T + bias (+resid); x rows [M][K]
  GemmArgs linear_desc(const bf16_t* x, int M, int K, const Mat& W, const Vec* bias, const bf16_t* resid, void* out, int N,
                       int out_mode = OUT_BF16) const {
    GemmArgs g = base(M, N);
    g.p_src[0] = x; g.p_c[0] = K; g.nplain = 1;
    g.W = w16(W); g.ldw = W.K;
    g.bias = bias ? v32(*bias) : nullptr;
    g.resid = resid; g.ld_res = N;
    g.out = out; g.out_mode = out_mode;
    return g;
  }
  // 3x3 conv (pad 1) as implicit GEMM over the NHWC source; stride 2 / ups: fused nearest-2x upsample in front
  GemmArgs conv_desc(const bf16_t* src, int C, int Hin, int Win, int Hout, int Wout, int stride, int ups, int N) const {
    GemmArgs g = base(B * Hout * Wout, N);
    g.conv_src = src; g.conv_c = C; g.ntaps = 9;
    g.Hin = Hin; g.Win = Win; g.Hout = Hout; g.Wout = Wout; g.stride = stride; g.ups = ups;
    return g;
  }
  // ... with the packed weights [W.N][9 C (+ shortcut segment)] and the bias of a conv layer
  GemmArgs conv_desc(const bf16_t* src, int C, int Hin, int Win, int Hout, int Wout, int stride, int ups, const Mat& W, const Vec& bias) const {
    GemmArgs g = conv_desc(src, C, Hin, Win, Hout, Wout, stride, ups, W.N);
    g.W = w16(W); g.ldw = W.K; g.bias = v32(bias);
    return g;
  }
  // The second conv of a resnet over the normalised g2 ([cout] channels).  The block input x0 (| x1: the channel concatenation) rides along
  // as K segments under the 1x1-shortcut columns of w2 -- or, without a shortcut, is the residual.  g2 null: the shortcut GEMM alone, no
  // bias (the Winograd walk, whose output transform adds it to the conv)
  GemmArgs conv2_desc(const bf16_t* g2, int H, int W, int cout, const Mat& w2, const Vec& b2, bool shortcut, const bf16_t* x0, int c0,
                      const bf16_t* x1, int c1) const {
    GemmArgs g = g2 ? conv_desc(g2, cout, H, W, H, W, 1, 0, w2, b2) : base(B * H * W, cout);
    if (!g2) { g.W = w16(w2) + 9 * cout; g.ldw = w2.K; }
    if (shortcut) {
      g.p_src[0] = x0; g.p_c[0] = c0; g.nplain = 1;
      if (x1) { g.p_src[1] = x1; g.p_c[1] = c1; g.nplain = 2; }
    } else {
      g.resid = x0; g.ld_res = cout;
    }
    return g;
  }
  // GroupNorm (+SiLU) over x0 (| x1: the channel concatenation of the two) into out; statistics inputs / outputs are the caller's
  GnArgs gn_args(const bf16_t* x0, int C0, const bf16_t* x1, int C1, int HW, const Vec& w, const Vec& b, float eps, int silu, bf16_t* out) const {
    GnArgs a; std::memset(&a, 0, sizeof(a));
    a.src0 = x0; a.C0 = C0; a.src1 = x1; a.C1 = C1;
    a.B = B; a.HW = HW; a.G = groups;
    a.gamma = v32(w); a.beta = v32(b); a.eps = eps; a.silu = silu; a.out = out; a.partial = gn_partial;
    return a;
  }
  // softmax(Q K^T / sqrt(D)) V per head, D = C / heads; the output (O / O8), lse and the fp8 factors are the caller's
  AttnArgs attn_args(const bf16_t* Q, int ldq, const bf16_t* K, int ldk, const bf16_t* Vt, int ldvt, int C, int heads, int Nq, int Nk,
                     long vt_bstride) const {
    AttnArgs a; std::memset(&a, 0, sizeof(a));
    a.vt_bstride = vt_bstride;
    a.Q = Q; a.ldq = ldq; a.K = K; a.ldk = ldk; a.Vt = Vt; a.ldvt = ldvt; a.ldo = C;
    a.B = B; a.H = heads; a.D = C / heads; a.Nq = Nq; a.Nk = Nk;
    a.scale = 1.0f / sqrtf((float)a.D);
    return a;
  }
};

}  // namespace dfhm
using namespace dfhm;

// The inference walk of the U-Net: dfh_unet::Run (the launch context with the layers as functions), run() -- the dry walk that plans the
// workspace and the real one -- and run_cache().
#include "unet_model.h"

struct dfh_unet::Run : WalkBase {
  dfh_unet* u;
  int temb_ld = 0;                 // row stride of the time-embedding rows: temb_total, or 0 when the whole batch shares one cached row
  // fp8 walk: per transformer layer and batch element the largest |V| of the self-attention (tracked by the V projection's epilogue,
  // zeroed at the start of the walk) and of the cross-attention (amax_slabs over the text V^T, once per forward or per run): [n_att][B]
  float* amax_self = nullptr; const float* amax_cross = nullptr;
  const dfh::WalkKnobs& kn = dfh::WalkKnobs::get();

  // Ba: the batch every tensor is ALLOCATED for (the call's batch); B: the batch the launches run on.  They differ only inside the
  // shared prefix of a guidance batch whose last `dup` images repeat the inputs of the `dup` images before them (dfh_unet::dup_tail):
  // there B = Ba - dup, and dup_images() then copies the repeated images' rows into place.
  int Ba;
  Run(dfh_unet* u_, int B_, hipStream_t s_, bool dry_) : WalkBase(*u_, u_->cfg.norm_num_groups, B_, s_, dry_), u(u_), Ba(B_) {}
  Tensor palloc(int H, int W, int C) { return Tensor{(bf16_t*)persist.alloc((size_t)Ba * H * W * C * 2), H, W, C}; }
  Tensor talloc(int H, int W, int C) { return Tensor{(bf16_t*)temp.alloc((size_t)Ba * H * W * C * 2), H, W, C}; }
  void dup_bytes(void* p, size_t per_image, int n) {   // images [Ba - n, Ba) := images [Ba - 2n, Ba - n) of a [Ba][per_image bytes] buffer
    if (rc || dry || n <= 0) return;
    char* c = (char*)p;
    if (hipMemcpyAsync(c + (size_t)(Ba - n) * per_image, c + (size_t)(Ba - 2 * n) * per_image, (size_t)n * per_image, hipMemcpyDeviceToDevice, s) != hipSuccess) {
      dfh::set_error("hipMemcpyAsync failed (dup_bytes)"); rc = -2;
    }
  }
  void dup_images(Tensor& t, int n) {               // the same for a tensor; its producer statistics no longer cover it
    t.gst = nullptr;
    dup_bytes(t.p, (size_t)t.H * t.W * t.C * 2, n);
  }

  // o / bump: the output tensor and the allocator it came from when the output feeds a GroupNorm -- the epilogue then leaves
  // that GroupNorm's statistics beside it (64x64 level: the launches the 256 x 160 tile takes).  DFH_GN_PRE=0 turns it off (A/B).
  // rs_bn (out): column tile of the row statistics the launch wrote into g.rowstat (0 = none)
  void gemm(GemmArgs g, Tensor* o = nullptr, Bump* bump = nullptr, int* rs_bn = nullptr) {
    if (rs_bn) *rs_bn = 0;
    if (rc) return;
    float* gst = nullptr;
    const int G = groups;
    // the consumers take at most GN_MAX_CHUNKS chunks per (image, group): a level fits when its 256-row chunk count does; gemm_launch
    // refuses the 128-row writer by itself when HW / 128 would exceed it (96x96 latents: 36 chunks of 256 rows, 72 of 128)
    if (o && bump && kn.gn_pre && o->C % G == 0 && (dfh::gstat_chunks_fit(o->H * o->W, 256) || dfh::gstat_chunks_fit(o->H * o->W, 128))) {
      gst = (float*)bump->alloc((size_t)Ba * G * ((o->H * o->W) / 128) * 2 * sizeof(float));      // same in the dry run; chunks of 256 or 128 pixel rows
      g.gstat = gst; g.gstat_cpg = o->C / G; g.gstat_hw = o->H * o->W;
    }
    if (!gemm_ready(g)) return;
    int gst_rows = 0;
    rc = dfh::gemm_launch(g, s, 0, 0, -1, &gst_rows, rs_bn);
    if (o && gst_rows) { o->gst = gst; o->gst_cpg = g.gstat_cpg; o->gst_chunks = g.gstat_hw / gst_rows; }
  }
  // out = act(x . W^T + bias) (+resid); x rows [M][K]
  // rowstat / rs_bn: ask the launch for the per-row statistics of its output (a LayerNorm folded into the consumers, gemm.h)
  void linear(const bf16_t* x, int M, int K, const Mat& W, const Vec* bias, int act, const bf16_t* resid, void* out,
              int N, int out_mode = OUT_BF16, int ld_out = -1, int rows_per_b = 0, Tensor* o = nullptr, Bump* bump = nullptr,
              float* rowstat = nullptr, int* rs_bn = nullptr) {
    GemmArgs g = linear_desc(x, M, K, W, bias, resid, out, N, out_mode);
    g.act = act; g.ld_out = ld_out < 0 ? (act == ACT_GEGLU ? N / 2 : N) : ld_out;
    if (rows_per_b) g.rows_per_b = rows_per_b;
    g.rowstat = rowstat;
    gemm(g, o, bump, rs_bn);
  }
  // the consumer of a folded LayerNorm: raw rows x [M][K] (K = C of the LayerNorm), statistics st ([C / st_bn][M][2]) from x's producer
  GemmArgs folded(const bf16_t* x, int M, const Fold& f, const float* st, int st_bn, int act, void* out, int out_mode, int ld_out,
                  int rows_per_b) const {
    GemmArgs g = base(M, f.N);
    g.p_src[0] = x; g.p_c[0] = f.K; g.nplain = 1;
    g.W = u->fold_w() + f.w; g.ldw = f.K;
    g.bias = u->fold_v() + f.b; g.ln_s = u->fold_v() + f.s;
    g.ln_stat = st; g.ln_cnt = st_bn; g.ln_parts = st_bn > 0 ? f.K / st_bn : 0; g.ln_eps = 1e-5f;
    g.act = act; g.out = out; g.out_mode = out_mode; g.ld_out = ld_out < 0 ? (act == ACT_GEGLU ? f.N / 2 : f.N) : ld_out;
    if (rows_per_b) g.rows_per_b = rows_per_b;
    return g;
  }
  void groupnorm(const Tensor& x0, const Tensor* x1, const Vec& w, const Vec& b, float eps, int silu, Tensor& out) {
    if (rc || dry) return;
    GnArgs a = gn_args(x0.p, x0.C, x1 ? x1->p : nullptr, x1 ? x1->C : 0, x0.H * x0.W, w, b, eps, silu, out.p);
    if (!x1 && x0.gst && x0.gst_cpg == x0.C / a.G) { a.pre = x0.gst; a.pre_chunks = x0.gst_chunks; }   // summed by its producer
    rc = dfh::groupnorm_launch(a, s);
  }
  bool use8(const Mat8& m) const { return u->fp8 && m.on; }        // the forward entry checks that arena8 is bound
  // LayerNorm whose output is quantised per token + the fp8 GEMM that consumes it (gemm_fp8.hip)
  void layernorm8(const bf16_t* x, const Vec& w, const Vec& b, uint8_t* q, float* sc, int M, int C) {
    if (rc || dry) return;
    rc = dfh::layernorm_fp8_launch(x, v32(w), v32(b), q, sc, M, C, 1e-5f, s);
  }
  void linear8(const uint8_t* q, const float* sc, int M, const Mat8& W, const Vec* bias, int act, void* out, int out_mode = OUT_BF16,
               int ld_out = -1, int rows_per_b = 0, float* amax = nullptr) {
    if (rc || dry) return;
    Fp8GemmArgs g; std::memset(&g, 0, sizeof(g));
    g.A = q; g.sA = sc; g.W = u->arena8 + W.off; g.sW = (const float*)(u->arena8 + W.soff);
    g.M = M; g.N = W.N; g.K = W.K; g.bias = bias ? v32(*bias) : nullptr; g.act = act;
    g.out = out; g.out_mode = out_mode; g.ld_out = ld_out < 0 ? (act == ACT_GEGLU ? W.N / 2 : W.N) : ld_out;
    g.rows_per_b = rows_per_b; g.zero = (const uint8_t*)zero; g.amax = amax;
    rc = dfh::gemm_fp8_launch(g, s);
  }
  // ---- fp8 walk (round 4): every operand of these launches is e4m3
  Fp8GemmArgs args8(const uint8_t* A, int M, const Mat8& W, const Vec* bias, void* out) const {
    Fp8GemmArgs g; std::memset(&g, 0, sizeof(g));
    g.A = A; g.W = u->arena8 + W.off; g.sW = (const float*)(u->arena8 + W.soff);
    g.M = M; g.N = W.N; g.K = W.K; g.bias = bias ? v32(*bias) : nullptr;
    g.out = out; g.out_mode = OUT_BF16; g.ld_out = W.N; g.zero = (const uint8_t*)zero;
    return g;
  }
  void gemm8(const Fp8GemmArgs& g) {
    if (rc || dry) return;
    rc = dfh::gemm_fp8_launch(g, s);
  }
  // GroupNorm without its affine, as e4m3 under the static scale 448 / GN_Z (the consumer's weights carry gamma)
  void groupnorm8(const Tensor& x, float eps, uint8_t* q) {
    if (rc || dry) return;
    GnArgs a; std::memset(&a, 0, sizeof(a));
    a.src0 = x.p; a.C0 = x.C; a.B = B; a.HW = x.H * x.W; a.G = u->cfg.norm_num_groups; a.eps = eps; a.partial = gn_partial;
    a.out8 = q; a.q_mul = 448.0f / dfh_unet::GN_Z;
    if (x.gst && x.gst_cpg == x.C / a.G) { a.pre = x.gst; a.pre_chunks = x.gst_chunks; }
    rc = dfh::groupnorm_launch(a, s);
  }
  // f8: operand factors of the fp8 attention products (AttL::f8a_off) or null
  void attention8(const bf16_t* Q, int ldq, const bf16_t* K, int ldk, const bf16_t* Vt, int ldvt, uint8_t* O8, const float* amax, int C,
                  int heads, int Nq, int Nk, long vt_bstride = 0, const float* f8 = nullptr) {
    if (rc || dry) return;
    AttnArgs a = attn_args(Q, ldq, K, ldk, Vt, ldvt, C, heads, Nq, Nk, vt_bstride);
    if (f8) { a.f8_rq = f8; a.f8_rk = f8 + C; a.f8_rv = f8 + 2 * C; a.f8_hs = f8 + 3 * C; }
    a.O8 = O8; a.o_amax = amax;
    rc = dfh::attention_launch(a, s);
  }
  void layernorm(const bf16_t* x, const Vec& w, const Vec& b, bf16_t* y, int M, int C) {
    if (rc || dry) return;
    rc = dfh::layernorm_launch(x, v32(w), v32(b), y, M, C, 1e-5f, s);
  }
  void attention(const bf16_t* Q, int ldq, const bf16_t* K, int ldk, const bf16_t* Vt, int ldvt, bf16_t* O, int C,
                 int heads, int Nq, int Nk, long vt_bstride = 0) {
    if (rc || dry) return;
    AttnArgs a = attn_args(Q, ldq, K, ldk, Vt, ldvt, C, heads, Nq, Nk, vt_bstride);
    a.O = O;
    rc = dfh::attention_launch(a, s);
  }

  // ---- the two prologues run() and run_cache() share
  // all time_emb_proj rows of B sinusoid rows tsin: the MLP (SiLU folded into both epilogues: only silu(emb) is ever consumed), then
  // every resnet's projection in one GEMM (fp32 [B][temb_total])
  void temb_rows(const bf16_t* tsin, bf16_t* e1, bf16_t* e2, float* rows) {
    const int c0 = u->cfg.block_out_channels[0], temb = 4 * c0;
    linear(tsin, B, c0, u->te1, &u->te1b, ACT_SILU, nullptr, e1, temb);
    linear(e1, B, temb, u->te2, &u->te2b, ACT_SILU, nullptr, e2, temb);
    linear(e2, B, temb, u->tproj, &u->tprojb, ACT_NONE, nullptr, rows, u->temb_total, OUT_F32);
  }
  // the text states to bf16 (ehs16), then text K for every transformer layer in one GEMM ([B*T][x_total]) and V^T in another
  // ([B][x_total][Tp])
  void text_kv_all(const void* ehs, int ehs_bf16, bf16_t* ehs16, bf16_t* kx, bf16_t* vxt) {
    const int T = u->cfg.text_len, X = u->cfg.cross_attention_dim, Tp = (T + 7) & ~7;
    if (!dry && !rc) {
      if (ehs_bf16) (void)hipMemcpyAsync(ehs16, ehs, (size_t)B * T * X * 2, hipMemcpyDeviceToDevice, s);
      else rc = dfh::cast_f32_to_bf16_launch((const float*)ehs, ehs16, (long)B * T * X, s);
    }
    linear(ehs16, B * T, X, u->kx_all, nullptr, ACT_NONE, nullptr, kx, u->x_total);
    linear(ehs16, B * T, X, u->vx_all, nullptr, ACT_NONE, nullptr, vxt, u->x_total, OUT_BF16_T, Tp, T);
  }

  // 3x3 conv (pad 1) as implicit GEMM; optional stride-2 / fused nearest-2x upsample
  Tensor conv(const Tensor& x, const ConvL& c, int stride, int ups, bool to_persist) {
    const int Ho = ups ? x.H * 2 : (stride == 2 ? x.H / 2 : x.H);
    const int Wo = ups ? x.W * 2 : (stride == 2 ? x.W / 2 : x.W);
    Tensor o = to_persist ? palloc(Ho, Wo, c.cout) : talloc(Ho, Wo, c.cout);
    // nearest-2x upsample + conv: four 2x2 convs over the source image with the summed taps (4/9 of the multiply-adds), one launch
    // over the four phase planes.  DFH_UPS_PHASE=0 keeps the 3x3 conv over the virtual upsampled image (A/B).
    if (ups == 1 && c.has_ph && u->fold_valid && kn.ups_phase && !dry && x.C == c.cin) {
      GemmArgs g = base(B * x.H * x.W, c.cout);
      g.conv_src = x.p; g.conv_c = x.C; g.ntaps = 4; g.phase2x = 1; g.nbatch = 4; g.w_bs = (long)c.cout * 4 * x.C;
      g.Hin = x.H; g.Win = x.W; g.Hout = x.H; g.Wout = x.W; g.stride = 1; g.rows_per_b = x.H * x.W;
      g.W = u->fold_w() + c.ph; g.ldw = 4 * x.C; g.bias = v32(c.b);
      g.out = o.p;
      gemm(g);
      return o;
    }
    GemmArgs g = conv_desc(x.p, x.C, x.H, x.W, Ho, Wo, stride, ups, c.w, c.b);
    g.out = o.p;
    gemm(g, &o, to_persist ? &persist : &temp);
    return o;
  }

  // Winograd F(2x2, 3x3) conv in three stages (winograd.hip); the scratch (V, M) is planned by the dry run too.
  //   wino_in   : V = B^T d B of the conv's input.  nw / nb: the GroupNorm(+SiLU) in front of the conv runs inside the transform (x, x1 = its
  //               raw, possibly concatenated input); Mprev: that input is the output transform of the PREVIOUS conv's planes (+ pbias + temb row),
  //               rebuilt inside the kernel (conv1 -> conv2 of a resnet); neither: x is the already normalised tensor
  //   wino_gemm : ONE batched GEMM over the sixteen transform-domain planes
  //   wino_out  : A^T m A + bias (+ time-embedding row) (+ residual)
  bf16_t* wino_in(const Tensor& x, const Tensor* x1, const Vec* nw, const Vec* nb, const bf16_t* Mprev = nullptr, const Vec* pbias = nullptr,
                  const float* prowvec = nullptr, int prv_off = 0) {
    const int C = x.C + (x1 ? x1->C : 0);
    const long mt = (long)B * (x.H / 2) * (x.W / 2);
    bf16_t* V = (bf16_t*)temp.alloc((size_t)16 * mt * C * 2);
    if (rc || dry) return V;
    if (nw) rc = dfh::gn_wino_input_launch(x.p, x.C, x1 ? x1->p : nullptr, x1 ? x1->C : 0, v32(*nw), v32(*nb), u->cfg.norm_eps,
                                           u->cfg.norm_num_groups, V, B, x.H, x.W, s, Mprev, pbias ? v32(*pbias) : nullptr, prowvec, temb_ld, prv_off);
    else rc = dfh::wino_input_launch(x.p, V, B, x.H, x.W, C, s);
    return V;
  }
  bf16_t* wino_gemm(const bf16_t* V, int H, int W, int C, size_t uoff, int cout) {
    const long mt = (long)B * (H / 2) * (W / 2);
    bf16_t* Mb = (bf16_t*)temp.alloc((size_t)16 * mt * cout * 2);
    if (rc || dry) return Mb;
    GemmArgs g = base((int)mt, cout);
    g.p_src[0] = V; g.p_c[0] = C; g.nplain = 1; g.W = u->fold_w() + uoff; g.ldw = C;
    g.nbatch = 16; g.a_bs = mt * C; g.w_bs = (long)cout * C; g.o_bs = mt * cout; g.w_blocked = dfh::wino_blocked(cout, C);
    g.out = Mb; g.zero = zero;
    g.prof_flops = 2.0 * B * H * W * (double)cout * 9.0 * C;
    rc = dfh::gemm_launch(g, s, dfh::wino_gemm_tile(g), 0, -1);
    dfh::census(dfh::CK_CONV_WINO);
    return Mb;
  }
  void wino_out(const bf16_t* Mb, const Vec& bias, const float* rowvec, int rv_off, const bf16_t* resid, Tensor& o) {
    if (rc || dry) return;
    rc = dfh::wino_output_launch(Mb, o.p, v32(bias), rowvec, temb_ld, rv_off, resid, B, o.H, o.W, o.C, s);
  }

  Tensor resnet(const Tensor& x0, const Tensor* x1, const ResL& r, const float* temb_all) {
    const int H = x0.H, W = x0.W;
    Tensor out = palloc(H, W, r.cout);
    const size_t mark = temp.off;
    Tensor g1 = talloc(H, W, r.cin);
    Tensor h1 = talloc(H, W, r.cout);
    // DFH_WINO: 0 = direct implicit GEMM everywhere, 1 = Winograd at H * W <= 64 (the 8x8 level), 2 = also at H * W <= 256 (A/B)
    const bool wino = r.has_u && (dry || u->fold_valid) && ((kn.wino >= 1 && H * W <= 64) || (kn.wino >= 2 && H * W <= kn.wino_maxhw));
    if (wino) {
      // the GroupNorms in front of the two convs run inside the input transforms where the (image, group) slab fits the kernel
      // (DFH_WINO_GN=0: separate GroupNorm launches, A/B)
      const int G = u->cfg.norm_num_groups;
      // conv1 -> conv2: the tensor between them (conv1's output, GroupNorm 2's input) is rebuilt from conv1's transform-domain planes
      // inside conv2's input transform -- no output-transform launch, no round trip (DFH_WINO_CHAIN=0: materialise it, A/B)
      const bf16_t* V1;
      if (kn.wino_gn && dfh::gn_wino_ok(x0.C, x1 ? x1->C : 0, G, H, W)) V1 = wino_in(x0, x1, &r.n1w, &r.n1b);
      else {
        groupnorm(x0, x1, r.n1w, r.n1b, u->cfg.norm_eps, 1, g1);
        V1 = wino_in(g1, nullptr, nullptr, nullptr);
      }
      const bf16_t* M1 = wino_gemm(V1, H, W, r.cin, r.u1, r.cout);
      const bool gn2 = kn.wino_gn && dfh::gn_wino_ok(r.cout, 0, G, H, W);
      const bool chain = gn2 && kn.wino_chain;
      Tensor g2 = talloc(H, W, r.cout);
      const bf16_t* V2;
      if (chain) V2 = wino_in(h1, nullptr, &r.n2w, &r.n2b, M1, &r.b1, temb_all, r.temb_off);     // h1 only names the shape: it is never written
      else {
        wino_out(M1, r.b1, temb_all, r.temb_off, nullptr, h1);
        if (gn2) V2 = wino_in(h1, nullptr, &r.n2w, &r.n2b);
        else {
          groupnorm(h1, nullptr, r.n2w, r.n2b, u->cfg.norm_eps, 1, g2);
          V2 = wino_in(g2, nullptr, nullptr, nullptr);
        }
      }
      const bf16_t* resid = x0.p;
      if (r.shortcut) {      // the 1x1 shortcut over the (possibly concatenated) block input: its own GEMM, added by the output transform
        Tensor sc = talloc(H, W, r.cout);
        GemmArgs g = conv2_desc(nullptr, H, W, r.cout, r.w2, r.b2, true, x0.p, x0.C, x1 ? x1->p : nullptr, x1 ? x1->C : 0);
        g.out = sc.p;
        gemm(g);
        resid = sc.p;
      }
      const bf16_t* M2 = wino_gemm(V2, H, W, r.cout, r.u2, r.cout);
      wino_out(M2, r.b2, nullptr, 0, resid, out);
      temp.off = mark;
      return out;
    }
    groupnorm(x0, x1, r.n1w, r.n1b, u->cfg.norm_eps, 1, g1);
    {
      GemmArgs g = conv_desc(g1.p, r.cin, H, W, H, W, 1, 0, r.w1, r.b1);
      g.rowvec = temb_all; g.rv_ld = temb_ld; g.rv_off = r.temb_off; g.rows_per_b = H * W;
      g.out = h1.p;
      gemm(g, &h1, &temp);
    }
    Tensor g2 = talloc(H, W, r.cout);
    groupnorm(h1, nullptr, r.n2w, r.n2b, u->cfg.norm_eps, 1, g2);
    {
      GemmArgs g = conv2_desc(g2.p, H, W, r.cout, r.w2, r.b2, r.shortcut, x0.p, x0.C, x1 ? x1->p : nullptr, x1 ? x1->C : 0);
      g.out = out.p;
      gemm(g, &out, &persist);
    }
    temp.off = mark;
    return out;
  }

  // ---- transformer block.  Its two forms -- transformer(): bf16 and the round-2 fp8 set; transformer_fp8(): every linear in e4m3 -- share
  // the entry allocations, the shared-prefix bookkeeping, the attention scratch and the addressing of the text K / V^T: the helpers below.
  //
  // pre_n > 0 (first transformer block of a guidance batch, dfh_unet::dup_tail): the last pre_n images have the same INPUT as the pre_n
  // before them and differ only in their text states, so everything up to the self-attention output is computed for B - pre_n images
  // and the repeated images' rows are copied; from the self-attention output projection on the block runs on the whole batch.
  struct Block {
    int C, N, Np, pre_n; bool pre;          // pre: inside the shared prefix (B is the call's batch less pre_n until prefix_end)
    size_t mark; Tensor out, h0, n1, qk, at, h1, h2;
    float* st;                              // row statistics of a folded LayerNorm's input: [C / bn][M][2], bn >= 64
    uint8_t* n8; float* s8; bf16_t* vt;     // a LayerNorm's output as e4m3 + token scales (fp8 only); V^T [B][C][Np]
  };
  Block block_enter(const Tensor& x, int C, int pre_n) {
    Block b{}; b.C = C; b.N = x.H * x.W; b.pre_n = pre_n;
    b.out = palloc(x.H, x.W, C);
    b.mark = temp.off;
    b.pre = pre_n > 0 && !dry && 2 * pre_n <= B;
    if (b.pre) B -= pre_n;
    b.st = (float*)temp.alloc((size_t)Ba * b.N * ((C + 63) / 64) * 2 * sizeof(float));
    b.h0 = talloc(x.H, x.W, C);
    return b;
  }
  void block_scratch(Block& b, bool f8) {   // what the block needs from the self-attention on
    const int H = b.out.H, W = b.out.W, C = b.C;
    b.n1 = talloc(H, W, C);
    b.n8 = f8 ? (uint8_t*)temp.alloc((size_t)Ba * b.N * C) : nullptr;
    b.s8 = f8 ? (float*)temp.alloc((size_t)Ba * b.N * sizeof(float)) : nullptr;
    b.qk = talloc(H, W, 2 * C);
    b.Np = (b.N + 7) & ~7;                  // V^T rows padded to 8 keys (the 2x2 level of tiny configs has N = 4)
    b.vt = (bf16_t*)temp.alloc((size_t)Ba * C * b.Np * 2);
    b.at = talloc(H, W, C); b.h1 = talloc(H, W, C); b.h2 = talloc(H, W, C);
  }
  void prefix_end(Block& b) {               // the whole batch from here on; the caller copies what else it made for the prefix
    B += b.pre_n;
    dup_images(b.h0, b.pre_n);
    dfh::census(dfh::CK_DUP_PREFIX);
  }
  Tensor block_leave(const Block& b) { temp.off = b.mark; return b.out; }
  // text K / V^T of a layer live inside the batched projections computed once per forward
  struct TextKV { const bf16_t* k; int ldk; const bf16_t* vt; int ldvt; long vt_bs; };
  TextKV text_kv(const AttL& a, const bf16_t* kx, const bf16_t* vxt, int T) const {
    const int Tp = (T + 7) & ~7, XT = u->x_total;
    return {kx + a.x_off, XT, vxt + (size_t)a.x_off * Tp, Tp, (long)XT * Tp};
  }

  Tensor transformer(const Tensor& x, const AttL& a, const bf16_t* kx, const bf16_t* vxt, int T, int pre_n = 0) {
    if (use8(a.qk8) && a.pin8.on) return transformer_fp8(x, a, kx, vxt, T, pre_n);
    const int H = x.H, W = x.W, C = a.C, N = H * W;
    // LayerNorm folding (gemm.h, lnfold.hip): the GEMM that produces a LayerNorm's input leaves per-row statistics of its output, the
    // projections behind the LayerNorm run on the raw rows with gamma folded into their weights and fix the rows up in their
    // epilogue -- no layernorm_kernel launch, no normalised copy of the tensor.  Falls back to the LayerNorm kernel + plain weights
    // whenever the producer ran on a kernel that writes no statistics or a consumer would split K.  DFH_LN_FOLD=0 turns it off (A/B).
    const bool f8 = use8(a.qk8);                    // the round-2 fp8 set (DFH_FP8_EXT=0): LayerNorm -> e4m3 + token scales -> block-scaled MFMA GEMM
    const bool fold = u->fold_valid && kn.ln_fold && !f8 && !dry;
    Block b = block_enter(x, C, pre_n);
    Tensor &out = b.out, &h0 = b.h0;
    float* const st = b.st;
    int M = B * N, bn = 0;
    auto try_folded = [&](std::initializer_list<GemmArgs> gs) {
      if (!fold || bn <= 0 || C % bn) return false;
      for (const GemmArgs& g : gs) if (!dfh::gemm_ln_consumer_ok(g)) return false;
      for (const GemmArgs& g : gs) gemm(g);
      dfh::census(dfh::CK_LN_FOLDED);
      return true;
    };
    // PROBE builds only (DFH_TOKEN_LINEAR=1 with the probe library): the K = N = C projections on the register-resident token-linear kernel
    // (scripts/probes/kernels/token_linear.hip).  Parity-tested, measured slower than the tile GEMM here -- 37 / 46 us against 27 / 34 us per
    // launch at M = 65536, sampling step 15.7 -> 15.9 ms (profiles/r05/token_linear_ab.txt): one workgroup per CU leaves its prologue (row
    // loads, first weight slice) and epilogue exposed twice per launch, and every 128-token tile re-streams the whole 200-KB matrix
#ifdef DFH_PROBES
    const bool tl = fold && kn.token_linear && a.has_tl && dfh::token_linear_eligible(C, C, M);
    auto token_linear = [&](const bf16_t* xin, size_t img, const float* bias, const bf16_t* resid, const Fold* f, bf16_t* o, bool stats) {
      if (rc) return;
      TokLinArgs t; std::memset(&t, 0, sizeof(t));
      t.x = xin; t.img = (const unsigned char*)(u->fold_w() + img); t.bias = bias; t.resid = resid; t.out = o; t.M = M;
      if (f) { t.ln_stat = st; t.ln_parts = C / bn; t.ln_cnt = bn; t.ln_eps = 1e-5f; t.ln_s = u->fold_v() + f->s; t.bias = u->fold_v() + f->b; }
      if (stats) t.rowstat = st;
      rc = dfh::token_linear_launch(t, s);
      if (stats) bn = C;                            // one record per row over all C columns
    };
#else
    constexpr bool tl = false;
    auto token_linear = [](const bf16_t*, size_t, const float*, const bf16_t*, const Fold*, bf16_t*, bool) {};
#endif
    // GroupNorm FOLDED into proj_in (norm.h GnFoldArgs): per-image weights W . gamma . rstd and a per-image row vector for the mean /
    // beta terms, so proj_in reads the block input itself and the normalised copy (one read + one write of the tensor) is never made.
    // Pays while the per-image weights (B x C x C) are small against the tensor: C <= DFH_GN_FOLD (default 320: the five 64x64-level
    // blocks; 0 = off).  Same box, sampling step: off 15.97 / 15.93, 320: 15.83 / 15.78, 640: 15.86 / 15.90, 1280: 16.01 / 16.00 ms
    // (profiles/r05/gn_fold_ab.txt).  The images must be whole 128-row tiles.
    const bool gfold = !tl && C <= kn.gn_fold && N % 128 == 0 && a.pin.K == C && a.pin.N == C;
    if (gfold) {
      bf16_t* wimg = (bf16_t*)temp.alloc((size_t)Ba * C * C * 2);
      float* rv = (float*)temp.alloc((size_t)Ba * C * sizeof(float));
      if (!rc && !dry) {
        GnFoldArgs f; std::memset(&f, 0, sizeof(f));
        f.x = x.p; f.B = B; f.HW = N; f.C = C; f.G = u->cfg.norm_num_groups; f.eps = 1e-6f; f.gamma = v32(a.nw); f.beta = v32(a.nb);
        if (x.gst && x.gst_cpg == C / f.G) { f.pre = x.gst; f.pre_chunks = x.gst_chunks; }
        f.partial = gn_partial; f.W = w16(a.pin); f.ldw = a.pin.K; f.N = C; f.bias = v32(a.pinb); f.Wimg = wimg; f.rv = rv;
        rc = dfh::groupnorm_fold_launch(f, s);
      }
      GemmArgs g = base(M, C);
      g.p_src[0] = x.p; g.p_c[0] = C; g.nplain = 1;
      g.W = wimg; g.ldw = C; g.w_img_bs = (long)C * C;
      g.rowvec = rv; g.rv_ld = C; g.rv_off = 0; g.rows_per_b = N;
      g.out = h0.p; g.rowstat = fold ? st : nullptr;
      gemm(g, nullptr, nullptr, &bn);
    } else {
      Tensor gn = talloc(H, W, C);
      groupnorm(x, nullptr, a.nw, a.nb, 1e-6f, 0, gn);
      if (tl) token_linear(gn.p, a.tl_pin, v32(a.pinb), nullptr, nullptr, h0.p, true);
      else linear(gn.p, M, C, a.pin, &a.pinb, ACT_NONE, nullptr, h0.p, C, OUT_BF16, -1, 0, nullptr, nullptr, fold ? st : nullptr, &bn);
    }
    // --- self attention
    block_scratch(b, f8);
    Tensor &n1 = b.n1, &qk = b.qk, &at = b.at, &h1 = b.h1, &h2 = b.h2;
    uint8_t* const n8 = b.n8; float* const s8 = b.s8; bf16_t* const vt = b.vt; const int Np = b.Np;
    // q | k and V^T from ONE launch (columns 2C .. 3C leave transposed into vt: GemmArgs::out2) wherever the column tile divides 2C;
    // DFH_QKV_MERGE=0 keeps the two launches (A/B)
    auto with_v = [&](GemmArgs g) {               // q | k launch -> q | k | v: same rows, N = 3C, the v columns into vt
      g.N = 3 * C; g.out2 = vt; g.ld_out2 = Np; g.n_split = 2 * C; g.rows_per_b = N;
      return g;
    };
    const bool v_contig = a.v.off == a.qk.off + (size_t)2 * C * C && a.v.K == a.qk.K;   // packed back to back (build_attn)
    bool done = false;
    if (!f8 && kn.qkv_merge && !dry) {
      GemmArgs gq = with_v(folded(h0.p, M, a.fqk, st, bn, ACT_NONE, qk.p, OUT_BF16, 2 * C, 0));
      if (dfh::gemm_out2_ok(gq)) done = try_folded({gq});
    }
    if (!done) done = try_folded({folded(h0.p, M, a.fqk, st, bn, ACT_NONE, qk.p, OUT_BF16, -1, 0),
                                  folded(h0.p, M, a.fv, st, bn, ACT_NONE, vt, OUT_BF16_T, Np, N)});
    if (!done) {
      if (f8) layernorm8(h0.p, a.l1w, a.l1b, n8, s8, M, C);
      else layernorm(h0.p, a.l1w, a.l1b, n1.p, M, C);
      bool merged = false;
      if (!f8 && kn.qkv_merge && !dry && v_contig) {
        GemmArgs g = base(M, 2 * C);
        g.p_src[0] = n1.p; g.p_c[0] = C; g.nplain = 1; g.W = w16(a.qk); g.ldw = C; g.out = qk.p; g.ld_out = 2 * C;
        g = with_v(g);
        if (dfh::gemm_out2_ok(g)) { gemm(g); merged = true; }
      }
      if (!merged) {
        if (f8) linear8(n8, s8, M, a.qk8, nullptr, ACT_NONE, qk.p);
        else linear(n1.p, M, C, a.qk, nullptr, ACT_NONE, nullptr, qk.p, 2 * C);
        if (f8) linear8(n8, s8, M, a.v8, nullptr, ACT_NONE, vt, OUT_BF16_T, Np, N);
        else linear(n1.p, M, C, a.v, nullptr, ACT_NONE, nullptr, vt, C, OUT_BF16_T, Np, N);
      }
    }
    attention(qk.p, 2 * C, qk.p + C, 2 * C, vt, Np, at.p, C, a.heads, N, N);
    if (b.pre) {                                     // end of the shared prefix: the whole batch from here on
      prefix_end(b); dup_images(at, pre_n);
      M = B * N;
    }
    if (tl) token_linear(at.p, a.tl_o1, v32(a.o1b), h0.p, nullptr, h1.p, true);
    else linear(at.p, M, C, a.o1, &a.o1b, ACT_NONE, h0.p, h1.p, C, OUT_BF16, -1, 0, nullptr, nullptr, fold ? st : nullptr, &bn);
    // --- cross attention over the T text tokens
    if (tl && bn > 0 && C % bn == 0) {
      token_linear(h1.p, a.tl_q2, nullptr, nullptr, &a.fq2, qk.p, false);
      dfh::census(dfh::CK_LN_FOLDED);
    } else if (!try_folded({folded(h1.p, M, a.fq2, st, bn, ACT_NONE, qk.p, OUT_BF16, -1, 0)})) {
      if (f8) { layernorm8(h1.p, a.l2w, a.l2b, n8, s8, M, C); linear8(n8, s8, M, a.q28, nullptr, ACT_NONE, qk.p); }
      else {
        layernorm(h1.p, a.l2w, a.l2b, n1.p, M, C);
        linear(n1.p, M, C, a.q2, nullptr, ACT_NONE, nullptr, qk.p, C);
      }
    }
    const TextKV t = text_kv(a, kx, vxt, T);
    attention(qk.p, C, t.k, t.ldk, t.vt, t.ldvt, at.p, C, a.heads, N, T, t.vt_bs);
    if (tl) token_linear(at.p, a.tl_o2, v32(a.o2b), h1.p, nullptr, h2.p, true);
    else linear(at.p, M, C, a.o2, &a.o2b, ACT_NONE, h1.p, h2.p, C, OUT_BF16, -1, 0, nullptr, nullptr, fold ? st : nullptr, &bn);
    // --- GEGLU feed-forward
    // statistics of the block's output for the next GroupNorm, written by the fused kernel's epilogue in 128-token chunks (allocated in the
    // dry run as well: the unfused path plans 256-token chunks through gemm())
    const int G = u->cfg.norm_num_groups;
    const bool mlp_gst_ok = a.has_mlp && N % 128 == 0 && C % G == 0 && N / 128 <= (int)GN_MAX_CHUNKS;
    float* mlp_gst = mlp_gst_ok ? (float*)persist.alloc((size_t)B * G * (N / 128) * 2 * sizeof(float)) : nullptr;
    Tensor ff = talloc(H, W, 4 * C);
    // the whole feed-forward + proj_out in one kernel where the X tile fits the register file (C = 320: the 64x64 level); needs the row
    // statistics of h2 from its producer like every folded-LayerNorm consumer.  DFH_MLP_FUSED=0: the two-launch walk, 1 / 2: the two forms of the kernel (A/B)
    const bool mlp_off = dfh::mlp_fused_form() == 0;
    if (fold && !mlp_off && a.has_mlp && bn > 0 && C % bn == 0 && dfh::mlp_fused_eligible(C, M)) {
      MlpArgs ma; std::memset(&ma, 0, sizeof(ma));
      ma.x = h2.p; ma.resid = x.p; ma.img = (const unsigned char*)(u->fold_w() + a.mlp_img);
      ma.ln_stat = st; ma.ln_parts = C / bn; ma.ln_cnt = bn; ma.ln_eps = 1e-5f;
      ma.bias = u->fold_v() + a.fffp.b; ma.out = out.p; ma.M = M;
      if (dfh::mlp_fused_form() == 2 && mlp_gst && kn.gn_pre) {
        ma.gstat = mlp_gst; ma.gstat_cpg = C / G; ma.gstat_hw = N;
        out.gst = mlp_gst; out.gst_cpg = C / G; out.gst_chunks = N / 128;
        dfh::census(dfh::CK_GSTAT_WRITTEN);
      }
#ifdef DFH_PROBES
      if (!rc && dfh::mlp_fused_form() == 1) rc = dfh::mlp_fused_launch(ma, s); else
#endif
      if (!rc) rc = dfh::mlp2_fused_launch(ma, s);
      dfh::census(dfh::CK_LN_FOLDED);                  // LayerNorm 3 is consumed folded here too
      return block_leave(b);
    }
    if (!try_folded({folded(h2.p, M, a.fff1, st, bn, ACT_GEGLU, ff.p, OUT_BF16, -1, 0)})) {
      if (f8) { layernorm8(h2.p, a.l3w, a.l3b, n8, s8, M, C); linear8(n8, s8, M, a.ff18, &a.ff1b, ACT_GEGLU, ff.p); }
      else {
        layernorm(h2.p, a.l3w, a.l3b, n1.p, M, C);
        linear(n1.p, M, C, a.ff1, &a.ff1b, ACT_GEGLU, nullptr, ff.p, 8 * C);
      }
    }
    // ff.net.2 and proj_out as ONE linear over the two K segments [GEGLU output | h2] (AttL::fffp) + the block's residual
    GemmArgs gf = base(M, C);
    gf.p_src[0] = ff.p; gf.p_c[0] = 4 * C; gf.p_src[1] = h2.p; gf.p_c[1] = C; gf.nplain = 2;
    gf.ldw = 5 * C; gf.resid = x.p; gf.ld_res = C; gf.out = out.p;
    if (dry) gemm(gf);                                                   // planning: its split-K slabs, whichever path runs later
    if (u->fold_valid && kn.ffp_fold && !dry) {      // DFH_FFP_FOLD=0: the two linears (A/B)
      gf.W = u->fold_w() + a.fffp.w; gf.bias = u->fold_v() + a.fffp.b;
      gemm(gf, &out, &persist);                                          // feeds the next block's GroupNorm
    } else {
      linear(ff.p, M, 4 * C, a.ff2, &a.ff2b, ACT_NONE, h2.p, h0.p, C);   // h0 is dead by now: reuse
      linear(h0.p, M, C, a.pout, &a.poutb, ACT_NONE, x.p, out.p, C, OUT_BF16, -1, 0, &out, &persist);   // feeds the next block's GroupNorm
    }
    return block_leave(b);
  }

  // The all-e4m3 block (round 4: proj_in, both to_out, ff.net.2 and proj_out in e4m3 as well as the LayerNorm-fed projections), every
  // operand quantised by the kernel that produces it.  One straight line: none of the bf16 block's choices exists here.
  Tensor transformer_fp8(const Tensor& x, const AttL& a, const bf16_t* kx, const bf16_t* vxt, int T, int pre_n) {
    const int C = a.C, N = x.H * x.W;
    Block b = block_enter(x, C, pre_n);
    uint8_t* a8 = (uint8_t*)temp.alloc((size_t)Ba * N * C);          // e4m3 operand of proj_in, then of the two to_out
    block_scratch(b, true);       // b.st, b.n1 and b.at are never touched here: they keep the workspace plan of an fp8 context what it was
    float* am_self = amax_self + (size_t)a.idx * Ba;
    const float* am_cross = amax_cross + (size_t)a.idx * Ba;
    int M = B * N;
    groupnorm8(x, 1e-6f, a8);
    Fp8GemmArgs g = args8(a8, M, a.pin8, nullptr, b.h0.p);
    g.bias = (const float*)(u->arena8 + a.pin8.boff); g.sa_mul = dfh_unet::GN_Z / 448.0f;
    gemm8(g);
    // --- self attention: q | k and V^T (with the largest |V| per image), products on the e4m3 MFMA where the layer has operand factors
    // and the keys make whole 64-key tiles
    layernorm8(b.h0.p, a.l1w, a.l1b, b.n8, b.s8, M, C);
    linear8(b.n8, b.s8, M, a.qk8, nullptr, ACT_NONE, b.qk.p);
    linear8(b.n8, b.s8, M, a.v8, nullptr, ACT_NONE, b.vt, OUT_BF16_T, b.Np, N, am_self);
    const float* f8attn = (a.f8a && N % 64 == 0) ? (const float*)(u->arena8 + a.f8a_off) : nullptr;
    attention8(b.qk.p, 2 * C, b.qk.p + C, 2 * C, b.vt, b.Np, a8, am_self, C, a.heads, N, N, 0, f8attn);
    if (b.pre) {                                     // end of the shared prefix: rows, e4m3 attention output and its per-image max
      prefix_end(b); dup_bytes(a8, (size_t)N * C, pre_n); dup_bytes(am_self, sizeof(float), pre_n);
      M = B * N;
    }
    g = args8(a8, M, a.o18, &a.o1b, b.h1.p);
    g.sA = am_self; g.sa_div = N; g.sa_mul = 1.0f / 448.0f; g.resid = b.h0.p; g.ld_res = C;
    gemm8(g);
    // --- cross attention over the T text tokens
    layernorm8(b.h1.p, a.l2w, a.l2b, b.n8, b.s8, M, C);
    linear8(b.n8, b.s8, M, a.q28, nullptr, ACT_NONE, b.qk.p);
    const TextKV t = text_kv(a, kx, vxt, T);
    attention8(b.qk.p, C, t.k, t.ldk, t.vt, t.ldvt, a8, am_cross, C, a.heads, N, T, t.vt_bs);
    g = args8(a8, M, a.o28, &a.o2b, b.h2.p);
    g.sA = am_cross; g.sa_div = N; g.sa_mul = 1.0f / 448.0f; g.resid = b.h1.p; g.ld_res = C;
    gemm8(g);
    // --- GEGLU feed-forward: the hidden tensor in e4m3 with one E8M0 scale per token and 32 hidden units, written by the GEGLU epilogue
    // and consumed by ff.net.2 through the MFMA's scale operand; ff.net.2's output (+ bias + h2) likewise, consumed by proj_out (+ the
    // block's residual)
    uint8_t* ff8 = (uint8_t*)temp.alloc((size_t)M * 4 * C);
    uint8_t* ffsx = (uint8_t*)temp.alloc((size_t)(4 * C / 32) * M + 256);
    uint8_t* t8 = (uint8_t*)temp.alloc((size_t)M * C);
    uint8_t* tsx = (uint8_t*)temp.alloc((size_t)(C / 32) * M + 256);
    layernorm8(b.h2.p, a.l3w, a.l3b, b.n8, b.s8, M, C);
    g = args8(b.n8, M, a.ff18, &a.ff1b, ff8);
    g.sA = b.s8; g.act = ACT_GEGLU; g.out_mode = OUT_FP8_MX; g.ld_out = 4 * C; g.out_sx = ffsx;
    gemm8(g);
    g = args8(ff8, M, a.ff28, &a.ff2b, t8);
    g.sx = ffsx; g.resid = b.h2.p; g.ld_res = C; g.out_mode = OUT_FP8_MX; g.ld_out = C; g.out_sx = tsx;
    gemm8(g);
    g = args8(t8, M, a.pout8, &a.poutb, b.out.p);
    g.sx = tsx; g.resid = x.p; g.ld_res = C;
    gemm8(g);
    return block_leave(b);
  }
};

// amax_cross[layer][b] = max |V^T| of the layer's slice of the batched text V^T
int dfh_unet::cross_amax(const bf16_t* vxt, int B, float* out, hipStream_t s) {
  const int Tp = (cfg.text_len + 7) & ~7;
  // the pad columns T .. Tp - 1 of V^T are never written: only the T real keys count
  return dfh::amax_slabs_launch(vxt, (long)x_total * Tp, Tp, cfg.text_len, slab_row0(), slab_rows(), out, n_att, B, s);
}


int dfh_unet::run(const void* sample, int sample_bf16, const float* timestep, const void* ehs, int ehs_bf16, float* out, int B,
                  hipStream_t s, bool dry, const RunCache* rcache) {
  if (!dry && B != plan.batch) run(nullptr, 0, nullptr, nullptr, 0, nullptr, B, nullptr, true);      // plan this batch first; bind() checks it fits
  Run r(this, B, s, dry);
  r.temb_ld = (rcache && rcache->temb_row) ? 0 : temb_total;
  // one-shot hint of the caller (dfh_unet_set_dup_tail): the last `dup` images repeat the sample / timestep of the `dup` before them
  const int dup = (!dry && dup_tail > 0 && 2 * dup_tail <= B) ? dup_tail : 0;
  if (!dry) dup_tail = 0;
  const int S = cfg.sample_size, T = cfg.text_len, X = cfg.cross_attention_dim;
  const int* boc = cfg.block_out_channels;
  const int nb = cfg.num_blocks, temb = boc[0] * 4;
  // the fold region comes first (fold_layernorms), the walk's own workspace behind it
  if (!dry && !r.bind(ws + fold_bytes(), walk_bytes(), plan)) return r.rc;
  if (!dry && fold_dirty) { if (int rc = fold_layernorms(s)) return rc; }      // derived weights (LayerNorm / ff2 . proj_out folds): lazily
  taps.clear();

  // ---- time embedding: sinusoid -> MLP (SiLU folded into both epilogues: only silu(emb) is ever
  //      consumed) -> all 22 time_emb_proj rows in one GEMM (fp32 [B][temb_total])
  bf16_t* tsin = (bf16_t*)r.persist.alloc((size_t)B * boc[0] * 2);
  bf16_t* e1 = (bf16_t*)r.persist.alloc((size_t)B * temb * 2);
  bf16_t* e2 = (bf16_t*)r.persist.alloc((size_t)B * temb * 2);
  float* temb_all = (float*)r.persist.alloc((size_t)B * temb_total * 4);
  const bool t_cached = rcache && rcache->temb_row, x_cached = rcache && rcache->kx && rcache->vxt;
  if (!dry && !t_cached) r.rc = dfh::timestep_embed_launch(timestep, tsin, B, boc[0], s);
  if (dry || !t_cached) r.temb_rows(tsin, e1, e2, temb_all);      // the dry run plans for the uncached walk (same workspace either way)
  else temb_all = const_cast<float*>(rcache->temb_row);

  // ---- inputs to kernel layout
  const int Tp = (T + 7) & ~7;
  bf16_t* ehs16 = (bf16_t*)r.persist.alloc((size_t)B * T * X * 2);
  bf16_t* kx = (bf16_t*)r.persist.alloc((size_t)B * T * x_total * 2);
  bf16_t* vxt = (bf16_t*)r.persist.alloc((size_t)B * x_total * Tp * 2);
  if (dry || !x_cached) r.text_kv_all(ehs, ehs_bf16, ehs16, kx, vxt);
  else {
    kx = const_cast<bf16_t*>(rcache->kx); vxt = const_cast<bf16_t*>(rcache->vxt);
    dfh::census(dfh::CK_TEXT_CACHED);
  }
  if (fp8) {
    r.amax_self = (float*)r.persist.alloc((size_t)n_att * B * 4);
    float* xam = (float*)r.persist.alloc((size_t)n_att * B * 4);
    r.amax_cross = xam;
    if (!dry && !r.rc) {
      if (hipMemsetAsync(r.amax_self, 0, (size_t)n_att * B * 4, s) != hipSuccess) { dfh::set_error("hipMemsetAsync failed"); return -2; }
      if (x_cached && rcache->xamax) r.amax_cross = rcache->xamax;
      else r.rc = cross_amax(vxt, B, xam, s);
    }
  }
  Tensor x = r.palloc(S, S, conv_in.cin);   // in_channels padded to a multiple of 8
  if (!dry && !r.rc) r.rc = dfh::nchw_to_nhwc_launch(sample, sample_bf16, x.p, B, cfg.in_channels, S * S, s);
  if (dup && !r.rc) {
    // DFH_CHECK_DUP=1 (debugging a caller): verify what the hint claims -- the repeated images' inputs equal the ones they repeat --
    // with a synchronous compare of the converted input rows; a wrong hint is an error, not a silently different result
    if (dfh::WalkKnobs::get().check_dup) {
      const size_t per = (size_t)S * S * conv_in.cin * 2, n = (size_t)dup * per;
      std::vector<char> a(n), b(n);
      if (hipStreamSynchronize(s) != hipSuccess || hipMemcpy(a.data(), (char*)x.p + (size_t)(B - 2 * dup) * per, n, hipMemcpyDeviceToHost) != hipSuccess ||
          hipMemcpy(b.data(), (char*)x.p + (size_t)(B - dup) * per, n, hipMemcpyDeviceToHost) != hipSuccess) { dfh::set_error("DFH_CHECK_DUP: copy failed"); return -2; }
      if (std::memcmp(a.data(), b.data(), n) != 0) { dfh::set_error("dfh_unet_set_dup_tail: the last images do NOT repeat the inputs of the ones before them"); return -1; }
      if (timestep && !(rcache && rcache->temb_row)) {
        std::vector<float> t(B);
        if (hipMemcpy(t.data(), timestep, (size_t)B * 4, hipMemcpyDeviceToHost) != hipSuccess) { dfh::set_error("DFH_CHECK_DUP: copy failed"); return -2; }
        for (int i = 0; i < dup; ++i)
          if (t[B - dup + i] != t[B - 2 * dup + i]) { dfh::set_error("dfh_unet_set_dup_tail: the repeated images sit at other timesteps"); return -1; }
      }
    }
  }

  // Shared prefix of a guidance batch (reference difashion.py:388-427, 494-512: the branches of classifier-free guidance that differ only
  // in their PROMPT get the same latent / mutual / history input): conv_in, the first resnet and the first transformer block up to its
  // self-attention see no text state, so they run once for the repeated images.
  if (dup) r.B = B - dup;
  Tensor h = r.conv(x, conv_in, 1, 0, true);
  taps["conv_in"] = h;
  std::vector<Tensor> skips{h};
  for (int i = 0; i < nb; ++i) {
    for (int j = 0; j < cfg.layers_per_block; ++j) {
      const bool first = dup && i == 0 && j == 0;
      h = r.resnet(h, nullptr, down_res[i][j], temb_all);
      if (first) {
        r.B = B;
        r.dup_images(skips[0], dup); taps["conv_in"] = skips[0];
        if (!cfg.down_attn[i]) r.dup_images(h, dup);
        else { const float* g = h.gst; r.dup_images(h, dup); h.gst = g; }     // the block's entry GroupNorm still runs on the prefix (transformer(): pre_n), which the producer statistics cover
      }
      if (cfg.down_attn[i]) h = r.transformer(h, down_att[i][j], kx, vxt, T, first ? dup : 0);
      skips.push_back(h);
    }
    if (i != nb - 1) { h = r.conv(h, down_samp[i], 2, 0, true); skips.push_back(h); }
    taps["down" + std::to_string(i)] = h;
  }
  h = r.resnet(h, nullptr, mid_res[0], temb_all);
  h = r.transformer(h, mid_att, kx, vxt, T);
  h = r.resnet(h, nullptr, mid_res[1], temb_all);
  taps["mid"] = h;
  for (int i = 0; i < nb; ++i) {
    for (int j = 0; j < (int)up_res[i].size(); ++j) {
      Tensor sk = skips.back(); skips.pop_back();
      h = r.resnet(h, &sk, up_res[i][j], temb_all);
      if (!up_att[i].empty()) h = r.transformer(h, up_att[i][j], kx, vxt, T);
    }
    if (i != nb - 1) h = r.conv(h, up_samp[i], 1, 1, true);
    taps["up" + std::to_string(i)] = h;
  }
  Tensor g = r.palloc(h.H, h.W, h.C);
  r.groupnorm(h, nullptr, cnw, cnb, cfg.norm_eps, 1, g);
  {
    GemmArgs ga = r.conv_desc(g.p, g.C, S, S, S, S, 1, 0, conv_out.w, conv_out.b);
    ga.out = out; ga.out_mode = OUT_F32_T; ga.ld_out = S * S; ga.rows_per_b = S * S;
    r.gemm(ga);
  }
  if (dry) { plan = r.plan(); taps.clear(); }
  else last_batch = B;
  return r.rc;
}

// Fills a run cache: see unet_model.h
int dfh_unet::run_cache(const void* ehs, int ehs_bf16, int B, const float* timesteps, int n_t, void* cache, hipStream_t s) {
  if (B != plan.batch) run(nullptr, 0, nullptr, nullptr, 0, nullptr, B, nullptr, true);
  Run r(this, B, s, false);
  // scratch: the front of the persist region, whose plan holds these five buffers and more
  if (!r.bind(ws + fold_bytes(), walk_bytes(), plan)) return r.rc;
  const int T = cfg.text_len, X = cfg.cross_attention_dim;
  const int temb = cfg.block_out_channels[0] * 4, c0 = cfg.block_out_channels[0];
  bf16_t* kx = (bf16_t*)cache;
  bf16_t* vxt = (bf16_t*)((char*)cache + cache_kx_bytes(*this, B));
  float* table = (float*)((char*)cache + cache_kx_bytes(*this, B) + cache_vxt_bytes(*this, B));
  float* xamax = (float*)((char*)table + (((size_t)n_t * temb_total * 4 + 255) & ~(size_t)255));
  bf16_t* ehs16 = (bf16_t*)r.persist.alloc((size_t)B * T * X * 2);
  r.text_kv_all(ehs, ehs_bf16, ehs16, kx, vxt);
  if (fp8 && !r.rc) r.rc = cross_amax(vxt, B, xamax, s);
  bf16_t* tsin = (bf16_t*)r.persist.alloc((size_t)B * c0 * 2);
  bf16_t* e1 = (bf16_t*)r.persist.alloc((size_t)B * temb * 2);
  bf16_t* e2 = (bf16_t*)r.persist.alloc((size_t)B * temb * 2);
  float* trow = (float*)r.persist.alloc((size_t)B * temb_total * 4);
  for (int t0 = 0; t0 < n_t && !r.rc; t0 += B) {
    // always B rows (the planned GEMM shapes); rows past n_t repeat the last timestep and are not copied out
    const int n = std::min(B, n_t - t0);
    r.rc = dfh::timestep_embed_launch(timesteps + t0, tsin, n, c0, s);
    if (r.rc) break;
    if (n < B) (void)hipMemsetAsync(tsin + (size_t)n * c0, 0, (size_t)(B - n) * c0 * 2, s);
    r.temb_rows(tsin, e1, e2, trow);
    if (!r.rc) (void)hipMemcpyAsync(table + (size_t)t0 * temb_total, trow, (size_t)n * temb_total * 4, hipMemcpyDeviceToDevice, s);
  }
  return r.rc;
}

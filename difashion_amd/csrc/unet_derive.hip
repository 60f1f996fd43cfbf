// Everything derived from the master weights: the packed arenas (pack, pack_train, pack_all), the e4m3 copies (quantize_fp8) and the
// folded / transformed copies at the head of the workspace (fold_layernorms).
#include "unet_model.h"

int dfh_unet::pack(const float* const* master, int count, hipStream_t s) {
  if (int rc = pack_params(master, count, s)) return rc;
  if (int rc = quantize_fp8(s)) return rc;   // e4m3 copies of the LayerNorm-fed projections from the freshly packed bf16 matrices
  fold_valid = false; fold_dirty = true;     // the folded copies are re-derived by the next INFERENCE walk (a training step never pays)
  return 0;
}

int dfh_unet::pack_train(const float* const* master, int count, hipStream_t s) {
  DFH_REQUIRE(count == (int)params.size(), "parameter count mismatch");
  DFH_REQUIRE(arena16t != nullptr, "training arenas not bound");
  tab_packt.clear();
  for (const TPackOp& op : tpacks) {
    void* src = (void*)master[op.param];
    DFH_REQUIRE(src != nullptr, "null master parameter: " + params[op.param].name);
    tab_packt.add(src, op);
  }
  return tab_packt.launch(nullptr, arena16t, s);
}

// pack() + pack_train() of a training step in one pass over the masters: every weight that has exactly one plain and one transposed pack
// goes through a PACK2 op (read once, written to arena16 AND arena16t); vectors, the few weights packed more than once and the
// accumulating biases keep their own ops.  Same bytes in both arenas as the two separate calls (tests/test_gpu_train.py).
int dfh_unet::pack_all(const float* const* master, int count, hipStream_t s) {
  DFH_REQUIRE(count == (int)params.size(), "parameter count mismatch");
  DFH_REQUIRE(arena16 && arena32 && arena16t, "arenas not bound");
  std::vector<int> n_plain(params.size(), 0), n_tr(params.size(), 0), tr_at(params.size(), -1);
  for (const PackOp& op : packs) if (op.kind != PK_VEC) ++n_plain[op.param];
  for (size_t i = 0; i < tpacks.size(); ++i) { ++n_tr[tpacks[i].param]; tr_at[tpacks[i].param] = (int)i; }
  tab_pack2.clear(); tab_pack_acc.clear(); tab_packt.clear();
  for (const PackOp& op : packs) {
    void* src = (void*)master[op.param];
    DFH_REQUIRE(src != nullptr, "null master parameter: " + params[op.param].name);
    if (op.kind == PK_VEC) { (op.accumulate ? tab_pack_acc : tab_pack2).add(src, op); continue; }
    const bool twin = n_plain[op.param] == 1 && n_tr[op.param] == 1;
    const TPackOp* t = twin ? &tpacks[tr_at[op.param]] : nullptr;
    if (t && t->N == op.N && t->K == op.K && (t->conv != 0) == (op.kind != PK_MAT) && t->geglu == op.geglu) {
      if (op.kind == PK_MAT)
        tab_pack2.add2(src, TAB_PACK2_MAT, (long)op.dst, op.N, op.K, op.ldw, op.row_off, op.col_off, op.geglu, 0, (long)t->dst, t->ldt, t->t_row_off, t->t_col_off, 0);
      else
        tab_pack2.add2(src, TAB_PACK2_CONV, (long)op.dst, op.N, op.K, op.ldw, 0, op.col_off, 0, op.cin_pad, (long)t->dst, t->ldt, 0, t->t_col_off, t->o_pad);
      n_tr[op.param] = -1;                      // its transposed pack is done
    } else {
      tab_pack2.add(src, op);
    }
  }
  for (const TPackOp& op : tpacks) {            // transposed packs without a twin
    if (n_tr[op.param] < 0) continue;
    void* src = (void*)master[op.param];
    tab_packt.add(src, op);
  }
  if (int rc = tab_pack2.launch(arena32, arena16, s, arena16t)) return rc;
  if (int rc = tab_pack_acc.launch(arena32, arena16, s)) return rc;
  if (int rc = tab_packt.launch(nullptr, arena16t, s)) return rc;
  if (int rc = quantize_fp8(s)) return rc;
  fold_valid = false; fold_dirty = true;
  return 0;
}

int dfh_unet::quantize_fp8(hipStream_t s) {
  if (!fp8 || !arena8) return 0;
  if (hipMemcpyAsync(arena8 + a8_slab_off, slab_host.data(), slab_host.size() * sizeof(int), hipMemcpyHostToDevice, s) != hipSuccess) {
    dfh::set_error("uploading the V^T slab table failed"); return -2;
  }
  for (AttL* a : atts) {
    const Mat* src[8] = {&a->qk, &a->v, &a->q2, &a->ff1, &a->o1, &a->o2, &a->ff2, &a->pout};
    const Mat8* dst[8] = {&a->qk8, &a->v8, &a->q28, &a->ff18, &a->o18, &a->o28, &a->ff28, &a->pout8};
    for (int i = 0; i < 8; ++i) {
      if (!dst[i]->on) continue;
      if (int rc = dfh::quant_rows_fp8_launch(arena16 + src[i]->off, src[i]->K, arena8 + dst[i]->off, (float*)(arena8 + dst[i]->soff),
                                              src[i]->N, src[i]->K, s)) return rc;
    }
    if (a->pin8.on) {
      // proj_in behind the GroupNorm whose kernel emits the un-affined normalised value: W' = W . diag(gamma) (bf16, in the activation
      // workspace, which no walk is using while weights are derived), b' = bias + W . beta, then the per-channel quantisation of W'
      const int C = a->C;
      DFH_REQUIRE(ws && fold_bytes() + (size_t)C * C * 2 + (size_t)C * 4 + 512 <= ws_bytes, "workspace too small for the fp8 proj_in fold");
      bf16_t* wf = (bf16_t*)(ws + fold_bytes());
      float* sv = (float*)(ws + fold_bytes() + (((size_t)C * C * 2 + 255) & ~(size_t)255));
      if (int rc = dfh::ln_fold_launch(arena16 + a->pin.off, a->pin.K, arena32 + a->nw.off, arena32 + a->nb.off, arena32 + a->pinb.off, wf, sv,
                                       (float*)(arena8 + a->pin8.boff), C, C, s)) return rc;
      if (int rc = dfh::quant_rows_fp8_launch(wf, C, arena8 + a->pin8.off, (float*)(arena8 + a->pin8.soff), C, C, s)) return rc;
    }
    if (a->f8a) {
      // operand factors of the fp8 attention: bounds of q, k, v behind LayerNorm 1 from W . diag(gamma) and W . beta (bf16 / fp32 scratch)
      const int C = a->C;
      DFH_REQUIRE(ws && fold_bytes() + (size_t)3 * C * C * 2 + (size_t)6 * C * 4 + 1024 <= ws_bytes, "workspace too small for the fp8 attention scales");
      bf16_t* wf = (bf16_t*)(ws + fold_bytes());
      float* sv = (float*)(ws + fold_bytes() + (((size_t)3 * C * C * 2 + 255) & ~(size_t)255));
      float* bv = sv + 3 * C;
      if (int rc = dfh::ln_fold_launch(arena16 + a->qk.off, C, arena32 + a->l1w.off, arena32 + a->l1b.off, nullptr, wf, sv, bv, 3 * C, C, s)) return rc;
      float* f = (float*)(arena8 + a->f8a_off);
      if (int rc = dfh::attn_scales_launch(wf, bv, C, a->heads, f, f + C, f + 2 * C, f + 3 * C, s)) return rc;
    }
  }
  return 0;
}

// W' / s / b' of every LayerNorm-fed projection from the freshly packed bf16 matrices (needs the workspace: after dfh_unet_bind)
int dfh_unet::fold_layernorms(hipStream_t s) {
  fold_valid = false;
  if (!ws || !arena16 || !arena32) return 0;
  // a transformer width the 16-byte kernels cannot take (C % 8 != 0) has no folded weights: the walk must not read its (unwritten)
  // fold slots, so the whole inference walk then stays on the unfolded path (fold_valid stays false)
  for (AttL* a : atts) if (a->C % 8) return 0;
  for (AttL* a : atts) {
    if (fp8 && a->qk8.on) continue;                 // the fp8 walk of this layer reads none of the folded bf16 copies: not derived
    const Mat* src[4] = {&a->qk, &a->v, &a->q2, &a->ff1};
    const Fold* dst[4] = {&a->fqk, &a->fv, &a->fq2, &a->fff1};
    const Vec* gam[4] = {&a->l1w, &a->l1w, &a->l2w, &a->l3w};
    const Vec* bet[4] = {&a->l1b, &a->l1b, &a->l2b, &a->l3b};
    for (int i = 0; i < 4; ++i) {
      const float* bias = i == 3 ? arena32 + a->ff1b.off : nullptr;
      if (int rc = dfh::ln_fold_launch(arena16 + src[i]->off, src[i]->K, arena32 + gam[i]->off, arena32 + bet[i]->off, bias,
                                       fold_w() + dst[i]->w, fold_v() + dst[i]->s, fold_v() + dst[i]->b, src[i]->N, src[i]->K, s)) return rc;
    }
  }
#ifdef DFH_PROBES
  for (AttL* a : atts) {
    if (!dfh::WalkKnobs::get().token_linear || !a->has_tl || (fp8 && a->qk8.on)) continue;
    const int C = a->C;
    if (int rc = dfh::token_linear_pack_launch(arena16 + a->pin.off, a->pin.K, fold_w() + a->tl_pin, s)) return rc;
    if (int rc = dfh::token_linear_pack_launch(arena16 + a->o1.off, a->o1.K, fold_w() + a->tl_o1, s)) return rc;
    if (int rc = dfh::token_linear_pack_launch(fold_w() + a->fq2.w, C, fold_w() + a->tl_q2, s)) return rc;
    if (int rc = dfh::token_linear_pack_launch(arena16 + a->o2.off, a->o2.K, fold_w() + a->tl_o2, s)) return rc;
  }
#endif
  for (ResL* r : ress) {
    if (!r->has_u) continue;
    if (int rc = dfh::wino_weight_launch(arena16 + r->w1.off, r->w1.K, fold_w() + r->u1, r->cout, r->cin, dfh::wino_blocked(r->cout, r->cin), s)) return rc;
    if (int rc = dfh::wino_weight_launch(arena16 + r->w2.off, r->w2.K, fold_w() + r->u2, r->cout, r->cout, dfh::wino_blocked(r->cout, r->cout), s)) return rc;
  }
  for (ConvL& c : up_samp)
    if (c.has_ph)
      if (int rc = dfh::ups_phase_fold_launch(arena16 + c.w.off, c.w.K, fold_w() + c.ph, c.cout, c.cin, s)) return rc;
  // ff.net.2 . proj_out: [pout . ff2 | pout] and its bias.  The product runs on the GEMM kernel itself (A = pout [C][C], the W operand
  // = ff2^T [4C][C], transposed into the activation workspace, which no walk is using while the weights are being derived)
  bf16_t* scratch = (bf16_t*)(ws + fold_bytes());
  bf16_t* zero = scratch;                                   // 256 zero bytes, then the transposed matrix
  if (hipMemsetAsync(zero, 0, 256, s) != hipSuccess) { dfh::set_error("hipMemsetAsync failed"); return -2; }
  for (AttL* a : atts) {
    const int C = a->C;
    if (C % 8) continue;
    if (fp8 && a->pout8.on) continue;               // fp8 walk: ff.net.2 and proj_out are two e4m3 launches, the folded matrix is unused
    DFH_REQUIRE(fold_bytes() + 256 + (size_t)4 * C * C * 2 <= ws_bytes, "workspace too small for the weight-fold scratch");
    bf16_t* w2t = scratch + 128;
    if (int rc = dfh::transpose_bf16_launch(arena16 + a->ff2.off, w2t, 1, C, 4 * C, 4 * C, C, 0, 0, s)) return rc;
    GemmArgs g; std::memset(&g, 0, sizeof(g));
    g.M = C; g.N = 4 * C; g.rows_per_b = C;
    g.p_src[0] = arena16 + a->pout.off; g.p_c[0] = C; g.nplain = 1;
    g.W = w2t; g.ldw = C; g.zero = zero;
    g.out = fold_w() + a->fffp.w; g.ld_out = 5 * C; g.out_mode = OUT_BF16;
    if (int rc = dfh::gemm_launch(g, s, 0, /*force_split=*/1)) return rc;
    if (hipMemcpy2DAsync(fold_w() + a->fffp.w + 4 * C, (size_t)5 * C * 2, arena16 + a->pout.off, (size_t)C * 2, (size_t)C * 2, C,
                         hipMemcpyDeviceToDevice, s) != hipSuccess) { dfh::set_error("hipMemcpy2DAsync failed"); return -2; }
    if (int rc = dfh::matvec_bias_launch(arena16 + a->pout.off, C, arena32 + a->ff2b.off, arena32 + a->poutb.off,
                                         fold_v() + a->fffp.b, C, C, s)) return rc;
    if (a->has_mlp && dfh::mlp_fused_form() > 0) {     // the fused feed-forward's weight image from the two folded matrices just derived
#ifdef DFH_PROBES
      auto pack = dfh::mlp_fused_form() == 1 ? dfh::mlp_pack_launch : dfh::mlp2_pack_launch;
#else
      auto pack = dfh::mlp2_pack_launch;
#endif
      if (int rc = pack(fold_w() + a->fff1.w, fold_v() + a->fff1.s, fold_v() + a->fff1.b, fold_w() + a->fffp.w, fold_w() + a->mlp_img, s)) return rc;
    }
  }
  fold_valid = true; fold_dirty = false;
  return 0;
}

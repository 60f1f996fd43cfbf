// How a dfh_unet is laid out, host only: its layers with their slots in the parameter table, the packed arenas and the fold region
// (build), the e4m3 arena (enable_fp8) and the transposed arena of the training path (build_train).  Nothing here launches a kernel.
#include "unet_model.h"

Fold dfh_unet::fold_alloc(int N, int K) {
  Fold f; f.N = N; f.K = K;
  f.w = fold16; fold16 += ((size_t)N * K + 127) & ~(size_t)127;
  f.s = fold32; fold32 += (N + 63) & ~63;
  f.b = fold32; fold32 += (N + 63) & ~63;
  return f;
}

void dfh_unet::build_resnet(const std::string& pre, int cin, int cout, ResL& r, int res) {
  const int temb = cfg.block_out_channels[0] * 4;
  // Winograd (winograd.hip) where it pays and where its bf16 transform-domain roundings are a small part of the layer's error budget:
  // the wide layers (>= 512 channels both ways) of the levels of at most 16 x 16 pixels
  if (res % 2 == 0 && res * res <= wino_max_hw() && cin % 8 == 0 && cout % 8 == 0 && std::min(cin, cout) >= 512) {
    r.has_u = true;
    r.u1 = fold16; fold16 += ((size_t)16 * cout * cin + 127) & ~(size_t)127;
    r.u2 = fold16; fold16 += ((size_t)16 * cout * cout + 127) & ~(size_t)127;
  }
  r.cin = cin; r.cout = cout; r.shortcut = cin != cout; r.pre = pre;
  r.n1w = vec(pre + ".norm1.weight", cin);
  r.n1b = vec(pre + ".norm1.bias", cin);
  r.w1 = mat_alloc(cout, 9 * cin);
  conv_into(pre + ".conv1.weight", cout, cin, r.w1, 0);
  r.b1 = vec(pre + ".conv1.bias", cout);
  r.temb_off = temb_total;
  temb_total += cout;
  // time_emb_proj rows are packed later into the batched matrix (needs the final total): build() does it from the indices
  r.p_tw = add_param(pre + ".time_emb_proj.weight", {cout, temb});
  r.p_tb = add_param(pre + ".time_emb_proj.bias", {cout});
  r.n2w = vec(pre + ".norm2.weight", cout);
  r.n2b = vec(pre + ".norm2.bias", cout);
  r.w2 = mat_alloc(cout, 9 * cout + (r.shortcut ? cin : 0));
  conv_into(pre + ".conv2.weight", cout, cout, r.w2, 0);
  r.b2 = vec(pre + ".conv2.bias", cout);
  if (r.shortcut) {
    mat_into(pre + ".conv_shortcut.weight", cout, cin, true, r.w2, 0, 9 * cout, 0);
    vec_into(pre + ".conv_shortcut.bias", cout, r.b2.off, 0, /*accumulate=*/1);
  }
}

void dfh_unet::build_attn(const std::string& pre, int C, int heads, AttL& a) {
  const bool lin = cfg.use_linear_projection != 0;
  const int X = cfg.cross_attention_dim;
  a.C = C; a.heads = heads; a.pre = pre;
  a.nw = vec(pre + ".norm.weight", C);
  a.nb = vec(pre + ".norm.bias", C);
  a.pin = mat(pre + ".proj_in.weight", C, C, !lin);
  a.pinb = vec(pre + ".proj_in.bias", C);
  const std::string tb = pre + ".transformer_blocks.0";
  a.l1w = vec(tb + ".norm1.weight", C); a.l1b = vec(tb + ".norm1.bias", C);
  a.l2w = vec(tb + ".norm2.weight", C); a.l2b = vec(tb + ".norm2.bias", C);
  a.l3w = vec(tb + ".norm3.weight", C); a.l3b = vec(tb + ".norm3.bias", C);
  a.qk = mat_alloc(2 * C, C);
  mat_into(tb + ".attn1.to_q.weight", C, C, false, a.qk, 0, 0, 0);
  mat_into(tb + ".attn1.to_k.weight", C, C, false, a.qk, C, 0, 0);
  a.v = mat(tb + ".attn1.to_v.weight", C, C);
  a.o1 = mat(tb + ".attn1.to_out.0.weight", C, C);
  a.o1b = vec(tb + ".attn1.to_out.0.bias", C);
  a.q2 = mat(tb + ".attn2.to_q.weight", C, C);
  a.x_off = x_total;            // to_k / to_v of every layer are packed into two stacked matrices (below)
  x_total += C;
  a.p_k2 = add_param(tb + ".attn2.to_k.weight", {C, X});
  a.p_v2 = add_param(tb + ".attn2.to_v.weight", {C, X});
  a.o2 = mat(tb + ".attn2.to_out.0.weight", C, C);
  a.o2b = vec(tb + ".attn2.to_out.0.bias", C);
  a.ff1 = mat(tb + ".ff.net.0.proj.weight", 8 * C, C, false, /*geglu=*/1);
  a.ff1b.N = 8 * C; a.ff1b.off = alloc32(8 * C);
  vec_into(tb + ".ff.net.0.proj.bias", 8 * C, a.ff1b.off, 1, 0);
  a.ff2 = mat(tb + ".ff.net.2.weight", C, 4 * C);
  a.ff2b = vec(tb + ".ff.net.2.bias", C);
  a.pout = mat(pre + ".proj_out.weight", C, C, !lin);
  a.poutb = vec(pre + ".proj_out.bias", C);
  // q | k and v share one folded matrix [3C][C] (and one s / b' vector): ONE launch writes q | k and V^T (GemmArgs::out2); fqk / fv
  // are views of it for the two-launch fallback
  a.fqkv = fold_alloc(3 * C, C);
  a.fqk = a.fqkv; a.fqk.N = 2 * C;
  a.fv = a.fqkv; a.fv.N = C; a.fv.w += (size_t)2 * C * C; a.fv.s += 2 * C; a.fv.b += 2 * C;
  a.fq2 = fold_alloc(C, C); a.fff1 = fold_alloc(8 * C, C);
  a.fffp = fold_alloc(C, 5 * C);
  if (dfh::mlp_fused_eligible(C, 128)) {
    a.has_mlp = true; a.mlp_img = fold16;
    fold16 += (dfh::mlp_fused_image_bytes() / 2 + 127) & ~(size_t)127;
  }
#ifdef DFH_PROBES
  if (dfh::token_linear_eligible(C, C, 128)) {
    a.has_tl = true;
    for (size_t* o : {&a.tl_pin, &a.tl_o1, &a.tl_q2, &a.tl_o2}) { *o = fold16; fold16 += (dfh::token_linear_image_bytes() / 2 + 127) & ~(size_t)127; }
  }
#endif
}

void dfh_unet::build_conv(const std::string& pre, int cout, int cin, ConvL& c) {
  // conv_out has 4 output channels; conv_in 8 (or 4, padded to 8 with zero weights) input channels:
  // both go through the same GEMM
  const int cp = (cin + 7) & ~7;
  c.cin = cp; c.cout = cout; c.pre = pre;
  c.w = mat_alloc(cout, 9 * cp);
  conv_into(pre + ".weight", cout, cin, c.w, 0, cp);
  c.b = vec(pre + ".bias", cout);
}

int dfh_unet::build() {
  const int nb = cfg.num_blocks;
  const int* boc = cfg.block_out_channels;
  const int temb = boc[0] * 4;
  build_conv("conv_in", boc[0], cfg.in_channels, conv_in);
  te1 = mat("time_embedding.linear_1.weight", temb, boc[0]);
  te1b = vec("time_embedding.linear_1.bias", temb);
  te2 = mat("time_embedding.linear_2.weight", temb, temb);
  te2b = vec("time_embedding.linear_2.bias", temb);
  down_res.resize(nb); down_att.resize(nb); down_samp.resize(nb);
  up_res.resize(nb); up_att.resize(nb); up_samp.resize(nb);
  int ch = boc[0];
  for (int i = 0; i < nb; ++i) {
    const int oc = boc[i];
    down_res[i].resize(cfg.layers_per_block);
    if (cfg.down_attn[i]) down_att[i].resize(cfg.layers_per_block);
    for (int j = 0; j < cfg.layers_per_block; ++j) {
      const std::string b = "down_blocks." + std::to_string(i);
      build_resnet(b + ".resnets." + std::to_string(j), j == 0 ? ch : oc, oc, down_res[i][j], cfg.sample_size >> i);
    }
    for (int j = 0; j < cfg.layers_per_block && cfg.down_attn[i]; ++j)
      build_attn("down_blocks." + std::to_string(i) + ".attentions." + std::to_string(j), oc, cfg.num_heads[i], down_att[i][j]);
    if (i != nb - 1) build_conv("down_blocks." + std::to_string(i) + ".downsamplers.0.conv", oc, oc, down_samp[i]);
    ch = oc;
  }
  const int mid = boc[nb - 1];
  build_resnet("mid_block.resnets.0", mid, mid, mid_res[0], cfg.sample_size >> (nb - 1));
  build_attn("mid_block.attentions.0", mid, cfg.num_heads[nb - 1], mid_att);
  build_resnet("mid_block.resnets.1", mid, mid, mid_res[1], cfg.sample_size >> (nb - 1));
  int out_ch = boc[nb - 1];
  for (int i = 0; i < nb; ++i) {
    const int prev = out_ch;
    out_ch = boc[nb - 1 - i];
    const int in_ch = boc[nb - 1 - std::min(i + 1, nb - 1)];
    const bool att = cfg.down_attn[nb - 1 - i] != 0;
    const int L = cfg.layers_per_block + 1;
    up_res[i].resize(L);
    if (att) up_att[i].resize(L);
    const std::string b = "up_blocks." + std::to_string(i);
    for (int j = 0; j < L; ++j) {
      const int skip = (j == L - 1) ? in_ch : out_ch;
      const int hid = (j == 0) ? prev : out_ch;
      build_resnet(b + ".resnets." + std::to_string(j), hid + skip, out_ch, up_res[i][j], cfg.sample_size >> (nb - 1 - i));
    }
    for (int j = 0; j < L && att; ++j)
      build_attn(b + ".attentions." + std::to_string(j), out_ch, cfg.num_heads[nb - 1 - i], up_att[i][j]);
    if (i != nb - 1) {
      build_conv(b + ".upsamplers.0.conv", out_ch, out_ch, up_samp[i]);
      if (out_ch % 8 == 0) {
        up_samp[i].ph = fold16; up_samp[i].has_ph = true;
        fold16 += ((size_t)16 * out_ch * out_ch + 127) & ~(size_t)127;
      }
    }
  }
  cnw = vec("conv_norm_out.weight", boc[0]);
  cnb = vec("conv_norm_out.bias", boc[0]);
  build_conv("conv_out", cfg.out_channels, boc[0], conv_out);
  // batched time_emb_proj: [temb_total][temb] + bias; rows of each resnet at its temb_off
  tproj = mat_alloc(temb_total, temb);
  tprojb.N = temb_total; tprojb.off = alloc32(temb_total);
  // batched cross-attention K / V projections of the text states: [x_total][cross_dim] each
  kx_all = mat_alloc(x_total, cfg.cross_attention_dim);
  vx_all = mat_alloc(x_total, cfg.cross_attention_dim);
  // the layers in walk order, once: nothing resizes the vectors they point into after this
  for (auto& lv : down_res) for (ResL& r : lv) ress.push_back(&r);
  ress.push_back(&mid_res[0]); ress.push_back(&mid_res[1]);
  for (auto& lv : up_res) for (ResL& r : lv) ress.push_back(&r);
  for (auto& lv : down_att) for (AttL& a : lv) atts.push_back(&a);
  atts.push_back(&mid_att);
  for (auto& lv : up_att) for (AttL& a : lv) atts.push_back(&a);
  const int X = cfg.cross_attention_dim;
  for (const AttL* a : atts) {
    packs.push_back({a->p_k2, PK_MAT, kx_all.off, a->C, X, X, a->x_off, 0, 0, 0});
    packs.push_back({a->p_v2, PK_MAT, vx_all.off, a->C, X, X, a->x_off, 0, 0, 0});
  }
  for (const ResL* r : ress) {
    packs.push_back({r->p_tw, PK_MAT, tproj.off, r->cout, temb, temb, r->temb_off, 0, 0, 0});
    packs.push_back({r->p_tb, PK_VEC, tprojb.off + (size_t)r->temb_off, r->cout, 0, 0, 0, 0, 0, 0});
  }
  return 0;
}

// fp8 copies exist for the transformer layers whose width the 64-deep contraction divides
int dfh_unet::enable_fp8() {
  if (fp8) return 0;
  a8 = 0;
  auto take = [&](const Mat& m, Mat8& q, bool with_bias = false) {
    q.N = m.N; q.K = m.K; q.on = true;
    q.off = a8; a8 += ((size_t)m.N * m.K + 255) & ~(size_t)255;
    q.soff = a8; a8 += ((size_t)m.N * sizeof(float) + 255) & ~(size_t)255;
    if (with_bias) { q.boff = a8; a8 += ((size_t)m.N * sizeof(float) + 255) & ~(size_t)255; }
  };
  // DFH_FP8_EXT=0: only the round-2 set (the LayerNorm-fed projections) -- A/B switch
  const bool ext_off = !dfh::WalkKnobs::get().fp8_ext;
  int idx = 0;
  for (AttL* a : atts) {
    a->idx = idx++;
    if (a->C % 64) continue;
    take(a->qk, a->qk8); take(a->v, a->v8); take(a->q2, a->q28); take(a->ff1, a->ff18);
    if (ext_off) continue;
    take(a->o1, a->o18); take(a->o2, a->o28); take(a->ff2, a->ff28); take(a->pout, a->pout8); take(a->pin, a->pin8, true);
    // opt-in (dfh_unet_enable_fp8_attention / DFH_FP8_ATTN=1): see dfh_unet::fp8_attention
    const bool attn_off = !(fp8_attention || dfh::WalkKnobs::get().fp8_attn);
    const int D = a->C / a->heads;
    const bool v_contig = a->v.off == a->qk.off + (size_t)2 * a->C * a->C && a->v.K == a->qk.K;
    if (!attn_off && v_contig && (D == 40 || D == 80 || D == 160)) {
      a->f8a = true; a->f8a_off = a8; a8 += ((size_t)(3 * a->C + a->heads) * sizeof(float) + 255) & ~(size_t)255;
    }
  }
  n_att = idx;
  // (row offset, row count) of every layer's slice of the batched cross-attention V^T: the slabs of amax_slabs_kernel
  a8_slab_off = a8; a8 += ((size_t)2 * n_att * sizeof(int) + 255) & ~(size_t)255;
  slab_host.assign(2 * n_att, 0);
  for (AttL* a : atts) { slab_host[a->idx] = a->x_off; slab_host[n_att + a->idx] = a->C; }
  fp8 = true;
  return 0;
}

// transposed packs of the training path (arena16t): see bwd_elementwise.hip pack_*_t kernels
int dfh_unet::build_train() {
  if (train_built) return 0;
  std::map<std::string, int> idx;
  for (int i = 0; i < (int)params.size(); ++i) idx[params[i].name] = i;
  auto talloc = [&](int N, int K) { Mat m; m.N = N; m.K = K; m.off = a16t; a16t += ((size_t)N * K + 127) & ~(size_t)127; return m; };
  auto tmat = [&](const std::string& name, int N, int K, const Mat& dst, int t_row_off, int t_col_off, int geglu) {
    tpacks.push_back({idx.at(name), 0, dst.off, N, K, dst.K, t_row_off, t_col_off, geglu, 0});
  };
  auto tconv = [&](const std::string& name, int cout, int cin, const Mat& dst, int o_pad) {
    tpacks.push_back({idx.at(name), 1, dst.off, cout, cin, dst.K, 0, 0, 0, o_pad});
  };
  const int temb = cfg.block_out_channels[0] * 4;
  tprojt = talloc(temb, temb_total);
  te2t = talloc(temb, temb);
  tmat("time_embedding.linear_2.weight", temb, temb, te2t, 0, 0, 0);
  auto res = [&](ResL& r) {
    r.w1t = talloc(r.cin, 9 * r.cout);
    tconv(r.pre + ".conv1.weight", r.cout, r.cin, r.w1t, r.cout);
    r.w2t = talloc(r.cout, 9 * r.cout);
    tconv(r.pre + ".conv2.weight", r.cout, r.cout, r.w2t, r.cout);
    if (r.shortcut) {
      r.wst = talloc(r.cin, r.cout);
      tmat(r.pre + ".conv_shortcut.weight", r.cout, r.cin, r.wst, 0, 0, 0);
    }
    tmat(r.pre + ".time_emb_proj.weight", r.cout, temb, tprojt, 0, r.temb_off, 0);
  };
  auto att = [&](AttL& a) {
    const int C = a.C;
    const std::string tb = a.pre + ".transformer_blocks.0";
    a.pint = talloc(C, C); tmat(a.pre + ".proj_in.weight", C, C, a.pint, 0, 0, 0);
    a.qkvt = talloc(C, 3 * C);
    tmat(tb + ".attn1.to_q.weight", C, C, a.qkvt, 0, 0, 0);
    tmat(tb + ".attn1.to_k.weight", C, C, a.qkvt, 0, C, 0);
    tmat(tb + ".attn1.to_v.weight", C, C, a.qkvt, 0, 2 * C, 0);
    a.o1t = talloc(C, C); tmat(tb + ".attn1.to_out.0.weight", C, C, a.o1t, 0, 0, 0);
    a.q2t = talloc(C, C); tmat(tb + ".attn2.to_q.weight", C, C, a.q2t, 0, 0, 0);
    a.o2t = talloc(C, C); tmat(tb + ".attn2.to_out.0.weight", C, C, a.o2t, 0, 0, 0);
    a.ff1t = talloc(C, 8 * C); tmat(tb + ".ff.net.0.proj.weight", 8 * C, C, a.ff1t, 0, 0, 1);
    a.ff2t = talloc(4 * C, C); tmat(tb + ".ff.net.2.weight", C, 4 * C, a.ff2t, 0, 0, 0);
    a.poutt = talloc(C, C); tmat(a.pre + ".proj_out.weight", C, C, a.poutt, 0, 0, 0);
  };
  auto cv = [&](ConvL& c, int real_cin) {
    const int op = (c.cout + 7) & ~7;
    c.wt = talloc(c.cin, 9 * op);                  // rows beyond real_cin / columns beyond cout stay zero (zero-filled arena)
    tconv(c.pre + ".weight", c.cout, real_cin, c.wt, op);
  };
  cv(conv_in, cfg.in_channels);
  cv(conv_out, conv_out.cin);
  // the mid block behind the up blocks: the order arena16t has been laid out in from the start (its offsets are in every recorded plan)
  for (ResL* r : ress) if (r != &mid_res[0] && r != &mid_res[1]) res(*r);
  res(mid_res[0]); res(mid_res[1]);
  for (AttL* a : atts) if (a != &mid_att) att(*a);
  att(mid_att);
  for (int i = 0; i + 1 < cfg.num_blocks; ++i) { cv(down_samp[i], down_samp[i].cin); cv(up_samp[i], up_samp[i].cin); }
  train_built = true;
  return 0;
}

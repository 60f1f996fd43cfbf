#!/usr/bin/env python3
"""Output identity of the fp32 evaluation rows that share csrc/f32_tile.h (the CLIP towers' and the compatibility scorer's Linears and
LayerNorms, the LPIPS convolution and its score sum, the Inception convolution, classifier, means and statistics, the ragged ranking)
between two builds of the library (GPU only).

One process, one library (DFH_LIB chooses it): a fixed list of seeded cases goes through the public entry points, and one line per case
carries the SHA-256 of every output.  Run it with each build and compare the two outputs line for line:

  DFH_LIB=<other build> python scripts/f32_rows_identity.py > a.txt;  python scripts/f32_rows_identity.py > b.txt;  cmp a.txt b.txt
  python scripts/f32_rows_identity.py --only scorer          # the cases whose name contains the text

Weights and inputs come from seeds (CPU generators): no fixtures.  The shapes are the smallest that reach every edge of the shared
steps: ragged M and N tiles, a ragged last k-tile, one and many k-tiles, one M tile, both LPIPS chunk widths, partial spatial tiles."""
import ctypes as C
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import difashion_amd as da
from difashion_amd import _lib
from tests.test_gpu_inception import CONV_CASES

DEV = "cuda"


def sha(t):
    return hashlib.sha256(t.contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()[:32]


def rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator(device="cpu").manual_seed(seed))


def seeded(module, seed):
    """Every parameter from one CPU generator: matrices at 0.7 / sqrt(fan-in), vectors at 0.1 (+ 1 for a norm's weight)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    with torch.no_grad():
        for name, p in module.named_parameters():
            if name.startswith("scaling_layer."):
                continue
            v = torch.randn(p.shape, generator=g)
            v = v * (0.7 / p[0].numel() ** 0.5) if p.dim() >= 2 else 0.1 * v + (1.0 if name.endswith("weight") else 0.0)
            p.copy_(v.abs() if name.startswith("lin") else v)
    return module.to(DEV)


def ids(B, T, vocab, seed):
    return torch.randint(1, vocab - 1, (B, T), generator=torch.Generator(device="cpu").manual_seed(seed))


TEXT_A = dict(vocab_size=1000, hidden_size=64, intermediate_size=128, num_hidden_layers=3, num_attention_heads=2, hidden_act="quick_gelu")
TEXT_B = dict(vocab_size=1000, hidden_size=96, intermediate_size=160, num_hidden_layers=2, num_attention_heads=2, hidden_act="gelu",
              projection_dim=48)


def text_encode(B, T):
    out = seeded(da.CLIPTextModel(**TEXT_A, init_seed=None), 11)(ids(B, T, 1000, 12), output_hidden_states=True)
    return dict(last=out.last_hidden_state, pooled=out.pooler_output, hidden=torch.stack(out.hidden_states))


def text_embeds():
    m = seeded(da.CLIPTextModelWithProjection(**TEXT_B, init_seed=None), 21)
    tok = ids(4, 77, 1000, 22)
    out = m(tok)
    return dict(embeds=out.text_embeds, last=out.last_hidden_state, pooled=out.pooler_output, encode_text=m.encode_text(tok))


def vision(image, patch, B):
    m = seeded(da.CLIPVisionModelWithProjection(hidden_size=64, intermediate_size=128, projection_dim=32, num_hidden_layers=2,
                                                num_attention_heads=2, image_size=image, patch_size=patch, init_seed=None), 31)
    out = m(rnd(B, 3, image, image, seed=32).to(DEV), output_hidden_states=True)
    return dict(embeds=out.image_embeds, last=out.last_hidden_state, pooled=out.pooler_output, hidden=torch.stack(out.hidden_states))


def scorer(dim, outfits, items):
    ce = da.CompatibilityEvaluator(seeded(da.FashionEvaluator(dim), 41), DEV)
    real, gen = rnd(50, dim, seed=42).to(DEV), rnd(outfits * items, dim, seed=43).to(DEV)
    ol = torch.randint(1, 50, (outfits, items), generator=torch.Generator(device="cpu").manual_seed(44))
    ol[:, 0] = -torch.arange(outfits)                       # one generated item an outfit
    emb, logits, scores = ce.evaluate_compatibility(ol, real, gen, return_all=True)
    return dict(emb=emb, logits=logits, scores=scores)


def pred_score(outfits):
    return dict(logits=seeded(da.FashionEvaluator(64), 41).pred_score(rnd(outfits, 256, seed=45).to(DEV)))


def lpips_conv(cin, cout, h, w):
    w_cin = 3 if cin == 4 else cin                          # the first layer: three channels padded to four
    x, wt, bias = rnd(2, h, w, cin, seed=51).to(DEV), (rnd(cout, w_cin, 3, 3, seed=52) * (2.0 / (9 * w_cin)) ** 0.5).to(DEV), rnd(cout, seed=53).to(DEV)
    packed, out = torch.empty(9 * cin * cout, device=DEV), torch.empty((2, h, w, cout), device=DEV)
    _lib.call("dfh_lpips_conv3x3_relu", _lib.ptr(x), _lib.ptr(wt), w_cin, _lib.ptr(bias), _lib.ptr(packed), _lib.ptr(out), 2, h, w, cin, cout,
              _lib.stream_ptr())
    return dict(out=out)


def lpips_forward(h, w):
    m = seeded(da.LPIPS(init_seed=None), 61)
    a, b = (rnd(2, 3, h, w, seed=s).clamp(-1, 1).to(DEV) for s in (62, 63))
    val, layers = m(a, b, retPerLayer=True)
    return dict(distance=val, per_layer=torch.cat(layers))


def incep_conv(cin, cout, k, stride, pad, h, w, ldc, offset, n=3):
    g = torch.Generator(device="cpu").manual_seed(cin * 131 + cout)
    cin_pad = (cin + 3) // 4 * 4
    x = torch.zeros((n, h, w, cin_pad))
    x[..., :cin] = torch.randn((n, h, w, cin), generator=g)
    wt = torch.randn((cout, cin, k[0], k[1]), generator=g) * (2.0 / (cin * k[0] * k[1])) ** 0.5
    bn = [(0.75 + 0.5 * torch.rand(cout, generator=g)).to(DEV), (0.1 * torch.randn(cout, generator=g)).to(DEV),
          (0.2 * torch.randn(cout, generator=g)).to(DEV), (0.5 + torch.rand(cout, generator=g)).to(DEV)]
    x, wt = x.to(DEV), wt.to(DEV)
    oh, ow = (h + 2 * pad[0] - k[0]) // stride + 1, (w + 2 * pad[1] - k[1]) // stride + 1
    out = torch.full((n, oh, ow, ldc), float("nan"), device=DEV)
    packed = torch.empty((cout * (k[0] * k[1] * cin_pad + 2),), device=DEV)
    _lib.call("dfh_incep_conv_bn_relu", _lib.ptr(x), _lib.ptr(wt), cin, (C.c_void_p * 4)(*[t.data_ptr() for t in bn]), _lib.ptr(packed), _lib.ptr(out),
              n, h, w, cin_pad, cout, k[0], k[1], stride, pad[0], pad[1], ldc, offset, _lib.stream_ptr())
    return dict(out=out[..., offset:offset + cout], packed=packed)


def incep_fc(n, K, classes):
    feat, wt, bias = rnd(n, K, seed=71).to(DEV), (rnd(classes, K, seed=72) * K ** -0.5).to(DEV), rnd(classes, seed=73).to(DEV)
    logits, probs = torch.empty((n, classes), device=DEV), torch.empty((n, classes), device=DEV)
    _lib.call("dfh_incep_fc_softmax", _lib.ptr(feat), _lib.ptr(wt), _lib.ptr(bias), _lib.ptr(logits), _lib.ptr(probs), n, K, classes, _lib.stream_ptr())
    return dict(logits=logits, probs=probs)


def incep_gmean(n, hw, c):
    x, out = rnd(n, hw, c, seed=74).to(DEV), torch.empty((n, c), device=DEV)
    _lib.call("dfh_incep_global_mean", _lib.ptr(x), _lib.ptr(out), n, hw, c, _lib.stream_ptr())
    return dict(mean=out)


def incep_stats(N, D):
    act = rnd(N, D, seed=75).to(DEV)
    mu, sigma = torch.empty((D,), dtype=torch.float64, device=DEV), torch.empty((D, D), dtype=torch.float64, device=DEV)
    _lib.call("dfh_incep_stats", _lib.ptr(act), N, D, _lib.ptr(mu), _lib.ptr(sigma), _lib.stream_ptr())
    return dict(mu=mu, sigma=sigma)


def incep_model(make):
    m = make().to(DEV)                                      # the wrappers' own seeded stand-ins (init_seed=0)
    x = torch.rand(2, 3, 80, 96, generator=torch.Generator(device="cpu").manual_seed(81)).to(DEV)
    out = m(x)
    return {f"block{b}": t for b, t in zip(m.output_blocks, out)} if isinstance(out, list) else dict(probs=out, feat=m.feature_extract(x))


def ragged_rank():
    gen, table = rnd(75, 44, seed=91).to(DEV), rnd(150, 44, seed=92).to(DEV)
    perm = torch.randperm(150, generator=torch.Generator(device="cpu").manual_seed(93))
    r = da.rank_candidates(gen, table, (torch.tensor([0] * 5 + [1] * 70), [perm[:3], perm[3:133]]), 100)
    return dict(ids=r.ids, positions=r.positions, sims=r.sims, counts=r.counts)


def all_finite(name, v):
    return name == "sims" or not v.is_floating_point() or bool(torch.isfinite(v).all())       # empty rank slots hold -inf


CASES = [
    ("text dfh_clip_encode 64/128 x3 B=5 T=77 quick_gelu (M=385)", lambda: text_encode(5, 77)),
    ("text dfh_clip_text_embeds 96/160 x2 B=4 T=77 gelu proj 48", text_embeds),
    ("text dfh_clip_encode 64/128 x3 B=3 T=5 (one M tile)", lambda: text_encode(3, 5)),
    ("vision dfh_clipv_encode 42 px patch 14 (K=588)", lambda: vision(42, 14, 3)),
    ("vision dfh_clipv_encode 112 px patch 8 (T=197)", lambda: vision(112, 8, 2)),
    ("scorer dfh_compat_score feat_dim 44, 5 x 3", lambda: scorer(44, 5, 3)),
    ("scorer dfh_compat_score feat_dim 1024, 1 x 4", lambda: scorer(1024, 1, 4)),
    ("scorer dfh_compat_score feat_dim 1024, 65 x 4", lambda: scorer(1024, 65, 4)),
    ("scorer dfh_compat_pred_score 65 embeddings", lambda: pred_score(65)),
] + [(f"lpips dfh_lpips_conv3x3_relu ({cin}, {cout}, {h}, {w})", lambda s=(cin, cout, h, w): lpips_conv(*s))
     for cin, cout, h, w in ((4, 64, 19, 23), (64, 128, 19, 23), (256, 256, 11, 13), (512, 512, 9, 10))] + [
    ("lpips dfh_lpips_forward 16x16, 2 pairs", lambda: lpips_forward(16, 16)),
    ("lpips dfh_lpips_forward 37x45, 2 pairs", lambda: lpips_forward(37, 45)),
] + [("incep dfh_incep_conv_bn_relu n=3 " + str(c).replace(" ", ""), lambda c=c: incep_conv(*c)) for c in CONV_CASES] + [
    ("incep dfh_incep_fc_softmax n=5 K=100 classes=50", lambda: incep_fc(5, 100, 50)),
    ("incep dfh_incep_global_mean n=2 HW=35 C=70", lambda: incep_gmean(2, 35, 70)),
    ("incep dfh_incep_stats (5, 70)", lambda: incep_stats(5, 70)),
    ("incep dfh_incep_stats (33, 130)", lambda: incep_stats(33, 130)),
    ("incep FIDInceptionV3((0, 1, 2, 3)) 2 x 80 x 96, resize", lambda: incep_model(lambda: da.FIDInceptionV3((0, 1, 2, 3)))),
    ("incep InceptionV3(num_classes=50) 2 x 80 x 96, resize", lambda: incep_model(lambda: da.InceptionV3(num_classes=50, resize_input=True, normalize_input=True))),
    ("rank rank_candidates 5 + 70 rows, 3 / 130 candidates, dim 44", ragged_rank),
]


if __name__ == "__main__":
    only = sys.argv[sys.argv.index("--only") + 1] if "--only" in sys.argv else ""
    torch.set_grad_enabled(False)
    print(f"# storage={_lib.storage()}", flush=True)
    for name, run in CASES:
        if only not in name:
            continue
        outs = run()
        torch.cuda.synchronize()
        finite = all(all_finite(k, v) for k, v in outs.items())
        print(f"{name:62s} " + " ".join(f"{k} {sha(v)}" for k, v in outs.items()) + ("" if finite else " NOT-FINITE"), flush=True)

#!/usr/bin/env python3
"""Throughput of the HIP CLIP image encoder at the evaluation's shape: 200 images of ViT-H/14 (224 x 224, 257 tokens)
in batches of 50, timed with HIP events after one warm-up batch.  Writes one JSON line to profiles/clip_vision_bench.json: images / s,
ms per batch, achieved TFLOP/s against the 157.3 TFLOP/s fp32-MFMA peak, and -- from a second, separately profiled batch
(dfh_prof_begin / dfh_prof_end bracket every launch with events, so it is not the timed run) -- the split by kernel class:
linears / attention / LayerNorm / embedding.

    python scripts/bench_clip_vision.py [--images 200] [--batch 50] [--model vit_h_14|vit_l_14] [--out profiles/clip_vision_bench.json]
"""
import argparse
import os

import torch
from _rowbench import ROOT, emit, header, randomise

import difashion_amd as da  # noqa: E402
from difashion_amd import _lib  # noqa: E402

PEAK_FP32_MFMA_TFLOPS = 157.3
MODELS = {
    "vit_h_14": dict(hidden_size=1280, intermediate_size=5120, projection_dim=1024, num_hidden_layers=32, num_attention_heads=16,
                     image_size=224, patch_size=14, hidden_act="gelu"),
    "vit_l_14": dict(hidden_size=1024, intermediate_size=4096, projection_dim=768, num_hidden_layers=24, num_attention_heads=16,
                     image_size=224, patch_size=14, hidden_act="quick_gelu"),
}


def flops_per_image(cfg):
    """Multiply-adds x 2 of one image: (linears, attention products, patch embedding + projection)."""
    D, I, L, T = cfg["hidden_size"], cfg["intermediate_size"], cfg["num_hidden_layers"], 1 + (cfg["image_size"] // cfg["patch_size"]) ** 2
    linears = 2.0 * L * T * (4 * D * D + 2 * D * I)
    attention = 4.0 * L * T * T * D
    embed = 2.0 * (T - 1) * D * 3 * cfg["patch_size"] ** 2 + 2.0 * D * cfg["projection_dim"]
    return linears, attention, embed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=200)
    ap.add_argument("--batch", type=int, default=50)
    ap.add_argument("--model", default="vit_h_14", choices=list(MODELS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_vision_bench.json"))
    a = ap.parse_args()
    cfg = MODELS[a.model]
    torch.cuda.set_device(0)
    # weights: small random values drawn on the device (the speed does not depend on them; parity is tests/test_gpu_clip_vision.py)
    m = da.CLIPVisionModelWithProjection(**cfg, init_seed=None).to("cuda").eval().requires_grad_(False)
    g = torch.Generator(device="cuda").manual_seed(0)
    randomise(m, g)
    n_batches = max(1, a.images // a.batch)
    px = torch.randn(n_batches, a.batch, 3, cfg["image_size"], cfg["image_size"], generator=g, device="cuda")
    m.encode_image(px[0])                                   # warm-up: workspace allocation, code-object load
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(n_batches + 1)]
    ev[0].record()
    for i in range(n_batches):
        emb = m.encode_image(px[i])
        ev[i + 1].record()
    torch.cuda.synchronize()
    assert torch.isfinite(emb).all()
    per_batch = [ev[i].elapsed_time(ev[i + 1]) for i in range(n_batches)]
    total_ms = ev[0].elapsed_time(ev[-1])
    lin, att, emb_f = flops_per_image(cfg)
    flops = (lin + att + emb_f) * a.batch * n_batches
    tflops = flops / (total_ms * 1e-3) / 1e12
    # per-class split from a profiled batch of its own
    _lib.prof_begin()
    m.encode_image(px[0])
    prof = _lib.prof_end()
    names = {"gemm_linear": "linears", "attention": "attention", "layernorm": "layernorm", "other": "embedding"}
    prof_ms = sum(prof[k]["ms"] for k in names)
    split = {v: dict(ms=round(prof[k]["ms"], 3), launches=prof[k]["launches"], share_of_time=round(prof[k]["ms"] / prof_ms, 4),
                     tflops=round(prof[k]["flops"] / (prof[k]["ms"] * 1e-3) / 1e12, 2) if prof[k]["ms"] > 0 else 0.0) for k, v in names.items()}
    res = dict(model=a.model, images=a.batch * n_batches, batch=a.batch, images_per_s=round(a.batch * n_batches / (total_ms * 1e-3), 2),
               ms_per_batch=round(total_ms / n_batches, 3), ms_per_batch_each=[round(t, 3) for t in per_batch],
               tflops=round(tflops, 2), fraction_of_fp32_mfma_peak=round(tflops / PEAK_FP32_MFMA_TFLOPS, 4),
               peak_tflops=PEAK_FP32_MFMA_TFLOPS, flops_share=dict(linears=round(lin / (lin + att + emb_f), 4),
                                                                  attention=round(att / (lin + att + emb_f), 4),
                                                                  embedding=round(emb_f / (lin + att + emb_f), 4)),
               profiled_batch=split, **header())
    emit(res, a.out)


if __name__ == "__main__":
    main()

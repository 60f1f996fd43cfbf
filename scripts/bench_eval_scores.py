#!/usr/bin/env python3
"""Throughput of DESIGN.md row f6, reported and not gated: one JSON line to profiles/eval_scores_bench.json.

  * compatibility scorer: outfits / s at 4096 outfits x 4 items x 1024 (dfh_compat_score on device ids: the kernels, gather included,
    without evaluate_compatibility's host-side check of the ids);
  * pair cosine: rows / s at 65 536 x 1024 against its byte time (two reads of rows x dim fp32 at the HBM peak);
  * encode_text of the 51 category prompts on the OpenCLIP ViT-H/14 text shape, beside dfh_clip_encode over the same tower.

Every shape is warmed up twice, then timed with HIP events over windows of >= 0.2 s; the figure is the median of five windows and the
spread (min .. max) is kept.  Weights are small random values drawn on the device: the speed does not depend on them.

    python scripts/bench_eval_scores.py [--out profiles/eval_scores_bench.json]
"""
import argparse
import os

import torch
from _rowbench import ROOT, emit, header, randomise, timed

import difashion_amd as da  # noqa: E402

PEAK_HBM_GBPS = 8000.0
TEXT_H = dict(vocab_size=49408, hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, num_attention_heads=16,
              max_position_embeddings=77, hidden_act="gelu", eos_token_id=2, projection_dim=1024)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_scores_bench.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    torch.set_grad_enabled(False)
    g = torch.Generator(device="cuda").manual_seed(0)
    res = header()

    O, items, dim = 4096, 4, 1024
    ev = da.FashionEvaluator(dim).to("cuda")
    real, gen = torch.randn(20000, dim, generator=g, device="cuda"), torch.randn(O * items, dim, generator=g, device="cuda")
    ol = torch.randint(1, 20000, (O, items), generator=g, device="cuda")
    ol[:, 0] = -torch.arange(O, device="cuda")
    # the kernels alone (gather included): device ids straight into the entry point, without evaluate_compatibility's host-side range check
    # of the ids and their copy to the device
    t = timed(lambda: ev._score("bench", real, gen, ol, O, items))
    pairs = O * items * (items - 1) // 2
    flops = 2.0 * (O * items * dim * 1024 + pairs * (2048 * 512 + 512 * 512 + 512 * 256 + 256 * 256) + O * (256 * 128 + 128 * 128 + 128 * 32 + 32))
    res["compat"] = dict(outfits=O, items=items, dim=dim, outfits_per_s=round(O / (t["ms"] * 1e-3), 1), tflops=round(flops / (t["ms"] * 1e-3) / 1e12, 2), **t)

    rows = 65536
    x, y = torch.randn(rows, dim, generator=g, device="cuda"), torch.randn(rows, dim, generator=g, device="cuda")
    t = timed(lambda: da.pair_cosine(x, y))
    byte_ms = 2.0 * rows * dim * 4 / (PEAK_HBM_GBPS * 1e9) * 1e3
    res["pair_cosine"] = dict(rows=rows, dim=dim, rows_per_s=round(rows / (t["ms"] * 1e-3), 1), byte_time_ms=round(byte_ms, 4),
                              fraction_of_byte_time=round(byte_ms / t["ms"], 3), peak_hbm_gbps=PEAK_HBM_GBPS, **t)

    K = 1000
    cand = torch.randint(0, 20000, (256, K), generator=g, device="cuda").cpu()
    t = timed(lambda: da.candidate_cosine(x[:256], real, cand))
    res["candidates"] = dict(rows=256, K=K, dim=dim, sims_per_s=round(256 * K / (t["ms"] * 1e-3), 1), **t)

    m = da.CLIPTextModelWithProjection(**TEXT_H, init_seed=None).to("cuda").eval().requires_grad_(False)
    randomise(m, g)
    ids = torch.randint(1, 49000, (51, 77), generator=torch.Generator().manual_seed(0))
    ids[:, 0], ids[:, 40] = 49406, 49407
    t_embeds = timed(lambda: m.encode_text(ids))
    base = da.CLIPTextModel(**{k: v for k, v in TEXT_H.items() if k != "projection_dim"}, init_seed=None).to("cuda").eval().requires_grad_(False)
    randomise(base, g)
    t_encode = timed(lambda: base(ids))
    res["encode_text"] = dict(prompts=51, seq_len=77, shape="OpenCLIP ViT-H/14 text tower, 24 x 1024, projection 1024", **t_embeds)
    res["clip_encode_same_tower"] = dict(prompts=51, seq_len=77, **t_encode)
    emit(res, a.out)


if __name__ == "__main__":
    main()

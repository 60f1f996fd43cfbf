#!/usr/bin/env python3
"""Throughput of DESIGN.md row f7, reported and not gated: one JSON line to profiles/image_processor_bench.json.

  * uint8 source: 200 x 512^2 -> 224 (200 is the reference's cnn_batch_size), device-event ms and images / s;
  * fp32 source (what vae.decode leaves on the device): the same;
  * sheets: 50 sheets of 4 x 512^2 (grid=4, the 1024^2 outfit sheet), never materialised;
  * each against its byte time: the input once plus the fp32 output once at the HBM peak, and the fraction reached;
  * beside them, in the same run: encode_image of the same 200 images at ViT-H/14, and PIL's ms per image on this host where PIL imports.

Every case is warmed up twice, then timed with HIP events over windows of >= 0.2 s; the figure is the median of five windows and the
spread (min .. max) is kept.  The kernel's time does not depend on the pixel values.

    python scripts/bench_image_processor.py [--out profiles/image_processor_bench.json] [--no-tower]
"""
import argparse
import os
import time

import numpy as np
import torch
from _rowbench import ROOT, emit, header, randomise, timed

import difashion_amd as da  # noqa: E402

PEAK_HBM_GBPS = 8000.0
VIT_H_14 = dict(hidden_size=1280, intermediate_size=5120, projection_dim=1024, num_hidden_layers=32, num_attention_heads=16,
                image_size=224, patch_size=14, hidden_act="gelu")


def case(p, src, images, grid=None):
    t = timed(lambda: p(images=src, grid=grid))
    nbytes = src.numel() * src.element_size() + images * 3 * 224 * 224 * 4
    byte_ms = nbytes / (PEAK_HBM_GBPS * 1e9) * 1e3
    return dict(images=images, source=f"{src.dtype} {tuple(src.shape)}", grid=grid, images_per_s=round(images / (t["ms"] * 1e-3), 1),
                bytes=nbytes, byte_time_ms=round(byte_ms, 4), fraction_of_byte_time=round(byte_ms / t["ms"], 3),
                peak_hbm_gbps=PEAK_HBM_GBPS, **t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "image_processor_bench.json"))
    ap.add_argument("--no-tower", action="store_true", help="leave out encode_image at ViT-H/14")
    a = ap.parse_args()
    torch.cuda.set_device(0)
    torch.set_grad_enabled(False)
    g = torch.Generator(device="cuda").manual_seed(0)
    res = header(card=True)
    p = da.CLIPImageProcessor()

    u8 = torch.randint(0, 256, (200, 512, 512, 3), generator=g, device="cuda", dtype=torch.uint8)
    res["uint8_512_to_224"] = case(p, u8, 200)
    f32 = torch.rand((200, 3, 512, 512), generator=g, device="cuda") * 2 - 1
    res["fp32_512_to_224"] = case(p, f32, 200)
    del f32
    res["sheets_4x512_to_224"] = case(p, u8, 50, grid=4)

    if not a.no_tower:
        m = da.CLIPVisionModelWithProjection(**VIT_H_14, init_seed=None).to("cuda").eval().requires_grad_(False)
        randomise(m, g)
        px = p(images=u8).pixel_values
        t = timed(lambda: m.encode_image(px), windows=3, min_window_ms=1.0)
        res["encode_image_vit_h_14"] = dict(images=200, ms_per_image=round(t["ms"] / 200, 4), **t)
    try:
        from PIL import Image
        img = Image.fromarray(u8[0].cpu().numpy())
        sheet = Image.fromarray(np.zeros((1024, 1024, 3), np.uint8))
        out = {}
        for name, im in (("512", img), ("1024_sheet", sheet)):
            im.resize((224, 224), 3)
            t0 = time.perf_counter()
            for _ in range(10):
                im.resize((224, 224), 3)
            out[name + "_ms_per_image"] = round((time.perf_counter() - t0) / 10 * 1e3, 3)
        import PIL
        res["pil_on_this_host"] = dict(version=PIL.__version__, **out)
    except ImportError:
        res["pil_on_this_host"] = None
    emit(res, a.out)


if __name__ == "__main__":
    main()

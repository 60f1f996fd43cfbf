#!/usr/bin/env python3
"""Time of DESIGN.md row f10, the JPEG save / open round trip, reported and not gated: one JSON line to profiles/jpeg_roundtrip_bench.json.

  * device time per image of ``jpeg_roundtrip`` at 512^2 (quality 75, 4:2:0, the reference's setting) for batches 1, 16 and 64, uint8
    source, and batch 64 from the fp32 source ``vae.decode`` leaves on the device;
  * each against its byte floor: the source once, the decoded planes written and read once, the result once (about 2.4 MB a 512^2
    image over both launches) at the HBM peak, and the fraction reached;
  * beside them, in the same run: PIL's own round trip (save to memory, open, convert) on one core of this host.

Every case is warmed up twice, then timed with HIP events over windows of >= 0.2 s; the figure is the median of five windows and the
spread (min .. max) is kept.  The kernels' time does not depend on the pixel values.

    python scripts/bench_jpeg.py [--out profiles/jpeg_roundtrip_bench.json]
"""
import argparse
import io
import os
import time

import numpy as np
import torch
from _rowbench import ROOT, _lib, emit, header, timed

import difashion_amd as da  # noqa: E402

PEAK_HBM_GBPS = 8000.0
H = W = 512


def case(src, images):
    t = timed(lambda: da.jpeg_roundtrip(src))
    planes = _lib.raw().dfh_jpeg_workspace_bytes(images, H, W, 2)
    nbytes = src.numel() * src.element_size() + 2 * planes + images * H * W * 3
    byte_ms = nbytes / (PEAK_HBM_GBPS * 1e9) * 1e3
    return dict(images=images, source=f"{src.dtype} {tuple(src.shape)}", us_per_image=round(t["ms"] / images * 1e3, 3),
                bytes_per_image=nbytes // images, byte_time_ms=round(byte_ms, 5), fraction_of_byte_time=round(byte_ms / t["ms"], 4),
                peak_hbm_gbps=PEAK_HBM_GBPS, **t)


def pil_round_trip_ms(a, reps=20):
    from PIL import Image

    def once():
        f = io.BytesIO()
        Image.fromarray(a).save(f, "JPEG")
        f.seek(0)
        return np.array(Image.open(f).convert("RGB"))
    once()
    t0 = time.perf_counter()
    for _ in range(reps):
        once()
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_roundtrip_bench.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    torch.set_grad_enabled(False)
    g = torch.Generator(device="cuda").manual_seed(0)
    res = header(card=True)
    res["setting"] = dict(quality=75, subsampling="4:2:0", height=H, width=W)
    u8 = torch.randint(0, 256, (64, H, W, 3), generator=g, device="cuda", dtype=torch.uint8)
    for n in (1, 16, 64):
        res[f"uint8_batch_{n}"] = case(u8[:n], n)
    f32 = torch.rand((64, 3, H, W), generator=g, device="cuda") * 2 - 1
    res["fp32_batch_64"] = case(f32, 64)
    del f32
    try:
        import PIL
        y, x = np.mgrid[0:H, 0:W]
        photo = np.clip(np.stack([128 + 100 * np.sin(x / 7.0 + c) * np.cos(y / 5.0 - c) for c in range(3)], -1)
                        + np.random.default_rng(0).normal(0, 12, (H, W, 3)), 0, 255).astype(np.uint8)
        res["pil_on_this_host"] = dict(version=PIL.__version__, one_core=True, photo_like_ms_per_image=round(pil_round_trip_ms(photo), 3),
                                       noise_ms_per_image=round(pil_round_trip_ms(u8[0].cpu().numpy()), 3))
    except ImportError:
        res["pil_on_this_host"] = None
    emit(res, a.out)


if __name__ == "__main__":
    main()

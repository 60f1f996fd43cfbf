"""Fixtures of the CLIP image preprocessing: tests/golden/imgproc_*.npz.

    python tests/golden/make_golden_image_processor.py

Runs the REAL third-party code on the seeded inputs of tests/helpers_image_processor.py -- ``PIL.Image.resize`` for every case,
``transformers.CLIPImageProcessor`` (its PIL backend) for every case with a crop, the grid cases' sheets included -- and records what they give:
the resized, cropped uint8 image, the real class's ``pixel_values`` for the small cases (for the 224-pixel cases the uint8 image plus
the table stand for the float planes, which would not fit a committed file), the real class's 3 x 256 table read off a 256-level ramp
image, a checksum of the inputs, and the Pillow / transformers versions.  Nothing of this project's code takes part in an output,
apart from ``evalio.image_grid`` / ``difashion.postprocess`` which build the sheet / quantise the fp32 source as the callers do."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import PIL                                                            # noqa: E402
import transformers                                                   # noqa: E402
from PIL import Image                                                 # noqa: E402
from transformers import CLIPImageProcessor                          # noqa: E402

from tests import helpers_image_processor as H                       # noqa: E402


def real_processor(edge, crop, resample):
    return CLIPImageProcessor(size={"shortest_edge": edge}, crop_size={"height": crop, "width": crop}, resample=resample)


def pil_resize_crop(img, edge, crop, resample):
    """PIL's resize to transformers' output size, then the floor-centred crop (crop 0: none)."""
    rh, rw = H.resized_size(img.shape[0], img.shape[1], edge)
    r = np.asarray(Image.fromarray(img).resize((rw, rh), resample))
    if crop == 0:
        return r
    top, left = (rh - crop) // 2, (rw - crop) // 2
    return np.ascontiguousarray(r[top:top + crop, left:left + crop])


def real_lut():
    """The real class's table: a 28 x 28 image holding every level in every channel goes through untouched by the resize."""
    ramp = (np.arange(28 * 28) % 256).astype(np.uint8).reshape(28, 28, 1).repeat(3, axis=2)
    px = real_processor(28, 28, 3)(images=[Image.fromarray(ramp)], return_tensors="np")["pixel_values"][0]
    lut = np.zeros((3, 256), np.float32)
    for c in range(3):
        lut[c][ramp[..., c].ravel()] = px[c].ravel()
    return lut


def main():
    versions = np.array([PIL.__version__, transformers.__version__])
    lut = real_lut()
    np.savez_compressed(os.path.join(H.GOLDEN, "imgproc_lut.npz"), lut=lut, versions=versions)
    for name, (B, h, w, edge, crop, resample, _, grid) in H.CASES.items():
        items = H.case_images(name)
        if grid:
            from difashion_amd.evalio import image_grid
            src = [np.asarray(image_grid([Image.fromarray(im) for im in items[b * grid:(b + 1) * grid]])) for b in range(B)]
        else:
            src = list(items)
        out = dict(u8=np.stack([pil_resize_crop(im, edge, crop, resample) for im in src]), checksum=H.checksum(items), versions=versions)
        if name in H.TRANSFORMERS_CASES:
            px = real_processor(edge, crop, resample)(images=[Image.fromarray(im) for im in src], return_tensors="np")["pixel_values"]
            assert px.dtype == np.float32 and np.array_equal(px, H.apply_lut(out["u8"], lut)), name      # resize + crop + table IS the class
            out["pixel_values"] = px
        np.savez_compressed(H.fixture_path(name), **out)
        print(name, out["u8"].shape, os.path.getsize(H.fixture_path(name)))
    # the fp32 source: difashion.postprocess(x, "pil"), then the real processor; the NaN is recorded as the 0 it has to become
    import torch
    from difashion_amd.difashion import postprocess
    x, nan_at = H.f32_source()
    B, h, w, edge, crop, resample = H.F32_CASE
    clean = x.copy()
    clean[nan_at] = -1.0
    pils = postprocess(torch.from_numpy(clean), "pil")
    px = real_processor(edge, crop, resample)(images=pils, return_tensors="np")["pixel_values"]
    u8 = np.stack([pil_resize_crop(np.asarray(p), edge, crop, resample) for p in pils])
    assert np.array_equal(px, H.apply_lut(u8, lut))
    np.savez_compressed(H.fixture_path("f32_source"), u8=u8, pixel_values=px, quantised=np.stack([np.asarray(p) for p in pils]),
                        checksum=H.checksum(x), versions=versions)
    print("f32_source", u8.shape, os.path.getsize(H.fixture_path("f32_source")))
    # fp32 items into sheets: postprocess, evalio.image_grid, the real processor
    from difashion_amd.evalio import image_grid
    xg = H.f32_grid_source()
    B, h, w, edge, crop, resample, grid = H.F32_GRID_CASE
    pils = postprocess(torch.from_numpy(xg), "pil")
    sheets = [image_grid(pils[b * grid:(b + 1) * grid]) for b in range(B)]
    px = real_processor(edge, crop, resample)(images=sheets, return_tensors="np")["pixel_values"]
    u8 = np.stack([pil_resize_crop(np.asarray(s), edge, crop, resample) for s in sheets])
    assert np.array_equal(px, H.apply_lut(u8, lut))
    np.savez_compressed(H.fixture_path("f32_grid3"), u8=u8, pixel_values=px, checksum=H.checksum(xg), versions=versions)
    print("f32_grid3", u8.shape, os.path.getsize(H.fixture_path("f32_grid3")))


if __name__ == "__main__":
    main()

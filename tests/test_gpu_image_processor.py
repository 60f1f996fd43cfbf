"""-m gpu: row f7 -- the CLIP image preprocessing kernel against what the REAL ``PIL.Image.resize`` and the REAL
``transformers.CLIPImageProcessor`` gave for the same seeded images (tests/golden/make_golden_image_processor.py).

Every comparison is BIT EQUALITY, on ``pixel_values`` and on the uint8 image in front of the lookup, and every case is run twice to show
the rerun is bit-identical.  The shapes are the smallest at which the kernel can go wrong: a non-integer ratio in both orientations
with a crop offset on either axis and a batch stride, an axis that is not resampled, no resampling at all, an upscale, a scale of 7.1
whose 31-tap halo exceeds the band, an image of only 0 / 255 pixels (the clipped intermediate), bilinear, the two sheet forms, the
fp32 source with ties / out-of-range values / a NaN, fp32 items into sheets, and the real sizes (512 -> 224 and the 1024 sheet: several bands, both tile edges).
The inputs are regenerated from the case's seed; the fixture's checksum proves they are the same bytes."""
import numpy as np
import pytest
import torch

import difashion_amd as da
from difashion_amd import _lib
from tests import helpers_image_processor as H
from tests.gpu_util import DEV

pytestmark = pytest.mark.gpu
LUT = H.load_fixture("lut")["lut"]


def processor(name):
    _, _, _, edge, crop, resample, _, _ = H.CASES[name]
    crop = crop or edge
    return da.CLIPImageProcessor(size={"shortest_edge": edge}, crop_size={"height": crop, "width": crop}, resample=resample)


def equal(tag, got, want):
    got = got.cpu().numpy()
    diff = int((got != want).sum()) if got.shape == want.shape else -1
    print(f"imgproc parity {tag}: shape {got.shape} differing {diff} of {want.size}")
    assert got.shape == want.shape and got.dtype == want.dtype and diff == 0, tag


@pytest.mark.parametrize("name", [n for n, c in H.CASES.items() if c[4]])
def test_pixel_values_and_uint8_equal_pil_and_transformers(name):
    grid = H.CASES[name][7]
    fx = H.load_fixture(name)
    items = H.case_images(name)
    assert fx["checksum"] == H.checksum(items)
    p = processor(name)
    src = torch.from_numpy(items).to(DEV)
    _lib.census_reset()
    px, u8 = p.preprocess_uint8(src, grid=grid or None)
    assert _lib.census()["imgproc"] == 1                                      # one launch a call
    equal(name + " uint8", u8, fx["u8"])
    equal(name + " pixel_values", px, fx["pixel_values"] if "pixel_values" in fx else H.apply_lut(fx["u8"], LUT))
    out = p(images=src, grid=grid or None)
    assert torch.equal(out.pixel_values, px) and torch.equal(out["pixel_values"], px)
    px2, u82 = p.preprocess_uint8(src, grid=grid or None)                     # the rerun is bit-identical
    assert torch.equal(px2, px) and torch.equal(u82, u8)
    assert px.device.type == "cuda" and px.dtype == torch.float32 and px.is_contiguous()


def test_resize_alone_bilinear_upscale():
    """29 x 29 -> 51 x 51 bilinear through ``resize``: the reference's Resize(512, BILINEAR) of the 291-pixel images in small."""
    name = "h29_w29_to_51_bilinear"
    fx = H.load_fixture(name)
    items = H.case_images(name)
    assert fx["checksum"] == H.checksum(items)
    p = da.CLIPImageProcessor()
    src = torch.from_numpy(items).to(DEV)
    u8 = p.resize(src, size=51, resample=2)
    equal(name, u8, fx["u8"])
    assert torch.equal(p.resize(src, size={"shortest_edge": 51}, resample=2), u8)


def test_fp32_source_equals_postprocess_then_the_processor():
    """A seeded tensor in [-1, 1], exact ties, values beyond +-1, infinities: ``postprocess(.., "pil")`` then the real processor.  The
    NaN quantises to 0 (the fixture was made with -1 in its place)."""
    x, nan_at = H.f32_source()
    fx = H.load_fixture("f32_source")
    assert fx["checksum"] == H.checksum(x)
    _, _, _, edge, crop, resample = H.F32_CASE
    p = da.CLIPImageProcessor(size={"shortest_edge": edge}, crop_size={"height": crop, "width": crop}, resample=resample)
    src = torch.from_numpy(x).to(DEV)
    px, u8 = p.preprocess_uint8(src)
    equal("f32_source uint8", u8, fx["u8"])
    equal("f32_source pixel_values", px, fx["pixel_values"])
    # the quantisation on its own, every pixel: a resize to the source's own size is the identity
    q = da.CLIPImageProcessor().resize(src, size=min(x.shape[2:]))
    equal("f32_source quantised", q, fx["quantised"])
    b, c, yy, xx = nan_at
    assert int(q[b, yy, xx, c]) == 0
    px2, u82 = p.preprocess_uint8(src)
    assert torch.equal(px2, px) and torch.equal(u82, u8)


def test_fp32_items_into_sheets_equal_postprocess_image_grid_and_the_processor():
    """The fp32 source together with ``grid=3`` (what ``sample_outfits(output_type="image")`` sheets are): the fetch resolves the cell of
    every float it quantises, the fourth cell is white."""
    x = H.f32_grid_source()
    fx = H.load_fixture("f32_grid3")
    assert fx["checksum"] == H.checksum(x)
    _, _, _, edge, crop, resample, grid = H.F32_GRID_CASE
    p = da.CLIPImageProcessor(size={"shortest_edge": edge}, crop_size={"height": crop, "width": crop}, resample=resample)
    src = torch.from_numpy(x).to(DEV)
    px, u8 = p.preprocess_uint8(src, grid=grid)
    equal("f32_grid3 uint8", u8, fx["u8"])
    equal("f32_grid3 pixel_values", px, fx["pixel_values"])
    px2, u82 = p.preprocess_uint8(src, grid=grid)
    assert torch.equal(px2, px) and torch.equal(u82, u8)


def test_a_list_of_two_sizes_comes_back_in_input_order():
    from PIL import Image
    a, b = H.case_images("h61_w40"), H.case_images("h40_w61")
    fa, fb = H.load_fixture("h61_w40"), H.load_fixture("h40_w61")
    order = [("a", 0), ("b", 0), ("a", 1), ("b", 1), ("b", 2), ("a", 2)]
    images = [Image.fromarray((a if s == "a" else b)[i]) for s, i in order]
    images[1] = np.asarray(images[1])                                         # numpy arrays and PIL images mix
    p = processor("h61_w40")
    _lib.census_reset()
    px = p(images=images, return_tensors="pt", device=DEV).pixel_values
    assert _lib.census()["imgproc"] == 2                                      # one launch a size group
    want = np.stack([(fa if s == "a" else fb)["pixel_values"][i] for s, i in order])
    equal("size groups", px, want)


def test_extract_image_features_equals_encode_image_of_the_processor_output():
    from tests.helpers_clip_vision import case_inputs
    cfg, params, _ = case_inputs("tiny_quickgelu")
    m = da.CLIPVisionModelWithProjection(**cfg.kwargs(), init_seed=None)
    m.load_state_dict(params)
    m = m.to(DEV).eval().requires_grad_(False)
    S = cfg.image_size
    p = da.CLIPImageProcessor(size={"shortest_edge": S}, crop_size={"height": S, "width": S})
    images = torch.from_numpy(np.random.default_rng(5).integers(0, 256, (5, 70, 90, 3)).astype(np.uint8)).to(DEV)
    feats = da.extract_image_features(m, p, images, batch_size=2)
    want = m.encode_image(p(images=images).pixel_values)
    assert feats.shape == (5, cfg.projection_dim) and feats.device.type == "cuda"
    # a row of the tower does not depend on the batch it rides in, so 2 + 2 + 1 images give the bits of 5
    assert torch.equal(feats, want)
    from PIL import Image
    pils = [Image.fromarray(im) for im in images.cpu().numpy()]
    assert torch.equal(da.extract_image_features(m, p, pils, batch_size=2), want)

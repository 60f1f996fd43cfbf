"""A numpy restatement of the CLIP image preprocessing and the cases its tests share.

The restatement is PIL's 8-bit resize as Pillow's Resample.c does it -- coefficient tables in double, 22-bit integer coefficients, a
horizontal pass, then a vertical pass, the intermediate image clipped to uint8 -- followed by transformers' floor-centred crop and a
3 x 256 fp32 lookup.  It is written from that description, apart from the library, and is held to the REAL PIL / transformers by
the fixtures of tests/golden/make_golden_image_processor.py (and live, where they import)."""
import math
import os
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
OPENAI_CLIP_MEAN = [0.48145466, 0.4578275, 0.40821073]
OPENAI_CLIP_STD = [0.26862954, 0.26130258, 0.27577711]
BICUBIC, BILINEAR = 3, 2
PRECISION_BITS = 22


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


FILTERS = {BICUBIC: (_bicubic, 2.0), BILINEAR: (_bilinear, 1.0)}


def coefficients(in_size, out_size, resample):
    """-> (bounds int32 [out][2] = (first tap, tap count), coef int32 [out][ksize]) of one axis."""
    filt, fsupport = FILTERS[resample]
    scale = in_size / out_size
    fs = max(scale, 1.0)
    support = fsupport * fs
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), np.int32)
    coef = np.zeros((out_size, ksize), np.int32)
    ss = 1.0 / fs
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(0, int(center - support + 0.5))
        xmax = min(in_size, int(center + support + 0.5)) - xmin
        w = [filt((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        bounds[xx] = (xmin, xmax)
        for x, v in enumerate(w):
            coef[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
    return bounds, coef


def _pass(img, bounds, coef):
    """One pass along axis 1 of uint8 [H][W][C]: clip8((2^21 + sum pixel * k) >> 22) in 32-bit integers."""
    H, _, C = img.shape
    out = np.empty((H, len(bounds), C), np.uint8)
    src = img.astype(np.int64)
    for xx, (xmin, xmax) in enumerate(bounds):
        acc = (1 << (PRECISION_BITS - 1)) + np.tensordot(src[:, xmin:xmin + xmax, :], coef[xx, :xmax].astype(np.int64), axes=([1], [0]))
        assert np.abs(acc).max() < 2 ** 31
        out[:, xx, :] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def pil_resize(img, out_h, out_w, resample):
    """PIL.Image.resize((out_w, out_h), resample) of a uint8 [H][W][3] array."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    H, W, _ = img.shape
    if out_w != W:
        img = _pass(img, *coefficients(W, out_w, resample))
    if out_h != H:
        img = _pass(img.transpose(1, 0, 2), *coefficients(H, out_h, resample)).transpose(1, 0, 2)
    return np.ascontiguousarray(img)


def resized_size(h, w, shortest_edge):
    """transformers' get_resize_output_image_size(default_to_square=False): the short edge to shortest_edge, the other truncated."""
    short, long = (w, h) if w <= h else (h, w)
    new_short, new_long = shortest_edge, int(shortest_edge * long / short)
    return (new_long, new_short) if w <= h else (new_short, new_long)


def geometry(h, w, shortest_edge, crop_h, crop_w):
    rh, rw = resized_size(h, w, shortest_edge)
    return rh, rw, (rh - crop_h) // 2, (rw - crop_w) // 2


def lookup_table(mean=OPENAI_CLIP_MEAN, std=OPENAI_CLIP_STD):
    """3 x 256 fp32: ToTensor + Normalize in fp32, (v / 255 - mean) / std."""
    v = np.arange(256, dtype=np.float32) / np.float32(255)
    return np.stack([(v - np.float32(m)) / np.float32(s) for m, s in zip(mean, std)]).astype(np.float32)


def preprocess_u8(img, shortest_edge=224, crop_h=224, crop_w=224, resample=BICUBIC):
    """Resize + centre crop of one uint8 [H][W][3] image -> uint8 [crop_h][crop_w][3]."""
    rh, rw, top, left = geometry(img.shape[0], img.shape[1], shortest_edge, crop_h, crop_w)
    assert top >= 0 and left >= 0
    r = pil_resize(img, rh, rw, resample)
    return np.ascontiguousarray(r[top:top + crop_h, left:left + crop_w])


def apply_lut(u8, lut):
    """uint8 [..][h][w][3] -> fp32 [..][3][h][w]."""
    planes = [lut[c][u8[..., c]] for c in range(3)]
    return np.stack(planes, axis=-3).astype(np.float32)


def image_grid(items, n):
    """evalio.image_grid / the reference's merge_images on arrays: uint8 [n][h][w][3] -> the ceil(sqrt n)^2 sheet, white where empty."""
    g = int(math.ceil(math.sqrt(n)))
    h, w = items.shape[1:3]
    sheet = np.full((g * h, g * w, 3), 255, np.uint8)
    for i in range(n):
        r, c = divmod(i, g)
        sheet[r * h:(r + 1) * h, c * w:(c + 1) * w] = items[i]
    return sheet


def quantise(x):
    """difashion.postprocess(x, "pil") on an fp32 [B][3][H][W] array in [-1, 1] -> uint8 [B][H][W][3]; fp32 arithmetic, half to even."""
    x = np.asarray(x, np.float32)
    y = np.clip(x / np.float32(2) + np.float32(0.5), np.float32(0), np.float32(1))
    return np.rint(y * np.float32(255)).astype(np.uint8).transpose(0, 2, 3, 1)


# ---- the cases.  name: (batch, H, W, shortest_edge, crop, resample, kind of pixels, grid).  H x W is numpy's order (rows, columns).
CASES = {
    "h61_w40": (3, 61, 40, 28, 28, BICUBIC, "noise", 0),
    "h40_w61": (3, 40, 61, 28, 28, BICUBIC, "noise", 0),
    "h45_w28": (1, 45, 28, 28, 28, BICUBIC, "noise", 0),
    "h28_w45": (1, 28, 45, 28, 28, BICUBIC, "noise", 0),
    "h28_w28": (2, 28, 28, 28, 28, BICUBIC, "noise", 0),
    "h31_w20": (1, 31, 20, 28, 28, BICUBIC, "noise", 0),
    "h200_w300": (1, 200, 300, 28, 28, BICUBIC, "noise", 0),
    "h300_w200": (1, 300, 200, 28, 28, BICUBIC, "noise", 0),
    "h53_w37_binary": (1, 53, 37, 28, 28, BICUBIC, "binary", 0),
    "h61_w40_bilinear": (3, 61, 40, 28, 28, BILINEAR, "noise", 0),
    "h29_w29_to_51_bilinear": (2, 29, 29, 51, 0, BILINEAR, "noise", 0),
    "grid3_24": (2, 24, 24, 28, 28, BICUBIC, "noise", 3),
    "grid4_24": (2, 24, 24, 28, 28, BICUBIC, "noise", 4),
    "h512_w512": (2, 512, 512, 224, 224, BICUBIC, "smooth", 0),
    "grid4_512": (1, 512, 512, 224, 224, BICUBIC, "smooth", 4),
}
# what transformers' own processor is run on when the fixtures are made: every case with a crop whose float planes fit a committed
# file (the two 224-pixel cases keep the uint8 image plus the table instead), the sheets of the grid cases included
TRANSFORMERS_CASES = [n for n, c in CASES.items() if c[4] == 28]
F32_CASE = (3, 40, 61, 28, 28, BICUBIC)
F32_GRID_CASE = (2, 24, 24, 28, 28, BICUBIC, 3)                 # batch, H, W, shortest edge, crop, resample, grid: fp32 items into sheets


def case_images(name):
    """Seeded uint8 [items][H][W][3] of a case (items = batch * max(grid, 1)); regenerated everywhere, the fixture keeps a checksum."""
    B, H, W, _, _, _, kind, grid = CASES[name]
    n = B * max(grid, 1)
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    if kind == "binary":
        return (rng.integers(0, 2, (n, H, W, 3)) * 255).astype(np.uint8)
    if kind == "smooth":                                    # a gradient plus noise plus saturated patches: compresses in the fixture's output
        yy, xx = np.mgrid[0:H, 0:W]
        base = np.stack([(xx * 255 // max(W - 1, 1)), (yy * 255 // max(H - 1, 1)), ((xx + yy) % 256)], -1)[None].astype(np.int64)
        img = base + rng.integers(-40, 41, (n, H, W, 3))
        img[:, H // 4:H // 4 + 9, :, :] = 255
        img[:, :, W // 3:W // 3 + 7, :] = 0
        return np.clip(img, 0, 255).astype(np.uint8)
    return rng.integers(0, 256, (n, H, W, 3)).astype(np.uint8)


def f32_source():
    """The fp32 source case: a seeded tensor in [-1, 1] with exact ties ((k + 0.5) / 255) * 2 - 1, values beyond +-1 and one NaN.
    -> (x fp32 [3][3][40][61], (b, c, y, x) of the NaN)."""
    B, H, W = F32_CASE[:3]
    rng = np.random.default_rng(77)
    x = rng.uniform(-1, 1, (B, 3, H, W)).astype(np.float32)
    k = np.arange(255, dtype=np.float32)
    x[0, 0].reshape(-1)[:255] = ((k + np.float32(0.5)) / np.float32(255)) * np.float32(2) - np.float32(1)
    x[1, 1, 3, :20] = np.linspace(1.0, 3.0, 20, dtype=np.float32)
    x[1, 2, 5, :20] = np.linspace(-1.0, -3.0, 20, dtype=np.float32)
    x[1, 0, 7, 0], x[1, 0, 7, 1] = np.inf, -np.inf
    nan_at = (2, 1, 20, 30)
    x[nan_at] = np.nan
    return x, nan_at


def f32_grid_source():
    """The fp32 items of the fp32 sheet case: seeded in [-1.2, 1.2] (some beyond +-1) -> fp32 [6][3][24][24]."""
    B, H, W, _, _, _, grid = F32_GRID_CASE
    return np.random.default_rng(78).uniform(-1.2, 1.2, (B * grid, 3, H, W)).astype(np.float32)


def case_source(name):
    """-> uint8 [B][Hs][Ws][3]: the images the processor resizes (the sheets, for a grid case)."""
    B, _, _, _, _, _, _, grid = CASES[name]
    items = case_images(name)
    if not grid:
        return items
    return np.stack([image_grid(items[b * grid:(b + 1) * grid], grid) for b in range(B)])


def case_expected(name):
    """The restatement's uint8 output [B][out_h][out_w][3] of a case."""
    _, _, _, edge, crop, resample, _, _ = CASES[name]
    src = case_source(name)
    if crop == 0:
        rh, rw = resized_size(src.shape[1], src.shape[2], edge)
        return np.stack([pil_resize(im, rh, rw, resample) for im in src])
    return np.stack([preprocess_u8(im, edge, crop, crop, resample) for im in src])


def checksum(arr):
    return np.uint32(zlib.crc32(np.ascontiguousarray(arr).tobytes()))


def fixture_path(name):
    return os.path.join(GOLDEN, f"imgproc_{name}.npz")


def load_fixture(name):
    with np.load(fixture_path(name)) as z:
        return {k: z[k] for k in z.files}

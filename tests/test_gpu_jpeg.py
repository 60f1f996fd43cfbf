"""-m gpu: row f10 -- the JPEG save / open round trip on the device against the numpy restatement of tests/helpers_jpeg.py
(which tests/test_jpeg_cpu.py holds to the real PIL) and, for one case, against a real file written and read the way the reference does.

Every comparison is BIT EQUALITY, on the pixels and on the quantised coefficients (which tell an encode error from a decode error).  The
shapes are the smallest at which the kernels can go wrong: 1 x 1 (a lone partial MCU), exactly one MCU (16 x 16 at 4:2:0, 8 x 8 at
4:4:4), odd in both axes (17 x 23, 31 x 33: the last-column rule of the upsampler), an even height that is no multiple of 16 (30 x 46:
the bottom-padding rule of the chroma planes), 100 x 75 (two tile columns, a width that is no multiple of 4: the byte-store kernel) and
one 512 x 512 (the real size: many tiles, the four-pixel kernel)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import difashion_amd as da
from tests import helpers_jpeg as H
from tests.gpu_util import DEV, release_cached_gpu_memory

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [(1, 1), (8, 8), (16, 16), (17, 23), (31, 33), (30, 46), (100, 75)] + H.EXTRA_SIZES


def check(tag, images, kinds, h, w, quality, subsampling):
    src = torch.from_numpy(images).to(DEV)
    before = src.clone()
    px, coef = da.jpeg_roundtrip(src, quality, subsampling, return_coefficients=True)
    assert px.shape == (len(kinds), h, w, 3) and px.dtype == torch.uint8 and px.device.type == "cuda" and px.is_contiguous()
    assert torch.equal(src, before), tag                                      # the source is not written
    px, coef = px.cpu().numpy(), coef.cpu().numpy()
    for i, kind in enumerate(kinds):
        want_px, want_coef = H.expected(kind, h, w, quality, subsampling)
        dc, dp = int((coef[i] != want_coef).sum()) if coef[i].shape == want_coef.shape else -1, int((px[i] != want_px).sum())
        print(f"jpeg parity {tag} {kind}: coefficients differing {dc} of {want_coef.size}, pixels differing {dp} of {want_px.size}")
        assert dc == 0, (tag, kind, "coefficients: the encode half")
        assert dp == 0, (tag, kind, "pixels")
    return src, px


@pytest.mark.parametrize("size", SMALL, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pixels_and_coefficients_equal_the_restatement(size):
    h, w = size
    images = np.stack([H.case_image(kind, h, w) for kind in H.KINDS])
    for setting in H.SETTINGS:
        src, px = check(f"{h}x{w} {H.setting_id(setting)}", images, H.KINDS, h, w, *setting)
    again = da.jpeg_roundtrip(src, *H.SETTINGS[-1])                            # the rerun is bit-identical, with and without coefficients
    assert np.array_equal(again.cpu().numpy(), px)


def test_512_square():
    kinds = ("smooth", "checker")
    images = np.stack([H.case_image(kind, 512, 512) for kind in kinds])
    for setting in ((75, "4:2:0"), (90, "4:4:4")):
        check(f"512x512 {H.setting_id(setting)}", images, kinds, 512, 512, *setting)


def test_a_real_file_saved_and_opened_the_way_the_reference_does(tmp_path):
    """``img.save("0.jpg")`` / ``Image.open`` (inf4eval.py:787-790, evaluate_gor.py:207-215; evalio.save_batch_outputs writes the same way)."""
    from PIL import Image
    a = H.case_image("smooth", 100, 75)
    Image.fromarray(a).save(str(tmp_path / "0.jpg"))
    want = np.array(Image.open(str(tmp_path / "0.jpg")).convert("RGB"))
    got = da.jpeg_roundtrip(torch.from_numpy(a)[None].to(DEV))[0].cpu().numpy()
    assert got.shape == want.shape and int((got != want).sum()) == 0


def test_a_batch_equals_the_single_calls():
    h, w = 30, 46
    images = [torch.from_numpy(H.case_image(kind, h, w)).to(DEV) for kind in H.KINDS] + [torch.from_numpy(H.case_image("noise", w, h)).to(DEV).transpose(0, 1)]
    assert len(images) == 5
    px, coef = da.jpeg_roundtrip(images, return_coefficients=True)            # a list of same-size tensors, the last one not contiguous
    for i, im in enumerate(images):
        one_px, one_coef = da.jpeg_roundtrip(im[None], return_coefficients=True)
        assert torch.equal(px[i], one_px[0]) and torch.equal(coef[i], one_coef[0]), i
    stacked = torch.stack(images)
    part = stacked[1:4]                                                       # a contiguous slice off the 16-byte grid: re-based by the wrapper
    assert part.is_contiguous() and part.data_ptr() % 16 != 0
    assert torch.equal(da.jpeg_roundtrip(part), px[1:4])
    sl = da.jpeg_roundtrip(stacked[1:4, 1:, 1:])                              # a strided view
    for i in range(3):
        assert np.array_equal(sl[i].cpu().numpy(), H.roundtrip(images[i + 1][1:, 1:].cpu().numpy())[0])


def f32_case():
    """fp32 [2, 3, 17, 23] in [-1, 1] with exact ties, values beyond +-1, infinities and a NaN -> (x, the uint8 source of
    ``difashion.postprocess(.., "pil")`` with -1 in the NaN's place: a NaN quantises to 0)."""
    from difashion_amd.difashion import postprocess
    rng = np.random.default_rng(79)
    x = rng.uniform(-1, 1, (2, 3, 17, 23)).astype(np.float32)
    k = np.arange(255, dtype=np.float32)
    x[0, 0].reshape(-1)[:255] = ((k + np.float32(0.5)) / np.float32(255)) * np.float32(2) - np.float32(1)
    x[1, 1, 3, :20] = np.linspace(1.0, 3.0, 20, dtype=np.float32)
    x[1, 2, 5, :20] = np.linspace(-1.0, -3.0, 20, dtype=np.float32)
    x[1, 0, 7, 0], x[1, 0, 7, 1] = np.inf, -np.inf
    clean = x.copy()
    x[1, 1, 10, 11] = np.nan
    clean[1, 1, 10, 11] = -1.0
    u8 = np.stack([np.asarray(im) for im in postprocess(torch.from_numpy(clean), "pil")])
    return x, u8


def test_fp32_source_equals_postprocess_then_the_round_trip():
    x, u8 = f32_case()
    assert u8[1, 10, 11, 1] == 0 and u8.max() == 255
    src = torch.from_numpy(x).to(DEV)
    before = src.clone()
    for setting in ((75, "4:2:0"), (90, "4:4:4")):
        got, gcoef = da.jpeg_roundtrip(src, *setting, return_coefficients=True)
        want, wcoef = da.jpeg_roundtrip(torch.from_numpy(u8).to(DEV), *setting, return_coefficients=True)
        assert torch.equal(gcoef, wcoef) and torch.equal(got, want), setting
        for i in range(2):
            assert np.array_equal(got[i].cpu().numpy(), H.roundtrip(u8[i], *setting)[0]), setting
    assert torch.equal(src.view(torch.int32), before.view(torch.int32))       # bits: the NaN stays where it was


def test_round_trip_feeds_the_image_processor():
    """The result is the uint8 [B, H, W, 3] form the evaluation rows take."""
    a = np.stack([H.case_image("smooth", 64, 64), H.case_image("noise", 64, 64)])
    rt = da.jpeg_roundtrip(torch.from_numpy(a).to(DEV))
    p = da.CLIPImageProcessor(size={"shortest_edge": 32}, crop_size={"height": 32, "width": 32})
    want = p(images=torch.from_numpy(np.stack([H.expected(k, 64, 64, 75, "4:2:0")[0] for k in ("smooth", "noise")])).to(DEV)).pixel_values
    assert torch.equal(p(images=rt).pixel_values, want)


def test_fp16_storage_library_gives_the_same_bits():
    """The kernels are integer only: libdifashion_hip_f16.so, in a fresh process of its own, gives the bits of the bf16 build."""
    from tests.jpeg_fp16_child import case
    want = case(DEV)
    release_cached_gpu_memory()
    env = dict(os.environ, DFH_STORAGE="fp16")
    env.pop("DFH_LIB", None)
    r = subprocess.run([sys.executable, "-m", "tests.jpeg_fp16_child"], capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("JPEG_FP16_RESULT ")]
    assert line, r.stdout[-2000:]
    res = json.loads(line[-1][len("JPEG_FP16_RESULT "):])
    assert res["storage"] == "fp16" and "storage=fp16" in res["build_info"]
    assert res["digests"] == want

"""CPU (-m "not gpu"): row f10, the JPEG save / open round trip -- everything that needs no GPU.

The numpy restatement of tests/helpers_jpeg.py is what the GPU tests hold the kernels to, so it is held here to the installed PIL, bit
for bit, over the whole case list, and to a fixture PIL wrote (so the contract survives a PIL upgrade); run in wrapping int32 it equals
its int64 form on the widest inputs, which licenses 32-bit integers in the kernel.  The library's quantisation tables equal the ones
PIL's files carry at every quality, and every refusal of the C ABI is raised on the host, through ctypes, without a GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import difashion_amd as da
from difashion_amd import _lib
from tests import helpers_jpeg as H


def _need_turbo():
    from PIL import features
    if not features.check_feature("libjpeg_turbo"):
        pytest.skip("PIL is not built on libjpeg-turbo here: bit parity is stated against libjpeg-turbo's islow path")


@pytest.mark.parametrize("size", H.SIZES + H.EXTRA_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_restatement_equals_installed_pil(size):
    _need_turbo()
    h, w = size
    for kind in H.KINDS:
        a = H.case_image(kind, h, w)
        for quality, subsampling in H.SETTINGS:
            got, want = H.roundtrip(a, quality, subsampling)[0], H.pil_roundtrip(a, quality, subsampling)
            diff = int((got != want).sum())
            assert got.shape == want.shape and diff == 0, (kind, size, quality, subsampling, diff)


def test_default_arguments_are_what_pil_saves_by_default():
    """``img.save("0.jpg")`` without arguments (the reference's call) is quality 75, 4:2:0."""
    _need_turbo()
    import io
    from PIL import Image
    a = H.case_image("smooth", 31, 33)
    f = io.BytesIO()
    Image.fromarray(a).save(f, "JPEG")
    f.seek(0)
    assert np.array_equal(np.array(Image.open(f).convert("RGB")), H.roundtrip(a)[0])


def test_library_quant_tables_equal_the_tables_of_pil_files_at_every_quality():
    for quality in range(1, 101):
        luma, chroma = da.jpeg_quant_tables(quality)
        want_l, want_c = H.pil_quant_tables(quality)
        assert luma.shape == (8, 8) and np.array_equal(luma, want_l) and np.array_equal(chroma, want_c), quality
        rl, rc = H.quant_tables(quality)
        assert np.array_equal(luma, rl) and np.array_equal(chroma, rc), quality


@pytest.mark.parametrize("setting", [(1, "4:2:0"), (100, "4:4:4"), (1, "4:4:4"), (100, "4:2:0")], ids=H.setting_id)
def test_int32_restatement_equals_int64(setting):
    """The one-pixel checkerboard drives the DCT to its widest values, quality 100 (q = 1) keeps them through the inverse, quality 1
    (q = 255) makes the widest products of the dequantisation."""
    for h, w in ((17, 23), (64, 64)):
        for kind in ("checker", "noise"):
            a = H.case_image(kind, h, w)
            p64, c64 = H.roundtrip(a, *setting)
            p32, c32 = H.roundtrip(a, *setting, dtype=np.int32)
            assert np.array_equal(p64, p32) and np.array_equal(c64, c32), (kind, h, w)


def test_restatement_equals_the_golden_file():
    z = np.load(H.GOLDEN)
    n = 0
    for case in H.golden_cases():
        kind, h, w, quality, subsampling = case
        key = H.golden_key(*case)
        a = H.case_image(kind, h, w)
        assert str(z[key + "_input_sha256"]) == H.checksum(a), key             # the regenerated input is the fixture's input
        assert np.array_equal(H.expected(*case)[0], z[key]), key
        n += 1
    assert n == len([k for k in z.files if k.endswith("_input_sha256")]) and n >= 150


def _call(**over):
    """dfh_jpeg_roundtrip with made-up addresses: every refusal comes before any HIP call."""
    args = dict(src=1 << 20, src_kind=0, batch=2, h=17, w=23, quality=75, subsampling=2, dst=2 << 20, coef=3 << 20, ws=4 << 20, ws_bytes=None)
    args.update(over)
    if args["ws_bytes"] is None:
        args["ws_bytes"] = _lib.raw().dfh_jpeg_workspace_bytes(2, 17, 23, 2)
    return _lib.call("dfh_jpeg_roundtrip", C.c_void_p(args["src"]), args["src_kind"], args["batch"], args["h"], args["w"], args["quality"],
                     args["subsampling"], C.c_void_p(args["dst"]), C.c_void_p(args["coef"]), C.c_void_p(args["ws"]), args["ws_bytes"], None)


@pytest.mark.parametrize("over,message", [
    (dict(quality=0), "quality must be in"), (dict(quality=101), "quality must be in"),
    (dict(subsampling=1), "4:2:2"), (dict(subsampling=3), "subsampling must be"),
    (dict(h=0), "must be positive"), (dict(w=0), "must be positive"), (dict(batch=0), "must be positive"), (dict(w=-4), "must be positive"),
    (dict(src=0), "null argument"), (dict(dst=0), "null argument"), (dict(ws=0), "null argument"),
    (dict(src=(1 << 20) + 4), "16-byte aligned"), (dict(dst=(2 << 20) + 8), "16-byte aligned"), (dict(coef=(3 << 20) + 2), "16-byte aligned"),
    (dict(ws=(4 << 20) + 1), "16-byte aligned"),
    (dict(src_kind=2), "src_kind"),
    (dict(ws_bytes=100), "workspace smaller than dfh_jpeg_workspace_bytes"),
    (dict(dst=(1 << 20) + 16), "dst_hwc overlaps src"), (dict(dst=(1 << 20) - 16), "dst_hwc overlaps src"),
    (dict(ws=(1 << 20) + 32), "workspace overlaps"),
], ids=lambda v: "-".join(f"{k}={x}" for k, x in v.items()) if isinstance(v, dict) else None)
def test_guards_refuse_on_the_host_before_any_launch(over, message):
    with pytest.raises(_lib.DfhError, match=message):
        _call(**over)
    assert message.split()[0] in _lib.last_error()


def test_size_queries_and_quant_table_guards():
    lib = _lib.raw()
    # 17 x 23 at 4:2:0: two 16-row tiles of one 64-wide tile column: Y 32 x 64 + 2 x 16 x 32; at 4:4:4: three 8-row tiles, 3 x 24 x 64
    assert lib.dfh_jpeg_workspace_bytes(2, 17, 23, 2) == 2 * (32 * 64 + 2 * 16 * 32)
    assert lib.dfh_jpeg_workspace_bytes(1, 17, 23, 0) == 3 * 24 * 64
    assert lib.dfh_jpeg_coef_count(2, 17, 23, 2) == 2 * 64 * (3 * 3 + 2 * 2 * 2)
    assert lib.dfh_jpeg_coef_count(1, 17, 23, 0) == 64 * 3 * 9
    assert lib.dfh_jpeg_workspace_bytes(1, 17, 23, 1) == 0 and "subsampling" in _lib.last_error()
    assert lib.dfh_jpeg_workspace_bytes(0, 17, 23, 2) == 0 and lib.dfh_jpeg_coef_count(1, 0, 23, 2) == 0
    buf = (C.c_int * 64)()
    for q in (0, 101, -3):
        with pytest.raises(_lib.DfhError, match="quality must be in"):
            _lib.call("dfh_jpeg_quant_tables", q, buf, buf)
    with pytest.raises(_lib.DfhError, match="null argument"):
        _lib.call("dfh_jpeg_quant_tables", 75, None, buf)


def test_python_entry_refuses_cpu_tensors_and_other_subsamplings():
    x = torch.zeros(1, 8, 8, 3, dtype=torch.uint8)
    with pytest.raises(da.DfhError, match="no CPU fallback"):
        da.jpeg_roundtrip(x)
    with pytest.raises(da.DfhError, match="no CPU fallback"):
        da.jpeg_roundtrip([x[0], x[0]])
    for sub in ("4:2:2", 1, "4:1:1"):
        with pytest.raises(ValueError, match="is not built"):
            da.jpeg_roundtrip(x, subsampling=sub)
    with pytest.raises(ValueError, match="subsampling must be"):
        da.jpeg_roundtrip(x, subsampling="420")
    for q in (0, 101, 7.5):
        with pytest.raises(ValueError, match="quality"):
            da.jpeg_roundtrip(x, quality=q)
    with pytest.raises(ValueError, match="one size"):
        da.jpeg_roundtrip([x[0], torch.zeros(9, 8, 3, dtype=torch.uint8)])
    with pytest.raises(ValueError, match="no image"):
        da.jpeg_roundtrip([])
    assert "jpeg_roundtrip" in da.__all__ and "jpeg_quant_tables" in da.__all__

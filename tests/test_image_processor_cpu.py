"""CPU tier (-m "not gpu"): the host-only half of the CLIP image preprocessing -- the C ABI of the ``dfh_imgproc_*``
family in all three places (header, both libraries, ctypes), the library's coefficient tables and geometry against the numpy
restatement of tests/helpers_image_processor.py, the restatement against the fixtures the REAL ``PIL.Image.resize`` /
``transformers.CLIPImageProcessor`` produced (and against them live, where they import), refusals, the checkpoint file, and a
sanitizer run of the plan as a stand-alone program.  No compute call is made here; the kernel is held to the same fixtures on the GPU
(tests/test_gpu_image_processor.py).  Every comparison is bit equality."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import difashion_amd as da
from difashion_amd import _lib
from tests import helpers_image_processor as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILY = ["dfh_imgproc_create", "dfh_imgproc_destroy", "dfh_imgproc_resized_height", "dfh_imgproc_resized_width", "dfh_imgproc_out_height",
          "dfh_imgproc_out_width", "dfh_imgproc_crop_top", "dfh_imgproc_crop_left", "dfh_imgproc_ksize_x", "dfh_imgproc_ksize_y",
          "dfh_imgproc_table_bytes", "dfh_imgproc_fill_tables", "dfh_imgproc_run"]
# (in_h, in_w, shortest_edge, crop, resample, grid): every fixture shape, the shapes the restatement was first checked on, both filters
SHAPES = sorted({(h, w, e, c, r, g) for (_, h, w, e, c, r, _, g) in H.CASES.values()} | {H.F32_CASE[1:] + (0,)} |
                {(h, w, e, c, r, 0) for (h, w, e, c) in [(512, 512, 224, 224), (1024, 1024, 224, 224), (291, 291, 224, 224), (200, 300, 224, 224),
                                                          (53, 37, 28, 28), (31, 20, 28, 28), (7, 5, 28, 28), (224, 224, 224, 224),
                                                          (291, 291, 512, 0)] for r in (2, 3)})


def plan(h, w, edge, crop, resample, grid=0):
    handle = C.c_void_p()
    _lib.call("dfh_imgproc_create", C.byref(_lib.ImgProcConfigC(edge, crop, crop, resample)), h, w, grid, C.byref(handle))
    return handle


def test_every_imgproc_symbol_is_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "difashion_hip.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(dfh_imgproc_[a-z0-9_]+)\s*\(", src)) == set(FAMILY)
    assert "#define DFH_ABI_VERSION 8" in src
    for lib_name in _lib._LIB_NAMES.values():                                   # both storage builds export the row
        lib = C.CDLL(os.path.join(_lib.CSRC, lib_name))
        for n in FAMILY:
            assert hasattr(lib, n), f"{n} not exported by {lib_name}"
    for n in FAMILY:
        assert n in _lib.SIGNATURES, n
    body = re.search(r"typedef struct dfh_imgproc_config \{(.*?)\} dfh_imgproc_config;", src, flags=re.S).group(1)
    fields = [re.sub(r"^int\s+", "", d.strip()) for d in body.split(";") if d.strip()]
    assert fields == [f[0] for f in _lib.ImgProcConfigC._fields_] and C.sizeof(_lib.ImgProcConfigC) == 16
    assert "imgproc" in _lib.census()
    mk = open(os.path.join(_lib.CSRC, "Makefile")).read()
    assert "image_processor.hip" in mk and re.search(r"image_processor\.o:.*\n\t.*-ffp-contract=off", mk)
    text = open(os.path.join(_lib.CSRC, "image_processor.hip")).read()
    assert not re.search(r"\b(bf16_t|h16x8_t|DFH_F16|pack2bf|f2bf|atomic[A-Z]\w*|__hip_atomic\w*|getenv)\b", text)      # one source, integers and fp32, no atomics


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_tables_and_geometry_equal_the_restatement(shape):
    h, w, edge, crop, resample, grid = shape
    lib, p = _lib.raw(), plan(*shape)
    try:
        g = int(np.ceil(np.sqrt(max(grid, 1))))
        sh, sw = g * h, g * w
        rh, rw = H.resized_size(sh, sw, edge)
        assert (lib.dfh_imgproc_resized_height(p), lib.dfh_imgproc_resized_width(p)) == (rh, rw)
        oh, ow = (crop, crop) if crop else (rh, rw)
        assert (lib.dfh_imgproc_out_height(p), lib.dfh_imgproc_out_width(p)) == (oh, ow)
        assert (lib.dfh_imgproc_crop_top(p), lib.dfh_imgproc_crop_left(p)) == ((rh - oh) // 2, (rw - ow) // 2)
        bx, cx = H.coefficients(sw, rw, resample)
        by, cy = H.coefficients(sh, rh, resample)
        assert (lib.dfh_imgproc_ksize_x(p), lib.dfh_imgproc_ksize_y(p)) == (cx.shape[1], cy.shape[1])
        want = np.concatenate([bx.ravel(), cx.ravel(), by.ravel(), cy.ravel()])
        nbytes = lib.dfh_imgproc_table_bytes(p)
        assert nbytes == (want.size * 4 + 15) // 16 * 16
        buf = np.full(nbytes // 4 + 4, 0x5a5a5a5a, np.int32)
        _lib.call("dfh_imgproc_fill_tables", p, C.c_void_p(buf.ctypes.data), nbytes)
        np.testing.assert_array_equal(buf[:want.size], want)
        assert not buf[want.size:nbytes // 4].any() and (buf[nbytes // 4:] == 0x5a5a5a5a).all()       # padding zeroed, nothing beyond written
        assert np.abs(want).max() < 2 ** 23                                      # the kernel's 24-bit multiply
        # every output row / column sums to 2^22 within the rounding of its taps
        for c in (cx, cy):
            assert np.abs(c.sum(1) - (1 << 22)).max() <= c.shape[1]
        with pytest.raises(_lib.DfhError, match="buffer smaller"):
            _lib.call("dfh_imgproc_fill_tables", p, C.c_void_p(buf.ctypes.data), nbytes - 1)
    finally:
        lib.dfh_imgproc_destroy(p)


@pytest.mark.parametrize("name", list(H.CASES))
def test_restatement_equals_the_fixtures_of_pil_and_transformers(name):
    fx = H.load_fixture(name)
    assert os.path.getsize(H.fixture_path(name)) < 1 << 20
    assert fx["checksum"] == H.checksum(H.case_images(name))
    got = H.case_expected(name)
    assert got.dtype == np.uint8 and got.shape == fx["u8"].shape and np.array_equal(got, fx["u8"])
    if name in H.TRANSFORMERS_CASES:
        lut = da.CLIPImageProcessor().lookup_table()
        assert fx["pixel_values"].dtype == np.float32 and np.array_equal(H.apply_lut(got, lut), fx["pixel_values"])


def test_binary_fixture_needs_the_clipped_intermediate():
    """The 0 / 255 image saturates hundreds of output pixels, and a resize without the uint8 clip between the passes differs."""
    fx = H.load_fixture("h53_w37_binary")["u8"]
    assert int(((fx == 0) | (fx == 255)).sum()) >= 100
    img = H.case_images("h53_w37_binary")[0].astype(np.int64)
    bx, cx = H.coefficients(37, 28, 3)
    by, cy = H.coefficients(53, 40, 3)
    hor = np.stack([np.tensordot(img[:, a:a + n], cx[i, :n].astype(np.int64), axes=([1], [0])) for i, (a, n) in enumerate(bx)], 1)   # unclipped, x 2^22
    ver = np.stack([np.tensordot(hor[a:a + n], cy[i, :n].astype(np.int64), axes=([0], [0])) for i, (a, n) in enumerate(by)], 0)
    unclipped = np.clip((ver + (1 << 43)) >> 44, 0, 255).astype(np.uint8)[6:34]
    assert (unclipped != fx[0]).sum() > 0


def test_lookup_table_equals_the_real_class_and_follows_mean_and_std():
    fx = H.load_fixture("lut")
    p = da.CLIPImageProcessor()
    assert np.array_equal(p.lookup_table(), fx["lut"]) and np.array_equal(H.lookup_table(), fx["lut"])
    p.image_mean, p.image_std = [0.5, 0.5, 0.5], [0.5, 0.25, 1.0]
    v = np.arange(256, dtype=np.float32) / np.float32(255)
    assert np.array_equal(p.lookup_table()[1], (v - np.float32(0.5)) / np.float32(0.25))
    assert [str(x) for x in fx["versions"]][0].split(".")[0].isdigit()


def test_f32_quantisation_of_the_restatement_is_postprocess():
    from difashion_amd.difashion import postprocess
    x, nan_at = H.f32_source()
    fx = H.load_fixture("f32_source")
    assert fx["checksum"] == H.checksum(x)
    clean = x.copy()
    clean[nan_at] = -1.0
    q = H.quantise(clean)
    assert np.array_equal(q, fx["quantised"])
    assert np.array_equal(q, np.stack([np.asarray(p) for p in postprocess(torch.from_numpy(clean), "pil")]))
    assert 100 < int(((q > 0) & (q < 255) & (q % 2 == 0)).sum())                 # the ties are in there: half to even
    _, _, _, edge, crop, resample = H.F32_CASE
    u8 = np.stack([H.preprocess_u8(im, edge, crop, crop, resample) for im in q])
    assert np.array_equal(u8, fx["u8"]) and np.array_equal(H.apply_lut(u8, H.lookup_table()), fx["pixel_values"])


def test_f32_sheet_fixture_is_postprocess_image_grid_and_the_restatement():
    x = H.f32_grid_source()
    fx = H.load_fixture("f32_grid3")
    assert fx["checksum"] == H.checksum(x)
    B, _, _, edge, crop, resample, grid = H.F32_GRID_CASE
    q = H.quantise(x)
    u8 = np.stack([H.preprocess_u8(H.image_grid(q[b * grid:(b + 1) * grid], grid), edge, crop, crop, resample) for b in range(B)])
    assert np.array_equal(u8, fx["u8"]) and np.array_equal(H.apply_lut(u8, H.lookup_table()), fx["pixel_values"])


def test_restatement_equals_pil_and_transformers_live():
    """Where Pillow / transformers import, the same comparison against the installed versions (the fixture comparison always runs)."""
    try:
        from PIL import Image
    except ImportError:
        return
    rng = np.random.default_rng(3)
    for (h, w, oh, ow, rs) in [(61, 40, 42, 28, 3), (40, 61, 28, 42, 2), (31, 20, 43, 28, 3), (7, 5, 39, 28, 3), (224, 224, 224, 224, 3),
                               (291, 291, 224, 224, 3), (200, 300, 224, 336, 3), (29, 29, 51, 51, 2)]:
        img = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
        assert np.array_equal(np.asarray(Image.fromarray(img).resize((ow, oh), rs)), H.pil_resize(img, oh, ow, rs)), (h, w, oh, ow, rs)
    try:
        from transformers import CLIPImageProcessor
    except ImportError:
        return
    real = CLIPImageProcessor(size={"shortest_edge": 28}, crop_size={"height": 28, "width": 28})
    for (h, w) in [(200, 300), (40, 61), (61, 40), (28, 45)]:
        img = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
        want = real(images=[Image.fromarray(img)], return_tensors="np")["pixel_values"][0]
        assert np.array_equal(H.apply_lut(H.preprocess_u8(img, 28, 28, 28, 3), H.lookup_table()), want), (h, w)


def test_refusals_carry_messages():
    h = C.c_void_p()
    create = lambda cfg, ih=40, iw=61, grid=0: _lib.call("dfh_imgproc_create", cfg, ih, iw, grid, C.byref(h))
    with pytest.raises(_lib.DfhError, match="null argument"):
        create(None)
    for rs in (0, 1, 4, 5):                                                      # nearest, lanczos, box, hamming: not built
        with pytest.raises(_lib.DfhError, match="unsupported resample filter"):
            create(C.byref(_lib.ImgProcConfigC(28, 28, 28, rs)))
    with pytest.raises(_lib.DfhError, match="smaller than the crop"):
        create(C.byref(_lib.ImgProcConfigC(20, 28, 28, 3)))
    with pytest.raises(_lib.DfhError, match="in_h / in_w"):
        create(C.byref(_lib.ImgProcConfigC(28, 28, 28, 3)), 0, 61)
    with pytest.raises(_lib.DfhError, match="grid_n"):
        create(C.byref(_lib.ImgProcConfigC(28, 28, 28, 3)), 40, 61, -1)
    with pytest.raises(_lib.DfhError, match="LDS budget"):                       # one output row's taps no longer fit: scale 28
        create(C.byref(_lib.ImgProcConfigC(224, 224, 224, 3)), 6272, 6272)
    create(C.byref(_lib.ImgProcConfigC(224, 224, 224, 3)), 4032, 4032)           # scale 18 fits
    _lib.raw().dfh_imgproc_destroy(h)
    p, buf = plan(40, 61, 28, 28, 3), C.c_void_p(4096)
    run = lambda pl, tab, lut, src, kind, B, px, u8: _lib.call("dfh_imgproc_run", pl, tab, lut, src, kind, B, px, u8, None)
    try:
        for args in ((None, buf, buf, buf, 0, 1, buf, None), (p, None, buf, buf, 0, 1, buf, None), (p, buf, buf, None, 0, 1, buf, None),
                     (p, buf, buf, buf, 0, 1, None, None), (p, buf, None, buf, 0, 1, buf, None)):
            with pytest.raises(_lib.DfhError, match="null argument"):
                run(*args)
        with pytest.raises(_lib.DfhError, match="16-byte aligned"):
            run(p, buf, buf, C.c_void_p(4100), 0, 1, buf, None)
        with pytest.raises(_lib.DfhError, match="16-byte aligned"):
            run(p, C.c_void_p(4104), buf, buf, 0, 1, buf, None)
        with pytest.raises(_lib.DfhError, match="src_kind"):
            run(p, buf, buf, buf, 2, 1, buf, None)
        with pytest.raises(_lib.DfhError, match="batch must be positive"):
            run(p, buf, buf, buf, 0, 0, buf, None)
    finally:
        _lib.raw().dfh_imgproc_destroy(p)


def test_python_side_refusals():
    p = da.CLIPImageProcessor(size={"shortest_edge": 28}, crop_size={"height": 28, "width": 28})
    with pytest.raises(da.DfhError, match="no CPU fallback"):
        p(images=torch.zeros(1, 40, 61, 3, dtype=torch.uint8))
    with pytest.raises(da.DfhError, match="no CPU fallback"):
        p(images=torch.zeros(1, 3, 40, 61))
    with pytest.raises(da.DfhError, match="no CPU fallback"):
        p(images=[np.zeros((40, 61, 3), np.uint8)], device="cpu")
    with pytest.raises(ValueError, match="unsupported resample"):
        da.CLIPImageProcessor(resample=1)
    with pytest.raises(ValueError, match="unsupported resample"):
        p.resize(torch.zeros(1, 40, 61, 3, dtype=torch.uint8), size=28, resample=0)
    for name in ("do_resize", "do_center_crop", "do_rescale", "do_normalize", "do_convert_rgb"):
        with pytest.raises(NotImplementedError, match=name + "=False"):
            da.CLIPImageProcessor(**{name: False})
    with pytest.raises(ValueError, match="shortest_edge"):
        da.CLIPImageProcessor(size={"height": 224, "width": 224})
    with pytest.raises(ValueError, match="specify images"):
        p()
    d = da.CLIPImageProcessor()
    assert d.size == {"shortest_edge": 224} and d.crop_size == {"height": 224, "width": 224} and d.resample == 3
    assert d.image_mean == H.OPENAI_CLIP_MEAN and d.image_std == H.OPENAI_CLIP_STD and d.rescale_factor == 1 / 255


def test_preprocessor_config_round_trips_with_the_real_class(tmp_path):
    p = da.CLIPImageProcessor(size={"shortest_edge": 56}, crop_size={"height": 56, "width": 48}, resample=2, image_mean=[0.5, 0.4, 0.3])
    p.save_pretrained(str(tmp_path / "mine"))
    assert os.listdir(tmp_path / "mine") == ["preprocessor_config.json"]
    saved = json.load(open(tmp_path / "mine" / "preprocessor_config.json"))
    assert saved["image_processor_type"] == "CLIPImageProcessor" and saved["size"] == {"shortest_edge": 56} and saved["resample"] == 2
    q = da.CLIPImageProcessor.from_pretrained(str(tmp_path), subfolder="mine")
    assert q.to_dict() == p.to_dict()
    from transformers import CLIPImageProcessor
    real = CLIPImageProcessor.from_pretrained(str(tmp_path / "mine"))               # the real class reads what this class wrote ...
    assert dict(real.size) == {"shortest_edge": 56} and dict(real.crop_size) == {"height": 56, "width": 48} and int(real.resample) == 2
    assert list(real.image_mean) == [0.5, 0.4, 0.3] and list(real.image_std) == H.OPENAI_CLIP_STD
    CLIPImageProcessor(size={"shortest_edge": 32}, crop_size={"height": 30, "width": 32}, resample=3,
                       image_std=[0.2, 0.3, 0.4]).save_pretrained(str(tmp_path / "real"))
    r = da.CLIPImageProcessor.from_pretrained(str(tmp_path / "real"))               # ... and this class what the real class wrote
    assert r.size == {"shortest_edge": 32} and r.crop_size == {"height": 30, "width": 32} and r.resample == 3
    assert r.image_std == [0.2, 0.3, 0.4] and r.image_mean == H.OPENAI_CLIP_MEAN and r.rescale_factor == 1 / 255


def test_plan_and_tables_under_the_host_sanitizers(tmp_path):
    """csrc/image_processor.hip's host side, built with tests/native/imgproc_sanitize.hip into a program of its own under
    -fsanitize=address,undefined, over every shape of this file: geometry equal to the library's, no report."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found: the sanitizer build needs the compiler the library is built with")
    exe = str(tmp_path / "imgproc_sanitize")
    cmd = [hipcc, "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-Xarch_host", "-fsanitize=address,undefined",
           "-Xarch_host", "-fno-sanitize-recover=undefined", os.path.join(_lib.CSRC, "image_processor.hip"),
           os.path.join(ROOT, "tests", "native", "imgproc_sanitize.hip"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    shapes = SHAPES + [(40, 61, 20, 28, 3, 0), (6272, 6272, 224, 224, 3, 0), (40, 61, 28, 28, 9, 0)]      # three refusals ride along
    args = [str(v) for s in shapes for v in s]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0")                      # the HIP runtime's start-up allocations are not ours to free
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0 and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == len(shapes) and sum(l.startswith("refused: ") for l in lines) == 3
    lib = _lib.raw()
    for s, line in zip(SHAPES, lines):
        p = plan(*s)
        try:
            want = (f"-> {lib.dfh_imgproc_resized_height(p)} x {lib.dfh_imgproc_resized_width(p)} top {lib.dfh_imgproc_crop_top(p)} "
                    f"left {lib.dfh_imgproc_crop_left(p)} ksize {lib.dfh_imgproc_ksize_x(p)} {lib.dfh_imgproc_ksize_y(p)} ")
            assert want in line, (s, line)
        finally:
            lib.dfh_imgproc_destroy(p)

"""CPU tier (-m "not gpu"): the host-only half of the CLIP image encoder -- the C ABI of the ``dfh_clipv_*`` family in
all three places (header, both libraries, ctypes), the parameter table against the REAL ``transformers.CLIPVisionModelWithProjection``
state dict, config checks, refusals and the checkpoint directory.  No compute call is made here; the arithmetic is checked on the
GPU (tests/test_gpu_clip_vision.py) against the fixtures of tests/golden/make_golden_clip_vision.py."""
import ctypes as C
import dataclasses
import json
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import difashion_amd as da
from difashion_amd import _lib
from tests.helpers_clip_vision import (CASES, FULL_SIZE_ROWS, TINY_GELU, TINY_QUICKGELU, VIT_H_14, case_inputs, checksum, fixture_path,
                                       load_fixture, param_shapes)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILY = ["dfh_clipv_create", "dfh_clipv_destroy", "dfh_clipv_num_params", "dfh_clipv_param_name", "dfh_clipv_param_ndim",
          "dfh_clipv_param_dim", "dfh_clipv_workspace_bytes", "dfh_clipv_encode", "dfh_clipv_attention"]


def _config_c(cfg, **over):
    kw = dict(cfg.kwargs(), **over)
    return _lib.CLIPVisionConfigC(kw["hidden_size"], kw["intermediate_size"], kw["num_hidden_layers"], kw["num_attention_heads"],
                                  kw["image_size"], kw["patch_size"], kw["num_channels"], kw["projection_dim"],
                                  {"quick_gelu": 1, "gelu": 2}.get(kw["hidden_act"], 3), kw["layer_norm_eps"])


def _model(cfg, **kw):
    return da.CLIPVisionModelWithProjection(**cfg.kwargs(), **kw)


def test_every_clipv_symbol_is_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "difashion_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(dfh_clipv_[a-z0-9_]+)\s*\(", src))
    assert declared == set(FAMILY)
    assert "#define DFH_ABI_VERSION 8" in src
    for lib_name in _lib._LIB_NAMES.values():                                   # both storage builds export the row
        lib = C.CDLL(os.path.join(_lib.CSRC, lib_name))
        for n in FAMILY:
            assert hasattr(lib, n), f"{n} not exported by {lib_name}"
    for n in FAMILY:
        assert n in _lib.SIGNATURES, n
    # the ctypes mirror of dfh_clipv_config follows the header's field order
    body = re.search(r"typedef struct dfh_clipv_config \{(.*?)\} dfh_clipv_config;", src, flags=re.S).group(1)
    fields = [re.sub(r"^(int|float)\s+", "", d.strip()) for d in body.split(";") if d.strip()]
    assert fields == [f[0] for f in _lib.CLIPVisionConfigC._fields_]
    assert {"clipv_embed", "clipv_linear", "clipv_layernorm", "clipv_attention"} <= set(_lib.census())


def test_parameter_table_without_a_gpu_equals_the_real_class_tiny():
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    cfg = TINY_QUICKGELU
    m = _model(cfg)
    real = CLIPVisionModelWithProjection(CLIPVisionConfig(**cfg.kwargs()))
    want = [(k, tuple(v.shape)) for k, v in real.state_dict().items() if not k.endswith("position_ids")]
    assert m.param_table() == want == param_shapes(cfg)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == want
    assert "vision_model.pre_layrnorm.weight" in dict(want)                      # transformers' own spelling
    assert m.dtype == torch.float32 and m.device.type == "cpu" and m.num_tokens == 50
    assert not any(p.requires_grad for p in m.requires_grad_(False).parameters())
    for k in ("hidden_size", "intermediate_size", "projection_dim", "num_hidden_layers", "num_attention_heads", "num_channels",
              "image_size", "patch_size", "hidden_act", "layer_norm_eps"):
        assert m.config[k] == getattr(real.config, k) == getattr(m.config, k), k
    # seeded init: matrices drawn, norm weights ones, everything else zeros; without a seed a checkpoint is expected to follow
    sd = m.state_dict()
    assert float(sd["visual_projection.weight"].std()) > 0 and torch.equal(sd["vision_model.pre_layrnorm.weight"], torch.ones(64))
    assert not _model(cfg, init_seed=None).state_dict()["visual_projection.weight"].any()


def test_vit_h_14_table_equals_the_real_class_without_allocating_weights():
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    cfg = VIT_H_14
    with torch.device("meta"):
        real = CLIPVisionModelWithProjection(CLIPVisionConfig(**cfg.kwargs()))
    want = [(k, tuple(v.shape)) for k, v in real.state_dict().items() if not k.endswith("position_ids")]
    h = C.c_void_p()
    _lib.call("dfh_clipv_create", C.byref(_config_c(cfg)), C.byref(h))
    lib = _lib.raw()
    try:
        table = da.CLIPVisionModelWithProjection._table(h)
        assert table == want == param_shapes(cfg)
        n = sum(int(np.prod(s)) for _, s in table)
        assert n == 632_076_800 == sum(v.numel() for v in real.parameters())     # OpenCLIP ViT-H/14 vision tower + projection: 632 M
        assert len(table) == 5 + 16 * 32 + 3
        # workspace: x, ln, q k v, attention, MLP hidden of batch x 257 rows
        M = 50 * 257
        assert M * (6 * 1280 + 5120) * 4 < lib.dfh_clipv_workspace_bytes(h, 50) < M * (6 * 1280 + 5120) * 4 * 1.01
        assert lib.dfh_clipv_workspace_bytes(h, 0) == 0
        assert lib.dfh_clipv_param_name(h, 10_000) == b"" and lib.dfh_clipv_param_dim(h, 1, 9) == 0
    finally:
        lib.dfh_clipv_destroy(h)


@pytest.mark.parametrize("cfg,im2col_wider", [(TINY_QUICKGELU, False), (TINY_GELU, True), (dataclasses.replace(TINY_GELU, image_size=56), True),
                                              (VIT_H_14, False)], ids=["tiny_patch8", "tiny_patch14", "tiny_56_patch14", "vit_h_14"])
def test_workspace_bytes_are_pinned_exactly(cfg, im2col_wider):
    """x, ln, attention (3 D a row), the q k v region -- max(3 D, C p^2) wide, since it holds the im2col rows of the patch conv too --
    the MLP hidden, one pooled row per image, 64 floats of slack, 256 bytes for alignment."""
    h = C.c_void_p()
    _lib.call("dfh_clipv_create", C.byref(_config_c(cfg)), C.byref(h))
    lib = _lib.raw()
    try:
        D, I, T, K = cfg.hidden_size, cfg.intermediate_size, cfg.num_tokens, cfg.num_channels * cfg.patch_size ** 2
        assert (K > 3 * D) == im2col_wider                                       # both branches of the max are covered
        for B in (1, 3, 50):
            assert lib.dfh_clipv_workspace_bytes(h, B) == (B * T * (3 * D + max(3 * D, K) + I) + B * D + 64) * 4 + 256, B
    finally:
        lib.dfh_clipv_destroy(h)


def test_bad_configs_are_rejected_with_messages():
    h = C.c_void_p()
    for over, msg in ((dict(hidden_size=66), "multiples of 4"), (dict(num_attention_heads=3), "divide into the heads"),
                      (dict(hidden_size=72, num_attention_heads=4), "head dim"), (dict(hidden_size=1024, num_attention_heads=4), "head dim"),
                      (dict(image_size=60), "multiple of patch_size"), (dict(patch_size=7, image_size=56), "multiple of 4"),
                      (dict(hidden_act="relu"), "hidden_act"), (dict(num_hidden_layers=0), "num_hidden_layers"),
                      (dict(projection_dim=0), "projection_dim")):
        with pytest.raises(_lib.DfhError, match=msg):
            _lib.call("dfh_clipv_create", C.byref(_config_c(TINY_QUICKGELU, **over)), C.byref(h))
    with pytest.raises(_lib.DfhError, match="null argument"):
        _lib.call("dfh_clipv_create", None, C.byref(h))
    with pytest.raises(ValueError, match="hidden_act"):
        da.CLIPVisionModelWithProjection(**dict(TINY_QUICKGELU.kwargs(), hidden_act="relu"))


def test_encode_guards_its_arguments_before_any_launch():
    """Null arguments, table count, parameter alignment and the workspace size are refused on the host (no GPU is touched)."""
    cfg = TINY_QUICKGELU
    h = C.c_void_p()
    _lib.call("dfh_clipv_create", C.byref(_config_c(cfg)), C.byref(h))
    lib = _lib.raw()
    try:
        n = lib.dfh_clipv_num_params(h)
        good = (C.c_void_p * n)(*([4096] * n))
        buf = C.c_void_p(4096)
        need = lib.dfh_clipv_workspace_bytes(h, 2)
        enc = lambda arr, cnt, px, last, ws, ws_bytes: _lib.call("dfh_clipv_encode", h, arr, cnt, px, 2, last, None, None, None, ws, ws_bytes, None)
        with pytest.raises(_lib.DfhError, match="null argument"):
            enc(good, n, None, buf, buf, need)
        with pytest.raises(_lib.DfhError, match="count does not match"):
            enc(good, n - 1, buf, buf, buf, need)
        holed = (C.c_void_p * n)(*([4096] * 3 + [0] + [4096] * (n - 4)))
        with pytest.raises(_lib.DfhError, match="null parameter pointer: vision_model.pre_layrnorm.weight"):
            enc(holed, n, buf, buf, buf, need)
        odd = (C.c_void_p * n)(*([4096] * 5 + [4100] + [4096] * (n - 6)))
        with pytest.raises(_lib.DfhError, match="not 16-byte aligned: vision_model.encoder.layers.0.self_attn.k_proj.weight"):
            enc(odd, n, buf, buf, buf, need)
        with pytest.raises(_lib.DfhError, match="workspace smaller"):
            enc(good, n, buf, buf, buf, need - 1)
        with pytest.raises(_lib.DfhError, match="256-byte aligned"):
            enc(good, n, buf, buf, C.c_void_p(4096 + 16), need)
        with pytest.raises(_lib.DfhError, match="head dim"):
            _lib.call("dfh_clipv_attention", buf, buf, 1, 8, 2, 130, 1.0, None)
        with pytest.raises(_lib.DfhError, match="null argument"):
            _lib.call("dfh_clipv_attention", None, buf, 1, 8, 2, 64, 1.0, None)
    finally:
        lib.dfh_clipv_destroy(h)


def test_compute_path_refuses_cpu_tensors_and_wrong_inputs():
    cfg = TINY_QUICKGELU
    m = _model(cfg, init_seed=None)
    x = torch.zeros(1, 3, 56, 56)
    with pytest.raises(da.DfhError, match="no CPU fallback"):
        m(x)
    with pytest.raises(da.DfhError, match="no CPU fallback"):
        m.encode_image(x)
    with pytest.raises(ValueError, match="specify pixel_values"):
        m()
    with pytest.raises(NotImplementedError, match="attention mask"):
        m(x, attention_mask=torch.ones(1, 50))
    with pytest.raises(NotImplementedError, match="interpolate_pos_encoding"):
        m(x, interpolate_pos_encoding=True)


def test_checkpoint_directory_round_trips_and_loads_into_the_real_class(tmp_path):
    from transformers import CLIPVisionModelWithProjection
    cfg, params, _ = case_inputs("tiny_gelu")
    m = _model(cfg, init_seed=None)
    m.load_state_dict(params)
    m.save_pretrained(str(tmp_path / "image_encoder"))
    assert sorted(os.listdir(tmp_path / "image_encoder")) == ["config.json", "model.safetensors"]
    saved = json.load(open(tmp_path / "image_encoder" / "config.json"))
    assert saved["architectures"] == ["CLIPVisionModelWithProjection"] and saved["hidden_act"] == "gelu" and saved["patch_size"] == 14
    m2 = da.CLIPVisionModelWithProjection.from_pretrained(str(tmp_path), subfolder="image_encoder")
    assert m2.config == m.config and list(m2.state_dict()) == list(params)
    assert all(torch.equal(v, params[k]) for k, v in m2.state_dict().items())
    # the real class reads the directory this wrapper wrote ...
    real = CLIPVisionModelWithProjection.from_pretrained(str(tmp_path / "image_encoder")).eval()
    real_sd = {k: v for k, v in real.state_dict().items() if not k.endswith("position_ids")}
    assert list(real_sd) == list(params) and all(torch.equal(v, params[k]) for k, v in real_sd.items())
    assert real.config.hidden_act == "gelu" and real.config.projection_dim == cfg.projection_dim
    # ... and this wrapper reads the directory the real class wrote (position_ids or not)
    real.save_pretrained(str(tmp_path / "from_real"))
    m3 = da.CLIPVisionModelWithProjection.from_pretrained(str(tmp_path / "from_real"))
    assert m3.config == m.config and all(torch.equal(v, params[k]) for k, v in m3.state_dict().items())
    m3.load_state_dict(dict(params, **{"vision_model.embeddings.position_ids": torch.arange(10)[None]}))
    with pytest.raises(RuntimeError, match="Missing key"):
        m3.load_state_dict({k: v for k, v in params.items() if "pre_layrnorm" not in k})


@pytest.mark.parametrize("name", list(CASES))
def test_fixtures_belong_to_the_regenerated_inputs(name):
    """The committed fixtures hold what the GPU test needs: fp64 outputs, the fp32 class's own distance to them, and a checksum that
    the seeded weights and pixels regenerate to.  (Full-size weights are regenerated on the GPU leg only: 632 M values.)"""
    fx = load_fixture(name)
    cfg, _, _, full = CASES[name]
    assert os.path.getsize(fixture_path(name)) < 1 << 20
    keys = ["last_hidden_state", "pooler_output", "image_embeds"] + [f"hidden_{int(t)}" for t in fx["taps"]]
    for k in keys:
        assert fx[k].dtype == np.float32 and np.isfinite(fx[k]).all()
        assert 1e-8 < float(fx["ref_" + k]) < 1e-5, (k, fx["ref_" + k])          # fp32 against fp64: rounding noise, not a bug
    L = cfg.num_hidden_layers
    assert list(fx["taps"]) == ([0, L // 2, L] if full else list(range(L + 1)))
    rows = len(FULL_SIZE_ROWS) if full else cfg.num_tokens
    assert fx["last_hidden_state"].shape[1:] == (rows, cfg.hidden_size) and fx["image_embeds"].shape[1] == cfg.projection_dim
    np.testing.assert_array_equal(fx[f"hidden_{L}"], fx["last_hidden_state"])    # transformers: the last block's output, not normalised
    assert 2.0 / cfg.num_tokens < fx["attention_peak"].min() and fx["attention_peak"].max() < 0.8
    if not full:
        _, params, pixels = case_inputs(name)
        np.testing.assert_allclose(fx["checksum"], checksum(params, pixels), rtol=1e-12)


def test_product_file_is_in_both_builds_and_fp32():
    """The row is compiled into both storage builds from one source, and that source names neither 16-bit type."""
    mk = open(os.path.join(_lib.CSRC, "Makefile")).read()
    assert "clip_vision.hip" in mk and "clip_kernels.h" in mk and "f32_tile.h" in mk
    for name in ("clip_vision.hip", "f32_tile.h"):
        src = open(os.path.join(_lib.CSRC, name)).read()
        assert not re.search(r"\b(bf16_t|h16x8_t|DFH_F16|pack2bf|f2bf)\b", src), name
    r = subprocess.run(["nm", "-D", "--defined-only", os.path.join(_lib.CSRC, _lib._LIB_NAMES["fp16"])], capture_output=True, text=True)
    if r.returncode == 0:
        assert "dfh_clipv_encode" in r.stdout

"""CPU tier (-m "not gpu"): the host-only half of the 16-bit CLIP image encoder -- the C ABI of the
``dfh_clipvh_*`` family in header, both libraries and ctypes; the plan of the whole encode for every case (geometry, K padding, V^T
pitch, every launch's buffers inside the carved workspace, packed-copy size); the plan of the two new GEMM activations; the fixtures'
checksums and the yardstick file; the dtype switch and its refusals.  No compute call is made here: the arithmetic is checked on the
GPU (tests/test_gpu_clip_vision_half.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import difashion_amd as da
from difashion_amd import _lib
from tests.helpers_clip_vision import TINY_GELU, checksum
from tests.helpers_clip_vision_half import (FORMATS, HALF_CASES, NEW_CASES, YARDSTICKS, case_inputs, kept_rows, load_fixture, output_keys,
                                            yardstick)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILY = ["dfh_clipvh_plan", "dfh_clipvh_packed_bytes", "dfh_clipvh_pack", "dfh_clipvh_workspace_bytes", "dfh_clipvh_encode"]
ACT_GELU, ACT_QUICK_GELU = 5, 6


def _ctx(cfg):
    kw = cfg.kwargs()
    c = _lib.CLIPVisionConfigC(kw["hidden_size"], kw["intermediate_size"], kw["num_hidden_layers"], kw["num_attention_heads"], kw["image_size"],
                               kw["patch_size"], kw["num_channels"], kw["projection_dim"], {"quick_gelu": 1, "gelu": 2}[kw["hidden_act"]],
                               kw["layer_norm_eps"])
    h = C.c_void_p()
    _lib.call("dfh_clipv_create", C.byref(c), C.byref(h))
    return h


def _plan(h, batch):
    p = _lib.CLIPVHalfPlanC()
    _lib.call("dfh_clipvh_plan", h, batch, C.byref(p))
    return p


def test_every_clipvh_symbol_is_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "difashion_hip.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(dfh_clipvh_[a-z0-9_]+)\s*\(", src)) == set(FAMILY)
    assert "#define DFH_ABI_VERSION 8" in src                                   # additive: the ABI number stays
    for lib_name in _lib._LIB_NAMES.values():                                   # both storage builds carry the walk
        lib = C.CDLL(os.path.join(_lib.CSRC, lib_name))
        for n in FAMILY:
            assert hasattr(lib, n), f"{n} not exported by {lib_name}"
    for n in FAMILY:
        assert n in _lib.SIGNATURES, n
    # the ctypes mirrors follow the header's field order and array bounds
    for name, mirror in (("dfh_clipvh_launch", _lib.CLIPVHalfLaunchC), ("dfh_clipvh_region", _lib.CLIPVHalfRegionC),
                         ("dfh_clipvh_plan_info", _lib.CLIPVHalfPlanC)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, flags=re.S).group(1)
        fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                fields += [re.sub(r"\[.*\]", "", f.strip()) for f in re.sub(r"^[a-z_0-9]+\s+", "", decl).split(",")]
        assert fields == [f[0] for f in mirror._fields_], name
    assert f"#define DFH_CLIPVH_MAX_LAUNCHES {_lib.CLIPVH_MAX_LAUNCHES}" in src and f"#define DFH_CLIPVH_MAX_REGIONS {_lib.CLIPVH_MAX_REGIONS}" in src


@pytest.mark.parametrize("name", list(HALF_CASES))
def test_plan_geometry_and_workspace_bounds(name):
    cfg, _, batch, _ = HALF_CASES[name]
    D, I, T, H = cfg.hidden_size, cfg.intermediate_size, cfg.num_tokens, cfg.num_attention_heads
    K = cfg.num_channels * cfg.patch_size ** 2
    h = _ctx(cfg)
    lib = _lib.raw()
    try:
        for B in (1, batch, 7):
            p = _plan(h, B)
            M, Mp = B * T, B * (T - 1)
            assert (p.batch, p.tokens, p.hidden, p.intermediate, p.heads, p.head_dim, p.layers) == (B, T, D, I, H, D // H, cfg.num_hidden_layers)
            assert (p.rows, p.patch_rows, p.patch_k, p.patch_k_padded, p.ldvt) == (M, Mp, K, -(-K // 8) * 8, -(-T // 8) * 8)
            assert p.patch_k_padded % 8 == 0 and 0 <= p.patch_k_padded - K < 8 and p.ldvt % 8 == 0 and 0 <= p.ldvt - T < 8
            # dfh_attention's dispatch at these lengths: the 32x32x16 kernel from 256 tokens on at head dim 80 (ViT-H/14), else the 16x16x32 one
            assert p.attention_x32 == int(D // H == 80 and T >= 256)
            L = {p.launches[i].name.decode(): p.launches[i] for i in range(p.num_launches)}
            R = [p.regions[i] for i in range(p.num_regions)]
            assert list(L) == ["patch", "qkv", "out_proj", "fc1", "fc2"]
            gact = ACT_GELU if cfg.hidden_act == "gelu" else ACT_QUICK_GELU
            want = {"patch": (Mp, D, p.patch_k_padded, D, 0, 0, 0), "qkv": (M, 3 * D, D, 2 * D, 0, 0, 1), "out_proj": (M, D, D, D, 0, 1, 1),
                    "fc1": (M, I, D, I, gact, 0, 1), "fc2": (M, D, I, D, 0, 1, 1)}
            for n, l in L.items():
                assert (l.M, l.N, l.K, l.ld_out, l.act, l.resid, l.per_layer) == want[n], n
                assert l.lda == l.K == l.ldw and l.K % 8 == 0 and l.N % 8 == 0 and l.ld_out % 8 == 0, n
                # the buffers of the launch lie inside their regions
                assert R[l.a_region].bytes >= l.M * l.lda * 2 and R[l.out_region].bytes >= l.M * l.ld_out * 2, n
            q = L["qkv"]
            assert (q.n_split, q.ld_out2, q.rows_per_b) == (2 * D, p.ldvt, T) and R[q.out2_region].bytes >= B * D * p.ldvt * 2
            assert all(l.out2_region == -1 and l.n_split == 0 for n, l in L.items() if n != "qkv")
            # the carve: 256-byte aligned, disjoint, in order, inside the workspace the size query reports
            end = 0
            for r in R:
                assert r.offset % 256 == 0 and r.offset >= end and (r.bytes > 0 or r.name == b"splitk_partial"), r.name
                end = r.offset + r.bytes
            assert end <= p.workspace_bytes == lib.dfh_clipvh_workspace_bytes(h, B) < end + 256      # no slack: the caller aligns the block
            names = [r.name.decode() for r in R]
            assert names == ["zero", "im2col", "patch", "x", "ln", "qk", "vt", "attention", "mlp_hidden", "splitk_partial", "class_rows", "pooled"]
            assert R[names.index("x")].bytes == M * D * 2 and R[names.index("mlp_hidden")].bytes == M * I * 2
            # packed copy: every matrix once in 16 bits (the patch weight with its padded K) + the stacked fp32 q | k | v biases
            exact = D * p.patch_k_padded * 2 + cfg.num_hidden_layers * ((4 * D * D + 2 * D * I) * 2 + 3 * D * 4)
            assert exact <= p.packed_bytes == lib.dfh_clipvh_packed_bytes(h) <= exact + 256 * (1 + 5 * cfg.num_hidden_layers)
            # the offsets the pack writes are the ones the walk reads: the patch matrix, then per layer wqkv | wo | w1 | w2 | bqkv, each
            # rounded up to 256 bytes, computed by hand
            up = lambda n: -(-n // 256) * 256
            per_layer = up(3 * D * D * 2) + up(D * D * 2) + 2 * up(D * I * 2) + up(3 * D * 4)
            assert p.packed_bytes == up(D * p.patch_k_padded * 2) + cfg.num_hidden_layers * per_layer and per_layer % 256 == 0
    finally:
        lib.dfh_clipv_destroy(h)


def test_plan_pins_the_paddings_of_the_real_towers():
    h = _ctx(HALF_CASES["vit_h_14"][0])
    try:
        p = _plan(h, 200)
        assert (p.patch_k, p.patch_k_padded, p.tokens, p.ldvt, p.rows, p.head_dim, p.attention_x32) == (588, 592, 257, 264, 51400, 80, 1)
    finally:
        _lib.raw().dfh_clipv_destroy(h)
    h = _ctx(HALF_CASES["vit_l_14"][0])
    try:
        p = _plan(h, 200)
        assert (p.patch_k_padded, p.ldvt, p.head_dim, p.attention_x32) == (592, 264, 64, 0)
    finally:
        _lib.raw().dfh_clipv_destroy(h)


def test_plan_refuses_what_the_walk_cannot_run():
    h = _ctx(TINY_GELU)                                                          # head dim 16: the fp32 tower's, not a 16-bit attention kernel's
    lib = _lib.raw()
    try:
        p = _lib.CLIPVHalfPlanC()
        with pytest.raises(_lib.DfhError, match=r"head dim 16 is not built \(supported: 32, 40, 64, 80, 128, 160\)"):
            _lib.call("dfh_clipvh_plan", h, 2, C.byref(p))
        assert lib.dfh_clipvh_workspace_bytes(h, 2) == 0 and lib.dfh_clipvh_packed_bytes(h) == 0
        assert lib.dfh_clipv_workspace_bytes(h, 2) > 0                           # the fp32 tower still takes it
    finally:
        lib.dfh_clipv_destroy(h)
    # hidden 192 / 3 heads (head dim 64): 3 x 192 = 576 columns run on 160-column tiles, and V^T would begin at column 384, inside a tile.
    # Refused by the plan, by name, not by the q | k | v launch in the middle of a walk
    import dataclasses
    vit_tiny = dataclasses.replace(HALF_CASES["half_tiny_d64"][0], hidden_size=192, intermediate_size=768, num_attention_heads=3)
    h = _ctx(vit_tiny)
    try:
        with pytest.raises(_lib.DfhError, match="2 x hidden must be a multiple of 160"):
            _lib.call("dfh_clipvh_plan", h, 3, C.byref(_lib.CLIPVHalfPlanC()))
        assert lib.dfh_clipvh_workspace_bytes(h, 3) == 0 and lib.dfh_clipvh_packed_bytes(h) == 0
    finally:
        lib.dfh_clipv_destroy(h)
    m = da.CLIPVisionModelWithProjection(**vit_tiny.kwargs(), init_seed=None)
    with pytest.raises(da.DfhError, match="2 x hidden must be a multiple of 160"):
        m.set_compute_dtype(_lib.storage_dtype())
    assert m.compute_dtype == torch.float32
    d = _lib.GemmDesc()                                                          # what the launch itself would have said
    d.a0, d.a0_c, d.W, d.ldw, d.M, d.N, d.out, d.ld_out, d.force_order = 1, 192, 1, 192, 591, 576, 1, 384, -1
    info = _lib.GemmPlanInfo()
    _lib.call("dfh_gemm_plan", C.byref(d), None, C.byref(info))
    assert info.bn == 160 and 384 % info.bn != 0
    h = _ctx(HALF_CASES["half_tiny_d64"][0])
    try:
        with pytest.raises(_lib.DfhError, match="batch must be in"):
            _lib.call("dfh_clipvh_plan", h, 0, C.byref(_lib.CLIPVHalfPlanC()))
        assert lib.dfh_clipvh_workspace_bytes(h, 0) == 0
    finally:
        lib.dfh_clipv_destroy(h)


@pytest.mark.parametrize("M,N,K", [(50, 256, 128), (771, 640, 160), (51400, 5120, 1280)])
@pytest.mark.parametrize("act", [ACT_GELU, ACT_QUICK_GELU])
def test_gemm_plan_of_the_new_activations(M, N, K, act):
    """Both activations live in the two XACT instantiations of the eight-wave 128 x 160 tile only: single pass, two stages, whatever
    the shape or the force ids; LEAN when K is a whole number of 64-channel slices.  The same shape without them plans as before."""
    d = _lib.GemmDesc()
    d.a0, d.a0_c, d.W, d.ldw, d.M, d.N, d.out, d.ld_out, d.act, d.force_order = 1, K, 1, K, M, N, 1, N, act, -1
    d.bias = 1
    for force_tile, force_split in ((0, 0), (2, 0), (21, 0), (0, 4)):
        d.force_tile, d.force_split = force_tile, force_split
        info = _lib.GemmPlanInfo()
        _lib.call("dfh_gemm_plan", C.byref(d), None, C.byref(info))
        assert (info.kernel, info.tile, info.bm, info.bn, info.stages, info.split, info.wide) == (0, 5, 128, 160, 2, 1, 0), info.line
        assert info.lean == int(K % 64 == 0)
    d.force_tile = d.force_split = 0
    assert _lib.raw().dfh_gemm_partial_floats(C.byref(d)) == 0                   # the heuristics never ask for split-K slabs here
    for bad in (dict(out_mode=2), dict(N=N + 4), dict(ld_out=N + 4)):             # fp32 output / rows that are not 16-byte multiples
        e = _lib.GemmDesc()
        C.memmove(C.byref(e), C.byref(d), C.sizeof(d))
        e.force_tile = e.force_split = 0
        for k, v in bad.items():
            setattr(e, k, v)
        if "N" in bad:
            e.ld_out = N + 4
        with pytest.raises(_lib.DfhError, match="GELU / quick-GELU epilogue"):
            _lib.call("dfh_gemm_plan", C.byref(e), None, C.byref(_lib.GemmPlanInfo()))


@pytest.mark.parametrize("name", NEW_CASES)
def test_new_fixtures_hold_the_seeded_inputs_and_rows(name):
    cfg, params, pixels = case_inputs(name)
    fx = load_fixture(name)
    np.testing.assert_allclose(fx["checksum"], checksum(params, pixels), rtol=1e-12)
    B, T, D, L = pixels.shape[0], cfg.num_tokens, cfg.hidden_size, cfg.num_hidden_layers
    rows = kept_rows(T)
    assert list(fx["rows"]) == rows and list(fx["taps"]) == list(range(L + 1)) and 0 in rows and T - 1 in rows
    assert fx["image_embeds"].shape == (B, cfg.projection_dim) and fx["pooler_output"].shape == (B, D)
    for k in ["last_hidden_state"] + [f"hidden_{t}" for t in range(L + 1)]:
        assert fx[k].shape == (B, len(rows), D) and fx[k].dtype == np.float32 and np.isfinite(fx[k]).all(), k
    assert np.array_equal(fx[f"hidden_{L}"], fx["last_hidden_state"])
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", f"clipv_half_{name}.npz")) < 1 << 20


def test_yardstick_file_covers_every_case_output_and_format():
    ys = dict(np.load(YARDSTICKS))
    for name in HALF_CASES:
        cfg, params, pixels = case_inputs(name) if name in NEW_CASES else (None, None, None)
        fx = load_fixture(name)
        np.testing.assert_allclose(ys[f"{name}/checksum"], fx["checksum"], rtol=1e-12)
        for fmt in FORMATS:
            for key in output_keys(fx) + ["cos"]:
                v = yardstick(ys, name, fmt, key)
                assert np.isfinite(v) and 0 < v < 5e-2, (name, fmt, key, v)
        # what the formats are: fp16 carries 3 more mantissa bits than bf16
        assert yardstick(ys, name, "fp16", "image_embeds") < 0.3 * yardstick(ys, name, "bf16", "image_embeds")
    # the full-size towers, as the real class measures them here
    assert 1.0e-2 < yardstick(ys, "vit_h_14", "bf16", "image_embeds") < 1.5e-2 and yardstick(ys, "vit_h_14", "bf16", "cos") < 1e-4
    assert os.path.getsize(YARDSTICKS) < 64 << 10


def _tiny(**kw):
    return da.CLIPVisionModelWithProjection(**HALF_CASES["half_tiny_short"][0].kwargs(), **kw)


def test_compute_dtype_switch_never_casts_a_parameter():
    own, other = _lib.storage_dtype(), (torch.float16 if _lib.storage() == "bf16" else torch.bfloat16)
    m = _tiny()
    before = {k: v.clone() for k, v in m.state_dict().items()}
    assert m.compute_dtype == torch.float32 and m.dtype == torch.float32
    routes = {torch.bfloat16: m.bfloat16, torch.float16: m.half}
    assert routes[own]() is m and m.compute_dtype == own
    assert m.float() is m and m.compute_dtype == torch.float32
    assert m.to(dtype=own) is m and m.compute_dtype == own and m.to(torch.float32).compute_dtype == torch.float32
    assert m.to(own).compute_dtype == own and m.to("cpu", own).compute_dtype == own
    assert m.set_compute_dtype(torch.float32).compute_dtype == torch.float32
    assert _tiny(torch_dtype=own).compute_dtype == own and _tiny(torch_dtype=None).compute_dtype == torch.float32
    for mode in (own, torch.float32):
        m.set_compute_dtype(mode)
        sd = m.state_dict()
        assert m.dtype == torch.float32 and all(p.dtype == torch.float32 for p in m.parameters())
        assert list(sd) == list(before) and all(torch.equal(sd[k], before[k]) and sd[k].dtype == torch.float32 for k in sd)
    # the other 16-bit format: refused, the message says whose property the format is
    for route in (routes[other], lambda: m.to(dtype=other), lambda: m.set_compute_dtype(other), lambda: _tiny(torch_dtype=other)):
        with pytest.raises(da.DfhError, match=r"property of the process \(DFH_STORAGE / set_storage\(\)") as e:
            route()
        assert "stay fp32" in str(e.value)
    assert m.compute_dtype == torch.float32
    with pytest.raises(da.DfhError, match="computes in float32 or in"):
        m.double()
    with pytest.raises(TypeError, match="floating torch.dtype"):
        m.set_compute_dtype(torch.int32)


def test_unsupported_head_dim_is_refused_when_the_mode_is_enabled():
    m = da.CLIPVisionModelWithProjection(**TINY_GELU.kwargs())                   # head dim 16: fine in fp32
    with pytest.raises(da.DfhError, match=r"head dims 32, 40, 64, 80, 128, 160; this config has head dim 16"):
        m.set_compute_dtype(_lib.storage_dtype())
    assert m.compute_dtype == torch.float32
    with pytest.raises(da.DfhError, match="head dim 16"):
        da.CLIPVisionModelWithProjection(**TINY_GELU.kwargs(), torch_dtype=_lib.storage_dtype())


def test_checkpoints_stay_fp32_and_from_pretrained_takes_torch_dtype(tmp_path):
    own = _lib.storage_dtype()
    m = _tiny(init_seed=3, torch_dtype=own)
    m.save_pretrained(str(tmp_path / "enc"))
    import json
    from safetensors.torch import load_file
    cfg = json.load(open(tmp_path / "enc" / "config.json"))
    assert "torch_dtype" not in cfg and cfg["hidden_size"] == 128
    saved = load_file(str(tmp_path / "enc" / "model.safetensors"))
    assert all(v.dtype == torch.float32 for v in saved.values()) and not any("packed" in k for k in saved)
    assert all(torch.equal(saved[k], v) for k, v in m.state_dict().items())
    m2 = da.CLIPVisionModelWithProjection.from_pretrained(str(tmp_path / "enc"), torch_dtype=own)
    assert m2.compute_dtype == own and m2.dtype == torch.float32
    assert all(torch.equal(a, b) for a, b in zip(m2.state_dict().values(), m.state_dict().values()))
    assert da.CLIPVisionModelWithProjection.from_pretrained(str(tmp_path / "enc")).compute_dtype == torch.float32
    # the 16-bit mode has no CPU fallback either
    with pytest.raises(da.DfhError, match="no CPU fallback"):
        m2(torch.zeros(1, 3, 56, 56))


@pytest.mark.parametrize("key", ["torch_dtype", "dtype"])
@pytest.mark.parametrize("value", ["float16", "bfloat16", "float32"])
def test_a_checkpoints_own_dtype_key_never_selects_the_mode(tmp_path, key, value):
    """transformers records the dtype of the saved weights in ``config.json`` (``torch_dtype``; ``dtype`` from 4.56 on).  As there, that
    key does not choose the precision of the loaded model: only the caller's ``torch_dtype=`` does, and the fp32 tower stays the default."""
    import json
    m = _tiny(init_seed=3)
    m.save_pretrained(str(tmp_path / "enc"))
    path = tmp_path / "enc" / "config.json"
    cfg = json.load(open(path))
    cfg[key] = value
    json.dump(cfg, open(path, "w"))
    got = da.CLIPVisionModelWithProjection.from_pretrained(str(tmp_path / "enc"))
    assert got.compute_dtype == torch.float32 and got.dtype == torch.float32 and key not in got.config
    assert all(torch.equal(a, b) for a, b in zip(got.state_dict().values(), m.state_dict().values()))
    own = _lib.storage_dtype()
    assert da.CLIPVisionModelWithProjection.from_pretrained(str(tmp_path / "enc"), torch_dtype=own).compute_dtype == own
    assert da.CLIPVisionModelWithProjection.from_pretrained(str(tmp_path), subfolder="enc", torch_dtype=torch.float32).compute_dtype == torch.float32

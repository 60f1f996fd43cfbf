"""CPU tier (-m "not gpu"): the host-only half of the 16-bit CLIP text encoder -- the C ABI of the
``dfh_cliph_*`` family in header, both libraries and ctypes; the plan of the whole encode for every case (every launch's buffers inside
the carved workspace, packed-copy layout, hand-computed sizes of the full-size towers); its refusals; the fixtures' checksums and the
yardstick file; the dtype switch; the resource table of the kernels that existed before.  No compute call is made here: the arithmetic
is checked on the GPU (tests/test_gpu_clip_text_half.py)."""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

import difashion_amd as da
from difashion_amd import _lib
from oracle import clip_ref
from tests.helpers_clip_text_half import (FORMATS, HALF_CASES, YARDSTICKS, case_inputs, checksum, config_kwargs, fixture_path,
                                          kept_rows, kept_taps, load_fixture, output_keys, yardstick)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAMILY = ["dfh_cliph_plan", "dfh_cliph_packed_bytes", "dfh_cliph_pack", "dfh_cliph_workspace_bytes", "dfh_cliph_encode", "dfh_cliph_text_embeds"]
ACT_GELU, ACT_QUICK_GELU = 5, 6
up = lambda n: -(-n // 256) * 256


def _ctx(cfg):
    c = _lib.CLIPConfigC(cfg.vocab_size, cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers, cfg.num_attention_heads,
                         cfg.max_position_embeddings, {"quick_gelu": 1, "gelu": 2}[cfg.hidden_act], cfg.layer_norm_eps)
    h = C.c_void_p()
    _lib.call("dfh_clip_create", C.byref(c), C.byref(h))
    return h


def _plan(h, batch, T):
    p = _lib.CLIPTHalfPlanC()
    _lib.call("dfh_cliph_plan", h, batch, T, C.byref(p))
    return p


def test_every_cliph_symbol_is_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "difashion_hip.h")).read(), flags=re.S)
    assert set(re.findall(r"\b(dfh_cliph_[a-z0-9_]+)\s*\(", src)) == set(FAMILY)
    assert re.search(r"\bdfh_causal_attention\s*\(", src)
    assert "#define DFH_ABI_VERSION 8" in src                                   # additive: the ABI number stays
    for lib_name in _lib._LIB_NAMES.values():                                   # both storage builds carry the walk
        lib = C.CDLL(os.path.join(_lib.CSRC, lib_name))
        for n in FAMILY + ["dfh_causal_attention"]:
            assert hasattr(lib, n), f"{n} not exported by {lib_name}"
    for n in FAMILY + ["dfh_causal_attention"]:
        assert n in _lib.SIGNATURES, n
    # the ctypes mirror follows the header's field order
    body = re.search(r"typedef struct dfh_cliph_plan_info \{(.*?)\} dfh_cliph_plan_info;", src, flags=re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            fields += [re.sub(r"\[.*\]", "", f.strip()) for f in re.sub(r"^[a-z_0-9]+\s+", "", decl).split(",")]
    assert fields == [f[0] for f in _lib.CLIPTHalfPlanC._fields_]
    # the two census counters were appended: the older ids keep their numbers
    names = list(_lib.census())
    assert names[-2:] == ["cliph_attention", "cliph_embed"] and names[-3] == "imgproc"


@pytest.mark.parametrize("name", list(HALF_CASES))
def test_plan_geometry_and_workspace_bounds(name):
    cfg, _, batch, T, _, _ = HALF_CASES[name]
    D, I, H, L = cfg.hidden_size, cfg.intermediate_size, cfg.num_attention_heads, cfg.num_hidden_layers
    h = _ctx(cfg)
    lib = _lib.raw()
    try:
        for B, Tq in ((1, 1), (batch, T), (7, 33)):
            p = _plan(h, B, Tq)
            M = B * Tq
            assert (p.batch, p.tokens, p.hidden, p.intermediate, p.heads, p.head_dim, p.layers, p.rows) == (B, Tq, D, I, H, 64, L, M)
            # two workgroups of the attention kernel fit the 160 KiB of a CU's LDS with room to spare (four do)
            assert p.attention_lds_bytes == (128 * 72 + 64 * 136) * 2 == 35840 and 4 * p.attention_lds_bytes <= 160 * 1024
            Lh = {p.launches[i].name.decode(): p.launches[i] for i in range(p.num_launches)}
            R = [p.regions[i] for i in range(p.num_regions)]
            assert list(Lh) == ["qkv", "out_proj", "fc1", "fc2"]
            gact = ACT_GELU if cfg.hidden_act == "gelu" else ACT_QUICK_GELU
            want = {"qkv": (M, 3 * D, D, 3 * D, 0, 0, 1), "out_proj": (M, D, D, D, 0, 1, 1), "fc1": (M, I, D, I, gact, 0, 1), "fc2": (M, D, I, D, 0, 1, 1)}
            for n, l in Lh.items():
                assert (l.M, l.N, l.K, l.ld_out, l.act, l.resid, l.per_layer) == want[n], n
                assert l.lda == l.K == l.ldw and l.K % 8 == 0 and l.N % 8 == 0 and l.ld_out % 8 == 0, n
                assert l.out2_region == -1 and l.n_split == 0 and l.ld_out2 == 0, n
                # the buffers of the launch lie inside their regions
                assert R[l.a_region].bytes >= l.M * l.lda * 2 and R[l.out_region].bytes >= l.M * l.ld_out * 2, n
            names = [r.name.decode() for r in R]
            assert names == ["zero", "x", "ln", "qkv", "attention", "mlp_hidden", "splitk_partial", "x_fp32", "eos_rows", "pooled"]
            assert [names[Lh[n].a_region] for n in Lh] == ["ln", "attention", "ln", "mlp_hidden"]
            assert [names[Lh[n].out_region] for n in Lh] == ["qkv", "x", "mlp_hidden", "x"]
            # the carve: 256-byte aligned, disjoint, in order, inside the workspace the size query reports
            end = 0
            for r in R:
                assert r.offset % 256 == 0 and r.offset >= end and (r.bytes > 0 or r.name == b"splitk_partial"), r.name
                end = r.offset + r.bytes
            assert end <= p.workspace_bytes == lib.dfh_cliph_workspace_bytes(h, B, Tq) < end + 256       # no slack: the caller aligns the block
            by = dict(zip(names, R))
            assert by["x"].bytes == M * D * 2 and by["qkv"].bytes == M * 3 * D * 2 and by["mlp_hidden"].bytes == M * I * 2
            assert by["x_fp32"].bytes == M * D * 4 and by["eos_rows"].bytes == by["pooled"].bytes == B * D * 4
            # packed copy: per layer four 16-bit matrices and the stacked fp32 q | k | v bias, each 256-byte aligned
            per_layer = up(3 * D * D * 2) + up(D * D * 2) + 2 * up(D * I * 2) + up(3 * D * 4)
            assert p.packed_bytes == lib.dfh_cliph_packed_bytes(h) == L * per_layer and per_layer % 256 == 0
    finally:
        lib.dfh_clip_destroy(h)


def test_plan_pins_the_sizes_of_the_real_towers():
    """Hand-computed: the prompt table (51 x 77) of both full-size towers."""
    lib = _lib.raw()
    # packed weights by hand: 12 x (14 155 776 + 9 216) = 169 979 904 bytes (CLIP-L), 23 x (25 165 824 + 12 288) = 579 096 576 (OpenCLIP-H)
    for cfg, D, I, L, packed in ((clip_ref.SD15_CLIP, 768, 3072, 12, 169_979_904), (clip_ref.SD2_CLIP, 1024, 4096, 23, 579_096_576)):
        h = _ctx(cfg)
        try:
            p = _plan(h, 51, 77)
            M = 51 * 77
            assert M == 3927 and p.rows == M
            partial = p.regions[6].bytes
            assert p.regions[6].name == b"splitk_partial" and partial % 4 == 0
            # zero page + x, ln, attention (M D 16-bit each) + qkv (3 M D) + hidden (M I) + split-K slabs + the fp32 stream + two [51][D] fp32
            want = 256 + 3 * up(M * D * 2) + up(M * 3 * D * 2) + up(M * I * 2) + up(partial) + up(M * D * 4) + 2 * up(51 * D * 4)
            assert p.workspace_bytes == want == lib.dfh_cliph_workspace_bytes(h, 51, 77)
            # every size is a multiple of 256 already: 4 D^2 + 2 D I 16-bit elements and 3 D floats a layer
            assert p.packed_bytes == L * ((4 * D * D + 2 * D * I) * 2 + 3 * D * 4) == packed
        finally:
            lib.dfh_clip_destroy(h)


def test_plan_refuses_what_the_walk_cannot_run():
    lib = _lib.raw()
    fp32 = "the fp32 tower \\(dfh_clip_encode\\) takes this config"
    for cfg, d in ((clip_ref.TINY_CLIP, 16), (clip_ref.TINY_CLIP_GELU, 32)):     # the fp32 tower's tiny configs
        h = _ctx(cfg)
        try:
            with pytest.raises(_lib.DfhError, match=f"built for head dim 64 .*: head dim {d} is not built; {fp32}"):
                _plan(h, 2, 20)
            assert lib.dfh_cliph_workspace_bytes(h, 2, 20) == 0 and lib.dfh_cliph_packed_bytes(h) == 0
            assert lib.dfh_clip_workspace_bytes(h, 2, 20) > 0                    # the fp32 tower still takes it
        finally:
            lib.dfh_clip_destroy(h)
    import dataclasses
    tiny = HALF_CASES["thalf_tiny_77"][0]
    h = _ctx(dataclasses.replace(tiny, max_position_embeddings=128))
    try:
        assert _plan(h, 2, 128).tokens == 128
        for T in (129, 0, -1):
            with pytest.raises(_lib.DfhError, match=rf"sequence length must be in \[1, 128\], got {T}; {fp32}"):
                _plan(h, 2, T)
        assert lib.dfh_cliph_workspace_bytes(h, 2, 129) == 0
        with pytest.raises(_lib.DfhError, match="batch must be in"):
            _plan(h, 0, 77)
    finally:
        lib.dfh_clip_destroy(h)
    h = _ctx(tiny)                                                               # 77 positions: the config's own limit comes first
    try:
        with pytest.raises(_lib.DfhError, match=rf"sequence length must be in \[1, 77\], got 78; {fp32}"):
            _plan(h, 2, 78)
    finally:
        lib.dfh_clip_destroy(h)
    h = _ctx(dataclasses.replace(tiny, hidden_size=132))                         # 2 heads of 66: rows that are no 16-byte multiples
    try:
        with pytest.raises(_lib.DfhError, match=f"multiples of 8 .*got 132 / 256; {fp32}"):
            _plan(h, 2, 20)
        assert lib.dfh_cliph_workspace_bytes(h, 2, 20) == 0 and lib.dfh_clip_workspace_bytes(h, 2, 20) > 0
    finally:
        lib.dfh_clip_destroy(h)
    h = _ctx(dataclasses.replace(tiny, intermediate_size=260))
    try:
        with pytest.raises(_lib.DfhError, match="multiples of 8 .*got 128 / 260"):
            _plan(h, 2, 20)
    finally:
        lib.dfh_clip_destroy(h)


def test_encode_entry_points_check_their_pointers_before_any_launch():
    """Host-only: null and alignment checks of dfh_cliph_encode / _text_embeds / _pack / dfh_causal_attention (no GPU is touched)."""
    cfg = HALF_CASES["thalf_tiny_20"][0]
    h = _ctx(cfg)
    lib = _lib.raw()
    try:
        n = lib.dfh_clip_num_params(h)
        good = (C.c_void_p * n)(*([4096] * n))
        buf, need = C.c_void_p(4096), lib.dfh_cliph_workspace_bytes(h, 2, 16)
        enc = lambda arr, cnt, packed=buf, ws=buf, last=buf, nbytes=need: _lib.call(
            "dfh_cliph_encode", h, arr, cnt, packed, buf, last, None, 2, None, ws, nbytes, 2, 16, None)
        with pytest.raises(_lib.DfhError, match="count does not match dfh_clip_num_params"):
            enc(good, n - 1)
        with pytest.raises(_lib.DfhError, match="null argument"):
            enc(good, n, packed=None)
        with pytest.raises(_lib.DfhError, match="null parameter pointer"):
            enc((C.c_void_p * n)(*([4096] * (n - 1) + [0])), n)
        with pytest.raises(_lib.DfhError, match="not 16-byte aligned"):
            enc((C.c_void_p * n)(*([4096] * (n - 1) + [4100])), n)
        with pytest.raises(_lib.DfhError, match="workspace smaller than dfh_cliph_workspace_bytes"):
            enc(good, n, nbytes=need - 1)
        with pytest.raises(_lib.DfhError, match="256-byte aligned"):
            enc(good, n, ws=C.c_void_p(4096 + 64))
        with pytest.raises(_lib.DfhError, match="256-byte aligned"):
            enc(good, n, packed=C.c_void_p(4096 + 128))
        with pytest.raises(_lib.DfhError, match="outputs must be 16-byte aligned"):
            enc(good, n, last=C.c_void_p(4096 + 8))
        with pytest.raises(_lib.DfhError, match="sequence length must be in"):
            _lib.call("dfh_cliph_encode", h, good, n, buf, buf, buf, None, 2, None, buf, need, 2, 78, None)
        emb = lambda proj=buf, pdim=64: _lib.call("dfh_cliph_text_embeds", h, good, n, buf, proj, pdim, buf, buf, None, None, 2, None, buf, need, 2, 16, None)
        with pytest.raises(_lib.DfhError, match="null argument"):
            emb(proj=None)
        with pytest.raises(_lib.DfhError, match="projection_dim must be positive"):
            emb(pdim=0)
        with pytest.raises(_lib.DfhError, match="text_projection must be 16-byte aligned"):
            emb(proj=C.c_void_p(4100))
        with pytest.raises(_lib.DfhError, match="packed copy must be 256-byte aligned"):
            _lib.call("dfh_cliph_pack", h, good, n, C.c_void_p(4096 + 16), None)
        with pytest.raises(_lib.DfhError, match="null argument"):
            _lib.call("dfh_causal_attention", None, buf, 1, 8, 1, 64, 0.125, None)
        with pytest.raises(_lib.DfhError, match="16-byte aligned"):
            _lib.call("dfh_causal_attention", C.c_void_p(4098), buf, 1, 8, 1, 64, 0.125, None)
    finally:
        lib.dfh_clip_destroy(h)


@pytest.mark.parametrize("name", list(HALF_CASES))
def test_fixtures_hold_the_seeded_inputs_and_rows(name):
    cfg, params, proj, ids = case_inputs(name)
    fx = load_fixture(name)
    np.testing.assert_allclose(fx["checksum"], checksum(params, proj, ids), rtol=1e-12)
    assert np.array_equal(fx["input_ids"], ids.numpy())
    B, T, D, L = ids.shape[0], ids.shape[1], cfg.hidden_size, cfg.num_hidden_layers
    rows = kept_rows(cfg, ids)
    assert list(fx["rows"]) == rows and list(fx["taps"]) == kept_taps(name) and 0 in rows and T - 1 in rows
    if T > 64:
        assert {0, 1, 15, 16, 31, 32, 63, 64, T - 2, T - 1} <= set(rows) and len(rows) <= 10 + B
    else:
        assert rows == list(range(T))
    assert fx["text_embeds"].shape == (B, proj.shape[0]) and fx["pooler_output"].shape == (B, D)
    for k in ["last_hidden_state"] + [f"hidden_{t}" for t in kept_taps(name)]:
        assert fx[k].shape == (B, len(rows), D) and fx[k].dtype == np.float32 and np.isfinite(fx[k]).all(), k
    assert os.path.getsize(fixture_path(name)) < 1 << 20


def test_yardstick_file_covers_every_case_output_and_format():
    ys = dict(np.load(YARDSTICKS))
    for name in HALF_CASES:
        fx = load_fixture(name)
        np.testing.assert_allclose(ys[f"{name}/checksum"], fx["checksum"], rtol=1e-12)
        for fmt in FORMATS:
            for key in output_keys(fx) + ["cos"]:
                v = yardstick(ys, name, fmt, key)
                assert np.isfinite(v) and 0 < v < 5e-2, (name, fmt, key, v)
        # what the formats are: fp16 carries 3 more mantissa bits than bf16
        assert yardstick(ys, name, "fp16", "last_hidden_state") < 0.3 * yardstick(ys, name, "bf16", "last_hidden_state")
    # the full-size towers, as the real class measures them here
    assert 1.5e-2 < yardstick(ys, "sd2_openclip_h", "bf16", "last_hidden_state") < 2.0e-2 and yardstick(ys, "sd2_openclip_h", "bf16", "cos") < 1e-3
    assert os.path.getsize(YARDSTICKS) < 64 << 10


def _tiny(cls=da.CLIPTextModel, **kw):
    extra = dict(projection_dim=32) if cls is da.CLIPTextModelWithProjection else {}
    return cls(**config_kwargs(HALF_CASES["thalf_tiny_20"][0]), **extra, **kw)


@pytest.mark.parametrize("cls", [da.CLIPTextModel, da.CLIPTextModelWithProjection])
def test_compute_dtype_switch_never_casts_a_parameter(cls):
    own, other = _lib.storage_dtype(), (torch.float16 if _lib.storage() == "bf16" else torch.bfloat16)
    m = _tiny(cls)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    assert m.compute_dtype == torch.float32 and m.dtype == torch.float32
    routes = {torch.bfloat16: m.bfloat16, torch.float16: m.half}
    assert routes[own]() is m and m.compute_dtype == own
    assert m.float() is m and m.compute_dtype == torch.float32
    assert m.to(dtype=own) is m and m.compute_dtype == own and m.to(torch.float32).compute_dtype == torch.float32
    assert m.to(own).compute_dtype == own and m.to("cpu", own).compute_dtype == own
    assert m.set_compute_dtype(torch.float32).compute_dtype == torch.float32
    assert _tiny(cls, torch_dtype=own).compute_dtype == own and _tiny(cls, torch_dtype=None).compute_dtype == torch.float32
    for mode in (own, torch.float32):
        m.set_compute_dtype(mode)
        sd = m.state_dict()
        assert m.dtype == torch.float32 and all(p.dtype == torch.float32 for p in m.parameters())
        assert list(sd) == list(before) and all(torch.equal(sd[k], before[k]) and sd[k].dtype == torch.float32 for k in sd)
    # the other 16-bit format: refused, the message says whose property the format is
    for route in (routes[other], lambda: m.to(dtype=other), lambda: m.set_compute_dtype(other), lambda: _tiny(cls, torch_dtype=other)):
        with pytest.raises(da.DfhError, match=r"property of the process \(DFH_STORAGE / set_storage\(\)") as e:
            route()
        assert "stay fp32" in str(e.value)
    assert m.compute_dtype == torch.float32
    with pytest.raises(da.DfhError, match=f"{cls.__name__} computes in float32 or in"):
        m.double()
    with pytest.raises(TypeError, match="floating torch.dtype"):
        m.set_compute_dtype(torch.int32)


def test_unsupported_configs_are_refused_when_the_mode_is_enabled():
    m = da.CLIPTextModel(**config_kwargs(clip_ref.TINY_CLIP))                    # head dim 16: fine in fp32
    with pytest.raises(da.DfhError, match="head dim 16 is not built; the fp32 tower"):
        m.set_compute_dtype(_lib.storage_dtype())
    assert m.compute_dtype == torch.float32
    with pytest.raises(da.DfhError, match="head dim 32"):
        da.CLIPTextModel(**config_kwargs(clip_ref.TINY_CLIP_GELU), torch_dtype=_lib.storage_dtype())


def test_checkpoints_stay_fp32_and_from_pretrained_takes_torch_dtype(tmp_path):
    own = _lib.storage_dtype()
    for cls in (da.CLIPTextModel, da.CLIPTextModelWithProjection):
        d = str(tmp_path / cls.__name__)
        m = _tiny(cls, init_seed=3, torch_dtype=own)
        m.save_pretrained(d)
        from safetensors.torch import load_file
        cfg = json.load(open(os.path.join(d, "config.json")))
        assert "torch_dtype" not in cfg and cfg["hidden_size"] == 128
        saved = load_file(os.path.join(d, "model.safetensors"))
        assert all(v.dtype == torch.float32 for v in saved.values()) and not any("packed" in k for k in saved)
        assert all(torch.equal(saved[k], v) for k, v in m.state_dict().items())
        m2 = cls.from_pretrained(d, torch_dtype=own)
        assert m2.compute_dtype == own and m2.dtype == torch.float32
        assert all(torch.equal(a, b) for a, b in zip(m2.state_dict().values(), m.state_dict().values()))
        assert cls.from_pretrained(d).compute_dtype == torch.float32
        # a checkpoint's own dtype key (the dtype of the saved weights) never selects the mode
        for key, value in (("torch_dtype", "float16"), ("dtype", "bfloat16")):
            cfg2 = dict(cfg, **{key: value})
            json.dump(cfg2, open(os.path.join(d, "config.json"), "w"))
            got = cls.from_pretrained(d)
            assert got.compute_dtype == torch.float32 and key not in got.config
            assert cls.from_pretrained(d, torch_dtype=own).compute_dtype == own
        # the 16-bit mode has no CPU fallback either
        with pytest.raises(da.DfhError, match="no CPU fallback"):
            m2(torch.zeros(1, 8, dtype=torch.long))


def test_from_pretrained_pipeline_forwards_text_encoder_dtype(monkeypatch):
    """``DiFashion.from_pretrained_pipeline(text_encoder_dtype=...)`` hands the dtype to ``CLIPTextModel.from_pretrained`` as
    ``torch_dtype=``; the default ``None`` is today's call."""
    import inspect
    from difashion_amd.difashion import DiFashion
    sig = inspect.signature(DiFashion.from_pretrained_pipeline)
    assert sig.parameters["text_encoder_dtype"].default is None
    seen = {}

    class Stop(Exception):
        pass

    def fake(path, **kw):
        seen.update(kw)
        raise Stop

    monkeypatch.setattr(da.CLIPTextModel, "from_pretrained", staticmethod(fake))
    import types
    from difashion_amd import schedulers
    monkeypatch.setattr(schedulers.PNDMScheduler, "from_pretrained", classmethod(lambda cls, *a, **k: None))
    args = types.SimpleNamespace(pretrained_model_name_or_path="/nonexistent", revision=None)
    for dtype in (None, _lib.storage_dtype()):
        seen.clear()
        with pytest.raises(Stop):
            DiFashion.from_pretrained_pipeline(args, tokenizer=object(), text_encoder_dtype=dtype)
        assert seen["torch_dtype"] is dtype and seen["subfolder"] == "text_encoder"


def test_new_kernels_use_no_scratch_and_the_resource_table_is_recorded():
    """The new kernels, from the code objects of both libraries: no spilled VGPR, no scratch; the attention kernel's static LDS is what
    the plan reports, and its registers leave room for two workgroups (8 waves) a CU and more.  The comparison of every kernel that
    existed before against the parent commit's build -- VGPR / AGPR / SGPR / spills / scratch / LDS, both libraries -- is recorded in
    profiles/clip_text_half_resources.txt (as profiles/clip_vision_half_resources.txt records the image tower's): no kernel missing, no
    resource changed."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        from kernel_resources import object_kernels
    finally:
        sys.path.pop(0)
    table = open(os.path.join(ROOT, "profiles", "clip_text_half_resources.txt")).read()
    for lib, sub in (("bf16", ""), ("obj_f16", "obj_f16")):
        head = re.search(r"^\[%s\] parent kernels (\d+), now (\d+); missing 0; resource changes 0$" % lib, table, flags=re.M)
        assert head and int(head.group(2)) == int(head.group(1)) + 5, lib
        new = dict(object_kernels(os.path.join(_lib.CSRC, sub, "clip_text_half.o")))
        assert len(new) == 5 and all("cliph_" in k for k in new), sorted(new)
        for k, c in new.items():
            assert c["vgpr_spill_count"] == 0 and c["private_segment_fixed_size"] == 0 and c.get("sgpr_spill_count", 0) == 0, (lib, k, c)
            assert k in table, k
        attn = [c for k, c in new.items() if "cliph_causal_attention_kernel" in k]
        assert len(attn) == 1 and attn[0]["group_segment_fixed_size"] == 35840 and attn[0]["vgpr_count"] + attn[0]["agpr_count"] <= 128, attn

"""-m gpu: the 16-bit (bf16 / fp16) CLIP image encoder (csrc/clip_vision_half.hip behind
``CLIPVisionModelWithProjection(torch_dtype=...)`` / ``.half()`` / ``.bfloat16()``).

The rule is the project's own (rows f5 / f6 / f8 / f9): the HIP 16-bit path's distance from the fp64 values of the REAL
``transformers.CLIPVisionModelWithProjection`` must be at most 3 x the real class's own distance when it runs in the same 16-bit
format (tests/golden/clipv_half_yardsticks.npz, written by tests/golden/make_golden_clip_vision_half.py) -- for ``image_embeds``,
``pooler_output``, ``last_hidden_state``, every tap, and for the maximum of 1 - cos over the images' ``image_embeds``.  bf16 runs in
this process, fp16 in a fresh child under ``DFH_STORAGE=fp16`` (a process holds one storage format).  The measurements themselves and
the derivation of the op-level bounds are in tests/clip_vision_half_child.py; every figure is printed before it is asserted
(profiles/clip_vision_half_parity.txt holds one run's)."""
import functools
import json
import os
import subprocess
import sys

import pytest
import torch

import difashion_amd as da
from difashion_amd import _lib
from tests import clip_vision_half_child as measure
from tests.gpu_util import DEV, release_cached_gpu_memory
from tests.helpers_clip_vision import TINY_GELU, rel
from tests.helpers_clip_vision_half import FACTOR, HALF_CASES, YARDSTICKS, case_inputs, pixel_inputs, yardstick

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = lambda case: "x".join(map(str, case))


def _assert_parity(name, fmt, rec):
    assert all(rec["facts"].values()), (name, fmt, rec["facts"])
    for k, (e, r) in rec["dist"].items():                                       # every output, every tap, the cosine: none excused
        assert e <= FACTOR * r, (name, fmt, k, e, r)
    # which kernels ran: one 16-bit attention launch per block, none of the fp32 tower's attention kernel
    c, L = rec["census"], rec["layers"]
    assert c["attention_16"] + c["attention_x32"] == L and c["clipv_attention"] == 0 and c["layernorm"] == 2 * L and c["clipv_embed"] == 1, c
    cfg = HALF_CASES[name][0]
    x32 = cfg.hidden_size // cfg.num_attention_heads == 80 and cfg.num_tokens >= 256
    assert c["attention_x32"] == (L if x32 else 0), c


def _assert_op(kind, key, fmt, rec):
    assert rec["finite"] and rec["bands_untouched"] and rec["rerun_identical"], (kind, key, fmt, rec)
    assert rec["worst_ratio"] <= 1.0, (kind, key, fmt, rec)
    if kind == "gemm":
        assert rec["lean_tile"], (key, fmt, rec)


@pytest.mark.parametrize("name", list(HALF_CASES))
def test_bf16_encoder_within_three_times_the_real_class(name):
    assert _lib.storage() == "bf16"
    _assert_parity(name, "bf16", measure.parity(name))


@functools.lru_cache(maxsize=None)
def _fp16_child():
    assert _lib.storage() == "bf16"
    release_cached_gpu_memory()
    env = dict(os.environ, DFH_STORAGE="fp16")
    env.pop("DFH_LIB", None)
    r = subprocess.run([sys.executable, "-m", "tests.clip_vision_half_child"], capture_output=True, text=True, env=env, cwd=ROOT, timeout=900)
    print("\n".join(l for l in r.stdout.splitlines() if l.startswith("clipvh ")))      # the child's figures, before anything is asserted
    lines = [l for l in r.stdout.splitlines() if l.startswith("CLIPVH_RESULT ")]
    assert r.returncode == 0 and lines, f"the fp16 child ended with status {r.returncode}:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    res = json.loads(lines[-1][len("CLIPVH_RESULT "):])
    assert res["storage"] == "fp16" and "storage=fp16" in res["build_info"], res["build_info"]
    return res


@pytest.mark.timeout(900)
def test_fp16_encoder_and_ops_in_a_child_process():
    res = _fp16_child()
    assert sorted(res["parity"]) == sorted(HALF_CASES)
    for name, rec in res["parity"].items():
        _assert_parity(name, "fp16", rec)
    assert sorted(res["attention"]) == sorted(KEY(c) for c in measure.ATTENTION_CASES) and len(res["gemm"]) == 12
    for key, rec in res["attention"].items():
        _assert_op("attention", key, "fp16", rec)
    for key, rec in res["gemm"].items():
        _assert_op("gemm", key, "fp16", rec)


@pytest.mark.parametrize("case", measure.ATTENTION_CASES, ids=KEY)
def test_attention_at_ragged_lengths(case):
    rec = measure.attention_check(*case)
    _assert_op("attention", KEY(case), "bf16", rec)
    B, H, d, N = case
    assert rec["x32"] == (d == 80 and N >= 256)                                  # the dispatch at these lengths


@pytest.mark.parametrize("with_resid", [False, True], ids=["bias", "bias_resid"])
@pytest.mark.parametrize("act", [5, 6], ids=["gelu", "quick_gelu"])
@pytest.mark.parametrize("M", measure.GEMM_ROWS)
def test_gemm_activation_epilogues_at_ragged_rows(M, act, with_resid):
    _assert_op("gemm", f"{M}x{act}x{int(with_resid)}", "bf16", measure.gemm_check(M, act, with_resid))


def _model(name, dtype=None):
    cfg, params, pixels = case_inputs(name)
    return cfg, measure.hip_model(cfg, params, dtype), pixels.to(DEV)


def _all(out):
    return out.to_tuple()[:2] + tuple(out.hidden_states) + (out.pooler_output,)


def test_reruns_round_trips_and_repacks():
    own = _lib.storage_dtype()
    cfg, m, px = _model("half_tiny_d80")
    _, untouched, _ = _model("half_tiny_d80")
    want32 = _all(untouched(px, output_hidden_states=True))
    half = _all(m.set_compute_dtype(own)(px, output_hidden_states=True))
    assert all(torch.equal(a, b) for a, b in zip(half, _all(m(px, output_hidden_states=True))))        # a rerun is bit-identical
    assert not torch.equal(half[0], want32[0])
    # .bfloat16() -> .float(): the fp32 tower's bits again, and the masters never moved
    packed = m._packed
    back = _all(m.float()(px, output_hidden_states=True))
    assert all(torch.equal(a, b) for a, b in zip(back, want32))
    assert m._packed is packed and m._packed_sig is not None                     # the switch keeps the packed copy: nothing to remake on the way back
    assert all(p.dtype == torch.float32 for p in m.parameters()) and all(v.dtype == torch.float32 for v in m.state_dict().values())
    # a parameter update between two 16-bit calls is seen: the packed copy is remade
    m.set_compute_dtype(own)
    assert torch.equal(m(px).image_embeds, half[0])
    layers = m.vision_model.encoder.layers._modules                            # bare containers named "0", "1", ...
    saved = layers["1"].mlp.fc2.weight.detach().clone()
    with torch.no_grad():
        layers["1"].mlp.fc2.weight.mul_(1.5)
    moved = m(px)
    assert not torch.equal(moved.image_embeds, half[0]) and not torch.equal(moved.last_hidden_state, half[1])
    with torch.no_grad():
        layers["1"].mlp.fc2.weight.copy_(saved)
    assert torch.equal(m(px).image_embeds, half[0])                              # the old weights again: the old bits again
    with torch.no_grad():
        layers["0"].self_attn.q_proj.bias.add_(0.25)        # the stacked q | k | v bias is part of the copy
    assert not torch.equal(m(px).image_embeds, half[0])


def test_batch_of_one_agrees_with_the_batch_within_the_rule():
    """Not bitwise: the GEMM plan (tile, K split) depends on M = batch x tokens, so the summation order may differ."""
    import numpy as np
    own, fmt = _lib.storage_dtype(), _lib.storage()
    ys = dict(np.load(YARDSTICKS))
    for name in ("half_tiny_d64", "half_tiny_d80"):
        cfg, m, _ = _model(name, own)
        px = pixel_inputs(cfg, 3, 77).to(DEV)
        full = m(px, output_hidden_states=True)
        for b in range(3):
            one = m(px[b:b + 1], output_hidden_states=True)
            pairs = {"image_embeds": (one.image_embeds, full.image_embeds[b:b + 1]), "pooler_output": (one.pooler_output, full.pooler_output[b:b + 1]),
                     "last_hidden_state": (one.last_hidden_state, full.last_hidden_state[b:b + 1])}
            pairs.update({f"hidden_{t}": (one.hidden_states[t], full.hidden_states[t][b:b + 1]) for t in range(cfg.num_hidden_layers + 1)})
            for k, (a, f) in pairs.items():
                e, r = rel(a, f), yardstick(ys, name, fmt, k)
                assert e <= FACTOR * r, (name, b, k, e, r)


def test_evaluation_functions_take_a_half_precision_tower(tmp_path):
    own = _lib.storage_dtype()
    cfg, m, px = _model("half_tiny_short", own)
    m.save_pretrained(str(tmp_path / "enc"))
    from safetensors.torch import load_file
    assert all(v.dtype == torch.float32 for v in load_file(str(tmp_path / "enc" / "model.safetensors")).values())
    m2 = da.CLIPVisionModelWithProjection.from_pretrained(str(tmp_path / "enc"), torch_dtype=own).to(DEV)
    assert m2.compute_dtype == own and all(v.dtype == torch.float32 for v in m2.state_dict().values())
    assert torch.equal(m2(px).image_embeds, m(px).image_embeds)
    import numpy as np
    S = cfg.image_size
    proc = da.CLIPImageProcessor(size={"shortest_edge": S}, crop_size={"height": S, "width": S})
    images = torch.from_numpy(np.random.default_rng(5).integers(0, 256, (3, 70, 90, 3)).astype(np.uint8)).to(DEV)
    feats = da.extract_image_features(m2, proc, images, batch_size=3)
    assert feats.dtype == torch.float32 and feats.shape == (3, cfg.projection_dim) and torch.isfinite(feats).all()
    assert torch.equal(feats, m2.encode_image(proc(images=images).pixel_values))
    # ... and they are the 16-bit tower's features, not the fp32 tower's bits
    assert not torch.equal(da.extract_image_features(m2.float(), proc, images, batch_size=3), feats)


def test_error_behaviour():
    own, other = _lib.storage_dtype(), (torch.float16 if _lib.storage() == "bf16" else torch.bfloat16)
    cfg, m, px = _model("half_tiny_short", own)
    with pytest.raises(da.DfhError, match="property of the process"):
        m.set_compute_dtype(other)
    with pytest.raises(da.DfhError, match="property of the process"):
        m.to(dtype=other)
    assert m.compute_dtype == own
    with pytest.raises(TypeError, match=f"float32 or {own}"):
        m(px.to(other))                                                          # pixels in the other 16-bit format
    with pytest.raises(TypeError, match=f"float32 or {own}"):
        m(px.double())
    with pytest.raises(da.DfhError, match="no CPU fallback"):
        m(px.cpu())                                                              # pixels on the wrong device
    with pytest.raises(TypeError, match="float32"):
        m.float()(px.to(own))                                                    # fp32 mode takes fp32 pixels only, as before
    # an unsupported head dim: the old tiny_gelu config (head dim 16) stays an fp32-only tower
    from tests.helpers_clip_vision import case_inputs as fp32_case
    tcfg, tparams, tpx = fp32_case("tiny_gelu")
    t = measure.hip_model(tcfg, tparams, None)
    with pytest.raises(da.DfhError, match="head dims 32, 40, 64, 80, 128, 160"):
        t.set_compute_dtype(own)
    assert t.compute_dtype == torch.float32 and torch.isfinite(t(tpx.to(DEV)).image_embeds).all()
    assert TINY_GELU.hidden_size // TINY_GELU.num_attention_heads == 16

"""-m gpu: the HIP CLIP image encoder (csrc/clip_vision.hip behind ``difashion_amd.CLIPVisionModelWithProjection``)
against fixtures that the REAL ``transformers.CLIPVisionModelWithProjection`` produced in fp64 (tests/golden/make_golden_clip_vision.py)
-- the architecture of the OpenCLIP ViT-H/14 whose ``encode_image`` the reference's evaluation calls (Evaluation/extract_hist_embs.py:83-100,
Evaluation/eval_utils.py:91-135, :503-535).  Weights and pixels are regenerated from the case's seed; the fixture's checksum proves they are
the same tensors.

Stated tolerance: the fixture records, per output and per tap, how far the third-party class run in fp32 sits from its own fp64 run
(``ref_*``, relative L2).  The HIP encoder, fp32 end to end, must sit within 3 x that distance of the same fp64 values: the factor covers
another summation order (16x16x4 MFMA) and other exp / erf implementations; a kernel bug (wrong tile edge, missing key) is orders of
magnitude above it.  The attention kernel alone is held to the same rule against fp32 torch's distance to fp64 torch.  Every measured
distance is printed before it is asserted (profiles/clip_vision_parity.txt holds one run's)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import difashion_amd as da
from difashion_amd import _lib
from tests.gpu_util import DEV
from tests.helpers_clip_vision import CASES, TINY_CASES, case_inputs, checksum, load_fixture, rel, rows_of

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTOR = 3.0


def hip_clipv(cfg, params):
    m = da.CLIPVisionModelWithProjection(**cfg.kwargs(), init_seed=None)
    m.load_state_dict(params)
    return m.to(DEV).eval().requires_grad_(False)


@pytest.mark.parametrize("name", list(CASES))
def test_hip_encoder_matches_the_real_transformers_class(name):
    cfg, params, pixels = case_inputs(name)
    fx = load_fixture(name)
    np.testing.assert_allclose(fx["checksum"], checksum(params, pixels), rtol=1e-12)
    m = hip_clipv(cfg, params)
    del params
    out = m(pixels.to(DEV), output_hidden_states=True)
    B, T, D = pixels.shape[0], cfg.num_tokens, cfg.hidden_size
    assert out.last_hidden_state.shape == (B, T, D) and out.pooler_output.shape == (B, D) and out.image_embeds.shape == (B, cfg.projection_dim)
    assert all(t.dtype == torch.float32 and t.device.type == "cuda" for t in (out.image_embeds, out.last_hidden_state, out.pooler_output))
    assert len(out.hidden_states) == cfg.num_hidden_layers + 1 and torch.equal(out.hidden_states[-1], out.last_hidden_state)
    got = {"last_hidden_state": rows_of(fx, out.last_hidden_state.cpu()), "pooler_output": out.pooler_output.cpu(), "image_embeds": out.image_embeds.cpu()}
    for t in fx["taps"]:
        got[f"hidden_{int(t)}"] = rows_of(fx, out.hidden_states[int(t)].cpu())
    dist = {k: (rel(v, torch.from_numpy(fx[k])), float(fx["ref_" + k])) for k, v in got.items()}
    print("clipv parity", name, " ".join(f"{k}: hip {e:.2e} ref_fp32 {r:.2e} ratio {e / r:.2f};" for k, (e, r) in dist.items()))
    for k, (e, r) in dist.items():
        assert e <= FACTOR * r, (name, k, e, r)
    # the call forms: tuple indexing as in transformers, encode_image, reruns bit-identical (no atomics)
    again = m(pixels.to(DEV))
    assert again.hidden_states is None and torch.equal(again[0], out.image_embeds) and torch.equal(again[1], out.last_hidden_state)
    assert len(again) == 2 and len(out) == 3 and out[2] is out.hidden_states
    assert torch.equal(m(pixels.to(DEV), return_dict=False)[0], out.image_embeds)
    assert torch.equal(m.encode_image(pixels.to(DEV)), out.image_embeds)
    assert torch.equal(again.pooler_output, out.pooler_output)


def attention_reference(qkv, B, T, H, d, scale, dtype):
    q, k, v = (t.reshape(B, T, H, d).transpose(1, 2) for t in qkv.to(dtype).reshape(B * T, 3, H * d).unbind(1))
    return (torch.softmax(q @ k.transpose(-1, -2) * scale, dim=-1) @ v).transpose(1, 2).reshape(B * T, H * d)


# the issue's grid, plus head dims that are not a multiple of 16 / the largest one at ragged lengths
ATTENTION_CASES = [(T, d) for d in (64, 80) for T in (2, 50, 64, 65, 197, 257, 577, 1025)] + [(T, d) for d in (20, 128) for T in (65, 257)]


@pytest.mark.parametrize("T,d", ATTENTION_CASES)
def test_attention_kernel_alone(T, d):
    B, H = 2, 3
    g = torch.Generator().manual_seed(1000 * d + T)
    qkv = torch.randn(B * T, 3 * H * d, generator=g)
    qkv[:, :H * d] *= 1.5                                       # peaked, not one-hot, softmaxes
    scale = d ** -0.5
    want = attention_reference(qkv, B, T, H, d, scale, torch.float64)
    ref = rel(attention_reference(qkv, B, T, H, d, scale, torch.float32), want)
    dev_qkv = qkv.to(DEV)
    out = torch.full((B * T + 1, H * d), float("nan"), device=DEV)          # one guard row behind the output
    _lib.call("dfh_clipv_attention", _lib.ptr(dev_qkv), _lib.ptr(out), B, T, H, d, scale, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert torch.isnan(out[-1]).all()
    e = rel(out[:-1].cpu(), want)
    print(f"clipv attention T={T} d={d}: hip {e:.2e} torch_fp32 {ref:.2e} ratio {e / ref:.2f}")
    assert e <= FACTOR * ref, (T, d, e, ref)
    out2 = torch.empty_like(out)
    _lib.call("dfh_clipv_attention", _lib.ptr(dev_qkv), _lib.ptr(out2), B, T, H, d, scale, _lib.stream_ptr())
    assert torch.equal(out2[:-1], out[:-1])


def test_batch_independence_and_determinism():
    cfg, params, _ = case_inputs("tiny_long")
    m = hip_clipv(cfg, params)
    from tests.helpers_clip_vision import pixel_inputs
    px = pixel_inputs(cfg, 4, 77).to(DEV)
    full = m(px, output_hidden_states=True)
    again = m(px, output_hidden_states=True)
    for a, b in zip(full.to_tuple()[:2] + full.hidden_states + (full.pooler_output,), again.to_tuple()[:2] + again.hidden_states + (again.pooler_output,)):
        assert torch.equal(a, b)
    for b in range(4):
        one = m(px[b:b + 1])
        assert torch.equal(one.image_embeds, full.image_embeds[b:b + 1]) and torch.equal(one.last_hidden_state, full.last_hidden_state[b:b + 1])
        assert torch.equal(one.pooler_output, full.pooler_output[b:b + 1])


def test_error_behaviour():
    cfg, params, pixels = case_inputs("tiny_gelu")
    m = hip_clipv(cfg, params)
    with pytest.raises(ValueError, match="specify pixel_values"):
        m()
    with pytest.raises(da.DfhError, match="no CPU fallback"):
        m(pixels)                                                            # CPU pixels, model on the GPU
    with pytest.raises(da.DfhError, match="no CPU fallback"):
        hip_clipv(cfg, params).cpu()(pixels)
    with pytest.raises(TypeError, match="float32"):
        m(pixels.to(DEV).half())
    with pytest.raises(ValueError, match="doesn't match model"):
        m(torch.zeros(1, 3, 56, 56, device=DEV))
    with pytest.raises(ValueError, match="num_channels"):
        m(torch.zeros(1, 1, 42, 42, device=DEV))
    with pytest.raises(NotImplementedError):
        m(pixels.to(DEV), attention_mask=torch.ones(3, 10, device=DEV))
    with pytest.raises(NotImplementedError):
        m(pixels.to(DEV), interpolate_pos_encoding=True)
    with pytest.raises(da.DfhError, match="stay fp32"):
        hip_clipv(cfg, params).half()(pixels.to(DEV).half())
    assert m.dtype == torch.float32 and m.device.type == "cuda" and not any(p.requires_grad for p in m.parameters())


def test_checkpoint_round_trip_on_the_device(tmp_path):
    cfg, params, pixels = case_inputs("tiny_quickgelu")
    m = hip_clipv(cfg, params)
    want = m(pixels.to(DEV))
    m.save_pretrained(str(tmp_path / "image_encoder"))
    m2 = da.CLIPVisionModelWithProjection.from_pretrained(str(tmp_path), subfolder="image_encoder").to(DEV)
    assert m2.config.hidden_act == "quick_gelu" and m2.config.image_size == 56
    got = m2(pixels.to(DEV))
    assert torch.equal(got.image_embeds, want.image_embeds) and torch.equal(got.last_hidden_state, want.last_hidden_state)


def test_launch_census_of_one_encode():
    cfg, params, pixels = case_inputs("tiny_gelu")
    m = hip_clipv(cfg, params)
    _lib.census_reset()
    m(pixels.to(DEV))
    c = _lib.census()
    L = cfg.num_hidden_layers
    assert c["clipv_embed"] == 1 and c["clipv_attention"] == L and c["clipv_linear"] == 6 * L + 1 and c["clipv_layernorm"] == 2 * L + 2


@pytest.mark.timeout(600)
def test_fp16_library_gives_the_same_bits_on_the_tiny_cases():
    """The row is fp32 in both storage builds: under DFH_STORAGE=fp16 (a fresh child process: the storage format is fixed per process)
    every output of the tiny cases has the bits the default library gives."""
    assert _lib.storage() == "bf16"
    from tests.clip_vision_child import digests
    here = {name: digests(name) for name in TINY_CASES}
    from tests.gpu_util import release_cached_gpu_memory
    release_cached_gpu_memory()
    env = dict(os.environ, DFH_STORAGE="fp16")
    env.pop("DFH_LIB", None)
    r = subprocess.run([sys.executable, "-m", "tests.clip_vision_child"], capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    lines = [l for l in r.stdout.splitlines() if l.startswith("CLIPV_RESULT ")]
    assert r.returncode == 0 and lines, f"the fp16 child ended with status {r.returncode}:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    res = json.loads(lines[-1][len("CLIPV_RESULT "):])
    assert res["storage"] == "fp16" and "storage=fp16" in res["build_info"], res
    for name in TINY_CASES:
        assert res[name] == here[name], name

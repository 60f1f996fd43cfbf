"""-m gpu: the 16-bit (bf16 / fp16) CLIP text encoder (csrc/clip_text_half.hip behind
``CLIPTextModel(torch_dtype=...)`` / ``CLIPTextModelWithProjection`` / ``.half()`` / ``.bfloat16()``).

The rule is the project's own (rows f5 / f6 / f8 / f9): the HIP 16-bit path's distance from the fp64 values of the REAL
``transformers.CLIPTextModel`` / ``CLIPTextModelWithProjection`` must be at most 3 x the real class's own distance when it runs in the
same 16-bit format (tests/golden/clipt_half_yardsticks.npz, written by tests/golden/make_golden_clip_text_half.py) -- for
``text_embeds``, ``pooler_output``, ``last_hidden_state``, every stored tap, and for the maximum of 1 - cos over the sequences'
``text_embeds``.  bf16 runs in this process, fp16 in ONE fresh child under ``DFH_STORAGE=fp16`` (a process holds one storage format)
whose outcome, failure included, is kept and never retried.  The measurements themselves and the derivation of the op-level bound are in
tests/clip_text_half_child.py; every figure is printed before it is asserted (profiles/clip_text_half_parity.txt holds one run's)."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

import difashion_amd as da
from difashion_amd import _lib
from tests import clip_text_half_child as measure
from tests.gpu_util import DEV, release_cached_gpu_memory
from tests.helpers_clip_text_half import FACTOR, HALF_CASES, YARDSTICKS, case_inputs, rel, yardstick

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _assert_parity(name, fmt, rec):
    assert all(rec["facts"].values()), (name, fmt, rec["facts"])
    for k, (e, r) in rec["dist"].items():                                       # every output, every tap, the cosine: none excused
        assert e <= FACTOR * r, (name, fmt, k, e, r)
    # which kernels ran: one launch of the causal kernel per block and one embed launch; none of dfh_attention's kernels, none of the
    # image tower's.  (The fp32 text tower's clip_attention_kernel has no counter; the taps being exact 16-bit upcasts and the new
    # counter reading L show the 16-bit walk ran.)
    c, L = rec["census"], rec["layers"]
    assert c["cliph_attention"] == L and c["cliph_embed"] == 1 and c["layernorm"] == 2 * L, c
    assert c["attention_16"] == 0 and c["attention_x32"] == 0 and c["clipv_attention"] == 0, c


def _assert_attention(T, fmt, rec):
    assert rec["finite"] and rec["bands_untouched"] and rec["rerun_identical"] and rec["one_launch"], (T, fmt, rec)
    assert rec["worst_ratio"] <= 1.0, (T, fmt, rec)


def _assert_causal(fmt, res, keys):
    assert sorted(res, key=int) == [str(k) for k in keys], (fmt, res)
    for k, rec in res.items():
        assert rec["prefix_identical"] and rec["suffix_moved"] and rec.get("finite", True), (fmt, k, rec)


@pytest.mark.parametrize("name", list(HALF_CASES))
def test_bf16_encoder_within_three_times_the_real_class(name):
    assert _lib.storage() == "bf16"
    _assert_parity(name, "bf16", measure.parity(name))


_OUTCOME = {}          # "fp16" -> ("ok", result) | ("died", text): the child is started ONCE, whatever became of it


def _fp16_child():
    if "fp16" in _OUTCOME:
        return _OUTCOME["fp16"]
    assert _lib.storage() == "bf16"
    release_cached_gpu_memory()
    env = dict(os.environ, DFH_STORAGE="fp16")
    env.pop("DFH_LIB", None)
    try:
        r = subprocess.run([sys.executable, "-m", "tests.clip_text_half_child"], capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    except subprocess.TimeoutExpired as err:
        _OUTCOME["fp16"] = ("died", f"the fp16 child did not finish in {err.timeout} s")
        return _OUTCOME["fp16"]
    print("\n".join(l for l in r.stdout.splitlines() if l.startswith("clipth ")))      # the child's figures, before anything is asserted
    lines = [l for l in r.stdout.splitlines() if l.startswith("CLIPTH_RESULT ")]
    if r.returncode != 0 or not lines:
        _OUTCOME["fp16"] = ("died", f"the fp16 child ended with status {r.returncode}:\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}")
    else:
        _OUTCOME["fp16"] = ("ok", json.loads(lines[-1][len("CLIPTH_RESULT "):]))
    return _OUTCOME["fp16"]


@pytest.mark.timeout(700)
def test_fp16_encoder_and_ops_in_a_child_process():
    kind, res = _fp16_child()
    assert kind == "ok", res
    assert res["storage"] == "fp16" and "storage=fp16" in res["build_info"], res["build_info"]
    assert sorted(res["parity"]) == sorted(HALF_CASES)
    for name, rec in res["parity"].items():
        _assert_parity(name, "fp16", rec)
    assert sorted(res["attention"], key=int) == [str(T) for T in measure.ATTENTION_T]
    for T, rec in res["attention"].items():
        _assert_attention(T, "fp16", rec)
    _assert_causal("fp16", res["causality"], measure.CAUSAL_T0)
    _assert_causal("fp16", res["model_causality"], (0, 15, 16, 40, 75))


@pytest.mark.parametrize("T", measure.ATTENTION_T)
def test_causal_attention_against_fp64_softmax(T):
    _assert_attention(T, "bf16", measure.attention_check(T))


def test_causality_is_bitwise_at_op_and_model_level():
    """The tolerance-free test of the mask and of the skipped key tiles."""
    _assert_causal("bf16", measure.causality_check(), measure.CAUSAL_T0)
    _assert_causal("bf16", measure.model_causality_check(), (0, 15, 16, 40, 75))


def test_op_level_refusals():
    x = torch.zeros(4 * 8, 3 * 64, dtype=_lib.storage_dtype(), device=DEV)
    o = torch.zeros(4 * 8, 64, dtype=_lib.storage_dtype(), device=DEV)
    call = lambda T, d: _lib.call("dfh_causal_attention", _lib.ptr(x), _lib.ptr(o), 1, T, 1, d, 0.125, _lib.stream_ptr())
    with pytest.raises(da.DfhError, match="head dim 64"):
        call(8, 32)
    with pytest.raises(da.DfhError, match=r"\[1, 128\]"):
        call(129, 64)
    with pytest.raises(da.DfhError, match=r"\[1, 128\]"):
        call(0, 64)


def _model(name, dtype=None, with_projection=True):
    cfg, params, proj, ids = case_inputs(name)
    return cfg, measure.hip_model(cfg, params, proj, dtype, with_projection), ids.to(DEV)


def _all(out):
    return out.to_tuple()[:2] + tuple(out.hidden_states) + (out.pooler_output,)


def test_reruns_round_trips_and_repacks():
    own = _lib.storage_dtype()
    cfg, m, ids = _model("thalf_tiny_20")
    _, untouched, _ = _model("thalf_tiny_20")
    want32 = _all(untouched(ids, output_hidden_states=True))
    half = _all(m.set_compute_dtype(own)(ids, output_hidden_states=True))
    assert all(torch.equal(a, b) for a, b in zip(half, _all(m(ids, output_hidden_states=True))))          # a rerun is bit-identical
    assert not torch.equal(half[0], want32[0])
    # .bfloat16() -> .float(): the fp32 tower's bits again, and the masters never moved
    packed = m._packed
    back = _all(m.float()(ids, output_hidden_states=True))
    assert all(torch.equal(a, b) for a, b in zip(back, want32))
    assert m._packed is packed and m._packed_sig is not None                     # the switch keeps the packed copy: nothing to remake on the way back
    assert all(p.dtype == torch.float32 for p in m.parameters()) and all(v.dtype == torch.float32 for v in m.state_dict().values())
    # a parameter update between two 16-bit calls is seen: the packed copy is remade
    m.set_compute_dtype(own)
    assert torch.equal(m(ids).text_embeds, half[0])
    layers = m.text_model.encoder.layers._modules                                # bare containers named "0", "1", ...
    saved = layers["1"].mlp.fc2.weight.detach().clone()
    with torch.no_grad():
        layers["1"].mlp.fc2.weight.mul_(1.5)
    moved = m(ids)
    assert not torch.equal(moved.text_embeds, half[0]) and not torch.equal(moved.last_hidden_state, half[1])
    with torch.no_grad():
        layers["1"].mlp.fc2.weight.copy_(saved)
    assert torch.equal(m(ids).text_embeds, half[0])                              # the old weights again: the old bits again
    with torch.no_grad():
        layers["0"].self_attn.q_proj.bias.add_(0.25)        # the stacked q | k | v bias is part of the copy
    assert not torch.equal(m(ids).text_embeds, half[0])


def test_checkpoint_round_trip_with_torch_dtype(tmp_path):
    own = _lib.storage_dtype()
    for with_projection, cls in ((False, da.CLIPTextModel), (True, da.CLIPTextModelWithProjection)):
        cfg, m, ids = _model("thalf_tiny_20", own, with_projection)
        d = str(tmp_path / cls.__name__)
        m.save_pretrained(d)
        from safetensors.torch import load_file
        assert all(v.dtype == torch.float32 for v in load_file(os.path.join(d, "model.safetensors")).values())
        assert "torch_dtype" not in json.load(open(os.path.join(d, "config.json")))
        m2 = cls.from_pretrained(d, torch_dtype=own).to(DEV)
        assert m2.compute_dtype == own and all(v.dtype == torch.float32 for v in m2.state_dict().values())
        assert torch.equal(m2(ids)[0], m(ids)[0]) and torch.equal(m2(ids).pooler_output, m(ids).pooler_output)
        m3 = cls.from_pretrained(d).to(DEV)                                       # the default stays the fp32 tower
        assert m3.compute_dtype == torch.float32 and not torch.equal(m3(ids)[0], m(ids)[0])
        assert torch.equal(m3(ids)[0], m.float()(ids)[0])


def test_batch_of_one_agrees_with_the_batch_within_the_rule():
    """Not bitwise: the GEMM plan (tile, K split) depends on M = batch x tokens, so the summation order may differ."""
    own, fmt = _lib.storage_dtype(), _lib.storage()
    ys = dict(np.load(YARDSTICKS))
    for name in ("thalf_tiny_77", "thalf_tiny_20"):
        cfg, m, ids = _model(name, own)
        full = m(ids, output_hidden_states=True)
        for b in range(ids.shape[0]):
            one = m(ids[b:b + 1], output_hidden_states=True)
            pairs = {"text_embeds": (one.text_embeds, full.text_embeds[b:b + 1]), "pooler_output": (one.pooler_output, full.pooler_output[b:b + 1]),
                     "last_hidden_state": (one.last_hidden_state, full.last_hidden_state[b:b + 1])}
            pairs.update({f"hidden_{t}": (one.hidden_states[t], full.hidden_states[t][b:b + 1]) for t in range(cfg.num_hidden_layers + 1)})
            for k, (a, f) in pairs.items():
                e, r = rel(a, f), yardstick(ys, name, fmt, k)
                assert e <= FACTOR * r, (name, b, k, e, r)


def test_prompt_table_and_clip_score_take_a_half_precision_tower():
    from difashion_amd.data import category_prompt
    from difashion_amd.prompts import PromptTable
    from tests.helpers_clip_text_half import config_kwargs
    from tests.helpers_data import StubTokenizer, synthetic_dataset
    from oracle import clip_ref
    import dataclasses
    own = _lib.storage_dtype()
    cfg = dataclasses.replace(HALF_CASES["thalf_tiny_20"][0], vocab_size=1001)            # StubTokenizer ids run to 1000
    m = da.CLIPTextModel(init_seed=None, torch_dtype=own, **config_kwargs(cfg))
    m.load_state_dict(clip_ref.init_params(cfg, 5))
    m = m.to(DEV).eval()
    _, id_cate, _, _ = synthetic_dataset()
    table = PromptTable.build(m, StubTokenizer(), id_cate, DEV, batch_size=len(id_cate) + 1)          # the whole closed set in one call
    assert table.table.dtype == torch.float32 and table.table.shape == (len(id_cate) + 1, 16, cfg.hidden_size)
    # the table is that tower's direct output, bitwise: the same rows in the same batch (the GEMM plan depends on the batch)
    prompts = [category_prompt(id_cate[c]) for c in sorted(id_cate)] + [""]
    ids = StubTokenizer()(prompts, max_length=16, padding="max_length", truncation=True, return_tensors="pt").input_ids
    direct = m(ids.to(DEV))[0]
    assert torch.equal(table.table, direct) and torch.equal(table.null_prompt, direct[-1:])
    assert torch.equal(table.lookup(torch.tensor([[1, 2], [5, 1]])), direct[[1, 2, 5, 1]])
    assert not torch.equal(direct, m.float()(ids.to(DEV))[0])                                # ... and not the fp32 tower's bits
    # CLIPScore over a 16-bit text tower (and the fp32 image tower): a text projection of the image tower's width
    from tests.helpers_clip_text_half import projection_weight
    from tests.helpers_clip_vision_half import case_inputs as vcase
    vcfg, vparams, px = vcase("half_tiny_short")
    image = da.CLIPVisionModelWithProjection(**vcfg.kwargs(), init_seed=None)
    image.load_state_dict(vparams)
    image = image.to(DEV).eval()
    tcfg, params, _, tids = case_inputs("thalf_tiny_20")
    text = measure.hip_model(tcfg, params, projection_weight(tcfg, 7, vcfg.projection_dim), own)
    n = min(px.shape[0], tids.shape[0])
    px, tids = px[:n].to(DEV), tids[:n].to(DEV)
    score = da.CLIPScore(image, text).calculate_clip_score(px, tids)
    assert score.dtype == torch.float32 and score.shape == (n,) and torch.isfinite(score).all()
    assert torch.equal(score, da.pair_cosine(image.encode_image(px), text.encode_text(tids), 100.0))
    assert not torch.equal(score, da.CLIPScore(image, text.float()).calculate_clip_score(px, tids))


def test_difashion_forward_with_a_half_precision_text_encoder():
    """``from_pretrained_pipeline(text_encoder_dtype=...)`` hands ``torch_dtype=`` to ``CLIPTextModel.from_pretrained``; no SD checkpoint
    travels with the tests, so the path is exercised by constructing ``DiFashion`` with such a tower: the reference's golden training
    batch, the same draws, once with the fp32 text tower and once with the 16-bit one.  The loss stays within the bf16 training
    tolerance the golden batch is held to (2e-2 relative, tests/test_gpu_train.py / test_gpu_difashion.py) and is not the same number."""
    from oracle import clip_ref
    from tests.helpers import GLUE_CFG, glue_unet_params, load
    from tests.helpers_clip_text_half import config_kwargs
    from tests.test_gpu_difashion import CATE_NUM, H, IdentityVAE, Replay, TensorKeyDict
    from tests.test_gpu_pipeline import encoder
    from tests.test_gpu_unet import hip_unet
    own = _lib.storage_dtype()
    rec = load("train_b2_mse.npz")
    bsz = 2
    g = torch.Generator().manual_seed(31 + bsz)
    img_dataset = torch.randn(40, 4, H, H, generator=g) * 0.6
    null_img = torch.randn(4, H, H, generator=g) * 0.3
    outfits = torch.randint(1, 40, (bsz, 4), generator=g)
    cats = torch.randint(1, CATE_NUM, (bsz, 4), generator=g)
    uids = torch.arange(bsz) + 100
    hist = {u: TensorKeyDict({c: torch.randn(4, H, H, generator=g) * 0.5 for c in range(1, CATE_NUM, 2)}) for u in uids.tolist()}
    cfg = clip_ref.CLIPTextConfig(vocab_size=64, hidden_size=GLUE_CFG.cross_attention_dim, intermediate_size=128, num_hidden_layers=2,
                                  num_attention_heads=1, bos_token_id=62, pad_token_id=63)                 # one head of dim 64
    params = clip_ref.init_params(cfg, 9)
    ids = torch.full((bsz, 4, 77), 63, dtype=torch.long)                          # [bos, category word, eos, pad ...]
    ids[:, :, 0], ids[:, :, 1], ids[:, :, 2] = 62, cats + 5, 63

    class Tok:
        model_max_length = 77

        def __call__(self, texts, padding=None, max_length=77, truncation=True, return_tensors="pt"):
            out = torch.full((len(texts), max_length), 63, dtype=torch.long)
            out[:, 0] = 62
            return types.SimpleNamespace(input_ids=out)

    unet = hip_unet(GLUE_CFG, glue_unet_params(), max_batch=32)
    args = types.SimpleNamespace(use_history=True, use_mutual_guidance=True, eta=0.1, snr_gamma=None, noise_offset=0)
    losses, states = {}, {}
    for mode in (torch.float32, own):
        text = da.CLIPTextModel(init_seed=None, torch_dtype=mode, **config_kwargs(cfg))
        text.load_state_dict(params)
        text = text.to(DEV).eval().requires_grad_(False)
        m = Replay(args, vae=IdentityVAE(), unet=unet, fashion_encoder=encoder(rec), noise_scheduler=da.DDIMScheduler(prediction_type=str(rec["pred_type"])),
                   text_encoder=text, tokenizer=Tok())
        taps = {}
        torch.manual_seed(1234 + bsz)
        _lib.census_reset()
        with torch.no_grad():
            loss = m(dict(uids=uids, outfits=outfits, category=cats, input_ids=ids), img_dataset, hist, null_img, 0.2, 0.3, 0.2, torch.float32,
                     torch.Generator().manual_seed(77), taps=taps)
        torch.cuda.synchronize()
        assert _lib.census()["cliph_attention"] == (0 if mode == torch.float32 else 2 * cfg.num_hidden_layers)      # prompts + the null prompt
        losses[mode], states[mode] = float(loss), taps["ehs"].clone()
    l32, l16 = losses[torch.float32], losses[own]
    print(f"clipth difashion forward: loss fp32 text tower {l32!r}, {own} text tower {l16!r}, rel {abs(l16 - l32) / abs(l32):.2e}")
    assert np.isfinite(l16) and abs(l16 - l32) <= 2e-2 * abs(l32)
    assert l16 != l32 and not torch.equal(states[own], states[torch.float32])


def test_error_behaviour():
    own, other = _lib.storage_dtype(), (torch.float16 if _lib.storage() == "bf16" else torch.bfloat16)
    cfg, m, ids = _model("thalf_tiny_20", own)
    with pytest.raises(da.DfhError, match="property of the process"):
        m.set_compute_dtype(other)
    with pytest.raises(da.DfhError, match="property of the process"):
        m.to(dtype=other)
    assert m.compute_dtype == own
    with pytest.raises(da.DfhError, match="no CPU fallback"):
        measure.hip_model(*case_inputs("thalf_tiny_20")[:3], own).cpu()(ids.cpu())              # the model on the wrong device
    assert torch.equal(m(ids.cpu())[0], m(ids)[0])                                # tokenizer output (CPU ids) is moved, as in fp32 mode
    with pytest.raises(ValueError, match="max_position_embeddings"):
        m(torch.zeros(1, cfg.max_position_embeddings + 1, dtype=torch.long, device=DEV))
    with pytest.raises(IndexError):
        m(torch.full((1, 5), cfg.vocab_size, dtype=torch.long, device=DEV))
    with pytest.raises(IndexError):
        m(torch.full((1, 5), -1, dtype=torch.long, device=DEV))
    assert torch.isfinite(m(ids[:, :1])[0]).all()                                 # T = 1
    # an unsupported head dim: the old tiny config (head dim 16) stays an fp32-only tower and still runs
    from tests.helpers_clip import case_inputs as fp32_case
    from tests.test_gpu_clip import hip_clip
    tcfg, tparams, tids = fp32_case("tiny_short_seq")
    t = hip_clip(tcfg, tparams)
    with pytest.raises(da.DfhError, match="head dim 16 is not built"):
        t.set_compute_dtype(own)
    assert t.compute_dtype == torch.float32 and torch.isfinite(t(tids.to(DEV))[0]).all()

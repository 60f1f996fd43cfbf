"""Row f6 without a GPU: the fixtures belong to the regenerated inputs, the new entry points are declared, built and bound,
the state-dict names are the real classes', and every refusal that needs no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import difashion_amd as da
from difashion_amd import _lib
from tests import helpers_eval_scores as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["dfh_clip_text_embeds", "dfh_embed_pair_cosine", "dfh_embed_candidates", "dfh_compat_workspace_bytes", "dfh_compat_score",
               "dfh_compat_pred_score"]


def tiny_text_model(name="tiny_short_seq"):
    cfg, pd, params, ids = H.text_case_inputs(name)
    m = da.CLIPTextModelWithProjection(**H.text_kwargs(cfg, pd), init_seed=None)
    m.load_state_dict(params)
    return m, params, ids


@pytest.mark.parametrize("name", H.TEXT_TINY)
def test_text_fixture_checksums(name):
    cfg, pd, params, ids = H.text_case_inputs(name)
    fx = H.load_fixture("cliptp_" + name)
    np.testing.assert_allclose(fx["checksum"], H.text_checksum(params, ids), rtol=1e-12)
    assert np.array_equal(fx["input_ids"], ids.numpy())
    pos = H.TEXT_CASES[name][4]
    assert list(fx["eos_positions"]) == list(pos) and len(set(pos)) == len(pos) and 0 in pos and ids.shape[1] - 1 in pos
    assert fx["text_embeds"].shape == (len(pos), pd) and float(fx["ref_text_embeds"]) > 0


@pytest.mark.parametrize("name", list(H.COMPAT_CASES))
def test_compat_fixture_checksums(name):
    params, real, gen, ol = H.compat_case_inputs(name)
    fx = H.load_fixture("compat_" + name)
    np.testing.assert_allclose(fx["checksum"], H.compat_checksum(params, real, gen, ol), rtol=1e-12)
    O, items, dim, _ = H.COMPAT_CASES[name]
    assert np.array_equal(fx["olists"], ol.numpy()) and fx["outfit_emb"].shape == (O, 256) and fx["logits"].shape == (O,)
    assert int(ol[0, 0]) == 0 and (ol > 0).any() and (ol < 0).any()
    assert fx["pair_order"].tolist() == H.pair_order(items)
    np.testing.assert_allclose(fx["scores"], 1.0 / (1.0 + np.exp(-fx["logits"].astype(np.float64))), rtol=2e-7)


def test_score_fixture_checksums():
    for name, (rows, dim, _) in H.PAIR_CASES.items():
        fx = H.load_fixture("evalscore_pair_" + name)
        a, b = H.pair_inputs(name)
        np.testing.assert_allclose(fx["checksum"], H.scores_checksum(a, b), rtol=1e-12)
        want = 100.0 * torch.nn.functional.cosine_similarity(a.double(), b.double())
        assert fx["scores"].shape == (rows,) and float((torch.from_numpy(fx["scores"]).double() - want).abs().max()) < 1e-5
    for name, (K, _) in H.RETRIEVAL_CASES.items():
        fx = H.load_fixture("evalscore_retrieval_" + name)
        gen, table, cand = H.retrieval_inputs(name)
        np.testing.assert_allclose(fx["checksum"], H.scores_checksum(gen, table, cand), rtol=1e-12)
        assert np.array_equal(fx["candidates"], cand.numpy()) and fx["sims"].shape == (H.RETRIEVAL_ROWS, K)
        if K > 1:
            r = int(fx["tie_row"])
            assert cand[r, 0] == cand[r, 1] and fx["sims"][r, 0] == fx["sims"][r, 1] and fx["pred"][r] == 0


def test_new_symbols_in_header_library_and_binding():
    src = open(os.path.join(ROOT, "include", "difashion_hip.h")).read()
    assert "#define DFH_ABI_VERSION 8" in src and "#define DFH_COMPAT_NUM_PARAMS 32" in src
    decl = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.raw()
    for n in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % n, decl), n
        assert hasattr(lib, n) and n in _lib.SIGNATURES, n
    assert lib.dfh_abi_version() == 8
    f16 = C.CDLL(os.path.join(_lib.CSRC, "libdifashion_hip_f16.so"))
    assert all(hasattr(f16, n) for n in NEW_SYMBOLS)
    # the size query is host-only work
    assert lib.dfh_compat_workspace_bytes(0, 4, 1024) == 0 and lib.dfh_compat_workspace_bytes(1, 9, 1024) == 0
    small, big = lib.dfh_compat_workspace_bytes(1, 4, 1024), lib.dfh_compat_workspace_bytes(65, 4, 1024)
    assert 0 < small < big and big >= 4 * (65 * 4 * 2048 + 65 * 6 * (2048 + 1024))


def test_entry_points_refuse_before_any_launch():
    null = C.c_void_p(0)
    with pytest.raises(da.DfhError, match="null argument"):
        _lib.call("dfh_embed_pair_cosine", null, null, null, 1, 4, 100.0, null)
    with pytest.raises(da.DfhError, match="null argument"):
        _lib.call("dfh_embed_candidates", null, null, null, null, null, 1, 1, 4, 1, null)
    arr = (C.c_void_p * 32)(*([16] * 32))
    with pytest.raises(da.DfhError, match="DFH_COMPAT_NUM_PARAMS"):
        _lib.call("dfh_compat_score", arr, 31, 1024, null, 1, null, 0, null, 1, 4, null, null, null, null, 0, null)
    with pytest.raises(da.DfhError, match="items must be in"):
        _lib.call("dfh_compat_score", arr, 32, 1024, C.c_void_p(256), 9, null, 0, null, 1, 9, null, null, null, C.c_void_p(256), 1 << 30, null)
    with pytest.raises(da.DfhError, match="multiple of 4"):
        _lib.call("dfh_compat_score", arr, 32, 1022, C.c_void_p(256), 4, null, 0, null, 1, 4, null, null, null, C.c_void_p(256), 1 << 30, null)
    with pytest.raises(da.DfhError, match="workspace smaller"):
        _lib.call("dfh_compat_score", arr, 32, 1024, C.c_void_p(256), 4, null, 0, null, 1, 4, null, null, null, C.c_void_p(256), 64, null)
    m, _, _ = tiny_text_model()
    ctx = m._make_ctx()
    try:
        n = m._entry("num_params")(ctx)
        ptrs = (C.c_void_p * n)(*([16] * n))
        with pytest.raises(da.DfhError, match="null argument"):
            _lib.call("dfh_clip_text_embeds", ctx, ptrs, n, null, 32, C.c_void_p(256), C.c_void_p(256), null, null, 2, null, C.c_void_p(256),
                      1 << 30, 1, 5, null)
        with pytest.raises(da.DfhError, match="sequence length"):
            _lib.call("dfh_clip_text_embeds", ctx, ptrs, n, C.c_void_p(256), 32, C.c_void_p(256), C.c_void_p(256), null, null, 2, null,
                      C.c_void_p(256), 1 << 30, 1, 78, null)
    finally:
        m._entry("destroy")(ctx)


def test_text_model_with_projection_keys_and_refusals(tmp_path):
    m, params, ids = tiny_text_model()
    fx = H.load_fixture("cliptp_tiny_short_seq")
    assert list(m.state_dict()) == list(fx["param_names"]) == list(params)
    assert all(torch.equal(m.state_dict()[k], v) for k, v in params.items())
    # the native table is CLIPTextModel's: the projection is not part of it
    assert [n for n, _ in m.param_table()] == [k for k in params if k != "text_projection.weight"]
    assert m.config.projection_dim == 32 and m.text_projection.weight.shape == (32, 64)
    with pytest.raises(NotImplementedError):
        m(ids, attention_mask=torch.ones_like(ids))
    with pytest.raises(NotImplementedError):
        m(ids, position_ids=torch.arange(5)[None])
    with pytest.raises(NotImplementedError):
        m(ids, output_attentions=True)
    with pytest.raises(ValueError, match="specify input_ids"):
        m()
    with pytest.raises(da.DfhError, match="no CPU fallback"):
        m(ids)
    with pytest.raises(da.DfhError, match="no CPU fallback"):
        m.encode_text(ids)
    # the flattened key layout of newer transformers releases, and the position_ids buffer of old checkpoints
    flat = {(k[len("text_model."):] if k.startswith("text_model.") else k): v for k, v in params.items()}
    flat["embeddings.position_ids"] = torch.arange(77)[None]
    m2 = da.CLIPTextModelWithProjection(**m.config, init_seed=None)
    m2.load_state_dict(flat)
    assert all(torch.equal(m2.state_dict()[k], v) for k, v in params.items())
    m.save_pretrained(str(tmp_path / "text"))
    import json
    cfg = json.load(open(tmp_path / "text" / "config.json"))
    assert cfg["architectures"] == ["CLIPTextModelWithProjection"] and cfg["projection_dim"] == 32
    m3 = da.CLIPTextModelWithProjection.from_pretrained(str(tmp_path), subfolder="text")
    assert all(torch.equal(m3.state_dict()[k], v) for k, v in params.items())
    # CLIPTextModel is what it was: no projection key, same table
    assert "text_projection.weight" not in da.CLIPTextModel(**{k: v for k, v in m.config.items() if k != "projection_dim"}).state_dict()


def test_fashion_evaluator_keys_and_refusals():
    fx = H.load_fixture("compat_one_outfit")
    ev = da.FashionEvaluator(1024)
    assert list(ev.state_dict()) == list(fx["param_names"]) == [n for n, _ in H.compat_param_shapes(1024)]
    assert [tuple(v.shape) for v in ev.state_dict().values()] == [s for _, s in H.compat_param_shapes(1024)]
    assert sum(p.numel() for p in ev.parameters()) == 2615681 and len(list(ev.parameters())) == _lib_num_params()
    params, real, gen, ol = H.compat_case_inputs("one_outfit")
    ev.load_state_dict(params)
    assert not ev.training and not any(p.requires_grad for p in ev.parameters())
    with pytest.raises(NotImplementedError, match="inference only"):
        ev.train()
    assert ev.eval() is ev
    feats = H.compat_gather(real, gen, ol)
    for call in (ev, ev.outfit_emb):
        with pytest.raises(da.DfhError, match="no CPU fallback"):
            call(feats)
    with pytest.raises(da.DfhError, match="no CPU fallback"):
        ev.pred_score(torch.zeros(1, 256))
    with pytest.raises(ValueError, match="cnn_feats must be"):
        ev(torch.zeros(1, 4, 512))
    with pytest.raises(ValueError, match="multiple of 4"):
        da.FashionEvaluator(1022)
    ce = da.CompatibilityEvaluator(ev, "cpu")
    with pytest.raises(da.DfhError, match="no CPU fallback"):
        ce.evaluate_compatibility(ol, real, gen)
    with pytest.raises(IndexError):
        ce.evaluate_compatibility(torch.tensor([[1, 2, 300, 4]]), real, gen)
    with pytest.raises(IndexError):
        ce.evaluate_compatibility(torch.tensor([[1, 2, -40, 4]]), real, gen)
    with pytest.raises(TypeError, match="cnn_feats_gen is None"):
        ce.evaluate_compatibility(torch.tensor([[1, 2, 0, 4]]), real, None)


def _lib_num_params():
    src = open(os.path.join(ROOT, "include", "difashion_hip.h")).read()
    return int(re.search(r"#define DFH_COMPAT_NUM_PARAMS (\d+)", src).group(1))


def test_score_refusals():
    a = torch.zeros(3, 8)
    with pytest.raises(da.DfhError, match="no CPU fallback"):
        da.pair_cosine(a, a)
    with pytest.raises(da.DfhError, match="no CPU fallback"):
        da.candidate_cosine(a, a, torch.zeros(3, 2, dtype=torch.long))
    cs = da.CLIPScore(image_model=None, text_model=None)
    for bad in ("euclidean", "eiclidean"):
        with pytest.raises(ValueError, match=f"Unrecognized similarity function {bad}."):
            cs.calculate_clip_img_score(a, a, similarity_func=bad)
        with pytest.raises(ValueError, match=f"Unrecognized similarity function {bad}."):
            cs.personalization_sim(a, a, similarity_func=bad)
        with pytest.raises(ValueError, match=f"Unrecognized similarity function {bad}."):
            cs.retrieval(a, a, torch.zeros(3, 2, dtype=torch.long), similarity_func=bad)


class _Fake(torch.Tensor):
    """A tensor that says it lives on the GPU: the id checks run before anything touches the device."""
    @property
    def device(self):
        return torch.device("cuda", 0)


def test_candidate_ids_out_of_range_are_refused():
    gen, table = torch.zeros(3, 8).as_subclass(_Fake), torch.zeros(10, 8).as_subclass(_Fake)
    for bad in ([[0, 10]] * 3, [[-1, 2]] * 3):
        with pytest.raises(IndexError, match="out of range"):
            da.candidate_cosine(gen, table, torch.tensor(bad))
    with pytest.raises(ValueError, match="candidates must be"):
        da.candidate_cosine(gen, table, torch.zeros(2, 2, dtype=torch.long))
    with pytest.raises(TypeError, match="integer ids"):
        da.candidate_cosine(gen, table, torch.zeros(3, 2))

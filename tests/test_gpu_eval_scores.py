"""-m gpu: row f6 -- the text tower with projection, the embedding score kernels and the compatibility scorer against
fixtures that the REAL classes produced in fp64 (tests/golden/make_golden_clip_text_proj.py, make_golden_compat.py,
make_golden_eval_scores.py).  Weights and inputs are regenerated from the case's seed; the fixture's checksum proves they are the same
tensors.

Stated tolerances:
  * text tower and compatibility scorer: the fixture records, per output, how far the real class run in fp32 sits from its own fp64 run
    (``ref_*``, relative L2).  The HIP path, fp32 end to end, must sit within 3 x that distance of the same fp64 values -- the rule and
    the factor of tests/test_gpu_clip_vision.py for the same GEMM and LayerNorm kernels (another summation order, another erf / exp).
    The single-outfit case is held on outfit_emb and on |logit - fixture| <= 3 x the real class's own absolute fp32 distance.
  * pair scores: absolute error <= 100 (dim / 64 + 16) 2^-24 on the 0..100 scale (helpers_eval_scores.pair_bound: derived from the
    kernel's reduction shape, 1.9e-4 at dim 1024); retrieval sims the same without the factor 100; predictions exact.
Every measured distance is printed before it is asserted (profiles/eval_scores_parity.txt holds one run's "evalscore" lines)."""
import ctypes as C

import numpy as np
import pytest
import torch

import difashion_amd as da
from difashion_amd import _lib
from tests import helpers_eval_scores as H
from tests.gpu_util import DEV

pytestmark = pytest.mark.gpu
FACTOR = 3.0
NAN = float("nan")


def held(tag, dist):
    """dist: {output: (measured, yardstick)}; prints every pair, then asserts measured <= FACTOR x yardstick."""
    print(f"evalscore parity {tag}", " ".join(f"{k}: hip {e:.2e} ref_fp32 {r:.2e} ratio {e / r if r else float('inf'):.2f};" for k, (e, r) in dist.items()))
    for k, (e, r) in dist.items():
        assert e <= FACTOR * r, (tag, k, e, r)


# ------------------------------------------------------------------ text tower with projection
def hip_text(cfg, pd, params):
    m = da.CLIPTextModelWithProjection(**H.text_kwargs(cfg, pd), init_seed=None)
    m.load_state_dict(params)
    return m.to(DEV).eval().requires_grad_(False)


@pytest.mark.parametrize("name", list(H.TEXT_CASES))
def test_text_embeds_match_the_real_transformers_class(name):
    cfg, pd, params, ids = H.text_case_inputs(name)
    fx = H.load_fixture("cliptp_" + name)
    np.testing.assert_allclose(fx["checksum"], H.text_checksum(params, ids), rtol=1e-12)
    m = hip_text(cfg, pd, params)
    out = m(ids.to(DEV), output_hidden_states=True)
    B, T, D = ids.shape[0], ids.shape[1], cfg.hidden_size
    assert out.text_embeds.shape == (B, pd) and out.pooler_output.shape == (B, D) and out.last_hidden_state.shape == (B, T, D)
    assert len(out.hidden_states) == cfg.num_hidden_layers + 1 and len(out) == 3 and out[0] is out.text_embeds and out[1] is out.last_hidden_state
    got = {"text_embeds": out.text_embeds.cpu(), "pooler_output": out.pooler_output.cpu(),
           "last_hidden_state": H.text_rows_of(fx, out.last_hidden_state.cpu())}
    for t in fx["taps"]:
        got[f"hidden_{int(t)}"] = H.text_rows_of(fx, out.hidden_states[int(t)].cpu())
    dist = {k: (H.rel(v, torch.from_numpy(fx[k])), float(fx["ref_" + k])) for k, v in got.items()}
    # hidden_0 (token + position embedding, one fp32 add) has yardstick 0: the real class's fp32 run IS the rounded fp64 run there
    held(f"text {name}", dist)
    # the call forms: encode_text (no last_hidden_state formed), tuples, reruns bit-identical
    assert torch.equal(m.encode_text(ids.to(DEV)), out.text_embeds) and torch.equal(m.encode_text(ids), out.text_embeds)
    again = m(ids.to(DEV))
    assert again.hidden_states is None and len(again) == 2 and torch.equal(again[0], out.text_embeds) and torch.equal(again[1], out.last_hidden_state)
    assert torch.equal(m(ids.to(DEV), return_dict=False)[0], out.text_embeds)
    # CLIPTextModel on the same text_model.* weights: gather-then-normalise == normalise-then-gather, bit for bit
    base = da.CLIPTextModel(**{k: v for k, v in H.text_kwargs(cfg, pd).items() if k != "projection_dim"}, init_seed=None)
    base.load_state_dict({k: v for k, v in params.items() if k.startswith("text_model.")})
    ref = base.to(DEV)(ids.to(DEV), output_hidden_states=True)
    assert torch.equal(ref.pooler_output, out.pooler_output) and torch.equal(ref.last_hidden_state, out.last_hidden_state)
    assert all(torch.equal(a, b) for a, b in zip(ref.hidden_states, out.hidden_states))
    pos = torch.tensor(H.TEXT_CASES[name][4], device=DEV)
    assert torch.equal(out.pooler_output, out.last_hidden_state[torch.arange(B, device=DEV), pos])


def test_text_embeds_batch_independence_guard_rows_and_checkpoint(tmp_path):
    cfg, pd, params, ids = H.text_case_inputs("tiny_gelu_eos")
    m = hip_text(cfg, pd, params)
    dev_ids = ids.to(DEV)
    full = m(dev_ids)
    for b in range(ids.shape[0]):
        one = m(dev_ids[b:b + 1])
        assert torch.equal(one.text_embeds, full.text_embeds[b:b + 1]) and torch.equal(one.pooler_output, full.pooler_output[b:b + 1])
    # one NaN guard row behind every output of the entry point
    B, T, D = ids.shape[0], ids.shape[1], cfg.hidden_size
    arr, count = m._prepare(torch.device(DEV, torch.cuda.current_device()), B, T)
    embeds, pooled = torch.full((B + 1, pd), NAN, device=DEV), torch.full((B + 1, D), NAN, device=DEV)
    last = torch.full((B * T + 1, D), NAN, device=DEV)
    L = cfg.num_hidden_layers
    taps = torch.full(((L + 1) * B * T + 1, D), NAN, device=DEV)
    _lib.call("dfh_clip_text_embeds", m._ctx, arr, count, _lib.ptr(m.text_projection.weight), pd, _lib.ptr(dev_ids), _lib.ptr(embeds),
              _lib.ptr(pooled), _lib.ptr(last), int(cfg.eos_token_id), _lib.ptr(taps), _lib.ptr(m._ws), m._ws.numel(), B, T, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert torch.isnan(embeds[-1]).all() and torch.isnan(pooled[-1]).all() and torch.isnan(last[-1]).all() and torch.isnan(taps[-1]).all()
    with_taps = m(dev_ids, output_hidden_states=True)
    assert torch.equal(taps[:-1].view(L + 1, B, T, D), torch.stack(with_taps.hidden_states))
    assert torch.equal(embeds[:-1], full.text_embeds) and torch.equal(pooled[:-1], full.pooler_output)
    assert torch.equal(last[:-1].view(B, T, D), full.last_hidden_state)
    m.save_pretrained(str(tmp_path / "text_encoder"))
    m2 = da.CLIPTextModelWithProjection.from_pretrained(str(tmp_path), subfolder="text_encoder").to(DEV)
    assert m2.config.projection_dim == pd and torch.equal(m2(dev_ids).text_embeds, full.text_embeds)
    with pytest.raises(NotImplementedError):
        m(dev_ids, attention_mask=torch.ones_like(dev_ids))
    with pytest.raises(IndexError):
        m(torch.full((1, 5), cfg.vocab_size))


# ------------------------------------------------------------------ compatibility scorer
def hip_compat(params, dim):
    ev = da.FashionEvaluator(dim)
    ev.load_state_dict(params)
    return da.CompatibilityEvaluator(ev, DEV)


@pytest.mark.parametrize("name", list(H.COMPAT_CASES))
def test_compatibility_matches_the_real_fashion_evaluator(name):
    params, real, gen, ol = H.compat_case_inputs(name)
    O, items, dim, _ = H.COMPAT_CASES[name]
    fx = H.load_fixture("compat_" + name)
    np.testing.assert_allclose(fx["checksum"], H.compat_checksum(params, real, gen, ol), rtol=1e-12)
    ce = hip_compat(params, dim)
    real_d, gen_d = real.to(DEV), gen.to(DEV)
    emb, logits, scores = ce.evaluate_compatibility(ol, real_d, gen_d, return_all=True)
    assert emb.shape == (O, 256) and logits.shape == (O,) and scores.shape == (O,)
    want = {k: torch.from_numpy(fx[k]) for k in ("outfit_emb", "logits", "scores")}
    if O == 1:
        d_abs, ref_abs = float((logits.cpu().double() - want["logits"].double()).abs().max()), float(fx["ref_abs_logits"])
        print(f"evalscore parity compat {name} |logit - fixture|: hip {d_abs:.2e} ref_fp32 {ref_abs:.2e} ratio {d_abs / ref_abs if ref_abs else float('inf'):.2f}")
        held(f"compat {name}", {"outfit_emb": (H.rel(emb.cpu(), want["outfit_emb"]), float(fx["ref_outfit_emb"]))})
        assert d_abs <= FACTOR * ref_abs, (name, d_abs, ref_abs)
    else:
        held(f"compat {name}", {k: (H.rel(v.cpu(), want[k]), float(fx["ref_" + k])) for k, v in (("outfit_emb", emb), ("logits", logits), ("scores", scores))})
    # the call forms agree bit for bit: the scores alone, the list-of-lists olists of the reference's DataLoader, a rerun
    assert torch.equal(ce.evaluate_compatibility(ol, real_d, gen_d), scores)
    assert torch.equal(ce.evaluate_compatibility([list(map(int, r)) for r in ol], real_d, gen_d), scores)
    # through the gather == FashionEvaluator on the pre-gathered tensor
    feats = H.compat_gather(real, gen, ol).to(DEV)
    ev = ce.evaluator
    assert torch.equal(ev(feats), logits) and torch.equal(ev.outfit_emb(feats), emb) and torch.equal(ev.pred_score(emb), logits)
    assert torch.equal(scores, torch.sigmoid(logits)) or float((scores - torch.sigmoid(logits)).abs().max()) <= 2 ** -23


def test_compatibility_batch_independence_and_guard_rows():
    name = "tile_edge"
    params, real, gen, ol = H.compat_case_inputs(name)
    O, items, dim, _ = H.COMPAT_CASES[name]
    ce = hip_compat(params, dim)
    ev = ce.evaluator
    real_d, gen_d, ol_d = real.to(DEV), gen.to(DEV), ol.to(DEV)
    emb, logits, scores = ce.evaluate_compatibility(ol, real_d, gen_d, return_all=True)
    ones = [ce.evaluate_compatibility(ol[o:o + 1], real_d, gen_d, return_all=True) for o in range(O)]
    for i, k in enumerate(("outfit_emb", "logits", "scores")):
        assert torch.equal(torch.cat([t[i] for t in ones]), (emb, logits, scores)[i]), k
    # NaN guard rows behind the three outputs, straight through the C entry point
    g_emb, g_log, g_sc = torch.full((O + 1, 256), NAN, device=DEV), torch.full((O + 1,), NAN, device=DEV), torch.full((O + 1,), NAN, device=DEV)
    arr, keep = ev._pointers()
    ws = ev._workspace(real_d.device, O, items, dim)
    _lib.call("dfh_compat_score", arr, 32, dim, _lib.ptr(real_d), real.shape[0], _lib.ptr(gen_d), gen.shape[0], _lib.ptr(ol_d), O, items,
              _lib.ptr(g_emb), _lib.ptr(g_log), _lib.ptr(g_sc), _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
    torch.cuda.synchronize()
    assert torch.isnan(g_emb[-1]).all() and torch.isnan(g_log[-1]) and torch.isnan(g_sc[-1])
    assert torch.equal(g_emb[:-1], emb) and torch.equal(g_log[:-1], logits) and torch.equal(g_sc[:-1], scores)
    with pytest.raises(da.DfhError, match="no CPU fallback"):
        ce.evaluate_compatibility(ol, real, gen_d)
    with pytest.raises(ValueError, match="2 to 8 items"):
        ev(torch.zeros(2, 9, dim, device=DEV))


# ------------------------------------------------------------------ pair scores and retrieval
class Recorded:
    """Stands where a tower stands: hands back the recorded embeddings."""

    def encode_image(self, x):
        return x

    encode_text = encode_image


@pytest.mark.parametrize("name", list(H.PAIR_CASES))
def test_pair_scores(name):
    rows, dim, _ = H.PAIR_CASES[name]
    a, b = H.pair_inputs(name)
    fx = H.load_fixture("evalscore_pair_" + name)
    np.testing.assert_allclose(fx["checksum"], H.scores_checksum(a, b), rtol=1e-12)
    a_d, b_d = a.to(DEV), b.to(DEV)
    out = torch.full((rows + 1,), NAN, device=DEV)
    _lib.call("dfh_embed_pair_cosine", _lib.ptr(a_d), _lib.ptr(b_d), _lib.ptr(out), rows, dim, 100.0, _lib.stream_ptr())
    torch.cuda.synchronize()
    assert torch.isnan(out[-1])
    err, bound = float((out[:-1].cpu().double() - torch.from_numpy(fx["scores"]).double()).abs().max()), H.pair_bound(dim, 100.0)
    print(f"evalscore parity pair {name} rows={rows} dim={dim}: max |hip - fp64| {err:.2e} bound {bound:.2e} ratio {err / bound:.2f} "
          f"(torch fp32: {float(fx['ref_scores']):.2e})")
    assert err <= bound, (name, err, bound)
    cs = da.CLIPScore(Recorded(), Recorded())
    for got in (cs.calculate_clip_score(a_d, b_d), cs.calculate_clip_img_score(a_d, b_d), cs.personalization_sim(a_d, b_d), da.pair_cosine(a_d, b_d)):
        assert torch.equal(got, out[:-1])
    # a batch equals its rows run one at a time; a misaligned view takes the scalar path and stays inside the bound
    assert torch.equal(torch.cat([da.pair_cosine(a_d[r:r + 1], b_d[r:r + 1]) for r in range(min(rows, 65))]), out[:min(rows, 65)])
    pad = torch.zeros(rows * dim + 1, device=DEV)
    pad[1:] = a_d.flatten()
    odd = da.pair_cosine(pad[1:].view(rows, dim), b_d)
    assert float((odd.cpu().double() - torch.from_numpy(fx["scores"]).double()).abs().max()) <= bound


def test_pair_zero_row_gives_nan_in_its_own_score_only():
    a, b = H.pair_inputs("tile_edge")
    a_d, b_d = a.to(DEV), b.to(DEV)
    want = da.pair_cosine(a_d, b_d)
    a_d[7] = 0.0
    got = da.pair_cosine(a_d, b_d)
    keep = torch.arange(a.shape[0], device=DEV) != 7
    assert torch.isnan(got[7]) and torch.equal(got[keep], want[keep])
    gen, table, cand = H.retrieval_inputs("k5")
    gen_d, table_d = gen.to(DEV), table.to(DEV)
    sims0, pred0 = da.candidate_cosine(gen_d, table_d, cand)
    table_d[int(cand[1, 4])] = 0.0
    sims, pred = da.candidate_cosine(gen_d, table_d, cand)
    nan = torch.isnan(sims)
    assert nan[1, 4] and int(nan.sum()) == int((cand == cand[1, 4]).sum()) and torch.equal(sims[~nan], sims0[~nan])
    assert int(pred[1]) == 4                      # torch.argmax takes a NaN for the maximum


@pytest.mark.parametrize("name", list(H.RETRIEVAL_CASES))
def test_retrieval(name):
    K, _ = H.RETRIEVAL_CASES[name]
    gen, table, cand = H.retrieval_inputs(name)
    fx = H.load_fixture("evalscore_retrieval_" + name)
    np.testing.assert_allclose(fx["checksum"], H.scores_checksum(gen, table, cand), rtol=1e-12)
    rows, dim = gen.shape
    gen_d, table_d, cand_d = gen.to(DEV), table.to(DEV), cand.to(DEV)
    sims = torch.full((rows + 1, K), NAN, device=DEV)
    pred = torch.full((rows + 1,), -7, dtype=torch.int64, device=DEV)
    _lib.call("dfh_embed_candidates", _lib.ptr(gen_d), _lib.ptr(table_d), _lib.ptr(cand_d), _lib.ptr(sims), _lib.ptr(pred), rows, K, dim,
              table.shape[0], _lib.stream_ptr())
    torch.cuda.synchronize()
    assert torch.isnan(sims[-1]).all() and int(pred[-1]) == -7
    err, bound = float((sims[:-1].cpu().double() - torch.from_numpy(fx["sims"]).double()).abs().max()), H.pair_bound(dim, 1.0)
    print(f"evalscore parity retrieval {name} K={K}: max |hip - fp64| {err:.2e} bound {bound:.2e} ratio {err / bound:.2f} "
          f"(torch fp32: {float(fx['ref_sims']):.2e}); pred {pred[:-1].tolist()}")
    assert err <= bound, (name, err, bound)
    assert pred[:-1].cpu().tolist() == fx["pred"].tolist()
    if K > 1:
        r = int(fx["tie_row"])
        assert sims[r, 0] == sims[r, 1] and int(pred[r]) == 0           # the planted tie resolves to the lower index
    s2, p2 = da.CLIPScore(Recorded()).retrieval(gen_d, table_d, cand)   # CPU ids, as a DataLoader hands them over
    assert torch.equal(s2, sims[:-1]) and torch.equal(p2, pred[:-1])
    for r in range(rows):                                               # every row alone equals its row of the batch
        s1, p1 = da.candidate_cosine(gen_d[r:r + 1], table_d, cand[r:r + 1])
        assert torch.equal(s1, sims[r:r + 1]) and torch.equal(p1, pred[r:r + 1])
    with pytest.raises(IndexError):
        da.candidate_cosine(gen_d, table_d[:100], cand + 100)

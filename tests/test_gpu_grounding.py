"""-m gpu: the grounding retrieval (csrc/eval_rank.hip) against what the REFERENCE's ``clip_og_retrieval_given_data`` made of
the same seeded inputs in fp64 (tests/golden/make_golden_grounding.py).  Inputs are regenerated from the case's seed; the fixture's
checksum proves they are the same tensors.

Stated tolerances:
  * ranked ids, positions, counts, ``preds`` and the four recalls: EQUAL to the fixture.  Consecutive similarities through rank 101
    stand at least 2.3e-3 apart in every row (5e-3 in the rows of the nine single lengths; tests/test_grounding_cpu.py recomputes it),
    three orders above the bound below, so any correct fp32 arithmetic ranks as fp64 does;
  * returned similarities: |hip - fp64| <= helpers_grounding.rank_bound(dim) = (dim / 64 + 30) 2^-24, derived there from the kernels'
    summation shape (2.7e-6 at dim 1024);
  * the rows whose order the reference leaves open (a repeated id, two bit-equal table rows, NaN, signed zeros) follow the row's rule
    -- among equals the lower position first -- as helpers_grounding.expected_ranking's fp64 stable sort states it;
  * every batch-invariance, rerun and storage-build comparison is bit for bit.
Every measured distance is printed before it is asserted (profiles/grounding_parity.txt holds one run's "grounding parity" lines)."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import difashion_amd as da
from difashion_amd import _lib
from tests import helpers_eval_scores as HE
from tests import helpers_grounding as H
from tests.gpu_util import DEV, release_cached_gpu_memory

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = H.TOPN[-1]


class Recorded:
    """Stands where the image tower stands: hands back the recorded embeddings."""

    def encode_image(self, x):
        return x


def same_bits(a: da.RankResult, b: da.RankResult) -> bool:
    return (torch.equal(a.ids, b.ids) and torch.equal(a.positions, b.positions) and torch.equal(a.counts, b.counts)
            and torch.equal(a.sims.view(torch.int32), b.sims.view(torch.int32)))


def rows_of(r: da.RankResult, idx) -> da.RankResult:
    return da.RankResult(r.ids[idx], r.positions[idx], r.sims[idx], r.counts[idx])


@functools.lru_cache(maxsize=None)
def case_run(name):
    """One ranking of the case, shared by the tests below and left unchanged."""
    inp, fx = H.case_inputs(name), H.load_fixture(name)
    np.testing.assert_allclose(fx["checksum"], H.checksum(inp), rtol=1e-12)
    gen_d, table_d = inp["gen"].to(DEV), inp["table"].to(DEV)
    return inp, fx, gen_d, table_d, da.rank_candidates(gen_d, table_d, inp["candidates"], N)


@pytest.mark.parametrize("name", list(H.CASES))
def test_ranking_equals_the_reference(name):
    inp, fx, gen_d, table_d, ranked = case_run(name)
    rows, dim = inp["gen"].shape
    assert ranked.ids.shape == (rows, N) and ranked.ids.dtype == torch.int64 and ranked.counts.dtype == torch.int32
    live = np.isfinite(fx["sims"])
    got = ranked.sims.cpu().numpy()
    err, bound = float(np.abs(got.astype(np.float64)[live] - fx["sims"].astype(np.float64)[live]).max()), H.rank_bound(dim)
    print(f"grounding parity {name} rows={rows} dim={dim} sets {sorted(set(inp['set_len']))}: max |hip - fp64| {err:.2e} bound {bound:.2e} "
          f"ratio {err / bound:.2f} (torch fp32: {float(fx['ref_sims']):.2e}; smallest gap {float(fx['min_gap']):.2e})")
    assert np.array_equal(ranked.ids.cpu().numpy(), fx["ids"]) and np.array_equal(ranked.positions.cpu().numpy(), fx["positions"])
    assert np.array_equal(ranked.counts.cpu().numpy(), fx["counts"]) and np.array_equal(ranked.preds.cpu().numpy(), fx["preds"])
    assert err <= bound, (name, err, bound)
    assert np.array_equal(got[~live], fx["sims"][~live])                  # the -inf padding
    # recall: the four cutoffs equal the reference's floats; the hit positions are the first rank of the ground truth
    hit_pos, hits = da.recall_at(ranked, inp["grds"], H.TOPN)
    assert [h / rows for h in hits] == fx["recall"].tolist()
    where = [np.nonzero(fx["ids"][r] == int(inp["grds"][r]))[0] for r in range(rows)]
    assert hit_pos.tolist() == [int(w[0]) if len(w) else -1 for w in where]
    assert da.recall_at(ranked, inp["grds"].tolist(), ())[1] == []


def test_counts_and_padding_of_short_sets():
    inp, fx, _, _, ranked = case_run("main")
    for n in (1, 7, 64):
        r = inp["set_len"].index(n)
        assert int(ranked.counts[r]) == n
        assert (ranked.ids[r, n:] == -1).all() and (ranked.positions[r, n:] == -1).all() and torch.isneginf(ranked.sims[r, n:]).all()
        assert sorted(ranked.positions[r, :n].tolist()) == list(range(n)) and (ranked.ids[r, :n] >= 0).all()
    for n in (100, 101, 2500):
        r = inp["set_len"].index(n)
        assert int(ranked.counts[r]) == N and (ranked.ids[r] >= 0).all() and torch.isfinite(ranked.sims[r]).all()


def test_tie_duplicate_nan_and_signed_zero_rows_follow_the_stated_order():
    inp = H.special_inputs()
    gen_d, table_d = inp["gen"].to(DEV), inp["table"].to(DEV)
    ranked = da.rank_candidates(gen_d, table_d, inp["candidates"], N)
    for r, name in enumerate(H.SPECIAL_ROWS):
        cand = inp["candidates"][r]
        sims = H.cosine64(inp["gen"][r], inp["table"], cand)
        pos = H.expected_ranking(sims, N)
        k = len(cand)
        got = ranked.sims[r, :k].cpu().numpy().astype(np.float64)
        print(f"grounding parity special {name}: positions {ranked.positions[r, :k].tolist()}")
        assert int(ranked.counts[r]) == k and ranked.positions[r, :k].tolist() == pos and ranked.ids[r, :k].tolist() == cand[pos].tolist()
        assert (ranked.ids[r, k:] == -1).all() and torch.isneginf(ranked.sims[r, k:]).all()
        want = sims[pos]
        assert np.array_equal(np.isnan(got), np.isnan(want)) and np.nanmax(np.abs(got - want)) <= H.rank_bound(H.SPECIAL_DIM)
    s = {name: ranked.sims[r] for r, name in enumerate(H.SPECIAL_ROWS)}
    p = {name: ranked.positions[r] for r, name in enumerate(H.SPECIAL_ROWS)}
    assert s["dup"][3] == s["dup"][4] and p["dup"][3] < p["dup"][4]                      # one id twice: equal bits, lower position first
    assert s["twins"][3] == s["twins"][4] and p["twins"][3] < p["twins"][4]              # bit-equal rows under two ids
    assert torch.isnan(s["nan"][:2]).all() and p["nan"][0] < p["nan"][1] and not torch.isnan(s["nan"][2:22]).any()
    assert (s["zero"][10:12] == 0).all() and p["zero"][10:12].tolist() == [2, 9] and (s["zero"][:10] > 0).all() and (s["zero"][12:17] < 0).all()
    # a zero GENERATED row: NaN in its own similarities only, which then rank by position; the other rows keep their bits
    gen_z = gen_d.clone()
    gen_z[1] = 0.0
    rz = da.rank_candidates(gen_z, table_d, inp["candidates"], N)
    k = len(inp["candidates"][1])
    assert torch.isnan(rz.sims[1, :k]).all() and rz.positions[1, :k].tolist() == list(range(k))
    keep = [0, 2, 3]
    assert same_bits(rows_of(rz, keep), rows_of(ranked, keep))
    # a row with NO candidate: count 0, the whole list is padding, its neighbour keeps its bits
    re = da.rank_candidates(gen_d[:2], table_d, [[], inp["candidates"][1]], N)
    assert int(re.counts[0]) == 0 and (re.ids[0] == -1).all() and (re.positions[0] == -1).all() and torch.isneginf(re.sims[0]).all()
    assert int(re.preds[0]) == -1 and same_bits(rows_of(re, [1]), rows_of(ranked, [1]))


def test_batch_invariance_reruns_and_bands_give_the_same_bits():
    inp, fx, gen_d, table_d, ranked = case_run("main")
    norms = da.embed_row_norms(table_d)
    assert same_bits(da.rank_candidates(gen_d, table_d, inp["candidates"], N, table_norms=norms), ranked)          # a rerun
    shared = inp["shared_rows"]
    cand = inp["candidates"][shared[0]]
    together = da.rank_candidates(gen_d[shared], table_d, [cand] * len(shared), N, table_norms=norms)
    assert same_bits(together, rows_of(ranked, shared))                                       # ranked with other sets' rows or alone with its set
    ones = [da.rank_candidates(gen_d[r:r + 1], table_d, [cand], N, table_norms=norms) for r in shared]
    assert same_bits(da.RankResult(*(torch.cat([getattr(o, f) for o in ones]) for f in ("ids", "positions", "sims", "counts"))), together)
    # two bands forced by a workspace cap of 40 rows of the set (320 floats a row), and the whole case one row a band
    assert same_bits(da.rank_candidates(gen_d[shared], table_d, [cand] * len(shared), N, table_norms=norms, workspace_cap=40 * 320 * 4), together)
    assert same_bits(da.rank_candidates(gen_d, table_d, inp["candidates"], N, table_norms=norms, workspace_cap=1), ranked)
    # device-resident candidate lists and the (set ids, sets) form
    dev_c = {id(c): c.to(DEV) for c in inp["candidates"]}
    assert same_bits(da.rank_candidates(gen_d, table_d, [dev_c[id(c)] for c in inp["candidates"]], N), ranked)
    uniq = list({id(c): c for c in inp["candidates"]}.values())
    key_of = {id(c): i for i, c in enumerate(uniq)}
    assert same_bits(da.rank_candidates(gen_d, table_d, ([key_of[id(c)] for c in inp["candidates"]], uniq), N), ranked)
    by_name = {f"category {i}": c for i, c in enumerate(uniq)}
    assert same_bits(da.rank_candidates(gen_d, table_d, ([f"category {key_of[id(c)]}" for c in inp["candidates"]], by_name), N), ranked)
    # a smaller list is the head of the larger one
    top10 = da.rank_candidates(gen_d, table_d, inp["candidates"], 10)
    assert torch.equal(top10.ids, ranked.ids[:, :10]) and torch.equal(top10.sims.view(torch.int32), ranked.sims[:, :10].contiguous().view(torch.int32))
    assert torch.equal(top10.counts, ranked.counts.clamp(max=10))


def test_guard_rows_and_workspace_are_respected():
    """Straight through the C entry point: one sentinel row behind every output and a pattern behind the workspace stay untouched."""
    inp, fx, gen_d, table_d, ranked = case_run("main")
    shared = inp["shared_rows"]
    cand = inp["candidates"][shared[0]].to(DEV)
    g = gen_d[shared].contiguous()
    rows, n = len(shared), len(cand)
    gn, tn = da.embed_row_norms(g), da.embed_row_norms(table_d)
    need = _lib.raw().dfh_embed_rank_workspace_bytes(rows, n, N)
    ws = torch.full((need + 1024,), 0xAB, dtype=torch.uint8, device=DEV)
    ids = torch.full((rows + 1, N), -7, dtype=torch.int64, device=DEV)
    pos, sims = torch.full_like(ids, -7), torch.full((rows + 1, N), float("nan"), device=DEV)
    counts = torch.full((rows + 1,), -7, dtype=torch.int32, device=DEV)
    off, rs = (C.c_int64 * 2)(0, n), (C.c_int * rows)(*([0] * rows))
    args = lambda nmax, nbytes: (_lib.ptr(g), _lib.ptr(gn), rows, g.shape[1], _lib.ptr(table_d), _lib.ptr(tn), table_d.shape[0], _lib.ptr(cand), off, 1, rs,
                                 nmax, _lib.ptr(ws), nbytes, _lib.ptr(ids), _lib.ptr(pos), _lib.ptr(sims), _lib.ptr(counts), _lib.stream_ptr())
    with pytest.raises(da.DfhError, match="nmax must be in"):
        _lib.call("dfh_embed_rank", *args(129, need))
    with pytest.raises(da.DfhError, match="workspace smaller than"):
        _lib.call("dfh_embed_rank", *args(N, need - 1))
    with pytest.raises(ValueError, match="top_n must be in 1 .. 128"):
        da.rank_candidates(gen_d, table_d, inp["candidates"], 129)
    _lib.call("dfh_embed_rank", *args(N, need))
    torch.cuda.synchronize()
    assert (ids[-1] == -7).all() and (pos[-1] == -7).all() and torch.isnan(sims[-1]).all() and int(counts[-1]) == -7
    assert (ws[need:] == 0xAB).all()
    assert same_bits(da.RankResult(ids[:-1], pos[:-1], sims[:-1], counts[:-1]), rows_of(ranked, shared))
    with pytest.raises(IndexError):
        da.rank_candidates(gen_d, table_d[:100], inp["candidates"], N)


def test_fp16_storage_library_gives_the_same_bits():
    """The row is fp32 only: libdifashion_hip_f16.so, in a process of its own, gives the bits of the bf16 build."""
    name = "main"
    _, _, _, _, ranked = case_run(name)
    release_cached_gpu_memory()
    env = dict(os.environ, DFH_STORAGE="fp16")
    env.pop("DFH_LIB", None)
    r = subprocess.run([sys.executable, "-m", "tests.grounding_fp16_child", name], capture_output=True, text=True, env=env, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("GROUNDING_FP16_RESULT ")]
    assert line, r.stdout[-2000:]
    res = json.loads(line[-1][len("GROUNDING_FP16_RESULT "):])
    assert res["storage"] == "fp16" and "storage=fp16" in res["build_info"]
    assert res["ids"] == ranked.ids.flatten().tolist() and res["positions"] == ranked.positions.flatten().tolist()
    assert res["sims"] == ranked.sims.flatten().cpu().view(torch.int32).tolist() and res["counts"] == ranked.counts.tolist()


def test_grounding_retrieval_and_the_reference_signature():
    inp, fx, gen_d, table_d, ranked = case_run("main")
    rows = gen_d.shape[0]
    cs = da.CLIPScore(Recorded())
    preds, recall, again = cs.grounding_retrieval(gen_d, table_d, inp["candidates"], H.TOPN, inp["grds"], batch_size=32)
    assert same_bits(again, ranked) and torch.equal(preds, ranked.preds) and recall == fx["recall"].tolist()
    assert cs.grounding_retrieval([g for g in gen_d], table_d, inp["candidates"], H.TOPN)[1] is None
    p2, r2, _ = cs.grounding_retrieval_from_features(gen_d, table_d, inp["candidates"], H.TOPN, inp["grds"].tolist())
    assert torch.equal(p2, preds) and r2 == recall
    # the reference's signature over a dataset of (image, candidates) pairs, CPU-side as a Dataset yields them
    gen4eval = [(inp["gen"][r], inp["candidates"][r]) for r in range(rows)]
    for fn in (da.clip_og_retrieval_given_data, da.clip_gor_retrieval_given_data):
        p3, r3 = fn(gen4eval, inp["grds"].tolist(), inp["table"], 16, list(H.TOPN), DEV, num_workers=0, clip=cs)
        assert torch.equal(p3.cpu(), torch.from_numpy(fx["preds"])) and r3 == fx["recall"].tolist()
    # at K = 5 the best id is CLIPScore.retrieval's prediction on the existing retrieval inputs
    gen, table, cand = HE.retrieval_inputs("k5")
    g5, t5 = gen.to(DEV), table.to(DEV)
    sims5, pred5 = cs.retrieval(g5, t5, cand)
    best, _, r5 = cs.grounding_retrieval(g5, t5, [c for c in cand], topN=(1, 5))
    assert torch.equal(best.cpu(), cand[torch.arange(cand.shape[0]), pred5.cpu()]) and r5.positions[:, 0].tolist() == pred5.tolist()
    assert float((r5.sims[:, 0] - sims5.max(dim=1).values).abs().max()) <= H.rank_bound(gen.shape[1]) + HE.pair_bound(gen.shape[1], 1.0)

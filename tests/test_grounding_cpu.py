"""The grounding-retrieval row without a GPU: the new entry points are declared, built into both libraries and bound
with matching argument counts; every argument guard that needs no device; the pure-Python candidate-set and band helpers; the fixtures'
own conditions recomputed in fp64 (gaps, ladder foot above the crowd, the reference's ranking = the stated order); the recall arithmetic."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import difashion_amd as da
from difashion_amd import _lib, evalscores as ES
from tests import helpers_grounding as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ["dfh_embed_row_norms", "dfh_embed_rank_workspace_bytes", "dfh_embed_rank", "dfh_embed_recall"]
P = C.c_void_p(256)              # a non-null, 256-byte aligned stand-in: every guard below fires before a pointer is followed
NULL = C.c_void_p(0)


def test_new_symbols_in_header_both_libraries_and_binding():
    src = open(os.path.join(ROOT, "include", "difashion_hip.h")).read()
    assert "#define DFH_ABI_VERSION 8" in src and "#define DFH_EMBED_RANK_NMAX 128" in src
    decl = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    lib = _lib.raw()
    f16 = C.CDLL(os.path.join(_lib.CSRC, "libdifashion_hip_f16.so"))
    for n in NEW_SYMBOLS:
        m = re.search(r"\b%s\s*\(([^;]*?)\)\s*;" % n, decl, flags=re.S)
        assert m, n
        assert len(m.group(1).split(",")) == len(_lib.SIGNATURES[n][1]), n          # as many arguments bound as declared
        assert hasattr(lib, n) and hasattr(f16, n), n
    assert lib.dfh_abi_version() == 8 and ES.RANK_NMAX == 128
    for name in ("rank_candidates", "embed_row_norms", "recall_at", "RankResult", "clip_og_retrieval_given_data", "clip_gor_retrieval_given_data"):
        assert name in da.__all__ and hasattr(da, name)
    assert da.clip_gor_retrieval_given_data is da.clip_og_retrieval_given_data
    assert hasattr(da.CLIPScore, "grounding_retrieval") and hasattr(da.CLIPScore, "grounding_retrieval_from_features")


def test_workspace_query_is_host_arithmetic():
    q = _lib.raw().dfh_embed_rank_workspace_bytes
    assert q(1, 1, 100) == 64 * 4 + 256 and q(70, 300, 100) == 70 * 320 * 4 + 256 and q(3, 64, 1) == 3 * 64 * 4 + 256
    assert q(2, 0, 5) == 2 * 64 * 4 + 256                       # an empty set still has a row of the block
    assert q(8192, 20000, 100) == 8192 * 20032 * 4 + 256        # beyond 2^31 bytes of products: size_t arithmetic
    assert q(0, 5, 5) == 0 and q(1, -1, 5) == 0 and q(1, 5, 0) == 0 and q(1, 5, 129) == 0


def rank_call(**kw):
    a = dict(gen=P, gen_norms=P, rows=2, dim=8, table=P, table_norms=P, table_rows=10, cand=P, set_off=[0, 3, 5], row_set=[0, 1], nmax=4, ws=P,
             ws_bytes=1 << 20, ids=P, pos=P, sims=P, counts=P)
    a.update(kw)
    off = (C.c_int64 * len(a["set_off"]))(*a["set_off"]) if a["set_off"] is not None else NULL
    rs = (C.c_int * len(a["row_set"]))(*a["row_set"]) if a["row_set"] is not None else NULL
    _lib.call("dfh_embed_rank", a["gen"], a["gen_norms"], a["rows"], a["dim"], a["table"], a["table_norms"], a["table_rows"], a["cand"], off,
              len(a["set_off"]) - 1 if a["set_off"] is not None else 1, rs, a["nmax"], a["ws"], a["ws_bytes"], a["ids"], a["pos"], a["sims"],
              a["counts"], NULL)


def test_rank_guards_are_reached_without_a_device():
    for k in ("gen", "gen_norms", "table", "table_norms", "cand", "ws", "ids", "pos", "sims", "counts"):
        with pytest.raises(da.DfhError, match="null argument"):
            rank_call(**{k: NULL})
    with pytest.raises(da.DfhError, match="null argument"):
        rank_call(set_off=None)
    with pytest.raises(da.DfhError, match="must be positive"):
        rank_call(rows=0)
    with pytest.raises(da.DfhError, match="multiple of 4"):
        rank_call(dim=10)
    with pytest.raises(da.DfhError, match="16-byte aligned"):
        rank_call(table=C.c_void_p(264))
    with pytest.raises(da.DfhError, match="256-byte aligned"):
        rank_call(ws=C.c_void_p(272))
    for bad in (0, 129):
        with pytest.raises(da.DfhError, match=r"nmax must be in \[1, DFH_EMBED_RANK_NMAX \(128\)\]"):
            rank_call(nmax=bad)
    with pytest.raises(da.DfhError, match="set_off must be monotone"):
        rank_call(set_off=[0, 5, 3])
    with pytest.raises(da.DfhError, match="set_off must start"):
        rank_call(set_off=[-1, 3, 5])
    with pytest.raises(da.DfhError, match=r"outside \[0, nsets\)"):
        rank_call(row_set=[0, 2])
    with pytest.raises(da.DfhError, match="grouped by set"):
        rank_call(row_set=[1, 0])
    # two rows, longest set 3 -> 2 x 64 floats + 256
    with pytest.raises(da.DfhError, match="workspace smaller than dfh_embed_rank_workspace_bytes"):
        rank_call(ws_bytes=2 * 64 * 4 + 255)
    with pytest.raises(da.DfhError, match="null argument"):
        _lib.call("dfh_embed_row_norms", NULL, P, 1, 4, NULL)
    with pytest.raises(da.DfhError, match="multiple of 4"):
        _lib.call("dfh_embed_row_norms", P, P, 1, 6, NULL)
    with pytest.raises(da.DfhError, match="null argument"):
        _lib.call("dfh_embed_recall", P, P, 1, 4, NULL, P, 1, P, P, NULL)
    with pytest.raises(da.DfhError, match="nmax must be in"):
        _lib.call("dfh_embed_recall", P, P, 1, 129, P, P, 1, P, P, NULL)
    with pytest.raises(da.DfhError, match="up to 64 cutoffs"):
        _lib.call("dfh_embed_recall", P, P, 1, 4, P, P, 65, P, P, NULL)
    with pytest.raises(da.DfhError, match="up to 64 cutoffs"):
        _lib.call("dfh_embed_recall", P, P, 1, 4, P, NULL, 2, P, P, NULL)


def test_candidate_sets_ragged_duplicate_empty_and_out_of_range():
    a, b = torch.tensor([5, 1, 9]), torch.tensor([2, 2, 7, 0], dtype=torch.int32)
    flat, off, row_set, order = ES._candidate_sets([a, b, a, [5, 1, 9], [], torch.tensor([2, 2, 7, 0]), []], 7, 10)
    # identity first (rows 0 and 2), content second (row 3 a list, row 5 another dtype), the empty list is a set like any other
    assert row_set == [0, 1, 0, 0, 2, 1, 2] and off == [0, 3, 7, 7] and flat.tolist() == [5, 1, 9, 2, 2, 7, 0] and flat.dtype == torch.int64
    assert order == [0, 2, 3, 1, 5, 4, 6]                                 # by set, stable
    # the (set ids, sets) forms: a dict keyed by category, a list indexed by position
    sets = {"tops": a, "shoes": b}
    flat2, off2, rs2, order2 = ES._candidate_sets((["shoes", "tops", "shoes"], sets), 3, 10)
    assert rs2 == [0, 1, 0] and off2 == [0, 4, 7] and flat2.tolist() == [2, 2, 7, 0, 5, 1, 9] and order2 == [0, 2, 1]
    assert ES._candidate_sets((torch.tensor([1, 1, 0]), [a, b]), 3, 10)[2] == [0, 0, 1]
    # two rows given as a tuple of two id tensors are two rows, not the (set ids, sets) form
    assert ES._candidate_sets((a, b), 2, 10)[2] == [0, 1]
    flat3, off3, _, _ = ES._candidate_sets([[], []], 2, 10)
    assert flat3.numel() == 0 and off3 == [0, 0]
    for bad in ([a, torch.tensor([3, 10])], [a, [-1]]):
        with pytest.raises(IndexError, match=r"out of range \[0, 10\)"):
            ES._candidate_sets(bad, 2, 10)
    with pytest.raises(ValueError, match="holds 2 lists for 3 rows"):
        ES._candidate_sets([a, b], 3, 10)
    with pytest.raises(TypeError, match="integer ids"):
        ES._candidate_sets([torch.tensor([0.5])], 1, 10)
    with pytest.raises(ValueError, match="1-D"):
        ES._candidate_sets([torch.zeros(2, 2, dtype=torch.long)], 1, 10)
    with pytest.raises(IndexError, match="names no candidate set"):
        ES._candidate_sets((["hats"], sets), 1, 10)


def test_rank_bands_cover_the_rows_under_the_cap():
    lens = [1] * 3 + [300] * 70 + [2500] * 2
    assert ES._rank_bands(lens, 1 << 30) == [(0, 75)]
    for cap in (1, 4096, 320 * 4 * 30, 2560 * 4):
        bands = ES._rank_bands(lens, cap)
        assert bands[0][0] == 0 and bands[-1][1] == len(lens) and all(a[1] == b[0] for a, b in zip(bands, bands[1:]))
        for a, b in bands:
            ld = (max(lens[a:b]) + 63) // 64 * 64
            assert b > a and (b - a == 1 or (b - a) * ld * 4 <= cap)
    assert ES._rank_bands(lens, 1) == [(r, r + 1) for r in range(75)] and ES._rank_bands([], 100) == []


@pytest.mark.parametrize("name", list(H.CASES))
def test_fixture_conditions_recomputed_in_fp64(name):
    inp, fx = H.case_inputs(name), H.load_fixture(name)
    np.testing.assert_allclose(fx["checksum"], H.checksum(inp), rtol=1e-12)
    n = H.TOPN[-1]
    rows = inp["gen"].shape[0]
    assert fx["ids"].shape == (rows, n) and list(fx["topn"]) == list(H.TOPN)
    assert sorted(set(inp["set_len"])) == sorted(set(H.CASES[name]["lens"]) | ({H.CASES[name]["shared"][0]} if H.CASES[name]["shared"] else set()))
    hit_pos, smallest, crowd_top = [], np.inf, -np.inf
    for r in range(rows):
        cand = inp["candidates"][r]
        sims = H.cosine64(inp["gen"][r], inp["table"], cand)
        k = min(len(cand), n)
        if len(cand) > 1:
            smallest = min(smallest, H.ladder_gaps(sims, min(len(cand), n + 1) - 1).min())
        ranked = np.sort(sims)[::-1]
        if len(cand) > H.LADDER:
            assert ranked[H.LADDER - 1] > 0.34 and ranked[H.LADDER] < H.CROWD_MAX      # the ladder's foot stands above the crowd
            crowd_top = max(crowd_top, ranked[H.LADDER])
        pos = H.expected_ranking(sims, n)
        assert fx["counts"][r] == k and fx["positions"][r, :k].tolist() == pos and fx["ids"][r, :k].tolist() == cand[pos].tolist()
        assert (fx["ids"][r, k:] == -1).all() and (fx["positions"][r, k:] == -1).all() and np.isneginf(fx["sims"][r, k:]).all()
        assert np.abs(fx["sims"][r, :k].astype(np.float64) - sims[pos]).max() <= 2.0 ** -24
        assert fx["preds"][r] == fx["ids"][r, 0]
        where = np.nonzero(fx["ids"][r, :k] == int(inp["grds"][r]))[0]
        hit_pos.append(int(where[0]) if len(where) else -1)
    assert smallest > 1e-3 and float(fx["min_gap"]) > 1e-3 and abs(smallest - float(fx["min_gap"])) < 1e-9
    assert float(fx["ref_sims"]) < 1e-5 and H.rank_bound(inp["gen"].shape[1]) < H.LADDER_STEP / 500
    print(f"grounding fixture {name}: smallest gap {smallest:.6e}, crowd top {crowd_top:.3f}, torch fp32 off by {float(fx['ref_sims']):.2e}")
    # the recall arithmetic from hit positions: the reference's `grd in topN_iids[:N]`
    assert H.recall_from_hit_positions(hit_pos, H.TOPN) == fx["recall"].tolist()
    if name == "main":
        assert len(inp["shared_rows"]) == 70 and len({id(inp["candidates"][r]) for r in inp["shared_rows"]}) == 1
        assert {h for h in hit_pos} >= {-1, 0, 9, 10, 19, 20, 49, 50, 99}               # both sides of every cutoff are populated


def test_recall_arithmetic_from_hit_positions():
    assert H.recall_from_hit_positions([0, 9, 10, -1, 99, 100], (10, 20, 50, 100)) == [2 / 6, 3 / 6, 3 / 6, 4 / 6]
    assert H.recall_from_hit_positions(torch.tensor([-1, -1]), (1,)) == [0.0]
    assert H.recall_from_hit_positions([0, 3, -1, 7], (1, 5)) == [0.25, 0.5]


def test_special_rows_expected_order_is_the_stated_rule():
    inp = H.special_inputs()
    want = {}
    for name, g, cand in zip(H.SPECIAL_ROWS, inp["gen"], inp["candidates"]):
        sims = H.cosine64(g, inp["table"], cand)
        pos = H.expected_ranking(sims, H.TOPN[-1])
        assert len(pos) == len(cand) < H.TOPN[-1]
        want[name] = (sims, pos, cand)
    sims, pos, cand = want["dup"]
    twice = [j for j in range(len(cand)) if int(cand[j]) == 3]
    assert len(twice) == 2 and pos[3:5] == twice and sims[twice[0]] == sims[twice[1]]
    sims, pos, cand = want["twins"]
    pair = sorted(j for j in range(len(cand)) if int(cand[j]) in (23, 40))
    assert pos[3:5] == pair and torch.equal(inp["table"][23], inp["table"][40])
    sims, pos, cand = want["nan"]
    nans = [j for j in range(len(cand)) if np.isnan(sims[j])]
    assert len(nans) == 2 and pos[:2] == nans and {int(cand[j]) for j in nans} == {61, 62}
    sims, pos, cand = want["zero"]
    assert [int(cand[j]) for j in pos[10:12]] == [79, 78] and pos[10] == 2 and pos[11] == 9 and sims[2] == 0 and sims[9] == 0
    assert (sims[pos[:10]] > 0.8).all() and (sims[pos[12:]] < -0.8).all()
    assert H.expected_ranking([0.0, -0.0, float("nan"), 1.0, float("nan"), -0.0], 6) == [2, 4, 3, 0, 1, 5]


class _Fake(torch.Tensor):
    """A tensor that says it lives on the GPU: the checks below run before anything touches the device."""
    @property
    def device(self):
        return torch.device("cuda", 0)


def test_python_refusals():
    gen, table = torch.zeros(3, 8), torch.zeros(10, 8)
    with pytest.raises(da.DfhError, match="no CPU fallback"):
        da.rank_candidates(gen, table, [[0]] * 3, 5)
    with pytest.raises(da.DfhError, match="no CPU fallback"):
        da.embed_row_norms(table)
    fg, ft = gen.as_subclass(_Fake), table.as_subclass(_Fake)
    for bad in (0, 129):
        with pytest.raises(ValueError, match="top_n must be in 1 .. 128"):
            da.rank_candidates(fg, ft, [[0]] * 3, bad)
    with pytest.raises(IndexError, match="out of range"):
        da.rank_candidates(fg, ft, [[0], [10], [1]], 5, table_norms=torch.zeros(10).as_subclass(_Fake))
    with pytest.raises(ValueError, match="multiple of 4"):
        da.rank_candidates(torch.zeros(3, 6).as_subclass(_Fake), torch.zeros(10, 6).as_subclass(_Fake), [[0]] * 3, 5)
    cs = da.CLIPScore(image_model=None)
    with pytest.raises(ValueError, match="ascending positive cutoffs"):
        cs.grounding_retrieval_from_features(fg, ft, [[0]] * 3, topN=(20, 10))
    for bad in ("euclidean", "eiclidean"):
        with pytest.raises(ValueError, match=f"Unrecognized similarity function {bad}."):
            da.clip_og_retrieval_given_data([(gen[0], [0])], [0], table, 1, [10], similarity_func=bad, clip=cs)

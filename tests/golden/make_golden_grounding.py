#!/usr/bin/env python3
"""Golden vectors for the grounding retrieval from the REAL reference function.  Build machine only (needs the reference
checkout, found as make_golden_compat.py finds it); the committed ``grounding_*.npz`` are what travels.

``Evaluation/eval_utils.py`` is imported as make_golden_eval_scores.py imports it: names-only stubs, the ``open_clip`` stub's model
handing back its argument from ``encode_image``, so the "images" fed to the reference are the recorded embeddings.  What runs is the
reference's own ``clip_og_retrieval_given_data`` (eval_utils.py:725-767), one row at a time as it does, on the CPU in fp64 (recorded) and
in fp32.  It returns only ``(preds, all_recall)``; the similarities and the ``topk`` indices it ranks by are caught on the way by
wrapping the NAMES ``F.cosine_similarity`` and ``torch.topk`` inside eval_utils -- no arithmetic lives in the wrappers.

The script asserts, per row, a gap above 1e-3 between consecutive similarities through rank min(len, 101) in fp64, that the fp32 run
ranks identically, and that the returned ``preds`` are the first column of the caught ranking.  The rows whose order the reference does
not define (ties, NaN, signed zeros: helpers_grounding.special_inputs) are not recorded here.

    python tests/golden/make_golden_grounding.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import make_golden_eval_scores  # noqa: E402
from helpers_grounding import CASES, TOPN, case_inputs, checksum, fixture_path, ladder_gaps  # noqa: E402


class TorchNames:
    """Stands where eval_utils' ``torch`` name stands: every attribute is torch's own, ``topk`` records what it returns."""

    def __init__(self, caught):
        self._caught = caught

    def __getattr__(self, k):
        return getattr(torch, k)

    def topk(self, *a, **kw):
        out = torch.topk(*a, **kw)
        self._caught.append(out[1])
        return out


def run(eu, sims_caught, topk_caught, inp, dtype):
    del sims_caught[:], topk_caught[:]
    rows = inp["gen"].shape[0]
    gen4eval = [(inp["gen"][r].to(dtype), inp["candidates"][r]) for r in range(rows)]
    preds, all_recall = eu.clip_og_retrieval_given_data(gen4eval, inp["grds"].tolist(), inp["table"].to(dtype), 1, list(TOPN), "cpu", num_workers=0)
    assert len(sims_caught) == rows and len(topk_caught) == rows
    n = TOPN[-1]
    ids, pos = np.full((rows, n), -1, np.int64), np.full((rows, n), -1, np.int64)
    sims = np.full((rows, n), -np.inf, np.float64)
    for r in range(rows):
        idx = topk_caught[r]
        k = len(idx)
        assert k == min(n, len(inp["candidates"][r]))
        pos[r, :k], ids[r, :k] = idx.numpy(), inp["candidates"][r][idx].numpy()
        sims[r, :k] = sims_caught[r][idx].double().numpy()
        assert int(preds[r]) == ids[r, 0]
    return ids, pos, sims, preds.numpy(), np.array(all_recall, dtype=np.float64), [s.double().numpy() for s in sims_caught]


def main():
    torch.manual_seed(0)
    torch.set_grad_enabled(False)
    eu, sims_caught = make_golden_eval_scores.import_eval_utils()
    topk_caught = []
    eu.torch = TorchNames(topk_caught)
    for name in CASES:
        inp = case_inputs(name)
        ids, pos, sims, preds, recall, full = run(eu, sims_caught, topk_caught, inp, torch.float64)
        ids32, pos32, sims32, preds32, recall32, _ = run(eu, sims_caught, topk_caught, inp, torch.float32)
        gaps = []
        for r, s in enumerate(full):
            if len(s) > 1:
                gaps.append(float(ladder_gaps(s, min(len(s), TOPN[-1] + 1) - 1).min()))
                assert gaps[-1] > 1e-3, (name, r, gaps[-1])
        assert np.array_equal(ids, ids32) and np.array_equal(pos, pos32) and np.array_equal(recall, recall32), "fp32 and fp64 must rank identically"
        stored = sims.astype(np.float32)
        held = np.isfinite(sims)                                   # the -inf padding of rows shorter than the list is not a distance
        off = float(np.abs(sims32[held] - stored.astype(np.float64)[held]).max())
        np.savez_compressed(fixture_path(name), checksum=checksum(inp), ids=ids, positions=pos, sims=stored, preds=preds, recall=recall,
                            topn=np.array(TOPN), counts=np.array([min(TOPN[-1], len(c)) for c in inp["candidates"]], dtype=np.int32),
                            ref_sims=np.array(off), min_gap=np.array(min(gaps)))
        print(f"wrote grounding_{name}.npz: {ids.shape[0]} rows, recall {recall.tolist()}, smallest gap {min(gaps):.6e}, torch fp32 off by {off:.2e}")


if __name__ == "__main__":
    main()

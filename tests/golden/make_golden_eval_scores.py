#!/usr/bin/env python3
"""Golden vectors for the embedding score kernels from the REAL reference functions.  Build machine only (needs the
reference checkout, DIFASHION_REFERENCE or /root/reference); the committed ``evalscore_*.npz`` are what travels.

``Evaluation/eval_utils.py`` is imported behind the names-only stubs of make_golden_compat.py.  Its ``CLIPScore.__init__`` asks
``open_clip`` for a model: the stub hands back an object whose ``encode_image`` / ``encode_text`` RETURN THEIR ARGUMENT, so the
"images" and "texts" fed to the reference are the recorded embeddings themselves -- no arithmetic lives in the stub.  What runs is the
reference's own
  * ``CLIPScore.calculate_clip_score`` and ``calculate_clip_img_score`` (eval_utils.py:101-135) and, one row a call (it returns a mean),
    ``evaluate_personalization_given_data_sim`` (:503-538): the three must agree on every pair case;
  * ``calculate_clip_retrieval_acc_given_data2`` (:687-723) for the retrieval cases; it returns the predictions, and the similarity
    matrix it takes the argmax of is caught on the way by wrapping the ``F.cosine_similarity`` NAME inside eval_utils.
Every case runs in fp64 (recorded, stored as fp32) and in fp32 (``ref_*``: the largest absolute distance of that run from the record).
The script asserts that the best candidate of every retrieval row stands more than 1e-3 clear of the second best in fp64, except in
the row with the planted tie (two equal ids), where the tied pair stands that clear of the rest: ``pred`` must match exactly.

    python tests/golden/make_golden_eval_scores.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import make_golden_compat  # noqa: E402
from helpers_eval_scores import (PAIR_CASES, RETRIEVAL_CASES, TIE_ROW, fixture_path, pair_inputs, retrieval_inputs,  # noqa: E402
                                 scores_checksum)


class RecordedEmbeddings:
    """Stands where the OpenCLIP model stands: the encoders hand back what they are given."""

    def to(self, *a, **kw):
        return self

    def eval(self):
        return self

    def encode_image(self, x):
        return x

    def encode_text(self, x):
        return x


def import_eval_utils():
    make_golden_compat.import_reference()
    import eval_utils
    oc = sys.modules["open_clip"]
    oc.create_model_and_transforms = lambda *a, **kw: (RecordedEmbeddings(), None, None)
    oc.get_tokenizer = lambda *a, **kw: None
    caught = []
    real_f = eval_utils.F

    def cosine_similarity(*a, **kw):
        out = real_f.cosine_similarity(*a, **kw)
        caught.append(out)
        return out
    eval_utils.F = types.SimpleNamespace(cosine_similarity=cosine_similarity)
    return eval_utils, caught


def pair_scores(eu, a, b):
    clip = eu.CLIPScore(device="cpu")
    s = clip.calculate_clip_score(a, b)
    assert torch.equal(clip.calculate_clip_img_score(a, b), s)
    per_row = [eu.evaluate_personalization_given_data_sim([(a[r], b[r])], 1, "cpu", num_workers=0) for r in range(a.shape[0])]
    assert torch.equal(torch.tensor(per_row, dtype=s.dtype), s)
    return s


def retrieval(eu, caught, gen, table, cand):
    del caught[:]
    acc, preds = eu.calculate_clip_retrieval_acc_given_data2([(gen[r], cand[r]) for r in range(gen.shape[0])], table, gen.shape[0], "cpu",
                                                             num_workers=0)
    assert len(caught) == 1 and caught[0].shape == cand.shape
    return caught[0], preds, acc


def main():
    torch.manual_seed(0)
    torch.set_grad_enabled(False)
    eu, caught = import_eval_utils()
    for name in PAIR_CASES:
        a, b = pair_inputs(name)
        s64 = pair_scores(eu, a.double(), b.double())
        s32 = pair_scores(eu, a, b)
        stored = s64.float()
        np.savez_compressed(fixture_path("evalscore_pair_" + name), checksum=scores_checksum(a, b), scores=stored.numpy(),
                            ref_scores=np.array(float((s32.double() - stored.double()).abs().max())))
        print(f"wrote evalscore_pair_{name}.npz: {tuple(a.shape)}, scores {float(s64.min()):.2f} .. {float(s64.max()):.2f}, torch fp32 off by "
              f"{float((s32.double() - stored.double()).abs().max()):.2e}")
    for name in RETRIEVAL_CASES:
        gen, table, cand = retrieval_inputs(name)
        sims64, pred64, acc = retrieval(eu, caught, gen.double(), table.double(), cand)
        sims32, pred32, _ = retrieval(eu, caught, gen, table, cand)
        K = cand.shape[1]
        gaps = []
        for r in range(gen.shape[0]):
            top = torch.sort(sims64[r], descending=True).values
            if K > 1 and r == TIE_ROW:
                assert top[0] == top[1] and int(pred64[r]) == 0, "the planted tie must be the best pair, resolved to the lower index"
                top = top[1:]
            if len(top) > 1:
                gaps.append(float(top[0] - top[1]))
                assert gaps[-1] > 1e-3, (name, r, gaps[-1])
        stored = sims64.float()
        np.savez_compressed(fixture_path("evalscore_retrieval_" + name), checksum=scores_checksum(gen, table, cand), sims=stored.numpy(),
                            pred=pred64.numpy(), candidates=cand.numpy(), tie_row=np.array(TIE_ROW if K > 1 else -1),
                            ref_sims=np.array(float((sims32.double() - stored.double()).abs().max())))
        print(f"wrote evalscore_retrieval_{name}.npz: K = {K}, accuracy {acc:.2f}, pred {pred64.tolist()}, smallest gap "
              f"{min(gaps) if gaps else float('nan'):.3f}, torch fp32 off by {float((sims32.double() - stored.double()).abs().max()):.2e}")


if __name__ == "__main__":
    main()

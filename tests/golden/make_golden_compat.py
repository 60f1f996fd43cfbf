#!/usr/bin/env python3
"""Golden vectors for the compatibility scorer from the REAL reference classes.  Build machine only (needs the
reference checkout, DIFASHION_REFERENCE or /root/reference); the committed ``compat_*.npz`` are what travels.

``Evaluation/compatibility_evaluator/compatibility_net.py`` and ``Evaluation/eval_utils.py`` die at import here (torchvision,
open_clip, lpips, pytorch_fid are absent): ``sys.modules`` stubs supply the NAMES they import and nothing else -- no arithmetic lives
in a stub.  What runs is the reference's own ``FashionEvaluator`` (eval mode: Dropout is the identity) under the reference's own
``CompatibilityEvaluator.evaluate_compatibility`` (eval_utils.py:574-588), called on an object that carries only ``.evaluator``
(its ``__init__`` would download an OpenCLIP checkpoint).  Per case of ``tests/helpers_eval_scores.COMPAT_CASES``: seeded weights
under the class's state-dict names, seeded feature tables and olists, the run in fp64 (recorded, stored as fp32) and in fp32
(``ref_*``: its distance from the recorded values; for the logits relative L2 over the case, and ``ref_abs_logits`` the largest
absolute difference, which the single-outfit case is held to).

    python tests/golden/make_golden_compat.py [case ...]
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
REF = os.path.join(os.environ.get("DIFASHION_REFERENCE", "/root/reference"), "Evaluation")

from helpers_eval_scores import (COMPAT_CASES, compat_case_inputs, compat_checksum, compat_gather, fixture_path, pair_order,  # noqa: E402
                                 rel)


def import_reference():
    """(FashionEvaluator, evaluate_compatibility) of the reference, imported behind names-only stubs."""
    def stub(name, **attrs):
        if name not in sys.modules:
            m = types.ModuleType(name)
            for k, v in attrs.items():
                setattr(m, k, v)
            sys.modules[name] = m
        return sys.modules[name]
    try:
        import torchvision  # noqa: F401
    except ImportError:
        stub("torchvision").models = stub("torchvision.models", inception_v3=None)
    stub("pytorch_fid").fid_score = stub("pytorch_fid.fid_score", calculate_frechet_distance=None)
    sys.modules["pytorch_fid"].inception = stub("pytorch_fid.inception", fid_inception_v3=None)
    stub("lpips")
    stub("open_clip")
    try:
        import tqdm  # noqa: F401
    except ImportError:
        stub("tqdm", tqdm=lambda it, **kw: it)
    sys.path.insert(0, REF)
    from compatibility_evaluator.compatibility_net import FashionEvaluator
    import eval_utils
    return FashionEvaluator, eval_utils.CompatibilityEvaluator.evaluate_compatibility


def run(FashionEvaluator, evaluate_compatibility, params, real, gen, ol, dtype):
    ev = FashionEvaluator(cnn_feat_dim=real.shape[1]).eval().to(dtype)
    assert list(ev.state_dict()) == list(params), "state-dict names / order differ from tests/helpers_eval_scores.compat_param_shapes"
    ev.load_state_dict({k: v.to(dtype) for k, v in params.items()})
    holder = types.SimpleNamespace(evaluator=ev)
    scores = evaluate_compatibility(holder, [list(map(int, row)) for row in ol], real.to(dtype), gen.to(dtype))
    feats = compat_gather(real, gen, ol).to(dtype)
    emb = ev.outfit_emb(feats)
    logits = ev.pred_score(emb)
    assert torch.equal(torch.sigmoid(ev(feats)), scores) and torch.equal(torch.sigmoid(logits), scores)
    return emb, logits, scores


def main(names):
    torch.manual_seed(0)
    torch.set_grad_enabled(False)
    FashionEvaluator, evaluate_compatibility = import_reference()
    for name in names:
        params, real, gen, ol = compat_case_inputs(name)
        O, items, dim, _ = COMPAT_CASES[name]
        assert (ol > 0).any() and (ol <= 0).any() and int(ol[0, 0]) == 0
        e64, l64, s64 = run(FashionEvaluator, evaluate_compatibility, params, real, gen, ol, torch.float64)
        e32, l32, s32 = run(FashionEvaluator, evaluate_compatibility, params, real, gen, ol, torch.float32)
        # the synthetic weights exercise the network: live ReLUs, scores off the sigmoid's rails and not all alike
        assert 0.05 < float((e64 > 0).double().mean()) < 0.95 and 0.02 < float(s64.min()) and float(s64.max()) < 0.98
        rec = {"checksum": compat_checksum(params, real, gen, ol), "olists": ol.numpy(), "param_names": np.array(list(params)),
               "pair_order": np.array(pair_order(items)), "ref_abs_logits": np.array(float((l32.double() - l64.float().double()).abs().max()))}
        for key, t64, t32 in (("outfit_emb", e64, e32), ("logits", l64, l32), ("scores", s64, s32)):
            stored = t64.float()
            rec[key] = stored.numpy()
            rec["ref_" + key] = np.array(rel(t32, stored))
        np.savez_compressed(fixture_path("compat_" + name), **rec)
        print(f"wrote compat_{name}.npz ({os.path.getsize(fixture_path('compat_' + name)) / 1024:.0f} KiB): {O} outfits x {items} items x {dim}, "
              f"scores {float(s64.min()):.3f} .. {float(s64.max()):.3f}, live ReLU share {float((e64 > 0).double().mean()):.2f}, "
              f"ref_fp32 outfit_emb={float(rec['ref_outfit_emb']):.2e} logits={float(rec['ref_logits']):.2e} "
              f"(abs {float(rec['ref_abs_logits']):.2e}) scores={float(rec['ref_scores']):.2e}")


if __name__ == "__main__":
    main(sys.argv[1:] or list(COMPAT_CASES))

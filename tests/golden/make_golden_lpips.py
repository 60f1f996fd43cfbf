#!/usr/bin/env python3
"""Golden vectors for the LPIPS row.  Build machine only; the committed ``lpips_*.npz`` are what travels.

The ``lpips`` package and ``torchvision`` are not installed here, so the network is the plain-torch restatement of
tests/helpers_lpips.py (an UNPINNED oracle: its conv, pool and division are torch's own).  Per case of ``helpers_lpips.CASES``, 8 pairs at
the full VGG16 widths with seeded weights and inputs: the restatement's run in fp64 (``per_layer64``, ``total64``, stored as fp32), the
VALUES of its own fp32 run (``per_layer32``, ``total32``) and a checksum of the weights and inputs.  The float image of the uint8 case
comes from the reference's own ``im2tensor_lpips`` (Evaluation/eval_utils.py:467-470; DIFASHION_REFERENCE or /root/reference), imported
behind names-only stubs as tests/golden/make_golden_compat.py does.  ``lpips_retrieval.npz`` holds the fp64 scores, ``torch.argmin``
predictions and accuracy of the 3 x 5 retrieval case.  The order of ``torch.argmin`` (a NaN wins, then the lowest index) is pinned here
against torch on ``helpers_lpips.ARGMIN_ROWS``.

    python tests/golden/make_golden_lpips.py [case ...]
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
REF = os.path.join(os.environ.get("DIFASHION_REFERENCE", "/root/reference"), "Evaluation")

import helpers_lpips as H  # noqa: E402


def import_im2tensor():
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
    import eval_utils
    return eval_utils.im2tensor_lpips


def main(names):
    torch.manual_seed(0)
    torch.set_grad_enabled(False)
    im2tensor_lpips = import_im2tensor()
    params = H.make_params()
    # torch.argmin's order, which the argmin kernel and helpers_lpips.argmin_order restate
    rows = torch.from_numpy(H.ARGMIN_ROWS)
    assert np.array_equal(torch.argmin(rows, dim=-1).numpy(), H.argmin_order(H.ARGMIN_ROWS)), "torch.argmin's order differs from the restatement"
    assert torch.argmin(rows, dim=-1).tolist() == [1, 1, 0, 0, 4, 1]
    for name in names:
        a, b = H.case_inputs(name)
        if H.CASES[name][2] == "u8":
            fa, fb = (torch.stack([im2tensor_lpips(im.numpy()) for im in t]) for t in (a, b))
            assert torch.equal(fa, H.im2tensor(a)) and torch.equal(fb, H.im2tensor(b)) and fa.dtype == torch.float32
        else:
            fa, fb = a, b
        p64, t64 = H.lpips_forward(params, fa, fb, torch.float64)
        p32, t32 = H.lpips_forward(params, fa, fb, torch.float32)
        live = [float((t > 0).double().mean()) for t in H.vgg_taps(params, H.scaling_layer(params, fa.double()))]
        assert all(0.3 < v < 0.7 for v in live), live
        rec = {"checksum": H.checksum(params, a, b), "per_layer64": p64.float().numpy(), "total64": t64.float().numpy(),
               "per_layer32": p32.numpy(), "total32": t32.numpy()}
        np.savez_compressed(H.fixture_path("lpips_" + name), **rec)
        print(f"wrote lpips_{name}.npz ({os.path.getsize(H.fixture_path('lpips_' + name))} bytes): total {float(t64.min()):.3e} .. {float(t64.max()):.3e}, "
              f"live ReLU share per tap {' '.join(f'{v:.2f}' for v in live)}, fp32 distance total {H.rel(t32, t64):.2e} per layer "
              + " ".join(f"{H.rel(p32[:, k], p64[:, k]):.2e}" for k in range(5)))
    gen, cand = H.retrieval_inputs()
    _, s64 = H.lpips_forward(params, gen, cand, torch.float64)
    rows_n, K = H.RETRIEVAL[:2]
    s64 = s64.reshape(rows_n, K)
    preds = torch.argmin(s64, dim=-1)
    assert preds.tolist() == list(H.NEAREST)
    srt = s64.sort(dim=-1).values
    assert float((srt[:, 1] / srt[:, 0]).min()) > 1.5, "the nearest candidate must win by a margin no fp32 rounding can close"
    np.savez_compressed(H.fixture_path("lpips_retrieval"), checksum=H.checksum(params, gen, cand), scores64=s64.float().numpy(), preds=preds.numpy(),
                        accuracy=np.array(float((preds == 0).sum()) / rows_n))
    print(f"wrote lpips_retrieval.npz: preds {preds.tolist()} accuracy {float((preds == 0).sum()) / rows_n:.4f}")


if __name__ == "__main__":
    main(sys.argv[1:] or list(H.CASES))

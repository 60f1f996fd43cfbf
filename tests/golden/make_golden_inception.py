#!/usr/bin/env python3
"""Golden vectors for the FID / Inception Score row.  Build machine only; the committed ``inception_*.npz`` are what travels.

``torchvision`` and ``pytorch_fid`` are not installed here, so the network is the plain-torch restatement of tests/helpers_inception.py (an
UNPINNED oracle: its conv, batch_norm, pools and interpolate are torch's own).  Per case of ``helpers_inception.CASES``, 4 images at the
full Inception v3 widths: the conv / fc weights come from seeds, the BatchNorm running statistics are CALIBRATED on the case's own inputs
(every BatchNorm sees zero-mean, unit-variance input, so about half of every ReLU is live at any depth) and committed in the fixture
(``bn_mean``, ``bn_var``: the 94 layers' vectors in table order).  Stored: the four pooled taps of the fp64 run (``tap{b}_64``) and the
VALUES of the restatement's own fp32 run (``tap{b}_32``), for ``tv`` the probabilities and labels, the live ReLU shares and a checksum.

The score arithmetic of ``helpers_inception.inception_score`` is held against the reference's own
``calculate_inception_score_given_data`` (Evaluation/eval_utils.py:339-406; DIFASHION_REFERENCE or /root/reference) on canned
probabilities: the module is imported behind names-only stubs, its network class replaced by one that returns the canned rows.

    python tests/golden/make_golden_inception.py [case ...]
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
REF = os.path.join(os.environ.get("DIFASHION_REFERENCE", "/root/reference"), "Evaluation")

import helpers_inception as H  # noqa: E402


def import_eval_utils():
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
    return eval_utils


def check_score_arithmetic():
    """helpers_inception.inception_score == the reference's own lines, on canned probabilities, for one and for three splits."""
    eval_utils = import_eval_utils()
    g = torch.Generator().manual_seed(5)
    canned = torch.softmax(3.0 * torch.randn((11, 50), generator=g), dim=1)
    cate = torch.argmax(canned, dim=1)
    cate[::3] = (cate[::3] + 1) % 50

    class Canned(torch.nn.Module):
        def __init__(self, model_path, num_classes):
            super().__init__()
            self.num_classes, self.at = num_classes, 0

        def forward(self, x):
            rows = canned[self.at:self.at + x.shape[0]]
            self.at += x.shape[0]
            return rows

    eval_utils.InceptionV3 = Canned
    for splits in (1, 3):
        ref = eval_utils.calculate_inception_score_given_data(torch.rand(11, 3, 8, 8), cate, None, 50, 4, "cpu", num_workers=0, num_splits=splits)
        mine = H.inception_score(canned, cate, splits)
        assert np.allclose(ref, mine, rtol=1e-6, atol=0, equal_nan=True), (ref, mine)
        assert np.isnan(ref[2]) == (splits == 1)
    print("inception_score restatement == calculate_inception_score_given_data on canned probabilities (1 and 3 splits)")


def main(names):
    torch.manual_seed(0)
    torch.set_grad_enabled(False)
    check_score_arithmetic()
    for name in names:
        variant, _, _, classes, _ = H.CASES[name]
        params = H.make_params(variant, classes or 50)
        x = H.case_inputs(name)
        chk = H.checksum(params, x)
        H.Net(params, variant, torch.float64, calibrate=True).forward(x)
        r64 = H.Net(params, variant, torch.float64).forward(x)
        r32 = H.Net(params, variant, torch.float32).forward(x)
        convs = [row[0] for row in H.layer_table()]
        rec = {"checksum": chk, "live": np.array(r64["live"]),
               "bn_mean": torch.cat([params[n + ".bn.running_mean"] for n in convs]).numpy(),
               "bn_var": torch.cat([params[n + ".bn.running_var"] for n in convs]).numpy()}
        dist = []
        for b in range(4):
            t64, t32 = r64["taps"][b], r32["taps"][b]
            assert t64.shape == (H.IMAGES, H.BLOCK_DIMS[b]) and bool(torch.isfinite(t64).all()) and bool(torch.isfinite(t32).all())
            assert 0.2 < r64["live"][b] < 0.8, (name, b, r64["live"])
            dist.append(H.rel(t32, t64))
            assert dist[-1] > 0, "the fp32 run must differ from the fp64 run: the yardstick of the GPU test is this distance"
            rec[f"tap{b}_64"], rec[f"tap{b}_32"] = t64.numpy(), t32.numpy()
        extra = ""
        if variant == "tv":
            p64, p32 = r64["probs"], r32["probs"]
            top = p64.sort(dim=1, descending=True).values
            margin = top[:, 0] - top[:, 1]
            # a run three times the fp32 run's distance away (what the GPU test allows) moves top-1 and runner-up by 3 err each: 10 err is safe
            assert float(margin.min()) > 10 * float((p32.double() - p64).abs().max()), "the top-1 class must lead by a margin the fp32 run does not close"
            assert torch.equal(torch.argmax(p64, 1), torch.argmax(p32, 1))
            rec.update(probs_64=p64.numpy(), probs_32=p32.numpy(), labels=torch.argmax(p64, 1).numpy())
            extra = f", top-1 margin >= {float(margin.min()):.3e}, probs fp32 distance {H.rel(p32, p64):.2e}, labels {torch.argmax(p64, 1).tolist()}"
        np.savez_compressed(H.fixture_path("inception_" + name), **rec)
        size = os.path.getsize(H.fixture_path("inception_" + name))
        assert size < 1 << 20, size
        print(f"wrote inception_{name}.npz ({size} bytes): live ReLU share per tap {' '.join(f'{v:.2f}' for v in r64['live'])}, fp32 distance per tap "
              + " ".join(f"{d:.2e}" for d in dist) + extra)


if __name__ == "__main__":
    main(sys.argv[1:] or list(H.CASES))

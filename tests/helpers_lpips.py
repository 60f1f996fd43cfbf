"""What the LPIPS tests share: a plain-torch restatement of ``lpips.LPIPS(net="vgg", version="0.1")``, the seeded
parameters and inputs of the fixture cases, and the fixture files.

The oracle is UNPINNED: neither the ``lpips`` package nor ``torchvision`` is installed where the fixtures are made, so the network is
restated here from the package's published source -- the ScalingLayer, torchvision's ``vgg16().features`` up to ``relu5_3`` (thirteen
``F.conv2d(padding=1)`` + ReLU, ``F.max_pool2d(2, 2)`` in front of slices 2 to 5), ``normalize_tensor`` with eps 1e-10 OUTSIDE the root,
the squared difference, the bias-free 1 x 1 ``lin`` conv, the spatial mean and the sum over the five layers.  Its convolution, pooling and
division are torch's own.  Only ``im2tensor_lpips`` of the uint8 case comes from the reference's own code
(tests/golden/make_golden_lpips.py).
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
# (C_out, torchvision features index, slice) of the thirteen convs; a slice ends in a tap
CONVS = [(64, 0, 1), (64, 2, 1), (128, 5, 2), (128, 7, 2), (256, 10, 3), (256, 12, 3), (256, 14, 3), (512, 17, 4), (512, 19, 4), (512, 21, 4),
         (512, 24, 5), (512, 26, 5), (512, 28, 5)]
TAP_CHANNELS = (64, 128, 256, 512, 512)
PAIRS = 8
PARAM_SEED = 20
# case -> (H, W, input form, seed)
CASES = {"min_16x16": (16, 16, "f32", 1), "odd_21x27": (21, 27, "f32", 2), "two_tiles_37x45": (37, 45, "f32", 3), "u8_24x40": (24, 40, "u8", 4)}
RETRIEVAL = (3, 5, 16, 16, 9)           # rows, K, H, W, seed


def rel(a: torch.Tensor, b: torch.Tensor) -> float:
    return float((a.double() - b.double()).norm() / b.double().norm())


def fixture_path(stem: str) -> str:
    return os.path.join(GOLDEN, stem + ".npz")


def load_fixture(stem: str):
    return dict(np.load(fixture_path(stem)))


def param_shapes():
    """The 33 entries of the package's state dict (without the duplicate ``lins.*``), in order."""
    shapes = {"scaling_layer.shift": (1, 3, 1, 1), "scaling_layer.scale": (1, 3, 1, 1)}
    cin = 3
    for cout, idx, sl in CONVS:
        shapes[f"net.slice{sl}.{idx}.weight"] = (cout, cin, 3, 3)
        shapes[f"net.slice{sl}.{idx}.bias"] = (cout,)
        cin = cout
    for k, c in enumerate(TAP_CHANNELS):
        shapes[f"lin{k}.model.1.weight"] = (1, c, 1, 1)
    return shapes


def make_params(seed: int = PARAM_SEED):
    """Conv weights randn * sqrt(2 / (9 C_in)), biases 0.1 randn, lin weights rand * 2 / C (non-negative, as the trained ones are), the
    package's shift / scale constants: about half of every tap's ReLUs are live and the distances are of the order 1e-2."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name, shape in param_shapes().items():
        if name == "scaling_layer.shift":
            t = torch.tensor(SHIFT).view(shape)
        elif name == "scaling_layer.scale":
            t = torch.tensor(SCALE).view(shape)
        elif name.startswith("lin"):
            t = torch.rand(shape, generator=g) * (2.0 / shape[1])
        elif name.endswith(".weight"):
            t = torch.randn(shape, generator=g) * (2.0 / (9 * shape[1])) ** 0.5
        else:
            t = 0.1 * torch.randn(shape, generator=g)
        out[name] = t
    return out


def im2tensor(u8_nhwc: torch.Tensor) -> torch.Tensor:
    """``im2tensor_lpips`` (eval_utils.py:467-470) per image: float64 ``v / 127.5 - 1``, then float32, CHW."""
    return torch.from_numpy(np.ascontiguousarray((u8_nhwc.numpy() / (255. / 2.) - 1.).transpose(0, 3, 1, 2)).astype(np.float32))


def case_inputs(name: str):
    """(in0, in1): fp32 [8, 3, H, W] in [-1, 1], or for the uint8 case uint8 [8, H, W, 3]; in1 = clamp(in0 + 0.5 randn)."""
    H, W, form, seed = CASES[name]
    g = torch.Generator().manual_seed(seed)
    if form == "u8":
        a = torch.randint(0, 256, (PAIRS, H, W, 3), generator=g, dtype=torch.uint8)
        b = (a.float() + 0.5 * 127.5 * torch.randn((PAIRS, H, W, 3), generator=g)).round().clamp(0, 255).to(torch.uint8)
        return a, b
    a = torch.rand((PAIRS, 3, H, W), generator=g) * 2 - 1
    b = (a + 0.5 * torch.randn((PAIRS, 3, H, W), generator=g)).clamp(-1, 1)
    return a, b


def retrieval_inputs():
    """(gen, candidates): rows * K fp32 images each.  Row r's generated image is repeated K times; its nearest candidate (the image
    plus a little noise) sits at index NEAREST[r], the others are unrelated images."""
    rows, K, H, W, seed = RETRIEVAL
    g = torch.Generator().manual_seed(seed)
    base = torch.rand((rows, 3, H, W), generator=g) * 2 - 1
    gen = base[:, None].expand(rows, K, 3, H, W).reshape(rows * K, 3, H, W).contiguous()
    cand = torch.rand((rows, K, 3, H, W), generator=g) * 2 - 1
    for r, k in enumerate(NEAREST):
        cand[r, k] = (base[r] + 0.05 * torch.randn((3, H, W), generator=g)).clamp(-1, 1)
    return gen, cand.reshape(rows * K, 3, H, W).contiguous()


NEAREST = (0, 3, 0)


def checksum(params, in0, in1) -> np.ndarray:
    ts = [params["net.slice1.0.weight"], params["net.slice5.28.bias"], params["lin4.model.1.weight"], in0, in1]
    return np.array([float(t.double().sum()) for t in ts] + [float(t.double().abs().sum()) for t in ts])


# ------------------------------------------------------------------ the restatement
def scaling_layer(params, x):
    return (x - params["scaling_layer.shift"].to(x.dtype)) / params["scaling_layer.scale"].to(x.dtype)


def vgg_taps(params, x):
    """relu1_2, relu2_2, relu3_3, relu4_3, relu5_3 of ``x`` [N, 3, H, W] (already scaled), in x's dtype."""
    taps, sl_now = [], 1
    for cout, idx, sl in CONVS:
        if sl != sl_now:
            taps.append(x)
            x = F.max_pool2d(x, kernel_size=2, stride=2)
            sl_now = sl
        x = F.relu(F.conv2d(x, params[f"net.slice{sl}.{idx}.weight"].to(x.dtype), params[f"net.slice{sl}.{idx}.bias"].to(x.dtype), padding=1))
    return taps + [x]


def normalize_tensor(x, eps=1e-10):
    return x / (torch.sqrt(torch.sum(x ** 2, dim=1, keepdim=True)) + eps)


def layer_score(f0, f1, lin_weight):
    """[N]: spatial mean of the 1 x 1 lin conv over (normalize(f0) - normalize(f1))^2."""
    d = (normalize_tensor(f0) - normalize_tensor(f1)) ** 2
    return F.conv2d(d, lin_weight.to(d.dtype)).mean([2, 3]).reshape(-1)


def lpips_forward(params, in0, in1, dtype=torch.float32, normalize=False):
    """-> (per_layer [N, 5], total [N]) in ``dtype``; in0 / in1 fp32 NCHW."""
    in0, in1 = in0.to(dtype), in1.to(dtype)
    if normalize:
        in0, in1 = 2 * in0 - 1, 2 * in1 - 1
    t0, t1 = vgg_taps(params, scaling_layer(params, in0)), vgg_taps(params, scaling_layer(params, in1))
    per = torch.stack([layer_score(a, b, params[f"lin{k}.model.1.weight"]) for k, (a, b) in enumerate(zip(t0, t1))], dim=1)
    total = per[:, 0]
    for k in range(1, 5):
        total = total + per[:, k]
    return per, total


def argmin_order(scores: np.ndarray) -> np.ndarray:
    """``torch.argmin(dim=-1)`` restated: a NaN is the minimum, the lowest index wins among equals (and among NaNs)."""
    out = np.zeros(scores.shape[0], np.int64)
    for r, row in enumerate(scores):
        best, bk = row[0], 0
        for k in range(1, len(row)):
            if best != best:
                break
            if row[k] != row[k] or row[k] < best:
                best, bk = row[k], k
        out[r] = bk
    return out


ARGMIN_ROWS = np.array([[3., 1., 2., 1., 5.], [2., float("nan"), 0., float("nan"), 1.], [0., 0., 0., 0., 0.], [float("nan")] * 5,
                        [4., 3., 2., 1., 0.], [float("inf"), -float("inf"), 0., -float("inf"), 1.]], np.float32)

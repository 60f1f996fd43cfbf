"""What the Inception tests share: a plain-torch restatement of the two Inception v3 variants of the reference's
evaluation, the shape table of every layer, the seeded parameters and inputs of the fixture cases, and the fixture files.

The oracle is UNPINNED: neither ``torchvision`` nor ``pytorch_fid`` is installed where the fixtures are made, so the network is restated
here from their published sources -- every ``BasicConv2d`` as ``F.conv2d(bias=None)`` -> ``F.batch_norm(eps=1e-3, running statistics)`` ->
ReLU, the Mixed blocks with torchvision's layer names, ``tv`` (``inception_v3`` with ``transform_input`` and ``fc``: pool branches
``F.avg_pool2d(3, 1, 1)``) and ``fid`` (``fid_inception_v3``: ``count_include_pad=False``, ``Mixed_7c`` pools with ``F.max_pool2d(3, 1, 1)``,
no ``fc``).  Its convolution, normalisation, pooling and interpolation are torch's own, runnable in fp32 and fp64.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BLOCK_DIMS = (64, 192, 768, 2048)
SIDE = 299
IMAGES = 4
PARAM_SEED = 30
# case -> (variant, H, W, num_classes, input seed)
CASES = {"fid_up_75x91": ("fid", 75, 91, 0, 1), "fid_299": ("fid", 299, 299, 0, 2), "tv_down_320x300": ("tv", 320, 300, 50, 3)}


def rel(a, b) -> float:
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / b.norm())


def fixture_path(stem: str) -> str:
    return os.path.join(GOLDEN, stem + ".npz")


def load_fixture(stem: str):
    return dict(np.load(fixture_path(stem)))


# ------------------------------------------------------------------ the shape table
def _pair(v):
    return (v, v) if isinstance(v, int) else tuple(v)


def layer_table():
    """[(name, C_in, C_out, (KH, KW), stride, (padH, padW))] of the 94 BasicConv2d in torchvision's module order (AuxLogits left out)."""
    t = []

    def add(name, cin, cout, k, stride=1, pad=0):
        t.append((name, cin, cout, _pair(k), stride, _pair(pad)))

    add("Conv2d_1a_3x3", 3, 32, 3, 2)
    add("Conv2d_2a_3x3", 32, 32, 3)
    add("Conv2d_2b_3x3", 32, 64, 3, 1, 1)
    add("Conv2d_3b_1x1", 64, 80, 1)
    add("Conv2d_4a_3x3", 80, 192, 3)
    cin = 192
    for name, pf in (("Mixed_5b", 32), ("Mixed_5c", 64), ("Mixed_5d", 64)):
        add(name + ".branch1x1", cin, 64, 1)
        add(name + ".branch5x5_1", cin, 48, 1)
        add(name + ".branch5x5_2", 48, 64, 5, 1, 2)
        add(name + ".branch3x3dbl_1", cin, 64, 1)
        add(name + ".branch3x3dbl_2", 64, 96, 3, 1, 1)
        add(name + ".branch3x3dbl_3", 96, 96, 3, 1, 1)
        add(name + ".branch_pool", cin, pf, 1)
        cin = 224 + pf
    add("Mixed_6a.branch3x3", 288, 384, 3, 2)
    add("Mixed_6a.branch3x3dbl_1", 288, 64, 1)
    add("Mixed_6a.branch3x3dbl_2", 64, 96, 3, 1, 1)
    add("Mixed_6a.branch3x3dbl_3", 96, 96, 3, 2)
    for name, c7 in (("Mixed_6b", 128), ("Mixed_6c", 160), ("Mixed_6d", 160), ("Mixed_6e", 192)):
        add(name + ".branch1x1", 768, 192, 1)
        add(name + ".branch7x7_1", 768, c7, 1)
        add(name + ".branch7x7_2", c7, c7, (1, 7), 1, (0, 3))
        add(name + ".branch7x7_3", c7, 192, (7, 1), 1, (3, 0))
        add(name + ".branch7x7dbl_1", 768, c7, 1)
        add(name + ".branch7x7dbl_2", c7, c7, (7, 1), 1, (3, 0))
        add(name + ".branch7x7dbl_3", c7, c7, (1, 7), 1, (0, 3))
        add(name + ".branch7x7dbl_4", c7, c7, (7, 1), 1, (3, 0))
        add(name + ".branch7x7dbl_5", c7, 192, (1, 7), 1, (0, 3))
        add(name + ".branch_pool", 768, 192, 1)
    add("Mixed_7a.branch3x3_1", 768, 192, 1)
    add("Mixed_7a.branch3x3_2", 192, 320, 3, 2)
    add("Mixed_7a.branch7x7x3_1", 768, 192, 1)
    add("Mixed_7a.branch7x7x3_2", 192, 192, (1, 7), 1, (0, 3))
    add("Mixed_7a.branch7x7x3_3", 192, 192, (7, 1), 1, (3, 0))
    add("Mixed_7a.branch7x7x3_4", 192, 192, 3, 2)
    for name, cin in (("Mixed_7b", 1280), ("Mixed_7c", 2048)):
        add(name + ".branch1x1", cin, 320, 1)
        add(name + ".branch3x3_1", cin, 384, 1)
        add(name + ".branch3x3_2a", 384, 384, (1, 3), 1, (0, 1))
        add(name + ".branch3x3_2b", 384, 384, (3, 1), 1, (1, 0))
        add(name + ".branch3x3dbl_1", cin, 448, 1)
        add(name + ".branch3x3dbl_2", 448, 384, 3, 1, 1)
        add(name + ".branch3x3dbl_3a", 384, 384, (1, 3), 1, (0, 1))
        add(name + ".branch3x3dbl_3b", 384, 384, (3, 1), 1, (1, 0))
        add(name + ".branch_pool", cin, 192, 1)
    return t


LAYERS = {row[0]: row for row in layer_table()}
BN_LEAVES = ("bn.weight", "bn.bias", "bn.running_mean", "bn.running_var")
BLOCK_KIND = {"Mixed_5b": "A", "Mixed_5c": "A", "Mixed_5d": "A", "Mixed_6a": "B", "Mixed_6b": "C", "Mixed_6c": "C", "Mixed_6d": "C", "Mixed_6e": "C",
              "Mixed_7a": "D", "Mixed_7b": "E", "Mixed_7c": "E"}


def param_shapes(variant: str, num_classes: int = 50):
    """The state dict the HIP classes keep, in order: five entries a BasicConv2d, then ``fc.*`` for ``tv``."""
    shapes = {}
    for name, cin, cout, k, _, _ in layer_table():
        shapes[name + ".conv.weight"] = (cout, cin, k[0], k[1])
        for leaf in BN_LEAVES:
            shapes[f"{name}.{leaf}"] = (cout,)
    if variant == "tv":
        shapes["fc.weight"] = (num_classes, 2048)
        shapes["fc.bias"] = (num_classes,)
    return shapes


def make_params(variant: str, num_classes: int = 50, seed: int = PARAM_SEED):
    """Conv weights randn * sqrt(2 / fan_in), BN weight in [0.75, 1.25], BN bias 0.1 randn, running statistics (0, 1) until
    ``calibrate`` replaces them (the fixtures carry the calibrated ones), fc weight and bias 0.1 randn."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name, shape in param_shapes(variant, num_classes).items():
        if name.endswith(".conv.weight"):
            t = torch.randn(shape, generator=g) * (2.0 / (shape[1] * shape[2] * shape[3])) ** 0.5
        elif name.endswith(".bn.weight"):
            t = 0.75 + 0.5 * torch.rand(shape, generator=g)
        elif name.endswith(".bn.running_mean"):
            t = torch.zeros(shape)
        elif name.endswith(".bn.running_var"):
            t = torch.ones(shape)
        else:
            t = 0.1 * torch.randn(shape, generator=g)
        out[name] = t
    return out


def foreign_state_dict(params, variant: str):
    """What the foreign checkpoint carries beside ``params``: ``num_batches_tracked`` per BatchNorm, ``AuxLogits.*`` and (``fid``) ``fc.*``."""
    sd = {}
    for k, v in params.items():
        sd[k] = v.clone()
        if k.endswith(".bn.running_var"):
            sd[k.replace("running_var", "num_batches_tracked")] = torch.tensor(7)
    sd.update({"AuxLogits.conv0.conv.weight": torch.zeros(128, 768, 1, 1), "AuxLogits.conv0.bn.num_batches_tracked": torch.tensor(7),
               "AuxLogits.fc.weight": torch.zeros(50, 768), "AuxLogits.fc.bias": torch.zeros(50)})
    if variant == "fid":
        sd.update({"fc.weight": torch.zeros(1008, 2048), "fc.bias": torch.zeros(1008)})
    return sd


def case_inputs(name: str) -> torch.Tensor:
    """fp32 [4, 3, H, W] in [0, 1]: a smooth colour ramp per image plus noise, so that resizing has something to interpolate."""
    _, H, W, _, seed = CASES[name]
    g = torch.Generator().manual_seed(seed)
    yy = torch.linspace(0, 1, H).view(1, 1, H, 1)
    xx = torch.linspace(0, 1, W).view(1, 1, 1, W)
    ph = torch.rand((IMAGES, 3, 1, 1), generator=g) * 6.28
    base = 0.5 + 0.25 * torch.sin(6.0 * yy + ph) * torch.cos(5.0 * xx - ph)
    return (base + 0.2 * torch.randn((IMAGES, 3, H, W), generator=g)).clamp(0, 1).contiguous()


def checksum(params, x) -> np.ndarray:
    """Weighted sums of the seeded (uncalibrated) parameters and the inputs: the fixture was made from these tensors."""
    s = 0.0
    for i, (k, v) in enumerate(params.items()):
        if not k.endswith(("running_mean", "running_var")):
            s += float(v.double().sum()) * (1 + i % 7)
    ramp = (torch.arange(x.numel(), dtype=torch.float64) % 13).view(x.shape)
    return np.array([s, float(x.double().sum()), float((x.double() * ramp).sum())])


# ------------------------------------------------------------------ the restatement
def prep(x, variant: str, resize_input: bool = True, normalize_input: bool = True):
    if resize_input:
        x = F.interpolate(x, size=(SIDE, SIDE), mode="bilinear", align_corners=False)
    if normalize_input:
        x = 2 * x - 1
    if variant == "tv":                                  # torchvision's _transform_input (weights='DEFAULT' switches it on)
        c0 = torch.unsqueeze(x[:, 0], 1) * (0.229 / 0.5) + (0.485 - 0.5) / 0.5
        c1 = torch.unsqueeze(x[:, 1], 1) * (0.224 / 0.5) + (0.456 - 0.5) / 0.5
        c2 = torch.unsqueeze(x[:, 2], 1) * (0.225 / 0.5) + (0.406 - 0.5) / 0.5
        x = torch.cat((c0, c1, c2), 1)
    return x


class Net:
    """One run of the restatement over ``params`` in ``dtype``.  ``calibrate``: every BatchNorm's running statistics are first set to
    the mean / biased variance of its own input over this batch (rounded to fp32), in ``params``."""

    def __init__(self, params, variant: str, dtype=torch.float32, calibrate: bool = False):
        self.p, self.variant, self.dtype, self.calibrate = params, variant, dtype, calibrate

    def conv(self, name, x):
        _, _, _, _, stride, pad = LAYERS[name]
        P = self.p
        y = F.conv2d(x, P[name + ".conv.weight"].to(self.dtype), None, stride, pad)
        if self.calibrate:
            P[name + ".bn.running_mean"] = y.double().mean((0, 2, 3)).float()
            P[name + ".bn.running_var"] = y.double().var((0, 2, 3), unbiased=False).float()
        y = F.batch_norm(y, P[name + ".bn.running_mean"].to(self.dtype), P[name + ".bn.running_var"].to(self.dtype),
                         P[name + ".bn.weight"].to(self.dtype), P[name + ".bn.bias"].to(self.dtype), False, 0.0, 1e-3)
        return F.relu(y)

    def chain(self, prefix, names, x):
        for n in names:
            x = self.conv(f"{prefix}.{n}", x)
        return x

    def avg(self, x):
        return F.avg_pool2d(x, 3, 1, 1) if self.variant == "tv" else F.avg_pool2d(x, 3, 1, 1, count_include_pad=False)

    def block(self, name, x):
        kind = BLOCK_KIND[name]
        if kind == "A":
            out = [self.conv(name + ".branch1x1", x), self.chain(name, ["branch5x5_1", "branch5x5_2"], x),
                   self.chain(name, ["branch3x3dbl_1", "branch3x3dbl_2", "branch3x3dbl_3"], x), self.conv(name + ".branch_pool", self.avg(x))]
        elif kind == "B":
            out = [self.conv(name + ".branch3x3", x), self.chain(name, ["branch3x3dbl_1", "branch3x3dbl_2", "branch3x3dbl_3"], x), F.max_pool2d(x, 3, 2)]
        elif kind == "C":
            out = [self.conv(name + ".branch1x1", x), self.chain(name, ["branch7x7_1", "branch7x7_2", "branch7x7_3"], x),
                   self.chain(name, ["branch7x7dbl_1", "branch7x7dbl_2", "branch7x7dbl_3", "branch7x7dbl_4", "branch7x7dbl_5"], x),
                   self.conv(name + ".branch_pool", self.avg(x))]
        elif kind == "D":
            out = [self.chain(name, ["branch3x3_1", "branch3x3_2"], x),
                   self.chain(name, ["branch7x7x3_1", "branch7x7x3_2", "branch7x7x3_3", "branch7x7x3_4"], x), F.max_pool2d(x, 3, 2)]
        else:
            b3 = self.conv(name + ".branch3x3_1", x)
            bd = self.chain(name, ["branch3x3dbl_1", "branch3x3dbl_2"], x)
            pooled = F.max_pool2d(x, 3, 1, 1) if self.variant == "fid" and name == "Mixed_7c" else self.avg(x)
            out = [self.conv(name + ".branch1x1", x), self.conv(name + ".branch3x3_2a", b3), self.conv(name + ".branch3x3_2b", b3),
                   self.conv(name + ".branch3x3dbl_3a", bd), self.conv(name + ".branch3x3dbl_3b", bd), self.conv(name + ".branch_pool", pooled)]
        return torch.cat(out, 1)

    def forward(self, x, resize_input: bool = True, normalize_input: bool = True, last_block: int = 3):
        """-> dict: ``taps`` (the four block outputs averaged over their pixels, [N, C] each), ``live`` (the share of positive values in
        the ReLU outputs that feed each tap) and for ``tv`` ``logits`` / ``probs``."""
        x = prep(x.to(self.dtype), self.variant, resize_input, normalize_input)
        taps, live = [], []

        def tap(feeds, t):
            live.append(float((feeds > 0).double().mean()))
            taps.append(t.mean((2, 3)))

        x = self.conv("Conv2d_1a_3x3", x)
        x = self.conv("Conv2d_2b_3x3", self.conv("Conv2d_2a_3x3", x))
        feeds = x
        x = F.max_pool2d(x, 3, 2)
        tap(feeds, x)
        if last_block >= 1:
            x = self.conv("Conv2d_4a_3x3", self.conv("Conv2d_3b_1x1", x))
            feeds = x
            x = F.max_pool2d(x, 3, 2)
            tap(feeds, x)
        if last_block >= 2:
            for name in ("Mixed_5b", "Mixed_5c", "Mixed_5d", "Mixed_6a", "Mixed_6b", "Mixed_6c", "Mixed_6d", "Mixed_6e"):
                x = self.block(name, x)
            tap(x, x)
        out = {"taps": taps, "live": live}
        if last_block >= 3:
            for name in ("Mixed_7a", "Mixed_7b", "Mixed_7c"):
                x = self.block(name, x)
            tap(x, x)
            if self.variant == "tv":
                out["logits"] = F.linear(taps[3], self.p["fc.weight"].to(self.dtype), self.p["fc.bias"].to(self.dtype))
                out["probs"] = torch.softmax(out["logits"], dim=1)
        return out


def load_case(name: str):
    """(variant, params with the fixture's calibrated BatchNorm statistics, inputs, fixture)."""
    variant, _, _, classes, _ = CASES[name]
    fx = load_fixture("inception_" + name)
    params = make_params(variant, classes or 50)
    convs = [row[0] for row in layer_table()]
    off = 0
    for n in convs:
        c = LAYERS[n][2]
        params[n + ".bn.running_mean"] = torch.from_numpy(fx["bn_mean"][off:off + c].copy())
        params[n + ".bn.running_var"] = torch.from_numpy(fx["bn_var"][off:off + c].copy())
        off += c
    return variant, params, case_inputs(name), fx


# ------------------------------------------------------------------ the score arithmetic of calculate_inception_score_given_data, restated
def inception_score(probs: torch.Tensor, cate: torch.Tensor, num_splits: int = 1, eps: float = 1e-16):
    """eval_utils.py:371-406 on ``probs`` in their own dtype: (acc, mean entropy, std entropy, mean score, std score)."""
    n, classes = probs.shape
    acc = int((torch.argmax(probs, dim=1) == cate).sum()) / n
    uniform = torch.ones(classes, dtype=probs.dtype) / classes
    scores, entropy = [], []
    for i in range(num_splits):
        part = probs[i * n // num_splits:(i + 1) * n // num_splits, :]
        ent = - part * torch.log(part + eps)
        entropy.append(torch.mean(torch.sum(ent, 1)))
        kl = part * (torch.log(part + eps) - torch.log(torch.unsqueeze(uniform, 0)))
        scores.append(torch.exp(torch.mean(torch.sum(kl, 1))))
    entropy, scores = torch.stack(entropy), torch.stack(scores)
    return acc, torch.mean(entropy).item(), torch.std(entropy).item(), torch.mean(scores).item(), torch.std(scores).item()

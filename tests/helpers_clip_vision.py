"""Case table shared by tests/golden/make_golden_clip_vision.py (writes the fixtures from the REAL
``transformers.CLIPVisionModelWithProjection``, run in fp64), tests/test_clip_vision_cpu.py and tests/test_gpu_clip_vision.py (HIP
encoder vs fixtures).  Weights and pixel inputs are regenerated from the seeds on every box (CPU generator: the same tensors
everywhere); the fixtures hold the real class's outputs plus a checksum of the inputs they were computed from.

Weight scales (``init_params``): chosen so that the tower is exercised, not idle, through its full depth -- q / k projections wide
enough for peaked but not one-hot softmaxes over up to 257 keys, residual branches that keep the stream finite over 32 blocks,
jittered LayerNorm affines, non-zero biases.  The fixture script asserts both conditions on the real class's attention maps."""
import dataclasses
import os
from typing import Dict, List, Tuple

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@dataclasses.dataclass(frozen=True)
class VisionConfig:
    """transformers ``CLIPVisionConfig`` key names."""
    hidden_size: int
    intermediate_size: int
    num_hidden_layers: int
    num_attention_heads: int
    image_size: int
    patch_size: int
    projection_dim: int
    hidden_act: str
    num_channels: int = 3
    layer_norm_eps: float = 1e-5

    @property
    def num_tokens(self) -> int:
        return 1 + (self.image_size // self.patch_size) ** 2

    def kwargs(self) -> dict:
        return dataclasses.asdict(self)


TINY_QUICKGELU = VisionConfig(64, 128, 2, 4, 56, 8, 32, "quick_gelu")          # T = 50
TINY_GELU = VisionConfig(64, 128, 2, 4, 42, 14, 32, "gelu")                    # T = 10
TINY_LONG = VisionConfig(64, 128, 2, 4, 112, 8, 32, "quick_gelu")              # T = 197: several key tiles, ragged ends
VIT_L_14 = VisionConfig(1024, 4096, 24, 16, 224, 14, 768, "quick_gelu")        # OpenAI CLIP ViT-L/14, head dim 64
VIT_H_14 = VisionConfig(1280, 5120, 32, 16, 224, 14, 1024, "gelu")             # OpenCLIP ViT-H/14, head dim 80: the reference's model

# name -> (config, weight seed, batch, full size: taps embeddings / middle / last on a fixed set of token rows)
CASES = {
    "tiny_quickgelu": (TINY_QUICKGELU, 21, 3, False),
    "tiny_gelu": (TINY_GELU, 22, 3, False),
    "tiny_long": (TINY_LONG, 23, 3, False),
    "vit_l_14": (VIT_L_14, 24, 2, True),
    "vit_h_14": (VIT_H_14, 25, 2, True),
}
TINY_CASES = [n for n, c in CASES.items() if not c[3]]
# token rows of the full-size cases the fixtures keep (a committed file stays small): the class token, both sides of every 64-key
# tile edge of the attention kernel, and the ragged last row
FULL_SIZE_ROWS = [0, 1, 2, 31, 32, 63, 64, 65, 100, 127, 128, 129, 160, 191, 192, 193, 224, 254, 255, 256]


def param_shapes(cfg: VisionConfig) -> List[Tuple[str, Tuple[int, ...]]]:
    """State-dict names, order and shapes of transformers' CLIPVisionModelWithProjection (tests/test_clip_vision_cpu.py checks this
    list against the real class)."""
    D, I, p = cfg.hidden_size, cfg.intermediate_size, cfg.patch_size
    vm = "vision_model."
    out = [(vm + "embeddings.class_embedding", (D,)), (vm + "embeddings.patch_embedding.weight", (D, cfg.num_channels, p, p)),
           (vm + "embeddings.position_embedding.weight", (cfg.num_tokens, D)), (vm + "pre_layrnorm.weight", (D,)), (vm + "pre_layrnorm.bias", (D,))]
    for l in range(cfg.num_hidden_layers):
        b = f"{vm}encoder.layers.{l}."
        for proj in ("k_proj", "v_proj", "q_proj", "out_proj"):
            out += [(f"{b}self_attn.{proj}.weight", (D, D)), (f"{b}self_attn.{proj}.bias", (D,))]
        out += [(b + "layer_norm1.weight", (D,)), (b + "layer_norm1.bias", (D,)), (b + "mlp.fc1.weight", (I, D)), (b + "mlp.fc1.bias", (I,)),
                (b + "mlp.fc2.weight", (D, I)), (b + "mlp.fc2.bias", (D,)), (b + "layer_norm2.weight", (D,)), (b + "layer_norm2.bias", (D,))]
    out += [(vm + "post_layernorm.weight", (D,)), (vm + "post_layernorm.bias", (D,)), ("visual_projection.weight", (cfg.projection_dim, D))]
    return out


def init_params(cfg: VisionConfig, seed: int) -> Dict[str, torch.Tensor]:
    """Seeded synthetic weights, drawn in table order from ONE CPU generator."""
    g = torch.Generator().manual_seed(seed)
    D = cfg.hidden_size
    out = {}
    for name, shape in param_shapes(cfg):
        leaf = name.split(".")[-2]
        r = torch.randn(shape, generator=g)
        if "norm" in leaf:
            t = r * 0.1 + (1.0 if name.endswith("weight") else 0.0)
        elif name.endswith(".bias"):
            t = r * 0.05
        elif name.endswith("class_embedding") or leaf == "position_embedding":
            t = r * 0.5
        elif leaf == "patch_embedding":
            t = r * (1.0 / (shape[1] * shape[2] * shape[3]) ** 0.5)
        elif leaf in ("q_proj", "k_proj"):
            t = r * (1.3 / D ** 0.5)
        else:
            t = r * (0.7 / shape[1] ** 0.5)
        out[name] = t
    return out


def pixel_inputs(cfg: VisionConfig, batch: int, seed: int) -> torch.Tensor:
    """Normalised-image-like inputs: unit-scale noise plus a smooth per-image, per-channel offset."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn((batch, cfg.num_channels, cfg.image_size, cfg.image_size), generator=g)
    return x + 0.5 * torch.randn((batch, cfg.num_channels, 1, 1), generator=g)


def case_inputs(name):
    cfg, seed, batch, _ = CASES[name]
    return cfg, init_params(cfg, seed), pixel_inputs(cfg, batch, seed + 1000)


def checksum(params, pixels) -> np.ndarray:
    """Fingerprint of the regenerated inputs (float64 sums of a few tensors + the pixels)."""
    keys = sorted(params)
    pick = [keys[0], keys[len(keys) // 2], keys[-1]]
    return np.array([float(params[k].double().sum()) for k in pick] + [float(params[k].double().abs().sum()) for k in pick]
                    + [float(pixels.double().sum()), float(pixels.double().abs().sum())])


def fixture_path(name):
    return os.path.join(GOLDEN, f"clipv_{name}.npz")


def load_fixture(name):
    return dict(np.load(fixture_path(name)))


def rows_of(fx, t: torch.Tensor) -> torch.Tensor:
    """The token rows of a [B, T, D] tensor that the fixture keeps (all of them for the tiny cases)."""
    return t[:, torch.from_numpy(fx["rows"]).long()] if "rows" in fx else t


def rel(a: torch.Tensor, b: torch.Tensor) -> float:
    return float((a.double() - b.double()).norm() / b.double().norm())

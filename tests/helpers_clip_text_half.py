"""Case table of the 16-bit (bf16 / fp16) CLIP text encoder, shared by tests/golden/make_golden_clip_text_half.py (fixtures and
yardsticks from the REAL ``transformers.CLIPTextModel`` / ``CLIPTextModelWithProjection``), tests/test_clip_text_half_cpu.py and
tests/test_gpu_clip_text_half.py.  Weights come from ``oracle.clip_ref.init_params`` and ids from ``prompt_like_ids`` (row 0 is the
empty prompt, the last row is full), exactly as tests/helpers_clip.py regenerates them; ``text_projection.weight`` is seeded here.

The tiny cases of the fp32 tower have head dims 16 and 32, which the 16-bit causal attention kernel (head dim 64) does not take; the
cases here are the smallest shapes at which the 16-bit walk can still go wrong:
  thalf_tiny_77   hidden 128, 2 heads, quick_gelu, argmax pooling (eos_token_id 2), batch 5, T = 77: four full 16-row slabs + 13,
                  M = 385 is ragged
  thalf_tiny_20   gelu, first-eos pooling (eos_token_id 999, pad 0), batch 3, T = 20: shorter than one wave's pair of slabs
  thalf_tiny_64   batch 2, T = 64: a whole number of slabs, the mask is the only edge
and the two full-size towers of tests/helpers_clip.py (same configs and seeds).

The rule: the HIP 16-bit path's distance from the fp64 values must be at most FACTOR x the real
class's own distance when it runs in the same 16-bit format (``clipt_half_yardsticks.npz``)."""
import os
from typing import Dict, List

import numpy as np
import torch

from oracle import clip_ref
from tests.helpers_clip import CASES as FP32_CASES
from tests.helpers_clip import GOLDEN, rel  # noqa: F401
from tests.helpers_clip_half import FACTOR, FORMATS, TORCH_DTYPE, max_one_minus_cos, yardstick  # noqa: F401

_TINY = dict(vocab_size=1000, hidden_size=128, intermediate_size=256, num_hidden_layers=2, num_attention_heads=2, bos_token_id=998)
THALF_TINY_77 = clip_ref.CLIPTextConfig(hidden_act="quick_gelu", eos_token_id=2, pad_token_id=999, **_TINY)
THALF_TINY_20 = clip_ref.CLIPTextConfig(hidden_act="gelu", eos_token_id=999, pad_token_id=0, **_TINY)
THALF_TINY_64 = clip_ref.CLIPTextConfig(hidden_act="quick_gelu", eos_token_id=2, pad_token_id=999, **_TINY)

# name -> (config, weight seed, batch, sequence length, projection_dim, full size)
HALF_CASES = {
    "thalf_tiny_77": (THALF_TINY_77, 41, 5, 77, 64, False),
    "thalf_tiny_20": (THALF_TINY_20, 42, 3, 20, 64, False),
    "thalf_tiny_64": (THALF_TINY_64, 43, 2, 64, 64, False),
    "sd15_clip_l": FP32_CASES["sd15_clip_l"][:4] + (768, True),
    "sd2_openclip_h": FP32_CASES["sd2_openclip_h"][:4] + (1024, True),
}
TINY_CASES = [n for n, c in HALF_CASES.items() if not c[5]]
YARDSTICKS = os.path.join(GOLDEN, "clipt_half_yardsticks.npz")


def config_kwargs(cfg) -> dict:
    return dict(vocab_size=cfg.vocab_size, hidden_size=cfg.hidden_size, intermediate_size=cfg.intermediate_size,
                num_hidden_layers=cfg.num_hidden_layers, num_attention_heads=cfg.num_attention_heads,
                max_position_embeddings=cfg.max_position_embeddings, hidden_act=cfg.hidden_act, layer_norm_eps=cfg.layer_norm_eps,
                eos_token_id=cfg.eos_token_id, bos_token_id=cfg.bos_token_id, pad_token_id=cfg.pad_token_id)


def projection_weight(cfg, seed: int, projection_dim: int) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed + 500)
    return torch.randn(projection_dim, cfg.hidden_size, generator=g) * (0.7 / cfg.hidden_size ** 0.5)


def case_inputs(name):
    """-> (config, tower parameters, text_projection.weight, ids)."""
    cfg, seed, batch, T, pdim, _ = HALF_CASES[name]
    return cfg, clip_ref.init_params(cfg, seed), projection_weight(cfg, seed, pdim), clip_ref.prompt_like_ids(cfg, batch, T, seed + 1000)


def checksum(params, proj, ids) -> np.ndarray:
    """Order-independent fingerprint of the regenerated inputs (float64 sums of a few tensors, the projection and the ids)."""
    keys = sorted(params)
    pick = [keys[0], keys[len(keys) // 2], keys[-1]]
    return np.array([float(params[k].double().sum()) for k in pick] + [float(params[k].double().abs().sum()) for k in pick]
                    + [float(proj.double().sum()), float(proj.double().abs().sum()), float(ids.double().sum())])


def eos_positions(cfg, ids: torch.Tensor) -> List[int]:
    pos = ids.argmax(dim=-1) if cfg.eos_token_id == 2 else (ids == cfg.eos_token_id).int().argmax(dim=-1)
    return [int(p) for p in pos]


def kept_rows(cfg, ids: torch.Tensor) -> List[int]:
    """Token rows a fixture keeps (a committed file stays small): every row of a short sequence; else rows 0, 1, both sides of the
    slab edges 16 / 32 / 64, the last two rows and each sequence's eos row."""
    T = ids.shape[-1]
    if T <= 64:
        return list(range(T))
    return sorted({0, 1, 15, 16, 31, 32, 63, 64, T - 2, T - 1} | set(eos_positions(cfg, ids)))


def kept_taps(name) -> List[int]:
    L = HALF_CASES[name][0].num_hidden_layers
    return [0, L // 2, L] if HALF_CASES[name][5] else list(range(L + 1))


def fixture_path(name: str) -> str:
    return os.path.join(GOLDEN, f"clipt_half_{name}.npz")


def load_fixture(name: str) -> Dict[str, np.ndarray]:
    return dict(np.load(fixture_path(name)))


def output_keys(fx) -> List[str]:
    return ["text_embeds", "pooler_output", "last_hidden_state"] + [f"hidden_{int(t)}" for t in fx["taps"]]

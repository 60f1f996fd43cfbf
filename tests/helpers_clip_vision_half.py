"""Case table of the 16-bit (bf16 / fp16) CLIP image encoder, shared by tests/golden/make_golden_clip_vision_half.py (fixtures and
yardsticks from the REAL ``transformers.CLIPVisionModelWithProjection``), tests/test_clip_vision_half_cpu.py and
tests/test_gpu_clip_vision_half.py.  Weights and pixels are regenerated from the seeds exactly as tests/helpers_clip_vision.py does.

The tiny cases of the fp32 tower have head dim 16, which the 16-bit attention kernels do not have; the cases here are the smallest
shapes at which the 16-bit walk can still go wrong:
  half_tiny_d64   head dim 64, T = 197 (three full key tiles + a ragged one, two query workgroups), patch K = 192, M = 591
  half_tiny_d80   head dim 80, T = 257 (the x32 attention kernel; V^T rows padded 257 -> 264), patch K = 588 -> 592, M = 771
  half_tiny_short head dim 64, T = 50: shorter than one key tile and one query workgroup
and the two full-size towers of tests/helpers_clip_vision.py, whose committed fp64 fixtures are reused.

The rule: the HIP 16-bit path's distance from the fp64 values must be at most FACTOR x the real
class's own distance when it runs in the same 16-bit format (``clipv_half_yardsticks.npz``)."""
import os
from typing import Dict, List

import numpy as np
from tests.helpers_clip_half import FACTOR, FORMATS, TORCH_DTYPE, max_one_minus_cos, yardstick  # noqa: F401
from tests.helpers_clip_vision import CASES as FP32_CASES
from tests.helpers_clip_vision import FULL_SIZE_ROWS, GOLDEN, VisionConfig, init_params, pixel_inputs, rel  # noqa: F401

HALF_TINY_D64 = VisionConfig(128, 256, 2, 2, 112, 8, 32, "quick_gelu")        # T = 197, d = 64
HALF_TINY_D80 = VisionConfig(160, 640, 2, 2, 224, 14, 64, "gelu")             # T = 257, d = 80, patch K = 588
HALF_TINY_SHORT = VisionConfig(128, 256, 2, 2, 56, 8, 32, "gelu")             # T = 50, d = 64

# name -> (config, weight seed, batch, full size)
HALF_CASES = {
    "half_tiny_d64": (HALF_TINY_D64, 31, 3, False),
    "half_tiny_d80": (HALF_TINY_D80, 32, 3, False),
    "half_tiny_short": (HALF_TINY_SHORT, 33, 2, False),
    "vit_l_14": FP32_CASES["vit_l_14"],
    "vit_h_14": FP32_CASES["vit_h_14"],
}
NEW_CASES = [n for n, c in HALF_CASES.items() if not c[3]]
YARDSTICKS = os.path.join(GOLDEN, "clipv_half_yardsticks.npz")


def case_inputs(name):
    cfg, seed, batch, _ = HALF_CASES[name]
    return cfg, init_params(cfg, seed), pixel_inputs(cfg, batch, seed + 1000)


def fixture_path(name: str) -> str:
    """The fp64 values of a case: the new tiny cases have files of their own, the full-size ones reuse the fp32 tower's."""
    return os.path.join(GOLDEN, f"clipv_half_{name}.npz" if name in NEW_CASES else f"clipv_{name}.npz")


def load_fixture(name: str) -> Dict[str, np.ndarray]:
    return dict(np.load(fixture_path(name)))


def kept_rows(T: int) -> List[int]:
    """Token rows a new fixture keeps (a committed file stays small): every row of a short sequence, else the class token, both
    sides of every 64-key tile edge and the ragged last rows."""
    return list(range(T)) if T <= 64 else sorted({r for r in FULL_SIZE_ROWS if r < T} | {T - 2, T - 1})


def output_keys(fx) -> List[str]:
    return ["image_embeds", "pooler_output", "last_hidden_state"] + [f"hidden_{int(t)}" for t in fx["taps"]]

"""What the case tables and the measurement scripts of the two 16-bit (bf16 / fp16) CLIP towers share: tests/helpers_clip_vision_half.py
and tests/helpers_clip_text_half.py (the rule and its yardsticks), tests/clip_vision_half_child.py and tests/clip_text_half_child.py (the
op-level guard bands).  Those modules import the names from here and re-export them.

The rule: the HIP 16-bit path's distance from the fp64 values must be at most FACTOR x the real
class's own distance when it runs in the same 16-bit format."""
import numpy as np
import torch

FACTOR = 3.0
FORMATS = ("bf16", "fp16")
TORCH_DTYPE = {"bf16": torch.bfloat16, "fp16": torch.float16}
GUARD = 4096                       # sentinel elements in front of and behind every op-level output


def max_one_minus_cos(a: torch.Tensor, b: torch.Tensor) -> float:
    a, b = a.double(), b.double()
    return float((1.0 - (a * b).sum(-1) / (a.norm(dim=-1) * b.norm(dim=-1))).max())


def yardstick(ys, name: str, fmt: str, key: str) -> float:
    """The real class's own distance from fp64 in format ``fmt``: relative L2 of output ``key``, or ``key`` = "cos" for the
    maximum of 1 - cos over the rows of the tower's embeds (``image_embeds`` / ``text_embeds``)."""
    return float(ys[f"{name}/{fmt}/{key}"])


def u16():
    """Unit roundoff of the storage format of the library this process runs."""
    from difashion_amd import _lib
    return 2.0 ** -11 if _lib.storage() == "fp16" else 2.0 ** -8


def _guarded(shape, dtype, sentinel):
    """A tensor of ``shape`` inside a flat buffer with GUARD sentinel elements on either side -> (buffer, view)."""
    n = int(np.prod(shape))
    buf = torch.full((GUARD + n + GUARD,), sentinel, dtype=dtype, device="cuda")
    return buf, buf[GUARD:GUARD + n].view(*shape)


def _bands_untouched(buf, sentinel):
    return bool((buf[:GUARD] == sentinel).all() and (buf[-GUARD:] == sentinel).all())

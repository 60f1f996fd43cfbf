"""The JPEG save / open round trip on the MI355X HIP path.

The reference never scores the images it generates: it writes each with ``img.save("<i>.jpg")`` (inf4eval.py:787-790, PIL's baseline
JPEG at quality 75, 4:2:0) and every metric reads the file back with ``Image.open`` (evaluate_gor.py:207-215, evaluate_fitb.py).
``jpeg_roundtrip`` gives exactly those pixels -- the uint8 RGB array of
``Image.fromarray(x).save(f, "JPEG", quality=..., subsampling=...)`` then ``np.array(Image.open(f).convert("RGB"))`` -- on the device,
without a byte stream: entropy coding is lossless, so the round trip is libjpeg's integer colour conversion, chroma downsampling, DCT
and quantisation and the inverse of each (``dfh_jpeg_roundtrip``, csrc/jpeg.hip, two launches).  The result is what
``CLIPImageProcessor``, ``LPIPS``, ``fid_given_data`` and ``inception_score_given_data`` take.  No PyTorch / CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib
from ._native import grow_buffer

SRC_U8_HWC, SRC_F32_CHW = 0, 1
# subsampling= as PIL spells it -> PIL's number, which the C ABI shares
_SUBSAMPLING = {"4:4:4": 0, "4:2:0": 2, 0: 0, 2: 2}
_NOT_BUILT = {"4:2:2": "4:2:2", 1: "4:2:2", "4:1:1": "4:1:1", "4:4:0": "4:4:0", "keep": "'keep' (only for files that were JPEGs)"}


class _Workspace:
    """The decoded Y / Cb / Cr planes between the two launches: one growable device block, reused across calls."""
    _ws = None


_HOLDER = _Workspace()


def _subsampling_code(subsampling) -> int:
    if subsampling in _NOT_BUILT:
        raise ValueError(f"subsampling={subsampling!r}: {_NOT_BUILT[subsampling]} is not built -- the HIP round trip covers '4:2:0' (PIL's "
                         "default, what the reference's img.save writes) and '4:4:4'")
    if isinstance(subsampling, bool) or subsampling not in _SUBSAMPLING:
        raise ValueError(f"subsampling must be '4:2:0' or '4:4:4' (or PIL's numbers 2 / 0), got {subsampling!r}")
    return _SUBSAMPLING[subsampling]


def jpeg_quant_tables(quality: int = 75) -> Tuple[np.ndarray, np.ndarray]:
    """-> (luminance, chrominance): the 8 x 8 tables libjpeg quantises with at ``quality``, natural order (host only, no GPU)."""
    luma, chroma = (C.c_int * 64)(), (C.c_int * 64)()
    _lib.call("dfh_jpeg_quant_tables", int(quality), luma, chroma)
    return np.array(luma, dtype=np.int32).reshape(8, 8), np.array(chroma, dtype=np.int32).reshape(8, 8)


def jpeg_roundtrip(images: Union[torch.Tensor, Sequence[torch.Tensor]], quality: int = 75, subsampling: Union[str, int] = "4:2:0", *,
                   return_coefficients: bool = False):
    """uint8 ``[B, H, W, 3]`` on the device: the images after PIL's JPEG save and open at ``quality`` / ``subsampling``.

    ``images``: a uint8 ``[B, H, W, 3]`` or fp32 ``[B, 3, H, W]`` (in [-1, 1], quantised as ``difashion.postprocess(.., "pil")`` does, a
    NaN becomes 0) device tensor, or a list of same-size device tensors of one of the two forms without the batch axis.  The source is
    not written.  ``return_coefficients=True`` -> ``(pixels, coefficients)``: the quantised DCT coefficients as int16
    ``[B, blocks, 64]`` in natural order, per image the Y blocks row-major, then Cb, then Cr (real blocks only)."""
    if isinstance(images, (list, tuple)):
        if not images:
            raise ValueError("images holds no image")
        if not all(isinstance(im, torch.Tensor) for im in images):
            raise TypeError("a list of images must hold device tensors (uint8 [H, W, 3] or float32 [3, H, W])")
        if len({tuple(im.shape) for im in images}) != 1:
            raise ValueError("a list of images must hold one size: call once per size")
        images = torch.stack(list(images))
    if not isinstance(images, torch.Tensor):
        raise TypeError(f"images must be a device tensor or a list of device tensors, got {type(images).__name__}")
    code = _subsampling_code(subsampling)
    if isinstance(quality, bool) or int(quality) != quality or not 1 <= int(quality) <= 100:
        raise ValueError(f"quality must be an integer in 1 .. 100, got {quality!r}")
    src = images
    if src.device.type != "cuda":
        raise _lib.DfhError("jpeg_roundtrip runs only on the MI355X HIP path: move the images to 'cuda' (no CPU fallback; on the host "
                            "PIL itself is the round trip)")
    if src.dtype == torch.uint8 and src.dim() == 4 and src.shape[3] == 3:
        kind, (n, h, w) = SRC_U8_HWC, src.shape[:3]
    elif src.dtype == torch.float32 and src.dim() == 4 and src.shape[1] == 3:
        kind, n, (h, w) = SRC_F32_CHW, src.shape[0], src.shape[2:]
    else:
        raise TypeError(f"images must be uint8 [B, H, W, 3] or float32 [B, 3, H, W] in [-1, 1], got {src.dtype} {tuple(src.shape)}")
    n, h, w = int(n), int(h), int(w)
    if n < 1 or h < 1 or w < 1:
        raise ValueError(f"images holds no pixel: shape {tuple(src.shape)}")
    src = src.contiguous()
    if src.data_ptr() % 16:                                           # a slice of a batch: the library wants a 16-byte base
        src = src.clone()
    lib = _lib.raw()
    need = lib.dfh_jpeg_workspace_bytes(n, h, w, code)
    if need == 0:
        raise _lib.DfhError(f"dfh_jpeg_workspace_bytes refused: {_lib.last_error()}")
    ws = grow_buffer(_HOLDER, "_ws", need, src.device)
    out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=src.device)
    coef = None
    if return_coefficients:
        count = lib.dfh_jpeg_coef_count(n, h, w, code)
        coef = torch.empty((n, count // (64 * n), 64), dtype=torch.int16, device=src.device)
    with torch.cuda.device(src.device):
        _lib.call("dfh_jpeg_roundtrip", _lib.ptr(src), kind, n, h, w, int(quality), code, _lib.ptr(out), _lib.ptr(coef), _lib.ptr(ws),
                  ws.numel(), _lib.stream_ptr())
    return (out, coef) if return_coefficients else out

"""``CLIPImageProcessor`` on the MI355X HIP path, behind the transformers call signature.

What the reference's evaluation does to every image in front of ``encode_image`` (Evaluation/extract_hist_embs.py:83-100,
evaluate_gor.py:193-236, evaluate_fitb.py): ``open_clip``'s transform -- PIL bicubic ``Resize(224)``, ``CenterCrop(224)``, ``ToTensor``,
``Normalize`` -- on a DataLoader worker.  Here the images are resized, cropped and normalised on the device in one launch per call
(``dfh_imgproc_run``, csrc/image_processor.hip), bit for bit what ``PIL.Image.resize`` + ``transformers.CLIPImageProcessor`` give:
the resize is PIL's integer arithmetic over coefficient tables the library computes in double on the host, the crop is transformers'
floor-centred one, and ``(v / 255 - mean) / std`` is a 3 x 256 fp32 table built here in that order of operations.

Sources: uint8 ``[B, H, W, 3]`` or fp32 ``[B, 3, H, W]`` in [-1, 1] device tensors (what ``vae.decode`` leaves on the device; quantised as
``difashion.postprocess(.., "pil")`` does, a NaN becomes 0), or a list of PIL images / HWC uint8 arrays, uploaded per size group.
``grid=n`` scores the ``ceil(sqrt n)``-wide white contact sheet of every n consecutive items (``evalio.image_grid``) without building
it.  No PyTorch / CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import json
import os
from typing import Dict, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib

OPENAI_CLIP_MEAN = [0.48145466, 0.4578275, 0.40821073]
OPENAI_CLIP_STD = [0.26862954, 0.26130258, 0.27577711]
CONFIG_NAME = "preprocessor_config.json"
SRC_U8_HWC, SRC_F32_CHW = 0, 1


class BatchFeature(dict):
    """transformers' return object in small: ``["pixel_values"]`` and ``.pixel_values``."""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None


class _Plan:
    """One (input size, sheet) under one config: the library's host-only plan and its coefficient tables on the device."""

    def __init__(self, cfg: _lib.ImgProcConfigC, in_h: int, in_w: int, grid: int, device: torch.device):
        self.handle = C.c_void_p()
        _lib.call("dfh_imgproc_create", C.byref(cfg), in_h, in_w, grid, C.byref(self.handle))
        lib = _lib.raw()
        self.out_h, self.out_w = lib.dfh_imgproc_out_height(self.handle), lib.dfh_imgproc_out_width(self.handle)
        nbytes = lib.dfh_imgproc_table_bytes(self.handle)
        host = torch.empty(nbytes // 4, dtype=torch.int32)
        _lib.call("dfh_imgproc_fill_tables", self.handle, C.c_void_p(host.data_ptr()), nbytes)
        self.tables = host.to(device)

    def __del__(self):
        if getattr(self, "handle", None) and _lib._lib is not None:
            _lib._lib.dfh_imgproc_destroy(self.handle)
            self.handle = None


class CLIPImageProcessor:
    """transformers' ``CLIPImageProcessor`` signature and defaults.  Only the all-True ``do_*`` form is built (the only one the
    evaluation uses); ``resample`` is PIL's numbering, 3 = bicubic or 2 = bilinear."""
    model_input_names = ["pixel_values"]

    def __init__(self, do_resize: bool = True, size: Optional[Dict[str, int]] = None, resample: int = 3, do_center_crop: bool = True,
                 crop_size: Optional[Dict[str, int]] = None, do_rescale: bool = True, rescale_factor: float = 1 / 255,
                 do_normalize: bool = True, image_mean: Optional[Sequence[float]] = None, image_std: Optional[Sequence[float]] = None,
                 do_convert_rgb: bool = True, **unused):
        for name, v in (("do_resize", do_resize), ("do_center_crop", do_center_crop), ("do_rescale", do_rescale),
                        ("do_normalize", do_normalize), ("do_convert_rgb", do_convert_rgb)):
            if not v:
                raise NotImplementedError(f"{name}=False is not built: the HIP path runs resize, centre crop, rescale and normalise as one "
                                          "kernel (the all-True default is the form the evaluation uses)")
        self.do_resize = self.do_center_crop = self.do_rescale = self.do_normalize = self.do_convert_rgb = True
        size = {"shortest_edge": 224} if size is None else ({"shortest_edge": int(size)} if isinstance(size, int) else dict(size))
        if set(size) != {"shortest_edge"}:
            raise ValueError(f"size must be {{'shortest_edge': n}} (CLIP's resize rule), got {size}")
        crop_size = {"height": 224, "width": 224} if crop_size is None else (
            {"height": int(crop_size), "width": int(crop_size)} if isinstance(crop_size, int) else dict(crop_size))
        if set(crop_size) != {"height", "width"}:
            raise ValueError(f"crop_size must be {{'height': h, 'width': w}}, got {crop_size}")
        self.size, self.crop_size = size, crop_size
        self.resample = self._check_resample(resample)
        self.rescale_factor = float(rescale_factor)
        self.image_mean = list(OPENAI_CLIP_MEAN if image_mean is None else image_mean)
        self.image_std = list(OPENAI_CLIP_STD if image_std is None else image_std)
        self._plans: Dict[tuple, _Plan] = {}
        self._lut: Optional[Tuple[tuple, torch.Tensor]] = None

    @staticmethod
    def _check_resample(resample) -> int:
        r = int(resample)
        if r not in (2, 3):
            raise ValueError(f"unsupported resample filter {resample!r}: PIL numbering, 3 (bicubic) or 2 (bilinear)")
        return r

    # ------------------------------------------------------------------ the tables
    def lookup_table(self) -> np.ndarray:
        """3 x 256 fp32, ``(v * rescale_factor - mean) / std`` in fp32 -- ``ToTensor`` + ``Normalize``; 1 / 255 is applied as a division."""
        if len(self.image_mean) != 3 or len(self.image_std) != 3:
            raise ValueError("image_mean / image_std must hold three values (RGB)")
        v = np.arange(256, dtype=np.float32)
        v = v / np.float32(255) if self.rescale_factor == 1 / 255 else v * np.float32(self.rescale_factor)
        return np.stack([(v - np.float32(m)) / np.float32(s) for m, s in zip(self.image_mean, self.image_std)]).astype(np.float32)

    def _device_lut(self, device: torch.device) -> torch.Tensor:
        key = (tuple(self.image_mean), tuple(self.image_std), self.rescale_factor, str(device))
        if self._lut is None or self._lut[0] != key:                 # rebuilt when mean / std change
            self._lut = (key, torch.from_numpy(self.lookup_table()).to(device))
        return self._lut[1]

    def _plan(self, in_h: int, in_w: int, grid: int, device: torch.device, edge: int, crop: Tuple[int, int], resample: int) -> _Plan:
        key = (in_h, in_w, grid, str(device), edge, crop, resample)
        if key not in self._plans:
            self._plans[key] = _Plan(_lib.ImgProcConfigC(edge, crop[0], crop[1], resample), in_h, in_w, grid, device)
        return self._plans[key]

    # ------------------------------------------------------------------ one launch
    def _run(self, src: torch.Tensor, grid: int, edge: int, crop: Tuple[int, int], resample: int, want_pixels: bool, want_u8: bool):
        if src.device.type != "cuda":
            raise _lib.DfhError("CLIPImageProcessor runs only on the MI355X HIP path: move the images to 'cuda' or pass PIL images / "
                                "numpy arrays with device='cuda' (no CPU fallback)")
        if src.dtype == torch.uint8 and src.dim() == 4 and src.shape[3] == 3:
            kind, (n, h, w) = SRC_U8_HWC, src.shape[:3]
        elif src.dtype == torch.float32 and src.dim() == 4 and src.shape[1] == 3:
            kind, n, (h, w) = SRC_F32_CHW, src.shape[0], src.shape[2:]
        else:
            raise TypeError(f"images must be uint8 [B, H, W, 3] or float32 [B, 3, H, W] in [-1, 1], got {src.dtype} {tuple(src.shape)}")
        per = max(int(grid or 0), 1)
        if n < 1 or n % per:
            raise ValueError(f"{n} images do not make whole sheets of grid={grid}")
        B = n // per
        src = src.contiguous()
        if src.data_ptr() % 16:                                       # a slice of a batch: the kernel's wide loads want a 16-byte base
            src = src.clone()
        plan = self._plan(int(h), int(w), int(grid or 0), src.device, edge, crop, resample)
        pixels = torch.empty((B, 3, plan.out_h, plan.out_w), dtype=torch.float32, device=src.device) if want_pixels else None
        u8 = torch.empty((B, plan.out_h, plan.out_w, 3), dtype=torch.uint8, device=src.device) if want_u8 else None
        lut = self._device_lut(src.device) if want_pixels else None
        with torch.cuda.device(src.device):
            _lib.call("dfh_imgproc_run", plan.handle, _lib.ptr(plan.tables), _lib.ptr(lut), _lib.ptr(src), kind, B, _lib.ptr(pixels),
                      _lib.ptr(u8), _lib.stream_ptr())
        return pixels, u8

    @staticmethod
    def _to_rgb_array(img) -> np.ndarray:
        if isinstance(img, np.ndarray):
            if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
                raise TypeError(f"numpy images must be uint8 [H, W, 3], got {img.dtype} {img.shape}")
            return np.ascontiguousarray(img)
        if hasattr(img, "convert"):                                   # PIL: do_convert_rgb
            return np.asarray(img if img.mode == "RGB" else img.convert("RGB"))
        raise TypeError(f"images must be device tensors, PIL images or HWC uint8 numpy arrays, got {type(img).__name__}")

    def _process(self, images, device, grid, edge, crop, resample, want_pixels, want_u8):
        if isinstance(images, torch.Tensor):
            return self._run(images, grid, edge, crop, resample, want_pixels, want_u8)
        if not isinstance(images, (list, tuple)):
            images = [images]
        if not images:
            raise ValueError("images holds no image")
        if all(isinstance(im, torch.Tensor) for im in images):
            return self._run(torch.stack(list(images)), grid, edge, crop, resample, want_pixels, want_u8)
        dev = torch.device("cuda" if device is None else device)
        if dev.type != "cuda":
            raise _lib.DfhError(f"CLIPImageProcessor runs only on the MI355X HIP path, not on {dev} (no CPU fallback)")
        arrays = [self._to_rgb_array(im) for im in images]
        groups: Dict[tuple, list] = {}
        for i, a in enumerate(arrays):
            groups.setdefault(a.shape[:2], []).append(i)
        if grid and len(groups) > 1:
            raise ValueError("grid= needs items of one size (the cells of a sheet)")
        outs = [None, None]
        for idx in groups.values():                                   # one upload and one launch a size group, outputs in input order
            src = torch.from_numpy(np.stack([arrays[i] for i in idx])).to(dev)
            res = self._run(src, grid, edge, crop, resample, want_pixels, want_u8)
            if len(groups) == 1:
                return res
            for k, r in enumerate(res):
                if r is None:
                    continue
                if outs[k] is None:
                    outs[k] = torch.empty((len(arrays),) + tuple(r.shape[1:]), dtype=r.dtype, device=dev)
                elif outs[k].shape[1:] != r.shape[1:]:
                    raise ValueError("images of different sizes resize to different sizes here: pass a crop, or one size a call")
                outs[k][torch.as_tensor(idx, device=dev)] = r
        return tuple(outs)

    # ------------------------------------------------------------------ processor(images=...)
    def __call__(self, images=None, return_tensors: Optional[str] = "pt", device=None, grid: Optional[int] = None, **unused) -> BatchFeature:
        if images is None:
            raise ValueError("You have to specify images")
        if return_tensors not in (None, "pt"):
            raise ValueError(f"return_tensors={return_tensors!r}: the pixel values stay on the device as torch tensors ('pt')")
        crop = (int(self.crop_size["height"]), int(self.crop_size["width"]))
        pixels, _ = self._process(images, device, grid, int(self.size["shortest_edge"]), crop, self.resample, True, False)
        return BatchFeature(pixel_values=pixels)

    preprocess = __call__

    def resize(self, images, size: Union[int, Dict[str, int], None] = None, resample: Optional[int] = None, device=None,
               grid: Optional[int] = None) -> torch.Tensor:
        """The resized uint8 image ``[B, h, w, 3]`` on the device, without crop or lookup (the reference's ``Resize(512, BILINEAR)`` of
        the 291-pixel Polyvore images)."""
        size = self.size if size is None else ({"shortest_edge": int(size)} if isinstance(size, int) else dict(size))
        if set(size) != {"shortest_edge"}:
            raise ValueError(f"size must be an int or {{'shortest_edge': n}}, got {size}")
        resample = self.resample if resample is None else self._check_resample(resample)
        _, u8 = self._process(images, device, grid, int(size["shortest_edge"]), (0, 0), resample, False, True)
        return u8

    def preprocess_uint8(self, images, device=None, grid: Optional[int] = None):
        """-> (pixel_values, the resized and cropped uint8 image the lookup read): tells a resize error from a lookup error."""
        crop = (int(self.crop_size["height"]), int(self.crop_size["width"]))
        return self._process(images, device, grid, int(self.size["shortest_edge"]), crop, self.resample, True, True)

    # ------------------------------------------------------------------ preprocessor_config.json
    def to_dict(self) -> dict:
        return {"crop_size": dict(self.crop_size), "do_center_crop": True, "do_convert_rgb": True, "do_normalize": True, "do_rescale": True,
                "do_resize": True, "image_mean": list(self.image_mean), "image_processor_type": "CLIPImageProcessor",
                "image_std": list(self.image_std), "resample": self.resample, "rescale_factor": self.rescale_factor, "size": dict(self.size)}

    def save_pretrained(self, save_directory: str, **unused):
        os.makedirs(save_directory, exist_ok=True)
        with open(os.path.join(save_directory, CONFIG_NAME), "w") as f:
            f.write(json.dumps(self.to_dict(), indent=2, sort_keys=True) + "\n")

    @classmethod
    def from_pretrained(cls, path: str, subfolder: Optional[str] = None, **unused) -> "CLIPImageProcessor":
        d = os.path.join(path, subfolder) if subfolder else path
        with open(os.path.join(d, CONFIG_NAME)) as f:
            cfg = json.load(f)
        kind = cfg.get("image_processor_type", "CLIPImageProcessor")
        if not kind.startswith("CLIPImageProcessor"):
            raise ValueError(f"{os.path.join(d, CONFIG_NAME)} describes a {kind}, not a CLIPImageProcessor")
        keys = ("do_resize", "size", "resample", "do_center_crop", "crop_size", "do_rescale", "rescale_factor", "do_normalize", "image_mean",
                "image_std", "do_convert_rgb")
        return cls(**{k: cfg[k] for k in keys if cfg.get(k) is not None})

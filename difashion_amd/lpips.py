"""``lpips.LPIPS(net="vgg")`` on the MI355X HIP path, behind the ``lpips`` package's call signature.

What the reference's evaluation runs over every generated / ground-truth pair of a checkpoint (Evaluation/eval_utils.py:473-501,
:769-821; 512 x 512 items in evaluate_fitb.py:179-205, the merged 1024 x 1024 outfit sheet in evaluate_gor.py:217-237): the
ScalingLayer, torchvision's VGG16 features up to ``relu5_3``, and per tap layer the unit-normalised squared difference under the 1 x 1
``lin`` weights, averaged over the pixels and summed over the five layers.

All arithmetic runs in the kernel library (``dfh_lpips_forward``, csrc/lpips.hip) in fp32 on the fp32 matrix instruction, in both
storage builds.  The parameters live under the package's state-dict names (``scaling_layer.*``, ``net.slice{1..5}.{i}.*`` with
torchvision's ``features`` indices, ``lin{k}.model.1.weight``); the conv weights are read through a packed copy that is remade when the
masters change.  Inference only; nothing is downloaded; no PyTorch / CPU fallback.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _lib
from ._native import FrozenDict, PackedModule

SRC_U8_HWC, SRC_F32_CHW = 0, 1
SHIFT = (-.030, -.088, -.188)
SCALE = (.458, .448, .450)
NUM_LAYERS = 5


def im2tensor_table() -> np.ndarray:
    """The reference's ``im2tensor_lpips`` (eval_utils.py:467-470) for every uint8 value: ``float32(float64(v) / 127.5 - 1.0)``."""
    return (np.arange(256, dtype=np.float64) / (255. / 2.) - 1.).astype(np.float32)


class LPIPS(PackedModule):
    family = "lpips"
    _inference_only = ("LPIPS is inference only on this path (the lpips package's eval_mode=True): there is no Dropout "
                       "and no backward kernel; .eval() is the only mode")
    _from_pretrained_kw = dict(pretrained=False)
    _lut = None
    _fp32_rule = "parameters must stay fp32 (the kernels read them in place or pack their own fp32 copy)"

    def __init__(self, pretrained: bool = True, net: str = "vgg", version: str = "0.1", lpips: bool = True, spatial: bool = False,
                 pnet_rand: bool = False, pnet_tune: bool = False, use_dropout: bool = True, model_path: Optional[str] = None,
                 eval_mode: bool = True, verbose: bool = False, max_workspace_bytes: int = 4 << 30, init_seed: Optional[int] = 0, **unused):
        super().__init__()
        if net not in ("vgg", "vgg16"):
            raise NotImplementedError(f"net={net!r}: only VGG16 ('vgg' / 'vgg16') is built on the HIP path; 'alex' and 'squeeze' are out of scope")
        if version != "0.1":
            raise NotImplementedError(f"version={version!r}: only version '0.1' (with the ScalingLayer) is built")
        if not lpips:
            raise NotImplementedError("lpips=False (the unweighted feature average) is not built")
        if spatial:
            raise NotImplementedError("spatial=True (the per-pixel map) is not built: the score is the spatial mean")
        if pnet_tune:
            raise NotImplementedError("pnet_tune=True: this path is inference only, there is no backward kernel")
        if not eval_mode:
            raise NotImplementedError("eval_mode=False: this path is inference only (Dropout is the identity)")
        self._set_workspace_limit(max_workspace_bytes)
        self.config = FrozenDict(net="vgg", version=version)
        table = self.param_table()
        self._names = [n for n, _ in table]
        # seeded stand-ins (the lin weights made non-negative, as the trained ones are); real weights come in through load_state_dict,
        # from_pretrained or load_reference_weights -- pretrained / pnet_rand never fetch anything
        self._build_parameters(table, lambda name: False, init_seed, 0.02, unseeded_zeros=True)
        with torch.no_grad():
            self.scaling_layer.shift.copy_(torch.tensor(SHIFT).view(1, 3, 1, 1))
            self.scaling_layer.scale.copy_(torch.tensor(SCALE).view(1, 3, 1, 1))
            for k in range(NUM_LAYERS):
                getattr(self, f"lin{k}").model._modules["1"].weight.abs_()
        super().train(False)
        self.requires_grad_(False)
        if pretrained and model_path is not None:
            self.load_reference_weights(torch.load(model_path, map_location="cpu", weights_only=True), None)

    # ------------------------------------------------------------------ plumbing
    def _c_config(self) -> _lib.LpipsConfigC:
        return _lib.LpipsConfigC(0)                      # DFH_LPIPS_NET_VGG16

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        """Drops the ``lins.*`` duplicates of ``lin{k}.*`` that the package's module list adds to its state dict."""
        return super().load_state_dict({k: v for k, v in state_dict.items() if not k.startswith("lins.")}, strict=strict, **kw)

    @torch.no_grad()
    def load_reference_weights(self, lin_state_dict, vgg16_state_dict):
        """The two files the package reads: its own ``weights/v0.1/vgg.pth`` (``lin{k}.model.1.weight``; a duplicate ``lins.*`` is
        ignored) and torchvision's ``vgg16`` checkpoint (``features.{i}.{weight,bias}``).  Either may be None (left as it is)."""
        mine = dict(self.named_parameters())
        if lin_state_dict is not None:
            lins = {k: v for k, v in lin_state_dict.items() if not k.startswith("lins.")}
            want = [f"lin{k}.model.1.weight" for k in range(NUM_LAYERS)]
            missing = [k for k in want if k not in lins]
            if missing:
                raise KeyError(f"load_reference_weights: the lin state dict lacks {missing}")
            for k in want:
                mine[k].copy_(lins[k].reshape(mine[k].shape))
        if vgg16_state_dict is not None:
            for name in self._names:
                if not name.startswith("net."):
                    continue
                _, _, idx, leaf = name.split(".")
                key = f"features.{idx}.{leaf}"
                if key not in vgg16_state_dict:
                    raise KeyError(f"load_reference_weights: the vgg16 state dict lacks {key}")
                mine[name].copy_(vgg16_state_dict[key].reshape(mine[name].shape))
        return self

    def pairs_per_call(self, H: int, W: int) -> int:
        """How many pairs one launch sequence takes so that its workspace stays under ``max_workspace_bytes``."""
        self._context()
        need = self._entry("workspace_bytes")
        if need(self._ctx, 1, H, W) == 0:
            raise ValueError(f"images must be between 16 and 8192 pixels a side (four 2 x 2 pools leave the fifth level empty below 16), got {H} x {W}")
        per = need(self._ctx, 2, H, W) - need(self._ctx, 1, H, W)
        n = (self.max_workspace_bytes - (need(self._ctx, 1, H, W) - per)) // per
        if n < 1:
            raise _lib.DfhError(f"one {H} x {W} pair needs a workspace of {need(self._ctx, 1, H, W)} bytes, max_workspace_bytes is "
                                f"{self.max_workspace_bytes}")
        return int(min(n, 32767))

    # ------------------------------------------------------------------ model(in0, in1)
    @torch.no_grad()
    def forward(self, in0: torch.Tensor, in1: torch.Tensor, retPerLayer: bool = False, normalize: bool = False):
        """``[N, 1, 1, 1]`` fp32; with ``retPerLayer`` ``(val, [five [N, 1, 1, 1]])``.  Inputs: fp32 ``[N, 3, H, W]`` in [-1, 1]
        (``normalize=True``: in [0, 1]) or uint8 ``[N, H, W, 3]`` (what ``np.array(pil_image)`` gives; ``im2tensor_lpips`` is applied)."""
        if not isinstance(in0, torch.Tensor) or not isinstance(in1, torch.Tensor):
            raise TypeError("in0 and in1 must be tensors")
        dev = self._require_hip_fp32("LPIPS")
        if in0.shape != in1.shape or in0.dtype != in1.dtype or in0.device != in1.device:
            raise ValueError(f"in0 and in1 must share shape, dtype and device, got {tuple(in0.shape)} {in0.dtype} on {in0.device} and "
                             f"{tuple(in1.shape)} {in1.dtype} on {in1.device}")
        u8 = in0.dtype == torch.uint8 and in0.dim() == 4 and in0.shape[3] == 3
        self._check_images(in0, dev, " or uint8 [N, H, W, 3]", u8)
        if u8:
            kind, (N, H, W) = SRC_U8_HWC, in0.shape[:3]
            if normalize:
                raise ValueError("normalize=True applies to float images in [0, 1]; uint8 images go through im2tensor_lpips")
            if self._lut is None or self._lut.device != dev:
                self._lut = torch.from_numpy(im2tensor_table()).to(dev)
        else:
            kind, N, (H, W) = SRC_F32_CHW, in0.shape[0], in0.shape[2:]
        N, H, W = int(N), int(H), int(W)
        step = self.pairs_per_call(H, W)
        dist = torch.empty((N,), dtype=torch.float32, device=dev)
        layers = torch.empty((N, NUM_LAYERS), dtype=torch.float32, device=dev)
        if N:
            with torch.cuda.device(dev):
                arr, count, packed = self._prepare(dev)
                ws = self._workspace(dev, min(step, N), H, W)
                for i in range(0, N, step):
                    n = min(step, N - i)
                    a, b = self._chunk(in0, i, n), self._chunk(in1, i, n)
                    _lib.call("dfh_lpips_forward", self._ctx, arr, count, _lib.ptr(packed), _lib.ptr(a), _lib.ptr(b), kind,
                              _lib.ptr(self._lut if kind == SRC_U8_HWC else None), int(bool(normalize)), n, H, W, _lib.ptr(dist[i:]),
                              _lib.ptr(layers[i:]), _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
        val = dist.view(N, 1, 1, 1)
        if retPerLayer:
            return val, [layers[:, k].contiguous().view(N, 1, 1, 1) for k in range(NUM_LAYERS)]
        return val


def group_argmin(scores: torch.Tensor) -> torch.Tensor:
    """``torch.argmin(scores, dim=-1)`` of a ``[rows, K]`` fp32 device tensor on the HIP path (a NaN wins, then the lowest index)."""
    if not isinstance(scores, torch.Tensor) or scores.device.type != "cuda":
        raise _lib.DfhError("group_argmin runs only on the MI355X HIP path: move the scores to 'cuda' (no CPU fallback)")
    if scores.dtype != torch.float32 or scores.dim() != 2 or scores.shape[1] < 1:
        raise TypeError(f"scores must be float32 [rows, K >= 1], got {scores.dtype} {tuple(scores.shape)}")
    scores = scores.contiguous()
    pred = torch.empty((scores.shape[0],), dtype=torch.int64, device=scores.device)
    if scores.shape[0]:
        with torch.cuda.device(scores.device):
            _lib.call("dfh_lpips_group_argmin", _lib.ptr(scores), _lib.ptr(pred), scores.shape[0], scores.shape[1], _lib.stream_ptr())
    return pred


__all__ = ["LPIPS", "group_argmin", "im2tensor_table"]

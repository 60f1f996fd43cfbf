"""Inception v3 on the MI355X HIP path, for the first two columns of the reference's tables: ``FIDInceptionV3``
behind pytorch_fid's class (Evaluation/eval_utils.py:137-280) and ``InceptionV3`` behind the reference's fine-tuned classifier (:17-89).

All arithmetic runs in the kernel library (``dfh_incep_forward``, csrc/inception.hip) in fp32 on the fp32 matrix instruction, in both
storage builds.  The parameters live under torchvision's state-dict names (``<layer>.conv.weight``, ``<layer>.bn.{weight, bias,
running_mean, running_var}``, ``fc.*``); the kernels read a packed copy (weights tap-major, BatchNorm folded to scale / shift) that is
remade when the masters change.  Inference only; nothing is downloaded; no PyTorch / CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

from . import _lib
from ._native import FrozenDict, PackedModule

VARIANT_TV, VARIANT_FID = 0, 1
BLOCK_DIMS = (64, 192, 768, 2048)
SIDE = 299


def plan(ctx, n: int, H: int, W: int):
    """The launch plan of ``n`` images of ``H`` x ``W`` as the library computes it (host arithmetic only): a list of ``IncepLaunchC``."""
    count = _lib.call_count("dfh_incep_plan_count", ctx, n, H, W)
    out = []
    for i in range(count):
        e = _lib.IncepLaunchC()
        _lib.call("dfh_incep_plan_entry", ctx, n, H, W, i, C.byref(e))
        out.append(e)
    return out


class _Inception(PackedModule):
    family = "incep"
    _inference_only = ("{name} is inference only on this path (BatchNorm runs on its running statistics, "
                       "there is no backward kernel); .eval() is the only mode")
    _fp32_rule = "parameters must stay fp32 (the kernels pack their own fp32 copy)"
    _dropped = ()                                        # state-dict prefixes of the foreign checkpoint that never run here

    def _init_network(self, init_seed: Optional[int], max_workspace_bytes: int):
        self._set_workspace_limit(max_workspace_bytes)
        table = self.param_table()
        self._names = [n for n, _ in table]
        # seeded stand-ins: He-scaled conv weights, identity BatchNorm statistics; real weights come in through load_state_dict,
        # from_pretrained or load_reference_weights -- nothing is fetched
        self._build_parameters(table, lambda name: name.endswith(".bn.weight"), init_seed, 1.0, unseeded_zeros=True)
        with torch.no_grad():
            for name, p in self.named_parameters():
                if name.endswith(".bn.running_var"):
                    p.fill_(1.0)
                elif name.endswith(".conv.weight"):
                    p.mul_((2.0 / (p.shape[1] * p.shape[2] * p.shape[3])) ** 0.5)
                elif name == "fc.weight":
                    p.mul_(0.02)
        super().train(False)
        self.requires_grad_(False)

    # ------------------------------------------------------------------ plumbing
    def _c_config(self) -> _lib.IncepConfigC:
        c = self.config
        return _lib.IncepConfigC(self.variant, int(c.get("num_classes", 0)), int(self.resize_input), int(self.normalize_input), self._block_mask())

    def _block_mask(self) -> int:
        return 8

    def set_input_flags(self, resize_input: bool, normalize_input: bool):
        """Whether the first kernel resizes to 299 x 299 and applies ``2 x - 1``: part of the native context, which is remade on a change."""
        flags = (bool(resize_input), bool(normalize_input))
        if flags != (self.resize_input, self.normalize_input):
            self.resize_input, self.normalize_input = flags
            self.config.update(resize_input=flags[0], normalize_input=flags[1])
            self._destroy_ctx()
        return self

    def _clean(self, state_dict):
        return {k: v for k, v in state_dict.items() if not k.endswith("num_batches_tracked") and not k.startswith(self._dropped)}

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        """Drops what the foreign checkpoint carries but eval never runs: ``num_batches_tracked``, ``AuxLogits.*`` (and ``fc.*`` for FID)."""
        return super().load_state_dict(self._clean(state_dict), strict=strict, **kw)

    @torch.no_grad()
    def load_reference_weights(self, state_dict):
        """A torchvision ``inception_v3`` / pytorch_fid ``fid_inception_v3`` state dict (or the reference's fine-tuned checkpoint)."""
        sd = self._clean(state_dict)
        mine = dict(self.named_parameters())
        missing = [k for k in self._names if k not in sd]
        if missing:
            raise KeyError(f"load_reference_weights: the state dict lacks {missing[:4]}{' ...' if len(missing) > 4 else ''}")
        for k in self._names:
            mine[k].copy_(sd[k].reshape(mine[k].shape))
        return self

    def images_per_call(self, H: int, W: int) -> int:
        """How many images one launch sequence takes so that its workspace stays under ``max_workspace_bytes``."""
        ctx = self._context()
        need = self._entry("workspace_bytes")
        one = need(ctx, 1, H, W)
        if one == 0:
            raise ValueError(f"images of {H} x {W} are refused: {_lib.last_error()}")
        if one > self.max_workspace_bytes:
            raise _lib.DfhError(f"one {H} x {W} image needs a workspace of {one} bytes, max_workspace_bytes is {self.max_workspace_bytes}")
        lo, hi = 1, 65535                                # the regions are rounded per call: search the largest n that fits
        while lo < hi:
            mid = (lo + hi + 1) // 2
            if need(ctx, mid, H, W) <= self.max_workspace_bytes:
                lo = mid
            else:
                hi = mid - 1
        return lo

    @torch.no_grad()
    def _run(self, x: torch.Tensor, what: str):
        """-> (taps: {block: [N, C]}, probs [N, classes] or None)"""
        if not isinstance(x, torch.Tensor):
            raise TypeError(f"{what}: the images must be a tensor")
        dev = self._require_hip_fp32(what)
        self._check_images(x, dev)
        N, H, W = int(x.shape[0]), int(x.shape[2]), int(x.shape[3])
        mask = self._block_mask()
        taps = {b: torch.empty((N, BLOCK_DIMS[b]), dtype=torch.float32, device=dev) for b in range(4) if mask >> b & 1}
        classes = int(self.config.get("num_classes", 0))
        probs = torch.empty((N, classes), dtype=torch.float32, device=dev) if self.variant == VARIANT_TV else None
        if N:
            step = self.images_per_call(H, W)
            with torch.cuda.device(dev):
                arr, count, packed = self._prepare(dev)
                ws = self._workspace(dev, min(step, N), H, W)
                for i in range(0, N, step):
                    n = min(step, N - i)
                    a = self._chunk(x, i, n)
                    tp = (C.c_void_p * 4)(*[taps[b][i:].data_ptr() if b in taps else 0 for b in range(4)])
                    _lib.call("dfh_incep_forward", self._ctx, arr, count, _lib.ptr(packed), _lib.ptr(a), n, H, W, tp,
                              _lib.ptr(None if probs is None else probs[i:]), _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
        return taps, probs


class FIDInceptionV3(_Inception):
    """pytorch_fid's ``InceptionV3`` with ``fid_inception_v3`` weights.  ``forward(inp)`` takes fp32 ``[N, 3, H, W]`` in [0, 1] and returns
    one ``[N, C, 1, 1]`` per output block, C = 64 / 192 / 768 / 2048.

    Deviation: blocks 0 to 2 come back ALREADY AVERAGED over their pixels (``[N, C, 1, 1]``, not the ``[N, C, h, w]`` map), which is what
    ``get_activations`` does to them next (eval_utils.py:304-305); the map itself is never materialised for the caller.  The walk stops at
    the last needed block."""
    variant = VARIANT_FID
    _dropped = ("AuxLogits.", "fc.")
    DEFAULT_BLOCK_INDEX = 3
    BLOCK_INDEX_BY_DIM = {64: 0, 192: 1, 768: 2, 2048: 3}

    def __init__(self, output_blocks: Sequence[int] = (DEFAULT_BLOCK_INDEX,), resize_input: bool = True, normalize_input: bool = True,
                 requires_grad: bool = False, use_fid_inception: bool = True, max_workspace_bytes: int = 4 << 30, init_seed: Optional[int] = 0):
        super().__init__()
        if requires_grad:
            raise NotImplementedError("requires_grad=True: this path is inference only, there is no backward kernel")
        if not use_fid_inception:
            raise NotImplementedError("use_fid_inception=False: only the FID variant of the feature extractor is built (InceptionV3 is the classifier)")
        blocks = sorted(int(b) for b in output_blocks)
        if not blocks or blocks[0] < 0 or blocks[-1] > 3 or len(set(blocks)) != len(blocks):
            raise ValueError(f"output_blocks must be distinct indices in 0 .. 3, got {tuple(output_blocks)}")
        self.output_blocks = blocks
        self.last_needed_block = blocks[-1]
        self.resize_input, self.normalize_input = bool(resize_input), bool(normalize_input)
        self.config = FrozenDict(output_blocks=blocks, resize_input=self.resize_input, normalize_input=self.normalize_input)
        self._init_network(init_seed, max_workspace_bytes)

    def _block_mask(self) -> int:
        return sum(1 << b for b in self.output_blocks)

    def forward(self, inp: torch.Tensor):
        taps, _ = self._run(inp, "FIDInceptionV3")
        return [taps[b].view(inp.shape[0], BLOCK_DIMS[b], 1, 1) for b in self.output_blocks]


class InceptionV3(_Inception):
    """The reference's classifier (eval_utils.py:17-89): torchvision's ``inception_v3`` with ``transform_input`` and a
    ``num_classes``-wide ``fc``.  ``forward(x)``: softmax probabilities ``[N, num_classes]``; ``feature_extract(x)``: ``[N, 2048]``.  The
    input is fp32 ``[N, 3, 299, 299]`` in [-1, 1] (the caller has resized and normalised, as the reference's loop does); the evaluation
    entry ``inception_score_given_data`` hands over [0, 1] images of any size instead and lets the kernel do both."""
    variant = VARIANT_TV
    _dropped = ("AuxLogits.",)

    def __init__(self, model_path: Optional[str] = None, num_classes: int = 50, max_workspace_bytes: int = 4 << 30, init_seed: Optional[int] = 0,
                 resize_input: bool = False, normalize_input: bool = False, tap_blocks: Sequence[int] = (3,)):
        super().__init__()
        self._tap_blocks = sorted({3, *(int(b) for b in tap_blocks)})      # block 3 feeds the classifier; 0 .. 2 only for pooled_taps()
        if self._tap_blocks[0] < 0 or self._tap_blocks[-1] > 3:
            raise ValueError(f"tap_blocks must be indices in 0 .. 3, got {tuple(tap_blocks)}")
        if not 1 <= int(num_classes) <= 4096:
            raise ValueError(f"num_classes must be in 1 .. 4096, got {num_classes}")
        self.num_classes = int(num_classes)
        self.resize_input, self.normalize_input = bool(resize_input), bool(normalize_input)
        self.config = FrozenDict(num_classes=self.num_classes, resize_input=self.resize_input, normalize_input=self.normalize_input)
        self._init_network(init_seed, max_workspace_bytes)
        if model_path is not None:
            self.load_reference_weights(torch.load(model_path, map_location="cpu", weights_only=True))

    def _block_mask(self) -> int:
        return sum(1 << b for b in self._tap_blocks)

    def pooled_taps(self, x: torch.Tensor):
        """{block: [N, C]} for the constructor's ``tap_blocks``: the block outputs averaged over their pixels."""
        self._check_size(x)
        return self._run(x, "InceptionV3")[0]

    def _check_size(self, x):
        if isinstance(x, torch.Tensor) and x.dim() == 4 and not self.resize_input and tuple(x.shape[2:]) != (SIDE, SIDE):
            raise ValueError(f"InceptionV3 takes 299 x 299 images (resize_input=True resizes in the kernel), got {tuple(x.shape[2:])}")

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        self._check_size(x)
        return self._run(x, "InceptionV3")[1]

    def feature_extract(self, x: torch.Tensor) -> torch.Tensor:
        self._check_size(x)
        return self._run(x, "InceptionV3")[0][3]


__all__ = ["FIDInceptionV3", "InceptionV3", "plan", "BLOCK_DIMS"]

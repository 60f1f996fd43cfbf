"""``CLIPVisionModelWithProjection`` on the MI355X HIP path, behind the transformers call signature.

What the reference's evaluation scripts require of the image side of their OpenCLIP ViT-H/14:
  * ``model.encode_image(images)`` on batches of preprocessed 224 x 224 images -- Evaluation/extract_hist_embs.py:83-100 (history
    embeddings per user), Evaluation/eval_utils.py:91-135 (CLIP score, CLIP image score), :503-535 (personalisation similarity).
This class is that shared feature extractor under the architecture and the state-dict key names of
``transformers.CLIPVisionModelWithProjection`` (``vision_model.*`` with transformers' own ``pre_layrnorm`` spelling,
``visual_projection.weight``); ``open_clip`` checkpoints must be exported under those names first.  Resizing /
normalising the images is ``CLIPImageProcessor`` (image_processor.py, row f7); the metrics computed from the embeddings are row f6
(evalscores.py).

All arithmetic runs in the kernel library.  fp32 by default (``dfh_clipv_encode``, csrc/clip_vision.hip): the fp32 matrix instruction,
in both storage builds, the fp32 ``nn.Parameter``s read in place (no packed copy).  Opt-in, what ``open_clip``'s ``precision="bf16"`` /
``"fp16"`` and transformers' ``torch_dtype=`` / ``.half()`` give: the tower in the process's 16-bit storage format
(``dfh_clipvh_encode``, csrc/clip_vision_half.hip) -- ``torch_dtype=`` at construction or in ``from_pretrained``,
``set_compute_dtype(dtype)``, ``.half()`` / ``.bfloat16()`` / ``.float()`` / ``.to(dtype=...)``.  None of these casts a parameter: the
masters, ``state_dict()`` and checkpoints stay fp32, and the 16-bit weights are a packed copy that is remade whenever a parameter
changes and is never saved.  Every output is an fp32 tensor in both modes.  The switch itself is ``ClipTower``'s (_native.py), shared with the text tower (clip.py).
No PyTorch / CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib
from ._native import ClipTower, TupleOutput


class CLIPVisionModelOutput(TupleOutput):
    """transformers' output object: ``.image_embeds`` / ``[0]``, ``.last_hidden_state`` / ``[1]``, ``.hidden_states``; plus
    ``.pooler_output`` (the post-LayerNorm class token that ``visual_projection`` reads), which the evaluation tests compare too."""
    _fields = ("image_embeds", "last_hidden_state", "hidden_states")

    def __init__(self, image_embeds, last_hidden_state, pooler_output, hidden_states=None):
        self.image_embeds, self.last_hidden_state, self.pooler_output = image_embeds, last_hidden_state, pooler_output
        self.hidden_states = hidden_states


class CLIPVisionModelWithProjection(ClipTower):
    family = "clipv"
    architecture, model_type = "CLIPVisionModelWithProjection", "clip_vision_model"

    def __init__(self, hidden_size: int = 1280, intermediate_size: int = 5120, projection_dim: int = 1024, num_hidden_layers: int = 32,
                 num_attention_heads: int = 16, num_channels: int = 3, image_size: int = 224, patch_size: int = 14,
                 hidden_act: str = "gelu", layer_norm_eps: float = 1e-5, init_seed: Optional[int] = 0, init_std: float = 0.02,
                 torch_dtype: Optional[torch.dtype] = None, **unused):
        super().__init__()
        self._init_tower(init_seed, init_std, "the CLIP vision towers use 'quick_gelu' (OpenAI ViT-L/14) / 'gelu' (OpenCLIP ViT-H/14)",
                         hidden_size=hidden_size, intermediate_size=intermediate_size, projection_dim=projection_dim,
                         num_hidden_layers=num_hidden_layers, num_attention_heads=num_attention_heads, num_channels=num_channels,
                         image_size=image_size, patch_size=patch_size, hidden_act=hidden_act, layer_norm_eps=layer_norm_eps)
        if torch_dtype is not None:
            self.set_compute_dtype(torch_dtype)

    # ------------------------------------------------------------------ compute precision (ClipTower; the parameters are never cast)
    half_family = "clipvh"
    HALF_HEAD_DIMS = (32, 40, 64, 80, 128, 160)          # the head dims dfh_attention's kernels are built for

    def _check_half_config(self) -> None:
        d = self.config["hidden_size"] // self.config["num_attention_heads"]
        if d not in self.HALF_HEAD_DIMS:
            raise _lib.DfhError(f"the 16-bit tower runs on the 16-bit attention kernels, which are built for head dims "
                                f"{', '.join(map(str, self.HALF_HEAD_DIMS))}; this config has head dim {d} (hidden_size "
                                f"{self.config['hidden_size']} / {self.config['num_attention_heads']} heads): keep float32")
        # everything else the walk needs of the config (sizes, the q | k | v launch's column tile) is the plan's to say: host-only work
        ctx = self._make_ctx()
        try:
            _lib.call("dfh_clipvh_plan", ctx, 1, C.byref(_lib.CLIPVHalfPlanC()))
        finally:
            self._entry("destroy")(ctx)

    # ------------------------------------------------------------------ plumbing
    def _c_config(self) -> _lib.CLIPVisionConfigC:
        cfg = self.config
        return _lib.CLIPVisionConfigC(cfg["hidden_size"], cfg["intermediate_size"], cfg["num_hidden_layers"], cfg["num_attention_heads"],
                                      cfg["image_size"], cfg["patch_size"], cfg["num_channels"], cfg["projection_dim"],
                                      self._ACT[cfg["hidden_act"]], cfg["layer_norm_eps"])

    @property
    def num_tokens(self) -> int:
        return 1 + (self.config["image_size"] // self.config["patch_size"]) ** 2

    # ------------------------------------------------------------------ model(pixel_values)
    @torch.no_grad()
    def forward(self, pixel_values: Optional[torch.Tensor] = None, attention_mask=None, output_attentions=None,
                output_hidden_states: Optional[bool] = None, interpolate_pos_encoding: bool = False, return_dict: Optional[bool] = None):
        if pixel_values is None:
            raise ValueError("You have to specify pixel_values")
        if attention_mask is not None or output_attentions:
            raise NotImplementedError("the vision tower attends over all patches: no attention mask, no attention maps on this path")
        if interpolate_pos_encoding:
            raise NotImplementedError("interpolate_pos_encoding=True is not built: resize the images to the model's image_size "
                                      "(the evaluation scripts' preprocessing does)")
        dev = self._require_hip_fp32("CLIPVisionModelWithProjection")
        cfg = self.config
        S, Cn = cfg["image_size"], cfg["num_channels"]
        if pixel_values.dim() != 4 or pixel_values.shape[1] != Cn:
            raise ValueError(f"pixel_values must be [batch, {Cn}, {S}, {S}] (num_channels = {Cn}), got {tuple(pixel_values.shape)}")
        if tuple(pixel_values.shape[2:]) != (S, S):
            raise ValueError(f"Input image size ({pixel_values.shape[2]}*{pixel_values.shape[3]}) doesn't match model ({S}*{S}).")
        half = self._compute_dtype != torch.float32
        if half and pixel_values.dtype not in (torch.float32, self._compute_dtype):
            raise TypeError(f"pixel_values must be float32 or {self._compute_dtype} (the compute dtype), got {pixel_values.dtype}")
        if not half and pixel_values.dtype != torch.float32:
            raise TypeError(f"pixel_values must be float32 (the tower computes in float32; set_compute_dtype / .half() / .bfloat16() "
                            f"select the 16-bit tower), got {pixel_values.dtype}")
        if pixel_values.device != dev:
            raise _lib.DfhError(f"pixel_values live on {pixel_values.device}, the model on {dev}: move them to the model's device "
                                "(no CPU fallback)")
        B = pixel_values.shape[0]
        if B < 1:
            raise ValueError("pixel_values holds no image")
        px = pixel_values.contiguous()
        arr, count = self._prepare_half(dev, B) if half else self._prepare(dev, B)
        D, L, T = cfg["hidden_size"], cfg["num_hidden_layers"], self.num_tokens
        last = torch.empty((B, T, D), dtype=torch.float32, device=dev)
        pooled = torch.empty((B, D), dtype=torch.float32, device=dev)
        embeds = torch.empty((B, cfg["projection_dim"]), dtype=torch.float32, device=dev)
        hs = taps = None
        if output_hidden_states:
            hs = torch.empty((L + 1, B, T, D), dtype=torch.float32, device=dev)
            taps = (C.c_void_p * (L + 1))(*[hs[i].data_ptr() for i in range(L + 1)])
        if half:
            _lib.call("dfh_clipvh_encode", self._ctx, arr, count, _lib.ptr(self._packed), _lib.ptr(px), int(px.dtype != torch.float32), B,
                      _lib.ptr(last), _lib.ptr(pooled), _lib.ptr(embeds), taps, _lib.ptr(self._ws), self._ws.numel(), _lib.stream_ptr())
        else:
            _lib.call("dfh_clipv_encode", self._ctx, arr, count, _lib.ptr(px), B, _lib.ptr(last), _lib.ptr(pooled), _lib.ptr(embeds),
                      taps, _lib.ptr(self._ws), self._ws.numel(), _lib.stream_ptr())
        out = CLIPVisionModelOutput(embeds, last, pooled, tuple(hs[i] for i in range(L + 1)) if hs is not None else None)
        return out if return_dict is None or return_dict else out.to_tuple()

    def encode_image(self, pixel_values: torch.Tensor) -> torch.Tensor:
        """``open_clip``'s name for the projected image embedding (what the reference's evaluation scripts call)."""
        return self.forward(pixel_values).image_embeds

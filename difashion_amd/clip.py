"""``CLIPTextModel`` on the MI355X HIP path, behind the transformers call signature.

What the reference requires of ``self.text_encoder`` (DiFashion/models/difashion.py):
  * ``CLIPTextModel.from_pretrained(path, subfolder="text_encoder", revision=...)`` (:70-72) -- a transformers directory
    (``config.json`` + ``model.safetensors`` / ``pytorch_model.bin``) with ``text_model.*`` keys (transformers 4.32.1, README.md:24);
  * ``text_encoder(input_ids)[0]`` -- last_hidden_state (B, 77, D) for the category prompts of a training batch (:224), the
    empty prompt (:234, :352) and the prompts of the slots a sampling call fills (:340-342); no attention mask is passed;
  * ``text_encoder.dtype`` (:342, :411-425), ``.requires_grad_(False)`` (:107), ``.to(device)``.

All arithmetic runs in the kernel library.  fp32 by default (``dfh_clip_encode``, csrc/clip.hip) on the fp32 matrix instruction: the
prompts are a closed set encoded once per run (``prompts.PromptTable``), so the encoder is built to agree with the fp32 class
to summation-order noise; the fp32 ``nn.Parameter``s are read in place (no packed copy).  Opt-in, what the reference's
``--mixed_precision fp16`` autocast and transformers' ``torch_dtype=`` / ``.half()`` give: the tower in the process's 16-bit storage
format (``dfh_cliph_encode``, csrc/clip_text_half.hip; head dim 64, at most 128 tokens) -- ``torch_dtype=`` at construction or in
``from_pretrained``, ``set_compute_dtype(dtype)``, ``.half()`` / ``.bfloat16()`` / ``.float()`` / ``.to(dtype=...)`` (``ClipTower``).
None of these casts a parameter: masters, ``state_dict()`` and checkpoints stay fp32, the 16-bit weights are a packed copy that is
remade whenever a parameter changes and is never saved, and every output is an fp32 tensor in both modes.  No PyTorch / CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib
from ._native import ClipTower, TupleOutput, require_params_on


class BaseModelOutputWithPooling(TupleOutput):
    """transformers' output object as far as the reference (and ``output_hidden_states=True`` debugging) uses it: ``[0]`` /
    ``.last_hidden_state``, ``[1]`` / ``.pooler_output``, ``.hidden_states``."""
    _fields = ("last_hidden_state", "pooler_output", "hidden_states")

    def __init__(self, last_hidden_state, pooler_output, hidden_states=None):
        self.last_hidden_state, self.pooler_output, self.hidden_states = last_hidden_state, pooler_output, hidden_states


class CLIPTextModel(ClipTower):
    family = "clip"
    architecture, model_type = "CLIPTextModel", "clip_text_model"

    def __init__(self, vocab_size: int = 49408, hidden_size: int = 768, intermediate_size: int = 3072, num_hidden_layers: int = 12,
                 num_attention_heads: int = 12, max_position_embeddings: int = 77, hidden_act: str = "quick_gelu",
                 layer_norm_eps: float = 1e-5, eos_token_id: int = 2, bos_token_id: int = 49406, pad_token_id: int = 1,
                 init_seed: Optional[int] = 0, init_std: float = 0.02, torch_dtype: Optional[torch.dtype] = None, **unused):
        super().__init__()
        self._init_tower(init_seed, init_std, "the CLIP text towers of SD-1.5 / SD-2 use 'quick_gelu' / 'gelu'",
                         vocab_size=vocab_size, hidden_size=hidden_size, intermediate_size=intermediate_size,
                         num_hidden_layers=num_hidden_layers, num_attention_heads=num_attention_heads,
                         max_position_embeddings=max_position_embeddings, hidden_act=hidden_act, layer_norm_eps=layer_norm_eps,
                         eos_token_id=eos_token_id, bos_token_id=bos_token_id, pad_token_id=pad_token_id)
        if torch_dtype is not None:
            self.set_compute_dtype(torch_dtype)

    # ------------------------------------------------------------------ compute precision (ClipTower; the parameters are never cast)
    half_family = "cliph"

    def _check_half_config(self) -> None:
        """Head dim 64, sizes that are multiples of 8: the plan's to say, at the longest sequence the config allows (host-only work)."""
        ctx = self._make_ctx()
        try:
            _lib.call("dfh_cliph_plan", ctx, 1, min(int(self.config["max_position_embeddings"]), 128), C.byref(_lib.CLIPTHalfPlanC()))
        finally:
            self._entry("destroy")(ctx)

    # ------------------------------------------------------------------ plumbing
    def _c_config(self) -> _lib.CLIPConfigC:
        cfg = self.config
        return _lib.CLIPConfigC(cfg["vocab_size"], cfg["hidden_size"], cfg["intermediate_size"], cfg["num_hidden_layers"],
                                cfg["num_attention_heads"], cfg["max_position_embeddings"], self._ACT[cfg["hidden_act"]], cfg["layer_norm_eps"])

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        """Accepts the 4.32.1 layout (``text_model.*``, what published checkpoints hold), the flattened layout of newer transformers
        releases, and drops the ``position_ids`` buffer old checkpoints carry."""
        sd = {k if k.startswith("text_model.") else "text_model." + k: v for k, v in state_dict.items()}
        return super().load_state_dict(sd, strict=strict, **kw)

    # ------------------------------------------------------------------ text_encoder(input_ids)
    def _ids_on_device(self, what: str, input_ids, attention_mask, position_ids, output_attentions):
        """The checks of ``forward`` that both text classes share -> (device, ids [B, T] int64 on it, B, T)."""
        if input_ids is None:
            raise ValueError("You have to specify input_ids")
        if attention_mask is not None or position_ids is not None or output_attentions:
            raise NotImplementedError("the reference calls text_encoder(input_ids) only (difashion.py:224,340): no padding mask, "
                                      "default positions, no attention maps on this path")
        dev = self._require_hip_fp32(what)
        cfg = self.config
        T = tuple(input_ids.shape)[-1]
        if T > cfg["max_position_embeddings"]:
            raise ValueError(f"Sequence length must be less than max_position_embeddings (got `sequence length`: {T} and "
                             f"max_position_embeddings: {cfg['max_position_embeddings']}")
        # nn.Embedding raises on out-of-range ids too.  Checked where the ids LIVE: tokenizer output is a CPU tensor (no device sync then);
        # ids that already sit on the GPU cost one sync, and the encoder runs once per run (PromptTable.build)
        lo, hi = int(input_ids.min()), int(input_ids.max())
        ids = input_ids.reshape(-1, T).to(device=dev, dtype=torch.int64).contiguous()
        if lo < 0 or hi >= cfg["vocab_size"]:
            raise IndexError(f"input_ids out of range [0, {cfg['vocab_size']}): min {lo}, max {hi}")
        return dev, ids, ids.shape[0], T

    @torch.no_grad()
    def forward(self, input_ids: Optional[torch.Tensor] = None, attention_mask=None, position_ids=None, output_attentions=None,
                output_hidden_states: Optional[bool] = None, return_dict: Optional[bool] = None):
        dev, ids, B, T = self._ids_on_device("CLIPTextModel", input_ids, attention_mask, position_ids, output_attentions)
        cfg = self.config
        half = self._compute_dtype != torch.float32
        arr, count = self._prepare_half(dev, B, T) if half else self._prepare(dev, B, T)
        D, L = cfg["hidden_size"], cfg["num_hidden_layers"]
        last = torch.empty((B, T, D), dtype=torch.float32, device=dev)
        pooled = torch.empty((B, D), dtype=torch.float32, device=dev)
        hs = torch.empty((L + 1, B, T, D), dtype=torch.float32, device=dev) if output_hidden_states else None
        tail = (_lib.ptr(ids), _lib.ptr(last), _lib.ptr(pooled), int(cfg["eos_token_id"]), _lib.ptr(hs), _lib.ptr(self._ws), self._ws.numel(), B, T,
                _lib.stream_ptr())
        if half:
            _lib.call("dfh_cliph_encode", self._ctx, arr, count, _lib.ptr(self._packed), *tail)
        else:
            _lib.call("dfh_clip_encode", self._ctx, arr, count, *tail)
        out = BaseModelOutputWithPooling(last, pooled, tuple(hs[i] for i in range(L + 1)) if hs is not None else None)
        return out if return_dict is None or return_dict else out.to_tuple()


class CLIPTextModelOutput(TupleOutput):
    """transformers' output object: ``.text_embeds`` / ``[0]``, ``.last_hidden_state`` / ``[1]``, ``.hidden_states``; plus
    ``.pooler_output`` (the final-LayerNorm row at the eos position that ``text_projection`` reads)."""
    _fields = ("text_embeds", "last_hidden_state", "hidden_states")

    def __init__(self, text_embeds, last_hidden_state, pooler_output, hidden_states=None):
        self.text_embeds, self.last_hidden_state, self.pooler_output = text_embeds, last_hidden_state, pooler_output
        self.hidden_states = hidden_states


class CLIPTextModelWithProjection(CLIPTextModel):
    """The text side of the evaluation's OpenCLIP ViT-H/14 (``encode_text``, Evaluation/eval_utils.py:101-114) under
    the architecture and key names of ``transformers.CLIPTextModelWithProjection``: ``CLIPTextModel``'s tower, parameter table and
    native object plus ``text_projection.weight`` (``dfh_clip_text_embeds``, csrc/clip.hip: final LayerNorm and projection on the pooled
    rows only)."""
    architecture = "CLIPTextModelWithProjection"

    def __init__(self, projection_dim: int = 1024, init_seed: Optional[int] = 0, init_std: float = 0.02, **text_config):
        # text_config may carry torch_dtype=: CLIPTextModel's constructor selects the mode (text_projection is read in fp32 either way)
        super().__init__(init_seed=init_seed, init_std=init_std, **text_config)
        if projection_dim < 1:
            raise ValueError(f"projection_dim must be positive, got {projection_dim}")
        self.register_to_config(projection_dim=projection_dim)
        # not in the native table (dfh_clip_num_params is CLIPTextModel's): a parameter of its own, handed over as a separate pointer
        self._build_parameters([("text_projection.weight", (projection_dim, self.config["hidden_size"]))], lambda name: False,
                               None if init_seed is None else init_seed + 1, init_std, unseeded_zeros=True)

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        """``text_model.*`` + ``text_projection.weight``; the flattened tower keys of newer transformers releases are accepted too."""
        own = lambda k: k.startswith(("text_model.", "text_projection."))
        return ClipTower.load_state_dict(self, {k if own(k) else "text_model." + k: v for k, v in state_dict.items()}, strict=strict, **kw)

    @torch.no_grad()
    def forward(self, input_ids: Optional[torch.Tensor] = None, attention_mask=None, position_ids=None, output_attentions=None,
                output_hidden_states: Optional[bool] = None, return_dict: Optional[bool] = None):
        dev, ids, B, T = self._ids_on_device("CLIPTextModelWithProjection", input_ids, attention_mask, position_ids, output_attentions)
        cfg = self.config
        D, L, Pd = cfg["hidden_size"], cfg["num_hidden_layers"], cfg["projection_dim"]
        embeds = torch.empty((B, Pd), dtype=torch.float32, device=dev)
        last = torch.empty((B, T, D), dtype=torch.float32, device=dev)
        pooled = torch.empty((B, D), dtype=torch.float32, device=dev)
        hs = torch.empty((L + 1, B, T, D), dtype=torch.float32, device=dev) if output_hidden_states else None
        self._text_embeds(dev, ids, B, T, embeds, pooled, last, hs)
        out = CLIPTextModelOutput(embeds, last, pooled, tuple(hs[i] for i in range(L + 1)) if hs is not None else None)
        return out if return_dict is None or return_dict else out.to_tuple()

    @torch.no_grad()
    def encode_text(self, input_ids: torch.Tensor) -> torch.Tensor:
        """``open_clip``'s name for the projected text embedding (what ``CLIPScore.calculate_clip_score`` calls): only the pooled rows
        go through the final LayerNorm, ``last_hidden_state`` is not formed."""
        dev, ids, B, T = self._ids_on_device("CLIPTextModelWithProjection", input_ids, None, None, None)
        embeds = torch.empty((B, self.config["projection_dim"]), dtype=torch.float32, device=dev)
        self._text_embeds(dev, ids, B, T, embeds, None, None, None)
        return embeds

    def _text_embeds(self, dev, ids, B, T, embeds, pooled, last, hs):
        """One ``dfh_clip_text_embeds`` / ``dfh_cliph_text_embeds`` call of the selected tower; ``pooled`` / ``last`` / ``hs`` may be None."""
        half = self._compute_dtype != torch.float32
        arr, count = self._prepare_half(dev, B, T) if half else self._prepare(dev, B, T)
        proj = self.text_projection.weight
        require_params_on(dev, [proj])
        tail = (_lib.ptr(proj), self.config["projection_dim"], _lib.ptr(ids), _lib.ptr(embeds), _lib.ptr(pooled), _lib.ptr(last),
                int(self.config["eos_token_id"]), _lib.ptr(hs), _lib.ptr(self._ws), self._ws.numel(), B, T, _lib.stream_ptr())
        if half:
            _lib.call("dfh_cliph_text_embeds", self._ctx, arr, count, _lib.ptr(self._packed), *tail)
        else:
            _lib.call("dfh_clip_text_embeds", self._ctx, arr, count, *tail)

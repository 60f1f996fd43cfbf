"""What the native-backed model wrappers (unet.py, vae.py, clip.py, clip_vision.py, lpips.py, inception.py; the checkpoint part also
mutual.py) share: the Python counterpart of csrc/walk_common.h, of csrc/clip_tower.h for the two CLIP towers (``ClipTower``,
``TupleOutput``), and the base of the models that run on a packed copy of their parameters (``PackedModule``: LPIPS, Inception v3).

``NativeModule`` drives one family of C entry points (``dfh_<family>_create / _destroy / _num_params / _param_name / _param_ndim /
_param_dim``): handle lifecycle, the parameter tree built from the C table, the table-ordered parameter list, the pack signature and
the device / dtype guard.  A subclass supplies ``family``, ``_c_config()`` and what is its own (DESIGN.md section 3 lists which
differences between the wrappers are deliberate).  The free functions are the checkpoint-directory halves every wrapper uses.
"""
from __future__ import annotations

import ctypes as C
import json
import os
from typing import Callable, Optional

import torch
import torch.nn as nn

from . import _lib


class FrozenDict(dict):
    """diffusers-style config: attribute and mapping access."""

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError as e:
            raise AttributeError(k) from e


class _Node(nn.Module):
    """Bare container used to rebuild the diffusers module tree from dotted parameter names."""


def pack_signature(params):
    """What a packed copy of ``params`` was made from: storage and version of every tensor, and the epoch the fused optimizer bumps
    when a native kernel rewrites master weights in place."""
    return tuple((p.data_ptr(), p._version) for p in params) + (_lib.weight_epoch(),)


def save_checkpoint(module: nn.Module, save_directory: str, extra: dict, weights_name: Optional[str] = None):
    """``config.json`` (the module's config, then ``extra``) + the state dict as one safetensors file."""
    from safetensors.torch import save_file
    os.makedirs(save_directory, exist_ok=True)
    cfg = dict(module.config)
    cfg.update(extra)
    with open(os.path.join(save_directory, module.config_name), "w") as f:
        json.dump(cfg, f, indent=2)
    save_file({k: v.detach().cpu().contiguous() for k, v in module.state_dict().items()},
              os.path.join(save_directory, weights_name or module.weights_name))


def read_checkpoint_config(cls, path: str, subfolder: Optional[str] = None):
    """(checkpoint directory, its config without the ``_``-prefixed bookkeeping keys)."""
    d = os.path.join(path, subfolder) if subfolder else path
    with open(os.path.join(d, cls.config_name)) as f:
        cfg = json.load(f)
    return d, {k: v for k, v in cfg.items() if not k.startswith("_")}


def grow_buffer(holder, attr: str, nbytes: int, dev: torch.device) -> torch.Tensor:
    """The uint8 device block ``holder.<attr>``, reused unless it is missing, on another device or smaller than ``nbytes``."""
    buf = getattr(holder, attr)
    if buf is None or buf.device != dev or buf.numel() < nbytes:
        setattr(holder, attr, None)                      # release the old block before asking for the larger one
        buf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        setattr(holder, attr, buf)
    return buf


def current_packed_copy(module, fam: str, plist, arr, dev: torch.device) -> torch.Tensor:
    """The device block ``module._packed`` holding a packed copy of ``plist`` that is current: ``<fam>_pack`` runs when the block is new
    (it holds no copy yet) or when a parameter was written, replaced or moved since the last pack (the pack signature)."""
    old = module._packed
    packed = grow_buffer(module, "_packed", getattr(_lib.raw(), fam + "_packed_bytes")(module._ctx), dev)
    if packed is not old:
        module._packed_sig = None
    sig = pack_signature(plist)
    if sig != module._packed_sig:
        _lib.call(fam + "_pack", module._ctx, arr, len(plist), _lib.ptr(packed), _lib.stream_ptr())
        module._packed_sig = sig
    return packed


def require_params_on(dev: torch.device, params) -> None:
    """The kernels read the parameters in place through raw pointers."""
    if any(p.device != dev or not p.is_contiguous() for p in params):
        raise _lib.DfhError("all parameters must be contiguous and on one device")


def require_hip_fp32(what: str, params, fp32_rule: str) -> torch.device:
    """The device of ``params``' first tensor, or a refusal: it is not on the GPU, or one of ``params`` is not fp32."""
    dev = params[0].device
    if dev.type != "cuda":
        raise _lib.DfhError(f"{what} runs only on the MI355X HIP path: move it to 'cuda' (no CPU fallback)")
    if any(p.dtype != torch.float32 for p in params):
        raise _lib.DfhError(fp32_rule)
    return dev


class NativeModule(nn.Module):
    family: str = ""                     # entry-point prefix: dfh_<family>_*
    config_name = "config.json"
    weights_name = "diffusion_pytorch_model.safetensors"
    _fp32_rule = "master parameters must stay fp32 (the kernels pack their own bf16 copies)"
    _ctx = None
    _names = None
    _packed_sig = None

    # ------------------------------------------------------------------ native handle
    def _c_config(self):
        raise NotImplementedError

    @classmethod
    def _entry(cls, name: str):
        return getattr(_lib.raw(), f"dfh_{cls.family}_{name}")

    def _make_ctx(self):
        c = self._c_config()
        h = C.c_void_p()
        _lib.call(f"dfh_{self.family}_create", C.byref(c), C.byref(h))
        return h

    @classmethod
    def _table(cls, ctx):
        name, ndim, dim = cls._entry("param_name"), cls._entry("param_ndim"), cls._entry("param_dim")
        return [(name(ctx, i).decode(), tuple(dim(ctx, i, d) for d in range(ndim(ctx, i)))) for i in range(cls._entry("num_params")(ctx))]

    def param_table(self):
        """[(checkpoint key, shape)] as the native library enumerates them."""
        ctx = self._make_ctx()
        try:
            return self._table(ctx)
        finally:
            self._entry("destroy")(ctx)

    def _destroy_ctx(self):
        if self._ctx is not None:
            self._entry("destroy")(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self._destroy_ctx()
        except Exception:
            pass

    # ------------------------------------------------------------------ parameters
    def _build_parameters(self, table, is_norm: Callable[[str], bool], init_seed: Optional[int], init_std: float,
                          unseeded_zeros: bool = False):
        """The parameter tree straight from the C table (single source of truth for names and shapes): ``_Node`` containers down
        the dotted name; an entry whose module already holds the parameter (the U-Net's real ``conv_in``) is filled in place.
        Non-norm weights are one ``randn(shape) * init_std`` each, in table order, from a CPU generator that is seeded only when
        ``init_seed`` is given; without a seed they are zeros if ``unseeded_zeros`` (a checkpoint follows).  Norm weights are ones,
        everything else zeros."""
        g = torch.Generator(device="cpu")
        if init_seed is not None:
            g.manual_seed(init_seed)
        for name, shape in table:
            if not name.endswith(".weight"):
                t = torch.zeros(shape)
            elif is_norm(name):
                t = torch.ones(shape)
            elif init_seed is None and unseeded_zeros:
                t = torch.zeros(shape)
            else:
                t = torch.randn(shape, generator=g) * init_std
            *path, leaf = name.split(".")
            m = self
            for p in path:
                if p not in m._modules:
                    m.add_module(p, _Node())
                m = m._modules[p]
            if leaf in m._parameters:
                m._parameters[leaf].data.copy_(t)
            else:
                m.register_parameter(leaf, nn.Parameter(t))

    def _params_by_name(self):
        return dict(self.named_parameters())

    def _plist(self):
        """The parameters in table order.  Resolved by name on every call: modules get replaced (the pipeline swaps the U-Net's
        ``conv_in``), and a cached list would hand the kernels a dead tensor."""
        named = self._params_by_name()
        return [named[n] for n in self._names]

    _signature = staticmethod(pack_signature)

    @staticmethod
    def _pointers(plist):
        return (C.c_void_p * len(plist))(*[p.data_ptr() for p in plist])

    def _pack_with(self, entry_name: str, force: bool = False):
        """Run pack entry point ``entry_name`` over the master parameters unless the packed copy is still current."""
        plist = self._plist()
        sig = self._signature(plist)
        if not force and sig == self._packed_sig:
            return
        _lib.call(entry_name, self._ctx, self._pointers(plist), len(plist), _lib.stream_ptr())
        self._packed_sig = sig

    # ------------------------------------------------------------------ plumbing
    def register_to_config(self, **kwargs):
        self.config.update(kwargs)

    @property
    def device(self) -> torch.device:
        return next(self.parameters()).device

    @property
    def dtype(self) -> torch.dtype:
        return next(self.parameters()).dtype

    def _require_hip_fp32(self, what: str) -> torch.device:
        return require_hip_fp32(what, [next(self.parameters())], self._fp32_rule)


class TupleOutput:
    """transformers-style output object: attributes, and the tuple protocol over those of ``_fields`` that are not None."""
    _fields = ()

    def to_tuple(self):
        return tuple(v for v in (getattr(self, f) for f in self._fields) if v is not None)

    def __getitem__(self, i):
        return self.to_tuple()[i]

    def __iter__(self):
        return iter(self.to_tuple())

    def __len__(self):
        return len(self.to_tuple())


class ClipTower(NativeModule):
    """What CLIPTextModel and CLIPVisionModelWithProjection share: fp32 masters read in place (no arenas, no pack step), one workspace
    block, the transformers checkpoint directory, and the opt-in 16-bit compute mode (``torch_dtype=`` / ``set_compute_dtype`` /
    ``.half()`` / ``.bfloat16()`` over a packed copy).  A subclass supplies ``family``, ``half_family``, ``architecture``, ``model_type``,
    ``_c_config()`` and ``_check_half_config()``."""
    weights_name = "model.safetensors"
    _fp32_rule = "parameters must stay fp32 (the kernels read them in place)"
    _ACT = {"quick_gelu": 1, "gelu": 2}
    architecture = model_type = ""
    _ws = None

    def _init_tower(self, init_seed: Optional[int], init_std: float, act_hint: str, **config):
        """``config`` in the key order of ``config.json``; ``act_hint``: which activations this tower's checkpoints use."""
        if config["hidden_act"] not in self._ACT:
            raise ValueError(f"hidden_act {config['hidden_act']!r}: {act_hint}")
        self.config = FrozenDict(**config)
        table = self.param_table()
        self._names = [n for n, _ in table]             # no bind / pack step that would fill them later: the masters are read in place
        # "norm", not "layer_norm": transformers spells the vision tower's first LayerNorm pre_layrnorm
        self._build_parameters(table, lambda name: "norm" in name.split(".")[-2], init_seed, init_std, unseeded_zeros=True)

    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        """Drops the ``position_ids`` buffer that checkpoints written by older transformers releases carry."""
        return super().load_state_dict({k: v for k, v in state_dict.items() if not k.endswith("position_ids")}, strict=strict, **kw)

    def _prepare(self, dev: torch.device, *batch_args):
        """Context, a workspace of ``dfh_<family>_workspace_bytes(ctx, *batch_args)`` on ``dev`` and the checked parameters:
        (pointer array, count) for the encode call."""
        if self._ctx is None:
            self._ctx = self._make_ctx()
        grow_buffer(self, "_ws", self._entry("workspace_bytes")(self._ctx, *batch_args), dev)
        plist = self._plist()
        require_params_on(dev, plist)
        return self._pointers(plist), len(plist)

    # ------------------------------------------------------------------ compute precision (the parameters are never cast)
    # A tower computes in float32 (the default walk, dfh_<family>_*) or, opt-in, in the process's 16-bit storage format (the walk of
    # dfh_<half_family>_* over a packed 16-bit copy of the weights).  The masters, state_dict() and checkpoints stay fp32 either way.
    half_family: str = ""                # entry-point prefix of the 16-bit walk: dfh_<half_family>_plan / _packed_bytes / _pack / ...
    _compute_dtype = torch.float32
    _packed = None

    @property
    def compute_dtype(self) -> torch.dtype:
        """``torch.float32`` (the default tower) or the process's 16-bit storage dtype.  ``.dtype`` stays the parameters' float32."""
        return self._compute_dtype

    def _check_half_config(self) -> None:
        """Refuse a config the 16-bit walk cannot run (host-only work: the plan of the 16-bit family says)."""
        raise NotImplementedError

    def set_compute_dtype(self, dtype):
        """Select the tower ``forward`` runs: ``torch.float32``, or the 16-bit storage format of this process (``torch.bfloat16`` under
        the default library, ``torch.float16`` under ``DFH_STORAGE=fp16``)."""
        if isinstance(dtype, str):
            dtype = getattr(torch, dtype, dtype)
        if not isinstance(dtype, torch.dtype) or not dtype.is_floating_point:
            raise TypeError(f"set_compute_dtype: a floating torch.dtype is expected, got {dtype!r}")
        if dtype == torch.float32:
            self._compute_dtype = torch.float32          # the packed copy stays: its signature says whether it is still current
            return self
        if dtype not in (torch.float16, torch.bfloat16):
            raise _lib.DfhError(f"{self.architecture} computes in float32 or in {_lib.storage_dtype()}, not in {dtype}; the "
                                "parameters stay fp32 either way")
        if dtype != _lib.storage_dtype():
            raise _lib.DfhError(f"{dtype} is not this process's 16-bit format: the {_lib.storage()}-storage kernel library is selected, and "
                                f"the format is a property of the process (DFH_STORAGE / set_storage() choose it before first use), so the "
                                f"tower computes in float32 or {_lib.storage_dtype()} here.  Whatever the mode, the parameters stay fp32 "
                                "(the 16-bit weights are a packed copy)")
        self._check_half_config()
        self._compute_dtype = dtype
        return self

    def half(self):
        return self.set_compute_dtype(torch.float16)

    def bfloat16(self):
        return self.set_compute_dtype(torch.bfloat16)

    def float(self):
        return self.set_compute_dtype(torch.float32)

    def double(self):
        return self.set_compute_dtype(torch.float64)

    def to(self, *args, **kwargs):
        """``nn.Module.to`` whose dtype part selects the compute precision instead of casting the parameters."""
        device, dtype, non_blocking, _ = torch._C._nn._parse_to(*args, **kwargs)
        if dtype is not None:
            self.set_compute_dtype(dtype)
        return super().to(device, non_blocking=non_blocking) if device is not None else self

    def _prepare_half(self, dev: torch.device, *batch_args):
        """``_prepare`` of the 16-bit tower: its workspace, and a packed 16-bit copy of the weights that is current -- remade when a
        parameter was written, replaced or moved since the last pack (the pack signature), never saved."""
        if self._ctx is None:
            self._ctx = self._make_ctx()
        fam = f"dfh_{self.half_family}"
        need = getattr(_lib.raw(), fam + "_workspace_bytes")(self._ctx, *batch_args)
        if need == 0:
            raise _lib.DfhError(f"{fam}_workspace_bytes refused: {_lib.last_error()}")
        grow_buffer(self, "_ws", need, dev)
        plist = self._plist()
        require_params_on(dev, plist)
        arr = self._pointers(plist)
        current_packed_copy(self, fam, plist, arr, dev)
        return arr, len(plist)

    # ------------------------------------------------------------------ checkpoints (transformers directory layout)
    def save_pretrained(self, save_directory: str, **unused):
        save_checkpoint(self, save_directory, dict(architectures=[self.architecture], model_type=self.model_type))

    @classmethod
    def from_pretrained(cls, path: str, subfolder: Optional[str] = None, variant: Optional[str] = None, revision=None,
                        torch_dtype: Optional[torch.dtype] = None, **unused):
        """Only the caller's ``torch_dtype=`` selects the 16-bit tower.  The ``torch_dtype`` / ``dtype`` key that transformers writes into
        ``config.json`` records the dtype of the saved weights; as in transformers it does not choose the precision of the model."""
        from ._ckpt import TRANSFORMERS_STEMS, load_weights
        d, cfg = read_checkpoint_config(cls, path, subfolder)
        for key in ("torch_dtype", "dtype"):
            cfg.pop(key, None)
        model = cls(init_seed=None, **cfg)
        model.load_state_dict(load_weights(d, variant, TRANSFORMERS_STEMS))
        return model if torch_dtype is None else model.set_compute_dtype(torch_dtype)


class PackedModule(NativeModule):
    """What the inference-only models that run on a packed copy of their parameters share (LPIPS, the two Inception variants): the
    growable blocks ``_ws`` (the workspace of one call) and ``_packed`` (held across calls), ``_prepare``, the ``max_workspace_bytes``
    limit, the refusal to train, the checkpoint directory and the checks of an image batch.  A subclass supplies ``family``,
    ``_c_config()``, ``_inference_only`` and, where its constructor needs them, ``_from_pretrained_kw``."""
    weights_name = "model.safetensors"
    _inference_only = ""                 # the sentence train(True) is refused with; {name}: the class
    _from_pretrained_kw: dict = {}       # what from_pretrained passes the constructor besides init_seed=None and the saved config
    _ws = _packed = None

    def _set_workspace_limit(self, max_workspace_bytes: int):
        if max_workspace_bytes < 1:
            raise ValueError(f"max_workspace_bytes must be positive, got {max_workspace_bytes}")
        self.max_workspace_bytes = int(max_workspace_bytes)

    def train(self, mode: bool = True):
        if mode:
            raise NotImplementedError(self._inference_only.format(name=type(self).__name__))
        return super().train(False)

    def save_pretrained(self, save_directory: str, **unused):
        save_checkpoint(self, save_directory, dict(architectures=[type(self).__name__]))

    @classmethod
    def from_pretrained(cls, path: str, subfolder: Optional[str] = None, variant: Optional[str] = None, **kw):
        from ._ckpt import load_weights
        d, cfg = read_checkpoint_config(cls, path, subfolder)
        cfg.pop("architectures", None)
        model = cls(init_seed=None, **cls._from_pretrained_kw, **cfg, **kw)
        model.load_state_dict(load_weights(d, variant, ("model",)))
        return model

    def _context(self):
        if self._ctx is None:
            self._ctx = self._make_ctx()
        return self._ctx

    def _prepare(self, dev: torch.device):
        """Context, checked parameters and a current packed copy -> (pointer array, count, packed)."""
        self._context()
        plist = self._plist()
        require_params_on(dev, plist)
        arr = self._pointers(plist)
        return arr, len(plist), current_packed_copy(self, f"dfh_{self.family}", plist, arr, dev)

    def _workspace(self, dev: torch.device, *batch_args) -> torch.Tensor:
        """``_ws`` grown to ``dfh_<family>_workspace_bytes(ctx, *batch_args)``."""
        return grow_buffer(self, "_ws", self._entry("workspace_bytes")(self._ctx, *batch_args), dev)

    @staticmethod
    def _chunk(x: torch.Tensor, i: int, n: int) -> torch.Tensor:
        """Rows ``i .. i + n`` of a batch as the kernels read them: contiguous and 16-byte aligned."""
        a = x[i:i + n].contiguous()
        return a.clone() if a.data_ptr() % 16 else a       # a slice of a batch of odd-sized images

    def _check_images(self, x, dev: torch.device, other_form: str = "", in_other_form: bool = False):
        """``x`` lives on the model's device ``dev`` and is fp32 ``[N, 3, H, W]`` (or in the caller's ``other_form``)."""
        if x.device != dev:
            raise _lib.DfhError(f"the images live on {x.device}, the model on {dev}: move them to the model's device (no CPU fallback)")
        if not in_other_form and (x.dtype != torch.float32 or x.dim() != 4 or x.shape[1] != 3):
            raise TypeError(f"images must be float32 [N, 3, H, W]{other_form}, got {x.dtype} {tuple(x.shape)}")

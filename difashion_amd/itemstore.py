"""The device-resident item store: cached VAE posteriors and history means for ``DiFashion``.

The reference encodes ``bsz x 4`` item images on every training step (DiFashion/models/difashion.py:123-136), one more for
``null_img``, and builds the history condition from a host dict of pre-averaged latents (data_utils.py:142-155), one copy per row.
The VAE is frozen and the item images are fixed wherever the transform is deterministic, so the posterior of every item can be
computed ONCE and kept in HBM:

  * ``ItemLatentStore`` -- one fp32 row ``[mean | std]`` per item; ``modes(iids)`` / ``sample(iids)`` are one ``dfh_item_gather`` launch
    and give ``latent_dist.mode() * sf`` / ``latent_dist.sample() * sf`` bit for bit (``std`` is the distribution's own tensor, the
    kernel's operations are torch's, separately rounded; the draw is the same ``torch.randn`` call at the same place of the stream);
  * ``HistoryTable`` -- the reference's raw ``history`` dict (``uid -> category -> [iids]``) as CSR arrays on the device;
    ``rows(uids, cates, null_latent)`` is one ``dfh_history_rows`` launch that averages the items' means from the SAME table.

Both drop into ``DiFashion.forward`` / ``fashion_generation`` where ``img_dataset`` / ``history`` go.  The store is valid while an
item's image does not change between steps: ``Resize`` + a crop of the same size on square images, no ``--random_flip``.  Under a
random crop of non-square images or a random flip it is not, and the image path remains.

Host side: dict lookups and index lists (plumbing); all arithmetic runs in libdifashion_hip.so (csrc/item_store.hip), no fallback.
"""
from __future__ import annotations

import json
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from . import _lib


def _require_device(t: torch.Tensor, what: str):
    if t.device.type != "cuda":
        raise _lib.DfhError(f"{what}: the table lives on {t.device}; the gather kernels run on the HIP device only (no CPU fallback) -- "
                            "build the store on, or load it to, the GPU")


class ItemLatentStore:
    """Per item one fp32 row ``[mean | std]`` of the VAE posterior (``std`` absent in a means-only store), on ``device``.

    ``scale`` is what a gathered row is multiplied by: ``vae.config.scaling_factor`` for a store of raw posteriors (``build``), 1 for a
    store of already scaled modes (``from_latents``).  ``scaling_factor`` remembers the VAE's value either way."""

    def __init__(self, table: torch.Tensor, latent_shape: Sequence[int], scaling_factor: float, scale: float, has_std: bool):
        latent_shape = tuple(int(s) for s in latent_shape)
        row_elems = int(np.prod(latent_shape))
        if table.dim() != 2 or table.dtype != torch.float32 or not table.is_contiguous():
            raise ValueError("the table is a contiguous fp32 matrix [items][row]")
        if table.shape[1] != row_elems * (2 if has_std else 1):
            raise ValueError(f"a table row holds {table.shape[1]} floats, the latent shape {latent_shape} "
                             f"{'with' if has_std else 'without'} std needs {row_elems * (2 if has_std else 1)}")
        if row_elems % 4:
            raise ValueError("C x H x W of a latent must be a multiple of 4 (rows are read as float4)")
        self.table, self.latent_shape, self.row_elems = table, latent_shape, row_elems
        self.scaling_factor, self.scale, self.has_std = float(scaling_factor), float(scale), bool(has_std)

    # ------------------------------------------------------------------ construction
    @classmethod
    @torch.no_grad()
    def build(cls, vae, img_dataset, device, batch_size: int = 64) -> "ItemLatentStore":
        """Encode every item once, in index order, in batches of ``batch_size``.  ``std`` is the ``.std`` tensor of each batch's
        ``latent_dist`` itself, so ``sample`` repeats the image path's arithmetic on the same numbers."""
        if hasattr(vae, "to"):
            vae = vae.to(device)
        n = len(img_dataset)
        if n == 0:
            raise ValueError("the item table is empty")
        table, shape = None, None
        for start in range(0, n, batch_size):
            stop = min(start + batch_size, n)
            imgs = torch.stack([img_dataset[i] for i in range(start, stop)], dim=0)
            imgs = imgs.to(memory_format=torch.contiguous_format).float().to(device)
            dist = vae.encode(imgs).latent_dist
            mean, std = dist.mean, dist.std
            if table is None:
                shape = tuple(mean.shape[1:])
                table = torch.empty((n, 2 * mean[0].numel()), dtype=torch.float32, device=mean.device)
            e = table.shape[1] // 2
            table[start:stop, :e] = mean.reshape(stop - start, e)
            table[start:stop, e:] = std.reshape(stop - start, e)
        return cls(table, shape, vae.config.scaling_factor, vae.config.scaling_factor, True)

    @classmethod
    def from_latents(cls, all_latents, scaling_factor: float, device=None) -> "ItemLatentStore":
        """Wrap the ``all_item_latents.npy`` cache of ``data.preprocess_dataset`` -- ``mode() * scaling_factor`` per item -- as a
        means-only store with scale 1.  ``sample`` on such a store raises: the cache has no std."""
        lat = torch.as_tensor(np.asarray(all_latents) if not isinstance(all_latents, torch.Tensor) else all_latents).float()
        if lat.dim() < 2:
            raise ValueError("all_latents is [items][C][H][W]")
        table = lat.reshape(lat.shape[0], -1).contiguous()
        if device is not None:
            table = table.to(device)
        return cls(table, lat.shape[1:], scaling_factor, 1.0, False)

    # ------------------------------------------------------------------ persistence: one .npy and a small JSON of settings
    def save(self, path: str) -> None:
        np.save(path + ".npy", self.table.detach().cpu().numpy())
        with open(path + ".json", "w") as f:
            json.dump(dict(items=len(self), latent_shape=list(self.latent_shape), scaling_factor=self.scaling_factor, scale=self.scale,
                           has_std=self.has_std, dtype="float32"), f)

    @classmethod
    def load(cls, path: str, device=None) -> "ItemLatentStore":
        with open(path + ".json") as f:
            meta = json.load(f)
        table = torch.from_numpy(np.load(path + ".npy"))
        if table.shape[0] != meta["items"]:
            raise ValueError(f"{path}.npy holds {table.shape[0]} items, {path}.json says {meta['items']}")
        if device is not None:
            table = table.to(device)
        return cls(table, meta["latent_shape"], meta["scaling_factor"], meta["scale"], meta["has_std"])

    # ------------------------------------------------------------------ sizes
    def __len__(self) -> int:
        return self.table.shape[0]

    @property
    def nbytes(self) -> int:
        return self.table.numel() * 4

    @property
    def device(self) -> torch.device:
        return self.table.device

    # ------------------------------------------------------------------ the gathers
    def _ids(self, iids) -> torch.Tensor:
        """int64 ids on the table's device.  Ids that arrive on the CPU are range-checked there before upload; ids already on the
        device are not synced for a check -- the kernel turns a bad id into a row of NaN."""
        t = iids if isinstance(iids, torch.Tensor) else torch.as_tensor(iids, dtype=torch.int64)
        if t.is_floating_point() or t.dtype == torch.bool:
            raise TypeError(f"item ids must be integers, got {t.dtype}")
        t = t.reshape(-1)
        if t.device.type == "cpu" and t.numel() and (int(t.min()) < 0 or int(t.max()) >= len(self)):
            raise IndexError(f"item id out of range [0, {len(self)}): {int(t.min() if int(t.min()) < 0 else t.max())}")
        return t.to(device=self.device, dtype=torch.int64).contiguous()

    def _gather(self, iids, eps: Optional[torch.Tensor]) -> torch.Tensor:
        ids = self._ids(iids)
        _require_device(self.table, "ItemLatentStore")
        n = ids.numel()
        out = torch.empty((n,) + self.latent_shape, dtype=torch.float32, device=self.device)
        _lib.call("dfh_item_gather", _lib.ptr(self.table), len(self), self.table.shape[1], self.row_elems, _lib.ptr(ids), n, _lib.ptr(eps),
                  self.scale, _lib.ptr(out), _lib.stream_ptr())
        return out

    def modes(self, iids) -> torch.Tensor:
        """``vae.encode(images[iids]).latent_dist.mode() * scaling_factor`` -> (n, C, H, W)."""
        return self._gather(iids, None)

    def sample(self, iids, eps: Optional[torch.Tensor] = None, generator: Optional[torch.Generator] = None) -> torch.Tensor:
        """``vae.encode(images[iids]).latent_dist.sample(generator) * scaling_factor`` -> (n, C, H, W).  Without ``eps`` the noise is
        drawn by the very call ``DiagonalGaussianDistribution.sample`` makes, so the RNG stream is consumed identically."""
        if not self.has_std:
            raise ValueError("this store holds means only (from_latents): it cannot sample; build it with ItemLatentStore.build")
        n = len(iids) if not isinstance(iids, torch.Tensor) else iids.numel()
        shape = (n,) + self.latent_shape
        if eps is None:
            eps = torch.randn(shape, generator=generator, device=self.device, dtype=torch.float32)
        elif tuple(eps.shape) != shape or eps.dtype != torch.float32 or eps.device != self.device:
            raise ValueError(f"eps must be fp32 {shape} on {self.device}")
        return self._gather(iids, eps.contiguous())

    def null_latent(self) -> torch.Tensor:
        """The scaled mode of item 0: ``null_img = img_dataset[0]`` in the reference."""
        return self.modes([0])[0]


class HistoryTable:
    """The reference's raw ``history`` dict (``uid -> category -> [iids]``) against an ``ItemLatentStore``: CSR arrays on the device
    (``seg_items`` int64, ``seg_offsets`` int64) and a host map ``(uid, category) -> segment``.

    Keys are matched BY INTEGER VALUE, whether they arrive as Python ints or 0-d tensors.  This is what ``TensorKeyDict`` does in the
    tests -- and NOT what a plain dict does on the dict path: there ``DiFashion._history_rows`` keeps the reference's literal
    ``cate in history[uid]`` with a 0-d tensor ``cate``, which hashes by identity and falls back to the null latent."""

    def __init__(self, history: Dict, store: ItemLatentStore):
        self.store = store
        self.segment_of: Dict = {}
        items: List[int] = []
        offsets = [0]
        for uid, per_cate in history.items():
            if isinstance(uid, str):                      # data.history_latents adds hist["null"]; the raw dict has no such key
                continue
            for cate, iids in per_cate.items():
                ids = [int(i) for i in (iids.tolist() if hasattr(iids, "tolist") else iids)]
                bad = [i for i in ids if i < 0 or i >= len(store)]
                if bad:
                    raise IndexError(f"history[{int(uid)}][{int(cate)}]: item id out of range [0, {len(store)}): {bad[0]}")
                self.segment_of[(int(uid), int(cate))] = len(offsets) - 1
                items += ids
                offsets.append(len(items))
        self.items, self.offsets = items, offsets
        self.seg_items = torch.tensor(items if items else [0], dtype=torch.int64, device=store.device)
        self.seg_offsets = torch.tensor(offsets, dtype=torch.int64, device=store.device)

    def __len__(self) -> int:
        return len(self.offsets) - 1

    def segment_ids(self, uids, cates, use_history: bool = True) -> List[int]:
        """Per row the segment of ``(uid, category)``; -1 for a missing user, a missing category, or ``use_history=False``."""
        if len(uids) != len(cates):
            raise ValueError(f"{len(uids)} uids for {len(cates)} categories")
        if not use_history:
            return [-1] * len(uids)
        return [self.segment_of.get((int(u), int(c)), -1) for u, c in zip(uids, cates)]

    def rows(self, uids, cates, null_latent: torch.Tensor, use_history: bool = True) -> torch.Tensor:
        """(rows, C, H, W): per row the mean of the scaled modes of its segment's items, summed in list order; the null latent where
        the row has no segment.  One launch."""
        st = self.store
        segs = self.segment_ids(uids, cates, use_history)
        _require_device(st.table, "HistoryTable")
        null = null_latent.to(device=st.device, dtype=torch.float32).contiguous()
        if null.numel() != st.row_elems:
            raise ValueError(f"null_latent holds {null.numel()} values, a latent {st.latent_shape} has {st.row_elems}")
        row_seg = torch.tensor(segs, dtype=torch.int32).to(st.device)
        out = torch.empty((len(segs),) + st.latent_shape, dtype=torch.float32, device=st.device)
        _lib.call("dfh_history_rows", _lib.ptr(st.table), len(st), st.table.shape[1], st.row_elems, _lib.ptr(self.seg_items),
                  _lib.ptr(self.seg_offsets), _lib.ptr(row_seg), len(segs), _lib.ptr(null), st.scale, _lib.ptr(out), _lib.stream_ptr())
        return out

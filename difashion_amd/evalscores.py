"""The embedding-side metrics of the reference's evaluation on the MI355X HIP path.

What the reference computes from the CLIP embeddings once ``encode_image`` / ``encode_text`` have run (Evaluation/eval_utils.py):
  * ``CLIPScore.calculate_clip_score`` (:101-114), ``calculate_clip_img_score`` (:117-135) and the personalisation similarity
    (:503-538): normalise, ``100 * F.cosine_similarity`` per row;
  * the retrieval accuracy (:652-723, five candidates a row) and ranking (:725-767, thousands): cosine against ``cnn_features[candidates]``
    and an argmax;
  * ``CompatibilityEvaluator.evaluate_compatibility`` (:574-588) over ``FashionEvaluator``
    (Evaluation/compatibility_evaluator/compatibility_net.py:14-81), which the reference runs one outfit at a time.
And, over images and not embeddings:
  * ``calculate_lpips_given_data`` (:473-501) and the two ``calculate_lpips_retrieval_acc_given_data*`` (:769-821) over an ``LPIPS`` model
    (lpips.py): ``lpips_given_data`` and ``lpips_retrieval`` below, batch by batch without the DataLoader;
  * ``calculate_fid_given_data`` (:282-337) and ``calculate_inception_score_given_data`` (:339-406) over the two Inception v3 models
    (inception.py): ``activation_statistics``, ``frechet_distance`` (the one host step, as in the reference),
    ``fid_given_data``, ``inception_rows``, ``inception_score_from_probs`` and ``inception_score_given_data`` at the end of the file.

All arithmetic runs in the kernel library (csrc/eval_scores.hip: ``dfh_embed_pair_cosine``, ``dfh_embed_candidates``,
``dfh_compat_score``) in fp32, in both storage builds.  The ``nn.Linear`` / ``nn.LayerNorm`` modules of ``FashionEvaluator`` only HOLD
the parameters under the reference's state-dict names; they are never called.  No PyTorch / CPU fallback.  Only the cosine similarity is
built: the reference's euclidean branches return a 0-d tensor per batch that its own ``torch.cat`` cannot take.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch
import torch.nn as nn

from . import _lib
from ._native import grow_buffer, require_hip_fp32, require_params_on

NUM_PARAMS = 32          # DFH_COMPAT_NUM_PARAMS
EMB_DIM = 256


def _require_cosine(similarity_func: str) -> None:
    if similarity_func != "cosine":
        raise ValueError(f"Unrecognized similarity function {similarity_func}.")


def _device_rows(t: torch.Tensor, what: str) -> torch.Tensor:
    """A contiguous fp32 matrix on the GPU, or a refusal."""
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise _lib.DfhError(f"{what} runs only on the MI355X HIP path: move it to 'cuda' (no CPU fallback)")
    if t.dtype != torch.float32:
        raise TypeError(f"{what} must be float32 (the scores are fp32 end to end), got {t.dtype}")
    return t.contiguous()


def pair_cosine(a: torch.Tensor, b: torch.Tensor, scale: float = 100.0) -> torch.Tensor:
    """``scale * F.cosine_similarity(a / |a|, b / |b|)`` per row of two [rows, dim] device tensors."""
    a, b = _device_rows(a, "pair_cosine: a"), _device_rows(b, "pair_cosine: b")
    if a.dim() != 2 or a.shape != b.shape or a.device != b.device:
        raise ValueError(f"pair_cosine needs two [rows, dim] tensors of one shape on one device, got {tuple(a.shape)} and {tuple(b.shape)}")
    out = torch.empty((a.shape[0],), dtype=torch.float32, device=a.device)
    if a.shape[0]:
        with torch.cuda.device(a.device):
            _lib.call("dfh_embed_pair_cosine", _lib.ptr(a), _lib.ptr(b), _lib.ptr(out), a.shape[0], a.shape[1], float(scale), _lib.stream_ptr())
    return out


def candidate_cosine(gen: torch.Tensor, table: torch.Tensor, candidates: torch.Tensor):
    """``F.cosine_similarity(gen[:, None], table[candidates], dim=-1)`` and its ``argmax(dim=1)`` -> (sims [rows, K], preds [rows])."""
    gen, table = _device_rows(gen, "candidate_cosine: gen"), _device_rows(table, "candidate_cosine: table")
    if gen.dim() != 2 or table.dim() != 2 or gen.shape[1] != table.shape[1] or gen.device != table.device:
        raise ValueError(f"gen [rows, dim] and table [table_rows, dim] must share dim and device, got {tuple(gen.shape)} and {tuple(table.shape)}")
    cand = torch.as_tensor(candidates)
    if cand.dtype not in (torch.int64, torch.int32, torch.int16, torch.uint8, torch.int8):
        raise TypeError(f"candidates must be integer ids, got {cand.dtype}")
    if cand.dim() != 2 or cand.shape[0] != gen.shape[0] or cand.shape[1] < 1:
        raise ValueError(f"candidates must be [rows = {gen.shape[0]}, K >= 1], got {tuple(cand.shape)}")
    # indexing raises on out-of-range ids; checked where the ids live (a DataLoader batch is a CPU tensor: no device sync then)
    lo, hi = (int(cand.min()), int(cand.max())) if cand.numel() else (0, 0)
    if lo < 0 or hi >= table.shape[0]:
        raise IndexError(f"candidate ids out of range [0, {table.shape[0]}): min {lo}, max {hi}")
    cand = cand.to(device=gen.device, dtype=torch.int64).contiguous()
    rows, K = cand.shape
    sims = torch.empty((rows, K), dtype=torch.float32, device=gen.device)
    preds = torch.empty((rows,), dtype=torch.int64, device=gen.device)
    if rows:
        with torch.cuda.device(gen.device):
            _lib.call("dfh_embed_candidates", _lib.ptr(gen), _lib.ptr(table), _lib.ptr(cand), _lib.ptr(sims), _lib.ptr(preds), rows, K,
                      gen.shape[1], table.shape[0], _lib.stream_ptr())
    return sims, preds


@torch.no_grad()
def extract_image_features(image_model, processor, images, batch_size: int = 200) -> torch.Tensor:
    """The reference's ``extract_cnn_features`` (Evaluation/extract_hist_embs.py:81-103) without the DataLoader worker: ``processor``
    (``CLIPImageProcessor``) then ``image_model.encode_image`` batch by batch -> [N, projection_dim] fp32 on the model's device.
    ``images``: a device tensor in one of the processor's forms, or a sequence of PIL images / HWC uint8 arrays."""
    if batch_size < 1:
        raise ValueError(f"batch_size must be positive, got {batch_size}")
    n = images.shape[0] if isinstance(images, torch.Tensor) else len(images)
    if n < 1:
        raise ValueError("images holds no image")
    feats = []
    for i in range(0, n, batch_size):
        batch = images[i:i + batch_size]
        pixels = processor(images=batch if isinstance(batch, torch.Tensor) else list(batch), return_tensors="pt",
                           device=image_model.device).pixel_values
        feats.append(image_model.encode_image(pixels))
    return torch.cat(feats)


def _image_batches(images, batch_size: int, what: str):
    """Batches of a device tensor, or of a list of per-image device tensors (stacked a batch at a time)."""
    if batch_size < 1:
        raise ValueError(f"batch_size must be positive, got {batch_size}")
    n = images.shape[0] if isinstance(images, torch.Tensor) else len(images)
    if n < 1:
        raise ValueError(f"{what} holds no image")
    for i in range(0, n, batch_size):
        batch = images[i:i + batch_size]
        yield batch if isinstance(batch, torch.Tensor) else torch.stack(list(batch))


@torch.no_grad()
def lpips_given_data(model, gen, grd, batch_size: int = 64) -> torch.Tensor:
    """The per-pair scores ``[N]`` of ``calculate_lpips_given_data`` (eval_utils.py:473-501); the reference's number is their mean.
    ``gen`` / ``grd``: device tensors in one of ``LPIPS.forward``'s input forms, or lists of per-image device tensors."""
    n0 = gen.shape[0] if isinstance(gen, torch.Tensor) else len(gen)
    n1 = grd.shape[0] if isinstance(grd, torch.Tensor) else len(grd)
    if n0 != n1:
        raise ValueError(f"gen holds {n0} images, grd {n1}")
    return torch.cat([model(a, b).reshape(-1) for a, b in zip(_image_batches(gen, batch_size, "gen"), _image_batches(grd, batch_size, "grd"))])


@torch.no_grad()
def lpips_retrieval(model, gen, candidates, K: int = 5, batch_size: int = 64):
    """``calculate_lpips_retrieval_acc_given_data`` (eval_utils.py:796-821): ``gen`` and ``candidates`` hold ``rows * K`` images each,
    row-major, a row's first candidate being the ground truth.  Returns ``(scores [rows, K], preds [rows], accuracy)``: ``preds`` is
    ``torch.argmin`` over a row on the HIP path, the accuracy the share of ``preds == 0``."""
    from .lpips import group_argmin
    if K < 1:
        raise ValueError(f"K must be positive, got {K}")
    scores = lpips_given_data(model, gen, candidates, batch_size)
    if scores.numel() % K:
        raise ValueError(f"{scores.numel()} pairs do not make whole rows of K={K}")
    scores = scores.reshape(-1, K)
    preds = group_argmin(scores)
    return scores, preds, int((preds == 0).sum()) / scores.shape[0]


class FashionEvaluator(nn.Module):
    """compatibility_net.py's class under its own state-dict names (``feat_layer.*``, ``emb_layer.{0,1,4,5,8,9,12,13}.*``,
    ``eval_layer.{0,1,4,5,8,9,12}.*``), inference only: Dropout is the identity, every outfit of a call runs together."""

    def __init__(self, cnn_feat_dim: int):
        super().__init__()
        if cnn_feat_dim < 4 or cnn_feat_dim % 4:
            raise ValueError(f"cnn_feat_dim must be a positive multiple of 4 (the kernels read rows as float4), got {cnn_feat_dim}")
        self.cnn_feat_dim = cnn_feat_dim
        self.feat_layer = nn.Linear(cnn_feat_dim, 1024)

        def stack(dims, last=None):
            mods = []
            for k, n in zip(dims[:-1], dims[1:]):
                mods += [nn.Linear(k, n), nn.LayerNorm(n), nn.ReLU(), nn.Dropout(0.35)]
            return nn.Sequential(*(mods + ([nn.Linear(dims[-1], last)] if last else [])))

        self.emb_layer = stack([2048, 512, 512, 256, EMB_DIM])
        self.eval_layer = stack([EMB_DIM, 128, 128, 32], last=1)
        for m in self.modules():
            if isinstance(m, nn.Linear):                      # the reference's xavier_normal_initialization
                nn.init.xavier_normal_(m.weight.data)
                nn.init.constant_(m.bias.data, 0)
        self._ws = None
        super().train(False)
        self.requires_grad_(False)

    def train(self, mode: bool = True):
        if mode:
            raise NotImplementedError("FashionEvaluator is inference only on this path (eval_utils.py:550 puts it in eval mode): there is "
                                      "no Dropout and no backward kernel; .eval() is the only mode")
        return super().train(False)

    # ------------------------------------------------------------------ plumbing
    def _require_hip_fp32(self, what: str, *tensors) -> torch.device:
        plist = list(self.parameters())
        dev = require_hip_fp32(what, plist, "parameters must stay fp32 (the kernels read them in place)")
        require_params_on(dev, plist)
        if torch.is_grad_enabled() and any(p.requires_grad for p in plist):
            raise _lib.DfhError(f"{what} is inference only: call it under torch.no_grad() or .requires_grad_(False)")
        for t in tensors:
            if t is None:
                continue
            if t.device != dev:
                raise _lib.DfhError(f"{what}: a tensor lives on {t.device}, the model on {dev}: move it to the model's device (no CPU fallback)")
            if t.dtype != torch.float32:
                raise TypeError(f"{what}: features must be float32, got {t.dtype}")
        return dev

    def _pointers(self):
        plist = list(self.parameters())
        assert len(plist) == NUM_PARAMS
        return (C.c_void_p * NUM_PARAMS)(*[p.data_ptr() for p in plist]), plist

    def _workspace(self, dev, outfits: int, items: int, dim: int) -> torch.Tensor:
        return grow_buffer(self, "_ws", _lib.raw().dfh_compat_workspace_bytes(outfits, items, dim), dev)

    def _score(self, what, feats_real, feats_gen, olists, outfits, items, want_scores=True):
        """-> (outfit_emb [O, 256], logits [O], scores [O])"""
        dev = self._require_hip_fp32(what, feats_real, feats_gen)
        if not 2 <= items <= 8:
            raise ValueError(f"{what}: outfits of 2 to 8 items are built, got {items}")
        dim = self.cnn_feat_dim
        emb = torch.empty((outfits, EMB_DIM), dtype=torch.float32, device=dev)
        logits = torch.empty((outfits,), dtype=torch.float32, device=dev) if want_scores else None
        scores = torch.empty((outfits,), dtype=torch.float32, device=dev) if want_scores else None
        if outfits == 0:
            return emb, logits, scores
        arr, keep = self._pointers()
        ws = self._workspace(dev, outfits, items, dim)
        with torch.cuda.device(dev):
            _lib.call("dfh_compat_score", arr, NUM_PARAMS, dim, _lib.ptr(feats_real), feats_real.shape[0],
                      _lib.ptr(feats_gen), 0 if feats_gen is None else feats_gen.shape[0], _lib.ptr(olists), outfits, items, _lib.ptr(emb),
                      _lib.ptr(logits), _lib.ptr(scores), _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
        del keep
        return emb, logits, scores

    def _gathered(self, cnn_feats: torch.Tensor, what: str):
        if not isinstance(cnn_feats, torch.Tensor) or cnn_feats.dim() != 3 or cnn_feats.shape[2] != self.cnn_feat_dim:
            raise ValueError(f"{what}: cnn_feats must be [outfits, items, {self.cnn_feat_dim}], got "
                             f"{tuple(cnn_feats.shape) if isinstance(cnn_feats, torch.Tensor) else type(cnn_feats)}")
        self._require_hip_fp32(what, cnn_feats)
        O, items, dim = cnn_feats.shape
        return cnn_feats.contiguous().reshape(O * items, dim), O, items

    # ------------------------------------------------------------------ the reference's three methods
    @torch.no_grad()
    def outfit_emb(self, cnn_feats: torch.Tensor) -> torch.Tensor:
        flat, O, items = self._gathered(cnn_feats, "FashionEvaluator.outfit_emb")
        return self._score("FashionEvaluator.outfit_emb", flat, None, None, O, items, want_scores=False)[0]

    @torch.no_grad()
    def pred_score(self, o_embs: torch.Tensor) -> torch.Tensor:
        dev = self._require_hip_fp32("FashionEvaluator.pred_score", o_embs)
        if o_embs.dim() != 2 or o_embs.shape[1] != EMB_DIM:
            raise ValueError(f"o_embs must be [outfits, {EMB_DIM}], got {tuple(o_embs.shape)}")
        o_embs = o_embs.contiguous()
        O = o_embs.shape[0]
        logits = torch.empty((O,), dtype=torch.float32, device=dev)
        if O:
            arr, keep = self._pointers()
            ws = self._workspace(dev, O, 2, 4)
            with torch.cuda.device(dev):
                _lib.call("dfh_compat_pred_score", arr, NUM_PARAMS, _lib.ptr(o_embs), O, _lib.ptr(logits), None, _lib.ptr(ws), ws.numel(),
                          _lib.stream_ptr())
            del keep
        return logits

    @torch.no_grad()
    def forward(self, cnn_feats: torch.Tensor) -> torch.Tensor:
        flat, O, items = self._gathered(cnn_feats, "FashionEvaluator")
        return self._score("FashionEvaluator", flat, None, None, O, items)[1]


class CompatibilityEvaluator:
    """eval_utils.py:540-588 without the CLIP model it also holds (``CLIPVisionModelWithProjection.encode_image`` is that part)."""

    def __init__(self, evaluator: FashionEvaluator, device="cuda"):
        self.device = torch.device(device)
        self.evaluator = evaluator.to(self.device).eval()

    @torch.no_grad()
    def evaluate_compatibility(self, outfits, cnn_feats: torch.Tensor, cnn_feats_gen: Optional[torch.Tensor], return_all: bool = False):
        """``outfits``: [O, items] integer ids, an id <= 0 reads ``cnn_feats_gen[-id]``, an id > 0 reads ``cnn_feats[id]``.  Returns the
        sigmoid scores [O]; ``return_all=True``: (outfit_emb, logits, scores)."""
        ev = self.evaluator
        what = "evaluate_compatibility"
        ol = torch.as_tensor(outfits)
        if ol.dim() != 2 or ol.dtype not in (torch.int64, torch.int32, torch.int16, torch.int8):
            raise ValueError(f"outfits must be [outfits, items] integer ids, got {tuple(ol.shape)} {ol.dtype}")
        for t, name in ((cnn_feats, "cnn_feats"), (cnn_feats_gen, "cnn_feats_gen")):
            if t is not None and (t.dim() != 2 or t.shape[1] != ev.cnn_feat_dim or t.shape[0] < 1):
                raise ValueError(f"{name} must be [rows >= 1, {ev.cnn_feat_dim}], got {tuple(t.shape)}")
        if ol.numel():
            # what indexing would raise on; checked where the ids live
            lo, hi = int(ol.min()), int(ol.max())
            if hi >= cnn_feats.shape[0]:
                raise IndexError(f"item id {hi} out of range for cnn_feats with {cnn_feats.shape[0]} rows")
            if lo <= 0 and cnn_feats_gen is None:
                raise TypeError("outfits hold generated items (ids <= 0) but cnn_feats_gen is None")
            if lo <= 0 and -lo >= cnn_feats_gen.shape[0]:
                raise IndexError(f"generated item id {lo} out of range for cnn_feats_gen with {cnn_feats_gen.shape[0]} rows")
        ev._require_hip_fp32(what, cnn_feats, cnn_feats_gen)
        ol = ol.to(device=cnn_feats.device, dtype=torch.int64).contiguous()
        emb, logits, scores = ev._score(what, cnn_feats.contiguous(), None if cnn_feats_gen is None else cnn_feats_gen.contiguous(), ol,
                                        ol.shape[0], ol.shape[1])
        return (emb, logits, scores) if return_all else scores


class CLIPScore:
    """eval_utils.py:91-135 over the two HIP towers: ``image_model.encode_image`` (CLIPVisionModelWithProjection) and
    ``text_model.encode_text`` (CLIPTextModelWithProjection).  Images are preprocessed pixel tensors, texts are token ids (the tokenizer
    stays with the caller)."""

    def __init__(self, image_model, text_model=None):
        self.image_model, self.text_model = image_model, text_model

    @torch.no_grad()
    def calculate_clip_score(self, images: torch.Tensor, token_ids: torch.Tensor) -> torch.Tensor:
        if self.text_model is None:
            raise _lib.DfhError("calculate_clip_score needs the text tower: CLIPScore(image_model, text_model)")
        return pair_cosine(self.image_model.encode_image(images), self.text_model.encode_text(token_ids), 100.0)

    @torch.no_grad()
    def calculate_clip_img_score(self, images1: torch.Tensor, images2: torch.Tensor, similarity_func: str = "cosine") -> torch.Tensor:
        _require_cosine(similarity_func)
        return pair_cosine(self.image_model.encode_image(images1), self.image_model.encode_image(images2), 100.0)

    @torch.no_grad()
    def personalization_sim(self, images: torch.Tensor, hist_embs: torch.Tensor, similarity_func: str = "cosine") -> torch.Tensor:
        """Per-row score of ``evaluate_personalization_given_data_sim`` (eval_utils.py:515-531): generated images against the user's
        history embedding."""
        _require_cosine(similarity_func)
        return pair_cosine(self.image_model.encode_image(images), hist_embs, 100.0)

    @torch.no_grad()
    def retrieval(self, images: torch.Tensor, cnn_features: torch.Tensor, candidates: torch.Tensor, similarity_func: str = "cosine"):
        """(sims [rows, K], preds [rows]) of ``calculate_clip_retrieval_acc_given_data2`` (eval_utils.py:702-715); the ranking of
        ``clip_og_retrieval_given_data`` (:733-745) is a ``topk`` over the same sims."""
        _require_cosine(similarity_func)
        return candidate_cosine(self.image_model.encode_image(images), cnn_features, candidates)


# ------------------------------------------------------------------ FID and the Inception Score (csrc/inception.hip)
@torch.no_grad()
def activation_statistics(model, data, batch_size: int = 50, dims: int = 2048):
    """``calculate_activation_statistics`` (eval_utils.py:282-320): ``(mu [dims], sigma [dims, dims])`` as fp64 DEVICE tensors --
    ``np.mean(act, axis=0)`` and ``np.cov(act, rowvar=False)`` of the float64 copy of the pooled activations, on the fp64 matrix
    instruction.  ``model``: a ``FIDInceptionV3`` whose first output block is ``dims`` wide; ``data``: fp32 ``[N, 3, H, W]`` in [0, 1]
    on the device, or a list of per-image device tensors."""
    acts = []
    for batch in _image_batches(data, batch_size, "data"):
        pred = model(batch)[0]
        if pred.shape[1] != dims:
            raise ValueError(f"the model's first output block is {pred.shape[1]} wide, dims={dims}")
        acts.append(pred.reshape(pred.shape[0], dims))
    act = torch.cat(acts).contiguous()
    N = act.shape[0]
    if N < 2:
        raise ValueError(f"the covariance needs at least two images (N - 1 divides), got {N}")
    mu = torch.empty((dims,), dtype=torch.float64, device=act.device)
    sigma = torch.empty((dims, dims), dtype=torch.float64, device=act.device)
    with torch.cuda.device(act.device):
        _lib.call("dfh_incep_stats", _lib.ptr(act), N, dims, _lib.ptr(mu), _lib.ptr(sigma), _lib.stream_ptr())
    return mu, sigma


def frechet_distance(mu1, sigma1, mu2, sigma2, eps: float = 1e-6) -> float:
    """pytorch_fid's ``calculate_frechet_distance`` restated in fp64 on the HOST -- the one host step of the row, where the reference
    has it: ``|mu1 - mu2|^2 + tr s1 + tr s2 - 2 tr sqrtm(s1 s2)``, with the ``eps`` offset on both covariances when the root is not
    finite and the imaginary-diagonal check at 1e-3.  Takes numpy arrays or tensors (device tensors are copied to the host)."""
    import numpy as np
    try:
        from scipy import linalg
    except ImportError as e:
        raise ImportError("frechet_distance needs scipy (scipy.linalg.sqrtm, as pytorch_fid does): install scipy; the statistics "
                          "themselves (activation_statistics) do not need it") from e

    def host(a):
        return np.asarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=np.float64)

    def root(a):
        r = linalg.sqrtm(a)
        return r[0] if isinstance(r, tuple) else r

    mu1, mu2 = np.atleast_1d(host(mu1)), np.atleast_1d(host(mu2))
    sigma1, sigma2 = np.atleast_2d(host(sigma1)), np.atleast_2d(host(sigma2))
    if mu1.shape != mu2.shape:
        raise ValueError("Training and test mean vectors have different lengths")
    if sigma1.shape != sigma2.shape:
        raise ValueError("Training and test covariances have different dimensions")
    diff = mu1 - mu2
    covmean = root(sigma1.dot(sigma2))
    if not np.isfinite(covmean).all():
        offset = np.eye(sigma1.shape[0]) * eps
        covmean = root((sigma1 + offset).dot(sigma2 + offset))
    if np.iscomplexobj(covmean):
        if not np.allclose(np.diagonal(covmean).imag, 0, atol=1e-3):
            raise ValueError(f"Imaginary component {np.max(np.abs(covmean.imag))}")
        covmean = covmean.real
    return float(diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2 * np.trace(covmean))


@torch.no_grad()
def fid_given_data(gen, grd, batch_size: int = 50, dims: int = 2048, model=None) -> float:
    """``calculate_fid_given_data`` (eval_utils.py:322-337).  ``model``: a ``FIDInceptionV3`` on the device holding the FID weights
    (built for block ``BLOCK_INDEX_BY_DIM[dims]``); None makes one with seeded stand-in weights on the images' device."""
    from .inception import FIDInceptionV3
    if dims not in FIDInceptionV3.BLOCK_INDEX_BY_DIM:
        raise ValueError(f"dims must be one of {sorted(FIDInceptionV3.BLOCK_INDEX_BY_DIM)}, got {dims}")
    if model is None:
        first = gen if isinstance(gen, torch.Tensor) else gen[0]
        model = FIDInceptionV3([FIDInceptionV3.BLOCK_INDEX_BY_DIM[dims]]).to(first.device)
    m1, s1 = activation_statistics(model, gen, batch_size, dims)
    m2, s2 = activation_statistics(model, grd, batch_size, dims)
    return frechet_distance(m1, s1, m2, s2)


@torch.no_grad()
def inception_rows(probs: torch.Tensor, cate: Optional[torch.Tensor] = None, eps: float = 1e-16):
    """Per image of ``probs [N, classes]``: ``(label int64, entropy, kl, correct)`` -- ``argmax``, ``-sum p log(p + eps)``,
    ``sum p (log(p + eps) - log(1 / classes))`` and ``label == cate`` (zeros without ``cate``), on the HIP path."""
    probs = _device_rows(probs, "inception_rows: probs")
    if probs.dim() != 2 or probs.shape[0] < 1 or probs.shape[1] < 1:
        raise ValueError(f"probs must be [N >= 1, classes >= 1], got {tuple(probs.shape)}")
    N, dev = probs.shape[0], probs.device
    if cate is not None:
        if not isinstance(cate, torch.Tensor) or cate.device != dev or cate.numel() != N:
            raise ValueError(f"cate must hold one label per image on {dev}")
        cate = cate.reshape(N).to(torch.int64).contiguous()
    label = torch.empty((N,), dtype=torch.int64, device=dev)
    ent, kl, correct = (torch.empty((N,), dtype=torch.float32, device=dev) for _ in range(3))
    with torch.cuda.device(dev):
        _lib.call("dfh_incep_is_rows", _lib.ptr(probs), _lib.ptr(cate), N, probs.shape[1], float(eps), _lib.ptr(label), _lib.ptr(ent), _lib.ptr(kl),
                  _lib.ptr(correct), _lib.stream_ptr())
    return label, ent, kl, correct


@torch.no_grad()
def inception_score_from_probs(probs: torch.Tensor, cate: torch.Tensor, num_splits: int = 1, eps: float = 1e-16):
    """The arithmetic of ``calculate_inception_score_given_data`` after the network (eval_utils.py:371-406) on ``probs [N, classes]``:
    ``(acc, mean entropy, std entropy, mean score, std score)``; split ``i`` holds images ``[i N // num_splits, (i + 1) N // num_splits)``,
    the standard deviations are unbiased (``nan`` for one split, as the reference's are)."""
    _, ent, kl, correct = inception_rows(probs, cate, eps)
    N = probs.shape[0]
    if not 1 <= num_splits <= N:
        raise ValueError(f"num_splits must be in 1 .. {N}, got {num_splits}")
    out = torch.empty((num_splits, 3), dtype=torch.float32, device=probs.device)
    with torch.cuda.device(probs.device):
        _lib.call("dfh_incep_is_splits", _lib.ptr(ent), _lib.ptr(kl), _lib.ptr(correct), N, num_splits, _lib.ptr(out), _lib.stream_ptr())
    rows = out.cpu().double()                            # num_splits x 3 numbers: the last step is host arithmetic on them

    def mean_std(v):
        m = float(v.mean())
        return m, (float(((v - m) ** 2).sum() / (len(v) - 1)) ** 0.5 if len(v) > 1 else float("nan"))

    acc = float(rows[:, 2].sum()) / N
    return (acc,) + mean_std(rows[:, 0]) + mean_std(rows[:, 1])


@torch.no_grad()
def inception_score_given_data(model, data, cate, batch_size: int = 50, num_splits: int = 1, eps: float = 1e-16, resize_input: bool = True,
                               normalize_input: bool = True):
    """``calculate_inception_score_given_data`` (eval_utils.py:339-406) over an ``InceptionV3`` on the device: ``data`` fp32
    ``[N, 3, H, W]`` (or a list of per-image tensors) in [0, 1], ``cate [N]`` the categories.  The resize to 299 x 299 and ``2 x - 1``
    run in the network's first kernel."""
    model.set_input_flags(resize_input, normalize_input)
    probs = torch.cat([model(batch) for batch in _image_batches(data, batch_size, "data")])
    if not isinstance(cate, torch.Tensor):
        cate = torch.as_tensor(list(cate))
    return inception_score_from_probs(probs, cate.to(probs.device), num_splits, eps)

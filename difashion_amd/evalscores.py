"""The embedding-side metrics of the reference's evaluation on the MI355X HIP path.

What the reference computes from the CLIP embeddings once ``encode_image`` / ``encode_text`` have run (Evaluation/eval_utils.py):
  * ``CLIPScore.calculate_clip_score`` (:101-114), ``calculate_clip_img_score`` (:117-135) and the personalisation similarity
    (:503-538): normalise, ``100 * F.cosine_similarity`` per row;
  * the retrieval accuracy (:652-723, five candidates a row): cosine against ``cnn_features[candidates]`` and an argmax;
  * the grounding retrieval (:725-767, ``clip_og_retrieval_given_data``): every image against ALL items of its category -- ragged
    candidate sets -- the best 100 kept in order, recall@{10,20,50,100} (csrc/eval_rank.hip: ``rank_candidates``,
    ``CLIPScore.grounding_retrieval``);
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


# ------------------------------------------------------------------ grounding retrieval: ragged top-N ranking, recall@N (csrc/eval_rank.hip)
RANK_NMAX = 128                      # DFH_EMBED_RANK_NMAX
RANK_WORKSPACE_CAP = 256 << 20       # bytes of similarities materialised at a time (rank_candidates cuts its rows into bands under it)
_INT_DTYPES = (torch.int64, torch.int32, torch.int16, torch.uint8, torch.int8)


class RankResult:
    """What ``rank_candidates`` returns, in the caller's row order: ``ids [rows, top_n]`` int64 item ids, ``positions [rows, top_n]`` int64
    indices into the row's candidate list, ``sims [rows, top_n]`` fp32 and ``counts [rows]`` int32 = min(len(candidates), top_n).  Slots
    from ``counts[r]`` on hold id -1, position -1, similarity -inf.  ``preds`` is the best id of every row."""
    __slots__ = ("ids", "positions", "sims", "counts")

    def __init__(self, ids, positions, sims, counts):
        self.ids, self.positions, self.sims, self.counts = ids, positions, sims, counts

    @property
    def preds(self) -> torch.Tensor:
        return self.ids[:, 0]


def _id_list(c, what: str) -> torch.Tensor:
    t = c if isinstance(c, torch.Tensor) else torch.as_tensor(list(c), dtype=torch.int64)
    if t.dtype not in _INT_DTYPES:
        raise TypeError(f"{what} must hold integer ids, got {t.dtype}")
    if t.dim() != 1:
        raise ValueError(f"{what} must be a 1-D list of ids, got shape {tuple(t.shape)}")
    return t.to(torch.int64)


def _candidate_sets(candidates, rows: int, table_rows: int):
    """The ragged candidate lists of ``rows`` rows as the kernels take them -> ``(flat, set_off, row_set, order)``: ``flat`` the int64 ids
    of the DISTINCT lists back to back (a CPU tensor unless a list lives on a device), ``set_off`` their ``nsets + 1`` offsets,
    ``row_set[r]`` the set of caller row r and ``order`` the caller rows sorted by set (stable), which is how the kernels want them.

    ``candidates``: one 1-D integer tensor or list per row, or the tuple ``(set_ids [rows], sets)`` with ``sets`` a dict or list of such
    lists.  Equal lists are found by identity first (a dataset hands the same per-category tensor to every row of the category) and, for
    lists on the CPU, by content second.  Ids outside [0, table_rows) raise IndexError, checked where the ids live: CPU ids on the CPU,
    device ids with one ``aminmax``."""
    if isinstance(candidates, tuple) and len(candidates) == 2 and (isinstance(candidates[1], dict) or (
            isinstance(candidates[1], (list, tuple)) and len(candidates[1]) > 0 and not isinstance(candidates[1][0], int))):
        set_ids, sets = candidates
        set_ids = set_ids.tolist() if isinstance(set_ids, torch.Tensor) else list(set_ids)
        try:
            per_row = [sets[k] for k in set_ids]
        except (KeyError, IndexError) as e:
            raise IndexError(f"set id {e.args[0]!r} names no candidate set") from e
    else:
        per_row = list(candidates)
    if len(per_row) != rows:
        raise ValueError(f"candidates holds {len(per_row)} lists for {rows} rows")
    uniq, by_identity, by_content, row_set = [], {}, {}, []
    for r, c in enumerate(per_row):
        s = by_identity.get(id(c))
        if s is None:
            t = _id_list(c, f"candidates of row {r}")
            key = (t.numel(), t.numpy().tobytes()) if t.device.type == "cpu" else None
            s = by_content.get(key) if key is not None else None
            if s is None:
                s = len(uniq)
                uniq.append(t)
                if key is not None:
                    by_content[key] = s
            by_identity[id(c)] = s
        row_set.append(s)
    set_off = [0]
    for t in uniq:
        set_off.append(set_off[-1] + t.numel())
    devs = [t.device for t in uniq if t.device.type != "cpu"]
    flat = torch.cat([t.to(devs[0]) for t in uniq]) if devs else (torch.cat(uniq) if uniq else torch.empty(0, dtype=torch.int64))
    if flat.numel():
        lo, hi = (int(v) for v in torch.aminmax(flat)) if devs else (int(flat.min()), int(flat.max()))
        if lo < 0 or hi >= table_rows:
            raise IndexError(f"candidate ids out of range [0, {table_rows}): min {lo}, max {hi}")
    order = sorted(range(rows), key=row_set.__getitem__)
    return flat, set_off, row_set, order


def _rank_bands(lens, cap_bytes: int):
    """Cut rows (their sets' lengths in kernel order) into bands ``(start, stop)`` whose similarity block -- rows x the band's longest set
    rounded up to 64, fp32 -- stays under ``cap_bytes``; a band holds at least one row."""
    bands, start, longest = [], 0, 0
    for r, n in enumerate(lens):
        ld = (max(longest, n, 1) + 63) // 64 * 64
        if r > start and (r - start + 1) * ld * 4 > cap_bytes:
            bands.append((start, r))
            start, ld = r, (max(n, 1) + 63) // 64 * 64
        longest = ld
    if len(lens) > start:
        bands.append((start, len(lens)))
    return bands


def embed_row_norms(x: torch.Tensor) -> torch.Tensor:
    """``|x_r|`` of a [rows, dim] fp32 device matrix (dim a multiple of 4): the table norms ``rank_candidates`` takes, computed once for
    many batches."""
    x = _device_rows(x, "embed_row_norms: x")
    if x.dim() != 2 or x.shape[1] % 4:
        raise ValueError(f"embed_row_norms needs [rows, dim] with dim a multiple of 4, got {tuple(x.shape)}")
    out = torch.empty((x.shape[0],), dtype=torch.float32, device=x.device)
    if x.shape[0]:
        with torch.cuda.device(x.device):
            _lib.call("dfh_embed_row_norms", _lib.ptr(x), _lib.ptr(out), x.shape[0], x.shape[1], _lib.stream_ptr())
    return out


@torch.no_grad()
def rank_candidates(gen: torch.Tensor, table: torch.Tensor, candidates, top_n: int, table_norms: Optional[torch.Tensor] = None,
                    workspace_cap: int = RANK_WORKSPACE_CAP) -> RankResult:
    """Every row of ``gen [rows, dim]`` ranked by cosine similarity against ITS OWN candidate list of rows of ``table [table_rows, dim]``;
    the best ``top_n`` (at most 128) kept in order -> ``RankResult``.  The ranking of ``clip_og_retrieval_given_data``
    (eval_utils.py:733-750) for all rows at once, candidate lists of any lengths (``_candidate_sets`` says which forms).

    Order: descending, a NaN above everything (``torch.topk``'s order), among equal values (-0.0 and +0.0, two NaNs) the lower position
    in the candidate list first.  A zero row gives NaN in its own similarities only.  The rows of one list share matrix tiles; the result
    of a row does not depend on the rows it is ranked with, on ``workspace_cap`` or on the order of the rows."""
    gen, table = _device_rows(gen, "rank_candidates: gen"), _device_rows(table, "rank_candidates: table")
    if gen.dim() != 2 or table.dim() != 2 or gen.shape[1] != table.shape[1] or gen.device != table.device or table.shape[0] < 1:
        raise ValueError(f"gen [rows, dim] and table [table_rows >= 1, dim] must share dim and device, got {tuple(gen.shape)} and {tuple(table.shape)}")
    rows, dim = gen.shape
    if dim % 4:
        raise ValueError(f"dim must be a multiple of 4 (the kernels read rows as float4), got {dim}")
    if not 1 <= int(top_n) <= RANK_NMAX:
        raise ValueError(f"top_n must be in 1 .. {RANK_NMAX}, got {top_n}")
    top_n, dev = int(top_n), gen.device
    flat, set_off, row_set, order = _candidate_sets(candidates, rows, table.shape[0])
    if table_norms is None:
        table_norms = embed_row_norms(table)
    elif table_norms.shape != (table.shape[0],) or table_norms.device != dev or table_norms.dtype != torch.float32:
        raise ValueError(f"table_norms must be embed_row_norms(table): fp32 [{table.shape[0]}] on {dev}")
    ids = torch.empty((rows, top_n), dtype=torch.int64, device=dev)
    pos, sims = torch.empty_like(ids), torch.empty((rows, top_n), dtype=torch.float32, device=dev)
    counts = torch.empty((rows,), dtype=torch.int32, device=dev)
    if rows == 0:
        return RankResult(ids, pos, sims, counts)
    flat = (flat if flat.numel() else torch.zeros(1, dtype=torch.int64)).to(dev).contiguous()
    sorted_rows = order != list(range(rows))
    order_t = torch.tensor(order, dtype=torch.int64, device=dev) if sorted_rows else None
    gen_s = gen.index_select(0, order_t) if sorted_rows else gen            # rows grouped by set: a copy of rows, no arithmetic
    gen_norms = embed_row_norms(gen_s)
    row_set_s = [row_set[r] for r in order]
    lens = [set_off[s + 1] - set_off[s] for s in row_set_s]
    bands = _rank_bands(lens, int(workspace_cap))
    lib = _lib.raw()
    need = max(lib.dfh_embed_rank_workspace_bytes(b - a, max(lens[a:b]), top_n) for a, b in bands)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    c_off = (C.c_int64 * len(set_off))(*set_off)
    out = (ids, pos, sims, counts) if not sorted_rows else (torch.empty_like(ids), torch.empty_like(pos), torch.empty_like(sims), torch.empty_like(counts))
    with torch.cuda.device(dev):
        for a, b in bands:
            c_rows = (C.c_int * (b - a))(*row_set_s[a:b])
            _lib.call("dfh_embed_rank", _lib.ptr(gen_s[a:]), _lib.ptr(gen_norms[a:]), b - a, dim, _lib.ptr(table), _lib.ptr(table_norms),
                      table.shape[0], _lib.ptr(flat), c_off, len(set_off) - 1, c_rows, top_n, _lib.ptr(ws), ws.numel(), _lib.ptr(out[0][a:]),
                      _lib.ptr(out[1][a:]), _lib.ptr(out[2][a:]), _lib.ptr(out[3][a:]), _lib.stream_ptr())
    if sorted_rows:                                                        # back to the caller's row order
        for dst, src in zip((ids, pos, sims, counts), out):
            dst.index_copy_(0, order_t, src)
    return RankResult(ids, pos, sims, counts)


@torch.no_grad()
def recall_at(ranked: RankResult, grds, cutoffs):
    """``(hit_pos [rows] int32, hits)``: the first rank at which row r's list holds ``grds[r]`` (-1: nowhere), and per cutoff N the number
    of rows with ``0 <= hit_pos < N`` -- the reference's ``grd in topN_iids[:N]`` (eval_utils.py:754-762) -- as Python ints."""
    dev, rows = ranked.ids.device, ranked.ids.shape[0]
    grd = (grds if isinstance(grds, torch.Tensor) else torch.as_tensor([int(g) for g in grds], dtype=torch.int64)).reshape(-1)
    if grd.numel() != rows or grd.dtype not in _INT_DTYPES:
        raise ValueError(f"grds must hold one integer id per row ({rows}), got {grd.numel()} of {grd.dtype}")
    cuts = [int(c) for c in cutoffs]
    if len(cuts) > 64:
        raise ValueError(f"at most 64 cutoffs, got {len(cuts)}")
    grd = grd.to(device=dev, dtype=torch.int64).contiguous()
    hit_pos = torch.empty((rows,), dtype=torch.int32, device=dev)
    hits = torch.zeros((len(cuts),), dtype=torch.int64, device=dev)
    if rows:
        cut_t = torch.tensor(cuts, dtype=torch.int32, device=dev) if cuts else None
        with torch.cuda.device(dev):
            _lib.call("dfh_embed_recall", _lib.ptr(ranked.ids), _lib.ptr(ranked.counts), rows, ranked.ids.shape[1], _lib.ptr(grd), _lib.ptr(cut_t),
                      len(cuts), _lib.ptr(hit_pos), _lib.ptr(hits if cuts else None), _lib.stream_ptr())
    return hit_pos, hits.tolist()


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
        """(sims [rows, K], preds [rows]) of ``calculate_clip_retrieval_acc_given_data2`` (eval_utils.py:702-715): K candidates a row, the
        best one.  The ranking of ``clip_og_retrieval_given_data`` (:733-750) -- a whole category per row, the best 100 in order -- is
        ``grounding_retrieval`` below."""
        _require_cosine(similarity_func)
        return candidate_cosine(self.image_model.encode_image(images), cnn_features, candidates)

    @torch.no_grad()
    def grounding_retrieval_from_features(self, gen_feats: torch.Tensor, cnn_features: torch.Tensor, candidates, topN=(10, 20, 50, 100),
                                          grds=None, table_norms: Optional[torch.Tensor] = None):
        """``grounding_retrieval`` for a caller that holds the generated images' embeddings ``[rows, dim]`` already."""
        cuts = [int(n) for n in topN]
        if not cuts or any(n < 1 for n in cuts) or sorted(cuts) != cuts:
            raise ValueError(f"topN must be ascending positive cutoffs, got {topN}")
        ranked = rank_candidates(gen_feats, cnn_features, candidates, cuts[-1], table_norms)
        all_recall = None
        if grds is not None:
            _, hits = recall_at(ranked, grds, cuts)
            all_recall = [h / ranked.ids.shape[0] for h in hits]
        return ranked.preds, all_recall, ranked

    @torch.no_grad()
    def grounding_retrieval(self, images, cnn_features: torch.Tensor, candidates, topN=(10, 20, 50, 100), grds=None, batch_size: int = 200,
                            table_norms: Optional[torch.Tensor] = None, device=None):
        """``clip_og_retrieval_given_data`` (eval_utils.py:725-767) for all images at once: ``encode_image`` in batches of ``batch_size``,
        then ONE ranking of every row against its own candidate list at ``topN[-1]`` (at most 128) -> ``(preds [rows], all_recall,
        ranked)``: the best id of each row (the "grounded" item), recall@N per cutoff as floats (None without ``grds``) and the
        ``RankResult``.  ``images``: a tensor of preprocessed pixels or a list of per-image tensors, moved batch by batch to ``device``
        (default: the image model's); ``candidates``: see ``rank_candidates``."""
        dev = device if device is not None else getattr(self.image_model, "device", None)
        feats = torch.cat([self.image_model.encode_image(b if dev is None else b.to(dev)) for b in _image_batches(images, batch_size, "images")])
        return self.grounding_retrieval_from_features(feats, cnn_features, candidates, topN, grds, table_norms)


@torch.no_grad()
def clip_og_retrieval_given_data(gen4eval, grds, cnn_features, batch_size, topN, device=None, num_workers=1, similarity_func="cosine", *,
                                 clip: CLIPScore):
    """The reference's function under its own signature and return ``(preds, all_recall)`` (eval_utils.py:725-767).  ``gen4eval[i]`` is
    ``(image, candidates)`` as ``FashionRetrievalDataset`` yields them; ``clip`` is the ``CLIPScore`` to use (the reference builds one
    from OpenCLIP weights on every call).  ``num_workers`` is accepted and unused: nothing is loaded here."""
    _require_cosine(similarity_func)
    items = [gen4eval[i] for i in range(len(gen4eval))]
    if not items:
        raise ValueError("gen4eval holds no image")
    if device is not None:
        cnn_features = cnn_features.to(device)
    preds, all_recall, _ = clip.grounding_retrieval([it[0] for it in items], cnn_features, [it[1] for it in items], topN, grds, batch_size,
                                                    device=device)
    return preds, all_recall


clip_gor_retrieval_given_data = clip_og_retrieval_given_data      # the name Evaluation/evaluate_grounding_gor.py:255 calls


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

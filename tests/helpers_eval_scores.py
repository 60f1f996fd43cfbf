"""Case tables shared by the three fixture scripts of DESIGN.md row f6 (tests/golden/make_golden_clip_text_proj.py,
make_golden_compat.py, make_golden_eval_scores.py), tests/test_eval_scores_cpu.py and tests/test_gpu_eval_scores.py.  Weights and inputs
are regenerated from the seeds on every box (CPU generator: the same tensors everywhere); the fixtures hold the REAL classes' fp64
outputs (stored as fp32), the distance of their own fp32 run from those (``ref_*``) and a checksum of the inputs they were computed
from."""
import dataclasses
import os
from itertools import combinations

import numpy as np
import torch

from oracle import clip_ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def rel(a: torch.Tensor, b: torch.Tensor) -> float:
    return float((a.double() - b.double()).norm() / b.double().norm())


def load_fixture(stem: str):
    return dict(np.load(os.path.join(GOLDEN, stem + ".npz")))


def fixture_path(stem: str) -> str:
    return os.path.join(GOLDEN, stem + ".npz")


def _sums(tensors) -> np.ndarray:
    return np.array([float(t.double().sum()) for t in tensors] + [float(t.double().abs().sum()) for t in tensors])


# ------------------------------------------------------------------ text tower with projection
OPENCLIP_H_TEXT = clip_ref.CLIPTextConfig(hidden_size=1024, intermediate_size=4096, num_hidden_layers=24, num_attention_heads=16,
                                          hidden_act="gelu", pad_token_id=0)          # OpenCLIP ViT-H/14 text tower, all 24 layers

# name -> (text config, projection_dim, weight seed, sequence length, eos position of every row, full size)
TEXT_CASES = {
    "tiny_quickgelu": (clip_ref.TINY_CLIP, 32, 31, 77, (0, 76, 1, 40, 75), False),           # eos_token_id = 2: the argmax rule
    "tiny_gelu_eos": (clip_ref.TINY_CLIP_GELU, 48, 32, 77, (0, 76, 33, 5), False),           # in-vocabulary eos, twice in a row: first-eos rule
    "tiny_short_seq": (clip_ref.TINY_CLIP, 32, 33, 5, (0, 4, 2, 1), False),
    "openclip_h": (OPENCLIP_H_TEXT, 1024, 34, 77, (0, 76, 37), True),
}
TEXT_TINY = [n for n, c in TEXT_CASES.items() if not c[5]]
# token rows of the full-size case the fixture keeps: both ends, the 64-row tile edge of the linears, around the pooled positions
FULL_SIZE_ROWS = [0, 1, 31, 32, 37, 63, 64, 65, 75, 76]


def text_kwargs(cfg, projection_dim) -> dict:
    return dict(dataclasses.asdict(cfg), projection_dim=projection_dim)


def text_params(cfg, projection_dim, seed):
    """The tower's seeded weights (oracle.clip_ref.init_params) plus ``text_projection.weight`` from a generator of its own."""
    params = clip_ref.init_params(cfg, seed)
    g = torch.Generator().manual_seed(seed + 500)
    params["text_projection.weight"] = torch.randn((projection_dim, cfg.hidden_size), generator=g) * (0.7 / cfg.hidden_size ** 0.5)
    return params


def text_ids(cfg, T, eos_positions, seed) -> torch.Tensor:
    """[bos, words, eos, pad ...] rows with the eos at a chosen index of every row (index 0: the row starts with it).  The tokenizer's
    eos is the highest id under the argmax rule; under the first-eos rule it is written twice in a row where there is room."""
    g = torch.Generator().manual_seed(seed)
    eos = cfg.vocab_size - 1 if cfg.eos_token_id == 2 else cfg.eos_token_id
    words_hi = min(cfg.bos_token_id, eos, cfg.vocab_size - 2)
    ids = torch.full((len(eos_positions), T), cfg.pad_token_id, dtype=torch.long)
    for b, pos in enumerate(eos_positions):
        if pos > 0:
            ids[b, 0] = cfg.bos_token_id
            ids[b, 1:pos] = torch.randint(1, words_hi, (pos - 1,), generator=g)
        ids[b, pos] = eos
        if cfg.eos_token_id != 2 and pos + 1 < T:
            ids[b, pos + 1] = eos
    return ids


def text_case_inputs(name):
    cfg, pd, seed, T, pos, _ = TEXT_CASES[name]
    return cfg, pd, text_params(cfg, pd, seed), text_ids(cfg, T, pos, seed + 1000)


def text_checksum(params, ids) -> np.ndarray:
    keys = sorted(params)
    return np.concatenate([_sums([params[k] for k in (keys[0], keys[len(keys) // 2], keys[-1])]), [float(ids.double().sum())]])


def text_rows_of(fx, t: torch.Tensor) -> torch.Tensor:
    return t[:, torch.from_numpy(fx["rows"]).long()] if "rows" in fx else t


# ------------------------------------------------------------------ compatibility scorer
# name -> (outfits, items, cnn_feat_dim, seed): one outfit, more outfit rows than a 64-row tile (65 x 4 = 260 item rows, 390 pair rows),
# odd counts, five items (10 pairs), two items (one pair) at a narrow feature dim
COMPAT_CASES = {
    "one_outfit": (1, 4, 1024, 41),
    "tile_edge": (65, 4, 1024, 42),
    "three_items": (7, 3, 1024, 43),
    "five_items": (6, 5, 1024, 44),
    "two_items_narrow": (9, 2, 64, 45),
    "ragged_k": (5, 3, 44, 46),          # feat_dim 44: one full and one ragged 32-wide k-tile in feat_layer's GEMM
}
COMPAT_REAL_ROWS, COMPAT_GEN_ROWS = 300, 40


def compat_param_shapes(dim):
    out = [("feat_layer.weight", (1024, dim)), ("feat_layer.bias", (1024,))]
    for stack, dims, tail in (("emb_layer", [2048, 512, 512, 256, 256], None), ("eval_layer", [256, 128, 128, 32], 1)):
        for l, (k, n) in enumerate(zip(dims[:-1], dims[1:])):
            out += [(f"{stack}.{4 * l}.weight", (n, k)), (f"{stack}.{4 * l}.bias", (n,)), (f"{stack}.{4 * l + 1}.weight", (n,)),
                    (f"{stack}.{4 * l + 1}.bias", (n,))]
        if tail:
            out += [(f"{stack}.{4 * (len(dims) - 1)}.weight", (tail, dims[-1])), (f"{stack}.{4 * (len(dims) - 1)}.bias", (tail,))]
    return out


def compat_params(dim, seed):
    """Linears: randn at xavier-normal scale sqrt(2 / (fan_in + fan_out)); LayerNorm weights 1 + 0.1 randn; every bias 0.1 randn."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name, shape in compat_param_shapes(dim):
        r = torch.randn(shape, generator=g)
        if len(shape) == 2:
            out[name] = r * (2.0 / (shape[0] + shape[1])) ** 0.5
        elif name.endswith("weight"):
            out[name] = 1.0 + 0.1 * r
        else:
            out[name] = 0.1 * r
    return out


def compat_case_inputs(name):
    """-> (params, feats_real [300, dim], feats_gen [40, dim], olists [outfits, items] int64).  The olists mix real ids (> 0) with generated
    ones (<= 0); outfit 0 opens with id 0 (= feats_gen[0]) and holds the last row of either table."""
    O, items, dim, seed = COMPAT_CASES[name]
    g = torch.Generator().manual_seed(seed + 1000)
    real = torch.randn((COMPAT_REAL_ROWS, dim), generator=g)
    gen = torch.randn((COMPAT_GEN_ROWS, dim), generator=g)
    ol = torch.randint(1, COMPAT_REAL_ROWS, (O, items), generator=g)
    neg = -torch.randint(0, COMPAT_GEN_ROWS, (O, items), generator=g)
    ol = torch.where(torch.rand((O, items), generator=g) < 0.4, neg, ol)
    ol[0, 0] = 0
    ol[0, 1] = -(COMPAT_GEN_ROWS - 1)
    if items > 2:
        ol[0, 2] = COMPAT_REAL_ROWS - 1
    return compat_params(dim, seed), real, gen, ol


def compat_checksum(params, real, gen, ol) -> np.ndarray:
    keys = sorted(params)
    return np.concatenate([_sums([params[keys[0]], params[keys[-1]], real, gen]), [float(ol.double().sum()), float(ol.double().abs().sum())]])


def compat_gather(real, gen, ol) -> torch.Tensor:
    """The loop of evaluate_compatibility (eval_utils.py:575-584) as indexing: [outfits, items, dim]."""
    return torch.stack([torch.stack([gen[-int(i)] if int(i) <= 0 else real[int(i)] for i in row]) for row in ol])


def pair_order(items):
    return [list(c) for c in combinations(range(items), 2)]


# ------------------------------------------------------------------ pair scores and retrieval
PAIR_CASES = {"one_row": (1, 1024, 51), "tile_edge": (65, 1024, 52), "narrow": (130, 20, 53), "clip_l": (5, 768, 54)}      # (rows, dim, seed)
RETRIEVAL_TABLE_ROWS, RETRIEVAL_DIM, RETRIEVAL_ROWS = 1200, 1024, 9
RETRIEVAL_CASES = {"k1": (1, 61), "k5": (5, 62), "k1000": (1000, 63)}                                                   # (K, seed)
TIE_ROW = 3                 # in this row candidate 1 repeats candidate 0's id, and the rest are made worse than both


def pair_inputs(name):
    """Embedding-like rows: a shared direction plus noise, so the scores spread over tens of points instead of sitting at 0."""
    rows, dim, seed = PAIR_CASES[name]
    g = torch.Generator().manual_seed(seed)
    common = torch.randn((rows, dim), generator=g)
    a = common + 0.8 * torch.randn((rows, dim), generator=g)
    b = 0.7 * common + torch.randn((rows, dim), generator=g)
    return a * 3.0, b * 0.5


def retrieval_inputs(name):
    """-> (gen [9, 1024], table [1200, 1024], cand [9, K]).  Candidate 2 % K of every row is pulled towards the row's embedding, so the
    best candidate stands clear of the second best; row TIE_ROW repeats its first id."""
    K, seed = RETRIEVAL_CASES[name]
    g = torch.Generator().manual_seed(seed)
    table = torch.randn((RETRIEVAL_TABLE_ROWS, RETRIEVAL_DIM), generator=g)
    cand = torch.stack([torch.randperm(RETRIEVAL_TABLE_ROWS, generator=g)[:K] for _ in range(RETRIEVAL_ROWS)])
    gen = torch.randn((RETRIEVAL_ROWS, RETRIEVAL_DIM), generator=g)
    for r in range(RETRIEVAL_ROWS):
        gen[r] += 0.5 * table[cand[r, 2 % K]]
    if K > 1:
        gen[TIE_ROW] = torch.randn((RETRIEVAL_DIM,), generator=g) + 0.5 * table[cand[TIE_ROW, 0]]
        cand[TIE_ROW, 1] = cand[TIE_ROW, 0]
    return gen, table, cand


def scores_checksum(*tensors) -> np.ndarray:
    return _sums(tensors)


def pair_bound(dim: int, scale: float) -> float:
    """Absolute error of one cosine at fp32: per lane a run of dim / 64 fused multiply-adds, a 6-step wave tree, and the roundings of
    two norms, one divide and one scale -- (dim / 64 + 16) units of 2^-24 on a value of at most 1, times the scale."""
    return scale * (dim / 64 + 16) * 2.0 ** -24

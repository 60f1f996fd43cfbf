"""difashion_amd -- MI355X (gfx950) native implementation of DiFashion's parallel conditional
denoising U-Net path, behind the diffusers UNet2DConditionModel / DDIMScheduler call signatures.

Compute lives in ``csrc/libdifashion_hip.so`` (C ABI: ``include/difashion_hip.h``); this package is
the Python host side mirroring the reference interface.  ``DFH_STORAGE=fp16`` / ``set_storage("fp16")`` selects, per
process and before first use, the fp16-storage build of the same kernels (``libdifashion_hip_f16.so``, inference only).  Importing the package does not need a GPU;
running any op does, and fails loudly if the library was not built (no CPU fallback).
"""
from . import _lib, data, evalio, prompts
from ._lib import DfhError, set_storage, storage
from .mutual import MutualEncoder
from .pipeline import OutfitSampler, guidance_plan, sample_outfits, sampling_tables, train_forward, training_tables
from .schedulers import DDIMScheduler, DPMSolverMultistepScheduler, PNDMScheduler
from .training import AdamW8bit, EMAModel, FusedAdamW, clip_grad_norm_, train_step
from .unet import UNet2DConditionModel, UNet2DConditionOutput
from .vae import AutoencoderKL
from .clip import CLIPTextModel, CLIPTextModelOutput, CLIPTextModelWithProjection
from .clip_vision import CLIPVisionModelOutput, CLIPVisionModelWithProjection
from .image_processor import CLIPImageProcessor
from .jpeg import jpeg_quant_tables, jpeg_roundtrip
from .evalscores import (CLIPScore, CompatibilityEvaluator, FashionEvaluator, candidate_cosine, extract_image_features, lpips_given_data,
                         lpips_retrieval, pair_cosine)
from .evalscores import (RankResult, clip_gor_retrieval_given_data, clip_og_retrieval_given_data, embed_row_norms, rank_candidates,
                         recall_at)
from .lpips import LPIPS
from .evalscores import (activation_statistics, fid_given_data, frechet_distance, inception_rows, inception_score_from_probs,
                         inception_score_given_data)
from .inception import FIDInceptionV3, InceptionV3
from .difashion import DiFashion
from .itemstore import HistoryTable, ItemLatentStore

__all__ = [
    "DfhError", "set_storage", "storage", "UNet2DConditionModel", "UNet2DConditionOutput", "DDIMScheduler", "PNDMScheduler",
    "DPMSolverMultistepScheduler",
    "MutualEncoder", "OutfitSampler", "sample_outfits", "train_forward", "guidance_plan", "sampling_tables", "training_tables",
    "FusedAdamW", "AdamW8bit", "EMAModel", "clip_grad_norm_", "train_step", "AutoencoderKL", "CLIPTextModel", "DiFashion",
    "CLIPVisionModelWithProjection", "CLIPVisionModelOutput", "CLIPTextModelWithProjection", "CLIPTextModelOutput", "CLIPScore",
    "CompatibilityEvaluator", "FashionEvaluator", "pair_cosine", "candidate_cosine", "CLIPImageProcessor", "extract_image_features",
    "LPIPS", "lpips_given_data", "lpips_retrieval",
    "RankResult", "rank_candidates", "embed_row_norms", "recall_at", "clip_og_retrieval_given_data", "clip_gor_retrieval_given_data",
    "FIDInceptionV3", "InceptionV3", "activation_statistics", "frechet_distance", "fid_given_data", "inception_rows",
    "inception_score_from_probs", "inception_score_given_data",
    "ItemLatentStore", "HistoryTable",
    "jpeg_roundtrip", "jpeg_quant_tables",
]

"""ctypes binding of libdifashion_hip.so (C ABI: include/difashion_hip.h).

There is NO fallback: if the HIP library is missing, import of the compute path raises.  PyTorch is
used on the host side only for device memory, streams and torch.distributed (plumbing).
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
# The 16-bit storage format of activations and packed weights is a property of the PROCESS: each format is a build of its own
# of the kernel library (csrc/Makefile), chosen before the library is first loaded -- DFH_STORAGE=fp16 in the environment or
# set_storage("fp16"); unset means bf16.  The fp16 library is inference only (training and the fp8 legs refuse there).
_LIB_NAMES = {"bf16": "libdifashion_hip.so", "fp16": "libdifashion_hip_f16.so"}


def _env_storage() -> str:
    v = (os.environ.get("DFH_STORAGE") or "bf16").strip().lower()
    if v not in _LIB_NAMES:
        raise ValueError(f"DFH_STORAGE={v!r}: the storage format is 'bf16' (default) or 'fp16'")
    return v


_STORAGE = _env_storage()
# DFH_LIB=<path>: load another build of the library (same-box A/B probes); the product path never sets it
LIB_PATH = os.environ.get("DFH_LIB") or os.path.join(CSRC, _LIB_NAMES[_STORAGE])
HEADER = os.path.join(os.path.dirname(_HERE), "include", "difashion_hip.h")

DFH_MAX_BLOCKS = 4


class DfhError(RuntimeError):
    pass


class UNetConfigC(C.Structure):
    _fields_ = [
        ("sample_size", C.c_int), ("in_channels", C.c_int), ("out_channels", C.c_int), ("num_blocks", C.c_int),
        ("block_out_channels", C.c_int * DFH_MAX_BLOCKS), ("layers_per_block", C.c_int),
        ("cross_attention_dim", C.c_int), ("num_heads", C.c_int * DFH_MAX_BLOCKS),
        ("down_attn", C.c_int * DFH_MAX_BLOCKS), ("use_linear_projection", C.c_int),
        ("norm_num_groups", C.c_int), ("norm_eps", C.c_float), ("text_len", C.c_int),
    ]


class VAEConfigC(C.Structure):
    _fields_ = [("in_channels", C.c_int), ("out_channels", C.c_int), ("latent_channels", C.c_int), ("num_blocks", C.c_int),
                ("block_out_channels", C.c_int * DFH_MAX_BLOCKS), ("layers_per_block", C.c_int), ("norm_num_groups", C.c_int)]


class CLIPConfigC(C.Structure):
    _fields_ = [("vocab_size", C.c_int), ("hidden_size", C.c_int), ("intermediate_size", C.c_int), ("num_hidden_layers", C.c_int),
                ("num_attention_heads", C.c_int), ("max_position_embeddings", C.c_int), ("hidden_act", C.c_int),
                ("layer_norm_eps", C.c_float)]


class CLIPVisionConfigC(C.Structure):
    _fields_ = [("hidden_size", C.c_int), ("intermediate_size", C.c_int), ("num_hidden_layers", C.c_int), ("num_attention_heads", C.c_int),
                ("image_size", C.c_int), ("patch_size", C.c_int), ("num_channels", C.c_int), ("projection_dim", C.c_int),
                ("hidden_act", C.c_int), ("layer_norm_eps", C.c_float)]


CLIPVH_MAX_LAUNCHES, CLIPVH_MAX_REGIONS = 8, 16


class CLIPVHalfLaunchC(C.Structure):
    _fields_ = [("name", C.c_char * 16)] + \
               [(n, C.c_int) for n in ("M", "N", "K", "lda", "ldw", "ld_out", "n_split", "ld_out2", "rows_per_b", "act", "resid", "per_layer",
                                       "a_region", "out_region", "out2_region")]


class CLIPVHalfRegionC(C.Structure):
    _fields_ = [("name", C.c_char * 16), ("offset", C.c_size_t), ("bytes", C.c_size_t)]


class CLIPVHalfPlanC(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("batch", "tokens", "hidden", "intermediate", "heads", "head_dim", "layers", "projection_dim",
                                       "patch_k", "patch_k_padded", "rows", "patch_rows", "ldvt", "attention_x32", "num_launches", "num_regions")] + \
               [("workspace_bytes", C.c_size_t), ("packed_bytes", C.c_size_t), ("launches", CLIPVHalfLaunchC * CLIPVH_MAX_LAUNCHES),
                ("regions", CLIPVHalfRegionC * CLIPVH_MAX_REGIONS)]


class CLIPTHalfPlanC(C.Structure):
    """dfh_cliph_plan_info: the 16-bit text tower's plan (launches and regions in the image tower's record types)."""
    _fields_ = [(n, C.c_int) for n in ("batch", "tokens", "hidden", "intermediate", "heads", "head_dim", "layers", "rows",
                                       "attention_lds_bytes", "num_launches", "num_regions")] + \
               [("workspace_bytes", C.c_size_t), ("packed_bytes", C.c_size_t), ("launches", CLIPVHalfLaunchC * CLIPVH_MAX_LAUNCHES),
                ("regions", CLIPVHalfRegionC * CLIPVH_MAX_REGIONS)]


class ImgProcConfigC(C.Structure):
    _fields_ = [("shortest_edge", C.c_int), ("crop_height", C.c_int), ("crop_width", C.c_int), ("resample", C.c_int)]


class LpipsConfigC(C.Structure):
    _fields_ = [("net", C.c_int)]


class IncepConfigC(C.Structure):
    _fields_ = [("variant", C.c_int), ("num_classes", C.c_int), ("resize_input", C.c_int), ("normalize_input", C.c_int), ("block_mask", C.c_int)]


class IncepLaunchC(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("kind", "conv", "pool_mode", "block", "KH", "KW", "stride", "padH", "padW", "Hin", "Win", "Cin", "Hout", "Wout",
                                       "Cout", "ldc", "offset", "src_region", "dst_region")] + \
               [(n, C.c_size_t) for n in ("src_off", "src_floats", "dst_off", "dst_floats")] + [("name", C.c_char * 48)]


class GemmDesc(C.Structure):
    _fields_ = [
        ("conv_src", C.c_void_p), ("conv_c", C.c_int), ("conv", C.c_int),
        ("batch", C.c_int), ("Hin", C.c_int), ("Win", C.c_int), ("stride", C.c_int), ("upsample", C.c_int),
        ("a0", C.c_void_p), ("a0_c", C.c_int), ("a1", C.c_void_p), ("a1_c", C.c_int),
        ("W", C.c_void_p), ("ldw", C.c_int),
        ("M", C.c_int), ("N", C.c_int),
        ("bias", C.c_void_p),
        ("rowvec", C.c_void_p), ("rv_ld", C.c_int), ("rv_off", C.c_int), ("rows_per_b", C.c_int),
        ("resid", C.c_void_p), ("ld_res", C.c_int),
        ("act", C.c_int),
        ("out", C.c_void_p), ("ld_out", C.c_int), ("out_mode", C.c_int),
        ("partial", C.c_void_p), ("partial_floats", C.c_size_t),
        ("zero_page", C.c_void_p),
        ("force_tile", C.c_int), ("force_split", C.c_int), ("force_order", C.c_int),
        ("gstat", C.c_void_p), ("gstat_cpg", C.c_int), ("gstat_hw", C.c_int),
        ("w_img_stride", C.c_size_t),
    ]


class GemmPlanExtra(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("nbatch", "phase2x", "w_blocked", "n_split", "want_rowstat", "ln_cnt", "pre_out")]


class GemmPlanInfo(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("kernel", "tile", "bm", "bn", "stages", "lean", "wide", "split", "n_major", "tm_xm", "tm_gm",
                                       "gstat_rows", "rowstat_bn", "census")] + [("line", C.c_char * 512)]


class Fp8GemmDesc(C.Structure):
    _fields_ = [
        ("A", C.c_void_p), ("lda", C.c_int),
        ("sA", C.c_void_p), ("sa_div", C.c_int), ("sa_mul", C.c_float),
        ("sx", C.c_void_p),
        ("W", C.c_void_p), ("sW", C.c_void_p),
        ("M", C.c_int), ("N", C.c_int), ("K", C.c_int),
        ("bias", C.c_void_p), ("resid", C.c_void_p), ("ld_res", C.c_int), ("act", C.c_int),
        ("out", C.c_void_p), ("ld_out", C.c_int), ("out_mode", C.c_int), ("out_sx", C.c_void_p), ("rows_per_b", C.c_int), ("amax", C.c_void_p),
        ("zero_page", C.c_void_p),
    ]


class StepCoef(C.Structure):
    _fields_ = [("kind", C.c_int), ("vpred", C.c_int), ("sqrt_a_t", C.c_float), ("sqrt_b_t", C.c_float),
                ("sqrt_a_prev", C.c_float), ("dir_coef", C.c_float), ("std_dev", C.c_float)]


class MultistepCoef(C.Structure):
    """dfh_multistep_coef: conversion, kind and scalar coefficients of one dfh_cfg_multistep call."""
    _fields_ = [("conv", C.c_int), ("kind", C.c_int), ("terms", C.c_int), ("c0", C.c_float), ("c1", C.c_float), ("w", C.c_float * 4),
                ("cx", C.c_float), ("ce", C.c_float), ("cd0", C.c_float), ("cr", C.c_float), ("cd1", C.c_float)]


class ProfClass(C.Structure):
    _fields_ = [("name", C.c_char * 32), ("launches", C.c_int), ("ms", C.c_double), ("flops", C.c_double),
                ("bytes", C.c_double)]


_vp, _i, _f, _sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t

# name -> (restype, argtypes); status-returning functions are wrapped to raise DfhError
SIGNATURES = {
    "dfh_abi_version": (_i, []),
    "dfh_last_error": (C.c_char_p, []),
    "dfh_build_info": (C.c_char_p, []),
    "dfh_prof_begin": (_i, []),
    "dfh_prof_end": (_i, [C.POINTER(ProfClass), _i]),
    "dfh_census_reset": (None, []),
    "dfh_census_count": (_i, []),
    "dfh_census_name": (C.c_char_p, [_i]),
    "dfh_census_get": (C.c_long, [_i]),
    "dfh_walk_switches": (_sz, [C.c_char_p, _sz]),
    "dfh_unet_create": (_i, [C.POINTER(UNetConfigC), C.POINTER(_vp)]),
    "dfh_unet_destroy": (None, [_vp]),
    "dfh_unet_num_params": (_i, [_vp]),
    "dfh_unet_param_name": (C.c_char_p, [_vp, _i]),
    "dfh_unet_param_ndim": (_i, [_vp, _i]),
    "dfh_unet_param_dim": (_i, [_vp, _i, _i]),
    "dfh_unet_arena16_bytes": (_sz, [_vp]),
    "dfh_unet_arena32_bytes": (_sz, [_vp]),
    "dfh_unet_workspace_bytes": (_sz, [_vp, _i]),
    "dfh_unet_bind": (_i, [_vp, _vp, _vp, _vp, _sz, _i]),
    "dfh_unet_pack": (_i, [_vp, C.POINTER(_vp), _i, _vp]),
    "dfh_unet_forward": (_i, [_vp, _vp, _i, _vp, _vp, _i, _vp, _i, _vp]),
    "dfh_unet_run_cache_bytes": (_sz, [_vp, _i, _i]),
    "dfh_unet_run_cache": (_i, [_vp, _vp, _i, _i, _vp, _i, _vp, _sz, _vp]),
    "dfh_unet_set_dup_tail": (_i, [_vp, _i]),
    "dfh_unet_forward_cached": (_i, [_vp, _vp, _i, _vp, _i, _i, _i, _vp, _vp]),
    "dfh_unet_debug_tap": (_i, [_vp, C.c_char_p, _vp, _sz, _vp]),
    "dfh_clip_create": (_i, [C.POINTER(CLIPConfigC), C.POINTER(_vp)]),
    "dfh_clip_destroy": (None, [_vp]),
    "dfh_clip_num_params": (_i, [_vp]),
    "dfh_clip_param_name": (C.c_char_p, [_vp, _i]),
    "dfh_clip_param_ndim": (_i, [_vp, _i]),
    "dfh_clip_param_dim": (_i, [_vp, _i, _i]),
    "dfh_clip_workspace_bytes": (_sz, [_vp, _i, _i]),
    "dfh_clip_encode": (_i, [_vp, C.POINTER(_vp), _i, _vp, _vp, _vp, _i, _vp, _vp, _sz, _i, _i, _vp]),
    "dfh_clip_text_embeds": (_i, [_vp, C.POINTER(_vp), _i, _vp, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _sz, _i, _i, _vp]),
    "dfh_embed_pair_cosine": (_i, [_vp, _vp, _vp, _i, _i, _f, _vp]),
    "dfh_embed_candidates": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _vp]),
    "dfh_embed_row_norms": (_i, [_vp, _vp, _i, _i, _vp]),
    "dfh_embed_rank_workspace_bytes": (_sz, [_i, C.c_long, _i]),
    "dfh_embed_rank": (_i, [_vp, _vp, _i, _i, _vp, _vp, _i, _vp, _vp, _i, _vp, _i, _vp, _sz, _vp, _vp, _vp, _vp, _vp]),
    "dfh_embed_recall": (_i, [_vp, _vp, _i, _i, _vp, _vp, _i, _vp, _vp, _vp]),
    "dfh_item_gather": (_i, [_vp, C.c_long, C.c_long, _i, _vp, C.c_long, _vp, _f, _vp, _vp]),
    "dfh_history_rows": (_i, [_vp, C.c_long, C.c_long, _i, _vp, _vp, _vp, C.c_long, _vp, _f, _vp, _vp]),
    "dfh_compat_workspace_bytes": (_sz, [_i, _i, _i]),
    "dfh_compat_score": (_i, [C.POINTER(_vp), _i, _i, _vp, _i, _vp, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "dfh_compat_pred_score": (_i, [C.POINTER(_vp), _i, _vp, _i, _vp, _vp, _vp, _sz, _vp]),
    "dfh_clipv_create": (_i, [C.POINTER(CLIPVisionConfigC), C.POINTER(_vp)]),
    "dfh_clipv_destroy": (None, [_vp]),
    "dfh_clipv_num_params": (_i, [_vp]),
    "dfh_clipv_param_name": (C.c_char_p, [_vp, _i]),
    "dfh_clipv_param_ndim": (_i, [_vp, _i]),
    "dfh_clipv_param_dim": (_i, [_vp, _i, _i]),
    "dfh_clipv_workspace_bytes": (_sz, [_vp, _i]),
    "dfh_clipv_encode": (_i, [_vp, C.POINTER(_vp), _i, _vp, _i, _vp, _vp, _vp, C.POINTER(_vp), _vp, _sz, _vp]),
    "dfh_clipv_attention": (_i, [_vp, _vp, _i, _i, _i, _i, _f, _vp]),
    "dfh_clipvh_plan": (_i, [_vp, _i, C.POINTER(CLIPVHalfPlanC)]),
    "dfh_clipvh_packed_bytes": (_sz, [_vp]),
    "dfh_clipvh_pack": (_i, [_vp, C.POINTER(_vp), _i, _vp, _vp]),
    "dfh_clipvh_workspace_bytes": (_sz, [_vp, _i]),
    "dfh_clipvh_encode": (_i, [_vp, C.POINTER(_vp), _i, _vp, _vp, _i, _i, _vp, _vp, _vp, C.POINTER(_vp), _vp, _sz, _vp]),
    "dfh_cliph_plan": (_i, [_vp, _i, _i, C.POINTER(CLIPTHalfPlanC)]),
    "dfh_cliph_packed_bytes": (_sz, [_vp]),
    "dfh_cliph_pack": (_i, [_vp, C.POINTER(_vp), _i, _vp, _vp]),
    "dfh_cliph_workspace_bytes": (_sz, [_vp, _i, _i]),
    "dfh_cliph_encode": (_i, [_vp, C.POINTER(_vp), _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _sz, _i, _i, _vp]),
    "dfh_cliph_text_embeds": (_i, [_vp, C.POINTER(_vp), _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _sz, _i, _i, _vp]),
    "dfh_causal_attention": (_i, [_vp, _vp, _i, _i, _i, _i, _f, _vp]),
    "dfh_imgproc_create": (_i, [C.POINTER(ImgProcConfigC), _i, _i, _i, C.POINTER(_vp)]),
    "dfh_imgproc_destroy": (None, [_vp]),
    "dfh_imgproc_resized_height": (_i, [_vp]),
    "dfh_imgproc_resized_width": (_i, [_vp]),
    "dfh_imgproc_out_height": (_i, [_vp]),
    "dfh_imgproc_out_width": (_i, [_vp]),
    "dfh_imgproc_crop_top": (_i, [_vp]),
    "dfh_imgproc_crop_left": (_i, [_vp]),
    "dfh_imgproc_ksize_x": (_i, [_vp]),
    "dfh_imgproc_ksize_y": (_i, [_vp]),
    "dfh_imgproc_table_bytes": (_sz, [_vp]),
    "dfh_imgproc_fill_tables": (_i, [_vp, _vp, _sz]),
    "dfh_imgproc_run": (_i, [_vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp]),
    "dfh_jpeg_quant_tables": (_i, [_i, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "dfh_jpeg_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "dfh_jpeg_coef_count": (_sz, [_i, _i, _i, _i]),
    "dfh_jpeg_roundtrip": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "dfh_lpips_create": (_i, [C.POINTER(LpipsConfigC), C.POINTER(_vp)]),
    "dfh_lpips_destroy": (None, [_vp]),
    "dfh_lpips_num_params": (_i, [_vp]),
    "dfh_lpips_param_name": (C.c_char_p, [_vp, _i]),
    "dfh_lpips_param_ndim": (_i, [_vp, _i]),
    "dfh_lpips_param_dim": (_i, [_vp, _i, _i]),
    "dfh_lpips_packed_bytes": (_sz, [_vp]),
    "dfh_lpips_pack": (_i, [_vp, C.POINTER(_vp), _i, _vp, _vp]),
    "dfh_lpips_workspace_bytes": (_sz, [_vp, _i, _i, _i]),
    "dfh_lpips_forward": (_i, [_vp, C.POINTER(_vp), _i, _vp, _vp, _vp, _i, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "dfh_lpips_group_argmin": (_i, [_vp, _vp, _i, _i, _vp]),
    "dfh_lpips_prep": (_i, [_vp, _i, _vp, _vp, _vp, _i, _vp, _i, _i, _i, _vp]),
    "dfh_lpips_conv3x3_relu": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "dfh_lpips_maxpool2x2": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "dfh_lpips_layer_score": (_i, [_vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "dfh_incep_create": (_i, [C.POINTER(IncepConfigC), C.POINTER(_vp)]),
    "dfh_incep_destroy": (None, [_vp]),
    "dfh_incep_num_params": (_i, [_vp]),
    "dfh_incep_param_name": (C.c_char_p, [_vp, _i]),
    "dfh_incep_param_ndim": (_i, [_vp, _i]),
    "dfh_incep_param_dim": (_i, [_vp, _i, _i]),
    "dfh_incep_packed_bytes": (_sz, [_vp]),
    "dfh_incep_pack": (_i, [_vp, C.POINTER(_vp), _i, _vp, _vp]),
    "dfh_incep_plan_count": (_i, [_vp, _i, _i, _i]),
    "dfh_incep_plan_entry": (_i, [_vp, _i, _i, _i, _i, C.POINTER(IncepLaunchC)]),
    "dfh_incep_workspace_bytes": (_sz, [_vp, _i, _i, _i]),
    "dfh_incep_forward": (_i, [_vp, C.POINTER(_vp), _i, _vp, _vp, _i, _i, _i, C.POINTER(_vp), _vp, _vp, _sz, _vp]),
    "dfh_incep_prep": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp]),
    "dfh_incep_conv_bn_relu": (_i, [_vp, _vp, _i, C.POINTER(_vp), _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "dfh_incep_pool": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "dfh_incep_global_mean": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "dfh_incep_fc_softmax": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "dfh_incep_is_rows": (_i, [_vp, _vp, _i, _i, _f, _vp, _vp, _vp, _vp, _vp]),
    "dfh_incep_is_splits": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp]),
    "dfh_incep_stats": (_i, [_vp, _i, _i, _vp, _vp, _vp]),
    "dfh_vae_create": (_i, [C.POINTER(VAEConfigC), C.POINTER(_vp)]),
    "dfh_vae_destroy": (None, [_vp]),
    "dfh_vae_num_params": (_i, [_vp]),
    "dfh_vae_param_name": (C.c_char_p, [_vp, _i]),
    "dfh_vae_param_ndim": (_i, [_vp, _i]),
    "dfh_vae_param_dim": (_i, [_vp, _i, _i]),
    "dfh_vae_arena16_bytes": (_sz, [_vp]),
    "dfh_vae_arena32_bytes": (_sz, [_vp]),
    "dfh_vae_workspace_bytes": (_sz, [_vp, _i, _i, _i]),
    "dfh_vae_bind": (_i, [_vp, _vp, _vp, _vp, _sz]),
    "dfh_vae_pack": (_i, [_vp, C.POINTER(_vp), _i, _vp]),
    "dfh_vae_encode": (_i, [_vp, _vp, _vp, _i, _i, _vp]),
    "dfh_vae_decode": (_i, [_vp, _vp, _vp, _i, _i, _vp]),
    "dfh_unet_arena16t_bytes": (_sz, [_vp]),
    "dfh_unet_grad16_bytes": (_sz, [_vp]),
    "dfh_unet_grad32_bytes": (_sz, [_vp]),
    "dfh_unet_train_workspace_bytes": (_sz, [_vp, _i]),
    "dfh_unet_bind_train": (_i, [_vp, _vp, _vp, _vp, _vp, _sz, _i]),
    "dfh_unet_set_checkpointing": (_i, [_vp, _i]),
    "dfh_unet_checkpointing": (_i, [_vp]),
    "dfh_unet_train_workspace_regions": (_i, [_vp, _i, C.POINTER(_sz)]),
    "dfh_unet_pack_train": (_i, [_vp, C.POINTER(_vp), _i, _vp]),
    "dfh_unet_pack_all": (_i, [_vp, C.POINTER(_vp), _i, _vp]),
    "dfh_unet_grad_sumsq": (_i, [_vp, _vp]),
    "dfh_unet_forward_train": (_i, [_vp, _vp, _i, _vp, _vp, _i, _vp, _i, _vp]),
    "dfh_unet_backward": (_i, [_vp, _vp, _vp, C.POINTER(_vp), _i, _i, _vp]),
    "dfh_unet_backward_begin": (_i, [_vp, _vp, _vp, _sz, _vp]),
    "dfh_unet_backward_next": (_i, [_vp, C.POINTER(_sz), C.POINTER(_sz), _vp]),
    "dfh_unet_backward_finish": (_i, [_vp, C.POINTER(_vp), _i, _i, _vp]),
    "dfh_gemm_partial_floats": (_sz, [C.POINTER(GemmDesc)]),
    "dfh_gemm": (_i, [C.POINTER(GemmDesc), _vp]),
    "dfh_gemm_wgrad": (_i, [C.POINTER(GemmDesc), _vp, _i, _vp, _i, _i, _vp]),
    "dfh_gemm_wgrad_partial_floats": (_sz, [C.POINTER(GemmDesc), _i]),
    "dfh_groupnorm_fold": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, C.c_float, _vp, _i, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp]),
    "dfh_gemm_wgrad_plan": (_i, [C.POINTER(GemmDesc), _i, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "dfh_gemm_plan": (_i, [C.POINTER(GemmDesc), C.POINTER(GemmPlanExtra), C.POINTER(GemmPlanInfo)]),
    "dfh_colsum": (_i, [_vp, _i, _i, _i, _i, _vp, _i, _vp]),
    "dfh_groupnorm": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _vp, _vp, _f, _i, _vp, _vp, _vp]),
    "dfh_gemm_gstat": (_i, [C.POINTER(GemmDesc), _vp, C.POINTER(C.c_int)]),
    "dfh_groupnorm_pre": (_i, [_vp, _i, _i, _i, _i, _vp, _vp, _f, _i, _vp, _vp, _i, _vp, _vp]),
    "dfh_groupnorm_stats": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _vp, _vp, _f, _i, _vp, _vp, _vp, _vp]),
    "dfh_groupnorm_bwd": (_i, [_vp, _i, _vp, _i, _vp, _i, _i, _i, _vp, _vp, _vp, _i, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp]),
    "dfh_attention_lse": (_i, [_vp, _i, _vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _i, _i, _f, _vp, _vp]),
    "dfh_attention_delta": (_i, [_vp, _vp, _i, _vp, _i, _i, _i, _i, _vp]),
    "dfh_attention_bwd": (_i, [_vp, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _vp, _vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _i, _i, _f, _vp]),
    "dfh_layernorm_bwd": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _i, _f, _vp]),
    "dfh_pack_matrix_t": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "dfh_pack_conv3x3_t": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "dfh_unpack_matrix": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "dfh_unpack_conv3x3": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "dfh_unpack_vector": (_i, [_vp, _vp, _i, _i, _i, _vp]),
    "dfh_pool2x2_sum": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "dfh_add_bf16": (_i, [_vp, _vp, _sz, _i, _vp]),
    "dfh_geglu_fwd": (_i, [_vp, _vp, _sz, _i, _vp]),
    "dfh_geglu_bwd": (_i, [_vp, _vp, _vp, _sz, _i, _vp]),
    "dfh_act_fwd": (_i, [_vp, _vp, _sz, _i, _vp]),
    "dfh_act_bwd": (_i, [_vp, _vp, _vp, _vp, _vp, _sz, _i, _f, _vp]),
    "dfh_nhwc_to_nchw_f32": (_i, [_vp, _vp, _i, _i, _i, _i, _f, _i, _vp]),
    "dfh_transpose_bf16": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _sz, _sz, _vp]),
    "dfh_mse_bwd": (_i, [_vp, _vp, _vp, _vp, _i, _i, _f, _vp, _vp]),
    "dfh_assemble_bwd": (_i, [_vp, _vp, _vp, _i, _i, _f, _vp]),
    "dfh_sumsq": (_i, [_vp, _sz, _vp, _vp]),
    "dfh_adamw": (_i, [_vp, _vp, _vp, _vp, _sz, _f, _f, _f, _f, _f, _i, _vp, _f, _vp]),
    "dfh_ema": (_i, [_vp, _vp, _sz, _f, _vp]),
    "dfh_adamw_ema": (_i, [_vp, _vp, _vp, _vp, _vp, _sz, _f, _f, _f, _f, _f, _i, _vp, _f, _f, _vp]),
    "dfh_q8_table": (_i, [_i, _vp]),
    "dfh_q8_quantize": (_i, [_vp, _vp, _vp, _sz, _i, _vp]),
    "dfh_q8_dequantize": (_i, [_vp, _vp, _vp, _sz, _i, _vp]),
    "dfh_adamw8": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _f, _f, _f, _f, _f, _i, _vp, _f, _f, _vp]),
    "dfh_wire_pack": (_i, [_vp, _vp, _sz, _sz, _vp]),
    "dfh_wire_shard_mean": (_i, [_vp, _vp, _i, _sz, _vp]),
    "dfh_wire_unpack": (_i, [_vp, _vp, _sz, _vp]),
    "dfh_layernorm": (_i, [_vp, _vp, _vp, _vp, _i, _i, _f, _vp]),
    "dfh_gemm_out2": (_i, [C.POINTER(GemmDesc), _vp, _i, _i, _vp]),
    "dfh_ups_phase_fold": (_i, [_vp, _i, _vp, _i, _i, _vp]),
    "dfh_conv_up2x": (_i, [_vp, _i, _i, _i, _i, _vp, _i, _vp, _vp, _vp, _vp]),
    "dfh_wino_weights": (_i, [_vp, _i, _vp, _i, _i, _i, _vp]),
    "dfh_wino_blocked": (_i, [_i, _i]),
    "dfh_prof_saved_flops": (C.c_double, []),
    "dfh_wino_input": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "dfh_gn_wino_input_ok": (_i, [_i, _i, _i, _i, _i]),
    "dfh_gn_wino_input_chain": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _f, _i, _vp, _i, _i, _i, _vp]),
    "dfh_gn_wino_input": (_i, [_vp, _i, _vp, _i, _vp, _vp, _f, _i, _vp, _i, _i, _i, _vp]),
    "dfh_conv3x3_wino_scratch_bytes": (C.c_size_t, [_i, _i, _i, _i, _i]),
    "dfh_conv3x3_wino": (_i, [_vp, _i, _i, _i, _i, _vp, _i, _i, _vp, _vp, _i, _i, _vp, _vp, _vp, C.c_size_t, _vp, _vp]),
    "dfh_gemm_batched": (_i, [C.POINTER(GemmDesc), _i, C.c_long, C.c_long, C.c_long, _vp]),
    "dfh_ln_fold": (_i, [_vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp]),
    "dfh_gemm_ln": (_i, [C.POINTER(GemmDesc), _vp, C.POINTER(C.c_int), _vp, _i, _i, _f, _vp, _vp]),
    "dfh_quantize_rows_fp8": (_i, [_vp, _i, _vp, _vp, _i, _i, _vp]),
    "dfh_layernorm_fp8": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _f, _vp]),
    "dfh_gemm_fp8": (_i, [C.POINTER(Fp8GemmDesc), _vp]),
    "dfh_mlp_fused_image_bytes": (_sz, []),
    "dfh_mlp_fused_pack": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "dfh_mlp_fused": (_i, [_vp, _vp, _vp, _vp, _i, _i, _f, _vp, _vp, _i, _i, _vp, _i, _i, _vp]),
    "dfh_groupnorm_fp8": (_i, [_vp, _i, _i, _i, _i, _f, _f, _vp, _vp, _vp]),
    "dfh_attention_fp8out": (_i, [_vp, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _i, _f, _vp]),
    "dfh_amax_slabs": (_i, [_vp, C.c_long, _i, _i, _vp, _vp, _vp, _i, _i, _vp]),
    "dfh_attention_fp8": (_i, [_vp, _i, _vp, _i, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _f, _vp]),
    "dfh_attn_scales": (_i, [_vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp]),
    "dfh_unet_enable_fp8": (_i, [_vp]),
    "dfh_unet_enable_fp8_attention": (_i, [_vp, _i]),
    "dfh_unet_arena8_bytes": (_sz, [_vp]),
    "dfh_unet_bind_fp8": (_i, [_vp, _vp]),
    "dfh_attention": (_i, [_vp, _i, _vp, _i, _vp, _i, _vp, _i, _i, _i, _i, _i, _i, _f, _vp]),
    "dfh_timestep_embedding": (_i, [_vp, _vp, _i, _i, _vp]),
    "dfh_nchw_to_nhwc_bf16": (_i, [_vp, _i, _vp, _i, _i, _i, _vp]),
    "dfh_cast_f32_to_bf16": (_i, [_vp, _vp, _sz, _vp]),
    "dfh_pack_conv3x3": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "dfh_pack_matrix": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "dfh_pack_vector": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "dfh_mutual_reduce": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "dfh_assemble_input": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _f, _i, _vp]),
    "dfh_cfg_step": (_i, [_vp, _vp, _vp, _vp, _sz, _i, _f, _f, _f, C.POINTER(StepCoef), _vp]),
    "dfh_cfg_multistep": (_i, [_vp] * 9 + [_sz, _i, _f, _f, _f, C.POINTER(MultistepCoef), _vp]),
    "dfh_noise_mix": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp]),
    "dfh_mse_rows": (_i, [_vp, _vp, _vp, _i, _i, _vp]),
}
_NO_STATUS = {"dfh_abi_version", "dfh_census_count", "dfh_unet_checkpointing", "dfh_unet_num_params", "dfh_unet_param_ndim", "dfh_unet_param_dim", "dfh_vae_num_params",
              "dfh_vae_param_ndim", "dfh_vae_param_dim", "dfh_clip_num_params", "dfh_clip_param_ndim", "dfh_clip_param_dim",
              "dfh_clipv_num_params", "dfh_clipv_param_ndim", "dfh_clipv_param_dim", "dfh_lpips_num_params", "dfh_lpips_param_ndim", "dfh_lpips_param_dim",
              "dfh_imgproc_resized_height", "dfh_imgproc_resized_width", "dfh_imgproc_out_height", "dfh_imgproc_out_width", "dfh_imgproc_crop_top",
              "dfh_imgproc_crop_left", "dfh_imgproc_ksize_x", "dfh_imgproc_ksize_y",
              "dfh_incep_num_params", "dfh_incep_param_ndim", "dfh_incep_param_dim"}

_lib = None
_UNBOUND = set()
ABI_VERSION = 8          # == DFH_ABI_VERSION of include/difashion_hip.h (checked when the library is loaded)


def storage() -> str:
    """'bf16' or 'fp16': the 16-bit storage format of this process's kernel library."""
    return _STORAGE


def set_storage(name: str) -> None:
    """Choose the storage format before the library is first used.  Raises once the library is loaded with the other format."""
    global _STORAGE, LIB_PATH
    name = str(name).strip().lower()
    if name not in _LIB_NAMES:
        raise ValueError(f"set_storage({name!r}): the storage format is 'bf16' or 'fp16'")
    if name == _STORAGE:
        return
    if _lib is not None:
        raise DfhError(f"set_storage({name!r}): the {_STORAGE} library is already loaded ({LIB_PATH}); the storage format is fixed "
                       "per process -- set DFH_STORAGE or call set_storage() before the first use")
    _STORAGE = name
    if not os.environ.get("DFH_LIB"):
        LIB_PATH = os.path.join(CSRC, _LIB_NAMES[name])


def storage_dtype():
    """The torch dtype that tensor dtype code 1 of the C ABI means in this process."""
    import torch
    return torch.float16 if _STORAGE == "fp16" else torch.bfloat16


def dtype_code(t, what: str = "tensor") -> int:
    """C-ABI dtype code of a tensor: 0 = float32, 1 = the library's storage type.  The other 16-bit type is refused."""
    import torch
    if t.dtype == torch.float32:
        return 0
    if t.dtype == storage_dtype():
        return 1
    if t.dtype in (torch.float16, torch.bfloat16):
        raise TypeError(f"{what} is {t.dtype}, but this process runs the {_STORAGE}-storage library: pass float32 or "
                        f"{storage_dtype()} (DFH_STORAGE / set_storage() select the other library)")
    raise TypeError(f"{what} must be float32 or {storage_dtype()}, got {t.dtype}")


def require_bf16(what: str) -> None:
    """Training and the fp8 legs exist in the bf16 library only."""
    if _STORAGE != "bf16":
        raise DfhError(f"{what} is refused under DFH_STORAGE=fp16: the fp16-storage library is inference only (training has no loss "
                       "scaling; the fp8 epilogues are calibrated against bf16 producers) -- run it with the default bf16 storage")


def build(force: bool = False) -> str:
    """Compile the HIP sources for gfx950 (hipcc cross-compiles without a GPU): both storage builds of the library."""
    args = ["make", "-C", CSRC, "-j", str(min(8, os.cpu_count() or 1))]
    if force:
        subprocess.run(["make", "-C", CSRC, "clean"], check=True, capture_output=True)
    r = subprocess.run(args, capture_output=True, text=True)
    if r.returncode != 0:
        raise DfhError("building libdifashion_hip.so / libdifashion_hip_f16.so failed:\n" + r.stdout[-4000:] + r.stderr[-4000:])
    return LIB_PATH


def raw():
    """The ctypes CDLL with prototypes set.  Raises if the library has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise DfhError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU / PyTorch fallback for the compute path)")
        lib = C.CDLL(LIB_PATH)
        # DFH_LIB=<path> loads another build; it is held to the same ABI check as the default path.  Only with the explicit
        # DFH_LIB_ALLOW_ABI_MISMATCH=1 (same-box A/B probes against LAST ROUND's library) are missing entry points left unbound and
        # the ABI number ignored -- and then call() refuses an unbound entry point instead of calling it through ctypes' default
        # int prototype (which truncates pointers and size_t).  Never on the product path.
        probe = bool(os.environ.get("DFH_LIB")) and os.environ.get("DFH_LIB_ALLOW_ABI_MISMATCH") == "1"
        unbound = set()
        for name, (res, args) in SIGNATURES.items():
            if probe and not hasattr(lib, name):
                unbound.add(name)
                continue
            fn = getattr(lib, name)       # AttributeError here = header/library drift
            fn.restype = res
            fn.argtypes = args
        got = lib.dfh_abi_version()
        if got != ABI_VERSION and not probe:
            raise DfhError(f"{LIB_PATH} reports ABI {got}, this Python side binds ABI {ABI_VERSION} (include/difashion_hip.h "
                           "DFH_ABI_VERSION): rebuild the library (`python -c 'import __graft_entry__ as g; g.build()'`)"
                           + ("; DFH_LIB_ALLOW_ABI_MISMATCH=1 loads it anyway for an A/B probe" if os.environ.get("DFH_LIB") else ""))
        info = lib.dfh_build_info().decode()
        built = info.split("storage=")[1].split()[0] if "storage=" in info else "bf16"      # older builds (DFH_LIB probes): bf16
        if built != _STORAGE:
            raise DfhError(f"{LIB_PATH} is a {built}-storage build, this process selected {_STORAGE} (DFH_STORAGE / set_storage())")
        global _UNBOUND
        _UNBOUND = unbound
        _lib = lib
    return _lib


def last_error() -> str:
    return raw().dfh_last_error().decode()


def call(name: str, *args):
    """Call a status-returning entry point; raise DfhError with the library's message on failure."""
    lib = raw()
    if name in _UNBOUND:
        raise DfhError(f"{name} is not exported by {LIB_PATH} (an older build loaded under DFH_LIB_ALLOW_ABI_MISMATCH=1)")
    rc = getattr(lib, name)(*args)
    if name not in _NO_STATUS and SIGNATURES[name][0] is _i and rc != 0:
        raise DfhError(f"{name} failed ({rc}): {last_error()}")
    return rc


def call_count(name: str, *args):
    """Call an entry point that returns a count (>= 0) or a negative status."""
    lib = raw()
    if name in _UNBOUND:
        raise DfhError(f"{name} is not exported by {LIB_PATH} (an older build loaded under DFH_LIB_ALLOW_ABI_MISMATCH=1)")
    rc = getattr(lib, name)(*args)
    if rc < 0:
        raise DfhError(f"{name} failed ({rc}): {last_error()}")
    return rc


_WEIGHT_EPOCH = 0


def weight_epoch() -> int:
    """Bumped by the fused optimizer after it rewrites master weights in place (torch version counters do not see a
    native kernel's writes); part of every pack signature."""
    return _WEIGHT_EPOCH


def bump_weight_epoch():
    global _WEIGHT_EPOCH
    _WEIGHT_EPOCH += 1


def prof_begin():
    call("dfh_prof_begin")


def prof_end():
    """-> {class name: dict(launches, ms, flops, bytes)} since prof_begin (synchronises the device)."""
    arr = (ProfClass * 16)()
    n = raw().dfh_prof_end(arr, 16)
    if n < 0:
        raise DfhError(f"dfh_prof_end failed: {last_error()}")
    return {arr[i].name.decode(): dict(launches=arr[i].launches, ms=arr[i].ms, flops=arr[i].flops, bytes=arr[i].bytes)
            for i in range(n)}


def census_reset():
    raw().dfh_census_reset()


def census():
    """-> {kernel family: launches since census_reset()} (host-side counters of the launchers; test infrastructure)."""
    lib = raw()
    return {lib.dfh_census_name(i).decode(): int(lib.dfh_census_get(i)) for i in range(lib.dfh_census_count())}


def walk_switches():
    """-> {DFH_* name: value as text}: the walk and launcher switches as this process's library read them (no GPU needed)."""
    lib = raw()
    buf = C.create_string_buffer(lib.dfh_walk_switches(None, 0) + 1)
    lib.dfh_walk_switches(buf, len(buf))
    return dict(line.split("=", 1) for line in buf.value.decode().splitlines())


def stream_ptr():
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    """Device pointer of a torch tensor (None -> NULL)."""
    return C.c_void_p(0 if t is None else t.data_ptr())


# ---- gradient epochs: FusedAdamW.zero_grad() opens an epoch; whatever writes a gradient (autograd accumulation, the native
#      U-Net backward) stamps the parameter with the epoch it wrote in; step() updates only parameters stamped since the last
#      zero_grad -- torch.optim.AdamW's "skip parameters whose .grad is None" for gradient views that are never None.
_GRAD_EPOCH = [1]


def grad_epoch() -> int:
    return _GRAD_EPOCH[0]


def next_grad_epoch() -> int:
    _GRAD_EPOCH[0] += 1
    return _GRAD_EPOCH[0]


def stamp_grads(params) -> None:
    e = _GRAD_EPOCH[0]
    for p in params:
        p._dfh_grad_epoch = e

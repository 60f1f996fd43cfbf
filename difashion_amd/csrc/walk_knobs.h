// Every DFH_* switch that decides which kernels a walk (unet_model.h, unet_train.hip) or a launcher runs, in one struct.  The GEMM plan's
// switches are GemmKnobs (gemm_plan.h); DFH_PROF_DUMP and DFH_GEMM_PLAN_DUMP name files and are not switches.  DESIGN.md 4.1 has the table.
//
// WalkKnobs::get() reads ALL names from the environment at the first use of any one, once per process.  That is safe because nothing sets
// one of these names inside a process that has already loaded the library: the tests, scripts/*.py and bench.py all set them for child
// processes.  A new switch keeps to that: one line in the list below, set from outside the process, never re-read.
//
// Host code only (walk_knobs.hip); dfh_walk_switches prints the struct, one NAME=value line per field in the order below, without a GPU.
#pragma once
#include <stddef.h>

namespace dfh {

// X(type, field, NAME, parse, default).  Three parses:
//   off_at_0 : on unless the value starts with '0'      on_at_1 : off unless the value starts with '1'      as_int / as_double : atoi / atof
#define DFH_WALK_KNOBS(X)                                                                                                                  \
  /* the inference walk (unet_model.h) */                                                                                                  \
  X(int, wino_maxhw, DFH_WINO_MAXHW, as_int, 256)             /* largest image (pixels) whose wide resnet convs take Winograd; 1024 adds 32x32 */ \
  X(bool, fp8_ext, DFH_FP8_EXT, off_at_0, true)               /* 0: only the LayerNorm-fed projections in e4m3 (the round-2 set) */          \
  X(bool, fp8_attn, DFH_FP8_ATTN, on_at_1, false)             /* 1: the e4m3 attention products, as dfh_unet_enable_fp8_attention */         \
  X(bool, token_linear, DFH_TOKEN_LINEAR, on_at_1, false)     /* 1: the token-linear kernel on the K = N = C projections; probe builds only */ \
  X(bool, gn_pre, DFH_GN_PRE, off_at_0, true)                 /* 0: no GroupNorm statistics from the producing GEMM / fused MLP epilogue */   \
  X(bool, ups_phase, DFH_UPS_PHASE, off_at_0, true)           /* 0: the upsample convs as a 3x3 conv over the virtual upsampled image */      \
  X(int, wino, DFH_WINO, as_int, 2)                           /* 0: direct convs everywhere, 1: Winograd at H * W <= 64, 2: up to wino_maxhw */ \
  X(bool, wino_gn, DFH_WINO_GN, off_at_0, true)               /* 0: separate GroupNorm launches in front of the Winograd convs */             \
  X(bool, wino_chain, DFH_WINO_CHAIN, off_at_0, true)         /* 0: conv1's output is materialised between the two Winograd convs */          \
  X(bool, ln_fold, DFH_LN_FOLD, off_at_0, true)               /* 0: LayerNorm kernels + plain weights */                                      \
  X(int, gn_fold, DFH_GN_FOLD, as_int, 320)                   /* widest block whose entry GroupNorm folds into proj_in; 0 = off */            \
  X(bool, qkv_merge, DFH_QKV_MERGE, off_at_0, true)           /* 0: q | k and V^T as two launches */                                          \
  X(bool, ffp_fold, DFH_FFP_FOLD, off_at_0, true)             /* 0: ff.net.2 and proj_out as two linears */                                   \
  X(bool, check_dup, DFH_CHECK_DUP, on_at_1, false)           /* 1: verify the dup-tail hint with a synchronous compare */                    \
  /* the training walk (unet_train.hip) */                                                                                                 \
  X(double, train_side_min_flop, DFH_TRAIN_SIDE_MIN_FLOP, as_double, 2e10)   /* smaller weight-gradient launches stay on the main stream */  \
  X(bool, train_ups_phase, DFH_TRAIN_UPS_PHASE, off_at_0, true)              /* 0: 3x3 conv over the upsampled image + 2x2 sum pool backward */ \
  X(bool, train_geglu_fused, DFH_TRAIN_GEGLU_FUSED, off_at_0, true)          /* 0: ff.net.0 and the gating as two launches */               \
  X(bool, train_side, DFH_TRAIN_SIDE, off_at_0, true)                        /* 0: no second stream for the weight gradients */            \
  /* the launchers */                                                                                                                      \
  X(int, gn_sc, DFH_GN_SC, as_int, 512)                       /* norm.hip: statistics chunks to aim for over the batch (probe) */             \
  X(int, gn_ac, DFH_GN_AC, as_int, 1024)                      /* norm.hip: the same for the apply pass (probe) */                             \
  X(int, gn_small_max, DFH_GN_SMALL_MAX, as_int, 16)          /* norm.hip: units per thread up to which the one-kernel GroupNorm runs */      \
  X(bool, gn_mid, DFH_GN_MID, off_at_0, true)                 /* norm.hip: 0 = no group-quad kernel between the small and the two-kernel path */ \
  X(bool, attn_x32, DFH_ATTN_X32, off_at_0, true)             /* attention.hip: 0 = the 16x16 MFMA kernel everywhere */                       \
  X(bool, attn_xs, DFH_ATTN_XS, off_at_0, true)               /* attention_x32.hip: 0 = no short-key (cross-attention) kernel */              \
  X(int, attn_variant, DFH_ATTN_VARIANT, as_int, 0)           /* attention_x32.hip: experiment instantiations; probe builds only */           \
  X(int, attn_qb64, DFH_ATTN_QB64, as_int, 2)                 /* attention_x32.hip: query blocks per wave at D = 64 (probe) */                \
  X(int, attn_bwd_x32, DFH_ATTN_BWD_X32, as_int, 0)           /* attention_bwd.hip: 32x32 MFMA in pass 1 (1, 2) / pass 2 (1, 3) */            \
  X(int, wgrad_plan, DFH_WGRAD_PLAN, as_int, 2)               /* wgrad.hip: 1 = the earlier slice candidates (1 or multiples of 8) */         \
  X(int, mlp_fused, DFH_MLP_FUSED, as_int, 2)                 /* mlp_fused2.hip: 0 = the two-launch feed-forward; 1 / 2 = the kernel's forms */

struct WalkKnobs {
#define DFH_X(type, field, name, parse, dflt) type field;
  DFH_WALK_KNOBS(DFH_X)
#undef DFH_X
  static const WalkKnobs& get();
};

// the body of dfh_walk_switches: writes at most cap - 1 characters and a NUL, returns the length of the whole text
size_t walk_switches_text(char* buf, size_t cap);

}  // namespace dfh

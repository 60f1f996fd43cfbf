/* libdifashion_hip.so -- C ABI of the MI355X (gfx950) DiFashion denoising path.
 *
 * The reference has no C ABI / FFI: its boundary is Python duck-typing on two objects held by
 * DiFashion (``self.unet``, ``self.noise_scheduler``).  This header is what the
 * Python host side (difashion_amd/, mirroring the diffusers call signatures) binds through ctypes;
 * INTEGRATION.md shows the binding a maintainer of the reference would add.  Every entry point
 * names the reference interface it replaces (DiFashion/models/difashion.py = "df.py"; diffusers
 * 0.18.2 classes are external, pinned by the reference README.md:27).
 *
 * Conventions: plain pointers and sizes only (no torch types); all pointers are DEVICE pointers
 * unless marked host; ``stream`` is a hipStream_t passed as void*; every function returns 0 on
 * success or a negative status, with the message available from dfh_last_error(); nothing
 * throws; nothing allocates device memory (callers own arenas / workspaces); a context is
 * re-entrant per instance and not thread-safe when shared.
 *
 * dtypes: "bf16" = raw uint16 bfloat16 bits.  Activations inside the library are NHWC bf16; the
 * public tensors keep the reference's layouts (NCHW latents, [B][77][D] text states).
 */
#ifndef DIFASHION_HIP_H
#define DIFASHION_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Bumped whenever an entry point, a struct layout or the meaning of an argument changes (round 4: 4).  The Python host side
 * (difashion_amd/_lib.py ABI_VERSION) refuses a library that reports another number: a stale .so next to new Python, or the reverse,
 * fails at load time instead of at a symbol lookup or silently. */
#define DFH_ABI_VERSION 8
#define DFH_MAX_BLOCKS 4

/* ------------------------------------------------------------------ library */
int dfh_abi_version(void);
const char* dfh_last_error(void);          /* message of the last failing call on this thread */
const char* dfh_build_info(void);          /* "gfx950 ..." */

/* Per-kernel-class timing with HIP events recorded on the launch stream (bench.py "roofline"):
 * between begin and end every launch is bracketed by two events; end synchronises and sums, per
 * class, launches / elapsed ms / ALGORITHMIC flops and bytes (DESIGN.md "Measurement").  Not for
 * use inside a timed region whose wall clock is being reported (adds two event records per launch). */
typedef struct dfh_prof_class {
  char name[32];
  int launches;
  double ms, flops, bytes;
} dfh_prof_class;
int dfh_prof_begin(void);
int dfh_prof_end(dfh_prof_class* out, int max_classes);   /* returns the number of classes written (7) */
/* flops of the reference algorithm that the launches of the window reported but did not execute: the upsampler convs
 * run 4 of the 9 taps (phase planes), the Winograd convs 16 multiply-adds per 2x2 outputs and channel instead of 36 */
double dfh_prof_saved_flops(void);

/* Launch census: how many times each kernel family was launched since the last reset (host-side counters bumped by the launchers).
 * Test infrastructure for "which kernels did this walk take" (tests/test_gpu_unet.py: the batch-16 forward of the bench workload). */
void dfh_census_reset(void);
int dfh_census_count(void);
const char* dfh_census_name(int i);
long dfh_census_get(int i);
/* The DFH_* switches of the model walks and the launchers as this process read them (host code, no GPU needed): one
 * NAME=value line per switch, on/off switches as 1 / 0.  The environment is read once per process, at the first use of any switch.
 * Writes at most cap - 1 characters and a NUL into buf (buf may be NULL with cap 0); returns the length of the whole text. */
size_t dfh_walk_switches(char* buf, size_t cap);

/* ------------------------------------------------------------------ U-Net context
 * Replaces: diffusers UNet2DConditionModel as constructed at df.py:77-93 (in_channels widened to
 * 8) and called at df.py:249-253 (training) and df.py:518-523 (sampling). */
typedef struct dfh_unet_config {
  int sample_size;                  /* latent H = W (64) */
  int in_channels;                  /* 8: [latent | history latent], df.py:83-85 */
  int out_channels;                 /* 4 */
  int num_blocks;                   /* 4 */
  int block_out_channels[DFH_MAX_BLOCKS]; /* 320,640,1280,1280 */
  int layers_per_block;             /* 2 */
  int cross_attention_dim;          /* 768 (SD-1.5) / 1024 (SD-2) */
  int num_heads[DFH_MAX_BLOCKS];    /* diffusers "attention_head_dim": 8,8,8,8 / 5,10,20,20 */
  int down_attn[DFH_MAX_BLOCKS];    /* 1,1,1,0 */
  int use_linear_projection;        /* only changes parameter shapes (1x1 conv == linear in NHWC) */
  int norm_num_groups;              /* 32 */
  float norm_eps;                   /* 1e-5 */
  int text_len;                     /* 77 */
} dfh_unet_config;

typedef struct dfh_unet dfh_unet;

int dfh_unet_create(const dfh_unet_config* cfg, dfh_unet** out);   /* host-only work */
void dfh_unet_destroy(dfh_unet* u);

/* Parameter table, in diffusers state-dict order/names: the single source of truth
 * the Python module builds its nn.Parameters from (checkpoint drop-in, df.py:77-79, train.py:524-547). */
int dfh_unet_num_params(const dfh_unet* u);
const char* dfh_unet_param_name(const dfh_unet* u, int i);
int dfh_unet_param_ndim(const dfh_unet* u, int i);
int dfh_unet_param_dim(const dfh_unet* u, int i, int d);

/* Packed-weight arenas (bf16 GEMM operands in kernel layout, fp32 vectors) and activation workspace.
 * Sizes are bytes; buffers are caller-allocated device memory, 256-byte aligned. */
size_t dfh_unet_arena16_bytes(const dfh_unet* u);
size_t dfh_unet_arena32_bytes(const dfh_unet* u);
size_t dfh_unet_workspace_bytes(dfh_unet* u, int batch);
int dfh_unet_bind(dfh_unet* u, void* arena16, void* arena32, void* workspace, size_t workspace_bytes, int max_batch);

/* fp8 linears inside the U-Net walk (inference): call dfh_unet_enable_fp8 right after create (it changes the workspace plan),
 * allocate dfh_unet_arena8_bytes, bind it; dfh_unet_pack then also refreshes the e4m3 copies + per-channel scales. */
int dfh_unet_enable_fp8(dfh_unet* u);
/* optional, BEFORE dfh_unet_enable_fp8: also run the self-attention products QK^T / PV on the e4m3 MFMA (csrc/attention_fp8.hip; head dims
 * 40 / 80 / 160, whole 64-key tiles).  Off by default: measured slower than the bf16 kernels on this model (profiles/r04). */
int dfh_unet_enable_fp8_attention(dfh_unet* u, int on);
size_t dfh_unet_arena8_bytes(const dfh_unet* u);
int dfh_unet_bind_fp8(dfh_unet* u, void* arena8);

/* fp32 master parameters (device pointers, table order) -> packed arenas.  Call after every
 * weight update (optimizer step / load_state_dict). */
int dfh_unet_pack(dfh_unet* u, const float* const* master_params, int count, void* stream);

/* noise_pred = unet(sample, timestep, encoder_hidden_states).sample
 *   sample   : [B][in_channels][H][W]  fp32 (sample_bf16=0) or bf16 (1), NCHW as in df.py:216/:515
 *   timestep : [B] fp32 (the host side expands the 0-d / int / (B,) forms, df.py:251,:520)
 *   ehs      : [B][text_len][cross_attention_dim] fp32 (ehs_bf16=0) or bf16 (1)
 *   out      : [B][out_channels][H][W] fp32, NCHW */
int dfh_unet_forward(dfh_unet* u, const void* sample, int sample_bf16, const float* timestep,
                     const void* ehs, int ehs_bf16, float* out, int batch, void* stream);

/* Per-run constants of a sampling loop.  In fashion_generation the prompt states are fixed for the whole run (df.py:340-357, stacked
 * once at :388-427) and the timesteps are the schedule's list (:356, :456), the same for every row of the CFG batch: the
 * cross-attention K / V^T of all transformer blocks and the time-embedding rows (time_embedding MLP + all 22 time_emb_proj) depend on
 * nothing else.  dfh_unet_run_cache computes them once into a caller-owned, 256-byte-aligned buffer of dfh_unet_run_cache_bytes;
 * dfh_unet_forward_cached is dfh_unet_forward for a batch whose rows all sit at timesteps[t_index], with those launches skipped
 * (5 GEMMs + 2 small kernels per step).  The cache is valid until the weights are re-packed or the text states change. */
size_t dfh_unet_run_cache_bytes(const dfh_unet* u, int batch, int n_timesteps);
int dfh_unet_run_cache(dfh_unet* u, const void* ehs, int ehs_bf16, int batch, const float* timesteps /* device [n] */, int n_timesteps,
                       void* cache, size_t cache_bytes, void* stream);
/* One-shot hint for the NEXT dfh_unet_forward / dfh_unet_forward_cached call: the last `images` images of its batch have the same
 * sample and timestep as the `images` before them and differ only in their encoder_hidden_states -- the prompt-only branch of
 * classifier-free guidance (difashion.py:388-427, 494-512: category_prompts vs null_prompts over the same latent / mutual / history
 * input).  conv_in, the first resnet and the first transformer block up to its self-attention are then computed once for the pair.
 * The caller vouches for the equality (DFH_CHECK_DUP=1 verifies it with a synchronous compare: debugging aid); the call clears the hint. */
int dfh_unet_set_dup_tail(dfh_unet* u, int images);
int dfh_unet_forward_cached(dfh_unet* u, const void* sample, int sample_bf16, const void* cache, int batch, int n_timesteps, int t_index,
                            float* out, void* stream);

/* ------------------------------------------------------------------ training step (train.py:691-716)
 * Replaces torch autograd through the U-Net: accelerator.backward(loss) at DiFashion/train.py:699 for the module
 * called at DiFashion/models/difashion.py:249-253.  Shares arena16/arena32 with the inference path
 * (dfh_unet_bind + dfh_unet_pack first) and adds
 *   arena16t  : bf16 transposed/flipped weight packs for the data-gradient GEMMs   (dfh_unet_arena16t_bytes)
 *   grad16/32 : fp32 gradient arenas in the PACKED layouts of arena16 / arena32      (dfh_unet_grad16/32_bytes)
 *   workspace : the activations one step keeps + gradient buffers                    (dfh_unet_train_workspace_bytes)
 * All pointers 256-byte aligned device memory; arena16t must be zero-filled before the first pack. */
size_t dfh_unet_arena16t_bytes(dfh_unet* u);
size_t dfh_unet_grad16_bytes(const dfh_unet* u);
size_t dfh_unet_grad32_bytes(const dfh_unet* u);
size_t dfh_unet_train_workspace_bytes(dfh_unet* u, int batch);
int dfh_unet_bind_train(dfh_unet* u, void* arena16t, void* grad16, void* grad32, void* workspace, size_t workspace_bytes,
                        int max_batch);
/* Gradient checkpointing of the training walk (train.py:559-560, unet.enable_gradient_checkpointing()); a property of the context.
 *   0 : off (default) -- the workspace holds every activation of the step;
 *   1 : every resnet / transformer layer keeps only its output; the backward runs the layer's forward launches again, into one
 *       recompute region shared by all layers, right before the layer's backward launches;
 *   2 : as 1, but the two attention outputs of a transformer layer (and their log-sum-exp rows) are kept and the attention kernels
 *       do not run again.
 * The gradients are those of mode 0: the same kernels run on the same operands.  dfh_unet_train_workspace_bytes answers for the
 * current mode, so set it BEFORE dfh_unet_bind_train: a change of mode unbinds the training workspace.  Refused for a mode outside
 * 0..2 and between a dfh_unet_forward_train and its backward.
 * dfh_unet_train_workspace_regions: the parts of dfh_unet_train_workspace_bytes (their sum + 256) in bytes --
 * regions[0] head (zero page, GroupNorm partials, split-K slabs), [1] persistent activations, [2] layer-internal gradient stack,
 * [3] recompute region (0 in mode 0). */
int dfh_unet_set_checkpointing(dfh_unet* u, int mode);
int dfh_unet_checkpointing(const dfh_unet* u);
int dfh_unet_train_workspace_regions(dfh_unet* u, int batch, size_t* regions);
/* master parameters -> arena16t; call together with dfh_unet_pack after every weight update */
int dfh_unet_pack_train(dfh_unet* u, const float* const* master_params, int count, void* stream);
/* dfh_unet_pack + dfh_unet_pack_train in one pass over the master parameters (each weight is read once and written to both arenas);
 * what a training step calls after the optimizer moved the weights.  Needs dfh_unet_bind_train. */
int dfh_unet_pack_all(dfh_unet* u, const float* const* master_params, int count, void* stream);
/* out != NULL: from now on the gradient un-pack at the end of dfh_unet_backward / _backward_finish also writes
 * out[0] = sum of the squares of every gradient value it wrote into master_grads (the final values, also when it accumulates): the
 * clip norm of train.py:700 without another pass over the gradients.  Deterministic (per-block partials, fixed-order reduce).
 * out == NULL switches it off.  The float must stay valid until then. */
int dfh_unet_grad_sumsq(dfh_unet* u, float* out);
/* same arguments and result as dfh_unet_forward; keeps the activations the backward needs */
int dfh_unet_forward_train(dfh_unet* u, const void* sample, int sample_bf16, const float* timestep,
                           const void* ehs, int ehs_bf16, float* out, int batch, void* stream);
/* Backward of the LAST dfh_unet_forward_train (one backward per forward).
 *   d_out        : [B][out_channels][H][W] fp32, gradient of the loss wrt the noise prediction
 *   d_sample     : [B][in_channels][H][W] fp32 or NULL (gradient wrt the assembled input -> MutualEncoder)
 *   master_grads : table-order device pointers to the fp32 .grad of each parameter; gradients are ADDED
 *                  (entries may be NULL to skip a frozen parameter).  encoder_hidden_states gets no gradient
 *                  (frozen CLIP text states, df.py:229-247).
 *   overwrite    : 1 = the gradients hold nothing yet (first backward after zero_grad): they are STORED, which saves
 *                  zero-filling and re-reading 3.4 GB; 0 = added (gradient accumulation over micro-batches). */
int dfh_unet_backward(dfh_unet* u, const float* d_out, float* d_sample, float* const* master_grads, int count, int overwrite,
                      void* stream);

/* The same backward in pieces, for data-parallel training: the caller all-reduces finished ranges of the packed fp32
 * gradient arena (the ``grad16`` buffer of dfh_unet_bind_train) on a second stream while the walk continues -- the
 * reference's DDP buckets (accelerate / torch DDP around train.py:611,699) without an autograd hook per parameter.
 *   begin  : arms the walk; ``bucket_floats`` = granularity of the ranges (floats of grad16).  Returns the tape length.
 *   next   : runs layers from the back of the tape until some range of grad16 is FINAL (no later layer writes into it),
 *            returns 1 with [*lo, *hi) in floats, 0 when the tape is exhausted (every range has been handed out), < 0 on error.
 *   finish : un-packs grad16 / grad32 (whatever they hold by then, e.g. the all-reduced average) into the master
 *            gradients exactly as dfh_unet_backward does.  dfh_unet_backward == begin + next until 0 + finish. */
int dfh_unet_backward_begin(dfh_unet* u, const float* d_out, float* d_sample, size_t bucket_floats, void* stream);
int dfh_unet_backward_next(dfh_unet* u, size_t* lo, size_t* hi, void* stream);
int dfh_unet_backward_finish(dfh_unet* u, float* const* master_grads, int count, int overwrite, void* stream);

/* Copies a named NHWC bf16 intermediate of the LAST forward into ``dst`` as fp32 NCHW (layer-level
 * parity tests).  Names: "conv_in", "down0".."down3", "mid", "up0".."up3". */
int dfh_unet_debug_tap(dfh_unet* u, const char* name, float* dst, size_t dst_floats, void* stream);

/* ------------------------------------------------------------------ AutoencoderKL
 * Replaces diffusers' AutoencoderKL as the reference calls it: vae.encode(images).latent_dist (df.py:129,144,376,435-437)
 * and vae.decode(latents / scaling_factor) (df.py:580).  Same ownership rules as dfh_unet: caller-owned, zero-filled
 * arenas + workspace, fp32 master parameters in table order with diffusers state-dict names. */
typedef struct dfh_vae_config {
  int in_channels;                 /* 3 */
  int out_channels;                /* 3 */
  int latent_channels;             /* 4 */
  int num_blocks;                  /* 4 */
  int block_out_channels[DFH_MAX_BLOCKS];   /* 128, 256, 512, 512 */
  int layers_per_block;            /* 2 */
  int norm_num_groups;             /* 32 */
} dfh_vae_config;
typedef struct dfh_vae dfh_vae;
int dfh_vae_create(const dfh_vae_config* cfg, dfh_vae** out);
void dfh_vae_destroy(dfh_vae* u);
int dfh_vae_num_params(const dfh_vae* u);
const char* dfh_vae_param_name(const dfh_vae* u, int i);
int dfh_vae_param_ndim(const dfh_vae* u, int i);
int dfh_vae_param_dim(const dfh_vae* u, int i, int d);
size_t dfh_vae_arena16_bytes(const dfh_vae* u);
size_t dfh_vae_arena32_bytes(const dfh_vae* u);
/* encode != 0: size = image side; else size = latent side */
size_t dfh_vae_workspace_bytes(dfh_vae* u, int encode, int batch, int size);
int dfh_vae_bind(dfh_vae* u, void* arena16, void* arena32, void* workspace, size_t workspace_bytes);
int dfh_vae_pack(dfh_vae* u, const float* const* master_params, int count, void* stream);
/* images [B][in_channels][S][S] fp32 -> moments [B][2*latent_channels][S/8][S/8] fp32 = [mean | logvar] */
int dfh_vae_encode(dfh_vae* u, const float* images, float* moments, int batch, int image_size, void* stream);
/* latents [B][latent_channels][s][s] fp32 -> images [B][4][8s][8s] fp32 (out_channels = 3 used, the 4th plane is padding) */
int dfh_vae_decode(dfh_vae* u, const float* latents, float* images, int batch, int latent_size, void* stream);

/* ------------------------------------------------------------------ CLIP text encoder
 * Replaces transformers' CLIPTextModel as the reference builds and calls it: CLIPTextModel.from_pretrained(..., subfolder="text_encoder")
 * at df.py:70-72, text_encoder(input_ids)[0] at df.py:224,234 (every training batch) and df.py:340-342,352 (every sampling call).
 * fp32 end to end (csrc/clip.hip: linears on v_mfma_f32_16x16x4_f32): the prompts are a closed set encoded once per run, so the
 * encoder is built for agreement with the fp32 class (1e-6), not for speed.  The fp32 master parameters are read in place
 * (nn.Linear layout): no arenas, no pack step; parameter table in transformers 4.32.1 state-dict order / names ("text_model.*"). */
typedef struct dfh_clip_config {
  int vocab_size;                  /* 49408 */
  int hidden_size;                 /* 768 (SD-1.5, CLIP ViT-L/14) / 1024 (SD-2, OpenCLIP ViT-H/14) */
  int intermediate_size;           /* 3072 / 4096 */
  int num_hidden_layers;           /* 12 / 23 */
  int num_attention_heads;         /* 12 / 16 */
  int max_position_embeddings;     /* 77 (<= 128) */
  int hidden_act;                  /* 1 quick_gelu (SD-1.5) / 2 gelu, erf form (SD-2) */
  float layer_norm_eps;            /* 1e-5 */
} dfh_clip_config;
typedef struct dfh_clip dfh_clip;
int dfh_clip_create(const dfh_clip_config* cfg, dfh_clip** out);   /* host-only work */
void dfh_clip_destroy(dfh_clip* c);
int dfh_clip_num_params(const dfh_clip* c);
const char* dfh_clip_param_name(const dfh_clip* c, int i);
int dfh_clip_param_ndim(const dfh_clip* c, int i);
int dfh_clip_param_dim(const dfh_clip* c, int i, int d);
size_t dfh_clip_workspace_bytes(const dfh_clip* c, int batch, int seq_len);
/* outputs = text_encoder(input_ids):
 *   master_params     : HOST array of `count` device pointers to the fp32 parameters, table order, each 16-byte aligned
 *   input_ids         : [batch][seq_len] int64 (tokenizer output, data_utils.py:107-110); causal mask only, no padding mask (the
 *                       reference passes input_ids alone).  Ids outside [0, vocab_size) are CLAMPED here; refusing them, as
 *                       nn.Embedding does, is the caller's part (the Python wrapper raises IndexError)
 *   last_hidden_state : [batch][seq_len][hidden_size] fp32 = outputs[0], after final_layer_norm
 *   pooler_output     : [batch][hidden_size] fp32 or NULL; the row at argmax(input_ids) when eos_token_id == 2 (transformers 4.32.1),
 *                       else at the first eos_token_id
 *   hidden_states     : NULL, or [num_hidden_layers + 1][batch][seq_len][hidden_size] fp32 = output_hidden_states=True (embeddings
 *                       output, then every layer's output; layer-level parity tests)
 *   workspace         : >= dfh_clip_workspace_bytes(batch, seq_len), 256-byte aligned */
int dfh_clip_encode(dfh_clip* c, const float* const* master_params, int count, const int64_t* input_ids, float* last_hidden_state,
                    float* pooler_output, int eos_token_id, float* hidden_states, void* workspace, size_t workspace_bytes, int batch,
                    int seq_len, void* stream);
/* text_embeds = CLIPTextModelWithProjection(input_ids) = open_clip's encode_text (Evaluation/eval_utils.py:101-114):
 * the walk of dfh_clip_encode over the same dfh_clip object and parameter table, then the pooled row of every sequence (the rule of
 * pooler_output above, found on the device) is gathered from the last block's output, normalised by final_layer_norm -- those `batch`
 * rows only -- and projected without bias.
 *   text_projection   : [projection_dim][hidden_size] fp32, 16-byte aligned: a pointer of its own, not part of the parameter table
 *   text_embeds       : [batch][projection_dim] fp32
 *   pooler_output     : NULL, or [batch][hidden_size]: the bits dfh_clip_encode gives (LayerNorm is row-local)
 *   last_hidden_state : NULL, or [batch][seq_len][hidden_size]: only then does the LayerNorm over all batch * seq_len rows run
 *   hidden_states, workspace (>= dfh_clip_workspace_bytes): as in dfh_clip_encode */
int dfh_clip_text_embeds(dfh_clip* c, const float* const* master_params, int count, const float* text_projection, int projection_dim,
                         const int64_t* input_ids, float* text_embeds, float* pooler_output, float* last_hidden_state, int eos_token_id,
                         float* hidden_states, void* workspace, size_t workspace_bytes, int batch, int seq_len, void* stream);

/* ------------------------------------------------------------------ embedding-side metrics of the evaluation
 * csrc/eval_scores.hip; fp32 in both storage builds, no atomics (reruns are bit-identical, a row does not depend on its batch).
 *
 * out[r] = scale * <a_r, b_r> / (|a_r| |b_r|): 100 * F.cosine_similarity of Evaluation/eval_utils.py:101-135 (CLIP score, CLIP image
 * score) and :503-538 (personalisation similarity).  a, b [rows][dim] fp32 dense, out [rows]; no scratch.  A zero row gives NaN in its
 * own score, as the reference's x / x.norm() does. */
int dfh_embed_pair_cosine(const float* a, const float* b, float* out, int rows, int dim, float scale, void* stream);
/* sims[r][k] = cos(gen_r, table[cand[r][k]]), pred[r] = argmax_k sims[r][k] (ties: the lowest k; a NaN counts as the maximum, as
 * torch.argmax has it): the retrieval accuracy of eval_utils.py:652-723 (K = 5) and the ranking of :725-767 (K in the thousands).
 * gen [rows][dim], table [table_rows][dim] fp32, cand [rows][K] int64 gathered in the kernel, sims [rows][K] fp32, pred [rows] int64.
 * Ids outside [0, table_rows) are CLAMPED here; refusing them, as indexing does, is the caller's part (the Python side raises). */
int dfh_embed_candidates(const float* gen, const float* table, const int64_t* cand, float* sims, int64_t* pred, int rows, int K, int dim,
                         int table_rows, void* stream);

/* Grounding retrieval (csrc/eval_rank.hip): the ranking of clip_og_retrieval_given_data (eval_utils.py:725-767, called
 * by Evaluation/evaluate_grounding_gor.py:237-266) -- every generated row against ALL items of its category, the nmax best kept in
 * order, then recall@N of the ground-truth item.  Candidate sets are ragged: a flat id list cut by offsets.  fp32 in both storage
 * builds, no atomics, no allocation, no scratch; reruns are bit-identical and a row's result does not depend on the rows it rides with.
 *
 * norms[r] = |x_r| of x [rows][dim] fp32 (dim a multiple of 4, x 16-byte aligned), one wave a row.  A caller that ranks many batches
 * against one table computes the table's norms once. */
int dfh_embed_row_norms(const float* x, float* norms, int rows, int dim, void* stream);
/* The largest top-N list a row keeps. */
#define DFH_EMBED_RANK_NMAX 128
/* Bytes of the similarity workspace of one dfh_embed_rank call: rows x (max_set_len rounded up to 64) floats + 256; 0 for arguments
 * the call would refuse.  Host-only. */
size_t dfh_embed_rank_workspace_bytes(int rows, long max_set_len, int nmax);
/* For every row r, with S = row_set[r] and its candidates c_j = cand_ids[set_off[S] + j], j < len = set_off[S + 1] - set_off[S]:
 *   sim_j = <gen_r, table[c_j]> / (|gen_r| |table[c_j]|)   on v_mfma_f32_16x16x4_f32: a 64 x 64 tile of rows THAT SHARE ONE SET by
 *           candidates, the table rows gathered in the tile's loads, k-tiles of 32 summed with a compensated add; the similarities
 *           of the call's rows are materialised in `workspace` ([rows][ld] floats) and read once by the selection;
 *   out_ids / out_pos / out_sims [rows][nmax]: the best min(len, nmax) in order -- descending, a NaN above everything (torch.topk's
 *           order), and among EQUAL values (-0.0 == +0.0, NaN == NaN for this purpose) the lower position j first -- as item id c_j
 *           (int64), position j (int64) and similarity; slots from out_counts[r] = min(len, nmax) on hold id -1, position -1, sim -inf.
 * A zero row (generated or table) gives NaN in its own similarities only.
 *   gen [rows][dim], table [table_rows][dim] fp32, 16-byte aligned, dim a multiple of 4; gen_norms [rows], table_norms [table_rows]
 *           from dfh_embed_row_norms;
 *   cand_ids  : DEVICE int64 [set_off[nsets]].  Ids outside [0, table_rows) are CLAMPED before they address anything; refusing them,
 *               as indexing does, is the caller's part (the ids live on the device: the Python side checks them where they live);
 *   set_off   : HOST int64 [nsets + 1], monotone, from 0;  row_set: HOST int [rows], ascending (rows arrive grouped by set) -- both are
 *               read before the launches: they are the launch geometry (one GEMM and one selection launch per run of equal row_set);
 *   nmax      : 1 .. DFH_EMBED_RANK_NMAX;
 *   workspace : >= dfh_embed_rank_workspace_bytes(rows, longest set of these rows, nmax), 256-byte aligned.  A caller bounds it by
 *               ranking its rows in bands; the result does not depend on the cut. */
int dfh_embed_rank(const float* gen, const float* gen_norms, int rows, int dim, const float* table, const float* table_norms, int table_rows,
                   const int64_t* cand_ids, const int64_t* set_off, int nsets, const int* row_set, int nmax, void* workspace,
                   size_t workspace_bytes, int64_t* out_ids, int64_t* out_pos, float* out_sims, int* out_counts, void* stream);
/* hit_pos[r] = the first rank j < counts[r] with ids[r][j] == grd[r], -1 if none (the reference's `grd in topN_iids[:N]` is
 * 0 <= hit_pos[r] < N); hits[c] = #{r : 0 <= hit_pos[r] < cutoffs[c]} from one workgroup's integer reduction.
 * ids [rows][nmax] int64, counts [rows] int, grd [rows] int64, cutoffs [ncut] int (ncut <= 64; 0: hit_pos only), hit_pos [rows] int,
 * hits [ncut] int64 -- all on the device. */
int dfh_embed_recall(const int64_t* ids, const int* counts, int rows, int nmax, const int64_t* grd, const int* cutoffs, int ncut, int* hit_pos,
                     int64_t* hits, void* stream);

/* ------------------------------------------------------------------ the device-resident item store
 * csrc/item_store.hip.  The VAE posterior of every item is computed once and kept as one fp32 table row [mean | std] (row_stride
 * floats apart, row_elems = C x H x W each half); the model's inputs are then row gathers.  fp32 in both storage builds and compiled
 * without mul+add contraction: every result below is the stated chain of separate IEEE fp32 operations.  No atomics, nothing
 * allocated, no scratch, no workspace, one launch each.  A lane owns one float4 of the output row; the grid is (row, 1024-float slab).
 * All row offsets are 64-bit.  Refused on the host, by message, before any HIP call: null pointers, row_elems or row_stride not a
 * multiple of 4, row_stride < row_elems, a pointer that is not 16-byte aligned, negative counts.  rows == 0 is a no-op.
 *
 * out[r][j] = (table[iid_r][j] + table[iid_r][row_elems + j] * eps[r][j]) * scale: `latent_dist.sample() * scaling_factor` with the
 * caller's eps.  eps == NULL: out[r][j] = table[iid_r][j] * scale, `latent_dist.mode() * scaling_factor`; the std half is then never
 * read, so a means-only table (row_stride == row_elems) is legal -- with eps, row_stride < 2 * row_elems is refused.
 *   table [table_rows][row_stride] fp32; iids [rows] int64 ON THE DEVICE; eps, out [rows][row_elems] fp32.
 * An id outside [0, table_rows) writes a row of NaN and reads nothing (the ids live on the device: no sync for a check). */
int dfh_item_gather(const float* table, long table_rows, long row_stride, int row_elems, const int64_t* iids, long rows, const float* eps,
                    float scale, float* out, void* stream);
/* The history condition (data_utils.py:142-155: the mean latent of a user's history items of one category) from the item table itself.
 * Row r with segment s = row_seg[r], items i_k = seg_items[seg_offsets[s] + k], k < count = seg_offsets[s + 1] - seg_offsets[s]:
 *   acc = 0;  for k in list order: t_k = table[i_k][j] * scale (rounded), acc = acc + t_k (rounded);  out[r][j] = acc / (float)count
 * -- one accumulator, one IEEE division; at least four item loads in flight per lane, the adds still in list order.  A row with
 * row_seg[r] == -1 or an empty segment copies null_row [row_elems].  Only the first row_elems floats of a table row are read.
 *   seg_items int64, seg_offsets int64 [S + 1], row_seg int32 [rows]: all ON THE DEVICE; row_seg < S is the caller's part.  An item id
 *   outside [0, table_rows) adds NaN and reads nothing. */
int dfh_history_rows(const float* table, long table_rows, long row_stride, int row_elems, const int64_t* seg_items, const int64_t* seg_offsets,
                     const int* row_seg, long rows, const float* null_row, float scale, float* out, void* stream);

/* The compatibility scorer: FashionEvaluator (Evaluation/compatibility_evaluator/compatibility_net.py:14-81) under the gather of
 * CompatibilityEvaluator.evaluate_compatibility (eval_utils.py:574-588), all outfits of a call at once.  Inference: Dropout is the
 * identity.  Linears on v_mfma_f32_16x16x4_f32, LayerNorm + ReLU fused per row.
 *   params      : HOST array of DFH_COMPAT_NUM_PARAMS device pointers, fp32, 16-byte aligned, in the class's state-dict order:
 *                 feat_layer.{weight,bias}, emb_layer.{0,1,4,5,8,9,12,13}.{weight,bias}, eval_layer.{0,1,4,5,8,9,12}.{weight,bias}
 *   feat_dim    : cnn_feat_dim, a multiple of 4
 *   feats_real  : [real_rows][feat_dim]; feats_gen: [gen_rows][feat_dim] or NULL (gen_rows = 0)
 *   olists      : [outfits][items] int64: an id <= 0 reads feats_gen[-id], an id > 0 reads feats_real[id] (ids out of range are
 *                 CLAMPED here, the Python side refuses them).  NULL: feats_real is the gathered [outfits][items][feat_dim] tensor
 *   items       : 2 .. 8; all items (items - 1) / 2 pairs in itertools.combinations order
 *   outfit_emb  : NULL, or [outfits][256];  logits, scores: NULL, or [outfits] (scores = sigmoid(logits))
 *   workspace   : >= dfh_compat_workspace_bytes(outfits, items, feat_dim), 256-byte aligned */
#define DFH_COMPAT_NUM_PARAMS 32
size_t dfh_compat_workspace_bytes(int outfits, int items, int feat_dim);
int dfh_compat_score(const float* const* params, int count, int feat_dim, const float* feats_real, int real_rows, const float* feats_gen,
                     int gen_rows, const int64_t* olists, int outfits, int items, float* outfit_emb, float* logits, float* scores,
                     void* workspace, size_t workspace_bytes, void* stream);
/* FashionEvaluator.pred_score on its own: eval_layer over outfit_emb [outfits][256] -> logits, scores (either may be NULL).
 * workspace: >= dfh_compat_workspace_bytes(outfits, 2, 4) */
int dfh_compat_pred_score(const float* const* params, int count, const float* outfit_emb, int outfits, float* logits, float* scores,
                          void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ CLIP image encoder: vision tower + projection
 * Replaces (arithmetic) the OpenCLIP ViT-H/14 ``encode_image`` that the reference's Evaluation/ scripts call on every generated and
 * ground-truth image (Evaluation/extract_hist_embs.py:83-100, Evaluation/eval_utils.py:91-135, :503-535), under the architecture and
 * key names of transformers' CLIPVisionModelWithProjection ("vision_model.*", "visual_projection.weight"; "pre_layrnorm" is the
 * library's own spelling).  fp32 end to end in both storage builds (csrc/clip_vision.hip): patch embedding as im2col + GEMM, the
 * linears and LayerNorms of the text tower, and a bidirectional attention kernel that streams K / V through LDS in key tiles
 * (online softmax), so the sequence length is not bounded by LDS.  Master parameters are read in place: no arenas, no pack step.
 * Image resize / normalisation is the dfh_imgproc family below (row f7); the metrics computed from the embeddings are row f6. */
typedef struct dfh_clipv_config {
  int hidden_size;                 /* 1024 (ViT-L/14) / 1280 (ViT-H/14) */
  int intermediate_size;           /* 4096 / 5120 */
  int num_hidden_layers;           /* 24 / 32 */
  int num_attention_heads;         /* 16: head dim 64 / 80; any multiple of 4 up to 128 */
  int image_size;                  /* 224 */
  int patch_size;                  /* 14: tokens = 1 + (image_size / patch_size)^2 = 257 */
  int num_channels;                /* 3 */
  int projection_dim;              /* 768 / 1024 */
  int hidden_act;                  /* 1 quick_gelu (OpenAI ViT-L/14) / 2 gelu, erf form (OpenCLIP ViT-H/14) */
  float layer_norm_eps;            /* 1e-5 */
} dfh_clipv_config;
typedef struct dfh_clipv dfh_clipv;
int dfh_clipv_create(const dfh_clipv_config* cfg, dfh_clipv** out);   /* host-only work */
void dfh_clipv_destroy(dfh_clipv* c);
int dfh_clipv_num_params(const dfh_clipv* c);
const char* dfh_clipv_param_name(const dfh_clipv* c, int i);
int dfh_clipv_param_ndim(const dfh_clipv* c, int i);
int dfh_clipv_param_dim(const dfh_clipv* c, int i, int d);
size_t dfh_clipv_workspace_bytes(const dfh_clipv* c, int batch);
/* outputs = vision_model(pixel_values), T = 1 + (image_size / patch_size)^2:
 *   master_params     : HOST array of `count` device pointers to the fp32 parameters, table order, each 16-byte aligned
 *   pixel_values      : [batch][num_channels][image_size][image_size] fp32 (already resized and normalised)
 *   last_hidden_state : [batch][T][hidden_size] fp32, the output of the last block (NOT normalised, as in transformers)
 *   pooler_output     : NULL, or [batch][hidden_size] = post_layernorm(last_hidden_state[:, 0])
 *   image_embeds      : NULL, or [batch][projection_dim] = visual_projection(pooler_output)
 *   hidden_states     : NULL, or a HOST array of num_hidden_layers + 1 device pointers, each NULL or [batch][T][hidden_size] fp32:
 *                       entry 0 receives the pre_layrnorm output, entry l the output of block l (output_hidden_states=True)
 *   workspace         : >= dfh_clipv_workspace_bytes(batch), 256-byte aligned */
int dfh_clipv_encode(dfh_clipv* c, const float* const* master_params, int count, const float* pixel_values, int batch,
                     float* last_hidden_state, float* pooler_output, float* image_embeds, float* const* hidden_states,
                     void* workspace, size_t workspace_bytes, void* stream);
/* The attention kernel of the vision tower on its own (tests, microbenchmarks): O = softmax(Q K^T * scale) V per (batch, head), no
 * mask.  qkv [batch * T][3 * heads * head_dim] fp32 (q | k | v, heads contiguous inside each), out [batch * T][heads * head_dim];
 * head_dim a multiple of 4 up to 128, any T >= 1. */
int dfh_clipv_attention(const float* qkv, float* out, int batch, int T, int heads, int head_dim, float scale, void* stream);

/* ---- the same tower in the library's 16-bit storage format (bf16; fp16 in libdifashion_hip_f16.so), opt-in (csrc/clip_vision_half.hip):
 * the `dfh_clipvh_*` family works on a dfh_clipv context (the `dfh_clipv_*` name set above is the fp32 tower's and stays as it is).
 * What transformers' torch_dtype= / .half() and open_clip's precision="bf16" / "fp16" give: 16-bit weights and a 16-bit residual stream
 * between launches, with every accumulation, LayerNorm statistic, softmax and activation in fp32.  The walk: im2col (16-bit rows, K
 * zero-padded to a multiple of 8) -> patch GEMM -> class token + position embeddings + pre_layrnorm in one launch -> per block LayerNorm,
 * ONE q | k | v launch (q | k row-major, V transposed per image with rows padded to a multiple of 8 keys), dfh_attention's kernels,
 * out-proj + residual, LayerNorm, fc1 + GELU / quick-GELU in the GEMM epilogue, fc2 + residual -> post_layernorm of the class rows and
 * visual_projection in fp32 arithmetic.  No atomics: a rerun is bit-identical.  Head dims: those of dfh_attention (32, 40, 64, 80, 128, 160).
 *   packed copy  : dfh_clipvh_packed_bytes(c) bytes, 256-byte aligned, written by dfh_clipvh_pack from the fp32 masters and remade by the
 *                  caller whenever a master changes: per matrix [N][K] 16-bit, K-contiguous -- the patch-conv weight as
 *                  [hidden][C p p padded to a multiple of 8], q | k | v stacked as one [3 hidden][hidden] matrix with their biases
 *                  stacked as one fp32 [3 hidden] vector.  All other biases, the LayerNorm affines, class / position embeddings and
 *                  visual_projection are read from the fp32 masters in place.
 *   pixel_values : fp32 (pixel_dtype 0) or the storage format (1), aligned to its element size
 *   outputs      : as dfh_clipv_encode, all fp32, each 16-byte aligned (the non-null hidden_states entries too); last_hidden_state and
 *                  hidden_states are exact upcasts of the 16-bit stream
 *   workspace    : >= dfh_clipvh_workspace_bytes(c, batch) (0: refused, see dfh_last_error), 256-byte aligned
 * A config whose 2 x hidden is no whole number of the q | k | v launch's column tiles (hidden 192: 160-column tiles) is refused by every
 * entry point of the family, dfh_clipvh_plan included, before anything is launched.
 * dfh_clipvh_plan is the host function both the size query and the walk are built on (no GPU needed): every GEMM launch's
 * M / N / K / leading dims, the V^T padding and the byte range of every workspace region. */
#define DFH_CLIPVH_MAX_LAUNCHES 8
#define DFH_CLIPVH_MAX_REGIONS 16
typedef struct dfh_clipvh_launch {
  char name[16];                   /* patch, qkv, out_proj, fc1, fc2 */
  int M, N, K;                     /* K as the kernel walks it (patch: padded) */
  int lda, ldw, ld_out;            /* elements */
  int n_split, ld_out2, rows_per_b;/* qkv: columns [n_split, N) leave transposed per image into [batch][N - n_split][ld_out2] */
  int act;                         /* 0 none, 5 gelu, 6 quick_gelu (dfh_gemm_desc.act) */
  int resid;                       /* 1: + the residual stream, in place */
  int per_layer;                   /* 1: launched once per block */
  int a_region, out_region, out2_region;   /* indices into regions (-1: none) */
} dfh_clipvh_launch;
typedef struct dfh_clipvh_region {
  char name[16];
  size_t offset, bytes;            /* inside the workspace; offsets are multiples of 256 */
} dfh_clipvh_region;
typedef struct dfh_clipvh_plan_info {
  int batch, tokens, hidden, intermediate, heads, head_dim, layers, projection_dim;
  int patch_k, patch_k_padded;     /* C p p and its multiple of 8 (588 -> 592 at patch 14) */
  int rows, patch_rows;            /* batch * tokens, batch * (tokens - 1) */
  int ldvt;                        /* V^T row pitch: tokens rounded up to a multiple of 8 (257 -> 264) */
  int attention_x32;               /* 1: dfh_attention takes the 32x32x16 kernel at this length and head dim, 0: the 16x16x32 one */
  int num_launches, num_regions;
  size_t workspace_bytes, packed_bytes;
  dfh_clipvh_launch launches[DFH_CLIPVH_MAX_LAUNCHES];
  dfh_clipvh_region regions[DFH_CLIPVH_MAX_REGIONS];
} dfh_clipvh_plan_info;
int dfh_clipvh_plan(const dfh_clipv* c, int batch, dfh_clipvh_plan_info* out);   /* host-only work */
size_t dfh_clipvh_packed_bytes(const dfh_clipv* c);
int dfh_clipvh_pack(dfh_clipv* c, const float* const* master_params, int count, void* packed, void* stream);
size_t dfh_clipvh_workspace_bytes(const dfh_clipv* c, int batch);
int dfh_clipvh_encode(dfh_clipv* c, const float* const* master_params, int count, const void* packed, const void* pixel_values,
                      int pixel_dtype, int batch, float* last_hidden_state, float* pooler_output, float* image_embeds,
                      float* const* hidden_states, void* workspace, size_t workspace_bytes, void* stream);

/* ---- the CLIP text encoder in the library's 16-bit storage format, opt-in (csrc/clip_text_half.hip): the
 * `dfh_cliph_*` family works on a dfh_clip context (the `dfh_clip_*` name set above is the fp32 tower's and stays as it is).  What
 * transformers' torch_dtype= / .half() and the reference's `--mixed_precision fp16` autocast give: 16-bit weights and a 16-bit residual
 * stream between launches, every accumulation, LayerNorm statistic, softmax and activation in fp32.  The walk: token gather + position
 * add in fp32, rounded once -> per block LayerNorm, ONE q | k | v launch into [rows][3 hidden], the causal attention kernel (one
 * workgroup per (sequence, head), head dim 64, at most 128 tokens), out-proj + residual, LayerNorm, fc1 + GELU / quick-GELU in the GEMM
 * epilogue, fc2 + residual -> final_layer_norm and (text_embeds) text_projection in fp32 arithmetic.  No atomics: a rerun is bit-identical.
 *   packed copy  : dfh_cliph_packed_bytes(c) bytes, 256-byte aligned, written by dfh_cliph_pack from the fp32 masters and remade by the
 *                  caller whenever a master changes: per layer q | k | v stacked as one [3 hidden][hidden] matrix, out_proj, fc1, fc2
 *                  ([N][K] 16-bit, K-contiguous) and the q | k | v biases stacked as one fp32 [3 hidden] vector.  Token / position
 *                  embeddings, all other biases, the LayerNorm affines and text_projection are read from the fp32 masters in place.
 *   outputs      : as dfh_clip_encode / dfh_clip_text_embeds, all fp32, each 16-byte aligned; hidden_states are exact upcasts of the
 *                  16-bit stream, last_hidden_state = final_layer_norm (fp32 arithmetic) of the upcast stream
 *   workspace    : >= dfh_cliph_workspace_bytes(c, batch, seq_len) (0: refused, see dfh_last_error), 256-byte aligned
 * Refused by every entry point of the family, dfh_cliph_plan included, before anything is launched (each message names the fp32 tower as
 * the alternative): a head dim other than 64, hidden / intermediate sizes that are no multiples of 8, a sequence length outside
 * [1, min(128, max_position_embeddings)].
 * dfh_cliph_plan is the host function both size queries and the walk are built on (no GPU needed): every GEMM launch's M / N / K /
 * leading dims (dfh_clipvh_launch; n_split / ld_out2 / out2_region unused) and the byte range of every workspace region. */
typedef struct dfh_cliph_plan_info {
  int batch, tokens, hidden, intermediate, heads, head_dim, layers;
  int rows;                        /* batch * tokens */
  int attention_lds_bytes;         /* static LDS of one workgroup of the causal attention kernel */
  int num_launches, num_regions;
  size_t workspace_bytes, packed_bytes;
  dfh_clipvh_launch launches[DFH_CLIPVH_MAX_LAUNCHES];   /* qkv, out_proj, fc1, fc2 */
  dfh_clipvh_region regions[DFH_CLIPVH_MAX_REGIONS];
} dfh_cliph_plan_info;
int dfh_cliph_plan(const dfh_clip* c, int batch, int seq_len, dfh_cliph_plan_info* out);   /* host-only work */
size_t dfh_cliph_packed_bytes(const dfh_clip* c);
int dfh_cliph_pack(dfh_clip* c, const float* const* master_params, int count, void* packed, void* stream);
size_t dfh_cliph_workspace_bytes(const dfh_clip* c, int batch, int seq_len);
/* arguments as dfh_clip_encode, plus the packed copy */
int dfh_cliph_encode(dfh_clip* c, const float* const* master_params, int count, const void* packed, const int64_t* input_ids,
                     float* last_hidden_state, float* pooler_output, int eos_token_id, float* hidden_states, void* workspace,
                     size_t workspace_bytes, int batch, int seq_len, void* stream);
/* arguments as dfh_clip_text_embeds, plus the packed copy: the eos rows are gathered from the 16-bit stream first, final_layer_norm and
 * text_projection run in fp32 on those rows only; last_hidden_state (NULL: not formed) and pooler_output have dfh_cliph_encode's bits */
int dfh_cliph_text_embeds(dfh_clip* c, const float* const* master_params, int count, const void* packed, const float* text_projection,
                          int projection_dim, const int64_t* input_ids, float* text_embeds, float* pooler_output, float* last_hidden_state,
                          int eos_token_id, float* hidden_states, void* workspace, size_t workspace_bytes, int batch, int seq_len, void* stream);
/* The causal attention kernel of the 16-bit text tower on its own (tests, microbenchmarks): O = softmax(mask(Q K^T * scale)) V per
 * (batch, head), key j > query i masked.  qkv [batch * T][3 * heads * 64] in the storage format (q | k | v, heads contiguous inside
 * each), out [batch * T][heads * 64] in the storage format, both 16-byte aligned; head_dim must be 64, T in [1, 128]. */
int dfh_causal_attention(const void* qkv, void* out, int batch, int T, int heads, int head_dim, float scale, void* stream);

/* ------------------------------------------------------------------ CLIP image preprocessing
 * Replaces (arithmetic) open_clip's / transformers' image transform in front of the tower (Evaluation/extract_hist_embs.py:83-100,
 * evaluate_gor.py:193-236): PIL's antialiased 8-bit resize (horizontal pass, then vertical pass, integer arithmetic over 22-bit
 * coefficient tables computed in double, the intermediate image clipped to uint8), a floor-centred crop and a 3 x 256 fp32 lookup
 * ((v / 255 - mean) / std).  csrc/image_processor.hip: ONE launch does all three, the intermediate image lives in LDS; integers and
 * fp32 only, the same in both storage builds, no atomics (reruns are bit-identical).
 * A plan is host-only: the geometry of one (input size, sheet) under one config, and the coefficient tables the launch reads. */
typedef struct dfh_imgproc_config {
  int shortest_edge;               /* 224: the shorter edge goes here, the other to (int)(shortest_edge * long / short) */
  int crop_height;                 /* 224; 0 (with crop_width 0): no crop, the output is the resized image */
  int crop_width;                  /* 224; top = (h - crop_height) / 2, left = (w - crop_width) / 2 (transformers' rounding) */
  int resample;                    /* PIL numbering: 3 bicubic (a = -0.5) / 2 bilinear */
} dfh_imgproc_config;
typedef struct dfh_imgproc dfh_imgproc;
#define DFH_IMGPROC_SRC_U8_HWC 0   /* uint8 [items][in_h][in_w][3], what np.asarray(pil_image) gives */
#define DFH_IMGPROC_SRC_F32_CHW 1  /* fp32 [items][3][in_h][in_w] in [-1, 1] (vae.decode): quantised as x / 2 + 0.5, clamp to [0, 1], * 255,
                                      round half to even -- difashion.postprocess(.., "pil"); a NaN becomes 0 */
/* in_h, in_w: the size of one source item.  grid_n = 0: every item is an image of its own.  grid_n = n >= 1: output image b reads the
 * virtual g x g sheet (g = ceil(sqrt(n)), row-major, white in the empty cells) of items b * n .. b * n + n - 1 (evalio.image_grid);
 * the sheet is resolved when a pixel is fetched and never materialised.  Refused: an unsupported filter, sizes < 1, a resized image
 * smaller than the crop, a shape whose one-row band does not fit the LDS budget of the kernel. */
int dfh_imgproc_create(const dfh_imgproc_config* cfg, int in_h, int in_w, int grid_n, dfh_imgproc** out);
void dfh_imgproc_destroy(dfh_imgproc* p);
int dfh_imgproc_resized_height(const dfh_imgproc* p);
int dfh_imgproc_resized_width(const dfh_imgproc* p);
int dfh_imgproc_out_height(const dfh_imgproc* p);        /* crop_height, or the resized height without a crop */
int dfh_imgproc_out_width(const dfh_imgproc* p);
int dfh_imgproc_crop_top(const dfh_imgproc* p);
int dfh_imgproc_crop_left(const dfh_imgproc* p);
int dfh_imgproc_ksize_x(const dfh_imgproc* p);           /* taps a row of the horizontal table holds */
int dfh_imgproc_ksize_y(const dfh_imgproc* p);
size_t dfh_imgproc_table_bytes(const dfh_imgproc* p);
/* host_buffer (>= table_bytes) receives int32: bounds_x [resized_w][2] (first tap, tap count), coef_x [resized_w][ksize_x], bounds_y
 * [resized_h][2], coef_y [resized_h][ksize_y]; every |coefficient| < 2^23.  The caller copies it to the device and keeps it. */
int dfh_imgproc_fill_tables(const dfh_imgproc* p, void* host_buffer, size_t buffer_bytes);
/* pixel_values [batch][3][out_h][out_w] fp32 = lut[c][resized, cropped uint8]; out_u8 [batch][out_h][out_w][3] = that uint8 image.
 * Either may be NULL, not both; lut_dev (3 x 256 fp32) may be NULL without pixel_values.  src holds batch * max(grid_n, 1) items.
 * tables_dev, lut_dev, src, pixel_values: 16-byte aligned device pointers.  Nothing is allocated here. */
int dfh_imgproc_run(const dfh_imgproc* p, const void* tables_dev, const float* lut_dev, const void* src, int src_kind, int batch,
                    float* pixel_values, uint8_t* out_u8, void* stream);

/* ------------------------------------------------------------------ the JPEG save / open round trip
 * Replaces (arithmetic) `img.save("<i>.jpg")` of every generated item (inf4eval.py:787-790) followed by `Image.open` where the metrics
 * read it back (evaluate_gor.py:207-215, evaluate_fitb.py): PIL's baseline JPEG through libjpeg's "islow" path in both directions,
 * without the byte stream (entropy coding is lossless).  RGB -> YCbCr, 2 x 2 chroma downsampling, forward DCT, quantisation,
 * dequantisation, inverse DCT with libjpeg's wrapping range limit, "fancy" chroma upsampling, YCbCr -> RGB: 32-bit integers with fixed
 * rounding, equal to PIL bit for bit, the same in both storage builds.  csrc/jpeg.hip: two launches, no atomics, nothing allocated. */
#define DFH_JPEG_SUBSAMPLING_444 0 /* PIL's numbering of `subsampling=` */
#define DFH_JPEG_SUBSAMPLING_420 2
/* Host only: the two quantisation tables libjpeg uses at `quality` (1 .. 100), 64 values each in natural (row-major) order. */
int dfh_jpeg_quant_tables(int quality, int* luma64, int* chroma64);
/* Bytes of the workspace of one call (the decoded Y, Cb, Cr planes, padded to whole tiles); 0 with a message for arguments the round
 * trip refuses. */
size_t dfh_jpeg_workspace_bytes(int batch, int h, int w, int subsampling);
/* int16 elements `coef` receives: 64 for every real block, batch * (ceil(h/8) * ceil(w/8) + 2 * chroma blocks). */
size_t dfh_jpeg_coef_count(int batch, int h, int w, int subsampling);
/* src: uint8 [batch][h][w][3] (src_kind DFH_IMGPROC_SRC_U8_HWC) or fp32 [batch][3][h][w] in [-1, 1] (DFH_IMGPROC_SRC_F32_CHW, quantised
 * as dfh_imgproc_run does).  dst_hwc: uint8 [batch][h][w][3].  coef (may be NULL): the quantised coefficients, int16 in natural order,
 * [batch][Y, Cb, Cr][block row][block column][64], real blocks only (the dummy blocks that fill an MCU are not part of it).
 * Refused on the host before any launch: quality outside 1 .. 100, a subsampling other than the two above, batch / h / w below 1, a null
 * pointer or one that is not 16-byte aligned, a workspace smaller than dfh_jpeg_workspace_bytes, dst_hwc overlapping src. */
int dfh_jpeg_roundtrip(const void* src, int src_kind, int batch, int h, int w, int quality, int subsampling, uint8_t* dst_hwc, int16_t* coef,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------ LPIPS on VGG16
 * Replaces (arithmetic) lpips.LPIPS(net="vgg", version="0.1", spatial=False) as Evaluation/eval_utils.py:473-501 and :769-821 call it:
 * the ScalingLayer, torchvision's vgg16().features up to relu5_3 (thirteen 3x3 convolutions with ReLU, four 2x2 max-pools), per tap
 * layer the unit-normalised squared difference under the 1x1 "lin" weights and its spatial mean, and the sum of the five layers.
 * csrc/lpips.hip: fp32 end to end, the same in both storage builds, convolutions on v_mfma_f32_16x16x4_f32 as an implicit GEMM over
 * NHWC activations; no atomics, nothing allocated; a pair's result does not depend on the batch it rides in.
 * The convolution adds up one input-channel chunk of 32 (x 9 taps) in fresh accumulators and adds that to the running sum.
 * Parameters, DFH_LPIPS_NUM_PARAMS = 33, in this order (the names of the lpips package's state dict):
 *   scaling_layer.shift, scaling_layer.scale                                    [1][3][1][1]
 *   net.slice{1..5}.{0,2 | 5,7 | 10,12,14 | 17,19,21 | 24,26,28}.{weight,bias}  [C_out][C_in][3][3], [C_out]
 *   lin{0..4}.model.1.weight                                                    [1][C][1][1], C = 64, 128, 256, 512, 512 */
#define DFH_LPIPS_NUM_PARAMS 33
#define DFH_LPIPS_NUM_LAYERS 5
#define DFH_LPIPS_PARTIALS 256     /* partial sums a (pair, layer) in the workspace */
#define DFH_LPIPS_NET_VGG16 0
#define DFH_LPIPS_SRC_U8_HWC 0     /* uint8 [n][H][W][3]: lut[v] = float32(float64(v) / 127.5 - 1.0) (im2tensor_lpips), 256 fp32 */
#define DFH_LPIPS_SRC_F32_CHW 1    /* fp32 [n][3][H][W] in [-1, 1], the lpips input form; normalize != 0: 2 x - 1 first ([0, 1] input) */
typedef struct dfh_lpips_config {
  int net;                         /* DFH_LPIPS_NET_VGG16; every other network is refused */
} dfh_lpips_config;
typedef struct dfh_lpips dfh_lpips;
int dfh_lpips_create(const dfh_lpips_config* cfg, dfh_lpips** out);   /* host-only work */
void dfh_lpips_destroy(dfh_lpips* c);
int dfh_lpips_num_params(const dfh_lpips* c);
const char* dfh_lpips_param_name(const dfh_lpips* c, int i);
int dfh_lpips_param_ndim(const dfh_lpips* c, int i);
int dfh_lpips_param_dim(const dfh_lpips* c, int i, int d);
/* The packed conv weights, [chunk][tap][channel][C_out] a layer (chunks of 32 input channels; the first layer is one chunk of 4, its
 * fourth channel 0): 4 * sum over the thirteen convs of 9 * C_in_padded * C_out bytes = 58 844 160. */
size_t dfh_lpips_packed_bytes(const dfh_lpips* c);
int dfh_lpips_pack(dfh_lpips* c, const float* const* params, int count, void* packed, void* stream);
/* Two ping-pong activation buffers of 2 * pairs images at the widest level (64 channels at H x W) + the partial sums:
 *   4 * (2 * (2 * pairs * H * W * 64) + pairs * DFH_LPIPS_NUM_LAYERS * DFH_LPIPS_PARTIALS) + 256 bytes; 0 for H or W outside [16, 8192] */
size_t dfh_lpips_workspace_bytes(const dfh_lpips* c, int pairs, int H, int W);
/* distance[p] = lpips(in0[p], in1[p]), p < pairs; per_layer: NULL, or [pairs][5], distance[p] = per_layer[p][0] + ... + [4] in that order.
 *   params   : HOST array of `count` device pointers to the fp32 parameters, table order, each 16-byte aligned
 *   packed   : what dfh_lpips_pack wrote (>= dfh_lpips_packed_bytes)
 *   in0, in1 : `pairs` images each in the form src_kind; lut: the 256-entry table of the uint8 form, else NULL
 *   workspace: >= dfh_lpips_workspace_bytes(pairs, H, W), 256-byte aligned
 * Refused on the host before any HIP call, with a message each: a wrong count; a null pointer and a pointer that is not 16-byte
 * aligned, by name; H or W below 16 (the fifth level would be empty); a workspace that is too small. */
int dfh_lpips_forward(dfh_lpips* c, const float* const* params, int count, const void* packed, const void* in0, const void* in1, int src_kind,
                      const float* lut, int normalize, int pairs, int H, int W, float* distance, float* per_layer, void* workspace,
                      size_t workspace_bytes, void* stream);
/* pred[r] = argmin_k scores[r * K + k] in torch.argmin's order: a NaN is the minimum, the lowest index wins among equals */
int dfh_lpips_group_argmin(const float* scores, int64_t* pred, int rows, int K, void* stream);
/* The kernels of the walk on their own (tests, microbenchmarks).  Activations are NHWC fp32.
 * prep: out [n][H][W][4] = ((x - shift[c]) / scale[c], 0), bit for bit torch's ops.
 * conv3x3_relu: out [n][H][W][C_out] = relu(conv2d(x [n][H][W][C_in], weight [C_out][w_cin][3][3], bias, padding=1)); C_in is 4 or a
 *   multiple of 32, C_out a multiple of 64, input channels from w_cin up carry zero weights; packed: 9 * C_in * C_out floats.
 * maxpool2x2: out [n][H/2][W/2][C], floor mode, a NaN propagates.
 * layer_score: out[p] = mean over the pixels of sum_c w_c (x_c / (|x| + 1e-10) - y_c / (|y| + 1e-10))^2 for x = feat[p], y = feat[pairs + p],
 *   feat [2 pairs][H][W][C], C <= 512; partial: pairs * DFH_LPIPS_PARTIALS floats. */
int dfh_lpips_prep(const void* src, int src_kind, const float* lut, const float* shift, const float* scale, int normalize, float* out, int n,
                   int H, int W, void* stream);
int dfh_lpips_conv3x3_relu(const float* x, const float* weight, int w_cin, const float* bias, float* packed, float* out, int n, int H, int W,
                           int C_in, int C_out, void* stream);
int dfh_lpips_maxpool2x2(const float* x, float* out, int n, int H, int W, int C, void* stream);
int dfh_lpips_layer_score(const float* feat, const float* lin_weight, int pairs, int H, int W, int C, float* partial, float* out, void* stream);

/* ------------------------------------------------------------------ Inception v3: FID and the Inception Score
 * Replaces (arithmetic) the two networks of Evaluation/eval_utils.py: pytorch_fid's FIDInceptionV3 (:137-280, variant FID) and
 * torchvision's inception_v3 under the fine-tuned classifier (:17-89, variant TV), the per-image entropy / KL terms of the customised
 * Inception Score (:382-398) and np.mean / np.cov of the activations (:318-319).  csrc/inception.hip: fp32 NHWC in both storage builds,
 * every convolution ONE implicit-GEMM kernel on v_mfma_f32_16x16x4_f32 with BatchNorm folded to a per-channel scale / shift and ReLU in
 * the epilogue, written into a channel slice of the concatenated output; the statistics on v_mfma_f64_16x16x4_f64.  No atomics, nothing
 * allocated; every per-image value is a function of its image alone.
 * The convolution sums K = KH * KW * C_in in k-tiles of 32: each tile in fresh accumulators, added to the running sum with a compensated
 * (Kahan) add (f32_tile.h TileKahanSum), so the rounding error does not grow with K (up to 4032 here).
 * Parameters under torchvision's state-dict names, per BasicConv2d <layer>.conv.weight [C_out][C_in][KH][KW], <layer>.bn.weight, .bn.bias,
 * .bn.running_mean, .bn.running_var [C_out], in torchvision's module order (AuxLogits left out), then for TV fc.weight [classes][2048],
 * fc.bias: 94 convolutions -> 470 entries (FID), 472 (TV). */
#define DFH_INCEP_VARIANT_TV 0       /* torchvision: transform_input, avg pools count the padding, fc + softmax */
#define DFH_INCEP_VARIANT_FID 1      /* pytorch_fid: avg pools leave the padding out, Mixed_7c pools with max, no fc */
#define DFH_INCEP_NUM_CONVS 94
#define DFH_INCEP_NUM_BLOCKS 4       /* taps: 64 after maxpool1, 192 after maxpool2, 768 after Mixed_6e, 2048 after the global average */
#define DFH_INCEP_SIDE 299
/* launch kinds of the plan */
#define DFH_INCEP_K_PREP 0
#define DFH_INCEP_K_CONV 1
#define DFH_INCEP_K_POOL 2
#define DFH_INCEP_K_GMEAN 3
#define DFH_INCEP_K_FC 4
#define DFH_INCEP_K_SOFTMAX 5
/* pool modes */
#define DFH_INCEP_POOL_MAX_S2 0      /* max_pool2d(3, 2) */
#define DFH_INCEP_POOL_MAX_S1 1      /* max_pool2d(3, 1, 1) */
#define DFH_INCEP_POOL_AVG_INCL 2    /* avg_pool2d(3, 1, 1), count_include_pad=True: always / 9 */
#define DFH_INCEP_POOL_AVG_EXCL 3    /* avg_pool2d(3, 1, 1, count_include_pad=False): / the pixels inside the image */
/* regions of a launch's source / destination */
#define DFH_INCEP_REGION_INPUT (-1)  /* the caller's images */
#define DFH_INCEP_REGION_TAP (-2)    /* the caller's taps[block] */
#define DFH_INCEP_REGION_PROBS (-3)  /* the caller's probs */
typedef struct dfh_incep_config {
  int variant;                       /* DFH_INCEP_VARIANT_* */
  int num_classes;                   /* TV: width of fc (1 .. 4096); FID: ignored */
  int resize_input, normalize_input; /* bilinear to 299 x 299; 2 x - 1 */
  int block_mask;                    /* bit b: tap b is written; the walk stops after the highest bit.  TV: bit 3 is required (the classifier) */
} dfh_incep_config;
typedef struct dfh_incep_launch {
  int kind, conv, pool_mode, block;  /* conv: index into the layer list or -1; block: the tap of a GMEAN or -1 */
  int KH, KW, stride, padH, padW;
  int Hin, Win, Cin, Hout, Wout, Cout, ldc, offset;      /* the output is channels [offset, offset + Cout) of a tensor with ldc channels */
  int src_region, dst_region;        /* workspace region 0 .. 3 (4: the logits) or DFH_INCEP_REGION_* */
  size_t src_off, src_floats, dst_off, dst_floats;       /* in floats from the workspace base: the launch reads / writes inside [off, off + floats) */
  char name[48];                     /* the layer (state-dict prefix) or the pool / head step */
} dfh_incep_launch;
typedef struct dfh_incep dfh_incep;
int dfh_incep_create(const dfh_incep_config* cfg, dfh_incep** out);   /* host-only work */
void dfh_incep_destroy(dfh_incep* c);
int dfh_incep_num_params(const dfh_incep* c);
const char* dfh_incep_param_name(const dfh_incep* c, int i);
int dfh_incep_param_ndim(const dfh_incep* c, int i);
int dfh_incep_param_dim(const dfh_incep* c, int i, int d);
/* Per convolution [C_out][KH * KW * C_in_padded] weights (k = tap * C_in_padded + channel; the first layer's three channels padded to
 * four), then scale [C_out] = bn.weight / sqrt(running_var + 1e-3) and shift [C_out] = bn.bias - running_mean * scale. */
size_t dfh_incep_packed_bytes(const dfh_incep* c);
int dfh_incep_pack(dfh_incep* c, const float* const* params, int count, void* packed, void* stream);
/* The launch plan of n images of H x W: pure host arithmetic.  count: the number of launches, negative on a refusal. */
int dfh_incep_plan_count(const dfh_incep* c, int n, int H, int W);
int dfh_incep_plan_entry(const dfh_incep* c, int n, int H, int W, int i, dfh_incep_launch* out);
/* Four activation regions, each the largest tensor the plan puts there, + n * num_classes logits (TV), + 256 bytes; 0 on a refusal. */
size_t dfh_incep_workspace_bytes(const dfh_incep* c, int n, int H, int W);
/* in: fp32 [n][3][H][W]; taps: HOST array of DFH_INCEP_NUM_BLOCKS device pointers, taps[b] = [n][64 | 192 | 768 | 2048] for every bit
 * of block_mask (the spatial mean of the block's output; others ignored); probs: TV [n][num_classes] softmax, FID NULL.
 * Refused on the host before any HIP call: a wrong count, a null / misaligned pointer by name, a missing tap, a small workspace,
 * without resize_input a side below 75 (Mixed_7a would be empty). */
int dfh_incep_forward(dfh_incep* c, const float* const* params, int count, const void* packed, const float* in, int n, int H, int W,
                      float* const* taps, float* probs, void* workspace, size_t workspace_bytes, void* stream);
/* The kernels on their own (tests, microbenchmarks).  Activations are NHWC fp32.
 * prep: out [n][OH][OW][4], (OH, OW) = resize ? (299, 299) : (H, W); affine != 0: TV's transform_input after 2 x - 1.
 * conv_bn_relu: out[.., offset : offset + C_out] of [n][OH][OW][ldc] = relu(batch_norm(conv2d(x [n][H][W][C_in], weight
 *   [C_out][w_cin][KH][KW], stride, (padH, padW)), eps 1e-3)); bn: weight, bias, running_mean, running_var; C_in a multiple of 4, input
 *   channels from w_cin up carry zero weights; packed: C_out * (KH * KW * C_in + 2) floats.
 * pool: the four 3 x 3 pools into a channel slice; C, ldc, offset multiples of 4.
 * global_mean: out [n][C] = the mean over the H * W pixels, summed in fp64 in a fixed order.
 * fc_softmax: probs [n][classes] = softmax(feat [n][K] . weight [classes][K]^T + bias); logits: n * classes floats of scratch.
 * is_rows: per image label = argmax (the lowest index among equals, a NaN wins), ent = -sum p log(p + eps),
 *   kl = sum p (log(p + eps) - log(1 / classes)), correct = (label == cate) (cate NULL: 0).
 * is_splits: out [splits][3] = (mean ent, exp(mean kl), sum correct) over images [s N / splits, (s + 1) N / splits), in index order.
 * stats: mu [D] = np.mean(act, 0), sigma [D][D] = np.cov(act, rowvar=False) of the float64 copy of act [N][D] (two-pass, / (N - 1));
 *   N >= 2; sigma is written symmetric. */
int dfh_incep_prep(const float* src, int n, int H, int W, int resize, int normalize, int affine, float* out, void* stream);
int dfh_incep_conv_bn_relu(const float* x, const float* weight, int w_cin, const float* const* bn, float* packed, float* out, int n, int H, int W,
                           int C_in, int C_out, int KH, int KW, int stride, int padH, int padW, int ldc, int offset, void* stream);
int dfh_incep_pool(const float* x, float* out, int mode, int n, int H, int W, int C, int ldc, int offset, void* stream);
int dfh_incep_global_mean(const float* x, float* out, int n, int HW, int C, void* stream);
int dfh_incep_fc_softmax(const float* feat, const float* weight, const float* bias, float* logits, float* probs, int n, int K, int classes,
                         void* stream);
int dfh_incep_is_rows(const float* probs, const int64_t* cate, int n, int classes, float eps, int64_t* label, float* ent, float* kl,
                      float* correct, void* stream);
int dfh_incep_is_splits(const float* ent, const float* kl, const float* correct, int n, int splits, float* out, void* stream);
int dfh_incep_stats(const float* act, int N, int D, double* mu, double* sigma, void* stream);

/* ------------------------------------------------------------------ op-level entry points (tests, profiling)
 * ResnetBlock2D conv3x3 / Downsample2D / Upsample2D / 1x1 conv / Linear, as one implicit GEMM:
 *   out[M][N] = act( conv3x3(x) (+ a0 . W[:, k0:] + a1 . W[:, k1:]) + bias + rowvec[b] ) + resid */
typedef struct dfh_gemm_desc {
  const void* conv_src; int conv_c; int conv;   /* conv != 0: 3x3 pad 1 over NHWC bf16 [B][Hin][Win][conv_c] */
  int batch, Hin, Win, stride, upsample;        /* stride 1|2; upsample: nearest 2x before the conv */
  const void* a0; int a0_c; const void* a1; int a1_c; /* plain K segments, rows [M][c] bf16 */
  const void* W; int ldw;                       /* bf16 [N][ldw], K-contiguous, segments in the order above */
  int M, N;
  const float* bias;                            /* [N] or NULL */
  const float* rowvec; int rv_ld, rv_off, rows_per_b;  /* + rowvec[m / rows_per_b][rv_off + n] (time embedding) */
  const void* resid; int ld_res;                /* + resid[m][n] bf16 */
  int act;                                      /* 0 none 1 silu 2 leaky_relu(0.01) 3 tanh 4 GEGLU (W/bias pre-interleaved); 5 gelu (exact erf)
                                                 * 6 quick_gelu (x sigmoid(1.702 x)): plain linears, 16-bit row-major output, N and ld_out
                                                 * multiples of 8, always the eight-wave 128x160 tile in a single pass (force ids ignored) */
  void* out; int ld_out; int out_mode;          /* 0 bf16 [M][ld] 1 bf16 [b][N][ld] 2 fp32 [M][ld] 3 fp32 [b][N][ld] */
  float* partial; size_t partial_floats;        /* split-K slabs (dfh_gemm_partial_floats) */
  const void* zero_page;                        /* >= 256 zero bytes */
  int force_tile, force_split, force_order;     /* 0,0,-1 = heuristics; force_order 2 / 3 = tile ids n-major / m-major.  force_tile (GemmForceTile,
                                                 * gemm.h): 1-5 gemm_bf16_kernel tiles 256x160 / 256x128 / 128x64 / 128x160 / 128x128; 6 the wide
                                                 * 256x160 kernel, 9 its 256x128 sibling; 10 the eight-wave 128x160 tile; 21 the 256x320 tile; 23 the
                                                 * 256x256 GEGLU tile; probe library only (refused here): 7 / 8 wide experiment tiles, 11 / 12
                                                 * wave-specialised, 13-18 k-loop ablations, 20 halo conv, 24 persistent 128x160, 30 token linear */
  float* gstat; int gstat_cpg, gstat_hw;        /* optional: GroupNorm statistics of the output for the consumer (channels per group,
                                                 * pixels per image): [image][group][hw / rows][2] sums / sums of squares, rows = 256
                                                 * or 128 (dfh_gemm_gstat reports which); only through dfh_gemm_gstat (dfh_gemm ignores the three fields) */
  size_t w_img_stride;                          /* 0, or per-IMAGE weights: rows [i * rows_per_b, (i + 1) * rows_per_b) multiply W + i * w_img_stride
                                                 * (elements) -- dfh_groupnorm_fold; 128-row-tile launches without conv taps / split-K */
} dfh_gemm_desc;
size_t dfh_gemm_partial_floats(const dfh_gemm_desc* d);
int dfh_gemm(const dfh_gemm_desc* d, void* stream);
/* dfh_gemm + the output statistics for the consuming GroupNorm (d->gstat ..., sized for gstat_hw / 128 chunks); *written = the pixel rows
 * per statistics chunk they were produced with (256 or 128: pass gstat_hw / *written as the chunk count to dfh_groupnorm_pre), 0 when the
 * launch ran on a kernel that cannot (the caller then runs plain dfh_groupnorm) */
int dfh_gemm_gstat(const dfh_gemm_desc* d, void* stream, int* written);
/* GroupNorm folded into the 1x1 projection that consumes it (transformer entry, difashion.py:249-253): from x [B][HW][C] (statistics: the
 * producer's partials `pre` [B][G][pre_chunks][2], or NULL -> summed here into `partial`, >= B * 64 * G * 2 floats), gamma / beta and the
 * projection W [N][ldw] (+ bias) it writes per-image weights Wimg [B][N][C] = bf16(W gamma rstd) and the row vectors rv [B][N] =
 * bias + W . beta - Wimg . mean; then  proj(GroupNorm(x)) = dfh_gemm(a0 = x, W = Wimg, w_img_stride = N * C, rowvec = rv, rows_per_b = HW). */
int dfh_groupnorm_fold(const void* x, int B, int HW, int C, int G, const float* gamma, const float* beta, float eps, const float* pre,
                       int pre_chunks, float* partial, const void* W, int ldw, int N, const float* bias, void* Wimg, float* rv, void* stream);
/* Weight gradient of the same op (train.py:699 backward): dW[n][k] += sum_m dY[m][n] * A[m][k], where A is the
 * forward operand described by d (conv_src / a0 / a1 segments, M, N, zero_page; W / out / epilogue fields unused).
 * dW: fp32 [N][ldw] in the PACKED weight layout, accumulated (dW += ...; the sum over pixel slices is a fixed-order slab reduce, so
 * reruns are bit-identical).  msplit: 0 = the launcher's plan; n > 0 = n equal pixel slices of every 160 x 160 output tile;
 * -n = whole tiles in full rounds of 512 blocks and the remaining tiles in n slices. */
int dfh_gemm_wgrad(const dfh_gemm_desc* d, const void* dY, int ldy, float* dW, int ldw, int msplit, void* stream);
/* fp32 slab floats (d->partial / d->partial_floats) that call needs when it splits the pixel range; 0 = none */
size_t dfh_gemm_wgrad_partial_floats(const dfh_gemm_desc* d, int msplit);
/* the decomposition that call would launch (host code, no GPU needed): output tiles, how many of them run whole, pixel slices of the rest */
int dfh_gemm_wgrad_plan(const dfh_gemm_desc* d, int msplit, int* tiles, int* whole_tiles, int* slices);
/* The launch dfh_gemm / dfh_gemm_gstat / dfh_gemm_ln / dfh_gemm_out2 / dfh_gemm_batched would make for d (host code, no GPU needed, nothing is
 * launched; pointers of d are only tested for presence, W / out / zero_page / partial may be NULL): which kernel, tile, K split, tile order
 * and statistics chunk.  x (may be NULL) carries what a descriptor cannot say; d->gstat_cpg / gstat_hw > 0 ask for GroupNorm statistics.
 * Returns 0 and the plan, or the refusal the launch would meet (dfh_last_error); out->line holds either as the text line that
 * DFH_GEMM_PLAN_DUMP=<file> appends per launch. */
typedef struct dfh_gemm_plan_extra {
  int nbatch;        /* > 1: planes of a batched launch (dfh_gemm_batched, the Winograd planes) */
  int phase2x;       /* 1: the four phase planes of an upsample conv (dfh_conv_up2x); d describes the 3x3 conv over the SOURCE image */
  int w_blocked;     /* W in 16 x 64 blocks (dfh_wino_blocked) */
  int n_split;       /* > 0: a second destination from column n_split on (dfh_gemm_out2) */
  int want_rowstat;  /* row statistics for a folded LayerNorm (dfh_gemm_ln as producer) */
  int ln_cnt;        /* > 0: a folded-LayerNorm consumer whose producer wrote column tiles of ln_cnt (dfh_gemm_ln as consumer) */
  int pre_out;       /* the GEGLU pre-activations as a second output (training walk) */
} dfh_gemm_plan_extra;
typedef struct dfh_gemm_plan_info {
  int kernel;        /* 0 gemm_bf16_kernel tile, 1 its 256 x 320 tile, 2 its 256 x 256 GEGLU tile, 3 gemm_wide_kernel, 4.. probe kernels */
  int tile;          /* gemm_bf16_kernel tile index (force_tile - 1; 5 = the eight-wave 128 x 160 tile) */
  int bm, bn, stages, lean;
  int wide;          /* gemm_wide_kernel variant (1 = 256 x 160, 4 = 256 x 128, 5 = 256 x 128 with pre_out) */
  int split;         /* K slices; > 1: the split-K reduce follows */
  int n_major, tm_xm, tm_gm;
  int gstat_rows;    /* pixel rows per statistics chunk (dfh_gemm_gstat's *written), 0 = the kernel cannot write them */
  int rowstat_bn;    /* dfh_gemm_ln's *rowstat_bn */
  int census;        /* index of the dfh_census_* counter the launch bumps */
  char line[512];
} dfh_gemm_plan_info;
int dfh_gemm_plan(const dfh_gemm_desc* d, const dfh_gemm_plan_extra* x, dfh_gemm_plan_info* out);
/* out[g][n] += sum over the rows of group g of Y[m][n] (bias gradient: groups = 1; time-embedding gradient:
 * groups = batch, rows_per_group = H*W). */
int dfh_colsum(const void* Y, int ldy, int N, int groups, int rows_per_group, float* out, int ld_out, void* stream);

/* GroupNorm(32, C, eps)(+SiLU) over NHWC bf16, optional fused channel concat of two sources
 * (ResnetBlock2D.norm1/norm2, conv_norm_out, Transformer2DModel.norm).  partial: >= B*64*G*2 floats */
int dfh_groupnorm(const void* src0, int c0, const void* src1, int c1, int batch, int hw, int groups,
                  const float* gamma, const float* beta, float eps, int silu, void* out, float* partial, void* stream);
/* the same with the statistics supplied by the producing dfh_gemm (gstat, chunks = hw / 256): one launch, the tensor is read once */
int dfh_groupnorm_pre(const void* src, int c, int batch, int hw, int groups, const float* gamma, const float* beta, float eps,
                      int silu, void* out, const float* gstat, int chunks, float* stats_out, void* stream);
/* LayerNorm over the last dim of [M][C] bf16 (BasicTransformerBlock.norm1/2/3) */
int dfh_layernorm(const void* x, const float* gamma, const float* beta, void* y, int M, int C, float eps, void* stream);
/* dfh_gemm with a SECOND destination: output columns [n_split, N) leave transposed per batch of d->rows_per_b rows into out2
 * ([batch][N - n_split][ld_out2] bf16), columns [0, n_split) into d->out as usual -- attention's q | k and V^T from one launch over the
 * rows both projections share (diffusers Attention.to_q / to_k / to_v of attn1).  Fails when the launch heuristics would split K or
 * pick a column tile that does not divide n_split. */
int dfh_gemm_out2(const dfh_gemm_desc* d, void* out2, int ld_out2, int n_split, void* stream);
/* ---- LayerNorm folded into the projections around it (inference walk of BasicTransformerBlock: x + attn1(LN1(x)), + attn2(LN2(x)),
 * + ff(LN3(x)); reached from df.py:518-523).  LN(x) . W^T = rstd * (x . W'^T - mean * s) + b' with W' = W * gamma, s = rowsum(W'),
 * b' = bias + W . beta: the consumer GEMM runs on the raw rows and fixes them up in its epilogue, the statistics come from the
 * epilogue of the GEMM that produced x -- no LayerNorm launch, no normalised copy of the tensor in HBM.
 *   dfh_ln_fold : packed bf16 W [N][ldw] -> WF [N][K] bf16, s [N], b [N] (bias may be NULL)
 *   dfh_gemm_ln : dfh_gemm plus, as producer, rowstat (per output row and column tile (mean, centred sum of squares),
 *                 [N / bn][M][2] floats; *rowstat_bn = bn, 0 when this launch could not write them) and / or, as consumer, ln_stat =
 *                 the producer's rowstat (ln_parts column tiles of ln_cnt columns each), ln_s = s, d->bias = b', d->W = WF */
int dfh_ln_fold(const void* W, int ldw, const float* gamma, const float* beta, const float* bias, void* WF, float* s, float* b, int N, int K,
                void* stream);
int dfh_gemm_ln(const dfh_gemm_desc* d, float* rowstat, int* rowstat_bn, const float* ln_stat, int ln_parts, int ln_cnt, float ln_eps,
                const float* ln_s, void* stream);
/* ---- nearest-2x upsample + 3x3 conv (diffusers Upsample2D: F.interpolate(scale_factor=2, mode="nearest") then conv, the up-block
 * upsamplers reached from df.py:518-523) as FOUR 2x2 convs over the source image: output pixel (2y + py, 2x + px) sees source rows
 * {y - 1 + py, y + py} and columns alike, each with the sum of the 3x3 taps that land on it -- 4/9 of the multiply-adds.
 *   dfh_ups_phase_fold : packed bf16 W [N][ldw >= 9 C] (tap-major columns) -> WP [4][N][4 C] bf16, the summed taps per phase py * 2 + px
 *   dfh_conv_up2x      : src [batch][H][W][C] bf16 -> out [batch][2H][2W][N] bf16 = conv3x3(upsample2x(src)) + bias, one launch */
int dfh_ups_phase_fold(const void* W, int ldw, void* WP, int N, int C, void* stream);
int dfh_conv_up2x(const void* src, int batch, int H, int W, int C, const void* WP, int N, const float* bias, void* out,
                  const void* zero_page, void* stream);
/* ---- Winograd F(2x2, 3x3) for stride-1 3x3 convs (ResnetBlock2D.conv1 / conv2 at the deep levels; df.py:249-253,518-523): sixteen
 * transform-domain GEMMs over the 2x2 output tiles instead of nine taps per pixel (2.25 x fewer multiply-adds), U / V / M rounded to bf16.
 *   dfh_wino_weights : packed bf16 W [N][ldw >= 9 C] -> U [16][N][C] bf16 (G g G^T, fp32 arithmetic, rounded once)
 *   dfh_conv3x3_wino : src [batch][H][W][C] bf16 (H, W even) -> out [batch][H][W][N] bf16 = conv3x3(src) + bias (+ rowvec row of the
 *                      image: rowvec[b * rv_ld + rv_off + n]) (+ resid [batch][H][W][N] bf16); three launches (input transform, one
 *                      batched GEMM, output transform) over `scratch` (dfh_conv3x3_wino_scratch_bytes, 256-byte aligned) */
int dfh_wino_weights(const void* W, int ldw, void* U, int N, int C, int blocked, void* stream);
/* the input transform alone: src [batch][H][W][C] bf16 -> V [16][batch * H/2 * W/2][C] bf16 = B^T d B per 4x4 patch (stride 2, zero padded);
 * dfh_gn_wino_input: the same over silu(GroupNorm(concat(src0, src1))) (ResnetBlock2D.norm1 / norm2 + nonlinearity in front of the conv),
 * one launch, the normalised tensor never goes to HBM; dfh_gn_wino_input_ok tells whether the (image, group) slab fits the kernel */
int dfh_wino_input(const void* src, void* V, int batch, int H, int W, int C, void* stream);
int dfh_gn_wino_input_ok(int c0, int c1, int groups, int H, int W);
int dfh_gn_wino_input(const void* src0, int c0, const void* src1, int c1, const float* gamma, const float* beta, float eps, int groups,
                      void* V, int batch, int H, int W, void* stream);
/* conv1 -> conv2 of a ResnetBlock2D: the tensor between the two convs is rebuilt from conv1's transform-domain planes Mprev [16][batch H W / 4][C]
 * (A^T m A + pbias + the image's row prowvec[b * prv_ld + prv_off + c], rounded to bf16 as the stored tensor would be) inside conv2's
 * GroupNorm + input transform: no output-transform launch, no round trip of that tensor */
int dfh_gn_wino_input_chain(const void* Mprev, const float* pbias, const float* prowvec, int prv_ld, int prv_off, int C, const float* gamma,
                            const float* beta, float eps, int groups, void* V, int batch, int H, int W, void* stream);
/* 1 when the library stores U of an N x C conv in 16-row x 64-column blocks ([16][N / 16][C / 64][16][64]: every 2-KB DRAM burst of the
 * weight stream is used whole); pass the same value as `blocked` / `u_blocked` */
int dfh_wino_blocked(int N, int C);
size_t dfh_conv3x3_wino_scratch_bytes(int batch, int H, int W, int C, int N);
int dfh_conv3x3_wino(const void* src, int batch, int H, int W, int C, const void* U, int u_blocked, int N, const float* bias, const float* rowvec,
                     int rv_ld, int rv_off, const void* resid, void* out, void* scratch, size_t scratch_bytes, const void* zero_page,
                     void* stream);
/* dfh_gemm over nbatch independent planes in ONE launch (grid.y): plane z reads d->a0 + z * a_bs, d->W + z * w_bs and writes
 * d->out + z * o_bs (strides in bf16 elements).  One plain K segment, bias-only epilogue, bf16 row-major output, no split-K. */
int dfh_gemm_batched(const dfh_gemm_desc* d, int nbatch, long a_bs, long w_bs, long o_bs, void* stream);
/* ---- fp8 (OCP e4m3fn) linears: BASELINE configs[4].  The reference has no fp8 path (fp16 autocast, run_inf4eval.sh:1); these
 * replace the same diffusers linears as dfh_gemm (BasicTransformerBlock attn1.to_q/k/v, attn2.to_q, ff.net.0.proj reached from
 * df.py:249-253,518-523) when the caller opts in.
 *   dfh_quantize_rows_fp8 : bf16 [R][K] (row stride ldx) -> e4m3 [R][K] + scale[R] = amax / 448 (weights: one scale per output channel)
 *   dfh_layernorm_fp8     : dfh_layernorm whose output is quantised per token: q [M][C] e4m3, scale [M]
 *   dfh_gemm_fp8          : out = epilogue(sa(m) * sW[n] * sum_k 2^(sx[k / 32][m] - 127) A[m][k] W[n][k]); K % 64 == 0; act 0 or 4
 *                           (GEGLU, packed rows).  Activation scales, any combination: sA (a float per group of sa_div rows: per token,
 *                           or per image), sa_mul (a constant), sx (E8M0 block scales per row and 32 contraction elements, the
 *                           hardware's scale operand; layout [K / 32][M] bytes).  out_mode 0 (bf16 [M][ld_out]), 1 (bf16 transposed per
 *                           batch of rows_per_b rows; amax != NULL: amax[b] = max(amax[b], max |out| of batch element b), the
 *                           caller zeroes it) or 4 (e4m3 [M][ld_out] + E8M0 block scales of the OUTPUT in out_sx [N_out / 32][M]:
 *                           the operand of the next fp8 GEMM, e.g. the GEGLU hidden tensor for ff.net.2).  Zero-initialise the descriptor.
 *   dfh_groupnorm_fp8     : GroupNorm WITHOUT its affine, as e4m3: q = e4m3(clamp((x - mean) * rstd * q_mul)) -- the operand of an fp8
 *                           proj_in whose weights carry gamma (and whose bias carries W . beta): a static scale, no statistics of q needed
 *   dfh_attention_fp8out  : dfh_attention whose output leaves as e4m3 scaled by 448 / v_amax[b] (|O| <= max |V| of the batch element)
 *   dfh_amax_slabs        : out[s][b] = max |x| over rows row0[s] .. + nrows[s] of batch element b of a bf16 [B][.][ld] tensor */
typedef struct dfh_gemm_fp8_desc {
  const void* A; int lda;                    /* e4m3 [M][lda]; lda 0 = K */
  const float* sA; int sa_div; float sa_mul;
  const void* sx;
  const void* W; const float* sW;            /* e4m3 [N][K], one scale per output channel */
  int M, N, K;
  const float* bias; const void* resid; int ld_res; int act;
  void* out; int ld_out; int out_mode; void* out_sx; int rows_per_b; float* amax;
  const void* zero_page;
} dfh_gemm_fp8_desc;
int dfh_quantize_rows_fp8(const void* x, int ldx, void* q, float* scale, int R, int K, void* stream);
int dfh_layernorm_fp8(const void* x, const float* gamma, const float* beta, void* q, float* scale, int M, int C, float eps, void* stream);
int dfh_gemm_fp8(const dfh_gemm_fp8_desc* d, void* stream);
/* Fused GEGLU feed-forward + proj_out of a transformer block at C = 320 (csrc/mlp_fused2.hip; replaces the ff.net.0 / ff.net.2 / proj_out
 * launches of diffusers BasicTransformerBlock.ff + Transformer2DModel.proj_out at the 64x64 level, reference call site
 * DiFashion/models/difashion.py:518-523):  out = [pout . ff2 | pout] . [GEGLU(LN3(x) . W1^T + b1) | x] + bias + resid.
 *   dfh_mlp_fused_pack : builds the layer's weight image (dfh_mlp_fused_image_bytes() bytes) from the LayerNorm-folded GEGLU projection
 *                        w1 ([8 C][C] bf16, rows packed 16 values | 16 gates; s1 / b1 its fold vectors, dfh_ln_fold) and w2p = [C][5 C]
 *   dfh_mlp_fused      : x / resid / out [M][320] bf16, M a multiple of 128; ln_stat = per-row statistics of x ([ln_parts][M][2]: mean
 *                        and centred sum of squares per column tile of ln_cnt columns, as dfh_gemm's row statistics) */
size_t dfh_mlp_fused_image_bytes(void);
/* form: 2 = the kernel (eight waves of 16 tokens on v_mfma_f32_16x16x32_bf16, two per SIMD).  1 = its first form (four waves of 32 tokens, one per
 * SIMD) exists in the probe library only (scripts/probes); an image packed for one form is only valid for that form */
int dfh_mlp_fused_pack(const void* w1, const float* s1, const float* b1, const void* w2p, void* img, int form, void* stream);
/* gstat (form 2, may be NULL): GroupNorm statistics of out for its consumer, [image][320 / gstat_cpg][gstat_hw / 128][2] = (sum, sum of squares) of
 * the bf16-rounded outputs per (image of gstat_hw tokens, group of gstat_cpg channels, 128-token chunk) */
int dfh_mlp_fused(const void* x, const void* resid, const void* img, const float* ln_stat, int ln_parts, int ln_cnt, float ln_eps,
                  const float* bias, void* out, int M, int form, float* gstat, int gstat_cpg, int gstat_hw, void* stream);
int dfh_groupnorm_fp8(const void* src, int batch, int HW, int C, int groups, float eps, float q_mul, void* q, float* partial, void* stream);
int dfh_attention_fp8out(const void* Q, int ldq, const void* K, int ldk, const void* Vt, int ldvt, void* O8, int ldo, const float* v_amax,
                         int batch, int heads, int head_dim, int Nq, int Nk, float scale, void* stream);
int dfh_amax_slabs(const void* x, long bstride, int ld, int cols, const int* row0, const int* nrows, float* out, int nslab, int batch,
                   void* stream);
/* Self-attention with both products on the e4m3 MFMA (csrc/attention_fp8.hip): bf16 Q / K / V^T in HBM, quantised on the way into the
 * matrix pipe with STATIC per-channel factors (q * rq, k * rk with rq * rk = 1 / hs[h] per head, v * rv; [heads * head_dim] each, hs
 * [heads]); bf16 output.  head_dim 40 / 80 / 160, Nk a multiple of 64.  dfh_attn_scales derives the factors from the LayerNorm-folded
 * projection weights wf [3C][C] (rows q | k | v, bf16) and biases bf [3C]: bound = |row|_2 sqrt(C) + |bias| for a LayerNorm-ed input. */
int dfh_attention_fp8(const void* Q, int ldq, const void* K, int ldk, const void* Vt, int ldvt, void* O, int ldo, const float* rq,
                      const float* rk, const float* rv, const float* hs, int batch, int heads, int head_dim, int Nq, int Nk, float scale,
                      void* stream);
int dfh_attn_scales(const void* wf, const float* bf, int C, int heads, float* rq, float* rk, float* rv, float* hs, void* stream);
/* softmax(Q K^T * scale) V; Q [B][Nq][ldq], K [B][Nk][ldk], Vt [B][H*D][ldvt] (V transposed), O [B][Nq][ldo]; bf16 */
int dfh_attention(const void* Q, int ldq, const void* K, int ldk, const void* Vt, int ldvt, void* O, int ldo,
                  int batch, int heads, int head_dim, int Nq, int Nk, float scale, void* stream);
/* Timesteps(flip_sin_to_cos=True, freq_shift=0): t [B] fp32 -> [B][dim] bf16 */
int dfh_timestep_embedding(const float* t, void* out, int batch, int dim, void* stream);
int dfh_nchw_to_nhwc_bf16(const void* x, int x_bf16, void* out, int batch, int C, int HW, void* stream);
int dfh_cast_f32_to_bf16(const float* x, void* y, size_t n, void* stream);

/* weight packing (fp32 master -> bf16 kernel layout) */
int dfh_pack_conv3x3(const float* w_oihw, void* out, int Cout, int Cin, int ldw, int col_off, void* stream);
int dfh_pack_matrix(const float* w, void* out, int N, int K, int ldw, int row_off, int col_off, int geglu, void* stream);
int dfh_pack_vector(const float* v, float* out, int N, int off, int geglu, int accumulate, void* stream);

/* ------------------------------------------------------------------ backward / training-step ops (train.py:691-716)
 * dfh_groupnorm with the (mean, rstd) pairs [B][G][2] kept for the backward pass */
int dfh_groupnorm_stats(const void* src0, int c0, const void* src1, int c1, int batch, int hw, int groups,
                        const float* gamma, const float* beta, float eps, int silu, void* out, float* partial,
                        float* stats_out, void* stream);
/* GroupNorm(+SiLU) backward: dx0/dx1 bf16 (acc != 0: add into the buffer), dgamma/dbeta fp32 += (atomics) */
int dfh_groupnorm_bwd(const void* src0, int c0, const void* src1, int c1, const void* dy, int batch, int hw, int groups,
                      const float* gamma, const float* beta, const float* stats, int silu, void* dx0, int acc0,
                      void* dx1, int acc1, float* dgamma, float* dbeta, float* partial, void* stream);
/* attention for training: forward that also returns the per-row log2-domain log-sum-exp [B][H][Nq], and the
 * flash-style backward (V ROW-major [B][Nk][ldv] here; delta = rowsum(dO * O) from dfh_attention_delta) */
int dfh_attention_lse(const void* Q, int ldq, const void* K, int ldk, const void* Vt, int ldvt, void* O, int ldo,
                      int batch, int heads, int head_dim, int Nq, int Nk, float scale, float* lse, void* stream);
int dfh_attention_delta(const void* O, const void* dO, int ld, float* delta, int batch, int heads, int head_dim, int Nq, void* stream);
int dfh_attention_bwd(const void* Q, int ldq, const void* K, int ldk, const void* V, int ldv, const void* dO, int ldo,
                      const float* lse, const float* delta, void* dQ, int lddq, void* dK, int lddk, void* dV, int lddv,
                      int batch, int heads, int head_dim, int Nq, int Nk, float scale, void* stream);
int dfh_layernorm_bwd(const void* x, const void* dy, const float* gamma, void* dx, int accumulate, float* dgamma,
                      float* dbeta, int M, int C, float eps, void* stream);
/* transposed / flipped weight packing so that data gradients reuse dfh_gemm:
 *   linear: Wt[t_row_off + k][t_col_off + n] = w[n][k];  conv3x3: W'[c][t_col_off + (8-t)*o_pad + o] = w[o][c][t] */
int dfh_pack_matrix_t(const float* w, void* out, int N, int K, int ldt, int t_row_off, int t_col_off, int geglu, void* stream);
int dfh_pack_conv3x3_t(const float* w, void* out, int Cout, int Cin, int ldt, int t_col_off, int o_pad, void* stream);
/* packed fp32 gradient -> master layout (+=): inverses of dfh_pack_matrix / dfh_pack_conv3x3 / dfh_pack_vector */
int dfh_unpack_matrix(const float* g, float* grad, int N, int K, int ldw, int row_off, int col_off, int geglu, void* stream);
int dfh_unpack_conv3x3(const float* g, float* grad, int Cout, int Cin, int ldw, int col_off, int cin_pad, void* stream);
int dfh_unpack_vector(const float* g, float* grad, int N, int off, int geglu, void* stream);
int dfh_pool2x2_sum(const void* in, void* out, int batch, int H, int W, int C, void* stream);   /* nearest-2x backward */
int dfh_add_bf16(void* dst, const void* src, size_t n, int accumulate, void* stream);
int dfh_geglu_fwd(const void* pre, void* y, size_t M, int N2, void* stream);
int dfh_geglu_bwd(const void* pre, const void* dy, void* dpre, size_t M, int N2, void* stream);
int dfh_act_fwd(const void* pre, void* y, size_t n, int kind, void* stream);      /* 1 silu 2 leaky_relu 3 tanh */
int dfh_act_bwd(const void* ref_bf16, const float* ref_f32, const void* dy_bf16, const float* dy_f32, void* dpre, size_t n,
                int kind, float scale, void* stream);
int dfh_nhwc_to_nchw_f32(const void* src, float* dst, int batch, int HW, int Cp, int C, float scale, int accumulate, void* stream);
int dfh_transpose_bf16(const void* in, void* out, int batch, int R, int C, int ld_in, int ld_out, size_t in_bstride,
                       size_t out_bstride, void* stream);
int dfh_mse_bwd(const float* pred, const float* target, const float* w, float* dpred, int rows, int L, float loss_scale,
                const float* scale_dev /* optional device scalar multiplied in (upstream d loss) */, void* stream);
int dfh_assemble_bwd(const float* dx, const uint8_t* mutual_real, float* dmutual, int rows, int CL, float eta, void* stream);
/* optimizer: torch.optim.AdamW step with the clip_grad_norm_ coefficient derived on device from *sumsq (may be NULL),
 * squared-norm accumulation, diffusers EMAModel update */
int dfh_sumsq(const float* g, size_t n, float* out, void* stream);
int dfh_adamw(float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2, float eps,
              float weight_decay, int step, const float* sumsq, float max_norm, void* stream);
/* dfh_adamw with the EMA update of the same elements folded in (one pass over the parameters instead of two) */
int dfh_adamw_ema(float* p, const float* g, float* m, float* v, float* shadow, size_t n, float lr, float beta1, float beta2, float eps,
                  float weight_decay, int step, const float* sumsq, float max_norm, float ema_decay, void* stream);
int dfh_ema(float* shadow, const float* p, size_t n, float decay, void* stream);
/* AdamW with block-wise 8-bit optimizer states (the reference's bnb.optim.AdamW8bit under --use_8bit_adam, train.py:573-593).  A block is
 * 64 consecutive elements; each block has one fp32 absmax per moment, each element one uint8 code per moment, x = table[code] * absmax.
 * The tables are the dynamic (tree) 8-bit type of Dettmers et al., 256 ascending fp32 entries: signed (exp_avg; no -1, code of 0 = 127)
 * and unsigned (exp_avg_sq; code of 0 = 0).  Quantising takes absmax = max |x| exactly and the nearest entry, with three fixed rules: an
 * all-zero block stores absmax 0 and zero codes; a second moment v > 0 never takes code 0 (it takes code 1); a block that holds a NaN or
 * an Inf stores a non-finite absmax.  Every device entry point needs n % 64 == 0 and 16-byte aligned fp32 buffers; the fp16-storage
 * library refuses them like dfh_adamw.  dfh_q8_table is host only (no GPU needed) and answers in both libraries.
 * dfh_adamw8 = dfh_adamw / dfh_adamw_ema (shadow may be NULL) on such states: the parameter moves by the unquantised new moments. */
int dfh_q8_table(int is_signed, float* out256_host);
int dfh_q8_quantize(const float* x, unsigned char* codes, float* absmax, size_t n, int is_signed, void* stream);
int dfh_q8_dequantize(const unsigned char* codes, const float* absmax, float* x, size_t n, int is_signed, void* stream);
int dfh_adamw8(float* p, const float* g, unsigned char* m8, float* m_absmax, unsigned char* v8, float* v_absmax,
               float* shadow /* may be NULL */, size_t n, float lr, float beta1, float beta2, float eps, float weight_decay,
               int step, const float* sumsq /* may be NULL */, float max_norm, float ema_decay, void* stream);
/* bf16 wire format of the data-parallel gradient exchange (replaces DDP's fp32 all-reduce behind accelerator.backward, train.py:611,699;
 * difashion_amd/dist.py exchange_bf16): fp32 range -> bf16 wire of n_pad elements (zero padding, n_pad % 8 == 0) | this rank's shard =
 * the `world` received contributions ([world][per] bf16) summed in fp32 in rank order, / world, rounded once | bf16 wire -> fp32 range */
int dfh_wire_pack(const float* g, void* wire, size_t n, size_t n_pad, void* stream);
int dfh_wire_shard_mean(const void* recv, void* shard, int world, size_t per, void* stream);
int dfh_wire_unpack(const void* wire, float* g, size_t n, void* stream);

/* ------------------------------------------------------------------ DiFashion glue (reference-owned arithmetic)
 * Sibling reduce feeding MutualEncoder: df.py:160-170 (training mean) / df.py:475-489 (sampling sum).
 *   out[j] = sum_k wtab[j][k] * (table[j][k] >= 0 ? gen[table] : given[-(table+1)])   (slot order)
 *   gen/given: fp32 rows of L = 4*H*W; out bf16 [rows][L] (MLP operand), out_f32 optional. */
int dfh_mutual_reduce(const float* gen, const float* given, const int32_t* table, const float* wtab,
                      void* out_bf16, float* out_f32, int rows, int olen, int L, void* stream);
/* Input assembly df.py:215-216 / :514-515 incl. CFG replica stacking: x [R*F][8][H][W] fp32 NCHW */
int dfh_assemble_input(const float* latents, const float* mutual, const float* hist, const float* null_latent,
                       const uint8_t* mutual_real, const uint8_t* hist_real, float* x, int R, int F, int CL,
                       float one_minus_eta, float eta, int per_row_flags, void* stream);
/* Guidance combine df.py:525-566 fused with scheduler.step df.py:569 (DDIMScheduler.step / PNDM transfer) */
typedef struct dfh_step_coef {
  int kind;            /* -1 combine only, 0 DDIM, 1 linear (x' = a*x - b*eps) */
  int vpred;
  float sqrt_a_t, sqrt_b_t, sqrt_a_prev, dir_coef, std_dev;
} dfh_step_coef;
int dfh_cfg_step(const float* eps_all, float* latents, float* eps_out, const float* noise, size_t n, int mode,
                 float cate_scale, float hist_scale, float mutual_scale, const dfh_step_coef* k, void* stream);
/* Guidance combine fused with one step of a multistep scheduler (PNDM's PLMS branch, DPM-Solver++ 2M), fp32, one launch.  Per element i < n:
 *   m = combine(mode, out_all, i)                      -> m_out[i] if given
 *   x = x_src[i]                                       -> x_save[i] if given
 *   q = m | (x - c1*m) / c0 | c0*x - c1*m   (conv 0|1|2) -> q_out[i] if given (the newest history slot)
 *   kind 0 PLMS: b = w[0]*q; b = b + w[j]*h_j (j = 1..terms-1); x' = cx*x - ce*b
 *   kind 1 DPM1: x' = cx*x - cd0*q        kind 2 DPM2: x' = (cx*x - cd0*q) - cd1*(cr*(q - h1))
 *   latents[i] = x'
 * h1..h3 are the earlier converted outputs, newest first; the caller rotates the pointers.  latents == x_src is the in-place call;
 * latents must not share memory with h1..h3 or q_out.  Every product and sum is rounded on its own (no fused multiply-add). */
typedef struct dfh_multistep_coef {
  int conv;            /* 0 none, 1 x0 from an epsilon prediction, 2 x0 from a v prediction */
  int kind;            /* 0 PLMS, 1 DPM1, 2 DPM2 */
  int terms;           /* PLMS: 1..4 */
  float c0, c1;
  float w[4];
  float cx, ce;
  float cd0, cr, cd1;
} dfh_multistep_coef;
int dfh_cfg_multistep(const float* out_all, const float* x_src, float* latents, float* m_out /* may be NULL */,
                      float* q_out /* may be NULL */, float* x_save /* may be NULL */, const float* h1, const float* h2,
                      const float* h3, size_t n, int mode, float cate_scale, float hist_scale, float mutual_scale,
                      const dfh_multistep_coef* k, void* stream);
/* DDIMScheduler.add_noise / get_velocity df.py:158,:244 */
int dfh_noise_mix(const float* x0, const float* noise, const int64_t* t, const float* sqrt_acp, const float* sqrt_1m_acp,
                  float* noisy, float* velocity, int rows, int L, void* stream);
/* per-row MSE of df.py:256-264 (fp32) */
int dfh_mse_rows(const float* pred, const float* target, float* out, int rows, int L, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DIFASHION_HIP_H */

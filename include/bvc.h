/* libbvc_hip.so -- C ABI of the MI355X-native (gfx950) self-supervised video pre-training step.
 *
 * The reference (ssheybani/baby-vision-curriculum) is pure Python and has no FFI of its own: its
 * entry points call a model object.  This header is the boundary a maintainer binds (ctypes stub in
 * INTEGRATION.md) so that object's arithmetic runs as hand-written HIP.  Each entry point cites the
 * reference interface it replaces; paths are relative to the reference checkout, "HF" is
 * transformers/models/videomae/modeling_videomae.py (5.15.0), which the reference instantiates at
 * pretraining/generative/pretrain_videomae.py:61-64.
 *
 * Conventions
 *  - every function returns 0 (BVC_OK) or a negative bvc_status; bvc_last_error() returns a
 *    thread-local message.  No C++ exception crosses this boundary, HIP errors are translated.
 *  - all pointers named *_dev are device pointers borrowed from the caller (torch tensors); the
 *    library never owns parameters, gradients, inputs or outputs.  Workspaces (saved activations,
 *    bf16 weight copies) belong to the context.
 *  - kernels are enqueued on the caller's HIP stream (`stream`, a hipStream_t passed as void*); the
 *    calls do not synchronise.  One host thread drives a context at a time (one process per GPU,
 *    as the reference's mp.spawn launcher does, pretrain_videomae.py:509-513).
 */
#ifndef BVC_H
#define BVC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BVC_OK 0
#define BVC_ERR_INVALID (-1) /* bad argument / unsupported shape */
#define BVC_ERR_HIP (-2)     /* a HIP runtime call failed */
#define BVC_ERR_STATE (-3)   /* call order violated (e.g. backward without a matching forward) */

const char* bvc_last_error(void);
/* Library build info: "gfx950;<git-less build tag>" */
const char* bvc_version(void);
/* Process-wide kernel-selection switches (the reference has no counterpart: ATen picks its cuBLAS kernels by itself).  They
 * exist for the parity tests and the same-process A/B tools, never change results beyond the documented tolerances, and
 * replace the environment variables earlier builds read:
 *   "gemm8"       0 (default) = the measured selection; 1 = the 256-row persistent GEMM for every product it can take,
 *                 whatever its size (runs the kernel set of the 256-clip benchmark at oracle-sized batches); -1 = never
 *   "dw_overlap"  1 = a layer's grouped weight-gradient launch runs on the context's side stream (default 0)
 *   "row_ln"      the LayerNorms of 384-wide stacks (VideoMAE decoder, JEPA predictor) inside the epilogues of the products next to
 *                 them (BVC_EPI_RESID_LN / BVC_EPI_DLN): 0 (default) = the measured selection, 1 = whenever the shapes allow,
 *                 -1 = never (separate LayerNorm passes)
 *   "deterministic" 0 (default) / 1: while 1, every forward and backward entry point (bvc_videomae_*, bvc_vit_*, bvc_predictor_*,
 *                 bvc_op_*) gives the same bits on every run for the same inputs, parameters, batch, device and build.  The f32 atomics
 *                 whose arrival order the scheduler decides - split-K / accumulating GEMM outputs (tile config 13 included), fused bias
 *                 gradients (rowsum), LayerNorm parameter partials, column sums - are replaced by plain stores of the partials into a
 *                 workspace and a separate pass that adds them in a fixed order.  Results differ from mode 0 in the last bits only.
 *                 Workspace: library-owned, grow-only, one buffer per (device, stream) - so that work on two streams never shares
 *                 one - allocated by the first deterministic launch on that stream that needs more (a growth synchronises that
 *                 stream once) and reused afterwards; model contexts and bvc_op_* callers share it.  It lives until
 *                 bvc_deterministic_workspace_release() or the end of the process: a process that creates and destroys streams should
 *                 release it after destroying them (each stream ever used keeps its buffer, and a new stream that reuses a destroyed
 *                 stream's handle would take over that buffer).  Tile configs that have no deterministic form (the experiment
 *                 kernels 3-5, 8, 14 of a -DBVC_EXPERIMENTS build) return BVC_ERR_INVALID for split / accumulating / bias-gradient
 *                 outputs; tile configs 6 / 7 / 9 run them on the 128 x 128 / 128 x 64 deterministic kernel.
 *                 Read at every launch, so it may change between calls (not while a call is being enqueued elsewhere).
 *   "head_pad"    0 (default) / 1: 1 = heads of 80 / 88 dims run zero-padded to 96 (padded weight copies, pad / unpad launches), the
 *                 layout of earlier builds; 0 = in place.  Read when a model context allocates its stacks (same-process A/Bs only).
 *   "dec_tail"    1 (default) / 0: tail mode of the VideoMAE pre-training step.  The head, the loss and the final LayerNorm read only the
 *                 decoded rows of the decoder's [visible | decoded] rows per clip, so the LAST decoder layer runs everything behind its
 *                 qkv product (attention queries, proj, LayerNorm 2, the MLP, their input- and weight-gradient products) on those
 *                 rows alone.  Taken when the decoded rows per clip are a multiple of 128, the layer's LayerNorms run in the 384-wide
 *                 epilogues ("row_ln"), the heads are 64 wide, a clip has more than 160 rows (below, the whole-head attention backward
 *                 serves) and no gate is set; otherwise, and with 0, the layer runs on all rows with the launches and the results of
 *                 earlier builds.  Read by every forward (its backward follows the forward).
 *   "dec_first"   -1 (default) / 0 / 1: first mode of the VideoMAE pre-training step.  The decoded rows enter the FIRST decoder layer as
 *                 mask_token + the sinusoid of their position, so that layer's LayerNorm 1 and qkv row of such a row depend on the position
 *                 alone: they are computed once per position and copied into the qkv the attention kernels read, and in the backward
 *                 the rows' share of the qkv weight and bias gradients, of LayerNorm 1's and of the mask token's gradient follows from
 *                 the per-position sums of d qkv (f32, clips in ascending order: the same bits on every run).  The visible rows take the
 *                 per-row path.  1 = whenever the decoder has more than one layer, unpadded heads and no gate; -1 = that, from the
 *                 batch at which it was measured to pay; 0 = never (the launches and results of earlier builds).  Read by every forward.
 * bvc_get_option returns the value, or BVC_ERR_INVALID for an unknown name; bvc_set_option rejects values outside the list. */
int bvc_set_option(const char* name, int value);
int bvc_get_option(const char* name);
/* bytes the deterministic mode's workspace holds on the current HIP device (all streams; 0 before its first use) */
int64_t bvc_deterministic_workspace_bytes(void);
/* synchronises the current HIP device, then frees its deterministic workspaces (all streams); the next deterministic launch
 * allocates again */
int bvc_deterministic_workspace_release(void);

/* ------------------------------------------------------------------------------------------------
 * VideoMAE pre-training step.
 * Replaces transformers.VideoMAEConfig as built by get_config(), pretrain_videomae.py:43-58.        */
typedef struct bvc_videomae_config {
    int image_size, patch_size, num_channels, num_frames, tubelet_size;
    int hidden_size, num_hidden_layers, num_attention_heads, intermediate_size;
    int decoder_hidden_size, decoder_num_hidden_layers, decoder_num_attention_heads, decoder_intermediate_size;
    float layer_norm_eps;   /* 1e-12: every VideoMAELayer LayerNorm (HF:336-337) */
    float decoder_norm_eps; /* 1e-5 : decoder.norm (HF:484) */
    int norm_pix_loss;      /* 1 in the reference (pretrain_videomae.py:57) */
} bvc_videomae_config;

typedef struct bvc_ctx bvc_ctx;

/* Flat parameter layout.  Parameters and gradients live in ONE contiguous fp32 buffer each (forward
 * order: patch embed | encoder layers | encoder_to_decoder, mask_token | decoder layers | decoder.norm
 * | decoder.head), so casts, the optimiser and the data-parallel all-reduce are single large
 * transfers.  Entry `index` names a state-dict key of VideoMAEForPreTraining (the 264 keys that
 * model.module.state_dict() returns at pretrain_videomae.py:76) and where it sits in the buffer. */
int bvc_videomae_param_count(const bvc_videomae_config* cfg);
int64_t bvc_videomae_param_numel(const bvc_videomae_config* cfg);
int bvc_videomae_param_info(const bvc_videomae_config* cfg, int index, char* name, int name_cap, int64_t* offset,
                            int64_t* numel, int* ndim, int64_t shape[5]);

/* Allocates workspaces for up to `max_batch` clips with `num_masked` masked tokens per clip. */
int bvc_videomae_create(const bvc_videomae_config* cfg, int max_batch, int num_masked, bvc_ctx** out);
void bvc_videomae_destroy(bvc_ctx* ctx);
/* The same for a step that reconstructs only `num_decoded` of the `num_masked` masked tokens of every clip (1 <= num_decoded <=
 * num_masked; decoder masking as in VideoMAE V2, Wang et al., CVPR 2023, section 3.2): the decoder runs on (seq_len - num_masked) +
 * num_decoded rows per clip and the loss is taken on the decoded tokens.  bvc_videomae_create is the num_decoded == num_masked case.
 * bvc_videomae_backward, _tap, _shadow and _destroy take such a context as they take any other; the taps "x_full" / "dec<i>" then have
 * batch * (seq_len - num_masked + num_decoded) rows and "labels" batch * num_decoded. */
int bvc_videomae_create_dual(const bvc_videomae_config* cfg, int max_batch, int num_masked, int num_decoded, bvc_ctx** out);

/* Replaces `outputs = xmodel(inputs, bool_masked_pos=m); outputs.loss` (pretrain_videomae.py:301-302,
 * i.e. VideoMAEForPreTraining.forward, HF:531-671).
 *   pixels_dev  f32 [batch][num_frames][channels][H][W]   (loader output, homeview.py:218-231)
 *   mask_dev    u8  [batch][seq_len], 1 = masked; every row must hold exactly num_masked ones
 *   params_dev  f32 flat parameter buffer (layout above)
 *   loss_dev    f32 scalar  (mean squared error over masked, per-patch-normalised pixels)
 *   logits_dev  optional f32 [batch][num_masked][patch_dim] (outputs.logits), may be NULL
 * A row with a different number of ones makes the loss NaN (flag checked on the device, no host sync). */
int bvc_videomae_forward(bvc_ctx* ctx, const float* pixels_dev, const uint8_t* mask_dev, int batch,
                         const float* params_dev, float* loss_dev, float* logits_dev, void* stream);

/* Called on the host, from inside bvc_videomae_backward, after every kernel that finalises the
 * gradient range [offset, offset+count) of the flat gradient buffer has been enqueued on `stream`.
 * The data-parallel wrapper records an event there and starts the RCCL all-reduce of that range on
 * its communication stream (what DistributedDataParallel's bucket hooks do at
 * pretrain_videomae.py:180-181,312).  Ranges arrive tail-first (decoder head ... patch embed). */
typedef void (*bvc_bucket_fn)(int64_t offset, int64_t count, void* user);

/* Pixel source of the *_px entry points.  BVC_PIXELS_F32: f32 clips already normalised by the loader (what the reference's
 * dataloader hands over, homeview.py:218-231).  BVC_PIXELS_U8: the loader's uint8 frames, normalised while they are read as
 * (u / 255 - mean[c]) / std[c] - ToTensor + Normalize with the same operation order, hence bit-identical values - so that
 * a quarter of the bytes cross PCIe and HBM (the input side of the step).  NULL format = BVC_PIXELS_F32. */
enum { BVC_PIXELS_F32 = 0, BVC_PIXELS_U8 = 1 };
typedef struct bvc_pixel_format {
    int dtype;
    float mean[4], std[4]; /* per channel; used for BVC_PIXELS_U8 only */
} bvc_pixel_format;
int bvc_videomae_forward_px(bvc_ctx* ctx, const void* pixels_dev, const bvc_pixel_format* fmt, const uint8_t* mask_dev, int batch,
                            const float* params_dev, float* loss_dev, float* logits_dev, void* stream);
/* bvc_videomae_forward_px with a decode mask:
 *   decode_mask_dev u8 [batch][seq_len], 1 = the token gets a mask-token row in the decoder and is a loss target; every row must hold
 *                   exactly num_decoded ones, all of them on masked tokens.  NULL (contexts with num_decoded == num_masked only) =
 *                   every masked token: exactly bvc_videomae_forward_px, the same launches and bits.
 *   logits_dev      optional f32 [batch][num_decoded][patch_dim], rows in ascending token order
 *   loss_dev        the mean over batch * num_decoded * patch_dim elements
 * A row with another count, or with a decoded token that is visible to the encoder (its target would leak into the loss), makes the
 * loss NaN (flag checked on the device, no host sync). */
int bvc_videomae_forward_dual(bvc_ctx* ctx, const void* pixels_dev, const bvc_pixel_format* fmt, const uint8_t* mask_dev,
                              const uint8_t* decode_mask_dev, int batch, const float* params_dev, float* loss_dev, float* logits_dev,
                              void* stream);

/* Replaces autograd's backward of the step (scaler.scale(loss).backward(), pretrain_videomae.py:312).
 *   grad_loss_dev f32 scalar on the device: d(objective)/d(loss) (GradScaler's scale)
 *   grads_dev     f32 flat gradient buffer, OVERWRITTEN with d(objective)/d(param) */
int bvc_videomae_backward(bvc_ctx* ctx, const float* grad_loss_dev, float* grads_dev, bvc_bucket_fn on_bucket,
                          void* user, void* stream);
/* The context's bf16 copy of the flat parameters (what every product reads) and the hand-shake that lets the caller keep it
 * current instead of the forward: *shadow_bf16 / *numel (either may be NULL) describe it - element i mirrors element i of the flat
 * parameter buffer; valid = 1 vouches that it matches the parameters the NEXT forward will be given (that forward then skips its
 * cast pass over all parameters; the vouch is consumed by it), valid = 0 withdraws the vouch, valid < 0 only queries.
 * bvc_op_sgd_step / bvc_op_adam_step write the copy together with the parameters (their bf16_shadow argument).  Replaces nothing
 * in the reference: autocast re-casts every weight on every forward (pretrain_videomae.py:306-308). */
int bvc_videomae_shadow(bvc_ctx* ctx, int valid, void** shadow_bf16, int64_t* numel);

/* Copies a saved activation of the last forward as f32 into dst_dev (parity probes: "embed",
 * "enc<i>", "x_full", "dec<i>", "labels").  Returns the element count via *numel.
 * "dec<last>" always has nvis + ndec rows per clip.  After a forward in tail mode ("dec_tail") the visible rows of that output were
 * never computed: the call completes them on the spot with the ordinary kernels (a few launches on B * nvis rows, in spare memory of
 * the context, with the parameters the forward was given) - ask before an optimiser step rewrites those. */
int bvc_videomae_tap(bvc_ctx* ctx, const char* name, float* dst_dev, int64_t capacity, int64_t* numel, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Encoder-only inference: the embedding extraction that runs between curriculum stages.
 * Replaces transformers.VideoMAEForVideoClassification(num_labels=0).forward as called at
 * benchmarks/compute_embeddings_videomae.py:78-96 (model assembly) and :253-264 (xmodel(pixel_values=inputs).logits):
 * every token (no mask) -> patch embedding + sinusoid -> encoder layers -> mean over tokens -> fc_norm LayerNorm.
 * `params` is a flat f32 buffer holding the "videomae.*" entries in the order of bvc_videomae_param_info (they are the
 * leading bvc_videomae_encoder_param_numel() elements of the pre-training layout, so a pre-training buffer can be passed
 * as is).  Forward only; the context owns workspaces for max_batch clips. */
typedef struct bvc_encoder_ctx bvc_encoder_ctx;
int64_t bvc_videomae_encoder_param_numel(const bvc_videomae_config* cfg);
int bvc_videomae_encoder_create(const bvc_videomae_config* cfg, int max_batch, bvc_encoder_ctx** out);
void bvc_videomae_encoder_destroy(bvc_encoder_ctx* ctx);
/*   pixels_dev   f32 [batch][T][C][H][W]
 *   fc_norm_w/b  f32 [hidden] or both NULL (then `pooled` is the plain token mean)
 *   tokens_dev   f32 [batch][L][hidden] last_hidden_state, or NULL
 *   pooled_dev   f32 [batch][hidden] = fc_norm(mean over tokens), or NULL                                     */
int bvc_videomae_encode(bvc_encoder_ctx* ctx, const float* pixels_dev, int batch, const float* params_dev,
                        const float* fc_norm_w, const float* fc_norm_b, float fc_norm_eps, float* tokens_dev,
                        float* pooled_dev, void* stream);
int bvc_videomae_encode_px(bvc_encoder_ctx* ctx, const void* pixels_dev, const bvc_pixel_format* fmt, int batch,
                           const float* params_dev, const float* fc_norm_w, const float* fc_norm_b, float fc_norm_eps,
                           float* tokens_dev, float* pooled_dev, void* stream);
/* Linear probe (encoder frozen, fc_norm trainable): dfc_norm_w / dfc_norm_b (f32 [hidden], written) of the last encode's fc_norm
 * from dpooled_dev (f32 [batch][hidden]), with the pre-norm pooled rows and statistics that encode kept.  Fixed summation order. */
int bvc_videomae_encoder_fc_norm_backward(bvc_encoder_ctx* ctx, const float* dpooled_dev, const float* fc_norm_w, float* dfc_norm_w,
                                          float* dfc_norm_b, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Fine-tuning: VideoMAEForVideoClassification.forward(pixel_values, labels) with autograd through the encoder.  Same parameters
 * and the same forward as bvc_videomae_encode_px (its pooled rows are bitwise equal), but every layer keeps its activations at
 * all batch x L tokens for the backward (about 36 x hidden bytes per token and layer).  The context owns workspaces for max_batch
 * clips; create refuses, before allocating, a batch whose widest bf16 operand reaches 4 GiB and names the largest that fits. */
typedef struct bvc_cls_ctx bvc_cls_ctx;
int bvc_videomae_cls_create(const bvc_videomae_config* cfg, int max_batch, bvc_cls_ctx** out);
void bvc_videomae_cls_destroy(bvc_cls_ctx* ctx);
/*   pooled_dev   f32 [batch][hidden] = fc_norm(mean over tokens); fc_norm_w/b are required
 *   tokens_dev   f32 [batch][L][hidden] last_hidden_state, or NULL                                               */
int bvc_videomae_cls_forward_px(bvc_cls_ctx* ctx, const void* pixels_dev, const bvc_pixel_format* fmt, int batch,
                                const float* params_dev, const float* fc_norm_w, const float* fc_norm_b, float fc_norm_eps,
                                float* pooled_dev, float* tokens_dev, void* stream);
/* dpooled_dev f32 [batch][hidden] -> grads_dev (the encoder's flat f32 gradients, overwritten), dfc_norm_w / dfc_norm_b (f32 [hidden],
 * overwritten).  Gradient ranges of grads_dev are reported tail-first through on_bucket (may be NULL), as bvc_videomae_backward does. */
int bvc_videomae_cls_backward(bvc_cls_ctx* ctx, const float* dpooled_dev, float* grads_dev, float* dfc_norm_w, float* dfc_norm_b,
                              bvc_bucket_fn on_bucket, void* user, void* stream);
/* as bvc_videomae_shadow (the copy covers the encoder's parameters) */
int bvc_videomae_cls_shadow(bvc_cls_ctx* ctx, int valid, void** shadow_bf16, int64_t* numel);

/* Per-layer outputs of the two classification contexts: output_hidden_states / output_attentions of
 * VideoMAEForVideoClassification.forward (HF VideoMAEEncoder.forward collects them layer by layer).  L = num_hidden_layers,
 * N = seq_len, D = hidden_size, H = num_attention_heads; either pointer may be NULL (NULL struct = neither):
 *   hidden_states f32 [L + 1][batch][N][D]   slot 0 = the embedding output (patch embedding + position table), slot i + 1 = the
 *                                            output of layer i - of the forward that ran, gates of a set_drop included
 *   attentions    f32 [L][batch][H][N][N]    softmax(q k^T / sqrt(D / H)) of layer i, row = query, column = key (bvc_op_attention_probs
 *                                            on the layer's qkv and lse, at the stack's attention width with the true head's scale)
 * bvc_videomae_encode_ex is bvc_videomae_encode_px with these outputs: given hidden_states, the embedding product writes slot 0 and
 * layer i reads slot i and writes slot i + 1 - the same launches as without it, on other pointers, and no copy for the hidden states
 * themselves.  last_hidden_state then IS slot L: a caller that wants both should read it there and pass tokens_dev = NULL (the Python
 * shim does); a non-NULL tokens_dev is still served, by one device-to-device copy of slot L.  Given attentions, one attn_probs_kernel
 * launch follows each layer.  out == NULL or both members NULL: exactly
 * bvc_videomae_encode_px.  bvc_videomae_cls_introspect is valid between a bvc_videomae_cls_forward_px of the same context and
 * its backward (BVC_ERR_STATE otherwise): it copies each layer's kept residual stream and recomputes the probabilities from each
 * layer's kept qkv and lse; the forward and the backward themselves are unchanged. */
typedef struct bvc_introspect {
    float* hidden_states;
    float* attentions;
} bvc_introspect;
int bvc_videomae_encode_ex(bvc_encoder_ctx* ctx, const void* pixels_dev, const bvc_pixel_format* fmt, int batch,
                           const float* params_dev, const float* fc_norm_w, const float* fc_norm_b, float fc_norm_eps,
                           float* tokens_dev, float* pooled_dev, const bvc_introspect* out, void* stream);
int bvc_videomae_cls_introspect(bvc_cls_ctx* ctx, const bvc_introspect* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Stochastic depth and hidden dropout: a gate on the two residual branches of every pre-LN layer of a context,
 *     h     = x_in + g1 .* (proj(ctx) + b_o)        g(row, col) = path_scale[layer][branch][row / rows_per_sample]
 *     x_out = h    + g2 .* (fc2(act) + b_2)                       * keep(row, col) / (1 - hidden_p)
 * Replaces DropPath / drop_path (pretraining/predictive/vision_transformer.py:145-164, Block.forward :229-230) and
 * VideoMAESelfOutput.dropout / VideoMAEOutput.dropout (HF:270-274, 316-320).
 *   path_scale      device f32 [layers][2][samples] (branch 0 = attention, 1 = MLP): 0 for a dropped sample, 1 / (1 - rate) for a
 *                   kept one; NULL = no stochastic depth.  Copied into the context by the set_drop call (stream-ordered).
 *   rows_per_sample rows that share one path_scale entry: the tokens of one sequence of the call (a clip's seq_len; ntok for
 *                   bvc_vit_forward; Nc + Np for the predictor, whose samples are its nsets * B sequences)
 *   hidden_p        element dropout probability in [0, 1) on both branch outputs; the keep mask is NOT stored: it is a function of
 *                   (seed, offset, layer, branch, element index row * width + col) - Philox4x32-10, counter = {index / 4 low,
 *                   index / 4 high | (2 layer + branch) << 8, offset low, offset high}, key = seed; output (index % 4) below
 *                   hidden_p * 2^32 drops the element - that the backward evaluates again.  bvc_op_dropout_mask /
 *                   bvc_dropout_mask_host give the same mask as bytes (1 = kept).
 * bvc_*_set_drop sets the gate for the NEXT forward of the context and the backward that belongs to it; later forwards run ungated
 * until it is called again.  drop == NULL, or hidden_p == 0 with path_scale == NULL, switches it off.  With the gate off a context
 * launches exactly the kernels it launches without this interface.  While it is on, the two branch products of a layer run the
 * BVC_EPI_RESID_GATE epilogue of the 128 x 128 / 128 x 64 / 64 x 64 kernel and the LayerNorms run as separate passes; in the
 * backward the residual gradient passes ungated and the bf16 copies that feed a branch are gated where they are produced. */
typedef struct bvc_branch_drop {
    float hidden_p;
    uint64_t seed, offset;
    const float* path_scale;
    int rows_per_sample;
} bvc_branch_drop;
int bvc_videomae_cls_set_drop(bvc_cls_ctx* ctx, const bvc_branch_drop* drop, int samples, void* stream);
/* forward only (a train-mode module under torch.no_grad(), a train-mode linear probe) */
int bvc_videomae_encoder_set_drop(bvc_encoder_ctx* ctx, const bvc_branch_drop* drop, int samples, void* stream);
/* ------------------------------------------------------------------------------------------------
 * Mixup / CutMix inside the patch gather.  One entry per clip of the call: clip b enters the patch-embedding product composed with
 * clip `partner`, at pixel (t, c, y, x) of either source dtype (values as normalised by the pixel format)
 *     inside the box, rows [y0, y1) x columns [x0, x1) of every frame:   the partner's pixel
 *     outside it:                                                         lam * own + (1 - lam) * partner in f32 (own when lam == 1)
 * and is then rounded to bf16 as the plain gather rounds.  Mixup = empty box, lam < 1; CutMix = a box, lam = 1; partner = b with
 * lam = 1 and an empty box leaves the clip as it is.  The mixed clip is never written: a run of pixels the box covers is read from
 * the partner alone, a run outside it with lam == 1 from the clip alone, so CutMix moves the bytes of the plain gather and Mixup reads
 * the source twice.  The backward is unchanged (the patch-embedding weight gradient reads the gathered operand; pixels get none).
 * The *_set_mix calls arm the NEXT forward of the context (cls_forward_px; encode_px / encode_ex): that forward copies the table
 * (device memory, `samples` entries, alive until that forward has been enqueued) into the context on its stream, gathers through
 * it and disarms; `samples` must equal its batch (BVC_ERR_INVALID otherwise).  mix_dev == NULL disarms.  With nothing armed a
 * forward launches exactly what it launches without this interface.  An entry with a partner outside [0, samples), a box outside
 * the image or a lam outside [0, 1] is clamped before any address is formed and makes that forward's pooled rows (and tokens) NaN:
 * the flag is checked on the device, without a host sync. */
typedef struct bvc_clip_mix {
    int partner;
    float lam;
    int y0, y1, x0, x1;
} bvc_clip_mix; /* 24 bytes */
int bvc_videomae_cls_set_mix(bvc_cls_ctx* ctx, const bvc_clip_mix* mix_dev, int samples, void* stream);
/* forward only (a train-mode linear probe, a train-mode module under torch.no_grad()) */
int bvc_videomae_encoder_set_mix(bvc_encoder_ctx* ctx, const bvc_clip_mix* mix_dev, int samples, void* stream);
/* ------------------------------------------------------------------------------------------------
 * Random erasing inside the patch gather, before the mix.  Each clip has `boxes` (<= BVC_ERASE_MAX_BOXES) table entries; at pixel
 * (t, c, y, x) of clip s the LAST entry j with y0 <= y < y1 and x0 <= x < x1 replaces the source pixel (a normalised value) by
 *     mode 0 (const): 0
 *     mode 1 (rand):  one N(0, 1) value per clip, frame, box and channel
 *     mode 2 (pixel): one N(0, 1) value per element
 * The boxes are the same in every frame, the noise is fresh per frame; an empty box (y0 >= y1 or x0 >= x1) erases nothing.  Then
 * the clip's bvc_clip_mix entry (when a mix is armed as well) composes the ERASED clip with its ERASED partner: a clip's erased
 * content depends on (seed, offset, clip, position) only, the same as `own` and as somebody's `partner`.  The erased clip is never
 * written and a run of pixels a box covers is not loaded.
 * The values are Box-Muller normals of Philox4x32-10 draws: key = the halves of `seed`, counter words 2 and 3 = the halves of
 * `offset`.  Pixel noise: element e = (((s T + t) C + c) H + y) W + x, q = e >> 2, lane = e & 3, counter words 0 and 1 =
 * low 32 bits of q and (q >> 32) | 0xE0 << 16.  Colours: e = ((s T + t) 4 + j) 4 + c (C <= 4), the same split, tag 0xE1 << 16.
 * From one call's outputs r0 .. r3, lanes 0 / 1 are the cos / sin branch on (r0, r1) and lanes 2 / 3 on (r2, r3):
 * u1 = ((ra >> 8) + 1) 2^-24, u2 = (rb >> 8) 2^-24, z = sqrt(-2 ln u1) {cos, sin}(2 pi u2) in f32, so |z| <= 5.77.
 * The *_set_erase calls follow *_set_mix: they arm the NEXT forward of the context, which copies the table ([samples][boxes] entries
 * of device memory, alive until that forward has been enqueued), gathers through it and disarms; `samples` must equal its batch
 * (BVC_ERR_INVALID otherwise), boxes must lie in [1, BVC_ERASE_MAX_BOXES], tab_dev == NULL disarms.  Mix and erase are independent:
 * either, both or neither may be armed.  An entry with a box outside the image or a mode outside 0 .. 2 is clamped before any
 * address or counter is formed and makes that forward's pooled rows (and tokens) NaN, as a bad mix entry does. */
#define BVC_ERASE_MAX_BOXES 4
typedef struct bvc_erase_box {
    int y0, y1, x0, x1;
    int mode;
} bvc_erase_box; /* 20 bytes; mode 0 const, 1 rand, 2 pixel */
int bvc_videomae_cls_set_erase(bvc_cls_ctx* ctx, const bvc_erase_box* tab_dev, int samples, int boxes, uint64_t seed, uint64_t offset,
                               void* stream);
/* forward only */
int bvc_videomae_encoder_set_erase(bvc_encoder_ctx* ctx, const bvc_erase_box* tab_dev, int samples, int boxes, uint64_t seed,
                                   uint64_t offset, void* stream);
/* the f32 values the gather writes for erased elements: kind 0 the pixel noise of a whole batch [B][T][C][H][W] (W % 4 == 0), kind 1
 * the colours [B][T][4][4] (box, channel) */
int bvc_op_erase_noise(uint64_t seed, uint64_t offset, int kind, int B, int T, int C, int H, int W, float* out_dev, void* stream);
/* keep bytes (1 = kept, 0 = dropped) of the M x N element mask of one branch, row-major, on the device and on the host */
int bvc_op_dropout_mask(uint64_t seed, uint64_t offset, int layer, int branch, int M, int N, float p, uint8_t* out_dev, void* stream);
int bvc_dropout_mask_host(uint64_t seed, uint64_t offset, int layer, int branch, int M, int N, float p, uint8_t* out_host);

/* ------------------------------------------------------------------------------------------------
 * Clip transforms on uint8 frames: resize, crop, flip, colour jitter and grayscale, between the upload of the loader's frames and
 * the model.  Replaces, frame for frame, what the reference's loaders run on the host through torchvision / PIL:
 * Resize + CenterCrop (pretraining/generative/homeview.py:227-231) and RandomResizedCrop, RandomApply([ColorJitter]), RandomGrayscale,
 * RandomHorizontalFlip (pretraining/predictive/homeview.py:118-178, pretraining/contrastive/homeview.py:120-181).  The host draws one
 * bvc_frame_aug per OUTPUT frame; the library applies the table.
 *   src              index of the source frame ([F_src][3][Hs][Ws] uint8): several entries may name one frame (two views, repeats)
 *   x0, y0, w, h     region of the source frame
 *   Hr, Wr           size the region is resized to: antialiased bilinear (triangle filter of support max(1, w / Wr), pixel centres at
 *                    i + 0.5, taps clipped to the region and renormalised), a horizontal pass rounded half-up to uint8 and then a
 *                    vertical pass rounded half-up to uint8, with the weights in the fixed point of torch's uint8 path: bit for
 *                    bit what F.interpolate(uint8, mode="bilinear", antialias=True) gives on the region (PIL's Image.resize(BILINEAR)
 *                    does the same at a finer weight precision); a region of the resized size is copied bit for bit
 *   oy, ox           where the Ho x Wo output window sits in the resized image
 *                    (RandomResizedCrop: region = the crop box, (Hr, Wr) = (Ho, Wo), window at 0;  Resize + CenterCrop: region = the
 *                    whole frame, short side -> S, window centred)
 *   flip             non-zero mirrors the output columns
 *   nops, order      number of ColorJitter stages (0 .. 4) and their order: stage i is op (order >> 4 i) & 15, 0 = brightness,
 *                    1 = contrast, 2 = saturation, 3 = hue; each op at most once
 *   factor[op]       the op's factor: the blend ratio of brightness / contrast / saturation (>= 0), the hue shift in [-0.5, 0.5]
 *   gray             non-zero: a grayscale stage (three equal channels) after the jitter stages
 * Every colour stage is f32 arithmetic on the previous stage's uint8 values, rounded as torchvision's tensor functions round uint8
 * images: blend ratio * a + (1 - ratio) * b, clamped and truncated (b = 0, the frame's mean gray, the pixel's gray); gray =
 * trunc(0.2989 r + 0.587 g + 0.114 b); hue through float HSV and back with * (255 + 1 - 1e-3), truncated.  The contrast mean is the
 * mean of the truncated gray of the whole output frame as it stands when that stage runs, from an integer sum: the same bits on every
 * run and in either deterministic mode.
 * bvc_op_clip_transform: src_dev / table_dev / out_dev ([F_out][3][Ho][Wo] uint8, i.e. [B][T][C][H][W]) are device memory;
 * table_host is the same table in host memory (the host drew it), read during the call only: the entries are validated there, without
 * a device sync, and it tells the call whether any frame needs the second pass.  workspace_dev holds
 * bvc_op_clip_transform_workspace bytes, 4-byte aligned (per-frame filter precisions, per-tile gray sums).  Two launches for a table
 * without contrast stages (the precisions; resize + the colour stages), three otherwise; no atomics.  BVC_ERR_INVALID with a message for channels != 3, an empty region or
 * one outside the source, a window outside the resized image, a shrink factor above BVC_AUG_MAX_SCALE per axis, a resized edge above 16384, an unknown op or a
 * factor out of range.
 * bvc_clip_transform_host: the same arithmetic compiled for the host (csrc/augment.h), on host memory; needs no GPU. */
#define BVC_AUG_MAX_SCALE 16
typedef struct bvc_frame_aug {
    int32_t src;
    int32_t x0, y0, w, h;
    int32_t Hr, Wr;
    int32_t oy, ox;
    int32_t flip;
    int32_t nops, order;
    float factor[4];
    int32_t gray;
} bvc_frame_aug; /* 68 bytes */
int64_t bvc_op_clip_transform_workspace(int F_out, int Ho, int Wo);
int bvc_op_clip_transform(const uint8_t* src_dev, int F_src, int channels, int Hs, int Ws, const bvc_frame_aug* table_host,
                          const bvc_frame_aug* table_dev, int F_out, int Ho, int Wo, uint8_t* out_dev, void* workspace_dev, void* stream);
int bvc_clip_transform_host(const uint8_t* src, int F_src, int channels, int Hs, int Ws, const bvc_frame_aug* table, int F_out, int Ho,
                            int Wo, uint8_t* out);
/* The post stage: the two remaining transforms of the reference's _get_transform, on the uint8 frames [F][3][H][W] that the stage above
 * produced.  'b' GaussianBlur(p = 0.5), i.e. PIL's ImageFilter.GaussianBlur(radius ~ U(0.1, 2.0)), and 'o' RandomHorizontalFlip +
 * RandomRotation((-90, 90)), i.e. PIL's Image.rotate(angle, NEAREST, expand=False, fillcolor=0); the flip stays in bvc_frame_aug
 * (it commutes bit for bit with a symmetric integer blur and with pointwise colour).  One bvc_frame_post per frame; per frame the order
 * is blur, gray, rotation (the reference's b, g, o).  Everything is integer arithmetic (the gray is the stage above's), restated from
 * Pillow: the device, the host twin and PIL give the same bytes.
 *   blur_r           integer box radius, -1 = no blur.  Pillow approximates the Gaussian by three box passes along the rows and then
 *                    three along the columns, every pass rounded to uint8, taps beyond the frame reading the edge value of that
 *                    pass's input:  out[x] = (ww * sum_{|i| <= r} in[x + i] + fw * (in[x - r - 1] + in[x + r + 1]) + 2^23) >> 24
 *   blur_ww, blur_fw the 8.24 fixed-point weights of the box and of its two far taps; bvc_aug_blur_weights (host only) derives
 *                    (r, ww, fw) from the Gaussian radius as Pillow does, types included (f32, the square root and the floor in f64, an
 *                    f32 division for ww); it refuses a negative radius, a NaN and a radius above BVC_AUG_MAX_BLUR_RADIUS.  Radius 0 is
 *                    ww = 2^24, fw = 0: the identity
 *   gray             non-zero: the grayscale stage of the stage above (trunc(0.2989 r + 0.587 g + 0.114 b)), applied AFTER the blur
 *   rotate, rot[6]   non-zero: output pixel (x, y) copies in[yin][xin] with xin = (a2 + a1 y + a0 x) >> 16 and yin = (a5 + a4 y + a3 x)
 *                    >> 16 (arithmetic shifts) when that lies inside the frame, and is 0 otherwise; a0 .. a5 is the inverse affine map
 *                    in 16.16 fixed point as Pillow's affine_fixed builds it (bvc.augment.rotation_coeffs)
 * bvc_op_clip_post: in_dev / table_dev / out_dev / workspace_dev are device memory, table_host is the same table in host memory, read
 * during the call only: it is validated there, without a device sync, and tells the call what to launch.  At most two launches: the
 * blur kernel when some frame blurs or turns gray (frames that do neither are copied through by their workgroups), the rotation
 * kernel when some frame rotates (the others are copied); with both the frames pass through workspace_dev
 * (bvc_op_clip_post_workspace bytes, needed only then).  A table that is the identity everywhere is served by one device-to-device
 * copy.  No atomics: nothing for the deterministic mode to switch.  BVC_ERR_INVALID with a message for blur_r outside [-1, 3], weights
 * with (2 r + 1) ww + 2 fw > 2^24, a rotating frame with an edge above 4096, |a0|, |a1|, |a3|, |a4| > 65537 or |a2|, |a5| > 2^30 (the
 * bounds keep every intermediate inside int32), and in / out that overlap.  The kernels do not trust the device copy of the table: they
 * clamp blur_r, take over-weight entries as "no blur" and test every gather's source index.
 * bvc_clip_post_host: the same arithmetic compiled for the host (csrc/augment.h), on host memory; needs no GPU. */
typedef struct bvc_frame_post {
    int32_t blur_r;
    uint32_t blur_ww, blur_fw;
    int32_t gray;
    int32_t rotate;
    int32_t rot[6];
} bvc_frame_post; /* 44 bytes */
#define BVC_AUG_MAX_BLUR_RADIUS 4.0f /* Gaussian radius; gives blur_r <= 3 */
int bvc_aug_blur_weights(float radius, int32_t* r, uint32_t* ww, uint32_t* fw);
int64_t bvc_op_clip_post_workspace(int F, int H, int W);
int bvc_op_clip_post(const uint8_t* in_dev, const bvc_frame_post* table_host, const bvc_frame_post* table_dev, int F, int H, int W,
                     uint8_t* out_dev, void* workspace_dev, void* stream);
int bvc_clip_post_host(const uint8_t* in, const bvc_frame_post* table, int F, int H, int W, uint8_t* out);
/* RandAugment (the timm "rand-m7-n4-mstd0.5-inc1" family of the VideoMAE fine-tuning recipes): a third stage on uint8 frames
 * [F][3][H][W].  One bvc_frame_randaug per frame: up to BVC_RANDAUG_MAX_OPS stages, applied in order, each on the frame as the stage
 * before left it; an op may repeat.  Statistics (histograms, the mean) are of that one frame as it stands.  Each op gives the bytes of
 * the named PIL call on an RGB frame (arithmetic in csrc/randaug.h); the device, the host twin and PIL agree bit for bit.
 *   op  0 AutoContrast  ImageOps.autocontrast         1 Equalize     ImageOps.equalize           2 Invert      ImageOps.invert
 *       3 Posterize     ival = bits, 0 .. 8           4 Solarize     ival = threshold, 0 .. 256  5 SolarizeAdd ival = add, 0 .. 110
 *       6 Color  7 Contrast  8 Brightness  9 Sharpness  ImageEnhance.*(im).enhance(fval), fval finite and >= 0
 *       10 ShearX  11 ShearY  12 TranslateX  13 TranslateY  14 Rotate  Image.transform(AFFINE, NEAREST) / Image.rotate(NEAREST):
 *       aff[6] is the inverse map in 16.16 fixed point as in bvc_frame_post.rot (bvc.augment.affine_coeffs, rotation_coeffs), with the
 *       same bounds; pixels whose source lies outside the frame take fill[0 .. 2]
 *   ival, fval and aff are read only by the ops named with them.
 * bvc_op_clip_randaug: in_dev / table_dev / out_dev / workspace_dev are device memory, table_host is the same table in host memory,
 * read during the call only: validated there, without a device sync, and it tells the call what to launch.  The host walks the stage
 * index; per stage one read-write pass over the frames that have such a stage, and, when some frame's stage is AutoContrast, Equalize
 * or Contrast, before it one read of those frames into integer histograms (integer LDS and global atomics: order-independent, so
 * nothing for the deterministic mode to switch) and a small kernel that turns them into byte tables.  Frames alternate between out_dev
 * and workspace_dev (bvc_op_clip_randaug_workspace bytes, 4-byte aligned, overlapping neither in nor out) so that each frame's last
 * stage lands in out_dev.  A table with nops == 0 everywhere is one device-to-device copy.  BVC_ERR_INVALID with a message that names the
 * field for nops outside 0 .. 8, an unknown op, a non-finite or negative fval, an ival outside its op's range, an affine op on a frame
 * with an edge above 4096 or with |aff[0, 1, 3, 4]| > 65537 or |aff[2, 5]| > 2^30, and in / out that overlap - before anything is
 * launched.  The kernels do not trust the device copy of the table: they clamp nops and ival, copy through an unknown op and test every
 * gather's source index.
 * bvc_clip_randaug_host: the same arithmetic compiled for the host, on host memory; needs no GPU.
 * bvc_frame_randaug_bytes: sizeof the entry, for bindings that restate its layout. */
#define BVC_RANDAUG_MAX_OPS 8
typedef struct bvc_randaug_stage {
    int32_t op;
    int32_t ival;
    float fval;
    int32_t aff[6];
} bvc_randaug_stage; /* 36 bytes */
typedef struct bvc_frame_randaug {
    int32_t nops;
    uint8_t fill[4]; /* r, g, b, unused */
    bvc_randaug_stage stage[BVC_RANDAUG_MAX_OPS];
} bvc_frame_randaug; /* 296 bytes */
int bvc_frame_randaug_bytes(void);
int64_t bvc_op_clip_randaug_workspace(int F, int H, int W);
int bvc_op_clip_randaug(const uint8_t* in_dev, const bvc_frame_randaug* table_host, const bvc_frame_randaug* table_dev, int F, int H, int W,
                        uint8_t* out_dev, void* workspace_dev, void* stream);
int bvc_clip_randaug_host(const uint8_t* in, const bvc_frame_randaug* table, int F, int H, int W, uint8_t* out);
/* JPEG decode (baseline Huffman) to planar RGB uint8 [3][H][W], the bytes libjpeg-turbo gives at its defaults (ISLOW IDCT, fancy
 * upsampling, the 16-bit YCbCr tables; arithmetic in csrc/jpeg.h, shared by the kernels and the host twin).
 * Decoded: 8-bit SOF0 / SOF1, one component (three equal channels) or three YCbCr components with luma 1x1, 2x1 or 2x2 and chroma
 * 1x1, JFIF colour or Adobe transform 1, up to four DQT tables (8- or 16-bit), Huffman tables 0 and 1 of each class, DRI / RSTn, one
 * scan, 1 .. BVC_JPEG_MAX_DIM pixels a side.  Everything else is refused at parse with a BVC_JPEG_REFUSE_* reason.
 * bvc_jpeg_parse: plain C++, NO HIP call on its path - it may run in loader workers that never open the device.  Walks the markers
 * (every length checked against n), fills *info (tables in decode form, rebuilt from the DHT counts; over-subscribed, over-long or
 * out-of-range tables are refused, so the device never sees a table it could walk off), and scans the entropy-coded bytes once for
 * 0xFF to list the independent segments: seg[4 * i + 0 .. 3] = first byte, end byte (offsets into data), first MCU, MCU count.  A
 * file without DRI is one segment; RSTn numbering is checked; the last segment takes every MCU that is left.  At most max_seg records
 * are written, info->nseg is the full count (seg may be NULL with max_seg 0).  Returns BVC_OK, a positive BVC_JPEG_REFUSE_* (also in
 * info->reason), or BVC_ERR_INVALID for a null argument.  A scan that runs to the end of the data without EOI is not refused: the
 * file decodes as far as it goes and BVC_JPEG_ST_NO_EOI is pre-set in info->flags and raised in the image's status.
 * Status bits of a decoded image (0 = every segment decoded cleanly): a reader that needs bits past the end of its segment
 * (TRUNCATED), a code that matches nothing (BAD_CODE) and a run past coefficient 63 (BAD_RUN) end the segment; its remaining blocks
 * are DC-only at the component's last DC prediction.  The reader never forms an address outside [begin, end) of its segment.
 * The caller fills blob_offset (where the file's bytes begin in the blob) and seg_first (index of the image's first record in the
 * concatenated segment table); bvc_op_jpeg_decode_workspace fills plane_offset of n infos and returns the workspace bytes (the
 * components' uint8 planes padded to whole MCUs, 1.5 bytes per padded pixel at 4:2:0).  Infos with reason != 0 take no part.
 * bvc_op_jpeg_decode: blob_dev / infos_dev / segs_dev / out_offsets_dev / status_dev / workspace_dev are device memory; infos_host,
 * segs_host and out_offsets_host are the same tables in host memory, read during the call only: validated there (every range against
 * blob_bytes, out_bytes and the workspace) and they set the launch geometry.  Two kernels, no synchronisation, no atomics: (1) one
 * lane per segment - entropy decode, dequantise, IDCT with the block in LDS, 8-byte rows into the planes; (2) upsample, colour-convert
 * and crop into out_dev + out_offsets[i].  status_dev[i] is written for every image (0 for refused ones, whose output is not
 * touched).  lanes = segments per wave, 1 .. 64, or 0 to let the call choose by the number of segments.  stages = 3; 1 or 2 launch one
 * of the two kernels alone, for measurements (2 reads the planes an earlier call left in the workspace).
 * bvc_jpeg_decode_host: parse's info and segments -> RGB, the same arithmetic compiled for the host; returns the status bits (>= 0).
 * bvc_jpeg_info_bytes: sizeof the descriptor, for bindings that restate its layout.
 *
 * bvc_op_jpeg_decode_split / _workspace: the same call with a second path for long segments - a file without DRI is ONE segment and
 * would sit on one lane.  split: segments of at least this many bytes (and of at least 2 * BVC_JPEG_SPLIT_MIN_CHUNK and fewer than
 * 2^28 bytes) take the split path, 0 = none; every other segment goes through the one-lane kernel unchanged, in the same call.
 * chunk: bytes per lane, 0 (BVC_JPEG_SPLIT_DEFAULT_CHUNK) or >= BVC_JPEG_SPLIT_MIN_CHUNK.  Chunk layout, deterministic:
 *   one workgroup of T = BVC_JPEG_SPLIT_THREADS lanes per split segment [begin, end);
 *   c = max(chunk, ceil((end - begin) / T) rounded up to a multiple of 4)      (bvc_jpeg_split_chunk)
 *   chunk j = bytes [begin + j c, min(begin + (j + 1) c, end)), j < ceil((end - begin) / c) <= T, on lane j.
 * A lane decodes the symbols that start in its chunk.  Lane 0 enters at the true state, every other lane at a guess; in rounds, lane
 * j takes over the exit state lane j - 1 recorded (bit position, block within the MCU, zig-zag index, dead) and decodes again until
 * a workgroup-wide reduction says that no exit changed - at most chunks - 1 rounds, after which the chain is right by induction
 * from chunk 0.  Bit positions are those of the RAW file, a stuffed 00 belonging to its FF.  All waiting is the barrier of one
 * workgroup: no workgroup waits for another, no atomics.  A speculative lane that meets a bad code, a bad run or the data's end
 * records "dead" and raises nothing.  An exclusive scan of the blocks completed per chunk places every chunk; blocks beyond the
 * segment's last (the padding bits decode as garbage) are dropped; a last pass writes AC coefficients dequantised (64 int16 per
 * block, natural order) and DC differences into the workspace; a wrapping 32-bit scan per component turns the differences into DC
 * values; jpeg_idct_kernel (one lane per block) writes the planes, and the colour kernel runs as before.  When the true chain ends
 * before the segment's last block (what the one-lane decoder reports as TRUNCATED, BAD_CODE or BAD_RUN) the segment is flagged on
 * the device and decoded again, whole, by the one-lane decoder in a launch that skips every other segment: bytes and status of a
 * damaged file are the one-lane path's by construction.  info_out_dev: int32 [n][2], per image the segments that fell back and the
 * most hand-over rounds one of its segments took (0, 0 without split segments).  The workspace holds, after that of
 * bvc_op_jpeg_decode, per segment a flag, a round count and a routed segment record, and per 8 x 8 block 4 + 128 bytes.
 * bvc_jpeg_decode_host_split: the split path in plain C++, its lanes run one after another (csrc/jpeg.h, decode_segment_split);
 * info_out: int32 [2] as above.  bvc_jpeg_split_chunk: c of the rule above for a segment of `bytes` bytes. */
#define BVC_JPEG_MAX_DIM 4096
#define BVC_JPEG_SPLIT_THREADS 512
#define BVC_JPEG_SPLIT_MIN_CHUNK 16
#define BVC_JPEG_SPLIT_DEFAULT_CHUNK 64
enum {
    BVC_JPEG_REFUSE_NOT_JPEG = 1, BVC_JPEG_REFUSE_BAD_LENGTH = 2, BVC_JPEG_REFUSE_PROGRESSIVE = 3, BVC_JPEG_REFUSE_ARITHMETIC = 4,
    BVC_JPEG_REFUSE_LOSSLESS = 5, BVC_JPEG_REFUSE_PRECISION = 6, BVC_JPEG_REFUSE_COMPONENTS = 7, BVC_JPEG_REFUSE_RGB = 8,
    BVC_JPEG_REFUSE_SAMPLING = 9, BVC_JPEG_REFUSE_MULTI_SCAN = 10, BVC_JPEG_REFUSE_HUFFMAN = 11, BVC_JPEG_REFUSE_QUANT = 12,
    BVC_JPEG_REFUSE_SIZE = 13, BVC_JPEG_REFUSE_SCAN_HEADER = 14, BVC_JPEG_REFUSE_RESTART = 15, BVC_JPEG_REFUSE_HEADER = 16
};
enum { BVC_JPEG_ST_TRUNCATED = 1, BVC_JPEG_ST_BAD_CODE = 2, BVC_JPEG_ST_BAD_RUN = 4, BVC_JPEG_ST_NO_EOI = 8 };
typedef struct bvc_jpeg_huff {
    uint16_t look[256];  /* by the next 8 bits: (code length << 8) | symbol, 0 = the code is longer than 8 bits */
    int32_t maxcode[18]; /* [l], l = 1 .. 16: largest code of length l, -1 = none; [17] ends every search */
    int32_t valoff[18];  /* [l]: huffval index of a code of length l = code + valoff[l] (valptr - mincode) */
    uint8_t huffval[256];
} bvc_jpeg_huff; /* 912 bytes */
typedef struct bvc_jpeg_info {
    int32_t width, height;
    int32_t ncomp;            /* 1 or 3 */
    int32_t hs, vs;           /* luma sampling: 1x1, 2x1 or 2x2 (1x1 for one component) */
    int32_t mcus_x, mcus_y;
    int32_t restart_interval; /* MCUs, 0 = none */
    int32_t scan_begin, scan_end; /* the entropy-coded bytes, offsets into the file */
    int32_t nseg;
    int32_t reason;           /* 0, or the BVC_JPEG_REFUSE_* parse returned */
    int32_t flags;            /* status bits known at parse (BVC_JPEG_ST_NO_EOI) */
    int32_t seg_first;        /* caller: index of the first segment record */
    int64_t blob_offset;      /* caller: where the file begins in the blob */
    int64_t plane_offset;     /* bvc_op_jpeg_decode_workspace: where the planes begin in the workspace, a multiple of 16 */
    uint8_t tq[4], td[4], ta[4]; /* per component: quantisation table, DC table, AC table (huff[td], huff[2 + ta]) */
    uint32_t pad_;
    uint16_t qt[4][64];       /* natural (row-major) order */
    bvc_jpeg_huff huff[4];    /* DC 0, DC 1, AC 0, AC 1 */
} bvc_jpeg_info; /* 4248 bytes */
int bvc_jpeg_info_bytes(void);
int bvc_jpeg_parse(const uint8_t* data, int64_t n, bvc_jpeg_info* info, int32_t* seg, int max_seg);
int bvc_jpeg_decode_host(const uint8_t* data, int64_t n, const bvc_jpeg_info* info, const int32_t* seg, uint8_t* out_rgb);
int64_t bvc_op_jpeg_decode_workspace(bvc_jpeg_info* infos_host, int n);
int bvc_op_jpeg_decode(const uint8_t* blob_dev, int64_t blob_bytes, const bvc_jpeg_info* infos_host, const bvc_jpeg_info* infos_dev, int n,
                       const int32_t* segs_host, const int32_t* segs_dev, int64_t nseg, const int64_t* out_offsets_host,
                       const int64_t* out_offsets_dev, uint8_t* out_dev, int64_t out_bytes, int32_t* status_dev, void* workspace_dev,
                       int64_t workspace_bytes, int lanes, int stages, void* stream);
int bvc_jpeg_split_chunk(int bytes, int chunk);
int bvc_jpeg_decode_host_split(const uint8_t* data, int64_t n, const bvc_jpeg_info* info, const int32_t* seg, int split, int chunk,
                               uint8_t* out_rgb, int32_t* info_out);
int64_t bvc_op_jpeg_decode_split_workspace(bvc_jpeg_info* infos_host, int n);
int bvc_op_jpeg_decode_split(const uint8_t* blob_dev, int64_t blob_bytes, const bvc_jpeg_info* infos_host, const bvc_jpeg_info* infos_dev,
                             int n, const int32_t* segs_host, const int32_t* segs_dev, int64_t nseg, const int64_t* out_offsets_host,
                             const int64_t* out_offsets_dev, uint8_t* out_dev, int64_t out_bytes, int32_t* status_dev, void* workspace_dev,
                             int64_t workspace_bytes, int lanes, int stages, int split, int chunk, int32_t* info_out_dev, void* stream);

/* ------------------------------------------------------------------------------------------------
 * JEPA encoder and predictor (pretraining/predictive/vision_transformer.py).  Same conventions as above: flat f32
 * parameter / gradient buffers whose entries carry the reference's state-dict keys (pos_embed, patch_embed.proj.*,
 * blocks.N.{norm1,attn.qkv,attn.proj,norm2,mlp.fc1,mlp.fc2}.*, norm.* / mask_token, predictor_pos_embed,
 * predictor_embed.*, predictor_blocks.N.*, predictor_norm.*, predictor_proj.*), borrowed device pointers, caller's stream.
 * Token index lists are int32 (the reference's int64 masks are narrowed by the host shim).                          */
typedef struct bvc_vit_config {
    int image_size, patch_size, num_channels, num_frames, tubelet_size;
    int embed_dim, depth, num_heads, mlp_hidden;
    float eps; /* 1e-6: vit_base() etc. build LayerNorm with eps=1e-6 (vision_transformer.py:546-568) */
} bvc_vit_config;
typedef struct bvc_vit_ctx bvc_vit_ctx;
int bvc_vit_param_count(const bvc_vit_config* cfg);
int64_t bvc_vit_param_numel(const bvc_vit_config* cfg);
int bvc_vit_param_info(const bvc_vit_config* cfg, int index, char* name, int name_cap, int64_t* offset, int64_t* numel,
                       int* ndim, int64_t shape[5]);
int bvc_vit_create(const bvc_vit_config* cfg, int max_batch, bvc_vit_ctx** out);
void bvc_vit_destroy(bvc_vit_ctx* ctx);
/* Replaces encoder(imgs, masks_enc) and target_encoder(imgs) (pretrain_jepa.py:386,395; VisionTransformer.forward,
 * vision_transformer.py:378-402).  imgs f32 [B][T][C][H][W]; idx int32 [B][ntok] = tokens kept per sample, NULL = all;
 * out f32 [B*ntok][embed_dim] (after the final LayerNorm). */
int bvc_vit_forward(bvc_vit_ctx* ctx, const float* imgs_dev, const int* idx_dev, int batch, int ntok, const float* params_dev,
                    float* out_dev, void* stream);
int bvc_vit_forward_px(bvc_vit_ctx* ctx, const void* imgs_dev, const bvc_pixel_format* fmt, const int* idx_dev, int batch, int ntok,
                       const float* params_dev, float* out_dev, void* stream);
/* d(out) f32 [B*ntok][embed_dim] -> flat gradients (overwritten); buckets reported tail-first as for VideoMAE. */
int bvc_vit_backward(bvc_vit_ctx* ctx, const float* dout_dev, float* grads_dev, bvc_bucket_fn on_bucket, void* user, void* stream);
/* as bvc_videomae_shadow */
int bvc_vit_shadow(bvc_vit_ctx* ctx, int valid, void** shadow_bf16, int64_t* numel);
/* stochastic depth / hidden dropout of the next forward and its backward (bvc_branch_drop above); samples = batch */
int bvc_vit_set_drop(bvc_vit_ctx* ctx, const bvc_branch_drop* drop, int samples, void* stream);

typedef struct bvc_predictor_config {
    int seq_len;    /* tokens of the full grid (num_patches of the encoder) */
    int embed_dim;  /* encoder width */
    int pred_dim;   /* predictor_embed_dim (384) */
    int depth, num_heads, mlp_hidden;
    float eps;
} bvc_predictor_config;
typedef struct bvc_pred_ctx bvc_pred_ctx;
int bvc_predictor_param_count(const bvc_predictor_config* cfg);
int64_t bvc_predictor_param_numel(const bvc_predictor_config* cfg);
int bvc_predictor_param_info(const bvc_predictor_config* cfg, int index, char* name, int name_cap, int64_t* offset,
                             int64_t* numel, int* ndim, int64_t shape[5]);
int bvc_predictor_create(const bvc_predictor_config* cfg, int max_batch, int max_sets, int max_tokens, bvc_pred_ctx** out);
void bvc_predictor_destroy(bvc_pred_ctx* ctx);
/* Replaces predictor(z, masks_enc, masks_pred) (pretrain_jepa.py:396; VisionTransformerPredictor.forward,
 * vision_transformer.py:494-535).  z f32 [B*Nc][embed_dim]; idx_ctx int32 [B][Nc]; idx_pred int32 [nsets][B][Np];
 * out f32 [nsets*B*Np][embed_dim], rows ordered mask-set-major then sample, as apply_masks/cat produce them. */
int bvc_predictor_forward(bvc_pred_ctx* ctx, const float* z_dev, const int* idx_ctx_dev, const int* idx_pred_dev, int B, int Nc,
                          int nsets, int Np, const float* params_dev, float* out_dev, void* stream);
int bvc_predictor_backward(bvc_pred_ctx* ctx, const float* dout_dev, float* grads_dev, float* dz_dev, void* stream);
/* as bvc_videomae_shadow */
int bvc_predictor_shadow(bvc_pred_ctx* ctx, int valid, void** shadow_bf16, int64_t* numel);
/* as bvc_vit_set_drop; samples = nsets * B sequences, ordered as the predictor's rows (mask-set-major) */
int bvc_predictor_set_drop(bvc_pred_ctx* ctx, const bvc_branch_drop* drop, int samples, void* stream);
/* The same, reporting gradient ranges tail-first (bvc_bucket_fn, as bvc_videomae_backward / bvc_vit_backward do) so that the
 * data-parallel wrapper can start the predictor's all-reduce per block: DDP(predictor, static_graph=True), pretrain_jepa.py:303. */
int bvc_predictor_backward_cb(bvc_pred_ctx* ctx, const float* dout_dev, float* grads_dev, float* dz_dev, bvc_bucket_fn on_bucket,
                              void* user, void* stream);

/* forward_target's post-processing (pretrain_jepa.py:387-392): F.layer_norm without affine over the feature dim, then the
 * rows the prediction masks select: out[(i*B+b)*Np + j] = LN(h[b*L + idx_pred[i][b][j]]) */
int bvc_op_target_select(const float* h, const int* idx_pred, float* out, int nsets, int B, int Np, int L, int D, float eps, void* stream);
/* F.smooth_l1_loss(z, h), beta = 1, mean (pretrain_jepa.py:400); workspace = bvc_op_smooth_l1_workspace(n) floats */
int bvc_op_smooth_l1_workspace(int64_t n);
int bvc_op_smooth_l1_fwd(const float* z, const float* h, int64_t n, float* workspace, float* loss, void* stream);
int bvc_op_smooth_l1_bwd(const float* z, const float* h, const float* grad_loss, int64_t n, float* dz, void* stream);
/* target <- momentum * target + (1 - momentum) * online over a flat range (pretrain_jepa.py:431-432) */
int bvc_op_ema(float* target, const float* online, int64_t n, float momentum, void* stream);
/* mean over the tokens of each sample, f32 [batch][ntok][dim] -> [batch][dim], and its backward (dx = dmean / ntok for every
 * token): `xmodel(inputs).mean(1)` of benchmarks/compute_embeddings_jepa.py:242 and the pooling between a ViT trunk and the
 * SimCLR head (BASELINE config 5).  Fixed summation order. */
int bvc_op_token_mean(const float* x, int batch, int ntok, int dim, float* out, void* stream);
int bvc_op_token_mean_bwd(const float* dmean, int batch, int ntok, int dim, float* dx, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Operator-level entry points (the kernels the step is built from; also used by the parity tests). */
enum { BVC_GEMM_NT = 0, BVC_GEMM_NN = 1, BVC_GEMM_TN = 2 };
enum {
    BVC_EPI_F32 = 0, BVC_EPI_BF16 = 1, BVC_EPI_GELU = 2, BVC_EPI_RESID = 3, BVC_EPI_POS = 4, BVC_EPI_E2D = 5,
    BVC_EPI_LOSS = 6, BVC_EPI_DGELU = 7, BVC_EPI_F32_BF16 = 8, BVC_EPI_RELU = 9, BVC_EPI_DRELU = 10,
    BVC_EPI_NCE = 11, BVC_EPI_NCE_BWD = 12, BVC_EPI_RESID_LN = 13, BVC_EPI_DLN = 14, BVC_EPI_RESID_GATE = 15
};
/* BVC_EPI_GELU writes TWO bf16 outputs: C2 = gelu(v + bias) and C = gelu'(v + bias), the factor the backward product needs (the
 * forward epilogue has the erf and the exponential at hand; the backward epilogue BVC_EPI_DGELU, C = v * aux with aux = that C, is
 * then one multiply per element).  BVC_EPI_RELU / BVC_EPI_DRELU: C = max(v + bias, 0) / C = v where aux > 0. */
/* C[M,N] = epilogue(alpha * alpha_dev[0] * sum_k A(m,k) B(k,n)); bf16 operands, f32 accumulation.
 * Replaces the nn.Linear forward / backward GEMMs that ATen dispatches for HF:225-237,269-275,299-322. */
typedef struct bvc_gemm_desc {
    const void* A; const void* B;   /* bf16 */
    int M, N, K, lda, ldb;
    uint32_t a_bytes, b_bytes;      /* extents of the A / B allocations (rows past them read as 0) */
    float alpha;
    const float* alpha_dev;         /* optional device scalar multiplied into alpha */
    int epi, split_k;
    void* C; int ldc; int seg_rows; void* C2;               /* seg_*: see below */
    const float* bias; const float* resid; const void* aux; int ldaux; int seg_stride;
    const int* rowtok; const float* pos; const float* labels; float* partial;
    int rin, rout;
    float* rowsum;                  /* TN only: rowsum[m] += alpha * sum_k A(m,k)  (bias gradient of the same dY) */
    /* BVC_EPI_RESID_LN / BVC_EPI_DLN: the LayerNorm next to a Linear whose output rows are 384 wide (VideoMAE decoder, JEPA
     * predictor), computed in the product's epilogue on 128 x 384 tiles that hold complete rows (N == ldc == 384, one problem,
     * tile config 12 / -1).  Replaces the separate nn.LayerNorm passes of HF:339-357 / vision_transformer.py:225-231.
     *   RESID_LN (NT):  v = alpha AB + bias + resid -> C (f32);  C2 (bf16) = (v - mean) rstd ln_gamma + ln_beta, biased variance,
     *                   rstd = 1 / sqrt(var + ln_eps);  ln_mean / ln_rstd [M] written.
     *   DLN (NN):       g = alpha AB = d/d(LayerNorm output);  xhat = (ln_x - ln_mean) ln_rstd;
     *                   C (f32, in/out) += ln_rstd (g gamma - mean(g gamma) - xhat mean(g gamma xhat));  C2 (bf16) = the new C;
     *                   ln_dgamma += sum_m g xhat, ln_dbeta += sum_m g  (through ln_part: scratch of 256 x 2 x 384 floats). */
    const float* ln_gamma; const float* ln_beta;
    float* ln_mean; float* ln_rstd;
    float ln_eps; int seg_off;
    const float* ln_x;
    float* ln_part; float* ln_dgamma; float* ln_dbeta;
    /* BVC_EPI_RESID_LN / BVC_EPI_DLN only, optional (seg_rows == 0: none).  The product's M rows are the segments [seg_off, seg_off +
     * seg_rows) of every seg_stride rows of a longer array, stored compact: row r of segment c is row c seg_stride + seg_off + r of
     * that array.  ONE side pointer of the problem is addressed through the map - `resid` of RESID_LN (read), `C` of DLN (the f32
     * residual gradient, read and written in place); every other pointer is compact.  seg_rows is a multiple of 128, so a 128-row
     * tile lies in one segment and the map is one scalar per tile; bvc_op_gemm rejects a map that is not of that form (seg_rows a
     * multiple of 128 that divides M, 0 <= seg_off, seg_off + seg_rows <= seg_stride) and any map on another epilogue.  (The three fields sit in the alignment holes behind ldc, ldaux
     * and ln_eps: the descriptor's size and every other offset are what they were.) */
} bvc_gemm_desc;
/* tile_cfg: -1 auto; 0 = 128x128, 1 = 128x64, 2 = 64x64 (one workgroup per tile); 6 / 7 = persistent 128x128 / 128x64,
 * 9 = persistent 128x128 with deferred stores; 10 / 11 = 256x256 / 256x128, one 512-thread workgroup per CU (gemm8.hip);
 * 12 = 128x384 (TN only); 13 = 10 for TN products with plain f32 outputs that are ACCUMULATED: C += A^T B by f32 atomics even when
 * split_k == 1 (C pre-zeroed or holding the values to add to, as for split_k > 1) - bvc_op_gemm_plan_dw returns it for groups whose
 * unsplit tiles fill half to 15/16 of the chip: their K ranges are then balanced over all CUs.
 * (3-5 and 8 are experiment kernels that exist only in a -DBVC_EXPERIMENTS build.)  stages: -1 auto, 2..4 = K-loop variant. */
int bvc_op_gemm(const bvc_gemm_desc* problems, int count, int layout, int tile_cfg, int stages, void* stream);
int bvc_op_gemm_num_tiles(const bvc_gemm_desc* problem, int tile_cfg);
/* BVC_EPI_RESID_GATE: one NT product C f32 = resid + gate .* (alpha AB + bias) with the gate of (layer, branch) of `drop`
 * (path_scale indexed [(2 layer + branch) * samples + m / rows_per_sample], samples = ceil(M / rows_per_sample)); split_k == 1,
 * tile_cfg -1 / 0 / 1 / 2.  bvc_op_gemm rejects this epilogue (it has no gate to give it).  bvc_op_gemm_gate_kernel: the
 * instantiation it runs, as bvc_op_gemm_kernel reports the others. */
int bvc_op_gemm_gate(const bvc_gemm_desc* problem, const bvc_branch_drop* drop, int layer, int branch, int tile_cfg, void* stream);
int bvc_op_gemm_gate_kernel(const bvc_gemm_desc* problem, int tile_cfg, char* name, int name_cap);
/* Introspection of the selection above, nothing is launched: the kernel instantiation bvc_op_gemm would run for these problems,
 * named as rocprofv3 prints it (e.g. "bvc::gemm8_kernel<256, true, true, 2>"), so that per-product timings can be attributed to the
 * rows of a kernel-stats table (bench.py's `roofline.kernels`); and the (tile_cfg, split_k) plan the step uses for a group of
 * weight-gradient products (returns the tile config, writes split_k into the descriptors). */
int bvc_op_gemm_kernel(const bvc_gemm_desc* problems, int count, int layout, int tile_cfg, int stages, char* name, int name_cap);
/* 1 when the step runs the LayerNorms of a transformer stack of this shape (tokens rows, width, MLP width, heads) inside the epilogues of
 * the neighbouring products (BVC_EPI_RESID_LN / BVC_EPI_DLN) under the current options, 0 when they are separate passes */
int bvc_op_row_ln_selected(int tokens, int width, int mlp_width, int heads);
int bvc_op_gemm_plan_dw(bvc_gemm_desc* problems, int count);

/* softmax(QK^T/sqrt(d))V for head_dim d = 32, 64, 80, 88, 96 or 128; qkv bf16 [B*N][3*d*H]; replaces HF:181-206 / SDPA (HF:239-252) and
 * Attention.forward of pretraining/predictive/vision_transformer.py:198-210 (the ViT-B predictor has d = 32, the ViT-Ti predictor
 * d = 128; ViT-H / ViT-g encoders and VideoMAE-H have 80 / 88-wide heads, which run in place: head h at column h*d) */
int bvc_op_attention_fwd(const void* qkv, void* ctx_out, float* lse, int B, int N, int H, int head_dim, void* stream);
int bvc_op_attention_bwd(const void* qkv, const void* ctx_in, const void* dctx, const float* lse, float* delta_scratch,
                         void* dqkv, int B, int N, int H, int head_dim, void* stream);
/* one of the backward's two kernels alone (timing probes): part 1 = dQ (+ delta_scratch), part 2 = dK / dV (reads delta_scratch) */
int bvc_op_attention_bwd_part(const void* qkv, const void* ctx_in, const void* dctx, const float* lse, float* delta_scratch,
                              void* dqkv, int B, int N, int H, int head_dim, int part, void* stream);
/* the head width a model context allocated now runs attention at for heads of head_dim dims (stack.h attn_width): head_dim itself
 * for 32 / 64 / 80 / 88 / 96 / 128 (80 / 88: 96 while "head_pad" is 1), the next of 32 / 64 / 96 / 128 (zero-padded) otherwise */
int bvc_op_attention_width(int head_dim);
/* the forward / backward with an explicit softmax scale (0 = 1/sqrt(head_dim)): what a caller that zero-pads narrower heads to a
 * wider head_dim passes (1/sqrt of the true width; bvc_set_option("head_pad", 1) runs 80 / 88 that way) */
int bvc_op_attention_fwd_scaled(const void* qkv, void* ctx_out, float* lse, int B, int N, int H, int head_dim, float softmax_scale,
                                void* stream);
int bvc_op_attention_bwd_scaled(const void* qkv, const void* ctx_in, const void* dctx, const float* lse, float* delta_scratch,
                                void* dqkv, int B, int N, int H, int head_dim, float softmax_scale, void* stream);
/* The attention probabilities the forward never stores (HF:181-206 eager attention_probs, before dropout): probs f32 [B][H][N][N],
 * row = query, column = key, = exp2(q.k * scale * log2 e - lse[query]) from the same qkv and the lse (log2 units) that
 * bvc_op_attention_fwd / _fwd_scaled wrote for it; softmax_scale as for the _scaled entry points (0 = 1/sqrt(head_dim)).  Every one of
 * the B * H * N * N elements is written (64-bit addressing: the output may exceed 4 GiB; qkv may not), nothing else is.  No atomics:
 * the same bits on every run. */
int bvc_op_attention_probs(const void* qkv, const float* lse, float* probs, int B, int N, int H, int head_dim, float softmax_scale,
                           void* stream);
/* Embedding retrieval (csrc/retrieval.hip; the reference's notebooks/EvaluateEmbeddings.ipynb get_nn_score / topk_retrieval): for
 * each of the Q f32 query rows (row stride ldq elements) the k <= 64 best of the N f32 key rows (row stride ldk elements) of D
 * columns, as out_idx int32 [Q][k] and out_val f32 [Q][k].  metric 0 = cosine: score = q.key / (|q| |key|) with inverse norm 0
 * for a zero row, out_val = the cosine distance 1 - score (sklearn cosine_distances); metric 1 = Euclidean: d2 = max(|q|^2 +
 * |key|^2 - 2 q.key, 0), out_val = sqrt(d2) (sklearn euclidean_distances).  All arithmetic is f32: q.key is one fused
 * multiply-add chain over d = 0 .. D-1 whatever tile, key split or chunk the pair falls into.  Each row of the outputs is ordered
 * best first: out_val ascending (a non-increasing function of the score) and, among bit-equal out_val, out_idx ascending; with
 * fewer than k keys the remaining slots hold index -1 and distance +inf.  The reported index is key_base + the key's row.
 *   key_splits    0 = chosen by the library (bvc_op_topk_splits), else that many ranges of key tiles run as workgroups of their own
 *                 (capped at the number of 128-key tiles); the result does not depend on it, bit for bit.
 *   accumulate    1 = out_idx / out_val hold the result of earlier calls (same queries, metric and k, other keys): this call
 *                 merges its keys into them, and a loop of calls over the chunks of a gallery gives the bits of one call over the
 *                 whole gallery.  0 = they are overwritten.
 *   workspace     bvc_op_topk_workspace(Q, N, D, k, key_splits) bytes (8-byte aligned; -1 for invalid sizes): row statistics and the
 *                 per-split lists.  No [Q][N] array exists anywhere.
 * Read: the D columns of the Q and N rows (never the ldq - D / ldk - D padding), and out_idx / out_val when accumulate.  Written:
 * the Q * k indices, the Q * k values, the workspace; nothing else.  No atomics on floats (integer LDS counters only, and the order
 * above makes the result independent of arrival order): the same bits on every run.  BVC_ERR_INVALID (bvc_last_error) and nothing
 * launched for k outside 1 .. 64, a non-positive size, a null pointer, a stride below D or key_base + N beyond int. */
int64_t bvc_op_topk_workspace(int Q, int N, int D, int k, int key_splits);
/* what key_splits = 0 resolves to for this shape (-1 for invalid sizes) */
int bvc_op_topk_splits(int Q, int N, int D, int k);
int bvc_op_topk(const float* queries, int64_t ldq, const float* keys, int64_t ldk, int Q, int N, int D, int k, int metric,
                int key_splits, int key_base, int accumulate, int* out_idx, float* out_val, void* workspace, void* stream);
/* Linear separability (csrc/separability.hip; the reference's notebooks/EvaluateEmbeddings.ipynb get_separability_score with
 * method='svm': StandardScaler + LinearSVC).  bvc_op_colstats: StandardScaler's statistics of the n f32 rows (row stride ldx
 * elements) of D columns: mean f32 [D] and inv_std f32 [D] = 1 / sqrt(population variance), exactly 1 where the variance is exactly 0;
 * sums in float64 in a fixed order, one rounding to f32 each.  Read: the D columns of the n rows (never the ldx - D padding);
 * written: mean and inv_std.
 * bvc_op_linear_pass: one evaluation for K one-vs-rest squared-hinge problems at once.  Row i is used as xs_i = [(x_i - mean) *
 * inv_std (two f32 roundings), 1]: D + 1 columns, the last one carrying the (regularised) intercept; the standardised matrix is
 * never stored.  W and V are f32 [K][D + 1]; column j of the outputs belongs to label class0 + j: y_ij = +1 where labels[i]
 * (int32, on the device) == class0 + j, else -1 (a two-class problem is one column, class0 = 1).  z_ij = w_j . xs_i is one f32
 * fused-multiply-add chain over d = 0 .. D starting at 0.
 *   mode 0 GRAD      out_loss[j] = sum_i max(0, 1 - y z)^2,  out_G[j][d] = sum_i a_ij xs_id with a = -2 C y max(0, 1 - y z):
 *                    C * out_loss + |w_j|^2 / 2 is the objective and out_G + W its gradient.
 *   mode 1 HESSVEC   out_G[j][d] = sum_i a_ij xs_id with a = 2 C [1 - y z(W) > 0] (xs_i . v_j): out_G + V is the generalised
 *                    Hessian at W times V.  out_loss is not used.
 *   mode 2 DECISION  out_pred int32 [n] = the column of the largest z of the row (the smaller column among equal ones, as
 *                    numpy.argmax), for K = 1 z > 0; out_dec f32 [n][K], when not null, receives z.  labels, V, C, out_G are not used.
 * Sums over rows are f32 chains in ascending row order inside each of bvc_op_linear_pass_splits(n, D, K) contiguous row ranges
 * (whole tiles of bvc_op_linear_pass_tile_rows(D) rows), and the ranges are added in ascending order: no atomics on floats, the
 * same bits on every run.  Read: the D columns of the n rows - once per chunk of 32 columns of W, so once for K <= 32 and ceil(K / 32)
 * times otherwise -, labels, mean, inv_std, W (V).  Written: the named outputs and the
 * workspace (bvc_op_linear_pass_workspace(n, D, K, mode) bytes, -1 for invalid sizes; no [n][D] array exists in it).
 * BVC_ERR_INVALID and nothing launched for a non-positive size, D above 1343, K above 1024 (more classes: a host loop over class
 * chunks), an unknown mode, a null pointer among those the mode uses, a pointer that is not 4-byte aligned, or a stride below D. */
int bvc_op_colstats(const float* x, int64_t ldx, int n, int D, float* mean, float* inv_std, void* stream);
int64_t bvc_op_linear_pass_workspace(int n, int D, int K, int mode);
int bvc_op_linear_pass_splits(int n, int D, int K);
int bvc_op_linear_pass_tile_rows(int D);
int bvc_op_linear_pass(const float* x, int64_t ldx, const int* labels, const float* mean, const float* inv_std, const float* W,
                       const float* V, int n, int D, int K, int class0, int mode, float C, float* out_G, float* out_loss, int* out_pred,
                       float* out_dec, void* workspace, void* stream);
/* Attentive pooling (csrc/attnpool.hip): the part of an attentive probe's cross-attention block that touches the tokens.  For each
 * of the B clips, R <= 16 query rows u f32 [R][D] softmax-pool the STANDARDISED token rows of x f32 [B][N] rows of D columns (row
 * stride ldx elements):  xh_j = (x_j - mean_j) / sqrt(var_j + eps) (biased variance, as nn.LayerNorm without its affine),
 * s_jr = xh_j . u_r,  p_jr = softmax over the N tokens,  pooled f32 [B][R][D] = sum_j p_jr xh_j,  lse f32 [B][R] = log sum_j
 * exp(s_jr) (natural log).  LayerNorm's weight and bias, the K / V projections and the query fold into u and into [B][D] algebra
 * (bvc/attentive.py); no K or V array exists.  All arithmetic is f32 (v_mfma_f32_16x16x4_f32 products).
 *   splits      0 = chosen by the library from the shape (bvc_op_attn_pool_splits), else the tokens of every clip are cut into that
 *               many contiguous ranges [s N / splits, (s + 1) N / splits) (up to 256; empty ranges are legal) run by workgroups of
 *               their own and merged in ascending order.  Different split counts agree to rounding, not bit for bit.
 *   workspace   bvc_op_attn_pool_workspace(B, N, D, R, splits) bytes, 16-byte aligned (-1 for a refused shape); serves the forward
 *               and the backward of that shape; its contents on entry do not matter.
 * Backward, for dpooled f32 [B][R][D] (pooled and lse as the forward wrote them): du f32 [R][D] = the gradient of u summed over
 * the clips (written, not accumulated), and, unless dx is NULL, dx f32 [B][N] rows of D columns (row stride lddx) = the gradient
 * of x through the scores, the pooled rows and the standardisation.  With dx NULL nothing of it is computed or stored.
 * Read: the D columns of the rows (never the ldx - D padding).  Written: the named outputs and the workspace, nothing else.  No
 * atomics and no host synchronisation or allocation: the same bits on every run, a clip's pooled / lse / dx do not depend on the
 * other clips, and the calls may be captured in a graph.  BVC_ERR_INVALID (bvc_last_error) and nothing launched unless
 * B, N >= 1, D % 64 == 0 with 64 <= D <= 2048, 1 <= R <= 16, 0 <= splits <= 256, ldx (lddx) >= D and a multiple of 4, and
 * x, u, dpooled, dx and the workspace 16-byte aligned. */
int bvc_op_attn_pool_splits(int B, int N, int D, int R);
int64_t bvc_op_attn_pool_workspace(int B, int N, int D, int R, int splits);
int bvc_op_attn_pool_fwd(const float* x, int64_t ldx, const float* u, int B, int N, int D, int R, float eps, int splits, float* pooled,
                         float* lse, void* workspace, void* stream);
int bvc_op_attn_pool_bwd(const float* x, int64_t ldx, const float* u, const float* pooled, const float* lse, const float* dpooled, int B,
                         int N, int D, int R, float eps, int splits, float* du, float* dx, int64_t lddx, void* workspace, void* stream);
/* NT-Xent / SupCon loss (csrc/ntxent.hip) over n feature rows f f32 [n] rows of p columns (row stride ldf elements) with one
 * integer group id per row: groups int32 [n], or NULL for g_i = i mod (n / views), the view-major layout of `views` views.  A
 * negative id belongs to no group.  With zn_i = f_i / max(|f_i|, eps), s_ij = zn_i . zn_j / temperature,
 * P(i) = { j != i : g_j == g_i >= 0 } and c_i = |P(i)|:
 *   lse f32 [n]       D_i = log sum_{k != i} exp(s_ik) over ALL other rows (natural log; -inf for n = 1)
 *   npos int32 [n]    c_i
 *   row_loss f32 [n]  l_i = D_i - (1 / c_i) sum_{j in P(i)} s_ij, 0 where c_i = 0
 *   stats2 f32 [2]    { sum_i l_i / max(1, m), m = #{ i : c_i > 0 } }
 * Two views per sample give SimCLR's NT-Xent, label ids the supervised contrastive loss L_out.  Rows are excluded by index, never
 * by value.  Backward, for per-row upstream weights row_weight f32 [n] (ignored where c_i = 0; for the mean: gout / max(1, m)):
 * df f32 [n] rows of p columns (row stride lddf) = sum_i row_weight_i d l_i / d f, through the normalisation (where |f_i| <= eps
 * the clamp is active and zn_i = f_i / eps).  lse and npos as the forward wrote them; nothing else survives from the forward.
 * All arithmetic is f32 (v_mfma_f32_32x32x2_f32 products); no [n][n] array is stored by the forward, the backward holds a block of
 * block_rows x n f32 in the workspace.
 *   key_splits  0 = chosen by the library (bvc_op_ntxent_splits), else the key tiles (128 rows) of every query tile are cut into that
 *               many contiguous ranges (up to 256; empty ranges are legal), merged in ascending order.  Different split counts agree
 *               to rounding, not bit for bit.
 *   block_rows  0 = chosen by the library (bvc_op_ntxent_block_rows: the most whole 128-row tiles whose block stays under 256 MiB),
 *               else rounded up to a multiple of 128.
 *   workspace   bvc_op_ntxent_workspace(n, p, key_splits, block_rows) bytes, 16-byte aligned (-1 for a refused shape); serves the
 *               forward and the backward; its contents on entry do not matter.
 * Read: the p columns of the rows (never the ldf - p padding).  Written: the named outputs and the workspace, nothing else.  No
 * atomics and no host synchronisation or allocation: the same bits on every run, and the calls may be captured in a graph.
 * BVC_ERR_INVALID (bvc_last_error) and nothing launched unless 1 <= n <= 32768, 1 <= p <= 8192, temperature and eps positive and
 * finite, ldf (lddf) >= p, 0 <= key_splits <= 256, block_rows >= 0, and, with groups NULL, views >= 1 dividing n. */
int bvc_op_ntxent_splits(int n, int p);
int bvc_op_ntxent_block_rows(int n, int p);
int64_t bvc_op_ntxent_workspace(int n, int p, int key_splits, int block_rows);
int bvc_op_ntxent_fwd(const float* f, int64_t ldf, const int32_t* groups, int views, int n, int p, float temperature, float eps,
                      int key_splits, float* row_loss, float* lse, int32_t* npos, float* stats2, void* workspace, void* stream);
int bvc_op_ntxent_bwd(const float* f, int64_t ldf, const int32_t* groups, int views, int n, int p, float temperature, float eps,
                      const float* lse, const int32_t* npos, const float* row_weight, int key_splits, int block_rows, float* df,
                      int64_t lddf, void* workspace, void* stream);
/* Prototype cross-entropy (csrc/proto_ce.hip): the loss of DINO and of the [CLS] half of iBOT / DINOv2 for ONE (teacher view,
 * student view) pair.  xs, xt f32 [m] rows of p columns (row strides ldxs, ldxt): row i of xt is the teacher row paired with row i
 * of xs.  vs, vt f32 [K] rows of p columns (row strides ldvs, ldvt): the student's and the teacher's prototype weights, the
 * weight-normalised last layer of a DINO head with gain 1.  center f32 [K] or NULL (= 0): any per-prototype shift.  With
 * xsn_i = xs_i / max(|xs_i|, eps), wsn_k = vs_k / |vs_k| (xtn, wtn likewise), s_ik = xsn_i . wsn_k / tau_s and
 * t_ik = (xtn_i . wtn_k - center_k) / tau_t:
 *   lse_s f32 [m]         Ls_i = log sum_k exp(s_ik)
 *   lse_t f32 [m]         Lt_i = log sum_k exp(t_ik)
 *   row_loss f32 [m]      l_i = Ls_i - sum_k q_ik s_ik,  q_ik = exp(t_ik - Lt_i)   (= sum_k -q_ik log_softmax(s_i)_k)
 *   stats2 f32 [2]        { sum_i l_i / m,  the number of zero rows of vs plus the number of zero rows of vt }
 *   batch_center f32 [K]  (1 / m) sum_i xtn_i . wtn_k, the raw teacher scores before centre and temperature; may be NULL
 * A prototype row of norm 0 has no direction: it is given wsn_k = 0 (wtn_k = 0), so it scores 0, takes part in the softmax with
 * that score and receives dvs_k = 0; stats2[1] counts such rows on the device, so that a caller can look at it when it next
 * synchronises anyway.  Only an exact 0 counts: a row holding NaN gives NaN scores, and the loss shows it.
 * Backward, for per-row weights row_weight f32 [m] (the mean: gout / m); the teacher side and center get no gradient: dS_ik = w_i (exp(s_ik - Ls_i) - q_ik) / tau_s, dxsn = dS wsn, dwsn = dS^T xsn,
 * dxs_i = (dxsn_i - xsn_i (xsn_i . dxsn_i)) / max(|xs_i|, eps) (dxsn_i / eps where the clamp is active),
 * dvs_k = (dwsn_k - wsn_k (wsn_k . dwsn_k)) / |vs_k|.  dxs f32 [m] rows (stride lddxs), dvs f32 [K] rows (stride lddvs).  lse_s and
 * lse_t as the forward wrote them; nothing else survives from the forward.
 * All arithmetic is f32 (v_mfma_f32_32x32x2_f32 products, every score one accumulation chain over the p columns); the forward stores
 * no array of m x K elements, the backward holds two blocks of m x block f32 in the workspace.
 *   splits     0 = chosen by the library (bvc_op_proto_ce_splits: about two workgroups per CU, at most one per 128-prototype tile, at
 *              most 512), else the prototype tiles of every 128-row tile are cut into that many contiguous ranges (up to 2048; empty
 *              ranges are legal), merged in ascending order.  Different split counts agree to rounding, not bit for bit.
 *   block      0 = chosen by the library (bvc_op_proto_ce_block: the most whole 128-prototype tiles whose dS block [m up to 128][block]
 *              f32 stays under 64 MiB), else rounded up to a multiple of 128.  dvs has the same bits for every block (the
 *              contraction over the rows is complete within a block); dxs is summed block after block and agrees to rounding.
 *   workspace  bvc_op_proto_ce_workspace(m, K, p, splits, block) bytes, 16-byte aligned (-1 for a refused shape); serves the forward
 *              and the backward; its contents on entry do not matter.  The forward touches only the leading part (the vectors, the
 *              split partials and the four normalised operands), whose size does not depend on block: a caller of the forward alone
 *              may pass bvc_op_proto_ce_workspace(m, K, p, splits, 128) bytes, the smallest block (137 MiB instead of 327 MiB at
 *              m = 1024, K = 65536, p = 256).  It holds the normalised operands (2 m p + 2 K p floats, m
 *              and K rounded up to 128, p to 32), in the backward also the transposes and gradients of a block, 2 m block floats
 *              of dS and the partial products of dxsn (up to 32 MiB).  m = 1024, K = 65536, p = 256: 327 MiB.  The largest shape (m = 32768, K = 262144, p = 8192): 21.2 GiB.
 * Read: the p columns of the rows (never the stride padding).  Written: the named outputs and the workspace, nothing else.  No
 * atomics and no host synchronisation or allocation: the same bits on every run, and the calls may be captured in a graph.
 * BVC_ERR_INVALID (bvc_last_error) and nothing launched unless 1 <= m <= 32768, 1 <= K <= 262144, 1 <= p <= 8192, tau_s, tau_t and
 * eps positive and finite, every stride at least p, 0 <= splits <= 2048, block >= 0 and no required pointer null. */
int bvc_op_proto_ce_splits(int m, int K, int p);
int bvc_op_proto_ce_block(int m, int K, int p);
int64_t bvc_op_proto_ce_workspace(int m, int K, int p, int splits, int block);
int bvc_op_proto_ce_fwd(const float* xs, int64_t ldxs, const float* vs, int64_t ldvs, const float* xt, int64_t ldxt, const float* vt,
                        int64_t ldvt, const float* center, int m, int K, int p, float tau_s, float tau_t, float eps, int splits,
                        float* row_loss, float* lse_s, float* lse_t, float* stats2, float* batch_center, void* workspace, void* stream);
int bvc_op_proto_ce_bwd(const float* xs, int64_t ldxs, const float* vs, int64_t ldvs, const float* xt, int64_t ldxt, const float* vt,
                        int64_t ldvt, const float* center, int m, int K, int p, float tau_s, float tau_t, float eps, const float* lse_s,
                        const float* lse_t, const float* row_weight, int splits, int block, float* dxs, int64_t lddxs, float* dvs,
                        int64_t lddvs, void* workspace, void* stream);
/* Feature cross-correlation with a reduced epilogue (csrc/xcorr.hip): Barlow Twins, VICReg's covariance term and linear CKA.
 * x f32 [n] rows of p columns (row stride ldx elements), y f32 [n] rows of q columns (row stride ldy); y may be the SAME POINTER as
 * x with q == p and ldy == ldx, the auto-covariance ("alias") case.  Per column j of x (likewise of y):
 *   mu_j = mean_i x_ij,  var_j = sum_i (x_ij - mu_j)^2 / (n - ddof),  r_j = 1 (norm 0: centre only) or 1 / sqrt(var_j + eps)
 *   (norm 1: standardise),  xh_ij = (x_ij - mu_j) r_j.  A constant column is no special case: var 0, xh 0, r = 1 / sqrt(eps).
 * With C = scale xh^T yh [p][q], which is never stored by the forward, and t = diag_target:
 *   mean_x, var_x f32 [p]; mean_y, var_y f32 [q] (not written, and may be NULL, in the alias case)
 *   stats2 f32 [2]   { on = sum_i (C_ii - t)^2 over i < min(p, q),  off = sum_{i != j} C_ij^2 }
 * Barlow Twins: norm 1, ddof 0, eps 1e-5, scale 1 / n, t 1.  VICReg covariance: alias, norm 0, ddof 1, scale 1 / (n - 1), w_on 0.
 * Linear CKA: norm 0, scale 1, t 0, so that on + off = |xc^T yc|_F^2.
 * Backward, for w f32 [2] ON THE DEVICE = { d / d on, d / d off } and the optional upstream gradients dvar_x f32 [p], dvar_y f32 [q]
 * of the returned variances (NULL = zero): G_ii = 2 w_on (C_ii - t), G_ij = 2 w_off C_ij, dxh = scale yh G^T, dyh = scale xh G
 * (alias: dxh = scale xh (G + G^T)), a_j = dvar_j - (norm ? r_j^2 / 2 sum_i dxh_ij xh_ij : 0),
 * dx_ij = r_j (dxh_ij - mean_i' dxh_i'j) + 2 (x_ij - mu_j) a_j / (n - ddof).  dx f32 [n] rows of p columns (row stride lddx), dy f32
 * [n] rows of q columns (row stride lddy; NULL in the alias case, where dx is the whole gradient).  mean_* and var_* as the forward
 * wrote them; nothing else survives from the forward.
 * All arithmetic is f32 (v_mfma_f32_32x32x2_f32 products); every element of C is one accumulation chain over the rows in ascending
 * order.  The column statistics, the sums of the squares and the backward's column sums are f64 sums in a fixed order with one
 * rounding.  Diagonal membership and padding are decided by index, never by value.
 *   block_cols  0 = chosen by the library (bvc_op_xcorr_block_cols: the most whole 128-column tiles whose G block
 *               [block_cols][max(p, q) up to 32] f32 stays under 128 MiB), else rounded up to a multiple of 128.  The backward
 *               holds one such block of G, and dxh [n][block_cols] f32, in the workspace.  Every blocking gives the same bits.
 *               The cap covers G only: dxh is n x block_cols x 4 bytes (512 MiB at n = 32768 with 4096 columns); a smaller
 *               block_cols shrinks both.
 *   workspace   bvc_op_xcorr_workspace(n, p, q, alias, block_cols, backward) bytes, 16-byte aligned (-1 for a refused shape);
 *               backward = 0 sizes the forward (the transposed operands and one f64 pair per tile: no [p][q] array), backward = 1
 *               the backward of that blocking: the transposed and the row-major copies of both operands (4 x n x width x 4 bytes,
 *               half of that in the alias case), the G block and dxh.  The largest shape (n = 32768, p = q = 8192, distinct
 *               operands, automatic blocking) takes 4.6 GiB in the backward and 2.0 GiB in the forward.  Its contents on entry do
 *               not matter.
 * The explicit alias and y passed as a bit-equal copy give the same forward bits; their gradients (dx against dx + dy) agree to
 * rounding.  Read: the p (q) columns of the rows, never the stride padding.  Written: the named outputs and the workspace, nothing
 * else.  No atomics and no host synchronisation or allocation: the same bits on every run, and the calls may be captured in a graph.
 * BVC_ERR_INVALID (bvc_last_error) and nothing launched unless 1 <= n <= 32768, 1 <= p, q <= 8192, norm and ddof in {0, 1},
 * n - ddof >= 1, scale positive and finite, diag_target finite, eps positive and finite when norm == 1, every stride at least
 * the width, no required pointer null, x and y 4-byte and the workspace 16-byte aligned, block_cols >= 0, x == y only with q == p and ldy == ldx, and dy NULL in the alias case. */
int bvc_op_xcorr_block_cols(int n, int p, int q);
int64_t bvc_op_xcorr_workspace(int n, int p, int q, int alias, int block_cols, int backward);
int bvc_op_xcorr_fwd(const float* x, int64_t ldx, const float* y, int64_t ldy, int n, int p, int q, int norm, int ddof, float eps, float scale,
                     float diag_target, float* mean_x, float* var_x, float* mean_y, float* var_y, float* stats2, void* workspace, void* stream);
int bvc_op_xcorr_bwd(const float* x, int64_t ldx, const float* y, int64_t ldy, int n, int p, int q, int norm, int ddof, float eps, float scale,
                     float diag_target, const float* mean_x, const float* var_x, const float* mean_y, const float* var_y, const float* w,
                     const float* dvar_x, const float* dvar_y, int block_cols, float* dx, int64_t lddx, float* dy, int64_t lddy,
                     void* workspace, void* stream);
/* nn.LayerNorm forward/backward (HF:336-337,484); rows may be strided by (rin, rout, roff), rin<=0 = dense */
int bvc_op_layernorm_fwd(const float* x, int rin, int rout, int roff, const float* gamma, const float* beta, void* y_bf16,
                         float* mean, float* rstd, int M, int D, float eps, void* stream);
/* workspace: bvc_op_layernorm_bwd_workspace(M, D) floats of scratch */
int bvc_op_layernorm_bwd(const void* dy_bf16, const float* x, int rin, int rout, int roff, const float* mean,
                         const float* rstd, const float* gamma, float* dres, int accumulate, void* dres_bf16,
                         float* dgamma, float* dbeta, float* workspace, int M, int D, void* stream);
int64_t bvc_op_layernorm_bwd_workspace(int M, int D);
/* the same over dense rows with the bf16 copy alone gated: dres_bf16 = bf16(gate .* dres) for (layer, branch) of `drop` */
int bvc_op_layernorm_bwd_gate(const void* dy_bf16, const float* x, const float* mean, const float* rstd, const float* gamma, float* dres,
                              int accumulate, void* dres_bf16, float* dgamma, float* dbeta, float* workspace, int M, int D,
                              const bvc_branch_drop* drop, int layer, int branch, void* stream);
int bvc_op_colsum_bf16(const void* X, int M, int N, int ld, float alpha, const float* alpha_dev, float* out, void* stream);
/* out[n] += sum over rows m of X f32 [M][D] (rows strided by (rin, rout, roff) as for LayerNorm, rin <= 0 = dense): the mask-token
 * gradient of the VideoMAE decoder / JEPA predictor; D % 4 == 0 */
int bvc_op_colsum_f32(const float* X, int rin, int rout, int roff, int M, int D, float* out, void* stream);
int bvc_op_cast_bf16(const float* in, void* out, int64_t n, void* stream);
/* SimCLR loss pieces (info_nce_loss, pretraining/contrastive/pretrain_simclr.py:114-128, with its masks :284-292):
 * row_normalize = the two norms of F.cosine_similarity; the (2B x 2B) similarity is a GEMM of the normalised rows with
 * BVC_EPI_NCE (loss partials, nothing materialised) / BVC_EPI_NCE_BWD (bf16 d loss / d (cos/T)); nce_finalize folds
 * the partials: loss = logsumexp over ALL negative entries - mean over the tridiagonal positives; stats = {lse, -1/npos}. */
int bvc_op_row_normalize(const float* f, void* fn_bf16, float* inv_norm, int n, int p, float eps, void* stream);
int bvc_op_row_normalize_bwd(const float* f, const float* inv_norm, const float* dfn, float* df, int n, int p, void* stream);
int bvc_op_nce_finalize(const float* partial, int ntiles, float inv_temperature, int64_t npos, float* loss, float* stats, void* stream);
/* One-pass torch.optim.SGD(momentum, nesterov) update over a flat f32 range, replacing the optimiser step at
 * pretrain_videomae.py:187-189,313.  grad_scale / found_inf are GradScaler's device scalars (may be NULL):
 * gradients are divided by *grad_scale, and nothing is touched when *found_inf != 0.
 * bf16_shadow (may be NULL): the bf16 copy of `params` a model context keeps for its products (bvc_videomae_shadow / bvc_vit_shadow /
 * bvc_predictor_shadow, same offset as `params` inside the flat buffer): written with the updated parameters, so that the next
 * forward does not have to re-cast all of them. */
int bvc_op_sgd_step(float* params, float* grads, float* momentum_buf, int64_t n, float lr, float momentum, float dampening,
                    float weight_decay, int nesterov, int first_step, int maximize, const float* grad_scale,
                    const float* found_inf, int write_unscaled_grads, void* bf16_shadow, void* stream);
/* One-pass torch.optim.AdamW / Adam update over a flat f32 range (pretrain_videomae.py:190-193, pretrain_simclr.py:238-240).
 * state3 = device {step count, lr / (1 - beta1^step), sqrt(1 - beta2^step)}: bvc_op_adam_prepare advances it once per optimiser
 * step (not at all when *found_inf != 0), bvc_op_adam_step consumes it.  Hyper-parameters are doubles (python floats) and are
 * combined in double before the cast to f32, as torch does.  decoupled = 1: AdamW (p *= 1 - lr wd); 0: Adam (g += wd p). */
int bvc_op_adam_prepare(float* state3, double lr, double beta1, double beta2, const float* found_inf, void* stream);
int bvc_op_adam_step(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, double lr, double beta1, double beta2,
                     double eps, double weight_decay, int decoupled, int maximize, const float* state3, const float* grad_scale,
                     const float* found_inf, int write_unscaled_grads, void* bf16_shadow, void* stream);
/* The same updates for an optimiser with PARAMETER GROUPS over one flat buffer, as ONE launch (the reference's JEPA optimiser,
 * pretraining/predictive/helper.py:123-147: four groups - encoder / predictor weights with weight decay, their biases and 1-D
 * tensors with weight_decay 0 - over a layout that interleaves weights and biases).  The flat range [0, n) is cut into `nseg`
 * segments: seg_start (device int64 [nseg + 1], ascending element offsets, seg_start[0] = 0, seg_start[nseg] = n), seg_group
 * (device int32 [nseg]: the owning group, or -1 for elements no group owns - frozen parameters: left untouched), blk_seg (device
 * int32 [ceil(n / 1024)]: the segment holding element 1024 b).  The groups' hyper-parameters are host values passed per call
 * (schedules change them every step; the table is static).  Same arithmetic as bvc_op_sgd_step / bvc_op_adam_step per element. */
#define BVC_OPT_MAX_GROUPS 8
typedef struct bvc_sgd_groups {
    int ngroups;
    float lr[BVC_OPT_MAX_GROUPS], momentum[BVC_OPT_MAX_GROUPS], dampening[BVC_OPT_MAX_GROUPS], weight_decay[BVC_OPT_MAX_GROUPS];
    int nesterov[BVC_OPT_MAX_GROUPS], first_step[BVC_OPT_MAX_GROUPS], maximize[BVC_OPT_MAX_GROUPS];
} bvc_sgd_groups;
typedef struct bvc_adam_groups {
    int ngroups;
    double lr[BVC_OPT_MAX_GROUPS], beta1[BVC_OPT_MAX_GROUPS], beta2[BVC_OPT_MAX_GROUPS], eps[BVC_OPT_MAX_GROUPS], weight_decay[BVC_OPT_MAX_GROUPS];
    int decoupled[BVC_OPT_MAX_GROUPS], maximize[BVC_OPT_MAX_GROUPS];
} bvc_adam_groups;
int bvc_op_sgd_step_segments(float* params, float* grads, float* momentum_buf, int64_t n, const int64_t* seg_start, const int32_t* seg_group,
                             const int32_t* blk_seg, int nseg, const bvc_sgd_groups* groups, const float* grad_scale, const float* found_inf,
                             int write_unscaled_grads, void* bf16_shadow, void* stream);
/* state = device f32 [3 ngroups] ({step count, lr / (1 - beta1^step), sqrt(1 - beta2^step)} per group, advanced inside the call
 * unless *found_inf != 0); hyper_scratch = device f64 [3 ngroups] the call uploads lr / beta1 / beta2 into */
int bvc_op_adam_step_segments(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, const int64_t* seg_start,
                              const int32_t* seg_group, const int32_t* blk_seg, int nseg, const bvc_adam_groups* groups, float* state,
                              double* hyper_scratch, const float* grad_scale, const float* found_inf, int write_unscaled_grads,
                              void* bf16_shadow, void* stream);
/* The segment updates for MORE parameter groups than a by-value struct carries (layer-wise learning-rate decay: 2 (layers + 2)
 * groups, 28 / 52 / 68 at base / large / huge).  Same segment table, same arithmetic per element; the hyper-parameters are plain host
 * arrays of `ngroups` entries (1..BVC_OPT_TABLE_MAX_GROUPS), read before the call returns.  Inside the call they are stored into
 * group_table (device f32 [8 ngroups], 16-byte aligned, owned by the caller, contents need not survive between calls) by small
 * kernels that take BVC_OPT_TABLE_CHUNK groups per launch as kernel arguments - no host synchronisation, no copy out of host memory
 * that has to outlive the call - and the update kernel reads row seg_group[s] of it.  A segment whose group is outside [0, ngroups) is
 * left untouched.  state = device f32 [3 ngroups] as for bvc_op_adam_step_segments. */
#define BVC_OPT_TABLE_MAX_GROUPS 1024
#define BVC_OPT_TABLE_CHUNK 64
int bvc_op_sgd_step_table(float* params, float* grads, float* momentum_buf, int64_t n, const int64_t* seg_start, const int32_t* seg_group,
                          const int32_t* blk_seg, int nseg, int ngroups, const float* lr, const float* momentum, const float* dampening,
                          const float* weight_decay, const int32_t* nesterov, const int32_t* first_step, const int32_t* maximize,
                          float* group_table, const float* grad_scale, const float* found_inf, int write_unscaled_grads,
                          void* bf16_shadow, void* stream);
int bvc_op_adam_step_table(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, const int64_t* seg_start,
                           const int32_t* seg_group, const int32_t* blk_seg, int nseg, int ngroups, const double* lr, const double* beta1,
                           const double* beta2, const double* eps, const double* weight_decay, const int32_t* decoupled,
                           const int32_t* maximize, float* state, float* group_table, const float* grad_scale, const float* found_inf,
                           int write_unscaled_grads, void* bf16_shadow, void* stream);
/* GradScaler's inf check (scaler.step at pretrain_videomae.py:313 -> torch.amp.GradScaler._check_inf_per_device) as one read-only
 * pass over a flat f32 range: *found_inf (device f32) is set to 1 if any element is Inf or NaN; it is never cleared here. */
int bvc_op_nonfinite_check(const float* x, int64_t n, float* found_inf, void* stream);
/* Gradient-norm clipping (torch.nn.utils.clip_grad_norm_) without a pass of its own over the gradients.
 *
 * The squared norm of the OWNED segments of a flat f32 range - the segment table of the optimiser entry points above: seg_start
 * [nseg + 1], seg_group [nseg], -1 = owned by nobody - comes out of one read, and GradScaler's inf check rides on the same read.  A
 * plain contiguous range is a table of one segment.
 *
 * bvc_grad_norm_items_host (host, no GPU): the static work list of a table.  Every element of every owned segment lies in exactly one
 * item (start, length, segment); no item crosses a segment boundary or is longer than bvc_op_grad_norm_item_cap() elements; unowned
 * segments get none; the items of a segment are adjacent and ascending, seg_first_item [nseg + 1] (may be NULL) indexes them.
 * items == NULL: only *nitems (and seg_first_item) are written, so a caller can size its array.
 *
 * bvc_op_grad_sqnorm_items: one launch pair.  The first launch takes one workgroup per item and writes the item's sum of squares to
 * item_partial [nitems] (device f64): 16-byte loads from the first 16-byte boundary inside the item on, scalar loads for the up to
 * three elements before it and after the last whole vector, so `x` needs 4-byte alignment only and segments may start anywhere.
 * found_inf (device f32, may be NULL) is set to 1 if an element INSIDE AN ITEM is Inf or NaN (the test of bvc_op_nonfinite_check);
 * it is never cleared.  The second launch adds the partials in a fixed order into seg_sq [nseg] (may be NULL; 0 for an unowned
 * segment) and total_sq [1]; with as_norm != 0 both receive the square roots.  No atomics: the same bits on every run.
 * Accuracy: a thread adds at most bvc_op_grad_norm_chain() squares serially in f32 (fused multiply-add); everything above that is
 * added in f64 and rounded to f32 once.
 *
 * bvc_op_clip_finalize: out3 = {total_norm, clip_coef, eff_scale} from sq [nranges] (one entry per flat buffer or loose run of an
 * optimiser), in one tiny launch: total_norm = sqrt(sum sq) / scale, clip_coef = min(1, max_norm / (total_norm + 1e-6)),
 * eff_scale = scale / clip_coef, scale = *grad_scale or 1 when grad_scale is NULL.  Passing &out3[2] where a step entry point takes
 * grad_scale makes that step unscale AND clip; no optimiser kernel knows about clipping.
 *
 * bvc_op_scale_by_dev: x[i] *= *coef (device scalar) for the immediate form; nothing is written when *coef == 1. */
#define BVC_GRAD_NORM_ITEM_CAP 16384
typedef struct bvc_norm_item {
    int64_t start;      /* first element, relative to the range */
    int32_t length;     /* 1 .. BVC_GRAD_NORM_ITEM_CAP */
    int32_t segment;
} bvc_norm_item;
int bvc_op_grad_norm_item_cap(void);
int bvc_op_grad_norm_chain(void);
int bvc_grad_norm_items_host(const int64_t* seg_start, const int32_t* seg_group, int nseg, bvc_norm_item* items, int64_t items_cap,
                             int64_t* seg_first_item, int64_t* nitems);
int bvc_op_grad_sqnorm_items(const float* x, const bvc_norm_item* items, int64_t nitems, const int64_t* seg_first_item, int nseg,
                             double* item_partial, float* seg_sq, float* total_sq, int as_norm, float* found_inf, void* stream);
int bvc_op_clip_finalize(const float* sq, int nranges, float max_norm, const float* grad_scale, float* out3, void* stream);
int bvc_op_scale_by_dev(float* x, int64_t n, const float* coef, void* stream);
/* Layer-wise trust ratios: LARS (the form of SimCLR's and MAE's LARS) and LAMB (You et al. 2020, with bias correction) over a flat f32
 * range, one trust ratio per SEGMENT of the segment table above (one segment per parameter tensor; a plain contiguous tensor is a
 * table of one segment).  Per tensor w with gradient g (g already divided by *grad_scale and negated under maximize):
 *   LARS:  d = g + weight_decay w;  q = trust_coefficient ||w|| / ||d|| if adapt and ||w|| > 0 and ||d|| > 0, else 1;  d = q d;
 *          buf = momentum buf + d;  w -= lr (nesterov ? d + momentum buf : buf)
 *   LAMB:  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g g;  u = (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + eps) + weight_decay w;
 *          r = ||w|| / ||u|| if adapt and ||w|| > 0 and ||u|| > 0, else 1;  w -= lr r u
 * These two entry points are the only path, for any number of groups (1..BVC_OPT_TABLE_MAX_GROUPS); the hyper-parameters are plain
 * host arrays of `ngroups` entries, read before the call returns.  Each call makes its whole launch sequence on `stream`, with no
 * host synchronisation, no allocation and no copy from host memory that has to outlive the call:
 *   1. one writer launch per BVC_OPT_TABLE_CHUNK groups: the groups' rows of group_table (as kernel arguments); for LAMB also the
 *      groups' step scalars in `state` (advanced unless *found_inf != 0),
 *   2. one workgroup per item of the work list (bvc_grad_norm_items_host of the same table): LARS reads w and g once and forms d,
 *      LAMB updates exp_avg / exp_avg_sq in place (and writes the unscaled g back) and forms u; either leaves the item's
 *      sum w^2 and sum d^2 (sum u^2) in item_partial as f64 (a thread adds at most bvc_op_grad_norm_chain() squares serially in f32),
 *   3. one workgroup per segment: the partials of the segment's items added in f64 in a fixed order -> seg_stats[s] =
 *      {||w||, ||d|| or ||u||, ratio}; a segment no group owns gets {0, 0, 1},
 *   4. one launch over the whole range in 1024-element blocks (blk_seg as above): LARS applies momentum and the step, LAMB recomputes
 *      u from the updated moments with the device function step 2 used - the applied update is the one whose norm was taken - and
 *      both write the parameters and, where given, their bf16 shadow.
 * No atomics: the same bits on every run.  Every launch returns at once when *found_inf != 0, so a step GradScaler skips writes
 * nothing: not the parameters, the state, the step counts, seg_stats or the shadow.  The LARS item pass also SETS *found_inf (where
 * found_inf is not NULL) when a gradient element inside an item is Inf or NaN, as bvc_op_grad_sqnorm_items does.
 * Caller-owned device buffers: group_table f32 [8 ngroups] (16-byte aligned; contents need not survive between calls), item_partial
 * f64 [2 max(nitems, 1)] (scratch), seg_stats f32 [3 nseg] (the last step's values; read it whenever the stream allows), momentum_buf
 * / exp_avg / exp_avg_sq f32 [n], state f32 [3 ngroups] = {step count, 1 / (1 - b1^step), 1 / sqrt(1 - b2^step)} per group.  params,
 * grads and the state arrays are 16-byte aligned.  momentum_buf may be NULL when every group's momentum is 0.  grad_scale, found_inf,
 * write_unscaled_grads and bf16_shadow mean what they mean for bvc_op_sgd_step_table / bvc_op_adam_step_table. */
int bvc_op_lars_step_table(float* params, float* grads, float* momentum_buf, int64_t n, const int64_t* seg_start, const int32_t* seg_group,
                           const int32_t* blk_seg, int nseg, const bvc_norm_item* items, int64_t nitems, const int64_t* seg_first_item,
                           int ngroups, const float* lr, const float* momentum, const float* weight_decay, const float* trust_coefficient,
                           const int32_t* nesterov, const int32_t* adapt, const int32_t* maximize, float* group_table, double* item_partial,
                           float* seg_stats, const float* grad_scale, float* found_inf, int write_unscaled_grads, void* bf16_shadow,
                           void* stream);
int bvc_op_lamb_step_table(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, const int64_t* seg_start,
                           const int32_t* seg_group, const int32_t* blk_seg, int nseg, const bvc_norm_item* items, int64_t nitems,
                           const int64_t* seg_first_item, int ngroups, const double* lr, const double* beta1, const double* beta2,
                           const double* eps, const double* weight_decay, const int32_t* adapt, const int32_t* maximize, float* state,
                           float* group_table, double* item_partial, float* seg_stats, const float* grad_scale, const float* found_inf,
                           int write_unscaled_grads, void* bf16_shadow, void* stream);
/* boolean mask -> ascending visible / masked token lists (the order x[~mask] / x[mask] produce, HF:121,578-579) */
int bvc_op_mask_index(const uint8_t* mask, int B, int L, int nvis, int nmask, int* vis_idx, int* msk_idx, int* status, void* stream);
/* the same with a decode mask: the visible list and the ascending list of the ndec decoded tokens per clip; *status |= 1 when a clip's
 * visible count is not nvis, its decoded count is not ndec, or a decoded token is not masked (vis_idx [B][nvis], dec_idx [B][ndec]) */
int bvc_op_dual_mask_index(const uint8_t* mask, const uint8_t* decode_mask, int B, int L, int nvis, int ndec, int* vis_idx, int* dec_idx,
                           int* status, void* stream);
/* 1 when a VideoMAE pre-training forward of `clips` clips runs its first decoder layer by position under the options in force ("dec_first";
 * unpadded heads and no gate assumed), 0 otherwise */
int bvc_op_dec_first_selected(int clips, int decoder_layers);
/* dec_slot [B][L]: the slot j of position p among clip b's decoded tokens (dec_idx[b][j] == p), -1 where clip b does not decode p */
int bvc_op_dec_slot(const int* dec_idx, int* dec_slot, int B, int L, int ndec, void* stream);
/* S[p][c] = sum over clips b = 0 .. B-1, in that order, of dqkv[b][nvis + dec_slot[b][p]][c] (bf16 [B][Ld][W] in, f32 sums; a slot of -1
 * adds nothing; W a multiple of 8).  S (f32 [L][W]) and / or the bf16 pair hi = bf16(S), lo = bf16(S - hi) ([L][W] each; both or
 * neither).  No atomics: two runs give the same bits. */
int bvc_op_first_reduce(const void* dqkv_bf16, const int* dec_slot, int B, int L, int Ld, int nvis, int W, float* S, void* hi_bf16,
                        void* lo_bf16, void* stream);
/* tube patches of the visible tokens in Conv3d weight order (HF:157-177) */
int bvc_op_gather_patches(const float* clip, const int* vis_idx, void* A_bf16, int B, int nvis, int T, int C, int H, int W,
                          int ts, int ps, void* stream);
/* the same through a bvc_clip_mix table of B entries (device), from either pixel format (fmt NULL = f32); idx [B][n] tokens per clip.
 * Out-of-range entries are clamped (no status word at this level). */
int bvc_op_gather_patches_mix(const void* clip, const bvc_pixel_format* fmt, const int* idx, void* A_bf16, const bvc_clip_mix* mix,
                              int B, int n, int T, int C, int H, int W, int ts, int ps, void* stream);
/* the same through a bvc_erase_box table of [B][boxes] entries as well (erase each clip, then mix the batch); mix NULL = no mix, boxes
 * in [1, BVC_ERASE_MAX_BOXES], C <= 4.  Out-of-range entries are clamped (no status word at this level). */
int bvc_op_gather_patches_aug(const void* clip, const bvc_pixel_format* fmt, const int* idx, void* A_bf16, const bvc_clip_mix* mix,
                              const bvc_erase_box* erase, int boxes, uint64_t seed, uint64_t offset, int B, int n, int T, int C, int H,
                              int W, int ts, int ps, void* stream);
/* per-patch-normalised pixel targets of the masked tokens (HF:588-661) */
int bvc_op_pixel_labels(const float* clip, const int* msk_idx, float* labels, int B, int nmask, int T, int C, int H, int W,
                        int ts, int ps, int norm_pix, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Communication: one RCCL rank per process (one process per GPU), the communication stream and its event fences owned by the
 * library.  Replaces, for this path, what the reference reaches through torch.distributed:
 *   dist.init_process_group("nccl", rank=rank, world_size=world)      pretraining/generative/pretrain_videomae.py:87-90
 *   DistributedDataParallel's gradient reducer                         pretrain_videomae.py:180-181,312 (bucketed all-reduce, mean)
 *   AllReduce / AllGather autograd nodes                               pretraining/generative/ddputils.py:53-68,
 *                                                                      pretraining/predictive/distributed.py:49-76
 * RCCL is bound at run time (the librccl.so already mapped into the process when there is one - torch ships its own - else the
 * loader's), so the library links without it and loads on a machine without a GPU.
 * Rendezvous: rank 0 calls bvc_comm_unique_id and hands the 128 bytes to the other ranks by any side channel (the Python shim
 * broadcasts them over the process group the entry script has already initialised); every rank then calls bvc_comm_init with
 * its HIP device current.  All calls on one communicator come from the host thread that drives the step. */
#define BVC_COMM_ID_BYTES 128
typedef struct bvc_comm bvc_comm;
int bvc_comm_unique_id(void* id_out_host /* BVC_COMM_ID_BYTES */);
int bvc_comm_init(int rank, int world, const void* id_host, bvc_comm** out);
int bvc_comm_destroy(bvc_comm* comm);
/* the communication stream (hipStream_t), e.g. to record timing events around a bucket; owned by the communicator */
void* bvc_comm_stream(const bvc_comm* comm);
int bvc_comm_rank(const bvc_comm* comm);
int bvc_comm_world(const bvc_comm* comm);
/* path and version of the RCCL library in use (thread-local string; loads the library on first use) */
const char* bvc_comm_library(void);
/* One gradient bucket: in-place sum (average != 0: mean) over ranks of count f32 at buf, enqueued on the communication stream
 * behind an event recorded on producer_stream (the stream whose kernels wrote buf).  Returns immediately: this is the call a
 * bvc_bucket_fn makes while the rest of backward is still being enqueued. */
int bvc_allreduce_bucket(bvc_comm* comm, float* buf_dev, int64_t count, int average, void* producer_stream);
/* `stream` waits (event, no host block) for every bucket enqueued so far: end of backward, before the optimiser reads the gradients */
int bvc_comm_wait(bvc_comm* comm, void* stream);
/* Collectives whose result the caller's next kernels consume.  They too run on the communication stream (one communicator, one
 * stream, program order), fenced both ways: after everything enqueued on `stream` so far, and `stream` continues after them.
 *   allgather  recv[r * bytes_per_rank ...] = rank r's send buffer           (SimCLR global-batch negatives, forward)
 *   allreduce  in-place sum / mean of count f32                              (its backward; the loss scalar of AllReduce, ddputils.py:53-68)
 *   broadcast  root's buffer to every rank                                   (module-state sync at wrap time) */
int bvc_allgather(bvc_comm* comm, const void* send_dev, void* recv_dev, int64_t bytes_per_rank, void* stream);
int bvc_allreduce(bvc_comm* comm, float* buf_dev, int64_t count, int average, void* stream);
int bvc_broadcast(bvc_comm* comm, void* buf_dev, int64_t bytes, int root, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* BVC_H */

// VideoMAE on gfx950: the pre-training, inference and fine-tuning contexts, their workspaces and forward / backward schedules.
// Host code only - every kernel lives in gemm.hip / attention.hip / rowops.hip, the layer schedule in stack.hip, what the contexts
// share around it in context.hip, and the entry points that belong to no model in ops.hip.
//
// Follows VideoMAEForPreTraining.forward (HF:531-671; instantiated by the reference at
// pretraining/generative/pretrain_videomae.py:61-64) with these MI355X-first changes:
//   * the tube patch embedding is a gather-GEMM over the VISIBLE tokens only (the reference convolves
//     all 1568 tokens and throws 90 % away, HF:119-122);
//   * sinusoid tables are built once and stay in HBM (the reference re-uploads them every step, HF:114-116,575-576);
//   * mask -> token lists are built on the device, no nonzero()/host sync;
//   * MSE and d(logits) are fused into the head GEMM's epilogue; the loss is reduced in a fixed order;
//   * parameters / gradients are one flat buffer each; weight gradients of a layer are one grouped GEMM.
// Numerics: bf16 MFMA operands, f32 accumulation, f32 residual stream, f32 LayerNorm / softmax / loss
// statistics, f32 master weights and gradients.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "context.h"

using namespace bvc;

// ------------------------------------------------------------------ flat parameter layout
namespace {

struct Layout : ParamTable {
    int64_t pe_w = 0, pe_b = 0, e2d_w = 0, mask_token = 0, norm_w = 0, norm_b = 0, head_w = 0, head_b = 0;
    std::vector<LayerOff> enc, dec;
};

int check_config(const bvc_videomae_config& c) {
    BVC_REQUIRE(c.image_size > 0 && c.patch_size > 0 && c.image_size % c.patch_size == 0, "config: image_size %% patch_size != 0");
    BVC_REQUIRE(c.num_frames > 0 && c.tubelet_size > 0 && c.num_frames % c.tubelet_size == 0, "config: num_frames %% tubelet_size != 0");
    BVC_REQUIRE(c.patch_size % 8 == 0, "config: patch_size must be a multiple of 8");
    // the widths check_vit (jepa.hip) accepts: heads of any multiple of 8 up to 128 dims (attention.hip runs 32 / 64 / 80 / 88 / 96 /
    // 128 as they are, other widths zero-padded: stack.h attn_width), rows up to 1536 wide (rowops.hip: the 6-chunk LayerNorm)
    BVC_REQUIRE(c.num_attention_heads > 0 && c.hidden_size % c.num_attention_heads == 0, "config: encoder head_dim undefined (hidden_size %d %% num_attention_heads %d != 0)",
                c.hidden_size, c.num_attention_heads);
    BVC_REQUIRE(c.decoder_num_attention_heads > 0 && c.decoder_hidden_size % c.decoder_num_attention_heads == 0,
                "config: decoder head_dim undefined (decoder_hidden_size %d %% decoder_num_attention_heads %d != 0)", c.decoder_hidden_size, c.decoder_num_attention_heads);
    const int hd = c.hidden_size / c.num_attention_heads, hdd = c.decoder_hidden_size / c.decoder_num_attention_heads;
    BVC_REQUIRE(hd % 8 == 0 && hd <= 128, "config: encoder head_dim %d unsupported (multiples of 8 up to 128)", hd);
    BVC_REQUIRE(hdd % 8 == 0 && hdd <= 128, "config: decoder head_dim %d unsupported (multiples of 8 up to 128)", hdd);
    BVC_REQUIRE(c.hidden_size % 64 == 0 && c.decoder_hidden_size % 64 == 0, "config: hidden sizes must be multiples of 64");
    BVC_REQUIRE(c.hidden_size <= 1536 && c.decoder_hidden_size <= 1536, "config: hidden sizes above 1536 unsupported (hidden %d, decoder %d)",
                c.hidden_size, c.decoder_hidden_size);
    BVC_REQUIRE(c.intermediate_size % 64 == 0 && c.decoder_intermediate_size % 64 == 0, "config: intermediate sizes must be multiples of 64");
    BVC_REQUIRE((c.num_channels * c.tubelet_size * c.patch_size * c.patch_size) % 64 == 0, "config: patch dim must be a multiple of 64");
    BVC_REQUIRE(c.num_hidden_layers >= 1 && c.decoder_num_hidden_layers >= 1, "config: need at least one layer each");
    return BVC_OK;
}

Layout make_layout(const bvc_videomae_config& c) {
    Layout L;
    const int64_t D = c.hidden_size, Dd = c.decoder_hidden_size;
    const int64_t P = (int64_t)c.num_channels * c.tubelet_size * c.patch_size * c.patch_size;
    const std::string pe = "videomae.embeddings.patch_embeddings.projection.";
    L.pe_w = L.add(pe + "weight", {D, c.num_channels, c.tubelet_size, c.patch_size, c.patch_size});
    L.pe_b = L.add(pe + "bias", {D});
    for (int i = 0; i < c.num_hidden_layers; ++i)
        L.enc.push_back(add_layer_params(L, "videomae.encoder.layer." + std::to_string(i) + ".", D, c.intermediate_size, true));
    L.e2d_w = L.add("encoder_to_decoder.weight", {Dd, D});
    L.mask_token = L.add("mask_token", {1, 1, Dd});
    for (int i = 0; i < c.decoder_num_hidden_layers; ++i)
        L.dec.push_back(add_layer_params(L, "decoder.decoder_layers." + std::to_string(i) + ".", Dd, c.decoder_intermediate_size, true));
    L.norm_w = L.add("decoder.norm.weight", {Dd});
    L.norm_b = L.add("decoder.norm.bias", {Dd});
    L.head_w = L.add("decoder.head.weight", {P, Dd});
    L.head_b = L.add("decoder.head.bias", {P});
    return L;
}

}  // namespace

struct bvc_ctx {
    bvc_videomae_config cfg;
    Layout lay;
    int max_batch, nmask, nvis, L, P;
    // the decoder reconstructs ndec of the nmask masked tokens (all of them unless the context was made by bvc_videomae_create_dual):
    // Ld = nvis + ndec rows per clip, the visible tokens first
    int ndec, Ld;
    Arena arena;
    Work w;
    // constants
    float *pos_enc, *pos_dec;
    // per-step state
    int batch = 0;
    bool have_forward = false;
    Shadow shadow;     // bf16 copy of the flat parameters (bvc_videomae_shadow)
    const float* params = nullptr;
    int *vis_idx, *dec_idx, *status;     // dec_idx [B][ndec]: the decoded masked tokens, ascending
    PatchFront front;  // the visible tubes
    Stack enc, dec;
    bf16_t* xe_bf;     // bf16 [B*nvis][D] encoder output
    float *meanf, *rstdf;
    bf16_t* lnf;       // bf16 [B*ndec][Dd]
    float* labels;     // f32 [B*ndec][P]
    bf16_t* diff;      // bf16 [B*ndec][P]  logits - labels
    float* partial;
    int npartial = 0;
    float *dres_enc, *dres_dec;
    bf16_t* de2d;
    // the last forward ran the last decoder layer in tail mode (stack.h LayerTail): dec.x_out and that layer's activations behind qkv
    // hold the B * ndec decoded rows, compact; its backward and the "dec<last>" tap follow suit
    bool tail_on = false;
    // first mode of the first decoder layer (stack.h LayerFirst): the per-position tables and compact operands, allocated when the decoder
    // has the shapes for it; first_on = the last forward ran that way (its backward follows suit)
    int *dec_slot = nullptr, *pos_iota = nullptr;      // [B][L]; [2 L] = p mod L
    LayerFirst first{};
    bool first_on = false;
};

namespace {

int upload_sinusoid(float* dst, int n, int d) {   // HF:80-91, float64 then cast
    std::vector<float> out((size_t)n * d);
    for (int p = 0; p < n; ++p)
        for (int j = 0; j < d; ++j) {
            const double ang = (double)p / pow(10000.0, 2.0 * (j / 2) / (double)d);
            out[(size_t)p * d + j] = (float)((j & 1) ? cos(ang) : sin(ang));
        }
    if (hipMemcpy(dst, out.data(), out.size() * 4, hipMemcpyHostToDevice) != hipSuccess) { set_error("create: pos upload failed"); return BVC_ERR_HIP; }
    return BVC_OK;
}

// the softmax scale a stack passes to its attention launches: the true head's when the heads run zero-padded, the default otherwise
float stack_sm_scale(const Stack& s) { return s.hdp != s.hd ? 1.0f / sqrtf((float)s.hd) : 0.f; }

}  // namespace

// ============================================================================ C ABI
extern "C" {

int bvc_videomae_param_count(const bvc_videomae_config* cfg) {
    if (!cfg || check_config(*cfg) != BVC_OK) return BVC_ERR_INVALID;
    return (int)make_layout(*cfg).entries.size();
}

int64_t bvc_videomae_param_numel(const bvc_videomae_config* cfg) {
    if (!cfg || check_config(*cfg) != BVC_OK) return BVC_ERR_INVALID;
    return make_layout(*cfg).total;
}

int bvc_videomae_param_info(const bvc_videomae_config* cfg, int index, char* name, int name_cap, int64_t* offset,
                            int64_t* numel, int* ndim, int64_t shape[5]) {
    BVC_REQUIRE(cfg && name && offset && numel && ndim && shape, "param_info: null argument");
    TRY(check_config(*cfg));
    return param_info(make_layout(*cfg), index, name, name_cap, offset, numel, ndim, shape);
}

void bvc_videomae_destroy(bvc_ctx* c) {
    if (!c) return;
    free_work(c->w);
    c->arena.release();
    delete c;
}

int bvc_videomae_create(const bvc_videomae_config* cfg, int max_batch, int num_masked, bvc_ctx** out) {
    return bvc_videomae_create_dual(cfg, max_batch, num_masked, num_masked, out);
}

int bvc_videomae_create_dual(const bvc_videomae_config* cfg, int max_batch, int num_masked, int num_decoded, bvc_ctx** out) {
    BVC_REQUIRE(cfg && out, "create: null argument");
    TRY(check_config(*cfg));
    BVC_REQUIRE(max_batch >= 1, "create: max_batch must be >= 1");
    const PatchGeom pg = patch_geom(*cfg);
    const int L = seq_len(pg), nvis = L - num_masked, Ld = nvis + num_decoded;
    BVC_REQUIRE(num_masked >= 1 && nvis >= 1, "create: num_masked=%d must leave at least one visible and one masked token of %d", num_masked, L);
    BVC_REQUIRE(num_decoded >= 1 && num_decoded <= num_masked, "create: num_decoded=%d must lie in [1, num_masked=%d]", num_decoded, num_masked);
    // decoder side: Md rows of Ld per clip, Mm decoded rows
    const size_t B = max_batch, Mv = B * nvis, Md = B * Ld, Mm = B * num_decoded;
    const int D = cfg->hidden_size, Dd = cfg->decoder_hidden_size, I = cfg->intermediate_size, Id = cfg->decoder_intermediate_size;
    const int H = cfg->num_attention_heads, Hd = cfg->decoder_num_attention_heads;
    {   // refuse before allocating anything (alloc_stack checks it again).  The widest operand is the decoder's fc1 output (VideoMAE-H:
        // 1568 x 2560 per clip, 4 GiB at 534 clips; from 2 GiB, 267 clips, the 256-row persistent GEMM hands those products to the
        // 128 x 128 kernels)
        const size_t we = std::max<size_t>(3 * (size_t)H * attn_width(D / H), (size_t)I), wd = std::max<size_t>(3 * (size_t)Hd * attn_width(Dd / Hd), (size_t)Id);
        const bool dec = Ld * wd >= nvis * we;
        TRY(refuse_operand_extent("create", max_batch, dec ? Ld : nvis, dec ? wd : we, dec ? "decoder" : "encoder"));
    }
    bvc_ctx* c = new bvc_ctx();
    Making guard{[&] { bvc_videomae_destroy(c); }};
    c->cfg = *cfg;
    c->lay = make_layout(*cfg);
    c->max_batch = max_batch;
    c->L = L; c->P = patch_dim(pg);
    c->nmask = num_masked; c->nvis = nvis; c->ndec = num_decoded; c->Ld = Ld;
    TRY(c->arena.alloc(&c->pos_enc, (size_t)L * D));
    TRY(c->arena.alloc(&c->pos_dec, (size_t)L * Dd));
    TRY(c->shadow.alloc(c->arena, c->lay.total));
    TRY(c->arena.alloc(&c->vis_idx, Mv));
    TRY(c->arena.alloc(&c->dec_idx, Mm));
    // token 0 everywhere: a clip whose mask (or decode) count differs from the context's leaves entries unwritten, and the gather kernels
    // must then read in-range indices (the status word flags the clip; the Python side raises on the next step)
    BVC_CHECK_HIP(hipMemset(c->vis_idx, 0, (size_t)Mv * sizeof(int)));
    BVC_CHECK_HIP(hipMemset(c->dec_idx, 0, (size_t)Mm * sizeof(int)));
    TRY(c->arena.alloc(&c->status, 4));
    TRY(c->front.alloc(c->arena, pg, Mv, false));
    TRY(alloc_stack(c->arena, c->enc, D, I, H, cfg->num_hidden_layers, cfg->layer_norm_eps, Mv, B * H * nvis));
    TRY(alloc_stack(c->arena, c->dec, Dd, Id, Hd, cfg->decoder_num_hidden_layers, cfg->layer_norm_eps, Md, B * Hd * Ld));
    TRY(c->arena.alloc(&c->xe_bf, Mv * D));
    TRY(c->arena.alloc(&c->meanf, Mm));
    TRY(c->arena.alloc(&c->rstdf, Mm));
    TRY(c->arena.alloc(&c->lnf, Mm * Dd));
    TRY(c->arena.alloc(&c->labels, Mm * c->P));
    TRY(c->arena.alloc(&c->diff, Mm * c->P));
    TRY(c->arena.alloc(&c->partial, (Mm / 64 + 2) * (c->P / 64 + 2)));
    TRY(c->arena.alloc(&c->dres_enc, Mv * D));
    TRY(c->arena.alloc(&c->dres_dec, Md * Dd));
    TRY(c->arena.alloc(&c->de2d, Mv * Dd));
    TRY(alloc_work(c->arena, c->w, std::max(Mv * D, Md * Dd), std::max(Mv * I, Md * Id), std::max(B * H * nvis, B * Hd * Ld),
                   std::max(ln_bwd_workspace_floats_upto((int)Mv, D), ln_bwd_workspace_floats_upto((int)Md, Dd))));
    TRY(upload_sinusoid(c->pos_enc, L, D));
    TRY(upload_sinusoid(c->pos_dec, L, Dd));
    if (c->dec.nlayers >= 2 && c->dec.hdp == c->dec.hd) {
        LayerFirst& f = c->first;
        const size_t T = 2 * (size_t)L, Mf = Mv + T;
        float* t0 = nullptr;
        f.nvis = nvis; f.ndec = num_decoded; f.L = L;
        TRY(c->arena.alloc(&c->dec_slot, B * L));
        TRY(c->arena.alloc(&c->pos_iota, T));
        TRY(c->arena.alloc(&t0, T * Dd));
        TRY(c->arena.alloc(&f.tmean, T));
        TRY(c->arena.alloc(&f.trstd, T));
        TRY(c->arena.alloc(&f.ln1c, Mf * Dd));
        TRY(c->arena.alloc(&f.qc, Mf * 3 * c->dec.Da));
        TRY(c->arena.alloc(&f.xt, T * Dd));
        TRY(c->arena.alloc(&f.dt, T * Dd));
        TRY(c->arena.alloc(&f.dyt, T * Dd));
        TRY(c->arena.alloc(&f.part, ln_bwd_workspace_floats_upto((int)T, Dd)));
        TRY(c->arena.alloc(&f.xv, Mv * Dd));
        TRY(c->arena.alloc(&f.dyv, 2 * Mv * Dd));
        f.t0 = t0; f.dec_idx = c->dec_idx; f.dec_slot = c->dec_slot;
        TRY(launch_iota_mod(c->pos_iota, (int)T, L, nullptr));
        BVC_CHECK_HIP(hipStreamSynchronize(nullptr));
    }
    guard.done = true;
    *out = c;
    return BVC_OK;
}

int bvc_videomae_forward(bvc_ctx* c, const float* pixels, const uint8_t* mask, int batch, const float* params,
                         float* loss, float* logits, void* stream) {
    return bvc_videomae_forward_px(c, pixels, nullptr, mask, batch, params, loss, logits, stream);
}

int bvc_videomae_forward_px(bvc_ctx* c, const void* pixels_any, const bvc_pixel_format* fmt, const uint8_t* mask, int batch,
                            const float* params, float* loss, float* logits, void* stream) {
    return bvc_videomae_forward_dual(c, pixels_any, fmt, mask, nullptr, batch, params, loss, logits, stream);
}

int bvc_videomae_forward_dual(bvc_ctx* c, const void* pixels_any, const bvc_pixel_format* fmt, const uint8_t* mask, const uint8_t* decode_mask,
                              int batch, const float* params, float* loss, float* logits, void* stream) {
    BVC_REQUIRE(c && pixels_any && mask && params && loss, "forward: null argument");
    BVC_REQUIRE(decode_mask || c->ndec == c->nmask, "forward: the context decodes %d of %d masked tokens and needs a decode mask", c->ndec, c->nmask);
    PixelSrc pixels;
    TRY(pixel_src("forward", pixels_any, fmt, c->cfg.num_channels, &pixels));
    BVC_REQUIRE(batch >= 1 && batch <= c->max_batch, "forward: batch %d outside [1, %d]", batch, c->max_batch);
    hipStream_t st = (hipStream_t)stream;
    const bvc_videomae_config& cf = c->cfg;
    const Layout& L = c->lay;
    const int B = batch, nvis = c->nvis, ndec = c->ndec, Lq = c->L, Ld = c->Ld;
    const int Mv = B * nvis, Mm = B * ndec;
    const int D = cf.hidden_size, Dd = cf.decoder_hidden_size, P = c->P;
    c->have_forward = false;
    c->batch = B;
    c->params = params;
    c->w.params = params;
    c->w.wbf = c->shadow.wbf;
    const bf16_t* W = c->shadow.wbf;

    TRY(c->shadow.refresh(params, st));
    BVC_CHECK_HIP(hipMemsetAsync(c->status, 0, 16, st));
    if (decode_mask) TRY(launch_dual_mask_index(mask, decode_mask, B, Lq, nvis, ndec, c->vis_idx, c->dec_idx, c->status, st));
    else TRY(launch_mask_index(mask, B, Lq, nvis, ndec, c->vis_idx, c->dec_idx, c->status, st));
    // tube patch embedding of the visible tokens + bias + sinusoid
    TRY(c->front.embed(pixels, c->vis_idx, B, nvis, W + L.pe_w, params + L.pe_b, c->pos_enc, c->enc.act[0].x_in, D, st, "forward"));
    TRY(stack_forward(c->w, c->enc, L.enc, B, nvis, st, true));
    // encoder -> decoder glue (HF:566-582)
    TRY(launch_gather_rows_bf16(c->enc.x_out, identity_rows(), c->xe_bf, Mv, D, st));
    {
        GemmProblem p = gemm(c->xe_bf, (size_t)Mv * D, D, W + L.e2d_w, (size_t)Dd * D, D, Mv, Dd, D, EPI_E2D, c->dec.act[0].x_in, Dd);
        p.rowtok = c->vis_idx; p.pos = c->pos_dec; p.rin = nvis; p.rout = Ld;
        TRY(launch_gemm(&p, 1, GEMM_NT, -1, st));
    }
    // the decoded rows enter as mask_token + pos[p]: in first mode the first layer works on the L-row table of them (twice over: stack.h) and
    // writes the rows themselves when it assembles its qkv
    c->first_on = c->dec_slot != nullptr && layer_first_ok(c->w, c->dec, B, nvis, ndec);
    if (c->first_on) {
        TRY(launch_dec_slot(c->dec_idx, c->dec_slot, B, Lq, ndec, st));
        TRY(launch_fill_masked(const_cast<float*>(c->first.t0), params + L.mask_token, c->pos_dec, c->pos_iota, 1, 2 * Lq, 0, 2 * Lq, Dd, st));
    } else {
        TRY(launch_fill_masked(c->dec.act[0].x_in, params + L.mask_token, c->pos_dec, c->dec_idx, B, Ld, nvis, ndec, Dd, st));
    }
    // the head reads the decoded rows only: the last layer computes nothing else behind its qkv product when the shapes allow (tail mode)
    const LayerTail lt{nvis, ndec};
    c->tail_on = layer_tail_ok(c->w, c->dec, B, nvis, ndec);
    TRY(stack_forward(c->w, c->dec, L.dec, B, Ld, st, true, c->tail_on ? &lt : nullptr, c->first_on ? &c->first : nullptr));
    // last ndec tokens -> LayerNorm -> head, fused with the pixel-target MSE (HF:497-501,588-664); in tail mode x_out holds just those rows
    const RowMap tail = c->tail_on ? identity_rows() : RowMap{ndec, Ld, nvis};
    TRY(launch_ln_fwd(c->dec.x_out, tail, params + L.norm_w, params + L.norm_b, c->lnf, c->meanf, c->rstdf, Mm, Dd, cf.decoder_norm_eps, st));
    TRY(launch_labels(pixels, c->dec_idx, c->labels, B, ndec, c->front.pg, cf.norm_pix_loss, st));
    {
        GemmProblem p = gemm(c->lnf, (size_t)Mm * Dd, Dd, W + L.head_w, (size_t)P * Dd, Dd, Mm, P, Dd, EPI_LOSS, c->diff, P);
        p.bias = params + L.head_b; p.labels = c->labels; p.partial = c->partial; p.C2 = logits;
        c->npartial = gemm_num_tiles(p, -1);
        TRY(launch_gemm(&p, 1, GEMM_NT, -1, st));
    }
    TRY(launch_loss_finalize(c->partial, c->npartial, (double)Mm * (double)P, c->status, loss, st));
    c->have_forward = true;
    return BVC_OK;
}

int bvc_videomae_backward(bvc_ctx* c, const float* grad_loss, float* G, bvc_bucket_fn on_bucket, void* user, void* stream) {
    BVC_REQUIRE(c && grad_loss && G, "backward: null argument");
    if (!c->have_forward) { set_error("backward: no forward state (call bvc_videomae_forward first; one backward per forward)"); return BVC_ERR_STATE; }
    c->have_forward = false;
    hipStream_t st = (hipStream_t)stream;
    const bvc_videomae_config& cf = c->cfg;
    const Layout& L = c->lay;
    const int B = c->batch, nvis = c->nvis, ndec = c->ndec, Ld = c->Ld;
    const int Mv = B * nvis, Md = B * Ld, Mm = B * ndec;
    const int D = cf.hidden_size, Dd = cf.decoder_hidden_size, P = c->P;
    const bf16_t* W = c->shadow.wbf;
    const float* params = c->params;
    begin_backward(c->w);

    BVC_CHECK_HIP(hipMemsetAsync(G, 0, (size_t)L.total * 4, st));
    // d loss / d logits = (2 / (Mm P)) * diff * grad_loss  - folded into alpha of the three head products
    const float cmse = (float)(2.0 / ((double)Mm * (double)P));
    {
        GemmProblem p = gemm(c->diff, (size_t)Mm * P, P, c->lnf, (size_t)Mm * Dd, Dd, P, Dd, Mm, EPI_F32, G + L.head_w, Dd);
        p.alpha = cmse; p.alpha_dev = grad_loss;
        p.rowsum = G + L.head_b;
        const int tile = plan_dw(&p, 1);
        TRY(launch_gemm(&p, 1, GEMM_TN, tile, st));
    }
    {
        GemmProblem p = gemm(c->diff, (size_t)Mm * P, P, W + L.head_w, (size_t)P * Dd, Dd, Mm, Dd, P, EPI_BF16, c->w.dln, Dd);
        p.alpha = cmse; p.alpha_dev = grad_loss;
        TRY(launch_gemm(&p, 1, GEMM_NN, -1, st));
    }
    // visible rows of the decoder stream receive no gradient from the head
    const RowMap tail{ndec, Ld, nvis};
    const LayerTail lt{nvis, ndec};
    if (c->tail_on) {
        // tail mode: the LayerNorm backward writes every decoded row of dres_dec, so only the visible rows are zeroed (one strided fill);
        // x_out and the bf16 copy hold the decoded rows compact - nothing of dyb[0] is left unwritten, its fill is gone
        BVC_CHECK_HIP(hipMemset2DAsync(c->dres_dec, (size_t)Ld * Dd * 4, 0, (size_t)nvis * Dd * 4, (size_t)B, st));
        TRY(launch_ln_bwd(c->w.dln, c->dec.x_out, tail, c->meanf, c->rstdf, params + L.norm_w, c->dres_dec, 0, c->w.dyb[0],
                          G + L.norm_w, G + L.norm_b, c->w.ln_part, Mm, Dd, st, nullptr, true));
    } else {
        BVC_CHECK_HIP(hipMemsetAsync(c->dres_dec, 0, (size_t)Md * Dd * 4, st));
        BVC_CHECK_HIP(hipMemsetAsync(c->w.dyb[0], 0, (size_t)Md * Dd * 2, st));
        TRY(launch_ln_bwd(c->w.dln, c->dec.x_out, tail, c->meanf, c->rstdf, params + L.norm_w, c->dres_dec, 0, c->w.dyb[0],
                          G + L.norm_w, G + L.norm_b, c->w.ln_part, Mm, Dd, st));
    }
    if (on_bucket) on_bucket(L.norm_w, L.total - L.norm_w, user);
    c->first.dtoken = G + L.mask_token;
    TRY(stack_backward(c->w, c->dec, L.dec, c->dres_dec, G, B, Ld, st, on_bucket, user, c->tail_on ? &lt : nullptr, c->first_on ? &c->first : nullptr));
    // decoder input: mask token, encoder_to_decoder
    TRY(launch_colsum_f32(c->dres_dec, tail, Mm, Dd, G + L.mask_token, st));
    const RowMap headrows{nvis, Ld, 0};
    TRY(launch_gather_rows_bf16(c->dres_dec, headrows, c->de2d, Mv, Dd, st));
    {
        GemmProblem p = gemm(c->de2d, (size_t)Mv * Dd, Dd, c->xe_bf, (size_t)Mv * D, D, Dd, D, Mv, EPI_F32, G + L.e2d_w, D);
        const int tile = plan_dw(&p, 1);
        TRY(launch_gemm(&p, 1, GEMM_TN, tile, st));
    }
    {
        GemmProblem p = gemm(c->de2d, (size_t)Mv * Dd, Dd, W + L.e2d_w, (size_t)Dd * D, D, Mv, D, Dd, EPI_F32_BF16, c->dres_enc, D);
        p.C2 = c->w.dyb[c->w.seq % 3];   // last read (as a dW operand) by backward step seq-3, fenced since
        TRY(launch_gemm(&p, 1, GEMM_NN, -1, st));
    }
    if (on_bucket) on_bucket(L.e2d_w, L.dec.front().ln1w - L.e2d_w, user);
    TRY(stack_backward(c->w, c->enc, L.enc, c->dres_enc, G, B, nvis, st, on_bucket, user));
    TRY(c->front.embed_backward(c->w, Mv, D, G + L.pe_w, G + L.pe_b, st));
    TRY(join_both(c->w, st, on_bucket, user));
    if (on_bucket) on_bucket(0, L.enc.front().ln1w, user);
    return BVC_OK;
}

// "dec<last>" after a forward in tail mode: the layer's output exists for the decoded rows only (dec.x_out, compact).  The visible rows
// are completed here, off the training path: attention with the query window (0, nvis), then proj + residual, LayerNorm 2, fc1 + GELU
// and fc2 + residual on the B * nvis gathered rows with the ordinary kernels.  Scratch: the layer's own activation buffers, allocated
// for B * Ld rows, hold B * ndec in tail mode - the completion lives in the B * nvis rows behind them, so neither a later backward
// nor a second tap finds anything changed.  It uses the parameters of the forward (the caller's `params` and the bf16 copy): ask for the
// tap before an optimiser step rewrites them.
static int tail_tap(bvc_ctx* c, float* dst, hipStream_t st) {
    const Layout& L = c->lay;
    Stack& s = c->dec;
    LayerAct& a = s.act.back();
    const LayerOff& o = L.dec.back();
    const int B = c->batch, nvis = c->nvis, ndec = c->ndec, Ld = c->Ld, D = s.D, I = s.I, Da = s.Da;
    const size_t Mq = (size_t)B * ndec, Mv = (size_t)B * nvis;
    const float* P = c->params;
    const bf16_t* W = c->shadow.wbf;
    bf16_t *ctx_v = a.ctx + Mq * Da, *ln2o_v = a.ln2o + Mq * D, *pre_v = a.pre + Mq * I, *act_v = a.act + Mq * I;
    float *lse_v = a.lse + (size_t)B * s.H * ndec, *h_v = a.h + Mq * D, *mean_v = a.mean2 + Mq, *rstd_v = a.rstd2 + Mq, *out_v = s.x_out + Mq * D;
    const size_t full = (size_t)Ld * D * 4, vis = (size_t)nvis * D * 4, dec = (size_t)ndec * D * 4;
    TRY(launch_attn_fwd_win(a.qkv, ctx_v, lse_v, B, Ld, s.H, s.hdp, 0, nvis, st));
    BVC_CHECK_HIP(hipMemcpy2DAsync(h_v, vis, a.x_in, full, vis, (size_t)B, hipMemcpyDeviceToDevice, st));     // the residual input of the visible rows
    {
        GemmProblem p = gemm(ctx_v, Mv * Da, Da, W + o.wo, (size_t)D * Da, Da, (int)Mv, D, Da, EPI_RESID, h_v, D);
        p.bias = P + o.bo; p.resid = h_v;
        TRY(launch_gemm(&p, 1, GEMM_NT, -1, st));
    }
    TRY(launch_ln_fwd(h_v, identity_rows(), P + o.ln2w, P + o.ln2b, ln2o_v, mean_v, rstd_v, (int)Mv, D, s.eps, st));
    {
        GemmProblem p = gemm(ln2o_v, Mv * D, D, W + o.w1, (size_t)I * D, D, (int)Mv, I, D, EPI_GELU, pre_v, I);
        p.bias = P + o.b1; p.C2 = act_v;
        TRY(launch_gemm(&p, 1, GEMM_NT, -1, st));
    }
    {
        GemmProblem p = gemm(act_v, Mv * I, I, W + o.w2, (size_t)D * I, I, (int)Mv, D, I, EPI_RESID, out_v, D);
        p.bias = P + o.b2; p.resid = h_v;
        TRY(launch_gemm(&p, 1, GEMM_NT, -1, st));
    }
    BVC_CHECK_HIP(hipMemcpy2DAsync(dst, full, out_v, vis, vis, (size_t)B, hipMemcpyDeviceToDevice, st));
    BVC_CHECK_HIP(hipMemcpy2DAsync(dst + (size_t)nvis * D, full, s.x_out, dec, dec, (size_t)B, hipMemcpyDeviceToDevice, st));
    return BVC_OK;
}

int bvc_videomae_tap(bvc_ctx* c, const char* name, float* dst, int64_t capacity, int64_t* numel, void* stream) {
    BVC_REQUIRE(c && name && dst && numel, "tap: null argument");
    BVC_REQUIRE(c->batch > 0, "tap: no forward has run");
    const int B = c->batch;
    const size_t Mv = (size_t)B * c->nvis, Md = (size_t)B * c->Ld, Mm = (size_t)B * c->ndec;
    const int D = c->cfg.hidden_size, Dd = c->cfg.decoder_hidden_size;
    const float* src = nullptr;
    size_t n = 0;
    int idx = -1;
    if (!strcmp(name, "embed")) { src = c->enc.act[0].x_in; n = Mv * D; }
    else if (!strcmp(name, "x_full")) { src = c->dec.act[0].x_in; n = Md * Dd; }
    else if (!strcmp(name, "labels")) { src = c->labels; n = Mm * c->P; }
    else if (sscanf(name, "enc%d", &idx) == 1 && idx >= 0 && idx < c->enc.nlayers) {
        src = idx + 1 < c->enc.nlayers ? c->enc.act[idx + 1].x_in : c->enc.x_out; n = Mv * D;
    } else if (sscanf(name, "dec%d", &idx) == 1 && idx >= 0 && idx < c->dec.nlayers) {
        src = idx + 1 < c->dec.nlayers ? c->dec.act[idx + 1].x_in : c->dec.x_out; n = Md * Dd;
    }
    BVC_REQUIRE(src, "tap: unknown activation '%s'", name);
    *numel = (int64_t)n;
    BVC_REQUIRE((int64_t)n <= capacity, "tap: destination holds %lld elements, '%s' has %lld", (long long)capacity, name, (long long)n);
    if (src == c->dec.x_out && c->tail_on) return tail_tap(c, dst, (hipStream_t)stream);
    BVC_CHECK_HIP(hipMemcpyAsync(dst, src, n * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return BVC_OK;
}

// ------------------------------------------------------------------ encoder-only inference (embedding extraction)
// Replaces VideoMAEForVideoClassification(num_labels=0).forward as benchmarks/compute_embeddings_videomae.py:78-96,253-264
// uses it between curriculum stages: all tokens (no mask) -> encoder -> mean over tokens -> fc_norm (HF
// VideoMAEForVideoClassification.forward; VideoMAEModel.layernorm is None under use_mean_pooling).  Forward only: ONE set of
// layer activations is reused by every layer, so the working set is independent of depth.
struct bvc_encoder_ctx {
    bvc_videomae_config cfg;
    Layout lay;
    int max_batch, L;
    Arena arena;
    Work w;            // parameter views only; no backward scratch is allocated
    Stack st;          // one LayerAct
    float *pos_enc, *xa, *xb, *pooled, *mean, *rstd;
    Shadow shadow;           // never vouched: every encode casts
    PatchFront front;
    int pooled_batch = 0;    // clips whose pre-norm pooled rows and fc_norm statistics the last encode left (0: none)
    DropState drop;          // bvc_videomae_encoder_set_drop: the forward gate of a train-mode module on the forward-only path
    MixState mix;            // bvc_videomae_encoder_set_mix
    EraseState erase;        // bvc_videomae_encoder_set_erase
};

void bvc_videomae_encoder_destroy(bvc_encoder_ctx* c) {
    if (!c) return;
    c->arena.release();
    delete c;
}

int64_t bvc_videomae_encoder_param_numel(const bvc_videomae_config* cfg) {
    if (!cfg || check_config(*cfg) != BVC_OK) return BVC_ERR_INVALID;
    return make_layout(*cfg).e2d_w;    // the "videomae.*" entries are the leading part of the pre-training layout
}

int bvc_videomae_encoder_create(const bvc_videomae_config* cfg, int max_batch, bvc_encoder_ctx** out) {
    BVC_REQUIRE(cfg && out && max_batch >= 1, "encoder_create: bad argument");
    TRY(check_config(*cfg));
    const PatchGeom pg = patch_geom(*cfg);
    const size_t M = (size_t)max_batch * seq_len(pg);
    const int D = cfg->hidden_size, I = cfg->intermediate_size, H = cfg->num_attention_heads;
    BVC_REQUIRE(M * (size_t)std::max(I, patch_dim(pg)) * 2 + operand_tail_bytes((size_t)std::max(I, patch_dim(pg))) <= 0x100000000ull, "encoder_create: max_batch %d needs operands above 4 GiB", max_batch);
    bvc_encoder_ctx* c = new bvc_encoder_ctx();
    Making guard{[&] { bvc_videomae_encoder_destroy(c); }};
    c->cfg = *cfg;
    c->lay = make_layout(*cfg);
    c->max_batch = max_batch;
    c->L = seq_len(pg);
    TRY(c->arena.alloc(&c->pos_enc, (size_t)c->L * D));
    TRY(c->shadow.alloc(c->arena, c->lay.e2d_w));
    TRY(c->front.alloc(c->arena, pg, M, true));
    TRY(alloc_stack(c->arena, c->st, D, I, H, 1, cfg->layer_norm_eps, M, (size_t)max_batch * H * c->L));
    TRY(alloc_drop(c->arena, c->drop, cfg->num_hidden_layers, max_batch));
    TRY(alloc_mix(c->arena, c->mix, max_batch));
    TRY(alloc_erase(c->arena, c->erase, max_batch));
    TRY(c->arena.alloc(&c->xa, M * D));
    TRY(c->arena.alloc(&c->xb, M * D));
    TRY(c->arena.alloc(&c->pooled, (size_t)max_batch * D));
    TRY(c->arena.alloc(&c->mean, (size_t)max_batch));
    TRY(c->arena.alloc(&c->rstd, (size_t)max_batch));
    TRY(upload_sinusoid(c->pos_enc, c->L, D));
    guard.done = true;
    *out = c;
    return BVC_OK;
}

int bvc_videomae_encode(bvc_encoder_ctx* c, const float* pixels, int batch, const float* params, const float* fc_norm_w,
                        const float* fc_norm_b, float fc_norm_eps, float* tokens, float* pooled, void* stream) {
    return bvc_videomae_encode_px(c, pixels, nullptr, batch, params, fc_norm_w, fc_norm_b, fc_norm_eps, tokens, pooled, stream);
}

int bvc_videomae_encode_px(bvc_encoder_ctx* c, const void* pixels_any, const bvc_pixel_format* fmt, int batch, const float* params,
                           const float* fc_norm_w, const float* fc_norm_b, float fc_norm_eps, float* tokens, float* pooled,
                           void* stream) {
    return bvc_videomae_encode_ex(c, pixels_any, fmt, batch, params, fc_norm_w, fc_norm_b, fc_norm_eps, tokens, pooled, nullptr, stream);
}

int bvc_videomae_encode_ex(bvc_encoder_ctx* c, const void* pixels_any, const bvc_pixel_format* fmt, int batch, const float* params,
                           const float* fc_norm_w, const float* fc_norm_b, float fc_norm_eps, float* tokens, float* pooled,
                           const bvc_introspect* out, void* stream) {
    float* const hs = out ? out->hidden_states : nullptr;      // [L + 1][B][N][D]: the residual stream runs through it
    float* const att = out ? out->attentions : nullptr;        // [L][B][H][N][N]
    BVC_REQUIRE(c && pixels_any && params && (tokens || pooled || hs || att), "encode: null argument");
    PixelSrc pixels;
    TRY(pixel_src("encode", pixels_any, fmt, c->cfg.num_channels, &pixels));
    BVC_REQUIRE(batch >= 1 && batch <= c->max_batch, "encode: batch %d outside [1, %d]", batch, c->max_batch);
    BVC_REQUIRE((fc_norm_w == nullptr) == (fc_norm_b == nullptr), "encode: fc_norm weight and bias go together");
    hipStream_t st = (hipStream_t)stream;
    const bvc_videomae_config& cf = c->cfg;
    const Layout& L = c->lay;
    const int B = batch, N = c->L, M = B * N, D = cf.hidden_size;
    c->w.params = params;
    c->w.wbf = c->shadow.wbf;
    c->w.drop = &c->drop;
    TRY(take_drop(c->drop, B, N, "encode"));
    TRY(c->shadow.refresh(params, st));
    const size_t slot = (size_t)M * D;                         // one hidden state
    float* x = hs ? hs : c->xa;                                // given hidden_states, slot 0 is the embedding output
    float* y = c->xb;
    bool mixed = false;
    TRY(c->front.embed(pixels, c->front.idx_all, B, N, c->shadow.wbf + L.pe_w, params + L.pe_b, c->pos_enc, x, D, st, "encode", &c->mix, &mixed,
                       &c->erase));
    const int nl = (int)L.enc.size();
    for (int i = 0; i < nl; ++i) {
        // the last layer writes straight into the caller's buffer; with hidden_states, layer i reads slot i and writes slot i + 1
        float* dst = hs ? hs + (size_t)(i + 1) * slot : (i + 1 == nl && tokens) ? tokens : y;
        c->w.drop_layer = i;     // one LayerAct serves every layer: the gate is keyed by the real layer
        TRY(layer_forward(c->w, c->st, 0, L.enc[i], x, dst, B, N, st));
        if (att)
            TRY(launch_attn_probs(c->st.act[0].qkv, c->st.act[0].lse, att + (size_t)i * B * c->st.H * N * N, B, N, c->st.H, c->st.hdp, st,
                                  stack_sm_scale(c->st)));
        if (dst == y) std::swap(x, y); else x = dst;
    }
    if (hs && tokens) BVC_CHECK_HIP(hipMemcpyAsync(tokens, x, slot * 4, hipMemcpyDeviceToDevice, st));
    if (mixed && tokens) TRY(launch_poison_on_status(tokens, slot, c->mix.status, st));
    c->drop.active = false;      // forward only: nothing follows that would need the gate
    c->pooled_batch = 0;
    if (pooled) {
        float* mp = fc_norm_w ? c->pooled : pooled;
        TRY(launch_token_mean(x, B, N, D, mp, st));
        if (fc_norm_w)
            TRY(launch_ln_fwd(mp, identity_rows(), fc_norm_w, fc_norm_b, nullptr, c->mean, c->rstd, B, D, fc_norm_eps, st, pooled));
        if (fc_norm_w) c->pooled_batch = B;
        if (mixed) TRY(launch_poison_on_status(pooled, (size_t)B * D, c->mix.status, st));
    }
    return BVC_OK;
}

int bvc_videomae_encoder_set_drop(bvc_encoder_ctx* c, const bvc_branch_drop* drop, int samples, void* stream) {
    BVC_REQUIRE(c, "encoder_set_drop: null context");
    return set_drop(c->drop, drop, samples, "encoder_set_drop", (hipStream_t)stream);
}

int bvc_videomae_encoder_set_mix(bvc_encoder_ctx* c, const bvc_clip_mix* mix_dev, int samples, void* stream) {
    (void)stream;      // the table is copied by the forward that consumes it, on that forward's stream
    BVC_REQUIRE(c, "encoder_set_mix: null context");
    return set_mix(c->mix, mix_dev, samples, c->max_batch, "encoder_set_mix");
}

int bvc_videomae_encoder_set_erase(bvc_encoder_ctx* c, const bvc_erase_box* tab_dev, int samples, int boxes, uint64_t seed, uint64_t offset,
                                   void* stream) {
    (void)stream;      // as for the mix: copied by the forward that consumes it
    BVC_REQUIRE(c, "encoder_set_erase: null context");
    return set_erase(c->erase, tab_dev, samples, boxes, seed, offset, c->max_batch, "encoder_set_erase");
}

int bvc_videomae_encoder_fc_norm_backward(bvc_encoder_ctx* c, const float* dpooled, const float* fc_norm_w, float* dfc_norm_w,
                                          float* dfc_norm_b, void* stream) {
    BVC_REQUIRE(c && dpooled && fc_norm_w && dfc_norm_w && dfc_norm_b, "encoder_fc_norm_backward: null argument");
    if (c->pooled_batch < 1) {
        set_error("encoder_fc_norm_backward: the last encode ran no fc_norm (call bvc_videomae_encode_px with fc_norm weights first)");
        return BVC_ERR_STATE;
    }
    return launch_fcnorm_bwd_bcast(dpooled, c->pooled, c->mean, c->rstd, fc_norm_w, nullptr, nullptr, dfc_norm_w, dfc_norm_b,
                                   c->pooled_batch, c->L, c->cfg.hidden_size, (hipStream_t)stream);
}

// ------------------------------------------------------------------ fine-tuning (VideoMAEForVideoClassification with labels)
// The encoder of the inference context above at full sequence length, with autograd: every layer keeps its own LayerAct (M = B * L
// tokens) for the backward, as the pre-training encoder does for its visible tokens.  The forward issues the launches of
// bvc_videomae_encode_px in the same order on the same shapes (layer_forward without the next layer's LayerNorm in the fc2 epilogue,
// as the inference context runs it), so its pooled rows equal the inference context's bit for bit.
struct bvc_cls_ctx {
    bvc_videomae_config cfg;
    Layout lay;
    int max_batch, L;
    Arena arena;
    Work w;
    Stack enc;         // num_hidden_layers LayerActs
    float *pos_enc, *pooled_pre, *mean, *rstd, *fcw, *dres;
    Shadow shadow;               // bvc_videomae_cls_shadow
    PatchFront front;
    int batch = 0;
    bool have_forward = false;
    DropState drop;              // bvc_videomae_cls_set_drop
    MixState mix;                // bvc_videomae_cls_set_mix
    EraseState erase;            // bvc_videomae_cls_set_erase
};

void bvc_videomae_cls_destroy(bvc_cls_ctx* c) {
    if (!c) return;
    free_work(c->w);
    c->arena.release();
    delete c;
}

int bvc_videomae_cls_create(const bvc_videomae_config* cfg, int max_batch, bvc_cls_ctx** out) {
    BVC_REQUIRE(cfg && out, "cls_create: null argument");
    TRY(check_config(*cfg));
    BVC_REQUIRE(max_batch >= 1, "cls_create: max_batch must be >= 1");
    const PatchGeom pg = patch_geom(*cfg);
    const size_t L = seq_len(pg), P = patch_dim(pg);
    const int D = cfg->hidden_size, I = cfg->intermediate_size, H = cfg->num_attention_heads;
    const size_t Da = (size_t)H * attn_width(D / H);
    // refuse before allocating anything: the widest operand is fc1's output, or the qkv product's when the heads are padded
    // (VideoMAE-B: 1568 x 3072 per clip, 4 GiB at 446 clips)
    TRY(refuse_operand_extent("cls_create", max_batch, L, std::max(std::max(3 * Da, (size_t)I), P), nullptr));
    bvc_cls_ctx* c = new bvc_cls_ctx();
    Making guard{[&] { bvc_videomae_cls_destroy(c); }};
    c->cfg = *cfg;
    c->lay = make_layout(*cfg);
    c->max_batch = max_batch;
    c->L = (int)L;
    const size_t M = (size_t)max_batch * L;
    TRY(c->arena.alloc(&c->pos_enc, L * D));
    TRY(c->shadow.alloc(c->arena, c->lay.e2d_w));
    TRY(c->front.alloc(c->arena, pg, M, true));
    TRY(alloc_stack(c->arena, c->enc, D, I, H, cfg->num_hidden_layers, cfg->layer_norm_eps, M, (size_t)max_batch * H * L));
    TRY(alloc_drop(c->arena, c->drop, cfg->num_hidden_layers, max_batch));
    TRY(alloc_mix(c->arena, c->mix, max_batch));
    TRY(alloc_erase(c->arena, c->erase, max_batch));
    TRY(c->arena.alloc(&c->pooled_pre, (size_t)max_batch * D));
    TRY(c->arena.alloc(&c->mean, (size_t)max_batch));
    TRY(c->arena.alloc(&c->rstd, (size_t)max_batch));
    TRY(c->arena.alloc(&c->fcw, (size_t)D));
    TRY(c->arena.alloc(&c->dres, M * D));
    TRY(alloc_work(c->arena, c->w, M * std::max((size_t)D, (size_t)c->enc.Da), M * I, (size_t)max_batch * H * L,
                   ln_bwd_workspace_floats_upto((int)M, D)));
    TRY(upload_sinusoid(c->pos_enc, c->L, D));
    guard.done = true;
    *out = c;
    return BVC_OK;
}

int bvc_videomae_cls_forward_px(bvc_cls_ctx* c, const void* pixels_any, const bvc_pixel_format* fmt, int batch, const float* params,
                                const float* fc_norm_w, const float* fc_norm_b, float fc_norm_eps, float* pooled, float* tokens,
                                void* stream) {
    BVC_REQUIRE(c && pixels_any && params && fc_norm_w && fc_norm_b && pooled, "cls_forward: null argument");
    PixelSrc pixels;
    TRY(pixel_src("cls_forward", pixels_any, fmt, c->cfg.num_channels, &pixels));
    BVC_REQUIRE(batch >= 1 && batch <= c->max_batch, "cls_forward: batch %d outside [1, %d]", batch, c->max_batch);
    hipStream_t st = (hipStream_t)stream;
    const Layout& L = c->lay;
    const int B = batch, N = c->L, M = B * N, D = c->cfg.hidden_size;
    c->have_forward = false;
    c->batch = B;
    c->w.params = params;
    c->w.wbf = c->shadow.wbf;
    c->w.drop = &c->drop;
    TRY(take_drop(c->drop, B, N, "cls_forward"));
    TRY(c->shadow.refresh(params, st));
    bool mixed = false;
    TRY(c->front.embed(pixels, c->front.idx_all, B, N, c->shadow.wbf + L.pe_w, params + L.pe_b, c->pos_enc, c->enc.act[0].x_in, D, st,
                       "cls_forward", &c->mix, &mixed, &c->erase));
    TRY(stack_forward(c->w, c->enc, L.enc, B, N, st, false));     // unchained, as the inference context runs its layers
    TRY(launch_token_mean(c->enc.x_out, B, N, D, c->pooled_pre, st));
    TRY(launch_ln_fwd(c->pooled_pre, identity_rows(), fc_norm_w, fc_norm_b, nullptr, c->mean, c->rstd, B, D, fc_norm_eps, st, pooled));
    BVC_CHECK_HIP(hipMemcpyAsync(c->fcw, fc_norm_w, (size_t)D * 4, hipMemcpyDeviceToDevice, st));
    if (tokens) BVC_CHECK_HIP(hipMemcpyAsync(tokens, c->enc.x_out, (size_t)M * D * 4, hipMemcpyDeviceToDevice, st));
    if (mixed) {
        TRY(launch_poison_on_status(pooled, (size_t)B * D, c->mix.status, st));
        if (tokens) TRY(launch_poison_on_status(tokens, (size_t)M * D, c->mix.status, st));
    }
    c->have_forward = true;
    return BVC_OK;
}

int bvc_videomae_cls_backward(bvc_cls_ctx* c, const float* dpooled, float* G, float* dfc_norm_w, float* dfc_norm_b,
                              bvc_bucket_fn on_bucket, void* user, void* stream) {
    BVC_REQUIRE(c && dpooled && G && dfc_norm_w && dfc_norm_b, "cls_backward: null argument");
    if (!c->have_forward) { set_error("cls_backward: no forward state (call bvc_videomae_cls_forward_px first; one backward per forward)"); return BVC_ERR_STATE; }
    c->have_forward = false;
    hipStream_t st = (hipStream_t)stream;
    const Layout& L = c->lay;
    const int B = c->batch, N = c->L, M = B * N, D = c->cfg.hidden_size;
    begin_backward(c->w);
    BVC_CHECK_HIP(hipMemsetAsync(G, 0, (size_t)L.e2d_w * 4, st));
    // fc_norm backward on the B pooled rows and the token-mean broadcast into the last layer's residual gradient, one pass
    Gate gtop;     // (the first bf16 copy feeds the last layer's MLP branch: gated here when that context has a gate on)
    TRY(launch_fcnorm_bwd_bcast(dpooled, c->pooled_pre, c->mean, c->rstd, c->fcw, c->dres, c->w.dyb[c->w.seq % 3], dfc_norm_w, dfc_norm_b,
                                B, N, D, st, top_gate(c->drop, gtop)));
    TRY(stack_backward(c->w, c->enc, L.enc, c->dres, G, B, N, st, on_bucket, user));
    TRY(c->front.embed_backward(c->w, M, D, G + L.pe_w, G + L.pe_b, st));
    TRY(join_both(c->w, st, on_bucket, user));
    if (on_bucket) on_bucket(0, L.enc.front().ln1w, user);
    return BVC_OK;
}

int bvc_videomae_cls_introspect(bvc_cls_ctx* c, const bvc_introspect* out, void* stream) {
    BVC_REQUIRE(c && out, "cls_introspect: null argument");
    if (!c->have_forward) { set_error("cls_introspect: no forward state (call it between bvc_videomae_cls_forward_px and its backward)"); return BVC_ERR_STATE; }
    hipStream_t st = (hipStream_t)stream;
    const int B = c->batch, N = c->L, D = c->cfg.hidden_size, H = c->enc.H, nl = c->enc.nlayers;
    const size_t slot = (size_t)B * N * D;
    if (out->hidden_states)
        for (int i = 0; i <= nl; ++i)
            BVC_CHECK_HIP(hipMemcpyAsync(out->hidden_states + (size_t)i * slot, i < nl ? c->enc.act[i].x_in : c->enc.x_out, slot * 4,
                                         hipMemcpyDeviceToDevice, st));
    if (out->attentions)
        for (int i = 0; i < nl; ++i)
            TRY(launch_attn_probs(c->enc.act[i].qkv, c->enc.act[i].lse, out->attentions + (size_t)i * B * H * N * N, B, N, H, c->enc.hdp, st,
                                  stack_sm_scale(c->enc)));
    return BVC_OK;
}

int bvc_videomae_cls_set_drop(bvc_cls_ctx* c, const bvc_branch_drop* drop, int samples, void* stream) {
    BVC_REQUIRE(c, "cls_set_drop: null context");
    return set_drop(c->drop, drop, samples, "cls_set_drop", (hipStream_t)stream);
}

int bvc_videomae_cls_set_mix(bvc_cls_ctx* c, const bvc_clip_mix* mix_dev, int samples, void* stream) {
    (void)stream;      // the table is copied by the forward that consumes it, on that forward's stream
    BVC_REQUIRE(c, "cls_set_mix: null context");
    return set_mix(c->mix, mix_dev, samples, c->max_batch, "cls_set_mix");
}

int bvc_videomae_cls_set_erase(bvc_cls_ctx* c, const bvc_erase_box* tab_dev, int samples, int boxes, uint64_t seed, uint64_t offset,
                               void* stream) {
    (void)stream;      // as for the mix: copied by the forward that consumes it
    BVC_REQUIRE(c, "cls_set_erase: null context");
    return set_erase(c->erase, tab_dev, samples, boxes, seed, offset, c->max_batch, "cls_set_erase");
}

int bvc_videomae_cls_shadow(bvc_cls_ctx* c, int valid, void** shadow_bf16, int64_t* numel) {
    BVC_REQUIRE(c, "videomae_cls_shadow: null context");
    return c->shadow.query(valid, shadow_bf16, numel);
}

int bvc_videomae_shadow(bvc_ctx* c, int valid, void** shadow_bf16, int64_t* numel) {
    BVC_REQUIRE(c, "videomae_shadow: null context");
    return c->shadow.query(valid, shadow_bf16, numel);
}

}  // extern "C"

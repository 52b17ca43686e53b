// Entry points that belong to no model: error text, options, the deterministic workspace, and the operator-level bvc_op_* wrappers
// (GEMM, attention, row kernels, optimisers, gradient norm, SimCLR and JEPA losses).  Host code only.
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include "attnpool.h"
#include "ntxent.h"
#include "proto_ce.h"
#include "xcorr.h"
#include "context.h"
#include "optim_layerwise.h"

namespace bvc {
static thread_local char g_err[1024] = "";
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
const char* last_error() { return g_err; }
}  // namespace bvc

using namespace bvc;

extern "C" {

const char* bvc_last_error(void) { return bvc::last_error(); }
const char* bvc_version(void) { return "gfx950;bvc-hip-r5"; }

int bvc_set_option(const char* name, int value) {
    BVC_REQUIRE(name != nullptr, "set_option: null name");
    if (!strcmp(name, "gemm8")) { BVC_REQUIRE(value >= -1 && value <= 1, "set_option: gemm8 takes -1 / 0 / 1"); options().gemm8 = value; }
    else if (!strcmp(name, "dw_overlap")) options().dw_overlap = value != 0;
    else if (!strcmp(name, "row_stagger")) options().row_stagger = value != 0;
    else if (!strcmp(name, "row_ln")) { BVC_REQUIRE(value >= -1 && value <= 1, "set_option: row_ln takes -1 / 0 / 1"); options().row_ln = value; }
    else if (!strcmp(name, "deterministic")) { BVC_REQUIRE(value == 0 || value == 1, "set_option: deterministic takes 0 / 1"); options().deterministic = value; }
    else if (!strcmp(name, "head_pad")) { BVC_REQUIRE(value == 0 || value == 1, "set_option: head_pad takes 0 / 1"); options().head_pad = value; }
    else if (!strcmp(name, "dec_tail")) { BVC_REQUIRE(value == 0 || value == 1, "set_option: dec_tail takes 0 / 1"); options().dec_tail = value; }
    else if (!strcmp(name, "dec_first")) { BVC_REQUIRE(value >= -1 && value <= 1, "set_option: dec_first takes -1 / 0 / 1"); options().dec_first = value; }
    else BVC_REQUIRE(false, "set_option: unknown option '%s'", name);
    return BVC_OK;
}
int bvc_get_option(const char* name) {
    if (name && !strcmp(name, "gemm8")) return options().gemm8;
    if (name && !strcmp(name, "dw_overlap")) return options().dw_overlap;
    if (name && !strcmp(name, "row_ln")) return options().row_ln;
    if (name && !strcmp(name, "row_stagger")) return options().row_stagger;
    if (name && !strcmp(name, "deterministic")) return options().deterministic;
    if (name && !strcmp(name, "head_pad")) return options().head_pad;
    if (name && !strcmp(name, "dec_tail")) return options().dec_tail;
    if (name && !strcmp(name, "dec_first")) return options().dec_first;
    bvc::set_error("get_option: unknown option '%s'", name ? name : "(null)");
    return BVC_ERR_INVALID;
}

// ------------------------------------------------------------------ operator-level entry points
int bvc_op_gemm(const bvc_gemm_desc* problems, int count, int layout, int tile_cfg, int stages, void* stream) {
    BVC_REQUIRE(problems, "op_gemm: null problems");
    BVC_REQUIRE(layout >= 0 && layout <= 2, "op_gemm: bad layout %d", layout);
    return launch_gemm(problems, count, (GemmLayout)layout, tile_cfg, (hipStream_t)stream, stages);
}
static int op_gate(const bvc_branch_drop* drop, int layer, int branch, int M, Gate* g) {
    BVC_REQUIRE(drop && layer >= 0 && layer < (1 << 22) && (branch == 0 || branch == 1), "gate: null description, or layer / branch out of range");
    BVC_REQUIRE(drop->hidden_p >= 0.f && drop->hidden_p < 1.f && drop->rows_per_sample >= 1, "gate: hidden_p outside [0, 1) or rows_per_sample < 1");
    const int samples = (M + drop->rows_per_sample - 1) / drop->rows_per_sample;
    *g = make_gate(drop->hidden_p, drop->seed, drop->offset,
                   drop->path_scale ? drop->path_scale + ((size_t)layer * 2 + branch) * samples : nullptr, drop->rows_per_sample, layer, branch);
    return BVC_OK;
}
int bvc_op_gemm_gate(const bvc_gemm_desc* problem, const bvc_branch_drop* drop, int layer, int branch, int tile_cfg, void* stream) {
    BVC_REQUIRE(problem, "op_gemm_gate: null problem");
    Gate g;
    TRY(op_gate(drop, layer, branch, problem->M, &g));
    return launch_gemm_gate(*problem, g, tile_cfg, (hipStream_t)stream);
}
int bvc_op_gemm_gate_kernel(const bvc_gemm_desc* problem, int tile_cfg, char* name, int name_cap) {
    BVC_REQUIRE(problem && name && name_cap > 0, "op_gemm_gate_kernel: null argument");
    DryRun& d = dry_run();
    d.on = true;
    d.name[0] = 0;
    const int rc = launch_gemm_gate(*problem, make_gate(0.f, 0, 0, nullptr, 1, 0, 0), tile_cfg, nullptr);
    d.on = false;
    if (rc == BVC_OK) snprintf(name, name_cap, "%s", d.name);
    return rc;
}
int bvc_op_dropout_mask(uint64_t seed, uint64_t offset, int layer, int branch, int M, int N, float p, uint8_t* out_dev, void* stream) {
    BVC_REQUIRE(out_dev && M >= 1 && N >= 1 && layer >= 0 && layer < (1 << 22) && (branch == 0 || branch == 1) && p >= 0.f && p < 1.f,
                "op_dropout_mask: bad argument");
    return launch_dropout_mask(make_gate(p, seed, offset, nullptr, 1, layer, branch), (size_t)M * N, out_dev, (hipStream_t)stream);
}
int bvc_dropout_mask_host(uint64_t seed, uint64_t offset, int layer, int branch, int M, int N, float p, uint8_t* out_host) {
    BVC_REQUIRE(out_host && M >= 1 && N >= 1 && layer >= 0 && layer < (1 << 22) && (branch == 0 || branch == 1) && p >= 0.f && p < 1.f,
                "dropout_mask_host: bad argument");
    dropout_mask_host(make_gate(p, seed, offset, nullptr, 1, layer, branch), (size_t)M * N, out_host);
    return BVC_OK;
}
int bvc_op_layernorm_bwd_gate(const void* dy, const float* x, const float* mean, const float* rstd, const float* gamma, float* dres,
                              int accumulate, void* dres_bf16, float* dgamma, float* dbeta, float* workspace, int M, int D,
                              const bvc_branch_drop* drop, int layer, int branch, void* stream) {
    Gate g;
    TRY(op_gate(drop, layer, branch, M, &g));
    return launch_ln_bwd((const bf16_t*)dy, x, identity_rows(), mean, rstd, gamma, dres, accumulate, (bf16_t*)dres_bf16, dgamma, dbeta,
                         workspace, M, D, (hipStream_t)stream, &g);
}
int bvc_op_gemm_kernel(const bvc_gemm_desc* problems, int count, int layout, int tile_cfg, int stages, char* name, int name_cap) {
    BVC_REQUIRE(problems && name && name_cap > 0, "op_gemm_kernel: null argument");
    BVC_REQUIRE(layout >= 0 && layout <= 2, "op_gemm_kernel: bad layout %d", layout);
    DryRun& d = dry_run();
    d.on = true;
    d.name[0] = 0;
    const int rc = launch_gemm(problems, count, (GemmLayout)layout, tile_cfg, nullptr, stages);
    d.on = false;
    if (rc == BVC_OK) snprintf(name, name_cap, "%s", d.name);
    return rc;
}
int64_t bvc_deterministic_workspace_bytes(void) { return (int64_t)det_scratch_bytes(); }
int bvc_deterministic_workspace_release(void) { return det_scratch_release(); }
int bvc_op_gemm_plan_dw(bvc_gemm_desc* problems, int count) {
    BVC_REQUIRE(problems && count >= 1 && count <= 4, "op_gemm_plan_dw: bad argument");
    return plan_dw(problems, count);
}
int bvc_op_gemm_num_tiles(const bvc_gemm_desc* problem, int tile_cfg) {
    if (!problem) return BVC_ERR_INVALID;
    return gemm_num_tiles(*problem, tile_cfg);
}
int bvc_op_attention_fwd(const void* qkv, void* ctx_out, float* lse, int B, int N, int H, int head_dim, void* stream) {
    BVC_REQUIRE(qkv && ctx_out && lse, "op_attention_fwd: null argument");
    return launch_attn_fwd((const bf16_t*)qkv, (bf16_t*)ctx_out, lse, B, N, H, head_dim, (hipStream_t)stream);
}
int bvc_op_attention_bwd(const void* qkv, const void* ctx_in, const void* dctx, const float* lse, float* delta, void* dqkv,
                         int B, int N, int H, int head_dim, void* stream) {
    BVC_REQUIRE(qkv && ctx_in && dctx && lse && delta && dqkv, "op_attention_bwd: null argument");
    return launch_attn_bwd((const bf16_t*)qkv, (const bf16_t*)ctx_in, (const bf16_t*)dctx, lse, delta, (bf16_t*)dqkv, B, N, H, head_dim,
                           (hipStream_t)stream);
}
int bvc_op_attention_bwd_part(const void* qkv, const void* ctx_in, const void* dctx, const float* lse, float* delta, void* dqkv,
                              int B, int N, int H, int head_dim, int part, void* stream) {
    BVC_REQUIRE(qkv && ctx_in && dctx && lse && delta && dqkv, "op_attention_bwd_part: null argument");
    BVC_REQUIRE(part == 1 || part == 2, "op_attention_bwd_part: part is 1 (dQ + delta) or 2 (dK, dV)");
    return launch_attn_bwd((const bf16_t*)qkv, (const bf16_t*)ctx_in, (const bf16_t*)dctx, lse, delta, (bf16_t*)dqkv, B, N, H, head_dim,
                           (hipStream_t)stream, 0.f, part);
}
int bvc_op_attention_width(int head_dim) {
    BVC_REQUIRE(head_dim > 0 && head_dim <= 128 && head_dim % 8 == 0, "op_attention_width: head_dim %d unsupported", head_dim);
    return attn_width(head_dim);
}
int bvc_op_attention_fwd_scaled(const void* qkv, void* ctx_out, float* lse, int B, int N, int H, int head_dim, float softmax_scale,
                                void* stream) {
    BVC_REQUIRE(qkv && ctx_out && lse && softmax_scale >= 0.f, "op_attention_fwd_scaled: bad argument");
    return launch_attn_fwd((const bf16_t*)qkv, (bf16_t*)ctx_out, lse, B, N, H, head_dim, (hipStream_t)stream, softmax_scale);
}
int bvc_op_attention_bwd_scaled(const void* qkv, const void* ctx_in, const void* dctx, const float* lse, float* delta, void* dqkv,
                                int B, int N, int H, int head_dim, float softmax_scale, void* stream) {
    BVC_REQUIRE(qkv && ctx_in && dctx && lse && delta && dqkv && softmax_scale >= 0.f, "op_attention_bwd_scaled: bad argument");
    return launch_attn_bwd((const bf16_t*)qkv, (const bf16_t*)ctx_in, (const bf16_t*)dctx, lse, delta, (bf16_t*)dqkv, B, N, H, head_dim,
                           (hipStream_t)stream, softmax_scale);
}
int bvc_op_attention_probs(const void* qkv, const float* lse, float* probs, int B, int N, int H, int head_dim, float softmax_scale,
                           void* stream) {
    BVC_REQUIRE(qkv && lse && probs && softmax_scale >= 0.f, "op_attention_probs: bad argument");
    return launch_attn_probs((const bf16_t*)qkv, lse, probs, B, N, H, head_dim, (hipStream_t)stream, softmax_scale);
}
int bvc_op_layernorm_fwd(const float* x, int rin, int rout, int roff, const float* gamma, const float* beta, void* y,
                         float* mean, float* rstd, int M, int D, float eps, void* stream) {
    BVC_REQUIRE(x && gamma && beta && y && mean && rstd, "op_layernorm_fwd: null argument");
    return launch_ln_fwd(x, RowMap{rin, rout, roff}, gamma, beta, (bf16_t*)y, mean, rstd, M, D, eps, (hipStream_t)stream);
}
int bvc_op_layernorm_bwd(const void* dy, const float* x, int rin, int rout, int roff, const float* mean, const float* rstd,
                         const float* gamma, float* dres, int accumulate, void* dres_bf16, float* dgamma, float* dbeta,
                         float* workspace, int M, int D, void* stream) {
    BVC_REQUIRE(dy && x && mean && rstd && gamma && dres && dgamma && dbeta && workspace, "op_layernorm_bwd: null argument");
    return launch_ln_bwd((const bf16_t*)dy, x, RowMap{rin, rout, roff}, mean, rstd, gamma, dres, accumulate, (bf16_t*)dres_bf16,
                         dgamma, dbeta, workspace, M, D, (hipStream_t)stream);
}
int64_t bvc_op_layernorm_bwd_workspace(int M, int D) { return (int64_t)ln_bwd_workspace_floats(M, D); }
int bvc_op_colsum_f32(const float* X, int rin, int rout, int roff, int M, int D, float* out, void* stream) {
    BVC_REQUIRE(X && out && M > 0 && D > 0, "op_colsum_f32: bad argument");
    return launch_colsum_f32(X, RowMap{rin, rout, roff}, M, D, out, (hipStream_t)stream);
}
int bvc_op_colsum_bf16(const void* X, int M, int N, int ld, float alpha, const float* alpha_dev, float* out, void* stream) {
    BVC_REQUIRE(X && out, "op_colsum_bf16: null argument");
    return launch_colsum_bf16_scaled((const bf16_t*)X, M, N, ld, alpha, alpha_dev, out, (hipStream_t)stream);
}
int bvc_op_sgd_step(float* params, float* grads, float* momentum_buf, int64_t n, float lr, float momentum, float dampening,
                    float weight_decay, int nesterov, int first_step, int maximize, const float* grad_scale,
                    const float* found_inf, int write_unscaled_grads, void* bf16_shadow, void* stream) {
    BVC_REQUIRE(params && grads && n >= 0, "op_sgd_step: bad argument");
    return launch_sgd_step(params, grads, momentum_buf, (size_t)n, lr, momentum, dampening, weight_decay, nesterov, first_step,
                           maximize, grad_scale, found_inf, write_unscaled_grads, (bf16_t*)bf16_shadow, (hipStream_t)stream);
}
int bvc_op_adam_prepare(float* state3, double lr, double beta1, double beta2, const float* found_inf, void* stream) {
    BVC_REQUIRE(state3, "op_adam_prepare: null state");
    return launch_adam_prep(state3, lr, beta1, beta2, found_inf, (hipStream_t)stream);
}
int bvc_op_adam_step(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, double lr, double beta1, double beta2,
                     double eps, double weight_decay, int decoupled, int maximize, const float* state3, const float* grad_scale,
                     const float* found_inf, int write_unscaled_grads, void* bf16_shadow, void* stream) {
    BVC_REQUIRE(params && grads && exp_avg && exp_avg_sq && state3 && n >= 0, "op_adam_step: bad argument");
    return launch_adam_step(params, grads, exp_avg, exp_avg_sq, (size_t)n, lr, beta1, beta2, eps, weight_decay, decoupled, maximize,
                            state3, grad_scale, found_inf, write_unscaled_grads, (bf16_t*)bf16_shadow, (hipStream_t)stream);
}
int bvc_op_row_ln_selected(int tokens, int width, int mlp_width, int heads) {
    if (tokens <= 0 || width <= 0 || heads <= 0 || width % heads != 0) return 0;
    Stack s;
    s.D = width; s.I = mlp_width; s.H = heads; s.nlayers = 0; s.eps = 0.f; s.x_out = nullptr;
    s.hd = width / heads; s.hdp = attn_width(s.hd); s.Da = heads * s.hdp;
    return fuse_row_ln(s, tokens) ? 1 : 0;
}
int bvc_op_dec_first_selected(int clips, int decoder_layers) {
    if (clips <= 0 || decoder_layers <= 0) return 0;
    Work w;
    Stack s;
    s.D = 384; s.I = 1536; s.H = 6; s.nlayers = decoder_layers; s.eps = 0.f; s.x_out = nullptr;
    s.hd = 64; s.hdp = attn_width(s.hd); s.Da = s.H * s.hdp;
    return layer_first_ok(w, s, clips, 1, 1) ? 1 : 0;
}
int bvc_op_sgd_step_segments(float* params, float* grads, float* momentum_buf, int64_t n, const int64_t* seg_start, const int32_t* seg_group,
                             const int32_t* blk_seg, int nseg, const bvc_sgd_groups* groups, const float* grad_scale, const float* found_inf,
                             int write_unscaled_grads, void* bf16_shadow, void* stream) {
    BVC_REQUIRE(params && grads && n >= 0, "op_sgd_step_segments: bad argument");
    return launch_sgd_step_segments(params, grads, momentum_buf, n, seg_start, seg_group, blk_seg, nseg, groups, grad_scale, found_inf,
                                    write_unscaled_grads, (bf16_t*)bf16_shadow, (hipStream_t)stream);
}
int bvc_op_adam_step_segments(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, const int64_t* seg_start,
                              const int32_t* seg_group, const int32_t* blk_seg, int nseg, const bvc_adam_groups* groups, float* state,
                              double* hyper_scratch, const float* grad_scale, const float* found_inf, int write_unscaled_grads,
                              void* bf16_shadow, void* stream) {
    BVC_REQUIRE(params && grads && exp_avg && exp_avg_sq && n >= 0, "op_adam_step_segments: bad argument");
    return launch_adam_step_segments(params, grads, exp_avg, exp_avg_sq, n, seg_start, seg_group, blk_seg, nseg, groups, state, hyper_scratch,
                                     grad_scale, found_inf, write_unscaled_grads, (bf16_t*)bf16_shadow, (hipStream_t)stream);
}
int bvc_op_sgd_step_table(float* params, float* grads, float* momentum_buf, int64_t n, const int64_t* seg_start, const int32_t* seg_group,
                          const int32_t* blk_seg, int nseg, int ngroups, const float* lr, const float* momentum, const float* dampening,
                          const float* weight_decay, const int32_t* nesterov, const int32_t* first_step, const int32_t* maximize,
                          float* group_table, const float* grad_scale, const float* found_inf, int write_unscaled_grads,
                          void* bf16_shadow, void* stream) {
    BVC_REQUIRE(params && grads && n >= 0, "op_sgd_step_table: bad argument");
    return launch_sgd_step_table(params, grads, momentum_buf, n, seg_start, seg_group, blk_seg, nseg, ngroups, lr, momentum, dampening,
                                 weight_decay, nesterov, first_step, maximize, group_table, grad_scale, found_inf, write_unscaled_grads,
                                 (bf16_t*)bf16_shadow, (hipStream_t)stream);
}
int bvc_op_adam_step_table(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, const int64_t* seg_start,
                           const int32_t* seg_group, const int32_t* blk_seg, int nseg, int ngroups, const double* lr, const double* beta1,
                           const double* beta2, const double* eps, const double* weight_decay, const int32_t* decoupled,
                           const int32_t* maximize, float* state, float* group_table, const float* grad_scale, const float* found_inf,
                           int write_unscaled_grads, void* bf16_shadow, void* stream) {
    BVC_REQUIRE(params && grads && exp_avg && exp_avg_sq && n >= 0, "op_adam_step_table: bad argument");
    return launch_adam_step_table(params, grads, exp_avg, exp_avg_sq, n, seg_start, seg_group, blk_seg, nseg, ngroups, lr, beta1, beta2, eps,
                                  weight_decay, decoupled, maximize, state, group_table, grad_scale, found_inf, write_unscaled_grads,
                                  (bf16_t*)bf16_shadow, (hipStream_t)stream);
}
int bvc_op_nonfinite_check(const float* x, int64_t n, float* found_inf, void* stream) {
    BVC_REQUIRE(x && found_inf && n >= 0, "op_nonfinite_check: bad argument");
    return launch_nonfinite_check(x, (size_t)n, found_inf, (hipStream_t)stream);
}
int bvc_op_grad_norm_item_cap(void) { return BVC_GRAD_NORM_ITEM_CAP; }
int bvc_op_grad_norm_chain(void) { return grad_norm_chain(); }
int bvc_grad_norm_items_host(const int64_t* seg_start, const int32_t* seg_group, int nseg, bvc_norm_item* items, int64_t items_cap,
                             int64_t* seg_first_item, int64_t* nitems) {
    BVC_REQUIRE(nseg >= 0 && nitems && (nseg == 0 || (seg_start && seg_group)) && (items == nullptr || items_cap >= 0),
                "grad_norm_items_host: bad argument");
    return grad_norm_items_host(seg_start, seg_group, nseg, items, items_cap, seg_first_item, nitems);
}
int bvc_op_grad_sqnorm_items(const float* x, const bvc_norm_item* items, int64_t nitems, const int64_t* seg_first_item, int nseg,
                             double* item_partial, float* seg_sq, float* total_sq, int as_norm, float* found_inf, void* stream) {
    BVC_REQUIRE(x && total_sq && nitems >= 0, "op_grad_sqnorm_items: bad argument");
    return launch_grad_sqnorm_items(x, items, nitems, seg_first_item, nseg, item_partial, seg_sq, total_sq, as_norm, found_inf,
                                    (hipStream_t)stream);
}
int bvc_op_clip_finalize(const float* sq, int nranges, float max_norm, const float* grad_scale, float* out3, void* stream) {
    BVC_REQUIRE(out3 && nranges >= 0 && (nranges == 0 || sq) && !(max_norm < 0.f) && max_norm == max_norm, "op_clip_finalize: bad argument");
    return launch_clip_finalize(sq, nranges, max_norm, grad_scale, out3, (hipStream_t)stream);
}
int bvc_op_scale_by_dev(float* x, int64_t n, const float* coef, void* stream) {
    BVC_REQUIRE(x && coef && n >= 0 && ((uintptr_t)x % 4) == 0, "op_scale_by_dev: bad argument");
    return launch_scale_by_dev(x, (size_t)n, coef, (hipStream_t)stream);
}
int bvc_op_lars_step_table(float* params, float* grads, float* momentum_buf, int64_t n, const int64_t* seg_start, const int32_t* seg_group,
                           const int32_t* blk_seg, int nseg, const bvc_norm_item* items, int64_t nitems, const int64_t* seg_first_item,
                           int ngroups, const float* lr, const float* momentum, const float* weight_decay, const float* trust_coefficient,
                           const int32_t* nesterov, const int32_t* adapt, const int32_t* maximize, float* group_table, double* item_partial,
                           float* seg_stats, const float* grad_scale, float* found_inf, int write_unscaled_grads, void* bf16_shadow,
                           void* stream) {
    BVC_REQUIRE(params && grads && n >= 0, "op_lars_step_table: bad argument");
    return launch_lars_step_table(params, grads, momentum_buf, n, seg_start, seg_group, blk_seg, nseg, items, nitems, seg_first_item, ngroups,
                                  lr, momentum, weight_decay, trust_coefficient, nesterov, adapt, maximize, group_table, item_partial,
                                  seg_stats, grad_scale, found_inf, write_unscaled_grads, (bf16_t*)bf16_shadow, (hipStream_t)stream);
}
int bvc_op_lamb_step_table(float* params, float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, const int64_t* seg_start,
                           const int32_t* seg_group, const int32_t* blk_seg, int nseg, const bvc_norm_item* items, int64_t nitems,
                           const int64_t* seg_first_item, int ngroups, const double* lr, const double* beta1, const double* beta2,
                           const double* eps, const double* weight_decay, const int32_t* adapt, const int32_t* maximize, float* state,
                           float* group_table, double* item_partial, float* seg_stats, const float* grad_scale, const float* found_inf,
                           int write_unscaled_grads, void* bf16_shadow, void* stream) {
    BVC_REQUIRE(params && grads && exp_avg && exp_avg_sq && n >= 0, "op_lamb_step_table: bad argument");
    return launch_lamb_step_table(params, grads, exp_avg, exp_avg_sq, n, seg_start, seg_group, blk_seg, nseg, items, nitems, seg_first_item,
                                  ngroups, lr, beta1, beta2, eps, weight_decay, adapt, maximize, state, group_table, item_partial, seg_stats,
                                  grad_scale, found_inf, write_unscaled_grads, (bf16_t*)bf16_shadow, (hipStream_t)stream);
}
int bvc_op_row_normalize(const float* f, void* fn_bf16, float* inv_norm, int n, int p, float eps, void* stream) {
    BVC_REQUIRE(f && fn_bf16 && inv_norm, "op_row_normalize: null argument");
    return launch_row_normalize(f, (bf16_t*)fn_bf16, inv_norm, n, p, eps, (hipStream_t)stream);
}
int bvc_op_row_normalize_bwd(const float* f, const float* inv_norm, const float* dfn, float* df, int n, int p, void* stream) {
    BVC_REQUIRE(f && inv_norm && dfn && df, "op_row_normalize_bwd: null argument");
    return launch_row_normalize_bwd(f, inv_norm, dfn, df, n, p, (hipStream_t)stream);
}
int bvc_op_nce_finalize(const float* partial, int ntiles, float inv_temperature, int64_t npos, float* loss, float* stats, void* stream) {
    BVC_REQUIRE(partial && loss && stats && ntiles > 0 && npos > 0, "op_nce_finalize: bad argument");
    return launch_nce_finalize(partial, ntiles, inv_temperature, (double)npos, loss, stats, (hipStream_t)stream);
}
int bvc_op_cast_bf16(const float* in, void* out, int64_t n, void* stream) {
    BVC_REQUIRE(in && out && n >= 0, "op_cast_bf16: bad argument");
    return launch_cast_bf16(in, (bf16_t*)out, (size_t)n, (hipStream_t)stream);
}
int bvc_op_mask_index(const uint8_t* mask, int B, int L, int nvis, int nmask, int* vis_idx, int* msk_idx, int* status, void* stream) {
    BVC_REQUIRE(mask && vis_idx && msk_idx && status, "op_mask_index: null argument");
    return launch_mask_index(mask, B, L, nvis, nmask, vis_idx, msk_idx, status, (hipStream_t)stream);
}
int bvc_op_dual_mask_index(const uint8_t* mask, const uint8_t* decode_mask, int B, int L, int nvis, int ndec, int* vis_idx, int* dec_idx,
                           int* status, void* stream) {
    BVC_REQUIRE(mask && decode_mask && vis_idx && dec_idx && status, "op_dual_mask_index: null argument");
    BVC_REQUIRE(B >= 1 && L >= 1 && nvis >= 1 && nvis < L && ndec >= 1 && ndec <= L - nvis, "op_dual_mask_index: bad counts (L %d, nvis %d, ndec %d)", L, nvis, ndec);
    return launch_dual_mask_index(mask, decode_mask, B, L, nvis, ndec, vis_idx, dec_idx, status, (hipStream_t)stream);
}
int bvc_op_dec_slot(const int* dec_idx, int* dec_slot, int B, int L, int ndec, void* stream) {
    BVC_REQUIRE(dec_idx && dec_slot && B >= 1 && L >= 1 && ndec >= 1 && ndec <= L, "op_dec_slot: bad argument");
    return launch_dec_slot(dec_idx, dec_slot, B, L, ndec, (hipStream_t)stream);
}
int bvc_op_first_reduce(const void* dqkv, const int* dec_slot, int B, int L, int Ld, int nvis, int W, float* S, void* hi_bf16, void* lo_bf16,
                        void* stream) {
    BVC_REQUIRE(dqkv && dec_slot, "op_first_reduce: null argument");
    return launch_first_reduce((const bf16_t*)dqkv, dec_slot, B, L, Ld, nvis, W, S, (bf16_t*)hi_bf16, (bf16_t*)lo_bf16, (hipStream_t)stream);
}
int bvc_op_gather_patches(const float* clip, const int* vis_idx, void* A, int B, int nvis, int T, int C, int H, int W, int ts,
                          int ps, void* stream) {
    BVC_REQUIRE(clip && vis_idx && A, "op_gather_patches: null argument");
    return launch_gather_patches(pixels_f32(clip), vis_idx, (bf16_t*)A, B, nvis, PatchGeom{T, C, H, W, ts, ps}, (hipStream_t)stream);
}
int bvc_op_gather_patches_mix(const void* clip, const bvc_pixel_format* fmt, const int* idx, void* A, const bvc_clip_mix* mix, int B, int n,
                              int T, int C, int H, int W, int ts, int ps, void* stream) {
    BVC_REQUIRE(clip && idx && A && mix, "op_gather_patches_mix: null argument");
    BVC_REQUIRE(T >= 1 && C >= 1 && H >= 1 && W >= 1 && ts >= 1 && ps >= 1 && T % ts == 0 && H % ps == 0 && W % ps == 0,
                "op_gather_patches_mix: bad geometry");
    PixelSrc px;
    TRY(pixel_src("op_gather_patches_mix", clip, fmt, C, &px));
    return launch_gather_patches_mix(px, idx, (bf16_t*)A, B, n, PatchGeom{T, C, H, W, ts, ps}, mix, (hipStream_t)stream);
}
int bvc_op_gather_patches_aug(const void* clip, const bvc_pixel_format* fmt, const int* idx, void* A, const bvc_clip_mix* mix,
                              const bvc_erase_box* erase, int boxes, uint64_t seed, uint64_t offset, int B, int n, int T, int C, int H, int W,
                              int ts, int ps, void* stream) {
    BVC_REQUIRE(clip && idx && A && erase, "op_gather_patches_aug: null argument");
    BVC_REQUIRE(boxes >= 1 && boxes <= BVC_ERASE_MAX_BOXES, "op_gather_patches_aug: %d boxes per clip outside [1, %d]", boxes, BVC_ERASE_MAX_BOXES);
    BVC_REQUIRE(T >= 1 && C >= 1 && H >= 1 && W >= 1 && ts >= 1 && ps >= 1 && T % ts == 0 && H % ps == 0 && W % ps == 0,
                "op_gather_patches_aug: bad geometry");
    PixelSrc px;
    TRY(pixel_src("op_gather_patches_aug", clip, fmt, C, &px));
    return launch_gather_patches_aug(px, idx, (bf16_t*)A, B, n, PatchGeom{T, C, H, W, ts, ps}, mix, erase_tab(erase, boxes, seed, offset),
                                     (hipStream_t)stream);
}
int bvc_op_erase_noise(uint64_t seed, uint64_t offset, int kind, int B, int T, int C, int H, int W, float* out_dev, void* stream) {
    BVC_REQUIRE(out_dev, "op_erase_noise: null argument");
    return launch_erase_noise(erase_tab(nullptr, 0, seed, offset), kind, B, T, C, H, W, out_dev, (hipStream_t)stream);
}
int bvc_op_pixel_labels(const float* clip, const int* msk_idx, float* labels, int B, int nmask, int T, int C, int H, int W, int ts,
                        int ps, int norm_pix, void* stream) {
    BVC_REQUIRE(clip && msk_idx && labels, "op_pixel_labels: null argument");
    return launch_labels(pixels_f32(clip), msk_idx, labels, B, nmask, PatchGeom{T, C, H, W, ts, ps}, norm_pix, (hipStream_t)stream);
}

// ============================================================================ JEPA operator-level entry points
int bvc_op_target_select(const float* h, const int* idx_pred, float* out, int nsets, int B, int Np, int L, int D, float eps, void* stream) {
    BVC_REQUIRE(h && idx_pred && out, "op_target_select: null argument");
    return launch_target_select(h, idx_pred, out, nsets, B, Np, L, D, eps, (hipStream_t)stream);
}
int bvc_op_smooth_l1_workspace(int64_t n) { return smooth_l1_blocks((size_t)n); }
int bvc_op_smooth_l1_fwd(const float* z, const float* h, int64_t n, float* workspace, float* loss, void* stream) {
    BVC_REQUIRE(z && h && workspace && loss && n > 0, "op_smooth_l1_fwd: bad argument");
    return launch_smooth_l1_fwd(z, h, (size_t)n, workspace, loss, (hipStream_t)stream);
}
int bvc_op_smooth_l1_bwd(const float* z, const float* h, const float* grad_loss, int64_t n, float* dz, void* stream) {
    BVC_REQUIRE(z && h && grad_loss && dz && n > 0, "op_smooth_l1_bwd: bad argument");
    return launch_smooth_l1_bwd(z, h, grad_loss, (size_t)n, dz, (hipStream_t)stream);
}
int bvc_op_ema(float* target, const float* online, int64_t n, float momentum, void* stream) {
    BVC_REQUIRE(target && online && n >= 0, "op_ema: bad argument");
    return launch_ema(target, online, (size_t)n, momentum, (hipStream_t)stream);
}

int bvc_op_token_mean(const float* x, int batch, int ntok, int dim, float* out, void* stream) {
    BVC_REQUIRE(x && out && batch > 0 && ntok > 0 && dim > 0, "op_token_mean: bad argument");
    return launch_token_mean(x, batch, ntok, dim, out, (hipStream_t)stream);
}
int bvc_op_token_mean_bwd(const float* dmean, int batch, int ntok, int dim, float* dx, void* stream) {
    BVC_REQUIRE(dmean && dx && batch > 0 && ntok > 0 && dim > 0, "op_token_mean_bwd: bad argument");
    return launch_token_mean_bwd(dmean, batch, ntok, dim, dx, (hipStream_t)stream);
}

// ============================================================================ attentive pooling (attnpool.hip)
int bvc_op_attn_pool_splits(int B, int N, int D, int R) { return attn_pool_splits(B, N, D, R); }
int64_t bvc_op_attn_pool_workspace(int B, int N, int D, int R, int splits) { return attn_pool_workspace(B, N, D, R, splits); }
int bvc_op_attn_pool_fwd(const float* x, int64_t ldx, const float* u, int B, int N, int D, int R, float eps, int splits, float* pooled,
                         float* lse, void* workspace, void* stream) {
    return launch_attn_pool_fwd(x, ldx, u, B, N, D, R, eps, splits, pooled, lse, workspace, (hipStream_t)stream);
}
int bvc_op_attn_pool_bwd(const float* x, int64_t ldx, const float* u, const float* pooled, const float* lse, const float* dpooled, int B,
                         int N, int D, int R, float eps, int splits, float* du, float* dx, int64_t lddx, void* workspace, void* stream) {
    return launch_attn_pool_bwd(x, ldx, u, pooled, lse, dpooled, B, N, D, R, eps, splits, du, dx, lddx, workspace, (hipStream_t)stream);
}

// ============================================================================ feature-correlation losses (xcorr.hip)
int bvc_op_xcorr_block_cols(int n, int p, int q) { return xcorr_block_cols(n, p, q); }
int64_t bvc_op_xcorr_workspace(int n, int p, int q, int alias, int block_cols, int backward) {
    return xcorr_workspace(n, p, q, alias, block_cols, backward);
}
int bvc_op_xcorr_fwd(const float* x, int64_t ldx, const float* y, int64_t ldy, int n, int p, int q, int norm, int ddof, float eps, float scale,
                     float diag_target, float* mean_x, float* var_x, float* mean_y, float* var_y, float* stats2, void* workspace, void* stream) {
    return launch_xcorr_fwd(x, ldx, y, ldy, n, p, q, norm, ddof, eps, scale, diag_target, mean_x, var_x, mean_y, var_y, stats2, workspace,
                            (hipStream_t)stream);
}
int bvc_op_xcorr_bwd(const float* x, int64_t ldx, const float* y, int64_t ldy, int n, int p, int q, int norm, int ddof, float eps, float scale,
                     float diag_target, const float* mean_x, const float* var_x, const float* mean_y, const float* var_y, const float* w,
                     const float* dvar_x, const float* dvar_y, int block_cols, float* dx, int64_t lddx, float* dy, int64_t lddy,
                     void* workspace, void* stream) {
    return launch_xcorr_bwd(x, ldx, y, ldy, n, p, q, norm, ddof, eps, scale, diag_target, mean_x, var_x, mean_y, var_y, w, dvar_x, dvar_y,
                            block_cols, dx, lddx, dy, lddy, workspace, (hipStream_t)stream);
}
// ============================================================================ NT-Xent / SupCon loss (ntxent.hip)
int bvc_op_ntxent_splits(int n, int p) { return ntxent_splits(n, p); }
int bvc_op_ntxent_block_rows(int n, int p) { return ntxent_block_rows(n, p); }
int64_t bvc_op_ntxent_workspace(int n, int p, int key_splits, int block_rows) { return ntxent_workspace(n, p, key_splits, block_rows); }
int bvc_op_ntxent_fwd(const float* f, int64_t ldf, const int32_t* groups, int views, int n, int p, float temperature, float eps,
                      int key_splits, float* row_loss, float* lse, int32_t* npos, float* stats2, void* workspace, void* stream) {
    return launch_ntxent_fwd(f, ldf, groups, views, n, p, temperature, eps, key_splits, row_loss, lse, npos, stats2, workspace,
                             (hipStream_t)stream);
}
int bvc_op_ntxent_bwd(const float* f, int64_t ldf, const int32_t* groups, int views, int n, int p, float temperature, float eps,
                      const float* lse, const int32_t* npos, const float* row_weight, int key_splits, int block_rows, float* df,
                      int64_t lddf, void* workspace, void* stream) {
    return launch_ntxent_bwd(f, ldf, groups, views, n, p, temperature, eps, lse, npos, row_weight, key_splits, block_rows, df, lddf,
                             workspace, (hipStream_t)stream);
}
// ============================================================================ prototype cross-entropy, DINO (proto_ce.hip)
int bvc_op_proto_ce_splits(int m, int K, int p) { return proto_ce_splits(m, K, p); }
int bvc_op_proto_ce_block(int m, int K, int p) { return proto_ce_block(m, K, p); }
int64_t bvc_op_proto_ce_workspace(int m, int K, int p, int splits, int block) { return proto_ce_workspace(m, K, p, splits, block); }
int bvc_op_proto_ce_fwd(const float* xs, int64_t ldxs, const float* vs, int64_t ldvs, const float* xt, int64_t ldxt, const float* vt,
                        int64_t ldvt, const float* center, int m, int K, int p, float tau_s, float tau_t, float eps, int splits,
                        float* row_loss, float* lse_s, float* lse_t, float* stats2, float* batch_center, void* workspace, void* stream) {
    return launch_proto_ce_fwd(xs, ldxs, vs, ldvs, xt, ldxt, vt, ldvt, center, m, K, p, tau_s, tau_t, eps, splits, row_loss, lse_s, lse_t,
                               stats2, batch_center, workspace, (hipStream_t)stream);
}
int bvc_op_proto_ce_bwd(const float* xs, int64_t ldxs, const float* vs, int64_t ldvs, const float* xt, int64_t ldxt, const float* vt,
                        int64_t ldvt, const float* center, int m, int K, int p, float tau_s, float tau_t, float eps, const float* lse_s,
                        const float* lse_t, const float* row_weight, int splits, int block, float* dxs, int64_t lddxs, float* dvs,
                        int64_t lddvs, void* workspace, void* stream) {
    return launch_proto_ce_bwd(xs, ldxs, vs, ldvs, xt, ldxt, vt, ldvt, center, m, K, p, tau_s, tau_t, eps, lse_s, lse_t, row_weight, splits,
                               block, dxs, lddxs, dvs, lddvs, workspace, (hipStream_t)stream);
}

}  // extern "C"

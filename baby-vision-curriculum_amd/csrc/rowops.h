// HBM-bound row / element kernels (internal to libbvc_hip.so).
#pragma once
#include "common.h"
#include "dropgate.h"

namespace bvc {

// logical row m -> physical row (m / rin) * rout + roff + m % rin; rin <= 0 means identity.
// Used to address "the last nmask tokens of every clip" without copying them out.
struct RowMap { int rin, rout, roff; };
static inline RowMap identity_rows() { return RowMap{0, 0, 0}; }

// clip [B][T][C][H][W]; tubes of ts frames x ps x ps pixels
struct PatchGeom { int T, C, H, W, ts, ps; };

// Where the pixels come from: f32 already normalised by the loader, or the loader's uint8 frames normalised on the fly as
// (u / 255 - mean[c]) / std[c]  - the arithmetic of ToTensor + Normalize (homeview.py:221-230), same operation order, so the
// two forms give bit-identical values while the uint8 one moves a quarter of the bytes over PCIe and out of HBM.
struct PixelSrc {
    const void* ptr;
    int is_u8;
    float mean[4], stdv[4];
};
static inline PixelSrc pixels_f32(const float* p) { return PixelSrc{p, 0, {0, 0, 0, 0}, {1, 1, 1, 1}}; }

// gamma == nullptr: no affine.  y (bf16) and/or y32 (f32) receive the result; mean / rstd may be null.
int launch_ln_fwd(const float* x, RowMap rm, const float* gamma, const float* beta, bf16_t* y, float* mean, float* rstd,
                  int M, int D, float eps, hipStream_t s, float* y32 = nullptr);
// `part` = scratch of ln_bwd_workspace_floats(M, D) floats (per-workgroup dgamma / dbeta partials)
size_t ln_bwd_workspace_floats(int M, int D);
size_t ln_bwd_workspace_floats_upto(int Mmax, int D);
int launch_ln_bwd(const bf16_t* dy, const float* x, RowMap rm, const float* mean, const float* rstd, const float* gamma,
                  float* dres, int accumulate, bf16_t* dres_bf, float* dgamma, float* dbeta, float* part, int M, int D, hipStream_t s,
                  const Gate* gate = nullptr,      // gate: dres_bf = bf16(gate .* dres) (ln_bwd_gate_kernel), dres itself ungated
                  bool compact_x = false);         // x and dres_bf are stored by logical row ([M][D]), only dres goes through rm
// dgamma[c] += sum_b part[b][0][c], dbeta[c] += sum_b part[b][1][c] over nblk partial rows of [2][D] floats (what ln_bwd and the fused
// LayerNorm-backward epilogue of gemm8.hip leave behind)
int launch_ln_param_reduce(const float* part, int nblk, int D, float* dgamma, float* dbeta, hipStream_t s);
int launch_colsum_bf16(const bf16_t* X, int M, int N, int ld, float alpha, float* out, hipStream_t s);
int launch_colsum_bf16_scaled(const bf16_t* X, int M, int N, int ld, float alpha, const float* alpha_dev, float* out, hipStream_t s);
int launch_colsum_f32(const float* X, RowMap rm, int M, int D, float* out, hipStream_t s);
int launch_token_mean(const float* x, int B, int N, int D, float* out, hipStream_t s);
int launch_token_mean_bwd(const float* dmean, int B, int N, int D, float* dx, hipStream_t s);
// backward of y = LayerNorm(p) over B pooled rows p = token_mean(x) (saved mean / rstd of p), in one launch and a fixed order:
// dgamma / dbeta (written, not accumulated) and, unless dres is nullptr, d/dx broadcast to all N token rows of each clip as f32
// dres [B*N][D] and its bf16 copy dres_bf
int launch_fcnorm_bwd_bcast(const float* dy, const float* p, const float* mean, const float* rstd, const float* gamma, float* dres,
                            bf16_t* dres_bf, float* dgamma, float* dbeta, int B, int N, int D, hipStream_t s, const Gate* gate = nullptr);
// out[e] = 1 where element e of the gate's element mask is kept (n = M * N elements, row-major), on the device and on the host
int launch_dropout_mask(const Gate& gate, size_t n, uint8_t* out, hipStream_t s);
void dropout_mask_host(const Gate& gate, size_t n, uint8_t* out);
int launch_cast_bf16(const float* in, bf16_t* out, size_t n, hipStream_t s);
int launch_gather_rows_bf16(const float* in, RowMap rm, bf16_t* out, int M, int D, hipStream_t s);
int launch_mask_index(const uint8_t* mask, int B, int L, int nvis, int nmask, int* vis_idx, int* msk_idx, int* status, hipStream_t s);
// mask + decode mask (a subset of the mask) -> visible list and the list of decoded masked tokens, both in ascending token order
int launch_dual_mask_index(const uint8_t* mask, const uint8_t* decode, int B, int L, int nvis, int ndec, int* vis_idx, int* dec_idx,
                           int* status, hipStream_t s);
int launch_gather_patches(PixelSrc clip, const int* vis_idx, bf16_t* A, int B, int nvis, PatchGeom pg, hipStream_t s);
// the same with clip b composed with clip mix[b].partner on the way (Mixup / CutMix, bvc_clip_mix in include/bvc.h); mix is a device
// table of B entries; entries out of range are clamped and raise bit 0 of *status (status may be null: clamped silently)
typedef bvc_clip_mix ClipMix;
int launch_gather_patches_mix(PixelSrc clip, const int* idx, bf16_t* A, int B, int n, PatchGeom pg, const ClipMix* mix, hipStream_t s,
                              int* status = nullptr);
// the same with every clip erased first (random erasing, bvc_erase_box in include/bvc.h): a device table of [B][boxes] entries and
// the generator's key and call offset; mix may be null (no mix).  Entries out of range are clamped and raise bit 0 of *status
typedef bvc_erase_box EraseBox;
struct EraseTab {
    const EraseBox* tab;
    int boxes;
    uint32_t key0, key1, off0, off1;
};
inline EraseTab erase_tab(const EraseBox* tab, int boxes, uint64_t seed, uint64_t offset) {
    return EraseTab{tab, boxes, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)offset, (uint32_t)(offset >> 32)};
}
int launch_gather_patches_aug(PixelSrc clip, const int* idx, bf16_t* A, int B, int n, PatchGeom pg, const ClipMix* mix, EraseTab er,
                              hipStream_t s, int* status = nullptr);
// the values that kernel writes: kind 0 the pixel noise of a batch [B][T][C][H][W], kind 1 the colours [B][T][4][4] (er.tab unused)
int launch_erase_noise(EraseTab er, int kind, int B, int T, int C, int H, int W, float* out, hipStream_t s);
// x[0 .. count) = NaN when bit 0 of *status is set (the device-side report of a failed input check; no host sync)
int launch_poison_on_status(float* x, size_t count, const int* status, hipStream_t s);
// dec_idx [B][ndec]: the tokens the decoder reconstructs (every masked token, or the decoded subset), ascending per clip;
// Ld = nvis + ndec: the decoder's rows per clip
int launch_labels(PixelSrc clip, const int* dec_idx, float* labels, int B, int ndec, PatchGeom pg, int norm_pix, hipStream_t s);
int launch_fill_masked(float* xfull, const float* mask_token, const float* pos, const int* dec_idx, int B, int Ld, int nvis,
                       int ndec, int D, hipStream_t s);
// The first decoder layer by position (stack.h LayerFirst):
// dec_slot [B][L] = the slot of position p among clip b's decoded rows (dec_idx [B][ndec]), -1 where the clip does not decode p
int launch_dec_slot(const int* dec_idx, int* dec_slot, int B, int L, int ndec, hipStream_t s);
// full-layout qkv (bf16, W columns) from the compact visible rows and the table rows t2[dec_idx]; the f32 mask rows of x_full from t0[dec_idx]
int launch_first_assemble(const bf16_t* qkv_vis, const bf16_t* t2, const float* t0, const int* dec_idx, bf16_t* qkv, float* xfull, int B,
                          int nvis, int ndec, int W, int D, hipStream_t s);
// S[p][:] = sum over clips, ascending, of dqkv[b][nvis + dec_slot[b][p]][:] in f32 (no atomics, the same bits on every run); outputs S
// (f32 [L][W]) and / or its bf16 pair hi + lo
int launch_first_reduce(const bf16_t* dqkv, const int* dec_slot, int B, int L, int Ld, int nvis, int W, float* S, bf16_t* hi, bf16_t* lo,
                        hipStream_t s);
int launch_gather_rows_copy_bf16(const bf16_t* in, RowMap rm, bf16_t* out, int M, int W, hipStream_t s);
// hi + lo = a + b (b may be null) as a bf16 pair, n elements each: hi = bf16(a + b), lo = bf16(a + b - hi)
int launch_pair_split(const float* a, const float* b, bf16_t* hi, bf16_t* lo, size_t n, hipStream_t s);
int launch_sgd_step(float* p, float* g, float* buf, size_t n, float lr, float momentum, float dampening, float wd, int nesterov,
                    int first, int maximize, const float* grad_scale, const float* found_inf, int write_grad, bf16_t* shadow,
                    hipStream_t s);
int launch_adam_prep(float* state, double lr, double beta1, double beta2, const float* found_inf, hipStream_t s);
int launch_adam_step(float* p, float* g, float* m, float* v, size_t n, double lr, double beta1, double beta2, double eps, double wd,
                     int decoupled, int maximize, const float* state, const float* grad_scale, const float* found_inf, int write_grad,
                     bf16_t* shadow, hipStream_t s);
int launch_sgd_step_segments(float* p, float* g, float* buf, int64_t n, const int64_t* seg_start, const int* seg_group, const int* blk_seg,
                             int nseg, const bvc_sgd_groups* groups, const float* grad_scale, const float* found_inf, int write_grad,
                             bf16_t* shadow, hipStream_t s);
int launch_adam_step_segments(float* p, float* g, float* m, float* v, int64_t n, const int64_t* seg_start, const int* seg_group,
                              const int* blk_seg, int nseg, const bvc_adam_groups* groups, float* state, double* hyper_dev,
                              const float* grad_scale, const float* found_inf, int write_grad, bf16_t* shadow, hipStream_t s);
// the same with the groups' hyper-parameters in a device table (table: f32 [8 ngroups], written inside the call), any number of groups
int launch_sgd_step_table(float* p, float* g, float* buf, int64_t n, const int64_t* seg_start, const int* seg_group, const int* blk_seg,
                          int nseg, int ngroups, const float* lr, const float* momentum, const float* dampening, const float* wd,
                          const int* nesterov, const int* first_step, const int* maximize, float* table, const float* grad_scale,
                          const float* found_inf, int write_grad, bf16_t* shadow, hipStream_t s);
int launch_adam_step_table(float* p, float* g, float* m, float* v, int64_t n, const int64_t* seg_start, const int* seg_group,
                           const int* blk_seg, int nseg, int ngroups, const double* lr, const double* beta1, const double* beta2,
                           const double* eps, const double* wd, const int* decoupled, const int* maximize, float* state, float* table,
                           const float* grad_scale, const float* found_inf, int write_grad, bf16_t* shadow, hipStream_t s);
int launch_pad_heads(const bf16_t* wqkv, const float* bqkv, const bf16_t* wo, bf16_t* wqkv_p, float* bqkv_p, bf16_t* wo_p, int D, int H,
                     int hd, int hdp, hipStream_t s);
int launch_unpad_head_grads(const float* gwqkv_p, const float* gbqkv_p, const float* gwo_p, float* gwqkv, float* gbqkv, float* gwo, int D,
                            int H, int hd, int hdp, hipStream_t s);
int launch_nonfinite_check(const float* x, size_t n, float* found_inf, hipStream_t s);
// gradient norms for clipping (include/bvc.h, "gradient-norm clipping"): the host work list, the item kernel + fixed-order reduce
// (one launch pair), the clip values on the device, x *= *coef
int grad_norm_chain();
int grad_norm_items_host(const int64_t* seg_start, const int32_t* seg_group, int nseg, bvc_norm_item* items, int64_t items_cap,
                         int64_t* seg_first_item, int64_t* nitems);
int launch_grad_sqnorm_items(const float* x, const bvc_norm_item* items, int64_t nitems, const int64_t* seg_first_item, int nseg,
                             double* item_partial, float* seg_sq, float* total_sq, int as_norm, float* found_inf, hipStream_t s);
int launch_clip_finalize(const float* sq, int nranges, float max_norm, const float* grad_scale, float* out3, hipStream_t s);
int launch_scale_by_dev(float* x, size_t n, const float* coef, hipStream_t s);
int launch_row_normalize(const float* f, bf16_t* fn, float* inv, int n, int p, float eps, hipStream_t s);
int launch_row_normalize_bwd(const float* f, const float* inv, const float* dfn, float* df, int n, int p, hipStream_t s);
int launch_nce_finalize(const float* partial, int ntiles, float inv_t, double npos, float* loss, float* stats, hipStream_t s);
int launch_target_select(const float* h, const int* idx, float* out, int nsets, int B, int Np, int L, int D, float eps, hipStream_t s);
int launch_pred_assemble(const float* xe, const float* mask_token, const float* pos, const int* idx_pred, float* X, int nsets, int B,
                         int Nc, int Np, int D, hipStream_t s);
int launch_pred_ctx_grad(const float* dX, bf16_t* dxe, int nsets, int B, int Nc, int Np, int D, hipStream_t s);
int smooth_l1_blocks(size_t n);
int launch_smooth_l1_fwd(const float* z, const float* h, size_t n, float* partial, float* loss, hipStream_t s);
int launch_smooth_l1_bwd(const float* z, const float* h, const float* gout, size_t n, float* dz, hipStream_t s);
int launch_ema(float* k, const float* q, size_t n, float m, hipStream_t s);
int launch_iota_mod(int* idx, int n, int L, hipStream_t s);
int launch_loss_finalize(const float* partial, int n, double count, const int* status, float* loss, hipStream_t s);

}  // namespace bvc

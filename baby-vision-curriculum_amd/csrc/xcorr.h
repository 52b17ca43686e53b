// Feature cross-correlation with a reduced epilogue over f32 columns (csrc/xcorr.hip): Barlow Twins, VICReg's covariance term, linear CKA.
#pragma once
#include "common.h"

namespace bvc {

constexpr int kXcMaxN = 32768;                       // rows (the contraction)
constexpr int kXcMaxP = 8192;                        // columns of either operand
constexpr int64_t kXcGBlockBytes = 128ll << 20;      // cap of the backward's G block [block_cols][width of the other operand] f32

int xcorr_block_cols(int n, int p, int q);
int64_t xcorr_workspace(int n, int p, int q, int alias, int block_cols, int backward);
int launch_xcorr_fwd(const float* x, int64_t ldx, const float* y, int64_t ldy, int n, int p, int q, int norm, int ddof, float eps, float scale,
                     float diag_target, float* mean_x, float* var_x, float* mean_y, float* var_y, float* stats2, void* workspace, hipStream_t s);
int launch_xcorr_bwd(const float* x, int64_t ldx, const float* y, int64_t ldy, int n, int p, int q, int norm, int ddof, float eps, float scale,
                     float diag_target, const float* mean_x, const float* var_x, const float* mean_y, const float* var_y, const float* w,
                     const float* dvar_x, const float* dvar_y, int block_cols, float* dx, int64_t lddx, float* dy, int64_t lddy,
                     void* workspace, hipStream_t s);

}  // namespace bvc

// Layer-wise trust ratios: the LARS and LAMB launch sequences over a segment table (internal to libbvc_hip.so; include/bvc.h,
// "Layer-wise trust ratios", describes the sequence and every caller-owned buffer).
#pragma once
#include "common.h"

namespace bvc {

int launch_lars_step_table(float* p, float* g, float* buf, int64_t n, const int64_t* seg_start, const int* seg_group, const int* blk_seg,
                           int nseg, const bvc_norm_item* items, int64_t nitems, const int64_t* seg_first_item, int ngroups,
                           const float* lr, const float* momentum, const float* wd, const float* trust, const int* nesterov,
                           const int* adapt, const int* maximize, float* table, double* item_partial, float* seg_stats,
                           const float* grad_scale, float* found_inf, int write_grad, bf16_t* shadow, hipStream_t s);
int launch_lamb_step_table(float* p, float* g, float* m, float* v, int64_t n, const int64_t* seg_start, const int* seg_group,
                           const int* blk_seg, int nseg, const bvc_norm_item* items, int64_t nitems, const int64_t* seg_first_item,
                           int ngroups, const double* lr, const double* beta1, const double* beta2, const double* eps, const double* wd,
                           const int* adapt, const int* maximize, float* state, float* table, double* item_partial, float* seg_stats,
                           const float* grad_scale, const float* found_inf, int write_grad, bf16_t* shadow, hipStream_t s);

}  // namespace bvc

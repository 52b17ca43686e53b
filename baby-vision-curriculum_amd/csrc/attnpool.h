// Attentive pooling (csrc/attnpool.hip): softmax-pooling of standardised token rows by R learned queries, forward and backward.
#pragma once
#include "common.h"

namespace bvc {
// what splits = 0 resolves to for this shape; -1 (and bvc_last_error) for a shape the kernels refuse
int attn_pool_splits(int B, int N, int D, int R);
// bytes of workspace the forward and the backward need for this shape and split count (0 = the library's choice); -1 when refused
int64_t attn_pool_workspace(int B, int N, int D, int R, int splits);
int launch_attn_pool_fwd(const float* x, int64_t ldx, const float* u, int B, int N, int D, int R, float eps, int splits, float* pooled,
                         float* lse, void* workspace, hipStream_t s);
int launch_attn_pool_bwd(const float* x, int64_t ldx, const float* u, const float* pooled, const float* lse, const float* dpooled, int B,
                         int N, int D, int R, float eps, int splits, float* du, float* dx, int64_t lddx, void* workspace, hipStream_t s);
}  // namespace bvc

// Attention launchers (internal to libbvc_hip.so); head_dim 32, 64, 80, 88, 96 or 128 (D = head_dim * H; 80 / 88 in place).
// softmax_scale = 0 means head_dim^-1/2; a caller that zero-pads a narrower head (JEPA ViT-L predictor: 24 -> 32) passes
// the scale of the TRUE head width - the padded lanes contribute nothing to q.k, the context or any gradient (ViT-H / ViT-g
// under bvc_set_option("head_pad", 1): 80 / 88 -> 96).
#pragma once
#include "common.h"

namespace bvc {
// qkv bf16 [B*N][3D] -> ctx bf16 [B*N][D], lse f32 [B*H][N] (log2 units)
int launch_attn_fwd(const bf16_t* qkv, bf16_t* ctx, float* lse, int B, int N, int H, int head_dim, hipStream_t stream,
                    float softmax_scale = 0.f);
// dctx bf16 [B*N][D] (+ saved qkv, ctx, lse) -> dqkv bf16 [B*N][3D]; delta f32 [B*H][N] is scratch
int launch_attn_bwd(const bf16_t* qkv, const bf16_t* ctx, const bf16_t* dctx, const float* lse, float* delta,
                    bf16_t* dqkv, int B, int N, int H, int head_dim, hipStream_t stream, float softmax_scale = 0.f, int parts = 3);
// parts: bit 0 = the dQ kernel (also writes delta = rowsum(dO * O)), bit 1 = the dK / dV kernel (reads delta); 3 = the backward
// qkv + the lse a forward left -> probs f32 [B][H][N][N] = softmax(q k^T scale), row = query, column = key (attention_probs.hip)
int launch_attn_probs(const bf16_t* qkv, const float* lse, float* probs, int B, int N, int H, int head_dim, hipStream_t stream,
                      float softmax_scale = 0.f);
// Query window: the queries are rows q_off .. q_off + Nq - 1 of every clip, the keys all N rows.  Q is read (dQ written) at the physical
// rows of the full qkv / dqkv; ctx, dctx, lse and delta are compact - [B*Nq][D] and [B*H][Nq].  The backward takes a window that ends
// with the clip (q_off + Nq == N) and writes exact zeros into the q columns of the rows in front of it; dK / dV cover all N rows.
bool attn_window_ok(int head_dim);
int launch_attn_fwd_win(const bf16_t* qkv, bf16_t* ctx, float* lse, int B, int N, int H, int head_dim, int q_off, int Nq, hipStream_t stream,
                        float softmax_scale = 0.f);
int launch_attn_bwd_win(const bf16_t* qkv, const bf16_t* ctx, const bf16_t* dctx, const float* lse, float* delta, bf16_t* dqkv, int B, int N,
                        int H, int head_dim, int q_off, int Nq, hipStream_t stream, float softmax_scale = 0.f);
}  // namespace bvc

// Attentive pooling: R <= 16 learned queries U [R][D] softmax-pool the STANDARDISED token rows of each clip,
//     xh_j = (x_j - mean_j) * rstd_j,   s_jr = xh_j . U_r,   p_jr = softmax over j,   pooled_r = sum_j p_jr xh_j,
// which is all of an attentive probe's cross-attention block that touches [B][N][D] (bvc/attentive.py folds LayerNorm's affine, the
// K / V projections and the query into U and into [B][D] algebra).  One streaming pass over x forward, one backward.
//
// Layout.  One workgroup (256 threads = 4 waves) owns one clip and one contiguous range of its tokens (range s of `splits`:
// tokens [s N / splits, (s + 1) N / splits), possibly empty) and walks it in tiles of 16 tokens:
//   stage    wave w standardises token slots w, w + 4, w + 8, w + 12 (float4 loads, the row in registers, mean then centred variance,
//            xor-butterfly sums) and stores xh into the LDS image xs [16][D + 8]; up to D = 1024 the rows of the NEXT tile are loaded
//            into registers right after, so that their latency hides behind this tile's products;
//   scores   S [16 tokens][16 queries] = xs . U^T on v_mfma_f32_16x16x4_f32; wave w sums over the 16-column chunks w, w + 4, ..,
//            the four partial tiles meet in LDS and every wave adds them in the order 0, 1, 2, 3;
//   softmax  lane (r = lane & 15, kk = lane >> 4) holds the four tokens ap_slot(kk, 0 .. 3) of query r: running max and sum per r,
//            identical in the four waves;
//   update   pooled^T [column][r] += xs^T . P on the same MFMA: wave w owns the 16-column blocks w, w + 4, .., one f32x4 accumulator
//            each (D / 64 of them), rescaled by exp(m_old - m_new) first.  The probabilities are the B operand straight from the
//            softmax registers; xs is the A operand.
// MFMA row i of the score tile is token slot ap_slot(i >> 2, i & 3), a permutation chosen so that the b128 operand reads of the
// scores and the b32 operand reads of the update both spread over all LDS banks with the 8-float row padding.
// Exact-f32 MFMA, not packed VALU: the two products are 16 x 16 x D and D x 16 x 16 per tile, the MFMA takes ONE register per operand
// and leaves the VALU to the standardisation and the softmax; at R = 12 .. 16 flop/byte the packed-VALU form would sit at its peak.
// U (and dpooled in the backward) are read from global memory per tile: 64 KiB at most, L2-resident, and an LDS copy beside xs
// would halve the workgroups per CU.
// exp is exp2f of the difference times log2 e: the library form of v_exp_f32, which keeps results below 2^-126 (the bare instruction
// flushes them, and a token at probability 1e-39 still owns a dx row of that size).
// The split partials (max, sum, un-normalised pooled) go to the workspace and ap_combine_kernel merges them in split order; the
// backward's per-workgroup dU partials are summed by ap_du_reduce_kernel in (clip, split) order.  No atomics anywhere: the same bits
// on every run, and a clip's results do not depend on the other clips.
#include "attnpool.h"

#include <math.h>

namespace bvc {
namespace {

constexpr int kApThreads = 256;
constexpr int kApTile = 16;          // tokens per tile = rows of one MFMA
constexpr int kApMaxR = 16;
constexpr int kApPad = 8;            // floats of padding per LDS row
constexpr int kApMaxSplits = 256;
constexpr int kApLdsLimit = 160 * 1024;
constexpr float kApLog2e = 1.4426950408889634f;

// token slot of MFMA row 4 kk + t
__device__ __forceinline__ int ap_slot(int kk, int t) { return (kk & 1) * 2 + (kk >> 1) * 8 + (t & 1) + 4 * (t >> 1); }

__device__ __forceinline__ f32x4 ap_mfma(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

struct ApArgs {
    const float* x;
    const float* u;
    int64_t ldx;
    int B, N, D, R, splits, tile_tok;
    float eps;
    float* part;             // [B][splits][R][D]: forward un-normalised pooled, backward dU partials
    float* ml;               // [B][splits][R][2]: forward (max, sum)
    const float* pooled;     // backward
    const float* lse;
    const float* dpooled;
    float* dx;
    int64_t lddx;
};

// Rows of one tile in registers: wave w holds token slots w + 4 (i0 + g), g < G, lane l the float4 columns l, l + 64, ..
template <int NV4, int G>
__device__ __forceinline__ void ap_load_rows(float4 (&v)[G][NV4], const float* xrow0, int64_t ldx, int ntok, int nq, int wave, int lane,
                                             int i0) {
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int slot = wave + 4 * (i0 + g);
        const bool live = slot < ntok;
#pragma unroll
        for (int j = 0; j < NV4; ++j) {
            const int q = lane + 64 * j;
            v[g][j] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (live && q < nq) v[g][j] = *reinterpret_cast<const float4*>(xrow0 + (int64_t)slot * ldx + 4 * q);
        }
    }
}

// Standardise those rows into xs (slots >= tile_tok are skipped, rows beyond the tile's tokens are zero rows).  The G rows advance
// together so that their butterflies overlap.
template <int NV4, int G>
__device__ __forceinline__ void ap_norm_rows(float4 (&v)[G][NV4], int tile_tok, int D, float eps, float* xs, int LD, float* rstd_s, int wave,
                                             int lane, int i0) {
    const int nq = D >> 2;
    const float fD = (float)D;
    float sum[G], sq[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        sum[g] = 0.f;
#pragma unroll
        for (int j = 0; j < NV4; ++j) sum[g] += (v[g][j].x + v[g][j].y) + (v[g][j].z + v[g][j].w);
    }
#pragma unroll
    for (int g = 0; g < G; ++g) sum[g] = wave_sum(sum[g]) / fD;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const float mean = sum[g];
        sq[g] = 0.f;
#pragma unroll
        for (int j = 0; j < NV4; ++j) {
            if (lane + 64 * j < nq) {
                v[g][j].x -= mean; v[g][j].y -= mean; v[g][j].z -= mean; v[g][j].w -= mean;
                sq[g] = fmaf(v[g][j].x, v[g][j].x, sq[g]); sq[g] = fmaf(v[g][j].y, v[g][j].y, sq[g]);
                sq[g] = fmaf(v[g][j].z, v[g][j].z, sq[g]); sq[g] = fmaf(v[g][j].w, v[g][j].w, sq[g]);
            }
        }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) sq[g] = 1.0f / sqrtf(wave_sum(sq[g]) / fD + eps);
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const int slot = wave + 4 * (i0 + g);
        if (slot >= tile_tok) continue;      // wave-uniform
        const float rstd = sq[g];
        if (rstd_s && lane == 0) rstd_s[slot] = rstd;
#pragma unroll
        for (int j = 0; j < NV4; ++j) {
            const int q = lane + 64 * j;
            if (q < nq)
                *reinterpret_cast<float4*>(xs + slot * LD + 4 * q) =
                    make_float4(v[g][j].x * rstd, v[g][j].y * rstd, v[g][j].z * rstd, v[g][j].w * rstd);
        }
    }
}

// One tile into xs.  PF (all four rows of a wave fit in registers): the rows were loaded ahead into `pf`; otherwise two rows at a time.
template <int NV4, bool PF>
__device__ __forceinline__ void ap_stage(float4 (&pf)[PF ? 4 : 1][NV4], const float* xrow0, int64_t ldx, int ntok, int tile_tok, int D, float eps,
                                         float* xs, int LD, float* rstd_s, int wave, int lane) {
    if constexpr (PF) {
        ap_norm_rows<NV4, 4>(pf, tile_tok, D, eps, xs, LD, rstd_s, wave, lane, 0);
    } else {
#pragma unroll
        for (int i0 = 0; i0 < 4; i0 += 2) {
            float4 v[2][NV4];
            ap_load_rows<NV4, 2>(v, xrow0, ldx, ntok, D >> 2, wave, lane, i0);
            ap_norm_rows<NV4, 2>(v, tile_tok, D, eps, xs, LD, rstd_s, wave, lane, i0);
        }
    }
}

// This wave's share of xs . U^T (and xs . G^T when TWO) into the partial tiles sp (gp): [wave][MFMA row][query].
template <int NBT, bool TWO>
__device__ __forceinline__ void ap_scores(const float* xs, int LD, int tile_tok, const float* u, const float* g, int R, int D, int nb,
                                          float* sp, float* gp, int wave, int lane) {
    const int i = lane & 15, kk = lane >> 4;
    const int slot = ap_slot(i >> 2, i & 3);
    const bool arow = slot < tile_tok, brow = i < R;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0, g0 = a0, g1 = a0;
#pragma unroll
    for (int b = 0; b < NBT; ++b) {
        if (b < nb) {
            const int c = 16 * (wave + 4 * b) + 4 * kk;
            const float4 av = arow ? *reinterpret_cast<const float4*>(xs + slot * LD + c) : zero;
            const float4 uv = brow ? *reinterpret_cast<const float4*>(u + (size_t)i * D + c) : zero;
            a0 = ap_mfma(av.x, uv.x, a0);
            a1 = ap_mfma(av.y, uv.y, a1);
            a0 = ap_mfma(av.z, uv.z, a0);
            a1 = ap_mfma(av.w, uv.w, a1);
            if (TWO) {
                const float4 gv = brow ? *reinterpret_cast<const float4*>(g + (size_t)i * D + c) : zero;
                g0 = ap_mfma(av.x, gv.x, g0);
                g1 = ap_mfma(av.y, gv.y, g1);
                g0 = ap_mfma(av.z, gv.z, g0);
                g1 = ap_mfma(av.w, gv.w, g1);
            }
        }
    }
    a0 += a1;
#pragma unroll
    for (int e = 0; e < 4; ++e) sp[(wave * 16 + 4 * kk + e) * 16 + i] = a0[e];
    if (TWO) {
        g0 += g1;
#pragma unroll
        for (int e = 0; e < 4; ++e) gp[(wave * 16 + 4 * kk + e) * 16 + i] = g0[e];
    }
}

// acc^T [column][query] += xs^T . W for this wave's column blocks; W = w[0 .. 3] of lane (query lane & 15, tokens ap_slot(kk, t))
template <int NBT>
__device__ __forceinline__ void ap_update(const float* xs, int LD, int tile_tok, const float (&w)[4], int nb, f32x4 (&acc)[NBT], int wave,
                                          int lane) {
    const int i = lane & 15, kk = lane >> 4;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int slot = ap_slot(kk, t);
        const bool arow = slot < tile_tok;
#pragma unroll
        for (int b = 0; b < NBT; ++b) {
            if (b < nb) {
                const float av = arow ? xs[slot * LD + 16 * (wave + 4 * b) + i] : 0.f;
                acc[b] = ap_mfma(av, w[t], acc[b]);
            }
        }
    }
}

// acc^T of lane: columns 16 (wave + 4 b) + 4 (lane >> 4) + 0 .. 3 of query lane & 15 -> out [R][D]
template <int NBT>
__device__ __forceinline__ void ap_store_acc(const f32x4 (&acc)[NBT], float* out, int R, int D, int nb, int wave, int lane) {
    const int i = lane & 15, kk = lane >> 4;
    if (i >= R) return;
#pragma unroll
    for (int b = 0; b < NBT; ++b)
        if (b < nb)
            *reinterpret_cast<float4*>(out + (size_t)i * D + 16 * (wave + 4 * b) + 4 * kk) = make_float4(acc[b][0], acc[b][1], acc[b][2], acc[b][3]);
}

// waves per SIMD the LDS image leaves room for (a register budget for the compiler, not a requirement of the code)
constexpr int ap_fwd_waves(int nbt) { return nbt <= 12 ? 3 : nbt <= 16 ? 2 : 1; }
constexpr int ap_bwd_waves(int nbt, bool two_images) { return two_images ? (nbt <= 8 ? 2 : 1) : (nbt <= 16 ? 2 : 1); }

template <int NBT>
__global__ __launch_bounds__(kApThreads, ap_fwd_waves(NBT)) void ap_fwd_kernel(ApArgs a) {
    extern __shared__ float4 ap_lds4[];
    float* lds = reinterpret_cast<float*>(ap_lds4);
    const int D = a.D, R = a.R, LD = D + kApPad, nb = D >> 6;
    float* xs = lds;
    float* sp = xs + kApTile * LD;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = blockIdx.x / a.splits, sidx = blockIdx.x % a.splits;
    const int beg = (int)((int64_t)sidx * a.N / a.splits), end = (int)((int64_t)(sidx + 1) * a.N / a.splits);
    const float* xb = a.x + (int64_t)b * a.N * a.ldx;
    const int i = lane & 15, kk = lane >> 4;

    float m = -INFINITY, l = 0.f;
    f32x4 acc[NBT];
#pragma unroll
    for (int q = 0; q < NBT; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};

    // the next tile's rows are loaded into registers while this tile is computed (up to D = 1024, where a wave's four rows fit)
    constexpr bool PF = NBT <= 16;
    float4 pf[PF ? 4 : 1][NBT / 4];
    if (PF && beg < end) ap_load_rows<NBT / 4, PF ? 4 : 1>(pf, xb + (int64_t)beg * a.ldx, a.ldx, min(kApTile, end - beg), D >> 2, wave, lane, 0);
#pragma unroll 1
    for (int tok0 = beg; tok0 < end; tok0 += kApTile) {
        const int ntok = min(kApTile, end - tok0);
        ap_stage<NBT / 4, PF>(pf, xb + (int64_t)tok0 * a.ldx, a.ldx, ntok, kApTile, D, a.eps, xs, LD, nullptr, wave, lane);
        __syncthreads();
        if (PF && tok0 + kApTile < end)
            ap_load_rows<NBT / 4, PF ? 4 : 1>(pf, xb + (int64_t)(tok0 + kApTile) * a.ldx, a.ldx, min(kApTile, end - tok0 - kApTile), D >> 2, wave, lane, 0);
        ap_scores<NBT, false>(xs, LD, kApTile, a.u, nullptr, R, D, nb, sp, nullptr, wave, lane);
        __syncthreads();
        float s[4], p[4];
        float mt = -INFINITY;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int row = 4 * kk + t;
            s[t] = ((sp[row * 16 + i] + sp[(16 + row) * 16 + i]) + sp[(32 + row) * 16 + i]) + sp[(48 + row) * 16 + i];
            if (ap_slot(kk, t) < ntok) mt = fmaxf(mt, s[t]);
        }
        mt = fmaxf(mt, __shfl_xor(mt, 16, 64));
        mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
        const float mn = fmaxf(m, mt);
        const float alpha = exp2f((m - mn) * kApLog2e);
#pragma unroll
        for (int t = 0; t < 4; ++t) p[t] = ap_slot(kk, t) < ntok ? exp2f((s[t] - mn) * kApLog2e) : 0.f;
        float ps = (p[0] + p[1]) + (p[2] + p[3]);
        ps += __shfl_xor(ps, 16, 64);
        ps += __shfl_xor(ps, 32, 64);
        l = fmaf(l, alpha, ps);
        m = mn;
#pragma unroll
        for (int q = 0; q < NBT; ++q) acc[q] *= alpha;
        ap_update<NBT>(xs, LD, kApTile, p, nb, acc, wave, lane);
        __syncthreads();
    }
    const size_t slot = (size_t)b * a.splits + sidx;
    ap_store_acc<NBT>(acc, a.part + slot * R * D, R, D, nb, wave, lane);
    if (wave == 0 && kk == 0 && i < R) {
        a.ml[(slot * R + i) * 2] = m;
        a.ml[(slot * R + i) * 2 + 1] = l;
    }
}

// pooled [b][r][:] = sum_s w_s part_s / L,  lse = M + log L, with M = max_s m_s, w_s = exp(m_s - M), L = sum_s w_s l_s; s ascending
__global__ __launch_bounds__(kApThreads) void ap_combine_kernel(const float* part, const float* ml, int D, int R, int splits, float* pooled,
                                                                float* lse) {
    __shared__ float wsh[kApMaxSplits];
    const int b = blockIdx.x / R, r = blockIdx.x % R;
    float M = -INFINITY;
    for (int s = 0; s < splits; ++s) M = fmaxf(M, ml[(((size_t)b * splits + s) * R + r) * 2]);
    float L = 0.f;
    for (int s = 0; s < splits; ++s) {
        const float* e = ml + (((size_t)b * splits + s) * R + r) * 2;
        const float w = exp2f((e[0] - M) * kApLog2e);
        L = fmaf(w, e[1], L);
        if (threadIdx.x == 0) wsh[s] = w;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < D; c += kApThreads) {
        float acc = 0.f;
        for (int s = 0; s < splits; ++s) acc = fmaf(wsh[s], part[(((size_t)b * splits + s) * R + r) * D + c], acc);
        pooled[((size_t)b * R + r) * D + c] = acc / L;
    }
    if (threadIdx.x == 0) lse[(size_t)b * R + r] = M + logf(L);
}

// Backward.  Per tile: xh, the scores and dp = xh . dpooled^T as in the forward; p = exp(s - lse), ds = p (dp - delta);
// dU^T += xs^T . dS (the forward's update); with DX: dxh = P . dpooled + dS . U per 16-column block (K = the 16 queries, operands p / ds
// re-derived in the transposed lane map from the same LDS sums), staged in dxs, then the LayerNorm backward of each row.
template <int NBT, bool DX>
__global__ __launch_bounds__(kApThreads, ap_bwd_waves(NBT, DX)) void ap_bwd_kernel(ApArgs a) {
    extern __shared__ float4 ap_lds4[];
    float* lds = reinterpret_cast<float*>(ap_lds4);
    const int D = a.D, R = a.R, LD = D + kApPad, nb = D >> 6, TT = a.tile_tok;
    float* xs = lds;
    float* dxs = xs + TT * LD;                       // DX only
    float* sp = xs + (DX ? 2 : 1) * TT * LD;
    float* gp = sp + 4 * 256;
    float* lse_s = gp + 4 * 256;
    float* delta_s = lse_s + 16;
    float* rstd_s = delta_s + 16;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = blockIdx.x / a.splits, sidx = blockIdx.x % a.splits;
    const int beg = (int)((int64_t)sidx * a.N / a.splits), end = (int)((int64_t)(sidx + 1) * a.N / a.splits);
    const float* xb = a.x + (int64_t)b * a.N * a.ldx;
    const float* gb = a.dpooled + (size_t)b * R * D;
    const int i = lane & 15, kk = lane >> 4;

    // delta_r = dpooled_r . pooled_r: one wave per query, lane-strided fmaf chains and the xor butterfly
    for (int r = wave; r < kApMaxR; r += 4) {
        float d = 0.f;
        if (r < R) {
            const float* pr = a.pooled + ((size_t)b * R + r) * D;
            for (int c = lane; c < D; c += 64) d = fmaf(gb[(size_t)r * D + c], pr[c], d);
            d = wave_sum(d);
        }
        if (lane == 0) {
            delta_s[r] = d;
            lse_s[r] = r < R ? a.lse[(size_t)b * R + r] : 0.f;
        }
    }
    __syncthreads();
    const float lse_r = lse_s[i], delta_r = delta_s[i];

    f32x4 acc[NBT];
#pragma unroll
    for (int q = 0; q < NBT; ++q) acc[q] = f32x4{0.f, 0.f, 0.f, 0.f};

    constexpr bool PF = NBT <= 16;
    float4 pf[PF ? 4 : 1][NBT / 4];
    if (PF && beg < end) ap_load_rows<NBT / 4, PF ? 4 : 1>(pf, xb + (int64_t)beg * a.ldx, a.ldx, min(TT, end - beg), D >> 2, wave, lane, 0);
#pragma unroll 1
    for (int tok0 = beg; tok0 < end; tok0 += TT) {
        const int ntok = min(TT, end - tok0);
        ap_stage<NBT / 4, PF>(pf, xb + (int64_t)tok0 * a.ldx, a.ldx, ntok, TT, D, a.eps, xs, LD, rstd_s, wave, lane);
        __syncthreads();
        if (PF && tok0 + TT < end)
            ap_load_rows<NBT / 4, PF ? 4 : 1>(pf, xb + (int64_t)(tok0 + TT) * a.ldx, a.ldx, min(TT, end - tok0 - TT), D >> 2, wave, lane, 0);
        ap_scores<NBT, true>(xs, LD, TT, a.u, gb, R, D, nb, sp, gp, wave, lane);
        __syncthreads();
        float ds[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int row = 4 * kk + t;
            const float s = ((sp[row * 16 + i] + sp[(16 + row) * 16 + i]) + sp[(32 + row) * 16 + i]) + sp[(48 + row) * 16 + i];
            const float dp = ((gp[row * 16 + i] + gp[(16 + row) * 16 + i]) + gp[(32 + row) * 16 + i]) + gp[(48 + row) * 16 + i];
            const float p = (ap_slot(kk, t) < ntok && i < R) ? exp2f((s - lse_r) * kApLog2e) : 0.f;
            ds[t] = p * (dp - delta_r);
        }
        ap_update<NBT>(xs, LD, TT, ds, nb, acc, wave, lane);
        if (DX) {
            // transposed lane map: lane = (MFMA row i, queries 4 kk + t)
            const bool live = ap_slot(i >> 2, i & 3) < ntok;
            float pT[4], dsT[4];
            const float4 s0 = *reinterpret_cast<const float4*>(sp + i * 16 + 4 * kk), s1 = *reinterpret_cast<const float4*>(sp + (16 + i) * 16 + 4 * kk);
            const float4 s2 = *reinterpret_cast<const float4*>(sp + (32 + i) * 16 + 4 * kk), s3 = *reinterpret_cast<const float4*>(sp + (48 + i) * 16 + 4 * kk);
            const float4 g0 = *reinterpret_cast<const float4*>(gp + i * 16 + 4 * kk), g1 = *reinterpret_cast<const float4*>(gp + (16 + i) * 16 + 4 * kk);
            const float4 g2 = *reinterpret_cast<const float4*>(gp + (32 + i) * 16 + 4 * kk), g3 = *reinterpret_cast<const float4*>(gp + (48 + i) * 16 + 4 * kk);
            const float sT[4] = {((s0.x + s1.x) + s2.x) + s3.x, ((s0.y + s1.y) + s2.y) + s3.y, ((s0.z + s1.z) + s2.z) + s3.z, ((s0.w + s1.w) + s2.w) + s3.w};
            const float gT[4] = {((g0.x + g1.x) + g2.x) + g3.x, ((g0.y + g1.y) + g2.y) + g3.y, ((g0.z + g1.z) + g2.z) + g3.z, ((g0.w + g1.w) + g2.w) + g3.w};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int r = 4 * kk + t;
                pT[t] = (live && r < R) ? exp2f((sT[t] - lse_s[r]) * kApLog2e) : 0.f;
                dsT[t] = pT[t] * (gT[t] - delta_s[r]);
            }
#pragma unroll
            for (int q = 0; q < NBT; ++q) {
                if (q < nb) {
                    const int col = 16 * (wave + 4 * q) + i;
                    f32x4 c0 = {0.f, 0.f, 0.f, 0.f}, c1 = c0;
#pragma unroll
                    for (int t = 0; t < 4; ++t) {
                        const int r = 4 * kk + t;
                        const float gv = r < R ? gb[(size_t)r * D + col] : 0.f;
                        const float uv = r < R ? a.u[(size_t)r * D + col] : 0.f;
                        c0 = ap_mfma(pT[t], gv, c0);
                        c1 = ap_mfma(dsT[t], uv, c1);
                    }
                    c0 += c1;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int slot = ap_slot(kk, e);
                        if (slot < TT) dxs[slot * LD + col] = c0[e];
                    }
                }
            }
            __syncthreads();
            // dx_j = rstd_j (dxh_j - mean(dxh_j) - xh_j mean(dxh_j . xh_j)) for this wave's rows
            const int nq = D >> 2;
            const float fD = (float)D;
            for (int slot = wave; slot < ntok; slot += 4) {
                float s1 = 0.f, s2 = 0.f;
                for (int q = lane; q < nq; q += 64) {
                    const float4 g = *reinterpret_cast<const float4*>(dxs + slot * LD + 4 * q);
                    const float4 h = *reinterpret_cast<const float4*>(xs + slot * LD + 4 * q);
                    s1 += (g.x + g.y) + (g.z + g.w);
                    s2 = fmaf(g.x, h.x, s2); s2 = fmaf(g.y, h.y, s2); s2 = fmaf(g.z, h.z, s2); s2 = fmaf(g.w, h.w, s2);
                }
                const float m1 = wave_sum(s1) / fD, m2 = wave_sum(s2) / fD, rstd = rstd_s[slot];
                float* out = a.dx + ((int64_t)b * a.N + tok0 + slot) * a.lddx;
                for (int q = lane; q < nq; q += 64) {
                    const float4 g = *reinterpret_cast<const float4*>(dxs + slot * LD + 4 * q);
                    const float4 h = *reinterpret_cast<const float4*>(xs + slot * LD + 4 * q);
                    *reinterpret_cast<float4*>(out + 4 * q) = make_float4(rstd * ((g.x - m1) - h.x * m2), rstd * ((g.y - m1) - h.y * m2),
                                                                         rstd * ((g.z - m1) - h.z * m2), rstd * ((g.w - m1) - h.w * m2));
                }
            }
        }
        __syncthreads();
    }
    ap_store_acc<NBT>(acc, a.part + ((size_t)b * a.splits + sidx) * R * D, R, D, nb, wave, lane);
}

// du [r][c] = sum over (clip, split) of the partials, ascending
__global__ __launch_bounds__(kApThreads) void ap_du_reduce_kernel(const float* part, int nparts, int RD, float* du) {
    const int e = blockIdx.x * kApThreads + threadIdx.x;
    if (e >= RD) return;
    float acc = 0.f;
    for (int p = 0; p < nparts; ++p) acc += part[(size_t)p * RD + e];
    du[e] = acc;
}

int ap_check_shape(const char* who, int B, int N, int D, int R, int splits) {
    BVC_REQUIRE(B >= 1 && N >= 1, "%s: B %d and N %d must be positive", who, B, N);
    BVC_REQUIRE(D >= 64 && D <= 2048 && D % 64 == 0, "%s: D %d is not a multiple of 64 in 64 .. 2048", who, D);
    BVC_REQUIRE(R >= 1 && R <= kApMaxR, "%s: R %d outside 1 .. %d", who, R, kApMaxR);
    BVC_REQUIRE(splits >= 0 && splits <= kApMaxSplits, "%s: splits %d outside 0 .. %d", who, splits, kApMaxSplits);
    BVC_REQUIRE((int64_t)B * kApMaxSplits < 0x7fffffffll, "%s: B %d exceeds the grid", who, B);
    return BVC_OK;
}

// about four workgroups per CU, at least 64 tokens per split
int ap_auto_splits(int B, int N) {
    int s = (1024 + B - 1) / B;
    if (s > N / 64) s = N / 64;
    if (s > 64) s = 64;
    return s < 1 ? 1 : s;
}

template <int NBT>
int ap_launch_fwd(const ApArgs& a, size_t lds, hipStream_t s) {
    static bool attr_set = false;
    if (!attr_set) {
        BVC_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&ap_fwd_kernel<NBT>), hipFuncAttributeMaxDynamicSharedMemorySize, kApLdsLimit));
        attr_set = true;
    }
    ap_fwd_kernel<NBT><<<dim3((unsigned)(a.B * a.splits)), dim3(kApThreads), lds, s>>>(a);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}
template <int NBT>
int ap_launch_bwd(const ApArgs& a, size_t lds, hipStream_t s) {
    static bool attr_set = false;
    if (!attr_set) {
        BVC_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&ap_bwd_kernel<NBT, true>), hipFuncAttributeMaxDynamicSharedMemorySize, kApLdsLimit));
        BVC_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&ap_bwd_kernel<NBT, false>), hipFuncAttributeMaxDynamicSharedMemorySize, kApLdsLimit));
        attr_set = true;
    }
    if (a.dx) ap_bwd_kernel<NBT, true><<<dim3((unsigned)(a.B * a.splits)), dim3(kApThreads), lds, s>>>(a);
    else ap_bwd_kernel<NBT, false><<<dim3((unsigned)(a.B * a.splits)), dim3(kApThreads), lds, s>>>(a);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

// accumulator counts compiled: D / 64 <= 4, 12, 16, 24, 32
#define AP_DISPATCH(fn, nb, ...)                                                                                         \
    ((nb) <= 4 ? fn<4>(__VA_ARGS__) : (nb) <= 12 ? fn<12>(__VA_ARGS__) : (nb) <= 16 ? fn<16>(__VA_ARGS__) \
     : (nb) <= 24 ? fn<24>(__VA_ARGS__) : fn<32>(__VA_ARGS__))

}  // namespace

int attn_pool_splits(int B, int N, int D, int R) {
    if (ap_check_shape("op_attn_pool_splits", B, N, D, R, 0) != BVC_OK) return -1;
    return ap_auto_splits(B, N);
}

int64_t attn_pool_workspace(int B, int N, int D, int R, int splits) {
    if (ap_check_shape("op_attn_pool_workspace", B, N, D, R, splits) != BVC_OK) return -1;
    const int s = splits > 0 ? splits : ap_auto_splits(B, N);
    return (int64_t)B * s * R * (D + 2) * 4;
}

int launch_attn_pool_fwd(const float* x, int64_t ldx, const float* u, int B, int N, int D, int R, float eps, int splits, float* pooled,
                         float* lse, void* workspace, hipStream_t s) {
    if (int rc = ap_check_shape("op_attn_pool_fwd", B, N, D, R, splits)) return rc;
    BVC_REQUIRE(x && u && pooled && lse && workspace, "op_attn_pool_fwd: null argument");
    BVC_REQUIRE(ldx >= D && ldx % 4 == 0, "op_attn_pool_fwd: row stride %lld below D %d or not a multiple of 4", (long long)ldx, D);
    BVC_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)u & 15) == 0 && ((uintptr_t)workspace & 15) == 0 && ((uintptr_t)pooled & 3) == 0 &&
                    ((uintptr_t)lse & 3) == 0, "op_attn_pool_fwd: x, u and the workspace must be 16-byte aligned");
    BVC_REQUIRE(eps >= 0.f, "op_attn_pool_fwd: negative eps");
    ApArgs a{};
    a.x = x; a.u = u; a.ldx = ldx; a.B = B; a.N = N; a.D = D; a.R = R; a.eps = eps;
    a.splits = splits > 0 ? splits : ap_auto_splits(B, N);
    a.tile_tok = kApTile;
    a.part = static_cast<float*>(workspace);
    a.ml = a.part + (size_t)B * a.splits * R * D;
    const size_t lds = ((size_t)kApTile * (D + kApPad) + 4 * 256) * 4;
    if (int rc = AP_DISPATCH(ap_launch_fwd, D / 64, a, lds, s)) return rc;
    ap_combine_kernel<<<dim3((unsigned)(B * R)), dim3(kApThreads), 0, s>>>(a.part, a.ml, D, R, a.splits, pooled, lse);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

int launch_attn_pool_bwd(const float* x, int64_t ldx, const float* u, const float* pooled, const float* lse, const float* dpooled, int B,
                         int N, int D, int R, float eps, int splits, float* du, float* dx, int64_t lddx, void* workspace, hipStream_t s) {
    if (int rc = ap_check_shape("op_attn_pool_bwd", B, N, D, R, splits)) return rc;
    BVC_REQUIRE(x && u && pooled && lse && dpooled && du && workspace, "op_attn_pool_bwd: null argument");
    BVC_REQUIRE(ldx >= D && ldx % 4 == 0, "op_attn_pool_bwd: row stride %lld below D %d or not a multiple of 4", (long long)ldx, D);
    BVC_REQUIRE(!dx || (lddx >= D && lddx % 4 == 0 && ((uintptr_t)dx & 15) == 0),
                "op_attn_pool_bwd: dx must be 16-byte aligned with a row stride (%lld) of at least D, a multiple of 4", (long long)lddx);
    BVC_REQUIRE(((uintptr_t)x & 15) == 0 && ((uintptr_t)u & 15) == 0 && ((uintptr_t)dpooled & 15) == 0 && ((uintptr_t)workspace & 15) == 0 &&
                    ((uintptr_t)pooled & 3) == 0 && ((uintptr_t)lse & 3) == 0 && ((uintptr_t)du & 3) == 0,
                "op_attn_pool_bwd: x, u, dpooled and the workspace must be 16-byte aligned");
    BVC_REQUIRE(eps >= 0.f, "op_attn_pool_bwd: negative eps");
    ApArgs a{};
    a.x = x; a.u = u; a.ldx = ldx; a.B = B; a.N = N; a.D = D; a.R = R; a.eps = eps;
    a.splits = splits > 0 ? splits : ap_auto_splits(B, N);
    a.pooled = pooled; a.lse = lse; a.dpooled = dpooled; a.dx = dx; a.lddx = lddx;
    a.part = static_cast<float*>(workspace);
    // with dx two images (xh, dxh) share the LDS: 16-token tiles up to D = 1024, 8-token tiles above
    a.tile_tok = (dx && D > 1024) ? 8 : kApTile;
    const size_t lds = ((size_t)(dx ? 2 : 1) * a.tile_tok * (D + kApPad) + 8 * 256 + 48) * 4;
    static_assert((2 * 16 * (1024 + kApPad) + 8 * 256 + 48) * 4 <= kApLdsLimit && (2 * 8 * (2048 + kApPad) + 8 * 256 + 48) * 4 <= kApLdsLimit &&
                      (16 * (2048 + kApPad) + 8 * 256 + 48) * 4 <= kApLdsLimit, "attnpool: LDS");
    if (int rc = AP_DISPATCH(ap_launch_bwd, D / 64, a, lds, s)) return rc;
    ap_du_reduce_kernel<<<dim3((unsigned)((R * D + kApThreads - 1) / kApThreads)), dim3(kApThreads), 0, s>>>(a.part, B * a.splits, R * D, du);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

}  // namespace bvc

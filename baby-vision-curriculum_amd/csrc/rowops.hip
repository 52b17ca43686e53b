// HBM-bound row / element kernels of the ViT step (gfx950): LayerNorm fwd/bwd, column sums for
// bias gradients, parameter cast, mask -> index lists, tube-patch gather, pixel targets, decoder
// input fill, loss finalize.  All are one-pass streaming kernels with 8-16 B per lane accesses.
#include "rowops.h"
#include "gemm.h"

#include <algorithm>

namespace bvc {

constexpr int kMaxChunks = 4;   // float4 chunks per lane: D <= 1024 (the instantiations every width up to ViT-L runs)
constexpr int kWideChunks = 6;  // D <= 1536: ViT-H (1280), ViT-g (1408); launched only when D > 1024

__device__ __forceinline__ int map_row(int m, RowMap rm) {
    return rm.rin > 0 ? (m / rm.rin) * rm.rout + rm.roff + (m % rm.rin) : m;
}

// sum over the LPR lanes that share a row (64: the wave; 32: each half-wave holds its own row - xor distances < 32 stay inside a half)
template <int LPR>
__device__ __forceinline__ float row_sum(float v) {
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// ============================================================================ LayerNorm forward
// LPR lanes per row: 64 (one wave per row) or 32 (two rows per wave: widths up to 512 that are multiples of 128 - the decoder's and
// the predictor's 384 - would leave half of the wave idle in the second of their 1.5 float4 chunks per lane); y = (x - mean) * rstd * gamma + beta in bf16; saves mean / rstd (biased variance,
// torch.nn.LayerNorm semantics, HF:336-337)
template <int LPR, int NC>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const float* __restrict__ x, RowMap rm, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, bf16_t* __restrict__ y, float* __restrict__ y32,
                                                     float* __restrict__ mean, float* __restrict__ rstd, int M, int D, float eps) {
    constexpr int RPW = 64 / LPR, RPBK = 4 * RPW;        // rows per wave, rows per workgroup and pass
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane % LPR, rsel = lane / LPR;
    const int nch = D >> 2;
    // grid-stride over rows (the launch is capped at a few workgroups per CU): 100352 four-row workgroups per decoder LayerNorm
    // at 256 clips cost more in workgroup turnover than the rows take to stream
    for (int m0 = blockIdx.x * RPBK + wave * RPW; m0 < M; m0 += gridDim.x * RPBK) {
    const int m = m0 + rsel;
    const bool live = m < M;                             // (a half-wave past the last row idles; its shuffles stay in its own half)
    const f32x4* xr = reinterpret_cast<const f32x4*>(x + (size_t)map_row(live ? m : M - 1, rm) * D);
    f32x4 v[NC];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        const int c = sub + LPR * i;
        if (c < nch) { v[i] = xr[c]; s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]); }
    }
    const float mu = row_sum<LPR>(s) / D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        const int c = sub + LPR * i;
        if (c < nch) {
#pragma unroll
            for (int e = 0; e < 4; ++e) { const float d = v[i][e] - mu; q += d * d; }
        }
    }
    const float rs = rsqrtf(row_sum<LPR>(q) / D + eps);
    if (!live) continue;
    if (sub == 0 && mean) { mean[m] = mu; rstd[m] = rs; }
    uint2* yr = y ? reinterpret_cast<uint2*>(y + (size_t)m * D) : nullptr;
    f32x4* yf = y32 ? reinterpret_cast<f32x4*>(y32 + (size_t)m * D) : nullptr;
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        const int c = sub + LPR * i;
        if (c < nch) {
            f32x4 o = (v[i] - mu) * rs;
            if (gamma) o = o * reinterpret_cast<const f32x4*>(gamma)[c] + reinterpret_cast<const f32x4*>(beta)[c];
            if (yr) yr[c] = uint2{pack2bf(o[0], o[1]), pack2bf(o[2], o[3])};
            if (yf) yf[c] = o;
        }
    }
    }
}

// ============================================================================ LayerNorm backward
// dx = rstd * (g - mean(g) - xhat * mean(g * xhat)),  g = dy * gamma;  dres (+)= dx; optional bf16 copy;
// per-workgroup partials of dgamma = sum_rows dy * xhat and dbeta = sum_rows dy go to part[block][2][D]
// (every workgroup hammering the same D addresses with atomics serialises: measured 2x on the kernel);
// ln_param_reduce_kernel folds them into the gradients
// GATED: the bf16 copy alone is multiplied by the gate of the residual branch it feeds (dropgate.h; element index = physical row * D +
// column); dres itself, the residual gradient, passes ungated.
template <int RPB, int LPR, int NC, bool GATED>
__device__ __forceinline__ void ln_bwd_body(const bf16_t* __restrict__ dy, const float* __restrict__ x, RowMap rm,
                                            const float* __restrict__ mean, const float* __restrict__ rstd,
                                            const float* __restrict__ gamma, float* __restrict__ dres,
                                            int accumulate, bf16_t* __restrict__ dres_bf, float* __restrict__ part,
                                            int M, int D, const Gate& gate, int compact) {
    // per-wave (per half-wave for LPR = 32) column partials, [4 RPW][dgamma | dbeta][D]: sized by D at launch (a static 32 KiB array
    // capped the kernel at 5 workgroups per CU; at D = 384 this is 24 KiB and the register budget decides: 6-7)
    extern __shared__ __attribute__((aligned(16))) float red[];
    constexpr int RPW = 64 / LPR;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int sub = lane % LPR, rsel = lane / LPR;
    const int nch = D >> 2;
    f32x4 gam[NC], dg[NC], db[NC];
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        const int c = sub + LPR * i;
        gam[i] = c < nch ? reinterpret_cast<const f32x4*>(gamma)[c] : f32x4{0, 0, 0, 0};
        dg[i] = f32x4{0, 0, 0, 0};
        db[i] = f32x4{0, 0, 0, 0};
    }
    const float invD = 1.f / D;
    // grid-stride over row groups of RPB rows: the launch is capped at a few workgroups per CU, so the column partials below are
    // written once per RESIDENT workgroup (2048 x 2 D floats) instead of once per RPB rows (25088 x 2 D at the decoder's 256-clip
    // size: 77 MB per LayerNorm backward, and a reduction kernel to match)
    const int ngroups = (M + RPB - 1) / RPB;
    for (int grp = blockIdx.x; grp < ngroups; grp += gridDim.x)
    for (int it = 0; it < RPB / (4 * RPW); ++it) {
        const int mw = grp * RPB + (it * 4 + wave) * RPW;     // first row of this wave
        if (mw >= M) break;
        const int m = mw + rsel;
        const bool live = m < M;
        const int mc = live ? m : M - 1;
        const size_t xrow = (size_t)map_row(mc, rm) * D;       // the row of dres; with `compact`, x and the bf16 copy are stored by logical row
        const size_t crow = compact ? (size_t)mc * D : xrow;
        const f32x4* xr = reinterpret_cast<const f32x4*>(x + crow);
        const uint2* dyr = reinterpret_cast<const uint2*>(dy + (size_t)mc * D);
        const float mu = mean[mc], rs = rstd[mc];
        f32x4 xh[NC], g[NC];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            const int c = sub + LPR * i;
            if (c < nch) {
                const uint2 d = dyr[c];
                f32x4 dyv = {__uint_as_float(d.x << 16), __uint_as_float(d.x & 0xffff0000u),
                             __uint_as_float(d.y << 16), __uint_as_float(d.y & 0xffff0000u)};
                if (!live) dyv = f32x4{0, 0, 0, 0};      // a half-wave past the last row adds nothing to the column sums
                xh[i] = (xr[c] - mu) * rs;
                g[i] = dyv * gam[i];
                dg[i] += dyv * xh[i];
                db[i] += dyv;
#pragma unroll
                for (int e = 0; e < 4; ++e) { s1 += g[i][e]; s2 += g[i][e] * xh[i][e]; }
            }
        }
        s1 = row_sum<LPR>(s1) * invD;
        s2 = row_sum<LPR>(s2) * invD;
        if (!live) continue;
        f32x4* dr = reinterpret_cast<f32x4*>(dres + xrow);
        uint2* db16 = dres_bf ? reinterpret_cast<uint2*>(dres_bf + crow) : nullptr;
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            const int c = sub + LPR * i;
            if (c < nch) {
                f32x4 dx = (g[i] - s1 - xh[i] * s2) * rs;
                if (accumulate) dx += dr[c];
                dr[c] = dx;
                if constexpr (GATED) {
                    if (db16) {
                        const int prow = map_row(mc, rm);
                        const f32x4 w = gate_apply4(gate, prow, (uint64_t)prow * nch + c, dx);
                        db16[c] = uint2{pack2bf(w[0], w[1]), pack2bf(w[2], w[3])};
                    }
                } else {
                    if (db16) db16[c] = uint2{pack2bf(dx[0], dx[1]), pack2bf(dx[2], dx[3])};
                }
            }
        }
    }
    // cross-wave reduction of the column partials (4 RPW of them), then one partial row per workgroup
    const int slot = wave * RPW + rsel;
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        const int c = sub + LPR * i;
        if (c < nch) {
            *reinterpret_cast<f32x4*>(red + (slot * 2 + 0) * D + c * 4) = dg[i];
            *reinterpret_cast<f32x4*>(red + (slot * 2 + 1) * D + c * 4) = db[i];
        }
    }
    __syncthreads();
    float* pg = part + (size_t)blockIdx.x * 2 * D;
    for (int col = threadIdx.x; col < D; col += 256) {
        float a = 0.f, b = 0.f;
#pragma unroll
        for (int w = 0; w < 4 * RPW; ++w) { a += red[(2 * w) * D + col]; b += red[(2 * w + 1) * D + col]; }
        pg[col] = a;
        pg[D + col] = b;
    }
}

template <int RPB, int LPR, int NC>
__global__ __launch_bounds__(256) void ln_bwd_kernel(const bf16_t* __restrict__ dy, const float* __restrict__ x, RowMap rm,
                                                     const float* __restrict__ mean, const float* __restrict__ rstd,
                                                     const float* __restrict__ gamma, float* __restrict__ dres,
                                                     int accumulate, bf16_t* __restrict__ dres_bf, float* __restrict__ part,
                                                     int M, int D, int compact) {
    ln_bwd_body<RPB, LPR, NC, false>(dy, x, rm, mean, rstd, gamma, dres, accumulate, dres_bf, part, M, D, Gate{}, compact);
}
template <int RPB, int LPR, int NC>
__global__ __launch_bounds__(256) void ln_bwd_gate_kernel(const bf16_t* __restrict__ dy, const float* __restrict__ x, RowMap rm,
                                                          const float* __restrict__ mean, const float* __restrict__ rstd,
                                                          const float* __restrict__ gamma, float* __restrict__ dres,
                                                          int accumulate, bf16_t* __restrict__ dres_bf, float* __restrict__ part,
                                                          int M, int D, const Gate gate) {
    ln_bwd_body<RPB, LPR, NC, true>(dy, x, rm, mean, rstd, gamma, dres, accumulate, dres_bf, part, M, D, gate, 0);
}

// dgamma[c] += sum_b part[b][0][c], dbeta[c] += sum_b part[b][1][c]; grid (ceil(2D/256), ceil(nblk/ROWS))
// ROWS = 16: one chain of 16 partial rows per workgroup, then one atomic.  ROWS = 64 (more than kLnReduceWide partial rows): four such
// chains added pairwise, then one atomic - with 16 rows per workgroup the 2048 partial rows of a large LayerNorm ended in a chain of
// 128 f32 atomics per column, whose rounding error (3 - 4 x that of torch's reduction, varying with the arrival order) sat at the
// bar of tests/test_gpu_rowops.py; at most 32 atomics leave it at about half of that
constexpr int kLnReduceWide = 256;
template <int ROWS>
__global__ __launch_bounds__(256) void ln_param_reduce_kernel(const float* __restrict__ part, int nblk, int D,
                                                              float* __restrict__ dgamma, float* __restrict__ dbeta) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= 2 * D) return;
    const int b0 = blockIdx.y * ROWS, b1 = min(nblk, b0 + ROWS);
    float s[ROWS / 16];
#pragma unroll
    for (int j = 0; j < ROWS / 16; ++j) {
        float v[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) v[i] = b0 + 16 * j + i < b1 ? part[(size_t)(b0 + 16 * j + i) * 2 * D + c] : 0.f;   // 16 loads in flight
        s[j] = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) s[j] += v[i];
    }
    float t = s[0];
    if constexpr (ROWS == 64) t = (s[0] + s[1]) + (s[2] + s[3]);
    atomicAdd(c < D ? dgamma + c : dbeta + (c - D), t);
}

// Deterministic mode (options().deterministic): column c of nrows partial rows of W floats, added in row order onto its output -
// out0[c] for c < split, out1[c - split] otherwise: v = out + part[0][c] + part[1][c] + ...  Replaces the atomics of
// ln_param_reduce_kernel (part = the [2][D] rows, split = D) and of the column sums (their per-row-block partials, split = W).
// grid ceil(W / 256); 8 loads in flight per thread.
__global__ __launch_bounds__(256) void det_rows_reduce_kernel(const float* __restrict__ part, int nrows, int W, int split,
                                                              float* __restrict__ out0, float* __restrict__ out1) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= W) return;
    float* o = c < split ? out0 + c : out1 + (c - split);
    float s = *o;
    int b = 0;
    for (; b + 8 <= nrows; b += 8) {
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = part[(size_t)(b + i) * W + c];
#pragma unroll
        for (int i = 0; i < 8; ++i) s += v[i];
    }
    for (; b < nrows; ++b) s += part[(size_t)b * W + c];
    *o = s;
}
// first pass of the two-pass form: mid[y][c] = part[y per][c] + ... + part[y per + per - 1][c] (row order; grid (ceil(W / 256), chunks))
__global__ __launch_bounds__(256) void det_rows_chunk_kernel(const float* __restrict__ part, int nrows, int W, int per,
                                                             float* __restrict__ mid) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= W) return;
    const int b0 = blockIdx.y * per, b1 = min(nrows, b0 + per);
    float s = 0.f;
    int b = b0;
    for (; b + 8 <= b1; b += 8) {
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = part[(size_t)(b + i) * W + c];
#pragma unroll
        for (int i = 0; i < 8; ++i) s += v[i];
    }
    for (; b < b1; ++b) s += part[(size_t)b * W + c];
    mid[(size_t)blockIdx.y * W + c] = s;
}

// Fixed-order column reduce of nrows partial rows (deterministic mode).  One thread per column alone leaves the chip idle (W = 2 D = 768
// columns = 3 workgroups walking ~10^4 rows: 2.6 ms per step at 256 clips); rows are therefore summed in chunks of ~sqrt(nrows), in
// order, then the chunk sums in order - the same association on every run.  `mid` = det_rows_chunks(nrows) x W floats of scratch.
static int det_rows_chunk_rows(int nrows) {
    int per = 16;
    while ((long long)per * per < nrows) per *= 2;
    return per;
}
static size_t det_rows_mid_floats(int nrows, int W) {
    const int per = det_rows_chunk_rows(nrows);
    return nrows > per ? (size_t)((nrows + per - 1) / per) * W : 0;
}
static int launch_det_rows_reduce(const float* part, int nrows, int W, int split, float* out0, float* out1, float* mid, hipStream_t s) {
    const int per = det_rows_chunk_rows(nrows);
    if (nrows > per) {
        const int chunks = (nrows + per - 1) / per;
        hipLaunchKernelGGL(det_rows_chunk_kernel, dim3((W + 255) / 256, chunks), dim3(256), 0, s, part, nrows, W, per, mid);
        BVC_CHECK_HIP(hipGetLastError());
        part = mid;
        nrows = chunks;
    }
    hipLaunchKernelGGL(det_rows_reduce_kernel, dim3((W + 255) / 256), dim3(256), 0, s, part, nrows, W, split, out0, out1);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

// ============================================================================ column sums
// out[n] += alpha * sum_m X[m][n]   (bias gradients), X bf16 [M][ld]; grid (ceil(N/512), ceil(M/RB))
// DET: no atomics - row block y writes its partial row to out[y][N] (det_rows_reduce_kernel adds them in order)
template <bool DET>
__device__ __forceinline__ void colsum_bf16_body(const bf16_t* __restrict__ X, int M, int N, int ld, float alpha,
                                                 const float* __restrict__ alpha_dev, float* __restrict__ out, int RB) {
    __shared__ float red[4][512];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = (blockIdx.x * 64 + lane) * 8;
    float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const int r0 = blockIdx.y * RB, r1 = min(M, r0 + RB);
    if (col < N) {
        for (int m = r0 + wave; m < r1; m += 4) {
            const bf16x8 v = *reinterpret_cast<const bf16x8*>(X + (size_t)m * ld + col);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] += bf2f((bf16_t)v[e]);
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) red[wave][lane * 8 + e] = acc[e];
    __syncthreads();
    for (int c = threadIdx.x; c < 512; c += 256) {
        const int n = blockIdx.x * 512 + c;
        if (n < N) {
            const float v = (alpha_dev ? alpha * alpha_dev[0] : alpha) * ((red[0][c] + red[1][c]) + (red[2][c] + red[3][c]));
            if constexpr (DET) out[(size_t)blockIdx.y * N + n] = v;
            else atomicAdd(out + n, v);
        }
    }
}
__global__ __launch_bounds__(256) void colsum_bf16_kernel(const bf16_t* __restrict__ X, int M, int N, int ld, float alpha,
                                                          const float* __restrict__ alpha_dev, float* __restrict__ out, int RB) {
    colsum_bf16_body<false>(X, M, N, ld, alpha, alpha_dev, out, RB);
}
__global__ __launch_bounds__(256) void colsum_bf16_det_kernel(const bf16_t* __restrict__ X, int M, int N, int ld, float alpha,
                                                              const float* __restrict__ alpha_dev, float* __restrict__ part, int RB) {
    colsum_bf16_body<true>(X, M, N, ld, alpha, alpha_dev, part, RB);
}

// out[n] += sum over mapped rows of X f32 [..][D]   (mask-token gradient); grid (ceil(D/256), ceil(M/RB))
template <bool DET>
__device__ __forceinline__ void colsum_f32_body(const float* __restrict__ X, RowMap rm, int M, int D, float* __restrict__ out, int RB) {
    __shared__ float red[4][256];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int col = (blockIdx.x * 64 + lane) * 4;
    f32x4 acc = {0, 0, 0, 0};
    const int r0 = blockIdx.y * RB, r1 = min(M, r0 + RB);
    if (col < D) {
        // four partial sums per lane, added pairwise at the end: chains of 16 rows instead of one of 64 (a serial f32 sum of 64 rows
        // measured 4.2 x the error of torch's sum at M = 256), and four loads in flight
        f32x4 a1 = {0, 0, 0, 0}, a2 = {0, 0, 0, 0}, a3 = {0, 0, 0, 0};
        int m = r0 + wave;
        for (; m + 12 < r1; m += 16) {
            acc += *reinterpret_cast<const f32x4*>(X + (size_t)map_row(m, rm) * D + col);
            a1 += *reinterpret_cast<const f32x4*>(X + (size_t)map_row(m + 4, rm) * D + col);
            a2 += *reinterpret_cast<const f32x4*>(X + (size_t)map_row(m + 8, rm) * D + col);
            a3 += *reinterpret_cast<const f32x4*>(X + (size_t)map_row(m + 12, rm) * D + col);
        }
        for (; m < r1; m += 4) acc += *reinterpret_cast<const f32x4*>(X + (size_t)map_row(m, rm) * D + col);
        acc = (acc + a1) + (a2 + a3);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) red[wave][lane * 4 + e] = acc[e];
    __syncthreads();
    const int c = threadIdx.x;
    const int n = blockIdx.x * 256 + c;
    if constexpr (DET) {
        if (n < D) out[(size_t)blockIdx.y * D + n] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
    } else {
        if (n < D) atomicAdd(out + n, (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]));
    }
}
__global__ __launch_bounds__(256) void colsum_f32_kernel(const float* __restrict__ X, RowMap rm, int M, int D,
                                                         float* __restrict__ out, int RB) {
    colsum_f32_body<false>(X, rm, M, D, out, RB);
}
__global__ __launch_bounds__(256) void colsum_f32_det_kernel(const float* __restrict__ X, RowMap rm, int M, int D,
                                                             float* __restrict__ part, int RB) {
    colsum_f32_body<true>(X, rm, M, D, part, RB);
}

// out[b][d] = mean over the N tokens of clip b (sequence_output.mean(1), HF VideoMAEForVideoClassification.forward);
// grid (ceil(D/64), B); thread = 4 columns x one of 16 row phases; fixed summation order (no atomics)
__global__ __launch_bounds__(256) void token_mean_kernel(const float* __restrict__ x, int N, int D, float* __restrict__ out) {
    __shared__ float red[16][64];
    const int cg = threadIdx.x & 15, rp = threadIdx.x >> 4;
    const int col = blockIdx.x * 64 + cg * 4;
    const float* xb = x + (size_t)blockIdx.y * N * D;
    f32x4 acc = {0, 0, 0, 0};
    if (col < D)
        for (int m = rp; m < N; m += 16) acc += *reinterpret_cast<const f32x4*>(xb + (size_t)m * D + col);
#pragma unroll
    for (int e = 0; e < 4; ++e) red[rp][cg * 4 + e] = acc[e];
    __syncthreads();
    if (threadIdx.x < 64) {
        float t = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) t += red[r][threadIdx.x];
        const int n = blockIdx.x * 64 + threadIdx.x;
        if (n < D) out[(size_t)blockIdx.y * D + n] = t / (float)N;
    }
}

// dx[b][m][d] = dmean[b][d] / N   (backward of token_mean); one f32x4 per thread
__global__ void token_mean_bwd_kernel(const float* __restrict__ dmean, float* __restrict__ dx, int N, int D, size_t total4) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total4) return;
    const size_t e = i * 4;
    const int d = (int)(e % D);
    const size_t b = e / ((size_t)N * D);
    f32x4 g = *reinterpret_cast<const f32x4*>(dmean + b * D + d);
    const float inv = 1.f / (float)N;
    g *= inv;
    *reinterpret_cast<f32x4*>(dx + e) = g;
}

// Backward of fc_norm(token_mean(x)) (VideoMAEForVideoClassification fine-tuning) in one launch, no atomics.
// Workgroup (x, b) with b < B re-derives clip b's LayerNorm backward from its pooled row p (D <= 1536 floats):
//   g = dy * gamma,  dp = rstd * (g - mean(g) - xhat * mean(g * xhat)),  xhat = (p - mean) * rstd,
// keeps dp / N in LDS and writes it to token rows [x * kFcRows, x * kFcRows + kFcRows) of the clip, in f32 (dres) and as the bf16 copy
// (dres_bf) the last encoder layer's backward reads.  Workgroups of row y == pblk write dgamma = sum_b dy * xhat and dbeta = sum_b dy for
// 256 columns each, over the B rows in order: the same bits on every run.  dres == nullptr (pblk = 0): the parameter gradients only.
constexpr int kFcRows = 32;
template <bool GATED>     // GATED: the bf16 copy is multiplied by the gate of the last layer's MLP branch (dropgate.h), as in ln_bwd_body
__device__ __forceinline__ void fcnorm_bwd_bcast_body(const float* __restrict__ dy, const float* __restrict__ p,
                                                      const float* __restrict__ mean, const float* __restrict__ rstd,
                                                      const float* __restrict__ gamma, float* __restrict__ dres,
                                                      bf16_t* __restrict__ dres_bf, float* __restrict__ dgamma,
                                                      float* __restrict__ dbeta, int B, int N, int D, int pblk, const Gate& gate) {
    const int b = blockIdx.y;
    if (b == pblk) {
        const int d = blockIdx.x * 256 + threadIdx.x;
        if (d >= D) return;
        float sg = 0.f, sb = 0.f;
        for (int r = 0; r < B; ++r) {
            const float g = dy[(size_t)r * D + d];
            sg += g * ((p[(size_t)r * D + d] - mean[r]) * rstd[r]);
            sb += g;
        }
        dgamma[d] = sg;
        dbeta[d] = sb;
        return;
    }
    const int r0 = blockIdx.x * kFcRows;
    if (r0 >= N) return;
    __shared__ __attribute__((aligned(16))) float dps[1536];
    __shared__ float red[2][4];
    const float mu = mean[b], rs = rstd[b];
    const float* dyr = dy + (size_t)b * D;
    const float* pr = p + (size_t)b * D;
    float s1 = 0.f, s2 = 0.f;
    for (int d = threadIdx.x; d < D; d += 256) {
        const float g = dyr[d] * gamma[d];
        s1 += g;
        s2 += g * ((pr[d] - mu) * rs);
    }
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { red[0][wave] = s1; red[1][wave] = s2; }
    __syncthreads();
    const float m1 = ((red[0][0] + red[0][1]) + (red[0][2] + red[0][3])) / (float)D;
    const float m2 = ((red[1][0] + red[1][1]) + (red[1][2] + red[1][3])) / (float)D;
    for (int d = threadIdx.x; d < D; d += 256) {
        const float g = dyr[d] * gamma[d];
        dps[d] = (rs * (g - m1 - ((pr[d] - mu) * rs) * m2)) / (float)N;
    }
    __syncthreads();
    const int nch = D >> 2, rows = min(N - r0, kFcRows);
    const size_t base = ((size_t)b * N + r0) * D;
    for (int i = threadIdx.x; i < rows * nch; i += 256) {
        const int r = i / nch, c = i - r * nch;
        const f32x4 v = *reinterpret_cast<const f32x4*>(dps + c * 4);
        const size_t o = base + (size_t)r * D + (size_t)c * 4;
        *reinterpret_cast<f32x4*>(dres + o) = v;
        if constexpr (GATED) {
            const f32x4 w = gate_apply4(gate, b * N + r0 + r, (uint64_t)(o >> 2), v);
            *reinterpret_cast<uint2*>(dres_bf + o) = uint2{pack2bf(w[0], w[1]), pack2bf(w[2], w[3])};
        } else {
            *reinterpret_cast<uint2*>(dres_bf + o) = uint2{pack2bf(v[0], v[1]), pack2bf(v[2], v[3])};
        }
    }
}
__global__ __launch_bounds__(256) void fcnorm_bwd_bcast_kernel(const float* __restrict__ dy, const float* __restrict__ p,
                                                               const float* __restrict__ mean, const float* __restrict__ rstd,
                                                               const float* __restrict__ gamma, float* __restrict__ dres,
                                                               bf16_t* __restrict__ dres_bf, float* __restrict__ dgamma,
                                                               float* __restrict__ dbeta, int B, int N, int D, int pblk) {
    fcnorm_bwd_bcast_body<false>(dy, p, mean, rstd, gamma, dres, dres_bf, dgamma, dbeta, B, N, D, pblk, Gate{});
}
__global__ __launch_bounds__(256) void fcnorm_bwd_bcast_gate_kernel(const float* __restrict__ dy, const float* __restrict__ p,
                                                                    const float* __restrict__ mean, const float* __restrict__ rstd,
                                                                    const float* __restrict__ gamma, float* __restrict__ dres,
                                                                    bf16_t* __restrict__ dres_bf, float* __restrict__ dgamma,
                                                                    float* __restrict__ dbeta, int B, int N, int D, int pblk, const Gate gate) {
    fcnorm_bwd_bcast_body<true>(dy, p, mean, rstd, gamma, dres, dres_bf, dgamma, dbeta, B, N, D, pblk, gate);
}

// ============================================================================ dropout mask (what the gates above apply, made visible)
// out[e] = 1 where element e of the (layer, branch) mask is KEPT; one thread per four elements, any M x N
__global__ __launch_bounds__(256) void dropout_mask_kernel(const Gate gate, size_t n, uint8_t* __restrict__ out) {
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q * 4 >= n) return;
    uint32_t r[4];
    gate_draws(gate, q, r);
#pragma unroll
    for (int e = 0; e < 4; ++e)
        if (q * 4 + e < n) out[q * 4 + e] = r[e] >= gate.thr ? 1 : 0;
}

// ============================================================================ elementwise
__global__ void cast_f32_bf16_kernel(const float* __restrict__ in, bf16_t* __restrict__ out, size_t n) {
    const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 8;
    if (i + 8 <= n) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(in + i);
        const f32x4 b = *reinterpret_cast<const f32x4*>(in + i + 4);
        *reinterpret_cast<uint4*>(out + i) = uint4{pack2bf(a[0], a[1]), pack2bf(a[2], a[3]), pack2bf(b[0], b[1]), pack2bf(b[2], b[3])};
    } else {
        for (size_t j = i; j < n; ++j) out[j] = f2bf(in[j]);
    }
}

// out bf16 [M][D] = in f32 [map_row(m)][D]
__global__ void gather_rows_bf16_kernel(const float* __restrict__ in, RowMap rm, bf16_t* __restrict__ out, int M, int D) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;   // float4 item
    const int nch = D >> 2;
    if (i >= (size_t)M * nch) return;
    const int m = (int)(i / nch), c = (int)(i % nch);
    const f32x4 v = *reinterpret_cast<const f32x4*>(in + (size_t)map_row(m, rm) * D + c * 4);
    *reinterpret_cast<uint2*>(out + (size_t)m * D + c * 4) = uint2{pack2bf(v[0], v[1]), pack2bf(v[2], v[3])};
}

// ============================================================================ mask -> ordered index lists
// one wave per clip: ascending token order for both lists (boolean-mask gather order, HF:121,578-579,661)
__global__ void mask_index_kernel(const uint8_t* __restrict__ mask, int L, int nvis, int nmask, int* __restrict__ vis_idx,
                                  int* __restrict__ msk_idx, int* __restrict__ status) {
    const int b = blockIdx.x, lane = threadIdx.x;
    int nv = 0, nm = 0;
    const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    for (int base = 0; base < L; base += 64) {
        const int t = base + lane;
        const bool in = t < L;
        const bool mk = in && mask[(size_t)b * L + t] != 0;
        const unsigned long long bm = __ballot(mk), bv = __ballot(in && !mk);
        if (mk) { const int p = nm + __popcll(bm & below); if (p < nmask) msk_idx[(size_t)b * nmask + p] = t; }
        if (in && !mk) { const int p = nv + __popcll(bv & below); if (p < nvis) vis_idx[(size_t)b * nvis + p] = t; }
        nm += __popcll(bm);
        nv += __popcll(bv);
    }
    if (lane == 0 && (nv != nvis || nm != nmask)) atomicOr(status, 1);
}

// The same with a second byte mask that picks the masked tokens the decoder reconstructs (VideoMAE V2's decoder masking): vis_idx as
// above, dec_idx the decoded tokens in ascending token order, so the boolean-gather order (HF:578-582) holds for the subset.  The
// status word is raised when a clip's visible count is not nvis, its decoded count is not ndec, or a decoded token is not masked (a
// decoded token the encoder sees would leak its target into the loss).
__global__ void dual_mask_index_kernel(const uint8_t* __restrict__ mask, const uint8_t* __restrict__ decode, int L, int nvis, int ndec,
                                       int* __restrict__ vis_idx, int* __restrict__ dec_idx, int* __restrict__ status) {
    const int b = blockIdx.x, lane = threadIdx.x;
    int nv = 0, nd = 0, nbad = 0;
    const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    for (int base = 0; base < L; base += 64) {
        const int t = base + lane;
        const bool in = t < L;
        const bool mk = in && mask[(size_t)b * L + t] != 0;
        const bool dk = in && decode[(size_t)b * L + t] != 0;
        const unsigned long long bv = __ballot(in && !mk), bd = __ballot(dk);
        if (dk) { const int p = nd + __popcll(bd & below); if (p < ndec) dec_idx[(size_t)b * ndec + p] = t; }
        if (in && !mk) { const int p = nv + __popcll(bv & below); if (p < nvis) vis_idx[(size_t)b * nvis + p] = t; }
        nd += __popcll(bd);
        nv += __popcll(bv);
        nbad += __popcll(__ballot(dk && !mk));
    }
    if (lane == 0 && (nv != nvis || nd != ndec || nbad != 0)) atomicOr(status, 1);
}

// four consecutive pixels of channel c starting at element `src` (a multiple of 4)
__device__ __forceinline__ f32x4 load_pixels4(const PixelSrc& px, size_t src, int c) {
    if (!px.is_u8) return *reinterpret_cast<const f32x4*>(reinterpret_cast<const float*>(px.ptr) + src);
    const uint32_t w = *reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(px.ptr) + src);
    const float mu = px.mean[c & 3], sd = px.stdv[c & 3];
    f32x4 v;
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = ((float)((w >> (8 * j)) & 0xffu) / 255.f - mu) / sd;
    return v;
}

// ============================================================================ tube-patch gather (visible tokens only)
// A[m][k], k = ((c*ts + dt)*ps + dy)*ps + dx  (Conv3d weight order, HF:157-162), clip f32 [B][T][C][H][W]
__global__ void gather_patches_kernel(const PixelSrc clip, const int* __restrict__ vis_idx, bf16_t* __restrict__ A,
                                      int B, int nvis, PatchGeom pg) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int K = pg.C * pg.ts * pg.ps * pg.ps;
    const int k8 = K >> 3;
    if (i >= (size_t)B * nvis * k8) return;
    const int m = (int)(i / k8);
    const int k = (int)(i % k8) * 8;
    const int dx = k % pg.ps, dy = (k / pg.ps) % pg.ps, dt = (k / (pg.ps * pg.ps)) % pg.ts, c = k / (pg.ps * pg.ps * pg.ts);
    const int b = m / nvis, tok = vis_idx[m];
    const int wp = pg.W / pg.ps, hp = pg.H / pg.ps;
    const int tp = tok / (hp * wp), yp = (tok / wp) % hp, xp = tok % wp;
    const size_t src = ((((size_t)b * pg.T + tp * pg.ts + dt) * pg.C + c) * pg.H + yp * pg.ps + dy) * pg.W + xp * pg.ps + dx;
    const f32x4 a = load_pixels4(clip, src, c);
    const f32x4 d = load_pixels4(clip, src + 4, c);
    *reinterpret_cast<uint4*>(A + (size_t)m * K + k) =
        uint4{pack2bf(a[0], a[1]), pack2bf(a[2], a[3]), pack2bf(d[0], d[1]), pack2bf(d[2], d[3])};
}

// ============================================================================ tube-patch gather with Mixup / CutMix
// The gather above with clip b composed, on its way into A, with a partner clip (ClipMix = bvc_clip_mix, one entry per clip): inside
// the entry's box the partner's pixel, outside it lam * own + (1 - lam) * partner in f32 (the own pixel itself when lam == 1).  Both
// come through load_pixels4, so they are normalised values for either source dtype, and the mixed clip is never written anywhere.
// A thread's 8-pixel run lies in one image row.  A run the box covers whole reads the partner only, a run outside the box with
// lam == 1 reads its own clip only - the second load is not issued where its value is unused, so a CutMix moves the bytes of the plain
// gather; only a run a box edge cuts, or one that is blended, reads both.  A 64-lane wave covers one 16 x 16 patch over two frames,
// so the branch is wave-uniform except on the patches a vertical box edge crosses.
// WAVE_ROW: K / 8 is a multiple of 64 (every configuration of the reference: K = 1536), so a wave lies in one row of A and the row,
// its clip, its token and the clip's table entry are wave-uniform: read once per wave through the scalar unit, decoded in SGPRs.
// Entries are not trusted: a partner outside [0, B) and a box outside the image are clamped before any address is formed, and bit 0 of
// *status (when given) is raised, as is done for a lam outside [0, 1].
template <bool WAVE_ROW>
__global__ void gather_patches_mix_kernel(const PixelSrc clip, const int* __restrict__ idx, bf16_t* __restrict__ A, int B, int n,
                                          PatchGeom pg, const ClipMix* __restrict__ mix, int* __restrict__ status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int K = pg.C * pg.ts * pg.ps * pg.ps;
    const int k8 = K >> 3;
    if (i >= (size_t)B * n * k8) return;
    const int mv = (int)(i / k8);
    const int m = WAVE_ROW ? __builtin_amdgcn_readfirstlane(mv) : mv;
    const int k = (int)(i - (size_t)m * k8) * 8;
    const int dx = k % pg.ps, dy = (k / pg.ps) % pg.ps, dt = (k / (pg.ps * pg.ps)) % pg.ts, c = k / (pg.ps * pg.ps * pg.ts);
    const int b = m / n, tok = idx[m];
    const int wp = pg.W / pg.ps, hp = pg.H / pg.ps;
    const int tp = tok / (hp * wp), yp = (tok / wp) % hp, xp = tok % wp;
    const int y = yp * pg.ps + dy, x = xp * pg.ps + dx;
    const ClipMix e = mix[b];
    const int partner = min(max(e.partner, 0), B - 1);
    const int y0 = min(max(e.y0, 0), pg.H), y1 = min(max(e.y1, 0), pg.H), x0 = min(max(e.x0, 0), pg.W), x1 = min(max(e.x1, 0), pg.W);
    const float lam = e.lam;
    if (status && k == 0 && m % n == 0 &&
        (partner != e.partner || y0 != e.y0 || y1 != e.y1 || x0 != e.x0 || x1 != e.x1 || !(lam >= 0.f && lam <= 1.f)))
        atomicOr(status, 1);
    const size_t in_clip = ((((size_t)(tp * pg.ts + dt)) * pg.C + c) * pg.H + y) * pg.W + x;
    const size_t per_clip = (size_t)pg.T * pg.C * pg.H * pg.W;
    const size_t own = (size_t)b * per_clip + in_clip, oth = (size_t)partner * per_clip + in_clip;
    // pixels of the run inside the box: [lo, hi) in run coordinates
    const bool row_in = y >= y0 && y < y1;
    const int lo = row_in ? max(x0 - x, 0) : 8, hi = row_in ? min(x1 - x, 8) : 0;
    const bool all_in = lo == 0 && hi == 8, none_in = lo >= hi;
    // every lane reads one source: the partner where the box covers the run, its own clip otherwise; only a run that is cut or blended
    // goes on to read the partner as well
    const size_t first = all_in ? oth : own;
    f32x4 a = load_pixels4(clip, first, c);
    f32x4 d = load_pixels4(clip, first + 4, c);
    if (!(all_in || (none_in && lam == 1.0f))) {
        const f32x4 a1 = load_pixels4(clip, oth, c), d1 = load_pixels4(clip, oth + 4, c);
        const float rem = 1.0f - lam;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float ma = lam == 1.0f ? a[j] : lam * a[j] + rem * a1[j];
            const float md = lam == 1.0f ? d[j] : lam * d[j] + rem * d1[j];
            a[j] = (j >= lo && j < hi) ? a1[j] : ma;
            d[j] = (j + 4 >= lo && j + 4 < hi) ? d1[j] : md;
        }
    }
    *reinterpret_cast<uint4*>(A + (size_t)m * K + k) =
        uint4{pack2bf(a[0], a[1]), pack2bf(a[2], a[3]), pack2bf(d[0], d[1]), pack2bf(d[2], d[3])};
}

// ============================================================================ tube-patch gather with random erasing, then Mixup / CutMix
// Four N(0, 1) values from one Philox call (include/bvc.h, bvc_erase_box): counter {low q, high q | tag << 16, offset}, key = seed;
// lanes 0 / 1 the cos / sin branch of Box-Muller on (r0, r1), lanes 2 / 3 on (r2, r3).  Both uniforms are exact in f32 and u1 > 0.
__device__ __forceinline__ f32x4 erase_normals4(const EraseTab& er, uint64_t q, uint32_t tag) {
    uint32_t r[4];
    philox4x32_10((uint32_t)q, (uint32_t)(q >> 32) | (tag << 16), er.off0, er.off1, er.key0, er.key1, r);
    f32x4 z;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const float u1 = (float)((r[2 * h] >> 8) + 1u) * 0x1p-24f, u2 = (float)(r[2 * h + 1] >> 8) * 0x1p-24f;
        const float rad = sqrtf(-2.0f * logf(u1));
        float sn, cs;
        sincosf(6.283185307179586f * u2, &sn, &cs);
        z[2 * h] = rad * cs;
        z[2 * h + 1] = rad * sn;
    }
    return z;
}

// out: kind 0 the pixel noise of elements 4 i .. 4 i + 3 of a batch, kind 1 the four channels' colours of (clip, frame, box) i
__global__ void erase_noise_kernel(EraseTab er, int kind, size_t quads, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < quads) reinterpret_cast<f32x4*>(out)[i] = erase_normals4(er, i, kind == 0 ? 0xE0u : 0xE1u);
}

// What the boxes of clip s (row = its `boxes` table entries) put on the 8-pixel run of frame t, channel c, image row y that starts at
// column x, whose first element is e0 (a multiple of 4): v[p] for every covered pixel p, the later box over the earlier.  Returns
// the bit mask of covered pixels; *bad is set when an entry had to be clamped.  The entries and c are wave-uniform in the
// WAVE_ROW instantiation (scalar loads, clamps in SGPRs); t, y and x are per lane.  Colours cost one Philox call per rand box that
// touches the run, pixel noise one per covered half of the run, after the last box is known.
__device__ __forceinline__ int erase_run(const EraseTab& er, const EraseBox* __restrict__ row, const PatchGeom& pg, int s, int t, int c,
                                         int y, int x, uint64_t e0, float (&v)[8], bool* bad) {
    int cov = 0, pix = 0;
#pragma unroll
    for (int j = 0; j < BVC_ERASE_MAX_BOXES; ++j) {
        if (j >= er.boxes) break;
        const EraseBox e = row[j];
        const int y0 = min(max(e.y0, 0), pg.H), y1 = min(max(e.y1, 0), pg.H), x0 = min(max(e.x0, 0), pg.W), x1 = min(max(e.x1, 0), pg.W);
        const int mode = min(max(e.mode, 0), 2);
        if (y0 != e.y0 || y1 != e.y1 || x0 != e.x0 || x1 != e.x1 || mode != e.mode) *bad = true;
        const int lo = max(x0 - x, 0), hi = min(x1 - x, 8);
        if (y < y0 || y >= y1 || lo >= hi) continue;
        const int m = ((1 << hi) - 1) & ~((1 << lo) - 1);
        cov |= m;
        if (mode == 2) { pix |= m; continue; }
        pix &= ~m;
        float val = 0.f;
        if (mode == 1) val = erase_normals4(er, ((uint64_t)s * pg.T + t) * 4 + j, 0xE1u)[c & 3];
#pragma unroll
        for (int p = 0; p < 8; ++p) v[p] = (m >> p) & 1 ? val : v[p];
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if (!((pix >> (4 * h)) & 15)) continue;
        const f32x4 z = erase_normals4(er, (e0 >> 2) + h, 0xE0u);
#pragma unroll
        for (int p = 0; p < 4; ++p) v[4 * h + p] = (pix >> (4 * h + p)) & 1 ? z[p] : v[4 * h + p];
    }
    return cov;
}

// the run of clip s after erasing: the erased values where a box covers it, the source elsewhere - not loaded when all is covered
__device__ __forceinline__ void erased_pixels8(const PixelSrc& clip, const EraseTab& er, const PatchGeom& pg, int s, int t, int c, int y,
                                               int x, size_t src, f32x4& a, f32x4& d, bool* bad) {
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const int cov = erase_run(er, er.tab + (size_t)s * er.boxes, pg, s, t, c, y, x, (uint64_t)src, v, bad);
    if (cov != 0xff) {
        a = load_pixels4(clip, src, c);
        d = load_pixels4(clip, src + 4, c);
    }
    if (cov) {
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            a[p] = (cov >> p) & 1 ? v[p] : a[p];
            d[p] = (cov >> (p + 4)) & 1 ? v[p + 4] : d[p];
        }
    }
}

// gather_patches_mix_kernel with every clip erased before it is mixed: out = mix entry of clip b applied to erased(b) and
// erased(partner), where erased(s) is clip s with its boxes' content in place of the source (bvc_erase_box).  A clip's erased content
// is a function of (seed, offset, clip, position) only, so it is the same read as `own` and as a `partner`.  As in the mix kernel a
// source is read only where its value is used; of that, a run a box covers whole issues no load and a run no box touches costs the
// box compares alone.  mix == nullptr: no mix (partner b, lam 1, empty box).  Neither table is trusted: boxes are clamped to the
// image and modes to 0 .. 2 before any address or counter is formed, and the first thread of clip b raises bit 0 of *status for
// clip b's entries.
template <bool WAVE_ROW>
__global__ void gather_patches_aug_kernel(const PixelSrc clip, const int* __restrict__ idx, bf16_t* __restrict__ A, int B, int n,
                                          PatchGeom pg, const ClipMix* __restrict__ mix, const EraseTab er, int* __restrict__ status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int K = pg.C * pg.ts * pg.ps * pg.ps;
    const int k8 = K >> 3;
    if (i >= (size_t)B * n * k8) return;
    const int mv = (int)(i / k8);
    const int m = WAVE_ROW ? __builtin_amdgcn_readfirstlane(mv) : mv;
    const int k = (int)(i - (size_t)m * k8) * 8;
    const int dx = k % pg.ps, dy = (k / pg.ps) % pg.ps, dt = (k / (pg.ps * pg.ps)) % pg.ts, c = k / (pg.ps * pg.ps * pg.ts);
    const int b = m / n, tok = idx[m];
    const int wp = pg.W / pg.ps, hp = pg.H / pg.ps;
    const int tp = tok / (hp * wp), yp = (tok / wp) % hp, xp = tok % wp;
    const int t = tp * pg.ts + dt, y = yp * pg.ps + dy, x = xp * pg.ps + dx;
    ClipMix e = ClipMix{b, 1.0f, 0, 0, 0, 0};
    if (mix) e = mix[b];
    const int partner = min(max(e.partner, 0), B - 1);
    const int y0 = min(max(e.y0, 0), pg.H), y1 = min(max(e.y1, 0), pg.H), x0 = min(max(e.x0, 0), pg.W), x1 = min(max(e.x1, 0), pg.W);
    const float lam = e.lam;
    bool bad = partner != e.partner || y0 != e.y0 || y1 != e.y1 || x0 != e.x0 || x1 != e.x1 || !(lam >= 0.f && lam <= 1.f);
    const size_t in_clip = ((((size_t)t) * pg.C + c) * pg.H + y) * pg.W + x;
    const size_t per_clip = (size_t)pg.T * pg.C * pg.H * pg.W;
    const size_t own = (size_t)b * per_clip + in_clip, oth = (size_t)partner * per_clip + in_clip;
    // pixels of the run inside the mix box: [lo, hi) in run coordinates
    const bool row_in = y >= y0 && y < y1;
    const int lo = row_in ? max(x0 - x, 0) : 8, hi = row_in ? min(x1 - x, 8) : 0;
    const bool all_in = lo == 0 && hi == 8, none_in = lo >= hi;
    f32x4 a = {0.f, 0.f, 0.f, 0.f}, d = a, a1 = a, d1 = a;
    bool bad_oth = false;      // the partner's entries are reported by the partner's own first thread
    if (!all_in) erased_pixels8(clip, er, pg, b, t, c, y, x, own, a, d, &bad);
    if (!(none_in && lam == 1.0f)) erased_pixels8(clip, er, pg, partner, t, c, y, x, oth, a1, d1, &bad_oth);
    if (all_in) { a = a1; d = d1; }
    else if (!(none_in && lam == 1.0f)) {
        const float rem = 1.0f - lam;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float ma = lam == 1.0f ? a[j] : lam * a[j] + rem * a1[j];
            const float md = lam == 1.0f ? d[j] : lam * d[j] + rem * d1[j];
            a[j] = (j >= lo && j < hi) ? a1[j] : ma;
            d[j] = (j + 4 >= lo && j + 4 < hi) ? d1[j] : md;
        }
    }
    if (status && k == 0 && m % n == 0) {
        // a run the mix box covers whole did not look at clip b's own entries: check them here
        if (all_in) {
            for (int j = 0; j < er.boxes && j < BVC_ERASE_MAX_BOXES; ++j) {
                const EraseBox q = er.tab[(size_t)b * er.boxes + j];
                bad |= q.y0 < 0 || q.y0 > pg.H || q.y1 < 0 || q.y1 > pg.H || q.x0 < 0 || q.x0 > pg.W || q.x1 < 0 || q.x1 > pg.W ||
                       q.mode < 0 || q.mode > 2;
            }
        }
        if (bad) atomicOr(status, 1);
    }
    *reinterpret_cast<uint4*>(A + (size_t)m * K + k) =
        uint4{pack2bf(a[0], a[1]), pack2bf(a[2], a[3]), pack2bf(d[0], d[1]), pack2bf(d[2], d[3])};
}

// x[i] = NaN for every i when bit 0 of *status is set: how a call whose device-side input check failed reports it without a host sync
__global__ void poison_on_status_kernel(float* __restrict__ x, size_t count, const int* __restrict__ status) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count && (*status & 1)) x[i] = __builtin_nanf("");
}

// ============================================================================ pixel targets (HF:588-661)
// one workgroup per masked token: un-normalise, per-channel mean / unbiased variance over ts*ps*ps
// values, labels[(dt,dy,dx,c)] = (f - mean) / (sqrt(var) + 1e-6)
__global__ __launch_bounds__(256) void labels_kernel(const PixelSrc clip, const int* __restrict__ dec_idx,
                                                     float* __restrict__ labels, int ndec, PatchGeom pg, int norm_pix) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* buf = reinterpret_cast<float*>(smem);   // [C][E]
    const int E = pg.ts * pg.ps * pg.ps, C = pg.C;
    float* stat = buf + C * E;                     // [C][2]
    // (one workgroup per token on purpose: a grid-stride form with 4096 workgroups measured 1565 vs 1413 us at 256 clips - the
    //  load -> barrier -> statistics -> barrier -> store chain of a token hides its latency only behind OTHER workgroups)
    // XCD-aware order (round 4): a patch row is 64 B, half of a 128-B line whose other half belongs to the next token in x - usually the
    // next masked token of the clip.  Workgroups b and b + 1 run on different XCDs (different L2s), so with m = blockIdx.x both fetched
    // the line: 4.45 GB read for 2.2 GB of pixels at 256 clips.  Each XCD takes a contiguous run of tokens instead.
    const int nb = gridDim.x, xq = nb >> 3, xr = nb & 7, xcd = blockIdx.x & 7;
    const int m = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + (blockIdx.x >> 3);
    const int b = m / ndec, tok = dec_idx[m];
    const int wp = pg.W / pg.ps, hp = pg.H / pg.ps;
    const int tp = tok / (hp * wp), yp = (tok / wp) % hp, xp = tok % wp;
    const float mean3[3] = {0.485f, 0.456f, 0.406f}, std3[3] = {0.229f, 0.224f, 0.225f};
    const int e4n = E >> 2;
    for (int i = threadIdx.x; i < C * e4n; i += 256) {
        const int c = i / e4n, e = (i % e4n) * 4;
        const int dx = e % pg.ps, dy = (e / pg.ps) % pg.ps, dt = e / (pg.ps * pg.ps);
        const size_t src = ((((size_t)b * pg.T + tp * pg.ts + dt) * C + c) * pg.H + yp * pg.ps + dy) * pg.W + xp * pg.ps + dx;
        f32x4 v = load_pixels4(clip, src, c);
        if (C == 3) v = v * std3[c] + mean3[c];
        *reinterpret_cast<f32x4*>(buf + c * E + e) = v;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c = wave; c < C; c += 4) {
        float s = 0.f;
        for (int e = lane; e < E; e += 64) s += buf[c * E + e];
        const float mu = wave_sum(s) / E;
        float q = 0.f;
        for (int e = lane; e < E; e += 64) { const float d = buf[c * E + e] - mu; q += d * d; }
        const float var = wave_sum(q) / (E - 1);
        if (lane == 0) { stat[2 * c] = norm_pix ? mu : 0.f; stat[2 * c + 1] = norm_pix ? sqrtf(var) + 1e-6f : 1.f; }
    }
    __syncthreads();
    float* out = labels + (size_t)m * C * E;
    for (int o = threadIdx.x * 4; o < C * E; o += 1024) {
        f32x4 r;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = (o + j) / C, c = (o + j) % C;
            r[j] = (buf[c * E + e] - stat[2 * c]) / stat[2 * c + 1];
        }
        *reinterpret_cast<f32x4*>(out + o) = r;
    }
}

// The same targets, one WAVE per masked token (round 4).  The workgroup-per-token form above keeps 8 tokens (48 KB of reads) in flight
// per CU and chains load -> barrier -> statistics -> barrier -> store inside each: 1.41 ms at 256 clips for 4.7 GB = 3.3 TB/s.  Here a
// token's 1536 values are loaded by one wave (NCH 16-byte chunks per lane, all in flight together), parked in the wave's own LDS rows
// and never meet a workgroup barrier; 24 tokens per CU are in flight.  Same arithmetic in the same order as labels_kernel (per channel:
// lane-strided sums, wave_sum, two passes), so the labels are bit-identical.  Tokens are taken XCD by XCD like above.
template <int NCH>
__global__ __launch_bounds__(256, 6) void labels_wave_kernel(const PixelSrc clip, const int* __restrict__ dec_idx,
                                                          float* __restrict__ labels, int ntok, int ndec, PatchGeom pg, int norm_pix) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int E = pg.ts * pg.ps * pg.ps, C = pg.C;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int per_wave = C * E + 2 * C + ((4 - ((C * E + 2 * C) & 3)) & 3);         // floats, kept a multiple of 16 bytes
    float* buf = reinterpret_cast<float*>(smem) + wave * per_wave;                   // [C][E]
    float* stat = buf + C * E;                                                       // [C][2]
    const int nb = gridDim.x, xq = nb >> 3, xr = nb & 7, xcd = blockIdx.x & 7;
    const int blk = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + (blockIdx.x >> 3);
    const int m = blk * 4 + wave;
    if (m >= ntok) return;                       // whole waves leave; nothing below synchronises across waves
    const int b = m / ndec, tok = dec_idx[m];
    const int wp = pg.W / pg.ps, hp = pg.H / pg.ps;
    const int tp = tok / (hp * wp), yp = (tok / wp) % hp, xp = tok % wp;
    const float mean3[3] = {0.485f, 0.456f, 0.406f}, std3[3] = {0.229f, 0.224f, 0.225f};
    const int e4n = E >> 2, nchunk = C * e4n;
    f32x4 v[NCH];
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        const int i = lane + 64 * k;
        if (i < nchunk) {
            const int c = i / e4n, e = (i % e4n) * 4;
            const int dx = e % pg.ps, dy = (e / pg.ps) % pg.ps, dt = e / (pg.ps * pg.ps);
            const size_t src = ((((size_t)b * pg.T + tp * pg.ts + dt) * C + c) * pg.H + yp * pg.ps + dy) * pg.W + xp * pg.ps + dx;
            v[k] = load_pixels4(clip, src, c);
        }
    }
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        const int i = lane + 64 * k;
        if (i < nchunk) {
            const int c = i / e4n, e = (i % e4n) * 4;
            f32x4 w = v[k];
            if (C == 3) w = w * std3[c] + mean3[c];
            *reinterpret_cast<f32x4*>(buf + c * E + e) = w;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    for (int c = 0; c < C; ++c) {
        float s = 0.f;
        for (int e = lane; e < E; e += 64) s += buf[c * E + e];
        const float mu = wave_sum(s) / E;
        float q = 0.f;
        for (int e = lane; e < E; e += 64) { const float d = buf[c * E + e] - mu; q += d * d; }
        const float var = wave_sum(q) / (E - 1);
        if (lane == 0) { stat[2 * c] = norm_pix ? mu : 0.f; stat[2 * c + 1] = norm_pix ? sqrtf(var) + 1e-6f : 1.f; }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    float* out = labels + (size_t)m * C * E;
    for (int o = lane * 4; o < C * E; o += 256) {
        f32x4 r;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = (o + j) / C, c = (o + j) % C;
            r[j] = (buf[c * E + e] - stat[2 * c]) / stat[2 * c + 1];
        }
        *reinterpret_cast<f32x4*>(out + o) = r;
    }
}

// Three channels, E a multiple of 256 (the reference's 2 x 16 x 16 tubes: E = 512) - the same wave-per-token form with the arithmetic
// cut down (round 4): the strip experiment (profiles/r04_y_labels_strip_kernel.patch.txt) showed that a token cost a wave ~20 us of
// vector work, not of memory time.  Here (a) the statistics come from the lane's own registers (a lane's chunks k = 2c, 2c + 1 are channel
// c: eight values per channel, two-pass mean / unbiased variance with one wave_sum each) instead of 48 LDS reads; (b) C is a constant, so
// the (element, channel) of an output position costs a multiply-shift instead of a runtime division (24 of them per lane before);
// (c) one IEEE division per channel (1 / (sqrt(var) + 1e-6)) and a multiply per value instead of a division per value: within one f32
// rounding of (f - mean) / (sqrt(var) + 1e-6).  The per-lane channel of output position 4 lane + 256 k + j is (lane + k + j) mod 3, so
// with the channel statistics rotated by lane mod 3 once, every use is a compile-time register.
template <int NE>      // NE = E / 256: chunks per lane and channel
__global__ __launch_bounds__(256, 6) void labels_wave3_kernel(const PixelSrc clip, const int* __restrict__ dec_idx, float* __restrict__ labels,
                                                              int ntok, int ndec, PatchGeom pg, int norm_pix) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int C = 3, E = 256 * NE, CE = C * E, NCH = C * NE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float* buf = reinterpret_cast<float*>(smem) + wave * CE;                          // [C][E], this wave's token
    const int nb = gridDim.x, xq = nb >> 3, xr = nb & 7, xcd = blockIdx.x & 7;
    const int blk = (xcd < xr ? xcd * (xq + 1) : xr * (xq + 1) + (xcd - xr) * xq) + (blockIdx.x >> 3);
    const int m = blk * 4 + wave;
    if (m >= ntok) return;
    const int b = m / ndec, tok = dec_idx[m];
    const int wp = pg.W / pg.ps, hp = pg.H / pg.ps;
    const int tp = tok / (hp * wp), yp = (tok / wp) % hp, xp = tok % wp;
    const float mean3[3] = {0.485f, 0.456f, 0.406f}, std3[3] = {0.229f, 0.224f, 0.225f};
    f32x4 v[NCH];
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        constexpr int e4n = E / 4;
        const int i = lane + 64 * k;
        const int c = k / NE, e = (i - c * e4n) * 4;                 // (64 NE chunks per channel: chunk k of a lane is channel k / NE)
        const int dx = e % pg.ps, dy = (e / pg.ps) % pg.ps, dt = e / (pg.ps * pg.ps);
        const size_t src = ((((size_t)b * pg.T + tp * pg.ts + dt) * C + c) * pg.H + yp * pg.ps + dy) * pg.W + xp * pg.ps + dx;
        v[k] = load_pixels4(clip, src, c);
    }
    float mu[3], rinv[3];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        float sm = 0.f;
#pragma unroll
        for (int k = c * NE; k < (c + 1) * NE; ++k) {
            v[k] = v[k] * std3[c] + mean3[c];
            *reinterpret_cast<f32x4*>(buf + c * E + (lane + 64 * (k - c * NE)) * 4) = v[k];
            sm += (v[k][0] + v[k][1]) + (v[k][2] + v[k][3]);
        }
        const float mean = wave_sum(sm) * (1.0f / E);
        float q = 0.f;
#pragma unroll
        for (int k = c * NE; k < (c + 1) * NE; ++k)
#pragma unroll
            for (int j = 0; j < 4; ++j) { const float d = v[k][j] - mean; q += d * d; }
        const float var = wave_sum(q) / (float)(E - 1);
        mu[c] = norm_pix ? mean : 0.f;
        rinv[c] = norm_pix ? 1.0f / (sqrtf(var) + 1e-6f) : 1.f;
    }
    // statistics rotated by lane mod 3: mr[i] = mu[(lane + i) mod 3]
    const int l3 = lane % 3;
    float mr[3], rr[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const int c = l3 + i;      // 0 .. 4
        mr[i] = (c == 0 || c == 3) ? mu[0] : (c == 1 || c == 4) ? mu[1] : mu[2];
        rr[i] = (c == 0 || c == 3) ? rinv[0] : (c == 1 || c == 4) ? rinv[1] : rinv[2];
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    float* out = labels + (size_t)m * CE;
#pragma unroll
    for (int k = 0; k < CE / 256; ++k) {
        const int o = lane * 4 + 256 * k;
        f32x4 r;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int t = o + j, e = t / 3, c = t - 3 * e;           // output position t = e * C + c
            r[j] = (buf[c * E + e] - mr[(k + j) % 3]) * rr[(k + j) % 3];
        }
        *reinterpret_cast<f32x4*>(out + o) = r;
    }
}

// x_full[b][nvis + j][:] = mask_token + pos[dec_idx[b][j]]   (HF:580-582)
__global__ void fill_masked_kernel(float* __restrict__ xfull, const float* __restrict__ mask_token, const float* __restrict__ pos,
                                   const int* __restrict__ dec_idx, int B, int Ld, int nvis, int ndec, int D) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int nch = D >> 2;
    if (i >= (size_t)B * ndec * nch) return;
    const int m = (int)(i / nch), c = (int)(i % nch);
    const int b = m / ndec, j = m % ndec;
    const f32x4 mt = reinterpret_cast<const f32x4*>(mask_token)[c];
    const f32x4 pe = reinterpret_cast<const f32x4*>(pos + (size_t)dec_idx[m] * D)[c];
    reinterpret_cast<f32x4*>(xfull + ((size_t)b * Ld + nvis + j) * D)[c] = mt + pe;
}

// ============================================================================ first decoder layer by position (stack.h LayerFirst)
// dec_slot[b][p] = j where dec_idx[b][j] == p; the caller fills dec_slot with -1 first (positions clip b does not decode keep it)
__global__ void dec_slot_kernel(const int* __restrict__ dec_idx, int* __restrict__ dec_slot, int B, int L, int ndec) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)B * ndec) return;
    const int b = (int)(i / ndec), p = dec_idx[i];
    if ((unsigned)p < (unsigned)L) dec_slot[(size_t)b * L + p] = (int)(i % ndec);
}

// qkv[b][r][:] = r < nvis ? qkv_vis[b][r][:] : t2[dec_idx[b][r - nvis]][:]  (bf16, W columns, 16 bytes per item), and
// x_full[b][nvis + j][:] = t0[dec_idx[b][j]][:]                             (f32, D columns: what fill_masked_kernel writes)
__global__ void first_assemble_kernel(const bf16_t* __restrict__ qkv_vis, const bf16_t* __restrict__ t2, const float* __restrict__ t0,
                                      const int* __restrict__ dec_idx, bf16_t* __restrict__ qkv, float* __restrict__ xfull, int B,
                                      int nvis, int ndec, int W, int D) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int wch = W >> 3, dch = D >> 2, Ld = nvis + ndec;
    const size_t n1 = (size_t)B * Ld * wch;
    if (i < n1) {
        const size_t row = i / wch;
        const int c = (int)(i % wch), b = (int)(row / Ld), r = (int)(row % Ld);
        const bf16_t* src = r < nvis ? qkv_vis + ((size_t)b * nvis + r) * W : t2 + (size_t)dec_idx[(size_t)b * ndec + (r - nvis)] * W;
        reinterpret_cast<uint4*>(qkv + row * W)[c] = reinterpret_cast<const uint4*>(src)[c];
        return;
    }
    const size_t j = i - n1;
    if (j >= (size_t)B * ndec * dch) return;
    const size_t m = j / dch;
    const int c = (int)(j % dch), b = (int)(m / ndec), jj = (int)(m % ndec);
    reinterpret_cast<f32x4*>(xfull + ((size_t)b * Ld + nvis + jj) * D)[c] = reinterpret_cast<const f32x4*>(t0 + (size_t)dec_idx[m] * D)[c];
}

// S[p][c] = sum over the clips b = 0 .. B-1, in that order, of dqkv[b][nvis + dec_slot[b][p]][c] (clips with slot -1 add nothing), f32.
// One wave per (position, 512 columns), 16 bytes per lane and clip; eight clips' rows are in flight before they are added, in clip
// order.  Outputs (each optional): S as f32, and its bf16 pair hi = bf16(S), lo = bf16(S - hi).
constexpr int kFirstReduceClips = 8;
__global__ __launch_bounds__(64) void first_reduce_kernel(const bf16_t* __restrict__ dqkv, const int* __restrict__ dec_slot, int B, int L,
                                                          int Ld, int nvis, int W, float* __restrict__ S, bf16_t* __restrict__ hi,
                                                          bf16_t* __restrict__ lo) {
    const int p = blockIdx.x, col = (blockIdx.y * 64 + threadIdx.x) * 8;
    if (col >= W) return;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int b0 = 0; b0 < B; b0 += kFirstReduceClips) {
        uint4 v[kFirstReduceClips];
#pragma unroll
        for (int u = 0; u < kFirstReduceClips; ++u) {
            const int b = b0 + u;
            const int slot = b < B ? dec_slot[(size_t)b * L + p] : -1;
            v[u] = slot >= 0 ? *reinterpret_cast<const uint4*>(dqkv + ((size_t)b * Ld + nvis + slot) * W + col) : uint4{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int u = 0; u < kFirstReduceClips; ++u) {
            const uint32_t w[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                acc[2 * e] += __uint_as_float(w[e] << 16);
                acc[2 * e + 1] += __uint_as_float(w[e] & 0xffff0000u);
            }
        }
    }
    const size_t o = (size_t)p * W + col;
    if (S) {
        *reinterpret_cast<f32x4*>(S + o) = f32x4{acc[0], acc[1], acc[2], acc[3]};
        *reinterpret_cast<f32x4*>(S + o + 4) = f32x4{acc[4], acc[5], acc[6], acc[7]};
    }
    if (hi) {
        uint32_t h[4], l[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            h[e] = pack2bf(acc[2 * e], acc[2 * e + 1]);
            l[e] = pack2bf(acc[2 * e] - __uint_as_float(h[e] << 16), acc[2 * e + 1] - __uint_as_float(h[e] & 0xffff0000u));
        }
        *reinterpret_cast<uint4*>(hi + o) = uint4{h[0], h[1], h[2], h[3]};
        *reinterpret_cast<uint4*>(lo + o) = uint4{l[0], l[1], l[2], l[3]};
    }
}

// out bf16 [M][W] = in bf16 [map_row(m)][W]
__global__ void gather_rows_copy_bf16_kernel(const bf16_t* __restrict__ in, RowMap rm, bf16_t* __restrict__ out, int M, int W) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;   // 16-byte item
    const int nch = W >> 3;
    if (i >= (size_t)M * nch) return;
    const int m = (int)(i / nch), c = (int)(i % nch);
    reinterpret_cast<uint4*>(out + (size_t)m * W)[c] = reinterpret_cast<const uint4*>(in + (size_t)map_row(m, rm) * W)[c];
}

// v = a + b (b may be null; n float4 items each) as a bf16 pair: hi = bf16(v), lo = bf16(v - hi)
__global__ void pair_split_kernel(const float* __restrict__ a, const float* __restrict__ b, bf16_t* __restrict__ hi, bf16_t* __restrict__ lo,
                                  size_t n) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;   // float4 item
    if (i >= n) return;
    f32x4 v = reinterpret_cast<const f32x4*>(a)[i];
    if (b) v += reinterpret_cast<const f32x4*>(b)[i];
    const uint32_t h0 = pack2bf(v[0], v[1]), h1 = pack2bf(v[2], v[3]);
    const uint32_t l0 = pack2bf(v[0] - __uint_as_float(h0 << 16), v[1] - __uint_as_float(h0 & 0xffff0000u));
    const uint32_t l1 = pack2bf(v[2] - __uint_as_float(h1 << 16), v[3] - __uint_as_float(h1 & 0xffff0000u));
    reinterpret_cast<uint2*>(hi)[i] = uint2{h0, h1};
    reinterpret_cast<uint2*>(lo)[i] = uint2{l0, l1};
}

// loss = sum(partials) / count, fixed summation order; NaN if the mask index kernel flagged a bad mask
__global__ __launch_bounds__(256) void loss_finalize_kernel(const float* __restrict__ partial, int n, double count,
                                                            const int* __restrict__ status, float* __restrict__ loss) {
    __shared__ double red[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += (double)partial[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) *loss = (status && *status) ? __int_as_float(0x7fc00000) : (float)(red[0] / count);
}

// ============================================================================ JEPA pieces
// token gather with an index list: logical row m of a [nsets*B*n] output reads x[(b*L + idx[m])] where b = (m / n) % B;
// used as RowGather in the target selection below
// targets (pretrain_jepa.py:384-392): h = layer_norm(target_encoder(imgs)) without affine, rows picked by the 4 prediction
// masks, set-major then sample:  out[(i*B + b)*Np + j] = LN(h[b*L + idx[(i*B + b)*Np + j]]).  One wave per row.
template <int NC>
__global__ __launch_bounds__(256) void target_select_kernel(const float* __restrict__ h, const int* __restrict__ idx,
                                                            float* __restrict__ out, int rows, int B, int Np, int L, int D, float eps) {
    const int lane = threadIdx.x & 63, m = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= rows) return;
    const int b = (m / Np) % B;
    const f32x4* xr = reinterpret_cast<const f32x4*>(h + ((size_t)b * L + idx[m]) * D);
    const int nch = D >> 2;
    f32x4 v[NC];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        const int c = lane + 64 * i;
        if (c < nch) { v[i] = xr[c]; s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]); }
    }
    const float mu = wave_sum(s) / D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        const int c = lane + 64 * i;
        if (c < nch) {
#pragma unroll
            for (int e = 0; e < 4; ++e) { const float d = v[i][e] - mu; q += d * d; }
        }
    }
    const float rs = rsqrtf(wave_sum(q) / D + eps);
    f32x4* o = reinterpret_cast<f32x4*>(out + (size_t)m * D);
#pragma unroll
    for (int i = 0; i < NC; ++i) {
        const int c = lane + 64 * i;
        if (c < nch) o[c] = (v[i] - mu) * rs;
    }
}

// predictor input (vision_transformer.py:507-524): sequence s = i*B + b is [ctx tokens of sample b ; mask_token + pos[pred idx]]
__global__ void pred_assemble_kernel(const float* __restrict__ xe, const float* __restrict__ mask_token, const float* __restrict__ pos,
                                     const int* __restrict__ idx_pred, float* __restrict__ X, int nseq, int B, int Nc, int Np, int D) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int nch = D >> 2, T = Nc + Np;
    if (i >= (size_t)nseq * T * nch) return;
    const int c = (int)(i % nch);
    const int t = (int)((i / nch) % T), sq = (int)(i / ((size_t)nch * T));
    f32x4 v;
    if (t < Nc) {
        v = reinterpret_cast<const f32x4*>(xe + ((size_t)(sq % B) * Nc + t) * D)[c];
    } else {
        v = reinterpret_cast<const f32x4*>(mask_token)[c] + reinterpret_cast<const f32x4*>(pos + (size_t)idx_pred[(size_t)sq * Np + (t - Nc)] * D)[c];
    }
    reinterpret_cast<f32x4*>(X + ((size_t)sq * T + t) * D)[c] = v;
}

// gradient of the replicated context tokens: dxe[b*Nc + t] = sum_i dX[(i*B + b)][t]  -> bf16 (GEMM operand)
__global__ void pred_ctx_grad_kernel(const float* __restrict__ dX, bf16_t* __restrict__ dxe, int nsets, int B, int Nc, int Np, int D) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int nch = D >> 2, T = Nc + Np;
    if (i >= (size_t)B * Nc * nch) return;
    const int c = (int)(i % nch);
    const int t = (int)((i / nch) % Nc), b = (int)(i / ((size_t)nch * Nc));
    f32x4 a = {0, 0, 0, 0};
    for (int k = 0; k < nsets; ++k) a += reinterpret_cast<const f32x4*>(dX + (((size_t)k * B + b) * T + t) * D)[c];
    reinterpret_cast<uint2*>(dxe + ((size_t)b * Nc + t) * D)[c] = uint2{pack2bf(a[0], a[1]), pack2bf(a[2], a[3])};
}

// smooth-L1 (beta = 1, mean; pretrain_jepa.py:399-402): per-block partial sums, folded by loss_finalize_kernel
__global__ __launch_bounds__(256) void smooth_l1_fwd_kernel(const float* __restrict__ z, const float* __restrict__ h, size_t n,
                                                            float* __restrict__ partial) {
    __shared__ float red[4];
    float s = 0.f;
    for (size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4; i < n; i += (size_t)gridDim.x * 1024) {
        if (i + 4 <= n) {
            const f32x4 d = *reinterpret_cast<const f32x4*>(z + i) - *reinterpret_cast<const f32x4*>(h + i);
#pragma unroll
            for (int e = 0; e < 4; ++e) { const float a = fabsf(d[e]); s += a < 1.f ? 0.5f * a * a : a - 0.5f; }
        } else {
            for (size_t j = i; j < n; ++j) { const float a = fabsf(z[j] - h[j]); s += a < 1.f ? 0.5f * a * a : a - 0.5f; }
        }
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// dz = gout / n * clamp(z - h, -1, 1)
__global__ void smooth_l1_bwd_kernel(const float* __restrict__ z, const float* __restrict__ h, const float* __restrict__ gout,
                                     size_t n, float* __restrict__ dz) {
    const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= n) return;
    const float g = gout[0] / (float)n;
    if (i + 4 <= n) {
        const f32x4 d = *reinterpret_cast<const f32x4*>(z + i) - *reinterpret_cast<const f32x4*>(h + i);
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = g * fminf(fmaxf(d[e], -1.f), 1.f);
        *reinterpret_cast<f32x4*>(dz + i) = o;
    } else {
        for (size_t j = i; j < n; ++j) dz[j] = g * fminf(fmaxf(z[j] - h[j], -1.f), 1.f);
    }
}

// momentum update of the target encoder (pretrain_jepa.py:426-432): k = m * k + (1 - m) * q over a flat range
__global__ void ema_kernel(float* __restrict__ k, const float* __restrict__ q, size_t n, float m) {
    const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= n) return;
    if (i + 4 <= n) {
        const f32x4 kv = *reinterpret_cast<f32x4*>(k + i), qv = *reinterpret_cast<const f32x4*>(q + i);
        *reinterpret_cast<f32x4*>(k + i) = kv * m + qv * (1.f - m);
    } else {
        for (size_t j = i; j < n; ++j) k[j] = k[j] * m + q[j] * (1.f - m);
    }
}

// idx[b*L + t] = t  (identity token list: "all tokens" for the target encoder)
__global__ void iota_mod_kernel(int* __restrict__ idx, int n, int L) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) idx[i] = i % L;
}

// ============================================================================ SimCLR loss pieces
// fn = f / max(||f||, eps) in bf16 (operand of the similarity GEMM), inv[i] = 1 / max(||f_i||, eps);
// F.cosine_similarity semantics (pretraining/contrastive/pretrain_simclr.py:116).  One wave per row.
__global__ __launch_bounds__(256) void row_normalize_kernel(const float* __restrict__ f, bf16_t* __restrict__ fn,
                                                            float* __restrict__ inv, int n, int p, float eps) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const f32x4* fr = reinterpret_cast<const f32x4*>(f + (size_t)row * p);
    float ss = 0.f;
    for (int c = lane; c < p / 4; c += 64) { const f32x4 v = fr[c]; ss += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3]; }
    const float r = 1.f / fmaxf(sqrtf(wave_sum(ss)), eps);
    if (lane == 0) inv[row] = r;
    uint2* o = reinterpret_cast<uint2*>(fn + (size_t)row * p);
    for (int c = lane; c < p / 4; c += 64) { const f32x4 v = fr[c] * r; o[c] = uint2{pack2bf(v[0], v[1]), pack2bf(v[2], v[3])}; }
}

// df = inv * (dfn - fhat * (fhat . dfn)),  fhat = f * inv   (backward of the row normalisation)
__global__ __launch_bounds__(256) void row_normalize_bwd_kernel(const float* __restrict__ f, const float* __restrict__ inv,
                                                                const float* __restrict__ dfn, float* __restrict__ df, int n, int p) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= n) return;
    const f32x4* fr = reinterpret_cast<const f32x4*>(f + (size_t)row * p);
    const f32x4* gr = reinterpret_cast<const f32x4*>(dfn + (size_t)row * p);
    const float r = inv[row];
    float dot = 0.f;
    for (int c = lane; c < p / 4; c += 64) { const f32x4 a = fr[c] * r, g = gr[c]; dot += a[0] * g[0] + a[1] * g[1] + a[2] * g[2] + a[3] * g[3]; }
    dot = wave_sum(dot);
    f32x4* o = reinterpret_cast<f32x4*>(df + (size_t)row * p);
    for (int c = lane; c < p / 4; c += 64) { const f32x4 a = fr[c] * r; o[c] = (gr[c] - a * dot) * r; }
}

// loss = logsumexp(negatives) - mean(positives) from the per-tile partials of the EPI_NCE similarity GEMM
// (partial[2t] = sum exp(s - 1/T) over negatives, partial[2t+1] = sum s over positives); stats = {lse, -1/npos}
__global__ __launch_bounds__(256) void nce_finalize_kernel(const float* __restrict__ partial, int ntiles, float inv_t,
                                                           double npos, float* __restrict__ loss, float* __restrict__ stats) {
    __shared__ double red[2][256];
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < ntiles; i += 256) { a += (double)partial[2 * i]; b += (double)partial[2 * i + 1]; }
    red[0][threadIdx.x] = a; red[1][threadIdx.x] = b;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (threadIdx.x < o) { red[0][threadIdx.x] += red[0][threadIdx.x + o]; red[1][threadIdx.x] += red[1][threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double lse = (double)inv_t + log(red[0][0]);
        *loss = (float)(lse - red[1][0] / npos);
        stats[0] = (float)lse;
        stats[1] = (float)(-1.0 / npos);
    }
}

// ============================================================================ fused SGD (momentum / Nesterov)
// torch.optim.SGD semantics (pretrain_videomae.py:187-189) over a flat range, one pass:
//   g = grad / grad_scale (+ wd * p);  buf = first ? g : m * buf + (1 - damp) * g;  d = nesterov ? g + m * buf : buf;
//   p -= lr * d;   the unscaled gradient is written back (what grad_logger reads after scaler.step).
// Skips everything when *found_inf != 0 (GradScaler's contract for optimisers with _step_supports_amp_scaling).
__global__ void sgd_step_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ buf, size_t n, float lr,
                                float momentum, float dampening, float wd, int nesterov, int first, int maximize,
                                const float* __restrict__ grad_scale, const float* __restrict__ found_inf, int write_grad,
                                bf16_t* __restrict__ shadow) {
    if (found_inf && *found_inf != 0.f) return;
    const float inv = grad_scale ? 1.f / *grad_scale : 1.f;
    const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= n) return;
    if (i + 4 <= n) {
        f32x4 pv = *reinterpret_cast<f32x4*>(p + i);
        f32x4 gv = *reinterpret_cast<f32x4*>(g + i) * inv;
        if (maximize) gv = -gv;
        const f32x4 gu = gv;
        if (wd != 0.f) gv += pv * wd;
        f32x4 d = gv;
        if (momentum != 0.f) {
            f32x4 bv = first ? gv : *reinterpret_cast<f32x4*>(buf + i) * momentum + gv * (1.f - dampening);
            *reinterpret_cast<f32x4*>(buf + i) = bv;
            d = nesterov ? gv + bv * momentum : bv;
        }
        const f32x4 pn = pv - d * lr;
        *reinterpret_cast<f32x4*>(p + i) = pn;
        // the bf16 copy the next forward's products read (round 4): written here, the per-forward cast pass over all parameters goes
        if (shadow) *reinterpret_cast<uint2*>(shadow + i) = uint2{pack2bf(pn[0], pn[1]), pack2bf(pn[2], pn[3])};
        if (write_grad) *reinterpret_cast<f32x4*>(g + i) = gu;
    } else {
        for (size_t j = i; j < n; ++j) {
            float gv = g[j] * inv;
            if (maximize) gv = -gv;
            const float gu = gv;
            if (wd != 0.f) gv += p[j] * wd;
            float d = gv;
            if (momentum != 0.f) {
                const float bv = first ? gv : buf[j] * momentum + gv * (1.f - dampening);
                buf[j] = bv;
                d = nesterov ? gv + bv * momentum : bv;
            }
            p[j] -= lr * d;
            if (shadow) shadow[j] = f2bf(p[j]);
            if (write_grad) g[j] = gu;
        }
    }
}

// torch.optim.Adam / AdamW (pretrain_videomae.py:190-193: AdamW(betas=(0.9, 0.95)) / Adam) over a flat range.
// adam_prep: state[0] = step count (f32, advanced unless *found_inf != 0), state[1] = lr / (1 - beta1^step),
// state[2] = sqrt(1 - beta2^step) - the scalars torch derives in double on the host, derived in double here
__global__ void adam_prep_kernel(float* __restrict__ state, double lr, double beta1, double beta2, const float* __restrict__ found_inf) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (found_inf && *found_inf != 0.f) return;
    const double step = (double)state[0] + 1.0;
    state[0] = (float)step;
    state[1] = (float)(lr / (1.0 - pow(beta1, step)));
    state[2] = (float)sqrt(1.0 - pow(beta2, step));
}

//   g = grad / grad_scale;  AdamW: p *= 1 - lr wd;  Adam: g += wd p;  m += (g - m)(1 - b1);  v = b2 v + (1 - b2) g^2;
//   p -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps)            (torch/optim/adam.py _single_tensor_adam, same operation order)
__global__ void adam_step_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                 size_t n, float omb1, float beta2, float omb2, float eps, float wd, float decay_mul, int decoupled,
                                 int maximize, const float* __restrict__ state, const float* __restrict__ grad_scale,
                                 const float* __restrict__ found_inf, int write_grad, bf16_t* __restrict__ shadow) {
    if (found_inf && *found_inf != 0.f) return;
    const float inv = grad_scale ? 1.f / *grad_scale : 1.f;
    const float step_size = state[1], bc2s = state[2];
    const size_t i0 = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i0 >= n) return;
    const bool vec = i0 + 4 <= n;
    float pv[4], gv[4], mv[4], vv[4];
    const int cnt = vec ? 4 : (int)(n - i0);
    if (vec) {
        *reinterpret_cast<f32x4*>(pv) = *reinterpret_cast<const f32x4*>(p + i0);
        *reinterpret_cast<f32x4*>(gv) = *reinterpret_cast<const f32x4*>(g + i0);
        *reinterpret_cast<f32x4*>(mv) = *reinterpret_cast<const f32x4*>(m + i0);
        *reinterpret_cast<f32x4*>(vv) = *reinterpret_cast<const f32x4*>(v + i0);
    } else {
        for (int e = 0; e < cnt; ++e) { pv[e] = p[i0 + e]; gv[e] = g[i0 + e]; mv[e] = m[i0 + e]; vv[e] = v[i0 + e]; }
    }
    float gu[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float gr = gv[e] * inv;
        if (maximize) gr = -gr;
        gu[e] = gr;
        float pe = pv[e];
        if (wd != 0.f) {
            if (decoupled) pe *= decay_mul; else gr += wd * pe;
        }
        const float me = mv[e] + omb1 * (gr - mv[e]);
        const float ve = vv[e] * beta2 + omb2 * (gr * gr);
        const float denom = sqrtf(ve) / bc2s + eps;
        pv[e] = pe - step_size * (me / denom);
        mv[e] = me; vv[e] = ve;
    }
    if (vec) {
        *reinterpret_cast<f32x4*>(p + i0) = *reinterpret_cast<f32x4*>(pv);
        *reinterpret_cast<f32x4*>(m + i0) = *reinterpret_cast<f32x4*>(mv);
        *reinterpret_cast<f32x4*>(v + i0) = *reinterpret_cast<f32x4*>(vv);
        if (shadow) *reinterpret_cast<uint2*>(shadow + i0) = uint2{pack2bf(pv[0], pv[1]), pack2bf(pv[2], pv[3])};
        if (write_grad) *reinterpret_cast<f32x4*>(g + i0) = *reinterpret_cast<f32x4*>(gu);
    } else {
        for (int e = 0; e < cnt; ++e) {
            p[i0 + e] = pv[e]; m[i0 + e] = mv[e]; v[i0 + e] = vv[e];
            if (shadow) shadow[i0 + e] = f2bf(pv[e]);
            if (write_grad) g[i0 + e] = gu[e];
        }
    }
}

// ============================================================================ the same updates over a flat buffer with PARAMETER GROUPS
// The reference's JEPA optimiser has four groups (pretraining/predictive/helper.py:123-147: encoder / predictor weights with weight
// decay, their biases and 1-D tensors with weight_decay 0) and the flat layout interleaves weights and biases: a launch per run of
// memory-adjacent parameters of one group would be ~9 launches per layer.  Here ONE launch covers the whole flat buffer: a static
// table cuts it into segments (seg_start[s] .. seg_start[s + 1], ascending, element offsets) owned by group seg_group[s] (-1: no
// group - frozen parameters, padding - left untouched), blk_seg[b] is the segment that holds element 1024 b (so that a thread
// finds its segment in one or two steps), and the groups' hyper-parameters travel by value as kernel arguments (they change per
// step under a schedule; the table does not).  A quad of elements inside one segment takes the vector path - the same arithmetic,
// statement for statement, as sgd_step_kernel / adam_step_kernel -, a quad that straddles a boundary goes element by element.
struct SgdGroupsDev {
    float lr[BVC_OPT_MAX_GROUPS], wd[BVC_OPT_MAX_GROUPS], momentum[BVC_OPT_MAX_GROUPS], dampening[BVC_OPT_MAX_GROUPS];
    int flags[BVC_OPT_MAX_GROUPS];      // 1 = nesterov, 2 = maximize, 4 = first step (buf = g)
};
struct AdamGroupsDev {
    float omb1[BVC_OPT_MAX_GROUPS], beta2[BVC_OPT_MAX_GROUPS], omb2[BVC_OPT_MAX_GROUPS], eps[BVC_OPT_MAX_GROUPS], wd[BVC_OPT_MAX_GROUPS],
        decay_mul[BVC_OPT_MAX_GROUPS];
    int flags[BVC_OPT_MAX_GROUPS];      // 1 = decoupled (AdamW), 2 = maximize
};

// hyper-parameter of group `grp` out of a by-value table: a select chain (kernel arguments live in scalar registers and cannot be
// indexed by a per-lane value without a trip through scratch)
template <typename T>
__device__ __forceinline__ T pick_group(const T (&tab)[BVC_OPT_MAX_GROUPS], int grp) {
    T v = tab[0];
#pragma unroll
    for (int i = 1; i < BVC_OPT_MAX_GROUPS; ++i) v = grp == i ? tab[i] : v;
    return v;
}

__device__ __forceinline__ int find_segment(const int64_t* __restrict__ seg_start, int s, int64_t i) {
    while (seg_start[s + 1] <= i) ++s;
    return s;
}

__global__ __launch_bounds__(256) void sgd_step_seg_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ buf, int64_t n,
                                                           const int64_t* __restrict__ seg_start, const int* __restrict__ seg_group,
                                                           const int* __restrict__ blk_seg, const SgdGroupsDev G,
                                                           const float* __restrict__ grad_scale, const float* __restrict__ found_inf,
                                                           int write_grad, bf16_t* __restrict__ shadow) {
    if (found_inf && *found_inf != 0.f) return;
    const float inv = grad_scale ? 1.f / *grad_scale : 1.f;
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    int s = find_segment(seg_start, blk_seg[blockIdx.x], i);
    if (i + 4 <= n && i + 4 <= seg_start[s + 1]) {
        const int grp = seg_group[s];
        if (grp < 0) return;
        const float lr = pick_group(G.lr, grp), wd = pick_group(G.wd, grp), momentum = pick_group(G.momentum, grp),
                    dampening = pick_group(G.dampening, grp);
        const int fl = pick_group(G.flags, grp);
        f32x4 pv = *reinterpret_cast<f32x4*>(p + i);
        f32x4 gv = *reinterpret_cast<f32x4*>(g + i) * inv;
        if (fl & 2) gv = -gv;
        const f32x4 gu = gv;
        if (wd != 0.f) gv += pv * wd;
        f32x4 d = gv;
        if (momentum != 0.f) {
            f32x4 bv = (fl & 4) ? gv : *reinterpret_cast<f32x4*>(buf + i) * momentum + gv * (1.f - dampening);
            *reinterpret_cast<f32x4*>(buf + i) = bv;
            d = (fl & 1) ? gv + bv * momentum : bv;
        }
        const f32x4 pn = pv - d * lr;
        *reinterpret_cast<f32x4*>(p + i) = pn;
        if (shadow) *reinterpret_cast<uint2*>(shadow + i) = uint2{pack2bf(pn[0], pn[1]), pack2bf(pn[2], pn[3])};
        if (write_grad) *reinterpret_cast<f32x4*>(g + i) = gu;
    } else {
        for (int64_t j = i; j < n && j < i + 4; ++j) {
            s = find_segment(seg_start, s, j);
            const int grp = seg_group[s];
            if (grp < 0) continue;
            const float lr = pick_group(G.lr, grp), wd = pick_group(G.wd, grp), momentum = pick_group(G.momentum, grp),
                        dampening = pick_group(G.dampening, grp);
            const int fl = pick_group(G.flags, grp);
            float gv = g[j] * inv;
            if (fl & 2) gv = -gv;
            const float gu = gv;
            if (wd != 0.f) gv += p[j] * wd;
            float d = gv;
            if (momentum != 0.f) {
                const float bv = (fl & 4) ? gv : buf[j] * momentum + gv * (1.f - dampening);
                buf[j] = bv;
                d = (fl & 1) ? gv + bv * momentum : bv;
            }
            p[j] -= lr * d;
            if (shadow) shadow[j] = f2bf(p[j]);
            if (write_grad) g[j] = gu;
        }
    }
}

// state[3 grp + {0, 1, 2}] as adam_prep_kernel's state3, one thread per group
__global__ void adam_prep_groups_kernel(float* __restrict__ state, int ngroups, const double* __restrict__ hyper /* [ngroups][3]: lr, beta1, beta2 */,
                                        const float* __restrict__ found_inf) {
    const int grp = threadIdx.x;
    if (blockIdx.x != 0 || grp >= ngroups) return;
    if (found_inf && *found_inf != 0.f) return;
    const double lr = hyper[3 * grp], beta1 = hyper[3 * grp + 1], beta2 = hyper[3 * grp + 2];
    const double step = (double)state[3 * grp] + 1.0;
    state[3 * grp] = (float)step;
    state[3 * grp + 1] = (float)(lr / (1.0 - pow(beta1, step)));
    state[3 * grp + 2] = (float)sqrt(1.0 - pow(beta2, step));
}

__global__ __launch_bounds__(256) void adam_step_seg_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                            int64_t n, const int64_t* __restrict__ seg_start, const int* __restrict__ seg_group,
                                                            const int* __restrict__ blk_seg, const AdamGroupsDev G, const float* __restrict__ state,
                                                            const float* __restrict__ grad_scale, const float* __restrict__ found_inf,
                                                            int write_grad, bf16_t* __restrict__ shadow) {
    if (found_inf && *found_inf != 0.f) return;
    const float inv = grad_scale ? 1.f / *grad_scale : 1.f;
    const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i0 >= n) return;
    int s = find_segment(seg_start, blk_seg[blockIdx.x], i0);
    const bool vec = i0 + 4 <= n && i0 + 4 <= seg_start[s + 1];
    const int cnt = i0 + 4 <= n ? 4 : (int)(n - i0);
    float pv[4], gv[4], mv[4], vv[4], gu[4];
    int grp4[4];
    if (vec) {
        *reinterpret_cast<f32x4*>(pv) = *reinterpret_cast<const f32x4*>(p + i0);
        *reinterpret_cast<f32x4*>(gv) = *reinterpret_cast<const f32x4*>(g + i0);
        *reinterpret_cast<f32x4*>(mv) = *reinterpret_cast<const f32x4*>(m + i0);
        *reinterpret_cast<f32x4*>(vv) = *reinterpret_cast<const f32x4*>(v + i0);
        const int grp = seg_group[s];
        if (grp < 0) return;
#pragma unroll
        for (int e = 0; e < 4; ++e) grp4[e] = grp;
    } else {
        for (int e = 0; e < 4; ++e) {
            grp4[e] = -1;
            pv[e] = gv[e] = mv[e] = vv[e] = 0.f;
            if (e < cnt) {
                s = find_segment(seg_start, s, i0 + e);
                grp4[e] = seg_group[s];
                pv[e] = p[i0 + e]; gv[e] = g[i0 + e]; mv[e] = m[i0 + e]; vv[e] = v[i0 + e];
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int grp = grp4[e] < 0 ? 0 : grp4[e];
        const float omb1 = pick_group(G.omb1, grp), beta2 = pick_group(G.beta2, grp), omb2 = pick_group(G.omb2, grp),
                    eps = pick_group(G.eps, grp), wd = pick_group(G.wd, grp), decay_mul = pick_group(G.decay_mul, grp);
        const int fl = pick_group(G.flags, grp);
        const float step_size = state[3 * grp + 1], bc2s = state[3 * grp + 2];
        float gr = gv[e] * inv;
        if (fl & 2) gr = -gr;
        gu[e] = gr;
        float pe = pv[e];
        if (wd != 0.f) {
            if (fl & 1) pe *= decay_mul; else gr += wd * pe;
        }
        const float me = mv[e] + omb1 * (gr - mv[e]);
        const float ve = vv[e] * beta2 + omb2 * (gr * gr);
        const float denom = sqrtf(ve) / bc2s + eps;
        pv[e] = pe - step_size * (me / denom);
        mv[e] = me; vv[e] = ve;
    }
    if (vec) {
        *reinterpret_cast<f32x4*>(p + i0) = *reinterpret_cast<f32x4*>(pv);
        *reinterpret_cast<f32x4*>(m + i0) = *reinterpret_cast<f32x4*>(mv);
        *reinterpret_cast<f32x4*>(v + i0) = *reinterpret_cast<f32x4*>(vv);
        if (shadow) *reinterpret_cast<uint2*>(shadow + i0) = uint2{pack2bf(pv[0], pv[1]), pack2bf(pv[2], pv[3])};
        if (write_grad) *reinterpret_cast<f32x4*>(g + i0) = *reinterpret_cast<f32x4*>(gu);
    } else {
        for (int e = 0; e < cnt; ++e) {
            if (grp4[e] < 0) continue;
            p[i0 + e] = pv[e]; m[i0 + e] = mv[e]; v[i0 + e] = vv[e];
            if (shadow) shadow[i0 + e] = f2bf(pv[e]);
            if (write_grad) g[i0 + e] = gu[e];
        }
    }
}

// ============================================================================ parameter groups beyond BVC_OPT_MAX_GROUPS: a device table
// Layer-wise learning-rate decay gives 2 (L + 2) groups (28 / 52 / 68 at base / large / huge) - too many for a by-value struct with a
// select chain.  The kernels below walk the SAME segment table and read the hyper-parameters of seg_group[s] from a device table
// with one 32-byte row per group (two 16-byte loads per lane; a row is shared by every lane of a segment and stays in cache):
//   SGD row:  { lr, wd, momentum, dampening | flags, 0, 0, 0 }               flags as in SgdGroupsDev
//   Adam row: { omb1, beta2, omb2, eps | wd, decay_mul, flags, 0 }          flags as in AdamGroupsDev; step scalars in state[3 grp + ..]
// The rows change per step under a schedule.  They reach the device as KERNEL ARGUMENTS of small writer kernels (a chunk of
// BVC_OPT_TABLE_CHUNK groups by value per launch, stored with ordinary vector stores): the runtime copies kernel arguments at launch,
// so there is no host buffer whose lifetime matters, no host synchronisation, and writer and consumer are ordered by the stream
// however far the host runs ahead.  The arithmetic per element is that of sgd_step_seg_kernel / adam_step_seg_kernel, statement for
// statement; a group index outside the table (a malformed segment table) is treated like -1: left untouched.
constexpr int kOptRowFloats = 8;
struct SgdChunkDev {
    float lr[BVC_OPT_TABLE_CHUNK], wd[BVC_OPT_TABLE_CHUNK], momentum[BVC_OPT_TABLE_CHUNK], dampening[BVC_OPT_TABLE_CHUNK];
    int flags[BVC_OPT_TABLE_CHUNK];
};
struct AdamChunkDev {
    double lr[BVC_OPT_TABLE_CHUNK], beta1[BVC_OPT_TABLE_CHUNK], beta2[BVC_OPT_TABLE_CHUNK];     // for the step scalars, in double
    float omb1[BVC_OPT_TABLE_CHUNK], beta2f[BVC_OPT_TABLE_CHUNK], omb2[BVC_OPT_TABLE_CHUNK], eps[BVC_OPT_TABLE_CHUNK], wd[BVC_OPT_TABLE_CHUNK],
        decay_mul[BVC_OPT_TABLE_CHUNK];
    int flags[BVC_OPT_TABLE_CHUNK];
};
static_assert(sizeof(SgdChunkDev) + 64 <= 4096 && sizeof(AdamChunkDev) + 64 <= 4096, "a chunk must fit the kernel-argument segment");

// rows [g0, g0 + count) of the SGD table, one thread per group
__global__ void sgd_table_write_kernel(float* __restrict__ table, int g0, int count, const SgdChunkDev C) {
    const int t = threadIdx.x;
    if (blockIdx.x != 0 || t >= count) return;
    float* row = table + (size_t)(g0 + t) * kOptRowFloats;
    *reinterpret_cast<f32x4*>(row) = f32x4{C.lr[t], C.wd[t], C.momentum[t], C.dampening[t]};
    *reinterpret_cast<f32x4*>(row + 4) = f32x4{__int_as_float(C.flags[t]), 0.f, 0.f, 0.f};
}

// rows [g0, g0 + count) of the Adam table and the groups' step scalars (adam_prep_groups_kernel's formulas, in double; not advanced
// on a step the scaler skips - the rows are written either way, adam_step_table_kernel does not read them on such a step)
__global__ void adam_prep_table_kernel(float* __restrict__ state, float* __restrict__ table, int g0, int count, const AdamChunkDev C,
                                       const float* __restrict__ found_inf) {
    const int t = threadIdx.x;
    if (blockIdx.x != 0 || t >= count) return;
    const int grp = g0 + t;
    float* row = table + (size_t)grp * kOptRowFloats;
    *reinterpret_cast<f32x4*>(row) = f32x4{C.omb1[t], C.beta2f[t], C.omb2[t], C.eps[t]};
    *reinterpret_cast<f32x4*>(row + 4) = f32x4{C.wd[t], C.decay_mul[t], __int_as_float(C.flags[t]), 0.f};
    if (found_inf && *found_inf != 0.f) return;
    const double lr = C.lr[t], beta1 = C.beta1[t], beta2 = C.beta2[t];
    const double step = (double)state[3 * grp] + 1.0;
    state[3 * grp] = (float)step;
    state[3 * grp + 1] = (float)(lr / (1.0 - pow(beta1, step)));
    state[3 * grp + 2] = (float)sqrt(1.0 - pow(beta2, step));
}

// Rounding.  This file is compiled with floating-point contraction on, and which multiply of a sum of two products the compiler fuses
// (buf * momentum + g * (1 - dampening); v * beta2 + (1 - beta2) * g^2) follows the shape of the surrounding code, not the statement:
// the by-value kernels fuse the LEFT product in their vector paths and neither in sgd_step_seg_kernel's element path, and
// adam_step_seg_kernel's m + (1 - beta1) (g - m) is not fused at all (its sum is paired with the denominator's in one packed add).
// Results here have to equal theirs bit for bit, so contraction is off in the two kernels below and every fused multiply-add the
// by-value kernels perform is written out; tests/test_gpu_optim_groups.py compares the two paths bit for bit on the GPU.
__global__ __launch_bounds__(256) void sgd_step_table_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ buf, int64_t n,
                                                             const int64_t* __restrict__ seg_start, const int* __restrict__ seg_group,
                                                             const int* __restrict__ blk_seg, const float* __restrict__ table, int ngroups,
                                                             const float* __restrict__ grad_scale, const float* __restrict__ found_inf,
                                                             int write_grad, bf16_t* __restrict__ shadow) {
#pragma clang fp contract(off)
    if (found_inf && *found_inf != 0.f) return;
    const float inv = grad_scale ? 1.f / *grad_scale : 1.f;
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    int s = find_segment(seg_start, blk_seg[blockIdx.x], i);
    if (i + 4 <= n && i + 4 <= seg_start[s + 1]) {
        const int grp = seg_group[s];
        if (grp < 0 || grp >= ngroups) return;
        const f32x4 r0 = *reinterpret_cast<const f32x4*>(table + (size_t)grp * kOptRowFloats);
        const float lr = r0[0], wd = r0[1], momentum = r0[2], dampening = r0[3];
        const int fl = __float_as_int(table[(size_t)grp * kOptRowFloats + 4]);
        const f32x4 pv = *reinterpret_cast<f32x4*>(p + i);
        f32x4 gv = *reinterpret_cast<f32x4*>(g + i) * inv;
        if (fl & 2) gv = -gv;
        const f32x4 gu = gv;
        if (wd != 0.f) {
#pragma unroll
            for (int e = 0; e < 4; ++e) gv[e] = __builtin_fmaf(pv[e], wd, gv[e]);
        }
        f32x4 d = gv;
        if (momentum != 0.f) {
            f32x4 bv = gv;
            if (!(fl & 4)) {
                const f32x4 bo = *reinterpret_cast<f32x4*>(buf + i), gd = gv * (1.f - dampening);
#pragma unroll
                for (int e = 0; e < 4; ++e) bv[e] = __builtin_fmaf(bo[e], momentum, gd[e]);
            }
            *reinterpret_cast<f32x4*>(buf + i) = bv;
            if (fl & 1) {
#pragma unroll
                for (int e = 0; e < 4; ++e) d[e] = __builtin_fmaf(bv[e], momentum, gv[e]);
            } else {
                d = bv;
            }
        }
        f32x4 pn;
#pragma unroll
        for (int e = 0; e < 4; ++e) pn[e] = __builtin_fmaf(-d[e], lr, pv[e]);
        *reinterpret_cast<f32x4*>(p + i) = pn;
        if (shadow) *reinterpret_cast<uint2*>(shadow + i) = uint2{pack2bf(pn[0], pn[1]), pack2bf(pn[2], pn[3])};
        if (write_grad) *reinterpret_cast<f32x4*>(g + i) = gu;
    } else {
        for (int64_t j = i; j < n && j < i + 4; ++j) {
            s = find_segment(seg_start, s, j);
            const int grp = seg_group[s];
            if (grp < 0 || grp >= ngroups) continue;
            const f32x4 r0 = *reinterpret_cast<const f32x4*>(table + (size_t)grp * kOptRowFloats);
            const float lr = r0[0], wd = r0[1], momentum = r0[2], dampening = r0[3];
            const int fl = __float_as_int(table[(size_t)grp * kOptRowFloats + 4]);
            float gv = g[j] * inv;
            if (fl & 2) gv = -gv;
            const float gu = gv;
            if (wd != 0.f) gv = __builtin_fmaf(p[j], wd, gv);
            float d = gv;
            if (momentum != 0.f) {
                const float bv = (fl & 4) ? gv : buf[j] * momentum + gv * (1.f - dampening);      // both products rounded, as there
                buf[j] = bv;
                d = (fl & 1) ? __builtin_fmaf(bv, momentum, gv) : bv;
            }
            p[j] = __builtin_fmaf(-lr, d, p[j]);
            if (shadow) shadow[j] = f2bf(p[j]);
            if (write_grad) g[j] = gu;
        }
    }
}

__global__ __launch_bounds__(256) void adam_step_table_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                                              int64_t n, const int64_t* __restrict__ seg_start, const int* __restrict__ seg_group,
                                                              const int* __restrict__ blk_seg, const float* __restrict__ table, int ngroups,
                                                              const float* __restrict__ state, const float* __restrict__ grad_scale,
                                                              const float* __restrict__ found_inf, int write_grad, bf16_t* __restrict__ shadow) {
#pragma clang fp contract(off)
    if (found_inf && *found_inf != 0.f) return;
    const float inv = grad_scale ? 1.f / *grad_scale : 1.f;
    const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i0 >= n) return;
    int s = find_segment(seg_start, blk_seg[blockIdx.x], i0);
    const bool vec = i0 + 4 <= n && i0 + 4 <= seg_start[s + 1];
    const int cnt = i0 + 4 <= n ? 4 : (int)(n - i0);
    float pv[4], gv[4], mv[4], vv[4], gu[4];
    int grp4[4];
    if (vec) {
        *reinterpret_cast<f32x4*>(pv) = *reinterpret_cast<const f32x4*>(p + i0);
        *reinterpret_cast<f32x4*>(gv) = *reinterpret_cast<const f32x4*>(g + i0);
        *reinterpret_cast<f32x4*>(mv) = *reinterpret_cast<const f32x4*>(m + i0);
        *reinterpret_cast<f32x4*>(vv) = *reinterpret_cast<const f32x4*>(v + i0);
        const int grp = seg_group[s];
        if (grp < 0 || grp >= ngroups) return;
#pragma unroll
        for (int e = 0; e < 4; ++e) grp4[e] = grp;
    } else {
        for (int e = 0; e < 4; ++e) {
            grp4[e] = -1;
            pv[e] = gv[e] = mv[e] = vv[e] = 0.f;
            if (e < cnt) {
                s = find_segment(seg_start, s, i0 + e);
                grp4[e] = seg_group[s] < ngroups ? seg_group[s] : -1;
                pv[e] = p[i0 + e]; gv[e] = g[i0 + e]; mv[e] = m[i0 + e]; vv[e] = v[i0 + e];
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int grp = grp4[e] < 0 ? 0 : grp4[e];
        const f32x4 r0 = *reinterpret_cast<const f32x4*>(table + (size_t)grp * kOptRowFloats);
        const f32x4 r1 = *reinterpret_cast<const f32x4*>(table + (size_t)grp * kOptRowFloats + 4);
        const float omb1 = r0[0], beta2 = r0[1], omb2 = r0[2], eps = r0[3], wd = r1[0], decay_mul = r1[1];
        const int fl = __float_as_int(r1[2]);
        const float step_size = state[3 * grp + 1], bc2s = state[3 * grp + 2];
        float gr = gv[e] * inv;
        if (fl & 2) gr = -gr;
        gu[e] = gr;
        float pe = pv[e];
        if (wd != 0.f) {
            if (fl & 1) pe *= decay_mul; else gr = __builtin_fmaf(wd, pe, gr);
        }
        const float me = mv[e] + omb1 * (gr - mv[e]);      // product and sum rounded separately, as there
        const float ve = __builtin_fmaf(vv[e], beta2, omb2 * (gr * gr));
        const float denom = sqrtf(ve) / bc2s + eps;
        pv[e] = __builtin_fmaf(-step_size, me / denom, pe);
        mv[e] = me; vv[e] = ve;
    }
    if (vec) {
        *reinterpret_cast<f32x4*>(p + i0) = *reinterpret_cast<f32x4*>(pv);
        *reinterpret_cast<f32x4*>(m + i0) = *reinterpret_cast<f32x4*>(mv);
        *reinterpret_cast<f32x4*>(v + i0) = *reinterpret_cast<f32x4*>(vv);
        if (shadow) *reinterpret_cast<uint2*>(shadow + i0) = uint2{pack2bf(pv[0], pv[1]), pack2bf(pv[2], pv[3])};
        if (write_grad) *reinterpret_cast<f32x4*>(g + i0) = *reinterpret_cast<f32x4*>(gu);
    } else {
        for (int e = 0; e < cnt; ++e) {
            if (grp4[e] < 0) continue;
            p[i0 + e] = pv[e]; m[i0 + e] = mv[e]; v[i0 + e] = vv[e];
            if (shadow) shadow[i0 + e] = f2bf(pv[e]);
            if (write_grad) g[i0 + e] = gu[e];
        }
    }
}

// ============================================================================ zero-padded attention heads (hd -> hdp)
// The JEPA predictor inherits the encoder's head COUNT (vision_transformer.py:447,463: num_heads=encoder.num_heads), so ViT-L
// gives 16 heads of 24 dims - not an MFMA-friendly width.  The heads are run at 32 dims with zero padding: padded copies of
// the bf16 qkv / proj weights are made per use and the padded weight gradients are compacted back (all tiny: Dp = 384).
//   qkv rows:  r' = (which * H + h) * hdp + j  <-  r = (which * H + h) * hd + j   (j < hd; other rows zero)
//   proj cols: c' = h * hdp + j                <-  c = h * hd + j
__global__ void pad_qkv_kernel(const bf16_t* __restrict__ w, const float* __restrict__ b, bf16_t* __restrict__ wp, float* __restrict__ bp,
                               int H, int hd, int hdp, int D) {
    const int rp = blockIdx.x;                       // padded row in [0, 3 H hdp)
    const int j = rp % hdp, wh = rp / hdp;
    const bool live = j < hd;
    const int r = wh * hd + j;
    for (int c = threadIdx.x; c < D; c += blockDim.x) wp[(size_t)rp * D + c] = live ? w[(size_t)r * D + c] : (bf16_t)0;
    if (threadIdx.x == 0) bp[rp] = live ? b[r] : 0.f;
}
__global__ void pad_cols_kernel(const bf16_t* __restrict__ w, bf16_t* __restrict__ wp, int rows, int H, int hd, int hdp) {
    const int r = blockIdx.x;
    for (int cp = threadIdx.x; cp < H * hdp; cp += blockDim.x) {
        const int j = cp % hdp, h = cp / hdp;
        wp[(size_t)r * H * hdp + cp] = j < hd ? w[(size_t)r * H * hd + h * hd + j] : (bf16_t)0;
    }
}
// gradients back to the reference's layout (plain stores: nothing else writes these ranges)
__global__ void unpad_qkv_grad_kernel(const float* __restrict__ gwp, const float* __restrict__ gbp, float* __restrict__ gw,
                                      float* __restrict__ gb, int H, int hd, int hdp, int D) {
    const int r = blockIdx.x;                        // true row in [0, 3 H hd)
    const int j = r % hd, wh = r / hd;
    const int rp = wh * hdp + j;
    for (int c = threadIdx.x; c < D; c += blockDim.x) gw[(size_t)r * D + c] = gwp[(size_t)rp * D + c];
    if (threadIdx.x == 0) gb[r] = gbp[rp];
}
__global__ void unpad_cols_grad_kernel(const float* __restrict__ gwp, float* __restrict__ gw, int rows, int H, int hd, int hdp) {
    const int r = blockIdx.x;
    for (int c = threadIdx.x; c < H * hd; c += blockDim.x) {
        const int j = c % hd, h = c / hd;
        gw[(size_t)r * H * hd + c] = gwp[(size_t)r * H * hdp + h * hdp + j];
    }
}

// GradScaler's inf check as ONE read-only pass: *found_inf = 1 if any element of x is Inf or NaN (never cleared here).
// torch does it with _amp_foreach_non_finite_check_and_unscale_(grads, found_inf, inv_scale = 1): a read AND a write of every
// gradient, 6 multi-tensor launches for VideoMAE-base (0.24 ms per step at 3.1 TB/s); this reads 377 MB once.
__global__ void nonfinite_check_kernel(const float* __restrict__ x, size_t n, float* __restrict__ found_inf) {
    const size_t stride = (size_t)gridDim.x * blockDim.x * 4;
    bool bad = false;
    size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    for (; i + 4 <= n; i += stride) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(x + i);
        // (v - v) is 0 for finite values and NaN for Inf / NaN
        const float t = (v[0] - v[0]) + (v[1] - v[1]) + (v[2] - v[2]) + (v[3] - v[3]);
        bad |= (t != 0.f);
    }
    for (; i < n; ++i) bad |= ((x[i] - x[i]) != 0.f);      // tail of the last vector
    if (__any(bad) && (threadIdx.x & 63) == 0) *found_inf = 1.0f;
}

// ---------------------------------------------------------------------------------------------- gradient norms (clipping)
// Squared norm of the owned segments of a flat f32 range in ONE read, with GradScaler's inf check riding on the same read.
// The range is cut on the host (grad_norm_items_host below) into items of at most kNormItemCap elements that never cross a segment
// boundary; one workgroup takes one item.  Inside an item the first 16-byte boundary splits off up to 3 head elements, whole 16-byte
// vectors follow and up to 3 tail elements remain; thread t takes vectors t, t + 256, ... (at most kNormChain of them) into four f32
// accumulators by fused multiply-add - the longest serial f32 chain any element's square passes through is kNormChain terms.
// Everything after that (the four lanes, the head / tail squares, the wave, the four waves, the items of a segment, the segments)
// is added in f64 in a fixed order: no atomics, the same bits on every run, and no f32 rounding besides the final cast.
constexpr int kNormItemCap = BVC_GRAD_NORM_ITEM_CAP;
constexpr int kNormChain = kNormItemCap / (256 * 4);
static_assert(kNormChain * 256 * 4 == kNormItemCap, "an item is a whole number of 16-byte vectors per thread");

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// 256 threads -> the sum in thread 0 (waves added as (w0 + w1) + (w2 + w3))
__device__ __forceinline__ double block_sum_f64(double v, double* lds4) {
    v = wave_sum_f64(v);
    if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = v;
    __syncthreads();
    return (lds4[0] + lds4[1]) + (lds4[2] + lds4[3]);
}

__global__ __launch_bounds__(256) void grad_sqnorm_items_kernel(const float* __restrict__ x, const bvc_norm_item* __restrict__ items,
                                                                double* __restrict__ item_partial, float* __restrict__ found_inf) {
    __shared__ double lds4[4];
    const bvc_norm_item it = items[blockIdx.x];
    const float* __restrict__ p = x + it.start;
    const int len = it.length, tid = threadIdx.x;
    int head = (int)((4 - (((uintptr_t)p >> 2) & 3)) & 3);       // elements before the first 16-byte boundary
    head = head < len ? head : len;
    const int nvec = (len - head) >> 2;
    const int tail0 = head + 4 * nvec;
    const f32x4* __restrict__ pv = reinterpret_cast<const f32x4*>(p + head);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    float t = 0.f;                                               // (v - v) is 0 for finite values and NaN for Inf / NaN
    if (nvec == kNormChain * 256) {                              // a full item: every load of the thread is issued before the first use
        f32x4 v[kNormChain];
#pragma unroll
        for (int k = 0; k < kNormChain; ++k) v[k] = pv[tid + 256 * k];
#pragma unroll
        for (int k = 0; k < kNormChain; ++k) {
            acc = __builtin_elementwise_fma(v[k], v[k], acc);
            t += (v[k][0] - v[k][0]) + (v[k][1] - v[k][1]) + (v[k][2] - v[k][2]) + (v[k][3] - v[k][3]);
        }
    } else {
#pragma unroll 4
        for (int i = tid; i < nvec; i += 256) {
            const f32x4 v = pv[i];
            acc = __builtin_elementwise_fma(v, v, acc);
            t += (v[0] - v[0]) + (v[1] - v[1]) + (v[2] - v[2]) + (v[3] - v[3]);
        }
    }
    double ht = 0.0;                                             // head / tail elements: at most one of each per thread
    if (tid < head) { const float h = p[tid]; ht = (double)h * (double)h; t += h - h; }
    if (tail0 + tid < len) { const float e = p[tail0 + tid]; ht += (double)e * (double)e; t += e - e; }
    const double mine = (((double)acc[0] + (double)acc[1]) + ((double)acc[2] + (double)acc[3])) + ht;
    const double sum = block_sum_f64(mine, lds4);
    if (tid == 0) item_partial[blockIdx.x] = sum;
    if (found_inf != nullptr && __any(t != 0.f) && (tid & 63) == 0) *found_inf = 1.0f;
}

// item partials -> seg_sq[s] (block s < nseg: the items seg_first_item[s] .. seg_first_item[s + 1] of segment s, nothing for an unowned
// one) and total_sq (the last block: every item), f64 in a fixed order, cast to f32 at the end; as_norm: the square roots instead
__global__ __launch_bounds__(256) void grad_sqnorm_reduce_kernel(const double* __restrict__ item_partial, const int64_t* __restrict__ seg_first_item,
                                                                 int nseg, int64_t nitems, float* __restrict__ seg_sq,
                                                                 float* __restrict__ total_sq, int as_norm) {
    __shared__ double lds4[4];
    const bool total = seg_sq == nullptr || (int)blockIdx.x == nseg;
    const int64_t lo = total ? 0 : seg_first_item[blockIdx.x], hi = total ? nitems : seg_first_item[blockIdx.x + 1];
    double a = 0.0;
#pragma unroll 8
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) a += item_partial[i];      // (loads run ahead, the additions keep their order)
    const double sum = block_sum_f64(a, lds4);
    if (threadIdx.x == 0) {
        const float r = as_norm ? (float)sqrt(sum) : (float)sum;
        if (total) *total_sq = r; else seg_sq[blockIdx.x] = r;
    }
}

// out = {total_norm, clip_coef, eff_scale}: total_norm = sqrt(sum sq) / scale, clip_coef = min(1, max_norm / (total_norm + 1e-6)) with
// torch's clamp (a NaN stays a NaN), eff_scale = scale / clip_coef - what a step kernel divides the gradients by to unscale AND clip.
// The few sq entries are added in f64, the rest is f32 arithmetic as torch.nn.utils.clip_grad_norm_ does it.
__global__ void clip_finalize_kernel(const float* __restrict__ sq, int nranges, float max_norm, const float* __restrict__ grad_scale,
                                     float* __restrict__ out) {
    if (threadIdx.x != 0) return;
    double s = 0.0;
    for (int i = 0; i < nranges; ++i) s += (double)sq[i];
    const float scale = grad_scale ? *grad_scale : 1.f;
    const float norm = sqrtf((float)s) / scale;
    const float c = max_norm / (norm + 1e-6f);
    const float coef = c > 1.f ? 1.f : c;
    out[0] = norm; out[1] = coef; out[2] = scale / coef;
}

// x *= *coef; nothing is written when *coef == 1 (an inactive clip costs the read of one scalar)
__global__ void scale_by_dev_kernel(float* __restrict__ x, size_t n, const float* __restrict__ coef) {
    const float c = *coef;
    if (c == 1.0f) return;
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, nthreads = (size_t)gridDim.x * blockDim.x;
    size_t head = (4 - (((uintptr_t)x >> 2) & 3)) & 3;
    head = head < n ? head : n;
    const size_t nvec = (n - head) / 4;
    f32x4* __restrict__ xv = reinterpret_cast<f32x4*>(x + head);
    for (size_t i = tid; i < nvec; i += nthreads) xv[i] = xv[i] * c;
    if (tid < head) x[tid] *= c;
    if (head + 4 * nvec + tid < n) x[head + 4 * nvec + tid] *= c;
}

// ============================================================================ launchers
static inline unsigned blocks_for(size_t items, int per = 256) { return (unsigned)((items + per - 1) / per); }

// two rows per wave (32 lanes each) when a row is at most 512 wide and a whole number of float4 per lane: 384 = 3 per lane
static inline bool ln_half_wave_rows(int D) { return D <= 512 && D % 128 == 0; }
// grid of a grid-stride row kernel: at most `cap` workgroups, and every workgroup the same number of row groups (2560 groups on
// 2048 workgroups would give a quarter of them twice the work of the rest)
static inline int balanced_grid(int ngroups, int cap) {
    if (ngroups <= cap) return ngroups > 0 ? ngroups : 1;
    // a few groups per workgroup: keep every CU's resident slots full rather than even (encoder LayerNorm backward at 256 clips,
    // 2560 groups: 2048 workgroups 99-105 us, 1280 even ones 118 us - five per CU do not cover the HBM latency)
    if (ngroups < 4 * cap) return cap;
    const int rounds = (ngroups + cap - 1) / cap;
    return (ngroups + rounds - 1) / rounds;
}
constexpr int kLnFwdMaxBlocks = 4096;      // 16 per CU (the kernel holds its row in registers: 8 resident workgroups per CU and a second round)

int launch_ln_fwd(const float* x, RowMap rm, const float* gamma, const float* beta, bf16_t* y, float* mean, float* rstd,
                  int M, int D, float eps, hipStream_t s, float* y32) {
    BVC_REQUIRE(D % 4 == 0 && D <= kWideChunks * 256, "ln_fwd: D=%d unsupported", D);
    if (D > kMaxChunks * 256)
        hipLaunchKernelGGL((ln_fwd_kernel<64, kWideChunks>), dim3(balanced_grid((M + 3) / 4, kLnFwdMaxBlocks)), dim3(256), 0, s, x, rm, gamma, beta, y, y32, mean, rstd, M, D, eps);
    else if (ln_half_wave_rows(D))
        hipLaunchKernelGGL((ln_fwd_kernel<32, kMaxChunks>), dim3(balanced_grid((M + 7) / 8, kLnFwdMaxBlocks)), dim3(256), 0, s, x, rm, gamma, beta, y, y32, mean, rstd, M, D, eps);
    else
        hipLaunchKernelGGL((ln_fwd_kernel<64, kMaxChunks>), dim3(balanced_grid((M + 3) / 4, kLnFwdMaxBlocks)), dim3(256), 0, s, x, rm, gamma, beta, y, y32, mean, rstd, M, D, eps);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

// 64 rows per workgroup for M >= 65536 was measured slower (B=64 decoder: 1276 vs 1157 us per step for the LN backward, which
// outweighs the 70 us saved in the partial reduction), so the third tier stays unused.
static inline int ln_bwd_rows_per_block(int M) { return M >= 16384 ? 16 : 4; }
constexpr int kLnBwdMaxBlocks = 2048;      // 8 per CU: every CU keeps its ~7 resident workgroups (register-limited) busy to the end

size_t ln_bwd_workspace_floats(int M, int D) {
    const int rpb = ln_bwd_rows_per_block(M);
    return (size_t)((M + rpb - 1) / rpb) * 2 * D;
}

// enough for every row count m <= Mmax (the rows-per-workgroup choice is not monotonic in m)
size_t ln_bwd_workspace_floats_upto(int Mmax, int D) {
    size_t best = ln_bwd_workspace_floats(Mmax, D);
    for (int edge : {16383, 65535}) {
        const size_t w = ln_bwd_workspace_floats(Mmax < edge ? Mmax : edge, D);
        best = w > best ? w : best;
    }
    return best;
}

int launch_ln_bwd(const bf16_t* dy, const float* x, RowMap rm, const float* mean, const float* rstd, const float* gamma,
                  float* dres, int accumulate, bf16_t* dres_bf, float* dgamma, float* dbeta, float* part, int M, int D, hipStream_t s,
                  const Gate* gate, bool compact_x) {
    BVC_REQUIRE(D % 4 == 0 && D <= kWideChunks * 256, "ln_bwd: D=%d unsupported", D);
    BVC_REQUIRE(!(gate && compact_x), "ln_bwd: the gated form has no compact operands");
    const int compact = compact_x ? 1 : 0;
    BVC_REQUIRE(part != nullptr, "ln_bwd: workspace missing");
    // rows per workgroup: enough workgroups to keep >= 16 waves per CU streaming (the kernel is HBM-bound and
    // each wave walks its rows serially), few enough that the per-column atomics stay negligible
    const int rpb = ln_bwd_rows_per_block(M);
    const int rpg = rpb == 4 && ln_half_wave_rows(D) ? 8 : rpb;          // rows per row group of the instantiation launched below
    const int nblk = balanced_grid((M + rpg - 1) / rpg, kLnBwdMaxBlocks);
    const bool half = ln_half_wave_rows(D);
    const size_t lds = (size_t)(half ? 16 : 8) * D * sizeof(float);
#define BVC_LN_BWD(RPB_, LPR_, NC_) hipLaunchKernelGGL((ln_bwd_kernel<RPB_, LPR_, NC_>), dim3(nblk), dim3(256), lds, s, dy, x, rm, mean, rstd, gamma, dres, accumulate, dres_bf, part, M, D, compact)
#define BVC_LN_BWD_G(RPB_, LPR_, NC_) hipLaunchKernelGGL((ln_bwd_gate_kernel<RPB_, LPR_, NC_>), dim3(nblk), dim3(256), lds, s, dy, x, rm, mean, rstd, gamma, dres, accumulate, dres_bf, part, M, D, *gate)
    if (gate) {      // the same grid and instantiation choice, the bf16 copy gated
        BVC_REQUIRE(dres_bf && gate->rows >= 1 && (double)M * D < 4398046511104.0, "ln_bwd: a gate needs the bf16 copy and rows per sample >= 1");
        if (D > kMaxChunks * 256) { if (rpb == 16) BVC_LN_BWD_G(16, 64, kWideChunks); else BVC_LN_BWD_G(4, 64, kWideChunks); }
        else if (rpb == 16) { if (half) BVC_LN_BWD_G(16, 32, kMaxChunks); else BVC_LN_BWD_G(16, 64, kMaxChunks); }
        else { if (half) BVC_LN_BWD_G(8, 32, kMaxChunks); else BVC_LN_BWD_G(4, 64, kMaxChunks); }
    }
    else if (D > kMaxChunks * 256) { if (rpb == 16) BVC_LN_BWD(16, 64, kWideChunks); else BVC_LN_BWD(4, 64, kWideChunks); }
    else if (rpb == 16) { if (half) BVC_LN_BWD(16, 32, kMaxChunks); else BVC_LN_BWD(16, 64, kMaxChunks); }
    else { if (half) BVC_LN_BWD(8, 32, kMaxChunks); else BVC_LN_BWD(4, 64, kMaxChunks); }
#undef BVC_LN_BWD
#undef BVC_LN_BWD_G
    BVC_CHECK_HIP(hipGetLastError());
    return launch_ln_param_reduce(part, nblk, D, dgamma, dbeta, s);
}

int launch_ln_param_reduce(const float* part, int nblk, int D, float* dgamma, float* dbeta, hipStream_t s) {
    BVC_REQUIRE(part && dgamma && dbeta && nblk > 0 && D > 0, "ln_param_reduce: bad argument");
    if (options().deterministic) {     // all partial rows in index order, no atomics
        float* mid = nullptr;
        if (const size_t f = det_rows_mid_floats(nblk, 2 * D)) {
            mid = det_scratch(f, s);
            if (!mid) return BVC_ERR_HIP;
        }
        return launch_det_rows_reduce(part, nblk, 2 * D, D, dgamma, dbeta, mid, s);
    }
    if (nblk > kLnReduceWide)
        hipLaunchKernelGGL(ln_param_reduce_kernel<64>, dim3((2 * D + 255) / 256, (nblk + 63) / 64), dim3(256), 0, s, part, nblk, D, dgamma, dbeta);
    else
        hipLaunchKernelGGL(ln_param_reduce_kernel<16>, dim3((2 * D + 255) / 256, (nblk + 15) / 16), dim3(256), 0, s, part, nblk, D, dgamma, dbeta);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

int launch_colsum_bf16_scaled(const bf16_t* X, int M, int N, int ld, float alpha, const float* alpha_dev, float* out, hipStream_t s) {
    BVC_REQUIRE(N % 8 == 0 && ld % 8 == 0, "colsum_bf16: N and ld must be multiples of 8");
    const int RB = M >= 16384 ? 256 : 64;
    if (options().deterministic) {     // partial rows into the workspace, then a fixed-order column reduce
        const int nrb = (M + RB - 1) / RB;
        if (nrb <= 0) return BVC_OK;
        float* part = det_scratch((size_t)nrb * N + det_rows_mid_floats(nrb, N), s);
        if (!part) return BVC_ERR_HIP;
        hipLaunchKernelGGL(colsum_bf16_det_kernel, dim3((N + 511) / 512, nrb), dim3(256), 0, s, X, M, N, ld, alpha, alpha_dev, part, RB);
        BVC_CHECK_HIP(hipGetLastError());
        return launch_det_rows_reduce(part, nrb, N, N, out, out, part + (size_t)nrb * N, s);
    }
    hipLaunchKernelGGL(colsum_bf16_kernel, dim3((N + 511) / 512, (M + RB - 1) / RB), dim3(256), 0, s, X, M, N, ld, alpha, alpha_dev, out, RB);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

int launch_colsum_bf16(const bf16_t* X, int M, int N, int ld, float alpha, float* out, hipStream_t s) {
    return launch_colsum_bf16_scaled(X, M, N, ld, alpha, nullptr, out, s);
}

int launch_colsum_f32(const float* X, RowMap rm, int M, int D, float* out, hipStream_t s) {
    BVC_REQUIRE(D % 4 == 0, "colsum_f32: D must be a multiple of 4");
    const int RB = 256;
    if (options().deterministic) {
        const int nrb = (M + RB - 1) / RB;
        if (nrb <= 0) return BVC_OK;
        float* part = det_scratch((size_t)nrb * D + det_rows_mid_floats(nrb, D), s);
        if (!part) return BVC_ERR_HIP;
        hipLaunchKernelGGL(colsum_f32_det_kernel, dim3((D + 255) / 256, nrb), dim3(256), 0, s, X, rm, M, D, part, RB);
        BVC_CHECK_HIP(hipGetLastError());
        return launch_det_rows_reduce(part, nrb, D, D, out, out, part + (size_t)nrb * D, s);
    }
    hipLaunchKernelGGL(colsum_f32_kernel, dim3((D + 255) / 256, (M + RB - 1) / RB), dim3(256), 0, s, X, rm, M, D, out, RB);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

int launch_token_mean(const float* x, int B, int N, int D, float* out, hipStream_t s) {
    BVC_REQUIRE(D % 4 == 0, "token_mean: D must be a multiple of 4");
    hipLaunchKernelGGL(token_mean_kernel, dim3((D + 63) / 64, B), dim3(256), 0, s, x, N, D, out);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

int launch_token_mean_bwd(const float* dmean, int B, int N, int D, float* dx, hipStream_t s) {
    BVC_REQUIRE(D % 4 == 0, "token_mean_bwd: D must be a multiple of 4");
    const size_t total4 = (size_t)B * N * D / 4;
    hipLaunchKernelGGL(token_mean_bwd_kernel, dim3(blocks_for(total4)), dim3(256), 0, s, dmean, dx, N, D, total4);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

int launch_dropout_mask(const Gate& gate, size_t n, uint8_t* out, hipStream_t s) {
    BVC_REQUIRE(out && n > 0 && (double)n < 4398046511104.0, "dropout_mask: bad argument");
    hipLaunchKernelGGL(dropout_mask_kernel, dim3(blocks_for((n + 3) / 4)), dim3(256), 0, s, gate, n, out);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

void dropout_mask_host(const Gate& gate, size_t n, uint8_t* out) {
    for (size_t q = 0; q * 4 < n; ++q) {
        uint32_t r[4];
        gate_draws(gate, q, r);
        for (int e = 0; e < 4 && q * 4 + e < n; ++e) out[q * 4 + e] = r[e] >= gate.thr ? 1 : 0;
    }
}

int launch_fcnorm_bwd_bcast(const float* dy, const float* p, const float* mean, const float* rstd, const float* gamma, float* dres,
                            bf16_t* dres_bf, float* dgamma, float* dbeta, int B, int N, int D, hipStream_t s, const Gate* gate) {
    BVC_REQUIRE(dy && p && mean && rstd && gamma && dgamma && dbeta && B >= 1 && N >= 1, "fcnorm_bwd_bcast: bad argument");
    BVC_REQUIRE(D % 4 == 0 && D <= 1536, "fcnorm_bwd_bcast: D=%d unsupported (a multiple of 4 up to 1536)", D);
    BVC_REQUIRE((dres == nullptr) == (dres_bf == nullptr), "fcnorm_bwd_bcast: dres and its bf16 copy go together");
    const int pcols = (D + 255) / 256;
    if (!dres) {
        hipLaunchKernelGGL(fcnorm_bwd_bcast_kernel, dim3(pcols, 1), dim3(256), 0, s, dy, p, mean, rstd, gamma, dres, dres_bf, dgamma, dbeta,
                           B, N, D, 0);
    } else {
        const int chunks = (N + kFcRows - 1) / kFcRows;
        if (gate) {
            BVC_REQUIRE(gate->rows == N, "fcnorm_bwd_bcast: the gate's rows per sample (%d) must be the token count %d", gate->rows, N);
            hipLaunchKernelGGL(fcnorm_bwd_bcast_gate_kernel, dim3(std::max(chunks, pcols), B + 1), dim3(256), 0, s, dy, p, mean, rstd, gamma, dres,
                               dres_bf, dgamma, dbeta, B, N, D, B, *gate);
        } else {
            hipLaunchKernelGGL(fcnorm_bwd_bcast_kernel, dim3(std::max(chunks, pcols), B + 1), dim3(256), 0, s, dy, p, mean, rstd, gamma, dres,
                               dres_bf, dgamma, dbeta, B, N, D, B);
        }
    }
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

int launch_cast_bf16(const float* in, bf16_t* out, size_t n, hipStream_t s) {
    hipLaunchKernelGGL(cast_f32_bf16_kernel, dim3(blocks_for((n + 7) / 8)), dim3(256), 0, s, in, out, n);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

int launch_gather_rows_bf16(const float* in, RowMap rm, bf16_t* out, int M, int D, hipStream_t s) {
    hipLaunchKernelGGL(gather_rows_bf16_kernel, dim3(blocks_for((size_t)M * (D / 4))), dim3(256), 0, s, in, rm, out, M, D);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

int launch_mask_index(const uint8_t* mask, int B, int L, int nvis, int nmask, int* vis_idx, int* msk_idx, int* status, hipStream_t s) {
    hipLaunchKernelGGL(mask_index_kernel, dim3(B), dim3(64), 0, s, mask, L, nvis, nmask, vis_idx, msk_idx, status);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

int launch_dual_mask_index(const uint8_t* mask, const uint8_t* decode, int B, int L, int nvis, int ndec, int* vis_idx, int* dec_idx,
                           int* status, hipStream_t s) {
    hipLaunchKernelGGL(dual_mask_index_kernel, dim3(B), dim3(64), 0, s, mask, decode, L, nvis, ndec, vis_idx, dec_idx, status);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

int launch_gather_patches(PixelSrc clip, const int* vis_idx, bf16_t* A, int B, int nvis, PatchGeom pg, hipStream_t s) {
    BVC_REQUIRE(pg.ps % 8 == 0 && pg.W % 4 == 0, "gather_patches: patch size must be a multiple of 8");
    const size_t items = (size_t)B * nvis * (pg.C * pg.ts * pg.ps * pg.ps / 8);
    hipLaunchKernelGGL(gather_patches_kernel, dim3(blocks_for(items)), dim3(256), 0, s, clip, vis_idx, A, B, nvis, pg);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

int launch_gather_patches_mix(PixelSrc clip, const int* idx, bf16_t* A, int B, int n, PatchGeom pg, const ClipMix* mix, hipStream_t s,
                              int* status) {
    BVC_REQUIRE(clip.ptr && idx && A && mix, "gather_patches_mix: null argument");
    BVC_REQUIRE(B >= 1 && n >= 1, "gather_patches_mix: B=%d clips of n=%d tokens", B, n);
    BVC_REQUIRE(pg.ps % 8 == 0 && pg.W % 4 == 0, "gather_patches_mix: patch size must be a multiple of 8");
    const size_t items = (size_t)B * n * (pg.C * pg.ts * pg.ps * pg.ps / 8);
    if ((pg.C * pg.ts * pg.ps * pg.ps / 8) % 64 == 0)
        hipLaunchKernelGGL(gather_patches_mix_kernel<true>, dim3(blocks_for(items)), dim3(256), 0, s, clip, idx, A, B, n, pg, mix, status);
    else
        hipLaunchKernelGGL(gather_patches_mix_kernel<false>, dim3(blocks_for(items)), dim3(256), 0, s, clip, idx, A, B, n, pg, mix, status);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

int launch_gather_patches_aug(PixelSrc clip, const int* idx, bf16_t* A, int B, int n, PatchGeom pg, const ClipMix* mix, EraseTab er,
                              hipStream_t s, int* status) {
    BVC_REQUIRE(clip.ptr && idx && A && er.tab, "gather_patches_aug: null argument");
    BVC_REQUIRE(B >= 1 && n >= 1, "gather_patches_aug: B=%d clips of n=%d tokens", B, n);
    BVC_REQUIRE(er.boxes >= 1 && er.boxes <= BVC_ERASE_MAX_BOXES, "gather_patches_aug: %d boxes per clip outside [1, %d]", er.boxes, BVC_ERASE_MAX_BOXES);
    BVC_REQUIRE(pg.ps % 8 == 0 && pg.W % 4 == 0, "gather_patches_aug: patch size must be a multiple of 8");
    BVC_REQUIRE(pg.C <= 4, "gather_patches_aug: %d channels (the colour counter holds at most 4)", pg.C);
    const size_t items = (size_t)B * n * (pg.C * pg.ts * pg.ps * pg.ps / 8);
    if ((pg.C * pg.ts * pg.ps * pg.ps / 8) % 64 == 0)
        hipLaunchKernelGGL(gather_patches_aug_kernel<true>, dim3(blocks_for(items)), dim3(256), 0, s, clip, idx, A, B, n, pg, mix, er, status);
    else
        hipLaunchKernelGGL(gather_patches_aug_kernel<false>, dim3(blocks_for(items)), dim3(256), 0, s, clip, idx, A, B, n, pg, mix, er, status);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

int launch_erase_noise(EraseTab er, int kind, int B, int T, int C, int H, int W, float* out, hipStream_t s) {
    BVC_REQUIRE(out && (kind == 0 || kind == 1), "erase_noise: kind %d unknown", kind);
    BVC_REQUIRE(B >= 1 && T >= 1 && C >= 1 && H >= 1 && W >= 1 && W % 4 == 0, "erase_noise: bad geometry (W must be a multiple of 4)");
    const size_t quads = kind == 0 ? (size_t)B * T * C * H * (W / 4) : (size_t)B * T * 4;
    hipLaunchKernelGGL(erase_noise_kernel, dim3(blocks_for(quads)), dim3(256), 0, s, er, kind, quads, out);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

int launch_poison_on_status(float* x, size_t count, const int* status, hipStream_t s) {
    hipLaunchKernelGGL(poison_on_status_kernel, dim3(blocks_for(count)), dim3(256), 0, s, x, count, status);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

int launch_labels(PixelSrc clip, const int* dec_idx, float* labels, int B, int ndec, PatchGeom pg, int norm_pix, hipStream_t s) {
    BVC_REQUIRE(pg.ps % 4 == 0, "labels: patch size must be a multiple of 4");
    const int E = pg.ts * pg.ps * pg.ps;
    const size_t lds = (size_t)(pg.C * E + 2 * pg.C) * 4;
    // one wave per token when a token is at most 8 x 64 chunks of 16 bytes (C E <= 2048 values: every configuration of the reference)
    const int nchunk = pg.C * (E >> 2), ntok = B * ndec;
    if (pg.C == 3 && (E == 512 || E == 256)) {      // the reference's tubes: constant channel count, statistics from registers
        const int nblk = (ntok + 3) / 4;
        if (E == 512) hipLaunchKernelGGL(labels_wave3_kernel<2>, dim3(nblk), dim3(256), (size_t)4 * 3 * E * 4, s, clip, dec_idx, labels, ntok, ndec, pg, norm_pix);
        else hipLaunchKernelGGL(labels_wave3_kernel<1>, dim3(nblk), dim3(256), (size_t)4 * 3 * E * 4, s, clip, dec_idx, labels, ntok, ndec, pg, norm_pix);
        BVC_CHECK_HIP(hipGetLastError());
        return BVC_OK;
    }
    if (nchunk <= 512 && lds <= 16384) {
        const int per_wave = (pg.C * E + 2 * pg.C + 3) & ~3;
        const int nblk = (ntok + 3) / 4;
        if (nchunk <= 384)
            hipLaunchKernelGGL(labels_wave_kernel<6>, dim3(nblk), dim3(256), (size_t)per_wave * 16, s, clip, dec_idx, labels, ntok, ndec, pg, norm_pix);
        else
            hipLaunchKernelGGL(labels_wave_kernel<8>, dim3(nblk), dim3(256), (size_t)per_wave * 16, s, clip, dec_idx, labels, ntok, ndec, pg, norm_pix);
        BVC_CHECK_HIP(hipGetLastError());
        return BVC_OK;
    }
    hipLaunchKernelGGL(labels_kernel, dim3(B * ndec), dim3(256), lds, s, clip, dec_idx, labels, ndec, pg, norm_pix);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

int launch_fill_masked(float* xfull, const float* mask_token, const float* pos, const int* dec_idx, int B, int Ld, int nvis,
                       int ndec, int D, hipStream_t s) {
    hipLaunchKernelGGL(fill_masked_kernel, dim3(blocks_for((size_t)B * ndec * (D / 4))), dim3(256), 0, s, xfull, mask_token, pos, dec_idx, B, Ld, nvis, ndec, D);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

int launch_dec_slot(const int* dec_idx, int* dec_slot, int B, int L, int ndec, hipStream_t s) {
    BVC_CHECK_HIP(hipMemsetAsync(dec_slot, 0xff, (size_t)B * L * sizeof(int), s));
    hipLaunchKernelGGL(dec_slot_kernel, dim3(blocks_for((size_t)B * ndec)), dim3(256), 0, s, dec_idx, dec_slot, B, L, ndec);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

int launch_first_assemble(const bf16_t* qkv_vis, const bf16_t* t2, const float* t0, const int* dec_idx, bf16_t* qkv, float* xfull, int B,
                          int nvis, int ndec, int W, int D, hipStream_t s) {
    BVC_REQUIRE(W % 8 == 0 && D % 4 == 0, "first_assemble: W must be a multiple of 8, D of 4");
    const size_t items = (size_t)B * (nvis + ndec) * (W / 8) + (size_t)B * ndec * (D / 4);
    hipLaunchKernelGGL(first_assemble_kernel, dim3(blocks_for(items)), dim3(256), 0, s, qkv_vis, t2, t0, dec_idx, qkv, xfull, B, nvis, ndec, W, D);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

int launch_first_reduce(const bf16_t* dqkv, const int* dec_slot, int B, int L, int Ld, int nvis, int W, float* S, bf16_t* hi, bf16_t* lo,
                        hipStream_t s) {
    BVC_REQUIRE(B >= 1 && L >= 1 && W >= 8 && W % 8 == 0 && nvis >= 0 && Ld > nvis, "first_reduce: bad shape (B %d, L %d, Ld %d, nvis %d, W %d)", B, L, Ld, nvis, W);
    BVC_REQUIRE((hi == nullptr) == (lo == nullptr) && (S || hi), "first_reduce: no output, or half of the bf16 pair");
    hipLaunchKernelGGL(first_reduce_kernel, dim3(L, (W + 511) / 512), dim3(64), 0, s, dqkv, dec_slot, B, L, Ld, nvis, W, S, hi, lo);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

int launch_gather_rows_copy_bf16(const bf16_t* in, RowMap rm, bf16_t* out, int M, int W, hipStream_t s) {
    BVC_REQUIRE(W % 8 == 0, "gather_rows_copy_bf16: W must be a multiple of 8");
    hipLaunchKernelGGL(gather_rows_copy_bf16_kernel, dim3(blocks_for((size_t)M * (W / 8))), dim3(256), 0, s, in, rm, out, M, W);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

int launch_pair_split(const float* a, const float* b, bf16_t* hi, bf16_t* lo, size_t n, hipStream_t s) {
    BVC_REQUIRE(n % 4 == 0 && n > 0, "pair_split: the element count must be a positive multiple of 4");
    hipLaunchKernelGGL(pair_split_kernel, dim3(blocks_for(n / 4)), dim3(256), 0, s, a, b, hi, lo, n / 4);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

int launch_target_select(const float* h, const int* idx, float* out, int nsets, int B, int Np, int L, int D, float eps, hipStream_t s) {
    BVC_REQUIRE(D % 4 == 0 && D <= kWideChunks * 256, "target_select: D=%d unsupported", D);
    const int rows = nsets * B * Np;
    if (D > kMaxChunks * 256)
        hipLaunchKernelGGL(target_select_kernel<kWideChunks>, dim3((rows + 3) / 4), dim3(256), 0, s, h, idx, out, rows, B, Np, L, D, eps);
    else
        hipLaunchKernelGGL(target_select_kernel<kMaxChunks>, dim3((rows + 3) / 4), dim3(256), 0, s, h, idx, out, rows, B, Np, L, D, eps);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

int launch_pred_assemble(const float* xe, const float* mask_token, const float* pos, const int* idx_pred, float* X, int nsets, int B,
                         int Nc, int Np, int D, hipStream_t s) {
    const size_t items = (size_t)nsets * B * (Nc + Np) * (D / 4);
    hipLaunchKernelGGL(pred_assemble_kernel, dim3(blocks_for(items)), dim3(256), 0, s, xe, mask_token, pos, idx_pred, X, nsets * B, B, Nc, Np, D);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

int launch_pred_ctx_grad(const float* dX, bf16_t* dxe, int nsets, int B, int Nc, int Np, int D, hipStream_t s) {
    hipLaunchKernelGGL(pred_ctx_grad_kernel, dim3(blocks_for((size_t)B * Nc * (D / 4))), dim3(256), 0, s, dX, dxe, nsets, B, Nc, Np, D);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

int smooth_l1_blocks(size_t n) { return (int)std::min<size_t>(1024, (n + 1023) / 1024); }

int launch_smooth_l1_fwd(const float* z, const float* h, size_t n, float* partial, float* loss, hipStream_t s) {
    BVC_REQUIRE(n > 0, "smooth_l1: empty input");
    const int nb = smooth_l1_blocks(n);
    hipLaunchKernelGGL(smooth_l1_fwd_kernel, dim3(nb), dim3(256), 0, s, z, h, n, partial);
    BVC_CHECK_HIP(hipGetLastError());
    return launch_loss_finalize(partial, nb, (double)n, nullptr, loss, s);
}

int launch_smooth_l1_bwd(const float* z, const float* h, const float* gout, size_t n, float* dz, hipStream_t s) {
    hipLaunchKernelGGL(smooth_l1_bwd_kernel, dim3(blocks_for((n + 3) / 4)), dim3(256), 0, s, z, h, gout, n, dz);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

int launch_ema(float* k, const float* q, size_t n, float m, hipStream_t s) {
    if (n == 0) return BVC_OK;
    hipLaunchKernelGGL(ema_kernel, dim3(blocks_for((n + 3) / 4)), dim3(256), 0, s, k, q, n, m);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

int launch_iota_mod(int* idx, int n, int L, hipStream_t s) {
    hipLaunchKernelGGL(iota_mod_kernel, dim3(blocks_for((size_t)n)), dim3(256), 0, s, idx, n, L);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

int launch_row_normalize(const float* f, bf16_t* fn, float* inv, int n, int p, float eps, hipStream_t s) {
    BVC_REQUIRE(p % 4 == 0, "row_normalize: width must be a multiple of 4");
    hipLaunchKernelGGL(row_normalize_kernel, dim3((n + 3) / 4), dim3(256), 0, s, f, fn, inv, n, p, eps);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

int launch_row_normalize_bwd(const float* f, const float* inv, const float* dfn, float* df, int n, int p, hipStream_t s) {
    BVC_REQUIRE(p % 4 == 0, "row_normalize_bwd: width must be a multiple of 4");
    hipLaunchKernelGGL(row_normalize_bwd_kernel, dim3((n + 3) / 4), dim3(256), 0, s, f, inv, dfn, df, n, p);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

int launch_nce_finalize(const float* partial, int ntiles, float inv_t, double npos, float* loss, float* stats, hipStream_t s) {
    hipLaunchKernelGGL(nce_finalize_kernel, dim3(1), dim3(256), 0, s, partial, ntiles, inv_t, npos, loss, stats);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

int launch_sgd_step(float* p, float* g, float* buf, size_t n, float lr, float momentum, float dampening, float wd, int nesterov,
                    int first, int maximize, const float* grad_scale, const float* found_inf, int write_grad, bf16_t* shadow,
                    hipStream_t s) {
    BVC_REQUIRE(momentum == 0.f || buf != nullptr, "sgd_step: momentum needs a buffer");
    BVC_REQUIRE(shadow == nullptr || (uintptr_t)shadow % 8 == 0, "sgd_step: the bf16 shadow must be 8-byte aligned");
    BVC_REQUIRE(((uintptr_t)p % 16 == 0) && ((uintptr_t)g % 16 == 0) && (buf == nullptr || (uintptr_t)buf % 16 == 0),
                "sgd_step: buffers must be 16-byte aligned");
    if (n == 0) return BVC_OK;
    hipLaunchKernelGGL(sgd_step_kernel, dim3(blocks_for((n + 3) / 4)), dim3(256), 0, s, p, g, buf, n, lr, momentum, dampening, wd,
                       nesterov, first, maximize, grad_scale, found_inf, write_grad, shadow);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

int launch_adam_prep(float* state, double lr, double beta1, double beta2, const float* found_inf, hipStream_t s) {
    hipLaunchKernelGGL(adam_prep_kernel, dim3(1), dim3(64), 0, s, state, lr, beta1, beta2, found_inf);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

int launch_adam_step(float* p, float* g, float* m, float* v, size_t n, double lr, double beta1, double beta2, double eps, double wd,
                     int decoupled, int maximize, const float* state, const float* grad_scale, const float* found_inf, int write_grad,
                     bf16_t* shadow, hipStream_t s) {
    BVC_REQUIRE(((uintptr_t)p % 16 == 0) && ((uintptr_t)g % 16 == 0) && ((uintptr_t)m % 16 == 0) && ((uintptr_t)v % 16 == 0),
                "adam_step: buffers must be 16-byte aligned");
    BVC_REQUIRE(shadow == nullptr || (uintptr_t)shadow % 8 == 0, "adam_step: the bf16 shadow must be 8-byte aligned");
    if (n == 0) return BVC_OK;
    // hyper-parameters arrive as doubles (python floats) and are combined in double before the cast, as torch does
    hipLaunchKernelGGL(adam_step_kernel, dim3(blocks_for((n + 3) / 4)), dim3(256), 0, s, p, g, m, v, n, (float)(1.0 - beta1), (float)beta2,
                       (float)(1.0 - beta2), (float)eps, (float)wd, (float)(1.0 - lr * wd), decoupled, maximize, state, grad_scale,
                       found_inf, write_grad, shadow);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

static int check_segments(const char* who, int64_t n, const int64_t* seg_start, const int* seg_group, const int* blk_seg, int nseg, int ngroups) {
    BVC_REQUIRE(seg_start && seg_group && blk_seg && nseg > 0, "%s: segment table missing", who);
    BVC_REQUIRE(ngroups >= 1 && ngroups <= BVC_OPT_MAX_GROUPS, "%s: %d parameter groups (1..%d)", who, ngroups, BVC_OPT_MAX_GROUPS);
    BVC_REQUIRE(n > 0, "%s: empty range", who);
    return BVC_OK;
}

int launch_sgd_step_segments(float* p, float* g, float* buf, int64_t n, const int64_t* seg_start, const int* seg_group, const int* blk_seg,
                             int nseg, const bvc_sgd_groups* gr, const float* grad_scale, const float* found_inf, int write_grad,
                             bf16_t* shadow, hipStream_t s) {
    BVC_REQUIRE(gr != nullptr, "sgd_step_segments: groups missing");
    if (int rc = check_segments("sgd_step_segments", n, seg_start, seg_group, blk_seg, nseg, gr->ngroups)) return rc;
    BVC_REQUIRE(((uintptr_t)p % 16 == 0) && ((uintptr_t)g % 16 == 0) && (buf == nullptr || (uintptr_t)buf % 16 == 0),
                "sgd_step_segments: buffers must be 16-byte aligned");
    BVC_REQUIRE(shadow == nullptr || (uintptr_t)shadow % 8 == 0, "sgd_step_segments: the bf16 shadow must be 8-byte aligned");
    SgdGroupsDev G;
    for (int i = 0; i < BVC_OPT_MAX_GROUPS; ++i) {
        const int j = i < gr->ngroups ? i : 0;
        BVC_REQUIRE(gr->momentum[j] == 0.f || buf != nullptr, "sgd_step_segments: momentum needs a buffer");
        G.lr[i] = gr->lr[j]; G.wd[i] = gr->weight_decay[j]; G.momentum[i] = gr->momentum[j]; G.dampening[i] = gr->dampening[j];
        G.flags[i] = (gr->nesterov[j] ? 1 : 0) | (gr->maximize[j] ? 2 : 0) | (gr->first_step[j] ? 4 : 0);
    }
    hipLaunchKernelGGL(sgd_step_seg_kernel, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0, s, p, g, buf, n, seg_start, seg_group, blk_seg, G,
                       grad_scale, found_inf, write_grad, shadow);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

int launch_adam_step_segments(float* p, float* g, float* m, float* v, int64_t n, const int64_t* seg_start, const int* seg_group,
                              const int* blk_seg, int nseg, const bvc_adam_groups* gr, float* state, double* hyper_dev,
                              const float* grad_scale, const float* found_inf, int write_grad, bf16_t* shadow, hipStream_t s) {
    BVC_REQUIRE(gr != nullptr && state != nullptr && hyper_dev != nullptr, "adam_step_segments: groups / state missing");
    if (int rc = check_segments("adam_step_segments", n, seg_start, seg_group, blk_seg, nseg, gr->ngroups)) return rc;
    BVC_REQUIRE(((uintptr_t)p % 16 == 0) && ((uintptr_t)g % 16 == 0) && ((uintptr_t)m % 16 == 0) && ((uintptr_t)v % 16 == 0),
                "adam_step_segments: buffers must be 16-byte aligned");
    BVC_REQUIRE(shadow == nullptr || (uintptr_t)shadow % 8 == 0, "adam_step_segments: the bf16 shadow must be 8-byte aligned");
    AdamGroupsDev G;
    double hyper[3 * BVC_OPT_MAX_GROUPS];
    for (int i = 0; i < BVC_OPT_MAX_GROUPS; ++i) {
        const int j = i < gr->ngroups ? i : 0;
        // hyper-parameters arrive as doubles (python floats) and are combined in double before the cast, as torch does
        G.omb1[i] = (float)(1.0 - gr->beta1[j]); G.beta2[i] = (float)gr->beta2[j]; G.omb2[i] = (float)(1.0 - gr->beta2[j]);
        G.eps[i] = (float)gr->eps[j]; G.wd[i] = (float)gr->weight_decay[j]; G.decay_mul[i] = (float)(1.0 - gr->lr[j] * gr->weight_decay[j]);
        G.flags[i] = (gr->decoupled[j] ? 1 : 0) | (gr->maximize[j] ? 2 : 0);
        hyper[3 * i] = gr->lr[j]; hyper[3 * i + 1] = gr->beta1[j]; hyper[3 * i + 2] = gr->beta2[j];
    }
    // the step-dependent scalars of every group in one tiny launch (lr, beta1, beta2 as doubles: 192 bytes through a pageable copy)
    BVC_CHECK_HIP(hipMemcpyAsync(hyper_dev, hyper, sizeof(double) * 3 * gr->ngroups, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(adam_prep_groups_kernel, dim3(1), dim3(64), 0, s, state, gr->ngroups, hyper_dev, found_inf);
    hipLaunchKernelGGL(adam_step_seg_kernel, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0, s, p, g, m, v, n, seg_start, seg_group, blk_seg, G, state,
                       grad_scale, found_inf, write_grad, shadow);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

static int check_table(const char* who, int64_t n, const int64_t* seg_start, const int* seg_group, const int* blk_seg, int nseg, int ngroups,
                       const float* table) {
    BVC_REQUIRE(seg_start && seg_group && blk_seg && nseg > 0, "%s: segment table missing", who);
    BVC_REQUIRE(ngroups >= 1 && ngroups <= BVC_OPT_TABLE_MAX_GROUPS, "%s: %d parameter groups (1..%d)", who, ngroups, BVC_OPT_TABLE_MAX_GROUPS);
    BVC_REQUIRE(table != nullptr && (uintptr_t)table % 16 == 0, "%s: the group table must be a 16-byte aligned device buffer", who);
    BVC_REQUIRE(n > 0, "%s: empty range", who);
    return BVC_OK;
}

int launch_sgd_step_table(float* p, float* g, float* buf, int64_t n, const int64_t* seg_start, const int* seg_group, const int* blk_seg,
                          int nseg, int ngroups, const float* lr, const float* momentum, const float* dampening, const float* wd,
                          const int* nesterov, const int* first_step, const int* maximize, float* table, const float* grad_scale,
                          const float* found_inf, int write_grad, bf16_t* shadow, hipStream_t s) {
    if (int rc = check_table("sgd_step_table", n, seg_start, seg_group, blk_seg, nseg, ngroups, table)) return rc;
    BVC_REQUIRE(lr && momentum && dampening && wd && nesterov && first_step && maximize, "sgd_step_table: hyper-parameter array missing");
    BVC_REQUIRE(((uintptr_t)p % 16 == 0) && ((uintptr_t)g % 16 == 0) && (buf == nullptr || (uintptr_t)buf % 16 == 0),
                "sgd_step_table: buffers must be 16-byte aligned");
    BVC_REQUIRE(shadow == nullptr || (uintptr_t)shadow % 8 == 0, "sgd_step_table: the bf16 shadow must be 8-byte aligned");
    for (int i = 0; i < ngroups; ++i) BVC_REQUIRE(momentum[i] == 0.f || buf != nullptr, "sgd_step_table: momentum needs a buffer");
    for (int g0 = 0; g0 < ngroups; g0 += BVC_OPT_TABLE_CHUNK) {
        const int count = ngroups - g0 < BVC_OPT_TABLE_CHUNK ? ngroups - g0 : BVC_OPT_TABLE_CHUNK;
        SgdChunkDev C;
        for (int t = 0; t < BVC_OPT_TABLE_CHUNK; ++t) {
            const int j = g0 + (t < count ? t : 0);
            C.lr[t] = lr[j]; C.wd[t] = wd[j]; C.momentum[t] = momentum[j]; C.dampening[t] = dampening[j];
            C.flags[t] = (nesterov[j] ? 1 : 0) | (maximize[j] ? 2 : 0) | (first_step[j] ? 4 : 0);
        }
        hipLaunchKernelGGL(sgd_table_write_kernel, dim3(1), dim3(BVC_OPT_TABLE_CHUNK), 0, s, table, g0, count, C);
    }
    hipLaunchKernelGGL(sgd_step_table_kernel, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0, s, p, g, buf, n, seg_start, seg_group, blk_seg,
                       (const float*)table, ngroups, grad_scale, found_inf, write_grad, shadow);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

int launch_adam_step_table(float* p, float* g, float* m, float* v, int64_t n, const int64_t* seg_start, const int* seg_group,
                           const int* blk_seg, int nseg, int ngroups, const double* lr, const double* beta1, const double* beta2,
                           const double* eps, const double* wd, const int* decoupled, const int* maximize, float* state, float* table,
                           const float* grad_scale, const float* found_inf, int write_grad, bf16_t* shadow, hipStream_t s) {
    if (int rc = check_table("adam_step_table", n, seg_start, seg_group, blk_seg, nseg, ngroups, table)) return rc;
    BVC_REQUIRE(lr && beta1 && beta2 && eps && wd && decoupled && maximize && state, "adam_step_table: hyper-parameter array / state missing");
    BVC_REQUIRE(((uintptr_t)p % 16 == 0) && ((uintptr_t)g % 16 == 0) && ((uintptr_t)m % 16 == 0) && ((uintptr_t)v % 16 == 0),
                "adam_step_table: buffers must be 16-byte aligned");
    BVC_REQUIRE(shadow == nullptr || (uintptr_t)shadow % 8 == 0, "adam_step_table: the bf16 shadow must be 8-byte aligned");
    for (int g0 = 0; g0 < ngroups; g0 += BVC_OPT_TABLE_CHUNK) {
        const int count = ngroups - g0 < BVC_OPT_TABLE_CHUNK ? ngroups - g0 : BVC_OPT_TABLE_CHUNK;
        AdamChunkDev C;
        for (int t = 0; t < BVC_OPT_TABLE_CHUNK; ++t) {
            const int j = g0 + (t < count ? t : 0);
            // hyper-parameters arrive as doubles (python floats) and are combined in double before the cast, as torch does - on the
            // host, with the very expressions of launch_adam_step_segments, so that both paths hand the kernels the same floats
            C.omb1[t] = (float)(1.0 - beta1[j]); C.beta2f[t] = (float)beta2[j]; C.omb2[t] = (float)(1.0 - beta2[j]);
            C.eps[t] = (float)eps[j]; C.wd[t] = (float)wd[j]; C.decay_mul[t] = (float)(1.0 - lr[j] * wd[j]);
            C.flags[t] = (decoupled[j] ? 1 : 0) | (maximize[j] ? 2 : 0);
            C.lr[t] = lr[j]; C.beta1[t] = beta1[j]; C.beta2[t] = beta2[j];
        }
        hipLaunchKernelGGL(adam_prep_table_kernel, dim3(1), dim3(BVC_OPT_TABLE_CHUNK), 0, s, state, table, g0, count, C, found_inf);
    }
    hipLaunchKernelGGL(adam_step_table_kernel, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0, s, p, g, m, v, n, seg_start, seg_group, blk_seg,
                       (const float*)table, ngroups, (const float*)state, grad_scale, found_inf, write_grad, shadow);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

int launch_pad_heads(const bf16_t* wqkv, const float* bqkv, const bf16_t* wo, bf16_t* wqkv_p, float* bqkv_p, bf16_t* wo_p, int D, int H,
                     int hd, int hdp, hipStream_t s) {
    hipLaunchKernelGGL(pad_qkv_kernel, dim3(3 * H * hdp), dim3(128), 0, s, wqkv, bqkv, wqkv_p, bqkv_p, H, hd, hdp, D);
    hipLaunchKernelGGL(pad_cols_kernel, dim3(D), dim3(128), 0, s, wo, wo_p, D, H, hd, hdp);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

int launch_unpad_head_grads(const float* gwqkv_p, const float* gbqkv_p, const float* gwo_p, float* gwqkv, float* gbqkv, float* gwo, int D,
                            int H, int hd, int hdp, hipStream_t s) {
    hipLaunchKernelGGL(unpad_qkv_grad_kernel, dim3(3 * H * hd), dim3(128), 0, s, gwqkv_p, gbqkv_p, gwqkv, gbqkv, H, hd, hdp, D);
    hipLaunchKernelGGL(unpad_cols_grad_kernel, dim3(D), dim3(128), 0, s, gwo_p, gwo, D, H, hd, hdp);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

int launch_nonfinite_check(const float* x, size_t n, float* found_inf, hipStream_t s) {
    BVC_REQUIRE(((uintptr_t)x % 16) == 0, "nonfinite_check: buffer must be 16-byte aligned");
    if (n == 0) return BVC_OK;
    const size_t want = (n / 4 + 255) / 256 + 1;
    const unsigned blocks = (unsigned)(want < 8192 ? want : 8192);
    hipLaunchKernelGGL(nonfinite_check_kernel, dim3(blocks), dim3(256), 0, s, x, n, found_inf);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

int grad_norm_chain() { return kNormChain; }

// The static work list of a segment table (host): every owned segment (seg_group >= 0) is cut front to back into items of at most
// kNormItemCap elements, in segment order, so that the items of a segment are adjacent and ascending; seg_first_item[s] is the index
// of segment s's first item (seg_first_item[nseg] = the item count).  items == nullptr: count only.
int grad_norm_items_host(const int64_t* seg_start, const int32_t* seg_group, int nseg, bvc_norm_item* items, int64_t items_cap,
                         int64_t* seg_first_item, int64_t* nitems) {
    int64_t count = 0;
    for (int s = 0; s < nseg; ++s) {
        BVC_REQUIRE(seg_start[s] <= seg_start[s + 1], "grad_norm_items: seg_start must ascend (segment %d)", s);
        if (seg_first_item) seg_first_item[s] = count;
        if (seg_group[s] < 0) continue;
        for (int64_t at = seg_start[s]; at < seg_start[s + 1]; at += kNormItemCap) {
            const int64_t left = seg_start[s + 1] - at;
            if (items) {
                BVC_REQUIRE(count < items_cap, "grad_norm_items: more than the %lld items the caller has room for", (long long)items_cap);
                items[count] = bvc_norm_item{at, (int32_t)(left < kNormItemCap ? left : kNormItemCap), (int32_t)s};
            }
            ++count;
        }
    }
    if (seg_first_item) seg_first_item[nseg] = count;
    *nitems = count;
    return BVC_OK;
}

int launch_grad_sqnorm_items(const float* x, const bvc_norm_item* items, int64_t nitems, const int64_t* seg_first_item, int nseg,
                             double* item_partial, float* seg_sq, float* total_sq, int as_norm, float* found_inf, hipStream_t s) {
    BVC_REQUIRE(((uintptr_t)x % 4) == 0, "grad_sqnorm_items: the range must be 4-byte aligned");
    BVC_REQUIRE(nitems <= 0x7fffffff, "grad_sqnorm_items: %lld items", (long long)nitems);
    BVC_REQUIRE(nitems == 0 || (items != nullptr && item_partial != nullptr), "grad_sqnorm_items: item table / partials missing");
    BVC_REQUIRE(seg_sq == nullptr || (seg_first_item != nullptr && nseg >= 0), "grad_sqnorm_items: seg_sq needs seg_first_item");
    if (nitems > 0)
        hipLaunchKernelGGL(grad_sqnorm_items_kernel, dim3((unsigned)nitems), dim3(256), 0, s, x, items, item_partial, found_inf);
    hipLaunchKernelGGL(grad_sqnorm_reduce_kernel, dim3(seg_sq ? (unsigned)nseg + 1 : 1u), dim3(256), 0, s, (const double*)item_partial,
                       seg_first_item, nseg, nitems, seg_sq, total_sq, as_norm);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

int launch_clip_finalize(const float* sq, int nranges, float max_norm, const float* grad_scale, float* out3, hipStream_t s) {
    hipLaunchKernelGGL(clip_finalize_kernel, dim3(1), dim3(64), 0, s, sq, nranges, max_norm, grad_scale, out3);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

int launch_scale_by_dev(float* x, size_t n, const float* coef, hipStream_t s) {
    if (n == 0) return BVC_OK;
    const size_t want = (n / 4 + 255) / 256 + 1;
    hipLaunchKernelGGL(scale_by_dev_kernel, dim3((unsigned)(want < 8192 ? want : 8192)), dim3(256), 0, s, x, n, coef);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

int launch_loss_finalize(const float* partial, int n, double count, const int* status, float* loss, hipStream_t s) {
    hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(256), 0, s, partial, n, count, status, loss);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

}  // namespace bvc

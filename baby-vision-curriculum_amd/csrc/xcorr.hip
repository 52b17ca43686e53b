// Feature cross-correlation with a reduced epilogue (bvc_op_xcorr_fwd / _bwd): x f32 [n][p], y f32 [n][q] (y may alias x),
//     mu_j = mean_i x_ij,  var_j = sum_i (x_ij - mu_j)^2 / (n - ddof),  r_j = norm ? 1 / sqrt(var_j + eps) : 1,  xh_ij = (x_ij - mu_j) r_j,
//     C = scale xh^T yh  [p][q],   on = sum_i (C_ii - t)^2,   off = sum_{i != j} C_ij^2.
// Barlow Twins (norm 1, scale 1 / n, t 1), VICReg's covariance term (alias, norm 0, scale 1 / (n - 1), w_on 0) and linear CKA
// (norm 0, scale 1, t 0: on + off = |xc^T yc|_F^2) are parameter settings.  Backward, for w = {d / d on, d / d off} on the device:
//     G_ii = 2 w_on (C_ii - t),  G_ij = 2 w_off C_ij,   dxh = scale yh G^T,   dyh = scale xh G   (alias: dxh = scale xh (G + G^T) = 2 scale xh G,
//     C is symmetric bit for bit there),   a_j = dvar_j - (norm ? r_j^2 / 2 sum_i dxh_ij xh_ij : 0),
//     dx_ij = r_j (dxh_ij - mean_i' dxh_i'j) + 2 (x_ij - mu_j) a_j / (n - ddof).
//
// Arithmetic: f32 throughout, every element of C ONE accumulation chain over the rows in ascending order on v_mfma_f32_32x32x2_f32.
// The three products are f32t_product of f32_tile.h, C [128][128] = A [128][K] . B [128][K]^T over padded operands in the workspace;
// the epilogues below take their rows (A side) and columns (B side) from its helpers.
//   prologue  xc_stats_kernel: column mean and variance, summed in f64 in a fixed order, one rounding to f32.  xc_centre_kernel: from
//             the ROUNDED mean and variance (what the backward is handed), the transposed operand xhT [p][nK] (nK = n up to 32, the
//             contraction index contiguous) and, in the backward, the row-major xh [n][pK] (pK = p up to 32).  Elements beyond n or p
//             are zero BY INDEX: x - mu of a padded zero is not zero.
//   forward   xc_fwd_kernel, one workgroup per 128 x 128 tile of C: the K loop over the rows, then every lane squares its 64
//             elements (c - t on the diagonal, decided by index) into two f64 sums, a fixed tree folds the workgroup, the tile's
//             (on, off) goes to the workspace; xc_final_kernel adds the tiles in a fixed order in f64 and rounds once.  No [p][q] array.
//   backward  for blocks of R columns of x: xc_g_kernel recomputes that block of C and writes scale G [R][qK]; xc_dxh_kernel is
//             yh [n][qK] . G [R][qK]^T = dxh [n][R] on the same loop; xc_dx_kernel sums each column's dxh and dxh xh in f64 in a fixed
//             order and writes dx.  Then the same for blocks of columns of y with the operands' roles swapped (G^T is recomputed, not
//             transposed: every element of dyh stays one chain over all p).  The alias case runs the first pass only, with 2 G.
// No atomics: the same bits on every run and for every blocking.  Nothing in the workspace survives a call.
#include "f32_tile.h"
#include "xcorr.h"

#include <math.h>

namespace bvc {
namespace {

// ---------------------------------------------------------------- prologue
// 32 columns per workgroup, 8 row lanes: lane ry sums rows ry, ry + 8, .. in f64, the 8 partials are added in ascending order
__global__ __launch_bounds__(256) void xc_stats_kernel(const float* __restrict__ x, int64_t ld, int n, int p, int ddof,
                                                       float* __restrict__ mean, float* __restrict__ var) {
    __shared__ double sh[8][32];
    const int c = threadIdx.x & 31, ry = threadIdx.x >> 5;
    const int col = blockIdx.x * 32 + c;
    const bool ok = col < p;
    double s = 0.0;
    if (ok)
        for (int i = ry; i < n; i += 8) s += (double)x[(int64_t)i * ld + col];
    sh[ry][c] = s;
    __syncthreads();
    double tot = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) tot += sh[k][c];
    const double mu = tot / (double)n;
    __syncthreads();
    double v = 0.0;
    if (ok)
        for (int i = ry; i < n; i += 8) {
            const double d = (double)x[(int64_t)i * ld + col] - mu;
            v = fma(d, d, v);
        }
    sh[ry][c] = v;
    __syncthreads();
    if (ry == 0 && ok) {
        double vt = 0.0;
#pragma unroll
        for (int k = 0; k < 8; ++k) vt += sh[k][c];
        mean[col] = (float)mu;
        var[col] = (float)(vt / (double)(n - ddof));
    }
}

__device__ __forceinline__ float xc_rscale(float var, int norm, float eps) { return norm ? 1.0f / sqrtf(var + eps) : 1.0f; }

// 32 x 32 tiles of (x - mu) r: xh [n][pK] (when not null) and xhT [p][nK]; zero beyond n and p, by index
__global__ __launch_bounds__(256) void xc_centre_kernel(const float* __restrict__ x, int64_t ld, int n, int p, int nK, int pK,
                                                        const float* __restrict__ mean, const float* __restrict__ var, int norm, float eps,
                                                        float* __restrict__ xh, float* __restrict__ xhT) {
    __shared__ float t[32][33];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int j0 = blockIdx.x * 32, i0 = blockIdx.y * 32;
    const int col = j0 + tx;
    const float mu = col < p ? mean[col] : 0.f;
    const float r = col < p ? xc_rscale(var[col], norm, eps) : 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = i0 + ty + 8 * k;
        const float v = (i < n && col < p) ? (x[(int64_t)i * ld + col] - mu) * r : 0.f;
        t[ty + 8 * k][tx] = v;
        if (xh && i < n) xh[(int64_t)i * pK + col] = v;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int j = j0 + ty + 8 * k;
        if (j < p) xhT[(int64_t)j * nK + i0 + tx] = t[tx][ty + 8 * k];
    }
}

// ---------------------------------------------------------------- forward
struct XcFwdArgs {
    const float* xhT; const float* yhT;
    double* part;                // [tiles][2]: on, off
    int p, q, nK;
    float scale, target;
};

__global__ __launch_bounds__(256) void xc_fwd_kernel(XcFwdArgs a) {
    __shared__ __attribute__((aligned(16))) float ldsA[kF32Tile * kF32Row];
    __shared__ __attribute__((aligned(16))) float ldsB[kF32Tile * kF32Row];
    __shared__ double red[2][256];
    const int tid = threadIdx.x;
    const F32TileLane L = f32t_lane(tid);
    const int ptiles = (a.p + kF32Tile - 1) / kF32Tile;
    const int rt = blockIdx.x % ptiles, ct = blockIdx.x / ptiles;
    f32x16 acc[2][2];
    f32t_product(a.xhT, a.nK, rt * kF32Tile, a.p, a.yhT, a.nK, ct * kF32Tile, a.q, a.nK, ldsA, ldsB, tid, acc);
    double on = 0.0, off = 0.0;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int cb = F32T_BROW(L, ct * kF32Tile, j);
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int ca = F32T_AROW(L, rt * kF32Tile, i, e);
                if (ca < a.p && cb < a.q) {
                    const float c = acc[i][j][e] * a.scale;
                    if (ca == cb) {
                        const double d = (double)(c - a.target);
                        on = fma(d, d, on);
                    } else {
                        off = fma((double)c, (double)c, off);
                    }
                }
            }
        }
    red[0][tid] = on;
    red[1][tid] = off;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) { red[0][tid] += red[0][tid + o]; red[1][tid] += red[1][tid + o]; }
        __syncthreads();
    }
    if (tid == 0) {
        a.part[(int64_t)blockIdx.x * 2] = red[0][0];
        a.part[(int64_t)blockIdx.x * 2 + 1] = red[1][0];
    }
}

// stats = {on, off}: thread t sums tiles t, t + 256, .. in f64, then a fixed tree, one rounding
__global__ __launch_bounds__(256) void xc_final_kernel(const double* __restrict__ part, int tiles, float* __restrict__ stats2) {
    __shared__ double red[2][256];
    double on = 0.0, off = 0.0;
    for (int i = threadIdx.x; i < tiles; i += 256) { on += part[(int64_t)i * 2]; off += part[(int64_t)i * 2 + 1]; }
    red[0][threadIdx.x] = on;
    red[1][threadIdx.x] = off;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) { red[0][threadIdx.x] += red[0][threadIdx.x + o]; red[1][threadIdx.x] += red[1][threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { stats2[0] = (float)red[0][0]; stats2[1] = (float)red[1][0]; }
}

// ---------------------------------------------------------------- backward
// One pass: the gradient of the operand "own" (width po, its columns index the rows of G) against "other" (width qo).
struct XcBwdArgs {
    const float* ownT; const float* otherT;      // [po][nK], [qo][nK]
    const float* own; const float* other;        // [n][poK], [n][qoK]
    const float* src; int64_t ldsrc;             // the own operand as given
    const float* mean; const float* var; const float* dvar; const float* w;
    float* G;                    // [rb][qoK]
    float* dxh;                  // [n][R]
    float* dout; int64_t lddout;
    int n, nK, po, qo, poK, qoK, R, c0, rb;      // this block: own columns c0 .. c0 + rb
    int norm, ddof;
    float eps, scale, target, factor;            // factor 2 in the alias case (G + G^T)
};

// G [a - c0][b] = factor scale 2 (a == b ? w_on (C_ab - t) : w_off C_ab);  0 for b beyond qo (the K tail of the next product)
__global__ __launch_bounds__(256) void xc_g_kernel(XcBwdArgs a) {
    __shared__ __attribute__((aligned(16))) float ldsA[kF32Tile * kF32Row];
    __shared__ __attribute__((aligned(16))) float ldsB[kF32Tile * kF32Row];
    const int tid = threadIdx.x;
    const F32TileLane L = f32t_lane(tid);
    const int rtiles = (a.rb + kF32Tile - 1) / kF32Tile;
    const int rt = blockIdx.x % rtiles, ct = blockIdx.x / rtiles;
    const int a0 = a.c0 + rt * kF32Tile, b0 = ct * kF32Tile;
    const float f = 2.0f * a.scale * a.factor;
    const float won = a.w[0] * f, woff = a.w[1] * f;
    f32x16 acc[2][2];
    f32t_product(a.ownT, a.nK, a0, a.po, a.otherT, a.nK, b0, a.qo, a.nK, ldsA, ldsB, tid, acc);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int ca = F32T_AROW(L, a0, i, e);
            if (ca >= a.c0 + a.rb) continue;
            float* grow = a.G + (int64_t)(ca - a.c0) * a.qoK;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int cb = F32T_BROW(L, b0, j);
                if (cb >= a.qoK) continue;
                const float c = acc[i][j][e] * a.scale;
                const float v = ca == cb ? won * (c - a.target) : woff * c;
                grow[cb] = cb < a.qo ? v : 0.f;
            }
        }
}

// dxh [i][a - c0] = sum_b other [i][b] G [a - c0][b]
__global__ __launch_bounds__(256) void xc_dxh_kernel(XcBwdArgs a) {
    __shared__ __attribute__((aligned(16))) float ldsA[kF32Tile * kF32Row];
    __shared__ __attribute__((aligned(16))) float ldsB[kF32Tile * kF32Row];
    const int tid = threadIdx.x;
    const F32TileLane L = f32t_lane(tid);
    const int ctiles = (a.rb + kF32Tile - 1) / kF32Tile;
    const int ct = blockIdx.x % ctiles, rt = blockIdx.x / ctiles;
    f32x16 acc[2][2];
    f32t_product(a.other, a.qoK, rt * kF32Tile, a.n, a.G, a.qoK, ct * kF32Tile, a.rb, a.qoK, ldsA, ldsB, tid, acc);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int row = F32T_AROW(L, rt * kF32Tile, i, e);
            if (row >= a.n) continue;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int c = F32T_BROW(L, ct * kF32Tile, j);
                if (c < a.rb) a.dxh[(int64_t)row * a.R + c] = acc[i][j][e];
            }
        }
}

// 32 columns of the block per workgroup: column sums of dxh and dxh xh in f64 (8 row lanes, added in ascending order), then dx
__global__ __launch_bounds__(256) void xc_dx_kernel(XcBwdArgs a) {
    __shared__ double sh[2][8][32];
    const int c = threadIdx.x & 31, ry = threadIdx.x >> 5;
    const int cl = blockIdx.x * 32 + c;
    const int col = a.c0 + cl;
    const bool ok = cl < a.rb;
    double s1 = 0.0, s2 = 0.0;
    if (ok)
        for (int i = ry; i < a.n; i += 8) {
            const double d = (double)a.dxh[(int64_t)i * a.R + cl];
            s1 += d;
            s2 = fma(d, (double)a.own[(int64_t)i * a.poK + col], s2);
        }
    sh[0][ry][c] = s1;
    sh[1][ry][c] = s2;
    __syncthreads();
    if (!ok) return;
    double t1 = 0.0, t2 = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) { t1 += sh[0][k][c]; t2 += sh[1][k][c]; }
    const float mu = a.mean[col];
    const float r = xc_rscale(a.var[col], a.norm, a.eps);
    const float m1 = (float)(t1 / (double)a.n);
    const float av = (a.dvar ? a.dvar[col] : 0.f) - (a.norm ? 0.5f * r * r * (float)t2 : 0.f);
    const float coef = 2.0f * av / (float)(a.n - a.ddof);
    for (int i = ry; i < a.n; i += 8) {
        const float d = a.dxh[(int64_t)i * a.R + cl];
        a.dout[(int64_t)i * a.lddout + col] = fmaf(a.src[(int64_t)i * a.ldsrc + col] - mu, coef, r * (d - m1));
    }
}

// ---------------------------------------------------------------- host side
int xc_k(int v) { return (v + kF32KStep - 1) / kF32KStep * kF32KStep; }
int xc_tiles(int v) { return (v + kF32Tile - 1) / kF32Tile; }

int xc_check_shape(const char* who, int n, int p, int q, int block_cols) {
    BVC_REQUIRE(n >= 1 && n <= kXcMaxN, "%s: n %d outside 1 .. %d", who, n, kXcMaxN);
    BVC_REQUIRE(p >= 1 && p <= kXcMaxP, "%s: p %d outside 1 .. %d", who, p, kXcMaxP);
    BVC_REQUIRE(q >= 1 && q <= kXcMaxP, "%s: q %d outside 1 .. %d", who, q, kXcMaxP);
    BVC_REQUIRE(block_cols >= 0, "%s: negative block_cols %d", who, block_cols);
    return BVC_OK;
}

int xc_check_args(const char* who, const float* x, int64_t ldx, const float* y, int64_t ldy, int n, int p, int q, int norm, int ddof,
                  float eps, float scale, float target, const void* workspace) {
    BVC_REQUIRE(norm == 0 || norm == 1, "%s: norm %d is neither 0 nor 1", who, norm);
    BVC_REQUIRE(ddof == 0 || ddof == 1, "%s: ddof %d is neither 0 nor 1", who, ddof);
    BVC_REQUIRE(n - ddof >= 1, "%s: n - ddof = %d leaves nothing to divide by", who, n - ddof);
    BVC_REQUIRE(isfinite(scale) && scale > 0.f, "%s: scale %g is not a positive finite number", who, (double)scale);
    BVC_REQUIRE(isfinite(target), "%s: diag_target %g is not finite", who, (double)target);
    BVC_REQUIRE(!norm || (isfinite(eps) && eps > 0.f), "%s: eps %g is not a positive finite number", who, (double)eps);
    BVC_REQUIRE(x && y && workspace, "%s: null argument", who);
    BVC_REQUIRE(ldx >= p, "%s: row stride of x %lld below p %d", who, (long long)ldx, p);
    BVC_REQUIRE(ldy >= q, "%s: row stride of y %lld below q %d", who, (long long)ldy, q);
    BVC_REQUIRE(x != y || (q == p && ldy == ldx), "%s: alias of x and y with q %d != p %d or ldy %lld != ldx %lld", who, q, p, (long long)ldy,
                (long long)ldx);
    BVC_REQUIRE(((uintptr_t)x & 3) == 0 && ((uintptr_t)y & 3) == 0 && ((uintptr_t)workspace & 15) == 0,
                "%s: x and y must be 4-byte, the workspace 16-byte aligned", who);
    return BVC_OK;
}

// whole tiles of columns under the cap of the G block, at least one tile, at most all columns
int xc_auto_block_cols(int p, int q) {
    const int wide = xc_k(p > q ? p : q), most = xc_tiles(p > q ? p : q) * kF32Tile;
    int64_t r = kXcGBlockBytes / ((int64_t)wide * 4) / kF32Tile * kF32Tile;
    if (r < kF32Tile) r = kF32Tile;
    if (r > most) r = most;
    return (int)r;
}
int xc_resolve_block_cols(int p, int q, int block_cols) {
    if (block_cols <= 0) return xc_auto_block_cols(p, q);
    const int most = xc_tiles(p > q ? p : q) * kF32Tile;
    const int64_t r = ((int64_t)block_cols + kF32Tile - 1) / kF32Tile * kF32Tile;
    return (int)(r > most ? most : r);
}

struct XcLayout {
    int nK, pK, qK, R;
    int64_t xhT, yhT, xh, yh, part, G, dxh, total;
};
XcLayout xc_layout(int n, int p, int q, bool alias, int block_cols, bool backward) {
    XcLayout w{};
    w.nK = xc_k(n); w.pK = xc_k(p); w.qK = xc_k(q);
    w.R = xc_resolve_block_cols(p, q, block_cols);
    int64_t o = 0;
    w.xhT = o; o += ws_align((int64_t)p * w.nK * 4);
    w.yhT = alias ? w.xhT : o; if (!alias) o += ws_align((int64_t)q * w.nK * 4);
    if (backward) {
        w.xh = o; o += ws_align((int64_t)n * w.pK * 4);
        w.yh = alias ? w.xh : o; if (!alias) o += ws_align((int64_t)n * w.qK * 4);
        w.G = o; o += ws_align((int64_t)w.R * (w.pK > w.qK ? w.pK : w.qK) * 4);
        w.dxh = o; o += ws_align((int64_t)n * w.R * 4);
    } else {
        w.part = o; o += ws_align((int64_t)xc_tiles(p) * xc_tiles(q) * 16);
    }
    w.total = o;
    return w;
}

int xc_centre(const float* x, int64_t ld, int n, int p, int nK, int pK, const float* mean, const float* var, int norm, float eps, float* xh,
              float* xhT, hipStream_t s) {
    xc_centre_kernel<<<dim3((unsigned)(pK / 32), (unsigned)(nK / 32)), dim3(256), 0, s>>>(x, ld, n, p, nK, pK, mean, var, norm, eps, xh, xhT);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

int xc_pass(XcBwdArgs a, hipStream_t s) {
    const int otiles = xc_tiles(a.qoK), ntiles = xc_tiles(a.n);
    for (int c0 = 0; c0 < a.po; c0 += a.R) {
        a.c0 = c0;
        a.rb = a.po - c0 < a.R ? a.po - c0 : a.R;
        const int btiles = xc_tiles(a.rb);
        xc_g_kernel<<<dim3((unsigned)(btiles * otiles)), dim3(256), 0, s>>>(a);
        xc_dxh_kernel<<<dim3((unsigned)(btiles * ntiles)), dim3(256), 0, s>>>(a);
        xc_dx_kernel<<<dim3((unsigned)((a.rb + 31) / 32)), dim3(256), 0, s>>>(a);
        BVC_CHECK_HIP(hipGetLastError());
    }
    return BVC_OK;
}

}  // namespace

int xcorr_block_cols(int n, int p, int q) {
    if (xc_check_shape("op_xcorr_block_cols", n, p, q, 0) != BVC_OK) return -1;
    return xc_auto_block_cols(p, q);
}

int64_t xcorr_workspace(int n, int p, int q, int alias, int block_cols, int backward) {
    if (xc_check_shape("op_xcorr_workspace", n, p, q, block_cols) != BVC_OK) return -1;
    if (alias && q != p) { set_error("op_xcorr_workspace: alias with q %d != p %d", q, p); return -1; }
    return xc_layout(n, p, q, alias != 0, block_cols, backward != 0).total;
}

int launch_xcorr_fwd(const float* x, int64_t ldx, const float* y, int64_t ldy, int n, int p, int q, int norm, int ddof, float eps, float scale,
                     float diag_target, float* mean_x, float* var_x, float* mean_y, float* var_y, float* stats2, void* workspace, hipStream_t s) {
    const char* who = "op_xcorr_fwd";
    if (int rc = xc_check_shape(who, n, p, q, 0)) return rc;
    if (int rc = xc_check_args(who, x, ldx, y, ldy, n, p, q, norm, ddof, eps, scale, diag_target, workspace)) return rc;
    const bool alias = x == y;
    BVC_REQUIRE(mean_x && var_x && stats2 && (alias || (mean_y && var_y)), "%s: null argument", who);
    const XcLayout w = xc_layout(n, p, q, alias, 0, false);
    float* xhT = ws_at<float>(workspace, w.xhT);
    float* yhT = ws_at<float>(workspace, w.yhT);
    xc_stats_kernel<<<dim3((unsigned)((p + 31) / 32)), dim3(256), 0, s>>>(x, ldx, n, p, ddof, mean_x, var_x);
    if (int rc = xc_centre(x, ldx, n, p, w.nK, w.pK, mean_x, var_x, norm, eps, nullptr, xhT, s)) return rc;
    if (!alias) {
        xc_stats_kernel<<<dim3((unsigned)((q + 31) / 32)), dim3(256), 0, s>>>(y, ldy, n, q, ddof, mean_y, var_y);
        if (int rc = xc_centre(y, ldy, n, q, w.nK, w.qK, mean_y, var_y, norm, eps, nullptr, yhT, s)) return rc;
    }
    const int tiles = xc_tiles(p) * xc_tiles(q);
    XcFwdArgs a{xhT, yhT, ws_at<double>(workspace, w.part), p, q, w.nK, scale, diag_target};
    xc_fwd_kernel<<<dim3((unsigned)tiles), dim3(256), 0, s>>>(a);
    xc_final_kernel<<<dim3(1), dim3(256), 0, s>>>(a.part, tiles, stats2);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

int launch_xcorr_bwd(const float* x, int64_t ldx, const float* y, int64_t ldy, int n, int p, int q, int norm, int ddof, float eps, float scale,
                     float diag_target, const float* mean_x, const float* var_x, const float* mean_y, const float* var_y, const float* w,
                     const float* dvar_x, const float* dvar_y, int block_cols, float* dx, int64_t lddx, float* dy, int64_t lddy,
                     void* workspace, hipStream_t s) {
    const char* who = "op_xcorr_bwd";
    if (int rc = xc_check_shape(who, n, p, q, block_cols)) return rc;
    if (int rc = xc_check_args(who, x, ldx, y, ldy, n, p, q, norm, ddof, eps, scale, diag_target, workspace)) return rc;
    const bool alias = x == y;
    BVC_REQUIRE(!(alias && dy), "%s: dy must be null in the alias case", who);
    BVC_REQUIRE(mean_x && var_x && w && dx && (alias || (mean_y && var_y && dy)), "%s: null argument", who);
    BVC_REQUIRE(lddx >= p, "%s: row stride of dx %lld below p %d", who, (long long)lddx, p);
    BVC_REQUIRE(alias || lddy >= q, "%s: row stride of dy %lld below q %d", who, (long long)lddy, q);
    const XcLayout l = xc_layout(n, p, q, alias, block_cols, true);
    float* xhT = ws_at<float>(workspace, l.xhT);
    float* yhT = ws_at<float>(workspace, l.yhT);
    float* xh = ws_at<float>(workspace, l.xh);
    float* yh = ws_at<float>(workspace, l.yh);
    if (int rc = xc_centre(x, ldx, n, p, l.nK, l.pK, mean_x, var_x, norm, eps, xh, xhT, s)) return rc;
    if (!alias)
        if (int rc = xc_centre(y, ldy, n, q, l.nK, l.qK, mean_y, var_y, norm, eps, yh, yhT, s)) return rc;
    XcBwdArgs a{};
    a.w = w; a.G = ws_at<float>(workspace, l.G); a.dxh = ws_at<float>(workspace, l.dxh);
    a.n = n; a.nK = l.nK; a.R = l.R; a.norm = norm; a.ddof = ddof; a.eps = eps; a.scale = scale; a.target = diag_target;
    a.factor = alias ? 2.0f : 1.0f;
    a.ownT = xhT; a.otherT = yhT; a.own = xh; a.other = yh; a.src = x; a.ldsrc = ldx; a.mean = mean_x; a.var = var_x; a.dvar = dvar_x;
    a.dout = dx; a.lddout = lddx; a.po = p; a.qo = q; a.poK = l.pK; a.qoK = l.qK;
    if (int rc = xc_pass(a, s)) return rc;
    if (!alias) {
        a.ownT = yhT; a.otherT = xhT; a.own = yh; a.other = xh; a.src = y; a.ldsrc = ldy; a.mean = mean_y; a.var = var_y; a.dvar = dvar_y;
        a.dout = dy; a.lddout = lddy; a.po = q; a.qo = p; a.poK = l.qK; a.qoK = l.pK;
        if (int rc = xc_pass(a, s)) return rc;
    }
    return BVC_OK;
}

}  // namespace bvc

// Prototype cross-entropy, the loss of DINO / the [CLS] half of iBOT and DINOv2 (bvc_op_proto_ce_fwd / _bwd): m paired student and
// teacher rows xs, xt [m][p] scored against K student and teacher prototypes vs, vt [K][p] (the weight-normalised last layer of a
// DINO head with gain 1), an optional per-prototype shift center [K]:
//     xsn_i = xs_i / max(|xs_i|, eps),  wsn_k = vs_k / |vs_k| (0 for a zero row),  xtn, wtn likewise,
//     s_ik = xsn_i . wsn_k / tau_s,     t_ik = (xtn_i . wtn_k - center_k) / tau_t,
//     Ls_i = log sum_k exp(s_ik),       Lt_i = log sum_k exp(t_ik),       q_ik = exp(t_ik - Lt_i),
//     l_i = Ls_i - sum_k q_ik s_ik,     loss = sum_i l_i / m,             bc_k = (1 / m) sum_i xtn_i . wtn_k.
// Backward, per-row weights w_i, no gradient on the teacher side:
//     dS_ik = w_i (exp(s_ik - Ls_i) - q_ik) / tau_s,  dxsn = dS wsn,  dwsn = dS^T xsn,  then the two normalisations backwards.
//
// Arithmetic: f32 throughout, every score ONE accumulation chain over d on v_mfma_f32_32x32x2_f32 (f32_tile.h): 1 / tau_t = 14 ... 25
// stands in front of the exponential ("Prototype cross-entropy (DINO)").
//   prologue  pc_rows_kernel (one wave per row, once per operand): the normalised, zero-padded operands xsn, xtn [mP][pP] and wsn, wtn
//             [KP][pP] (mP, KP up to 128, pP up to 32), the inverse norms, the clamp flags of the rows and the zero flags of the
//             prototypes.  batch_center is linear: pc_colmean_kernel (f64 column mean of xtn, fixed order) and pc_center_kernel
//             (one wave per prototype, f64).
//   forward   pc_fwd_kernel, one workgroup per (128 paired rows on the B side, prototype split): for each prototype tile of the split
//             two f32t_products on the same LDS stages, wsn_tile . xsn_rows^T then wtn_tile . xtn_rows^T, so that s_ik and t_ik sit on
//             the same (lane, element); per lane and B row five running numbers (max_s, sum_s), (max_t, sum_t) and
//             a = sum_k exp(t_ik - max_t) s_ik.  The four lanes of a row meet in LDS in a fixed order; pc_combine_kernel merges the
//             splits in ascending order (l_i = Ls_i - a_i / sum_t,i), pc_stats_kernel sums the rows in f64.  No [m][K] array exists.
//   backward  in blocks of KB prototypes: pc_ds_kernel recomputes both products and writes dS [mP][KB] and its transpose [KB][mP];
//             pc_dw_kernel is dwsn [KB][pP] = dS^T . xsn (the contraction over mP is complete within the block) and pc_dvrow_kernel
//             its normalisation backward; pc_dx_kernel is dS . wsn[block] in slices of the block's prototypes (few output tiles, a
//             long contraction) and pc_dxsum_kernel adds the slices in ascending order into dxsn (the first block assigns, the later
//             launches add, in ascending block order on the one stream); pc_dxrow_kernel ends with the normalisation backward of xs.
// Padding prototypes and rows are excluded by INDEX, never by value.  No atomics: the same bits on every run.  Nothing in the
// workspace survives a call.
#include "f32_tile.h"
#include "proto_ce.h"

#include <math.h>

namespace bvc {
namespace {

constexpr int kPcCUs = 256;         // CUs of the MI355X, the number ntxent.hip (kNxCUs) and its split heuristic use: keep the two in step
constexpr float kPcLog2e = 1.4426950408889634f;
constexpr int kPcPart = 8;           // floats per (split, row): max_s, sum_s, max_t, sum_t, a, 3 unused

__device__ __forceinline__ float pc_exp(float x) { return exp2f(x * kPcLog2e); }

// ---------------------------------------------------------------- prologue
struct PcRowArgs {
    const float* x; int64_t ldx;
    int n, nP, p, pP;
    int proto;                   // 0: feature rows (norm clamped at eps, flag = the clamp is NOT active), 1: prototypes (flag = zero row)
    float eps;
    float* inv; int32_t* flag; float* xn;
    // backward, feature rows of the student only (lse_s == nullptr otherwise)
    const float* lse_s; const float* lse_t; const float* row_weight;
    float* rLs; float* rLt; float* rw;
};

__global__ __launch_bounds__(256) void pc_rows_kernel(PcRowArgs a) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.nP) return;
    float* z = a.xn + (int64_t)row * a.pP;
    if (row >= a.n) {
        for (int d = lane; d < a.pP; d += 64) z[d] = 0.f;
        if (lane == 0) {
            a.inv[row] = 0.f; a.flag[row] = 0;
            if (a.lse_s) { a.rLs[row] = 0.f; a.rLt[row] = 0.f; a.rw[row] = 0.f; }
        }
        return;
    }
    const float* x = a.x + (int64_t)row * a.ldx;
    float ss = 0.f;
    for (int d = lane; d < a.p; d += 64) ss = fmaf(x[d], x[d], ss);
    ss = wave_sum(ss);
    const float nrm = sqrtf(ss);
    const bool zero = a.proto && nrm == 0.f;      // a NaN norm is not a zero row: it propagates into every score of the prototype
    const float den = a.proto ? nrm : fmaxf(nrm, a.eps);
    for (int d = lane; d < a.pP; d += 64) z[d] = (d < a.p && !zero) ? x[d] / den : 0.f;
    if (lane == 0) {
        a.inv[row] = zero ? 0.f : 1.0f / den;
        a.flag[row] = a.proto ? (int32_t)zero : (int32_t)(nrm > a.eps);
        if (a.lse_s) { a.rLs[row] = a.lse_s[row]; a.rLt[row] = a.lse_t[row]; a.rw[row] = a.row_weight[row]; }
    }
}

// out [C][R] = in [R][C]^T, 32 x 32 tiles (both sizes are multiples of 32); blockIdx.x walks R, blockIdx.y walks C
__global__ __launch_bounds__(256) void pc_transpose_kernel(const float* __restrict__ in, float* __restrict__ out, int R, int C) {
    __shared__ float t[32][33];
    const int x = threadIdx.x & 31, y = threadIdx.x >> 5;
    const int i0 = blockIdx.x * 32, d0 = blockIdx.y * 32;
#pragma unroll
    for (int k = 0; k < 4; ++k) t[y + 8 * k][x] = in[(int64_t)(i0 + y + 8 * k) * C + d0 + x];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) out[(int64_t)(d0 + y + 8 * k) * R + i0 + x] = t[x][y + 8 * k];
}

// xbar [pP] (f64) = the column mean of xtn over the m rows: row group y sums rows y, y + 8, .. in ascending order, the eight groups
// are added in ascending order
__global__ __launch_bounds__(256) void pc_colmean_kernel(const float* __restrict__ xtn, int m, int pP, double* __restrict__ xbar) {
    __shared__ double part[8][32];
    const int x = threadIdx.x & 31, y = threadIdx.x >> 5;
    const int col = blockIdx.x * 32 + x;
    double acc = 0.0;
    for (int i = y; i < m; i += 8) acc += (double)xtn[(int64_t)i * pP + col];
    part[y][x] = acc;
    __syncthreads();
    if (y == 0) {
        double tot = 0.0;
#pragma unroll
        for (int g = 0; g < 8; ++g) tot += part[g][x];
        xbar[col] = tot / (double)m;
    }
}

// bc_k = wtn_k . xbar, one wave per prototype, f64
__global__ __launch_bounds__(256) void pc_center_kernel(const float* __restrict__ wtn, const double* __restrict__ xbar, int K, int pP,
                                                        float* __restrict__ bc) {
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= K) return;
    const float* w = wtn + (int64_t)k * pP;
    double acc = 0.0;
    for (int d = lane; d < pP; d += 64) acc += (double)w[d] * xbar[d];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if (lane == 0) bc[k] = (float)acc;
}

// ---------------------------------------------------------------- forward
struct PcFwdArgs {
    const float* xsn; const float* xtn; const float* wsn; const float* wtn; const float* center;
    float* part;                 // [splits][mP][kPcPart]
    int m, mP, K, KP, pP, splits;
    float its, itt;              // 1 / tau_s, 1 / tau_t
};

__global__ __launch_bounds__(256) void pc_fwd_kernel(PcFwdArgs a) {
    __shared__ __attribute__((aligned(16))) float ldsA[kF32Tile * kF32Row];
    __shared__ __attribute__((aligned(16))) float ldsB[kF32Tile * kF32Row];
    __shared__ float cen[2][kF32Tile];
    __shared__ float red[4][kF32Tile][5];
    const int tid = threadIdx.x;
    const F32TileLane L = f32t_lane(tid);
    const int rtiles = a.mP / kF32Tile, tiles = a.KP / kF32Tile;
    const int rt = blockIdx.x % rtiles, split = blockIdx.x / rtiles;
    const int q0 = rt * kF32Tile;
    const int t_begin = (int)((int64_t)tiles * split / a.splits), t_end = (int)((int64_t)tiles * (split + 1) / a.splits);

    int ql[2];
    float ms[2], ls[2], mt[2], lt[2], av[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        ql[j] = F32T_BROW(L, 0, j);
        ms[j] = -INFINITY; ls[j] = 0.f; mt[j] = -INFINITY; lt[j] = 0.f; av[j] = 0.f;
    }

    for (int t = t_begin; t < t_end; ++t) {
        const int k0 = t * kF32Tile;
        // read after the K loops' barriers; two images by parity: the next tile's write cannot meet this tile's readers
        float* const cent = cen[(t - t_begin) & 1];
        if (tid < kF32Tile) cent[tid] = (a.center && k0 + tid < a.K) ? a.center[k0 + tid] : 0.f;
        f32x16 accS[2][2], accT[2][2];
        f32t_product(a.wsn, a.pP, k0, a.KP, a.xsn, a.pP, q0, a.mP, a.pP, ldsA, ldsB, tid, accS);
        f32t_product(a.wtn, a.pP, k0, a.KP, a.xtn, a.pP, q0, a.mP, a.pP, ldsA, ldsB, tid, accT);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float xs = -INFINITY, xt = -INFINITY;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int kl = F32T_AROW(L, 0, i, e);
                    const float s = accS[i][j][e] * a.its;
                    const float tt = (accT[i][j][e] - cent[kl]) * a.itt;
                    accS[i][j][e] = s;
                    accT[i][j][e] = tt;
                    if (k0 + kl < a.K) { xs = fmaxf(xs, s); xt = fmaxf(xt, tt); }
                }
            const float ns = fmaxf(ms[j], xs), nt = fmaxf(mt[j], xt);
            const float as = ms[j] == -INFINITY ? 0.f : pc_exp(ms[j] - ns);
            const float at = mt[j] == -INFINITY ? 0.f : pc_exp(mt[j] - nt);
            float sum_s = 0.f, sum_t = 0.f, sum_a = 0.f;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const bool ok = F32T_AROW(L, k0, i, e) < a.K;
                    const float s = accS[i][j][e];
                    const float es = ok ? pc_exp(s - ns) : 0.f;
                    const float et = ok ? pc_exp(accT[i][j][e] - nt) : 0.f;
                    sum_s += es;
                    sum_t += et;
                    sum_a = fmaf(et, s, sum_a);
                }
            ls[j] = fmaf(ls[j], as, sum_s);
            lt[j] = fmaf(lt[j], at, sum_t);
            av[j] = fmaf(av[j], at, sum_a);
            ms[j] = ns;
            mt[j] = nt;
        }
    }

    // the four lanes of a row (wk, h), merged in that order
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        float* o = red[L.wk * 2 + L.h][ql[j]];
        o[0] = ms[j]; o[1] = ls[j]; o[2] = mt[j]; o[3] = lt[j]; o[4] = av[j];
    }
    __syncthreads();
    if (tid < kF32Tile) {
        float Ms = -INFINITY, Mt = -INFINITY;
#pragma unroll
        for (int s = 0; s < 4; ++s) { Ms = fmaxf(Ms, red[s][tid][0]); Mt = fmaxf(Mt, red[s][tid][2]); }
        float Ls = 0.f, Lt = 0.f, A = 0.f;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const float m1 = red[s][tid][0], m2 = red[s][tid][2];
            const float w1 = m1 == -INFINITY ? 0.f : pc_exp(m1 - Ms);
            const float w2 = m2 == -INFINITY ? 0.f : pc_exp(m2 - Mt);
            Ls = fmaf(w1, red[s][tid][1], Ls);
            Lt = fmaf(w2, red[s][tid][3], Lt);
            A = fmaf(w2, red[s][tid][4], A);
        }
        float* o = a.part + ((int64_t)split * a.mP + q0 + tid) * kPcPart;
        o[0] = Ms; o[1] = Ls; o[2] = Mt; o[3] = Lt; o[4] = A;
    }
}

// splits merged in ascending order: Ls = Ms + log sum_s, Lt = Mt + log sum_t, l = Ls - a / sum_t
__global__ __launch_bounds__(256) void pc_combine_kernel(const float* __restrict__ part, int m, int mP, int splits, float* __restrict__ row_loss,
                                                         float* __restrict__ lse_s, float* __restrict__ lse_t) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    float Ms = -INFINITY, Mt = -INFINITY;
    for (int s = 0; s < splits; ++s) {
        const float* e = part + ((int64_t)s * mP + i) * kPcPart;
        Ms = fmaxf(Ms, e[0]);
        Mt = fmaxf(Mt, e[2]);
    }
    float Ls = 0.f, Lt = 0.f, A = 0.f;
    for (int s = 0; s < splits; ++s) {
        const float* e = part + ((int64_t)s * mP + i) * kPcPart;
        const float w1 = e[0] == -INFINITY ? 0.f : pc_exp(e[0] - Ms);
        const float w2 = e[2] == -INFINITY ? 0.f : pc_exp(e[2] - Mt);
        Ls = fmaf(w1, e[1], Ls);
        Lt = fmaf(w2, e[3], Lt);
        A = fmaf(w2, e[4], A);
    }
    const float D = Ms + logf(Ls);
    lse_s[i] = D;
    lse_t[i] = Mt + logf(Lt);
    row_loss[i] = D - A / Lt;
}

// stats = {sum l_i / m, the number of zero prototype rows of vs and of vt}: thread t sums rows t, t + 256, .. in f64, then a fixed tree
__global__ __launch_bounds__(256) void pc_stats_kernel(const float* __restrict__ row_loss, int m, const int32_t* __restrict__ zero_s,
                                                       const int32_t* __restrict__ zero_t, int K, float* __restrict__ stats2) {
    __shared__ double sl[256];
    __shared__ int sz[256];
    double acc = 0.0;
    int cnt = 0;
    for (int i = threadIdx.x; i < m; i += 256) acc += (double)row_loss[i];
    for (int k = threadIdx.x; k < K; k += 256) cnt += zero_s[k] + zero_t[k];
    sl[threadIdx.x] = acc;
    sz[threadIdx.x] = cnt;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) { sl[threadIdx.x] += sl[threadIdx.x + o]; sz[threadIdx.x] += sz[threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        stats2[0] = (float)(sl[0] / (double)m);
        stats2[1] = (float)sz[0];
    }
}

// ---------------------------------------------------------------- backward
struct PcBwdArgs {
    const float* xsn; const float* xtn; const float* wsn; const float* wtn; const float* center;
    const float* xsnT;           // [pP][mP]
    float* wsnT;                 // [pP][kb]: the block's rows of wsn, transposed
    const float* rLs; const float* rLt; const float* rw;
    const float* inv_x; const int32_t* live_x; const float* inv_w;
    float* dS;                   // [mP][ldS], kb columns used
    float* dST;                  // [kb][mP]
    float* dwsn;                 // [kb][pP]
    float* dxsn;                 // [mP][pP]
    float* dxp;                  // [kparts][mP][pP]: the block's partial products of dxsn, one per slice of its prototypes
    int kslice, kparts;          // prototypes per slice (a multiple of 128), slices of this block
    float* dxs; int64_t lddxs; float* dvs; int64_t lddvs;
    int m, mP, K, KP, p, pP, ldS, kblk0, kb, first;      // this block: prototypes kblk0 .. kblk0 + kb (kb a multiple of 128)
    float its, itt, eps;
};

// dS [i][k - kblk0] = w_i (exp(s_ik - Ls_i) - exp(t_ik - Lt_i)) / tau_s and the same transposed; 0 for k >= K and i >= m
__global__ __launch_bounds__(256) void pc_ds_kernel(PcBwdArgs a) {
    __shared__ __attribute__((aligned(16))) float ldsA[kF32Tile * kF32Row];
    __shared__ __attribute__((aligned(16))) float ldsB[kF32Tile * kF32Row];
    __shared__ float cent[kF32Tile];
    const int tid = threadIdx.x;
    const F32TileLane L = f32t_lane(tid);
    const int ptiles = a.kb / kF32Tile;
    const int pt = blockIdx.x % ptiles, rt = blockIdx.x / ptiles;
    const int kl0 = pt * kF32Tile, k0 = a.kblk0 + kl0, q0 = rt * kF32Tile;
    if (tid < kF32Tile) cent[tid] = (a.center && k0 + tid < a.K) ? a.center[k0 + tid] : 0.f;      // read after the K loops' barriers
    f32x16 accS[2][2], accT[2][2];
    f32t_product(a.wsn, a.pP, k0, a.KP, a.xsn, a.pP, q0, a.mP, a.pP, ldsA, ldsB, tid, accS);
    f32t_product(a.wtn, a.pP, k0, a.KP, a.xtn, a.pP, q0, a.mP, a.pP, ldsA, ldsB, tid, accT);
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int irow = F32T_BROW(L, q0, j);
        const float Ls = a.rLs[irow], Lt = a.rLt[irow], w = a.rw[irow];
        const bool rok = irow < a.m;
        float* const srow = a.dS + (int64_t)irow * a.ldS;
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                f32x4 v;
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const int e = 4 * q + c;
                    const int kl = F32T_AROW(L, 0, i, e);
                    const float s = accS[i][j][e] * a.its;
                    const float tt = (accT[i][j][e] - cent[kl]) * a.itt;
                    const float g = w * (pc_exp(s - Ls) - pc_exp(tt - Lt)) * a.its;
                    const float val = (rok && k0 + kl < a.K) ? g : 0.f;
                    a.dST[(int64_t)(kl0 + kl) * a.mP + irow] = val;
                    v[c] = val;
                }
                // elements 4 q .. 4 q + 3 are four consecutive prototypes
                *reinterpret_cast<f32x4*>(srow + kl0 + F32T_AROW(L, 0, i, 4 * q)) = v;
            }
    }
}

// dwsn [k - kblk0][c] = sum_i dST [k - kblk0][i] xsnT [c][i]
__global__ __launch_bounds__(256) void pc_dw_kernel(PcBwdArgs a) {
    __shared__ __attribute__((aligned(16))) float ldsA[kF32Tile * kF32Row];
    __shared__ __attribute__((aligned(16))) float ldsB[kF32Tile * kF32Row];
    const int tid = threadIdx.x;
    const F32TileLane L = f32t_lane(tid);
    const int ctiles = (a.pP + kF32Tile - 1) / kF32Tile;
    const int ct = blockIdx.x % ctiles, pt = blockIdx.x / ctiles;
    f32x16 acc[2][2];
    f32t_product(a.dST, a.mP, pt * kF32Tile, a.kb, a.xsnT, a.mP, ct * kF32Tile, a.pP, a.mP, ldsA, ldsB, tid, acc);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int kl = F32T_AROW(L, pt * kF32Tile, i, e);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int c = F32T_BROW(L, ct * kF32Tile, j);
                if (c < a.pP) a.dwsn[(int64_t)kl * a.pP + c] = acc[i][j][e];
            }
        }
}

// dxp [part][i][c] = sum over the part's slice of k of dS [i][k - kblk0] wsnT [c][k - kblk0].  The product has only
// (mP / 128) x (pP / 128) output tiles and a contraction of up to the whole K: the slices are what fills the chip.
__global__ __launch_bounds__(256) void pc_dx_kernel(PcBwdArgs a) {
    __shared__ __attribute__((aligned(16))) float ldsA[kF32Tile * kF32Row];
    __shared__ __attribute__((aligned(16))) float ldsB[kF32Tile * kF32Row];
    const int tid = threadIdx.x;
    const F32TileLane L = f32t_lane(tid);
    const int ctiles = (a.pP + kF32Tile - 1) / kF32Tile, rtiles = a.mP / kF32Tile;
    const int ct = blockIdx.x % ctiles, rt = blockIdx.x / ctiles % rtiles, part = blockIdx.x / (ctiles * rtiles);
    const int kb0 = part * a.kslice;
    const int klen = a.kb - kb0 < a.kslice ? a.kb - kb0 : a.kslice;
    f32x16 acc[2][2];
    f32t_product(a.dS + kb0, a.ldS, rt * kF32Tile, a.mP, a.wsnT + kb0, a.kb, ct * kF32Tile, a.pP, klen, ldsA, ldsB, tid, acc);
    float* const out = a.dxp + (int64_t)part * a.mP * a.pP;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int il = F32T_AROW(L, rt * kF32Tile, i, e);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int c = F32T_BROW(L, ct * kF32Tile, j);
                if (c < a.pP) out[(int64_t)il * a.pP + c] = acc[i][j][e];
            }
        }
}

// dxsn (+)= the block's parts, added in ascending order: the first block assigns, the later launches add in ascending block order
__global__ __launch_bounds__(256) void pc_dxsum_kernel(PcBwdArgs a) {
    const int64_t n = (int64_t)a.mP * a.pP;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float sum = a.dxp[i];
    for (int part = 1; part < a.kparts; ++part) sum += a.dxp[(int64_t)part * n + i];
    a.dxsn[i] = a.first ? sum : a.dxsn[i] + sum;
}

// dvs_k = (dwsn_k - wsn_k (wsn_k . dwsn_k)) / |vs_k|, 0 for a zero row (inv = 0); one wave per prototype of the block
__global__ __launch_bounds__(256) void pc_dvrow_kernel(PcBwdArgs a) {
    const int lane = threadIdx.x & 63;
    const int kl = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int k = a.kblk0 + kl;
    if (kl >= a.kb || k >= a.K) return;
    const float* z = a.wsn + (int64_t)k * a.pP;
    const float* g = a.dwsn + (int64_t)kl * a.pP;
    float* out = a.dvs + (int64_t)k * a.lddvs;
    const float inv = a.inv_w[k];
    if (inv == 0.f) {
        for (int d = lane; d < a.p; d += 64) out[d] = 0.f;
        return;
    }
    float dot = 0.f;
    for (int d = lane; d < a.p; d += 64) dot = fmaf(z[d], g[d], dot);
    dot = wave_sum(dot);
    for (int d = lane; d < a.p; d += 64) out[d] = inv * (g[d] - z[d] * dot);
}

// dxs_i = inv_i (dxsn_i - xsn_i (xsn_i . dxsn_i)), or dxsn_i / eps where the norm was clamped; one wave per row
__global__ __launch_bounds__(256) void pc_dxrow_kernel(PcBwdArgs a) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.m) return;
    const float* z = a.xsn + (int64_t)row * a.pP;
    const float* g = a.dxsn + (int64_t)row * a.pP;
    float* out = a.dxs + (int64_t)row * a.lddxs;
    if (a.live_x[row]) {
        float dot = 0.f;
        for (int d = lane; d < a.p; d += 64) dot = fmaf(z[d], g[d], dot);
        dot = wave_sum(dot);
        const float inv = a.inv_x[row];
        for (int d = lane; d < a.p; d += 64) out[d] = inv * (g[d] - z[d] * dot);
    } else {
        for (int d = lane; d < a.p; d += 64) out[d] = g[d] / a.eps;
    }
}

// ---------------------------------------------------------------- host side
int pc_up(int n, int q) { return (n + q - 1) / q * q; }

int pc_check_shape(const char* who, int m, int K, int p, int splits, int block) {
    BVC_REQUIRE(m >= 1 && m <= kPcMaxM, "%s: m %d outside 1 .. %d", who, m, kPcMaxM);
    BVC_REQUIRE(K >= 1 && K <= kPcMaxK, "%s: K %d outside 1 .. %d", who, K, kPcMaxK);
    BVC_REQUIRE(p >= 1 && p <= kPcMaxP, "%s: p %d outside 1 .. %d", who, p, kPcMaxP);
    BVC_REQUIRE(splits >= 0 && splits <= kPcMaxSplits, "%s: splits %d outside 0 .. %d", who, splits, kPcMaxSplits);
    BVC_REQUIRE(block >= 0, "%s: negative block %d", who, block);
    return BVC_OK;
}

int pc_check_args(const char* who, const float* xs, int64_t ldxs, const float* vs, int64_t ldvs, const float* xt, int64_t ldxt,
                  const float* vt, int64_t ldvt, const float* center, int p, float tau_s, float tau_t, float eps, const void* workspace) {
    BVC_REQUIRE(xs && vs && xt && vt && workspace, "%s: null argument", who);
    BVC_REQUIRE(ldxs >= p && ldvs >= p && ldxt >= p && ldvt >= p, "%s: a row stride (%lld, %lld, %lld, %lld) is below p %d", who,
                (long long)ldxs, (long long)ldvs, (long long)ldxt, (long long)ldvt, p);
    BVC_REQUIRE(isfinite(tau_s) && tau_s > 0.f, "%s: tau_s %g is not a positive finite number", who, (double)tau_s);
    BVC_REQUIRE(isfinite(tau_t) && tau_t > 0.f, "%s: tau_t %g is not a positive finite number", who, (double)tau_t);
    BVC_REQUIRE(isfinite(eps) && eps > 0.f, "%s: eps %g is not a positive finite number", who, (double)eps);
    BVC_REQUIRE((((uintptr_t)xs | (uintptr_t)vs | (uintptr_t)xt | (uintptr_t)vt | (uintptr_t)center) & 3) == 0 &&
                    ((uintptr_t)workspace & 15) == 0,
                "%s: the operands must be 4-byte, the workspace 16-byte aligned", who);
    return BVC_OK;
}

// about two workgroups per CU, every split at least one prototype tile, at most 512
int pc_auto_splits(int m, int K) {
    const int rtiles = pc_up(m, kF32Tile) / kF32Tile, tiles = pc_up(K, kF32Tile) / kF32Tile;
    int s = (2 * kPcCUs + rtiles - 1) / rtiles;
    if (s > tiles) s = tiles;
    if (s > 512) s = 512;
    return s < 1 ? 1 : s;
}

// whole prototype tiles under the cap of a dS block, at least one tile, at most all prototypes
int pc_auto_block(int m, int K) {
    const int mP = pc_up(m, kF32Tile), KP = pc_up(K, kF32Tile);
    int64_t b = kPcDsBlockBytes / ((int64_t)mP * 4) / kF32Tile * kF32Tile;
    if (b < kF32Tile) b = kF32Tile;
    if (b > KP) b = KP;
    return (int)b;
}
int pc_resolve_block(int m, int K, int block) {
    if (block <= 0) return pc_auto_block(m, K);
    const int KP = pc_up(K, kF32Tile);
    const int64_t b = ((int64_t)block + kF32Tile - 1) / kF32Tile * kF32Tile;
    return (int)(b > KP ? KP : b);
}

// slices of a block's prototypes for dxsn: about two workgroups per CU over the (row tile, column tile, slice) grid, whole tiles
int pc_dx_max_parts(int mP, int pP, int kb) {
    const int out_tiles = mP / kF32Tile * ((pP + kF32Tile - 1) / kF32Tile);
    int parts = (2 * kPcCUs + out_tiles - 1) / out_tiles;
    const int tiles = kb / kF32Tile;
    if (parts > tiles) parts = tiles;
    return parts < 1 ? 1 : parts;
}
int pc_dx_slice(int mP, int pP, int kb) {
    const int tiles = kb / kF32Tile, parts = pc_dx_max_parts(mP, pP, kb);
    return (tiles + parts - 1) / parts * kF32Tile;      // ceil(kb / slice) <= parts
}

struct PcLayout {
    int mP, KP, pP, splits, KB;
    int64_t inv_xs, live_xs, inv_xt, live_xt, rLs, rLt, rw, inv_ws, zero_s, inv_wt, zero_t, xbar, part, xsn, xtn, wsn, wtn, xsnT, wsnT, dS,
        dST, dwsn, dxsn, dxp, total;
};
PcLayout pc_layout(int m, int K, int p, int splits, int block) {
    PcLayout w;
    w.mP = pc_up(m, kF32Tile); w.KP = pc_up(K, kF32Tile); w.pP = pc_up(p, kF32KStep);
    w.splits = splits > 0 ? splits : pc_auto_splits(m, K);
    w.KB = pc_resolve_block(m, K, block);
    int64_t o = 0;
    const int64_t mv = ws_align((int64_t)w.mP * 4), kv = ws_align((int64_t)w.KP * 4);
    const int64_t xmat = ws_align((int64_t)w.mP * w.pP * 4), wmat = ws_align((int64_t)w.KP * w.pP * 4);
    const int64_t bmat = ws_align((int64_t)w.KB * w.pP * 4), dsb = ws_align((int64_t)w.mP * w.KB * 4);
    w.inv_xs = o; o += mv; w.live_xs = o; o += mv; w.inv_xt = o; o += mv; w.live_xt = o; o += mv;
    w.rLs = o; o += mv; w.rLt = o; o += mv; w.rw = o; o += mv;
    w.inv_ws = o; o += kv; w.zero_s = o; o += kv; w.inv_wt = o; o += kv; w.zero_t = o; o += kv;
    w.xbar = o; o += ws_align((int64_t)w.pP * 8);
    w.part = o; o += ws_align((int64_t)w.splits * w.mP * kPcPart * 4);
    w.xsn = o; o += xmat; w.xtn = o; o += xmat; w.wsn = o; o += wmat; w.wtn = o; o += wmat;
    w.xsnT = o; o += xmat; w.wsnT = o; o += bmat;
    w.dS = o; o += dsb; w.dST = o; o += dsb;
    w.dwsn = o; o += bmat; w.dxsn = o; o += xmat;
    w.dxp = o; o += (int64_t)pc_dx_max_parts(w.mP, w.pP, w.KB) * xmat;      // no block has more parts than a whole one may
    w.total = o;
    return w;
}

struct PcOperands { const float* xs; int64_t ldxs; const float* vs; int64_t ldvs; const float* xt; int64_t ldxt; const float* vt; int64_t ldvt; };

// the four normalised operands; lse_s != nullptr also copies the backward's per-row vectors
int pc_prologue(const PcLayout& w, const PcOperands& in, int m, int K, int p, float eps, const float* lse_s, const float* lse_t,
                const float* row_weight, void* ws, hipStream_t s) {
    PcRowArgs r{};
    r.p = p; r.pP = w.pP; r.eps = eps;
    r.x = in.xs; r.ldx = in.ldxs; r.n = m; r.nP = w.mP; r.proto = 0;
    r.inv = ws_at<float>(ws, w.inv_xs); r.flag = ws_at<int32_t>(ws, w.live_xs); r.xn = ws_at<float>(ws, w.xsn);
    r.lse_s = lse_s; r.lse_t = lse_t; r.row_weight = row_weight;
    r.rLs = ws_at<float>(ws, w.rLs); r.rLt = ws_at<float>(ws, w.rLt); r.rw = ws_at<float>(ws, w.rw);
    pc_rows_kernel<<<dim3((unsigned)(w.mP / 4)), dim3(256), 0, s>>>(r);
    r.lse_s = nullptr; r.lse_t = nullptr; r.row_weight = nullptr;
    r.x = in.xt; r.ldx = in.ldxt;
    r.inv = ws_at<float>(ws, w.inv_xt); r.flag = ws_at<int32_t>(ws, w.live_xt); r.xn = ws_at<float>(ws, w.xtn);
    pc_rows_kernel<<<dim3((unsigned)(w.mP / 4)), dim3(256), 0, s>>>(r);
    r.n = K; r.nP = w.KP; r.proto = 1;
    r.x = in.vs; r.ldx = in.ldvs;
    r.inv = ws_at<float>(ws, w.inv_ws); r.flag = ws_at<int32_t>(ws, w.zero_s); r.xn = ws_at<float>(ws, w.wsn);
    pc_rows_kernel<<<dim3((unsigned)(w.KP / 4)), dim3(256), 0, s>>>(r);
    r.x = in.vt; r.ldx = in.ldvt;
    r.inv = ws_at<float>(ws, w.inv_wt); r.flag = ws_at<int32_t>(ws, w.zero_t); r.xn = ws_at<float>(ws, w.wtn);
    pc_rows_kernel<<<dim3((unsigned)(w.KP / 4)), dim3(256), 0, s>>>(r);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

}  // namespace

int proto_ce_splits(int m, int K, int p) {
    if (pc_check_shape("op_proto_ce_splits", m, K, p, 0, 0) != BVC_OK) return -1;
    return pc_auto_splits(m, K);
}

int proto_ce_block(int m, int K, int p) {
    if (pc_check_shape("op_proto_ce_block", m, K, p, 0, 0) != BVC_OK) return -1;
    return pc_auto_block(m, K);
}

int64_t proto_ce_workspace(int m, int K, int p, int splits, int block) {
    if (pc_check_shape("op_proto_ce_workspace", m, K, p, splits, block) != BVC_OK) return -1;
    return pc_layout(m, K, p, splits, block).total;
}

int launch_proto_ce_fwd(const float* xs, int64_t ldxs, const float* vs, int64_t ldvs, const float* xt, int64_t ldxt, const float* vt,
                        int64_t ldvt, const float* center, int m, int K, int p, float tau_s, float tau_t, float eps, int splits,
                        float* row_loss, float* lse_s, float* lse_t, float* stats2, float* batch_center, void* workspace, hipStream_t s) {
    if (int rc = pc_check_shape("op_proto_ce_fwd", m, K, p, splits, 0)) return rc;
    if (int rc = pc_check_args("op_proto_ce_fwd", xs, ldxs, vs, ldvs, xt, ldxt, vt, ldvt, center, p, tau_s, tau_t, eps, workspace)) return rc;
    BVC_REQUIRE(row_loss && lse_s && lse_t && stats2, "op_proto_ce_fwd: null argument");
    const PcLayout w = pc_layout(m, K, p, splits, 0);
    const PcOperands in{xs, ldxs, vs, ldvs, xt, ldxt, vt, ldvt};
    if (int rc = pc_prologue(w, in, m, K, p, eps, nullptr, nullptr, nullptr, workspace, s)) return rc;
    PcFwdArgs a{};
    a.xsn = ws_at<float>(workspace, w.xsn); a.xtn = ws_at<float>(workspace, w.xtn);
    a.wsn = ws_at<float>(workspace, w.wsn); a.wtn = ws_at<float>(workspace, w.wtn);
    a.center = center; a.part = ws_at<float>(workspace, w.part);
    a.m = m; a.mP = w.mP; a.K = K; a.KP = w.KP; a.pP = w.pP; a.splits = w.splits;
    a.its = 1.0f / tau_s; a.itt = 1.0f / tau_t;
    pc_fwd_kernel<<<dim3((unsigned)(w.mP / kF32Tile * w.splits)), dim3(256), 0, s>>>(a);
    BVC_CHECK_HIP(hipGetLastError());
    pc_combine_kernel<<<dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s>>>(a.part, m, w.mP, w.splits, row_loss, lse_s, lse_t);
    pc_stats_kernel<<<dim3(1), dim3(256), 0, s>>>(row_loss, m, ws_at<int32_t>(workspace, w.zero_s), ws_at<int32_t>(workspace, w.zero_t), K, stats2);
    if (batch_center) {
        double* xbar = ws_at<double>(workspace, w.xbar);
        pc_colmean_kernel<<<dim3((unsigned)(w.pP / 32)), dim3(256), 0, s>>>(a.xtn, m, w.pP, xbar);
        pc_center_kernel<<<dim3((unsigned)((K + 3) / 4)), dim3(256), 0, s>>>(a.wtn, xbar, K, w.pP, batch_center);
    }
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

int launch_proto_ce_bwd(const float* xs, int64_t ldxs, const float* vs, int64_t ldvs, const float* xt, int64_t ldxt, const float* vt,
                        int64_t ldvt, const float* center, int m, int K, int p, float tau_s, float tau_t, float eps, const float* lse_s,
                        const float* lse_t, const float* row_weight, int splits, int block, float* dxs, int64_t lddxs, float* dvs,
                        int64_t lddvs, void* workspace, hipStream_t s) {
    if (int rc = pc_check_shape("op_proto_ce_bwd", m, K, p, splits, block)) return rc;
    if (int rc = pc_check_args("op_proto_ce_bwd", xs, ldxs, vs, ldvs, xt, ldxt, vt, ldvt, center, p, tau_s, tau_t, eps, workspace)) return rc;
    BVC_REQUIRE(lse_s && lse_t && row_weight && dxs && dvs, "op_proto_ce_bwd: null argument");
    BVC_REQUIRE(lddxs >= p && lddvs >= p, "op_proto_ce_bwd: a row stride of the gradients (%lld, %lld) is below p %d", (long long)lddxs,
                (long long)lddvs, p);
    const PcLayout w = pc_layout(m, K, p, splits, block);
    const PcOperands in{xs, ldxs, vs, ldvs, xt, ldxt, vt, ldvt};
    if (int rc = pc_prologue(w, in, m, K, p, eps, lse_s, lse_t, row_weight, workspace, s)) return rc;
    PcBwdArgs a{};
    a.xsn = ws_at<float>(workspace, w.xsn); a.xtn = ws_at<float>(workspace, w.xtn);
    a.wsn = ws_at<float>(workspace, w.wsn); a.wtn = ws_at<float>(workspace, w.wtn);
    a.center = center;
    float* xsnT = ws_at<float>(workspace, w.xsnT);
    a.xsnT = xsnT; a.wsnT = ws_at<float>(workspace, w.wsnT);
    a.rLs = ws_at<float>(workspace, w.rLs); a.rLt = ws_at<float>(workspace, w.rLt); a.rw = ws_at<float>(workspace, w.rw);
    a.inv_x = ws_at<float>(workspace, w.inv_xs); a.live_x = ws_at<int32_t>(workspace, w.live_xs); a.inv_w = ws_at<float>(workspace, w.inv_ws);
    a.dS = ws_at<float>(workspace, w.dS); a.dST = ws_at<float>(workspace, w.dST);
    a.dwsn = ws_at<float>(workspace, w.dwsn); a.dxsn = ws_at<float>(workspace, w.dxsn);
    a.dxp = ws_at<float>(workspace, w.dxp);
    a.dxs = dxs; a.lddxs = lddxs; a.dvs = dvs; a.lddvs = lddvs;
    a.m = m; a.mP = w.mP; a.K = K; a.KP = w.KP; a.p = p; a.pP = w.pP; a.ldS = w.KB;
    a.its = 1.0f / tau_s; a.itt = 1.0f / tau_t; a.eps = eps;
    pc_transpose_kernel<<<dim3((unsigned)(w.mP / 32), (unsigned)(w.pP / 32)), dim3(256), 0, s>>>(a.xsn, xsnT, w.mP, w.pP);
    BVC_CHECK_HIP(hipGetLastError());
    const int rtiles = w.mP / kF32Tile, ctiles = (w.pP + kF32Tile - 1) / kF32Tile;
    for (int k0 = 0; k0 < w.KP; k0 += w.KB) {
        a.kblk0 = k0;
        a.kb = w.KP - k0 < w.KB ? w.KP - k0 : w.KB;
        a.first = k0 == 0;
        const int ptiles = a.kb / kF32Tile;
        pc_transpose_kernel<<<dim3((unsigned)(a.kb / 32), (unsigned)(w.pP / 32)), dim3(256), 0, s>>>(a.wsn + (int64_t)k0 * w.pP, a.wsnT, a.kb, w.pP);
        pc_ds_kernel<<<dim3((unsigned)(ptiles * rtiles)), dim3(256), 0, s>>>(a);
        pc_dw_kernel<<<dim3((unsigned)(ptiles * ctiles)), dim3(256), 0, s>>>(a);
        pc_dvrow_kernel<<<dim3((unsigned)(a.kb / 4)), dim3(256), 0, s>>>(a);
        // at most pc_dx_max_parts(kb) <= pc_dx_max_parts(KB) slices: what the layout reserved
        a.kslice = pc_dx_slice(w.mP, w.pP, a.kb);
        a.kparts = (a.kb + a.kslice - 1) / a.kslice;
        pc_dx_kernel<<<dim3((unsigned)(rtiles * ctiles * a.kparts)), dim3(256), 0, s>>>(a);
        pc_dxsum_kernel<<<dim3((unsigned)(((int64_t)w.mP * w.pP + 255) / 256)), dim3(256), 0, s>>>(a);
        BVC_CHECK_HIP(hipGetLastError());
    }
    pc_dxrow_kernel<<<dim3((unsigned)((m + 3) / 4)), dim3(256), 0, s>>>(a);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

}  // namespace bvc

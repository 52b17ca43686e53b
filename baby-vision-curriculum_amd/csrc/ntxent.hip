// NT-Xent / SupCon: a contrastive loss over n f32 feature rows f [n][p] with one integer group id per row (bvc_op_ntxent_fwd / _bwd).
//     zn_i = f_i / max(|f_i|, eps),   s_ij = zn_i . zn_j / T,   P(i) = { j != i : g_j == g_i >= 0 },   c_i = |P(i)|,
//     D_i = log sum_{k != i} exp(s_ik),   l_i = D_i - (1 / c_i) sum_{j in P(i)} s_ij  (0 when c_i = 0),   loss = sum l_i / max(1, #{c_i > 0}).
// Two views per sample give SimCLR's NT-Xent, label ids SupCon's L_out.  Backward, with per-row weights w_i (0 where c_i = 0):
//     G_ij = w_i (exp(s_ij - D_i) - [j in P(i)] / c_i),   E = G + G^T,   dzn = (1 / T) E zn,
//     df_i = inv_i (dzn_i - zn_i (zn_i . dzn_i))   (dzn_i / eps where the clamp of the norm is active).
//
// Arithmetic: f32 throughout.  Every score is ONE accumulation chain over d on v_mfma_f32_32x32x2_f32: with 1 / T = 10 ... 100 in
// front of the exponential, bf16 operands are three to four orders of magnitude worse ("NT-Xent").
//
// The three products are f32t_product of f32_tile.h, C [128][128] = A [128][K] . B [128][K]^T over padded operands in the workspace;
// the epilogues below take their rows (A side, on the accumulator elements) and columns (B side, on the lane) from its helpers.
//   prologue  nx_rows_kernel (one wave per row): inv, the clamp flag, zn [nP][pP] with zero tails (nP = n up to 128, pP = p up to
//             32), the group ids and, in the backward, the per-row vectors D, w, w / c; nx_transpose_kernel: znT [pP][nP].
//   forward   nx_fwd_kernel, one workgroup per (128 query rows, key split): A = key tile of zn, B = the query rows of zn.  After the K
//             loop of a key tile every lane updates, for its two query rows, a running (max, sum), the positive-score sum and the
//             positive count over its 32 keys of the tile; the four lanes of a row meet in LDS at the end, in a fixed order, and the
//             split's (max, sum, possum, count) goes to the workspace.  nx_combine_kernel merges the splits in ascending order,
//             nx_stats_kernel sums the row losses in a fixed order (f64).  No [n][n] array exists in the forward.
//   backward  in blocks of R rows: nx_e_kernel recomputes the scores of [R][n] and writes E (A = the block's rows, B = all rows: E is
//             symmetric, G_ji needs only row vectors of j), nx_dzn_kernel is E [R][nP] . znT [pP][nP]^T on the same loop, and
//             nx_dfrow_kernel is the normalisation backward of each row.
// Rows and keys are excluded by INDEX (j == i, j >= n), never by value.  No atomics: the same bits on every run.  Nothing in the
// workspace survives a call: the backward recomputes zn from f.
#include "f32_tile.h"
#include "ntxent.h"

#include <math.h>

namespace bvc {
namespace {

constexpr int kNxCUs = 256;
constexpr float kNxLog2e = 1.4426950408889634f;

__device__ __forceinline__ float nx_exp(float x) { return exp2f(x * kNxLog2e); }

// ---------------------------------------------------------------- prologue
struct NxRowArgs {
    const float* f; int64_t ldf;
    const int32_t* groups; int views;
    int n, nP, p, pP;
    float eps;
    float* inv; int32_t* live; int32_t* gid; float* zn;
    // backward only (lse == nullptr in the forward)
    const float* lse; const int32_t* npos; const float* row_weight;
    float* Dp; float* wv; float* wc;
};

__global__ __launch_bounds__(256) void nx_rows_kernel(NxRowArgs a) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.nP) return;
    float* z = a.zn + (int64_t)row * a.pP;
    if (row >= a.n) {
        for (int d = lane; d < a.pP; d += 64) z[d] = 0.f;
        if (lane == 0) {
            a.inv[row] = 0.f; a.live[row] = 0; a.gid[row] = -1;
            if (a.lse) { a.Dp[row] = 0.f; a.wv[row] = 0.f; a.wc[row] = 0.f; }
        }
        return;
    }
    const float* x = a.f + (int64_t)row * a.ldf;
    float ss = 0.f;
    for (int d = lane; d < a.p; d += 64) ss = fmaf(x[d], x[d], ss);
    ss = wave_sum(ss);
    const float nrm = sqrtf(ss), den = fmaxf(nrm, a.eps);
    for (int d = lane; d < a.pP; d += 64) z[d] = d < a.p ? x[d] / den : 0.f;
    if (lane == 0) {
        a.inv[row] = 1.0f / den;
        a.live[row] = nrm > a.eps;
        a.gid[row] = a.groups ? a.groups[row] : row % (a.n / a.views);
        if (a.lse) {
            const int c = a.npos[row];
            const float w = c > 0 ? a.row_weight[row] : 0.f, D = a.lse[row];
            a.Dp[row] = isfinite(D) ? D : 0.f;      // (n = 1: no other row, nothing reads it)
            a.wv[row] = w;
            a.wc[row] = c > 0 ? w / (float)c : 0.f;
        }
    }
}

// znT [pP][nP] = zn [nP][pP]^T, 32 x 32 tiles (both sizes are multiples of 32)
__global__ __launch_bounds__(256) void nx_transpose_kernel(const float* __restrict__ zn, float* __restrict__ znT, int nP, int pP) {
    __shared__ float t[32][33];
    const int x = threadIdx.x & 31, y = threadIdx.x >> 5;
    const int d0 = blockIdx.x * 32, i0 = blockIdx.y * 32;
#pragma unroll
    for (int k = 0; k < 4; ++k) t[y + 8 * k][x] = zn[(int64_t)(i0 + y + 8 * k) * pP + d0 + x];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) znT[(int64_t)(d0 + y + 8 * k) * nP + i0 + x] = t[x][y + 8 * k];
}

// ---------------------------------------------------------------- forward
struct NxFwdArgs {
    const float* zn; const int32_t* gid;
    float* part;                 // [splits][nP][4]: max, sum, positive-score sum, positive count
    int n, nP, pP, splits;
    float invT;
};

__global__ __launch_bounds__(256) void nx_fwd_kernel(NxFwdArgs a) {
    __shared__ __attribute__((aligned(16))) float ldsA[kF32Tile * kF32Row];
    __shared__ __attribute__((aligned(16))) float ldsB[kF32Tile * kF32Row];
    __shared__ int32_t kg[2][kF32Tile];
    __shared__ float red[4][kF32Tile][4];
    const int tid = threadIdx.x;
    const F32TileLane L = f32t_lane(tid);
    const int tiles = a.nP / kF32Tile;
    const int qt = blockIdx.x % tiles, split = blockIdx.x / tiles;
    const int q0 = qt * kF32Tile;
    const int t_begin = (int)((int64_t)tiles * split / a.splits), t_end = (int)((int64_t)tiles * (split + 1) / a.splits);

    int ql[2], qi[2]; int32_t gq[2];
    float m[2], l[2], ps[2], pc[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        ql[j] = F32T_BROW(L, 0, j);
        qi[j] = q0 + ql[j];
        gq[j] = a.gid[qi[j]];
        m[j] = -INFINITY; l[j] = 0.f; ps[j] = 0.f; pc[j] = 0.f;
    }

    for (int t = t_begin; t < t_end; ++t) {
        const int key0 = t * kF32Tile;
        // read after the K loop's barriers; two images by parity: the next tile's write cannot meet this tile's readers
        int32_t* const kgt = kg[(t - t_begin) & 1];
        if (tid < kF32Tile) kgt[tid] = a.gid[key0 + tid];
        f32x16 acc[2][2];
        f32t_product(a.zn, a.pP, key0, a.nP, a.zn, a.pP, q0, a.nP, a.pP, ldsA, ldsB, tid, acc);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float mt = -INFINITY;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int ki = F32T_AROW(L, key0, i, e);
                    const float s = acc[i][j][e] * a.invT;
                    acc[i][j][e] = s;
                    if (ki < a.n && ki != qi[j]) mt = fmaxf(mt, s);
                }
            const float mn = fmaxf(m[j], mt);
            const float alpha = m[j] == -INFINITY ? 0.f : nx_exp(m[j] - mn);
            float sum = 0.f;
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int kl = F32T_AROW(L, 0, i, e);
                    const int ki = key0 + kl;
                    const bool ok = ki < a.n && ki != qi[j];
                    const float s = acc[i][j][e];
                    sum += ok ? nx_exp(s - mn) : 0.f;
                    const bool pos = ok && gq[j] >= 0 && kgt[kl] == gq[j];
                    ps[j] += pos ? s : 0.f;
                    pc[j] += pos ? 1.f : 0.f;
                }
            l[j] = fmaf(l[j], alpha, sum);
            m[j] = mn;
        }
    }

    // the four lanes of a row (wk, h), merged in that order
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        float* o = red[L.wk * 2 + L.h][ql[j]];
        o[0] = m[j]; o[1] = l[j]; o[2] = ps[j]; o[3] = pc[j];
    }
    __syncthreads();
    if (tid < kF32Tile) {
        float M = -INFINITY;
#pragma unroll
        for (int s = 0; s < 4; ++s) M = fmaxf(M, red[s][tid][0]);
        float Lsum = 0.f, PS = 0.f, PC = 0.f;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const float ms = red[s][tid][0];
            const float w = ms == -INFINITY ? 0.f : nx_exp(ms - M);
            Lsum = fmaf(w, red[s][tid][1], Lsum);
            PS += red[s][tid][2];
            PC += red[s][tid][3];
        }
        float* o = a.part + ((int64_t)split * a.nP + q0 + tid) * 4;
        o[0] = M; o[1] = Lsum; o[2] = PS; o[3] = PC;
    }
}

// splits merged in ascending order: D = M + log L, l = D - possum / c
__global__ __launch_bounds__(256) void nx_combine_kernel(const float* __restrict__ part, int n, int nP, int splits, float* __restrict__ row_loss,
                                                         float* __restrict__ lse, int32_t* __restrict__ npos) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float M = -INFINITY;
    for (int s = 0; s < splits; ++s) M = fmaxf(M, part[((int64_t)s * nP + i) * 4]);
    float Lsum = 0.f, PS = 0.f, PC = 0.f;
    for (int s = 0; s < splits; ++s) {
        const float* e = part + ((int64_t)s * nP + i) * 4;
        const float w = e[0] == -INFINITY ? 0.f : nx_exp(e[0] - M);
        Lsum = fmaf(w, e[1], Lsum);
        PS += e[2];
        PC += e[3];
    }
    const float D = Lsum > 0.f ? M + logf(Lsum) : -INFINITY;
    const int c = (int)PC;
    lse[i] = D;
    npos[i] = c;
    row_loss[i] = c > 0 ? D - PS / (float)c : 0.f;
}

// stats = {sum l_i / max(1, m), m}: thread t sums rows t, t + 256, .. in f64, then a fixed tree
__global__ __launch_bounds__(256) void nx_stats_kernel(const float* __restrict__ row_loss, const int32_t* __restrict__ npos, int n,
                                                       float* __restrict__ stats2) {
    __shared__ double sl[256];
    __shared__ int sm[256];
    double acc = 0.0;
    int cnt = 0;
    for (int i = threadIdx.x; i < n; i += 256) {
        acc += (double)row_loss[i];
        cnt += npos[i] > 0;
    }
    sl[threadIdx.x] = acc;
    sm[threadIdx.x] = cnt;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) { sl[threadIdx.x] += sl[threadIdx.x + o]; sm[threadIdx.x] += sm[threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        stats2[0] = (float)(sl[0] / (double)max(1, sm[0]));
        stats2[1] = (float)sm[0];
    }
}

// ---------------------------------------------------------------- backward
struct NxBwdArgs {
    const float* zn; const float* znT; const int32_t* gid;
    const float* Dp; const float* wv; const float* wc; const float* inv; const int32_t* live;
    float* E;                    // [rb][nP]
    float* dzn;                  // [rb][pP]: E . zn, not yet times 1 / T
    float* df; int64_t lddf;
    int n, nP, p, pP, r0, rb;    // this block: rows r0 .. r0 + rb (rb a multiple of 128)
    float invT, eps;
};

// E [i - r0][j] = w_i exp(s_ij - D_i) + w_j exp(s_ij - D_j) - [same group] (w_i / c_i + w_j / c_j);  0 for j == i and beyond n
__global__ __launch_bounds__(256) void nx_e_kernel(NxBwdArgs a) {
    __shared__ __attribute__((aligned(16))) float ldsA[kF32Tile * kF32Row];
    __shared__ __attribute__((aligned(16))) float ldsB[kF32Tile * kF32Row];
    __shared__ float rD[kF32Tile], rW[kF32Tile], rC[kF32Tile];
    __shared__ int32_t rG[kF32Tile];
    const int tid = threadIdx.x;
    const F32TileLane L = f32t_lane(tid);
    const int rtiles = a.rb / kF32Tile;
    const int rt = blockIdx.x % rtiles, ct = blockIdx.x / rtiles;
    const int i0 = a.r0 + rt * kF32Tile, j0 = ct * kF32Tile;
    if (tid < kF32Tile) {      // read after the K loop's barriers
        rD[tid] = a.Dp[i0 + tid]; rW[tid] = a.wv[i0 + tid]; rC[tid] = a.wc[i0 + tid]; rG[tid] = a.gid[i0 + tid];
    }
    f32x16 acc[2][2];
    f32t_product(a.zn, a.pP, i0, a.nP, a.zn, a.pP, j0, a.nP, a.pP, ldsA, ldsB, tid, acc);
    int cj[2]; int32_t gj[2]; float Dj[2], wj[2], wcj[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        cj[j] = F32T_BROW(L, j0, j);
        gj[j] = a.gid[cj[j]]; Dj[j] = a.Dp[cj[j]]; wj[j] = a.wv[cj[j]]; wcj[j] = a.wc[cj[j]];
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int il = F32T_AROW(L, 0, i, e);
            const int gi = i0 + il;
            const float Di = rD[il], wi = rW[il], wci = rC[il];
            const int32_t gri = rG[il];
            float* erow = a.E + (int64_t)(gi - a.r0) * a.nP;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const float s = acc[i][j][e] * a.invT;
                const bool ok = gi < a.n && cj[j] < a.n && gi != cj[j];
                const bool pos = gj[j] >= 0 && gj[j] == gri;
                const float v = fmaf(wi, nx_exp(s - Di), wj[j] * nx_exp(s - Dj[j])) - (pos ? wci + wcj[j] : 0.f);
                erow[cj[j]] = ok ? v : 0.f;
            }
        }
}

// dzn [i - r0][c] = sum_k E [i - r0][k] znT [c][k]
__global__ __launch_bounds__(256) void nx_dzn_kernel(NxBwdArgs a) {
    __shared__ __attribute__((aligned(16))) float ldsA[kF32Tile * kF32Row];
    __shared__ __attribute__((aligned(16))) float ldsB[kF32Tile * kF32Row];
    const int tid = threadIdx.x;
    const F32TileLane L = f32t_lane(tid);
    const int ctiles = (a.pP + kF32Tile - 1) / kF32Tile;
    const int ct = blockIdx.x % ctiles, rt = blockIdx.x / ctiles;
    f32x16 acc[2][2];
    f32t_product(a.E, a.nP, rt * kF32Tile, a.rb, a.znT, a.nP, ct * kF32Tile, a.pP, a.nP, ldsA, ldsB, tid, acc);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int il = F32T_AROW(L, rt * kF32Tile, i, e);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int c = F32T_BROW(L, ct * kF32Tile, j);
                if (c < a.pP) a.dzn[(int64_t)il * a.pP + c] = acc[i][j][e];
            }
        }
}

// df_i = inv_i (dzn_i - zn_i (zn_i . dzn_i)), or dzn_i / eps where the norm was clamped; one wave per row of the block
__global__ __launch_bounds__(256) void nx_dfrow_kernel(NxBwdArgs a) {
    const int lane = threadIdx.x & 63;
    const int il = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int row = a.r0 + il;
    if (il >= a.rb || row >= a.n) return;
    const float* z = a.zn + (int64_t)row * a.pP;
    const float* g = a.dzn + (int64_t)il * a.pP;
    float* out = a.df + (int64_t)row * a.lddf;
    if (a.live[row]) {
        float dot = 0.f;
        for (int d = lane; d < a.p; d += 64) dot = fmaf(z[d], g[d] * a.invT, dot);
        dot = wave_sum(dot);
        const float inv = a.inv[row];
        for (int d = lane; d < a.p; d += 64) out[d] = inv * (g[d] * a.invT - z[d] * dot);
    } else {
        for (int d = lane; d < a.p; d += 64) out[d] = g[d] * a.invT / a.eps;
    }
}

// ---------------------------------------------------------------- host side
int nx_np(int n) { return (n + kF32Tile - 1) / kF32Tile * kF32Tile; }
int nx_pp(int p) { return (p + kF32KStep - 1) / kF32KStep * kF32KStep; }

int nx_check_shape(const char* who, int n, int p, int key_splits, int block_rows) {
    BVC_REQUIRE(n >= 1 && n <= kNxMaxN, "%s: n %d outside 1 .. %d", who, n, kNxMaxN);
    BVC_REQUIRE(p >= 1 && p <= kNxMaxP, "%s: p %d outside 1 .. %d", who, p, kNxMaxP);
    BVC_REQUIRE(key_splits >= 0 && key_splits <= kNxMaxSplits, "%s: key_splits %d outside 0 .. %d", who, key_splits, kNxMaxSplits);
    BVC_REQUIRE(block_rows >= 0, "%s: negative block_rows %d", who, block_rows);
    return BVC_OK;
}

int nx_check_args(const char* who, const float* f, int64_t ldf, const int32_t* groups, int views, int n, int p, float temperature,
                  float eps, const void* workspace) {
    BVC_REQUIRE(f && workspace, "%s: null argument", who);
    BVC_REQUIRE(ldf >= p, "%s: row stride %lld below p %d", who, (long long)ldf, p);
    BVC_REQUIRE(isfinite(temperature) && temperature > 0.f, "%s: temperature %g is not a positive finite number", who, (double)temperature);
    BVC_REQUIRE(isfinite(eps) && eps > 0.f, "%s: eps %g is not a positive finite number", who, (double)eps);
    BVC_REQUIRE(groups || (views >= 1 && n % views == 0), "%s: views %d does not divide n %d", who, views, n);
    BVC_REQUIRE(((uintptr_t)f & 3) == 0 && ((uintptr_t)groups & 3) == 0 && ((uintptr_t)workspace & 15) == 0,
                "%s: f and groups must be 4-byte, the workspace 16-byte aligned", who);
    return BVC_OK;
}

// about two workgroups per CU, every split at least one key tile, at most 64
int nx_auto_splits(int n) {
    const int tiles = nx_np(n) / kF32Tile;
    int s = (2 * kNxCUs + tiles - 1) / tiles;
    if (s > tiles) s = tiles;
    if (s > 64) s = 64;
    return s < 1 ? 1 : s;
}

// whole tiles of rows under the cap of the E block, at least one tile, at most all rows
int nx_auto_block_rows(int n) {
    const int nP = nx_np(n);
    int64_t r = kNxEBlockBytes / ((int64_t)nP * 4) / kF32Tile * kF32Tile;
    if (r < kF32Tile) r = kF32Tile;
    if (r > nP) r = nP;
    return (int)r;
}
int nx_resolve_block_rows(int n, int block_rows) {
    if (block_rows <= 0) return nx_auto_block_rows(n);
    const int nP = nx_np(n);
    int64_t r = ((int64_t)block_rows + kF32Tile - 1) / kF32Tile * kF32Tile;
    return (int)(r > nP ? nP : r);
}

struct NxLayout {
    int nP, pP, splits, R;
    int64_t inv, live, gid, Dp, wv, wc, part, zn, znT, E, dzn, total;
};
NxLayout nx_layout(int n, int p, int key_splits, int block_rows) {
    NxLayout w;
    w.nP = nx_np(n); w.pP = nx_pp(p);
    w.splits = key_splits > 0 ? key_splits : nx_auto_splits(n);
    w.R = nx_resolve_block_rows(n, block_rows);
    int64_t o = 0;
    const int64_t vec = ws_align((int64_t)w.nP * 4);
    w.inv = o; o += vec; w.live = o; o += vec; w.gid = o; o += vec; w.Dp = o; o += vec; w.wv = o; o += vec; w.wc = o; o += vec;
    w.part = o; o += ws_align((int64_t)w.splits * w.nP * 16);
    w.zn = o; o += ws_align((int64_t)w.nP * w.pP * 4);
    w.znT = o; o += ws_align((int64_t)w.nP * w.pP * 4);
    w.E = o; o += ws_align((int64_t)w.R * w.nP * 4);
    w.dzn = o; o += ws_align((int64_t)w.R * w.pP * 4);
    w.total = o;
    return w;
}

int nx_prologue(const NxLayout& w, NxRowArgs& ra, void* ws, hipStream_t s) {
    ra.nP = w.nP; ra.pP = w.pP;
    ra.inv = ws_at<float>(ws, w.inv); ra.live = ws_at<int32_t>(ws, w.live); ra.gid = ws_at<int32_t>(ws, w.gid); ra.zn = ws_at<float>(ws, w.zn);
    ra.Dp = ws_at<float>(ws, w.Dp); ra.wv = ws_at<float>(ws, w.wv); ra.wc = ws_at<float>(ws, w.wc);
    nx_rows_kernel<<<dim3((unsigned)(w.nP / 4)), dim3(256), 0, s>>>(ra);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

}  // namespace

int ntxent_splits(int n, int p) {
    if (nx_check_shape("op_ntxent_splits", n, p, 0, 0) != BVC_OK) return -1;
    return nx_auto_splits(n);
}

int ntxent_block_rows(int n, int p) {
    if (nx_check_shape("op_ntxent_block_rows", n, p, 0, 0) != BVC_OK) return -1;
    return nx_auto_block_rows(n);
}

int64_t ntxent_workspace(int n, int p, int key_splits, int block_rows) {
    if (nx_check_shape("op_ntxent_workspace", n, p, key_splits, block_rows) != BVC_OK) return -1;
    return nx_layout(n, p, key_splits, block_rows).total;
}

int launch_ntxent_fwd(const float* f, int64_t ldf, const int32_t* groups, int views, int n, int p, float temperature, float eps,
                      int key_splits, float* row_loss, float* lse, int32_t* npos, float* stats2, void* workspace, hipStream_t s) {
    if (int rc = nx_check_shape("op_ntxent_fwd", n, p, key_splits, 0)) return rc;
    if (int rc = nx_check_args("op_ntxent_fwd", f, ldf, groups, views, n, p, temperature, eps, workspace)) return rc;
    BVC_REQUIRE(row_loss && lse && npos && stats2, "op_ntxent_fwd: null argument");
    const NxLayout w = nx_layout(n, p, key_splits, 0);
    NxRowArgs ra{};
    ra.f = f; ra.ldf = ldf; ra.groups = groups; ra.views = views; ra.n = n; ra.p = p; ra.eps = eps;
    if (int rc = nx_prologue(w, ra, workspace, s)) return rc;
    NxFwdArgs a{ra.zn, ra.gid, ws_at<float>(workspace, w.part), n, w.nP, w.pP, w.splits, 1.0f / temperature};
    nx_fwd_kernel<<<dim3((unsigned)(w.nP / kF32Tile * w.splits)), dim3(256), 0, s>>>(a);
    BVC_CHECK_HIP(hipGetLastError());
    nx_combine_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s>>>(a.part, n, w.nP, w.splits, row_loss, lse, npos);
    nx_stats_kernel<<<dim3(1), dim3(256), 0, s>>>(row_loss, npos, n, stats2);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

int launch_ntxent_bwd(const float* f, int64_t ldf, const int32_t* groups, int views, int n, int p, float temperature, float eps,
                      const float* lse, const int32_t* npos, const float* row_weight, int key_splits, int block_rows, float* df,
                      int64_t lddf, void* workspace, hipStream_t s) {
    if (int rc = nx_check_shape("op_ntxent_bwd", n, p, key_splits, block_rows)) return rc;
    if (int rc = nx_check_args("op_ntxent_bwd", f, ldf, groups, views, n, p, temperature, eps, workspace)) return rc;
    BVC_REQUIRE(lse && npos && row_weight && df, "op_ntxent_bwd: null argument");
    BVC_REQUIRE(lddf >= p, "op_ntxent_bwd: row stride of df %lld below p %d", (long long)lddf, p);
    const NxLayout w = nx_layout(n, p, key_splits, block_rows);
    NxRowArgs ra{};
    ra.f = f; ra.ldf = ldf; ra.groups = groups; ra.views = views; ra.n = n; ra.p = p; ra.eps = eps;
    ra.lse = lse; ra.npos = npos; ra.row_weight = row_weight;
    if (int rc = nx_prologue(w, ra, workspace, s)) return rc;
    float* znT = ws_at<float>(workspace, w.znT);
    nx_transpose_kernel<<<dim3((unsigned)(w.pP / 32), (unsigned)(w.nP / 32)), dim3(256), 0, s>>>(ra.zn, znT, w.nP, w.pP);
    BVC_CHECK_HIP(hipGetLastError());
    NxBwdArgs a{};
    a.zn = ra.zn; a.znT = znT; a.gid = ra.gid; a.Dp = ra.Dp; a.wv = ra.wv; a.wc = ra.wc; a.inv = ra.inv; a.live = ra.live;
    a.E = ws_at<float>(workspace, w.E); a.dzn = ws_at<float>(workspace, w.dzn); a.df = df; a.lddf = lddf;
    a.n = n; a.nP = w.nP; a.p = p; a.pP = w.pP; a.invT = 1.0f / temperature; a.eps = eps;
    const int tiles = w.nP / kF32Tile, ctiles = (w.pP + kF32Tile - 1) / kF32Tile;
    for (int r0 = 0; r0 < w.nP; r0 += w.R) {
        a.r0 = r0;
        a.rb = w.nP - r0 < w.R ? w.nP - r0 : w.R;
        const int rtiles = a.rb / kF32Tile;
        nx_e_kernel<<<dim3((unsigned)(rtiles * tiles)), dim3(256), 0, s>>>(a);
        nx_dzn_kernel<<<dim3((unsigned)(rtiles * ctiles)), dim3(256), 0, s>>>(a);
        nx_dfrow_kernel<<<dim3((unsigned)(a.rb / 4)), dim3(256), 0, s>>>(a);
        BVC_CHECK_HIP(hipGetLastError());
    }
    return BVC_OK;
}

}  // namespace bvc

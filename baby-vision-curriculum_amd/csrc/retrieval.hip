// Embedding retrieval: for every f32 query row the k best f32 key rows under the cosine or the Euclidean metric, as indices and
// distances, without ever storing a [Q][N] array (bvc_op_topk; the reference scores its embeddings with sklearn's dense
// cosine_distances + argsort in notebooks/EvaluateEmbeddings.ipynb get_nn_score / topk_retrieval).
//
// Arithmetic: f32 throughout.  dot(q, key) is ONE accumulation chain over d = 0 .. D-1 on v_mfma_f32_32x32x2_f32, which is bit for
// bit a d-ordered fmaf chain starting at 0; the D tail of the last 32-wide step is zero-filled (fma(0, 0, acc) = acc), there is no
// split over D, and the chain of a pair does not depend on where the pair sits in a tile, a key split or a chunk of an accumulate
// loop.  The row statistics come from one kernel (retr_rownorm_kernel: lane l sums x[d]^2 over d = l, l + 64, .. with fmaf, then the
// xor butterfly 32, 16, .. 1): 1 / sqrt(|x|^2) (0 for a zero row) for cosine, |x|^2 for Euclidean.
//   cosine     score = (dot * inv|key|) * inv|q|            value = 1 - score                       (sklearn cosine_distances)
//   Euclidean  d2 = max(fma(-2, dot, |q|^2 + |key|^2), 0)    value = sqrt(d2)                        (sklearn euclidean_distances)
//
// Order: total.  The value is a non-increasing function of the score (1 - s and sqrt are monotone and correctly rounded), and the
// order is (value ascending, key index ascending): better score first, and among candidates whose results are bit-equal the smaller
// index.  Ranking on the RETURNED bits is what lets accumulate = 1 restart from nothing but an earlier call's outputs and still
// give the bits of one call over the concatenated gallery.  Every candidate is one unsigned 64-bit word,
//   high = order-preserving image of the bits of -value, low = ~index      (real candidates are > 0; 0 = empty slot),
// so sorting, merging and thresholding are one unsigned compare, and the result does not depend on arrival order anywhere.
//
// retr_topk_kernel: one workgroup owns 128 queries and a range of key tiles (128 keys each).  Per key tile the K loop of f32_tile.h,
// here over the caller's rows as they are (any stride, any D: f32t_load_raw), with the KEYS as the A operand: the query is on the
// lane, so a lane keeps its two queries' thresholds in registers and the candidate counters of one instruction's lanes are distinct.
// Selection: per query row a sorted list of k words in LDS and its k-th word as the threshold.  A lane turns its 64 scores into
// words, appends those above the threshold to the row's queue (integer LDS counter), and a wave merges a row's queue into its list
// by rank (every word counts the words above it: the ranks of distinct words are a permutation, so there is nothing to sort).  A
// queue holds 32 words; what does not fit stays in its register and is offered again after the merge, against the raised
// threshold - so the first tiles take several passes and later ones one pass with few or no survivors.  A queue is merged
// once it is half full (and at the end), not after every tile: the cost of a merge hardly depends on what the queue holds.
// Each workgroup writes its rows' lists to the workspace ([split][Q][k] words); retr_finish_kernel merges the splits (and, with
// accumulate, the outputs of the earlier calls) per query by the same rank merge and writes indices and values.  No float atomics,
// no dependence on timing: the same bits on every run, for every key_splits and every chunking.
#include <math.h>

#include "f32_tile.h"

namespace bvc {

typedef unsigned long long u64;

constexpr int kRetrQueue = 32;       // candidate words per row and pass
constexpr int kRetrMaxK = 64;
constexpr int kRetrCUs = 256;

__device__ __forceinline__ u64 retr_word(float value, int index) {
    uint32_t u = __float_as_uint(-value);
    u ^= (u >> 31) ? 0xffffffffu : 0x80000000u;
    return ((u64)u << 32) | (uint32_t)~index;
}
__device__ __forceinline__ float retr_value(u64 w) {
    uint32_t u = (uint32_t)(w >> 32);
    u ^= (u >> 31) ? 0x80000000u : 0xffffffffu;
    return -__uint_as_float(u);
}

// Merge the words cand[0 .. ncand) (0 = none) into the descending list[0 .. k) (0 = empty, after the real ones), by one wave.
// Real words are distinct, so rank = number of real words above is a permutation of 0 .. count-1; the best k are scattered.
// Lane l holds list[l] and cand[l]; candidate t is broadcast from its lane and ranked by two ballots (list words above it,
// candidates above it), so the only LDS traffic is one read and one write of each word: no dependent chain of LDS reads.
__device__ __forceinline__ void retr_merge_row(u64* list, int k, const u64* cand, int ncand, int lane) {
    const u64 mine = lane < k ? list[lane] : 0ull;
    const u64 c = lane < ncand ? cand[lane] : 0ull;
    const uint32_t clo = (uint32_t)c, chi = (uint32_t)(c >> 32);
    int rank_l = lane, rank_c = 0;
    for (int t = 0; t < ncand; ++t) {      // (ncand is wave-uniform)
        const u64 x = ((u64)(uint32_t)__builtin_amdgcn_readlane((int)chi, t) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)clo, t);
        rank_l += x > mine;
        const int above = __popcll(__ballot(mine > x)) + __popcll(__ballot(c > x));
        if (lane == t) rank_c = above;
    }
    __builtin_amdgcn_wave_barrier();      // every read of the old list is above, every write below (one wave: LDS is in order)
    if (mine != 0ull && rank_l < k) list[rank_l] = mine;
    if (c != 0ull && rank_c < k) list[rank_c] = c;
    __builtin_amdgcn_wave_barrier();
}

// out[row] = 1 / sqrt(sum x^2) (0 for a zero row) when inverse, else sum x^2.  One wave per row.
__global__ __launch_bounds__(256) void retr_rownorm_kernel(const float* __restrict__ x, int64_t ld, int rows, int D, int inverse,
                                                           float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* p = x + row * ld;
    float s = 0.f;
    for (int d = lane; d < D; d += 64) s = fmaf(p[d], p[d], s);
    s = wave_sum(s);
    if (lane == 0) out[row] = inverse ? (s > 0.f ? 1.0f / sqrtf(s) : 0.f) : s;
}

// The rows of this wave (wave + 4 l, l = 0 .. 31) whose queue holds at least `least` words: merge, raise the threshold, empty the
// queue.  Lane l looks at one row's counter and the wave walks the set bits.  A queue is left to fill to half (least = 16) before
// it is merged - a later merge costs one pass whatever it holds, and a stale threshold only lets more candidates in - and every
// queue is flushed (least = 1) after the last tile.  A queue that overflowed is full, so the pass after an overflow finds room.
__device__ __forceinline__ void retr_merge_rows(u64* list, u64* queue, u64* thr, int* cnt, int k, int least, int wave, int lane) {
    const int mine = lane < kF32Tile / 4 ? cnt[wave + 4 * lane] : 0;
    u64 work = __ballot(mine >= least);
    while (work) {
        const int l = __ffsll((unsigned long long)work) - 1;
        work &= work - 1;
        const int row = wave + 4 * l;
        const int n = min(__builtin_amdgcn_readlane(mine, l), kRetrQueue);
        retr_merge_row(list + row * kRetrMaxK, k, queue + row * kRetrQueue, n, lane);
        if (lane == 0) { thr[row] = list[row * kRetrMaxK + k - 1]; cnt[row] = 0; }
    }
}

struct RetrArgs {
    const float* q; const float* keys;
    int64_t ldq, ldk;
    const float* qstat; const float* kstat;      // per-row statistic of retr_rownorm_kernel
    u64* lists;                                   // [splits][Q][k]
    int Q, N, D, k, splits, key_base, select;
};

// dynamic LDS (bytes): operands 2 x 128 x 36 x 4 | lists 128 x 64 x 8 | queues 128 x 32 x 8 | thresholds 128 x 8 | key statistic
// 128 x 4 | counters 128 x 4 | 2 pass flags
constexpr int kRetrOffList = 2 * kF32Tile * kF32Row * 4;
constexpr int kRetrOffQueue = kRetrOffList + kF32Tile * kRetrMaxK * 8;
constexpr int kRetrOffThr = kRetrOffQueue + kF32Tile * kRetrQueue * 8;
constexpr int kRetrOffStat = kRetrOffThr + kF32Tile * 8;
constexpr int kRetrOffCnt = kRetrOffStat + kF32Tile * 4;
constexpr int kRetrOffFlag = kRetrOffCnt + kF32Tile * 4;
constexpr int kRetrLds = kRetrOffFlag + 16;

template <int METRIC, bool VEC>
__global__ __launch_bounds__(256) void retr_topk_kernel(RetrArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* const ldsK = reinterpret_cast<float*>(smem);
    float* const ldsQ = ldsK + kF32Tile * kF32Row;
    u64* const list = reinterpret_cast<u64*>(smem + kRetrOffList);
    u64* const queue = reinterpret_cast<u64*>(smem + kRetrOffQueue);
    u64* const thr = reinterpret_cast<u64*>(smem + kRetrOffThr);
    float* const kstat = reinterpret_cast<float*>(smem + kRetrOffStat);
    int* const cnt = reinterpret_cast<int*>(smem + kRetrOffCnt);
    int* const flag = reinterpret_cast<int*>(smem + kRetrOffFlag);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const F32TileLane L = f32t_lane(tid);
    const int qtiles = (a.Q + kF32Tile - 1) / kF32Tile;
    const int qt = blockIdx.x % qtiles, split = blockIdx.x / qtiles;      // query tiles of one split run side by side
    const int q0 = qt * kF32Tile;
    const int ktiles = (a.N + kF32Tile - 1) / kF32Tile;
    const int t_begin = (int)((int64_t)ktiles * split / a.splits), t_end = (int)((int64_t)ktiles * (split + 1) / a.splits);
    const int k = a.k;

    for (int i = tid; i < kF32Tile * kRetrMaxK; i += 256) list[i] = 0ull;
    if (tid < kF32Tile) { thr[tid] = 0ull; cnt[tid] = 0; }
    if (tid < 2) flag[tid] = 0;

    // this lane's two queries (j = 0, 1): local row, validity, statistic
    int ql[2]; bool qok[2]; float qs[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        ql[j] = F32T_BROW(L, 0, j);
        qok[j] = q0 + ql[j] < a.Q;
        qs[j] = a.qstat[min(q0 + ql[j], a.Q - 1)];
    }
    const int ksteps = (a.D + kF32KStep - 1) / kF32KStep;
    int pass = 0;
    __syncthreads();

    for (int t = t_begin; t < t_end; ++t) {
        const int key0 = t * kF32Tile;
        if (tid < kF32Tile) kstat[tid] = a.kstat[min(key0 + tid, a.N - 1)];      // read after the K loop's barriers
        f32x16 acc[2][2];
        f32t_zero(acc);
        f32x4 vk[4], vq[4];
        f32t_load_raw<VEC>(a.keys, a.ldk, key0, a.N, 0, a.D, tid, vk);
        f32t_load_raw<VEC>(a.q, a.ldq, q0, a.Q, 0, a.D, tid, vq);
        for (int s = 0; s < ksteps; ++s) {
            f32t_stage(ldsK, tid, vk);
            f32t_stage(ldsQ, tid, vq);
            __syncthreads();
            if (s + 1 < ksteps) {
                f32t_load_raw<VEC>(a.keys, a.ldk, key0, a.N, (s + 1) * kF32KStep, a.D, tid, vk);
                f32t_load_raw<VEC>(a.q, a.ldq, q0, a.Q, (s + 1) * kF32KStep, a.D, tid, vq);
            }
            f32t_step(ldsK, ldsQ, tid, acc);
            __syncthreads();      // the stage is free for the next step's write
        }

        // ---- values in place.  Element e of acc[i][j]: key row F32T_AROW(L, 0, i, e), query ql[j]
        uint32_t pend[2] = {0u, 0u};       // per j: bit 16 i + e = still to be offered
        float reach[2];                    // the value of the row's threshold (+inf while its list is not full): a value above it
#pragma unroll                             // cannot pass, so the 64-bit word is built only for the few that are at or below it
        for (int j = 0; j < 2; ++j) {
            const u64 th = thr[ql[j]];
            reach[j] = th ? retr_value(th) : INFINITY;
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int kl = F32T_AROW(L, 0, i, e);
                const float ks = kstat[kl];
                const bool kok = key0 + kl < a.N;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const float dot = acc[i][j][e];
                    float v;
                    if (METRIC == 0) v = 1.0f - (dot * ks) * qs[j];
                    else v = sqrtf(fmaxf(fmaf(-2.0f, dot, qs[j] + ks), 0.0f));
                    acc[i][j][e] = v + 0.0f;      // (-0 -> +0: one image per value)
                    if (kok && qok[j] && v <= reach[j]) pend[j] |= 1u << (16 * i + e);
                }
            }
        if (!a.select) pend[0] = pend[1] = 0u;      // timing ablation of tools/bench_retrieval.py only: accept nothing

        // ---- offer, merge, repeat while a queue overflowed
        for (;;) {
            const int par = pass & 1;
            bool over = false;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                if (pend[j] == 0u) continue;
                const u64 th = thr[ql[j]];
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const uint32_t bit = 1u << (16 * i + e);
                        if (pend[j] & bit) {
                            const int kl = F32T_AROW(L, 0, i, e);
                            const u64 w = retr_word(acc[i][j][e], a.key_base + key0 + kl);
                            if (w > th) {
                                const int slot = atomicAdd(&cnt[ql[j]], 1);
                                if (slot < kRetrQueue) { queue[ql[j] * kRetrQueue + slot] = w; pend[j] &= ~bit; }
                                else over = true;
                            } else pend[j] &= ~bit;      // the threshold only rises
                        }
                    }
            }
            if (over) flag[par] = 1;
            __syncthreads();
            const int again = flag[par];
            if (tid == 0) flag[par ^ 1] = 0;
            retr_merge_rows(list, queue, thr, cnt, k, kRetrQueue / 2, wave, lane);
            ++pass;
            __syncthreads();
            if (!again) break;
        }
    }

    // ---- what is still queued, then this split's lists
    retr_merge_rows(list, queue, thr, cnt, k, 1, wave, lane);
    __syncthreads();
    for (int i = tid; i < kF32Tile * k; i += 256) {
        const int row = i / k, j = i - row * k;
        if (q0 + row < a.Q) a.lists[((int64_t)split * a.Q + q0 + row) * k + j] = list[row * kRetrMaxK + j];
    }
}

// One wave per query: merge the splits' lists (and the earlier calls' outputs when accumulate) and write indices and values.
__global__ __launch_bounds__(256) void retr_finish_kernel(const u64* __restrict__ lists, int Q, int k, int splits, int accumulate,
                                                          int* __restrict__ out_idx, float* __restrict__ out_val) {
    __shared__ u64 sl[4][kRetrMaxK], sc[4][kRetrMaxK];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t q = (int64_t)blockIdx.x * 4 + wave;
    if (q >= Q) return;      // (wave-uniform; no workgroup barrier below)
    u64 w = 0ull;
    if (accumulate && lane < k) {
        const int idx = out_idx[q * k + lane];
        if (idx >= 0) w = retr_word(out_val[q * k + lane] + 0.0f, idx);
    }
    sl[wave][lane] = w;
    __builtin_amdgcn_wave_barrier();
    for (int s = 0; s < splits; ++s) {
        sc[wave][lane] = lane < k ? lists[((int64_t)s * Q + q) * k + lane] : 0ull;
        __builtin_amdgcn_wave_barrier();
        retr_merge_row(sl[wave], k, sc[wave], k, lane);
    }
    if (lane < k) {
        w = sl[wave][lane];
        out_idx[q * k + lane] = w ? (int)~(uint32_t)w : -1;
        out_val[q * k + lane] = w ? retr_value(w) : INFINITY;
    }
}

// ---------------------------------------------------------------- host side

static int retr_auto_splits(int Q, int N) {
    // One workgroup per CU at a time (LDS), so the cost of s splits is rounds x work of a workgroup:
    //   ceil(query tiles x s / CUs) x (key tiles per split + 8),   8 tiles standing for a split's start-up passes and its merge.
    // Few query tiles: the key range is cut until the CUs are busy; many: s is chosen so that the last round is nearly full.
    // Each split covers at least 4 key tiles, at most 64 splits; ties go to the smaller s.
    const int64_t qtiles = ((int64_t)Q + kF32Tile - 1) / kF32Tile, ktiles = ((int64_t)N + kF32Tile - 1) / kF32Tile;
    int64_t most = ktiles / 4;
    if (most > 64) most = 64;
    int best = 1;
    int64_t best_cost = -1;
    for (int64_t s = 1; s <= (most > 1 ? most : 1); ++s) {
        const int64_t rounds = (qtiles * s + kRetrCUs - 1) / kRetrCUs;
        const int64_t cost = rounds * ((ktiles + s - 1) / s + 8);
        if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = (int)s; }
    }
    return best;
}

static int retr_resolve_splits(int Q, int N, int key_splits) {
    const int64_t ktiles = ((int64_t)N + kF32Tile - 1) / kF32Tile;
    int s = key_splits > 0 ? key_splits : retr_auto_splits(Q, N);
    if (s > ktiles) s = (int)ktiles;      // no empty split
    return s;
}

static int retr_check_shape(int Q, int N, int D, int k, int key_splits) {
    BVC_REQUIRE(Q > 0 && N > 0 && D > 0, "op_topk: non-positive size (Q %d, N %d, D %d)", Q, N, D);
    BVC_REQUIRE(k >= 1 && k <= kRetrMaxK, "op_topk: k %d outside 1 .. %d", k, kRetrMaxK);
    BVC_REQUIRE(key_splits >= 0, "op_topk: negative key_splits %d", key_splits);
    return BVC_OK;
}

int64_t retr_workspace(int Q, int N, int D, int k, int key_splits) {
    if (retr_check_shape(Q, N, D, k, key_splits) != BVC_OK) return -1;
    const int s = retr_resolve_splits(Q, N, key_splits);
    return ws_align((int64_t)Q * 4) + ws_align((int64_t)N * 4) + (int64_t)s * Q * k * 8;
}

int retr_splits(int Q, int N, int D, int k) {
    if (retr_check_shape(Q, N, D, k, 0) != BVC_OK) return -1;
    return retr_resolve_splits(Q, N, 0);
}

int launch_topk(const float* queries, int64_t ldq, const float* keys, int64_t ldk, int Q, int N, int D, int k, int metric,
                int key_splits, int key_base, int accumulate, int* out_idx, float* out_val, void* workspace, hipStream_t stream,
                int select) {
    if (int rc = retr_check_shape(Q, N, D, k, key_splits)) return rc;
    BVC_REQUIRE(queries && keys && out_idx && out_val && workspace, "op_topk: null argument");
    BVC_REQUIRE(metric == 0 || metric == 1, "op_topk: metric %d (0 cosine, 1 euclidean)", metric);
    BVC_REQUIRE(ldq >= D && ldk >= D, "op_topk: row stride below D (ldq %lld, ldk %lld, D %d)", (long long)ldq, (long long)ldk, D);
    BVC_REQUIRE(key_base >= 0 && (int64_t)key_base + N <= 0x7fffffffll, "op_topk: key_base %d + N %d overflows int", key_base, N);
    BVC_REQUIRE(accumulate == 0 || accumulate == 1, "op_topk: accumulate %d", accumulate);
    BVC_REQUIRE(((uintptr_t)queries & 3) == 0 && ((uintptr_t)keys & 3) == 0 && ((uintptr_t)workspace & 7) == 0, "op_topk: misaligned pointer");
    const int splits = retr_resolve_splits(Q, N, key_splits);
    const int64_t qtiles = ((int64_t)Q + kF32Tile - 1) / kF32Tile;
    BVC_REQUIRE(qtiles * splits < 0x7fffffffll, "op_topk: %lld workgroups exceed the grid", (long long)(qtiles * splits));

    float* qstat = ws_at<float>(workspace, 0);
    float* kstat = ws_at<float>(workspace, ws_align((int64_t)Q * 4));
    u64* lists = ws_at<u64>(workspace, ws_align((int64_t)Q * 4) + ws_align((int64_t)N * 4));

    retr_rownorm_kernel<<<dim3((unsigned)(((int64_t)Q + 3) / 4)), dim3(256), 0, stream>>>(queries, ldq, Q, D, metric == 0, qstat);
    retr_rownorm_kernel<<<dim3((unsigned)(((int64_t)N + 3) / 4)), dim3(256), 0, stream>>>(keys, ldk, N, D, metric == 0, kstat);
    BVC_CHECK_HIP(hipGetLastError());

    RetrArgs a{queries, keys, ldq, ldk, qstat, kstat, lists, Q, N, D, k, splits, key_base, select};
    const bool vec = ((uintptr_t)queries & 15) == 0 && ((uintptr_t)keys & 15) == 0 && ldq % 4 == 0 && ldk % 4 == 0;
    void (*kern)(RetrArgs) = metric == 0 ? (vec ? retr_topk_kernel<0, true> : retr_topk_kernel<0, false>)
                                         : (vec ? retr_topk_kernel<1, true> : retr_topk_kernel<1, false>);
    static_assert(kRetrLds <= 160 * 1024, "retrieval: LDS");
    BVC_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, kRetrLds));
    kern<<<dim3((unsigned)(qtiles * splits)), dim3(256), kRetrLds, stream>>>(a);
    BVC_CHECK_HIP(hipGetLastError());
    retr_finish_kernel<<<dim3((unsigned)(((int64_t)Q + 3) / 4)), dim3(256), 0, stream>>>(lists, Q, k, splits, accumulate, out_idx, out_val);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

}  // namespace bvc

extern "C" {

int64_t bvc_op_topk_workspace(int Q, int N, int D, int k, int key_splits) { return bvc::retr_workspace(Q, N, D, k, key_splits); }
int bvc_op_topk_splits(int Q, int N, int D, int k) { return bvc::retr_splits(Q, N, D, k); }
int bvc_op_topk(const float* queries, int64_t ldq, const float* keys, int64_t ldk, int Q, int N, int D, int k, int metric,
                int key_splits, int key_base, int accumulate, int* out_idx, float* out_val, void* workspace, void* stream) {
    return bvc::launch_topk(queries, ldq, keys, ldk, Q, N, D, k, metric, key_splits, key_base, accumulate, out_idx, out_val, workspace,
                            (hipStream_t)stream, 1);
}

#ifdef BVC_EXPERIMENTS
// bvc_op_topk with the selection switched off (nothing passes the threshold; the outputs are all -1 / +inf): what
// tools/bench_retrieval.py subtracts to get the selection's share of the time.  Experiments builds only; not in include/bvc.h.
int bvc_exp_topk_no_select(const float* queries, int64_t ldq, const float* keys, int64_t ldk, int Q, int N, int D, int k, int metric,
                           int key_splits, int* out_idx, float* out_val, void* workspace, void* stream) {
    return bvc::launch_topk(queries, ldq, keys, ldk, Q, N, D, k, metric, key_splits, 0, 0, out_idx, out_val, workspace,
                            (hipStream_t)stream, 0);
}
#endif

}  // extern "C"

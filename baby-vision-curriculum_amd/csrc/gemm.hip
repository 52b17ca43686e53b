// bf16 x bf16 -> f32 MFMA GEMM for gfx950 (MI355X), with the fused epilogues the ViT step needs: the per-tile kernel
// (every output tile is one workgroup) and the host-side launcher / tile planner.  gemm_persist.hip holds the persistent form
// that chains tiles for the short-K products; gemm_tile.h the staging / fragment helpers both share.
//
// Structure (per 256-thread workgroup = 4 waves as 2x2, 64-deep K steps):
//   * A and B tiles go HBM -> LDS directly with `buffer_load_dwordx4 ... lds` (LDS-DMA, 1 KiB per
//     wave-instruction).  The buffer descriptor's bounds check returns zeros for rows past the end of
//     the allocation, which is how ragged M / ragged contraction lengths are handled - no host padding.
//   * two LDS slots, "early refill": a wave pulls all fragments of the current K step into registers, a barrier proves
//     the slot drained, the slot is refilled with K step t+2 and only then do the MFMAs run - two K steps of DMA are in
//     flight under the MFMAs; waits are counted (`s_waitcnt vmcnt(N)`) and barriers raw, so the DMA flies across them.
//   * LDS images are XOR-swizzled on the 16-byte chunk index.  LDS-DMA writes lane-linear, so the
//     swizzle is applied to the per-lane SOURCE address and again on the read (both sides or neither).
//   * k-contiguous operands are read with ds_read_b128; operands whose contraction index is the
//     strided one (dX = dY W, dW = dY^T X) stay in their natural layout in HBM and LDS and are
//     transposed on the LDS read by ds_read_b64_tr_b16 - no transposed copies of weights or activations.
//   * v_mfma_f32_16x16x32_bf16 with the operands swapped, so each lane ends up with 4 consecutive
//     output columns of one row; the epilogue parks the f32 tile in LDS and re-reads it row-major so that every global
//     load / store is a full 128-B line per 8 lanes, and fetches all its side inputs before its first store (loads and
//     stores retire through one in-order counter).
//   * block index -> tile mapping is XCD-aware (blocks b and b+8 share an XCD/L2): each XCD gets a contiguous run of
//     tiles, walked in column panels sized for its L2 (NT / NN) or along the short side with K-splits fastest (TN).
//   * up to 4 independent problems per launch (grouped GEMM) to fill 256 CUs with the small
//     weight-gradient products of one transformer layer; split-K with f32 atomics; fused bias gradients.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "gemm_tile.h"

namespace bvc {

Options& options() {
    static Options o;
    return o;
}
DryRun& dry_run() {
    static thread_local DryRun d;
    return d;
}

// ------------------------------------------------------------------ the kernel
// Two LDS slots; waits use a COUNTED vmcnt and raw s_barrier so that the refill DMA keeps flying across barriers
// (a __syncthreads() would drain it).  NS is kept as a template parameter for the launcher's LDS sizing only (= 2).
// DET (gemm_det_kernel, the deterministic mode): the f32 atomics of split-K outputs and of the fused bias gradient become plain
// stores into per-problem workspace slabs - p.partial = [split][M][N] (dense rows of N), p.ln_part = [split][M] - that
// launch_gemm's fixed-order reduce (det_reduce_kernel) adds onto C / rowsum.  Problems whose outputs are stored (split_k == 1) are
// stored as in the default kernel.
template <int BM, int BN, bool AT, bool BT, int NS, int LB = 2, bool EARLY_ = true>
__global__ __launch_bounds__(256, LB) void gemm_kernel(const GemmGroup g) {
    constexpr bool DET = false;
#include "gemm_kernel_body.inc"
}
template <int BM, int BN, bool AT, bool BT>
__global__ __launch_bounds__(256, 2) void gemm_det_kernel(const GemmGroup g) {
    constexpr bool DET = true, EARLY_ = true;
#include "gemm_kernel_body.inc"
}

// The gated residual product (EPI_RESID_GATE, dropgate.h): the same K loop, NT operands, one epilogue.  An instantiation of its own,
// so that the kernels above stay what they are for every context that has no gate switched on.
template <int BM, int BN>
__global__ __launch_bounds__(256, 2) void gemm_gate_kernel(const GemmGroup g, const Gate gate) {
    constexpr bool DET = false, EARLY_ = true, AT = false, BT = false;
#define BVC_BODY_GATE 1
#include "gemm_kernel_body.inc"
#undef BVC_BODY_GATE
}

// ------------------------------------------------------------------ deterministic mode: workspace and fixed-order reduce
// One pass over the slabs a gemm_det_kernel / gemm8_kernel<.., 6> launch wrote: C[m][n] = C[m][n] + slab[0][m][n] + slab[1][m][n] + ...
// (left to right, split order) for the problems whose outputs were split or accumulating, rowsum[m] = rowsum[m] + rslab[0][m] + ... for
// those with a fused bias gradient.  Four consecutive columns per thread; the work items of the group's problems are concatenated.
struct DetReduce {
    int nprob;
    long long start[kMaxGroup + 1];     // first work item of problem i: its M N / 4 output quads, then (if rowsum) its M rows
    float* C[kMaxGroup]; const float* slab[kMaxGroup]; float* rowsum[kMaxGroup]; const float* rslab[kMaxGroup];
    int M[kMaxGroup], N[kMaxGroup], ldc[kMaxGroup], S[kMaxGroup];
};

__global__ __launch_bounds__(256) void det_reduce_kernel(const DetReduce r) {
    const long long w = (long long)blockIdx.x * 256 + threadIdx.x;
    if (w >= r.start[r.nprob]) return;
    int i = 0;
#pragma unroll
    for (int q = 1; q < kMaxGroup; ++q)
        if (q < r.nprob && w >= r.start[q]) i = q;
    const long long j = w - r.start[i];
    const int M = r.M[i], N = r.N[i], S = r.S[i];
    const long long quads = r.C[i] ? (long long)M * (N / 4) : 0;
    if (j < quads) {
        const int m = (int)(j / (N / 4)), n = (int)(j % (N / 4)) * 4;
        f32x4* c = reinterpret_cast<f32x4*>(r.C[i] + (size_t)m * r.ldc[i] + n);
        const float* s = r.slab[i] + (size_t)m * N + n;
        f32x4 v = *c;
        for (int k = 0; k < S; ++k) v += *reinterpret_cast<const f32x4*>(s + (size_t)k * M * N);
        *c = v;
    } else {
        const int m = (int)(j - quads);
        float v = r.rowsum[i][m];
        for (int k = 0; k < S; ++k) v += r.rslab[i][(size_t)k * M + m];
        r.rowsum[i][m] = v;
    }
}

namespace {
struct DetBuf { int dev; hipStream_t stream; float* ptr; size_t floats; };
std::mutex& det_mutex() { static std::mutex m; return m; }
std::vector<DetBuf>& det_bufs() { static std::vector<DetBuf> v; return v; }
}  // namespace

float* det_scratch(size_t floats, hipStream_t stream) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) { set_error("det_scratch: hipGetDevice failed"); return nullptr; }
    std::lock_guard<std::mutex> lock(det_mutex());
    for (DetBuf& b : det_bufs()) {
        if (b.dev != dev || b.stream != stream) continue;
        if (b.floats >= floats) return b.ptr;
        // grow: the stream's earlier kernels may still read the old buffer
        if (hipStreamSynchronize(stream) != hipSuccess || hipFree(b.ptr) != hipSuccess) {
            set_error("det_scratch: releasing the old workspace failed");
            return nullptr;
        }
        const size_t want = std::max(floats, b.floats + b.floats / 2);
        b.ptr = nullptr; b.floats = 0;
        if (hipMalloc(&b.ptr, want * sizeof(float)) != hipSuccess) {
            set_error("det_scratch: hipMalloc of %zu bytes failed", want * sizeof(float));
            b.ptr = nullptr;
            return nullptr;
        }
        b.floats = want;
        return b.ptr;
    }
    DetBuf b{dev, stream, nullptr, floats};
    if (hipMalloc(&b.ptr, floats * sizeof(float)) != hipSuccess) {
        set_error("det_scratch: hipMalloc of %zu bytes failed", floats * sizeof(float));
        return nullptr;
    }
    det_bufs().push_back(b);
    return b.ptr;
}

int det_scratch_release() {
    int dev = 0;
    BVC_CHECK_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(det_mutex());
    BVC_CHECK_HIP(hipDeviceSynchronize());      // kernels of any stream may still read them
    std::vector<DetBuf>& v = det_bufs();
    for (size_t i = 0; i < v.size();) {
        if (v[i].dev != dev) { ++i; continue; }
        BVC_CHECK_HIP(hipFree(v[i].ptr));
        v.erase(v.begin() + i);
    }
    return BVC_OK;
}

size_t det_scratch_bytes() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    std::lock_guard<std::mutex> lock(det_mutex());
    size_t n = 0;
    for (const DetBuf& b : det_bufs())
        if (b.dev == dev) n += b.floats * sizeof(float);
    return n;
}

// ------------------------------------------------------------------ host side
static void tile_dims(int cfg, int& bm, int& bn) {
    if (cfg == 10 || cfg == 11) { bm = 256; bn = cfg == 10 ? 256 : 128; return; }    // gemm8.hip
    if (cfg == 12) { bm = 128; bn = 384; return; }                                     // gemm8.hip, weight gradients of 384-multiples
    if (cfg == 14) { bm = 128; bn = 256; return; }                                     // gemm_pp.hip: 128 x 256 units, the two wave rows take turns
    bm = cfg == 2 ? 64 : 128;
    bn = cfg == 0 ? 128 : 64;
}

static int tiles_for(const GemmProblem& p, int cfg) {
    int bm, bn;
    tile_dims(cfg, bm, bn);
    return ((p.M + bm - 1) / bm) * ((p.N + bn - 1) / bn);
}

// Can the LayerNorm next to a Linear with N output columns ride in that product's epilogue (EPI_RESID_LN / EPI_DLN)?  Full rows in one
// 128 x 384 tile, whole-row offsets inside 32 bits.
bool gemm_row_ln_ok(int M, int N, int K) { return N == 384 && K % 64 == 0 && K >= 128 && M > 0 && (double)M * 1536.0 < 4294000000.0; }

int gemm_pick_tile(const GemmProblem* probs, int nprob, int tile_cfg) {
    if (tile_cfg == 6 || tile_cfg == 7) return tile_cfg - 6;     // the persistent kernel: 128x128 / 128x64 tiles
    if (tile_cfg == 9) return 0;                                  // persistent 128x128 with deferred stores
    if (tile_cfg >= 10 && tile_cfg <= 12) return tile_cfg;        // gemm8.hip: 256x256 / 256x128 / 128x384
    if (tile_cfg == 14) return tile_cfg;                          // gemm_pp.hip
    if (tile_cfg >= 15 && tile_cfg <= 18) return 0;               // gemm_as.hip: 128 x 128 output tiles
    if (tile_cfg >= 0) return tile_cfg;
    // Measured on MI355X (profiles/r01_b_microbench.json): a workgroup's speed is set by its L2->LDS fill
    // rate (~70 GB/s per CU), so the big tile (64 FLOP/B) wins once it alone covers the 256 CUs ~1.5x;
    // below that, more and smaller workgroups win.  Narrow outputs (N <= 384) prefer 128x64 (3 workgroups/CU).
    int t0 = 0, t1 = 0, nmax = 0;
    for (int i = 0; i < nprob; ++i) {
        t0 += tiles_for(probs[i], 0) * probs[i].split_k;
        t1 += tiles_for(probs[i], 1) * probs[i].split_k;
        nmax = probs[i].N > nmax ? probs[i].N : nmax;
    }
    // ... unless there are at least two full rounds of 128x128 tiles anyway (B >= ~40 decoder shapes): then the big tile is as
    // fast at K = 384 and 15 % faster at K = 1536 (profiles/r01_e_gemm_ksweep_b64.txt, N = 384 rows), and it can be chained
    if (nmax <= 384) return t0 >= 1024 ? 0 : (t1 >= 256 ? 1 : 2);
    if (t0 >= 400) return 0;
    if (t1 >= 400) return 1;
    return 2;
}

// Column tiles per panel for the kernel's tile walk (see gemm_kernel).  Model: an XCD owns rows_x = tiles_m / 8 tile rows of
// the problem; with panels of G column tiles the A rows are fetched once per panel, and the B panel is fetched once if it fits
// ~2 MiB of the L2 and otherwise once per resident wave of 64 workgroups.  Candidates: no panels, or the widest panel that fits.
static int pick_panel(const GemmProblem& p, int cfg, GemmLayout layout) {
    if (BVC_EXP_ENV("BVC_GEMM_LEGACY_WALK") != nullptr) return 0;     // experiments build: read per launch for same-process A/Bs
    if (const char* pe = BVC_EXP_ENV("BVC_GEMM_PANEL")) {             // experiments build: force the panel width (A/B of the walk model)
        const int tn = (p.N + (cfg == 10 ? 256 : 128) - 1) / (cfg == 10 ? 256 : 128), gq = atoi(pe);
        if (layout != GEMM_TN && gq > 0) return gq < tn ? gq : tn;
    }
    // Same-box A/B at B=64 (profiles/r01_e_walk_ab_b64.txt): the panel walk is worth +5 % on the encoder fc1 shape and is
    // neutral elsewhere for NT / NN; the split-K weight-gradient launches are 2-10 % FASTER with the legacy walk (splits
    // fastest, short side first) although it fetches more - the Infinity Cache absorbs the re-reads - so TN keeps it.
    if (layout == GEMM_TN) return 0;
    int bm, bn;
    tile_dims(cfg, bm, bn);
    const int tiles_m = (p.M + bm - 1) / bm, tiles_n = (p.N + bn - 1) / bn;
    const double kper = (double)((p.K + p.split_k - 1) / p.split_k);
    const double a_slab = bm * kper * 2.0, b_slab = bn * kper * 2.0, cap = 2.0 * 1024 * 1024;
    const double rows_x = tiles_m / 8.0 > 1.0 ? tiles_m / 8.0 : 1.0;
    auto cost = [&](int G) {
        const double npan = (double)((tiles_n + G - 1) / G);
        const double waves = rows_x * G / 64.0 > 1.0 ? rows_x * G / 64.0 : 1.0;
        return rows_x * a_slab * npan + tiles_n * b_slab * (G * b_slab <= cap ? 1.0 : waves);
    };
    int gmax = (int)(cap / b_slab);
    if ((cfg == 10 || cfg == 11) && gmax < 2) {
        // Long K on the one-workgroup-per-CU kernel (round 4): not even two column tiles' B slabs fit the L2 budget, so no panel is
        // kept across rounds whatever G is - what counts is the set of tiles RESIDENT on the XCD (32 workgroups that started together
        // and advance along K in step): with G = 1 they are 32 row tiles of one column, 33 distinct operand tiles per K step for 64
        // fetched - rocprofv3 measures an L2 hit rate of 0.485 on the 8192^3 square (profiles/r04_k_pmc_mem_g8.txt) and half of all
        // fills cross the fabric.  A square-ish resident set (G = 6: 5.3 x 6 tiles, 11.3 distinct per 64 fetched) brings the square
        // from 907 to 742 us = 1.48 PFLOP/s (profiles/r04_k_panel_ab.txt); the step's K >= 1536 products (tiles_n = 3) are neutral.
        const int gq = cfg == 10 ? 6 : 8;
        return gq < tiles_n ? gq : tiles_n;
    }
    if (gmax < 1) gmax = 1;
    if (gmax >= tiles_n) return tiles_n;
    const int npan = (tiles_n + gmax - 1) / gmax;
    const int G = (tiles_n + npan - 1) / npan;
    return cost(G) < cost(tiles_n) ? G : tiles_n;
}

static int pick_gemm8(const GemmProblem* probs, int nprob, GemmLayout layout);
// (loss partials are written per tile of the kernel that launch_gemm picks for an NT problem: the same selection, gemm8 included)
int gemm_num_tiles(const GemmProblem& p, int tile_cfg) {
    if (tile_cfg < 0) {
        const int g8 = pick_gemm8(&p, 1, GEMM_NT);
        if (g8 > 0) tile_cfg = g8;
    }
    return tiles_for(p, gemm_pick_tile(&p, 1, tile_cfg));
}

template <int BM, int BN, bool AT, bool BT, int NS, int LB = 2, bool EARLY = true>
static int launch_one(const GemmGroup& g, int nblocks, hipStream_t stream) {
    constexpr size_t lds = (size_t)NS * (BM + BN) * 64 * 2;
    if (dry_run().on) {
        snprintf(dry_run().name, sizeof(dry_run().name), "bvc::gemm_kernel<%d, %d, %s, %s, %d, %d, %s>", BM, BN, AT ? "true" : "false",
                 BT ? "true" : "false", NS, LB, EARLY ? "true" : "false");
        return BVC_OK;
    }
    static bool attr_set = false;   // > 64 KiB of dynamic LDS needs the attribute once per kernel
    if (lds > 65536 && !attr_set) {
        BVC_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_kernel<BM, BN, AT, BT, NS, LB, EARLY>),
                                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        attr_set = true;
    }
    hipLaunchKernelGGL((gemm_kernel<BM, BN, AT, BT, NS, LB, EARLY>), dim3(nblocks), dim3(256), lds, stream, g);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

// the deterministic instantiations (DET = true) of the 128 x 128 / 128 x 64 / 64 x 64 kernel: early-refill K loop, two LDS slots
template <int BM, int BN, bool AT, bool BT>
static int launch_det_one(const GemmGroup& g, int nblocks, hipStream_t stream) {
    constexpr size_t lds = (size_t)2 * (BM + BN) * 64 * 2;
    static_assert(lds <= 65536, "gemm_det_kernel: dynamic LDS above 64 KiB would need the attribute");
    if (dry_run().on) {
        snprintf(dry_run().name, sizeof(dry_run().name), "bvc::gemm_det_kernel<%d, %d, %s, %s>", BM, BN, AT ? "true" : "false", BT ? "true" : "false");
        return BVC_OK;
    }
    hipLaunchKernelGGL((gemm_det_kernel<BM, BN, AT, BT>), dim3(nblocks), dim3(256), lds, stream, g);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

template <int BM, int BN>
static int launch_det_cfg(const GemmGroup& g, GemmLayout layout, int nblocks, hipStream_t stream) {
    switch (layout) {
        case GEMM_NT: return launch_det_one<BM, BN, false, false>(g, nblocks, stream);
        case GEMM_NN: return launch_det_one<BM, BN, false, true>(g, nblocks, stream);
        case GEMM_TN: return launch_det_one<BM, BN, true, true>(g, nblocks, stream);
        default: set_error("launch_gemm: bad layout %d", (int)layout); return BVC_ERR_INVALID;
    }
}

template <int BM, int BN, int NS>
static int launch_cfg(const GemmGroup& g, GemmLayout layout, int nblocks, hipStream_t stream) {
    switch (layout) {
        case GEMM_NT: return launch_one<BM, BN, false, false, NS>(g, nblocks, stream);
        case GEMM_NN: return launch_one<BM, BN, false, true, NS>(g, nblocks, stream);
        case GEMM_TN: return launch_one<BM, BN, true, true, NS>(g, nblocks, stream);
        default: set_error("launch_gemm: bad layout %d", (int)layout); return BVC_ERR_INVALID;
    }
}

template <int BM, int BN>
static int launch_stages(const GemmGroup& g, GemmLayout layout, int stages, int nblocks, hipStream_t stream) {
    // experiment hooks (same-run A/B; box-to-box variance on the pool is +-40 %): stages 3 = AGPR-form MFMA for TN (measured
    // 5-25 % slower), stages 4 = the other K-loop variant for the layout
    if (stages == 3 && layout == GEMM_TN) return launch_one<BM, BN, true, true, 2, 1>(g, nblocks, stream);
    if (stages == 4) {
        if (layout == GEMM_NT) return launch_one<BM, BN, false, false, 2, 2, false>(g, nblocks, stream);
        if (layout == GEMM_NN) return launch_one<BM, BN, false, true, 2, 2, false>(g, nblocks, stream);
        return launch_one<BM, BN, true, true, 2, 2, false>(g, nblocks, stream);
    }
    return launch_cfg<BM, BN, 2>(g, layout, nblocks, stream);
}

// The K loop keeps two K-steps of LDS-DMA in flight out of two LDS slots (see gemm_kernel); deeper rings were measured
// slower (they cost the second resident workgroup per CU), so `stages` is accepted for API stability and ignored.
int gemm_pick_stages(int, GemmLayout, int, int stages) { return (stages == 3 || stages == 4) ? stages : 2; }

int launch_gemm_big_nt(const GemmProblem& p, int cfg, hipStream_t stream);   // experiments/gemm_big.hip (tile configs 3-5, experiments build only)
// gemm_persist.hip; returns 1 when the problem is not eligible.  defer: 0 = stores in the epilogue, 1 = deferred where possible,
// 2 = deferred or not at all (tile config 9, tests)
int launch_gemm_persist(const GemmGroup& g, GemmLayout layout, int cfg, hipStream_t stream, int defer);
// gemm8.hip: 256 x bn tiles, one 512-thread workgroup per CU; returns 1 when the group is not eligible.  det: the deterministic
// weight-gradient instantiation (epilogue class 6: slabs instead of atomics, see launch_gemm)
int launch_gemm8(const GemmGroup& g, GemmLayout layout, int bn, hipStream_t stream, bool det = false);
// gemm_as.hip: A-stationary kernel for K = 384 products with bf16 outputs (tile configs 15 / 16); returns 1 when the problem is not eligible
int launch_gemm_as(const GemmProblem& p, GemmLayout layout, int variant, hipStream_t stream);
bool gemm_as_ok(const GemmProblem& p, GemmLayout layout);
// experiments/gemm_pp.hip (experiments build only): 128 x 256 units, K loop of one wave row under the epilogue of the other;
// built and measured in round 4 (profiles/r04_d_*): correct, bit-identical, and NOT faster - see its header
int launch_gemm_pp(const GemmGroup& g, GemmLayout layout, hipStream_t stream);

// Which products go to the 256-row persistent kernel (gemm8.hip) when the caller leaves the tile choice open.  Fitted to the
// same-process A/Bs of every product of the step at 16, 64 and 256 clips (profiles/r02_e_gemm8_ab_b{16,64,256}.txt, tools/ab/gemm8_ab.py):
// its K loop runs ~1.2 PFLOP/s against ~0.8 for the 128 x 128 kernels, but it is ONE workgroup per CU - a launch needs about two
// full rounds of tiles and ~45 GFLOP to amortise prologue and tail, and an epilogue is not hidden by a second resident workgroup:
//   * 256 x 256: plain bf16-output epilogues (BF16 / GELU / RELU) and f32-output ones (residual, positional, plain) with >= 448
//     tiles whose last column tile is at least 85 % full (encoder qkv / fc1 / dX at >= 64 clips, decoder qkv / fc1: -20 ... -27 %
//     at 256 clips, -5 ... -10 % at 64; encoder proj / fc2 at 256 clips);
//   * 256 x 128: input-gradient products (NN, bf16 out) and residual products (f32 + residual) with K >= 1024 and >= 224 tiles
//     when the 256-wide tile would be half empty (decoder N = 384: dX-fc1, dX-qkv, fc2);
//   * never: GELU' / ReLU' (their side-input epilogue still parks through LDS and drains the prefetch: no gain measured),
//     launches below 45 GFLOP (at 16 clips gemm8 loses 5-50 % on every product).
// Returns 10 / 11 (tile configs) or -1.
static int pick_gemm8(const GemmProblem* probs, int nprob, GemmLayout layout) {
    const int mode = options().gemm8;
    if (mode < 0 || nprob != 1 || layout == GEMM_TN) return -1;
    const GemmProblem& p = probs[0];
    if (p.split_k != 1 || p.K % 64 != 0) return -1;
    if (p.a_bytes >= 0x80000000u || p.b_bytes >= 0x80000000u) return -1;    // gemm8 addresses operands below 2 GiB (its out-of-range sentinel)
    // (the gated epilogues - GELU' / ReLU' - joined once the forward saved gelu' itself: one multiply per element instead of ~14
    //  vector instructions nothing hid on this kernel; decoder dX-fc2 at 256 clips 769 vs 878 us - profiles/r02_i_gelu_grad_saved.txt)
    const bool gated = p.epi == EPI_DGELU || p.epi == EPI_DRELU;
    const bool bf = p.epi == EPI_BF16 || p.epi == EPI_GELU || p.epi == EPI_RELU;
    // f32 out (+ f32 side input); the head + MSE product (f32 labels in, bf16 difference out, per-tile loss partials) rides the same
    // class since round 3: 868 vs 1120 us at 256 clips, 256 vs 303 at 64 (tools/debug/head_loss_ab.py)
    const bool resid = (p.epi == EPI_RESID || p.epi == EPI_POS || p.epi == EPI_F32 || p.epi == EPI_LOSS) && layout == GEMM_NT;
    if (!bf && !resid && !gated) return -1;
    const int tm = (p.M + 255) / 256, tn256 = (p.N + 255) / 256, tn128 = (p.N + 127) / 128;
    // the register-epilogue class keeps the tile-padded bias vector in 32 KiB of LDS (launch_gemm8 refuses wider outputs)
    const bool fits256 = !bf || (size_t)tn256 * 256 * 4 <= 32768, fits128 = !bf || (size_t)tn128 * 128 * 4 <= 32768;
    if (mode > 0) {      // forced (tests, A/B tools): the widest tile the output fills at least half of
        if (fits256 && (gated || p.N > 128)) return 10;
        return fits128 && !gated ? 11 : -1;
    }
    if (2.0 * p.M * p.N * p.K < 45e9) return -1;
    const bool full256 = (double)p.N >= 0.85 * 256.0 * tn256;
    // (the f32 class runs its side inputs in four passes on 256 x 256 tiles: encoder proj / fc2 / patch embedding at 256 clips
    //  -10 / -21 / -17 %, a loss below 448 tiles - profiles/r02_g_gemm8_resid_ab.txt)
    if (full256 && fits256 && tm * tn256 >= 448) return 10;
    if (gated) return -1;                   // 256 x 128 tiles lose on them at every size measured
    if (p.epi != EPI_LOSS && fits128 && (bf ? layout == GEMM_NN : p.N <= 384) && p.K >= 1024 && tm * tn128 >= (resid ? 1024 : 224)) return 11;
    return -1;
}

template <int BM, int BN>
static int launch_gate_one(const GemmGroup& g, const Gate& gate, int nblocks, hipStream_t stream) {
    constexpr size_t lds = (size_t)2 * (BM + BN) * 64 * 2;
    static_assert(lds <= 65536, "gemm_gate_kernel: dynamic LDS above 64 KiB would need the attribute");
    if (dry_run().on) {
        snprintf(dry_run().name, sizeof(dry_run().name), "bvc::gemm_gate_kernel<%d, %d>", BM, BN);
        return BVC_OK;
    }
    hipLaunchKernelGGL((gemm_gate_kernel<BM, BN>), dim3(nblocks), dim3(256), lds, stream, g, gate);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

int launch_gemm_gate(const GemmProblem& p0, const Gate& gate, int tile_cfg, hipStream_t stream) {
    GemmProblem p = p0;
    p.epi = EPI_RESID_GATE;
    BVC_REQUIRE(tile_cfg >= -1 && tile_cfg <= 2, "launch_gemm_gate: tile config %d (the gated epilogue runs on tile configs 0 / 1 / 2)", tile_cfg);
    BVC_REQUIRE(p.M > 0 && p.N > 0 && p.K > 0, "launch_gemm_gate: empty problem (%d,%d,%d)", p.M, p.N, p.K);
    BVC_REQUIRE(p.N % 8 == 0 && p.K % 64 == 0, "launch_gemm_gate: N=%d must be a multiple of 8 and K=%d of 64", p.N, p.K);
    BVC_REQUIRE(p.lda % 8 == 0 && p.ldb % 8 == 0 && p.ldc % 8 == 0, "launch_gemm_gate: leading dims must be multiples of 8");
    BVC_REQUIRE(p.split_k == 1, "launch_gemm_gate: split_k must be 1");
    BVC_REQUIRE(p.A && p.B && p.C && p.resid, "launch_gemm_gate: null operand, output or residual");
    BVC_REQUIRE(gate.rows >= 1 && (double)p.M * p.N < 4398046511104.0, "launch_gemm_gate: bad gate (rows per sample %d) or more than 2^42 elements", gate.rows);
    const int cfg = gemm_pick_tile(&p, 1, tile_cfg);
    GemmGroup g;
    g.nprob = 1;
    g.bal_units = g.bal_lb = g.bal_tiles = 0;
    g.accum = 0;
    g.stagger = 0;
    g.dbg = 0;
    const int total = tiles_for(p, cfg);
    for (int i = 0; i < kMaxGroup; ++i) { g.prob[i] = p; g.panel[i] = pick_panel(p, cfg, GEMM_NT); g.tile_start[i] = i == 0 ? 0 : total; }
    g.tile_start[kMaxGroup] = total;
    switch (cfg) {
        case 0: return launch_gate_one<128, 128>(g, gate, total, stream);
        case 1: return launch_gate_one<128, 64>(g, gate, total, stream);
        default: return launch_gate_one<64, 64>(g, gate, total, stream);
    }
}

int launch_gemm(const GemmProblem* probs, int nprob, GemmLayout layout, int tile_cfg, hipStream_t stream, int stages) {
    BVC_REQUIRE(nprob >= 1 && nprob <= kMaxGroup, "launch_gemm: nprob %d out of range", nprob);
    for (int i = 0; i < nprob; ++i)
        BVC_REQUIRE(probs[i].epi != EPI_RESID_GATE, "launch_gemm: BVC_EPI_RESID_GATE needs its gate (bvc_op_gemm_gate / a context with bvc_*_set_drop)");
    static thread_local bool skip_g8 = false;      // set while an auto-picked gemm8 launch that turned the problem down is re-planned
    bool auto_g8 = false;
    if (probs[0].epi == EPI_RESID_LN || probs[0].epi == EPI_DLN) {
        // LayerNorm fused into a 384-wide product: exists on the full-row tile of gemm8.hip only (the caller asks gemm_row_ln_ok first)
        const GemmProblem& p = probs[0];
        BVC_REQUIRE(nprob == 1 && (tile_cfg < 0 || tile_cfg == 12), "launch_gemm: the LayerNorm epilogues take one problem on tile config 12");
        BVC_REQUIRE(gemm_row_ln_ok(p.M, p.N, p.K) && p.ldc == p.N && p.split_k == 1 && p.a_bytes < 0x80000000u && p.b_bytes < 0x80000000u,
                    "launch_gemm: the LayerNorm epilogues need N == ldc == 384, K %% 64 == 0, operands below 2 GiB (M=%d N=%d K=%d)", p.M, p.N, p.K);
        BVC_REQUIRE(p.C && p.C2 && p.ln_mean && p.ln_rstd && p.ln_gamma, "launch_gemm: LayerNorm epilogue with a null output / statistic / scale");
        if (p.epi == EPI_RESID_LN) BVC_REQUIRE(layout == GEMM_NT && p.resid && p.ln_beta, "launch_gemm: RESID_LN is an NT product with a residual and a LayerNorm bias");
        if (p.epi == EPI_DLN) BVC_REQUIRE(layout == GEMM_NN && p.ln_x && p.ln_part && p.ln_dgamma && p.ln_dbeta, "launch_gemm: DLN is an NN product with the LayerNorm input, partial scratch and parameter gradients");
        // the segment map shifts the base of the mapped side array's buffer descriptor (gemm8.hip): a bad map would defeat its range check
        if (p.seg_rows != 0)
            BVC_REQUIRE(p.seg_rows > 0 && p.seg_rows % 128 == 0 && p.M % p.seg_rows == 0 && p.seg_off >= 0 && p.seg_stride > 0 &&
                            (long long)p.seg_off + p.seg_rows <= (long long)p.seg_stride,
                        "launch_gemm: bad segment map (seg_rows %d: a multiple of 128 that divides M = %d; seg_off %d + seg_rows <= seg_stride %d)",
                        p.seg_rows, p.M, p.seg_off, p.seg_stride);
        tile_cfg = 12;
    } else {
        for (int i = 0; i < nprob; ++i)
            BVC_REQUIRE(probs[i].seg_rows == 0, "launch_gemm: a segment map (seg_rows %d) exists for BVC_EPI_RESID_LN / BVC_EPI_DLN only", probs[i].seg_rows);
    }
    // K = 384 products with a plain bf16 output (decoder / predictor qkv): the A-stationary kernel (gemm_as.hip), whose epilogue runs under
    // the next N tile's MFMAs.  Same-process A/B against the kernels picked below (profiles/r05_l_as_ab_batches.txt, r05_i_as_ab_b256.txt):
    // decoder qkv -6.5 % at 16 clips, -10 % at 32 ... 128, -11.5 % at 256.  Its GELU form does not win (the GELU arithmetic beside the
    // MFMAs costs more than it hides: +13 ... +22 % overlapped, -6 ... +5 % behind the tile) and stays a tile config for A/Bs.
    if (tile_cfg < 0 && stages < 0 && nprob == 1 && options().gemm8 >= 0 && probs[0].epi == EPI_BF16 && gemm_as_ok(probs[0], layout) &&
        (options().gemm8 > 0 || probs[0].M >= 16384) && BVC_EXP_ENV("BVC_GEMM_NO_AS") == nullptr)
        return launch_gemm_as(probs[0], layout, 0, stream);
    if (tile_cfg < 0 && stages < 0 && !skip_g8) {
        const int g8 = pick_gemm8(probs, nprob, layout);
        if (g8 > 0) { tile_cfg = g8; auto_g8 = true; }
    }
    if (tile_cfg >= 15 && tile_cfg <= 18) {      // gemm_as.hip: A-stationary kernel for K = 384 (16: epilogue behind its own tile; 17 / 18: the same two with late LDS-DMA; A/Bs)
        BVC_REQUIRE(nprob == 1, "launch_gemm: tile configs 15 - 18 take one problem");
        const int rc = launch_gemm_as(probs[0], layout, tile_cfg - 15, stream);
        BVC_REQUIRE(rc != 1, "launch_gemm: tile configs 15 - 18 (A-stationary kernel) take NT products with K = 384, N %% 128 == 0, BF16 / GELU epilogues");
        return rc;
    }
    if ((tile_cfg >= 3 && tile_cfg <= 5) || tile_cfg == 8) {
#ifdef BVC_EXPERIMENTS
        BVC_REQUIRE(nprob == 1 && layout == GEMM_NT, "launch_gemm: tile configs 3-5 (32-deep K steps) are NT, one problem");
        BVC_REQUIRE(!options().deterministic || probs[0].split_k == 1, "launch_gemm: tile configs 3-5 have no deterministic split-K form");
        return launch_gemm_big_nt(probs[0], tile_cfg, stream);
#else
        BVC_REQUIRE(false, "launch_gemm: tile configs 3-5 / 8 exist only in a -DBVC_EXPERIMENTS build (csrc/experiments/gemm_big.hip)");
#endif
    }
    // tile config 13 = tile config 10 (256 x 256, gemm8.hip) for weight gradients whose outputs are ACCUMULATED: C += dY^T X by f32
    // atomics whether K is split or not (C pre-zeroed, as for split_k > 1).  An unsplit group that fills only part of the chip can
    // then take the balanced walk (plan_balance in gemm8.hip); plan_dw returns it for such groups.
    bool accum = false;
    if (tile_cfg == 13) {
        BVC_REQUIRE(layout == GEMM_TN, "launch_gemm: tile config 13 (accumulating 256 x 256 tiles) is for weight gradients (TN)");
        for (int i = 0; i < nprob; ++i) BVC_REQUIRE(probs[i].epi == EPI_F32, "launch_gemm: tile config 13 takes plain f32 outputs");
        accum = true;
        tile_cfg = 10;
    }
    const int cfg = gemm_pick_tile(probs, nprob, tile_cfg);
    GemmGroup g;
    g.nprob = nprob;
    g.bal_units = g.bal_lb = g.bal_tiles = 0;
    g.accum = accum ? 1 : 0;
    g.stagger = 0;
    {
        const char* e = BVC_EXP_ENV("BVC_GEMM_DEBUG");
        g.dbg = e ? atoi(e) : 0;
    }
    int total = 0;
    for (int i = 0; i < nprob; ++i) {
        const GemmProblem& p = probs[i];
        BVC_REQUIRE(p.M > 0 && p.N > 0 && p.K > 0, "launch_gemm: empty problem %d (%d,%d,%d)", i, p.M, p.N, p.K);
        BVC_REQUIRE(p.N % 8 == 0, "launch_gemm: N=%d must be a multiple of 8", p.N);
        BVC_REQUIRE(p.lda % 8 == 0 && p.ldb % 8 == 0 && p.ldc % 8 == 0, "launch_gemm: leading dims must be multiples of 8");
        if (layout != GEMM_TN) BVC_REQUIRE(p.K % 64 == 0, "launch_gemm: K=%d must be a multiple of 64 for k-contiguous operands", p.K);
        if (layout == GEMM_TN) BVC_REQUIRE(p.M % 8 == 0, "launch_gemm: TN needs M %% 8 == 0 (M=%d)", p.M);
        if (layout == GEMM_TN)
            BVC_REQUIRE(tn_tail_ok(p.K, p.lda) && tn_tail_ok(p.K, p.ldb),
                        "launch_gemm: TN with K=%d (no multiple of 64), lda=%d, ldb=%d: the 32-bit byte offsets of the rows past K in the last K step "
                        "would wrap past 4 GiB into the operand instead of reading as zero", p.K, p.lda, p.ldb);
        BVC_REQUIRE(p.split_k >= 1, "launch_gemm: split_k must be >= 1");
        if (p.rowsum) BVC_REQUIRE(layout == GEMM_TN, "launch_gemm: rowsum (bias gradient) is fused into TN products only");
        if (p.split_k > 1)
            BVC_REQUIRE(p.epi == EPI_F32 || (p.epi == EPI_RESID && p.resid == p.C),
                        "launch_gemm: split_k needs an accumulating f32 epilogue");
        g.prob[i] = p;
        g.panel[i] = pick_panel(p, cfg, layout);
        if (cfg >= 10 && cfg <= 12 && layout == GEMM_TN && BVC_EXP_ENV("BVC_G8_TN_LEGACY_WALK") == nullptr) {
            // weight gradients on the persistent kernel: K splits SLOWEST, tiles row-major inside a split.  An XCD's ~32 resident
            // units are then the tiles of one or two K ranges of one problem, which share their dY / X slices through its L2; with
            // the splits fastest (the 128 x 128 kernel's walk) neighbours share nothing and every unit streams its own slices
            // from HBM: 15.6 GB per decoder layer at 256 clips for 4.5 GB of operands (profiles/r02_f_dw_walk_ab.txt).
            int bm, bn;
            tile_dims(cfg, bm, bn);
            g.panel[i] = (p.N + bn - 1) / bn;
            if (BVC_EXP_ENV("BVC_G8_TN_SHORT_FAST") != nullptr) g.panel[i] = -1;
        }
        g.tile_start[i] = total;
        total += tiles_for(p, cfg) * p.split_k;
    }
    g.tile_start[nprob] = total;
    for (int i = nprob; i < kMaxGroup; ++i) { g.prob[i] = probs[0]; g.panel[i] = g.panel[0]; g.tile_start[i + 1] = total; }
    if (options().deterministic) {
        // Deterministic mode: the problems whose results the default kernels accumulate by f32 atomics in scheduling order (split or
        // accumulating outputs, fused bias gradients) run on the DET instantiations, which store every (tile, split) partial into a
        // workspace slab (p.partial = [split][M][N], p.ln_part = [split][M]); det_reduce_kernel then adds the slabs onto C / rowsum in
        // split order.  The reduce is enqueued here, before the caller can report the gradient range finished (bucket callbacks).
        DetReduce r;
        memset(&r, 0, sizeof(r));
        r.nprob = nprob;
        size_t floats = 0;
        long long items = 0;
        size_t at[kMaxGroup][2];
        for (int i = 0; i < nprob; ++i) {
            const GemmProblem& p = probs[i];
            const bool slab = p.split_k > 1 || accum;
            r.start[i] = items;
            r.M[i] = p.M; r.N[i] = p.N; r.ldc[i] = p.ldc; r.S[i] = p.split_k;
            at[i][0] = at[i][1] = (size_t)-1;
            if (slab) {
                BVC_REQUIRE(p.ldc % 4 == 0, "launch_gemm: deterministic reduce needs ldc %% 4 == 0");
                at[i][0] = floats; floats += ((size_t)p.split_k * p.M * p.N + 63) & ~(size_t)63;
                r.C[i] = reinterpret_cast<float*>(p.C);
                items += (long long)p.M * (p.N / 4);
            }
            if (p.rowsum) {
                at[i][1] = floats; floats += ((size_t)p.split_k * p.M + 63) & ~(size_t)63;
                r.rowsum[i] = p.rowsum;
                items += p.M;
            }
        }
        r.start[nprob] = items;
        if (items > 0) {
            BVC_REQUIRE(cfg <= 2 || (cfg >= 10 && cfg <= 12),
                        "launch_gemm: tile config %d has no deterministic form (split / accumulating outputs, fused bias gradients)", cfg);
            float* ws = nullptr;
            if (!dry_run().on) {
                ws = det_scratch(floats, stream);
                if (!ws) return BVC_ERR_HIP;
            }
            for (int i = 0; i < nprob; ++i) {
                if (at[i][0] != (size_t)-1) g.prob[i].partial = ws ? ws + at[i][0] : nullptr;
                if (at[i][1] != (size_t)-1) g.prob[i].ln_part = ws ? ws + at[i][1] : nullptr;
                r.slab[i] = g.prob[i].partial;
                r.rslab[i] = g.prob[i].ln_part;
            }
            int rc;
            if (cfg >= 10) {
                rc = launch_gemm8(g, layout, cfg == 10 ? 256 : cfg == 11 ? 128 : 384, stream, true);
                BVC_REQUIRE(rc != 1, "launch_gemm: tile configs 10 - 12 take split / accumulating / bias-gradient outputs in TN products only");
            } else {
                switch (cfg) {
                    case 0: rc = launch_det_cfg<128, 128>(g, layout, total, stream); break;
                    case 1: rc = launch_det_cfg<128, 64>(g, layout, total, stream); break;
                    default: rc = launch_det_cfg<64, 64>(g, layout, total, stream); break;
                }
            }
            if (rc != BVC_OK || dry_run().on) return rc;
            hipLaunchKernelGGL(det_reduce_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, stream, r);
            BVC_CHECK_HIP(hipGetLastError());
            return BVC_OK;
        }
    }
    if (cfg == 14) {
#ifdef BVC_EXPERIMENTS
        const int rc = launch_gemm_pp(g, layout, stream);
        BVC_REQUIRE(rc != 1, "launch_gemm: tile config 14 (ping-pong kernel) does not take this problem");
        return rc;
#else
        BVC_REQUIRE(false, "launch_gemm: tile config 14 exists only in a -DBVC_EXPERIMENTS build (csrc/experiments/gemm_pp.hip)");
#endif
    }
    if (cfg >= 10 && cfg <= 12) {
        const int rc = launch_gemm8(g, layout, cfg == 10 ? 256 : cfg == 11 ? 128 : 384, stream);
        if (rc == 1 && auto_g8) {     // the selection and the kernel's own eligibility test disagree: never an error for the caller
            skip_g8 = true;
            const int rc2 = launch_gemm(probs, nprob, layout, -1, stream, stages);
            skip_g8 = false;
            return rc2;
        }
        BVC_REQUIRE(rc != 1, "launch_gemm: tile configs 10 - 12 (persistent one-workgroup-per-CU kernel) do not take this problem");
        return rc;
    }
    int kmax = 0;
    for (int i = 0; i < nprob; ++i) kmax = probs[i].K > kmax ? probs[i].K : kmax;
    int ns = gemm_pick_stages(cfg, layout, kmax, stages);
    // One round of 128x128 tiles (the encoder's proj / fc2 / dX-proj at B=64: 480 workgroups): the plain double buffer beat the
    // early-refill loop by 6-11 % for NT and for NN at K <= 768 in the same-process tile sweep (profiles/r01_f_tile_sweep_b64.txt),
    // and tied elsewhere - with every workgroup resident at once there is no second round whose prologue the deeper prefetch hides.
    if (stages < 0 && nprob == 1 && cfg == 0 && total <= 512 && probs[0].split_k == 1 &&
        (layout == GEMM_NT || (layout == GEMM_NN && probs[0].K <= 768)))
        ns = 4;
    // short-K single products with many tile rounds go to the persistent kernel (tile config 6 forces it, for tests);
    // BVC_GEMM_NO_PERSIST=1 keeps them on gemm_kernel (same-process A/B)
    // Same-box A/B at B=64 (profiles/r01_f_persist_ab_b64.txt): 128x128 persistent -12 ... -15 % on every eligible product; the
    // 128x64 form wins only at short K (decoder proj, K=384: -5 %) and LOSES 6-16 % at K >= 1152, where the per-tile kernel's
    // third resident workgroup per CU matters more than the chaining - so it is taken up to K = 512 only.
    const bool auto_persist = tile_cfg < 0 && stages < 3 && g.dbg == 0 && (cfg == 0 || (cfg == 1 && probs[0].K <= 512)) &&
                              BVC_EXP_ENV("BVC_GEMM_NO_PERSIST") == nullptr;
    if (nprob == 1 && (tile_cfg == 6 || tile_cfg == 7 || tile_cfg == 9 || auto_persist)) {
        // deferred stores (gemm_persist.hip) measured on the decoder shapes at B=64 (profiles/r01_f_gemm_ksweep_b64.txt, tile 9 vs 6):
        // GELU' epilogue -8 ... -18 % at K <= 384, -2 % at K = 768; plain bf16 +-0; GELU (two outputs, 253 VGPRs) +8 % slower.
        // So: the GELU' products only.  BVC_GEMM_DEFER=1 / =0 force it on (where possible) / off for A/Bs.
        const char* dv = BVC_EXP_ENV("BVC_GEMM_DEFER");
        const int defer = tile_cfg == 9 ? 2 : tile_cfg >= 0 ? 0 : dv ? (dv[0] == '1' ? 1 : 0) : (probs[0].epi == EPI_DGELU ? 1 : 0);
        const int rc = launch_gemm_persist(g, layout, cfg, stream, defer);
        if (rc != 1) return rc;
        BVC_REQUIRE(tile_cfg < 6, "launch_gemm: tile configs 6 / 7 / 9 (persistent kernels) do not take this problem");
    }
    switch (cfg) {
        case 0: return launch_stages<128, 128>(g, layout, ns, total, stream);
        case 1: return launch_stages<128, 64>(g, layout, ns, total, stream);
        default: return launch_stages<64, 64>(g, layout, ns, total, stream);
    }
}

}  // namespace bvc

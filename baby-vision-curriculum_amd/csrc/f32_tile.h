// The f32 MFMA tile of retrieval.hip, ntxent.hip and xcorr.hip: C [128][128] = A [128][K] . B [128][K]^T, both operands
// contraction-contiguous, every element ONE accumulation chain over d in ascending order on v_mfma_f32_32x32x2_f32 (bit for bit a
// d-ordered fmaf chain starting at 0).  This header is the only place that knows the LDS row format, which lane reads which
// fragment and which accumulator element is which (row, column): the ops built on it promise the same bits for every blocking,
// split and chunking, so a change of the loop has to reach all of them at once.
//
// 256 threads = 4 waves as 2 (A halves, wk) x 2 (B halves, wq); a wave holds 64 x 64 as 2 x 2 accumulators of 32 x 32.  A K step is
// 32 floats: operands global -> registers (the next step's, under the MFMAs) -> LDS (36-float rows, even d in floats 0..15 and odd
// d in 16..31 of a row, so lane (r, h) of the MFMA reads its 16 operands of a step - d = 2 kk + h - as four ds_read_b128,
// conflict-free at a 9-slot row stride).
// The B row is on the lane, the A rows are on the accumulator elements: a lane owns two B rows (j = 0, 1), so what belongs to a B
// row (a threshold, a running maximum) stays in its registers, and a store of one accumulator element by a wave is two runs of
// 32 consecutive floats.
#pragma once
#include "common.h"

namespace bvc {

constexpr int kF32Tile = 128;        // rows of A and of B per tile
constexpr int kF32KStep = 32;        // floats of the contraction per LDS stage
constexpr int kF32Row = 36;          // floats per LDS operand row (32 + 4: ds_read_b128 of 16 rows land on 16 different slots)

// ---------------------------------------------------------------- who holds what
struct F32TileLane { int r, h, wk, wq; };      // lane = r + 32 h, wave = wk + 2 wq
__device__ __forceinline__ F32TileLane f32t_lane(int tid) {
    const int lane = tid & 63, wave = tid >> 6;
    return {lane & 31, lane >> 5, wave & 1, wave >> 1};
}
// acc[i][j][e] = sum_d A[arow][d] B[brow][d],   arow = a0 + wk * 64 + 32 * i + (e & 3) + 8 * (e >> 2) + 4 * h,
// brow = b0 + wq * 64 + 32 * j + r,   for operands whose tile starts at row a0 / b0 (0 gives the row within the tile).
// Macros, not functions: hipcc optimises an inline function on its own before it inlines it, without the caller's knowledge of
// a0 and b0, and the sums then come out associated differently - the instruction streams of nx_fwd_kernel and xc_fwd_kernel
// change (profiles/f32_tile_refactor_report.txt).  L is the F32TileLane of the thread.
#define F32T_AROW(L, a0, i, e) ((a0) + (L).wk * 64 + 32 * (i) + ((e) & 3) + 8 * ((e) >> 2) + 4 * (L).h)
#define F32T_BROW(L, b0, j) ((b0) + (L).wq * 64 + 32 * (j) + (L).r)

// ---------------------------------------------------------------- global -> registers
// 16 floats of 4 rows (rows r0 + 32 m) of a 128-row x 32-float stage: thread t reads floats 4 (t & 7) .. + 3 of row t >> 3.
// Padded operands (a workspace): 16-byte aligned rows, K a multiple of 32, rows past the end repeat the last one (their products
// are never used).
__device__ __forceinline__ void f32t_load(const float* __restrict__ base, int64_t ld, int row0, int rows, int d0, int tid, f32x4 (&v)[4]) {
    const int c = (tid & 7) * 4 + d0, r0 = tid >> 3;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int row = min(row0 + r0 + 32 * m, rows - 1);
        v[m] = *reinterpret_cast<const f32x4*>(base + (int64_t)row * ld + c);
    }
}
// Rows as the caller has them: any stride, any D, VEC when every row is 16-byte aligned.
// No load sits under a per-lane condition (hipcc would branch around each and wait for it before the next): a whole step of
// 16-byte-aligned rows is four unconditional 16-byte loads, chosen by a workgroup-uniform test; everything else - the D tail,
// unaligned rows - is sixteen unconditional 4-byte loads from the column clamped to D - 1 of the same row, zeroed by a select
// (fma(0, 0, acc) = acc: the chain does not see the tail).
template <bool VEC>
__device__ __forceinline__ void f32t_load_raw(const float* __restrict__ base, int64_t ld, int row0, int rows, int d0, int D, int tid,
                                              f32x4 (&v)[4]) {
    const int c = (tid & 7) * 4 + d0, r0 = tid >> 3;
    if (VEC && d0 + kF32KStep <= D) {
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int row = min(row0 + r0 + 32 * m, rows - 1);      // rows past the end repeat the last one (never selected)
            v[m] = *reinterpret_cast<const f32x4*>(base + (int64_t)row * ld + c);
        }
    } else {
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int row = min(row0 + r0 + 32 * m, rows - 1);
            const float* p = base + (int64_t)row * ld;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float x = p[min(c + e, D - 1)];
                v[m][e] = c + e < D ? x : 0.f;
            }
        }
    }
}

// ---------------------------------------------------------------- registers -> LDS -> MFMA
// floats d = 4 c .. 4 c + 3 of a row go to the even-d half at 2 c, 2 c + 1 (d = 4 c, 4 c + 2) and the odd-d half at 16 + 2 c ..
__device__ __forceinline__ void f32t_stage(float* lds, int tid, const f32x4 (&v)[4]) {
    const int c = tid & 7, r0 = tid >> 3;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        float* row = lds + (r0 + 32 * m) * kF32Row;
        *reinterpret_cast<f32x2*>(row + 2 * c) = f32x2{v[m][0], v[m][2]};
        *reinterpret_cast<f32x2*>(row + 16 + 2 * c) = f32x2{v[m][1], v[m][3]};
    }
}

__device__ __forceinline__ void f32t_zero(f32x16 (&acc)[2][2]) {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
}

// one staged K step: eight ds_read_b128 of A and of B, then 64 MFMAs in ascending d.  Takes tid, not the lane's coordinates: with
// those as arguments hipcc orders the fragment addresses differently in every product kernel.
__device__ __forceinline__ void f32t_step(const float* ldsA, const float* ldsB, int tid, f32x16 (&acc)[2][2]) {
    const F32TileLane L = f32t_lane(tid);
    f32x4 fa[2][4], fb[2][4];      // element e of piece m: d = 2 (4 m + e) + h of the step
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            fa[b][m] = *reinterpret_cast<const f32x4*>(ldsA + (L.wk * 64 + 32 * b + L.r) * kF32Row + 16 * L.h + 4 * m);
            fb[b][m] = *reinterpret_cast<const f32x4*>(ldsB + (L.wq * 64 + 32 * b + L.r) * kF32Row + 16 * L.h + 4 * m);
        }
#pragma unroll
    for (int kk = 0; kk < 16; ++kk)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[i][kk >> 2][kk & 3], fb[j][kk >> 2][kk & 3], acc[i][j], 0, 0, 0);
}

// The whole tile over padded operands.  Ends with a barrier: the stages are free on return.
__device__ __forceinline__ void f32t_product(const float* __restrict__ A, int64_t lda, int a0, int arows, const float* __restrict__ B,
                                             int64_t ldb, int b0, int brows, int K, float* ldsA, float* ldsB, int tid, f32x16 (&acc)[2][2]) {
    f32t_zero(acc);
    const int ksteps = K / kF32KStep;
    f32x4 va[4], vb[4];
    f32t_load(A, lda, a0, arows, 0, tid, va);
    f32t_load(B, ldb, b0, brows, 0, tid, vb);
    for (int s = 0; s < ksteps; ++s) {
        f32t_stage(ldsA, tid, va);
        f32t_stage(ldsB, tid, vb);
        __syncthreads();
        if (s + 1 < ksteps) {
            f32t_load(A, lda, a0, arows, (s + 1) * kF32KStep, tid, va);
            f32t_load(B, ldb, b0, brows, (s + 1) * kF32KStep, tid, vb);
        }
        f32t_step(ldsA, ldsB, tid, acc);
        __syncthreads();
    }
}

}  // namespace bvc

// bf16 MFMA GEMM for gfx950: problem descriptors and launcher (internal to libbvc_hip.so).
#pragma once
#include "common.h"
#include "dropgate.h"
#include "../../include/bvc.h"

namespace bvc {

// C[M,N] = epilogue(alpha * sum_k A(m,k) * B(k,n))
// Operand storage ("layout"):
//   GEMM_NT : A stored [M][lda] (k contiguous), B stored [N][ldb] (k contiguous)   y = x W^T   (forward Linear)
//   GEMM_NN : A stored [M][lda] (k contiguous), B stored [K][ldb] (n contiguous)   dx = dy W   (input gradient)
//   GEMM_TN : A stored [K][lda] (m contiguous), B stored [K][ldb] (n contiguous)   dW = dy^T x (weight gradient)
enum GemmLayout { GEMM_NT = BVC_GEMM_NT, GEMM_NN = BVC_GEMM_NN, GEMM_TN = BVC_GEMM_TN };

enum GemmEpilogue {
    EPI_F32 = BVC_EPI_F32,          // C f32 = v (+bias)            ; split_k>1: atomicAdd into C (C pre-zeroed / accumulating)
    EPI_BF16 = BVC_EPI_BF16,        // C bf16 = v (+bias)
    EPI_GELU = BVC_EPI_GELU,        // C bf16 = gelu'(v+bias) (what the backward product multiplies by), C2 bf16 = gelu(v+bias)
    EPI_RESID = BVC_EPI_RESID,      // C f32 = resid + v + bias      (resid may alias C); split_k>1: atomicAdd, resid must alias C
    EPI_POS = BVC_EPI_POS,          // C f32 = v + bias + pos[rowtok[m]][n]
    EPI_E2D = BVC_EPI_E2D,          // C f32[(m/rin)*rout + m%rin][n] = v + pos[rowtok[m]][n]
    EPI_LOSS = BVC_EPI_LOSS,        // d = v + bias - labels[m][n]; C bf16 = d; C2 f32 = v+bias (optional); partial[tile] = sum d^2
    EPI_DGELU = BVC_EPI_DGELU,      // C bf16 = v * aux[m][n], aux = the gelu' saved by EPI_GELU
    EPI_F32_BF16 = BVC_EPI_F32_BF16, // C f32 = v (+bias), C2 bf16 = same value
    EPI_RELU = BVC_EPI_RELU,         // C bf16 = relu(v + bias)
    EPI_DRELU = BVC_EPI_DRELU,       // C bf16 = v * (aux > 0)
    EPI_NCE = BVC_EPI_NCE,           // SimCLR loss partials (no C): see gemm.hip
    EPI_NCE_BWD = BVC_EPI_NCE_BWD,   // C bf16 = d loss / d (cos/T)
    EPI_RESID_LN = BVC_EPI_RESID_LN, // C f32 = resid + v + bias, C2 bf16 = LayerNorm(C) (N = 384: full rows in one tile; gemm8.hip only)
    EPI_DLN = BVC_EPI_DLN,           // LayerNorm backward fused into the dX product that feeds it (N = 384; gemm8.hip only)
    EPI_RESID_GATE = BVC_EPI_RESID_GATE // C f32 = resid + gate .* (v + bias) (dropgate.h; gemm_gate_kernel through launch_gemm_gate only)
};

// the public descriptor IS the internal problem record (include/bvc.h)
using GemmProblem = bvc_gemm_desc;

constexpr int kMaxGroup = 4;

// Process-wide switches behind bvc_set_option (include/bvc.h): what the parity tests and the same-process A/B tools flip.
//   gemm8:      0 = the measured selection (pick_gemm8 / plan_dw), 1 = the 256-row persistent kernel for EVERY product it can take
//               (whatever its size: how the tests run the bench's kernel set at oracle-sized batches), -1 = never
//   dw_overlap: 1 = the grouped weight-gradient launch of a layer runs on the context's side stream (no gain measured; A/B only)
//   row_ln:     LayerNorm fused into the neighbouring 384-wide product (gemm8.hip EC 4 / 5): 0 = the measured selection, 1 = whenever
//               the shapes allow, -1 = never (the separate ln_fwd / ln_bwd passes)
//   row_stagger: 1 (default) = the workgroups of a row-epilogue launch (gemm8.hip EC 4 / 5) start spread over one unit time, so that their
//               HBM-heavy epilogues do not all fall together; 0 = all start together (A/B)
//   deterministic: 1 = every reduction whose order the default kernels leave to the scheduler (f32 atomics: split-K / accumulating
//               GEMM outputs, fused bias gradients, LayerNorm parameter partials, column sums) runs in a fixed order instead: partials
//               go to a workspace slab with plain stores, a separate pass adds them in index order (launch_gemm, rowops.hip)
//   head_pad:   1 = heads of 80 / 88 dims run zero-padded to 96 in HBM (padded weight copies, pad / unpad launches per layer call), as
//               before the in-place attention instantiations; 0 (default) = in place.  Read when a stack is allocated (A/B only)
//   dec_tail:   1 (default) = the last decoder layer of the VideoMAE pre-training step runs everything behind its qkv product on the decoded
//               rows only (stack.h LayerTail) when the shapes allow; 0 = on all rows, as before that mode existed (A/B)
//   dec_first:  the first decoder layer of the VideoMAE pre-training step computes LayerNorm 1 and qkv of the mask rows once per position
//               (stack.h LayerFirst): -1 (default) = the measured gate, 1 = whenever the shapes allow, 0 = never (A/B)
struct Options { int gemm8 = 0; int dw_overlap = 0; int row_ln = 0; int row_stagger = 1; int deterministic = 0; int head_pad = 0; int dec_tail = 1; int dec_first = -1; };
Options& options();

// Workspace of the deterministic mode: library-owned, grow-only, one buffer per (device, stream) - kernels on one stream use it in
// stream order, kernels on different streams never share it.  Returns nullptr (error set) when the allocation fails.  Grown on the
// first deterministic launch that needs more (synchronises that stream once, then reused); never shrinks.
float* det_scratch(size_t floats, hipStream_t stream);
// bytes the deterministic workspace holds on the current device (all streams)
size_t det_scratch_bytes();
// synchronise the current device and free its deterministic workspaces (all streams)
int det_scratch_release();

// bvc_op_gemm_kernel: while `on`, the launchers write the name of the kernel instantiation they would launch (as rocprofv3
// prints it) and launch nothing - what bench.py uses to attribute its per-product timings to the rows of a kernel-stats table.
struct DryRun { bool on = false; char name[160] = ""; };
DryRun& dry_run();

// A TN product walks its K rows (of ld elements) 64 at a time; the rows past K in the last step read as zero only because their byte
// offsets lie past a_bytes / b_bytes.  The kernels form those offsets in 32 bits (gemm_tile.h stage_tile), so roundup64(K) rows plus one
// tile of columns must end below 2^32 bytes, or the surplus rows wrap to small offsets INSIDE the operand and real data joins the sum.
// launch_gemm refuses a product outside tn_tail_ok; the contexts keep every token count they accept inside it (operand_tail_bytes
// is what the up to 63 surplus rows and the columns add to a [tokens][columns] bf16 operand).
constexpr size_t operand_tail_bytes(size_t bf16_columns) { return 64 * bf16_columns * 2 + 1024; }
constexpr bool tn_tail_ok(int K, int ld) { return K % 64 == 0 || ((size_t)K + 63) / 64 * 64 * (size_t)ld * 2 + 1024 <= 0x100000000ull; }

// Launch 1..4 independent problems of the same layout as ONE grid (grouped GEMM) on `stream`.
// tile_cfg: -1 = pick from the tile count; 0 = 128x128, 1 = 128x64, 2 = 64x64.
// stages: -1 = pick from the grid size; 2..4 = LDS ring depth (K-steps of LDS-DMA in flight + 1).
int launch_gemm(const GemmProblem* probs, int nprob, GemmLayout layout, int tile_cfg, hipStream_t stream, int stages = -1);

// One NT product with the gated residual epilogue (EPI_RESID_GATE; split_k == 1) on the 128 x 128 / 128 x 64 / 64 x 64 kernel.
// tile_cfg: -1 = pick from the tile count, 0 / 1 / 2 as for launch_gemm.  The caller vouches that gate.path_scale (if any) holds
// ceil(M / gate.rows) entries.
int launch_gemm_gate(const GemmProblem& p, const Gate& gate, int tile_cfg, hipStream_t stream);

// number of loss partials an EPI_LOSS problem writes with the tile config launch_gemm would pick
int gemm_num_tiles(const GemmProblem& p, int tile_cfg);
int gemm_pick_tile(const GemmProblem* probs, int nprob, int tile_cfg);
bool gemm_row_ln_ok(int M, int N, int K);
// scratch floats an EPI_DLN problem needs in ln_part (one [2][384] row per workgroup of the one-workgroup-per-CU grid)
constexpr size_t kRowLnPartFloats = 512 * 2 * 384;

}  // namespace bvc

// Linear separability score: the kernels of a one-vs-rest squared-hinge linear SVM fitted on f32 embeddings (bvc_op_colstats,
// bvc_op_linear_pass; the reference scores its embeddings with sklearn's StandardScaler + LinearSVC in
// notebooks/EvaluateEmbeddings.ipynb get_separability_score).  Per class c, with y = +1 on the rows of class c and -1 elsewhere and
// xs the standardised row with a constant 1 appended (column D), the objective is
//   f_c(w) = 1/2 |w|^2 + C sum_i max(0, 1 - y_i w.xs_i)^2                  (w = [coefficients, intercept]: the intercept is regularised)
// and one pass gives, for K classes at once, either its data term's loss and gradient (GRAD), the data term of the generalised
// Hessian times a vector (HESSVEC), or the decision values and their argmax (DECISION).
//
// bvc_op_colstats: one workgroup per 8 columns, 32 row lanes per column; lane q of a column sums rows q, q + 32, .. in float64, the 32
// lane sums are added in lane order; mean = sum / n; the second sweep sums (x - mean)^2 the same way (population variance), and
// inv_std = 1 / sqrt(var), 1 where var == 0.  Both are rounded to f32 once.
//
// bvc_op_linear_pass, sep_pass_kernel: 256 threads = 4 waves; a workgroup owns a range of row tiles (R = 32 rows, 16 from D = 832 on)
// and a chunk of 32 classes.  A tile is standardised on load - xs = (x - mean) * inv_std, two f32 roundings - and lies in LDS as
// [R][D + 1 padded to 16] floats (row stride 18 mod 32 floats); X is read once per chunk of 32 classes - once in all for K <= 32,
// ceil(K / 32) times otherwise (6 times at 174 classes; where those repeats are served from has not been measured) - and the
// standardised matrix exists nowhere else.  W (and V) are read from L2 as the B operand, 16 steps ahead of the chain that consumes them.
//   1. Z = Xs W^T on v_mfma_f32_16x16x4_f32, one 16 x 16 block per wave: bit for bit the fmaf chain z = fma(xs[d], w[d], z) over
//      d = 0 .. D (the intercept, times 1, comes last) starting at 0; columns past D are zero on both sides (fma(0, 0, z) = z).
//   2. the element-wise stage in the accumulator's registers, A to LDS as [R][32]:
//        GRAD      m = 1 - y z;  a = m > 0 ? (-2 C y) m : 0;  loss term m > 0 ? m^2 : 0
//        HESSVEC   a = 1 - y z(W) > 0 ? (2 C) z(V) : 0          (both products from the same operand read)
//        DECISION  z is stored to the [n][K] decision array; no second product
//   3. G += A^T Xs on the same MFMA, 32 classes x (D + 1) columns in the accumulators of the four waves for the whole row range.
// Row sums: an element of G is ONE fmaf chain over the rows of the workgroup's range in ascending row order (rows past n add
// fma(0, 0, g) = g), the loss of a class one fmaf chain loss = fma(m, m, loss) over the same rows in the same order; the ranges are
// the `splits` contiguous runs of row tiles  tiles * s / splits .. tiles * (s + 1) / splits, and sep_reduce_kernel adds the
// per-range partials in ascending range order starting from range 0's value.  splits is a function of (n, D, K) alone
// (bvc_op_linear_pass_splits): no float atomics anywhere, the same bits on every run, deterministic mode or not.
// DECISION: sep_argmax_kernel, one thread per row, keeps the first strict maximum (ties to the smaller class); one column: z > 0.
//
// Bounds: D <= 1343 (a 16-row tile of D + 1 <= 1344 columns is 85 KB of LDS; the accumulators of G, 8 floats per 64 columns, are
// what ends the range: 168 registers there).  A two-read form for wider rows is not built: larger D is refused.  K <= 1024 columns
// per call; more classes are a host loop over class chunks (the classes are independent).
#include <math.h>

#include "common.h"

namespace bvc {

constexpr int kSepKc = 32;         // classes per workgroup: two 16-wide MFMA blocks
constexpr int kSepAs = 48;         // floats per row of the A / loss-term images (48 = 16 mod 32: the two row halves of a read hit different banks)
constexpr int kSepMaxK = 1024;
constexpr int kSepMaxD = 1343;
constexpr int kSepCUs = 256;
constexpr int kSepDevices = 64;     // devices whose kernels' LDS attribute is remembered
constexpr int kSepAhead = 16;      // steps of product 1 whose W operands are loaded ahead
enum { kSepGrad = 0, kSepHessvec = 1, kSepDecision = 2 };

// ---------------------------------------------------------------- column statistics
// kSepStatCols columns x kSepStatLanes row lanes per workgroup; the row loop keeps four loads in flight and adds them in row order
constexpr int kSepStatCols = 8, kSepStatLanes = 32;
__global__ __launch_bounds__(256) void sep_colstats_kernel(const float* __restrict__ x, int64_t ldx, int n, int D,
                                                           float* __restrict__ mean, float* __restrict__ inv_std) {
    __shared__ double part[kSepStatLanes][kSepStatCols];
    __shared__ double mu[kSepStatCols];
    const int c = threadIdx.x % kSepStatCols, q = threadIdx.x / kSepStatCols;
    const int col = blockIdx.x * kSepStatCols + c;
    const bool ok = col < D;
    const float* p = x + (ok ? col : D - 1);
    constexpr int L = kSepStatLanes;
    double s = 0.0;
    for (int r = q; r < n; r += 4 * L) {      // rows past the end are loaded from the last row and not added
        const float v0 = p[(int64_t)r * ldx], v1 = p[(int64_t)min(r + L, n - 1) * ldx];
        const float v2 = p[(int64_t)min(r + 2 * L, n - 1) * ldx], v3 = p[(int64_t)min(r + 3 * L, n - 1) * ldx];
        s += (double)v0;
        if (r + L < n) s += (double)v1;
        if (r + 2 * L < n) s += (double)v2;
        if (r + 3 * L < n) s += (double)v3;
    }
    part[q][c] = s;
    __syncthreads();
    if (q == 0) {
        double t = part[0][c];
        for (int j = 1; j < L; ++j) t += part[j][c];
        mu[c] = t / (double)n;
    }
    __syncthreads();
    const double m = mu[c];
    s = 0.0;
    for (int r = q; r < n; r += 4 * L) {
        const float v0 = p[(int64_t)r * ldx], v1 = p[(int64_t)min(r + L, n - 1) * ldx];
        const float v2 = p[(int64_t)min(r + 2 * L, n - 1) * ldx], v3 = p[(int64_t)min(r + 3 * L, n - 1) * ldx];
        const double d0 = (double)v0 - m, d1 = (double)v1 - m, d2 = (double)v2 - m, d3 = (double)v3 - m;
        s += d0 * d0;
        if (r + L < n) s += d1 * d1;
        if (r + 2 * L < n) s += d2 * d2;
        if (r + 3 * L < n) s += d3 * d3;
    }
    __syncthreads();
    part[q][c] = s;
    __syncthreads();
    if (q == 0 && ok) {
        double t = part[0][c];
        for (int j = 1; j < L; ++j) t += part[j][c];
        const double var = t / (double)n;
        mean[col] = (float)m;
        inv_std[col] = var > 0.0 ? (float)(1.0 / sqrt(var)) : 1.0f;
    }
}

// ---------------------------------------------------------------- the pass
struct SepArgs {
    const float* x; int64_t ldx;
    const int* labels; const float* mean; const float* inv_std;
    const float* W; const float* V;
    float* part_G;        // [splits][K][D + 1]
    float* part_loss;     // [splits][K]
    float* dec;           // [n][K]
    int n, D, K, class0, splits, stride;
    float C;
};

// RB: 16-row blocks per tile; NB: 16-column blocks of G per wave (columns 16 (wave + 4 q), q < NB)
template <int MODE, int RB, int NB>
__global__ __launch_bounds__(256) void sep_pass_kernel(SepArgs a) {
    extern __shared__ __attribute__((aligned(16))) float sep_lds[];
    constexpr int R = 16 * RB;
    float* const xs = sep_lds;                       // [R][stride]
    float* const as = xs + R * a.stride;             // [R][kSepAs]
    float* const ls = as + R * kSepAs;               // [R][kSepAs] loss terms (GRAD)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i16 = lane & 15, h = lane >> 4;
    const int chunks = (a.K + kSepKc - 1) / kSepKc;
    const int chunk = blockIdx.x % chunks, split = blockIdx.x / chunks;      // the class chunks of one row range run side by side
    const int k0 = chunk * kSepKc;
    const int D1 = a.D + 1, stride = a.stride;
    const int dsteps = (D1 + 3) / 4;
    const int tiles = (a.n + R - 1) / R;
    const int t_begin = (int)((int64_t)tiles * split / a.splits), t_end = (int)((int64_t)tiles * (split + 1) / a.splits);

    // product 1: wave -> (row block zr, class block zc); with one row block only waves 0 and 1 have a block
    const bool zwave = wave < 2 * RB;
    const int zr = RB == 2 ? wave >> 1 : 0, zc = wave & 1;
    const int wk = min(k0 + 16 * zc + i16, a.K - 1);                         // this lane's class as the B operand (clamped)
    const bool wok = k0 + 16 * zc + i16 < a.K;
    const float* const wrow = a.W + (int64_t)wk * D1;
    const float* const vrow = MODE == kSepHessvec ? a.V + (int64_t)wk * D1 : nullptr;

    f32x4 acc[2][NB];
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int q = 0; q < NB; ++q) acc[cb][q] = f32x4{0.f, 0.f, 0.f, 0.f};
    float loss = 0.f;                                                        // thread k < 32: the chain of class k0 + k

    for (int t = t_begin; t < t_end; ++t) {
        const int row0 = t * R;
        // ---- stage: wave w takes rows w, w + 4, ..; a lane column lane, lane + 64, ..  No load under a per-lane condition:
        // row and column are clamped into the array and the value is chosen afterwards.
        // Column outside, rows inside: a lane keeps mean and inv_std of its column and has its R / 4 rows' loads in flight at once.
        for (int c = lane; c < stride; c += 64) {
            const int cc = min(c, a.D - 1);
            const float mu = a.mean[cc], is = a.inv_std[cc];
            float v[R / 4];
#pragma unroll
            for (int j = 0; j < R / 4; ++j) v[j] = a.x[(int64_t)min(row0 + wave + 4 * j, a.n - 1) * a.ldx + cc];
#pragma unroll
            for (int j = 0; j < R / 4; ++j) {
                const bool rok = row0 + wave + 4 * j < a.n;
                xs[(wave + 4 * j) * stride + c] = !rok ? 0.f : c < a.D ? (v[j] - mu) * is : c == a.D ? 1.0f : 0.f;
            }
        }
        __syncthreads();

        // ---- 1. Z block of this wave
        if (zwave) {
            f32x4 z = {0.f, 0.f, 0.f, 0.f}, zv = {0.f, 0.f, 0.f, 0.f};
            const float* const arow = xs + (16 * zr + i16) * stride + h;
            // W (and V) come straight from L2, 4 bytes per lane and step: kSepAhead steps are loaded while the previous kSepAhead
            // are consumed, so the load latency is spread over a group instead of being paid at every step of the chain.
            float wc[kSepAhead], wn[kSepAhead], vc[kSepAhead], vn[kSepAhead];
#pragma unroll
            for (int j = 0; j < kSepAhead; ++j) {
                wc[j] = wrow[min(4 * j + h, a.D)];
                vc[j] = MODE == kSepHessvec ? vrow[min(4 * j + h, a.D)] : 0.f;
            }
            for (int s0 = 0; s0 < dsteps; s0 += kSepAhead) {
#pragma unroll
                for (int j = 0; j < kSepAhead; ++j) {      // (clamped into the row: the last group's look-ahead reads column D again)
                    wn[j] = wrow[min(4 * (s0 + kSepAhead + j) + h, a.D)];
                    vn[j] = MODE == kSepHessvec ? vrow[min(4 * (s0 + kSepAhead + j) + h, a.D)] : 0.f;
                }
#pragma unroll
                for (int j = 0; j < kSepAhead; ++j) {
                    const int s = s0 + j, d = 4 * s + h;
                    if (s < dsteps) {      // (wave-uniform)
                        const bool ok = wok && d < D1;
                        const float xa = arow[4 * s];
                        z = __builtin_amdgcn_mfma_f32_16x16x4f32(xa, ok ? wc[j] : 0.f, z, 0, 0, 0);
                        if (MODE == kSepHessvec) zv = __builtin_amdgcn_mfma_f32_16x16x4f32(xa, ok ? vc[j] : 0.f, zv, 0, 0, 0);
                    }
                }
#pragma unroll
                for (int j = 0; j < kSepAhead; ++j) { wc[j] = wn[j]; vc[j] = vn[j]; }
            }
            // ---- 2. element e: tile row 16 zr + 4 h + e, class k0 + 16 zc + i16
            const int cls = k0 + 16 * zc + i16;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int r = 16 * zr + 4 * h + e;
                const bool rok = row0 + r < a.n;
                if (MODE == kSepDecision) {
                    if (rok && cls < a.K) a.dec[(int64_t)(row0 + r) * a.K + cls] = z[e];
                } else {
                    const int lab = a.labels[min(row0 + r, a.n - 1)];
                    const float y = lab == a.class0 + cls ? 1.0f : -1.0f;
                    const float m = 1.0f - y * z[e];
                    const bool on = rok && cls < a.K && m > 0.f;
                    float av;
                    if (MODE == kSepGrad) {
                        av = on ? (-2.0f * a.C * y) * m : 0.f;
                        ls[r * kSepAs + 16 * zc + i16] = on ? m : 0.f;
                    } else {
                        av = on ? (2.0f * a.C) * zv[e] : 0.f;
                    }
                    as[r * kSepAs + 16 * zc + i16] = av;
                }
            }
        }
        if (MODE != kSepDecision) {
            __syncthreads();
            // ---- 3. G += A^T Xs: A operand = class 16 cb + i16 at row 4 s + h, B operand = row 4 s + h at column 16 db + i16
            float af[2][R / 4];
#pragma unroll
            for (int cb = 0; cb < 2; ++cb)
#pragma unroll
                for (int s = 0; s < R / 4; ++s) af[cb][s] = as[(4 * s + h) * kSepAs + 16 * cb + i16];
#pragma unroll
            for (int q = 0; q < NB; ++q) {
                const int db = wave + 4 * q;
                if (16 * db < D1) {      // (wave-uniform)
#pragma unroll
                    for (int s = 0; s < R / 4; ++s) {
                        const float xb = xs[(4 * s + h) * stride + 16 * db + i16];
                        acc[0][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[0][s], xb, acc[0][q], 0, 0, 0);
                        acc[1][q] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[1][s], xb, acc[1][q], 0, 0, 0);
                    }
                }
            }
            if (MODE == kSepGrad && tid < kSepKc) {
                for (int r = 0; r < R; ++r) {
                    const float m = ls[r * kSepAs + tid];
                    loss = fmaf(m, m, loss);
                }
            }
        }
        __syncthreads();      // the tile and the A image are free for the next stage
    }

    if (MODE == kSepDecision) return;
    // ---- this range's partials.  Element e of acc[cb][q]: class k0 + 16 cb + 4 h + e, column 16 (wave + 4 q) + i16
    float* const pg = a.part_G + (int64_t)split * a.K * D1;
#pragma unroll
    for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int q = 0; q < NB; ++q) {
            const int d = 16 * (wave + 4 * q) + i16;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int cls = k0 + 16 * cb + 4 * h + e;
                if (cls < a.K && d < D1) pg[(int64_t)cls * D1 + d] = acc[cb][q][e];
            }
        }
    if (MODE == kSepGrad && tid < kSepKc && k0 + tid < a.K) a.part_loss[(int64_t)split * a.K + k0 + tid] = loss;
}

// out[i] = part[0][i] + part[1][i] + .. in that order (i over K (D + 1) elements of G, then the K losses)
__global__ __launch_bounds__(256) void sep_reduce_kernel(const float* __restrict__ part_G, const float* __restrict__ part_loss, int splits,
                                                         int64_t ng, int K, float* __restrict__ out_G, float* __restrict__ out_loss) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < ng) {
        float s = part_G[i];
        for (int j = 1; j < splits; ++j) s += part_G[(int64_t)j * ng + i];
        out_G[i] = s;
    } else if (out_loss && i < ng + K) {
        const int k = (int)(i - ng);
        float s = part_loss[k];
        for (int j = 1; j < splits; ++j) s += part_loss[(int64_t)j * K + k];
        out_loss[k] = s;
    }
}

__global__ __launch_bounds__(256) void sep_argmax_kernel(const float* __restrict__ dec, int n, int K, int* __restrict__ pred) {
    const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (row >= n) return;
    const float* p = dec + row * K;
    if (K == 1) { pred[row] = p[0] > 0.f ? 1 : 0; return; }
    float best = p[0];
    int at = 0;
    for (int k = 1; k < K; ++k) {
        const float v = p[k];
        if (v > best) { best = v; at = k; }
    }
    pred[row] = at;
}

// ---------------------------------------------------------------- host side
static int sep_tile_rows(int D) { return D + 1 <= 832 ? 32 : 16; }
static int sep_stride(int D) {      // D + 1 padded to 16 columns, then to 18 mod 32 (conflict-free operand reads of product 1)
    int s = (D + 1 + 15) / 16 * 16;
    while (s % 32 != 18) ++s;
    return s;
}
static int sep_resolve_splits(int n, int D, int K) {
    const int R = sep_tile_rows(D);
    const int64_t tiles = ((int64_t)n + R - 1) / R;
    const int chunks = (K + kSepKc - 1) / kSepKc;
    int64_t s = kSepCUs / chunks;
    if (s < 1) s = 1;
    return (int)(s < tiles ? s : tiles);
}

static int sep_check_shape(int n, int D, int K, int mode) {
    BVC_REQUIRE(n > 0 && D > 0 && K > 0, "op_linear_pass: non-positive size (n %d, D %d, K %d)", n, D, K);
    BVC_REQUIRE(D <= kSepMaxD, "op_linear_pass: D %d above %d", D, kSepMaxD);
    BVC_REQUIRE(K <= kSepMaxK, "op_linear_pass: K %d above %d columns per call", K, kSepMaxK);
    BVC_REQUIRE(mode >= kSepGrad && mode <= kSepDecision, "op_linear_pass: mode %d (0 grad, 1 hessvec, 2 decision)", mode);
    return BVC_OK;
}

int64_t sep_workspace(int n, int D, int K, int mode) {
    if (sep_check_shape(n, D, K, mode) != BVC_OK) return -1;
    if (mode == kSepDecision) return ws_align((int64_t)n * K * 4);
    const int s = sep_resolve_splits(n, D, K);
    return ws_align((int64_t)s * K * (D + 1) * 4) + ws_align((int64_t)s * K * 4);
}

template <int MODE>
static int sep_launch(const SepArgs& a, int grid, hipStream_t stream) {
    const int R = sep_tile_rows(a.D);
    const size_t lds = ((size_t)R * a.stride + 2 * (size_t)R * kSepAs) * 4;
    const int blocks = (a.D + 1 + 15) / 16;
    void (*kern)(SepArgs) = R == 16 ? sep_pass_kernel<MODE, 1, 21> : blocks <= 16 ? sep_pass_kernel<MODE, 2, 4> : sep_pass_kernel<MODE, 2, 13>;
    BVC_REQUIRE(lds <= 160 * 1024, "op_linear_pass: %zu bytes of LDS", lds);
    // the attribute is raised once per kernel instance and device, not at every one of a fit's ~1000 launches
    const int which = R == 16 ? 0 : blocks <= 16 ? 1 : 2;
    static size_t allowed[kSepDevices][3] = {};
    int device = 0;
    BVC_CHECK_HIP(hipGetDevice(&device));
    if (device < 0 || device >= kSepDevices || allowed[device][which] < lds) {
        BVC_CHECK_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
        if (device >= 0 && device < kSepDevices) allowed[device][which] = 160 * 1024;
    }
    kern<<<dim3((unsigned)grid), dim3(256), lds, stream>>>(a);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

int launch_linear_pass(const float* x, int64_t ldx, const int* labels, const float* mean, const float* inv_std, const float* W,
                       const float* V, int n, int D, int K, int class0, int mode, float C, float* out_G, float* out_loss, int* out_pred,
                       float* out_dec, void* workspace, hipStream_t stream) {
    if (int rc = sep_check_shape(n, D, K, mode)) return rc;
    BVC_REQUIRE(x && mean && inv_std && W && workspace, "op_linear_pass: null argument");
    BVC_REQUIRE(ldx >= D, "op_linear_pass: row stride %lld below D %d", (long long)ldx, D);
    BVC_REQUIRE(class0 >= 0, "op_linear_pass: negative class0 %d", class0);
    if (mode == kSepDecision) BVC_REQUIRE(out_pred, "op_linear_pass: decision needs out_pred");
    else BVC_REQUIRE(labels && out_G, "op_linear_pass: null labels or out_G");
    if (mode == kSepGrad) BVC_REQUIRE(out_loss && C > 0.f, "op_linear_pass: grad needs out_loss and C > 0");
    if (mode == kSepHessvec) BVC_REQUIRE(V && C > 0.f, "op_linear_pass: hessvec needs V and C > 0");
    BVC_REQUIRE((((uintptr_t)x | (uintptr_t)workspace | (uintptr_t)labels | (uintptr_t)mean | (uintptr_t)inv_std | (uintptr_t)W | (uintptr_t)V |
                  (uintptr_t)out_G | (uintptr_t)out_loss | (uintptr_t)out_pred | (uintptr_t)out_dec) & 3) == 0, "op_linear_pass: misaligned pointer");

    const int splits = sep_resolve_splits(n, D, K);
    const int chunks = (K + kSepKc - 1) / kSepKc;
    SepArgs a{};
    a.x = x; a.ldx = ldx; a.labels = labels; a.mean = mean; a.inv_std = inv_std; a.W = W; a.V = V;
    a.n = n; a.D = D; a.K = K; a.class0 = class0; a.splits = splits; a.stride = sep_stride(D); a.C = C;
    if (mode == kSepDecision) {
        a.dec = out_dec ? out_dec : ws_at<float>(workspace, 0);
        if (int rc = sep_launch<kSepDecision>(a, splits * chunks, stream)) return rc;
        sep_argmax_kernel<<<dim3((unsigned)(((int64_t)n + 255) / 256)), dim3(256), 0, stream>>>(a.dec, n, K, out_pred);
        BVC_CHECK_HIP(hipGetLastError());
        return BVC_OK;
    }
    const int64_t ng = (int64_t)K * (D + 1);
    a.part_G = ws_at<float>(workspace, 0);
    a.part_loss = ws_at<float>(workspace, ws_align(splits * ng * 4));
    if (int rc = mode == kSepGrad ? sep_launch<kSepGrad>(a, splits * chunks, stream) : sep_launch<kSepHessvec>(a, splits * chunks, stream)) return rc;
    sep_reduce_kernel<<<dim3((unsigned)((ng + K + 255) / 256)), dim3(256), 0, stream>>>(a.part_G, a.part_loss, splits, ng, K, out_G,
                                                                                       mode == kSepGrad ? out_loss : nullptr);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

}  // namespace bvc

extern "C" {

int bvc_op_colstats(const float* x, int64_t ldx, int n, int D, float* mean, float* inv_std, void* stream) {
    BVC_REQUIRE(n > 0 && D > 0, "op_colstats: non-positive size (n %d, D %d)", n, D);
    BVC_REQUIRE(x && mean && inv_std, "op_colstats: null argument");
    BVC_REQUIRE(ldx >= D, "op_colstats: row stride %lld below D %d", (long long)ldx, D);
    bvc::sep_colstats_kernel<<<dim3((unsigned)((D + bvc::kSepStatCols - 1) / bvc::kSepStatCols)), dim3(256), 0, (hipStream_t)stream>>>(x, ldx, n, D, mean, inv_std);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}
int64_t bvc_op_linear_pass_workspace(int n, int D, int K, int mode) { return bvc::sep_workspace(n, D, K, mode); }
int bvc_op_linear_pass_splits(int n, int D, int K) {
    if (bvc::sep_check_shape(n, D, K, 0) != BVC_OK) return -1;
    return bvc::sep_resolve_splits(n, D, K);
}
int bvc_op_linear_pass_tile_rows(int D) { return D > 0 && D <= bvc::kSepMaxD ? bvc::sep_tile_rows(D) : -1; }
int bvc_op_linear_pass(const float* x, int64_t ldx, const int* labels, const float* mean, const float* inv_std, const float* W,
                       const float* V, int n, int D, int K, int class0, int mode, float C, float* out_G, float* out_loss, int* out_pred,
                       float* out_dec, void* workspace, void* stream) {
    return bvc::launch_linear_pass(x, ldx, labels, mean, inv_std, W, V, n, D, K, class0, mode, C, out_G, out_loss, out_pred, out_dec,
                                   workspace, (hipStream_t)stream);
}

}  // extern "C"

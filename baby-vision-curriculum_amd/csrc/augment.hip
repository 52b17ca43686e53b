// Clip transforms on uint8 frames (include/bvc.h, bvc_frame_aug; arithmetic in augment.h): resize + crop + flip + colour jitter, and
// the post stage on their output (bvc_frame_post): blur, gray, rotation - its two kernels are described where they stand, below.
//
// clip_precision_kernel  one workgroup per output frame: the fixed-point precision of its two axes (the largest tap weight over the
//                      whole resized axis decides it) into the head of the workspace.
// clip_resize_kernel   one workgroup per 32 x 32 tile of one output frame, all three channels.  The tap weights of the tile's 32
//                      columns and 32 rows go to LDS once; the horizontal pass reads the source bytes and leaves its uint8 result for
//                      the source rows the tile needs in LDS (80 rows at most at a time: a tile whose rows need more runs in row
//                      groups); the vertical pass reads that image, applies the colour stages in front of the contrast stage (all
//                      of them, and the grayscale stage, when the chain has none), mirrors and stores.  A frame with a contrast
//                      stage also leaves the tile's integer gray sum in the workspace: a plain store, no atomics.
// clip_colour_kernel   only when some frame has a contrast stage: adds the frame's tile sums (integers, so the order is immaterial),
//                      and runs the chain from the contrast stage on, in place, four pixels per thread.  Frames without one exit.
#include "augment.h"
#include "common.h"

namespace bvc {
namespace aug {

constexpr int kTile = 32;                 // output tile edge
constexpr int kRowCap = 80;               // source rows of the horizontal image held at a time (>= kMaxTaps)
constexpr int kWStride = kMaxTaps + 1;    // odd: the 32 columns' weight rows start on 32 different banks
static_assert(kRowCap >= kMaxTaps, "one output row's taps must fit");

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
    return v;
}

__device__ __forceinline__ double wave_max_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

__global__ __launch_bounds__(256) void clip_precision_kernel(const Entry* __restrict__ table, int F_src, int Hs, int Ws, int Ho, int Wo,
                                                             int* __restrict__ prec) {
    __shared__ double red[2][4];
    const int f = blockIdx.x, tid = threadIdx.x;
    const Entry e = sanitize(table[f], F_src, Hs, Ws, Ho, Wo);
    const Axis ax = make_axis(e.w, e.Wr), ay = make_axis(e.h, e.Hr);
    double mx = 0.0, my = 0.0;
    for (int i = tid; i < e.Wr; i += 256) mx = fmax(mx, max_weight(ax, i));
    for (int i = tid; i < e.Hr; i += 256) my = fmax(my, max_weight(ay, i));
    mx = wave_max_f64(mx); my = wave_max_f64(my);
    if ((tid & 63) == 0) { red[0][tid >> 6] = mx; red[1][tid >> 6] = my; }
    __syncthreads();
    if (tid < 2) prec[2 * f + tid] = precision_of(fmax(fmax(red[tid][0], red[tid][1]), fmax(red[tid][2], red[tid][3])));
}

__global__ __launch_bounds__(256) void clip_resize_kernel(const uint8_t* __restrict__ src, int F_src, int Hs, int Ws,
                                                          const Entry* __restrict__ table, int Ho, int Wo, uint8_t* __restrict__ out,
                                                          const int* __restrict__ prec, uint32_t* __restrict__ partial, int tiles_x,
                                                          int tiles) {
    __shared__ int wx[kTile * kWStride], wy[kTile * kWStride];
    __shared__ int fx[kTile], nx[kTile], fy[kTile], ny[kTile];
    __shared__ uint8_t hor[3][kRowCap][kTile];
    __shared__ uint32_t red[4];
    __shared__ Entry entry;        // in LDS, not registers: the stages index its factors by op
    const int tid = threadIdx.x;
    const int f = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const int r0 = (tile / tiles_x) * kTile, c0 = (tile % tiles_x) * kTile;
    const int rows = min(kTile, Ho - r0), cols = min(kTile, Wo - c0);
    if (tid == 0) entry = sanitize(table[f], F_src, Hs, Ws, Ho, Wo);
    __syncthreads();
    const Entry& e = entry;
    const int px = min(max(prec[2 * f], 1), 21), py = min(max(prec[2 * f + 1], 1), 21);

    if (tid < kTile) {
        nx[tid] = tid < cols ? taps(make_axis(e.w, e.Wr), e.ox + c0 + tid, px, &wx[tid * kWStride], &fx[tid]) : 0;
    } else if (tid >= 64 && tid < 64 + kTile) {
        const int r = tid - 64;
        ny[r] = r < rows ? taps(make_axis(e.h, e.Hr), e.oy + r0 + r, py, &wy[r * kWStride], &fy[r]) : 0;
    }
    __syncthreads();

    const int j = tid & (kTile - 1), lane_row = tid / kTile;      // 8 rows of 32 columns per sweep
    const bool live = j < cols;
    const int cpos = contrast_at(e);
    const uint8_t* sf = src + (size_t)e.src * 3 * Hs * Ws + (size_t)e.y0 * Ws + e.x0;
    uint8_t* of = out + (size_t)f * 3 * Ho * Wo;
    const int jout = e.flip ? Wo - 1 - (c0 + j) : c0 + j;
    uint32_t gsum = 0;

    for (int a = 0; a < rows;) {
        const int base = fy[a];
        int b = a + 1;
        while (b < rows && fy[b] + ny[b] - base <= kRowCap) ++b;
        const int span = min(fy[b - 1] + ny[b - 1] - base, kRowCap);
        // horizontal pass: source rows base .. base + span of the region, the tile's columns
        if (live) {
            const int first = fx[j], n = nx[j];
            const int* w = &wx[j * kWStride];
            for (int r = lane_row; r < span; r += 256 / kTile) {
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const uint8_t* row = sf + ((size_t)c * Hs + base + r) * Ws + first;
                    int acc = 0;
                    for (int k = 0; k < n; ++k) acc += w[k] * (int)row[k];
                    hor[c][r][j] = (uint8_t)fixed_u8(acc, px);
                }
            }
        }
        __syncthreads();
        // vertical pass, the colour stages local to a pixel, store
        if (live) {
            for (int r = a + lane_row; r < b; r += 256 / kTile) {
                const int first = min(fy[r] - base, kRowCap - 1), n = min(ny[r], kRowCap - first);
                const int* w = &wy[r * kWStride];
                int p[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    int acc = 0;
                    for (int k = 0; k < n; ++k) acc += w[k] * (int)hor[c][first + k][j];
                    p[c] = fixed_u8(acc, py);
                }
                stages(e, 0, cpos, 0.f, p);
                if (cpos == e.nops) {
                    if (e.gray) to_gray(p);
                } else {
                    gsum += (uint32_t)gray_u8(p);
                }
#pragma unroll
                for (int c = 0; c < 3; ++c) of[((size_t)c * Ho + r0 + r) * Wo + jout] = (uint8_t)p[c];
            }
        }
        __syncthreads();
        a = b;
    }
    if (cpos < e.nops) {        // uniform over the workgroup
        gsum = wave_sum_u32(gsum);
        if ((tid & 63) == 0) red[tid >> 6] = gsum;
        __syncthreads();
        if (tid == 0) partial[(size_t)f * tiles + tile] = red[0] + red[1] + red[2] + red[3];
    }
}

// pixels 4 q .. 4 q + 3 of a frame's plane per thread; `vec` = the planes are 4-byte aligned and a multiple of 4 long
__global__ __launch_bounds__(256) void clip_colour_kernel(const Entry* __restrict__ table, int Ho, int Wo, uint8_t* __restrict__ out,
                                                          const uint32_t* __restrict__ partial, int tiles, int chunks, int vec) {
    const int f = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
    __shared__ Entry entry;
    if (threadIdx.x == 0) {
        entry = table[f];
        entry.nops = entry.nops < 0 ? 0 : (entry.nops > 4 ? 4 : entry.nops);
    }
    __syncthreads();
    const Entry& e = entry;
    const int cpos = contrast_at(e);
    if (cpos == e.nops) return;
    uint32_t lo = 0, hi = 0;       // 64-bit sum of the tile sums as two words: every wave adds all of them
    for (int t = threadIdx.x & 63; t < tiles; t += 64) {
        const uint32_t v = partial[(size_t)f * tiles + t];
        lo += v & 0xFFFFu; hi += v >> 16;
    }
    lo = wave_sum_u32(lo); hi = wave_sum_u32(hi);
    const float mean = gray_mean(((uint64_t)hi << 16) + lo, Ho, Wo);

    const int plane = Ho * Wo;
    const int q = (chunk * 256 + threadIdx.x) * 4;
    if (q >= plane) return;
    uint8_t* of = out + (size_t)f * 3 * plane;
    uint8_t px[3][4];
    const int n = min(4, plane - q);
    if (vec) {
#pragma unroll
        for (int c = 0; c < 3; ++c) *reinterpret_cast<uint32_t*>(px[c]) = *reinterpret_cast<const uint32_t*>(of + (size_t)c * plane + q);
    } else {
        for (int c = 0; c < 3; ++c)
            for (int i = 0; i < n; ++i) px[c][i] = of[(size_t)c * plane + q + i];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (i < n) {
            int p[3] = {px[0][i], px[1][i], px[2][i]};
            stages(e, cpos, e.nops, mean, p);
            if (e.gray) to_gray(p);
            px[0][i] = (uint8_t)p[0]; px[1][i] = (uint8_t)p[1]; px[2][i] = (uint8_t)p[2];
        }
    }
    if (vec) {
#pragma unroll
        for (int c = 0; c < 3; ++c) *reinterpret_cast<uint32_t*>(of + (size_t)c * plane + q) = *reinterpret_cast<const uint32_t*>(px[c]);
    } else {
        for (int c = 0; c < 3; ++c)
            for (int i = 0; i < n; ++i) of[(size_t)c * plane + q + i] = px[c][i];
    }
}

static int tiles_of(int Ho, int Wo) { return ((Ho + kTile - 1) / kTile) * ((Wo + kTile - 1) / kTile); }

static int check_call(const char* who, const void* src, int F_src, int channels, int Hs, int Ws, const Entry* table, int F_out, int Ho, int Wo,
                      const void* out, bool* second_pass) {
    BVC_REQUIRE(src && table && out, "%s: null argument", who);
    BVC_REQUIRE(channels == 3, "%s: %d channels (the colour stages are defined for 3)", who, channels);
    BVC_REQUIRE(F_src >= 1 && Hs >= 1 && Ws >= 1 && F_out >= 1 && Ho >= 1 && Wo >= 1, "%s: empty source or output", who);
    BVC_REQUIRE((int64_t)Ho * Wo <= (1 << 24) && (int64_t)Hs * Ws <= (1 << 28), "%s: frame too large", who);
    BVC_REQUIRE((int64_t)F_out * ((int64_t)Ho * Wo / 1024 + tiles_of(Ho, Wo)) < (1ll << 30), "%s: too many output frames", who);
    *second_pass = false;
    char msg[512];
    for (int f = 0; f < F_out; ++f) {
        if (invalid(table[f], f, F_src, Hs, Ws, Ho, Wo, msg, sizeof(msg))) {
            set_error("%s", msg);
            return BVC_ERR_INVALID;
        }
        if (contrast_at(table[f]) < table[f].nops) *second_pass = true;
    }
    return BVC_OK;
}

// ---------------------------------------------------------------- post stage (bvc_frame_post)
// clip_blur_kernel    one workgroup per 32 x 64 tile of one frame, three channels.  The tile plus a halo of 3 (r + 1) pixels (rounded up
//                     to whole words along the rows) sits in LDS as REPLICATE-PADDED words of four pixels: positions beyond the frame
//                     hold the frame's edge value, and every pass computes a position beyond the frame as its nearest position inside,
//                     so the padding is again the edge value of the next pass's input - the per-pass clamp against the frame, with no
//                     clamp in the inner loops.  Six passes ping-pong between two images; a row pass builds four outputs from three
//                     words, a column pass from 2 r + 3 words of one column with two 16-bit sums per register.  Each pass is exact
//                     r + 1 pixels further inside the region than its input, hence the halo.  Gray, then the store, whole words
//                     where the planes allow.  A frame without blur has no halo and no pass: its workgroups copy (or gray) the tile.
// clip_rotate_kernel  a gather: four output pixels of a plane per thread, three channels, the map stepped from pixel to pixel,
//                     whole-word stores where the planes allow; frames that do not rotate are copied.
constexpr int kBlurW = 64, kBlurH = 32;              // output tile
constexpr int kBlurHalo = 3 * (kMaxBoxRadius + 1);   // 12: three passes per direction
constexpr int kBlurDw = (kBlurW + 2 * kBlurHalo) / 4, kBlurRows = kBlurH + 2 * kBlurHalo;      // 22 words x 56 rows per channel
static_assert(kBlurHalo % 4 == 0 && kBlurW % 4 == 0, "the padded region is made of whole words");

// One pass's rounding with 24-bit multiplies (full rate; the 32-bit one is not).  The kernel runs the passes only for ww < 2^24 (ww = 2^24
// is the identity: fw = 0 there), an accepted fw is at most 2^23 and a sum of taps at most 7 x 255; the products fit 32 bits.
__device__ __forceinline__ uint32_t box24(uint32_t inner, uint32_t far, uint32_t ww, uint32_t fw) {
    return (__umul24(ww, inner) + __umul24(fw, far) + (1u << 23)) >> 24;
}
// four outputs of a row pass from the words left of, at and right of them
template <int R>
__device__ __forceinline__ uint32_t box4_row(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t ww, uint32_t fw) {
    uint32_t b[12];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        b[k] = (w0 >> (8 * k)) & 255u; b[4 + k] = (w1 >> (8 * k)) & 255u; b[8 + k] = (w2 >> (8 * k)) & 255u;
    }
    uint32_t o = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        uint32_t inner = 0;
#pragma unroll
        for (int i = -R; i <= R; ++i) inner += b[4 + j + i];
        o |= box24(inner, b[4 + j - R - 1] + b[4 + j + R + 1], ww, fw) << (8 * j);
    }
    return o;
}
// the same four outputs one by one from the bytes of the row, each centred on its nearest column inside the frame [xlo, xhi]
// (region columns); every index is also held inside the row of `n` bytes
template <int R>
__device__ __forceinline__ uint32_t box4_row_edge(const uint8_t* row, int x0, int xlo, int xhi, int n, uint32_t ww, uint32_t fw) {
    uint32_t o = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int xc = min(max(x0 + j, xlo), xhi);
        uint32_t inner = 0;
#pragma unroll
        for (int i = -R; i <= R; ++i) inner += row[min(max(xc + i, 0), n - 1)];
        const uint32_t far = (uint32_t)row[min(max(xc - R - 1, 0), n - 1)] + (uint32_t)row[min(max(xc + R + 1, 0), n - 1)];
        o |= box24(inner, far, ww, fw) << (8 * j);
    }
    return o;
}
// four outputs of a column pass: rows yc - R - 1 .. yc + R + 1 of one word column (`col` = its word in row 0, rows kBlurDw words apart)
template <int R>
__device__ __forceinline__ uint32_t box4_col(const uint32_t* col, int yc, int rows, uint32_t ww, uint32_t fw) {
    uint32_t in_e = 0, in_o = 0, far_e = 0, far_o = 0;       // bytes 0 | 2 and bytes 1 | 3 as two 16-bit sums (at most 7 x 255)
#pragma unroll
    for (int i = -R - 1; i <= R + 1; ++i) {
        const uint32_t w = col[min(max(yc + i, 0), rows - 1) * kBlurDw];
        if (i == -R - 1 || i == R + 1) { far_e += w & 0x00FF00FFu; far_o += (w >> 8) & 0x00FF00FFu; }
        else { in_e += w & 0x00FF00FFu; in_o += (w >> 8) & 0x00FF00FFu; }
    }
    return box24(in_e & 0xFFFFu, far_e & 0xFFFFu, ww, fw) | (box24(in_o & 0xFFFFu, far_o & 0xFFFFu, ww, fw) << 8) |
           (box24(in_e >> 16, far_e >> 16, ww, fw) << 16) | (box24(in_o >> 16, far_o >> 16, ww, fw) << 24);
}

typedef uint32_t BlurImage[3][kBlurRows][kBlurDw];

// word t + 256 of a plane of NDW words per row from word t, without a division
template <int NDW>
__device__ __forceinline__ void next_word(int& ry, int& d) {
    d += 256 % NDW;
    ry += 256 / NDW;
    if (d >= NDW) { d -= NDW; ++ry; }
}

// One tile at box radius R (-1: no blur, no halo, no pass), so that the region's size divides by constants: load the padded region,
// run the six passes (they start from img[0] and end there), gray, store.
template <int R>
__device__ __forceinline__ void blur_tile(BlurImage* img, const uint8_t* __restrict__ inf, uint8_t* __restrict__ of, int H, int W, int r0,
                                          int c0, uint32_t ww, uint32_t fw, int gray, int vec, int tid) {
    constexpr int hal = 3 * (R + 1), hal4 = (hal + 3) & ~3, dw0 = hal4 / 4;
    constexpr int rows = kBlurH + 2 * hal, ndw = (kBlurW + 2 * hal4) / 4, tdw = kBlurW / 4;
    static_assert(rows <= kBlurRows && ndw <= kBlurDw, "the region fits the image");
    const int y_org = r0 - hal, x_org = c0 - hal4;            // frame position of the region's first row and column
    const int xlo = -x_org, xhi = W - 1 - x_org, ylo = -y_org, yhi = H - 1 - y_org;      // the frame in region columns and rows
    const size_t plane = (size_t)H * W;

    // a thread's words of one plane are (ry, d) = (t / ndw, t % ndw) for t = tid, tid + 256, ...; every task covers the three channels
    const int ry_first = tid / ndw, d_first = tid % ndw;
    for (int ry = ry_first, d = d_first; ry < rows; next_word<ndw>(ry, d)) {
        const int y = min(max(y_org + ry, 0), H - 1), x = x_org + 4 * d;
        const uint8_t* src = inf + (size_t)y * W;
        uint32_t v[3];
        if (vec && x >= 0 && x + 3 < W) {
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = *reinterpret_cast<const uint32_t*>(src + (size_t)c * plane + x);
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                v[c] = 0;
#pragma unroll
                for (int k = 0; k < 4; ++k) v[c] |= (uint32_t)src[(size_t)c * plane + min(max(x + k, 0), W - 1)] << (8 * k);
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) img[0][c][ry][d] = v[c];
    }
    __syncthreads();
    if constexpr (R >= 0) {
        int cur = 0;
        for (int pass = 0; pass < 3; ++pass) {
            for (int ry = ry_first, d = d_first; ry < rows; next_word<ndw>(ry, d)) {
                const bool inside = 4 * d >= xlo && 4 * d + 3 <= xhi;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const uint32_t* row = img[cur][c][ry];
                    uint32_t o;
                    if (inside) o = box4_row<R>(row[max(d - 1, 0)], row[d], row[min(d + 1, ndw - 1)], ww, fw);
                    else o = box4_row_edge<R>(reinterpret_cast<const uint8_t*>(row), 4 * d, xlo, xhi, 4 * ndw, ww, fw);
                    img[cur ^ 1][c][ry][d] = o;
                }
            }
            __syncthreads();
            cur ^= 1;
        }
        // a column pass is exact R + 1 rows further inside than its input: only those rows are computed (and read by the next)
        for (int pass = 0; pass < 3; ++pass) {
            const int lo = (pass + 1) * (R + 1), n = (rows - 2 * lo) * tdw;
            for (int t = tid; t < 3 * n; t += 256) {
                const int c = (t >= n) + (t >= 2 * n), rem = t - c * n, ry = lo + rem / tdw, d = dw0 + rem % tdw;
                img[cur ^ 1][c][ry][d] = box4_col<R>(&img[cur][c][0][d], min(max(ry, ylo), yhi), rows, ww, fw);
            }
            __syncthreads();
            cur ^= 1;
        }
    }
    for (int t = tid; t < kBlurH * tdw; t += 256) {
        const int ry = t / tdw, dd = t % tdw;
        const int y = r0 + ry, x = c0 + 4 * dd;
        if (y >= H || x >= W) continue;
        uint32_t w[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) w[c] = img[0][c][hal + ry][dw0 + dd];
        if (gray) {
            uint32_t g = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int px[3] = {(int)((w[0] >> (8 * k)) & 255u), (int)((w[1] >> (8 * k)) & 255u), (int)((w[2] >> (8 * k)) & 255u)};
                g |= (uint32_t)gray_u8(px) << (8 * k);
            }
            w[0] = w[1] = w[2] = g;
        }
        if (vec) {          // W is a multiple of 4: the word lies inside the row
#pragma unroll
            for (int c = 0; c < 3; ++c) *reinterpret_cast<uint32_t*>(of + (size_t)c * plane + (size_t)y * W + x) = w[c];
        } else {
            const int n = min(4, W - x);
            for (int c = 0; c < 3; ++c)
                for (int k = 0; k < n; ++k) of[(size_t)c * plane + (size_t)y * W + x + k] = (uint8_t)(w[c] >> (8 * k));
        }
    }
}

// `vec`: every plane of `in` and `out` starts on a 4-byte boundary and W is a multiple of 4
__global__ __launch_bounds__(256) void clip_blur_kernel(const uint8_t* __restrict__ in, const Post* __restrict__ table, int H, int W,
                                                        uint8_t* __restrict__ out, int tiles_x, int tiles, int vec) {
    __shared__ BlurImage img[2];
    const int tid = threadIdx.x;
    const int f = blockIdx.x / tiles, tile = blockIdx.x % tiles;
    const int r0 = (tile / tiles_x) * kBlurH, c0 = (tile % tiles_x) * kBlurW;
    const Post p = post_sanitize(table[f]);
    // -1 .. 3, the same in every thread of the workgroup; ww = 2^24 leaves fw = 0: every pass is the identity, as no blur is
    const int r = p.blur_ww >= (1u << 24) ? -1 : p.blur_r;
    const uint8_t* inf = in + (size_t)f * 3 * H * W;
    uint8_t* of = out + (size_t)f * 3 * H * W;
    switch (r) {
        case 0: blur_tile<0>(img, inf, of, H, W, r0, c0, p.blur_ww, p.blur_fw, p.gray, vec, tid); break;
        case 1: blur_tile<1>(img, inf, of, H, W, r0, c0, p.blur_ww, p.blur_fw, p.gray, vec, tid); break;
        case 2: blur_tile<2>(img, inf, of, H, W, r0, c0, p.blur_ww, p.blur_fw, p.gray, vec, tid); break;
        case 3: blur_tile<3>(img, inf, of, H, W, r0, c0, p.blur_ww, p.blur_fw, p.gray, vec, tid); break;
        default: blur_tile<-1>(img, inf, of, H, W, r0, c0, 0u, 0u, p.gray, vec, tid); break;
    }
}

// pixels 4 q .. 4 q + 3 of a frame's plane per thread; `vec` = the planes of `out` are 4-byte aligned and a multiple of 4 long
__global__ __launch_bounds__(256) void clip_rotate_kernel(const uint8_t* __restrict__ in, const Post* __restrict__ table, int H, int W,
                                                          uint8_t* __restrict__ out, int chunks, int vec) {
    const int f = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
    const int plane = H * W;
    const int q = (chunk * 256 + threadIdx.x) * 4;
    if (q >= plane) return;
    const Post p = table[f];
    const uint8_t* inf = in + (size_t)f * 3 * plane;
    uint8_t* of = out + (size_t)f * 3 * plane;
    const int n = min(4, plane - q);
    uint32_t w[3] = {0, 0, 0};
    int y = q / W, x = q - y * W;
    // rot_source's two sums, stepped: a0 and a3 per pixel, a1 and a4 per row, in the same wrapping arithmetic (so the same bits)
    uint32_t row_x = (uint32_t)p.rot[2] + (uint32_t)p.rot[1] * (uint32_t)y, row_y = (uint32_t)p.rot[5] + (uint32_t)p.rot[4] * (uint32_t)y;
    uint32_t sx = row_x + (uint32_t)p.rot[0] * (uint32_t)x, sy = row_y + (uint32_t)p.rot[3] * (uint32_t)x;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (i < n) {
            const int xin = p.rotate ? (int32_t)sx >> 16 : x, yin = p.rotate ? (int32_t)sy >> 16 : y;
            if (xin >= 0 && xin < W && yin >= 0 && yin < H) {
                const uint8_t* s = inf + (size_t)yin * W + xin;
#pragma unroll
                for (int c = 0; c < 3; ++c) w[c] |= (uint32_t)s[(size_t)c * plane] << (8 * i);
            }
            sx += (uint32_t)p.rot[0]; sy += (uint32_t)p.rot[3];
            if (++x == W) {
                x = 0; ++y;
                row_x += (uint32_t)p.rot[1]; row_y += (uint32_t)p.rot[4];
                sx = row_x; sy = row_y;
            }
        }
    }
    if (vec) {
#pragma unroll
        for (int c = 0; c < 3; ++c) *reinterpret_cast<uint32_t*>(of + (size_t)c * plane + q) = w[c];
    } else {
        for (int c = 0; c < 3; ++c)
            for (int i = 0; i < n; ++i) of[(size_t)c * plane + q + i] = (uint8_t)(w[c] >> (8 * i));
    }
}

static int blur_tiles(int H, int W) { return ((H + kBlurH - 1) / kBlurH) * ((W + kBlurW - 1) / kBlurW); }

static bool ranges_overlap(const void* a, const void* b, size_t n) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + n && y < x + n;
}

// what the table asks for; refuses what the kernels would have to clamp
static int check_post(const char* who, const void* in, const Post* table, int F, int H, int W, const void* out, bool* blur, bool* rotate) {
    BVC_REQUIRE(in && table && out, "%s: null argument", who);
    BVC_REQUIRE(F >= 1 && H >= 1 && W >= 1, "%s: empty input", who);
    BVC_REQUIRE((int64_t)H * W <= (1 << 24), "%s: frame too large", who);
    BVC_REQUIRE((int64_t)F * ((int64_t)H * W / 1024 + 1 + blur_tiles(H, W)) < (1ll << 30), "%s: too many frames", who);
    BVC_REQUIRE(!ranges_overlap(in, out, (size_t)F * 3 * H * W), "%s: in and out overlap", who);
    *blur = *rotate = false;
    char msg[512];
    for (int f = 0; f < F; ++f) {
        if (invalid_post(table[f], f, H, W, msg, sizeof(msg))) {
            set_error("%s", msg);
            return BVC_ERR_INVALID;
        }
        if (table[f].blur_r >= 0 || table[f].gray) *blur = true;
        if (table[f].rotate) *rotate = true;
    }
    return BVC_OK;
}

}  // namespace aug
}  // namespace bvc

using namespace bvc;

extern "C" {

int64_t bvc_op_clip_transform_workspace(int F_out, int Ho, int Wo) {
    if (F_out < 1 || Ho < 1 || Wo < 1) return 0;
    return (int64_t)F_out * (2 + aug::tiles_of(Ho, Wo)) * (int64_t)sizeof(uint32_t);      // [F_out][2] precisions | [F_out][tiles] gray sums
}

int bvc_op_clip_transform(const uint8_t* src_dev, int F_src, int channels, int Hs, int Ws, const bvc_frame_aug* table_host,
                          const bvc_frame_aug* table_dev, int F_out, int Ho, int Wo, uint8_t* out_dev, void* workspace_dev, void* stream) {
    bool second = false;
    BVC_REQUIRE(table_dev && workspace_dev && ((uintptr_t)workspace_dev % 4) == 0, "op_clip_transform: null table or workspace, or a workspace off 4-byte alignment");
    const int rc = aug::check_call("op_clip_transform", src_dev, F_src, channels, Hs, Ws, table_host, F_out, Ho, Wo, out_dev, &second);
    if (rc != BVC_OK) return rc;
    const int tiles_x = (Wo + aug::kTile - 1) / aug::kTile, tiles = aug::tiles_of(Ho, Wo);
    int* prec = (int*)workspace_dev;
    uint32_t* partial = (uint32_t*)workspace_dev + 2 * (size_t)F_out;
    hipLaunchKernelGGL(aug::clip_precision_kernel, dim3((unsigned)F_out), dim3(256), 0, (hipStream_t)stream, table_dev, F_src, Hs, Ws, Ho, Wo,
                       prec);
    BVC_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(aug::clip_resize_kernel, dim3((unsigned)(F_out * tiles)), dim3(256), 0, (hipStream_t)stream, src_dev, F_src, Hs, Ws,
                       table_dev, Ho, Wo, out_dev, prec, partial, tiles_x, tiles);
    BVC_CHECK_HIP(hipGetLastError());
    if (second) {
        const int plane = Ho * Wo, chunks = (plane + 1023) / 1024;
        const int vec = plane % 4 == 0 && ((uintptr_t)out_dev % 4) == 0;
        hipLaunchKernelGGL(aug::clip_colour_kernel, dim3((unsigned)(F_out * chunks)), dim3(256), 0, (hipStream_t)stream, table_dev, Ho, Wo,
                           out_dev, partial, tiles, chunks, vec);
        BVC_CHECK_HIP(hipGetLastError());
    }
    return BVC_OK;
}

int bvc_clip_transform_host(const uint8_t* src, int F_src, int channels, int Hs, int Ws, const bvc_frame_aug* table, int F_out, int Ho,
                            int Wo, uint8_t* out) {
    bool second = false;
    const int rc = aug::check_call("clip_transform_host", src, F_src, channels, Hs, Ws, table, F_out, Ho, Wo, out, &second);
    if (rc != BVC_OK) return rc;
    aug::clip_transform_host(src, F_src, Hs, Ws, table, F_out, Ho, Wo, out);
    return BVC_OK;
}

int bvc_aug_blur_weights(float radius, int32_t* r, uint32_t* ww, uint32_t* fw) {
    BVC_REQUIRE(r && ww && fw, "aug_blur_weights: null argument");
    BVC_REQUIRE(aug::blur_weights(radius, r, ww, fw) == 0, "aug_blur_weights: radius %g outside [0, %g]", (double)radius,
                (double)BVC_AUG_MAX_BLUR_RADIUS);
    return BVC_OK;
}

int64_t bvc_op_clip_post_workspace(int F, int H, int W) {
    if (F < 1 || H < 1 || W < 1) return 0;
    return (int64_t)F * 3 * H * W;      // the frames between the blur and the rotation kernel
}

int bvc_op_clip_post(const uint8_t* in_dev, const bvc_frame_post* table_host, const bvc_frame_post* table_dev, int F, int H, int W,
                     uint8_t* out_dev, void* workspace_dev, void* stream) {
    bool blur = false, rotate = false;
    BVC_REQUIRE(table_dev, "op_clip_post: null device table");
    const int rc = aug::check_post("op_clip_post", in_dev, table_host, F, H, W, out_dev, &blur, &rotate);
    if (rc != BVC_OK) return rc;
    const size_t bytes = (size_t)F * 3 * H * W;
    if (!blur && !rotate) {      // the identity everywhere: one copy
        BVC_CHECK_HIP(hipMemcpyAsync(out_dev, in_dev, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
        return BVC_OK;
    }
    uint8_t* mid = (uint8_t*)workspace_dev;
    if (blur && rotate)
        BVC_REQUIRE(mid && !aug::ranges_overlap(mid, in_dev, bytes) && !aug::ranges_overlap(mid, out_dev, bytes),
                    "op_clip_post: blur and rotation in one call need a workspace that overlaps neither in nor out");
    if (blur) {
        uint8_t* dst = rotate ? mid : out_dev;
        const int tiles_x = (W + aug::kBlurW - 1) / aug::kBlurW, tiles = aug::blur_tiles(H, W);
        const int vec = W % 4 == 0 && ((uintptr_t)in_dev % 4) == 0 && ((uintptr_t)dst % 4) == 0;
        hipLaunchKernelGGL(aug::clip_blur_kernel, dim3((unsigned)(F * tiles)), dim3(256), 0, (hipStream_t)stream, in_dev, table_dev, H, W, dst,
                           tiles_x, tiles, vec);
        BVC_CHECK_HIP(hipGetLastError());
    }
    if (rotate) {
        const uint8_t* src = blur ? mid : in_dev;
        const int plane = H * W, chunks = (plane + 1023) / 1024;
        const int vec = plane % 4 == 0 && ((uintptr_t)out_dev % 4) == 0;
        hipLaunchKernelGGL(aug::clip_rotate_kernel, dim3((unsigned)(F * chunks)), dim3(256), 0, (hipStream_t)stream, src, table_dev, H, W,
                           out_dev, chunks, vec);
        BVC_CHECK_HIP(hipGetLastError());
    }
    return BVC_OK;
}

int bvc_clip_post_host(const uint8_t* in, const bvc_frame_post* table, int F, int H, int W, uint8_t* out) {
    bool blur = false, rotate = false;
    const int rc = aug::check_post("clip_post_host", in, table, F, H, W, out, &blur, &rotate);
    if (rc != BVC_OK) return rc;
    aug::clip_post_host(in, table, F, H, W, out);
    return BVC_OK;
}

}  // extern "C"

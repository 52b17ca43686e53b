// Clip transforms on uint8 frames (include/bvc.h, bvc_frame_aug; arithmetic in augment.h): resize + crop + flip + colour jitter.
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

}  // extern "C"

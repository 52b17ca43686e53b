// RandAugment on uint8 frames (include/bvc.h, bvc_frame_randaug; arithmetic in randaug.h).  The host walks the stage index
// s = 0 .. max nops - 1; per stage at most three launches, and only frames that have a stage s take part in them:
//
// randaug_hist_kernel   only when some frame's stage s is AutoContrast, Equalize or Contrast: one workgroup per 16384 pixels of such
//                       a frame (the others exit before they read anything) counts its three channels - or L, for Contrast - into
//                       256-bin histograms in LDS with integer LDS atomics and adds the non-empty bins to the frame's [3][256] uint32
//                       histograms in the workspace with integer global atomics.  Integer adds commute: any order gives the same bits.
// randaug_lut_kernel    one workgroup per such frame, one thread per bin: lo / hi / the prefix sums of the histogram -> the frame's
//                       [3][256] byte tables (randaug.h's f64 expressions, evaluated here), and the histograms zeroed again for the
//                       next statistics stage.
// randaug_apply_kernel  one workgroup per 4096 pixels of a frame, 16 consecutive pixels of each plane per thread, by op class:
//                       table look-up (the table copied or, for the ops that need no statistics, built in LDS), colour blend,
//                       3 x 3 blend, gather (that one in four sweeps of 4 pixels per thread).  Reads the frame where the stage before left it and writes the other buffer.
//
// Buffers: frame f with n stages writes stage s to `out` when n - 1 - s is even and to the workspace frames when it is odd, and reads
// what stage s - 1 wrote (stage 0 reads `in`): the last stage always lands in `out`, with one spare buffer, whatever n is.  A frame
// without stages is copied by the apply kernel of stage 0.
#include "randaug.h"
#include "common.h"

namespace bvc {
namespace ra {

constexpr int kPix = 16;                      // pixels of one plane per thread
constexpr int kChunk = 256 * kPix;            // per workgroup of the apply kernel
constexpr int kHistRounds = 4;                // chunks per workgroup of the histogram kernel
constexpr int kHistBytes = 3 * 256 * 4, kLutBytes = 3 * 256;       // per frame, in the workspace

struct Px16 { uint32_t w[4]; };
__device__ __forceinline__ int byte_of(const Px16& p, int i) { return (int)((p.w[i >> 2] >> (8 * (i & 3))) & 255u); }
__device__ __forceinline__ void or_byte(Px16& p, int i, int v) { p.w[i >> 2] |= (uint32_t)v << (8 * (i & 3)); }

// n <= 16 bytes at p.  vec = 16: p is 16-byte aligned and n = 16; vec = 4: p is 4-byte aligned and n a multiple of 4; else bytes
__device__ __forceinline__ Px16 load16(const uint8_t* p, int n, int vec) {
    Px16 r = {{0u, 0u, 0u, 0u}};
    if (vec == 16) {
        const uint4 v = *reinterpret_cast<const uint4*>(p);
        r.w[0] = v.x; r.w[1] = v.y; r.w[2] = v.z; r.w[3] = v.w;
    } else if (vec == 4) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (4 * k < n) r.w[k] = *reinterpret_cast<const uint32_t*>(p + 4 * k);
    } else {
#pragma unroll
        for (int i = 0; i < kPix; ++i)
            if (i < n) or_byte(r, i, p[i]);
    }
    return r;
}
__device__ __forceinline__ void store16(uint8_t* p, const Px16& r, int n, int vec) {
    if (vec == 16) {
        *reinterpret_cast<uint4*>(p) = make_uint4(r.w[0], r.w[1], r.w[2], r.w[3]);
    } else if (vec == 4) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (4 * k < n) *reinterpret_cast<uint32_t*>(p + 4 * k) = r.w[k];
    } else {
#pragma unroll
        for (int i = 0; i < kPix; ++i)
            if (i < n) p[i] = (uint8_t)byte_of(r, i);
    }
}

// where stage s of frame f (n stages; n = 0 runs the copy as its stage 0) reads and writes
__device__ __forceinline__ void stage_buffers(const uint8_t* in, uint8_t* out, uint8_t* work, int f, size_t frame, int n, int s,
                                              const uint8_t** src, uint8_t** dst) {
    const bool to_out = n == 0 || ((n - 1 - s) & 1) == 0;
    *dst = (to_out ? out : work) + (size_t)f * frame;
    *src = (s == 0 ? in : (to_out ? work : out)) + (size_t)f * frame;
}

__global__ __launch_bounds__(256) void randaug_hist_kernel(const uint8_t* __restrict__ in, uint8_t* out, uint8_t* work,
                                                           const Entry* __restrict__ table, int s, int H, int W, uint32_t* __restrict__ hist,
                                                           int chunks, int vec) {
    __shared__ uint32_t h[3][256];
    const int tid = threadIdx.x;
    const int f = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
    const int n = sanitize_nops(table[f].nops);
    if (s >= n) return;
    const int op = sanitize_stage(table[f].stage[s]).op;
    if (!is_stat(op)) return;
    const int plane = H * W;
    const uint8_t* sf;
    uint8_t* unused;
    stage_buffers(in, out, work, f, (size_t)3 * plane, n, s, &sf, &unused);
#pragma unroll
    for (int c = 0; c < 3; ++c) h[c][tid] = 0u;
    __syncthreads();
    for (int it = 0; it < kHistRounds; ++it) {
        const int q = (chunk * kHistRounds + it) * kChunk + tid * kPix;
        if (q >= plane) break;
        const int cnt = min(kPix, plane - q);
        Px16 v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = load16(sf + (size_t)c * plane + q, cnt, vec);
#pragma unroll
        for (int i = 0; i < kPix; ++i) {
            if (i < cnt) {
                if (op == OP_CONTRAST) {
                    atomicAdd(&h[0][luma_u8(byte_of(v[0], i), byte_of(v[1], i), byte_of(v[2], i))], 1u);
                } else {
#pragma unroll
                    for (int c = 0; c < 3; ++c) atomicAdd(&h[c][byte_of(v[c], i)], 1u);
                }
            }
        }
    }
    __syncthreads();
    uint32_t* hf = hist + (size_t)f * 3 * 256;
    for (int c = 0; c < (op == OP_CONTRAST ? 1 : 3); ++c) {
        const uint32_t v = h[c][tid];
        if (v) atomicAdd(&hf[c * 256 + tid], v);
    }
}

// inclusive prefix sum over the workgroup's 256 values, through `sh`; every thread receives its own sum and *total the last one.  The
// sums stay in sh[0] (eight steps: the last one writes there) until the next call.
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t (*sh)[256], uint32_t* total) {
    const int tid = threadIdx.x;
    int cur = 0;
    sh[0][tid] = v;
    __syncthreads();
#pragma unroll
    for (int o = 1; o < 256; o <<= 1) {
        const uint32_t t = sh[cur][tid] + (tid >= o ? sh[cur][tid - o] : 0u);
        sh[cur ^ 1][tid] = t;
        __syncthreads();
        cur ^= 1;
    }
    const uint32_t r = sh[cur][tid];
    *total = sh[cur][255];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(256) void randaug_lut_kernel(const Entry* __restrict__ table, int s, int H, int W, uint32_t* __restrict__ hist,
                                                          uint8_t* __restrict__ luts) {
    __shared__ uint32_t sh[2][256];
    __shared__ int lo, hi, nz;
    const int tid = threadIdx.x, f = blockIdx.x;
    if (s >= sanitize_nops(table[f].nops)) return;
    const Stage st = sanitize_stage(table[f].stage[s]);
    if (!is_stat(st.op)) return;
    uint32_t* hf = hist + (size_t)f * 3 * 256;
    uint8_t* lf = luts + (size_t)f * kLutBytes;
    const uint32_t count = (uint32_t)(H * W);
    if (st.op == OP_CONTRAST) {
        const uint32_t hv = hf[tid];
        hf[tid] = 0u;
        uint32_t sum;
        block_scan((uint32_t)tid * hv, sh, &sum);       // at most 255 * 2^24: inside uint32
        const int v = blend_u8(contrast_mean(sum, count), tid, st.fval);
#pragma unroll
        for (int c = 0; c < 3; ++c) lf[c * 256 + tid] = (uint8_t)v;
        return;
    }
    for (int c = 0; c < 3; ++c) {
        const uint32_t hv = hf[c * 256 + tid];
        hf[c * 256 + tid] = 0u;
        if (tid == 0) { lo = 256; hi = -1; nz = 0; }
        __syncthreads();
        if (hv) { atomicMin(&lo, tid); atomicMax(&hi, tid); atomicAdd(&nz, 1); }
        uint32_t total;
        const uint32_t upto = block_scan(hv, sh, &total);      // its barriers also publish lo, hi, nz
        int v;
        if (st.op == OP_AUTOCONTRAST) {
            v = autocontrast_lut(tid, lo, hi);
        } else {
            const uint32_t last = hi > 0 ? total - sh[0][hi - 1] : total;      // the last non-empty bin: everything from it on
            v = equalize_lut(tid, upto - hv, equalize_step(nz, total, last));
        }
        lf[c * 256 + tid] = (uint8_t)v;
        __syncthreads();      // lo, hi, nz and sh[0] are read before the next channel overwrites them
    }
}

// Pixels q .. q + 3 of a frame's planes through the 16.16 map: rot_source's two sums, stepped as clip_rotate_kernel steps them (a0 and
// a3 per pixel, a1 and a4 per row, the same wrapping arithmetic, so the same bits).  Four pixels per thread, not sixteen: a wave's
// loads then cover 256 neighbouring output pixels, whose sources lie close together.  vec >= 4: the planes are whole aligned words.
__device__ __forceinline__ void gather4(const uint8_t* __restrict__ sf, uint8_t* __restrict__ df, const int32_t* a, const uint32_t* fc, int q,
                                        int H, int W, int vec) {
    const int plane = H * W, n = min(4, plane - q);
    uint32_t w[3] = {0u, 0u, 0u};
    int y = q / W, x = q - y * W;
    uint32_t row_x = (uint32_t)a[2] + (uint32_t)a[1] * (uint32_t)y, row_y = (uint32_t)a[5] + (uint32_t)a[4] * (uint32_t)y;
    uint32_t sx = row_x + (uint32_t)a[0] * (uint32_t)x, sy = row_y + (uint32_t)a[3] * (uint32_t)x;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (i < n) {
            const int xin = (int32_t)sx >> 16, yin = (int32_t)sy >> 16;
            const bool inside = xin >= 0 && xin < W && yin >= 0 && yin < H;
            const uint8_t* p = sf + (inside ? (size_t)yin * W + xin : (size_t)0);
#pragma unroll
            for (int c = 0; c < 3; ++c) w[c] |= (inside ? (uint32_t)p[(size_t)c * plane] : fc[c]) << (8 * i);
            sx += (uint32_t)a[0]; sy += (uint32_t)a[3];
            if (++x == W) {
                x = 0; ++y;
                row_x += (uint32_t)a[1]; row_y += (uint32_t)a[4];
                sx = row_x; sy = row_y;
            }
        }
    }
    if (vec >= 4) {
#pragma unroll
        for (int c = 0; c < 3; ++c) *reinterpret_cast<uint32_t*>(df + (size_t)c * plane + q) = w[c];
    } else {
        for (int c = 0; c < 3; ++c)
            for (int i = 0; i < n; ++i) df[(size_t)c * plane + q + i] = (uint8_t)(w[c] >> (8 * i));
    }
}

__global__ __launch_bounds__(256) void randaug_apply_kernel(const uint8_t* __restrict__ in, uint8_t* out, uint8_t* work,
                                                            const Entry* __restrict__ table, const uint8_t* __restrict__ luts, int s, int H,
                                                            int W, int chunks, int vec) {
    __shared__ uint8_t lut[3][256];
    const int tid = threadIdx.x;
    const int f = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
    const int n = sanitize_nops(table[f].nops);
    if (s >= n && !(n == 0 && s == 0)) return;
    Stage st = {};
    if (n == 0) st.op = OP_COPY;
    else st = sanitize_stage(table[f].stage[s]);
    const int op = st.op;      // the same in every thread of the workgroup
    const int plane = H * W;
    const uint8_t* sf;
    uint8_t* df;
    stage_buffers(in, out, work, f, (size_t)3 * plane, n, s, &sf, &df);
    if (is_lut(op)) {
        if (is_stat(op)) {
#pragma unroll
            for (int c = 0; c < 3; ++c) lut[c][tid] = luts[(size_t)f * kLutBytes + c * 256 + tid];
        } else {
            const uint8_t v = (uint8_t)param_lut(st, tid);
            lut[0][tid] = lut[1][tid] = lut[2][tid] = v;
        }
        __syncthreads();
    }
    if (is_affine(op)) {      // the workgroup's pixels in four sweeps of 4 per thread
        const uint8_t* fill = table[f].fill;
        const uint32_t fc[3] = {fill[0], fill[1], fill[2]};
#pragma unroll
        for (int k = 0; k < kPix / 4; ++k) {
            const int q4 = chunk * kChunk + (k * 256 + tid) * 4;
            if (q4 < plane) gather4(sf, df, st.aff, fc, q4, H, W, vec);
        }
        return;
    }
    const int q = (chunk * 256 + tid) * kPix;
    if (q >= plane) return;
    const int cnt = min(kPix, plane - q);

    if (is_lut(op) || op == OP_COPY) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const Px16 v = load16(sf + (size_t)c * plane + q, cnt, vec);
            Px16 o = v;
            if (op != OP_COPY) {
                o = Px16{{0u, 0u, 0u, 0u}};
#pragma unroll
                for (int i = 0; i < kPix; ++i) or_byte(o, i, lut[c][byte_of(v, i)]);      // bytes beyond cnt are not stored
            }
            store16(df + (size_t)c * plane + q, o, cnt, vec);
        }
    } else if (op == OP_COLOR) {
        Px16 v[3], o[3] = {{{0u, 0u, 0u, 0u}}, {{0u, 0u, 0u, 0u}}, {{0u, 0u, 0u, 0u}}};
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = load16(sf + (size_t)c * plane + q, cnt, vec);
#pragma unroll
        for (int i = 0; i < kPix; ++i) {
            const int L = luma_u8(byte_of(v[0], i), byte_of(v[1], i), byte_of(v[2], i));
#pragma unroll
            for (int c = 0; c < 3; ++c) or_byte(o[c], i, blend_u8(L, byte_of(v[c], i), st.fval));
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) store16(df + (size_t)c * plane + q, o[c], cnt, vec);
    } else if (op == OP_SHARPNESS) {
        const int y0 = q / W, x0 = q - y0 * W;
        const bool one_inner_row = x0 + cnt <= W && W >= 3 && y0 >= 1 && y0 + 1 < H;
        for (int c = 0; c < 3; ++c) {
            const uint8_t* pl = sf + (size_t)c * plane;
            Px16 o = {{0u, 0u, 0u, 0u}};
            if (one_inner_row) {
                // the run and one column on either side, of three rows, as six words per row with the run in words 1 .. 4: column
                // x0 - 1 + j is byte j + 3.  Columns beyond the frame only serve pixels that are copied.
                uint32_t rw[3][6];
                const uint8_t* row = pl + (size_t)y0 * W;
                if (vec >= 4 && W % 4 == 0 && cnt == kPix) {
                    // whole words: the run starts on a word of its row (16 | q and 4 | W), the word before it exists when x0 >= 4
                    // and the one after it when the run ends before the row does
                    const int mid_vec = vec == 16 && W % 16 == 0 ? 16 : 4;
#pragma unroll
                    for (int r = 0; r < 3; ++r) {
                        const uint8_t* rp = row + (ptrdiff_t)(r - 1) * W + x0;
                        rw[r][0] = x0 >= 4 ? *reinterpret_cast<const uint32_t*>(rp - 4) : 0u;
                        rw[r][5] = x0 + kPix < W ? *reinterpret_cast<const uint32_t*>(rp + kPix) : 0u;
                        const Px16 mid = load16(rp, kPix, mid_vec);
#pragma unroll
                        for (int k = 0; k < 4; ++k) rw[r][1 + k] = mid.w[k];
                    }
                } else {
#pragma unroll
                    for (int r = 0; r < 3; ++r) {
#pragma unroll
                        for (int k = 0; k < 6; ++k) rw[r][k] = 0u;
#pragma unroll
                        for (int j = 0; j < kPix + 2; ++j) {
                            if (j < cnt + 2) {
                                const int xj = min(max(x0 - 1 + j, 0), W - 1);
                                rw[r][(j + 3) >> 2] |= (uint32_t)row[(ptrdiff_t)(r - 1) * W + xj] << (8 * ((j + 3) & 3));
                            }
                        }
                    }
                }
                auto at = [&](int r, int j) { return (int)((rw[r][(j + 3) >> 2] >> (8 * ((j + 3) & 3))) & 255u); };
#pragma unroll
                for (int i = 0; i < kPix; ++i) {
                    if (i < cnt) {
                        const int x = x0 + i, v = at(1, i + 1);
                        const int d = x >= 1 && x + 1 < W ? smooth9_u8(at(0, i), at(0, i + 1), at(0, i + 2), at(1, i), v, at(1, i + 2), at(2, i),
                                                                       at(2, i + 1), at(2, i + 2))
                                                          : v;
                        or_byte(o, i, blend_u8(d, v, st.fval));
                    }
                }
            } else {
                int y = y0, x = x0;
#pragma unroll
                for (int i = 0; i < kPix; ++i) {
                    if (i < cnt) {
                        const uint8_t* p = pl + (size_t)y * W + x;
                        const bool inner = y >= 1 && y + 1 < H && x >= 1 && x + 1 < W;
                        const int v = *p;
                        const int d = inner ? smooth_u8(p - W - 1, p - 1, p + W - 1) : v;
                        or_byte(o, i, blend_u8(d, v, st.fval));
                        if (++x == W) { x = 0; ++y; }
                    }
                }
            }
            store16(df + (size_t)c * plane + q, o, cnt, vec);
        }
    }
}

static bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + nb && y < x + na;
}

static int apply_chunks(int H, int W) { return (H * W + kChunk - 1) / kChunk; }

// what the table asks for; refuses what the kernels would have to clamp.  stat[s]: some frame's stage s needs statistics
static int check_call(const char* who, const void* in, const Entry* table, int F, int H, int W, const void* out, int* max_nops,
                      bool (&stat)[kMaxOps]) {
    BVC_REQUIRE(in && table && out, "%s: null argument", who);
    BVC_REQUIRE(F >= 1 && H >= 1 && W >= 1, "%s: empty input", who);
    BVC_REQUIRE((int64_t)H * W <= (1 << 24), "%s: frame too large", who);
    BVC_REQUIRE((int64_t)F * apply_chunks(H, W) < (1ll << 30), "%s: too many frames", who);
    const size_t bytes = (size_t)F * 3 * H * W;
    BVC_REQUIRE(!ranges_overlap(in, bytes, out, bytes), "%s: in and out overlap", who);
    *max_nops = 0;
    for (int s = 0; s < kMaxOps; ++s) stat[s] = false;
    char msg[512];
    for (int f = 0; f < F; ++f) {
        if (invalid(table[f], f, H, W, msg, sizeof(msg))) {
            set_error("%s", msg);
            return BVC_ERR_INVALID;
        }
        *max_nops = table[f].nops > *max_nops ? table[f].nops : *max_nops;
        for (int s = 0; s < table[f].nops; ++s)
            if (is_stat(table[f].stage[s].op)) stat[s] = true;
    }
    return BVC_OK;
}

}  // namespace ra
}  // namespace bvc

using namespace bvc;

extern "C" {

int bvc_frame_randaug_bytes(void) { return (int)sizeof(bvc_frame_randaug); }

int64_t bvc_op_clip_randaug_workspace(int F, int H, int W) {
    if (F < 1 || H < 1 || W < 1) return 0;
    // [F][3][256] uint32 histograms | [F][3][256] byte tables (together a multiple of 16 bytes per frame) | the spare frames
    return (int64_t)F * (ra::kHistBytes + ra::kLutBytes) + (int64_t)F * 3 * H * W;
}

int bvc_op_clip_randaug(const uint8_t* in_dev, const bvc_frame_randaug* table_host, const bvc_frame_randaug* table_dev, int F, int H, int W,
                        uint8_t* out_dev, void* workspace_dev, void* stream) {
    int max_nops = 0;
    bool stat[ra::kMaxOps];
    BVC_REQUIRE(table_dev, "op_clip_randaug: null device table");
    const int rc = ra::check_call("op_clip_randaug", in_dev, table_host, F, H, W, out_dev, &max_nops, stat);
    if (rc != BVC_OK) return rc;
    const size_t bytes = (size_t)F * 3 * H * W;
    hipStream_t st = (hipStream_t)stream;
    if (max_nops == 0) {      // the identity everywhere: one copy
        BVC_CHECK_HIP(hipMemcpyAsync(out_dev, in_dev, bytes, hipMemcpyDeviceToDevice, st));
        return BVC_OK;
    }
    const size_t need = (size_t)bvc_op_clip_randaug_workspace(F, H, W);
    BVC_REQUIRE(workspace_dev && ((uintptr_t)workspace_dev % 4) == 0, "op_clip_randaug: null workspace, or one off 4-byte alignment");
    BVC_REQUIRE(!ra::ranges_overlap(workspace_dev, need, in_dev, bytes) && !ra::ranges_overlap(workspace_dev, need, out_dev, bytes),
                "op_clip_randaug: the workspace overlaps in or out");
    uint32_t* hist = (uint32_t*)workspace_dev;
    uint8_t* luts = (uint8_t*)workspace_dev + (size_t)F * ra::kHistBytes;
    uint8_t* work = luts + (size_t)F * ra::kLutBytes;
    const int plane = H * W, chunks = ra::apply_chunks(H, W), hchunks = (chunks + ra::kHistRounds - 1) / ra::kHistRounds;
    const uintptr_t all = (uintptr_t)in_dev | (uintptr_t)out_dev | (uintptr_t)work;
    const int vec = plane % 16 == 0 && all % 16 == 0 ? 16 : (plane % 4 == 0 && all % 4 == 0 ? 4 : 1);
    bool any_stat = false;
    for (int s = 0; s < max_nops; ++s) any_stat = any_stat || stat[s];
    if (any_stat) BVC_CHECK_HIP(hipMemsetAsync(hist, 0, (size_t)F * ra::kHistBytes, st));      // the table kernel leaves them zero again
    for (int s = 0; s < max_nops; ++s) {
        if (stat[s]) {
            hipLaunchKernelGGL(ra::randaug_hist_kernel, dim3((unsigned)(F * hchunks)), dim3(256), 0, st, in_dev, out_dev, work, table_dev, s, H,
                               W, hist, hchunks, vec);
            BVC_CHECK_HIP(hipGetLastError());
            hipLaunchKernelGGL(ra::randaug_lut_kernel, dim3((unsigned)F), dim3(256), 0, st, table_dev, s, H, W, hist, luts);
            BVC_CHECK_HIP(hipGetLastError());
        }
        hipLaunchKernelGGL(ra::randaug_apply_kernel, dim3((unsigned)(F * chunks)), dim3(256), 0, st, in_dev, out_dev, work, table_dev, luts, s,
                           H, W, chunks, vec);
        BVC_CHECK_HIP(hipGetLastError());
    }
    return BVC_OK;
}

int bvc_clip_randaug_host(const uint8_t* in, const bvc_frame_randaug* table, int F, int H, int W, uint8_t* out) {
    int max_nops = 0;
    bool stat[ra::kMaxOps];
    const int rc = ra::check_call("clip_randaug_host", in, table, F, H, W, out, &max_nops, stat);
    if (rc != BVC_OK) return rc;
    ra::clip_randaug_host(in, table, F, H, W, out);
    return BVC_OK;
}

}  // extern "C"

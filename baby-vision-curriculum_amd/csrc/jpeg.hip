// JPEG decode on the device (include/bvc.h, bvc_op_jpeg_decode; arithmetic in jpeg.h).  Two kernels, no coefficient traffic through HBM:
//
// jpeg_entropy_idct_kernel   one lane per segment (a restart interval, or the whole scan of a file without DRI); `lanes` lanes of each
//                            64-wide workgroup are in use, so that a call with few segments spreads them over many waves and a call
//                            with many packs them.  jpeg.h's decode_segment: one Huffman symbol per iteration of the loop - lanes
//                            diverge inside a symbol and when a block completes, not from symbol to symbol - a 64-bit bit buffer
//                            refilled from the lane's own byte range, the current block in LDS at a stride of 65 dwords per lane (the
//                            zig-zag position is a run-time index; 65 is odd, so the lanes' blocks start on different banks),
//                            dequantised as it is decoded, the 8 x 8 IDCT in place, eight 8-byte rows into the component's padded
//                            plane.  The segment's status bits go to one int32 per segment behind the planes.
// jpeg_colour_kernel         one thread per run of 4 output pixels: fancy upsampling, YCbCr -> RGB, crop; 4-byte stores where the run
//                            is whole and aligned.  The first workgroup of every image ORs its segments' status bits (a tree in LDS,
//                            no atomics) into status[image].
#include "jpeg.h"
#include "common.h"

namespace bvc {
namespace jpg {

constexpr int kRun = 4;      // output pixels per thread of the colour kernel

__global__ __launch_bounds__(64) void jpeg_entropy_idct_kernel(const uint8_t* __restrict__ blob, const Info* __restrict__ infos, int n,
                                                               const int32_t* __restrict__ segs, int nseg, int lanes,
                                                               uint8_t* __restrict__ work, int32_t* __restrict__ seg_status) {
    extern __shared__ int32_t lds[];      // lanes x kBlockDwords
    const int lane = threadIdx.x;
    if (lane >= lanes) return;
    const int s = blockIdx.x * lanes + lane;
    if (s >= nseg) return;
    int lo = 0, hi = n - 1;      // the last image whose first segment is not after s (images without segments share their successor's)
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (infos[mid].seg_first <= s) lo = mid; else hi = mid - 1;
    }
    const Info* I = &infos[lo];
    const int32_t* sg = segs + (size_t)kSegInts * s;
    seg_status[s] = decode_segment(I, blob + I->blob_offset, sg[0], sg[1], sg[2], sg[3], lds + lane * kBlockDwords, work + I->plane_offset);
}

__global__ __launch_bounds__(256) void jpeg_colour_kernel(const Info* __restrict__ infos, const uint8_t* __restrict__ work,
                                                          const int32_t* __restrict__ seg_status, const int64_t* __restrict__ out_offsets,
                                                          uint8_t* __restrict__ out, int32_t* __restrict__ status) {
    __shared__ int32_t sh[256];
    const Info* I = &infos[blockIdx.y];
    const int tid = threadIdx.x;
    const bool live = I->reason == 0;
    if (blockIdx.x == 0) {
        int32_t st = 0;
        if (live)
            for (int s = tid; s < I->nseg; s += 256) st |= seg_status[I->seg_first + s];
        sh[tid] = st;
        __syncthreads();
        for (int w = 128; w > 0; w >>= 1) {
            if (tid < w) sh[tid] |= sh[tid + w];
            __syncthreads();
        }
        if (tid == 0) status[blockIdx.y] = live ? (sh[0] | I->flags) : 0;
    }
    if (!live) return;
    const int W = I->width, H = I->height, runs = (W + kRun - 1) / kRun;
    const int t = blockIdx.x * 256 + tid;
    if (t >= H * runs) return;
    const int y = t / runs, x0 = (t % runs) * kRun, cnt = min(kRun, W - x0);
    const uint8_t* planes = work + I->plane_offset;
    uint32_t w[3] = {0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < kRun; ++i) {
        if (i < cnt) {
            int r, g, b;
            pixel_rgb(I, planes, x0 + i, y, &r, &g, &b);
            w[0] |= (uint32_t)r << (8 * i);
            w[1] |= (uint32_t)g << (8 * i);
            w[2] |= (uint32_t)b << (8 * i);
        }
    }
    const size_t plane = (size_t)H * W;
    uint8_t* o = out + out_offsets[blockIdx.y] + (size_t)y * W + x0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        uint8_t* p = o + c * plane;
        if (cnt == kRun && ((uintptr_t)p & 3u) == 0) {
            *reinterpret_cast<uint32_t*>(p) = w[c];
        } else {
#pragma unroll
            for (int i = 0; i < kRun; ++i)
                if (i < cnt) p[i] = (uint8_t)(w[c] >> (8 * i));
        }
    }
}

static int64_t align16(int64_t v) { return (v + 15) & ~(int64_t)15; }

// what parse() promises about an info, checked again on the copy the call is given: every size the kernels derive from it
static bool info_sane(const Info& I) {
    if (I.width < 1 || I.height < 1 || I.width > BVC_JPEG_MAX_DIM || I.height > BVC_JPEG_MAX_DIM) return false;
    if (I.ncomp != 1 && I.ncomp != 3) return false;
    const bool samp = (I.hs == 1 && I.vs == 1) || (I.ncomp == 3 && I.hs == 2 && (I.vs == 1 || I.vs == 2));
    if (!samp) return false;
    if (I.mcus_x != (I.width + 8 * I.hs - 1) / (8 * I.hs) || I.mcus_y != (I.height + 8 * I.vs - 1) / (8 * I.vs)) return false;
    for (int c = 0; c < 3; ++c)
        if (I.tq[c] > 3 || I.td[c] > 1 || I.ta[c] > 1) return false;
    return I.nseg >= 1 && I.scan_begin >= 0 && I.scan_end >= I.scan_begin;
}

}  // namespace jpg
}  // namespace bvc

using namespace bvc;

extern "C" {

int bvc_jpeg_info_bytes(void) { return (int)sizeof(bvc_jpeg_info); }

int bvc_jpeg_parse(const uint8_t* data, int64_t n, bvc_jpeg_info* info, int32_t* seg, int max_seg) {
    BVC_REQUIRE(data && info && n >= 0 && max_seg >= 0 && (seg || max_seg == 0), "jpeg_parse: null argument");
    return jpg::parse(data, n, info, seg, max_seg);
}

int bvc_jpeg_decode_host(const uint8_t* data, int64_t n, const bvc_jpeg_info* info, const int32_t* seg, uint8_t* out_rgb) {
    BVC_REQUIRE(data && info && seg && out_rgb, "jpeg_decode_host: null argument");
    BVC_REQUIRE(info->reason == 0 && jpg::info_sane(*info), "jpeg_decode_host: the info is not one that bvc_jpeg_parse accepted");
    const int total = info->mcus_x * info->mcus_y;
    int next = 0;
    for (int s = 0; s < info->nseg; ++s) {
        const int32_t* g = seg + (size_t)jpg::kSegInts * s;
        BVC_REQUIRE(g[0] >= 0 && g[0] <= g[1] && g[1] <= n && g[2] == next && g[3] >= 1 && g[3] <= total - next,
                    "jpeg_decode_host: segment %d is outside the file or the image", s);
        next += g[3];
    }
    BVC_REQUIRE(next == total, "jpeg_decode_host: the segments do not cover the image");
    return jpg::decode_host(data, info, seg, out_rgb);
}

int64_t bvc_op_jpeg_decode_workspace(bvc_jpeg_info* infos_host, int n) {
    if (!infos_host || n < 1) return 0;
    int64_t at = 0, nseg = 0;
    for (int i = 0; i < n; ++i) {
        bvc_jpeg_info& I = infos_host[i];
        I.plane_offset = at;
        if (I.reason != 0 || !jpg::info_sane(I)) continue;
        at += jpg::align16(jpg::plane_bytes(&I));
        nseg += I.nseg;
    }
    return at + 4 * nseg;      // the planes, then one int32 of status bits per segment
}

int bvc_op_jpeg_decode(const uint8_t* blob_dev, int64_t blob_bytes, const bvc_jpeg_info* infos_host, const bvc_jpeg_info* infos_dev, int n,
                       const int32_t* segs_host, const int32_t* segs_dev, int64_t nseg, const int64_t* out_offsets_host,
                       const int64_t* out_offsets_dev, uint8_t* out_dev, int64_t out_bytes, int32_t* status_dev, void* workspace_dev,
                       int64_t workspace_bytes, int lanes, int stages, void* stream) {
    BVC_REQUIRE(blob_dev && infos_host && infos_dev && out_offsets_host && out_offsets_dev && out_dev && status_dev,
                "op_jpeg_decode: null argument");
    BVC_REQUIRE(n >= 1 && n <= 65535, "op_jpeg_decode: 1 .. 65535 images per call, not %d", n);
    BVC_REQUIRE(nseg >= 0 && nseg < (1ll << 30) && (nseg == 0 || (segs_host && segs_dev)), "op_jpeg_decode: bad segment table");
    BVC_REQUIRE(lanes >= 0 && lanes <= 64, "op_jpeg_decode: lanes is 0 (choose) or 1 .. 64, not %d", lanes);
    BVC_REQUIRE(stages >= 1 && stages <= 3, "op_jpeg_decode: stages is 3 (both kernels), or 1 / 2 for one of them alone, not %d", stages);
    int64_t plane_at = 0, seg_at = 0, out_at = 0;
    int max_runs = 0;
    for (int i = 0; i < n; ++i) {
        const bvc_jpeg_info& I = infos_host[i];
        BVC_REQUIRE(I.seg_first == seg_at, "op_jpeg_decode: image %d: seg_first %d is not the running count %lld", i, I.seg_first, (long long)seg_at);
        if (I.reason != 0) {
            BVC_REQUIRE(I.nseg == 0, "op_jpeg_decode: image %d is refused and has segments", i);
            continue;
        }
        BVC_REQUIRE(jpg::info_sane(I), "op_jpeg_decode: image %d: the info is not one that bvc_jpeg_parse accepted", i);
        BVC_REQUIRE(I.nseg <= nseg - seg_at, "op_jpeg_decode: image %d: more segments than the table holds", i);
        BVC_REQUIRE(I.blob_offset >= 0 && I.blob_offset <= blob_bytes, "op_jpeg_decode: image %d: blob_offset outside the blob", i);
        const int total = I.mcus_x * I.mcus_y;
        int next = 0;
        for (int s = 0; s < I.nseg; ++s) {
            const int32_t* g = segs_host + (size_t)jpg::kSegInts * (seg_at + s);
            BVC_REQUIRE(g[0] >= 0 && g[0] <= g[1] && g[1] <= blob_bytes - I.blob_offset && g[2] == next && g[3] >= 1 && g[3] <= total - next,
                        "op_jpeg_decode: image %d: segment %d is outside the blob or the image", i, s);
            next += g[3];
        }
        BVC_REQUIRE(next == total, "op_jpeg_decode: image %d: the segments do not cover the image", i);
        seg_at += I.nseg;
        const int64_t pb = jpg::align16(jpg::plane_bytes(&I));
        BVC_REQUIRE(I.plane_offset == plane_at, "op_jpeg_decode: image %d: plane_offset is not what bvc_op_jpeg_decode_workspace set", i);
        plane_at += pb;
        const int64_t ob = (int64_t)3 * I.width * I.height;
        BVC_REQUIRE(out_offsets_host[i] >= out_at && out_offsets_host[i] <= out_bytes - ob,
                    "op_jpeg_decode: image %d: its output overlaps the one before or ends outside out", i);
        out_at = out_offsets_host[i] + ob;
        const int runs = (I.height * ((I.width + jpg::kRun - 1) / jpg::kRun) + 255) / 256;
        max_runs = runs > max_runs ? runs : max_runs;
    }
    BVC_REQUIRE(seg_at == nseg, "op_jpeg_decode: the infos name %lld segments, the table holds %lld", (long long)seg_at, (long long)nseg);
    hipStream_t st = (hipStream_t)stream;
    if (nseg == 0) {      // every image refused
        BVC_CHECK_HIP(hipMemsetAsync(status_dev, 0, (size_t)n * 4, st));
        return BVC_OK;
    }
    BVC_REQUIRE(workspace_dev && ((uintptr_t)workspace_dev % 16) == 0 && workspace_bytes >= plane_at + 4 * nseg,
                "op_jpeg_decode: null workspace, one off 16-byte alignment, or fewer than %lld bytes", (long long)(plane_at + 4 * nseg));
    uint8_t* work = (uint8_t*)workspace_dev;
    int32_t* seg_status = (int32_t*)(work + plane_at);
    if (lanes == 0) {      // few segments: one per wave, on as many waves as there are; many: packed
        const int64_t want = (nseg + 2047) / 2048;
        lanes = want < 1 ? 1 : (want > 64 ? 64 : (int)want);
    }
    const unsigned blocks = (unsigned)((nseg + lanes - 1) / lanes);
    if (stages & 1)
        hipLaunchKernelGGL(jpg::jpeg_entropy_idct_kernel, dim3(blocks), dim3(64), (size_t)lanes * jpg::kBlockDwords * 4, st, blob_dev, infos_dev,
                           n, segs_dev, (int)nseg, lanes, work, seg_status);
    BVC_CHECK_HIP(hipGetLastError());
    if (stages & 2)
        hipLaunchKernelGGL(jpg::jpeg_colour_kernel, dim3((unsigned)(max_runs < 1 ? 1 : max_runs), (unsigned)n), dim3(256), 0, st, infos_dev,
                           work, seg_status, out_offsets_dev, out_dev, status_dev);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

}  // extern "C"

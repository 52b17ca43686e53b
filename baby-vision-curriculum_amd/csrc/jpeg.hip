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
// bvc_op_jpeg_decode_split adds, for segments of at least `split` bytes (include/bvc.h has the chunk layout; DESIGN.md the design):
// jpeg_split_route_kernel    the segment table the one-lane kernel gets in such a call: split segments have no MCUs in it
// jpeg_split_kernel          one workgroup per split segment, one lane per chunk of its bytes: speculative decode, hand-over rounds
//                            until no exit state changes (one __syncthreads_or per round; nothing waits on another workgroup),
//                            placement by a scan, dequantised AC coefficients and DC differences into the workspace, the DC scan
// jpeg_idct_kernel           one lane per block of those segments: coefficients -> samples in the planes; per image the counts
// jpeg_entropy_idct_flagged_kernel   decode_segment on the segments whose chain ended early (damaged): the fall-back
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

// ---------------------------------------------------------------- the split path (bvc_op_jpeg_decode_split)
// per segment: the record the one-lane kernel is given (split segments with no MCUs: their lanes leave at once), no flag, no rounds,
// and the clean status that a split segment keeps unless it falls back
__global__ __launch_bounds__(256) void jpeg_split_route_kernel(const int32_t* __restrict__ segs, int nseg, int split, int32_t* __restrict__ routed,
                                                               int32_t* __restrict__ flag, int32_t* __restrict__ rounds,
                                                               int32_t* __restrict__ seg_status) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= nseg) return;
    const int32_t* g = segs + (size_t)kSegInts * s;
    const bool sp = seg_is_split(g[1] - g[0], split);
    *reinterpret_cast<int4*>(routed + (size_t)kSegInts * s) = make_int4(g[0], g[1], g[2], sp ? 0 : g[3]);      // 16-byte aligned: SplitLayout
    flag[s] = 0;
    rounds[s] = 0;
    if (sp) seg_status[s] = 0;
}

// the image of segment s: the last one whose first segment is not after s
__device__ __forceinline__ int image_of_segment(const Info* __restrict__ infos, int n, int s) {
    int lo = 0, hi = n - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (infos[mid].seg_first <= s) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// exclusive scan of one int per lane over the workgroup, in place in buf[kSplitThreads]; returns the lane's prefix, *total the sum
__device__ __forceinline__ int32_t split_scan(int32_t v, int32_t* buf, int tid, int32_t* total) {
    buf[tid] = v;
    __syncthreads();
    for (int off = 1; off < kSplitThreads; off <<= 1) {
        const int32_t t = tid >= off ? buf[tid - off] : 0;
        __syncthreads();
        buf[tid] = (int32_t)((uint32_t)buf[tid] + (uint32_t)t);
        __syncthreads();
    }
    const int32_t incl = buf[tid];
    *total = buf[kSplitThreads - 1];
    __syncthreads();
    return (int32_t)((uint32_t)incl - (uint32_t)v);
}

// One workgroup per segment, one lane per chunk (jpeg.h, decode_chunk; the layout is in include/bvc.h).  Every barrier is reached by
// all kSplitThreads lanes: the loop bounds and the exit conditions are the same in every lane.
__global__ __launch_bounds__(kSplitThreads) void jpeg_split_kernel(const uint8_t* __restrict__ blob, const Info* __restrict__ infos, int n,
                                                                   const int32_t* __restrict__ segs, int split, int chunk,
                                                                   int16_t* __restrict__ coef_all, int32_t* __restrict__ dc_all,
                                                                   int32_t* __restrict__ flag, int32_t* __restrict__ rounds_out) {
    __shared__ uint32_t hand_pos[2][kSplitThreads], hand_meta[2][kSplitThreads];
    __shared__ int32_t scan[3][kSplitThreads];
    const int s = blockIdx.x, tid = threadIdx.x;
    const int32_t* sg = segs + (size_t)kSegInts * s;
    const int begin = sg[0], end = sg[1], bytes = end - begin;
    if (!seg_is_split(bytes, split)) return;      // the whole workgroup
    const Info* I = &infos[image_of_segment(infos, n, s)];
    const uint8_t* file = blob + I->blob_offset;
    const int hv = I->hs * I->vs, nblk = I->ncomp == 1 ? 1 : hv + 2, need = sg[3] * nblk;
    const int c = split_chunk_bytes(bytes, chunk), nch = (bytes + c - 1) / c;
    const bool live = tid < nch;
    const uint32_t stop = 8u * (uint32_t)min((int64_t)(tid + 1) * c, (int64_t)bytes);
    int16_t* coef = coef_all + I->plane_offset + (size_t)sg[2] * nblk * 64;      // 128 bytes per block, as 64 bytes of plane
    int32_t* dc = dc_all + I->plane_offset / 16 + (size_t)sg[2] * nblk;

    SplitState guess = {0u, 0u}, entry = {0u, 0u}, exit_ = {0u, 0u};
    int count = 0;
    if (live) {
        if (tid > 0) entry = guess = split_guess(file, begin, end, tid * c);
        exit_ = decode_chunk<false>(I, file, begin, end, stop, entry, nblk, hv, 0, 0, nullptr, nullptr, &count);
        hand_pos[0][tid] = exit_.pos;
        hand_meta[0][tid] = exit_.meta;
    }
    __syncthreads();
    int cur = 0, rounds = 0;
    for (int round = 1; round < nch; ++round) {
        int changed = 0;
        if (live) {
            if (tid > 0) {
                const SplitState e = split_entry(SplitState{hand_pos[cur][tid - 1], hand_meta[cur][tid - 1]}, guess);
                if (!split_same(e, entry)) {
                    entry = e;
                    const SplitState x = decode_chunk<false>(I, file, begin, end, stop, entry, nblk, hv, 0, 0, nullptr, nullptr, &count);
                    changed = !split_same(x, exit_);
                    exit_ = x;
                }
            }
            hand_pos[cur ^ 1][tid] = exit_.pos;
            hand_meta[cur ^ 1][tid] = exit_.meta;
        }
        const int any = __syncthreads_or(changed);
        cur ^= 1;
        ++rounds;
        if (!any) break;
    }
    // placement: the true chain ends at the first dead exit; what later lanes decoded from their guesses is dropped
    int32_t total;
    const int32_t dead_before = split_scan(live && (exit_.meta & kSplitDead) ? 1 : 0, scan[0], tid, &total);      // every lane scans
    const bool chain = live && dead_before == 0;
    const int32_t first = split_scan(chain ? count : 0, scan[0], tid, &total);
    if (total < need) {      // the true chain ended early: the one-lane decoder has the contract for that
        if (tid == 0) {
            flag[s] = 1;
            rounds_out[s] = rounds;
        }
        return;
    }
    uint4* z = reinterpret_cast<uint4*>(coef);
    for (int64_t i = tid; i < (int64_t)need * 8; i += kSplitThreads) z[i] = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
    if (chain) {
        int nb;
        decode_chunk<true>(I, file, begin, end, stop, entry, nblk, hv, first, need, coef, dc, &nb);
    }
    __syncthreads();
    // DC: differences -> predictions -> dequantised values, per component, each lane a run of consecutive blocks
    const int per = (need + kSplitThreads - 1) / kSplitThreads, lo = min(tid * per, need), hi = min(lo + per, need);
    uint32_t sum[3] = {0u, 0u, 0u};
    for (int b = lo; b < hi; ++b) {
        const int bi = b % nblk, comp = bi < hv ? 0 : bi - hv + 1;
        const uint32_t d = (uint32_t)dc[b];
        sum[0] += comp == 0 ? d : 0u;
        sum[1] += comp == 1 ? d : 0u;
        sum[2] += comp == 2 ? d : 0u;
    }
    int32_t unused;
    uint32_t pred0 = (uint32_t)split_scan((int32_t)sum[0], scan[0], tid, &unused);
    uint32_t pred1 = 0u, pred2 = 0u;
    if (nblk > 1) {
        pred1 = (uint32_t)split_scan((int32_t)sum[1], scan[1], tid, &unused);
        pred2 = (uint32_t)split_scan((int32_t)sum[2], scan[2], tid, &unused);
    }
    const uint32_t q0 = I->qt[I->tq[0] & 3][0], q1 = I->qt[I->tq[1] & 3][0], q2 = I->qt[I->tq[2] & 3][0];
    for (int b = lo; b < hi; ++b) {
        const int bi = b % nblk, comp = bi < hv ? 0 : bi - hv + 1;
        const uint32_t d = (uint32_t)dc[b];
        int32_t v;
        if (comp == 0) { pred0 += d; v = dequant((int32_t)pred0, q0); }
        else if (comp == 1) { pred1 += d; v = dequant((int32_t)pred1, q1); }
        else { pred2 += d; v = dequant((int32_t)pred2, q2); }
        dc[b] = v;
    }
    if (tid == 0) {
        flag[s] = 0;
        rounds_out[s] = rounds;
    }
}

// The one-lane decoder on the segments whose flag is set (the fall-back of the split path); every other lane leaves at once.
__global__ __launch_bounds__(64) void jpeg_entropy_idct_flagged_kernel(const uint8_t* __restrict__ blob, const Info* __restrict__ infos, int n,
                                                                       const int32_t* __restrict__ segs, int nseg, int lanes,
                                                                       const int32_t* __restrict__ flag, uint8_t* __restrict__ work,
                                                                       int32_t* __restrict__ seg_status) {
    extern __shared__ int32_t lds[];      // lanes x kBlockDwords
    const int lane = threadIdx.x;
    if (lane >= lanes) return;
    const int s = blockIdx.x * lanes + lane;
    if (s >= nseg || !flag[s]) return;
    const Info* I = &infos[image_of_segment(infos, n, s)];
    const int32_t* sg = segs + (size_t)kSegInts * s;
    seg_status[s] = decode_segment(I, blob + I->blob_offset, sg[0], sg[1], sg[2], sg[3], lds + lane * kBlockDwords, work + I->plane_offset);
}

// One lane per 8 x 8 block of image blockIdx.y: blocks of split segments that did not fall back go from coefficients to samples.  The
// first workgroup of every image counts its flagged segments and takes the largest round count (a tree in LDS) into info_out.
__global__ __launch_bounds__(64) void jpeg_idct_kernel(const Info* __restrict__ infos, const int32_t* __restrict__ segs, int split,
                                                       uint8_t* __restrict__ work, const int16_t* __restrict__ coef_all,
                                                       const int32_t* __restrict__ dc_all, const int32_t* __restrict__ flag,
                                                       const int32_t* __restrict__ rounds, int32_t* __restrict__ info_out) {
    __shared__ int32_t lds[64 * kBlockDwords];
    const Info* I = &infos[blockIdx.y];
    const int tid = threadIdx.x;
    const bool live = I->reason == 0;
    if (blockIdx.x == 0) {
        int32_t fb = 0, mr = 0;
        if (live)
            for (int s = tid; s < I->nseg; s += 64) {
                fb += flag[I->seg_first + s];
                mr = max(mr, rounds[I->seg_first + s]);
            }
        lds[tid] = fb;
        lds[64 + tid] = mr;
        __syncthreads();
        for (int w = 32; w > 0; w >>= 1) {
            if (tid < w) {
                lds[tid] += lds[tid + w];
                lds[64 + tid] = max(lds[64 + tid], lds[64 + tid + w]);
            }
            __syncthreads();
        }
        if (tid == 0) {
            info_out[2 * blockIdx.y] = lds[0];
            info_out[2 * blockIdx.y + 1] = lds[64];
        }
        __syncthreads();
    }
    if (!live) return;
    const int nblk = I->ncomp == 1 ? 1 : I->hs * I->vs + 2;
    const int b = blockIdx.x * 64 + tid;
    if (b >= I->mcus_x * I->mcus_y * nblk) return;
    const int mcu = b / nblk;
    int lo = 0, hi = I->nseg - 1;      // the image's last segment that does not begin after this MCU
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (segs[(size_t)kSegInts * (I->seg_first + mid) + 2] <= mcu) lo = mid; else hi = mid - 1;
    }
    const int s = I->seg_first + lo;
    const int32_t* sg = segs + (size_t)kSegInts * s;
    if (!seg_is_split(sg[1] - sg[0], split) || flag[s]) return;
    const uint4* coef = reinterpret_cast<const uint4*>(coef_all + I->plane_offset + (size_t)b * 64);      // 128 bytes, 32-byte aligned
    int32_t* blk = lds + tid * kBlockDwords;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint4 v = coef[i];
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            blk[8 * i + 2 * e] = (int32_t)(int16_t)(w[e] & 0xffffu);
            blk[8 * i + 2 * e + 1] = (int32_t)(int16_t)(w[e] >> 16);
        }
    }
    blk[0] = dc_all[I->plane_offset / 16 + b];
    idct_block(I, b, blk, work + I->plane_offset);
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

int bvc_jpeg_split_chunk(int bytes, int chunk) {
    BVC_REQUIRE(bytes >= 0 && (chunk == 0 || chunk >= jpg::kSplitMinChunk), "jpeg_split_chunk: chunk is 0 or >= %d, not %d", jpg::kSplitMinChunk, chunk);
    return jpg::split_chunk_bytes(bytes, chunk);
}

int bvc_jpeg_decode_host_split(const uint8_t* data, int64_t n, const bvc_jpeg_info* info, const int32_t* seg, int split, int chunk,
                               uint8_t* out_rgb, int32_t* info_out) {
    BVC_REQUIRE(data && info && seg && out_rgb && info_out, "jpeg_decode_host_split: null argument");
    BVC_REQUIRE(info->reason == 0 && jpg::info_sane(*info), "jpeg_decode_host_split: the info is not one that bvc_jpeg_parse accepted");
    BVC_REQUIRE(split >= 0 && (chunk == 0 || chunk >= jpg::kSplitMinChunk), "jpeg_decode_host_split: split >= 0 and chunk 0 or >= %d",
                jpg::kSplitMinChunk);
    const int total = info->mcus_x * info->mcus_y;
    int next = 0;
    for (int s = 0; s < info->nseg; ++s) {
        const int32_t* g = seg + (size_t)jpg::kSegInts * s;
        BVC_REQUIRE(g[0] >= 0 && g[0] <= g[1] && g[1] <= n && g[2] == next && g[3] >= 1 && g[3] <= total - next,
                    "jpeg_decode_host_split: segment %d is outside the file or the image", s);
        next += g[3];
    }
    BVC_REQUIRE(next == total, "jpeg_decode_host_split: the segments do not cover the image");
    return jpg::decode_host_split(data, info, seg, split, chunk, out_rgb, info_out);
}

namespace {
// the split path's part of the workspace, behind the planes and the status words of bvc_op_jpeg_decode
struct SplitLayout {
    int64_t flag, rounds, routed, dc, coef, total;
    SplitLayout(int64_t planes, int64_t nseg) {
        flag = jpg::align16(planes + 4 * nseg);
        rounds = jpg::align16(flag + 4 * nseg);
        routed = jpg::align16(rounds + 4 * nseg);
        dc = jpg::align16(routed + 4 * jpg::kSegInts * nseg);
        coef = jpg::align16(dc + planes / 4 + 4);      // one int32 per block, indexed from plane_offset / 16
        total = coef + 2 * planes;                     // 64 int16 per block
    }
};
}  // namespace

int64_t bvc_op_jpeg_decode_split_workspace(bvc_jpeg_info* infos_host, int n) {
    const int64_t plain = bvc_op_jpeg_decode_workspace(infos_host, n);
    if (!infos_host || n < 1) return 0;
    int64_t nseg = 0;
    for (int i = 0; i < n; ++i)
        if (infos_host[i].reason == 0 && jpg::info_sane(infos_host[i])) nseg += infos_host[i].nseg;
    return SplitLayout(plain - 4 * nseg, nseg).total;
}

int bvc_op_jpeg_decode_split(const uint8_t* blob_dev, int64_t blob_bytes, const bvc_jpeg_info* infos_host, const bvc_jpeg_info* infos_dev,
                             int n, const int32_t* segs_host, const int32_t* segs_dev, int64_t nseg, const int64_t* out_offsets_host,
                             const int64_t* out_offsets_dev, uint8_t* out_dev, int64_t out_bytes, int32_t* status_dev, void* workspace_dev,
                             int64_t workspace_bytes, int lanes, int stages, int split, int chunk, int32_t* info_out_dev, void* stream) {
    BVC_REQUIRE(blob_dev && infos_host && infos_dev && out_offsets_host && out_offsets_dev && out_dev && status_dev && info_out_dev,
                "op_jpeg_decode_split: null argument");
    BVC_REQUIRE(n >= 1 && n <= 65535, "op_jpeg_decode_split: 1 .. 65535 images per call, not %d", n);
    BVC_REQUIRE(nseg >= 0 && nseg < (1ll << 30) && (nseg == 0 || (segs_host && segs_dev)), "op_jpeg_decode_split: bad segment table");
    BVC_REQUIRE(lanes >= 0 && lanes <= 64, "op_jpeg_decode_split: lanes is 0 (choose) or 1 .. 64, not %d", lanes);
    BVC_REQUIRE(stages >= 1 && stages <= 3, "op_jpeg_decode_split: stages is 3, or 1 / 2 for one side alone, not %d", stages);
    BVC_REQUIRE(split >= 0, "op_jpeg_decode_split: split is 0 (no segment) or a number of bytes, not %d", split);
    BVC_REQUIRE(chunk == 0 || chunk >= jpg::kSplitMinChunk, "op_jpeg_decode_split: chunk is 0 (choose) or >= %d bytes, not %d",
                jpg::kSplitMinChunk, chunk);
    int64_t plane_at = 0, seg_at = 0, out_at = 0, nsplit = 0;
    int max_runs = 0, max_blocks = 0;
    for (int i = 0; i < n; ++i) {
        const bvc_jpeg_info& I = infos_host[i];
        BVC_REQUIRE(I.seg_first == seg_at, "op_jpeg_decode_split: image %d: seg_first %d is not the running count %lld", i, I.seg_first,
                    (long long)seg_at);
        if (I.reason != 0) {
            BVC_REQUIRE(I.nseg == 0, "op_jpeg_decode_split: image %d is refused and has segments", i);
            continue;
        }
        BVC_REQUIRE(jpg::info_sane(I), "op_jpeg_decode_split: image %d: the info is not one that bvc_jpeg_parse accepted", i);
        BVC_REQUIRE(I.nseg <= nseg - seg_at, "op_jpeg_decode_split: image %d: more segments than the table holds", i);
        BVC_REQUIRE(I.blob_offset >= 0 && I.blob_offset <= blob_bytes, "op_jpeg_decode_split: image %d: blob_offset outside the blob", i);
        const int total = I.mcus_x * I.mcus_y;
        int next = 0;
        bool any = false;
        for (int s = 0; s < I.nseg; ++s) {
            const int32_t* g = segs_host + (size_t)jpg::kSegInts * (seg_at + s);
            BVC_REQUIRE(g[0] >= 0 && g[0] <= g[1] && g[1] <= blob_bytes - I.blob_offset && g[2] == next && g[3] >= 1 && g[3] <= total - next,
                        "op_jpeg_decode_split: image %d: segment %d is outside the blob or the image", i, s);
            next += g[3];
            any = any || jpg::seg_is_split(g[1] - g[0], split);
            nsplit += jpg::seg_is_split(g[1] - g[0], split);
        }
        BVC_REQUIRE(next == total, "op_jpeg_decode_split: image %d: the segments do not cover the image", i);
        seg_at += I.nseg;
        const int64_t pb = jpg::align16(jpg::plane_bytes(&I));
        BVC_REQUIRE(I.plane_offset == plane_at, "op_jpeg_decode_split: image %d: plane_offset is not what the workspace call set", i);
        plane_at += pb;
        const int64_t ob = (int64_t)3 * I.width * I.height;
        BVC_REQUIRE(out_offsets_host[i] >= out_at && out_offsets_host[i] <= out_bytes - ob,
                    "op_jpeg_decode_split: image %d: its output overlaps the one before or ends outside out", i);
        out_at = out_offsets_host[i] + ob;
        const int runs = (I.height * ((I.width + jpg::kRun - 1) / jpg::kRun) + 255) / 256;
        max_runs = runs > max_runs ? runs : max_runs;
        const int blocks = total * (I.ncomp == 1 ? 1 : I.hs * I.vs + 2);
        if (any) max_blocks = blocks > max_blocks ? blocks : max_blocks;
    }
    BVC_REQUIRE(seg_at == nseg, "op_jpeg_decode_split: the infos name %lld segments, the table holds %lld", (long long)seg_at, (long long)nseg);
    hipStream_t st = (hipStream_t)stream;
    if (stages & 1) BVC_CHECK_HIP(hipMemsetAsync(info_out_dev, 0, (size_t)n * 8, st));
    if (nseg == 0) {      // every image refused
        BVC_CHECK_HIP(hipMemsetAsync(status_dev, 0, (size_t)n * 4, st));
        return BVC_OK;
    }
    const SplitLayout L(plane_at, nseg);
    const int64_t want_bytes = nsplit ? L.total : plane_at + 4 * nseg;
    BVC_REQUIRE(workspace_dev && ((uintptr_t)workspace_dev % 16) == 0 && workspace_bytes >= want_bytes,
                "op_jpeg_decode_split: null workspace, one off 16-byte alignment, or fewer than %lld bytes", (long long)want_bytes);
    uint8_t* work = (uint8_t*)workspace_dev;
    int32_t* seg_status = (int32_t*)(work + plane_at);
    if (lanes == 0) {
        const int64_t want = (nseg + 2047) / 2048;
        lanes = want < 1 ? 1 : (want > 64 ? 64 : (int)want);
    }
    const unsigned blocks = (unsigned)((nseg + lanes - 1) / lanes);
    const size_t lds = (size_t)lanes * jpg::kBlockDwords * 4;
    if ((stages & 1) && nsplit == 0)      // nothing to split: the launches of bvc_op_jpeg_decode
        hipLaunchKernelGGL(jpg::jpeg_entropy_idct_kernel, dim3(blocks), dim3(64), lds, st, blob_dev, infos_dev, n, segs_dev, (int)nseg, lanes,
                           work, seg_status);
    if ((stages & 1) && nsplit > 0) {
        int32_t* flag = (int32_t*)(work + L.flag);
        int32_t* rounds = (int32_t*)(work + L.rounds);
        int32_t* routed = (int32_t*)(work + L.routed);
        int32_t* dc = (int32_t*)(work + L.dc);
        int16_t* coef = (int16_t*)(work + L.coef);
        hipLaunchKernelGGL(jpg::jpeg_split_route_kernel, dim3((unsigned)((nseg + 255) / 256)), dim3(256), 0, st, segs_dev, (int)nseg, split,
                           routed, flag, rounds, seg_status);
        if (nsplit < nseg)      // the segments below `split`: the one-lane kernel as it is; split ones have no MCUs in `routed`
            hipLaunchKernelGGL(jpg::jpeg_entropy_idct_kernel, dim3(blocks), dim3(64), lds, st, blob_dev, infos_dev, n, routed, (int)nseg, lanes,
                               work, seg_status);
        hipLaunchKernelGGL(jpg::jpeg_split_kernel, dim3((unsigned)nseg), dim3(jpg::kSplitThreads), 0, st, blob_dev, infos_dev, n, segs_dev,
                           split, chunk, coef, dc, flag, rounds);
        hipLaunchKernelGGL(jpg::jpeg_idct_kernel, dim3((unsigned)((max_blocks + 63) / 64), (unsigned)n), dim3(64), 0, st, infos_dev, segs_dev,
                           split, work, coef, dc, flag, rounds, info_out_dev);
        hipLaunchKernelGGL(jpg::jpeg_entropy_idct_flagged_kernel, dim3(blocks), dim3(64), lds, st, blob_dev, infos_dev, n, segs_dev, (int)nseg,
                           lanes, flag, work, seg_status);
    }
    BVC_CHECK_HIP(hipGetLastError());
    if (stages & 2)
        hipLaunchKernelGGL(jpg::jpeg_colour_kernel, dim3((unsigned)(max_runs < 1 ? 1 : max_runs), (unsigned)n), dim3(256), 0, st, infos_dev,
                           work, seg_status, out_offsets_dev, out_dev, status_dev);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

}  // extern "C"

// Baseline JPEG decode to planar RGB uint8 (include/bvc.h, bvc_jpeg_info): the arithmetic that the kernels of jpeg.hip and the host twin
// share, and the parser.  The bar is the bytes of libjpeg-turbo at its defaults, restated:
//
//   entropy   Huffman, libjpeg's HUFF_LOOKAHEAD scheme: the next 8 bits index look[]; a longer code is found by maxcode[l] and read from
//             huffval[code + valoff[l]].  A 64-bit buffer, refilled from the segment's own bytes, FF 00 -> FF in the refill; FF followed
//             by anything else ends the data.  Past the end the buffer feeds zero bits, and a symbol that needed one of them is dropped
//             and ends the segment (TRUNCATED), as do a code that matches nothing (BAD_CODE) and a run past coefficient 63 (BAD_RUN):
//             the block keeps what it has and every later block of the segment is DC-only at its component's last DC prediction.
//   dequant   coefficient * table entry, kept to 16 bits as the 16-bit multiply of libjpeg-turbo's vector IDCT keeps it
//   IDCT      jidctint ("ISLOW"): CONST_BITS 13, PASS1_BITS 2, columns first (descale 11), rows second (descale 18), the result masked
//             to 10 bits and range-limited: v < 128: v + 128; v < 512: 255; v < 896: 0; else v - 896.  32-bit wrapping arithmetic.
//   upsample  "fancy": 2x1 (3 cur + neighbour + 1 | 2) >> 2; 2x2 the triangle filter on 3 near + far column sums, + 8 | 7, >> 4; the
//             first and last samples are those of the component's real down-sampled width and height.  A component at most two
//             samples wide is replicated instead (libjpeg-turbo chooses the box filter there).
//   colour    R = Y + ((91881 cr + 32768) >> 16), B = Y + ((116130 cb + 32768) >> 16), G = Y + ((-22554 cb - 46802 cr + 32768) >> 16),
//             cb / cr centred at 128, arithmetic shifts, clamped.  One component is shown as three equal channels.
//
// parse() and decode_host() are host code; everything marked JPG_HD compiles for both sides.  This header compiles without HIP.
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/bvc.h"

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define JPG_HD __host__ __device__ __forceinline__
#else
#define JPG_HD inline
#endif

#include <vector>

namespace bvc {
namespace jpg {

typedef bvc_jpeg_info Info;
typedef bvc_jpeg_huff Huff;
static_assert(sizeof(Huff) == 912, "bvc_jpeg_huff layout");
static_assert(sizeof(Info) == 4248, "bvc_jpeg_info layout");

constexpr int kSegInts = 4;      // a segment record: first byte, end byte, first MCU, MCU count
constexpr int kBlockDwords = 65; // a lane's block in LDS: 64 coefficients and one dword, so that the stride is odd in dwords

// zig-zag position -> natural (row-major) position
JPG_HD int natural_of(int k) {
    constexpr uint8_t t[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                               41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                               30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};
    return t[k & 63];
}

// ---------------------------------------------------------------- the bit reader
struct Bits {
    const uint8_t* p;      // the file
    int pos, end;          // next byte, and the end of the segment: no address outside [pos, end) is formed
    uint64_t buf;          // the next bits, from bit 63 down; zero below the valid ones
    int cnt;               // valid bits in buf, >= 0
};

JPG_HD void refill(Bits& b) {
    while (b.cnt <= 56 && b.pos < b.end) {
        if (b.cnt <= 32 && b.pos + 4 <= b.end) {      // four bytes at once when none of them is FF
            const uint32_t b0 = b.p[b.pos], b1 = b.p[b.pos + 1], b2 = b.p[b.pos + 2], b3 = b.p[b.pos + 3];
            if (b0 != 255u && b1 != 255u && b2 != 255u && b3 != 255u) {
                b.buf |= (uint64_t)((b0 << 24) | (b1 << 16) | (b2 << 8) | b3) << (32 - b.cnt);
                b.cnt += 32;
                b.pos += 4;
                continue;
            }
        }
        const uint32_t c = b.p[b.pos];
        if (c == 255u) {
            if (b.pos + 1 < b.end && b.p[b.pos + 1] == 0) {
                b.pos += 2;
            } else {      // a marker or a fill byte inside the segment, or a lone FF at its end: the data stop here
                b.pos = b.end;
                break;
            }
        } else {
            b.pos += 1;
        }
        b.buf |= (uint64_t)c << (56 - b.cnt);
        b.cnt += 8;
    }
}

// drop n <= 16 bits; true when one of them was not there
JPG_HD bool consume(Bits& b, int n) {
    b.buf <<= n;
    b.cnt -= n;
    if (b.cnt < 0) {
        b.cnt = 0;
        return true;
    }
    return false;
}

// One Huffman symbol from the next 16 bits (zero-padded): its length in *len, or -1 when no code matches.  Every index is in range
// whatever the table holds.
JPG_HD int huff_symbol(const Huff* h, uint32_t peek16, int* len) {
    const uint32_t lk = h->look[(peek16 >> 8) & 255u];
    if (lk) {
        *len = (int)(lk >> 8) & 15;
        return (int)(lk & 255u);
    }
    int l = 9;
    int code = (int)(peek16 >> 7);
    while (l <= 16 && code > h->maxcode[l]) {
        ++l;
        code = (int)(peek16 >> ((16 - l) & 15));
    }
    if (l > 16) {
        *len = 0;
        return -1;
    }
    *len = l;
    return h->huffval[(code + h->valoff[l]) & 255];
}

JPG_HD int extend(uint32_t bits, int s) { return bits < (1u << (s - 1)) ? (int)bits - (1 << s) + 1 : (int)bits; }
JPG_HD int32_t dequant(int32_t v, uint32_t q) { return (int32_t)(int16_t)(uint16_t)((uint32_t)v * q); }

// ---------------------------------------------------------------- IDCT
JPG_HD int32_t mulc(int32_t a, int32_t c) { return (int32_t)((uint32_t)a * (uint32_t)c); }
JPG_HD int32_t add(int32_t a, int32_t b) { return (int32_t)((uint32_t)a + (uint32_t)b); }
JPG_HD int32_t sub(int32_t a, int32_t b) { return (int32_t)((uint32_t)a - (uint32_t)b); }
JPG_HD int32_t shl(int32_t a, int n) { return (int32_t)((uint32_t)a << n); }
JPG_HD int32_t descale(int32_t x, int n) { return add(x, 1 << (n - 1)) >> n; }

JPG_HD int range_limit(int32_t x) {
    const int v = (int)(x & 1023);
    return v < 128 ? v + 128 : (v < 512 ? 255 : (v < 896 ? 0 : v - 896));
}

// one 8-point pass of jidctint on in[0 .. 7]; out[i] before the descale
JPG_HD void idct8(const int32_t in[8], int32_t out[8]) {
    int32_t z2 = in[2], z3 = in[6];
    int32_t z1 = mulc(add(z2, z3), 4433);
    int32_t tmp2 = add(z1, mulc(z3, -15137));
    int32_t tmp3 = add(z1, mulc(z2, 6270));
    z2 = in[0];
    z3 = in[4];
    int32_t tmp0 = shl(add(z2, z3), 13);
    int32_t tmp1 = shl(sub(z2, z3), 13);
    const int32_t tmp10 = add(tmp0, tmp3), tmp13 = sub(tmp0, tmp3), tmp11 = add(tmp1, tmp2), tmp12 = sub(tmp1, tmp2);
    tmp0 = in[7];
    tmp1 = in[5];
    tmp2 = in[3];
    tmp3 = in[1];
    z1 = add(tmp0, tmp3);
    z2 = add(tmp1, tmp2);
    z3 = add(tmp0, tmp2);
    int32_t z4 = add(tmp1, tmp3);
    const int32_t z5 = mulc(add(z3, z4), 9633);
    tmp0 = mulc(tmp0, 2446);
    tmp1 = mulc(tmp1, 16819);
    tmp2 = mulc(tmp2, 25172);
    tmp3 = mulc(tmp3, 12299);
    z1 = mulc(z1, -7373);
    z2 = mulc(z2, -20995);
    z3 = add(mulc(z3, -16069), z5);
    z4 = add(mulc(z4, -3196), z5);
    tmp0 = add(tmp0, add(z1, z3));
    tmp1 = add(tmp1, add(z2, z4));
    tmp2 = add(tmp2, add(z2, z3));
    tmp3 = add(tmp3, add(z1, z4));
    out[0] = add(tmp10, tmp3);
    out[7] = sub(tmp10, tmp3);
    out[1] = add(tmp11, tmp2);
    out[6] = sub(tmp11, tmp2);
    out[2] = add(tmp12, tmp1);
    out[5] = sub(tmp12, tmp1);
    out[3] = add(tmp13, tmp0);
    out[4] = sub(tmp13, tmp0);
}

JPG_HD void store8(uint8_t* dst, uint32_t lo, uint32_t hi) {      // dst is 8-byte aligned
#if defined(__HIP_DEVICE_COMPILE__)
    *reinterpret_cast<uint2*>(dst) = make_uint2(lo, hi);
#else
    const uint32_t w[2] = {lo, hi};
    uint8_t bytes[8];
    for (int i = 0; i < 8; ++i) bytes[i] = (uint8_t)(w[i >> 2] >> (8 * (i & 3)));
    memcpy(dst, bytes, 8);
#endif
}

// the dequantised block blk[64] (natural order), in place, to eight 8-byte rows at dst
JPG_HD void idct_store(int32_t* blk, uint8_t* dst, int stride) {
    int32_t in[8], out[8];
    for (int c = 0; c < 8; ++c) {
#pragma unroll
        for (int r = 0; r < 8; ++r) in[r] = blk[8 * r + c];
        idct8(in, out);
#pragma unroll
        for (int r = 0; r < 8; ++r) blk[8 * r + c] = descale(out[r], 11);
    }
    for (int r = 0; r < 8; ++r) {
#pragma unroll
        for (int c = 0; c < 8; ++c) in[c] = blk[8 * r + c];
        idct8(in, out);
        uint32_t w[2] = {0u, 0u};
#pragma unroll
        for (int c = 0; c < 8; ++c) w[c >> 2] |= (uint32_t)range_limit(descale(out[c], 18)) << (8 * (c & 3));
        store8(dst + (size_t)r * stride, w[0], w[1]);
    }
}

// ---------------------------------------------------------------- planes
JPG_HD int luma_stride(const Info* I) { return I->mcus_x * 8 * I->hs; }
JPG_HD int chroma_stride(const Info* I) { return I->mcus_x * 8; }
JPG_HD int64_t luma_bytes(const Info* I) { return (int64_t)luma_stride(I) * (I->mcus_y * 8 * I->vs); }
JPG_HD int64_t chroma_bytes(const Info* I) { return (int64_t)chroma_stride(I) * (I->mcus_y * 8); }
JPG_HD int64_t plane_bytes(const Info* I) { return luma_bytes(I) + (I->ncomp == 3 ? 2 * chroma_bytes(I) : 0); }

// ---------------------------------------------------------------- stage 1: one segment
// Entropy-decodes MCUs [first_mcu, first_mcu + mcu_count) from file[begin, end), one symbol per iteration of the loop, and writes
// every block of theirs into the planes.  blk: 64 dwords of the caller's.  Returns the status bits.
JPG_HD int decode_segment(const Info* I, const uint8_t* file, int begin, int end, int first_mcu, int mcu_count, int32_t* blk,
                          uint8_t* planes) {
    const int hs = I->hs, hv = I->hs * I->vs, ncomp = I->ncomp, mcus_x = I->mcus_x;
    const int nblk = ncomp == 1 ? 1 : hv + 2;
    const int mcu_end = first_mcu + mcu_count;
    Bits b = {file, begin, end, 0ull, 0};
    int st = 0;
    int32_t pred0 = 0, pred1 = 0, pred2 = 0;
    int mcu = first_mcu, bi = 0, k = 0, comp = 0;
    bool dead = false;
    const Huff* dc = &I->huff[I->td[0] & 1];
    const Huff* ac = &I->huff[2 + (I->ta[0] & 1)];
    const uint16_t* q = I->qt[I->tq[0] & 3];
    for (int i = 0; i < 64; ++i) blk[i] = 0;
    while (mcu < mcu_end) {
        bool done = false;
        const int32_t pred = comp == 0 ? pred0 : (comp == 1 ? pred1 : pred2);
        if (dead) {
            blk[0] = dequant(pred, q[0]);
            done = true;
        } else {
            if (b.cnt < 32) refill(b);      // a symbol takes at most 16 + 15 bits
            int len;
            const int sym = huff_symbol(k == 0 ? dc : ac, (uint32_t)(b.buf >> 48), &len);
            int err = sym < 0 ? BVC_JPEG_ST_BAD_CODE : 0;
            bool over = consume(b, len);
            const int s = sym & 15, r = (sym >> 4) & 15;
            uint32_t bits = 0u;
            if (!err && s) {
                bits = (uint32_t)(b.buf >> (64 - s));
                over = consume(b, s) || over;
            }
            if (!err && over) err = BVC_JPEG_ST_TRUNCATED;
            if (k == 0) {
                int32_t p = pred;
                if (!err) p = add(pred, s ? extend(bits, s) : 0);
                if (comp == 0) pred0 = p; else if (comp == 1) pred1 = p; else pred2 = p;
                blk[0] = dequant(p, q[0]);
                k = 1;
            } else if (!err) {
                if (s) {
                    k += r;
                    if (k > 63) {
                        err = BVC_JPEG_ST_BAD_RUN;
                    } else {
                        const int nat = natural_of(k);
                        blk[nat] = dequant(extend(bits, s), q[nat]);
                        k += 1;
                    }
                } else if (r == 15) {
                    k += 16;
                    if (k > 63) err = BVC_JPEG_ST_BAD_RUN;
                } else {
                    k = 64;      // end of block
                }
            }
            if (err) {
                st |= err;
                dead = true;
            }
            done = dead || k > 63;
        }
        if (done) {
            const int mx = mcu % mcus_x, my = mcu / mcus_x;
            uint8_t* dst;
            int stride;
            if (comp == 0) {
                stride = ncomp == 1 ? mcus_x * 8 : luma_stride(I);
                const int bx = ncomp == 1 ? mx : mx * hs + bi % hs, by = ncomp == 1 ? my : my * I->vs + bi / hs;
                dst = planes + ((size_t)by * 8) * stride + (size_t)bx * 8;
            } else {
                stride = chroma_stride(I);
                dst = planes + luma_bytes(I) + (comp == 2 ? chroma_bytes(I) : 0) + ((size_t)my * 8) * stride + (size_t)mx * 8;
            }
            idct_store(blk, dst, stride);
            for (int i = 0; i < 64; ++i) blk[i] = 0;
            k = 0;
            bi += 1;
            if (bi == nblk) {
                bi = 0;
                mcu += 1;
            }
            const int c = bi < hv ? 0 : bi - hv + 1;
            if (c != comp) {
                comp = c;
                dc = &I->huff[I->td[c] & 1];
                ac = &I->huff[2 + (I->ta[c] & 1)];
                q = I->qt[I->tq[c] & 3];
            }
        }
    }
    return st;
}

// ---------------------------------------------------------------- stage 1, split: one segment on the lanes of a workgroup
// include/bvc.h, bvc_op_jpeg_decode_split.  The segment's bytes are cut into chunks, one lane per chunk; a lane decodes the symbols
// that START inside its chunk.  States that lanes hand to each other live in ONE coordinate system: bit positions in the raw file,
// relative to the segment's first byte, where a stuffed 00 belongs to its FF - a position is never inside a stuffed byte, and the
// position after the last bit of an FF is the first bit after its 00.
constexpr int kSplitThreads = BVC_JPEG_SPLIT_THREADS;      // lanes of a workgroup = the most chunks a segment is cut into
constexpr int kSplitMinChunk = BVC_JPEG_SPLIT_MIN_CHUNK;   // a symbol is at most 31 bits: an entry point lies inside its own chunk
constexpr int kSplitDefaultChunk = BVC_JPEG_SPLIT_DEFAULT_CHUNK;
constexpr int kSplitMaxBytes = 1 << 28;                    // bit positions are 32-bit

struct SplitState {
    uint32_t pos;       // the next symbol's first bit
    uint32_t meta;      // block within the MCU | zig-zag index k << 3 | kSplitDead
};
constexpr uint32_t kSplitDead = 1u << 9;      // an error, or the end of the data inside a symbol, lies before this point

JPG_HD bool split_same(SplitState a, SplitState b) { return a.pos == b.pos && a.meta == b.meta; }
JPG_HD SplitState split_dead() { return SplitState{0u, kSplitDead}; }

JPG_HD bool seg_is_split(int bytes, int split) { return split > 0 && bytes >= split && bytes >= 2 * kSplitMinChunk && bytes < kSplitMaxBytes; }
// bytes per lane: max(chunk, bytes / kSplitThreads rounded up to a multiple of 4)
JPG_HD int split_chunk_bytes(int bytes, int chunk) {
    const int c = chunk > 0 ? chunk : kSplitDefaultChunk, per = ((bytes + kSplitThreads - 1) / kSplitThreads + 3) & ~3;
    return c > per ? c : per;
}

// the reader of the split path: Bits, and where it is in the raw file
struct SBits {
    Bits b;
    uint64_t ff;      // aligned with b.buf: the last bit of every buffered FF whose stuffed 00 follows it in the file
    bool hard;        // the data ended at a marker or a lone FF: b.pos says nothing any more
};

JPG_HD void refill(SBits& s) {
    Bits& b = s.b;
    while (b.cnt <= 56 && b.pos < b.end) {
        if (b.cnt <= 32 && b.pos + 4 <= b.end) {
            const uint32_t b0 = b.p[b.pos], b1 = b.p[b.pos + 1], b2 = b.p[b.pos + 2], b3 = b.p[b.pos + 3];
            if (b0 != 255u && b1 != 255u && b2 != 255u && b3 != 255u) {
                b.buf |= (uint64_t)((b0 << 24) | (b1 << 16) | (b2 << 8) | b3) << (32 - b.cnt);
                b.cnt += 32;
                b.pos += 4;
                continue;
            }
        }
        const uint32_t c = b.p[b.pos];
        if (c == 255u) {
            if (b.pos + 1 < b.end && b.p[b.pos + 1] == 0) {
                b.pos += 2;
                s.ff |= 1ull << (56 - b.cnt);
            } else {
                b.pos = b.end;
                s.hard = true;
                break;
            }
        } else {
            b.pos += 1;
        }
        b.buf |= (uint64_t)c << (56 - b.cnt);
        b.cnt += 8;
    }
}

JPG_HD bool consume(SBits& s, int n) {
    s.ff <<= n;
    return consume(s.b, n);
}

JPG_HD int popcount64(uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __popcll(v);
#else
    return __builtin_popcountll(v);
#endif
}

// the next bit's position; an FF that is not consumed whole still has its 00 ahead
JPG_HD uint32_t position(const SBits& s, int begin) { return (uint32_t)(8 * (s.b.pos - begin) - s.b.cnt - 8 * popcount64(s.ff)); }

// where a lane that knows nothing enters chunk bytes [at, ...) of the segment: at the chunk's first byte that is not a stuffed 00,
// at the start of an MCU
JPG_HD SplitState split_guess(const uint8_t* file, int begin, int end, int at) {
    const int p = begin + at;
    const bool stuffed = at > 0 && p < end && file[p] == 0 && file[p - 1] == 255u;
    return SplitState{(uint32_t)(8 * (at + (stuffed ? 1 : 0))), 0u};
}

// what a lane enters its chunk with: the state its predecessor handed over, or its own guess when that is dead - a dead hand-over
// must not undo a lane that found the true chain by itself; placement ends the true chain at the first dead exit
JPG_HD SplitState split_entry(SplitState handed, SplitState guess) { return (handed.meta & kSplitDead) ? guess : handed; }

// One chunk: from state `in`, every symbol that starts before bit `stop`.  Returns the state at the first symbol at or after `stop`,
// or split_dead() when a bad code, a bad run or the end of the data came first (no status is raised here: the caller decides what a
// dead chain means), and in *blocks the blocks that were completed.  After the data's end at a marker positions mean nothing, so the
// lane goes on to the last buffered bit and leaves dead.  kWrite: block first_block + i of the segment, if it is below `need`, gets
// its AC coefficients dequantised into coef (64 int16 in natural order per block) and its DC DIFFERENCE into dc.
// nblk, hv: blocks per MCU, luma blocks per MCU.  No byte outside [begin, end) is read and every table index is masked.
template <bool kWrite>
JPG_HD SplitState decode_chunk(const Info* I, const uint8_t* file, int begin, int end, uint32_t stop, SplitState in, int nblk, int hv,
                               int first_block, int need, int16_t* coef, int32_t* dc, int* blocks) {
    *blocks = 0;
    if (in.meta & kSplitDead) return split_dead();
    if (in.pos >= stop) return in;
    int bi = (int)(in.meta & 7u), k = (int)((in.meta >> 3) & 63u), nb = 0;
    if (bi >= nblk) return split_dead();
    int at = begin + (int)(in.pos >> 3);
    if (at > end) at = end;
    SBits s = {{file, at, end, 0ull, 0}, 0ull, false};
    refill(s);
    consume(s, (int)(in.pos & 7u));
    int comp = bi < hv ? 0 : bi - hv + 1;
    const Huff* hdc = &I->huff[I->td[comp] & 1];
    const Huff* hac = &I->huff[2 + (I->ta[comp] & 1)];
    const uint16_t* q = I->qt[I->tq[comp] & 3];
    for (;;) {
        const uint32_t pos = position(s, begin);
        if (!s.hard && pos >= stop) {
            *blocks = nb;
            return SplitState{pos, (uint32_t)bi | ((uint32_t)k << 3)};
        }
        if (s.b.cnt < 32) refill(s);
        int len;
        const int sym = huff_symbol(k == 0 ? hdc : hac, (uint32_t)(s.b.buf >> 48), &len);
        bool err = sym < 0 || len < 1;      // a table of the caller's with a code of no bits: every pass of this loop takes at least one
        bool over = consume(s, len);
        const int sz = sym & 15, r = (sym >> 4) & 15;
        uint32_t bits = 0u;
        if (!err && sz) {
            bits = (uint32_t)(s.b.buf >> (64 - sz));
            over = consume(s, sz) || over;
        }
        err = err || over;
        const int blk = first_block + nb;
        if (!err) {
            if (k == 0) {
                if (kWrite && blk < need) dc[blk] = sz ? extend(bits, sz) : 0;
                k = 1;
            } else if (sz) {
                k += r;
                if (k > 63) {
                    err = true;
                } else {
                    const int nat = natural_of(k);
                    if (kWrite && blk < need) coef[(size_t)blk * 64 + nat] = (int16_t)dequant(extend(bits, sz), q[nat]);
                    k += 1;
                }
            } else if (r == 15) {
                k += 16;
                err = k > 63;
            } else {
                k = 64;      // end of block
            }
        }
        if (err) {
            *blocks = nb;
            return split_dead();
        }
        if (k > 63) {
            k = 0;
            nb += 1;
            bi = bi + 1 == nblk ? 0 : bi + 1;
            const int c = bi < hv ? 0 : bi - hv + 1;
            if (c != comp) {
                comp = c;
                hdc = &I->huff[I->td[c] & 1];
                hac = &I->huff[2 + (I->ta[c] & 1)];
                q = I->qt[I->tq[c] & 3];
            }
        }
    }
}

// where block bi of MCU mcu goes in the planes (decode_segment's layout)
JPG_HD uint8_t* block_dst(const Info* I, uint8_t* planes, int mcu, int bi, int* stride) {
    const int hs = I->hs, hv = I->hs * I->vs, mcus_x = I->mcus_x;
    const int mx = mcu % mcus_x, my = mcu / mcus_x;
    if (I->ncomp == 1) {
        *stride = mcus_x * 8;
        return planes + ((size_t)my * 8) * *stride + (size_t)mx * 8;
    }
    if (bi < hv) {
        *stride = luma_stride(I);
        return planes + ((size_t)(my * I->vs + bi / hs) * 8) * *stride + (size_t)(mx * hs + bi % hs) * 8;
    }
    *stride = chroma_stride(I);
    return planes + luma_bytes(I) + (bi - hv == 1 ? chroma_bytes(I) : 0) + ((size_t)my * 8) * *stride + (size_t)mx * 8;
}

// block b of the image (MCU-major, as the scan has them): blk, its 64 dequantised coefficients in natural order (in place) -> samples
JPG_HD void idct_block(const Info* I, int b, int32_t* blk, uint8_t* planes) {
    const int nblk = I->ncomp == 1 ? 1 : I->hs * I->vs + 2;
    int stride;
    uint8_t* dst = block_dst(I, planes, b / nblk, b % nblk, &stride);
    idct_store(blk, dst, stride);
}

// ---------------------------------------------------------------- stage 2: one pixel
JPG_HD int clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// the chroma sample of plane c (stride cs) at full-resolution (x, y)
JPG_HD int chroma_at(const Info* I, const uint8_t* c, int cs, int x, int y) {
    if (I->hs == 1) return c[(size_t)y * cs + x];
    const int cw = (I->width + 1) >> 1, i = x >> 1;
    if (I->vs == 1) {
        const uint8_t* row = c + (size_t)y * cs;
        const int cur = row[i];
        if (cw <= 2) return cur;
        if (x & 1) return i == cw - 1 ? cur : (3 * cur + row[i + 1] + 2) >> 2;
        return i == 0 ? cur : (3 * cur + row[i - 1] + 1) >> 2;
    }
    const int ch = (I->height + 1) >> 1, j = y >> 1;
    const uint8_t* near = c + (size_t)j * cs;
    if (cw <= 2) return near[i];
    const int jf = (y & 1) ? (j + 1 < ch ? j + 1 : ch - 1) : (j > 0 ? j - 1 : 0);
    const uint8_t* far = c + (size_t)jf * cs;
    const int cur = 3 * near[i] + far[i];
    if (x & 1) return i == cw - 1 ? (4 * cur + 7) >> 4 : (3 * cur + 3 * near[i + 1] + far[i + 1] + 7) >> 4;
    return i == 0 ? (4 * cur + 8) >> 4 : (3 * cur + 3 * near[i - 1] + far[i - 1] + 8) >> 4;
}

JPG_HD void pixel_rgb(const Info* I, const uint8_t* planes, int x, int y, int* r, int* g, int* b) {
    if (I->ncomp == 1) {
        *r = *g = *b = planes[(size_t)y * (I->mcus_x * 8) + x];
        return;
    }
    const int Y = planes[(size_t)y * luma_stride(I) + x];
    const uint8_t* pcb = planes + luma_bytes(I);
    const int cs = chroma_stride(I);
    const int cb = chroma_at(I, pcb, cs, x, y) - 128, cr = chroma_at(I, pcb + chroma_bytes(I), cs, x, y) - 128;
    *r = clamp255(Y + ((91881 * cr + 32768) >> 16));
    *g = clamp255(Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16));
    *b = clamp255(Y + ((116130 * cb + 32768) >> 16));
}

// ---------------------------------------------------------------- host: parse
struct Reader {
    const uint8_t* d;
    int64_t n;
    int be16(int64_t p) const { return (d[p] << 8) | d[p + 1]; }
};

// the decode form of one DHT table; false when libjpeg would refuse it
inline bool build_huff(const uint8_t counts[16], const uint8_t* vals, int nvals, bool is_dc, Huff* h) {
    memset(h, 0, sizeof(*h));
    int code = 0, p = 0;
    for (int l = 1; l <= 16; ++l) {
        const int cnt = counts[l - 1];
        h->valoff[l] = p - code;
        for (int i = 0; i < cnt; ++i, ++p, ++code) {
            if (p >= nvals || p >= 256) return false;
            h->huffval[p] = vals[p];
            if (is_dc && vals[p] > 15) return false;
            if (l <= 8) {
                const int first = code << (8 - l), span = 1 << (8 - l);
                if (first + span > 256) return false;
                for (int e = 0; e < span; ++e) h->look[first + e] = (uint16_t)((l << 8) | vals[p]);
            }
        }
        h->maxcode[l] = cnt ? code - 1 : -1;
        if (code >= (1 << l)) return false;      // over-subscribed, or the all-ones code in use
        code <<= 1;
    }
    h->maxcode[0] = -1;
    h->maxcode[17] = 0x7fffffff;
    return true;
}

// include/bvc.h, bvc_jpeg_parse
inline int parse(const uint8_t* data, int64_t n, Info* info, int32_t* seg, int max_seg) {
    memset(info, 0, sizeof(*info));
    auto refuse = [&](int why) { info->reason = why; return why; };
    if (n < 4 || data[0] != 0xFF || data[1] != 0xD8) return refuse(BVC_JPEG_REFUSE_NOT_JPEG);
    if (n > 0x7fffffff) return refuse(BVC_JPEG_REFUSE_BAD_LENGTH);
    const Reader R = {data, n};
    bool have_sof = false, jfif = false, adobe = false, have_q[4] = {false, false, false, false}, have_h[4] = {false, false, false, false};
    int transform = -1, comp_id[3] = {0, 0, 0}, comp_h[3] = {0, 0, 0}, comp_v[3] = {0, 0, 0};
    int64_t pos = 2;
    for (;;) {
        if (pos + 2 > n) return refuse(BVC_JPEG_REFUSE_BAD_LENGTH);
        if (data[pos] != 0xFF) return refuse(BVC_JPEG_REFUSE_HEADER);
        while (pos < n && data[pos] == 0xFF) ++pos;
        if (pos >= n) return refuse(BVC_JPEG_REFUSE_BAD_LENGTH);
        const int m = data[pos++];
        if (m == 0x01) continue;
        if (m == 0x00 || (m >= 0xD0 && m <= 0xD9)) return refuse(BVC_JPEG_REFUSE_HEADER);
        if (pos + 2 > n) return refuse(BVC_JPEG_REFUSE_BAD_LENGTH);
        const int L = R.be16(pos);
        if (L < 2 || pos + L > n) return refuse(BVC_JPEG_REFUSE_BAD_LENGTH);
        const int64_t body = pos + 2, stop = pos + L;
        if (m == 0xC2) return refuse(BVC_JPEG_REFUSE_PROGRESSIVE);
        if (m == 0xC3 || m == 0xC7) return refuse(BVC_JPEG_REFUSE_LOSSLESS);
        if (m >= 0xC9 && m <= 0xCF) return refuse(BVC_JPEG_REFUSE_ARITHMETIC);      // the arithmetic SOFs and DAC
        if (m == 0xC5 || m == 0xC6) return refuse(BVC_JPEG_REFUSE_HEADER);      // hierarchical
        if (m == 0xC0 || m == 0xC1) {
            if (have_sof || L < 8) return refuse(BVC_JPEG_REFUSE_HEADER);
            if (data[body] != 8) return refuse(BVC_JPEG_REFUSE_PRECISION);
            info->height = R.be16(body + 1);
            info->width = R.be16(body + 3);
            const int nc = data[body + 5];
            if (info->height < 1 || info->width < 1 || info->height > BVC_JPEG_MAX_DIM || info->width > BVC_JPEG_MAX_DIM)
                return refuse(BVC_JPEG_REFUSE_SIZE);
            if (nc != 1 && nc != 3) return refuse(BVC_JPEG_REFUSE_COMPONENTS);
            if (L != 8 + 3 * nc) return refuse(BVC_JPEG_REFUSE_BAD_LENGTH);
            info->ncomp = nc;
            for (int c = 0; c < nc; ++c) {
                comp_id[c] = data[body + 6 + 3 * c];
                comp_h[c] = data[body + 7 + 3 * c] >> 4;
                comp_v[c] = data[body + 7 + 3 * c] & 15;
                const int tq = data[body + 8 + 3 * c];
                if (tq > 3) return refuse(BVC_JPEG_REFUSE_QUANT);
                info->tq[c] = (uint8_t)tq;
                if (comp_h[c] < 1 || comp_h[c] > 4 || comp_v[c] < 1 || comp_v[c] > 4) return refuse(BVC_JPEG_REFUSE_SAMPLING);
            }
            if (nc == 3) {
                const bool luma_ok = (comp_h[0] == 1 && comp_v[0] == 1) || (comp_h[0] == 2 && comp_v[0] == 1) || (comp_h[0] == 2 && comp_v[0] == 2);
                if (!luma_ok || comp_h[1] != 1 || comp_v[1] != 1 || comp_h[2] != 1 || comp_v[2] != 1) return refuse(BVC_JPEG_REFUSE_SAMPLING);
                info->hs = comp_h[0];
                info->vs = comp_v[0];
            } else {
                info->hs = info->vs = 1;      // a scan of one component is not interleaved: its sampling factors do not matter
            }
            info->mcus_x = (info->width + 8 * info->hs - 1) / (8 * info->hs);
            info->mcus_y = (info->height + 8 * info->vs - 1) / (8 * info->vs);
            have_sof = true;
        } else if (m == 0xC4) {
            int64_t p = body;
            while (p < stop) {
                if (p + 17 > stop) return refuse(BVC_JPEG_REFUSE_BAD_LENGTH);
                const int tc = data[p] >> 4, th = data[p] & 15;
                int total = 0;
                for (int i = 0; i < 16; ++i) total += data[p + 1 + i];
                if (tc > 1 || th > 1 || total > 256) return refuse(BVC_JPEG_REFUSE_HUFFMAN);
                if (p + 17 + total > stop) return refuse(BVC_JPEG_REFUSE_BAD_LENGTH);
                if (!build_huff(data + p + 1, data + p + 17, total, tc == 0, &info->huff[2 * tc + th])) return refuse(BVC_JPEG_REFUSE_HUFFMAN);
                have_h[2 * tc + th] = true;
                p += 17 + total;
            }
        } else if (m == 0xDB) {
            int64_t p = body;
            while (p < stop) {
                const int pq = data[p] >> 4, tq = data[p] & 15;
                if (pq > 1 || tq > 3) return refuse(BVC_JPEG_REFUSE_QUANT);
                if (p + 1 + 64 * (pq + 1) > stop) return refuse(BVC_JPEG_REFUSE_BAD_LENGTH);
                for (int i = 0; i < 64; ++i)
                    info->qt[tq][natural_of(i)] = (uint16_t)(pq ? R.be16(p + 1 + 2 * i) : data[p + 1 + i]);
                have_q[tq] = true;
                p += 1 + 64 * (pq + 1);
            }
        } else if (m == 0xDD) {
            if (L != 4) return refuse(BVC_JPEG_REFUSE_BAD_LENGTH);
            info->restart_interval = R.be16(body);
        } else if (m == 0xE0) {
            if (L >= 7 && memcmp(data + body, "JFIF", 5) == 0) jfif = true;
        } else if (m == 0xEE) {
            if (L >= 14 && memcmp(data + body, "Adobe", 5) == 0) {
                adobe = true;
                transform = data[body + 11];
            }
        } else if (m == 0xDA) {
            if (!have_sof) return refuse(BVC_JPEG_REFUSE_HEADER);
            if (L < 3) return refuse(BVC_JPEG_REFUSE_BAD_LENGTH);
            const int ns = data[body];
            if (ns < 1 || ns > 4 || L != 6 + 2 * ns) return refuse(BVC_JPEG_REFUSE_BAD_LENGTH);
            if (ns != info->ncomp) return refuse(BVC_JPEG_REFUSE_MULTI_SCAN);
            for (int c = 0; c < ns; ++c) {
                if (data[body + 1 + 2 * c] != comp_id[c]) return refuse(BVC_JPEG_REFUSE_SCAN_HEADER);
                const int td = data[body + 2 + 2 * c] >> 4, ta = data[body + 2 + 2 * c] & 15;
                if (td > 1 || ta > 1 || !have_h[td] || !have_h[2 + ta]) return refuse(BVC_JPEG_REFUSE_HUFFMAN);
                if (!have_q[info->tq[c]]) return refuse(BVC_JPEG_REFUSE_QUANT);
                info->td[c] = (uint8_t)td;
                info->ta[c] = (uint8_t)ta;
            }
            if (data[body + 1 + 2 * ns] != 0 || data[body + 2 + 2 * ns] != 63 || data[body + 3 + 2 * ns] != 0)
                return refuse(BVC_JPEG_REFUSE_SCAN_HEADER);
            pos = stop;
            break;
        }
        pos = stop;
    }
    if (info->ncomp == 3) {
        if (adobe && transform == 0) return refuse(BVC_JPEG_REFUSE_RGB);
        if (adobe && transform != 1) return refuse(BVC_JPEG_REFUSE_COMPONENTS);
        if (!adobe && !jfif && comp_id[0] == 'R' && comp_id[1] == 'G' && comp_id[2] == 'B') return refuse(BVC_JPEG_REFUSE_RGB);
    }
    // the scan: one pass for 0xFF
    const int total = info->mcus_x * info->mcus_y, ri = info->restart_interval;
    info->scan_begin = (int32_t)pos;
    int nseg = 0;
    int64_t seg_begin = pos, i = pos, scan_end = n;
    int end_marker = -1;
    auto emit = [&](int64_t b, int64_t e, int first, int count) {
        if (seg && nseg < max_seg) {
            seg[kSegInts * nseg + 0] = (int32_t)b;
            seg[kSegInts * nseg + 1] = (int32_t)e;
            seg[kSegInts * nseg + 2] = first;
            seg[kSegInts * nseg + 3] = count;
        }
        ++nseg;
    };
    while (i < n) {
        const uint8_t* f = (const uint8_t*)memchr(data + i, 0xFF, (size_t)(n - i));
        if (!f) break;
        i = f - data;
        int64_t j = i + 1;
        while (j < n && data[j] == 0xFF) ++j;
        if (j >= n) {      // the data end inside a run of FF
            scan_end = i;
            break;
        }
        const int m = data[j];
        if (m == 0) {      // a stuffed FF (after fill bytes the reader stops at the first of them)
            i = j + 1;
            continue;
        }
        if (m >= 0xD0 && m <= 0xD7) {
            if (ri == 0 || m - 0xD0 != (nseg & 7)) return refuse(BVC_JPEG_REFUSE_RESTART);
            if ((int64_t)(nseg + 1) * ri >= total) return refuse(BVC_JPEG_REFUSE_RESTART);      // a segment with no MCU left for it
            emit(seg_begin, i, nseg * ri, ri);
            seg_begin = i = j + 1;
            continue;
        }
        scan_end = i;
        end_marker = m;
        break;
    }
    if (end_marker >= 0 && end_marker != 0xD9) return refuse(BVC_JPEG_REFUSE_MULTI_SCAN);
    if (end_marker < 0) info->flags |= BVC_JPEG_ST_NO_EOI;
    const int first = ri ? nseg * ri : 0;
    emit(seg_begin, scan_end < seg_begin ? seg_begin : scan_end, first, total - first);
    info->scan_end = (int32_t)scan_end;
    info->nseg = nseg;
    return BVC_OK;
}

// ---------------------------------------------------------------- host twin
// include/bvc.h, bvc_jpeg_decode_host: info and seg as parse() left them (info->nseg records)
inline int decode_host(const uint8_t* data, const Info* I, const int32_t* seg, uint8_t* out) {
    std::vector<uint8_t> planes((size_t)plane_bytes(I));
    int32_t blk[64];
    int st = I->flags;
    for (int s = 0; s < I->nseg; ++s)
        st |= decode_segment(I, data, seg[kSegInts * s], seg[kSegInts * s + 1], seg[kSegInts * s + 2], seg[kSegInts * s + 3], blk, planes.data());
    const size_t plane = (size_t)I->height * I->width;
    for (int y = 0; y < I->height; ++y)
        for (int x = 0; x < I->width; ++x) {
            int r, g, b;
            pixel_rgb(I, planes.data(), x, y, &r, &g, &b);
            out[(size_t)y * I->width + x] = (uint8_t)r;
            out[plane + (size_t)y * I->width + x] = (uint8_t)g;
            out[2 * plane + (size_t)y * I->width + x] = (uint8_t)b;
        }
    return st;
}

// ---------------------------------------------------------------- host twin of the split path
// jpeg_split_kernel in plain C++, its lanes run one after another: the same chunks, the same rounds, the same placement.  coef / dc:
// the IMAGE's coefficient blocks and DC values (mcus_x * mcus_y * blocks per MCU of them).  Returns true when the true chain ended
// before the segment's last block: the caller decodes the segment again with decode_segment.  *rounds: hand-over rounds taken.
inline bool decode_segment_split(const Info* I, const uint8_t* file, int begin, int end, int first_mcu, int mcu_count, int chunk,
                                 int16_t* coef, int32_t* dc, int* rounds) {
    const int hv = I->hs * I->vs, nblk = I->ncomp == 1 ? 1 : hv + 2;
    const int bytes = end - begin, c = split_chunk_bytes(bytes, chunk), nch = (bytes + c - 1) / c, need = mcu_count * nblk;
    coef += (size_t)first_mcu * nblk * 64;
    dc += (size_t)first_mcu * nblk;
    std::vector<SplitState> guess(nch), entry(nch), exit_(nch), hand[2];
    std::vector<int> count(nch);
    hand[0].resize(nch);
    hand[1].resize(nch);
    auto stop = [&](int j) { return (uint32_t)(8 * ((int64_t)(j + 1) * c < bytes ? (j + 1) * c : bytes)); };
    for (int j = 0; j < nch; ++j) {
        entry[j] = guess[j] = j == 0 ? SplitState{0u, 0u} : split_guess(file, begin, end, j * c);
        exit_[j] = decode_chunk<false>(I, file, begin, end, stop(j), entry[j], nblk, hv, 0, 0, nullptr, nullptr, &count[j]);
        hand[0][j] = exit_[j];
    }
    int cur = 0, r = 0;
    for (int round = 1; round < nch; ++round) {
        bool any = false;
        for (int j = 0; j < nch; ++j) {
            const SplitState e = j > 0 ? split_entry(hand[cur][j - 1], guess[j]) : entry[j];
            if (!split_same(e, entry[j])) {
                entry[j] = e;
                const SplitState x = decode_chunk<false>(I, file, begin, end, stop(j), entry[j], nblk, hv, 0, 0, nullptr, nullptr, &count[j]);
                any = any || !split_same(x, exit_[j]);
                exit_[j] = x;
            }
            hand[cur ^ 1][j] = exit_[j];
        }
        cur ^= 1;
        ++r;
        if (!any) break;
    }
    *rounds = r;
    std::vector<int> first(nch);
    int total = 0;
    bool chain = true;      // the true chain: up to the first dead exit
    for (int j = 0; j < nch; ++j) {
        first[j] = total;
        if (!chain) count[j] = -1;
        total += chain ? count[j] : 0;
        chain = chain && !(exit_[j].meta & kSplitDead);
    }
    if (total < need) return true;
    for (size_t i = 0; i < (size_t)need * 64; ++i) coef[i] = 0;
    for (int j = 0; j < nch; ++j) {
        int n;
        if (count[j] >= 0) decode_chunk<true>(I, file, begin, end, stop(j), entry[j], nblk, hv, first[j], need, coef, dc, &n);
    }
    int32_t pred[3] = {0, 0, 0};
    for (int b = 0; b < need; ++b) {
        const int bi = b % nblk, comp = bi < hv ? 0 : bi - hv + 1;
        pred[comp] = add(pred[comp], dc[b]);
        dc[b] = dequant(pred[comp], I->qt[I->tq[comp] & 3][0]);
    }
    return false;
}

// include/bvc.h, bvc_jpeg_decode_host_split.  info_out[0]: segments that fell back; info_out[1]: the most rounds a segment took.
inline int decode_host_split(const uint8_t* data, const Info* I, const int32_t* seg, int split, int chunk, uint8_t* out, int32_t* info_out) {
    std::vector<uint8_t> planes((size_t)plane_bytes(I));
    const int nblk = I->ncomp == 1 ? 1 : I->hs * I->vs + 2;
    const size_t blocks = (size_t)I->mcus_x * I->mcus_y * nblk;
    std::vector<int16_t> coef;
    std::vector<int32_t> dc;
    int32_t blk[64];
    int st = I->flags;
    info_out[0] = info_out[1] = 0;
    for (int s = 0; s < I->nseg; ++s) {
        const int32_t* g = seg + kSegInts * s;
        bool whole = !seg_is_split(g[1] - g[0], split);
        if (!whole) {
            if (coef.empty()) {
                coef.resize(blocks * 64);
                dc.resize(blocks);
            }
            int rounds = 0;
            whole = decode_segment_split(I, data, g[0], g[1], g[2], g[3], chunk, coef.data(), dc.data(), &rounds);
            info_out[0] += whole;
            info_out[1] = rounds > info_out[1] ? rounds : info_out[1];
            if (!whole)
                for (int b = g[2] * nblk; b < (g[2] + g[3]) * nblk; ++b) {
                    for (int i = 1; i < 64; ++i) blk[i] = coef[(size_t)b * 64 + i];
                    blk[0] = dc[b];
                    idct_block(I, b, blk, planes.data());
                }
        }
        if (whole) st |= decode_segment(I, data, g[0], g[1], g[2], g[3], blk, planes.data());
    }
    const size_t plane = (size_t)I->height * I->width;
    for (int y = 0; y < I->height; ++y)
        for (int x = 0; x < I->width; ++x) {
            int r, g, b;
            pixel_rgb(I, planes.data(), x, y, &r, &g, &b);
            out[(size_t)y * I->width + x] = (uint8_t)r;
            out[plane + (size_t)y * I->width + x] = (uint8_t)g;
            out[2 * plane + (size_t)y * I->width + x] = (uint8_t)b;
        }
    return st;
}

}  // namespace jpg
}  // namespace bvc

// RandAugment on uint8 frames (include/bvc.h, bvc_frame_randaug): the arithmetic that the kernels of randaug.hip and the host twin share.
// Every op is "the bytes of this PIL call on an RGB frame", restated:
//
//   0 AutoContrast  per channel: lo / hi = first / last non-empty histogram bin; hi <= lo: identity; else scale = 255.0 / (hi - lo),
//                   offset = -lo * scale (f64), lut[i] = clamp(int(i * scale + offset))
//   1 Equalize      per channel: nz = the non-empty bins; fewer than two: identity; step = (sum(nz) - nz[-1]) / 255, 0: identity; else
//                   n = step / 2, and for i in turn lut[i] = min(255, n / step), n += h[i]
//   2 Invert        255 - v                       3 Posterize(bits)   v & ~(2^(8 - bits) - 1)
//   4 Solarize(t)   v < t ? v : 255 - v            5 SolarizeAdd(a)    v < 128 ? min(255, v + a) : v
//   6 Color(f)      blend with L = (19595 r + 38470 g + 7471 b + 32768) >> 16 on all three channels
//   7 Contrast(f)   blend with m = int(sum(L) / count + 0.5), the division in f64
//   8 Brightness(f) blend with 0                  9 Sharpness(f)      blend with ImageFilter.SMOOTH of the frame
//   10 .. 14 ShearX, ShearY, TranslateX, TranslateY, Rotate: augment.h's 16.16 map (rot_source); pixels without a source take `fill`
//
//   blend   t = d + f * (v - d) in f32, no contraction; out = trunc(min(max(t, 0), 255))
//   SMOOTH  the outermost rows and columns copied (the whole frame when H < 3 or W < 3); inside, in f32,
//           ss = 0.5; ss += (below[-1] k1 + below[0] k1) + below[1] k1; ss += (mid[-1] k1 + mid[0] k5) + mid[1] k1; ss += the row above
//           likewise; out = trunc(clamp(ss)), k1 = 1 / 13, k5 = 5 / 13 (Pillow's ImagingFilter3x3 starts with the row below)
//
// Ops 0 .. 5, 7 and 8 are one 256-entry table per (frame, channel) once the histograms are known.  The histograms are integers and so
// is everything derived from them up to one f64 division: the result has the same bits however the frame was tiled.
//
// This header compiles without HIP, like augment.h.
#pragma once
#include "augment.h"

#pragma clang fp contract(off)

namespace bvc {
namespace ra {

enum {
    OP_AUTOCONTRAST = 0, OP_EQUALIZE = 1, OP_INVERT = 2, OP_POSTERIZE = 3, OP_SOLARIZE = 4, OP_SOLARIZE_ADD = 5, OP_COLOR = 6,
    OP_CONTRAST = 7, OP_BRIGHTNESS = 8, OP_SHARPNESS = 9, OP_SHEAR_X = 10, OP_SHEAR_Y = 11, OP_TRANSLATE_X = 12, OP_TRANSLATE_Y = 13,
    OP_ROTATE = 14, kNumOps = 15,
    OP_COPY = 15      // no table may name it: what sanitize_stage() makes of an unknown op, and what a frame without stages runs
};
constexpr int kMaxOps = BVC_RANDAUG_MAX_OPS;
constexpr int kMaxAdd = 110;

typedef bvc_frame_randaug Entry;
typedef bvc_randaug_stage Stage;

AUG_HD bool is_stat(int op) { return op == OP_AUTOCONTRAST || op == OP_EQUALIZE || op == OP_CONTRAST; }
AUG_HD bool is_lut(int op) { return op <= OP_SOLARIZE_ADD || op == OP_CONTRAST || op == OP_BRIGHTNESS; }
AUG_HD bool is_affine(int op) { return op >= OP_SHEAR_X && op <= OP_ROTATE; }

// A stage count and a stage that keep every address in range whatever the table holds; the identity on what invalid() accepts.  The
// factor and the coefficients need no clamp: a blend ends in a clamp (a NaN as 0) and every gather tests its source index first.
AUG_HD int sanitize_nops(int nops) { return nops < 0 ? 0 : (nops > kMaxOps ? kMaxOps : nops); }
AUG_HD Stage sanitize_stage(Stage s) {
    if (s.op < 0 || s.op >= kNumOps) s.op = OP_COPY;
    const int top = s.op == OP_POSTERIZE ? 8 : (s.op == OP_SOLARIZE ? 256 : (s.op == OP_SOLARIZE_ADD ? kMaxAdd : -1));      // -1: ival is not read
    if (top >= 0) s.ival = s.ival < 0 ? 0 : (s.ival > top ? top : s.ival);
    return s;
}

// why an entry is refused (false = accepted); `msg` receives the reason
inline bool invalid(const Entry& e, int f, int H, int W, char* msg, size_t cap) {
#define RA_REFUSE(cond, ...) do { if (cond) { snprintf(msg, cap, __VA_ARGS__); return true; } } while (0)
    RA_REFUSE(e.nops < 0 || e.nops > kMaxOps, "clip_randaug: frame %d has nops %d (0 .. %d)", f, e.nops, kMaxOps);
    for (int s = 0; s < e.nops; ++s) {
        const Stage& st = e.stage[s];
        RA_REFUSE(st.op < 0 || st.op >= kNumOps, "clip_randaug: frame %d: stage %d has unknown op %d (0 .. %d)", f, s, st.op, kNumOps - 1);
        RA_REFUSE(!(st.fval >= 0.f) || !(st.fval <= 3.0e38f), "clip_randaug: frame %d: stage %d has fval %g (finite, >= 0)", f, s,
                  (double)st.fval);
        const int top = st.op == OP_POSTERIZE ? 8 : (st.op == OP_SOLARIZE ? 256 : (st.op == OP_SOLARIZE_ADD ? kMaxAdd : -1));
        RA_REFUSE(top >= 0 && (st.ival < 0 || st.ival > top), "clip_randaug: frame %d: stage %d (op %d) has ival %d (0 .. %d)", f, s, st.op,
                  st.ival, top);
        if (is_affine(st.op)) {
            RA_REFUSE(H > aug::kMaxRotEdge || W > aug::kMaxRotEdge, "clip_randaug: frame %d: stage %d maps a %d x %d frame (edges up to %d)", f, s,
                      W, H, aug::kMaxRotEdge);
            for (int i = 0; i < 6; ++i) {
                const int64_t v = st.aff[i] < 0 ? -(int64_t)st.aff[i] : (int64_t)st.aff[i];
                const int bound = i % 3 == 2 ? aug::kMaxRotOffset : aug::kMaxRotLinear;
                RA_REFUSE(v > bound, "clip_randaug: frame %d: stage %d: aff[%d] = %d out of range (|a| <= %d)", f, s, i, st.aff[i], bound);
            }
        }
    }
#undef RA_REFUSE
    return false;
}

// ---------------------------------------------------------------- per value
AUG_HD int blend_u8(int d, int v, float f) { return aug::trunc_u8((float)d + f * ((float)v - (float)d)); }
AUG_HD int luma_u8(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }

// ops 2 .. 5 and 8: the table entry of value v from the stage's parameters alone
AUG_HD int param_lut(const Stage& s, int v) {
    switch (s.op) {
        case OP_INVERT: return 255 - v;
        case OP_POSTERIZE: return v & ~((1 << (8 - s.ival)) - 1) & 255;
        case OP_SOLARIZE: return v < s.ival ? v : 255 - v;
        case OP_SOLARIZE_ADD: return v < 128 ? (v + s.ival > 255 ? 255 : v + s.ival) : v;
        case OP_BRIGHTNESS: return blend_u8(0, v, s.fval);
        default: return v;
    }
}

// ops 0, 1 and 7: the table entry of value i from the facts of the channel's histogram
AUG_HD int autocontrast_lut(int i, int lo, int hi) {
    if (hi <= lo) return i;
    const double scale = 255.0 / (double)(hi - lo);
    const double offset = -(double)lo * scale;
    const int ix = (int)((double)i * scale + offset);
    return ix < 0 ? 0 : (ix > 255 ? 255 : ix);
}
// nz non-empty bins holding `total` pixels, `last` of them in the last one
AUG_HD uint32_t equalize_step(int nz, uint32_t total, uint32_t last) { return nz <= 1 ? 0u : (total - last) / 255u; }
// `before` = the pixels in bins below i (a frame has at most 2^24 pixels: no sum leaves uint32)
AUG_HD int equalize_lut(int i, uint32_t before, uint32_t step) {
    if (step == 0) return i;
    const uint32_t q = (step / 2 + before) / step;
    return q > 255u ? 255 : (int)q;
}
// `sum` = the sum of L over the frame's `count` pixels
AUG_HD int contrast_mean(uint32_t sum, uint32_t count) { return (int)((double)sum / (double)count + 0.5); }

// SMOOTH at one interior pixel from the row above (u), its own row (m) and the row below (d), left to right
AUG_HD int smooth9_u8(int u0, int u1, int u2, int m0, int m1, int m2, int d0, int d1, int d2) {
    const float k1 = 1.0f / 13.0f, k5 = 5.0f / 13.0f;
    float ss = 0.5f;
    ss = ss + (((float)d0 * k1 + (float)d1 * k1) + (float)d2 * k1);
    ss = ss + (((float)m0 * k1 + (float)m1 * k5) + (float)m2 * k1);
    ss = ss + (((float)u0 * k1 + (float)u1 * k1) + (float)u2 * k1);
    return aug::trunc_u8(ss);
}
// the same from memory: each argument points at the left one of that row's three values
AUG_HD int smooth_u8(const uint8_t* up, const uint8_t* mid, const uint8_t* down) {
    return smooth9_u8(up[0], up[1], up[2], mid[0], mid[1], mid[2], down[0], down[1], down[2]);
}

// ---------------------------------------------------------------- host twin
// the three tables of a statistics op from the frame as it stands
inline void stat_luts_host(const Stage& st, const uint8_t* src, int H, int W, uint8_t (&lut)[3][256]) {
    const size_t plane = (size_t)H * W;
    if (st.op == OP_CONTRAST) {
        uint32_t sum = 0;
        for (size_t i = 0; i < plane; ++i) sum += (uint32_t)luma_u8(src[i], src[plane + i], src[2 * plane + i]);
        const int m = contrast_mean(sum, (uint32_t)plane);
        for (int v = 0; v < 256; ++v) lut[0][v] = lut[1][v] = lut[2][v] = (uint8_t)blend_u8(m, v, st.fval);
        return;
    }
    for (int c = 0; c < 3; ++c) {
        uint32_t h[256] = {0};
        for (size_t i = 0; i < plane; ++i) ++h[src[c * plane + i]];
        int lo = 256, hi = -1, nz = 0;
        for (int i = 0; i < 256; ++i)
            if (h[i]) { lo = i < lo ? i : lo; hi = i; ++nz; }
        const uint32_t step = equalize_step(nz, (uint32_t)plane, hi >= 0 ? h[hi] : 0u);
        uint32_t before = 0;
        for (int i = 0; i < 256; ++i) {
            lut[c][i] = (uint8_t)(st.op == OP_AUTOCONTRAST ? autocontrast_lut(i, lo, hi) : equalize_lut(i, before, step));
            before += h[i];
        }
    }
}

// one stage on one frame, src -> dst (they do not overlap)
inline void stage_host(const Stage& st, const uint8_t* fill, const uint8_t* src, uint8_t* dst, int H, int W) {
    const size_t plane = (size_t)H * W;
    if (is_lut(st.op)) {
        uint8_t lut[3][256];
        if (is_stat(st.op)) {
            stat_luts_host(st, src, H, W, lut);
        } else {
            for (int v = 0; v < 256; ++v) lut[0][v] = lut[1][v] = lut[2][v] = (uint8_t)param_lut(st, v);
        }
        for (int c = 0; c < 3; ++c)
            for (size_t i = 0; i < plane; ++i) dst[c * plane + i] = lut[c][src[c * plane + i]];
    } else if (st.op == OP_COLOR) {
        for (size_t i = 0; i < plane; ++i) {
            const int L = luma_u8(src[i], src[plane + i], src[2 * plane + i]);
            for (int c = 0; c < 3; ++c) dst[c * plane + i] = (uint8_t)blend_u8(L, src[c * plane + i], st.fval);
        }
    } else if (st.op == OP_SHARPNESS) {
        for (int c = 0; c < 3; ++c)
            for (int y = 0; y < H; ++y)
                for (int x = 0; x < W; ++x) {
                    const uint8_t* p = src + c * plane + (size_t)y * W + x;
                    const bool inner = y >= 1 && y + 1 < H && x >= 1 && x + 1 < W;
                    const int d = inner ? smooth_u8(p - W - 1, p - 1, p + W - 1) : (int)*p;
                    dst[c * plane + (size_t)y * W + x] = (uint8_t)blend_u8(d, *p, st.fval);
                }
    } else if (is_affine(st.op)) {
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                int xin, yin;
                const bool inside = aug::rot_source(st.aff, x, y, H, W, &xin, &yin);
                for (int c = 0; c < 3; ++c) dst[c * plane + (size_t)y * W + x] = inside ? src[c * plane + (size_t)yin * W + xin] : fill[c];
            }
    } else {
        for (size_t i = 0; i < 3 * plane; ++i) dst[i] = src[i];
    }
}

// The whole stage on host memory: per frame its stages in order, each on the frame as the one before left it.
inline void clip_randaug_host(const uint8_t* in, const Entry* table, int F, int H, int W, uint8_t* out) {
    const size_t frame = (size_t)3 * H * W;
    std::vector<uint8_t> a(frame), b(frame);
    for (int f = 0; f < F; ++f) {
        const Entry& e = table[f];
        const int n = sanitize_nops(e.nops);
        for (size_t i = 0; i < frame; ++i) a[i] = in[(size_t)f * frame + i];
        for (int s = 0; s < n; ++s) {
            stage_host(sanitize_stage(e.stage[s]), e.fill, a.data(), b.data(), H, W);
            a.swap(b);
        }
        for (size_t i = 0; i < frame; ++i) out[(size_t)f * frame + i] = a[i];
    }
}

}  // namespace ra
}  // namespace bvc

// Clip transforms (include/bvc.h, bvc_frame_aug and bvc_frame_post): the arithmetic that the kernels of augment.hip and the host twins share.
//
// Geometry, per output frame: region (x0, y0, w, h) of the source frame -> antialiased bilinear resize to (Hr, Wr) -> the Ho x Wo
// window at (oy, ox) -> optional mirror of the columns.  The resize is separable and runs as torch's upsample_bilinear2d_aa and PIL's
// Image.resize(BILINEAR) run it on uint8 images: a horizontal pass rounded half-up to uint8, then a vertical pass rounded half-up to
// uint8.  Taps of output index i along an axis of `n` source samples resized to `m`:
//     scale = n / m, support = max(1, scale), center = scale (i + 0.5),
//     first = max(0, int(center - support + 0.5)), end = min(n, int(center + support + 0.5)),
//     w_k = max(0, 1 - |(k - center + 0.5) / max(1, scale)|) for k in [first, end), divided by their sum
// all in f64 (at::native's _compute_indices_min_size_weights_aa with the triangle filter, as its uint8 path calls it), then turned
// into fixed point at the precision torch derives from the axis' largest weight (below, "geometry"): the resize reproduces
// F.interpolate(uint8, mode="bilinear", antialias=True) bit for bit.  With n == m the taps are {1, 0}: the frame is copied.
//
// Colour, on the uint8 values of the resized window, every stage in f32 and back to uint8 as torchvision's tensor functions do:
//     brightness  trunc(clamp(f * v))                         contrast  trunc(clamp(f * v + (1 - f) * mean))
//     saturation  trunc(clamp(f * v + (1 - f) * gray))        hue       uint8 -> v / 255 -> HSV, h + f mod 1, -> RGB, trunc(v * (256 - 1e-3))
//     gray = trunc(0.2989 r + 0.587 g + 0.114 b);  mean = the mean of gray over the whole frame as it stands when the contrast stage
//     runs: an integer sum divided once, so it has the same bits however the frame was tiled.
//
// This header compiles without HIP (the stand-alone sanitizer check of the host twin includes nothing else).
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../include/bvc.h"

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define AUG_HD __host__ __device__ __forceinline__
#else
#define AUG_HD inline
#endif

// no contraction of a * b + c into an fma anywhere below (and in augment.hip, which includes this): the kernels and the host twin then
// perform the same f32 operations in the same order and agree bit for bit
#pragma clang fp contract(off)

namespace bvc {
namespace aug {

enum { OP_BRIGHTNESS = 0, OP_CONTRAST = 1, OP_SATURATION = 2, OP_HUE = 3 };
constexpr int kMaxScale = BVC_AUG_MAX_SCALE;   // largest region / resized ratio per axis
constexpr int kMaxTaps = 2 * kMaxScale + 4;    // end - first <= 2 support + 1
constexpr int kMaxResized = 1 << 14;           // largest resized edge: bounds the per-axis scan for the largest weight

typedef bvc_frame_aug Entry;

// An entry with every index forced into range, so that no address formed from it leaves the source or the output; the identity
// on entries that validate() accepts.
AUG_HD Entry sanitize(Entry e, int F_src, int Hs, int Ws, int Ho, int Wo) {
    e.src = e.src < 0 ? 0 : (e.src >= F_src ? F_src - 1 : e.src);
    e.x0 = e.x0 < 0 ? 0 : (e.x0 >= Ws ? Ws - 1 : e.x0);
    e.y0 = e.y0 < 0 ? 0 : (e.y0 >= Hs ? Hs - 1 : e.y0);
    e.w = e.w < 1 ? 1 : (e.w > Ws - e.x0 ? Ws - e.x0 : e.w);
    e.h = e.h < 1 ? 1 : (e.h > Hs - e.y0 ? Hs - e.y0 : e.h);
    e.Wr = e.Wr < Wo ? Wo : (e.Wr > kMaxResized && kMaxResized >= Wo ? kMaxResized : e.Wr);
    e.Hr = e.Hr < Ho ? Ho : (e.Hr > kMaxResized && kMaxResized >= Ho ? kMaxResized : e.Hr);
    if (e.w > (int64_t)kMaxScale * e.Wr) e.w = kMaxScale * e.Wr;
    if (e.h > (int64_t)kMaxScale * e.Hr) e.h = kMaxScale * e.Hr;
    e.ox = e.ox < 0 ? 0 : (e.ox > e.Wr - Wo ? e.Wr - Wo : e.ox);
    e.oy = e.oy < 0 ? 0 : (e.oy > e.Hr - Ho ? e.Hr - Ho : e.oy);
    e.nops = e.nops < 0 ? 0 : (e.nops > 4 ? 4 : e.nops);
    return e;
}

// why an entry is refused (false = accepted); `msg` receives the reason
inline bool invalid(const Entry& e, int f, int F_src, int Hs, int Ws, int Ho, int Wo, char* msg, size_t cap) {
#define AUG_REFUSE(cond, ...) do { if (cond) { snprintf(msg, cap, __VA_ARGS__); return true; } } while (0)
    AUG_REFUSE(e.src < 0 || e.src >= F_src, "clip_transform: frame %d names source frame %d of %d", f, e.src, F_src);
    AUG_REFUSE(e.w < 1 || e.h < 1, "clip_transform: frame %d has an empty region (%d x %d)", f, e.w, e.h);
    AUG_REFUSE(e.x0 < 0 || e.y0 < 0 || (int64_t)e.x0 + e.w > Ws || (int64_t)e.y0 + e.h > Hs,
               "clip_transform: frame %d: region (x0 %d, y0 %d, %d x %d) lies outside the %d x %d source", f, e.x0, e.y0, e.w, e.h, Ws, Hs);
    AUG_REFUSE(e.Hr < 1 || e.Wr < 1 || e.Hr > kMaxResized || e.Wr > kMaxResized, "clip_transform: frame %d resizes to %d x %d (1 .. %d)", f,
               e.Wr, e.Hr, kMaxResized);
    AUG_REFUSE(e.ox < 0 || e.oy < 0 || (int64_t)e.ox + Wo > e.Wr || (int64_t)e.oy + Ho > e.Hr,
               "clip_transform: frame %d: window (ox %d, oy %d, %d x %d) lies outside the %d x %d resized image", f, e.ox, e.oy, Wo, Ho,
               e.Wr, e.Hr);
    AUG_REFUSE(e.w > (int64_t)kMaxScale * e.Wr || e.h > (int64_t)kMaxScale * e.Hr,
               "clip_transform: frame %d shrinks %d x %d to %d x %d, more than the supported factor %d per axis", f, e.w, e.h, e.Wr, e.Hr,
               kMaxScale);
    AUG_REFUSE(e.nops < 0 || e.nops > 4, "clip_transform: frame %d has %d colour stages (0 .. 4)", f, e.nops);
    int seen = 0;
    for (int i = 0; i < e.nops; ++i) {
        const int op = (e.order >> (4 * i)) & 15;
        AUG_REFUSE(op > OP_HUE, "clip_transform: frame %d: stage %d has unknown op %d", f, i, op);
        AUG_REFUSE(seen & (1 << op), "clip_transform: frame %d: op %d appears twice", f, op);
        seen |= 1 << op;
        const float v = e.factor[op];
        AUG_REFUSE(!(op == OP_HUE ? (v >= -0.5f && v <= 0.5f) : v >= 0.f) || v > 1e6f,
                   "clip_transform: frame %d: factor %g of op %d out of range", f, (double)v, op);
    }
#undef AUG_REFUSE
    return false;
}

// ---------------------------------------------------------------- geometry
// Fixed point, as torch's uint8 path (and PIL's) has it: the f64 weights of an axis become integers w * 2^p, p the largest
// precision below 22 at which the largest weight OF THE WHOLE RESIZED AXIS still fits 15 bits, and a pass is
// (2^(p-1) + sum w_k v_k) >> p, clamped.  Integer sums: the host and the device cannot disagree.
struct Axis {
    double scale, support, invscale;
    int n;     // source samples of the region along this axis
};
AUG_HD Axis make_axis(int region, int resized) {
    Axis a;
    a.scale = (double)region / (double)resized;
    a.support = a.scale >= 1.0 ? a.scale : 1.0;
    a.invscale = a.scale >= 1.0 ? 1.0 / a.scale : 1.0;
    a.n = region;
    return a;
}
// taps of resized index i: first source sample (relative to the region) and count; the filter's centre in *center
AUG_HD int tap_range(const Axis& a, int i, int* first, double* center) {
    const double c = a.scale * ((double)i + 0.5);
    int lo = (int)(c - a.support + 0.5), hi = (int)(c + a.support + 0.5);
    lo = lo < 0 ? 0 : (lo > a.n - 1 ? a.n - 1 : lo);
    hi = hi > a.n ? a.n : hi;
    const int count = hi - lo;
    *first = lo;
    *center = c;
    return count < 1 ? 1 : (count > kMaxTaps ? kMaxTaps : count);
}
// weight of source sample k before normalisation
AUG_HD double tap_raw(const Axis& a, double center, int k) {
    double x = ((double)k - center + 0.5) * a.invscale;
    x = x < 0.0 ? -x : x;
    return x < 1.0 ? 1.0 - x : 0.0;
}
// the largest normalised weight of index i (the quotient of the largest: dividing by one positive total keeps the order)
AUG_HD double max_weight(const Axis& a, int i) {
    int first;
    double center, total = 0.0, m = 0.0;
    const int count = tap_range(a, i, &first, &center);
    for (int k = 0; k < count; ++k) {
        const double r = tap_raw(a, center, first + k);
        total = total + r;
        m = r > m ? r : m;
    }
    return total > 0.0 ? m / total : 1.0;
}
AUG_HD int precision_of(double wmax) {
    int p = 0;
    for (; p < 22; ++p)
        if ((int)(0.5 + wmax * (double)(1 << (p + 1))) >= (1 << 15)) break;
    return p < 1 ? 1 : p;
}
// the normalised weights of index i as integers at precision p
AUG_HD int taps(const Axis& a, int i, int p, int* wi, int* first) {
    double center, total = 0.0;
    const int count = tap_range(a, i, first, &center);
    for (int k = 0; k < count; ++k) total = total + tap_raw(a, center, *first + k);
    for (int k = 0; k < count; ++k) {
        const double w = total > 0.0 ? tap_raw(a, center, *first + k) / total : (k == 0 ? 1.0 : 0.0);   // total == 0: unreachable for accepted entries
        wi[k] = (int)(0.5 + w * (double)(1 << p));
    }
    return count;
}
AUG_HD int fixed_u8(int acc, int p) {
    const int v = (acc + (1 << (p - 1))) >> p;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// ---------------------------------------------------------------- colour
AUG_HD int trunc_u8(float v) {
    v = v > 0.f ? (v < 255.f ? v : 255.f) : 0.f;      // a NaN (a factor no accepted entry has) ends as 0
    return (int)v;
}
AUG_HD int gray_u8(const int (&p)[3]) { return (int)((0.2989f * (float)p[0] + 0.587f * (float)p[1]) + 0.114f * (float)p[2]); }
AUG_HD int blend_u8(int a, float b, float ratio) { return trunc_u8(ratio * (float)a + (1.0f - ratio) * b); }

AUG_HD void hue_u8(int (&p)[3], float shift) {
    const float r = (float)p[0] / 255.0f, g = (float)p[1] / 255.0f, b = (float)p[2] / 255.0f;
    const float maxc = fmaxf(r, fmaxf(g, b)), minc = fminf(r, fminf(g, b));
    const bool eqc = maxc == minc;
    const float cr = maxc - minc;
    const float s = cr / (eqc ? 1.0f : maxc);
    const float div = eqc ? 1.0f : cr;
    const float rc = (maxc - r) / div, gc = (maxc - g) / div, bc = (maxc - b) / div;
    float h;
    if (maxc == r) h = bc - gc;
    else if (maxc == g) h = (2.0f + rc) - bc;
    else h = (4.0f + gc) - rc;
    h = h / 6.0f + 1.0f;
    h = h - floorf(h);
    h = h + shift;
    h = h - floorf(h);
    h = h >= 0.f ? h : 0.f;      // only a NaN shift gets here
    const float h6 = h * 6.0f;
    const float fl = floorf(h6);
    const float f = h6 - fl;
    const int i = ((int)fl) % 6;
    const float v = maxc;
    float pp = v * (1.0f - s), q = v * (1.0f - s * f), t = v * (1.0f - s * (1.0f - f));
    pp = fminf(fmaxf(pp, 0.f), 1.f); q = fminf(fmaxf(q, 0.f), 1.f); t = fminf(fmaxf(t, 0.f), 1.f);
    float o0, o1, o2;
    switch (i) {
        case 0: o0 = v; o1 = t; o2 = pp; break;
        case 1: o0 = q; o1 = v; o2 = pp; break;
        case 2: o0 = pp; o1 = v; o2 = t; break;
        case 3: o0 = pp; o1 = q; o2 = v; break;
        case 4: o0 = t; o1 = pp; o2 = v; break;
        default: o0 = v; o1 = pp; o2 = q; break;
    }
    const float back = 255.0f + 1.0f - 1e-3f;
    p[0] = (int)(o0 * back); p[1] = (int)(o1 * back); p[2] = (int)(o2 * back);
}

// stages [from, to) of the entry's chain on one pixel; `mean` serves a contrast stage in that range
AUG_HD void stages(const Entry& e, int from, int to, float mean, int (&p)[3]) {
    for (int i = from; i < to; ++i) {
        const int op = (e.order >> (4 * i)) & 15;
        const float f = e.factor[op & 3];
        if (op == OP_BRIGHTNESS) {
            for (int c = 0; c < 3; ++c) p[c] = blend_u8(p[c], 0.f, f);
        } else if (op == OP_CONTRAST) {
            for (int c = 0; c < 3; ++c) p[c] = blend_u8(p[c], mean, f);
        } else if (op == OP_SATURATION) {
            const float g = (float)gray_u8(p);
            for (int c = 0; c < 3; ++c) p[c] = blend_u8(p[c], g, f);
        } else {
            hue_u8(p, f);
        }
    }
}
AUG_HD void to_gray(int (&p)[3]) { p[0] = p[1] = p[2] = gray_u8(p); }
// index of the contrast stage, or nops when the chain has none: stages before it are local to a pixel
AUG_HD int contrast_at(const Entry& e) {
    for (int i = 0; i < e.nops; ++i)
        if (((e.order >> (4 * i)) & 15) == OP_CONTRAST) return i;
    return e.nops;
}
AUG_HD float gray_mean(uint64_t sum, int Ho, int Wo) { return (float)sum / (float)((int64_t)Ho * Wo); }

// ---------------------------------------------------------------- host twin
// The whole transform on host memory, frame by frame, through the functions above.
inline void clip_transform_host(const uint8_t* src, int F_src, int Hs, int Ws, const Entry* table, int F_out, int Ho, int Wo, uint8_t* out) {
    std::vector<int> wx((size_t)Wo * kMaxTaps), wy((size_t)Ho * kMaxTaps);
    std::vector<int> fx(Wo), nx(Wo), fy(Ho), ny(Ho);
    std::vector<uint8_t> hor, res((size_t)3 * Ho * Wo);
    for (int f = 0; f < F_out; ++f) {
        const Entry e = sanitize(table[f], F_src, Hs, Ws, Ho, Wo);
        const Axis ax = make_axis(e.w, e.Wr), ay = make_axis(e.h, e.Hr);
        double mx = 0.0, my = 0.0;
        for (int i = 0; i < e.Wr; ++i) mx = fmax(mx, max_weight(ax, i));
        for (int i = 0; i < e.Hr; ++i) my = fmax(my, max_weight(ay, i));
        const int px = precision_of(mx), py = precision_of(my);
        for (int j = 0; j < Wo; ++j) nx[j] = taps(ax, e.ox + j, px, &wx[(size_t)j * kMaxTaps], &fx[j]);
        for (int r = 0; r < Ho; ++r) ny[r] = taps(ay, e.oy + r, py, &wy[(size_t)r * kMaxTaps], &fy[r]);
        const int base = fy[0], span = fy[Ho - 1] + ny[Ho - 1] - base;
        hor.assign((size_t)3 * span * Wo, 0);
        const uint8_t* sf = src + (size_t)e.src * 3 * Hs * Ws;
        for (int c = 0; c < 3; ++c)
            for (int r = 0; r < span; ++r) {
                const uint8_t* row = sf + ((size_t)c * Hs + e.y0 + base + r) * Ws + e.x0;
                for (int j = 0; j < Wo; ++j) {
                    int acc = 0;
                    for (int k = 0; k < nx[j]; ++k) acc += wx[(size_t)j * kMaxTaps + k] * (int)row[fx[j] + k];
                    hor[((size_t)c * span + r) * Wo + j] = (uint8_t)fixed_u8(acc, px);
                }
            }
        const int cpos = contrast_at(e);
        uint64_t gsum = 0;
        for (int r = 0; r < Ho; ++r)
            for (int j = 0; j < Wo; ++j) {
                int p[3];
                for (int c = 0; c < 3; ++c) {
                    int acc = 0;
                    for (int k = 0; k < ny[r]; ++k)
                        acc += wy[(size_t)r * kMaxTaps + k] * (int)hor[((size_t)c * span + (fy[r] - base + k)) * Wo + j];
                    p[c] = fixed_u8(acc, py);
                }
                stages(e, 0, cpos, 0.f, p);
                if (cpos == e.nops) {
                    if (e.gray) to_gray(p);
                } else {
                    gsum += (uint64_t)gray_u8(p);
                }
                for (int c = 0; c < 3; ++c) res[((size_t)c * Ho + r) * Wo + j] = (uint8_t)p[c];
            }
        const float mean = gray_mean(gsum, Ho, Wo);
        uint8_t* of = out + (size_t)f * 3 * Ho * Wo;
        for (int r = 0; r < Ho; ++r)
            for (int j = 0; j < Wo; ++j) {
                int p[3];
                for (int c = 0; c < 3; ++c) p[c] = res[((size_t)c * Ho + r) * Wo + j];
                if (cpos < e.nops) {
                    stages(e, cpos, e.nops, mean, p);
                    if (e.gray) to_gray(p);
                }
                const int jj = e.flip ? Wo - 1 - j : j;
                for (int c = 0; c < 3; ++c) of[((size_t)c * Ho + r) * Wo + jj] = (uint8_t)p[c];
            }
    }
}

// ---------------------------------------------------------------- post stage: blur, gray, rotation (bvc_frame_post)
// Blur is Pillow's GaussianBlur: three box passes along the rows, then three along the columns, every pass rounded to uint8, taps
// beyond the frame reading the edge value of that pass's input.  One pass, in uint32 (the largest value is 255 * 2^24 + 2^23):
//     out[x] = (ww * sum_{|i| <= r} in[x + i] + fw * (in[x - r - 1] + in[x + r + 1]) + 2^23) >> 24
// Rotation is PIL's Image.rotate(NEAREST, expand=False, fillcolor=0): output pixel (x, y) copies in[yin][xin],
//     xin = (a2 + a1 y + a0 x) >> 16,  yin = (a5 + a4 y + a3 x) >> 16     (arithmetic shifts), and is 0 when that lies outside.
typedef bvc_frame_post Post;
constexpr int kMaxBoxRadius = 3;        // what BVC_AUG_MAX_BLUR_RADIUS gives
constexpr int kMaxRotEdge = 4096;       // with the coefficient bounds below every intermediate of the map stays inside int32
constexpr int kMaxRotLinear = 65537, kMaxRotOffset = 1 << 30;

// Pillow's _gaussian_blur_radius and the weights of ImagingLineBoxBlur8, with their types: f32 except where Pillow's own expression
// is evaluated in f64 (the square root and the floor), and an f32 division for ww.
inline int blur_weights(float radius, int32_t* r, uint32_t* ww, uint32_t* fw) {
    if (!(radius >= 0.f) || radius > BVC_AUG_MAX_BLUR_RADIUS) return -1;
    const float sigma2 = radius * radius / 3;
    const float L = (float)sqrt(12.0 * sigma2 + 1.0);
    const float l = (float)floor((L - 1.0) / 2.0);
    float a = (2 * l + 1) * (l * (l + 1) - 3 * sigma2);
    a /= 6 * (sigma2 - (l + 1) * (l + 1));
    const float fr = l + a;
    const int ri = (int)fr;
    const uint32_t w = (uint32_t)((float)(1 << 24) / (fr * 2 + 1));
    *r = ri;
    *ww = w;
    *fw = ((1u << 24) - (uint32_t)(2 * ri + 1) * w) / 2;
    return 0;
}

// An entry whose blur cannot leave uint32 or the halo: the radius forced into [-1, 3], weights above 2^24 in total mean "no blur".
// The identity on entries that invalid_post() accepts.  rot[] needs no clamp: every gather tests its source index first.
AUG_HD Post post_sanitize(Post p) {
    p.blur_r = p.blur_r < -1 ? -1 : (p.blur_r > kMaxBoxRadius ? kMaxBoxRadius : p.blur_r);
    if (p.blur_r >= 0 && (uint64_t)(2 * p.blur_r + 1) * p.blur_ww + 2 * (uint64_t)p.blur_fw > (1u << 24)) p.blur_r = -1;
    return p;
}

inline bool invalid_post(const Post& p, int f, int H, int W, char* msg, size_t cap) {
#define AUG_REFUSE(cond, ...) do { if (cond) { snprintf(msg, cap, __VA_ARGS__); return true; } } while (0)
    AUG_REFUSE(p.blur_r < -1 || p.blur_r > kMaxBoxRadius, "clip_post: frame %d has blur_r %d (-1 .. %d)", f, p.blur_r, kMaxBoxRadius);
    AUG_REFUSE(p.blur_r >= 0 && (uint64_t)(2 * p.blur_r + 1) * p.blur_ww + 2 * (uint64_t)p.blur_fw > (1u << 24),
               "clip_post: frame %d: blur weights (%d x %u + 2 x %u) exceed 2^24", f, 2 * p.blur_r + 1, p.blur_ww, p.blur_fw);
    if (p.rotate) {
        AUG_REFUSE(H > kMaxRotEdge || W > kMaxRotEdge, "clip_post: frame %d rotates a %d x %d frame (edges up to %d)", f, W, H, kMaxRotEdge);
        for (int i = 0; i < 6; ++i) {
            const int64_t v = p.rot[i] < 0 ? -(int64_t)p.rot[i] : (int64_t)p.rot[i];
            AUG_REFUSE(v > (i % 3 == 2 ? kMaxRotOffset : kMaxRotLinear), "clip_post: frame %d: rot[%d] = %d out of range (|a| <= %d)", f, i,
                       p.rot[i], i % 3 == 2 ? kMaxRotOffset : kMaxRotLinear);
        }
    }
#undef AUG_REFUSE
    return false;
}

// source pixel of output pixel (x, y); false = outside the frame.  Unsigned arithmetic: an entry that no call accepts wraps
// instead of overflowing, and the range test makes any result safe.
AUG_HD bool rot_source(const int32_t* a, int x, int y, int H, int W, int* xin, int* yin) {
    const int32_t xi = (int32_t)((uint32_t)a[2] + (uint32_t)a[1] * (uint32_t)y + (uint32_t)a[0] * (uint32_t)x) >> 16;
    const int32_t yi = (int32_t)((uint32_t)a[5] + (uint32_t)a[4] * (uint32_t)y + (uint32_t)a[3] * (uint32_t)x) >> 16;
    *xin = xi;
    *yin = yi;
    return xi >= 0 && xi < W && yi >= 0 && yi < H;
}

AUG_HD uint32_t box_u8(uint32_t inner, uint32_t far, uint32_t ww, uint32_t fw) { return (ww * inner + fw * far + (1u << 23)) >> 24; }

// one box pass over n samples `stride` apart
inline void box_line_host(const uint8_t* in, uint8_t* out, int n, size_t stride, int r, uint32_t ww, uint32_t fw) {
    auto at = [&](int x) { return (uint32_t)in[(size_t)(x < 0 ? 0 : (x > n - 1 ? n - 1 : x)) * stride]; };
    for (int x = 0; x < n; ++x) {
        uint32_t inner = 0;
        for (int i = -r; i <= r; ++i) inner += at(x + i);
        out[(size_t)x * stride] = (uint8_t)box_u8(inner, at(x - r - 1) + at(x + r + 1), ww, fw);
    }
}

// The post stage on host memory, whole frames at a time: blur, then gray, then rotation.
inline void clip_post_host(const uint8_t* in, const Post* table, int F, int H, int W, uint8_t* out) {
    const size_t plane = (size_t)H * W;
    std::vector<uint8_t> a(3 * plane), b(3 * plane);
    for (int f = 0; f < F; ++f) {
        const Post p = post_sanitize(table[f]);
        const uint8_t* inf = in + (size_t)f * 3 * plane;
        uint8_t* of = out + (size_t)f * 3 * plane;
        for (size_t i = 0; i < 3 * plane; ++i) a[i] = inf[i];
        if (p.blur_r >= 0) {
            for (int pass = 0; pass < 3; ++pass) {
                for (int c = 0; c < 3; ++c)
                    for (int y = 0; y < H; ++y) box_line_host(&a[c * plane + (size_t)y * W], &b[c * plane + (size_t)y * W], W, 1, p.blur_r, p.blur_ww, p.blur_fw);
                a.swap(b);
            }
            for (int pass = 0; pass < 3; ++pass) {
                for (int c = 0; c < 3; ++c)
                    for (int x = 0; x < W; ++x) box_line_host(&a[c * plane + x], &b[c * plane + x], H, (size_t)W, p.blur_r, p.blur_ww, p.blur_fw);
                a.swap(b);
            }
        }
        if (p.gray)
            for (size_t i = 0; i < plane; ++i) {
                int px[3] = {a[i], a[plane + i], a[2 * plane + i]};
                to_gray(px);
                a[i] = a[plane + i] = a[2 * plane + i] = (uint8_t)px[0];
            }
        for (int y = 0; y < H; ++y)
            for (int x = 0; x < W; ++x) {
                int xin = x, yin = y;
                const bool inside = p.rotate ? rot_source(p.rot, x, y, H, W, &xin, &yin) : true;
                for (int c = 0; c < 3; ++c) of[c * plane + (size_t)y * W + x] = inside ? a[c * plane + (size_t)yin * W + xin] : (uint8_t)0;
            }
    }
}

}  // namespace aug
}  // namespace bvc

// Stand-alone check of the clip transforms' host twins (csrc/augment.h) for a sanitizer build: runs the twin over the shapes of
// tests/test_augment_host.py, with full colour chains, border-touching regions and a table of out-of-range entries (which the twin
// must clamp, not follow), then the post twin (blur, gray, rotation) over the shapes of tests/test_augment_post_host.py and a table of
// out-of-range entries (blur_r = 9, weights that overflow, wild rot[]), and prints a checksum.  No GPU, no Python:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude tools/augment_host_check.cpp -o augment_host_check
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../baby-vision-curriculum_amd/csrc/augment.h"

using bvc::aug::Entry;

static uint32_t rng_state = 12345u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

static Entry whole(int src, int Hs, int Ws, int Ho, int Wo) {
    Entry e = {};
    e.src = src; e.w = Ws; e.h = Hs; e.Hr = Ho; e.Wr = Wo;
    e.factor[0] = e.factor[1] = e.factor[2] = 1.f;
    return e;
}

static uint64_t run(int F_src, int Hs, int Ws, const std::vector<Entry>& table, int Ho, int Wo, bool must_be_valid) {
    std::vector<uint8_t> src((size_t)F_src * 3 * Hs * Ws), out((size_t)table.size() * 3 * Ho * Wo);
    for (auto& v : src) v = (uint8_t)rnd();
    char msg[512];
    for (size_t f = 0; f < table.size(); ++f)
        if (bvc::aug::invalid(table[f], (int)f, F_src, Hs, Ws, Ho, Wo, msg, sizeof(msg)) && must_be_valid) {
            fprintf(stderr, "unexpected refusal: %s\n", msg);
            exit(1);
        }
    bvc::aug::clip_transform_host(src.data(), F_src, Hs, Ws, table.data(), (int)table.size(), Ho, Wo, out.data());
    uint64_t sum = 0;
    for (auto v : out) sum = sum * 31 + v;
    return sum;
}

using bvc::aug::Post;

static Post post_entry(float radius, int gray, double angle, int H, int W) {
    Post p = {};
    p.blur_r = -1;
    if (radius >= 0.f && bvc::aug::blur_weights(radius, &p.blur_r, &p.blur_ww, &p.blur_fw) != 0) {
        fprintf(stderr, "unexpected refusal of radius %g\n", (double)radius);
        exit(1);
    }
    p.gray = gray;
    if (angle > -1000.0) {      // a plain f64 matrix is enough here: Pillow's rounding of it is bvc.augment.rotation_coeffs' business
        const double t = -angle * 3.14159265358979323846 / 180.0, m[6] = {cos(t), sin(t), 0, -sin(t), cos(t), 0};
        const double cx = W / 2.0, cy = H / 2.0;
        const double m2 = m[0] * -cx + m[1] * -cy + cx, m5 = m[3] * -cx + m[4] * -cy + cy;
        auto fix = [](double v) { return (int32_t)floor(v * 65536.0 + 0.5); };
        p.rotate = 1;
        p.rot[0] = fix(m[0]); p.rot[1] = fix(m[1]); p.rot[2] = fix(m2 + 0.5 * m[0] + 0.5 * m[1]);
        p.rot[3] = fix(m[3]); p.rot[4] = fix(m[4]); p.rot[5] = fix(m5 + 0.5 * m[3] + 0.5 * m[4]);
    }
    return p;
}

static uint64_t run_post(int H, int W, const std::vector<Post>& table, bool must_be_valid) {
    const size_t n = table.size() * 3 * (size_t)H * W;
    std::vector<uint8_t> in(n), out(n);
    for (auto& v : in) v = (uint8_t)rnd();
    char msg[512];
    for (size_t f = 0; f < table.size(); ++f)
        if (bvc::aug::invalid_post(table[f], (int)f, H, W, msg, sizeof(msg)) == must_be_valid) {
            if (must_be_valid) fprintf(stderr, "unexpected refusal: %s\n", msg);
            else fprintf(stderr, "entry %d of the out-of-range table was accepted\n", (int)f);
            exit(1);
        }
    bvc::aug::clip_post_host(in.data(), table.data(), (int)table.size(), H, W, out.data());
    uint64_t sum = 0;
    for (auto v : out) sum = sum * 31 + v;
    return sum;
}

static uint64_t post_checks() {
    const int shapes[][2] = {{1, 9}, {2, 5}, {3, 3}, {17, 40}, {33, 65}, {24, 24}, {64, 48}, {1, 1}};
    const float radii[] = {0.f, 0.1f, 0.3f, 1.0f, 2.0f, 4.0f};
    const double angles[] = {0.0, 90.0, -90.0, 45.0, -45.0, 1e-3, 180.0, -37.5};
    uint64_t sum = 0;
    for (const auto& s : shapes) {
        const int H = s[0], W = s[1];
        std::vector<Post> t;
        for (float r : radii) t.push_back(post_entry(r, 0, -2000.0, H, W));
        for (double a : angles) t.push_back(post_entry(-1.f, 0, a, H, W));
        t.push_back(post_entry(1.3f, 1, 30.0, H, W));
        t.push_back(post_entry(-1.f, 1, -2000.0, H, W));
        t.push_back(post_entry(-1.f, 0, -2000.0, H, W));
        sum ^= run_post(H, W, t, true);
        // entries the op refuses: the twin clamps the radius, takes over-weight entries as "no blur" and tests every gather
        std::vector<Post> bad;
        for (int i = 0; i < 12; ++i) {
            Post p = post_entry(1.0f, i & 1, -2000.0, H, W);
            if (i % 3 == 0) p.blur_r = 9;
            if (i == 0) p.blur_ww = p.blur_fw = 1000u;      // light enough to run: the radius is clamped to 3
            if (i % 3 == 1) { p.blur_ww = 0xFFFFFFFFu - rnd(); p.blur_fw = 0xFFFFFFFFu - rnd(); }
            if (i % 3 == 2) p.blur_r = -7 - i;
            if (i >= 4 || i % 3 == 2) {
                p.rotate = 1;
                for (int k = 0; k < 6; ++k) p.rot[k] = (int32_t)((rnd() << 8) ^ rnd());
                p.rot[i % 6] = i & 1 ? INT32_MIN : INT32_MAX;
            }
            bad.push_back(p);
        }
        sum ^= run_post(H, W, bad, false);
    }
    int32_t r;
    uint32_t ww, fw;
    const float refused[] = {-1.f, 4.5f, NAN, INFINITY};
    for (float v : refused)
        if (bvc::aug::blur_weights(v, &r, &ww, &fw) == 0) {
            fprintf(stderr, "radius %g was accepted\n", (double)v);
            exit(1);
        }
    return sum;
}

int main() {
    const int shapes[][4] = {{37, 53, 16, 16}, {9, 12, 16, 16}, {64, 48, 16, 24}, {53, 37, 32, 16}, {17, 16, 16, 16}, {240, 320, 32, 32},
                             {16, 16, 16, 16}, {256, 340, 224, 224}, {400, 70, 64, 48}, {57, 71, 40, 40}};
    uint64_t sum = 0;
    for (const auto& s : shapes) {
        const int Hs = s[0], Ws = s[1], Ho = s[2], Wo = s[3];
        std::vector<Entry> t;
        t.push_back(whole(0, Hs, Ws, Ho, Wo));
        for (int i = 0; i < 8; ++i) {       // random regions, the last four touching a border each; full chains in rotating order
            Entry e = whole(i % 2, Hs, Ws, Ho, Wo);
            e.w = 1 + (int)(rnd() % Ws); e.h = 1 + (int)(rnd() % Hs);
            if (e.w > 16 * Wo) e.w = 16 * Wo;
            if (e.h > 16 * Ho) e.h = 16 * Ho;
            e.x0 = i == 4 ? 0 : (i == 5 ? Ws - e.w : (int)(rnd() % (Ws - e.w + 1)));
            e.y0 = i == 6 ? 0 : (i == 7 ? Hs - e.h : (int)(rnd() % (Hs - e.h + 1)));
            e.flip = i & 1; e.gray = (i >> 1) & 1; e.nops = 4;
            const int perm[4][4] = {{0, 1, 2, 3}, {1, 0, 3, 2}, {3, 2, 1, 0}, {2, 3, 0, 1}};
            for (int k = 0; k < 4; ++k) e.order |= perm[i % 4][k] << (4 * k);
            e.factor[0] = 0.2f + 1.6f * (float)(rnd() % 1000) / 999.f;
            e.factor[1] = 0.2f + 1.6f * (float)(rnd() % 1000) / 999.f;
            e.factor[2] = 0.2f + 1.6f * (float)(rnd() % 1000) / 999.f;
            e.factor[3] = -0.2f + 0.4f * (float)(rnd() % 1000) / 999.f;
            t.push_back(e);
        }
        sum ^= run(2, Hs, Ws, t, Ho, Wo, true);
        // Resize + CenterCrop: the window inside a larger resized image
        Entry c = whole(1, Hs, Ws, Ho + 5, Wo + 9);
        c.oy = 2; c.ox = 4;
        sum ^= run(2, Hs, Ws, {c}, Ho, Wo, true);
        // entries the op refuses: the twin clamps them before it forms an address
        std::vector<Entry> bad;
        for (int i = 0; i < 12; ++i) {
            Entry e = whole((int)rnd() - (1 << 23), Hs, Ws, Ho, Wo);
            e.x0 = (int)(rnd() % 4096) - 2048; e.y0 = (int)(rnd() % 4096) - 2048;
            e.w = (int)(rnd() % 100000) - 50; e.h = (int)(rnd() % 100000) - 50;
            e.Hr = (int)(rnd() % 64) - 8; e.Wr = (int)(rnd() % 64) - 8;
            e.ox = (int)(rnd() % 512) - 256; e.oy = (int)(rnd() % 512) - 256;
            e.nops = (int)(rnd() % 16) - 4; e.order = (int)rnd();
            bad.push_back(e);
        }
        sum ^= run(2, Hs, Ws, bad, Ho, Wo, false);
    }
    sum ^= post_checks();
    printf("augment_host_check ok: checksum %016llx\n", (unsigned long long)sum);
    return 0;
}

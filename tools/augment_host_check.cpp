// Stand-alone check of the clip transforms' host twin (csrc/augment.h) for a sanitizer build: runs the twin over the shapes of
// tests/test_augment_host.py, with full colour chains, border-touching regions and a table of out-of-range entries (which the twin
// must clamp, not follow), and prints a checksum.  No GPU, no Python:
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
    printf("augment_host_check ok: checksum %016llx\n", (unsigned long long)sum);
    return 0;
}

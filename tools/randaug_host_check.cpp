// Stand-alone check of RandAugment's host twin (csrc/randaug.h) for a sanitizer build: runs the twin over the shapes of
// tests/test_randaug_host.py on noise, constant, two-level and tiny frames (the histogram edge cases), every op alone at the ends of
// its range, chains of eight stages, and a table of out-of-range entries (which the twin must clamp or copy through, not follow), and
// prints a checksum.  No GPU, no Python:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude tools/randaug_host_check.cpp -o randaug_host_check
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../baby-vision-curriculum_amd/csrc/randaug.h"

using bvc::ra::Entry;
using bvc::ra::Stage;

static uint32_t rng_state = 54321u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

static Stage stage(int op, int ival, float fval, double a, double b, double c, double d, double e, double f) {
    Stage s = {};
    s.op = op; s.ival = ival; s.fval = fval;
    auto fix = [](double v) { return (int32_t)floor(v * 65536.0 + 0.5); };
    s.aff[0] = fix(a); s.aff[1] = fix(b); s.aff[2] = fix(c + 0.5 * a + 0.5 * b);
    s.aff[3] = fix(d); s.aff[4] = fix(e); s.aff[5] = fix(f + 0.5 * d + 0.5 * e);
    return s;
}

// op at one of two ends of its range (or a drawn value, which = 2)
static Stage op_stage(int op, int which, int H, int W) {
    const double u = which == 0 ? -1.0 : (which == 1 ? 1.0 : (double)(rnd() % 2001) / 1000.0 - 1.0);
    const int ival = op == bvc::ra::OP_POSTERIZE ? (which == 0 ? 0 : (which == 1 ? 8 : (int)(rnd() % 9)))
                   : op == bvc::ra::OP_SOLARIZE ? (which == 0 ? 0 : (which == 1 ? 256 : (int)(rnd() % 257)))
                                                : (which == 0 ? 0 : (which == 1 ? 110 : (int)(rnd() % 111)));
    const float fval = (float)(1.0 + 0.9 * u);
    switch (op) {
        case bvc::ra::OP_SHEAR_X: return stage(op, 0, 0.f, 1, 0.3 * u, 0, 0, 1, 0);
        case bvc::ra::OP_SHEAR_Y: return stage(op, 0, 0.f, 1, 0, 0, 0.3 * u, 1, 0);
        case bvc::ra::OP_TRANSLATE_X: return stage(op, 0, 0.f, 1, 0, (which == 2 ? 0.45 : 1.5) * u * W, 0, 1, 0);
        case bvc::ra::OP_TRANSLATE_Y: return stage(op, 0, 0.f, 1, 0, 0, 0, 1, (which == 2 ? 0.45 : 1.5) * u * H);
        case bvc::ra::OP_ROTATE: {
            const double t = -30.0 * u * 3.14159265358979323846 / 180.0, cx = W / 2.0, cy = H / 2.0;
            return stage(op, 0, 0.f, cos(t), sin(t), cos(t) * -cx + sin(t) * -cy + cx, -sin(t), cos(t), -sin(t) * -cx + cos(t) * -cy + cy);
        }
        default: return stage(op, ival, fval, 1, 0, 0, 0, 1, 0);
    }
}

static void fill_frame(uint8_t* p, size_t n, int kind) {
    for (size_t i = 0; i < n; ++i) p[i] = kind == 0 ? (uint8_t)rnd() : (kind == 1 ? (uint8_t)77 : (uint8_t)(rnd() & 1 ? 40 : 199));
}

static uint64_t run(int H, int W, const std::vector<Entry>& table, bool must_be_valid) {
    const size_t frame = (size_t)3 * H * W, n = table.size() * frame;
    std::vector<uint8_t> in(n), out(n);
    for (size_t f = 0; f < table.size(); ++f) fill_frame(&in[f * frame], frame, (int)(f % 3));
    char msg[512];
    for (size_t f = 0; f < table.size(); ++f)
        if (bvc::ra::invalid(table[f], (int)f, H, W, msg, sizeof(msg)) == must_be_valid) {
            if (must_be_valid) fprintf(stderr, "unexpected refusal: %s\n", msg);
            else fprintf(stderr, "entry %d of the out-of-range table was accepted\n", (int)f);
            exit(1);
        }
    bvc::ra::clip_randaug_host(in.data(), table.data(), (int)table.size(), H, W, out.data());
    uint64_t sum = 0;
    for (auto v : out) sum = sum * 31 + v;
    return sum;
}

int main() {
    const int shapes[][2] = {{1, 9}, {2, 5}, {3, 3}, {17, 40}, {33, 65}, {64, 64}, {1, 1}, {5, 2}};
    uint64_t sum = 0;
    for (const auto& s : shapes) {
        const int H = s[0], W = s[1];
        std::vector<Entry> t;
        for (int op = 0; op < bvc::ra::kNumOps; ++op)
            for (int which = 0; which < 3; ++which)
                for (int kind = 0; kind < 3; ++kind) {      // run() fills frame f by f % 3: every op meets every kind of frame
                    Entry e = {};
                    e.nops = 1; e.fill[0] = 124; e.fill[1] = 116; e.fill[2] = 104;
                    e.stage[0] = op_stage(op, which, H, W);
                    t.push_back(e);
                }
        for (int i = 0; i < 9; ++i) {      // chains of 0 .. 8 stages, ops repeating
            Entry e = {};
            e.nops = i;
            for (int k = 0; k < i; ++k) e.stage[k] = op_stage((int)(rnd() % bvc::ra::kNumOps), 2, H, W);
            t.push_back(e);
        }
        sum ^= run(H, W, t, true);
        // entries the op refuses: the twin clamps nops and ival, copies through an unknown op and tests every gather
        std::vector<Entry> bad;
        for (int i = 0; i < 15; ++i) {
            Entry e = {};
            e.nops = i % 3 == 0 ? 9 + (int)(rnd() % 1000) : 1 + (int)(rnd() % 8);
            for (int k = 0; k < bvc::ra::kMaxOps; ++k) {
                Stage& st = e.stage[k];
                st = op_stage((k + i) % bvc::ra::kNumOps, 2, H, W);
            }
            Stage& st = e.stage[0];
            if (i % 3 == 1) st.op = i & 1 ? 15 + (int)(rnd() % 100000) : -1 - (int)(rnd() % 100000);
            if (i % 3 == 2) {
                st.op = bvc::ra::OP_POSTERIZE + i % 3;      // an op that reads ival
                st.ival = i & 1 ? INT32_MAX - (int)(rnd() % 7) : INT32_MIN + (int)(rnd() % 7);
            }
            if (i == 3 || i == 9) { e.nops = 4; st.op = bvc::ra::OP_ROTATE; for (int k = 0; k < 6; ++k) st.aff[k] = (int32_t)((rnd() << 8) ^ rnd()); st.aff[i % 6] = INT32_MIN; }
            if (i == 6 || i == 12) { e.nops = 2; st.op = bvc::ra::OP_COLOR + i % 4; st.fval = i == 6 ? NAN : -INFINITY; }
            if (i == 0) e.nops = -5;
            bad.push_back(e);
        }
        sum ^= run(H, W, bad, false);
    }
    printf("randaug_host_check ok: checksum %016llx\n", (unsigned long long)sum);
    return 0;
}

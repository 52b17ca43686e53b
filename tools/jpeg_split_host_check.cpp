// Stand-alone check of the split path of the JPEG decode (csrc/jpeg.h: decode_chunk, decode_segment_split and the fall-back to
// decode_segment) for a sanitizer build.  jpeg_split_kernel calls the same jpeg.h functions for the reader, the tables, the chunk step
// and the bounds, so this run is where the device's bounds are proven before anything runs on a GPU.
// Arguments and inputs as tools/jpeg_host_check.cpp: fixture files (tests/golden/jpeg_*.json: every "jpeg_b64" string in them) or raw
// .jpg files; each file as it is, cut at EVERY length, with each restart segment in turn cut to half its bytes, and with 2000 seeded
// single-byte and 2000 single-bit flips.  Whatever parse accepts goes through the one-lane twin and through the split twin at the
// smallest chunk and at 64, every splittable segment split, into buffers of exactly 3 * H * W bytes; the three must agree in every
// byte and in the status, an input the twin decodes cleanly must not fall back, and one whose every segment is splittable must fall
// back when the twin raises TRUNCATED, BAD_CODE or BAD_RUN.  Prints a checksum over every status, output and round count.
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_split_host_check.cpp -o jpeg_split_host_check
//   ./jpeg_split_host_check tests/golden/jpeg_decode.json tests/golden/jpeg_split.json
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../baby-vision-curriculum_amd/csrc/jpeg.h"

using namespace bvc::jpg;

static uint32_t rng_state = 97531u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

static uint64_t sum = 1469598103934665603ull;
static void mix(uint64_t v) { sum = (sum ^ v) * 1099511628211ull; }
static long n_parsed = 0, n_decoded = 0, n_flagged = 0, n_fallback = 0, n_split_segments = 0, max_rounds = 0;

static void fail(const char* what, size_t size) {
    fprintf(stderr, "jpeg_split_host_check: %s (an input of %zu bytes)\n", what, size);
    exit(1);
}

static void run(const std::vector<uint8_t>& file) {
    std::vector<uint8_t> data(file.begin(), file.end());      // an exact-size copy on the heap
    bvc_jpeg_info info;
    std::vector<int32_t> seg(4 * 8);
    int rc = parse(data.data(), (int64_t)data.size(), &info, seg.data(), 8);
    ++n_parsed;
    mix((uint64_t)rc);
    if (rc != BVC_OK) return;
    if (info.nseg > 8) {
        seg.assign((size_t)4 * info.nseg, 0);
        if (parse(data.data(), (int64_t)data.size(), &info, seg.data(), info.nseg) != BVC_OK) fail("second parse differs", data.size());
    }
    const int split = 2 * kSplitMinChunk;
    int splittable = 0;
    for (int s = 0; s < info.nseg; ++s) splittable += seg_is_split(seg[4 * s + 1] - seg[4 * s], split);
    n_split_segments += splittable;
    std::vector<uint8_t> want((size_t)3 * info.width * info.height), got(want.size());
    const int st = decode_host(data.data(), &info, seg.data(), want.data());
    ++n_decoded;
    n_flagged += st != 0;
    mix((uint64_t)st);
    for (auto v : want) mix(v);
    const int err = st & (BVC_JPEG_ST_TRUNCATED | BVC_JPEG_ST_BAD_CODE | BVC_JPEG_ST_BAD_RUN);
    for (int chunk : {kSplitMinChunk, 64}) {
        int32_t extra[2];
        if (decode_host_split(data.data(), &info, seg.data(), split, chunk, got.data(), extra) != st) fail("status differs", data.size());
        if (got != want) fail("bytes differ", data.size());
        if (extra[0] < 0 || extra[0] > splittable) fail("more fall-backs than split segments", data.size());
        if (!err && extra[0]) fail("an input the twin decodes cleanly fell back", data.size());
        if (err && splittable == info.nseg && !extra[0]) fail("a damaged input did not fall back", data.size());
        n_fallback += extra[0];
        max_rounds = extra[1] > max_rounds ? extra[1] : max_rounds;
        mix((uint64_t)extra[0]);
        mix((uint64_t)extra[1]);
    }
}

static int b64(int c) {
    if (c >= 'A' && c <= 'Z') return c - 'A';
    if (c >= 'a' && c <= 'z') return c - 'a' + 26;
    if (c >= '0' && c <= '9') return c - '0' + 52;
    return c == '+' ? 62 : (c == '/' ? 63 : -1);
}

static std::vector<std::vector<uint8_t>> load(const char* path) {
    FILE* fh = fopen(path, "rb");
    if (!fh) { fprintf(stderr, "cannot open %s\n", path); exit(1); }
    std::string s;
    char buf[65536];
    size_t k;
    while ((k = fread(buf, 1, sizeof(buf), fh)) > 0) s.append(buf, k);
    fclose(fh);
    std::vector<std::vector<uint8_t>> files;
    const std::string p(path);
    if (p.size() < 5 || p.substr(p.size() - 5) != ".json") {
        files.emplace_back(s.begin(), s.end());
        return files;
    }
    const std::string key = "\"jpeg_b64\": \"";
    for (size_t at = s.find(key); at != std::string::npos; at = s.find(key, at + 1)) {
        std::vector<uint8_t> f;
        uint32_t acc = 0;
        int bits = 0;
        for (size_t i = at + key.size(); i < s.size() && s[i] != '"'; ++i) {
            const int v = b64(s[i]);
            if (v < 0) continue;      // padding
            acc = (acc << 6) | (uint32_t)v;
            bits += 6;
            if (bits >= 8) { bits -= 8; f.push_back((uint8_t)(acc >> bits)); }
        }
        files.push_back(f);
    }
    return files;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: %s fixture.json | file.jpg ...\n", argv[0]); return 2; }
    int nfiles = 0;
    for (int a = 1; a < argc; ++a)
        for (const auto& file : load(argv[a])) {
            ++nfiles;
            run(file);
            for (size_t len = 0; len < file.size(); ++len) run(std::vector<uint8_t>(file.begin(), file.begin() + len));
            {      // each segment cut short
                bvc_jpeg_info info;
                std::vector<int32_t> seg(4 * 4096);
                if (parse(file.data(), (int64_t)file.size(), &info, seg.data(), 4096) == BVC_OK)
                    for (int k = 0; k < info.nseg && k < 4096; ++k) {
                        const int b = seg[4 * k], e = seg[4 * k + 1];
                        std::vector<uint8_t> m(file.begin(), file.begin() + b + (e - b) / 2);
                        m.insert(m.end(), file.begin() + e, file.end());
                        run(m);
                    }
            }
            for (int i = 0; i < 2000 && !file.empty(); ++i) {
                std::vector<uint8_t> m(file);
                m[rnd() % m.size()] = (uint8_t)rnd();
                run(m);
            }
            for (int i = 0; i < 2000 && !file.empty(); ++i) {
                std::vector<uint8_t> m(file);
                m[rnd() % m.size()] ^= (uint8_t)(1u << (rnd() % 8));
                run(m);
            }
        }
    printf("jpeg_split_host_check ok: %d files, %ld inputs parsed, %ld decoded three ways (%ld with a raised status), %ld split segments, "
           "%ld fall-backs, at most %ld rounds, checksum %016llx\n",
           nfiles, n_parsed, n_decoded, n_flagged, n_split_segments, n_fallback, max_rounds, (unsigned long long)sum);
    return 0;
}

// Stand-alone check of the JPEG parser and host twin (csrc/jpeg.h) for a sanitizer build.  The device kernels call the same jpeg.h
// functions for table look-up, bit refill and bounds, so this run is where those bounds are proven before anything runs on a GPU.
// Arguments: fixture files (tests/golden/jpeg_*.json: every "jpeg_b64" string in them) or raw .jpg files.  Each file goes through parse
// + twin as it is, then cut at EVERY length, with each restart segment in turn cut to half its bytes (the rest of the file kept), and
// with 2000 seeded single-byte and 2000 single-bit flips anywhere in headers and scan.
// Whatever parse accepts is decoded into a buffer of exactly 3 * H * W bytes; segment ranges are checked against the file here too.
// Prints a checksum over every status and output.  No GPU, no Python:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/jpeg_host_check.cpp -o jpeg_host_check
//   ./jpeg_host_check tests/golden/jpeg_decode.json tests/golden/jpeg_refuse.json
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../baby-vision-curriculum_amd/csrc/jpeg.h"

static uint32_t rng_state = 97531u;
static uint32_t rnd() { rng_state = rng_state * 1664525u + 1013904223u; return rng_state >> 8; }

static uint64_t sum = 1469598103934665603ull;
static void mix(uint64_t v) { sum = (sum ^ v) * 1099511628211ull; }
static long n_parsed = 0, n_decoded = 0, n_flagged = 0;

static void run(const std::vector<uint8_t>& file) {
    // an exact-size copy on the heap: one byte past either end is the sanitizer's to catch
    std::vector<uint8_t> data(file.begin(), file.end());
    bvc_jpeg_info info;
    std::vector<int32_t> seg(4 * 8);
    int rc = bvc::jpg::parse(data.data(), (int64_t)data.size(), &info, seg.data(), 8);
    ++n_parsed;
    mix((uint64_t)rc);
    if (rc != BVC_OK) return;
    if (info.nseg > 8) {
        seg.assign((size_t)4 * info.nseg, 0);
        if (bvc::jpg::parse(data.data(), (int64_t)data.size(), &info, seg.data(), info.nseg) != BVC_OK) { fprintf(stderr, "second parse differs\n"); exit(1); }
    }
    int next = 0;
    for (int s = 0; s < info.nseg; ++s) {
        const int32_t* g = &seg[4 * s];
        if (g[0] < 0 || g[0] > g[1] || g[1] > (int64_t)data.size() || g[2] != next || g[3] < 1) { fprintf(stderr, "segment %d out of range\n", s); exit(1); }
        next += g[3];
    }
    if (next != info.mcus_x * info.mcus_y) { fprintf(stderr, "segments do not cover the image\n"); exit(1); }
    std::vector<uint8_t> out((size_t)3 * info.width * info.height);
    const int st = bvc::jpg::decode_host(data.data(), &info, seg.data(), out.data());
    ++n_decoded;
    n_flagged += st != 0;
    mix((uint64_t)st);
    for (auto v : out) mix(v);
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
                if (bvc::jpg::parse(file.data(), (int64_t)file.size(), &info, seg.data(), 4096) == BVC_OK)
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
    printf("jpeg_host_check ok: %d files, %ld inputs parsed, %ld decoded (%ld with a raised status), checksum %016llx\n", nfiles, n_parsed,
           n_decoded, n_flagged, (unsigned long long)sum);
    return 0;
}

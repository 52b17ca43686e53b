// The pieces of context.h (host code only - every kernel lives in gemm.hip / attention.hip / rowops.hip).
#include "context.h"

#include <stdio.h>

namespace bvc {

int Shadow::refresh(const float* params, hipStream_t st) {
    const bool vouched = valid;
    valid = false;
    return vouched ? BVC_OK : launch_cast_bf16(params, wbf, (size_t)numel, st);
}

int Shadow::query(int vouch, void** p, int64_t* n) {
    if (p) *p = wbf;
    if (n) *n = numel;
    if (vouch >= 0) valid = vouch != 0;
    return BVC_OK;
}

int alloc_mix(Arena& a, MixState& m, int max_batch) {
    TRY(a.alloc(&m.table, (size_t)max_batch));
    return a.alloc(&m.status, 4);
}

int set_mix(MixState& m, const bvc_clip_mix* mix, int samples, int max_batch, const char* who) {
    m.armed = nullptr;
    if (!mix) return BVC_OK;
    BVC_REQUIRE(samples >= 1 && samples <= max_batch, "%s: %d samples outside [1, %d]", who, samples, max_batch);
    m.armed = mix;
    m.samples = samples;
    return BVC_OK;
}

int alloc_erase(Arena& a, EraseState& e, int max_batch) { return a.alloc(&e.table, (size_t)max_batch * BVC_ERASE_MAX_BOXES); }

int set_erase(EraseState& e, const bvc_erase_box* tab, int samples, int boxes, uint64_t seed, uint64_t offset, int max_batch, const char* who) {
    e.armed = nullptr;
    if (!tab) return BVC_OK;
    BVC_REQUIRE(samples >= 1 && samples <= max_batch, "%s: %d samples outside [1, %d]", who, samples, max_batch);
    BVC_REQUIRE(boxes >= 1 && boxes <= BVC_ERASE_MAX_BOXES, "%s: %d boxes per clip outside [1, %d]", who, boxes, BVC_ERASE_MAX_BOXES);
    e.armed = tab;
    e.samples = samples;
    e.boxes = boxes;
    e.seed = seed;
    e.offset = offset;
    return BVC_OK;
}

// the gather of a forward: the plain kernel, or - consuming an armed table - the mix kernel on the context's copy of it, or - consuming
// an armed erase table, with or without a mix - the erase-then-mix kernel on the context's copies of both
static int gather_for_forward(MixState& m, EraseState* er, bool* mixed, PixelSrc pixels, const int* idx, bf16_t* A, int B, int N, PatchGeom pg,
                              const char* who, hipStream_t st) {
    const bvc_clip_mix* src = m.armed;
    const bvc_erase_box* esrc = er ? er->armed : nullptr;
    m.armed = nullptr;
    if (er) er->armed = nullptr;
    *mixed = src != nullptr || esrc != nullptr;
    if (!src && !esrc) return launch_gather_patches(pixels, idx, A, B, N, pg, st);
    if (src) BVC_REQUIRE(m.samples == B, "%s: the mix was set for %d samples, the call has %d", who, m.samples, B);
    if (esrc) BVC_REQUIRE(er->samples == B, "%s: the erase was set for %d samples, the call has %d", who, er->samples, B);
    if (src) BVC_CHECK_HIP(hipMemcpyAsync(m.table, src, (size_t)B * sizeof(ClipMix), hipMemcpyDeviceToDevice, st));
    BVC_CHECK_HIP(hipMemsetAsync(m.status, 0, 4, st));
    if (!esrc) return launch_gather_patches_mix(pixels, idx, A, B, N, pg, m.table, st, m.status);
    BVC_CHECK_HIP(hipMemcpyAsync(er->table, esrc, (size_t)B * er->boxes * sizeof(EraseBox), hipMemcpyDeviceToDevice, st));
    return launch_gather_patches_aug(pixels, idx, A, B, N, pg, src ? m.table : nullptr, erase_tab(er->table, er->boxes, er->seed, er->offset), st,
                                     m.status);
}

int pixel_src(const char* who, const void* pixels, const bvc_pixel_format* fmt, int channels, PixelSrc* out) {
    PixelSrc px = pixels_f32((const float*)pixels);
    if (fmt && fmt->dtype != BVC_PIXELS_F32) {
        BVC_REQUIRE(fmt->dtype == BVC_PIXELS_U8, "%s: pixel format: dtype %d unknown", who, fmt->dtype);
        BVC_REQUIRE(channels <= 4, "%s: pixel format: uint8 input supports at most 4 channels", who);
        px.is_u8 = 1;
        for (int c = 0; c < 4; ++c) {
            BVC_REQUIRE(fmt->std[c] != 0.f || c >= channels, "%s: pixel format: std[%d] is zero", who, c);
            px.mean[c] = fmt->mean[c];
            px.stdv[c] = c < channels ? fmt->std[c] : 1.f;
        }
    }
    *out = px;
    return BVC_OK;
}

int PatchFront::alloc(Arena& a, PatchGeom geom, size_t max_tokens, bool identity_list) {
    pg = geom;
    L = seq_len(geom);
    Kp = patch_dim(geom);
    TRY(a.alloc(&Ape, max_tokens * Kp));
    if (!identity_list) return BVC_OK;
    TRY(a.alloc(&idx_all, max_tokens));
    TRY(launch_iota_mod(idx_all, (int)max_tokens, L, nullptr));
    BVC_CHECK_HIP(hipStreamSynchronize(nullptr));
    return BVC_OK;
}

int PatchFront::embed(PixelSrc px, const int* idx, int B, int N, const bf16_t* w, const float* bias, const float* pos, float* out, int D,
                      hipStream_t st, const char* who, MixState* mix, bool* mixed, EraseState* erase) {
    if (mix) TRY(gather_for_forward(*mix, erase, mixed, px, idx, Ape, B, N, pg, who, st));
    else TRY(launch_gather_patches(px, idx, Ape, B, N, pg, st));
    const int M = B * N;
    GemmProblem p = gemm(Ape, (size_t)M * Kp, Kp, w, (size_t)D * Kp, Kp, M, D, Kp, EPI_POS, out, D);
    p.bias = bias; p.rowtok = idx; p.pos = pos;
    return launch_gemm(&p, 1, GEMM_NT, -1, st);
}

int PatchFront::embed_backward(Work& w, int M, int D, float* gw, float* gb, hipStream_t st) {
    GemmProblem p = gemm(w.dyb[w.seq % 3], (size_t)M * D, D, Ape, (size_t)M * Kp, Kp, D, Kp, M, EPI_F32, gw, Kp);
    p.rowsum = gb;
    const int tile = plan_dw(&p, 1);
    return launch_gemm(&p, 1, GEMM_TN, tile, st);
}

int stack_forward(Work& w, Stack& s, const std::vector<LayerOff>& off, int B, int N, hipStream_t st, bool chain_ln, const LayerTail* last,
                  const LayerFirst* first) {
    for (int i = 0; i < s.nlayers; ++i) {
        const bool end = i + 1 == s.nlayers;
        TRY(layer_forward(w, s, i, off[i], s.act[i].x_in, end ? s.x_out : s.act[i + 1].x_in, B, N, st, chain_ln && !end ? &off[i + 1] : nullptr,
                          end ? last : nullptr, i == 0 ? first : nullptr));
    }
    return BVC_OK;
}

int stack_backward(Work& w, Stack& s, const std::vector<LayerOff>& off, float* dres, float* G, int B, int N, hipStream_t st,
                   bvc_bucket_fn on_bucket, void* user, const LayerTail* last, const LayerFirst* first) {
    for (int i = s.nlayers - 1; i >= 0; --i)
        TRY(layer_backward(w, s, i, off[i], s.act[i].x_in, dres, G, B, N, st, on_bucket, user, i + 1 == s.nlayers ? last : nullptr, i == 0 ? first : nullptr));
    return BVC_OK;
}

int join_both(Work& w, hipStream_t st, bvc_bucket_fn on_bucket, void* user) {
    TRY(join_side(w, w.seq & 1, st, on_bucket, user));
    return join_side(w, (w.seq + 1) & 1, st, on_bucket, user);
}

int param_info(const ParamTable& t, int index, char* name, int name_cap, int64_t* offset, int64_t* numel, int* ndim, int64_t shape[5]) {
    BVC_REQUIRE(index >= 0 && index < (int)t.entries.size(), "param_info: index %d out of range", index);
    const ParamEntry& e = t.entries[index];
    snprintf(name, name_cap, "%s", e.name.c_str());
    *offset = e.offset; *numel = e.numel; *ndim = e.ndim;
    for (int i = 0; i < 5; ++i) shape[i] = e.shape[i];
    return BVC_OK;
}

int refuse_operand_extent(const char* who, int max_batch, size_t tokens_per_clip, size_t bf16_columns, const char* side_name) {
    const size_t per_clip = tokens_per_clip * bf16_columns * 2, bytes = (size_t)max_batch * per_clip;
    // (a weight-gradient product walks its token rows 64 at a time: the up to 63 rows past the last token must keep their 32-bit byte
    //  offsets below 2^32 as well, or they would wrap into the operand instead of reading as zero - launch_gemm refuses such a product)
    const size_t limit = 0x100000000ull - operand_tail_bytes(bf16_columns);
    if (bytes <= limit) return BVC_OK;
    char side[32] = "";
    if (side_name) snprintf(side, sizeof(side), "the %s's ", side_name);
    set_error("%s: max_batch %d exceeds the 4 GiB operand extent: %s%zu tokens x %zu bf16 columns are %.2f GiB; at most %zu clips", who, max_batch,
              side, (size_t)max_batch * tokens_per_clip, bf16_columns, bytes / 1073741824.0, limit / per_clip);
    return BVC_ERR_INVALID;
}

}  // namespace bvc

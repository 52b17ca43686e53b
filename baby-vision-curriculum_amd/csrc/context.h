// What the model contexts (videomae.hip, jepa.hip) share around the per-layer schedule of stack.h: the bf16 shadow of the parameters,
// the patch-embedding front end with its Mixup / CutMix state, the loops over a stack's layers, and small creation helpers (host code).
#pragma once
#include <functional>

#include "stack.h"

namespace bvc {

// bf16 copy of the leading `numel` flat parameters.  bvc_*_shadow may vouch (valid) that it already matches the parameters the next
// forward will be given - the fused optimisers write it together with them; the vouch holds for ONE forward.
struct Shadow {
    bf16_t* wbf = nullptr;
    int64_t numel = 0;
    bool valid = false;
    int alloc(Arena& a, int64_t n) { numel = n; return a.alloc(&wbf, (size_t)n); }
    int refresh(const float* params, hipStream_t st);     // casts unless vouched; always clears the vouch
    int query(int vouch, void** p, int64_t* n);           // the body of bvc_*_shadow (vouch < 0: leave the vouch as it is)
};

// Mixup / CutMix of a classification context (bvc_*_set_mix)
struct MixState {
    ClipMix* table = nullptr;          // the context's copy, max_batch entries
    int* status = nullptr;             // bit 0: an entry of the last mixed forward was out of range
    const bvc_clip_mix* armed = nullptr;
    int samples = 0;
};
int alloc_mix(Arena& a, MixState& m, int max_batch);
int set_mix(MixState& m, const bvc_clip_mix* mix, int samples, int max_batch, const char* who);

// Random erasing of a classification context (bvc_*_set_erase); its forward reports through the MixState's status word
struct EraseState {
    EraseBox* table = nullptr;         // the context's copy, max_batch * BVC_ERASE_MAX_BOXES entries
    const bvc_erase_box* armed = nullptr;
    int samples = 0, boxes = 0;
    uint64_t seed = 0, offset = 0;
};
int alloc_erase(Arena& a, EraseState& e, int max_batch);
int set_erase(EraseState& e, const bvc_erase_box* tab, int samples, int boxes, uint64_t seed, uint64_t offset, int max_batch, const char* who);

template <typename Config>   // bvc_videomae_config and bvc_vit_config name these fields alike
PatchGeom patch_geom(const Config& c) { return PatchGeom{c.num_frames, c.num_channels, c.image_size, c.image_size, c.tubelet_size, c.patch_size}; }
inline int seq_len(PatchGeom g) { return (g.T / g.ts) * (g.H / g.ps) * (g.W / g.ps); }
inline int patch_dim(PatchGeom g) { return g.C * g.ts * g.ps * g.ps; }
int pixel_src(const char* who, const void* pixels, const bvc_pixel_format* fmt, int channels, PixelSrc* out);

// tube patch embedding as a gather-GEMM over the tokens a call keeps (HF:109-124,164-177; vision_transformer.py:383-391)
struct PatchFront {
    PatchGeom pg;
    int L = 0, Kp = 0;         // tokens per clip, pixels per tube
    int* idx_all = nullptr;    // identity token list [max_tokens] (optional)
    bf16_t* Ape = nullptr;     // bf16 [max_tokens][Kp] gathered tubes
    // with identity_list, idx_all is filled on the null stream and that stream synchronised: a first forward on any stream may read it
    int alloc(Arena& a, PatchGeom geom, size_t max_tokens, bool identity_list);
    // gather (consuming an armed mix and an armed erase, when the context has them) + projection + bias + pos[idx] -> out f32 [B*N][D];
    // *mixed: either was armed, so mix->status is to be checked
    int embed(PixelSrc px, const int* idx, int B, int N, const bf16_t* w, const float* bias, const float* pos, float* out, int D,
              hipStream_t st, const char* who, MixState* mix = nullptr, bool* mixed = nullptr, EraseState* erase = nullptr);
    // weight and bias gradients from the stack's last bf16 copy (pixels need no gradient)
    int embed_backward(Work& w, int M, int D, float* gw, float* gb, hipStream_t st);
};

// every layer of a stack on its own activations.  chain_ln: layer i's fc2 epilogue may produce layer i + 1's first LayerNorm
// (layer_forward's `next`); last: tail mode of the last layer; first: first mode of layer 0
int stack_forward(Work& w, Stack& s, const std::vector<LayerOff>& off, int B, int N, hipStream_t st, bool chain_ln, const LayerTail* last = nullptr,
                  const LayerFirst* first = nullptr);
int stack_backward(Work& w, Stack& s, const std::vector<LayerOff>& off, float* dres, float* G, int B, int N, hipStream_t st,
                   bvc_bucket_fn on_bucket, void* user, const LayerTail* last = nullptr, const LayerFirst* first = nullptr);
// fence the last side-stream launches of a backward (older one first so ranges keep arriving tail-first)
int join_both(Work& w, hipStream_t st, bvc_bucket_fn on_bucket, void* user);

int param_info(const ParamTable& t, int index, char* name, int name_cap, int64_t* offset, int64_t* numel, int* ndim, int64_t shape[5]);

// a *_create body destroys its half-made context on every early return: Making guard{[&] { destroy(c); }}; ... guard.done = true;
struct Making {
    std::function<void()> undo;
    bool done = false;
    ~Making() { if (!done) undo(); }
};
// every bf16 operand travels with a 32-bit byte extent: refuse a max_batch whose widest operand (tokens x columns) reaches 4 GiB
int refuse_operand_extent(const char* who, int max_batch, size_t tokens_per_clip, size_t bf16_columns, const char* side_name);

}  // namespace bvc

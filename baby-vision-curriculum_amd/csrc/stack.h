// Pre-LN transformer stack shared by the VideoMAE encoder/decoder and the JEPA encoder/predictor (host code).
// One layer = LN -> fused qkv Linear -> attention -> proj (+residual) -> LN -> fc1 + GELU -> fc2 (+residual), which is
// VideoMAELayer (HF:339-357) and Block (pretraining/predictive/vision_transformer.py:213-231) alike.
#pragma once
#include <string>
#include <vector>

#include "attention.h"
#include "gemm.h"
#include "rowops.h"

namespace bvc {

#define TRY(expr)                      \
    do {                               \
        int _rc = (expr);              \
        if (_rc != BVC_OK) return _rc; \
    } while (0)

// offsets (elements) of one layer's parameters in a flat f32 buffer; q | k | v weights are one [3d][d] matrix
struct LayerOff {
    int64_t ln1w, ln1b, wqkv, bqkv, wo, bo, ln2w, ln2b, w1, b1, w2, b2, end;
};

struct ParamEntry {
    std::string name;
    int64_t offset, numel;
    int ndim;
    int64_t shape[5];
};

struct ParamTable {
    std::vector<ParamEntry> entries;
    int64_t total = 0;
    int64_t add(const std::string& name, std::initializer_list<int64_t> shp);
};

// saved activations of one transformer layer
struct LayerAct {
    float* x_in;      // f32 [M][D]  layer input (residual stream)
    float* h;         // f32 [M][D]  after attention residual
    bf16_t* ln1o;     // bf16 [M][D]
    bf16_t* qkv;      // bf16 [M][3D]
    bf16_t* ctx;      // bf16 [M][D]
    float* lse;       // f32 [B*H][N]
    bf16_t* ln2o;     // bf16 [M][D]
    bf16_t* pre;      // bf16 [M][I]: gelu'(fc1 pre-activation), written by the forward fc1 epilogue for the backward dX-fc2 product
    bf16_t* act;      // bf16 [M][I]
    float *mean1, *rstd1, *mean2, *rstd2;
};

struct Stack {
    int D, I, H, nlayers;
    float eps;
    std::vector<LayerAct> act;
    float* x_out;     // f32 [M][D] output of the last layer
    // attention width: heads of hd = D / H dims run at hdp = attn_width(hd) dims (hdp == hd unless hd is not 32 / 64 / 80 / 88 / 96 /
    // 128, e.g. 24 -> 32, zero padded); Da = H * hdp is the row width of qkv thirds and of ctx.  Scratch below exists only when hdp != hd.
    int hd, hdp, Da;
    // set by a layer whose fc2 epilogue already produced the NEXT layer's first LayerNorm (ln1o / mean1 / rstd1), cleared by the consumer
    bool ln1_ready = false;
    bf16_t *wqkv_pad = nullptr, *wo_pad = nullptr;             // bf16 [3 Da][D], [D][Da]
    float *bqkv_pad = nullptr;                                 // f32 [3 Da]
    float *gwqkv_pad = nullptr, *gbqkv_pad = nullptr, *gwo_pad = nullptr;   // f32 gradients in the padded layout
};

// device allocations owned by a context
struct Arena {
    std::vector<void*> ptrs;
    template <typename T>
    int alloc(T** p, size_t count) {
        void* q = nullptr;
        BVC_CHECK_HIP(hipMalloc(&q, count * sizeof(T) + 256));
        ptrs.push_back(q);
        *p = reinterpret_cast<T*>(q);
        return BVC_OK;
    }
    void release() {
        for (void* p : ptrs) (void)hipFree(p);
        ptrs.clear();
    }
};

// per-call parameter views + the backward scratch shared by every layer of a context
struct Work {
    const float* params = nullptr;   // f32 flat parameters of the current call
    const bf16_t* wbf = nullptr;     // their bf16 shadow
    // dY operands of the weight-gradient products are multi-buffered so that the grouped dW launch of backward step s may
    // run on the side stream while the main stream works on step s+1 (opt-in, BVC_DW_OVERLAP=1; no gain measured)
    bf16_t *dyb[3] = {}, *dhb[2] = {}, *dqkv[2] = {}, *dh[2] = {};
    bf16_t *dln = nullptr, *dctx = nullptr;
    float *delta = nullptr, *ln_part = nullptr;
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join[2] = {nullptr, nullptr};
    bool overlap = false;
    int seq = 0;
    bool join_pending[2] = {false, false};
    int64_t pend_lo[2], pend_hi[2];
    // Gate on the residual branches (dropgate.h): nullptr / inactive = none, and layer_forward / layer_backward launch what they
    // always launched.  drop_layer >= 0 overrides the layer index the gate is keyed by (a context that reuses one LayerAct).
    const DropState* drop = nullptr;
    int drop_layer = -1;
};

// the head width a stack runs attention at (attention.hip): 80 / 88 in place unless bvc_set_option("head_pad", 1) asks for the
// zero-padded 96 of earlier builds; other widths round up to 32 / 64 / 96 / 128 (zero-padded copies of the qkv / proj weights)
inline int attn_width(int hd) {
    if ((hd == 80 || hd == 88) && !options().head_pad) return hd;
    return hd <= 32 ? 32 : hd <= 64 ? 64 : hd <= 96 ? 96 : 128;
}

// Tail mode of a LAST layer whose consumer reads only the trailing `ndec` rows of every clip's N = nvis + ndec rows (the VideoMAE decoder:
// head, loss and final LayerNorm see the decoded tokens only).  The leading nvis rows are needed as keys and values, so the first
// LayerNorm and the qkv product cover them; behind that nothing reads what the layer would compute for them, and in the backward their
// incoming gradient is exactly zero.  With a LayerTail, layer_forward / layer_backward run the attention queries, proj, LayerNorm 2,
// fc1, fc2 and their input- and weight-gradient products on the B * ndec decoded rows, stored compact.
struct LayerTail { int nvis, ndec; };
// may this stack's last layer run in tail mode for B clips of nvis + ndec rows (options, shapes, gate)?
bool layer_tail_ok(const Work& w, const Stack& s, int B, int nvis, int ndec);

// First mode of a FIRST layer whose trailing `ndec` rows of every clip enter as token + pos[p] (the VideoMAE decoder: mask_token + the
// sinusoid of the row's position p, one of L): such a row's first LayerNorm and qkv row depend on p alone.  With a LayerFirst,
// layer_forward computes them once per position (T1 = LN1(t0), T2 = T1 Wqkv^T + b: L rows), runs LayerNorm 1 and the qkv product of the
// B * nvis visible rows compact, and assembles the full-layout qkv the attention kernels read (and the f32 mask rows of x_in, the residual
// input of proj).  layer_backward sums dqkv over the clips that decode a position (S, f32, clips in ascending order) and derives the mask
// rows' share of dWqkv, dbqkv, LayerNorm 1's dgamma / dbeta and d token from S, T1 and the per-position statistics - LayerNorm's backward
// is linear in its incoming gradient once xhat and rstd are fixed; S and S Wqkv travel as bf16 hi + lo pairs, so the by-position
// products carry no rounding the per-row ones did not.  The visible rows take the unfused path (dX qkv, then the LayerNorm backward
// through a row map; where the stack's LayerNorms run in the epilogues, which hand the backward an unrounded dX, as a pair too).  The mask rows of dres are left as the residual gradient that reaches LayerNorm 1: the caller's column sum over them
// plus what layer_backward adds to `dtoken` is the token's gradient.  Buffers (owned by the caller):
struct LayerFirst {
    int nvis, ndec, L;
    const int* dec_idx;     // [B][ndec] position of every decoded row
    const int* dec_slot;    // [B][L]    slot of position p among clip b's decoded rows, or -1
    const float* t0;        // f32 [2 L][D]  token + pos[p], the L rows twice (the hi and the lo half of a pair meet the same statistics)
    float *tmean, *trstd;   // f32 [2 L]
    bf16_t* ln1c;           // bf16 [B nvis + 2 L][D]    LayerNorm 1 of the visible rows, compact, then T1 twice
    bf16_t* qc;             // bf16 [B nvis + 2 L][3 D]  forward: qkv of the visible rows, then T2; backward: their dqkv, then S hi, S lo
    float *xt, *dt;         // f32 [2 L][D]  S Wqkv (hi rows, lo rows); the LayerNorm backward of the table rows
    bf16_t* dyt;            // bf16 [2 L][D] xt's two halves added, as a pair
    float* part;            // ln_bwd_workspace_floats_upto(2 L, D)
    float* xv;              // f32 [B nvis][D]     dX qkv of the visible rows when the layer's LayerNorms run in the epilogues (f32 there too)
    bf16_t* dyv;            // bf16 [2 B nvis][D]  ... as a pair
    float* dtoken;          // f32 [D] gradient of the token (set for the backward)
};
// may this stack's first layer run in first mode for B clips (options, shapes, the measured gate)?
bool layer_first_ok(const Work& w, const Stack& s, int B, int nvis, int ndec);

LayerOff add_layer_params(ParamTable& t, const std::string& prefix, int64_t d, int64_t inter, bool hf_names);
int alloc_stack(Arena& a, Stack& s, int D, int I, int H, int nlayers, float eps, size_t M, size_t BHN);
// MD = max tokens x width, MI = max tokens x intermediate, over every stack that will use this scratch
int alloc_work(Arena& a, Work& w, size_t MD, size_t MI, size_t delta_elems, size_t lnpart_elems);
void free_work(Work& w);

GemmProblem gemm(const bf16_t* A, size_t a_elems, int lda, const bf16_t* B, size_t b_elems, int ldb, int M, int N, int K,
                 int epi, void* C, int ldc);
int plan_dw(GemmProblem* g, int n);
int join_side(Work& w, int parity, hipStream_t st, bvc_bucket_fn on_bucket, void* user);
void begin_backward(Work& w);
// next: the parameters of layer li + 1 when its activations are s.act[li + 1] (its first LayerNorm may then be produced by this
// layer's fc2 epilogue), nullptr for the last layer or when the caller reuses one set of activations
// tail: see LayerTail (the caller asks layer_tail_ok first and passes the same descriptor to the layer's backward); x_out then holds
// the B * ndec decoded rows only
// first: see LayerFirst (layer 0 only; the caller asks layer_first_ok first and passes the same descriptor to the layer's backward)
int layer_forward(Work& w, Stack& s, int li, const LayerOff& o, const float* x_in, float* x_out, int B, int N, hipStream_t st,
                  const LayerOff* next = nullptr, const LayerTail* tail = nullptr, const LayerFirst* first = nullptr);
// Do the LayerNorms of this stack run inside the epilogues of the 384-wide products next to them (gemm8.hip, EPI_RESID_LN / EPI_DLN)?
bool fuse_row_ln(const Stack& s, int M);
// bvc_*_set_drop: validates the public description and copies path_scale ([nlayers][2][samples], device) into the context's buffer
int set_drop(DropState& d, const bvc_branch_drop* drop, int samples, const char* who, hipStream_t st);
int alloc_drop(Arena& a, DropState& d, int nlayers, int max_samples);
// a forward takes the armed state (one forward and its backward); checks it against the call's row groups
int take_drop(DropState& d, int samples, int rows, const char* who);
// the gate the producer of a stack's first backward bf16 copy applies (the last layer's MLP branch), or nullptr
inline const Gate* top_gate(const DropState& d, Gate& store) {
    if (!d.active) return nullptr;
    store = d.gate(d.nlayers - 1, 1);
    return &store;
}
int layer_backward(Work& w, Stack& s, int li, const LayerOff& o, const float* x_in, float* dres, float* G, int B, int N,
                   hipStream_t st, bvc_bucket_fn on_bucket, void* user, const LayerTail* tail = nullptr, const LayerFirst* first = nullptr);

}  // namespace bvc

// Shared pre-LN transformer stack: allocation, one-layer forward / backward schedules (host code).
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include "stack.h"

namespace bvc {

int64_t ParamTable::add(const std::string& name, std::initializer_list<int64_t> shp) {
    ParamEntry e;
    e.name = name;
    e.offset = total;
    e.numel = 1;
    e.ndim = (int)shp.size();
    int i = 0;
    for (auto s : shp) { e.shape[i++] = s; e.numel *= s; }
    for (; i < 5; ++i) e.shape[i] = 1;
    entries.push_back(e);
    total += e.numel;
    return e.offset;
}

// hf_names: transformers' VideoMAELayer keys (separate query/key/value tensors, adjacent in memory);
// otherwise the JEPA Block keys (norm1, attn.qkv, attn.proj, norm2, mlp.fc1, mlp.fc2)
LayerOff add_layer_params(ParamTable& t, const std::string& p, int64_t d, int64_t inter, bool hf_names) {
    LayerOff o;
    if (hf_names) {
        o.ln1w = t.add(p + "layernorm_before.weight", {d});
        o.ln1b = t.add(p + "layernorm_before.bias", {d});
        o.wqkv = t.add(p + "attention.attention.query.weight", {d, d});
        t.add(p + "attention.attention.key.weight", {d, d});
        t.add(p + "attention.attention.value.weight", {d, d});
        o.bqkv = t.add(p + "attention.attention.query.bias", {d});
        t.add(p + "attention.attention.key.bias", {d});
        t.add(p + "attention.attention.value.bias", {d});
        o.wo = t.add(p + "attention.output.dense.weight", {d, d});
        o.bo = t.add(p + "attention.output.dense.bias", {d});
        o.ln2w = t.add(p + "layernorm_after.weight", {d});
        o.ln2b = t.add(p + "layernorm_after.bias", {d});
        o.w1 = t.add(p + "intermediate.dense.weight", {inter, d});
        o.b1 = t.add(p + "intermediate.dense.bias", {inter});
        o.w2 = t.add(p + "output.dense.weight", {d, inter});
        o.b2 = t.add(p + "output.dense.bias", {d});
    } else {
        o.ln1w = t.add(p + "norm1.weight", {d});
        o.ln1b = t.add(p + "norm1.bias", {d});
        o.wqkv = t.add(p + "attn.qkv.weight", {3 * d, d});
        o.bqkv = t.add(p + "attn.qkv.bias", {3 * d});
        o.wo = t.add(p + "attn.proj.weight", {d, d});
        o.bo = t.add(p + "attn.proj.bias", {d});
        o.ln2w = t.add(p + "norm2.weight", {d});
        o.ln2b = t.add(p + "norm2.bias", {d});
        o.w1 = t.add(p + "mlp.fc1.weight", {inter, d});
        o.b1 = t.add(p + "mlp.fc1.bias", {inter});
        o.w2 = t.add(p + "mlp.fc2.weight", {d, inter});
        o.b2 = t.add(p + "mlp.fc2.bias", {d});
    }
    o.end = t.total;
    return o;
}

int alloc_stack(Arena& a, Stack& s, int D, int I, int H, int nlayers, float eps, size_t M, size_t BHN) {
    s.D = D; s.I = I; s.H = H; s.nlayers = nlayers; s.eps = eps;
    s.hd = D / H;
    s.hdp = attn_width(s.hd);
    BVC_REQUIRE(D % H == 0 && s.hd <= 128 && s.hd % 8 == 0, "stack: head_dim %d unsupported (multiples of 8 up to 128)", s.hd);
    s.Da = H * s.hdp;
    const size_t Da = s.Da;
    // operand extents travel as 32-bit byte counts (bvc_gemm_desc.a_bytes / b_bytes, buffer descriptors): the widest bf16
    // activation of a layer has to stay below 4 GiB (VideoMAE-base decoder: ~890 clips per GPU; from 2 GiB on - 445 clips - the
    // 256-row persistent kernel, which marks dropped loads with offset bit 31, hands the product to the 128 x 128 kernels)
    // (... and the last 64-row step of a weight gradient over fewer tokens than M must not wrap either: gemm.h tn_tail_ok)
    BVC_REQUIRE(M * std::max<size_t>(3 * Da, (size_t)I) * 2 + operand_tail_bytes(std::max<size_t>(3 * Da, (size_t)I)) <= 0x100000000ull,
                "stack: %zu tokens x %zu columns of bf16 exceed the 4 GiB operand extent; use a smaller per-GPU batch", M, std::max<size_t>(3 * Da, (size_t)I));
    if (s.hdp != s.hd) {
        TRY(a.alloc(&s.wqkv_pad, 3 * Da * D));
        TRY(a.alloc(&s.wo_pad, (size_t)D * Da));
        TRY(a.alloc(&s.bqkv_pad, 3 * Da));
        TRY(a.alloc(&s.gwqkv_pad, 3 * Da * D));
        TRY(a.alloc(&s.gbqkv_pad, 3 * Da));
        TRY(a.alloc(&s.gwo_pad, (size_t)D * Da));
    }
    s.act.resize(nlayers);
    for (auto& l : s.act) {
        TRY(a.alloc(&l.x_in, M * D));
        TRY(a.alloc(&l.h, M * D));
        TRY(a.alloc(&l.ln1o, M * D));
        TRY(a.alloc(&l.qkv, M * 3 * Da));
        TRY(a.alloc(&l.ctx, M * Da));
        TRY(a.alloc(&l.lse, BHN));
        TRY(a.alloc(&l.ln2o, M * D));
        TRY(a.alloc(&l.pre, M * I));
        TRY(a.alloc(&l.act, M * I));
        TRY(a.alloc(&l.mean1, M));
        TRY(a.alloc(&l.rstd1, M));
        TRY(a.alloc(&l.mean2, M));
        TRY(a.alloc(&l.rstd2, M));
    }
    TRY(a.alloc(&s.x_out, M * D));
    return BVC_OK;
}

int alloc_work(Arena& a, Work& w, size_t MD, size_t MI, size_t delta_elems, size_t lnpart_elems) {
    for (int i = 0; i < 3; ++i) TRY(a.alloc(&w.dyb[i], MD));
    for (int i = 0; i < 2; ++i) {
        TRY(a.alloc(&w.dhb[i], MD));
        TRY(a.alloc(&w.dqkv[i], 3 * MD));
        TRY(a.alloc(&w.dh[i], MI));
    }
    TRY(a.alloc(&w.dln, MD));
    TRY(a.alloc(&w.dctx, MD));
    TRY(a.alloc(&w.delta, delta_elems));
    TRY(a.alloc(&w.ln_part, std::max(lnpart_elems, kRowLnPartFloats)));      // (also the per-workgroup partial rows of the fused LayerNorm backward)
    // Measured on MI355X (B=16): running the grouped dW launch on a side stream next to the dX chain gains nothing
    // (1398 vs 1419 clips/s) - each GEMM already holds all of a CU's LDS - so it is opt-in for experiments.
    w.overlap = false;      // bvc_set_option("dw_overlap", 1), read at every begin_backward
    BVC_CHECK_HIP(hipStreamCreateWithFlags(&w.side, hipStreamNonBlocking));
    BVC_CHECK_HIP(hipEventCreateWithFlags(&w.ev_fork, hipEventDisableTiming));
    BVC_CHECK_HIP(hipEventCreateWithFlags(&w.ev_join[0], hipEventDisableTiming));
    BVC_CHECK_HIP(hipEventCreateWithFlags(&w.ev_join[1], hipEventDisableTiming));
    return BVC_OK;
}

void free_work(Work& w) {
    if (w.side) { (void)hipStreamSynchronize(w.side); (void)hipStreamDestroy(w.side); w.side = nullptr; }
    if (w.ev_fork) { (void)hipEventDestroy(w.ev_fork); w.ev_fork = nullptr; }
    for (int i = 0; i < 2; ++i) if (w.ev_join[i]) { (void)hipEventDestroy(w.ev_join[i]); w.ev_join[i] = nullptr; }
}

void begin_backward(Work& w) {
    w.overlap = options().dw_overlap != 0;
    w.seq = 0;
    w.join_pending[0] = w.join_pending[1] = false;
}

GemmProblem gemm(const bf16_t* A, size_t a_elems, int lda, const bf16_t* B, size_t b_elems, int ldb, int M, int N, int K,
                 int epi, void* C, int ldc) {
    GemmProblem p;
    memset(&p, 0, sizeof(p));
    p.A = A; p.B = B; p.M = M; p.N = N; p.K = K; p.lda = lda; p.ldb = ldb;
    p.a_bytes = (uint32_t)(a_elems * 2); p.b_bytes = (uint32_t)(b_elems * 2);
    p.alpha = 1.f; p.epi = epi; p.split_k = 1; p.C = C; p.ldc = ldc;
    return p;
}

// Tile and split-K choice for a group of weight-gradient products (contraction over all tokens).
// Measured (profiles/r01_b_microbench.json): when the 128x128 tiles alone cover the chip (encoder layer: 432)
// use them unsplit; otherwise 64x64 tiles with just enough K-splits for ~850 workgroups (decoder layer: 432 x 2).
int plan_dw(GemmProblem* g, int n) {
    // Largest tile that still gives about one full wave of blocks (256 CUs x 2 resident) once K is split; the split is capped
    // at 12 (each split adds one f32 atomic pass over the output) and at 8 K-steps per block.  Fitted to the same-box sweep
    // in profiles/r01_d_dw_sweep.txt (tools/ab/dw_sweep.py): dec layer group 128x128 split 4 = 125 us vs 64x64 split 2 = 155 us.
    static const int bm[3] = {128, 128, 64}, bn[3] = {128, 64, 64};
    int ksteps = 1 << 30;
    for (int i = 0; i < n; ++i) ksteps = std::min(ksteps, (g[i].K + 63) / 64);
    // The 256-row persistent kernel (gemm8.hip; tile config 10 = 256 x 256, 11 = 256 x 128): one workgroup per CU walks its units
    // (tile x K split) as one stream of K tiles, so the split is chosen for ~230 units on the 256 CUs, at least 16 K tiles each.
    // Same-process A/B at 64 clips (profiles/r02_e_gemm8_ab_b64.txt): encoder layer 256 x 256 split 2 (216 units) 181 us vs
    // 256 x 128 unsplit 218 us vs the 128 x 128 kernel 220 us; decoder layer 256 x 256 split 6 (228 units) 549 us vs 626 us.
    const int g8 = options().gemm8;
    if (g8 >= 0) {
        bool ok = true, by384 = true;
        double flops = 0.0, outs = 0.0;
        int units256 = 0, units384 = 0;
        for (int i = 0; i < n; ++i) {
            ok = ok && g[i].epi == EPI_F32 && g[i].a_bytes < 0x80000000u && g[i].b_bytes < 0x80000000u;
            by384 = by384 && g[i].N % 384 == 0 && g[i].M % 128 == 0;
            flops += 2.0 * g[i].M * g[i].N * g[i].K;
            outs += (double)g[i].M * g[i].N;
            units256 += ((g[i].M + 255) / 256) * ((g[i].N + 255) / 256);
            units384 += ((g[i].M + 127) / 128) * ((g[i].N + 383) / 384);
        }
        // Widths that are multiples of 384 but not of 256 (decoder, JEPA predictor: 384 / 1152 / 1536) leave 256 x 256 tiles partly
        // empty - the four weight gradients of a VideoMAE decoder layer fill 71 % of 38 such tiles and 100 % of 36 tiles of 128 x 384
        // (tile config 12).  Taken when the 256-wide tiling would execute >= 1.2x the MFMA work of the outputs.  K split: the fewest
        // splits that give every CU one unit (units x split as close below a multiple of 256 as it gets), at least 16 K tiles each.
        // (same-process A/B, profiles/r03_b_dw_tile12_ab_b{16,64,256}.txt: decoder layer group 1522 vs 2312 us at 256 clips, 383 vs
        //  558 at 64, 125 vs 139 (the 128 x 128 kernel) at 16 - it needs a shorter stream than the 256 x 256 tile to pay off)
        const bool long_enough = g8 > 0 ? ksteps >= 2 : (ksteps >= 16 && flops >= 80e9);
        if (ok && by384 && long_enough && units256 * 65536.0 >= 1.2 * outs) {
            // (up to 24 splits since round 4: the head's 12 tiles x 21 = 252 units, 498 vs 564 us with 16 splits at 256 clips -
            //  profiles/r04_o_head_dw_splits.txt; an atomic pass over its 2.4 MB of outputs per split is noise)
            const int smax = std::max(1, std::min(24, ksteps / (g8 > 0 ? 2 : 16)));
            // Members whose K ranges differ by 2 x and more (first mode: the qkv member contracts over the visible rows and the
            // position tables, a ninth of the others' rows at the benchmark's shape) get splits of their own: every unit about
            // as long as the longest member's, so that the short member's tiles do not hold a CU for a fraction of the launch
            // while the split is chosen for them.  s_i = ceil(K tiles_i / unit length); the unit length is the longest member's
            // K tiles over sp, sp chosen by the same cost as below.  The walk and the deterministic reduce take splits per problem.
            int kmax = 0;
            for (int i = 0; i < n; ++i) kmax = std::max(kmax, (g[i].K + 63) / 64);
            if (kmax >= 2 * ksteps) {
                const int per_min = g8 > 0 ? 2 : 16;
                int best_sp = 0;
                double best_cost = 1e300;
                for (int sp = 1; sp <= std::max(1, std::min(24, kmax / per_min)); ++sp) {
                    const int len = (kmax + sp - 1) / sp;
                    int units = 0, longest = 0;
                    for (int i = 0; i < n; ++i) {
                        const int kt = (g[i].K + 63) / 64;
                        const int si = std::max(1, std::min((kt + len - 1) / len, std::max(1, kt / per_min)));
                        units += ((g[i].M + 127) / 128) * ((g[i].N + 383) / 384) * si;
                        longest = std::max(longest, (kt + si - 1) / si);
                    }
                    const int rounds = (units + 255) / 256;
                    const double cost = (double)rounds * longest + 4.0 * rounds;
                    if (cost < best_cost * 0.999) { best_cost = cost; best_sp = sp; }
                }
                const int len = (kmax + best_sp - 1) / best_sp;
                int units = 0;
                for (int i = 0; i < n; ++i) {
                    const int kt = (g[i].K + 63) / 64;
                    g[i].split_k = std::max(1, std::min((kt + len - 1) / len, std::max(1, kt / per_min)));
                    units += ((g[i].M + 127) / 128) * ((g[i].N + 383) / 384) * g[i].split_k;
                }
                if (units >= (g8 > 0 ? 1 : 160)) return 12;
            }
            int best = 1;
            double best_cost = 1e300;
            for (int sp = 1; sp <= smax; ++sp) {
                const int rounds = (units384 * sp + 255) / 256;
                const double cost = (double)rounds * ((ksteps + sp - 1) / sp) + 4.0 * rounds;     // K tiles on the critical path + an epilogue per round
                if (cost < best_cost * 0.999) { best_cost = cost; best = sp; }
            }
            if (units384 * best >= (g8 > 0 ? 1 : 160)) {
                for (int i = 0; i < n; ++i) g[i].split_k = best;
                return 12;
            }
        }
        if (ok && g8 > 0 && ksteps >= 2) {          // forced (tests, A/B tools): 256 x 256 tiles, K split for ~230 units as below
            const int split = std::max(1, std::min((232 + units256 / 2) / units256, ksteps / 2));
            for (int i = 0; i < n; ++i) g[i].split_k = split;
            return 10;
        }
        // short launches stay on the 128 x 128 kernel (at 16 clips: encoder layer 53 vs 85 us, decoder layer 139 vs 151 us,
        // profiles/r02_e_gemm8_ab_b16.txt): one workgroup per CU needs a long stream to amortise its prologue and tail
        if (ok && ksteps >= 16 && flops >= 140e9) {
            for (int t = 0; t < 2; ++t) {            // prefer the bigger tile when it still fills the chip
                const int bnw = t == 0 ? 256 : 128;
                int units = 0;
                for (int i = 0; i < n; ++i) units += ((g[i].M + 255) / 256) * ((g[i].N + bnw - 1) / bnw);
                int split = std::max(1, (232 + units / 2) / units);
                split = std::min(split, std::max(1, ksteps / 16));
                if (units >= 16 && units * split >= (t == 0 ? 200 : 160) && units * split <= 272) {
                    for (int i = 0; i < n; ++i) g[i].split_k = split;
                    return t == 0 ? 10 : 11;
                }
            }
            // 256 x 256 tiles that fill half to 15/16 of the chip unsplit and overflow it when split (ViT-L layers: 192 tiles): tile
            // config 13 - the outputs are accumulated by f32 atomics (every caller of plan_dw zeroes the gradient buffer first, as for a
            // K split), which lets gemm8's balanced walk hand the tails of the K ranges to the idle CUs (launch_gemm, plan_balance)
            if (units256 >= 128 && units256 <= 240 && ksteps >= 64) {
                for (int i = 0; i < n; ++i) g[i].split_k = 1;
                return 13;
            }
        }
    }
    const int cap = std::max(1, std::min(12, ksteps / 8));
    int tile = 2, split = 1;
    for (int t = 0; t < 3; ++t) {
        int tiles = 0;
        for (int i = 0; i < n; ++i) tiles += ((g[i].M + bm[t] - 1) / bm[t]) * ((g[i].N + bn[t] - 1) / bn[t]);
        const int s = std::max(1, std::min(cap, (480 + tiles / 2) / tiles));
        tile = t; split = s;
        if (tiles * s >= 400) break;
    }
    for (int i = 0; i < n; ++i) g[i].split_k = split;
    return tile;
}

// A 128 x 384 tile of gemm8.hip holds complete rows of a 384-wide Linear output, so the LayerNorm that follows proj / fc2 (forward) or
// precedes fc1 / qkv (backward: their dX products) runs in that product's epilogue instead of as an HBM pass of its own.  Measured at 256
// clips (profiles/r05_e_rowln_products_stagger_b256.txt): proj + LN 416 vs 330 + 173 us, fc2 + LN 693 vs 684 + 172, dX fc1 + LN bwd 866
// vs 562 + 472, dX qkv + LN bwd 749 vs 433 + 473; whole step -0.5 % at 16 clips ... -2.2 % at 256 (r05_h_rowln_ab_batches.txt).  Below
// 128 units (JEPA predictor at small batches) the separate passes stay.  bvc_set_option("row_ln", 1 / -1) forces either way; a forced gemm8 forces it too.
bool fuse_row_ln(const Stack& s, int M) {
    const int mode = options().row_ln;
    if (mode < 0 || options().gemm8 < 0) return false;
    if (!gemm_row_ln_ok(M, s.D, s.D) || s.I % 64 != 0 || (3 * s.Da) % 64 != 0) return false;
    if ((size_t)M * std::max<size_t>(3 * (size_t)s.Da, (size_t)s.I) * 2 >= 0x80000000ull) return false;    // gemm8 addresses operands below 2 GiB
    if (mode > 0 || options().gemm8 > 0) return true;
    return M >= 128 * 128;     // (16 clips of 1568 tokens = 196 units: -0.5 %; 32: -1.3 %; 64: -1.3 %; 128: -2.0 %; 256: -2.2 % of the step)
}

// Tail mode (stack.h LayerTail): on by default, bvc_set_option("dec_tail", 0) switches it off.  It needs the row-LayerNorm epilogues (their
// segment map carries the one full-layout side array of proj and of dX fc1), decoded rows in whole 128-row units per clip (a unit then
// never straddles a clip), no gate on the branches, and heads the attention kernels have a query window for, in place (no padded copies).
bool layer_tail_ok(const Work& w, const Stack& s, int B, int nvis, int ndec) {
    if (!options().dec_tail || nvis < 1 || ndec < 128 || ndec % 128 != 0) return false;
    if (w.drop != nullptr && w.drop->active) return false;
    if (s.hdp != s.hd || !attn_window_ok(s.hd)) return false;
    if (nvis + ndec <= 160) return false;      // the whole-head attention backward's range: the window form (two kernels) was not measured against it
    return fuse_row_ln(s, B * (nvis + ndec)) && gemm_row_ln_ok(B * ndec, s.D, s.D);
}

// First mode (stack.h LayerFirst): bvc_set_option("dec_first", 1 / 0 / -1) = on whenever the shapes allow / off / the measured gate.  A
// stack of one layer keeps it off (that layer may be the tail layer), and so do padded heads (the padded qkv copies are not wired
// through the by-position products) and a gate on the branches.
// Same-process A/B of the base step, forward + backward (profiles/dec_first_bench_parent_ab.txt): 256 clips -0.88 / -0.98 ms of 76.9, 64 clips
// -0.17 / -0.18 of 22.3, 16 clips +0.03 / +0.04 of 7.7 - the by-position launches cost more than they save there.  Between 16 and 64: not measured.
constexpr int kFirstAutoClips = 64;
bool layer_first_ok(const Work& w, const Stack& s, int B, int nvis, int ndec) {
    const int mode = options().dec_first;
    if (mode == 0 || s.nlayers < 2 || nvis < 1 || ndec < 1 || B < 1) return false;
    if (w.drop != nullptr && w.drop->active) return false;
    if (s.hdp != s.hd || s.D % 8 != 0) return false;
    if (mode > 0) return true;
    return B >= kFirstAutoClips;
}

int alloc_drop(Arena& a, DropState& d, int nlayers, int max_samples) {
    d.nlayers = nlayers;
    d.max_samples = max_samples;
    return a.alloc(&d.path_scale, (size_t)nlayers * 2 * max_samples);
}

int set_drop(DropState& d, const bvc_branch_drop* drop, int samples, const char* who, hipStream_t st) {
    d.armed = false;
    if (!drop || (drop->hidden_p == 0.f && drop->path_scale == nullptr)) return BVC_OK;      // off
    BVC_REQUIRE(drop->hidden_p >= 0.f && drop->hidden_p < 1.f, "%s: hidden_p %g outside [0, 1)", who, (double)drop->hidden_p);
    BVC_REQUIRE(samples >= 1 && samples <= d.max_samples, "%s: %d samples outside [1, %d]", who, samples, d.max_samples);
    BVC_REQUIRE(drop->rows_per_sample >= 1, "%s: rows_per_sample must be >= 1", who);
    d.hidden_p = drop->hidden_p;
    d.seed = drop->seed;
    d.offset = drop->offset;
    d.samples = samples;
    d.rows = drop->rows_per_sample;
    d.has_path = drop->path_scale != nullptr;
    if (d.has_path)
        BVC_CHECK_HIP(hipMemcpyAsync(d.path_scale, drop->path_scale, (size_t)d.nlayers * 2 * samples * sizeof(float), hipMemcpyDeviceToDevice, st));
    d.armed = true;
    return BVC_OK;
}

int take_drop(DropState& d, int samples, int rows, const char* who) {
    d.active = d.armed;
    d.armed = false;
    if (!d.active) return BVC_OK;
    if (d.samples != samples || d.rows != rows) {
        d.active = false;
        set_error("%s: the gate was set for %d samples of %d rows, the call has %d of %d", who, d.samples, d.rows, samples, rows);
        return BVC_ERR_INVALID;
    }
    return BVC_OK;
}

int layer_forward(Work& w, Stack& s, int li, const LayerOff& o, const float* x_in, float* x_out, int B, int N, hipStream_t st,
                  const LayerOff* next, const LayerTail* tail, const LayerFirst* first) {
    LayerAct& a = s.act[li];
    const int D = s.D, I = s.I, M = B * N;
    // tail mode: everything behind the qkv product runs on the Mq = B * ndec decoded rows, stored compact (ctx, lse, h, ln2o, mean2, rstd2,
    // pre, act and x_out hold Mq rows); only the residual input of proj is read in the full layout, through the epilogue's segment map
    const int Mq = tail ? B * tail->ndec : M;
    if (tail) BVC_REQUIRE(next == nullptr && tail->nvis + tail->ndec == N && layer_tail_ok(w, s, B, tail->nvis, tail->ndec), "layer_forward: tail mode is not available for this layer");
    const float* P = w.params;
    const bf16_t* W = w.wbf;
    const float eps = s.eps;
    // a gate on the branches: both branch products take the gated epilogue of the 128 x 128 kernel, the LayerNorms run as separate passes
    const bool gated = w.drop != nullptr && w.drop->active;
    const int gl = w.drop_layer >= 0 ? w.drop_layer : li;
    const bool fuse = !gated && fuse_row_ln(s, M);
    if (li == 0) s.ln1_ready = false;
    if (first) BVC_REQUIRE(li == 0 && !tail && x_in == a.x_in && first->nvis + first->ndec == N && layer_first_ok(w, s, B, first->nvis, first->ndec),
                           "layer_forward: first mode is not available for this layer");
    // (the previous layer's fc2 epilogue may have left this layer's first LayerNorm behind)
    if (first) {
        // LayerNorm 1 of the table rows (twice: stack.h) and of the visible rows, one qkv product over [visible | T1] -> [qkv | T2]
        const int Mv = B * first->nvis;
        TRY(launch_ln_fwd(first->t0, identity_rows(), P + o.ln1w, P + o.ln1b, first->ln1c + (size_t)Mv * D, first->tmean, first->trstd, 2 * first->L, D, eps, st));
        TRY(launch_ln_fwd(x_in, RowMap{first->nvis, N, 0}, P + o.ln1w, P + o.ln1b, first->ln1c, a.mean1, a.rstd1, Mv, D, eps, st));
    } else if (!(fuse && s.ln1_ready)) TRY(launch_ln_fwd(x_in, identity_rows(), P + o.ln1w, P + o.ln1b, a.ln1o, a.mean1, a.rstd1, M, D, eps, st));
    s.ln1_ready = false;
    const int Da = s.Da;
    const bool pad = s.hdp != s.hd;
    const bf16_t *Wqkv = W + o.wqkv, *Wo = W + o.wo;
    const float* bqkv = P + o.bqkv;
    const float sm_scale = pad ? 1.0f / sqrtf((float)s.hd) : 0.f;
    if (pad) {
        TRY(launch_pad_heads(W + o.wqkv, P + o.bqkv, W + o.wo, s.wqkv_pad, s.bqkv_pad, s.wo_pad, D, s.H, s.hd, s.hdp, st));
        Wqkv = s.wqkv_pad; Wo = s.wo_pad; bqkv = s.bqkv_pad;
    }
    if (first) {
        const int Mf = B * first->nvis + first->L;
        GemmProblem p = gemm(first->ln1c, (size_t)Mf * D, D, Wqkv, (size_t)3 * Da * D, D, Mf, 3 * Da, D, EPI_BF16, first->qc, 3 * Da);
        p.bias = bqkv;
        TRY(launch_gemm(&p, 1, GEMM_NT, -1, st));
        TRY(launch_first_assemble(first->qc, first->qc + (size_t)B * first->nvis * 3 * Da, first->t0, first->dec_idx, a.qkv, a.x_in, B, first->nvis,
                                  first->ndec, 3 * Da, D, st));
    } else {
        GemmProblem p = gemm(a.ln1o, (size_t)M * D, D, Wqkv, (size_t)3 * Da * D, D, M, 3 * Da, D, EPI_BF16, a.qkv, 3 * Da);
        p.bias = bqkv;
        TRY(launch_gemm(&p, 1, GEMM_NT, -1, st));
    }
    if (tail) TRY(launch_attn_fwd_win(a.qkv, a.ctx, a.lse, B, N, s.H, s.hdp, tail->nvis, tail->ndec, st, sm_scale));
    else TRY(launch_attn_fwd(a.qkv, a.ctx, a.lse, B, N, s.H, s.hdp, st, sm_scale));
    {
        GemmProblem p = gemm(a.ctx, (size_t)Mq * Da, Da, Wo, (size_t)D * Da, Da, Mq, D, Da, fuse ? EPI_RESID_LN : EPI_RESID, a.h, D);
        p.bias = P + o.bo; p.resid = x_in;
        if (fuse) { p.C2 = a.ln2o; p.ln_gamma = P + o.ln2w; p.ln_beta = P + o.ln2b; p.ln_mean = a.mean2; p.ln_rstd = a.rstd2; p.ln_eps = eps; }
        if (tail) { p.seg_rows = tail->ndec; p.seg_stride = N; p.seg_off = tail->nvis; }
        if (gated) TRY(launch_gemm_gate(p, w.drop->gate(gl, 0), -1, st));
        else TRY(launch_gemm(&p, 1, GEMM_NT, -1, st));
    }
    if (!fuse) TRY(launch_ln_fwd(a.h, identity_rows(), P + o.ln2w, P + o.ln2b, a.ln2o, a.mean2, a.rstd2, M, D, eps, st));
    {
        GemmProblem p = gemm(a.ln2o, (size_t)Mq * D, D, W + o.w1, (size_t)I * D, D, Mq, I, D, EPI_GELU, a.pre, I);
        p.bias = P + o.b1; p.C2 = a.act;
        TRY(launch_gemm(&p, 1, GEMM_NT, -1, st));
    }
    {
        const bool fuse_next = fuse && next != nullptr && li + 1 < (int)s.act.size();
        GemmProblem p = gemm(a.act, (size_t)Mq * I, I, W + o.w2, (size_t)D * I, I, Mq, D, I, fuse_next ? EPI_RESID_LN : EPI_RESID, x_out, D);
        p.bias = P + o.b2; p.resid = a.h;
        if (fuse_next) {      // the next layer's first LayerNorm, out of this epilogue's complete rows
            LayerAct& an = s.act[li + 1];
            p.C2 = an.ln1o; p.ln_gamma = P + next->ln1w; p.ln_beta = P + next->ln1b; p.ln_mean = an.mean1; p.ln_rstd = an.rstd1; p.ln_eps = eps;
        }
        if (gated) TRY(launch_gemm_gate(p, w.drop->gate(gl, 1), -1, st));
        else TRY(launch_gemm(&p, 1, GEMM_NT, -1, st));
        s.ln1_ready = fuse_next;
    }
    return BVC_OK;
}

// Fence a side-stream weight-gradient launch into the main stream and report its gradient range.
int join_side(Work& c_, int parity, hipStream_t st, bvc_bucket_fn on_bucket, void* user) {
    if (!c_.join_pending[parity]) return BVC_OK;
    BVC_CHECK_HIP(hipStreamWaitEvent(st, c_.ev_join[parity], 0));
    c_.join_pending[parity] = false;
    if (on_bucket) on_bucket(c_.pend_lo[parity], c_.pend_hi[parity] - c_.pend_lo[parity], user);
    return BVC_OK;
}

// dres (f32 [M][D]) holds d/d(layer output) on entry and d/d(layer input) on exit; dyb[seq % 3] is its bf16 copy.
// The four weight gradients (+ bias gradients) of the layer are one grouped launch on the side stream, overlapping the
// next layer's dX chain; its gradient range [o.ln1w, o.end) is reported when that launch has been fenced (two steps later).
// Tail mode (the layer's forward ran with the same LayerTail): dyb, dh, dhb and dctx hold the Mq decoded rows, compact; dres keeps the full
// layout - the dX fc1 epilogue adds into its decoded rows through the segment map, the visible rows (zero on entry: the head sends them no
// gradient) reach the dX qkv product untouched.
int layer_backward(Work& c_, Stack& s, int li, const LayerOff& o, const float* x_in, float* dres, float* G, int B, int N,
                   hipStream_t st, bvc_bucket_fn on_bucket, void* user, const LayerTail* tail, const LayerFirst* first) {
    LayerAct& a = s.act[li];
    const int D = s.D, I = s.I, M = B * N;
    const int Mq = tail ? B * tail->ndec : M;
    const float* P = c_.params;
    const bf16_t* W = c_.wbf;
    const int q = c_.seq, par = q & 1;
    bf16_t* dyb = c_.dyb[q % 3];
    bf16_t* dyb_next = c_.dyb[(q + 1) % 3];
    bf16_t *dh = c_.dh[par], *dhb = c_.dhb[par], *dqkv = c_.dqkv[par];
    // the buffers of this parity were last read by the side launch of step q-2
    TRY(join_side(c_, par, st, on_bucket, user));
    // MLP
    {
        GemmProblem p = gemm(dyb, (size_t)Mq * D, D, W + o.w2, (size_t)D * I, I, Mq, I, D, EPI_DGELU, dh, I);
        p.aux = a.pre; p.ldaux = I;
        TRY(launch_gemm(&p, 1, GEMM_NN, -1, st));
    }
    // Gated branches (dropgate.h): dres passes ungated; the bf16 copies that feed a branch are gated where they are produced - dhb by this
    // layer's attention gate, the next step's dyb by the MLP gate of the layer below (the copy after layer 0 feeds the patch
    // embedding: ungated).  The weight and bias gradients then need no change.
    const bool gated = c_.drop != nullptr && c_.drop->active;
    Gate g_attn, g_below;
    if (gated) { g_attn = c_.drop->gate(li, 0); if (li > 0) g_below = c_.drop->gate(li - 1, 1); }
    const bool fuse = !gated && fuse_row_ln(s, M);
    if (tail) BVC_REQUIRE(fuse && tail->nvis + tail->ndec == N, "layer_backward: tail mode needs the row-LayerNorm epilogues");
    if (fuse) {      // dX of fc1 with the second LayerNorm's backward in its epilogue: dres += ..., dhb = bf16(dres), dgamma / dbeta
        GemmProblem p = gemm(dh, (size_t)Mq * I, I, W + o.w1, (size_t)I * D, D, Mq, D, I, EPI_DLN, dres, D);
        p.C2 = dhb; p.ln_x = a.h; p.ln_mean = a.mean2; p.ln_rstd = a.rstd2; p.ln_gamma = P + o.ln2w;
        p.ln_part = c_.ln_part; p.ln_dgamma = G + o.ln2w; p.ln_dbeta = G + o.ln2b;
        if (tail) { p.seg_rows = tail->ndec; p.seg_stride = N; p.seg_off = tail->nvis; }
        TRY(launch_gemm(&p, 1, GEMM_NN, -1, st));
    } else {
        GemmProblem p = gemm(dh, (size_t)M * I, I, W + o.w1, (size_t)I * D, D, M, D, I, EPI_BF16, c_.dln, D);
        TRY(launch_gemm(&p, 1, GEMM_NN, -1, st));
        TRY(launch_ln_bwd(c_.dln, a.h, identity_rows(), a.mean2, a.rstd2, P + o.ln2w, dres, 1, dhb, G + o.ln2w, G + o.ln2b, c_.ln_part, M, D, st,
                          gated ? &g_attn : nullptr));
    }
    // attention
    const int Da = s.Da;
    const bool pad = s.hdp != s.hd;
    const bf16_t *Wqkv = W + o.wqkv, *Wo = W + o.wo;
    const float sm_scale = pad ? 1.0f / sqrtf((float)s.hd) : 0.f;
    if (pad) {   // the padded weight copies are shared by all layers: rebuild this layer's
        TRY(launch_pad_heads(W + o.wqkv, P + o.bqkv, W + o.wo, s.wqkv_pad, s.bqkv_pad, s.wo_pad, D, s.H, s.hd, s.hdp, st));
        Wqkv = s.wqkv_pad; Wo = s.wo_pad;
    }
    {
        GemmProblem p = gemm(dhb, (size_t)Mq * D, D, Wo, (size_t)D * Da, Da, Mq, Da, D, EPI_BF16, c_.dctx, Da);
        TRY(launch_gemm(&p, 1, GEMM_NN, -1, st));
    }
    if (tail) TRY(launch_attn_bwd_win(a.qkv, a.ctx, c_.dctx, a.lse, c_.delta, dqkv, B, N, s.H, s.hdp, tail->nvis, tail->ndec, st, sm_scale));
    else TRY(launch_attn_bwd(a.qkv, a.ctx, c_.dctx, a.lse, c_.delta, dqkv, B, N, s.H, s.hdp, st, sm_scale));
    const int Mv = first ? B * first->nvis : 0, Lp = first ? first->L : 0;
    if (first) {
        // first mode: S hi / lo behind the compact visible dqkv rows (one K range for the weight gradient below); dX qkv of the visible rows
        // as bf16 for the separate LayerNorm backward, of the S rows as f32, then as a pair.  The next bf16 copy is not produced: what
        // follows the first layer of such a stack reads the f32 rows.
        BVC_REQUIRE(li == 0 && !tail && !pad && !gated && first->nvis + first->ndec == N && first->dtoken, "layer_backward: first mode is not available for this layer");
        const int W3 = 3 * Da;
        bf16_t* shi = first->qc + (size_t)Mv * W3;
        TRY(launch_first_reduce(dqkv, first->dec_slot, B, Lp, N, first->nvis, W3, nullptr, shi, shi + (size_t)Lp * W3, st));
        TRY(launch_gather_rows_copy_bf16(dqkv, RowMap{first->nvis, N, 0}, first->qc, Mv, W3, st));
        // (the visible rows: bf16 as the separate LayerNorm passes take it, or - where the off path's epilogue would have seen the f32 product -
        //  f32 and then a pair, so that the two paths differ by no rounding of their own)
        GemmProblem p = gemm(first->qc, (size_t)Mv * W3, W3, Wqkv, (size_t)W3 * D, D, Mv, D, W3, fuse ? EPI_F32 : EPI_BF16, fuse ? (void*)first->xv : (void*)c_.dln, D);
        TRY(launch_gemm(&p, 1, GEMM_NN, -1, st));
        if (fuse) TRY(launch_pair_split(first->xv, nullptr, first->dyv, first->dyv + (size_t)Mv * D, (size_t)Mv * D, st));
        GemmProblem t = gemm(shi, (size_t)2 * Lp * W3, W3, Wqkv, (size_t)W3 * D, D, 2 * Lp, D, W3, EPI_F32, first->xt, D);
        TRY(launch_gemm(&t, 1, GEMM_NN, -1, st));
        TRY(launch_pair_split(first->xt, first->xt + (size_t)Lp * D, first->dyt, first->dyt + (size_t)Lp * D, (size_t)Lp * D, st));
    } else if (fuse) {      // dX of qkv with the first LayerNorm's backward in its epilogue: dres becomes d/d(layer input), dyb_next its bf16 copy
        GemmProblem p = gemm(dqkv, (size_t)M * 3 * Da, 3 * Da, Wqkv, (size_t)3 * Da * D, D, M, D, 3 * Da, EPI_DLN, dres, D);
        p.C2 = dyb_next; p.ln_x = x_in; p.ln_mean = a.mean1; p.ln_rstd = a.rstd1; p.ln_gamma = P + o.ln1w;
        p.ln_part = c_.ln_part; p.ln_dgamma = G + o.ln1w; p.ln_dbeta = G + o.ln1b;
        TRY(launch_gemm(&p, 1, GEMM_NN, -1, st));
    } else {
        GemmProblem p = gemm(dqkv, (size_t)M * 3 * Da, 3 * Da, Wqkv, (size_t)3 * Da * D, D, M, D, 3 * Da, EPI_BF16, c_.dln, D);
        TRY(launch_gemm(&p, 1, GEMM_NN, -1, st));
    }
    // the four weight gradients of the layer as one grouped launch:  dW = dY^T X,  db = column sums of dY
    hipStream_t ws = st;
    if (c_.overlap) {
        BVC_CHECK_HIP(hipEventRecord(c_.ev_fork, st));
        BVC_CHECK_HIP(hipStreamWaitEvent(c_.side, c_.ev_fork, 0));
        ws = c_.side;
    }
    {
        GemmProblem g[4];
        // (tail mode: the fc2 / fc1 / proj members contract over the Mq compact rows, the qkv member over all M)
        g[0] = gemm(dyb, (size_t)Mq * D, D, a.act, (size_t)Mq * I, I, D, I, Mq, EPI_F32, G + o.w2, I);
        g[1] = gemm(dh, (size_t)Mq * I, I, a.ln2o, (size_t)Mq * D, D, I, D, Mq, EPI_F32, G + o.w1, D);
        g[2] = gemm(dhb, (size_t)Mq * D, D, a.ctx, (size_t)Mq * Da, Da, D, Da, Mq, EPI_F32, pad ? s.gwo_pad : G + o.wo, Da);
        g[3] = gemm(dqkv, (size_t)M * 3 * Da, 3 * Da, a.ln1o, (size_t)M * D, D, 3 * Da, D, M, EPI_F32, pad ? s.gwqkv_pad : G + o.wqkv, D);
        if (first) {     // [visible dqkv | S hi | S lo]^T [LN1 visible | T1 | T1]: the mask rows' share rides in the same contraction
            const int Kf = Mv + 2 * Lp;
            g[3] = gemm(first->qc, (size_t)Kf * 3 * Da, 3 * Da, first->ln1c, (size_t)Kf * D, D, 3 * Da, D, Kf, EPI_F32, G + o.wqkv, D);
        }
        g[0].rowsum = G + o.b2;     // bias gradients ride along as one extra MFMA column each
        g[1].rowsum = G + o.b1;
        g[2].rowsum = G + o.bo;
        g[3].rowsum = pad ? s.gbqkv_pad : G + o.bqkv;
        const int tile = plan_dw(g, 4);
        if (pad) {   // split-K accumulates with atomics: the padded scratch is zeroed like the gradient buffer is
            BVC_CHECK_HIP(hipMemsetAsync(s.gwo_pad, 0, (size_t)D * Da * 4, ws));
            BVC_CHECK_HIP(hipMemsetAsync(s.gwqkv_pad, 0, (size_t)3 * Da * D * 4, ws));
            BVC_CHECK_HIP(hipMemsetAsync(s.gbqkv_pad, 0, (size_t)3 * Da * 4, ws));
        }
        TRY(launch_gemm(g, 4, GEMM_TN, tile, ws));
        if (pad)
            TRY(launch_unpad_head_grads(s.gwqkv_pad, s.gbqkv_pad, s.gwo_pad, G + o.wqkv, G + o.bqkv, G + o.wo, D, s.H, s.hd, s.hdp, ws));
    }
    if (first) {
        const RowMap vis{first->nvis, N, 0};
        TRY(launch_ln_bwd(fuse ? first->dyv : c_.dln, x_in, vis, a.mean1, a.rstd1, P + o.ln1w, dres, 1, nullptr, G + o.ln1w, G + o.ln1b, c_.ln_part, Mv, D, st));
        if (fuse) TRY(launch_ln_bwd(first->dyv + (size_t)Mv * D, x_in, vis, a.mean1, a.rstd1, P + o.ln1w, dres, 1, nullptr, G + o.ln1w, G + o.ln1b, c_.ln_part, Mv, D, st));
        TRY(launch_ln_bwd(first->dyt, first->t0, identity_rows(), first->tmean, first->trstd, P + o.ln1w, first->dt, 0, nullptr, G + o.ln1w, G + o.ln1b,
                          first->part, 2 * Lp, D, st));
        TRY(launch_colsum_f32(first->dt, identity_rows(), 2 * Lp, D, first->dtoken, st));
    } else if (!fuse) TRY(launch_ln_bwd(c_.dln, x_in, identity_rows(), a.mean1, a.rstd1, P + o.ln1w, dres, 1, dyb_next, G + o.ln1w, G + o.ln1b, c_.ln_part, M, D, st,
                                 gated && li > 0 ? &g_below : nullptr));
    if (c_.overlap) {
        BVC_CHECK_HIP(hipEventRecord(c_.ev_join[par], c_.side));
        c_.join_pending[par] = true;
        c_.pend_lo[par] = o.ln1w;
        c_.pend_hi[par] = o.end;
    } else if (on_bucket) {
        on_bucket(o.ln1w, o.end - o.ln1w, user);
    }
    c_.seq = q + 1;
    return BVC_OK;
}

}  // namespace bvc

// Layer-wise trust ratios: LARS and LAMB over a flat f32 range cut into segments (one per parameter tensor), include/bvc.h
// "Layer-wise trust ratios".  Both are two streaming passes with a tiny reduction between them:
//
//   items pass    one workgroup per bvc_norm_item - the work list of the gradient-norm pass (rowops.hip), at most kItemCap elements,
//                 never across a segment boundary.  LARS reads w and g and forms d = g / scale + wd w; LAMB reads w, g, m, v, updates
//                 m and v in place and forms u.  Thread t takes 16-byte vectors t, t + 256, ... of the item: every f32 accumulator adds
//                 at most kChain squares (fused multiply-add); lanes, head / tail elements, waves and the four waves are added in f64
//                 in a fixed order into item_partial[2 i] = sum w^2 and item_partial[2 i + 1] = sum d^2 (u^2).
//   ratio         one workgroup per segment adds its items' partials in f64 in a fixed order: seg_stats[s] = {||w||, ||d||, ratio}.
//   apply pass    1024 elements per workgroup over the whole range with blk_seg, as the *_step_table kernels of rowops.hip: a quad
//                 inside one segment takes 16-byte loads and stores, a quad across a boundary goes element by element.
//
// No atomics anywhere.  The quantity whose norm is taken (d, u) and the one that is applied come out of ONE __device__ function each
// (lars_d, lamb_u) and this file is compiled without floating-point contraction, every fused multiply-add written out: the two passes
// cannot round differently.  Every kernel returns at once when *found_inf != 0.
//
// Group rows (8 floats, written per call from kernel arguments as rowops.hip's tables are):
//   LARS: { lr, wd, momentum, trust_coefficient | flags, 0, 0, 0 }      flags: 1 = nesterov, 2 = maximize, 4 = adapt
//   LAMB: { 1 - b1, b2, 1 - b2, eps | wd, lr, flags, 0 }                flags: 2 = maximize, 4 = adapt
//   LAMB step scalars: state[3 grp + {0, 1, 2}] = { step, 1 / (1 - b1^step), 1 / sqrt(1 - b2^step) }
#include "optim_layerwise.h"

#pragma clang fp contract(off)

namespace bvc {
namespace {

constexpr int kRowFloats = 8;
constexpr int kItemCap = BVC_GRAD_NORM_ITEM_CAP;
constexpr int kChain = kItemCap / (256 * 4);
static_assert(kChain * 256 * 4 == kItemCap, "an item is a whole number of 16-byte vectors per thread");

// (find_segment, wave_sum_f64 and block_sum_f64 as in rowops.hip)
__device__ __forceinline__ int find_segment(const int64_t* __restrict__ seg_start, int s, int64_t i) {
    while (seg_start[s + 1] <= i) ++s;
    return s;
}
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// 256 threads -> the sum in every thread (waves added as (w0 + w1) + (w2 + w3))
__device__ __forceinline__ double block_sum_f64(double v, double* lds4) {
    v = wave_sum_f64(v);
    if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = v;
    __syncthreads();
    return (lds4[0] + lds4[1]) + (lds4[2] + lds4[3]);
}
__device__ __forceinline__ double lanes_f64(const f32x4 a) { return ((double)a[0] + (double)a[1]) + ((double)a[2] + (double)a[3]); }
__device__ __forceinline__ bool skipped(const float* found_inf) { return found_inf != nullptr && *found_inf != 0.f; }

// ---------------------------------------------------------------------------------------------- LARS
struct LarsRow { float lr, wd, momentum, trust; int fl; };
__device__ __forceinline__ LarsRow lars_row(const float* __restrict__ table, int grp) {
    const f32x4 r0 = *reinterpret_cast<const f32x4*>(table + (size_t)grp * kRowFloats);
    return LarsRow{r0[0], r0[1], r0[2], r0[3], __float_as_int(table[(size_t)grp * kRowFloats + 4])};
}
// the unscaled (and, under maximize, negated) gradient, and d = that + wd w: what the norm is taken of and what is applied
__device__ __forceinline__ float lars_g(float g, float inv, int fl) {
    const float gr = g * inv;
    return (fl & 2) ? -gr : gr;
}
__device__ __forceinline__ float lars_d(float gr, float w, float wd) { return __builtin_fmaf(wd, w, gr); }

struct LarsChunkDev {
    float lr[BVC_OPT_TABLE_CHUNK], wd[BVC_OPT_TABLE_CHUNK], momentum[BVC_OPT_TABLE_CHUNK], trust[BVC_OPT_TABLE_CHUNK];
    int flags[BVC_OPT_TABLE_CHUNK];
};
struct LambChunkDev {
    double beta1[BVC_OPT_TABLE_CHUNK], beta2[BVC_OPT_TABLE_CHUNK];      // for the step scalars, in double
    float omb1[BVC_OPT_TABLE_CHUNK], beta2f[BVC_OPT_TABLE_CHUNK], omb2[BVC_OPT_TABLE_CHUNK], eps[BVC_OPT_TABLE_CHUNK], wd[BVC_OPT_TABLE_CHUNK],
        lr[BVC_OPT_TABLE_CHUNK];
    int flags[BVC_OPT_TABLE_CHUNK];
};
static_assert(sizeof(LarsChunkDev) + 64 <= 4096 && sizeof(LambChunkDev) + 64 <= 4096, "a chunk must fit the kernel-argument segment");

// rows [g0, g0 + count) of the LARS table, one thread per group
__global__ void lars_table_write_kernel(float* __restrict__ table, int g0, int count, const LarsChunkDev C, const float* __restrict__ found_inf) {
    const int t = threadIdx.x;
    if (blockIdx.x != 0 || t >= count || skipped(found_inf)) return;
    float* row = table + (size_t)(g0 + t) * kRowFloats;
    *reinterpret_cast<f32x4*>(row) = f32x4{C.lr[t], C.wd[t], C.momentum[t], C.trust[t]};
    *reinterpret_cast<f32x4*>(row + 4) = f32x4{__int_as_float(C.flags[t]), 0.f, 0.f, 0.f};
}

// sum w^2 and sum d^2 of one item; *found_inf is set when a gradient element of the item is Inf or NaN
__global__ __launch_bounds__(256) void lars_norm_items_kernel(const float* __restrict__ w, const float* __restrict__ g,
                                                              const bvc_norm_item* __restrict__ items, const int* __restrict__ seg_group,
                                                              const float* __restrict__ table, int ngroups,
                                                              const float* __restrict__ grad_scale, float* __restrict__ found_inf,
                                                              double* __restrict__ item_partial) {
    __shared__ double lds_w[4], lds_d[4];
    __shared__ int skip;
    const int tid = threadIdx.x;
    // other workgroups of this very launch may set *found_inf: one thread reads it for the whole workgroup, so that either every wave
    // leaves here or every wave reaches the barriers below
    if (tid == 0) skip = skipped(found_inf);
    __syncthreads();
    if (skip) return;
    const bvc_norm_item it = items[blockIdx.x];
    const int grp = seg_group[it.segment];
    if (grp < 0 || grp >= ngroups) {                             // (uniform per workgroup) a malformed table: nothing to add
        if (tid == 0) { item_partial[2 * (size_t)blockIdx.x] = 0.0; item_partial[2 * (size_t)blockIdx.x + 1] = 0.0; }
        return;
    }
    const float inv = grad_scale ? 1.f / *grad_scale : 1.f;
    const LarsRow R = lars_row(table, grp);
    const float* __restrict__ pw = w + it.start;
    const float* __restrict__ pg = g + it.start;
    const int len = it.length;
    int head = (int)((4 - (it.start & 3)) & 3);                 // w and g are 16-byte aligned: elements before the first boundary
    head = head < len ? head : len;
    const int nvec = (len - head) >> 2;
    const int tail0 = head + 4 * nvec;
    const f32x4* __restrict__ vw = reinterpret_cast<const f32x4*>(pw + head);
    const f32x4* __restrict__ vg = reinterpret_cast<const f32x4*>(pg + head);
    f32x4 aw = {0.f, 0.f, 0.f, 0.f}, ad = {0.f, 0.f, 0.f, 0.f};
    float t = 0.f;                                               // (v - v) is 0 for finite values and NaN for Inf / NaN
    for (int i0 = tid; i0 < nvec; i0 += 4 * 256) {               // four vectors of each array are loaded before the first use
        f32x4 a[4], b[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int i = i0 + 256 * k;
            const bool in = i < nvec;
            a[k] = in ? vw[i] : f32x4{0.f, 0.f, 0.f, 0.f};      // (zeros add nothing: d = 0)
            b[k] = in ? vg[i] : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float d = lars_d(lars_g(b[k][e], inv, R.fl), a[k][e], R.wd);
                aw[e] = __builtin_fmaf(a[k][e], a[k][e], aw[e]);
                ad[e] = __builtin_fmaf(d, d, ad[e]);
                t += b[k][e] - b[k][e];
            }
        }
    }
    double hw = 0.0, hd = 0.0;                                   // head / tail elements: at most one of each per thread
    if (tid < head) {
        const float we = pw[tid], ge = pg[tid], d = lars_d(lars_g(ge, inv, R.fl), we, R.wd);
        hw = (double)we * (double)we; hd = (double)d * (double)d; t += ge - ge;
    }
    if (tail0 + tid < len) {
        const float we = pw[tail0 + tid], ge = pg[tail0 + tid], d = lars_d(lars_g(ge, inv, R.fl), we, R.wd);
        hw += (double)we * (double)we; hd += (double)d * (double)d; t += ge - ge;
    }
    const double sw = block_sum_f64(lanes_f64(aw) + hw, lds_w), sd = block_sum_f64(lanes_f64(ad) + hd, lds_d);
    if (tid == 0) { item_partial[2 * (size_t)blockIdx.x] = sw; item_partial[2 * (size_t)blockIdx.x + 1] = sd; }
    if (found_inf != nullptr && __any(t != 0.f) && (tid & 63) == 0) *found_inf = 1.0f;
}

// item partials -> seg_stats[s] = {||w||, ||d|| or ||u||, ratio}, block s = segment s; f64 in a fixed order, cast to f32 at the end
__global__ __launch_bounds__(256) void trust_ratio_kernel(const double* __restrict__ item_partial, const int64_t* __restrict__ seg_first_item,
                                                          const int* __restrict__ seg_group, const float* __restrict__ table, int ngroups,
                                                          int lamb, const float* __restrict__ found_inf, float* __restrict__ seg_stats) {
    __shared__ double lds_w[4], lds_d[4];
    if (skipped(found_inf)) return;
    const int s = blockIdx.x, grp = seg_group[s];
    const bool owned = grp >= 0 && grp < ngroups;
    const int64_t lo = owned ? seg_first_item[s] : 0, hi = owned ? seg_first_item[s + 1] : 0;
    double a = 0.0, b = 0.0;
#pragma unroll 4
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) { a += item_partial[2 * i]; b += item_partial[2 * i + 1]; }
    const double sw = block_sum_f64(a, lds_w), sd = block_sum_f64(b, lds_d);
    if (threadIdx.x != 0) return;
    const double nw = sqrt(sw), nd = sqrt(sd);
    double ratio = 1.0;
    if (owned) {
        const float* row = table + (size_t)grp * kRowFloats;
        const int fl = __float_as_int(lamb ? row[6] : row[4]);
        const double coef = lamb ? 1.0 : (double)row[3];
        if ((fl & 4) && nw > 0.0 && nd > 0.0) ratio = coef * nw / nd;
    }
    seg_stats[3 * (size_t)s] = (float)nw; seg_stats[3 * (size_t)s + 1] = (float)nd; seg_stats[3 * (size_t)s + 2] = (float)ratio;
}

// d = ratio d;  buf = momentum buf + d;  w -= lr (nesterov ? d + momentum buf : buf)
__device__ __forceinline__ float lars_update(float w, float gr, float* bv, float ratio, const LarsRow& R) {
    const float d = lars_d(gr, w, R.wd) * ratio;
    float upd = d;
    if (R.momentum != 0.f) {
        *bv = __builtin_fmaf(*bv, R.momentum, d);
        upd = (R.fl & 1) ? __builtin_fmaf(*bv, R.momentum, d) : *bv;
    }
    return __builtin_fmaf(-R.lr, upd, w);
}

__global__ __launch_bounds__(256) void lars_apply_kernel(float* __restrict__ p, float* __restrict__ g, float* __restrict__ buf, int64_t n,
                                                         const int64_t* __restrict__ seg_start, const int* __restrict__ seg_group,
                                                         const int* __restrict__ blk_seg, const float* __restrict__ table, int ngroups,
                                                         const float* __restrict__ seg_stats, const float* __restrict__ grad_scale,
                                                         const float* __restrict__ found_inf, int write_grad, bf16_t* __restrict__ shadow) {
    if (skipped(found_inf)) return;
    const float inv = grad_scale ? 1.f / *grad_scale : 1.f;
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    int s = find_segment(seg_start, blk_seg[blockIdx.x], i);
    if (i + 4 <= n && i + 4 <= seg_start[s + 1]) {
        const int grp = seg_group[s];
        if (grp < 0 || grp >= ngroups) return;
        const f32x4 pv = *reinterpret_cast<const f32x4*>(p + i);
        const f32x4 gv = *reinterpret_cast<const f32x4*>(g + i);
        const LarsRow R = lars_row(table, grp);
        f32x4 bv = {0.f, 0.f, 0.f, 0.f};
        if (R.momentum != 0.f) bv = *reinterpret_cast<const f32x4*>(buf + i);
        const float ratio = seg_stats[3 * (size_t)s + 2];
        f32x4 pn, gu;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            gu[e] = lars_g(gv[e], inv, R.fl);
            float b = bv[e];
            pn[e] = lars_update(pv[e], gu[e], &b, ratio, R);
            bv[e] = b;
        }
        *reinterpret_cast<f32x4*>(p + i) = pn;
        if (R.momentum != 0.f) *reinterpret_cast<f32x4*>(buf + i) = bv;
        if (shadow) *reinterpret_cast<uint2*>(shadow + i) = uint2{pack2bf(pn[0], pn[1]), pack2bf(pn[2], pn[3])};
        if (write_grad) *reinterpret_cast<f32x4*>(g + i) = gu;
    } else {
        for (int64_t j = i; j < n && j < i + 4; ++j) {
            s = find_segment(seg_start, s, j);
            const int grp = seg_group[s];
            if (grp < 0 || grp >= ngroups) continue;
            const LarsRow R = lars_row(table, grp);
            const float gu = lars_g(g[j], inv, R.fl);
            float b = R.momentum != 0.f ? buf[j] : 0.f;
            const float pn = lars_update(p[j], gu, &b, seg_stats[3 * (size_t)s + 2], R);
            p[j] = pn;
            if (R.momentum != 0.f) buf[j] = b;
            if (shadow) shadow[j] = f2bf(pn);
            if (write_grad) g[j] = gu;
        }
    }
}

// ---------------------------------------------------------------------------------------------- LAMB
struct LambRow { float omb1, beta2, omb2, eps, wd, lr; int fl; float rbc1, rsbc2; };
__device__ __forceinline__ LambRow lamb_row(const float* __restrict__ table, const float* __restrict__ state, int grp) {
    const f32x4 r0 = *reinterpret_cast<const f32x4*>(table + (size_t)grp * kRowFloats);
    const f32x4 r1 = *reinterpret_cast<const f32x4*>(table + (size_t)grp * kRowFloats + 4);
    return LambRow{r0[0], r0[1], r0[2], r0[3], r1[0], r1[1], __float_as_int(r1[2]), state[3 * grp + 1], state[3 * grp + 2]};
}
// m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g g  (adam_step_table_kernel's statements); returns the unscaled gradient
__device__ __forceinline__ float lamb_moments(float g, float inv, float* m, float* v, const LambRow& R) {
    float gr = g * inv;
    if (R.fl & 2) gr = -gr;
    *m = *m + R.omb1 * (gr - *m);
    *v = __builtin_fmaf(*v, R.beta2, R.omb2 * (gr * gr));
    return gr;
}
// u = (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + eps) + wd w: what the norm is taken of (pass 1) and what is applied (pass 2)
__device__ __forceinline__ float lamb_u(float m, float v, float w, const LambRow& R) {
    return __builtin_fmaf(R.wd, w, (m * R.rbc1) / (sqrtf(v) * R.rsbc2 + R.eps));
}

// rows [g0, g0 + count) of the LAMB table and the groups' step scalars (in double; nothing on a step the scaler skips)
__global__ void lamb_prep_table_kernel(float* __restrict__ state, float* __restrict__ table, int g0, int count, const LambChunkDev C,
                                       const float* __restrict__ found_inf) {
    const int t = threadIdx.x;
    if (blockIdx.x != 0 || t >= count || skipped(found_inf)) return;
    const int grp = g0 + t;
    float* row = table + (size_t)grp * kRowFloats;
    *reinterpret_cast<f32x4*>(row) = f32x4{C.omb1[t], C.beta2f[t], C.omb2[t], C.eps[t]};
    *reinterpret_cast<f32x4*>(row + 4) = f32x4{C.wd[t], C.lr[t], __int_as_float(C.flags[t]), 0.f};
    const double step = (double)state[3 * grp] + 1.0;
    state[3 * grp] = (float)step;
    state[3 * grp + 1] = (float)(1.0 / (1.0 - pow(C.beta1[t], step)));
    state[3 * grp + 2] = (float)(1.0 / sqrt(1.0 - pow(C.beta2[t], step)));
}

// pass 1: the moments of one item in place (and the unscaled gradient back), sum w^2 and sum u^2
__global__ __launch_bounds__(256) void lamb_moment_items_kernel(const float* __restrict__ w, float* __restrict__ g, float* __restrict__ m,
                                                                float* __restrict__ v, const bvc_norm_item* __restrict__ items,
                                                                const int* __restrict__ seg_group, const float* __restrict__ table,
                                                                int ngroups, const float* __restrict__ state,
                                                                const float* __restrict__ grad_scale, const float* __restrict__ found_inf,
                                                                int write_grad, double* __restrict__ item_partial) {
    __shared__ double lds_w[4], lds_u[4];
    if (skipped(found_inf)) return;
    const bvc_norm_item it = items[blockIdx.x];
    const int grp = seg_group[it.segment], tid = threadIdx.x;
    if (grp < 0 || grp >= ngroups) {                             // (uniform per workgroup) a malformed table: nothing to add
        if (tid == 0) { item_partial[2 * (size_t)blockIdx.x] = 0.0; item_partial[2 * (size_t)blockIdx.x + 1] = 0.0; }
        return;
    }
    const float inv = grad_scale ? 1.f / *grad_scale : 1.f;
    const LambRow R = lamb_row(table, state, grp);
    const int64_t at = it.start;
    const int len = it.length;
    int head = (int)((4 - (at & 3)) & 3);                       // all four arrays are 16-byte aligned
    head = head < len ? head : len;
    const int nvec = (len - head) >> 2;
    const int tail0 = head + 4 * nvec;
    const f32x4* __restrict__ vw = reinterpret_cast<const f32x4*>(w + at + head);
    f32x4* __restrict__ vg = reinterpret_cast<f32x4*>(g + at + head);
    f32x4* __restrict__ vm = reinterpret_cast<f32x4*>(m + at + head);
    f32x4* __restrict__ vv = reinterpret_cast<f32x4*>(v + at + head);
    f32x4 aw = {0.f, 0.f, 0.f, 0.f}, au = {0.f, 0.f, 0.f, 0.f};
    for (int i0 = tid; i0 < nvec; i0 += 2 * 256) {               // two vectors of each array are loaded before the first use
        f32x4 a[2], b[2], c[2], d[2];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int i = i0 + 256 * k;
            if (i < nvec) { a[k] = vw[i]; b[k] = vg[i]; c[k] = vm[i]; d[k] = vv[i]; }
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int i = i0 + 256 * k;
            if (i >= nvec) continue;
            f32x4 gu;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float me = c[k][e], ve = d[k][e];
                gu[e] = lamb_moments(b[k][e], inv, &me, &ve, R);
                const float u = lamb_u(me, ve, a[k][e], R);
                aw[e] = __builtin_fmaf(a[k][e], a[k][e], aw[e]);
                au[e] = __builtin_fmaf(u, u, au[e]);
                c[k][e] = me; d[k][e] = ve;
            }
            vm[i] = c[k]; vv[i] = d[k];
            if (write_grad) vg[i] = gu;
        }
    }
    double hw = 0.0, hu = 0.0;                                   // head / tail elements: at most one of each per thread
#pragma unroll
    for (int part = 0; part < 2; ++part) {
        const int j = part == 0 ? tid : tail0 + tid;
        if (part == 0 ? tid < head : j < len) {
            const float we = w[at + j];
            float me = m[at + j], ve = v[at + j];
            const float gu = lamb_moments(g[at + j], inv, &me, &ve, R);
            const float u = lamb_u(me, ve, we, R);
            hw += (double)we * (double)we; hu += (double)u * (double)u;
            m[at + j] = me; v[at + j] = ve;
            if (write_grad) g[at + j] = gu;
        }
    }
    const double sw = block_sum_f64(lanes_f64(aw) + hw, lds_w), su = block_sum_f64(lanes_f64(au) + hu, lds_u);
    if (tid == 0) { item_partial[2 * (size_t)blockIdx.x] = sw; item_partial[2 * (size_t)blockIdx.x + 1] = su; }
}

// pass 2: w -= lr ratio u, u recomputed from the updated moments and the parameters pass 1 saw
__global__ __launch_bounds__(256) void lamb_apply_kernel(float* __restrict__ p, const float* __restrict__ m, const float* __restrict__ v, int64_t n,
                                                         const int64_t* __restrict__ seg_start, const int* __restrict__ seg_group,
                                                         const int* __restrict__ blk_seg, const float* __restrict__ table, int ngroups,
                                                         const float* __restrict__ state, const float* __restrict__ seg_stats,
                                                         const float* __restrict__ found_inf, bf16_t* __restrict__ shadow) {
    if (skipped(found_inf)) return;
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n) return;
    int s = find_segment(seg_start, blk_seg[blockIdx.x], i);
    if (i + 4 <= n && i + 4 <= seg_start[s + 1]) {
        const int grp = seg_group[s];
        if (grp < 0 || grp >= ngroups) return;
        const f32x4 pv = *reinterpret_cast<const f32x4*>(p + i);
        const f32x4 mv = *reinterpret_cast<const f32x4*>(m + i);
        const f32x4 vv = *reinterpret_cast<const f32x4*>(v + i);
        const LambRow R = lamb_row(table, state, grp);
        const float step = R.lr * seg_stats[3 * (size_t)s + 2];
        f32x4 pn;
#pragma unroll
        for (int e = 0; e < 4; ++e) pn[e] = __builtin_fmaf(-step, lamb_u(mv[e], vv[e], pv[e], R), pv[e]);
        *reinterpret_cast<f32x4*>(p + i) = pn;
        if (shadow) *reinterpret_cast<uint2*>(shadow + i) = uint2{pack2bf(pn[0], pn[1]), pack2bf(pn[2], pn[3])};
    } else {
        for (int64_t j = i; j < n && j < i + 4; ++j) {
            s = find_segment(seg_start, s, j);
            const int grp = seg_group[s];
            if (grp < 0 || grp >= ngroups) continue;
            const LambRow R = lamb_row(table, state, grp);
            const float step = R.lr * seg_stats[3 * (size_t)s + 2];
            const float pn = __builtin_fmaf(-step, lamb_u(m[j], v[j], p[j], R), p[j]);
            p[j] = pn;
            if (shadow) shadow[j] = f2bf(pn);
        }
    }
}

int check_layerwise(const char* who, int64_t n, const int64_t* seg_start, const int* seg_group, const int* blk_seg, int nseg,
                    const bvc_norm_item* items, int64_t nitems, const int64_t* seg_first_item, int ngroups, const float* table,
                    const double* item_partial, const float* seg_stats, const bf16_t* shadow) {
    BVC_REQUIRE(seg_start && seg_group && blk_seg && nseg > 0, "%s: segment table missing", who);
    BVC_REQUIRE(ngroups >= 1 && ngroups <= BVC_OPT_TABLE_MAX_GROUPS, "%s: %d parameter groups (1..%d)", who, ngroups, BVC_OPT_TABLE_MAX_GROUPS);
    BVC_REQUIRE(table != nullptr && (uintptr_t)table % 16 == 0, "%s: the group table must be a 16-byte aligned device buffer", who);
    BVC_REQUIRE(n > 0, "%s: empty range", who);
    BVC_REQUIRE(nitems >= 0 && nitems <= 0x7fffffff, "%s: %lld items", who, (long long)nitems);
    BVC_REQUIRE(seg_first_item != nullptr && (nitems == 0 || items != nullptr), "%s: work list missing", who);
    BVC_REQUIRE(item_partial != nullptr && (uintptr_t)item_partial % 8 == 0 && seg_stats != nullptr, "%s: item_partial / seg_stats missing", who);
    BVC_REQUIRE(shadow == nullptr || (uintptr_t)shadow % 8 == 0, "%s: the bf16 shadow must be 8-byte aligned", who);
    return BVC_OK;
}

}  // namespace

int launch_lars_step_table(float* p, float* g, float* buf, int64_t n, const int64_t* seg_start, const int* seg_group, const int* blk_seg,
                           int nseg, const bvc_norm_item* items, int64_t nitems, const int64_t* seg_first_item, int ngroups,
                           const float* lr, const float* momentum, const float* wd, const float* trust, const int* nesterov,
                           const int* adapt, const int* maximize, float* table, double* item_partial, float* seg_stats,
                           const float* grad_scale, float* found_inf, int write_grad, bf16_t* shadow, hipStream_t s) {
    if (int rc = check_layerwise("lars_step_table", n, seg_start, seg_group, blk_seg, nseg, items, nitems, seg_first_item, ngroups, table,
                                 item_partial, seg_stats, shadow)) return rc;
    BVC_REQUIRE(lr && momentum && wd && trust && nesterov && adapt && maximize, "lars_step_table: hyper-parameter array missing");
    BVC_REQUIRE(((uintptr_t)p % 16 == 0) && ((uintptr_t)g % 16 == 0) && (buf == nullptr || (uintptr_t)buf % 16 == 0),
                "lars_step_table: buffers must be 16-byte aligned");
    for (int i = 0; i < ngroups; ++i) BVC_REQUIRE(momentum[i] == 0.f || buf != nullptr, "lars_step_table: momentum needs a buffer");
    for (int g0 = 0; g0 < ngroups; g0 += BVC_OPT_TABLE_CHUNK) {
        const int count = ngroups - g0 < BVC_OPT_TABLE_CHUNK ? ngroups - g0 : BVC_OPT_TABLE_CHUNK;
        LarsChunkDev C;
        for (int t = 0; t < BVC_OPT_TABLE_CHUNK; ++t) {
            const int j = g0 + (t < count ? t : 0);
            C.lr[t] = lr[j]; C.wd[t] = wd[j]; C.momentum[t] = momentum[j]; C.trust[t] = trust[j];
            C.flags[t] = (nesterov[j] ? 1 : 0) | (maximize[j] ? 2 : 0) | (adapt[j] ? 4 : 0);
        }
        hipLaunchKernelGGL(lars_table_write_kernel, dim3(1), dim3(BVC_OPT_TABLE_CHUNK), 0, s, table, g0, count, C, (const float*)found_inf);
    }
    if (nitems > 0)
        hipLaunchKernelGGL(lars_norm_items_kernel, dim3((unsigned)nitems), dim3(256), 0, s, (const float*)p, (const float*)g, items, seg_group,
                           (const float*)table, ngroups, grad_scale, found_inf, item_partial);
    hipLaunchKernelGGL(trust_ratio_kernel, dim3((unsigned)nseg), dim3(256), 0, s, (const double*)item_partial, seg_first_item, seg_group,
                       (const float*)table, ngroups, 0, (const float*)found_inf, seg_stats);
    hipLaunchKernelGGL(lars_apply_kernel, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0, s, p, g, buf, n, seg_start, seg_group, blk_seg,
                       (const float*)table, ngroups, (const float*)seg_stats, grad_scale, (const float*)found_inf, write_grad, shadow);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

int launch_lamb_step_table(float* p, float* g, float* m, float* v, int64_t n, const int64_t* seg_start, const int* seg_group,
                           const int* blk_seg, int nseg, const bvc_norm_item* items, int64_t nitems, const int64_t* seg_first_item,
                           int ngroups, const double* lr, const double* beta1, const double* beta2, const double* eps, const double* wd,
                           const int* adapt, const int* maximize, float* state, float* table, double* item_partial, float* seg_stats,
                           const float* grad_scale, const float* found_inf, int write_grad, bf16_t* shadow, hipStream_t s) {
    if (int rc = check_layerwise("lamb_step_table", n, seg_start, seg_group, blk_seg, nseg, items, nitems, seg_first_item, ngroups, table,
                                 item_partial, seg_stats, shadow)) return rc;
    BVC_REQUIRE(lr && beta1 && beta2 && eps && wd && adapt && maximize && state, "lamb_step_table: hyper-parameter array / state missing");
    BVC_REQUIRE(((uintptr_t)p % 16 == 0) && ((uintptr_t)g % 16 == 0) && ((uintptr_t)m % 16 == 0) && ((uintptr_t)v % 16 == 0),
                "lamb_step_table: buffers must be 16-byte aligned");
    for (int g0 = 0; g0 < ngroups; g0 += BVC_OPT_TABLE_CHUNK) {
        const int count = ngroups - g0 < BVC_OPT_TABLE_CHUNK ? ngroups - g0 : BVC_OPT_TABLE_CHUNK;
        LambChunkDev C;
        for (int t = 0; t < BVC_OPT_TABLE_CHUNK; ++t) {
            const int j = g0 + (t < count ? t : 0);
            // hyper-parameters arrive as doubles (python floats) and are combined in double before the cast
            C.omb1[t] = (float)(1.0 - beta1[j]); C.beta2f[t] = (float)beta2[j]; C.omb2[t] = (float)(1.0 - beta2[j]);
            C.eps[t] = (float)eps[j]; C.wd[t] = (float)wd[j]; C.lr[t] = (float)lr[j];
            C.flags[t] = (maximize[j] ? 2 : 0) | (adapt[j] ? 4 : 0);
            C.beta1[t] = beta1[j]; C.beta2[t] = beta2[j];
        }
        hipLaunchKernelGGL(lamb_prep_table_kernel, dim3(1), dim3(BVC_OPT_TABLE_CHUNK), 0, s, state, table, g0, count, C, found_inf);
    }
    if (nitems > 0)
        hipLaunchKernelGGL(lamb_moment_items_kernel, dim3((unsigned)nitems), dim3(256), 0, s, (const float*)p, g, m, v, items, seg_group,
                           (const float*)table, ngroups, (const float*)state, grad_scale, found_inf, write_grad, item_partial);
    hipLaunchKernelGGL(trust_ratio_kernel, dim3((unsigned)nseg), dim3(256), 0, s, (const double*)item_partial, seg_first_item, seg_group,
                       (const float*)table, ngroups, 1, found_inf, seg_stats);
    hipLaunchKernelGGL(lamb_apply_kernel, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0, s, p, (const float*)m, (const float*)v, n, seg_start,
                       seg_group, blk_seg, (const float*)table, ngroups, (const float*)state, (const float*)seg_stats, found_inf, shadow);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

}  // namespace bvc

// Gate on the two residual branches of a pre-LN layer: stochastic depth (one f32 per sample) and hidden dropout (one bit per element).
//   g(row, col) = path_scale[row / rows] * keep(row, col) / (1 - p)
// The element mask is never stored.  It comes from a counter-based generator (Philox4x32-10) that forward epilogue, backward row
// kernels, bvc_op_dropout_mask and its host twin all evaluate - the same __host__ __device__ code - so the backward regenerates what
// the forward applied.  Counter layout, for element e = row * N + col of branch `branch` (0 = attention, 1 = MLP) of layer `layer`:
//   counter = { low 32 bits of e / 4,  (e / 4) >> 32 | (2 layer + branch) << 8,  low / high 32 bits of the call offset },
//   key     = { low / high 32 bits of the seed };
// the four 32-bit outputs belong to elements 4 (e / 4) .. + 3, and an element is DROPPED when its output is below p * 2^32.
#pragma once
#include <stdint.h>

#include "common.h"

namespace bvc {

struct Gate {
    const float* path_scale;   // f32 [samples] of this (layer, branch): 0 or 1 / (1 - rate); nullptr = no stochastic depth
    int rows;                  // rows per sample
    uint32_t thr;              // drop threshold p * 2^32; 0 = no hidden dropout
    float inv_keep;            // 1 / (1 - p)
    uint32_t key0, key1, off0, off1;
    uint32_t stream;           // 2 layer + branch
};

__host__ __device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                                       uint32_t (&out)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1; c3 = (uint32_t)p0; c0 = n0; c2 = n2;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// the draws of elements 4 q .. 4 q + 3 of the gate's branch
__host__ __device__ __forceinline__ void gate_draws(const Gate& g, uint64_t q, uint32_t (&out)[4]) {
    philox4x32_10((uint32_t)q, (uint32_t)(q >> 32) | (g.stream << 8), g.off0, g.off1, g.key0, g.key1, out);
}

// v[0..3] (elements 4 q .. 4 q + 3 of physical row `row`) times the gate
__device__ __forceinline__ f32x4 gate_apply4(const Gate& g, int row, uint64_t q, f32x4 v) {
    if (g.path_scale) v = v * g.path_scale[row / g.rows];
    if (g.thr) {
        uint32_t r[4];
        gate_draws(g, q, r);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = r[e] >= g.thr ? v[e] * g.inv_keep : 0.f;
    }
    return v;
}

static inline uint32_t drop_threshold(float p) {
    const double t = (double)p * 4294967296.0;
    return t <= 0.0 ? 0u : t >= 4294967295.0 ? 4294967295u : (uint32_t)t;
}

// Gate of one branch from the public description (include/bvc.h bvc_branch_drop); scale = the [samples] row of that branch or nullptr
static inline Gate make_gate(float hidden_p, uint64_t seed, uint64_t offset, const float* scale, int rows, int layer, int branch) {
    Gate g;
    g.path_scale = scale;
    g.rows = rows > 0 ? rows : 1;
    g.thr = drop_threshold(hidden_p);
    g.inv_keep = hidden_p > 0.f ? 1.0f / (1.0f - hidden_p) : 1.0f;
    g.key0 = (uint32_t)seed; g.key1 = (uint32_t)(seed >> 32);
    g.off0 = (uint32_t)offset; g.off1 = (uint32_t)(offset >> 32);
    g.stream = (uint32_t)(2 * layer + branch);
    return g;
}

// Per-context state behind bvc_*_set_drop: armed by set_drop, taken by the next forward (active) and kept for its backward.
struct DropState {
    bool armed = false, active = false;
    float hidden_p = 0.f;
    uint64_t seed = 0, offset = 0;
    float* path_scale = nullptr;    // device f32 [nlayers][2][samples], owned by the context (capacity nlayers * 2 * max_samples)
    bool has_path = false;
    int samples = 0, rows = 0, nlayers = 0, max_samples = 0;
    Gate gate(int layer, int branch) const {
        return make_gate(hidden_p, seed, offset, has_path ? path_scale + ((size_t)layer * 2 + branch) * samples : nullptr, rows, layer, branch);
    }
};

}  // namespace bvc

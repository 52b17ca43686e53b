// Attention probabilities P = softmax(Q K^T scale) as a dense f32 [B][H][N][N] array, from what an attention forward leaves
// behind: qkv (layout of attention.hip) and lse (f32 [B*H][N], log2 units).  The flash kernels never hold P outside registers;
// this kernel writes it for the callers that want to look at it (output_attentions, HF:181-206 eager attention_probs).
//
//   P[q][k] = exp2(q.k * scale * log2 e - lse[q])       one product, one exponential, no running maximum, no reduction
//
// so every element depends on its own query row, its own key row and one lse entry: no atomics, no scratch, no LDS, no barrier,
// and the result is the same on every run.  It does not touch, include or share code with the tuned kernels of attention.hip.
//
// Orientation: S = Q K^T with v_mfma_f32_32x32x16_bf16, A = Q (row = query), B = K^T (column = key), the key-on-the-lane
// orientation of the dK / dV kernel.  The 32 x 32 f32 result has its column (key) on the lane and its rows (queries) in the 16
// registers, so one store instruction writes, for each lane half, 32 consecutive keys of one query row: a contiguous 128-byte
// segment.  Both operands are in the layout the MFMA wants as they sit in HBM - lane (r, h) holds 8 consecutive head dims of
// row r, 16 bytes - so they are read straight into registers by buffer loads (out-of-extent lanes read 0).
//
// Traffic per head at N = 1568: N^2 * 4 = 9.8 MB of stores to HBM against 0.4 MB of q and k read from it - but every 32-query
// wave re-reads its keys' fragments from L2 (nothing is shared through LDS), N / 32 * N * HD * 2 = 9.8 MB at HD = 64, so the L2
// traffic equals the stores.  The grid is sized for stores in flight, not for MFMA rate: one wave owns 32 query rows x up to
// kKeyChunk keys, four waves (128 query rows) per workgroup, (clip-head, 128-row tile, key chunk) flattened into blockIdx.x.
// N = 1568: 13 x 4 workgroups per head.  K
// fragments of the next 32 keys are loaded before the current tile's product and stores.  Q of a wave is read once.
//
// Head widths: 32, 64, 80, 88, 96, 128.  ceil(HD / 16) k-steps; 80 is five whole steps, 88 five and a half - the upper lane half
// of its last step holds zeros instead of the next head's columns, so 80 / 88 run in place on the unpadded array.
// Ragged N: query and key rows past N are clamped to row N - 1 of the SAME clip for the loads (nothing outside the clip is read,
// and a key never enters another key's column), and neither rows nor columns past N are stored.
#include <math.h>

#include "attention.h"

namespace bvc {

constexpr int kKeyChunk = 512;     // keys per wave: 16 tiles of 32, 64 KiB of stores

template <int HD>
__device__ __forceinline__ void load_frags(__amdgpu_buffer_rsrc_t rs, uint32_t row_off, int h, bf16x8 (&f)[(HD + 15) / 16]) {
#pragma unroll
    for (int st = 0; st < (HD + 15) / 16; ++st) {
        const int col = 16 * st + 8 * h;
        if (HD % 16 == 0 || col < HD) f[st] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rs, row_off + (uint32_t)col * 2u, 0, 0));
        else f[st] = bf16x8{0, 0, 0, 0, 0, 0, 0, 0};
    }
}

template <int HD>
__global__ __launch_bounds__(256) void attn_probs_kernel(const bf16_t* __restrict__ qkv, const float* __restrict__ lse,
                                                         float* __restrict__ probs, int N, int H, int qtiles, int kchunks,
                                                         float scale_log2, uint32_t qkv_bytes) {
    constexpr int NS = (HD + 15) / 16;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    int bid = blockIdx.x;
    const int kc = bid % kchunks;
    bid /= kchunks;
    const int qt = bid % qtiles;
    const int bh = bid / qtiles;
    const int b = bh / H, hh = bh - b * H;
    const int q0 = qt * 128 + wave * 32;
    if (q0 >= N) return;      // (wave-uniform; the kernel has no barrier)
    const int D = H * HD;
    const uint32_t pitch = (uint32_t)(3 * D) * 2u;      // bytes per qkv row
    const __amdgpu_buffer_rsrc_t rs = make_rsrc(qkv, qkv_bytes);
    const uint32_t clip = (uint32_t)b * (uint32_t)N;    // first row of the clip; every byte offset below is < qkv_bytes < 2^32

    bf16x8 qf[NS];
    load_frags<HD>(rs, (clip + (uint32_t)min(q0 + r, N - 1)) * pitch + (uint32_t)(hh * HD) * 2u, h, qf);
    // accumulator register `reg` of lane half h is query row q0 + (reg & 3) + 8 (reg >> 2) + 4 h
    float nl[16];
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int row = q0 + (reg & 3) + 8 * (reg >> 2) + 4 * h;
        nl[reg] = -lse[(size_t)bh * N + min(row, N - 1)];
    }
    const int key_end = min(N, (kc + 1) * kKeyChunk);
    int key0 = kc * kKeyChunk;
    const uint32_t kcol = (uint32_t)(D + hh * HD) * 2u;
    bf16x8 kf[NS], kn[NS];
    load_frags<HD>(rs, (clip + (uint32_t)min(key0 + r, N - 1)) * pitch + kcol, h, kf);
    float* const out = probs + ((size_t)bh * N + q0) * (size_t)N;      // row q0 of this head, 64-bit
    for (; key0 < key_end; key0 += 32) {
        const bool more = key0 + 32 < key_end;      // (wave-uniform)
        if (more) load_frags<HD>(rs, (clip + (uint32_t)min(key0 + 32 + r, N - 1)) * pitch + kcol, h, kn);
        f32x16 s;
#pragma unroll
        for (int i = 0; i < 16; ++i) s[i] = 0.f;
#pragma unroll
        for (int st = 0; st < NS; ++st) s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(qf[st], kf[st], s, 0, 0, 0);
        const int key = key0 + r;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int rr = (reg & 3) + 8 * (reg >> 2) + 4 * h;
            const float p = __builtin_amdgcn_exp2f(fmaf(s[reg], scale_log2, nl[reg]));
            if (key < N && q0 + rr < N) __builtin_nontemporal_store(p, out + (size_t)rr * N + key);
        }
        if (more) {
#pragma unroll
            for (int st = 0; st < NS; ++st) kf[st] = kn[st];
        }
    }
}

template <int HD>
static int probs_hd(const bf16_t* qkv, const float* lse, float* probs, int B, int N, int H, hipStream_t stream, float sm_scale) {
    const int qtiles = (N + 127) / 128, kchunks = (N + kKeyChunk - 1) / kKeyChunk;
    const size_t blocks = (size_t)B * H * qtiles * kchunks;
    BVC_REQUIRE(blocks < 0x7fffffffull, "attn_probs: %zu workgroups exceed the grid", blocks);
    const float scale_log2 = (sm_scale > 0.f ? sm_scale : 1.0f / sqrtf((float)HD)) * 1.4426950408889634f;
    const uint32_t qkv_bytes = (uint32_t)((size_t)B * N * 3 * H * HD * 2);
    attn_probs_kernel<HD><<<dim3((unsigned)blocks), dim3(256), 0, stream>>>(qkv, lse, probs, N, H, qtiles, kchunks, scale_log2, qkv_bytes);
    BVC_CHECK_HIP(hipGetLastError());
    return BVC_OK;
}

int launch_attn_probs(const bf16_t* qkv, const float* lse, float* probs, int B, int N, int H, int head_dim, hipStream_t stream,
                      float sm_scale) {
    BVC_REQUIRE(qkv && lse && probs, "attn_probs: null argument");
    BVC_REQUIRE(B > 0 && N > 0 && H > 0, "attn_probs: empty shape");
    BVC_REQUIRE(sm_scale >= 0.f, "attn_probs: negative softmax scale");
    BVC_REQUIRE((size_t)B * N * 3 * H * head_dim * 2 < 0xffffffffull, "attn_probs: qkv larger than 4 GiB");
    BVC_REQUIRE(((uintptr_t)qkv & 15) == 0, "attn_probs: qkv must be 16-byte aligned");
    switch (head_dim) {
        case 32: return probs_hd<32>(qkv, lse, probs, B, N, H, stream, sm_scale);
        case 64: return probs_hd<64>(qkv, lse, probs, B, N, H, stream, sm_scale);
        case 80: return probs_hd<80>(qkv, lse, probs, B, N, H, stream, sm_scale);
        case 88: return probs_hd<88>(qkv, lse, probs, B, N, H, stream, sm_scale);
        case 96: return probs_hd<96>(qkv, lse, probs, B, N, H, stream, sm_scale);
        case 128: return probs_hd<128>(qkv, lse, probs, B, N, H, stream, sm_scale);
        default: break;
    }
    BVC_REQUIRE(false, "attn_probs: head_dim %d unsupported (32, 64, 80, 88, 96 or 128)", head_dim);
}

}  // namespace bvc

// Prototype cross-entropy (DINO self-distillation) over f32 feature rows and two sets of prototype weights (csrc/proto_ce.hip),
// forward and backward.
#pragma once
#include "common.h"

namespace bvc {

constexpr int kPcMaxM = 32768;                       // rows
constexpr int kPcMaxK = 262144;                      // prototypes
constexpr int kPcMaxP = 8192;                        // feature width
constexpr int kPcMaxSplits = 2048;                   // prototype splits of the forward (one per prototype tile at the largest K)
constexpr int64_t kPcDsBlockBytes = 64ll << 20;      // cap of EACH of the backward's two dS blocks [m][block] f32 in the workspace

int proto_ce_splits(int m, int K, int p);
int proto_ce_block(int m, int K, int p);
int64_t proto_ce_workspace(int m, int K, int p, int splits, int block);
int launch_proto_ce_fwd(const float* xs, int64_t ldxs, const float* vs, int64_t ldvs, const float* xt, int64_t ldxt, const float* vt,
                        int64_t ldvt, const float* center, int m, int K, int p, float tau_s, float tau_t, float eps, int splits,
                        float* row_loss, float* lse_s, float* lse_t, float* stats2, float* batch_center, void* workspace, hipStream_t s);
int launch_proto_ce_bwd(const float* xs, int64_t ldxs, const float* vs, int64_t ldvs, const float* xt, int64_t ldxt, const float* vt,
                        int64_t ldvt, const float* center, int m, int K, int p, float tau_s, float tau_t, float eps, const float* lse_s,
                        const float* lse_t, const float* row_weight, int splits, int block, float* dxs, int64_t lddxs, float* dvs,
                        int64_t lddvs, void* workspace, hipStream_t s);

}  // namespace bvc

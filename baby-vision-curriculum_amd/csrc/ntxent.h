// NT-Xent / SupCon loss over f32 feature rows with integer group ids (csrc/ntxent.hip), forward and backward.
#pragma once
#include "common.h"

namespace bvc {

constexpr int kNxMaxN = 32768;                       // rows
constexpr int kNxMaxP = 8192;                        // feature width
constexpr int kNxMaxSplits = 256;                    // key splits of the forward
constexpr int64_t kNxEBlockBytes = 256ll << 20;      // cap of the backward's E block [block_rows][n] f32 in the workspace

int ntxent_splits(int n, int p);
int ntxent_block_rows(int n, int p);
int64_t ntxent_workspace(int n, int p, int key_splits, int block_rows);
int launch_ntxent_fwd(const float* f, int64_t ldf, const int32_t* groups, int views, int n, int p, float temperature, float eps,
                      int key_splits, float* row_loss, float* lse, int32_t* npos, float* stats2, void* workspace, hipStream_t s);
int launch_ntxent_bwd(const float* f, int64_t ldf, const int32_t* groups, int views, int n, int p, float temperature, float eps,
                      const float* lse, const int32_t* npos, const float* row_weight, int key_splits, int block_rows, float* df,
                      int64_t lddf, void* workspace, hipStream_t s);

}  // namespace bvc

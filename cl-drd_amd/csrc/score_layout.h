// The column layout of the N-way scorers (reference models/nway_dual_encoder.py:30-44): which passage is behind logit column j of row b.
//   mode 0: the row's own N passages;
//   mode 1: own N, then every other sample's passages in global order;
//   mode 2: own N, then the next sample's N (cyclic).
// The scorers (score.hip) and the duplicate-passage rule of softmax_ce (contrastive.hip) read it from here and nowhere else.
#pragma once
#include <hip/hip_runtime.h>

__host__ __device__ __forceinline__ int score_cols(int B, int N, int mode) { return mode == 0 ? N : (mode == 1 ? B * N : 2 * N); }

// row of p [B * N, d] (index into pids [B * N]) behind logit column j of row b
__host__ __device__ __forceinline__ int col_to_passage(int mode, int b, int j, int B, int N) {
    if (j < N) return b * N + j;
    const int jj = j - N;
    if (mode == 1) return jj < b * N ? jj : jj + N;
    return ((b + 1) % B) * N + jj;
}

// The inverse for the in-batch block, as the bwd_p kernels walk it.  mode 1: every row b but the owner scores passage m, at this column.
__host__ __device__ __forceinline__ int in_batch_col(int m, int b, int N) { return N + (m < b * N ? m : m - N); }
// mode 2: one other row scores the passages of row bo (passage bo * N + o at its column N + o): the row in front of it.
__host__ __device__ __forceinline__ int in_batch_prev_row(int bo, int B) { return (bo - 1 + B) % B; }

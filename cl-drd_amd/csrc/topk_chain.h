// The chained search of one shard (topk.hip: cldrd_flatip_chain), shared by the entry points of the three row modes
// (cldrd_flatip_search: fp32 / fp16 rows, topk.hip; cldrd_flatip_search_i8: int8 rows, topk_i8.hip).
#pragma once
#include <hip/hip_runtime.h>

// The rows of the shard.  R8 != nullptr: int8-row mode (R8, scale).  Else P16 is the scan's operand and the re-score reads P32, or - P32 == nullptr,
// fp16-row mode - P16 itself.
struct FlatipRows {
    const void* P16;
    const float* P32;
    const void* R8;
    const float* scale;
    long long rows;
};
// The queries, all [nq] / [nq, d] (qd: [2, nq, d]).  The scan's operand is qh (fp16 copy) or, in int8-row mode, the digit planes qd with their scale sq.
struct FlatipQueries {
    const float* q32;
    const void* qh;
    const void* qd;
    const float* sq;
    const float* thr;
    const float* eps;
    const double* qmu;
    int nq;
};
// Per tile of `qtile` queries, back to back on `st`: every row (exhaustive) or the scan (tiled: through the tiled fp16 kernels) -> select -> exact
// re-score -> sort + cut.  The callers have checked the arguments; buffers as cldrd_flatip_search documents them.
int cldrd_flatip_chain(const FlatipQueries& Q, const FlatipRows& P, int d, int k, int qtile, int* counts, int* cand_rows, float* cand_scores, int cap,
                       int* rows2, float* scores2, int cap2, int* n2, int* status, float* khat, float* D, int* I, int exhaustive, int tiled,
                       hipStream_t st);

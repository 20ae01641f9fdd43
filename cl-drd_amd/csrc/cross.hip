// Cross-encoder (teacher) scoring of (query, passage) pairs: pair assembly from token-cache rows and the classification head.
//
// A cross-encoder (HF BertForSequenceClassification / DistilBertForSequenceClassification) reads `[CLS] q' [SEP] p' [SEP]` with
// token types 0 up to and including the first [SEP], 1 after it.  The query and passage tables are tokenised once as single sequences
// (`[CLS] q [SEP]`, dataset TokenCache / SequenceTokenCache), so a pair is two slices of two cache rows: the host decides how many content
// tokens of each side survive the tokenizer's `longest_first` truncation (models/cross_encoder.py pair_lengths) and where each pair
// starts in the packed batch (cu); cldrd_build_pairs only moves tokens.  The encoder then runs on the packed rows as on any packed batch
// and cldrd_cls_head_fwd turns its fp32 CLS rows into logits.
#include "common.h"

namespace {

template <int BYTES>
__device__ __forceinline__ long long load_tok(const void* base, size_t i) {
    if (BYTES == 2) return (long long)((const uint16_t*)base)[i];
    return (long long)((const int32_t*)base)[i];
}

// One wave per pair.  Pair m = rows cu[m] .. cu[m + 1] of the packed batch; row j of it:
//   0: q[0] ([CLS]);  1 .. a: q[1 .. a];  a + 1: q[lq - 1] ([SEP]);  a + 2 .. a + 1 + b: p[1 .. b];  a + 2 + b: p[lp - 1] ([SEP]).
// A pair of a + 2 rows is the single sequence `[CLS] q' [SEP]` (empty passage text).  Every read index is clamped into its row.
template <int QB, int PB>
__global__ __launch_bounds__(256) void build_pairs_kernel(const void* __restrict__ q_tok, const int* __restrict__ q_lens, int q_stride,
                                                          const void* __restrict__ p_tok, const int* __restrict__ p_lens, int p_stride,
                                                          const int* __restrict__ q_rows, const int* __restrict__ p_rows,
                                                          const int* __restrict__ keep_q, const int* __restrict__ keep_p,
                                                          const int* __restrict__ cu, int n_pairs, long long* __restrict__ out_ids,
                                                          int* __restrict__ out_types, int* __restrict__ out_pos) {
    const int lane = threadIdx.x & 63;
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= n_pairs) return;
    const size_t qo = (size_t)q_rows[m] * q_stride, po = (size_t)p_rows[m] * p_stride;
    const int lq = min(max(q_lens[q_rows[m]], 1), q_stride), lp = min(max(p_lens[p_rows[m]], 1), p_stride);
    const int a = min(max(keep_q[m], 0), max(lq - 2, 0)), b = min(max(keep_p[m], 0), max(lp - 2, 0));
    const int c0 = cu[m], n = cu[m + 1] - c0;
    for (int j = lane; j < n; j += 64) {
        long long t;
        if (j <= a) t = load_tok<QB>(q_tok, qo + j);
        else if (j == a + 1) t = load_tok<QB>(q_tok, qo + lq - 1);
        else if (j < a + 2 + b) t = load_tok<PB>(p_tok, po + min(j - a - 1, p_stride - 1));
        else t = load_tok<PB>(p_tok, po + lp - 1);
        out_ids[c0 + j] = t;
        if (out_types) out_types[c0 + j] = j <= a + 1 ? 0 : 1;
        if (out_pos) out_pos[c0 + j] = j;
    }
}

__device__ __forceinline__ float wave_sum(float s) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    return s;
}

// One block per CLS row: h = act(W1 x + b1) in LDS, then logits = W2 h + b2.  One wave per output feature (lanes stride over the
// contiguous weight row, fixed-order butterfly sum: the result does not depend on M or on the launch).
template <int ACT>      // 0: tanh (BERT pooler), 1: ReLU (DistilBERT pre_classifier)
__global__ __launch_bounds__(256) void cls_head_kernel(const float* __restrict__ cls, const float* __restrict__ w1, const float* __restrict__ b1,
                                                       const float* __restrict__ w2, const float* __restrict__ b2, float* __restrict__ out,
                                                       int d, int nl) {
    __shared__ float x[1024], h[1024];
    const int m = blockIdx.x, lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    for (int k = threadIdx.x; k < d; k += 256) x[k] = cls[(size_t)m * d + k];
    __syncthreads();
    for (int j = w; j < d; j += 4) {
        const float* wr = w1 + (size_t)j * d;
        float s = 0.f;
        for (int k = lane; k < d; k += 64) s += wr[k] * x[k];
        s = wave_sum(s) + b1[j];
        if (lane == 0) h[j] = ACT == 0 ? tanhf(s) : fmaxf(s, 0.f);
    }
    __syncthreads();
    for (int l = w; l < nl; l += 4) {
        const float* wr = w2 + (size_t)l * d;
        float s = 0.f;
        for (int k = lane; k < d; k += 64) s += wr[k] * h[k];
        s = wave_sum(s) + b2[l];
        if (lane == 0) out[(size_t)m * nl + l] = s;
    }
}

}  // namespace

extern "C" int cldrd_build_pairs(const void* q_tok, const int* q_lens, int q_stride, int q_bytes, const void* p_tok, const int* p_lens,
                                 int p_stride, int p_bytes, const int* q_rows, const int* p_rows, const int* keep_q, const int* keep_p,
                                 const int* cu, int n_pairs, long long* out_ids, int* out_types, int* out_pos, void* stream) {
    CLDRD_CHECK(n_pairs > 0 && q_stride > 0 && p_stride > 0, "build_pairs: bad shape");
    CLDRD_CHECK((q_bytes == 2 || q_bytes == 4) && (p_bytes == 2 || p_bytes == 4), "build_pairs: token tables are uint16 or int32");
    CLDRD_CHECK(q_tok && q_lens && p_tok && p_lens && q_rows && p_rows && keep_q && keep_p && cu && out_ids, "build_pairs: null pointer");
    const dim3 grid((n_pairs + 3) / 4), block(256);
    const hipStream_t st = (hipStream_t)stream;
#define CLDRD_PAIRS(QB, PB) hipLaunchKernelGGL((build_pairs_kernel<QB, PB>), grid, block, 0, st, q_tok, q_lens, q_stride, p_tok, p_lens, p_stride, \
                                               q_rows, p_rows, keep_q, keep_p, cu, n_pairs, out_ids, out_types, out_pos)
    if (q_bytes == 2 && p_bytes == 2) CLDRD_PAIRS(2, 2);
    else if (q_bytes == 2) CLDRD_PAIRS(2, 4);
    else if (p_bytes == 2) CLDRD_PAIRS(4, 2);
    else CLDRD_PAIRS(4, 4);
#undef CLDRD_PAIRS
    CLDRD_LAUNCH_CHECK();
    return 0;
}

extern "C" int cldrd_cls_head_fwd(const float* cls, const float* w1, const float* b1, const float* w2, const float* b2, float* out, int M,
                                  int d, int num_labels, int act, void* stream) {
    CLDRD_CHECK(M > 0 && d > 0 && d <= 1024 && num_labels > 0, "cls_head_fwd: need M > 0, 0 < d <= 1024, num_labels > 0");
    CLDRD_CHECK(act == 0 || act == 1, "cls_head_fwd: act is 0 (tanh) or 1 (ReLU)");
    CLDRD_CHECK(cls && w1 && b1 && w2 && b2 && out, "cls_head_fwd: null pointer");
    if (act == 0) hipLaunchKernelGGL(cls_head_kernel<0>, dim3(M), dim3(256), 0, (hipStream_t)stream, cls, w1, b1, w2, b2, out, d, num_labels);
    else hipLaunchKernelGGL(cls_head_kernel<1>, dim3(M), dim3(256), 0, (hipStream_t)stream, cls, w1, b1, w2, b2, out, d, num_labels);
    CLDRD_LAUNCH_CHECK();
    return 0;
}

// Curriculum selection on the device (dataset/curriculum_file.py: select_examples): from a query's K candidates and their teacher scores,
// the teacher order, the top n_rel and the seeded samples of the most-hard / semi-hard rank windows - what the host path derives from a
// 100 M-line run file with a parse, two lexsorts and a gather per window.  The GPU already holds the search's ids and the teacher's scores
// as dense [queries, K] arrays; this kernel reads them once (12 bytes per candidate).
//
// One workgroup per query, everything about the query in LDS.  Nothing here is bandwidth or MFMA bound, so ranks are COUNTED, not sorted:
//   teacher rank of candidate i = #{j : s_j > s_i or (s_j == s_i and j < i)}     (score desc, ties by run position; -0.0 == 0.0)
//   key rank inside a window    = #{b : (key_b, pid_b, b) < (key_a, pid_a, a)}   (the stable lexsort((pid, key)) of the host path)
// K^2 / 256 compares per thread: 156 at K = 200, 4096 at the limit K = 1024; the inner loop reads one LDS word that every lane shares
// (a broadcast, no bank conflict).  A rank is a count over the other live candidates, so it is < count whatever the scores are: a score that
// breaks the finite-score precondition can leave `order` with repeated / unset (-1) entries but never an index outside the row.
#include "common.h"

namespace {

constexpr int CUR_MAX_K = 1024;
constexpr int CUR_THREADS = 256;

__host__ __device__ __forceinline__ uint64_t splitmix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

struct CurSpec {
    int n_rel, n_most, most_lo, most_hi, n_semi, semi_lo, semi_hi, min_candidates;
};

__global__ __launch_bounds__(CUR_THREADS) void curriculum_select_kernel(const long long* __restrict__ qid, const long long* __restrict__ pid,
                                                                        const float* __restrict__ score, const int* __restrict__ count, int K,
                                                                        CurSpec sp, uint64_t seed_key, int* __restrict__ order,
                                                                        int* __restrict__ keep, long long* __restrict__ sel_pid,
                                                                        float* __restrict__ sel_score) {
    __shared__ float s_score[CUR_MAX_K];
    __shared__ int s_order[CUR_MAX_K];
    __shared__ uint64_t s_key[CUR_MAX_K];
    __shared__ long long s_pid[CUR_MAX_K];
    __shared__ int s_pick[CUR_MAX_K];
    const int q = blockIdx.x, tid = threadIdx.x;
    const size_t row = (size_t)q * K;
    int c = count[q];
    c = c < 0 ? 0 : (c > K ? K : c);

    for (int i = tid; i < K; i += CUR_THREADS) {
        s_order[i] = -1;
        if (i < c) s_score[i] = score[row + i];
    }
    __syncthreads();
    for (int i = tid; i < c; i += CUR_THREADS) {
        const float si = s_score[i];
        int r = 0;
        for (int j = 0; j < c; ++j) {
            const float sj = s_score[j];
            r += (sj > si || (sj == si && j < i)) ? 1 : 0;
        }
        s_order[r] = i;           // r <= c - 1: inside the row
    }
    __syncthreads();
    for (int i = tid; i < K; i += CUR_THREADS) order[row + i] = i < c ? s_order[i] : -1;
    const bool kept = c >= sp.min_candidates;
    if (tid == 0) keep[q] = kept ? 1 : 0;
    if (!kept) return;            // (uniform over the workgroup) the row's sel_* stay as they were

    const int n_sel = sp.n_rel + sp.n_most + sp.n_semi;
    const size_t out = (size_t)q * n_sel;
    for (int t = tid; t < sp.n_rel; t += CUR_THREADS) {
        const int at = s_order[t];
        if (at < 0) continue;     // only with non-finite scores (precondition broken)
        sel_pid[out + t] = pid[row + at];
        sel_score[out + t] = s_score[at];
    }
    const uint64_t q_key = splitmix64(seed_key ^ (uint64_t)qid[q]);
    int base = sp.n_rel;
    for (int w = 0; w < 2; ++w) {
        const int n = w ? sp.n_semi : sp.n_most, lo = w ? sp.semi_lo : sp.most_lo, hi = w ? sp.semi_hi : sp.most_hi;
        if (n == 0) continue;
        const int W = hi - lo + 1;              // lo - 1 + W = hi <= min_candidates <= c: the window lies inside the live ranks
        __syncthreads();                        // the previous window's readers are done with s_key / s_pid / s_pick
        for (int a = tid; a < W; a += CUR_THREADS) {
            const int at = s_order[lo - 1 + a];
            const long long p = at < 0 ? 0 : pid[row + at];
            s_pid[a] = p;
            s_key[a] = splitmix64(q_key ^ (uint64_t)p);
        }
        __syncthreads();
        for (int a = tid; a < W; a += CUR_THREADS) {
            const uint64_t ka = s_key[a];
            const long long pa = s_pid[a];
            int r = 0;
            for (int b = 0; b < W; ++b) {
                const uint64_t kb = s_key[b];
                const long long pb = s_pid[b];
                r += (kb < ka || (kb == ka && (pb < pa || (pb == pa && b < a)))) ? 1 : 0;
            }
            s_pick[a] = r < n ? 1 : 0;          // exactly n of the W ranks 0 .. W - 1 are below n
        }
        __syncthreads();
        for (int a = tid; a < W; a += CUR_THREADS) {
            if (!s_pick[a]) continue;
            int pos = 0;                        // picked candidates in front of this one: its place in teacher order
            for (int b = 0; b < a; ++b) pos += s_pick[b];
            const int at = s_order[lo - 1 + a];
            sel_pid[out + base + pos] = s_pid[a];
            sel_score[out + base + pos] = at < 0 ? 0.f : s_score[at];
        }
        base += n;
    }
}

}  // namespace

extern "C" int cldrd_curriculum_select(const long long* qid, const long long* pid, const float* score, const int* count, int nq, int K,
                                       int n_rel, int n_most_hard, int most_lo, int most_hi, int n_semi_hard, int semi_lo, int semi_hi,
                                       unsigned long long seed, int* order, int* keep, long long* sel_pid, float* sel_score, void* stream) {
    CLDRD_CHECK(nq > 0 && K > 0, "curriculum_select: nq and K must be positive");
    CLDRD_CHECK(K <= CUR_MAX_K, "curriculum_select: K is at most 1024 (a longer list is selected on the host: dataset.curriculum_file.select_examples)");
    CLDRD_CHECK(qid && pid && score && count && order && keep && sel_pid && sel_score, "curriculum_select: null pointer");
    CLDRD_CHECK(n_rel >= 0 && n_most_hard >= 0 && n_semi_hard >= 0 && n_rel + n_most_hard + n_semi_hard > 0,
                "curriculum_select: counts must be non-negative and select at least one candidate");
    const int lo[2] = {most_lo, semi_lo}, hi[2] = {most_hi, semi_hi}, n[2] = {n_most_hard, n_semi_hard};
    int need = n_rel;
    for (int w = 0; w < 2; ++w) {
        if (n[w] == 0) continue;
        CLDRD_CHECK(lo[w] > n_rel && hi[w] >= lo[w] && hi[w] - lo[w] + 1 >= n[w],
                    "curriculum_select: a window starts after n_rel and holds at least the number drawn from it (1-based inclusive ranks)");
        need = hi[w] > need ? hi[w] : need;
    }
    CLDRD_CHECK(n[0] == 0 || n[1] == 0 || (lo[0] > hi[1] || lo[1] > hi[0]), "curriculum_select: the two windows overlap");
    const CurSpec sp{n_rel, n_most_hard, most_lo, most_hi, n_semi_hard, semi_lo, semi_hi, need};
    hipLaunchKernelGGL(curriculum_select_kernel, dim3(nq), dim3(CUR_THREADS), 0, (hipStream_t)stream, qid, pid, score, count, K, sp,
                       splitmix64((uint64_t)seed), order, keep, sel_pid, sel_score);
    CLDRD_LAUNCH_CHECK();
    return 0;
}

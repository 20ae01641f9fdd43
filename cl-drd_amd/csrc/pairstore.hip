// Teacher score store on the device (retriever/score_store.py): a SEGMENT is three parallel arrays (qid int64, pid int64, score fp32)
// whose entries are strictly ascending in the key (qid, pid) - lexicographic, qid major, signed 64-bit compares throughout.
//
//   pair_lookup  the pairs of a CSR batch (qid[nq], starts[nq + 1], pid[total]) searched in one segment.  One workgroup per query row:
//                the row's range [lo, hi) of its qid in seg_q is found ONCE (a lower bound over the segment, then a gallop for the end of
//                the run - a run is a query's candidates, a few hundred entries), then every lane binary-searches its pid inside that
//                range.  A flat one-thread-per-pair search over 1e8 entries is ~27 dependent loads per pair, most of them HBM misses
//                (~900 cycles each); here a pair pays ~8 steps inside a range of a few KiB that the row's first lanes pulled into L2,
//                and the upper levels of the qid search are shared by every workgroup.
//   pair_merge   two segments with no common key merged into one: a merge-path partition per output tile of 2048 entries (two
//                binary searches over the inputs per workgroup), the tile's inputs staged in LDS, a second partition per thread in LDS,
//                8 entries merged sequentially per thread, the tile written back coalesced.  Two neighbouring output entries with the
//                same key can only come from different inputs (each input is strictly ascending): that raises the flag.
#include "common.h"

namespace {

constexpr int PS_THREADS = 256;
constexpr int PS_ITEMS = 8;                         // entries merged per thread
constexpr int PS_TILE = PS_THREADS * PS_ITEMS;      // output entries per workgroup
constexpr long long PS_MAX_N = 2147483647ll;        // entries per segment: 2^31 - 1

// (aq, ap) <= (bq, bp)
__device__ __forceinline__ bool key_le(long long aq, long long ap, long long bq, long long bp) { return aq < bq || (aq == bq && ap <= bp); }

__global__ __launch_bounds__(PS_THREADS) void pair_lookup_kernel(const long long* __restrict__ seg_q, const long long* __restrict__ seg_p,
                                                                 const float* __restrict__ seg_s, long long n,
                                                                 const long long* __restrict__ qid, const long long* __restrict__ starts,
                                                                 const long long* __restrict__ pid, long long total,
                                                                 float* __restrict__ score_out, unsigned char* __restrict__ hit) {
    __shared__ long long s_range[2];
    const long long row = blockIdx.x;
    long long a = starts[row], b = starts[row + 1];
    a = a < 0 ? 0 : (a > total ? total : a);        // a malformed starts[] never reaches outside pid / score_out / hit
    b = b < a ? a : (b > total ? total : b);
    if (a == b) return;                             // (uniform over the workgroup) an empty row
    if (threadIdx.x == 0) {
        const long long q = qid[row];
        long long lo = 0, hi = n;                   // first entry with seg_q >= q
        while (lo < hi) {
            const long long mid = lo + ((hi - lo) >> 1);
            if (seg_q[mid] < q) lo = mid + 1; else hi = mid;
        }
        long long end = lo;
        if (lo < n && seg_q[lo] == q) {             // gallop to the end of the run: first entry with seg_q > q
            long long step = 1, last = lo;          // seg_q[last] == q
            while (last + step < n && seg_q[last + step] == q) { last += step; step <<= 1; }
            long long l = last + 1, h = last + step < n ? last + step : n;      // seg_q[h] > q or h == n
            while (l < h) {
                const long long mid = l + ((h - l) >> 1);
                if (seg_q[mid] == q) l = mid + 1; else h = mid;
            }
            end = l;
        }
        s_range[0] = lo;
        s_range[1] = end;
    }
    __syncthreads();
    const long long r0 = s_range[0], r1 = s_range[1];
    if (r0 == r1) return;                           // the segment does not hold this query
    for (long long i = a + threadIdx.x; i < b; i += PS_THREADS) {
        const long long p = pid[i];
        long long lo = r0, hi = r1;
        while (lo < hi) {
            const long long mid = lo + ((hi - lo) >> 1);
            if (seg_p[mid] < p) lo = mid + 1; else hi = mid;
        }
        if (lo < r1 && seg_p[lo] == p) {
            score_out[i] = seg_s[lo];
            hit[i] = 1;
        }
    }
}

// number of a's entries among the first d entries of the merge (an a entry goes first on equal keys); 0 <= d <= na + nb
template <typename Q, typename P>
__device__ __forceinline__ long long merge_path(Q aq, P ap, long long na, Q bq, P bp, long long nb, long long d) {
    long long lo = d > nb ? d - nb : 0, hi = d < na ? d : na;
    while (lo < hi) {
        const long long mid = lo + ((hi - lo) >> 1);            // lo <= mid < hi: 0 <= d - 1 - mid <= nb - 1
        if (key_le(aq[mid], ap[mid], bq[d - 1 - mid], bp[d - 1 - mid])) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(PS_THREADS) void pair_merge_kernel(const long long* __restrict__ a_q, const long long* __restrict__ a_p,
                                                                const float* __restrict__ a_s, long long na,
                                                                const long long* __restrict__ b_q, const long long* __restrict__ b_p,
                                                                const float* __restrict__ b_s, long long nb, long long* __restrict__ o_q,
                                                                long long* __restrict__ o_p, float* __restrict__ o_s, int* __restrict__ dup) {
    __shared__ long long s_q[PS_TILE];
    __shared__ long long s_p[PS_TILE];
    __shared__ float s_s[PS_TILE];
    __shared__ long long s_cut[2];
    const int tid = threadIdx.x;
    const long long N = na + nb;
    const long long d0 = (long long)blockIdx.x * PS_TILE;
    const long long d1 = d0 + PS_TILE < N ? d0 + PS_TILE : N;
    if (tid < 2) s_cut[tid] = merge_path(a_q, a_p, na, b_q, b_p, nb, tid ? d1 : d0);
    __syncthreads();
    const long long a0 = s_cut[0], b0 = d0 - a0;
    const int cnt = (int)(d1 - d0);
    // sorted inputs give a0 <= a1 <= a0 + cnt; the clamp keeps every index below inside a and b whatever the inputs hold
    // (a0 + ca <= na and b0 + cb = d1 - (a0 + ca) <= nb follow from the bounds merge_path starts from)
    const long long span = s_cut[1] - a0;
    const int ca = (int)(span < 0 ? 0 : (span > cnt ? cnt : span)), cb = cnt - ca;     // ca + cb = cnt <= PS_TILE
    for (int i = tid; i < cnt; i += PS_THREADS) {                               // a's part of the tile, then b's
        const bool from_a = i < ca;
        const long long at = from_a ? a0 + i : b0 + (i - ca);
        s_q[i] = from_a ? a_q[at] : b_q[at];
        s_p[i] = from_a ? a_p[at] : b_p[at];
        s_s[i] = from_a ? a_s[at] : b_s[at];
    }
    __syncthreads();
    const int ld = tid * PS_ITEMS < cnt ? tid * PS_ITEMS : cnt;                 // this thread's first output entry inside the tile
    int ai = (int)merge_path(s_q, s_p, (long long)ca, s_q + ca, s_p + ca, (long long)cb, (long long)ld);
    int bi = ca + (ld - ai);
    long long rq[PS_ITEMS], rp[PS_ITEMS];
    float rs[PS_ITEMS];
#pragma unroll
    for (int k = 0; k < PS_ITEMS; ++k) {
        if (ld + k < cnt) {                                                     // then ai < ca or bi < cnt
            const bool take_a = bi >= cnt || (ai < ca && key_le(s_q[ai], s_p[ai], s_q[bi], s_p[bi]));
            const int at = take_a ? ai : bi;
            rq[k] = s_q[at];
            rp[k] = s_p[at];
            rs[k] = s_s[at];
            ai += take_a ? 1 : 0;
            bi += take_a ? 0 : 1;
        }
    }
    __syncthreads();                                                            // every thread has read its inputs: LDS becomes the output tile
#pragma unroll
    for (int k = 0; k < PS_ITEMS; ++k) {
        if (ld + k < cnt) {
            s_q[ld + k] = rq[k];
            s_p[ld + k] = rp[k];
            s_s[ld + k] = rs[k];
        }
    }
    __syncthreads();
    bool same = false;
    for (int i = tid; i < cnt; i += PS_THREADS) {
        const long long q = s_q[i], p = s_p[i];
        o_q[d0 + i] = q;
        o_p[d0 + i] = p;
        o_s[d0 + i] = s_s[i];
        if (i > 0) {
            same |= q == s_q[i - 1] && p == s_p[i - 1];
        } else {                                                                // the entry in front of the tile is the larger of these two
            if (a0 > 0) same |= q == a_q[a0 - 1] && p == a_p[a0 - 1];
            if (b0 > 0) same |= q == b_q[b0 - 1] && p == b_p[b0 - 1];
        }
    }
    if (same) dup[0] = 1;
}

}  // namespace

extern "C" int cldrd_pair_lookup(const long long* seg_q, const long long* seg_p, const float* seg_s, long long n, const long long* qid,
                                 const long long* starts, const long long* pid, long long nq, long long total, float* score_out,
                                 unsigned char* hit, void* stream) {
    CLDRD_CHECK(seg_q && seg_p && seg_s && qid && starts && pid && score_out && hit, "pair_lookup: null pointer");
    CLDRD_CHECK(n >= 1 && n <= PS_MAX_N, "pair_lookup: a segment holds 1 .. 2^31 - 1 entries (the caller skips an empty one)");
    CLDRD_CHECK(nq >= 1 && nq <= PS_MAX_N, "pair_lookup: nq must be 1 .. 2^31 - 1 (a batch without queries is the caller's no-op)");
    CLDRD_CHECK(total >= 0, "pair_lookup: total must not be negative");
    hipLaunchKernelGGL(pair_lookup_kernel, dim3((unsigned)nq), dim3(PS_THREADS), 0, (hipStream_t)stream, seg_q, seg_p, seg_s, n, qid, starts,
                       pid, total, score_out, hit);
    CLDRD_LAUNCH_CHECK();
    return 0;
}

extern "C" int cldrd_pair_merge(const long long* a_q, const long long* a_p, const float* a_s, long long na, const long long* b_q,
                                const long long* b_p, const float* b_s, long long nb, long long* out_q, long long* out_p, float* out_s,
                                int* dup_flag, void* stream) {
    CLDRD_CHECK(a_q && a_p && a_s && b_q && b_p && b_s && out_q && out_p && out_s && dup_flag, "pair_merge: null pointer");
    CLDRD_CHECK(na >= 1 && nb >= 1, "pair_merge: na and nb are at least 1 (with an empty side the result is the other side: the caller's copy)");
    CLDRD_CHECK(na <= PS_MAX_N && nb <= PS_MAX_N && na + nb <= PS_MAX_N, "pair_merge: a segment holds at most 2^31 - 1 entries (na + nb)");
    const long long N = na + nb;
    hipLaunchKernelGGL(pair_merge_kernel, dim3((unsigned)((N + PS_TILE - 1) / PS_TILE)), dim3(PS_THREADS), 0, (hipStream_t)stream, a_q, a_p,
                       a_s, na, b_q, b_p, b_s, nb, out_q, out_p, out_s, dup_flag);
    CLDRD_LAUNCH_CHECK();
    return 0;
}

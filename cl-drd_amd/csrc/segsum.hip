// Deterministic scatter-add of rows: an inverted index of the keys (cldrd_key_order) and a per-key sum of the contribution rows in a fixed
// order (cldrd_segment_sum_rows).  The deterministic mode of the embedding backward: cldrd_embed_ln_bwd_rows stores one fp32 row per token,
// the two kernels here turn the rows into the word / position table gradients without a float atomic - the same bits on every run.
//
// key_order: a stable LSD radix sort of (key, row) by 8-bit digits, then the CSR starts by binary search in the sorted keys.  Per pass:
//   hist     one wave per tile of 1024 consecutive entries counts its digits (LDS integer atomics: a count does not depend on order)
//   scan     exclusive scan of hist[digit][tile] (digit-major: the start of every (digit, tile) run in the output)
//   scatter  the same wave walks its tile 64 entries at a time IN ORDER; the rank of an entry among the earlier entries of its digit is
//            a ballot match inside the step plus a running count per digit - positions never come from an atomic
// The number of passes depends on n_keys alone (ceil(bits(n_keys - 1) / 8), at least 1), so the launch sequence is fixed for a graph.
#include "common.h"
#include "../../include/cldrd_hip.h"

namespace {

constexpr int SEG_C = CLDRD_SEGMENT_CHUNK;
static_assert(SEG_C == 64, "a chunk's row indices are one wave-wide load (lane j holds entry j)");

constexpr int RADIX_BITS = 8, RADIX = 1 << RADIX_BITS;
constexpr int SORT_TILE = 1024;          // entries per wave: 16 steps of 64

__device__ __forceinline__ int clamp_key(long long k, int n_keys) { return k < 0 ? 0 : (k >= n_keys ? n_keys - 1 : (int)k); }

// entry i of the pass input: the first pass reads the caller's int64 keys (clamped) and numbers the rows itself
__device__ __forceinline__ void sort_entry(const long long* __restrict__ keys64, const int* __restrict__ kin, const int* __restrict__ vin, int i,
                                           int n_keys, int& key, int& val) {
    if (keys64) { key = clamp_key(keys64[i], n_keys); val = i; }
    else { key = kin[i]; val = vin[i]; }
}

__global__ __launch_bounds__(64) void radix_hist_kernel(const long long* __restrict__ keys64, const int* __restrict__ kin, int T, int n_keys,
                                                        int shift, int* __restrict__ hist, int ntiles) {
    __shared__ int cnt[RADIX];
    const int lane = threadIdx.x, tile = blockIdx.x;
    for (int i = lane; i < RADIX; i += 64) cnt[i] = 0;
    __syncthreads();
    const int lo = tile * SORT_TILE, hi = min(T, lo + SORT_TILE);
    for (int i = lo + lane; i < hi; i += 64) {
        const int key = keys64 ? clamp_key(keys64[i], n_keys) : kin[i];
        atomicAdd(&cnt[(key >> shift) & (RADIX - 1)], 1);
    }
    __syncthreads();
    for (int i = lane; i < RADIX; i += 64) hist[(size_t)i * ntiles + tile] = cnt[i];
}

// in-place exclusive scan of n ints by one workgroup: thread t owns the contiguous piece [t * per, (t + 1) * per)
__global__ __launch_bounds__(1024) void scan_kernel(int* __restrict__ a, int n) {
    __shared__ int part[1024];
    const int t = threadIdx.x, per = (n + 1023) / 1024;
    const int lo = min(n, t * per), hi = min(n, lo + per);
    int s = 0;
    for (int i = lo; i < hi; ++i) s += a[i];
    part[t] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) {          // Hillis-Steele inclusive scan of the 1024 piece sums
        const int v = t >= o ? part[t - o] : 0;
        __syncthreads();
        part[t] += v;
        __syncthreads();
    }
    int run = part[t] - s;
    for (int i = lo; i < hi; ++i) { const int v = a[i]; a[i] = run; run += v; }
}

__global__ __launch_bounds__(64) void radix_scatter_kernel(const long long* __restrict__ keys64, const int* __restrict__ kin,
                                                           const int* __restrict__ vin, int T, int n_keys, int shift,
                                                           const int* __restrict__ hist, int ntiles, int* __restrict__ kout, int* __restrict__ vout) {
    __shared__ int base[RADIX];          // next output position of each digit for this tile
    const int lane = threadIdx.x, tile = blockIdx.x;
    for (int i = lane; i < RADIX; i += 64) base[i] = hist[(size_t)i * ntiles + tile];
    __syncthreads();
    const int lo = tile * SORT_TILE, hi = min(T, lo + SORT_TILE);
    const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    for (int s = lo; s < hi; s += 64) {
        const int i = s + lane;
        const bool live = i < hi;
        int key = 0, val = 0;
        if (live) sort_entry(keys64, kin, vin, i, n_keys, key, val);
        const int dg = (key >> shift) & (RADIX - 1);
        unsigned long long peers = __ballot(live);          // lanes of this step with my digit
#pragma unroll
        for (int b = 0; b < RADIX_BITS; ++b) {
            const unsigned long long m = __ballot((dg >> b) & 1);
            peers &= ((dg >> b) & 1) ? m : ~m;
        }
        const int rank = __popcll(peers & below), n = __popcll(peers);
        int p = 0;
        if (live) p = base[dg] + rank;
        __syncthreads();
        if (live && rank == n - 1) base[dg] = p + 1;          // the last peer moves the digit's cursor past the step
        __syncthreads();
        if (live && p >= 0 && p < T) { kout[p] = key; vout[p] = val; }
    }
}

// offsets[k] = number of sorted keys below k = lower bound of k, k = 0 .. n_keys
__global__ __launch_bounds__(256) void csr_offsets_kernel(const int* __restrict__ sorted, int T, int n_keys, int* __restrict__ offsets) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k > n_keys) return;
    int lo = 0, hi = T;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (sorted[mid] < k) lo = mid + 1; else hi = mid;
    }
    offsets[k] = lo;
}

// ---- per-key sums ---------------------------------------------------------------------------------------------------------------------
// One wave sums one chunk: SEG_C = 64 consecutive list entries, left to right, 4 columns per lane (a 256-column slice of the row per wave;
// blockIdx.y walks the slices of d).  The row numbers of a chunk are one coalesced load, lane j holding entry j, handed round by shuffles;
// the row loads themselves are independent, so eight are in flight per lane while the adds keep their order.
struct ListRef {           // list of key k: entries i = 0 .. n - 1
    const int* order;      // row of entry i = order[start + i]; null: the strided form, row = start + i * stride
    int start, n, stride;
};
__device__ __forceinline__ float4 chunk_sum(const float* __restrict__ rows, int T, int d, int c, const ListRef& L, int e0, int lane) {
    const int n = min(SEG_C, L.n - e0);
    int mine = 0;
    if (lane < n) mine = L.order ? L.order[L.start + e0 + lane] : L.start + (e0 + lane) * L.stride;
    mine = min(max(mine, 0), T - 1);
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    const bool on = c < d;
    int i = 0;
    for (; i + 8 <= n; i += 8) {
        float4 v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int r = __shfl(mine, i + u, 64);
            v[u] = on ? *(const float4*)(rows + (size_t)r * d + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            if (i + u == 0) s = v[u];
            else { s.x += v[u].x; s.y += v[u].y; s.z += v[u].z; s.w += v[u].w; }
        }
    }
    for (; i < n; ++i) {
        const int r = __shfl(mine, i, 64);
        const float4 v = on ? *(const float4*)(rows + (size_t)r * d + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        if (i == 0) s = v;
        else { s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w; }
    }
    return s;
}

constexpr int SEG_WAVES = 16;
// A workgroup of 16 waves owns `kpb` consecutive keys.  A key of one chunk is one wave's work (wave w takes keys w, w + 16, ... of the group).
// A longer list is taken by all 16 waves together, 16 chunks per round: the chunk sums meet in LDS and wave 0 adds them onto the running
// sum in chunk order - so a hot key ([PAD]: half the rows of a padded batch; [CLS] / [SEP]: one row per sequence) is spread over
// 16 waves x d / 256 workgroups instead of running down one wave.  Every branch on the list length is uniform across the workgroup.
__global__ __launch_bounds__(1024) void segment_sum_kernel(const float* __restrict__ rows, const int* __restrict__ order,
                                                           const int* __restrict__ offsets, int T, int d, int n_keys, int kpb,
                                                           float* __restrict__ out, int accumulate) {
    __shared__ float4 part[SEG_WAVES][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int c = blockIdx.y * 256 + lane * 4;
    const int k0 = blockIdx.x * kpb, k1 = min(n_keys, k0 + kpb);
    auto list_of = [&](int k) {
        ListRef L;
        L.order = order;
        if (order) {
            const int a = min(max(offsets[k], 0), T), b = min(max(offsets[k + 1], a), T);
            L.start = a; L.n = b - a; L.stride = 0;
        } else {
            L.start = k; L.n = k < T ? (T - k + n_keys - 1) / n_keys : 0; L.stride = n_keys;
        }
        return L;
    };
    auto store = [&](int k, const float4& s) {
        if (c >= d) return;
        float4* o = (float4*)(out + (size_t)k * d + c);
        if (accumulate) { const float4 p = *o; *o = make_float4(p.x + s.x, p.y + s.y, p.z + s.z, p.w + s.w); }
        else *o = s;
    };
    for (int k = k0 + w; k < k1; k += SEG_WAVES) {          // single-chunk keys: one wave each
        const ListRef L = list_of(k);
        if (L.n < 1 || L.n > SEG_C) continue;
        store(k, chunk_sum(rows, T, d, c, L, 0, lane));
    }
    for (int k = k0; k < k1; ++k) {                          // longer lists: the whole workgroup, key after key
        const ListRef L = list_of(k);
        if (L.n <= SEG_C) continue;
        const int nchunks = (L.n + SEG_C - 1) / SEG_C;
        float4 total = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int b = 0; b < nchunks; b += SEG_WAVES) {
            if (b + w < nchunks) part[w][lane] = chunk_sum(rows, T, d, c, L, (b + w) * SEG_C, lane);
            __syncthreads();
            if (w == 0) {
                const int m = min(SEG_WAVES, nchunks - b);
                for (int j = 0; j < m; ++j) {
                    const float4 v = part[j][lane];
                    if (b + j == 0) total = v;
                    else { total.x += v.x; total.y += v.y; total.z += v.z; total.w += v.w; }
                }
            }
            __syncthreads();
        }
        if (w == 0) store(k, total);
    }
}

inline int key_passes(int n_keys) {
    int bits = 0;
    while (bits < 31 && (1 << bits) < n_keys) ++bits;
    const int p = (bits + RADIX_BITS - 1) / RADIX_BITS;
    return p < 1 ? 1 : p;
}
inline size_t key_order_ints(int T) { return 3 * (size_t)T + (size_t)RADIX * ((T + SORT_TILE - 1) / SORT_TILE); }

}  // namespace

extern "C" size_t cldrd_key_order_workspace(int T, int n_keys) {
    if (T <= 0 || n_keys <= 0 || T > (1 << 22) || n_keys > (1 << 20)) return 0;
    return key_order_ints(T) * sizeof(int);
}

extern "C" int cldrd_key_order(const long long* keys, int T, int n_keys, int* order, int* offsets, void* workspace, size_t workspace_bytes,
                               void* stream) {
    CLDRD_CHECK(T > 0 && T <= (1 << 22), "key_order: need 0 < T <= 2^22");
    CLDRD_CHECK(n_keys > 0 && n_keys <= (1 << 20), "key_order: need 0 < n_keys <= 2^20");
    CLDRD_CHECK(keys != nullptr && order != nullptr && offsets != nullptr, "key_order: null keys, order or offsets");
    CLDRD_CHECK(workspace != nullptr && workspace_bytes >= key_order_ints(T) * sizeof(int), "key_order: workspace smaller than key_order_workspace(T, n_keys)");
    hipStream_t st = (hipStream_t)stream;
    const int ntiles = (T + SORT_TILE - 1) / SORT_TILE, passes = key_passes(n_keys);
    int* kbuf[2] = {(int*)workspace, (int*)workspace + T};
    int* vtmp = (int*)workspace + 2 * (size_t)T;
    int* hist = (int*)workspace + 3 * (size_t)T;
    const int* kin = nullptr;
    const int* vin = nullptr;
    for (int p = 0; p < passes; ++p) {
        const long long* k64 = p == 0 ? keys : nullptr;
        int* kout = kbuf[p & 1];
        int* vout = ((passes - 1 - p) & 1) ? vtmp : order;          // the last pass lands in `order`
        hipLaunchKernelGGL(radix_hist_kernel, dim3(ntiles), dim3(64), 0, st, k64, kin, T, n_keys, p * RADIX_BITS, hist, ntiles);
        CLDRD_LAUNCH_CHECK();
        hipLaunchKernelGGL(scan_kernel, dim3(1), dim3(1024), 0, st, hist, RADIX * ntiles);
        CLDRD_LAUNCH_CHECK();
        hipLaunchKernelGGL(radix_scatter_kernel, dim3(ntiles), dim3(64), 0, st, k64, kin, vin, T, n_keys, p * RADIX_BITS, (const int*)hist, ntiles, kout, vout);
        CLDRD_LAUNCH_CHECK();
        kin = kout; vin = vout;
    }
    hipLaunchKernelGGL(csr_offsets_kernel, dim3((n_keys + 1 + 255) / 256), dim3(256), 0, st, kin, T, n_keys, offsets);
    CLDRD_LAUNCH_CHECK();
    return 0;
}

extern "C" int cldrd_segment_sum_rows(const float* rows, const int* order, const int* offsets, int T, int d, int n_keys, float* out, int accumulate,
                                      void* stream) {
    CLDRD_CHECK(T > 0, "segment_sum_rows: need T > 0");
    CLDRD_CHECK(n_keys > 0, "segment_sum_rows: need n_keys > 0");
    CLDRD_CHECK(d > 0 && d <= 1024 && d % 4 == 0, "segment_sum_rows: need 0 < d <= 1024, d % 4 == 0");
    CLDRD_CHECK(rows != nullptr && out != nullptr, "segment_sum_rows: null rows or out");
    CLDRD_CHECK((order == nullptr) == (offsets == nullptr), "segment_sum_rows: order and offsets go together (both null: the strided form)");
    // keys per workgroup, from the shape alone (the grid of a captured graph must not depend on the data): where the mean list is a
    // chunk or more (the position table of a padded batch) every key is taken by a whole workgroup, else 16 keys share one
    const int kpb = (long long)T >= (long long)n_keys * SEG_C ? 1 : SEG_WAVES;
    hipLaunchKernelGGL(segment_sum_kernel, dim3((n_keys + kpb - 1) / kpb, (d + 255) / 256), dim3(SEG_WAVES * 64), 0, (hipStream_t)stream, rows, order,
                       offsets, T, d, n_keys, kpb, out, accumulate);
    CLDRD_LAUNCH_CHECK();
    return 0;
}

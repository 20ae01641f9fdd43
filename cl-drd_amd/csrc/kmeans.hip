// k-means of embedding rows on the device (cldrd_amd/cluster.py; topic-aware batches cluster the query embeddings once before training).
// The definition of what is computed stands in include/cldrd_hip.h; this file is the schedule.
//
// cldrd_kmeans_assign   nearest centroid of every point, ONE launch, the [n, k] score matrix never leaves the registers.  The arithmetic is the
//   f32-input MFMA (v_mfma_f32_32x32x2_f32: bit for bit a k-ordered fmaf chain) in the tile shape of gemm_nt_f32_kernel: 128 x 128 x 32, 4 waves,
//   each 2 x 2 tiles of 32 x 32, operands global -> registers -> LDS (rows padded to 36 floats), the next K tile's loads issued before the current
//   tile's MFMAs.  A workgroup owns 128 POINTS and walks ALL centroid tiles in ascending order (the X block is re-streamed per centroid tile,
//   as a GEMM would: at d = 768 it is 393 KB).  It computes S^T = C_tile . X_tile^T: centroids in the accumulator rows, a point on a lane (the
//   attention kernels' "lane owns one query column"), so the running (best, index) of a point is a scan over the lane's own registers:
//     a lane meets its centroids in ascending index (tiles ascending, tile halves ascending, accumulator rows ascending), and a strict `>`
//     keeps the lowest index of equal scores;
//     after the last tile the two lane halves of a wave, then the two waves that share a point, are combined by (higher score, then lower index):
//     one shuffle, one pass through LDS.  No cross-workgroup reduction, no atomic.
//   One schedule for every n and k: assign[i] / best[i] are a function of row i and of C only.  Chain order of a dot product, the same for every
//   (i, j): K tiles ascending; inside a tile step (q, u), q = 0..3, u = 0..3, adds t = 4 q + u and then t = 16 + 4 q + u.  Rows >= n and centroid
//   rows >= k are read as zeros; such a centroid never enters the scan and such a point is never stored.
// cldrd_kmeans_half_sqnorm / cldrd_kmeans_finish   one wave per centroid row; the fp64 sum of squares adds a lane's columns lane, lane + 64, ...
//   in ascending order and the 64 lane sums by a butterfly: a fixed order.  The count of empty clusters is a second single-workgroup launch
//   (integer sums in a fixed tree), so nothing needs zeroing first.
#include "attention_common.h"      // mfma_drain
#include <climits>
#include <cstdio>

namespace {

constexpr int KT = 128;          // points per workgroup / centroids per tile
constexpr int KK = 32;           // K tile
constexpr int KLD = 36;          // LDS row pitch in floats

__global__ __launch_bounds__(256) void kmeans_assign_kernel(const float* __restrict__ X, int ldx, int n, int d, const float* __restrict__ Cn,
                                                             const float* __restrict__ hsq, int k, long long* __restrict__ assign,
                                                             float* __restrict__ best) {
    __shared__ __attribute__((aligned(16))) float Cs[KT * KLD];
    __shared__ __attribute__((aligned(16))) float Xs[KT * KLD];
    __shared__ float Hs[KT];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.x * KT;
    const int wc = (wave >> 1) * 64, wp = (wave & 1) * 64;          // the wave's centroid rows / points inside the tile
    const int r = lane & 31, h = lane >> 5;
    float4 gc[4], gx[4];
    // global -> register staging: float4 number idx = tid + 256 i of a [128][32] tile: row idx >> 3, columns 4 (idx & 7) ..
    auto fetch = [&](int c0, int k0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = tid + 256 * i, row = idx >> 3, c = (idx & 7) * 4;
            gc[i] = (c0 + row < k) ? *(const float4*)(Cn + (size_t)(c0 + row) * d + k0 + c) : make_float4(0.f, 0.f, 0.f, 0.f);
            gx[i] = (m0 + row < n) ? *(const float4*)(X + (size_t)(m0 + row) * ldx + k0 + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    float bs[2] = {-INFINITY, -INFINITY};          // running best of points wp + r and wp + 32 + r over this lane's centroid rows
    int bj[2] = {INT_MAX, INT_MAX};
    for (int c0 = 0; c0 < k; c0 += KT) {
        f32x16 acc[2][2];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;
        fetch(c0, 0);
        for (int k0 = 0; k0 < d; k0 += KK) {
            __syncthreads();                    // the previous tile's reads (and the previous centroid tile's reads of Hs) are done
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int idx = tid + 256 * i, row = idx >> 3, c = (idx & 7) * 4;
                *(float4*)(Cs + row * KLD + c) = gc[i];
                *(float4*)(Xs + row * KLD + c) = gx[i];
            }
            if (k0 == 0 && tid < KT) Hs[tid] = c0 + tid < k ? hsq[c0 + tid] : 0.f;
            __syncthreads();
            if (k0 + KK < d) fetch(c0, k0 + KK);
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                float4 a[2], w[2];
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    a[t] = *(const float4*)(Cs + (wc + 32 * t + r) * KLD + 16 * h + 4 * q);
                    w[t] = *(const float4*)(Xs + (wp + 32 * t + r) * KLD + 16 * h + 4 * q);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int tc = 0; tc < 2; ++tc)
#pragma unroll
                        for (int tp = 0; tp < 2; ++tp) {
                            const float av = u == 0 ? a[tc].x : u == 1 ? a[tc].y : u == 2 ? a[tc].z : a[tc].w;
                            const float wv = u == 0 ? w[tp].x : u == 1 ? w[tp].y : u == 2 ? w[tp].z : w[tp].w;
                            acc[tc][tp] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, wv, acc[tc][tp], 0, 0, 0);
                        }
            }
        }
        mfma_drain();          // behind a loop with a run-time count, in front of the first read of the accumulators (see mfma_drain)
        // accumulator element e of lane (r, h) in tile (tc, tp): centroid c0 + wc + 32 tc + (e & 3) + 8 (e >> 2) + 4 h, point wp + 32 tp + r
#pragma unroll
        for (int tc = 0; tc < 2; ++tc)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int row = wc + 32 * tc + (e & 3) + 8 * (e >> 2) + 4 * h, j = c0 + row;
                if (j >= k) continue;
                const float hj = Hs[row];
#pragma unroll
                for (int tp = 0; tp < 2; ++tp) {
                    const float s = acc[tc][tp][e] - hj;
                    if (s > bs[tp]) { bs[tp] = s; bj[tp] = j; }
                }
            }
    }
    // the other lane half holds the other centroid rows of the same points: higher score, then lower index
#pragma unroll
    for (int tp = 0; tp < 2; ++tp) {
        const float os = __shfl_xor(bs[tp], 32, 64);
        const int oj = __shfl_xor(bj[tp], 32, 64);
        if (os > bs[tp] || (os == bs[tp] && oj < bj[tp])) { bs[tp] = os; bj[tp] = oj; }
    }
    // the two waves that share the points meet in LDS (the operand tiles are free behind the barrier)
    __syncthreads();
    float* red_s = Cs;                  // [2][128]
    int* red_j = (int*)Xs;              // [2][128]
    if (h == 0) {
#pragma unroll
        for (int tp = 0; tp < 2; ++tp) {
            red_s[(wave >> 1) * KT + wp + 32 * tp + r] = bs[tp];
            red_j[(wave >> 1) * KT + wp + 32 * tp + r] = bj[tp];
        }
    }
    __syncthreads();
    if (tid < KT && m0 + tid < n) {
        float s = red_s[tid];
        int j = red_j[tid];
        const float os = red_s[KT + tid];
        const int oj = red_j[KT + tid];
        if (os > s || (os == s && oj < j)) { s = os; j = oj; }
        if (j >= k) j = 0;          // no score compared greater than -inf (a NaN row): centroid 0, best stays -inf
        assign[m0 + tid] = j;
        if (best) best[m0 + tid] = s;
    }
}

// fp32(0.5 * sum_t row[t]^2), the sum in fp64 in a fixed order; every lane of the wave returns it
__device__ __forceinline__ float half_sqnorm_row(const float* __restrict__ row, int d, int lane) {
    double s = 0.0;
    for (int t = lane; t < d; t += 64) { const double v = (double)row[t]; s += v * v; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    return (float)(0.5 * s);
}

__global__ __launch_bounds__(256) void kmeans_half_sqnorm_kernel(const float* __restrict__ Cn, int k, int d, float* __restrict__ hsq) {
    const int lane = threadIdx.x & 63, j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= k) return;
    const float v = half_sqnorm_row(Cn + (size_t)j * d, d, lane);
    if (lane == 0) hsq[j] = v;
}

__global__ __launch_bounds__(256) void kmeans_finish_kernel(const float* __restrict__ sums, const int* __restrict__ offsets, float* __restrict__ Cn,
                                                             float* __restrict__ hsq, int k, int d) {
    const int lane = threadIdx.x & 63, j = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (j >= k) return;
    const int m = offsets[j + 1] - offsets[j];
    float* row = Cn + (size_t)j * d;
    if (m > 0) {
        const float fm = (float)m;
        for (int t = lane; t < d; t += 64) row[t] = __fdiv_rn(sums[(size_t)j * d + t], fm);
    }
    // a lane reads back only the columns it wrote itself
    const float v = half_sqnorm_row(row, d, lane);
    if (lane == 0) hsq[j] = v;
}

__global__ __launch_bounds__(1024) void kmeans_count_empty_kernel(const int* __restrict__ offsets, int k, int* __restrict__ n_empty) {
    __shared__ int part[16];
    int c = 0;
    for (int j = threadIdx.x; j < k; j += 1024) c += offsets[j + 1] - offsets[j] > 0 ? 0 : 1;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int w = 0; w < 16; ++w) s += part[w];
        n_empty[0] = s;
    }
}

inline bool aligned_to(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

int kmeans_refuse(const char* op, const char* why) {
    char msg[200];
    snprintf(msg, sizeof(msg), "%s: %s", op, why);
    return cldrd_set_error(msg);
}
#define KMEANS_CHECK(cond, why) do { if (!(cond)) return kmeans_refuse(op, why); } while (0)

// the limits every entry point shares: the width d and the centroid table
int kmeans_check_centroids(const char* op, const float* C, const float* h, int k, int d) {
    KMEANS_CHECK(d % 32 == 0 && d >= 32 && d <= 1024, "d must be a multiple of 32 with 32 <= d <= 1024");
    KMEANS_CHECK(k >= 1 && k <= 65536, "k must be 1 .. 65536");
    KMEANS_CHECK(C != nullptr, "null C");
    KMEANS_CHECK(h != nullptr, "null h");
    KMEANS_CHECK(aligned_to(C, 16), "C must be 16-byte aligned");
    KMEANS_CHECK(aligned_to(h, 16), "h must be 16-byte aligned");
    return 0;
}

}  // namespace

extern "C" int cldrd_kmeans_assign(const float* X, int ldx, int n, int d, const float* C, const float* h, int k, long long* assign, float* best,
                                   void* stream) {
    const char* op = "kmeans_assign";
    if (int rc = kmeans_check_centroids(op, C, h, k, d)) return rc;
    KMEANS_CHECK(n >= 1 && n <= (1 << 22), "n must be 1 .. 2^22");
    KMEANS_CHECK(k <= n, "k must not exceed n");
    KMEANS_CHECK(ldx >= d && ldx % 4 == 0, "ldx must cover a row (ldx >= d) and be a multiple of 4");
    KMEANS_CHECK(X != nullptr, "null X");
    KMEANS_CHECK(assign != nullptr, "null assign");
    KMEANS_CHECK(aligned_to(X, 16), "X must be 16-byte aligned");
    KMEANS_CHECK(aligned_to(assign, 16), "assign must be 16-byte aligned");
    KMEANS_CHECK(best == nullptr || aligned_to(best, 16), "best must be 16-byte aligned");
    hipLaunchKernelGGL(kmeans_assign_kernel, dim3((n + KT - 1) / KT), dim3(256), 0, (hipStream_t)stream, X, ldx, n, d, C, h, k, assign, best);
    CLDRD_LAUNCH_CHECK();
    return 0;
}

extern "C" int cldrd_kmeans_half_sqnorm(const float* C, int k, int d, float* h, void* stream) {
    const char* op = "kmeans_half_sqnorm";
    if (int rc = kmeans_check_centroids(op, C, h, k, d)) return rc;
    hipLaunchKernelGGL(kmeans_half_sqnorm_kernel, dim3((k + 3) / 4), dim3(256), 0, (hipStream_t)stream, C, k, d, h);
    CLDRD_LAUNCH_CHECK();
    return 0;
}

extern "C" int cldrd_kmeans_finish(const float* sums, const int* offsets, float* C, float* h, int* n_empty, int k, int d, void* stream) {
    const char* op = "kmeans_finish";
    if (int rc = kmeans_check_centroids(op, C, h, k, d)) return rc;
    KMEANS_CHECK(sums != nullptr, "null sums");
    KMEANS_CHECK(offsets != nullptr, "null offsets");
    KMEANS_CHECK(n_empty != nullptr, "null n_empty");
    KMEANS_CHECK(aligned_to(sums, 16), "sums must be 16-byte aligned");
    KMEANS_CHECK(aligned_to(offsets, 16), "offsets must be 16-byte aligned");
    KMEANS_CHECK(aligned_to(n_empty, 16), "n_empty must be 16-byte aligned");
    hipLaunchKernelGGL(kmeans_finish_kernel, dim3((k + 3) / 4), dim3(256), 0, (hipStream_t)stream, sums, offsets, C, h, k, d);
    CLDRD_LAUNCH_CHECK();
    hipLaunchKernelGGL(kmeans_count_empty_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, offsets, k, n_empty);
    CLDRD_LAUNCH_CHECK();
    return 0;
}

// int8-row mode of the flat index (retriever/retrieval_utils.py: FlatIPIndex, to_gpu(dev, int8_rows=True)).
//
// The shard keeps mu (fp32 [d], its mean row), R8 (int8 [n, d]) and a (fp32 [n], one scale per row) and nothing else of the rows:
//     c = p - mu (fp32),  a_r = max_j |c_j| / 127 (fp32, correctly rounded),  R8[r, j] = clamp(rint(c_j / a_r), -127, 127)
// (a_r = 0 and R8[r] = 0 for an all-zero c).  The stored row is mu + a_r R8[r] and its score
//     s(q, r) = fp32( <q, mu> + a_r <q, R8[r]> )             both sums and the product in fp64, one rounding (rescore_i8_kernel).
//
// The scan works on INTEGERS.  A query is split into two int8 digits of a common scale sq = max_j |q_j| / 16256:
//     t_j = rint(q_j / sq) in [-16256, 16256],  l_j = ((t_j + 64) mod 128) - 64 in [-64, 63],  h_j = (t_j - l_j) / 128 in [-127, 127]
// and H = <h, R8[r]>, L = <l, R8[r]> are exact int32 sums of v_mfma_i32_16x16x64_i8 (|H| <= 127 127 d = 33 M at d = 2048).  128 H + L would
// overflow int32 there, so the scan score is PINNED as
//     s^ = fmaf(128.0f, (float)H, (float)L) * (sq * a_r)       conversions round to nearest even, products in fp32
// which tests/test_gpu_index_int8.py restates in numpy and compares bit for bit.
//
// Bound (thresholds_i8_kernel), against the exact centred score s_c = a_r <q, R8[r]> of the STORED row:
//   1. query digits.  t_j = rint(fl(q_j / sq)): the division rounds by at most 2^-24 16256 < 2^-10 units, the clamp at +-16256 cuts less than that
//      (fl(max|q| / 16256) is within 2^-24 of the quotient), so q_j = sq (t_j + e_j) with |e_j| <= 1/2 + 2^-9, and
//          |s_c - sq a_r <t, R8[r]>| <= sq (1/2 + 2^-9) a_r |R8[r]|_1 <= sq (1/2 + 2^-9) B1,          B1 = max_r a_r |R8[r]|_1
//      (B1 comes from exact integer row sums at attach time: quantize_i8_kernel).  A query with max|q| < 2^-100 gets no digits and sq = 2 max|q|:
//      then t = 0, |q_j| <= sq / 2 and the same line holds (and a subnormal sq never divides anything).
//   2. the fp32 roundings of s^.  With T = 128 H + L = <t, R8[r]> and N = |R8[r]|_2: |L| <= 64 sqrt(d) N, |T| <= |t|_2 N with
//      |t|_2 <= |q| / sq + (1/2 + 2^-9) sqrt(d), and |128 H| <= |T| + |L|; so every magnitude below is at most M = (|q| / sq + 65 sqrt(d)) N.
//      (float)H moves 128 H by 2^-24 |128 H|, (float)L moves L by 2^-24 |L|, the fma rounds once (2^-24 |F|), fl(sq a_r) and the final product
//      round once each: five roundings of relative size 2^-24 on a value of at most M sq a_r (1 + 2^-22), i.e.
//          5 2^-24 (|q| + 65 sq sqrt(d)) max_r a_r |R8[r]|_2 (1 + 2^-22).
//   eps = (1. + 2.) (1 + 1e-6) + 1e-30 (results below the fp32 normal range).  thr = est - 2 eps, as in the 16-bit modes (select_compact_kernel of
//   topk.hip explains the 2).  At d = 768 term 1 is ~2-3e-3 of the score spread, a tenth of the fp16 scan's eps; term 2 is ~1e-2 of term 1.
#include "common.h"
#include "topk_chain.h"
#include "../../include/cldrd_hip.h"
#include <float.h>

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ uint32_t pack4i8(int a, int b, int c, int e) {
    return (uint32_t)(a & 255) | ((uint32_t)(b & 255) << 8) | ((uint32_t)(c & 255) << 16) | ((uint32_t)(e & 255) << 24);
}
__device__ __forceinline__ int quant1(float c, float a) {       // clamp(rint(c / a), -127, 127), a > 0
    return (int)fminf(fmaxf(rintf(__fdiv_rn(c, a)), -127.f), 127.f);
}

// One pass per fp32 chunk (the chunking of index_center_cast_kernel, topk.hip): one wave per row, lane l owns columns 4 l .. 4 l + 3 (+ 256 per
// further group; d <= 2048: eight groups, kept in registers between the maximum and the rounding).  Writes R8, a, the bf16 threshold sample
// (the STORED centred row a_r R8[r], row r = i * s_stride of the whole shard), and the running maxima of a_r |R8[r]|_1 and a_r^2 |R8[r]|_2^2 as
// fp32 bit patterns (non-negative floats order like their bits): each is the fp32 value of the fp64 product of a_r (a_r^2: exact in fp64) with the
// exact integer sum.  *flag |= 1 for a value that is not finite.
__global__ __launch_bounds__(256) void quantize_i8_kernel(const float* __restrict__ P, const float* __restrict__ mu, size_t rows, size_t row0, int d,
                                                           int8_t* __restrict__ R8, float* __restrict__ scale, bf16_t* __restrict__ sample,
                                                           size_t s_stride, size_t s_rows, unsigned int* __restrict__ b1_bits,
                                                           unsigned int* __restrict__ c2_bits, unsigned int* __restrict__ flag) {
    constexpr int MAXG = 8;
    const int lane = threadIdx.x & 63;
    float best1 = 0.f, best2 = 0.f;
    bool bad = false;
    for (size_t r = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += (size_t)gridDim.x * 4) {
        const float* pr = P + r * d;
        float c[MAXG][4];
        float amax = 0.f;
#pragma unroll
        for (int g = 0; g < MAXG; ++g) {
            const int j = lane * 4 + 256 * g;
            if (j < d) {
                const float4 v = *(const float4*)(pr + j);
                const float4 m = *(const float4*)(mu + j);
                c[g][0] = v.x - m.x; c[g][1] = v.y - m.y; c[g][2] = v.z - m.z; c[g][3] = v.w - m.w;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    bad |= !(fabsf(c[g][i]) <= FLT_MAX);
                    amax = fmaxf(amax, fabsf(c[g][i]));
                }
            } else {
                c[g][0] = c[g][1] = c[g][2] = c[g][3] = 0.f;
            }
        }
        amax = wave_max(amax);
        const float a = __fdiv_rn(amax, 127.f);
        const bool live = a > 0.f && amax <= FLT_MAX;
        const size_t gr = row0 + r;
        const bool in_sample = sample != nullptr && gr % s_stride == 0 && gr / s_stride < s_rows;
        bf16_t* so = in_sample ? sample + (gr / s_stride) * d : nullptr;
        int l1 = 0, s2 = 0;
#pragma unroll
        for (int g = 0; g < MAXG; ++g) {
            const int j = lane * 4 + 256 * g;
            if (j < d) {
                int v[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    v[i] = live ? quant1(c[g][i], a) : 0;
                    l1 += abs(v[i]);
                    s2 += v[i] * v[i];
                }
                *(uint32_t*)(R8 + r * d + j) = pack4i8(v[0], v[1], v[2], v[3]);
                if (in_sample) {
                    uint2 u;
                    u.x = pack2bf(a * (float)v[0], a * (float)v[1]);
                    u.y = pack2bf(a * (float)v[2], a * (float)v[3]);
                    *(uint2*)(so + j) = u;
                }
            }
        }
        l1 = wave_sum_i(l1);
        s2 = wave_sum_i(s2);
        const float as = live ? a : 0.f;
        if (lane == 0) scale[r] = as;
        best1 = fmaxf(best1, (float)((double)as * (double)l1));
        best2 = fmaxf(best2, (float)(((double)as * (double)as) * (double)s2));
    }
    if (lane == 0 && best1 > 0.f) atomicMax(b1_bits, __float_as_uint(best1));
    if (lane == 0 && best2 > 0.f) atomicMax(c2_bits, __float_as_uint(best2));
    if (bad && flag) atomicOr(flag, 1u);
}

// One block per query: the two digit planes qd[0] = h, qd[1] = l (int8 [nq, d] each, `plane` bytes apart), sq, |q| (fp32 of the fp64 sum of
// squares' root), the bf16 copy for the threshold GEMM, *flag |= 1 for a value that is not finite.  Thread t owns columns 4 t .. 4 t + 3 (+ 1024).
__global__ __launch_bounds__(256) void prep_queries_i8_kernel(const float* __restrict__ q, int8_t* __restrict__ qd, size_t plane, bf16_t* __restrict__ qb,
                                                               float* __restrict__ sq, float* __restrict__ qnorm, int d, unsigned int* __restrict__ flag) {
    __shared__ float redm[4];
    __shared__ double reds[4];
    const float* row = q + (size_t)blockIdx.x * d;
    float x[2][4];
    float amax = 0.f;
    double s = 0.0;
    bool bad = false;
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        const int j = threadIdx.x * 4 + 1024 * g;
        if (j < d) {
            const float4 v = *(const float4*)(row + j);
            x[g][0] = v.x; x[g][1] = v.y; x[g][2] = v.z; x[g][3] = v.w;
            uint2 u; u.x = pack2bf(v.x, v.y); u.y = pack2bf(v.z, v.w);
            *(uint2*)(qb + (size_t)blockIdx.x * d + j) = u;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                bad |= !(fabsf(x[g][i]) <= FLT_MAX);
                amax = fmaxf(amax, fabsf(x[g][i]));
                s += (double)x[g][i] * (double)x[g][i];
            }
        } else {
            x[g][0] = x[g][1] = x[g][2] = x[g][3] = 0.f;
        }
    }
    amax = wave_max(amax);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) { redm[threadIdx.x >> 6] = amax; reds[threadIdx.x >> 6] = s; }
    __syncthreads();
    amax = fmaxf(fmaxf(redm[0], redm[1]), fmaxf(redm[2], redm[3]));
    const bool digits = amax >= 0x1p-100f && amax <= FLT_MAX;
    const float scale = digits ? __fdiv_rn(amax, 16256.f) : (amax <= FLT_MAX ? 2.0f * amax : 0.f);
#pragma unroll
    for (int g = 0; g < 2; ++g) {
        const int j = threadIdx.x * 4 + 1024 * g;
        if (j < d) {
            int h[4], l[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int t = digits ? (int)fminf(fmaxf(rintf(__fdiv_rn(x[g][i], scale)), -16256.f), 16256.f) : 0;
                l[i] = ((t + 64) & 127) - 64;
                h[i] = (t - l[i]) >> 7;
            }
            *(uint32_t*)(qd + (size_t)blockIdx.x * d + j) = pack4i8(h[0], h[1], h[2], h[3]);
            *(uint32_t*)(qd + plane + (size_t)blockIdx.x * d + j) = pack4i8(l[0], l[1], l[2], l[3]);
        }
    }
    if (threadIdx.x == 0) {
        sq[blockIdx.x] = scale;
        qnorm[blockIdx.x] = (float)sqrt((reds[0] + reds[1]) + (reds[2] + reds[3]));
    }
    if (bad && flag) atomicOr(flag, 1u);
}

// eps[q] >= |s^ - s_c| for every row of the shard (derivation at the top of this file); thr[q] = est[q] - 2 eps[q]
__global__ void thresholds_i8_kernel(const float* __restrict__ est, const float* __restrict__ sq, const float* __restrict__ qnorm, float b1, float cnorm,
                                     int d, float* __restrict__ thr, float* __restrict__ eps, int nq) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nq) return;
    const double s = sq[i], qn = qnorm[i], rd = sqrt((double)d);
    const double e = s * (0.5 + 0x1p-9) * (double)b1 + 5.0 * 0x1p-24 * (qn + 65.0 * s * rd) * (double)cnorm * (1.0 + 0x1p-22);
    const float ef = (float)(e * (1.0 + 1e-6)) + 1e-30f;
    eps[i] = ef;
    if (est) thr[i] = est[i] - 2.0f * ef;
}

// The scan.  NW waves, wave w keeps the two digit planes of queries 16 w .. 16 w + 15 as MFMA B fragments for the whole K range (8 KS
// registers; KS = k-steps of 64 this instance holds, ksn <= KS of them in use: one schedule for every width).  The rows stream through a
// double-buffered LDS tile of R whole rows (R d contiguous bytes of HBM, read once per launch; R = 64, or 32 where two tiles of 64 do not fit
// the LDS): the global loads of tile i + 1 are in flight while tile i is multiplied, and a tile is large enough for that to cover most of their
// latency.  The row scales of a tile travel with it through the LDS: vector memory returns in order, so a wait for a scale fetched from
// global memory behind the next tile's loads would wait for that whole tile (a hit's returning atomic still does).  LDS rows are d + 16 bytes
// apart, so the sixteen 16-byte A fragments a quarter wave reads (one row each, 16 bytes of one row per lane and k-step) fall into sixteen
// different bank groups.  Lane map of v_mfma_i32_16x16x64_i8 as used here: A lane l = row l & 15,
// bytes 64 ks + 16 (l >> 4) .. + 15; B lane l = query l & 15, the same bytes; D[j] of lane l = <row 4 (l >> 4) + j, query l & 15>
// (tests/test_gpu_index_int8.py: test_lane_map).  Every (query, row) with s^ >= thr[query] goes straight to the query's global list; a hit past
// `cap` still counts in counts[query] (select: status bit 2) and in *dropped.
template <int KS, int NW, int R>
__global__ __launch_bounds__(64 * NW) void scan_i8_kernel(const int8_t* __restrict__ R8, const float* __restrict__ scale, const int8_t* __restrict__ qd,
                                                          size_t plane, const float* __restrict__ sq, const float* __restrict__ thr, int nq, int rows,
                                                          int d, int* __restrict__ counts, int* __restrict__ dropped, int* __restrict__ cand_rows,
                                                          float* __restrict__ cand_scores, int cap) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int T = 64 * NW, PPT = (R * 4 * KS + T - 1) / T;                // 16-byte pieces of a tile per thread
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int ksn = d / 64, cpr = d / 16, ldr = d + 16, npieces = R * cpr;
    const int ntiles = (rows + R - 1) / R;

    const int qn = wid * 16 + (lane & 15);
    const bool qlive = qn < nq;
    const int8_t* qp = qd + (size_t)(qlive ? qn : nq - 1) * d + 16 * (lane >> 4);
    i32x4 bh[KS], bl[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {                                  // branch-free: a k-step past the width re-reads step 0 and is zeroed
        const int on = ks < ksn ? -1 : 0;
        const int8_t* p = qp + (ks & on) * 64;
        bh[ks] = *(const i32x4*)p & on;
        bl[ks] = *(const i32x4*)(p + plane) & on;
    }
    const float thr_q = qlive ? thr[qn] : __builtin_inff();
    const float sq_q = qlive ? sq[qn] : 0.f;

    uint4 stage[PPT];
    float stage_scale = 0.f;
    auto load_tile = [&](int tile) {
        const int row_base = tile * R;
        if ((int)threadIdx.x < R) stage_scale = row_base + (int)threadIdx.x < rows ? scale[row_base + threadIdx.x] : 0.f;
#pragma unroll
        for (int i = 0; i < PPT; ++i) {
            const int p = (int)threadIdx.x + i * T;
            const int row = p / cpr;
            stage[i] = make_uint4(0u, 0u, 0u, 0u);
            if (p < npieces && row_base + row < rows) stage[i] = ld16_stream(R8 + (size_t)row_base * d + (size_t)p * 16);
        }
    };
    auto store_tile = [&](char* buf) {
        if ((int)threadIdx.x < R) ((float*)(buf + R * ldr))[threadIdx.x] = stage_scale;
#pragma unroll
        for (int i = 0; i < PPT; ++i) {
            const int p = (int)threadIdx.x + i * T;
            if (p < npieces) {
                const int row = p / cpr, c = p - row * cpr;
                *(uint4*)(buf + row * ldr + c * 16) = stage[i];
            }
        }
    };
    char* bufs[2] = {smem, smem + R * ldr + R * 4};                    // a buffer: R rows of ldr bytes, then their R scales
    int t = blockIdx.x;
    if (t < ntiles) { load_tile(t); store_tile(bufs[0]); }
    __syncthreads();
    for (int it = 0; t < ntiles; t += gridDim.x, ++it) {
        const int next = t + gridDim.x;
        if (next < ntiles) load_tile(next);
        const char* sb = bufs[it & 1];
#pragma unroll 1
        for (int mt = 0; mt < R / 16; ++mt) {
            const int row0 = t * R + mt * 16 + 4 * (lane >> 4);
            const f32x4 ar = *(const f32x4*)(sb + R * ldr + 4 * (mt * 16 + 4 * (lane >> 4)));
            const char* ap = sb + (mt * 16 + (lane & 15)) * ldr + 16 * (lane >> 4);
            i32x4 ah = {0, 0, 0, 0}, al = {0, 0, 0, 0};
            // k-steps past the row's width (ks >= ksn) multiply whatever LDS bytes follow the row by zero query digits: exact zeros in integer
            // arithmetic, and the allocation is sized for KS k-steps whatever d is, so the reads stay inside it
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const i32x4 a = *(const i32x4*)(ap + ks * 64);
                ah = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, bh[ks], ah, 0, 0, 0);
                al = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, bl[ks], al, 0, 0, 0);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float w = sq_q * ar[j];
                const float s = fmaf(128.0f, (float)ah[j], (float)al[j]) * w;
                if (s >= thr_q && row0 + j < rows) {
                    const int pos = atomicAdd(counts + qn, 1);
                    if (pos < cap) {
                        cand_rows[(size_t)qn * cap + pos] = row0 + j;
                        cand_scores[(size_t)qn * cap + pos] = s;
                    } else {
                        atomicAdd(dropped, 1);
                    }
                }
            }
        }
        if (next < ntiles) store_tile(bufs[(it + 1) & 1]);
        __syncthreads();
    }
}

// exact re-score (rescore16_kernel of topk.hip on int8 rows): one wave per candidate, 8 row bytes per lane and step, fp64 accumulation in a fixed
// order, scores2 = fp32(qmu[q] + a_r * sum), the product in fp64, one rounding
__device__ __forceinline__ double dot4_i8(const float4 a, uint32_t w, double s) {
    s = fma((double)a.x, (double)(int8_t)(w & 255u), s); s = fma((double)a.y, (double)(int8_t)((w >> 8) & 255u), s);
    s = fma((double)a.z, (double)(int8_t)((w >> 16) & 255u), s); s = fma((double)a.w, (double)(int8_t)(w >> 24), s);
    return s;
}
__global__ __launch_bounds__(256) void rescore_i8_kernel(const float* __restrict__ q, const int8_t* __restrict__ R8, const float* __restrict__ scale,
                                                          const double* __restrict__ qmu, int d, const int* __restrict__ counts,
                                                          const int* __restrict__ cand_rows, float* __restrict__ cand_scores, int cap) {
    const int qi = blockIdx.y;
    const int n = min(counts[qi], cap);
    const int lane = threadIdx.x & 63;
    const float* qr = q + (size_t)qi * d;
    const double base = qmu[qi];
    for (int c = blockIdx.x * 4 + (threadIdx.x >> 6); c < n; c += gridDim.x * 4) {
        const int r = cand_rows[(size_t)qi * cap + c];
        const int8_t* pr = R8 + (size_t)r * d;
        double s = 0.0;
        for (int j = lane * 8; j < d; j += 512) {
            const uint2 bu = *(const uint2*)(pr + j);
            s = dot4_i8(*(const float4*)(qr + j), bu.x, s);
            s = dot4_i8(*(const float4*)(qr + j + 4), bu.y, s);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == 0) {
            const double prod = (double)scale[r] * s;
            cand_scores[(size_t)qi * cap + c] = (float)(base + prod);
        }
    }
}

template <int KS, int NW, int R>
int launch_scan_i8(const int8_t* R8, const float* scale, const int8_t* qd, size_t plane, const float* sq, const float* thr, int nq, int rows, int d,
                   int* counts, int* dropped, int* cand_rows, float* cand_scores, int cap, hipStream_t st) {
    constexpr int lds = 2 * R * (64 * KS + 16 + 4);                    // for KS k-steps whatever d is: see the k loop of the kernel
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute((const void*)scan_i8_kernel<KS, NW, R>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        attr_set = true;
    }
    static_assert(lds <= 160 * 1024 && R % 16 == 0, "two tiles must fit the LDS");
    const int ntiles = (rows + R - 1) / R;
    // the launch takes 16 NW queries; more of them (up to the caller's tile) go through further launches over the same rows
    for (int lo = 0; lo < nq; lo += 16 * NW) {
        const int m = nq - lo < 16 * NW ? nq - lo : 16 * NW;
        hipLaunchKernelGGL((scan_i8_kernel<KS, NW, R>), dim3(ntiles < 256 ? ntiles : 256), dim3(64 * NW), lds, st, R8, scale, qd + (size_t)lo * d, plane,
                           sq + lo, thr + lo, m, rows, d, counts + lo, dropped, cand_rows + (size_t)lo * cap, cand_scores + (size_t)lo * cap, cap);
        CLDRD_LAUNCH_CHECK();
    }
    return 0;
}

}  // namespace

// R8 / a / sample / maxima of one fp32 chunk of a shard (rows [row0, row0 + rows); a whole shard is one chunk with row0 = 0).  *b1_bits, *c2_bits
// and *flag accumulate over the chunks: zero them before the first one.
extern "C" int cldrd_index_quantize_i8(const float* P, const float* mu, size_t rows, size_t row0, int d, void* R8, float* scale, void* sample_bf16,
                                       size_t s_stride, size_t s_rows, unsigned int* b1_bits, unsigned int* c2_bits, unsigned int* flag, void* stream) {
    CLDRD_CHECK(rows > 0 && d > 0 && d % 64 == 0 && d <= 2048, "index_quantize_i8: int8 rows need a width that is a multiple of 64 and at most 2048");
    CLDRD_CHECK(R8 != nullptr && scale != nullptr && b1_bits != nullptr && c2_bits != nullptr, "index_quantize_i8: null operands");
    CLDRD_CHECK(sample_bf16 == nullptr || s_stride > 0, "index_quantize_i8: sample stride");
    CLDRD_CHECK((uintptr_t)P % 16 == 0 && (uintptr_t)mu % 16 == 0 && (uintptr_t)R8 % 4 == 0 && (uintptr_t)sample_bf16 % 8 == 0, "index_quantize_i8: aligned operands");
    const int nb = (int)((rows + 3) / 4 < 4096 ? (rows + 3) / 4 : 4096);
    hipLaunchKernelGGL(quantize_i8_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, P, mu, rows, row0, d, (int8_t*)R8, scale, (bf16_t*)sample_bf16,
                       s_stride, s_rows, b1_bits, c2_bits, flag);
    CLDRD_LAUNCH_CHECK();
    return 0;
}

// qd: int8 [2, nq, d] (plane 0 = h, plane 1 = l); sq, qnorm: fp32 [nq]; q_bf16: [nq, d]
extern "C" int cldrd_topk_prep_queries_i8(const float* q, void* qd, void* q_bf16, float* sq, float* qnorm, int nq, int d, unsigned int* flag, void* stream) {
    CLDRD_CHECK(nq > 0 && d > 0 && d % 64 == 0 && d <= 2048, "topk_prep_queries_i8: int8 rows need a width that is a multiple of 64 and at most 2048");
    CLDRD_CHECK((uintptr_t)q % 16 == 0 && (uintptr_t)qd % 16 == 0 && (uintptr_t)q_bf16 % 8 == 0, "topk_prep_queries_i8: aligned operands");
    hipLaunchKernelGGL(prep_queries_i8_kernel, dim3(nq), dim3(256), 0, (hipStream_t)stream, q, (int8_t*)qd, (size_t)nq * d, (bf16_t*)q_bf16, sq, qnorm, d, flag);
    CLDRD_LAUNCH_CHECK();
    return 0;
}

// b1 = max_r a_r |R8[r]|_1, cnorm = max_r a_r |R8[r]|_2 (the caller may pass them with its own slack)
extern "C" int cldrd_topk_thresholds_i8(const float* est, const float* sq, const float* qnorm, float b1, float cnorm, int d, float* thr, float* eps, int nq,
                                        void* stream) {
    CLDRD_CHECK(nq > 0 && d > 0 && (est == nullptr || thr != nullptr) && sq != nullptr && qnorm != nullptr, "topk_thresholds_i8: bad arguments");
    hipLaunchKernelGGL(thresholds_i8_kernel, dim3((nq + 255) / 256), dim3(256), 0, (hipStream_t)stream, est, sq, qnorm, b1, cnorm, d, thr, eps, nq);
    CLDRD_LAUNCH_CHECK();
    return 0;
}

// One scan of nq <= 256 queries (digit planes qd[0], qd[1] of nq_plane queries each: `qd` points at the first query of this call inside plane 0)
// over `rows` rows.  counts: nq list lengths + 1 dropped-hit counter (the layout cldrd_topk_select reads), zeroed by the caller.
extern "C" int cldrd_topk_scan_i8(const void* qd, long long nq_plane, const float* sq, const float* thr, const void* R8, const float* scale, int nq,
                                  long long rows, int d, int* counts, int* cand_rows, float* cand_scores, int cap, void* stream) {
    CLDRD_CHECK(nq > 0 && nq <= 256 && nq_plane >= nq && rows > 0 && rows < 2147483647LL - 64 && cap > 0, "topk_scan_i8: bad arguments");
    CLDRD_CHECK(d > 0 && d % 64 == 0 && d <= 2048, "topk_scan_i8: int8 rows need a width that is a multiple of 64 and at most 2048");
    CLDRD_CHECK((uintptr_t)qd % 16 == 0 && (uintptr_t)R8 % 16 == 0, "topk_scan_i8: aligned operands");
    const size_t plane = (size_t)nq_plane * d;
    hipStream_t st = (hipStream_t)stream;
#define CLDRD_SCAN_I8(KS, NW, R) return launch_scan_i8<KS, NW, R>((const int8_t*)R8, scale, (const int8_t*)qd, plane, sq, thr, nq, (int)rows, d, counts, counts + nq, \
                                                            cand_rows, cand_scores, cap, st)
    if (d <= 128) CLDRD_SCAN_I8(2, 8, 64);
    if (d <= 256) CLDRD_SCAN_I8(4, 8, 64);
    if (d <= 384) CLDRD_SCAN_I8(6, 8, 64);
    if (d <= 512) CLDRD_SCAN_I8(8, 8, 64);
    if (d <= 768) CLDRD_SCAN_I8(12, 8, 64);
    if (d <= 1024) CLDRD_SCAN_I8(16, 8, 32);
    if (d <= 1536) CLDRD_SCAN_I8(24, 4, 32);                // above 1024: 192 / 256 query registers per lane, one wave per SIMD, 64 queries per launch
    CLDRD_SCAN_I8(32, 4, 32);
#undef CLDRD_SCAN_I8
}

extern "C" int cldrd_topk_rescore_i8(const float* q, const void* R8, const float* scale, const double* qmu, int d, const int* counts, const int* cand_rows,
                                     float* cand_scores, int nq, int cap, void* stream) {
    CLDRD_CHECK(nq > 0 && d > 0 && d % 64 == 0 && cap > 0 && R8 != nullptr && scale != nullptr && qmu != nullptr, "topk_rescore_i8: bad arguments");
    CLDRD_CHECK((uintptr_t)q % 16 == 0 && (uintptr_t)R8 % 8 == 0, "topk_rescore_i8: aligned operands");
    hipLaunchKernelGGL(rescore_i8_kernel, dim3(64, nq), dim3(256), 0, (hipStream_t)stream, q, (const int8_t*)R8, scale, qmu, d, counts, cand_rows, cand_scores, cap);
    CLDRD_LAUNCH_CHECK();
    return 0;
}

// The chain of cldrd_flatip_search in int8-row mode, per query tile back to back on `stream`: scan (or every row when exhaustive) -> select ->
// re-score from R8 / a -> sort + cut.  Same counts / status / n2 / khat contract; qtile = 128.  A hit is only ever lost to `cap`, which sets
// status bit 2 of THAT query; bit 4 then marks every query of the pass, and the caller may ignore it.
extern "C" int cldrd_flatip_search_i8(const float* q32, const void* qd, const float* sq, const float* thr, const float* eps, const void* R8,
                                      const float* scale, const double* qmu, long long rows, int d, int nq, int k, int qtile, int* counts, int* cand_rows,
                                      float* cand_scores, int cap, int* rows2, float* scores2, int cap2, int* n2, int* status, float* khat, float* D,
                                      int* I, int exhaustive, void* stream) {
    CLDRD_CHECK(R8 != nullptr && scale != nullptr && qmu != nullptr, "flatip_search_i8: int8 rows need R8, their scales and qmu");
    CLDRD_CHECK(nq > 0 && rows > 0 && k > 0 && cap > 0 && cap <= 8192 && cap2 > 0 && cap2 <= 8192, "flatip_search_i8: bad arguments");
    CLDRD_CHECK(d > 0 && d % 64 == 0 && d <= 2048, "flatip_search_i8: int8 rows need a width that is a multiple of 64 and at most 2048");
    CLDRD_CHECK(qtile == 128, "flatip_search_i8: the query tile is 128");
    CLDRD_CHECK(exhaustive == 0 || exhaustive == 1, "flatip_search_i8: exhaustive is 0 or 1");
    CLDRD_CHECK(!exhaustive || rows <= cap, "flatip_search_i8: exhaustive mode needs rows <= cap");
    CLDRD_CHECK(exhaustive || (qd != nullptr && sq != nullptr), "flatip_search_i8: a scan needs the query digits");
    return cldrd_flatip_chain(FlatipQueries{q32, nullptr, qd, sq, thr, eps, qmu, nq}, FlatipRows{nullptr, nullptr, R8, scale, rows}, d, k, qtile, counts,
                              cand_rows, cand_scores, cap, rows2, scores2, cap2, n2, status, khat, D, I, exhaustive, 0, (hipStream_t)stream);
}

// N-way scoring, forward + analytic backward, fp32: the dot product of the reference (models/nway_dual_encoder.py:30-47, optional in-batch
// negatives) and cosine similarity (--apply_consine_similarity), and row normalisation.  Which passage a logit column scores:
// score_layout.h.
//
// Cosine: the reference's launch script scripts/unity/cosine_nway_listwise.sh names the flag; the trainer it starts is not in the reference's
// tree, so the arithmetic is this package's (README: Cosine-similarity scoring), with eps as in torch.nn.functional.cosine_similarity:
//     nq = max(||q||, eps)   np_j = max(||p_j||, eps)   logit_j = scale * <q, p_j> / (nq * np_j)
// One kernel body per pass serves both scorers (template <bool COS>): the same grids, loads in flight and order of every sum; cosine adds
// the inverse norms (one launch more in the forward) and, in the backward, the scalar sum_j g_j logit_j of the row.  What only cosine needs
// stands under `if constexpr (COS)`: the dot-product kernels carry none of it.
// No float atomics: every sum has one order, so two calls give the same bits (--deterministic, graph replay == eager).
//
// inv_norms[B + B*N]: 1 / max(||row||, eps), queries first.  A row whose norm was clamped (||row|| <= eps) is stored NEGATED: the backward
// then takes its norm as the constant eps (no second term) and uses the magnitude.
#include <float.h>

#include "common.h"
#include "score_layout.h"

namespace {

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// one wave per row of q (rows 0..B-1) or p (rows B..)
__global__ __launch_bounds__(256) void cos_inv_norm_kernel(const float* __restrict__ q, const float* __restrict__ p, float* __restrict__ inv,
                                                            int B, int rows, int d, float eps) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int lane = threadIdx.x & 63;
    const float* x = r < B ? q + (size_t)r * d : p + (size_t)(r - B) * d;
    float s = 0.f;
    for (int c = lane * 4; c < d; c += 256) {
        const float4 a = *(const float4*)(x + c);
        s += a.x * a.x + a.y * a.y + a.z * a.z + a.w * a.w;
    }
    s = wave_sum(s);
    if (lane == 0) {
        const float n = sqrtf(s);
        inv[r] = n > eps ? 1.0f / n : -(1.0f / eps);
    }
}

// one wave per (query, column) pair.  Dot product: inv and scale are unused.
template <bool COS>
__global__ __launch_bounds__(256) void score_fwd_kernel(const float* __restrict__ q, const float* __restrict__ p, const float* __restrict__ inv,
                                                         float* __restrict__ logits, int B, int N, int Np, int d, int mode, float scale) {
    const int o = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (o >= B * Np) return;
    const int lane = threadIdx.x & 63;
    const int b = o / Np, j = o % Np;
    const int m = col_to_passage(mode, b, j, B, N);
    const float* qr = q + (size_t)b * d;
    const float* pr = p + (size_t)m * d;
    float s = 0.f;
    for (int c = lane * 4; c < d; c += 256) {
        const float4 a = *(const float4*)(qr + c), w = *(const float4*)(pr + c);
        s += a.x * w.x + a.y * w.y + a.z * w.z + a.w * w.w;
    }
    s = wave_sum(s);
    if (lane == 0) {
        if constexpr (COS) s = scale * ((s * fabsf(inv[b])) * fabsf(inv[B + m]));
        logits[o] = s;
    }
}

// dot:    dq[b] = sum_j g_j p_j                                                             p_j = p[passage(b, j)], j ascending
// cosine: dq[b] = iq * (scale * sum_j g_j ip_j p_j  -  (sum_j g_j logit_j) * iq * q[b])
template <bool COS>
__global__ __launch_bounds__(256) void score_bwd_q_kernel(const float* __restrict__ dl, const float* __restrict__ lg, const float* __restrict__ q,
                                                           const float* __restrict__ p, const float* __restrict__ inv, float* __restrict__ dq,
                                                           int B, int N, int Np, int d, int mode, float scale) {
    // grid (B, column chunks of 256): with one block per query a thread walked its Np passages one dependent load after the other
    // (26 us at B = 8, N = 32 on the step's critical path between the loss and the first backward GEMM); the loads of eight passages are
    // now in flight together.  Same summation order (j ascending): same bits.
    const int b = blockIdx.x;
    const int c = blockIdx.y * blockDim.x + threadIdx.x;
    if (c >= d) return;
    const float* ivp = COS ? inv + B : nullptr;
    float s = 0.f, gl = 0.f;
    int j = 0;
    for (; j + 8 <= Np; j += 8) {
        float v[8], w[8], l[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int m = col_to_passage(mode, b, j + u, B, N);
            w[u] = dl[(size_t)b * Np + j + u];
            v[u] = p[(size_t)m * d + c];
            if constexpr (COS) { l[u] = lg[(size_t)b * Np + j + u]; v[u] = fabsf(ivp[m]) * v[u]; }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            s += w[u] * v[u];
            if constexpr (COS) gl += w[u] * l[u];
        }
    }
    for (; j < Np; ++j) {
        const int m = col_to_passage(mode, b, j, B, N);
        const float w = dl[(size_t)b * Np + j];
        if constexpr (COS) {
            s += w * (fabsf(ivp[m]) * p[(size_t)m * d + c]);
            gl += w * lg[(size_t)b * Np + j];
        } else {
            s += w * p[(size_t)m * d + c];
        }
    }
    if constexpr (COS) {
        const float iq = inv[b], aq = fabsf(iq);
        float r = scale * s;
        if (iq > 0.f) r -= gl * (aq * q[(size_t)b * d + c]);
        s = aq * r;
    }
    dq[(size_t)b * d + c] = s;
}

// Over every (b, j) with passage(b, j) == m, the owner first, then b ascending:
// dot:    dp[m] = sum g q[b]
// cosine: dp[m] = ip * (scale * sum g iq_b q[b]  -  (sum g logit) * ip * p[m])
template <bool COS>
__global__ __launch_bounds__(256) void score_bwd_p_kernel(const float* __restrict__ dl, const float* __restrict__ lg, const float* __restrict__ q,
                                                           const float* __restrict__ p, const float* __restrict__ inv, float* __restrict__ dp,
                                                           int B, int N, int Np, int d, int mode, float scale) {
    const int m = blockIdx.x;
    const int bo = m / N, o = m % N;
    const size_t own = (size_t)bo * Np + o;
    float ip = 0.f, ap = 0.f, gl = 0.f;
    int bprev = 0;
    if constexpr (COS) {
        bprev = in_batch_prev_row(bo, B);               // cosine walks mode 2 twice (gl, then s): taken once, up here
        ip = inv[B + m], ap = fabsf(ip);
        gl = dl[own] * lg[own];
        if (mode == 1) {
            for (int b = 0; b < B; ++b)
                if (b != bo) { const size_t e = (size_t)b * Np + in_batch_col(m, b, N); gl += dl[e] * lg[e]; }
        } else if (mode == 2) {
            const size_t e = (size_t)bprev * Np + N + o;
            gl += dl[e] * lg[e];
        }
    }
    auto qv = [&](int b, int c) -> float {              // the query's element as this scorer's sum takes it
        if constexpr (COS) return fabsf(inv[b]) * q[(size_t)b * d + c];
        else return q[(size_t)b * d + c];
    };
    for (int c = threadIdx.x; c < d; c += blockDim.x) {
        float s = dl[own] * qv(bo, c);
        if (mode == 1) {
            for (int b = 0; b < B; ++b)
                if (b != bo) s += dl[(size_t)b * Np + in_batch_col(m, b, N)] * qv(b, c);
        } else if (mode == 2) {
            const int b = COS ? bprev : in_batch_prev_row(bo, B);
            s += dl[(size_t)b * Np + N + o] * qv(b, c);
        }
        if constexpr (COS) {
            float r = scale * s;
            if (ip > 0.f) r -= gl * (ap * p[(size_t)m * d + c]);
            s = ap * r;
        }
        dp[(size_t)m * d + c] = s;
    }
}

// out[r] = x[r] / max(||x[r]||, eps): one wave per row; the sum of squares and the norm in fp64, every element one fp64 division rounded
// to fp32 once (half an ulp from the exact quotient).  A lane reads all its elements of the row before the wave writes any (out may alias x).
__global__ __launch_bounds__(256) void l2_normalize_rows_kernel(const float* x, size_t ld_x, float* out, size_t n,
                                                                 int d, float eps) {
    const size_t r = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;
    const int lane = threadIdx.x & 63;
    const float* xr = x + r * ld_x;
    float* orow = out + r * (size_t)d;
    double s = 0.0;
    for (int c = lane * 4; c < d; c += 256) {
        const float4 a = *(const float4*)(xr + c);
        s += (double)a.x * a.x + (double)a.y * a.y + (double)a.z * a.z + (double)a.w * a.w;
    }
    s = wave_sum_f64(s);
    const double den = fmax(sqrt(s), (double)eps);
    for (int c = lane * 4; c < d; c += 256) {
        const float4 a = *(const float4*)(xr + c);
        *(float4*)(orow + c) = make_float4((float)(a.x / den), (float)(a.y / den), (float)(a.z / den), (float)(a.w / den));
    }
}

// The launches behind the four entry points: the logits (after the inverse norms, for cosine), and dq then dp.
template <bool COS>
int launch_score_fwd(const float* q, const float* p, const float* inv, float* logits, int B, int N, int d, int mode, float scale, void* stream) {
    const int Np = score_cols(B, N, mode);
    hipLaunchKernelGGL(score_fwd_kernel<COS>, dim3((B * Np + 3) / 4), dim3(256), 0, (hipStream_t)stream, q, p, inv, logits, B, N, Np, d, mode,
                       scale);
    CLDRD_LAUNCH_CHECK();
    return 0;
}
template <bool COS>
int launch_score_bwd(const float* dl, const float* lg, const float* q, const float* p, const float* inv, float* dq, float* dp, int B, int N,
                     int d, int mode, float scale, void* stream) {
    const int Np = score_cols(B, N, mode);
    hipLaunchKernelGGL(score_bwd_q_kernel<COS>, dim3(B, (d + 255) / 256), dim3(256), 0, (hipStream_t)stream, dl, lg, q, p, inv, dq, B, N, Np, d,
                       mode, scale);
    CLDRD_LAUNCH_CHECK();
    hipLaunchKernelGGL(score_bwd_p_kernel<COS>, dim3(B * N), dim3(256), 0, (hipStream_t)stream, dl, lg, q, p, inv, dp, B, N, Np, d, mode, scale);
    CLDRD_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" int cldrd_score_fwd(const float* q, const float* p, float* logits, int B, int N, int d, int mode, void* stream) {
    CLDRD_CHECK(B > 0 && N > 0 && d > 0 && d % 4 == 0 && mode >= 0 && mode <= 2, "score_fwd: bad arguments");
    return launch_score_fwd<false>(q, p, nullptr, logits, B, N, d, mode, 1.f, stream);
}

extern "C" int cldrd_score_bwd(const float* dlogits, const float* q, const float* p, float* dq, float* dp, int B, int N, int d,
                               int mode, void* stream) {
    CLDRD_CHECK(B > 0 && N > 0 && d > 0 && mode >= 0 && mode <= 2, "score_bwd: bad arguments");
    return launch_score_bwd<false>(dlogits, nullptr, q, p, nullptr, dq, dp, B, N, d, mode, 1.f, stream);
}

extern "C" int cldrd_score_cos_fwd(const float* q, const float* p, float* logits, float* inv_norms, int B, int N, int d, int mode, float scale,
                                   float eps, void* stream) {
    CLDRD_CHECK(q && p && logits && inv_norms, "score_cos_fwd: null pointer");
    CLDRD_CHECK(B > 0 && N > 0, "score_cos_fwd: need B > 0 and N > 0");
    CLDRD_CHECK(d > 0 && d % 4 == 0, "score_cos_fwd: need d > 0 and d % 4 == 0");
    CLDRD_CHECK(mode >= 0 && mode <= 2, "score_cos_fwd: mode must be 0, 1 or 2");
    CLDRD_CHECK(scale > 0.f && scale <= FLT_MAX, "score_cos_fwd: scale must be finite and > 0");
    CLDRD_CHECK(eps > 0.f, "score_cos_fwd: eps must be > 0");
    const int rows = B + B * N;
    hipLaunchKernelGGL(cos_inv_norm_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, q, p, inv_norms, B, rows, d, eps);
    CLDRD_LAUNCH_CHECK();
    return launch_score_fwd<true>(q, p, inv_norms, logits, B, N, d, mode, scale, stream);
}

extern "C" int cldrd_score_cos_bwd(const float* dlogits, const float* logits, const float* q, const float* p, const float* inv_norms, float* dq,
                                   float* dp, int B, int N, int d, int mode, float scale, void* stream) {
    CLDRD_CHECK(dlogits && logits && q && p && inv_norms && dq && dp, "score_cos_bwd: null pointer");
    CLDRD_CHECK(B > 0 && N > 0, "score_cos_bwd: need B > 0 and N > 0");
    CLDRD_CHECK(d > 0 && d % 4 == 0, "score_cos_bwd: need d > 0 and d % 4 == 0");
    CLDRD_CHECK(mode >= 0 && mode <= 2, "score_cos_bwd: mode must be 0, 1 or 2");
    CLDRD_CHECK(scale > 0.f && scale <= FLT_MAX, "score_cos_bwd: scale must be finite and > 0");
    return launch_score_bwd<true>(dlogits, logits, q, p, inv_norms, dq, dp, B, N, d, mode, scale, stream);
}

extern "C" int cldrd_l2_normalize_rows(const float* x, size_t ld_x, float* out, size_t n, int d, float eps, void* stream) {
    CLDRD_CHECK(x && out, "l2_normalize_rows: null pointer");
    CLDRD_CHECK(d > 0 && d % 4 == 0, "l2_normalize_rows: need d > 0 and d % 4 == 0");
    CLDRD_CHECK(ld_x >= (size_t)d && ld_x % 4 == 0, "l2_normalize_rows: need ld_x >= d and ld_x % 4 == 0");
    CLDRD_CHECK(eps > 0.f, "l2_normalize_rows: eps must be > 0");
    CLDRD_CHECK(x != out || ld_x == (size_t)d, "l2_normalize_rows: in place needs ld_x == d");
    CLDRD_CHECK((n + 3) / 4 <= 0x7fffffffull, "l2_normalize_rows: too many rows");
    if (n == 0) return 0;
    hipLaunchKernelGGL(l2_normalize_rows_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, x, ld_x, out, n, d, eps);
    CLDRD_LAUNCH_CHECK();
    return 0;
}

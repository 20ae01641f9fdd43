// The fp32 evaluation pass of the encoder (HipEncoder.encode(fp32=True); the reference's `use_fp16=False` encode, retriever/retrieval_utils.py:30-58):
// a Linear layer and the attention of one layer with EVERY operand in fp32, on the f32-input MFMA of gfx950 (v_mfma_f32_32x32x2_f32: bit for bit a
// k-ordered fmaf chain, one rounding per product, at 1/16 of the 16-bit MFMA rate).  Evaluation only: no dropout, no tape, no LSE, no keep bits.
// What is already fp32 elsewhere is reused unchanged (cldrd_embed_ln_fwd / cldrd_layernorm_fwd with out32, cldrd_gather_rows, cldrd_cls_head_fwd).
//
// The property the pass is built for: a ROW's result does not depend on which other rows share the launch.  That is what makes the mode a yardstick
// (packed == padded, a batch == its sequences encoded alone, all bit for bit), and it is why both kernels have ONE schedule:
//
// cldrd_gemm_nt_f32   C[M,N] = A[M,K] . W[N,K]^T (+ bias) (erf-GELU) (+ residual).  One tile configuration for every M: 128 x 128 x 32 per workgroup,
//   4 waves, each 2 x 2 tiles of 32 x 32; no split-K, no small-M variant.  A and W tiles go global -> registers -> LDS (rows padded to 36 floats: 16-byte
//   aligned rows whose b128 reads spread over the banks); the next K tile's global loads are issued before the current tile's MFMAs.  No ring, no
//   LDS-DMA: at 64 cycles per MFMA the operand traffic is far from the limit.  K order, the same for every output element: K tiles ascending; inside
//   a tile step (q, j), q = 0..3, j = 0..3, adds k = 4 q + j and then k = 16 + 4 q + j (lane half h of the MFMA holds k = 16 h + 4 q + j, so that a
//   lane fetches its 16 values of a row as four float4).  Rows >= M and weight rows >= N are read as zeros and never stored.
//   W is the fp32 master weight, read in place.  GELU = 0.5 x (1 + erff(x / sqrt 2)) with libm-grade erff, no fast-math intrinsic.
//
// cldrd_attention_fwd_f32 / cldrd_attention_cls_fwd_f32   softmax(Q K^T / 8 + key mask) . V, head dim 64, L <= 256, padded rows + int64 mask or
//   packed rows through cu_rows (the _hd32 pair: the same kernel at head dim 32, scale 1 / sqrt(32), see attention_f32_kernel).  Chosen schedule: STREAMING 32-key blocks with an online softmax, no LDS at all.  One wave owns 32 queries of one
//   (sequence, head); per key block it computes S^T = K_blk . Q^T (keys in the accumulator rows, queries on the lanes: the softmax reductions run
//   over a lane's own 16 registers plus one exchange between the lane halves), and the accumulator tile is then the A operand of P . V as it
//   stands (a product that sums over the tile's row index needs no lane movement).  K rows (as MFMA A operand) and V elements (as B operand)
//   are fetched straight from global memory / L2 into the operand registers: at 4096 MFMA cycles per key block there is nothing to gain from staging.
//   Fixed order: key blocks ascending; head-dim chain of a score 0, 32, 1, 33, ...; keys of a block enter P . V as 0, 4, 1, 5, 2, 6, 3, 7, 8, 12, ...
//   A masked key has p = 0 exactly and its V value is replaced by 0; a key block without any valid key is skipped.  So the padded and the packed
//   layout of the same sequences run the same operations on the same numbers: same bits, at every L.  A sequence without any valid key gives zeros.
//   The CLS form is the same kernel body given one query row per sequence (qc, with a pitch) and K | V rows of width 2 d: bit for bit row 0
//   of the full form.  Queries of a wave's tile beyond the sequence are computed on a clamped row and not stored.
#include "common.h"
#include <cstdio>

namespace {

constexpr int GT = 128;          // tile rows / columns of the GEMM workgroup
constexpr int GK = 32;           // K tile
constexpr int GLD = 36;          // LDS row pitch in floats

__device__ __forceinline__ float gelu_erf_f32(float x) { return 0.5f * x * (1.0f + erff(x * 0.70710678118654752f)); }

__global__ __launch_bounds__(256) void gemm_nt_f32_kernel(const float* __restrict__ A, const float* __restrict__ W, float* __restrict__ C, int M, int N,
                                                           int K, int lda, int ldw, int ldc, const float* __restrict__ bias,
                                                           const float* __restrict__ residual, int ldr, int act) {
    __shared__ __attribute__((aligned(16))) float As[GT * GLD];
    __shared__ __attribute__((aligned(16))) float Ws[GT * GLD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.y * GT, n0 = blockIdx.x * GT;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    const int r = lane & 31, h = lane >> 5;
    // global -> register staging: float4 number idx = tid + 256 i of a [128][32] tile: row idx >> 3, columns 4 (idx & 7) ..
    float4 ga[4], gw[4];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = tid + 256 * i, row = idx >> 3, c = (idx & 7) * 4;
            ga[i] = (m0 + row < M) ? *(const float4*)(A + (size_t)(m0 + row) * lda + k0 + c) : make_float4(0.f, 0.f, 0.f, 0.f);
            gw[i] = (n0 + row < N) ? *(const float4*)(W + (size_t)(n0 + row) * ldw + k0 + c) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;
    fetch(0);
    for (int k0 = 0; k0 < K; k0 += GK) {
        __syncthreads();                    // the previous tile's reads are done
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = tid + 256 * i, row = idx >> 3, c = (idx & 7) * 4;
            *(float4*)(As + row * GLD + c) = ga[i];
            *(float4*)(Ws + row * GLD + c) = gw[i];
        }
        __syncthreads();
        if (k0 + GK < K) fetch(k0 + GK);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float4 a[2], w[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                a[t] = *(const float4*)(As + (wm + 32 * t + r) * GLD + 16 * h + 4 * q);
                w[t] = *(const float4*)(Ws + (wn + 32 * t + r) * GLD + 16 * h + 4 * q);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int ta = 0; ta < 2; ++ta)
#pragma unroll
                    for (int tb = 0; tb < 2; ++tb) {
                        const float av = j == 0 ? a[ta].x : j == 1 ? a[ta].y : j == 2 ? a[ta].z : a[ta].w;
                        const float wv = j == 0 ? w[tb].x : j == 1 ? w[tb].y : j == 2 ? w[tb].z : w[tb].w;
                        acc[ta][tb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, wv, acc[ta][tb], 0, 0, 0);
                    }
        }
    }
    // epilogue: accumulator element e of lane (r, h) is row (e & 3) + 8 (e >> 2) + 4 h, column r of its 32 x 32 tile
#pragma unroll
    for (int ta = 0; ta < 2; ++ta)
#pragma unroll
        for (int tb = 0; tb < 2; ++tb) {
            const int n = n0 + wn + 32 * tb + r;
            if (n >= N) continue;
            const float bv = bias ? bias[n] : 0.f;
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int m = m0 + wm + 32 * ta + (e & 3) + 8 * (e >> 2) + 4 * h;
                if (m >= M) continue;
                float v = acc[ta][tb][e];
                if (bias) v += bv;
                if (act & 1) v = gelu_erf_f32(v);
                if (residual) v += residual[(size_t)m * ldr + n];
                C[(size_t)m * ldc + n] = v;
            }
        }
}

// One wave = 32 queries of one (sequence, head).  q / k / v / o: element 0 of the first row; ld*: row pitches in floats.
// CLS form: q_per_seq != 0: one query row per sequence (row m of q, pitch ldq; output row m of o).
// DH: the head dim, 64 or 32.  Lane half h holds head dims DH/2 h .. DH/2 h + DH/2 - 1 of its Q / K row, so the chain of a score adds the head dims
// 0, DH/2, 1, DH/2 + 1, ... (DH = 32: 0, 16, 1, 17, ..., 15, 31), and the context is DH / 32 accumulator tiles of 32 head dims.  The finished score
// is multiplied ONCE by 1 / sqrt(DH): 0.125, exact, at 64; at 32 the fp32 nearest to 1 / sqrt(32), which is no power of two - the product rounds
// once more (two relative errors of 2^-24 on the score, paid for in the tests' bound).  Everything else - key order, masking, skipping - is the
// same text for both.
template <int DH>
__global__ __launch_bounds__(256) void attention_f32_kernel(const float* __restrict__ q, int ldq, const float* __restrict__ k, const float* __restrict__ v,
                                                             int ldkv, float* __restrict__ o, int ldo, const long long* __restrict__ mask,
                                                             const int* __restrict__ cu, int L, int H, int q_per_seq) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int m = blockIdx.x / H, head = blockIdx.x % H;
    const int qt = blockIdx.y * (blockDim.x >> 6) + wave;
    int row0, klen;
    if (cu) {
        row0 = cu[m];
        klen = cu[m + 1] - row0;
        klen = klen < 0 ? 0 : (klen > L ? L : klen);
    } else {
        row0 = m * L;
        klen = L;
    }
    const int nq = q_per_seq ? 1 : klen;
    if (qt * 32 >= nq) return;
    // Q fragment (B operand): query qt * 32 + r (clamped to the sequence), head dims 32 h .. 32 h + 31
    const int qi = min(qt * 32 + r, nq - 1);
    constexpr int HB = DH / 2;            // head dims per lane half
    constexpr float SCALE = DH == 64 ? 0.125f : 0.17677669529663688110f;
    const float* qrow = q_per_seq ? q + (size_t)m * ldq + head * DH : q + (size_t)(row0 + qi) * ldq + head * DH;
    float qf[HB];
#pragma unroll
    for (int i = 0; i < HB / 4; ++i) {
        const float4 t = *(const float4*)(qrow + HB * h + 4 * i);
        qf[4 * i] = t.x; qf[4 * i + 1] = t.y; qf[4 * i + 2] = t.z; qf[4 * i + 3] = t.w;
    }
    f32x16 o0, o1;                       // context, head dims r and 32 + r of query (e & 3) + 8 (e >> 2) + 4 h
#pragma unroll
    for (int e = 0; e < 16; ++e) { o0[e] = 0.f; o1[e] = 0.f; }
    float mrun = -INFINITY, lrun = 0.f;  // running max / sum of query r (both lane halves hold the same values)
    const int nblk = (klen + 31) >> 5;
    for (int kb = 0; kb < nblk; ++kb) {
        const int key = kb * 32 + r;
        bool ok = key < klen;
        if (ok && mask) ok = mask[(size_t)m * L + key] != 0;
        const unsigned long long valid = __ballot(ok) & 0xFFFFFFFFull;       // bit j: key kb * 32 + j takes part
        if (valid == 0ull) continue;                                        // (wave-uniform)
        // K fragment (A operand): key row, clamped into the sequence; head dims as Q
        const float* krow = k + (size_t)(row0 + min(key, klen - 1)) * ldkv + head * DH + HB * h;
        float kf[HB];
#pragma unroll
        for (int i = 0; i < HB / 4; ++i) {
            const float4 t = *(const float4*)(krow + 4 * i);
            kf[4 * i] = t.x; kf[4 * i + 1] = t.y; kf[4 * i + 2] = t.z; kf[4 * i + 3] = t.w;
        }
        // V elements (B operand of P . V): step t of lane half h takes key (t & 3) + 8 (t >> 2) + 4 h, head dims r and 32 + r
        float v0[16], v1[16];
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            const int j = (t & 3) + 8 * (t >> 2) + 4 * h;
            const bool vj = (valid >> j) & 1ull;
            const float* vrow = v + (size_t)(row0 + min(kb * 32 + j, klen - 1)) * ldkv + head * DH;
            const float a = vrow[r], b = DH == 64 ? vrow[DH - 32 + r] : 0.f;
            v0[t] = vj ? a : 0.f;
            v1[t] = vj ? b : 0.f;
        }
        f32x16 s;
#pragma unroll
        for (int e = 0; e < 16; ++e) s[e] = 0.f;
#pragma unroll
        for (int i = 0; i < HB; ++i) s = __builtin_amdgcn_mfma_f32_32x32x2f32(kf[i], qf[i], s, 0, 0, 0);
        // s[e]: score of key (e & 3) + 8 (e >> 2) + 4 h (block-relative) and query r
        float mx = -INFINITY;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int j = (e & 3) + 8 * (e >> 2) + 4 * h;
            s[e] = ((valid >> j) & 1ull) ? s[e] * SCALE : -INFINITY;
            mx = fmaxf(mx, s[e]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float mnew = fmaxf(mrun, mx);                                  // finite: the block has a valid key
        const float alpha = mrun == -INFINITY ? 0.f : expf(mrun - mnew);
        float ps = 0.f;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const float p = s[e] == -INFINITY ? 0.f : expf(s[e] - mnew);
            s[e] = p;
            ps += p;
        }
        ps += __shfl_xor(ps, 32, 64);
        lrun = lrun * alpha + ps;
        mrun = mnew;
        // rescale the context rows: row (e & 3) + 8 (e >> 2) + 4 h needs the alpha of that query, which lives on lane = query
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const float ar = __shfl(alpha, (e & 3) + 8 * (e >> 2) + 4 * h, 64);
            o0[e] *= ar;
            if constexpr (DH == 64) o1[e] *= ar;
        }
#pragma unroll
        for (int t = 0; t < 16; ++t) {
            o0 = __builtin_amdgcn_mfma_f32_32x32x2f32(s[t], v0[t], o0, 0, 0, 0);
            if constexpr (DH == 64) o1 = __builtin_amdgcn_mfma_f32_32x32x2f32(s[t], v1[t], o1, 0, 0, 0);
        }
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int qq = (e & 3) + 8 * (e >> 2) + 4 * h;
        const float lr = __shfl(lrun, qq, 64);
        const int qabs = qt * 32 + qq;
        if (qabs >= nq) continue;
        float* orow = q_per_seq ? o + (size_t)m * ldo + head * DH : o + (size_t)(row0 + qabs) * ldo + head * DH;
        orow[r] = lr > 0.f ? o0[e] / lr : 0.f;
        if constexpr (DH == 64) orow[32 + r] = lr > 0.f ? o1[e] / lr : 0.f;
    }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" int cldrd_gemm_nt_f32(const float* A, const float* W, float* C, int M, int N, int K, int lda, int ldw, int ldc, const float* bias,
                                 const float* residual, int ldr, int act, void* stream) {
    CLDRD_CHECK(A != nullptr && W != nullptr, "gemm_nt_f32: null operand");
    CLDRD_CHECK(C != nullptr, "gemm_nt_f32: null output");
    CLDRD_CHECK(M > 0 && N > 0 && K > 0, "gemm_nt_f32: M, N, K must be positive");
    CLDRD_CHECK(K % 32 == 0, "gemm_nt_f32: K must be a multiple of 32");
    CLDRD_CHECK(N % 8 == 0, "gemm_nt_f32: N must be a multiple of 8");
    CLDRD_CHECK(lda >= K && ldw >= K && ldc >= N && lda % 4 == 0 && ldw % 4 == 0, "gemm_nt_f32: row pitches must cover a row (lda, ldw multiples of 4)");
    CLDRD_CHECK(aligned16(A) && aligned16(W), "gemm_nt_f32: A and W must be 16-byte aligned");
    CLDRD_CHECK(residual == nullptr || ldr >= N, "gemm_nt_f32: a residual needs its row pitch (ldr >= N)");
    CLDRD_CHECK((act & ~1) == 0, "gemm_nt_f32: act is 0 or 1 (erf-GELU)");
    CLDRD_CHECK((M + GT - 1) / GT <= 65535, "gemm_nt_f32: M too large");
    hipLaunchKernelGGL(gemm_nt_f32_kernel, dim3((N + GT - 1) / GT, (M + GT - 1) / GT), dim3(256), 0, (hipStream_t)stream, A, W, C, M, N, K, lda, ldw, ldc,
                       bias, residual, ldr, act);
    CLDRD_LAUNCH_CHECK();
    return 0;
}

namespace {

// The two attention entry points of a head dim DH: the argument checks (messages under the entry point's own name `op`) and the launch
int attn_f32_refuse(const char* op, const char* why) {
    char msg[160];
    snprintf(msg, sizeof(msg), "%s: %s", op, why);
    return cldrd_set_error(msg);
}
#define ATTN_F32_CHECK(cond, why) do { if (!(cond)) return attn_f32_refuse(op, why); } while (0)

template <int DH>
int attention_f32_full(const char* op, const float* qkv, const long long* mask, const int* cu_rows, float* ctx, int nseq, int L, int H, void* stream) {
    ATTN_F32_CHECK(qkv != nullptr, "null qkv");
    ATTN_F32_CHECK(ctx != nullptr, "null output");
    ATTN_F32_CHECK(mask == nullptr || cu_rows == nullptr, "a packed batch (cu_rows) takes its key mask from the lengths: mask must be NULL");
    ATTN_F32_CHECK(nseq > 0 && H > 0 && L > 0 && L <= 256, "need nseq > 0, H > 0, 0 < L <= 256");
    ATTN_F32_CHECK((long long)nseq * H <= 0x7FFFFFFFll && (long long)nseq * L * 3 * H * DH <= 0x7FFFFFFFFFFll, "batch too large");
    ATTN_F32_CHECK(aligned16(qkv), "qkv must be 16-byte aligned");
    const int d = H * DH;
    hipLaunchKernelGGL(attention_f32_kernel<DH>, dim3(nseq * H, (L + 127) / 128), dim3(256), 0, (hipStream_t)stream, qkv, 3 * d, qkv + d, qkv + 2 * d,
                       3 * d, ctx, d, mask, cu_rows, L, H, 0);
    CLDRD_LAUNCH_CHECK();
    return 0;
}

template <int DH>
int attention_f32_cls(const char* op, const float* qc, int ldq, const float* kv, const long long* mask, const int* cu_rows, float* ctx, int nseq, int L,
                      int H, void* stream) {
    ATTN_F32_CHECK(qc != nullptr && kv != nullptr, "null operand");
    ATTN_F32_CHECK(ctx != nullptr, "null output");
    ATTN_F32_CHECK(mask == nullptr || cu_rows == nullptr, "a packed batch (cu_rows) takes its key mask from the lengths: mask must be NULL");
    ATTN_F32_CHECK(nseq > 0 && H > 0 && L > 0 && L <= 256, "need nseq > 0, H > 0, 0 < L <= 256");
    ATTN_F32_CHECK((long long)nseq * H <= 0x7FFFFFFFll, "batch too large");
    ATTN_F32_CHECK(ldq >= H * DH && ldq % 4 == 0, "the query row pitch must cover a row and be a multiple of 4");
    ATTN_F32_CHECK(aligned16(qc) && aligned16(kv), "qc and kv must be 16-byte aligned");
    const int d = H * DH;
    hipLaunchKernelGGL(attention_f32_kernel<DH>, dim3(nseq * H, 1), dim3(64), 0, (hipStream_t)stream, qc, ldq, kv, kv + d, 2 * d, ctx, d, mask, cu_rows,
                       L, H, 1);
    CLDRD_LAUNCH_CHECK();
    return 0;
}

}  // namespace

extern "C" int cldrd_attention_fwd_f32(const float* qkv, const long long* mask, const int* cu_rows, float* ctx, int nseq, int L, int H, void* stream) {
    return attention_f32_full<64>("attention_fwd_f32", qkv, mask, cu_rows, ctx, nseq, L, H, stream);
}

extern "C" int cldrd_attention_cls_fwd_f32(const float* qc, int ldq, const float* kv, const long long* mask, const int* cu_rows, float* ctx, int nseq,
                                           int L, int H, void* stream) {
    return attention_f32_cls<64>("attention_cls_fwd_f32", qc, ldq, kv, mask, cu_rows, ctx, nseq, L, H, stream);
}

// Head dim 32: qkv [rows, 3*H*32], ctx [rows, H*32]; qc [nseq, H*32] with pitch ldq, kv [rows, 2*H*32].  Any H (no head pairs here: a wave owns one head).
extern "C" int cldrd_attention_fwd_f32_hd32(const float* qkv, const long long* mask, const int* cu_rows, float* ctx, int nseq, int L, int H,
                                            void* stream) {
    return attention_f32_full<32>("attention_fwd_f32_hd32", qkv, mask, cu_rows, ctx, nseq, L, H, stream);
}

extern "C" int cldrd_attention_cls_fwd_f32_hd32(const float* qc, int ldq, const float* kv, const long long* mask, const int* cu_rows, float* ctx,
                                                int nseq, int L, int H, void* stream) {
    return attention_f32_cls<32>("attention_cls_fwd_f32_hd32", qc, ldq, kv, mask, cu_rows, ctx, nseq, L, H, stream);
}

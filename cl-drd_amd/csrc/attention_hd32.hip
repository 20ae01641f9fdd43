// Fused multi-head self-attention at HEAD DIM 32, evaluation forward only: softmax(Q K^T / sqrt(32) + key mask) . V, sequences <= 256 tokens, no
// dropout, no LSE, no keep bits.  Reference call site: the cross-encoder teacher the reference names, cross-encoder/ms-marco-MiniLM-L-6-v2
// (evaluation/reranking_evaluator.py:292: hidden 384, 12 heads), and every other MiniLM-shaped BERT.  Training at head dim 32 does not exist.
//
// One workgroup owns one (sequence, PAIR of adjacent heads 2 p, 2 p + 1).  The pair's Q, K, V slices are the same 128-byte rows the head-dim-64 kernels
// load ([Lp, 64] tiles, RSB = 144, at column 64 p of each of Q | K | V), so load_tile, row_frag and tr_frag apply unchanged; columns 32 j .. 32 j + 31
// of a tile belong to head j of the pair.  H must be EVEN: the second head's slice then ends inside Q (K, V), and no 16-byte load reads past a row.
//
// A wave's unit of work is a (query block of 32, head j): S^T = K_kb . Q^T is two mfma_f32_32x32x16 over the 16-byte fragments s = 2 j, 2 j + 1
// (lane = query column, as in attention.hip), the softmax runs in the log2 domain with scale2 = (1 / sqrt(32)) log2(e) folded into one fp32
// constant, and P . V accumulates ONE transposed tile O^T[d][q] from tr_frag(sV, key, 32 j, lane).  One schedule for every tile height: STREAMING
// over the live key blocks with a running maximum (attn_fwd_kernel's loop at half the MFMAs per score).  The all-scores-in-registers form the
// head-dim-64 family runs up to L = 128 was not built: per score this kernel does half the MFMA work for the same exp / VALU work, so it is VALU-bound
// either way, and one body makes an item's bits a function of its length and the format ONLY - not of the tile height, the other items of the
// launch, their number or their order (the units of a workgroup share nothing but the read-only tiles).  The 2 NKB units of an item go round-robin
// over the waves with the head index fastest: a short sequence in a tall tile still spreads over the waves.
// The block loop is left early (kb >= nb): every iteration ends in mfma_drain(), see attention_common.h.
#include "attention_common.h"

namespace {

constexpr float SCALE2_HD32 = (float)(0.17677669529663688110 * 1.44269504088896340736);      // (1 / sqrt(32)) log2(e), rounded to fp32 once

template <int NKB, bool F16>
__global__ __launch_bounds__(NKB > 4 ? 512 : 256) void attn_fwd_hd32_kernel(const bf16_t* __restrict__ qkv, const int64_t* __restrict__ mask,
                                                                             bf16_t* __restrict__ ctx, int L, int H, bf16_t* __restrict__ ctx16,
                                                                             const int* __restrict__ cu, const int* __restrict__ seq_list) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int Lp = 32 * NKB;
    constexpr int NWAVES = NKB > 4 ? 8 : 4;
    char* sQ = smem;
    char* sK = sQ + Lp * RSB;
    char* sV = sK + Lp * RSB;
    float* sBias = (float*)(sV + Lp * RSB);
    const int HP = H >> 1;                                   // head pairs
    const int seq = seq_of(seq_list, blockIdx.x / HP), pair = blockIdx.x % HP;
    const SeqRows sr = seq_rows(cu, seq, L);
    const int dm = H * 32, ld = 3 * dm;
    const bf16_t* base = qkv + (size_t)sr.row0 * ld + pair * 64;
    load_tile(sQ, base, ld, sr.len, Lp);
    load_tile(sK, base + dm, ld, sr.len, Lp);
    load_tile(sV, base + 2 * dm, ld, sr.len, Lp);
    fill_key_bias(sBias, mask, seq, L, Lp, sr.len);
    __syncthreads();

    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const int nb = live_blocks(sr.len);
    for (int unit = wid; unit < 2 * NKB; unit += NWAVES) {
        const int qb = unit >> 1, j = unit & 1;
        if (qb >= nb) break;                                  // query blocks beyond the sequence: nothing to store (units ascend in qb)
        const int q = qb * 32 + r;
        bf16x8 qf[2];
#pragma unroll
        for (int s = 0; s < 2; ++s) qf[s] = row_frag(sQ, q, 2 * j + s, h);
        float m = NEG_BIG * 4.f, lsum = 0.f;                  // lsum: this half's share of the denominator
        f32x16 O[1] = {(f32x16){0.f}};                        // O[0][t] = ctx^T[d = rowmap(t, h)][q] of head j
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) {
            if (kb >= nb) break;
            f32x16 S = (f32x16){0.f};
#pragma unroll
            for (int s = 0; s < 2; ++s)
                S = mfma32<F16>(row_frag(sK, kb * 32 + r, 2 * j + s, h), qf[s], S);
            // S[t] = <K[key], Q[q]> with key = 32 kb + rowmap(t, h); keys rowmap(4u .. 4u+3, h) = 8u + 4h + 0..3 are consecutive
            float v[16];
            float mloc = NEG_BIG * 4.f;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float4 b4 = *(const float4*)(sBias + kb * 32 + 8 * u + 4 * h);
                const float bb[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
                for (int e = 0; e < 4; e += 2) {      // packed fp32: two keys per instruction
                    const cldrd_f32v2 w = fma2((cldrd_f32v2){S[4 * u + e], S[4 * u + e + 1]}, splat2(SCALE2_HD32), (cldrd_f32v2){bb[e], bb[e + 1]});
                    v[4 * u + e] = w.x; v[4 * u + e + 1] = w.y;
                    mloc = fmaxf(mloc, fmaxf(w.x, w.y));
                }
            }
            mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
            const float mn = fmaxf(m, mloc);
            const float alpha = __builtin_amdgcn_exp2f(m - mn);
            m = mn;
            float psum = 0.f;
#pragma unroll
            for (int t = 0; t < 16; t += 2) {
                const cldrd_f32v2 dv = (cldrd_f32v2){v[t], v[t + 1]} - splat2(mn);
                const float p0 = __builtin_amdgcn_exp2f(dv.x), p1 = __builtin_amdgcn_exp2f(dv.y);
                psum += p0 + p1;
                v[t] = p0; v[t + 1] = p1;
            }
            lsum = fmaf(lsum, alpha, psum);
#pragma unroll
            for (int t = 0; t < 16; t += 2) {
                const cldrd_f32v2 o2 = (cldrd_f32v2){O[0][t], O[0][t + 1]} * splat2(alpha);
                O[0][t] = o2.x; O[0][t + 1] = o2.y;
            }
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)       // operands as in attention.hip: O^T[d][q], a lane (= query) holds consecutive head dimensions
                O[0] = mfma32<F16>(tr_frag(sV, kb * 32 + 16 * s2 + 4 * h, 32 * j, lane), pack8x<F16>(v + 8 * s2), O[0]);
            mfma_drain();
        }
        const float l = lsum + __shfl_xor(lsum, 32, 64);
        store_ctx_rows<F16, true>(O, 1.0f / l, ctx, ctx16, ((size_t)sr.row0 + q) * dm + (2 * pair + j) * 32, h, q < sr.len);
    }
}

// CLS row only (the last encoder layer): attn_cls_fwd_kernel at 32 columns per head, without probabilities and without dropout.  One wavefront
// per (sequence, head); qc: [nseq, H*32], kv: [rows, 2*H*32] = K | V.
template <bool F16>
__global__ __launch_bounds__(64) void attn_cls_fwd_hd32_kernel(const bf16_t* __restrict__ qc, const bf16_t* __restrict__ kv,
                                                                const int64_t* __restrict__ mask, bf16_t* __restrict__ ctx, int L, int H,
                                                                bf16_t* __restrict__ ctx16, const int* __restrict__ cu) {
    __shared__ float sp[256];
    __shared__ float sq[32];
    __shared__ float so[16][32];
    const int seq = blockIdx.x / H, hd = blockIdx.x % H, lane = threadIdx.x;
    const int dm = H * 32;
    if (lane < 32) sq[lane] = x2f<F16>(qc[(size_t)seq * dm + hd * 32 + lane]);
    __syncthreads();
    const SeqRows sr = seq_rows(cu, seq, L);          // packed K | V rows: see seq_rows
    const int len = sr.len;
    const bf16_t* kb = kv + (size_t)sr.row0 * 2 * dm + hd * 32;
    const bf16_t* vb = kb + dm;
    constexpr float scale = 0.17677669529663688110f;       // the fp32 nearest to 1 / sqrt(32)
    float sc[4];
    float mx = -3.0e38f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int key = lane + 64 * i;
        float s = -1.0e30f;
        if (key < len && (!mask || mask[(size_t)seq * L + key] != 0)) {
            const bf16_t* kr = kb + (size_t)key * 2 * dm;
            float a = 0.f;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const uint4 u = *(const uint4*)(kr + c * 8);
                const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    a += x2f<F16>((bf16_t)(w[e] & 0xFFFFu)) * sq[c * 8 + 2 * e] + x2f<F16>((bf16_t)(w[e] >> 16)) * sq[c * 8 + 2 * e + 1];
            }
            s = a * scale;
        }
        sc[i] = s;
        mx = fmaxf(mx, s);
    }
    mx = wave_max(mx);
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) { sc[i] = __expf(sc[i] - mx); sum += (lane + 64 * i < L) ? sc[i] : 0.f; }
    sum = wave_sum(sum);
    const float inv = 1.0f / sum;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int key = lane + 64 * i;
        if (key < L) sp[key] = sc[i] * inv;
    }
    __syncthreads();
    // ctx = P V.  Four lanes share a key row (16 bytes = 8 features each), sixteen keys per instruction; the sixteen key groups are combined through LDS.
    const int c4 = lane & 3, g = lane >> 2;
    float o8[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o8[e] = 0.f;
    for (int k0 = 0; k0 < len; k0 += 16) {          // keys >= len: p = 0 and (padded layout) zero rows: + 0.0f, skipped
        const int key = k0 + g;
        if (key < len) {
            const float pk = sp[key];
            const uint4 u = *(const uint4*)(vb + (size_t)key * 2 * dm + c4 * 8);
            const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                o8[2 * e] += pk * x2f<F16>((bf16_t)(w[e] & 0xFFFFu));
                o8[2 * e + 1] += pk * x2f<F16>((bf16_t)(w[e] >> 16));
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) so[g][c4 * 8 + e] = o8[e];
    __syncthreads();
    if (lane < 32) {
        float o = 0.f;
#pragma unroll
        for (int gg = 0; gg < 16; ++gg) o += so[gg][lane];
        if (ctx) ctx[(size_t)seq * dm + hd * 32 + lane] = f2x<F16>(o);
        if (ctx16) ctx16[(size_t)seq * dm + hd * 32 + lane] = f2x<true>(o);       // fp16 copy of a bf16 pass (out-projection operand)
    }
}

template <int NKB, bool F16>
int launch_fwd_hd32(const bf16_t* qkv, const int64_t* mask, const int* cu, const int* seq_list, bf16_t* ctx, bf16_t* ctx16, int n, int L, int H,
                    hipStream_t st) {
    const size_t lds = 3 * 32 * NKB * RSB + 32 * NKB * sizeof(float);
    return attn_launch(attn_fwd_hd32_kernel<NKB, F16>, n * (H / 2), NKB > 4 ? 512 : 256, lds, st, qkv, mask, ctx, L, H, ctx16, cu, seq_list);
}

}  // namespace

// qkv: 16-bit [rows, 3*H*32] (Q | K | V, heads contiguous inside each), H even; ctx: [rows, H*32].  Layouts (mask / cu_rows / seq_list, n_list,
// Ltile) and formats: include/cldrd_hip.h.  A packed batch gives bit for bit the padded batch's real rows and writes nothing else.
extern "C" int cldrd_attention_fwd_hd32(const void* qkv, const long long* mask, const int* cu_rows, const int* seq_list, int n_list, int Ltile,
                                        void* ctx, int nseq, int L, int H, int fmt, void* ctx_f16_copy, void* stream) {
    if (attn_check("attention_fwd_hd32", mask, cu_rows, seq_list, n_list, Ltile, nseq, L, H)) return 1;
    CLDRD_CHECK(H % 2 == 0, "attention_fwd_hd32: head dim 32 needs an even number of heads (a workgroup loads a pair of adjacent heads)");
    CLDRD_CHECK(fmt == CLDRD_FMT_BF16 || fmt == CLDRD_FMT_F16, "attention_fwd_hd32: fmt is 0 (bf16) or 1 (fp16)");
    CLDRD_CHECK(ctx != nullptr || ctx_f16_copy != nullptr, "attention_fwd_hd32: no output");
    CLDRD_CHECK(!(fmt != CLDRD_FMT_BF16 && (ctx_f16_copy != nullptr || ctx == nullptr)), "attention_fwd_hd32: the fp16 pass writes ctx only");
    const int n = seq_list ? n_list : nseq;          // sequences of THIS launch (items = n x H / 2)
    const int Lt = seq_list ? Ltile : L;             // rows a sequence of this launch can have: the kernel's tile height
    const hipStream_t st = (hipStream_t)stream;
    if (fmt == CLDRD_FMT_F16)
        return with_nkb<8>((Lt + 31) / 32, [&](auto k) {
            return launch_fwd_hd32<decltype(k)::value, true>((const bf16_t*)qkv, (const int64_t*)mask, cu_rows, seq_list, (bf16_t*)ctx, nullptr, n, L, H, st);
        });
    return with_nkb<8>((Lt + 31) / 32, [&](auto k) {
        return launch_fwd_hd32<decltype(k)::value, false>((const bf16_t*)qkv, (const int64_t*)mask, cu_rows, seq_list, (bf16_t*)ctx,
                                                          (bf16_t*)ctx_f16_copy, n, L, H, st);
    });
}

// qc: 16-bit [nseq, H*32] (CLS queries); kv: [rows, 2*H*32] = K | V (padded, or packed with cu_rows); ctx: [nseq, H*32]
extern "C" int cldrd_attention_cls_fwd_hd32(const void* qc, const void* kv, const long long* mask, const int* cu_rows, void* ctx, int nseq, int L,
                                            int H, int fmt, void* ctx_f16_copy, void* stream) {
    if (attn_check("attention_cls_fwd_hd32", mask, cu_rows, nullptr, 0, 0, nseq, L, H)) return 1;
    CLDRD_CHECK(H % 2 == 0, "attention_cls_fwd_hd32: head dim 32 needs an even number of heads");
    CLDRD_CHECK(fmt == CLDRD_FMT_BF16 || fmt == CLDRD_FMT_F16, "attention_cls_fwd_hd32: fmt is 0 (bf16) or 1 (fp16)");
    CLDRD_CHECK(ctx != nullptr || ctx_f16_copy != nullptr, "attention_cls_fwd_hd32: no output");
    CLDRD_CHECK(!(fmt != CLDRD_FMT_BF16 && (ctx_f16_copy != nullptr || ctx == nullptr)), "attention_cls_fwd_hd32: the fp16 pass writes ctx only");
    CLDRD_CHECK(qc != nullptr && kv != nullptr, "attention_cls_fwd_hd32: null operand");
    if (fmt == CLDRD_FMT_F16)
        hipLaunchKernelGGL(attn_cls_fwd_hd32_kernel<true>, dim3(nseq * H), dim3(64), 0, (hipStream_t)stream, (const bf16_t*)qc, (const bf16_t*)kv,
                           (const int64_t*)mask, (bf16_t*)ctx, L, H, (bf16_t*)nullptr, cu_rows);
    else
        hipLaunchKernelGGL(attn_cls_fwd_hd32_kernel<false>, dim3(nseq * H), dim3(64), 0, (hipStream_t)stream, (const bf16_t*)qc, (const bf16_t*)kv,
                           (const int64_t*)mask, (bf16_t*)ctx, L, H, (bf16_t*)ctx_f16_copy, cu_rows);
    CLDRD_LAUNCH_CHECK();
    return 0;
}

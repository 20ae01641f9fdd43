// Fused multi-head self-attention for the BERT/DistilBERT encoder, forward and backward.
//
// Reference call site: HF DistilBertSelfAttention / BertSelfAttention reached from
// models/nway_dual_encoder.py:52,56,64: softmax(Q K^T / sqrt(dh) + key mask) -> dropout -> . V,
// dh = 64, sequences <= 256 tokens.  One workgroup owns one (sequence, head): Q, K, V (and dO) live in LDS
// for the whole kernel, so the L x L score matrix never touches HBM and no cross-workgroup reduction exists.
//
// MFMA 32x32x16 bf16 throughout.  Forward computes S^T = K Q^T so that a lane owns one query column: the
// row softmax is a register-local reduction plus one cross-half shuffle, and the S^T accumulator tile is
// reused directly as the A operand of P.V (cdna_hip_programming.md section 3, "accumulator tile as the next MFMA's
// operand"); V is consumed through ds_read_b64_tr_b16 transposing reads.  Backward recomputes P from the
// saved log-sum-exp in two sweeps: key-on-lane (dK, dV accumulate in registers over all query blocks) and
// query-on-lane (dQ accumulates over all key blocks).  Probabilities and dS are rounded to bf16 only as
// MFMA operands; softmax statistics, LSE and delta are fp32.
#include "attention_common.h"      // the LDS tile and its fragment reads, format switches, packed-batch row map, context stores, launch helper

namespace {

// ---------------------------------------------------------------------------------------------------------------
// Every pass exists in two launch forms: ONE ITEM per workgroup (load -> barrier -> compute), and PERSISTENT (one workgroup per CU walks its items
// and fetches the next one under the arithmetic of the current one).  The forms differ in how an item's tiles reach LDS and in nothing else: the
// arithmetic of a block - and the stores behind it - is one function below, called by both kernels of a pair, which is why the pair gives the same
// bits (the tests flip cldrd_set_tuning("attn_fwd2" / "attn_bwd2", 0) and compare).  One exception: the streaming forward pair (attn_fwd_kernel /
// attn_fwd3_kernel) shares prologue and stores, but each kernel carries the block loop itself (see attn_fwd3_kernel).

// Prologue of the one-item kernels: the item's Q, K, V head slices into their LDS tiles (rows >= its length zero).  With the bias fill below, the
// caller's __syncthreads() completes it.
__device__ __forceinline__ void load_item_tiles(char* sQ, char* sK, char* sV, const bf16_t* __restrict__ qkv, int hd, SeqRows sr, int H, int Lp) {
    const int dm = H * 64, ld = 3 * dm;
    const bf16_t* base = qkv + (size_t)sr.row0 * ld + hd * 64;
    load_tile(sQ, base, ld, sr.len, Lp);
    load_tile(sK, base + dm, ld, sr.len, Lp);
    load_tile(sV, base + 2 * dm, ld, sr.len, Lp);
}

// LSE of query q (log2 domain in, natural log out): lanes r and r + 32 hold the same value, the lower half stores it.  A query block beyond the
// sequence passes (0, len): the closed form of its zero rows (see seq_rows).
__device__ __forceinline__ void store_lse(float* __restrict__ lse, int seq, int hd, int H, int L, int q, int h, float m, float l) {
    if (h == 0 && q < L && lse) lse[((size_t)seq * H + hd) * L + q] = (m + __log2f(l)) * LN2;
}


// Where the all-scores forward takes its dropout keep decisions from.  row(rowidx, q) once per query: mask row rowidx = (seq*H + hd)*L + q;
// pair(p, kb, t, h) zeroes the dropped ones of the two probabilities of keys 32 kb + rowmap(t, h) and + 1 (a column pair of the mask).
struct KeepHash {                 // hashed on the spot (common.h): the one-item kernel
    uint64_t seed; uint32_t thresh; uint32_t rk;
    __device__ __forceinline__ void row(uint32_t rowidx, int) { rk = drop_rowkey(seed, rowidx); }
    __device__ __forceinline__ void pair(cldrd_f32v2& p, int kb, int t, int h) const {
        const uint32_t hh = drop_pair(rk, (uint32_t)(kb * 32 + rowmap(t, h)));
        p.x = drop_keep_lo(hh, thresh) ? p.x : 0.f;
        p.y = drop_keep_hi(hh, thresh) ? p.y : 0.f;
    }
};
template <int Lp>
struct KeepBits {                 // the loader waves' dword [kb][q] in LDS (attn_fwd2_kernel): two adjacent bits
    const uint32_t* sBits; int q;
    __device__ __forceinline__ void row(uint32_t, int q_) { q = q_; }
    __device__ __forceinline__ void pair(cldrd_f32v2& p, int kb, int t, int h) const {
        const uint32_t w = sBits[kb * Lp + q] >> (4 * h);
        p.x = keep_bit(p.x, w, rowmap(t, 0));
        p.y = keep_bit(p.y, w, rowmap(t, 0) + 1);
    }
};

// DROP is a template parameter: as a run-time test hipcc branched on it per element (16 branches per MFMA tile, with the
// accumulators re-read from AGPRs on both sides), which made these kernels VALU-bound.
//
// All-scores forward of one query block (L <= 128): Q fragments -> 16 NKB score accumulators -> softmax -> P.V -> LSE and context rows.  Called by one wave
// with the item's tiles complete in LDS; shared by attn_fwd_full_kernel and attn_fwd2_kernel, which differ in `keep` only.
template <int NKB, bool DROP, bool F16, class Keep>
__device__ __forceinline__ void fwd_full_block(const char* sQ, const char* sK, const char* sV, const float* sBias, Keep keep, int qb, int nb, int lane,
                                               int seq, int hd, SeqRows sr, int L, int H, float scale, float drop_scale, bf16_t* __restrict__ ctx,
                                               bf16_t* __restrict__ ctx16, float* __restrict__ lse) {
    const int r = lane & 31, h = lane >> 5;
    bf16x8 qf[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[s] = row_frag(sQ, qb * 32 + r, s, h);
    f32x16 S[NKB];
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
        if (kb >= nb) break;
        S[kb] = (f32x16){0.f};
#pragma unroll
        for (int s = 0; s < 4; ++s)
            S[kb] = mfma32<F16>(row_frag(sK, kb * 32 + r, s, h), qf[s], S[kb]);
        mfma_drain();
    }
    // S[kb][t] = <K[key], Q[q]> with key = 32 kb + rowmap(t, h), q = 32 qb + r
    // softmax in the log2 domain (v_exp_f32 is 2^x): scores * scale * log2(e) + bias, bias read 4 keys at a time
    // (keys rowmap(4u .. 4u+3, h) = 8u + 4h + 0..3 are consecutive)
    const float scale2 = scale * LOG2E;
    float mx = NEG_BIG * 4.f;
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (kb >= nb) break;
            const float4 b4 = *(const float4*)(sBias + kb * 32 + 8 * u + 4 * h);
            const float bb[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
            for (int j = 0; j < 4; j += 2) {      // two keys per packed fp32 instruction (v_pk_fma_f32: same IEEE results as two v_fma_f32)
                const cldrd_f32v2 v = fma2((cldrd_f32v2){S[kb][4 * u + j], S[kb][4 * u + j + 1]}, splat2(scale2), (cldrd_f32v2){bb[j], bb[j + 1]});
                S[kb][4 * u + j] = v.x; S[kb][4 * u + j + 1] = v.y;
                mx = fmaxf(mx, fmaxf(v.x, v.y));
            }
        }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    float sum = 0.f;
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb)
#pragma unroll
        for (int t = 0; t < 16; t += 2) {
            if (kb >= nb) break;
            const cldrd_f32v2 d = (cldrd_f32v2){S[kb][t], S[kb][t + 1]} - splat2(mx);
            const float e0 = __builtin_amdgcn_exp2f(d.x), e1 = __builtin_amdgcn_exp2f(d.y);
            S[kb][t] = e0; S[kb][t + 1] = e1;
            sum += e0;
            sum += e1;
        }
    sum += __shfl_xor(sum, 32, 64);
    const int q = qb * 32 + r;
    store_lse(lse, seq, hd, H, L, q, h, mx, sum);
    const float inv = 1.0f / sum;
    // dropout mask element (row, col) = ((seq*H + hd)*L + q, key); keys rowmap(t, h), t even / odd, are a column pair
    keep.row((uint32_t)((seq * H + hd) * L + q), q);
    f32x16 O[2] = {(f32x16){0.f}, (f32x16){0.f}};
#pragma unroll
    for (int kb = 0; kb < NKB; ++kb) {
        if (kb >= nb) break;
        float pv[16];
#pragma unroll
        for (int t = 0; t < 16; t += 2) {
            cldrd_f32v2 p = (cldrd_f32v2){S[kb][t], S[kb][t + 1]} * splat2(inv);
            if (DROP) {
                p = p * splat2(drop_scale);
                keep.pair(p, kb, t, h);
            }
            pv[t] = p.x; pv[t + 1] = p.y;
        }
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            const bf16x8 pa = pack8x<F16>(pv + 8 * s2);
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)      // operands swapped: O^T[d][q], so that a lane (= query) holds consecutive head dimensions
                O[dt] = mfma32<F16>(tr_frag(sV, kb * 32 + 16 * s2 + 4 * h, dt * 32, lane), pa, O[dt]);
        }
        mfma_drain();
    }
    store_ctx_rows<F16, false>(O, 1.0f, ctx, ctx16, ((size_t)sr.row0 + q) * (H * 64) + hd * 64, h, q < sr.len);
}

// Forward with all the scores of a query block in registers (16 NKB accumulators): for L <= 128 this is ~7 % faster than the
// streaming form below (16 score MFMAs back to back, one softmax pass, 16 P.V MFMAs) and is what the train step uses.
template <int NKB, bool DROP, bool F16 = false>
__global__ __launch_bounds__(256) void attn_fwd_full_kernel(const bf16_t* __restrict__ qkv, const int64_t* __restrict__ mask,
                                                        bf16_t* __restrict__ ctx, float* __restrict__ lse, int L, int H,
                                                        float scale, uint32_t drop_thresh, float drop_scale, SeedArg seed_a,
                                                        bf16_t* __restrict__ ctx16, const int* __restrict__ cu, const int* __restrict__ seq_list) {
    const uint64_t seed = seed_a.get();
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int Lp = 32 * NKB;
    char* sQ = smem;
    char* sK = sQ + Lp * RSB;
    char* sV = sK + Lp * RSB;
    float* sBias = (float*)(sV + Lp * RSB);
    const int seq = seq_of(seq_list, blockIdx.x / H), hd = blockIdx.x % H;
    const SeqRows sr = seq_rows(cu, seq, L);
    load_item_tiles(sQ, sK, sV, qkv, hd, sr, H, Lp);
    fill_key_bias(sBias, mask, seq, L, Lp, sr.len);
    __syncthreads();

    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int nb = live_blocks(sr.len);
    for (int qb = wid; qb < NKB; qb += 4) {
        if (qb >= nb)         // a query block beyond the sequence: nothing to store but the LSE of its zero rows
            store_lse(lse, seq, hd, H, L, qb * 32 + (lane & 31), lane >> 5, 0.f, (float)sr.len);
        else
            fwd_full_block<NKB, DROP, F16>(sQ, sK, sV, sBias, KeepHash{seed, drop_thresh, 0u}, qb, nb, lane, seq, hd, sr, L, H, scale, drop_scale, ctx,
                                           ctx16, lse);
    }
}

// Forward for L <= 128 and many (sequence, head) items: one persistent 8-wave workgroup per CU.  Waves 0..3 compute (fwd_full_block, one
// query block each; their keep decisions are the loader's bits in LDS), waves 4..7 only move data: they issue the global loads of the NEXT
// item's Q, K, V into registers, wait, and write them to the second LDS buffer - so an item's HBM latency sits under the previous item's
// arithmetic instead of in front of its own (the kernel above does load -> barrier -> compute per workgroup and overlaps only across the
// two workgroups a CU can hold).  One __syncthreads per item.
template <int NKB, bool DROP, bool F16 = false>
__global__ __launch_bounds__(512) void attn_fwd2_kernel(const bf16_t* __restrict__ qkv, const int64_t* __restrict__ mask,
                                                         bf16_t* __restrict__ ctx, float* __restrict__ lse, int L, int H,
                                                         float scale, uint32_t drop_thresh, float drop_scale, SeedArg seed_a, int nitems,
                                                         uint32_t* __restrict__ bits_out, bf16_t* __restrict__ ctx16, const int* __restrict__ cu, const int* __restrict__ seq_list) {
    const uint64_t seed = seed_a.get();
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int Lp = 32 * NKB;
    constexpr int TILE = Lp * RSB;
    constexpr int NBITS = DROP ? Lp * NKB : 0;          // dropout keep bits of an item: dword [kb][q] = keys 32 kb .. 32 kb + 31 of query q
    constexpr int BUF = 3 * TILE + (Lp + NBITS) * (int)sizeof(float);
    constexpr int NCH = NKB;                            // 16-byte chunks per loader thread and tile: Lp * 8 / 256
    const int tid = threadIdx.x, wid = tid >> 6;
    const bool loader = wid >= 4;
    const int rw = wid & 3;
    const int dm = H * 64, ld = 3 * dm;
    auto opaque = [](int x) { asm volatile("" : "+v"(x)); return x; };      // keeps address halves from being hoisted out of the item loop: see attn_bwd2_kernel
    int tb = tid & 255;
    uint4 pq[NCH], pk[NCH], pv[NCH];
    float p_bias = 0.f;
    auto issue = [&](int item) {
        const int seq = seq_of(seq_list, item / H), hd = item % H;
        const SeqRows nr = seq_rows(cu, seq, L);
        const bf16_t* base = qkv + (size_t)nr.row0 * ld + hd * 64;
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            const int idx = tb + 256 * j, row = idx >> 3, ch = idx & 7;
            pq[j] = pk[j] = pv[j] = make_uint4(0, 0, 0, 0);
            if (row < nr.len) {
                const bf16_t* rp = base + (size_t)row * ld + ch * 8;
                pq[j] = *(const uint4*)rp;
                pk[j] = *(const uint4*)(rp + dm);
                pv[j] = *(const uint4*)(rp + 2 * dm);
            }
        }
        if (tb < Lp) p_bias = (tb < nr.len && (!mask || mask[(size_t)seq * L + tb] != 0)) ? 0.f : NEG_BIG;
    };
    auto commit = [&](int b) {
        char* base = smem + b * BUF;
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            const int idx = tb + 256 * j, row = idx >> 3, ch = idx & 7;
            const int off = row * RSB + ch * 16;
            *(uint4*)(base + off) = pq[j];
            *(uint4*)(base + TILE + off) = pk[j];
            *(uint4*)(base + 2 * TILE + off) = pv[j];
        }
        if (tb < Lp) ((float*)(base + 3 * TILE))[tb] = p_bias;
    };
    // The loader waves have time to spare: they also evaluate the dropout hash of the next item (one mix32 per key PAIR, common.h) and
    // leave the keep decisions as bits in LDS - and in `bits_out` for the backward, which then hashes nothing.  With the hash in the
    // compute waves (one per SIMD here) dropout cost 23 us of 70 per layer.
    auto make_bits = [&](int b, int item) {
        if constexpr (DROP) {
            const int seq = seq_of(seq_list, item / H), hd = item % H;
            uint32_t* sb = (uint32_t*)(smem + b * BUF + 3 * TILE) + Lp;
            for (int idx = tb; idx < NBITS; idx += 256) {
                const int q = idx % Lp, kb = idx / Lp;
                const uint32_t rk = drop_rowkey(seed, (uint32_t)((seq * H + hd) * L + q));
                uint32_t w = 0;
#pragma unroll
                for (int pp = 0; pp < 16; ++pp) {
                    const uint32_t hh = drop_pair(rk, (uint32_t)(kb * 32 + 2 * pp));
                    w |= (drop_keep_lo(hh, drop_thresh) ? 1u : 0u) << (2 * pp);
                    w |= (drop_keep_hi(hh, drop_thresh) ? 1u : 0u) << (2 * pp + 1);
                }
                sb[idx] = w;
                if (bits_out) bits_out[(size_t)item * NBITS + idx] = w;
            }
        }
    };
    int item = blockIdx.x;
    if (loader && item < nitems) { issue(item); commit(0); make_bits(0, item); }
    __syncthreads();
    int cur = 0;
    for (; item < nitems; item += gridDim.x) {
        const int next = item + gridDim.x;
        const char* sQ = smem + cur * BUF;
        const char* sK = sQ + TILE;
        const char* sV = sK + TILE;
        const float* sBias = (const float*)(sV + TILE);
        const uint32_t* sBits = (const uint32_t*)(sBias + Lp);
        const int seq = seq_of(seq_list, item / H), hd = item % H;
        const SeqRows sr = seq_rows(cu, seq, L);
        const int nb = live_blocks(sr.len);
        const int t_ = opaque(tid);
        const int lane = t_ & 63;
        tb = t_ & 255;
        if (loader) {
            if (next < nitems) { issue(next); commit(cur ^ 1); make_bits(cur ^ 1, next); }
        } else if (rw < NKB && rw >= nb) {      // a query block beyond the sequence: nothing to store but the LSE of its zero rows
            store_lse(lse, seq, hd, H, L, rw * 32 + (lane & 31), lane >> 5, 0.f, (float)sr.len);
        } else if (rw < nb) {
            fwd_full_block<NKB, DROP, F16>(sQ, sK, sV, sBias, KeepBits<Lp>{sBits, 0}, rw, nb, lane, seq, hd, sr, L, H, scale, drop_scale, ctx, ctx16, lse);
        }
        __syncthreads();          // the other buffer is complete, and nobody reads this one any more
        cur ^= 1;
    }
}

// Forward, streaming over the key blocks with a running maximum (one pass, "flash" form): per 32-key block
//   S^T = K_kb . Q^T (lane = query column)  ->  m' = max(m, colmax)  ->  O^T *= 2^(m - m'),  l = l 2^(m - m') + sum p,
//   p = 2^(s - m')  ->  O^T += V_kb^T . (keep . p)         (the S^T tile is the B operand as it is; V through ds_read_tr)
// and at the end ctx = O^T / l (x 1/(1-p_drop)), LSE = m + log2 l.  Everything per query is a per-lane scalar because the
// output is accumulated TRANSPOSED (lane = query column, registers = head dimension): no cross-lane traffic but one
// shuffle per block, and 16 + 32 accumulator registers whatever L is (the first version kept all of S in registers:
// 16 NKB of them, which spilled from L = 192 up and ran 2x slower at L = 256).
// The two streaming kernels share their prologue and stores with the rest of the file but each keeps this loop in its own text: as one function called
// by both, attn_fwd3_kernel<8, false> (the index encode at L = 256) measured 1.3 % slower than before, several times its run-to-run spread
// (profiles/attention_shared_bodies.txt).  A change to the loop goes into both; the tests hold the pair to bit equality.
template <int NKB, bool DROP, bool F16 = false>
__global__ __launch_bounds__(NKB > 4 ? 512 : 256) void attn_fwd_kernel(const bf16_t* __restrict__ qkv, const int64_t* __restrict__ mask,
                                                        bf16_t* __restrict__ ctx, float* __restrict__ lse, int L, int H,
                                                        float scale, uint32_t drop_thresh, float drop_scale, SeedArg seed_a,
                                                        bf16_t* __restrict__ ctx16, const int* __restrict__ cu, const int* __restrict__ seq_list) {
    const uint64_t seed = seed_a.get();
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int Lp = 32 * NKB;
    constexpr int NWAVES = NKB > 4 ? 8 : 4;          // one query / key block per wave up to L = 256 (2 waves per SIMD at one workgroup per CU)
    char* sQ = smem;
    char* sK = sQ + Lp * RSB;
    char* sV = sK + Lp * RSB;
    float* sBias = (float*)(sV + Lp * RSB);
    const int seq = seq_of(seq_list, blockIdx.x / H), hd = blockIdx.x % H;
    const SeqRows sr = seq_rows(cu, seq, L);
    load_item_tiles(sQ, sK, sV, qkv, hd, sr, H, Lp);
    fill_key_bias(sBias, mask, seq, L, Lp, sr.len);
    __syncthreads();

    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const float scale2 = scale * LOG2E;      // scores in the log2 domain (v_exp_f32 is 2^x)
    const int nb = live_blocks(sr.len);
    for (int qb = wid; qb < NKB; qb += NWAVES) {
        if (qb >= nb) {       // a query block beyond the sequence: nothing to store but the LSE of its zero rows
            store_lse(lse, seq, hd, H, L, qb * 32 + r, h, 0.f, (float)sr.len);
            continue;
        }
        const int q = qb * 32 + r;
        bf16x8 qf[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) qf[s] = row_frag(sQ, qb * 32 + r, s, h);
        // dropout mask element (row, col) = ((seq*H + hd)*L + q, key); keys rowmap(t, h), t even / odd, are a column pair
        const uint32_t rk = drop_rowkey(seed, (uint32_t)((seq * H + hd) * L + q));
        float m = NEG_BIG * 4.f, lsum = 0.f;                       // lsum: this half's share of the denominator
        f32x16 O[2] = {(f32x16){0.f}, (f32x16){0.f}};              // O[dt][t] = ctx^T[d = 32 dt + rowmap(t, h)][q]
#pragma unroll
        for (int kb = 0; kb < NKB; ++kb) {
            if (kb >= nb) break;
            f32x16 S = (f32x16){0.f};
#pragma unroll
            for (int s = 0; s < 4; ++s)
                S = mfma32<F16>(row_frag(sK, kb * 32 + r, s, h), qf[s], S);
            // S[t] = <K[key], Q[q]> with key = 32 kb + rowmap(t, h); keys rowmap(4u .. 4u+3, h) = 8u + 4h + 0..3 are consecutive
            float v[16];
            float mloc = NEG_BIG * 4.f;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float4 b4 = *(const float4*)(sBias + kb * 32 + 8 * u + 4 * h);
                const float bb[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
                for (int j = 0; j < 4; j += 2) {      // packed fp32: two keys per instruction
                    const cldrd_f32v2 w = fma2((cldrd_f32v2){S[4 * u + j], S[4 * u + j + 1]}, splat2(scale2), (cldrd_f32v2){bb[j], bb[j + 1]});
                    v[4 * u + j] = w.x; v[4 * u + j + 1] = w.y;
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
                float p0 = __builtin_amdgcn_exp2f(dv.x), p1 = __builtin_amdgcn_exp2f(dv.y);
                psum += p0 + p1;
                if (DROP) {
                    const uint32_t hh = drop_pair(rk, (uint32_t)(kb * 32 + rowmap(t, h)));
                    p0 = drop_keep_lo(hh, drop_thresh) ? p0 : 0.f;
                    p1 = drop_keep_hi(hh, drop_thresh) ? p1 : 0.f;
                }
                v[t] = p0; v[t + 1] = p1;
            }
            lsum = fmaf(lsum, alpha, psum);
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int t = 0; t < 16; t += 2) {
                    const cldrd_f32v2 o2 = (cldrd_f32v2){O[dt][t], O[dt][t + 1]} * splat2(alpha);
                    O[dt][t] = o2.x; O[dt][t + 1] = o2.y;
                }
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                const bf16x8 pb = pack8x<F16>(v + 8 * s2);
#pragma unroll
                for (int dt = 0; dt < 2; ++dt)
                    O[dt] = mfma32<F16>(tr_frag(sV, kb * 32 + 16 * s2 + 4 * h, dt * 32, lane), pb, O[dt]);
            }
            mfma_drain();
        }
        const float l = lsum + __shfl_xor(lsum, 32, 64);
        store_lse(lse, seq, hd, H, L, q, h, m, l);
        const float inv = (DROP ? drop_scale : 1.0f) / l;
        store_ctx_rows<F16, true>(O, inv, ctx, ctx16, ((size_t)sr.row0 + q) * (H * 64) + hd * 64, h, q < sr.len);
    }
}

// Streaming forward for 128 < L <= 256 and many (sequence, head) items (round 5: cfg5's index encode runs at max_length 256, reference
// retriever/index_text.py:37; cfg4 trains BERT-base at L = 256): ONE persistent 8-wave workgroup per CU walks its items.  The one-item form
// above does load -> barrier -> compute per workgroup, and at L = 256 an item's Q, K, V tiles (110 KB of LDS) leave room for one workgroup
// per CU: nothing overlaps the 147 KB of HBM reads of an item with the arithmetic of another, and every CU loads at the same moment.  Here
//   * Q never goes through LDS: a wave's four Q fragments are 64 bytes per lane straight from global memory (row_frag's layout);
//   * K, V (+ the key bias) are double-buffered in LDS (2 x 74 KB): each thread requests its 16-byte pieces of the NEXT item into registers
//     before it starts on the current item (issue early), and writes them to the other buffer when it is done (write late): an item's HBM
//     latency sits under the previous item's arithmetic; one __syncthreads per item;
//   * the block loop is attn_fwd_kernel's, one query block per wave, its Q fragments taken from the prefetch registers.  It is written out here a
//     second time: as one function called by both kernels it made this kernel 1.3 % slower at L = 256 without dropout (the index encode;
//     profiles/attention_shared_bodies.txt).  Change the two loops together; test_attention_fwd_persistent_kernels_at_block_boundaries compares them.
template <int NKB, bool DROP, bool F16 = false>
__global__ __launch_bounds__(512) void attn_fwd3_kernel(const bf16_t* __restrict__ qkv, const int64_t* __restrict__ mask,
                                                         bf16_t* __restrict__ ctx, float* __restrict__ lse, int L, int H,
                                                         float scale, uint32_t drop_thresh, float drop_scale, SeedArg seed_a, int nitems,
                                                         bf16_t* __restrict__ ctx16, const int* __restrict__ cu, const int* __restrict__ seq_list) {
    const uint64_t seed = seed_a.get();
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int Lp = 32 * NKB;
    constexpr int TILE = Lp * RSB;
    constexpr int BUF = 2 * TILE + Lp * (int)sizeof(float);
    constexpr int NCH = (Lp * 8 + 511) / 512;           // 16-byte pieces per thread and tile
    const int dm = H * 64, ld = 3 * dm;
    auto opaque = [](int x) { asm volatile("" : "+v"(x)); return x; };      // see attn_bwd2_kernel: keeps 40 address halves from being hoisted
    int tid = threadIdx.x;
    u32x4 pk[NCH], pv[NCH];          // (first-class vector values: as `uint4` structs hipcc kept the two arrays in scratch memory)
    bf16x8 qn[4];
    long long pm = 0;
    int p_len = 0;                   // row count of the prefetched item (L, or its length in the packed layout)
    // Every load of issue() is UNCONDITIONAL on a clamped row (no exec-masked region, no branch): the compiler can then count its vmcnt waits -
    // the pieces are consumed at commit(), behind this item's ctx stores, and must not wait for those (vmcnt counts stores too).  A row >= L
    // therefore arrives as a copy of row L - 1 instead of zeros: a K row that the key bias masks (score + -1e30 is -1e30 whatever the score),
    // a V row that meets p = 0, a Q row whose output nobody stores - all finite, results unchanged bit for bit.
    const long long* mask_or_any = mask ? (const long long*)mask : (const long long*)qkv;      // null mask: the value loaded is ignored
    auto issue = [&](int item) {
        const int seq = seq_of(seq_list, item / H), hd = item % H;
        const SeqRows nr = seq_rows(cu, seq, L);
        p_len = nr.len;
        const bf16_t* base = qkv + (size_t)nr.row0 * ld + hd * 64;
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            const int idx = tid + 512 * j, row = min(idx >> 3, nr.len - 1), ch = idx & 7;
            const bf16_t* rp = base + (size_t)row * ld + ch * 8;
            pk[j] = *(const u32x4*)(rp + dm);
            pv[j] = *(const u32x4*)(rp + 2 * dm);
        }
        pm = mask_or_any[mask ? (size_t)seq * L + min(tid, L - 1) : (size_t)0];
        // this wave's Q block of the item: row 32 qb + r, 16-byte pieces 2 s + h (row_frag's layout)
        const int lane = tid & 63, r = lane & 31, h = lane >> 5, qb = min(tid >> 6, NKB - 1);
        const int qrow = min(qb * 32 + r, nr.len - 1);
#pragma unroll
        for (int s = 0; s < 4; ++s) qn[s] = *(const bf16x8*)(base + (size_t)qrow * ld + (2 * s + h) * 8);
    };
    auto commit = [&](int b) {
        char* base = smem + b * BUF;
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            const int idx = tid + 512 * j, row = idx >> 3, ch = idx & 7;
            if (NCH * 512 == Lp * 8 || idx < Lp * 8) {
                const int off = row * RSB + ch * 16;
                *(u32x4*)(base + off) = pk[j];
                *(u32x4*)(base + TILE + off) = pv[j];
            }
        }
        if (tid < Lp) ((float*)(base + 2 * TILE))[tid] = (tid < p_len && (!mask || pm != 0)) ? 0.f : NEG_BIG;
    };
    int item = blockIdx.x;
    bf16x8 qf[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) qf[s] = (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
    if (item < nitems) {
        issue(item);
        commit(0);
#pragma unroll
        for (int s = 0; s < 4; ++s) qf[s] = qn[s];
    }
    __syncthreads();
    int cur = 0;
    const float scale2 = scale * LOG2E;      // scores in the log2 domain (v_exp_f32 is 2^x)
    for (; item < nitems; item += gridDim.x) {
        const int next = item + gridDim.x;
        tid = opaque((int)threadIdx.x);
        // in flight while this item is computed.  UNCONDITIONAL (the last item of a workgroup requests itself again: cache hits, and the
        // commit below lands in the buffer nobody reads any more): with the prefetch registers live across a branch hipcc kept them in scratch
        // memory - a scratch store and an s_waitcnt vmcnt(0) behind every load
        issue(next < nitems ? next : item);
        const char* sK = smem + cur * BUF;
        const char* sV = sK + TILE;
        const float* sBias = (const float*)(sV + TILE);
        const int seq = seq_of(seq_list, item / H), hd = item % H;
        const SeqRows sr = seq_rows(cu, seq, L);
        const int nb = live_blocks(sr.len);
        const int lane = tid & 63, wid = tid >> 6;
        const int r = lane & 31, h = lane >> 5;
        if (wid < NKB && wid >= nb) {          // a query block beyond the sequence: nothing to store but the LSE of its zero rows (see seq_rows)
            store_lse(lse, seq, hd, H, L, wid * 32 + r, h, 0.f, (float)sr.len);
        } else if (wid < nb) {
            const int qb = wid;
            const int q = qb * 32 + r;
            // dropout mask element (row, col) = ((seq*H + hd)*L + q, key); keys rowmap(t, h), t even / odd, are a column pair
            const uint32_t rk = drop_rowkey(seed, (uint32_t)((seq * H + hd) * L + q));
            float m = NEG_BIG * 4.f, lsum = 0.f;                       // lsum: this half's share of the denominator
            f32x16 O[2] = {(f32x16){0.f}, (f32x16){0.f}};              // O[dt][t] = ctx^T[d = 32 dt + rowmap(t, h)][q]
#pragma unroll
            for (int kb = 0; kb < NKB; ++kb) {
                if (kb >= nb) break;
                f32x16 S = (f32x16){0.f};
#pragma unroll
                for (int s = 0; s < 4; ++s)
                    S = mfma32<F16>(row_frag(sK, kb * 32 + r, s, h), qf[s], S);
                float v[16];
                float mloc = NEG_BIG * 4.f;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float4 b4 = *(const float4*)(sBias + kb * 32 + 8 * u + 4 * h);
                    const float bb[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
                    for (int j = 0; j < 4; j += 2) {      // packed fp32: two keys per instruction
                        const cldrd_f32v2 w = fma2((cldrd_f32v2){S[4 * u + j], S[4 * u + j + 1]}, splat2(scale2), (cldrd_f32v2){bb[j], bb[j + 1]});
                        v[4 * u + j] = w.x; v[4 * u + j + 1] = w.y;
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
                    float p0 = __builtin_amdgcn_exp2f(dv.x), p1 = __builtin_amdgcn_exp2f(dv.y);
                    psum += p0 + p1;
                    if (DROP) {
                        const uint32_t hh = drop_pair(rk, (uint32_t)(kb * 32 + rowmap(t, h)));
                        p0 = drop_keep_lo(hh, drop_thresh) ? p0 : 0.f;
                        p1 = drop_keep_hi(hh, drop_thresh) ? p1 : 0.f;
                    }
                    v[t] = p0; v[t + 1] = p1;
                }
                lsum = fmaf(lsum, alpha, psum);
#pragma unroll
                for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                    for (int t = 0; t < 16; t += 2) {
                        const cldrd_f32v2 o2 = (cldrd_f32v2){O[dt][t], O[dt][t + 1]} * splat2(alpha);
                        O[dt][t] = o2.x; O[dt][t + 1] = o2.y;
                    }
#pragma unroll
                for (int s2 = 0; s2 < 2; ++s2) {
                    const bf16x8 pb = pack8x<F16>(v + 8 * s2);
#pragma unroll
                    for (int dt = 0; dt < 2; ++dt)
                        O[dt] = mfma32<F16>(tr_frag(sV, kb * 32 + 16 * s2 + 4 * h, dt * 32, lane), pb, O[dt]);
                }
                mfma_drain();
            }
            const float l = lsum + __shfl_xor(lsum, 32, 64);
            store_lse(lse, seq, hd, H, L, q, h, m, l);
            const float inv = (DROP ? drop_scale : 1.0f) / l;
            store_ctx_rows<F16, true>(O, inv, ctx, ctx16, ((size_t)sr.row0 + q) * (H * 64) + hd * 64, h, q < sr.len);
        }
        commit(cur ^ 1);
#pragma unroll
        for (int s = 0; s < 4; ++s) qf[s] = qn[s];
        __syncthreads();          // the other buffer is complete, and nobody reads this one any more
        cur ^= 1;
    }
}

// The backward's view of an item in LDS: Q, K, V, dO tiles; per key the mask bias; per query the LSE (log2 domain), delta = rowsum(dO . O) and the dropout
// row key; sBits (BITS only): the forward's keep bits, dword [kb][q].
struct BwdTiles {
    const char *sQ, *sK, *sV, *sdO;
    const float *sBias, *sLse, *sDelta;
    const uint32_t *sRk, *sBits;
};
// What a wave holds for the whole of a sweep: its 32 keys (sweep A: K and V rows, mask bias) or its 32 queries (sweep B: Q and dO rows, LSE, delta, row key)
struct BwdKeyRows { bf16x8 kf[4], vf[4]; float bias_k; };
struct BwdQueryRows { bf16x8 qf[4], dof[4]; float lse_q, delta_q; uint32_t rk_q; };
__device__ __forceinline__ void bwd_load_keys(const BwdTiles& T, int kb, int lane, BwdKeyRows& K) {
    const int r = lane & 31, h = lane >> 5;
#pragma unroll
    for (int s = 0; s < 4; ++s) { K.kf[s] = row_frag(T.sK, kb * 32 + r, s, h); K.vf[s] = row_frag(T.sV, kb * 32 + r, s, h); }
    K.bias_k = T.sBias[kb * 32 + r];
}
__device__ __forceinline__ void bwd_load_queries(const BwdTiles& T, int qb, int lane, BwdQueryRows& Q) {
    const int r = lane & 31, h = lane >> 5;
#pragma unroll
    for (int s = 0; s < 4; ++s) { Q.qf[s] = row_frag(T.sQ, qb * 32 + r, s, h); Q.dof[s] = row_frag(T.sdO, qb * 32 + r, s, h); }
    const int q = qb * 32 + r;
    Q.lse_q = T.sLse[q]; Q.delta_q = T.sDelta[q];
    Q.rk_q = T.sRk[q];
}

// Sweep A, one query block qb against the wave's key block kb (key on lane): S and dP, P / dP / dS per element, dV += P_drop^T dO, dK += dS^T Q.
// The block loop, and the mfma_drain() that a loop with a run-time count needs, stay with the kernel: attn_bwd_kernel unrolls over NKB (padded)
// or rolls to nb (VARLEN), attn_bwd2_kernel rolls to nb.  BITS: the keep decision is bit `r` of the forward's dword instead of the hash.
template <int NKB, bool DROP, bool BITS, bool F16>
__device__ __forceinline__ void bwd_key_step(const BwdTiles& T, const BwdKeyRows& K, int qb, int kb, int lane, float scale2, uint32_t drop_thresh,
                                             float drop_scale, f32x16 (&dK)[2], f32x16 (&dV)[2]) {
    constexpr int Lp = 32 * NKB;
    const int r = lane & 31, h = lane >> 5, key = kb * 32 + r;
    f32x16 S = (f32x16){0.f}, dP = (f32x16){0.f};
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        S = mfma32<F16>(row_frag(T.sQ, qb * 32 + r, s, h), K.kf[s], S);
        dP = mfma32<F16>(row_frag(T.sdO, qb * 32 + r, s, h), K.vf[s], dP);
    }
    // S[t], dP[t]: query q = 32 qb + rowmap(t, h), key = 32 kb + r
    float pd[16], ds[16];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        // queries rowmap(4u .. 4u+3, h) are consecutive: their LSE / delta / dropout row keys come as 16-byte LDS reads
        const int q4 = qb * 32 + 8 * u + 4 * h;
        const float4 l4 = *(const float4*)(T.sLse + q4), d4 = *(const float4*)(T.sDelta + q4);
        const float ll[4] = {l4.x, l4.y, l4.z, l4.w}, dd[4] = {d4.x, d4.y, d4.z, d4.w};
        uint4 k4 = make_uint4(0, 0, 0, 0);
        if (DROP) k4 = BITS ? *(const uint4*)(T.sBits + kb * Lp + q4) : *(const uint4*)(T.sRk + q4);      // BITS: dwords [kb][q4 .. q4+3], bit = key
        const uint32_t kk[4] = {k4.x, k4.y, k4.z, k4.w};
#pragma unroll
        for (int j = 0; j < 4; j += 2) {      // two queries per packed fp32 instruction (the same IEEE operations as the scalar form)
            const int t = 4 * u + j;
            const cldrd_f32v2 a2 = fma2((cldrd_f32v2){S[t], S[t + 1]}, splat2(scale2), splat2(K.bias_k)) - (cldrd_f32v2){ll[j], ll[j + 1]};
            const cldrd_f32v2 p2 = {__builtin_amdgcn_exp2f(a2.x), __builtin_amdgcn_exp2f(a2.y)};
            cldrd_f32v2 pd2 = p2, dp2 = {dP[t], dP[t + 1]};
            if (DROP) {
                pd2 = p2 * splat2(drop_scale);
                dp2 = dp2 * splat2(drop_scale);
                if constexpr (BITS) {
                    pd2.x = keep_bit(pd2.x, kk[j], r); pd2.y = keep_bit(pd2.y, kk[j + 1], r);
                    dp2.x = keep_bit(dp2.x, kk[j], r); dp2.y = keep_bit(dp2.y, kk[j + 1], r);
                } else {
                    const bool keep0 = dropout_keep(kk[j], (uint32_t)key, drop_thresh), keep1 = dropout_keep(kk[j + 1], (uint32_t)key, drop_thresh);
                    pd2.x = keep0 ? pd2.x : 0.f; pd2.y = keep1 ? pd2.y : 0.f;
                    dp2.x = keep0 ? dp2.x : 0.f; dp2.y = keep1 ? dp2.y : 0.f;
                }
            }
            pd[t] = pd2.x; pd[t + 1] = pd2.y;
            const cldrd_f32v2 ds2 = p2 * (dp2 - (cldrd_f32v2){dd[j], dd[j + 1]});
            ds[t] = ds2.x; ds[t + 1] = ds2.y;
        }
    }
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
        const bf16x8 pb = pack8x<F16>(pd + 8 * s2), sb = pack8x<F16>(ds + 8 * s2);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
            dV[dt] = mfma32<F16>(tr_frag(T.sdO, qb * 32 + 16 * s2 + 4 * h, dt * 32, lane), pb, dV[dt]);
            dK[dt] = mfma32<F16>(tr_frag(T.sQ, qb * 32 + 16 * s2 + 4 * h, dt * 32, lane), sb, dK[dt]);
        }
    }
}

// Sweep B, one key block kb against the wave's query block qb (query on lane): S^T and dP^T, dS per element, dQ += dS K.  Loop and drain: as for sweep A.
// BITS: the keep decisions of the lane's query are the forward's dword [kb][q], shifted to the lane's half.
template <int NKB, bool DROP, bool BITS, bool F16>
__device__ __forceinline__ void bwd_query_step(const BwdTiles& T, const BwdQueryRows& Q, int kb, int qb, int lane, float scale2, uint32_t drop_thresh,
                                               float drop_scale, f32x16 (&dQ)[2]) {
    constexpr int Lp = 32 * NKB;
    const int r = lane & 31, h = lane >> 5, q = qb * 32 + r;
    f32x16 ST = (f32x16){0.f}, dPT = (f32x16){0.f};
    uint32_t wbits = 0;
    if constexpr (BITS) wbits = T.sBits[kb * Lp + q] >> (4 * h);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        ST = mfma32<F16>(row_frag(T.sK, kb * 32 + r, s, h), Q.qf[s], ST);
        dPT = mfma32<F16>(row_frag(T.sV, kb * 32 + r, s, h), Q.dof[s], dPT);
    }
    float ds[16];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int key4 = kb * 32 + 8 * u + 4 * h;
        const float4 b4 = *(const float4*)(T.sBias + key4);
        const float bb[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
        for (int j = 0; j < 4; j += 2) {
            const int t = 4 * u + j;
            // packed fp32 (v_pk_fma_f32 / v_pk_add_f32 / v_pk_mul_f32: two keys per instruction, the same IEEE operations as before)
            const cldrd_f32v2 a2 = fma2((cldrd_f32v2){ST[t], ST[t + 1]}, splat2(scale2), (cldrd_f32v2){bb[j], bb[j + 1]}) - splat2(Q.lse_q);
            const cldrd_f32v2 p2 = {__builtin_amdgcn_exp2f(a2.x), __builtin_amdgcn_exp2f(a2.y)};
            cldrd_f32v2 dp2 = {dPT[t], dPT[t + 1]};
            if (DROP) dp2 = dp2 * splat2(drop_scale);
            float dp0 = dp2.x, dp1 = dp2.y;
            if (DROP) {
                if constexpr (BITS) {       // keys key4 + j, key4 + j + 1: adjacent bits of the forward's dword [kb][q]
                    dp0 = keep_bit(dp0, wbits, 8 * u + j);
                    dp1 = keep_bit(dp1, wbits, 8 * u + j + 1);
                } else {
                    const uint32_t hh = drop_pair(Q.rk_q, (uint32_t)(key4 + j));
                    dp0 = drop_keep_lo(hh, drop_thresh) ? dp0 : 0.f;
                    dp1 = drop_keep_hi(hh, drop_thresh) ? dp1 : 0.f;
                }
            }
            const cldrd_f32v2 ds2 = p2 * ((cldrd_f32v2){dp0, dp1} - splat2(Q.delta_q));
            ds[t] = ds2.x; ds[t + 1] = ds2.y;
        }
    }
#pragma unroll
    for (int s2 = 0; s2 < 2; ++s2) {
        const bf16x8 sa = pack8x<F16>(ds + 8 * s2);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
            // operands swapped: D[d][q], so a lane (= query) ends up with 4 consecutive head dimensions per register quad and dQ
            // leaves in 8-byte stores (the other order gave 32 two-byte stores per lane)
            dQ[dt] = mfma32<F16>(tr_frag(T.sK, kb * 32 + 16 * s2 + 4 * h, dt * 32, lane), sa, dQ[dt]);
    }
}

// dK (x scale) and dV rows of a key block, at ok / ov (the lane's key row).  dV[dt][t] = dV[key][d = 32 dt + rowmap(t, h)]: regs 4u..4u+3 are 4 consecutive d
template <bool F16>
__device__ __forceinline__ void store_dkdv(const f32x16 (&dK)[2], const f32x16 (&dV)[2], float scale, bf16_t* ok, bf16_t* ov, int h, bool live) {
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int u = 0; u < 4; u += 2) {
            uint2 a[2], b[2];
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int t = 4 * (u + k);
                a[k].x = pack2x_scaled<F16>(dK[dt][t], dK[dt][t + 1], scale);
                a[k].y = pack2x_scaled<F16>(dK[dt][t + 2], dK[dt][t + 3], scale);
                b[k].x = pack2x<F16>(dV[dt][t], dV[dt][t + 1]);
                b[k].y = pack2x<F16>(dV[dt][t + 2], dV[dt][t + 3]);
            }
            const uint4 wa = widen_pair(a[0], a[1]), wb = widen_pair(b[0], b[1]);      // 16 contiguous bytes per lane (see widen_pair)
            const int d0 = dt * 32 + 8 * (u + h);
            if (live) {
                *(uint4*)(ok + d0) = wa;
                *(uint4*)(ov + d0) = wb;
            }
        }
}
// dQ (x scale) rows of a query block, at oq (the lane's query row).  dQ[dt][t] = dQ[q][d = 32 dt + rowmap(t, h)]: regs 4u..4u+3 are 4 consecutive d
template <bool F16>
__device__ __forceinline__ void store_dq(const f32x16 (&dQ)[2], float scale, bf16_t* oq, int h, bool live) {
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int u = 0; u < 4; u += 2) {
            uint2 a[2];
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int t = 4 * (u + k);
                a[k].x = pack2x_scaled<F16>(dQ[dt][t], dQ[dt][t + 1], scale);
                a[k].y = pack2x_scaled<F16>(dQ[dt][t + 2], dQ[dt][t + 3], scale);
            }
            const uint4 w = widen_pair(a[0], a[1]);
            if (live) *(uint4*)(oq + dt * 32 + 8 * (u + h)) = w;
        }
}

// VARLEN (a packed batch, launch_bwd_d): the two block loops are ROLLED and run over the live blocks only - a sequence of 74 tokens at L = 256 does
// 3 x 3 block pairs instead of 8 x 8 (measured on packed cfg4, BERT-base L = 256, 29 % real tokens: this kernel was 16 % of the step with whole waves
// skipped only).  Same per-block arithmetic in the same order: the same bits.  The padded instantiation keeps its unrolled loops.
template <int NKB, bool DROP, bool F16 = false, bool VARLEN = false>
__global__ __launch_bounds__(NKB > 4 ? 512 : 256) void attn_bwd_kernel(const bf16_t* __restrict__ qkv, const int64_t* __restrict__ mask,
                                                        const bf16_t* __restrict__ ctx, const bf16_t* __restrict__ dctx,
                                                        const float* __restrict__ lse, bf16_t* __restrict__ dqkv, int L, int H,
                                                        float scale, uint32_t drop_thresh, float drop_scale, SeedArg seed_a,
                                                        const int* __restrict__ cu, const int* __restrict__ seq_list) {
    const uint64_t seed = seed_a.get();
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int Lp = 32 * NKB;
    constexpr int NWAVES = NKB > 4 ? 8 : 4;          // one query / key block per wave up to L = 256 (2 waves per SIMD at one workgroup per CU)
    char* sQ = smem;
    char* sK = sQ + Lp * RSB;
    char* sV = sK + Lp * RSB;
    char* sdO = sV + Lp * RSB;
    float* sBias = (float*)(sdO + Lp * RSB);
    float* sLse = sBias + Lp;
    float* sDelta = sLse + Lp;
    uint32_t* sRk = (uint32_t*)(sDelta + Lp);          // dropout row key of every query row (common.h)
    const int seq = seq_of(seq_list, blockIdx.x / H), hd = blockIdx.x % H;
    const int dm = H * 64, ld = 3 * dm;
    const SeqRows sr = seq_rows(cu, seq, L);
    const int len = sr.len;
    load_item_tiles(sQ, sK, sV, qkv, hd, sr, H, Lp);
    {   // dO tile + delta[q] = sum_d dO[q][d] * O[q][d]
        const bf16_t* dob = dctx + (size_t)sr.row0 * dm + hd * 64;
        const bf16_t* ob = ctx + (size_t)sr.row0 * dm + hd * 64;
        for (int idx = threadIdx.x; idx < Lp * 8; idx += blockDim.x) {
            const int row = idx >> 3, ch = idx & 7;
            uint4 v = make_uint4(0, 0, 0, 0), o = make_uint4(0, 0, 0, 0);
            if (row < len) {
                v = *(const uint4*)(dob + (size_t)row * dm + ch * 8);
                o = *(const uint4*)(ob + (size_t)row * dm + ch * 8);
            }
            *(uint4*)(sdO + row * RSB + ch * 16) = v;
            const uint32_t vv[4] = {v.x, v.y, v.z, v.w}, oo[4] = {o.x, o.y, o.z, o.w};
            float dsum = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) dsum += dot2x<F16>(vv[j], oo[j]);
            dsum += __shfl_xor(dsum, 1, 64); dsum += __shfl_xor(dsum, 2, 64); dsum += __shfl_xor(dsum, 4, 64);
            if (ch == 0) sDelta[row] = dsum;
        }
    }
    for (int k = threadIdx.x; k < Lp; k += blockDim.x) {
        sBias[k] = key_bias(mask, seq, L, k, len);
        sLse[k] = k < L ? lse[((size_t)seq * H + hd) * L + k] * LOG2E : 1.0e30f;      // log2 domain; rows >= L: P = 2^-inf = 0
        sRk[k] = drop_rowkey(seed, (uint32_t)((seq * H + hd) * L + k));
    }
    __syncthreads();
    const BwdTiles T = {sQ, sK, sV, sdO, sBias, sLse, sDelta, sRk, nullptr};

    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;

    const float scale2 = scale * LOG2E;      // scores, mask bias and LSE live in the log2 domain (v_exp_f32 is 2^x)

    const int nb = live_blocks(len);          // live blocks (see seq_rows): whole waves are skipped; inside a live wave the padded
                                             // instantiation's block loops stay unrolled over all NKB blocks (an early exit from an unrolled
                                             // loop cost 40-90 VGPRs and spilled from NKB = 5 up), the VARLEN one's are rolled and stop at nb
    const int nbl = VARLEN ? nb : NKB;
    // ---------------- sweep A: key on lane; dK, dV for 32 keys accumulate over all query blocks ----------------
    for (int kb = wid; kb < NKB; kb += NWAVES) {
        if (kb >= nb) continue;
        BwdKeyRows K;
        bwd_load_keys(T, kb, lane, K);
        f32x16 dK[2] = {(f32x16){0.f}, (f32x16){0.f}}, dV[2] = {(f32x16){0.f}, (f32x16){0.f}};
#pragma unroll (VARLEN ? 1 : NKB)
        for (int qb = 0; qb < nbl; ++qb) {
            bwd_key_step<NKB, DROP, false, F16>(T, K, qb, kb, lane, scale2, drop_thresh, drop_scale, dK, dV);
            if (VARLEN) mfma_drain();
        }
        const int key = kb * 32 + r;
        bf16_t* ok = dqkv + ((size_t)sr.row0 + key) * ld + dm + hd * 64;
        store_dkdv<F16>(dK, dV, scale, ok, ok + dm, h, key < len);
    }

    // ---------------- sweep B: query on lane; dQ for 32 queries accumulates over all key blocks ----------------
    for (int qb = wid; qb < NKB; qb += NWAVES) {
        if (qb >= nb) continue;
        BwdQueryRows Q;
        bwd_load_queries(T, qb, lane, Q);
        f32x16 dQ[2] = {(f32x16){0.f}, (f32x16){0.f}};
#pragma unroll (VARLEN ? 1 : NKB)
        for (int kb = 0; kb < nbl; ++kb) {
            bwd_query_step<NKB, DROP, false, F16>(T, Q, kb, qb, lane, scale2, drop_thresh, drop_scale, dQ);
            if (VARLEN) mfma_drain();
        }
        const int q = qb * 32 + r;
        store_dq<F16>(dQ, scale, dqkv + ((size_t)sr.row0 + q) * ld + hd * 64, h, q < len);
    }
}

// Backward, persistent two-role form for L <= 128 and many (sequence, head) items.
//
// Measured on the kernel above at cfg2 (3072 items, two 4-wave workgroups per CU): loading an item's tiles takes 50 us of the
// 158 when every CU does it at once (HBM-bound: 252 MB), sweep A 3.2 us and sweep B 4.2 us per item at ONE wave per SIMD - and a
// workgroup does the three one after the other, so a CU overlaps them only across its two resident workgroups (LDS and the VGPRs
// allow no third).  Here one 8-wave workgroup per CU walks its items:
//   * waves 0..3 run sweep A while waves 4..7 run sweep B on the same tiles (two waves per SIMD, different work);
//   * waves 4..7 first issue the global loads of the NEXT item into registers (Q, K, V, dO, O: 80 VGPRs), run their sweep, then
//     write them to the other LDS buffer (with delta, mask bias, LSE, dropout row keys): issue-early / write-late, the HBM latency
//     sits under the sweep;  one __syncthreads per item.
// The sweeps are attn_bwd_kernel's (bwd_key_step / bwd_query_step and their loads and stores); this form adds the roles, the prefetch, the forward's
// keep bits (BITS), and block loops that are always rolled and stop at the last live block (the prefetch registers need the room).
template <int NKB, bool DROP, bool BITS, bool F16 = false>
__global__ __launch_bounds__(512) void attn_bwd2_kernel(const bf16_t* __restrict__ qkv, const int64_t* __restrict__ mask,
                                                         const bf16_t* __restrict__ ctx, const bf16_t* __restrict__ dctx,
                                                         const float* __restrict__ lse, bf16_t* __restrict__ dqkv, int L, int H,
                                                         float scale, uint32_t drop_thresh, float drop_scale, SeedArg seed_a, int nitems,
                                                         const uint32_t* __restrict__ drop_bits, const int* __restrict__ cu, const int* __restrict__ seq_list) {
    const uint64_t seed = seed_a.get();
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int Lp = 32 * NKB;
    constexpr int TILE = Lp * RSB;
    constexpr int NBITS = BITS ? Lp * NKB : 0;          // the forward's dropout keep bits (attn_fwd2_kernel): dword [kb][q]
    constexpr int NBW = (NBITS + 255) / 256;
    constexpr int BUF = 4 * TILE + (4 * Lp + NBITS) * (int)sizeof(float);
    constexpr int NCH = NKB;                            // 16-byte chunks per thread and tile: Lp * 8 / 256
    const int tid = threadIdx.x, wid = tid >> 6;
    const bool role_b = wid >= 4;
    const int rw = wid & 3;
    const int dm = H * 64, ld = 3 * dm;
    const float scale2 = scale * LOG2E;
    // per-lane indices are re-derived from an OPAQUE copy of the thread id in every iteration: hipcc otherwise hoists the loop-
    // invariant halves of ~40 64-bit load / store addresses out of the item loop and spills them (76 VGPRs of scratch at L = 128)
    auto opaque = [](int x) { asm volatile("" : "+v"(x)); return x; };
    int tb = tid & 255;
    uint4 pq[NCH], pk[NCH], pv[NCH], pdo[NCH], po[NCH];
    // raw prefetched scalars of the next item: consumed in commit(), i.e. BEHIND the sweep.  (Until round 4 issue() compared the mask word
    // and scaled the LSE at once: the compiler had to wait for those two loads right there with vmcnt(0) - the counter is in order - and
    // with them for the twenty tile loads issued just before: the "issue early, write late" prefetch waited for itself.)
    long long p_mask = 1;
    float p_lse = 0.f;
    int p_len = 0;                   // row count of the prefetched item (L, or its length in the packed layout)
    uint32_t pbits[NBW > 0 ? NBW : 1];
    auto issue = [&](int item) {
        const int seq = seq_of(seq_list, item / H), hd = item % H;
        const SeqRows nr = seq_rows(cu, seq, L);
        p_len = nr.len;
        const bf16_t* base = qkv + (size_t)nr.row0 * ld + hd * 64;
        const bf16_t* dob = dctx + (size_t)nr.row0 * dm + hd * 64;
        const bf16_t* ob = ctx + (size_t)nr.row0 * dm + hd * 64;
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            const int idx = tb + 256 * j, row = idx >> 3, ch = idx & 7;
            pq[j] = pk[j] = pv[j] = pdo[j] = po[j] = make_uint4(0, 0, 0, 0);
            if (row < nr.len) {
                const bf16_t* rp = base + (size_t)row * ld + ch * 8;
                pq[j] = ld16_stream(rp);                          // q, k, v, o: the forward's tape, read once (common.h)
                pk[j] = ld16_stream(rp + dm);
                pv[j] = ld16_stream(rp + 2 * dm);
                pdo[j] = *(const uint4*)(dob + (size_t)row * dm + ch * 8);
                po[j] = ld16_stream(ob + (size_t)row * dm + ch * 8);
            }
        }
        if (tb < Lp) {
            const int tc = tb < L ? tb : L - 1;           // clamped: the compare with L happens in commit()
            p_mask = mask ? mask[(size_t)seq * L + tc] : 1;
            p_lse = lse[((size_t)seq * H + hd) * L + tc];
        }
        if constexpr (BITS) {
#pragma unroll
            for (int j = 0; j < NBW; ++j) pbits[j] = tb + 256 * j < NBITS ? drop_bits[(size_t)item * NBITS + tb + 256 * j] : 0u;
        }
    };
    auto commit = [&](int b, int item) {
        const int seq = seq_of(seq_list, item / H), hd = item % H;
        char* base = smem + b * BUF;
        float* fl = (float*)(base + 4 * TILE);
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            const int idx = tb + 256 * j, row = idx >> 3, ch = idx & 7;
            const int off = row * RSB + ch * 16;
            *(uint4*)(base + off) = pq[j];
            *(uint4*)(base + TILE + off) = pk[j];
            *(uint4*)(base + 2 * TILE + off) = pv[j];
            *(uint4*)(base + 3 * TILE + off) = pdo[j];
            const uint32_t vv[4] = {pdo[j].x, pdo[j].y, pdo[j].z, pdo[j].w}, oo[4] = {po[j].x, po[j].y, po[j].z, po[j].w};
            float dsum = 0.f;
#pragma unroll
            for (int e = 0; e < 4; ++e) dsum += dot2x<F16>(vv[e], oo[e]);
            dsum += __shfl_xor(dsum, 1, 64); dsum += __shfl_xor(dsum, 2, 64); dsum += __shfl_xor(dsum, 4, 64);
            if (ch == 0) fl[2 * Lp + row] = dsum;
        }
        if (tb < Lp) {
            fl[tb] = (tb < p_len && p_mask != 0) ? 0.f : NEG_BIG;
            fl[Lp + tb] = tb < L ? p_lse * LOG2E : 1.0e30f;
            ((uint32_t*)fl)[3 * Lp + tb] = drop_rowkey(seed, (uint32_t)((seq * H + hd) * L + tb));
        }
        if constexpr (BITS) {
#pragma unroll
            for (int j = 0; j < NBW; ++j)
                if (tb + 256 * j < NBITS) ((uint32_t*)fl)[4 * Lp + tb + 256 * j] = pbits[j];
        }
    };
    int item = blockIdx.x;
    if (role_b && item < nitems) { issue(item); commit(0, item); }
    __syncthreads();
    int cur = 0;
    for (; item < nitems; item += gridDim.x) {
        const int next = item + gridDim.x;
        const bool has_next = next < nitems;
        const char* tiles = smem + cur * BUF;
        const float* fl = (const float*)(tiles + 4 * TILE);
        const BwdTiles T = {tiles, tiles + TILE, tiles + 2 * TILE, tiles + 3 * TILE, fl, fl + Lp, fl + 2 * Lp, (const uint32_t*)fl + 3 * Lp,
                            (const uint32_t*)fl + 4 * Lp};
        const int seq = seq_of(seq_list, item / H), hd = item % H;
        const SeqRows sr = seq_rows(cu, seq, L);
        const int len = sr.len, nb = live_blocks(len);
        const int t_ = opaque(tid);
        const int lane = t_ & 63, r = lane & 31, h = lane >> 5;
        tb = t_ & 255;
        if (role_b) {
            if (has_next) issue(next);
            if (rw < nb) {        // ---- sweep B: query on lane; dQ for 32 queries accumulates over all (live) key blocks
                const int qb = rw;
                BwdQueryRows Q;
                bwd_load_queries(T, qb, lane, Q);
                f32x16 dQ[2] = {(f32x16){0.f}, (f32x16){0.f}};
                for (int kb = 0; kb < nb; ++kb) {
                    bwd_query_step<NKB, DROP, BITS, F16>(T, Q, kb, qb, lane, scale2, drop_thresh, drop_scale, dQ);
                    mfma_drain();
                }
                const int q = qb * 32 + r;
                store_dq<F16>(dQ, scale, dqkv + ((size_t)sr.row0 + q) * ld + hd * 64, h, q < len);
            }
            if (has_next) commit(cur ^ 1, next);
        } else if (rw < nb) {     // ---- sweep A: key on lane; dK, dV for 32 keys accumulate over all (live) query blocks
            const int kb = rw;
            BwdKeyRows K;
            bwd_load_keys(T, kb, lane, K);
            f32x16 dK[2] = {(f32x16){0.f}, (f32x16){0.f}}, dV[2] = {(f32x16){0.f}, (f32x16){0.f}};
            for (int qb = 0; qb < nb; ++qb)
                bwd_key_step<NKB, DROP, BITS, F16>(T, K, qb, kb, lane, scale2, drop_thresh, drop_scale, dK, dV);
            mfma_drain();     // behind the loop (see mfma_drain): its only exit falls through to here, in front of the first read of dK / dV
            const int key = kb * 32 + r;
            bf16_t* ok = dqkv + ((size_t)sr.row0 + key) * ld + dm + hd * 64;
            store_dkdv<F16>(dK, dV, scale, ok, ok + dm, h, key < len);
        }
        __syncthreads();          // the other buffer is complete, and nobody reads this one any more
        cur ^= 1;
    }
}

int attn_num_cus() {
    static int n = 0;
    if (n == 0) {
        int dev = 0, v = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || v <= 0) v = 256;
        n = v;
    }
    return n;
}

bool attn_fwd2_enabled(int nseq, int L, int H) {
    return L <= 128 && nseq * H >= 2 * attn_num_cus() && g_cldrd_tune_attn_fwd2 != 0;
}

// One launch's arguments: the entry point fills them once, every launcher reads them.  nseq: the sequences of THIS launch (items = nseq x H);
// L: the batch's row stride of lse / keep bits / dropout row keys (the tile height is the launcher's NKB); p, seed: as the caller gave them.
struct AttnFwdArgs {
    const bf16_t* qkv; const int64_t* mask; const int* cu; const int* seq_list;
    bf16_t* ctx; float* lse; int nseq, L, H; float scale, p; unsigned long long seed; uint32_t* bits_out; bf16_t* ctx16; hipStream_t st;
};
struct AttnBwdArgs {
    const bf16_t* qkv; const int64_t* mask; const int* cu; const int* seq_list;
    const bf16_t* ctx; const bf16_t* dctx; const float* lse; bf16_t* dqkv; int nseq, L, H; float scale, p; unsigned long long seed;
    const uint32_t* drop_bits; hipStream_t st;
};

// f(std::true_type) when dropout is active for this p, else f(std::false_type); a DROP = false launcher passes the kernels p = 0 and no keep bits
bool attn_drops(float p) { return p > 0.f && dropout_thresh16(p) > 0; }
template <class F>
int with_drop(float p, F&& f) { return attn_drops(p) ? f(std::true_type{}) : f(std::false_type{}); }


template <int NKB, bool DROP, bool F16>
int launch_fwd_full(const AttnFwdArgs& a, bf16_t* ctx16) {      // the all-scores one-item kernel (L <= 128)
    const float p = DROP ? a.p : 0.f;
    const size_t lds = 3 * 32 * NKB * RSB + 32 * NKB * sizeof(float);
    return attn_launch(attn_fwd_full_kernel<NKB, DROP, F16>, a.nseq * a.H, 256, lds, a.st, a.qkv, a.mask, a.ctx, a.lse, a.L, a.H, a.scale,
                       DROP ? dropout_thresh16(p) : 0u, 1.0f / (1.0f - p), seed_arg(a.seed), ctx16, a.cu, a.seq_list);
}

template <int NKB, bool DROP>
int launch_fwd_f16(const AttnFwdArgs& a) {      // fp16 in, fp16 out: no second copy; the all-scores-in-registers kernel only (L <= 128)
    return launch_fwd_full<NKB, DROP, true>(a, nullptr);
}

template <int NKB, bool DROP, bool F16>
int launch_fwd(const AttnFwdArgs& a) {
    const float p = DROP ? a.p : 0.f, drop_scale = 1.0f / (1.0f - p);
    const uint32_t thresh = DROP ? dropout_thresh16(p) : 0u;
    const size_t lds = 3 * 32 * NKB * RSB + 32 * NKB * sizeof(float);
    const int nitems = a.nseq * a.H, cus = attn_num_cus();
    if constexpr (NKB <= 4) {
        // many items: the persistent loader / compute kernel (cldrd_set_tuning("attn_fwd2", 0) keeps the one-item-per-workgroup kernel: A/B runs and tests)
        if (attn_fwd2_enabled(a.nseq, 32 * NKB, a.H))         // (the tile height, not L: a listed launch of short sequences has L > 128)
            return attn_launch(attn_fwd2_kernel<NKB, DROP, F16>, cus, 512, 2 * (lds + (DROP ? 32 * NKB * NKB * sizeof(uint32_t) : 0)), a.st, a.qkv, a.mask,
                               a.ctx, a.lse, a.L, a.H, a.scale, thresh, drop_scale, seed_arg(a.seed), nitems, DROP ? a.bits_out : nullptr, a.ctx16, a.cu,
                               a.seq_list);
        return launch_fwd_full<NKB, DROP, F16>(a, a.ctx16);
    } else {
        // many items at 128 < L <= 256: the persistent streaming kernel (K / V double-buffered, Q from global memory); cldrd_set_tuning("attn_fwd2", 0)
        // keeps the one-item-per-workgroup kernel (tests: the two are bit-identical)
        if (nitems >= 2 * cus && g_cldrd_tune_attn_fwd2 != 0)
            return attn_launch(attn_fwd3_kernel<NKB, DROP, F16>, cus, 512, 2 * (2 * 32 * NKB * RSB + 32 * NKB * sizeof(float)), a.st, a.qkv, a.mask, a.ctx,
                               a.lse, a.L, a.H, a.scale, thresh, drop_scale, seed_arg(a.seed), nitems, a.ctx16, a.cu, a.seq_list);
        return attn_launch(attn_fwd_kernel<NKB, DROP, F16>, nitems, 512, lds, a.st, a.qkv, a.mask, a.ctx, a.lse, a.L, a.H, a.scale, thresh, drop_scale,
                           seed_arg(a.seed), a.ctx16, a.cu, a.seq_list);
    }
}

template <int NKB, bool DROP, bool F16>
int launch_bwd(const AttnBwdArgs& a) {
    const float p = DROP ? a.p : 0.f, drop_scale = 1.0f / (1.0f - p);
    const uint32_t thresh = DROP ? dropout_thresh16(p) : 0u;
    const int nitems = a.nseq * a.H;
    const size_t lds = 4 * 32 * NKB * RSB + 4 * 32 * NKB * sizeof(float);
    if constexpr (NKB <= 4) {
        // many items: the persistent two-role kernel (cldrd_set_tuning("attn_bwd2", 0) keeps the one-item-per-workgroup kernel: tests)
        const int cus = attn_num_cus();
        if (nitems >= 2 * cus && g_cldrd_tune_attn_bwd2 != 0) {
            auto go = [&](auto bits) {       // bits: the forward left its keep bits (room for them behind each LDS buffer), else the kernel re-hashes
                constexpr bool BITS = decltype(bits)::value;
                return attn_launch(attn_bwd2_kernel<NKB, DROP, BITS, F16>, cus, 512, 2 * (lds + (BITS ? 32 * NKB * NKB * sizeof(uint32_t) : 0)), a.st, a.qkv,
                                   a.mask, a.ctx, a.dctx, a.lse, a.dqkv, a.L, a.H, a.scale, thresh, drop_scale, seed_arg(a.seed), nitems,
                                   BITS ? a.drop_bits : nullptr, a.cu, a.seq_list);
            };
            return DROP && a.drop_bits ? go(std::integral_constant<bool, DROP>{}) : go(std::false_type{});
        }
    }
    auto go = [&](auto varlen) {
        return attn_launch(attn_bwd_kernel<NKB, DROP, F16, decltype(varlen)::value>, nitems, NKB > 4 ? 512 : 256, lds, a.st, a.qkv, a.mask, a.ctx, a.dctx,
                           a.lse, a.dqkv, a.L, a.H, a.scale, thresh, drop_scale, seed_arg(a.seed), a.cu, a.seq_list);
    };
    // a packed batch: the instantiation whose block loops stop at the sequence's last live block
    return a.cu != nullptr && NKB > 1 ? go(std::true_type{}) : go(std::false_type{});
}


}  // namespace

// Does the forward for this shape run the persistent kernel that leaves the dropout keep bits behind?  Returns the number of 32-bit
// words of the bit array (nseq*H items x [key block][query]), 0 when the bits are not produced (the backward then hashes itself).
extern "C" long long cldrd_attention_bits_words(int nseq, int L, int H, float dropout_p) {
    if (!attn_drops(dropout_p) || nseq <= 0 || L <= 0 || H <= 0 || !attn_fwd2_enabled(nseq, L, H)) return 0;
    const long long nkb = (L + 31) / 32;
    return (long long)nseq * H * 32 * nkb * nkb;
}

// qkv: 16-bit [rows, 3*H*64] (Q | K | V, heads contiguous inside each); ctx: [rows, H*64]; lse: fp32 [nseq, H, L] (may be null for inference).
// Layouts (mask / cu_rows / seq_list, n_list, Ltile): include/cldrd_hip.h.  A packed batch gives bit for bit what cldrd_unpack_rows16 -> the
// padded call -> cldrd_gather_rows give, without the two row moves and without loading padding rows.
// drop_bits_out (optional, cldrd_attention_bits_words() words): receives the dropout keep bits for cldrd_attention_bwd (none for L > 128).
// ctx_f16_copy (optional, bf16 pass only): the same context in fp16 - the operand of an fp16 out-projection GEMM; ctx itself may then be null
// (an evaluation forward keeps no bf16 tape).
extern "C" int cldrd_attention_fwd(const void* qkv, const long long* mask, const int* cu_rows, const int* seq_list, int n_list, int Ltile,
                                   void* ctx, float* lse, int nseq, int L, int H, float dropout_p, unsigned long long seed, int fmt,
                                   void* drop_bits_out, void* ctx_f16_copy, void* stream) {
    if (attn_check("attention_fwd", mask, cu_rows, seq_list, n_list, Ltile, nseq, L, H)) return 1;
    const int n = seq_list ? n_list : nseq;          // sequences of THIS launch (items = n x H)
    const int Lt = seq_list ? Ltile : L;             // rows a sequence of this launch can have: the kernels' tile height
    CLDRD_CHECK(ctx != nullptr || ctx_f16_copy != nullptr, "attention_fwd: no output");
    CLDRD_CHECK(!(fmt != CLDRD_FMT_BF16 && (ctx_f16_copy != nullptr || ctx == nullptr)), "attention_fwd: the fp16 pass writes ctx only");
    CLDRD_CHECK(fmt == CLDRD_FMT_BF16 || fmt == CLDRD_FMT_F16 || fmt == CLDRD_FMT_F16_TAPE, "attention_fwd: fmt is 0 (bf16), 1 (fp16, L <= 128, no keep bits) or 5 (fp16, every kernel of the bf16 path)");
    CLDRD_CHECK(fmt != CLDRD_FMT_F16 || Lt <= 128, "attention_fwd: the fp16 forward handles L <= 128");
    const AttnFwdArgs a = {(const bf16_t*)qkv, (const int64_t*)mask, cu_rows, seq_list, (bf16_t*)ctx, lse,
                           n, L, H, 0.125f /* 1 / sqrt(64) */, dropout_p, seed,
                           (uint32_t*)drop_bits_out, (bf16_t*)ctx_f16_copy, (hipStream_t)stream};
    const int nkb = (Lt + 31) / 32;
    if (fmt == CLDRD_FMT_F16_TAPE)            // fp16 activations through the whole kernel family (round 4: the all-fp16 training mode)
        return with_nkb<8>(nkb, [&](auto k) { return with_drop(dropout_p, [&](auto d) { return launch_fwd<decltype(k)::value, decltype(d)::value, true>(a); }); });
    if (fmt == CLDRD_FMT_F16)            // fp16 activations, evaluation passes: the all-scores-in-registers kernel only
        return with_nkb<4>(nkb, [&](auto k) { return with_drop(dropout_p, [&](auto d) { return launch_fwd_f16<decltype(k)::value, decltype(d)::value>(a); }); });
    return with_nkb<8>(nkb, [&](auto k) { return with_drop(dropout_p, [&](auto d) { return launch_fwd<decltype(k)::value, decltype(d)::value, false>(a); }); });
}

// drop_bits (optional): what cldrd_attention_fwd left for the same (nseq, L, H, dropout_p, seed); null: the mask is re-hashed.
// fmt != CLDRD_FMT_BF16: q / k / v, ctx, dctx and dqkv are fp16 (the all-fp16 training mode: gradients carry the loss scale).
// Packed batch: rows of dqkv that do not exist in the packed layout (padding) are not written - in the padded layout they receive zeros.
extern "C" int cldrd_attention_bwd(const void* qkv, const long long* mask, const int* cu_rows, const int* seq_list, int n_list, int Ltile,
                                   const void* ctx, const void* dctx, const float* lse, void* dqkv, int nseq, int L, int H, float dropout_p,
                                   unsigned long long seed, int fmt, const void* drop_bits, void* stream) {
    if (attn_check("attention_bwd", mask, cu_rows, seq_list, n_list, Ltile, nseq, L, H)) return 1;
    const int n = seq_list ? n_list : nseq, Lt = seq_list ? Ltile : L;          // as in cldrd_attention_fwd
    CLDRD_CHECK(lse != nullptr, "attention_bwd: lse is required");
    const AttnBwdArgs a = {(const bf16_t*)qkv, (const int64_t*)mask, cu_rows, seq_list, (const bf16_t*)ctx, (const bf16_t*)dctx, lse,
                           (bf16_t*)dqkv, n, L, H, 0.125f, dropout_p, seed,
                           (const uint32_t*)drop_bits, (hipStream_t)stream};
    const int nkb = (Lt + 31) / 32;
    if (fmt != CLDRD_FMT_BF16)
        return with_nkb<8>(nkb, [&](auto k) { return with_drop(dropout_p, [&](auto d) { return launch_bwd<decltype(k)::value, decltype(d)::value, true>(a); }); });
    return with_nkb<8>(nkb, [&](auto k) { return with_drop(dropout_p, [&](auto d) { return launch_bwd<decltype(k)::value, decltype(d)::value, false>(a); }); });
}

// ---------------------------------------------------------------------------------------------------------------
// CLS-only attention for the LAST encoder layer.  The reference pools `last_hidden_state[:, 0, :]`
// (models/nway_dual_encoder.py:52,56,64), so in the last layer only the query of token 0 matters:
// K and V are still needed for every token, but the score matrix shrinks to one row per (sequence, head) and
// everything after attention runs on one row per sequence.  One wavefront per (sequence, head).
namespace {

template <bool F16>
__global__ __launch_bounds__(64) void attn_cls_fwd_kernel(const bf16_t* __restrict__ qc, const bf16_t* __restrict__ kv,
                                                           const int64_t* __restrict__ mask, bf16_t* __restrict__ ctx,
                                                           float* __restrict__ probs, int L, int H, float scale,
                                                           uint32_t drop_thresh, float drop_scale, SeedArg seed_a, bf16_t* __restrict__ ctx16,
                                                           const int* __restrict__ cu) {
    const uint64_t seed = seed_a.get();
    __shared__ float sp[256];
    __shared__ float sq[64];
    const int seq = blockIdx.x / H, hd = blockIdx.x % H, lane = threadIdx.x;
    const int dm = H * 64;
    sq[lane] = x2f<F16>(qc[(size_t)seq * dm + hd * 64 + lane]);
    __syncthreads();
    const SeqRows sr = seq_rows(cu, seq, L);          // packed K | V rows: see seq_rows
    const int len = sr.len;
    const bf16_t* kb = kv + (size_t)sr.row0 * 2 * dm + hd * 64;
    const bf16_t* vb = kb + dm;
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
            for (int c = 0; c < 8; ++c) {
                const uint4 u = *(const uint4*)(kr + c * 8);
                const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    a += x2f<F16>((bf16_t)(w[j] & 0xFFFFu)) * sq[c * 8 + 2 * j] + x2f<F16>((bf16_t)(w[j] >> 16)) * sq[c * 8 + 2 * j + 1];
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
        if (key < L) {
            const float p = sc[i] * inv;
            probs[((size_t)seq * H + hd) * L + key] = p;
            float pd = p;
            if (drop_thresh) pd = dropout_keep(drop_rowkey(seed, (uint32_t)((seq * H + hd) * L)), (uint32_t)key, drop_thresh) ? p * drop_scale : 0.f;
            sp[key] = pd;
        }
    }
    __syncthreads();
    // ctx = P V.  Eight lanes share a key row (16 bytes = 8 features each), eight keys per instruction: L / 8 row-block loads instead of
    // the L dependent 2-byte-per-lane loads this loop was until round 3 (24 of the kernel's 34 us at L = 128: pure load latency, on the
    // step's critical path between the last K / V projection and the loss).  The eight key groups are combined through LDS.
    const int c8 = lane & 7, g = lane >> 3;
    float o8[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) o8[j] = 0.f;
    for (int k0 = 0; k0 < len; k0 += 8) {           // keys >= len: p = 0 and (padded layout) zero rows: + 0.0f, skipped
        const int key = k0 + g;
        if (key < len) {
            const float pk = sp[key];
            const uint4 u = *(const uint4*)(vb + (size_t)key * 2 * dm + c8 * 8);
            const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                o8[2 * j] += pk * x2f<F16>((bf16_t)(w[j] & 0xFFFFu));
                o8[2 * j + 1] += pk * x2f<F16>((bf16_t)(w[j] >> 16));
            }
        }
    }
    __shared__ float so[8][64];
#pragma unroll
    for (int j = 0; j < 8; ++j) so[g][c8 * 8 + j] = o8[j];
    __syncthreads();
    float o = 0.f;
#pragma unroll
    for (int gg = 0; gg < 8; ++gg) o += so[gg][lane];
    if (ctx) ctx[(size_t)seq * dm + hd * 64 + lane] = f2x<F16>(o);
    if (ctx16) ctx16[(size_t)seq * dm + hd * 64 + lane] = f2x<true>(o);       // fp16 copy of a bf16 pass (out-projection operand)
}

template <bool F16>
__global__ __launch_bounds__(64) void attn_cls_bwd_kernel(const bf16_t* __restrict__ qc, const bf16_t* __restrict__ kv,
                                                           const float* __restrict__ probs, const bf16_t* __restrict__ dctx,
                                                           bf16_t* __restrict__ dqc, bf16_t* __restrict__ dkv, int L, int H,
                                                           float scale, uint32_t drop_thresh, float drop_scale, SeedArg seed_a,
                                                           const int* __restrict__ cu) {
    const uint64_t seed = seed_a.get();
    __shared__ float sds[256], spd[256], sdo[64];
    const int seq = blockIdx.x / H, hd = blockIdx.x % H, lane = threadIdx.x;
    const int dm = H * 64;
    sdo[lane] = x2f<F16>(dctx[(size_t)seq * dm + hd * 64 + lane]);
    const float qd = x2f<F16>(qc[(size_t)seq * dm + hd * 64 + lane]);
    __syncthreads();
    const SeqRows sr = seq_rows(cu, seq, L);
    const int len = sr.len;
    const bf16_t* kb = kv + (size_t)sr.row0 * 2 * dm + hd * 64;
    const bf16_t* vb = kb + dm;
    float p[4], dp[4], dot = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int key = lane + 64 * i;
        p[i] = dp[i] = 0.f;
        if (key < len) {
            p[i] = probs[((size_t)seq * H + hd) * L + key];
            const bf16_t* vr = vb + (size_t)key * 2 * dm;
            float a = 0.f;
#pragma unroll
            for (int c = 0; c < 8; ++c) {
                const uint4 u = *(const uint4*)(vr + c * 8);
                const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    a += x2f<F16>((bf16_t)(w[j] & 0xFFFFu)) * sdo[c * 8 + 2 * j] + x2f<F16>((bf16_t)(w[j] >> 16)) * sdo[c * 8 + 2 * j + 1];
            }
            float pdv = p[i];
            if (drop_thresh) {
                const bool keep = dropout_keep(drop_rowkey(seed, (uint32_t)((seq * H + hd) * L)), (uint32_t)key, drop_thresh);
                pdv = keep ? p[i] * drop_scale : 0.f;
                a = keep ? a * drop_scale : 0.f;
            }
            dp[i] = a;
            spd[key] = pdv;
            dot += p[i] * a;
        }
    }
    dot = wave_sum(dot);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int key = lane + 64 * i;
        if (key < len) sds[key] = p[i] * (dp[i] - dot) * scale;
    }
    __syncthreads();
    // dq = sum_key ds[key] K[key]; dK[key] = ds[key] q; dV[key] = p_drop[key] dO.  Eight lanes per key row (16 bytes = 8 features
    // each), eight keys per instruction (see attn_cls_fwd_kernel): L / 8 row-block loads and 2 L / 8 row-block stores instead of L + 2 L
    // two-byte-per-lane accesses; the eight key groups' dq partial sums are combined through LDS.
    __shared__ float sqd[64];
    sqd[lane] = qd;
    __syncthreads();
    bf16_t* dkb = dkv + (size_t)sr.row0 * 2 * dm + hd * 64;
    const int c8 = lane & 7, g = lane >> 3;
    float q8[8], do8[8], dq8[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { q8[j] = sqd[c8 * 8 + j]; do8[j] = sdo[c8 * 8 + j]; dq8[j] = 0.f; }
    for (int k0 = 0; k0 < len; k0 += 8) {
        const int key = k0 + g;
        if (key < len) {
            const float ds = sds[key], pd = spd[key];
            const uint4 u = *(const uint4*)(kb + (size_t)key * 2 * dm + c8 * 8);
            const uint32_t w[4] = {u.x, u.y, u.z, u.w};
            uint32_t ok[4], ov[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                dq8[2 * j] += ds * x2f<F16>((bf16_t)(w[j] & 0xFFFFu));
                dq8[2 * j + 1] += ds * x2f<F16>((bf16_t)(w[j] >> 16));
                ok[j] = (uint32_t)f2x<F16>(ds * q8[2 * j]) | ((uint32_t)f2x<F16>(ds * q8[2 * j + 1]) << 16);
                ov[j] = (uint32_t)f2x<F16>(pd * do8[2 * j]) | ((uint32_t)f2x<F16>(pd * do8[2 * j + 1]) << 16);
            }
            *(uint4*)(dkb + (size_t)key * 2 * dm + c8 * 8) = make_uint4(ok[0], ok[1], ok[2], ok[3]);
            *(uint4*)(dkb + (size_t)key * 2 * dm + dm + c8 * 8) = make_uint4(ov[0], ov[1], ov[2], ov[3]);
        }
    }
    __shared__ float sdq[8][64];
#pragma unroll
    for (int j = 0; j < 8; ++j) sdq[g][c8 * 8 + j] = dq8[j];
    __syncthreads();
    float dq = 0.f;
#pragma unroll
    for (int gg = 0; gg < 8; ++gg) dq += sdq[gg][lane];
    dqc[(size_t)seq * dm + hd * 64 + lane] = f2x<F16>(dq);
}

// dst[m * stride_rows] += src[m]  (bf16 rows of d elements)
template <int FMT>      // 0: bf16 += bf16; 1: fp32 += fp32; 2: fp16 dst += fp32 src (fp32 add, one rounding: the fp16 gradient stream)
__global__ __launch_bounds__(256) void add_rows_strided_kernel(void* __restrict__ dst_v, const void* __restrict__ src_v, int M, int d,
                                                                int stride_rows) {
    const int m = blockIdx.x;
    for (int c = threadIdx.x; c < d; c += blockDim.x) {
        const size_t o = (size_t)m * stride_rows * d + c;
        if (FMT == 1) ((float*)dst_v)[o] += ((const float*)src_v)[(size_t)m * d + c];
        else if (FMT == 2) ((_Float16*)dst_v)[o] = (_Float16)((float)((const _Float16*)dst_v)[o] + ((const float*)src_v)[(size_t)m * d + c]);
        else ((bf16_t*)dst_v)[o] = f2bf(bf2f(((const bf16_t*)dst_v)[o]) + bf2f(((const bf16_t*)src_v)[(size_t)m * d + c]));
    }
}

}  // namespace

// qc: 16-bit [nseq, H*64] (CLS queries); kv: [rows, 2*H*64] = K | V (padded, or packed with cu_rows: include/cldrd_hip.h); ctx: [nseq, H*64];
// probs: fp32 [nseq, H, L] in either layout
extern "C" int cldrd_attention_cls_fwd(const void* qc, const void* kv, const long long* mask, const int* cu_rows, void* ctx, float* probs,
                                       int nseq, int L, int H, float dropout_p, unsigned long long seed, int fmt, void* ctx_f16_copy,
                                       void* stream) {
    if (attn_check("attention_cls_fwd", mask, cu_rows, nullptr, 0, 0, nseq, L, H)) return 1;
    CLDRD_CHECK(probs != nullptr, "attention_cls_fwd: need a probs buffer");
    CLDRD_CHECK((ctx != nullptr || ctx_f16_copy != nullptr) && !(fmt != CLDRD_FMT_BF16 && (ctx_f16_copy != nullptr || ctx == nullptr)), "attention_cls_fwd: outputs");
    const uint32_t th = dropout_p > 0.f ? dropout_thresh16(dropout_p) : 0u;
    if (fmt != CLDRD_FMT_BF16)
        hipLaunchKernelGGL(attn_cls_fwd_kernel<true>, dim3(nseq * H), dim3(64), 0, (hipStream_t)stream, (const bf16_t*)qc, (const bf16_t*)kv,
                           (const int64_t*)mask, (bf16_t*)ctx, probs, L, H, 0.125f, th, 1.0f / (1.0f - dropout_p), seed_arg(seed), (bf16_t*)nullptr, cu_rows);
    else
        hipLaunchKernelGGL(attn_cls_fwd_kernel<false>, dim3(nseq * H), dim3(64), 0, (hipStream_t)stream, (const bf16_t*)qc, (const bf16_t*)kv,
                           (const int64_t*)mask, (bf16_t*)ctx, probs, L, H, 0.125f, th, 1.0f / (1.0f - dropout_p), seed_arg(seed), (bf16_t*)ctx_f16_copy, cu_rows);
    CLDRD_LAUNCH_CHECK();
    return 0;
}

// dqc: [nseq, H*64]; dkv: [rows, 2*H*64] in the layout of kv (every row written)
extern "C" int cldrd_attention_cls_bwd(const void* qc, const void* kv, const int* cu_rows, const float* probs, const void* dctx, void* dqc,
                                       void* dkv, int nseq, int L, int H, float dropout_p, unsigned long long seed, int fmt, void* stream) {
    if (attn_check("attention_cls_bwd", nullptr, cu_rows, nullptr, 0, 0, nseq, L, H)) return 1;
    const uint32_t th = dropout_p > 0.f ? dropout_thresh16(dropout_p) : 0u;
    if (fmt != CLDRD_FMT_BF16)
        hipLaunchKernelGGL(attn_cls_bwd_kernel<true>, dim3(nseq * H), dim3(64), 0, (hipStream_t)stream, (const bf16_t*)qc, (const bf16_t*)kv, probs,
                           (const bf16_t*)dctx, (bf16_t*)dqc, (bf16_t*)dkv, L, H, 0.125f, th, 1.0f / (1.0f - dropout_p), seed_arg(seed), cu_rows);
    else
        hipLaunchKernelGGL(attn_cls_bwd_kernel<false>, dim3(nseq * H), dim3(64), 0, (hipStream_t)stream, (const bf16_t*)qc, (const bf16_t*)kv, probs,
                           (const bf16_t*)dctx, (bf16_t*)dqc, (bf16_t*)dkv, L, H, 0.125f, th, 1.0f / (1.0f - dropout_p), seed_arg(seed), cu_rows);
    CLDRD_LAUNCH_CHECK();
    return 0;
}

int cldrd_launch_add_rows_idx(void* dst, const void* src, int M, int d, const int* idx, int fmt, hipStream_t st);      // pack.hip
// dst[idx ? idx[m] : m * stride_rows] += src[m]; fmt: enum cldrd_stream_fmt
extern "C" int cldrd_add_rows(void* dst, const void* src, int M, int d, int stride_rows, const int* idx, int fmt, void* stream) {
    CLDRD_CHECK(M > 0 && d > 0 && (idx || stride_rows > 0), "add_rows: bad shape");
    if (idx) return cldrd_launch_add_rows_idx(dst, src, M, d, idx, fmt, (hipStream_t)stream);
    decltype(&add_rows_strided_kernel<1>) kern;      // fmt: 0 bf16, 1 fp32, 2 fp16
    if (fmt == 1) kern = add_rows_strided_kernel<1>;
    else if (fmt == 2) kern = add_rows_strided_kernel<2>;
    else kern = add_rows_strided_kernel<0>;
    hipLaunchKernelGGL(kern, dim3(M), dim3(256), 0, (hipStream_t)stream, dst, src, M, d, stride_rows);
    CLDRD_LAUNCH_CHECK();
    return 0;
}

// Device and host helpers shared by the attention kernel files (attention.hip: head dim 64, forward and backward; attention_hd32.hip: head dim 32,
// evaluation forward): the [L, 64]-column LDS tile with its fragment reads, the 16-bit format switches, the packed-batch row map, the widened
// context stores, the launch helper and the layout check of the C entry points.  Everything lives in an anonymous namespace: each file compiles
// its own copy.
#pragma once
#include "common.h"
#include "../../include/cldrd_hip.h"      // enum cldrd_fmt16
#include <cstdio>
#include <type_traits>

namespace {

constexpr int RSB = 144;                 // LDS row stride in bytes (64 bf16 + 8 pad): b128 row reads conflict-free
constexpr float NEG_BIG = -1.0e30f;
constexpr float LOG2E = 1.4426950408889634f, LN2 = 0.6931471805599453f;

__device__ __forceinline__ int rowmap(int t, int h) { return (t & 3) + 8 * (t >> 2) + 4 * h; }

__device__ __forceinline__ bf16x8 row_frag(const char* tile, int row, int s, int h) {
    return *(const bf16x8*)(tile + row * RSB + (2 * s + h) * 16);
}
// 8 elements k = {row0 + 0..3, row0 + 8 + 0..3} of column (col0 + (lane & 31)) -- the k order of an accumulator tile
__device__ __forceinline__ bf16x8 tr_frag(const char* tile, int row0, int col0, int lane) {
    const int g = lane >> 4, qq = (lane >> 2) & 3, pp = lane & 3;
    const char* p = tile + (row0 + qq) * RSB + (col0 + 16 * (g & 1) + 4 * pp) * 2;
    const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) bf16x4*)p);
    const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) bf16x4*)(p + 8 * RSB));
    return (bf16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}
__device__ __forceinline__ bf16x8 pack8(const float* v) {
    bf16x8 r;
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = (short)f2bf(v[j]);
    return r;
}

// 16-bit activation format of the FORWARD kernels: bf16 (default), or fp16 for the high-precision forward of the query tower
// (encoder.py: 11-bit significand operands, same MFMA rate; the backward always runs on the bf16 tape).
typedef _Float16 f16x8_t __attribute__((ext_vector_type(8)));
__device__ __forceinline__ bf16_t f2h(float f) { const _Float16 h = (_Float16)f; return __builtin_bit_cast(bf16_t, h); }
__device__ __forceinline__ float h2f(bf16_t v) { return (float)__builtin_bit_cast(_Float16, v); }
template <bool F16> __device__ __forceinline__ bf16_t f2x(float f) { if constexpr (F16) return f2h(f); else return f2bf(f); }
template <bool F16> __device__ __forceinline__ float x2f(bf16_t v) { if constexpr (F16) return h2f(v); else return bf2f(v); }
template <bool F16>
__device__ __forceinline__ bf16x8 pack8x(const float* v) {
    bf16x8 r;
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = (short)f2x<F16>(v[j]);
    return r;
}
template <bool F16>
__device__ __forceinline__ f32x16 mfma32(bf16x8 a, bf16x8 b, f32x16 c) {
    if constexpr (F16) return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

template <bool F16> __device__ __forceinline__ uint32_t pack2x(float lo, float hi) {
    if constexpr (F16) {
        typedef _Float16 h2_t __attribute__((ext_vector_type(2)));
        const cldrd_f32v2 f = {lo, hi};
        return __builtin_bit_cast(uint32_t, __builtin_convertvector(f, h2_t));      // one v_cvt_pk_f16_f32
    } else return pack2bf(lo, hi);
}
template <bool F16> __device__ __forceinline__ uint32_t pack2x_scaled(float lo, float hi, float scale) {      // one v_pk_mul_f32 + one convert
    const cldrd_f32v2 m = (cldrd_f32v2){lo, hi} * splat2(scale);
    return pack2x<F16>(m.x, m.y);
}
// sum of the two products of a dword pair of 16-bit values (delta = rowsum(dO . O))
template <bool F16> __device__ __forceinline__ float dot2x(uint32_t a, uint32_t b) {
    if constexpr (F16) return h2f((bf16_t)(a & 0xFFFFu)) * h2f((bf16_t)(b & 0xFFFFu)) + h2f((bf16_t)(a >> 16)) * h2f((bf16_t)(b >> 16));
    else return __uint_as_float(a << 16) * __uint_as_float(b << 16) + __uint_as_float(a & 0xFFFF0000u) * __uint_as_float(b & 0xFFFF0000u);
}

// dropout by keep BITS: value * (bit `pos` of w ? 1 : 0) as one v_bfe_i32 (0 / all ones) and one v_and
__device__ __forceinline__ float keep_bit(float v, uint32_t w, int pos) {
    return __uint_as_float(__float_as_uint(v) & (uint32_t)__builtin_amdgcn_sbfe((int)w, pos, 1));
}

// Output rows of the 32 x 32 MFMA layout: lanes r and r + 32 hold ADJACENT 8-byte pieces (4 head dimensions each) of the same row, so the
// natural store is 8 bytes per lane - twice the store instructions, and a row-per-lane store is issue-bound per instruction
// (tools/micro/store_rate.hip; cdna_hip_programming.md T21).  One v_permlane32_swap per dword trades the upper half-wave's piece of
// column group u against the lower half-wave's piece of group u + 1: afterwards a lane of the lower half holds the 16 contiguous bytes of
// group u, a lane of the upper half those of group u + 1 -> one 16-byte store at column 8 (u + h).  Executed by all lanes (outside `if (row < L)`).
__device__ __forceinline__ uint4 widen_pair(const uint2& g0, const uint2& g1) {
    typedef unsigned attn_u32x2 __attribute__((ext_vector_type(2)));
    const attn_u32x2 rx = __builtin_amdgcn_permlane32_swap(g0.x, g1.x, false, false);
    const attn_u32x2 ry = __builtin_amdgcn_permlane32_swap(g0.y, g1.y, false, false);
    return make_uint4(rx[0], ry[0], rx[1], ry[1]);
}

// Packed ("varlen") batches: with `cu` given, the rows of sequence `seq` are rows cu[seq] .. cu[seq + 1] of qkv / ctx / dctx / dqkv (pack.hip's
// layout: Tp = sum of the lengths rows, no padding rows anywhere) instead of rows seq * L .. seq * L + L of the padded layout; keys and queries
// >= the sequence's length arrive in LDS as zero rows and are masked, exactly what the padded layout holds after cldrd_unpack_rows16 - so the two
// layouts give the same bits - and are neither read nor written.  LSE, keep bits and probabilities stay [nseq, H, L(, ..)] (small).
// Blocks of 32 keys / queries that lie entirely beyond a sequence's length are SKIPPED (nb = ceil(len / 32) live blocks): a masked key's
// probability is exactly 0 and a zero query row's output is never stored, so every skipped MFMA would have added +0.0f - same bits, less work
// (a packed MS MARCO batch at max_length 256 holds 37 % real tokens: 3 of 8 blocks per side).  The LSE of a skipped (all-zero) query row has the
// closed form log(len): scores 0, maximum 0, denominator = the number of unmasked keys, exactly what the arithmetic gives.
// A block loop that can be LEFT EARLY ends in a branch right behind an MFMA, and the code at the branch target reads that MFMA's accumulator.
// hipcc (ROCm 7.2) counts the wait states between an XDL write and a VALU read of its result along the fall-through path only: in
// attn_fwd_full_kernel<4> with two live blocks the exit edge reached `v_accvgpr_read a63 / a62` four cycles behind the MFMA that writes
// a[48:63] - stale scores for keys 58, 59, 62, 63 of every sequence of 59 .. 64 tokens (tools/wgrad_attn_fuzz.py found it; the keys are masked
// in shorter sequences, which is why nothing else noticed).  mfma_drain() ends every block iteration of such a loop, in front of the next
// iteration's exit test: 24 wait states (more than the longest XDL result latency) on BOTH ways out of the branch, pinned against the schedulers;
// they pass under the last MFMA of the block, which occupies the pipe for longer than that.  Drained: the key-block loops of the forward bodies (fwd_full_block, the two streaming kernels),
// both block loops of attn_bwd_kernel when VARLEN, and both sweeps of attn_bwd2_kernel (its count nb is a run-time value in either layout).  In the
// key-side sweep of attn_bwd2_kernel (dK, dV: four accumulators, the kernel's register peak) the drain stands BEHIND the loop instead of at the end of
// its body: the loop's only exit falls through to it, so the wait states lie between the last MFMA and the first read of dK / dV all the same, and on the
// back edge nothing reads dK / dV before the next iteration's last MFMAs, which take them as their own C operand a whole iteration later.  Inside the body
// it put the L = 128 dropout instantiations at 256 VGPRs with 28 bytes of scratch (profiles/one_schedule_timing.txt).
__device__ __forceinline__ void mfma_drain() {
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_nop 15\n\ts_nop 7" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
}

__device__ __forceinline__ int live_blocks(int len) { return (len + 31) >> 5; }      // 32-row blocks that hold a row < len (see seq_rows)
// A launch may cover a LIST of sequences (seq_list, device int32; null: all of them in order): item i / H is then the list position and
// seq_list[i / H] the sequence - how a packed batch with L > 128 sends its sequences of at most 128 tokens (most of an MS MARCO batch) to the
// L <= 128 kernels (persistent, double-buffered) and only the long ones to the streaming / one-item kernels: `L` stays the stride of LSE and of
// the dropout row keys, the kernel's tile height comes from its NKB.
__device__ __forceinline__ int seq_of(const int* __restrict__ seq_list, int pos) { return seq_list ? seq_list[pos] : pos; }
struct SeqRows { int row0, len; };
__device__ __forceinline__ SeqRows seq_rows(const int* __restrict__ cu, int seq, int L) {
    if (cu) { const int c0 = cu[seq]; return {c0, cu[seq + 1] - c0}; }
    return {seq * L, L};
}

// copy a [L, 64] bf16 head slice (row stride ld elements) into an LDS tile of Lp rows, zero-filling rows >= L
__device__ __forceinline__ void load_tile(char* tile, const bf16_t* src, int ld, int L, int Lp) {
    for (int idx = threadIdx.x; idx < Lp * 8; idx += blockDim.x) {
        const int row = idx >> 3, ch = idx & 7;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (row < L) v = *(const uint4*)(src + (size_t)row * ld + ch * 8);
        *(uint4*)(tile + row * RSB + ch * 16) = v;
    }
}

// Mask bias of key k: 0, or NEG_BIG for a key that is masked or beyond the sequence
__device__ __forceinline__ float key_bias(const int64_t* __restrict__ mask, int seq, int L, int k, int len) {
    return (k < len && (!mask || mask[(size_t)seq * L + k] != 0)) ? 0.f : NEG_BIG;
}
// The key bias of one item, as the forward kernels fill it (attn_bwd_kernel fills it in the loop that also converts the LSE and hashes the row keys)
__device__ __forceinline__ void fill_key_bias(float* sBias, const int64_t* __restrict__ mask, int seq, int L, int Lp, int len) {
    for (int k = threadIdx.x; k < Lp; k += blockDim.x) sBias[k] = key_bias(mask, seq, L, k, len);
}

// Context rows of a query block, at ctx / ctx16 + orow (the lane's query row).  O[dt][t] = ctx^T[d = 32 dt + rowmap(t, h)][q]: registers 4u .. 4u+3
// are 4 consecutive head dimensions of the lane's query row; one v_permlane32_swap pair makes them 16 contiguous bytes (widen_pair): 4 (+ 4 for the
// fp16 copy) 16-byte stores per lane instead of 32 (+ 32) two-byte ones.  (Round 2 tried the transposed form with 8-byte stores and found it 8 %
// slower; round 5, with the widened stores: profiles/r05_microbench.txt section 6.)
// NDT: accumulator tiles of 32 head dimensions per query row - 2 at head dim 64, 1 at head dim 32 (attention_hd32.hip: orow then points at the head's 32 columns).
// ctx: the kernel's own format (may be absent); ctx16: an fp16 copy of a bf16 pass (out-projection operand).  SCALE: the streaming form's deferred
// 1 / l (x 1 / (1 - p_drop)); the all-scores form has normalised its probabilities already and multiplies by nothing here.
template <bool F16, bool SCALE, int NDT = 2>
__device__ __forceinline__ void store_ctx_rows(const f32x16 (&O)[NDT], float inv, bf16_t* __restrict__ ctx, bf16_t* __restrict__ ctx16, size_t orow, int h,
                                               bool live) {
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
        for (int u = 0; u < 4; u += 2) {
            uint2 o[2], o16[2];
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int b = 4 * (u + k);
                float v[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = SCALE ? O[dt][b + e] * inv : O[dt][b + e];
                o[k].x = pack2x<F16>(v[0], v[1]);
                o[k].y = pack2x<F16>(v[2], v[3]);
                o16[k].x = (uint32_t)f2x<true>(v[0]) | ((uint32_t)f2x<true>(v[1]) << 16);
                o16[k].y = (uint32_t)f2x<true>(v[2]) | ((uint32_t)f2x<true>(v[3]) << 16);
            }
            if (ctx) {
                const uint4 w = widen_pair(o[0], o[1]);
                if (live) *(uint4*)(ctx + orow + dt * 32 + 8 * (u + h)) = w;
            }
            if (ctx16) {
                const uint4 w = widen_pair(o16[0], o16[1]);
                if (live) *(uint4*)(ctx16 + orow + dt * 32 + 8 * (u + h)) = w;
            }
        }
}

// f(std::integral_constant<int, n>) for n = nkb clamped to 1 .. MAX: the runtime number of 32-key blocks as a template argument
template <int MAX, class F>
int with_nkb(int nkb, F&& f) {
    if constexpr (MAX > 1) {
        if (nkb < MAX) return with_nkb<MAX - 1>(nkb, f);
    }
    return f(std::integral_constant<int, MAX>{});
}

// Every launch of this family: the dynamic-LDS limit of the kernel, the launch, the launch check
template <class... P, class... A>
int attn_launch(void (*kern)(P...), int grid, int block, size_t lds, hipStream_t st, A... args) {
    (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(block), lds, st, args...);
    CLDRD_LAUNCH_CHECK();
    return 0;
}

// The shape limits and the layout rule of include/cldrd_hip.h, checked here for all four entry points (`op` names the caller in the message)
int attn_check(const char* op, const long long* mask, const int* cu_rows, const int* seq_list, int n_list, int Ltile, int nseq, int L, int H) {
    const char* why = nullptr;
    if (!(nseq > 0 && L > 0 && L <= 256 && H > 0)) why = "need 0 < L <= 256";
    else if (cu_rows != nullptr && mask != nullptr) why = "a packed batch (cu_rows) takes no mask";
    else if (seq_list != nullptr && !(cu_rows != nullptr && n_list > 0 && n_list <= nseq && Ltile > 0 && Ltile <= L))
        why = "a sequence list goes with a packed batch, 0 < n_list <= nseq, 0 < Ltile <= L";
    if (why == nullptr) return 0;
    char msg[128];
    snprintf(msg, sizeof(msg), "%s: %s", op, why);
    return cldrd_set_error(msg);
}

}  // namespace

// Weight gradient: dW[N1,N2] (+)= sum_m A[m,N1] * B[m,N2]   (A = dY, B = X; bf16 in, fp32 out), optionally with the
// bias gradient db[N1] (+)= sum_m A[m,N1] folded in.
//
// The reduction index m (tokens) is the ROW index of both operands, so neither is K-contiguous: the MFMA fragments are
// fetched with gfx950's transposing LDS read (ds_read_b64_tr_b16) from row-major [64 tokens][cols] tiles that arrive
// by LDS-DMA.  The 16-B slot index is XOR-swizzled with f(m) = 2*((m&3) | ((m>>3)&1)<<2) (on the DMA source address
// and on the read address): every transposed read then touches all 64 banks exactly once.
//
// (Round 3: the NT kernel's third A slot / separate operand rings were tried here too and removed again - nothing for the step, and the
// restructured K loop read 7.4 instead of 5.9 GB per passage-tower group: profiles/r03_microbench.txt.)
// Tile 256 (n1) x 128 (n2), 512 threads = 4 x 2 waves of 64 x 64, MFMA 16x16x32; 64-token K tiles in two LDS slots.
// Same software pipeline as gemm_nt_ring.hip: per 32-token k-step the A fragments are refilled in place as soon as
// their last MFMA has issued, the B fragments are double-buffered, reads are threaded between the MFMAs
// (sched_group_barrier), one raw s_barrier per K tile, the DMA of K tile t+2 is issued half-way through K tile t.
// M = tokens is huge and N1 x N2 small, so the token range of a tile is cut into chunks, one workgroup each; each writes an fp32 slab
// and a second pass sums the slabs in a fixed order (bitwise reproducible, no float atomics).
// The bias gradient costs one extra MFMA per A fragment in the n2 == 0 tiles: B = all-ones.
//
// Rows >= M of the last 64-token K tile are fetched from a zero page instead of the operands (the LDS-DMA source address is per
// lane), so the operands need neither padding nor a zeroed tail.
//
// GROUPED launch (cldrd_wgrad_group): the weight gradients are not on the critical path of the backward (only the data gradients
// are), so the trainer defers them and hands all of a tower's problems - 4 per layer - to ONE launch.  Work item = (problem, token
// chunk, output tile), ordered tile-fastest so that the workgroups running at the same time on one XCD compute neighbouring tiles
// of the same problem at the same token position (shared A / B panels in that XCD's L2).  Workgroups of an XCD stay together only for
// about 256 K tiles (wgrad_splits_group), so long token ranges are cut even where the tiles alone would fill the CUs.  How they are cut is
// a host-side PLAN per problem (wgrad_plan_group): n_long chunks of c_long K tiles, then n_short chunks of c_short, the long items of all
// problems first in the launch, the short ones last, where they fill the round the long items leave part empty.  At cfg2 (25 problems,
// 32 768 tokens) one split count for the launch meant 3 x 171 K tiles and a last round a third full; the plan is two chunks of 256 for
// 18 problems, 256 + 2 x 128 or 4 x 128 for three small ones, one short item per tile of the CLS-only layer's four-K-tile problems: 1 305
// items instead of 1 944, 342 MB written instead of 510, the launch 2.39 -> 2.25 ms and its reduction 117 -> 86 us
// (profiles/wgrad_balanced_timing.txt).  A problem with one chunk writes dW directly; a group of ONE problem keeps the single split
// count and the bits it always had.
// Tried and dropped: adding the slabs up inside the launch (arrival counter per tile, agent-scope release / acquire, the last arriver
// reads the slabs in chunk order).  Correct and reproducible, and the 86-us reduction launch goes away, but with a release at the end of
// every workgroup and the slabs re-read inside it the launch grew from 2.25 to 2.44 ms: +0.05 ms per step (same file).
#include <algorithm>
#include <functional>
#include <type_traits>
#include <vector>

#include "common.h"

namespace {

constexpr int BK = 64;                 // tokens per LDS slot
constexpr int MAXP = 32;               // problems per launch (kernel-argument block: 32 x 104 B + header, see the static_assert)

struct TnProblem {
    const bf16_t* A; const bf16_t* B; float* dW; float* dbias;      // dbias may be null
    int M, N1, N2, lda, ldb;
    int tiles, nt2;                    // (N1 / T1) * (N2 / T2), N2 / T2
    int nt1, n1_fast;                  // N1 / T1; tile order inside a split: n2 fastest (0) or n1 fastest (1), see cldrd_wgrad_group
    // Chunk plan (host: wgrad_plan_group).  The token range is cut into n_long chunks of clen[0] K tiles followed by chunks of clen[1]
    // K tiles (the last chunk may be shorter).  A launch runs the long items of ALL its problems first, then the short ones: region
    // r = 0 (long) / 1 (short), first[r] = this problem's first work item counted from the start of region r; items of a problem inside a
    // region: chunk-major, tile-minor.
    int first[2], clen[2];
    int n_long, chunks;                // long chunks; all chunks = fp32 slabs of this problem (1: the tile is complete, dW is written directly)
    long long slab_off;                // chunks > 1: float offset of this problem's slabs in the workspace
};
struct TnGroupArgs {
    int n, items_long, accumulate;      // items_long: work items of region 0 (the grid holds items_long + the short items)
    float* slabs;
    const float* inv_scale;            // device scalar or null: every output (dW, dbias) is multiplied by it - the operands of the all-fp16
                                       // training mode carry the loss scale, parameter gradients do not (capi.hip: cldrd_set_loss_scale)
    float* sq_out;                     // slab reduction only: [gridDim.y][gridDim.x] sums of squares of what each workgroup wrote, or null
    TnProblem p[MAXP];
};
// the table travels in the kernel-argument block (the launch is captured in a graph: no device-side copy to keep alive)
static_assert(sizeof(TnProblem) == 104 && sizeof(TnGroupArgs) <= 4096, "TnGroupArgs must fit the 4-KiB kernel-argument block");

__device__ __attribute__((aligned(4096))) uint4 g_zero_page[256];     // 4 KiB of zeros: DMA source of token rows >= M

__device__ __forceinline__ int swz(int m) { return 2 * ((m & 3) | (((m >> 3) & 1) << 2)); }
// 16-byte chunk c of token row m -> position inside the row.  Rows of 256 / 512 bytes: c ^ swz(m).  Rows of 384 bytes (24 chunks,
// the 192-column B tile): chunks 0..15 as before, chunks 16..23 permute among themselves with 2 ((m>>1)&1 | ((m>>3)&1)<<1); odd
// rows start 128 bytes into a 256-byte bank window, and tools/lds_bank_sim.py shows every transposed read still touches each of
// the 64 banks once.  The map is an involution, so the DMA applies it on the source side.
template <int ROWB>
__device__ __forceinline__ int chunk_pos(int c, int m) {
    if (ROWB == 384 && c >= 16) return 16 + ((c - 16) ^ (2 * (((m >> 1) & 1) | (((m >> 3) & 1) << 1))));
    return c ^ swz(m);
}

// One MFMA operand = two transposing reads (token rows m and m + 4: same swizzle, fixed byte distance HI).  They are issued
// by hand: hipcc models the ds_read_tr builtin as an LDS access that may alias the LDS-DMA in flight and puts
// s_waitcnt vmcnt(0) in front of it, which drains the two K tiles being prefetched on every k-step (the kernel then runs at
// DMA latency, not at MFMA rate).  The price is that the lgkmcnt waits are ours too, see kstep().
// One LDS-DMA piece (1 KiB per wave), saddr form: LDS destination = m0 + lane*16, source = uniform 64-bit base + per-lane 32-bit offset
// (hipcc turned `base + kt*stride + zext(off)` into two 64-bit VALU adds per piece and kept every offset as a register pair: 245 -> 225
// VGPRs for the 256 x 192 tile, +1..2 %).  Tried on the way and dropped: the bias gradient by v_dot2c_f32_bf16 instead of the all-ones
// MFMA (frees 24 VGPRs, but the launch ran 15 % slower even without a bias problem in it) and a 256 x 256 tile (spills only outside
// the K loop, 1018 TF/s at 4096^3 against 877 for 256 x 128, but no better than 256 x 192 on the encoder shapes once the tile counts
// are rounded to whole rounds of CUs).
__device__ __forceinline__ void tn_dma16(uint32_t lds_addr, uint32_t voff, const void* sbase) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" ::"s"(lds_addr), "v"(voff), "s"(sbase) : "memory", "m0");
}
// Round 4: the two transposing reads of a fragment are the BUILTIN again, and every LDS-DMA of the kernel is inline asm instead (the
// partial-tile path included).  Rounds 1-3 had it the other way round - reads in asm because hipcc, seeing a global_load_lds builtin
// anywhere in the loop, put s_waitcnt vmcnt(0) in front of every LDS read - and paid for it: two 64-bit asm outputs are two unrelated
// register pairs, so hipcc copied every fragment into a 4-register tuple before its MFMA (56 v_mov per 48 MFMAs in the K loop;
// PMC: 1.66 VALU instructions per MFMA in a kernel that has no arithmetic) and the hand-counted lgkmcnt waits had to live with the
// 4-bit counter.  With no VMEM instruction visible to it the compiler inserts exact lgkmcnt waits for its own reads and allocates lo / hi
// as one tuple (no copies); the vmcnt waits of the DMA ring stay ours.
struct Frag { bf16x4 lo, hi; };
template <int OFF, int HI>
__device__ __forceinline__ void tr_issue(Frag& f, uint32_t addr) {
    typedef __attribute__((address_space(3))) bf16x4* lds4;
    f.lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4)(uintptr_t)(addr + OFF));
    f.hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds4)(uintptr_t)(addr + OFF + HI));
}
__device__ __forceinline__ bf16x8 frag8(const Frag& f) { return __builtin_shufflevector(f.lo, f.hi, 0, 1, 2, 3, 4, 5, 6, 7); }
// one LDS-DMA piece with a per-lane 64-bit source address (partial last K tile: rows >= M come from the zero page)
__device__ __forceinline__ void tn_dma16_addr(uint32_t lds_addr, const void* src) {
    asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off" ::"s"(lds_addr), "v"(src) : "memory", "m0");
}

typedef _Float16 tn_f16x8 __attribute__((ext_vector_type(8)));
template <bool F16>
__device__ __forceinline__ f32x4 tn_mfma(bf16x8 a, bf16x8 b, f32x4 c) {
    if constexpr (F16) return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(tn_f16x8, a), __builtin_bit_cast(tn_f16x8, b), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}
// F16: the operands are fp16 (round 4: the all-fp16 training mode), same MFMA rate, same tiles
template <int T1, int T2, int NW, bool F16 = false>
__global__ __launch_bounds__(64 * NW, 2) void gemm_tn_kernel(TnGroupArgs ga) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NBF = T2 == 192 ? 3 : 4;              // B fragments (16 n2 columns each) per wave
    constexpr int WGN = T2 / (16 * NBF), WGM = NW / WGN;        // wave grid; a wave owns (16 FA) x (16 NBF) of the tile
    constexpr int FA = T1 / WGM / 16;                   // A fragments (16 n1 columns each) per wave
    constexpr int A_BYTES = BK * T1 * 2, B_BYTES = BK * T2 * 2, SLOT = A_BYTES + B_BYTES;
    constexpr int LPR_A = T1 / 8, RA = 64 / LPR_A;      // lanes per A row, A rows per 1-KiB piece
    constexpr int APW = A_BYTES / 1024 / NW, BPW = B_BYTES / 1024 / NW;     // pieces per wave
    constexpr int NSLOT = 3 * SLOT <= 160 * 1024 ? 3 : 2;                   // 3: K tiles kt+1 and kt+2 stay in flight
    constexpr int G = APW + BPW;                        // LDS-DMA instructions per wave per K tile
    const int lane = threadIdx.x & 63;
    const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // Long items first, short items last; each region is spread over the XCDs on its own, so every XCD works through its share of the
    // long items, then its share of the short ones, and neighbouring tiles of a (problem, chunk) still meet in one XCD's L2.
    const int rg = (int)blockIdx.x >= ga.items_long ? 1 : 0;             // wave-uniform, like everything down to c1 / c2
    const int id = rg ? xcd_remap(blockIdx.x - ga.items_long, gridDim.x - ga.items_long) : xcd_remap(blockIdx.x, ga.items_long);
    int pi = 0;
    while (pi + 1 < ga.n && id >= ga.p[pi + 1].first[rg]) ++pi;          // scalar loads from the argument block
    const TnProblem& P = ga.p[pi];
    const bf16_t* __restrict__ A = P.A;
    const bf16_t* __restrict__ B = P.B;
    const int M = P.M, N1 = P.N1, N2 = P.N2, lda = P.lda, ldb = P.ldb;
    const int nt2 = P.nt2, ntiles = P.tiles;
    const int local = id - P.first[rg];
    const int chunk = local / ntiles, tile = local % ntiles;      // the tiles of one chunk are neighbours: they share A/B rows
    const int c1 = (P.n1_fast ? tile % P.nt1 : tile / nt2) * T1, c2 = (P.n1_fast ? tile / P.nt1 : tile % nt2) * T2;
    const int ktotal = (M + BK - 1) / BK;
    const int clen = P.clen[rg];
    const int kbeg = (rg ? P.n_long * P.clen[0] : 0) + chunk * clen;
    const int nk = min(ktotal, kbeg + clen) - kbeg;
    const int slab = (rg ? P.n_long : 0) + chunk;
    const int wm = wid / WGN, wn = wid % WGN;
    const bool do_bias = P.dbias != nullptr && c2 == 0 && wn == 0;
    const int mtail = M & (BK - 1);                    // valid rows of the last K tile (0: it is complete)

    // ---- LDS-DMA.  A piece = RA token rows x (T1*2) B; a B piece = 1 KiB of the row-major B image; wave w owns pieces APW*w.. / BPW*w..
    uint32_t oa[APW], ob[BPW];
#pragma unroll
    for (int i = 0; i < APW; ++i) {
        const int r = RA * (APW * wid + i) + lane / LPR_A;
        oa[i] = (uint32_t)r * (uint32_t)(lda * 2) + (uint32_t)(c1 * 2) + (uint32_t)(((lane % LPR_A) ^ swz(r)) * 16);
    }
#pragma unroll
    for (int i = 0; i < BPW; ++i) {
        const int byte = (BPW * wid + i) * 1024 + lane * 16;            // position in the LDS image of the B tile (row-major, T2*2-byte rows)
        const int r = byte / (T2 * 2), pos = (byte % (T2 * 2)) / 16;
        ob[i] = (uint32_t)r * (uint32_t)(ldb * 2) + (uint32_t)(c2 * 2) + (uint32_t)(chunk_pos<T2 * 2>(pos, r) * 16);
    }
    auto stage = [&](int slot, int kt) {
        const char* pa = (const char*)A + (size_t)(kbeg + kt) * BK * lda * 2;
        const char* pb = (const char*)B + (size_t)(kbeg + kt) * BK * ldb * 2;
        if (mtail != 0 && kbeg + kt == ktotal - 1) {
            // last, partial K tile: token rows >= M come from the zero page (once per workgroup at most; rows recomputed here
            // instead of being kept in registers)
            const char* zp = (const char*)g_zero_page + lane * 16;
            const uint32_t lb = (uint32_t)(uintptr_t)LDS_PTR(smem) + slot * SLOT;
#pragma unroll
            for (int i = 0; i < APW; ++i) {
                const int r = RA * (APW * wid + i) + lane / LPR_A;
                tn_dma16_addr(lb + (APW * wid + i) * 1024, r < mtail ? pa + oa[i] : zp);
            }
#pragma unroll
            for (int i = 0; i < BPW; ++i) {
                const int r = ((BPW * wid + i) * 1024 + lane * 16) / (T2 * 2);
                tn_dma16_addr(lb + A_BYTES + (BPW * wid + i) * 1024, r < mtail ? pb + ob[i] : zp);
            }
            return;
        }
        const uint32_t lbase = (uint32_t)(uintptr_t)LDS_PTR(smem) + slot * SLOT;
#pragma unroll
        for (int i = 0; i < APW; ++i) tn_dma16(lbase + (APW * wid + i) * 1024, oa[i], pa);
#pragma unroll
        for (int i = 0; i < BPW; ++i) tn_dma16(lbase + A_BYTES + (BPW * wid + i) * 1024, ob[i], pb);
    };

    // ---- transposed-read addressing: 16-lane group g reads token rows 8g+q (+4); lane (4q+pp) supplies cols 4pp..4pp+3.
    // Token row m = 32 ks + 8 g + 4 r + q: swz(m) depends on q and g only, so one LDS offset per column tile t covers every
    // k-step (ks: + 32 rows) and both reads (r: + 4 rows) through the instruction's immediate offset.
    const int g = lane >> 4, q = (lane >> 2) & 3, pp = lane & 3;
    const int m0 = 8 * g + q;
    uint32_t ra[FA], rb[NBF];
#pragma unroll
    for (int t = 0; t < FA; ++t) {
        const int ca = wm * (16 * FA) + t * 16 + 4 * pp;
        ra[t] = (uint32_t)(uintptr_t)LDS_PTR(smem) + m0 * (T1 * 2) + (((ca >> 3) ^ swz(m0)) * 16) + (ca & 7) * 2;
    }
#pragma unroll
    for (int t = 0; t < NBF; ++t) {
        const int cb = wn * (16 * NBF) + t * 16 + 4 * pp;
        rb[t] = (uint32_t)(uintptr_t)LDS_PTR(smem) + A_BYTES + m0 * (T2 * 2) + chunk_pos<T2 * 2>(cb >> 3, m0) * 16 + (cb & 7) * 2;
    }

    f32x4 acc[FA][NBF];
    f32x4 accb[FA];
#pragma unroll
    for (int i = 0; i < FA; ++i) {
        accb[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < NBF; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    const short one = F16 ? (short)0x3C00 : (short)0x3F80;     // 1.0 in the operand format
    const bf16x8 ones = (bf16x8){one, one, one, one, one, one, one, one};

    // waves w and w + NW/2 share a SIMD: the second half issues its LDS-DMA one k-step later, so the two do not stall the
    // MFMA pipe at the same time (measured on the NT kernel: +2..9 %)
    const bool late_wave = NW == 8 && wid >= 4;
    using KS0 = std::integral_constant<int, 0>;
    using KS1 = std::integral_constant<int, 1>;

    // The whole K sweep, instantiated twice: with and without the bias-gradient MFMA (B = all-ones) per A fragment.  Which one a wave
    // runs is decided ONCE (wave-uniform), not per fragment row: until round 3 every row of the K loop carried a v_cndmask / v_cmp /
    // s_cbranch and three v_mov rebuilding the all-ones operand.
    auto sweep = [&](auto bias_tag) {
        constexpr bool WB = decltype(bias_tag)::value;
        Frag af[FA], b0[NBF], b1[NBF];
        auto mfma_row = [&](int t1, Frag (&bc)[NBF]) {
            const bf16x8 a = frag8(af[t1]);
#pragma unroll
            for (int t2 = 0; t2 < NBF; ++t2)
                // swapped operands: D'[n2][n1] so the lane's 4 accumulators run along n2 (contiguous in dW rows)
                acc[t1][t2] = tn_mfma<F16>(frag8(bc[t2]), a, acc[t1][t2]);
            if constexpr (WB) accb[t1] = tn_mfma<F16>(ones, a, accb[t1]);
        };
        // K tile kt+1 must have landed (with three slots K tile kt+2, issued one tile ago, may stay in flight) and every read of this K
        // tile's slot must be back before the slot is handed to the DMA: lgkmcnt(0) covers the compiler's reads, which are all issued
        // above this point (sched_barrier).
        auto sync_and_recycle = [&](int slot, int kt) {
            if (NSLOT == 3 && kt + 2 < nk) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(G) : "memory");
            else asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            if (!late_wave && kt + NSLOT < nk) stage(slot, kt + NSLOT);  // slot of K tile kt: every wave holds its fragments in registers
            __builtin_amdgcn_sched_barrier(0);
        };
        // one 32-token k-step over (af, bc), FA < 8 (the 128 x 128 tile); the next fragments come from slot offset noff, k-step NKS of that slot.
        // Reads are issued right behind the MFMA row that last used their destination; the compiler waits (exact lgkmcnt) where a fragment is used.
        auto kstep = [&](Frag (&bc)[NBF], Frag (&bn)[NBF], uint32_t noff, auto nks_tag, bool sync, int slot, int kt) {
            constexpr int NKS = decltype(nks_tag)::value;
            constexpr int OA = NKS * 32 * T1 * 2, OB = NKS * 32 * T2 * 2;
            mfma_row(0, bc);
            __builtin_amdgcn_sched_barrier(0);
            if (sync) {
                sync_and_recycle(slot, kt);
            } else if (late_wave && slot >= 0 && kt + NSLOT < nk) {
                stage(slot, kt + NSLOT);                       // postponed from the previous K tile's barrier (see gemm_nt_ring.hip)
                __builtin_amdgcn_sched_barrier(0);
            }
            tr_issue<OA, 4 * T1 * 2>(af[0], ra[0] + noff);
#pragma unroll
            for (int t = 0; t < NBF; ++t) tr_issue<OB, 4 * T2 * 2>(bn[t], rb[t] + noff);
#pragma unroll
            for (int t1 = 1; t1 < FA; ++t1) {
                __builtin_amdgcn_sched_barrier(0);
                mfma_row(t1, bc);
                __builtin_amdgcn_sched_barrier(0);
                tr_issue<OA, 4 * T1 * 2>(af[t1], ra[t1] + noff);
            }
            __builtin_amdgcn_sched_barrier(0);
        };
        // FA = 8 (the 256-row tiles): A fragments are refilled FOUR rows after their last use instead of at once, so that every request is
        // four MFMA rows old when its fragment is used: fragment f of k-step s+1 is requested after row f + 4 (rows 0..3 request fragments
        // 4..7 of the SAME k-step, rows 4..7 fragments 0..3 and B of the next one).  A k-step starts with A0..A3 and B in registers only;
        // the slot of K tile kt is free (barrier + DMA of K tile kt+2) after row 4 of its second k-step; the very last k-step still issues
        // its (unused) requests, which the compiler retires before the registers are reused.
        // one 32-token k-step; current fragments at slot offset coff / k-step CKS, the next k-step's at noff / NKS
        auto kstep8 = [&](Frag (&bc)[NBF], Frag (&bn)[NBF], uint32_t coff, auto cks_tag, uint32_t noff, auto nks_tag, bool sync, int slot, int kt) {
            constexpr int CKS = decltype(cks_tag)::value, NKS = decltype(nks_tag)::value;
            constexpr int COA = CKS * 32 * T1 * 2, NOA = NKS * 32 * T1 * 2, NOB = NKS * 32 * T2 * 2;
            mfma_row(0, bc);
            __builtin_amdgcn_sched_barrier(0);
            if (!sync && late_wave && slot >= 0 && kt + NSLOT < nk) {
                stage(slot, kt + NSLOT);                       // postponed from the previous K tile's barrier (see gemm_nt_ring.hip)
                __builtin_amdgcn_sched_barrier(0);
            }
            tr_issue<COA, 4 * T1 * 2>(af[4], ra[4] + coff);
#pragma unroll
            for (int t1 = 1; t1 < 4; ++t1) {
                __builtin_amdgcn_sched_barrier(0);
                mfma_row(t1, bc);
                __builtin_amdgcn_sched_barrier(0);
                tr_issue<COA, 4 * T1 * 2>(af[t1 + 4], ra[t1 + 4] + coff);
            }
            __builtin_amdgcn_sched_barrier(0);
            mfma_row(4, bc);
            __builtin_amdgcn_sched_barrier(0);
            if (sync) sync_and_recycle(slot, kt);
#pragma unroll
            for (int t = 0; t < NBF; ++t) tr_issue<NOB, 4 * T2 * 2>(bn[t], rb[t] + noff);
            tr_issue<NOA, 4 * T1 * 2>(af[0], ra[0] + noff);
#pragma unroll
            for (int t1 = 5; t1 < 8; ++t1) {
                __builtin_amdgcn_sched_barrier(0);
                mfma_row(t1, bc);
                __builtin_amdgcn_sched_barrier(0);
                tr_issue<NOA, 4 * T1 * 2>(af[t1 - 4], ra[t1 - 4] + noff);
            }
            __builtin_amdgcn_sched_barrier(0);
        };

        if constexpr (FA == 8) {
            stage(0, 0);
            if (NSLOT == 3 && nk > 1) {
                stage(1, 1);
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(G) : "memory");
            } else {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            if (NSLOT == 3) { if (nk > 2) stage(2, 2); } else { if (nk > 1) stage(1, 1); }
#pragma unroll
            for (int t = 0; t < NBF; ++t) tr_issue<0, 4 * T2 * 2>(b0[t], rb[t]);
#pragma unroll
            for (int t = 0; t < 4; ++t) tr_issue<0, 4 * T1 * 2>(af[t], ra[t]);
            int cs = 0, ps = -1;                               // slots of K tiles kt and kt-1
            for (int kt = 0; kt + 1 < nk; ++kt) {
                const int ns = cs == NSLOT - 1 ? 0 : cs + 1;
                kstep8(b0, b1, (uint32_t)(cs * SLOT), KS0{}, (uint32_t)(cs * SLOT), KS1{}, false, ps, kt - 1);
                kstep8(b1, b0, (uint32_t)(cs * SLOT), KS1{}, (uint32_t)(ns * SLOT), KS0{}, true, cs, kt);
                ps = cs;
                cs = ns;
            }
            kstep8(b0, b1, (uint32_t)(cs * SLOT), KS0{}, (uint32_t)(cs * SLOT), KS1{}, false, ps, nk - 2);
            kstep8(b1, b0, (uint32_t)(cs * SLOT), KS1{}, (uint32_t)(cs * SLOT), KS0{}, false, -1, nk);      // its next-k-step requests read stale LDS: unused
        } else {
            stage(0, 0);
            if (NSLOT == 3 && nk > 1) {
                stage(1, 1);
                asm volatile("s_waitcnt vmcnt(%0)" ::"n"(G) : "memory");
            } else {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
            if (NSLOT == 3) { if (nk > 2) stage(2, 2); } else { if (nk > 1) stage(1, 1); }
            tr_issue<0, 4 * T1 * 2>(af[0], ra[0]);
#pragma unroll
            for (int t = 0; t < NBF; ++t) tr_issue<0, 4 * T2 * 2>(b0[t], rb[t]);
#pragma unroll
            for (int t = 1; t < FA; ++t) tr_issue<0, 4 * T1 * 2>(af[t], ra[t]);
            int cs = 0, ps = -1;                               // slots of K tiles kt and kt-1
            for (int kt = 0; kt + 1 < nk; ++kt) {
                const int ns = cs == NSLOT - 1 ? 0 : cs + 1;
                kstep(b0, b1, (uint32_t)(cs * SLOT), KS1{}, false, ps, kt - 1);
                kstep(b1, b0, (uint32_t)(ns * SLOT), KS0{}, true, cs, kt);
                ps = cs;
                cs = ns;
            }
            kstep(b0, b1, (uint32_t)(cs * SLOT), KS1{}, false, ps, nk - 2);
#pragma unroll
            for (int t1 = 0; t1 < FA; ++t1) mfma_row(t1, b1);
        }
    };
    if (nk > 0) {
        if (do_bias) sweep(std::true_type{});
        else sweep(std::false_type{});
    }

    // ---- output.  One chunk: the tile is complete, write (or add to) dW / dbias directly.  Several: this chunk's slab.
    const bool direct = P.chunks == 1;
    float* outW = direct ? P.dW : ga.slabs + P.slab_off + (size_t)slab * ((size_t)N1 * N2 + (size_t)N1);
    float* outB = direct ? P.dbias : outW + (size_t)N1 * N2;
    const bool add = direct && ga.accumulate != 0;
    const float osc = (direct && ga.inv_scale) ? *ga.inv_scale : 1.0f;      // slabs stay raw: the reduction applies the factor
#pragma unroll
    for (int t1 = 0; t1 < FA; ++t1) {
        const int n1 = c1 + wm * (16 * FA) + t1 * 16 + (lane & 15);
#pragma unroll
        for (int t2 = 0; t2 < NBF; ++t2) {
            const int n2 = c2 + wn * (16 * NBF) + t2 * 16 + 4 * (lane >> 4);
            float4 v = make_float4(acc[t1][t2][0] * osc, acc[t1][t2][1] * osc, acc[t1][t2][2] * osc, acc[t1][t2][3] * osc);
            float4* dst = (float4*)(outW + (size_t)n1 * N2 + n2);
            if (add) { const float4 o = *dst; v.x += o.x; v.y += o.y; v.z += o.z; v.w += o.w; }
            *dst = v;
        }
        if (do_bias && lane < 16) {       // every n2 row of D' holds the same column sums
            float b = accb[t1][0] * osc;
            if (add) b += outB[n1];
            outB[n1] = b;
        }
    }
}

// out[i] (+)= sum_s slabs[s][i], fixed order; the tail [n_main, n_main + n_bias) goes to out_bias.
__global__ void reduce_slabs_kernel(const float* __restrict__ slabs, float* __restrict__ out, float* __restrict__ out_bias,
                                    size_t n_main4, size_t n_all4, int splits, size_t slab_stride4, int accumulate) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_all4; i += stride) {
        float4 s = ((const float4*)slabs)[i];
        for (int k = 1; k < splits; ++k) {
            const float4 t = ((const float4*)slabs)[i + k * slab_stride4];
            s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
        }
        float4* dst = i < n_main4 ? (float4*)out + i : (float4*)out_bias + (i - n_main4);
        if (accumulate) {
            const float4 o = *dst;
            s.x += o.x; s.y += o.y; s.z += o.z; s.w += o.w;
        }
        *dst = s;
    }
}

// the same for every problem of a group in one launch: blockIdx.y = problem.  A problem with a single chunk has no slabs (the GEMM wrote
// its dW); when the clip norm's partial sums are wanted it is read once more here, so that the sink sees everything the group wrote.
__global__ __launch_bounds__(256) void reduce_slabs_group_kernel(TnGroupArgs ga) {
    const TnProblem& P = ga.p[blockIdx.y];
    if (P.chunks == 1 && !ga.sq_out) return;            // written directly by the GEMM and nobody asks for its sum of squares
    const size_t n_main4 = (size_t)P.N1 * P.N2 / 4, n_all4 = n_main4 + (P.dbias ? (size_t)P.N1 / 4 : 0);
    const size_t stride4 = ((size_t)P.N1 * P.N2 + (size_t)P.N1) / 4;
    const float4* slabs = (const float4*)(ga.slabs + P.slab_off);
    const size_t step = (size_t)gridDim.x * blockDim.x;
    const float osc = ga.inv_scale ? *ga.inv_scale : 1.0f;
    float sq = 0.f;
    if (P.chunks == 1) {
        // no slabs: the GEMM launch in front of this one wrote dW / dbias; only the clip norm's share is taken here (same slots, same order)
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_all4; i += step) {
            const float4 s = i < n_main4 ? ((const float4*)P.dW)[i] : ((const float4*)P.dbias)[i - n_main4];
            sq += s.x * s.x + s.y * s.y + s.z * s.z + s.w * s.w;
        }
    }
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; P.chunks > 1 && i < n_all4; i += step) {
        float4 s = slabs[i];
        for (int k = 1; k < P.chunks; ++k) {
            const float4 t = slabs[i + k * stride4];
            s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
        }
        s.x *= osc; s.y *= osc; s.z *= osc; s.w *= osc;
        float4* dst = i < n_main4 ? (float4*)P.dW + i : (float4*)P.dbias + (i - n_main4);
        if (ga.accumulate) {
            const float4 o = *dst;
            s.x += o.x; s.y += o.y; s.z += o.z; s.w += o.w;
        }
        *dst = s;
        sq += s.x * s.x + s.y * s.y + s.z * s.z + s.w * s.w;
    }
    if (ga.sq_out) {       // the clip norm's share of this workgroup (capi.hip: cldrd_set_norm_sink): fixed order, no atomics
        __shared__ float red[4];
        sq = wave_sum(sq);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sq;
        __syncthreads();
        if (threadIdx.x == 0) ga.sq_out[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
    }
}

}  // namespace

// ---- host side ---------------------------------------------------------------------------------------------------------
struct WgradTile { int t1, t2; };
constexpr int WGRAD_MAXK = 256;      // longest item in K tiles: the drift cap, see wgrad_splits_group

// One tile shape per launch: 256 x 192 (8 waves of 128 x 48: 7 LDS-DMA pieces per 48 MFMAs per wave, the ratio of the NT kernel's
// BN = 192) when every problem allows it, else 256 x 128 (8 waves of 64 x 64), else 128 x 128 (4 waves).  The 256 x 256 tile of
// round 1 (all 256 VGPRs, spills, two LDS slots: 430-480 TF/s against 690-810) came back in round 4 without the spills (below).
static WgradTile wgrad_tile_group(const int* N1, const int* N2, int n) {
    bool ok192 = true, ok128w = true;
    for (int i = 0; i < n; ++i) {
        ok192 = ok192 && N1[i] % 256 == 0 && N2[i] % 192 == 0;
        ok128w = ok128w && N1[i] % 256 == 0 && N2[i] % 128 == 0;
    }
    bool ok256 = true;
    for (int i = 0; i < n; ++i) ok256 = ok256 && N1[i] % 256 == 0 && N2[i] % 256 == 0;
    // Round 4: 256 x 256 (8 waves of 128 x 64; 256 VGPRs, no spills with the rewritten K sweep, two 64-KiB LDS slots) for GROUPS: 8 LDS-DMA
    // pieces per 64 MFMAs per wave instead of 7 per 48, and the passage tower's three-layer group becomes 324 tiles instead of 432.  Alone per
    // problem it is +3..7 % on the FFN shapes, -2 % on QKV, -14 % at 4096^3; in the step 11.70 -> 11.44 and 11.67 ->
    // 11.48 ms (profiles/r04_microbench.txt).  Single problems keep the measured per-shape choice below.
    if (ok256 && n > 1) return {256, 256};
    if (ok192 && (!ok128w || n > 1)) return {256, 192};
    if (ok192) {
        // single problem: small outputs stay on 256 x 128 (measured at T = 32768: 768 x 768 -7 % on 256 x 192, the others +3..10 %)
        if ((N1[0] / 256) * (N2[0] / 192) >= 24) return {256, 192};
    }
    if (ok128w) return {256, 128};
    return {128, 128};
}

// Token splits per output tile.  One workgroup occupies a CU (LDS).  With `sp` splits an item of problem p sweeps
// ceil(ktotal_p / sp) K tiles plus a fixed cost (pipeline fill, output write) of about OVERHEAD K-tile times; the items are handed
// out in order, so the launch takes about (total work / 256 CUs) rounded up to whole largest items.  Splits > 1 add the fp32 slabs
// written and read back (bytes / ~5 TB/s, in units of the ~1.5 us a K tile takes) and the reduction launches.  Smallest modelled
// time wins; ties go to fewer splits.  (Weighting every problem by its OWN token count matters: the 120 tiles of the CLS-only last
// layer sweep 4 K tiles, the 744 of the full layers 512 - counting them alike chose 2 splits and paid 0.3 GB of slabs per step.)
static int wgrad_splits_group(const int* M, const int* N1, const int* N2, int n, WgradTile t) {
    int ktotal = 1;
    double out_bytes = 0.0;
    long tiles_all = 0;
    for (int i = 0; i < n; ++i) {
        ktotal = ktotal > (M[i] + BK - 1) / BK ? ktotal : (M[i] + BK - 1) / BK;
        out_bytes += 4.0 * N1[i] * N2[i];
        tiles_all += (long)(N1[i] / t.t1) * (N2[i] / t.t2);
    }
    if (tiles_all <= 0) return 1;
    const int overhead = 6;
    // Workgroups of one XCD share A / B panels through its 4-MiB L2 only while they sweep the same token range at about the same
    // time; nothing synchronises them, so over a long sweep they drift apart and every one of them streams its operands from HBM
    // (measured at cfg2: 512 K tiles per item, no split: 3.2 ms for the passage tower's group; 2 splits of 256: 2.9 ms + 0.1 ms of
    // slabs).  Items are therefore capped at WGRAD_MAXK K tiles.
    const int sp_min = (ktotal + WGRAD_MAXK - 1) / WGRAD_MAXK;
    int best = sp_min;
    double best_cost = -1.0;
    for (int sp = sp_min; sp <= 64 && sp <= ktotal; ++sp) {
        double work = 0.0;
        for (int i = 0; i < n; ++i) {
            const long tiles = (long)(N1[i] / t.t1) * (N2[i] / t.t2);
            const int kt = (M[i] + BK - 1) / BK;
            work += (double)tiles * sp * ((kt + sp - 1) / sp + overhead);
        }
        const double item = (ktotal + sp - 1) / sp + overhead;
        double cost = item * (double)(long)((work / 256.0 + item - 1e-9) / item);          // whole largest items
        if (cost < item) cost = item;
        if (sp > 1) cost += 2.0 * sp * out_bytes / 5.0e12 / 1.5e-6 + 4.0;
        if (best_cost < 0 || cost < best_cost - 1e-9) { best_cost = cost; best = sp; }
    }
    return best;
}


// ---- chunk plan of a group launch -----------------------------------------------------------------------------------------------------
// One split count for the whole launch leaves a tail: at cfg2 the passage tower's 25 problems become 1 674 items of 171 K tiles (+ the
// CLS-only layer's four-K-tile ones), 6.5 items per CU, and the last round runs a third full.  A plan gives every problem its own cut -
// n_long chunks of c_long K tiles, then n_short chunks of c_short - and the launch runs all long items first, the short ones last, so
// the short items fill the tail.  The plan is a pure function of the shapes: a small candidate set (every uniform count, as before, and
// c_long x c_short x the share of long ranges re-cut into short chunks) is scored by replaying the dispatch - 256 CUs, one workgroup
// each (LDS), items handed out in launch order to whichever CU is free first, item cost = K tiles + OVERHEAD - plus the slab bytes
// and the reduction launch in the same units as wgrad_splits_group.  Smallest modelled time wins among the candidates whose replay is
// no longer than that of every uniform count up to 8; ties go to the earlier candidate (uniform, fewer chunks).
struct WgradChunks { int n_long, c_long, n_short, c_short; };
struct WgradPlan {
    WgradChunks p[MAXP];
    int items_long, items_short;
    double makespan, cost;             // replayed dispatch; + slab traffic and reduction launch
};

static inline int wgrad_ktiles(int M) { return (M + BK - 1) / BK; }
static inline int wgrad_chunks(const WgradChunks& c) { return c.n_long + c.n_short; }
static inline int xcd_remap_host(int orig, int nwg) {          // common.h: xcd_remap
    const int q = nwg >> 3, r = nwg & 7, xcd = orig & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (orig >> 3);
}

// Fills items_*, makespan and cost of `pl` from its chunk table.  `beat` >= 0: the replay is skipped (false) when even perfectly balanced
// work could not come in under `beat`.
static bool wgrad_plan_score(const int* M, const int* N1, const int* N2, int n, WgradTile t, WgradPlan& pl, double beat = -1.0) {
    const int overhead = 6, slots = 256;
    double slab_bytes = 0.0, work = 0.0, longest = 0.0;
    std::vector<float> cost[2];                                // per item, in item order of its region
    for (int i = 0; i < n; ++i) {
        const int tiles = (N1[i] / t.t1) * (N2[i] / t.t2), kt = wgrad_ktiles(M[i]);
        const WgradChunks& c = pl.p[i];
        if (wgrad_chunks(c) > 1) slab_bytes += 2.0 * wgrad_chunks(c) * 4.0 * N1[i] * N2[i];
        for (int rg = 0; rg < 2; ++rg) {
            const int clen = rg ? c.c_short : c.c_long;
            for (int ch = 0; ch < (rg ? c.n_short : c.n_long); ++ch) {
                const int kbeg = (rg ? c.n_long * c.c_long : 0) + ch * clen;
                const int nk = std::max(0, std::min(kt, kbeg + clen) - kbeg);      // (a uniform split of a short problem has empty chunks)
                cost[rg].insert(cost[rg].end(), (size_t)tiles, (float)(nk + overhead));
                work += (double)tiles * (nk + overhead);
                longest = std::max(longest, (double)(nk + overhead));
            }
        }
    }
    pl.items_long = (int)cost[0].size();
    pl.items_short = (int)cost[1].size();
    const double extra = slab_bytes > 0.0 ? slab_bytes / 5.0e12 / 1.5e-6 + 4.0 : 0.0;      // slabs written and read back, the reduction launch
    if (beat >= 0.0 && std::max(work / slots, longest) + extra >= beat) return false;
    std::vector<double> heap(slots, 0.0);                      // min-heap of the times at which the CUs fall free
    double end = 0.0;
    for (int rg = 0; rg < 2; ++rg) {
        const int cnt = (int)cost[rg].size();
        for (int s = 0; s < cnt; ++s) {                        // launch order: the kernel's xcd_remap per region
            std::pop_heap(heap.begin(), heap.end(), std::greater<double>());
            heap.back() += cost[rg][xcd_remap_host(s, cnt)];
            end = std::max(end, heap.back());
            std::push_heap(heap.begin(), heap.end(), std::greater<double>());
        }
    }
    pl.makespan = end;
    pl.cost = end + extra;
    return true;
}

// `sp` chunks of ceil(ktotal / sp) K tiles for every problem, all in the long region: what a launch did before there was a plan (a short
// problem then gets empty chunks too); `trim` drops those
static void wgrad_plan_uniform(const int* M, int n, int sp, bool trim, WgradPlan& pl) {
    for (int i = 0; i < n; ++i) {
        const int kt = wgrad_ktiles(M[i]), per = (kt + sp - 1) / sp;
        pl.p[i] = {trim ? (kt + per - 1) / per : sp, per, 0, 0};
    }
}

static WgradPlan wgrad_plan_search(const int* M, const int* N1, const int* N2, int n, WgradTile t, int force_uniform) {
    WgradPlan best;
    int ktotal = 1;
    for (int i = 0; i < n; ++i) ktotal = std::max(ktotal, wgrad_ktiles(M[i]));
    // one problem keeps the rule (and the bits) it had
    if (force_uniform > 0 || n == 1) {
        wgrad_plan_uniform(M, n, force_uniform > 0 ? std::min(force_uniform, ktotal) : wgrad_splits_group(M, N1, N2, n, t), false, best);
        wgrad_plan_score(M, N1, N2, n, t, best);
        return best;
    }
    // A plan must also replay no longer than the best of the uniform counts up to 8 does (slab bytes aside): that one is always eligible.
    WgradPlan c;
    double span_cap = -1.0;
    for (int sp = (ktotal + WGRAD_MAXK - 1) / WGRAD_MAXK; sp <= 8 && sp <= ktotal; ++sp) {
        wgrad_plan_uniform(M, n, sp, true, c);
        wgrad_plan_score(M, N1, N2, n, t, c);
        if (span_cap < 0.0 || c.makespan < span_cap) span_cap = c.makespan;
    }
    bool have = false;
    auto consider = [&](WgradPlan& c) {
        if (!wgrad_plan_score(M, N1, N2, n, t, c, have ? best.cost - 1e-9 : -1.0)) return;
        if (span_cap >= 0.0 && c.makespan > span_cap + 1e-9) return;
        if (!have || c.cost < best.cost - 1e-9) { best = c; have = true; }
    };
    for (int sp = (ktotal + WGRAD_MAXK - 1) / WGRAD_MAXK; sp <= 64 && sp <= ktotal; ++sp) {
        wgrad_plan_uniform(M, n, sp, true, c);
        consider(c);
    }
    static const int c_longs[] = {256, 171, 128}, c_shorts[] = {32, 64, 128};
    static const double shares[] = {0.0, 1.0 / 16, 1.0 / 8, 3.0 / 16, 1.0 / 4, 3.0 / 8, 1.0 / 2};
    for (int cl : c_longs) {
        for (int cs : c_shorts) {
            if (cs >= cl) continue;
            // long ranges of a problem: ceil(kt / cl); problems of at most cs K tiles are one short item.  `want` of all (tile, range)
            // pairs are re-cut, taken from the end of the problem list, a problem's last range first: fixed shares, and what the long
            // items have beyond whole rounds of 256 CUs (the short items then start on a level front).
            long all = 0;
            for (int i = 0; i < n; ++i)
                if (wgrad_ktiles(M[i]) > cs) all += (long)(N1[i] / t.t1) * (N2[i] / t.t2) * ((wgrad_ktiles(M[i]) + cl - 1) / cl);
            // (want, cover): cover = re-cut at least `want` (one more range of the smallest problem that still has one), else at most
            std::vector<std::pair<long, bool>> wants;
            for (double share : shares) wants.push_back({(long)(share * (double)all + 0.5), false});
            for (long rounds = all / 256; rounds >= 0 && rounds + 2 > all / 256; --rounds) wants.push_back({all - 256 * rounds, true});
            for (const auto& w : wants) {
                int nl[MAXP];
                long done = 0;
                for (int i = n - 1; i >= 0; --i) {
                    const int kt = wgrad_ktiles(M[i]);
                    const long tiles = (long)(N1[i] / t.t1) * (N2[i] / t.t2);
                    nl[i] = kt <= cs ? 0 : (kt + cl - 1) / cl;
                    while (nl[i] > 0 && done + tiles <= w.first) { --nl[i]; done += tiles; }
                }
                if (w.second && done < w.first) {
                    int pick = -1;
                    for (int i = n - 1; i >= 0; --i)
                        if (nl[i] > 0 && (pick < 0 || (N1[i] / t.t1) * (N2[i] / t.t2) < (N1[pick] / t.t1) * (N2[pick] / t.t2))) pick = i;
                    if (pick >= 0) --nl[pick];
                }
                for (int i = 0; i < n; ++i) {
                    const int kt = wgrad_ktiles(M[i]);
                    if (kt <= cs) { c.p[i] = {0, cl, 1, kt}; continue; }
                    const int rest = kt - std::min(kt, nl[i] * cl);
                    c.p[i] = {nl[i], cl, (rest + cs - 1) / cs, cs};
                }
                consider(c);
            }
        }
    }
    return best;
}

// the search is repeated for every launch of an eager step: remember the last few answers (shapes, tile and the forced split count are the key)
static WgradPlan wgrad_plan_group(const int* M, const int* N1, const int* N2, int n, WgradTile t, int force_uniform = 0) {
    struct Entry { std::vector<int> key; WgradPlan plan; };
    thread_local std::vector<Entry> cache;
    std::vector<int> key = {n, t.t1, t.t2, force_uniform};
    for (int i = 0; i < n; ++i) { key.push_back(M[i]); key.push_back(N1[i]); key.push_back(N2[i]); }
    for (const Entry& e : cache)
        if (e.key == key) return e.plan;
    if (cache.size() >= 16) cache.erase(cache.begin());
    cache.push_back({key, wgrad_plan_search(M, N1, N2, n, t, force_uniform)});
    return cache.back().plan;
}

// The planner's answer for inspection (host only, no device call; tests/test_wgrad_plan.py).  Per problem: chunks[4 i ..] = n_long,
// c_long, n_short, c_short (K tiles of 64 tokens).  info[0..7] = tile rows, tile columns, work items, launches, bytes of the kernel-argument
// block, its limit, problems per launch, 0.  model[0] = replayed makespan, model[1] = modelled cost (K-tile times; summed over the launches).
// uniform_splits > 0: that many token splits for every problem, the form every group launch had before, scored by the same model.
extern "C" int cldrd_wgrad_plan(const int* M, const int* N1, const int* N2, int n, int uniform_splits, int* chunks, int* info, double* model) {
    CLDRD_CHECK(n > 0, "wgrad_plan: no problems");
    for (int i = 0; i < n; ++i)
        CLDRD_CHECK(M[i] > 0 && N1[i] % 128 == 0 && (N2[i] % 128 == 0 || (N1[i] % 256 == 0 && N2[i] % 192 == 0)), "wgrad_plan: unsupported shape");
    const WgradTile t = wgrad_tile_group(N1, N2, n);
    int items = 0, launches = 0;
    double makespan = 0.0, cost = 0.0;
    for (int lo = 0; lo < n; lo += MAXP, ++launches) {
        const int m = std::min(n - lo, MAXP);
        const WgradPlan pl = wgrad_plan_group(M + lo, N1 + lo, N2 + lo, m, t, uniform_splits);
        for (int i = 0; i < m; ++i) {
            chunks[4 * (lo + i) + 0] = pl.p[i].n_long; chunks[4 * (lo + i) + 1] = pl.p[i].c_long;
            chunks[4 * (lo + i) + 2] = pl.p[i].n_short; chunks[4 * (lo + i) + 3] = pl.p[i].c_short;
        }
        items += pl.items_long + pl.items_short;
        makespan += pl.makespan;
        cost += pl.cost;
    }
    info[0] = t.t1; info[1] = t.t2; info[2] = items; info[3] = launches;
    info[4] = (int)sizeof(TnGroupArgs); info[5] = 4096; info[6] = MAXP; info[7] = 0;
    model[0] = makespan; model[1] = cost;
    return 0;
}

extern "C" int cldrd_wgrad_splits(int M, int N1, int N2) {
    if (N1 % 128 != 0 || !(N2 % 128 == 0 || (N1 % 256 == 0 && N2 % 192 == 0))) return 1;
    return wgrad_splits_group(&M, &N1, &N2, 1, wgrad_tile_group(&N1, &N2, 1));
}

template <int T1, int T2, int NW, bool F16 = false>
static int launch_tn_group(const TnGroupArgs& g, int items, hipStream_t st) {
    constexpr int slot = BK * (T1 + T2) * 2;
    constexpr int lds = (3 * slot <= 160 * 1024 ? 3 : 2) * slot;
    static bool attr_set = false;
    if (!attr_set) {
        (void)hipFuncSetAttribute((const void*)gemm_tn_kernel<T1, T2, NW, F16>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        attr_set = true;
    }
    hipLaunchKernelGGL((gemm_tn_kernel<T1, T2, NW, F16>), dim3(items), dim3(64 * NW), lds, st, g);
    CLDRD_LAUNCH_CHECK();
    return 0;
}

// floats of workspace a group needs (0 when no token split is used)
extern "C" size_t cldrd_wgrad_group_workspace(const int* M, const int* N1, const int* N2, int n) {
    if (n <= 0) return 0;
    const WgradTile t = wgrad_tile_group(N1, N2, n);
    size_t tot = 0;
    for (int lo = 0; lo < n; lo += MAXP) {
        const int m = n - lo < MAXP ? n - lo : MAXP;
        const WgradPlan pl = wgrad_plan_group(M + lo, N1 + lo, N2 + lo, m, t);
        for (int i = 0; i < m; ++i)
            if (wgrad_chunks(pl.p[i]) > 1) tot += (size_t)wgrad_chunks(pl.p[i]) * ((size_t)N1[lo + i] * N2[lo + i] + (size_t)N1[lo + i]);
    }
    return tot;
}

// dW[i][N1[i], N2[i]] (+)= A[i][:M[i]]^T . B[i][:M[i]] and dbias[i][N1[i]] (+)= column sums of A[i] (dbias[i] may be null) for n
// problems in one launch (more than 32: several launches).  The pointer / shape arrays live on the HOST.
extern "C" int cldrd_wgrad_group(const void* const* A, const void* const* B, float* const* dW, float* const* dbias, const int* M,
                                 const int* N1, const int* N2, const int* lda, const int* ldb, int n, float* workspace,
                                 size_t workspace_bytes, int accumulate, void* stream) {
    CLDRD_CHECK(n > 0, "wgrad_group: no problems");
    for (int i = 0; i < n; ++i) {
        CLDRD_CHECK(M[i] > 0, "wgrad: empty problem");
        CLDRD_CHECK(N1[i] % 128 == 0 && (N2[i] % 128 == 0 || (N1[i] % 256 == 0 && N2[i] % 192 == 0)),
                    "wgrad: N1 and N2 must be multiples of 128 (or 256 x 192)");
        CLDRD_CHECK(lda[i] % 8 == 0 && ldb[i] % 8 == 0, "wgrad: lda/ldb must be multiples of 8");
        CLDRD_CHECK(((uintptr_t)A[i] % 16 == 0) && ((uintptr_t)B[i] % 16 == 0) && ((uintptr_t)dW[i] % 16 == 0), "wgrad: operands must be 16-byte aligned");
        CLDRD_CHECK(dbias[i] == nullptr || (uintptr_t)dbias[i] % 16 == 0, "wgrad: dbias must be 16-byte aligned");
        CLDRD_CHECK((double)lda[i] * 2.0 * 72.0 < 4.0e9 && (double)ldb[i] * 2.0 * 72.0 < 4.0e9, "wgrad: row pitch too large");
    }
    hipStream_t st = (hipStream_t)stream;
    const WgradTile t = wgrad_tile_group(N1, N2, n);
    bool any128 = false;
    for (int i = 0; i < n; ++i) any128 = any128 || N2[i] % 128 != 0;
    CLDRD_CHECK(!(t.t2 != 192 && any128), "wgrad_group: problems with N2 % 128 != 0 need every problem to fit the 256 x 192 tile");
    const size_t need = cldrd_wgrad_group_workspace(M, N1, N2, n);
    CLDRD_CHECK(need == 0 || (workspace != nullptr && ((uintptr_t)workspace % 16 == 0) && workspace_bytes >= need * sizeof(float)), "wgrad: workspace too small");
    size_t slab_off = 0;
    for (int lo = 0; lo < n; lo += MAXP) {
        const int m = n - lo < MAXP ? n - lo : MAXP;
        const WgradPlan pl = wgrad_plan_group(M + lo, N1 + lo, N2 + lo, m, t);
        TnGroupArgs g;
        g.n = m; g.items_long = pl.items_long; g.accumulate = accumulate & 1; g.slabs = workspace;
        g.inv_scale = g_cldrd_loss_scale ? g_cldrd_loss_scale + 1 : nullptr;
        g.sq_out = nullptr;
        int first[2] = {0, 0};
        bool reduce = false;
        for (int i = 0; i < m; ++i) {
            TnProblem& P = g.p[i];
            const int j = lo + i;
            P.A = (const bf16_t*)A[j]; P.B = (const bf16_t*)B[j]; P.dW = dW[j]; P.dbias = dbias[j];
            P.M = M[j]; P.N1 = N1[j]; P.N2 = N2[j]; P.lda = lda[j]; P.ldb = ldb[j];
            P.nt2 = N2[j] / t.t2; P.nt1 = N1[j] / t.t1; P.tiles = P.nt1 * P.nt2;
            // The 32 workgroups that run side by side on one XCD take consecutive tiles of a problem and share operand panels through its
            // L2.  With n2 fastest they cover (32 / nt2) A panels x all nt2 B panels: fine while nt2 is small (QKV, FFN1: nt2 = 4).  FFN2 has
            // 3 n1 tiles x 16 n2 tiles: n2 fastest covers 2 of the 3 rows, so every panel of h (the 200-MB operand) is fetched by 2 concurrent
            // tiles now and again by the third row later; n1 fastest puts all 3 tiles of an h panel side by side: h streams from HBM once.
            P.n1_fast = (P.nt2 > P.nt1 && P.nt1 <= 32) ? 1 : 0;
            P.first[0] = first[0]; P.first[1] = first[1];
            P.clen[0] = pl.p[i].c_long; P.clen[1] = pl.p[i].c_short;
            P.n_long = pl.p[i].n_long; P.chunks = wgrad_chunks(pl.p[i]);
            P.slab_off = (long long)slab_off;
            first[0] += P.tiles * pl.p[i].n_long; first[1] += P.tiles * pl.p[i].n_short;
            if (P.chunks > 1) { slab_off += (size_t)P.chunks * ((size_t)N1[j] * N2[j] + (size_t)N1[j]); reduce = true; }
        }
        const int items = first[0] + first[1];
        int rc;
        if (t.t2 == 256) {
            rc = (accumulate & 2) ? launch_tn_group<256, 256, 8, true>(g, items, st) : launch_tn_group<256, 256, 8>(g, items, st);
        } else if (accumulate & 2) {             // bit 1 of `accumulate`: fp16 operands
            if (t.t1 == 256 && t.t2 == 192) rc = launch_tn_group<256, 192, 8, true>(g, items, st);
            else if (t.t1 == 256) rc = launch_tn_group<256, 128, 8, true>(g, items, st);
            else rc = launch_tn_group<128, 128, 4, true>(g, items, st);
        } else if (t.t1 == 256 && t.t2 == 192) rc = launch_tn_group<256, 192, 8>(g, items, st);
        else if (t.t1 == 256) rc = launch_tn_group<256, 128, 8>(g, items, st);
        else rc = launch_tn_group<128, 128, 4>(g, items, st);
        if (rc) return rc;
        if (!reduce) cldrd_norm_sink_miss();          // every tile written directly by the GEMM: no slab reduction to take the sums of squares from
        if (reduce) {
            size_t biggest = 0;
            for (int i = 0; i < m; ++i) biggest = biggest > (size_t)g.p[i].N1 * g.p[i].N2 / 4 ? biggest : (size_t)g.p[i].N1 * g.p[i].N2 / 4;
            const int rb = (int)((biggest + 255) / 256 < 256 ? (biggest + 255) / 256 : 256);
            g.sq_out = cldrd_norm_sink_take(rb * m);       // clip-norm partial sums of what this reduction writes, when a sink is set
            hipLaunchKernelGGL(reduce_slabs_group_kernel, dim3(rb, m), dim3(256), 0, st, g);       // one reduction launch for the group
            CLDRD_LAUNCH_CHECK();
        }
    }
    return 0;
}

// the single-problem form (a group of one).  workspace floats needed: cldrd_wgrad_splits(M, N1, N2) * (N1*N2 + N1)
extern "C" int cldrd_wgrad16(const void* A, const void* B, float* dW, float* dbias, int M, int N1, int N2, int lda, int ldb,
                                float* workspace, size_t workspace_bytes, int accumulate, void* stream) {
    return cldrd_wgrad_group(&A, &B, &dW, &dbias, &M, &N1, &N2, &lda, &ldb, 1, workspace, workspace_bytes, accumulate, stream);
}

// Large-M NT GEMM: dispatch and the bf16 instantiations of gemm_nt_ring_kernel (gemm_nt_ring_kernel.h); the fp16-operand forward
// flavours are instantiated in gemm_nt_ring16.hip (a second translation unit: the two compile side by side).
#include "gemm_nt_ring_kernel.h"

namespace {

// The compiled flavours are EpiBf16Ring (gemm_epilogue.h); anything else runs on the generic instantiation.
template <int BN>
int launch_ring(const GemmNtArgs& a, hipStream_t st) {
    return epi_dispatch(EpiBf16Ring{}, epi_flavour(a), [&](auto e) { return launch_ring_epi<BN, decltype(e)::value>(a, st); },
                        [&] { return launch_ring_epi<BN, EPI_GENERIC>(a, st); });
}

}  // namespace

// Top-k scan with the index rows as M (256-row tiles) and up to 128 queries as N.
int cldrd_gemm_nt_ring_scan(const GemmNtArgs& a, hipStream_t st) {
    return a.in_f16 ? launch_ring_epi<128, EPI_FILTER | EPI_F16IN>(a, st) : launch_ring_epi<128, EPI_FILTER>(a, st);
}

int cldrd_gemm_nt_ring16_launch(const GemmNtArgs& a, int bn, hipStream_t st);    // gemm_nt_ring16.hip

// Returns -1 if this variant does not apply (caller falls back to the 128x128 kernel), else the launch status.
int cldrd_gemm_nt_ring_dispatch(const GemmNtArgs& a_in, hipStream_t st) {
    GemmNtArgs a = a_in;
    if (a.K % BK != 0) return -1;
    if ((double)a.M * a.lda * 2.0 >= 4.0e9 || (double)a.N * a.ldb * 2.0 >= 4.0e9) return -1;   // 32-bit DMA offsets
    if (a.M < NT_RING_MIN_M) return -1;
    const long tiles_m = (a.M + BM - 1) / BM;
    const bool ok256 = a.N % 256 == 0, ok192 = a.N % 192 == 0;
    if (!ok256 && !ok192) return -1;
    int bn;
    if (ok256 && ok192) {
        // prefer the tile count that fills whole rounds of 256 CUs; tie -> the larger tile
        const long t256 = tiles_m * (a.N / 256), t192 = tiles_m * (a.N / 192);
        const double e256 = (double)t256 / (double)(((t256 + 255) / 256) * 256), e192 = (double)t192 / (double)(((t192 + 255) / 256) * 256);
        bn = (e192 > e256 + 0.15) ? 192 : 256;     // measured: N=768 -> 192, N=2304/3072 -> 256 (profiles/r01_gemm_bench.txt)
    } else {
        bn = ok256 ? 256 : 192;
    }
    // N-tile group: about 2 MB of B (bn rows x K) per group
    // (only for short K: with K >= 2048 the tiles of a round sweep K in step, L2 holds the current K slices of every panel, and a
    // group pass would re-read the A panels - PMC: 436 MB instead of 293 MB for N = 768, K = 2304 / 3072)
    a.gn = a.K <= 1024 ? (int)(2.0e6 / ((double)bn * a.K * 2.0) + 0.5) : 0;
    if (a.gn < 0) a.gn = 0;
    // (A persistent tile walk with a register epilogue - gemm_nt_pers.hip of rounds 2-3 - measured equal to this kernel within 1 % on
    // the encoder shapes and in the training step, profiles/r02_microbench.txt, and was removed in round 4.)
    if (a.in_f16) return cldrd_gemm_nt_ring16_launch(a, bn, st);       // fp16 operands: the forward FFN flavours, or -1
    return bn == 256 ? launch_ring<256>(a, st) : launch_ring<192>(a, st);
}

// Softmax cross-entropy (InfoNCE) of a row's positives against its negatives, with a temperature: value + analytic gradient in ONE launch,
// fp32.  The reference has no such loss (its trainers are pairwise / listwise rank losses only); this is THIS package's definition, the loss
// every dense-retrieval trainer pairs with in-batch negatives and with cosine scoring (README: Contrastive training).
//
// Per row b of logits [B, Np], classes decided from labels [B, Np] alone:
//   positive  label >= pos_min when a pos_min is given, else label == the row's maximum label (an exact tie: several positives);
//   negative  label <= neg_max and not positive;
//   neutral   everything else: in neither sum, gradient 0 (the lower-ranked relT passages are probably relevant: using them as negatives is
//             the false-negative problem).
// Duplicate rule, only with pids [B, N] (the passage id behind column c is pids[passage(mode, b, c)], the column layout of score_fwd): a
// negative column whose pid equals the pid of a positive or neutral column of the same row becomes neutral.
// With z = logits / tau, P / G the positive / negative sets, Z = sum_{j in G} exp(z_j):
//   L_b  = (1/|P|) sum_{i in P} [ log(exp(z_i) + Z) - z_i ]
//   loss = mean of L_b over the valid rows (|P| >= 1 and |G| >= 1), or their sum;  no valid row: 0
//   d loss / d logits[b,i], i in P:  w (exp(z_i) / (exp(z_i) + Z) - 1)        w = 1 / (tau |P| R), R = valid rows (mean) or 1 (sum)
//   d loss / d logits[b,j], j in G:  w exp(z_j) sum_{i in P} 1 / (exp(z_i) + Z)
//   neutral columns and invalid rows: 0.
// Everything is evaluated after subtracting the row's maximum z over P u G.
#include "common.h"
#include "score_layout.h"

namespace {

enum { CE_NEUTRAL = 0, CE_POS = 1, CE_NEG = 2 };

// LDS bytes of one row: z [Np] floats, the columns kept out of the negatives by their label [Np] uint16, the class [Np] bytes
__host__ __device__ constexpr size_t softmax_ce_lds_bytes(int Np) { return (size_t)7 * Np + 16; }

__device__ unsigned int softmax_ce_tickets[ARRIVAL_SLOTS];      // arrival counters of softmax_ce_kernel launches (common.h: arrived_last)

// One workgroup per row.  A row's sums are block reductions in a fixed order; the one cross-row quantity, {sum of L_b, R}, is added in a
// fixed order by the workgroup that arrives last (common.h: arrived_last):
// no float atomics, the same bits on every launch.  Every workgroup writes its row's gradient for R = 1; under the 'mean' reduction the
// last workgroup then multiplies the whole gradient by 1 / R (R is not known before every row's duplicate rule has run).
__global__ __launch_bounds__(256) void softmax_ce_kernel(const float* __restrict__ logits, const float* __restrict__ labels,
                                                          const long long* __restrict__ pids, float* grad, float* row_out,
                                                          float* __restrict__ loss_out, int B, int Np, int N, int mode, float tau,
                                                          float pos_min, int has_pos_min, float neg_max, int mean_reduction, int slot) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    __shared__ float red[4];
    __shared__ int n_keep;                           // number of kept columns
    float* z = sm;                                                   // [Np]
    unsigned short* keep = (unsigned short*)(z + Np);                // [Np] columns that are positive or neutral by their label
    unsigned char* cls = (unsigned char*)(keep + Np);                // [Np]
    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const float NINF = -__builtin_inff();
    const float* lab = labels + (size_t)b * Np;
    const float* lg = logits + (size_t)b * Np;
    float* g = grad + (size_t)b * Np;

    // ---- classes from the labels
    float lmax = NINF;
    if (!has_pos_min) {
        for (int i = tid; i < Np; i += blockDim.x) lmax = fmaxf(lmax, lab[i]);
        lmax = block_max(lmax, red);
    }
    if (tid == 0) n_keep = 0;
    __syncthreads();
    for (int i = tid; i < Np; i += blockDim.x) {
        const float l = lab[i];
        const bool pos = has_pos_min ? l >= pos_min : l == lmax;
        const int c = pos ? CE_POS : (l <= neg_max ? CE_NEG : CE_NEUTRAL);
        cls[i] = (unsigned char)c;
        z[i] = lg[i] / tau;
        if (pids && c != CE_NEG) keep[atomicAdd(&n_keep, 1)] = (unsigned short)i;      // the order of the list decides nothing
    }
    __syncthreads();
    // ---- duplicate rule: a negative whose passage is also behind a positive or neutral column of this row leaves the negatives
    if (pids) {
        const int nk = n_keep;
        for (int i = tid; i < Np; i += blockDim.x) {
            if (cls[i] != CE_NEG) continue;
            const long long p = pids[col_to_passage(mode, b, i, B, N)];
            bool dup = false;
            for (int k = 0; k < nk && !dup; ++k) dup = pids[col_to_passage(mode, b, keep[k], B, N)] == p;
            if (dup) cls[i] = CE_NEUTRAL;            // keep[] lists label classes only: no thread reads another thread's cls here
        }
        __syncthreads();
    }
    // ---- the row's maximum over P u G, |P|, |G|
    float m = NINF, np = 0.f, ng = 0.f;
    for (int i = tid; i < Np; i += blockDim.x) {
        const int c = cls[i];
        if (c == CE_NEUTRAL) continue;
        m = fmaxf(m, z[i]);
        if (c == CE_POS) np += 1.f; else ng += 1.f;
    }
    m = block_max(m, red);
    np = block_sum(np, red);                         // whole numbers <= 8192: exact
    ng = block_sum(ng, red);
    const bool valid = np >= 1.f && ng >= 1.f;
    float row_loss = 0.f;
    if (valid) {                                     // (block-uniform)
        float zp = 0.f;
        for (int i = tid; i < Np; i += blockDim.x)
            if (cls[i] == CE_NEG) zp += expf(z[i] - m);
        const float Z = block_sum(zp, red);
        float lp = 0.f, sp = 0.f;
        for (int i = tid; i < Np; i += blockDim.x) {
            if (cls[i] != CE_POS) continue;
            const float zi = z[i] - m, e = expf(zi), D = e + Z;
            lp += e >= Z ? log1pf(Z / e) : logf(D) - zi;         // log(e + Z) - zi; the first form keeps a small Z beside e = 1
            sp += 1.f / D;
        }
        const float l = block_sum(lp, red);
        const float S = block_sum(sp, red);
        const float w = 1.0f / (tau * np);
        for (int i = tid; i < Np; i += blockDim.x) {
            const int c = cls[i];
            float v = 0.f;
            if (c == CE_POS) {
                const float e = expf(z[i] - m);
                v = -w * (Z / (e + Z));              // e / (e + Z) - 1 without the cancellation
            } else if (c == CE_NEG) {
                v = w * expf(z[i] - m) * S;
            }
            g[i] = v;
        }
        row_loss = l / np;
    } else {
        for (int i = tid; i < Np; i += blockDim.x) g[i] = 0.f;
    }
    // ---- publish the row; the workgroup that arrives last finishes the call
    if (tid == 0) { row_out[2 * b] = row_loss; row_out[2 * b + 1] = valid ? 1.f : 0.f; }
    if (!arrived_last(softmax_ce_tickets + slot, B)) return;
    float ls = 0.f, rs = 0.f;
    for (int r = tid; r < B; r += blockDim.x) {      // thread t adds rows t, t + 256, ... in ascending order, then the block sum: a fixed order
        ls += __hip_atomic_load(row_out + 2 * r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        rs += __hip_atomic_load(row_out + 2 * r + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const float L = block_sum(ls, red);
    const float R = block_sum(rs, red);
    if (tid == 0) {
        loss_out[0] = mean_reduction ? (R > 0.f ? L / R : 0.f) : L;
        loss_out[1] = R;
    }
    if (mean_reduction && R > 1.f) {
        const float inv = 1.0f / R;
        const size_t n = (size_t)B * Np;
        for (size_t i = tid; i < n; i += blockDim.x)
            grad[i] = __hip_atomic_load(grad + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) * inv;
    }
}

}  // namespace

// include/cldrd_hip.h.  One launch, one workgroup per row; takes the place of cldrd_loss_fwd_bwd / cldrd_lambda_term on the loss stream.
extern "C" int cldrd_softmax_ce(const float* logits, const float* labels, int B, int Np, const long long* pids, int N, int mode, float tau,
                                float pos_min, int has_pos_min, float neg_max, int mean_reduction, float* loss_out, float* grad,
                                float* workspace, void* stream) {
    CLDRD_CHECK(logits && labels && loss_out && grad && workspace, "softmax_ce: null pointer");
    CLDRD_CHECK(B > 0, "softmax_ce: need B > 0");
    CLDRD_CHECK(Np >= 1 && Np <= 8192, "softmax_ce: need 1 <= Np <= 8192");
    CLDRD_CHECK(tau > 0.f && tau <= 3.0e38f, "softmax_ce: the temperature tau must be finite and > 0");
    CLDRD_CHECK(mode >= 0 && mode <= 2, "softmax_ce: mode must be 0, 1 or 2");
    CLDRD_CHECK((has_pos_min == 0 || has_pos_min == 1) && (mean_reduction == 0 || mean_reduction == 1),
                "softmax_ce: has_pos_min and mean_reduction must be 0 or 1");
    CLDRD_CHECK(neg_max == neg_max, "softmax_ce: neg_max is NaN");
    CLDRD_CHECK(!has_pos_min || pos_min > neg_max, "softmax_ce: need pos_min > neg_max");
    if (pids) {
        CLDRD_CHECK(N >= 1 && (long long)B * N <= 0x7fffffffLL, "softmax_ce: pids need N >= 1");
        CLDRD_CHECK(Np == score_cols(B, N, mode), "softmax_ce: Np does not match mode, B and N (mode 0: N, 1: B * N, 2: 2 * N)");
    }
    static std::atomic<unsigned int> launches{0};
    const int slot = arrival_next_slot(launches);
    hipLaunchKernelGGL(softmax_ce_kernel, dim3(B), dim3(256), softmax_ce_lds_bytes(Np), (hipStream_t)stream, logits, labels, pids, grad,
                       workspace, loss_out, B, Np, N, mode, tau, pos_min, has_pos_min, neg_max, mean_reduction, slot);
    CLDRD_LAUNCH_CHECK();
    return 0;
}

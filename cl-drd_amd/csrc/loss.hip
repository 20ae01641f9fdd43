// The list-wise distillation losses, forward + analytic backward, fp32 (the scorers in front of them: score.hip).
//
// Reference: losses/kl_div.py:11-22, losses/margin_mse.py:8-19, losses/ranknet.py:3-44, losses/lambda_rank.py:3-96
// (SURVEY.md K6-K10).  The reference materialises three [B,N,N] tensors, sorts, and synchronises with the
// host twice per call (ranknet.py:16,40); here one workgroup owns one row: ranks come from an in-LDS count
// (stable: ties by index), the pair loop runs over LDS, loss and pair count are wave-reduced, and the
// gradient is written directly (no autograd graph, no host sync).
#include "common.h"

namespace {

enum { LOSS_KL = 0, LOSS_MSE = 1, LOSS_RANKNET = 2, LOSS_LAMBDA = 3, LOSS_WPOINT = 4 };

__device__ __forceinline__ float NEG_INF_F() { return -__builtin_inff(); }

// One block per row.  Writes the un-normalised gradient and the row's {loss sum, pair count}.
__global__ __launch_bounds__(256) void loss_row_kernel(int kind, const float* __restrict__ y_pred, const float* __restrict__ y_true,
                                                        const float* __restrict__ bweight, float* __restrict__ grad,
                                                        float* __restrict__ row_out, int B, int N, float T, float pad) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    float* s = sm;            // [N]
    float* t = s + N;         // [N]
    float* rk = t + N;        // [N] 1/rank
    __shared__ float red[4];
    const int b = blockIdx.x;
    for (int i = threadIdx.x; i < N; i += blockDim.x) { s[i] = y_pred[(size_t)b * N + i]; t[i] = y_true[(size_t)b * N + i]; }
    __syncthreads();
    float lsum = 0.f, cnt = 0.f;
    if (kind == LOSS_KL) {
        const float iT = 1.0f / T;
        float ms = NEG_INF_F(), mt = ms;
        for (int i = threadIdx.x; i < N; i += blockDim.x) { ms = fmaxf(ms, s[i] * iT); mt = fmaxf(mt, t[i] * iT); }
        ms = block_max(ms, red); mt = block_max(mt, red);
        float es = 0.f, et = 0.f;
        for (int i = threadIdx.x; i < N; i += blockDim.x) { es += __expf(s[i] * iT - ms); et += __expf(t[i] * iT - mt); }
        es = block_sum(es, red); et = block_sum(et, red);
        const float lzs = ms + __logf(es), lzt = mt + __logf(et);
        for (int i = threadIdx.x; i < N; i += blockDim.x) {
            const float ls = s[i] * iT - lzs, lt = t[i] * iT - lzt;
            const float pt = __expf(lt);
            lsum += pt * (lt - ls);
            grad[(size_t)b * N + i] = (__expf(ls) - pt) * iT / (float)B;
        }
        cnt = 0.f;
    } else if (kind == LOSS_MSE) {
        float sd = 0.f;
        for (int i = threadIdx.x; i < N; i += blockDim.x) sd += s[i] - t[i];
        sd = block_sum(sd, red);
        const float mean = sd / (float)N;
        const float k = 4.0f / ((float)B * (float)N);     // 4/(B N^2) * N
        for (int i = threadIdx.x; i < N; i += blockDim.x) {
            const float dc = (s[i] - t[i]) - mean;
            lsum += dc * dc;
            grad[(size_t)b * N + i] = k * dc;
        }
        lsum *= 2.0f / ((float)B * (float)N);              // 2/(B N^2) * N * sum (d - mean)^2
    } else if (kind == LOSS_WPOINT) {
        // weighted_pointwise_loss (reference losses/weighted_pointwise.py:3-14): mean over B*N of softplus(-y/T) * weight
        const float iT = 1.0f / T, k = 1.0f / ((float)B * (float)N);
        for (int i = threadIdx.x; i < N; i += blockDim.x) {
            const float z = -s[i] * iT, w = t[i];
            const float e = __expf(-fabsf(z));
            lsum += (log1pf(e) + fmaxf(z, 0.f)) * w;
            grad[(size_t)b * N + i] = -(z > 0.f ? 1.f / (1.f + e) : e / (1.f + e)) * iT * w * k;      // -sigmoid(z)/T * w / (B N)
        }
        lsum *= k;
    } else {
        const bool by_rank = (kind == LOSS_LAMBDA);
        if (by_rank) {
            for (int i = threadIdx.x; i < N; i += blockDim.x) {
                const bool pi = t[i] == pad;
                const float ki = pi ? NEG_INF_F() : s[i];
                int r = 1;
                for (int j = 0; j < N; ++j) {
                    const float kj = (t[j] == pad) ? NEG_INF_F() : s[j];
                    r += (kj > ki) || (kj == ki && j < i);
                }
                rk[i] = 1.0f / (float)r;
            }
            __syncthreads();
        }
        const float bw = bweight ? bweight[b] : 1.0f;
        for (int i = threadIdx.x; i < N; i += blockDim.x) {
            const float si = s[i], ti = t[i];
            float gi = 0.f;
            if (ti != pad) {
                for (int j = 0; j < N; ++j) {
                    const float tj = t[j];
                    if (tj == pad || tj == ti) continue;
                    const float w = (by_rank ? fabsf(rk[i] - rk[j]) : 1.0f) * bw;
                    if (ti > tj) {            // pair (i, j)
                        const float df = fminf(fmaxf(si - s[j], -1e8f), 1e8f);
                        const float e = __expf(-fabsf(df));
                        lsum += w * (log1pf(e) + fmaxf(-df, 0.f));
                        cnt += 1.f;
                        gi -= w * (df > 0.f ? e / (1.f + e) : 1.f / (1.f + e));      // sigma(-df)
                    } else {                  // pair (j, i)
                        const float df = fminf(fmaxf(s[j] - si, -1e8f), 1e8f);
                        const float e = __expf(-fabsf(df));
                        gi += w * (df > 0.f ? e / (1.f + e) : 1.f / (1.f + e));
                    }
                }
            }
            grad[(size_t)b * N + i] = gi;
        }
    }
    lsum = block_sum(lsum, red);
    cnt = block_sum(cnt, red);
    if (threadIdx.x == 0) { row_out[2 * b] = lsum; row_out[2 * b + 1] = cnt; }
}

// loss_out[0] = loss, loss_out[1] = pair count; scales grad for the 'mean' reduction of the pairwise losses.
__global__ __launch_bounds__(256) void loss_finalize_kernel(int kind, const float* __restrict__ row_out, float* __restrict__ grad,
                                                             float* __restrict__ loss_out, int B, int N, int mean_reduction) {
    __shared__ float tot[2];
    if (threadIdx.x == 0) {
        float l = 0.f, c = 0.f;
        for (int b = 0; b < B; ++b) { l += row_out[2 * b]; c += row_out[2 * b + 1]; }
        tot[0] = l; tot[1] = c;
    }
    __syncthreads();
    const float l = tot[0], c = tot[1];
    if (kind == LOSS_KL) {
        if (threadIdx.x == 0) { loss_out[0] = l / (float)B; loss_out[1] = 0.f; }
        return;
    }
    if (kind == LOSS_MSE || kind == LOSS_WPOINT) {
        if (threadIdx.x == 0) { loss_out[0] = l; loss_out[1] = 0.f; }
        return;
    }
    if (mean_reduction) {
        const float inv = 1.0f / c;           // c == 0 -> inf/nan, as torch.mean of an empty selection
        if (threadIdx.x == 0) { loss_out[0] = c > 0.f ? l * inv : __int_as_float(0x7fc00000); loss_out[1] = c; }
        for (int i = threadIdx.x; i < B * N; i += blockDim.x) grad[i] = c > 0.f ? grad[i] * inv : __int_as_float(0x7fc00000);
    } else if (threadIdx.x == 0) {
        loss_out[0] = l; loss_out[1] = c;
    }
}

// LambdaLoss framework (reference losses/standard_lambda_rank.py:3-117, allRank's lambda_loss): one block per slate.
// Everything lives in "sorted by prediction" positions p = 0..N-1 (padded items sort last: their keys are -inf):
//   pair (p, q) counts iff both are real items, p < k and q < k, and (except ndcgLoss1) true[p] > true[q];
//   term = -log( clamp( clamp(sigmoid(sigma (s_p - s_q)), eps) ^ W_pq, eps) ), natural or base-2 log;
//   W per weighing scheme from gains G = (2^true - 1 | true - 1) / maxDCG@k and discounts D_p = log2(2 + p).
// The gradient flows through the score difference only (sort indices and weights are constants for autograd); clamp passes
// the gradient where its input is >= the bound, as torch.clamp does.
enum { LL_NONE = 0, LL_NDCG1 = 1, LL_NDCG2 = 2, LL_LAMBDARANK = 3, LL_NDCG2PP = 4, LL_RANKNET = 5, LL_GTDIFF = 6, LL_GTDIFF_POW = 7 };

struct LambdaParams { int scheme, k; float eps, sigma, mu; int log2_red, gain_linear; };      // k: already min'ed against "no truncation"

// LDS floats of one slate of N items: the labels (lambda_stage_labels) and the five arrays of lambda_row_body.
__host__ __device__ constexpr size_t lambda_lds_floats(int N) { return (size_t)6 * N; }

// lab[0..N) <- the slate's labels, -inf where the label equals the padding indicator (judged on the label as given); then, on the
// labels that are not padding: flags bit 0: columns n_rel..N-1 become their mean (left-to-right fp32 sum, one division); bit 1: the
// row's minimum is subtracted; `offset` is added last.  flags == 0 and offset == 0 leave the labels as given.  Ends with a barrier.
__device__ __forceinline__ void lambda_stage_labels(const float* __restrict__ yt, float* lab, float* red, int N, float pad, int flags,
                                                    int n_rel, float offset) {
    const float NINF = NEG_INF_F();
    for (int i = threadIdx.x; i < N; i += blockDim.x) lab[i] = yt[i] == pad ? NINF : yt[i];
    __syncthreads();
    if (flags & 1) {
        if (threadIdx.x == 0) {
            float s = 0.f;
            int n = 0;
            for (int i = n_rel; i < N; ++i)
                if (lab[i] != NINF) { s += lab[i]; ++n; }
            red[0] = n > 0 ? s / (float)n : 0.f;
        }
        __syncthreads();
        const float m = red[0];
        for (int i = n_rel + threadIdx.x; i < N; i += blockDim.x)
            if (lab[i] != NINF) lab[i] = m;
        __syncthreads();
    }
    if (flags & 2) {
        float v = NINF;                                         // max of the negated labels = -(row minimum); padding never wins
        for (int i = threadIdx.x; i < N; i += blockDim.x)
            if (lab[i] != NINF) v = fmaxf(v, -lab[i]);
        const float mn = -block_max(v, red);
        for (int i = threadIdx.x; i < N; i += blockDim.x)
            if (lab[i] != NINF) lab[i] -= mn;
        __syncthreads();
    }
    if (offset != 0.f) {
        for (int i = threadIdx.x; i < N; i += blockDim.x)
            if (lab[i] != NINF) lab[i] += offset;
        __syncthreads();
    }
}

// Number of pairs lambda_row_body counts for this slate, without their terms (the 'mean' reduction of the term kernel divides by
// the count of ALL rows, which every workgroup takes this way before it writes a gradient).  top: [N] ints of LDS scratch.
__device__ __forceinline__ float lambda_row_pairs(const float* __restrict__ yp, const float* lab, int* top, float* red, int N,
                                                  int scheme, int k) {
    const float NINF = NEG_INF_F();
    const int kk = k < N ? k : N;
    for (int i = threadIdx.x; i < N; i += blockDim.x) {
        int in = lab[i] != NINF;
        if (in && kk < N) {                                     // position of item i in the stable descending order of the predictions
            const float si = yp[i];
            int pos_s = 0;
            for (int j = 0; j < N; ++j) {
                const float sj = lab[j] == NINF ? NINF : yp[j];
                pos_s += (sj > si) || (sj == si && j < i);
            }
            in = pos_s < kk;
        }
        top[i] = in;
    }
    __syncthreads();
    float c = 0.f;
    for (int i = threadIdx.x; i < N; i += blockDim.x) {
        if (!top[i]) continue;
        for (int j = 0; j < N; ++j) c += (top[j] && (scheme == LL_NDCG1 || lab[i] > lab[j])) ? 1.f : 0.f;
    }
    return block_sum(c, red);                                   // whole numbers <= N^2 <= 2^24: exact in fp32, whatever the order
}

// One slate: yp its N predictions (global), lab its N labels (LDS, -inf = padding), sm 5 * N floats of LDS.  On return (all threads,
// behind a barrier) gp[p] = d sum-of-terms / d prediction of the item at sorted position p, item[p] = that item's column, and
// lsum / cnt = the slate's sum of terms / number of pairs in every thread.
__device__ __forceinline__ void lambda_row_body(const float* __restrict__ yp, const float* lab, float* sm, float* red, int N,
                                                const LambdaParams& P, float& lsum_out, float& cnt_out) {
    float* ps = sm;                  // [N] prediction at sorted position (padded: -inf)
    float* ts = ps + N;              // [N] label at sorted position (padded: -inf)
    float* G = ts + N;               // [N] gain at sorted position
    float* gp = G + N;               // [N] gradient at sorted position
    int* item = (int*)(gp + N);      // [N] original column at sorted position
    const int scheme = P.scheme, k = P.k, log2_red = P.log2_red, gain_linear = P.gain_linear;
    const float eps = P.eps, sigma = P.sigma, mu = P.mu;
    const float NINF = NEG_INF_F();
    // ---- positions: stable descending order of the (masked) predictions; maxDCG from the descending labels
    float dcg = 0.f;
    for (int i = threadIdx.x; i < N; i += blockDim.x) {
        const bool padded = lab[i] == NINF;
        const float si = padded ? NINF : yp[i], ti = lab[i];
        int pos_s = 0, pos_t = 0;
        for (int j = 0; j < N; ++j) {
            const float tj = lab[j];
            const float sj = tj == NINF ? NINF : yp[j];
            pos_s += (sj > si) || (sj == si && j < i);
            pos_t += (tj > ti) || (tj == ti && j < i);
        }
        ps[pos_s] = si; ts[pos_s] = ti; item[pos_s] = i;
        if (pos_t < k) {
            const float tc = fmaxf(ti, 0.f);
            dcg += (gain_linear ? tc - 1.f : exp2f(tc) - 1.f) / log2f(2.f + (float)pos_t);
        }
    }
    const float maxdcg = fmaxf(block_sum(dcg, red), eps);      // block_sum synchronises: ps / ts / item are complete after it
    for (int p = threadIdx.x; p < N; p += blockDim.x) {
        const float tc = fmaxf(ts[p], 0.f);
        G[p] = (gain_linear ? tc - 1.f : exp2f(tc) - 1.f) / maxdcg;
    }
    __syncthreads();
    const float logk = log2_red ? 1.4426950408889634f : 1.0f;
    auto weight = [&](int p, int q) -> float {
        const float Dp = log2f(2.f + (float)p), Dq = log2f(2.f + (float)q);
        float lr = 0.f, n2 = 0.f;
        if (scheme == LL_LAMBDARANK || scheme == LL_NDCG2PP) lr = fabsf(1.f / Dp - 1.f / Dq) * fabsf(G[p] - G[q]);
        if (scheme == LL_NDCG2 || scheme == LL_NDCG2PP) {
            const int dl = p > q ? p - q : q - p;
            n2 = dl == 0 ? 0.f : fabsf(1.f / log2f(1.f + (float)dl) - 1.f / log2f(2.f + (float)dl)) * fabsf(G[p] - G[q]);
        }
        switch (scheme) {
            case LL_NDCG1: return G[p] / Dp;
            case LL_NDCG2: return n2;
            case LL_LAMBDARANK: return lr;
            case LL_NDCG2PP: return mu * n2 + lr;
            case LL_GTDIFF: return fabsf(fmaxf(ts[p], 0.f) - fmaxf(ts[q], 0.f));
            case LL_GTDIFF_POW: { const float a = fmaxf(ts[p], 0.f), c = fmaxf(ts[q], 0.f); return fabsf(a * a - c * c); }
            default: return 1.f;
        }
    };
    // term(p, q) and d term / d (s_p - s_q)
    auto term = [&](int p, int q, float& dterm) -> float {
        const float W = weight(p, q);
        const float d = fminf(fmaxf(ps[p] - ps[q], -1e8f), 1e8f);
        const float u = 1.f / (1.f + __expf(-sigma * d));
        const float a = fmaxf(u, eps);
        const float bw = powf(a, W);
        const float c = fmaxf(bw, eps);
        // d(-log c)/dd = -(1/c) [bw >= eps] W a^(W-1) [u >= eps] sigma u (1-u), and the clamp of d passes inside (-1e8, 1e8)
        const bool live = bw >= eps && u >= eps && fabsf(ps[p] - ps[q]) <= 1e8f;
        dterm = live ? -logk * (W * bw / a) / c * sigma * u * (1.f - u) : 0.f;
        return -logk * __logf(c);
    };
    const int kk = k < N ? k : N;
    float lsum = 0.f, cnt = 0.f;
    for (int p = threadIdx.x; p < N; p += blockDim.x) {
        float g = 0.f;
        if (p < kk && ts[p] != NINF) {
            for (int q = 0; q < kk; ++q) {
                if (q == p && scheme != LL_NDCG1) continue;
                if (ts[q] == NINF) continue;
                const float td = ts[p] - ts[q];
                float dt;
                if (scheme == LL_NDCG1 || td > 0.f) {          // pair (p, q): p is the first index
                    lsum += term(p, q, dt);
                    cnt += 1.f;
                    if (q != p) g += dt;                       // (p, p) only exists for ndcgLoss1: s_p - s_p has no gradient
                }
                if (q != p && (scheme == LL_NDCG1 || td < 0.f)) {          // pair (q, p): p is the second index
                    (void)term(q, p, dt);
                    g -= dt;
                }
            }
        }
        gp[p] = g;
    }
    __syncthreads();
    lsum_out = block_sum(lsum, red);
    cnt_out = block_sum(cnt, red);
}

__global__ __launch_bounds__(256) void lambda_loss_row_kernel(const float* __restrict__ y_pred, const float* __restrict__ y_true,
                                                               float* __restrict__ grad, float* __restrict__ row_out, int N,
                                                               LambdaParams P, float pad) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    __shared__ float red[4];
    const int b = blockIdx.x;
    float* lab = sm;
    lambda_stage_labels(y_true + (size_t)b * N, lab, red, N, pad, 0, N, 0.f);
    float lsum, cnt;
    lambda_row_body(y_pred + (size_t)b * N, lab, sm + N, red, N, P, lsum, cnt);
    const float* gp = sm + 4 * N;
    const int* item = (const int*)(sm + 5 * N);
    for (int p = threadIdx.x; p < N; p += blockDim.x) grad[(size_t)b * N + item[p]] = gp[p];
    if (threadIdx.x == 0) { row_out[2 * b] = lsum; row_out[2 * b + 1] = cnt; }
}

__device__ unsigned int lambda_term_tickets[ARRIVAL_SLOTS];      // arrival counters of lambda_term_kernel launches (common.h: arrived_last)

// The term form of lambda_loss (cldrd_lambda_term): one workgroup per slate = the first Ns columns of a row of logits [B, Np].
//   term = lambda_loss(logits[:, :Ns], labels'), labels' = the staged labels (lambda_stage_labels);
//   grad[b, :Ns] (+)= alpha * d term / d logits, loss_out[0] (+)= alpha * term, *term_out = term.
// Under the 'mean' reduction every gradient entry is divided by the pair count of ALL rows; each workgroup takes that count itself
// (lambda_row_pairs over every row: compares only, cheap next to its own row's pair loop of exp / pow / log), so it writes its
// final gradient in one pass and the accumulate form needs no second buffer.  The value is the one cross-row sum: every workgroup
// publishes {sum of terms, pairs} to row_out, and thread 0 of the workgroup that arrives last (common.h: arrived_last) adds the rows in
// ascending order, with loads that bypass its L1.  Fixed order, no float atomics: the same bits on every launch, and the bits of
// lambda_loss_row_kernel + loss_finalize_kernel where the two forms compute the same thing.
__global__ __launch_bounds__(256) void lambda_term_kernel(const float* __restrict__ logits, const float* __restrict__ labels,
                                                           float* __restrict__ grad, float* row_out, float* __restrict__ loss_out,
                                                           float* __restrict__ term_out, int B, int Np, int Ns, LambdaParams P, float pad,
                                                           int mean_reduction, int label_flags, int n_rel, float label_offset, float alpha,
                                                           int accumulate, int slot) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    __shared__ float red[4];
    const int b = blockIdx.x;
    const float QNAN = __int_as_float(0x7fc00000);
    float* lab = sm;
    float c = 0.f;
    if (mean_reduction) {
        for (int r = 0; r < B; ++r) {
            lambda_stage_labels(labels + (size_t)r * Ns, lab, red, Ns, pad, label_flags, n_rel, label_offset);
            c += lambda_row_pairs(logits + (size_t)r * Np, lab, (int*)(sm + Ns), red, Ns, P.scheme, P.k);
            __syncthreads();                                    // lab / top are rewritten for the next row
        }
    }
    const float inv = 1.0f / c;
    lambda_stage_labels(labels + (size_t)b * Ns, lab, red, Ns, pad, label_flags, n_rel, label_offset);
    float lsum, cnt;
    lambda_row_body(logits + (size_t)b * Np, lab, sm + Ns, red, Ns, P, lsum, cnt);
    const float* gp = sm + 4 * Ns;
    const int* item = (const int*)(sm + 5 * Ns);
    float* g = grad + (size_t)b * Np;
    for (int p = threadIdx.x; p < Ns; p += blockDim.x) {
        float v = gp[p];
        if (mean_reduction) v = c > 0.f ? v * inv : QNAN;       // c == 0: the mean of an empty selection, as loss_finalize_kernel
        if (!accumulate) g[item[p]] = alpha * v;
        else if (alpha != 0.f) g[item[p]] += alpha * v;         // alpha == 0 leaves grad bit for bit (x + 0 would turn a -0 into +0)
    }
    if (!accumulate)
        for (int j = Ns + threadIdx.x; j < Np; j += blockDim.x) g[j] = 0.f;
    if (threadIdx.x == 0) { row_out[2 * b] = lsum; row_out[2 * b + 1] = cnt; }
    if (!arrived_last(lambda_term_tickets + slot, B) || threadIdx.x != 0) return;
    float l = 0.f, n = 0.f;
    for (int r = 0; r < B; ++r) {
        l += __hip_atomic_load(row_out + 2 * r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        n += __hip_atomic_load(row_out + 2 * r + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    float term = l;
    if (mean_reduction) term = n > 0.f ? l * (1.0f / n) : QNAN;
    if (!accumulate) { loss_out[0] = alpha * term; loss_out[1] = n; }
    else if (alpha != 0.f) loss_out[0] += alpha * term;
    if (term_out) *term_out = term;
}

// Logit-norm regulariser of the multistep-curriculum trainers (reference nway_listwise_1.py:348-350):
//   reg = lambda * ||logits||_2 over the whole [B, N] matrix;  loss_out[0] += reg;  grad += lambda * logits / ||logits||_2;
//   reg_out = reg (the trainer logs it and its ratio to the loss).  One workgroup: B * N is a few hundred numbers.
__global__ __launch_bounds__(256) void logit_reg_kernel(const float* __restrict__ logits, int n, float lambda, float* __restrict__ loss_out,
                                                         float* __restrict__ grad, float* __restrict__ reg_out) {
    __shared__ float red[4];
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += blockDim.x) s += logits[i] * logits[i];
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    const float norm = sqrtf((red[0] + red[1]) + (red[2] + red[3]));
    const float inv = norm > 0.f ? lambda / norm : 0.f;      // d||x||/dx at 0: torch gives 0 (subgradient)
    for (int i = threadIdx.x; i < n; i += blockDim.x) grad[i] += inv * logits[i];
    if (threadIdx.x == 0) {
        loss_out[0] += lambda * norm;
        if (reg_out) *reg_out = lambda * norm;
    }
}

// Teacher-score distillation term behind cldrd_loss_fwd_bwd: kd = KLDiv(T) or MarginMSE of logits[:, :Nt] against teacher [B, Nt]
// (reference losses/kl_div.py:11-22, losses/margin_mse.py:8-19 on a [B, Nt] input); loss_out[0] += alpha * kd, grad[:, :Nt] += alpha * d kd,
// *term_out = kd.  Columns Nt..Np-1 of a row (the in-batch negatives: no teacher score) are neither read nor written.
// One workgroup, one WAVE per row (rows wave, wave + waves, ...): the C ABI gives this term no workspace for per-row partial sums, and
// B * Nt is a few hundred to a few thousand numbers.  A row's reductions are wave shuffles (no barrier inside the row loop); each wave adds
// its rows in ascending order, thread 0 adds the waves in ascending order: the same bits on every call, no float atomics.
__global__ __launch_bounds__(512) void distill_term_kernel(int kind, const float* __restrict__ logits, int B, int Np,
                                                           const float* __restrict__ teacher, int Nt, float alpha, float T,
                                                           float* __restrict__ loss_out, float* __restrict__ grad, float* __restrict__ term_out) {
    __shared__ float part[8];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, waves = blockDim.x >> 6;
    const bool add = alpha != 0.f;            // alpha == 0 leaves loss_out and grad bit for bit (x + 0 would turn a -0 into +0)
    float acc = 0.f;
    for (int b = wave; b < B; b += waves) {
        const float* s = logits + (size_t)b * Np;
        const float* t = teacher + (size_t)b * Nt;
        float* g = grad + (size_t)b * Np;
        float row = 0.f;
        if (kind == LOSS_KL) {
            const float iT = 1.0f / T;
            float ms = NEG_INF_F(), mt = ms;
            for (int i = lane; i < Nt; i += 64) { ms = fmaxf(ms, s[i] * iT); mt = fmaxf(mt, t[i] * iT); }
            ms = wave_max(ms); mt = wave_max(mt);
            float es = 0.f, et = 0.f;
            for (int i = lane; i < Nt; i += 64) { es += __expf(s[i] * iT - ms); et += __expf(t[i] * iT - mt); }
            es = wave_sum(es); et = wave_sum(et);
            const float lzs = ms + __logf(es), lzt = mt + __logf(et);
            const float k = alpha * iT / (float)B;
            for (int i = lane; i < Nt; i += 64) {
                const float ls = s[i] * iT - lzs, lt = t[i] * iT - lzt;
                const float pt = __expf(lt);
                row += pt * (lt - ls);
                if (add) g[i] += k * (__expf(ls) - pt);
            }
        } else {
            float sd = 0.f;
            for (int i = lane; i < Nt; i += 64) sd += s[i] - t[i];
            const float mean = wave_sum(sd) / (float)Nt;
            const float k = alpha * 4.0f / ((float)B * (float)Nt);
            for (int i = lane; i < Nt; i += 64) {
                const float dc = (s[i] - t[i]) - mean;
                row += dc * dc;
                if (add) g[i] += k * dc;
            }
        }
        acc += wave_sum(row);
    }
    if (lane == 0) part[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float kd = 0.f;
        for (int w = 0; w < waves; ++w) kd += part[w];
        kd *= kind == LOSS_KL ? 1.0f / (float)B : 2.0f / ((float)B * (float)Nt);      // batchmean | 2/(B Nt^2) * Nt * sum (d - mean)^2
        if (add) loss_out[0] += alpha * kd;
        if (term_out) *term_out = kd;
    }
}

}  // namespace

// kind: 0 KLDiv(T), 1 MarginMSE, 2 ranknet, 3 lambda_mrr (batch_weight != null -> bweight_lambda_mrr).
// loss_out: device float[2] = {loss, number of valid pairs}; grad: device [B, N] = d loss / d y_pred;
// workspace: device float[2*B].
extern "C" int cldrd_loss_fwd_bwd(int kind, const float* y_pred, const float* y_true, const float* batch_weight, float* loss_out,
                                  float* grad, float* workspace, int B, int N, float T, float pad_indicator, int mean_reduction,
                                  void* stream) {
    CLDRD_CHECK(kind >= 0 && kind <= 4, "loss: unknown kind");
    CLDRD_CHECK(B > 0 && N > 0 && N <= 8192, "loss: need 0 < N <= 8192");
    CLDRD_CHECK(T > 0.f, "loss: T must be positive");
    hipLaunchKernelGGL(loss_row_kernel, dim3(B), dim3(256), 3 * N * sizeof(float), (hipStream_t)stream, kind, y_pred, y_true,
                       batch_weight, grad, workspace, B, N, T, pad_indicator);
    CLDRD_LAUNCH_CHECK();
    hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, kind, (const float*)workspace, grad, loss_out, B, N,
                       mean_reduction);
    CLDRD_LAUNCH_CHECK();
    return 0;
}

// loss_out[0] += lambda * ||logits||_2, grad += its gradient, *reg_out = the added term (reference nway_listwise_1.py:348-350).
// Call after cldrd_loss_fwd_bwd on the same stream.
extern "C" int cldrd_logit_norm_reg(const float* logits, int n, float reg_lambda, float* loss_out, float* grad, float* reg_out,
                                    void* stream) {
    CLDRD_CHECK(n > 0 && reg_lambda >= 0.f, "logit_norm_reg: bad arguments");
    hipLaunchKernelGGL(logit_reg_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, logits, n, reg_lambda, loss_out, grad, reg_out);
    CLDRD_LAUNCH_CHECK();
    return 0;
}

// loss_out[0] += alpha * kd, grad[:, :Nt] += alpha * d kd / d logits[:, :Nt], *term_out = kd (unweighted; may be null), with
// kd = KLDiv(T) (kind 0) or MarginMSE (kind 1) of logits[:, :Nt] (row stride Np) against teacher [B, Nt].  Columns >= Nt are untouched.
// Call after cldrd_loss_fwd_bwd (and cldrd_logit_norm_reg) on the same stream; without a rank term the caller zeroes loss_out / grad first.
extern "C" int cldrd_distill_term(int kind, const float* logits, int B, int Np, const float* teacher, int Nt, float alpha, float T,
                                  float* loss_out, float* grad, float* term_out, void* stream) {
    CLDRD_CHECK(kind == LOSS_KL || kind == LOSS_MSE, "distill_term: kind must be 0 (KLDiv) or 1 (MarginMSE)");
    CLDRD_CHECK(B > 0 && Nt >= 1 && Nt <= Np, "distill_term: need B > 0 and 1 <= Nt <= Np");
    CLDRD_CHECK(alpha >= 0.f && T > 0.f, "distill_term: need alpha >= 0 and T > 0");
    CLDRD_CHECK(logits && teacher && loss_out && grad, "distill_term: null pointer");
    hipLaunchKernelGGL(distill_term_kernel, dim3(1), dim3(512), 0, (hipStream_t)stream, kind, logits, B, Np, teacher, Nt, alpha, T, loss_out,
                       grad, term_out);
    CLDRD_LAUNCH_CHECK();
    return 0;
}

// lambda_loss of reference losses/standard_lambda_rank.py:3-95.  scheme: 0 None, 1 ndcgLoss1, 2 ndcgLoss2, 3 lambdaRank,
// 4 ndcgLoss2PP, 5 rankNet, 6 rankNetWeightedByGTDiff, 7 rankNetWeightedByGTDiffPowed; k <= 0 = no truncation.
// loss_out[2] = {loss, number of pairs}; grad [B, N]; workspace 2*B floats.
extern "C" int cldrd_lambda_loss_fwd_bwd(const float* y_pred, const float* y_true, float* loss_out, float* grad, float* workspace,
                                         int B, int N, int scheme, int k, float eps, float sigma, float mu, float pad_indicator,
                                         int mean_reduction, int log2_reduction, int gain_linear, void* stream) {
    CLDRD_CHECK(B > 0 && N > 0 && N <= 4096, "lambda_loss: need 0 < N <= 4096");
    CLDRD_CHECK(scheme >= 0 && scheme <= 7, "lambda_loss: unknown weighing scheme");
    const LambdaParams P{scheme, k > 0 ? k : N, eps, sigma, mu, log2_reduction, gain_linear};
    hipLaunchKernelGGL(lambda_loss_row_kernel, dim3(B), dim3(256), lambda_lds_floats(N) * sizeof(float), (hipStream_t)stream, y_pred, y_true,
                       grad, workspace, N, P, pad_indicator);
    CLDRD_LAUNCH_CHECK();
    hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (int)LOSS_RANKNET, (const float*)workspace, grad,
                       loss_out, B, N, mean_reduction);
    CLDRD_LAUNCH_CHECK();
    return 0;
}

// The term form of cldrd_lambda_loss_fwd_bwd, one launch (include/cldrd_hip.h): the slate of row b is logits[b, :Ns], its labels
// labels[b, :] after the label transform; accumulate 0 writes loss_out / grad (columns >= Ns: zero), 1 adds to them.
extern "C" int cldrd_lambda_term(const float* logits, int B, int Np, const float* labels, int Ns, int label_flags, int n_rel,
                                 float label_offset, int scheme, int k, float eps, float sigma, float mu, float pad_indicator,
                                 int mean_reduction, int log2_reduction, int gain_linear, float alpha, int accumulate, float* loss_out,
                                 float* grad, float* term_out, float* workspace, void* stream) {
    CLDRD_CHECK(logits && labels && loss_out && grad && workspace, "lambda_term: null pointer");
    CLDRD_CHECK(B > 0 && Ns >= 1 && Ns <= Np, "lambda_term: need B > 0 and 1 <= Ns <= Np");
    CLDRD_CHECK(Ns <= 4096, "lambda_term: need Ns <= 4096");
    CLDRD_CHECK(scheme >= 0 && scheme <= 7, "lambda_term: unknown weighing scheme");
    CLDRD_CHECK(label_flags >= 0 && label_flags <= 3, "lambda_term: label_flags must be 0..3 (bit 0 mean, bit 1 row_min)");
    CLDRD_CHECK(n_rel >= 0 && n_rel <= Ns, "lambda_term: need 0 <= n_rel <= Ns");
    CLDRD_CHECK(alpha >= 0.f, "lambda_term: need alpha >= 0");
    CLDRD_CHECK(accumulate == 0 || accumulate == 1, "lambda_term: accumulate must be 0 or 1");
    static std::atomic<unsigned int> launches{0};
    const int slot = arrival_next_slot(launches);
    const LambdaParams P{scheme, k > 0 ? k : Ns, eps, sigma, mu, log2_reduction, gain_linear};
    hipLaunchKernelGGL(lambda_term_kernel, dim3(B), dim3(256), lambda_lds_floats(Ns) * sizeof(float), (hipStream_t)stream, logits, labels,
                       grad, workspace, loss_out, term_out, B, Np, Ns, P, pad_indicator, mean_reduction, label_flags, n_rel, label_offset,
                       alpha, accumulate, slot);
    CLDRD_LAUNCH_CHECK();
    return 0;
}

/* cldrd_hip.h - C ABI of libcldrd_hip.so: the MI355X (gfx950) kernels behind the CL-DRD hot path.
 *
 * The reference (HansiZeng/CL-DRD) is pure Python and has no FFI: its hot path bottoms out in PyTorch /
 * HuggingFace / faiss calls.  Each entry point below replaces one of those call sites; the Python host code in
 * cl-drd_amd/ (a mirror of the reference's models / losses / retriever modules) binds them with ctypes, and
 * INTEGRATION.md shows the stub a maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM) unless stated; the caller owns all memory;
 *   - bf16 tensors are passed as void* (raw bfloat16 bits), fp32 as float*, token ids / masks as int64;
 *   - matrices are row-major; `ld*` are row strides in ELEMENTS;
 *   - `stream` is a hipStream_t (NULL = default stream); all calls are asynchronous and graph-capturable
 *     (no allocation, no host synchronisation inside);
 *   - return value 0 = launched; non-zero = rejected, cldrd_last_error() gives the reason (thread local).
 *     Nothing is computed on the CPU: without a gfx950 device the launches fail.
 *   - dropout: keep-mask = hash(seed, element index) (counter based); the backward entry points regenerate the
 *     mask from the same (p, seed), nothing is stored.  p = 0 disables it.
 */
#ifndef CLDRD_HIP_H
#define CLDRD_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

const char* cldrd_last_error(void);
int cldrd_version(void);
int cldrd_device_ok(void);            /* 1 if device 0 is a gfx950 */
/* The library reads NO environment variable.  The few kernel choices tests need to reach go through this call (process-wide):
 * key "gemm_splitk" (0 heuristic, 1 never split K, n > 1 n splits of the small-M Linear GEMM), "gemm_nt64" (1: the one-launch
 * 64 x 64 kernel for small-M GEMMs with K <= 1024 when gemm_splitk is 0, 0: never), "attn_fwd2" / "attn_bwd2" (1: persistent
 * attention kernels where they apply, 0: one item per workgroup).  Every choice computes the same function. */
int cldrd_set_tuning(const char* key, int value);

/* ---- encoder Linear layers -------------------------------------------------------------------------------
 * Replaces torch.nn.Linear inside the HF encoder (reference models/nway_dual_encoder.py:52,56,64 ->
 * transformers DistilBERT q_lin/k_lin/v_lin/out_lin/ffn.lin1/ffn.lin2, BERT query/key/value/dense).
 *   C[M,N] = epilogue(alpha * A[M,K] . B[N,K]^T)
 *   epilogue order: + bias[N] -> (store preact) -> act (bit 0 = erf-GELU) -> * gelu'(gelu_pre) -> dropout -> + residual
 *   act bit 1 = derivative form of the saved activation input: `preact` receives gelu'(pre-activation) instead of the
 *   pre-activation (forward, act = 3), and `gelu_pre` is taken to hold that derivative already (backward, act = 2: the epilogue
 *   multiplies by it and evaluates nothing) - what torch saves for GELU's backward is its input; saving the derivative moves the
 *   erf / exp out of the data-gradient GEMM's epilogue, which was VALU-bound.
 *   `preact` / `gelu_pre` are [M, ldc]: they have no leading dimension of their own and share C's row pitch; both and `bias` 16-byte aligned.
 *   K % 64 == 0; A/B/C 16-byte aligned; out_f32 != 0 stores fp32 instead of bf16; res_f32 != 0: `residual` is fp32
 *   (the fp32 residual stream: out-projection / FFN2 add the fp32 LayerNorm output and store the fp32 pre-LN sum, as the
 *   reference's autocast does - trainer/multistep-curriculum/nway_listwise_1.py:334).
 *   fmt (enum cldrd_fmt16 below): the 16-bit format of A, B, a 16-bit C and the GELU tape.  The entry points are named "16", not "bf16": both
 *   formats run at the same MFMA rate and fp16 is the DEFAULT arithmetic mode of the package (the reference's own, CLDRD_AMP in README.md). */
enum cldrd_fmt16 {
    CLDRD_FMT_BF16 = 0,          /* A, B, 16-bit C, preact / gelu_pre: bf16 (CLDRD_AMP=bf16: every operand of every pass) */
    CLDRD_FMT_F16 = 1,           /* A, B and a 16-bit C: fp16 (evaluation passes of the fp16 mode; no preact / gelu_pre) */
    CLDRD_FMT_F16_C_BF16 = 3,    /* fp16 A and B, bf16 C: the QKV projection of an evaluation pass whose attention kernels are bf16 */
    CLDRD_FMT_F16_TAPE = 5       /* fp16 everywhere incl. preact / gelu_pre: a training pass of the fp16 mode */
};
/* ln_* (all four or none): the fp32 residual given as a LayerNorm still to be applied: `residual` holds the pre-LN sum s (fp32, res_f32 = 1) and
 * the epilogue adds (s - ln_mean[m]) * ln_rstd[m] * ln_gamma[n] + ln_beta[n] - exactly what cldrd_layernorm_fwd would have written
 * as its fp32 output, which it then need not write (HF: hidden = LayerNorm(...); out = dense(x) + hidden).
 * workspace (optional): problems of fewer than 1024 rows whose one-pass grid would leave most CUs idle (CLS-only last layer, query
 * tower) are split along K: fp32 partials in `workspace` (cldrd_gemm_nt_splitk_workspace() bytes; 0 = this shape is not split), summed in
 * a fixed order and finished with the same epilogue by a second launch.  workspace = NULL: one pass.
 * fmt != CLDRD_FMT_BF16 also serves M >= 1024 (csrc/gemm_nt_ring16.hip). */
size_t cldrd_gemm_nt_splitk_workspace(int M, int N, int K);
int cldrd_gemm_nt16(const void* A, const void* B, void* C, int M, int N, int K, int lda, int ldb, int ldc,
                    const float* bias, const void* residual, int ldr, void* preact, const void* gelu_pre,
                    int act, float alpha, float dropout_p, unsigned long long seed, int out_f32, int res_f32, int fmt,
                    const float* ln_mean, const float* ln_rstd, const float* ln_gamma, const float* ln_beta,
                    float* workspace, size_t workspace_bytes, void* stream);

/* Weight gradient dW[N1,N2] (+)= A[M,N1]^T . B[M,N2]   (A = dY, B = layer input; autograd's Linear backward), and,
 * when dbias != NULL, the bias gradient dbias[N1] (+)= column sums of A in the same pass.
 * N1, N2 multiples of 128 (or N1 % 256 == 0 and N2 % 192 == 0); rows >= M are never read (no padding contract).
 * cldrd_wgrad_group: n such problems in ONE launch (the pointer / shape arrays are HOST arrays).  The weight gradients are off the
 * critical path of the backward, so the trainer defers them: with a tower's 20+ problems in one launch every workgroup sweeps all
 * tokens of its output tile and writes dW once - no token split, no fp32 partial slabs, no reduction launches.
 * workspace (floats): cldrd_wgrad_group_workspace(...) for a group (fp32 slabs of the problems whose token range is cut; 0 when none is),
 * cldrd_wgrad_splits(M,N1,N2) * (N1 * N2 + N1) for the single-problem form. */
int cldrd_wgrad_splits(int M, int N1, int N2);
int cldrd_wgrad16(const void* A, const void* B, float* dW, float* dbias, int M, int N1, int N2, int lda, int ldb,
                     float* workspace, size_t workspace_bytes, int accumulate, void* stream);
size_t cldrd_wgrad_group_workspace(const int* M, const int* N1, const int* N2, int n);
/* The chunk plan a group launch of these shapes uses (host only, no device call): every problem's token range is cut into n_long chunks
 * of c_long K tiles (64 tokens each) followed by n_short chunks of c_short, the launch runs all long items first, the short ones last.
 * chunks[4 i ..] = n_long, c_long, n_short, c_short of problem i;  info[0..7] = tile rows, tile columns, work items, launches (32 problems
 * each), bytes of the kernel-argument block, its limit, problems per launch, 0;  model[0] = makespan of the replayed dispatch (256 CUs,
 * items in launch order, K tiles + 6 per item), model[1] = that plus the slab traffic and the reduction launch, in K-tile times.
 * uniform_splits > 0: the same numbers for that many token splits of every problem instead of the planner's choice. */
int cldrd_wgrad_plan(const int* M, const int* N1, const int* N2, int n, int uniform_splits, int* chunks, int* info, double* model);
int cldrd_wgrad_group(const void* const* A, const void* const* B, float* const* dW, float* const* dbias, const int* M,
                      const int* N1, const int* N2, const int* lda, const int* ldb, int n, float* workspace,
                      size_t workspace_bytes, int accumulate, void* stream);

/* ---- attention (HF DistilBertSelfAttention / BertSelfAttention, head dim 64, L <= 256) --------------------
 * One entry point per operation; the layout of the [rows, .] tensors (qkv, ctx, dctx, dqkv, kv, dkv) is said by the arguments behind them:
 *   cu_rows == NULL  PADDED: rows = nseq * L, sequence m owns rows m * L .. m * L + L - 1; mask: int64 [nseq, L], 0 = padded key, or NULL.
 *   cu_rows != NULL  PACKED (layout of "packed batches" below): sequence m owns rows cu_rows[m] .. cu_rows[m + 1], rows = cu_rows[nseq]; cu_rows:
 *                    device int32 [nseq + 1], every length in 1 .. L.  mask must be NULL: keys beyond a sequence's length are masked (right padding:
 *                    what the tokenizer's attention_mask says) and padding rows are neither loaded nor stored.  The reference pads every sequence of
 *                    a batch to the longest (dataset/nway_dataset.py:105-106, dataset/sequence_dataset.py:50-51) and HF attention then computes on
 *                    the padding.  Results are bit for bit those of cldrd_unpack_rows16 -> the padded call -> cldrd_gather_rows.
 *   seq_list != NULL a LIST of a packed batch's sequences (needs cu_rows; device int32 [n_list], positions in 0 .. nseq - 1, 0 < n_list <= nseq, each
 *                    listed sequence at most Ltile tokens long, 0 < Ltile <= L): the launch runs the kernels of tile height Ltile.  A packed batch at
 *                    L = 256 sends its sequences of at most 128 tokens (most of an MS MARCO batch) through the persistent L <= 128 kernels and the
 *                    others through a second call.  seq_list == NULL: n_list and Ltile are ignored.
 * lse, probs and the keep bits are [nseq, H, L(, ..)] in every layout: LSE rows and dropout row keys keep the stride L of the batch, so forward and
 * backward of a sequence must be given the same nseq and L (the lists may differ).
 * qkv: [rows, 3*H*64] = Q | K | V;  ctx: [rows, H*64];  lse: fp32 [nseq, H, L] (NULL allowed in forward-only use, required by the backward).
 * fmt: CLDRD_FMT_BF16; CLDRD_FMT_F16_TAPE: q / k / v, ctx, dctx and dqkv are fp16 (a training pass of the fp16 mode); forward only: CLDRD_FMT_F16
 * (fp16, rows of at most 128 tokens, no keep bits: evaluation passes).  The backward takes any non-zero fmt as fp16.
 * Dropout keep bits: for L <= 128 and at least two (sequence, head) items per CU the forward runs as a persistent loader / compute kernel whose
 * loader waves evaluate the dropout hash and leave the keep decisions behind as bits in drop_bits_out ([item][key block][query] dwords, optional);
 * the backward for the same (nseq, L, H, dropout_p, seed) then reads them (drop_bits) instead of hashing again.  cldrd_attention_bits_words() says
 * how many 32-bit words that is for a shape (0: this shape does not produce bits - pass NULL and the backward re-hashes).
 * ctx_f16_copy (optional, bf16 pass only): the same context vectors in fp16 - the A operand of an fp16-operand out-projection GEMM (round 3: the
 * out-projection's operands carry most of the remaining logit drift of a 12-layer tower); ctx may then be NULL (no bf16 tape wanted). */
long long cldrd_attention_bits_words(int nseq, int L, int H, float dropout_p);
int cldrd_attention_fwd(const void* qkv, const long long* mask, const int* cu_rows, const int* seq_list, int n_list, int Ltile,
                        void* ctx, float* lse, int nseq, int L, int H, float dropout_p, unsigned long long seed, int fmt,
                        void* drop_bits_out, void* ctx_f16_copy, void* stream);
int cldrd_attention_bwd(const void* qkv, const long long* mask, const int* cu_rows, const int* seq_list, int n_list, int Ltile,
                        const void* ctx, const void* dctx, const float* lse, void* dqkv, int nseq, int L, int H, float dropout_p,
                        unsigned long long seed, int fmt, const void* drop_bits, void* stream);

/* CLS-only attention of the LAST layer (the reference pools last_hidden_state[:, 0, :], models/nway_dual_encoder.py:52,56,64):
 * qc: [nseq, H*64] = queries of token 0; kv: [rows, 2*H*64] = K | V of every token, padded or packed as above (no lists); ctx/dctx/dqc: [nseq, H*64];
 * probs: fp32 [nseq, H, L] (softmax row, saved for the backward; required); dkv: [rows, 2*H*64] in the layout of kv (every row written).
 * cldrd_add_rows: dst[row(m)] += src[m] for rows of d elements (puts the CLS-row gradients back); row(m) = idx ? idx[m] : m * stride_rows (idx: device
 * int32 [M], the CLS rows of a packed batch; stride_rows is then ignored), fmt: enum cldrd_stream_fmt below. */
int cldrd_attention_cls_fwd(const void* qc, const void* kv, const long long* mask, const int* cu_rows, void* ctx, float* probs,
                            int nseq, int L, int H, float dropout_p, unsigned long long seed, int fmt, void* ctx_f16_copy, void* stream);
int cldrd_attention_cls_bwd(const void* qc, const void* kv, const int* cu_rows, const float* probs, const void* dctx, void* dqc, void* dkv,
                            int nseq, int L, int H, float dropout_p, unsigned long long seed, int fmt, void* stream);
int cldrd_add_rows(void* dst, const void* src, int M, int d, int stride_rows, const int* idx, int fmt, void* stream);

/* ---- attention at head dim 32 (MiniLM-shaped BERT: hidden 384 / 12 heads), EVALUATION forward only (csrc/attention_hd32.hip) ---------------
 * No dropout, no LSE, no keep bits, no probs, no backward: a head-dim-32 model runs the evaluation passes and is refused for training.
 * cldrd_attention_fwd_hd32: qkv: 16-bit [rows, 3*H*32] = Q | K | V, heads contiguous inside each; ctx: [rows, H*32].  Layout rule (mask / cu_rows /
 *   seq_list, n_list, Ltile) exactly that of cldrd_attention_fwd; 0 < L <= 256.  H must be EVEN: a workgroup loads a PAIR of adjacent heads as one
 *   128-byte row slice, and with an even H no slice reads past a row.  fmt: CLDRD_FMT_BF16 (bf16 in, bf16 ctx and / or an fp16 copy in ctx_f16_copy;
 *   at least one of the two) or CLDRD_FMT_F16 (fp16 in, fp16 ctx, no copy; every L <= 256); anything else is refused.
 *   A packed batch gives the padded batch's bits on every real row and writes nothing else.  One schedule: the bits of a sequence's rows depend on
 *   its own length and the format, not on the tile height, the other sequences of the launch, their number or their order.
 * cldrd_attention_cls_fwd_hd32: the CLS form of the last layer - qc: [nseq, H*32] queries of token 0; kv: [rows, 2*H*32] = K | V of every token,
 *   padded or packed as above (no lists); ctx / ctx_f16_copy: [nseq, H*32]; fmt and the even-H rule as above. */
int cldrd_attention_fwd_hd32(const void* qkv, const long long* mask, const int* cu_rows, const int* seq_list, int n_list, int Ltile,
                             void* ctx, int nseq, int L, int H, int fmt, void* ctx_f16_copy, void* stream);
int cldrd_attention_cls_fwd_hd32(const void* qc, const void* kv, const long long* mask, const int* cu_rows, void* ctx, int nseq, int L, int H,
                                 int fmt, void* ctx_f16_copy, void* stream);

/* ---- the fp32 evaluation pass (csrc/encoder_f32.hip): the reference's `use_fp16=False` encode, retriever/retrieval_utils.py:30-58 ----------
 * Every operand fp32, accumulation on the f32-input MFMA (bit for bit a k-ordered fmaf chain).  Each op has ONE schedule, whatever the shape:
 * a row's result does not depend on which other rows share the launch, so packed == padded and a batch == its sequences alone, bit for bit.
 * Evaluation only: no dropout, no LSE, no keep bits, no tape.
 * cldrd_gemm_nt_f32: C[M,N] = A[M,K] . W[N,K]^T -> + bias[N] (optional) -> erf-GELU (act = 1, erff) -> + residual[M,N] (optional, pitch ldr).
 *   K % 32 == 0, N % 8 == 0, any M > 0; A and W 16-byte aligned, lda and ldw multiples of 4; W is the fp32 master weight, read in place.
 * cldrd_attention_fwd_f32: ctx[rows, H*64] = softmax(Q K^T / 8 + key mask) V from qkv fp32 [rows, 3*H*64]; layouts as cldrd_attention_fwd
 *   (padded rows + int64 mask or NULL, or packed rows through cu_rows - never both; no lists); L <= 256.  A masked key contributes exactly zero.
 * cldrd_attention_cls_fwd_f32: the CLS form - qc: [nseq, H*64] queries of token 0 with row pitch ldq; kv: [rows, 2*H*64] = K | V of every token,
 *   padded or packed as above; ctx: [nseq, H*64].  Bit for bit row 0 of the full form.
 * cldrd_attention_fwd_f32_hd32 / cldrd_attention_cls_fwd_f32_hd32: the same two at head dim 32 (every 64 above reads 32; any H): the same kernel
 *   text and guarantees.  A score's chain adds the head dims 0, 16, 1, 17, ..., 15, 31; the finished score is multiplied once by the fp32 nearest
 *   to 1 / sqrt(32) (no power of two: one more rounding than the exact 1 / 8 of head dim 64). */
int cldrd_gemm_nt_f32(const float* A, const float* W, float* C, int M, int N, int K, int lda, int ldw, int ldc, const float* bias,
                      const float* residual, int ldr, int act, void* stream);
int cldrd_attention_fwd_f32(const float* qkv, const long long* mask, const int* cu_rows, float* ctx, int nseq, int L, int H, void* stream);
int cldrd_attention_cls_fwd_f32(const float* qc, int ldq, const float* kv, const long long* mask, const int* cu_rows, float* ctx, int nseq,
                                int L, int H, void* stream);
int cldrd_attention_fwd_f32_hd32(const float* qkv, const long long* mask, const int* cu_rows, float* ctx, int nseq, int L, int H, void* stream);
int cldrd_attention_cls_fwd_f32_hd32(const float* qc, int ldq, const float* kv, const long long* mask, const int* cu_rows, float* ctx, int nseq,
                                     int L, int H, void* stream);

/* ---- embeddings + LayerNorm (HF Embeddings.forward, sa_layer_norm / output_layer_norm) --------------------
 * d <= 1024, d % 4 == 0.  `partial` scratch: cldrd_ln_partial_blocks(T) * 3 * d floats. */
int cldrd_ln_partial_blocks(int T);
/* Token types: type_ids == NULL: every row takes row 0 of type_table (NULL for DistilBERT, which has none); type_vocab is ignored.
 * type_ids != NULL (cross-encoder pairs): device int32 [T] (clamped to 0 .. type_vocab - 1) into the whole [type_vocab, d] table, which is then
 * required.  With all-zero type_ids it computes what type_ids == NULL does. */
int cldrd_embed_ln_fwd(const long long* ids, const float* word, const float* pos, const float* type_table, const int* type_ids,
                       int type_vocab, const float* gamma, const float* beta, void* out, float* mean, float* rstd, int T, int L,
                       int d, int vocab, float eps, float dropout_p, unsigned long long seed, float* out32, int out_f16,
                       const int* pos_idx, void* stream);
int cldrd_embed_ln_bwd(const void* dy, const long long* ids, const float* word, const float* pos, const float* type0,
                       const float* gamma, const float* mean, const float* rstd, float* dword, float* dpos,
                       float* dtype0, float* dgamma, float* dbeta, float* partial, int T, int L, int d, int vocab,
                       float dropout_p, unsigned long long seed, int accumulate, const int* pos_idx, int grad_fmt, int branch_f16,
                       const void* dy_branch, void* stream);
/* ---- the deterministic mode of the embedding backward: rows stored once, summed per table row in a fixed order, no float atomics ----
 * cldrd_embed_ln_bwd_rows: cldrd_embed_ln_bwd with dx_rows (fp32 [T, d]) in place of dword / dpos: row r receives the value cldrd_embed_ln_bwd
 *   adds into both tables for token r (the same arithmetic, bit for bit); every row is written, zeros for a token whose dy is zero.
 *   dgamma / dbeta / dtype0 as there.
 * cldrd_key_order: keys int64 [T] (clamped to 0 .. n_keys - 1, as the kernels clamp ids) -> order int32 [T], the STABLE ascending permutation of
 *   the rows by key, and offsets int32 [n_keys + 1], the CSR starts (rows of key k: order[offsets[k] .. offsets[k + 1])).  Device only, no
 *   read-back; the launch sequence depends on n_keys alone.  0 < T <= 2^22, 0 < n_keys <= 2^20; workspace: cldrd_key_order_workspace bytes.
 * cldrd_segment_sum_rows: for every key k with a non-empty list r_0 < r_1 < ... : the list is cut into chunks of CLDRD_SEGMENT_CHUNK consecutive
 *   entries, each chunk is summed in fp32 left to right, the chunk sums are added left to right in chunk order -> s;
 *   out[k] = accumulate ? out[k] + s : s (out fp32 [n_keys, d]).  Keys without rows are left untouched.  order == offsets == NULL: the strided
 *   form, row r has key r % n_keys (the position table of a padded batch: no sort).  d % 4 == 0, d <= 1024; rows / out 16-byte aligned.
 * CLDRD_SEGMENT_CHUNK = 64: the guide's rule is a quarter of one wave's share of the rows, and a training batch of 16 K .. 64 K token rows over the
 *   4 K waves the kernel keeps in flight gives a share of 4 .. 16 rows - the 512 measured there belongs to a problem a hundred times larger.  64 is
 *   the smallest chunk whose row numbers are still one full wave-wide load, and it cuts the one long list of a padded batch ([PAD], half the
 *   rows) into hundreds of chunks that 16 waves x d / 256 workgroups take in parallel. */
#define CLDRD_SEGMENT_CHUNK 64
int cldrd_embed_ln_bwd_rows(const void* dy, const long long* ids, const float* word, const float* pos, const float* type0,
                            const float* gamma, const float* mean, const float* rstd, float* dx_rows,
                            float* dtype0, float* dgamma, float* dbeta, float* partial, int T, int L, int d, int vocab,
                            float dropout_p, unsigned long long seed, int accumulate, const int* pos_idx, int grad_fmt, int branch_f16,
                            const void* dy_branch, void* stream);
size_t cldrd_key_order_workspace(int T, int n_keys);          /* bytes; 0 outside the supported range */
int cldrd_key_order(const long long* keys, int T, int n_keys, int* order, int* offsets, void* workspace, size_t workspace_bytes, void* stream);
int cldrd_segment_sum_rows(const float* rows, const int* order, const int* offsets, int T, int d, int n_keys, float* out, int accumulate,
                           void* stream);
/* ---- k-means of embedding rows (csrc/kmeans.hip): topic-aware batches cluster the query embeddings once, cldrd_amd/cluster.py ----------------
 * X fp32 [n, d] with row pitch ldx; C fp32 [k, d] contiguous; h_j = fp32(0.5 * sum_t C[j,t]^2), the sum taken in fp64 and rounded once.
 *     s(i, j)   = fp32( dot(x_i, c_j) - h_j )     dot: an fp32 fma chain over t in ONE fixed order, the same for every (i, j)
 *     assign[i] = the lowest j that attains max_j s(i, j)          (= nearest centroid in L2; ties go to the lower index)
 *     best[i]   = that maximum                                      (||x_i||^2 - 2 best[i] is the squared distance)
 * cldrd_kmeans_assign: one launch on the f32-input MFMA; the [n, k] scores never reach memory.  assign int64 [n]; best fp32 [n] or NULL.  One
 *   schedule for every n and k: assign[i] and best[i] are a function of row i and of C only - not of n, of the other rows or of how the rows are
 *   spread over launches.  No atomic, no cross-workgroup reduction.  A row holding a NaN gets centroid 0 and best = -inf.
 * cldrd_kmeans_half_sqnorm: h as defined above.
 * cldrd_kmeans_finish: the end of an update step.  sums fp32 [k, d] and offsets int32 [k + 1] come from cldrd_key_order(assign) ->
 *   cldrd_segment_sum_rows(X, order, offsets): a cluster's sum is taken in that kernel's documented order (ascending row, chunks of
 *   CLDRD_SEGMENT_CHUNK).  m = offsets[j + 1] - offsets[j] > 0: C[j] = fp32(sums[j] / fp32(m)), one rounding per element; m == 0: the centroid keeps
 *   its row (sums[j] is not read) and is counted in n_empty (int32 [1], overwritten).  h is recomputed for every row.  With the sort and the segment sum
 *   a whole Lloyd iteration is bit-reproducible: no float atomics anywhere.
 * Limits, checked before anything touches the device (cldrd_last_error names the entry point and the argument): d % 32 == 0, 32 <= d <= 1024
 *   (the segment sum's bound); 1 <= k <= 65536; assign: k <= n <= 2^22 (the key sort's bound), ldx >= d, ldx % 4 == 0; every pointer
 *   16-byte aligned; no null pointer except best.  The update needs contiguous X (ldx == d): cldrd_segment_sum_rows takes no pitch. */
int cldrd_kmeans_assign(const float* X, int ldx, int n, int d, const float* C, const float* h, int k, long long* assign, float* best, void* stream);
int cldrd_kmeans_half_sqnorm(const float* C, int k, int d, float* h, void* stream);
int cldrd_kmeans_finish(const float* sums, const int* offsets, float* C, float* h, int* n_empty, int k, int d, void* stream);
/* out = LN(x)*gamma+beta (bf16); cls_out (fp32 [T/cls_stride, d], optional) receives rows r % cls_stride == 0:
 * the `[0][:, 0, :]` CLS pooling of models/nway_dual_encoder.py:52,56,64.
 * x_f32 != 0: x is fp32 (the pre-LN sum of the fp32 residual stream) and out32 (optional) receives the fp32 output next to
 * the bf16 copy the GEMMs read; cldrd_embed_ln_fwd has the same optional out32.
 * out_f16 != 0: `out` is fp16 (operand of an fp16 forward GEMM; in the all-fp16 training mode also the backward's tape). */
int cldrd_layernorm_fwd(const void* x, const float* gamma, const float* beta, void* out, float* mean, float* rstd,
                        int T, int d, float eps, float* cls_out, int cls_stride, int x_f32, float* out32, int out_f16,
                        void* stream);
/* The format of the GRADIENT STREAM - the rows that carry dL/dx from one backward kernel to the next - is said by one code wherever such rows
 * are passed (grad_fmt of cldrd_embed_ln_bwd and cldrd_layernorm_bwd, fmt of cldrd_scatter_cls_grad and cldrd_add_rows):
 *   CLDRD_STREAM_BF16  dy is read and dx written as bf16 rows; no dy_branch.
 *   CLDRD_STREAM_F32   dy and dx are fp32 rows; needs x_f32 (the pre-LN sums of the fp32 residual stream) and dx_dropped, the 16-bit MFMA operand
 *                      of the next data-gradient GEMM (written without dropout too); dy_branch (16-bit, optional) is added to dy on load - the
 *                      output of the data-gradient GEMM of the branch that joins the residual path here.  operand_f16 / branch_f16 != 0:
 *                      dx_dropped and dy_branch are fp16, not bf16 (the all-fp16 training mode).
 *   CLDRD_STREAM_F16   dy and dx are fp16 rows carrying the loss scale; needs x_f32; dx_dropped and dy_branch are fp16 whatever operand_f16 /
 *                      branch_f16 say; dx_dropped may be NULL when no dropout separates the stream from the MFMA operand (dx then is that operand).
 * cldrd_add_rows takes an fp32 src with the fp32 and fp16 streams (fp16 dst += fp32 src, one rounding), a bf16 src with the bf16 one. */
enum cldrd_stream_fmt { CLDRD_STREAM_BF16 = 0, CLDRD_STREAM_F32 = 1, CLDRD_STREAM_F16 = 2 };
/* dx = LN backward of dy; dx_dropped (optional) = dropout-masked dx for the branch that passed through dropout;
 * dgamma/dbeta/dbias (each optional) receive sum(dy*xhat), sum(dy), sum(dx_dropped or dx).  x_f32 != 0: x holds fp32 pre-LN sums. */
int cldrd_layernorm_bwd(const void* dy, const void* x, const float* mean, const float* rstd, const float* gamma,
                        void* dx, void* dx_dropped, float* dgamma, float* dbeta, float* dbias, float* partial, int T,
                        int d, float dropout_p, unsigned long long seed, int accumulate, int x_f32, int grad_fmt, int operand_f16,
                        const void* dy_branch, void* stream);
/* Deferred form: call cldrd_layernorm_bwd with dgamma = dbeta = dbias = NULL (its `partial` then keeps the per-block sums and must
 * stay untouched), and reduce the scratch buffers of n such calls in ONE launch afterwards.  T[i] = the T of call i; outputs as
 * above, bit-identical to the immediate form.  (The parameter gradients of a LayerNorm are not on the backward's critical path.) */
int cldrd_ln_reduce_group(const float* const* partial, const int* T, float* const* dgamma, float* const* dbeta,
                          float* const* dbias, int n, int d, int accumulate, void* stream);
/* out[N] (+)= column sums of bf16 x[T,N] (bias gradients).  partial: ceil(T/128) * N floats. */
int cldrd_colsum_bf16(const void* x, float* out, float* partial, int T, int N, int ld, int accumulate, void* stream);
/* g = zeros([T,d] rows of format fmt); g[row(r)] = dcls[r]  (gradient of the CLS pooling); row(r) = idx ? idx[r] : r * stride, as in cldrd_add_rows. */
int cldrd_scatter_cls_grad(const float* dcls, void* g, int R, int d, int stride, const int* idx, int T, int fmt, void* stream);

/* ---- N-way scoring (models/nway_dual_encoder.py:30-47) ----------------------------------------------------
 * mode 0: logits[B,N]; 1: in-batch, all negatives [B,B*N]; 2: in-batch, next sample's N [B,2N]. fp32. */
int cldrd_score_fwd(const float* q, const float* p, float* logits, int B, int N, int d, int mode, void* stream);
int cldrd_score_bwd(const float* dlogits, const float* q, const float* p, float* dq, float* dp, int B, int N, int d,
                    int mode, void* stream);

/* ---- cosine-similarity scoring (--apply_consine_similarity; csrc/cosine.hip) ----------------------------------
 * The reference's scripts/unity/cosine_nway_listwise.sh names the flag, its tree has no trainer behind it: the arithmetic is this
 * package's.  With nq = max(||q||, eps), np_j = max(||p_j||, eps) (eps as in torch.nn.functional.cosine_similarity: 1e-8):
 *     logits[b, j] = scale * <q[b], p[passage(b, j)]> / (nq_b * np_j)          modes, B, N, d as cldrd_score_fwd; fp32
 * inv_norms: device float[B + B*N], written by the forward (1 / nq per query, then 1 / np per passage; the entry of a row whose norm
 * was clamped, ||row|| <= eps, is stored negated) and read by the backward, which also reads the forward's logits:
 *     dq[b] = iq * (scale * sum_j g_j ip_j p_j - (sum_j g_j logit_j) * iq * q[b])
 *     dp[m] = ip * (scale * sum g iq_b q[b]    - (sum g logit)       * ip * p[m])      sums over every (b, j) with passage(b, j) == m
 * with the second term dropped for a clamped row (its norm is the constant eps).  Forward: two launches (norms, logits); backward: two.
 * No float atomics, every sum in one fixed order: two calls give the same bits.  d % 4 == 0; scale finite and > 0; eps > 0. */
int cldrd_score_cos_fwd(const float* q, const float* p, float* logits, float* inv_norms, int B, int N, int d, int mode, float scale,
                        float eps, void* stream);
int cldrd_score_cos_bwd(const float* dlogits, const float* logits, const float* q, const float* p, const float* inv_norms, float* dq,
                        float* dp, int B, int N, int d, int mode, float scale, void* stream);
/* out[r, :d] = x[r * ld_x : +d] / max(||x[r]||, eps) for r < n, fp32; out is dense [n, d] and may be x itself (then ld_x == d).  The sum
 * of squares, the norm and each division are taken in fp64 and the quotient rounded to fp32 once.  d % 4 == 0, ld_x >= d, ld_x % 4 == 0. */
int cldrd_l2_normalize_rows(const float* x, size_t ld_x, float* out, size_t n, int d, float eps, void* stream);

/* ---- losses (losses/kl_div.py, margin_mse.py, ranknet.py, lambda_rank.py) ---------------------------------
 * kind 0 KLDiv(T) | 1 MarginMSE | 2 ranknet_loss | 3 lambda_mrr_loss (batch_weight != NULL: bweight_lambda_mrr_loss).
 * loss_out: float[2] = {loss, valid pair count}; grad [B,N] = dloss/dy_pred; workspace float[2*B]. */
int cldrd_loss_fwd_bwd(int kind, const float* y_pred, const float* y_true, const float* batch_weight, float* loss_out,
                       float* grad, float* workspace, int B, int N, float T, float pad_indicator, int mean_reduction,
                       void* stream);

/* Logit-norm regulariser `reg_loss = pred_logits.norm(2) * args.reg_lambda; loss += reg_loss`
 * (trainer/multistep-curriculum/nway_listwise_1.py:348-350): loss_out[0] += reg, grad[n] += d reg / d logits, *reg_out = reg
 * (reg_out may be null).  Same stream as, and after, cldrd_loss_fwd_bwd. */
int cldrd_logit_norm_reg(const float* logits, int n, float reg_lambda, float* loss_out, float* grad, float* reg_out, void* stream);

/* Teacher-score distillation term added behind cldrd_loss_fwd_bwd (and cldrd_logit_norm_reg) on the same stream.
 * kd = KLDiv(T)(logits[:, :Nt], teacher) (kind 0; losses/kl_div.py:11-22, batchmean, no T^2 factor) or
 *      MarginMSE()(logits[:, :Nt], teacher) (kind 1; losses/margin_mse.py:8-19, mean over B*Nt*Nt margins);
 * loss_out[0] += alpha * kd, grad[b, i] += alpha * d kd / d logits[b, i] for i < Nt, *term_out = kd (unweighted; term_out may be null).
 * logits and grad are [B, Np] (row stride Np), teacher is [B, Nt]; columns Nt..Np-1 (the in-batch negatives of
 * models/nway_dual_encoder.py:30-44, which have no teacher score) are neither read nor written.  1 <= Nt <= Np, alpha >= 0, T > 0.
 * alpha == 0 leaves loss_out and grad bit for bit.  Without a rank term the caller zeroes loss_out / grad first.  Deterministic: the
 * cross-row sum has a fixed order (no float atomics). */
int cldrd_distill_term(int kind, const float* logits, int B, int Np, const float* teacher, int Nt, float alpha, float T,
                       float* loss_out, float* grad, float* term_out, void* stream);

/* lambda_loss of losses/standard_lambda_rank.py:3-95 (allRank LambdaLoss framework): value + d loss / d y_pred in one call.
 * scheme: 0 None, 1 ndcgLoss1_scheme, 2 ndcgLoss2_scheme, 3 lambdaRank_scheme, 4 ndcgLoss2PP_scheme, 5 rankNet_scheme,
 * 6 rankNetWeightedByGTDiff_scheme, 7 rankNetWeightedByGTDiffPowed_scheme (:98-127); k <= 0: no truncation; gain_linear:
 * gain="linear" instead of "power"; log2_reduction: reduction_log="binary".  loss_out[2] = {loss, pairs}; workspace 2*B floats.
 * cldrd_loss_fwd_bwd kind 4 is weighted_pointwise_loss (losses/weighted_pointwise.py:3-14; y_true carries the weights). */
int cldrd_lambda_loss_fwd_bwd(const float* y_pred, const float* y_true, float* loss_out, float* grad, float* workspace, int B, int N,
                              int scheme, int k, float eps, float sigma, float mu, float pad_indicator, int mean_reduction,
                              int log2_reduction, int gain_linear, void* stream);

/* The term form of cldrd_lambda_loss_fwd_bwd, on the model of cldrd_distill_term: ONE launch, one workgroup per slate.
 *   term = lambda_loss(logits[:, :Ns], labels') with scheme ... gain_linear as above (pad_indicator may be -inf: nothing is padding);
 *   accumulate 0: loss_out[2] = {alpha * term, pairs}, grad[b, i] = alpha * d term / d logits[b, i] for i < Ns, 0 for Ns <= i < Np;
 *   accumulate 1: loss_out[0] += alpha * term, grad[b, i] += ... for i < Ns; columns Ns..Np-1 are neither read nor written, and
 *                 alpha == 0 leaves loss_out and grad bit for bit;
 *   *term_out = term (unweighted; term_out may be null).
 * logits and grad are [B, Np] (row stride Np), labels is [B, Ns], 1 <= Ns <= Np, Ns <= 4096, alpha >= 0.
 * labels': padding is judged on the labels as given (label == pad_indicator); on the other labels of a row, in this order:
 *   label_flags bit 0 (mean): columns n_rel..Ns-1 become their fp32 mean (left-to-right sum, one division; n_rel == Ns: nothing),
 *   label_flags bit 1 (row_min): the row's minimum is subtracted (lambda_loss clamps labels at 0: log-softmax teacher scores, all
 *   <= 0, would otherwise have no gain at all), then label_offset is added.  0 <= n_rel <= Ns.
 * workspace: 2*B floats, as for cldrd_lambda_loss_fwd_bwd.  Deterministic: the cross-row sum has a fixed order (no float atomics);
 * with accumulate 0, alpha 1, Ns == Np, label_flags 0 and label_offset 0 the outputs equal cldrd_lambda_loss_fwd_bwd's bit for bit.
 * Up to 32 launches of this entry point may be in flight on one device at a time (each takes one of 32 arrival counters in turn). */
int cldrd_lambda_term(const float* logits, int B, int Np, const float* labels, int Ns, int label_flags, int n_rel, float label_offset,
                      int scheme, int k, float eps, float sigma, float mu, float pad_indicator, int mean_reduction, int log2_reduction,
                      int gain_linear, float alpha, int accumulate, float* loss_out, float* grad, float* term_out, float* workspace,
                      void* stream);

/* Softmax cross-entropy (InfoNCE) of a row's positives against its negatives, with a temperature: value + d loss / d logits in ONE launch,
 * one workgroup per row; the fused trainer's --loss softmax_ce, in the place of cldrd_loss_fwd_bwd / cldrd_lambda_term on the loss stream.
 * The reference has no such loss: this is this package's definition.
 * logits, labels, grad: [B, Np] fp32 (labels: the label-mode constants, in-batch columns at -0.5).  Column classes of a row, from the labels:
 *   positive: label >= pos_min when has_pos_min, else label == the row's maximum label (an exact tie at the maximum: several positives);
 *   negative: label <= neg_max and not positive;   neutral: everything else - in neither sum, gradient 0.   has_pos_min: pos_min > neg_max.
 * Duplicate rule, only when pids != NULL (int64 [B, N], the passage ids of the rows' own columns; mode 0 / 1 / 2 and N as cldrd_score_fwd,
 * Np = N | B * N | 2 * N): a negative column whose pid equals the pid of a positive or neutral column of the same row becomes neutral.  The
 * passage behind column c of row b: c < N: pids[b][c]; mode 1, c >= N: global index g = c - N, shifted by N when g >= b * N; mode 2,
 * c >= N: pids[(b + 1) % B][c - N].  pids == NULL: mode and N are not used.
 * With z = logits / tau, P / G the positive / negative sets of row b and Z = sum_{j in G} exp(z_j):
 *   L_b  = (1/|P|) * sum_{i in P} [ log(exp(z_i) + Z) - z_i ]
 *   loss = mean of L_b over the valid rows (|P| >= 1 and |G| >= 1) when mean_reduction, else their sum; no valid row: 0
 *   d loss / d logits[b,i], i in P:  w * (exp(z_i) / (exp(z_i) + Z) - 1)
 *   d loss / d logits[b,j], j in G:  w * exp(z_j) * sum_{i in P} 1 / (exp(z_i) + Z)
 *        w = 1 / (tau * |P| * R),  R = number of valid rows (mean) or 1 (sum);   neutral columns and invalid rows: 0
 * evaluated after subtracting the row's maximum z over P u G.  With one positive this is cross_entropy(z[P u G], target).
 * loss_out: float[2] = {loss, valid rows}; grad: every element is written; workspace: 2*B floats.  tau > 0, 1 <= Np <= 8192.
 * Deterministic: the cross-row sum has a fixed order (no float atomics).  Up to 32 launches of this entry point may be in flight on one
 * device at a time (arrival counters as cldrd_lambda_term). */
int cldrd_softmax_ce(const float* logits, const float* labels, int B, int Np, const long long* pids, int N, int mode, float tau,
                     float pos_min, int has_pos_min, float neg_max, int mean_reduction, float* loss_out, float* grad, float* workspace,
                     void* stream);

/* ---- optimizer step (trainer/multistep-curriculum/nway_listwise_1.py:353-367) ------------------------------
 * One flat fp32 buffer for all parameters.  clip out: float[3] = {grad L2 norm, clip coefficient, non-finite flag}.
 * decay_flags: one byte per 64 parameters: bit 0 = weight decay applies, bit 1 = leave the 16-bit shadows of this chunk unwritten
 * (embedding tables: read in fp32 by the embedding kernels). */
int cldrd_sqnorm_blocks(void);
int cldrd_grad_clip_coef(const float* g, size_t n, float max_norm, float* partial, float* out, void* stream);
/* The same norm taken in pieces (the trainer takes the part of it whose gradients are complete early on its second stream, under the
 * last weight-gradient launch): cldrd_sqnorm_partial writes exactly nblk partial sums of squares of g[0, n) to partial[0, nblk);
 * cldrd_clip_coef reduces nblk_total of them (fixed order, fp64) to out[3] as cldrd_grad_clip_coef does. */
int cldrd_sqnorm_partial(const float* g, size_t n, float* partial, int nblk, void* stream);
/* Clip-norm partial sums from the kernels that WRITE the gradients (round 5): while a sink is set (thread-local, like the loss scale),
 * cldrd_wgrad_group - when it reduces token-split slabs - and cldrd_ln_reduce_group also write one sum of squares per workgroup of the
 * values they wrote to slots[used ...]; cldrd_norm_sink_used() returns the number of slots written since cldrd_set_norm_sink, -1 when
 * a launch could not contribute (a weight-gradient group without slabs) or -2 when the sink was too small for a launch: the caller then
 * takes that range's norm with cldrd_sqnorm_partial as before.  cldrd_clip_coef reduces the slots like any others.  slots = NULL: off. */
void cldrd_set_norm_sink(float* slots, int capacity);
int cldrd_norm_sink_used(void);
int cldrd_clip_coef(const float* partial, int nblk_total, float max_norm, float* out, void* stream);
/* shadow16 (NULL: none): the step also leaves an fp16 copy (RNE, as cldrd_cast_f16) of the updated parameters [h16_begin, h16_end) there
 * (shadow16[0] = parameter h16_begin; bounds multiples of 4): the query tower's high-precision forward reads fp16 weights. */
int cldrd_adamw_step(float* p, const float* g, float* m, float* v, const unsigned char* decay_flags, void* shadow,
                     size_t n, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                     const float* clip, void* shadow16, size_t h16_begin, size_t h16_end, void* stream);
int cldrd_cast_bf16(const float* src, void* dst, size_t n, void* stream);
int cldrd_transpose_cast_batched(const float* src, void* dst, const long long* desc, const int* tile_prefix, int ndesc,
                                 int total_tiles, void* stream);
/* Same transposes from the bf16 shadow (rows and cols multiples of 64, offsets multiples of 8 elements; tile_prefix in 64x64 tiles). */
int cldrd_transpose_bf16_batched(const void* src, void* dst, const long long* desc, const int* tile_prefix, int ndesc, int total_tiles,
                                 void* stream);

/* ---- exact inner-product top-k over one index shard (retriever/retrieval_utils.py:131-153 -> faiss IndexFlatIP.search) ---
 * The shard lives in HBM twice: fp32 rows (exact scores) and a 16-bit shadow the scan streams (fp16 by default: 11-bit
 * significand, so |scan - exact| <= eps is 8x tighter than with bf16; `f16` selects the MFMA type of the scan entry points).
 *
 * cldrd_flatip_search is the whole search of nq device-resident queries in passes of qtile = 128 queries (the reference's
 * batching, retrieve_top_passages.py:88) or 256 (two reference batches share one pass over the index bytes), enqueued back to
 * back with no host round trip; per pass:
 *   scan:    16-bit MFMA scores Q[qtile,d] . P[rows,d]^T; (query, row) pairs with score >= thr[query] are appended to the query's
 *            candidate list (cand_rows / cand_scores: [qtile, cap]).  counts = qtile list lengths + 1 counter of hits the
 *            streaming kernel had to drop (its on-chip list overflowed within one tile), zeroed by the caller;
 *   select:  t^ = kk-th largest scan score of the list; rows with scan score >= t^ - 2 eps[query] are kept (rows2, n2) - no other
 *            row can be in the exact top-kk (proof in csrc/topk.hip); status[query] = 0 when that proof holds, else a bit mask
 *            (1 fewer than kk candidates, 2 list overflow, 4 dropped hits, 8 thr above t^ - 2 eps, 16 kept set > cap2);
 *   rescore: exact fp32 <q, P32[row]> of the kept rows (fixed summation order);
 *   sort:    (score desc, row asc), first k -> D[nq,k], I[nq,k] (row index, -1 / -inf = missing).
 * The caller reads `status` once per search and redoes unproven queries with thresholds of its choice (same entry point).
 * `exhaustive` is a bit mask: bit 0 (rows <= cap): no scan, every row is re-scored; bit 1: the scan runs through the tiled kernels
 * (cldrd_topk_scan_filter with tiled != 0: no on-chip hit list, so status bit 4 cannot occur) - the retry form for passes that dropped hits.
 * Pieces, also callable one by one: prep (fp16 + bf16 copies and norms of the queries; *flag |= 1 if a value exceeds the fp16
 * range), kth (thr estimate: kth largest of sample scores), thresholds (eps[q] = bound on |scan - exact|, thr = est - 2 eps). */
int cldrd_cast_f16(const float* src, void* dst, size_t n, unsigned int* flag, void* stream);
int cldrd_topk_prep_queries(const float* q, void* q_f16, void* q_bf16, float* qnorm, int nq, int d, unsigned int* flag, void* stream);
int cldrd_topk_thresholds(const float* est, const float* qnorm, float pmax, int d, float* thr, float* eps, int nq, void* stream);
int cldrd_flatip_search(const float* q32, const void* q16, const float* thr, const float* eps, const void* P16, const float* P32,
                        const double* qmu, long long rows, int d, int nq, int k, int qtile, int* counts, int* cand_rows, float* cand_scores, int cap,
                        int* rows2, float* scores2, int cap2, int* n2, int* status, float* khat, float* D, int* I,
                        int exhaustive, void* stream);
/* tiled != 0: the same contract through the tiled GEMM kernels (any d % 64 == 0; hits go straight to the global lists, nothing is dropped) */
int cldrd_topk_scan_filter(const void* Q, const void* P, int nq, long long rows, int d, const float* thr, int* counts,
                           int* cand_rows, float* cand_scores, int cap, int f16, int tiled, void* stream);
int cldrd_topk_kth_largest(const float* scores, int ld, int nq, int S, int kth, float* thr, void* stream);
/* counts has nq + 1 entries (counts[nq] = dropped hits of the scan) */
int cldrd_topk_select(const int* counts, const int* cand_rows, const float* cand_scores, int nq, int cap, int kk, const float* thr,
                      const float* eps, int* rows2, int cap2, int* n2, int* status, float* khat, int exhaustive, void* stream);
int cldrd_topk_rescore(const float* q, const float* P32, const void* P16, const double* qmu, int d, const int* counts, const int* cand_rows,
                       float* cand_scores, int nq, int cap, void* stream);
int cldrd_topk_sort(const int* counts, const int* cand_rows, const float* cand_scores, int nq, int cap, int k, float* D,
                    int* I, void* stream);
/* Row modes.  P32 != NULL: fp32-row mode, the re-score reads the fp32 rows (P16 is the scan shadow only; qmu must be NULL).  P32 == NULL: fp16-row
 * mode, an index that keeps per shard mu (fp32 [d], the mean row) and P16 = fp16(p - mu) and NO fp32 rows (half the resident bytes of the scan
 * shadow + fp32 rows pair); P16 and qmu are then required.  The stored row is mu + P16[r]; its score is fp32(<q, mu> + <q, P16[r]>), both sums
 * in fp64, one rounding:
 *   cldrd_query_dot64        out[q] = <q, mu> in fp64 (device double [nq], fixed summation order): the qmu argument
 *   cldrd_topk_rescore       fp16-row mode: the rows are read from P16 (16-byte loads when d % 8 == 0) and qmu[query] is added before the rounding
 *   cldrd_flatip_search      fp16-row mode: P16 is the scan's operand and the re-scored row; same passes, status bits and `exhaustive` mask (bit 0:
 *                            no scan, every row re-scored from P16)
 *   cldrd_gather_cast_rows   dst[i] = bf16(src[i * stride]) from fp32 rows, or (src_f16 != 0) from fp16 rows: the threshold sample of an index
 *   cldrd_index_center_cast  rows [row0, row0 + rows) of a shard attached chunk by chunk (below; a whole shard is one chunk with row0 = 0) */
int cldrd_query_dot64(const float* q, const float* mu, int d, double* out, int nq, void* stream);
int cldrd_row_sqnorm_max(const float* P, size_t rows, int d, unsigned int* out, void* stream);
int cldrd_gather_cast_rows(const void* src, int src_f16, void* dst, size_t n_out, size_t stride, int d, void* stream);
/* Attaching an index shard to a GPU (what faiss' index_cpu_to_gpu does behind retriever/retrieval_utils.py:155-162 - here: the scan shadow
 * and its error-bound statistics), three launches over the fp32 rows P[rows, d]:
 *   cldrd_index_col_mean    mu[d] = mean row (fp64 column sums, fixed order); workspace: cldrd_index_col_mean_workspace(rows, d) device bytes
 *   cldrd_index_center_cast P16[r] = fp16(P[r] - mu) (the scan's operand), sample[i] = bf16(P[i * s_stride] - mu) for i < s_rows (the threshold
 *                           sample; may be NULL), *cmax_bits = bit pattern of the fp32 value of max_r |P[r] - mu|^2 (fp64 row sums; zero it
 *                           first), *flag |= 1 when a centred value is outside the fp16 range.  P, P16 point at row `row0` of the shard and
 *                           hold `rows` rows; the sample is the WHOLE shard's (a chunk writes the sample rows that fall inside it); *cmax_bits
 *                           and *flag accumulate over the chunks
 *   cldrd_map_ids           out[i] = I[i] < 0 ? -1 : (ids ? ids[I[i]] : I[i] + id_offset): faiss IndexIDMap applied to a result list */
size_t cldrd_index_col_mean_workspace(size_t rows, int d);
int cldrd_index_col_mean(const float* P, size_t rows, int d, float* mu, void* workspace, size_t workspace_bytes, void* stream);
int cldrd_index_center_cast(const float* P, const float* mu, size_t rows, size_t row0, int d, void* P16, void* sample_bf16, size_t s_stride,
                            size_t s_rows, unsigned int* cmax_bits, unsigned int* flag, void* stream);
int cldrd_map_ids(const int* I, const long long* ids, long long id_offset, long long* out, size_t n, void* stream);
/* int8-row mode (csrc/topk_i8.hip; d % 64 == 0, d <= 2048): the shard keeps mu, R8 (int8 [rows, d]) and a (fp32 [rows]) and no other form of the rows.
 * With c = p - mu (fp32): a_r = max_j |c_j| / 127, R8[r, j] = clamp(rint(c_j / a_r), -127, 127) (correctly rounded divisions, half to even; an
 * all-zero c gives a_r = 0, R8[r] = 0).  The stored row is mu + a_r R8[r]; its score is fp32(<q, mu> + a_r <q, R8[r]>), sums and product in fp64, one
 * rounding.  The scan multiplies int8 query digits (sq = max|q| / 16256, t = rint(q / sq), l = ((t + 64) mod 128) - 64, h = (t - l) / 128) with R8 on
 * the i8 MFMA, H = <h, R8[r]>, L = <l, R8[r]> exact in int32, and scores s^ = fmaf(128.0f, (float)H, (float)L) * (sq * a_r) in fp32.
 *   cldrd_index_quantize_i8    one fp32 chunk of a shard (rows [row0, row0 + rows), as cldrd_index_center_cast): R8, a, the bf16 threshold sample of the
 *                              stored centred rows, *b1_bits / *c2_bits = bit patterns of the fp32 values of max_r a_r |R8[r]|_1 and max_r a_r^2 |R8[r]|_2^2
 *                              (fp64 products with the exact integer sums), *flag |= 1 for a value that is not finite; the three words accumulate over
 *                              the chunks (zero them first)
 *   cldrd_topk_prep_queries_i8 qd = int8 [2, nq, d] (plane 0: h, plane 1: l), sq and |q| (fp32 [nq]), the bf16 copy for the threshold GEMM, *flag |= 1
 *                              for a value that is not finite.  A query with max|q| < 2^-100 gets zero digits and sq = 2 max|q|
 *   cldrd_topk_thresholds_i8   eps[q] >= |s^ - a_r <q, R8[r]>| from sq, |q|, b1 = max_r a_r |R8[r]|_1 and cnorm = max_r a_r |R8[r]|_2 (derivation in
 *                              csrc/topk_i8.hip); thr = est - 2 eps (est may be NULL: eps only)
 *   cldrd_topk_scan_i8         nq <= 256 queries of the digit planes (`qd` points at this call's first query in plane 0, the planes hold nq_plane queries
 *                              each) against the rows: every (query, row) with s^ >= thr[query] is appended to the query's list; counts = nq list lengths
 *                              + 1 counter of the hits that found their list full (those also count in counts[query]), zeroed by the caller
 *   cldrd_topk_rescore_i8      cand_scores[q][c] = fp32(qmu[q] + a_r <q, R8[row]>) for c < counts[q] (qmu: cldrd_query_dot64)
 *   cldrd_flatip_search_i8     the chain of cldrd_flatip_search per tile of qtile = 128 queries: scan (exhaustive = 1: every row, rows <= cap) -> select
 *                              -> rescore_i8 -> sort; the same counts / n2 / status / khat contract */
int cldrd_index_quantize_i8(const float* P, const float* mu, size_t rows, size_t row0, int d, void* R8, float* scale, void* sample_bf16,
                            size_t s_stride, size_t s_rows, unsigned int* b1_bits, unsigned int* c2_bits, unsigned int* flag, void* stream);
int cldrd_topk_prep_queries_i8(const float* q, void* qd, void* q_bf16, float* sq, float* qnorm, int nq, int d, unsigned int* flag, void* stream);
int cldrd_topk_thresholds_i8(const float* est, const float* sq, const float* qnorm, float b1, float cnorm, int d, float* thr, float* eps, int nq,
                             void* stream);
int cldrd_topk_scan_i8(const void* qd, long long nq_plane, const float* sq, const float* thr, const void* R8, const float* scale, int nq,
                       long long rows, int d, int* counts, int* cand_rows, float* cand_scores, int cap, void* stream);
int cldrd_topk_rescore_i8(const float* q, const void* R8, const float* scale, const double* qmu, int d, const int* counts, const int* cand_rows,
                          float* cand_scores, int nq, int cap, void* stream);
int cldrd_flatip_search_i8(const float* q32, const void* qd, const float* sq, const float* thr, const float* eps, const void* R8,
                           const float* scale, const double* qmu, long long rows, int d, int nq, int k, int qtile, int* counts, int* cand_rows,
                           float* cand_scores, int cap, int* rows2, float* scores2, int cap2, int* n2, int* status, float* khat, float* D,
                           int* I, int exhaustive, void* stream);

/* ---- variable-length packing (csrc/pack.hip) -----------------------------------------------------------------------------------
 * The reference pads every sequence of a batch to the longest one (dataset/sequence_dataset.py:50-51, nway_dataset.py:103-107) and the
 * encoder computes on the padding.  Packed layout: tokens of sequence m = rows cu[m] .. cu[m+1] of a [Tp, features] matrix (cu: device
 * int32 [nseq + 1]); Linear / LayerNorm / weight gradients run on the Tp real rows, attention on the same rows through the
 * cldrd_attention_* calls above given cu_rows (until round 6: on the padded [nseq * L, .] layout, rows moved by the two calls below).
 * cldrd_embed_ln_fwd / _bwd take pos_idx (device int32 [T], the position of every row inside its sequence; NULL: row % L).
 *   unpack_rows16: dst[m * L + j] = j < len[m] ? src[cu[m] + j] : 0  (16-bit rows of w elements);  gather_rows: dst[p] = src[idx[p]]
 *   (rows of row_bytes bytes: packing, CLS rows);  the CLS rows of a packed batch go to cldrd_scatter_cls_grad / cldrd_add_rows as idx. */
int cldrd_unpack_rows16(const void* src_packed, void* dst_padded, const int* cu, int nseq, int L, int w, void* stream);
int cldrd_gather_rows(const void* src, const int* idx, void* dst, int n, int row_bytes, void* stream);
int cldrd_gather_i64(const long long* src, const int* idx, long long* dst, int n, void* stream);      /* dst[p] = src[idx[p]]: token ids of the packed rows */

/* ---- per-step state in device memory: what lets a whole training step be captured into a HIP graph and replayed -------------------
 * Kernel arguments are frozen at capture; a dropout seed and the optimizer's lr / bias-corrected step size change every step.  With a
 * seed base installed, every launch of the calling thread passes its `seed` argument as an OFFSET and the kernels add the 64-bit word at
 * `base` (device memory) at run time; with the optimizer hyper-parameters installed, cldrd_adamw_step reads {lr, step size} from the
 * device float[2].  cldrd_write_step_state writes both (seeds[0..1]: one word per tower) in stream order - the one launch the trainer
 * makes in front of each replay.  NULL uninstalls; nothing installed = the by-value arguments, as before (bit-identical results). */
void cldrd_set_seed_base(const unsigned long long* base);
void cldrd_set_optim_hyper(const float* hyper);
/* The all-fp16 training mode (round 4; the reference trains under fp16 autocast + torch.cuda.amp.GradScaler, trainer/multistep-curriculum/
 * nway_listwise_1.py:334-359): every 16-bit tensor of the backward is fp16 and carries a loss scale S, parameter gradients never do.
 * `scale` = device float[72] {S, 1 / S, finite steps since the headroom changed, skipped steps, headroom exponent h <= 0, 3 unused, 64 scratch},
 * or null (off).  While set, launches of THIS thread read it on the device at run time: cldrd_wgrad_group, cldrd_layernorm_bwd /
 * cldrd_embed_ln_bwd (their parameter-gradient sums and the embedding-table scatter) multiply by 1 / S; cldrd_clip_coef /
 * cldrd_grad_clip_coef run the safety net (non-finite gradient norm: AdamW skips the step and the next steps get 4x more headroom;
 * growth_interval finite steps in a row give a factor 2 back).  cldrd_loss_scale_adapt sets S = 2^(12 + h - ceil(log2 max(|a|, |b|)))
 * from the gradient that enters the towers (a, b = dL/dCLS of the two towers, fp32, from cldrd_score_bwd) and multiplies both by it in
 * place: a power of two recomputed from the data every step, where GradScaler searches by overflowing and backing off. */
void cldrd_set_loss_scale(const float* scale, int growth_interval);
int cldrd_loss_scale_adapt(float* a, size_t na, float* b, size_t nb, float* state, void* stream);
/* n <= 8 small device-to-device copies in one launch (host arrays of pointers / byte counts): the inputs of a captured step. */
int cldrd_copy_segments(const void* const* src, void* const* dst, const size_t* bytes, int n, void* stream);
/* n <= 8 device ranges (16-byte aligned, sizes multiples of 16) set to zero in one launch: what optimizer.zero_grad() is reduced to - only the
 * embedding tables' gradients are accumulated into (reference nway_listwise_1.py:365 zeroes every gradient). */
int cldrd_zero_segments(void* const* dst, const size_t* bytes, int n, void* stream);
int cldrd_write_step_state(unsigned long long* seeds, unsigned long long seed0, unsigned long long seed1, float* hyper, float lr,
                           float beta1, float beta2, int adam_step, const float* scale_state, void* stream);

/* ---- cross-encoder scoring (csrc/cross.hip) --------------------------------------------------------------------------------------
 * cldrd_build_pairs: packed rows of `[CLS] q' [SEP] p' [SEP]` from token-cache rows (`[CLS] text [SEP]`, zero padded; tables of uint16 or
 *   int32 elements, q_bytes / p_bytes = 2 or 4, row strides in elements, lens device int32 per table row).  Pair m reads query row q_rows[m]
 *   and passage row p_rows[m], keeps keep_q[m] / keep_p[m] content tokens and owns packed rows cu[m] .. cu[m + 1] (cu: device int32
 *   [n_pairs + 1]; a pair of keep_q + 2 rows is the single sequence `[CLS] q' [SEP]`).  Writes token ids int64, token types int32 (0 up
 *   to and including the first [SEP], then 1; optional) and positions int32 (optional).  The host computes keep / cu (the tokenizer's
 *   longest_first truncation: models/cross_encoder.py pair_lengths).
 * cldrd_cls_head_fwd: logits fp32 [M, num_labels] = W2 act(W1 cls + b1) + b2 in fp32; cls fp32 [M, d], W1 [d, d], W2 [num_labels, d];
 *   act 0 = tanh (BERT pooler), 1 = ReLU (DistilBERT pre_classifier).  d <= 1024. */
int cldrd_build_pairs(const void* q_tok, const int* q_lens, int q_stride, int q_bytes, const void* p_tok, const int* p_lens, int p_stride,
                      int p_bytes, const int* q_rows, const int* p_rows, const int* keep_q, const int* keep_p, const int* cu, int n_pairs,
                      long long* out_ids, int* out_types, int* out_pos, void* stream);
int cldrd_cls_head_fwd(const float* cls, const float* w1, const float* b1, const float* w2, const float* b2, float* out, int M, int d,
                       int num_labels, int act, void* stream);

/* ---- curriculum selection (csrc/curriculum.hip; the device form of dataset/curriculum_file.py select_examples) ---------------------
 * From the search's ids and the teacher's scores as they lie in HBM to a curriculum stage's training examples, one workgroup per query.
 * In (device): qid int64 [nq]; pid int64 [nq, K], candidates in run order; score fp32 [nq, K]; count int32 [nq], the live candidates of
 * the row (clamped to 0 .. K; entries at positions >= count are never read).  The spec as dataset.curriculum_file.CurriculumSpec: n_rel,
 * and per window the number drawn and its 1-based inclusive teacher ranks lo .. hi (a window that draws nothing is ignored; one that
 * draws must start after n_rel and hold at least as many ranks as it draws, and the two must not overlap: refused otherwise).
 * Out (device):
 *   order int32 [nq, K]   order[q, r] = run position of the candidate at teacher rank r: score descending, ties by run position
 *                         ascending (-0.0 == 0.0); -1 at r >= count
 *   keep int32 [nq]       1 where count >= min_candidates = max(n_rel, hi of every window that draws), else 0
 *   sel_pid int64, sel_score fp32 [nq, n_rel + n_most_hard + n_semi_hard]: the top n_rel in teacher order, then from each window the
 *                         n candidates with the smallest key splitmix64(splitmix64(splitmix64(seed) ^ qid) ^ pid) (uint64 wrap-around,
 *                         ids as two's complement, ties by pid), written in teacher order.  Rows with keep == 0 are left untouched.
 * K <= 1024 (refused above).  Preconditions: the live scores are finite and the live pids of a row are distinct; a row that breaks
 * them gets an unspecified (never out-of-bounds) result. */
int cldrd_curriculum_select(const long long* qid, const long long* pid, const float* score, const int* count, int nq, int K,
                            int n_rel, int n_most_hard, int most_lo, int most_hi, int n_semi_hard, int semi_lo, int semi_hi,
                            unsigned long long seed, int* order, int* keep, long long* sel_pid, float* sel_score, void* stream);

/* ---- teacher score store (csrc/pairstore.hip; retriever/score_store.py) --------------------------------------------------------------
 * A segment is three parallel device arrays, q int64 / p int64 / s fp32, of 1 .. 2^31 - 1 entries strictly ascending in the key (q, p):
 * lexicographic, q major, signed 64-bit compares.
 * cldrd_pair_lookup: the pairs of a CSR batch - qid int64 [nq], starts int64 [nq + 1] (row r's pairs are starts[r] .. starts[r + 1],
 *   clamped to 0 .. total), pid int64 [total] - searched in ONE segment, one workgroup per row (rows of any length, 0 included).  A pair
 *   found at entry j gets score_out[i] = seg_s[j] (the stored bits) and hit[i] = 1 (uint8); a pair not found leaves both untouched, so
 *   calls over several segments accumulate.  nq >= 1 (refused otherwise).
 * cldrd_pair_merge: two segments with no key in common, na >= 1 and nb >= 1 entries, na + nb <= 2^31 - 1, merged into out_* of exactly
 *   na + nb entries.  *dup_flag (int32, device, zeroed by the caller) is set to 1 when a key occurs in both inputs (the output then
 *   holds it twice and is not a segment). */
int cldrd_pair_lookup(const long long* seg_q, const long long* seg_p, const float* seg_s, long long n, const long long* qid,
                      const long long* starts, const long long* pid, long long nq, long long total, float* score_out, unsigned char* hit,
                      void* stream);
int cldrd_pair_merge(const long long* a_q, const long long* a_p, const float* a_s, long long na, const long long* b_q, const long long* b_p,
                     const float* b_s, long long nb, long long* out_q, long long* out_p, float* out_s, int* dup_flag, void* stream);

/* ---- run file (retriever/retrieve_top_passages.py:98-105), HOST side: no GPU work -----------------------------------------
 * Writes `qid\tdocid\trank\tscore\n` for nq queries x k hits (rank 1..k) to `path`; the score text is Python's repr of the fp32
 * value widened to a double, which is what the reference's f-string prints.  All pointers are HOST pointers.  Formatted by nthreads
 * host threads (<= 0: one per hardware thread, at most 64).  Returns the number of lines or -1. */
long long cldrd_write_run_file(const char* path, const long long* qids, const long long* docids, const float* scores,
                               long long nq, int k, int nthreads);
int cldrd_py_float_repr(double x, char* out32);

/* ---- merge of per-shard top-k lists (the host-side merge of the 8-way sharded retrieve, BASELINE.json north_star; the reference meant
 * faiss' IndexShards for it: retriever/retrieval_utils.py:164-182, retrieve_top_passages.py:85-88) -------------------------------------
 * Shard r contributes, per query, scores fp32 [k_in] descending and global ids int64 [k_in] (-1 = missing, missing last).  Result: the
 * k_out best of the world * k_in candidates by (score desc; ties: shard asc, then list position asc = global row position asc, the tie
 * rule of the single-index search), padded with (-inf, -1).
 * cldrd_merge_topk: HOST pointers (shard_scores[r] / shard_ids[r] = that shard's [nq, k_in] block), nthreads host threads (<= 0: one
 *   per hardware thread, at most 64).  Unsorted lists are accepted (that query is partially sorted instead of merged).
 * cldrd_merge_topk_device: DEVICE pointers, scores / ids = [world, nq, k_in] (what a gather over RCCL leaves on rank 0), world * k_in
 *   <= 8192 and k_out <= world * k_in; one sort launch per call; `workspace` of cldrd_merge_topk_device_workspace() bytes. */
int cldrd_merge_topk(const float* const* shard_scores, const long long* const* shard_ids, int world, long long nq, int k_in, int k_out,
                     float* D, long long* I, int nthreads);
size_t cldrd_merge_topk_device_workspace(int world, long long nq, int k_in, int k_out);
int cldrd_merge_topk_device(const float* scores, const long long* ids, int world, long long nq, int k_in, int k_out, float* D,
                            long long* I, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif

/* memehip -- C ABI of the MI355X (gfx950) kernels behind the Subtask-2C fine-tune step.
 *
 * The reference (KevinMathewT/multimodal-propaganda-meme-classification) is 100 % Python and has
 * no FFI: its hot path reaches the arithmetic through PyTorch / transformers / timm calls.  Each
 * entry point below names the reference call site whose implied kernel it replaces
 * (paths relative to /root/reference/example_scripts).  INTEGRATION.md shows the ctypes binding.
 *
 * Two builds of the same sources export this ABI: libmemehip.so stores 16-bit tensors as bfloat16
 * ("bf16" below), libmemehip_f16.so (-DMH_FP16) as IEEE half with the same MFMA rate.  Gradient
 * streams of the 16-bit towers may carry a power-of-two scale (needed for half): it enters through
 * mh_head_bwd(out_scale) and is removed where parameter gradients are produced (MhGemmProblem.alpha,
 * the `scale` arguments below), so every f32 gradient buffer holds true gradients.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless marked "host"; no ownership transfer, no
 *     allocation, no synchronisation inside; work is enqueued on `stream` (a hipStream_t).
 *   - bf16 = raw uint16 bfloat16 storage; f32 = float; ids/masks/labels = int64 (torch.long),
 *     exactly the tensors the reference Dataset yields (Multimodal_example_task2C.txt:61-71).
 *   - return value: MH_OK (0) or an MhStatus code; nothing throws across the ABI.
 */
#ifndef MEMEHIP_H
#define MEMEHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum MhStatus {
    MH_OK = 0,
    MH_EINVAL = 1,  /* null pointer / bad flag */
    MH_ESHAPE = 2,  /* shape not supported by the gfx950 tiling (see each function) */
    MH_ELAUNCH = 3  /* hipLaunch / runtime error (hipGetLastError) */
} MhStatus;

typedef void* mh_stream_t; /* hipStream_t */

const char* mh_version(void);
const char* mh_status_str(int status);

/* ------------------------------------------------------------------------------------------
 * Grouped bf16 GEMM with fused epilogue:  C = epi(A . B^T)   (fp32 accumulate on MFMA)
 * replaces every nn.Linear inside both encoders, forward / dgrad / wgrad
 * (BertModel / timm ViT via Multimodal_example_task2C.txt:175,183 ; loss.backward() :216).
 *
 *   a_kmajor == 0 : A is [M][K] row-major (lda elements per row)     -- K contiguous
 *   a_kmajor == 1 : A is [K][M] row-major (lda elements per K row)   -- K strided
 *   b_kmajor == 0 : B is [N][K] (nn.Linear weight layout)            -- K contiguous
 *   b_kmajor == 1 : B is [K][N]                                      -- K strided
 *   forward  y = x W^T      : (0,0)  A=x[T][K]      B=W[N][K]
 *   dgrad    dx = dy W      : (0,1)  A=dy[T][N']    B=W[N'][K']   (contracts over N')
 *   wgrad    dW = dy^T x    : (1,1)  A=dy[T][N']    B=x[T][K']    (contracts over T)
 *
 * Epilogue order:  v = alpha * acc (+ bias[n]);  if drop_rng: v = dropout(v);  if aux: aux[m,n] = bf16(v);  if GELU: v = gelu_erf(v)
 *                  (quick-GELU x*sigmoid(1.702x) with MH_GEMM_QUICK_GELU, which also selects the derivative for `mul`);
 *                  if mul_dgelu: v *= gelu'(mul[m,n]);  if residual: v += residual[m,n];
 *                  C[m,n] = v  (bf16, or f32 when MH_GEMM_OUT_F32; += when MH_GEMM_ACCUM with f32).
 * rowsum (wgrad only, a_kmajor==1): rowsum[m] = sum_k A(m,k)  -- the bias gradient.
 * Constraints: N % 8 == 0 (128-column tiles; a last partial tile computes and discards the columns past N);
 * K % 64 == 0 unless the contraction dim is the leading (row) index of both operands (a_kmajor && b_kmajor), in
 * which case any K; M any when a_kmajor==0, else M % 8 == 0; ld* % 8 == 0; all bases 16-byte aligned; up to
 * MH_GEMM_MAX_GROUP problems.
 * ------------------------------------------------------------------------------------------ */
#define MH_GEMM_MAX_GROUP 8
#define MH_GEMM_GELU 1
#define MH_GEMM_OUT_F32 2
#define MH_GEMM_ACCUM 4
#define MH_GEMM_QUICK_GELU 8 /* the activation (MH_GEMM_GELU) and the derivative (mul) are quick-GELU x*sigmoid(1.702x): CLIP towers */
#define MH_GEMM_DERIV_AUX 16 /* with MH_GEMM_GELU: aux receives act'(v) instead of v (same exponential as the activation);
                              * with `mul`: the operand IS that stored derivative and is multiplied in as it is -- the pair moves
                              * the erf / exp of the backward epilogue into the forward one, where it is computed anyway */

typedef struct MhGemmProblem {
    const void* A;        /* bf16 */
    const void* B;        /* bf16 */
    void* C;              /* bf16 [M][ldc] or f32 [M][ldc] */
    const float* bias;    /* f32 [N] or NULL */
    const void* residual; /* bf16 [M][ldc] or NULL */
    void* aux;            /* bf16 [M][ldc] pre-activation copy or NULL */
    const void* mul;      /* bf16 [M][ldc] pre-activation whose gelu' scales the result, or NULL */
    float* rowsum;        /* f32 [M] or NULL */
    int32_t M, N, K;
    int32_t lda, ldb, ldc;
    int32_t flags;
    float alpha;          /* accumulator scale applied first (0 means 1): un-scales 16-bit gradient streams */
    const uint32_t* drop_rng; /* device u32[4] {seed_lo, seed_hi, step, -} or NULL: nn.Dropout on (acc + bias) */
    float drop_p;
    uint32_t drop_stream;     /* id of this dropout site (mask = f(rng, site, m * N + n)) */
    const int32_t* rows_dev;  /* device int32 or NULL: live token rows of a PACKED (padding-free) operand, read at launch
                                 time.  Clamps M (a_kmajor==0: tiles past it exit) or the contraction K (a_kmajor==1). */
    const int32_t* drop_rows; /* device int32 [M] or NULL: row m's index in the unpacked tensor (dropout mask index) */
    int32_t ksplit;           /* > 1: split-K for few-tile / long-contraction problems (conv weight gradients: K = B*H*W).  The
                                 contraction is cut into exactly `ksplit` chunks of ceil(K / ksplit) rounded up to 64 (the call
                                 returns MH_ESHAPE when that leaves a chunk empty: use mh_gemm_ksplit_for); chunk s writes
                                 alpha * partial to the f32 slab C + s*M*ldc; no epilogue operands; sum the slabs with
                                 mh_colsum_partials_f32(n_part = ksplit, D = M*ldc).  0 / 1 = off. */
    int32_t reserved_;
} MhGemmProblem;

int mh_gemm_bf16_grouped(const MhGemmProblem* problems /*host*/, int n_problems, int a_kmajor,
                         int b_kmajor, mh_stream_t stream);
/* a split count <= want for which every chunk of ceil(K/ksplit) rounded up to 64 is non-empty (1 when K is short) */
int mh_gemm_ksplit_for(int K, int want);
/* Host-only, launches nothing: 1 when mh_gemm_bf16_grouped runs this group on the skinny-M kernel (gemm_skinny_kernel: one wave per
 * 16 output columns, weights streamed to registers several K tiles ahead), 0 when on the 128x128 tile kernel.  The rule, a pure
 * function of the arguments (a captured graph replays the same kernel): a_kmajor == 0; every problem has M <= 64, no rows_dev,
 * ksplit <= 1 and no drop_rng; and the group is narrower than 128 column tiles of 128 in all (sum of ceil(N / 128) < 128: wider
 * launches fill the chip on the tile kernel).  Both kernels give the same bits; the launcher calls this very function. */
int mh_gemm_skinny_eligible(const MhGemmProblem* problems /*host*/, int n_problems, int a_kmajor, int b_kmajor);
/* (These two kernels are the library's only GEMMs.  What was measured against them and lost -- register staging, 4 / 16 waves,
 * 256x128 rings, four-slot ring, double-buffered fragments, K-split waves, persistent workgroups, stream-K, the 128x256 tile, the
 * direct-from-accumulator epilogue -- is recorded with its numbers in DESIGN.md section 5 and tools/lab/RESULTS.md.) */
/* profiling knob: device buffer of 4 x uint64 per workgroup of the largest launch; the 128x128 tile kernel records 100-MHz stamps per
 * workgroup {entry, first K stage landed, main loop done, epilogue stores issued}; NULL = off (tools/gemm_timeline.py) */
int mh_gemm_set_trace(void* device_buffer);

/* ------------------------------------------------------------------------------------------
 * LayerNorm over the last dim (D % 8 == 0, D <= 4096 forward, <= 2048 backward), one wavefront per row.
 * replaces nn.LayerNorm inside BertModel (eps 1e-12, post-LN) and timm ViT (eps 1e-6, pre-LN).
 *   fwd:  y = (x - mean) * rstd * gamma + beta ; saves mean[rows], rstd[rows] (f32)
 *   bwd:  dx (bf16; added to dx_add when non-NULL), partial dgamma/dbeta in
 *         part[2][n_part][D] (f32, one row per workgroup; the launch uses n_part workgroups) --
 *         finish with mh_colsum_partials_f32.
 * ------------------------------------------------------------------------------------------ */
int mh_layernorm_fwd(const void* x /*bf16*/, const float* gamma, const float* beta, void* y /*bf16*/,
                     float* y_f32 /*optional unrounded copy of y, or NULL*/, float* mean, float* rstd,
                     int rows, int D, float eps, mh_stream_t stream);
int mh_layernorm_bwd(const void* dy /*bf16*/, const void* x /*bf16*/, const float* gamma,
                     const float* mean, const float* rstd, const void* dx_add /*bf16 or NULL*/,
                     void* dx /*bf16*/, float* part /*[2][n_part][D]*/, int n_part, int rows, int D,
                     void* dx_drop /*bf16 or NULL: dx * dropout-mask/(1-p) of the Linear output that fed this LN*/,
                     const uint32_t* rng, float drop_p, uint32_t drop_stream, mh_stream_t stream);
/* Grouped forms: several LayerNorms of the same width D in ONE launch (the two towers' LayerNorms
 * sit at the same point of the lockstep layer schedule; each is too small to fill 256 CUs alone). */
#define MH_LN_MAX_JOBS 4
typedef struct MhLnFwdJob {
    const void* x; const float* gamma; const float* beta; void* y; float* y_f32; float* mean; float* rstd;
    int32_t rows; float eps;
    const int32_t* rows_dev;  /* device int32 or NULL: live rows of a packed tensor (<= rows), read at launch time.  x holds
                                 `rows` rows and the forward may READ any of them; only live rows are written */
} MhLnFwdJob;
typedef struct MhLnBwdJob {
    const void* dy; const void* x; const float* gamma; const float* mean; const float* rstd;
    const void* dx_add; void* dx; float* part; void* dx_drop; const uint32_t* rng;
    int32_t n_part; int32_t rows; float drop_p; uint32_t drop_stream;
    const int32_t* rows_dev;  /* as in MhLnFwdJob */
    const int32_t* drop_rows; /* device int32 [rows] or NULL: row index in the unpacked tensor (dropout mask index) */
} MhLnBwdJob;
int mh_layernorm_fwd_grouped(const MhLnFwdJob* jobs, int n_jobs, int D, mh_stream_t stream);
int mh_layernorm_bwd_grouped(const MhLnBwdJob* jobs, int n_jobs, int D, mh_stream_t stream);
/* batched finish of the partial column sums: for every job, out0[d] = sum_i part[0][i][d] and
 * out1[d] = sum_i part[1][i][d] (fixed order => bitwise reproducible); NULL outputs are skipped. */
#define MH_COLSUM_MAX_JOBS 64
typedef struct MhColsumJob {
    const float* part; /* [2][n_part][D] */
    float* out0;       /* [D] dgamma */
    float* out1;       /* [D] dbeta  */
} MhColsumJob;
int mh_colsum_partials_f32(const MhColsumJob* jobs /*host*/, int n_jobs, int n_part, int D,
                           float scale, mh_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Fused multi-head attention (head dim 64), flash-style, bf16 in / f32 softmax.
 * replaces BertSelfAttention / timm Attention (scores = q k^T / 8 + (1-mask)*min; softmax; P v).
 *   qkv : bf16 [B][S][3][H][64]  (the fused QKV projection output; row pitch 3*H*64)
 *   key_mask : int64 [B][S] (1 = attend) or NULL (ViT)
 *   out : bf16 [B][S][H][64] ; lse : f32 [B][H][S]  (log-sum-exp of the scaled scores)
 *   bwd : dqkv bf16 [B][S][3][H][64] from dout, recomputing P from lse; delta = rowsum(dout*out)
 *         is computed inside (workspace delta f32 [B][H][S]).
 *   rng != NULL, drop_p > 0: dropout on the probabilities (attention_probs_dropout_prob); mask element index
 *         ((b*H + h)*S + q)*S + k; the backward regenerates the same mask.
 *   A query with no key to attend to (key_mask all zeros for its sequence, e.g. the pooled row mh_pack_plan keeps for an
 *         empty mask row) gets out = 0 and lse = -inf, and contributes no gradient (its dq row is 0, and keys it sees are all
 *         masked).  BertSelfAttention would instead average V over all S positions; the packed form has dropped those rows.
 * ------------------------------------------------------------------------------------------ */
int mh_attn_fwd(const void* qkv, const int64_t* key_mask, void* out, float* lse, int B, int S, int H,
                const uint32_t* rng, float drop_p, uint32_t drop_stream, mh_stream_t stream);
int mh_attn_bwd(const void* qkv, const int64_t* key_mask, const void* out, const void* dout,
                const float* lse, float* delta, void* dqkv, int B, int S, int H, const uint32_t* rng,
                float drop_p, uint32_t drop_stream, mh_stream_t stream);
/* Packed (padding-free) form: sequence b owns token rows cu[b] .. cu[b+1]-1 of qkv / out / dout / dqkv (cu = device
 * int32 [B+1] from mh_pack_plan, at most S rows each); key_mask is indexed by PACKED row; lse / delta stay [B][H][S].
 * row_map (packed row -> b*S + position, or NULL) keeps the dropout mask indices those of the unpacked tensor. */
int mh_attn_fwd_packed(const void* qkv, const int64_t* key_mask, void* out, float* lse, const int32_t* cu,
                       const int32_t* row_map, int B, int S, int H, const uint32_t* rng, float drop_p,
                       uint32_t drop_stream, mh_stream_t stream);
int mh_attn_bwd_packed(const void* qkv, const int64_t* key_mask, const void* out, const void* dout,
                       const float* lse, float* delta, void* dqkv, const int32_t* cu, const int32_t* row_map, int B,
                       int S, int H, const uint32_t* rng, float drop_p, uint32_t drop_stream, mh_stream_t stream);

/* Grouped form: up to MH_ATTN_MAX_GROUP problems per call.  The two towers' attention of a layer pair
 * (ViT: 129..224 tokens, no dropout; text: <= 128 tokens) goes out as ONE launch per kernel: the short text heads
 * fill the occupancy holes of the ViT launch.  Other combinations run back to back.  The backward fields are
 * ignored by mh_attn_fwd_grouped; cu / row_map select the packed form per problem. */
#define MH_ATTN_MAX_GROUP 2
typedef struct MhAttnProblem {
    const void* qkv; const int64_t* key_mask; void* out; float* lse;
    const void* dout; float* delta; void* dqkv;
    const int32_t* cu; const int32_t* row_map;
    const uint32_t* rng; float drop_p; uint32_t drop_stream;
    int32_t B, S, H; int32_t reserved;
} MhAttnProblem;
int mh_attn_fwd_grouped(const MhAttnProblem* problems /*host*/, int n, mh_stream_t stream);
int mh_attn_bwd_grouped(const MhAttnProblem* problems /*host*/, int n, mh_stream_t stream);
/* backward of 129..224-token heads without mask / dropout / packing (the ViT tower): 1 = ONE pass per head (five products per
 * block pair, dQ summed across key blocks through LDS mailboxes in a fixed order), 2 = the same with the text tower's sweeps in
 * the same launch when two problems are grouped (default), 0 = the dQ sweep + dK/dV sweep */
int mh_attn_set_onepass(int on);

/* ------------------------------------------------------------------------------------------
 * Padding-free text tower.  BertModel computes every padded position and then ignores it (the keys are masked,
 * the pooling reads one row): rows with attention_mask == 0 influence neither the logits nor any gradient.
 * mh_pack_plan turns the Dataset's `text_mask` (Multimodal_example_task2C.txt:64) into the row bookkeeping of a
 * PACKED token stream that holds only the rows that matter: mask != 0, plus the pooled position of each sequence
 * (query-only when it is padding, e.g. the organizers' [:, -1, :] pooling).  Everything is device-side, so the
 * launch sequence (and a captured hipGraph) is the same for every batch; kernels read n_rows at run time.
 *   cu        int32 [B+1]  first packed row of each sequence (cu[B] = n_rows)
 *   row_map   int32 [B*S]  packed row -> b*S + position ; -1 past n_rows
 *   inv_map   int32 [B*S]  b*S + position -> packed row ; -1 for dropped (padding) positions
 *   pmask     int64 [B*S]  key mask by packed row (0 past n_rows)
 *   pool_rows int32 [B]    packed row of the pooled position
 *   n_rows    int32 [1]
 * mh_pack_rows: dst[r] = src[row_map[r]] for r < n_rows;  mh_unpack_rows: dst[d] = src[inv_map[d]], dropped rows 0.
 * B <= 1024.
 * ------------------------------------------------------------------------------------------ */
int mh_pack_plan(const int64_t* mask /*[B][S]*/, int B, int S, int pool_index, int32_t* cu, int32_t* row_map,
                 int32_t* inv_map, int64_t* pmask, int32_t* pool_rows, int32_t* n_rows, mh_stream_t stream);
int mh_pack_rows(const void* src /*bf16 [B*S][D]*/, const int32_t* row_map, const int32_t* n_rows, void* dst,
                 int max_rows, int D, mh_stream_t stream);
int mh_unpack_rows(const void* src /*bf16 packed [.][D]*/, const int32_t* inv_map, void* dst /*bf16 [max_rows][D]*/,
                   int max_rows, int D, mh_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Row jobs of the last encoder layer.  The classifier reads ONE row per sample from each tower (the pooled text
 * position, the ViT class token), and behind the last attention every block is row-wise: with these two calls the
 * blocks run on a compact [n][D] panel instead of every token row.
 *   compact row b  <->  full row  idx[b]  (device int32 [n], strictly ASCENDING)  or  b*stride + offset  (idx NULL)
 * mh_rows_gather:       dst[b] = src[row(b)]            src = full [rows][D], dst = compact [n][D]; a row index is
 *                       clamped into [0, rows) before it is used
 * mh_rows_scatter_zero: dst[row(b)] = src[b], every other row of dst[0 .. rows) = 0
 *                       src = compact [n][D], dst = full; rows = min(rows, *rows_dev) when rows_dev is given, rows
 *                       past it are not touched; an index outside [0, rows) writes nothing
 * 16-bit elements, D % 8 == 0, 16-byte aligned buffers.  Up to MH_ROWS_MAX_JOBS jobs (of any D) share one launch.
 * ------------------------------------------------------------------------------------------ */
#define MH_ROWS_MAX_JOBS 8
typedef struct {
    const void* src;
    void* dst;
    const int32_t* idx;        /* device, or NULL */
    const int32_t* rows_dev;   /* device, or NULL (scatter only) */
    int32_t n, rows, D, stride, offset; int32_t reserved_;
} MhRowsJob;
int mh_rows_gather(const MhRowsJob* jobs /*host*/, int n_jobs, mh_stream_t stream);
int mh_rows_scatter_zero(const MhRowsJob* jobs /*host*/, int n_jobs, mh_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * BERT embeddings: x = LN(word[ids] + pos[s] + type[0]) (BertEmbeddings; ids are the Dataset's
 * int64 `text`, Multimodal_example_task2C.txt:63).  type may be NULL (DistilBERT).
 * fwd saves the pre-LN sum (bf16) + mean/rstd for the backward.
 * bwd: d_pre = LN-backward; dword[id] += d_pre rows (deterministic, first-occurrence owner sums
 *      duplicates in position order; rows with id == pad_id get no gradient, as nn.Embedding
 *      padding_idx does); dpos[s] = sum_b ; dtype0 = sum_{b,s}.
 *      dword must be zero on entry except rows this call writes (it overwrites touched rows).
 * ------------------------------------------------------------------------------------------ */
int mh_bert_embed_fwd(const int64_t* ids, const float* word, const float* pos, const float* type0,
                      const float* gamma, const float* beta, void* pre /*bf16 [T][D]*/,
                      void* y /*bf16 [T][D]*/, float* mean, float* rstd, int B, int S, int D, int vocab,
                      float eps, const uint32_t* rng, float drop_p, uint32_t drop_stream /*dropout on y*/,
                      mh_stream_t stream);
int mh_bert_embed_bwd(const int64_t* ids, const void* d_pre /*bf16 [T][D]*/, float* dword /*[V][D]*/,
                      float* dpos /*[P][D]*/, float* dtype0 /*[D] or NULL*/, int B, int S, int D,
                      int vocab, int64_t pad_id, float scale,
                      uint8_t* row_live /*[V] or NULL: set to 1 for every table row that receives a gradient*/,
                      int32_t* first_pos /*[V], all INT32_MAX*/, int32_t* id_count /*[V], all 0*/
                      /* both NULL, or a persistent id index (restored to INT32_MAX / 0 on return): makes the duplicate-id
                         sum linear in the token count instead of quadratic -- the gathered batch of 8 ranks has 32 768 ids */,
                      mh_stream_t stream);
/* Gradient accumulation over micro-batches: mh_bert_embed_bwd with dword[id] += (the row sum, rounded to f32 times scale exactly
 * as mh_bert_embed_bwd stores it) for every row the call touches -- the same first-occurrence owner, the same order, the same
 * pad-row rule; rows it does not touch are left alone.  dpos / dtype0 are OVERWRITTEN as mh_bert_embed_bwd writes them (the caller
 * points them at a scratch and adds that with mh_accum_spans_f32). */
int mh_bert_embed_bwd_accum(const int64_t* ids, const void* d_pre /*bf16 [T][D]*/, float* dword /*[V][D]*/,
                            float* dpos /*[P][D]*/, float* dtype0 /*[D] or NULL*/, int B, int S, int D,
                            int vocab, int64_t pad_id, float scale, uint8_t* row_live, int32_t* first_pos, int32_t* id_count,
                            mh_stream_t stream);
/* RoBERTa-family embeddings (transformers RobertaEmbeddings: roberta-base, xlm-roberta-base): the same sum and LayerNorm with
 * the position row taken from the input ids,
 *     position_id = pad_id + (non-pad ids of the sequence up to and including the token)     for a non-pad token,
 *     position_id = pad_id                                                                    for a pad token,
 * and a position table whose row pad_id gets no gradient (nn.Embedding padding_idx).
 * mh_position_ids_from_input_ids (one wave per sequence, no atomics):
 *   pos_ids int32 [B][S]              the position id of every token
 *   pos_inv int32 [B][max_position]   the position s whose token reads table row p, or -1 (row pad_id: always -1); non-pad
 *                                     position ids ascend strictly, so a row has at most one token per sequence.  Every entry
 *                                     is written.
 *   A position id that would reach max_position (S + pad_id + 1 > max_position: the caller's error) is clamped to the last row
 *   in pos_ids and left out of pos_inv, so no kernel leaves the table.
 * mh_bert_embed_fwd_pos: mh_bert_embed_fwd with the position row pos_ids[t] (clamped into [0, max_position)); same f32
 *   additions in the same order, so a batch without pad tokens and a table shifted by pad_id + 1 rows give the same bits.
 * mh_embed_pos_bwd: dpos[p] = scale * sum_b d_pre[b*S + pos_inv[b][p]] over the b with pos_inv[b][p] >= 0, for EVERY row p of
 *   the table (rows nobody reads are written as zeros), samples summed in the order of mh_bert_embed_bwd's dpos (bitwise
 *   reproducible, and the same bits whenever both sum the same rows).  dtype0 != NULL: additionally dtype0 = scale * sum of
 *   d_pre over every token, pad tokens included (the token-type table has no padding_idx), through scratch (f32 [S][D]) as
 *   mh_bert_embed_bwd computes it.  The word table stays with mh_bert_embed_bwd. */
int mh_position_ids_from_input_ids(const int64_t* ids /*[B][S]*/, int32_t* pos_ids, int32_t* pos_inv, int B, int S, int pad_id,
                                   int max_position, mh_stream_t stream);
int mh_bert_embed_fwd_pos(const int64_t* ids, const float* word, const float* pos /*[max_position][D]*/, const float* type0,
                          const float* gamma, const float* beta, void* pre, void* y, float* mean, float* rstd, int B, int S,
                          int D, int vocab, float eps, const uint32_t* rng, float drop_p, uint32_t drop_stream,
                          const int32_t* pos_ids /*[B][S]*/, int max_position, mh_stream_t stream);
int mh_embed_pos_bwd(const void* d_pre /*bf16 [B*S][D]*/, const int32_t* pos_inv /*[B][max_position]*/,
                     float* dpos /*[max_position][D]*/, float* dtype0 /*[D] or NULL*/, float* scratch /*[S][D], with dtype0*/,
                     int B, int S, int D, int max_position, float scale, mh_stream_t stream);
/* Input pipeline on the device: ToTensor + Normalize of the reference transform
 * (Multimodal_example_task2C.txt:37-41) from decoded / resized / cropped uint8 pixels.
 *   src uint8 [B][H][W][3] (device) -> dst f32 [B][3][H][W] = (src/255 - mean[c]) / std[c]; W % 4 == 0; bit-exact
 *   with torchvision's float32 arithmetic.  mean / std: three host floats each. */
int mh_image_normalize_u8(const uint8_t* src, float* dst, int B, int H, int W, const float* mean3 /*host*/,
                          const float* std3 /*host*/, mh_stream_t stream);
/* The transforms in front of it, on decoded uint8 pixels after ONE host-to-device copy of the batch:
 * mh_image_resample_u8: PIL's antialiased bilinear resize (what torchvision's Resize does to a PIL image) in PIL's own 8-bit
 *   fixed point -- horizontal pass into a uint8 image, then the vertical pass; the host supplies, per image and output
 *   pixel, the source window {first, count} and the 22-bit integer coefficients (data.pil_resample_coeffs: PIL's
 *   precompute_coeffs / normalize_coeffs_8bpc), so the output equals PIL's bit for bit.  Only the output window asked for
 *   (the centre crop) is computed; `flip` (uint8 [B] or NULL) mirrors the output (RandomHorizontalFlip).  `vfirst` (uint8 [B] or
 *   NULL): images that take the vertical pass first, as Pillow's Image.resize does for a source with h > 100 w whose height shrinks
 *   (data.pil_resize_vertical_first); the 8-bit intermediate image makes the two orders differ by one grey level.
 *     arena: the batch's images back to back, uint8 [h][w][3] each at src_off[b]; hw int32 [B][2];
 *     xbounds / ybounds int32 [B][OW|OH][2]; xcoef / ycoef int32 [B][OW|OH][KX|KY];
 *     tmp uint8 [B][max(max_h * OW, OH * max_w)][3]: per image [h][OW] (horizontal first) or [OH][w] (vertical first); max_h >= every
 *     h, max_w >= the w of every vertical-first image (not read when vfirst is NULL); out uint8 [B][OH][OW][3].
 * mh_image_jitter_rotate_u8: ColorJitter (brightness / contrast / saturation / hue factors, per-image op order packed 2 bits
 *   per step: 0 brightness, 1 contrast, 2 saturation, 3 hue) with PIL's arithmetic on uint8 -- ImageEnhance = ImagingBlend in
 *   float32 (product and sum rounded separately), the hue op = Pillow's 8-bit RGB -> HSV -> RGB round trip with the H band shifted
 *   modulo 256 (torchvision adjust_hue on a PIL image) -- then RandomRotation = Image.rotate(angle, NEAREST, expand=False, fill 0)
 *   walked in 16.16 fixed point as libImaging's affine_fixed does.  Bit-exact against PIL (tests).  params: device array of 16
 *   32-bit words per image {f32 brightness, contrast, saturation; i32 hue (0 = no hue op, else 0x100 | uint8(hue_factor * 255));
 *   i32 order; i32 rotate (0 = angle 0); i32 a[6] (the fixed-point inverse map, data.pil_rotate_fixed_coeffs); 4 x pad};
 *   lsum: device u64 [B] workspace (L-image sums for the contrast mean).  (Multimodal_example_task2C.py:222-235.)  The random
 *   factors are drawn on the host. */
int mh_image_resample_u8(const uint8_t* arena, const int64_t* src_off, const int32_t* hw, const int32_t* xbounds,
                         const int32_t* xcoef, int KX, const int32_t* ybounds, const int32_t* ycoef, int KY, const uint8_t* flip,
                         const uint8_t* vfirst, uint8_t* tmp, uint8_t* out, int B, int max_h, int max_w, int OH, int OW,
                         mh_stream_t stream);
int mh_image_luma_sum_u8(const uint8_t* img, unsigned long long* sums, int B, int HW, mh_stream_t stream);
int mh_image_jitter_rotate_u8(const uint8_t* in, uint8_t* scratch, uint8_t* out, const void* params, unsigned long long* lsum,
                              int B, int H, int W, mh_stream_t stream);
/* The grayscale path (ResNet_example_task2B.py:158-167: convert("L") -> Resize -> CenterCrop -> ToTensor -> Normalize(mean=[0.45],
 * std=[0.22])): the L conversion runs on the SOURCE, at its own size, before the resize -- converting after an RGB resize gives other
 * pixels.  Same arena as mh_image_resample_u8.
 * mh_image_luma_u8: Pillow's RGB -> L (Convert.c rgb2l), L = (R*19595 + G*38470 + B*7471 + 0x8000) >> 16, of every image of the
 *   packed arena.  src_off[b] is a multiple of 3 (the images are whole RGB pixels back to back): the L image of b is written as
 *   uint8 [h][w] at gray + src_off[b] / 3, so gray needs (arena bytes) / 3 bytes.  max_hw >= h * w of every image.
 * mh_image_resample_l_u8: mh_image_resample_u8 on that one band -- the same windows, coefficients, pass order (`vfirst`), rounding and
 *   `flip`, src_off STILL the arena's RGB byte offsets (the image is read at gray + src_off[b] / 3);
 *   tmp uint8 [B][max(max_h * OW, OH * max_w)], out uint8 [B][OH][OW] (= [B][OH][OW][1]).
 * mh_image_normalize_l_u8: src uint8 [B][H][W] -> dst f32 [B][1][H][W] = (src/255 - mean) / std in torchvision's float32 arithmetic
 *   (bit-exact); n = B*H*W elements, src 4-byte and dst 16-byte aligned. */
int mh_image_luma_u8(const uint8_t* arena, const int64_t* src_off, const int32_t* hw, uint8_t* gray, int B, int max_hw,
                     mh_stream_t stream);
int mh_image_resample_l_u8(const uint8_t* gray, const int64_t* src_off, const int32_t* hw, const int32_t* xbounds,
                           const int32_t* xcoef, int KX, const int32_t* ybounds, const int32_t* ycoef, int KY, const uint8_t* flip,
                           const uint8_t* vfirst, uint8_t* tmp, uint8_t* out, int B, int max_h, int max_w, int OH, int OW,
                           mh_stream_t stream);
int mh_image_normalize_l_u8(const uint8_t* src, float* dst, int64_t n, float mean, float std, mh_stream_t stream);
/* The windows and coefficients mh_image_resample_u8 / _l_u8 read, made on the device instead of by the host (the host then sends
 * eight integers per image): Pillow's libImaging/Resample.c precompute_coeffs + normalize_coeffs_8bpc in float64, for the bilinear
 * filter (support 1) and Pillow's bicubic (a = -0.5, support 2) -- what BlipImageProcessor and CLIPImageProcessor resize with.  One
 * thread per (image, axis, output pixel) sums its window's weights one after the other, as Pillow does, and writes
 * int(+-0.5 + (w / sum) * 2^22); no product is fused with the sum behind it, so the tables equal data.pil_filter_coeffs -- and
 * Pillow's -- integer for integer.
 * mh_image_resample_ksize (host only): the window length ImagingResample allocates for a resize in_size -> out_size,
 *   ceil(support * max(in_size / out_size, 1)) * 2 + 1; 0 for a size < 1 or an unknown filter.
 * mh_image_resample_tables: spec: device int32 [B][8] = {in_w, in_h, resized_w, resized_h, first_x, first_y, 0, 0}; writes
 *   xbounds [B][OW][2], xcoef [B][OW][KX], ybounds [B][OH][2], ycoef [B][OH][KY] exactly as data.pil_filter_coeffs(in, resized, first,
 *   OW | OH, filter): output pixels first .. first + OW|OH - 1 of the resize in -> resized (first > 0: a centre crop's window).  Every
 *   entry of a coefficient row is written, zeros behind the window.  KX / KY >= the image's mh_image_resample_ksize; a window longer
 *   than K is the caller's error: the row keeps its first K taps (still divided by the whole window's sum), bounds[..][1] = K, and
 *   nothing outside the row is written.  An image whose spec holds a size < 1 gets empty windows.  One launch for both axes and the
 *   whole batch, on `stream` ahead of the resample.  MH_EINVAL: a NULL pointer; MH_ESHAPE: B / OH / OW / KX / KY < 1, B > 65535, an
 *   unknown filter. */
#define MH_FILTER_BILINEAR 0
#define MH_FILTER_BICUBIC 1
int mh_image_resample_ksize(int in_size, int out_size, int filter);
int mh_image_resample_tables(const int32_t* spec, int filter, int32_t* xbounds, int32_t* xcoef, int KX, int32_t* ybounds,
                             int32_t* ycoef, int KY, int B, int OH, int OW, mh_stream_t stream);
/* Dropout helpers.  mh_dropout_apply: x[i] *= mask(i)/(1-p) in place (16-bit), e.g. the gradient arriving at a
 * dropped activation.  mh_dropout_mask_u8: the 0/1 mask a site would use for element indices 0..n-1 (tests). */
int mh_dropout_apply(void* x, int64_t n, const uint32_t* rng, float p, uint32_t stream_id, mh_stream_t stream);
int mh_dropout_mask_u8(uint8_t* out, int64_t n, const uint32_t* rng, float p, uint32_t stream_id,
                       mh_stream_t stream);
/* zero the rows of dword named by ids (cheap re-zero of the dense table after the optimizer step) */
int mh_zero_rows_f32(const int64_t* ids, float* table, int n_ids, int D, int vocab, mh_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * ViT patch embedding (timm PatchEmbed conv 16x16/s16 == im2col + GEMM):
 *   mh_patchify: image f32 [B][C][H][W] -> patches bf16 [B*gh*gw][C*p*p], feature order (c,i,j),
 *                patch order row-major over (h,w)  (bit-exact cast-free gather, then RNE to bf16)
 *   mh_vit_assemble_fwd: x[b][0] = cls + pos[0]; x[b][1+p] = proj[b][p] + pos[1+p]   (bf16 out)
 *   mh_vit_assemble_bwd: dproj[b][p] = dx[b][1+p] (bf16); dpos[t] = sum_b dx[b][t]; dcls = sum_b dx[b][0]
 * ------------------------------------------------------------------------------------------ */
int mh_patchify(const float* image, void* patches, int B, int C, int H, int W, int P, mh_stream_t stream);
/* Generic patch gather: any patch size (CLIP ViT-L/14: 14), row pitch ld >= C*P*P elements; the columns C*P*P .. ld-1
 * are zero-filled, so the patch-projection GEMM can run with its contraction padded to a multiple of 64 (588 -> 640).
 * Same patch / feature order as mh_patchify; bit-exact gather + RNE. */
int mh_patchify_ld(const float* image, void* patches /*bf16 [B*gh*gw][ld]*/, int B, int C, int H, int W, int P, int ld,
                   mh_stream_t stream);
/* 2-D copy of 32-bit words with zero padding: dst[r][c] = c < cols ? src[r][c] : 0 for c < pad_to (ld_* in words).
 * Pads the [D][C*P*P] patch-projection weight (two 16-bit elements per word) to the GEMM's K, and un-pads its
 * f32 gradient. */
int mh_copy2d_u32(const void* src, int ld_src, void* dst, int ld_dst, int rows, int cols, int pad_to, mh_stream_t stream);
int mh_vit_assemble_fwd(const void* proj /*bf16 [B*Np][D]*/, const float* cls, const float* pos,
                        void* x /*bf16 [B][Np+1][D]*/, int B, int Np, int D, mh_stream_t stream);
int mh_vit_assemble_bwd(const void* dx /*bf16 [B][Np+1][D]*/, void* dproj /*bf16 [B*Np][D]*/,
                        float* dcls, float* dpos, int B, int Np, int D, float scale, mh_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Late-fusion head + cross-entropy, fp32 (Multimodal_example_task2C.txt:178-195, :248, :214):
 *   t = W_t h_t[:, pool] + b ; v = W_i h_i[:, 0] + b ; f = W_f [t;v] + b ; z = W_o f + b
 *   loss = mean_b( logsumexp(z_b) - z_b[y_b] )
 * The towers' final LayerNorm outputs are consumed UNROUNDED (f32) so the head adds no bf16 error.
 * mh_head_fwd writes logits [B][C] and keeps pooled, t|v (feat [B][2P]) and f ([B][P]).
 * mh_head_bwd consumes dlogits [B][C] (f32) and produces all head grads (f32, overwritten) and
 *   d_text_hidden / d_image_hidden rows (bf16, written into the [T][D] gradient buffers at the
 *   pooled token rows; the other rows must be zero-filled by the caller).
 * mh_ce_fwd_bwd: loss (scalar f32), dlogits = (softmax - onehot)/B, n_correct (argmax == label, first maximum wins).
 *   A label outside [0, C) -- nn.CrossEntropyLoss's ignore_index -100 included -- is read as class 0 (it is NOT ignored:
 *   the loss, dlogits and n_correct are those of label 0, and the mean stays over all B rows).  mh_ce_opts_fwd_bwd below
 *   ignores a label on request.
 * ------------------------------------------------------------------------------------------ */
typedef struct MhHeadParams {
    const float *Wt, *bt;   /* bert_fc   [P][Dt], [P] */
    const float *Wi, *bi;   /* image_fc  [P][Di], [P] */
    const float *Wf, *bf_;  /* fusion_fc [P][2P], [P] */
    const float *Wo, *bo;   /* output_fc [C][P],  [C] */
} MhHeadParams;
typedef struct MhHeadGrads {
    float *Wt, *bt, *Wi, *bi, *Wf, *bf_, *Wo, *bo;
} MhHeadGrads;

int mh_head_fwd(const MhHeadParams* p /*host*/, const float* text_hidden /*f32 [B][S][Dt]*/,
                const float* image_hidden /*f32 [B][Nt][Di]*/, int text_pool_index, float* pooled
                /*[B][Dt+Di] f32*/, float* feat /*[B][2P]*/, float* fused /*[B][P]*/,
                float* logits /*[B][C]*/, int B, int S, int Nt, int Dt, int Di, int P, int C,
                const uint32_t* rng, float drop_p, uint32_t drop_stream /*nn.Dropout(0.3) on the pooled text row,
                Multimodal_example_task2C.txt:160,178; mask index b*Dt + d*/,
                const int32_t* text_rows /*NULL, or device int32 [B]: row of text_hidden pooled for sample b (packed
                text tower) instead of b*S + text_pool_index*/, mh_stream_t stream);
int mh_head_bwd(const MhHeadParams* p /*host*/, const MhHeadGrads* g /*host*/, const float* dlogits,
                const float* pooled, const float* feat, const float* fused, float* dfeat /*[B][2P]*/,
                float* dfused /*[B][P]*/, void* d_text_hidden /*bf16 [B][S][Dt]*/,
                void* d_image_hidden /*bf16 [B][Nt][Di]*/, int text_pool_index, int B, int S, int Nt,
                int Dt, int Di, int P, int C, float out_scale, const uint32_t* rng, float drop_p,
                uint32_t drop_stream, const int32_t* text_rows /*as in mh_head_fwd*/, mh_stream_t stream);
/* The pooling stage on its own, for heads built outside this library (Kevin's Linear+BatchNorm1d+ReLU projections,
 * ConcatAttention3, the SVM baseline's feature dump: Multimodal_example_task2C.py:590-641, baselines/extract_feat.py):
 *   mh_pool_fwd: pooled[b] = [ text_hidden[b][pool or text_rows[b]] , image_hidden[b][0] ]  (f32 [B][Dt+Di])
 *   mh_pool_bwd: the reverse scatter of d_pooled into the 16-bit hidden-state gradient buffers (times out_scale);
 *                all other rows must be zero-filled by the caller. */
int mh_pool_fwd(const float* text_hidden, const float* image_hidden, int text_pool_index, float* pooled, int B, int S,
                int Nt, int Dt, int Di, const int32_t* text_rows, mh_stream_t stream);
int mh_pool_bwd(const float* d_pooled, void* d_text_hidden, void* d_image_hidden, int text_pool_index, int B, int S,
                int Nt, int Dt, int Di, float out_scale, const int32_t* text_rows, mh_stream_t stream);
/* BatchNorm1d over f32 [B][F] (+ optional fused ReLU): Kevin's `Linear + BatchNorm1d + ReLU` projections and the 1-logit
 * `Linear(512,1) + BatchNorm1d(1)` (Multimodal_example_task2C.py:603-605, :641-643).  Training: batch statistics
 * (biased variance), running statistics updated with momentum (unbiased variance), mean / rstd saved for the
 * backward.  Eval (training = 0): running statistics (also written to save_mean / save_rstd).  bwd: dx, dgamma, dbeta
 * (overwritten); `relu` is a bit set: MH_BN_RELU -- y (the forward output) masks the incoming gradient; MH_BN_FROZEN_STATS --
 * the forward ran in eval mode, the statistics are constants and dx = gamma rstd dy' (the reference's train() goes on
 * training in eval mode after its mid-epoch test(), Multimodal_example_task2C.py:755-780).  B <= 1024. */
#define MH_BN_RELU 1
#define MH_BN_FROZEN_STATS 2
int mh_bn1d_fwd(const float* x, int ldx, const float* gamma, const float* beta, float* running_mean, float* running_var,
                float* y, int ldy, float* save_mean, float* save_rstd, int B, int F, float eps, float momentum,
                int training, int relu, mh_stream_t stream);
int mh_bn1d_bwd(const float* dy, int lddy, const float* x, int ldx, const float* y, int ldy, const float* gamma,
                const float* save_mean, const float* save_rstd, float* dx, int lddx, float* dgamma, float* dbeta, int B,
                int F, int relu, mh_stream_t stream);
/* Row L2 normalisation (BinaryHead's l2_norm, example_scripts/Untitled-2.py:164-167): y[b][:] = x[b][:] / ||x[b]||_2 (no eps, as
 * the reference), norm[b] = ||x[b]||_2;  bwd: dx = (g - xhat (xhat . g)) / norm with xhat = the forward's y.  f32 [B][D], B <= 65535. */
int mh_l2norm_fwd(const float* x, float* y, float* norm, int B, int D, mh_stream_t stream);
int mh_l2norm_bwd(const float* g, const float* xhat, const float* norm, float* dx, int B, int D, mh_stream_t stream);
int mh_ce_fwd_bwd(const float* logits, const int64_t* labels, float* loss, float* dlogits,
                  int32_t* n_correct, int B, int C, float grad_scale,
                  const float* grad_scale_dev /*device f32[1] or NULL: the dynamic loss scale, multiplied into grad_scale*/,
                  mh_stream_t stream);
/* sigmoid focal loss over one logit per sample (torchvision.ops.sigmoid_focal_loss(inputs, targets, alpha, gamma,
 * reduction="mean") as called at Multimodal_example_task2C.py:167,711): loss, dlogits (stride ld), #(logit>0 == target).
 * alpha < 0 disables the class weighting, as in torchvision. */
int mh_focal_fwd_bwd(const float* logits, int ld, const float* targets /*f32 [B] in {0,1}*/, float* loss,
                     float* dlogits, int32_t* n_correct, int B, float alpha, float gamma, float grad_scale,
                     const float* grad_scale_dev /*as in mh_ce_fwd_bwd*/, mh_stream_t stream);
/* Cross-entropy with the arguments of torch.nn.functional.cross_entropy(weight=, ignore_index=, label_smoothing=, reduction=)
 * (nn.CrossEntropyLoss(weight=class_weights), Multimodal_example_task2C.py:166).  One workgroup, one thread per row, B <= 1024.
 *   w_c = class_weight[c] (1 when class_weight is NULL); k_i = 0 when has_ignore != 0 and y_i == ignore_index, else 1;
 *   l_i = k_i [ (1 - eps) w_{y_i} (lse_i - z_{i,y_i}) + (eps / C) sum_c w_c (lse_i - z_{i,c}) ],  eps = label_smoothing
 *   reduction MH_LOSS_MEAN: loss[0] = sum_i l_i / sum_i k_i w_{y_i} ; MH_LOSS_SUM: loss[0] = sum_i l_i ;
 *   MH_LOSS_NONE: loss[i] = l_i (B values) and dlogits holds the derivative of each row's OWN loss (the caller multiplies the
 *   upstream gradient in per row).
 * dlogits [B][C] = the exact derivative of the above times grad_scale * grad_scale_dev[0]; every element is written, an
 * ignored row as +0.0.  n_correct counts kept rows only (first maximum wins).  All rows ignored under MH_LOSS_MEAN: the loss
 * is NaN (0 / 0, as in torch), dlogits all zero, n_correct 0.  A label outside [0, C) that is not the ignore index is read as
 * class 0 (as in mh_ce_fwd_bwd).  MH_ESHAPE: label_smoothing outside [0, 1], an unknown reduction.
 * With class_weight NULL, label_smoothing 0, no ignored row and MH_LOSS_MEAN the result equals mh_ce_fwd_bwd's bit for bit. */
#define MH_LOSS_MEAN 0
#define MH_LOSS_SUM 1
#define MH_LOSS_NONE 2
int mh_ce_opts_fwd_bwd(const float* logits, const int64_t* labels, const float* class_weight /*device f32 [C] or NULL*/,
                       float* loss /*[1], or [B] with MH_LOSS_NONE*/, float* dlogits, int32_t* n_correct, int B, int C,
                       int64_t ignore_index, int has_ignore, float label_smoothing, int reduction, float grad_scale,
                       const float* grad_scale_dev /*as in mh_ce_fwd_bwd*/, mh_stream_t stream);
/* Binary cross-entropy with logits over one logit per sample (F.binary_cross_entropy_with_logits(x, t, pos_weight=)):
 *   l = (1 - t) softplus(x) + pos_weight t softplus(-x) ; loss = mean (MH_LOSS_MEAN) or sum (MH_LOSS_SUM) over the B rows;
 * dlogits (stride ld) and n_correct = #(logit > 0 == target > 0.5) as in mh_focal_fwd_bwd.  pos_weight = 1: none. */
int mh_bce_fwd_bwd(const float* logits, int ld, const float* targets /*f32 [B], soft targets allowed*/, float pos_weight,
                   float* loss, float* dlogits, int32_t* n_correct, int B, int reduction, float grad_scale,
                   const float* grad_scale_dev /*as in mh_ce_fwd_bwd*/, mh_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Heads on top of the towers (SURVEY section 8 f ranks 1-2), all fp32:
 *   Kevin's `Linear + BatchNorm1d + ReLU` projections, `ConcatAttention3`, `Linear(512,1) + BatchNorm1d(1)`
 *   (Multimodal_example_task2C.py:599-612, 476-499, 641-643) and the pooling branches of LLMWithClassificationHead
 *   (Multimodal_example_task2C.py:362-392, DistilBERT_example_task2A.py:185-210).
 *
 * mh_gemm_f32: C[M][N] = act(A . B^T + bias) in EXACT f32 on v_mfma_f32_32x32x2_f32 (an fmaf chain per element: the
 *   head adds no 16-bit rounding), any M / N / K, operand layouts as in mh_gemm_bf16_grouped (a_kmajor / b_kmajor).
 *   flags: MH_F32_ACCUM (C += ...), MH_F32_TANH, MH_F32_RELU, MH_F32_BN.
 *   MH_F32_BN (M <= 64, one row tile = the whole batch): nn.Linear -> nn.BatchNorm1d (-> ReLU with MH_F32_RELU) in ONE
 *   launch: z = A B^T + bias is kept in bn_z (for the backward), training mode normalises with the batch statistics
 *   (biased variance), saves mean / rstd and updates the running statistics (unbiased variance, momentum) exactly as
 *   mh_bn1d_fwd does; eval mode uses the running statistics.
 *   B = 1 (M = 1) in training mode is accepted, where nn.BatchNorm1d raises: the batch variance is 0, so the output is
 *   beta (ReLU'd), and the running variance takes the biased variance 0 in place of the undefined unbiased one.
 * ------------------------------------------------------------------------------------------ */
#define MH_F32_ACCUM 1
#define MH_F32_TANH 2
#define MH_F32_RELU 4
#define MH_F32_BN 8
typedef struct MhGemmF32 {
    const float* A; const float* B; float* C; const float* bias /*[N] or NULL*/;
    int32_t M, N, K, lda, ldb, ldc, flags;
    const float* bn_gamma; const float* bn_beta; float* bn_running_mean; float* bn_running_var;
    float* bn_save_mean; float* bn_save_rstd; float* bn_z /*[M][bn_ldz] pre-BatchNorm output or NULL*/;
    int32_t bn_ldz; float bn_eps; float bn_momentum; int32_t bn_training;
} MhGemmF32;
int mh_gemm_f32(const MhGemmF32* p /*host*/, int a_kmajor, int b_kmajor, mh_stream_t stream);
/* out[d] = scale * sum_r x[r][d] (bias gradients; fixed summation order) */
int mh_colsum_f32(const float* x, int ld, float* out, int rows, int D, float scale, mh_stream_t stream);
/* Sequence poolings over the last hidden state h f32 [B][S][D]:
 *   max   : out[b][d] = max_s h ; arg = the first maximising s (a NaN propagates as in torch.max: the first NaN along s
 *           wins) ; bwd writes dh (all of it) from dout and arg
 *   mean  : out = sum_s h m / clamp(sum_s m, 1e-9) with the int64 attention mask m [B][S]
 *   attn  : u = tanh(h W1^T + b1) comes from mh_gemm_f32(MH_F32_TANH); scores = u . w2 + b2 + (1 - m) * -1e9;
 *           p = softmax_s (saved [B][S]); out = sum_s p h.  bwd: du [B][S][A] (feed the two GEMMs for dW1 / dh),
 *           dh = p dout (the direct path; the GEMM adds du W1 with MH_F32_ACCUM), per-sample partials dw2_part [B][A],
 *           db2_part [B] (finish with mh_colsum_f32).  S <= 1024.
 *   cnn   : conv1d(D -> D, `taps` taps, same padding) + ReLU + max over positions, as a GEMM over zero-padded
 *           sequences: mh_pad_seq_f32 builds hp [B][Sp = S + taps - 1][D]; z = mh_gemm_f32(A = hp viewed with lda = D,
 *           K = taps * D, M = B*Sp - (taps-1), B = weight permuted to [O][taps][C]); mh_relu_max_fwd reduces the S valid
 *           rows of each sample (arg = -1 when the ReLU floor wins); bwd: mh_relu_max_bwd scatters dout into dz,
 *           two GEMMs give dW and da = dz W, mh_conv_fold_f32 sums the taps back into dh. */
int mh_pool_max_fwd(const float* h, float* out, int32_t* arg, int B, int S, int D, mh_stream_t stream);
int mh_pool_max_bwd(const float* dout, const int32_t* arg, float* dh, int B, int S, int D, mh_stream_t stream);
int mh_pool_mean_fwd(const float* h, const int64_t* mask, float* out, int B, int S, int D, mh_stream_t stream);
int mh_pool_mean_bwd(const float* dout, const int64_t* mask, float* dh, int B, int S, int D, mh_stream_t stream);
int mh_pool_attn_fwd(const float* h, const float* u, const float* w2, const float* b2, const int64_t* mask, float* p,
                     float* out, int B, int S, int D, int A, mh_stream_t stream);
int mh_pool_attn_bwd(const float* h, const float* u, const float* w2, const float* p, const float* dout, float* du, float* dh,
                     float* dw2_part, float* db2_part, int B, int S, int D, int A, mh_stream_t stream);
int mh_pad_seq_f32(const float* h, float* hp, int B, int S, int D, int pad, int Sp, mh_stream_t stream);
int mh_relu_max_fwd(const float* z, float* out, int32_t* arg, int B, int S, int Sp, int D, mh_stream_t stream);
int mh_relu_max_bwd(const float* dout, const int32_t* arg, float* dz, int rows, int Sp, int D, mh_stream_t stream);
int mh_conv_fold_f32(const float* da, float* dh, int B, int S, int D, int taps, int pad, int Sp, int rows, mh_stream_t stream);
/* ConcatAttention3's gate (Multimodal_example_task2C.py:495-496): y = softmax(g, dim=1) * c ; bwd: dg, dc from dy */
int mh_softmax_gate_fwd(const float* g, const float* c, float* y, int B, int F, mh_stream_t stream);
int mh_softmax_gate_bwd(const float* g, const float* c, const float* dy, float* dg, float* dc, int B, int F, mh_stream_t stream);

/* MCA3, the reference's fusion_method = "mca" (Multimodal_example_task2C.py:423-448), on 2-D features as its forward feeds it:
 * pa = W1 text + b1, pc = W3 caption + b3, pi = W2 image + b2 (all [B][U], computed by mh_gemm_f32);
 * score[i][j] = tanh(pa[j] + pc[j] + pi[i]) (the reference's [B,1,U] broadcast), e = V . score + bv, w[i][:] = softmax_j,
 * ctx[i] = [sum_j w[i][j] text[j] | sum_j w[i][j] caption[j]]  ([B][2U], the input of its `reduce` Linear).  B <= 1024.
 * bwd: from dctx: dpa (= dpc), dpi, dtext / dcaption (the direct paths), per-row partials dV_part [B][U] and dbv_part [B]
 * (summed by mh_colsum_f32); de_ws: workspace [B][B]. */
int mh_mca3_fwd(const float* pa, const float* pc, const float* pi, const float* Vw, const float* bv, const float* text,
                const float* caption, float* w, float* ctx, int B, int U, mh_stream_t stream);
int mh_mca3_bwd(const float* pa, const float* pc, const float* pi, const float* Vw, const float* text, const float* caption,
                const float* w, const float* dctx, float* de_ws, float* dpa, float* dpi, float* dtext, float* dcaption,
                float* dV_part, float* dbv_part, int B, int U, mh_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Conv tower (BASELINE config 2: torchvision ResNet-50 as wired at Multimodal_example_task2C.txt:164-165,183-184).
 * Activations are NHWC 16-bit = a row-major [B*H*W][C] matrix, so a convolution is mh_gemm_bf16_grouped:
 *   1x1 / stride 1 : directly on the activation matrix;  k x k or strided: on the mh_im2col_nhwc matrix
 *   (column order (kh, kw, c); weights packed to [Cout][(kh,kw,c)] by mh_conv_weight_pack);
 *   dgrad = the GEMM in the dgrad layout followed by mh_col2im_nhwc (gather form, no atomics);
 *   wgrad = the GEMM in the wgrad layout over the im2col matrix, un-packed by mh_conv_weight_unpack.
 * mh_bn2d_fwd / mh_bn2d_bwd: nn.BatchNorm2d over that matrix (M = B*H*W rows), training mode = per-replica batch
 *   statistics (biased variance for the normalisation, unbiased for the running statistics, momentum form), optional fused
 *   residual add and ReLU: y = relu(bn(x) + residual).  workspace: f32, >= mh_bn2d_workspace_elems(M, C) elements (the
 *   statistics are per-block partial sums; the rows per block shrink with M so that deep, narrow-M layers still fill the chip).
 *   bwd: dx, the residual-branch gradient dres (= dy masked by the ReLU), dgamma, dbeta (times `scale`).
 * mh_maxpool_* (k x k / stride / pad, first maximum wins, arg = tap index), mh_avgpool_* (global), mh_nchw_to_nhwc (f32 image
 * -> 16-bit NHWC with the channels zero-padded to Cp), mh_add_h16.
 * ------------------------------------------------------------------------------------------ */
int mh_nchw_to_nhwc(const float* x, void* y, int B, int C, int H, int W, int Cp, mh_stream_t stream);
int mh_im2col_nhwc(const void* x, void* col, int B, int H, int W, int C, int KH, int KW, int stride, int pad, int ldc,
                   mh_stream_t stream);
int mh_col2im_nhwc(const void* dcol, void* dx, int B, int H, int W, int C, int KH, int KW, int stride, int pad, int ldc,
                   mh_stream_t stream);
int mh_conv_weight_pack(const float* w /*[Cout][Cin][KH][KW]*/, void* out /*16-bit [Cout][ldk]*/, int Cout, int Cin, int KH, int KW,
                        int Cp, int ldk, mh_stream_t stream);
int mh_conv_weight_unpack(const float* gk /*[Cout][ldk]*/, float* g /*[Cout][Cin][KH][KW]*/, int Cout, int Cin, int KH, int KW, int Cp,
                          int ldk, float scale, mh_stream_t stream);
/* Every convolution of a tower in one launch (a ResNet-50 step has 53 weight packs and 53 weight-gradient finishes; at 5 us
 * of work each the launch latency is what they cost).  block_start is filled in by the library.
 * mh_conv_wgrad_finish_batched: g[Cout][Cin][KH][KW] (+)= scale * sum_s slabs[s][Cout][ldk] -- the fixed-order sum of the
 * split-K slabs of the weight-gradient GEMM (nsplit = 1: its plain f32 output) un-packed to the torch layout, optionally
 * accumulated into an existing .grad (autograd's accumulate semantics without a separate add launch per parameter). */
#define MH_CONV_MAX_JOBS 64
typedef struct MhConvPackJob {
    const float* w;   /* [Cout][Cin][KH][KW] f32 */
    void* out;        /* 16-bit [Cout][ldk] */
    int32_t Cout, Cin, KH, KW, Cp, ldk;
    int32_t block_start, reserved_;
} MhConvPackJob;
typedef struct MhConvWgradJob {
    const float* slabs;   /* [nsplit][Cout][ldk] f32 */
    float* g;             /* [Cout][Cin][KH][KW] f32 */
    int32_t Cout, Cin, KH, KW, Cp, ldk;
    int32_t nsplit, accumulate;
    float scale;
    int32_t block_start;
} MhConvWgradJob;
int mh_conv_weight_pack_batched(const MhConvPackJob* jobs, int n, mh_stream_t stream);
int mh_conv_wgrad_finish_batched(const MhConvWgradJob* jobs, int n, mh_stream_t stream);
int64_t mh_bn2d_workspace_elems(int M, int C);
/* mh_bn2d_bwd flags */
#define MH_BN_RELU 1
#define MH_BN_ACCUM_PARAM_GRADS 2   /* dgamma / dbeta are added to, not overwritten */
int mh_bn2d_fwd(const void* x, const float* gamma, const float* beta, float* running_mean, float* running_var, const void* residual,
                void* y, float* save_mean, float* save_rstd, float* workspace, int M, int C, float eps, float momentum, int training,
                int relu, mh_stream_t stream);
int mh_bn2d_apply(const void* x, const float* mean, const float* rstd, const float* gamma, const float* beta, const void* residual,
                  void* y, int M, int C, int relu, mh_stream_t stream);
/* y: the forward output (the ReLU mask is y > 0), or NULL with MH_BN_RELU when the forward had NO residual: the mask is then
 * recomputed from x as the forward computed y (16-bit rounding of (x - mean) rstd gamma + beta > 0), one tensor less to read */
int mh_bn2d_bwd(const void* dy, const void* x, const void* y, const float* gamma, const float* beta, const float* save_mean,
                const float* save_rstd, void* dx, void* dres, float* dgamma, float* dbeta, float* workspace, int M, int C,
                int flags /* MH_BN_* */, float scale, mh_stream_t stream);
/* ---- implicit GEMM (convgemm.hip): the same convolutions with NO im2col panel in HBM.  The panel exists only as addresses:
 * every 16-byte LDS-DMA chunk of the MFMA tile's operand is fetched from (pixel, tap, 8 channels) of the NHWC tensor, taps in
 * the padding read as zeros through the buffer bounds.  Weights are the packed [Cout][ldk] of mh_conv_weight_pack.
 *   mh_conv_fwd   y[B*Ho*Wo][Cout] = conv(x[B][H][W][C]); any KH x KW / stride / pad, C % 8 == 0 (C % 64 == 0 and
 *                 ldk == KH*KW*C take the wave-uniform tap walk).  bn_part (or NULL): f32 [2][Cout][ceil(B*Ho*Wo / 128)] -- per
 *                 128-row tile the column sums of y and y^2 (of the 16-bit values as stored), the layout mh_bn2d_fwd_parts reads:
 *                 train-mode BatchNorm2d (Multimodal_example_task2C.txt:164 resnet50) then needs no statistics pass.
 *   mh_conv_dgrad dx[B*H*W][C] = the input gradient from dy[B*Ho*Wo][Cout]; KH == KW, Cout % 64 == 0; stride 1, or stride 2 with
 *                 KH > 1 on an even H x W image -- then the four parity classes of input pixels (each meets only every second filter
 *                 tap) run as four stride-1 problems of ONE launch, scattered into every second row / column of dx, and a `bn`
 *                 part buffer holds 4 * ceil(B*(H/2)*(W/2) / 128) partial columns.  Other strided shapes return MH_ESHAPE and keep
 *                 the explicit dgrad GEMM + mh_col2im_nhwc (1x1 / stride 2: three of the four classes have no tap).
 *   mh_conv_wgrad slabs[ksplit][Cout][ldk] (f32) = alpha * dy^T im2col(x), the contraction over B*Ho*Wo pixels cut into
 *                 `ksplit` chunks (mh_gemm_ksplit_for(B*Ho*Wo, want)); mh_conv_wgrad_finish_batched sums the slabs.
 * Limits: every tensor < 2 GiB, B*H*W and B*Ho*Wo < 2^24. */
typedef struct MhConvGeom {
    int32_t B, H, W, C;            /* input NHWC (C = channels of the activation matrix, a multiple of 8) */
    int32_t KH, KW, stride, pad;
    int32_t Cout, ldk;             /* filters; row pitch of the packed weights (multiple of 64, >= KH*KW*C) */
} MhConvGeom;
/* workspace (forward, dgrad): NULL, or f32 [mh_conv_splitk(g, dgrad)][rows][columns] of the OUTPUT (rows x columns = B*Ho*Wo x Cout
 * forward, B*H*W x C dgrad).  With it, a convolution whose tile count leaves most CUs idle and whose contraction is long (ResNet-50's
 * last two stages at batch 32: 52-98 tiles of 32-72 K steps) is cut into that many K chunks -- f32 slabs summed in slab order by a
 * finishing launch that also rounds, stores and leaves the BatchNorm partials.  mh_conv_splitk returns 1 when no split is taken. */
int mh_conv_splitk(const MhConvGeom* g, int dgrad);
int mh_conv_fwd(const void* x, const void* wk, void* y, float* bn_part, float* workspace, const MhConvGeom* g, mh_stream_t stream);
/* bn (dgrad, or NULL): the BatchNorm2d (+ReLU, no residual) whose OUTPUT is this convolution's input.  dx is then that BatchNorm's
 * dy: the epilogue masks it by the ReLU (recomputed from z as the forward computed it), stores the MASKED gradient and leaves the
 * per-128-row-tile column sums part[2][C][ceil(B*H*W / 128)] = sum g', sum g' xhat -- the BatchNorm backward's statistics pass
 * over (dy, z) disappears: mh_bn2d_bwd_parts(dx, ...) finishes the sums and applies. */
typedef struct MhConvBnBwd {
    const void* z;                               /* 16-bit [B*H*W][C]: the BatchNorm's input */
    const float *mean, *rstd, *gamma, *beta;     /* f32 [C] */
    float* part;                                 /* f32 [2][C][ceil(B*H*W / 128)] */
    int32_t relu, reserved_;
    /* round 4: the gradient of a residual block's OUTPUT in the same epilogue.  `addend` (16-bit [B*H*W][C] or NULL) is the gradient
     * that reaches the block input through the other branch (the identity, or the downsample convolution's input gradient): it is
     * added to this convolution's (16-bit rounded) input gradient first -- the separate mh_add_h16 pass disappears.  `y_mask`
     * (16-bit [B*H*W][C] or NULL): the BatchNorm's ReLU came AFTER a residual add, so its mask is y > 0 of the block's stored output
     * (= this convolution's input activations), not recomputable from z alone. */
    const void* addend;
    const void* y_mask;
} MhConvBnBwd;
int mh_conv_dgrad(const void* dy, const void* wk, void* dx, float* workspace, const MhConvGeom* g, const MhConvBnBwd* bn,
                  mh_stream_t stream);
/* The input gradient of TWO convolutions that read the same [B][H][W][C] tensor, dx = dgrad(conv) + dgrad(conv2), both accumulated in f32
 * and rounded to 16 bits once -- a residual stage's first BasicBlock (ResNet-18/34), where the 3x3 / 2 conv1 and the 1x1 / 2 downsample
 * both send a gradient to the block input.  g: conv's geometry, what mh_conv_dgrad's strided branch accepts (k x k, k > 1, stride 2, even
 * H x W, Cout % 64 == 0) with the output grid (H/2) x (W/2) (k = 2 pad + 1 or 2 pad + 2).  conv2 is 1x1 / stride 2 / pad 0: dy2
 * [B*(H/2)*(W/2)][Cout2], wk2 its packed weight [Cout2][ldk2] (Cout2 % 64 == 0, ldk2 % 64 == 0, ldk2 >= C).  Still ONE launch of the four
 * parity-class problems: conv2 touches pixel (2h', 2w') from output (h', w') only, exactly what the class holding conv's centre tap does,
 * so its gradient is Cout2 / 64 more K tiles of that class (class (0, 0): 1 + 1 taps instead of 1 for a 3x3) -- no dgrad GEMM into an
 * [M][ldk2] panel, no mh_col2im_nhwc, no add.  bn: as for mh_conv_dgrad's strided branch (part: 4 * ceil(B*(H/2)*(W/2) / 128) columns).
 * MH_EINVAL: a null or misaligned pointer, a bn with missing fields; MH_ESHAPE: any other geometry (nothing is written). */
int mh_conv_dgrad_pair(const void* dy, const void* wk, const void* dy2, const void* wk2, int ldk2, int Cout2, void* dx, const MhConvGeom* g,
                       const MhConvBnBwd* bn, mh_stream_t stream);
/* BatchNorm2d backward from mh_conv_dgrad's partial sums: dy is ALREADY masked; finish (dgamma, dbeta, sums) + apply (dx) */
int mh_bn2d_bwd_parts(const void* dy_masked, const void* x, const float* part, int nblk, const float* gamma, const float* save_mean,
                      const float* save_rstd, void* dx, float* dgamma, float* dbeta, float* sums /* f32 [2][C] scratch */, int M, int C,
                      int flags /* MH_BN_ACCUM_PARAM_GRADS */, float scale, mh_stream_t stream);
int mh_conv_wgrad(const void* dy, const void* x, float* slabs, int ksplit, float alpha, const MhConvGeom* g, mh_stream_t stream);
/* the weight gradients of up to 6 convolutions in ONE launch (each alone is ~256 tiles: half of the 512 workgroup slots for ~26 us;
 * the backward defers them and launches consecutive layers together, with fewer K chunks each) */
#define MH_CONV_MAX_GROUP 6
typedef struct MhConvWgradProblem {
    const void* dy;      /* 16-bit [B*Ho*Wo][Cout] */
    const void* x;       /* 16-bit [B][H][W][C] */
    float* slabs;        /* f32 [ksplit][Cout][ldk] */
    int32_t ksplit;
    float alpha;
    MhConvGeom geom;
} MhConvWgradProblem;
int mh_conv_wgrad_grouped(const MhConvWgradProblem* problems /*host*/, int n, mh_stream_t stream);
/* mh_bn2d_fwd in training mode from statistics partials part[2][C][nblk] produced elsewhere (mh_conv_fwd): finish + apply */
int mh_bn2d_fwd_parts(const void* x, const float* part, int nblk, const float* gamma, const float* beta, float* running_mean,
                      float* running_var, const void* residual, void* y, float* save_mean, float* save_rstd, int M, int C, float eps,
                      float momentum, int relu, mh_stream_t stream);
int mh_maxpool_fwd(const void* x, void* y, uint8_t* arg, int B, int H, int W, int C, int K, int stride, int pad, mh_stream_t stream);
int mh_maxpool_bwd(const void* dy, const uint8_t* arg, void* dx, int B, int H, int W, int C, int K, int stride, int pad,
                   mh_stream_t stream);
int mh_avgpool_fwd(const void* x, float* y, int B, int HW, int C, mh_stream_t stream);
int mh_avgpool_bwd(const float* dy, void* dx, int B, int HW, int C, float scale, mh_stream_t stream);
int mh_add_h16(const void* a, const void* b, void* y, int64_t n, mh_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Depthwise convolution (ConvNeXt-tiny, the SVM baseline's image features: baselines/extract_feat.py:52-60 calls
 * img_model.avgpool(img_model.features(images)) on torchvision convnext_tiny; CNBlock's Conv2d(dim, dim, 7, padding=3, groups=dim)).
 * The extractor runs the forward under torch.no_grad(); the backward trains the same tower (convnext.ConvNeXtTiny.tower).
 *   mh_dwconv_weight_pack: torch weight f32 [C][1][K][K] -> tap-major f32 [K*K][C]
 *   mh_dwconv_nhwc: y[b][h][w][c] = bias[c] + sum_{i,j} wt[i*K+j][c] * x[b][h+i-K/2][w+j-K/2][c] (zero outside), 16-bit NHWC in / out,
 *                   f32 accumulation; C % 8 == 0, K == 7, stride 1.
 *   mh_dwconv_nhwc_dgrad: dx[b][h][w][c] = addend[b][h][w][c] + sum_{i,j} wt[(K-1-i)*K + (K-1-j)][c] * dy[b][h+i-K/2][w+j-K/2][c]: the
 *                   forward kernel with the taps of the SAME [K*K][C] weight image read in reverse; addend (16-bit, or NULL): the
 *                   CNBlock's residual-branch gradient, added in f32 before the one rounding.  Shape rules of the forward.
 *   mh_dwconv_nhwc_wgrad: dw[c][0][i][j] (f32, torch layout) = scale * sum_{b,h,w} dy[b][h][w][c] * x[b][h+i-K/2][w+j-K/2][c] (zero
 *                   outside), dbias[c] (or NULL) = scale * sum dy[b][h][w][c]; accum != 0 adds into dw / dbias.  x and dy are read
 *                   once; workgroups leave one f32 partial per slab of (image, tile) units in `workspace` (>=
 *                   mh_dwconv_wgrad_workspace_elems(B, H, W, C, K) f32 elements; 0 = the shape is refused), a second kernel sums the
 *                   slabs in a fixed order: no atomics, bit-identical from run to run.
 *   mh_layer_scale_bwd: CNBlock.layer_scale is folded into the second Linear (W' = gamma W, b' = gamma b), so the weight-gradient GEMM
 *                   yields dWp = dout^T h [C][K] and dbp = colsum(dout) [C] (f32).  One wave per row c:
 *                   dgamma[c] = sum_k W[c][k] dWp[c][k] + b[c] dbp[c], dW = gamma[c] dWp, db = gamma[c] dbp.  dW / db may BE dWp / dbp (in
 *                   place) when accum == 0; accum != 0 adds into dW, db and dgamma (then they must be buffers of their own).  K % 4 == 0.
 * The block's LayerNorm / Linear / GELU / Linear + residual run on mh_layernorm_fwd and mh_gemm_bf16_grouped; the patchify
 * stem and the 2x2 / stride-2 downsampling convolutions on mh_im2col_nhwc + mh_gemm_bf16_grouped (bias in the epilogue).
 * ------------------------------------------------------------------------------------------ */
int mh_dwconv_weight_pack(const float* w, float* wt, int C, int K, mh_stream_t stream);
int mh_dwconv_nhwc(const void* x, const float* wt, const float* bias, void* y, int B, int H, int W, int C, int K, mh_stream_t stream);
int mh_dwconv_nhwc_dgrad(const void* dy, const float* wt, const void* addend, void* dx, int B, int H, int W, int C, int K,
                         mh_stream_t stream);
int64_t mh_dwconv_wgrad_workspace_elems(int B, int H, int W, int C, int K);
int mh_dwconv_nhwc_wgrad(const void* x, const void* dy, float* dw, float* dbias, float* workspace, int B, int H, int W, int C, int K,
                         float scale, int accum, mh_stream_t stream);
int mh_layer_scale_bwd(const float* W, const float* b, const float* gamma, const float* dWp, const float* dbp, float* dW, float* db,
                       float* dgamma, int C, int K, int accum, mh_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Grouped 3x3 convolution (groupconv.hip): conv2 of a ResNeXt bottleneck (torchvision resnext50_32x4d, the image model of
 * example_scripts/Untitled-2.py:210-237: 32 groups of 4 / 8 / 16 / 32 channels), nn.Conv2d(C, C, 3, stride, padding=1, groups=groups,
 * bias=False) on NHWC 16-bit activations [B*H*W][C].  One wave owns 16 output channels and contracts, on mfma_f32_16x16x32, over the
 * channels of the groups those belong to only (Cg <= 16: 16 channels, two taps per K step; Cg == 32: 32 channels, one tap per step).
 * One geometry rule for every entry point: g->C == g->Cout == C, C % 32 == 0, Cg = C / groups in {4, 8, 16, 32}, KH == KW == 3,
 * pad == 1, stride 1 or 2, any B, H, W >= 1; g->ldk is not read; B*H*W < 2^24 and every tensor < 2 GiB.  Ho = (H - 1) / stride + 1.
 * Anything else: MH_ESHAPE.  A NULL pointer, a 16-bit tensor or packed weight not on a 16-byte boundary, an f32 tensor not on a 4-byte
 * boundary: MH_EINVAL.  In both cases nothing is written.
 *   mh_gconv_packed_elems: 16-bit elements of the packed weight (0: C / groups is refused) = 2 * (C / 16) * NS * 512, NS = 5 (Cg <= 16)
 *                   or 9 (Cg == 32).
 *   mh_gconv_weight_pack: w f32 [C][Cg][3][3] (the nn.Conv2d weight) -> wk, TWO images [2][C / 16][NS][64][8] of ready MFMA
 *                   fragments: element j of lane l of K step s of 16-channel block cb is M[row = 16 cb + (l & 15)][k = 8 (l >> 4) + j],
 *                   k -> (tap, contraction channel): Cg <= 16: tap = 2 s + (k >> 4), channel 16 cb + (k & 15); Cg == 32: tap = s,
 *                   channel 32 (cb / 2) + k; tap = 3 kh + kw.  Image 0 (forward): row = output channel, contraction = input channel;
 *                   image 1 (dgrad): row = input channel, contraction = output channel.  Channel pairs of two groups and tap 9 hold 0.
 *   mh_gconv_fwd:   y[B*Ho*Wo][C], rounded once from the f32 accumulators.  bn_part (or NULL): f32 [2][C][ceil(B*Ho*Wo / 128)], per 128-row
 *                   tile the column sums of y and y^2 of the values AS STORED -- what mh_bn2d_fwd_parts reads.
 *   mh_gconv_dgrad: dx[B*H*W][C] from dy[B*Ho*Wo][C], a gather per input pixel over the taps that reach it (stride 2: those of its
 *                   parity): no col2im panel, no scatter, every element of dx written exactly once.  No BatchNorm epilogue.
 *   mh_gconv_wgrad: dw f32 [C][Cg][3][3] = (accumulate ? dw : 0) + alpha * sum over the B*Ho*Wo pixels of dy x^T per tap -- the nn.Conv2d
 *                   weight's layout, so it can BE an f32 .grad.  workspace: f32, >= mh_gconv_wgrad_workspace_elems(g, groups) elements
 *                   (0: refused): workgroups leave per-chunk partials [chunk][C][Cg][9], a second kernel sums them in chunk order -- no
 *                   atomics, the same bits on every run.
 * ------------------------------------------------------------------------------------------ */
int mh_gconv_packed_elems(int C, int groups);
int mh_gconv_weight_pack(const float* w, void* wk, int C, int groups, mh_stream_t stream);
int mh_gconv_fwd(const void* x, const void* wk, void* y, float* bn_part, const MhConvGeom* g, int groups, mh_stream_t stream);
int mh_gconv_dgrad(const void* dy, const void* wk, void* dx, const MhConvGeom* g, int groups, mh_stream_t stream);
int mh_gconv_wgrad_workspace_elems(const MhConvGeom* g, int groups);
int mh_gconv_wgrad(const void* dy, const void* x, float* dw, float* workspace, int accumulate, float alpha, const MhConvGeom* g, int groups,
                   mh_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Squeeze-and-excitation (se.hip): timm's SEModule between a bottleneck's bn3 and its residual add (seresnext50_32x4d, the first
 * model of example_scripts/Untitled-2.py:362-371).  u = bn3(conv3(.)) [B*HW][C] 16-bit NHWC (no ReLU, no residual);
 *   pooled = mean_hw u (mh_avgpool_fwd);  hidden = relu(w1 pooled + b1);  s = sigmoid(w2 hidden + b2);  y = relu(u * s + shortcut).
 * w1 [R][C], b1 [R], w2 [C][R], b2 [C]: the nn.Conv2d(C, R, 1) / nn.Conv2d(R, C, 1) parameters; everything indexed [B][C] or [B][R] is f32.
 * One shape rule: C % 8 == 0, 8 <= C <= 4096, 1 <= R <= 256, HW >= 1 with HW * C / 8 < 2^31, B >= 1 -- B is a grid dimension: x (2^31 - 1)
 * for the two gate entry points, y (65535) for the three over the activation; anything else: MH_ESHAPE.  A NULL pointer, or a 16-bit tensor / s / dpooled not on a 16-byte boundary: MH_EINVAL.  In both cases nothing is
 * written.  No atomics: every sum has one owner and an order fixed by the shape, so two calls give the same bits.
 *   mh_se_gate_fwd:   hidden (stored after the ReLU) and s = 1 / (1 + expf(-a)) with the accurate expf: a saturated gate is exactly 0
 *                     (a < ~-88.7) or 1 (a > ~16.7), never NaN.  Two launches: a wave per (image, hidden unit), a thread per (image, channel).
 *   mh_se_apply_fwd:  y = relu(u * s[b] + shortcut), f32, rounded once to 16 bits.
 *   mh_se_apply_bwd_reduce: g = dy where y > 0 (dy's bits) else +0 -- the gradient of the shortcut branch --, and ds[b][c] = sum_hw g * u
 *                     in f32.  One workgroup owns 64 columns of an image over all of HW (rows ascending per thread, then a fixed tree).
 *   mh_se_gate_bwd:   back through the sigmoid, fc2, the ReLU (mask hidden > 0) and fc1: dpooled [B][C] keeps ds's scale (the gradient
 *                     stream's); dw1 [R][C], db1 [R], dw2 [C][R], db2 [C] = (accumulate ? target : 0) + alpha * the sum over the batch
 *                     (b ascending; alpha * sum is rounded to f32 before the add), in the nn.Conv2d layouts -- they can BE f32 .grads.
 *   mh_se_apply_bwd:  du = g * s[b] + dpooled[b] / HW (a true division), f32, rounded once to 16 bits.
 * ------------------------------------------------------------------------------------------ */
int mh_se_gate_fwd(const float* pooled, const float* w1, const float* b1, const float* w2, const float* b2, float* hidden, float* s, int B,
                   int C, int R, mh_stream_t stream);
int mh_se_apply_fwd(const void* u, const float* s, const void* shortcut, void* y, int B, int HW, int C, mh_stream_t stream);
int mh_se_apply_bwd_reduce(const void* dy, const void* y, const void* u, void* g, float* ds, int B, int HW, int C, mh_stream_t stream);
int mh_se_gate_bwd(const float* ds, const float* s, const float* hidden, const float* pooled, const float* w1, const float* w2,
                   float* dpooled, float* dw1, float* db1, float* dw2, float* db2, int B, int C, int R, float alpha, int accumulate,
                   mh_stream_t stream);
int mh_se_apply_bwd(const void* g, const float* s, const float* dpooled, void* du, int B, int HW, int C, mh_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Optimizer (torch.optim.Adam / AdamW, Multimodal_example_task2C.txt:249,217; HF Trainer
 * adamw_torch + max_grad_norm, DistilBERT_example_task2A.ipynb:3211-3213,3280):
 *   mh_sumsq_f32: out[0] = sum g^2 over n elements (two-pass deterministic; workspace >= 1024 f32)
 *   mh_adam_step: dense single-launch update over the flat parameter buffer.  Every per-step
 *     scalar is read from DEVICE memory so a captured hipGraph of the step can be replayed:
 *     hyper = f32[8] {lr, beta1, beta2, eps, weight_decay, 1/(1-beta1^t), 1/sqrt(1-beta2^t), grad_scale}
 *     g' = g * grad_scale * min(1, max_norm / (sqrt(*gnorm_sq)*|grad_scale| + 1e-6)) (clip only
 *          when gnorm_sq != NULL and max_norm > 0); a NON-FINITE *gnorm_sq skips the update altogether
 *          (parameters and moments untouched), as GradScaler.step does after an fp16 overflow.
 *          clip_norm_mult > 0 replaces |grad_scale| in the clip coefficient (only there): with clip_norm_mult = the static
 *          gradient-stream scale, sqrt(*gnorm_sq) * clip_norm_mult is the norm of the LOSS-SCALED gradients, i.e. the clip of the
 *          reference's default fp16 branch, which calls clip_grad_norm_(model.parameters(), 1.0) on the scaled gradients before
 *          scaler.step unscales them (Multimodal_example_task2C.py:712-717); 0 = clip the true gradients
 *     m = b1 m + (1-b1) g' ; v = b2 v + (1-b2) g'^2 ; p -= lr/bc1 * m / (sqrt(v)/sqrt(bc2) + eps)
 *     (L2 wd folds into g', decoupled wd scales p first); also refreshes the bf16 shadow copy
 *     p_bf16[i] for i < n_shadow (the GEMM operands).  n, n_shadow multiples of 4.
 *   mh_adam_step_rows: the same update over a [rows][D] table, skipping rows whose row_live byte is 0.  A row of
 *     the word-embedding table that has never received a gradient has g = m = v = 0, for which the dense update is
 *     the identity (with weight_decay == 0): skipping it is bit-identical to torch.optim.Adam and saves 28 B/element
 *     of HBM traffic on the 49 M-element table (a batch touches at most B*S of its 64 000 rows).
 *   mh_cast_f32_bf16: shadow refresh on its own (after load_state_dict).
 *     `overflow` (device int32[1] or NULL) selects the GUARDED form used when a slice is updated before the global norm can
 *     exist (optimizer-in-backward); `guard_ordinal` >= 1 is then this launch's position among the step's guarded launches (1, 2,
 *     ... in stream order).  *overflow holds the ordinal of the first launch of the step that met a non-finite gradient (0 = none):
 *     a launch that finds an EARLIER launch's mark does nothing; otherwise a 4-element vector whose gradient is not finite keeps its
 *     parameters and moments and marks *overflow with this launch's ordinal.  A launch never skips for its own mark, so what it
 *     updates depends on the gradient data only, not on workgroup scheduling: deterministic, identical on data-parallel replicas.
 *     The slices of a step run in backward order on one stream, so an overflow at the loss skips the whole step, one further down
 *     leaves the layers above it updated.
 *   mh_adam_skip_account (steps that may be skipped: fp16 runs, the reference's GradScaler, Multimodal_example_task2C.py:60-64,
 *     712-717): ONE launch per step AFTER the update launches.  A step is "bad" when *gnorm_sq is not finite (exact path: the
 *     update kernels skipped it as a whole) or *loss_scale->overflow is set (guarded path; cleared here).  It counts bad steps in
 *     state[0] (state[1] = this step was bad), updates the dynamic loss scale as torch.cuda.amp.GradScaler.update does (bad:
 *     scale *= backoff_factor, growth counter 0; else counter + 1 and, at growth_interval, scale *= growth_factor; clamped to
 *     [min_scale, max_scale]) and writes what the NEXT step's update kernels read: every group's bias corrections hyper[5..6] for
 *     t = *step_dev + 1 - state[0] (as with GradScaler.step, which does not call optimizer.step() after an overflow, a skipped
 *     step does not advance Adam's t; betas are passed as doubles, 1 - beta^t in double like the host) and, with a loss scale,
 *     hyper[7] = base_grad_scale / scale.  The loss kernels multiply *scale into dlogits (grad_scale_dev).
 * ------------------------------------------------------------------------------------------ */
#define MH_ADAM_MAX_GROUPS 8
typedef struct MhAdamSkipGroups {
    float* hyper[MH_ADAM_MAX_GROUPS];      /* device f32[8] per parameter group */
    double beta1[MH_ADAM_MAX_GROUPS];
    double beta2[MH_ADAM_MAX_GROUPS];
    int32_t n;
    int32_t reserved_;
} MhAdamSkipGroups;
typedef struct MhLossScale {
    float* scale;             /* device f32[1]: the dynamic loss scale, or NULL (only count / bias-correct) */
    int32_t* growth;          /* device int32[1]: clean steps since the last change */
    int32_t* overflow;        /* device int32[1] or NULL: raised by the guarded update kernels, cleared here */
    float growth_factor, backoff_factor, min_scale, max_scale;
    int32_t growth_interval;
    float base_grad_scale;    /* 1 / world size */
} MhLossScale;
int mh_adam_skip_account(const MhAdamSkipGroups* groups, const float* gnorm_sq /*device or NULL*/, int32_t* state /*device int32[2]*/,
                         const int32_t* step_dev /*device: the host's step count*/, const MhLossScale* loss_scale /*or NULL*/,
                         mh_stream_t stream);
int mh_sumsq_f32(const float* g, int64_t n, float* workspace /*>=1024 f32*/, float* out,
                 mh_stream_t stream);
int mh_adam_step(float* p, float* m, float* v, const float* g, void* p_bf16, int64_t n,
                 int64_t n_shadow, const float* hyper /*device f32[8]*/, int decoupled,
                 const float* gnorm_sq /*device or NULL*/, float max_norm, float clip_norm_mult /*0: clip true gradients*/,
                 int32_t* overflow /*device or NULL*/, int guard_ordinal /*>= 1 with overflow, else ignored*/, mh_stream_t stream);
int mh_adam_step_rows(float* p, float* m, float* v, const float* g,
                      uint8_t* row_live /*[rows] optimizer state: 1 = this row's m / v may be non-zero*/,
                      const uint8_t* row_touched /*[rows] or NULL: rows that have received a gradient (mh_bert_embed_bwd);
                      OR-ed into row_live*/, int rows, int D, const float* hyper /*device f32[8]*/, int decoupled,
                      const float* gnorm_sq, float max_norm, float clip_norm_mult, int32_t* overflow /*device or NULL*/,
                      int guard_ordinal, mh_stream_t stream);
int mh_cast_f32_bf16(const float* src, void* dst, int64_t n, mh_stream_t stream);
int mh_cast_bf16_f32(const void* src, float* dst, int64_t n, mh_stream_t stream);
/* Data-parallel gradient exchange with 16-bit wire format (ddp.GradientReducer(compress="bf16")): out[i] = 16-bit(sum_w
 * in[w][i]) with the sum in fp32 and a fixed order -- the shards received by the all-to-all, accumulated on receipt. */
int mh_sum_shards_16(const void* in /*[W][shard]*/, void* out /*[shard]*/, int W, int64_t shard, mh_stream_t stream);
/* Gradient accumulation over micro-batches: the small gradients of a backward (biases, LayerNorm, head, class token, position
 * and type tables) are written to a scratch mirror of their run of the flat gradient buffer and added into it here, several
 * spans per launch: dst[i] = dst[i] + src[i] for i < n, ONE f32 add of two stored f32 values per element (never contracted with
 * anything), 16-byte loads and stores.  dst and src 16-byte aligned, n >= 1 (any: the last 1..3 elements go one by one); spans
 * must not overlap. */
#define MH_SPAN_MAX_JOBS 16
typedef struct MhSpanJob {
    float* dst;         /* device */
    const float* src;   /* device */
    int64_t n;
} MhSpanJob;
int mh_accum_spans_f32(const MhSpanJob* jobs /*host*/, int n_jobs, mh_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * Autoregressive decode (decode.hip): BLIP image captioning, one new token per row and step
 * (BlipForConditionalGeneration.generate, greedy; Multimodal_example_task2C.py:195-256).  Every per-step state is read
 * on the device, so one step is captured once as a hipGraph and replayed per token.  Deterministic (fixed-order sums).
 *
 * mh_attn_decode: one query per (row b, head h) against T cached keys / values, head dim 64, scale 1/8, f32 online softmax.
 *   q  : 16-bit, (b, h) at q + b*ldq + h*64
 *   k,v: 16-bit, key j of (b, h) at k + b*ld_b + j*ld_t + h*64 (v likewise)
 *   t_dev == NULL: T keys (cross-attention over a fixed memory, e.g. 577 image tokens).
 *   t_dev != NULL: self-attention over a cache of capacity T: this step's k of (b, h) at kv_new + b*ld_new + h*64 and its
 *                  v H*64 elements further are stored into slot t = t_dev[0] first, and keys 0..t attend.  t >= T (the
 *                  cache is full): nothing is stored and the cached keys 0..T-1 attend, without this step's k / v.
 *   out: 16-bit, (b, h) at out + b*ldo + h*64.
 *   nsplit > 1: the keys are cut into nsplit chunks (rows * heads too few to fill the chip); partials (m, l, acc) go to
 *               workspace f32 [B*H][nsplit][66] and a second launch combines them in split order.  nsplit <= 64.
 *   ldq, ld_t, ld_b, ld_new multiples of 8; bases 16-byte aligned.
 * mh_decode_embed: y[b] = LayerNorm(word[ids[b]] + pos[t_dev[0]]) (f32 tables [V][D], [P][D]), 16-bit out [B][D], D <= 2048.
 *   An id outside [0, V) reads row 0 (id < 0) or V-1 (id >= V); t outside [0, P) reads row 0 or P-1 likewise.
 * mh_greedy_step: one launch per step over f32 logits [B][ldl] (columns >= V are never chosen; ties go to the lowest index;
 *   NaN ranks above every number, so a row holding a NaN picks its first NaN, and an all -inf row picks 0: torch.argmax).
 *   state int32[4] = {t, arrival counter (0), rows finished, output length once all rows finished (0 before)}.
 *   Column c = t + 1 of out_ids int64 [B][ld_out] receives the prompt token (c < prompt_len, read from out_ids itself), pad_id
 *   (row finished before), or the argmax, which marks the row finished when it is eos_id.  next_ids[b] = that token; t += 1.
 *
 * Beam search (rows are [image][beam], K beams per image, 2 <= K <= 8):
 * mh_attn_decode_beams: mh_attn_decode with two more arguments (mh_attn_decode is this call with kv_group 1 and src NULL).
 *   kv_group: row b reads the k / v of row b / kv_group (cross-attention: one copy of the image's k / v for its K beams).
 *             B % kv_group == 0; the self form (t_dev) needs kv_group 1.
 *   src     : self form only.  int32 [B][ld_src], ld_src >= T: key j < t of row b is read from cache row src[b][j] (entries
 *             are clamped to [0, B)); this step's k / v still go to slot t of row b itself.  mh_beam_step keeps the table.
 * mh_beam_step: two launches per step over f32 logits [B*K][ldl]: transformers' GenerationMixin._beam_search with one eos token.
 *   Per row the f32 log-softmax ((x - max) - log(sum)) plus the beam's running score and the row's top 2K; per image the
 *   ordered top 2K of the K*V candidates, the K running beams (the best that neither are eos nor reach cap, the maximum
 *   length), the finished beams (candidates among the first K that stop, scored logp / (c + 1 - prompt_len) ** length_penalty,
 *   merged with the K kept so far) and the early-stop heuristic.  early_stopping: 0 False, 1 True, 2 "never".
 *   Ties: the larger f32 value first, then the lower flat index beam * V + token; in the later selections the lower position.
 *   state int32[4] = {t, arrival counter (0), images closed this step (0), 1 once no image's finished beams can change}.
 *   Column c = t + 1: inside the prompt (c < prompt_len) every beam takes run_seq's token and is its own parent.  t += 1.
 *   The sequences (int32 [B*K][cap]) and src are permuted by parent in place; src[row][t] becomes the parent's row.
 *   Start: run_scores {0, -1e9, ...} per image, fin_scores -1e9, fin_flags 0, fin_len 0, heur 1, state 0, run_seq = fin_seq =
 *   the prompt padded with pad_id, next_ids the prompt's first token.  V >= 2K; logits must be finite or -inf.
 *
 * Logits processors (MhLogitsProcess; mh_greedy_step_processed / mh_beam_step_processed are the two calls above plus one, and the
 * two calls above are these with the neutral settings {1, 0, 0, 0}, which launch the kernels without any processing).  They are
 * transformers' own, in _get_logits_processor's order, over the row's history: its cur_len = t + 1 tokens so far, prompt included
 * (greedy: out_ids[b][0..t]; beams: run_seq[row][0..t], which already follows the row's parent).  Nothing is processed inside the
 * prompt (t + 1 < prompt_len).
 *   1. repetition_penalty p (RepetitionPenaltyLogitsProcessor): every distinct id of the history gets s = s < 0 ? s * p : s / p,
 *      once however often it occurs.  p finite and > 0; 1 is neutral.
 *   2. no_repeat_ngram_size n (NoRepeatNGramLogitsProcessor): wherever the last n - 1 tokens occur earlier in the history, the
 *      token that followed them becomes -inf (n = 1: every token seen).  Nothing is banned while cur_len < n.  0 is neutral.
 *   3. min_length (MinLengthLogitsProcessor): eos_id is -inf while cur_len < min_length (the prompt counts).
 *   4. min_new_tokens (MinNewTokensLengthLogitsProcessor): eos_id is -inf while cur_len - prompt_len < min_new_tokens.
 *   Greedy: they act on the raw f32 logits, before the argmax (an all -inf row picks 0).  Beams: they act on the row's f32
 *   log-softmax -- the log-sum-exp is taken over the unprocessed logits, the penalty therefore acts on values <= 0 -- before the
 *   beam's running score is added; -inf + score stays -inf.  Ties keep their rule.  The minimum lengths are tested against the
 *   device step counter, so a captured step replays correctly.
 *   Limits when any setting is not neutral (MH_ESHAPE otherwise): V <= MH_PROCESS_MAX_VOCAB (two bitmaps of V bits in 8 KB of
 *   LDS), ld_out / cap <= MH_PROCESS_MAX_HISTORY (the history in 4 KB of LDS), and for beams V >= 2K + cap + 1: at most one ban
 *   per history position plus eos, so every row keeps 2K finite candidates.  Settings outside their domain: MH_EINVAL.
 *   The work added is proportional to the history (cur_len * n / 256 comparisons per thread); no pass over V is added.
 * ------------------------------------------------------------------------------------------ */
#define MH_PROCESS_MAX_VOCAB 32768
#define MH_PROCESS_MAX_HISTORY 1024
typedef struct MhLogitsProcess {
    float repetition_penalty;
    int no_repeat_ngram_size, min_length, min_new_tokens;
} MhLogitsProcess;
typedef struct MhBeamState {
    int64_t* next_ids;   /* [B*K] the running beams' new tokens: the next step's input ids */
    int32_t* parents;    /* [B*K] the beam (0..K-1 of its image) each running beam continues */
    float* run_scores;   /* [B*K] */
    int32_t* run_seq;    /* [B*K][cap] */
    int32_t* src;        /* [B*K][cap] cache ancestry table of mh_attn_decode_beams, or NULL */
    int32_t* fin_seq;    /* [B*K][cap] finished beams, best first */
    float* fin_scores;   /* [B*K] */
    int32_t* fin_flags;  /* [B*K] 1: the slot holds a finished beam */
    int32_t* fin_len;    /* [B*K] its generated length */
    int32_t* heur;       /* [B] 1 while a running beam may still beat the worst finished one */
    int32_t* state;      /* [4] */
    float* cand_val;     /* [B*K][2K] workspace: each row's top 2K */
    int32_t* cand_idx;   /* [B*K][2K] */
} MhBeamState;
int mh_attn_decode(const void* q, int ldq, void* k, void* v, int64_t ld_b, int ld_t, const void* kv_new, int ld_new,
                   const int32_t* t_dev, int T, void* out, int ldo, float* workspace, int nsplit, int B, int H,
                   mh_stream_t stream);
int mh_attn_decode_beams(const void* q, int ldq, void* k, void* v, int64_t ld_b, int ld_t, const void* kv_new, int ld_new,
                         const int32_t* t_dev, int T, void* out, int ldo, float* workspace, int nsplit, int B, int H,
                         int kv_group, const int32_t* src, int ld_src, mh_stream_t stream);
int mh_beam_step(const float* logits, int ldl, int V, int B, int K, const MhBeamState* st, int cap, int prompt_len,
                 float length_penalty, int early_stopping, int64_t eos_id, mh_stream_t stream);
int mh_decode_embed(const int64_t* ids /*[B]*/, const int32_t* t_dev, const float* word, const float* pos, const float* gamma,
                    const float* beta, void* y, int B, int D, int V, int P, float eps, mh_stream_t stream);
int mh_greedy_step(const float* logits, int ldl, int V, int B, int64_t* out_ids, int ld_out, int64_t* next_ids,
                   int32_t* finished /*[B]*/, int32_t* state /*[4]*/, int prompt_len, int64_t eos_id, int64_t pad_id,
                   mh_stream_t stream);
int mh_greedy_step_processed(const float* logits, int ldl, int V, int B, int64_t* out_ids, int ld_out, int64_t* next_ids,
                             int32_t* finished /*[B]*/, int32_t* state /*[4]*/, int prompt_len, int64_t eos_id, int64_t pad_id,
                             const MhLogitsProcess* process, mh_stream_t stream);
int mh_beam_step_processed(const float* logits, int ldl, int V, int B, int K, const MhBeamState* st, int cap, int prompt_len,
                           float length_penalty, int early_stopping, int64_t eos_id, const MhLogitsProcess* process,
                           mh_stream_t stream);

/* Sampling (generate(do_sample=True)).  mh_sample_step is mh_greedy_step with a draw in place of the argmax: one launch per step,
 * one workgroup per row over f32 logits [B][ldl] (columns >= V are never read as candidates), the same out_ids / next_ids /
 * finished / state words, the same prompt column (c < prompt_len: the prompt's next token), finished row (pad_id), eos handling and
 * arrival counter.  Per generating row, in transformers' order (_get_logits_processor: processors, then the warpers):
 *   1. process (NULL or neutral: none): the four logits processors above, on the raw logits, as mh_greedy_step_processed.
 *   2. temperature: x = x / temperature, one correctly rounded f32 division (skipped when it is 1).
 *   3. top_k > 0 (TopKLogitsWarper): keep every i with x_i >= the k-th largest value; ties at the threshold are all kept
 *      (transformers removes `scores < kth`).  top_k = 0 or >= V: no filter.
 *   4. top_p < 1 (TopPLogitsWarper, min_tokens_to_keep 1), over the softmax of the top-k survivors with total mass Z: keep i iff the
 *      mass of the survivors with a strictly larger value is < top_p * Z.  Without ties this is transformers' ascending cumulative
 *      sum with `<= 1 - top_p` removed.  Where equal f32 values straddle the boundary, torch.sort leaves the choice open: this rule
 *      keeps them all.  The masses of this step are exact integer sums of exp(x - max) * 2^40, truncated: within 2^-25 of Z.
 *   5. draw: u = (h >> 8) * 2^-24 with h = hash(hash(hash(hash(rng[0] ^ 0x9E3779B9) + rng[1]) + row) + column), 32-bit arithmetic,
 *      hash the counter hash of the dropout sites; rng: device uint32[4] {seed_lo, seed_hi, -, -}, read by the kernel, so a
 *      captured launch serves every seed; column = t + 1.  The token is the first kept index, in ascending index order, whose
 *      inclusive prefix mass exceeds u * Z_kept; if rounding leaves none, the last kept index whose value is not -inf -- never an
 *      unkept one.  If the row's maximum is not finite (a NaN, +inf, or an all -inf row: Z_kept would not be a positive finite
 *      number), the token is mh_greedy_step's.  u_out (NULL or f32 [B]) receives every row's u.
 *   Deterministic: no floating-point atomics; every f32 mass is a fixed-order sum in which no term passes through more than 46
 *   additions (contract: 256), so it lies within 256 * 2^-24 = 2^-16 of the exact mass relative to Z; the same logits, settings and
 *   seed give the same token on every run, launched directly or replayed from a graph.
 *   Limits (MH_ESHAPE otherwise): V <= MH_PROCESS_MAX_VOCAB, with or without processors; temperature finite and > 0; top_k >= 0;
 *   0 < top_p <= 1; with processors their own limits.  sampling or rng NULL, or processor settings outside their domain: MH_EINVAL. */
typedef struct MhSampling {
    float temperature;
    int top_k;
    float top_p;
} MhSampling;
int mh_sample_step(const float* logits, int ldl, int V, int B, int64_t* out_ids, int ld_out, int64_t* next_ids,
                   int32_t* finished /*[B]*/, int32_t* state /*[4]*/, int prompt_len, int64_t eos_id, int64_t pad_id,
                   const MhSampling* sampling, const uint32_t* rng /*device u32[4]*/, float* u_out /*[B] or NULL*/,
                   const MhLogitsProcess* process /*NULL or neutral: none*/, mh_stream_t stream);

/* ------------------------------------------------------------------------------------------
 * SVM (svm.hip): sklearn.svm.SVC(C, kernel='linear') of the organizers' baselines (baselines/subtask_2c.py:61,85,
 * subtask_2b.py), i.e. libsvm's SMO solver for the C-SVC dual
 *     minimise 1/2 a^T Q a - e^T a   subject to  0 <= a_t <= C_t,  y^T a = 0,   Q_st = y_s y_t K_st,  K = X X^T
 * for a batch of P problems that share the labels y and the Gram matrix K and differ in their per-sample bounds Cv [P][n]
 * (a C grid, class_weight / sample_weight, fold masks: a sample with C_t = 0 never enters the working set and keeps a_t = 0).
 * K comes from mh_gemm_f32 (A = B = X); coef = (a * y)^T X and the decision values go through mh_gemm_f32 as well.
 *
 * Working-set selection WSS2 (Fan, Chen, Lin 2005), gradient G = Q a - e:
 *     I_up  = {y_t = +1, a_t < C_t} u {y_t = -1, a_t > 0},   I_low = {y_t = +1, a_t > 0} u {y_t = -1, a_t < C_t}
 *     i = argmax_{I_up} -y_t G_t (= Gmax);   j = argmax_{t in I_low, b_t > 0} b_t^2 / a_t  with  b_t = Gmax + y_t G_t,
 *     a_t = K_ii + K_tt - 2 K_it (1e-12 when not positive);   ties go to the LOWEST index (libsvm: the highest), so a run is
 *     deterministic (for j the rule holds up to the rounding of the quotient: the samples one thread owns are ordered by the
 *     cross-multiplied b_1^2 a_2 > b_2^2 a_1, one division per thread; a near-tie may so pick another j of the same gain to
 *     within an ulp, which optimality does not see); libsvm's two-variable update with its clipping against C_i and C_j;  stop when
 *     gap = Gmax - min_{I_low} -y_t G_t < tol.   rho = mean of y_t G_t over the free vectors (0 < a_t < C_t), or the midpoint of
 *     the two bounds when there is none; samples with C_t = 0 take no part in it.
 * One workgroup of 1024 threads per problem: alpha and G live in float64 registers, K is f32; n <= MH_SVC_MAX_N (16 samples per
 * thread), P <= MH_SVC_MAX_PROBLEMS, else MH_ESHAPE.  No unbounded device loop: a launch runs at most `budget` iterations per
 * problem (MH_SVC_LAUNCH_ITERS is what the package passes), then writes alpha, G and state[p] = {status, iterations so far,
 * gap, rho} (MH_SVC_STATE doubles) and returns; the caller launches again while a status is MH_SVC_RUNNING -- the buffers are the
 * whole state, so a launch resumes.  max_iter < 0: no limit; else status MH_SVC_MAXITER once that many iterations are done.
 *   mh_svc_init : alpha = 0, G = -1, state = {MH_SVC_RUNNING, 0, inf, 0}
 *   mh_svc_solve: one launch
 * ------------------------------------------------------------------------------------------ */
#define MH_SVC_MAX_N 16384
#define MH_SVC_MAX_PROBLEMS 64
#define MH_SVC_LAUNCH_ITERS 4096
#define MH_SVC_STATE 4
#define MH_SVC_RUNNING 0
#define MH_SVC_CONVERGED 1
#define MH_SVC_MAXITER 2
typedef struct MhSvcProblem {
    const float* K;      /* f32 [n][ldk] */
    const float* y;      /* f32 [n], +1 / -1 */
    const double* Cv;    /* f64 [P][n] */
    double* alpha;       /* f64 [P][n] */
    double* G;           /* f64 [P][n] */
    double* state;       /* f64 [P][MH_SVC_STATE] */
    int32_t n, ldk, P, budget;
    int32_t max_iter, reserved_;
    double tol;
} MhSvcProblem;
int mh_svc_init(const MhSvcProblem* p /*host*/, mh_stream_t stream);
int mh_svc_solve(const MhSvcProblem* p /*host*/, mh_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MEMEHIP_H */

/*
 * lrx.h -- C ABI of liblrx.so: the MI355X (gfx950) corpus-embedding + flat-IP search hot path of LightRetriever.
 *
 * The reference (caskcsg/lightretriever) is pure Python and has no FFI of its own; its
 * per-batch operator boundary is HybridModel.encode_passage / encode_query and faiss.IndexFlatIP.  Each entry
 * point below names the reference interface (file:line under /root/reference) it replaces.  All pointers are
 * DEVICE pointers unless the name says `host`; all sizes are element counts unless the name says `bytes`;
 * `stream` is a hipStream_t passed as void* (NULL = the null stream).  No entry point allocates device memory,
 * synchronises the device or touches torch: the caller (PyTorch-ROCm in this build) owns memory and streams.
 * Every function returns LRX_OK (0) or a negative error; lrx_last_error() gives the message (thread-local).
 */
#ifndef LRX_H
#define LRX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LRX_ABI_VERSION 9

enum {
  LRX_OK = 0,
  LRX_ERR_INVALID = -1,   /* bad argument / unsupported shape */
  LRX_ERR_HIP = -2,       /* a HIP runtime call failed */
  LRX_ERR_WORKSPACE = -3, /* workspace too small */
};

int lrx_abi_version(void);
const char* lrx_last_error(void);

/* ------------------------------------------------------------------------------------------------------------
 * Encoder model description: the subset of HF config.json that decides the dense-path arithmetic
 * (transformers LlamaConfig / Qwen2Config; reference loads it at finetune/modeling_encoder.py:602-633).
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct lrx_encoder_config {
  int32_t vocab_size;
  int32_t hidden_size;        /* H; multiple of 64 */
  int32_t num_layers;
  int32_t num_q_heads;
  int32_t num_kv_heads;
  int32_t head_dim;           /* 64 or 128 */
  int32_t intermediate_size;  /* multiple of 64 */
  float rms_eps;
  int32_t qkv_bias;           /* 1 for Qwen2.5 */
  int32_t max_positions;      /* rows of the RoPE table */
  int32_t norm_folded;        /* 1: the caller pre-multiplied the RMSNorm weights into the next projection's columns (wqkv := W_qkv diag(ln1),
                                 wgu := W_gu diag(ln2), fp32 product rounded to bf16); the layers then never materialise the normalised
                                 activations: the row statistic rsqrt(mean(x^2)+eps) is applied to the GEMM's fp32 accumulator and the
                                 residual GEMMs emit the sum of squares of the rows they write.  Same function; the two bf16 roundings of
                                 the normalised activations disappear (closer to the fp32 model).  ln1 / ln2 are ignored.            */
  int32_t precise_stream;     /* 1 (needs norm_folded = 0 and the ORIGINAL wqkv / wgu): the residual stream is kept in fp32; every residual GEMM
                                 adds into it with one rounding (to fp32) and also writes the next projection's bf16 operand bf16(x * gamma_next)
                                 -- the norm weight rides on the activation, the weights stay exact, the row statistic is applied to the consumer's
                                 accumulator as with norm_folded.  For deep backbones: at 32 layers the bf16 stream + folded weights spend ~1.1e-3
                                 of the 1e-3 cosine budget against the fp32 model (tools/exp/rounding_budget.py); +6 B / element of traffic
                                 per residual GEMM (~3 % of a step).  LrxEncoder switches it on for EVERY backbone (since round 5: the mode that
                                 holds 1e-3 on trained-like weights; EncoderConfig(precise_stream=False) selects the bf16 stream).
                                 2: the same with FP16 GEMM operands (round 6; on request): wqkv / wo / wgu / wdown hold fp16 values
                                 (the caller converts the bf16 checkpoint once: exact for every |w| in [6.1e-5, 65504]; biases, norm weights
                                 and the embedding stay bf16), the activations fp16(x * gamma), the attention and SwiGLU outputs travel as fp16
                                 and every projection runs on the f16 MFMA (same rate).  Three more mantissa bits per operand: 1 - cos against
                                 the fp32 model drops 14-42 x (8B, trained-like weights: 3.4e-4 -> 8e-6, tools/exp/rounding_fp16_o_act.py).
                                 Values outside fp16's range saturate and count (lrx_device_saturation_count).  -3.5 % docs/s (f16 MFMA power).
                                 3: the QKV projection only (LrxEncoder's default): wqkv as fp16, its A operand fp16(x * gamma) -- the one rounding
                                 that is 70 % of mode 1's distance to the fp32 model (8B, worst of 2 048 documents: 1.11e-3 -> 2.4e-4) for -0.3 %;
                                 wo / wgu / wdown stay bf16.                                                                             */
} lrx_encoder_config;

/* Per-layer weights, bf16 (precise_stream = 2: wqkv / wo / wgu / wdown as fp16; = 3: wqkv as fp16), nn.Linear layout [out, in] row-major (K contiguous).
 *   wqkv  [(nq + 2 nkv) * d, H]   rows = q_proj | k_proj | v_proj concatenated, the d rows of every q and k head in ROTARY-PAIR order:
 *                                 physical row 32 g + 16 i + t of a head = logical row i * d/2 + 16 g + t  (g < d/32, i < 2, t < 16), so that
 *                                 the fused QKV epilogue finds x_j and x_{j + d/2} in one lane and rotates on the fp32 accumulators; q and k
 *                                 leave the projection in the same order (q . k is invariant), v rows are in logical order
 *   wo    [H, nq * d]
 *   wgu   [2 * I, H]              gate/up interleaved in 16-row groups: rows [32j,32j+16) = gate[16j..], [32j+16,32j+32) = up[16j..]
 *   wdown [H, I]
 *   ln1, ln2 [H] bf16 (input_layernorm, post_attention_layernorm); bqkv [(nq+2nkv)*d] bf16 (same row order as wqkv) or NULL */
typedef struct lrx_layer_weights {
  const void* wqkv;
  const void* bqkv;
  const void* wo;
  const void* wgu;
  const void* wdown;
  const void* ln1;
  const void* ln2;
} lrx_layer_weights;

typedef struct lrx_encoder_weights {
  const void* embed;             /* [V, H] bf16 */
  const void* final_norm;        /* [H] bf16 */
  const float* rope_cos;         /* [max_positions, d/2] fp32: cos(position * inv_freq), the values LlamaRotaryEmbedding computes in fp32 */
  const float* rope_sin;
  const lrx_layer_weights* layers; /* HOST array of num_layers structs (device pointers inside) */
} lrx_encoder_weights;

/* What torch.ops.lrx.encode_packed takes as its `weights` argument: the address of one of these (both structs owned, and kept
 * alive, by whoever built them -- LrxEncoder.handle on the Python side).                                                       */
typedef struct lrx_encoder_handle {
  const lrx_encoder_config* cfg;
  const lrx_encoder_weights* w;
} lrx_encoder_handle;

/* Workspace (device bytes) needed by lrx_encode_packed for `total_tokens` packed tokens in `n_seqs` sequences. */
size_t lrx_encode_workspace_bytes(const lrx_encoder_config* cfg, int32_t total_tokens, int32_t n_seqs);

/* Document-side encoder forward on a packed batch.
 * Replaces: HybridModel.encode_passage dense branch (finetune/modeling_hybrid.py:205-278) including the HF
 * LlamaModel/Qwen2Model forward it calls (:248-260), utils/nested_input.py:114-166 (packing: the packed layout is
 * native here), finetune/dense_pooling.py:48-55 ('lasttoken'), the MRL slice and F.normalize (:272-278).
 *   ids        [total_tokens] int32 token ids, sequences back to back
 *   cu_seqlens [n_seqs + 1] int32, cu_seqlens[0] = 0, cu_seqlens[n_seqs] = total_tokens; every sequence non-empty
 *   out        fp32 rows, row b at out + b * out_row_stride, out_dim (<= H) floats each: the L2-normalised
 *              (if normalize != 0) last-token embedding, first out_dim dims (dense_shrink_dim / MRL).  May point
 *              directly into the index shard (the encoder writes in place; no host round trip).
 * max_seqlen: upper bound on any sequence length (<= cfg->max_positions).                                       */
int lrx_encode_packed(const lrx_encoder_config* cfg, const lrx_encoder_weights* w, const int32_t* ids,
                      const int32_t* cu_seqlens, int32_t n_seqs, int32_t total_tokens, int32_t max_seqlen,
                      float* out, int64_t out_row_stride, int32_t out_dim, int32_t normalize, void* workspace,
                      size_t workspace_bytes, void* stream);
/* The same with `out` = rows of an index shard: the last kernel also writes the rows' fp16 shadow (shadow_out = base of the shard's tiled
 * shadow, `out` row b = its row shadow_row0 + b: layout at lrx_shard_commit_rows; NULL = none; needs out_dim % 64 == 0) and raises the shard's
 * bounds (row_bounds, see lrx_shard_commit_rows; NULL = none), so the index needs no second pass over what the encoder just wrote
 * (FaissIndex.build's add, retriever/faiss_index.py:45-58).                                                                       */
int lrx_encode_packed_shard(const lrx_encoder_config* cfg, const lrx_encoder_weights* w, const int32_t* ids,
                            const int32_t* cu_seqlens, int32_t n_seqs, int32_t total_tokens, int32_t max_seqlen,
                            float* out, int64_t out_row_stride, int32_t out_dim, int32_t normalize, void* shadow_out,
                            int64_t shadow_row0, float* row_bounds, void* workspace, size_t workspace_bytes, void* stream);

/* Same forward, but returns the un-pooled final hidden states (after the final RMSNorm), bf16 [total_tokens, H]:
 * the `last_hidden_state` of lm(...) at finetune/modeling_hybrid.py:260.  Used by EmbeddingBag construction
 * (finetune/nonctx_emb_utils.py:296-306 takes last_hidden_state[:, -1]) and by tests.                           */
int lrx_encode_hidden(const lrx_encoder_config* cfg, const lrx_encoder_weights* w, const int32_t* ids,
                      const int32_t* cu_seqlens, int32_t n_seqs, int32_t total_tokens, int32_t max_seqlen,
                      void* hidden_out_bf16, void* workspace, size_t workspace_bytes, void* stream);

/* Shared-prefix encode.  Replaces the inner loop of construct_embedding_bag (finetune/nonctx_emb_utils.py:262-306: for every
 * vocabulary token run the LM on [bos] + prompt + [tok] + [eos] and keep last_hidden_state[:, -1]): all n_seqs sequences share
 * the same prefix_ids [prefix_len]; sequence i continues with suffix_ids[i*suffix_len .. +suffix_len).  The prefix is encoded
 * once (its per-layer K/V are captured), only the suffix tokens run through the layers.  out: fp32 rows [n_seqs, out_dim], the
 * final-norm hidden state of each sequence's LAST token (normalize = 0 for the EmbeddingBag table).                          */
size_t lrx_encode_prefixed_workspace_bytes(const lrx_encoder_config* cfg, int32_t prefix_len, int32_t n_seqs, int32_t suffix_len);
int lrx_encode_prefixed(const lrx_encoder_config* cfg, const lrx_encoder_weights* w, const int32_t* prefix_ids,
                        int32_t prefix_len, const int32_t* suffix_ids, int32_t n_seqs, int32_t suffix_len, float* out,
                        int64_t out_row_stride, int32_t out_dim, int32_t normalize, void* workspace,
                        size_t workspace_bytes, void* stream);

/* (ABI 8) The same with the pooling strategy of finetune/dense_pooling.py:12-82 as an argument (`--pooling_strategy`; the released models use
 * 'lasttoken', which is what the two entry points above compute): */
#define LRX_POOL_LASTTOKEN 0       /* the sequence's last token (dense_pooling.py:48-55) */
#define LRX_POOL_CLS 1             /* its first token (:32-33) */
#define LRX_POOL_MEAN 2            /* mean of the final-norm rows of all its tokens (:35-36), fp32, tokens added in order */
#define LRX_POOL_SECOND_TO_LAST 3  /* token len - 2 (:57-67) */
#define LRX_POOL_THIRD_TO_LAST 4   /* token len - 3 (:69-79) */
#define LRX_POOL_AVG_FIRST_LAST 5  /* mean over the tokens of (hidden_states[0] + hidden_states[-1]) / 2: the embedding rows and the final-norm rows (:38-41) */
#define LRX_POOL_AVG_TOP2 6        /* ... of (hidden_states[-2] + hidden_states[-1]) / 2: the stream before the final layer and the final-norm rows (:43-46) */
/* LASTTOKEN runs the final layer's O-projection / MLP on the pooled rows only; every other strategy runs all layers over all tokens and pools
 * from the residual stream (final norm inside the pooling kernel, fp32 when the stream is).  A sequence shorter than its strategy needs (the
 * reference asserts there) gets a zero row and raises lrx_device_error_count; an empty sequence (cu_seqlens[b + 1] <= cu_seqlens[b]) is too
 * short for every strategy, LASTTOKEN included, here and in lrx_pool_norm_mode, and lrx_gather_last_rows / lrx_scatter_last_rows answer it
 * with a zero row / with no write and the same counter (cu_seqlens lives on the device: only the kernels can see it).  The two-layer strategies add one column-sum pass over the other
 * hidden state (the embedding rows; the stream as it enters the final layer) -- served here only: lrx_pool_norm_mode sees one hidden state. */
int lrx_encode_packed_pooled(const lrx_encoder_config* cfg, const lrx_encoder_weights* w, const int32_t* ids,
                             const int32_t* cu_seqlens, int32_t n_seqs, int32_t total_tokens, int32_t max_seqlen, int32_t pooling,
                             float* out, int64_t out_row_stride, int32_t out_dim, int32_t normalize, void* shadow_out,
                             int64_t shadow_row0, float* row_bounds, void* workspace, size_t workspace_bytes, void* stream);

/* Dense + sparse document vectors in one pass.  Replaces HybridModel.encode_passage with encode_sparse
 * (finetune/modeling_hybrid.py:248-323): LM forward -> dense_reps (as lrx_encode_packed; dense_out may be NULL) and
 * sparse_reps = sparsify(max over the tokens tok_mask selects of hidden_t . lm_head^T)  (aggregate, sparse_pooling.py:244-278;
 * MaxLinearMapperFunction, utils/max_linear_map.py:8-88; get_sparse_emb, modeling_hybrid.py:176-203).
 * lm_head: bf16 [vocab, hidden] (NULL = tied to the embedding matrix), lm_head_bias: bf16 [vocab] or NULL.
 * tok_mask: uint8 [total_tokens] = get_sparse_attention_mask at the valid tokens (NULL = drop each sequence's first and last
 * token).  sparse_out: fp32 [n_seqs, sparse_row_stride >= vocab]; a sequence without any selected token gets finfo(bf16).min
 * before relu, like the reference.  round_bf16 = 1: log1p's result is rounded to bf16 (the tensor is bf16 in a bf16 run).   */
int lrx_encode_packed_sparse(const lrx_encoder_config* cfg, const lrx_encoder_weights* w, const void* lm_head,
                             const void* lm_head_bias, const int32_t* ids, const int32_t* cu_seqlens,
                             const uint8_t* tok_mask, int32_t n_seqs, int32_t total_tokens, int32_t max_seqlen,
                             float* dense_out, int64_t dense_row_stride, int32_t dense_dim, int32_t normalize,
                             float* sparse_out, int64_t sparse_row_stride, int32_t relu, int32_t log1p, int32_t round_bf16,
                             int32_t top_k, int32_t min_tokens_to_keep, void* workspace, size_t workspace_bytes, void* stream);

/* Per-kernel-class timing of the lrx_encode_* calls made since lrx_set_profiling / the previous lrx_get_profile: HIP events
 * are recorded on `stream` around every launch of the selected classes; nothing synchronises until lrx_get_profile reads
 * them (it waits for the recorded events, accumulates, and resets).  lrx_set_profiling(0) off, (1) every class, otherwise
 * bit (c + 1) of the argument selects class c (e.g. 1 << 3 = only the gate-up GEMM).
 * classes: 0 gemm/store (qkv), 1 gemm/residual (o, down), 2 gemm/swiglu (gate-up), 3 attention, 4 rmsnorm, 5 rope,
 * 6 other (embedding gather, positions, pool), 7 gemm_maxagg (LM-head GEMM with the max-aggregation epilogue).  Arrays of LRX_PROF_CLASSES entries; flops are algorithmic
 * (2*M*N*K for GEMMs, 2*2*d*sum_s(s*(s+1)/2)*nq for causal attention), 0 for the memory-bound classes.            */
#define LRX_PROF_CLASSES 8
void lrx_set_profiling(int32_t enabled);
/* (ABI 5) Measurement aids.  lrx_trace_marker: an empty kernel named k_trace_marker<id> (id 0..3) on `stream` -- delimits a region of a
 * rocprofv3 kernel trace (tools/check_trace_clean.py).  lrx_probe_stream_read: n_workgroups workgroups stream `bytes` (a multiple of 16)
 * of `buf` with 16-B loads and xor everything into sink[n_workgroups] (device, uint32): bytes / its duration = the read rate this box
 * reaches, the in-run ceiling bench.py reports next to the 8 TB/s of the spec.                                                    */
int lrx_trace_marker(int32_t id, void* stream);
int lrx_probe_stream_read(const void* buf, size_t bytes, uint32_t* sink, int32_t n_workgroups, void* stream);
int lrx_get_profile(float* ms, double* flops, int32_t* launches);

/* ------------------------------------------------------------------------------------------------------------
 * Individual kernels (unit-tested one by one against the oracle; same arithmetic the fused path uses)
 * ---------------------------------------------------------------------------------------------------------- */

/* out[t,:] = table[ids[t],:]  (nn.Embedding inside LlamaModel.forward)  bf16.  An id outside [0, vocab) never reaches the table: its
 * row is zero-filled and a device-side counter is raised (lrx_device_error_count).                                               */
int lrx_embedding_gather(const void* table, const int32_t* ids, int32_t n_tokens, int32_t hidden, int32_t vocab, void* out,
                         void* stream);
/* Number of out-of-range token ids any embedding gather (stand-alone or inside lrx_encode_*) has met since the last reset, plus the
 * attention work lists whose builder ran out of room (lrx_attn_build_items: their launches then compute nothing), plus the sequences
 * that were empty or shorter than their pooling strategy needs (lrx_pool_norm_mode, the last-row gathers and scatter), plus the candidate
 * entries >= n_rows that lrx_flat_ip_rerank / lrx_sq_fp16_ip_rerank skipped, plus what lrx_ivf_flat_ip_search / lrx_ivf_pq_ip_search /
 * lrx_ivf_sq_fp16_ip_search / lrx_ivf_sq_fp16_encode_rows / lrx_ivf_sq8_ip_search / lrx_ivf_sq8_encode_rows / lrx_ivf_sq8_decode_rows count (probe entries >= nlist, queries over max_scan_rows, stored rows outside the
 * shard, rows encoded for a cell outside [0, nlist)), plus the rows outside [0, n_bits) that lrx_selector_set_rows skipped, plus the entry-list
 * and graph-table entries >= n_rows that lrx_graph_ip_search skipped (one per time such an entry is met); -1 if the read
 * failed.  Non-zero = the rows of those calls are not the model's.  SYNCHRONISES the device (a blocking copy): call it at a point where
 * the caller waits for results anyway (LrxExactSearchModel.encode does, once per encode call, and raises).                         */
int64_t lrx_device_error_count(int32_t reset);
/* (ABI 6) Measurement aid of DEV builds (-DLRX_DEV_KNOBS; the shipping library reads no environment variable and records nothing): with
 * LRX_FUSED_PHASES bit 7 set in the environment the fused filter launch of the bounded search (sample + selection
 * + main pass in one persistent kernel) records per-workgroup phase timestamps (100 MHz clock; 8 words per workgroup: start, sample done,
 * selection start, selection done, first main K loop done, thresholds seen, ..., end); this copies the first n_words of them to the host.     */
int lrx_probe_fused_timestamps(uint64_t* out, int32_t n_words);
/* (ABI 5) fp16 range events since the last reset: q|k|v elements of the fused QKV + RoPE epilogue and fp16-shadow elements of pooled rows
 * that were beyond +-65504 and were stored as +-65504, or NaN and were stored as -65504 (counted once per wave instruction that saw any, so "0 or not" is
 * the meaningful reading).  0 on every checkpoint whose q|k|v stay inside fp16's range -- the precondition of the fp16 attention path;
 * a non-zero count means the embeddings of that call are not the model's.  -1 if the read failed.  SYNCHRONISES like the call above. */
int64_t lrx_device_saturation_count(int32_t reset);

/* LlamaRMSNorm (modeling_llama.py:53-67): y = w * bf16(x * rsqrt(mean(x^2) + eps)); x, w, y bf16; rows x hidden */
int lrx_rmsnorm(const void* x, const void* w, void* y, int32_t rows, int32_t hidden, float eps, void* stream);

/* C[M,N] = A[M,K] * B[N,K]^T, bf16 in, fp32 accumulate, bf16 out.  K % 64 == 0, N % 8 == 0.
 *   epilogue 0: C = acc (+ bias[n] if bias != NULL)          ldc = N
 *   epilogue 1: C = acc + resid[m,n]  (resid may alias C)    ldc = N
 *   epilogue 2: SwiGLU on gate/up-interleaved B (see wgu):   C[M, N/2] = silu(gate) * up, ldc = N/2           */
int lrx_gemm_bf16_nt(const void* A, const void* B, void* C, const void* bias, const void* resid, int32_t M,
                     int32_t N, int32_t K, int32_t epilogue, void* stream);

/* Fused QKV projection + rotary embedding: C[M, (nq+2nkv)*d] = A[M,K] * Wqkv^T (+ bias), then apply_rotary_pos_emb
 * (modeling_llama.py:130-160) on the q and k column blocks, on the fp32 accumulators with the fp32 cos/sin table (one rounding); v columns
 * are stored unrotated.  Wqkv / bias rows of the q and k heads in rotary-pair order (lrx_layer_weights); C is FP16 (saturating at
 * +-65504; 11 significant bits for both operands of q . k), q and k columns in the same pair order.                                */
int lrx_gemm_qkv_rope(const void* A, const void* Wqkv, void* C, const void* bias, const int32_t* positions,
                      const float* cos, const float* sin, int32_t M, int32_t K, int32_t num_q_heads,
                      int32_t num_kv_heads, int32_t head_dim, void* stream);

/* positions[t] = t - cu_seqlens[seq(t)] */
int lrx_build_positions(const int32_t* cu_seqlens, int32_t n_seqs, int32_t total_tokens, int32_t* positions, void* stream);

/* Varlen causal GQA attention (flash_attention_2 varlen call the reference requires for packing,
 * utils/nested_input.py:137-146): out[T, nq*d] bf16 = softmax(q k^T / sqrt(d), causal within each sequence) v.
 * qkv [T, (nq + 2 nkv) * d] FP16 as lrx_gemm_qkv_rope writes it (probabilities are rounded to fp16 too; fp32 accumulation).
 * last_tile_only != 0: only the 64-row q tile that holds each sequence's LAST token is computed (other rows of `out`
 * are left untouched) -- all the pooled path needs from the final layer.
 * A sequence's rows are addressed through one buffer descriptor: max_seqlen x (nq + 2 nkv) x d x 2 B must stay below 2 GiB
 * (>= 174 k tokens at 32 / 8 heads of 128, beyond every supported max_positions), else LRX_ERR_INVALID.        */
int lrx_attn_varlen_causal(const void* qkv, const int32_t* cu_seqlens, int32_t n_seqs, int32_t total_tokens,
                           int32_t max_seqlen, int32_t num_q_heads, int32_t num_kv_heads, int32_t head_dim,
                           void* out, int32_t last_tile_only, void* stream);

/* The same attention on a prebuilt WORK LIST (ABI 7): which (sequence, kv head, q tile) each persistent workgroup computes, and in which
 * order, depends on cu_seqlens and the head layout only, so the encoder builds it once per batch and every layer's launch reads it
 * (lrx_encode_* do this inside their workspace).  Results are bit-identical to lrx_attn_varlen_causal; the launch is ~5 % shorter on
 * the tiled path at head_dim 128 (0.95 against 1.00 ms at 32 / 8 heads, 256 x 512 tokens: the items are not derived per workgroup,
 * DESIGN.md 5.2).
 *   lrx_attn_items_bytes   size of the list; bounded by (total_tokens / 64 + n_seqs) x kv heads and non-decreasing in total_tokens and
 *                          max_seqlen (size once with the largest batch / longest sequence the caller will ever pass)
 *   lrx_attn_build_items   fills `items` (device memory, 16-byte aligned) on `stream`; one list per (cu_seqlens, max_seqlen, head
 *                          layout, last_tile_only) -- a list built with other arguments than the launch's gives wrong results.  Launches
 *                          nothing when the launch with the same arguments would not read a list (the K/V-resident geometries below).
 *                          At most 1024 persistent workgroups are planned (the builder is one block), whatever the CU count
 *   lrx_attn_varlen_causal_items   the launch (lrx_attn_varlen_causal's arguments + the list, which must not be NULL); `items` must stay
 *                          untouched until it has run.  Geometries served by the K/V-resident kernel (head_dim 64, max_seqlen <= 512)
 *                          do not read the list.                                                                                          */
size_t lrx_attn_items_bytes(int32_t n_seqs, int32_t total_tokens, int32_t max_seqlen, int32_t num_q_heads, int32_t num_kv_heads,
                            int32_t head_dim, int32_t last_tile_only);
int lrx_attn_build_items(const int32_t* cu_seqlens, int32_t n_seqs, int32_t total_tokens, int32_t max_seqlen, int32_t num_q_heads,
                         int32_t num_kv_heads, int32_t head_dim, int32_t last_tile_only, void* items, size_t items_bytes, void* stream);
int lrx_attn_varlen_causal_items(const void* qkv, const int32_t* cu_seqlens, const void* items, size_t items_bytes, int32_t n_seqs,
                                 int32_t total_tokens, int32_t max_seqlen, int32_t num_q_heads, int32_t num_kv_heads, int32_t head_dim,
                                 void* out, int32_t last_tile_only, void* stream);
/* Diagnostics: how many list builds (since the library was loaded) found their buffer too small -- 0 as long as the buffers come from
 * lrx_attn_items_bytes; such a build leaves an empty list (the launch then computes nothing).  Synchronises the device.                    */
int lrx_debug_attn_items_overflow(int32_t* count);

/* Attention of suffix queries over a shared prefix: qkv [n_seqs*suffix_len, (nq+2nkv)*d] (RoPE applied), prefix_kv
 * [prefix_len, 2*nkv*d] (k block | v block of one layer, RoPE applied); query j of a sequence sees the prefix keys and its own
 * suffix keys 0..j.  qkv and prefix_kv FP16 (lrx_gemm_qkv_rope output), out [n_seqs*suffix_len, nq*d] bf16.                    */
int lrx_attn_prefix_suffix(const void* qkv, const void* prefix_kv, int32_t n_seqs, int32_t suffix_len, int32_t prefix_len,
                           int32_t num_q_heads, int32_t num_kv_heads, int32_t head_dim, void* out, void* stream);

/* cu_seqlens[i] = i*len (i = 0..n_seqs), positions[t] = position_offset + t % len : equal-length batch layout built on device */
int lrx_uniform_layout(int32_t* cu_seqlens, int32_t* positions, int32_t n_seqs, int32_t len, int32_t position_offset, void* stream);

/* out[b, v] = max(finfo(bf16).min, max over tokens t of sequence b with tok_mask[t] of bf16(hidden[t,:] . lm_head[v,:] + bias[v])).
 * hidden bf16 [total_tokens, hidden_size] (hidden_size % 64 == 0), lm_head bf16 [vocab_size, hidden_size], out fp32
 * [n_seqs, out_row_stride]; row_seg_workspace: int32 [total_tokens] scratch.  The [tokens, vocab] logits are never written:
 * the maximum is taken per 256x256 tile in the GEMM epilogue and merged with integer atomics.                               */
int lrx_sparse_max_aggregate(const void* hidden, const void* lm_head, const void* bias, const int32_t* cu_seqlens,
                             const uint8_t* tok_mask, int32_t n_seqs, int32_t total_tokens, int32_t hidden_size,
                             int32_t vocab_size, float* out, int64_t out_row_stride, int32_t* row_seg_workspace, void* stream);

/* In place on fp32 [n_rows, row_stride]: relu -> log1p (-> bf16 rounding) -> top-k threshold (entries below the k-th largest
 * value of the row become 0, ties survive; k = max(top_k, min_tokens_to_keep); top_k = 0 disables)  (sparse_pooling.py:92-109). */
int lrx_sparsify(float* reps, int32_t n_rows, int32_t vocab_size, int64_t row_stride, int32_t relu, int32_t log1p,
                 int32_t round_bf16, int32_t top_k, int32_t min_tokens_to_keep, void* stream);

/* Quantise + compact (sparse_converter_mixin.py:129-137): per row the token ids whose round-half-even(max(x,0) * q) != 0, in
 * ascending id order, with that integer weight: ids_out / weights_out int32 [n_rows, capacity] (first `capacity` kept),
 * counts_out int32 [n_rows] = true number of non-zeros.                                                                    */
int lrx_sparse_compact(const float* reps, int32_t n_rows, int32_t vocab_size, int64_t row_stride, int32_t quantization_factor,
                       int32_t capacity, int32_t* ids_out, int32_t* weights_out, int32_t* counts_out, void* stream);

/* (added in ABI 8, additively) The same quantise + compact as ragged CSR, without a capacity: two launches around an exclusive scan of
 * the counts, which is the caller's (row_off[0] = 0, row_off[b + 1] = row_off[b] + counts_out[b]).
 *   lrx_sparse_csr_count: counts_out int32 [n_rows] = number of v with round-half-even(max(x[b, v], 0) * q) != 0 (fp32 arithmetic, the
 *                         arithmetic of lrx_sparse_compact); a row without any counts 1 when empty_marker != 0.
 *   lrx_sparse_csr_fill:  terms_out / weights_out int32 [row_off[n_rows]]: row b's (token id, weight) pairs at [row_off[b], row_off[b + 1])
 *                         in ascending id order; a row without any holds the single pair (vocab_size, 1) when empty_marker != 0 -- the
 *                         device form of the reference's {"-1": 1} (sparse_converter_mixin.py), an ordinary term.  Nothing is written
 *                         outside a row's range; the outputs need no clearing.
 * Each launch streams the [n_rows, vocab_size] fp32 rows once (16-byte loads when reps and row_stride * 4 are 16-byte aligned).            */
int lrx_sparse_csr_count(const float* reps, int32_t n_rows, int32_t vocab_size, int64_t row_stride, int32_t quantization_factor,
                         int32_t empty_marker, int32_t* counts_out, void* stream);
int lrx_sparse_csr_fill(const float* reps, int32_t n_rows, int32_t vocab_size, int64_t row_stride, int32_t quantization_factor,
                        int32_t empty_marker, const int64_t* row_off, int32_t* terms_out, int32_t* weights_out, void* stream);

/* Hit-list fusion (retriever/score_fuse_utils.py:3-91 on arrays; IEEE double like the reference's numpy float64).
 * Stage 1, one retrieval system: scores f64 / ids i64 [n_queries, k] (id < 0 = empty slot) -> contribution per entry:
 *   method 0 (fuse_scores_rrf):    1 / (param0 + rank), rank 1 = highest score of the row;
 *   method 1 (fuse_scores_linear): param0 * (s - min) / (max - min + param1), min/max over the row's valid entries.
 * Stage 2: the systems' (ids, contributions) concatenated per query in system order [n_queries, n_entries] -> union by id,
 * contributions of one id summed in system order, rows sorted by fused score (descending, lower id first among equals):
 * scores_out f64 / ids_out i64 [n_queries, n_entries] (-inf / -1 beyond counts_out[q]).  k, n_entries <= 4096.             */
int lrx_hit_contributions(const double* scores, const int64_t* ids, int32_t n_queries, int32_t k, int64_t row_stride,
                          int32_t method, double param0, double param1, double* contrib_out, int64_t contrib_row_stride,
                          void* stream);
int lrx_hit_union(const int64_t* ids, const double* contrib, int32_t n_queries, int32_t n_entries, int64_t row_stride,
                  double* scores_out, int64_t* ids_out, int32_t* counts_out, void* stream);

/* GEMMs with the folded-RMSNorm hooks: rscale [M] fp32 or NULL -- accumulator row m times rscale[m] before bias / RoPE / SwiGLU
 * (store and SwiGLU epilogues); ss_part [ceil(N/256), M] fp32 or NULL -- residual epilogue: sum of squares of the output row's
 * columns of each 256-wide n-tile, written (not accumulated) to slot [tile, m].                                                  */
int lrx_gemm_bf16_nt_fused(const void* A, const void* B, void* C, const void* bias, const void* resid, int32_t M, int32_t N,
                           int32_t K, int32_t epilogue, const float* rscale, float* ss_part, void* stream);
int lrx_gemm_qkv_rope_fused(const void* A, const void* Wqkv, void* C, const void* bias, const int32_t* positions,
                            const float* cos, const float* sin, int32_t M, int32_t K, int32_t num_q_heads,
                            int32_t num_kv_heads, int32_t head_dim, const float* rscale, void* stream);
/* (ABI 6) heads [head0, head0 + n_heads) of the fused projection -- numbered q_0 .. q_{nq-1}, k_0 .. k_{nkv-1}, v_0 .. v_{nkv-1} -- from that
 * row slice of Wqkv / bias into that column slice of C (rows of C keep the full (nq + 2 nkv) * d width).  lrx_encode_packed uses it in the
 * FINAL layer: k|v for every token, q only for the gathered last-token rows (the only q rows the pooled output depends on).            */
int lrx_gemm_qkv_rope_slice(const void* A, const void* Wqkv, void* C, const void* bias, const int32_t* positions,
                            const float* cos, const float* sin, int32_t M, int32_t K, int32_t num_q_heads,
                            int32_t num_kv_heads, int32_t head_dim, const float* rscale, int32_t head0, int32_t n_heads, void* stream);
/* Precise residual stream (lrx_encoder_config.precise_stream).  x32[M, N] (fp32, in place) += A[M, K] * B[N, K]^T; a16_out (bf16 [M, N],
 * may be NULL) = bf16(x32 * gamma[n]) (gamma bf16 [N], NULL = 1): the next projection's operand; ss_part as above, from the fp32 row.   */
int lrx_gemm_bf16_nt_resid32(const void* A, const void* B, float* x32, void* a16_out, const void* gamma, int32_t M, int32_t N,
                             int32_t K, float* ss_part, void* stream);
/* ... its start: x32[t, :] = table[ids[t], :], a16[t, :] = bf16(x32 * gamma), rscale_out[t] = rsqrt(mean(x32^2) + eps)              */
int lrx_embed_stream32(const void* table, const int32_t* ids, int32_t n_tokens, int32_t hidden, int32_t vocab, const void* gamma,
                       float* x32, void* a16, float* rscale_out, float eps, void* stream);
/* ... and its end: y bf16 = w * x32 * rsqrt(mean(x32^2) + eps), one rounding                                                         */
int lrx_rmsnorm_f32(const float* x, const void* w, void* y, int32_t rows, int32_t hidden, float eps, void* stream);
/* rscale_out[r] = rsqrt(mean(x[r,:]^2) + eps) for bf16 rows (LlamaRMSNorm's statistic, modeling_llama.py:53-67) */
int lrx_row_rscale(const void* x, int32_t rows, int32_t hidden_size, float eps, float* rscale_out, void* stream);
/* rscale_out[r] = rsqrt(sum_p ss_part[p, r] / hidden_size + eps), partials added in index order */
int lrx_finalize_rscale(const float* ss_part, int32_t n_parts, int32_t rows, int32_t hidden_size, float eps, float* rscale_out,
                        void* stream);

/* (added in ABI 9, additively) The FP16-OPERAND forms of the encoder kernels: what lrx_encode_* launches under lrx_encoder_config.precise_stream
 * = 2 (every projection) and = 3 (the QKV projection only), exported so that each can be tested on its own.  Each is the entry point named
 * with one or two format flags more; with every flag 0 it IS that entry point (same kernel, same bits).  "fp16 operand" means: the 16-bit
 * elements of that matrix are IEEE binary16 instead of bf16, multiplied on the f16 MFMA with fp32 accumulation; biases, norm weights (gamma)
 * and the embedding table stay bf16 in every mode.
 * The fp16 STORE RULE of the GEMM and embedding outputs: one rounding (to nearest even) of the fp32 value, SATURATING -- a value beyond
 * +-65504 is stored as +-65504 by sign, a NaN as -65504 -- and every such event is counted by lrx_device_saturation_count (the GEMMs: once per
 * wave instruction that saw any; the embedding: once per element).  No inf and no NaN is ever stored.
 *   lrx_gemm_nt_fused_ex        lrx_gemm_bf16_nt_fused; f16 != 0: A and B are fp16 and C [M, N / 2] is written as fp16 under the store rule.
 *                               Served for epilogue 2 (SwiGLU) only: f16 != 0 with epilogue 0 or 1 is LRX_ERR_INVALID, nothing is written.
 *   lrx_gemm_qkv_rope_slice_ex  lrx_gemm_qkv_rope_slice; f16 != 0: A and Wqkv are fp16 (bias bf16, rscale / cos / sin fp32).  C is fp16 under
 *                               the store rule either way.
 *   lrx_gemm_nt_resid32_ex      lrx_gemm_bf16_nt_resid32; f16 != 0: A and B are fp16 (x32 fp32 and gamma bf16 as before); out_f16 != 0:
 *                               a16_out = fp16(x32 * gamma[n]) under the store rule instead of bf16(..).  The two flags are independent
 *                               except that fp16 operands never write a bf16 operand: f16 != 0 with out_f16 == 0 and a16_out != NULL is
 *                               LRX_ERR_INVALID, nothing is written.  (precise_stream = 3 runs its down-projection with f16 = 0, out_f16 = 1.)
 *   lrx_embed_stream32_ex       lrx_embed_stream32; f16 != 0: a16 = fp16(x32 * gamma) under the store rule (the product of two bf16 numbers is
 *                               exact in fp32: one rounding in all).  x32 and rscale_out do not depend on the flag.
 *   lrx_attn_varlen_causal_ex   lrx_attn_varlen_causal (items == NULL, items_bytes ignored) / lrx_attn_varlen_causal_items (items != NULL);
 *                               out_f16 != 0: `out` is written as fp16.
 *   lrx_attn_prefix_suffix_ex   lrx_attn_prefix_suffix; out_f16 != 0: `out` is written as fp16.
 * The attention store is one rounding of the fp32 value and is NOT saturating: a row of the output is a convex combination of rows of v,
 * |o| <= max |v|, up to the rounding of the probabilities -- the kernels form (sum fp16(p_i) v_i) / (sum p_i), at most (1 + 2^-11) max |v| --
 * so it is finite for every max |v| <= 65472, the second largest fp16 number, and nothing is counted.  Only v = +-65504 itself can be stored
 * as inf; lrx_gemm_qkv_rope* writes that value only where it saturated, and counted it.  qkv / prefix_kv are fp16 in every mode.
 * Every other refusal is the one of the entry point without the flags.                                                                      */
int lrx_gemm_nt_fused_ex(const void* A, const void* B, void* C, const void* bias, const void* resid, int32_t M, int32_t N, int32_t K,
                         int32_t epilogue, const float* rscale, float* ss_part, int32_t f16, void* stream);
int lrx_gemm_qkv_rope_slice_ex(const void* A, const void* Wqkv, void* C, const void* bias, const int32_t* positions, const float* cos,
                               const float* sin, int32_t M, int32_t K, int32_t num_q_heads, int32_t num_kv_heads, int32_t head_dim,
                               const float* rscale, int32_t head0, int32_t n_heads, int32_t f16, void* stream);
int lrx_gemm_nt_resid32_ex(const void* A, const void* B, float* x32, void* a16_out, const void* gamma, int32_t M, int32_t N, int32_t K,
                           float* ss_part, int32_t f16, int32_t out_f16, void* stream);
int lrx_embed_stream32_ex(const void* table, const int32_t* ids, int32_t n_tokens, int32_t hidden, int32_t vocab, const void* gamma,
                          float* x32, void* a16, float* rscale_out, float eps, int32_t f16, void* stream);
int lrx_attn_varlen_causal_ex(const void* qkv, const int32_t* cu_seqlens, const void* items, size_t items_bytes, int32_t n_seqs,
                              int32_t total_tokens, int32_t max_seqlen, int32_t num_q_heads, int32_t num_kv_heads, int32_t head_dim,
                              void* out, int32_t last_tile_only, int32_t out_f16, void* stream);
int lrx_attn_prefix_suffix_ex(const void* qkv, const void* prefix_kv, int32_t n_seqs, int32_t suffix_len, int32_t prefix_len,
                              int32_t num_q_heads, int32_t num_kv_heads, int32_t head_dim, void* out, int32_t out_f16, void* stream);

/* dst[b, :] = src[cu_seqlens[b+1]-1, :]  (bf16 rows of `width` elements): the last-token rows, compacted. */
int lrx_gather_last_rows(const void* src, const int32_t* cu_seqlens, int32_t n_seqs, int32_t width, void* dst, void* stream);
/* (ABI 6) the inverse: dst[cu_seqlens[b+1]-1, 0:width] = src[b, 0:width]  (16-bit elements; rows of dst are dst_row_stride elements apart) */
int lrx_scatter_last_rows(const void* src, const int32_t* cu_seqlens, int32_t n_seqs, int32_t width, void* dst, int64_t dst_row_stride,
                          void* stream);

/* Last-token pooling + final RMSNorm on the pooled rows only + MRL slice + L2 normalise -> fp32 rows.
 * hidden = residual stream BEFORE the final norm [T, H] bf16; cu_seqlens == NULL means `hidden` already holds the
 * n_seqs pooled rows compacted ([n_seqs, H]).                                                                      */
int lrx_pool_norm(const void* hidden, const void* final_norm_w, const int32_t* cu_seqlens, int32_t n_seqs,
                  int32_t hidden_size, float eps, float* out, int64_t out_row_stride, int32_t out_dim,
                  int32_t normalize, void* stream);
/* ... and the shard maintenance fused into it: shadow_out (the shard's tiled fp16 shadow, row b of `out` = its row shadow_row0 + b; may be
 * NULL) and row_bounds (see lrx_shard_commit_rows; may be NULL).  hidden_f32 != 0: `hidden` holds fp32 rows (precise_stream), the norm
 * runs in fp32.                                                                                                                     */
int lrx_pool_norm_shard(const void* hidden, const void* final_norm_w, const int32_t* cu_seqlens, int32_t n_seqs,
                        int32_t hidden_size, float eps, float* out, int64_t out_row_stride, int32_t out_dim,
                        int32_t normalize, void* shadow_out, int64_t shadow_row0, float* row_bounds, int32_t hidden_f32, void* stream);

/* (ABI 8) ... and with the pooling strategy (LRX_POOL_LASTTOKEN .. LRX_POOL_THIRD_TO_LAST; cu_seqlens required for anything but LASTTOKEN): pooling(last_hidden, mask, strategy)
 * of finetune/dense_pooling.py:12-82 over `hidden` = the residual stream before the final norm, which runs inside (per pooled token). */
int lrx_pool_norm_mode(const void* hidden, const void* final_norm_w, const int32_t* cu_seqlens, int32_t n_seqs,
                       int32_t hidden_size, float eps, int32_t pooling, float* out, int64_t out_row_stride, int32_t out_dim,
                       int32_t normalize, void* shadow_out, int64_t shadow_row0, float* row_bounds, int32_t hidden_f32, void* stream);

/* Query side.  Replaces emb_bag.forward + slice + F.normalize at finetune/modeling_hybrid.py:472-490
 * (torch.nn.EmbeddingBag mode='mean', padding_idx) with inputs from tokenize_nonctx_qry_emb_bag
 * (finetune/nonctx_emb_utils.py:197-219).  table fp32 [V, H]; ids int64 [n_ids]; offsets int64 [n_bags];
 * padding_idx < 0 = none; empty bag -> zero row.  out fp32 [n_bags, out_dim].                                    */
int lrx_embedding_bag_mean(const float* table, int32_t vocab, int32_t hidden, const int64_t* ids, int64_t n_ids,
                           const int64_t* offsets, int32_t n_bags, int64_t padding_idx, float* out,
                           int64_t out_row_stride, int32_t out_dim, int32_t normalize, void* stream);

/* ------------------------------------------------------------------------------------------------------------
 * Flat inner-product index shard resident in HBM.  Replaces faiss.IndexFlatIP.search as called from
 * FaissIndex.search (retriever/faiss_index.py:27-40): exact fp32 scores, descending top-k, ids = row numbers
 * (+ id_base, so shards can return global rows), ties broken by lower row id, id -1 / score -FLT_MAX when k > N.
 *   X [N, D] fp32 row-major (row stride ldx floats), q [Q, D] fp32, D % 32 == 0, k <= 2048.
 * Memory: a shard that keeps the fp16 shadow below holds 6 bytes per element (fp32 rows + shadow: 1.5x the rows alone) -- BASELINE
 * config 3 (10M x 4096) on ONE 288-GB GPU is 164 + 82 GB + < 6 GB of workspace; row-sharded over 8 GPUs 31 GB each.
 * ---------------------------------------------------------------------------------------------------------- */
size_t lrx_flat_ip_workspace_bytes(int64_t n_rows, int32_t dim, int32_t n_queries, int32_t k);

/* One pass over the fp32 rows (six bf16 products = fp32-grade scores; the exact-fp32 MFMA for <= 32 queries) into a [Q, N] score
 * matrix, selection, exact rescoring (fp64 accumulation, one rounding).  The selection is rigorous: every row whose matrix score lies
 * within 2 eps6(q) = 2 (6 D + 8) 2^-23 |q| R of the k-th largest is rescored before the best k are returned (R = row_bounds[0] >=
 * max |x_row|).  row_bounds: DEVICE pointer to the shard's two bounds (lrx_shard_commit_rows) or NULL = not known: the rows are then
 * read once more to measure R.                                                                                                       */
int lrx_flat_ip_search(const float* X, int64_t n_rows, int64_t ldx, int32_t dim, const float* row_bounds, const float* q,
                       int32_t n_queries, int32_t k, int64_t id_base, float* out_scores, int64_t* out_ids, void* workspace,
                       size_t workspace_bytes, void* stream);

/* Same result as lrx_flat_ip_search (exact top-k, ids ascending among equal scores) at close to ONE pass over a 2-byte copy of the
 * shard and without a [queries, rows] score matrix, for shards whose rows satisfy the two bounds in row_bounds (DEVICE pointer to
 * two floats): row_bounds[0] >= max |x_row| and row_bounds[1] >= max |x_row - fp16(x_row)| (<= 0: unknown, 2^-11 * row_bounds[0] is
 * used).  lrx_shard_commit_rows / lrx_encode_packed_shard maintain both.  A single-product FP16 filter pass (fp16(q) . fp16(x), fp32
 * accumulation) bounds every score to +- eps(q) = |q - fp16(q)| R + |fp16(q)| E + (D+32) 2^-23 |fp16(q)| R (~7e-4 |q| R on normalised
 * rows; the bf16 filter of round 2 had 3.7e-3); a strided sample of the shard (every ss-th 128-row block, scored first) gives a lower
 * bound T' of the k-th largest filter score; the pass over the rest keeps only rows with filter score >= T' - 2 eps (a per-query
 * candidate list, ~1e-3 of the rows; capacity 64 k rounded up to a power of two, at least 64 Ki); the rows within 2 eps of the list's
 * k-th score are rescored exactly from the fp32 rows (fp64 accumulation, one rounding) and sorted.  Queries whose list or band
 * overflows (near-duplicate corpora, rows outside fp16's range) are redone by the six-product path (gated on a device flag, no host
 * sync).  Scores returned are the exactly rescored ones.  Bounds smaller than the true values void the guarantee.  row_bounds[1] <= 0
 * means "E not measured": the library then uses 2^-11 R + sqrt(dim) 2^-25, a bound for every shard with R <= 65504 (elements in fp16's
 * normal or subnormal range); with R > 65504 it uses E = R, i.e. every query takes the six-product path (exact, slower).
 * The CU count that sizes the persistent launches is cached per process for the device that was current at the first call.
 * X_shadow (optional, NULL = convert the fp32 rows on the fly: half the queries/s): the shard's TILED FP16 SHADOW kept by the caller
 * next to the fp32 rows -- round-to-nearest-even per element, saturating at +-65504; dim % 64 == 0; layout at lrx_shard_commit_rows;
 * row 0 of the array is the shard's row 0.
 * flags: LRX_SEARCH_FILTER_* below (A/B runs and tests; the result does not depend on it).  Per call -- there is no process-wide
 * search state, calls from several host threads (the reference's RPC server threads) do not interact.
 * Queries are processed in chunks of 256 (128 without X_shadow) over the same workspace, whose size therefore stops growing at
 * 256 queries: min(Q,128) * rows * 4 bytes for the gated fallback plus Q candidate lists.
 * dim has no upper limit here, nor in lrx_flat_ip_search, lrx_flat_ip_range_search, lrx_flat_ip_rerank and their lrx_sq_fp16_* forms:
 * query rows of up to 8192 floats are staged in LDS by the rescoring kernels, longer ones are read from global memory -- slower, the same
 * bits (served and tested at 8224 and 12288).  The inverted-file and graph entries refuse dim > 8192.                                 */
enum {
  LRX_SEARCH_FILTER_AUTO = 0,            /* score-free filter from 16 Ki rows on, score-matrix filter below                         */
  LRX_SEARCH_FILTER_MATRIX = 1,          /* always the score-matrix filter                                                           */
  LRX_SEARCH_FILTER_SCORE_FREE = 2,      /* the score-free (candidate-list) filter whenever the shard is large enough for a sample   */
  LRX_SEARCH_FILTER_SCORE_FREE_NO_GEMM = 3, /* like 2, but chunks of 129..256 queries never take the GEMM kernel for the main pass   */
  /* (ABI 6) OR-ed onto one of the above: the FUSED launch of the score-free filter -- sample pass, threshold selection and main pass in one
   * persistent kernel, for chunks of <= 128 queries over a shadow with dim % 256 == 0 -- is chosen by a measured rule (<= 16 queries, dim >= 512,
   * k <= 256, <= 8 blocks of 128 rows per CU: small query batches over a per-rank shard); these two bits force it on wherever it is eligible, or off */
  LRX_SEARCH_FUSED_ALWAYS = 4,
  LRX_SEARCH_FUSED_NEVER = 8,
  /* Exact rescoring of the band rows: per query (gather of its fp32 rows), or -- many queries x large k over a small shard, where every row
   * is wanted by several queries of a chunk -- grouped by ROW: each 16-row group staged once, the query rows streamed from L2; same bits.
   * Default: by a measured rule (rows of >= 8 KiB that a chunk of <= 256 queries wants >= 2.5 times: queries x k x 1.25 >= 2.5 x rows).
   * OR-able with the bits above; 16 | 32 is rejected.                                                                                     */
  LRX_SEARCH_REFINE_ROWS_ALWAYS = 16,
  LRX_SEARCH_REFINE_ROWS_NEVER = 32
};
size_t lrx_flat_ip_bounded_workspace_bytes(int64_t n_rows, int32_t dim, int32_t n_queries, int32_t k, int32_t flags);
int lrx_flat_ip_search_bounded(const float* X, int64_t n_rows, int64_t ldx, int32_t dim, const void* X_shadow, const float* row_bounds,
                               const float* q, int32_t n_queries, int32_t k, int64_t id_base, float* out_scores, int64_t* out_ids,
                               void* workspace, size_t workspace_bytes, int32_t flags, void* stream);
/* (ABI 5) The same search for a rank of a row-sharded index: besides (out_scores, out_ids) the LAST kernel of the chain also writes the
 * k results of every query as the 64-bit wire words of the exchange (out_wire [n_queries, k]; format and row_map as lrx_pack_topk
 * below), so nothing runs between the local search and the RCCL all-gather.  out_wire == NULL: identical to the call above.       */
int lrx_flat_ip_search_bounded_wire(const float* X, int64_t n_rows, int64_t ldx, int32_t dim, const void* X_shadow, const float* row_bounds,
                                    const float* q, int32_t n_queries, int32_t k, int64_t id_base, float* out_scores, int64_t* out_ids,
                                    const int64_t* row_map, uint64_t* out_wire, void* workspace, size_t workspace_bytes, int32_t flags,
                                    void* stream);
/* (ABI 5) Statistics for tools and bench legs.  lrx_search_fallback_count: queries any bounded search of this process has sent to its
 * exact six-product fallback since the last reset (list / band overflow: a performance event, the results are exact either way) -- and
 * the queries a range search sent to its score-matrix path because their candidate list overflowed;
 * SYNCHRONISES like lrx_device_error_count.  lrx_flat_ip_bounded_list_counts: counts_out[n_queries] (device, uint32) = candidate-list
 * entries of each query of the last chunk of the last search that used `workspace` -- the rows that passed the filter and reached the
 * refine step; pass that search's own (n_rows, dim, n_queries of that chunk, k, flags) and whether it had a shadow; zeros when that search
 * ran the score-matrix filter.  Asynchronous on `stream`.                                                                          */
int64_t lrx_search_fallback_count(int32_t reset);
/* (ABI 8) Queries per chunk the bounded search walks a call of `n_queries` in: 256 over a shadow (128 over fp32 rows), or -- where the main
 * pass runs on the GEMM kernel (shadow, dim >= 1024, score-free filter feasible) -- ONE pass over the shadow per up to 1024 queries (equal
 * chunks, a multiple of 16 each).  Callers that pipeline chunks themselves (FlatIPIndex.search) split at these boundaries.                */
int32_t lrx_flat_ip_bounded_chunk_queries(int64_t n_rows, int32_t dim, int32_t n_queries, int32_t k, int32_t flags, int32_t has_shadow);
int lrx_flat_ip_bounded_list_counts(const void* workspace, int64_t n_rows, int32_t dim, int32_t n_queries, int32_t k, int32_t flags,
                                    int32_t has_shadow, uint32_t* counts_out, void* stream);
/* (ABI 9) The stage state the last chunk of the last bounded search (flat or fp16-SQ) left in `workspace`, read-only: tests compare every
 * stage of the filter chain with an fp64 model.  Arguments as for lrx_flat_ip_bounded_list_counts + that search's ldx (dim for the
 * fp16-SQ index).  Copy kernels on `stream` only: no synchronisation, no allocation, nothing written to the workspace.
 *   plan_out    HOST int32[LRX_CHUNK_STATE_PLAN_INTS], filled before the call returns: {lists kept (score-free filter), fused launch, GEMM main
 *               pass, sample stride ss (every ss-th unit of rb rows is a sample unit), rb, list capacity, parts per query of the refine step,
 *               row-grouped rescoring, rows per entry of the sample's maxima (16 / 128), sample units, plain path (nothing else is written), 0}
 *   thr_eps_out device float[2 n_queries]: thr = T' - 2 eps as stored, then eps (zeros without lists)
 *   ints_out    device int32[3 n_queries + 8]: list count (uint32, raw: an overflowing list shows more than the capacity), flags, band size
 *               (sum of the parts' counts, -1 when a part reported overflow), then any_flag[8]
 *   entry_scores / entry_rows  device float / int64 [n_queries, max_entries]: the first min(count, capacity, max_entries) entries of each
 *               list as (fp32 filter score, row); the rest is left as the caller initialised it.  max_entries = 0: none.                       */
#define LRX_CHUNK_STATE_PLAN_INTS 12
int lrx_flat_ip_bounded_chunk_state(const void* workspace, int64_t n_rows, int32_t dim, int32_t n_queries, int32_t k, int32_t flags,
                                    int32_t has_shadow, int64_t ldx, int32_t* plan_out, float* thr_eps_out, int32_t* ints_out,
                                    int32_t max_entries, float* entry_scores, int64_t* entry_rows, void* stream);

/* (added in ABI 8, additively) Exact inner-product RANGE search (faiss IndexFlatIP::range_search): every row whose exact score -- the value
 * every search path reports, (float) of the fp64-accumulated sum of the fp32 products -- is STRICTLY greater than `radius`.  Result in faiss's
 * layout: lims[n_queries + 1] (device, int64; lims[0] = 0), query i's hits are out_scores / out_ids [lims[i], lims[i+1]) in ascending row
 * order, ids = id_base + row, scores bit-equal to what the top-k searches report.  Deterministic: the same arrays for any query batch size,
 * with or without X_shadow.  lims is always written and exact.  out_scores / out_ids are written only when the results fit `capacity`
 * (checked on the device): a call of up to one chunk of queries (256 with a shadow, 128 without) writes nothing to them when
 * lims[n_queries] > capacity and still returns LRX_OK -- read lims[n_queries] and call again with at least that capacity (as with
 * snprintf); a longer call checks chunk by chunk, so chunks that end within `capacity` may have been written.  Asynchronous on `stream`,
 * no host synchronisation.  X_shadow (tiled fp16 shadow, dim % 64 == 0) selects the candidate-list path: ONE pass over the shadow with
 * the threshold radius - eps(q), exact rescoring of the list; queries whose list overflows -- more than 64 Ki filter hits, or, at high hit density,
 * more hits in one step than a wave's LDS list holds (so possibly far fewer than 64 Ki) -- counted by
 * lrx_search_fallback_count -- and calls without a shadow, with dim % 64 != 0 or with <= 4096 rows take the score-matrix path (six-product
 * or exact-fp32 scores of <= 128 queries, exact rescoring of every row within 2 eps6(q) of the radius).  row_bounds as for
 * lrx_flat_ip_search_bounded; dim % 4 == 0; radius must not be NaN; workspace of lrx_flat_ip_range_workspace_bytes (grows with the
 * queries up to one chunk).                                                                                                          */
size_t lrx_flat_ip_range_workspace_bytes(int64_t n_rows, int32_t dim, int32_t n_queries, int32_t has_shadow);
int lrx_flat_ip_range_search(const float* X, int64_t n_rows, int64_t ldx, int32_t dim, const void* X_shadow, const float* row_bounds,
                             const float* q, int32_t n_queries, float radius, int64_t id_base, int64_t* lims, float* out_scores,
                             int64_t* out_ids, int64_t capacity, void* workspace, size_t workspace_bytes, void* stream);

/* (added in ABI 8, additively) RANGE search over the quantised and sparse indexes: the contract of lrx_flat_ip_range_search above -- lims /
 * out_scores / out_ids in faiss's layout, a row is in the result iff the score the index's own top-k search reports for it, bit for bit,
 * is strictly greater than `radius`; ids = id_base + row, ascending rows inside a query; exact, never truncated, deterministic (independent
 * of the query batch and of the path inside the library); lims always written; the outputs written only when lims[n_queries] <= capacity
 * (checked on the device; call again with at least lims[n_queries]).  radius must not be NaN; +inf gives an empty result; capacity >= 0;
 * out_scores / out_ids may be NULL only with capacity == 0.  n_rows == 0 or n_queries == 0: lims cleared, nothing launched.  Asynchronous
 * on `stream`, no host synchronisation.
 *
 * lrx_sq_fp16_ip_range_search  fp16 scalar-quantised index (codes / row_bounds / dim % 64 == 0 as for lrx_sq_fp16_ip_search below): the
 *     score is (float) of the fp64 sum of q_i * (float) c_i.  The chain is the flat one with the tiled codes in both roles -- ONE filter
 *     pass over the codes with the threshold radius - eps16(q), exact rescoring of the candidate lists from the codes; shards of <= 4096
 *     rows (the flat range search's rule, not the 16 Ki of the fp16-SQ top-k) and queries whose list overflowed (counted by lrx_search_fallback_count) take a one-product score matrix over the codes and
 *     the exact rescoring of every row within eps16(q) of the radius.  Capacity is checked per chunk of 256 queries, as in the flat call.
 * lrx_pq_ip_range_search       product-quantised index (arguments as for lrx_pq_ip_search): the score is the fp32 sum of the lookup table
 *     in ascending m, which the scan writes -- the predicate is applied to the scan's score matrix.
 * lrx_range_impact_search      impact index (arguments as for lrx_impact_search, the caller's overflow refusal included): a row is in the
 *     result iff it is a hit (S >= 1) and (float) S > radius; a negative radius returns every hit.
 *     (Named lrx_range_impact_*: the lrx_impact_* prefix is the top-k family's, and its tests pin that family to its three entry points.)
 * The last two run the scan driver twice (count per 4096-row segment, lims, scan again and fill in row order) and check `capacity` once for
 * the whole call.  row_chunk (trailing): rows per score matrix, 0 = the library's 4 Mi, otherwise a positive multiple of 128 -- for tests,
 * the result does not depend on it; pass the same value to the workspace function.                                                  */
size_t lrx_sq_fp16_ip_range_workspace_bytes(int64_t n_rows, int32_t dim, int32_t n_queries);
int lrx_sq_fp16_ip_range_search(const void* codes, int64_t n_rows, int32_t dim, const float* row_bounds, const float* q, int32_t n_queries,
                                float radius, int64_t id_base, int64_t* lims, float* out_scores, int64_t* out_ids, int64_t capacity,
                                void* workspace, size_t workspace_bytes, void* stream);
size_t lrx_pq_ip_range_workspace_bytes(int64_t n_rows, int32_t dim, int32_t M, int32_t n_queries, int64_t row_chunk);
int lrx_pq_ip_range_search(const void* codes, int64_t n_rows, const float* centroids, int32_t dim, int32_t M, const float* q, int32_t n_queries,
                           float radius, int64_t id_base, int64_t* lims, float* out_scores, int64_t* out_ids, int64_t capacity, void* workspace,
                           size_t workspace_bytes, void* stream, int64_t row_chunk);
size_t lrx_range_impact_workspace_bytes(int64_t n_rows, int32_t n_queries, int64_t row_chunk);
int lrx_range_impact_search(const void* postings, const int64_t* term_off, int32_t n_terms, int64_t n_rows, const int32_t* q_off,
                            const int32_t* q_term, const int32_t* q_cnt, int32_t n_queries, float radius, int64_t id_base, int64_t* lims,
                            float* out_scores, int64_t* out_ids, int64_t capacity, void* workspace, size_t workspace_bytes, int32_t window_rows,
                            void* stream, int64_t row_chunk);

/* (added in ABI 8, additively) fp16 SCALAR-QUANTISED inner-product index (faiss IndexScalarQuantizer(d, QT_fp16, METRIC_INNER_PRODUCT)):
 * the only resident copy of the rows is their codes c = fp16(x) -- round-to-nearest-even per element, saturating at +-65504 (faiss maps
 * an overflow to inf; counted by lrx_device_saturation_count) -- in the TILED layout of the shadow below (lrx_shard_commit_rows with X_shadow
 * writes them, and so does lrx_encode_packed_shard through shadow_out): 2 bytes per element instead of the 6 of a flat shard with shadow.
 * dim % 64 == 0.  Score s(q, r) = (float) sum_i (double) q_i (double) c_{r,i}: fp64 accumulation, one rounding -- the flat index's score
 * with x replaced by the decoded codes; for fp32 rows that are exactly fp16-representable both indexes return bit-identical results.
 * Exact top-k under that score, ties to the lower row, (-FLT_MAX, -1) padding when k > n_rows, independent of the query batch and the
 * chunking: the rules of lrx_flat_ip_search_bounded.  The search is that one's two-pass chain over the codes: the same filter (fp16(q) .
 * c, fp32 accumulation), whose error is bounded by eps16(q) = |q - fp16(q)| R16 + (D + 32) 2^-23 |fp16(q)| R16 with R16 = R + E taken
 * from row_bounds (the pair lrx_shard_commit_rows maintains; there is no |fp16(q)| E term), the exact rescoring from the codes, and --
 * for queries whose candidate list or band overflows, counted by lrx_search_fallback_count -- a gated score-matrix filter over the codes
 * with exact rescoring of the band kth - 2 eps16 (no host synchronisation).  Shards under 16 Ki rows take the score-matrix filter.
 * out_wire / row_map: as for lrx_flat_ip_search_bounded_wire (NULL: none).  flags: LRX_SEARCH_* above.  Queries per chunk:
 * lrx_sq_fp16_ip_chunk_queries (the role of lrx_flat_ip_bounded_chunk_queries); statistics: lrx_flat_ip_bounded_list_counts with
 * has_shadow = 1.  Workspace: lrx_sq_fp16_ip_workspace_bytes (grows with the queries up to one chunk).                              */
size_t lrx_sq_fp16_ip_workspace_bytes(int64_t n_rows, int32_t dim, int32_t n_queries, int32_t k, int32_t flags);
int32_t lrx_sq_fp16_ip_chunk_queries(int64_t n_rows, int32_t dim, int32_t n_queries, int32_t k, int32_t flags);
int lrx_sq_fp16_ip_search(const void* codes, int64_t n_rows, int32_t dim, const float* row_bounds, const float* q, int32_t n_queries,
                          int32_t k, int64_t id_base, float* out_scores, int64_t* out_ids, const int64_t* row_map, uint64_t* out_wire,
                          void* workspace, size_t workspace_bytes, int32_t flags, void* stream);
/* Exact decode of rows [row0, row0 + n_rows) of the tiled codes to fp32: out[i * ldo + c] = (float) code of row row0 + i, column c
 * (ldo >= dim).  For reconstruct_n and save; fp16 -> fp32 -> fp16 is exact, so lrx_shard_commit_rows of the decoded rows restores the codes. */
int lrx_sq_fp16_decode_rows(const void* codes, int64_t row0, int64_t n_rows, int32_t dim, float* out, int64_t ldo, void* stream);

/* Shard maintenance (FaissIndex.build / IndexFlatIP.add, retriever/faiss_index.py:45-58, for rows that were not written by
 * lrx_encode_packed_shard): one read of n_rows fp32 rows writes their fp16 shadow (X_shadow may be NULL: bounds only) and raises
 * row_bounds[0] = max |row|, row_bounds[1] = max |row - fp16(row)| (device, two floats, zero-initialised by the caller when the
 * shard is created; integer atomic max, order-independent).  dim % 4 == 0.                                                      */
int lrx_shard_commit_rows(const float* X, int64_t ldx, int64_t n_rows, int32_t dim, void* X_shadow, int64_t shadow_row0,
                          float* row_bounds, void* stream);
/* The shadow layout (dim % 64 == 0): X_shadow = base of an array [ceil(rows / 128)][dim / 64] of 16-KiB tiles (128 rows x 64 columns),
 * each tile fragment-major: [16-row group w = 0..7][k-step ks = 0..1][fq = 0..3][fi = 0..15][8] fp16 holds row 16 w + fi, columns
 * 32 ks + 8 fq .. + 7 of the tile (the MFMA 16x16x32 operand of one wave), i.e. element k of row r sits at
 *   ((r / 128) * (dim / 64) + k / 64) * 8192 + ((((r / 16) % 8) * 2 + (k / 32) % 2) * 64 + ((k / 8) % 4) * 16 + r % 16) * 8 + k % 8
 * -- allocated for whole 128-row blocks; shadow_row0 = index within that array of X's first row (writers); for
 * lrx_flat_ip_search_bounded the shard's row 0 is row 0 of the array.  A wave of the filter pass loads its operand with one
 * coalesced 1-KiB request straight into registers (no LDS staging of the corpus side).  (Round 2 also accepted a row-major bf16
 * shadow; it is gone: the tiled layout was faster at every shape and fp16 gives the narrower band.)                               */

/* (added in ABI 8, additively) PRODUCT-QUANTISED inner-product index (faiss IndexPQ(d, M, nbits = 8, METRIC_INNER_PRODUCT)), DESIGN §5.4.3.
 * ksub = 256 centroids per sub-space, dsub = dim / M (dim % M == 0).  centroids: fp32 C[M][256][dsub], faiss's layout
 * centroids[(m * 256 + j) * dsub + i].  The contract, which fixes (D, I) given the centroids and the codes:
 *   code[m]       = argmin_j sum_i (x[m dsub + i] - C[m][j][i])^2, each term an fp64 subtract and square, summed in order over i with
 *                   separate fp64 adds (no contraction); ties to the lower j.
 *   LUT[q][m][j]  = (float) sum_i (double) q[m dsub + i] * (double) C[m][j][i], in order over i (the products are exact in fp64, so a
 *                   contracted fma rounds the same).
 *   s(q, r)       = ((0.f + LUT[q][0][c0]) + LUT[q][1][c1]) + ... + LUT[q][M-1][c_{M-1}]: fp32 adds in ascending m.
 *   top-k         = the flat index's rules: score descending, ties to the lower row, (-FLT_MAX, -1) padding when k > n_rows, 1 <= k <= 2048.
 * faiss's own arithmetic (its LUT and accumulation order depend on the ISA) is not reproduced and cannot be pinned here.
 * THE CODE LAYOUT: Mp = M rounded up to 16; the codes are an array of 128-row blocks of 128 Mp bytes, each block sub-space-group major
 *   [Mp / 16][128 rows][16 bytes]: code m of row r sits at byte  (r / 128) 128 Mp + (m / 16) 2048 + (r % 128) 16 + m % 16
 * -- a lane of the scan loads the 16 codes of one group of its row with one 16-byte load and a wave's 64 loads are 1 KiB contiguous.  The
 * bytes of sub-spaces m >= M are padding (never read as codes).  Allocated for whole 128-row blocks.
 * lrx_pq_ip_search: LUT (lrx_pq_lut) -> k_pq_scan (the query's table in LDS, per-row lookups, [Q, rows] fp32 score matrix of a row chunk of
 * up to 4 Mi rows + 128-row block maxima) -> the flat index's exact top-k selection; row chunks are merged with lrx_merge_topk's kernel.
 * out_ids: id_base + row, or row_map[row] when row_map != NULL (a shard-local row -> its global row, as lrx_pack_topk).  Queries are walked
 * in chunks of lrx_pq_ip_chunk_queries (score matrices of <= 1 GiB, at most 65535 queries: the scan's grid.y); the workspace
 * (lrx_pq_ip_workspace_bytes) holds one chunk.  flags: 0. */
size_t lrx_pq_ip_workspace_bytes(int64_t n_rows, int32_t dim, int32_t M, int32_t n_queries, int32_t k);
int32_t lrx_pq_ip_chunk_queries(int64_t n_rows, int32_t dim, int32_t M, int32_t n_queries, int32_t k);
int lrx_pq_ip_search(const void* codes, int64_t n_rows, const float* centroids, int32_t dim, int32_t M, const float* q, int32_t n_queries,
                     int32_t k, int64_t id_base, float* out_scores, int64_t* out_ids, const int64_t* row_map, void* workspace,
                     size_t workspace_bytes, int32_t flags, void* stream);
/* Encode n_rows fp32 rows (row stride ldx >= dim) into rows row0 .. of the blocked codes (dim / M <= 64). */
int lrx_pq_encode(const float* x, int64_t n_rows, int64_t ldx, const float* centroids, int32_t dim, int32_t M, void* codes, int64_t row0,
                  void* stream);
/* Rows [row0, row0 + n_rows) decoded to fp32: out[i * ldo + m * dsub + e] = C[m][code_m][e] (ldo >= dim). */
int lrx_pq_decode_rows(const void* codes, int64_t row0, int64_t n_rows, const float* centroids, int32_t dim, int32_t M, float* out,
                       int64_t ldo, void* stream);
/* The lookup tables alone: lut[n_queries][M][256] fp32 (tests). */
int lrx_pq_lut(const float* q, int32_t n_queries, const float* centroids, int32_t dim, int32_t M, float* lut, void* stream);

/* (added in ABI 8, additively) BINARY flat index (faiss IndexBinaryFlat(d)) with the reference's float rerank (retriever/faiss_index.py
 * FaissBinaryIndex), DESIGN §5.4.4.  One bit per dimension: dim / 8 bytes per row.  The contract, which fixes every output:
 *   bits          bit j of a row or a query = 1 iff x[j] > threshold[j] -- strict, NaN gives 0; threshold: one float, or threshold_vec[dim]
 *                 when that is not NULL (np.where(x > threshold, 1, 0)).
 *   bytes         np.packbits order: dimension 8 i + b is bit 7 - b of byte i.  dim % 8 == 0, dim <= 16384.
 *   h(q, r)       = popcount(bits(q) XOR bits(r)), an integer in [0, dim].
 *   Hamming top-k   ascending h, ties to the lower row; D int32, I int64; positions beyond n_rows hold (2^31 - 1, -1).  (This tie rule is this
 *                 library's: faiss's depends on which of its kernels runs.)
 *   rerank        candidates = the Hamming top-min(binary_k, n_rows) under that rule; s(q, r) = (float) sum_j (double) q[j] * (bits(r)[j] ? +1 : -1),
 *                 fp64 accumulation, one rounding; result = the top-k candidates by s descending, ties to the lower row, (-FLT_MAX, -1) padding.
 *   limits        1 <= k <= binary_k <= 2048.  dim = 16384 is served (the widest histogram tile takes 131 088 B of LDS).  Any number of
 *                 queries the workspace holds: the rerank scores them 65535 per launch (grid.y).
 * THE CODE LAYOUT: the product-quantised index's, with M = dim / 8 bytes per row: G = ceil(dim / 128) 16-byte groups per row; the codes are an
 *   array of 128-row blocks of 2048 G bytes, each block group major [G][128 rows][16 bytes]: byte i of row r sits at
 *   (r / 128) 2048 G + (i / 16) 2048 + (r % 128) 16 + i % 16.  Bytes i >= dim / 8 of a row are ZERO (the writers below write them; the scan
 *   reads whole groups).  Allocated for whole 128-row blocks.
 * The search: queries packed -> scan 1 (per-query histogram of h, integer atomics) -> cutoff t_q and need_eq = kk - count(h < t_q) -> scan 2
 *   (rows with h < t_q appended to the query's list, ties h == t_q counted per 1024-row tile) -> prefix sum of the tie counts in row order ->
 *   scan 3 (the need_eq lowest ties, only over tiles that hold one) -> LDS sort of the <= 2048 (h, row) keys, or the rerank and its sort.
 *   h is recomputed by every scan, never stored.  No float atomics, no host synchronisation: deterministic.
 * out_ids: id_base + row, or row_map[row] when row_map != NULL.  Workspace: lrx_binary_workspace_bytes (the same for both searches).
 * flags: 0, or LRX_BINARY_SELECT_ONLY (tools: stop once the candidates are selected; the outputs are not written and may be NULL). */
enum { LRX_BINARY_SELECT_ONLY = 1 };
size_t lrx_binary_workspace_bytes(int64_t n_rows, int32_t dim, int32_t n_queries, int32_t binary_k);
int lrx_binary_hamming_search(const void* codes, int64_t n_rows, int32_t dim, const float* q, int32_t n_queries, float threshold,
                              const float* threshold_vec, int32_t k, int64_t id_base, int32_t* out_dist, int64_t* out_ids, const int64_t* row_map,
                              void* workspace, size_t workspace_bytes, int32_t flags, void* stream);
int lrx_binary_ip_search(const void* codes, int64_t n_rows, int32_t dim, const float* q, int32_t n_queries, float threshold,
                         const float* threshold_vec, int32_t k, int32_t binary_k, int64_t id_base, float* out_scores, int64_t* out_ids,
                         const int64_t* row_map, void* workspace, size_t workspace_bytes, int32_t flags, void* stream);
/* Binarise n_rows fp32 rows (row stride ldx >= dim) into rows row0 .. of the blocked codes. */
int lrx_binary_pack_rows(const float* x, int64_t n_rows, int64_t ldx, int32_t dim, float threshold, const float* threshold_vec, void* codes,
                         int64_t row0, void* stream);
/* Rows that are already packed (uint8, dim / 8 bytes each, row stride ld_bytes) into rows row0 .. of the blocked codes. */
int lrx_binary_store_rows(const void* bytes, int64_t n_rows, int64_t ld_bytes, int32_t dim, void* codes, int64_t row0, void* stream);
/* Rows [row0, row0 + n_rows) as row-major packed bytes: out_bytes[i * ldo + b] (ldo >= dim / 8). */
int lrx_binary_decode_rows(const void* codes, int64_t row0, int64_t n_rows, int32_t dim, void* out_bytes, int64_t ldo, void* stream);

/* (added in ABI 8, additively) 8-BIT SCALAR-QUANTISED inner-product index (faiss IndexScalarQuantizer(d, QT_8bit | QT_8bit_uniform,
 * METRIC_INNER_PRODUCT), range statistic RS_minmax with argument 0), DESIGN §5.4.5.  One byte per element, dim % 64 == 0, dim <= 65536.
 * qtype is faiss's QuantizerType: 0 = QT_8bit (a range per dimension), 2 = QT_8bit_uniform (one range for all).  All arithmetic below is fp32
 * with separate operations (no contraction) and IEEE division.  The contract, which fixes (D, I) given `trained` and the codes:
 *   train         vmin[i] = min_r x[r][i], vdiff[i] = max_r x[r][i] - vmin[i]; uniform: one vmin, vdiff over all elements.  NaN training values
 *                 are ignored (fminf / fmaxf semantics), -0 counts as +0; a range with no value that is not NaN gets vmin = vdiff = 0 (SQ8Index.train:
 *                 lrx_sq8_train_minmax leaves +inf / -inf there); the result does not depend on the order of the rows.
 *                 trained = vmin ++ vdiff: 2 dim floats (QT_8bit), 2 floats (QT_8bit_uniform).
 *   encode        t = vdiff[i] != 0 ? (x[i] - vmin[i]) / vdiff[i] : 0;  t < 0 -> 0, t > 1 -> 1, NaN -> 0;  code[i] = (uint8)(int)(255.f * t)
 *                 (truncation; rows outside the trained range clamp, as in faiss).
 *   decode        y[i] = vmin[i] + (((float)code[i] + 0.5f) / 255.f) * vdiff[i].
 *   s(q, r)       = (float) sum_i (double) q[i] * (double) y_r[i]: fp64 accumulation, one rounding.
 *   top-k         the flat index's rules: exact under s, score descending, ties to the lower row, (-FLT_MAX, -1) padding when k > n_rows,
 *                 1 <= k <= 2048.
 * faiss's own accumulation (fp32 SIMD, order depends on the ISA) is not reproduced.
 * THE CODE LAYOUT: an array of 128-row blocks of 128 dim bytes; a block is [dim / 64 column slices][8 groups of 16 rows] tiles of 1 KiB, each tile
 *   [4 pieces of 16 columns][16 rows][16 bytes] -- the i8 MFMA operand of one wave, lane 16 piece + row holding 16 consecutive codes of its
 *   row: one coalesced 16-byte-per-lane request.  Code i of row r sits at byte
 *     (r / 128) 128 dim + (i / 64) 8192 + ((r / 16) % 8) 1024 + ((i / 16) % 4) 256 + (r % 16) 16 + i % 16.
 *   Allocated for whole 128-row blocks (the scan reads whole blocks; what lies beyond n_rows is never reported).
 * lrx_sq8_ip_search, per chunk of lrx_sq8_ip_chunk_queries (<= 128) queries and row chunk of up to 4 Mi rows: query preparation (w = q vdiff / 255
 *   as two int8 digit planes, the bias, a rigorous per-query bound eps(q) on |filter score - s|, for finite inputs
 *   whose scores are normal fp32 numbers or zero) -> one scan of the codes on the i8 MFMA (exact i32
 *   sums; [Q, rows] fp32 filter scores + 128-row block maxima) -> per query: top-k of the filter scores, every row within 2 eps(q) of the k-th
 *   rescored from the codes with the contract's arithmetic, best k.  A band of more than 4096 rows is walked in windows (slow, exact; counted
 *   by lrx_search_fallback_count).  Row chunks are merged with lrx_merge_topk's kernel.  No decoded copy of the rows exists in memory.  No host
 *   synchronisation.  out_ids: id_base + row, or row_map[row] when row_map != NULL.  Workspace: lrx_sq8_ip_workspace_bytes.  flags: 0.      */
size_t lrx_sq8_ip_workspace_bytes(int64_t n_rows, int32_t dim, int32_t n_queries, int32_t k);
int32_t lrx_sq8_ip_chunk_queries(int64_t n_rows, int32_t dim, int32_t n_queries, int32_t k);
/* (added in ABI 9, additively; host only, for tests of the single stages) Where lrx_sq8_ip_search of the same arguments keeps the state of a query
 * chunk in the caller's workspace.  out = {queries per chunk qc, rows per score matrix rc, its row stride ld, the block maxima's row stride nblk_ld,
 * padded queries of a full chunk (16 x the scan's query tiles of qc), then byte offsets: digit tiles (0), scale (double[qc]), bias (double[qc]),
 * eps (float[qc]), score matrix (float[qc][ld]), block maxima (float[qc][nblk_ld]; one per 128 rows), and the workspace's size
 * (= lrx_sq8_ip_workspace_bytes)}.  Digit tile of (16-query tile t, 64-column slice c, plane p: 0 = hi, 1 = lo), n = 128 hi + lo: 1 KiB at
 * ((t dim / 64 + c) 2 + p) 1024, [16-column piece][query % 16][16 bytes].  A chunk of nq <= qc queries prepares the tiles of its own
 * 16 x (1, 2, 4 or 8 tiles >= nq / 16) queries, the padding queries with zero digits.  Every region is rewritten per query chunk and the matrix
 * per row chunk: after a search they show its last query chunk and last row chunk.  Returns LRX_OK or an argument error. */
#define LRX_SQ8_LAYOUT_INTS 12
int lrx_sq8_ip_workspace_layout(int64_t n_rows, int32_t dim, int32_t n_queries, int32_t k, int64_t out[LRX_SQ8_LAYOUT_INTS]);
int lrx_sq8_ip_search(const void* codes, int64_t n_rows, const float* trained, int32_t dim, int32_t qtype, const float* q, int32_t n_queries,
                      int32_t k, int64_t id_base, float* out_scores, int64_t* out_ids, const int64_t* row_map, void* workspace,
                      size_t workspace_bytes, int32_t flags, void* stream);
/* Column minima and maxima of n_rows fp32 rows (row stride ldx >= dim) folded into minmax[2][dim] (device; the caller initialises row 0 to +inf
 * and row 1 to -inf): callable repeatedly, so training walks a large input in pieces.  Integer atomics only. */
int lrx_sq8_train_minmax(const float* x, int64_t n_rows, int64_t ldx, int32_t dim, float* minmax, void* stream);
/* Encode n_rows fp32 rows (row stride ldx >= dim) into rows row0 .. of the tiled codes. */
int lrx_sq8_encode(const float* x, int64_t n_rows, int64_t ldx, const float* trained, int32_t dim, int32_t qtype, void* codes, int64_t row0,
                   void* stream);
/* Rows [row0, row0 + n_rows) decoded to fp32: out[i * ldo + j] (ldo >= dim). */
int lrx_sq8_decode_rows(const void* codes, int64_t row0, int64_t n_rows, const float* trained, int32_t dim, int32_t qtype, float* out,
                        int64_t ldo, void* stream);

/* (added in ABI 8, additively) IMPACT index: the sparse half of the hybrid retriever -- what Lucene serves for `-impact -pretokenized` over a
 * JsonVectorCollection, an integer dot product -- DESIGN §5.4.6.  The contract, which fixes (D, I) given the documents and the queries:
 *   documents     a document is a set of (term, weight) pairs, 1 <= weight < 2^31, a term at most once; its row is its insertion number.
 *   queries       a query is a set of (term, count) pairs, count >= 1; terms the index has never seen contribute nothing.
 *   terms         int32 ids here; the strings (token ids as strings, tokens, the empty-vector marker "-1", an ordinary term) and their
 *                 str -> int32 dictionary in first-seen order are the caller's (ImpactSearch).
 *   S(q, r)       = sum_t count_q[t] * weight_r[t], an exact integer.
 *   hits          row r is a hit iff S(q, r) >= 1, i.e. iff it shares a term with the query; a row that is no hit is never returned.
 *   score         (float) S: ONE round-to-nearest-even conversion -- exact below 2^24; from 2^24 on distinct integers may give one float.
 *   ranking       by the RETURNED float, descending, ties to the lower row (the flat index's rule, Lucene's docid rule); a list of fewer than k
 *                 hits is padded like the flat index pads past n_rows: score -FLT_MAX, id -1.  1 <= k <= 2048; k > n_rows is legal.
 *   overflow      the device accumulates in int32.  The CALLER refuses, before anything is launched, every query with
 *                 B_q = sum_t count_q[t] * maxw[t] >= 2^31 (maxw[t]: the largest weight of term t over all documents, int64 arithmetic):
 *                 S <= B_q, so no accumulator wraps.  ImpactIndex.search raises ValueError; this entry point cannot check it (it does not see
 *                 maxw) and its results are unspecified for such a query.
 * STORAGE, inverted: `postings` = nnz pairs {int32 row, int32 weight} (8 bytes, interleaved: the scan fetches a posting -- or two, 16 bytes --
 *   with one load from the cache lines its range search has just touched), grouped by term, ascending row inside a term;
 *   term_off int64 [n_terms + 1] (device): term t's postings are [term_off[t], term_off[t + 1]).  n_rows < 2^31.
 * QUERIES, CSR on the device: q_off int32 [n_queries + 1] ascending from 0, q_term / q_cnt int32 [q_off[n_queries]]; a term outside
 *   [0, n_terms) has no postings.
 * lrx_impact_search, per chunk of lrx_impact_chunk_queries queries and row chunk of up to 4 Mi rows: one workgroup per (query, window of W
 *   consecutive rows) walks the query's terms, finds the window's piece of each posting list by a lower-bound search on the rows and adds
 *   count * weight into int32 accumulators in LDS (integer adds: deterministic whatever the order), then writes its slice of the [Q, rows] fp32
 *   scores -- zeros included, nothing is cleared beforehand -- and their 128-row block maxima -> the flat index's selection (k_topk_select) ->
 *   results that are not hits become padding -> row chunks merged with lrx_merge_topk's kernel.  No host synchronisation.
 *   window_rows: 0 = the library's rule (32768, 8192 or 2048 rows: the largest that gives every CU two workgroups), else a multiple of 128 up
 *   to 32768 (tests, tools); the results do not depend on it.  out_ids: id_base + row, or row_map[row] when row_map != NULL.
 *   Workspace: lrx_impact_workspace_bytes.                                                                                                */
size_t lrx_impact_workspace_bytes(int64_t n_rows, int32_t n_queries, int32_t k);
int32_t lrx_impact_chunk_queries(int64_t n_rows, int32_t n_queries, int32_t k);
int lrx_impact_search(const void* postings, const int64_t* term_off, int32_t n_terms, int64_t n_rows, const int32_t* q_off,
                      const int32_t* q_term, const int32_t* q_cnt, int32_t n_queries, int32_t k, int64_t id_base, float* out_scores,
                      int64_t* out_ids, const int64_t* row_map, void* workspace, size_t workspace_bytes, int32_t window_rows, void* stream);

/* (added in ABI 8, additively) Exact fp32 linear map, the hot path of a PCA pre-transform (PCAMatrix / PreTransformIndex):
 *   out[r * ldo + o] = b[o] + sum_k A[o * d_in + k] * x[r * ldx + k]      r < n_rows, o < d_out; A row-major [d_out, d_in]; b may be NULL (+0).
 * fp32 operands on the f32-input MFMA.  Every output has ONE accumulator chain: it starts at b[o] and takes the products in ascending k, one
 * rounding per product.  No split-K, no atomics: a row's result depends on that row, A and b alone -- not on n_rows, on the row's position in
 * the call or on the tile it lands in.  Columns [d_out, ldo) of `out` are left untouched.
 * d_in % 8 == 0, 8 <= d_in <= 8192; any d_out >= 1 and n_rows >= 0 (0 rows: nothing is launched); ldx >= d_in, ldo >= d_out; anything else is
 * LRX_ERR_INVALID before any device work.  x and A are read 16 bytes at a time where their addresses allow it, 4 otherwise.  `out` must not
 * overlap x or A. */
int lrx_linear_transform(const float* x, int64_t n_rows, int64_t ldx, const float* A, const float* b, int32_t d_in, int32_t d_out, float* out,
                         int64_t ldo, void* stream);

/* (added in ABI 8, additively) RERANK: the exact scores of a CALLER's candidate rows and their top k -- the second stage of faiss
 * IndexRefineFlat / IndexRefine over a full-precision copy of the rows (RefineFlatIndex).
 *   candidates  cand_rows[i * ld_cand + j], j < n_cand: ROW numbers of query i's candidates (what a base search with id_base = 0 returns).
 *               An entry < 0 (the base's -1 padding) is skipped.  An entry >= n_rows is NEVER dereferenced: it is skipped and counted once in
 *               lrx_device_error_count.  A row that occurs twice is scored and reported twice, as faiss does.
 *   score       lrx_flat_ip_rerank: the flat index's score over the fp32 rows X[row * ldx + c], (float) of the fp64 sum of the fp32 products;
 *               lrx_sq_fp16_ip_rerank: the same over the tiled fp16 codes (lrx_sq_fp16_ip_search's layout and score).  Bit for bit what
 *               lrx_flat_ip_search_bounded / lrx_sq_fp16_ip_search report for that (query, row): the same device function computes it.
 *   order       score descending, ties to the lower row; (-FLT_MAX, -1) where fewer than k valid candidates exist.  out_ids = id_base + row,
 *               or row_map[row] when row_map != NULL (int64 [>= n_rows], device).  out_scores / out_ids: [n_queries, k], contiguous.
 *   a query's result depends on its own row of q and of cand_rows alone: not on n_queries, its position in the call or the split below.
 *   limits      1 <= k <= n_cand <= 2048; ld_cand >= n_cand; 0 <= n_rows < 2^32; q 16-byte aligned ([n_queries, dim] contiguous);
 *               fp32 rows: dim % 4 == 0, ldx >= dim, ldx % 4 == 0, X 16-byte aligned; codes: dim % 64 == 0.  n_queries == 0 launches nothing.
 *               Anything else is LRX_ERR_INVALID before any device work; a workspace under lrx_ip_rerank_workspace_bytes: LRX_ERR_WORKSPACE.
 * Two launches on `stream`, no host synchronisation, capturable in a HIP graph: grid (query, part) -- a part takes every part-count-th
 * candidate, one half-wave per row (a random gather of whole rows, non-temporal loads), and publishes packed (score, row) words -- then one
 * workgroup per query sorts at most 2048 words in LDS and writes the top k. */
size_t lrx_ip_rerank_workspace_bytes(int32_t n_queries, int32_t n_cand, int32_t k);
int lrx_flat_ip_rerank(const float* X, int64_t n_rows, int64_t ldx, int32_t dim, const float* q, int32_t n_queries, const int64_t* cand_rows,
                       int32_t n_cand, int64_t ld_cand, int32_t k, int64_t id_base, float* out_scores, int64_t* out_ids, const int64_t* row_map,
                       void* workspace, size_t workspace_bytes, void* stream);
int lrx_sq_fp16_ip_rerank(const void* codes, int64_t n_rows, int32_t dim, const float* q, int32_t n_queries, const int64_t* cand_rows,
                          int32_t n_cand, int64_t ld_cand, int32_t k, int64_t id_base, float* out_scores, int64_t* out_ids, const int64_t* row_map,
                          void* workspace, size_t workspace_bytes, void* stream);

/* (added in ABI 8, additively) INVERTED FILE: the exact top k over the rows of the cells a query probes -- the scan of faiss IndexIVFFlat
 * with METRIC_INNER_PRODUCT (IVFFlatIndex).  The caller owns the coarse quantiser: it passes the probe lists.
 *   rows        X[pos * ldx + c], fp32, stored CELL BY CELL: cell c holds positions [list_off[c], list_off[c + 1]) (int64 [nlist + 1], device,
 *               ascending, list_off[nlist] <= n_rows).  row_ids[pos] (int64 [n_rows], device) is the ORIGINAL row of a position; NULL: the
 *               position itself.  A position whose original row is outside [0, n_rows) is dropped and counted in lrx_device_error_count.
 *   probes      probes[i * ld_probe + j], j < nprobe: the cells of query i (what a coarse search with id_base = 0 returns).  An entry < 0 (the
 *               coarse search's padding) is skipped.  An entry >= nlist is NEVER dereferenced: it is skipped and counted once in
 *               lrx_device_error_count.  A cell named twice by one query is scanned once for it.
 *   max_scan_rows   the caller's bound on the rows any one query scans (IVFFlatIndex: the sum of its nprobe largest cells); it sizes the
 *               workspace.  A query whose cells hold more writes nothing, is counted once in lrx_device_error_count and returns padding.
 *   score       the flat index's: (float) of the fp64 sum of the fp32 products, by the device function of lrx_flat_ip_rerank's family
 *               (exact_dot_lds_row): bit for bit what lrx_flat_ip_search_bounded / lrx_flat_ip_rerank report for that (query, row).  No filter
 *               pass, no error band: every scanned row is scored exactly, once per query that probes its cell.
 *   order       score descending, ties to the lower ORIGINAL row; (-FLT_MAX, -1) where the probed cells hold fewer than k rows.  out_ids =
 *               id_base + row, or row_map[row] when row_map != NULL (int64 [>= n_rows], device).  out_scores / out_ids: [n_queries, k].
 *   a query's result depends on its own rows of q and probes alone: not on n_queries, its position in the call or the chunking below.
 *   limits      dim % 32 == 0, 32 <= dim <= 8192; 1 <= nlist; 1 <= nprobe <= min(nlist, 2048); ld_probe >= nprobe; 1 <= k <= 2048;
 *               0 <= n_rows < 2^32; 0 <= max_scan_rows < 2^31; ldx >= dim, ldx % 4 == 0, X and q 16-byte aligned ([n_queries, dim] contiguous).
 *               n_queries == 0 launches nothing.  Anything else is LRX_ERR_INVALID before any device work; a workspace under
 *               lrx_ivf_flat_ip_workspace_bytes: LRX_ERR_WORKSPACE.
 * Per chunk of queries (min(n_queries, 1024, 768 MiB / (8 max_scan_rows)): the workspace stays under 1 GiB and stops growing there) six
 * launches on `stream` (kernels only: no memset or copy node), no host synchronisation, capturable in a HIP graph: the counters' clear, the
 * probe plan (one workgroup per query), a counting sort of the (query, cell) pairs by cell that also lays out the work items (a probed cell =
 * groups of up to 64 KiB of consecutive stored rows), the CELL-MAJOR persistent scan -- a workgroup stages a group in LDS once and scores it
 * against every query that probes its cell, query rows streamed from L2; cells nobody probes cost nothing -- and one workgroup per query that
 * selects and sorts the top k of the query's packed (score, row) words. */
size_t lrx_ivf_flat_ip_workspace_bytes(int64_t n_rows, int32_t nlist, int32_t dim, int32_t n_queries, int32_t nprobe, int32_t k, int64_t max_scan_rows);
int lrx_ivf_flat_ip_search(const float* X, int64_t n_rows, int64_t ldx, int32_t dim, const int64_t* list_off, const int64_t* row_ids, int32_t nlist,
                           const float* q, int32_t n_queries, const int64_t* probes, int32_t nprobe, int64_t ld_probe, int64_t max_scan_rows,
                           int32_t k, int64_t id_base, float* out_scores, int64_t* out_ids, const int64_t* row_map,
                           void* workspace, size_t workspace_bytes, void* stream);

/* (added in ABI 9, additively) RANGE SEARCH over the probed cells -- faiss IndexIVF::range_search_preassigned with METRIC_INNER_PRODUCT, for
 * the four inverted-file entries.  Each lrx_ivf_*_ip_range_search takes the argument list of its top-k sibling with `k`
 * replaced by `float radius` and (out_scores, out_ids) by (lims, out_scores, out_ids, capacity); each *_range_workspace_bytes takes its
 * sibling's arguments without k.  It is the sibling's chain up to and including the scan -- the same host driver, the same kernels, the same
 * packed (score, row) words -- followed by a count, a prefix sum and an ordered fill instead of the selection.
 *   hit         a row the top-k search of the same arguments would have scanned whose score is STRICTLY greater than radius.  Scanned: the row
 *               lies in a cell the query's probe row names -- an entry < 0 is skipped; an entry >= nlist is skipped and counted once in
 *               lrx_device_error_count; a cell named twice is scanned once; a query whose cells hold more than max_scan_rows scans nothing, has
 *               no hits and is counted once.  Score: the fp32 value the sibling search reports for that (query, row), bit for bit.  The
 *               comparison is the float comparison score > radius: -0.0 and +0.0 are equal, a score equal to the radius is not a hit,
 *               radius = +inf gives no hits, radius = -inf every scanned row.  A NaN radius is LRX_ERR_INVALID before any device work.  A stored
 *               position whose original row is outside [0, n_rows) (dropped and counted by the scan) is never a hit.
 *   order       SEGMENT order, faiss's order for an IVF range search: the query's cells in the order of its probe row (after the skips above),
 *               inside a cell the rows by stored position -- ascending original row when the rows were added in order.  It depends on the
 *               query's own rows of q, probes and probe_scores alone, never on the batch.  It is NOT the ascending-row order of
 *               lrx_flat_ip_range_search, and hits are not sorted by score.
 *   layout      lrx_flat_ip_range_search's protocol: lims int64 [n_queries + 1] on the device, lims[0] = 0, hits of query i at
 *               [lims[i], lims[i + 1]) of out_scores / out_ids; out_ids = id_base + row, or row_map[row] when row_map != NULL.  lims is ALWAYS
 *               written and exact.  out_scores / out_ids are written only where they fit `capacity` entries, decided on the device per chunk
 *               of queries (a chunk whose lims end exceeds capacity writes nothing); the call returns LRX_OK either way: read lims[n_queries]
 *               and call again with at least that capacity.  capacity == 0 allows NULL out_scores / out_ids.  n_queries == 0 writes lims[0].
 *   limits      the sibling's argument checks, unchanged, without k; capacity >= 0; lims != NULL.  Workspace: the sibling's plus one uint32
 *               hit count per query of a chunk (lrx_ivf_*_ip_range_workspace_bytes >= the sibling's for any k); less is LRX_ERR_WORKSPACE.
 * Per chunk of queries (the sibling's chunk; lims carried across chunks on the device) the sibling's launches up to the scan, then three: the
 * count (one 1024-thread workgroup per query over its segment of words), the chunk's lims, and the fill -- the same walk with a stable
 * compaction (wave ballot and popcount, wave totals through LDS, a running base per workgroup), no atomics on the output.  No host
 * synchronisation, every size from the arguments alone, one stream. */
size_t lrx_ivf_flat_ip_range_workspace_bytes(int64_t n_rows, int32_t nlist, int32_t dim, int32_t n_queries, int32_t nprobe, int64_t max_scan_rows);
int lrx_ivf_flat_ip_range_search(const float* X, int64_t n_rows, int64_t ldx, int32_t dim, const int64_t* list_off, const int64_t* row_ids,
                                 int32_t nlist, const float* q, int32_t n_queries, const int64_t* probes, int32_t nprobe, int64_t ld_probe,
                                 int64_t max_scan_rows, float radius, int64_t id_base, int64_t* lims, float* out_scores, int64_t* out_ids,
                                 int64_t capacity, const int64_t* row_map, void* workspace, size_t workspace_bytes, void* stream);
size_t lrx_ivf_pq_ip_range_workspace_bytes(int64_t n_rows, int32_t nlist, int32_t dim, int32_t M, int32_t n_queries, int32_t nprobe,
                                           int64_t max_scan_rows);
int lrx_ivf_pq_ip_range_search(const void* codes, int64_t n_rows, const float* pq_centroids, int32_t dim, int32_t M, const int64_t* list_off,
                               const int64_t* row_ids, int32_t nlist, const float* q, int32_t n_queries, const int64_t* probes,
                               const float* probe_scores, int32_t nprobe, int64_t ld_probe, int32_t by_residual, int64_t max_scan_rows, float radius,
                               int64_t id_base, int64_t* lims, float* out_scores, int64_t* out_ids, int64_t capacity, const int64_t* row_map,
                               void* workspace, size_t workspace_bytes, void* stream);
size_t lrx_ivf_sq_fp16_ip_range_workspace_bytes(int64_t n_rows, int32_t nlist, int32_t dim, int32_t n_queries, int32_t nprobe, int64_t max_scan_rows);
int lrx_ivf_sq_fp16_ip_range_search(const void* codes, int64_t n_rows, int32_t dim, const int64_t* list_off, const int64_t* row_ids, int32_t nlist,
                                    const float* q, int32_t n_queries, const int64_t* probes, const float* probe_scores, int32_t nprobe,
                                    int64_t ld_probe, int32_t by_residual, int64_t max_scan_rows, float radius, int64_t id_base, int64_t* lims,
                                    float* out_scores, int64_t* out_ids, int64_t capacity, const int64_t* row_map, void* workspace,
                                    size_t workspace_bytes, void* stream);
size_t lrx_ivf_sq8_ip_range_workspace_bytes(int64_t n_rows, int32_t nlist, int32_t dim, int32_t n_queries, int32_t nprobe, int64_t max_scan_rows);
int lrx_ivf_sq8_ip_range_search(const void* codes, int64_t n_rows, int32_t dim, const float* trained, int32_t qtype, const int64_t* list_off,
                                const int64_t* row_ids, int32_t nlist, const float* q, int32_t n_queries, const int64_t* probes,
                                const float* probe_scores, int32_t nprobe, int64_t ld_probe, int32_t by_residual, int64_t max_scan_rows, float radius,
                                int64_t id_base, int64_t* lims, float* out_scores, int64_t* out_ids, int64_t capacity, const int64_t* row_map,
                                void* workspace, size_t workspace_bytes, void* stream);

/* (added under ABI 9, additively) ROW SELECTOR for the four inverted-file entries -- faiss SearchParameters(sel = IDSelectorBatch /
 * IDSelectorBitmap / IDSelectorRange / IDSelectorNot) (RowSelector): search a subset of the rows.
 *   selector    a bitmap over the ORIGINAL rows 0 .. n_bits - 1 of an index: the number a search reports before id_base / row_map -- not a
 *               stored position, not a mapped id.  Bit r is (bits[r >> 5] >> (r & 31)) & 1; bits: uint32 [ceil(n_bits / 32)] on the device.
 *               The bits at or beyond n_bits in the last word are written as 0 by every lrx_selector_* entry; no search reads them.
 *               0 <= n_bits < 2^32; n_bits == 0 launches nothing.  One kernel each on `stream`, capturable.
 *   lrx_selector_fill        every bit below n_bits = (value != 0).
 *   lrx_selector_from_mask   bit r = (mask[r] != 0), mask: n_bits bytes on the device; one thread packs the 32 bytes of a word (plain store).
 *   lrx_selector_set_rows    bit rows[i] is SET for i < n (int64, device; duplicates are fine; bits already set stay: fill first for a fresh
 *               selector).  A row outside [0, n_bits) is never turned into an address: it is skipped and counted in lrx_device_error_count.
 *   lrx_selector_invert      out = NOT in below n_bits, 0 at and beyond it; in == out is allowed.
 * Each lrx_ivf_*_ip_search_sel / lrx_ivf_*_ip_range_search_sel takes the argument list of its plain sibling with
 * (const uint32_t* sel_bits, int64_t sel_rows) inserted before `workspace`, and the sibling's *_workspace_bytes.
 *   sel_bits == NULL   the plain entry: the same kernels, the same bits (sel_rows is ignored).
 *   sel_bits != NULL   sel_rows must equal n_rows (LRX_ERR_INVALID otherwise, with the other argument checks and before the workspace
 *               check).  The result is the sibling's over the SELECTED rows of the probed cells: top k -- score descending, ties to the lower
 *               original row, (-FLT_MAX, -1) where fewer than k selected rows were scanned; range -- every selected row with a score >
 *               radius, in segment order.  Every scanned (query, row) pair is scored independently of the others, so a filtered result is the
 *               unfiltered full result restricted to the selected rows, bit for bit.  One selector per call, shared by its queries.
 *   unchanged   the probe-list rules (entries < 0, >= nlist, repeats), probe_scores / by_residual, the segment layout and max_scan_rows, which
 *               go by the UNFILTERED cell sizes: a query whose cells hold more than max_scan_rows is padding and counted whatever the
 *               selector says.  id_base / row_map apply after the filter.  A stored position whose original row is outside [0, n_rows) has no
 *               bit: it is dropped and counted as without a selector.
 * The chain is the sibling's with the scan kernel's selector instantiation: a deselected (query, row) pair becomes the null word 0 -- the word
 * the selection and the range kernels already drop -- before its score is computed; the cell-major scans test a staged group's rows once per
 * work item and do not read a group with no selected row from memory at all. */
int lrx_selector_fill(uint32_t* bits, int64_t n_bits, int32_t value, void* stream);
int lrx_selector_from_mask(const uint8_t* mask, int64_t n_bits, uint32_t* bits, void* stream);
int lrx_selector_set_rows(const int64_t* rows, int64_t n, int64_t n_bits, uint32_t* bits, void* stream);
int lrx_selector_invert(const uint32_t* in, uint32_t* out, int64_t n_bits, void* stream);
int lrx_ivf_flat_ip_search_sel(const float* X, int64_t n_rows, int64_t ldx, int32_t dim, const int64_t* list_off, const int64_t* row_ids, int32_t nlist,
                               const float* q, int32_t n_queries, const int64_t* probes, int32_t nprobe, int64_t ld_probe, int64_t max_scan_rows,
                               int32_t k, int64_t id_base, float* out_scores, int64_t* out_ids, const int64_t* row_map, const uint32_t* sel_bits,
                               int64_t sel_rows, void* workspace, size_t workspace_bytes, void* stream);
int lrx_ivf_flat_ip_range_search_sel(const float* X, int64_t n_rows, int64_t ldx, int32_t dim, const int64_t* list_off, const int64_t* row_ids,
                                     int32_t nlist, const float* q, int32_t n_queries, const int64_t* probes, int32_t nprobe, int64_t ld_probe,
                                     int64_t max_scan_rows, float radius, int64_t id_base, int64_t* lims, float* out_scores, int64_t* out_ids,
                                     int64_t capacity, const int64_t* row_map, const uint32_t* sel_bits, int64_t sel_rows, void* workspace,
                                     size_t workspace_bytes, void* stream);
int lrx_ivf_pq_ip_search_sel(const void* codes, int64_t n_rows, const float* pq_centroids, int32_t dim, int32_t M, const int64_t* list_off,
                             const int64_t* row_ids, int32_t nlist, const float* q, int32_t n_queries, const int64_t* probes,
                             const float* probe_scores, int32_t nprobe, int64_t ld_probe, int32_t by_residual, int64_t max_scan_rows, int32_t k,
                             int64_t id_base, float* out_scores, int64_t* out_ids, const int64_t* row_map, const uint32_t* sel_bits, int64_t sel_rows,
                             void* workspace, size_t workspace_bytes, void* stream);
int lrx_ivf_pq_ip_range_search_sel(const void* codes, int64_t n_rows, const float* pq_centroids, int32_t dim, int32_t M, const int64_t* list_off,
                                   const int64_t* row_ids, int32_t nlist, const float* q, int32_t n_queries, const int64_t* probes,
                                   const float* probe_scores, int32_t nprobe, int64_t ld_probe, int32_t by_residual, int64_t max_scan_rows,
                                   float radius, int64_t id_base, int64_t* lims, float* out_scores, int64_t* out_ids, int64_t capacity,
                                   const int64_t* row_map, const uint32_t* sel_bits, int64_t sel_rows, void* workspace, size_t workspace_bytes,
                                   void* stream);
int lrx_ivf_sq_fp16_ip_search_sel(const void* codes, int64_t n_rows, int32_t dim, const int64_t* list_off, const int64_t* row_ids, int32_t nlist,
                                  const float* q, int32_t n_queries, const int64_t* probes, const float* probe_scores, int32_t nprobe,
                                  int64_t ld_probe, int32_t by_residual, int64_t max_scan_rows, int32_t k, int64_t id_base, float* out_scores,
                                  int64_t* out_ids, const int64_t* row_map, const uint32_t* sel_bits, int64_t sel_rows, void* workspace,
                                  size_t workspace_bytes, void* stream);
int lrx_ivf_sq_fp16_ip_range_search_sel(const void* codes, int64_t n_rows, int32_t dim, const int64_t* list_off, const int64_t* row_ids, int32_t nlist,
                                        const float* q, int32_t n_queries, const int64_t* probes, const float* probe_scores, int32_t nprobe,
                                        int64_t ld_probe, int32_t by_residual, int64_t max_scan_rows, float radius, int64_t id_base, int64_t* lims,
                                        float* out_scores, int64_t* out_ids, int64_t capacity, const int64_t* row_map, const uint32_t* sel_bits,
                                        int64_t sel_rows, void* workspace, size_t workspace_bytes, void* stream);
int lrx_ivf_sq8_ip_search_sel(const void* codes, int64_t n_rows, int32_t dim, const float* trained, int32_t qtype, const int64_t* list_off,
                              const int64_t* row_ids, int32_t nlist, const float* q, int32_t n_queries, const int64_t* probes,
                              const float* probe_scores, int32_t nprobe, int64_t ld_probe, int32_t by_residual, int64_t max_scan_rows, int32_t k,
                              int64_t id_base, float* out_scores, int64_t* out_ids, const int64_t* row_map, const uint32_t* sel_bits, int64_t sel_rows,
                              void* workspace, size_t workspace_bytes, void* stream);
int lrx_ivf_sq8_ip_range_search_sel(const void* codes, int64_t n_rows, int32_t dim, const float* trained, int32_t qtype, const int64_t* list_off,
                                    const int64_t* row_ids, int32_t nlist, const float* q, int32_t n_queries, const int64_t* probes,
                                    const float* probe_scores, int32_t nprobe, int64_t ld_probe, int32_t by_residual, int64_t max_scan_rows,
                                    float radius, int64_t id_base, int64_t* lims, float* out_scores, int64_t* out_ids, int64_t capacity,
                                    const int64_t* row_map, const uint32_t* sel_bits, int64_t sel_rows, void* workspace, size_t workspace_bytes,
                                    void* stream);

/* (added in ABI 8, additively) INVERTED FILE over PRODUCT-QUANTISED codes: the top k under the ADC score over the rows of the cells a query
 * probes -- the scan of faiss IndexIVFPQ(quantizer, d, nlist, M, 8, METRIC_INNER_PRODUCT) (IVFPQIndex).  The caller owns the
 * coarse quantiser: it passes the probe lists and, with by_residual, the coarse scores of the probed cells.
 *   codes       the blocked PQ layout of lrx_pq_ip_search (128-row blocks, 16-sub-space groups, Mp = ceil(M / 16) * 16 bytes per row, whole
 *               blocks for n_rows rows), indexed by STORED POSITION, CELL BY CELL: cell c holds positions [list_off[c], list_off[c + 1]) (int64
 *               [nlist + 1], device, ascending, list_off[nlist] <= n_rows) -- a cell usually starts in the middle of a block.  row_ids[pos]
 *               (int64 [n_rows], device) is the ORIGINAL row of a position; NULL: the position itself.  A position whose original row is
 *               outside [0, n_rows) is dropped and counted in lrx_device_error_count.  lrx_pq_encode and lrx_pq_decode_rows work on this
 *               buffer unchanged, with row0 = the position.  pq_centroids: [M, 256, dim / M] fp32.
 *   probes      probes[i * ld_probe + j], j < nprobe: the cells of query i (what a coarse search with id_base = 0 returns).  An entry < 0 is
 *               skipped.  An entry >= nlist is NEVER dereferenced: it is skipped and counted once in lrx_device_error_count.  A cell named
 *               twice by one query is scanned once for it, with the base term of its FIRST occurrence.
 *   score       of (query i, position p in the probed cell probes[i][j]), fp32:
 *                   acc = by_residual ? probe_scores[i * ld_probe + j] : 0.f;   acc += LUT[i][m][code_m(p)]  for m = 0 .. M - 1, in order,
 *               one fp32 add each; LUT[i][m][c] = (float) of the fp64 sum in order of q_i's sub-vector m times centroid c of sub-space m
 *               (lrx_pq_lut).  For the inner product the residual table does not depend on the cell: <q, c + r> = <q, c> + sum_m <q_m,
 *               cb_m[code_m]>, so there is ONE table per query and the caller passes the cell term (IVFPQIndex: the coarse search's own exact
 *               scores).  probe_scores (fp32, the layout of probes) may be NULL when by_residual == 0; then a (query, row) score is bit for
 *               bit lrx_pq_ip_search's.
 *   max_scan_rows   the caller's bound on the rows any one query scans (IVFPQIndex: the sum of its nprobe largest cells); it sizes the
 *               workspace.  A query whose cells hold more writes nothing, is counted once in lrx_device_error_count and returns padding.
 *   order       score descending, ties to the lower ORIGINAL row; (-FLT_MAX, -1) where the probed cells hold fewer than k rows.  out_ids =
 *               id_base + row, or row_map[row] when row_map != NULL (int64 [>= n_rows], device).  out_scores / out_ids: [n_queries, k].
 *   a query's result depends on its own rows of q, probes and probe_scores alone: not on n_queries, its position in the call or the chunking.
 *   limits      dim % M == 0; 1 <= nlist; 1 <= nprobe <= min(nlist, 2048); ld_probe >= nprobe; 1 <= k <= 2048; 0 <= n_rows < 2^32;
 *               0 <= max_scan_rows < 2^31; q [n_queries, dim] contiguous.  n_queries == 0 launches nothing.  Anything else is LRX_ERR_INVALID
 *               with a message before any device work; a workspace under lrx_ivf_pq_ip_workspace_bytes: LRX_ERR_WORKSPACE.
 * Per chunk of queries (lrx_ivf_flat_ip_search's chunk) four launches on `stream` (kernels only: no memset or copy node, nothing to clear), no
 * host synchronisation, capturable in a HIP graph: the chunk's lookup tables into the head of the workspace, the probe plan (one workgroup per
 * query: a dense, ascending offset per probe slot), the QUERY-MAJOR scan -- grid (tiles, queries): a workgroup keeps its query's table in LDS
 * (in passes above 128 sub-spaces) and walks 1024-position tiles of the query's segment, the concatenation of its probed cells in probe order;
 * a lane finds its slot by a binary search over the slot offsets in LDS and reads its codes as 16-byte pieces -- and the selection of
 * lrx_ivf_flat_ip_search over the packed (score, row) words.  The workspace size never decreases in n_queries or max_scan_rows. */
size_t lrx_ivf_pq_ip_workspace_bytes(int64_t n_rows, int32_t nlist, int32_t dim, int32_t M, int32_t n_queries, int32_t nprobe, int32_t k,
                                     int64_t max_scan_rows);
int lrx_ivf_pq_ip_search(const void* codes, int64_t n_rows, const float* pq_centroids, int32_t dim, int32_t M, const int64_t* list_off,
                         const int64_t* row_ids, int32_t nlist, const float* q, int32_t n_queries, const int64_t* probes, const float* probe_scores,
                         int32_t nprobe, int64_t ld_probe, int32_t by_residual, int64_t max_scan_rows, int32_t k, int64_t id_base,
                         float* out_scores, int64_t* out_ids, const int64_t* row_map, void* workspace, size_t workspace_bytes, void* stream);

/* (added in ABI 8, additively) INVERTED FILE over fp16 SCALAR-QUANTISED codes: the exact top k, under the fp16 store's score, over the rows of
 * the cells a query probes -- the scan of faiss IndexIVFScalarQuantizer(quantizer, d, nlist, QT_fp16, METRIC_INNER_PRODUCT) (IVFSQIndex, DESIGN
 * 5.4.12).  The caller owns the coarse quantiser: it passes the probe lists and, with by_residual, the coarse scores of the probed cells.
 *   cells, probes, ids   lrx_ivf_flat_ip_search's, unchanged: list_off, row_ids, probes, ld_probe, max_scan_rows, id_base and row_map keep their
 *               meaning; score descending, ties to the lower ORIGINAL row; (-FLT_MAX, -1) padding; an entry < 0 is skipped; an entry >= nlist is
 *               NEVER dereferenced and is counted once in lrx_device_error_count; a cell named twice by one query is scanned once for it (with
 *               the base term of its FIRST occurrence); a query whose cells hold more than max_scan_rows returns padding and is counted once; a
 *               position whose original row is outside [0, n_rows) is dropped and counted.
 *   codes       fp16, ROW-MAJOR [n_rows, dim] by stored position, CELL BY CELL, 2 dim bytes per row (not the tiled layout of lrx_sq_fp16_ip_search);
 *               the base pointer 16-byte aligned.  A row's code is fp16(v_i) under lrx_shard_commit_rows' rounding rule -- round-to-nearest-even,
 *               saturating at +-65504 where faiss gives inf.  Without by_residual v = x; with it v_i = fl32(x_i - c_i), ONE fp32 subtraction of
 *               the centroid of the row's cell, then the fp16 rounding.  lrx_ivf_sq_fp16_encode_rows writes them.
 *   score       of a scanned (query i, row) pair of the probed cell probes[i][j]:  (float)(B + sum_e (double)q_e * (double)(float)code_e).  The
 *               sum is exact_dot's: lane `sub` of a half-wave takes elements 4 sub + 128 u + 0..3 of each 2048-element block, fp64
 *               accumulation, the xor tree 16, 8, 4, 2, 1; B joins the reduced sum; ONE rounding.  B = 0 without by_residual; with it
 *               B = (double)probe_scores[i * ld_probe + j], the caller's fp32 score of the cell for that query (faiss: coarse_dis).  by_residual
 *               with probe_scores == NULL is LRX_ERR_INVALID.  Without by_residual a pair's score is bit for bit what lrx_sq_fp16_ip_search
 *               and lrx_sq_fp16_ip_rerank report for the same code.  Every scanned row is scored exactly, once per query that probes its cell.
 *   a query's result depends on its own rows of q, probes and probe_scores alone: not on n_queries, its position in the call or the chunking.
 *   limits      dim % 32 == 0, 32 <= dim <= 8192; 1 <= nlist; 1 <= nprobe <= min(nlist, 2048); ld_probe >= nprobe; 1 <= k <= 2048;
 *               0 <= n_rows < 2^32; 0 <= max_scan_rows < 2^31; codes and q 16-byte aligned (q [n_queries, dim] contiguous).  n_queries == 0
 *               launches nothing.  Anything else is LRX_ERR_INVALID with a message before any device work; a workspace under
 *               lrx_ivf_sq_fp16_ip_workspace_bytes (= lrx_ivf_flat_ip_workspace_bytes of the same arguments): LRX_ERR_WORKSPACE.
 * Per chunk of queries (lrx_ivf_flat_ip_search's chunk) that entry's six launches on `stream` (kernels only: no memset or copy node), no host
 * synchronisation, every size from the arguments alone, capturable in a HIP graph: clear, plan, work items, scatter, the CELL-MAJOR persistent
 * scan over groups of lrx_ivf_sq_fp16_group_rows(dim) = min(128, 32768 / dim) consecutive code rows staged in LDS as fp16 (64 KiB: twice the
 * rows of the fp32 scan), and the selection.
 * lrx_ivf_sq_fp16_encode_rows: one kernel -- code rows [row0, row0 + n) from x[i * ldx + e] (fp32; ldx >= dim, ldx % 4 == 0, 16-byte aligned):
 * gather the centroid of cells[i] (int64 [n], device; centroids fp32 [nlist, dim] contiguous, NULL: no residual, and then cells may be NULL),
 * subtract, round, saturate.  A cells[i] outside [0, nlist) is never dereferenced: its codes are written as zeros and it is counted in
 * lrx_device_error_count.  row0 + n < 2^32. */
int32_t lrx_ivf_sq_fp16_group_rows(int32_t dim);
size_t lrx_ivf_sq_fp16_ip_workspace_bytes(int64_t n_rows, int32_t nlist, int32_t dim, int32_t n_queries, int32_t nprobe, int32_t k,
                                          int64_t max_scan_rows);
int lrx_ivf_sq_fp16_ip_search(const void* codes, int64_t n_rows, int32_t dim, const int64_t* list_off, const int64_t* row_ids, int32_t nlist,
                              const float* q, int32_t n_queries, const int64_t* probes, const float* probe_scores, int32_t nprobe, int64_t ld_probe,
                              int32_t by_residual, int64_t max_scan_rows, int32_t k, int64_t id_base, float* out_scores, int64_t* out_ids,
                              const int64_t* row_map, void* workspace, size_t workspace_bytes, void* stream);
int lrx_ivf_sq_fp16_encode_rows(const float* x, int64_t ldx, int64_t n, int32_t dim, const float* centroids, const int64_t* cells, int32_t nlist,
                                void* codes, int64_t row0, void* stream);

/* (added in ABI 9, additively) INVERTED FILE over 8-BIT SCALAR-QUANTISED codes: the exact top k, under the 8-bit store's score, over the rows of
 * the cells a query probes -- the scan of faiss IndexIVFScalarQuantizer(quantizer, d, nlist, QT_8bit | QT_8bit_uniform, METRIC_INNER_PRODUCT)
 * (IVFSQ8Index).  The caller owns the coarse quantiser: it passes the probe lists and, with by_residual, the coarse scores.
 *   cells, probes, ids, limits, errors, capture   lrx_ivf_sq_fp16_ip_search's, unchanged (the same host driver): list_off, row_ids, probes,
 *               ld_probe, max_scan_rows, id_base and row_map keep their meaning; score descending, ties to the lower ORIGINAL row; (-FLT_MAX, -1)
 *               padding; an entry < 0 is skipped; an entry >= nlist is NEVER dereferenced and is counted once in lrx_device_error_count; a cell
 *               named twice by one query is scanned once for it (with the base term of its FIRST occurrence); a query whose cells hold more
 *               than max_scan_rows returns padding and is counted once; a position whose original row is outside [0, n_rows) is dropped and
 *               counted.  dim % 32 == 0, 32 <= dim <= 8192; by_residual with probe_scores == NULL is LRX_ERR_INVALID; a workspace under
 *               lrx_ivf_sq8_ip_workspace_bytes (= lrx_ivf_flat_ip_workspace_bytes of the same arguments): LRX_ERR_WORKSPACE; argument errors
 *               are reported before any device work; no allocation, no host synchronisation, one stream, kernels only.
 *   qtype       0 (QT_8bit) or 2 (QT_8bit_uniform); anything else is LRX_ERR_INVALID, naming it.
 *   trained     vmin ++ vdiff, fp32, 16-byte aligned: 2 dim floats for QT_8bit, 2 for QT_8bit_uniform -- lrx_sq8_ip_search's `trained`.
 *   codes       uint8, ROW-MAJOR [n_rows, dim] by stored position, CELL BY CELL, dim bytes per row (not the tiled layout of lrx_sq8_ip_search);
 *               the base pointer 16-byte aligned.  The code of v_i is lrx_sq8_encode's: u = fl32((v_i - vmin_i) / vdiff_i) (IEEE division),
 *               u = 0 where vdiff_i == 0, where v_i is below the range or NaN, u clamped to 1, code = (int)(255.f * u) by truncation.  Without
 *               centroids v = x; with them v_i = fl32(x_i - c_i), ONE fp32 subtraction of the centroid of the row's cell.
 *   decoded     y_i = fl32(vmin_i + fl32(t * vdiff_i)), t = fl32(((float)code + 0.5f) / 255) with IEEE division, no contraction: lrx_sq8_decode_rows'.
 *   score       of a scanned (query i, row) pair of the probed cell probes[i][j]:  (float)(B + sum_e (double)q_e * (double)y_e).  The sum is
 *               exact_dot's: lane `sub` of a half-wave takes elements 4 sub + 128 u + 0..3 of each 2048-element block, fp64 accumulation,
 *               the xor tree 16, 8, 4, 2, 1; B joins the reduced sum; ONE rounding.  B = 0 without by_residual; with it
 *               B = (double)probe_scores[i * ld_probe + j].  So without by_residual the result equals lrx_ivf_flat_ip_search over the fp32 rows
 *               that lrx_ivf_sq8_decode_rows returns, bit for bit, on any probe lists.
 * The chain is lrx_ivf_flat_ip_search's six launches per chunk of queries; the scan walks groups of lrx_ivf_sq8_group_rows(dim) =
 * min(128, 16384 / dim) consecutive code rows, loaded once (16 bytes per lane, non-temporal) and DECODED ONCE to fp32 in LDS (64 KiB), then
 * scored against every query that probes the cell.
 * lrx_ivf_sq8_encode_rows: one kernel -- code rows [row0, row0 + n) from x[i * ldx + e] (fp32; ldx >= dim, ldx % 4 == 0, 16-byte aligned) under
 * the rule above; cells int64 [n] (device) and centroids fp32 [nlist, dim] contiguous (NULL: no residual, and then cells may be NULL).
 * lrx_ivf_sq8_decode_rows: one kernel -- out[i * ldo + e] (fp32, ldo >= dim) = the decoded element of code row row0 + i, plus the centroid of
 * cells[i] (ONE fp32 add) when centroids are given.  In both a cells[i] outside [0, nlist) is never dereferenced: the row's codes (or decoded
 * row) are zeros and it is counted in lrx_device_error_count.  row0 + n < 2^32. */
int32_t lrx_ivf_sq8_group_rows(int32_t dim);
size_t lrx_ivf_sq8_ip_workspace_bytes(int64_t n_rows, int32_t nlist, int32_t dim, int32_t n_queries, int32_t nprobe, int32_t k,
                                      int64_t max_scan_rows);
int lrx_ivf_sq8_ip_search(const void* codes, int64_t n_rows, int32_t dim, const float* trained, int32_t qtype, const int64_t* list_off,
                          const int64_t* row_ids, int32_t nlist, const float* q, int32_t n_queries, const int64_t* probes, const float* probe_scores,
                          int32_t nprobe, int64_t ld_probe, int32_t by_residual, int64_t max_scan_rows, int32_t k, int64_t id_base,
                          float* out_scores, int64_t* out_ids, const int64_t* row_map, void* workspace, size_t workspace_bytes, void* stream);
int lrx_ivf_sq8_encode_rows(const float* x, int64_t ldx, int64_t n, int32_t dim, const float* centroids, const int64_t* cells, int32_t nlist,
                            const float* trained, int32_t qtype, void* codes, int64_t row0, void* stream);
int lrx_ivf_sq8_decode_rows(const void* codes, int64_t row0, int64_t n, int32_t dim, const float* trained, int32_t qtype, const float* centroids,
                            const int64_t* cells, int32_t nlist, float* out, int64_t ldo, void* stream);

/* (added in ABI 9, additively) GRAPH: beam search over a fixed-degree neighbour graph -- the role faiss gives GpuIndexCagra / IndexHNSWCagra
 * (GraphFlatIndex).  The caller owns the coarse step: it passes each query's entry rows.  Every output is fixed by this text:
 * the traversal is a deterministic function of the scores, the graph and the entry lists.
 *   graph       graph[u * degree + j], j < degree: int32 rows, -1 = no edge.  Row-major, contiguous.
 *   score       the flat index's score over the fp32 rows X[row * ldx + c], (float) of the fp64 sum of the fp32 products, by the device function
 *               of lrx_flat_ip_rerank: bit for bit what that entry reports for the (query, row) pair.
 *   order       everywhere (beam, output): score descending, ties to the lower row.
 *   start       the beam is the best `beam` of the query's DISTINCT VALID entry rows entry_rows[i * ld_entry + j], j < n_entry.  An entry < 0 is
 *               skipped.  An entry >= n_rows is NEVER dereferenced: it is skipped and counted in lrx_device_error_count.
 *   step        the first `width` beam entries not yet expanded, in beam order, are marked expanded and their graph rows gathered.  A graph
 *               entry is skipped when it is -1, or >= n_rows (never dereferenced; counted as above), or a row already scored for this query.
 *               Each remaining row is scored once; the beam becomes the best `beam` of (beam U new rows).  Marks travel with their entries.
 *   stop        when no beam entry is unexpanded, or after max_iterations steps (0 = the default ceil(beam / width) + 32).  The loop is bounded
 *               by that count alone: no spin-wait, no communication between workgroups, no grid barrier.
 *   result      the first k beam entries, (-FLT_MAX, -1) where fewer exist.  out_ids = id_base + row, or row_map[row] when row_map != NULL
 *               (int64 [>= n_rows], device).  out_scores / out_ids: [n_queries, k], contiguous.  out_stats: NULL or int32 [n_queries, 2] =
 *               (steps taken, rows scored).
 *   visited set THE KERNEL'S SET FORGETS: "already scored" is kept in a 4096-slot LDS table that holds at most 3072 rows; when the next gather
 *               (width * degree rows, or a slice of 1024 entries) might not fit, the table is cleared and the current beam members are put
 *               back.  A forgotten row that is met again is scored again and dropped again -- the beam's last word never decreases once the beam
 *               is full, and nothing was dropped before that -- so ids, scores and the step count are those of an exact set; only `rows scored`
 *               grows.  With beam <= 1024 and width * degree <= 128 a query scores ~3000 rows between clears.
 *   a query's result depends on its own rows of q and entry_rows alone: not on n_queries or its position in the call.
 *   limits      dim % 32 == 0, 32 <= dim <= 8192; 8 <= degree <= 128, degree % 8 == 0; 1 <= k <= beam <= 2048; 1 <= width <= 8 and
 *               width * degree <= 1024; 0 <= n_rows < 2^31; 1 <= n_entry <= 2048, ld_entry >= n_entry; 0 <= max_iterations <= 65536; ldx >= dim,
 *               ldx % 4 == 0, X and q 16-byte aligned (q [n_queries, dim] contiguous).  n_queries == 0 launches nothing.  Anything else is
 *               LRX_ERR_INVALID with a message before any device work; a workspace under lrx_graph_ip_workspace_bytes: LRX_ERR_WORKSPACE.
 * One launch on `stream`, one workgroup of 512 threads per query, no host synchronisation, no allocation, capturable in a HIP graph.  The whole
 * traversal state (beam and candidate words, the visited table, the query row up to 4096 floats) is 56 KiB of LDS; NO global scratch is used, so
 * lrx_graph_ip_workspace_bytes is 0 for every argument today and `workspace` may then be NULL -- callers still size by it.  One half-wave scores
 * one row (a random gather of whole rows, non-temporal loads); graph rows are read with ordinary loads. */
size_t lrx_graph_ip_workspace_bytes(int32_t n_queries, int32_t n_entry, int32_t degree, int32_t beam, int32_t width);
int lrx_graph_ip_search(const float* X, int64_t n_rows, int64_t ldx, int32_t dim, const int32_t* graph, int32_t degree, const float* q,
                        int32_t n_queries, const int64_t* entry_rows, int32_t n_entry, int64_t ld_entry, int32_t k, int32_t beam, int32_t width,
                        int32_t max_iterations, int64_t id_base, float* out_scores, int64_t* out_ids, const int64_t* row_map, int32_t* out_stats,
                        void* workspace, size_t workspace_bytes, void* stream);
/* (added in ABI 9, additively) The integer step of the graph build (GraphFlatIndex): detour counts over kNN lists.
 * knn int32 [n_rows, K] (row-major; -1 = empty slot), counts int32 [n_rows, K].  counts[u][c] = the number of pairs (a, b) of list positions such
 * that, with v = knn[u][a] and w = knn[v][b], w stands in knn[u] at position c > max(a, b) (a row listed twice: its first position).  Empty slots
 * take no part; an entry >= n_rows is treated as one and never dereferenced.  1 <= K <= 256, 0 <= n_rows < 2^31 (0 rows: nothing is launched);
 * anything else is LRX_ERR_INVALID before any device work.  One launch, one workgroup per row, integer work only. */
int lrx_graph_detour_counts(const int32_t* knn, int64_t n_rows, int32_t K, int32_t* counts, void* stream);

/* Score pass only: scores[Q, ld] fp32 with ld = lrx_flat_ip_score_ld(N); columns >= N hold -FLT_MAX. */
int64_t lrx_flat_ip_score_ld(int64_t n_rows);
int lrx_flat_ip_scores(const float* X, int64_t n_rows, int64_t ldx, int32_t dim, const float* q, int32_t n_queries,
                       float* scores, void* stream);

/* Merge R per-shard result lists (after the RCCL all-gather of [Q,k] pairs; replaces faiss IndexShards' host merge
 * used via index_cpu_to_all_gpus, retriever/faiss_index.py:65-68) : in_scores/in_ids [R, Q, k] -> out [Q, k].
 * Limits: R * k <= 16384 (one LDS-resident bitonic merge per query); ids are carried as 32 bits inside the merge: 0 <= id < 2^32. */
int lrx_merge_topk(const float* in_scores, const int64_t* in_ids, int32_t n_parts, int32_t n_queries, int32_t k,
                   float* out_scores, int64_t* out_ids, void* stream);
/* The exchange form: one 64-bit word per hit (fp32 score bits << 32 | global row as uint32, 0xFFFFFFFF = none), so the
 * all-gather moves a single [Q, k] int64 array per rank.  lrx_pack_topk builds it from a shard's (scores, ids) -- row_map (may be
 * NULL) turns shard-local rows (ids - id_base) into global rows; ids < 0 stay "none"; global rows must be < 2^32 - 1 --
 * lrx_merge_topk_packed merges the gathered [R, Q, k] words (R * k <= 16384) with lrx_merge_topk's ordering rule.               */
int lrx_pack_topk(const float* scores, const int64_t* ids, const int64_t* row_map, int64_t id_base, int64_t n,
                  uint64_t* out_packed, void* stream);
int lrx_merge_topk_packed(const uint64_t* in_packed, int32_t n_parts, int32_t n_queries, int32_t k, float* out_scores,
                          int64_t* out_ids, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LRX_H */

/* cake_hip — C-ABI drop-in boundary for cake's layer-sharded LLM hot path,
 * implemented MI355X-native (hand-written HIP/CDNA4 kernels for gfx950,
 * RCCL point-to-point over xGMI for the inter-shard activation hop).
 *
 * This header is the FFI seam a Rust host (cake-core) would dlopen/bind,
 * mirroring the seam cake already proved in backends/rocm/ffi.rs:12-51.
 * Each entry point cites the reference interface it replaces
 * (file:line into /root/reference/cake-core/src).  See INTEGRATION.md for
 * the reference-side binding a cake maintainer would add.
 *
 * Conventions (mirrors backends/mod.rs:40-685 + cake/mod.rs:511-556):
 *   - every function returns 0 on success, nonzero error code otherwise;
 *     cake_hip_last_error() returns a human-readable message for the last
 *     failure on this thread (mirrors the Result/anyhow error strings the
 *     Forwarder contract uses, cake/mod.rs:520-533);
 *   - plain pointers + sizes only, no torch/candle types;
 *   - host-side f32 buffers at the boundary; the engine stores/computes
 *     bf16 with f32 accumulation on device (matching cake's CUDA backend
 *     dtype policy, attention.rs:270-277 + ops.cu f32 accumulators);
 *   - all engine calls are synchronous at the API boundary unless noted
 *     (ComputeBackend::synchronize semantics, backends/mod.rs:682-684).
 */
#ifndef CAKE_HIP_H
#define CAKE_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct cake_engine cake_engine;

/* ---- error reporting (mirrors backends/rocm/ffi.rs error-seam) ---------- */
const char *cake_hip_last_error(void);

/* ---- engine lifecycle ----------------------------------------------------
 * Replaces Context::from_args + TextModelBase::load
 * (cake/mod.rs:114-507, models/common/text_model.rs:150-263).
 *
 * config_json: contents of an HF-style config.json (the same file cake
 *   auto-detects, cake/mod.rs:82-110,268-274).
 * layer_lo/layer_hi: this shard's contiguous transformer-layer range
 *   [lo, hi) — cake's contiguous-range assignment (sharding/default.rs:11-130).
 * flags: CAKE_HIP_HAS_EMBED | CAKE_HIP_HAS_HEAD on the master-analog rank
 *   (embedding + lm_head live on rank 0, text_model.rs:158-193).
 * max_seq: KV-cache capacity in tokens (replaces cake's cat-per-token
 *   cache, cache.rs:195-196, with a preallocated device cache).
 * max_batch_tokens: largest prefill chunk (activation workspace rows).
 * device: HIP device ordinal for this process.
 */
enum {
  CAKE_HIP_HAS_EMBED = 1,
  CAKE_HIP_HAS_HEAD = 2,
  CAKE_HIP_USE_GRAPH = 4,   /* capture the decode step as a hipGraph */
  CAKE_HIP_STATS = 8,       /* per-kernel hipEvent timing (bench roofline) */
};

int cake_hip_engine_create(const char *config_json, int layer_lo,
                           int layer_hi, int flags, int max_seq,
                           int max_batch_tokens, int device,
                           cake_engine **out);

/* Resolve a cake topology YAML (sharding/topology.rs:134-169, including
 * "model.layers.0-15" range expressions, topology.rs:13,142-166) to the
 * contiguous layer range of `node_name`.  Returns an error if the node's
 * layers are non-contiguous (the build keeps cake's contiguous-range
 * model, SURVEY.md §2 topology row). */
int cake_hip_topology_node_range(const char *topology_yaml,
                                 const char *node_name, int *lo, int *hi);

void cake_hip_engine_free(cake_engine *e);

/* ---- weight loading ------------------------------------------------------
 * Replaces the safetensors VarBuilder path (utils/mod.rs:251-370): mmap the
 * file, select this shard's tensors by the "model.layers.N." prefix, and
 * upload straight to HBM as bf16.  F32, F16 and BF16 source dtypes accepted.
 * quantization_config.quant_method selects the weight format: "fp8"
 * (weight + weight_scale_inv) or "gptq" (4-bit qweight / qzeros / scales,
 * kept packed in HBM; bits 4, desc_act false, group_size % 32 == 0).
 * model_type "qwen2" (Qwen2 / Qwen2.5) additionally REQUIRES
 * model.layers.N.self_attn.{q,k,v}_proj.bias (F32, F16 or BF16, one
 * dimension) in every weight format; they are kept as one fused f32 row per
 * layer, and a missing or mis-shaped one is an error that names the tensor.
 * Other model types ignore bias tensors; a config with attention_bias or
 * mlp_bias true on another model type is refused at create (error 5).
 * model_type "phi3" (Phi-3, Phi-4-mini, Phi-4) reads the checkpoint's fused
 * tensors instead of the split ones: self_attn.qkv_proj (q|k|v rows) and
 * mlp.gate_up_proj (gate rows, then up rows), as .weight or, for gptq, as
 * .qweight/.qzeros/.scales; a missing or mis-shaped one is an error that names
 * it, and phi3 with fp8 is refused at create.
 * head_dim (or hidden_size / num_attention_heads) must be a multiple of 8 in
 * [8, 128], or exactly 256 (Falcon3); anything else is refused at create
 * (error 5) ahead of any device call.
 *
 * Rotary embedding read from config_json, for any model type:
 *  - partial_rotary_factor (top level, or inside rope_parameters; absent = 1):
 *    rd = (int)(head_dim * factor) leading dims of each head rotate, the rest
 *    pass through.  rd and head_dim - rd must be multiples of 4; rd < head_dim
 *    with QK-norm or with the qwen2 bias is refused (error 5).
 *  - rope_scaling / rope_parameters of type "llama3", or "longrope" / "su"
 *    (short_factor and long_factor of rd/2 entries each,
 *    original_max_position_embeddings in the dict or at top level, optional
 *    factor and attention_factor; HF _compute_longrope_parameters).  The
 *    LongRoPE list is chosen ONCE per engine: long_factor if the engine's
 *    max_seq exceeds original_max_position_embeddings, else short_factor.  HF
 *    transformers chooses per forward call by the current length and drops its
 *    cache at the crossing, which one preallocated cache cannot do: create the
 *    engine with max_seq <= original_max_position_embeddings to serve short
 *    contexts with the short list.  Other scaling types are ignored. */
int cake_hip_load_safetensors(cake_engine *e, const char *path);

/* Seeded random init on device (synthetic-weights benches; no network for
 * checkpoints).  RMS weights = 1, linear weights ~ scale * uniform(-1,1);
 * qwen2's q/k bias rows ~ uniform(-3,3), its v rows ~ uniform(-.25,.25). */
int cake_hip_init_random(cake_engine *e, uint64_t seed, float scale);

/* ---- generation ----------------------------------------------------------
 * Replaces TextModelBase::next_token / forward
 * (text_model.rs:266-368,397-495): greedy = ArgMax (text_model.rs:104).
 *
 * prefill: run the whole prompt (index_pos 0 after reset, or appended at the
 * current position), return the next greedy token and optionally the full
 * last-position logits (f32, vocab_size).  Only meaningful on the rank with
 * HAS_EMBED|HAS_HEAD; other ranks pass tokens=NULL and participate via the
 * RCCL pipeline.  n_tokens must match across ranks. */
int cake_hip_prefill(cake_engine *e, const uint32_t *tokens, int n_tokens,
                     uint32_t *next_token, float *logits_out);

/* decode: run `steps` greedy KV-cached decode steps from the current state
 * (context size 1 per step, text_model.rs:400-420).  tokens_out (rank 0
 * only, may be NULL on other ranks) receives the generated ids. */
int cake_hip_decode(cake_engine *e, int steps, uint32_t *tokens_out);

/* Clear KV cache + position — Goodbye semantics (worker.rs:364-384,
 * cache.rs:248-253). */
int cake_hip_reset(cake_engine *e);

/* ---- Forwarder mirror ----------------------------------------------------
 * Forwarder::forward / forward_batch (cake/mod.rs:519-546): run this
 * shard's blocks [layer_lo, layer_hi) on host-f32 hidden states
 * (seq, hidden), with KV appended at index_pos.  This is the unit the
 * worker serve-loop executes per Message::Batch (sharding/worker.rs:299-578)
 * and what the parity tests drive. */
int cake_hip_forward_hidden(cake_engine *e, const float *x, int seq,
                            int index_pos, float *out);

/* Same, over a contiguous SUB-range [lo_abs, hi_abs) of this shard's
 * layers (absolute layer indices).  The reference worker runs each op of a
 * Batch/SingleOp independently by layer name (worker.rs:442-515), so a
 * master may legally drive any subset of the shard — this is the entry the
 * wire worker maps those ops onto. */
int cake_hip_forward_hidden_range(cake_engine *e, const float *x, int seq,
                                  int index_pos, int lo_abs, int hi_abs,
                                  float *out);

/* ---- cluster transport ---------------------------------------------------
 * Replaces the TCP/zstd wire hop (sharding/client.rs:79-174 +
 * proto/message.rs) with an RCCL communicator over xGMI: the per-token
 * activation exchange becomes ncclSend/ncclRecv between adjacent ranks. */
#define CAKE_HIP_COMM_ID_BYTES 128
int cake_hip_comm_id(uint8_t out[CAKE_HIP_COMM_ID_BYTES]);
int cake_hip_comm_init(cake_engine *e, int rank, int world_size,
                       const uint8_t id[CAKE_HIP_COMM_ID_BYTES]);

/* ---- op-level surface (ComputeBackend mirror, for kernel parity tests) ---
 * Host f32 in/out; the engine quantizes to bf16, runs the gfx950 kernel,
 * and returns f32 — tests compare against oracle/ on bf16-quantized inputs.
 * These are NOT the product generation path; they exercise the same kernels
 * the path uses. */
/* backends/mod.rs:244-246 */
int cake_hip_op_rms_norm(int rows, int cols, float eps, const float *x,
                         const float *w, float *out, int device);
/* backends/mod.rs:206-241 — out[m,n] = sum_k x[m,k] * w[n,k]; w is (N,K) */
int cake_hip_op_linear(int M, int N, int K, const float *x, const float *w,
                       float *out, int device);
/* backends/mod.rs:82 + ops.cu:101-138 */
int cake_hip_op_silu_mul(long n, const float *gate, const float *up,
                         float *out, int device);
/* backends/mod.rs:444-482 — x (B,H,S,D), cos/sin (S, D/2) */
int cake_hip_op_rope(int b, int h, int s, int d, const float *x,
                     const float *cosv, const float *sinv, float *out,
                     int device);

/* Attention + KV-store op entries (test-only).  Every call allocates
 * buffers of exactly the engine's sizes, runs the real launch wrappers on a
 * private stream and frees the buffers.  Arguments are validated before any
 * device call (error 5): nh % nkv == 0; hd % 8 == 0 and 8 <= hd <= 128, or
 * hd == 256;
 * max_seq % 32 == 0; pos0 + S <= max_seq; 1 <= nchunk <= 64; the variant
 * must be one the prefill dispatcher can express.
 *
 * kv_store: rope [+ per-head QK-norm] + cache store of S raw qkv rows
 * (S, (nh+2*nkv)*hd) at positions pos0.. (decode != 0: the one-row decode
 * kernel at position pos0).  cos/sin are (max_seq, hd/2) f32 tables;
 * q_norm/k_norm are (hd) rows or both NULL.  kc/vc (nkv, max_seq, hd) and
 * vtc (nkv, hd, max_seq) are IN/OUT host images; q_out (S, nh*hd) receives
 * the roped q rows. */
int cake_hip_op_kv_store(int S, int pos0, int decode, int nh, int nkv, int hd,
                         int max_seq, const float *qkv, const float *cosv,
                         const float *sinv, const float *q_norm,
                         const float *k_norm, float eps, float *kc, float *vc,
                         float *vtc, float *q_out, int device);
/* kv_store with the q|k|v projection bias of qwen2: bias ((nh+2*nkv)*hd f32,
 * may be NULL) is added to every raw row in f32 ahead of the rotation (q, k)
 * and of the store (v).  NULL is op_kv_store bit for bit.  A bias together
 * with q_norm/k_norm is refused (error 5). */
int cake_hip_op_kv_store_bias(int S, int pos0, int decode, int nh, int nkv,
                              int hd, int max_seq, const float *qkv,
                              const float *cosv, const float *sinv,
                              const float *q_norm, const float *k_norm,
                              float eps, const float *bias, float *kc,
                              float *vc, float *vtc, float *q_out,
                              int device);
/* kv_store with partial rotary: only the first rd dims of each q and k head
 * rotate, cosv / sinv are (max_seq, rd/2); q's remaining dims stay as they
 * are, k's are copied to the cache.  rd and hd - rd must be multiples of 4;
 * rd < hd with q_norm/k_norm is refused.  rd == hd is op_kv_store bit for
 * bit. */
int cake_hip_op_kv_store_pr(int S, int pos0, int decode, int nh, int nkv,
                            int hd, int rd, int max_seq, const float *qkv,
                            const float *cosv, const float *sinv,
                            const float *q_norm, const float *k_norm,
                            float eps, float *kc, float *vc, float *vtc,
                            float *q_out, int device);
/* Causal [sliding-window] GQA attention of S post-rope q rows (S, nh*hd) at
 * positions pos0.. over the cache images; out (S, nh*hd).  Variant: hd 128
 * takes pfv 1 (nw 8, no split/deep) or pfv 2 with nw 4|8 and at most one of
 * split (0|1) / deep (0|1|2); hd 256 takes {1,4,0,0} (the MFMA-256 kernel)
 * or {0,0,0,0} (the plain hd-256 kernel); any other hd takes {0,0,0,0}
 * (generic kernel). */
int cake_hip_op_attn_prefill(int S, int pos0, int nh, int nkv, int hd,
                             int max_seq, int window, int pfv, int nw,
                             int split, int deep, const float *q,
                             const float *kc, const float *vc,
                             const float *vtc, float *out, int device);
/* Decode attention of one q row (nh*hd) at position pos, split over nchunk
 * chunks.  The arrival counters are zeroed once, then the kernel is launched
 * `repeats` (1..16) times back to back; out is (repeats, nh*hd). */
int cake_hip_op_attn_decode(int nh, int nkv, int hd, int max_seq, int pos,
                            int window, int nchunk, int repeats,
                            const float *q, const float *kc, const float *vc,
                            float *out, int device);
/* Host only: the launch choices the product makes for a prefill of S rows and
 * for decode at this head geometry: out = {pfv, nw, split, deep,
 * split_min_s, decode grid_y (0 = per-head kernel)}. */
int cake_hip_attn_dispatch(int S, int nh, int nkv, int hd, int out[6]);
/* Host only: the decode-attention kernel the product launches for this head
 * geometry and chunk count: 0 = per-head, 1 = grouped, 2 = short-context
 * (all chunks of a head in one workgroup; nchunk 4), 3 = the hd-256 kernel.
 * CAKE_ATTN_SHORT, read on every call: 0 = never the short kernel, 2 = also
 * at nchunk 8. */
int cake_hip_attn_decode_path(int nh, int nkv, int hd, int nchunk);
/* Host only: q-heads served by one block of the decode-attention kernel at
 * this geometry.  hd 256: the largest of 4, 3, 2, 1 that divides nh / nkv,
 * capped by CAKE_ATTN256_GB (read on every call).  The cap defaults to 1 (per
 * head), which measured faster; 2..4 opt in to the grouped kernel. */
int cake_hip_attn_decode_group(int nh, int nkv, int hd);
/* cake_hip_op_attn_decode with a chunk count PER LAUNCH: nlaunch (1..16)
 * launches back to back on one set of buffers, launch i split over
 * nchunks[i]; out is (nlaunch, nh*hd).  cnt_out (nh words, may be NULL)
 * receives the arrival counters after the last launch; they start at 0. */
int cake_hip_op_attn_decode_seq(int nh, int nkv, int hd, int max_seq, int pos,
                                int window, int nlaunch, const int *nchunks,
                                const float *q, const float *kc,
                                const float *vc, float *out,
                                uint32_t *cnt_out, int device);

/* Linear-layer op entries (test-only): GEMV, fp8 GEMV, gate-up, fused
 * qkv-rope, prefill GEMM, fp8 dequant.  Conventions of the attention entries
 * (private buffers of exact size, private stream, arguments validated before
 * any device call: error 5).  Every OUTPUT buffer has CAKE_HIP_OP_GUARD
 * elements past its end and starts filled with CAKE_HIP_OP_SENTINEL; the
 * guards are returned behind the payload, so a store past the end or an
 * element that no block wrote shows.  bf16 tensors cross as f32. */
#define CAKE_HIP_OP_GUARD 16
#define CAKE_HIP_OP_SENTINEL (-1152921504606846976.0f) /* -2^60 */
/* kind 0: launch_gemv (bf16 w (N,K)); 1: launch_gemv_fp8 (w8 (N,K) e4m3fn
 * bytes + sc (N/128, K/128) f32; N % 128 == 0, K % 128 == 0); 2: the
 * split-K residual GEMV (bf16, K % 16 == 0, epi 1 only).  K % 8 == 0, K >= 8.
 * epi 0: bf16 out; 1: bf16 out + res; 2: f32 out.  nw != NULL fuses the
 * rms_norm with eps (K <= 16384).  rows: output rows per block, 0 = the
 * product's policy (bf16 1|2|4|8, fp8 4|8).  alias: out == res, as the
 * engine's o/down projections run.  The kernel is launched `repeats` (1..16)
 * times back to back, repeat i on x row i and res row i; out is
 * (repeats, N + CAKE_HIP_OP_GUARD).
 * Counters are set once, before the first launch: split-K sets every arrival
 * word to cnt_init[0]; chain 1 (fp8 norm-chain produce, epi 1) sets the nine
 * words to cnt_init[0..9) and returns scale_out[repeats]; chain 2 (consume)
 * normalizes x with *scale_in and the nw row instead of the fused norm. */
int cake_hip_op_gemv(int kind, int N, int K, int epi, int rows, int alias,
                     int repeats, const float *x, const float *w,
                     const uint8_t *w8, const float *sc, const float *res,
                     const float *nw, float eps, int chain,
                     const uint32_t *cnt_init, const float *scale_in,
                     float *scale_out, float *out, int device);
/* out[c] = silu(g_c) * u_c, g = W[c,:].xn, u = W[I+c,:].xn; w is (2I, K).
 * bf16: rows 0|4|8.  fp8: I % 128 == 0, K % 128 == 0, sc (2I/128, K/128);
 * scale_in != NULL is the norm-chain consume (needs nw).  K <= 16384.
 * out is (I + CAKE_HIP_OP_GUARD). */
int cake_hip_op_gemv_gateup(int fp8, int I, int K, int rows, const float *x,
                            const float *w, const uint8_t *w8,
                            const float *sc, const float *nw, float eps,
                            const float *scale_in, float *out, int device);
/* Fused rms_norm -> qkv GEMV -> rope -> KV store of one decode row at `pos`.
 * w ((nh+2*nkv)*hd, K); cos/sin (max_seq, hd/2) f32; kc/vc/vtc IN/OUT images
 * as in op_kv_store; out ((nh+2*nkv)*hd + CAKE_HIP_OP_GUARD) is the qkv
 * activation row: the roped q rows, then sentinels (k and v go to the cache
 * only). */
int cake_hip_op_gemv_qkv_rope(int nh, int nkv, int hd, int max_seq, int pos,
                              int K, const float *x, const float *nw,
                              float eps, const float *w, const float *cosv,
                              const float *sinv, float *kc, float *vc,
                              float *vtc, float *out, int device);
/* The same with the bias row of op_kv_store_bias: non-NULL runs the biased
 * kernel (bias joins the f32 sums), NULL the unbiased one. */
int cake_hip_op_gemv_qkv_rope_bias(int nh, int nkv, int hd, int max_seq,
                                   int pos, int K, const float *x,
                                   const float *nw, float eps, const float *w,
                                   const float *cosv, const float *sinv,
                                   const float *bias, float *kc, float *vc,
                                   float *vtc, float *out, int device);
/* The same with partial rotary (tables (max_seq, rd/2)): rd < hd runs
 * k_gemv_qkv_rope_pr, rd == hd the full-rotation kernel (op_gemv_qkv_rope bit
 * for bit). */
int cake_hip_op_gemv_qkv_rope_pr(int nh, int nkv, int hd, int rd, int max_seq,
                                 int pos, int K, const float *x,
                                 const float *nw, float eps, const float *w,
                                 const float *cosv, const float *sinv,
                                 float *kc, float *vc, float *vtc, float *out,
                                 int device);
/* C[M,N] = A[M,K] @ W[N,K]^T (+ res) by an explicit variant: 0 128^2 tile,
 * 1 256^2, 2 128x256, 3 256^2 fine-phase, 4 hipBLASLt.  Variants 1..3 need
 * K % 64 == 0 (any number of 64-wide tiles >= 1); 0 and 4 take K % 8 == 0.
 * alias: C == res.  *ran = the variant that ran, or -1 when the library
 * rejected the shape (out then holds sentinels, or res when aliased).  out is
 * (M*N + CAKE_HIP_OP_GUARD). */
int cake_hip_op_gemm(int variant, int M, int N, int K, int epi, int alias,
                     const float *a, const float *w, const float *res,
                     float *out, int *ran, int device);
/* Blockwise fp8 -> bf16 dequant (N % 128 == 0, K % 128 == 0); out is
 * (N*K + CAKE_HIP_OP_GUARD). */
int cake_hip_op_dequant_fp8(int N, int K, const uint8_t *w8, const float *sc,
                            float *out, int device);
/* GPTQ 4-bit op entries.  The tensors are in CHECKPOINT layout and pass
 * through the loader's own repack: qweight (K/8, N) int32 (nibble b of word
 * [r, j] is q(8r + b, j)), qzeros (K/group, N/8) int32 (nibble j % 8 of word
 * [gi, j / 8] is z(gi, j)), scales (K/group, N) f32 holding f16-representable
 * values; W[j, k] = (q - (z + 1)) * s.  Rules (error 5): group % 32 == 0,
 * K % group == 0, 32 <= K <= 32768, N % 8 == 0.
 * gemv_w4: epi 0 bf16 out, 1 bf16 out + res; rows 0 (policy) | 4 | 8 (8
 * needs K <= 16384); alias: out == res; the kernel is launched `repeats`
 * (1..16) times, repeat i on x row i and res row i; out is
 * (repeats, N + CAKE_HIP_OP_GUARD). */
int cake_hip_op_gemv_w4(int N, int K, int group, int epi, int rows, int alias,
                        int repeats, const float *x, const int32_t *qweight,
                        const int32_t *qzeros, const float *scales,
                        const float *res, float *out, int device);
/* out[c] = silu(g_c) * u_c over one fused tensor of N = 2I rows (gate rows
 * [0, I), up rows [I, 2I)); x is already normalized.  I % 8 == 0,
 * K <= 16384, rows 0 | 4.  out is (I + CAKE_HIP_OP_GUARD). */
int cake_hip_op_gemv_gateup_w4(int I, int K, int group, int rows,
                               const float *x, const int32_t *qweight,
                               const int32_t *qzeros, const float *scales,
                               float *out, int device);
/* 4-bit -> bf16 (N, K) row-major, as the prefill path dequantizes into its
 * scratch; out is (N*K + CAKE_HIP_OP_GUARD). */
int cake_hip_op_dequant_w4(int N, int K, int group, const int32_t *qweight,
                           const int32_t *qzeros, const float *scales,
                           float *out, int device);
/* Prefill silu_mul over S rows of gu (S, 2I) = [gate | up]: out[s, c] =
 * silu(gu[s, c]) * gu[s, I + c]; I % 8 == 0.  out is
 * (S*I + CAKE_HIP_OP_GUARD). */
int cake_hip_op_silu_mul_rows(int S, int I, const float *gu, float *out,
                              int device);
/* rms_norm of outer*inner rows of `cols` elements inside one buffer of n
 * elements: row r starts at (r / inner) * outer_stride + (r % inner) * cols
 * (the per-head QK-norm layout; inner = rows, outer = 1 is the plain form).
 * cols % 8 == 0, outer_stride % 8 == 0, outer_stride >= inner * cols,
 * n == (outer-1) * outer_stride + inner * cols.  out is
 * (n + CAKE_HIP_OP_GUARD) in the same layout; elements between the rows keep
 * the sentinel. */
int cake_hip_op_rms_norm_rows(int outer, int inner, long outer_stride,
                              int cols, float eps, long n, const float *x,
                              const float *w, float *out, int device);
/* Host only: the kernel the product launches for a linear layer.  kind 0
 * plain GEMV (n = N), 1 gate-up GEMV (n = I), 2 fused qkv-rope GEMV, 3
 * split-K residual GEMV, 4 prefill GEMM (M rows).  out = {family
 * (CAKE_HIP_FAM_*), rows per block, KB (k blocks held in registers; 0 = the
 * streaming kernel), GEMM: library first (0|1), GEMM: hand-written variant}. */
enum {
  CAKE_HIP_FAM_GEMV_REG = 0,
  CAKE_HIP_FAM_GEMV_STREAM = 1,
  CAKE_HIP_FAM_GEMV_FP8 = 2,
  CAKE_HIP_FAM_GEMV_FP8_STREAM = 3,
  CAKE_HIP_FAM_GATEUP = 4,
  CAKE_HIP_FAM_GATEUP_FP8 = 5,
  CAKE_HIP_FAM_QKV_ROPE = 6,
  CAKE_HIP_FAM_SPLITK = 7,
  CAKE_HIP_FAM_GEMM = 8,
  CAKE_HIP_FAM_GEMV_W4 = 9,
  CAKE_HIP_FAM_GATEUP_W4 = 10,
  CAKE_HIP_FAM_GATEUP_GELU = 11, /* gemma3: the GELU-tanh twin of GATEUP */
};
/* fp8 is the quant selector: 0 bf16, 1 fp8.  The 4-bit (gptq) kernels need a
 * group size and are queried through cake_hip_linear_dispatch_w4. */
int cake_hip_linear_dispatch(int kind, int n, int K, int M, int fp8,
                             int out[5]);
/* Host only: the 4-bit kernel for kind 0 (plain GEMV, n = N) or 1 (gate-up,
 * n = I) at this K and group size (-1 = K); out as above, KB counting
 * 4096-wide k blocks (1 = two half-block row sets).  Error 5 when the shape
 * breaks a rule of the 4-bit path (see cake_hip_op_gemv_w4). */
int cake_hip_linear_dispatch_w4(int kind, int n, int K, int group,
                                int out[5]);
/* Host only: the five linear launches of one decode step of the model in
 * config_json, chosen by the predicates the engine itself uses: out[3*i..] =
 * {family, rows, KB} for i = qkv, o, gate-up, down, head.  The opt-in
 * split-K residual GEMV is not reflected. */
int cake_hip_decode_dispatch(const char *config_json, int out[15]);
/* Host only: the rope tables engine create builds for config_json at this
 * max_seq (a positive multiple of 32, as create rounds it), through the same
 * function: cosv and sinv are (max_seq, rd/2) f32 and may be NULL; *rd_out is
 * the rotated dims per head.  Every config refusal of create that concerns
 * the rotary fields is reported here as well (error 5). */
int cake_hip_rope_tables(const char *config_json, int max_seq, float *cosv,
                         float *sinv, int *rd_out);
/* cake_hip_rope_tables with a table selector: which 0 is that table (the
 * global layers' of a gemma3 config), which 1 the local (sliding) layers'
 * table, which only a gemma3 config has (error 5 otherwise). */
int cake_hip_rope_tables_ex(const char *config_json, int max_seq, int which,
                            float *cosv, float *sinv, int *rd_out);
/* Host only: what engine create plans for layer `layer` of config_json:
 * *window the attention span (0 = full), *rope_table 0 (global) or 1 (the
 * gemma3 local table), *q_scale the factor folded into the q-norm row
 * (sqrt(head_dim / query_pre_attn_scalar) for gemma3, else 1).  Any of the
 * three may be NULL.  Every config refusal of create is reported (error 5). */
int cake_hip_layer_dispatch(const char *config_json, int layer, int *window,
                            int *rope_table, float *q_scale);

/* ---- observability (bench roofline evidence) ----------------------------
 * JSON {"kernels": {name: {"launches": n, "ms": t, "bytes": b}}} — per-
 * kernel-family hipEvent timing + algorithmic bytes, collected while
 * CAKE_HIP_STATS was set (SURVEY.md §5 metrics row). */
int cake_hip_kernel_stats(cake_engine *e, char *buf, int cap);

/* Sampling config (create_logits_processor, text_model.rs:102-118):
 * temperature <= 0 => greedy ArgMax; > 0 => Gumbel-argmax at that
 * temperature (the on-GPU sampling trick cake uses, text_model.rs:108-111).
 * The noise stream is seeded and deterministic per (seed, step). */
int cake_hip_set_sampling(cake_engine *e, float temperature, uint64_t seed);
/* The rest of create_logits_processor (text_model.rs:102-118: TopK, TopP,
 * TopKThenTopP) and the repeat penalty the reference applies before every
 * sample (text_model.rs:433-452, helper :51-99; defaults 1.1 over the last
 * 128 tokens, lib.rs:193-198), all on the device and inside the decode and
 * prefill graphs:
 *   1. penalty: every unique id among the last repeat_last_n SAMPLED tokens
 *      (prompt tokens never count) gets l * (1/penalty) if l >= 0, else
 *      l * penalty; off when penalty == 1 or repeat_last_n == 0
 *   2. top-k: keep the k largest; off when top_k <= 0 or >= vocab
 *   3. top-p: among those, softmax at `temperature`, keep the minimal
 *      descending prefix whose mass reaches top_p; off when <= 0 or >= 1
 *   4. seeded Gumbel-argmax over the kept set; temperature <= 0 is the
 *      argmax of the penalised logits (top-k / top-p moot)
 * Tie rule: every entry equal to the boundary value of step 2 or 3 is kept,
 * so the kept set is { l' >= tau } and may exceed k on exact f32 ties.
 * The noise is indexed by a persistent draw counter that, like the history,
 * advances on every sampled token (prefill's included) and is cleared by
 * cake_hip_reset and by either setter.  Logits returned by cake_hip_prefill
 * stay unpenalised.  With all three options off this call IS
 * cake_hip_set_sampling(temperature, seed); cake_hip_set_sampling switches
 * them off again.  Error 5: repeat_last_n outside [0,1024], repeat_penalty
 * <= 0, NaN arguments, or an engine without the head / vocab > 2^18. */
int cake_hip_set_sampling_ex(cake_engine *e, float temperature, int top_k,
                             float top_p, float repeat_penalty,
                             int repeat_last_n, uint64_t seed);
/* Test-only: the sampler's launch wrapper on private buffers and a private
 * stream.  Runs `draws` (1..8192) consecutive draw indices from first_draw
 * on the same logits (V <= 2^18) and the same history (n_history <= 1024
 * ids < V, all of them penalised); tokens_out[draws], *kept_out = size of
 * the kept set, *thr_out = tau, the smallest kept penalised logit.
 * Arguments are validated before any device call (error 5). */
int cake_hip_op_sample(int V, const float *logits, float temperature,
                       int top_k, float top_p, float repeat_penalty,
                       const uint32_t *history, int n_history,
                       uint64_t seed, int first_draw, int draws,
                       uint32_t *tokens_out, int *kept_out, float *thr_out,
                       int device);
/* Test-only: `steps` (1..8192) consecutive launch_argmax calls on the same
 * f32 logits (V <= 2^24), private buffers and stream.  temperature <= 0 is
 * the greedy argmax, > 0 the seeded Gumbel-argmax.  The device step counter
 * starts at first_step (<= 2^20), pos at 0.  use_ring 0 passes a null ring
 * (the step counter then stays put).  Contract of the token: the first index
 * whose value equals the maximum over the non-NaN entries; 0 when no entry
 * is greater than -inf; always < V.
 * tokens_out[steps]: the token word after each launch.  pval_out / pidx_out
 * (256 + CAKE_HIP_OP_GUARD each): the partials of the LAST launch.  ring_out
 * (first_step + steps + CAKE_HIP_OP_GUARD words, ignored without use_ring):
 * the whole ring.  Partials, ring and their guards start as the bit pattern
 * of CAKE_HIP_OP_SENTINEL.  pos_step_out = {pos, step} after the last launch.
 * Arguments are validated before any device call (error 5). */
int cake_hip_op_argmax(int V, const float *logits, float temperature,
                       uint64_t seed, int first_step, int steps, int use_ring,
                       int advance_pos, uint32_t *tokens_out, float *pval_out,
                       int32_t *pidx_out, uint32_t *ring_out,
                       int *pos_step_out, int device);
/* Test-only: the embedding gathers on table (Vt, H), which crosses as f32 and
 * is uploaded through the f32 -> bf16 conversion.  mode 0: launch_embed_rows
 * on S ids; 1: launch_embed_token on one id; 2: the same, also producing the
 * fp8 norm chain's nscale = 1/sqrt(mean(x^2) + eps).  H % 8 == 0,
 * 8 <= H <= 16384 (what engine create accepts); ids < Vt.  out is
 * (S*H + CAKE_HIP_OP_GUARD); nscale_out is (1 + CAKE_HIP_OP_GUARD) and keeps
 * the sentinel unless mode 2. */
int cake_hip_op_embed(int Vt, int H, int S, int mode, const float *table,
                      const uint32_t *ids, float eps, float *out,
                      float *nscale_out, int device);
/* Test-only, gemma3 (kernels_gemma.hip); outputs carry CAKE_HIP_OP_GUARD
 * guard elements like the entries above, and arguments are validated before
 * any device call (error 5).
 * x (S, H) = bf16(x + bf16(rms_norm(t) * w)), the post-norm + residual add;
 * S == 1 is the decode launch, S > 1 the prefill one.  H % 8 == 0,
 * 8 <= H <= 16384, S <= 4096.  out is (S*H + guard). */
int cake_hip_op_postnorm_add(int S, int H, float eps, const float *x,
                             const float *t, const float *w, float *out,
                             int device);
/* [rms_norm ->] gate-up GEMV -> gelu_pytorch_tanh(gate) * up on bf16 weights
 * w (2I, K); nw may be NULL (x already normalized).  K % 8 == 0,
 * 8 <= K <= 16384, rows 0 | 4 | 8.  out is (I + guard). */
int cake_hip_op_gemv_gateup_gelu(int I, int K, int rows, const float *x,
                                 const float *w, const float *nw, float eps,
                                 float *out, int device);
/* Prefill gelu_mul over S rows of gu (S, 2I) = [gate | up]; any I >= 1 (a
 * multiple of 8 runs the vector loop the engine uses).  out is
 * (S*I + guard). */
int cake_hip_op_gelu_mul_rows(int S, int I, const float *gu, float *out,
                              int device);
/* The embedding gathers times bf16(sqrt(H)), rounded to bf16.  mode 0: rows
 * on S ids; 1: the token form on one id.  Limits as cake_hip_op_embed.  out
 * is (S*H + guard). */
int cake_hip_op_embed_scaled(int Vt, int H, int S, int mode,
                             const float *table, const uint32_t *ids,
                             float *out, int device);
int cake_hip_stats_reset(cake_engine *e);
int cake_hip_set_stats(cake_engine *e, int enabled);

int cake_hip_sync(cake_engine *e);

/* build info: returns "gfx950;<compile date>" */
const char *cake_hip_build_info(void);

#ifdef __cplusplus
}
#endif
#endif /* CAKE_HIP_H */

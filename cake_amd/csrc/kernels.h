// Host-side launch wrappers for the gfx950 kernels (kernels.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

using u16 = unsigned short;
using u32 = unsigned int;

void launch_f32_to_bf16(const float* in, u16* out, size_t n, hipStream_t s);
void launch_bf16_to_f32(const u16* in, float* out, size_t n, hipStream_t s);
void launch_fill_random(u16* out, size_t n, uint64_t seed, float scale,
                        hipStream_t s);
void launch_fill_const(u16* out, size_t n, float v, hipStream_t s);
void launch_rmsnorm(const u16* x, const u16* w, u16* out, int rows, int cols,
                    float eps, hipStream_t s);
void launch_rmsnorm_strided(const u16* x, const u16* w, u16* out, int outer,
                            int inner, size_t outer_stride, int cols,
                            float eps, hipStream_t s);
void launch_silu_mul(const u16* g, const u16* u, u16* out, size_t n,
                     hipStream_t s);
void launch_silu_mul_rows(const u16* gu, u16* out, int S, int I,
                          hipStream_t s);
// rows_override: output rows per block (1|2|4|8), 0 = gemv_rows_policy
void launch_gemv(const u16* W, const u16* x, void* out, const u16* res,
                 const u16* nw, float eps, int N, int K, int epi,
                 hipStream_t s, int rows_override = 0);
// host-side kernel choices of the GEMV launchers: rows per block, and the
// template KB (2048-wide k blocks for bf16, 4096-wide for fp8; 0 = the
// streaming kernel)
int gemv_rows_policy(int N, int K);
int gemv_fp8_rows_policy(int N);
int gemv_gateup_rows_policy();  // bf16 gate-up: 4, or CAKE_GU_ROWS = 8
int gemv_kb(int K);
int gemv_fp8_kb(int K);
int gemv_qkv_rope_kb(int K);
int gemv_splitk_kb(int K);
// rows: channels per block, 8 or (anything else, 0 included) 4
void launch_gemv_gateup(const u16* W, const u16* x, u16* out, const u16* nw,
                        float eps, int I, int K, int rows, hipStream_t s);
void launch_gemv_res_splitk(const u16* W, const u16* x, u16* out,
                            const u16* res, float* ws, u32* cnt, int N,
                            int K, hipStream_t s);
// fused rms_norm -> qkv GEMV -> rope -> KV-cache store (llama family).
// bias: the fused q|k|v projection bias row (Nq f32, qwen2) added to the f32
// sums; non-null runs k_gemv_qkv_rope_bias (kernels_qkv_bias.hip), null the
// unbiased kernel.  rd = rotated dims of a head: rd == hd runs these two
// kernels, rd < hd the partial-rotary form below (which takes no bias).
void launch_gemv_qkv_rope(const u16* W, const u16* x, u16* out, const u16* nw,
                          float eps, u16* kc, u16* vc, u16* vtc,
                          const float* cost, const float* sint,
                          const int* pos, int nh, int nkv, int hd, int rd,
                          int max_seq, int K, hipStream_t s,
                          const float* bias = nullptr);
// partial rotary (rd < hd, rd % 4 == 0, (hd - rd) % 4 == 0, no bias):
// k_gemv_qkv_rope_pr (kernels_qkv_pr.hip); tables are (max_seq, rd/2)
void launch_gemv_qkv_rope_pr(const u16* W, const u16* x, u16* out,
                             const u16* nw, float eps, u16* kc, u16* vc,
                             u16* vtc, const float* cost, const float* sint,
                             const int* pos, int nh, int nkv, int hd, int rd,
                             int max_seq, int K, hipStream_t s);
void launch_gemv_qkv_rope_bias(const u16* W, const u16* x, u16* out,
                               const u16* nw, float eps, u16* kc, u16* vc,
                               u16* vtc, const float* cost, const float* sint,
                               const int* pos, const float* bias, int nh,
                               int nkv, int hd, int max_seq, int K,
                               hipStream_t s);
// fp8 decode norm chain (replaces the split-norm rmsnorm LAUNCHES): the
// x-producing GEMV's epilogue publishes per-block sumsq partials of its
// QUANTIZED outputs; its last-arriving block reduces them in fixed order
// (deterministic) and writes scale_out = rsqrt(mean+eps); the consuming
// GEMV normalizes x in-register with scale_in * nw (re-quantized bf16, so
// it matches the rmsnorm-kernel-then-gemv pair bit-exactly given the same
// scale).  All pointers may be null (feature off / fallback path).
struct NormIO {
  const float* scale_in;  // consume: precomputed rms scale
  const u16* nw;          // consume: rms weight row
  float* part;            // produce: per-block sumsq partials [gridDim]
  u32* cnt;               // produce: counters[9] (8 residue shards + top)
  float* scale_out;       // produce: the scale for the NEXT consumer
  float eps;              // produce: rms_norm_eps
};
void launch_gemv_fp8(const unsigned char* W, const float* sc, const u16* x,
                     void* out, const u16* res, const u16* nw, float eps,
                     int N, int K, int epi, hipStream_t s,
                     NormIO nio = NormIO{}, int rows_override = 0);
void launch_gemv_gateup_fp8(const unsigned char* W, const float* sc,
                            const u16* x, u16* out, const u16* nw, float eps,
                            int I, int K, hipStream_t s,
                            NormIO nio = NormIO{});
void launch_dequant_fp8(const unsigned char* W, const float* sc, u16* out,
                        int N, int K, hipStream_t s);
void launch_fill_random_u8(unsigned char* out, size_t n, uint64_t seed,
                           hipStream_t s);
// GPTQ 4-bit family (kernels_w4.hip).  W: out-major packed nibbles, K/8 words
// per row; sz: (N, K/group) f32 pairs {s, -(z+1)*s}.  group % 32 == 0,
// K % group == 0, K <= 32768.  epi 0: bf16 out; 1: bf16 out + res (res may
// alias out).  rows_override: 4|8 rows per block, 0 = gemv_w4_rows_policy
// (KB 8 always runs 4).  No fused norm: x is already normalized.
int gemv_w4_kb(int K);  // 4096-wide k blocks: 1 (two half-block rows) |2|4|8
int gemv_w4_rows_policy(int N, int K);
void launch_gemv_w4(const u32* W, const float* sz, const u16* x, u16* out,
                    const u16* res, int N, int K, int group, int epi,
                    hipStream_t s, int rows_override = 0);
// 4 channels per block; K <= 16384
void launch_gemv_gateup_w4(const u32* W, const float* sz, const u16* x,
                           u16* out, int I, int K, int group, hipStream_t s);
void launch_dequant_w4(const u32* W, const float* sz, u16* out, int N, int K,
                       int group, hipStream_t s);
void launch_fill_random_u32(u32* out, size_t n, uint64_t seed, hipStream_t s);
void launch_embed_token(const u16* embed, const u32* tok, u16* x, int H,
                        hipStream_t s, float* nscale = nullptr,
                        float eps = 1e-5f);
void launch_embed_rows(const u16* embed, const u32* ids, u16* x, int S, int H,
                       hipStream_t s);
// Gemma 3 (kernels_gemma.hip).  Norm rows carry 1 + w folded in.
// x (rows, cols) = bf16(x + bf16(rms_norm(t) * w)) in place; cols % 8 == 0,
// cols <= 16384; t must not alias x
void launch_postnorm_add(u16* x, const u16* t, const u16* w, int rows,
                         int cols, float eps, hipStream_t s);
// the GELU-tanh twins of launch_gemv_gateup and launch_silu_mul_rows
void launch_gemv_gateup_gelu(const u16* W, const u16* x, u16* out,
                             const u16* nw, float eps, int I, int K, int rows,
                             hipStream_t s);
void launch_gelu_mul_rows(const u16* gu, u16* out, int S, int I,
                          hipStream_t s);
// embedding gathers times bf16(sqrt(H)), rounded to bf16; H % 8 == 0
void launch_embed_token_scaled(const u16* embed, const u32* tok, u16* x, int H,
                               hipStream_t s);
void launch_embed_rows_scaled(const u16* embed, const u32* ids, u16* x, int S,
                              int H, hipStream_t s);
// bias: the fused q|k|v projection bias row ((nh + 2*nkv)*hd f32, qwen2), added
// to the raw row in f32 before the rotation / the V store; null = none
void launch_rope_store_decode(u16* qkv, u16* kc, u16* vc, u16* vtc,
                              const float* cost, const float* sint,
                              const int* pos, int nh, int nkv, int hd, int rd,
                              int max_seq, const u16* qn, const u16* kn,
                              float eps, hipStream_t s,
                              const float* bias = nullptr);
void launch_rope_store_prefill(u16* qkv, u16* kc, u16* vc, u16* vtc,
                               const float* cost, const float* sint, int pos0,
                               int S, int nh, int nkv, int hd, int rd,
                               int max_seq, int qkv_stride, const u16* qn,
                               const u16* kn, float eps, hipStream_t s,
                               const float* bias = nullptr);
void launch_attn_decode(const u16* q, const u16* kc, const u16* vc,
                        const int* pos, float* ws, u32* cnt, u16* out, int nh,
                        int nkv, int hd, int max_seq, int nchunk, int window,
                        hipStream_t s);
// grid_y of the GQA-grouped decode-attention kernel for this head geometry
// (0 = per-head fallback kernel); the engine's chunk-count policy uses it.
// hd 256: nh / attn256_group(nh, nkv), never 0.
int attn_decode_grid_y(int nh, int nkv, int hd);
// which kernel launch_attn_decode runs for (geometry, nchunk): 0 per-head,
// 1 grouped, 2 short-context in-block split-KV (CAKE_ATTN_SHORT=0 -> 1),
// 3 the hd-256 kernel (kernels_attn256.hip)
int attn_decode_path(int nh, int nkv, int hd, int nchunk);
// hd 256 (kernels_attn256.hip).  attn256_group: q-heads per block of
// k_attn_decode_256, the largest of 4|3|2|1 dividing nh / nkv, capped by
// CAKE_ATTN256_GB (read per call; default 1 = per head, the faster route).  Same ws / cnt contract as
// launch_attn_decode, except that the elected block zeroes its cnt word.
int attn256_group(int nh, int nkv);
void launch_attn_decode_256(const u16* q, const u16* kc, const u16* vc,
                            const int* pos, float* ws, u32* cnt, u16* out,
                            int nh, int nkv, int max_seq, int nchunk,
                            int window, hipStream_t s);
// mfma != 0: k_attn_prefill_mfma_256 (reads vtc), else k_attn_prefill_256
void launch_attn_prefill_256(const u16* qkv, const u16* kc, const u16* vc,
                             const u16* vtc, u16* out, int S, int pos0,
                             int nh, int nkv, int max_seq, int qkv_stride,
                             int out_stride, int window, int mfma,
                             hipStream_t s);
// ws: split-KV partial workspace (nh * S * 2 * 132 f32) or nullptr to
// force the single-pass path
void launch_attn_prefill(const u16* qkv, const u16* kc, const u16* vc,
                         const u16* vtc, u16* out, float* ws, int S, int pos0,
                         int nh, int nkv, int hd, int max_seq, int qkv_stride,
                         int out_stride, int window, hipStream_t s);
// Prefill-attention variant for hd == 128: pfv 1 = per-wave MFMA kernel,
// >= 2 = LDS-staged kernel with nw (4|8) waves per block, optional split-KV
// (+ combine pass, only when ws != nullptr and S >= split_min_s) or a deep
// schedule (1|2, ignored under split).  hd 256: {pfv 1, nw 4} = the MFMA-256
// kernel, {pfv 0, nw 0} = the plain hd-256 kernel.  Other head dims always
// run the generic kernel.
struct PfVariant {
  int pfv = 2, nw = 8, split = 0, deep = 0, split_min_s = 1024;
};
// the variant the product picks for this shape (env knobs + size policy)
PfVariant attn_prefill_policy(int S, int nh, int hd);
// launch_attn_prefill == launch_attn_prefill_variant(attn_prefill_policy())
void launch_attn_prefill_variant(const u16* qkv, const u16* kc,
                                 const u16* vc, const u16* vtc, u16* out,
                                 float* ws, int S, int pos0, int nh, int nkv,
                                 int hd, int max_seq, int qkv_stride,
                                 int out_stride, int window, PfVariant v,
                                 hipStream_t s);
void launch_rope_simple(u16* x, const float* cost, const float* sint, int bh,
                        int s, int d, hipStream_t st);
void launch_argmax(const float* logits, int n, float* pval, int* pidx,
                   u32* tok, int* pos, u32* ring, int* step, int advance_pos,
                   float inv_temp, uint64_t seed, hipStream_t s);
void launch_advance_pos(int* pos, int by, hipStream_t s);
// On-device top-k / top-p / repeat-penalty sampler (kernels_sample.hip).
// One device allocation of sample_ws_bytes(V), carved by sample_ws_bind;
// hist / state persist across steps and must start zeroed.
constexpr int SAMPLE_HIST_CAP = 1024;  // history ring capacity (power of 2)
constexpr int SAMPLE_MAX_V = 1 << 18;  // block spans and u64 masses fit
struct SampleWs {
  unsigned long long* hmass;  // [6][2048] fixed-point mass histograms
  u32* hcnt;                  // [6][2048] count histograms
  void* sel;                  // selection state entering each pass
  float* work;                // [V] penalised logits (the raw ones stay raw)
  float *pmax, *pmin, *pval;  // [128] per-block partials
  int* pidx;
  u32* hist;   // ring of the last sampled ids
  u32* state;  // {history count, draw counter, kept, tau bits}
};
size_t sample_ws_bytes(int V);
SampleWs sample_ws_bind(void* base, int V);
// penalty (over the last `last_n` history ids) -> top-k -> top-p -> seeded
// Gumbel-argmax at draw index state[1] (inv_temp == 0: argmax), then the
// bookkeeping of launch_argmax; the token joins the history ring when
// advance_hist.  3 launches, +3 per active select.  V <= SAMPLE_MAX_V.
void launch_sample(const float* logits, int V, const SampleWs& b, u32* tok,
                   int* pos, u32* ring, int* step, int advance_pos,
                   float inv_temp, int top_k, float top_p, float penalty,
                   int last_n, int advance_hist, uint64_t seed,
                   hipStream_t s);
// Prefill GEMM variants: the four hand-written kernels and hipBLASLt.
enum {
  GEMM_V128 = 0,      // k_gemm_bf16, 128^2 tile, any K % 8 == 0
  GEMM_V256 = 1,      // k_gemm_256, K % 64 == 0
  GEMM_V128X256 = 2,  // k_gemm_128x256, K % 64 == 0
  GEMM_V256P = 3,     // k_gemm_256p, K % 64 == 0
  GEMM_VLIB = 4,      // hipBLASLt (may reject a shape)
};
struct GemmPolicy {
  bool lib_first;  // try hipBLASLt, fall back to `variant` if it rejects
  int variant;     // the hand-written kernel for this shape
};
// the choice the product makes for this shape (env knobs + size policy)
GemmPolicy gemm_policy(int M, int N, int K);
// runs exactly `variant`; false only when GEMM_VLIB rejects the shape
bool launch_gemm_variant(const u16* A, const u16* W, u16* C, const u16* res,
                         int M, int N, int K, int epi, int variant,
                         hipStream_t s);
// launch_gemm == gemm_policy -> [library ->] launch_gemm_variant
void launch_gemm(const u16* A, const u16* W, u16* C, const u16* res, int M,
                 int N, int K, int epi, hipStream_t s);
// hipBLASLt path for the plain prefill GEMMs (gemm_lib.hip); false => caller
// falls back to the hand-written kernels
bool launch_gemm_lib(const u16* A, const u16* W, u16* C, const u16* res,
                     int M, int N, int K, int epi, hipStream_t s);

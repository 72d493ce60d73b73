// What engine.hip, weights.hip and ops.hip share: the model config, the
// per-projection weight record, the engine itself, and the error / allocation
// helpers.  Host code only.
#pragma once
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <cmath>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../include/cake_hip.h"
#include "kernels.h"

// ---------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------
int set_err(int code, const char* fmt, ...);

#define HIP_TRY(x)                                                      \
  do {                                                                  \
    hipError_t _e = (x);                                                \
    if (_e != hipSuccess)                                               \
      return set_err(2, "%s:%d hip error: %s", __FILE__, __LINE__,      \
                     hipGetErrorString(_e));                            \
  } while (0)

// ---------------------------------------------------------------------------
// model config (mirrors models/common/config.rs:87-153 hot-path subset and
// the config.json auto-detect of cake/mod.rs:82-110,268-274)
// ---------------------------------------------------------------------------
struct ModelConfig {
  int hidden = 0, inter = 0, vocab = 0, layers = 0, nh = 0, nkv = 0;
  int head_dim = 0, max_pos = 4096;
  int window = 0;  // sliding_window tokens, 0 = full attention
                   // (cache.rs:173-205 trims KV to the window; here the
                   // attention span is bounded instead — same semantics)
  int mwl = 0;     // max_window_layers: layers < mwl attend FULL (qwen
                   // rule; HF layer_types condenses to this for the
                   // full-then-sliding pattern); 0 = all layers windowed
  int win_for(int layer_idx) const {
    if (gemma3) return is_local(layer_idx) ? window : 0;
    return (window > 0 && layer_idx >= mwl) ? window : 0;
  }
  // gemma3 (HF Gemma3ForCausalLM): four (1 + w) norms per layer, GELU-tanh
  // gate, embedding times sqrt(H), local (sliding) and global layers in any
  // order, each kind with its own rope table, scores scaled by
  // query_pre_attn_scalar^-0.5.  `local` holds one flag per layer.
  bool gemma3 = false;
  std::vector<char> local;
  bool is_local(int layer_idx) const {
    return layer_idx >= 0 && layer_idx < (int)local.size() && local[layer_idx];
  }
  // rope of the local layers; rope_theta / rope_lin are the global layers'.
  // rope_lin: rope type "linear", inv_freq / factor (1 = unscaled)
  float rope_local_theta = 10000.f, rope_local_lin = 1.f, rope_lin = 1.f;
  float qpas = 0;  // query_pre_attn_scalar; 0 = head_dim
  // the factor folded into the q-norm row so that the kernels' hd^-0.5 scores
  // come out as qpas^-0.5
  float q_fold() const {
    return qpas > 0 && qpas != (float)hd() ? sqrtf((float)hd() / qpas) : 1.f;
  }
  // this config with the local layers' rope in the global fields
  ModelConfig local_rope() const {
    ModelConfig c = *this;
    c.rope_theta = rope_local_theta;
    c.rope_lin = rope_local_lin;
    return c;
  }
  float rms_eps = 1e-5f, rope_theta = 10000.f;
  bool tied = false, qk_norm = false;
  bool qkv_bias = false;  // qwen2: q/k/v projections carry an additive bias
                          // (qwen2/config.rs:84, attention.rs:95-104)
  bool fp8 = false;  // quantization_config.quant_method == "fp8" (fp8.rs:20-40)
  bool w4 = false;   // quant_method == "gptq", bits 4 (gptq.rs:69-86)
  int group = 128;   // gptq group_size; -1 = one group per row
  int grp(int K) const { return group > 0 ? group : K; }
  // llama3 rope scaling (config.rs:50-65)
  bool rope_llama3 = false;
  float rs_factor = 1, rs_low = 1, rs_high = 4;
  float rs_orig = 0;
  // phi3 (Phi-3 / Phi-4): the checkpoint ships self_attn.qkv_proj and
  // mlp.gate_up_proj already fused (phi4/config.rs:88-89)
  bool fused_ckpt = false;
  // partial rotary (phi4/attention.rs:59-66): only the first rd() dims of a
  // head rotate; any model type
  float rotary_factor = 1.f;
  // LongRoPE ("longrope" / "su", HF _compute_longrope_parameters): one divisor
  // per frequency, short or long list by max_seq, and an attention factor on
  // cos and sin.  lr_factor / lr_attn 0 = absent.
  bool rope_long = false;
  std::vector<float> lr_short, lr_long;
  float lr_orig = 0, lr_factor = 0, lr_attn = 0;

  int hd() const { return head_dim ? head_dim : hidden / nh; }
  int rd() const { return (int)((float)hd() * rotary_factor); }
  int sq() const { return nh * hd(); }
  int skv() const { return nkv * hd(); }
  int nqkv() const { return sq() + 2 * skv(); }
};

int parse_config(const char* json, ModelConfig* c);
// gptq shape rules of the 4-bit kernels (engine create and the dispatch
// queries)
int w4_dim_err(const char* name, int N, int K, int g);
int w4_config_err(const ModelConfig& c);

// Full-rotation models without qk-norm and without fp8/4-bit weights take the
// fused rms_norm -> qkv GEMV -> rope -> KV-store kernel (the QK-norm rows
// exist exactly when c.qk_norm; qwen2 takes its biased twin, partial rotary
// the _pr form).  Shared by enqueue_layer_decode and cake_hip_decode_dispatch.
inline bool fused_qkv_rope_applies(const ModelConfig& c) {
  return !c.fp8 && !c.w4 && !c.qk_norm && c.hd() % 4 == 0 &&
         c.nqkv() % 4 == 0 && c.rd() % 4 == 0 && (c.hd() - c.rd()) % 4 == 0;
}

// ---------------------------------------------------------------------------
// one projection's weights: y (N) = W (N, K) x (K).  Alloc, load, random init
// and every launch read format and sizes from here.
// ---------------------------------------------------------------------------
enum WFmt { W_BF16, W_FP8, W_GPTQ };
struct Proj {
  int N = 0, K = 0;  // output rows, input width
  WFmt fmt = W_BF16;
  int g = 0;          // gptq: group size along K (c.grp(K)); else 0
  void* w = nullptr;  // bf16 (N, K) | e4m3fn bytes (N, K), fp8.rs:42-64 |
                      // gptq nibbles, out-major, K/8 words per row
                      // (kernels_w4.hip)
  float* aux = nullptr;  // fp8: blockwise 128x128 scale_inv (N/128, K/128) |
                         // gptq: per row (N, K/g) pairs {s, -(z+1)*s}
  u16* bf16() const { return (u16*)w; }
  unsigned char* fp8() const { return (unsigned char*)w; }
  u32* w4() const { return (u32*)w; }
  size_t elems() const { return (size_t)N * K; }
  size_t w_bytes() const {
    return fmt == W_BF16 ? elems() * 2 : fmt == W_FP8 ? elems() : elems() / 2;
  }
  size_t aux_elems() const {
    return fmt == W_FP8    ? (size_t)(N / 128) * (K / 128)
           : fmt == W_GPTQ ? (size_t)N * (K / g) * 2
                           : 0;
  }
  // algorithmic bytes of one pass over the weights, as the stats book them
  // (gptq counts its pairs, fp8 does not count its scales)
  double bytes() const {
    return (double)w_bytes() + (fmt == W_GPTQ ? aux_elems() * 4.0 : 0.0);
  }
};

struct LayerDev {
  int idx = 0;  // absolute layer index (per-layer attention window)
  u16 *rms1 = nullptr, *rms2 = nullptr;
  // fused q|k|v rows (attention.rs:109-114), o, fused gate|up rows
  // (mlp.rs:38-46), down
  Proj qkv, o, gu, down;
  u16 *qnorm = nullptr, *knorm = nullptr;
  // gemma3: rms2 is pre_feedforward_layernorm; post1 / post2 are
  // post_attention_layernorm / post_feedforward_layernorm, applied to the o
  // and down outputs ahead of the residual add; null otherwise
  u16 *post1 = nullptr, *post2 = nullptr;
  // this layer's rope tables (gemma3 local layers: the local pair)
  const float *cos_t = nullptr, *sin_t = nullptr;
  // qwen2: fused q|k|v projection bias, (Nq) f32 in qkv's row order (f32 so
  // that an F16 bias of a GPTQ checkpoint stays exact); null otherwise
  float* bqkv = nullptr;
  u16 *kc = nullptr, *vc = nullptr;  // (nkv, max_seq, hd) each
  u16 *vtc = nullptr;                // V transposed: (nkv, hd, max_seq)
};

// ---------------------------------------------------------------------------
// stats (per-kernel-family hipEvent timing + algorithmic bytes/flops)
// ---------------------------------------------------------------------------
struct FamStat {
  long launches = 0;
  double ms = 0, bytes = 0, flops = 0;
};
struct PendRec {
  const char* name;
  hipEvent_t e0, e1;
  double bytes, flops;
};
struct Stats {
  bool on = false;
  std::map<std::string, FamStat> fams;
  std::vector<PendRec> pend;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> pool;
  size_t pool_used = 0;
  static const size_t CAP = 32768;
  bool truncated = false;
};

// ---------------------------------------------------------------------------
// engine
// ---------------------------------------------------------------------------
struct cake_engine {
  ModelConfig c;
  int lo = 0, hi = 0;
  int flags = 0, device = 0;
  int max_seq = 0, bt = 0;  // KV capacity, max batch tokens
  bool has_embed() const { return flags & CAKE_HIP_HAS_EMBED; }
  bool has_head() const { return flags & CAKE_HIP_HAS_HEAD; }
  bool use_graph() const { return flags & CAKE_HIP_USE_GRAPH; }

  std::vector<void*> mem;   // every device allocation of this engine (ALLOC)
  std::vector<LayerDev> L;  // size hi-lo
  // lm_head aliases embed for a tied model that holds both
  u16 *embed = nullptr, *norm_w = nullptr, *lm_head = nullptr;
  float *cos_t = nullptr, *sin_t = nullptr;
  float *cos_l = nullptr, *sin_l = nullptr;  // gemma3 local layers' tables

  // workspaces
  u16 *x = nullptr, *xn = nullptr, *qkv = nullptr, *attn_out = nullptr;
  u16 *gu = nullptr, *act = nullptr;
  u16 *wscratch = nullptr;  // fp8/w4 prefill: per-layer dequantized weight
  float* logits = nullptr;
  float* fbuf = nullptr;
  u32* ids = nullptr;
  u32* ring = nullptr;
  static const int RING_CAP = 16384;
  float* pval = nullptr;
  int* pidx = nullptr;
  float* attn_ws = nullptr;
  float* pf_ws = nullptr;  // split-KV prefill partials [nh][bt][2][132]
  u32* attn_cnt = nullptr;
  float* gemv_ws = nullptr;   // split-K GEMV partials [N][2]
  u32* gemv_cnt = nullptr;    // split-K arrival counters (epoch-free)
  int splitk = 0;             // CAKE_GEMV_SPLITK (0 = off)
  int bf16_splitnorm = 0;     // CAKE_BF16_SPLITNORM — measured NEGATIVE on
                              // bf16 (-0.5% 32B, -2% 8B, -9% 0.6B): the bf16
                              // NORM GEMVs already stream at 4.4-6.1 TB/s, so
                              // the extra launch only costs; default off
  int fp8_splitnorm = 1;      // separate rmsnorm kernel ahead of non-NORM
                              // fp8 GEMVs — the fused-norm fp8 path measured
                              // 2.0 TB/s vs 135.5 vs 118.6 tok/s whole-model
                              // (CAKE_FP8_SPLITNORM=0 restores the fusion)
  // fp8 norm chain (kernels.h NormIO): sumsq partials + arrival counters +
  // scales for slot A (pre-qkv rms1, produced by embed/down) and slot B
  // (pre-gateup rms2, produced by the o projection)
  float* nsq_part = nullptr;  // [2][H]
  u32* nsq_cnt = nullptr;     // [2]
  float* nscale = nullptr;    // [2]
  // fp8 norm chain: measured NET NEGATIVE through three iterations
  // (profiles/r02_NOTES.md) — the producer-side election/publish overhead
  // exceeds the two rmsnorm launches it removes.  Default OFF; the code
  // stays env-gated as a documented negative (CAKE_FP8_NORMCHAIN=1).
  int fp8_normchain = 0;
  int* dev_pos = nullptr;
  int* dev_step = nullptr;
  u32* dev_tok = nullptr;
  int host_pos = 0;

  int nchunk = 8;   // split-KV chunks for decode attention (CAKE_NCHUNK)
  float inv_temp = 0.f;        // 0 = greedy ArgMax (text_model.rs:104)
  uint64_t sample_seed = 299792458ull;  // cake default seed (lib.rs:180)
  // top-k / top-p / repeat penalty (cake_hip_set_sampling_ex); all off =
  // the legacy launch_argmax path, untouched
  bool sample_ex = false;
  int top_k = 0, repeat_last_n = 0;
  float top_p = 1.f, repeat_penalty = 1.f;
  void* sample_mem = nullptr;  // backs sws (head engines, vocab permitting)
  SampleWs sws{};
  int gu_rows = 4;  // gate_up channels per block (CAKE_GU_ROWS)

  hipStream_t stream = nullptr;
  hipGraphExec_t graph = nullptr;
  // single-chunk pos-0 prefill graph (see cake_hip_prefill): keyed by the
  // exact token count; first sighting runs eager, second captures
  hipGraphExec_t pf_graph = nullptr;
  int pf_graph_S = -1, pf_seen_S = -1, pf_seen_cnt = 0;
  bool pf_graph_dead = false;
  bool weights_ready = false;

  ncclComm_t comm = nullptr;
  int rank = 0, world = 1;
  // multi-rank prefill comm/compute overlap (north_star: the activation
  // hop overlapped with the next chunk's compute on a second HIP stream)
  hipStream_t comm_stream = nullptr;
  u16* x2 = nullptr;            // second chunk-activation buffer
  hipEvent_t ev_comp[2] = {}, ev_comm[2] = {};
  int prefill_overlap = 1;      // CAKE_PREFILL_OVERLAP=0 restores serial

  Stats st;

  // multi-file (sharded) checkpoint loading state
  bool loading_multi = false;
  std::set<std::string> missing;
  std::set<std::string> loaded;
};

// hipMalloc into `owned`, the list its owner frees in one loop
int dev_alloc(std::vector<void*>& owned, void** p, size_t bytes);
#define ALLOC(owned, ptr, ty, count)                               \
  do {                                                             \
    void* _p = nullptr;                                            \
    int _r = dev_alloc((owned), &_p, sizeof(ty) * (size_t)(count)); \
    if (_r) return _r;                                             \
    (ptr) = (ty*)_p;                                               \
  } while (0)

// GPTQ checkpoint layout -> the device layout of kernels_w4.hip (weights.hip;
// the loader and the w4 op entries both come through here)
void w4_repack(const int32_t* qw, const int32_t* qz, const float* sc, size_t N,
               size_t K, size_t g, u32* W, float* sz);
// argument rules cake_hip_set_sampling_ex and cake_hip_op_sample share
int sampling_args_err(const char* who, float temperature, float top_p,
                      float repeat_penalty);

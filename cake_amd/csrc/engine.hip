// cake_hip engine — MI355X-native host runtime for cake's layer-sharded LLM
// hot path, behind the C-ABI of include/cake_hip.h.
//
// Replaces (from scratch, not a port):
//   - Context::from_args + TextModelBase::load  (cake/mod.rs:114-507,
//     text_model.rs:150-263): config.json parse, safetensors load with
//     per-shard tensor selection, fused QKV / gate_up weights
//     (attention.rs:109-114, mlp.rs:38-46), direct HBM upload as bf16
//   - the generation loop (text_model.rs:266-368,397-495): greedy ArgMax,
//     KV-cached decode with context size 1
//   - the Cache (cache.rs): preallocated device KV cache (no cat-per-token),
//     host-precomputed f32 RoPE tables incl. llama3 scaling (cache.rs:43-99),
//     partial rotary (phi4/attention.rs:59-66) and LongRoPE as HF
//     transformers computes it, with ONE factor list per engine: long_factor
//     if max_seq exceeds original_max_position_embeddings, else short_factor
//     (HF switches per call and drops its cache; build_rope_tables)
//   - the cluster transport (client.rs/worker.rs/proto/message.rs): the
//     per-token activation hop is RCCL ncclSend/ncclRecv over xGMI between
//     adjacent ranks holding contiguous layer ranges
//   - the topology YAML incl. "model.layers.A-B" range expressions
//     (topology.rs:134-169)
//
// The decode step is captured as a hipGraph (single-rank): one replay per
// token, with token id, position and generated-token ring all device-side so
// the graph is replayable (argmax kernel appends to the ring and advances
// the position).
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../include/cake_hip.h"
#include "json.hpp"
#include "kernels.h"

// ---------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------
static thread_local std::string g_err;
static int set_err(int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}
extern "C" const char* cake_hip_last_error(void) { return g_err.c_str(); }

#define HIP_TRY(x)                                                      \
  do {                                                                  \
    hipError_t _e = (x);                                                \
    if (_e != hipSuccess)                                               \
      return set_err(2, "%s:%d hip error: %s", __FILE__, __LINE__,      \
                     hipGetErrorString(_e));                            \
  } while (0)
#define NCCL_TRY(x)                                                     \
  do {                                                                  \
    ncclResult_t _e = (x);                                              \
    if (_e != ncclSuccess)                                              \
      return set_err(3, "%s:%d rccl error: %s", __FILE__, __LINE__,     \
                     ncclGetErrorString(_e));                           \
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
    return (window > 0 && layer_idx >= mwl) ? window : 0;
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

static int parse_config(const char* json, ModelConfig* c) {
  minijson::ValuePtr v;
  try {
    v = minijson::parse(json);
  } catch (const std::exception& e) {
    return set_err(5, "config.json: %s", e.what());
  }
  if (!v || v->kind != minijson::Value::Obj)
    return set_err(5, "config.json: not an object");
  auto geti = [&](const char* k, int d) {
    auto p = v->get(k);
    return p ? (int)p->num_or(d) : d;
  };
  c->hidden = geti("hidden_size", 0);
  c->inter = geti("intermediate_size", 0);
  c->vocab = geti("vocab_size", 0);
  c->layers = geti("num_hidden_layers", 0);
  c->nh = geti("num_attention_heads", 0);
  c->nkv = geti("num_key_value_heads", c->nh);
  c->head_dim = geti("head_dim", 0);
  c->max_pos = geti("max_position_embeddings", 4096);
  if (auto p = v->get("rms_norm_eps")) c->rms_eps = (float)p->num;
  if (auto p = v->get("rope_theta")) c->rope_theta = (float)p->num;
  if (auto p = v->get("tie_word_embeddings")) c->tied = p->bool_or(false);
  if (auto p = v->get("model_type")) {
    c->qk_norm = p->str.find("qwen3") != std::string::npos;
    c->qkv_bias = p->str == "qwen2";
    // qwen2's own default (qwen2/config.rs:7-9)
    if (c->qkv_bias && !v->get("rope_theta")) c->rope_theta = 1e6f;
    // phi3: fused checkpoint tensors; defaults of phi4/config.rs:7-9, 64
    // (num_key_value_heads already defaults to the head count above)
    c->fused_ckpt = p->str == "phi3";
    if (c->fused_ckpt && !v->get("rope_theta")) c->rope_theta = 1e6f;
  }
  // A bias this engine would silently drop is refused: only qwen2's q/k/v
  // bias is implemented (no o-proj or MLP bias, none under QK-norm).
  for (const char* k : {"attention_bias", "mlp_bias"})
    if (auto p = v->get(k))
      if (p->bool_or(false) && !c->qkv_bias)
        return set_err(5, "config.json: %s true is not supported (only the "
                          "q/k/v bias of model_type qwen2 is)", k);
  if (c->qkv_bias && c->qk_norm)
    return set_err(5, "config.json: q/k/v bias together with QK-norm is not "
                      "supported");
  // sliding window (mistral-style; qwen gates it behind use_sliding_window
  // and applies it only from max_window_layers up; HF "layer_types" has
  // the same full-then-sliding shape for these families)
  if (auto p = v->get("sliding_window"))
    if (p->kind == minijson::Value::Num) c->window = (int)p->num;
  if (auto p = v->get("use_sliding_window"))
    if (!p->bool_or(true)) c->window = 0;
  if (auto p = v->get("max_window_layers"))
    if (p->kind == minijson::Value::Num) c->mwl = (int)p->num;
  if (auto lt = v->get("layer_types"))
    if (lt->kind == minijson::Value::Arr) {
      // condense to the full-then-sliding boundary; reject other patterns
      int first_sliding = -1;
      for (size_t i = 0; i < lt->arr.size(); ++i) {
        const bool sl = lt->arr[i]->str == "sliding_attention";
        if (sl && first_sliding < 0) first_sliding = (int)i;
        if (!sl && first_sliding >= 0)
          return set_err(5, "layer_types: only the full-then-sliding "
                            "pattern is supported");
      }
      c->mwl = first_sliding < 0 ? c->layers : first_sliding;
    }
  if (auto qc = v->get("quantization_config"))
    if (auto qm = qc->get("quant_method")) {
      c->fp8 = qm->str == "fp8";
      c->w4 = qm->str == "gptq";
      if (c->w4) {  // AutoGPTQ 4-bit, no act-order (gptq.rs:69-86)
        int bits = 4;
        if (auto p = qc->get("bits")) bits = (int)p->num_or(4);
        if (bits != 4)
          return set_err(5, "gptq: bits %d unsupported (only 4-bit)", bits);
        if (auto p = qc->get("group_size")) c->group = (int)p->num_or(128);
        if (c->group == 0 || c->group < -1)
          return set_err(5, "gptq: group_size %d", c->group);
        if (auto p = qc->get("desc_act"))
          if (p->bool_or(false))
            return set_err(5, "gptq: desc_act true (act-order) is not "
                              "supported");
      }
    }
  if (auto rs = v->get("rope_scaling")) {
    if (rs->kind == minijson::Value::Obj) {
      auto ty = rs->get("rope_type");
      if (!ty) ty = rs->get("type");
      if (ty && ty->str == "llama3") {
        c->rope_llama3 = true;
        if (auto p = rs->get("factor")) c->rs_factor = (float)p->num;
        if (auto p = rs->get("low_freq_factor")) c->rs_low = (float)p->num;
        if (auto p = rs->get("high_freq_factor")) c->rs_high = (float)p->num;
        if (auto p = rs->get("original_max_position_embeddings"))
          c->rs_orig = (float)p->num;
      }
    }
  }
  if (!c->hidden || !c->vocab || !c->layers || !c->nh)
    return set_err(5, "config.json: missing required fields");
  if (c->fused_ckpt && c->fp8)
    return set_err(5, "config.json: quant_method fp8 with model_type phi3 is "
                      "not supported");
  // partial rotary: top-level (the on-disk form) or inside rope_parameters
  auto rp = v->get("rope_parameters");
  if (rp && rp->kind != minijson::Value::Obj) rp = nullptr;
  {
    auto p = v->get("partial_rotary_factor");
    if (!p && rp) p = rp->get("partial_rotary_factor");
    if (p && p->kind == minijson::Value::Num)
      c->rotary_factor = (float)p->num;
  }
  const int hd = c->hd(), rd = c->rd();
  if (rd != hd && (rd <= 0 || rd > hd || rd % 4 != 0 || (hd - rd) % 4 != 0))
    return set_err(5, "config.json: partial_rotary_factor %g gives %d rotary "
                      "dims of head_dim %d; both they and the rest must be "
                      "positive multiples of 4", (double)c->rotary_factor, rd,
                   hd);
  if (rd < hd && (c->qk_norm || c->qkv_bias))
    return set_err(5, "config.json: partial_rotary_factor %g together with "
                      "%s is not supported", (double)c->rotary_factor,
                   c->qk_norm ? "QK-norm" : "the qwen2 q/k/v bias");
  // LongRoPE, under rope_scaling or rope_parameters
  for (auto rs : {v->get("rope_scaling"), rp}) {
    if (!rs || rs->kind != minijson::Value::Obj) continue;
    auto ty = rs->get("rope_type");
    if (!ty) ty = rs->get("type");
    if (!ty || (ty->str != "longrope" && ty->str != "su")) continue;
    c->rope_long = true;
    for (int which = 0; which < 2; ++which) {
      const char* name = which ? "long_factor" : "short_factor";
      std::vector<float>& dst = which ? c->lr_long : c->lr_short;
      dst.clear();
      auto a = rs->get(name);
      if (a && a->kind == minijson::Value::Arr)
        for (auto& x : a->arr) dst.push_back((float)x->num);
      if ((int)dst.size() != rd / 2)
        return set_err(5, "config.json: longrope %s has %d entries, expected "
                          "%d (rotary dims / 2)", name, (int)dst.size(),
                       rd / 2);
    }
    auto om = rs->get("original_max_position_embeddings");
    if (!om) om = v->get("original_max_position_embeddings");
    if (!om || om->kind != minijson::Value::Num || om->num < 2)
      return set_err(5, "config.json: longrope needs "
                        "original_max_position_embeddings");
    c->lr_orig = (float)om->num;
    if (auto p = rs->get("factor"))
      if (p->kind == minijson::Value::Num) c->lr_factor = (float)p->num;
    if (auto p = rs->get("attention_factor"))
      if (p->kind == minijson::Value::Num) c->lr_attn = (float)p->num;
    break;
  }
  return 0;
}

// gptq shape rules of the 4-bit kernels (host only; engine create and the
// dispatch query): a lane's 32-k span must lie in one group, zero points pack
// 8 output columns per word, and the register GEMV covers K <= 32768
static int w4_dim_err(const char* name, int N, int K, int g) {
  if (K < 32 || K > 32768)
    return set_err(5, "gptq: %s in_features %d outside [32, 32768]", name, K);
  if (g < 32 || g % 32 != 0)
    return set_err(5, "gptq: group_size %d (of %s) must be a positive "
                   "multiple of 32", g, name);
  if (K % g != 0)
    return set_err(5, "gptq: %s in_features %d is not a multiple of "
                   "group_size %d", name, K, g);
  if (N < 8 || N % 8 != 0)
    return set_err(5, "gptq: %s out_features %d is not a multiple of 8",
                   name, N);
  return 0;
}
static int w4_config_err(const ModelConfig& c) {
  const int H = c.hidden, I = c.inter, Sq = c.sq(), Skv = c.skv();
  int r;
  if (c.fused_ckpt) {  // phi3: one packed tensor each, repacked whole
    if ((r = w4_dim_err("qkv_proj", c.nqkv(), H, c.grp(H)))) return r;
    if ((r = w4_dim_err("gate_up_proj", 2 * I, H, c.grp(H)))) return r;
    if ((r = w4_dim_err("o_proj", H, Sq, c.grp(Sq)))) return r;
    return w4_dim_err("down_proj", H, I, c.grp(I));
  }
  if ((r = w4_dim_err("q_proj", Sq, H, c.grp(H)))) return r;
  if ((r = w4_dim_err("k_proj/v_proj", Skv, H, c.grp(H)))) return r;
  if ((r = w4_dim_err("o_proj", H, Sq, c.grp(Sq)))) return r;
  if ((r = w4_dim_err("gate_proj/up_proj", I, H, c.grp(H)))) return r;
  if ((r = w4_dim_err("down_proj", H, I, c.grp(I)))) return r;
  return 0;
}

// ---------------------------------------------------------------------------
// RoPE tables (cache.rs:43-99; llama3 scaling 49-80) — host f32, same math
// as oracle/rope_tables
// ---------------------------------------------------------------------------
static void build_rope_tables(const ModelConfig& c, int max_seq,
                              std::vector<float>* cos_t,
                              std::vector<float>* sin_t) {
  int rd = c.rd();  // rotated dims: hd unless partial_rotary_factor < 1
  int half = rd / 2;
  std::vector<float> theta(half);
  for (int i = 0; i < half; ++i)
    theta[i] = 1.0f / powf(c.rope_theta, (float)(2 * i) / (float)rd);
  // LongRoPE (HF _compute_longrope_parameters): inv_freq_i =
  // 1 / (f_i * theta^(2i/rd)) and both tables times the attention factor m.
  // The list is chosen ONCE, by the engine's max_seq: long_factor if max_seq
  // exceeds original_max_position_embeddings, else short_factor.  (HF chooses
  // per forward call by the current length and drops its cache at the
  // crossing; one preallocated cache with one table cannot.)
  float m = 1.f;
  if (c.rope_long) {
    const std::vector<float>& f =
        (float)max_seq > c.lr_orig ? c.lr_long : c.lr_short;
    // in double, rounded once: the f32 exponent 2i/rd alone would cost
    // ln(theta) * 2^-24 relative on the frequency
    for (int i = 0; i < half; ++i)
      theta[i] = (float)(1.0 / ((double)f[i] * pow((double)c.rope_theta,
                                                   2.0 * i / (double)rd)));
    if (c.lr_attn > 0) {
      m = c.lr_attn;
    } else {
      const float s =
          c.lr_factor > 0 ? c.lr_factor : (float)c.max_pos / c.lr_orig;
      m = s <= 1.f ? 1.f : sqrtf(1.f + logf(s) / logf(c.lr_orig));
    }
  }
  if (c.rope_llama3 && c.rs_orig > 0) {
    float low_wl = c.rs_orig / c.rs_low;
    float high_wl = c.rs_orig / c.rs_high;
    for (int i = 0; i < half; ++i) {
      float f = theta[i];
      float wl = 2.0f * (float)M_PI / f;
      if (wl < high_wl) {
      } else if (wl > low_wl) {
        theta[i] = f / c.rs_factor;
      } else {
        float smooth = (c.rs_orig / wl - c.rs_low) / (c.rs_high - c.rs_low);
        theta[i] = (1.0f - smooth) * (f / c.rs_factor) + smooth * f;
      }
    }
  }
  cos_t->resize((size_t)max_seq * half);
  sin_t->resize((size_t)max_seq * half);
  for (int p = 0; p < max_seq; ++p)
    for (int i = 0; i < half; ++i) {
      float a = (float)p * theta[i];
      (*cos_t)[(size_t)p * half + i] = c.rope_long ? m * cosf(a) : cosf(a);
      (*sin_t)[(size_t)p * half + i] = c.rope_long ? m * sinf(a) : sinf(a);
    }
}

// The tables engine create builds for this config and max_seq (host only).
extern "C" int cake_hip_rope_tables(const char* config_json, int max_seq,
                                    float* cosv, float* sinv, int* rd_out) {
  ModelConfig c;
  int r = parse_config(config_json, &c);
  if (r) return r;
  if (max_seq < 32 || max_seq % 32 != 0)
    return set_err(5, "rope_tables: max_seq %d must be a positive multiple of "
                      "32 (engine create rounds up to one)", max_seq);
  std::vector<float> ct, st;
  build_rope_tables(c, max_seq, &ct, &st);
  if (cosv) memcpy(cosv, ct.data(), ct.size() * sizeof(float));
  if (sinv) memcpy(sinv, st.data(), st.size() * sizeof(float));
  if (rd_out) *rd_out = c.rd();
  return 0;
}

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
struct LayerDev {
  int idx = 0;  // absolute layer index (per-layer attention window)
  u16 *rms1 = nullptr, *rms2 = nullptr;
  u16 *wqkv = nullptr, *wo = nullptr, *wgu = nullptr, *wdown = nullptr;
  u16 *qnorm = nullptr, *knorm = nullptr;
  // qwen2: fused q|k|v projection bias, (Nq) f32 in wqkv's row order (f32 so
  // that an F16 bias of a GPTQ checkpoint stays exact); null otherwise
  float* bqkv = nullptr;
  u16 *kc = nullptr, *vc = nullptr;  // (nkv, max_seq, hd) each
  u16 *vtc = nullptr;                // V transposed: (nkv, hd, max_seq)
  // fp8 weights (e4m3fn bytes + blockwise 128x128 scale_inv, fp8.rs:42-64)
  unsigned char *wqkv8 = nullptr, *wo8 = nullptr, *wgu8 = nullptr,
                *wdown8 = nullptr;
  float *sqkv = nullptr, *so8 = nullptr, *sgu = nullptr, *sdown = nullptr;
  // gptq 4-bit weights (kernels_w4.hip layout: out-major packed nibbles,
  // K/8 words per row) + per-row (N, G) f32 pairs {s, -(z+1)*s}
  u32 *wqkv4 = nullptr, *wo4 = nullptr, *wgu4 = nullptr, *wdown4 = nullptr;
  float *zqkv = nullptr, *zo = nullptr, *zgu = nullptr, *zdown = nullptr;
};

struct cake_engine {
  ModelConfig c;
  int lo = 0, hi = 0;
  int flags = 0, device = 0;
  int max_seq = 0, bt = 0;  // KV capacity, max batch tokens
  bool has_embed() const { return flags & CAKE_HIP_HAS_EMBED; }
  bool has_head() const { return flags & CAKE_HIP_HAS_HEAD; }
  bool use_graph() const { return flags & CAKE_HIP_USE_GRAPH; }

  std::vector<LayerDev> L;  // size hi-lo
  u16 *embed = nullptr, *norm_w = nullptr, *lm_head = nullptr;
  float *cos_t = nullptr, *sin_t = nullptr;

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

static int dev_alloc(void** p, size_t bytes) {
  hipError_t e = hipMalloc(p, bytes);
  if (e != hipSuccess)
    return set_err(2, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e));
  return 0;
}
#define ALLOC(ptr, ty, count)                                   \
  do {                                                          \
    void* _p = nullptr;                                         \
    int _r = dev_alloc(&_p, sizeof(ty) * (size_t)(count));      \
    if (_r) return _r;                                          \
    (ptr) = (ty*)_p;                                            \
  } while (0)

// ---- stats helpers --------------------------------------------------------
static hipEvent_t ev_get(cake_engine* e, bool first) {
  Stats& s = e->st;
  if (first) {
    if (s.pool_used < s.pool.size()) return s.pool[s.pool_used].first;
    if (s.pool.size() >= Stats::CAP) return nullptr;
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess) return nullptr;
    if (hipEventCreate(&b) != hipSuccess) return nullptr;
    s.pool.push_back({a, b});
    return a;
  }
  return s.pool[s.pool_used].second;
}
struct StatScope {
  cake_engine* e;
  const char* name;
  double bytes, flops;
  bool active = false;
  StatScope(cake_engine* e_, const char* n, double b, double f)
      : e(e_), name(n), bytes(b), flops(f) {
    if (e->st.on) {
      hipEvent_t ev = ev_get(e, true);
      if (ev) {
        hipEventRecord(ev, e->stream);
        active = true;
      } else {
        e->st.truncated = true;
      }
    }
  }
  ~StatScope() {
    if (active) {
      hipEvent_t ev = ev_get(e, false);
      hipEventRecord(ev, e->stream);
      e->st.pend.push_back({name, e->st.pool[e->st.pool_used].first, ev,
                            bytes, flops});
      e->st.pool_used++;
    }
  }
};
static void stats_flush(cake_engine* e) {
  for (auto& r : e->st.pend) {
    float ms = 0;
    hipEventElapsedTime(&ms, r.e0, r.e1);
    auto& f = e->st.fams[r.name];
    f.launches++;
    f.ms += ms;
    f.bytes += r.bytes;
    f.flops += r.flops;
  }
  e->st.pend.clear();
  e->st.pool_used = 0;
}

// Full-rotation models without qk-norm and without fp8/4-bit weights take the
// fused rms_norm -> qkv GEMV -> rope -> KV-store kernel (the QK-norm rows
// exist exactly when c.qk_norm; qwen2 takes its biased twin, partial rotary
// the _pr form).  Shared with cake_hip_decode_dispatch.
// algorithmic bytes of one packed 4-bit tensor: nibbles + {s, -(z+1)s} pairs
static double w4_bytes(double N, double K, double g) {
  return N * K * 0.5 + N * (K / g) * 8.0;
}
static bool fused_qkv_rope_applies(const ModelConfig& c) {
  return !c.fp8 && !c.w4 && !c.qk_norm && c.hd() % 4 == 0 &&
         c.nqkv() % 4 == 0 && c.rd() % 4 == 0 && (c.hd() - c.rd()) % 4 == 0;
}

// ---------------------------------------------------------------------------
// per-layer decode / prefill enqueue (the Transformer::forward sequence,
// transformer.rs:103-135 + attention.rs:152-357 + mlp.rs:21-31)
// ---------------------------------------------------------------------------
static void enqueue_layer_decode(cake_engine* e, LayerDev& l,
                                 bool have_scale_a = true) {
  const ModelConfig& c = e->c;
  const int H = c.hidden, I = c.inter, hd = c.hd();
  const int Sq = c.sq(), Nq = c.nqkv();
  // Full-rotation models without qk-norm (llama family) take the fused
  // rms_norm -> qkv GEMV -> rope -> KV-store kernel: one launch instead of
  // two, with the rope applied to the dot-product sums in LDS.
  // (CAKE_BF16_SPLITNORM sends a partial-rotary model down the split route,
  // norm + GEMV + store: the A/B leg of k_gemv_qkv_rope_pr.  Full-rotation
  // models keep the fused kernel under it, as before.)
  const bool fused_qkv_rope =
      fused_qkv_rope_applies(c) && !l.qnorm && !l.knorm &&
      !(e->bf16_splitnorm && c.rd() != hd);
  if (fused_qkv_rope) {
    double wb = (double)Nq * H * 2;
    StatScope ss(e, "gemv_qkv", wb + 2.0 * H * 2 + Nq * 2, 2.0 * Nq * H);
    launch_gemv_qkv_rope(l.wqkv, e->x, e->qkv, l.rms1, c.rms_eps, l.kc,
                         l.vc, l.vtc, e->cos_t, e->sin_t, e->dev_pos, c.nh,
                         c.nkv, hd, c.rd(), e->max_seq, H, e->stream, l.bqkv);
  } else if (c.w4) {  // split norm -> 4-bit GEMV -> rope + KV store
    {
      StatScope ss(e, "rmsnorm", 2.0 * H * 2, 0);
      launch_rmsnorm(e->x, l.rms1, e->xn, 1, H, c.rms_eps, e->stream);
    }
    {
      StatScope ss(e, "gemv_w4", w4_bytes(Nq, H, c.grp(H)) + H * 2 + Nq * 2,
                   2.0 * Nq * H);
      launch_gemv_w4(l.wqkv4, l.zqkv, e->xn, e->qkv, nullptr, Nq, H,
                     c.grp(H), 0, e->stream);
    }
    StatScope ss(e, "rope_store", 0, 0);
    launch_rope_store_decode(e->qkv, l.kc, l.vc, l.vtc, e->cos_t, e->sin_t,
                             e->dev_pos, c.nh, c.nkv, hd, c.rd(), e->max_seq,
                             l.qnorm, l.knorm, c.rms_eps, e->stream, l.bqkv);
  } else {
    {  // rms_1 fused into the qkv projection (GEMV, x kept in registers)
      double wb = (double)Nq * H * (c.fp8 ? 1 : 2);
      StatScope ss(e, "gemv_qkv", wb + 2.0 * H * 2 + Nq * 2, 2.0 * Nq * H);
      if (c.fp8) {
        if (e->fp8_normchain && have_scale_a) {
          // norm chain: rms1 scale precomputed by the previous layer's
          // down projection (or embed for layer 0) — no norm launch
          NormIO nio{e->nscale + 0, l.rms1, nullptr, nullptr, nullptr, 0.f};
          launch_gemv_fp8(l.wqkv8, l.sqkv, e->x, e->qkv, nullptr, nullptr,
                          0.f, Nq, H, 0, e->stream, nio);
        } else if (e->fp8_splitnorm) {
          launch_rmsnorm(e->x, l.rms1, e->xn, 1, H, c.rms_eps, e->stream);
          launch_gemv_fp8(l.wqkv8, l.sqkv, e->xn, e->qkv, nullptr, nullptr,
                          0.f, Nq, H, 0, e->stream);
        } else {
          launch_gemv_fp8(l.wqkv8, l.sqkv, e->x, e->qkv, nullptr, l.rms1,
                          c.rms_eps, Nq, H, 0, e->stream);
        }
      }
      else if (e->bf16_splitnorm) {
        launch_rmsnorm(e->x, l.rms1, e->xn, 1, H, c.rms_eps, e->stream);
        launch_gemv(l.wqkv, e->xn, e->qkv, nullptr, nullptr, 0.f, Nq, H, 0,
                    e->stream);
      } else
        launch_gemv(l.wqkv, e->x, e->qkv, nullptr, l.rms1, c.rms_eps, Nq, H,
                    0, e->stream);
    }
    {  // [Qwen3 QK-norm, attention.rs:202-215 | qwen2 bias, fused +] rope +
       // KV store
      StatScope ss(e, "rope_store", (double)Nq * hd * 0, 0);
      launch_rope_store_decode(e->qkv, l.kc, l.vc, l.vtc, e->cos_t, e->sin_t,
                               e->dev_pos, c.nh, c.nkv, hd, c.rd(), e->max_seq,
                               l.qnorm, l.knorm, c.rms_eps, e->stream,
                               l.bqkv);
    }
  }
  {  // decode attention over the cache (single launch, split-KV combine)
    double kvbytes = 2.0 * (e->host_pos + 1) * c.skv() * 2;
    StatScope ss(e, "attn_decode", kvbytes + Sq * 2 * 2,
                 4.0 * (e->host_pos + 1) * Sq);
    launch_attn_decode(e->qkv, l.kc, l.vc, e->dev_pos, e->attn_ws,
                       e->attn_cnt, e->attn_out, c.nh, c.nkv, hd, e->max_seq,
                       e->nchunk, c.win_for(l.idx), e->stream);
  }
  if (c.w4) {  // o projection + residual (aliased)
    StatScope ss(e, "gemv_w4", w4_bytes(H, Sq, c.grp(Sq)) + Sq * 2 + H * 4,
                 2.0 * H * Sq);
    launch_gemv_w4(l.wo4, l.zo, e->attn_out, e->x, e->x, H, Sq, c.grp(Sq), 1,
                   e->stream);
  } else {  // o projection + residual
    double wb = (double)H * Sq * (c.fp8 ? 1 : 2);
    StatScope ss(e, "gemv_o", wb + Sq * 2 + H * 4, 2.0 * H * Sq);
    if (c.fp8) {
      NormIO nio{};
      if (e->fp8_normchain) {
        nio.part = e->nsq_part + H;
        nio.cnt = e->nsq_cnt + 16;
        nio.scale_out = e->nscale + 1;
        nio.eps = c.rms_eps;
      }
      launch_gemv_fp8(l.wo8, l.so8, e->attn_out, e->x, e->x, nullptr, 0.f,
                      H, Sq, 1, e->stream, nio);
    }
    else if (e->splitk == 2 && Sq % 16 == 0)
      launch_gemv_res_splitk(l.wo, e->attn_out, e->x, e->x, e->gemv_ws,
                             e->gemv_cnt, H, Sq, e->stream);
    else
      launch_gemv(l.wo, e->attn_out, e->x, e->x, nullptr, 0.f, H, Sq, 1,
                  e->stream);
  }
  if (c.w4) {  // split norm, gate_up GEMV + silu_mul, down + residual
    {
      StatScope ss(e, "rmsnorm", 2.0 * H * 2, 0);
      launch_rmsnorm(e->x, l.rms2, e->xn, 1, H, c.rms_eps, e->stream);
    }
    {
      StatScope ss(e, "gemv_gateup_w4",
                   w4_bytes(2 * I, H, c.grp(H)) + H * 2 + I * 2, 4.0 * I * H);
      launch_gemv_gateup_w4(l.wgu4, l.zgu, e->xn, e->act, I, H, c.grp(H),
                            e->stream);
    }
    StatScope ss(e, "gemv_w4", w4_bytes(H, I, c.grp(I)) + I * 2 + H * 4,
                 2.0 * H * I);
    launch_gemv_w4(l.wdown4, l.zdown, e->act, e->x, e->x, H, I, c.grp(I), 1,
                   e->stream);
    return;
  }
  {  // rms_2 fused into gate_up GEMV + silu_mul (mlp.rs:21-31)
    double wb = 2.0 * I * H * (c.fp8 ? 1 : 2);
    StatScope ss(e, "gemv_gateup", wb + 2.0 * H * 2 + I * 2, 4.0 * I * H);
    if (c.fp8) {
      if (e->fp8_normchain) {
        NormIO nio{e->nscale + 1, l.rms2, nullptr, nullptr, nullptr, 0.f};
        launch_gemv_gateup_fp8(l.wgu8, l.sgu, e->x, e->act, nullptr, 0.f,
                               I, H, e->stream, nio);
      } else if (e->fp8_splitnorm) {
        launch_rmsnorm(e->x, l.rms2, e->xn, 1, H, c.rms_eps, e->stream);
        launch_gemv_gateup_fp8(l.wgu8, l.sgu, e->xn, e->act, nullptr, 0.f,
                               I, H, e->stream);
      } else {
        launch_gemv_gateup_fp8(l.wgu8, l.sgu, e->x, e->act, l.rms2,
                               c.rms_eps, I, H, e->stream);
      }
    }
    else if (e->bf16_splitnorm) {
      launch_rmsnorm(e->x, l.rms2, e->xn, 1, H, c.rms_eps, e->stream);
      launch_gemv_gateup(l.wgu, e->xn, e->act, nullptr, 0.f, I, H,
                         e->gu_rows, e->stream);
    } else
      launch_gemv_gateup(l.wgu, e->x, e->act, l.rms2, c.rms_eps, I, H,
                         e->gu_rows, e->stream);
  }
  {  // down projection + residual
    double wb = (double)H * I * (c.fp8 ? 1 : 2);
    StatScope ss(e, "gemv_down", wb + I * 2 + H * 4, 2.0 * H * I);
    if (c.fp8) {
      NormIO nio{};
      if (e->fp8_normchain) {
        nio.part = e->nsq_part;
        nio.cnt = e->nsq_cnt;
        nio.scale_out = e->nscale;
        nio.eps = c.rms_eps;
      }
      launch_gemv_fp8(l.wdown8, l.sdown, e->act, e->x, e->x, nullptr, 0.f,
                      H, I, 1, e->stream, nio);
    }
    else if (e->splitk == 2 && I % 16 == 0)
      launch_gemv_res_splitk(l.wdown, e->act, e->x, e->x, e->gemv_ws,
                             e->gemv_cnt, H, I, e->stream);
    else
      launch_gemv(l.wdown, e->act, e->x, e->x, nullptr, 0.f, H, I, 1,
                  e->stream);
  }
}

static void enqueue_layer_prefill(cake_engine* e, LayerDev& l, int S,
                                  int pos0, u16* x = nullptr) {
  const ModelConfig& c = e->c;
  const int H = c.hidden, I = c.inter, hd = c.hd();
  const int Sq = c.sq(), Nq = c.nqkv();
  if (!x) x = e->x;
  {
    StatScope ss(e, "rmsnorm_pf", 2.0 * S * H * 2, 0);
    launch_rmsnorm(x, l.rms1, e->xn, S, H, c.rms_eps, e->stream);
  }
  const u16* wqkv = l.wqkv;
  const u16* wo = l.wo;
  const u16* wgu = l.wgu;
  const u16* wdown = l.wdown;
  if (c.fp8) {  // dequant into the shared scratch right before each GEMM
    StatScope ss(e, "dequant_fp8", (double)Nq * H * 3, 0);
    launch_dequant_fp8(l.wqkv8, l.sqkv, e->wscratch, Nq, H, e->stream);
    wqkv = e->wscratch;
  } else if (c.w4) {
    StatScope ss(e, "dequant_w4",
                 w4_bytes(Nq, H, c.grp(H)) + (double)Nq * H * 2, 0);
    launch_dequant_w4(l.wqkv4, l.zqkv, e->wscratch, Nq, H, c.grp(H),
                      e->stream);
    wqkv = e->wscratch;
  }
  {
    StatScope ss(e, "gemm_qkv", (double)Nq * H * 2 + (double)S * (H + Nq) * 2,
                 2.0 * S * Nq * H);
    launch_gemm(e->xn, wqkv, e->qkv, nullptr, S, Nq, H, 0, e->stream);
  }
  {  // [fused QK-norm | qkv bias +] rope + KV store for all S positions
    StatScope ss(e, "rope_store_pf", 0, 0);
    launch_rope_store_prefill(e->qkv, l.kc, l.vc, l.vtc, e->cos_t, e->sin_t,
                              pos0, S, c.nh, c.nkv, hd, c.rd(), e->max_seq,
                              Nq, l.qnorm, l.knorm, c.rms_eps, e->stream,
                              l.bqkv);
  }
  {
    double n_avg = pos0 + (S + 1) * 0.5;
    StatScope ss(e, "attn_prefill", 2.0 * S * n_avg * 2 * hd * c.nh / 4,
                 4.0 * S * n_avg * hd * c.nh);
    launch_attn_prefill(e->qkv, l.kc, l.vc, l.vtc, e->attn_out, e->pf_ws, S,
                        pos0, c.nh, c.nkv, hd, e->max_seq, Nq, Sq,
                        c.win_for(l.idx), e->stream);
  }
  if (c.fp8) {
    StatScope ss(e, "dequant_fp8", (double)H * Sq * 3, 0);
    launch_dequant_fp8(l.wo8, l.so8, e->wscratch, H, Sq, e->stream);
    wo = e->wscratch;
  } else if (c.w4) {
    StatScope ss(e, "dequant_w4",
                 w4_bytes(H, Sq, c.grp(Sq)) + (double)H * Sq * 2, 0);
    launch_dequant_w4(l.wo4, l.zo, e->wscratch, H, Sq, c.grp(Sq), e->stream);
    wo = e->wscratch;
  }
  {
    StatScope ss(e, "gemm_o", (double)H * Sq * 2 + (double)S * (Sq + H) * 2,
                 2.0 * S * H * Sq);
    launch_gemm(e->attn_out, wo, x, x, S, H, Sq, 1, e->stream);
  }
  {
    StatScope ss(e, "rmsnorm_pf", 2.0 * S * H * 2, 0);
    launch_rmsnorm(x, l.rms2, e->xn, S, H, c.rms_eps, e->stream);
  }
  if (c.fp8) {
    StatScope ss(e, "dequant_fp8", 2.0 * I * H * 3, 0);
    launch_dequant_fp8(l.wgu8, l.sgu, e->wscratch, 2 * I, H, e->stream);
    wgu = e->wscratch;
  } else if (c.w4) {
    StatScope ss(e, "dequant_w4",
                 w4_bytes(2 * I, H, c.grp(H)) + 2.0 * I * H * 2, 0);
    launch_dequant_w4(l.wgu4, l.zgu, e->wscratch, 2 * I, H, c.grp(H),
                      e->stream);
    wgu = e->wscratch;
  }
  {
    StatScope ss(e, "gemm_gateup",
                 2.0 * I * H * 2 + (double)S * (H + 2.0 * I) * 2,
                 4.0 * S * I * H);
    launch_gemm(e->xn, wgu, e->gu, nullptr, S, 2 * I, H, 0, e->stream);
  }
  {
    StatScope ss(e, "silu_mul", 3.0 * S * I * 2, 0);
    launch_silu_mul_rows(e->gu, e->act, S, I, e->stream);
  }
  if (c.fp8) {
    StatScope ss(e, "dequant_fp8", (double)H * I * 3, 0);
    launch_dequant_fp8(l.wdown8, l.sdown, e->wscratch, H, I, e->stream);
    wdown = e->wscratch;
  } else if (c.w4) {
    StatScope ss(e, "dequant_w4",
                 w4_bytes(H, I, c.grp(I)) + (double)H * I * 2, 0);
    launch_dequant_w4(l.wdown4, l.zdown, e->wscratch, H, I, c.grp(I),
                      e->stream);
    wdown = e->wscratch;
  }
  {
    StatScope ss(e, "gemm_down", (double)H * I * 2 + (double)S * (I + H) * 2,
                 2.0 * S * H * I);
    launch_gemm(e->act, wdown, x, x, S, H, I, 1, e->stream);
  }
}

static void enqueue_head_sample(cake_engine* e, int S, int advance_by,
                                u16* x = nullptr) {
  const ModelConfig& c = e->c;
  const int H = c.hidden, V = c.vocab;
  if (!x) x = e->x;
  {  // final norm on the last token (text_model.rs:336-346) fused into
     // the lm_head GEMV (f32 logits)
    StatScope ss(e, "gemv_head", (double)V * H * 2 + H * 2 + V * 4,
                 2.0 * V * H);
    launch_gemv(e->lm_head, x + (size_t)(S - 1) * H, e->logits, nullptr,
                e->norm_w, c.rms_eps, V, H, 2, e->stream);
  }
  if (advance_by > 1)
    launch_advance_pos(e->dev_pos, advance_by - 1, e->stream);
  if (e->sample_ex) {  // penalty -> top-k -> top-p -> Gumbel-argmax, with
                       // the same bookkeeping (text_model.rs:102-118,433-452)
    StatScope ss(e, "sample", (double)V * 4 * 3, 0);
    launch_sample(e->logits, V, e->sws, e->dev_tok, e->dev_pos, e->ring,
                  e->dev_step, 1, e->inv_temp, e->top_k, e->top_p,
                  e->repeat_penalty, e->repeat_last_n, 1, e->sample_seed,
                  e->stream);
  } else {  // greedy ArgMax / Gumbel sampling + ring append + pos++
            // (text_model.rs:102-118)
    StatScope ss(e, "argmax", (double)V * 4, 0);
    launch_argmax(e->logits, V, e->pval, e->pidx, e->dev_tok, e->dev_pos,
                  e->ring, e->dev_step, 1, e->inv_temp, e->sample_seed,
                  e->stream);
  }
}

// one full decode step on this rank (graph-capturable when world == 1)
static int enqueue_decode_step(cake_engine* e) {
  const ModelConfig& c = e->c;
  const int H = c.hidden;
  float* nsc = (e->c.fp8 && e->fp8_normchain) ? e->nscale : nullptr;
  if (e->world == 1) {
    launch_embed_token(e->embed, e->dev_tok, e->x, H, e->stream, nsc,
                       e->c.rms_eps);
    for (auto& l : e->L) enqueue_layer_decode(e, l);
    enqueue_head_sample(e, 1, 1);
    return 0;
  }
  if (e->rank == 0) {
    launch_embed_token(e->embed, e->dev_tok, e->x, H, e->stream, nsc,
                       e->c.rms_eps);
    for (auto& l : e->L) enqueue_layer_decode(e, l);
    NCCL_TRY(ncclSend(e->x, H, ncclBfloat16, 1, e->comm, e->stream));
    NCCL_TRY(ncclRecv(e->x, H, ncclBfloat16, e->world - 1, e->comm,
                      e->stream));
    enqueue_head_sample(e, 1, 1);
  } else {
    NCCL_TRY(ncclRecv(e->x, H, ncclBfloat16, e->rank - 1, e->comm,
                      e->stream));
    // rank > 0: the first layer's x arrives over RCCL with no producing
    // kernel, so its rms1 falls back to the split-norm launch
    for (size_t li = 0; li < e->L.size(); ++li)
      enqueue_layer_decode(e, e->L[li], li > 0);
    NCCL_TRY(ncclSend(e->x, H, ncclBfloat16, (e->rank + 1) % e->world,
                      e->comm, e->stream));
    launch_advance_pos(e->dev_pos, 1, e->stream);
  }
  return 0;
}

// ---------------------------------------------------------------------------
// C-ABI: lifecycle
// ---------------------------------------------------------------------------
extern "C" int cake_hip_engine_create(const char* config_json, int layer_lo,
                                      int layer_hi, int flags, int max_seq,
                                      int max_batch_tokens, int device,
                                      cake_engine** out) {
  ModelConfig c;
  int r = parse_config(config_json, &c);
  if (r) return r;
  if (layer_lo < 0 || layer_hi > c.layers || layer_lo >= layer_hi)
    return set_err(5, "bad layer range [%d,%d) of %d", layer_lo, layer_hi,
                   c.layers);
  if (c.hd() > 128 || c.hd() % 8 != 0)
    return set_err(5, "head_dim %d unsupported (must be <=128, mult of 8)",
                   c.hd());
  if (c.hidden > 16384)
    return set_err(5, "hidden_size %d unsupported (> 16384)", c.hidden);
  if (c.hidden % 8 || c.inter % 8)
    return set_err(5, "hidden/intermediate must be multiples of 8");
  if (c.w4 && (r = w4_config_err(c))) return r;
  if (max_seq <= 0) max_seq = c.max_pos;
  max_seq = (max_seq + 31) & ~31;  // MFMA prefill reads whole 32-pos tiles
  if (max_batch_tokens <= 0) max_batch_tokens = 2048;
  if (max_batch_tokens > max_seq) max_batch_tokens = max_seq;

  HIP_TRY(hipSetDevice(device));
  auto* e = new cake_engine();
  e->c = c;
  e->lo = layer_lo;
  e->hi = layer_hi;
  e->flags = flags;
  e->device = device;
  e->max_seq = max_seq;
  e->bt = max_batch_tokens;
  HIP_TRY(hipStreamCreate(&e->stream));

  const int H = c.hidden, I = c.inter, V = c.vocab;
  const int hd = c.hd(), Nq = c.nqkv(), Sq = c.sq();
  const int BT = e->bt;
  // weights
  if (c.fp8 && (H % 128 || I % 128 || Sq % 128 || c.skv() % 128))
    return set_err(5, "fp8 requires dims to be multiples of 128");
  e->L.resize(layer_hi - layer_lo);
  for (size_t li = 0; li < e->L.size(); ++li)
    e->L[li].idx = layer_lo + (int)li;
  for (auto& l : e->L) {
    ALLOC(l.rms1, u16, H);
    ALLOC(l.rms2, u16, H);
    if (c.fp8) {
      ALLOC(l.wqkv8, unsigned char, (size_t)Nq * H);
      ALLOC(l.wo8, unsigned char, (size_t)H * Sq);
      ALLOC(l.wgu8, unsigned char, (size_t)2 * I * H);
      ALLOC(l.wdown8, unsigned char, (size_t)H * I);
      ALLOC(l.sqkv, float, (size_t)(Nq / 128) * (H / 128));
      ALLOC(l.so8, float, (size_t)(H / 128) * (Sq / 128));
      ALLOC(l.sgu, float, (size_t)(2 * I / 128) * (H / 128));
      ALLOC(l.sdown, float, (size_t)(H / 128) * (I / 128));
    } else if (c.w4) {
      const size_t GH = H / c.grp(H), GS = Sq / c.grp(Sq), GI = I / c.grp(I);
      ALLOC(l.wqkv4, u32, (size_t)Nq * H / 8);
      ALLOC(l.wo4, u32, (size_t)H * Sq / 8);
      ALLOC(l.wgu4, u32, (size_t)2 * I * H / 8);
      ALLOC(l.wdown4, u32, (size_t)H * I / 8);
      ALLOC(l.zqkv, float, (size_t)Nq * GH * 2);
      ALLOC(l.zo, float, (size_t)H * GS * 2);
      ALLOC(l.zgu, float, (size_t)2 * I * GH * 2);
      ALLOC(l.zdown, float, (size_t)H * GI * 2);
    } else {
      ALLOC(l.wqkv, u16, (size_t)Nq * H);
      ALLOC(l.wo, u16, (size_t)H * Sq);
      ALLOC(l.wgu, u16, (size_t)2 * I * H);
      ALLOC(l.wdown, u16, (size_t)H * I);
    }
    if (c.qk_norm) {
      ALLOC(l.qnorm, u16, hd);
      ALLOC(l.knorm, u16, hd);
    }
    if (c.qkv_bias) ALLOC(l.bqkv, float, Nq);
    ALLOC(l.kc, u16, (size_t)c.nkv * max_seq * hd);
    ALLOC(l.vc, u16, (size_t)c.nkv * max_seq * hd);
    ALLOC(l.vtc, u16, (size_t)c.nkv * hd * max_seq);
    // zero the caches: positions >= n are masked (weight 0) but 0*NaN from
    // allocator garbage would still poison the PV MFMA
    HIP_TRY(hipMemset(l.kc, 0, (size_t)c.nkv * max_seq * hd * 2));
    HIP_TRY(hipMemset(l.vc, 0, (size_t)c.nkv * max_seq * hd * 2));
    HIP_TRY(hipMemset(l.vtc, 0, (size_t)c.nkv * hd * max_seq * 2));
  }
  if (e->has_embed()) ALLOC(e->embed, u16, (size_t)V * H);
  if (e->has_head()) {
    ALLOC(e->norm_w, u16, H);
    if (c.tied && e->has_embed())
      e->lm_head = e->embed;
    else
      ALLOC(e->lm_head, u16, (size_t)V * H);
  }
  // rope tables
  {
    std::vector<float> ct, st;
    build_rope_tables(c, max_seq, &ct, &st);
    ALLOC(e->cos_t, float, ct.size());
    ALLOC(e->sin_t, float, st.size());
    HIP_TRY(hipMemcpy(e->cos_t, ct.data(), ct.size() * 4,
                      hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->sin_t, st.data(), st.size() * 4,
                      hipMemcpyHostToDevice));
  }
  // workspaces
  ALLOC(e->x, u16, (size_t)BT * H);
  ALLOC(e->x2, u16, (size_t)BT * H);
  HIP_TRY(hipStreamCreate(&e->comm_stream));
  for (int i = 0; i < 2; ++i) {
    HIP_TRY(hipEventCreateWithFlags(&e->ev_comp[i], hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&e->ev_comm[i], hipEventDisableTiming));
  }
  if (const char* ov = getenv("CAKE_PREFILL_OVERLAP"))
    e->prefill_overlap = atoi(ov);
  ALLOC(e->xn, u16, (size_t)BT * H);
  ALLOC(e->qkv, u16, (size_t)BT * Nq);
  ALLOC(e->attn_out, u16, (size_t)BT * Sq);
  ALLOC(e->gu, u16, (size_t)BT * 2 * I);
  ALLOC(e->act, u16, (size_t)BT * I);
  if (c.fp8 || c.w4) {
    size_t mx = std::max((size_t)Nq * H,
                         std::max((size_t)H * Sq,
                                  std::max((size_t)2 * I * H,
                                           (size_t)H * I)));
    ALLOC(e->wscratch, u16, mx);
  }
  ALLOC(e->logits, float, V);
  ALLOC(e->fbuf, float, (size_t)BT * H);
  ALLOC(e->ids, u32, BT);
  ALLOC(e->ring, u32, cake_engine::RING_CAP);
  ALLOC(e->pval, float, 256);
  ALLOC(e->pidx, int, 256);
  if (e->has_head() && V >= 1 && V <= SAMPLE_MAX_V) {
    const size_t sb = sample_ws_bytes(V);
    ALLOC(e->sample_mem, char, sb);
    HIP_TRY(hipMemset(e->sample_mem, 0, sb));
    e->sws = sample_ws_bind(e->sample_mem, V);
  }
  if (const char* nc = getenv("CAKE_NCHUNK")) {
    int v = atoi(nc);
    if (v >= 1 && v <= 64) e->nchunk = v;
  }
  e->gu_rows = gemv_gateup_rows_policy();  // CAKE_GU_ROWS
  ALLOC(e->attn_ws, float, (size_t)c.nh * 64 * (hd + 4));  // nchunk <= 64; row stride 132 f32 = 16B-aligned
  if (hd == 128 && e->bt >= 1024)  // split-KV prefill partials
    ALLOC(e->pf_ws, float, (size_t)c.nh * e->bt * 2 * 132);
  ALLOC(e->attn_cnt, u32, c.nh);
  HIP_TRY(hipMemset(e->attn_cnt, 0, sizeof(u32) * c.nh));
  if (const char* sk = getenv("CAKE_GEMV_SPLITK"))
    e->splitk = atoi(sk);
  if (const char* sn = getenv("CAKE_FP8_SPLITNORM"))
    e->fp8_splitnorm = atoi(sn);
  if (const char* sn = getenv("CAKE_BF16_SPLITNORM"))
    e->bf16_splitnorm = atoi(sn);
  if (const char* ncv = getenv("CAKE_FP8_NORMCHAIN"))
    e->fp8_normchain = atoi(ncv);
  if (c.fp8) {
    ALLOC(e->nsq_part, float, (size_t)2 * H);
    ALLOC(e->nsq_cnt, u32, 2 * 16);  // 8 residue shards + top, per slot
    ALLOC(e->nscale, float, 2);
    HIP_TRY(hipMemset(e->nsq_cnt, 0, 2 * 16 * sizeof(u32)));
    HIP_TRY(hipMemset(e->nscale, 0, 2 * sizeof(float)));
  }
  {
    const size_t mx = (size_t)std::max(H, I);
    ALLOC(e->gemv_ws, float, mx * 2);
    ALLOC(e->gemv_cnt, u32, (mx + 1) / 2);
    HIP_TRY(hipMemset(e->gemv_cnt, 0, sizeof(u32) * ((mx + 1) / 2)));
  }
  ALLOC(e->dev_pos, int, 1);
  ALLOC(e->dev_step, int, 1);
  ALLOC(e->dev_tok, u32, 1);
  HIP_TRY(hipMemset(e->dev_pos, 0, 4));
  HIP_TRY(hipMemset(e->dev_step, 0, 4));
  HIP_TRY(hipMemset(e->dev_tok, 0, 4));
  *out = e;
  return 0;
}

extern "C" void cake_hip_engine_free(cake_engine* e) {
  if (!e) return;
  hipSetDevice(e->device);
  hipDeviceSynchronize();
  if (e->graph) hipGraphExecDestroy(e->graph);
  if (e->pf_graph) hipGraphExecDestroy(e->pf_graph);
  if (e->comm) ncclCommDestroy(e->comm);
  // (device allocations are freed with the process; engines live for the
  // process lifetime in the intended use — still free the big ones)
  for (auto& l : e->L) {
    hipFree(l.rms1); hipFree(l.rms2); hipFree(l.wqkv); hipFree(l.wo);
    hipFree(l.wgu); hipFree(l.wdown); hipFree(l.kc); hipFree(l.vc);
    hipFree(l.vtc);
    if (l.wqkv8) {
      hipFree(l.wqkv8); hipFree(l.wo8); hipFree(l.wgu8); hipFree(l.wdown8);
      hipFree(l.sqkv); hipFree(l.so8); hipFree(l.sgu); hipFree(l.sdown);
    }
    if (l.wqkv4) {
      hipFree(l.wqkv4); hipFree(l.wo4); hipFree(l.wgu4); hipFree(l.wdown4);
      hipFree(l.zqkv); hipFree(l.zo); hipFree(l.zgu); hipFree(l.zdown);
    }
    if (l.qnorm) { hipFree(l.qnorm); hipFree(l.knorm); }
    if (l.bqkv) hipFree(l.bqkv);
  }
  if (e->embed) hipFree(e->embed);
  if (e->lm_head && e->lm_head != e->embed) hipFree(e->lm_head);
  if (e->norm_w) hipFree(e->norm_w);
  hipFree(e->x); hipFree(e->xn); hipFree(e->qkv); hipFree(e->attn_out);
  hipFree(e->gu); hipFree(e->act); hipFree(e->logits); hipFree(e->fbuf);
  if (e->wscratch) hipFree(e->wscratch);
  hipFree(e->ids); hipFree(e->ring); hipFree(e->pval); hipFree(e->pidx);
  if (e->sample_mem) hipFree(e->sample_mem);
  hipFree(e->attn_ws); hipFree(e->pf_ws); hipFree(e->attn_cnt);
  hipFree(e->gemv_ws); hipFree(e->gemv_cnt);
  if (e->nsq_part) { hipFree(e->nsq_part); hipFree(e->nsq_cnt);
                     hipFree(e->nscale); }
  hipFree(e->dev_pos); hipFree(e->dev_step);
  hipFree(e->dev_tok); hipFree(e->cos_t); hipFree(e->sin_t);
  hipFree(e->x2);
  for (int i = 0; i < 2; ++i) {
    if (e->ev_comp[i]) hipEventDestroy(e->ev_comp[i]);
    if (e->ev_comm[i]) hipEventDestroy(e->ev_comm[i]);
  }
  if (e->comm_stream) hipStreamDestroy(e->comm_stream);
  hipStreamDestroy(e->stream);
  delete e;
}

// ---------------------------------------------------------------------------
// weight loading
// ---------------------------------------------------------------------------
struct StTensor {
  std::string dtype;
  std::vector<long> shape;
  size_t off0 = 0, off1 = 0;
};

static inline float b2f_host(u16 h) {
  union { u32 u; float f; } v{(u32)h << 16};
  return v.f;
}
// element i of an IEEE half array (possibly unaligned) as f32, exactly
static inline float f16_at(const char* src, size_t i) {
  _Float16 h;
  memcpy(&h, src + i * 2, 2);
  return (float)h;
}

// GPTQ checkpoint layout -> the device layout of kernels_w4.hip, for one
// projection (the loader and the w4 op entries both come through here).
//   qw (K/8, N) i32: nibble b of word [r, j] is q(k = 8r + b, j)
//   qz (G, N/8) i32: nibble j % 8 of word [gi, j / 8] is z(gi, j)
//   sc (G, N)   f32 (f16-representable)
// -> W (N, K/8): row j contiguous over k, same nibble order inside a word;
//    sz (N, G, 2) = {s, -(z+1)*s}: z + 1 may be 16 and does not wrap, words
//    are read as unsigned so the top nibble is (w >> 28) & 0xF.
static void w4_repack(const int32_t* qw, const int32_t* qz, const float* sc,
                      size_t N, size_t K, size_t g, u32* W, float* sz) {
  const size_t K8 = K / 8, G = K / g, N8 = N / 8;
  const size_t T = 32;  // transpose in tiles: both sides stay in cache
  for (size_t r0 = 0; r0 < K8; r0 += T)
    for (size_t j0 = 0; j0 < N; j0 += T)
      for (size_t r = r0; r < std::min(K8, r0 + T); ++r)
        for (size_t j = j0; j < std::min(N, j0 + T); ++j)
          W[j * K8 + r] = (u32)qw[r * N + j];
  for (size_t gi = 0; gi < G; ++gi)
    for (size_t j = 0; j < N; ++j) {
      const u32 z = ((u32)qz[gi * N8 + j / 8] >> (4 * (j % 8))) & 0xFu;
      const float s = sc[gi * N + j];
      sz[(j * G + gi) * 2] = s;
      sz[(j * G + gi) * 2 + 1] = -(float)(z + 1) * s;
    }
}

static int upload_weight_u8(cake_engine* e, unsigned char* dst,
                            const char* filebase, const StTensor& t,
                            size_t expect_elems) {
  size_t n = 1;
  for (long d : t.shape) n *= (size_t)d;
  if (n != expect_elems)
    return set_err(5, "fp8 tensor shape mismatch: got %zu want %zu", n,
                   expect_elems);
  if (t.dtype != "F8_E4M3" && t.dtype != "U8")
    return set_err(5, "expected F8_E4M3/U8 tensor, got %s", t.dtype.c_str());
  HIP_TRY(hipMemcpy(dst, filebase + t.off0, n, hipMemcpyHostToDevice));
  return 0;
}

static int upload_scale(cake_engine* e, float* dst, const char* filebase,
                        const StTensor& t, size_t expect_elems) {
  size_t n = 1;
  for (long d : t.shape) n *= (size_t)d;
  if (n != expect_elems)
    return set_err(5, "scale_inv shape mismatch: got %zu want %zu", n,
                   expect_elems);
  const char* src = filebase + t.off0;
  if (t.dtype == "F32") {
    HIP_TRY(hipMemcpy(dst, src, n * 4, hipMemcpyHostToDevice));
  } else if (t.dtype == "BF16") {
    std::vector<float> tmp(n);
    const u16* h = reinterpret_cast<const u16*>(src);
    for (size_t i = 0; i < n; ++i) {
      union { u32 u; float f; } v{(u32)h[i] << 16};
      tmp[i] = v.f;
    }
    HIP_TRY(hipMemcpy(dst, tmp.data(), n * 4, hipMemcpyHostToDevice));
  } else if (t.dtype == "F16") {
    std::vector<float> tmp(n);
    for (size_t i = 0; i < n; ++i) tmp[i] = f16_at(src, i);
    HIP_TRY(hipMemcpy(dst, tmp.data(), n * 4, hipMemcpyHostToDevice));
  } else {
    return set_err(5, "scale_inv dtype %s unsupported", t.dtype.c_str());
  }
  return 0;
}

static int upload_weight(cake_engine* e, u16* dst, const char* filebase,
                         const StTensor& t, size_t expect_elems) {
  size_t n = 1;
  for (long d : t.shape) n *= (size_t)d;
  if (n != expect_elems)
    return set_err(5, "tensor shape mismatch: got %zu want %zu elems", n,
                   expect_elems);
  const char* src = filebase + t.off0;
  if (t.dtype == "BF16") {
    HIP_TRY(hipMemcpy(dst, src, n * 2, hipMemcpyHostToDevice));
  } else if (t.dtype == "F32" || t.dtype == "F16") {
    // F16 (GPTQ checkpoints ship F16 norms and embeddings) widens exactly
    // to f32 and takes the same RNE path
    std::vector<u16> tmp(n);
    const float* f = reinterpret_cast<const float*>(src);
    const bool half = t.dtype == "F16";
    for (size_t i = 0; i < n; ++i) {
      union { float f; unsigned u; } v{half ? f16_at(src, i) : f[i]};
      unsigned r = ((v.u & 0x7fffffffu) > 0x7f800000u)
                       ? 0x7fc00000u
                       : v.u + 0x7fffu + ((v.u >> 16) & 1u);
      tmp[i] = (u16)(r >> 16);
    }
    HIP_TRY(hipMemcpy(dst, tmp.data(), n * 2, hipMemcpyHostToDevice));
  } else {
    return set_err(5, "unsupported safetensors dtype %s", t.dtype.c_str());
  }
  return 0;
}

// one projection's bias vector -> f32 (every source dtype widens exactly)
static int upload_bias(cake_engine* e, float* dst, const char* filebase,
                       const StTensor& t, const std::string& name,
                       size_t expect) {
  if (t.shape.size() != 1 || (size_t)t.shape[0] != expect) {
    std::string got;
    for (long d : t.shape) got += (got.empty() ? "" : ", ") + std::to_string(d);
    return set_err(5, "%s: shape (%s), expected (%zu)", name.c_str(),
                   got.c_str(), expect);
  }
  const char* src = filebase + t.off0;
  std::vector<float> tmp(expect);
  if (t.dtype == "F32") {
    memcpy(tmp.data(), src, expect * 4);
  } else if (t.dtype == "F16") {
    for (size_t i = 0; i < expect; ++i) tmp[i] = f16_at(src, i);
  } else if (t.dtype == "BF16") {
    for (size_t i = 0; i < expect; ++i) {
      u16 h;
      memcpy(&h, src + i * 2, 2);
      tmp[i] = b2f_host(h);
    }
  } else {
    return set_err(5, "%s: dtype %s, expected F32, F16 or BF16", name.c_str(),
                   t.dtype.c_str());
  }
  HIP_TRY(hipMemcpy(dst, tmp.data(), expect * 4, hipMemcpyHostToDevice));
  return 0;
}

// Load one safetensors file's relevant tensors (helper for single- and
// multi-file checkpoints).
static int load_safetensors_file(cake_engine* e, const char* path);

// Entry point: `path` may be (a) one .safetensors file, (b) a
// model.safetensors.index.json (sharded checkpoint — the layout cake's
// VarBuilder reads, utils/mod.rs:251-370), or (c) a directory containing
// either.
extern "C" int cake_hip_load_safetensors(cake_engine* e, const char* path) {
  std::string p(path);
  auto ends_with = [&](const std::string& s, const char* suf) {
    size_t n = strlen(suf);
    return s.size() >= n && s.compare(s.size() - n, n, suf) == 0;
  };
  // directory? try model.safetensors.index.json then model.safetensors
  if (!ends_with(p, ".safetensors") && !ends_with(p, ".json")) {
    std::string idx = p + "/model.safetensors.index.json";
    FILE* t = fopen(idx.c_str(), "rb");
    if (t) {
      fclose(t);
      p = idx;
    } else {
      p = p + "/model.safetensors";
    }
  }
  if (ends_with(p, ".json")) {
    // sharded checkpoint: weight_map = {tensor: file}; load each distinct
    // file once (tensors not present in a file are simply skipped there)
    FILE* f = fopen(p.c_str(), "rb");
    if (!f) return set_err(4, "cannot open %s", p.c_str());
    fseek(f, 0, SEEK_END);
    long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    std::string data((size_t)n, 0);
    if (fread(&data[0], 1, (size_t)n, f) != (size_t)n) {
      fclose(f);
      return set_err(4, "short read on %s", p.c_str());
    }
    fclose(f);
    minijson::ValuePtr v;
    try {
      v = minijson::parse(data);
    } catch (const std::exception& ex) {
      return set_err(4, "index.json: %s", ex.what());
    }
    auto wm = v->get("weight_map");
    if (!wm || wm->kind != minijson::Value::Obj)
      return set_err(4, "index.json has no weight_map");
    std::string dir = p.substr(0, p.find_last_of('/') + 1);
    std::vector<std::string> files;
    for (auto& kv : wm->obj) {
      const std::string& fn = kv.second->str;
      bool seen = false;
      for (auto& x : files) seen |= (x == fn);
      if (!seen) files.push_back(fn);
    }
    e->loading_multi = true;
    e->missing.clear();
    e->loaded.clear();
    for (auto& fn : files) {
      std::string full = dir + fn;
      int r = load_safetensors_file(e, full.c_str());
      if (r) {
        e->loading_multi = false;
        return r;
      }
    }
    e->loading_multi = false;
    // final presence check: every required tensor must have been seen
    if (!e->missing.empty())
      return set_err(4, "sharded checkpoint is missing tensor %s",
                     e->missing.begin()->c_str());
    HIP_TRY(hipDeviceSynchronize());
    e->weights_ready = true;
    return 0;
  }
  int r = load_safetensors_file(e, p.c_str());
  if (r) return r;
  HIP_TRY(hipDeviceSynchronize());
  e->weights_ready = true;
  return 0;
}

static int load_safetensors_file(cake_engine* e, const char* path) {
  HIP_TRY(hipSetDevice(e->device));
  FILE* f = fopen(path, "rb");
  if (!f) return set_err(4, "cannot open %s", path);
  fseek(f, 0, SEEK_END);
  long fsize = ftell(f);
  fseek(f, 0, SEEK_SET);
  std::vector<char> data((size_t)fsize);
  if (fread(data.data(), 1, (size_t)fsize, f) != (size_t)fsize) {
    fclose(f);
    return set_err(4, "short read on %s", path);
  }
  fclose(f);
  if (fsize < 8) return set_err(4, "bad safetensors file");
  uint64_t hlen;
  memcpy(&hlen, data.data(), 8);
  if ((long)(8 + hlen) > fsize) return set_err(4, "bad safetensors header");
  std::string header(data.data() + 8, hlen);
  minijson::ValuePtr hv;
  try {
    hv = minijson::parse(header);
  } catch (const std::exception& ex) {
    return set_err(4, "safetensors header: %s", ex.what());
  }
  std::map<std::string, StTensor> tensors;
  for (auto& kv : hv->obj) {
    if (kv.first == "__metadata__") continue;
    StTensor t;
    if (auto d = kv.second->get("dtype")) t.dtype = d->str;
    if (auto sh = kv.second->get("shape"))
      for (auto& d : sh->arr) t.shape.push_back((long)d->num);
    if (auto off = kv.second->get("data_offsets")) {
      t.off0 = (size_t)off->arr[0]->num;
      t.off1 = (size_t)off->arr[1]->num;
    }
    tensors[kv.first] = t;
  }
  const char* base = data.data() + 8 + hlen;
  const ModelConfig& c = e->c;
  const size_t H = c.hidden, I = c.inter, V = c.vocab;
  const size_t hd = c.hd(), Sq = c.sq(), Skv = c.skv();

  // In multi-file mode a tensor may live in another shard: record it as
  // pending instead of failing; the index loader checks completeness.
  auto need = [&](const std::string& name, StTensor* out_t) -> int {
    if (e->loading_multi && e->loaded.count(name))
      return -1;  // already uploaded from an earlier shard
    auto it = tensors.find(name);
    if (it == tensors.end()) {
      if (e->loading_multi) {
        e->missing.insert(name);
        return -1;  // sentinel: maybe in a later shard
      }
      return set_err(4, "missing tensor %s", name.c_str());
    }
    if (e->loading_multi) {
      e->loaded.insert(name);
      e->missing.erase(name);
    }
    *out_t = it->second;
    return 0;
  };
#define LOADW(NAME, UPLOAD_EXPR)                                       \
  do {                                                                 \
    int _r = need((NAME), &t);                                         \
    if (_r == -1) break; /* lives in another shard */                  \
    if (_r) return _r;                                                 \
    if ((_r = (UPLOAD_EXPR))) return _r;                               \
  } while (0)
  int r;
  StTensor t;
  // one gptq projection P (N out, K in, group g) -> rows [row0, row0 + N) of
  // the fused device tensor dw / dsz
  auto load_w4 = [&](const std::string& P, u32* dw, float* dsz, size_t row0,
                     size_t N, size_t K, size_t g) -> int {
    StTensor tq, tz, ts;
    int rr = need(P + ".qweight", &tq);
    if (rr == -1) return 0;  // lives in another shard, with its companions
    if (rr) return rr;
    for (auto nt : {std::make_pair(".qzeros", &tz),
                    std::make_pair(".scales", &ts)}) {
      rr = need(P + nt.first, nt.second);
      if (rr == -1)
        return set_err(4, "%s%s must be in the same file as %s.qweight",
                       P.c_str(), nt.first, P.c_str());
      if (rr) return rr;
    }
    const size_t G = K / g;
    auto shape_is = [](const StTensor& s, size_t a, size_t b) {
      return s.shape.size() == 2 && (size_t)s.shape[0] == a &&
             (size_t)s.shape[1] == b;
    };
    auto bad = [&](const char* suf, const StTensor& s, const char* dt,
                   size_t a, size_t b) {
      std::string got;
      for (long d : s.shape) got += (got.empty() ? "" : ", ") + std::to_string(d);
      return set_err(5, "%s%s: %s (%s), expected %s (%zu, %zu)", P.c_str(),
                     suf, s.dtype.c_str(), got.c_str(), dt, a, b);
    };
    if (tq.dtype != "I32" || !shape_is(tq, K / 8, N))
      return bad(".qweight", tq, "I32", K / 8, N);
    if (tz.dtype != "I32" || !shape_is(tz, G, N / 8))
      return bad(".qzeros", tz, "I32", G, N / 8);
    const bool sdt = ts.dtype == "F16" || ts.dtype == "BF16" ||
                     ts.dtype == "F32";
    if (!sdt || !shape_is(ts, G, N)) return bad(".scales", ts, "F16", G, N);
    std::vector<int32_t> qw(K / 8 * N), qz(G * (N / 8));
    memcpy(qw.data(), base + tq.off0, qw.size() * 4);
    memcpy(qz.data(), base + tz.off0, qz.size() * 4);
    std::vector<float> sc(G * N);
    const char* sp = base + ts.off0;
    for (size_t i = 0; i < sc.size(); ++i) {
      if (ts.dtype == "F16") {
        sc[i] = f16_at(sp, i);
      } else if (ts.dtype == "BF16") {
        u16 h;
        memcpy(&h, sp + i * 2, 2);
        sc[i] = b2f_host(h);
      } else {
        memcpy(&sc[i], sp + i * 4, 4);
      }
    }
    std::vector<u32> W(N * (K / 8));
    std::vector<float> sz(N * G * 2);
    w4_repack(qw.data(), qz.data(), sc.data(), N, K, g, W.data(), sz.data());
    HIP_TRY(hipMemcpy(dw + row0 * (K / 8), W.data(), W.size() * 4,
                      hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dsz + row0 * G * 2, sz.data(), sz.size() * 4,
                      hipMemcpyHostToDevice));
    return 0;
  };
  if (e->has_embed()) {
    LOADW("model.embed_tokens.weight", upload_weight(e, e->embed, base, t, V * H));
  }
  if (e->has_head()) {
    LOADW("model.norm.weight", upload_weight(e, e->norm_w, base, t, H));
    if (!(c.tied && e->has_embed())) {
      std::string name = c.tied ? "model.embed_tokens.weight"
                                : "lm_head.weight";
      LOADW(name, upload_weight(e, e->lm_head, base, t, V * H));
    }
  }
  for (int li = e->lo; li < e->hi; ++li) {
    LayerDev& l = e->L[li - e->lo];
    char p[128];
    snprintf(p, sizeof p, "model.layers.%d.", li);
    std::string pre(p);
    LOADW(pre + "input_layernorm.weight", upload_weight(e, l.rms1, base, t, H));
    LOADW(pre + "post_attention_layernorm.weight", upload_weight(e, l.rms2, base, t, H));
    if (c.fp8) {
      // fp8 weights + blockwise scale_inv (fp8.rs:42-64); fused qkv and
      // gate_up concatenate both the byte tensors and the scale rows
      const size_t Hb = H / 128, Sqb = Sq / 128, Skvb = Skv / 128,
                   Ib = I / 128;
      LOADW(pre + "self_attn.q_proj.weight", upload_weight_u8(e, l.wqkv8, base, t, Sq * H));
      LOADW(pre + "self_attn.k_proj.weight", upload_weight_u8(e, l.wqkv8 + Sq * H, base, t, Skv * H));
      LOADW(pre + "self_attn.v_proj.weight", upload_weight_u8(e, l.wqkv8 + (Sq + Skv) * H, base, t, Skv * H));
      LOADW(pre + "self_attn.q_proj.weight_scale_inv", upload_scale(e, l.sqkv, base, t, Sqb * Hb));
      LOADW(pre + "self_attn.k_proj.weight_scale_inv", upload_scale(e, l.sqkv + Sqb * Hb, base, t, Skvb * Hb));
      LOADW(pre + "self_attn.v_proj.weight_scale_inv", upload_scale(e, l.sqkv + (Sqb + Skvb) * Hb, base, t, Skvb * Hb));
      LOADW(pre + "self_attn.o_proj.weight", upload_weight_u8(e, l.wo8, base, t, H * Sq));
      LOADW(pre + "self_attn.o_proj.weight_scale_inv", upload_scale(e, l.so8, base, t, Hb * Sqb));
      LOADW(pre + "mlp.gate_proj.weight", upload_weight_u8(e, l.wgu8, base, t, I * H));
      LOADW(pre + "mlp.up_proj.weight", upload_weight_u8(e, l.wgu8 + I * H, base, t, I * H));
      LOADW(pre + "mlp.gate_proj.weight_scale_inv", upload_scale(e, l.sgu, base, t, Ib * Hb));
      LOADW(pre + "mlp.up_proj.weight_scale_inv", upload_scale(e, l.sgu + Ib * Hb, base, t, Ib * Hb));
      LOADW(pre + "mlp.down_proj.weight", upload_weight_u8(e, l.wdown8, base, t, H * I));
      LOADW(pre + "mlp.down_proj.weight_scale_inv", upload_scale(e, l.sdown, base, t, Hb * Ib));
    } else if (c.fused_ckpt) {
      // phi3: qkv_proj (q|k|v rows) and gate_up_proj (gate rows, then up
      // rows) are the engine's own wqkv / wgu layouts and load whole
      // (phi4/config.rs:88-89); a checkpoint with split names fails on the
      // fused name
      const size_t Nq = Sq + 2 * Skv;
      if (c.w4) {
        const size_t gH = c.grp((int)H), gS = c.grp((int)Sq), gI = c.grp((int)I);
        if ((r = load_w4(pre + "self_attn.qkv_proj", l.wqkv4, l.zqkv, 0, Nq, H, gH))) return r;
        if ((r = load_w4(pre + "self_attn.o_proj", l.wo4, l.zo, 0, H, Sq, gS))) return r;
        if ((r = load_w4(pre + "mlp.gate_up_proj", l.wgu4, l.zgu, 0, 2 * I, H, gH))) return r;
        if ((r = load_w4(pre + "mlp.down_proj", l.wdown4, l.zdown, 0, H, I, gI))) return r;
      } else {
        auto fused = [&](const std::string& name, u16* dst, size_t N) -> int {
          if (t.shape.size() != 2 || (size_t)t.shape[0] != N ||
              (size_t)t.shape[1] != H) {
            std::string got;
            for (long d : t.shape) got += (got.empty() ? "" : ", ") + std::to_string(d);
            return set_err(5, "%s: shape (%s), expected (%zu, %zu)",
                           name.c_str(), got.c_str(), N, H);
          }
          return upload_weight(e, dst, base, t, N * H);
        };
        LOADW(pre + "self_attn.qkv_proj.weight", fused(pre + "self_attn.qkv_proj.weight", l.wqkv, Nq));
        LOADW(pre + "self_attn.o_proj.weight", upload_weight(e, l.wo, base, t, H * Sq));
        LOADW(pre + "mlp.gate_up_proj.weight", fused(pre + "mlp.gate_up_proj.weight", l.wgu, 2 * I));
        LOADW(pre + "mlp.down_proj.weight", upload_weight(e, l.wdown, base, t, H * I));
      }
    } else if (c.w4) {
      // gptq: qweight/qzeros/scales per projection, repacked out-major at
      // the projection's row offset of the fused tensor (g_idx is ignored,
      // as gptq.rs does; so is every bias but qwen2's q/k/v, loaded below)
      const size_t gH = c.grp((int)H), gS = c.grp((int)Sq), gI = c.grp((int)I);
      if ((r = load_w4(pre + "self_attn.q_proj", l.wqkv4, l.zqkv, 0, Sq, H, gH))) return r;
      if ((r = load_w4(pre + "self_attn.k_proj", l.wqkv4, l.zqkv, Sq, Skv, H, gH))) return r;
      if ((r = load_w4(pre + "self_attn.v_proj", l.wqkv4, l.zqkv, Sq + Skv, Skv, H, gH))) return r;
      if ((r = load_w4(pre + "self_attn.o_proj", l.wo4, l.zo, 0, H, Sq, gS))) return r;
      if ((r = load_w4(pre + "mlp.gate_proj", l.wgu4, l.zgu, 0, I, H, gH))) return r;
      if ((r = load_w4(pre + "mlp.up_proj", l.wgu4, l.zgu, I, I, H, gH))) return r;
      if ((r = load_w4(pre + "mlp.down_proj", l.wdown4, l.zdown, 0, H, I, gI))) return r;
    } else {
    // fused qkv: upload q,k,v at row offsets (attention.rs:109-114)
    LOADW(pre + "self_attn.q_proj.weight", upload_weight(e, l.wqkv, base, t, Sq * H));
    LOADW(pre + "self_attn.k_proj.weight", upload_weight(e, l.wqkv + Sq * H, base, t, Skv * H));
    LOADW(pre + "self_attn.v_proj.weight", upload_weight(e, l.wqkv + (Sq + Skv) * H, base, t, Skv * H));
    LOADW(pre + "self_attn.o_proj.weight", upload_weight(e, l.wo, base, t, H * Sq));
    // fused gate_up (mlp.rs:38-46)
    LOADW(pre + "mlp.gate_proj.weight", upload_weight(e, l.wgu, base, t, I * H));
    LOADW(pre + "mlp.up_proj.weight", upload_weight(e, l.wgu + I * H, base, t, I * H));
    LOADW(pre + "mlp.down_proj.weight", upload_weight(e, l.wdown, base, t, H * I));
    }
    if (c.qkv_bias) {
      // qwen2, every weight format alike: required F32/F16/BF16 vectors at
      // the projection's row offset of the fused bias (attention.rs:95-104)
      LOADW(pre + "self_attn.q_proj.bias", upload_bias(e, l.bqkv, base, t, pre + "self_attn.q_proj.bias", Sq));
      LOADW(pre + "self_attn.k_proj.bias", upload_bias(e, l.bqkv + Sq, base, t, pre + "self_attn.k_proj.bias", Skv));
      LOADW(pre + "self_attn.v_proj.bias", upload_bias(e, l.bqkv + Sq + Skv, base, t, pre + "self_attn.v_proj.bias", Skv));
    }
    if (c.qk_norm) {
      LOADW(pre + "self_attn.q_norm.weight", upload_weight(e, l.qnorm, base, t, hd));
      LOADW(pre + "self_attn.k_norm.weight", upload_weight(e, l.knorm, base, t, hd));
    }
  }
#undef LOADW
  HIP_TRY(hipDeviceSynchronize());
  return 0;
}

extern "C" int cake_hip_init_random(cake_engine* e, uint64_t seed,
                                    float scale) {
  HIP_TRY(hipSetDevice(e->device));
  const ModelConfig& c = e->c;
  const size_t H = c.hidden, I = c.inter, V = c.vocab;
  const size_t hd = c.hd(), Sq = c.sq(), Skv = c.skv();
  // Salts derive from the tensor's IDENTITY (absolute layer index + slot),
  // not fill order, so a sharded engine's layer k gets bit-identical
  // weights to a monolithic engine's layer k — the multi-rank pipeline
  // parity tests depend on this.
  auto fill = [&](u16* p, size_t n, uint64_t salt) {
    launch_fill_random(p, n, seed + 0x1000193u * salt, scale, e->stream);
  };
  if (e->has_embed()) fill(e->embed, V * H, 1);
  if (e->has_head()) {
    launch_fill_const(e->norm_w, H, 1.0f, e->stream);
    if (!(c.tied && e->has_embed())) fill(e->lm_head, V * H, 2);
  }
  std::vector<float> hscales;
  auto fill_scales = [&](float* p, size_t n) {
    hscales.resize(n);
    for (size_t i = 0; i < n; ++i)
      hscales[i] = 3e-4f + 2e-4f * (float)((i * 2654435761u) % 1000) / 1000.f;
    hipMemcpy(p, hscales.data(), n * 4, hipMemcpyHostToDevice);
  };
  for (auto& l : e->L) {
    const uint64_t base = 16 + (uint64_t)l.idx * 8;
    launch_fill_const(l.rms1, H, 1.0f, e->stream);
    launch_fill_const(l.rms2, H, 1.0f, e->stream);
    if (c.fp8) {
      const size_t Hb = H / 128, Sqb = Sq / 128, Skvb = Skv / 128,
                   Ib = I / 128;
      launch_fill_random_u8(l.wqkv8, (Sq + 2 * Skv) * H,
                            seed + 0x1000193u * base, e->stream);
      launch_fill_random_u8(l.wo8, H * Sq, seed + 0x1000193u * (base + 1),
                            e->stream);
      launch_fill_random_u8(l.wgu8, 2 * I * H,
                            seed + 0x1000193u * (base + 2), e->stream);
      launch_fill_random_u8(l.wdown8, H * I,
                            seed + 0x1000193u * (base + 3), e->stream);
      fill_scales(l.sqkv, (Sqb + 2 * Skvb) * Hb);
      fill_scales(l.so8, Hb * Sqb);
      fill_scales(l.sgu, 2 * Ib * Hb);
      fill_scales(l.sdown, Hb * Ib);
    } else if (c.w4) {
      // random nibbles, stored zero 7 (z + 1 = 8: q - 8 in [-8, 7]) and
      // f16-representable scales around scale / 8 (+-20 %, by index), so the
      // weights spread over about +-scale like the bf16 init
      auto fill_sz = [&](float* p, size_t n) {
        hscales.resize(2 * n);
        for (size_t i = 0; i < n; ++i) {
          const float f =
              0.8f + 0.4f * (float)((i * 2654435761u) % 1000) / 1000.f;
          const float sv = (float)(_Float16)(scale * 0.125f * f);
          hscales[2 * i] = sv;
          hscales[2 * i + 1] = -8.f * sv;
        }
        hipMemcpy(p, hscales.data(), 2 * n * 4, hipMemcpyHostToDevice);
      };
      const size_t GH = H / c.grp((int)H), GS = Sq / c.grp((int)Sq),
                   GI = I / c.grp((int)I);
      launch_fill_random_u32(l.wqkv4, (Sq + 2 * Skv) * H / 8,
                             seed + 0x1000193u * base, e->stream);
      launch_fill_random_u32(l.wo4, H * Sq / 8,
                             seed + 0x1000193u * (base + 1), e->stream);
      launch_fill_random_u32(l.wgu4, 2 * I * H / 8,
                             seed + 0x1000193u * (base + 2), e->stream);
      launch_fill_random_u32(l.wdown4, H * I / 8,
                             seed + 0x1000193u * (base + 3), e->stream);
      fill_sz(l.zqkv, (Sq + 2 * Skv) * GH);
      fill_sz(l.zo, H * GS);
      fill_sz(l.zgu, 2 * I * GH);
      fill_sz(l.zdown, H * GI);
    } else {
      fill(l.wqkv, (Sq + 2 * Skv) * H, base);
      fill(l.wo, H * Sq, base + 1);
      fill(l.wgu, 2 * I * H, base + 2);
      fill(l.wdown, H * I, base + 3);
    }
    if (l.qnorm) {
      launch_fill_const(l.qnorm, hd, 1.0f, e->stream);
      launch_fill_const(l.knorm, hd, 1.0f, e->stream);
    }
    if (l.bqkv) {
      // slot 4 of the layer: q and k rows ~uniform(+-3) (real qwen2 q/k
      // biases are large), v rows ~uniform(+-0.25); splitmix64 of the index
      const uint64_t bs = seed + 0x1000193u * (base + 4);
      hscales.resize(Sq + 2 * Skv);
      for (size_t i = 0; i < hscales.size(); ++i) {
        uint64_t z = bs + 0x9e3779b97f4a7c15ull * (uint64_t)(i + 1);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        z ^= z >> 31;
        const float u = (float)(z >> 40) * 0x1p-23f - 1.f;  // [-1, 1)
        hscales[i] = u * (i < Sq + Skv ? 3.f : 0.25f);
      }
      hipMemcpy(l.bqkv, hscales.data(), hscales.size() * 4,
                hipMemcpyHostToDevice);
    }
  }
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->weights_ready = true;
  return 0;
}

// ---------------------------------------------------------------------------
// generation
// ---------------------------------------------------------------------------
extern "C" int cake_hip_reset(cake_engine* e) {
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  HIP_TRY(hipMemset(e->dev_pos, 0, 4));
  HIP_TRY(hipMemset(e->dev_step, 0, 4));
  HIP_TRY(hipMemset(e->dev_tok, 0, 4));
  // sampler history and draw counter start over with the sequence
  if (e->sample_mem) HIP_TRY(hipMemset(e->sws.state, 0, 4 * 4));
  // clear the KV caches (Goodbye semantics, worker.rs:364-384 /
  // cache.rs:248-253)
  const size_t kv_bytes = (size_t)e->c.nkv * e->max_seq * e->c.hd() * 2;
  for (auto& l : e->L) {
    HIP_TRY(hipMemsetAsync(l.kc, 0, kv_bytes, e->stream));
    HIP_TRY(hipMemsetAsync(l.vc, 0, kv_bytes, e->stream));
    HIP_TRY(hipMemsetAsync(l.vtc, 0, kv_bytes, e->stream));
  }
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->host_pos = 0;
  return 0;
}

extern "C" int cake_hip_prefill(cake_engine* e, const uint32_t* tokens,
                                int n_tokens, uint32_t* next_token,
                                float* logits_out) {
  HIP_TRY(hipSetDevice(e->device));
  if (!e->weights_ready) return set_err(1, "weights not loaded");
  if (n_tokens <= 0) return set_err(5, "n_tokens must be > 0");
  if (e->host_pos + n_tokens > e->max_seq)
    return set_err(5, "prefill exceeds max_seq (%d + %d > %d)", e->host_pos,
                   n_tokens, e->max_seq);
  const ModelConfig& c = e->c;
  const int H = c.hidden;
  const bool overlap = e->world > 1 && e->prefill_overlap != 0;
  int done = 0, ci = 0;
  while (done < n_tokens) {
    int S = std::min(n_tokens - done, e->bt);
    int pos0 = e->host_pos;
    bool last_chunk = (done + S == n_tokens);
    if (overlap) {
      // Pipelined multi-rank prefill (north_star's second-HIP-stream
      // overlap): chunk activations double-buffer between e->x / e->x2;
      // all RCCL calls go on comm_stream, ordered against compute by
      // events, so chunk c's hop to the next rank rides UNDER chunk
      // c+1's layers instead of serializing the whole ring per chunk.
      // Only the FINAL chunk's activation returns to rank 0 (the
      // intermediate returns the serial ring made were never consumed:
      // rank 0 uses only the last chunk for the head, text_model.rs:334).
      u16* xb = (ci & 1) ? e->x2 : e->x;
      hipEvent_t evc = e->ev_comp[ci & 1], evm = e->ev_comm[ci & 1];
      if (e->rank == 0) {
        if (!tokens) return set_err(5, "rank 0 needs tokens");
        HIP_TRY(hipMemcpyAsync(e->ids, tokens + done, (size_t)S * 4,
                               hipMemcpyHostToDevice, e->stream));
        // buffer reuse: chunk ci-2's send (comm_stream) must have read
        // xb before this chunk's embed overwrites it
        if (ci >= 2) HIP_TRY(hipStreamWaitEvent(e->stream, evm, 0));
        launch_embed_rows(e->embed, e->ids, xb, S, H, e->stream);
        for (auto& l : e->L) enqueue_layer_prefill(e, l, S, pos0, xb);
        HIP_TRY(hipEventRecord(evc, e->stream));
        HIP_TRY(hipStreamWaitEvent(e->comm_stream, evc, 0));
        NCCL_TRY(ncclSend(xb, (size_t)S * H, ncclBfloat16, 1, e->comm,
                          e->comm_stream));
        HIP_TRY(hipEventRecord(evm, e->comm_stream));  // send-done
        if (last_chunk) {
          NCCL_TRY(ncclRecv(xb, (size_t)S * H, ncclBfloat16, e->world - 1,
                            e->comm, e->comm_stream));
          HIP_TRY(hipEventRecord(evm, e->comm_stream));
          HIP_TRY(hipStreamWaitEvent(e->stream, evm, 0));
          enqueue_head_sample(e, S, S, xb);
        } else {
          launch_advance_pos(e->dev_pos, S, e->stream);
        }
      } else {
        NCCL_TRY(ncclRecv(xb, (size_t)S * H, ncclBfloat16, e->rank - 1,
                          e->comm, e->comm_stream));
        HIP_TRY(hipEventRecord(evm, e->comm_stream));
        HIP_TRY(hipStreamWaitEvent(e->stream, evm, 0));
        for (auto& l : e->L) enqueue_layer_prefill(e, l, S, pos0, xb);
        HIP_TRY(hipEventRecord(evc, e->stream));
        HIP_TRY(hipStreamWaitEvent(e->comm_stream, evc, 0));
        if (e->rank + 1 < e->world) {
          NCCL_TRY(ncclSend(xb, (size_t)S * H, ncclBfloat16, e->rank + 1,
                            e->comm, e->comm_stream));
        } else if (last_chunk) {
          NCCL_TRY(ncclSend(xb, (size_t)S * H, ncclBfloat16, 0, e->comm,
                            e->comm_stream));
        }
        launch_advance_pos(e->dev_pos, S, e->stream);
      }
    } else if (e->world == 1 || e->rank == 0) {
      if (!tokens) return set_err(5, "rank 0 needs tokens");
      HIP_TRY(hipMemcpyAsync(e->ids, tokens + done, (size_t)S * 4,
                             hipMemcpyHostToDevice, e->stream));
      auto enqueue_chunk = [&]() -> int {
        launch_embed_rows(e->embed, e->ids, e->x, S, H, e->stream);
        for (auto& l : e->L) enqueue_layer_prefill(e, l, S, pos0);
        if (e->world > 1) {
          NCCL_TRY(ncclSend(e->x, (size_t)S * H, ncclBfloat16, 1, e->comm,
                            e->stream));
          NCCL_TRY(ncclRecv(e->x, (size_t)S * H, ncclBfloat16, e->world - 1,
                            e->comm, e->stream));
        }
        if (last_chunk) {
          enqueue_head_sample(e, S, S);
        } else {
          launch_advance_pos(e->dev_pos, S, e->stream);
        }
        return 0;
      };
      // Prefill hipGraph (single rank, whole prompt in ONE chunk from
      // pos 0 — the serving/bench first-prefill case).  Measured with
      // in-context event stats (tools/prefill_stats.py): the eager 8B
      // S=2048 prefill carries ~1.7 ms of host launch gap on a ~33 ms
      // wall; replay removes it (~+1-2%) and makes the prefill a single
      // launch.  The ids H2D copy stays OUTSIDE the graph
      // (its source pointer varies per call); everything after reads
      // device state, so replay == eager.  First sighting of a shape
      // runs eager (it also builds the hipBLASLt plans, which allocate
      // and must not run under capture); the second captures; later
      // ones replay.  Any capture failure permanently falls back.
      static const bool pf_graph_env = [] {
        const char* v = getenv("CAKE_PREFILL_GRAPH");
        return !v || atoi(v) != 0;
      }();
      const bool whole = (done == 0 && last_chunk);
      const bool pg_ok = pf_graph_env && e->world == 1 && e->use_graph() &&
                         !e->st.on && !e->pf_graph_dead && whole &&
                         pos0 == 0 && e->has_head();
      if (pg_ok && e->pf_graph && e->pf_graph_S == S) {
        HIP_TRY(hipGraphLaunch(e->pf_graph, e->stream));
      } else if (pg_ok && e->pf_seen_S == S && e->pf_seen_cnt >= 1) {
        if (e->pf_graph) {
          HIP_TRY(hipGraphExecDestroy(e->pf_graph));
          e->pf_graph = nullptr;
        }
        hipError_t rc =
            hipStreamBeginCapture(e->stream, hipStreamCaptureModeGlobal);
        bool captured = false;
        if (rc == hipSuccess) {
          int r = enqueue_chunk();
          hipGraph_t g = nullptr;
          rc = hipStreamEndCapture(e->stream, &g);
          if (r == 0 && rc == hipSuccess && g &&
              hipGraphInstantiate(&e->pf_graph, g, nullptr, nullptr, 0) ==
                  hipSuccess) {
            hipGraphDestroy(g);
            e->pf_graph_S = S;
            captured = true;
            if (getenv("CAKE_DEBUG_PFGRAPH"))
              fprintf(stderr, "[cake_hip] prefill graph captured S=%d\n", S);
            HIP_TRY(hipGraphLaunch(e->pf_graph, e->stream));
          } else if (g) {
            hipGraphDestroy(g);
          }
        }
        if (!captured) {
          // nothing enqueued during a failed capture ran — do it eagerly
          (void)hipGetLastError();
          e->pf_graph_dead = true;
          int r = enqueue_chunk();
          if (r) return r;
        }
      } else {
        int r = enqueue_chunk();
        if (r) return r;
        if (whole) {
          if (e->pf_seen_S == S)
            e->pf_seen_cnt += 1;
          else {
            e->pf_seen_S = S;
            e->pf_seen_cnt = 1;
          }
        }
      }
    } else {
      NCCL_TRY(ncclRecv(e->x, (size_t)S * H, ncclBfloat16, e->rank - 1,
                        e->comm, e->stream));
      for (auto& l : e->L) enqueue_layer_prefill(e, l, S, pos0);
      NCCL_TRY(ncclSend(e->x, (size_t)S * H, ncclBfloat16,
                        (e->rank + 1) % e->world, e->comm, e->stream));
      launch_advance_pos(e->dev_pos, S, e->stream);
    }
    e->host_pos += S;
    done += S;
    ci += 1;
  }
  if (overlap) HIP_TRY(hipStreamSynchronize(e->comm_stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  stats_flush(e);
  if ((e->world == 1 || e->rank == 0) && e->has_head()) {
    if (next_token) {
      u32 tok;
      HIP_TRY(hipMemcpy(&tok, e->dev_tok, 4, hipMemcpyDeviceToHost));
      *next_token = tok;
    }
    if (logits_out) {
      HIP_TRY(hipMemcpy(logits_out, e->logits, (size_t)c.vocab * 4,
                        hipMemcpyDeviceToHost));
    }
  }
  return 0;
}

extern "C" int cake_hip_decode(cake_engine* e, int steps,
                               uint32_t* tokens_out) {
  HIP_TRY(hipSetDevice(e->device));
  if (!e->weights_ready) return set_err(1, "weights not loaded");
  if (steps <= 0 || steps > cake_engine::RING_CAP)
    return set_err(5, "steps out of range");
  if (e->host_pos + steps > e->max_seq)
    return set_err(5, "decode exceeds max_seq");
  HIP_TRY(hipMemsetAsync(e->dev_step, 0, 4, e->stream));
  // Split-KV chunk count for decode attention, by context length.  With
  // the K-prefetch kernel the curve is nearly flat (8..24 within 2%);
  // measured optima: ctx 2048 -> 8~12, 3960 -> 12~16, 7900 -> 16~24.
  // The graph bakes the grid in, so when the context grows across a
  // threshold the graph is dropped and lazily re-captured with the new
  // chunk count (capture costs ~1 step, amortized over thousands).
  const bool nchunk_fixed = getenv("CAKE_NCHUNK") != nullptr;
  // Chunk policy: the GQA-grouped kernel (grid_y = nkv*subg blocks per
  // chunk) wants ~2 blocks/CU of parallelism => ~512 blocks, bounded by
  // one 64-position tile per chunk and the ws capacity (64).  Values are
  // quantized so the graph re-captures only a handful of times as the
  // context grows.  The per-head fallback kernel keeps its r01 curve.
  // nchunk=1 (direct-write, no combine) measured NEGATIVE beyond 1-2
  // tiles: serial per-tile latency at 8-24 blocks beats the combine
  // saving (r02c11: ctx128 15.1us vs 11.0 at nchunk 4) — default off,
  // env knob kept for experiments
  static const int nc1_tiles =
      getenv("CAKE_NC1_TILES") ? atoi(getenv("CAKE_NC1_TILES")) : 0;
  const int gy = attn_decode_grid_y(e->c.nh, e->c.nkv, e->c.hd());
  auto want_nchunk = [gy](int pos) {
    if (gy > 0) {
      const int span_tiles = (pos + 64) / 64;
      if (span_tiles <= nc1_tiles) return 1;
      const int target = std::max(4, std::min(64, 512 / gy));
      const int v = std::min(span_tiles, target);
      return v <= 4 ? 4 : v <= 8 ? 8 : v <= 16 ? 16 : v <= 24 ? 24
             : v <= 32 ? 32 : v <= 48 ? 48 : 64;
    }
    return pos < 1024 ? 8 : pos < 6144 ? 12 : 16;
  };
  bool graph_ok = e->use_graph() && e->world == 1 && !e->st.on;
  if (!nchunk_fixed) {
    const int want = want_nchunk(e->host_pos);
    if (want != e->nchunk) {
      if (e->graph) {
        HIP_TRY(hipGraphExecDestroy(e->graph));
        e->graph = nullptr;
      }
      e->nchunk = want;
      // the epoch-free arrival counters advance by nchunk per step, so a
      // chunk-count change invalidates their modulo election: re-zero
      // (stream is idle here — the previous call ended in a sync)
      HIP_TRY(hipMemset(e->attn_cnt, 0, sizeof(u32) * e->c.nh));
    }
  }
  for (int s = 0; s < steps; ++s) {
    if (graph_ok && !e->graph) {
      // capture one decode step (device-side token/pos/ring make it
      // replayable)
      hipGraph_t g;
      HIP_TRY(hipStreamBeginCapture(e->stream, hipStreamCaptureModeGlobal));
      int r = enqueue_decode_step(e);
      if (r) {
        hipStreamEndCapture(e->stream, &g);
        return r;
      }
      HIP_TRY(hipStreamEndCapture(e->stream, &g));
      HIP_TRY(hipGraphInstantiate(&e->graph, g, nullptr, nullptr, 0));
      HIP_TRY(hipGraphDestroy(g));
    }
    if (graph_ok) {
      HIP_TRY(hipGraphLaunch(e->graph, e->stream));
    } else {
      int r = enqueue_decode_step(e);
      if (r) return r;
    }
    e->host_pos += 1;
    // bound in-flight work: sync every 64 steps to keep the queue shallow;
    // same cadence re-checks the chunk-count threshold as context grows
    if ((s & 63) == 63) {
      HIP_TRY(hipStreamSynchronize(e->stream));
      if (!nchunk_fixed) {
        const int want = want_nchunk(e->host_pos);
        if (want != e->nchunk) {
          if (e->graph) {
            HIP_TRY(hipGraphExecDestroy(e->graph));
            e->graph = nullptr;
          }
          e->nchunk = want;
          HIP_TRY(hipMemset(e->attn_cnt, 0, sizeof(u32) * e->c.nh));
        }
      }
    }
  }
  HIP_TRY(hipStreamSynchronize(e->stream));
  stats_flush(e);
  if (tokens_out && (e->world == 1 || e->rank == 0) && e->has_head()) {
    HIP_TRY(hipMemcpy(tokens_out, e->ring, (size_t)steps * 4,
                      hipMemcpyDeviceToHost));
  }
  return 0;
}

// Run a contiguous SUB-range [lo_abs, hi_abs) of this shard's layers — the
// unit the reference worker executes per op: each (layer_name, index_pos,
// block_idx) in a Batch/SingleOp is looked up and run independently
// (worker.rs:442-515), so a master may drive any subset of the shard.
extern "C" int cake_hip_forward_hidden_range(cake_engine* e, const float* x,
                                             int seq, int index_pos,
                                             int lo_abs, int hi_abs,
                                             float* out) {
  HIP_TRY(hipSetDevice(e->device));
  if (!e->weights_ready) return set_err(1, "weights not loaded");
  if (seq <= 0 || seq > e->bt) return set_err(5, "bad seq");
  if (lo_abs < e->lo || hi_abs > e->hi || lo_abs >= hi_abs)
    return set_err(5, "layer range [%d,%d) outside this shard [%d,%d)",
                   lo_abs, hi_abs, e->lo, e->hi);
  const int H = e->c.hidden;
  HIP_TRY(hipMemcpyAsync(e->fbuf, x, (size_t)seq * H * 4,
                         hipMemcpyHostToDevice, e->stream));
  launch_f32_to_bf16(e->fbuf, e->x, (size_t)seq * H, e->stream);
  // sync device position with the caller's index_pos
  HIP_TRY(hipStreamSynchronize(e->stream));
  HIP_TRY(hipMemcpy(e->dev_pos, &index_pos, 4, hipMemcpyHostToDevice));
  e->host_pos = index_pos;
  if (seq == 1) {
    // host-provided x: no producing kernel, first layer falls back
    for (int li = lo_abs; li < hi_abs; ++li)
      enqueue_layer_decode(e, e->L[li - e->lo], li > lo_abs);
  } else {
    for (int li = lo_abs; li < hi_abs; ++li)
      enqueue_layer_prefill(e, e->L[li - e->lo], seq, index_pos);
  }
  launch_advance_pos(e->dev_pos, seq, e->stream);
  launch_bf16_to_f32(e->x, e->fbuf, (size_t)seq * H, e->stream);
  HIP_TRY(hipMemcpyAsync(out, e->fbuf, (size_t)seq * H * 4,
                         hipMemcpyDeviceToHost, e->stream));
  HIP_TRY(hipStreamSynchronize(e->stream));
  stats_flush(e);
  e->host_pos += seq;
  return 0;
}

extern "C" int cake_hip_forward_hidden(cake_engine* e, const float* x,
                                       int seq, int index_pos, float* out) {
  return cake_hip_forward_hidden_range(e, x, seq, index_pos, e ? e->lo : 0,
                                       e ? e->hi : 0, out);
}

// ---------------------------------------------------------------------------
// comm (RCCL over xGMI)
// ---------------------------------------------------------------------------
extern "C" int cake_hip_comm_id(uint8_t out[CAKE_HIP_COMM_ID_BYTES]) {
  ncclUniqueId id;
  static_assert(sizeof(ncclUniqueId) == CAKE_HIP_COMM_ID_BYTES,
                "ncclUniqueId size");
  NCCL_TRY(ncclGetUniqueId(&id));
  memcpy(out, &id, sizeof id);
  return 0;
}

extern "C" int cake_hip_comm_init(cake_engine* e, int rank, int world_size,
                                  const uint8_t id[CAKE_HIP_COMM_ID_BYTES]) {
  HIP_TRY(hipSetDevice(e->device));
  ncclUniqueId nid;
  memcpy(&nid, id, sizeof nid);
  NCCL_TRY(ncclCommInitRank(&e->comm, world_size, nid, rank));
  e->rank = rank;
  e->world = world_size;
  return 0;
}

// ---------------------------------------------------------------------------
// topology (sharding/topology.rs:134-169 + range expr 13,142-166)
// ---------------------------------------------------------------------------
static bool expand_range(const std::string& s, std::vector<int>* out) {
  // match "(.+[^\d])(\d+)-(\d+)$" (topology.rs:13)
  size_t dash = s.rfind('-');
  if (dash == std::string::npos || dash + 1 >= s.size()) return false;
  size_t e2 = dash + 1;
  for (size_t i = e2; i < s.size(); ++i)
    if (!isdigit((unsigned char)s[i])) return false;
  size_t b1 = dash;
  while (b1 > 0 && isdigit((unsigned char)s[b1 - 1])) --b1;
  if (b1 == dash || b1 == 0 || isdigit((unsigned char)s[b1 - 1]))
    return false;
  int start = atoi(s.substr(b1, dash - b1).c_str());
  int stop = atoi(s.substr(e2).c_str());
  if (stop < start) return false;
  for (int n = start; n <= stop; ++n) out->push_back(n);
  return true;
}

static int layer_index(const std::string& name) {
  // "model.layers.N" -> N
  size_t dot = name.rfind('.');
  if (dot == std::string::npos) return -1;
  for (size_t i = dot + 1; i < name.size(); ++i)
    if (!isdigit((unsigned char)name[i])) return -1;
  return atoi(name.c_str() + dot + 1);
}

extern "C" int cake_hip_topology_node_range(const char* topology_yaml,
                                            const char* node_name, int* lo,
                                            int* hi) {
  // minimal YAML subset: top-level "name:", nested "  key: value",
  // "  layers:" followed by "    - item" entries
  std::vector<int> idx;
  std::string cur_node;
  bool in_layers = false;
  bool found = false;
  const char* p = topology_yaml;
  while (*p) {
    const char* nl = strchr(p, '\n');
    std::string line = nl ? std::string(p, nl - p) : std::string(p);
    p = nl ? nl + 1 : p + line.size();
    // strip comments and trailing ws
    size_t h = line.find('#');
    if (h != std::string::npos) line = line.substr(0, h);
    while (!line.empty() && (line.back() == ' ' || line.back() == '\r'))
      line.pop_back();
    if (line.empty()) continue;
    size_t indent = 0;
    while (indent < line.size() && line[indent] == ' ') ++indent;
    std::string body = line.substr(indent);
    if (indent == 0 && body.back() == ':') {
      cur_node = body.substr(0, body.size() - 1);
      in_layers = false;
      if (cur_node == node_name) found = true;
      continue;
    }
    if (cur_node != node_name) continue;
    if (body == "layers:") {
      in_layers = true;
      continue;
    }
    if (in_layers && body.size() > 2 && body[0] == '-') {
      std::string item = body.substr(1);
      while (!item.empty() && item.front() == ' ') item.erase(0, 1);
      if (!item.empty() && (item.front() == '"' || item.front() == '\'')) {
        item = item.substr(1, item.size() - 2);
      }
      std::vector<int> nums;
      if (expand_range(item, &nums)) {
        for (int n : nums) idx.push_back(n);
      } else {
        int n = layer_index(item);
        if (n < 0) return set_err(5, "bad layer name '%s'", item.c_str());
        idx.push_back(n);
      }
      continue;
    }
    if (body.find(':') != std::string::npos) in_layers = false;
  }
  if (!found) return set_err(5, "node '%s' not in topology", node_name);
  if (idx.empty()) return set_err(5, "node '%s' has no layers", node_name);
  int mn = idx[0], mx = idx[0];
  long sum = 0;
  for (int n : idx) {
    mn = std::min(mn, n);
    mx = std::max(mx, n);
    sum += n;
  }
  long want = (long)(mn + mx) * (mx - mn + 1) / 2;
  if (sum != want || (int)idx.size() != mx - mn + 1)
    return set_err(5, "node '%s' layers are not a contiguous range",
                   node_name);
  *lo = mn;
  *hi = mx + 1;
  return 0;
}

// ---------------------------------------------------------------------------
// op-level surface (kernel parity tests)
// ---------------------------------------------------------------------------
struct OpCtx {
  u16 *a = nullptr, *b = nullptr, *c = nullptr;
  float *fa = nullptr, *fb = nullptr, *fc = nullptr;
  size_t cap = 0;
  hipStream_t s = nullptr;
};
static int op_ctx(int device, size_t elems, OpCtx* o) {
  HIP_TRY(hipSetDevice(device));
  static thread_local OpCtx ctx;
  if (ctx.cap < elems) {
    if (ctx.a) {
      hipFree(ctx.a); hipFree(ctx.b); hipFree(ctx.c);
      hipFree(ctx.fa); hipFree(ctx.fb); hipFree(ctx.fc);
    }
    ctx.cap = elems;
    ALLOC(ctx.a, u16, elems);
    ALLOC(ctx.b, u16, elems);
    ALLOC(ctx.c, u16, elems);
    ALLOC(ctx.fa, float, elems);
    ALLOC(ctx.fb, float, elems);
    ALLOC(ctx.fc, float, elems);
    HIP_TRY(hipStreamCreate(&ctx.s));
  }
  *o = ctx;
  return 0;
}
static int up16(const float* src, float* fstage, u16* dst, size_t n,
                hipStream_t s) {
  HIP_TRY(hipMemcpyAsync(fstage, src, n * 4, hipMemcpyHostToDevice, s));
  launch_f32_to_bf16(fstage, dst, n, s);
  return 0;
}
static int down16(const u16* src, float* fstage, float* dst, size_t n,
                  hipStream_t s) {
  launch_bf16_to_f32(src, fstage, n, s);
  HIP_TRY(hipMemcpyAsync(dst, fstage, n * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return 0;
}

extern "C" int cake_hip_op_rms_norm(int rows, int cols, float eps,
                                    const float* x, const float* w,
                                    float* out, int device) {
  OpCtx o;
  size_t n = (size_t)rows * cols;
  int r = op_ctx(device, std::max(n, (size_t)cols), &o);
  if (r) return r;
  if ((r = up16(x, o.fa, o.a, n, o.s))) return r;
  if ((r = up16(w, o.fb, o.b, cols, o.s))) return r;
  launch_rmsnorm(o.a, o.b, o.c, rows, cols, eps, o.s);
  return down16(o.c, o.fc, out, n, o.s);
}

extern "C" int cake_hip_op_linear(int M, int N, int K, const float* x,
                                  const float* w, float* out, int device) {
  // the bf16x8 load granularity of every linear kernel (GEMV and GEMM)
  if (K < 8 || K % 8 != 0)
    return set_err(5, "op_linear: K must be a multiple of 8 (got %d)", K);
  OpCtx o;
  size_t n = std::max((size_t)M * K, std::max((size_t)N * K, (size_t)M * N));
  int r = op_ctx(device, n, &o);
  if (r) return r;
  if ((r = up16(x, o.fa, o.a, (size_t)M * K, o.s))) return r;
  if ((r = up16(w, o.fb, o.b, (size_t)N * K, o.s))) return r;
  if (M == 1) {
    launch_gemv(o.b, o.a, o.c, nullptr, nullptr, 0.f, N, K, 0, o.s);
  } else {
    // ragged K (% 64 != 0, % 8 == 0) handled by the 128^2 kernel's masked
    // tail tile; the dispatcher keeps such shapes off the big-tile paths
    launch_gemm(o.a, o.b, o.c, nullptr, M, N, K, 0, o.s);
  }
  return down16(o.c, o.fc, out, (size_t)M * N, o.s);
}

extern "C" int cake_hip_op_silu_mul(long n, const float* gate,
                                    const float* up, float* out, int device) {
  OpCtx o;
  int r = op_ctx(device, (size_t)n, &o);
  if (r) return r;
  if ((r = up16(gate, o.fa, o.a, n, o.s))) return r;
  if ((r = up16(up, o.fb, o.b, n, o.s))) return r;
  launch_silu_mul(o.a, o.b, o.c, n, o.s);
  return down16(o.c, o.fc, out, n, o.s);
}

// rope on (B,H,S,D) f32 with cos/sin (S, D/2) — staged through bf16 like the
// product path
extern "C" int cake_hip_op_rope(int b, int h, int s, int d, const float* x,
                                const float* cosv, const float* sinv,
                                float* out, int device) {
  OpCtx o;
  size_t n = (size_t)b * h * s * d;
  int r = op_ctx(device, n + (size_t)s * d, &o);
  if (r) return r;
  if ((r = up16(x, o.fa, o.a, n, o.s))) return r;
  // cos/sin stay f32 (the product path keeps f32 tables)
  HIP_TRY(hipMemcpyAsync(o.fb, cosv, (size_t)s * d / 2 * 4,
                         hipMemcpyHostToDevice, o.s));
  HIP_TRY(hipMemcpyAsync(o.fb + (size_t)s * d / 2, sinv,
                         (size_t)s * d / 2 * 4, hipMemcpyHostToDevice, o.s));
  launch_rope_simple(o.a, o.fb, o.fb + (size_t)s * d / 2, b * h, s, d, o.s);
  return down16(o.a, o.fc, out, n, o.s);
}

// ---- attention + KV-store op entries ---------------------------------------
// Per-call buffers with exactly the engine's sizes (freed on every return
// path), the real launch wrappers on a private stream.  Arguments are
// validated before any HIP call so the error paths run without a GPU.
struct OpBufs {
  std::vector<void*> ptrs;
  hipStream_t s = nullptr;
  ~OpBufs() {
    for (void* p : ptrs) hipFree(p);
    if (s) hipStreamDestroy(s);
  }
};
static int ob_alloc(OpBufs& b, void** p, size_t bytes) {
  int r = dev_alloc(p, bytes);
  if (r) return r;
  b.ptrs.push_back(*p);
  return 0;
}
// host f32 -> fresh device bf16 buffer of n elements
static int ob_up16(OpBufs& b, const float* src, size_t n, u16** dst) {
  void *stage = nullptr, *d = nullptr;
  int r;
  if ((r = ob_alloc(b, &stage, n * 4))) return r;
  if ((r = ob_alloc(b, &d, n * 2))) return r;
  *dst = (u16*)d;
  return up16(src, (float*)stage, *dst, n, b.s);
}
static int ob_down16(OpBufs& b, const u16* src, size_t n, float* dst) {
  void* stage = nullptr;
  int r;
  if ((r = ob_alloc(b, &stage, n * 4))) return r;
  return down16(src, (float*)stage, dst, n, b.s);
}
static int ob_upf32(OpBufs& b, const void* src, size_t bytes, void** dst) {
  int r;
  if ((r = ob_alloc(b, dst, bytes))) return r;
  HIP_TRY(hipMemcpyAsync(*dst, src, bytes, hipMemcpyHostToDevice, b.s));
  return 0;
}
static int attn_geom_err(const char* who, int nh, int nkv, int hd,
                         int max_seq) {
  if (nh <= 0 || nkv <= 0 || nh % nkv != 0)
    return set_err(5, "%s: nh %d must be a positive multiple of nkv %d", who,
                   nh, nkv);
  if (hd < 8 || hd > 128 || hd % 8 != 0)
    return set_err(5, "%s: hd %d must be a multiple of 8 in [8,128]", who,
                   hd);
  if (max_seq < 32 || max_seq % 32 != 0)
    return set_err(5, "%s: max_seq %d must be a positive multiple of 32",
                   who, max_seq);
  return 0;
}

// rd of the _pr op entries: the launchers' contract
static int op_rd_err(const char* who, int hd, int rd) {
  if (rd == hd) return 0;
  if (rd <= 0 || rd > hd || rd % 4 != 0 || (hd - rd) % 4 != 0)
    return set_err(5, "%s: rd %d of hd %d: both it and the rest must be "
                   "positive multiples of 4", who, rd, hd);
  return 0;
}

// shared body of cake_hip_op_kv_store[_bias|_pr]; bias may be null; the
// tables are (max_seq, rd/2)
static int op_kv_store_impl(const char* who, int S, int pos0, int decode,
                            int nh, int nkv, int hd, int rd, int max_seq,
                            const float* qkv, const float* cosv,
                            const float* sinv, const float* q_norm,
                            const float* k_norm, float eps,
                            const float* bias, float* kc, float* vc,
                            float* vtc, float* q_out, int device) {
  int r = attn_geom_err(who, nh, nkv, hd, max_seq);
  if (r) return r;
  if (S < 1 || pos0 < 0 || pos0 + S > max_seq)
    return set_err(5, "%s: rows [%d,%d+%d) outside the cache (max_seq %d)",
                   who, pos0, pos0, S, max_seq);
  if (decode && S != 1)
    return set_err(5, "%s: the decode store takes one row (got %d)", who, S);
  if ((q_norm == nullptr) != (k_norm == nullptr))
    return set_err(5, "%s: q_norm and k_norm go together", who);
  if (bias && q_norm)
    return set_err(5, "%s: a bias together with QK-norm is not supported",
                   who);
  if ((r = op_rd_err(who, hd, rd))) return r;
  if (rd != hd && q_norm)
    return set_err(5, "%s: rd < hd together with QK-norm is not supported",
                   who);
  OpBufs b;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipStreamCreate(&b.s));
  const int Nq = (nh + 2 * nkv) * hd;
  const size_t ncache = (size_t)nkv * max_seq * hd;
  const size_t ntab = (size_t)max_seq * (rd / 2);
  u16 *dqkv, *dkc, *dvc, *dvtc, *dqn = nullptr, *dkn = nullptr;
  void *dcos, *dsin, *dpos, *dbias = nullptr;
  if ((r = ob_up16(b, qkv, (size_t)S * Nq, &dqkv))) return r;
  if (bias && (r = ob_upf32(b, bias, (size_t)Nq * 4, &dbias))) return r;
  if ((r = ob_up16(b, kc, ncache, &dkc))) return r;
  if ((r = ob_up16(b, vc, ncache, &dvc))) return r;
  if ((r = ob_up16(b, vtc, ncache, &dvtc))) return r;
  if (q_norm) {
    if ((r = ob_up16(b, q_norm, hd, &dqn))) return r;
    if ((r = ob_up16(b, k_norm, hd, &dkn))) return r;
  }
  if ((r = ob_upf32(b, cosv, ntab * 4, &dcos))) return r;
  if ((r = ob_upf32(b, sinv, ntab * 4, &dsin))) return r;
  if ((r = ob_upf32(b, &pos0, sizeof(int), &dpos))) return r;
  if (decode)
    launch_rope_store_decode(dqkv, dkc, dvc, dvtc, (const float*)dcos,
                             (const float*)dsin, (const int*)dpos, nh, nkv,
                             hd, rd, max_seq, dqn, dkn, eps, b.s,
                             (const float*)dbias);
  else
    launch_rope_store_prefill(dqkv, dkc, dvc, dvtc, (const float*)dcos,
                              (const float*)dsin, pos0, S, nh, nkv, hd, rd,
                              max_seq, Nq, dqn, dkn, eps, b.s,
                              (const float*)dbias);
  HIP_TRY(hipGetLastError());
  std::vector<float> rows((size_t)S * Nq);
  if ((r = ob_down16(b, dqkv, rows.size(), rows.data()))) return r;
  for (int i = 0; i < S; ++i)
    memcpy(q_out + (size_t)i * nh * hd, rows.data() + (size_t)i * Nq,
           sizeof(float) * nh * hd);
  if ((r = ob_down16(b, dkc, ncache, kc))) return r;
  if ((r = ob_down16(b, dvc, ncache, vc))) return r;
  return ob_down16(b, dvtc, ncache, vtc);
}
extern "C" int cake_hip_op_kv_store(int S, int pos0, int decode, int nh,
                                    int nkv, int hd, int max_seq,
                                    const float* qkv, const float* cosv,
                                    const float* sinv, const float* q_norm,
                                    const float* k_norm, float eps, float* kc,
                                    float* vc, float* vtc, float* q_out,
                                    int device) {
  return op_kv_store_impl("op_kv_store", S, pos0, decode, nh, nkv, hd, hd,
                          max_seq, qkv, cosv, sinv, q_norm, k_norm, eps,
                          nullptr, kc, vc, vtc, q_out, device);
}
extern "C" int cake_hip_op_kv_store_bias(int S, int pos0, int decode, int nh,
                                         int nkv, int hd, int max_seq,
                                         const float* qkv, const float* cosv,
                                         const float* sinv,
                                         const float* q_norm,
                                         const float* k_norm, float eps,
                                         const float* bias, float* kc,
                                         float* vc, float* vtc, float* q_out,
                                         int device) {
  return op_kv_store_impl("op_kv_store_bias", S, pos0, decode, nh, nkv, hd,
                          hd, max_seq, qkv, cosv, sinv, q_norm, k_norm, eps,
                          bias, kc, vc, vtc, q_out, device);
}
extern "C" int cake_hip_op_kv_store_pr(int S, int pos0, int decode, int nh,
                                       int nkv, int hd, int rd, int max_seq,
                                       const float* qkv, const float* cosv,
                                       const float* sinv, const float* q_norm,
                                       const float* k_norm, float eps,
                                       float* kc, float* vc, float* vtc,
                                       float* q_out, int device) {
  return op_kv_store_impl("op_kv_store_pr", S, pos0, decode, nh, nkv, hd, rd,
                          max_seq, qkv, cosv, sinv, q_norm, k_norm, eps,
                          nullptr, kc, vc, vtc, q_out, device);
}

extern "C" int cake_hip_op_attn_prefill(int S, int pos0, int nh, int nkv,
                                        int hd, int max_seq, int window,
                                        int pfv, int nw, int split, int deep,
                                        const float* q, const float* kc,
                                        const float* vc, const float* vtc,
                                        float* out, int device) {
  const char* who = "op_attn_prefill";
  int r = attn_geom_err(who, nh, nkv, hd, max_seq);
  if (r) return r;
  if (S < 1 || pos0 < 0 || pos0 + S > max_seq)
    return set_err(5, "%s: rows [%d,%d+%d) outside the cache (max_seq %d)",
                   who, pos0, pos0, S, max_seq);
  if (window < 0) return set_err(5, "%s: window %d < 0", who, window);
  // what the dispatcher can express: hd 128 -> v1, or v2 with 4|8 waves and
  // at most one of split / deep; any other hd -> the generic kernel only
  const bool ok =
      hd == 128 ? ((pfv == 1 && nw == 8 && !split && !deep) ||
                   (pfv == 2 && (nw == 4 || nw == 8) &&
                    (split == 0 || split == 1) && deep >= 0 && deep <= 2 &&
                    !(split && deep)))
                : (pfv == 0 && nw == 0 && !split && !deep);
  if (!ok)
    return set_err(5, "%s: variant {pfv %d, nw %d, split %d, deep %d} is "
                   "not dispatchable at hd %d", who, pfv, nw, split, deep,
                   hd);
  OpBufs b;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipStreamCreate(&b.s));
  const int Sq = nh * hd;
  const size_t ncache = (size_t)nkv * max_seq * hd;
  u16 *dq, *dkc, *dvc, *dvtc;
  void *dout, *dws;
  if ((r = ob_up16(b, q, (size_t)S * Sq, &dq))) return r;
  if ((r = ob_up16(b, kc, ncache, &dkc))) return r;
  if ((r = ob_up16(b, vc, ncache, &dvc))) return r;
  if ((r = ob_up16(b, vtc, ncache, &dvtc))) return r;
  if ((r = ob_alloc(b, &dout, (size_t)S * Sq * 2))) return r;
  if ((r = ob_alloc(b, &dws, (size_t)nh * S * 2 * 132 * 4))) return r;
  HIP_TRY(hipMemsetAsync(dout, 0, (size_t)S * Sq * 2, b.s));
  PfVariant v;
  v.pfv = pfv;
  v.nw = nw;
  v.split = split;
  v.deep = deep;
  v.split_min_s = 1;  // the size policy belongs to the product wrapper
  launch_attn_prefill_variant(dq, dkc, dvc, dvtc, (u16*)dout, (float*)dws, S,
                              pos0, nh, nkv, hd, max_seq, Sq, Sq, window, v,
                              b.s);
  HIP_TRY(hipGetLastError());
  return ob_down16(b, (u16*)dout, (size_t)S * Sq, out);
}

extern "C" int cake_hip_op_attn_decode(int nh, int nkv, int hd, int max_seq,
                                       int pos, int window, int nchunk,
                                       int repeats, const float* q,
                                       const float* kc, const float* vc,
                                       float* out, int device) {
  const char* who = "op_attn_decode";
  int r = attn_geom_err(who, nh, nkv, hd, max_seq);
  if (r) return r;
  if (pos < 0 || pos + 1 > max_seq)
    return set_err(5, "%s: pos %d outside the cache (max_seq %d)", who, pos,
                   max_seq);
  if (window < 0) return set_err(5, "%s: window %d < 0", who, window);
  if (nchunk < 1 || nchunk > 64)
    return set_err(5, "%s: nchunk %d outside [1,64]", who, nchunk);
  if (repeats < 1 || repeats > 16)
    return set_err(5, "%s: repeats %d outside [1,16]", who, repeats);
  OpBufs b;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipStreamCreate(&b.s));
  const int Sq = nh * hd;
  const size_t ncache = (size_t)nkv * max_seq * hd;
  u16 *dq, *dkc, *dvc;
  void *dout, *dws, *dcnt, *dpos;
  if ((r = ob_up16(b, q, Sq, &dq))) return r;
  if ((r = ob_up16(b, kc, ncache, &dkc))) return r;
  if ((r = ob_up16(b, vc, ncache, &dvc))) return r;
  if ((r = ob_alloc(b, &dout, (size_t)repeats * Sq * 2))) return r;
  if ((r = ob_alloc(b, &dws, (size_t)nh * 64 * (hd + 4) * 4))) return r;
  if ((r = ob_alloc(b, &dcnt, (size_t)nh * 4))) return r;
  if ((r = ob_upf32(b, &pos, sizeof(int), &dpos))) return r;
  HIP_TRY(hipMemsetAsync(dout, 0, (size_t)repeats * Sq * 2, b.s));
  // counters zeroed ONCE: the launches below share them back to back, as the
  // product's decode loop does (epoch-free modulo election)
  HIP_TRY(hipMemsetAsync(dcnt, 0, (size_t)nh * 4, b.s));
  for (int i = 0; i < repeats; ++i)
    launch_attn_decode(dq, dkc, dvc, (const int*)dpos, (float*)dws,
                       (u32*)dcnt, (u16*)dout + (size_t)i * Sq, nh, nkv, hd,
                       max_seq, nchunk, window, b.s);
  HIP_TRY(hipGetLastError());
  return ob_down16(b, (u16*)dout, (size_t)repeats * Sq, out);
}

// The launch choices the product makes for a shape, for the host-side
// dispatch check: out = {pfv, nw, split, deep, split_min_s, decode grid_y}.
extern "C" int cake_hip_attn_dispatch(int S, int nh, int nkv, int hd,
                                      int out[6]) {
  const PfVariant v = attn_prefill_policy(S, nh, hd);
  out[0] = v.pfv;
  out[1] = v.nw;
  out[2] = v.split;
  out[3] = v.deep;
  out[4] = v.split_min_s;
  out[5] = attn_decode_grid_y(nh, nkv, hd);
  return 0;
}

extern "C" int cake_hip_attn_decode_path(int nh, int nkv, int hd, int nchunk) {
  return attn_decode_path(nh, nkv, hd, nchunk);
}

extern "C" int cake_hip_op_attn_decode_seq(
    int nh, int nkv, int hd, int max_seq, int pos, int window, int nlaunch,
    const int* nchunks, const float* q, const float* kc, const float* vc,
    float* out, uint32_t* cnt_out, int device) {
  const char* who = "op_attn_decode_seq";
  int r = attn_geom_err(who, nh, nkv, hd, max_seq);
  if (r) return r;
  if (pos < 0 || pos + 1 > max_seq)
    return set_err(5, "%s: pos %d outside the cache (max_seq %d)", who, pos,
                   max_seq);
  if (window < 0) return set_err(5, "%s: window %d < 0", who, window);
  if (nlaunch < 1 || nlaunch > 16)
    return set_err(5, "%s: nlaunch %d outside [1,16]", who, nlaunch);
  for (int i = 0; i < nlaunch; ++i)
    if (nchunks[i] < 1 || nchunks[i] > 64)
      return set_err(5, "%s: nchunk %d outside [1,64]", who, nchunks[i]);
  OpBufs b;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipStreamCreate(&b.s));
  const int Sq = nh * hd;
  const size_t ncache = (size_t)nkv * max_seq * hd;
  u16 *dq, *dkc, *dvc;
  void *dout, *dws, *dcnt, *dpos;
  if ((r = ob_up16(b, q, Sq, &dq))) return r;
  if ((r = ob_up16(b, kc, ncache, &dkc))) return r;
  if ((r = ob_up16(b, vc, ncache, &dvc))) return r;
  if ((r = ob_alloc(b, &dout, (size_t)nlaunch * Sq * 2))) return r;
  if ((r = ob_alloc(b, &dws, (size_t)nh * 64 * (hd + 4) * 4))) return r;
  if ((r = ob_alloc(b, &dcnt, (size_t)nh * 4))) return r;
  if ((r = ob_upf32(b, &pos, sizeof(int), &dpos))) return r;
  HIP_TRY(hipMemsetAsync(dout, 0, (size_t)nlaunch * Sq * 2, b.s));
  HIP_TRY(hipMemsetAsync(dcnt, 0, (size_t)nh * 4, b.s));
  for (int i = 0; i < nlaunch; ++i)
    launch_attn_decode(dq, dkc, dvc, (const int*)dpos, (float*)dws,
                       (u32*)dcnt, (u16*)dout + (size_t)i * Sq, nh, nkv, hd,
                       max_seq, nchunks[i], window, b.s);
  HIP_TRY(hipGetLastError());
  if (cnt_out) {
    HIP_TRY(hipMemcpyAsync(cnt_out, dcnt, (size_t)nh * 4,
                           hipMemcpyDeviceToHost, b.s));
    HIP_TRY(hipStreamSynchronize(b.s));
  }
  return ob_down16(b, (u16*)dout, (size_t)nlaunch * Sq, out);
}

// ---- linear op entries (GEMV / fp8 / GEMM) ---------------------------------
// Same conventions as the attention entries.  Every output buffer carries
// CAKE_HIP_OP_GUARD extra elements past its end and is pre-filled with
// CAKE_HIP_OP_SENTINEL; the guards come back with the output so a test sees
// an out-of-range store or an element no block wrote.
static const int OPG = CAKE_HIP_OP_GUARD;
static int ob_sent16(OpBufs& b, size_t n, u16** dst) {
  void* d = nullptr;
  int r = ob_alloc(b, &d, n * 2);
  if (r) return r;
  *dst = (u16*)d;
  launch_fill_const(*dst, n, CAKE_HIP_OP_SENTINEL, b.s);
  return 0;
}
static int ob_sent32(OpBufs& b, size_t n, float** dst) {
  std::vector<float> h(n, CAKE_HIP_OP_SENTINEL);
  void* d = nullptr;
  int r = ob_upf32(b, h.data(), n * 4, &d);
  if (r) return r;
  HIP_TRY(hipStreamSynchronize(b.s));  // h dies with this frame
  *dst = (float*)d;
  return 0;
}
static int ob_downf32(OpBufs& b, const void* src, size_t bytes, void* dst) {
  HIP_TRY(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, b.s));
  HIP_TRY(hipStreamSynchronize(b.s));
  return 0;
}
static int fp8_shape_err(const char* who, int N, int K) {
  if (N < 128 || K < 128 || N % 128 != 0 || K % 128 != 0)
    return set_err(5, "%s: fp8 weights need N %% 128 == 0 and K %% 128 == 0 "
                   "(got %d x %d)", who, N, K);
  return 0;
}

extern "C" int cake_hip_op_gemv(int kind, int N, int K, int epi, int rows,
                                int alias, int repeats, const float* x,
                                const float* w, const uint8_t* w8,
                                const float* sc, const float* res,
                                const float* nw, float eps, int chain,
                                const uint32_t* cnt_init,
                                const float* scale_in, float* scale_out,
                                float* out, int device) {
  const char* who = "op_gemv";
  if (kind < 0 || kind > 2) return set_err(5, "%s: kind %d", who, kind);
  if (N < 1) return set_err(5, "%s: N %d < 1", who, N);
  if (K < 8 || K % 8 != 0)
    return set_err(5, "%s: K must be a positive multiple of 8 (got %d)", who,
                   K);
  if (repeats < 1 || repeats > 16)
    return set_err(5, "%s: repeats %d outside [1,16]", who, repeats);
  if (epi < 0 || epi > 2) return set_err(5, "%s: epi %d", who, epi);
  if (!x || !out) return set_err(5, "%s: x and out are required", who);
  if (kind == 1) {
    int r = fp8_shape_err(who, N, K);
    if (r) return r;
    if (!w8 || !sc) return set_err(5, "%s: fp8 needs w8 and sc", who);
    if (rows != 0 && rows != 4 && rows != 8)
      return set_err(5, "%s: fp8 rows %d not in {0,4,8}", who, rows);
  } else {
    if (!w) return set_err(5, "%s: bf16 needs w", who);
    if (kind == 0 && rows != 0 && rows != 1 && rows != 2 && rows != 4 &&
        rows != 8)
      return set_err(5, "%s: rows %d not in {0,1,2,4,8}", who, rows);
  }
  if (kind == 2) {
    if (K % 16 != 0)
      return set_err(5, "%s: split-K needs K %% 16 == 0 (got %d)", who, K);
    if (epi != 1 || nw || rows != 0 || chain)
      return set_err(5, "%s: split-K is the residual epilogue only (epi 1, "
                     "no norm, no rows override, no chain)", who);
    if (!cnt_init) return set_err(5, "%s: split-K needs cnt_init", who);
  }
  if (nw && K > 16384)
    return set_err(5, "%s: the streaming kernels (K > 16384) have no norm",
                   who);
  if ((epi == 1) != (res != nullptr))
    return set_err(5, "%s: res goes with epi 1", who);
  if (alias && epi != 1)
    return set_err(5, "%s: alias needs the residual epilogue", who);
  if (chain < 0 || chain > 2 || (chain && kind != 1))
    return set_err(5, "%s: the norm chain is fp8 only (chain %d)", who,
                   chain);
  if (chain == 1 && (epi != 1 || !cnt_init || !scale_out || nw))
    return set_err(5, "%s: chain produce needs epi 1, cnt_init[9], "
                   "scale_out and no fused norm", who);
  if (chain == 2 && (!scale_in || !nw))
    return set_err(5, "%s: chain consume needs scale_in and the norm row",
                   who);
  OpBufs b;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipStreamCreate(&b.s));
  int r;
  const size_t ld = (size_t)N + OPG;  // out row stride per repeat
  u16 *dx, *dw = nullptr, *dres = nullptr, *dnw = nullptr, *dout16 = nullptr;
  float* dout32 = nullptr;
  void *dw8 = nullptr, *dsc = nullptr;
  if ((r = ob_up16(b, x, (size_t)repeats * K, &dx))) return r;
  if (kind == 1) {
    if ((r = ob_upf32(b, w8, (size_t)N * K, &dw8))) return r;
    if ((r = ob_upf32(b, sc, (size_t)(N / 128) * (K / 128) * 4, &dsc)))
      return r;
  } else {
    if ((r = ob_up16(b, w, (size_t)N * K, &dw))) return r;
  }
  if (nw && (r = ob_up16(b, nw, K, &dnw))) return r;
  if (epi == 2) {
    if ((r = ob_sent32(b, repeats * ld, &dout32))) return r;
  } else {
    if ((r = ob_sent16(b, repeats * ld, &dout16))) return r;
  }
  if (res) {
    // residual rows at the out stride, so alias can copy them in place
    std::vector<float> h(repeats * ld, CAKE_HIP_OP_SENTINEL);
    for (int i = 0; i < repeats; ++i)
      memcpy(h.data() + i * ld, res + (size_t)i * N, sizeof(float) * N);
    if ((r = ob_up16(b, h.data(), h.size(), &dres))) return r;
    HIP_TRY(hipStreamSynchronize(b.s));
    if (alias) dout16 = dres;  // out == res, as the engine does with e->x
  }
  void *dws = nullptr, *dcnt = nullptr, *dpart = nullptr, *dsin = nullptr;
  float* dsout = nullptr;
  if (kind == 2) {
    const size_t nc = (size_t)(N + 1) / 2;
    std::vector<uint32_t> h(nc, cnt_init[0]);
    if ((r = ob_alloc(b, &dws, (size_t)N * 2 * 4))) return r;
    if ((r = ob_upf32(b, h.data(), nc * 4, &dcnt))) return r;
    HIP_TRY(hipStreamSynchronize(b.s));
  }
  if (chain == 1) {
    if ((r = ob_alloc(b, &dpart, (size_t)N * 4))) return r;
    if ((r = ob_upf32(b, cnt_init, 9 * 4, &dcnt))) return r;
    if ((r = ob_sent32(b, repeats, &dsout))) return r;
  }
  if (chain == 2 && (r = ob_upf32(b, scale_in, 4, &dsin))) return r;
  for (int i = 0; i < repeats; ++i) {
    const u16* xi = dx + (size_t)i * K;
    const u16* ri = dres ? dres + i * ld : nullptr;
    void* oi = epi == 2 ? (void*)(dout32 + i * ld) : (void*)(dout16 + i * ld);
    if (kind == 0) {
      launch_gemv(dw, xi, oi, ri, dnw, eps, N, K, epi, b.s, rows);
    } else if (kind == 2) {
      launch_gemv_res_splitk(dw, xi, (u16*)oi, ri, (float*)dws, (u32*)dcnt,
                             N, K, b.s);
    } else {
      NormIO nio{};
      if (chain == 1) {
        nio.part = (float*)dpart;
        nio.cnt = (u32*)dcnt;
        nio.scale_out = dsout + i;
        nio.eps = eps;
      } else if (chain == 2) {
        nio.scale_in = (const float*)dsin;
        nio.nw = dnw;
      }
      launch_gemv_fp8((const unsigned char*)dw8, (const float*)dsc, xi, oi,
                      ri, chain == 2 ? nullptr : dnw, eps, N, K, epi, b.s,
                      nio, rows);
    }
  }
  HIP_TRY(hipGetLastError());
  if (chain == 1 &&
      (r = ob_downf32(b, dsout, (size_t)repeats * 4, scale_out)))
    return r;
  if (epi == 2) return ob_downf32(b, dout32, repeats * ld * 4, out);
  return ob_down16(b, dout16, repeats * ld, out);
}

extern "C" int cake_hip_op_gemv_gateup(int fp8, int I, int K, int rows,
                                       const float* x, const float* w,
                                       const uint8_t* w8, const float* sc,
                                       const float* nw, float eps,
                                       const float* scale_in, float* out,
                                       int device) {
  const char* who = "op_gemv_gateup";
  if (I < 1) return set_err(5, "%s: I %d < 1", who, I);
  if (K < 8 || K % 8 != 0 || K > 16384)
    return set_err(5, "%s: K must be a multiple of 8 in [8,16384] (got %d)",
                   who, K);
  if (!x || !out) return set_err(5, "%s: x and out are required", who);
  if (fp8) {
    int r = fp8_shape_err(who, I, K);  // I % 128 keeps gate/up blocks apart
    if (r) return r;
    if (!w8 || !sc) return set_err(5, "%s: fp8 needs w8 and sc", who);
    if (rows != 0 && rows != 4)
      return set_err(5, "%s: the fp8 kernel has 4 rows per block", who);
    if (scale_in && !nw)
      return set_err(5, "%s: chain consume needs the norm row", who);
  } else {
    if (!w) return set_err(5, "%s: bf16 needs w", who);
    if (rows != 0 && rows != 4 && rows != 8)
      return set_err(5, "%s: rows %d not in {0,4,8}", who, rows);
    if (scale_in) return set_err(5, "%s: the norm chain is fp8 only", who);
  }
  OpBufs b;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipStreamCreate(&b.s));
  int r;
  u16 *dx, *dw = nullptr, *dnw = nullptr, *dout;
  void *dw8 = nullptr, *dsc = nullptr, *dsin = nullptr;
  if ((r = ob_up16(b, x, K, &dx))) return r;
  if (nw && (r = ob_up16(b, nw, K, &dnw))) return r;
  if ((r = ob_sent16(b, (size_t)I + OPG, &dout))) return r;
  if (fp8) {
    if ((r = ob_upf32(b, w8, (size_t)2 * I * K, &dw8))) return r;
    if ((r = ob_upf32(b, sc, (size_t)(2 * I / 128) * (K / 128) * 4, &dsc)))
      return r;
    NormIO nio{};
    if (scale_in) {
      if ((r = ob_upf32(b, scale_in, 4, &dsin))) return r;
      nio.scale_in = (const float*)dsin;
      nio.nw = dnw;
    }
    launch_gemv_gateup_fp8((const unsigned char*)dw8, (const float*)dsc, dx,
                           dout, scale_in ? nullptr : dnw, eps, I, K, b.s,
                           nio);
  } else {
    if ((r = ob_up16(b, w, (size_t)2 * I * K, &dw))) return r;
    launch_gemv_gateup(dw, dx, dout, dnw, eps, I, K, rows, b.s);
  }
  HIP_TRY(hipGetLastError());
  return ob_down16(b, dout, (size_t)I + OPG, out);
}

// shared body of cake_hip_op_gemv_qkv_rope[_bias|_pr]; bias may be null; the
// tables are (max_seq, rd/2)
static int op_gemv_qkv_rope_impl(const char* who, int nh, int nkv, int hd,
                                 int rd, int max_seq, int pos, int K,
                                 const float* x, const float* nw, float eps, const float* w,
                                 const float* cosv, const float* sinv,
                                 const float* bias, float* kc, float* vc,
                                 float* vtc, float* out, int device) {
  int r = attn_geom_err(who, nh, nkv, hd, max_seq);
  if (r) return r;
  if (pos < 0 || pos >= max_seq)
    return set_err(5, "%s: pos %d outside the cache (max_seq %d)", who, pos,
                   max_seq);
  if (K < 8 || K % 8 != 0)
    return set_err(5, "%s: K must be a positive multiple of 8 (got %d)", who,
                   K);
  if (!x || !nw || !w || !out)
    return set_err(5, "%s: x, nw, w and out are required", who);
  if ((r = op_rd_err(who, hd, rd))) return r;
  OpBufs b;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipStreamCreate(&b.s));
  const int Nq = (nh + 2 * nkv) * hd;
  const size_t ncache = (size_t)nkv * max_seq * hd;
  const size_t ntab = (size_t)max_seq * (rd / 2);
  u16 *dx, *dnw, *dw, *dkc, *dvc, *dvtc, *dout;
  void *dcos, *dsin, *dpos, *dbias = nullptr;
  if ((r = ob_up16(b, x, K, &dx))) return r;
  if (bias && (r = ob_upf32(b, bias, (size_t)Nq * 4, &dbias))) return r;
  if ((r = ob_up16(b, nw, K, &dnw))) return r;
  if ((r = ob_up16(b, w, (size_t)Nq * K, &dw))) return r;
  if ((r = ob_up16(b, kc, ncache, &dkc))) return r;
  if ((r = ob_up16(b, vc, ncache, &dvc))) return r;
  if ((r = ob_up16(b, vtc, ncache, &dvtc))) return r;
  if ((r = ob_upf32(b, cosv, ntab * 4, &dcos))) return r;
  if ((r = ob_upf32(b, sinv, ntab * 4, &dsin))) return r;
  if ((r = ob_upf32(b, &pos, sizeof(int), &dpos))) return r;
  // the whole qkv activation row + guards: only the q part may be written
  if ((r = ob_sent16(b, (size_t)Nq + OPG, &dout))) return r;
  launch_gemv_qkv_rope(dw, dx, dout, dnw, eps, dkc, dvc, dvtc,
                       (const float*)dcos, (const float*)dsin,
                       (const int*)dpos, nh, nkv, hd, rd, max_seq, K, b.s,
                       (const float*)dbias);
  HIP_TRY(hipGetLastError());
  if ((r = ob_down16(b, dout, (size_t)Nq + OPG, out))) return r;
  if ((r = ob_down16(b, dkc, ncache, kc))) return r;
  if ((r = ob_down16(b, dvc, ncache, vc))) return r;
  return ob_down16(b, dvtc, ncache, vtc);
}
extern "C" int cake_hip_op_gemv_qkv_rope(int nh, int nkv, int hd, int max_seq,
                                         int pos, int K, const float* x,
                                         const float* nw, float eps,
                                         const float* w, const float* cosv,
                                         const float* sinv, float* kc,
                                         float* vc, float* vtc, float* out,
                                         int device) {
  return op_gemv_qkv_rope_impl("op_gemv_qkv_rope", nh, nkv, hd, hd, max_seq,
                               pos, K, x, nw, eps, w, cosv, sinv, nullptr, kc, vc,
                               vtc, out, device);
}
extern "C" int cake_hip_op_gemv_qkv_rope_bias(
    int nh, int nkv, int hd, int max_seq, int pos, int K, const float* x,
    const float* nw, float eps, const float* w, const float* cosv,
    const float* sinv, const float* bias, float* kc, float* vc, float* vtc,
    float* out, int device) {
  return op_gemv_qkv_rope_impl("op_gemv_qkv_rope_bias", nh, nkv, hd, hd,
                               max_seq, pos, K, x, nw, eps, w, cosv, sinv,
                               bias, kc, vc, vtc, out, device);
}
extern "C" int cake_hip_op_gemv_qkv_rope_pr(
    int nh, int nkv, int hd, int rd, int max_seq, int pos, int K,
    const float* x, const float* nw, float eps, const float* w,
    const float* cosv, const float* sinv, float* kc, float* vc, float* vtc,
    float* out, int device) {
  return op_gemv_qkv_rope_impl("op_gemv_qkv_rope_pr", nh, nkv, hd, rd,
                               max_seq, pos, K, x, nw, eps, w, cosv, sinv,
                               nullptr, kc, vc, vtc, out, device);
}

extern "C" int cake_hip_op_gemm(int variant, int M, int N, int K, int epi,
                                int alias, const float* a, const float* w,
                                const float* res, float* out, int* ran,
                                int device) {
  const char* who = "op_gemm";
  if (variant < GEMM_V128 || variant > GEMM_VLIB)
    return set_err(5, "%s: variant %d outside [0,4]", who, variant);
  if (M < 1 || N < 1) return set_err(5, "%s: M %d, N %d", who, M, N);
  if (K < 8 || K % 8 != 0)
    return set_err(5, "%s: K must be a positive multiple of 8 (got %d)", who,
                   K);
  // the three pipelined big-tile kernels step K in whole 64-wide tiles;
  // their prologues and tail waits are correct for any tile count >= 1
  if (variant >= GEMM_V256 && variant <= GEMM_V256P && K % 64 != 0)
    return set_err(5, "%s: variant %d needs K %% 64 == 0 (got %d)", who,
                   variant, K);
  if (epi < 0 || epi > 1) return set_err(5, "%s: epi %d", who, epi);
  if ((epi == 1) != (res != nullptr))
    return set_err(5, "%s: res goes with epi 1", who);
  if (alias && epi != 1)
    return set_err(5, "%s: alias needs the residual epilogue", who);
  if (!a || !w || !out || !ran)
    return set_err(5, "%s: a, w, out and ran are required", who);
  OpBufs b;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipStreamCreate(&b.s));
  int r;
  const size_t n = (size_t)M * N;
  u16 *da, *dw, *dres = nullptr, *dout = nullptr;
  if ((r = ob_up16(b, a, (size_t)M * K, &da))) return r;
  if ((r = ob_up16(b, w, (size_t)N * K, &dw))) return r;
  if (res) {
    std::vector<float> h(n + OPG, CAKE_HIP_OP_SENTINEL);
    memcpy(h.data(), res, n * sizeof(float));
    if ((r = ob_up16(b, h.data(), h.size(), &dres))) return r;
    HIP_TRY(hipStreamSynchronize(b.s));
  }
  if (alias) dout = dres;  // C == res, as the engine's o/down projections
  else if ((r = ob_sent16(b, n + OPG, &dout))) return r;
  const bool ok = launch_gemm_variant(da, dw, dout, dres, M, N, K, epi,
                                      variant, b.s);
  HIP_TRY(hipGetLastError());
  *ran = ok ? variant : -1;  // -1: the library rejected the shape
  return ob_down16(b, dout, n + OPG, out);
}

extern "C" int cake_hip_op_dequant_fp8(int N, int K, const uint8_t* w8,
                                       const float* sc, float* out,
                                       int device) {
  const char* who = "op_dequant_fp8";
  int r = fp8_shape_err(who, N, K);
  if (r) return r;
  if (!w8 || !sc || !out)
    return set_err(5, "%s: w8, sc and out are required", who);
  OpBufs b;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipStreamCreate(&b.s));
  const size_t n = (size_t)N * K;
  void *dw8, *dsc;
  u16* dout;
  if ((r = ob_upf32(b, w8, n, &dw8))) return r;
  if ((r = ob_upf32(b, sc, (size_t)(N / 128) * (K / 128) * 4, &dsc)))
    return r;
  if ((r = ob_sent16(b, n + OPG, &dout))) return r;
  launch_dequant_fp8((const unsigned char*)dw8, (const float*)dsc, dout, N, K,
                     b.s);
  HIP_TRY(hipGetLastError());
  return ob_down16(b, dout, n + OPG, out);
}

// ---- 4-bit (gptq) op entries: tensors arrive in CHECKPOINT layout and go
// through w4_repack, the loader's own routine, so the tests cover the repack
// together with the kernels
static int w4_op_upload(OpBufs& b, const char* who, int N, int K, int group,
                        const int32_t* qweight, const int32_t* qzeros,
                        const float* scales, u32** dW, float** dsz) {
  const size_t G = (size_t)K / group;
  std::vector<u32> W((size_t)N * (K / 8));
  std::vector<float> sz((size_t)N * G * 2);
  w4_repack(qweight, qzeros, scales, N, K, group, W.data(), sz.data());
  void *pw, *ps;
  int r;
  if ((r = ob_upf32(b, W.data(), W.size() * 4, &pw))) return r;
  if ((r = ob_upf32(b, sz.data(), sz.size() * 4, &ps))) return r;
  HIP_TRY(hipStreamSynchronize(b.s));  // the staging vectors die here
  *dW = (u32*)pw;
  *dsz = (float*)ps;
  (void)who;
  return 0;
}
static int w4_op_args(const char* who, int N, int K, int group,
                      const void* qweight, const void* qzeros,
                      const void* scales, const void* out) {
  int r = w4_dim_err(who, N, K, group);
  if (r) return r;
  if (!qweight || !qzeros || !scales || !out)
    return set_err(5, "%s: qweight, qzeros, scales and out are required",
                   who);
  return 0;
}

extern "C" int cake_hip_op_gemv_w4(int N, int K, int group, int epi, int rows,
                                   int alias, int repeats, const float* x,
                                   const int32_t* qweight,
                                   const int32_t* qzeros, const float* scales,
                                   const float* res, float* out, int device) {
  const char* who = "op_gemv_w4";
  int r = w4_op_args(who, N, K, group, qweight, qzeros, scales, out);
  if (r) return r;
  if (!x) return set_err(5, "%s: x is required", who);
  if (repeats < 1 || repeats > 16)
    return set_err(5, "%s: repeats %d outside [1,16]", who, repeats);
  if (epi < 0 || epi > 1) return set_err(5, "%s: epi %d", who, epi);
  if (rows != 0 && rows != 4 && rows != 8)
    return set_err(5, "%s: rows %d not in {0,4,8}", who, rows);
  if (rows == 8 && gemv_w4_kb(K) == 8)
    return set_err(5, "%s: rows 8 needs K <= 16384 (got %d)", who, K);
  if ((epi == 1) != (res != nullptr))
    return set_err(5, "%s: res goes with epi 1", who);
  if (alias && epi != 1)
    return set_err(5, "%s: alias needs the residual epilogue", who);
  OpBufs b;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipStreamCreate(&b.s));
  const size_t ld = (size_t)N + OPG;  // out row stride per repeat
  u16 *dx, *dres = nullptr, *dout = nullptr;
  u32* dW;
  float* dsz;
  if ((r = ob_up16(b, x, (size_t)repeats * K, &dx))) return r;
  if ((r = w4_op_upload(b, who, N, K, group, qweight, qzeros, scales, &dW,
                        &dsz)))
    return r;
  if ((r = ob_sent16(b, repeats * ld, &dout))) return r;
  if (res) {
    // residual rows at the out stride, so alias can copy them in place
    std::vector<float> h(repeats * ld, CAKE_HIP_OP_SENTINEL);
    for (int i = 0; i < repeats; ++i)
      memcpy(h.data() + i * ld, res + (size_t)i * N, sizeof(float) * N);
    if ((r = ob_up16(b, h.data(), h.size(), &dres))) return r;
    HIP_TRY(hipStreamSynchronize(b.s));
    if (alias) dout = dres;  // out == res, as the engine does with e->x
  }
  for (int i = 0; i < repeats; ++i)
    launch_gemv_w4(dW, dsz, dx + (size_t)i * K, dout + i * ld,
                   dres ? dres + i * ld : nullptr, N, K, group, epi, b.s,
                   rows);
  HIP_TRY(hipGetLastError());
  return ob_down16(b, dout, repeats * ld, out);
}

extern "C" int cake_hip_op_gemv_gateup_w4(int I, int K, int group, int rows,
                                          const float* x,
                                          const int32_t* qweight,
                                          const int32_t* qzeros,
                                          const float* scales, float* out,
                                          int device) {
  const char* who = "op_gemv_gateup_w4";
  if (I < 8 || I % 8 != 0)
    return set_err(5, "%s: I %d is not a positive multiple of 8", who, I);
  int r = w4_op_args(who, 2 * I, K, group, qweight, qzeros, scales, out);
  if (r) return r;
  if (K > 16384)
    return set_err(5, "%s: K must be <= 16384 (got %d)", who, K);
  if (!x) return set_err(5, "%s: x is required", who);
  if (rows != 0 && rows != 4)
    return set_err(5, "%s: the 4-bit gate-up kernel has 4 rows per block",
                   who);
  OpBufs b;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipStreamCreate(&b.s));
  u16 *dx, *dout;
  u32* dW;
  float* dsz;
  if ((r = ob_up16(b, x, K, &dx))) return r;
  if ((r = w4_op_upload(b, who, 2 * I, K, group, qweight, qzeros, scales,
                        &dW, &dsz)))
    return r;
  if ((r = ob_sent16(b, (size_t)I + OPG, &dout))) return r;
  launch_gemv_gateup_w4(dW, dsz, dx, dout, I, K, group, b.s);
  HIP_TRY(hipGetLastError());
  return ob_down16(b, dout, (size_t)I + OPG, out);
}

extern "C" int cake_hip_op_dequant_w4(int N, int K, int group,
                                      const int32_t* qweight,
                                      const int32_t* qzeros,
                                      const float* scales, float* out,
                                      int device) {
  const char* who = "op_dequant_w4";
  int r = w4_op_args(who, N, K, group, qweight, qzeros, scales, out);
  if (r) return r;
  OpBufs b;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipStreamCreate(&b.s));
  const size_t n = (size_t)N * K;
  u32* dW;
  float* dsz;
  u16* dout;
  if ((r = w4_op_upload(b, who, N, K, group, qweight, qzeros, scales, &dW,
                        &dsz)))
    return r;
  if ((r = ob_sent16(b, n + OPG, &dout))) return r;
  launch_dequant_w4(dW, dsz, dout, N, K, group, b.s);
  HIP_TRY(hipGetLastError());
  return ob_down16(b, dout, n + OPG, out);
}

extern "C" int cake_hip_op_silu_mul_rows(int S, int I, const float* gu,
                                         float* out, int device) {
  const char* who = "op_silu_mul_rows";
  if (S < 1 || I < 8 || I % 8 != 0)
    return set_err(5, "%s: S %d >= 1 and I %d a positive multiple of 8", who,
                   S, I);
  if (!gu || !out) return set_err(5, "%s: gu and out are required", who);
  OpBufs b;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipStreamCreate(&b.s));
  int r;
  u16 *dgu, *dout;
  if ((r = ob_up16(b, gu, (size_t)S * 2 * I, &dgu))) return r;
  if ((r = ob_sent16(b, (size_t)S * I + OPG, &dout))) return r;
  launch_silu_mul_rows(dgu, dout, S, I, b.s);
  HIP_TRY(hipGetLastError());
  return ob_down16(b, dout, (size_t)S * I + OPG, out);
}

extern "C" int cake_hip_op_rms_norm_rows(int outer, int inner,
                                         long outer_stride, int cols,
                                         float eps, long n, const float* x,
                                         const float* w, float* out,
                                         int device) {
  const char* who = "op_rms_norm_rows";
  if (outer < 1 || inner < 1 || cols < 1)
    return set_err(5, "%s: outer %d, inner %d, cols %d", who, outer, inner,
                   cols);
  // rows may not overlap, x is read and out written with 16-B vectors
  if (outer_stride < (long)inner * cols || outer_stride % 8 != 0 ||
      cols % 8 != 0)
    return set_err(5, "%s: outer_stride %ld must be a multiple of 8 >= "
                   "inner * cols, cols %d a multiple of 8", who, outer_stride,
                   cols);
  if (n != (long)(outer - 1) * outer_stride + (long)inner * cols)
    return set_err(5, "%s: buffer of %ld elements, rows end at %ld", who, n,
                   (long)(outer - 1) * outer_stride + (long)inner * cols);
  if (!x || !w || !out) return set_err(5, "%s: x, w, out are required", who);
  OpBufs b;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipStreamCreate(&b.s));
  int r;
  u16 *dx, *dw, *dout;
  if ((r = ob_up16(b, x, (size_t)n, &dx))) return r;
  if ((r = ob_up16(b, w, cols, &dw))) return r;
  if ((r = ob_sent16(b, (size_t)n + OPG, &dout))) return r;
  launch_rmsnorm_strided(dx, dw, dout, outer, inner, (size_t)outer_stride,
                         cols, eps, b.s);
  HIP_TRY(hipGetLastError());
  return ob_down16(b, dout, (size_t)n + OPG, out);
}

// The five linear launches of one decode step of this model, by the very
// predicates enqueue_layer_decode and enqueue_head_sample use (host only):
// out[i] = {family, rows, KB} for i = qkv, o, gate-up, down, head.  The
// opt-in split-K residual GEMV (CAKE_GEMV_SPLITK) is not reflected.
static void plain_dispatch(int N, int K, int quant, int* o) {
  if (quant == 2) {  // gptq 4-bit: one register family, K <= 32768
    o[0] = CAKE_HIP_FAM_GEMV_W4;
    o[1] = gemv_w4_rows_policy(N, K);
    o[2] = gemv_w4_kb(K);
  } else if (quant == 1) {
    o[2] = gemv_fp8_kb(K);
    o[0] = o[2] ? CAKE_HIP_FAM_GEMV_FP8 : CAKE_HIP_FAM_GEMV_FP8_STREAM;
    o[1] = gemv_fp8_rows_policy(N);
  } else {
    o[2] = gemv_kb(K);
    o[0] = o[2] ? CAKE_HIP_FAM_GEMV_REG : CAKE_HIP_FAM_GEMV_STREAM;
    o[1] = gemv_rows_policy(N, K);
  }
}
extern "C" int cake_hip_decode_dispatch(const char* config_json,
                                        int out[15]) {
  ModelConfig c;
  int r = parse_config(config_json, &c);
  if (r) return r;
  const int H = c.hidden, I = c.inter;
  if (c.w4 && (r = w4_config_err(c))) return r;
  const int quant = c.w4 ? 2 : c.fp8 ? 1 : 0;
  if (fused_qkv_rope_applies(c)) {
    out[0] = CAKE_HIP_FAM_QKV_ROPE;
    out[1] = 4;
    out[2] = gemv_qkv_rope_kb(H);
  } else {
    plain_dispatch(c.nqkv(), H, quant, out);
  }
  plain_dispatch(H, c.sq(), quant, out + 3);
  out[6] = c.w4 ? CAKE_HIP_FAM_GATEUP_W4
                : c.fp8 ? CAKE_HIP_FAM_GATEUP_FP8 : CAKE_HIP_FAM_GATEUP;
  out[7] = c.w4 || c.fp8 ? 4 : gemv_gateup_rows_policy();
  out[8] = c.w4 ? gemv_w4_kb(H) : c.fp8 ? gemv_fp8_kb(H) : gemv_kb(H);
  plain_dispatch(H, I, quant, out + 9);
  plain_dispatch(c.vocab, H, 0, out + 12);  // lm_head stays bf16
  return 0;
}

// The kernel choices the product makes for a linear layer (host only).
// kind: 0 plain GEMV, 1 gate-up GEMV, 2 fused qkv-rope GEMV, 3 split-K
// residual GEMV, 4 prefill GEMM.  out = {family, rows, KB (0 = streaming
// kernel), library first, hand-written GEMM variant}.
extern "C" int cake_hip_linear_dispatch(int kind, int n, int K, int M,
                                        int fp8, int out[5]) {
  if (kind < 0 || kind > 4 || n < 1 || K < 1 || M < 1)
    return set_err(5, "linear_dispatch: kind %d, n %d, K %d, M %d", kind, n,
                   K, M);
  if (fp8 < 0 || fp8 > 1)  // the quant selector: 0 bf16, 1 fp8; w4 needs a
                           // group size: cake_hip_linear_dispatch_w4
    return set_err(5, "linear_dispatch: quant %d (4-bit goes through "
                   "cake_hip_linear_dispatch_w4)", fp8);
  if (fp8 && kind >= 2)
    return set_err(5, "linear_dispatch: kind %d has no fp8 kernel", kind);
  out[0] = out[1] = out[2] = out[3] = out[4] = 0;
  switch (kind) {
    case 0:
      plain_dispatch(n, K, fp8, out);
      break;
    case 1:
      if (K > 16384)
        return set_err(5, "linear_dispatch: gate-up needs K <= 16384");
      out[0] = fp8 ? CAKE_HIP_FAM_GATEUP_FP8 : CAKE_HIP_FAM_GATEUP;
      out[1] = fp8 ? 4 : gemv_gateup_rows_policy();
      out[2] = fp8 ? gemv_fp8_kb(K) : gemv_kb(K);
      break;
    case 2:
      out[0] = CAKE_HIP_FAM_QKV_ROPE;
      out[1] = 4;
      out[2] = gemv_qkv_rope_kb(K);
      break;
    case 3:
      out[0] = CAKE_HIP_FAM_SPLITK;
      out[1] = 2;
      out[2] = gemv_splitk_kb(K);
      break;
    default: {
      const GemmPolicy p = gemm_policy(M, n, K);
      out[0] = CAKE_HIP_FAM_GEMM;
      out[3] = p.lib_first ? 1 : 0;
      out[4] = p.variant;
    }
  }
  return 0;
}

// The 4-bit twin: kind 0 plain GEMV (n = N), 1 gate-up GEMV (n = I).
extern "C" int cake_hip_linear_dispatch_w4(int kind, int n, int K, int group,
                                           int out[5]) {
  if (kind < 0 || kind > 1 || n < 1)
    return set_err(5, "linear_dispatch_w4: kind %d, n %d", kind, n);
  int r = w4_dim_err(kind ? "gate-up" : "gemv", n, K, group < 0 ? K : group);
  if (r) return r;
  out[0] = out[1] = out[2] = out[3] = out[4] = 0;
  if (kind == 0) {
    plain_dispatch(n, K, 2, out);
  } else {
    if (K > 16384)
      return set_err(5, "linear_dispatch_w4: gate-up needs K <= 16384");
    out[0] = CAKE_HIP_FAM_GATEUP_W4;
    out[1] = 4;
    out[2] = gemv_w4_kb(K);
  }
  return 0;
}

// ---------------------------------------------------------------------------
// stats / misc
// ---------------------------------------------------------------------------
// Sampling config (create_logits_processor, text_model.rs:102-118):
// temperature <= 0 -> greedy ArgMax; > 0 -> Gumbel-argmax at that
// temperature.  Changing it invalidates a captured decode graph.
static int apply_sampling(cake_engine* e, float temperature, int top_k,
                          float top_p, float repeat_penalty,
                          int repeat_last_n, uint64_t seed) {
  const int V = e->c.vocab;
  const bool k_on = top_k > 0 && top_k < V;
  const bool p_on = top_p > 0.f && top_p < 1.f;
  const bool pen_on = repeat_penalty != 1.f && repeat_last_n > 0;
  const bool ex = pen_on || (temperature > 0.f && (k_on || p_on));
  if (ex && !e->sample_mem)
    return set_err(5, "top-k/top-p/repeat-penalty sampling needs the head "
                   "on this engine and vocab <= %d", SAMPLE_MAX_V);
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->inv_temp = temperature > 0.f ? 1.0f / temperature : 0.f;
  e->sample_seed = seed;
  e->top_k = top_k;
  e->top_p = top_p;
  e->repeat_penalty = repeat_penalty;
  e->repeat_last_n = repeat_last_n;
  e->sample_ex = ex;
  // a new configuration starts a new draw sequence and an empty history
  if (e->sample_mem) HIP_TRY(hipMemset(e->sws.state, 0, 4 * 4));
  if (e->graph) {
    hipGraphExecDestroy(e->graph);
    e->graph = nullptr;
  }
  if (e->pf_graph) {  // inv_temp/seed are baked into the head-sample node
    hipGraphExecDestroy(e->pf_graph);
    e->pf_graph = nullptr;
    e->pf_graph_S = -1;
  }
  return 0;
}
extern "C" int cake_hip_set_sampling(cake_engine* e, float temperature,
                                     uint64_t seed) {
  return apply_sampling(e, temperature, 0, 1.f, 1.f, 0, seed);
}
static int sampling_args_err(const char* who, float temperature, float top_p,
                             float repeat_penalty) {
  if (std::isnan(temperature) || std::isnan(top_p) ||
      std::isnan(repeat_penalty))
    return set_err(5, "%s: NaN argument", who);
  if (!(repeat_penalty > 0.f))
    return set_err(5, "%s: repeat_penalty %g must be > 0", who,
                   repeat_penalty);
  return 0;
}
// The rest of create_logits_processor (text_model.rs:102-118) plus the
// repeat penalty (text_model.rs:433-452), all on the device.  With every
// option off this IS cake_hip_set_sampling(temperature, seed).
extern "C" int cake_hip_set_sampling_ex(cake_engine* e, float temperature,
                                        int top_k, float top_p,
                                        float repeat_penalty,
                                        int repeat_last_n, uint64_t seed) {
  int r = sampling_args_err("set_sampling_ex", temperature, top_p,
                            repeat_penalty);
  if (r) return r;
  if (repeat_last_n < 0 || repeat_last_n > SAMPLE_HIST_CAP)
    return set_err(5, "set_sampling_ex: repeat_last_n %d outside [0,%d]",
                   repeat_last_n, SAMPLE_HIST_CAP);
  return apply_sampling(e, temperature, top_k, top_p, repeat_penalty,
                        repeat_last_n, seed);
}

// Test-only: `draws` consecutive draw indices of the product's sampler on
// private buffers and a private stream; the history stays as given.
extern "C" int cake_hip_op_sample(int V, const float* logits,
                                  float temperature, int top_k, float top_p,
                                  float repeat_penalty,
                                  const uint32_t* history, int n_history,
                                  uint64_t seed, int first_draw, int draws,
                                  uint32_t* tokens_out, int* kept_out,
                                  float* thr_out, int device) {
  const char* who = "op_sample";
  int r = sampling_args_err(who, temperature, top_p, repeat_penalty);
  if (r) return r;
  if (V < 1 || V > SAMPLE_MAX_V)
    return set_err(5, "%s: V %d outside [1,%d]", who, V, SAMPLE_MAX_V);
  if (draws < 1 || draws > 8192)
    return set_err(5, "%s: draws %d outside [1,8192]", who, draws);
  if (first_draw < 0) return set_err(5, "%s: first_draw %d < 0", who,
                                     first_draw);
  if (n_history < 0 || n_history > SAMPLE_HIST_CAP)
    return set_err(5, "%s: n_history %d outside [0,%d]", who, n_history,
                   SAMPLE_HIST_CAP);
  if (!logits || !tokens_out || !kept_out || !thr_out ||
      (n_history > 0 && !history))
    return set_err(5, "%s: null argument", who);
  for (int i = 0; i < n_history; ++i)
    if (history[i] >= (uint32_t)V)
      return set_err(5, "%s: history id %u outside the vocabulary (%d)", who,
                     history[i], V);
  OpBufs b;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipStreamCreate(&b.s));
  void *dl, *mem, *dtoks, *dmisc;
  if ((r = ob_upf32(b, logits, (size_t)V * 4, &dl))) return r;
  const size_t sb = sample_ws_bytes(V);
  if ((r = ob_alloc(b, &mem, sb))) return r;
  if ((r = ob_alloc(b, &dtoks, (size_t)draws * 4))) return r;
  if ((r = ob_alloc(b, &dmisc, 3 * 4))) return r;  // tok, pos, step
  HIP_TRY(hipMemsetAsync(mem, 0, sb, b.s));
  HIP_TRY(hipMemsetAsync(dmisc, 0, 3 * 4, b.s));
  SampleWs ws = sample_ws_bind(mem, V);
  const u32 st[2] = {(u32)n_history, (u32)first_draw};
  if (n_history > 0)
    HIP_TRY(hipMemcpyAsync(ws.hist, history, (size_t)n_history * 4,
                           hipMemcpyHostToDevice, b.s));
  HIP_TRY(hipMemcpyAsync(ws.state, st, sizeof st, hipMemcpyHostToDevice,
                         b.s));
  const float inv_temp = temperature > 0.f ? 1.0f / temperature : 0.f;
  u32* misc = (u32*)dmisc;
  for (int d = 0; d < draws; ++d)
    launch_sample((const float*)dl, V, ws, misc, (int*)(misc + 1),
                  (u32*)dtoks, (int*)(misc + 2), 0, inv_temp, top_k, top_p,
                  repeat_penalty, n_history, 0, seed, b.s);
  HIP_TRY(hipGetLastError());
  u32 res[4];
  HIP_TRY(hipMemcpyAsync(tokens_out, dtoks, (size_t)draws * 4,
                         hipMemcpyDeviceToHost, b.s));
  HIP_TRY(hipMemcpyAsync(res, ws.state, sizeof res, hipMemcpyDeviceToHost,
                         b.s));
  HIP_TRY(hipStreamSynchronize(b.s));
  *kept_out = (int)res[2];
  memcpy(thr_out, &res[3], 4);
  return 0;
}

// Test-only: `steps` consecutive launch_argmax calls (the greedy /
// plain-temperature head of every decode step) on private buffers.  Every
// word of the partials and of the ring starts as the bit pattern of
// CAKE_HIP_OP_SENTINEL and both carry guards.
extern "C" int cake_hip_op_argmax(int V, const float* logits,
                                  float temperature, uint64_t seed,
                                  int first_step, int steps, int use_ring,
                                  int advance_pos, uint32_t* tokens_out,
                                  float* pval_out, int32_t* pidx_out,
                                  uint32_t* ring_out, int* pos_step_out,
                                  int device) {
  const char* who = "op_argmax";
  const int NP = 256;  // launch_argmax's partition count
  if (std::isnan(temperature))
    return set_err(5, "%s: NaN temperature", who);
  if (V < 1 || V > (1 << 24))
    return set_err(5, "%s: V %d outside [1,%d]", who, V, 1 << 24);
  if (steps < 1 || steps > 8192)
    return set_err(5, "%s: steps %d outside [1,8192]", who, steps);
  if (first_step < 0 || first_step > (1 << 20))
    return set_err(5, "%s: first_step %d outside [0,%d]", who, first_step,
                   1 << 20);
  if (advance_pos != 0 && advance_pos != 1)
    return set_err(5, "%s: advance_pos %d not 0|1", who, advance_pos);
  if (!logits || !tokens_out || !pval_out || !pidx_out || !pos_step_out ||
      (use_ring && !ring_out))
    return set_err(5, "%s: null argument", who);
  OpBufs b;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipStreamCreate(&b.s));
  int r;
  const size_t nring = (size_t)first_step + steps + OPG;
  void *dl, *dtoks, *dmisc;
  float *dpv, *dpi, *dring = nullptr;
  if ((r = ob_upf32(b, logits, (size_t)V * 4, &dl))) return r;
  if ((r = ob_sent32(b, NP + OPG, &dpv))) return r;
  if ((r = ob_sent32(b, NP + OPG, &dpi))) return r;
  if (use_ring && (r = ob_sent32(b, nring, &dring))) return r;
  if ((r = ob_alloc(b, &dtoks, (size_t)steps * 4))) return r;
  const int misc[3] = {0, 0, first_step};  // tok, pos, step
  if ((r = ob_upf32(b, misc, sizeof misc, &dmisc))) return r;
  u32* m = (u32*)dmisc;
  const float inv_temp = temperature > 0.f ? 1.0f / temperature : 0.f;
  for (int d = 0; d < steps; ++d) {
    launch_argmax((const float*)dl, V, dpv, (int*)dpi, m, (int*)(m + 1),
                  (u32*)dring, (int*)(m + 2), advance_pos, inv_temp, seed,
                  b.s);
    HIP_TRY(hipMemcpyAsync((u32*)dtoks + d, m, 4, hipMemcpyDeviceToDevice,
                           b.s));
  }
  HIP_TRY(hipGetLastError());
  int res[3];
  HIP_TRY(hipMemcpyAsync(tokens_out, dtoks, (size_t)steps * 4,
                         hipMemcpyDeviceToHost, b.s));
  HIP_TRY(hipMemcpyAsync(pval_out, dpv, (NP + OPG) * 4,
                         hipMemcpyDeviceToHost, b.s));
  HIP_TRY(hipMemcpyAsync(pidx_out, dpi, (NP + OPG) * 4,
                         hipMemcpyDeviceToHost, b.s));
  if (use_ring)
    HIP_TRY(hipMemcpyAsync(ring_out, dring, nring * 4, hipMemcpyDeviceToHost,
                           b.s));
  if ((r = ob_downf32(b, dmisc, sizeof res, res))) return r;
  pos_step_out[0] = res[1];
  pos_step_out[1] = res[2];
  return 0;
}

// Test-only: the embedding gathers on a (Vt, H) table that crosses the
// boundary as f32 and goes through the f32 -> bf16 upload every op entry
// uses.  mode 0: launch_embed_rows on S ids; 1: launch_embed_token on one
// id; 2: the same with the fp8 norm chain's nscale.
extern "C" int cake_hip_op_embed(int Vt, int H, int S, int mode,
                                 const float* table, const uint32_t* ids,
                                 float eps, float* out, float* nscale_out,
                                 int device) {
  const char* who = "op_embed";
  if (mode < 0 || mode > 2) return set_err(5, "%s: mode %d", who, mode);
  // the hidden sizes engine create accepts
  if (H < 8 || H > 16384 || H % 8 != 0)
    return set_err(5, "%s: H %d must be a multiple of 8 in [8,16384]", who, H);
  if (Vt < 1 || Vt > (1 << 20))
    return set_err(5, "%s: Vt %d outside [1,%d]", who, Vt, 1 << 20);
  if (S < 1 || S > 4096 || (mode != 0 && S != 1))
    return set_err(5, "%s: S %d (rows: 1..4096, token: 1)", who, S);
  if (!table || !ids || !out || !nscale_out)
    return set_err(5, "%s: null argument", who);
  for (int i = 0; i < S; ++i)
    if (ids[i] >= (uint32_t)Vt)
      return set_err(5, "%s: id %u outside the table (%d rows)", who, ids[i],
                     Vt);
  OpBufs b;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipStreamCreate(&b.s));
  int r;
  const size_t n = (size_t)S * H;
  u16 *dt, *dout;
  void* dids;
  float* dns;
  if ((r = ob_up16(b, table, (size_t)Vt * H, &dt))) return r;
  if ((r = ob_upf32(b, ids, (size_t)S * 4, &dids))) return r;
  if ((r = ob_sent16(b, n + OPG, &dout))) return r;
  if ((r = ob_sent32(b, 1 + OPG, &dns))) return r;
  if (mode == 0)
    launch_embed_rows(dt, (const u32*)dids, dout, S, H, b.s);
  else
    launch_embed_token(dt, (const u32*)dids, dout, H, b.s,
                       mode == 2 ? dns : nullptr, eps);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(nscale_out, dns, (1 + OPG) * 4,
                         hipMemcpyDeviceToHost, b.s));
  return ob_down16(b, dout, n + OPG, out);
}

extern "C" int cake_hip_set_stats(cake_engine* e, int enabled) {
  e->st.on = enabled != 0;
  return 0;
}
extern "C" int cake_hip_stats_reset(cake_engine* e) {
  stats_flush(e);
  e->st.fams.clear();
  e->st.truncated = false;
  return 0;
}
extern "C" int cake_hip_kernel_stats(cake_engine* e, char* buf, int cap) {
  stats_flush(e);
  std::string out = "{\"truncated\": ";
  out += e->st.truncated ? "true" : "false";
  out += ", \"kernels\": {";
  bool first = true;
  char tmp[256];
  for (auto& kv : e->st.fams) {
    if (!first) out += ", ";
    first = false;
    snprintf(tmp, sizeof tmp,
             "\"%s\": {\"launches\": %ld, \"ms\": %.4f, \"bytes\": %.0f, "
             "\"flops\": %.0f}",
             kv.first.c_str(), kv.second.launches, kv.second.ms,
             kv.second.bytes, kv.second.flops);
    out += tmp;
  }
  out += "}}";
  if ((int)out.size() + 1 > cap) return set_err(5, "buffer too small");
  memcpy(buf, out.c_str(), out.size() + 1);
  return 0;
}
extern "C" int cake_hip_sync(cake_engine* e) {
  HIP_TRY(hipSetDevice(e->device));
  HIP_TRY(hipStreamSynchronize(e->stream));
  stats_flush(e);
  return 0;
}
extern "C" const char* cake_hip_build_info(void) {
  return "gfx950;" __DATE__ " " __TIME__;
}

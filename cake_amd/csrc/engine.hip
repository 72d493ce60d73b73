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
//
// This file: config, engine create/free, the per-layer enqueue, the
// generation loop, comm, topology, sampling config and stats.  The weight
// loader and cake_hip_init_random are in weights.hip, the cake_hip_op_* test
// surface and the dispatch queries in ops.hip; engine_internal.h is what the
// three share.
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "engine_internal.h"
#include "json.hpp"

// ---------------------------------------------------------------------------
// errors
// ---------------------------------------------------------------------------
static thread_local std::string g_err;
int set_err(int code, const char* fmt, ...) {
  char buf[1024];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof buf, fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}
extern "C" const char* cake_hip_last_error(void) { return g_err.c_str(); }

#define NCCL_TRY(x)                                                     \
  do {                                                                  \
    ncclResult_t _e = (x);                                              \
    if (_e != ncclSuccess)                                              \
      return set_err(3, "%s:%d rccl error: %s", __FILE__, __LINE__,     \
                     ncclGetErrorString(_e));                           \
  } while (0)

// ---------------------------------------------------------------------------
// model config parse (the struct is in engine_internal.h)
// ---------------------------------------------------------------------------
// The gemma3-only fields of the text config object v (HF Gemma3TextConfig):
// what the family always sets, the layer kinds, both ropes, the score scale,
// and the refusals.
static int parse_gemma3(const minijson::Value& v, ModelConfig* c) {
  using minijson::Value;
  auto set_null = [&](const char* k) {
    auto p = v.get(k);
    return p && !p->is_null();
  };
  for (const char* k : {"final_logit_softcapping", "attn_logit_softcapping"})
    if (set_null(k))
      return set_err(5, "config.json: %s is not supported (gemma3 without "
                        "softcapping only)", k);
  if (auto p = v.get("hidden_activation"))
    if (!p->is_null() && p->str != "gelu_pytorch_tanh")
      return set_err(5, "config.json: hidden_activation %s is not supported "
                        "(gemma3 runs gelu_pytorch_tanh)", p->str.c_str());
  if (auto p = v.get("use_bidirectional_attention"))
    if (p->bool_or(false))
      return set_err(5, "config.json: use_bidirectional_attention true is "
                        "not supported");
  c->tied = true;
  c->qk_norm = true;
  c->window = 4096;  // sliding_window, if present, overwrites it below
  c->qpas = 256.f;
  if (auto p = v.get("query_pre_attn_scalar"))
    if (p->kind == Value::Num) c->qpas = (float)p->num;
  if (!(c->qpas > 0))
    return set_err(5, "config.json: query_pre_attn_scalar %g must be > 0",
                   (double)c->qpas);
  // layer kinds: layer_types in any order, or sliding_window_pattern
  c->local.assign(c->layers, 0);
  auto lt = v.get("layer_types");
  if (lt && lt->kind == Value::Arr) {
    if ((int)lt->arr.size() != c->layers)
      return set_err(5, "config.json: layer_types has %d entries for %d "
                        "layers", (int)lt->arr.size(), c->layers);
    for (int i = 0; i < c->layers; ++i) {
      const std::string& s = lt->arr[i]->str;
      if (s != "sliding_attention" && s != "full_attention")
        return set_err(5, "config.json: layer_types[%d] %s is not supported",
                       i, s.c_str());
      c->local[i] = s == "sliding_attention";
    }
  } else {
    int pat = 6;
    if (auto p = v.get("sliding_window_pattern"))
      if (p->kind == Value::Num) pat = (int)p->num;
    if (pat < 1)
      return set_err(5, "config.json: sliding_window_pattern %d", pat);
    for (int i = 0; i < c->layers; ++i) c->local[i] = (i + 1) % pat != 0;
  }
  // rope: rope_parameters {full_attention, sliding_attention}, or rope_theta
  // + rope_local_base_freq + rope_scaling (which concerns the global layers)
  c->rope_theta = 1e6f;
  c->rope_local_theta = 1e4f;
  if (auto p = v.get("rope_theta"))
    if (p->kind == Value::Num) c->rope_theta = (float)p->num;
  if (auto p = v.get("rope_local_base_freq"))
    if (p->kind == Value::Num) c->rope_local_theta = (float)p->num;
  auto one = [&](const minijson::ValuePtr& o, const char* where, float* theta,
                 float* lin) -> int {
    if (!o || o->kind != Value::Obj) return 0;
    if (auto p = o->get("rope_theta"))
      if (p->kind == Value::Num) *theta = (float)p->num;
    auto ty = o->get("rope_type");
    if (!ty) ty = o->get("type");
    if (!ty || ty->is_null() || ty->str == "default") return 0;
    if (ty->str != "linear")
      return set_err(5, "config.json: %s rope type %s is not supported "
                        "(gemma3: default or linear)", where, ty->str.c_str());
    auto f = o->get("factor");
    if (!f || f->kind != Value::Num || !(f->num > 0))
      return set_err(5, "config.json: %s linear rope needs a factor > 0",
                     where);
    *lin = (float)f->num;
    return 0;
  };
  int r;
  if ((r = one(v.get("rope_scaling"), "rope_scaling", &c->rope_theta,
               &c->rope_lin)))
    return r;
  if (auto rp = v.get("rope_parameters")) {
    if ((r = one(rp->get("full_attention"), "rope_parameters.full_attention",
                 &c->rope_theta, &c->rope_lin)))
      return r;
    if ((r = one(rp->get("sliding_attention"),
                 "rope_parameters.sliding_attention", &c->rope_local_theta,
                 &c->rope_local_lin)))
      return r;
  }
  return 0;
}

int parse_config(const char* json, ModelConfig* c) {
  minijson::ValuePtr v;
  try {
    v = minijson::parse(json);
  } catch (const std::exception& e) {
    return set_err(5, "config.json: %s", e.what());
  }
  if (!v || v->kind != minijson::Value::Obj)
    return set_err(5, "config.json: not an object");
  // gemma3_text, or gemma3 (the multimodal checkpoint) with the text model
  // nested under text_config: that object is parsed, every missing field
  // taking HF's Gemma3TextConfig default.  quantization_config stays at the
  // top level of either form.
  const minijson::ValuePtr root = v;
  bool g3 = false;
  if (auto p = v->get("model_type")) {
    g3 = p->str == "gemma3_text" || p->str == "gemma3";
    if (p->str == "gemma3") {
      auto tc = v->get("text_config");
      if (tc && tc->kind == minijson::Value::Obj) {
        v = tc;
      } else {
        v = std::make_shared<minijson::Value>();
        v->kind = minijson::Value::Obj;
      }
    }
  }
  auto geti = [&](const char* k, int d) {
    auto p = v->get(k);
    return p ? (int)p->num_or(d) : d;
  };
  c->gemma3 = g3;
  c->hidden = geti("hidden_size", g3 ? 2304 : 0);
  c->inter = geti("intermediate_size", g3 ? 9216 : 0);
  c->vocab = geti("vocab_size", g3 ? 262208 : 0);
  c->layers = geti("num_hidden_layers", g3 ? 26 : 0);
  c->nh = geti("num_attention_heads", g3 ? 8 : 0);
  c->nkv = geti("num_key_value_heads", g3 ? 4 : c->nh);
  c->head_dim = geti("head_dim", g3 ? 256 : 0);
  c->max_pos = geti("max_position_embeddings", g3 ? 131072 : 4096);
  if (g3) c->rms_eps = 1e-6f;
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
  if (g3) {
    int r = parse_gemma3(*v, c);
    if (r) return r;
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
    if (lt->kind == minijson::Value::Arr && !g3) {
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
  auto qc = v->get("quantization_config");
  if (!qc) qc = root->get("quantization_config");
  if (qc)
    if (auto qm = qc->get("quant_method")) {
      c->fp8 = qm->str == "fp8";
      c->w4 = qm->str == "gptq";
      if (g3 && (c->fp8 || c->w4))
        return set_err(5, "config.json: quant_method %s with model_type "
                          "gemma3 is not supported (the fp8 and gptq gate-up "
                          "kernels have no GELU form)", qm->str.c_str());
      if (c->fp8) {
        // the kernels and the loader's scale offsets are built for 128 x 128
        // blocks (fp8.rs:17); absent (or null) means that default
        auto bs = qc->get("weight_block_size");
        if (bs && !bs->is_null()) {
          // the value as written, for the message: a number or a list of them
          auto show = [](const minijson::Value& x) {
            char num[32];
            snprintf(num, sizeof num, "%g", x.num);
            return x.kind == minijson::Value::Num ? std::string(num)
                                                  : std::string("?");
          };
          std::string shown = show(*bs);
          if (bs->kind == minijson::Value::Arr) {
            shown = "[";
            for (size_t i = 0; i < bs->arr.size(); ++i)
              shown += (i ? ", " : "") + show(*bs->arr[i]);
            shown += "]";
          }
          if (shown != "[128, 128]")
            return set_err(5, "config.json: quantization_config."
                              "weight_block_size %s is not supported (fp8 "
                              "weights need [128, 128] blocks)",
                           shown.c_str());
        }
      }
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
int w4_dim_err(const char* name, int N, int K, int g) {
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
int w4_config_err(const ModelConfig& c) {
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
  // gemma3: either table, with rope type "linear" as inv_freq / factor; in
  // double and rounded once, like the LongRoPE frequencies below
  if (c.gemma3)
    for (int i = 0; i < half; ++i)
      theta[i] = (float)(1.0 / ((double)c.rope_lin *
                                pow((double)c.rope_theta, 2.0 * i / (double)rd)));
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
  return cake_hip_rope_tables_ex(config_json, max_seq, 0, cosv, sinv, rd_out);
}
// which: 0 = the (global) table every model has, 1 = the local layers' table
// of a gemma3 config
extern "C" int cake_hip_rope_tables_ex(const char* config_json, int max_seq,
                                       int which, float* cosv, float* sinv,
                                       int* rd_out) {
  ModelConfig c;
  int r = parse_config(config_json, &c);
  if (r) return r;
  if (which != 0 && which != 1)
    return set_err(5, "rope_tables: which %d not in {0, 1}", which);
  if (which == 1 && !c.gemma3)
    return set_err(5, "rope_tables: only a gemma3 config has a local table");
  if (which == 1) c = c.local_rope();
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

// Host only: what engine create plans for one layer of this config.
extern "C" int cake_hip_layer_dispatch(const char* config_json, int layer,
                                       int* window, int* rope_table,
                                       float* q_scale) {
  ModelConfig c;
  int r = parse_config(config_json, &c);
  if (r) return r;
  if (layer < 0 || layer >= c.layers)
    return set_err(5, "layer_dispatch: layer %d outside [0,%d)", layer,
                   c.layers);
  if (window) *window = c.win_for(layer);
  if (rope_table) *rope_table = c.gemma3 && c.is_local(layer) ? 1 : 0;
  if (q_scale) *q_scale = c.gemma3 ? c.q_fold() : 1.f;
  return 0;
}

int dev_alloc(std::vector<void*>& owned, void** p, size_t bytes) {
  hipError_t e = hipMalloc(p, bytes);
  if (e != hipSuccess)
    return set_err(2, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e));
  owned.push_back(*p);
  return 0;
}

// ---- stats helpers --------------------------------------------------------
static hipEvent_t ev_get(cake_engine* e, bool first) {
  Stats& s = e->st;
  if (first) {
    if (s.pool_used < s.pool.size()) return s.pool[s.pool_used].first;
    if (s.pool.size() >= Stats::CAP) return nullptr;
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess) return nullptr;
    if (hipEventCreate(&b) != hipSuccess) {
      hipEventDestroy(a);
      return nullptr;
    }
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

// ---------------------------------------------------------------------------
// per-layer decode / prefill enqueue (the Transformer::forward sequence,
// transformer.rs:103-135 + attention.rs:152-357 + mlp.rs:21-31).  The weight
// format switch lives in the three helpers below.
// ---------------------------------------------------------------------------
// Decode: out = p . rms_norm(e->x, nw); for the fused gate|up tensor
// (gateup) the kernel goes on to silu_mul and out has N/2 columns.  bf16 and
// fp8 fuse the norm into the GEMV, or run it as a launch of their own inside
// the same family (CAKE_BF16_SPLITNORM / CAKE_FP8_SPLITNORM), or, fp8 with
// chain_scale, read the scale its producer published (CAKE_FP8_NORMCHAIN).
// The 4-bit kernels take normalized x: always two launches, booked apart.
static void enqueue_norm_proj(cake_engine* e, const Proj& p, const u16* nw,
                              bool gateup, const float* chain_scale,
                              u16* out) {
  const int N = p.N, K = p.K, I = N / 2;
  const float eps = e->c.rms_eps;
  const double flops = 2.0 * N * K, out_bytes = (gateup ? I : N) * 2;
  auto norm = [&] { launch_rmsnorm(e->x, nw, e->xn, 1, K, eps, e->stream); };
  if (p.fmt == W_GPTQ) {
    {
      StatScope ss(e, "rmsnorm", 2.0 * K * 2, 0);
      norm();
    }
    StatScope ss(e, gateup ? "gemv_gateup_w4" : "gemv_w4",
                 p.bytes() + K * 2 + out_bytes, flops);
    if (gateup)
      launch_gemv_gateup_w4(p.w4(), p.aux, e->xn, out, I, K, p.g, e->stream);
    else
      launch_gemv_w4(p.w4(), p.aux, e->xn, out, nullptr, N, K, p.g, 0,
                     e->stream);
    return;
  }
  const bool gelu = gateup && e->c.gemma3;  // bf16 only (parse_config)
  StatScope ss(e, gelu ? "gemv_gateup_gelu" : gateup ? "gemv_gateup"
                                                      : "gemv_qkv",
               p.bytes() + 2.0 * K * 2 + out_bytes, flops);
  // x as the GEMV reads it, and the norm weight it applies itself (if any)
  const u16* x = e->x;
  const u16* fused_nw = nw;
  NormIO nio{};
  if (chain_scale) {
    nio.scale_in = chain_scale;
    nio.nw = nw;
    fused_nw = nullptr;
  } else if (p.fmt == W_FP8 ? e->fp8_splitnorm : e->bf16_splitnorm) {
    norm();
    x = e->xn;
    fused_nw = nullptr;
  }
  const float fused_eps = fused_nw ? eps : 0.f;
  if (p.fmt == W_FP8) {
    if (gateup)
      launch_gemv_gateup_fp8(p.fp8(), p.aux, x, out, fused_nw, fused_eps, I,
                             K, e->stream, nio);
    else
      launch_gemv_fp8(p.fp8(), p.aux, x, out, nullptr, fused_nw, fused_eps,
                      N, K, 0, e->stream, nio);
  } else if (gelu) {
    launch_gemv_gateup_gelu(p.bf16(), x, out, fused_nw, fused_eps, I, K,
                            e->gu_rows, e->stream);
  } else if (gateup) {
    launch_gemv_gateup(p.bf16(), x, out, fused_nw, fused_eps, I, K,
                       e->gu_rows, e->stream);
  } else {
    launch_gemv(p.bf16(), x, out, nullptr, fused_nw, fused_eps, N, K, 0,
                e->stream);
  }
}

// Decode: e->x += p . a, the residual projections (o, down; the residual is
// aliased).  Under the fp8 norm chain the epilogue publishes the rms scale of
// the new x into chain slot `slot` for the next norm_proj.  Every gptq GEMV
// books under gemv_w4.
static void enqueue_res_proj(cake_engine* e, const Proj& p, const char* fam,
                             const u16* a, int slot) {
  const int N = p.N, K = p.K;
  StatScope ss(e, p.fmt == W_GPTQ ? "gemv_w4" : fam,
               p.bytes() + K * 2 + N * 4, 2.0 * N * K);
  if (p.fmt == W_GPTQ) {
    launch_gemv_w4(p.w4(), p.aux, a, e->x, e->x, N, K, p.g, 1, e->stream);
  } else if (p.fmt == W_FP8) {
    NormIO nio{};
    if (e->fp8_normchain) {
      nio.part = e->nsq_part + (size_t)slot * N;
      nio.cnt = e->nsq_cnt + slot * 16;
      nio.scale_out = e->nscale + slot;
      nio.eps = e->c.rms_eps;
    }
    launch_gemv_fp8(p.fp8(), p.aux, a, e->x, e->x, nullptr, 0.f, N, K, 1,
                    e->stream, nio);
  } else if (e->splitk == 2 && K % 16 == 0) {
    launch_gemv_res_splitk(p.bf16(), a, e->x, e->x, e->gemv_ws, e->gemv_cnt,
                           N, K, e->stream);
  } else {
    launch_gemv(p.bf16(), a, e->x, e->x, nullptr, 0.f, N, K, 1, e->stream);
  }
}

// gemma3 decode: t = p . a with no residual (t is e->xn, free once the norm
// GEMV before it has run), then e->x = bf16(e->x + bf16(rms_norm(t) * post)).
static void enqueue_post_proj(cake_engine* e, const Proj& p, const char* fam,
                              const u16* a, const u16* post) {
  const int N = p.N, K = p.K;
  {
    StatScope ss(e, fam, p.bytes() + K * 2 + N * 2, 2.0 * N * K);
    launch_gemv(p.bf16(), a, e->xn, nullptr, nullptr, 0.f, N, K, 0,
                e->stream);
  }
  StatScope ss(e, "postnorm_add", 4.0 * N * 2, 0);
  launch_postnorm_add(e->x, e->xn, post, 1, N, e->c.rms_eps, e->stream);
}

// Prefill: the bf16 (N, K) weight launch_gemm reads.  fp8 and gptq dequantize
// into the shared e->wscratch right before each GEMM.
static const u16* gemm_weight(cake_engine* e, const Proj& p) {
  if (p.fmt == W_BF16) return p.bf16();
  const double io = p.bytes() + (double)p.elems() * 2;
  if (p.fmt == W_FP8) {
    StatScope ss(e, "dequant_fp8", io, 0);
    launch_dequant_fp8(p.fp8(), p.aux, e->wscratch, p.N, p.K, e->stream);
  } else {
    StatScope ss(e, "dequant_w4", io, 0);
    launch_dequant_w4(p.w4(), p.aux, e->wscratch, p.N, p.K, p.g, e->stream);
  }
  return e->wscratch;
}

// slot A of the fp8 norm chain (pre-qkv rms1) is produced by embed or the
// previous layer's down projection, slot B (pre-gateup rms2) by this layer's
// o projection; have_scale_a = false when x has no producing kernel
static void enqueue_layer_decode(cake_engine* e, LayerDev& l,
                                 bool have_scale_a = true) {
  const ModelConfig& c = e->c;
  const int H = c.hidden, hd = c.hd();
  const int Sq = c.sq(), Nq = c.nqkv();
  const bool chain = c.fp8 && e->fp8_normchain;
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
    StatScope ss(e, "gemv_qkv", l.qkv.bytes() + 2.0 * H * 2 + Nq * 2,
                 2.0 * Nq * H);
    launch_gemv_qkv_rope(l.qkv.bf16(), e->x, e->qkv, l.rms1, c.rms_eps, l.kc,
                         l.vc, l.vtc, l.cos_t, l.sin_t, e->dev_pos, c.nh,
                         c.nkv, hd, c.rd(), e->max_seq, H, e->stream, l.bqkv);
  } else {
    enqueue_norm_proj(e, l.qkv, l.rms1, false,
                      chain && have_scale_a ? e->nscale + 0 : nullptr, e->qkv);
    // [Qwen3 QK-norm, attention.rs:202-215 | qwen2 bias, fused +] rope +
    // KV store
    StatScope ss(e, "rope_store", 0, 0);
    launch_rope_store_decode(e->qkv, l.kc, l.vc, l.vtc, l.cos_t, l.sin_t,
                             e->dev_pos, c.nh, c.nkv, hd, c.rd(), e->max_seq,
                             l.qnorm, l.knorm, c.rms_eps, e->stream, l.bqkv);
  }
  {  // decode attention over the cache (single launch, split-KV combine)
    double kvbytes = 2.0 * (e->host_pos + 1) * c.skv() * 2;
    StatScope ss(e, "attn_decode", kvbytes + Sq * 2 * 2,
                 4.0 * (e->host_pos + 1) * Sq);
    launch_attn_decode(e->qkv, l.kc, l.vc, e->dev_pos, e->attn_ws,
                       e->attn_cnt, e->attn_out, c.nh, c.nkv, hd, e->max_seq,
                       e->nchunk, c.win_for(l.idx), e->stream);
  }
  if (c.gemma3) {  // sandwich norms: o and down go through their post-norm
    enqueue_post_proj(e, l.o, "gemv_o", e->attn_out, l.post1);
    enqueue_norm_proj(e, l.gu, l.rms2, true, nullptr, e->act);
    enqueue_post_proj(e, l.down, "gemv_down", e->act, l.post2);
    return;
  }
  enqueue_res_proj(e, l.o, "gemv_o", e->attn_out, 1);
  // rms_2 -> gate_up GEMV + silu_mul (mlp.rs:21-31)
  enqueue_norm_proj(e, l.gu, l.rms2, true, chain ? e->nscale + 1 : nullptr,
                    e->act);
  enqueue_res_proj(e, l.down, "gemv_down", e->act, 0);
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
  const u16* wqkv = gemm_weight(e, l.qkv);
  {
    StatScope ss(e, "gemm_qkv", (double)Nq * H * 2 + (double)S * (H + Nq) * 2,
                 2.0 * S * Nq * H);
    launch_gemm(e->xn, wqkv, e->qkv, nullptr, S, Nq, H, 0, e->stream);
  }
  {  // [fused QK-norm | qkv bias +] rope + KV store for all S positions
    StatScope ss(e, "rope_store_pf", 0, 0);
    launch_rope_store_prefill(e->qkv, l.kc, l.vc, l.vtc, l.cos_t, l.sin_t,
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
  const u16* wo = gemm_weight(e, l.o);
  {
    StatScope ss(e, "gemm_o", (double)H * Sq * 2 + (double)S * (Sq + H) * 2,
                 2.0 * S * H * Sq);
    if (c.gemma3)  // into xn (free after the qkv GEMM), no residual
      launch_gemm(e->attn_out, wo, e->xn, nullptr, S, H, Sq, 0, e->stream);
    else
      launch_gemm(e->attn_out, wo, x, x, S, H, Sq, 1, e->stream);
  }
  if (c.gemma3) {
    StatScope ss(e, "postnorm_add_pf", 4.0 * S * H * 2, 0);
    launch_postnorm_add(x, e->xn, l.post1, S, H, c.rms_eps, e->stream);
  }
  {
    StatScope ss(e, "rmsnorm_pf", 2.0 * S * H * 2, 0);
    launch_rmsnorm(x, l.rms2, e->xn, S, H, c.rms_eps, e->stream);
  }
  const u16* wgu = gemm_weight(e, l.gu);
  {
    StatScope ss(e, "gemm_gateup",
                 2.0 * I * H * 2 + (double)S * (H + 2.0 * I) * 2,
                 4.0 * S * I * H);
    launch_gemm(e->xn, wgu, e->gu, nullptr, S, 2 * I, H, 0, e->stream);
  }
  if (c.gemma3) {
    StatScope ss(e, "gelu_mul", 3.0 * S * I * 2, 0);
    launch_gelu_mul_rows(e->gu, e->act, S, I, e->stream);
  } else {
    StatScope ss(e, "silu_mul", 3.0 * S * I * 2, 0);
    launch_silu_mul_rows(e->gu, e->act, S, I, e->stream);
  }
  const u16* wdown = gemm_weight(e, l.down);
  {
    StatScope ss(e, "gemm_down", (double)H * I * 2 + (double)S * (I + H) * 2,
                 2.0 * S * H * I);
    if (c.gemma3)
      launch_gemm(e->act, wdown, e->xn, nullptr, S, H, I, 0, e->stream);
    else
      launch_gemm(e->act, wdown, x, x, S, H, I, 1, e->stream);
  }
  if (c.gemma3) {
    StatScope ss(e, "postnorm_add_pf", 4.0 * S * H * 2, 0);
    launch_postnorm_add(x, e->xn, l.post2, S, H, c.rms_eps, e->stream);
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
// the token(s) -> x; gemma3 scales the rows by bf16(sqrt(H))
static void enqueue_embed_token(cake_engine* e, float* nsc) {
  if (e->c.gemma3)
    launch_embed_token_scaled(e->embed, e->dev_tok, e->x, e->c.hidden,
                              e->stream);
  else
    launch_embed_token(e->embed, e->dev_tok, e->x, e->c.hidden, e->stream,
                       nsc, e->c.rms_eps);
}
static void enqueue_embed_rows(cake_engine* e, u16* x, int S) {
  if (e->c.gemma3)
    launch_embed_rows_scaled(e->embed, e->ids, x, S, e->c.hidden, e->stream);
  else
    launch_embed_rows(e->embed, e->ids, x, S, e->c.hidden, e->stream);
}

static int enqueue_decode_step(cake_engine* e) {
  const ModelConfig& c = e->c;
  const int H = c.hidden;
  float* nsc = (e->c.fp8 && e->fp8_normchain) ? e->nscale : nullptr;
  if (e->world == 1) {
    enqueue_embed_token(e, nsc);
    for (auto& l : e->L) enqueue_layer_decode(e, l);
    enqueue_head_sample(e, 1, 1);
    return 0;
  }
  if (e->rank == 0) {
    enqueue_embed_token(e, nsc);
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
// one projection (N, K) in the engine's weight format
static int alloc_proj(cake_engine* e, Proj* p, int N, int K) {
  const ModelConfig& c = e->c;
  p->N = N;
  p->K = K;
  p->fmt = c.fp8 ? W_FP8 : c.w4 ? W_GPTQ : W_BF16;
  p->g = c.w4 ? c.grp(K) : 0;
  ALLOC(e->mem, p->w, char, p->w_bytes());
  if (p->aux_elems()) ALLOC(e->mem, p->aux, float, p->aux_elems());
  return 0;
}

// Builds the engine into *out, which is set as soon as the engine exists:
// on a failing return the caller frees whatever was built so far.
static int engine_build(const char* config_json, int layer_lo, int layer_hi,
                        int flags, int max_seq, int max_batch_tokens,
                        int device, cake_engine** out) {
  ModelConfig c;
  int r = parse_config(config_json, &c);
  if (r) return r;
  if (layer_lo < 0 || layer_hi > c.layers || layer_lo >= layer_hi)
    return set_err(5, "bad layer range [%d,%d) of %d", layer_lo, layer_hi,
                   c.layers);
  if (c.hd() != 256 && (c.hd() < 8 || c.hd() > 128 || c.hd() % 8 != 0))
    return set_err(5, "head_dim %d unsupported (must be a multiple of 8 in "
                   "[8,128], or 256)", c.hd());
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
  auto* e = *out = new cake_engine();
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
  const size_t kv_elems = (size_t)c.nkv * max_seq * hd;
  for (auto& l : e->L) {
    ALLOC(e->mem, l.rms1, u16, H);
    ALLOC(e->mem, l.rms2, u16, H);
    if ((r = alloc_proj(e, &l.qkv, Nq, H))) return r;
    if ((r = alloc_proj(e, &l.o, H, Sq))) return r;
    if ((r = alloc_proj(e, &l.gu, 2 * I, H))) return r;
    if ((r = alloc_proj(e, &l.down, H, I))) return r;
    if (c.qk_norm) {
      ALLOC(e->mem, l.qnorm, u16, hd);
      ALLOC(e->mem, l.knorm, u16, hd);
    }
    if (c.qkv_bias) ALLOC(e->mem, l.bqkv, float, Nq);
    if (c.gemma3) {
      ALLOC(e->mem, l.post1, u16, H);
      ALLOC(e->mem, l.post2, u16, H);
    }
    // zero the caches: positions >= n are masked (weight 0) but 0*NaN from
    // allocator garbage would still poison the PV MFMA
    for (u16** kv : {&l.kc, &l.vc, &l.vtc}) {
      ALLOC(e->mem, *kv, u16, kv_elems);
      HIP_TRY(hipMemset(*kv, 0, kv_elems * 2));
    }
  }
  if (e->has_embed()) ALLOC(e->mem, e->embed, u16, (size_t)V * H);
  if (e->has_head()) {
    ALLOC(e->mem, e->norm_w, u16, H);
    if (c.tied && e->has_embed())
      e->lm_head = e->embed;  // an alias: e->mem holds the tensor once
    else
      ALLOC(e->mem, e->lm_head, u16, (size_t)V * H);
  }
  // rope tables
  {
    std::vector<float> ct, st;
    build_rope_tables(c, max_seq, &ct, &st);
    ALLOC(e->mem, e->cos_t, float, ct.size());
    ALLOC(e->mem, e->sin_t, float, st.size());
    HIP_TRY(hipMemcpy(e->cos_t, ct.data(), ct.size() * 4,
                      hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(e->sin_t, st.data(), st.size() * 4,
                      hipMemcpyHostToDevice));
    if (c.gemma3) {  // the local layers' table
      build_rope_tables(c.local_rope(), max_seq, &ct, &st);
      ALLOC(e->mem, e->cos_l, float, ct.size());
      ALLOC(e->mem, e->sin_l, float, st.size());
      HIP_TRY(hipMemcpy(e->cos_l, ct.data(), ct.size() * 4,
                        hipMemcpyHostToDevice));
      HIP_TRY(hipMemcpy(e->sin_l, st.data(), st.size() * 4,
                        hipMemcpyHostToDevice));
    }
    for (auto& l : e->L) {
      const bool loc = c.gemma3 && c.is_local(l.idx);
      l.cos_t = loc ? e->cos_l : e->cos_t;
      l.sin_t = loc ? e->sin_l : e->sin_t;
    }
  }
  // workspaces
  ALLOC(e->mem, e->x, u16, (size_t)BT * H);
  ALLOC(e->mem, e->x2, u16, (size_t)BT * H);
  HIP_TRY(hipStreamCreate(&e->comm_stream));
  for (int i = 0; i < 2; ++i) {
    HIP_TRY(hipEventCreateWithFlags(&e->ev_comp[i], hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&e->ev_comm[i], hipEventDisableTiming));
  }
  if (const char* ov = getenv("CAKE_PREFILL_OVERLAP"))
    e->prefill_overlap = atoi(ov);
  ALLOC(e->mem, e->xn, u16, (size_t)BT * H);
  ALLOC(e->mem, e->qkv, u16, (size_t)BT * Nq);
  ALLOC(e->mem, e->attn_out, u16, (size_t)BT * Sq);
  ALLOC(e->mem, e->gu, u16, (size_t)BT * 2 * I);
  ALLOC(e->mem, e->act, u16, (size_t)BT * I);
  if (c.fp8 || c.w4) {  // holds the largest dequantized projection
    const LayerDev& l = e->L[0];
    ALLOC(e->mem, e->wscratch, u16,
          std::max(std::max(l.qkv.elems(), l.o.elems()),
                   std::max(l.gu.elems(), l.down.elems())));
  }
  ALLOC(e->mem, e->logits, float, V);
  ALLOC(e->mem, e->fbuf, float, (size_t)BT * H);
  ALLOC(e->mem, e->ids, u32, BT);
  ALLOC(e->mem, e->ring, u32, cake_engine::RING_CAP);
  ALLOC(e->mem, e->pval, float, 256);
  ALLOC(e->mem, e->pidx, int, 256);
  if (e->has_head() && V >= 1 && V <= SAMPLE_MAX_V) {
    const size_t sb = sample_ws_bytes(V);
    ALLOC(e->mem, e->sample_mem, char, sb);
    HIP_TRY(hipMemset(e->sample_mem, 0, sb));
    e->sws = sample_ws_bind(e->sample_mem, V);
  }
  if (const char* nc = getenv("CAKE_NCHUNK")) {
    int v = atoi(nc);
    if (v >= 1 && v <= 64) e->nchunk = v;
  }
  e->gu_rows = gemv_gateup_rows_policy();  // CAKE_GU_ROWS
  ALLOC(e->mem, e->attn_ws, float, (size_t)c.nh * 64 * (hd + 4));  // nchunk <= 64; row stride 132 f32 = 16B-aligned
  if (hd == 128 && e->bt >= 1024)  // split-KV prefill partials
    ALLOC(e->mem, e->pf_ws, float, (size_t)c.nh * e->bt * 2 * 132);
  ALLOC(e->mem, e->attn_cnt, u32, c.nh);
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
    ALLOC(e->mem, e->nsq_part, float, (size_t)2 * H);
    ALLOC(e->mem, e->nsq_cnt, u32, 2 * 16);  // 8 residue shards + top, per slot
    ALLOC(e->mem, e->nscale, float, 2);
    HIP_TRY(hipMemset(e->nsq_cnt, 0, 2 * 16 * sizeof(u32)));
    HIP_TRY(hipMemset(e->nscale, 0, 2 * sizeof(float)));
  }
  {
    const size_t mx = (size_t)std::max(H, I);
    ALLOC(e->mem, e->gemv_ws, float, mx * 2);
    ALLOC(e->mem, e->gemv_cnt, u32, (mx + 1) / 2);
    HIP_TRY(hipMemset(e->gemv_cnt, 0, sizeof(u32) * ((mx + 1) / 2)));
  }
  ALLOC(e->mem, e->dev_pos, int, 1);
  ALLOC(e->mem, e->dev_step, int, 1);
  ALLOC(e->mem, e->dev_tok, u32, 1);
  HIP_TRY(hipMemset(e->dev_pos, 0, 4));
  HIP_TRY(hipMemset(e->dev_step, 0, 4));
  HIP_TRY(hipMemset(e->dev_tok, 0, 4));
  return 0;
}

extern "C" int cake_hip_engine_create(const char* config_json, int layer_lo,
                                      int layer_hi, int flags, int max_seq,
                                      int max_batch_tokens, int device,
                                      cake_engine** out) {
  cake_engine* e = nullptr;
  int r = engine_build(config_json, layer_lo, layer_hi, flags, max_seq,
                       max_batch_tokens, device, &e);
  if (r) {
    cake_hip_engine_free(e);  // the half-built engine; last_error stays
    return r;
  }
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
  for (void* p : e->mem) hipFree(p);
  for (auto& ev : e->st.pool) {
    hipEventDestroy(ev.first);
    hipEventDestroy(ev.second);
  }
  for (int i = 0; i < 2; ++i) {
    if (e->ev_comp[i]) hipEventDestroy(e->ev_comp[i]);
    if (e->ev_comm[i]) hipEventDestroy(e->ev_comm[i]);
  }
  if (e->comm_stream) hipStreamDestroy(e->comm_stream);
  if (e->stream) hipStreamDestroy(e->stream);
  delete e;
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
        enqueue_embed_rows(e, xb, S);
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
        enqueue_embed_rows(e, e->x, S);
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
  // The context crossed a chunk-count threshold: drop the graph (re-captured
  // lazily) and re-zero the epoch-free arrival counters, which advance by
  // nchunk per step, so a chunk-count change invalidates their modulo
  // election.  Called with the stream idle (after a sync).
  auto retune_nchunk = [&]() -> int {
    if (nchunk_fixed) return 0;
    const int want = want_nchunk(e->host_pos);
    if (want == e->nchunk) return 0;
    if (e->graph) {
      HIP_TRY(hipGraphExecDestroy(e->graph));
      e->graph = nullptr;
    }
    e->nchunk = want;
    HIP_TRY(hipMemset(e->attn_cnt, 0, sizeof(u32) * e->c.nh));
    return 0;
  };
  int r = retune_nchunk();
  if (r) return r;
  for (int s = 0; s < steps; ++s) {
    if (graph_ok && !e->graph) {
      // capture one decode step (device-side token/pos/ring make it
      // replayable)
      hipGraph_t g;
      HIP_TRY(hipStreamBeginCapture(e->stream, hipStreamCaptureModeGlobal));
      if ((r = enqueue_decode_step(e))) {
        hipStreamEndCapture(e->stream, &g);
        return r;
      }
      HIP_TRY(hipStreamEndCapture(e->stream, &g));
      HIP_TRY(hipGraphInstantiate(&e->graph, g, nullptr, nullptr, 0));
      HIP_TRY(hipGraphDestroy(g));
    }
    if (graph_ok) {
      HIP_TRY(hipGraphLaunch(e->graph, e->stream));
    } else if ((r = enqueue_decode_step(e))) {
      return r;
    }
    e->host_pos += 1;
    // bound in-flight work: sync every 64 steps to keep the queue shallow;
    // same cadence re-checks the chunk-count threshold as context grows
    if ((s & 63) == 63) {
      HIP_TRY(hipStreamSynchronize(e->stream));
      if ((r = retune_nchunk())) return r;
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
int sampling_args_err(const char* who, float temperature, float top_p,
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

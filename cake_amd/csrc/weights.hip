// Weights of the cake_hip engine: the safetensors loader (single file,
// sharded index or directory; split and fused checkpoints; bf16, fp8 and
// gptq projections) and cake_hip_init_random.  Both walk a layer's four Proj
// records (engine_internal.h) and take format and sizes from them.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "engine_internal.h"
#include "json.hpp"

// ---------------------------------------------------------------------------
// weight loading
// ---------------------------------------------------------------------------
struct StTensor {
  std::string dtype;
  std::vector<long> shape;
  size_t off0 = 0, off1 = 0;
  size_t elems() const {
    size_t n = 1;
    for (long d : shape) n *= (size_t)d;
    return n;
  }
  bool is2d(size_t a, size_t b) const {
    return shape.size() == 2 && (size_t)shape[0] == a && (size_t)shape[1] == b;
  }
  std::string shape_str() const {  // "a, b" for messages
    std::string s;
    for (long d : shape) s += (s.empty() ? "" : ", ") + std::to_string(d);
    return s;
  }
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
// n elements of an F32 / F16 / BF16 tensor (possibly unaligned) as f32, every
// one exact; false for any other dtype
static bool st_to_f32(const StTensor& t, const char* filebase, size_t n,
                      std::vector<float>* out) {
  const char* src = filebase + t.off0;
  out->resize(n);
  if (t.dtype == "F32") {
    memcpy(out->data(), src, n * 4);
  } else if (t.dtype == "F16") {
    for (size_t i = 0; i < n; ++i) (*out)[i] = f16_at(src, i);
  } else if (t.dtype == "BF16") {
    for (size_t i = 0; i < n; ++i) {
      u16 h;
      memcpy(&h, src + i * 2, 2);
      (*out)[i] = b2f_host(h);
    }
  } else {
    return false;
  }
  return true;
}

// GPTQ checkpoint layout -> the device layout of kernels_w4.hip, for one
// projection (the loader and the w4 op entries both come through here).
//   qw (K/8, N) i32: nibble b of word [r, j] is q(k = 8r + b, j)
//   qz (G, N/8) i32: nibble j % 8 of word [gi, j / 8] is z(gi, j)
//   sc (G, N)   f32 (f16-representable)
// -> W (N, K/8): row j contiguous over k, same nibble order inside a word;
//    sz (N, G, 2) = {s, -(z+1)*s}: z + 1 may be 16 and does not wrap, words
//    are read as unsigned so the top nibble is (w >> 28) & 0xF.
void w4_repack(const int32_t* qw, const int32_t* qz, const float* sc,
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
  const size_t n = t.elems();
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
  const size_t n = t.elems();
  if (n != expect_elems)
    return set_err(5, "scale_inv shape mismatch: got %zu want %zu", n,
                   expect_elems);
  std::vector<float> tmp;
  if (!st_to_f32(t, filebase, n, &tmp))
    return set_err(5, "scale_inv dtype %s unsupported", t.dtype.c_str());
  HIP_TRY(hipMemcpy(dst, tmp.data(), n * 4, hipMemcpyHostToDevice));
  return 0;
}

static int upload_weight(cake_engine* e, u16* dst, const char* filebase,
                         const StTensor& t, size_t expect_elems) {
  const size_t n = t.elems();
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

// A gemma3 norm row: bf16((1 + w) * mul), the sum and the product in f32 and
// one rounding (HF's Gemma3RMSNorm multiplies by 1 + w.float(); folding it
// here leaves every norm kernel its plain bf16 weight row).  mul is 1, or for
// q_norm the score-scale fold sqrt(head_dim / query_pre_attn_scalar).
static int upload_norm_1pw(cake_engine* e, u16* dst, const char* filebase,
                           const StTensor& t, size_t expect, float mul) {
  if (t.elems() != expect)
    return set_err(5, "tensor shape mismatch: got %zu want %zu elems",
                   t.elems(), expect);
  std::vector<float> w;
  if (!st_to_f32(t, filebase, expect, &w))
    return set_err(5, "unsupported safetensors dtype %s", t.dtype.c_str());
  std::vector<u16> tmp(expect);
  for (size_t i = 0; i < expect; ++i) {
    union { float f; unsigned u; } v{(1.0f + w[i]) * mul};
    unsigned r = ((v.u & 0x7fffffffu) > 0x7f800000u)
                     ? 0x7fc00000u
                     : v.u + 0x7fffu + ((v.u >> 16) & 1u);
    tmp[i] = (u16)(r >> 16);
  }
  HIP_TRY(hipMemcpy(dst, tmp.data(), expect * 2, hipMemcpyHostToDevice));
  return 0;
}

// one projection's bias vector -> f32 (every source dtype widens exactly)
static int upload_bias(cake_engine* e, float* dst, const char* filebase,
                       const StTensor& t, const std::string& name,
                       size_t expect) {
  if (t.shape.size() != 1 || (size_t)t.shape[0] != expect)
    return set_err(5, "%s: shape (%s), expected (%zu)", name.c_str(),
                   t.shape_str().c_str(), expect);
  std::vector<float> tmp;
  if (!st_to_f32(t, filebase, expect, &tmp))
    return set_err(5, "%s: dtype %s, expected F32, F16 or BF16", name.c_str(),
                   t.dtype.c_str());
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
  StTensor t;
  // gptq tensors P.{qweight,qzeros,scales} (`rows` out, p.K in, group p.g;
  // g_idx is ignored, as gptq.rs does) -> rows [row0, row0 + rows) of p,
  // repacked out-major
  auto load_w4 = [&](const std::string& P, const Proj& p, size_t row0,
                     size_t rows) -> int {
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
    const size_t N = rows, K = p.K, G = K / p.g;
    auto bad = [&](const char* suf, const StTensor& s, const char* dt,
                   size_t a, size_t b) {
      return set_err(5, "%s%s: %s (%s), expected %s (%zu, %zu)", P.c_str(),
                     suf, s.dtype.c_str(), s.shape_str().c_str(), dt, a, b);
    };
    if (tq.dtype != "I32" || !tq.is2d(K / 8, N))
      return bad(".qweight", tq, "I32", K / 8, N);
    if (tz.dtype != "I32" || !tz.is2d(G, N / 8))
      return bad(".qzeros", tz, "I32", G, N / 8);
    std::vector<float> sc;
    if (!ts.is2d(G, N) || !st_to_f32(ts, base, G * N, &sc))
      return bad(".scales", ts, "F16", G, N);
    std::vector<int32_t> qw(K / 8 * N), qz(G * (N / 8));
    memcpy(qw.data(), base + tq.off0, qw.size() * 4);
    memcpy(qz.data(), base + tz.off0, qz.size() * 4);
    std::vector<u32> W(N * (K / 8));
    std::vector<float> sz(N * G * 2);
    w4_repack(qw.data(), qz.data(), sc.data(), N, K, p.g, W.data(), sz.data());
    HIP_TRY(hipMemcpy(p.w4() + row0 * (K / 8), W.data(), W.size() * 4,
                      hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(p.aux + row0 * G * 2, sz.data(), sz.size() * 4,
                      hipMemcpyHostToDevice));
    return 0;
  };
  // The text model's tensor prefix.  A gemma3 checkpoint saved from the
  // multimodal class nests it (and carries vision tensors, which nothing
  // here asks for): the first candidate any tensor of this file starts with.
  std::string mp = "model.";
  if (c.gemma3)
    for (const char* cand : {"model.language_model.", "language_model.model.",
                             "model."}) {
      const std::string cs(cand);
      bool hit = false;
      for (auto& kv : tensors)
        if (kv.first.compare(0, cs.size(), cs) == 0 &&
            (kv.first.compare(cs.size(), 7, "layers.") == 0 ||
             kv.first.compare(cs.size(), 13, "embed_tokens.") == 0 ||
             kv.first.compare(cs.size(), 5, "norm.") == 0)) {
          hit = true;
          break;
        }
      if (hit) {
        mp = cs;
        break;
      }
    }
  // a plain norm row, or gemma3's (1 + w) form
  auto upload_norm = [&](u16* dst, size_t n, float mul) -> int {
    return c.gemma3 ? upload_norm_1pw(e, dst, base, t, n, mul)
                    : upload_weight(e, dst, base, t, n);
  };
  if (e->has_embed()) {
    LOADW(mp + "embed_tokens.weight", upload_weight(e, e->embed, base, t, V * H));
  }
  if (e->has_head()) {
    LOADW(mp + "norm.weight", upload_norm(e->norm_w, H, 1.f));
    if (!(c.tied && e->has_embed())) {
      std::string name = c.tied ? mp + "embed_tokens.weight"
                                : "lm_head.weight";
      LOADW(name, upload_weight(e, e->lm_head, base, t, V * H));
    }
  }
  // A projection is made of checkpoint tensors, each filling rows [row0,
  // row0 + rows) of the device tensor: q|k|v (attention.rs:109-114) and
  // gate|up (mlp.rs:38-46) concatenate along the rows, scale rows included.
  // phi3 ships qkv_proj and gate_up_proj already in that layout
  // (phi4/config.rs:88-89); its bf16 loader names the fused tensor when the
  // shape is off, and a checkpoint with split names fails on the fused name.
  struct Part {
    const char* name;
    size_t row0, rows;
    bool fused = false;
  };
  const std::vector<Part> split[4] = {
      {{"self_attn.q_proj", 0, Sq},
       {"self_attn.k_proj", Sq, Skv},
       {"self_attn.v_proj", Sq + Skv, Skv}},
      {{"self_attn.o_proj", 0, H}},
      {{"mlp.gate_proj", 0, I}, {"mlp.up_proj", I, I}},
      {{"mlp.down_proj", 0, H}}};
  const std::vector<Part> fused[4] = {
      {{"self_attn.qkv_proj", 0, Sq + 2 * Skv, true}},
      {{"self_attn.o_proj", 0, H}},
      {{"mlp.gate_up_proj", 0, 2 * I, true}},
      {{"mlp.down_proj", 0, H}}};
  for (int li = e->lo; li < e->hi; ++li) {
    LayerDev& l = e->L[li - e->lo];
    char p[128];
    snprintf(p, sizeof p, "layers.%d.", li);
    std::string pre = mp + p;
    LOADW(pre + "input_layernorm.weight", upload_norm(l.rms1, H, 1.f));
    if (c.gemma3) {  // rms2 is the norm ahead of the MLP in every family
      LOADW(pre + "post_attention_layernorm.weight", upload_norm(l.post1, H, 1.f));
      LOADW(pre + "pre_feedforward_layernorm.weight", upload_norm(l.rms2, H, 1.f));
      LOADW(pre + "post_feedforward_layernorm.weight", upload_norm(l.post2, H, 1.f));
    } else {
      LOADW(pre + "post_attention_layernorm.weight", upload_weight(e, l.rms2, base, t, H));
    }
    const Proj* projs[4] = {&l.qkv, &l.o, &l.gu, &l.down};
    for (int pi = 0; pi < 4; ++pi) {
      const Proj& pj = *projs[pi];
      const size_t K = pj.K;
      const std::vector<Part>& parts = (c.fused_ckpt ? fused : split)[pi];
      for (const Part& pt : parts) {
        const std::string P = pre + pt.name;
        if (pj.fmt == W_GPTQ) {
          int r = load_w4(P, pj, pt.row0, pt.rows);
          if (r) return r;
        } else if (pj.fmt == W_FP8) {
          LOADW(P + ".weight", upload_weight_u8(e, pj.fp8() + pt.row0 * K, base, t, pt.rows * K));
        } else {
          auto upload = [&]() -> int {
            if (pt.fused && !t.is2d(pt.rows, K))
              return set_err(5, "%s.weight: shape (%s), expected (%zu, %zu)",
                             P.c_str(), t.shape_str().c_str(), pt.rows, K);
            return upload_weight(e, pj.bf16() + pt.row0 * K, base, t, pt.rows * K);
          };
          LOADW(P + ".weight", upload());
        }
      }
      // fp8: blockwise scale_inv (fp8.rs:42-64) at the block-row offset
      if (pj.fmt == W_FP8)
        for (const Part& pt : parts)
          LOADW(pre + pt.name + ".weight_scale_inv",
                upload_scale(e, pj.aux + (pt.row0 / 128) * (K / 128), base, t, (pt.rows / 128) * (K / 128)));
    }
    if (c.qkv_bias) {
      // qwen2, every weight format alike: required F32/F16/BF16 vectors at
      // the projection's row offset of the fused bias (attention.rs:95-104);
      // every other bias in a checkpoint is ignored
      for (const Part& pt : split[0]) {
        const std::string name = pre + pt.name + ".bias";
        LOADW(name, upload_bias(e, l.bqkv + pt.row0, base, t, name, pt.rows));
      }
    }
    if (c.qk_norm) {
      LOADW(pre + "self_attn.q_norm.weight", upload_norm(l.qnorm, hd, c.q_fold()));
      LOADW(pre + "self_attn.k_norm.weight", upload_norm(l.knorm, hd, 1.f));
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
  const size_t H = c.hidden, V = c.vocab;
  const size_t hd = c.hd(), Sq = c.sq(), Skv = c.skv();
  // Salts derive from the tensor's IDENTITY (absolute layer index + slot),
  // not fill order, so a sharded engine's layer k gets bit-identical
  // weights to a monolithic engine's layer k — the multi-rank pipeline
  // parity tests depend on this.
  auto salted = [&](uint64_t salt) { return seed + 0x1000193u * salt; };
  if (e->has_embed())
    launch_fill_random(e->embed, V * H, salted(1), scale, e->stream);
  if (e->has_head()) {
    launch_fill_const(e->norm_w, H, 1.0f, e->stream);
    if (!(c.tied && e->has_embed()))
      launch_fill_random(e->lm_head, V * H, salted(2), scale, e->stream);
  }
  std::vector<float> host;
  // weights by format, then the companion tensor (host-side, by index)
  auto fill_proj = [&](const Proj& p, uint64_t s) {
    const size_t n = p.aux_elems();
    host.resize(n);
    if (p.fmt == W_BF16) {
      launch_fill_random(p.bf16(), p.elems(), s, scale, e->stream);
      return;
    }
    if (p.fmt == W_FP8) {
      launch_fill_random_u8(p.fp8(), p.elems(), s, e->stream);
      for (size_t i = 0; i < n; ++i)
        host[i] = 3e-4f + 2e-4f * (float)((i * 2654435761u) % 1000) / 1000.f;
    } else {
      // random nibbles, stored zero 7 (z + 1 = 8: q - 8 in [-8, 7]) and
      // f16-representable scales around scale / 8 (+-20 %, by index), so the
      // weights spread over about +-scale like the bf16 init
      launch_fill_random_u32(p.w4(), p.elems() / 8, s, e->stream);
      for (size_t i = 0; i < n / 2; ++i) {
        const float f =
            0.8f + 0.4f * (float)((i * 2654435761u) % 1000) / 1000.f;
        const float sv = (float)(_Float16)(scale * 0.125f * f);
        host[2 * i] = sv;
        host[2 * i + 1] = -8.f * sv;
      }
    }
    hipMemcpy(p.aux, host.data(), n * 4, hipMemcpyHostToDevice);
  };
  for (auto& l : e->L) {
    const uint64_t base = 16 + (uint64_t)l.idx * 8;  // slots base + 0..4
    launch_fill_const(l.rms1, H, 1.0f, e->stream);
    launch_fill_const(l.rms2, H, 1.0f, e->stream);
    const Proj* projs[4] = {&l.qkv, &l.o, &l.gu, &l.down};
    for (int i = 0; i < 4; ++i) fill_proj(*projs[i], salted(base + i));
    if (l.qnorm) {
      // gemma3: w = 0, so 1 + w = 1, times the score-scale fold on q
      launch_fill_const(l.qnorm, hd, c.gemma3 ? c.q_fold() : 1.0f, e->stream);
      launch_fill_const(l.knorm, hd, 1.0f, e->stream);
    }
    if (l.post1) {
      launch_fill_const(l.post1, H, 1.0f, e->stream);
      launch_fill_const(l.post2, H, 1.0f, e->stream);
    }
    if (l.bqkv) {
      // slot 4 of the layer: q and k rows ~uniform(+-3) (real qwen2 q/k
      // biases are large), v rows ~uniform(+-0.25); splitmix64 of the index
      const uint64_t bs = salted(base + 4);
      host.resize(Sq + 2 * Skv);
      for (size_t i = 0; i < host.size(); ++i) {
        uint64_t z = bs + 0x9e3779b97f4a7c15ull * (uint64_t)(i + 1);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        z ^= z >> 31;
        const float u = (float)(z >> 40) * 0x1p-23f - 1.f;  // [-1, 1)
        host[i] = u * (i < Sq + Skv ? 3.f : 0.25f);
      }
      hipMemcpy(l.bqkv, host.data(), host.size() * 4, hipMemcpyHostToDevice);
    }
  }
  HIP_TRY(hipStreamSynchronize(e->stream));
  e->weights_ready = true;
  return 0;
}

// The op-level surface of the C-ABI (include/cake_hip.h): every
// cake_hip_op_* entry, which runs one launch wrapper of kernels.h on private
// buffers for the kernel parity tests, and the host-only *_dispatch queries,
// which report the kernel choices the engine makes.
#include <algorithm>
#include <cstring>

#include "engine_internal.h"

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
  static thread_local std::vector<void*> mem;
  if (ctx.cap < elems) {
    for (void* p : mem) hipFree(p);
    mem.clear();
    ctx.cap = elems;
    ALLOC(mem, ctx.a, u16, elems);
    ALLOC(mem, ctx.b, u16, elems);
    ALLOC(mem, ctx.c, u16, elems);
    ALLOC(mem, ctx.fa, float, elems);
    ALLOC(mem, ctx.fb, float, elems);
    ALLOC(mem, ctx.fc, float, elems);
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
  return dev_alloc(b.ptrs, p, bytes);
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
  if (hd != 256 && (hd < 8 || hd > 128 || hd % 8 != 0))
    return set_err(5, "%s: hd %d must be a multiple of 8 in [8,128], or 256",
                   who, hd);
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
  // at most one of split / deep; hd 256 -> the MFMA-256 kernel {1, 4} or the
  // plain one {0, 0}; any other hd -> the generic kernel only
  const bool ok =
      hd == 256 ? (!split && !deep &&
                   ((pfv == 1 && nw == 4) || (pfv == 0 && nw == 0))) :
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

// q-heads per block of the decode-attention kernel at this geometry (host
// only): hd 256 -> attn256_group under CAKE_ATTN256_GB; hd 128 -> the grouped
// kernel's 4|2|1; anything else, or a per-head route, 1.
extern "C" int cake_hip_attn_decode_group(int nh, int nkv, int hd) {
  if (nh <= 0 || nkv <= 0 || nh % nkv != 0) return 1;
  if (hd == 256) return attn256_group(nh, nkv);
  const int gy = attn_decode_grid_y(nh, nkv, hd);
  return gy > 0 ? nh / gy : 1;
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
  out[6] = c.w4       ? CAKE_HIP_FAM_GATEUP_W4
           : c.fp8    ? CAKE_HIP_FAM_GATEUP_FP8
           : c.gemma3 ? CAKE_HIP_FAM_GATEUP_GELU
                      : CAKE_HIP_FAM_GATEUP;
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

// ---- gemma3 op entries (kernels_gemma.hip) ---------------------------------
// x (S, H) = bf16(x + bf16(rms_norm(t) * w)) in place, through the launcher
// both routes use: S == 1 is the decode launch (one wide block), S > 1 the
// prefill one.
extern "C" int cake_hip_op_postnorm_add(int S, int H, float eps,
                                        const float* x, const float* t,
                                        const float* w, float* out,
                                        int device) {
  const char* who = "op_postnorm_add";
  if (H < 8 || H > 16384 || H % 8 != 0)
    return set_err(5, "%s: H %d must be a multiple of 8 in [8,16384]", who, H);
  if (S < 1 || S > 4096) return set_err(5, "%s: S %d outside [1,4096]", who, S);
  if (!x || !t || !w || !out) return set_err(5, "%s: null argument", who);
  OpBufs b;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipStreamCreate(&b.s));
  int r;
  const size_t n = (size_t)S * H;
  u16 *dx, *dt, *dw, *dout;
  if ((r = ob_up16(b, x, n, &dx))) return r;
  if ((r = ob_up16(b, t, n, &dt))) return r;
  if ((r = ob_up16(b, w, H, &dw))) return r;
  if ((r = ob_sent16(b, n + OPG, &dout))) return r;
  HIP_TRY(hipMemcpyAsync(dout, dx, n * 2, hipMemcpyDeviceToDevice, b.s));
  launch_postnorm_add(dout, dt, dw, S, H, eps, b.s);
  HIP_TRY(hipGetLastError());
  return ob_down16(b, dout, n + OPG, out);
}

// The bf16 gate-up GEMV with the GELU-tanh gate; arguments as the bf16 form
// of cake_hip_op_gemv_gateup.
extern "C" int cake_hip_op_gemv_gateup_gelu(int I, int K, int rows,
                                            const float* x, const float* w,
                                            const float* nw, float eps,
                                            float* out, int device) {
  const char* who = "op_gemv_gateup_gelu";
  if (I < 1) return set_err(5, "%s: I %d < 1", who, I);
  if (K < 8 || K % 8 != 0 || K > 16384)
    return set_err(5, "%s: K must be a multiple of 8 in [8,16384] (got %d)",
                   who, K);
  if (!x || !w || !out) return set_err(5, "%s: x, w and out are required", who);
  if (rows != 0 && rows != 4 && rows != 8)
    return set_err(5, "%s: rows %d not in {0,4,8}", who, rows);
  OpBufs b;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipStreamCreate(&b.s));
  int r;
  u16 *dx, *dw, *dnw = nullptr, *dout;
  if ((r = ob_up16(b, x, K, &dx))) return r;
  if (nw && (r = ob_up16(b, nw, K, &dnw))) return r;
  if ((r = ob_sent16(b, (size_t)I + OPG, &dout))) return r;
  if ((r = ob_up16(b, w, (size_t)2 * I * K, &dw))) return r;
  launch_gemv_gateup_gelu(dw, dx, dout, dnw, eps, I, K, rows, b.s);
  HIP_TRY(hipGetLastError());
  return ob_down16(b, dout, (size_t)I + OPG, out);
}

extern "C" int cake_hip_op_gelu_mul_rows(int S, int I, const float* gu,
                                         float* out, int device) {
  const char* who = "op_gelu_mul_rows";
  if (S < 1 || S > 4096 || I < 1)
    return set_err(5, "%s: S %d in [1,4096] and I %d >= 1", who, S, I);
  if (!gu || !out) return set_err(5, "%s: gu and out are required", who);
  OpBufs b;
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipStreamCreate(&b.s));
  int r;
  u16 *dgu, *dout;
  if ((r = ob_up16(b, gu, (size_t)S * 2 * I, &dgu))) return r;
  if ((r = ob_sent16(b, (size_t)S * I + OPG, &dout))) return r;
  launch_gelu_mul_rows(dgu, dout, S, I, b.s);
  HIP_TRY(hipGetLastError());
  return ob_down16(b, dout, (size_t)S * I + OPG, out);
}

// The scaled embedding gathers; mode 0: launch_embed_rows_scaled on S ids,
// 1: launch_embed_token_scaled on one id.  Other arguments as
// cake_hip_op_embed.
extern "C" int cake_hip_op_embed_scaled(int Vt, int H, int S, int mode,
                                        const float* table,
                                        const uint32_t* ids, float* out,
                                        int device) {
  const char* who = "op_embed_scaled";
  if (mode < 0 || mode > 1) return set_err(5, "%s: mode %d", who, mode);
  if (H < 8 || H > 16384 || H % 8 != 0)
    return set_err(5, "%s: H %d must be a multiple of 8 in [8,16384]", who, H);
  if (Vt < 1 || Vt > (1 << 20))
    return set_err(5, "%s: Vt %d outside [1,%d]", who, Vt, 1 << 20);
  if (S < 1 || S > 4096 || (mode != 0 && S != 1))
    return set_err(5, "%s: S %d (rows: 1..4096, token: 1)", who, S);
  if (!table || !ids || !out) return set_err(5, "%s: null argument", who);
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
  if ((r = ob_up16(b, table, (size_t)Vt * H, &dt))) return r;
  if ((r = ob_upf32(b, ids, (size_t)S * 4, &dids))) return r;
  if ((r = ob_sent16(b, n + OPG, &dout))) return r;
  if (mode == 0)
    launch_embed_rows_scaled(dt, (const u32*)dids, dout, S, H, b.s);
  else
    launch_embed_token_scaled(dt, (const u32*)dids, dout, H, b.s);
  HIP_TRY(hipGetLastError());
  return ob_down16(b, dout, n + OPG, out);
}

#include "kernels_common.h"
#include "kernels.h"


// ---------------------------------------------------------------------------
// RoPE + KV store.  HF half-rotation (backends/mod.rs:470-477):
//   out[i] = x1*c - x2*s ; out[i+half] = x2*c + x1*s, cos/sin row = position.
// Decode: one token at *pos; K/V written into the preallocated cache at slot
// *pos (replaces cache.rs:195-196 cat).  qkv layout: (Sq | Skv | Skv) per row.
// grid = nh + 2*nkv blocks.
// ---------------------------------------------------------------------------
// Optional fused per-head QK-norm (attention.rs:202-215): applied to the
// head row before the rotation, re-quantized to bf16 so it matches the
// separate rmsnorm-kernel path bit-exactly.  One wave per head.
// Optional q|k|v projection bias (qwen2; `bias` = the fused (nh+2*nkv)*hd f32
// row, or null): every raw value gets float(raw) + bias[row] in f32, ahead of
// the rotation for q and k and ahead of the store for v, with no rounding in
// between.  A null bias leaves every output bit as it was.
__device__ inline float head_norm_scale(const u16* row, int hd, float eps) {
  float ss = 0.f;
  for (int i = threadIdx.x; i < hd; i += 64) {
    float f = b2f(row[i]);
    ss += f * f;
  }
  ss = wave_sum(ss);
  ss = __shfl(ss, 0, WAVE);
  return rsqrtf(ss / (float)hd + eps);
}
__device__ inline float nrm(const u16* row, const u16* w, int i, float sc,
                            bool on) {
  float v = b2f(row[i]);
  return on ? b2f(f2b(v * sc * b2f(w[i]))) : v;
}

__global__ void k_rope_store_decode(u16* __restrict__ qkv,
                                    u16* __restrict__ kc, u16* __restrict__ vc,
                                    u16* __restrict__ vtc,
                                    const float* __restrict__ cost,
                                    const float* __restrict__ sint,
                                    const int* __restrict__ pos, int nh,
                                    int nkv, int hd, int rd, int max_seq,
                                    const u16* __restrict__ qn,
                                    const u16* __restrict__ kn, float eps,
                                    const float* __restrict__ bias) {
  const int b = blockIdx.x;
  const int p = *pos;
  const int half = rd / 2;
  const float* c = cost + (size_t)p * half;
  const float* s = sint + (size_t)p * half;
  // this head's slice of the fused q|k|v projection bias (qwen2), or null
  const float* br = bias ? bias + (size_t)b * hd : nullptr;
  if (b < nh) {                       // [qk-norm +] rope q head in place
    u16* q = qkv + (size_t)b * hd;
    const bool on = qn != nullptr;
    const float sc = on ? head_norm_scale(q, hd, eps) : 1.f;
    for (int i = threadIdx.x; i < half; i += blockDim.x) {
      float x1 = nrm(q, qn, i, sc, on), x2 = nrm(q, qn, i + half, sc, on);
      if (br) {
        x1 += br[i];
        x2 += br[i + half];
      }
      q[i] = f2b(x1 * c[i] - x2 * s[i]);
      q[i + half] = f2b(x2 * c[i] + x1 * s[i]);
    }
  } else if (b < nh + nkv) {          // [qk-norm +] rope k head -> slot p
    const int h = b - nh;
    u16* k = qkv + (size_t)(nh + h) * hd;
    u16* dst = kc + ((size_t)h * max_seq + p) * hd;
    const bool on = kn != nullptr;
    const float sc = on ? head_norm_scale(k, hd, eps) : 1.f;
    for (int i = threadIdx.x; i < half; i += blockDim.x) {
      float x1 = nrm(k, kn, i, sc, on), x2 = nrm(k, kn, i + half, sc, on);
      if (br) {
        x1 += br[i];
        x2 += br[i + half];
      }
      dst[i] = f2b(x1 * c[i] - x2 * s[i]);
      dst[i + half] = f2b(x2 * c[i] + x1 * s[i]);
    }
    for (int i = rd + threadIdx.x; i < hd; i += blockDim.x)
      dst[i] = br ? f2b(b2f(k[i]) + br[i]) : k[i];
  } else {                            // v head -> cache slot p (+ V^T)
    const int h = b - nh - nkv;
    const u16* v = qkv + (size_t)(nh + nkv + h) * hd;
    u16* dst = vc + ((size_t)h * max_seq + p) * hd;
    u16* dstt = vtc + (size_t)h * hd * max_seq + p;
    for (int i = threadIdx.x; i < hd; i += blockDim.x) {
      const u16 e = br ? f2b(b2f(v[i]) + br[i]) : v[i];
      dst[i] = e;
      dstt[(size_t)i * max_seq] = e;
    }
  }
}

// Prefill: S tokens at positions pos0..pos0+S-1; qkv is (S, Sq+2*Skv).
// grid = (nh + 2*nkv, S)
__global__ void k_rope_store_prefill(u16* __restrict__ qkv,
                                     u16* __restrict__ kc, u16* __restrict__ vc,
                                     u16* __restrict__ vtc,
                                     const float* __restrict__ cost,
                                     const float* __restrict__ sint, int pos0,
                                     int nh, int nkv, int hd, int rd,
                                     int max_seq, int qkv_stride,
                                     const u16* __restrict__ qn,
                                     const u16* __restrict__ kn, float eps,
                                     const float* __restrict__ bias) {
  const int b = blockIdx.x;
  const int sidx = blockIdx.y;
  const int p = pos0 + sidx;
  const int half = rd / 2;
  const float* c = cost + (size_t)p * half;
  const float* s = sint + (size_t)p * half;
  u16* row = qkv + (size_t)sidx * qkv_stride;
  const float* br = bias ? bias + (size_t)b * hd : nullptr;
  if (b < nh) {
    u16* q = row + (size_t)b * hd;
    const bool on = qn != nullptr;
    const float sc = on ? head_norm_scale(q, hd, eps) : 1.f;
    for (int i = threadIdx.x; i < half; i += blockDim.x) {
      float x1 = nrm(q, qn, i, sc, on), x2 = nrm(q, qn, i + half, sc, on);
      if (br) {
        x1 += br[i];
        x2 += br[i + half];
      }
      q[i] = f2b(x1 * c[i] - x2 * s[i]);
      q[i + half] = f2b(x2 * c[i] + x1 * s[i]);
    }
  } else if (b < nh + nkv) {
    const int h = b - nh;
    u16* k = row + (size_t)(nh + h) * hd;
    u16* dst = kc + ((size_t)h * max_seq + p) * hd;
    const bool on = kn != nullptr;
    const float sc = on ? head_norm_scale(k, hd, eps) : 1.f;
    for (int i = threadIdx.x; i < half; i += blockDim.x) {
      float x1 = nrm(k, kn, i, sc, on), x2 = nrm(k, kn, i + half, sc, on);
      if (br) {
        x1 += br[i];
        x2 += br[i + half];
      }
      dst[i] = f2b(x1 * c[i] - x2 * s[i]);
      dst[i + half] = f2b(x2 * c[i] + x1 * s[i]);
    }
    for (int i = rd + threadIdx.x; i < hd; i += blockDim.x)
      dst[i] = br ? f2b(b2f(k[i]) + br[i]) : k[i];
  } else {
    const int h = b - nh - nkv;
    const u16* v = row + (size_t)(nh + nkv + h) * hd;
    u16* dst = vc + ((size_t)h * max_seq + p) * hd;
    u16* dstt = vtc + (size_t)h * hd * max_seq + p;
    for (int i = threadIdx.x; i < hd; i += blockDim.x) {
      const u16 e = br ? f2b(b2f(v[i]) + br[i]) : v[i];
      dst[i] = e;
      dstt[(size_t)i * max_seq] = e;
    }
  }
}

// ---------------------------------------------------------------------------
// Decode attention (attention.rs:300-343 semantics, GQA, f32 softmax), over
// the preallocated cache.  Split-KV in ONE launch: grid (NCHUNK, nh); each
// block computes an online-softmax partial over a contiguous slice of
// positions into ws[h][chunk] = {o[hd], m, l}; the LAST-arriving block of a
// head combines the partials (agent-scope release/acquire + arrival counter
// per cdna_hip_programming.md §6 Guideline 16 — placement-independent).
// cnt[nh] is zeroed once per chunk count, not per launch: the election is
// modulo nchunk (tests/test_attn_ops_gpu.py repeats launches on one zeroing).
// K/V row loads: 64 lanes x 4 B = one coalesced 256 B transaction.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_attn_decode_fused(
    const u16* __restrict__ q,         // (nh*hd), post-rope
    const u16* __restrict__ kc, const u16* __restrict__ vc,
    const int* __restrict__ pos, float* __restrict__ ws,
    u32* __restrict__ cnt, u16* __restrict__ outbuf, int nh, int nkv,
    int hd, int max_seq, int nchunk, int window) {
  const int h = blockIdx.y;
  const int chunk = blockIdx.x;
  const int n = *pos + 1;
  // sliding window (cache.rs:173-205 semantics): attention spans only the
  // last `window` positions; chunks partition [lo, n)
  const int lo = (window > 0 && n > window) ? n - window : 0;
  const int cs = (n - lo + nchunk - 1) / nchunk;
  const int start = lo + chunk * cs;
  const int end = min(start + cs, n);
  const int kvh = h / (nh / nkv);
  const int t = threadIdx.x, wid = t / WAVE, lane = t % WAVE;
  const int e0 = 2 * lane;             // dims (2*lane, 2*lane+1)
  const bool act = e0 + 1 < hd;
  float* wsrow = ws + ((size_t)h * nchunk + chunk) * (hd + 4);
#define WS_STORE(p, v)                                                     \
  __hip_atomic_store((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define WS_LOAD(p)                                                         \
  __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

  // Tiled two-phase structure: the serial online-softmax chain runs once
  // per TILE (128 positions), not per position — phase A computes a tile's
  // scores with 16-B coalesced K loads (16 lanes per position), phase B is
  // a block-wide softmax step, phase C accumulates PV with coalesced,
  // mutually independent V loads.  The per-position serial chain of the
  // naive version measured 128 GB/s at n=2048.
  __shared__ float sm[4], sl[4];
  __shared__ float so[4][128 + 8];
  __shared__ float stile[128];
  const float scale = rsqrtf((float)hd);
  const u16* kbase = kc + (size_t)kvh * max_seq * hd;
  const u16* vbase = vc + (size_t)kvh * max_seq * hd;
  // phase-A per-thread q slice: dims (t&15)*8 .. +8
  const int dgrp = t & 15;
  float qa[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int d = dgrp * 8 + j;
    qa[j] = d < hd ? b2f(q[(size_t)h * hd + d]) : 0.f;
  }
  float m = -INFINITY, l = 0.f, o0 = 0.f, o1 = 0.f;
  const int TILE = 128;
  // Loads below are UNGUARDED (addresses clamped into the cache, results
  // zeroed/-INF'd by weight instead): a load inside an `if (p < end)`
  // block costs hipcc a vmcnt(0) drain per unrolled iteration (the .s
  // showed 24 of them = zero memory-level parallelism, 0.5 TB/s at 8k
  // context); straight-line loads issue back-to-back and wait once.
  // Clamped addresses stay inside this kv-head's cache rows, and qa[] is
  // zero beyond hd, so out-of-range lanes contribute exact zeros.
  const int doff = min(dgrp * 8, hd - 8);
  const int eoff = min(e0, hd - 2);
  // K rows for the CURRENT sub-tile live in registers (ka) so the next
  // sub-tile's loads can issue during phase C and ride the memory system
  // behind C's loads — registers survive the barriers, and vmcnt retires
  // in FIFO order so C's counted waits drain the prefetch for free.
  short8 ka[TILE / 16];
  auto issue_k = [&](int s0) {
#pragma unroll
    for (int pass = 0; pass < TILE / 16; ++pass) {
      const int pc = max(0, min(s0 + pass * 16 + (t >> 4), end - 1));
      ka[pass] =
          *reinterpret_cast<const short8*>(kbase + (size_t)pc * hd + doff);
    }
  };
  if (start < end) issue_k(start);
  for (int sub0 = start; sub0 < end; sub0 += TILE) {
    // --- phase A: scores for [sub0, sub0+TILE) --------------------------
    // 256 threads = 16 positions per pass (16 lanes per position, each
    // holding 16 B of the K row in ka)
#pragma unroll
    for (int pass = 0; pass < TILE / 16; ++pass) {
      const int p = sub0 + pass * 16 + (t >> 4);
      float d = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) d = fmaf(b2f((u16)ka[pass][j]), qa[j], d);
      // reduce across the 16 lanes of this position
#pragma unroll
      for (int off = 8; off >= 1; off >>= 1) d += __shfl_xor(d, off, 16);
      if (dgrp == 0)
        stile[pass * 16 + (t >> 4)] = (p < end) ? d * scale : -INFINITY;
    }
    __syncthreads();
    // --- phase B: block softmax step over the tile ----------------------
    float lm = -INFINITY;
    for (int i = t; i < TILE; i += blockDim.x) lm = fmaxf(lm, stile[i]);
    lm = wave_max(lm);
    if (lane == 0) sm[wid] = lm;
    __syncthreads();
    const float tmax = fmaxf(fmaxf(sm[0], sm[1]), fmaxf(sm[2], sm[3]));
    const float mnew = fmaxf(m, tmax);
    const float alpha = (mnew == -INFINITY) ? 0.f : __expf(m - mnew);
    float psum = 0.f;
    for (int i = t; i < TILE; i += blockDim.x) {
      const float sv = stile[i];
      const float e = (sv == -INFINITY) ? 0.f : __expf(sv - mnew);
      stile[i] = e;
      psum += e;
    }
    psum = wave_sum(psum);
    if (lane == 0) sl[wid] = psum;
    __syncthreads();
    l = l * alpha + sl[0] + sl[1] + sl[2] + sl[3];
    o0 *= alpha;
    o1 *= alpha;
    m = mnew;
    // next sub-tile's K loads issue here, ahead of phase C's own loads —
    // C's waits retire them for free (FIFO vmcnt), so phase A of the next
    // iteration starts with its data already on chip
    if (sub0 + TILE < end) issue_k(sub0 + TILE);
    // --- phase C: PV accumulate (thread t: dims 2*lane, position residue
    // wid mod 4).  Batches of 16 unguarded u32 loads (both dims in one
    // load) issue together, then one wait covers all sixteen; the softmax
    // weight is read from LDS at consume time (cheap, and keeps the
    // register count inside 3-waves/SIMD occupancy).
#pragma unroll
    for (int g = 0; g < TILE / 4; g += 16) {
      unsigned int vv[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int pc = max(0, min(sub0 + (g + u) * 4 + wid, end - 1));
        vv[u] = *reinterpret_cast<const unsigned int*>(
            vbase + (size_t)pc * hd + eoff);
      }
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int po = (g + u) * 4 + wid;
        const float w = (act && sub0 + po < end) ? stile[po] : 0.f;
        o0 = fmaf(w, b2f((u16)(vv[u] & 0xffffu)), o0);
        o1 = fmaf(w, b2f((u16)(vv[u] >> 16)), o1);
      }
    }
    __syncthreads();  // stile reused next sub-tile
  }
  // combine the 4 position-residue partials per dim
  if (act) { so[wid][e0] = o0; so[wid][e0 + 1] = o1; }
  __syncthreads();
  if (t == 0) {
    WS_STORE(&wsrow[hd], m);
    WS_STORE(&wsrow[hd + 1], l);
  }
  for (int d = t; d < hd; d += blockDim.x)
    WS_STORE(&wsrow[d], so[0][d] + so[1][d] + so[2][d] + so[3][d]);

  // ---- publish partial + elect the combining block ----------------------
  // sc1 write-through publish (Guideline 16 R1 variant): the ws stores above
  // are agent-scope relaxed 4-B atomics (= sc1 stores, the natural width
  // here), so no release fence is needed — just drain, then count arrivals.
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every wave drains
  __syncthreads();
  if (t == 0) {
    // epoch-free election: counters monotonically accumulate, the block
    // drawing (v % nchunk) == nchunk-1 combines — no per-launch reset
    u32 v = __hip_atomic_fetch_add(&cnt[h], 1u, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
    sm[0] = (v % (u32)nchunk == (u32)(nchunk - 1)) ? 1.f : 0.f;
  }
  __syncthreads();
  if (sm[0] == 0.f) return;
  // reducer reads the slabs with sc1 loads — no acquire fence, no L1 risk

  // ---- combine this head's partials (runs in exactly one block) ----------
  float* base = ws + (size_t)h * nchunk * (hd + 4);
  // stage m,l in LDS (parallel sc1 loads; serial dependent uncached loads
  // were the reducer's cost), then combine with per-chunk weights from LDS
  if (t < nchunk) {
    sm[0] = 0.f;  // keep sm[0] clear; use so rows as staging
    so[0][t] = WS_LOAD(&base[t * (hd + 4) + hd]);
    so[1][t] = WS_LOAD(&base[t * (hd + 4) + hd + 1]);
  }
  __syncthreads();
  float M = -INFINITY;
  for (int c = 0; c < nchunk; ++c) M = fmaxf(M, so[0][c]);
  float L = 0.f;
  for (int c = 0; c < nchunk; ++c)
    if (so[0][c] != -INFINITY) L += so[1][c] * __expf(so[0][c] - M);
  // per-chunk weights once into LDS; an empty chunk has m = -INF and a
  // ZERO partial (its o-sums were stored as 0.0), so its weight
  // __expf(-INF - M) = 0 makes the unguarded load contribute exactly 0 —
  // no per-chunk guard, so the nchunk sc1 loads below issue in parallel
  // instead of one execz-guarded vmcnt(0) round trip each.
  if (t < nchunk) so[2][t] = __expf(so[0][t] - M);
  __syncthreads();
  for (int d = t; d < hd; d += blockDim.x) {
    float o = 0.f;
#pragma unroll 4
    for (int c = 0; c < nchunk; ++c)
      o += WS_LOAD(&base[c * (hd + 4) + d]) * so[2][c];
    outbuf[(size_t)h * hd + d] = f2b(o / L);
  }
#undef WS_STORE
#undef WS_LOAD
}

// ---------------------------------------------------------------------------
// Prefill attention — flash-style f32 online softmax, causal, GQA, over the
// cache (which already holds positions [0, pos0+S)).  One wave per query
// row; 4 rows per block.  (attention.rs:300-343 + cache.rs:150-160 mask.)
// q rows come from the post-rope qkv buffer.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_attn_prefill(
    const u16* __restrict__ qkv, const u16* __restrict__ kc,
    const u16* __restrict__ vc, u16* __restrict__ out, int S, int pos0,
    int nh, int nkv, int hd, int max_seq, int qkv_stride, int out_stride,
    int window) {
  const int h = blockIdx.y;
  const int t = threadIdx.x, wid = t / WAVE, lane = t % WAVE;
  const int sidx = blockIdx.x * 4 + wid;
  if (sidx >= S) return;
  const int kvh = h / (nh / nkv);
  const int e0 = 2 * lane;
  const bool act = e0 + 1 < hd;
  const int n = pos0 + sidx + 1;      // causal: attend to <= own position
  float q0 = 0.f, q1 = 0.f;
  if (act) {
    const u16* qr = qkv + (size_t)sidx * qkv_stride + (size_t)h * hd + e0;
    q0 = b2f(qr[0]);
    q1 = b2f(qr[1]);
  }
  const float scale = rsqrtf((float)hd);
  float m = -INFINITY, l = 0.f, o0 = 0.f, o1 = 0.f;
  const u16* kbase = kc + (size_t)kvh * max_seq * hd;
  const u16* vbase = vc + (size_t)kvh * max_seq * hd;
  const int p0 = (window > 0 && n > window) ? n - window : 0;
  for (int p = p0; p < n; ++p) {
    float dot = 0.f;
    if (act) {
      const u16* kr = kbase + (size_t)p * hd + e0;
      dot = q0 * b2f(kr[0]) + q1 * b2f(kr[1]);
    }
    dot = wave_sum(dot) * scale;
    dot = __shfl(dot, 0, WAVE);
    float mn = fmaxf(m, dot);
    float alpha = __expf(m - mn);
    float pw = __expf(dot - mn);
    float v0 = 0.f, v1 = 0.f;
    if (act) {
      const u16* vr = vbase + (size_t)p * hd + e0;
      v0 = b2f(vr[0]);
      v1 = b2f(vr[1]);
    }
    o0 = o0 * alpha + pw * v0;
    o1 = o1 * alpha + pw * v1;
    l = l * alpha + pw;
    m = mn;
  }
  if (act) {
    u16* orow = out + (size_t)sidx * out_stride + (size_t)h * hd + e0;
    orow[0] = f2b(o0 / l);
    orow[1] = f2b(o1 / l);
  }
}

// ---------------------------------------------------------------------------
// MFMA flash-attention prefill (hd == 128) — causal, GQA, f32 online
// softmax, bf16 I/O.  Structure after the guide's 8-wave 32x32 ladder
// (cdna_hip_programming.md §B "Fused attention prefill"), basic variant:
//   - 8 waves per workgroup, each wave owns 32 query rows of one head
//   - swapped QK^T: P = mfma(K_tile, Q_tile) so the softmax column is
//     lane-local (col j = q = lane&31); 32x32x16 bf16 MFMA, 8 per tile
//   - P -> bf16 pack + __shfl_xor(32) half-exchange assembles the PV
//     A-fragments in-register (the T12 idea without inline asm)
//   - PV reads V from a TRANSPOSED cache (vt[kvh][d][pos]) so the
//     B-fragment's 8-consecutive-k elements are one 16-B load
// Per 32-kv tile per wave: 16 MFMAs + ~16 16-B global loads; no LDS, no
// barriers (waves fully independent).
// ---------------------------------------------------------------------------

__global__ __launch_bounds__(512) void k_attn_prefill_mfma(
    const u16* __restrict__ qkv, const u16* __restrict__ kc,
    const u16* __restrict__ vtc, u16* __restrict__ out, int S, int pos0,
    int nh, int nkv, int max_seq, int qkv_stride, int out_stride,
    int window) {
  const int hd = 128;
  const int w = threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  const int lhalf = lane >> 5, lq = lane & 31;
  const int h = blockIdx.y;
  const int kvh = h / (nh / nkv);
  const int qb = blockIdx.x * 256 + w * 32;
  if (qb >= S) return;

  // Q fragments (persistent): B[k][j=q], lane holds q = lq, dims
  // kk*16 + lhalf*8 .. +8
  bf16x8 qf[8];
  {
    const int row = min(qb + lq, S - 1);
    const u16* qrow = qkv + (size_t)row * qkv_stride + (size_t)h * hd;
#pragma unroll
    for (int kk = 0; kk < 8; ++kk)
      qf[kk] = *reinterpret_cast<const bf16x8*>(qrow + kk * 16 + lhalf * 8);
  }

  f32x16 oacc[4];
#pragma unroll
  for (int db = 0; db < 4; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[db][r] = 0.f;
  float m = -INFINITY, l = 0.f;
  const float scale = rsqrtf((float)hd);
  const int q_abs = pos0 + qb + lq;
  const bool q_valid = qb + lq < S;
  const int n_wave = pos0 + min(qb + 32, S);  // kv needed by this wave
  const int ntiles = (n_wave + 31) / 32;
  // sliding window: the wave's SMALLEST query attends from
  // (pos0 + qb) - window + 1; whole tiles below that are skipped
  const int tile0 =
      (window > 0) ? max(0, pos0 + qb - (window - 1)) / 32 : 0;
  const u16* kbase = kc + (size_t)kvh * max_seq * hd;
  const u16* vtbase = vtc + (size_t)kvh * hd * max_seq;

  // K fragments for the CURRENT tile live in kf and are reloaded IN PLACE
  // for tile+1 right after the QK^T MFMAs consume them — the reload and
  // the current tile's V^T loads (issued before the softmax, in consumer
  // order) ride the memory system under the softmax VALU chain, the same
  // wait-at-first-consumer structure as the decode kernel.
  bf16x8 kf[8];
  auto load_k = [&](int pkv) {
    const u16* krow = kbase + (size_t)(pkv + lq) * hd;
#pragma unroll
    for (int kk = 0; kk < 8; ++kk)
      kf[kk] = *reinterpret_cast<const bf16x8*>(krow + kk * 16 + lhalf * 8);
  };
  load_k(tile0 * 32);
  for (int tile = tile0; tile < ntiles; ++tile) {
    const int pkv = tile * 32;
    f32x16 p;
#pragma unroll
    for (int r = 0; r < 16; ++r) p[r] = 0.f;
#pragma unroll
    for (int kk = 0; kk < 8; ++kk)
      p = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[kk], qf[kk], p, 0, 0, 0);
    // current tile's V^T fragments (addresses only — no score dependency)
    bf16x8 vf[2][4];
#pragma unroll
    for (int kk = 0; kk < 2; ++kk)
#pragma unroll
      for (int db = 0; db < 4; ++db)
        vf[kk][db] = *reinterpret_cast<const bf16x8*>(
            vtbase + (size_t)(db * 32 + lq) * max_seq + pkv + 16 * kk +
            lhalf * 8);
    // next tile's K, overwriting kf (the MFMAs above already read it)
    if (tile + 1 < ntiles) load_k(pkv + 32);
    // scale + causal mask (reg r -> kv row (r&3)+8*(r>>2)+4*lhalf)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int kv_abs = pkv + (r & 3) + 8 * (r >> 2) + 4 * lhalf;
      const bool vis = q_valid && kv_abs <= q_abs &&
                       (window == 0 || kv_abs > q_abs - window);
      p[r] = vis ? p[r] * scale : -INFINITY;
    }
    // online softmax stats for column q = lq (halves combined via xor-32)
    float tm = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) tm = fmaxf(tm, p[r]);
    tm = fmaxf(tm, __shfl_xor(tm, 32, WAVE));
    const float mnew = fmaxf(m, tm);
    const float alpha = (mnew == -INFINITY) ? 0.f : __expf(m - mnew);
    float ep[16];
    float tsum = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      ep[r] = (p[r] == -INFINITY) ? 0.f : __expf(p[r] - mnew);
      tsum += ep[r];
    }
    tsum += __shfl_xor(tsum, 32, WAVE);
    l = l * alpha + tsum;
    m = mnew;
    // pack expP to bf16 pairs and exchange halves: after this each lane can
    // assemble A[i=q=lq][k=kv] fragments for PV
    u32 pk[8], rcv[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      pk[i] = (u32)f2b(ep[2 * i]) | ((u32)f2b(ep[2 * i + 1]) << 16);
      rcv[i] = __shfl_xor(pk[i], 32, WAVE);
    }
    // per-row alpha for the O rescale (row q via lane shuffle)
    float arow[16];
#pragma unroll
    for (int r = 0; r < 16; ++r)
      arow[r] = __shfl(alpha, (r & 3) + 8 * (r >> 2) + 4 * lhalf, WAVE);
#pragma unroll
    for (int db = 0; db < 4; ++db)
#pragma unroll
      for (int r = 0; r < 16; ++r) oacc[db][r] *= arow[r];
    // PV: two K=16 windows over the 32-kv tile
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      union { u32 u[4]; bf16x8 v; } af;
      if (lhalf == 0) {
        af.u[0] = pk[4 * kk];
        af.u[1] = pk[4 * kk + 1];
        af.u[2] = rcv[4 * kk];
        af.u[3] = rcv[4 * kk + 1];
      } else {
        af.u[0] = rcv[4 * kk + 2];
        af.u[1] = rcv[4 * kk + 3];
        af.u[2] = pk[4 * kk + 2];
        af.u[3] = pk[4 * kk + 3];
      }
#pragma unroll
      for (int db = 0; db < 4; ++db)
        oacc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            af.v, vf[kk][db], oacc[db], 0, 0, 0);
    }
  }

  // epilogue: divide by l (per q row, via shuffle) and store
  float lrow[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float lv = __shfl(l, (r & 3) + 8 * (r >> 2) + 4 * lhalf, WAVE);
    lrow[r] = 1.f / lv;
  }
#pragma unroll
  for (int db = 0; db < 4; ++db) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int qrow = (r & 3) + 8 * (r >> 2) + 4 * lhalf;
      const int srow = qb + qrow;
      if (srow < S)
        out[(size_t)srow * out_stride + (size_t)h * hd + db * 32 + lq] =
            f2b(oacc[db][r] * lrow[r]);
    }
  }
}

// ---------------------------------------------------------------------------
// GQA-grouped decode attention (hd == 128) — round-2 redesign of
// k_attn_decode_fused for long context.
//
// Why: the per-q-head kernel above reads each K/V row once per Q HEAD —
// at GQA ratio 4 that is 4x the algorithmic bytes through the cache
// hierarchy, and its phase-C V reads are two dependent full-latency round
// trips per 128-position tile (r01 profiles: ~0.9-1.2 TB/s algorithmic KV
// read at 8k context vs ~6 TB/s sibling GEMVs, waves memory-parked).
//
// This kernel assigns ONE block to all GB q-heads of a kv head, stages the
// K and V tiles through LDS exactly once with global_load_lds (1 KiB
// DMA pieces, 2-deep double buffer), and keeps every wait a COUNTED
// s_waitcnt vmcnt(12) with raw s_barriers (guide §5 T3/T4: loads for tile
// t+2 are issued as soon as tile t's buffer is consumed, so the pipeline
// never drains).  Algorithmic bytes = logical bytes = one read per KV row.
//
//   grid (nchunk, nkv * subg), block 256 (4 waves); GB = q-heads per block,
//   R = 4/GB waves per head (position residues).
//   phase A: each wave computes ITS head's scores for the whole 64-position
//            tile, lane = position: 16 b128 reads walk the lane's K row
//            (XOR-unit swizzled image, conflict-free) while q comes from
//            LDS at a wave-uniform address (broadcast, 1 LDS cycle) — the
//            score ends up IN the lane that owns the position, so the
//            online softmax needs no cross-lane traffic beyond the tile
//            max/sum reduce.  (A first cut reduced 16-lane partial dots
//            with __shfl_xor and broadcast PV weights with dynamic __shfl:
//            both compile to ds_bpermute chains with lgkmcnt(0) between —
//            ~150 LDS-pipe ops per tile — and measured 3.7x SLOWER than
//            the per-head kernel.  Weights now go through one LDS row,
//            read back at wave-uniform addresses.)
//   phase B: per-head online softmax, wave-redundant across residues
//   phase C: PV accumulate (wave = head x residue, lane = dim pair),
//            weights read from the wave's own LDS row (broadcast)
//   combine: same split-KV partial {o,m,l} publish + arrival-counter
//            election as k_attn_decode_fused (Guideline 16 R1 variant),
//            one elected block combines all GB heads.
//
// Replaces attention.rs:300-343 decode semantics incl. the sliding-window
// span bound (cache.rs:173-205); parity: tests/test_gpu_parity.py + fuzzer.
// ---------------------------------------------------------------------------
// probe (CAKE_ATTN_PROBE, perf diagnosis only — results wrong when != 0):
// 1 = skip the elected combine, 2 = also skip the publish/election.
template <int GB>
__global__ __launch_bounds__(256) void k_attn_decode_g(
    const u16* __restrict__ q, const u16* __restrict__ kc,
    const u16* __restrict__ vc, const int* __restrict__ pos,
    float* __restrict__ ws, u32* __restrict__ cnt, u16* __restrict__ outbuf,
    int nh, int nkv, int max_seq, int nchunk, int window, int subg,
    int probe) {
  constexpr int TILE = 64;
  constexpr int R = 4 / GB;
  const int hd = 128;
  // ONE shared object (a second __shared__ makes hipcc drain vmcnt(0)
  // before every ds_read of a glds pipeline — guide §5 trap 4a)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  u16* kb = reinterpret_cast<u16*>(smem);                  // [2][TILE][128]
  u16* vb = reinterpret_cast<u16*>(smem + 2 * TILE * 256); // [2][TILE][128]
  float* sc = reinterpret_cast<float*>(smem + 4 * TILE * 256);  // [GB][TILE]
  float* qlds = sc + GB * TILE;                            // [GB][128] f32
  float* so = qlds + GB * 128;                             // [4][136] scratch

  const int yb = blockIdx.y;
  const int kvh = yb / subg, sub = yb % subg;
  const int h0 = kvh * (nh / nkv) + sub * GB;
  const int chunk = blockIdx.x;
  const int n = *pos + 1;
  const int lo = (window > 0 && n > window) ? n - window : 0;
  const int cs = (n - lo + nchunk - 1) / nchunk;
  const int start = lo + chunk * cs;
  const int end = min(start + cs, n);
  const int t = threadIdx.x, wid = t / WAVE, lane = t % WAVE;
  const float scale = rsqrtf(128.f);
  const u16* kbase = kc + (size_t)kvh * max_seq * hd;
  const u16* vbase = vc + (size_t)kvh * max_seq * hd;
#define WS_STORE(p, v)                                                     \
  __hip_atomic_store((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
#define WS_LOAD(p)                                                         \
  __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

  // Tile staging is REGISTER-staged (guide T14: issue the global loads
  // early, ds_write after the next barrier) — a first cut used
  // global_load_lds, whose per-CU landing cadence (~10 GB/s/CU measured
  // here; the guide's attention row warns glds variants of register-staged
  // attention all measure <= 0) capped the whole kernel.  Each wave stages
  // 4 KiB of K and 4 KiB of V per tile: 4 x 16 B per lane, plain b128
  // loads counted with vmcnt(4).
  //   The K image is XOR-unit swizzled (rule 21): slot s of row r holds
  // source unit s ^ (r & 15), so phase A's per-lane row walk (lane = row)
  // is bank-conflict-free; the permutation stays inside the 256-B row, so
  // source coalescing is unchanged.  V stays linear (row-uniform reads).
  //   Overshoot rows (tile tails + the never-consumed pipeline tail
  // stages) collapse onto row end-1: masked by -INF scores anyway, and
  // the repeat read is L2-resident instead of fresh HBM traffic (PMC
  // showed 2.08x algorithmic fetch with max_seq-clamped tail stages).
  short8 rk[4], rv[4];
  auto stage_load = [&](short8 (&regs)[4], const u16* base, int tb,
                        bool swz) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int r = (wid * 4 + j) * 4 + (int)(lane >> 4);
      const int row = min(tb + r, end - 1);
      const int unit = swz ? ((lane & 15) ^ (r & 15)) : (lane & 15);
      regs[j] = *reinterpret_cast<const short8*>(base + (size_t)row * 128 +
                                                 unit * 8);
    }
  };
  auto stage_write = [&](short8 (&regs)[4], u16* dstb) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      *reinterpret_cast<short8*>(dstb + (size_t)(wid * 4 + j) * 4 * 128 +
                                 lane * 8) = regs[j];
  };

  // q rows of the block's GB heads -> LDS as f32 (read back at wave-uniform
  // addresses = broadcast, 1 LDS cycle per b128)
  for (int i = t; i < GB * 128; i += 256)
    qlds[i] = b2f(q[(size_t)(h0 + i / 128) * hd + (i & 127)]);
  __syncthreads();

  const int hs = wid / R;   // the head this wave serves
  const int rres = wid % R; // its position residue (phase C)
  float m = -INFINITY, lsum = 0.f, o0 = 0.f, o1 = 0.f;
  const int nt = start < end ? (end - start + TILE - 1) / TILE : 0;
  if (nt > 0) {
    // prologue: K0/V0 into LDS (ONE wait — both groups fly together),
    // K1/V1 left in flight in registers
    stage_load(rk, kbase, start, true);
    stage_load(rv, vbase, start, false);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    stage_write(rk, kb);
    stage_write(rv, vb);
    stage_load(rk, kbase, start + TILE, true);
    stage_load(rv, vbase, start + TILE, false);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    for (int ti = 0; ti < nt; ++ti) {
      const int tb = start + ti * TILE;
      const int cur = ti & 1;
      u16* kcur = kb + (size_t)cur * TILE * 128;
      u16* vcur = vb + (size_t)cur * TILE * 128;
      // ---- A: this wave's head, lane = position, full 128-dot ----------
      float d = 0.f;
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        // K chunk: lane's row, swizzled unit u -> slot u ^ (lane & 15)
        short8 kv8 = *reinterpret_cast<const short8*>(
            kcur + (size_t)lane * 128 + ((u ^ (lane & 15)) * 8));
        f32x4 q0 = *reinterpret_cast<const f32x4*>(qlds + hs * 128 + u * 8);
        f32x4 q1 = *reinterpret_cast<const f32x4*>(
            qlds + hs * 128 + u * 8 + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          d = fmaf(b2f((u16)kv8[e]), q0[e], d);
          d = fmaf(b2f((u16)kv8[e + 4]), q1[e], d);
        }
      }
      // K(ti+1) regs landed -> write into the other K buffer, re-issue
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      stage_write(rk, kb + (size_t)(cur ^ 1) * TILE * 128);
      stage_load(rk, kbase, tb + 2 * TILE, true);
      // ---- B: per-head online softmax (lane = position) ----------------
      const float sv = (tb + lane < end) ? d * scale : -INFINITY;
      float tm = wave_max(sv);
      tm = __shfl(tm, 0, WAVE);
      const float mnew = fmaxf(m, tm);
      const float alpha = (mnew == -INFINITY) ? 0.f : __expf(m - mnew);
      const float ew = (sv == -INFINITY) ? 0.f : __expf(sv - mnew);
      float ts = wave_sum(ew);
      ts = __shfl(ts, 0, WAVE);
      lsum = lsum * alpha + ts;
      o0 *= alpha;
      o1 *= alpha;
      m = mnew;
      if (rres == 0) sc[hs * TILE + lane] = ew;  // C reads it broadcast
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();  // sc visible; kcur fully consumed
      // V(ti+1) regs landed -> write into the other V buffer, re-issue
      asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
      stage_write(rv, vb + (size_t)(cur ^ 1) * TILE * 128);
      stage_load(rv, vbase, tb + 2 * TILE, false);
      // ---- C: PV accumulate (wave = head x residue, lane = dim pair) ---
#pragma unroll
      for (int p8 = rres * 8; p8 < TILE; p8 += R * 8) {
        // 8 positions per step: weights via two broadcast b128 reads,
        // V rows per-lane b32 — independent, so the lgkm waits batch
        f32x4 w0 = *reinterpret_cast<const f32x4*>(sc + hs * TILE + p8);
        f32x4 w1 = *reinterpret_cast<const f32x4*>(sc + hs * TILE + p8 + 4);
        u32 vv[8];
#pragma unroll
        for (int e = 0; e < 8; ++e)
          vv[e] = *reinterpret_cast<const u32*>(
              vcur + (size_t)(p8 + e) * 128 + 2 * lane);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float wt = e < 4 ? w0[e] : w1[e - 4];
          o0 = fmaf(wt, b2f((u16)(vv[e] & 0xffffu)), o0);
          o1 = fmaf(wt, b2f((u16)(vv[e] >> 16)), o1);
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();  // buffer writes visible for the next A
    }
  }

  // ---- cross-residue combine + split-KV partial publish ------------------
  // (drain everything once — the tail stages are never consumed)
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (R > 1) {
    so[wid * 136 + 2 * lane] = o0;
    so[wid * 136 + 2 * lane + 1] = o1;
    __syncthreads();
    if (rres == 0) {
#pragma unroll
      for (int r = 1; r < R; ++r) {
        o0 += so[(wid + r) * 136 + 2 * lane];
        o1 += so[(wid + r) * 136 + 2 * lane + 1];
      }
    }
    __syncthreads();  // so reused below
  }
  if (probe >= 2) {  // perf probe: main loop only
    if (t == 0 && o0 == 1e30f) outbuf[0] = f2b(o1);  // keep results live
    return;
  }
  if (nchunk == 1) {
    // single-chunk fast path (short contexts): this block holds the head's
    // COMPLETE (o, m, l) — write the output directly and skip the whole
    // split-KV publish / election / combine (at ctx 128 that tail was
    // ~8 of the 11 us launch: acquire fence + ws round trip + staging)
    if (rres == 0) {
      const float inv = 1.f / lsum;
      outbuf[(size_t)(h0 + hs) * hd + 2 * lane] = f2b(o0 * inv);
      outbuf[(size_t)(h0 + hs) * hd + 2 * lane + 1] = f2b(o1 * inv);
    }
    return;
  }
  float* wsrow = ws + ((size_t)(h0 + hs) * nchunk + chunk) * (hd + 4);
  if (rres == 0) {
    WS_STORE(&wsrow[2 * lane], o0);
    WS_STORE(&wsrow[2 * lane + 1], o1);
    if (lane == 0) {
      WS_STORE(&wsrow[hd], m);
      WS_STORE(&wsrow[hd + 1], lsum);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every wave drains (R1)
  __syncthreads();
  // election: the LAST `take` arrivers each combine GB/take heads —
  // per-HEAD parallel combines instead of one block serially walking all
  // GB heads (probe evidence: the combine, not the K/V loop, was the
  // wall).  An elected block that is NOT the final arriver must WAIT for
  // the launch's remaining arrivals before it may read the partials
  // (without the poll, a slot-0 block at nchunk == take combined while
  // later chunks had not yet published — an intermittent wrong-token
  // race caught by the 8B graph-vs-eager determinism test).  The poll is
  // relaxed with s_sleep, bounded, and short: the stragglers are already
  // in their own publish sequence.
  const int take = min(GB, nchunk);
  if (t == 0) {
    const u32 v = __hip_atomic_fetch_add(&cnt[yb], 1u, __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_AGENT);
    const int slot0 = (int)(v % (u32)nchunk) - (nchunk - take);
    if (slot0 >= 0 && probe < 1) {
      const u32 target = v - (v % (u32)nchunk) + (u32)nchunk;
      for (int spin = 0; spin < (1 << 22); ++spin) {
        const u32 cur = __hip_atomic_load(&cnt[yb], __ATOMIC_RELAXED,
                                          __HIP_MEMORY_SCOPE_AGENT);
        if ((int)(cur - target) >= 0) break;  // wrap-safe distance
        __builtin_amdgcn_s_sleep(2);
      }
    }
    sc[0] = (float)slot0;
  }
  __syncthreads();
  const int slot = (int)sc[0];
  if (slot < 0 || probe >= 1) return;

  // ---- elected block combines its share of the GB heads ------------------
  const int hpb = GB / take;
  if (nchunk <= 32) {
    // small/mid-nchunk combine: read the partials directly with raw sc1
    // BUFFER loads at full ILP — non-atomic, so hipcc batches them
    // (relaxed-atomic loads emit one wait each — the fp8 norm-chain
    // lesson), valid without an acquire because the producers stored sc1,
    // clamped with weights 0 beyond nchunk.  No fence, no LDS staging
    // round (their fixed ~3-4 us dominated short/mid-context launches).
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(
        (void*)ws, (short)0, nh * 64 * (hd + 4) * 4, 0x00020000);
    auto wsld = [&](u32 fidx) {
      union { int i; float f; } u;
      u.i = __builtin_amdgcn_raw_buffer_load_b32(rsrc, fidx * 4, 0,
                                                 16 /*sc1*/);
      return u.f;
    };
    for (int h = h0 + slot * hpb; h < h0 + slot * hpb + hpb; ++h) {
      const u32 fbase = (u32)h * (u32)nchunk * (u32)(hd + 4);
      const float mc =
          lane < nchunk ? wsld(fbase + (u32)lane * (hd + 4) + hd)
                        : -INFINITY;
      const float lc =
          lane < nchunk ? wsld(fbase + (u32)lane * (hd + 4) + hd + 1) : 0.f;
      float M = wave_max(mc);
      M = __shfl(M, 0, WAVE);
      const float wc = (mc == -INFINITY) ? 0.f : __expf(mc - M);
      float L = wave_sum(lc * wc);
      L = __shfl(L, 0, WAVE);
      if (wid == 0 && lane < 32) so[lane] = lane < nchunk ? wc : 0.f;
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __syncthreads();
      if (t < hd) {
        float o = 0.f;
        if (nchunk <= 8) {
#pragma unroll
          for (int c = 0; c < 8; ++c) {
            const u32 cc = (u32)min(c, nchunk - 1);
            o = fmaf(wsld(fbase + cc * (hd + 4) + t), so[c], o);
          }
        } else {
#pragma unroll
          for (int c = 0; c < 32; ++c) {
            const u32 cc = (u32)min(c, nchunk - 1);
            o = fmaf(wsld(fbase + cc * (hd + 4) + t), so[c], o);
          }
        }
        outbuf[(size_t)h * hd + t] = f2b(o / L);
      }
      __syncthreads();  // so reused for the next head
    }
    return;
  }
  // Large nchunk: the first cut read partials with per-dim 4-B relaxed
  // (sc1) loads — nchunk x GB dependent uncached round trips dominated the
  // whole kernel wall.  Now: one agent acquire, bulk-stage the head's
  // partial block into LDS with wide PLAIN loads (Guideline 16:
  // sc1-publish + acquire -> plain loads; all loads issued before the LDS
  // writes), then lane-parallel reductions (chunk = lane for m/l; serial
  // per-thread for-c loops over strided LDS were ~10us per head).
  if (t == 0) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  __syncthreads();
  float* stagebuf = reinterpret_cast<float*>(smem);  // kb+vb area, 64 KiB
  for (int h = h0 + slot * hpb; h < h0 + slot * hpb + hpb; ++h) {
    const float* base = ws + (size_t)h * nchunk * (hd + 4);
    const int nf = nchunk * (hd + 4);  // <= 64*132*4 B = 33 KiB
    f32x4 tmp[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const int i = min(t * 4 + k * 1024, nf - 4);
      tmp[k] = *reinterpret_cast<const f32x4*>(base + i);
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const int i = t * 4 + k * 1024;
      if (i < nf) *reinterpret_cast<f32x4*>(stagebuf + i) = tmp[k];
    }
    __syncthreads();
    // chunk = lane: one LDS read per lane, wave-reduced (every wave
    // computes the same M/L redundantly; wave 0 publishes the weights)
    const float mc = lane < nchunk
                         ? stagebuf[(size_t)lane * (hd + 4) + hd]
                         : -INFINITY;
    const float lc = lane < nchunk
                         ? stagebuf[(size_t)lane * (hd + 4) + hd + 1]
                         : 0.f;
    float M = wave_max(mc);
    M = __shfl(M, 0, WAVE);
    const float wc = (mc == -INFINITY) ? 0.f : __expf(mc - M);
    float L = wave_sum(lc * wc);
    L = __shfl(L, 0, WAVE);
    if (wid == 0 && lane < nchunk) so[lane] = wc;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __syncthreads();
    // weighted sum: thread = (dim, chunk-half); halves pair-summed in the
    // tail of the 64 KiB stage region (beyond nf <= 8448 floats)
    float* psum = stagebuf + 16384 - 256;
    const int d = t & 127, half = t >> 7;
    const int nc2 = (nchunk + 1) >> 1;
    const int jend = min(half * nc2 + nc2, nchunk);
    float oa = 0.f, ob = 0.f;
    for (int j = half * nc2; j < jend; j += 2) {
      oa = fmaf(stagebuf[(size_t)j * (hd + 4) + d], so[j], oa);
      if (j + 1 < jend)
        ob = fmaf(stagebuf[(size_t)(j + 1) * (hd + 4) + d], so[j + 1], ob);
    }
    psum[half * 128 + d] = oa + ob;
    __syncthreads();
    if (t < hd)
      outbuf[(size_t)h * hd + t] = f2b((psum[t] + psum[128 + t]) / L);
    __syncthreads();  // stagebuf + so reused for the next head
  }
#undef WS_STORE
#undef WS_LOAD
}

// ---------------------------------------------------------------------------
// Short-context grouped decode attention (hd == 128, G % 4 == 0, nchunk 4|8):
// ALL chunks of a q head live in ONE workgroup, so the split-KV combine goes
// through LDS — no ws, no arrival counter, no atomic, no poll, no fence.
//
// Why: with one 64-position tile per chunk (context < 512) k_attn_decode_g
// is ~1 us of arithmetic behind five or six dependent global round trips
// (q -> barrier -> K/V -> publish sc1 -> returning atomic -> poll -> two
// rounds of uncached partial loads).  Here the only global round trips are
// pos, then {q, K, V} together, then the store.
//
//   grid nh * NCH / 16, block 1024 = 16 waves; wave = (head hs, chunk c),
//   HPB = 16 / NCH heads per block (NCH 4: the four heads of a kv quad;
//   NCH 8: two of them).  The HPB waves that share chunk c stage its tile
//   together (64 / HPB rows each, b128 register-staged, issued at kernel
//   entry BEFORE anything waits on q), into ONE 16 KiB LDS image per chunk
//   that holds the K tile for phase A and is then overwritten with the V
//   tile (already in registers) for phase C — 8 x 16 KiB fits the 160 KiB
//   LDS where separate K and V images would not.
//
// Arithmetic per wave is k_attn_decode_g<4>'s, operation for operation
// (same chunk partition, same 128-term dot order, same wave_max / wave_sum /
// __expf online softmax per tile, same PV order, same combine chain with
// clamped chunks weighted 0), so the output is bit-identical to it at the
// same (n, nchunk, window); tests/test_attn_short_gpu.py asserts that.
// A chunk may hold several tiles (a graph captured at nchunk 4 runs to
// position ~319): the tile loop carries (m, l, o) exactly as the grouped
// kernel does, with the next tile's loads in flight under phase C.
// ---------------------------------------------------------------------------
template <int NCH>
__global__ __launch_bounds__(1024) void k_attn_decode_short(
    const u16* __restrict__ q, const u16* __restrict__ kc,
    const u16* __restrict__ vc, const int* __restrict__ pos,
    u16* __restrict__ outbuf, int nh, int nkv, int max_seq, int window) {
  constexpr int TILE = 64;
  constexpr int HPB = 16 / NCH;  // q heads per block = waves per chunk
  constexpr int NL = 16 / HPB;   // 16-B units per lane per tile image
  // NCH 8 stages 64 VGPRs per wave inside the 128-VGPR budget of a 16-wave
  // block: fully unrolled phases spilled (up to 30 VGPRs to scratch), these
  // factors are the largest that do not
  constexpr int UA = NCH == 8 ? 8 : 16, UC = NCH == 8 ? 4 : 8;
  const int hd = 128;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  u16* tiles = reinterpret_cast<u16*>(smem);               // [NCH][TILE][128]
  float* sc = reinterpret_cast<float*>(smem + NCH * TILE * 256);  // [16][TILE]
  float* qlds = sc + 16 * TILE;                            // [HPB][128] f32
  float* po = qlds + HPB * 128;                            // [16][128]
  float* pm = po + 16 * 128;                               // [16]
  float* pl = pm + 16;                                     // [16]

  const int G = nh / nkv;
  const int quad = blockIdx.x / (4 / HPB), part = blockIdx.x % (4 / HPB);
  const int kvh = quad / (G / 4), sub = quad % (G / 4);
  const int h0 = kvh * G + sub * 4 + part * HPB;
  const int t = threadIdx.x, wid = t / WAVE, lane = t % WAVE;
  const int hs = wid / NCH;   // the head this wave serves
  const int chunk = wid % NCH;
  const int n = *pos + 1;
  const int lo = (window > 0 && n > window) ? n - window : 0;
  const int cs = (n - lo + NCH - 1) / NCH;
  const int start = lo + chunk * cs;
  const int end = min(start + cs, n);
  const float scale = rsqrtf(128.f);
  const u16* kbase = kc + (size_t)kvh * max_seq * hd;
  const u16* vbase = vc + (size_t)kvh * max_seq * hd;
  u16* tcur = tiles + (size_t)chunk * TILE * 128;

  // same staging image as k_attn_decode_g: K XOR-unit swizzled, V linear,
  // overshoot rows collapsed onto row end-1 (>= 0 even for an empty chunk,
  // so every load below is in range and needs no predicate)
  short8 rk[NL], rv[NL];
  auto stage_load = [&](short8 (&regs)[NL], const u16* base, int tb,
                        bool swz) {
#pragma unroll
    for (int j = 0; j < NL; ++j) {
      const int r = (hs * NL + j) * 4 + (int)(lane >> 4);
      const int row = min(tb + r, end - 1);
      const int unit = swz ? ((lane & 15) ^ (r & 15)) : (lane & 15);
      regs[j] = *reinterpret_cast<const short8*>(base + (size_t)row * 128 +
                                                 unit * 8);
    }
  };
  auto stage_write = [&](short8 (&regs)[NL]) {
#pragma unroll
    for (int j = 0; j < NL; ++j)
      *reinterpret_cast<short8*>(tcur + (size_t)(hs * NL + j) * 4 * 128 +
                                 lane * 8) = regs[j];
  };

  // ONE round trip for q, K and V of the first tile: nothing waits in between
  // (q is loaded by every thread at a clamped index: a load under a
  // divergent branch gets its own vmcnt(0) before the branch rejoins;
  // hipcc still issues it BEHIND the tile loads, so the waves that write q
  // to LDS wait for V as well — all of it is one round trip regardless)
  const u16 qv = q[(size_t)(h0 + min(t / 128, HPB - 1)) * hd + (t & 127)];
  stage_load(rk, kbase, start, true);
  stage_load(rv, vbase, start, false);
  if (t < HPB * 128) qlds[t] = b2f(qv);

  float m = -INFINITY, lsum = 0.f, o0 = 0.f, o1 = 0.f;
  const int nt = start < end ? (end - start + TILE - 1) / TILE : 0;
  const int ntmax = (cs + TILE - 1) / TILE;  // chunk 0's count: block-uniform
  for (int ti = 0; ti < ntmax; ++ti) {
    const int tb = start + ti * TILE;
    stage_write(rk);
    __syncthreads();  // K image (and q) visible
    if (ti < nt) {
      // ---- A: lane = position, full 128-dot ------------------------------
      float d = 0.f;
#pragma unroll UA
      for (int u = 0; u < 16; ++u) {
        short8 kv8 = *reinterpret_cast<const short8*>(
            tcur + (size_t)lane * 128 + ((u ^ (lane & 15)) * 8));
        f32x4 q0 = *reinterpret_cast<const f32x4*>(qlds + hs * 128 + u * 8);
        f32x4 q1 = *reinterpret_cast<const f32x4*>(
            qlds + hs * 128 + u * 8 + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          d = fmaf(b2f((u16)kv8[e]), q0[e], d);
          d = fmaf(b2f((u16)kv8[e + 4]), q1[e], d);
        }
      }
      // ---- B: online softmax ---------------------------------------------
      const float sv = (tb + lane < end) ? d * scale : -INFINITY;
      float tm = wave_max(sv);
      tm = __shfl(tm, 0, WAVE);
      const float mnew = fmaxf(m, tm);
      const float alpha = (mnew == -INFINITY) ? 0.f : __expf(m - mnew);
      const float ew = (sv == -INFINITY) ? 0.f : __expf(sv - mnew);
      float ts = wave_sum(ew);
      ts = __shfl(ts, 0, WAVE);
      lsum = lsum * alpha + ts;
      o0 *= alpha;
      o1 *= alpha;
      m = mnew;
      sc[wid * TILE + lane] = ew;  // the wave's own row; C reads it broadcast
    }
    __syncthreads();  // every wave is done with the K image
    stage_write(rv);
    if (ti + 1 < ntmax) {  // next tile's loads fly under phase C
      stage_load(rk, kbase, tb + TILE, true);
      stage_load(rv, vbase, tb + TILE, false);
    }
    __syncthreads();  // V image visible
    if (ti < nt) {
      // ---- C: PV accumulate, lane = dim pair -----------------------------
#pragma unroll UC
      for (int p8 = 0; p8 < TILE; p8 += 8) {
        f32x4 w0 = *reinterpret_cast<const f32x4*>(sc + wid * TILE + p8);
        f32x4 w1 = *reinterpret_cast<const f32x4*>(sc + wid * TILE + p8 + 4);
        u32 vv[8];
#pragma unroll
        for (int e = 0; e < 8; ++e)
          vv[e] = *reinterpret_cast<const u32*>(
              tcur + (size_t)(p8 + e) * 128 + 2 * lane);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float wt = e < 4 ? w0[e] : w1[e - 4];
          o0 = fmaf(wt, b2f((u16)(vv[e] & 0xffffu)), o0);
          o1 = fmaf(wt, b2f((u16)(vv[e] >> 16)), o1);
        }
      }
    }
    if (ti + 1 < ntmax) __syncthreads();  // V image consumed before next K
  }

  // ---- in-block split-KV combine through LDS -------------------------------
  po[wid * 128 + 2 * lane] = o0;
  po[wid * 128 + 2 * lane + 1] = o1;
  if (lane == 0) {
    pm[wid] = m;
    pl[wid] = lsum;
  }
  __syncthreads();
  if (chunk < 2) {  // two waves per head, 64 dims each
    const int hw = hs * NCH;
    const float mc = lane < NCH ? pm[hw + lane] : -INFINITY;
    const float lc = lane < NCH ? pl[hw + lane] : 0.f;
    float M = wave_max(mc);
    M = __shfl(M, 0, WAVE);
    const float wc = (mc == -INFINITY) ? 0.f : __expf(mc - M);
    float L = wave_sum(lc * wc);
    L = __shfl(L, 0, WAVE);
    const int d = chunk * 64 + lane;
    float o = 0.f;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const int cc = min(c, NCH - 1);
      const float w = c < NCH ? __shfl(wc, c, WAVE) : 0.f;
      o = fmaf(po[(hw + cc) * 128 + d], w, o);
    }
    outbuf[(size_t)(h0 + hs) * hd + d] = f2b(o / L);
  }
}

// grouped-kernel dispatch: grid_y (nkv * subg) when the GQA-grouped decode
// kernel applies to this head geometry, 0 = fall back to the per-head
// kernel.  The engine uses this for its split-KV chunk-count policy.
int attn_decode_grid_y(int nh, int nkv, int hd) {
  if (hd == 256 && nkv > 0 && nh > 0 && nh % nkv == 0)
    return nh / attn256_group(nh, nkv);
  if (hd != 128 || nkv <= 0 || nh % nkv != 0) return 0;
  if (getenv("CAKE_ATTN_V2") && atoi(getenv("CAKE_ATTN_V2")) == 0) return 0;
  const int G = nh / nkv;
  if (G >= 4 && G % 4 == 0) return nkv * (G / 4);
  if (G == 2 || G == 1) return nkv;
  return 0;
}

// which decode kernel launch_attn_decode runs: 0 = per-head
// (k_attn_decode_fused), 1 = grouped (k_attn_decode_g), 2 = short
// (k_attn_decode_short).  The short kernel is routed at nchunk 4 only: at
// nchunk 8 (two heads per block, 144 KiB of LDS, reduced unrolls) it
// measured no faster than the grouped kernel per launch and slower end to
// end (profiles/short_attn_NOTES.md), so there it runs only under
// CAKE_ATTN_SHORT=2.  CAKE_ATTN_SHORT=0 restores the grouped routing
// everywhere.  The knob is read per launch so a test can flip it.
int attn_decode_path(int nh, int nkv, int hd, int nchunk) {
  if (hd == 256) return 3;
  if (attn_decode_grid_y(nh, nkv, hd) <= 0) return 0;
  const char* e = getenv("CAKE_ATTN_SHORT");
  const int mode = e ? atoi(e) : 1;
  if (mode == 0 || (nh / nkv) % 4 != 0) return 1;
  if (nchunk == 4 || (nchunk == 8 && mode >= 2)) return 2;
  return 1;
}

// ---------------------------------------------------------------------------
// MFMA flash prefill v2 (hd == 128): same math/fragment structure as
// k_attn_prefill_mfma, but the K and V^T tiles are staged ONCE per block
// through LDS and shared by all 8 waves (the v1 kernel loaded them
// per-wave from global: 8x the logical traffic and 16 global loads per
// lane per tile).  Staging is register-staged (decode kernel's T14
// pattern): per tile each wave loads 16 B/lane of K and of V^T, writes
// them into the other LDS buffer behind counted vmcnt(1)/(0) waits, ONE
// raw barrier per tile.  K image [32][128] with unit ^= (row & 15); V^T
// image [128][32] (dim-major) with unit ^= (d & 3) ^ ((d >> 2) & 3) —
// both swizzles applied on the SOURCE address (rule 21), bank-conflict-
// free for the fragment reads.  Waves outside their causal/window tile
// range skip compute but keep staging/waits/barriers uniform.
// ---------------------------------------------------------------------------
// lane<->lane+32 half exchange via v_permlane32_swap + cndmask (2-3 VALU)
// instead of __shfl_xor(.,32) (ds_bpermute + lgkm wait on the LDS pipe)
__device__ inline u32 halfswap32(u32 x, int lhalf) {
  auto r = __builtin_amdgcn_permlane32_swap(x, x, false, false);
  return lhalf == 0 ? (u32)r[1] : (u32)r[0];
}
__device__ inline float halfswap32f(float x, int lhalf) {
  union { float f; u32 u; } a{x};
  a.u = halfswap32(a.u, lhalf);
  return a.f;
}

// NW = waves per block (8 => 256 q rows/block, 4 => 128).  At S=2048 the
// NW=8 grid is EXACTLY 256 blocks on 256 CUs with causally skewed work
// (first q block 8 KV tiles, last 64): one block per CU means the chip
// waits on the longest blocks while CUs that hosted early blocks sit
// empty (~36/64 = 56% utilization; the idle is invisible to per-wave SQ
// counters).  NW=4 doubles the block count so the scheduler backfills,
// and qb0 is REVERSED (longest q blocks dispatch first) so the tail is
// bounded by the average, not the max.
// the second launch_bounds arg (min 2 waves/SIMD) caps the register
// budget at 256: without it the NW=4 instantiation spilled 80 AGPRs
// (occupancy 1 wave/SIMD — one lone 4-wave block per CU, no backfill).
// NSPLIT=2 is flash-style split-KV for the CAUSAL SKEW: with one block
// per (q block, head) the wall is the LONGEST block's tile count (the
// last q rows of a pos0=0 chunk walk 8x the tiles of the first), and
// narrower blocks cannot shrink it (measured: NW=4 within 3% of NW=8).
// Each block instead halves ITS OWN tile range across blockIdx.z and
// writes unnormalized partials (o, m, l) to `ws` (row stride 132 f32);
// k_attn_pf_combine merges the two.  An empty half writes m=-inf, l=0,
// o=0, which the combine weighs to zero.
// DEEP=1: 3 LDS buffers with TWO load generations in flight (register
// sets alternate per generation) — covers HBM latency when the 1-tile
// budget of the 2-buffer schedule is short.  CAKE_PF_DEEP selects it.
template <int NW, int NSPLIT, int DEEP>
__global__ __launch_bounds__(NW * 64, 2) void k_attn_prefill_mfma2(
    const u16* __restrict__ qkv, const u16* __restrict__ kc,
    const u16* __restrict__ vtc, u16* __restrict__ out, float* __restrict__ ws,
    int S, int pos0, int nh, int nkv, int max_seq, int qkv_stride,
    int out_stride, int window) {
  const int hd = 128;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  u16* kb = reinterpret_cast<u16*>(smem);              // [2|3][32][128]
  u16* vb = reinterpret_cast<u16*>(smem + (DEEP ? 3 : 2) * 32 * 256);
  const int w = threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  const int lhalf = lane >> 5, lq = lane & 31;
  const int h = blockIdx.y;
  const int kvh = h / (nh / nkv);
  const int qb0 = (gridDim.x - 1 - blockIdx.x) * (NW * 32);
  const int qb = qb0 + w * 32;
  const bool wactive = qb < S;

  bf16x8 qf[8];
  {
    const int row = min(qb + lq, S - 1);
    const u16* qrow = qkv + (size_t)row * qkv_stride + (size_t)h * hd;
#pragma unroll
    for (int kk = 0; kk < 8; ++kk)
      qf[kk] = *reinterpret_cast<const bf16x8*>(qrow + kk * 16 + lhalf * 8);
  }
  f32x16 oacc[4];
#pragma unroll
  for (int db = 0; db < 4; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[db][r] = 0.f;
  float m = -INFINITY, l = 0.f;
  const float scale = rsqrtf(128.f);
  const int q_abs = pos0 + qb + lq;
  const bool q_valid = wactive && (qb + lq < S);
  const int n_wave = pos0 + min(qb + 32, S);
  const int n_blk = pos0 + min(qb0 + NW * 32, S);
  const int ntiles_w = wactive ? (n_wave + 31) / 32 : 0;
  const int ntiles_b = (n_blk + 31) / 32;
  const int tile0_w =
      (window > 0) ? max(0, pos0 + qb - (window - 1)) / 32 : 0;
  const int tile0_b =
      (window > 0) ? max(0, pos0 + qb0 - (window - 1)) / 32 : 0;
  const u16* kbase = kc + (size_t)kvh * max_seq * hd;
  const u16* vtbase = vtc + (size_t)kvh * hd * max_seq;

  // staging: the 32x128 K tile and 128x32 V^T tile are split evenly over
  // the NW waves, 16 B units per lane; NW=8 => one unit of each per lane,
  // NW=4 => two (PASSES per-lane 16-B units).  Tile bases stay inside
  // [0, max_seq) (max_seq is a multiple of 32; rows beyond the live
  // context are zeros and masked).
  constexpr int PASSES = 8 / NW;                 // 16-B units per lane
  constexpr int SETS = (DEEP == 1) ? 2 : 1;      // load generations in regs
  short8 rkp[SETS][PASSES], rvp[SETS][PASSES];
  const int krow_l = w * (4 * PASSES) + (lane >> (4 - (PASSES >> 1)));
  const int kslot0 = lane & (15 >> (PASSES >> 1));   // 0..15 (NW8), 0..7
  const int vdim_l = w * (16 * PASSES) + (lane >> (2 - (PASSES >> 1)));
  const int vslot0 = lane & (3 >> (PASSES >> 1));    // 0..3 (NW8), 0..1
  const int vswz_l = (vdim_l & 3) ^ ((vdim_l >> 2) & 3);
  auto load_k = [&](int st, int tb) {
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
      const int u = kslot0 + p * (16 / PASSES);
      rkp[st][p] = *reinterpret_cast<const short8*>(
          kbase + (size_t)(tb + krow_l) * 128 + (u ^ (krow_l & 15)) * 8);
    }
  };
  auto load_v = [&](int st, int tb) {
#pragma unroll
    for (int p = 0; p < PASSES; ++p) {
      const int u = vslot0 + p * (4 / PASSES);
      rvp[st][p] = *reinterpret_cast<const short8*>(
          vtbase + (size_t)vdim_l * max_seq + tb + (u ^ vswz_l) * 8);
    }
  };
  auto write_k = [&](int st, u16* dst) {
#pragma unroll
    for (int p = 0; p < PASSES; ++p)
      *reinterpret_cast<short8*>(
          dst + (size_t)krow_l * 128 + (kslot0 + p * (16 / PASSES)) * 8) =
          rkp[st][p];
  };
  auto write_v = [&](int st, u16* dst) {
#pragma unroll
    for (int p = 0; p < PASSES; ++p)
      *reinterpret_cast<short8*>(
          dst + (size_t)vdim_l * 32 + (vslot0 + p * (4 / PASSES)) * 8) =
          rvp[st][p];
  };

  // this block's tile range; NSPLIT=2 halves it across blockIdx.z
  int t_lo = tile0_b, t_hi = ntiles_b;
  if constexpr (NSPLIT == 2) {
    const int half = (t_hi - t_lo + 1) / 2;
    if (blockIdx.z == 0)
      t_hi = t_lo + half;
    else
      t_lo = t_lo + half;
  }

  if constexpr (DEEP == 2) {
    // Interleave schedule (CAKE_PF_DEEP=2): the NEXT tile's QK MFMAs are
    // issued before this tile's softmax, so the MFMA pipe drains under
    // the VALU exp/pack chain instead of convoying phase-by-phase.  LDS
    // is a 3-buffer ring (K(i) and K(i+1) resident at tile entry);
    // registers hold ONE staged generation (the 2-generation flight of
    // DEEP=1 measured 2.5-9x slower from spills).
    const int tbm = max_seq - 32;
    load_k(0, min(t_lo * 32, tbm));
    load_v(0, min(t_lo * 32, tbm));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    write_k(0, kb);
    write_v(0, vb);
    load_k(0, min((t_lo + 1) * 32, tbm));
    load_v(0, min((t_lo + 1) * 32, tbm));
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    write_k(0, kb + (size_t)1 * 32 * 128);
    write_v(0, vb + (size_t)1 * 128 * 32);
    load_k(0, min((t_lo + 2) * 32, tbm));
    load_v(0, min((t_lo + 2) * 32, tbm));
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();

    auto qk_tile = [&](const u16* kcur, f32x16& p) {
#pragma unroll
      for (int r = 0; r < 16; ++r) p[r] = 0.f;
#pragma unroll
      for (int kk = 0; kk < 8; ++kk) {
        const int u = kk * 2 + lhalf;
        bf16x8 kf = *reinterpret_cast<const bf16x8*>(
            kcur + (size_t)lq * 128 + (u ^ (lq & 15)) * 8);
        p = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[kk], p, 0, 0, 0);
      }
    };

    f32x16 pc, pn;
    if (wactive && t_lo >= tile0_w && t_lo < ntiles_w) qk_tile(kb, pc);
    for (int ti = t_lo; ti < t_hi; ++ti) {
      const int cur = (ti - t_lo) % 3;
      const int nxt = (ti + 1 - t_lo) % 3;
      const int wr2 = (ti + 2 - t_lo) % 3;
      const u16* vcur = vb + (size_t)cur * 128 * 32;
      const bool compute = wactive && ti >= tile0_w && ti < ntiles_w;
      const bool compute_n = wactive && ti + 1 >= tile0_w &&
                             ti + 1 < ntiles_w && ti + 1 < t_hi;
      const int pkv = ti * 32;
      if (compute_n) qk_tile(kb + (size_t)nxt * 32 * 128, pn);
      float mnew = m, alpha = 1.f, tsum = 0.f;
      float ep[16];
      if (compute) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int kv_abs = pkv + (r & 3) + 8 * (r >> 2) + 4 * lhalf;
          const bool vis = q_valid && kv_abs <= q_abs &&
                           (window == 0 || kv_abs > q_abs - window);
          pc[r] = vis ? pc[r] * scale : -INFINITY;
        }
        float tm = -INFINITY;
#pragma unroll
        for (int r = 0; r < 16; ++r) tm = fmaxf(tm, pc[r]);
        tm = fmaxf(tm, halfswap32f(tm, lhalf));
        mnew = fmaxf(m, tm);
        alpha = (mnew == -INFINITY) ? 0.f : __expf(m - mnew);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          ep[r] = (pc[r] == -INFINITY) ? 0.f : __expf(pc[r] - mnew);
          tsum += ep[r];
        }
        tsum += halfswap32f(tsum, lhalf);
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      write_k(0, kb + (size_t)wr2 * 32 * 128);
      write_v(0, vb + (size_t)wr2 * 128 * 32);
      {
        const int tb2 = min((ti + 3) * 32, tbm);
        load_k(0, tb2);
        load_v(0, tb2);
      }
      if (compute) {
        const bool norescale = __all(mnew == m);
        l = l * alpha + tsum;
        m = mnew;
        u32 pk[8], rcv[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          pk[i] = (u32)f2b(ep[2 * i]) | ((u32)f2b(ep[2 * i + 1]) << 16);
          rcv[i] = halfswap32(pk[i], lhalf);
        }
        if (!norescale) {
          float arow[16];
#pragma unroll
          for (int r = 0; r < 16; ++r)
            arow[r] =
                __shfl(alpha, (r & 3) + 8 * (r >> 2) + 4 * lhalf, WAVE);
#pragma unroll
          for (int db = 0; db < 4; ++db)
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[db][r] *= arow[r];
        }
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
          union { u32 u[4]; bf16x8 v; } af;
          if (lhalf == 0) {
            af.u[0] = pk[4 * kk];
            af.u[1] = pk[4 * kk + 1];
            af.u[2] = rcv[4 * kk];
            af.u[3] = rcv[4 * kk + 1];
          } else {
            af.u[0] = rcv[4 * kk + 2];
            af.u[1] = rcv[4 * kk + 3];
            af.u[2] = pk[4 * kk + 2];
            af.u[3] = pk[4 * kk + 3];
          }
#pragma unroll
          for (int db = 0; db < 4; ++db) {
            const int d0 = db * 32 + lq;
            const int u = kk * 2 + lhalf;
            bf16x8 vf = *reinterpret_cast<const bf16x8*>(
                vcur + (size_t)d0 * 32 +
                ((u ^ ((d0 & 3) ^ ((d0 >> 2) & 3))) * 8));
            oacc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
                af.v, vf, oacc[db], 0, 0, 0);
          }
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      pc = pn;
    }
  } else {
  const int tbmax = max_seq - 32;
  load_k(0, min(t_lo * 32, tbmax));
  load_v(0, min(t_lo * 32, tbmax));
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  write_k(0, kb);
  write_v(0, vb);
  load_k(DEEP ? 1 : 0, min((t_lo + 1) * 32, tbmax));
  load_v(DEEP ? 1 : 0, min((t_lo + 1) * 32, tbmax));
  if constexpr (DEEP) {  // second generation in flight
    load_k(0, min((t_lo + 2) * 32, tbmax));
    load_v(0, min((t_lo + 2) * 32, tbmax));
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();

  int cb = 0;  // current LDS buffer (mod 2|3 ring)
  for (int ti = t_lo; ti < t_hi; ++ti) {
    const int cur = cb;
    const int wrt = (cb + 1 == (DEEP ? 3 : 2)) ? 0 : cb + 1;
    cb = wrt;
    const int wset = DEEP ? ((ti + 1 - t_lo) & 1) : 0;
    const u16* kcur = kb + (size_t)cur * 32 * 128;
    const u16* vcur = vb + (size_t)cur * 128 * 32;
    const bool compute = wactive && ti >= tile0_w && ti < ntiles_w;
    const int pkv = ti * 32;
    f32x16 p;
    if (compute) {
#pragma unroll
      for (int r = 0; r < 16; ++r) p[r] = 0.f;
#pragma unroll
      for (int kk = 0; kk < 8; ++kk) {
        const int u = kk * 2 + lhalf;
        bf16x8 kf = *reinterpret_cast<const bf16x8*>(
            kcur + (size_t)lq * 128 + (u ^ (lq & 15)) * 8);
        p = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf, qf[kk], p, 0, 0, 0);
      }
    }
    // K(ti+1) regs landed -> ring buffer (younger ops still out)
    if constexpr (PASSES == 1)
      asm volatile("s_waitcnt vmcnt(%0)" ::"i"(DEEP ? 3 : 1) : "memory");
    else
      asm volatile("s_waitcnt vmcnt(%0)" ::"i"(DEEP ? 6 : 2) : "memory");
    write_k(wset, kb + (size_t)wrt * 32 * 128);
    float mnew = m, alpha = 1.f, tsum = 0.f;
    float ep[16];
    if (compute) {
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int kv_abs = pkv + (r & 3) + 8 * (r >> 2) + 4 * lhalf;
        const bool vis = q_valid && kv_abs <= q_abs &&
                         (window == 0 || kv_abs > q_abs - window);
        p[r] = vis ? p[r] * scale : -INFINITY;
      }
      float tm = -INFINITY;
#pragma unroll
      for (int r = 0; r < 16; ++r) tm = fmaxf(tm, p[r]);
      tm = fmaxf(tm, halfswap32f(tm, lhalf));
      mnew = fmaxf(m, tm);
      alpha = (mnew == -INFINITY) ? 0.f : __expf(m - mnew);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        ep[r] = (p[r] == -INFINITY) ? 0.f : __expf(p[r] - mnew);
        tsum += ep[r];
      }
      tsum += halfswap32f(tsum, lhalf);
    }
    // V(ti+1) regs landed -> ring buffer; re-issue the freed set
    if constexpr (DEEP)
      asm volatile("s_waitcnt vmcnt(%0)" ::"i"(PASSES == 1 ? 2 : 4)
                   : "memory");
    else
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    write_v(wset, vb + (size_t)wrt * 128 * 32);
    {
      const int tb2 = min((ti + (DEEP ? 3 : 2)) * 32, tbmax);
      load_k(wset, tb2);
      load_v(wset, tb2);
    }
    if (compute) {
      // exact defer-max (T13 with THR=0): when NO row's max grew this
      // tile, every alpha is exactly 1.0 and the O rescale (16 dynamic
      // shuffles -> ds_bpermute chains + 64 multiplies) is skipped
      // bit-identically.  Safe order: this tile's P enters O only after
      // the decision that covers it (the textbook order).
      const bool norescale = __all(mnew == m);
      l = l * alpha + tsum;
      m = mnew;
      u32 pk[8], rcv[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        pk[i] = (u32)f2b(ep[2 * i]) | ((u32)f2b(ep[2 * i + 1]) << 16);
        rcv[i] = halfswap32(pk[i], lhalf);
      }
      if (!norescale) {
        float arow[16];
#pragma unroll
        for (int r = 0; r < 16; ++r)
          arow[r] = __shfl(alpha, (r & 3) + 8 * (r >> 2) + 4 * lhalf, WAVE);
#pragma unroll
        for (int db = 0; db < 4; ++db)
#pragma unroll
          for (int r = 0; r < 16; ++r) oacc[db][r] *= arow[r];
      }
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        union { u32 u[4]; bf16x8 v; } af;
        if (lhalf == 0) {
          af.u[0] = pk[4 * kk];
          af.u[1] = pk[4 * kk + 1];
          af.u[2] = rcv[4 * kk];
          af.u[3] = rcv[4 * kk + 1];
        } else {
          af.u[0] = rcv[4 * kk + 2];
          af.u[1] = rcv[4 * kk + 3];
          af.u[2] = pk[4 * kk + 2];
          af.u[3] = pk[4 * kk + 3];
        }
#pragma unroll
        for (int db = 0; db < 4; ++db) {
          const int d0 = db * 32 + lq;
          const int u = kk * 2 + lhalf;
          bf16x8 vf = *reinterpret_cast<const bf16x8*>(
              vcur + (size_t)d0 * 32 +
              ((u ^ ((d0 & 3) ^ ((d0 >> 2) & 3))) * 8));
          oacc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af.v, vf,
                                                             oacc[db], 0,
                                                             0, 0);
        }
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // LDS writes visible; cur consumed
  }
  }  // DEEP != 2

  if (wactive) {
    if constexpr (NSPLIT == 2) {
      // unnormalized partial: o rows + per-row (m, l); both lane halves
      // hold identical m/l for their shared lq row — one writes
      if (lhalf == 0 && qb + lq < S) {
        float* wr = ws + ((size_t)(h * S + qb + lq) * 2 + blockIdx.z) * 132;
        wr[128] = m;
        wr[129] = l;
      }
#pragma unroll
      for (int db = 0; db < 4; ++db) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int qrow = (r & 3) + 8 * (r >> 2) + 4 * lhalf;
          const int srow = qb + qrow;
          if (srow < S)
            ws[((size_t)(h * S + srow) * 2 + blockIdx.z) * 132 + db * 32 +
               lq] = oacc[db][r];
        }
      }
    } else {
      float lrow[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        float lv = __shfl(l, (r & 3) + 8 * (r >> 2) + 4 * lhalf, WAVE);
        lrow[r] = 1.f / lv;
      }
#pragma unroll
      for (int db = 0; db < 4; ++db) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int qrow = (r & 3) + 8 * (r >> 2) + 4 * lhalf;
          const int srow = qb + qrow;
          if (srow < S)
            out[(size_t)srow * out_stride + (size_t)h * hd + db * 32 + lq] =
                f2b(oacc[db][r] * lrow[r]);
        }
      }
    }
  }
}

// merge the two split-KV partials of one (head, q row): standard flash
// combine — renormalize by exp(m_z - max) and the summed l
__global__ __launch_bounds__(256) void k_attn_pf_combine(
    const float* __restrict__ ws, u16* __restrict__ out, int S, int nh,
    int out_stride) {
  const int idx = blockIdx.x * 2 + threadIdx.x / 128;  // (h, row) slot
  const int d = threadIdx.x % 128;
  if (idx >= S * nh) return;
  const int h = idx / S, srow = idx % S;
  const float* w0 = ws + ((size_t)idx * 2 + 0) * 132;
  const float* w1 = ws + ((size_t)idx * 2 + 1) * 132;
  const float m0 = w0[128], l0 = w0[129];
  const float m1 = w1[128], l1 = w1[129];
  const float M = fmaxf(m0, m1);
  const float e0 = (m0 == -INFINITY) ? 0.f : __expf(m0 - M);
  const float e1 = (m1 == -INFINITY) ? 0.f : __expf(m1 - M);
  const float inv = 1.f / (l0 * e0 + l1 * e1);
  out[(size_t)srow * out_stride + (size_t)h * 128 + d] =
      f2b((w0[d] * e0 + w1[d] * e1) * inv);
}

void launch_rope_store_decode(u16* qkv, u16* kc, u16* vc, u16* vtc,
                              const float* cost, const float* sint,
                              const int* pos, int nh, int nkv, int hd, int rd,
                              int max_seq, const u16* qn, const u16* kn,
                              float eps, hipStream_t s, const float* bias) {
  hipLaunchKernelGGL(k_rope_store_decode, dim3(nh + 2 * nkv), dim3(64), 0, s,
                     qkv, kc, vc, vtc, cost, sint, pos, nh, nkv, hd, rd,
                     max_seq, qn, kn, eps, bias);
}
void launch_rope_store_prefill(u16* qkv, u16* kc, u16* vc, u16* vtc,
                               const float* cost, const float* sint, int pos0,
                               int S, int nh, int nkv, int hd, int rd,
                               int max_seq, int qkv_stride, const u16* qn,
                               const u16* kn, float eps, hipStream_t s,
                               const float* bias) {
  hipLaunchKernelGGL(k_rope_store_prefill, dim3(nh + 2 * nkv, S), dim3(64), 0,
                     s, qkv, kc, vc, vtc, cost, sint, pos0, nh, nkv, hd, rd,
                     max_seq, qkv_stride, qn, kn, eps, bias);
}
void launch_attn_decode(const u16* q, const u16* kc, const u16* vc,
                        const int* pos, float* ws, u32* cnt, u16* out, int nh,
                        int nkv, int hd, int max_seq, int nchunk, int window,
                        hipStream_t s) {
  if (hd == 256) {
    launch_attn_decode_256(q, kc, vc, pos, ws, cnt, out, nh, nkv, max_seq,
                           nchunk, window, s);
    return;
  }
  const int gy = attn_decode_grid_y(nh, nkv, hd);
  if (attn_decode_path(nh, nkv, hd, nchunk) == 2) {
    // tile image per chunk + scores[16][64] + q f32 [HPB][128] + partial
    // o [16][128] + m/l [16] each
    const size_t smem = (size_t)nchunk * 64 * 256 + 16 * 64 * 4 +
                        (size_t)(16 / nchunk) * 128 * 4 + 16 * 128 * 4 +
                        2 * 16 * 4;
    static bool attr = false;
    if (!attr) {
      hipFuncSetAttribute((const void*)&k_attn_decode_short<4>,
                          hipFuncAttributeMaxDynamicSharedMemorySize, 80 * 1024);
      hipFuncSetAttribute((const void*)&k_attn_decode_short<8>,
                          hipFuncAttributeMaxDynamicSharedMemorySize,
                          144 * 1024);
      attr = true;
    }
    if (nchunk == 4)
      hipLaunchKernelGGL(k_attn_decode_short<4>, dim3(nh / 4), dim3(1024),
                         smem, s, q, kc, vc, pos, out, nh, nkv, max_seq,
                         window);
    else
      hipLaunchKernelGGL(k_attn_decode_short<8>, dim3(nh / 2), dim3(1024),
                         smem, s, q, kc, vc, pos, out, nh, nkv, max_seq,
                         window);
    return;
  }
  if (gy > 0) {
    const int G = nh / nkv;
    const int GB = (G >= 4) ? 4 : G;
    const int subg = gy / nkv;
    // smem: K dbuf + V dbuf + scores[GB][64] + q f32 [GB][128] + scratch
    const size_t smem = 4 * 64 * 256 + (size_t)GB * 64 * 4 +
                        (size_t)GB * 128 * 4 + 4 * 136 * 4;
    static const int probe =
        getenv("CAKE_ATTN_PROBE") ? atoi(getenv("CAKE_ATTN_PROBE")) : 0;
    if (GB == 4)
      hipLaunchKernelGGL(k_attn_decode_g<4>, dim3(nchunk, gy), dim3(256),
                         smem, s, q, kc, vc, pos, ws, cnt, out, nh, nkv,
                         max_seq, nchunk, window, subg, probe);
    else if (GB == 2)
      hipLaunchKernelGGL(k_attn_decode_g<2>, dim3(nchunk, gy), dim3(256),
                         smem, s, q, kc, vc, pos, ws, cnt, out, nh, nkv,
                         max_seq, nchunk, window, subg, probe);
    else
      hipLaunchKernelGGL(k_attn_decode_g<1>, dim3(nchunk, gy), dim3(256),
                         smem, s, q, kc, vc, pos, ws, cnt, out, nh, nkv,
                         max_seq, nchunk, window, subg, probe);
    return;
  }
  hipLaunchKernelGGL(k_attn_decode_fused, dim3(nchunk, nh), dim3(256), 0, s,
                     q, kc, vc, pos, ws, cnt, out, nh, nkv, hd, max_seq,
                     nchunk, window);
}
// Product dispatch policy: the MFMA-prefill variant launch_attn_prefill
// picks for (S, nh, hd), from the env knobs (read once) and the size rules.
PfVariant attn_prefill_policy(int S, int nh, int hd) {
  static const int pfv =
      getenv("CAKE_PF_ATTN") ? atoi(getenv("CAKE_PF_ATTN")) : 2;
  static const int nw_env =
      getenv("CAKE_PF_NW") ? atoi(getenv("CAKE_PF_NW")) : 0;
  // split-KV default OFF: measured NEGATIVE at 8B S=2048 (attention
  // 4.73 -> 5.41 ms; 4k-prefill 62.0k -> 59.4k tok/s).  With the NW=4
  // 2-blocks/CU occupancy the scheduler already backfills the causal
  // skew, so halving every block's range only doubles the per-block
  // staging/prologue cost and adds the combine pass
  // (profiles/r02_NOTES.md).  Kept behind CAKE_PF_SPLIT=1.
  static const int split_env =
      getenv("CAKE_PF_SPLIT") ? atoi(getenv("CAKE_PF_SPLIT")) : 0;
  static const int deep_env =
      getenv("CAKE_PF_DEEP") ? atoi(getenv("CAKE_PF_DEEP")) : 0;
  if (hd == 256) {  // MFMA-256 (v1 structure, 4 waves) or the plain kernel
    PfVariant v256;
    v256.pfv = pfv == 0 ? 0 : 1;
    v256.nw = pfv == 0 ? 0 : 4;
    return v256;
  }
  // 128-row blocks whenever the 256-row grid can't give the scheduler
  // >= 2 blocks/CU of backfill against the causal work skew
  const bool nw4 = nw_env ? nw_env == 4
                          : (long)((S + 255) / 256) * nh < 512;
  PfVariant v;
  v.pfv = pfv;
  v.nw = nw4 ? 4 : 8;
  v.split = split_env != 0;
  v.deep = deep_env;
  // split-KV halves every block's own tile range (the wall is the
  // longest block); below S=1024 the extra combine launch costs more
  // than the balance buys (launch-bound small models)
  v.split_min_s = 1024;
  return v;
}
void launch_attn_prefill(const u16* qkv, const u16* kc, const u16* vc,
                         const u16* vtc, u16* out, float* ws, int S, int pos0,
                         int nh, int nkv, int hd, int max_seq, int qkv_stride,
                         int out_stride, int window, hipStream_t s) {
  launch_attn_prefill_variant(qkv, kc, vc, vtc, out, ws, S, pos0, nh, nkv,
                              hd, max_seq, qkv_stride, out_stride, window,
                              attn_prefill_policy(S, nh, hd), s);
}
void launch_attn_prefill_variant(const u16* qkv, const u16* kc,
                                 const u16* vc, const u16* vtc, u16* out,
                                 float* ws, int S, int pos0, int nh, int nkv,
                                 int hd, int max_seq, int qkv_stride,
                                 int out_stride, int window, PfVariant v,
                                 hipStream_t s) {
  const int pfv = v.pfv;
  if (hd == 256) {
    launch_attn_prefill_256(qkv, kc, vc, vtc, out, S, pos0, nh, nkv, max_seq,
                            qkv_stride, out_stride, window, pfv != 0, s);
    return;
  }
  if (hd == 128 && pfv >= 2) {
    const size_t smem2 = 2 * 32 * 256 + 2 * 128 * 64;
    const size_t smem3 = 3 * 32 * 256 + 3 * 128 * 64;
    const bool nw4 = v.nw == 4;
    const bool split = v.split && ws != nullptr && S >= v.split_min_s;
    const int deep = (!split && (v.deep == 1 || v.deep == 2)) ? v.deep : 0;
    const int gz = split ? 2 : 1;
    if (nw4 && split)
      hipLaunchKernelGGL((k_attn_prefill_mfma2<4, 2, 0>),
                         dim3((S + 127) / 128, nh, gz), dim3(256), smem2, s,
                         qkv, kc, vtc, out, ws, S, pos0, nh, nkv, max_seq,
                         qkv_stride, out_stride, window);
    else if (nw4 && deep == 2)
      hipLaunchKernelGGL((k_attn_prefill_mfma2<4, 1, 2>),
                         dim3((S + 127) / 128, nh, 1), dim3(256), smem3, s,
                         qkv, kc, vtc, out, ws, S, pos0, nh, nkv, max_seq,
                         qkv_stride, out_stride, window);
    else if (nw4 && deep == 1)
      hipLaunchKernelGGL((k_attn_prefill_mfma2<4, 1, 1>),
                         dim3((S + 127) / 128, nh, 1), dim3(256), smem3, s,
                         qkv, kc, vtc, out, ws, S, pos0, nh, nkv, max_seq,
                         qkv_stride, out_stride, window);
    else if (nw4)
      hipLaunchKernelGGL((k_attn_prefill_mfma2<4, 1, 0>),
                         dim3((S + 127) / 128, nh, 1), dim3(256), smem2, s,
                         qkv, kc, vtc, out, ws, S, pos0, nh, nkv, max_seq,
                         qkv_stride, out_stride, window);
    else if (split)
      hipLaunchKernelGGL((k_attn_prefill_mfma2<8, 2, 0>),
                         dim3((S + 255) / 256, nh, gz), dim3(512), smem2, s,
                         qkv, kc, vtc, out, ws, S, pos0, nh, nkv, max_seq,
                         qkv_stride, out_stride, window);
    else if (deep == 2)
      hipLaunchKernelGGL((k_attn_prefill_mfma2<8, 1, 2>),
                         dim3((S + 255) / 256, nh, 1), dim3(512), smem3, s,
                         qkv, kc, vtc, out, ws, S, pos0, nh, nkv, max_seq,
                         qkv_stride, out_stride, window);
    else if (deep == 1)
      hipLaunchKernelGGL((k_attn_prefill_mfma2<8, 1, 1>),
                         dim3((S + 255) / 256, nh, 1), dim3(512), smem3, s,
                         qkv, kc, vtc, out, ws, S, pos0, nh, nkv, max_seq,
                         qkv_stride, out_stride, window);
    else
      hipLaunchKernelGGL((k_attn_prefill_mfma2<8, 1, 0>),
                         dim3((S + 255) / 256, nh, 1), dim3(512), smem2, s,
                         qkv, kc, vtc, out, ws, S, pos0, nh, nkv, max_seq,
                         qkv_stride, out_stride, window);
    if (split)
      hipLaunchKernelGGL(k_attn_pf_combine, dim3(((long)S * nh + 1) / 2),
                         dim3(256), 0, s, ws, out, S, nh, out_stride);
  } else if (hd == 128) {
    hipLaunchKernelGGL(k_attn_prefill_mfma, dim3((S + 255) / 256, nh),
                       dim3(512), 0, s, qkv, kc, vtc, out, S, pos0, nh, nkv,
                       max_seq, qkv_stride, out_stride, window);
  } else {
    hipLaunchKernelGGL(k_attn_prefill, dim3((S + 3) / 4, nh), dim3(256), 0, s,
                       qkv, kc, vc, out, S, pos0, nh, nkv, hd, max_seq,
                       qkv_stride, out_stride, window);
  }
}

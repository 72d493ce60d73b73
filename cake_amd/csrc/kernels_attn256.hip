#include "kernels_common.h"
#include "kernels.h"

#include <algorithm>

// ---------------------------------------------------------------------------
// Attention at head_dim 256 (Falcon3; the widest of Gemma 3's needs).  Its
// own translation unit so that no kernel of kernels_attn.hip changes by an
// instruction (kernels_common.h, rule 19): only the host-side routing there
// knows about this file.
//
// K/V rows are 512 B.  All three kernels read K/V straight into registers
// (guide "Attention decode (single-token)": up to 8 query rows per kv head
// -> no LDS staging of the tiles).
// ---------------------------------------------------------------------------
namespace {
constexpr int HD = 256;
constexpr int TILE = 64;

#define WS_STORE(p, v)                                                     \
  __hip_atomic_store((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

// ---------------------------------------------------------------------------
// Decode: semantics of k_attn_decode_fused (f32 online softmax, scale
// 1/sqrt(hd), span [max(0, n - window), n), split-KV over nchunk chunks, ws
// row (hd + 4) floats per (head, chunk), one combining block), but ONE block
// serves GB q-heads of one kv head and reads each K row and each V row of its
// chunk once.
//
//   grid (nchunk, nh / GB), block 256 (4 waves), 64-position tiles.
//   A: 32 lanes per position (16 B of the K row each), 8 positions per pass,
//      8 passes.  Each thread forms 8*GB partial dots against the GB q
//      slices it keeps in registers; the 32-lane sums are a butterfly
//      REDUCE-SCATTER (each step halves the values a lane carries), 31
//      shuffles for 32 sums instead of 5 per sum.
//   B: wave g < GB runs head g's online-softmax step, lane = position; the
//      weights overwrite the scores in LDS, alpha goes through LDS.
//   C: wave w takes positions 16w..16w+15 of the tile, lane = 4 dims (one
//      8-B load per V row, 64 lanes = the 512-B row); the row feeds all GB
//      accumulators, weights are broadcast b128 LDS reads.
// Loads are unguarded with rows clamped to end-1 (masked by -INF scores / 0
// weights), as in k_attn_decode_fused; the next tile's K loads issue ahead
// of phase C.
//
// GB > 1 is correct and tested, and measured slower than GB 1 (phase A's
// 8*GB-value reduction and a GB-times longer serial tile on GB-times fewer
// blocks outweigh the saved KV reads; see attn256_group): opt-in only.
//
// Election: the block whose arrival draws nchunk-1 combines, and puts the
// word back to 0 before it does — nothing rests on a u32 count that never
// wraps, and a launch may follow one with another nchunk.  Partials are
// published with sc1 stores + vmcnt(0) as in k_attn_decode_fused; the
// combiner takes one agent acquire and reads them with plain loads.
// ---------------------------------------------------------------------------
template <int GB>
struct Sm256 {
  float so[4][GB][HD];     // per-wave partial o; the combine's staging
  float stile[GB][TILE];   // scores, then softmax weights
  float alpha[GB];
  float ml[GB][2];
  int elected;
};

template <int GB>
__global__ __launch_bounds__(256) void k_attn_decode_256(
    const u16* __restrict__ q, const u16* __restrict__ kc,
    const u16* __restrict__ vc, const int* __restrict__ pos,
    float* __restrict__ ws, u32* __restrict__ cnt, u16* __restrict__ outbuf,
    int nh, int nkv, int max_seq, int nchunk, int window, int subg) {
  constexpr int GP = GB == 3 ? 4 : GB;  // heads padded to a power of two
  constexpr int NV = 8 * GP;            // partial dots per thread and tile
  constexpr int LOGNV = GP == 1 ? 3 : GP == 2 ? 4 : 5;
  __shared__ __attribute__((aligned(16))) Sm256<GB> sm;

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
  const int dgrp = t & 31, prow = t >> 5;
  const float scale = rsqrtf((float)HD);
  const u16* kbase = kc + (size_t)kvh * max_seq * HD;
  const u16* vbase = vc + (size_t)kvh * max_seq * HD;

  float qa[GB][8];
#pragma unroll
  for (int g = 0; g < GB; ++g)
#pragma unroll
    for (int j = 0; j < 8; ++j)
      qa[g][j] = b2f(q[(size_t)(h0 + g) * HD + dgrp * 8 + j]);

  float o[GB][4];
#pragma unroll
  for (int g = 0; g < GB; ++g)
#pragma unroll
    for (int e = 0; e < 4; ++e) o[g][e] = 0.f;
  float m = -INFINITY, l = 0.f;  // head `wid`'s, in waves wid < GB

  short8 ka[8];
  auto issue_k = [&](int s0) {
#pragma unroll
    for (int pass = 0; pass < 8; ++pass) {
      const int pc = max(0, min(s0 + pass * 8 + prow, end - 1));
      ka[pass] =
          *reinterpret_cast<const short8*>(kbase + (size_t)pc * HD + dgrp * 8);
    }
  };
  if (start < end) issue_k(start);
  for (int sub0 = start; sub0 < end; sub0 += TILE) {
    // ---- A: v[g*8 + pass] = this thread's 8-dim share of (head g,
    // position pass*8 + prow) ---------------------------------------------
    float v[NV];
#pragma unroll
    for (int g = 0; g < GP; ++g)
#pragma unroll
      for (int pass = 0; pass < 8; ++pass) {
        float d = 0.f;
        if (g < GB) {
#pragma unroll
          for (int j = 0; j < 8; ++j)
            d = fmaf(b2f((u16)ka[pass][j]), qa[g < GB ? g : 0][j], d);
        }
        v[g * 8 + pass] = d;
      }
    // reduce-scatter over the 32 lanes of a position group: at mask 16 >> s
    // a lane keeps the half of its values that its bit selects and hands the
    // other half to its partner, so after LOGNV steps lane dgrp holds the
    // full sum of value (dgrp >> (5 - LOGNV)) in v[0]
#pragma unroll
    for (int s = 0; s < LOGNV; ++s) {
      const int half = NV >> (s + 1);
      const int mask = 16 >> s;
      const bool up = (dgrp & mask) != 0;
#pragma unroll
      for (int i = 0; i < half; ++i) {
        const float keep = up ? v[i + half] : v[i];
        const float send = up ? v[i] : v[i + half];
        v[i] = keep + __shfl_xor(send, mask, 32);
      }
    }
#pragma unroll
    for (int s = LOGNV; s < 5; ++s) v[0] += __shfl_xor(v[0], 16 >> s, 32);
    {
      const int idx = dgrp >> (5 - LOGNV);
      const int g = idx >> 3, pp = (idx & 7) * 8 + prow;
      if ((dgrp & ((1 << (5 - LOGNV)) - 1)) == 0 && g < GB)
        sm.stile[g][pp] = (sub0 + pp < end) ? v[0] * scale : -INFINITY;
    }
    __syncthreads();
    // ---- B: online-softmax step of head wid, lane = position -------------
    if (wid < GB) {
      const float sv = sm.stile[wid][lane];
      float tm = wave_max(sv);
      tm = __shfl(tm, 0, WAVE);
      const float mnew = fmaxf(m, tm);
      const float alpha = (mnew == -INFINITY) ? 0.f : __expf(m - mnew);
      const float ew = (sv == -INFINITY) ? 0.f : __expf(sv - mnew);
      float ts = wave_sum(ew);
      ts = __shfl(ts, 0, WAVE);
      l = l * alpha + ts;
      m = mnew;
      sm.stile[wid][lane] = ew;
      if (lane == 0) sm.alpha[wid] = alpha;
    }
    __syncthreads();
    // next tile's K rows ride the memory system behind phase C's loads
    if (sub0 + TILE < end) issue_k(sub0 + TILE);
    // ---- C: PV, wave = 16 positions, lane = dims 4*lane .. 4*lane+3 ------
#pragma unroll
    for (int g = 0; g < GB; ++g) {
      const float a = sm.alpha[g];
#pragma unroll
      for (int e = 0; e < 4; ++e) o[g][e] *= a;
    }
    uint2 vv[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int pc = max(0, min(sub0 + wid * 16 + u, end - 1));
      vv[u] = *reinterpret_cast<const uint2*>(vbase + (size_t)pc * HD +
                                              4 * lane);
    }
#pragma unroll
    for (int u4 = 0; u4 < 4; ++u4) {
      f32x4 w[GB];
#pragma unroll
      for (int g = 0; g < GB; ++g)
        w[g] = *reinterpret_cast<const f32x4*>(&sm.stile[g][wid * 16 + u4 * 4]);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const uint2 x = vv[u4 * 4 + e];
        const float v0 = b2f((u16)(x.x & 0xffffu)), v1 = b2f((u16)(x.x >> 16));
        const float v2 = b2f((u16)(x.y & 0xffffu)), v3 = b2f((u16)(x.y >> 16));
#pragma unroll
        for (int g = 0; g < GB; ++g) {
          o[g][0] = fmaf(w[g][e], v0, o[g][0]);
          o[g][1] = fmaf(w[g][e], v1, o[g][1]);
          o[g][2] = fmaf(w[g][e], v2, o[g][2]);
          o[g][3] = fmaf(w[g][e], v3, o[g][3]);
        }
      }
    }
    __syncthreads();  // stile / alpha reused by the next tile
  }

  // ---- the four waves' partial o, and (m, l) per head, through LDS --------
#pragma unroll
  for (int g = 0; g < GB; ++g)
#pragma unroll
    for (int e = 0; e < 4; ++e) sm.so[wid][g][4 * lane + e] = o[g][e];
  if (wid < GB && lane == 0) {
    sm.ml[wid][0] = m;
    sm.ml[wid][1] = l;
  }
  __syncthreads();
  if (nchunk == 1) {  // this block holds the complete (o, m, l): no ws round
#pragma unroll
    for (int g = 0; g < GB; ++g) {
      const float s4 = sm.so[0][g][t] + sm.so[1][g][t] + sm.so[2][g][t] +
                       sm.so[3][g][t];
      outbuf[(size_t)(h0 + g) * HD + t] = f2b(s4 / sm.ml[g][1]);
    }
    return;
  }
#pragma unroll
  for (int g = 0; g < GB; ++g) {
    float* wsrow = ws + ((size_t)(h0 + g) * nchunk + chunk) * (HD + 4);
    WS_STORE(&wsrow[t], sm.so[0][g][t] + sm.so[1][g][t] + sm.so[2][g][t] +
                            sm.so[3][g][t]);
    if (t < 2) WS_STORE(&wsrow[HD + t], sm.ml[g][t]);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every wave drains
  __syncthreads();
  if (t == 0) {
    const u32 a = __hip_atomic_fetch_add(&cnt[yb], 1u, __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_AGENT);
    const bool last = a == (u32)(nchunk - 1);
    // the word goes back to 0: every block of this launch has arrived, and
    // the next launch is stream-ordered behind this one
    if (last)
      __hip_atomic_store(&cnt[yb], 0u, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
    sm.elected = last ? 1 : 0;
  }
  __syncthreads();
  if (!sm.elected) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");

  // ---- combine the GB heads (one block per launch and kv group) -----------
  float* cm = &sm.so[0][0][0];  // [64] chunk maxima
  float* cl = &sm.so[1][0][0];  // [64] chunk sums
  float* cw = &sm.so[2][0][0];  // [64] chunk weights
  for (int g = 0; g < GB; ++g) {
    const float* base = ws + (size_t)(h0 + g) * nchunk * (HD + 4);
    if (t < nchunk) {
      cm[t] = base[(size_t)t * (HD + 4) + HD];
      cl[t] = base[(size_t)t * (HD + 4) + HD + 1];
    }
    __syncthreads();
    float M = -INFINITY;
    for (int c = 0; c < nchunk; ++c) M = fmaxf(M, cm[c]);
    float L = 0.f;
    for (int c = 0; c < nchunk; ++c)
      if (cm[c] != -INFINITY) L += cl[c] * __expf(cm[c] - M);
    // an empty chunk stored m = -INF and a zero partial: weight 0
    if (t < nchunk) cw[t] = (cm[t] == -INFINITY) ? 0.f : __expf(cm[t] - M);
    __syncthreads();
    float acc = 0.f;
#pragma unroll 8
    for (int c = 0; c < nchunk; ++c)
      acc = fmaf(base[(size_t)c * (HD + 4) + t], cw[c], acc);
    outbuf[(size_t)(h0 + g) * HD + t] = f2b(acc / L);
    __syncthreads();  // cm / cl / cw reused by the next head
  }
}

// ---------------------------------------------------------------------------
// Plain prefill: k_attn_prefill with four dims per lane (one 8-B load per
// row and lane) and P in f32.  One wave per query row, 4 rows per block.
// What CAKE_PF_ATTN=0 runs at hd 256, and the tests' cross-check.
// ---------------------------------------------------------------------------
__device__ inline void unpack4(uint2 x, float (&f)[4]) {
  f[0] = b2f((u16)(x.x & 0xffffu));
  f[1] = b2f((u16)(x.x >> 16));
  f[2] = b2f((u16)(x.y & 0xffffu));
  f[3] = b2f((u16)(x.y >> 16));
}

__global__ __launch_bounds__(256) void k_attn_prefill_256(
    const u16* __restrict__ qkv, const u16* __restrict__ kc,
    const u16* __restrict__ vc, u16* __restrict__ out, int S, int pos0,
    int nh, int nkv, int max_seq, int qkv_stride, int out_stride,
    int window) {
  const int h = blockIdx.y;
  const int t = threadIdx.x, wid = t / WAVE, lane = t % WAVE;
  const int sidx = blockIdx.x * 4 + wid;
  if (sidx >= S) return;
  const int kvh = h / (nh / nkv);
  const int e0 = 4 * lane;
  const int n = pos0 + sidx + 1;  // causal: attend to <= own position
  float qf[4], kf[4], vf[4];
  unpack4(*reinterpret_cast<const uint2*>(qkv + (size_t)sidx * qkv_stride +
                                          (size_t)h * HD + e0),
          qf);
  const float scale = rsqrtf((float)HD);
  float m = -INFINITY, l = 0.f, o[4] = {0.f, 0.f, 0.f, 0.f};
  const u16* kbase = kc + (size_t)kvh * max_seq * HD + e0;
  const u16* vbase = vc + (size_t)kvh * max_seq * HD + e0;
  const int p0 = (window > 0 && n > window) ? n - window : 0;
  for (int p = p0; p < n; ++p) {
    unpack4(*reinterpret_cast<const uint2*>(kbase + (size_t)p * HD), kf);
    unpack4(*reinterpret_cast<const uint2*>(vbase + (size_t)p * HD), vf);
    float dot = qf[0] * kf[0] + qf[1] * kf[1] + qf[2] * kf[2] + qf[3] * kf[3];
    dot = wave_sum(dot) * scale;
    dot = __shfl(dot, 0, WAVE);
    const float mn = fmaxf(m, dot);
    const float alpha = __expf(m - mn);
    const float pw = __expf(dot - mn);
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = o[e] * alpha + pw * vf[e];
    l = l * alpha + pw;
    m = mn;
  }
  u16* orow = out + (size_t)sidx * out_stride + (size_t)h * HD + e0;
  const float inv = 1.f / l;
  uint2 r;
  r.x = (u32)f2b(o[0] * inv) | ((u32)f2b(o[1] * inv) << 16);
  r.y = (u32)f2b(o[2] * inv) | ((u32)f2b(o[3] * inv) << 16);
  *reinterpret_cast<uint2*>(orow) = r;
}

// ---------------------------------------------------------------------------
// MFMA prefill: the structure of k_attn_prefill_mfma (swapped QK^T so the
// softmax column is lane-local, in-register P -> bf16 A-fragments, V^T
// B-fragments), sixteen K=16 steps over the head and eight 32-wide output
// blocks.  O alone is 128 accumulator registers per lane, so this is a
// one-wave-per-SIMD kernel: 4 waves, 128 query rows per block.  V^T
// fragments are loaded per K=16 window (8 at a time) to keep the live set
// down.  No LDS, no barriers.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_attn_prefill_mfma_256(
    const u16* __restrict__ qkv, const u16* __restrict__ kc,
    const u16* __restrict__ vtc, u16* __restrict__ out, int S, int pos0,
    int nh, int nkv, int max_seq, int qkv_stride, int out_stride,
    int window) {
  const int w = threadIdx.x / WAVE;
  const int lane = threadIdx.x % WAVE;
  const int lhalf = lane >> 5, lq = lane & 31;
  const int h = blockIdx.y;
  const int kvh = h / (nh / nkv);
  const int qb = blockIdx.x * 128 + w * 32;
  if (qb >= S) return;

  // Q fragments (persistent): B[k][j=q], lane holds q = lq, dims
  // kk*16 + lhalf*8 .. +8
  bf16x8 qf[16];
  {
    const int row = min(qb + lq, S - 1);
    const u16* qrow = qkv + (size_t)row * qkv_stride + (size_t)h * HD;
#pragma unroll
    for (int kk = 0; kk < 16; ++kk)
      qf[kk] = *reinterpret_cast<const bf16x8*>(qrow + kk * 16 + lhalf * 8);
  }

  f32x16 oacc[8];
#pragma unroll
  for (int db = 0; db < 8; ++db)
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[db][r] = 0.f;
  float m = -INFINITY, l = 0.f;
  const float scale = rsqrtf((float)HD);
  const int q_abs = pos0 + qb + lq;
  const bool q_valid = qb + lq < S;
  const int n_wave = pos0 + min(qb + 32, S);  // kv needed by this wave
  const int ntiles = (n_wave + 31) / 32;
  // sliding window: whole tiles below the wave's smallest query's span skip
  const int tile0 =
      (window > 0) ? max(0, pos0 + qb - (window - 1)) / 32 : 0;
  const u16* kbase = kc + (size_t)kvh * max_seq * HD;
  const u16* vtbase = vtc + (size_t)kvh * HD * max_seq;

  bf16x8 kf[16];
  auto load_k = [&](int pkv) {
    const u16* krow = kbase + (size_t)(pkv + lq) * HD;
#pragma unroll
    for (int kk = 0; kk < 16; ++kk)
      kf[kk] = *reinterpret_cast<const bf16x8*>(krow + kk * 16 + lhalf * 8);
  };
  load_k(tile0 * 32);
  for (int tile = tile0; tile < ntiles; ++tile) {
    const int pkv = tile * 32;
    f32x16 p;
#pragma unroll
    for (int r = 0; r < 16; ++r) p[r] = 0.f;
#pragma unroll
    for (int kk = 0; kk < 16; ++kk)
      p = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[kk], qf[kk], p, 0, 0, 0);
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
    // pack expP to bf16 pairs and exchange halves: each lane can then
    // assemble A[i=q=lq][k=kv] fragments for PV
    u32 pk[8], rcv[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      pk[i] = (u32)f2b(ep[2 * i]) | ((u32)f2b(ep[2 * i + 1]) << 16);
      rcv[i] = __shfl_xor(pk[i], 32, WAVE);
    }
    // per-row alpha for the O rescale (row q via lane shuffle)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float ar =
          __shfl(alpha, (r & 3) + 8 * (r >> 2) + 4 * lhalf, WAVE);
#pragma unroll
      for (int db = 0; db < 8; ++db) oacc[db][r] *= ar;
    }
    // PV: two K=16 windows over the 32-kv tile, V^T loaded per window
#pragma unroll
    for (int kk = 0; kk < 2; ++kk) {
      bf16x8 vf[8];
#pragma unroll
      for (int db = 0; db < 8; ++db)
        vf[db] = *reinterpret_cast<const bf16x8*>(
            vtbase + (size_t)(db * 32 + lq) * max_seq + pkv + 16 * kk +
            lhalf * 8);
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
      for (int db = 0; db < 8; ++db)
        oacc[db] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(
            af.v, vf[db], oacc[db], 0, 0, 0);
    }
  }

  // epilogue: divide by l (per q row, via shuffle) and store
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int qrow = (r & 3) + 8 * (r >> 2) + 4 * lhalf;
    const float inv = 1.f / __shfl(l, qrow, WAVE);
    const int srow = qb + qrow;
    if (srow < S) {
#pragma unroll
      for (int db = 0; db < 8; ++db)
        out[(size_t)srow * out_stride + (size_t)h * HD + db * 32 + lq] =
            f2b(oacc[db][r] * inv);
    }
  }
}
#undef WS_STORE
}  // namespace

// q-heads per block of k_attn_decode_256: the largest of 4, 3, 2, 1 that
// divides G and is within the cap CAKE_ATTN256_GB (read per launch, so a test
// or an A/B run can flip it).  The cap defaults to 1, the per-head route: the
// grouped instantiations measured SLOWER per launch at every G and context
// (G = 3 on Falcon3-7B: 29.4 / 53.8 / 77.5 us against 11.5 / 21.7 / 36.6 at
// contexts 128 / 2040 / 7900; G = 2 1.4x, G = 4 2.6x), so
// they run only under CAKE_ATTN256_GB=2|3|4.
int attn256_group(int nh, int nkv) {
  if (nkv <= 0 || nh <= 0 || nh % nkv != 0) return 1;
  const char* e = getenv("CAKE_ATTN256_GB");
  const int cap = e ? std::max(1, std::min(4, atoi(e))) : 1;
  const int G = nh / nkv;
  for (int gb = cap; gb > 1; --gb)
    if (G % gb == 0) return gb;
  return 1;
}

void launch_attn_decode_256(const u16* q, const u16* kc, const u16* vc,
                            const int* pos, float* ws, u32* cnt, u16* out,
                            int nh, int nkv, int max_seq, int nchunk,
                            int window, hipStream_t s) {
  const int GB = attn256_group(nh, nkv);
  const int subg = (nh / nkv) / GB;
  const dim3 grid(nchunk, nh / GB);
#define LAUNCH256(N)                                                        \
  hipLaunchKernelGGL(k_attn_decode_256<N>, grid, dim3(256), 0, s, q, kc, vc, \
                     pos, ws, cnt, out, nh, nkv, max_seq, nchunk, window,   \
                     subg)
  if (GB == 4) LAUNCH256(4);
  else if (GB == 3) LAUNCH256(3);
  else if (GB == 2) LAUNCH256(2);
  else LAUNCH256(1);
#undef LAUNCH256
}

void launch_attn_prefill_256(const u16* qkv, const u16* kc, const u16* vc,
                             const u16* vtc, u16* out, int S, int pos0,
                             int nh, int nkv, int max_seq, int qkv_stride,
                             int out_stride, int window, int mfma,
                             hipStream_t s) {
  if (mfma)
    hipLaunchKernelGGL(k_attn_prefill_mfma_256, dim3((S + 127) / 128, nh),
                       dim3(256), 0, s, qkv, kc, vtc, out, S, pos0, nh, nkv,
                       max_seq, qkv_stride, out_stride, window);
  else
    hipLaunchKernelGGL(k_attn_prefill_256, dim3((S + 3) / 4, nh), dim3(256), 0,
                       s, qkv, kc, vc, out, S, pos0, nh, nkv, max_seq,
                       qkv_stride, out_stride, window);
}

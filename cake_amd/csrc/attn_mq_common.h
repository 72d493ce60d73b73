// What the grouped MFMA decode kernels share: k_attn_decode_mq<64|128>
// (kernels_attn_mq.hip, bf16 cache) and k_attn_decode_kv8_mq
// (kernels_kv8_mq.hip, e4m3 cache).  Included by those two files and by
// kernels_attn_mq256.hip, whose k_attn_decode_mq256 keeps this contract with a
// 16-position wave step (wave w owns start + 16 w + 64 i .. + 16) and a softmax
// step of its own, and ends in the same mq_epilogue.
//
// Work split.  Grid (nchunk, nkv), 4 waves.  A block serves all G <= 16 heads
// of kv head blockIdx.y, padded to ONE 16-row MFMA operand, over chunk
// [start, end) of decode_span.  Wave w owns positions start + 32 w + 128 i ..
// + 32 through its own (m, l, O^T) for the 16 head rows (head = lane % 16); the
// main loop has no block barrier, every load address is clamped into
// [start, end - 1] and only the chunk's end is masked to -inf.  The main loops
// differ in every line (loads, staging, fragment reads) and stay in the kernel
// files; each calls mq_softmax_step once per 32-position step and ends in
// mq_epilogue.
//
// Split-KV contract: that of launch_attn_decode.  The 4 waves merge (m, l, O)
// once through LDS at the end of the chunk.  ws[h][chunk] = {o[hd], m, l} at
// stride hd + 4, agent-scope relaxed stores + vmcnt(0) drain, then an arrival
// counter cnt[kvh] (nkv words); the LAST-arriving block of a kv head combines
// the partials of all G heads behind one agent-scope acquire.  No block ever
// waits on another.  The elected block stores 0 to its word, so between these
// kernels' own launches the word is 0 and the chunk count may change freely on
// one zeroing.  The election is still modulo nchunk: launch_attn_decode hands
// the same words to its other kernels, which leave them at multiples of the
// chunk count, and the engine re-zeroes them when that count changes.  An
// empty chunk publishes m = -inf, l = 0, o = 0 and weighs exactly 0.
// nchunk == 1 writes the output directly, with no ws and no counter.  The
// combine keeps one weight per (head, chunk) in a [16][64] LDS table: the
// launchers refuse nchunk > 64.
#pragma once
#include "kernels_common.h"

// LDS traffic of one wave is in order; this only keeps the compiler from
// moving a lane's LDS reads across another lane's writes
__device__ inline void mq_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// One online-softmax step over a wave's 32 positions, per head = lane % 16.
// sc[t][r] is the score of position 16 t + 4 (lane / 16) + r, -inf where
// masked.  A head's tile max and sum are 8 registers plus two cross-lane steps
// (xor 16, xor 32).  P is split into bf16 hi + bf16 lo (lo = bf16(p - hi),
// |p - hi - lo| <= 2^-17 p) so that two MFMAs per V fragment keep P at
// f32-kernel accuracy; a masked position's P is exactly 0.  With PSCALE, p is
// multiplied by vsc[t][r] before the split and l still sums the unscaled
// exponentials; without it vsc is not read.  Updates m and l.
struct MqStep {
  float alpha;      // rescale of the running O^T and l
  bf16x8 phi, plo;  // B fragments of P
};
template <bool PSCALE>
__device__ inline MqStep mq_softmax_step(const float (&sc)[2][4],
                                         const f32x4* vsc, float& m, float& l,
                                         int lhalf) {
  float tm = -INFINITY;
#pragma unroll
  for (int tt = 0; tt < 2; ++tt)
#pragma unroll
    for (int r = 0; r < 4; ++r) tm = fmaxf(tm, sc[tt][r]);
  tm = fmaxf(tm, __shfl_xor(tm, 16, WAVE));
  tm = fmaxf(tm, halfswap32f(tm, lhalf));
  const float mnew = fmaxf(m, tm);
  const float alpha = (mnew == -INFINITY) ? 0.f : __expf(m - mnew);
  float tsum = 0.f;
  union { u32 u[4]; bf16x8 v; } phi, plo;
#pragma unroll
  for (int tt = 0; tt < 2; ++tt) {
    float p[4], d[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float e =
          (sc[tt][r] == -INFINITY) ? 0.f : __expf(sc[tt][r] - mnew);
      tsum += e;
      if constexpr (PSCALE)
        p[r] = e * vsc[tt][r];        // exact: the scale is a power of two
      else
        p[r] = e;
    }
    phi.u[2 * tt] = pack_bf16(p[0], p[1]);
    phi.u[2 * tt + 1] = pack_bf16(p[2], p[3]);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const u32 h = phi.u[2 * tt + (r >> 1)];
      union { u32 u; float f; } hv{(r & 1) ? (h & 0xffff0000u) : (h << 16)};
      d[r] = p[r] - hv.f;
    }
    plo.u[2 * tt] = pack_bf16(d[0], d[1]);
    plo.u[2 * tt + 1] = pack_bf16(d[2], d[3]);
  }
  tsum += __shfl_xor(tsum, 16, WAVE);
  tsum += halfswap32f(tsum, lhalf);
  l = l * alpha + tsum;
  m = mnew;
  return {alpha, phi.v, plo.v};
}

__device__ inline void mq_ws_store(float* p, float v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Everything after the main loop: merge the block's 4 waves, then either write
// the output (nchunk == 1) or publish the chunk's partial and, in the
// last-arriving block of the kv head, combine.  smem is the kernel's 4 wave
// slices of WSL bytes (16-B aligned), free for reuse once every wave is here;
// acc is O^T (acc[db][r] = dim 16 db + 4 (lane / 16) + r of head lane % 16).
template <int HD, int WSL>
__device__ inline void mq_epilogue(unsigned char* smem,
                                   const f32x4 (&acc)[HD / 16], float m,
                                   float l, float* ws, u32* cnt, u16* outbuf,
                                   int kvh, int chunk, int G, int nchunk,
                                   int t) {
  constexpr int DB = HD / 16;   // 16-dim blocks of O^T
  constexpr int OROW = HD + 1;  // merge image row, floats
  static_assert(16 * OROW * 4 + 128 <= WSL, "merge image fits a wave slice");
  static_assert(4 * WSL >= (16 * 64 + 16) * 4, "combine staging fits");
  __shared__ int elected;
  const int w = t / WAVE, lane = t % WAVE;
  const int g = lane >> 4, c16 = lane & 15;

  // ---- merge the 4 waves' (m, l, O) through LDS ---------------------------
  mq_wave_sync();
  float* fo = reinterpret_cast<float*>(smem + w * WSL);  // [16][OROW], m, l
#pragma unroll
  for (int db = 0; db < DB; ++db)
#pragma unroll
    for (int r = 0; r < 4; ++r)
      fo[c16 * OROW + db * 16 + 4 * g + r] = acc[db][r];
  if (g == 0) {
    fo[16 * OROW + c16] = m;
    fo[16 * OROW + 16 + c16] = l;
  }
  __syncthreads();
  for (int idx = t; idx < G * HD; idx += 256) {
    const int hh = idx / HD, d = idx % HD;
    float mw[4], M = -INFINITY;
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      mw[x] = reinterpret_cast<const float*>(smem + x * WSL)[16 * OROW + hh];
      M = fmaxf(M, mw[x]);
    }
    float o = 0.f, L = 0.f;
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      const float* fx = reinterpret_cast<const float*>(smem + x * WSL);
      const float wt = (mw[x] == -INFINITY) ? 0.f : __expf(mw[x] - M);
      o += wt * fx[hh * OROW + d];
      L += wt * fx[16 * OROW + 16 + hh];
    }
    const int h = kvh * G + hh;
    if (nchunk == 1) {
      outbuf[(size_t)h * HD + d] = f2b(o / L);
    } else {
      float* wsrow = ws + ((size_t)h * nchunk + chunk) * (HD + 4);
      mq_ws_store(&wsrow[d], o);
      if (d == 0) {
        mq_ws_store(&wsrow[HD], M);
        mq_ws_store(&wsrow[HD + 1], L);
      }
    }
  }
  if (nchunk == 1) return;

  // ---- publish, then the last-arriving block of this kv head combines ----
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every wave drains
  __syncthreads();
  if (t == 0) {
    const u32 v = __hip_atomic_fetch_add(&cnt[kvh], 1u, __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_AGENT);
    const int last = v % (u32)nchunk == (u32)(nchunk - 1);
    // every block of this launch has arrived: leave the word at zero (the
    // modulo only matters after another kernel's launches on this word)
    if (last)
      __hip_atomic_store(&cnt[kvh], 0u, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
    elected = last;
  }
  __syncthreads();
  if (!elected) return;

  // Combine.  One acquire, then plain (16-B) loads of the partials.  Weights:
  // wave = head, lane = chunk, max and sum by xor butterflies (every lane gets
  // them, in a fixed order).  Outputs: a thread owns 4 dims of one head; its
  // nchunk 16-B loads are independent and issue 8 at a time.
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  float* cw = reinterpret_cast<float*>(smem);  // [16][64] chunk weights
  float* cL = cw + 16 * 64;                    // [16]
  const float* hbase = ws + (size_t)kvh * G * nchunk * (HD + 4);
  for (int hh = w; hh < G; hh += 4) {
    const float* row =
        hbase + ((size_t)hh * nchunk + min(lane, nchunk - 1)) * (HD + 4);
    const float mc = lane < nchunk ? row[HD] : -INFINITY;
    const float lc = lane < nchunk ? row[HD + 1] : 0.f;
    float M = mc;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
      M = fmaxf(M, __shfl_xor(M, off, WAVE));
    const float wt = (mc == -INFINITY) ? 0.f : __expf(mc - M);
    float L = lc * wt;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) L += __shfl_xor(L, off, WAVE);
    cw[hh * 64 + lane] = wt;
    if (lane == 0) cL[hh] = L;
  }
  __syncthreads();
  for (int idx = t; idx < G * (HD / 4); idx += 256) {
    const int hh = idx / (HD / 4), d = 4 * (idx % (HD / 4));
    const float* col = hbase + (size_t)hh * nchunk * (HD + 4) + d;
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
    for (int c = 0; c < nchunk; ++c) {
      const f32x4 v =
          *reinterpret_cast<const f32x4*>(col + (size_t)c * (HD + 4));
      const float wt = cw[hh * 64 + c];
#pragma unroll
      for (int j = 0; j < 4; ++j) o[j] += v[j] * wt;
    }
    const float L = cL[hh];
    union { u16 h[4]; unsigned long long u; } pk;
#pragma unroll
    for (int j = 0; j < 4; ++j) pk.h[j] = f2b(o[j] / L);
    *reinterpret_cast<unsigned long long*>(
        outbuf + (size_t)(kvh * G + hh) * HD + d) = pk.u;
  }
}

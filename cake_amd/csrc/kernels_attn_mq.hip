// Grouped MFMA decode attention for any GQA ratio 1 <= G <= 16, head dims
// 64 and 128 (opt-in: launch_attn_decode's mq argument / CAKE_ATTN_MQ /
// config key decode_attention "mfma").
//
// Why: k_attn_decode_g splits its 4 waves as GB heads x R residues, which
// only divides for GB in {1, 2, 4}; G = 3, 5, 6, 7 and every hd-64 model ran
// the per-head kernel, which reads each K/V row once per q head.  Here the G
// q rows of one kv head are padded to ONE 16-row MFMA operand, so G is no
// template parameter and K/V are read once per kv head.
//
// Split of the work.  Grid (nchunk, nkv), 4 waves.  A block serves all G
// heads of kv head blockIdx.y over chunk [start, end) (chunks partition
// [lo, n) exactly as in k_attn_decode_fused).  Wave w owns positions
// start + 32 w + 128 i .. + 32: every K and V element of the chunk is loaded
// and consumed by exactly one wave, each wave carries its own (m, l, O^T)
// for the 16 head rows, and the main loop has NO block barrier.  Steps begin
// at `start`, which need not be tile-aligned (rows are the load granule), so
// only the chunk's end is masked.
//
// Per 32-position step of a wave (v_mfma_f32_16x16x32_bf16 throughout):
//   scores   D[pos][head] = K (A: 16 positions x 32 dims, 16-B global loads
//            straight into the fragment) x Q^T (B: dims x 16 heads, persistent
//            registers; heads >= G are zero rows).  Lane % 16 = head, the 4
//            registers + lane / 16 = position, so a head's tile max and sum
//            are 8 registers plus two cross-lane steps (xor 16, xor 32).
//            Products of bf16 accumulate in f32: scores are as exact as in
//            the f32 kernels.  Masked positions are selected to -inf before
//            any max or exp; their P is exactly 0.
//   P.V      O^T[d][head] += V^T (A: 16 dims x 32 positions) x P (B).  The D
//            fragment of the scores already IS the B fragment of P under the
//            k-slot permutation slot 8 g + 4 t + r <-> position 16 t + 4 g + r
//            (t = 16-position half, g = lane / 16, r = register), so P never
//            moves between lanes.  P is split into bf16 hi + bf16 lo
//            (lo = bf16(p - hi), |p - hi - lo| <= 2^-17 p): two MFMAs per V
//            fragment keep P at f32-kernel accuracy.  O^T has head = lane % 16
//            like m and l, so the rescale by alpha is lane-local.
//   V^T      the wave stages its 32 V rows row-major in its own LDS slice
//            (16-B global loads -> 16-B LDS writes) and reads the fragments
//            with the LDS transpose load ds_read_b64_tr_b16: within 16 lanes,
//            lane L addresses 4 dims (4 (L % 4) .. + 3) of row L / 4 and lane i
//            receives dim i of those 4 rows.  With rows 16 t + 4 g + (L / 4)
//            that is exactly the permuted k-slot order above.  Rows are padded
//            to HD + 16 elements (stride 72 / 40 dwords) to spread the 16 rows
//            of one read over the banks.
//   loads    the next step's K and V loads are issued after the score MFMAs
//            have consumed the K registers and the LDS writes the V registers;
//            they are unguarded (clamped to end - 1, see k_attn_decode_fused)
//            and wait only at their first use.
// The 4 waves merge (m, l, O) once through LDS at the end of the chunk.
//
// Split-KV contract: that of launch_attn_decode.  ws[h][chunk] = {o[hd], m,
// l} at stride hd + 4, agent-scope relaxed stores + vmcnt(0) drain, then an
// arrival counter cnt[kvh] (nkv words); the LAST-arriving block of a kv head
// combines the partials of all G heads behind one agent-scope acquire.  No block ever waits
// on another.  The elected block stores 0 to its word, so between this
// kernel's own launches the word is 0 and the chunk count may change freely on
// one zeroing.  The election is still modulo nchunk: launch_attn_decode hands
// the same words to its other kernels, which leave them at multiples of the
// chunk count, and the engine re-zeroes them when that count changes.  An empty chunk publishes m = -inf, l = 0,
// o = 0 and weighs exactly 0.  nchunk == 1 writes the output directly, with
// no ws and no counter.
//
// Resource report (hipcc -O3, gfx950, -Rpass-analysis=kernel-resource-usage):
//   HD 128: 192 VGPRs + 32 AGPRs, 0 B scratch, LDS 36868 B, 2 waves/SIMD
//   HD 64:  108 VGPRs + 16 AGPRs, 0 B scratch, LDS 20484 B, 4 waves/SIMD
// Measurements: DESIGN section 4.
#include <cstdio>

#include "kernels.h"
#include "kernels_common.h"

namespace {

using bf16x2 = __attribute__((ext_vector_type(2))) __bf16;
using v4i16 = __attribute__((ext_vector_type(4))) short;
using lds_v4i16 = __attribute__((address_space(3))) v4i16*;

// x of lane ^ 32 (v_permlane32_swap, as halfswap32 in kernels_attn.hip)
__device__ inline float mq_swap32(float x, int lhalf) {
  union { float f; u32 u; } a{x};
  auto r = __builtin_amdgcn_permlane32_swap(a.u, a.u, false, false);
  a.u = lhalf == 0 ? (u32)r[1] : (u32)r[0];
  return a.f;
}
// two f32 -> packed bf16 pair, round to nearest even (v_cvt_pk_bf16_f32)
__device__ inline u32 mq_pack(float lo, float hi) {
  f32x2 v = {lo, hi};
  union { bf16x2 b; u32 u; } c{__builtin_convertvector(v, bf16x2)};
  return c.u;
}
// LDS traffic of one wave is in order; this only keeps the compiler from
// moving a lane's LDS reads across another lane's writes
__device__ inline void mq_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int HD>
__global__ __launch_bounds__(256) void k_attn_decode_mq(
    const u16* __restrict__ q, const u16* __restrict__ kc,
    const u16* __restrict__ vc, const int* __restrict__ pos,
    float* __restrict__ ws, u32* __restrict__ cnt, u16* __restrict__ outbuf,
    int nh, int nkv, int max_seq, int nchunk, int window) {
  constexpr int KK = HD / 32;         // score MFMAs per 16 positions
  constexpr int DB = HD / 16;         // 16-dim blocks of O^T
  constexpr int NV = HD / 16;         // 16-B V loads per lane per step
  constexpr int VROW = HD + 16;       // padded LDS row, elements
  constexpr int WSL = 32 * VROW * 2;  // LDS bytes per wave
  constexpr int OROW = HD + 1;        // merge image row, floats
  static_assert(16 * OROW * 4 + 128 <= WSL, "merge image fits the V slice");
  static_assert(4 * WSL >= (16 * 64 + 16) * 4, "combine staging fits");
  __shared__ __attribute__((aligned(16))) unsigned char smem[4 * WSL];
  __shared__ int elected;

  const int kvh = blockIdx.y, chunk = blockIdx.x;
  const int G = nh / nkv;
  const int n = *pos + 1;
  const int lo = (window > 0 && n > window) ? n - window : 0;
  const int cs = (n - lo + nchunk - 1) / nchunk;
  const int start = lo + chunk * cs;
  const int end = min(start + cs, n);
  const int t = threadIdx.x, w = t / WAVE, lane = t % WAVE;
  const int g = lane >> 4, c16 = lane & 15, lhalf = lane >> 5;
#define WS_STORE(p, v)                                                     \
  __hip_atomic_store((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)

  const u16* kbase = kc + (size_t)kvh * max_seq * HD;
  const u16* vbase = vc + (size_t)kvh * max_seq * HD;
  u16* vl = reinterpret_cast<u16*>(smem + w * WSL);
  const float scale = rsqrtf((float)HD);

  // Q^T fragments: lane holds head c16, dims kk * 32 + 8 g .. + 8
  bf16x8 qf[KK];
  {
    const u16* qrow = q + (size_t)(kvh * G + min(c16, G - 1)) * HD + 8 * g;
#pragma unroll
    for (int kk = 0; kk < KK; ++kk) {
      union { uint4v u; bf16x8 v; } c;
      c.u = *reinterpret_cast<const uint4v*>(qrow + kk * 32);
      if (c16 >= G) c.u = uint4v{0u, 0u, 0u, 0u};
      qf[kk] = c.v;
    }
  }

  f32x4 acc[DB];
#pragma unroll
  for (int db = 0; db < DB; ++db) acc[db] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;

  // unguarded loads, addresses clamped into [start, end - 1]
  bf16x8 kf[2][KK];
  uint4v vr[NV];
  auto load_kv = [&](int p0) {
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
      const int pc = min(p0 + 16 * tt + c16, end - 1);
      const u16* krow = kbase + (size_t)pc * HD + 8 * g;
#pragma unroll
      for (int kk = 0; kk < KK; ++kk)
        kf[tt][kk] = *reinterpret_cast<const bf16x8*>(krow + kk * 32);
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int e = i * 512 + lane * 8;
      const int pc = min(p0 + e / HD, end - 1);
      vr[i] = *reinterpret_cast<const uint4v*>(vbase + (size_t)pc * HD +
                                               e % HD);
    }
  };

  const int pw = start + 32 * w;      // this wave's first position
  if (pw < end) load_kv(pw);
  for (int p0 = pw; p0 < end; p0 += 128) {
    // ---- V rows -> this wave's LDS slice ---------------------------------
    mq_wave_sync();                   // the previous step's reads are issued
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int e = i * 512 + lane * 8;
      *reinterpret_cast<uint4v*>(vl + (e / HD) * VROW + e % HD) = vr[i];
    }
    mq_wave_sync();
    // ---- scores ------------------------------------------------------------
    float sc[2][4];
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
      f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < KK; ++kk)
        s = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[tt][kk], qf[kk], s, 0,
                                                    0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r)
        sc[tt][r] =
            (p0 + 16 * tt + 4 * g + r < end) ? s[r] * scale : -INFINITY;
    }
    // next step's loads (clamped; the last step reloads row end - 1)
    load_kv(p0 + 128);
    // ---- online softmax, per head = lane % 16 ------------------------------
    float tm = -INFINITY;
#pragma unroll
    for (int tt = 0; tt < 2; ++tt)
#pragma unroll
      for (int r = 0; r < 4; ++r) tm = fmaxf(tm, sc[tt][r]);
    tm = fmaxf(tm, __shfl_xor(tm, 16, WAVE));
    tm = fmaxf(tm, mq_swap32(tm, lhalf));
    const float mnew = fmaxf(m, tm);
    const float alpha = (mnew == -INFINITY) ? 0.f : __expf(m - mnew);
    float tsum = 0.f;
    union { u32 u[4]; bf16x8 v; } phi, plo;
#pragma unroll
    for (int tt = 0; tt < 2; ++tt) {
      float p[4], d[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        p[r] = (sc[tt][r] == -INFINITY) ? 0.f : __expf(sc[tt][r] - mnew);
        tsum += p[r];
      }
      phi.u[2 * tt] = mq_pack(p[0], p[1]);
      phi.u[2 * tt + 1] = mq_pack(p[2], p[3]);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const u32 h = phi.u[2 * tt + (r >> 1)];
        union { u32 u; float f; } hv{(r & 1) ? (h & 0xffff0000u) : (h << 16)};
        d[r] = p[r] - hv.f;
      }
      plo.u[2 * tt] = mq_pack(d[0], d[1]);
      plo.u[2 * tt + 1] = mq_pack(d[2], d[3]);
    }
    tsum += __shfl_xor(tsum, 16, WAVE);
    tsum += mq_swap32(tsum, lhalf);
    l = l * alpha + tsum;
    m = mnew;
    // ---- P.V: O^T[d][head] += V^T x (P hi + P lo) --------------------------
    const u16* vrd = vl + (4 * g + (c16 >> 2)) * VROW + 4 * (c16 & 3);
#pragma unroll
    for (int db = 0; db < DB; ++db) {
      union { v4i16 h[2]; bf16x8 v; } vf;
      vf.h[0] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
          (lds_v4i16)(vrd + db * 16));
      vf.h[1] = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
          (lds_v4i16)(vrd + 16 * VROW + db * 16));
      f32x4 a = acc[db];
#pragma unroll
      for (int r = 0; r < 4; ++r) a[r] *= alpha;
      a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf.v, phi.v, a, 0, 0, 0);
      a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf.v, plo.v, a, 0, 0, 0);
      acc[db] = a;
    }
  }

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
      WS_STORE(&wsrow[d], o);
      if (d == 0) {
        WS_STORE(&wsrow[HD], M);
        WS_STORE(&wsrow[HD + 1], L);
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
#undef WS_STORE
}

}  // namespace

bool attn_decode_mq_on(int nh, int nkv, int hd, int mq) {
  if (mq < 0) {
    const char* e = getenv("CAKE_ATTN_MQ");
    mq = e ? atoi(e) : 0;
  }
  if (mq <= 0) return false;
  return (hd == 64 || hd == 128) && nh > 0 && nkv > 0 && nh % nkv == 0 &&
         nh / nkv <= 16;
}

void launch_attn_decode_mq(const u16* q, const u16* kc, const u16* vc,
                           const int* pos, float* ws, u32* cnt, u16* out,
                           int nh, int nkv, int hd, int max_seq, int nchunk,
                           int window, hipStream_t s) {
  // the combine keeps one weight per (head, chunk) in a [16][64] LDS table
  if (nchunk < 1 || nchunk > 64 || !attn_decode_mq_on(nh, nkv, hd, 1)) {
    fprintf(stderr, "launch_attn_decode_mq: nchunk %d outside [1,64] or shape "
            "(nh %d, nkv %d, hd %d) not served; nothing launched\n", nchunk,
            nh, nkv, hd);
    return;
  }
  if (hd == 128)
    hipLaunchKernelGGL(k_attn_decode_mq<128>, dim3(nchunk, nkv), dim3(256), 0,
                       s, q, kc, vc, pos, ws, cnt, out, nh, nkv, max_seq,
                       nchunk, window);
  else
    hipLaunchKernelGGL(k_attn_decode_mq<64>, dim3(nchunk, nkv), dim3(256), 0,
                       s, q, kc, vc, pos, ws, cnt, out, nh, nkv, max_seq,
                       nchunk, window);
}
